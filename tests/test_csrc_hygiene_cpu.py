"""The library's source directory holds what the shipped build compiles and nothing else (no GPU, no compile): no
preprocessor conditional -- one build, no `-D` variants --, no file that `build()` does not know, and no header that no
product source includes.  Laboratory code lives under tools/hip/ (tools/README.md)."""
import os
import re

from madnlp_jl_amd import _lib as L

CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b")
INCLUDE = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)


def _csrc_headers():
    """HEADERS without the public header under include/ (the one entry that lies outside csrc/)."""
    return [h for h in L.HEADERS if os.path.dirname(h) == ""]


def test_csrc_has_no_preprocessor_conditionals():
    found = []
    for name in sorted(os.listdir(L.CSRC)):
        with open(os.path.join(L.CSRC, name)) as f:
            found += [f"{name}:{i}: {ln.strip()}" for i, ln in enumerate(f, 1) if CONDITIONAL.match(ln)]
    assert not found, "compile-time switches belong to history, A/B runs compare two commits:\n" + "\n".join(found)


def test_csrc_files_are_exactly_the_sources_and_headers_of_the_build():
    outside = [h for h in L.HEADERS if os.path.dirname(h) != ""]
    assert [os.path.normpath(os.path.join(L.CSRC, h)) for h in outside] == \
        [os.path.normpath(os.path.join(L.CSRC, "..", "..", "include", "madnlp_hip.h"))]
    listed = L.SOURCES + _csrc_headers()
    assert len(set(listed)) == len(listed)
    assert sorted(os.listdir(L.CSRC)) == sorted(listed)
    for h in outside:
        assert os.path.isfile(os.path.join(L.CSRC, h))


def test_every_header_is_included_by_a_product_file():
    included = set()
    for name in L.SOURCES + _csrc_headers():
        with open(os.path.join(L.CSRC, name)) as f:
            included.update(os.path.basename(inc) for inc in INCLUDE.findall(f.read()))
    unused = [h for h in L.HEADERS if os.path.basename(h) not in included]
    assert not unused, f"headers in _lib.HEADERS that no file of csrc/ includes: {unused}"
