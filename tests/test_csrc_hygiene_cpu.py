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


# Where an option or an environment switch has to be used to stay: a test, a tool, the Julia glue, the benchmark, the driver
# entry or the Python package.  (Documents do not count: they describe, they do not run.)
USER_DIRS = ("tests", "tools", "julia")
USER_FILES = ("bench.py", "__graft_entry__.py")
ENV_READ_PY = re.compile(r"""os\.(?:environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]|getenv\s*\()\s*["'](MNK_\w+)["']""")
ALLOWED_WITHOUT_USER = {
    # a numeric tolerance of the public interface (the growth bound of quasi-definite pivot sequences): callers
    # set it, nothing in this tree needs another value than the default
    "bk_growth_tol_qd",
    # selects the operands inside the two bulk kernels: taking it out rewrites their register allocation, which needs an A/B
    # run on the device and is a change of its own
    "MNK_DAG_FAKE_SHARE",
}


def _option_keys():
    with open(os.path.join(L.CSRC, "ls.hip")) as f:
        src = f.read()
    body = src[src.index("int mnk_ls_set_option("):]
    body = body[:body.index("unknown option")]
    return sorted(set(re.findall(r'strcmp\(key, "([a-z0-9_]+)"\)', body)))


def _env_names():
    """(MNK_* names that csrc/ reads with getenv( and the package with os.environ, the package's texts without those reads)."""
    names = set()
    for name in sorted(os.listdir(L.CSRC)):
        with open(os.path.join(L.CSRC, name)) as f:
            names.update(re.findall(r'getenv\(\s*"(MNK_\w+)"', f.read()))
    pkg = os.path.dirname(L.CSRC)
    texts = []
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                text = f.read()
            names.update(ENV_READ_PY.findall(text))
            texts.append(ENV_READ_PY.sub("", text))   # (the read of a switch is not its user)
    return sorted(names), texts


def test_every_option_and_switch_has_a_user():
    """A key of mnk_ls_set_option, or an MNK_* environment name read in csrc/ or the package, that no test, tool, Julia glue,
    bench.py, __graft_entry__.py or package module names as a whole word selects a path nothing runs: its losing branches are
    untested surface of the schedules.  Such a key becomes the value it is set to (A/B runs compare two commits)."""
    root = os.path.dirname(os.path.dirname(L.CSRC))
    keys = _option_keys()
    envs, texts = _env_names()
    assert len(keys) > 30 and "pivot_tol" in keys and "MNK_OPTIONS" in envs   # (the parsers still find what they look for)
    for d in USER_DIRS:
        for dirpath, _, files in os.walk(os.path.join(root, d)):
            for name in files:
                if os.path.join(dirpath, name) == os.path.abspath(__file__):   # (naming a key here is not using it)
                    continue
                try:
                    with open(os.path.join(dirpath, name)) as f:
                        texts.append(f.read())
                except UnicodeDecodeError:   # (a binary fixture names nothing)
                    pass
    for name in USER_FILES:
        with open(os.path.join(root, name)) as f:
            texts.append(f.read())
    unused = [n for n in keys + envs
              if n not in ALLOWED_WITHOUT_USER and not any(re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % n, t) for t in texts)]
    assert not unused, f"options / environment switches that nothing uses: {unused}"
    stale = sorted(n for n in ALLOWED_WITHOUT_USER if n not in keys + envs)
    assert not stale, f"allow-list entries that no longer exist: {stale}"
