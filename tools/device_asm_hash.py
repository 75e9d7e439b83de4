#!/usr/bin/env python3
"""sha256 of the gfx950 device assembly of every product source (no GPU needed, no device opened).

    python tools/device_asm_hash.py [--root DIR] [--per-kernel]

Compiles each entry of `_lib.SOURCES` of the tree at DIR (default: this checkout) with the flags `build()` uses
(`_lib.FILE_FLAGS` included) plus `--cuda-device-only -S` into a temporary directory and prints `sha256  source` per file,
then the compiler's `.ident` line.  Two trees whose columns agree (same ident) run the same device code: that is how a
refactor of csrc/ shows that it changed no kernel (record: profiles/lab_removal_device_asm.txt).  SOURCES and FILE_FLAGS
are read from the tree that is hashed, so a parent checkout is compiled the way the parent builds.

One symbol is neutralised before hashing: hipcc names a per-translation-unit marker `__hip_cuid_<hash>` after a hash of the
source's PATH and the command line, so the raw text of two checkouts in different directories never agrees although the
code does.  Nothing else in the assembly depends on where the tree lies.

`--per-kernel` prints `sha256  source  kernel` for every kernel symbol instead (sorted by demangled name within a source): the hash
of the kernel's function body, from its label to its end label, which includes its `.amdhsa_kernel` block.  A change that removes
a kernel from a source renumbers the functions behind it, and with them the function index inside their local labels
(`.LBB<n>_<block>`, `.Lfunc_end<n>`, `.LJTI<n>_<table>`) and the counter of `.Ltmp<n>`; these numbers are neutralised too, and the
compiler's comments (which repeat them: `; in Loop: Header=BB<n>_<block>`, padded to a column) are left out, so a kernel that was
not touched keeps its hash (record: profiles/option_removal_device_asm.txt)."""
import argparse
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_lib_module(root):
    """`madnlp.jl_amd/_lib.py` of `root` as a module (its import loads no shared object and opens no device)."""
    path = os.path.join(root, "madnlp.jl_amd", "_lib.py")
    spec = importlib.util.spec_from_file_location("_mnk_lib_for_hash", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_bodies(asm):
    """{kernel symbol: its text from the label line to `.Lfunc_end<n>:`, without comments, function numbers neutralised} of one
    assembly file."""
    text = asm.decode(errors="replace")
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M):
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.M | re.S)
        if m is None:
            raise RuntimeError(f"no function body for kernel {name}")
        body = "\n".join(ln.split(";", 1)[0].rstrip() for ln in m.group(0).splitlines())
        body = re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", body)
        out[name] = re.sub(r"\.(Lfunc_end|Ltmp)\d+", r".\1", body)
    return out


def demangle(names):
    """Readable names through llvm-cxxfilt / c++filt, or the mangled ones if neither is installed."""
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or filt is None:
        return list(names)
    res = subprocess.run([filt] + list(names), capture_output=True, text=True)
    lines = res.stdout.splitlines()
    return lines if res.returncode == 0 and len(lines) == len(names) else list(names)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--per-kernel", action="store_true", help="one hash per kernel symbol instead of one per source")
    args = ap.parse_args()
    L = load_lib_module(os.path.abspath(args.root))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]

    with tempfile.TemporaryDirectory() as tmp:
        def asm_of(src):
            out = os.path.join(tmp, src.replace(".hip", ".s"))
            cmd = base + L.FILE_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(L.CSRC, src), "-o", out]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}:\n{res.stdout}{res.stderr}")
            with open(out, "rb") as f:
                return re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_", f.read())

        with ThreadPoolExecutor(max_workers=min(8, len(L.SOURCES))) as ex:
            asms = list(ex.map(asm_of, L.SOURCES))
    idents = set()
    for src, asm in zip(L.SOURCES, asms):
        if args.per_kernel:
            bodies = kernel_bodies(asm)
            names = list(bodies)
            for shown, name in sorted(zip(demangle(names), names)):
                print(f"{hashlib.sha256(bodies[name].encode()).hexdigest()}  {src}  {shown}")
        else:
            print(f"{hashlib.sha256(asm).hexdigest()}  {src}")
        idents.update(ln.strip() for ln in asm.decode(errors="replace").splitlines() if ln.lstrip().startswith(".ident"))
    for ident in sorted(idents):
        print(ident)
    return 0


if __name__ == "__main__":
    sys.exit(main())
