#!/usr/bin/env python3
"""Hashes of the device code of ksql_amd/csrc, to show that a host-side refactor left it alone.

    python tools/kernel_hashes.py <tree> [--files=a.hip,b.hip] [-DKHIP_TUNING] > hashes.txt

<tree> is a checkout of this repository.  Every .hip file is compiled for gfx950 with the Makefile's
flags (device side only).  Per file: the sha256 of its device assembly without the `.file`, `.ident`
and `__hip_cuid_` lines, which name the file and the build.  Per kernel: the sha256 of its function's
bytes in .text and of its 64-byte kernel descriptor (<name>.kd), so that kernels which moved to
another file can be compared by name.  The bytes are read from the relocatable object the assembler
makes of that assembly, before the link: there the distances that depend on where the linker puts a
kernel (descriptor to code, code to a __constant__ variable) are relocations, not bytes.
Lines: `asm <file> <hash>` and `kernel <name> <text hash> <kd hash> <text bytes>`; the kernel lines
are sorted by name and carry no file, so two trees with the same kernels in different files print
the same kernel lines.  --files: kernel lines only for the kernels of these files (the ones a change
moved code between); the asm lines cover every file."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READELF = os.environ.get("READELF", "/opt/rocm/llvm/bin/llvm-readelf")
LLVM_MC = os.environ.get("LLVM_MC", "/opt/rocm/llvm/bin/llvm-mc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-x", "hip", "--cuda-device-only"]


def sha(b):
    return hashlib.sha256(b).hexdigest()[:16]


def kernels(co):
    """{kernel: (text bytes, descriptor bytes)} of a relocatable device object."""
    secs = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)",
                         subprocess.check_output([READELF, "-S", "--wide", co], text=True), re.M):
        secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))  # address, file offset
    syms = {}
    for line in subprocess.check_output([READELF, "-s", "--wide", co], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[0].endswith(":") and f[6].isdigit():
            syms[f[7]] = (int(f[1], 16), int(f[2]), int(f[6]))  # value, size, section
    blob = open(co, "rb").read()

    def read(name):
        value, size, sec = syms[name]
        addr, off = secs[sec]
        return blob[off + value - addr: off + value - addr + size]

    return {n[:-3]: (read(n[:-3]), read(n)) for n in syms if n.endswith(".kd")}


def main():
    tree, extra = sys.argv[1], [a for a in sys.argv[2:] if not a.startswith("--files=")]
    only = [f for a in sys.argv[2:] if a.startswith("--files=") for f in a[8:].split(",")]
    src = os.path.join(tree, "ksql_amd", "csrc")
    kern = {}
    with tempfile.TemporaryDirectory() as tmp:
        for path in sorted(glob.glob(os.path.join(src, "*.hip"))):
            name = os.path.basename(path)
            asm, co = os.path.join(tmp, name + ".s"), os.path.join(tmp, name + ".co")
            subprocess.check_call([HIPCC] + FLAGS + extra + ["-S", path, "-o", asm])
            text = "".join(l for l in open(asm) if not re.search(r"^\s*\.(file|ident)\b|__hip_cuid_", l))
            print("asm", name, sha(text.encode()))
            if only and name not in only:
                continue
            subprocess.check_call([LLVM_MC, "-triple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-filetype=obj", asm, "-o", co])
            for k, (t, d) in kernels(co).items():  # (a template from a header may be in several files)
                kern.setdefault(k, []).append((sha(t), sha(d), len(t)))
    for k in sorted(kern):
        for h in sorted(kern[k]):
            print("kernel", k, *h)


if __name__ == "__main__":
    main()
