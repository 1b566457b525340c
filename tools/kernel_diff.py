#!/usr/bin/env python3
"""kernel_diff.py OLD NEW — do two builds hold the same gfx950 device code?

Each argument is a libwhisper_hip.so, an object file or an extracted code object.  Every gfx950 code object of an input is
extracted (llvm-objdump --offloading; the library holds one bundle per source), and for every kernel — a FUNC symbol with a
`.kd` companion — the function's bytes (by symbol value and size) and its 64-byte kernel descriptor are read.  Kernels are
matched across the two inputs by mangled name, whatever code object they sit in, so a kernel that moved to another source
file is compared with itself.

Bytes only: nothing is disassembled and no instruction is searched for.  One field of the descriptor is position, not
content: kernel_code_entry_byte_offset (bytes 16..23), the distance from the descriptor to the code, which changes whenever
another kernel of the same code object grows, shrinks, comes or goes.  It is compared as the distance from the function's
own symbol to the entry point (0 wherever the entry is the function's first byte).

Prints the counts of identical, differing, only-in-OLD and only-in-NEW kernels and every name that is not identical; the
exit status is 0 only when every kernel is identical.  Needs llvm-objdump and llvm-readelf (LLVM_BIN, default
/opt/rocm/llvm/bin) and no GPU.
"""
from __future__ import annotations

import glob
import os
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
EM_AMDGPU = 224


def code_objects(path: str, tmp: str) -> list:
    """The gfx950 code objects of `path`: the file itself if it is one, else what its offload bundles hold."""
    with open(path, "rb") as f:
        head = f.read(20)
    if head[:4] == b"\x7fELF" and struct.unpack_from("<H", head, 18)[0] == EM_AMDGPU:
        return [path]
    work = tempfile.mkdtemp(dir=tmp)   # llvm-objdump writes the bundles' entries beside its input
    copy = os.path.join(work, "in")
    shutil.copy(path, copy)
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", copy], check=True, stdout=subprocess.DEVNULL)
    return sorted(glob.glob(copy + ".*amdgcn-amd-amdhsa--gfx950"))


def kernels_of(co: str) -> dict:
    """{mangled name: (function bytes, descriptor with the entry offset taken from the function's symbol)} of one code object."""
    out = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--wide", "--section-headers", "--symbols", co],
                         check=True, capture_output=True, text=True).stdout
    sections, syms = {}, {}   # index -> (addr, file offset); name -> (value, size, type, section index)
    for line in out.splitlines():
        line = line.strip()
        if line.startswith("["):   # [Nr] Name Type Address Off Size ...   (the unnamed null section has one column less)
            f = line.replace("[", " ").replace("]", " ").split()
            if f[0].isdigit() and len(f) >= 6 and f[1] != "NULL":
                sections[int(f[0])] = (int(f[3], 16), int(f[4], 16))
        else:                      # Num: Value Size Type Bind Vis Ndx Name
            f = line.split()
            if len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit() and f[6].isdigit():
                syms[f[7]] = (int(f[1], 16), int(f[2]), f[3], int(f[6]))
    with open(co, "rb") as fh:
        blob = fh.read()

    def data(sym):
        addr, off = sections[sym[3]]
        return blob[sym[0] - addr + off: sym[0] - addr + off + sym[1]]

    found = {}
    for name, s in syms.items():
        kd = syms.get(name + ".kd")
        if s[2] != "FUNC" or kd is None:
            continue
        desc = bytearray(data(kd))
        if len(desc) != 64:
            raise SystemExit(f"{co}: descriptor of {name} has {len(desc)} bytes, not 64")
        entry = kd[0] + struct.unpack_from("<q", desc, 16)[0]
        struct.pack_into("<q", desc, 16, entry - s[0])
        found[name] = (data(s), bytes(desc))
    return found


def kernels(path: str, tmp: str) -> dict:
    allk = {}
    cos = code_objects(path, tmp)
    if not cos:
        raise SystemExit(f"{path}: no gfx950 code object")
    for co in cos:
        for name, k in kernels_of(co).items():
            if name in allk and allk[name] != k:
                raise SystemExit(f"{path}: kernel {name} sits in two code objects with different code")
            allk[name] = k
    return allk


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__.splitlines()[0], file=sys.stderr)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(argv[1], tmp), kernels(argv[2], tmp)
    both = sorted(set(old) & set(new))
    differing = [n for n in both if old[n] != new[n]]
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print(f"kernels: {len(old)} in OLD, {len(new)} in NEW")
    print(f"identical: {len(both) - len(differing)}  differing: {len(differing)}  only in OLD: {len(only_old)}  only in NEW: {len(only_new)}")
    for n in differing:
        what = " and ".join(w for w, i in (("code", 0), ("descriptor", 1)) if old[n][i] != new[n][i])
        print(f"differs ({what}): {n}")
    for n in only_old:
        print(f"only in OLD: {n}")
    for n in only_new:
        print(f"only in NEW: {n}")
    if differing or only_old or only_new:
        return 1
    print("all identical")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
