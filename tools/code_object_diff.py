#!/usr/bin/env python3
"""Compare two unbundled gfx950 code objects symbol by symbol:  code_object_diff.py OLD.co NEW.co

A code object is what `hipcc <the Makefile's FLAGS> --cuda-device-only --no-gpu-bundle-output -c X.hip -o X.co` writes.  For every FUNC
and OBJECT symbol the bytes it covers in the file are compared, so a kernel may move inside .text without counting as changed.  In a
kernel descriptor (`*.kd`, 64 bytes) bytes 16-23 hold the offset from the descriptor to the kernel's first byte, which depends only on
where the two landed: they are zeroed on both sides first.  `__hip_cuid_*` (a per-compilation id) is ignored.  A symbol without bytes in
the file (NOBITS, or a processor-specific section index) is compared by size.  Prints the one-sided and the differing symbols and
exits 1 if there is either; the script reads bytes and sizes only and knows nothing about what they encode.

Needs llvm-readelf: $LLVM_READELF, else $ROCM_PATH/llvm/bin (ROCM_PATH defaults to /opt/rocm), else the PATH."""
import os
import shutil
import subprocess
import sys


def readelf():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.environ.get("LLVM_READELF"), os.path.join(rocm, "llvm", "bin", "llvm-readelf"),
                 os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf")):
        if cand and os.path.exists(cand):
            return cand
    sys.exit("code_object_diff: llvm-readelf not found (set LLVM_READELF)")


def symbols(path):
    """name -> (type, size, bytes or None) for the FUNC and OBJECT symbols of .symtab (.dynsym repeats a subset of them)"""
    text = subprocess.run([readelf(), "-W", "--section-headers", "--symbols", path], check=True, capture_output=True, text=True).stdout
    blob = open(path, "rb").read()
    sections = {}                                     # index -> (type, address, file offset, size)
    out = {}
    table = None
    for line in text.splitlines():
        if line.startswith("Symbol table"):
            table = line.split("'")[1]
            continue
        f = line.split()
        if table is None and line.lstrip().startswith("["):
            f = line.replace("[", " ").replace("]", " ").split()       # "[ 7] .text PROGBITS addr off size ..."
            if len(f) >= 6 and f[0].isdigit() and f[0] != "0":
                sections[int(f[0])] = (f[2], int(f[3], 16), int(f[4], 16), int(f[5], 16))
            continue
        if table != ".symtab" or len(f) < 8 or not f[0].endswith(":") or f[3] not in ("FUNC", "OBJECT"):
            continue
        value, size, kind, ndx, name = int(f[1], 16), int(f[2]), f[3], f[6], f[7]
        if name.startswith("__hip_cuid_"):
            continue
        data = None
        if ndx.isdigit() and int(ndx) not in sections:
            sys.exit(f"code_object_diff: {path}: {name} is in section {ndx}, which the section-header listing of llvm-readelf did not show")
        if ndx.isdigit() and sections[int(ndx)][0] != "NOBITS":
            _, addr, off, sec_size = sections[int(ndx)]
            if not (addr <= value and value + size <= addr + sec_size):
                sys.exit(f"code_object_diff: {path}: {name} lies outside its section {ndx}")
            data = bytearray(blob[off + value - addr:off + value - addr + size])
            if name.endswith(".kd") and size >= 24:
                data[16:24] = bytes(8)
        if name in out:
            sys.exit(f"code_object_diff: {path}: {name} is defined twice")
        out[name] = (kind, size, None if data is None else bytes(data))
    return out


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = symbols(argv[1]), symbols(argv[2])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    kernels = sum(1 for n in new if n.endswith(".kd"))
    funcs = sum(1 for v in new.values() if v[0] == "FUNC")
    print(f"old: {len(old)} symbols, new: {len(new)} symbols ({kernels} kernel descriptors, {funcs} FUNC, {len(new) - funcs} OBJECT)")
    print(f"identical: {len(set(old) & set(new)) - len(differ)}, differing: {len(differ)}, only in old: {len(only_old)}, "
          f"only in new: {len(only_new)}")
    for title, names in (("only in old", only_old), ("only in new", only_new)):
        for n in names:
            print(f"{title}: {n}")
    for n in differ:
        (ko, so, bo), (kn, sn, bn) = old[n], new[n]
        what = f"type {ko} -> {kn}" if ko != kn else f"size {so} -> {sn}" if so != sn else \
            "bytes in the file on one side only" if bo is None or bn is None else \
            f"first differing byte at +{next(i for i in range(so) if bo[i] != bn[i])}"
        print(f"differs: {n} ({what})")
    return 1 if (only_old or only_new or differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
