#!/usr/bin/env python3
"""VGPR / spill / scratch / occupancy of every kernel in the built objects (build/*.o), from the code-object metadata.

    python tools/kernel_resources.py [substring]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "rustcrypto-elliptic-curves_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_object(obj, td):
    """the gfx950 code object bundled into a host object file, unbundled into the directory td; None if the object has none"""
    co, fat = os.path.join(td, "dev.co"), os.path.join(td, "fat.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], capture_output=True, text=True)
    return co if r.returncode == 0 and os.path.exists(co) else None


def demangle(symbol):
    return re.sub(r"\(.*", "", subprocess.run(["c++filt", symbol], capture_output=True, text=True).stdout.strip())


def kernel_metadata(co):
    """[(symbol, the FIELDS of its metadata)] for every kernel of a code object"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    rows = []
    for blk in notes.split("- .agpr_count:")[1:]:
        def g(key):
            m = re.search(r"\.%s:\s*(\S+)" % key, blk)
            return m.group(1) if m else "?"
        rows.append((g("name"), tuple(g(f) for f in FIELDS)))
    return rows


def objects(build):
    return sorted(fn for fn in os.listdir(build) if fn.endswith(".o"))


def main():
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    rows = []
    for fn in objects(BUILD):
        with tempfile.TemporaryDirectory() as td:
            co = code_object(os.path.join(BUILD, fn), td)
            if co is None:
                continue
            meta = kernel_metadata(co)
        for symbol, fields in meta:
            name = demangle(symbol)
            if pat in name:
                rows.append((fn, name) + fields)
    print("%-12s %-90s %5s %6s %5s %8s %7s" % ("object", "kernel", "vgpr", "spill", "sgpr", "scratchB", "ldsB"))
    for r in rows:
        print("%-12s %-90s %5s %6s %5s %8s %7s" % r)


if __name__ == "__main__":
    main()
