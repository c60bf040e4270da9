#!/usr/bin/env python
"""Compare the device code of two builds kernel by kernel.

  tools/device_code_diff.py <dir A> <dir B>     two output directories of tools/build_units_temps.sh (one subdirectory per unit)
  tools/device_code_diff.py <a.out> <b.out>     two *-hip-amdgcn-amd-amdhsa-gfx950.out code objects

Each code object is disassembled (llvm-objdump -d --no-show-raw-insn --no-leading-addr) and split by symbol; a unit passes when both
sides have the same symbols with identical text.  The text of a kernel that addresses a global of its unit holds its distance to it, so
the comparison also holds the kernels to their order in the code object.  Prints one line per unit and exits 1 on any difference."""
import glob
import os
import re
import subprocess
import sys

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
LABEL = re.compile(r"^<?([^\s<>:]+)>?:\s*$")


def symbols(path):
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = LABEL.match(line)
        if m and not line.startswith((" ", "\t")):
            name = m.group(1)
            out[name] = []
        elif name is not None:
            out[name].append(line.split("//")[0].strip())  # (the trailing comment is address and encoding: it moves with the kernel)
    return out


def compare(a, b):
    sa, sb = symbols(a), symbols(b)
    only = sorted(set(sa) ^ set(sb))
    diff = sorted(k for k in set(sa) & set(sb) if sa[k] != sb[k])
    return len(sa), only, diff


def code_object(unit_dir):
    found = glob.glob(os.path.join(unit_dir, "*-hip-amdgcn-amd-amdhsa-gfx950.out"))
    assert len(found) == 1, (unit_dir, found)
    return found[0]


def main():
    a, b = sys.argv[1:3]
    pairs = [("", a, b)] if os.path.isfile(a) else [
        (u, code_object(os.path.join(a, u)), code_object(os.path.join(b, u)))
        for u in sorted(os.listdir(a)) if os.path.isdir(os.path.join(a, u))]
    bad = 0
    for unit, fa, fb in pairs:
        n, only, diff = compare(fa, fb)
        print(f"{unit or os.path.basename(fa):24s} symbols {n:4d}  on one side only {len(only):3d}  differing {len(diff):3d}")
        for k in only + diff:
            print("   ", k)
        bad += len(only) + len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
