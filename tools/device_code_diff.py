#!/usr/bin/env python
"""Compare the device code of two builds kernel by kernel.

  tools/device_code_diff.py <dir A> <dir B>     two output directories of tools/build_units_temps.sh (one subdirectory per unit)
  tools/device_code_diff.py <a.out> <b.out>     two *-hip-amdgcn-amd-amdhsa-gfx950.out code objects

Each code object is disassembled (llvm-objdump -d --no-show-raw-insn --no-leading-addr) and split by symbol; a unit passes when both
sides have the same symbols with identical text.  The text of a kernel that addresses a global of its unit holds its distance to it, so
the comparison also holds the kernels to their order in the code object.  Prints one line per unit and exits 1 on any difference.
Where a unit or a symbol exists on one side only (a kernel moved to another unit, a unit removed), a closing section looks every such
symbol up in all units of the other side and says whether its text is identical there; one without a counterpart anywhere is listed and
counts as a difference.

For a kernel that differs it then says how (directories only; the resources come from the .amdgpu_metadata of the unit's *.s):
  "distances"   nothing but the literals of s_getpc_b64 / s_add_u32 pairs, the distances to globals of the unit
  "reordered"   equal SGPRs, VGPRs, scratch and static LDS, an equal multiset of vector floating-point opcodes (v_*_f64, v_rcp*, v_exp*,
                v_sqrt*, v_fma*), equal counts of ds_*, global_* and buffer_* instructions, instruction counts within 1 %: what remains
                is instruction order, registers, scalar code and waits
  "CHANGED"     anything else
with the instruction count and (SGPRs, VGPRs, scratch, LDS) of both sides."""
import collections
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


def resources(code_obj):
    """kernel -> (SGPRs, VGPRs, scratch bytes, static LDS bytes), from the metadata of the assembly next to the code object"""
    text = open(code_obj[:-len(".out")] + ".s").read()
    out = {}
    for entry in text.split("  - .agpr_count:")[1:]:
        f = {k: v for k, v in re.findall(r"^    \.(\w+):\s+(\S+)$", entry, re.M)}
        out[f["name"]] = tuple(int(f[k]) for k in ("sgpr_count", "vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    return out


FP = re.compile(r"v_\w+_f64|v_rcp|v_exp|v_sqrt|v_fma")
MEM = re.compile(r"(ds|global|buffer)_")


def profile(lines):
    ops = [ln.split()[0] for ln in lines if ln]
    return len(ops), collections.Counter(o for o in ops if FP.match(o)), collections.Counter(MEM.match(o).group(1) for o in ops if MEM.match(o))


def verdict(la, lb, ra, rb):
    """how two texts of one kernel differ (module docstring)"""
    if len(la) == len(lb) and all(x == y or (x.startswith("s_add_u32") and x.split()[:3] == y.split()[:3] and i and la[i - 1].startswith("s_getpc_b64"))
                                  for i, (x, y) in enumerate(zip(la, lb))):
        return "distances"
    (na, fa, ma), (nb, fb, mb) = profile(la), profile(lb)
    ok = ra == rb and fa == fb and ma == mb and abs(nb - na) <= 0.01 * na
    return f"{'reordered' if ok else 'CHANGED'}  instructions {na} -> {nb}  (sgpr, vgpr, scratch, lds) {ra} -> {rb}"


def compare(a, b, explain=False):
    sa, sb = symbols(a), symbols(b)
    only = sorted(set(sa) ^ set(sb))
    diff = sorted(k for k in set(sa) & set(sb) if sa[k] != sb[k])
    if explain and diff:
        ra, rb = resources(a), resources(b)
        diff = [f"{k}  {verdict(sa[k], sb[k], ra.get(k), rb.get(k))}" for k in diff]
    return len(sa), only, diff


def code_object(unit_dir):
    found = glob.glob(os.path.join(unit_dir, "*-hip-amdgcn-amd-amdhsa-gfx950.out"))
    assert len(found) == 1, (unit_dir, found)
    return found[0]


def units(d):
    return {u for u in os.listdir(d) if os.path.isdir(os.path.join(d, u))}


def moved(a, b):
    """Directories whose unit lists differ: the symbols of the units on one side only, and of their namesakes' one-sided symbols, looked
    up in ALL units of the other side.  -> lines, the number of symbols that differ or have no counterpart anywhere"""
    pool = [{k: (u, v) for u in sorted(units(d)) for k, v in symbols(code_object(os.path.join(d, u))).items()} for d in (a, b)]
    lines, bad = [], 0
    for k in sorted(set(pool[0]) | set(pool[1])):
        (ua, ta), (ub, tb) = pool[0].get(k, (None, None)), pool[1].get(k, (None, None))
        if ua == ub:
            continue  # (same unit: the per-unit lines above)
        if ua is None or ub is None:
            lines.append(f"    {k}  in {ua or ub} on the {'first' if ub is None else 'second'} side only")
        else:
            lines.append(f"    {k}  {ua} -> {ub}  {'identical' if ta == tb else 'DIFFERS'}")
        bad += ua is None or ub is None or ta != tb
    return lines, bad


def main():
    a, b = sys.argv[1:3]
    both = [] if os.path.isfile(a) else sorted(units(a) & units(b))
    pairs = [("", a, b)] if os.path.isfile(a) else [(u, code_object(os.path.join(a, u)), code_object(os.path.join(b, u))) for u in both]
    bad = 0
    shuffled = bool(both) and units(a) != units(b)
    for unit, fa, fb in pairs:
        n, only, diff = compare(fa, fb, explain=bool(unit))
        print(f"{unit or os.path.basename(fa):24s} symbols {n:4d}  on one side only {len(only):3d}  differing {len(diff):3d}")
        for k in only + diff:
            print("   ", k)
        shuffled = shuffled or (bool(unit) and bool(only))
        bad += len(diff) + (0 if unit else len(only))
    if shuffled:  # a unit or a symbol on one side only: it may have moved to another unit
        lines, n = moved(a, b)
        print(f"symbols whose unit differs {len(lines):3d}  of them differing or without a counterpart {n:3d}")
        print("\n".join(lines))
        bad += n
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
