#!/usr/bin/env python
"""Writes tests/golden/launch_reports.json: the report of crt_hip_last_kernel() for every case of tests/test_gpu_launch_reports.py.

Run it on the GPU with the library of the commit whose choices are to be pinned (CRT1D_HIP_LIB=<its libcrt1d_hip.so>), never with the
tree under test:   CRT1D_HIP_LIB=variants/libcrt1d_hip_parent.so python tools/gen_launch_reports.py [output.json]
The deep cases are searched here: the smallest nz at which the level launch reports the marker (monotone in nz: bisection)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_launch_reports as T  # noqa: E402

# scheme -> (marker, an nz that shows it: M = 16 still fits / the record is beyond 160 KB)
DEEP = {"n79": (" M=16", 1200), "zq": (" M=16", 2000), "2s": ("record in HBM", 12000)}


def first_nz(scheme, marker, hi, lo=T.NZ):
    """Smallest nz in (lo, hi] whose level report holds `marker` (lo's does not, hi's does)."""
    assert marker not in T.report("levels", scheme, "f64", 8, lo) and marker in T.report("levels", scheme, "f64", 8, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if marker in T.report("levels", scheme, "f64", 8, mid):
            hi = mid
        else:
            lo = mid
        T._inputs.pop((8, mid, "f64"), None)
    return hi


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "launch_reports.json")
    reports, deep = {}, {}
    for scheme in T.SCHEMES:
        for form, dtype, nb in T.shallow_cases(scheme):
            reports[T.case_id(form, scheme, dtype, nb, T.NZ)] = T.report(form, scheme, dtype, nb)
    for scheme, (marker, hi) in DEEP.items():
        nz = first_nz(scheme, marker, hi)
        deep[scheme] = {"nz": nz, "marker": marker}
        for z in (nz - 1, nz):
            reports[T.case_id("levels", scheme, "f64", 8, z)] = T.report("levels", scheme, "f64", 8, z)
    with open(out, "w") as f:
        json.dump({"reports": reports, "deep": deep}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(reports)} reports -> {out}")


if __name__ == "__main__":
    main()
