"""
Time of crt_hip_g_from_pdf_f64 (k_g_from_pdf; npsi = 24 caller angles per column, the eight PDFs of the tests mixed over the columns)
by device events, and beside it the precompute-only call (FLAG_PRECOMPUTE_ONLY: k_colpre and nothing else, nz = 60) for the same columns
as CRT_G_TABLE columns.

    python tools/leaf_pdf_bench.py --out profiles/leaf_pdf/leaf_pdf_bench.json

The events bracket whole calls, not kernels: `g_from_pdf_call` holds the read-back of the descriptors that precedes the launch (20 bytes
per column, one stream synchronisation) and the allocation of the three outputs, `precompute_only_call_<scheme>` the launch of k_colpre
through a prepared Plan.  Report only; no bar.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from crt1d_amd import _lib, batched  # noqa: E402

PDFS = [(0, (0.0, 0.0)), (2, (1.0, 0.0)), (1, (0.3, 0.0)), (2, (0.0, 0.0)), (1, (2.5, 0.0)), (2, (-1.0, 0.0)), (1, (1.0, 0.0)), (2, (0.0, -1.0))]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--ncol", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--npsi", type=int, default=24)
    ap.add_argument("--nz", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    res = {"device": torch.cuda.get_device_name(0), "npsi": args.npsi, "nz": args.nz, "ngl": _lib.LEAF_NGL, "cases": []}
    for ncol in args.ncol:
        kind = torch.as_tensor(np.array([PDFS[c % 8][0] for c in range(ncol)], dtype=np.int32), device=dev)
        param = torch.as_tensor(np.array([PDFS[c % 8][1] for c in range(ncol)], dtype=np.float64), device=dev)
        psi = torch.as_tensor(np.deg2rad(rng.uniform(0.0, 75.0, (ncol, args.npsi))), device=dev)
        case = {"ncol": ncol, "g_from_pdf_call": timed(lambda: batched.leaf_pdf_tables(kind, param, psi=psi), args.reps)}
        case["g_from_pdf_call"]["evaluations_of_G"] = ncol * (_lib.NQ + args.npsi)
        lai = torch.as_tensor(np.linspace(4.0, 0.0, args.nz)[None, :].repeat(ncol, 0), device=dev)
        cols = batched.Columns.from_leaf_pdf(psi[:, 0].contiguous(), lai, kind, param)
        one = torch.full((1, 1), 0.3, dtype=torch.float64, device=dev)
        bands = batched.Bands(one, one, one, one, one)
        for scheme in ("4s", "n79"):
            plan = batched.Plan(scheme, cols, bands, placement="none")
            case[f"precompute_only_call_{scheme}"] = timed(lambda: plan(flags=_lib.FLAG_PRECOMPUTE_ONLY), args.reps)
            del plan
        res["cases"].append(case)
        print(json.dumps(case))
        del cols, lai, kind, param, psi
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
