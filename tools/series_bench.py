"""Sun-angle series against the loop of per-step calls it replaces.

For every scheme, uniform and ragged dLAI, at ncol x nb x nz = 2e4 x 12 x 60, 4e3 x 107 x 60 and 1e3 x 300 x 60: nt = 24 sun states,
3 band groups, complete output (profiles=True).
  loop   : nt IntegratedPlan calls (crt_hip_integrated2_f64, K0 in front of each), one per sun state, on the same data
  series : one IntegratedSeriesPlan call (crt_hip_integrated_series_f64)
Timed with device events around `iters` repetitions, `reps` windows per side, the two sides alternating; the loop's own run-to-run
spread is (max - min) / median of its windows.  Before timing, every slice of the series output is compared with the loop's output of
that step (torch.equal).  --loop-lib PATH times the loop through another build of the library (e.g. the parent
commit's), loaded next to this tree's.

    python tools/series_bench.py --out profiles/series/series_bench.json [--loop-lib /path/to/libcrt1d_hip.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crt1d_amd import _lib, batched, synth  # noqa: E402

SHAPES = [(20000, 12, 60), (4000, 107, 60), (1000, 300, 60)]
SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--nt", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--schemes", default=",".join(SCHEMES))
    args = ap.parse_args()
    dev = "cuda:0"
    loop_fn = None
    if args.loop_lib:
        other = ctypes.CDLL(os.path.abspath(args.loop_lib))
        mine = _lib.load().crt_hip_integrated2_f64
        loop_fn = other.crt_hip_integrated2_f64
        loop_fn.restype, loop_fn.argtypes = mine.restype, mine.argtypes
    rows = []
    for ncol, nb, nz in SHAPES:
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=3, uniform_dlai=uniform)
            s = synth.make_sun_series(d, args.nt, seed=4)
            cols, bands, sun = batched.Columns.from_host(d, dev), batched.Bands.from_host(d, dev), batched.SunSeries.from_host(s, dev)
            w = torch.as_tensor(np.random.default_rng(5).uniform(0, 1, (3, nb)), device=dev)
            for scheme in args.schemes.split(","):
                ser = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, w, profiles=True)
                ws, out = None, None
                steps = []
                for t in range(args.nt):
                    c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla)
                    b = batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), bands.leaf_r, bands.leaf_t, bands.soil_r)
                    p = batched.IntegratedPlan(scheme, c, b, w, profiles=True, workspace=ws, out=out)
                    ws, out = p.workspace, p.out
                    if loop_fn is not None:
                        p._fn = loop_fn
                    steps.append(p)

                def loop():
                    for p in steps:
                        p()

                for _ in range(2):
                    loop()
                    ser()
                torch.cuda.synchronize()
                # the two sides must agree bit for bit at every step before their times are compared (the loop reuses one output set)
                got = ser()
                for t, p in enumerate(steps):
                    ref = p()
                    torch.cuda.synchronize()
                    for k, v in ref.items():
                        assert torch.equal(got[k][:, t], v), (scheme, ncol, nb, uniform, k, t)
                iters = max(1, int(40.0 / max(timed(loop, 1), 0.05)))
                tl, ts = [], []
                for _ in range(args.reps):
                    tl.append(timed(loop, iters))
                    ts.append(timed(ser, iters))
                ml, ms = statistics.median(tl), statistics.median(ts)
                row = dict(scheme=scheme, ncol=ncol, nb=nb, nz=nz, dlai="uniform" if uniform else "ragged", nt=args.nt, ngroup=3,
                           loop_ms=round(ml, 4), loop_spread=round((max(tl) - min(tl)) / ml, 4), series_ms=round(ms, 4),
                           series_spread=round((max(ts) - min(ts)) / ms, 4), series_over_loop=round(ms / ml, 4), iters=iters,
                           bitwise_equal=True, kernel=ser.last_kernel())
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = dict(command=" ".join(["python", "tools/series_bench.py"] + sys.argv[1:]), device=torch.cuda.get_device_name(0),
               loop="parent commit's library" if args.loop_lib else "this tree's library", timing="device events, median of windows", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
