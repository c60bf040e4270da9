"""Sun-angle series of level spectra against the loop of per-step level calls it replaces.

For every scheme, uniform and ragged dLAI, at ncol x nb x nz = 2e4 x 12 x 60, 4e3 x 107 x 60, 1e3 x 300 x 60 and 200 x 2151 x 60: nt = 24 sun
states, all four outputs, at the levels (0, nz-1) (f64 and f32) and at every 2nd level (f64).
  loop   : nt LevelsPlan calls (crt_hip_levels_f64 / _f32, K0 in front of each), one per sun state, on the same data
  series : one LevelsSeriesPlan call (crt_hip_levels_series_f64 / _f32)
Timed with device events around `iters` repetitions, `reps` windows per side, the two sides alternating; the loop's own run-to-run
spread is (max - min) / median of its windows.  Before timing, every slice of the series output is compared with the loop's output of
that step (torch.equal).  --loop-lib PATH times the loop through another build of the library (the parent commit's), loaded next to
this tree's.

    python tools/levels_series_bench.py --out profiles/levels_series/levels_series_bench.json --loop-lib /path/to/libcrt1d_hip.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crt1d_amd import _lib, batched, synth  # noqa: E402

SHAPES = [(20000, 12, 60), (4000, 107, 60), (1000, 300, 60), (200, 2151, 60)]
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
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--schemes", default=",".join(SCHEMES))
    ap.add_argument("--shapes", default=None, help="indices into SHAPES, e.g. 0,2")
    args = ap.parse_args()
    dev = "cuda:0"
    loop_fns = {}
    if args.loop_lib:
        other = ctypes.CDLL(os.path.abspath(args.loop_lib))
        for suffix in ("f64", "f32"):
            mine = getattr(_lib.load(), f"crt_hip_levels_{suffix}")
            fn = getattr(other, f"crt_hip_levels_{suffix}")
            fn.restype, fn.argtypes = mine.restype, mine.argtypes
            loop_fns[suffix] = fn
    shapes = SHAPES if args.shapes is None else [SHAPES[int(i)] for i in args.shapes.split(",")]
    rows = []
    for ncol, nb, nz in shapes:
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=3, uniform_dlai=uniform)
            s = synth.make_sun_series(d, args.nt, seed=4)
            cols, b64, s64 = batched.Columns.from_host(d, dev), batched.Bands.from_host(d, dev), batched.SunSeries.from_host(s, dev)
            b32 = batched.Bands(*[getattr(b64, k).to(torch.float32) for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
            s32 = batched.SunSeriesF32.from_host(s, dev)
            for levels, tag, io in (((0, nz - 1), "ends", "f64"), ((0, nz - 1), "ends", "f32"), (tuple(range(0, nz, 2)), "every 2nd", "f64")):
                bands, sun = (b64, s64) if io == "f64" else (b32, s32)
                for scheme in args.schemes.split(","):
                    ser = batched.LevelsSeriesPlan(scheme, cols, bands, sun, levels)
                    ws, out = None, None
                    steps = []
                    for t in range(args.nt):
                        c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla)
                        b = batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), bands.leaf_r, bands.leaf_t, bands.soil_r)
                        p = batched.LevelsPlan(scheme, c, b, levels, workspace=ws, out=out)
                        ws, out = p.workspace, p.out
                        if loop_fns:
                            p._fn = loop_fns[io]
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
                            assert torch.equal(got[k][:, t], v), (scheme, ncol, nb, uniform, tag, io, k, t)
                    iters = max(1, int(args.window_ms / max(timed(loop, 1), 0.05)))
                    tl, ts = [], []
                    for _ in range(args.reps):
                        tl.append(timed(loop, iters))
                        ts.append(timed(ser, iters))
                    ml, ms = statistics.median(tl), statistics.median(ts)
                    spread = (max(tl) - min(tl)) / ml
                    row = dict(scheme=scheme, ncol=ncol, nb=nb, nz=nz, dlai="uniform" if uniform else "ragged", nt=args.nt, levels=tag,
                               nsel=len(levels), io=io, loop_ms=round(ml, 4), loop_spread=round(spread, 4), series_ms=round(ms, 4),
                               series_spread=round((max(ts) - min(ts)) / ms, 4), series_over_loop=round(ms / ml, 4),
                               not_slower=bool(ms <= ml * (1 + spread)), iters=iters, bitwise_equal=True, kernel=ser.last_kernel())
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del ser, steps, got, ws, out
            torch.cuda.empty_cache()
    res = dict(command=" ".join(["python", "tools/levels_series_bench.py"] + sys.argv[1:]), device=torch.cuda.get_device_name(0),
               loop="parent commit's library" if args.loop_lib else "this tree's library", timing="device events, median of windows", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
