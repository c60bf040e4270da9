"""Level-subset solve against its neighbours: per scheme, at 1e4 x 300 x 60 fp64, uniform and ragged columns,
the time of one call of
    full   the profile solve (Plan, all nz levels of I_dr, I_df_d, I_df_u, F and the scheme's extras)
    int    IntegratedPlan with one band group (no profile written)
    lev2   LevelsPlan at (0, nz-1)
    levh   LevelsPlan at every 2nd level (30 of 60)
and, with float32 spectra, lev2 / levh of the f32 entry.  K0 (column precompute) is part of every call.  Device events around blocks of
--reps calls on one stream; the median of --blocks blocks is reported, after one warm-up block per case.

    python tools/levels_bench.py [--schemes 2s,n79] [--ncol 10000] [--blocks 7] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crt1d_amd import batched, spectra, synth  # noqa: E402


def timed(fn, blocks, reps):
    st = torch.cuda.current_stream()
    for _ in range(reps):  # warm-up block
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,4s,bl,g77,bf,n79,zq,zq_pa")
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--nb", type=int, default=300)
    ap.add_argument("--nz", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "levels_bench needs a GPU"
    ncol, nb, nz = args.ncol, args.nb, args.nz
    lev2, levh = (0, nz - 1), tuple(range(0, nz, 2))
    rows = []
    for uniform in (True, False):
        d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
        cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
        b32 = batched.Bands(*[None if getattr(bands, k) is None else getattr(bands, k).float()
                              for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
        w = torch.as_tensor(spectra.band_weights(d["wle"], ("solar",)), dtype=torch.float64, device="cuda")
        for scheme in args.schemes.split(","):
            r = {"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz]}
            plan = batched.Plan(scheme, cols, bands)
            r["full_ms"] = timed(plan, args.blocks, args.reps)
            del plan
            ip = batched.IntegratedPlan(scheme, cols, bands, w)
            r["int_ms"] = timed(ip, args.blocks, args.reps)
            for tag, lev in (("lev2", lev2), ("levh", levh)):
                lp = batched.LevelsPlan(scheme, cols, bands, lev)
                r[f"{tag}_ms"] = timed(lp, args.blocks, args.reps)
                r[f"{tag}_kernel"] = lp.last_kernel()
                lp32 = batched.LevelsPlan(scheme, cols, b32, lev)
                r[f"{tag}_f32_ms"] = timed(lp32, args.blocks, args.reps)
            torch.cuda.empty_cache()
            r["full_over_lev2"] = r["full_ms"] / r["lev2_ms"]
            rows.append(r)
            print(f"{scheme:5s} {r['columns']:7s} full {r['full_ms']:.3f}  int {r['int_ms']:.3f}  lev(0,nz-1) {r['lev2_ms']:.3f}"
                  f" [{r['full_over_lev2']:.1f}x]  lev(every 2nd) {r['levh_ms']:.3f}  f32 {r['lev2_f32_ms']:.3f} / {r['levh_f32_ms']:.3f} ms"
                  f"  | {r['lev2_kernel']} | {r['levh_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
