"""Sensor-band outputs against the path they replace: per scheme and shape, uniform and ragged columns, 13 sensor
bands, the time of
    sens   one SensorLevelsPlan call at (0, nz-1): the sums of I_dr, I_df_d, I_df_u, F, [ncol][2][13] each
    old    LevelsPlan at (0, nz-1) (the four spectra, [ncol][2][nb] each) followed by ceil(13 / 4) calls of crt_hip_band_reduce_f64 with dense
           weights over all nb bands -- on ONE of the four spectra (I_df_u): the cheapest reading of what a user has without the fused call
    old4   the same with all four spectra reduced (4 x ceil(13 / 4) calls): what it takes to get everything `sens` returns
in one process.  K0 (column precompute) is part of every call.  Device events around blocks of --reps calls on one stream; the median of
--blocks blocks is reported, after one warm-up block per case (the method of tools/levels_bench.py).

    python tools/sensor_bench.py [--schemes 2s,zq] [--shapes 10000x300x60,2000x2151x60] [--json profiles/sensor/sensor_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crt1d_amd import _lib, batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402

NSENS = 13


def sensor_weights(nb, rng):
    """13 overlapping supports of ~nb / 8 bands with random positive weights, spread over the spectrum (dense, zeros outside)."""
    w = np.zeros((NSENS, nb))
    width = max(1, nb // 8)
    for s in range(NSENS):
        lo = (s * (nb - width)) // (NSENS - 1)
        w[s, lo:lo + width] = rng.uniform(0.1, 1.0, width)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,zq")
    ap.add_argument("--shapes", default="10000x300x60,2000x2151x60")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sensor_bench needs a GPU"
    lib = _lib.load()
    rows = []
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        lev = (0, nz - 1)
        w = sensor_weights(nb, np.random.default_rng(7))
        sens = batched.SensorSet(w)
        wd = torch.as_tensor(w, device="cuda")
        chunks = [wd[i:i + 4].contiguous() for i in range(0, NSENS, 4)]
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            for scheme in args.schemes.split(","):
                r = {"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz], "nsens": NSENS}
                sp = batched.SensorLevelsPlan(scheme, cols, bands, lev, sens)
                r["sens_ms"] = timed(sp, args.blocks, args.reps)
                r["sens_kernel"] = sp.last_kernel()
                lp = batched.LevelsPlan(scheme, cols, bands, lev)
                red = {k: [torch.empty((ncol * 2, c.shape[0]), dtype=torch.float64, device="cuda") for c in chunks] for k in lp.out}
                stream = torch.cuda.current_stream().cuda_stream

                def old(keys):
                    lp()
                    for k in keys:
                        for c, o in zip(chunks, red[k]):
                            st = lib.crt_hip_band_reduce_f64(lp.out[k].data_ptr(), ncol * 2, nb, c.data_ptr(), c.shape[0], o.data_ptr(), stream)
                            assert st == 0, st

                r["levels_ms"] = timed(lp, args.blocks, args.reps)
                r["old_ms"] = timed(lambda: old(("I_df_u",)), args.blocks, args.reps)
                r["old4_ms"] = timed(lambda: old(tuple(lp.out)), args.blocks, args.reps)
                torch.cuda.synchronize()
                # the two paths compute the same sums (loosely: this is a benchmark, tests/test_gpu_sensor.py holds the bound)
                for k in lp.out:
                    ref = torch.cat(red[k], dim=1).view(ncol, 2, NSENS)
                    assert torch.allclose(sp.out[k], ref, rtol=1e-12, atol=0), (scheme, k)
                r["old_over_sens"] = r["old_ms"] / r["sens_ms"]
                r["old4_over_sens"] = r["old4_ms"] / r["sens_ms"]
                rows.append(r)
                print(f"{scheme:5s} {r['columns']:7s} {shape:14s} sens {r['sens_ms']:.3f}  levels {r['levels_ms']:.3f}  old {r['old_ms']:.3f}"
                      f" [{r['old_over_sens']:.2f}x]  old4 {r['old4_ms']:.3f} [{r['old4_over_sens']:.2f}x] ms | {r['sens_kernel']}", flush=True)
                del sp, lp, red
                torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
