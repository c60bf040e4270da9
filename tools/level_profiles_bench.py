"""Cost of the band partition's level profiles (``level_profiles=True``, crt1d_amd/dist.py) on one MI355X.

* ``crt_hip_bandsum_finish_f64`` at 1e5 columns x 100 levels x 3 groups -- the whole re-forming pass of BASELINE configs[3] on one rank
  after its reduce -- next to a device-to-device copy measured in the same run: time, rate over its compulsory traffic (reads aI_sl,
  aI_sh, I_dr, I_df_d, I_df_u, writes aI, F, I_d: 1.91 GB), share of 8 TB/s and of the measured copy rate;
* ``BandShardPlan`` step time for zq at a rank's shard of config 4 (1e5 columns x 38 bands x 100 levels, 4 column tiles, world of one:
  no collective), level_profiles off / on, keep_profiles True / False, and the same step with the four tiles' finish added (the compute a
  rank of a multi-rank run adds after its reduce);
* ``message_bytes`` in both modes (the multi-rank wire cost is not measured: one GPU).

    python tools/level_profiles_bench.py [--out FILE] [--reps 30]
"""
import argparse
import json
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crt1d_amd import batched, spectra, synth  # noqa: E402
from crt1d_amd.dist import BandShardPlan  # noqa: E402

PEAK_TBS = 8.0


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def finish_case(reps):
    ncol, nz, ng = 100_000, 100, 3
    d = synth.make_columns(ncol, 2, nz, seed=11)
    cols = batched.Columns.from_host(d)
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {k: torch.rand(sh, dtype=torch.float64, device="cuda", generator=g)
           for k, sh in batched.bandsum_shapes(ncol, nz, ng, profiles=True).items()}
    fin = batched.BandSumFinishPlan(cols, out)
    nl, nv = ncol * (nz - 1) * ng, ncol * nz * ng
    traffic = 8 * (3 * nl + 5 * nv)  # read aI_sl, aI_sh, I_dr, I_df_d, I_df_u; write aI, F, I_d
    t = event_ms(fin, reps)
    # a device-to-device copy of the same number of bytes (half read, half written)
    n = traffic // 16
    src = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    dst = torch.empty_like(src)
    tc = event_ms(lambda: dst.copy_(src), reps)
    fin_tbs = traffic / (t["median_ms"] * 1e-3) / 1e12
    copy_tbs = 2 * 8 * n / (tc["median_ms"] * 1e-3) / 1e12
    return {"shape": [ncol, nz, ng], "compulsory_bytes": traffic, "finish": t, "finish_TBs": fin_tbs,
            "finish_share_of_8TBs": fin_tbs / PEAK_TBS, "copy": tc, "copy_bytes_moved": 2 * 8 * n, "copy_TBs": copy_tbs,
            "finish_share_of_copy_rate": fin_tbs / copy_tbs}


def step_cases(reps):
    ncol, nb, nz, tiles = 100_000, 38, 100, 4
    d = synth.make_columns(ncol, nb, nz, seed=1234)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    bw = torch.as_tensor(spectra.band_weights(d["wle"])).cuda()
    rows = []
    for keep in (True, False):
        for lp in (False, True):
            plan = BandShardPlan("zq", cols, bands, bw, column_tiles=tiles, share_profiles=True, keep_profiles=keep, level_profiles=lp)

            def step():
                plan()
                plan.wait()

            row = {"keep_profiles": keep, "level_profiles": lp, "message_bytes": plan.message_bytes, "step": event_ms(step, reps)}
            if lp:  # + the finish every tile runs after a reduce in a multi-rank run
                fins = [batched.BandSumFinishPlan(cols.slice(t.clo, t.chi), t.views) for t in plan.tiles]

                def step_fin():
                    plan()
                    plan.wait()
                    for f in fins:
                        f()

                row["step_plus_finish"] = event_ms(step_fin, reps)
            rows.append(row)
            del plan
            torch.cuda.empty_cache()
    for keep in (True, False):
        off = next(r for r in rows if r["keep_profiles"] == keep and not r["level_profiles"])
        on = next(r for r in rows if r["keep_profiles"] == keep and r["level_profiles"])
        on["step_cost_vs_off"] = on["step"]["median_ms"] / off["step"]["median_ms"] - 1
        on["step_plus_finish_cost_vs_off"] = on["step_plus_finish"]["median_ms"] / off["step"]["median_ms"] - 1
    return {"shape": [ncol, nb, nz], "scheme": "zq", "column_tiles": tiles, "world": 1, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "finish": finish_case(a.reps), "band_shard_step": step_cases(max(5, a.reps // 3)),
           "wire": "not measured (one GPU: no multi-rank all-reduce)"}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
