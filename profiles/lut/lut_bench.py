"""k_lut_match against the best torch composition, the table build, and the twin retrieval's record.

    kernel   LutMatchPlan() -- k_lut_match + k_lut_merge -- with nbest 1 and 8 at ncol in {1e4, 1e5}, K in {4096, 65536}, nrow in {26, 104, 300},
             one block of observations with weights, no prior.  The kernel issues the four fp64 VALU instructions of the cost contract per
             (column, candidate, row); `bound_ms` is their time, 4 ncol K nrow / 64 wave instructions at RATE (profiles/r03/
             valu_latency.txt: dependent v_mul_f64 / v_add_f64, 4 waves per SIMD), and `bound_fraction` = bound_ms / ms.
    torch    chunked over K so that the residuals fit --chunk-bytes: torch.sub(m[None], y[:, None], out=buf); buf *= s[:, None]; buf *= buf;
             0.5 * buf.sum(-1); topk per chunk; a running merge by topk over (running | chunk).  Only where its ESTIMATED time (8 bytes x 6
             passes per triple at 4 TB/s) stays below --torch-seconds (the others would take minutes of a shared GPU); measured twice, and a
             case counts as a gain only outside that spread.
    build    LutTable.build for K = 4096 and 65536 on a 300-band, 60-level 2s template: 26 rows (2 levels x 13 sensor bands), 104 rows (8 x
             13) and the 300-band spectrum of one level; one run each, wall clock around a synchronise.
    single   one column (Model.retrieve(lut=)): K in {4096, 65536}, 104 rows, nbest 1 and 8 -- K split over up to 256 workgroups, and
             k_lut_merge merging their lists on one lane
    twin     tests/test_gpu_lut.py::twin_run: the errors of the retrieval started from the table, and how many of the 64 columns the same
             plan loses from a fixed mid-box start.

HIP events around blocks of launches on one stream; the median of the blocks after one warm-up block (tools/levels_bench.py).

    python profiles/lut/lut_bench.py [--json profiles/lut/lut_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crt1d_amd import batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402
from sensor_bench import sensor_weights  # noqa: E402

RATE = 484e9  # wave instructions per second, profiles/r03/valu_latency.txt
F64 = dict(dtype=torch.float64, device="cuda")


def problem(ncol, K, nrow, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g, **F64)  # noqa: E731
    table = batched.LutTable(r(K, 5), {"F": r(K, nrow)}, params=("a", "b", "c", "d", "e"), keys=("F",), shape=(1, nrow), scheme="2s", spectral=False)
    return table, r(ncol, 1, nrow), 0.5 + r(ncol, 1, nrow)


def blocks_for(seconds):
    return (7, max(1, min(20, int(0.05 / seconds)))) if seconds < 1.0 else (3, 1)


def run_kernel(args):
    rows = []
    for ncol in (10_000, 100_000):
        for K in (4096, 65536):
            for nrow in (26, 104, 300):
                table, y, s = problem(ncol, K, nrow)
                for nbest in (1, 8):
                    plan = batched.LutMatchPlan(table, {"F": y}, inv_sigma={"F": s}, nbest=nbest)
                    bound = 4.0 * ncol * K * nrow / 64 / RATE
                    ms = timed(plan, *blocks_for(1.25 * bound / 0.8))
                    r = dict(ncol=ncol, K=K, nrow=nrow, nbest=nbest, ms=ms, bound_ms=1e3 * bound, bound_fraction=1e3 * bound / ms,
                             kernel=plan.last_kernel())
                    print(f"kernel {ncol:6d} x {K:5d} x {nrow:3d} nbest {nbest}: {ms:10.3f} ms, {r['bound_fraction']:.2f} of the "
                          f"four-instruction bound | {r['kernel']}", flush=True)
                    rows.append(r)
                    del plan
                del table, y, s
                torch.cuda.empty_cache()
    return rows


def run_single(args):
    rows = []
    for K in (4096, 65536):
        table, y, s = problem(1, K, 104)
        for nbest in (1, 8):
            plan = batched.LutMatchPlan(table, {"F": y}, inv_sigma={"F": s}, nbest=nbest)
            r = dict(ncol=1, K=K, nrow=104, nbest=nbest, ms=timed(plan, 7, 20), kernel=plan.last_kernel())
            print(f"single column x {K:5d} x 104 nbest {nbest}: {r['ms']:.4f} ms | {r['kernel']}", flush=True)
            rows.append(r)
    return rows


def torch_match(table, y, s, nbest, chunk_bytes):
    m, y2, s2 = table.m["F"], y[:, 0], s[:, 0]
    ncol, (K, nrow) = y2.shape[0], m.shape
    kc = max(nbest, min(K, int(chunk_bytes // (8 * ncol * nrow))))
    buf = torch.empty((ncol, kc, nrow), **F64)
    best_c = torch.full((ncol, nbest), float("inf"), **F64)
    best_i = torch.full((ncol, nbest), -1, dtype=torch.int64, device="cuda")

    def run():
        best_c.fill_(float("inf"))
        best_i.fill_(-1)
        for k0 in range(0, K, kc):
            n = min(kc, K - k0)
            b = buf[:, :n]
            torch.sub(m[None, k0:k0 + n], y2[:, None], out=b)
            b.mul_(s2[:, None])
            b.mul_(b)
            c, i = torch.topk(b.sum(-1).mul_(0.5), min(nbest, n), dim=1, largest=False)
            cc, ii = torch.cat([best_c, c], dim=1), torch.cat([best_i, i + k0], dim=1)
            c2, j = torch.topk(cc, nbest, dim=1, largest=False)
            best_c.copy_(c2)
            best_i.copy_(torch.gather(ii, 1, j))
        return best_c, best_i

    return run


def run_torch(args, kernel_rows):
    rows = []
    for r in kernel_rows:
        est = r["ncol"] * r["K"] * r["nrow"] * 8 * 6 / 4e12
        if est > args.torch_seconds:
            rows.append(dict(ncol=r["ncol"], K=r["K"], nrow=r["nrow"], nbest=r["nbest"], torch_ms=None, kernel_ms=r["ms"],
                             verdict=f"not measured: estimated {est:.1f} s per pass"))
            continue
        table, y, s = problem(r["ncol"], r["K"], r["nrow"])
        run = torch_match(table, y, s, r["nbest"], args.chunk_bytes)
        c, i = run()
        plan = batched.LutMatchPlan(table, {"F": y}, inv_sigma={"F": s}, nbest=r["nbest"])
        out = plan()
        torch.cuda.synchronize()
        same_index = bool((out["index"].long() == i).all())
        ms = [timed(run, 2, 1) for _ in range(2)]
        lo, hi = min(ms), max(ms)
        row = dict(ncol=r["ncol"], K=r["K"], nrow=r["nrow"], nbest=r["nbest"], torch_ms=ms, kernel_ms=r["ms"], torch_over_kernel=[v / r["ms"] for v in ms],
                   verdict="gain" if r["ms"] < lo else "loss" if r["ms"] > hi else "inside torch's spread", same_index=same_index,
                   max_rel_cost_diff=float(((out["cost"] - c).abs() / c).max()))
        print(f"torch  {r['ncol']:6d} x {r['K']:5d} x {r['nrow']:3d} nbest {r['nbest']}: {lo:.1f} .. {hi:.1f} ms against {r['ms']:.3f} ms "
              f"[{row['verdict']}], same index {same_index}", flush=True)
        rows.append(row)
        del table, y, s, run, plan
        torch.cuda.empty_cache()
    return rows


def run_build(args):
    nb, nz = 300, 60
    d = synth.make_columns(1, nb, nz, seed=1234)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    sens = batched.SensorSet(sensor_weights(nb, np.random.default_rng(7)))
    g = torch.Generator(device="cuda").manual_seed(1)
    dirs = dict(d_leaf_r=torch.rand((2, nb), generator=g, **F64) * 0.02 - 0.01, d_soil_r=torch.rand((2, nb), generator=g, **F64) * 0.02 - 0.01)
    lo, hi = np.array([-1.0, -1.0, -0.5]), np.array([1.0, 1.0, 0.5])
    rows = []
    for K in (4096, 65536):
        q = batched.lut_sample(lo, hi, K)
        for label, levels, kw in (("26 rows: 2 levels x 13 sensor bands", (0, -1), dict(sensors=sens)),
                                  ("104 rows: 8 levels x 13 sensor bands", tuple(range(0, nz, 8))[:8], dict(sensors=sens)),
                                  ("300 rows: the spectrum of one level", (-1,), {})):
            for chunk in (256, 4096):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                table = batched.LutTable.build("2s", cols, bands, levels, q, keys=("I_df_u",), chunk=chunk, lai=True, **dirs, **kw)
                torch.cuda.synchronize()
                r = dict(K=K, rows=label, nrow=table.nrow, chunk=chunk, seconds=time.perf_counter() - t0)
                print(f"build  K {K:5d} {label}, chunk {chunk}: {r['seconds']:.3f} s", flush=True)
                rows.append(r)
                del table
                torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch-seconds", type=float, default=1.0)
    ap.add_argument("--chunk-bytes", type=float, default=8e9)
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernel,torch,single,build,twin")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lut_bench needs a GPU"
    skip = set(args.skip.split(","))
    prop = torch.cuda.get_device_properties(0)
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "rev": args.rev, "rate_wave_instructions_per_s": RATE}

    def save():
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)

    if "kernel" not in skip:
        out["kernel"] = run_kernel(args)
        save()
        if "torch" not in skip:
            out["torch"] = run_torch(args, out["kernel"])
            save()
    if "single" not in skip:
        out["single_column"] = run_single(args)
        save()
    if "build" not in skip:
        out["build"] = run_build(args)
        save()
    if "twin" not in skip:
        from test_gpu_lut import twin_run

        out["twin"] = twin_run()["summary"]
        print("twin  ", out["twin"], flush=True)
        save()


if __name__ == "__main__":
    main()
