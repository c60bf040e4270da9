"""crt_hip_lut_posterior_f64 against the chunked torch composition and against the match alone.

    entry      LutPosteriorPlan() -- the match with nbest = 1, k_lut_moments, k_lut_moments_finish -- with npar 5 and 10 at ncol in {1e4,
               1e5}, K in {4096, 65536}, nrow in {26, 104, 300} (the shapes of profiles/lut/lut_bench.py), one block of observations with
               weights, no prior, temperature 1.  `match_ms` is LutMatchPlan(nbest=1) on the same inputs and `over_match` the entry's time
               as a multiple of it: two passes of cost arithmetic put the floor near 2.
    skip       the share of (group of 64 columns, candidate) pairs whose weight is 0 in all 64 columns -- what k_lut_moments skips -- and the
               entry's time, for a wide posterior (the temperature at which the median ess is about K / 10), a narrow one (about 3) and
               a sharp one (T = 1e-4: nearly every weight underflows), at 1e4 x 4096 x 26 with npar 5; the weights are recomputed in
               torch for the count.
    baseline   the chunked torch composition of lut_bench.py extended by the weights and the moments: a first pass over the chunks of K
               for cmin, a second that forms exp(-(cost - cmin) / T) and accumulates S0, Sq, S1 = w^T d and S2 = (w d)^T d by matmul.  Only
               where its estimated time stays below --torch-seconds; measured twice, and a case counts as a gain only outside that spread.
               With --baseline-root it runs in a child process on another checkout (the parent commit's tree and library), so that
               nothing of this tree is loaded there.

HIP events around blocks of launches on one stream; the median of 7 blocks after one warm-up block (tools/levels_bench.py).

    python profiles/lut_posterior/lut_posterior_bench.py [--json profiles/lut_posterior/lut_posterior_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.abspath(__file__)


def _root():
    for i, a in enumerate(sys.argv):
        if a == "--root":
            return os.path.abspath(sys.argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.dirname(HERE)))


ROOT = _root()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from crt1d_amd import batched  # noqa: E402
from levels_bench import timed  # noqa: E402

F64 = dict(dtype=torch.float64, device="cuda")
SHAPES = [(ncol, K, nrow) for ncol in (10_000, 100_000) for K in (4096, 65536) for nrow in (26, 104, 300)]


def problem(ncol, K, nrow, npar, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g, **F64)  # noqa: E731
    table = batched.LutTable(r(K, npar), {"F": r(K, nrow)}, params=tuple(f"p{i}" for i in range(npar)), keys=("F",), shape=(1, nrow),
                             scheme="2s", spectral=False)
    return table, r(ncol, 1, nrow), 0.5 + r(ncol, 1, nrow)


def blocks_for(seconds):
    return (7, max(1, min(20, int(0.05 / seconds)))) if seconds < 1.0 else (7, 1)


def run_entry(args):
    rows = []
    for ncol, K, nrow in SHAPES:
        for npar in (5, 10):
            table, y, s = problem(ncol, K, nrow, npar)
            match = batched.LutMatchPlan(table, {"F": y}, inv_sigma={"F": s}, nbest=1)
            est = 4.0 * ncol * K * nrow / 64 / 484e9 / 0.55
            match_ms = timed(match, *blocks_for(est))
            plan = batched.LutPosteriorPlan(table, {"F": y}, inv_sigma={"F": s})
            ms = timed(plan, *blocks_for(3 * est))
            out = plan()
            torch.cuda.synchronize()
            r = dict(ncol=ncol, K=K, nrow=nrow, npar=npar, ms=ms, match_ms=match_ms, over_match=ms / match_ms, kernel=plan.last_kernel(),
                     ess_median=float(out["ess"].median()))
            print(f"entry {ncol:6d} x {K:5d} x {nrow:3d} npar {npar:2d}: {ms:10.3f} ms, match {match_ms:10.3f} ms, x {r['over_match']:.2f} "
                  f"| ess {r['ess_median']:.1f} | {r['kernel']}", flush=True)
            rows.append(r)
            del plan, match, table, y, s, out
            torch.cuda.empty_cache()
    return rows


def costs(table, y, s):
    m, y2, s2 = table.m["F"], y[:, 0], s[:, 0]
    return 0.5 * (((m[None] - y2[:, None]) * s2[:, None]) ** 2).sum(-1)


def run_skip(args):
    ncol, K, nrow, npar = 10_000, 4096, 26, 5
    table, y, s = problem(ncol, K, nrow, npar)
    c = costs(table, y, s)
    c -= c.min(dim=1, keepdim=True).values

    def ess(T):
        w = torch.exp(-c / T)
        return float(((w.sum(1) ** 2) / (w * w).sum(1)).median())

    rows = []
    for label, target in (("wide", K / 10), ("narrow", 3.0), ("sharp", None)):
        lo, hi = 1e-6, 1e6
        for _ in range(60 if target else 0):  # ess grows with T: bisection on a log scale
            mid = (lo * hi) ** 0.5
            lo, hi = (mid, hi) if ess(mid) < target else (lo, mid)
        T = hi if target else 1e-4  # (sharp: cost - cmin of nearly every candidate beyond the 745 T at which exp underflows to 0)
        w = torch.exp(-c / T)
        pad = (-ncol) % 64
        zero = torch.cat([w == 0, torch.ones((pad, K), dtype=torch.bool, device="cuda")]).reshape(-1, 64, K).all(dim=1)
        plan = batched.LutPosteriorPlan(table, {"F": y}, inv_sigma={"F": s}, temperature=T)
        r = dict(ncol=ncol, K=K, nrow=nrow, npar=npar, posterior=label, temperature=T, ess_median=ess(T), skipped_share=float(zero.double().mean()),
                 ms=timed(plan, 7, 20))
        print(f"skip  {label}: T = {T:.3g}, ess {r['ess_median']:.1f}, {100 * r['skipped_share']:.1f} % of the (64 columns, candidate) pairs "
              f"skipped, {r['ms']:.3f} ms", flush=True)
        rows.append(r)
    return rows


def torch_posterior(table, y, s, T, chunk_bytes):
    m, q, y2, s2 = table.m["F"], table.q, y[:, 0], s[:, 0]
    ncol, (K, nrow), npar = y2.shape[0], m.shape, table.q.shape[1]
    kc = max(1, min(K, int(chunk_bytes // (8 * ncol * nrow))))
    buf = torch.empty((ncol, kc, nrow), **F64)

    def cost(k0, n):
        b = buf[:, :n]
        torch.sub(m[None, k0:k0 + n], y2[:, None], out=b)
        b.mul_(s2[:, None])
        b.mul_(b)
        return b.sum(-1).mul_(0.5)

    def run():
        cmin = torch.full((ncol,), float("inf"), **F64)
        kb = torch.zeros((ncol,), dtype=torch.int64, device="cuda")
        for k0 in range(0, K, kc):
            c, i = cost(k0, min(kc, K - k0)).min(dim=1)
            better = c < cmin
            cmin, kb = torch.where(better, c, cmin), torch.where(better, i + k0, kb)
        qb = q[kb]
        s0, sq = torch.zeros((ncol,), **F64), torch.zeros((ncol,), **F64)
        s1, s2m = torch.zeros((ncol, npar), **F64), torch.zeros((ncol, npar, npar), **F64)
        for k0 in range(0, K, kc):
            n = min(kc, K - k0)
            w = torch.exp((cmin[:, None] - cost(k0, n)) / T)
            d = q[None, k0:k0 + n] - qb[:, None]
            t = w[:, :, None] * d
            s0 += w.sum(1)
            sq += (w * w).sum(1)
            s1 += t.sum(1)
            s2m += torch.bmm(t.transpose(1, 2), d)
        mm = s1 / s0[:, None]
        return qb + mm, s2m / s0[:, None, None] - mm[:, :, None] * mm[:, None, :], s0 * s0 / sq, kb

    return run


def run_baseline(args):
    rows = []
    for ncol, K, nrow in SHAPES:
        for npar in (5, 10):
            est = ncol * K * nrow * 8 * 12 / 4e12  # (two passes of the six of the match's composition)
            if est > args.torch_seconds:
                rows.append(dict(ncol=ncol, K=K, nrow=nrow, npar=npar, torch_ms=None, verdict=f"not measured: estimated {est:.1f} s per pass"))
                continue
            table, y, s = problem(ncol, K, nrow, npar)
            run = torch_posterior(table, y, s, 1.0, args.chunk_bytes)
            ms = [timed(run, 2, 1) for _ in range(2)]
            mean, cov, ess, kb = run()
            torch.cuda.synchronize()
            rows.append(dict(ncol=ncol, K=K, nrow=nrow, npar=npar, torch_ms=ms, mean_sum=float(mean.sum()), cov_trace_sum=float(cov.diagonal(dim1=1, dim2=2).sum()),
                             ess_median=float(ess.median())))
            print(f"torch {ncol:6d} x {K:5d} x {nrow:3d} npar {npar:2d}: {ms[0]:.1f}, {ms[1]:.1f} ms", flush=True)
            del table, y, s, run, mean, cov, ess, kb
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch-seconds", type=float, default=1.2)
    ap.add_argument("--chunk-bytes", type=float, default=8e9)
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: entry,skip,baseline")
    ap.add_argument("--only-baseline", action="store_true", help="the child's call: the torch composition alone")
    ap.add_argument("--root", default=None, help="the checkout whose crt1d_amd is imported (default: this file's)")
    ap.add_argument("--baseline-root", default=None, help="run the baseline in a child process on this checkout (with its own built library)")
    ap.add_argument("--bench", default=None, help="JSON file with the result lines of bench.py on this tree and on the parent's, recorded as given")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lut_posterior_bench needs a GPU"
    skip = set(args.skip.split(","))
    prop = torch.cuda.get_device_properties(0)
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "rev": args.rev}

    def save():
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)

    if args.only_baseline:
        out["baseline"] = run_baseline(args)
        save()
        return
    if "entry" not in skip:
        out["entry"] = run_entry(args)
        save()
    if "skip" not in skip:
        out["skip"] = run_skip(args)
        save()
    if "baseline" not in skip:
        if args.baseline_root:
            tmp = os.path.abspath(args.json or "lut_posterior_bench.json") + ".baseline"
            cmd = [sys.executable, HERE, "--only-baseline", "--root", args.baseline_root, "--json", tmp, "--torch-seconds", str(args.torch_seconds),
                   "--chunk-bytes", str(args.chunk_bytes)]
            subprocess.run(cmd, check=True, env=dict(os.environ, CRT1D_HIP_LIB=os.path.join(os.path.abspath(args.baseline_root), "crt1d_amd", "libcrt1d_hip.so")))
            with open(tmp) as f:
                base = json.load(f)["baseline"]
            os.remove(tmp)
            out["baseline_root"] = "a checkout of the parent commit, in a child process"
        else:
            base = run_baseline(args)
        entry = {(r["ncol"], r["K"], r["nrow"], r["npar"]): r["ms"] for r in out.get("entry", [])}
        for r in base:
            ms = entry.get((r["ncol"], r["K"], r["nrow"], r["npar"]))
            if ms is not None and r["torch_ms"]:
                r["entry_ms"], r["torch_over_entry"] = ms, [v / ms for v in r["torch_ms"]]
                r["verdict"] = "gain" if ms < min(r["torch_ms"]) else "loss" if ms > max(r["torch_ms"]) else "inside torch's spread"
        out["baseline"] = base
        save()
    if args.bench:
        with open(args.bench) as f:
            out["bench_py"] = json.load(f)
        save()


if __name__ == "__main__":
    main()
