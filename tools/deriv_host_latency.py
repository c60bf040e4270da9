#!/usr/bin/env python
"""Call latency of the three level-derivative plans (plan built once, ``__call__`` repeated), for an A/B of two checkouts in one job.

    python tools/deriv_host_latency.py worker <checkout root>            one JSON line: {config: [seconds per call, one per repeat]}
    python tools/deriv_host_latency.py ab <parent root> <new root> OUT   alternates parent, new, parent (each a fresh process) ROUNDS
                                                                         times and writes OUT (profiles/deriv_host/latency.json)

A repeat is CALLS calls and one synchronise behind them, on a host clock: what a caller who re-runs a plan in a loop pays per call.  The
two parent series give the parent's own run-to-run spread, the yardstick for the difference between the new tree and the parent."""
import json
import os
import statistics
import subprocess
import sys
import time

SHAPE = (6, 13, 9)  # (ncol, nb, nz)
SCHEMES = ("2s", "n79")
PLANS = ("jac", "dlai", "dleaf")
WARMUP, CALLS, REPEATS, ROUNDS = 300, 2000, 7, 3


def worker(root):
    sys.path.insert(0, root)
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(*SHAPE, seed=11)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    lev = tuple(range(SHAPE[2]))
    res = {}
    for scheme in SCHEMES:
        plans = {"jac": batched.LevelsJacPlan(scheme, cols, bands, lev), "dlai": batched.LevelsDlaiPlan(scheme, cols, bands, lev),
                 "dleaf": batched.LevelsDleafPlan(scheme, cols, bands, lev, tan)}
        for name in PLANS:
            plan = plans[name]
            for _ in range(WARMUP):
                plan()
            torch.cuda.synchronize()
            per = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    plan()
                torch.cuda.synchronize()
                per.append((time.perf_counter() - t0) / CALLS)
            res[f"{name}/{scheme}"] = per
    print(json.dumps(res))


def ab(parent, new, out):
    series = {"parent_a": {}, "new": {}, "parent_b": {}}
    for _ in range(ROUNDS):
        for label, root in (("parent_a", parent), ("new", new), ("parent_b", parent)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", root], check=True, capture_output=True, text=True,
                               timeout=300)
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                series[label].setdefault(k, []).extend(v)
    configs = {}
    for k in series["new"]:
        med = {label: statistics.median(s[k]) * 1e6 for label, s in series.items()}
        spread = abs(med["parent_a"] - med["parent_b"])
        parent_med = statistics.median(series["parent_a"][k] + series["parent_b"][k]) * 1e6
        configs[k] = {"median_us": {**{label: round(m, 3) for label, m in med.items()}, "parent": round(parent_med, 3)},
                      "parent_spread_us": round(spread, 3), "new_minus_parent_us": round(med["new"] - parent_med, 3),
                      "within_spread": abs(med["new"] - parent_med) <= spread}
        print(k, configs[k])
    doc = {"what": "time per plan call in microseconds: CALLS calls and one synchronise on a host clock, medians over ROUNDS x REPEATS repeats per "
                   "series (parent_a, new, parent_b alternate, each a fresh process); parent = both parent series together, parent_spread = "
                   "|parent_a - parent_b|",
           "shape_ncol_nb_nz": SHAPE, "warmup": WARMUP, "calls": CALLS, "repeats": REPEATS, "rounds": ROUNDS, "configs": configs}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "worker":
        worker(sys.argv[2])
    else:
        ab(*sys.argv[2:5])
