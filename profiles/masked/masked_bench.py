"""What ``evaluate=`` and ``check_every=`` of the retrieval plans buy over 20 steps: per scheme and shape, a
RetrievalPlan on the 13-band set of tools/sensor_bench.py and a SpectralRetrievalPlan, levels (0, nz-1), keys I_df_d and I_df_u, three
shared directions in (leaf_r, leaf_t, soil_r) plus ln LAI plus the leaf angle, a noise-free twin whose truths fill the box, default
damping, xtol = 1e-6.

    parent      plan.run(20) through the library and the package of --parent-root (any checkout with its library built, meant for the
                parent commit), in a CHILD process, measured TWICE: the two totals are the noise band
    all, running, accepted      this tree's evaluate= modes ("accepted": RetrievalPlan only)
    check4      run(20, check_every=4) with evaluate="running": host time, the synchronisations included

Every mode: one warm-up run, then --reps runs from reset(), device events before every step; reported are the median total, the median
time of every step, and -- from one more run, untimed -- the share of columns running before each step and accepted in it.

    python profiles/masked/masked_bench.py --parent-root variants/parent [--json profiles/masked/masked_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:  # (the child: the tree whose package and library it measures)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crt1d_amd import batched, synth  # noqa: E402
from sensor_bench import sensor_weights  # noqa: E402

KEYS = ("I_df_d", "I_df_u")
NTAN, NSTEP = 3, 20
LM = dict(lam0=1e-2, xtol=1e-6)


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        sens = batched.SensorSet(sensor_weights(nb, np.random.default_rng(7)))
        g = torch.Generator(device="cuda").manual_seed(1)
        dirs = [torch.rand((NTAN, nb), dtype=torch.float64, device="cuda", generator=g) * 0.02 - 0.01 for _ in range(3)]
        d = synth.make_columns(ncol, nb, nz, seed=1234)
        d["g_kind"] = np.full(ncol, 3, dtype=np.int32)  # ellipsoidal: the leaf angle is a live parameter
        d["g_param"] = np.full(ncol, 1.2)
        cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
        lo = torch.tensor([-1.0] * NTAN + [-0.7, 0.4], dtype=torch.float64, device="cuda")
        hi = torch.tensor([1.0] * NTAN + [0.7, 3.5], dtype=torch.float64, device="cuda")
        truth = lo + (hi - lo) * torch.rand((ncol, NTAN + 2), dtype=torch.float64, device="cuda", generator=g)
        for scheme in args.schemes.split(","):
            b = bands if scheme != "bl" else batched.Bands(bands.I_dr0, bands.I_df0, bands.leaf_r, bands.leaf_t, None)
            kw = dict(d_leaf_r=dirs[0], d_leaf_t=dirs[1], lai=True, leaf=True, lo=lo, hi=hi, **LM)
            if scheme != "bl":
                kw["d_soil_r"] = dirs[2]
            for kind in ("sensor", "spectral"):
                r = {"scheme": scheme, "plan": kind, "shape": [ncol, nb, nz], "npar": NTAN + 2}

                def make(y=None, p0=None, kind=kind, scheme=scheme, b=b, kw=kw, **extra):
                    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
                    if kind == "sensor":
                        y = y or {k: z(ncol, 2, sens.nsens) for k in KEYS}
                        return batched.RetrievalPlan(scheme, cols, b, (0, nz - 1), sens, y, keys=KEYS, p0=p0, **kw, **extra)
                    y = y or {k: z(ncol, 2, nb) for k in KEYS}
                    return batched.SpectralRetrievalPlan(scheme, cols, b, (0, nz - 1), y, keys=KEYS, p0=p0, **kw, **extra)

                plan = make(p0=truth)  # the observations: the plan's own forward result at the truth
                if kind == "sensor":
                    plan.step()
                    y = {k: v.clone() for k, v in plan.fwd.out.items()}
                else:
                    y = plan.fitted()
                del plan
                yield r, make, y


def measure(make, y, reps, check_every=None, **extra):
    plan = make(y, **extra)
    plan.run(NSTEP)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(NSTEP + 1)]
    totals, steps, host = [], [], []
    for _ in range(reps):
        plan.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if check_every is None:
            for i in range(NSTEP):
                ev[i].record()
                plan.step()
            ev[NSTEP].record()
            torch.cuda.synchronize()
            steps.append([ev[i].elapsed_time(ev[i + 1]) for i in range(NSTEP)])
            totals.append(ev[0].elapsed_time(ev[NSTEP]))
        else:
            plan.run(NSTEP, check_every=check_every)
            torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    out = {"host_ms": float(np.median(host))}
    if check_every is None:
        out.update(total_ms=float(np.median(totals)), step_ms=[float(v) for v in np.median(np.array(steps), axis=0)])
        plan.reset()
        running, accepted, before = [], [], plan.naccept.sum()
        for _ in range(NSTEP):
            running.append((plan.status == 0).double().mean())
            plan.step()
            now = plan.naccept.sum()
            accepted.append((now - before).double() / plan.status.numel())
            before = now
        out.update(running_share=[float(v) for v in running], accepted_share=[float(v) for v in accepted])
    else:
        out["steps_done"] = int(getattr(plan, "nsteps", NSTEP))
    del plan
    torch.cuda.empty_cache()
    return out


def run(args, parent):
    rows = []
    for r, make, y in cases(args):
        if parent:
            r["parent"] = [measure(make, y, args.reps) for _ in range(2)]
        else:
            r["all"] = measure(make, y, args.reps, evaluate="all")
            r["running"] = measure(make, y, args.reps, evaluate="running")
            if r["plan"] == "sensor":
                r["accepted"] = measure(make, y, args.reps, evaluate="accepted")
            r["check4"] = measure(make, y, args.reps, check_every=4, evaluate="running")
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl")
    ap.add_argument("--shapes", default="10000x300x60,2000x2151x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="tree (package + built library) of the parent commit")
    ap.add_argument("--parent-rev", default=None, help="git revision of that tree, recorded in the JSON as given")
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "parent"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "masked_bench needs a GPU"
    if args.role == "parent":
        json.dump({"rows": run(args, True)}, sys.stdout)
        return
    rows = run(args, False)
    if args.parent_root:
        cmd = [sys.executable, os.path.abspath(__file__), "--role", "parent", "--root", args.parent_root, "--schemes", args.schemes, "--shapes", args.shapes,
               "--reps", str(args.reps)]
        child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=500)  # a fresh process: its own library
        for r, p in zip(rows, json.loads(child.stdout.decode().strip().splitlines()[-1])["rows"]):
            assert (r["scheme"], r["plan"], r["shape"]) == (p["scheme"], p["plan"], p["shape"])
            r["parent"] = p["parent"]
    for r in rows:
        band = sorted(p["total_ms"] for p in r.get("parent", [])) or [float("nan")] * 2
        r["verdict"] = {m: "gain" if r[m]["total_ms"] < band[0] else "loss" if r[m]["total_ms"] > band[1] else "inside the parent's band"
                        for m in ("all", "running", "accepted") if m in r}
        first = {m: r[m]["step_ms"][0] for m in ("all", "running", "accepted") if m in r}  # every column runs in the first step
        print(f"{r['scheme']:3s} {r['plan']:8s} {'x'.join(map(str, r['shape'])):14s} parent {band[0]:.2f} .. {band[1]:.2f} ms | " +
              "  ".join(f"{m} {r[m]['total_ms']:.2f} [{r['verdict'][m]}]" for m in r["verdict"]) +
              f" | check4 host {r['check4']['host_ms']:.2f} ms after {r['check4']['steps_done']} steps (running host {r['running']['host_ms']:.2f})"
              f" | first step {first} | running share at step 1, 6, 11, 16, 20: {[round(r['all']['running_share'][i], 3) for i in (0, 5, 10, 15, 19)]}"
              f" | accepted share: {[round(r['all']['accepted_share'][i], 3) for i in (0, 5, 10, 15, 19)]}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "reps": args.reps, "nstep": NSTEP, "options": LM, "rev": args.rev, "parent_root": args.parent_root, "parent_rev": args.parent_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
