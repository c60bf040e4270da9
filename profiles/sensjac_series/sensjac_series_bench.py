"""The sensor-band Jacobian over a sun-angle series in one call against the loop of per-step calls it replaces: per
scheme, shape and nt, uniform and ragged columns, levels (0, nz-1), the 13-band set of tools/sensor_bench.py, ntan = 3 shared directions
plus ln LAI plus the leaf angle, all four outputs, the time of
    series     one SensorJacSeriesPlan call: k_colpre<canopy> + k_colsun, the side precomputes once per column, k_sens_jac_series
               (+ k_sens_jac_finish with several band slices)
    loop       nt SensorJacPlan calls, one per sun state, each with its own K0 and side precomputes; the inputs of every step (columns
               with that sun angle, spectra, tangent, plan, workspace, outputs) are prepared outside the timed region
The loop runs in a CHILD process, in the tree named by --loop-root -- any checkout with its library built, meant for the parent commit
(`git worktree add variants/parent <rev> && make -C variants/parent/crt1d_amd/csrc`; variants/ is not tracked) --; without it, in this
tree.  The child measures the loop TWICE per case: `loop_ms` is the first measurement, `loop_ms_again` the second, `loop_spread` their
relative difference -- the noise band a series-against-loop difference has to exceed.  The JSON records the path as given and the
revisions named by --rev and --loop-rev: it says what was measured, not what was meant.  Device events around blocks of --reps calls on
one stream; the median of --blocks blocks is reported, after one warm-up block per case (tools/levels_bench.py).

    python profiles/sensjac_series/sensjac_series_bench.py [--loop-root variants/parent --loop-rev <rev>] [--rev <rev>]
                                                           [--json profiles/sensjac_series/sensjac_series_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:  # (the child: the tree whose package and library it measures)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crt1d_amd import batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402
from sensor_bench import sensor_weights  # noqa: E402

NTAN = 3


def cases(args):
    """The same seeded inputs in both processes; the sun series stays on the host until a case needs it."""
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        sens = batched.SensorSet(sensor_weights(nb, np.random.default_rng(7)))
        g = torch.Generator(device="cuda").manual_seed(1)
        dirs = [torch.rand((NTAN, nb), dtype=torch.float64, device="cuda", generator=g) * 0.2 - 0.1 for _ in range(3)]
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            for nt in (int(v) for v in args.nt.split(",")):
                sun = batched.SunSeries.from_host(synth.make_sun_series(d, nt, seed=4321))
                for scheme in args.schemes.split(","):
                    yield ({"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz], "nt": nt, "nsens": sens.nsens,
                            "ntan": NTAN}, scheme, cols, bands, sun, (0, nz - 1), sens, dirs)
                del sun
                torch.cuda.empty_cache()


def run_series(args):
    rows = []
    for r, scheme, cols, bands, sun, lev, sens, dirs in cases(args):
        tan = batched.leaf_tangent_series(cols, sun, "param")
        plan = batched.SensorJacSeriesPlan(scheme, cols, bands, sun, lev, sens, d_leaf_r=dirs[0], d_leaf_t=dirs[1], d_soil_r=dirs[2], tangent=tan)
        r["series_ms"] = timed(plan, args.blocks, args.reps)
        r["series_kernel"] = plan.last_kernel()
        rows.append(r)
        del plan
        torch.cuda.empty_cache()
    return rows


def run_loop(args):
    """Only what the parent commit has: SensorJacPlan, leaf_tangent."""
    rows = []
    for r, scheme, cols, bands, sun, lev, sens, dirs in cases(args):
        plans = []
        for t in range(sun.nt):
            ct = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla)
            bt = batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), bands.leaf_r, bands.leaf_t, bands.soil_r)
            plans.append(batched.SensorJacPlan(scheme, ct, bt, lev, sens, d_leaf_r=dirs[0], d_leaf_t=dirs[1], d_soil_r=dirs[2],
                                               tangent=batched.leaf_tangent(ct, "param")))

        def loop():
            for p in plans:
                p()

        a, b = timed(loop, args.blocks, args.reps), timed(loop, args.blocks, args.reps)
        r.update(loop_ms=a, loop_ms_again=b, loop_spread=abs(a - b) / min(a, b), step_kernel=plans[-1].last_kernel())
        rows.append(r)
        del plans
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl,g77,bf")
    ap.add_argument("--shapes", default="10000x300x60,2000x2151x60")
    ap.add_argument("--nt", default="8,24")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the loop runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sensjac_series_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_loop(args)}, sys.stdout)
        return
    rows = run_series(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--nt", args.nt, "--blocks", str(args.blocks), "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=1100)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["columns"], r["shape"], r["nt"]) == (l["scheme"], l["columns"], l["shape"], l["nt"])
        r.update(l)
        r["loop_over_series"] = r["loop_ms"] / r["series_ms"]
        lost = r["series_ms"] > max(r["loop_ms"], r["loop_ms_again"]) * (1 + r["loop_spread"])
        r["verdict"] = "loss" if lost else "gain" if r["series_ms"] < min(r["loop_ms"], r["loop_ms_again"]) * (1 - r["loop_spread"]) else "within noise"
        print(f"{r['scheme']:4s} {r['columns']:7s} {'x'.join(map(str, r['shape'])):14s} nt={r['nt']:<3d} series {r['series_ms']:.3f}  loop {r['loop_ms']:.3f} / "
              f"{r['loop_ms_again']:.3f} [{r['loop_over_series']:.2f}x, spread {100 * r['loop_spread']:.1f}%, {r['verdict']}] ms | {r['series_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "rev": args.rev, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
