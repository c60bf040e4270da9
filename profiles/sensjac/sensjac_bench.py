"""The Jacobian of the sensor-band sums in one kernel against the composition it replaces: per scheme and shape,
uniform and ragged columns, levels (0, nz-1), the 13-band set of tools/sensor_bench.py, ntan = 3 shared directions plus ln LAI plus the
leaf angle, all four outputs, the time of
    fused      one SensorJacPlan call: K0, the side precomputes, k_sens_jac (+ k_sens_jac_finish with several band slices)
    compose    sensor_jvp + sensor_dlai + sensor_dleaf: three plans with a K0 each, eleven derivative arrays, the (ncol, nsel, ntan, nb)
               intermediate of sensor_jvp and the einsum of each with the dense (nsens, nb) weights, side by side into one array per key
The tangent along g_param is formed once outside both.  The composition runs in a CHILD process, in the tree named by --loop-root -- any
checkout with its library built, meant for the parent commit (`git worktree add variants/parent <rev> && make -C
variants/parent/crt1d_amd/csrc`; variants/ is not tracked) --; without it, in this tree.  The JSON records the path as given and the
revisions named by --rev and --loop-rev: it says what was measured, not what was meant.  Device events around blocks of --reps calls on
one stream; the median of --blocks blocks is reported, after one warm-up block per case (tools/levels_bench.py).

    python profiles/sensjac/sensjac_bench.py [--loop-root variants/parent --loop-rev <rev>] [--rev <rev>] [--json profiles/sensjac/sensjac_bench.json]
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

KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
JAC_KEYS = ("I_df_d", "I_df_u", "F")
NTAN = 3


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        sens = batched.SensorSet(sensor_weights(nb, np.random.default_rng(7)))
        g = torch.Generator(device="cuda").manual_seed(1)
        dirs = [torch.rand((NTAN, nb), dtype=torch.float64, device="cuda", generator=g) * 0.2 - 0.1 for _ in range(3)]
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            tan = batched.leaf_tangent(cols, "param")
            for scheme in args.schemes.split(","):
                yield ({"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz], "nsens": sens.nsens, "ntan": NTAN},
                       scheme, cols, bands, (0, nz - 1), sens, dirs, tan)


def run_fused(args):
    rows = []
    for r, scheme, cols, bands, lev, sens, dirs, tan in cases(args):
        plan = batched.SensorJacPlan(scheme, cols, bands, lev, sens, d_leaf_r=dirs[0], d_leaf_t=dirs[1], d_soil_r=dirs[2], tangent=tan)
        r["fused_ms"] = timed(plan, args.blocks, args.reps)
        r["fused_kernel"] = plan.last_kernel()
        rows.append(r)
        del plan
        torch.cuda.empty_cache()
    return rows


def run_compose(args):
    rows = []
    for r, scheme, cols, bands, lev, sens, dirs, tan in cases(args):
        def compose():
            a = batched.sensor_jvp(scheme, cols, bands, lev, sens, *dirs)
            b = batched.sensor_dlai(scheme, cols, bands, lev, sens)
            c = batched.sensor_dleaf(scheme, cols, bands, lev, tan, sens)
            z = torch.zeros_like(a["F"])  # (I_dr does not depend on the optics)
            return {k: torch.cat([a.get(k, z), b[k][..., None], c[k][..., None]], dim=-1) for k in KEYS}

        r["compose_ms"] = timed(compose, args.blocks, args.reps)
        rows.append(r)
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl,g77,bf")
    ap.add_argument("--shapes", default="10000x300x60,2000x2151x60")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the composition runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sensjac_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_compose(args)}, sys.stdout)
        return
    rows = run_fused(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--blocks", str(args.blocks), "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["columns"], r["shape"]) == (l["scheme"], l["columns"], l["shape"])
        r.update(l)
        r["compose_over_fused"] = r["compose_ms"] / r["fused_ms"]
        print(f"{r['scheme']:4s} {r['columns']:7s} {'x'.join(map(str, r['shape'])):14s} fused {r['fused_ms']:.3f}  compose {r['compose_ms']:.3f} "
              f"[{r['compose_over_fused']:.2f}x] ms | {r['fused_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "rev": args.rev, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
