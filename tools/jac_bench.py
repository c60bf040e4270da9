"""The Jacobian of the level spectra against the finite-difference loop it replaces: per scheme and shape, uniform
and ragged columns, levels (0, nz-1), the time of
    jac       one LevelsJacPlan call: d (I_df_d, I_df_u, F) / d (leaf_r, leaf_t, soil_r), [ncol][2][3][nb] each; one K0
    fd7       seven LevelsPlan calls on the same three spectra -- the primal and the six central-difference solves leaf_r +- h, leaf_t +- h,
              soil_r +- h -- each with its own K0, as a user of LevelsPlan has it; the subtractions that form the differences are NOT timed
    fd7_skip  the same with K0 once and CRT_FLAG_SKIP_PRECOMPUTE on the six others (the most a careful user could save)
The loop runs in a CHILD process, in the tree named by --loop-root -- any checkout with its library built, meant for the commit before the
Jacobian existed (`git worktree add variants/parent <rev> && make -C variants/parent/crt1d_amd/csrc`; variants/ is not tracked) --; without
it, in this tree.  The JSON records the path as given and the revision named by --loop-rev: it says what was measured, not what was meant.  Device events around blocks of --reps calls on one stream; the median of --blocks
blocks is reported, after one warm-up block per case (tools/levels_bench.py).

    python tools/jac_bench.py [--loop-root variants/parent --loop-rev <rev>] [--json profiles/jac/jac_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (the child: the tree whose package and library it measures)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from crt1d_amd import _lib, batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402

KEYS = ("I_df_d", "I_df_u", "F")
H = 1e-3


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            for scheme in args.schemes.split(","):
                yield {"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz]}, scheme, cols, bands, (0, nz - 1)


def run_jac(args):
    rows = []
    for r, scheme, cols, bands, lev in cases(args):
        plan = batched.LevelsJacPlan(scheme, cols, bands, lev)
        r["jac_ms"] = timed(plan, args.blocks, args.reps)
        r["jac_kernel"] = plan.last_kernel()
        rows.append(r)
        del plan
        torch.cuda.empty_cache()
    return rows


def run_loop(args):
    rows = []
    for r, scheme, cols, bands, lev in cases(args):
        sets = [bands]
        for name in ("leaf_r", "leaf_t", "soil_r"):
            for sgn in (1.0, -1.0):
                kw = {k: getattr(bands, k) for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")}
                kw[name] = kw[name] + sgn * H
                sets.append(batched.Bands(**kw))
        plans = [batched.LevelsPlan(scheme, cols, b, lev, keys=KEYS) for b in sets]
        shared = [plans[0]] + [batched.LevelsPlan(scheme, cols, b, lev, keys=KEYS, workspace=plans[0].workspace) for b in sets[1:]]

        def fd7():
            for p in plans:
                p()

        def fd7_skip():
            shared[0]()
            for p in shared[1:]:
                p(flags=_lib.FLAG_SKIP_PRECOMPUTE)

        r["fd7_ms"] = timed(fd7, args.blocks, args.reps)
        r["fd7_skip_ms"] = timed(fd7_skip, args.blocks, args.reps)
        r["levels_kernel"] = plans[0].last_kernel()
        rows.append(r)
        del plans, shared, sets
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,zq,n79")
    ap.add_argument("--shapes", default="10000x300x60,4000x107x60")
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the finite-difference loop runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jac_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_loop(args)}, sys.stdout)
        return
    rows = run_jac(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes, "--blocks", str(args.blocks),
           "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["columns"], r["shape"]) == (l["scheme"], l["columns"], l["shape"])
        r.update(l)
        r["fd7_over_jac"] = r["fd7_ms"] / r["jac_ms"]
        r["fd7_skip_over_jac"] = r["fd7_skip_ms"] / r["jac_ms"]
        print(f"{r['scheme']:4s} {r['columns']:7s} {'x'.join(map(str, r['shape'])):14s} jac {r['jac_ms']:.3f}  fd7 {r['fd7_ms']:.3f} [{r['fd7_over_jac']:.2f}x]"
              f"  fd7_skip {r['fd7_skip_ms']:.3f} [{r['fd7_skip_over_jac']:.2f}x] ms | {r['jac_kernel']} | {r['levels_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "h": H, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
