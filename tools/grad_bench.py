"""The gradient of a weighted sum of the level spectra against the composition it replaces: per scheme and shape,
uniform and ragged columns, levels (0, nz-1), all five outputs (leaf_r, leaf_t, soil_r [ncol][nb]; lai, leaf [ncol]), the time of
    grad       one LevelsGradPlan call: K0, the side precomputes, k_grad (+ k_grad_finish with several band slices)
    compose    LevelsJacPlan + LevelsDlaiPlan + LevelsDleafPlan, each with its own K0, writing eleven derivative arrays, and the torch
               contraction that reads them back with the weights: per array a product and a sum (--contract mulsum, the default) or an
               einsum (--contract einsum: torch runs "crb,crb->cb" as a batched matrix product with an inner dimension of nsel, far
               slower at two levels), summed per output
The tangent along g_param is formed once outside both (it does not depend on the weights).  The composition runs in a CHILD process, in the
tree named by --loop-root -- any checkout with its library built, meant for the commit before the entry existed (`git worktree add
variants/parent <rev> && make -C variants/parent/crt1d_amd/csrc`; variants/ is not tracked) --; without it, in this tree.  The JSON
records the path as given and the revisions named by --rev and --loop-rev: it says what was measured, not what was meant.  Device events
around blocks of --reps calls on one stream; the median of --blocks blocks is reported, after one warm-up block per case
(tools/levels_bench.py).

    python tools/grad_bench.py [--loop-root variants/parent --loop-rev <rev>] [--rev <rev>] [--json profiles/grad/grad_bench.json]
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

from crt1d_amd import batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402

KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
JAC_KEYS = ("I_df_d", "I_df_u", "F")


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            g = torch.Generator(device="cuda").manual_seed(1)
            w = {k: torch.rand((ncol, 2, nb), dtype=torch.float64, device="cuda", generator=g) * 2 - 1 for k in KEYS}
            tan = batched.leaf_tangent(cols, "param")
            for scheme in args.schemes.split(","):
                yield {"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz]}, scheme, cols, bands, (0, nz - 1), w, tan


def run_grad(args):
    rows = []
    for r, scheme, cols, bands, lev, w, tan in cases(args):
        plan = batched.LevelsGradPlan(scheme, cols, bands, lev, w, tangent=tan)
        r["grad_ms"] = timed(plan, args.blocks, args.reps)
        r["grad_kernel"] = plan.last_kernel()
        rows.append(r)
        del plan
        torch.cuda.empty_cache()
    return rows


def run_compose(args):
    rows = []
    for r, scheme, cols, bands, lev, w, tan in cases(args):
        jac = batched.LevelsJacPlan(scheme, cols, bands, lev)
        dlai = batched.LevelsDlaiPlan(scheme, cols, bands, lev)
        dleaf = batched.LevelsDleafPlan(scheme, cols, bands, lev, tan)

        if args.contract == "einsum":
            opt = lambda a, b: torch.einsum("crb,crb->cb", a, b)  # noqa: E731
            col = lambda a, b: torch.einsum("crb,crb->c", a, b)  # noqa: E731
        else:
            opt = lambda a, b: (a * b).sum(1)  # noqa: E731
            col = lambda a, b: (a * b).sum((1, 2))  # noqa: E731

        def compose():
            J, A, B = jac(), dlai(), dleaf()
            out = {}
            for p, name in enumerate(("leaf_r", "leaf_t", "soil_r")):
                out[name] = sum(opt(w[k], J[k][:, :, p, :]) for k in JAC_KEYS)
            out["lai"] = sum(col(w[k], A[k]) for k in KEYS)
            out["leaf"] = sum(col(w[k], B[k]) for k in KEYS)
            return out

        r["compose_ms"] = timed(compose, args.blocks, args.reps)
        r["compose_last_kernel"] = dleaf.last_kernel()
        rows.append(r)
        del jac, dlai, dleaf
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl,g77,bf")
    ap.add_argument("--shapes", default="10000x300x60,4000x107x60")
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the composition runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--contract", default="mulsum", choices=["mulsum", "einsum"],
                    help="the composition's torch contraction: a product and a sum per derivative array, or an einsum per array")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grad_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_compose(args)}, sys.stdout)
        return
    rows = run_grad(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--blocks", str(args.blocks), "--reps", str(args.reps), "--contract", args.contract]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["columns"], r["shape"]) == (l["scheme"], l["columns"], l["shape"])
        r.update(l)
        r["compose_over_grad"] = r["compose_ms"] / r["grad_ms"]
        print(f"{r['scheme']:4s} {r['columns']:7s} {'x'.join(map(str, r['shape'])):14s} grad {r['grad_ms']:.3f}  compose {r['compose_ms']:.3f} "
              f"[{r['compose_over_grad']:.2f}x] ms | {r['grad_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "contract": args.contract, "rev": args.rev, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
