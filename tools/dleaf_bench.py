"""The leaf-angle derivative of the level spectra against the finite-difference loop it replaces: per scheme and
shape, uniform and ragged columns, levels (0, nz-1), the time of
    dleaf     crt_hip_g_dparam_f64 and one LevelsDleafPlan call: d (I_dr, I_df_d, I_df_u, F) / d g_param, [ncol][2][nb] each; one K0 and
              the side precompute
    fd3       three LevelsPlan calls -- the primal and the central-difference solves g_param (1 +- h) -- each with its own K0: the
              parameter changes K_b, mu_bar and every tau_d quadrature, so nothing of the precompute can be shared; the subtraction that
              forms the difference is NOT timed
The loop runs in a CHILD process, in the tree named by --loop-root -- any checkout with its library built, meant for the commit before the
derivative existed (`git worktree add variants/parent <rev> && make -C variants/parent/crt1d_amd/csrc`; variants/ is not tracked) --;
without it, in this tree.  The JSON records the path as given and the revision named by --loop-rev: it says what was measured, not what
was meant.  Device events around blocks of --reps calls on one stream; the median of --blocks blocks is reported, after one warm-up block
per case (tools/levels_bench.py).

    python tools/dleaf_bench.py [--loop-root variants/parent --loop-rev <rev>] [--json profiles/dleaf/dleaf_bench.json]
"""
import argparse
import ctypes
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
H = 3e-3


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        for uniform in (True, False):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=uniform)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            for scheme in args.schemes.split(","):
                yield {"scheme": scheme, "columns": "uniform" if uniform else "ragged", "shape": [ncol, nb, nz]}, scheme, cols, bands, (0, nz - 1)


def run_dleaf(args):
    from crt1d_amd import _lib

    rows = []
    for r, scheme, cols, bands, lev in cases(args):
        tan = batched.leaf_tangent(cols, "param")
        plan = batched.LevelsDleafPlan(scheme, cols, bands, lev, tan)
        lib, c, st = _lib.load(), cols.c_struct(), torch.cuda.current_stream()

        def dleaf():  # the helper refills the plan's tangent in place, then the plan
            _lib.check(lib.crt_hip_g_dparam_f64(ctypes.byref(c), tan.dg_table.data_ptr(), tan.dg_at_psi.data_ptr(), st.cuda_stream), "crt_hip_g_dparam_f64")
            plan()

        r["dleaf_ms"] = timed(dleaf, args.blocks, args.reps)
        r["dleaf_kernel"] = plan.last_kernel()
        rows.append(r)
        del plan, tan
        torch.cuda.empty_cache()
    return rows


def run_loop(args):
    rows = []
    for r, scheme, cols, bands, lev in cases(args):
        sets = [batched.Columns(cols.psi, cols.lai, cols.g_kind, cols.g_param * s, cols.mla, cols.g_at_psi, cols.g_table) for s in (1.0, 1 + H, 1 - H)]
        plans = [batched.LevelsPlan(scheme, c, bands, lev, keys=KEYS) for c in sets]

        def fd3():
            for p in plans:
                p()

        r["fd3_ms"] = timed(fd3, args.blocks, args.reps)
        r["levels_kernel"] = plans[0].last_kernel()
        rows.append(r)
        del plans, sets
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl,g77,bf,n79,zq")
    ap.add_argument("--shapes", default="10000x300x60,4000x107x60")
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the finite-difference loop runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dleaf_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_loop(args)}, sys.stdout)
        return
    rows = run_dleaf(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--blocks", str(args.blocks), "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["columns"], r["shape"]) == (l["scheme"], l["columns"], l["shape"])
        r.update(l)
        r["fd3_over_dleaf"] = r["fd3_ms"] / r["dleaf_ms"]
        print(f"{r['scheme']:4s} {r['columns']:7s} {'x'.join(map(str, r['shape'])):14s} dleaf {r['dleaf_ms']:.3f}  fd3 {r['fd3_ms']:.3f} [{r['fd3_over_dleaf']:.2f}x] ms"
              f" | {r['dleaf_kernel']} | {r['levels_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "h": H, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
