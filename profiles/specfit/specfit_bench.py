"""One SpectralRetrievalPlan.step() against one iteration of the best loop that the pieces before it allow: per
scheme, shape and LAI profile (uniform / ragged), the upwelling spectrum I_df_u at the top of the canopy as the observation, band by band,
three shared directions in (leaf_r, leaf_t, soil_r) plus ln LAI plus the leaf angle, the time of
    plan    SpectralRetrievalPlan.step(): k_retrieve_apply, k_g_dparam, the column precompute + k_spec_normal, k_lm_step_normal
    loop    the same iteration from LevelsJacPlan, LevelsDlaiPlan, LevelsDleafPlan and LevelsPlan built ONCE on working tensors that
            crt_hip_retrieve_apply_f64 and crt_hip_g_dparam_f64 update in place (the forward plan on the Jacobian plan's workspace with
            FLAG_SKIP_PRECOMPUTE), a torch contraction of the tangents with the directions into J [ncol][nsel * nb][npar], and
            crt_hip_lm_step_f64 with nrow = nsel * nb reading that J
    normal, step   k_spec_normal (FLAG_SKIP_PRECOMPUTE: the kernel without the column precompute) and k_lm_step_normal alone, on the plan's own
            arrays
The loop runs in a CHILD process, in the tree named by --loop-root -- any checkout with its library built, meant for the parent commit
(variants/ is not tracked) --; without it, in this tree.  It runs TWICE: the difference of the two medians is the loop's own spread, and a
case counts as a gain or a loss only where the plan lies outside it.  The options keep every column running for all timed steps
(lam_up = 2, lam_max = 1e300).  Device events around blocks of --reps iterations on one stream; the median of --blocks blocks, after one
warm-up block per case (tools/levels_bench.py).

    python profiles/specfit/specfit_bench.py [--loop-root variants/parent --loop-rev <rev>] [--rev <rev>] [--json profiles/specfit/specfit_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:  # (the child: the tree whose package and library it measures)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from crt1d_amd import _lib, batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402

KEY = "I_df_u"
NTAN = 3
NPAR = NTAN + 2
LM = dict(lam0=1e-2, lam_up=2.0, lam_down=0.5, lam_max=1e300)


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        dirs = [torch.rand((NTAN, nb), dtype=torch.float64, device="cuda", generator=g) * 0.02 - 0.01 for _ in range(3)]
        truth0 = torch.rand((ncol, NPAR), dtype=torch.float64, device="cuda", generator=g) * 0.2 - 0.1
        for ragged in (False, True):
            d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=not ragged)
            cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
            truth = truth0.clone()
            truth[:, -1] += cols.g_param
            for scheme in args.schemes.split(","):
                r = {"scheme": scheme, "lai": "ragged" if ragged else "uniform", "shape": [ncol, nb, nz], "npar": NPAR}
                yield r, scheme, cols, bands, (nz - 1,), dirs, truth


def bounds():
    lo = torch.tensor([-1.0] * (NTAN + 1) + [0.2], dtype=torch.float64, device="cuda")
    hi = torch.tensor([1.0] * (NTAN + 1) + [5.0], dtype=torch.float64, device="cuda")
    return lo, hi


class Loop:
    """The host loop: everything that can be built once is built once; every tensor the plans read is updated in place by the library's
    own apply kernel; only the contraction to J runs in torch."""

    def __init__(self, scheme, cols, bands, lev, dirs, truth):
        ncol, nb, nz = cols.ncol, bands.nb, cols.nz
        self.lib = _lib.load()
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
        rows = lambda v: v.expand(ncol, -1).contiguous()  # noqa: E731
        self.wb = batched.Bands(rows(bands.I_dr0), rows(bands.I_df0), z(ncol, nb), z(ncol, nb), z(ncol, nb))
        self.wc = batched.Columns(cols.psi, cols.lai.clone(), cols.g_kind, cols.g_param.clone(), cols.mla, cols.g_at_psi, cols.g_table)
        self.tan = batched.LeafTangent(z(ncol, _lib.NQ), z(ncol))
        self.jac = batched.LevelsJacPlan(scheme, self.wc, self.wb, lev, keys=(KEY,))
        self.dlai = batched.LevelsDlaiPlan(scheme, self.wc, self.wb, lev, keys=(KEY,))
        self.dleaf = batched.LevelsDleafPlan(scheme, self.wc, self.wb, lev, tangent=self.tan, keys=(KEY,))
        self.fwd = batched.LevelsPlan(scheme, self.wc, self.wb, lev, keys=(KEY,), workspace=self.jac.workspace)
        self.D = torch.stack(dirs)  # (leaf_r | leaf_t | soil_r, ntan, nb)
        self.lo, self.hi = bounds()
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        self.p, self.p_trial = z(ncol, NPAR), z(ncol, NPAR)
        self.p[:, -1] = cols.g_param
        self.cost = torch.full((ncol,), float("inf"), dtype=torch.float64, device="cuda")
        self.lam = torch.full((ncol,), LM["lam0"], dtype=torch.float64, device="cuda")
        self.A, self.g = z(ncol, NPAR * (NPAR + 1) // 2), z(ncol, NPAR)
        self.status, self.naccept, self.nreject = (torch.zeros((ncol,), dtype=torch.int32, device="cuda") for _ in range(3))
        self.lai_scale = z(ncol)
        self.J = z(ncol, nb, NPAR)
        self._dirs = _lib.CrtOpticsDirs(NTAN, 0, ptr(dirs[0]), ptr(dirs[1]), ptr(dirs[2]))
        self._keep = (cols, bands, dirs)
        self._ap = _lib.CrtRetrieveApply(ncol, nz, nb, NPAR, NTAN, NTAN + 1, bands.col_stride(ncol), ptr(bands.leaf_r), ptr(bands.leaf_t),
                                         ptr(bands.soil_r), ptr(cols.lai), ptr(self.p_trial), ptr(self.wb.leaf_r),
                                         ptr(self.wb.leaf_t), ptr(self.wb.soil_r), ptr(self.lai_scale), ptr(self.wc.lai), ptr(self.wc.g_param))
        self._c = self.wc.c_struct()
        self._prob = _lib.CrtLmProblem(ncol, NPAR, LM["lam_up"], LM["lam_down"], 1e-12, LM["lam_max"], 0.0, 0.0, ptr(self.lo), ptr(self.hi), None, None)
        self._state = _lib.CrtLmState(*[ptr(v) for v in (self.p, self.p_trial, self.cost, self.lam, self.A, self.g, self.status, self.naccept,
                                                          self.nreject)])
        self.p_trial.copy_(truth)
        self.evaluate()
        self.y = self.fwd.out[KEY].clone()
        self.p_trial.copy_(self.p)
        self._obs = (_lib.CrtLmObs * 1)(_lib.CrtLmObs(nb, ptr(self.fwd.out[KEY]), ptr(self.J), ptr(self.y), None))

    def evaluate(self):
        h, ref = torch.cuda.current_stream().cuda_stream, ctypes.byref
        assert self.lib.crt_hip_retrieve_apply_f64(ref(self._ap), ref(self._dirs), h) == 0
        assert self.lib.crt_hip_g_dparam_f64(ref(self._c), self.tan.dg_table.data_ptr(), self.tan.dg_at_psi.data_ptr(), h) == 0
        j = self.jac()[KEY]
        self.fwd(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        a, b = self.dlai()[KEY], self.dleaf()[KEY]
        self.J[:, :, :NTAN] = torch.einsum("cqb,qkb->cbk", j[:, 0], self.D)
        self.J[:, :, NTAN] = a[:, 0]
        self.J[:, :, NTAN + 1] = b[:, 0]

    def __call__(self):
        self.evaluate()
        st = self.lib.crt_hip_lm_step_f64(ctypes.byref(self._prob), self._obs, 1, ctypes.byref(self._state), torch.cuda.current_stream().cuda_stream)
        assert st == 0


def run_plan(args):
    rows = []
    for r, scheme, cols, bands, lev, dirs, truth in cases(args):
        loop = Loop(scheme, cols, bands, lev, dirs, truth)  # (for the observations only)
        y = {KEY: loop.y}
        del loop
        lo, hi = bounds()
        plan = batched.SpectralRetrievalPlan(scheme, cols, bands, lev, y, keys=(KEY,), d_leaf_r=dirs[0], d_leaf_t=dirs[1],
                                             d_soil_r=dirs[2], lai=True, leaf=True, lo=lo, hi=hi, **LM)
        r["plan_ms"] = timed(plan.step, args.blocks, args.reps)
        lib, h = plan.lib, torch.cuda.current_stream().cuda_stream
        r["normal_ms"] = timed(lambda: plan.normal(flags=_lib.FLAG_SKIP_PRECOMPUTE), args.blocks, args.reps)
        r["kernel"] = plan.normal.last_kernel()
        r["step_ms"] = timed(lambda: lib.crt_hip_lm_step_normal_f64(ctypes.byref(plan._prob), plan._blk, 1, ctypes.byref(plan._state), h),
                             args.blocks, args.reps)
        res = plan.result()
        r["running_after"] = int((res["status"] == batched.LM_RUNNING).sum())
        rows.append(r)
        del plan
        torch.cuda.empty_cache()
    return rows


def run_loop(args):
    rows = []
    for r, *case in cases(args):
        r["loop_ms"] = [timed(Loop(*case), args.blocks, args.reps) for _ in range(2)]
        rows.append(r)
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl")
    ap.add_argument("--shapes", default="10000x300x60,2000x2151x60")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the loop runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "specfit_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_loop(args)}, sys.stdout)
        return
    rows = run_plan(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--blocks", str(args.blocks), "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["lai"], r["shape"]) == (l["scheme"], l["lai"], l["shape"])
        r.update(l)
        lo, hi = min(r["loop_ms"]), max(r["loop_ms"])
        r["verdict"] = "gain" if r["plan_ms"] < lo else "loss" if r["plan_ms"] > hi else "inside the loop's spread"
        r["loop_over_plan"] = [v / r["plan_ms"] for v in r["loop_ms"]]
        print(f"{r['scheme']:3s} {r['lai']:8s} {'x'.join(map(str, r['shape'])):14s} plan {r['plan_ms']:.3f}  loop {lo:.3f} .. {hi:.3f} ms "
              f"[{r['verdict']}]  k_spec_normal {r['normal_ms']:.4f}  k_lm_step_normal {r['step_ms']:.4f} ms | {r['kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "rev": args.rev, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
