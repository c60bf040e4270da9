"""One SpectralRetrievalPlan(sun=).step() against one iteration of the best loop that the pieces before the series form allow (DESIGN
section 3.23): per scheme, shape, LAI profile (uniform / ragged) and number of sun states nt, the upwelling spectrum I_df_u at the top of
the canopy of every sun state as the observation, band by band, three shared directions in (leaf_r, leaf_t, soil_r) plus ln LAI plus the
leaf angle, the time of
    plan    SpectralRetrievalPlan(sun=).step(): k_retrieve_apply, the series tangent refill, the canopy / sun / side precomputes +
            k_spec_normal_series + k_spec_normal_series_finish, k_lm_step_normal with one block
    loop    the same iteration from nt per-step SpectralNormalPlans built ONCE on working tensors that crt_hip_retrieve_apply_f64 updates in
            place (one apply per iteration: the working LAI, leaf-angle parameter and optics do not follow the sun), nt tangent refills
            (crt_hip_g_dparam_f64) into nt LeafTangents, the ascending torch sum of the nt (A | g | c2) into preallocated arrays, and
            crt_hip_lm_step_normal_f64 with one block
    normal  k_spec_normal_series + its finish kernel alone (FLAG_SKIP_PRECOMPUTE), on the plan's own arrays
The loop runs in a CHILD process, in the tree named by --loop-root -- any checkout with its library built, meant for the parent commit
(variants/ is not tracked) --; without it, in this tree.  It runs TWICE: the difference of the two medians is the loop's own spread, and a
case counts as a gain or a loss only where the plan lies outside it.  The options keep every column running for all timed steps
(lam_up = 2, lam_max = 1e300).  Device events around blocks of --reps iterations on one stream; the median of --blocks blocks, after one
warm-up block per case (tools/levels_bench.py).

    python profiles/specfit_series/specfit_series_bench.py [--loop-root variants/parent --loop-rev <rev>] [--rev <rev>] [--json <file>]
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
SUMS = ("A", "g", "c2")
NTAN = 3
NPAR = NTAN + 2
LM = dict(lam0=1e-2, lam_up=2.0, lam_down=0.5, lam_max=1e300)


def cases(args):
    """The same inputs in both processes: everything random comes from seeded generators."""
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        rand = lambda *s: torch.rand(s, dtype=torch.float64, device="cuda", generator=g)  # noqa: E731
        dirs = [rand(NTAN, nb) * 0.02 - 0.01 for _ in range(3)]
        truth0 = rand(ncol, NPAR) * 0.2 - 0.1
        for nt in (int(v) for v in args.nts.split(",")):
            psi = torch.deg2rad(torch.linspace(10.0, 70.0, nt, dtype=torch.float64, device="cuda")[None, :] + rand(ncol, nt) * 4.0)
            sun = batched.SunSeries(psi.contiguous(), rand(ncol, nt, nb) * 10.0, rand(ncol, nt, nb) * 5.0)
            for ragged in (False, True):
                d = synth.make_columns(ncol, nb, nz, seed=1234, uniform_dlai=not ragged)
                cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
                truth = truth0.clone()
                truth[:, -1] += cols.g_param
                for scheme in args.schemes.split(","):
                    r = {"scheme": scheme, "lai": "ragged" if ragged else "uniform", "shape": [ncol, nb, nz], "nt": nt, "npar": NPAR}
                    yield r, scheme, cols, bands, sun, (nz - 1,), dirs, truth


def bounds():
    lo = torch.tensor([-1.0] * (NTAN + 1) + [0.2], dtype=torch.float64, device="cuda")
    hi = torch.tensor([1.0] * (NTAN + 1) + [5.0], dtype=torch.float64, device="cuda")
    return lo, hi


class Loop:
    """The host loop on the per-step pieces: everything that can be built once is built once; every tensor the plans read is updated in place
    by the library's own kernels; only the sum over the sun states runs in torch, into arrays of its own."""

    def __init__(self, scheme, cols, bands, sun, lev, dirs, truth):
        ncol, nb, nz, nt = cols.ncol, bands.nb, cols.nz, sun.nt
        self.lib = _lib.load()
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
        self.wb = [batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), z(ncol, nb), z(ncol, nb), z(ncol, nb)) for t in range(1)]
        w = self.wb[0]
        self.wb += [batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), w.leaf_r, w.leaf_t, w.soil_r) for t in range(1, nt)]
        self.wc = [batched.Columns(sun.psi[:, 0].contiguous(), cols.lai.clone(), cols.g_kind, cols.g_param.clone(), cols.mla)]
        self.wc += [batched.Columns(sun.psi[:, t].contiguous(), self.wc[0].lai, cols.g_kind, self.wc[0].g_param, cols.mla) for t in range(1, nt)]
        self.tan = [batched.LeafTangent(z(ncol, _lib.NQ), z(ncol)) for _ in range(nt)]
        self.y = [z(ncol, len(lev), nb) for _ in range(nt)]
        kw = dict(keys=(KEY,), d_leaf_r=dirs[0], d_leaf_t=dirs[1], d_soil_r=dirs[2], lai=True, fwd=True)
        self.plans = [batched.SpectralNormalPlan(scheme, self.wc[t], self.wb[t], lev, {KEY: self.y[t]}, tangent=self.tan[t], **kw) for t in range(nt)]
        assert all(p.y[KEY].data_ptr() == y.data_ptr() for p, y in zip(self.plans, self.y))  # (read where they lie)
        self.sums = {k: torch.zeros_like(self.plans[0].out[k]) for k in SUMS}
        self.lo, self.hi = bounds()
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        self.p, self.p_trial = z(ncol, NPAR), z(ncol, NPAR)
        self.p[:, -1] = cols.g_param
        self.cost = torch.full((ncol,), float("inf"), dtype=torch.float64, device="cuda")
        self.lam = torch.full((ncol,), LM["lam0"], dtype=torch.float64, device="cuda")
        self.A, self.g = z(ncol, NPAR * (NPAR + 1) // 2), z(ncol, NPAR)
        self.status, self.naccept, self.nreject = (torch.zeros((ncol,), dtype=torch.int32, device="cuda") for _ in range(3))
        self.lai_scale = z(ncol)
        self._dirs = _lib.CrtOpticsDirs(NTAN, 0, ptr(dirs[0]), ptr(dirs[1]), ptr(dirs[2]))
        self._keep = (cols, bands, dirs, sun)
        self._ap = _lib.CrtRetrieveApply(ncol, nz, nb, NPAR, NTAN, NTAN + 1, bands.col_stride(ncol), ptr(bands.leaf_r), ptr(bands.leaf_t),
                                         ptr(bands.soil_r), ptr(cols.lai), ptr(self.p_trial), ptr(w.leaf_r), ptr(w.leaf_t), ptr(w.soil_r),
                                         ptr(self.lai_scale), ptr(self.wc[0].lai), ptr(self.wc[0].g_param))
        self._c = [c.c_struct() for c in self.wc]
        self._prob = _lib.CrtLmProblem(ncol, NPAR, LM["lam_up"], LM["lam_down"], 1e-12, LM["lam_max"], 0.0, 0.0, ptr(self.lo), ptr(self.hi), None, None)
        self._blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[ptr(self.sums[k]) for k in SUMS]))
        self._state = _lib.CrtLmState(*[ptr(v) for v in (self.p, self.p_trial, self.cost, self.lam, self.A, self.g, self.status, self.naccept,
                                                          self.nreject)])
        self.p_trial.copy_(truth)  # the observations: the model spectra at the truth
        self.evaluate()
        for t, plan in enumerate(self.plans):
            self.y[t].copy_(plan.out["fwd"][KEY])
            plan.write_fwd = False
        self.p_trial.copy_(self.p)

    def evaluate(self):
        h, ref = torch.cuda.current_stream().cuda_stream, ctypes.byref
        assert self.lib.crt_hip_retrieve_apply_f64(ref(self._ap), ref(self._dirs), h) == 0
        for t, plan in enumerate(self.plans):
            assert self.lib.crt_hip_g_dparam_f64(ref(self._c[t]), self.tan[t].dg_table.data_ptr(), self.tan[t].dg_at_psi.data_ptr(), h) == 0
            plan()
        for k in SUMS:  # ascending, from t = 0's bits
            s = self.sums[k]
            if len(self.plans) == 1:
                s.copy_(self.plans[0].out[k])
                continue
            torch.add(self.plans[0].out[k], self.plans[1].out[k], out=s)
            for plan in self.plans[2:]:
                s.add_(plan.out[k])

    def __call__(self):
        self.evaluate()
        st = self.lib.crt_hip_lm_step_normal_f64(ctypes.byref(self._prob), self._blk, 1, ctypes.byref(self._state),
                                                 torch.cuda.current_stream().cuda_stream)
        assert st == 0


def run_plan(args):
    rows = []
    for r, scheme, cols, bands, sun, lev, dirs, truth in cases(args):
        ncol, nb, nt = cols.ncol, bands.nb, sun.nt
        y = {KEY: torch.zeros((ncol, nt, len(lev), nb), dtype=torch.float64, device="cuda")}
        lo, hi = bounds()
        plan = batched.SpectralRetrievalPlan(scheme, cols, bands, lev, y, keys=(KEY,), sun=sun, d_leaf_r=dirs[0], d_leaf_t=dirs[1],
                                             d_soil_r=dirs[2], lai=True, leaf=True, lo=lo, hi=hi, **LM)
        assert plan.y[KEY].data_ptr() == y[KEY].data_ptr()  # (read where it lies)
        plan.p.copy_(truth)  # the observations: the model spectra at the truth
        y[KEY].copy_(plan.fitted()[KEY])
        plan.reset()
        r["plan_ms"] = timed(plan.step, args.blocks, args.reps)
        r["normal_ms"] = timed(lambda: plan.normal(flags=_lib.FLAG_SKIP_PRECOMPUTE), args.blocks, args.reps)
        r["kernel"] = plan.normal.last_kernel()
        res = plan.result()
        r["running_after"] = int((res["status"] == batched.LM_RUNNING).sum())
        r["cost_max"] = float(res["cost"].max())
        print(f"plan {r['scheme']} {r['lai']} {r['shape']} nt={nt}: {r['plan_ms']:.3f} ms", file=sys.stderr, flush=True)
        rows.append(r)
        del plan
        torch.cuda.empty_cache()
    return rows


def run_loop(args):
    rows = []
    for r, *case in cases(args):
        r["loop_ms"] = []
        for _ in range(2):
            loop = Loop(*case)
            r["loop_ms"].append(timed(loop, args.blocks, args.reps))
            r["loop_running_after"] = int((loop.status == 0).sum())
            r["loop_cost_max"] = float(loop.cost.max())
            del loop
            torch.cuda.empty_cache()
        print(f"loop {r['scheme']} {r['lai']} {r['shape']} nt={r['nt']}: {r['loop_ms']} ms", file=sys.stderr, flush=True)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="2s,bl")
    ap.add_argument("--shapes", default="10000x300x60,2000x2151x60")
    ap.add_argument("--nts", default="8,24")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-root", default=None, help="tree (package + built library) the loop runs in: the parent commit")
    ap.add_argument("--loop-rev", default=None, help="git revision of the --loop-root tree, recorded in the JSON as given")
    ap.add_argument("--rev", default=None, help="git revision of this tree, recorded in the JSON as given")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="main", choices=["main", "loop"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "specfit_series_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_loop(args)}, sys.stdout)
        return
    rows = run_plan(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--nts", args.nts, "--blocks", str(args.blocks), "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["lai"], r["shape"], r["nt"]) == (l["scheme"], l["lai"], l["shape"], l["nt"])
        r.update(l)
        lo, hi = min(r["loop_ms"]), max(r["loop_ms"])
        r["verdict"] = "gain" if r["plan_ms"] < lo else "loss" if r["plan_ms"] > hi else "inside the loop's spread"
        r["loop_over_plan"] = [v / r["plan_ms"] for v in r["loop_ms"]]
        print(f"{r['scheme']:3s} {r['lai']:8s} {'x'.join(map(str, r['shape'])):14s} nt={r['nt']:<3d} plan {r['plan_ms']:.3f}  loop {lo:.3f} .. {hi:.3f} ms "
              f"[{r['verdict']}]  k_spec_normal_series {r['normal_ms']:.4f} ms | {r['kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "rev": args.rev, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
