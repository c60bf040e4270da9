"""One RetrievalPlan.step() against one iteration of the best loop that the pieces before it allow: per scheme and
shape, per step and over a series of nt = 8 sun states, levels (0, nz-1), the 13-band set of tools/sensor_bench.py, all four outputs as
observations, three shared directions in (leaf_r, leaf_t, soil_r) plus ln LAI plus the leaf angle, the time of
    plan    RetrievalPlan.step(): k_retrieve_apply, k_g_dparam, the Jacobian call, the forward sums on its workspace, k_lm_step
    loop    the same iteration from SensorJacPlan + SensorLevelsPlan built ONCE on working tensors that torch updates in place
            (addmm / mul / copy_ with out=), crt_hip_g_dparam_f64 into the plan's tangent, gauss_newton_step, torch.where for accept /
            reject: the same algorithm (evaluation at the trial point, the normal equations of the accepted point kept as J and r)
    lm, apply   k_lm_step and k_retrieve_apply alone, on the plan's own arrays
The loop runs in a CHILD process, in the tree named by --loop-root -- any checkout with its library built, meant for the parent commit
(variants/ is not tracked) --; without it, in this tree.  It runs TWICE: the difference of the two medians is the loop's own spread, and a
case counts as a gain or a loss only where the plan lies outside it.  The JSON records the path as given and the revisions named by --rev
and --loop-rev.  The options keep every column running for all timed steps (lam_up = 2, lam_max = 1e300): a finished column would leave
k_lm_step at once.  Device events around blocks of --reps iterations on one stream; the median of --blocks blocks, after one warm-up
block per case (tools/levels_bench.py).

    python profiles/retrieve/retrieve_bench.py [--loop-root variants/parent --loop-rev <rev>] [--rev <rev>] [--json profiles/retrieve/retrieve_bench.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crt1d_amd import _lib, batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402
from sensor_bench import sensor_weights  # noqa: E402

KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
NTAN, NT = 3, 8
LM = dict(lam0=1e-2, lam_up=2.0, lam_down=0.5, lam_max=1e300)


def cases(args):
    for shape in args.shapes.split(","):
        ncol, nb, nz = (int(v) for v in shape.split("x"))
        sens = batched.SensorSet(sensor_weights(nb, np.random.default_rng(7)))
        g = torch.Generator(device="cuda").manual_seed(1)
        dirs = [torch.rand((NTAN, nb), dtype=torch.float64, device="cuda", generator=g) * 0.02 - 0.01 for _ in range(3)]
        d = synth.make_columns(ncol, nb, nz, seed=1234)
        cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
        truth = torch.rand((ncol, NTAN + 2), dtype=torch.float64, device="cuda", generator=g) * 0.2 - 0.1
        truth[:, -1] += cols.g_param
        for series in (False, True):
            sun = batched.SunSeries.from_host(synth.make_sun_series(d, NT)) if series else None
            for scheme in args.schemes.split(","):
                r = {"scheme": scheme, "mode": f"series nt={NT}" if series else "step", "shape": [ncol, nb, nz], "nsens": sens.nsens, "npar": NTAN + 2}
                yield r, scheme, cols, bands, sun, (0, nz - 1), sens, dirs, truth


class Loop:
    """The host loop: everything that can be built once is built once; every tensor the plans read is updated in place."""

    def __init__(self, scheme, cols, bands, sun, lev, sens, dirs, truth):
        ncol, nb = cols.ncol, bands.nb
        self.lib, self.sun = _lib.load(), sun
        self.base, self.dirs, self.lai0 = bands, dirs, cols.lai
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
        rows = lambda v: v.expand(ncol, -1).contiguous()  # noqa: E731
        self.wb = batched.Bands(rows(bands.I_dr0), rows(bands.I_df0), z(ncol, nb), z(ncol, nb), z(ncol, nb))
        self.wc = batched.Columns(cols.psi, cols.lai.clone(), cols.g_kind, cols.g_param.clone(), cols.mla, cols.g_at_psi, cols.g_table)
        kw = dict(d_leaf_r=dirs[0], d_leaf_t=dirs[1], d_soil_r=dirs[2])
        if sun is None:
            self.tan = batched.LeafTangent(z(ncol, _lib.NQ), z(ncol))
            self.jac = batched.SensorJacPlan(scheme, self.wc, self.wb, lev, sens, tangent=self.tan, **kw)
            self.fwd = batched.SensorLevelsPlan(scheme, self.wc, self.wb, lev, sens, workspace=self.jac.workspace)
        else:
            self.tan = batched.LeafTangentSeries(z(ncol, _lib.NQ), z(ncol, sun.nt))
            self.jac = batched.SensorJacSeriesPlan(scheme, self.wc, self.wb, sun, lev, sens, tangent=self.tan, **kw)
            self.fwd = batched.SensorLevelsSeriesPlan(scheme, self.wc, self.wb, sun, lev, sens, workspace=self.jac.workspace)
        self._c = self.wc.c_struct()
        self._s = None if sun is None else sun.c_struct()
        self.lo = torch.tensor([-1.0] * (NTAN + 1) + [0.2], dtype=torch.float64, device="cuda")
        self.hi = torch.tensor([1.0] * (NTAN + 1) + [5.0], dtype=torch.float64, device="cuda")
        self.p = z(ncol, NTAN + 2)
        self.p[:, -1] = cols.g_param
        self.trial = truth.clone()
        self.y = self.evaluate()[0].clone()
        self.trial = self.p.clone()
        self.cost = torch.full((ncol,), float("inf"), dtype=torch.float64, device="cuda")
        self.lam = torch.full((ncol,), LM["lam0"], dtype=torch.float64, device="cuda")
        self.r, self.J = torch.zeros_like(self.y), z(ncol, self.y.shape[1], NTAN + 2)

    def evaluate(self):
        t, b, wb, wc = self.trial, self.base, self.wb, self.wc
        for n, d in zip(("leaf_r", "leaf_t", "soil_r"), self.dirs):
            torch.addmm(getattr(b, n).expand(t.shape[0], -1), t[:, :NTAN], d, out=getattr(wb, n))
        torch.mul(self.lai0, torch.exp(t[:, NTAN])[:, None], out=wc.lai)
        wc.g_param.copy_(t[:, NTAN + 1])
        h = torch.cuda.current_stream().cuda_stream
        if self.sun is None:
            st = self.lib.crt_hip_g_dparam_f64(ctypes.byref(self._c), self.tan.dg_table.data_ptr(), self.tan.dg_at_psi.data_ptr(), h)
        else:
            st = self.lib.crt_hip_g_dparam_series_f64(ctypes.byref(self._c), ctypes.byref(self._s), self.tan.dg_table.data_ptr(),
                                                      self.tan.dg_at_psi.data_ptr(), h)
        assert st == 0
        J = self.jac()
        f = self.fwd(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        n = t.shape[0]
        return torch.cat([f[k].reshape(n, -1) for k in KEYS], dim=1), torch.cat([J[k].reshape(n, -1, NTAN + 2) for k in KEYS], dim=1)

    def __call__(self):
        f, J = self.evaluate()
        r = f - self.y
        cost = 0.5 * (r * r).sum(1)
        better = cost < self.cost
        self.p = torch.where(better[:, None], self.trial, self.p)
        self.r = torch.where(better[:, None], r, self.r)
        self.J = torch.where(better[:, None, None], J, self.J)
        self.cost = torch.where(better, cost, self.cost)
        self.lam = torch.where(better, self.lam * LM["lam_down"], self.lam * LM["lam_up"])
        self.trial = torch.minimum(torch.maximum(self.p + batched.gauss_newton_step(self.J, self.r, damping=self.lam), self.lo), self.hi)


def run_plan(args):
    rows = []
    for r, scheme, cols, bands, sun, lev, sens, dirs, truth in cases(args):
        loop = Loop(scheme, cols, bands, sun, lev, sens, dirs, truth)  # (for the observations only)
        nt = () if sun is None else (sun.nt,)
        y, o = {}, 0
        for k in KEYS:
            y[k] = loop.y[:, o:o + loop.y.shape[1] // 4].reshape(cols.ncol, *nt, 2, sens.nsens)
            o += loop.y.shape[1] // 4
        plan = batched.RetrievalPlan(scheme, cols, bands, lev, sens, y, keys=KEYS, sun=sun, d_leaf_r=dirs[0], d_leaf_t=dirs[1], d_soil_r=dirs[2],
                                     lai=True, leaf=True, lo=loop.lo, hi=loop.hi, **LM)
        del loop
        r["plan_ms"] = timed(plan.step, args.blocks, args.reps)
        r["jac_kernel"] = plan.jac.last_kernel() if plan.jac._composed else (plan.jac(), plan.jac.last_kernel())[1]
        lib, h = plan.lib, torch.cuda.current_stream().cuda_stream
        r["lm_ms"] = timed(lambda: lib.crt_hip_lm_step_f64(ctypes.byref(plan._prob), plan._obs, len(KEYS), ctypes.byref(plan._state), h),
                           args.blocks, args.reps)
        r["apply_ms"] = timed(lambda: lib.crt_hip_retrieve_apply_f64(ctypes.byref(plan._ap), ctypes.byref(plan._dirs), h), args.blocks, args.reps)
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
    assert torch.cuda.is_available(), "retrieve_bench needs a GPU"
    if args.role == "loop":
        json.dump({"rows": run_loop(args)}, sys.stdout)
        return
    rows = run_plan(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "loop", "--root", args.loop_root or ROOT, "--schemes", args.schemes, "--shapes", args.shapes,
           "--blocks", str(args.blocks), "--reps", str(args.reps)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)  # a fresh process: its own library
    loop = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for r, l in zip(rows, loop["rows"]):
        assert (r["scheme"], r["mode"], r["shape"]) == (l["scheme"], l["mode"], l["shape"])
        r.update(l)
        lo, hi = min(r["loop_ms"]), max(r["loop_ms"])
        r["verdict"] = "gain" if r["plan_ms"] < lo else "loss" if r["plan_ms"] > hi else "inside the loop's spread"
        r["loop_over_plan"] = [v / r["plan_ms"] for v in r["loop_ms"]]
        print(f"{r['scheme']:3s} {r['mode']:11s} {'x'.join(map(str, r['shape'])):14s} plan {r['plan_ms']:.3f}  loop {lo:.3f} .. {hi:.3f} ms "
              f"[{r['verdict']}]  k_lm_step {r['lm_ms']:.4f}  k_retrieve_apply {r['apply_ms']:.4f} ms | {r['jac_kernel']}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            prop = torch.cuda.get_device_properties(0)
            json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                       "blocks": args.blocks, "reps": args.reps, "rev": args.rev, "loop_root": args.loop_root or ".", "loop_rev": args.loop_rev,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
