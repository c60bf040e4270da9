"""The chained Levenberg-Marquardt step against the best composition the parent commit's library allows.

    kernels    npix = 1e4 pixels, nd in {12, 36} dates, npar in {5, 10}: k_lm_normal on 104 sensor rows per column (one block, weighted),
               k_lm_step_chain on its sums (the accepted path: cost is refilled with +inf before every call, one fill of npix doubles
               that is part of the figure) and k_lm_chain_covariance.
    baseline   the same step composed from what the parent has.  sensor: the per-column sums by crt_hip_lm_step_f64 on a scratch state
               (its A, g and cost are the sums); spectral: the sums are given, as crt_hip_spectral_normal_f64 leaves them.  Then torch:
               the pixel cost, torch.where for accept / reject and the lam update, the dense (nd npar)^2 scaled damped matrix of every
               pixel, torch.linalg.cholesky / cholesky_solve and the new trial point; the clamp and the xtol test are left out, which
               favours the composition.  Its time includes assembling the dense matrices (a fresh (npix, n, n) tensor per call, 10 GB
               at nd = 36, npar = 10, filled by indexed stores): a composition has to build them somehow, but a leaner assembly is
               conceivable, so the ratios are against this composition, not against a proven optimum.  Measured twice, each the
               median of 7 blocks of one call: a ratio counts as a gain only outside that spread.
    step       one full step() of the chained RetrievalPlan (4 sensor bands x 2 levels x 2 keys) and SpectralRetrievalPlan (2 keys x 2
               levels) for 2s and bl at 300 bands x 60 levels, --step-npix (1e4) pixels x 12 dates, npar = 3, next to the unchained plan on the
               same columns and to k_lm_step_chain alone: the share of a step the chain kernel takes beside the normal-equation evaluation.

HIP events around blocks of launches on one stream; the median of 7 blocks after one warm-up block (tools/levels_bench.py).

    python profiles/lm_chain/lm_chain_bench.py [--json profiles/lm_chain/lm_chain_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crt1d_amd import _lib, batched, synth  # noqa: E402
from levels_bench import timed  # noqa: E402

F64 = dict(dtype=torch.float64, device="cuda")
I32 = dict(dtype=torch.int32, device="cuda")
OPT = dict(lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0)
NROW = 104


def ptr(v):
    return None if v is None else v.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class State:
    def __init__(self, ncol, nunit, npar):
        ntri = npar * (npar + 1) // 2
        self.p, self.p_trial = 0.1 * torch.randn((ncol, npar), **F64), None
        self.p_trial = self.p.clone()
        self.cost, self.lam = torch.full((nunit,), float("inf"), **F64), torch.full((nunit,), 1e-2, **F64)
        self.A, self.g = torch.zeros((ncol, ntri), **F64), torch.zeros((ncol, npar), **F64)
        self.status, self.naccept, self.nreject = (torch.zeros((nunit,), **I32) for _ in range(3))
        self.c = _lib.CrtLmState(*[ptr(getattr(self, k)) for k in ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")])


def kernels_case(npix, nd, npar, blocks):
    lib = _lib.load()
    ncol, ntri, n = npix * nd, npar * (npar + 1) // 2, nd * npar
    torch.manual_seed(7)
    J = torch.randn((ncol, NROW, npar), **F64)
    f, y, s = torch.randn((ncol, NROW), **F64), torch.randn((ncol, NROW), **F64), 0.5 + torch.rand((ncol, NROW), **F64)
    w = 0.5 + 1.5 * torch.rand((nd - 1, npar), **F64)
    obs = (_lib.CrtLmObs * 1)(_lib.CrtLmObs(NROW, ptr(f), ptr(J), ptr(y), ptr(s)))
    sums = (torch.zeros((ncol, ntri), **F64), torch.zeros((ncol, npar), **F64), torch.zeros((ncol,), **F64))
    blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[ptr(v) for v in sums]))
    prob = _lib.CrtLmProblem(ncol, npar, *[OPT[k] for k in ("lam_up", "lam_down", "lam_min", "lam_max", "xtol", "ftol")], None, None, None, None)
    chain = _lib.CrtLmChain(npix, nd, 0, ptr(w))
    st = State(ncol, npix, npar)
    cov = torch.zeros((ncol, npar, npar), **F64)
    check = lambda rc: _lib.check(rc, "lm_chain_bench")  # noqa: E731

    def normal():
        check(lib.crt_hip_lm_normal_f64(ncol, npar, obs, 1, *[ptr(v) for v in sums], stream()))

    def step():
        st.cost.fill_(float("inf"))
        check(lib.crt_hip_lm_step_chain_f64(ctypes.byref(chain), ctypes.byref(prob), blk, 1, ctypes.byref(st.c), stream()))

    def covariance():
        check(lib.crt_hip_lm_chain_covariance_f64(ctypes.byref(chain), npar, ptr(st.A), ptr(cov), stream()))

    r = dict(npix=npix, nd=nd, npar=npar, nrow=NROW, lds_bytes=_lib.lm_chain_lds_bytes(nd, npar))
    r["normal_ms"] = timed(normal, blocks, 5)
    r["step_chain_ms"] = timed(step, blocks, 5)
    r["covariance_ms"] = timed(covariance, blocks, 5)
    assert int(st.naccept.min()) > 10 and int(st.status.max()) == 0 and bool(torch.isfinite(st.p_trial).all()) and bool(torch.isfinite(cov).all())

    # ---- the composition on the parent's entries ----
    col = State(ncol, ncol, npar)  # the scratch state of crt_hip_lm_step_f64: its A, g and cost are the sums of the trial point
    pix = State(ncol, npix, npar)
    col.p_trial = pix.p_trial
    col.c = _lib.CrtLmState(*[ptr(getattr(col, k)) for k in ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")])
    ti, tj = torch.tril_indices(npar, npar, device="cuda")
    w2 = torch.cat((w * w, torch.zeros((1, npar), **F64)))  # (nd, npar): the gap behind date d
    w2l = torch.cat((torch.zeros((1, npar), **F64), w * w))[:nd]
    eye = torch.eye(n, **F64)

    def compose(sensor):
        if sensor:
            col.cost.fill_(float("inf"))
            col.status.zero_()
            check(lib.crt_hip_lm_step_f64(ctypes.byref(prob), obs, 1, ctypes.byref(col.c), stream()))
            A_t, g_t, c_t = col.A, col.g, col.cost
        else:
            A_t, g_t, c_t = sums[0], sums[1], 0.5 * sums[2]
        pt = pix.p_trial.view(npix, nd, npar)
        e = (pt[:, 1:] - pt[:, :-1]) * w
        cost_t = c_t.view(npix, nd).sum(1) + 0.5 * (e * e).sum((1, 2))
        accept = cost_t < pix.cost
        a_col = accept.repeat_interleave(nd)[:, None]
        pix.p.copy_(torch.where(a_col, pix.p_trial, pix.p))
        pix.A.copy_(torch.where(a_col, A_t, pix.A))
        pix.g.copy_(torch.where(a_col, g_t, pix.g))
        pix.lam.copy_(torch.where(accept, (pix.lam * OPT["lam_down"]).clamp_min(OPT["lam_min"]), pix.lam * OPT["lam_up"]))
        pix.cost.copy_(torch.where(accept, cost_t, pix.cost))
        p = pix.p.view(npix, nd, npar)
        H = torch.zeros((npix, nd, npar, nd, npar), **F64)
        blkd = torch.zeros((npix, nd, npar, npar), **F64)
        blkd[:, :, ti, tj] = pix.A.view(npix, nd, -1)
        blkd = blkd + blkd.transpose(2, 3) - torch.diag_embed(torch.diagonal(blkd, dim1=2, dim2=3))
        blkd = blkd + torch.diag_embed((w2 + w2l).expand(npix, nd, npar))
        d = torch.arange(nd, device="cuda")
        k = torch.arange(npar, device="cuda")
        H[:, d, :, d, :] = blkd.permute(1, 0, 2, 3)
        H[:, d[1:, None], k, d[:-1, None], k] = -(w * w)
        H[:, d[:-1, None], k, d[1:, None], k] = -(w * w)
        H = H.view(npix, n, n)
        ep = (p[:, 1:] - p[:, :-1]) * (w * w)
        G = pix.g.view(npix, nd, npar).clone()
        G[:, 1:] += ep
        G[:, :-1] -= ep
        diag = torch.diagonal(H, dim1=1, dim2=2)
        dead = diag <= 0
        sc = torch.where(dead, torch.ones_like(diag), diag).rsqrt()
        M = H * sc[:, :, None] * sc[:, None, :] + eye * torch.where(dead, torch.ones_like(diag), pix.lam[:, None].expand_as(diag))[:, None, :]
        L = torch.linalg.cholesky(M)
        x = torch.cholesky_solve((-G.reshape(npix, n) * sc)[:, :, None], L)[:, :, 0] * sc
        pix.p_trial.copy_((pix.p + x.view(ncol, npar)))
        return x

    for kind in ("sensor", "spectral"):
        reps = []
        for _ in range(2):
            pix.cost.fill_(float("inf"))
            reps.append(timed(lambda: (pix.cost.fill_(float("inf")), compose(kind == "sensor")), blocks, 1))
        ours = r["step_chain_ms"] + (r["normal_ms"] if kind == "sensor" else 0.0)
        r[kind] = dict(ours_ms=ours, composition_ms=reps, ratio=[v / ours for v in reps])
    del J, f, y, s
    torch.cuda.empty_cache()
    return r


def step_case(scheme, spectral, npix, nd, blocks):
    nb, nz = 300, 60
    ncol = npix * nd
    d = synth.make_columns(npix, nb, nz, seed=3)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()  # noqa: E731
    rep = lambda v: np.repeat(v, nd, axis=0)  # noqa: E731
    psi = np.tile(np.deg2rad(np.linspace(15.0, 65.0, nd)), npix)
    cols = batched.Columns(t(psi), t(rep(d["lai"])), t(rep(d["g_kind"])).to(torch.int32), t(rep(d["g_param"])), t(rep(d["mla"])))
    bands = batched.Bands(t(rep(d["I_dr0"])), t(rep(d["I_df0"])), t(rep(d["leaf_r"])), t(rep(d["leaf_t"])), None if scheme == "bl" else t(rep(d["soil_r"])))
    mean = d["leaf_r"].mean(axis=0)
    dirs = t(np.stack((0.3 * mean * np.sin(np.linspace(0.0, 3.0, nb)), 0.3 * mean * np.cos(np.linspace(0.0, 2.0, nb)))))
    lev = (0, nz - 1)
    keys = ("I_df_d",) if scheme == "bl" else ("I_df_d", "I_df_u")
    w = np.zeros((4, nb))
    for s in range(4):
        w[s, 70 * s:70 * s + 60] = np.hanning(62)[1:61]
    sensors = batched.SensorSet(w)
    out = batched.solve_levels(scheme, cols, bands, lev, keys=keys) if spectral else batched.solve_sensor_levels(scheme, cols, bands, lev, sensors, keys=keys)
    y = {k: 1.02 * out[k] for k in keys}
    args = (scheme, cols, bands, lev) + (() if spectral else (sensors,)) + (y,)
    kw = dict(keys=keys, d_leaf_r=dirs, lai=True, lam0=1e-2)
    Plan = batched.SpectralRetrievalPlan if spectral else batched.RetrievalPlan
    res = dict(scheme=scheme, plan="spectral" if spectral else "sensor", npix=npix, nd=nd, npar=3, nb=nb, nz=nz)
    old = Plan(*args, **kw)
    res["unchained_step_ms"] = timed(lambda: old.step(), blocks, 3)
    del old
    new = Plan(*args, **kw, chain=nd, inv_sigma_chain=np.full((nd - 1, 3), 5.0))
    res["chained_step_ms"] = timed(lambda: new.step(), blocks, 3)
    s = torch.cuda.current_stream()
    # (the accepted path, as in kernels_case: without the refill the same sums are rejected until the pixels stall and return at once)
    res["chain_kernel_ms"] = timed(lambda: (new.cost.fill_(float("inf")), new.status.zero_(), new._step_chain(s)), blocks, 10)
    res["refill_ms"] = timed(lambda: (new.cost.fill_(float("inf")), new.status.zero_()), blocks, 10)
    res["chain_share"] = res["chain_kernel_ms"] / res["chained_step_ms"]
    res["chained_over_unchained"] = res["chained_step_ms"] / res["unchained_step_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "lm_chain_bench.json"))
    ap.add_argument("--npix", type=int, default=10_000)
    ap.add_argument("--step-npix", type=int, default=10_000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true", help="keep the kernel cases of an existing --json, measure the steps only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lm_chain_bench needs a GPU"
    out = dict(device=torch.cuda.get_device_name(0), blocks=args.blocks, kernels=[], steps=[])

    def save():
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)

    if os.path.exists(args.json) and args.skip_kernels:
        out["kernels"] = json.load(open(args.json)).get("kernels", [])
    for nd in (() if args.skip_kernels else (12, 36)):
        for npar in (5, 10):
            out["kernels"].append(kernels_case(args.npix, nd, npar, args.blocks))
            print(json.dumps(out["kernels"][-1]), flush=True)
            save()
    if not args.skip_steps:
        for scheme in ("2s", "bl"):
            for spectral in (False, True):
                out["steps"].append(step_case(scheme, spectral, args.step_npix, 12, args.blocks))
                print(json.dumps(out["steps"][-1]), flush=True)
                save()


if __name__ == "__main__":
    main()
