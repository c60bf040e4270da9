"""The chained Levenberg-Marquardt step with shared parameters against the chain without them and against a torch composition
(DESIGN section 3.29).

    kernels    npix = 1e4 pixels, (nd, npar, ns) in {(12, 5, 2), (12, 10, 5), (36, 5, 2), (36, 10, 5)}, the first ns parameters shared:
               k_lm_step_shared on given sums (the accepted path: cost is refilled with +inf before every call, one fill of npix
               doubles that is part of the figure) and k_lm_shared_covariance; next to them crt_hip_lm_step_chain_f64 /
               crt_hip_lm_chain_covariance_f64 at the same (nd, npar) on the same sums, through the PARENT commit's library where
               --parent-lib names one, which solve the larger system of nd * npar unknowns.  (Without --parent-lib they go through
               this library, whose chain entries since profiles/lm_unify launch the shared-parameter kernels with an empty shared set:
               the comparison then is k_lm_step_shared at ns against the same kernel at ns = 0, not against the kernels the recorded
               lm_shared_bench.json was measured against.)
    baseline   the torch composition of profiles/lm_chain/lm_chain_bench.py extended by the border: the pixel cost, torch.where for accept
               / reject, the dense (nd nv + ns)^2 scaled damped arrowhead matrix of every pixel assembled by indexed stores,
               torch.linalg.cholesky / cholesky_solve, the new trial point; no clamp, no xtol test, which favours the composition.
    step       one full step() of the chained RetrievalPlan and SpectralRetrievalPlan (2s, 300 bands x 60 levels, --step-npix pixels x
               12 dates, npar = 3: two leaf directions and ln LAI) with shared=("dir0", "dir1") and without.

Every figure is measured twice, each the median of 7 blocks after one warm-up block (HIP events, tools/levels_bench.py): a ratio counts
as a difference only outside that spread.

    python profiles/lm_shared/lm_shared_bench.py [--parent-lib PATH] [--json profiles/lm_shared/lm_shared_bench.json]
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
CASES = ((12, 5, 2), (12, 10, 5), (36, 5, 2), (36, 10, 5))


def ptr(v):
    return None if v is None else v.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def twice(fn, blocks, per_block):
    return [timed(fn, blocks, per_block) for _ in range(2)]


def parent_library(path):
    """The chain entries of another build of the library (the parent commit's), with the signatures of this tree's table."""
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _lib._CHAIN_SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib


class State:
    def __init__(self, p0, nunit):
        ncol, npar = p0.shape
        ntri = npar * (npar + 1) // 2
        self.p, self.p_trial = p0.clone(), p0.clone()
        self.cost, self.lam = torch.full((nunit,), float("inf"), **F64), torch.full((nunit,), 1e-2, **F64)
        self.A, self.g = torch.zeros((ncol, ntri), **F64), torch.zeros((ncol, npar), **F64)
        self.status, self.naccept, self.nreject = (torch.zeros((nunit,), **I32) for _ in range(3))
        self.c = _lib.CrtLmState(*[ptr(getattr(self, k)) for k in ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")])


def kernels_case(npix, nd, npar, ns, blocks, parent):
    lib = _lib.load()
    ncol, ntri, nv = npix * nd, npar * (npar + 1) // 2, npar - ns
    n = nd * nv + ns
    torch.manual_seed(7)
    nrow = 3 * npar
    J = torch.randn((ncol, nrow, npar), **F64)
    r = torch.randn((ncol, nrow), **F64)
    ti, tj = torch.tril_indices(npar, npar, device="cuda")
    full = torch.einsum("coi,coj->cij", J, J)
    sums = (full[:, ti, tj].contiguous(), torch.einsum("coi,co->ci", J, r).contiguous(), (r * r).sum(1).contiguous())
    del J, r
    w = 0.5 + 1.5 * torch.rand((nd - 1, npar), **F64)
    blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[ptr(v) for v in sums]))
    prob = _lib.CrtLmProblem(ncol, npar, *[OPT[k] for k in ("lam_up", "lam_down", "lam_min", "lam_max", "xtol", "ftol")], None, None, None, None)
    chain = _lib.CrtLmChain(npix, nd, 0, ptr(w))
    shared = _lib.CrtLmShared((1 << ns) - 1)
    p0 = 0.1 * torch.randn((ncol, npar), **F64)
    p0.view(npix, nd, npar)[:, 1:, :ns] = p0.view(npix, nd, npar)[:, :1, :ns]
    st, stc = State(p0, npix), State(p0, npix)
    cov = torch.zeros((ncol, npar, npar), **F64)
    check = lambda rc: _lib.check(rc, "lm_shared_bench")  # noqa: E731
    plib = parent or lib

    def step_shared():
        st.cost.fill_(float("inf"))
        check(lib.crt_hip_lm_step_shared_f64(ctypes.byref(chain), ctypes.byref(shared), ctypes.byref(prob), blk, 1, ctypes.byref(st.c), stream()))

    def cov_shared():
        check(lib.crt_hip_lm_shared_covariance_f64(ctypes.byref(chain), ctypes.byref(shared), npar, ptr(st.A), ptr(cov), stream()))

    def step_chain():
        stc.cost.fill_(float("inf"))
        check(plib.crt_hip_lm_step_chain_f64(ctypes.byref(chain), ctypes.byref(prob), blk, 1, ctypes.byref(stc.c), stream()))

    def cov_chain():
        check(plib.crt_hip_lm_chain_covariance_f64(ctypes.byref(chain), npar, ptr(stc.A), ptr(cov), stream()))

    res = dict(npix=npix, nd=nd, npar=npar, ns=ns, unknowns_shared=n, unknowns_chain=nd * npar, lds_bytes_shared=_lib.lm_shared_lds_bytes(nd, nv, ns),
               lds_bytes_chain=_lib.lm_chain_lds_bytes(nd, npar), chain_through="parent library" if parent else "this library")
    res["step_shared_ms"] = twice(step_shared, blocks, 5)
    res["covariance_shared_ms"] = twice(cov_shared, blocks, 5)
    assert int(st.naccept.min()) > 10 and int(st.status.max()) == 0 and bool(torch.isfinite(st.p_trial).all()) and bool(torch.isfinite(cov).all())
    res["step_chain_ms"] = twice(step_chain, blocks, 5)
    res["covariance_chain_ms"] = twice(cov_chain, blocks, 5)
    assert int(stc.naccept.min()) > 10 and int(stc.status.max()) == 0 and bool(torch.isfinite(cov).all())
    res["shared_over_chain_step"] = [a / b for a, b in zip(res["step_shared_ms"], res["step_chain_ms"])]
    res["shared_over_chain_covariance"] = [a / b for a, b in zip(res["covariance_shared_ms"], res["covariance_chain_ms"])]

    # ---- the torch composition on the same sums ----
    pix = State(p0, npix)
    kv, ks = torch.arange(ns, npar, device="cuda"), torch.arange(0, ns, device="cuda")
    wv = w[:, ns:]
    w2 = torch.cat((wv * wv, torch.zeros((1, nv), **F64)))
    w2l = torch.cat((torch.zeros((1, nv), **F64), wv * wv))[:nd]
    eye = torch.eye(n, **F64)
    d, k = torch.arange(nd, device="cuda"), torch.arange(nv, device="cuda")
    N = nd * nv

    def compose():
        A_t, g_t, c_t = sums[0], sums[1], 0.5 * sums[2]
        pt = pix.p_trial.view(npix, nd, npar)
        e = (pt[:, 1:, ns:] - pt[:, :-1, ns:]) * wv
        cost_t = c_t.view(npix, nd).sum(1) + 0.5 * (e * e).sum((1, 2))
        accept = cost_t < pix.cost
        a_col = accept.repeat_interleave(nd)[:, None]
        pix.p.copy_(torch.where(a_col, pix.p_trial, pix.p))
        pix.A.copy_(torch.where(a_col, A_t, pix.A))
        pix.g.copy_(torch.where(a_col, g_t, pix.g))
        pix.lam.copy_(torch.where(accept, (pix.lam * OPT["lam_down"]).clamp_min(OPT["lam_min"]), pix.lam * OPT["lam_up"]))
        pix.cost.copy_(torch.where(accept, cost_t, pix.cost))
        p = pix.p.view(npix, nd, npar)
        Ad = torch.zeros((npix, nd, npar, npar), **F64)
        Ad[:, :, ti, tj] = pix.A.view(npix, nd, -1)
        Ad = Ad + Ad.transpose(2, 3) - torch.diag_embed(torch.diagonal(Ad, dim1=2, dim2=3))
        H = torch.zeros((npix, n, n), **F64)
        Hv = H[:, :N, :N].view(npix, nd, nv, nd, nv)
        Hv[:, d, :, d, :] = (Ad[:, :, ns:, ns:] + torch.diag_embed((w2 + w2l).expand(npix, nd, nv))).permute(1, 0, 2, 3)
        Hv[:, d[1:, None], k, d[:-1, None], k] = -(wv * wv)
        Hv[:, d[:-1, None], k, d[1:, None], k] = -(wv * wv)
        border = Ad[:, :, :ns, ns:].permute(0, 2, 1, 3).reshape(npix, ns, N)
        H[:, N:, :N] = border
        H[:, :N, N:] = border.transpose(1, 2)
        H[:, N:, N:] = Ad[:, :, :ns, :ns].sum(1)
        ep = (p[:, 1:, ns:] - p[:, :-1, ns:]) * (wv * wv)
        gd = pix.g.view(npix, nd, npar)
        Gv = gd[:, :, ns:].clone()
        Gv[:, 1:] += ep
        Gv[:, :-1] -= ep
        G = torch.cat((Gv.reshape(npix, N), gd[:, :, :ns].sum(1)), dim=1)
        diag = torch.diagonal(H, dim1=1, dim2=2)
        dead = diag <= 0
        sc = torch.where(dead, torch.ones_like(diag), diag).rsqrt()
        M = H * sc[:, :, None] * sc[:, None, :] + eye * torch.where(dead, torch.ones_like(diag), pix.lam[:, None].expand_as(diag))[:, None, :]
        L = torch.linalg.cholesky(M)
        x = torch.cholesky_solve((-G * sc)[:, :, None], L)[:, :, 0] * sc
        new = p.clone()
        new[:, :, ns:] += x[:, :N].view(npix, nd, nv)
        new[:, :, :ns] = (p[:, :1, :ns] + x[:, None, N:])
        pix.p_trial.copy_(new.view(ncol, npar))
        return x

    res["composition_ms"] = twice(lambda: (pix.cost.fill_(float("inf")), compose()), blocks, 1)
    res["composition_over_shared_step"] = [a / b for a, b in zip(res["composition_ms"], res["step_shared_ms"])]
    # the composition and the kernel solve the same system: one step from the same start
    st2, px2 = State(p0, npix), State(p0, npix)
    check(lib.crt_hip_lm_step_shared_f64(ctypes.byref(chain), ctypes.byref(shared), ctypes.byref(prob), blk, 1, ctypes.byref(st2.c), stream()))
    pix.p.copy_(px2.p), pix.p_trial.copy_(px2.p_trial), pix.cost.fill_(float("inf")), pix.lam.fill_(1e-2)
    compose()
    res["composition_max_abs_diff"] = float((pix.p_trial - st2.p_trial).abs().max())
    torch.cuda.empty_cache()
    return res


def step_case(spectral, npix, nd, blocks):
    scheme, nb, nz = "2s", 300, 60
    d = synth.make_columns(npix, nb, nz, seed=3)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()  # noqa: E731
    rep = lambda v: np.repeat(v, nd, axis=0)  # noqa: E731
    psi = np.tile(np.deg2rad(np.linspace(15.0, 65.0, nd)), npix)
    cols = batched.Columns(t(psi), t(rep(d["lai"])), t(rep(d["g_kind"])).to(torch.int32), t(rep(d["g_param"])), t(rep(d["mla"])))
    bands = batched.Bands(t(rep(d["I_dr0"])), t(rep(d["I_df0"])), t(rep(d["leaf_r"])), t(rep(d["leaf_t"])), t(rep(d["soil_r"])))
    mean = d["leaf_r"].mean(axis=0)
    dirs = t(np.stack((0.3 * mean * np.sin(np.linspace(0.0, 3.0, nb)), 0.3 * mean * np.cos(np.linspace(0.0, 2.0, nb)))))
    lev, keys = (0, nz - 1), ("I_df_d", "I_df_u")
    w = np.zeros((4, nb))
    for s in range(4):
        w[s, 70 * s:70 * s + 60] = np.hanning(62)[1:61]
    sensors = batched.SensorSet(w)
    out = batched.solve_levels(scheme, cols, bands, lev, keys=keys) if spectral else batched.solve_sensor_levels(scheme, cols, bands, lev, sensors, keys=keys)
    y = {k: 1.02 * out[k] for k in keys}
    args = (scheme, cols, bands, lev) + (() if spectral else (sensors,)) + (y,)
    kw = dict(keys=keys, d_leaf_r=dirs, lai=True, lam0=1e-2, chain=nd, inv_sigma_chain=np.full((nd - 1, 3), 5.0))
    Plan = batched.SpectralRetrievalPlan if spectral else batched.RetrievalPlan
    res = dict(scheme=scheme, plan="spectral" if spectral else "sensor", npix=npix, nd=nd, npar=3, ns=2, nb=nb, nz=nz)
    s = torch.cuda.current_stream()
    for name, extra in (("chained", {}), ("shared", dict(shared=("dir0", "dir1")))):
        plan = Plan(*args, **kw, **extra)
        res[name + "_step_ms"] = twice(lambda: plan.step(), blocks, 3)
        res[name + "_closing_kernel_ms"] = twice(lambda: (plan.cost.fill_(float("inf")), plan.status.zero_(), plan._step_chain(s)), blocks, 10)
        del plan
    res["shared_over_chained_step"] = [a / b for a, b in zip(res["shared_step_ms"], res["chained_step_ms"])]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "lm_shared_bench.json"))
    ap.add_argument("--parent-lib", default=None, help="libcrt1d_hip.so built from the parent commit: the chain entries are measured through it")
    ap.add_argument("--npix", type=int, default=10_000)
    ap.add_argument("--step-npix", type=int, default=10_000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lm_shared_bench needs a GPU"
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    out = dict(device=torch.cuda.get_device_name(0), blocks=args.blocks, kernels=[], steps=[])

    def save():
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)

    for nd, npar, ns in CASES:
        out["kernels"].append(kernels_case(args.npix, nd, npar, ns, args.blocks, parent))
        print(json.dumps(out["kernels"][-1]), flush=True)
        save()
    if not args.skip_steps:
        for spectral in (False, True):
            out["steps"].append(step_case(spectral, args.step_npix, 12, args.blocks))
            print(json.dumps(out["steps"][-1]), flush=True)
            save()


if __name__ == "__main__":
    main()
