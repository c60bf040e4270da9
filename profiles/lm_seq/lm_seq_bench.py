"""The date-by-date retrieval against the chained one.

    kernels    npix = 1e4 pixels, (nd, npar) in {(12, 5), (36, 10), (365, 10)}: k_lm_prior_block and k_lm_predict on npix columns (one
               date's worth), k_lm_rts on the whole series.  Beside them, where nd fits the chain's LDS, crt_hip_lm_step_chain_f64 (the
               accepted path: cost refilled with +inf before every call, as profiles/lm_chain/lm_chain_bench.py does) and
               crt_hip_lm_chain_covariance_f64, each measured twice.  lm_chain.hip is untouched by this change (device_code_diff.txt), so
               those two are the parent commit's kernels.
    runs       SequentialPlan.run() against the chained plan's run() on one twin: --run-npix (1e4) pixels x 12 dates x 300 bands x 60
               levels, 2s and bl, sensor rows and spectra, npar = 3, --niter LM steps per date on both sides (the chain: --niter steps of
               all dates at once), noise-free, with the distance of both from the truth.  The chained run is measured twice.
    step       one step() of the unchained plan on npix * 12 columns with prior_precision against the same plan with a diagonal prior.

HIP events around blocks of launches on one stream; the median of 7 blocks after one warm-up block (tools/levels_bench.py).

    python profiles/lm_seq/lm_seq_bench.py [--json profiles/lm_seq/lm_seq_bench.json]
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


def ptr(v):
    return None if v is None else v.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def kernels_case(npix, nd, npar, blocks):
    lib = _lib.load()
    ncol, ntri = npix * nd, npar * (npar + 1) // 2
    torch.manual_seed(11)
    J = torch.randn((ncol, 3 * npar, npar), **F64)
    full = torch.einsum("coi,coj->cij", J, J) + torch.eye(npar, **F64)
    A = batched.pack_lower(full)  # (ncol, ntri): a filtered precision per (pixel, date)
    del J, full
    p = 0.1 * torch.randn((ncol, npar), **F64)
    w = 0.5 + 1.5 * torch.rand((nd - 1, npar), **F64)
    check = lambda rc: _lib.check(rc, "lm_seq_bench")  # noqa: E731
    r = dict(npix=npix, nd=nd, npar=npar)
    # one date's worth: npix columns
    mean, sums = torch.zeros((npix, npar), **F64), (torch.zeros((npix, ntri), **F64), torch.zeros((npix, npar), **F64), torch.zeros((npix,), **F64))
    pf = _lib.CrtLmPriorFull(npix, npar, ntri, ptr(A), ptr(mean))
    prec, info = torch.zeros((npix, ntri), **F64), torch.zeros((npix,), **I32)
    r["prior_block_ms"] = timed(lambda: check(lib.crt_hip_lm_prior_block_f64(ctypes.byref(pf), ptr(p), *[ptr(v) for v in sums], stream())), blocks, 20)
    r["predict_ms"] = timed(lambda: check(lib.crt_hip_lm_predict_f64(npix, npar, ptr(A), ptr(w), 0, ptr(prec), ptr(info), stream())), blocks, 20)
    assert not bool(info.any())
    p_s, cov, pinfo = torch.zeros((ncol, npar), **F64), torch.zeros((ncol, npar, npar), **F64), torch.zeros((npix,), **I32)
    chain = _lib.CrtLmChain(npix, nd, 0, ptr(w))
    r["rts_ms"] = timed(lambda: check(lib.crt_hip_lm_rts_f64(ctypes.byref(chain), npar, ptr(p), ptr(A), ptr(p_s), ptr(cov), ptr(pinfo), stream())),
                        blocks, 3)
    assert not bool(pinfo.any()) and bool(torch.isfinite(cov).all())
    # what the sweep moves through HBM: p_f, A_f and the weights in, p_s and cov_s out
    r["rts_bytes"] = 8 * (ncol * (2 * npar + ntri + npar * npar) + (nd - 1) * npar)
    r["rts_gb_s"] = r["rts_bytes"] / r["rts_ms"] / 1e6
    r["rts_us_per_date"] = 1e3 * r["rts_ms"] / nd
    if nd <= _lib.lm_chain_max_nd(npar):
        st = dict(p=p.clone(), p_trial=p.clone(), cost=torch.full((npix,), float("inf"), **F64), lam=torch.full((npix,), 1e-2, **F64), A=torch.zeros_like(A),
                  g=torch.zeros((ncol, npar), **F64), status=torch.zeros((npix,), **I32), naccept=torch.zeros((npix,), **I32), nreject=torch.zeros((npix,), **I32))
        cst = _lib.CrtLmState(*[ptr(st[k]) for k in ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")])
        g, c2 = 0.1 * torch.randn((ncol, npar), **F64), torch.ones((ncol,), **F64)
        blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(ptr(A), ptr(g), ptr(c2)))
        prob = _lib.CrtLmProblem(ncol, npar, *[OPT[k] for k in ("lam_up", "lam_down", "lam_min", "lam_max", "xtol", "ftol")], None, None, None, None)

        def step():
            st["cost"].fill_(float("inf"))
            check(lib.crt_hip_lm_step_chain_f64(ctypes.byref(chain), ctypes.byref(prob), blk, 1, ctypes.byref(cst), stream()))

        r["step_chain_ms"] = [timed(step, blocks, 3) for _ in range(2)]
        r["chain_covariance_ms"] = [timed(lambda: check(lib.crt_hip_lm_chain_covariance_f64(ctypes.byref(chain), npar, ptr(A), ptr(cov), stream())),
                                          blocks, 3) for _ in range(2)]
    torch.cuda.empty_cache()
    return r


def twin(scheme, spectral, npix, nd):
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
    sw = np.zeros((4, nb))
    for s in range(4):
        sw[s, 70 * s:70 * s + 60] = np.hanning(62)[1:61]
    sensors = batched.SensorSet(sw)
    rng = np.random.default_rng(5)
    truth = np.repeat(rng.uniform(-0.2, 0.2, (npix, 1, 3)), nd, axis=1)
    p = t(truth.reshape(ncol, 3))
    tc = batched.Columns(cols.psi, cols.lai * torch.exp(p[:, 2])[:, None], cols.g_kind, cols.g_param, cols.mla)
    tb = batched.Bands(bands.I_dr0, bands.I_df0, bands.leaf_r + p[:, 0, None] * dirs[0] + p[:, 1, None] * dirs[1], bands.leaf_t, bands.soil_r)
    out = batched.solve_levels(scheme, tc, tb, lev, keys=keys) if spectral else batched.solve_sensor_levels(scheme, tc, tb, lev, sensors, keys=keys)
    y = {k: out[k].clone() for k in keys}
    del tc, tb, out
    kw = dict(keys=keys, d_leaf_r=dirs, lai=True, lam0=1e-2)
    return (scheme, cols, bands, lev), sensors, y, kw, truth


def run_case(scheme, spectral, npix, nd, niter, blocks):
    head, sensors, y, kw, truth = twin(scheme, spectral, npix, nd)
    Plan = batched.SpectralRetrievalPlan if spectral else batched.RetrievalPlan
    args = head + (() if spectral else (sensors,)) + (y,)
    w = np.full((nd - 1, 3), 5.0)
    res = dict(scheme=scheme, plan="spectral" if spectral else "sensor", npix=npix, nd=nd, npar=3, niter=niter)
    dist = lambda p: float((p.reshape(npix, nd, 3).cpu() - torch.as_tensor(truth)).abs().max())  # noqa: E731
    chained = Plan(*args, **kw, chain=nd, inv_sigma_chain=w)
    res["chain_run_ms"] = [timed(lambda: chained.reset().run(niter), blocks, 1) for _ in range(2)]
    res["chain_distance"] = dist(chained.result()["p"])
    del chained
    torch.cuda.empty_cache()
    seq = batched.SequentialPlan(*head, y, nd=nd, inv_sigma_dyn=w, niter=niter, sensors=None if spectral else sensors, **kw)
    res["sequential_run_ms"] = timed(lambda: seq.run(), blocks, 1)
    res["sequential_filter_ms"] = timed(lambda: seq.run(smooth=False), blocks, 1)
    res["sequential_distance"] = dist(seq.run().result()["p"])
    res["sequential_over_chain"] = [res["sequential_run_ms"] / v for v in res["chain_run_ms"]]
    del seq
    torch.cuda.empty_cache()
    diag = Plan(*args, **kw, prior=np.zeros(3), inv_sigma_prior=np.ones(3))
    res["diag_prior_step_ms"] = [timed(lambda: diag.step(), blocks, 3) for _ in range(2)]
    del diag
    full = Plan(*args, **kw, prior_mean=np.zeros(3), prior_precision=np.eye(3))
    res["full_prior_step_ms"] = timed(lambda: full.step(), blocks, 3)
    del full
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "lm_seq_bench.json"))
    ap.add_argument("--npix", type=int, default=10_000)
    ap.add_argument("--run-npix", type=int, default=10_000)
    ap.add_argument("--niter", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--skip-runs", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lm_seq_bench needs a GPU"
    out = dict(device=torch.cuda.get_device_name(0), blocks=args.blocks, kernels=[], runs=[])

    def save():
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)

    for nd, npar in ((12, 5), (36, 10), (365, 10)):
        out["kernels"].append(kernels_case(args.npix, nd, npar, args.blocks))
        print(json.dumps(out["kernels"][-1]), flush=True)
        save()
    if not args.skip_runs:
        for scheme in ("2s", "bl"):
            for spectral in (False, True):
                out["runs"].append(run_case(scheme, spectral, args.run_npix, 12, args.niter, args.blocks))
                print(json.dumps(out["runs"][-1]), flush=True)
                save()


if __name__ == "__main__":
    main()
