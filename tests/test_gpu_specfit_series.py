"""GPU: the spectral normal equations over a sun-angle series (include/series/crt1d_hip_specfit_series.h; batched.SpectralNormalSeriesPlan,
SpectralRetrievalPlan(sun=), retrieve_spectral(sun=), Model.retrieve_spectral(psi=)).  Everything here is bitwise: the series kernel runs the
body of k_spec_normal, so there is no tolerance to derive.

1. Slice contract: [:, t] of A_t, g_t, c2_t and fwd against a SpectralNormalPlan of step t.
2. Sum contract: A, g, c2 against the sequential torch sum of the slices, and the step on the one summed block against the step on nt blocks.
3. Independence of the batch, of another column's mask and series; a sun state masked completely.
4. CRT_FLAG_SKIP_PRECOMPUTE and a LevelsSeriesPlan on the same workspace.
5. Twin retrieval against the host loop of the per-step pieces, state by state.
6. fitted(), nobs(), covariance(scale=True), the one-shots and the model."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_retrieve import STATE, _same, _t
from test_gpu_specfit import LMN

pytestmark = pytest.mark.gpu

CLOSED = ("2s", "bl", "g77", "bf")
PARAMS = ("leaf_r", "leaf_t", "soil_r")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
SUMS = ("A", "g", "c2")
ELLIPSOIDAL = 3
NCOL, NZ = 3, 10


def _observed(scheme, wide=False):
    """-> (levels, keys): I_df_u at the top; bl (no upward stream, nothing depends on a parameter at the top): I_dr and I_df_d at the ground
    and at mid-canopy.  wide: four keys at seven levels."""
    if wide:
        return (0, 1, 3, 4, 6, 8, 9), KEYS
    return ((0, NZ // 2), ("I_dr", "I_df_d")) if scheme == "bl" else ((NZ - 1,), ("I_df_u",))


@functools.lru_cache(maxsize=None)
def _inputs(scheme, nb, nt, wide=False):
    """Ragged columns of the ellipsoidal class, a sun series (shared incoming spectra for nt = 3, per column otherwise), the series tangent,
    directions shared over the columns, and observations with a tenth of the rows masked (NaN under the mask)."""
    import torch

    from crt1d_amd import batched, synth

    lev, keys = _observed(scheme, wide)
    ntan = 8 if wide else 3
    d = dict(synth.make_columns(NCOL, nb, NZ, seed=300 + nb + nt, uniform_dlai=False))
    rng = np.random.default_rng(11 * nb + nt)
    d["g_kind"] = np.full(NCOL, ELLIPSOIDAL, dtype=np.int32)
    d["g_param"] = rng.uniform(0.7, 2.0, NCOL)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    sun = batched.SunSeries.from_host(synth.make_sun_series(d, nt, seed=17 + nt, shared=nt == 3))
    assert sun.col_stride == (0 if nt == 3 else nt * nb)
    tan = batched.leaf_tangent_series(cols, sun, "param")
    dirs = {"d_" + k: _t(rng.uniform(-1.0, 1.0, (ntan, nb)) * d[k].mean(axis=0)) for k in PARAMS}
    shape = (NCOL, nt, len(lev), nb)
    y, s = {}, {}
    for k in keys:
        dead = rng.uniform(size=shape) < 0.1
        y[k] = _t(np.where(dead, np.nan, rng.uniform(0.0, 5.0, shape)))
        s[k] = _t(np.where(dead, 0.0, rng.uniform(0.5, 2.0, shape)))
    torch.cuda.synchronize()
    return dict(cols=cols, bands=bands, sun=sun, tan=tan, dirs=dirs, lev=lev, keys=keys, y=y, s=s, ntan=ntan)


def _clone(out, keys):
    res = {k: out[k].clone() for k in out if k != "fwd"}
    if "fwd" in out:
        res["fwd"] = {k: out["fwd"][k].clone() for k in keys}
    return res


def _series(scheme, P, *, cols=None, y=None, s=None, sun=None, tan=None, per_step=True, fwd=True, flags=0):
    """One call of a fresh SpectralNormalSeriesPlan on the case (or its columns `cols`, a slice).  -> plan, clones of its outputs"""
    import torch

    from crt1d_amd import batched

    c, b, sn, tn = P["cols"], P["bands"], P["sun"] if sun is None else sun, P["tan"] if tan is None else tan
    y, s = P["y"] if y is None else y, P["s"] if s is None else s
    if cols is not None:
        lo, hi = cols.start, cols.stop
        c, b, sn, tn = c.slice(lo, hi), b.slice(lo, hi), sn.slice(lo, hi), tn.slice(lo, hi)
        y, s = {k: v[cols].contiguous() for k, v in y.items()}, {k: v[cols].contiguous() for k, v in s.items()}
    plan = batched.SpectralNormalSeriesPlan(scheme, c, b, sn, P["lev"], y, keys=P["keys"], inv_sigma=s, **P["dirs"], lai=True, tangent=tn,
                                            per_step=per_step, fwd=fwd)
    out = plan(flags=flags)
    torch.cuda.synchronize()
    return plan, _clone(out, P["keys"])


def _steps(scheme, P, y=None, s=None):
    """The per-step plans on the inputs of every sun state: -> [clones of the outputs of step t]"""
    import torch

    from crt1d_amd import batched

    y, s = P["y"] if y is None else y, P["s"] if s is None else s
    res = []
    for t in range(P["sun"].nt):
        plan = batched.SpectralNormalPlan(scheme, batched._step_columns(P["cols"], P["sun"], t), batched._step_bands(P["bands"], P["sun"], t),
                                          P["lev"], {k: v[:, t].contiguous() for k, v in y.items()}, keys=P["keys"],
                                          inv_sigma={k: v[:, t].contiguous() for k, v in s.items()}, **P["dirs"], lai=True,
                                          tangent=P["tan"].step(t), fwd=True)
        res.append(_clone(plan(), P["keys"]))
        res[-1]["kernel"] = plan.last_kernel()
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _both(scheme, nb, nt, wide=False):
    P = _inputs(scheme, nb, nt, wide)
    plan, got = _series(scheme, P)
    return P, plan.last_kernel(), got, _steps(scheme, P)


def _check_slices(P, kernel, got, steps, nslice, per):
    import torch

    nt, npar = P["sun"].nt, P["ntan"] + 2
    assert got["A_t"].shape == (NCOL, nt, npar * (npar + 1) // 2) and got["g_t"].shape == (NCOL, nt, npar) and got["c2_t"].shape == (NCOL, nt)
    name = kernel.split("<")[1].split(">")[0]
    assert kernel == (f"k_spec_normal_series<{name}> nt={nt} nsel={len(P['lev'])} nkey={len(P['keys'])} npar={npar} slice={per} "
                      "+ k_spec_normal_series_finish")
    for t, ref in enumerate(steps):
        assert f"slice={per}" in ref["kernel"] and ("k_spec_normal_finish" in ref["kernel"]) == (nslice > 1)  # the same slices
        for k in SUMS:
            assert torch.equal(got[k + "_t"][:, t], ref[k]), (k, t)
            assert bool(torch.isfinite(ref[k]).all())
        for k in P["keys"]:
            assert torch.equal(got["fwd"][k][:, t], ref["fwd"][k]), (k, t)
    assert bool((got["c2"] > 0).all())


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 3, 5])
@pytest.mark.parametrize("nb", [5, 65, 300])  # a partial wave; two waves; two 256-lane slices
@pytest.mark.parametrize("scheme", CLOSED)
def test_slice_contract(scheme, nb, nt):
    P, kernel, got, steps = _both(scheme, nb, nt)
    _check_slices(P, kernel, got, steps, 2 if nb == 300 else 1, 150 if nb == 300 else nb)


@pytest.mark.parametrize("scheme", ["2s", "bl"])
def test_slice_contract_at_the_widest_rows(scheme):
    """Four keys x 7 levels x (10 + 1) = 308 rows: 64-lane slices, three of them at nb = 130."""
    P, kernel, got, steps = _both(scheme, 130, 2, True)
    _check_slices(P, kernel, got, steps, 3, 44)


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 3, 5])
@pytest.mark.parametrize("nb", [5, 65, 300])
@pytest.mark.parametrize("scheme", CLOSED)
def test_sum_contract(scheme, nb, nt):
    """A, g, c2 are the left-to-right sum of the slices from t = 0's bits; nt in {1, 3}: the step on the one summed block leaves the state
    the step on nt per-step blocks leaves."""
    import torch

    P, _, got, steps = _both(scheme, nb, nt)
    for k in SUMS:
        tot = got[k + "_t"][:, 0].clone()
        for t in range(1, nt):
            tot = tot + got[k + "_t"][:, t]
        assert torch.equal(got[k], tot), k
    _, bare = _series(scheme, P, per_step=False, fwd=False)  # the sums do not depend on what else is written
    assert set(bare) == set(SUMS) and all(torch.equal(bare[k], got[k]) for k in SUMS)
    if nt > 3:
        return
    rng = np.random.default_rng(nb + nt)
    p0 = _t(rng.normal(size=(NCOL, 5)))
    prior, isp = _t(rng.normal(size=(NCOL, 5))), _t(rng.uniform(0.5, 2.0, (NCOL, 5)))
    one = LMN([{k: got[k] for k in SUMS}], p0, prior=prior, isp=isp).step().snap()
    many = LMN([{k: steps[t][k] for k in SUMS} for t in range(nt)], p0, prior=prior, isp=isp).step().snap()
    assert _same(one, many) and np.all(one["naccept"] == 1)


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [65, 300])
@pytest.mark.parametrize("scheme", CLOSED)
def test_independence(scheme, nb):
    import torch

    from crt1d_amd import batched

    nt = 5  # (incoming spectra per column)
    P, _, full, _ = _both(scheme, nb, nt)
    every = [k + "_t" for k in SUMS] + list(SUMS)
    # a column alone is the column in the batch
    _, one = _series(scheme, P, cols=slice(1, 2))
    for k in every:
        assert torch.equal(one[k], full[k][1:2]), k
    for k in P["keys"]:
        assert torch.equal(one["fwd"][k], full["fwd"][k][1:2])
    # another column's mask does not reach this one
    s2 = {k: v.clone() for k, v in P["s"].items()}
    s2[P["keys"][0]][0, :, :, ::2] = 0.0
    s2[P["keys"][0]][2, 1:] = 0.0
    _, masked = _series(scheme, P, s=s2)
    for k in every:
        assert torch.equal(masked[k][1], full[k][1]), k
        assert not torch.equal(masked[k][0], full[k][0]) and not torch.equal(masked[k][2], full[k][2])
    # nor does another column's whole series
    sun = P["sun"]
    psi, I_dr0, I_df0 = sun.psi.clone(), sun.I_dr0.clone(), sun.I_df0.clone()
    psi[0] = psi[0].flip(0) * 0.9
    I_dr0[0], I_df0[2] = I_dr0[0] * 1.5, I_df0[2].flip(0)
    sun2 = batched.SunSeries(psi, I_dr0, I_df0)
    _, moved = _series(scheme, P, sun=sun2, tan=batched.leaf_tangent_series(P["cols"], sun2, "param"))
    for k in every:
        assert torch.equal(moved[k][1], full[k][1]), k
        assert not torch.equal(moved[k][0], full[k][0])
    # a sun state masked completely (the night) contributes +0; the NaN of its y does not spread
    night = 2
    s3 = {k: v.clone() for k, v in P["s"].items()}
    y3 = {k: v.clone() for k, v in P["y"].items()}
    for k in P["keys"]:
        s3[k][:, night] = 0.0
        y3[k][:, night] = float("nan")
    _, dark = _series(scheme, P, y=y3, s=s3)
    for k in SUMS:
        z = dark[k + "_t"][:, night]
        assert bool((z == 0).all()) and not bool(torch.signbit(z).any())
        tot = None
        for t in range(nt):
            if t != night:
                tot = dark[k + "_t"][:, t].clone() if tot is None else tot + dark[k + "_t"][:, t]
        assert bool(torch.isfinite(dark[k]).all()) and bool((dark[k] == tot).all()), k
        for t in range(nt):
            if t != night:
                assert torch.equal(dark[k + "_t"][:, t], full[k + "_t"][:, t])
    assert bool((dark["c2"] > 0).all())  # (every column keeps unmasked states)


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
def test_skip_precompute_and_the_shared_workspace(scheme):
    import torch

    from crt1d_amd import _lib, batched

    P, _, full, _ = _both(scheme, 300, 3)
    plan, first = _series(scheme, P)
    for v in plan.out.values():
        for w in (v.values() if isinstance(v, dict) else (v,)):
            w.fill_(-7.0)
    again = _clone(plan(flags=_lib.FLAG_SKIP_PRECOMPUTE), P["keys"])
    torch.cuda.synchronize()
    for k in [k + "_t" for k in SUMS] + list(SUMS):
        assert torch.equal(again[k], first[k]) and torch.equal(first[k], full[k]), k
    for k in P["keys"]:
        assert torch.equal(again["fwd"][k], first["fwd"][k])
    plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    want = f"k_colpre<canopy> + k_colsun nt=3{' + k_dlai_side' if scheme == 'bl' else ''} + k_dleaf_side<canopy>"
    assert plan.last_kernel() == want
    # the records come first and at the offsets of the level series: that plan runs on them
    alone = {k: v.clone() for k, v in batched.solve_levels_series(scheme, P["cols"], P["bands"], P["sun"], P["lev"], keys=P["keys"]).items()}
    lev = batched.LevelsSeriesPlan(scheme, P["cols"], P["bands"], P["sun"], P["lev"], keys=P["keys"], workspace=plan.workspace)
    shared = lev(flags=_lib.FLAG_SKIP_PRECOMPUTE)
    torch.cuda.synchronize()
    for k in P["keys"]:
        assert torch.equal(shared[k], alone[k]), k
    need = batched.spectral_normal_series_workspace_bytes(scheme, NCOL, NZ, 300, 3, len(P["lev"]), len(P["keys"]), 5)
    assert plan.workspace.numel() * plan.workspace.element_size() >= need > batched.levels_series_workspace_bytes(scheme, NCOL, NZ, 3)


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
NSTEP = 15


@functools.lru_cache(maxsize=None)
def _twin(scheme, nb=40, nt=5):
    """A noise-free twin over nt sun states: y from LevelsPlan at a known p*, 3 directions + ln LAI + the ellipsoidal x (the twin of
    tests/test_gpu_specfit.py with a sun-state axis).  bl: its soil direction is dead, so its directions lie in leaf_r, leaf_t, leaf_r."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nz = 4, NZ
    d = synth.make_columns(ncol, nb, nz, seed=5, uniform_dlai=False)
    rng = np.random.default_rng(41)
    wl = np.linspace(0.0, 3.0, nb)
    shapes = np.stack([np.sin(wl) + 1.5, np.cos(2 * wl), wl / 3.0])
    if scheme == "bl":
        dirs = {"d_leaf_r": _t(0.1 * d["leaf_r"].mean(axis=0) * shapes * np.array([1.0, 0.0, 1.0])[:, None]),
                "d_leaf_t": _t(0.1 * d["leaf_t"].mean(axis=0) * shapes * np.array([0.0, 1.0, 0.0])[:, None])}
        lev, keys = (0, nz // 2), ("I_dr", "I_df_d")
    else:
        dirs = {"d_leaf_r": _t(0.1 * d["leaf_r"].mean(axis=0) * shapes * np.array([1.0, 0.0, 0.0])[:, None]),
                "d_leaf_t": _t(0.1 * d["leaf_t"].mean(axis=0) * shapes * np.array([0.0, 1.0, 0.0])[:, None]),
                "d_soil_r": _t(0.1 * d["soil_r"].mean(axis=0) * shapes * np.array([0.0, 0.0, 1.0])[:, None])}
        lev, keys = (nz - 1,), ("I_df_u",)
    truth = torch.cat((_t(rng.uniform(-0.2, 0.2, (ncol, 3))), _t(rng.uniform(-0.2, 0.2, (ncol, 1))), _t(rng.uniform(0.8, 1.8, (ncol, 1)))), dim=1)
    kind = torch.full((ncol,), ELLIPSOIDAL, dtype=torch.int32, device="cuda")
    x0 = torch.full((ncol,), 1.2, dtype=torch.float64, device="cuda")
    cols = batched.Columns(_t(d["psi"]), _t(d["lai"]), kind, x0, _t(d["mla"]))
    bands = batched.Bands(_t(d["I_dr0"]), _t(d["I_df0"]), _t(d["leaf_r"]), _t(d["leaf_t"]), _t(d["soil_r"]))
    s = synth.make_sun_series(d, nt, seed=9)
    s["psi"] = np.deg2rad(np.linspace(15.0, 70.0, nt))[None, :] + np.deg2rad(rng.uniform(-3.0, 3.0, (ncol, nt)))  # a diurnal course
    sun = batched.SunSeries.from_host(s)
    # the observations: the level spectra of every sun state at p*
    tc = batched.Columns(cols.psi, cols.lai * torch.exp(truth[:, 3])[:, None], kind, truth[:, 4].contiguous(), cols.mla)
    spec = {n: getattr(bands, n) + (torch.einsum("ck,kb->cb", truth[:, :3], dirs["d_" + n]) if "d_" + n in dirs else 0.0) for n in PARAMS}
    tb = batched.Bands(bands.I_dr0, bands.I_df0, spec["leaf_r"], spec["leaf_t"], spec["soil_r"])
    X = [batched.solve_levels(scheme, batched._step_columns(tc, sun, t), batched._step_bands(tb, sun, t), lev, keys=keys) for t in range(nt)]
    y = {k: torch.stack([x[k].clone() for x in X], dim=1).contiguous() for k in keys}
    p0 = torch.cat((torch.zeros((ncol, 4), dtype=torch.float64, device="cuda"), x0[:, None]), dim=1)
    torch.cuda.synchronize()
    return dict(cols=cols, bands=bands, sun=sun, dirs=dirs, truth=truth, lev=lev, keys=keys, y=y, p0=p0)


def _twin_kw(P):
    lo, hi = np.array([-np.inf] * 4 + [0.2]), np.array([np.inf] * 4 + [5.0])
    return dict(keys=P["keys"], **P["dirs"], lai=True, leaf=True, p0=P["p0"], lo=lo, hi=hi, lam0=1e-2, lam_up=10.0, lam_down=0.1, xtol=0.0, ftol=0.0)


class HostLoop:
    """The loop the pieces without a series allow: the state, the apply step and the working tensors of a per-step SpectralRetrievalPlan
    (the working LAI, leaf-angle parameter and optics do not depend on the sun); per sun state the tangent refill and a SpectralNormalPlan on
    those tensors with the sun and the incoming spectra of the step; the ascending torch sum; crt_hip_lm_step_normal_f64 with one block."""

    def __init__(self, scheme, P):
        import torch

        from crt1d_amd import _lib, batched

        sun, nt = P["sun"], P["sun"].nt
        self.base = batched.SpectralRetrievalPlan(scheme, batched._step_columns(P["cols"], sun, 0), batched._step_bands(P["bands"], sun, 0),
                                                  P["lev"], {k: v[:, 0].contiguous() for k, v in P["y"].items()}, **_twin_kw(P))
        w, wb = self.base.cols, self.base.bands
        ncol = w.ncol
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
        self.cols = [batched.Columns(sun.psi[:, t].contiguous(), w.lai, w.g_kind, w.g_param, w.mla) for t in range(nt)]
        for c in self.cols:
            assert c.lai.data_ptr() == w.lai.data_ptr() and c.g_param.data_ptr() == w.g_param.data_ptr()  # (the working tensors themselves)
        self.tans = [batched.LeafTangent(new(ncol, _lib.NQ), new(ncol)) for _ in range(nt)]
        self.plans = []
        for t in range(nt):
            b = batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), wb.leaf_r, wb.leaf_t, wb.soil_r)
            assert b.leaf_r.data_ptr() == wb.leaf_r.data_ptr()
            self.plans.append(batched.SpectralNormalPlan(scheme, self.cols[t], b, P["lev"], {k: v[:, t].contiguous() for k, v in P["y"].items()},
                                                         keys=P["keys"], **P["dirs"], lai=True, tangent=self.tans[t]))
        self.sums = {k: torch.zeros_like(self.plans[0].out[k]) for k in SUMS}
        self._blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[self.sums[k].data_ptr() for k in SUMS]))

    def step(self):
        import torch

        from crt1d_amd import _lib, batched

        B, lib, h = self.base, self.base.lib, torch.cuda.current_stream().cuda_stream
        assert lib.crt_hip_retrieve_apply_f64(ctypes.byref(B._ap), ctypes.byref(B._dirs), h) == _lib.CRT_OK
        for t, plan in enumerate(self.plans):
            dg_table, dg_at_psi = batched.g_dparam(self.cols[t])
            self.tans[t].dg_table.copy_(dg_table)
            self.tans[t].dg_at_psi.copy_(dg_at_psi)
            plan()
        for k in SUMS:
            tot = self.plans[0].out[k].clone()
            for plan in self.plans[1:]:
                tot = tot + plan.out[k]
            self.sums[k].copy_(tot)
        assert lib.crt_hip_lm_step_normal_f64(ctypes.byref(B._prob), self._blk, 1, ctypes.byref(B._state), h) == _lib.CRT_OK
        return {k: getattr(B, k).cpu().numpy().copy() for k in STATE}


@pytest.mark.parametrize("scheme", ["2s", "bl"])
def test_twin_retrieval(scheme):
    """By the two contracts the plan's state is the host loop's after every step, bit for bit; the cost never increases; the parameter error
    against the truth is at most 10 x the host loop's own (the rule of tests/test_gpu_specfit.py::test_twin_retrieval)."""
    import torch

    from crt1d_amd import batched

    P = _twin(scheme)
    host = HostLoop(scheme, P)
    plan = batched.SpectralRetrievalPlan(scheme, P["cols"], P["bands"], P["lev"], P["y"], sun=P["sun"], **_twin_kw(P))
    assert plan.params == ("dir0", "dir1", "dir2", "lai", "leaf") and isinstance(plan.normal, batched.SpectralNormalSeriesPlan)
    costs = []
    for it in range(NSTEP):
        plan.step()
        torch.cuda.synchronize()
        state = {k: getattr(plan, k).cpu().numpy().copy() for k in STATE}
        ref = host.step()
        assert _same(state, ref), it
        costs.append(state["cost"])
    costs = np.stack(costs)
    truth = P["truth"].cpu().numpy()
    err, host_err = float(np.abs(state["p"] - truth).max()), float(np.abs(ref["p"] - truth).max())
    print(f"series twin {scheme}: parameter error plan {err:.3e}, host loop {host_err:.3e}; cost {costs[0].max():.3e} -> {costs[-1].max():.3e}; "
          f"accepted {state['naccept']}, rejected {state['nreject']}; {plan.normal.last_kernel()}")
    assert np.all(costs[1:] <= costs[:-1])
    assert err <= 10 * host_err, (err, host_err)


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
def test_fitted_nobs_covariance_and_one_shots():
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    P = _twin("2s")
    ncol, nt, nb = 4, P["sun"].nt, 40
    s = {"I_df_u": torch.ones_like(P["y"]["I_df_u"])}
    s["I_df_u"][1, 3] = 0.0  # a masked sun state of one column
    s["I_df_u"][2, :, :, :7] = 0.0
    plan = batched.SpectralRetrievalPlan("2s", P["cols"], P["bands"], P["lev"], P["y"], sun=P["sun"], inv_sigma=s, **_twin_kw(P)).run(6)
    fit = plan.fitted()
    assert set(fit) == {"I_df_u"} and fit["I_df_u"].shape == (ncol, nt, 1, nb) and bool(torch.isfinite(fit["I_df_u"]).all())
    want = torch.tensor([nt * nb, (nt - 1) * nb, nt * (nb - 7), nt * nb], dtype=torch.float64, device="cuda")
    assert torch.equal(plan.nobs(), want)
    cov, scaled = plan.covariance(), plan.covariance(scale=True)
    assert cov.shape == scaled.shape == (ncol, 5, 5)
    assert torch.allclose(scaled, cov * (2.0 * plan.cost / (want - 5))[:, None, None], rtol=1e-12, atol=0)
    res = batched.retrieve_spectral("2s", P["cols"], P["bands"], P["lev"], P["y"], sun=P["sun"], inv_sigma=s, niter=6, **_twin_kw(P))
    torch.cuda.synchronize()
    assert torch.equal(res["p"], plan.p) and torch.equal(res["cov"], cov) and res["params"] == plan.params
    sums = batched.spectral_normal_series("2s", P["cols"], P["bands"], P["sun"], P["lev"], P["y"], keys=P["keys"], lai=True, per_step=True)
    assert set(sums) == {"A", "g", "c2", "A_t", "g_t", "c2_t"} and sums["A"].shape == (ncol, 1) and sums["A_t"].shape == (ncol, nt, 1)
    assert bool((sums["c2"] > 0).all())
    # the model: the spectra of three sun angles, 3 % off, fitted by one direction and the LAI
    m = Model("2s", nlayers=12)
    psi = np.array([0.3, 0.6, 0.9])
    scheme, cols, b, sun = m._series_inputs(psi, None, None, "spectral retrieval")
    X = batched.solve_levels_series("2s", cols, b, sun, (-1,), keys=("I_df_u",))["I_df_u"][0].cpu().numpy()
    assert X.shape == (3, 1, m.nwl)
    y = {"I_df_u": 1.03 * X}
    d = np.random.default_rng(3).uniform(-0.05, 0.05, (1, m.nwl)) * m.copy_p()["leaf_r"]
    got = m.retrieve_spectral(y, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, psi=psi)
    assert got["params"] == ("dir0", "lai") and got["p"].shape == (2,) and got["cov"].shape == (2, 2) and np.isfinite(got["cost"])
    first = 0.5 * float(np.sum((0.03 / 1.03 * y["I_df_u"]) ** 2))
    assert got["cost"] < 0.5 * first  # (it did lower the cost of the starting point)
