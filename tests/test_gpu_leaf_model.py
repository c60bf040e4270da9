"""GPU: the plate model of leaf optics on the device (include_ext/crt1d_hip_leafmodel.h; batched.plate_leaf_optics, plate_leaf_ad and
``leaf_model=`` of the retrieval plans).  The oracle is tests/leaf_model_reference.py, pinned by tests/test_leaf_model_cpu.py.

1. Values and partials on the domain grid: values within 1e-11 (spectra are <= 1), each partial within 1e-11 * scale + 8 * spread --
   scale the largest magnitude of that parameter's leaf_r / leaf_t partial over the column, spread the reference's own
   complex128-minus-mpmath difference at that point, 8 the factor of tests/deriv_reference.py.
2. The clamps of k: finite, and bitwise the results at the clamp values.
3. Shapes where indexing can go wrong, against the complex-step reference alone: its own distance from mpmath is pinned at 1e-11 of
   scale (tests/test_leaf_model_cpu.py), so the bar is 1e-11 * scale for the device plus 1e-11 * scale for the reference.
4. Batch independence, bitwise.
5. The plumbing of the plans, bitwise against hand-made inputs.
6. - 8. Twin retrievals (spectral, sensor bands, sun series) against a host loop of the public pieces.
9. Autograd.  10. Model.retrieve_spectral is the batched call."""
import functools

import numpy as np
import pytest

import leaf_model_reference as R

pytestmark = pytest.mark.gpu

STATE = ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")
NSTEP = 25
SCALES = np.array([1.0, 40.0, 0.01, 0.005, 1.0])


def _t(v):
    import torch

    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


def _model(K, n, **kw):
    from crt1d_amd.leaf_model import PlateLeafModel

    return PlateLeafModel(K, n, **kw)


def _optics(model, q, **kw):
    import torch

    from crt1d_amd import batched

    out = batched.plate_leaf_optics(model, _t(q), **kw)
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() for v in out)


def _scale(d_r, d_t):
    return np.abs(np.stack([d_r, d_t])).max(axis=(0, 3))[:, :, None]  # [ncol][nm][1]


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_domain_values_and_partials():
    """Measured on MI355X: value error 5.8e-15; largest partial error 4.7e-12 of scale, 0.19 of the bar.  Without the partials the values
    keep their bits."""
    q, K, n = R.domain_grid()
    ref = R.reference(q, K, n)
    lr, lt, dr, dt = _optics(_model(K, n), q, partials=True)
    ev = max(np.abs(lr - ref["leaf_r"]).max(), np.abs(lt - ref["leaf_t"]).max())
    scale = _scale(ref["d_leaf_r"], ref["d_leaf_t"])
    ratio = max(float((np.abs(dr - ref["d_leaf_r"]) / (1e-11 * scale + 8 * ref["spread_r"])).max()),
                float((np.abs(dt - ref["d_leaf_t"]) / (1e-11 * scale + 8 * ref["spread_t"])).max()))
    rel = max(float((np.abs(dr - ref["d_leaf_r"]) / scale).max()), float((np.abs(dt - ref["d_leaf_t"]) / scale).max()))
    print(f"domain grid: value error {ev:.2e}; partial error {rel:.2e} of scale, {ratio:.3f} of the bar")
    assert np.all(np.isfinite(dr)) and np.all(np.isfinite(dt))
    assert ev <= 1e-11
    assert ratio <= 1.0
    lr2, lt2 = _optics(_model(K, n), q)  # without the partials: the same bits
    assert lr2.tobytes() == lr.tobytes() and lt2.tobytes() == lt.tobytes()


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1.0, 4.0])
def test_clamps(N):
    """K = 1 and N a power of two: k = C / N exactly.  k = 0, 1e-9 and 5e-7 give the bits of k = 1e-6; k = 700 those of k = 100 -- values
    and every row of the partials (the same K and N, hence the same chain factors on the same base partials)."""
    nb = 5
    K, n = np.ones((1, nb)), np.linspace(1.3, 1.6, nb)
    ks = np.array([0.0, 1e-9, 5e-7, 1e-6, 700.0, 100.0])
    q = np.stack([np.full(ks.size, N), ks * N], axis=1)
    assert np.array_equal(q[:, 1] / N, ks)
    out = _optics(_model(K, n), q, partials=True)
    for v in out:
        assert np.all(np.isfinite(v))
        for c in (0, 1, 2):
            assert v[c].tobytes() == v[3].tobytes(), c
        assert v[4].tobytes() == v[5].tobytes()
    ref = R.complex_step(q[[3, 5]], K, n)  # and those are the model at the clamp values (1e-9 of scale at k = 1e-6: the header)
    scale = _scale(ref[2], ref[3])
    assert np.abs(out[0][[3, 5]] - ref[0]).max() < 1e-11 and np.abs(out[1][[3, 5]] - ref[1]).max() < 1e-11
    assert (np.abs(out[2][[3, 5]] - ref[2]) / scale).max() < 1e-8 and (np.abs(out[3][[3, 5]] - ref[3]) / scale).max() < 1e-8


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nabs", [1, 7])
@pytest.mark.parametrize("ncol", [1, 3])
@pytest.mark.parametrize("nb", [1, 63, 65, 300, 500])  # 300: one-wave workgroups; 500: four-wave workgroups, a partial last wave
def test_shapes(nb, ncol, nabs):
    import torch

    from crt1d_amd import batched

    rng = np.random.default_rng(100 * nb + 10 * ncol + nabs)
    K = rng.uniform(1e-2, 2.0, (nabs, nb)) / nabs
    n = rng.uniform(1.3, 1.6, nb)
    q = np.concatenate([rng.uniform(1.0, 4.0, (ncol, 1)), rng.uniform(1.0, 4.0, (ncol, nabs))], axis=1)  # k in [2.5e-3, 8]
    nm = 1 + nabs
    model = _model(K, n)
    ref = R.complex_step(q, K, n)
    scale = _scale(ref[2], ref[3])
    ntan = min(nm + 1, 8)
    out = {"leaf_r": torch.full((ncol, nb), -7.0, dtype=torch.float64, device="cuda"), "leaf_t": torch.full((ncol, nb), -7.0, dtype=torch.float64, device="cuda"),
           "d_leaf_r": torch.full((ncol, ntan, nb), -7.0, dtype=torch.float64, device="cuda"),
           "d_leaf_t": torch.full((ncol, ntan, nb), -7.0, dtype=torch.float64, device="cuda")}
    got = batched.plate_leaf_optics(model, _t(q), partials=False, out=out)
    torch.cuda.synchronize()
    assert len(got) == 2 and got[0] is out["leaf_r"]
    assert bool((out["d_leaf_r"] == -7.0).all()) and bool((out["d_leaf_t"] == -7.0).all())  # partials=False writes nothing there
    first = [out[k].cpu().numpy().copy() for k in ("leaf_r", "leaf_t")]
    got = batched.plate_leaf_optics(model, _t(q), partials=True, out=out)
    torch.cuda.synchronize()
    lr, lt, dr, dt = (v.cpu().numpy() for v in got)
    assert lr.tobytes() == first[0].tobytes() and lt.tobytes() == first[1].tobytes()
    assert np.abs(lr - ref[0]).max() <= 1e-11 and np.abs(lt - ref[1]).max() <= 1e-11
    assert (np.abs(dr[:, :nm] - ref[2]) / scale).max() <= 2e-11 and (np.abs(dt[:, :nm] - ref[3]) / scale).max() <= 2e-11
    assert np.all(dr[:, nm:] == -7.0) and np.all(dt[:, nm:] == -7.0)  # the rows beyond nm keep the sentinel
    free = batched.plate_leaf_optics(model, _t(q), partials=True)  # arrays of its own: (ncol, nm, nb)
    torch.cuda.synchronize()
    assert tuple(free[2].shape) == (ncol, nm, nb) and free[2].cpu().numpy().tobytes() == np.ascontiguousarray(dr[:, :nm]).tobytes()
    with pytest.raises(ValueError):
        batched.plate_leaf_optics(model, _t(q[:, :-1]))


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_independence():
    q, K, n = R.domain_grid()
    model = _model(K, n)
    full = _optics(model, q, partials=True)
    part = _optics(model, q[1:3], partials=True)
    for a, b in zip(full, part):
        assert np.ascontiguousarray(a[1:3]).tobytes() == b.tobytes()


# ---- the twin problem -------------------------------------------------------------------------------------------------------------------
def _gauss(wl, c, w):
    return np.exp(-0.5 * ((wl - c) / w) ** 2)


@functools.lru_cache(maxsize=None)
def _twin():
    """The twin of the issue: 4 columns, 40 bands, 12 levels, 2s, I_df_u observed at level -1 and I_df_d at level 0; the unknowns
    (N, C_0, C_1, C_2, ln LAI scale).  Holds the host loop of plate_leaf_optics + spectral_normal + gauss_newton_step, run once."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nb, nz = 4, 40, 12
    d = synth.make_columns(ncol, nb, nz, seed=5)
    wl = np.linspace(0.45, 2.4, nb)
    n = 1.5 - 0.06 * (wl - 0.45) / 1.95
    K = np.stack([0.06 * _gauss(wl, 0.45, 0.08) + 0.05 * _gauss(wl, 0.67, 0.03),
                  40 * _gauss(wl, 1.45, 0.06) + 60 * _gauss(wl, 1.94, 0.07) + 20 * _gauss(wl, 2.4, 0.15) + 0.5 * _gauss(wl, 0.97, 0.04),
                  8 + 30 * _gauss(wl, 2.2, 0.3) + 20 * _gauss(wl, 0.45, 0.2)])
    model = _model(K, n, names=("cab", "cw", "cm"))
    rng = np.random.default_rng(41)
    truth = np.stack([rng.uniform(1.2, 2.2, ncol), rng.uniform(25, 60, ncol), rng.uniform(0.008, 0.02, ncol), rng.uniform(0.003, 0.01, ncol),
                      rng.uniform(-0.2, 0.2, ncol)], axis=1)
    u = np.random.default_rng(7).uniform(-1, 1, (4, 5))
    p0 = truth * (1 + 0.15 * u)
    p0[:, 4] = truth[:, 4] + 0.15 * u[:, 4]
    lo, hi = np.array([1.0, 0.0, 0.0, 0.0, -np.inf]), np.array([4.0, np.inf, np.inf, np.inf, np.inf])
    cols, bands = batched.Columns.from_host(d, "cuda"), batched.Bands.from_host(d, "cuda")
    lev, keys = (0, -1), ("I_df_d", "I_df_u")
    mask = {"I_df_d": torch.zeros((ncol, 2, nb), dtype=torch.float64, device="cuda"), "I_df_u": torch.zeros((ncol, 2, nb), dtype=torch.float64, device="cuda")}
    mask["I_df_d"][:, 0] = 1.0  # level 0: the ground
    mask["I_df_u"][:, 1] = 1.0  # level -1: the top
    zero = {k: torch.zeros((ncol, 2, nb), dtype=torch.float64, device="cuda") for k in keys}

    def inputs(p):
        lr, lt, dr, dt = batched.plate_leaf_optics(model, p[:, :4].contiguous(), partials=True)
        c = batched.Columns(cols.psi, cols.lai * torch.exp(p[:, 4])[:, None], cols.g_kind, cols.g_param, cols.mla)
        return c, batched.Bands(bands.I_dr0, bands.I_df0, lr, lt, bands.soil_r), dr, dt

    def normal(p, y, fwd=False):
        c, b, dr, dt = inputs(p)
        return batched.spectral_normal("2s", c, b, lev, y, keys=keys, inv_sigma=mask, d_leaf_r=dr, d_leaf_t=dt, lai=True, fwd=fwd)

    y = {k: v.clone() for k, v in normal(_t(truth), zero, fwd=True)["fwd"].items()}

    def step(o, lam):  # (A + lam diag A) delta = -g through gauss_newton_step: J = L^T of A = L L^T, r = L^-1 g
        i, j = np.tril_indices(5)
        A = torch.zeros((ncol, 5, 5), dtype=torch.float64, device="cuda")
        A[:, i, j] = o["A"]
        A[:, j, i] = o["A"]
        L = torch.linalg.cholesky(A)
        r = torch.linalg.solve_triangular(L, o["g"][:, :, None], upper=False)[:, :, 0]
        return batched.gauss_newton_step(L.transpose(1, 2).contiguous(), r, damping=lam)

    p = _t(p0)
    tlo, thi = _t(lo), _t(hi)
    lam = torch.full((ncol,), 1e-2, dtype=torch.float64, device="cuda")
    o = {k: v.clone() for k, v in normal(p, y).items()}
    hist = [0.5 * o["c2"]]
    for _ in range(NSTEP - 1):
        trial = torch.minimum(torch.maximum(p + step(o, lam), tlo), thi)
        ot = normal(trial, y)
        better = 0.5 * ot["c2"] < hist[-1]
        p = torch.where(better[:, None], trial, p)
        o = {k: torch.where(better.reshape(-1, *[1] * (v.ndim - 1)), ot[k], v) for k, v in o.items()}
        lam = torch.where(better, (lam / 10).clamp_min(1e-12), lam * 10)
        hist.append(0.5 * o["c2"])
    torch.cuda.synchronize()
    host_error = float((np.abs(p.cpu().numpy() - truth) / SCALES).max())
    return dict(cols=cols, bands=bands, model=model, truth=truth, p0=p0, lo=lo, hi=hi, lev=lev, keys=keys, mask=mask, y=y, inputs=inputs,
                host_error=host_error, host_hist=torch.stack(hist).cpu().numpy(), d=d, K=K, n=n)


def _spectral_plan(P, cols=slice(None), **kw):
    from crt1d_amd import batched

    c, b = P["cols"], P["bands"]
    if cols != slice(None):
        c, b = c.slice(cols.start, cols.stop), b.slice(cols.start, cols.stop)
    kw.setdefault("y", {k: v[cols] for k, v in P["y"].items()})
    kw.setdefault("inv_sigma", {k: v[cols] for k, v in P["mask"].items()})
    y = kw.pop("y")
    return batched.SpectralRetrievalPlan("2s", c, b, P["lev"], y, keys=P["keys"], lai=True, leaf_model=P["model"], p0=P["p0"][cols], lo=P["lo"],
                                         hi=P["hi"], lam0=1e-2, lam_up=10.0, lam_down=0.1, xtol=0.0, ftol=0.0, **kw)


def _state(plan):
    import torch

    torch.cuda.synchronize()
    return {k: getattr(plan, k).cpu().numpy().copy() for k in STATE}


def _run_and_check(P, plan, label, host_error, host_hist):
    """NSTEP single steps: the cost never increases, ends below 1e-12 of the first, and the parameter error (relative to SCALES) is at
    most 10 x the host loop's.  -> the final state"""
    costs = []
    for _ in range(NSTEP):
        costs.append(plan.step().cost.clone())
    state = _state(plan)
    costs = np.stack([c.cpu().numpy() for c in costs])
    err = float((np.abs(state["p"] - P["truth"]) / SCALES).max())
    print(f"{label}: parameter error plan {err:.3e}, host loop {host_error:.3e}; cost {costs[0].max():.3e} -> {costs[-1].max():.3e} "
          f"(host loop {host_hist[0].max():.3e} -> {host_hist[-1].max():.3e}); accepted {state['naccept']}, rejected {state['nreject']}")
    assert np.all(costs[1:] <= costs[:-1])
    assert costs[-1].max() < 1e-12 * costs[0].max()
    assert err <= 10 * host_error, (err, host_error)
    return state


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
def _handmade(P, plan, soil_dir):
    """The inputs of one evaluation at p0 made by hand: plate_leaf_optics for the spectra, its partials and the soil direction as
    per-column directions, the soil coefficient, the LAI scale (the plan's own exp) and g_param applied."""
    import torch

    from crt1d_amd import batched

    ncol, nb = 4, 40
    p0 = plan._p0
    lr, lt, dr, dt = batched.plate_leaf_optics(P["model"], p0[:, :4].contiguous(), partials=True)
    z = lambda: torch.zeros((ncol, 5, nb), dtype=torch.float64, device="cuda")  # noqa: E731
    d_r, d_t, d_s = z(), z(), z()
    d_r[:, :4], d_t[:, :4], d_s[:, 4] = dr, dt, soil_dir
    soil = P["bands"].soil_r + p0[:, 4, None] * soil_dir[None]
    c = P["cols"]
    cols = batched.Columns(c.psi, c.lai * plan.lai_scale[:, None], c.g_kind, p0[:, 6].contiguous(), c.mla)
    bands = batched.Bands(P["bands"].I_dr0, P["bands"].I_df0, lr, lt, soil)
    return cols, bands, dict(d_leaf_r=d_r, d_leaf_t=d_t, d_soil_r=d_s, lai=True, tangent=batched.leaf_tangent(cols, "param"))


def test_plumbing_bitwise():
    """After one step() of a plan with leaf_model (nm = 4 model parameters, one soil direction, ln LAI, the leaf angle) the normal plan's
    A, g, c2 are bitwise batched.spectral_normal on hand-made inputs; the Jacobian of a RetrievalPlan likewise batched.sensor_jacobian."""
    import torch

    from crt1d_amd import batched

    P = _twin()
    soil_dir = _t(0.1 * P["d"]["soil_r"].mean(axis=0))
    p0 = np.concatenate([P["p0"][:, :4], np.full((4, 1), 0.3), P["p0"][:, 4:], P["d"]["g_param"][:, None]], axis=1)
    lo, hi = np.concatenate([P["lo"][:4], [-1.0, -1.0, 0.2]]), np.concatenate([P["hi"][:4], [1.0, 1.0, 5.0]])
    plan = batched.SpectralRetrievalPlan("2s", P["cols"], P["bands"], P["lev"], P["y"], keys=P["keys"], inv_sigma=P["mask"], d_soil_r=soil_dir[None],
                                         lai=True, leaf=True, leaf_model=P["model"], p0=p0, lo=lo, hi=hi)
    assert plan.params == ("N", "cab", "cw", "cm", "dir0", "lai", "leaf") and plan.npar == 7
    plan.step()
    torch.cuda.synchronize()
    assert bool((plan._leaf.d_leaf_r[:, 4:] == 0).all()) and bool((plan._leaf.d_soil_r[:, :4] == 0).all())
    cols, bands, kw = _handmade(P, plan, soil_dir)
    ref = batched.spectral_normal("2s", cols, bands, P["lev"], P["y"], keys=P["keys"], inv_sigma=P["mask"], **kw)
    torch.cuda.synchronize()
    for k in ("A", "g", "c2"):
        assert plan.normal.out[k].cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), k
    assert np.array_equal(plan.cost.cpu().numpy(), 0.5 * ref["c2"].cpu().numpy())
    fit = plan.fitted()  # the accepted point is p0: the model spectra of the hand-made inputs
    fwd = batched.spectral_normal("2s", cols, bands, P["lev"], P["y"], keys=P["keys"], inv_sigma=P["mask"], fwd=True, **kw)["fwd"]
    torch.cuda.synchronize()
    for k in P["keys"]:
        assert fit[k].cpu().numpy().tobytes() == fwd[k].cpu().numpy().tobytes(), k

    sens = batched.SensorSet.from_supports(np.arange(8) * 5, np.full(8, 5), np.ones(40), nb=40)
    ys = {k: torch.ones((4, 2, 8), dtype=torch.float64, device="cuda") for k in P["keys"]}
    rp = batched.RetrievalPlan("2s", P["cols"], P["bands"], P["lev"], sens, ys, keys=P["keys"], d_soil_r=soil_dir[None], lai=True, leaf=True,
                               leaf_model=P["model"], p0=p0, lo=lo, hi=hi)
    assert rp.params == plan.params
    rp.step()
    torch.cuda.synchronize()
    cols, bands, kw = _handmade(P, rp, soil_dir)
    ref = batched.sensor_jacobian("2s", cols, bands, P["lev"], sens, keys=P["keys"], **kw)
    fwd = batched.solve_sensor_levels("2s", cols, bands, P["lev"], sens, keys=P["keys"])
    torch.cuda.synchronize()
    for k in P["keys"]:
        assert rp.jac.out[k].cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), k
        assert float((rp.fwd.out[k] - fwd[k]).abs().max()) <= 1e-11 * float(fwd[k].abs().max())


def test_plumbing_bl():
    """bl has no soil: the apply entry is given a zero direction array.  After one step the sums are bitwise spectral_normal on hand-made
    inputs, and the leaf rows of the plan are the model's partials."""
    import torch

    from crt1d_amd import batched

    P = _twin()
    c, b0 = P["cols"], P["bands"]
    bands = batched.Bands(b0.I_dr0, b0.I_df0, b0.leaf_r, b0.leaf_t, None)
    lev, keys = (0, 6), ("I_dr", "I_df_d")
    y = {k: torch.full((4, 2, 40), 0.3, dtype=torch.float64, device="cuda") for k in keys}
    plan = batched.SpectralRetrievalPlan("bl", c, bands, lev, y, keys=keys, lai=True, leaf_model=P["model"], p0=P["p0"], lo=P["lo"], hi=P["hi"])
    plan.step()
    lr, lt, dr, dt = batched.plate_leaf_optics(P["model"], plan._p0[:, :4].contiguous(), partials=True)
    cols = batched.Columns(c.psi, c.lai * plan.lai_scale[:, None], c.g_kind, c.g_param, c.mla)
    ref = batched.spectral_normal("bl", cols, batched.Bands(b0.I_dr0, b0.I_df0, lr, lt, None), lev, y, keys=keys, d_leaf_r=dr, d_leaf_t=dt, lai=True)
    torch.cuda.synchronize()
    assert torch.equal(plan._leaf.d_leaf_r, dr) and torch.equal(plan._leaf.d_leaf_t, dt)
    assert torch.equal(plan.bands.leaf_r, lr) and torch.equal(plan.bands.leaf_t, lt)
    for k in ("A", "g", "c2"):
        assert plan.normal.out[k].cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), k
    assert bool(torch.isfinite(plan.cost).all())


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
def test_twin_retrieval_spectral():
    """Measured on MI355X after 25 steps, largest parameter error relative to SCALES: plan 1.1e-14, host loop 7.8e-15; largest column cost
    9.4e-01 -> 1.8e-29 (host loop -> 3.2e-29).  reset().run(25) repeats the bits; columns 0-1 alone have their batch bits."""
    P = _twin()
    plan = _spectral_plan(P)
    assert plan.params == ("N", "cab", "cw", "cm", "lai")
    state = _run_and_check(P, plan, "twin spectral", P["host_error"], P["host_hist"])
    assert np.all(state["status"] == 0)
    again = _state(plan.reset().run(NSTEP))
    assert all(again[k].tobytes() == state[k].tobytes() for k in STATE)
    two = _state(_spectral_plan(P, cols=slice(0, 2)).run(NSTEP))
    assert all(two[k].tobytes() == state[k][:2].tobytes() for k in STATE)
    fit = plan.fitted()
    for k in P["keys"]:
        m = P["mask"][k]
        assert float(((fit[k] - P["y"][k]) * m).abs().max()) <= 1e-9 * float(P["y"][k].abs().max())


# ---- 7. ---------------------------------------------------------------------------------------------------------------------------------
def test_twin_retrieval_sensor_bands():
    """The same problem through RetrievalPlan: eight boxcar sensor bands of five spectral bands each, both keys; the host loop is
    plate_leaf_optics + sensor_jacobian + solve_sensor_levels + gauss_newton_step with the same lambda schedule.  Measured on MI355X after
    25 steps: plan 3.2e-14, host loop 2.5e-14; cost 3.8e+00 -> 8.7e-29 (host loop -> 5.7e-29)."""
    import torch

    from crt1d_amd import batched

    P = _twin()
    ncol = 4
    sens = batched.SensorSet.from_supports(np.arange(8) * 5, np.full(8, 5), np.ones(40), nb=40)
    ms = {k: v[:, :, :8].contiguous() for k, v in P["mask"].items()}  # (ncol, nsel, nsens): the same levels observed

    def evaluate(p):  # -> (r, J) over the observed rows: I_df_d at level 0, I_df_u at level -1
        c, b, dr, dt = P["inputs"](p)
        f = batched.solve_sensor_levels("2s", c, b, P["lev"], sens, keys=P["keys"])
        J = batched.sensor_jacobian("2s", c, b, P["lev"], sens, keys=P["keys"], d_leaf_r=dr, d_leaf_t=dt, lai=True)
        return (torch.cat([f["I_df_d"][:, 0], f["I_df_u"][:, 1]], dim=1).clone(), torch.cat([J["I_df_d"][:, 0], J["I_df_u"][:, 1]], dim=1).clone())

    ft, _ = evaluate(_t(P["truth"]))
    y = {"I_df_d": torch.zeros((ncol, 2, 8), dtype=torch.float64, device="cuda"), "I_df_u": torch.zeros((ncol, 2, 8), dtype=torch.float64, device="cuda")}
    y["I_df_d"][:, 0], y["I_df_u"][:, 1] = ft[:, :8], ft[:, 8:]
    p, tlo, thi = _t(P["p0"]), _t(P["lo"]), _t(P["hi"])
    lam = torch.full((ncol,), 1e-2, dtype=torch.float64, device="cuda")
    f, J = evaluate(p)
    r = f - ft
    hist = [0.5 * (r * r).sum(1)]
    for _ in range(NSTEP - 1):
        trial = torch.minimum(torch.maximum(p + batched.gauss_newton_step(J, r, damping=lam), tlo), thi)
        f2, J2 = evaluate(trial)
        r2 = f2 - ft
        better = 0.5 * (r2 * r2).sum(1) < hist[-1]
        p, r, J = torch.where(better[:, None], trial, p), torch.where(better[:, None], r2, r), torch.where(better[:, None, None], J2, J)
        lam = torch.where(better, (lam / 10).clamp_min(1e-12), lam * 10)
        hist.append(0.5 * (r * r).sum(1))
    torch.cuda.synchronize()
    host_error = float((np.abs(p.cpu().numpy() - P["truth"]) / SCALES).max())
    plan = batched.RetrievalPlan("2s", P["cols"], P["bands"], P["lev"], sens, y, keys=P["keys"], inv_sigma=ms, lai=True, leaf_model=P["model"],
                                 p0=P["p0"], lo=P["lo"], hi=P["hi"], lam0=1e-2, lam_up=10.0, lam_down=0.1, xtol=0.0, ftol=0.0)
    _run_and_check(P, plan, "twin sensor bands", host_error, torch.stack(hist).cpu().numpy())


# ---- 8. ---------------------------------------------------------------------------------------------------------------------------------
def test_sun_series():
    """A one-state SunSeries reproduces the per-step plan's state bitwise; with two sun states the plan runs and its cost is monotone
    (measured on MI355X: 1.8e+00 -> 5.7e-29 in 12 steps)."""
    import torch

    from crt1d_amd import batched

    P = _twin()
    c, b = P["cols"], P["bands"]
    one = batched.SunSeries(c.psi[:, None].contiguous(), b.I_dr0[:, None].contiguous(), b.I_df0[:, None].contiguous())
    plan = _spectral_plan(P, sun=one, y={k: v[:, None].contiguous() for k, v in P["y"].items()},
                          inv_sigma={k: v[:, None].contiguous() for k, v in P["mask"].items()})
    ref = _state(_spectral_plan(P).run(6))
    got = _state(plan.run(6))
    assert all(got[k].tobytes() == ref[k].tobytes() for k in STATE)

    psi2 = torch.stack([c.psi, 0.6 * c.psi + 0.2], dim=1).contiguous()
    two = batched.SunSeries(psi2, torch.stack([b.I_dr0, 0.8 * b.I_dr0], dim=1).contiguous(), torch.stack([b.I_df0, 1.1 * b.I_df0], dim=1).contiguous())
    mask = {k: torch.stack([v, v], dim=1).contiguous() for k, v in P["mask"].items()}
    zero = {k: torch.zeros_like(v) for k, v in mask.items()}
    truth = _spectral_plan(P, sun=two, y=zero, inv_sigma=mask)
    truth.reset(_t(P["truth"])).step()
    y = truth.fitted()
    plan = _spectral_plan(P, sun=two, y=y, inv_sigma=mask)
    costs = []
    for _ in range(12):
        costs.append(plan.step().cost.clone())
    torch.cuda.synchronize()
    costs = np.stack([v.cpu().numpy() for v in costs])
    print(f"two sun states: cost {costs[0].max():.3e} -> {costs[-1].max():.3e}")
    assert np.all(np.isfinite(costs)) and np.all(costs[1:] <= costs[:-1]) and np.all(costs[-1] < costs[0])


# ---- 9. ---------------------------------------------------------------------------------------------------------------------------------
def test_autograd():
    import torch

    from crt1d_amd import batched

    rng = np.random.default_rng(9)
    nb = 7
    K = np.stack([np.linspace(1e-2, 1.0, nb), np.linspace(1.0, 1e-2, nb)])
    model = _model(K, np.linspace(1.35, 1.55, nb))
    q = _t(np.stack([rng.uniform(1.2, 3.0, 2), rng.uniform(0.6, 1.0, 2), rng.uniform(0.6, 1.0, 2)], axis=1)).requires_grad_(True)  # k in [1e-2, 2]
    assert torch.autograd.gradcheck(lambda v: batched.plate_leaf_ad(model, v), (q,), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)
    lr, lt = batched.plate_leaf_ad(model, q)
    ref = batched.plate_leaf_optics(model, q.detach(), partials=True)
    assert torch.equal(lr, ref[0]) and torch.equal(lt, ref[1])
    (2.0 * lr.sum() + lt.sum()).backward()
    assert torch.allclose(q.grad, 2.0 * ref[2].sum(2) + ref[3].sum(2), rtol=1e-12, atol=1e-14)


# ---- 10. --------------------------------------------------------------------------------------------------------------------------------
def test_model_retrieve_spectral():
    """Model.retrieve_spectral(..., leaf_model=...) is the batched call on the model's own column: bitwise."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=12)
    nb = m.nwl
    wl = np.linspace(0.0, 1.0, nb)
    lm = _model(np.stack([0.05 * _gauss(wl, 0.2, 0.1), 8.0 + 20.0 * wl]), 1.5 - 0.05 * wl, names=("cab", "cm"))
    scheme, cols, b, sun = m._series_inputs(np.atleast_1d(float(m._p["psi"])), None, None, "spectral retrieval")
    cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
    b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
    y = {"I_df_u": 1.03 * batched.solve_levels("2s", cols, b, (-1,), keys=("I_df_u",))["I_df_u"][0].cpu().numpy()}
    kw = dict(p0=np.array([1.6, 30.0, 0.006, 0.0]), lo=np.array([1.0, 0.0, 0.0, -2.0]), hi=np.array([4.0, 200.0, 1.0, 2.0]))
    got = m.retrieve_spectral(y, levels=(-1,), lai=True, niter=6, leaf_model=lm, **kw)
    assert got["params"] == ("N", "cab", "cm", "lai") and got["p"].shape == (4,) and np.isfinite(got["cost"])
    ref = batched.retrieve_spectral("2s", cols, b, (-1,), {"I_df_u": y["I_df_u"][None]}, keys=("I_df_u",), niter=6, lai=True, leaf_model=lm, **kw)
    torch.cuda.synchronize()
    for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
        assert got[k].tobytes() == ref[k][0].cpu().numpy().tobytes(), k
