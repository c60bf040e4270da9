"""GPU: ``evaluate=`` and ``check_every=`` of the retrieval plans (include_mask/crt1d_hip_masked.h).

Noise-free twins: the observations are the plan's own forward result at a truth, the truths are spread over the box so that the units
(columns; with a chain: pixels) finish at different iterations, and unit 0 starts at its truth, so it stops at the first step.  Three
plans of one problem -- ``evaluate="all"`` (the plan as it was), ``"running"`` and, where it is served, ``"accepted"`` -- are stepped
side by side, and after EVERY step all of p, p_trial, cost, lam, A, g, status, naccept and nreject are bitwise equal.

So that the comparison cannot be vacuous, the ``"all"`` run (existing code) must show: a unit that stopped at least 3 steps before the
last step while another unit was still running at the last-but-third step, and a rejection after the first step.

Then ``run(60, check_every=3)`` against ``run(60)``, and ``covariance()`` / ``fitted()`` between the modes.

Variants: RetrievalPlan per step, with ``sun=``, with ``leaf_model=``, with ``chain=3``, with ``chain=3, shared=``; SpectralRetrievalPlan
per step, with ``sun=``, with ``chain=3``.  12 columns (4 pixels of 3 dates), 30 bands, 12 levels; 2s.  (bl has no upward stream to
observe at the canopy top; its masked kernels are held to the plain ones in tests/test_gpu_masked.py.)

Measured on MI355X, the "all" runs: the step after which each unit stopped (None: still running after 14) / its rejections.
  sensor               1 7 7 None None 5 9 4 12 None 6 6 / 0 0 0 6 8 0 0 0 2 9 0 0
  sensor-sun           1 6 5 7 7 6 8 5 5 None 12 6 / 0 0 0 0 0 0 0 0 0 9 5 0
  sensor-leaf-model    9 None x 11 / 8 5 3 6 5 7 6 7 7 7 6 5
  sensor-chain         1 None None None / 0 0 7 5          sensor-chain-shared  1 None None 14 / 0 0 5 4
  spectral             1 7 7 7 6 6 13 5 6 6 14 5 / 0 0 0 0 0 0 4 0 0 0 6 0
  spectral-sun         1 7 10 6 5 7 6 7 5 None 11 7 / 0 0 0 0 0 0 0 0 0 11 0 0
  spectral-chain       1 None None None / 0 9 0 6"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")
NSTEP = 14
NCOL, NB, NZ, ND, NT = 12, 30, 12, 3, 3
ELLIPSOIDAL = 3
OPTS = dict(lam0=1e-4, lam_up=10.0, lam_down=0.1, xtol=1e-9, ftol=0.0)
VARIANTS = ("sensor", "sensor-sun", "sensor-leaf-model", "sensor-chain", "sensor-chain-shared", "spectral", "spectral-sun", "spectral-chain")
# The leaf-model twin is so well conditioned that with a step tolerance every column converges within 8 steps without a rejection.  It runs
# without tolerances instead: unit 0, which starts at its truth, proposes its own point again from the second step on (cost_t == cost is
# a rejection), its damping passes lam_max = 1e2 at the ninth step and it stops as STALLED; the other units run on.
VARIANT_OPTS = {"sensor-leaf-model": dict(xtol=0.0, lam_max=1e2)}


def _t(v):
    import torch

    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


def _gauss(x, c, w):
    return np.exp(-0.5 * ((x - c) / w) ** 2)


@functools.lru_cache(maxsize=None)
def _base():
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(NCOL, NB, NZ, seed=5)
    rng = np.random.default_rng(41)
    kind = torch.full((NCOL,), ELLIPSOIDAL, dtype=torch.int32, device="cuda")
    x0 = torch.full((NCOL,), 1.2, dtype=torch.float64, device="cuda")
    cols = batched.Columns(_t(d["psi"]), _t(d["lai"]), kind, x0, _t(d["mla"]))
    bands = batched.Bands(_t(d["I_dr0"]), _t(d["I_df0"]), _t(d["leaf_r"]), _t(d["leaf_t"]), _t(d["soil_r"]))
    psi = np.deg2rad([22.0, 45.0, 64.0])[None, :] + np.deg2rad(rng.uniform(-2.0, 2.0, (NCOL, 1)))
    sun = batched.SunSeries(_t(psi), _t(d["I_dr0"][:, None, :] * np.cos(psi)[:, :, None]), _t(np.repeat(d["I_df0"][:, None, :], NT, axis=1)))
    w = np.zeros((5, NB))
    for s in range(5):
        w[s, 6 * s:6 * s + 6] = np.hanning(8)[1:7]
    dirn = _t(0.3 * d["leaf_r"].mean(axis=0) * np.sin(np.linspace(0.0, 3.0, NB)))
    wl = np.linspace(0.45, 2.4, NB)
    K = np.stack([0.06 * _gauss(wl, 0.45, 0.08) + 0.05 * _gauss(wl, 0.67, 0.03),
                  40 * _gauss(wl, 1.45, 0.06) + 60 * _gauss(wl, 1.94, 0.07) + 20 * _gauss(wl, 2.4, 0.15) + 0.5 * _gauss(wl, 0.97, 0.04),
                  8 + 30 * _gauss(wl, 2.2, 0.3) + 20 * _gauss(wl, 0.45, 0.2)])
    torch.cuda.synchronize()
    return dict(cols=cols, bands=bands, sun=sun, sensors=batched.SensorSet(w), dirn=dirn, K=K, n=1.5 - 0.06 * (wl - 0.45) / 1.95)


def _points(variant):
    """(p0, truth, lo, hi): the truths fill the box; unit 0 (a chain: every date of pixel 0) starts at its truth."""
    rng = np.random.default_rng(sum(map(ord, variant)))
    if "leaf-model" in variant:  # N, cab, cw, cm, ln LAI scale
        truth = np.stack([rng.uniform(1.2, 2.6, NCOL), rng.uniform(20, 70, NCOL), rng.uniform(0.006, 0.025, NCOL), rng.uniform(0.003, 0.012, NCOL),
                          rng.uniform(-0.5, 0.5, NCOL)], axis=1)
        p0 = np.tile(np.array([1.8, 40.0, 0.012, 0.006, 0.0]), (NCOL, 1))
        lo, hi = np.array([1.0, 0.0, 0.0, 0.0, -2.0]), np.array([4.0, 200.0, 0.1, 0.1, 2.0])
    else:  # one leaf-reflectance coefficient, ln LAI scale, the ellipsoidal x
        truth = np.stack([rng.uniform(-0.3, 0.3, NCOL), rng.uniform(-0.9, 0.9, NCOL), rng.uniform(0.4, 3.5, NCOL)], axis=1)
        p0 = np.tile(np.array([0.0, 0.0, 1.2]), (NCOL, 1))
        lo, hi = np.array([-0.5, -1.5, 0.2]), np.array([0.5, 1.5, 5.0])
    n0 = ND if "chain" in variant else 1
    truth[:n0] = p0[:n0]
    if "shared" in variant:  # the ln LAI scale is a constant of the pixel
        truth[:, 1] = np.repeat(truth[::ND, 1], ND)
    return p0, truth, lo, hi


def _plan(variant, evaluate, y=None, start=None, **opts):
    """The plan of ``variant``; y None: observations of zeros (the caller wants the forward result at ``start``)."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.leaf_model import PlateLeafModel

    B = _base()
    p0, truth, lo, hi = _points(variant)
    scheme, bands = "2s", B["bands"]
    kw = dict(OPTS, p0=_t(p0 if start is None else start), lo=lo, hi=hi, evaluate=evaluate)
    kw.update(VARIANT_OPTS.get(variant, {}))
    kw.update(opts)
    if "sun" in variant:
        kw["sun"] = B["sun"]
    nts = (NT,) if "sun" in variant else ()
    if "chain" in variant:
        kw.update(chain=ND, inv_sigma_chain=np.full((ND - 1, p0.shape[1]), 0.5))
    if "shared" in variant:
        kw["shared"] = ("lai",)
    if "leaf-model" in variant:
        kw.update(leaf_model=PlateLeafModel(B["K"], B["n"], names=("cab", "cw", "cm")), lai=True)
    else:
        kw.update(d_leaf_r=B["dirn"][None], lai=True, leaf=True)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    if variant.startswith("sensor"):
        lev, keys = ((0, NZ - 1), ("I_df_d", "I_df_u")) if "leaf-model" in variant else ((NZ - 1,), ("I_df_u",))
        y = y or {k: zeros(NCOL, *nts, len(lev), 5) for k in keys}
        return batched.RetrievalPlan(scheme, B["cols"], bands, lev, B["sensors"], y, keys=keys, **kw)
    y = y or {"I_df_u": zeros(NCOL, *nts, 1, NB)}
    return batched.SpectralRetrievalPlan(scheme, B["cols"], bands, (NZ - 1,), y, keys=("I_df_u",), **kw)


@functools.lru_cache(maxsize=None)
def _twin(variant):
    """The observations: the forward result of the plan itself at the truth (one step of a plan that starts there)."""
    import torch

    _, truth, _, _ = _points(variant)
    plan = _plan(variant, "all", start=truth)
    if variant.startswith("sensor"):
        plan.step()
        y = {k: v.clone() for k, v in plan.fwd.out.items()}
    else:
        y = plan.fitted()
    torch.cuda.synchronize()
    return y


def _state(plan):
    import torch

    torch.cuda.synchronize()
    return {k: getattr(plan, k).cpu().numpy().copy() for k in STATE}


def _modes(variant):
    return ("all", "running", "accepted") if variant in ("sensor", "sensor-sun", "sensor-leaf-model") else ("all", "running")


@pytest.mark.parametrize("variant", VARIANTS)
def test_modes_are_bitwise_the_plan_as_it_was(variant):
    y = _twin(variant)
    plans = {m: _plan(variant, m, y) for m in _modes(variant)}
    status, nreject = [], []
    for step in range(NSTEP):
        states = {m: _state(p.step()) for m, p in plans.items()}
        for m in plans:
            for k in STATE:
                assert states[m][k].tobytes() == states["all"][k].tobytes(), (variant, m, "step", step, k)
        status.append(states["all"]["status"]), nreject.append(states["all"]["nreject"])
    status, nreject = np.stack(status), np.stack(nreject)
    print(f"{variant}: stopped after step {[(int(np.argmax(status[:, u] != 0)) + 1 if status[-1, u] else None) for u in range(status.shape[1])]}, "
          f"rejections {nreject[-1].tolist()}, in the first step {nreject[0].tolist()}")
    # the condition, on the run of the existing code
    assert np.any(status[NSTEP - 4] != 0) and np.any(status[NSTEP - 4] == 0), "a unit stopped 3 steps before the last while another still ran"
    assert np.any(nreject[-1] > nreject[0]) and np.all(nreject[0] == 0), "a rejection after the first step"
    assert all(p.nsteps == NSTEP for p in plans.values())
    covs = {m: p.covariance().cpu().numpy() for m, p in plans.items()}
    for m in plans:
        assert covs[m].tobytes() == covs["all"].tobytes(), (variant, m, "covariance")
    if variant.startswith("spectral"):
        fits = {m: {k: v.cpu().numpy() for k, v in p.fitted().items()} for m, p in plans.items()}
        for m in plans:
            assert all(fits[m][k].tobytes() == fits["all"][k].tobytes() for k in fits["all"]), (variant, m, "fitted")
        assert all(np.all(np.isfinite(v)) for v in fits["running"].values())  # (every column is evaluated, the stopped ones too)


@pytest.mark.parametrize("variant", ["sensor-sun", "sensor-chain", "spectral"])
def test_check_every_ends_early_with_the_same_result(variant):
    """xtol = 1e-5, with which the last unit stops after step 19 (sensor-sun), 35 (sensor-chain) and 13 (spectral) on MI355X.  The per-step
    sensor twin is left out: one ill-conditioned column of it alternates between accepted and rejected steps at the rounding floor of
    its cost beyond 60 steps, whatever the tolerance."""
    import torch

    y = _twin(variant)
    _plan = functools.partial(globals()["_plan"], xtol=1e-5)
    full = _plan(variant, "all", y).run(60)
    ref = full.result()
    assert full.nsteps == 60 and int(full.running()) == 0
    for mode in _modes(variant):
        plan = _plan(variant, mode, y).run(60, check_every=3)
        torch.cuda.synchronize()
        assert plan.nsteps < 60 and plan.nsteps % 3 == 0 and int(plan.running()) == 0, (mode, plan.nsteps)
        got = plan.result()
        for k in ("p", "cost", "status", "lam", "naccept", "nreject"):
            assert got[k].cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), (variant, mode, k)
        assert plan.reset().nsteps == 0
    r = full.running()
    assert r.ndim == 0 and r.is_cuda and r.dtype == torch.int64


def test_one_shot_functions_take_evaluate():
    from crt1d_amd import batched

    B = _base()
    p0, _, lo, hi = _points("sensor")
    kw = dict(OPTS, p0=_t(p0), lo=lo, hi=hi, d_leaf_r=B["dirn"][None], lai=True, leaf=True, niter=8)
    a = (("2s", B["cols"], B["bands"], (NZ - 1,), B["sensors"], _twin("sensor")), dict(keys=("I_df_u",), **kw))
    b = (("2s", B["cols"], B["bands"], (NZ - 1,), _twin("spectral")), dict(keys=("I_df_u",), **kw))
    for fn, (args, kws), modes in ((batched.retrieve, a, ("running", "accepted")), (batched.retrieve_spectral, b, ("running",))):
        ref = fn(*args, **kws)
        for mode in modes:
            got = fn(*args, evaluate=mode, **kws)
            for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
                assert got[k].cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), (fn.__name__, mode, k)
