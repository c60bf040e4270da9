"""GPU: the masked entries and the accept decision (include_mask/crt1d_hip_masked.h), through ``skip=`` of the six inner plans and
through ``crt_hip_lm_decide_f64`` itself.

1. The six entries x 2s, bl, g77, bf x uniform and ragged LAI x one band slice and several (with the finish kernel).  Outputs and
   workspace are prefilled with a NaN-payload sentinel; for every mask pattern the evaluated columns hold the bits of the plain entry on
   the same inputs, the skipped columns hold the sentinel, and the workspace differs from the plain call's only by words that still hold
   the sentinel -- the slice partial sums of the skipped columns, ``(skipped columns) / ncol`` of what an all-skipped call leaves out.
   Patterns: none, all, alternating, first only, last only, all but one (5 of 6 neighbours skipped), and per-unit flags: unit = 3 on the
   6-column shapes, unit = 4 and 2 on the 8-column shape (a unit has to divide ncol: 3 does not divide 8).
   A NULL skip behind the masked entry: the plain bits and the plain ``crt_hip_last_kernel``.
2. One masked plan captured into a ``torch.cuda.CUDAGraph``: the replay reads the flags the array holds then.
3. ``crt_hip_lm_decide_f64`` on the random blocks of tests/test_gpu_retrieve.py: cost_t bitwise the NumPy restatement of the summation
   contract, skip_jac the definition (NaN cost, cost = +inf, cost == cost_t, columns that are not running), and a following
   ``crt_hip_lm_step_f64`` accepts exactly the columns with skip_jac == 0.

Shapes (ncol, nb, nz).  The sensor Jacobian and the spectral normal equations narrow their slices to the LDS: (6, 130, 20) with the 16
levels of tests/test_gpu_deriv_bits.py gives three and two slices.  The sensor-level kernels take up to 1024 bands per slice, so their
several-slice shape is (6, 1030, 5)."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_retrieve import LM, _dev, _normal_ref, _random_blocks, _split, _t

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "bl", "g77", "bf")
ENTRIES = ("sensor_levels", "sensor_levels_series", "sensor_jac", "sensor_jac_series", "spectral_normal", "spectral_normal_series")
L16 = tuple(range(15)) + (19,)
SMALL, SLICED, WIDE = (8, 37, 9), (6, 130, 20), (6, 1030, 5)
NT = 3
SENTINEL = 0x7FF80000DEADBEEF  # a quiet NaN with a payload
G_ELLIPSOIDAL = 3


def _shape(entry, sliced):
    if not sliced:
        return SMALL, tuple(range(SMALL[2]))
    return (WIDE, tuple(range(WIDE[2]))) if entry.startswith("sensor_levels") else (SLICED, L16)


@functools.lru_cache(maxsize=None)
def _inputs(shape, uniform):
    import torch

    from crt1d_amd import batched, synth

    ncol, nb, nz = shape
    d = dict(synth.make_columns(ncol, nb, nz, seed=11, uniform_dlai=uniform))
    rng = np.random.default_rng(3)
    d["g_kind"] = np.full(ncol, G_ELLIPSOIDAL, dtype=np.int32)
    d["g_param"] = rng.uniform(0.7, 2.0, ncol)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    sun = batched.SunSeries.from_host(synth.make_sun_series(d, NT, seed=77))
    dirs = {"d_" + k: _t(rng.uniform(-0.01, 0.01, (ncol, 3, nb)) * d[k][:, None, :]) for k in ("leaf_r", "leaf_t", "soil_r")}
    first = [0, nb // 3, max(nb // 2 - 2, 0)]
    count = [nb, 1, min(5, nb - first[2])]
    sensors = batched.SensorSet.from_supports(np.array(first), np.array(count), rng.uniform(-1.0, 1.0, int(np.sum(count))), nb=nb)
    torch.cuda.synchronize()
    return cols, bands, sun, dirs, sensors, rng.uniform(0.0, 5.0, (ncol, NT, 64, nb))


def _maker(entry, scheme, sliced, uniform, npar=5):
    """-> (make(skip, unit) -> plan, ncol).  npar = 5: three directions, ln LAI and the leaf angle; npar = 1: ln LAI alone."""
    from crt1d_amd import batched

    shape, lev = _shape(entry, sliced)
    cols, bands, sun, dirs, sensors, yy = _inputs(shape, uniform)
    if scheme == "bl":
        bands = batched.Bands(bands.I_dr0, bands.I_df0, bands.leaf_r, bands.leaf_t, None)
        dirs = {k: v for k, v in dirs.items() if k != "d_soil_r"}
    series = entry.endswith("series")
    axis = {}
    if not entry.startswith("sensor_levels"):
        axis = dict(lai=True)
        if npar == 5:
            tan = batched.leaf_tangent_series(cols, sun, "param") if series else batched.leaf_tangent(cols, "param")
            axis = dict(dirs, lai=True, tangent=tan)
    head = (scheme, cols, bands) + ((sun,) if series else ()) + (lev,)
    if entry.startswith("sensor_levels"):
        cls = batched.SensorLevelsSeriesPlan if series else batched.SensorLevelsPlan
        make = lambda skip, unit: cls(*head, sensors, skip=skip, skip_unit=unit)  # noqa: E731
    elif entry.startswith("sensor_jac"):
        cls = batched.SensorJacSeriesPlan if series else batched.SensorJacPlan
        make = lambda skip, unit: cls(*head, sensors, **axis, skip=skip, skip_unit=unit)  # noqa: E731
    else:
        y = _t(yy[:, :, :len(lev)] if series else yy[:, 0, :len(lev)])
        cls = batched.SpectralNormalSeriesPlan if series else batched.SpectralNormalPlan
        extra = dict(per_step=True) if series else {}
        make = lambda skip, unit: cls(*head, {"I_df_d": y, "F": y}, keys=("I_df_d", "F"), fwd=True, **extra, **axis, skip=skip, skip_unit=unit)  # noqa: E731
    return make, shape[0]


def _flat(plan):
    """name -> output tensor, the model spectra of the spectral plans included; the column is the first axis of every one."""
    out = {}
    for k, v in plan.out.items():
        if isinstance(v, dict):
            out.update({f"{k}.{q}": t for q, t in v.items()})
        else:
            out[k] = v
    return out


def _words(t):
    import torch

    n = t.numel() * t.element_size() // 8
    return t.reshape(-1).view(torch.uint8)[:n * 8].view(torch.int64)


def _prefill(plan):
    for t in list(_flat(plan).values()) + [plan.workspace]:
        _words(t).fill_(SENTINEL)


def _snap(plan):
    import torch

    torch.cuda.synchronize()
    return {k: _words(v).reshape(v.shape[0], -1).cpu().numpy().copy() for k, v in _flat(plan).items()}, _words(plan.workspace).cpu().numpy().copy()


def _patterns(ncol):
    one = lambda *idx: np.isin(np.arange(ncol), idx)  # noqa: E731
    pats = [("none", 1, np.zeros(ncol, bool)), ("all", 1, np.ones(ncol, bool)), ("alternating", 1, np.arange(ncol) % 2 == 0),
            ("first only", 1, one(0)), ("last only", 1, one(ncol - 1)), ("all but one", 1, ~one(ncol // 2))]
    for unit in ((3,) if ncol % 3 == 0 else (4, 2)):
        n = ncol // unit
        pats += [(f"unit {unit} first", unit, np.arange(n) == 0), (f"unit {unit} last", unit, np.arange(n) == n - 1)]
    return pats


def _check(entry, scheme, sliced, uniform, npar=5):
    import torch

    from crt1d_amd import _lib

    make, ncol = _maker(entry, scheme, sliced, uniform, npar)
    plain = make(None, 1)
    _prefill(plain)
    plain()
    ref, ref_ws = _snap(plain)
    report = plain.last_kernel()
    assert ("finish" in report) == (sliced or entry == "spectral_normal_series"), report  # the slice regime the case is meant to reach
    assert all(not np.any(v == np.int64(SENTINEL)) for v in ref.values()), "the plain call writes every element"
    plans, flags, left_out_by_all = {}, {}, None
    for name, unit, skipped in _patterns(ncol):
        if unit not in plans:
            flags[unit] = torch.zeros(ncol // unit, dtype=torch.int32, device="cuda")
            plans[unit] = make(flags[unit], unit)
        plan = plans[unit]
        flags[unit].copy_(torch.as_tensor(skipped.astype(np.int32) * 7))  # (any value but 0 skips)
        _prefill(plan)
        plan()
        got, ws = _snap(plan)
        assert "_masked" in plan.last_kernel() and plan.last_kernel().replace("_masked", "") == report
        col_skipped = np.repeat(skipped, unit)
        for k in ref:
            for c in range(ncol):
                if col_skipped[c]:
                    assert np.all(got[k][c] == np.int64(SENTINEL)), (name, k, c, "a skipped column was written")
                else:
                    assert np.array_equal(got[k][c], ref[k][c]), (name, k, c, "an evaluated column differs from the plain entry")
        differs = ws != ref_ws
        assert np.all(ws[differs] == np.int64(SENTINEL)), (name, "a workspace word differs from the plain call's and is not the sentinel")
        if name == "all":
            left_out_by_all = int(differs.sum())
            assert (left_out_by_all > 0) == (sliced or entry == "spectral_normal_series") and left_out_by_all % ncol == 0
        elif name == "none":
            assert not differs.any()
        else:
            assert int(differs.sum()) == left_out_by_all // ncol * int(col_skipped.sum()), (name, "the slice sums of the skipped columns, no more")
    # a NULL skip behind the masked entry: the plain launches
    plan = plans[1]
    flags[1].fill_(1)
    plan._mask = _lib.CrtColMask(None, 0)
    _prefill(plan)
    plan()
    got, ws = _snap(plan)
    assert plan.last_kernel() == report and np.array_equal(ws, ref_ws) and all(np.array_equal(got[k], ref[k]) for k in ref)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("sliced", [False, True], ids=["one-slice", "slices"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_masked_entry(entry, scheme, sliced, uniform):
    _check(entry, scheme, sliced, uniform)


@pytest.mark.parametrize("entry", ENTRIES[2:])
def test_masked_entry_with_one_parameter(entry):
    """npar = 1 (ln LAI alone): no direction pass and no leaf-angle side record."""
    _check(entry, "2s", False, False, npar=1)
    _check(entry, "bl", False, True, npar=1)


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["sensor_jac", "spectral_normal_series"])
def test_graph_replay_reads_the_flags_of_the_replay(entry):
    import torch

    make, ncol = _maker(entry, "2s", True, False)
    plain = make(None, 1)
    plain()
    ref, _ = _snap(plain)
    skip = torch.zeros(ncol, dtype=torch.int32, device="cuda")
    plan = make(skip, 1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan()
    for skipped in (np.arange(ncol) % 2 == 1, np.arange(ncol) < 2):
        skip.copy_(torch.as_tensor(skipped.astype(np.int32)))
        _prefill(plan)
        g.replay()
        got, _ = _snap(plan)
        for k in ref:
            for c in range(ncol):
                want = np.full_like(ref[k][c], np.int64(SENTINEL)) if skipped[c] else ref[k][c]
                assert np.array_equal(got[k][c], want), (k, c)


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("npar", [1, 5, 10])
@pytest.mark.parametrize("nrow", [1, 13, 64, 65, 200])
def test_decide(nrow, npar, nblk):
    """12 columns.  Columns 0-1: cost = +inf (the first step).  2-3: cost above cost_t (accepted).  4-5: cost below cost_t (rejected).
    6: cost == cost_t (strict: rejected).  7: a NaN in an observed row (cost_t NaN: skipped; with cost = +inf the step fails the start).
    8: the same with a finite cost (rejected).  9-11: not running (status 1, 2, 3): skipped, cost_t keeps its bits."""
    import torch

    from crt1d_amd import _lib

    ncol = 12
    rng = np.random.default_rng(5000 * nrow + 10 * npar + nblk)
    blocks = _random_blocks(rng, ncol, _split(nrow, nblk), npar)
    for c in (7, 8):
        blocks[-1]["f"][c, -1] = np.nan  # (the last block is never the one with holes unless it is block 0; make the row observed)
        if blocks[-1]["s"] is not None:
            blocks[-1]["s"][c, -1] = 1.5
    p0, prior = rng.normal(size=(ncol, npar)), rng.normal(size=(ncol, npar))
    isp = rng.uniform(0.5, 2.0, (ncol, npar))
    isp[:, npar // 2] = 0.0
    prior[:, npar // 2] = np.nan
    want = np.array([_normal_ref(blocks, c, npar, p0, prior, isp)[2] for c in range(ncol)])
    assert np.isnan(want[7]) and np.isnan(want[8]) and np.all(np.isfinite(np.delete(want, (7, 8))))
    cost = np.full(ncol, np.inf)
    cost[2:4], cost[4:6], cost[6], cost[8] = want[2:4] * 1.5, want[4:6] * 0.5, want[6], 1.0
    cost[9:] = want[9:] * 2.0
    lm = LM(_dev(blocks), _t(p0), prior=_t(prior), isp=_t(isp))
    lm.cost.copy_(_t(cost))
    lm.status[9:] = torch.tensor([1, 2, 3], dtype=torch.int32, device="cuda")
    skip = torch.full((ncol,), -5, dtype=torch.int32, device="cuda")
    cost_t = torch.empty(ncol, dtype=torch.float64, device="cuda")
    _words(cost_t).fill_(SENTINEL)
    before = lm.snap()
    st = lm.lib.crt_hip_lm_decide_f64(ctypes.byref(lm._prob), lm._obs, len(lm.blocks), ctypes.byref(lm._state), skip.data_ptr(), cost_t.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert st == _lib.CRT_OK and lm.lib.crt_hip_last_kernel().decode() == f"k_lm_decide npar={npar} nblk={nblk}"
    after = lm.snap()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)  # no state is written
    got_t, got_s = cost_t.cpu().numpy(), skip.cpu().numpy()
    assert got_t[:9].tobytes() == want[:9].tobytes()
    assert np.all(_words(cost_t).cpu().numpy()[9:] == np.int64(SENTINEL))
    running = np.arange(ncol) < 9
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got_s, (~(running & (want < cost))).astype(np.int32))
    assert got_s.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    lm.step()
    final = lm.snap()
    assert np.array_equal(final["naccept"] == 1, got_s == 0) and np.all(final["naccept"] <= 1)
    assert final["cost"][:4].tobytes() == want[:4].tobytes() and final["status"][7] == _lib.LM_FAILED_START
