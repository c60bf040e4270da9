"""GPU: the sensor-band Jacobian over a sun-angle series in one call (crt_hip_sensor_jac_series_f64, batched.SensorJacSeriesPlan),
g_dparam_series / leaf_tangent_series and Model.run_series_sensor_jacobian on top of it.

The comparator throughout is the per-step SensorJacPlan on the inputs of step t -- cols.psi = sun.psi[:, t] (g_at_psi likewise), the
incoming spectra of step t, tangent.step(t) -- compared with torch.equal: that plan is held to the composition and to the oracle by
tests/test_gpu_sensjac.py, so the series kernel needs no tolerance of its own.  The one bound in this file is that of the retrieval
(test_retrieval_needs_the_series), stated there."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_dleaf import KINDS, _host_kind
from test_gpu_sensjac import _slices

pytestmark = pytest.mark.gpu

CLOSED = ("2s", "bl", "g77", "bf")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
PARAMS = ("leaf_r", "leaf_t", "soil_r")
L16 = tuple(range(15)) + (19,)
# ((ncol, nb, nz), levels, nt): with 5 parameters a level takes 15 staging rows -- 9 levels: one 128-lane slice; 2 levels: 256 lanes, 257 =
# 129 + 128 and k_sens_jac_finish indexed by (column, t); 16 levels: 64 lanes, 130 = 44 + 43 + 43; one band
CASES = [((3, 13, 9), tuple(range(9)), 3), ((2, 257, 4), (0, 3), 2), ((2, 130, 20), L16, 2), ((4, 1, 5), tuple(range(5)), 1)]
PARSETS = ("dirs3+lai+leaf", "shared-dir", "leaf")


def test_the_cases_reach_every_slice_width():
    assert [_slices(s[1], len(lv), 5) for s, lv, _ in CASES] == [(1, 13), (2, 129), (3, 44), (1, 1)]
    assert 9 * 15 * 256 * 8 > 160 * 1024 - 4096 >= 9 * 15 * 128 * 8 and 16 * 15 * 128 * 8 > 160 * 1024 - 4096 >= 16 * 15 * 64 * 8


def _kind(shape):
    shapes = [c[0] for c in CASES]
    return list(KINDS)[shapes.index(shape) % 3] if shape in shapes else "ellipsoidal"  # every parametric leaf-angle kind is met


@functools.lru_cache(maxsize=None)
def _device(shape, uniform, nt, shared=False):
    """(cols, bands, sun) on the device; cols.psi is NOT a sun angle of the series (the entry must not read it)."""
    import torch

    from crt1d_amd import batched, synth

    d = _host_kind(shape, uniform, _kind(shape))
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    sun = batched.SunSeries.from_host(synth.make_sun_series(d, nt, seed=77, shared=shared))
    torch.cuda.synchronize()
    return cols, bands, sun


def _step(cols, bands, sun, t):
    """The per-step inputs of sun state t."""
    from crt1d_amd import batched

    rows = bands.leaf_r.shape[0]
    g = lambda v: v[:, t].expand(rows, -1).contiguous()  # noqa: E731
    c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla,
                        None if sun.g_at_psi is None else sun.g_at_psi[:, t].contiguous(), cols.g_table)
    return c, batched.Bands(g(sun.I_dr0), g(sun.I_df0), bands.leaf_r, bands.leaf_t, bands.soil_r)


@functools.lru_cache(maxsize=None)
def _sensors(shape, nsel):
    """5 sensor bands: all bands | one band | a support straddling the first slice boundary | one wholly in the second slice | one
    overlapping the others (one slice: the same shapes about the middle of the bands) -- the set of tests/test_gpu_sensjac.py."""
    from crt1d_amd import batched

    nb = shape[1]
    nslice, per = _slices(nb, nsel, 5)
    edge = per if nslice > 1 else nb // 2
    first, count = [], []
    for lo, hi in [(0, nb), (nb // 3, nb // 3 + 1), (edge - 2, edge + 3), (edge + 1, edge + 5), (nb // 4, nb // 4 + nb // 2)]:
        lo = min(max(lo, 0), nb - 1)
        hi = min(max(hi, lo + 1), nb)
        first.append(lo)
        count.append(hi - lo)
    w = np.random.default_rng(29).uniform(-1.0, 1.0, int(np.sum(count)))
    return batched.SensorSet.from_supports(np.array(first), np.array(count), w, nb=nb)


@functools.lru_cache(maxsize=None)
def _dirs(shape, uniform, ntan, shared):
    """Directions in the three spectra, relative to the spectra themselves: (ncol, ntan, nb), or (ntan, nb) shared."""
    import torch

    d = _host_kind(shape, uniform, _kind(shape))
    rng = np.random.default_rng(31)
    out = {}
    for k in PARAMS:
        base = d[k].mean(axis=0, keepdims=True) if shared else d[k]
        v = rng.uniform(-1.0, 1.0, (base.shape[0], ntan, shape[1])) * base[:, None, :]
        out["d_" + k] = torch.as_tensor(v[0] if shared else v).cuda()
    return out


def _parset(name, shape, uniform, cols, sun):
    """-> (kwargs of the series plan, t -> kwargs of the per-step plan)"""
    from crt1d_amd import batched

    tan = batched.leaf_tangent_series(cols, sun, "param")
    if name == "dirs3+lai+leaf":
        kw = dict(_dirs(shape, uniform, 3, False), lai=True)
    elif name == "shared-dir":
        kw = dict(d_leaf_t=_dirs(shape, uniform, 1, True)["d_leaf_t"], lai=False)
        return kw, lambda t: kw
    else:
        kw = dict(lai=False)
    return dict(kw, tangent=tan), lambda t: dict(kw, tangent=tan.step(t))


def _series(scheme, cols, bands, sun, lev, sensors, **kw):
    import torch

    from crt1d_amd import batched

    plan = batched.SensorJacSeriesPlan(scheme, cols, bands, sun, lev, sensors, **kw)
    got = plan()
    torch.cuda.synchronize()
    return plan, {k: v.clone() for k, v in got.items()}


def _per_step(scheme, cols, bands, sun, lev, sensors, t, **kw):
    import torch

    from crt1d_amd import batched

    got = batched.SensorJacPlan(scheme, *_step(cols, bands, sun, t), lev, sensors, **kw)()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in got.items()}


# ---- 1. (and 9: last_kernel) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", CLOSED)
def test_slices_are_bitwise_the_per_step_plan(scheme, uniform):
    import torch

    for shape, lev, nt in CASES:
        cols, bands, sun = _device(shape, uniform, nt)
        sensors = _sensors(shape, len(lev))
        for name in PARSETS:
            kw, kw_t = _parset(name, shape, uniform, cols, sun)
            plan, got = _series(scheme, cols, bands, sun, lev, sensors, **kw)
            npar = len(plan.params)
            assert plan.params == {"dirs3+lai+leaf": ("dir0", "dir1", "dir2", "lai", "leaf"), "shared-dir": ("dir0",), "leaf": ("leaf",)}[name]
            nslice, per = _slices(shape[1], len(lev), npar)
            assert plan.last_kernel() == (f"k_sens_jac_series<{scheme}> nt={nt} nsel={len(lev)} nsens={sensors.nsens} npar={npar} slice={per}" +
                                          (" + k_sens_jac_finish" if nslice > 1 else ""))
            for k in KEYS:
                assert got[k].shape == (shape[0], nt, len(lev), sensors.nsens, npar) and bool(got[k].isfinite().all()), (shape, name, k)
            for t in range(nt):
                ref = _per_step(scheme, cols, bands, sun, lev, sensors, t, **kw_t(t))
                for k in KEYS:
                    assert torch.equal(got[k][:, t], ref[k]), (scheme, shape, name, t, k)
            if scheme != "bl":
                assert bool((got["I_df_u"] != 0).any())


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
def test_shared_spectra_and_table_columns(scheme):
    import torch

    from crt1d_amd import batched
    from crt1d_amd.leaf_angle import PDF_ELLIPSOIDAL, PDF_TRIG

    shape, lev, nt = CASES[1]
    # sun given with one series of spectra for every column: (nt, nb)
    cols, bands, sun = _device(shape, False, nt, True)
    assert sun.I_dr0.shape[0] == 1 and sun.col_stride == 0
    flat = batched.SunSeries(sun.psi, sun.I_dr0[0], sun.I_df0[0])
    sensors = _sensors(shape, len(lev))
    kw, kw_t = _parset("dirs3+lai+leaf", shape, False, cols, sun)
    _, got = _series(scheme, cols, bands, flat, lev, sensors, **kw)
    for t in range(nt):
        ref = _per_step(scheme, cols, bands, sun, lev, sensors, t, **kw_t(t))
        for k in KEYS:
            assert torch.equal(got[k][:, t], ref[k]), (scheme, "shared spectra", t, k)
    # CRT_G_TABLE columns: G at the sun angles comes from sun.g_at_psi; a hand-made tangent series
    ncol = shape[0]
    kind = torch.tensor([PDF_TRIG, PDF_ELLIPSOIDAL], dtype=torch.int32, device="cuda")
    param = torch.tensor([[0.3, 0.1], [1.7, 0.0]], dtype=torch.float64, device="cuda")
    tcols = batched.Columns.from_leaf_pdf(cols.psi, cols.lai, kind, param)
    _, g_at, _ = batched.leaf_pdf_tables(kind, param, psi=sun.psi)
    tsun = batched.SunSeries(sun.psi, sun.I_dr0, sun.I_df0, g_at)
    rng = np.random.default_rng(8)
    r = lambda *s: torch.as_tensor(rng.uniform(-0.2, 0.2, s)).cuda()  # noqa: E731
    from crt1d_amd import _lib

    tan = batched.LeafTangentSeries(r(ncol, _lib.NQ), r(ncol, nt), r(ncol))
    d = _dirs(shape, False, 3, False)
    _, got = _series(scheme, tcols, bands, tsun, lev, sensors, tangent=tan, **d)
    for t in range(nt):
        ref = _per_step(scheme, tcols, bands, tsun, lev, sensors, t, tangent=tan.step(t), **d)
        for k in KEYS:
            assert torch.equal(got[k][:, t], ref[k]), (scheme, "G_TABLE", t, k)
        assert not torch.equal(got["F"][:, t, ..., 4], got["F"][:, (t + 1) % nt, ..., 4])


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_tangents_are_bitwise_the_per_step_functions():
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(5, 4, 6, seed=3)
    d["g_kind"] = np.array([3, 4, 5, 3, 0], dtype=np.int32)  # ellipsoidal, its approximation, Bonan's, ellipsoidal, spherical
    d["g_param"] = np.array([0.7, 1.6, 0.2, 1.0, 0.0])  # (x = 1: the series branch of the ellipsoidal normalisation)
    cols = batched.Columns.from_host(d)
    for nt in (1, 3, 60, 300):  # 55 sun states lie in the block of the nodes, the others in blocks of 192
        sun = batched.SunSeries.from_host(synth.make_sun_series(d, nt, seed=5))
        table, at_psi = batched.g_dparam_series(cols, sun)
        assert at_psi.shape == (5, nt)
        for t in sorted({0, nt // 2, 54 % nt, 55 % nt, 246 % nt, 247 % nt, nt - 1}):
            ct = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla)
            rt, rp = batched.g_dparam(ct)
            assert torch.equal(table, rt) and torch.equal(at_psi[:, t], rp), (nt, t)
            for wrt in batched.LEAF_WRT:
                a, b = batched.leaf_tangent_series(cols, sun, wrt).step(t), batched.leaf_tangent(ct, wrt)
                assert torch.equal(a.dg_table, b.dg_table) and torch.equal(a.dg_at_psi, b.dg_at_psi), (nt, t, wrt)
                assert (a.dmla is None and b.dmla is None) or torch.equal(a.dmla, b.dmla), (nt, t, wrt)
        ts = batched.leaf_tangent_series(cols, sun, "mla")
        assert ts.nt == nt and ts.slice(1, 3).dg_at_psi.shape == (2, nt) and torch.equal(ts.slice(1, 3).dmla, ts.dmla[1:3])


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
def test_bitwise_invariants(scheme):
    import torch

    from crt1d_amd import batched

    for shape, lev, nt in CASES[:3]:
        cols, bands, sun = _device(shape, False, nt)
        sensors = _sensors(shape, len(lev))
        kw, _ = _parset("dirs3+lai+leaf", shape, False, cols, sun)
        tan = kw["tangent"]
        _, full = _series(scheme, cols, bands, sun, lev, sensors, **kw)
        # a column alone is its row of the batch
        c = shape[0] - 1
        one_kw = {k: (v[c:c + 1].contiguous() if k.startswith("d_") else v) for k, v in kw.items()}
        _, one = _series(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), sun.slice(c, c + 1), lev, sensors, **dict(one_kw, tangent=tan.slice(c, c + 1)))
        for k in KEYS:
            assert torch.equal(one[k][0], full[k][c]), (scheme, shape, "column alone", k)
        # a series of the single step t is slice t
        t = nt - 1
        st = batched.SunSeries(sun.psi[:, t:t + 1].contiguous(), sun.I_dr0[:, t:t + 1].contiguous(), sun.I_df0[:, t:t + 1].contiguous())
        tt = batched.LeafTangentSeries(tan.dg_table, tan.dg_at_psi[:, t:t + 1].contiguous(), tan.dmla)
        _, single = _series(scheme, cols, bands, st, lev, sensors, **dict(kw, tangent=tt))
        for k in KEYS:
            assert torch.equal(single[k][:, 0], full[k][:, t]), (scheme, shape, "single step", k)
        # any subset of keys has the bits of the full call; the outputs not asked for are not touched
        for keys in (("F",), ("I_dr",), ("I_df_u", "I_df_d")):
            buf = torch.full((4,) + tuple(full["F"].shape), 3.25, dtype=torch.float64, device="cuda")  # the four arrays back to back
            out = {k: buf[i] for i, k in enumerate(KEYS)}
            plan = batched.SensorJacSeriesPlan(scheme, cols, bands, sun, lev, sensors, keys=keys, out={k: out[k] for k in keys}, **kw)
            sub = plan()
            torch.cuda.synchronize()
            assert set(sub) == set(keys)
            for k in KEYS:
                if k in keys:
                    assert sub[k] is out[k] and torch.equal(sub[k], full[k]), (scheme, shape, keys, k)
                else:
                    assert bool((out[k] == 3.25).all())


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
def test_flags_and_forward_sums(scheme):
    import torch

    from crt1d_amd import _lib, batched

    for ci in (0, 1):  # one slice; two slices with the finish kernel
        shape, lev, nt = CASES[ci]
        cols, bands, sun = _device(shape, True, nt)
        sensors = _sensors(shape, len(lev))
        kw, _ = _parset("dirs3+lai+leaf", shape, True, cols, sun)
        _, full = _series(scheme, cols, bands, sun, lev, sensors, **kw)
        plan = batched.SensorJacSeriesPlan(scheme, cols, bands, sun, lev, sensors, **kw)
        for v in plan.out.values():
            v.fill_(7.0)
        plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
        assert plan.last_kernel() == f"k_colpre<canopy> + k_colsun nt={nt}" + (" + k_dlai_side" if scheme == "bl" else "") + " + k_dleaf_side<canopy>"
        for v in plan.out.values():
            assert bool((v == 7.0).all())
        got = plan(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], full[k]), (scheme, shape, "precompute only + skip precompute", k)
        if ci == 0:  # the forward sums of the residual on this plan's workspace are those of a stand-alone plan (one slice)
            alone = {k: v.clone() for k, v in batched.solve_sensor_levels_series(scheme, cols, bands, sun, lev, sensors).items()}
            fwd = batched.SensorLevelsSeriesPlan(scheme, cols, bands, sun, lev, sensors, workspace=plan.workspace)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(fwd[k], alone[k]), (scheme, "forward sums on the Jacobian's workspace", k)


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
def test_graph_replay(scheme):
    """One replay of a captured plan equals the eager call (single stream, after a first call outside the capture); two band slices: the
    finish kernel is part of the graph."""
    import torch

    from crt1d_amd import batched

    shape, lev, nt = CASES[1]
    cols, bands, sun = _device(shape, True, nt)
    kw, _ = _parset("dirs3+lai+leaf", shape, True, cols, sun)
    plan = batched.SensorJacSeriesPlan(scheme, cols, bands, sun, lev, _sensors(shape, len(lev)), **kw)
    ref = {k: v.clone() for k, v in plan().items()}
    assert plan.last_kernel().endswith(" + k_sens_jac_finish")
    torch.cuda.synchronize()  # (the side stream below writes the same buffers)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan()
    for v in plan.out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(plan.out[k], ref[k]), k


# ---- 7. ---------------------------------------------------------------------------------------------------------------------------------
def test_long_series_across_two_grid_dimensions():
    """nt = 66 000 > 65 535: t runs over blockIdx.y and blockIdx.z, with the two band slices of 257 bands in blockIdx.z too."""
    import torch

    from crt1d_amd import batched, synth

    shape, lev, nt = (1, 257, 4), (0,), 66000
    d = _host_kind(shape, True, "ellipsoidal")
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    sun = batched.SunSeries.from_host(synth.make_sun_series(d, nt, seed=9))
    sensors = _sensors((2, 257, 4), 1)
    assert _slices(257, 1, 5)[0] == 2
    dirs = {k: v[:1].contiguous() for k, v in _dirs((2, 257, 4), True, 3, False).items()}
    tan = batched.leaf_tangent_series(cols, sun, "param")
    plan, got = _series("2s", cols, bands, sun, lev, sensors, tangent=tan, **dirs)
    assert f" nt={nt} " in plan.last_kernel() and plan.last_kernel().endswith(" + k_sens_jac_finish")
    for t in (0, 65534, 65535, 65536, nt - 1):
        ref = _per_step("2s", cols, bands, sun, lev, sensors, t, tangent=tan.step(t), **dirs)
        for k in KEYS:
            assert torch.equal(got[k][:, t], ref[k]), (t, k)


# ---- 8. ---------------------------------------------------------------------------------------------------------------------------------
DEEP = (2, 130, 24)  # (21 levels must exist before they can be refused for the LDS)


def _c_call(scheme, lev):
    """The C entry with a whole set of valid device arguments, sentinel outputs and a zeroed workspace -> (status, outputs, workspace)."""
    import torch

    from crt1d_amd import _lib, batched

    nt = 2
    cols, bands, sun = _device(DEEP, True, nt)
    sensors = _sensors(DEEP, 16)
    tan = batched.leaf_tangent_series(cols, sun, "param")
    dirs = _dirs(DEEP, True, 3, True)
    out = {k: torch.full((DEEP[0], nt, len(lev), sensors.nsens, 5), 3.25, dtype=torch.float64, device="cuda") for k in KEYS}
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device="cuda")
    c, b, sn, o = cols.c_struct(), bands.c_struct(DEEP[0]), sun.c_struct(), _lib.CrtOptions(0.501, 0, 0)
    cs, cd = sensors.c_struct(), _lib.CrtOpticsDirs(3, 0, *[dirs["d_" + k].data_ptr() for k in PARAMS])
    co, tn = _lib.CrtSensJacOut(*[out[k].data_ptr() for k in KEYS]), tan.c_struct()
    arr = (ctypes.c_int32 * len(lev))(*lev)
    st = _lib.load().crt_hip_sensor_jac_series_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(sn), ctypes.byref(o), arr,
                                                   len(lev), ctypes.byref(cs), ctypes.byref(cd), 1, ctypes.byref(tn), ctypes.byref(co), ws.data_ptr(),
                                                   ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, out, ws


@pytest.mark.parametrize("scheme", ["n79", "zq", "4s", "zq_pa"])
def test_refused_on_the_device(scheme):
    """CRT_ERR_UNSUPPORTED through the C entry with a whole set of valid device arguments: outputs and workspace untouched."""
    from crt1d_amd import _lib

    st, out, ws = _c_call(scheme, L16)
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == 3.25).all())
    assert bool((ws == 0).all())


@pytest.mark.parametrize("scheme", CLOSED)
def test_refused_beyond_the_lds(scheme):
    """5 parameters: 15 staging rows per level; 20 levels (300 rows) are served, 21 (315 > 312) refused before anything is written."""
    from crt1d_amd import _lib

    st, out, ws = _c_call(scheme, tuple(range(21)))
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == 3.25).all())
    assert bool((ws == 0).all())
    st, out, ws = _c_call(scheme, tuple(range(20)))
    assert st == _lib.CRT_OK
    for k, v in out.items():
        assert bool(v.isfinite().all()) and bool((v[..., 3:] != 3.25).all()), k


# ---- 9. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["n79", "zq"])
def test_composed_path(scheme):
    """n79 / zq: the per-step plan's composed path looped over t into the series layout."""
    import torch

    shape, lev, nt = CASES[0]
    cols, bands, sun = _device(shape, True, nt)
    sensors = _sensors(shape, len(lev))
    kw, kw_t = _parset("dirs3+lai+leaf", shape, True, cols, sun)
    plan, got = _series(scheme, cols, bands, sun, lev, sensors, **kw)
    assert plan.last_kernel().count("k_jac_tri<") == nt and plan.last_kernel().count("k_dlai_tri<") == 2 * nt, plan.last_kernel()
    for t in range(nt):
        ref = _per_step(scheme, cols, bands, sun, lev, sensors, t, **kw_t(t))
        for k in KEYS:
            assert got[k].shape == (shape[0], nt, len(lev), sensors.nsens, 5) and torch.equal(got[k][:, t], ref[k]), (scheme, t, k)


# ---- 10. --------------------------------------------------------------------------------------------------------------------------------
NITER = 14
ZENITHS = np.deg2rad([22.0, 45.0, 64.0])


def _retrieval(mode):
    """Damped Gauss-Newton on a noise-free problem that one sun state cannot solve: 2s, 4 columns, 30 bands (15 visible, 15 near-infrared),
    12 levels; observed are the upwelling sums I_df_u of TWO boxcar sensor bands at the top of the canopy at THREE sun zeniths (6
    observations; one sun state would give 2); unknowns: one leaf-reflectance coefficient, ln(LAI scale), the ellipsoidal x.  A step that
    raises a column's misfit is rejected and that column's damping raised, as _retrieval of tests/test_gpu_sensjac.py.  mode: "series" (one
    SensorJacSeriesPlan + one SensorLevelsSeriesPlan call per evaluation), "steps" (nt SensorJacPlan + SensorLevelsPlan calls),
    "composed" (sensor_jvp + sensor_dlai + sensor_dleaf per step; forward as "steps").
    -> (iterates (niter + 1, ncol, 3), misfit history (niter + 1, ncol), parameter error (3,))"""
    import torch

    from crt1d_amd import batched, synth

    ncol, nb, nz, nt = 4, 30, 12, len(ZENITHS)
    d = synth.make_columns(ncol, nb, nz, seed=5)
    t64 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).cuda()  # noqa: E731
    rng = np.random.default_rng(41)
    vis = np.arange(nb) < nb // 2
    leaf_r = np.where(vis, 0.08, 0.45) * rng.uniform(0.9, 1.1, (ncol, nb))
    leaf_t = np.where(vis, 0.06, 0.42) * rng.uniform(0.9, 1.1, (ncol, nb))
    soil_r = np.where(vis, 0.10, 0.25) * rng.uniform(0.9, 1.1, (ncol, nb))
    lai = np.linspace(1.0, 0.0, nz)[None, :] * rng.uniform(1.5, 3.0, ncol)[:, None]
    dirn = t64(0.3 * leaf_r.mean(axis=0))  # (nb,): one shared direction in leaf_r
    truth = torch.stack((t64(rng.uniform(-0.2, 0.2, ncol)), t64(rng.uniform(-0.15, 0.15, ncol)), t64(rng.uniform(0.8, 1.6, ncol))), dim=1)
    kind = torch.full((ncol,), KINDS["ellipsoidal"], dtype=torch.int32, device="cuda")
    psi = ZENITHS[None, :] + np.deg2rad(rng.uniform(-2.0, 2.0, (ncol, 1)))
    I_dr0 = d["I_dr0"][:, None, :] * np.cos(psi)[:, :, None]
    I_df0 = np.repeat(d["I_df0"][:, None, :], nt, axis=1)
    sun = batched.SunSeries(t64(psi), t64(I_dr0), t64(I_df0))
    w = np.zeros((2, nb))
    w[0, 2:13], w[1, 17:28] = 1.0, 1.0
    sensors = batched.SensorSet(w)
    lev, keys = (nz - 1,), ("I_df_u",)

    def inputs(p):
        cols = batched.Columns(sun.psi[:, 0].contiguous(), t64(lai) * torch.exp(p[:, 1])[:, None], kind, p[:, 2].contiguous(), t64(d["mla"]))
        bands = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), t64(leaf_r) + p[:, 0, None] * dirn, t64(leaf_t), t64(soil_r))
        return cols, bands

    def forward(p):  # (ncol, nt * 2)
        cols, bands = inputs(p)
        if mode == "series":
            o = batched.solve_sensor_levels_series("2s", cols, bands, sun, lev, sensors, keys=keys)["I_df_u"]
        else:
            o = torch.stack([batched.solve_sensor_levels("2s", *_step(cols, bands, sun, t), lev, sensors, keys=keys)["I_df_u"] for t in range(nt)], dim=1)
        return o.reshape(ncol, nt * 2)

    def jacobian(p):  # (ncol, nt * 2, 3)
        cols, bands = inputs(p)
        if mode == "series":
            J = batched.sensor_jacobian_series("2s", cols, bands, sun, lev, sensors, d_leaf_r=dirn[None],
                                               tangent=batched.leaf_tangent_series(cols, sun, "param"), keys=keys)["I_df_u"]
            return J.reshape(ncol, nt * 2, 3)
        rows = []
        for t in range(nt):
            ct, bt = _step(cols, bands, sun, t)
            tan = batched.leaf_tangent(ct, "param")
            if mode == "steps":
                rows.append(batched.sensor_jacobian("2s", ct, bt, lev, sensors, d_leaf_r=dirn[None], tangent=tan, keys=keys)["I_df_u"])
            else:
                a = batched.sensor_jvp("2s", ct, bt, lev, sensors, dirn[None], None, None, keys=keys)["I_df_u"]
                b = batched.sensor_dlai("2s", ct, bt, lev, sensors, keys=keys)["I_df_u"]
                c = batched.sensor_dleaf("2s", ct, bt, lev, tan, sensors, keys=keys)["I_df_u"]
                rows.append(torch.cat([a, b[..., None], c[..., None]], dim=-1))
        return torch.stack(rows, dim=1).reshape(ncol, nt * 2, 3)

    y = forward(truth).clone()
    zero = torch.zeros(ncol, dtype=torch.float64, device="cuda")
    p = torch.stack((zero, zero, torch.full_like(zero, 1.2)), dim=1)
    lam = torch.full((ncol,), 1e-2, dtype=torch.float64, device="cuda")
    r = forward(p) - y
    hist, its = [(r * r).sum(1)], [p.clone()]
    for _ in range(NITER):
        trial = p + batched.gauss_newton_step(jacobian(p), r, damping=lam)
        trial[:, 2] = trial[:, 2].clamp(0.2, 5.0)
        rt = forward(trial) - y
        better = (rt * rt).sum(1) < hist[-1]
        p = torch.where(better[:, None], trial, p)
        r = torch.where(better[:, None], rt, r)
        lam = torch.where(better, lam / 10, lam * 10)
        hist.append((r * r).sum(1))
        its.append(p.clone())
    torch.cuda.synchronize()
    return torch.stack(its).cpu().numpy(), torch.stack(hist).cpu().numpy(), (p - truth).abs().max(0).values.cpu().numpy()


def test_retrieval_needs_the_series():
    """(a) the iterates of the loop on the series plans are bitwise those of the loop on nt per-step plans; (b) the misfit never increases;
    (c) the final parameter error is at most 100 x that of the identical loop on the composed Jacobian, which itself ends below 1e-8 in
    every parameter (a bound relative to a loop that did not converge would show nothing).  The factor covers the amplification of
    rounding differences along 14 steps: both loops end at rounding level, where the last digits fluctuate (tests/test_gpu_sensjac.py
    measured 1.4e-13 against 9.5e-14 for one sun state).  Measured on MI355X, parameter errors (a, ln LAI, x) after 14 steps: series
    1.1e-15, 4.6e-15, 8.0e-15; composed 6.7e-16, 3.7e-16, 3.6e-15; largest column misfit 1.6e+01 -> 5.1e-29 (composed 6.5e-29)."""
    its_s, hist_s, err_s = _retrieval("series")
    its_p, hist_p, err_p = _retrieval("steps")
    its_c, hist_c, err_c = _retrieval("composed")
    print(f"series retrieval: parameter error (a, ln LAI, x) series {err_s}, composed {err_c}; misfit {hist_s[0].max():.3e} -> {hist_s[-1].max():.3e} "
          f"(composed {hist_c[-1].max():.3e})")
    assert np.array_equal(its_s, its_p) and np.array_equal(hist_s, hist_p)
    assert np.all(hist_s[1:] <= hist_s[:-1]) and np.all(hist_c[1:] <= hist_c[:-1])
    assert np.all(err_c < 1e-8), err_c
    assert err_s.max() <= 100 * err_c.max(), (err_s, err_c)


# ---- 11. --------------------------------------------------------------------------------------------------------------------------------
def test_model_run_series_sensor_jacobian():
    """Model.run_series_sensor_jacobian is the batched call on the model's own column: bitwise."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=60)
    nb = m.nwl
    w = np.zeros((3, nb))
    w[0, : nb // 2], w[1, nb // 3:], w[2, nb // 2] = 1.0, 0.5, 2.0
    d = np.random.default_rng(3).uniform(-0.1, 0.1, (2, nb))
    psi = np.deg2rad([10.0, 40.0, 70.0])
    got = m.run_series_sensor_jacobian(psi, w, levels=(0, -1), directions={"leaf_r": d, "soil_r": 2 * d}, lai=True, wrt_leaf="param")
    assert got["params"] == ("dir0", "dir1", "lai", "leaf")
    scheme, cols, b, sun = m._series_inputs(psi, None, None, "sensor Jacobian")
    ref = batched.sensor_jacobian_series("2s", cols, b, sun, (0, -1), batched.SensorSet(w), d_leaf_r=d, d_soil_r=2 * d,
                                         tangent=batched.leaf_tangent_series(cols, sun, "param"))
    torch.cuda.synchronize()
    for k in KEYS:
        assert got[k].shape == (3, 2, 3, 4) and np.array_equal(got[k], ref[k][0].cpu().numpy()), k
    assert m.run_series_sensor_jacobian(psi, w, lai=True)["params"] == ("lai",)
    with pytest.raises(ValueError, match="has no sensor Jacobian"):
        Model("4s", nlayers=60).run_series_sensor_jacobian(psi, w)
