"""GPU: the sun-angle series (crt_hip_integrated_series_f64) against the per-step entry crt_hip_integrated2_f64, bit for bit.

The yardstick is ``IntegratedPlan`` (pinned by the rest of the suite against the oracle and the goldens): for every step ``t``, slice
``[:, t]`` of every series output must be ``torch.equal`` to what ``IntegratedPlan`` writes for the same columns with the sun and the
incoming spectra of step ``t``.  No tolerance anywhere except ``Model.run_series`` (1e-12, the bar of tests/test_gpu_band.py)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
SHAPES = [(19, 300, 60), (7, 107, 61), (5, 12, 60), (3, 13, 9), (2, 1, 5), (2, 1024, 20), (3, 300, 100)]  # (ncol, nb, nz)
DEV = "cuda:0"


def _mods():
    from crt1d_amd import _lib, batched, synth

    return _lib, batched, synth


def _case(ncol, nb, nz, nt, *, uniform, seed=11, shared=False, per_column_optics=True, kinds=True):
    _lib, batched, synth = _mods()
    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform, per_column_optics=per_column_optics)
    if kinds:  # all six closed-form leaf-angle kinds over the columns
        d["g_kind"] = (np.arange(ncol) % 6).astype(np.int32)
        d["g_param"] = np.where(d["g_kind"] == 5, np.linspace(-0.3, 0.5, ncol), d["g_param"])
    s = synth.make_sun_series(d, nt, seed=seed + 1, shared=shared)
    cols = batched.Columns.from_host(d, DEV)
    bands = batched.Bands.from_host(d, DEV)
    sun = batched.SunSeries.from_host(s, DEV)
    return d, s, cols, bands, sun


def _band_w(nb, ng, seed=5):
    return torch.as_tensor(np.random.default_rng(seed).uniform(0.0, 1.0, (ng, nb)), device=DEV)


def _step(batched, scheme, cols, bands, sun, t, band_w, profiles, **kw):
    """The per-step call for sun state t: crt_hip_integrated2_f64 through IntegratedPlan."""
    ncol = cols.ncol
    c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla,
                        None if sun.g_at_psi is None else sun.g_at_psi[:, t].contiguous(), cols.g_table)
    idr, idf = sun.I_dr0[:, t], sun.I_df0[:, t]
    lr, lt, sr = bands.leaf_r, bands.leaf_t, bands.soil_r
    rows = max(idr.shape[0], lr.shape[0])
    ex = lambda v: v.expand(rows, -1).contiguous()  # noqa: E731  (Bands wants one shape for all five)
    b = batched.Bands(ex(idr), ex(idf), ex(lr), ex(lt), ex(sr))
    assert rows in (1, ncol)
    return batched.IntegratedPlan(scheme, c, b, band_w, profiles=profiles, **kw)()


def _assert_slices(batched, scheme, cols, bands, sun, band_w, profiles, steps=None, **kw):
    plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, band_w, profiles=profiles, **kw)
    got = plan()
    torch.cuda.synchronize()
    assert "series" in plan.last_kernel() and "k_colsun" in plan.last_kernel(), plan.last_kernel()
    for t in (range(sun.nt) if steps is None else steps):
        ref = _step(batched, scheme, cols, bands, sun, t, band_w, profiles, **kw)
        torch.cuda.synchronize()
        for k, v in ref.items():
            assert got[k].shape[:2] == (cols.ncol, sun.nt)
            assert torch.equal(got[k][:, t], v), (scheme, k, t, float((got[k][:, t] - v).abs().max()))
    return plan, got


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_series_slices_bitwise(scheme, shape, uniform):
    """8 schemes x uniform / ragged x 7 shapes x nt in {1, 3, 24} x profiles False / True, ngroup 1 and 3."""
    _lib, batched, synth = _mods()
    ncol, nb, nz = shape
    for nt in (1, 3, 24):
        d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=uniform, seed=100 + nt)
        for profiles, ng in ((False, 3), (True, 1), (True, 3), (False, 1)):
            _assert_slices(batched, scheme, cols, bands, sun, _band_w(nb, ng), profiles)  # every t


@pytest.mark.parametrize("scheme", SCHEMES)
def test_shared_series_and_broadcast_optics(scheme):
    """col_stride = 0 of the sun's spectra against the same series repeated per column; broadcast leaf optics (bands.col_stride = 0)."""
    _lib, batched, synth = _mods()
    ncol, nb, nz, nt = 6, 38, 33, 4
    w = _band_w(nb, 2)
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=False, shared=True)
    assert sun.col_stride == 0
    _, a = _assert_slices(batched, scheme, cols, bands, sun, w, True)
    rep = batched.SunSeries(sun.psi, sun.I_dr0.expand(ncol, -1, -1).contiguous(), sun.I_df0.expand(ncol, -1, -1).contiguous())
    assert rep.col_stride == nt * nb
    b = batched.solve_integrated_series(scheme, cols, bands, rep, w, profiles=True)
    for k in a:
        assert torch.equal(a[k], b[k]), (scheme, k)
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=True, per_column_optics=False)
    bands = batched.Bands(None, None, bands.leaf_r, bands.leaf_t, bands.soil_r)  # built without the incoming spectra
    assert bands.col_stride(ncol) == 0
    _assert_slices(batched, scheme, cols, bands, sun, w, False)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_g_table_columns(scheme):
    """CRT_G_TABLE columns: the canopy record comes from g_table, the sun record from the per-step g_at_psi."""
    _lib, batched, synth = _mods()
    from crt1d_amd import leaf_angle

    ncol, nb, nz, nt = 5, 20, 17, 3
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=False, kinds=False)
    nodes = _lib.quad_nodes(0.501)
    x = d["g_param"]
    G = lambda psi, xx: leaf_angle.G_ellipsoidal_approx(psi, xx)  # noqa: E731
    table = np.stack([G(nodes, x[c]) for c in range(ncol)])
    gat = np.stack([G(s["psi"][c], x[c]) for c in range(ncol)])
    kind = d["g_kind"].copy()
    kind[::2] = 6
    cols = batched.Columns(cols.psi, cols.lai, torch.as_tensor(kind, device=DEV), cols.g_param, cols.mla,
                           torch.zeros(ncol, dtype=torch.float64, device=DEV), torch.as_tensor(table, device=DEV))
    sun = batched.SunSeries(sun.psi, sun.I_dr0, sun.I_df0, torch.as_tensor(gat, device=DEV))
    _assert_slices(batched, scheme, cols, bands, sun, _band_w(nb, 3), True)
    with pytest.raises(ValueError):
        batched.IntegratedSeriesPlan(scheme, cols, bands, batched.SunSeries(sun.psi, sun.I_dr0, sun.I_df0), _band_w(nb, 3))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
def test_options(uniform):
    """n79 '9sky' and 4s mu_s = 0.33998."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(4, 25, 30, 3, uniform=uniform)
    _assert_slices(batched, "n79", cols, bands, sun, _band_w(25, 4), True, tau_d_method="9sky")
    _assert_slices(batched, "4s", cols, bands, sun, _band_w(25, 4), True, mu_s=0.33998)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_nt1_equals_per_step_call(scheme):
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(9, 40, 25, 1, uniform=True)
    w = _band_w(40, 3)
    got = batched.solve_integrated_series(scheme, cols, bands, sun, w, profiles=True)
    c = batched.Columns(sun.psi[:, 0].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla)
    b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), bands.leaf_r, bands.leaf_t, bands.soil_r)
    ref = batched.solve_integrated(scheme, c, b, w, profiles=True)
    for k, v in ref.items():
        assert torch.equal(got[k][:, 0], v), (scheme, k)


@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_long_series(scheme):
    """1 column, 4 bands, 5 levels, nt = 70 000 (more than a grid dimension of 65 535 holds), compared at a sample of steps."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(1, 4, 5, 70000, uniform=False, kinds=False)
    _assert_slices(batched, scheme, cols, bands, sun, _band_w(4, 2), True, steps=(0, 1, 8, 9, 65534, 65535, 65536, 69990, 69999))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_precompute_only_then_skip(scheme):
    """PRECOMPUTE_ONLY fills the records and writes no output; SKIP_PRECOMPUTE then serves new spectra from them."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(5, 30, 21, 3, uniform=False)
    w = _band_w(30, 3)
    plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, w, profiles=True)
    for v in plan.out.values():
        v.fill_(-7.0)
    plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in plan.out.values())
    assert "k_colsun" in plan.last_kernel() and "series" not in plan.last_kernel()
    sun.I_dr0.mul_(1.25)  # new spectra, same sun: in place, so the plan's pointers see them
    sun.I_df0.add_(0.5)
    got = {k: v.clone() for k, v in plan(flags=_lib.FLAG_SKIP_PRECOMPUTE).items()}
    full = batched.solve_integrated_series(scheme, cols, bands, sun, w, profiles=True)
    for k in full:
        assert torch.equal(got[k], full[k]), (scheme, k)
    for t in range(3):
        ref = _step(batched, scheme, cols, bands, sun, t, w, True)
        for k, v in ref.items():
            assert torch.equal(got[k][:, t], v), (scheme, k, t)


@pytest.mark.parametrize("scheme", ["2s", "bl", "n79", "zq_pa"])
def test_graph_capture_and_replay(scheme):
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(12, 64, 40, 5, uniform=True)
    w = _band_w(64, 3)
    plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, w, profiles=True)
    ref = {k: v.clone() for k, v in plan().items()}  # first call on the device: uploads the quadrature tables
    torch.cuda.synchronize()
    st = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            plan(stream=st)
    for v in plan.out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(plan.out[k], ref[k]), (scheme, k)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_last_kernel_names_series_kernel(scheme):
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(3, 16, 12, 2, uniform=True)
    plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, _band_w(16, 1))
    plan()
    name = plan.last_kernel()
    want = {"n79": "k_tri_int_series", "zq": "k_tri_int_series", "zq_pa": "k_zqpa_int_series"}.get(scheme, "k_int_series")
    assert want in name and "k_colpre<canopy>" in name and "k_colsun" in name, name


@pytest.mark.parametrize("scheme", SCHEMES)
def test_nb_1025_unsupported_and_untouched(scheme):
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(2, 1025, 6, 2, uniform=True)
    plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, _band_w(1025, 2), profiles=True)
    for v in plan.out.values():
        v.fill_(3.5)
    plan.workspace.fill_(0x5A)
    with pytest.raises(Exception) as ei:
        plan()
    torch.cuda.synchronize()
    assert "not supported" in str(ei.value) or "-3" in str(ei.value), str(ei.value)
    assert all(bool((v == 3.5).all()) for v in plan.out.values())
    assert bool((plan.workspace == 0x5A).all())  # nothing written at all: not even the records
    # the raw status
    st = plan._fn(_lib.SCHEME_IDS[scheme], ctypes.byref(plan._c), ctypes.byref(plan._b), ctypes.byref(plan._s), ctypes.byref(plan._o),
                  plan.band_w.data_ptr(), 2, ctypes.byref(plan._out), plan.workspace.data_ptr(), plan.workspace.numel(),
                  torch.cuda.current_stream().cuda_stream)
    assert st == _lib.CRT_ERR_UNSUPPORTED


@pytest.mark.parametrize("scheme", ["2s", "n79"])
def test_model_run_series(scheme):
    """Model.run_series against the loop update_p(psi) / run / calc_absorption / diagnostics.band over five sun angles: 1e-12, the bar
    tests/test_gpu_band.py holds diagnostics.band outputs to (g10)."""
    from crt1d_amd import diagnostics
    from crt1d_amd.model import Model

    psis = np.deg2rad([5.0, 20.0, 40.0, 60.0, 72.0])
    names = ("PAR", "NIR", "solar")
    m = Model(scheme, nlayers=60)
    res = m.run_series(psis, bands=names)
    keys = ("I_dr", "I_df_d", "I_df_u", "F", "I_d", "aI", "aI_df", "aI_dr", "aI_sh", "aI_sl", "aI_df_sl", "aI_df_sh")
    n = 0
    for t, p in enumerate(psis):
        m.update_p(psi=float(p))
        m.run()
        m.calc_absorption()
        ds = m.to_dataset()
        for name in names:
            ref_b = diagnostics.band(ds, band_name=name)
            scale_a = float(np.abs(ref_b["aI"]).max())
            for k in keys:
                ref = np.asarray(ref_b[k])
                got = res[name][k][t]
                assert got.shape == ref.shape, (k, got.shape, ref.shape)
                scale = scale_a if k.startswith("aI") else float(np.abs(ref).max())
                err = float(np.abs(got - ref).max()) / max(scale, 1e-300)
                print(f"run_series {scheme} {name} {k} t={t}: {err:.2e}")
                assert err <= 1e-12, (name, k, t, err)
                n += 1
    assert n == 5 * 3 * 12
