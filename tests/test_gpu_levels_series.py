"""GPU: the sun-angle series of level spectra (crt_hip_levels_series_f64 / _f32, batched.LevelsSeriesPlan) against the per-step entry
crt_hip_levels_f64 / _f32, bit for bit.

The yardstick is ``LevelsPlan`` (pinned by tests/test_gpu_levels.py against the full solve): for every step ``t``, slice ``[:, t]`` of every
series output must be ``torch.equal`` to what ``LevelsPlan`` writes for the same columns with the sun and the incoming spectra of step
``t``.  There is no tolerance anywhere in this file: ``Model.run_series_levels`` is held to ``np.array_equal`` as well."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
# (ncol, nb, nz): 2151 bands = three band slices; 150 levels = more caller levels than zq_pa's grid has rows
SHAPES = [(5, 12, 60), (3, 13, 9), (4, 107, 61), (3, 300, 60), (2, 1025, 20), (1, 2151, 60), (2, 300, 150)]
FAMILY = {"n79": "k_tri_lev_series<", "zq": "k_tri_lev_series<", "zq_pa": "k_zqpa_lev_series<"}
DEV = "cuda:0"


def _mods():
    from crt1d_amd import _lib, batched, synth

    return _lib, batched, synth


def _level_sets(nz):
    block = tuple(j for j in (1, 2, 5, 9, 10, 13, 15) if j < nz)  # several levels inside one block of 8: the shared walk
    return [(0,), (nz - 1,), (0, nz - 1), tuple(range(0, nz, 2))[:64], block]


def _to(bands, dtype):
    _lib, batched, synth = _mods()
    return batched.Bands(*[None if getattr(bands, k) is None else getattr(bands, k).to(dtype)
                           for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])


def _case(ncol, nb, nz, nt, *, uniform, seed=11, shared=False, per_column_optics=True, kinds=True, dtype=torch.float64):
    _lib, batched, synth = _mods()
    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform, per_column_optics=per_column_optics)
    if kinds:  # all six closed-form leaf-angle kinds over the columns
        d["g_kind"] = (np.arange(ncol) % 6).astype(np.int32)
        d["g_param"] = np.where(d["g_kind"] == 5, np.linspace(-0.3, 0.5, ncol), d["g_param"])
    s = synth.make_sun_series(d, nt, seed=seed + 1, shared=shared)
    cols = batched.Columns.from_host(d, DEV)
    bands = batched.Bands.from_host(d, DEV)
    if dtype == torch.float32:
        bands = _to(bands, dtype)
        sun = batched.SunSeriesF32.from_host(s, DEV)
    else:
        sun = batched.SunSeries.from_host(s, DEV)
    return d, s, cols, bands, sun


def _step_inputs(batched, cols, bands, sun, t):
    """Columns and Bands of the per-step call for sun state t."""
    ncol = cols.ncol
    c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla,
                        None if sun.g_at_psi is None else sun.g_at_psi[:, t].contiguous(), cols.g_table)
    idr, idf = sun.I_dr0[:, t], sun.I_df0[:, t]
    lr, lt, sr = bands.leaf_r, bands.leaf_t, bands.soil_r
    rows = max(idr.shape[0], lr.shape[0])
    ex = lambda v: v.expand(rows, -1).contiguous()  # noqa: E731  (Bands wants one shape for all five)
    assert rows in (1, ncol)
    return c, batched.Bands(ex(idr), ex(idf), ex(lr), ex(lt), ex(sr))


def _assert_slices(batched, scheme, cols, bands, sun, levels, steps=None, step_inputs=None, keys=KEYS, **kw):
    plan = batched.LevelsSeriesPlan(scheme, cols, bands, sun, levels, keys=keys, **kw)
    got = plan()
    torch.cuda.synchronize()
    name = plan.last_kernel()
    assert FAMILY.get(scheme, "k_lev_series<") in name and "k_colsun" in name, name
    assert (" f32" in name) == (bands.dtype == torch.float32), name
    assert set(got) == set(keys)
    for t in (range(sun.nt) if steps is None else steps):
        c, b = step_inputs[t] if step_inputs is not None else _step_inputs(batched, cols, bands, sun, t)
        ref = batched.LevelsPlan(scheme, c, b, levels, keys=keys, **kw)()
        torch.cuda.synchronize()
        for k, v in ref.items():
            assert got[k].shape == (cols.ncol, sun.nt, len(plan.levels), bands.nb) and got[k].dtype == bands.dtype
            assert torch.equal(got[k][:, t], v), (scheme, k, t, levels, float((got[k][:, t].double() - v.double()).abs().max()))
    return plan, got


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_series_slices_bitwise(scheme, uniform, dtype):
    """8 schemes x uniform / ragged x f64 / f32 x 7 shapes x nt in {1, 3, 24} x 5 level sets: every slice against LevelsPlan."""
    _lib, batched, synth = _mods()
    for ncol, nb, nz in SHAPES:
        for nt in (1, 3, 24):
            d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=uniform, seed=100 + nt, dtype=dtype)
            steps = [_step_inputs(batched, cols, bands, sun, t) for t in range(nt)]
            for lev in _level_sets(nz):
                _assert_slices(batched, scheme, cols, bands, sun, lev, step_inputs=steps)  # every t


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])  # one per kernel family
def test_slices_are_rows_of_the_full_solve(scheme, uniform):
    _lib, batched, synth = _mods()
    for ncol, nb, nz in [(4, 107, 61), (1, 2151, 60), (2, 300, 150)]:
        nt = 3
        d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=uniform, seed=7)
        for lev in _level_sets(nz)[2:]:
            got = batched.solve_levels_series(scheme, cols, bands, sun, lev)
            idx = torch.tensor(lev, device=DEV)
            for t in range(nt):
                c, b = _step_inputs(batched, cols, bands, sun, t)
                full = batched.solve(scheme, c, b)
                torch.cuda.synchronize()
                for k in KEYS:
                    assert torch.equal(got[k][:, t], full[k].index_select(1, idx)), (scheme, (ncol, nb, nz), lev, k, t)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_shared_series_and_broadcast_optics(scheme, dtype):
    """col_stride = 0 of the sun's spectra against the same series repeated per column; broadcast leaf optics (bands.col_stride = 0)."""
    _lib, batched, synth = _mods()
    ncol, nb, nz, nt = 6, 38, 33, 4
    lev = (0, 3, 17, 32)
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=False, shared=True, dtype=dtype)
    assert sun.col_stride == 0
    _, a = _assert_slices(batched, scheme, cols, bands, sun, lev)
    rep = type(sun)(sun.psi, sun.I_dr0.expand(ncol, -1, -1).contiguous(), sun.I_df0.expand(ncol, -1, -1).contiguous())
    assert rep.col_stride == nt * nb
    b = batched.solve_levels_series(scheme, cols, bands, rep, lev)
    for k in a:
        assert torch.equal(a[k], b[k]), (scheme, k)
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=True, per_column_optics=False, dtype=dtype)
    bands = batched.Bands(None, None, bands.leaf_r, bands.leaf_t, bands.soil_r)  # built without the incoming spectra
    assert bands.col_stride(ncol) == 0
    _assert_slices(batched, scheme, cols, bands, sun, lev)


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
    _assert_slices(batched, scheme, cols, bands, sun, (0, 8, 9, 16))
    with pytest.raises(ValueError):
        batched.LevelsSeriesPlan(scheme, cols, bands, batched.SunSeries(sun.psi, sun.I_dr0, sun.I_df0), (0,))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
def test_options(uniform):
    """'9sky' for the schemes with a tau_d quadrature in their record, and 4s mu_s = 0.33998."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(4, 25, 30, 3, uniform=uniform)
    for scheme in ("n79", "bl", "zq", "zq_pa"):
        _assert_slices(batched, scheme, cols, bands, sun, (0, 7, 29), tau_d_method="9sky")
    _assert_slices(batched, "4s", cols, bands, sun, (0, 7, 29), mu_s=0.33998)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_output_subsets_write_only_what_is_asked(scheme, dtype):
    """A subset of the four outputs, the others NULL: the given arrays lie between guard zones that stay untouched."""
    _lib, batched, synth = _mods()
    ncol, nb, nz, nt = 3, 70, 22, 4
    lev = (0, 9, 21)
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=True, dtype=dtype)
    full = batched.solve_levels_series(scheme, cols, bands, sun, lev)
    n, guard, sentinel = ncol * nt * len(lev) * nb, 4096, -12345.5
    for keys in (("I_df_u",), ("F", "I_dr"), ("I_df_d", "I_df_u", "F")):
        bufs = {k: torch.full((n + 2 * guard,), sentinel, dtype=dtype, device=DEV) for k in keys}
        out = {k: v[guard:guard + n].view(ncol, nt, len(lev), nb) for k, v in bufs.items()}
        plan = batched.LevelsSeriesPlan(scheme, cols, bands, sun, lev, keys=keys, out=out)
        assert [bool(getattr(plan._out, k)) for k in KEYS] == [k in keys for k in KEYS]  # NULL for what is not asked for
        got = plan()
        torch.cuda.synchronize()
        assert set(got) == set(keys)
        for k in keys:
            assert torch.equal(got[k], full[k]), (scheme, keys, k)
            assert bool((bufs[k][:guard] == sentinel).all()) and bool((bufs[k][guard + n:] == sentinel).all()), (scheme, keys, k)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_precompute_only_then_skip(scheme):
    """PRECOMPUTE_ONLY fills the records and writes no output; SKIP_PRECOMPUTE then serves new spectra from them."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(5, 30, 21, 3, uniform=False)
    lev = (0, 10, 20)
    plan = batched.LevelsSeriesPlan(scheme, cols, bands, sun, lev)
    for v in plan.out.values():
        v.fill_(-7.0)
    plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in plan.out.values())
    assert "k_colsun" in plan.last_kernel() and "series" not in plan.last_kernel()
    sun.I_dr0.mul_(1.25)  # new spectra, same sun: in place, so the plan's pointers see them
    sun.I_df0.add_(0.5)
    got = {k: v.clone() for k, v in plan(flags=_lib.FLAG_SKIP_PRECOMPUTE).items()}
    full = batched.solve_levels_series(scheme, cols, bands, sun, lev)
    for k in full:
        assert torch.equal(got[k], full[k]), (scheme, k)
    for t in range(3):
        c, b = _step_inputs(batched, cols, bands, sun, t)
        ref = batched.solve_levels(scheme, c, b, lev)
        for k, v in ref.items():
            assert torch.equal(got[k][:, t], v), (scheme, k, t)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_workspace_is_shared_with_the_integrated_series(scheme):
    """The header's claim: the record layouts of the two series entries coincide.  Records written by the integrated series serve the
    level series with SKIP_PRECOMPUTE, and the other way round, in one buffer of crt_hip_series_workspace_bytes."""
    _lib, batched, synth = _mods()
    ncol, nb, nz, nt = 4, 26, 19, 3
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=False)
    lev = (0, 8, 18)
    w = torch.as_tensor(np.random.default_rng(5).uniform(0.0, 1.0, (2, nb)), device=DEV)
    nbytes = batched.series_workspace_bytes(scheme, ncol, nz, nb, nt)
    assert batched.levels_series_workspace_bytes(scheme, ncol, nz, nt) <= nbytes
    ref_l = {k: v.clone() for k, v in batched.solve_levels_series(scheme, cols, bands, sun, lev).items()}
    ref_i = {k: v.clone() for k, v in batched.solve_integrated_series(scheme, cols, bands, sun, w, profiles=True).items()}
    # integrated series writes the records, the level series reads them
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    batched.IntegratedSeriesPlan(scheme, cols, bands, sun, w, workspace=ws)(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    got = batched.LevelsSeriesPlan(scheme, cols, bands, sun, lev, workspace=ws)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
    torch.cuda.synchronize()
    for k in ref_l:
        assert torch.equal(got[k], ref_l[k]), (scheme, k)
    # ... and the other way round
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    batched.LevelsSeriesPlan(scheme, cols, bands, sun, lev, workspace=ws)(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    got = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, w, profiles=True, workspace=ws)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
    torch.cuda.synchronize()
    for k in ref_i:
        assert torch.equal(got[k], ref_i[k]), (scheme, k)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", ["2s", "bl", "n79", "zq_pa"])
def test_graph_capture_and_replay(scheme, dtype):
    """Captured after the first call on the device; the replay is bitwise the direct call, also after new spectra have been written into
    the same input buffers."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(12, 64, 40, 5, uniform=True, dtype=dtype)
    lev = (0, 13, 39)
    plan = batched.LevelsSeriesPlan(scheme, cols, bands, sun, lev)
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
    sun.I_dr0.mul_(0.75)  # new spectra in the same buffers
    sun.I_df0.add_(0.25)
    for v in plan.out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in plan.out.items()}
    ref2 = batched.solve_levels_series(scheme, cols, bands, sun, lev)
    torch.cuda.synchronize()
    for k in ref2:
        assert torch.equal(got[k], ref2[k]), (scheme, k)
    assert not torch.equal(got["I_dr"], ref["I_dr"]), scheme  # the replay read the new spectra


@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_long_series(scheme):
    """1 column, 4 bands, 5 levels, nt = 70 000 (more than a grid dimension of 65 535 holds), compared at a sample of steps."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(1, 4, 5, 70000, uniform=False, kinds=False)
    _assert_slices(batched, scheme, cols, bands, sun, (0, 2, 4), steps=(0, 1, 8, 9, 65534, 65535, 65536, 69990, 69999))


def test_long_series_with_band_slices():
    """t over two grid dimensions AND two band slices in the third: 1 column, 1030 bands, nt = 66 000."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(1, 1030, 4, 66000, uniform=True, kinds=False)
    _assert_slices(batched, "2s", cols, bands, sun, (0, 3), steps=(0, 1, 65534, 65535, 65536, 65999), keys=("I_df_u",))


def test_unsupported_shape_is_untouched():
    """n79 at nz = 3000 (the level kernels serve nz <= 1360): CRT_ERR_UNSUPPORTED, found before K0 -- outputs and workspace untouched."""
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(2, 8, 3000, 2, uniform=True)
    plan = batched.LevelsSeriesPlan("n79", cols, bands, sun, (0, 2999))
    for v in plan.out.values():
        v.fill_(3.5)
    plan.workspace.fill_(0x5A)
    with pytest.raises(Exception) as ei:
        plan()
    torch.cuda.synchronize()
    assert "not supported" in str(ei.value) or "-3" in str(ei.value), str(ei.value)
    assert all(bool((v == 3.5).all()) for v in plan.out.values())
    assert bool((plan.workspace == 0x5A).all())  # nothing written at all: not even the records
    st = plan._fn(_lib.SCHEME_IDS["n79"], ctypes.byref(plan._c), ctypes.byref(plan._b), ctypes.byref(plan._s), ctypes.byref(plan._o),
                  plan._lev, 2, ctypes.byref(plan._out), plan.workspace.data_ptr(), plan.workspace.numel(),
                  torch.cuda.current_stream().cuda_stream)
    assert st == _lib.CRT_ERR_UNSUPPORTED
    # the closed forms serve this depth (record in LDS: 16 + 2 * 3000 doubles)
    _assert_slices(batched, "2s", cols, bands, sun, (0, 1501, 2999))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_last_kernel_names_series_kernel(scheme, dtype):
    _lib, batched, synth = _mods()
    d, s, cols, bands, sun = _case(3, 16, 12, 2, uniform=True, dtype=dtype)
    plan = batched.LevelsSeriesPlan(scheme, cols, bands, sun, (0, 11))
    plan()
    name = plan.last_kernel()
    assert FAMILY.get(scheme, "k_lev_series<") in name and "k_colpre<canopy>" in name and "k_colsun" in name and "nt=2" in name, name


def test_dtype_mismatch_is_rejected():
    _lib, batched, synth = _mods()
    d, s, cols, b64, s64 = _case(3, 16, 12, 2, uniform=True)
    _, _, _, b32, s32 = _case(3, 16, 12, 2, uniform=True, dtype=torch.float32)
    with pytest.raises(TypeError):
        batched.LevelsSeriesPlan("2s", cols, b64, s32, (0,))
    with pytest.raises(TypeError):
        batched.LevelsSeriesPlan("2s", cols, b32, s64, (0,))
    with pytest.raises(TypeError):
        batched.IntegratedSeriesPlan("2s", cols, b64, s32, torch.ones(1, 16, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        batched.LevelsSeriesPlan("2s", cols, b64, s64, (0,), out={"I_dr": torch.empty(3, 2, 1, 16, dtype=torch.float64, device=DEV)})
    with pytest.raises(TypeError):
        batched.LevelsSeriesPlan("2s", cols, b64, s64, (0,), keys=("F",), out={"F": torch.empty(3, 2, 1, 16, dtype=torch.float32, device=DEV)})
    with pytest.raises(ValueError):
        batched.LevelsSeriesPlan("2s", cols, b64, s64, (0,), keys=("F",), out={"F": torch.empty(3, 1, 2, 16, dtype=torch.float64, device=DEV)})


@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_model_run_series_levels(scheme):
    """Model.run_series_levels against the loop update_p(psi) / run / row selection over five sun angles: np.array_equal -- no band sum is
    involved, and both paths hand psi and the closed-form G to the device in the same way."""
    from crt1d_amd.model import Model

    psis = np.deg2rad([5.0, 20.0, 40.0, 60.0, 72.0])
    m = Model(scheme, nlayers=60)
    nz = len(m._p["lai"])
    levels = (0, 7, nz // 2, nz - 1)
    res = m.run_series_levels(psis, levels)
    top = m.run_series_levels(psis, -1)
    n = 0
    for t, p in enumerate(psis):
        m.update_p(psi=float(p))
        m.run()
        for k in KEYS:
            ref = np.asarray(m.out[k])[list(levels)]
            got = res[k][t]
            assert got.shape == ref.shape == (len(levels), m.nwl), (k, got.shape, ref.shape)
            err = float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-300)
            print(f"run_series_levels {scheme} {k} t={t}: max rel diff {err:.2e}")
            assert np.array_equal(got, ref), (scheme, k, t, err)
            assert np.array_equal(top[k][t, 0], np.asarray(m.out[k])[nz - 1]), (scheme, k, t)
            n += 1
    assert n == 5 * 4
    with pytest.raises(ValueError):
        m.run_series_levels(psis, nz)
    with pytest.raises(ValueError):
        m.run_series_levels(psis, 0, I_dr0_all=np.ones((3, m.nwl)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_spectral_totals_series(scheme, dtype):
    _lib, batched, synth = _mods()
    ncol, nb, nz, nt = 4, 45, 24, 3
    d, s, cols, bands, sun = _case(ncol, nb, nz, nt, uniform=False, dtype=dtype)
    got = batched.spectral_totals_series(scheme, cols, bands, sun)
    assert got.shape == (ncol, nt, nb, 4) and got.dtype == torch.float64
    for t in range(nt):
        c, b = _step_inputs(batched, cols, bands, sun, t)
        ref = batched.spectral_totals(scheme, c, b)
        assert torch.equal(got[:, t], ref), (scheme, t)
