"""GPU: sensor-band outputs (crt_hip_sensor_levels_f64 / _f32 / _series_f64, batched.SensorLevelsPlan / SensorLevelsSeriesPlan): the level
spectra folded with spectral responses inside the level kernels.

The yardstick of the values is the existing path: ``batched.solve_levels`` for the same inputs, contracted with the dense weights in NumPy
float64.  The bound is derived, not measured: a sum of ``n = count_s`` products in ANY order lies within ``gamma_n = n u / (1 - n u)``
(``u = 2^-53``) times ``sum |w x|`` of the exact sum, so two orders differ by at most ``2 gamma_n sum|w x|`` ~= ``n 2^-52 sum |w x|``:

    |dev - ref| <= count_s * 2^-52 * sum_b |w_s[b] X[b]|      elementwise.

Everything else in this file is bit for bit: the f32 entry against the f64 entry on the upcast spectra, a column alone against the column
in a batch, a series slice against the per-step call, a plan called twice, a captured replay."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
# (ncol, nb, nz): 107 = an odd band count; 2151 bands = three band slices; 150 levels = more caller levels than zq_pa's grid has rows
SHAPES = [(2, 1, 5), (3, 12, 7), (2, 107, 9), (2, 300, 12), (1, 2151, 6), (3, 300, 150)]
FAMILY = {"n79": "k_tri_lev_sens", "zq": "k_tri_lev_sens", "zq_pa": "k_zqpa_lev_sens"}
DEV = "cuda:0"
U52 = 2.0 ** -52


def _mods():
    from crt1d_amd import _lib, batched, synth

    return _lib, batched, synth


def _level_sets(nz):
    interior = tuple(sorted({min(max(j, 1), nz - 2) for j in (1, 2, 5)}))  # three interior levels that share a block of eight
    return [(0,), (nz - 1,), (0, nz - 1), interior]


def _dense_weights(nb, seed=0):
    """All the sensor sets of the issue in one set, clipped to nb: all ones over [0, nb); 13 overlapping supports of random positive
    weights; one band at 0 and one at nb - 1; at 2151 bands a support across a slice boundary and one inside the last slice."""
    rng = np.random.default_rng(seed)
    rows = [np.ones(nb)]
    width = max(1, min(nb, nb // 6 + 3))
    for k in range(13):
        lo = min(nb - 1, (k * max(nb - width, 0)) // 12) if nb > 1 else 0
        hi = min(nb, lo + width)
        r = np.zeros(nb)
        r[lo:hi] = rng.uniform(0.1, 1.0, hi - lo)
        rows.append(r)
    for b in (0, nb - 1):
        r = np.zeros(nb)
        r[b] = 0.75
        rows.append(r)
    if nb == 2151:
        for lo, hi in ((700, 740), (1500, 2100)):  # slices of 717 bands: [700, 740) crosses 717, [1500, 2100) lies in [1434, 2151)
            r = np.zeros(nb)
            r[lo:hi] = rng.uniform(0.1, 1.0, hi - lo)
            rows.append(r)
    return np.stack(rows)


def _case(ncol, nb, nz, *, uniform, seed=11, dtype=torch.float64):
    _lib, batched, synth = _mods()
    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform)
    cols, bands = batched.Columns.from_host(d, DEV), batched.Bands.from_host(d, DEV)
    if dtype == torch.float32:
        bands = _to(bands, dtype)
    return d, cols, bands


def _to(bands, dtype):
    _lib, batched, synth = _mods()
    return batched.Bands(*[None if getattr(bands, k) is None else getattr(bands, k).to(dtype)
                           for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])


def _assert_bound(got, spectra, w, count, what):
    """got (..., nsel, nsens) against einsum(spectra (..., nsel, nb), w (nsens, nb)) at the derived bound."""
    x = spectra.double().cpu().numpy() if isinstance(spectra, torch.Tensor) else np.asarray(spectra, dtype=np.float64)
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = np.einsum("...rb,sb->...rs", x, w)
    mag = np.einsum("...rb,sb->...rs", np.abs(x), np.abs(w))
    bound = count.astype(np.float64) * U52 * mag
    err = np.abs(g - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |dev - ref| / bound = {worst:.3f}")
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert np.all(np.isfinite(g)) and np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_against_levels_and_numpy(scheme, uniform):
    """(1) every shape x level set x sensor set against solve_levels + einsum at the derived bound; (6) sensor_albedo is the ratio of those."""
    _lib, batched, synth = _mods()
    for ncol, nb, nz in SHAPES:
        d, cols, bands = _case(ncol, nb, nz, uniform=uniform, seed=3 + nb)
        w = _dense_weights(nb)
        sens = batched.SensorSet(w)
        assert sens.w.device == cols.device and sens.nsens == w.shape[0]
        for lev in _level_sets(nz):
            plan = batched.SensorLevelsPlan(scheme, cols, bands, lev, sens)
            got = plan()
            torch.cuda.synchronize()
            name = plan.last_kernel()
            per = int(re.search(r"slice=(\d+)", name).group(1))  # several band slices <=> the finish kernel
            assert FAMILY.get(scheme, "k_lev_sens") in name and ("k_sens_finish" in name) == (per < nb) and (nb <= 1024 or per < nb), name
            spectra = batched.solve_levels(scheme, cols, bands, lev)
            for k in KEYS:
                assert got[k].shape == (ncol, len(lev), sens.nsens) and got[k].dtype == torch.float64
                _assert_bound(got[k], spectra[k], w, sens.count, f"{scheme} {(ncol, nb, nz)} {lev} {k}")
        alb = batched.sensor_albedo(scheme, cols, bands, sens)
        top = batched.solve_sensor_levels(scheme, cols, bands, (nz - 1,), sens)
        assert alb.shape == (ncol, sens.nsens)
        assert torch.equal(alb, top["I_df_u"][:, 0] / (top["I_dr"][:, 0] + top["I_df_d"][:, 0])), (scheme, (ncol, nb, nz))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_f32_entry_is_the_f64_entry_on_the_upcast_spectra(scheme, uniform):
    """(2) float spectra are widened on load; everything after that is the f64 code: bit for bit."""
    _lib, batched, synth = _mods()
    for ncol, nb, nz in SHAPES:
        d, cols, b32 = _case(ncol, nb, nz, uniform=uniform, seed=5, dtype=torch.float32)
        b64 = _to(b32, torch.float64)
        sens = batched.SensorSet(_dense_weights(nb))
        for lev in _level_sets(nz)[2:]:
            p32 = batched.SensorLevelsPlan(scheme, cols, b32, lev, sens)
            a = p32()
            assert p32._entry == "crt_hip_sensor_levels_f32" and " f32" in p32.last_kernel(), p32.last_kernel()
            b = batched.solve_sensor_levels(scheme, cols, b64, lev, sens)
            torch.cuda.synchronize()
            for k in KEYS:
                assert a[k].dtype == torch.float64 and torch.equal(a[k], b[k]), (scheme, (ncol, nb, nz), lev, k)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_independence(scheme, uniform):
    """(3) each column of a 3-column call equals the 1-column call, bit for bit (also with three band slices)."""
    _lib, batched, synth = _mods()
    for ncol, nb, nz in [(3, 12, 7), (3, 300, 150), (3, 2151, 6)]:
        d, cols, bands = _case(ncol, nb, nz, uniform=uniform, seed=9)
        sens = batched.SensorSet(_dense_weights(nb))
        lev = _level_sets(nz)[3] + (nz - 1,)
        full = batched.solve_sensor_levels(scheme, cols, bands, lev, sens)
        for c in range(ncol):
            one = batched.solve_sensor_levels(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), lev, sens)
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(full[k][c:c + 1], one[k]), (scheme, (ncol, nb, nz), c, k)


def _series_case(ncol, nb, nz, nt, *, uniform, seed=21, table=False):
    _lib, batched, synth = _mods()
    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform)
    s = synth.make_sun_series(d, nt, seed=seed + 1)
    cols, bands, sun = batched.Columns.from_host(d, DEV), batched.Bands.from_host(d, DEV), batched.SunSeries.from_host(s, DEV)
    if table:  # column 0 as a CRT_G_TABLE column: the canopy record from g_table, the sun records from the per-step g_at_psi
        from crt1d_amd import leaf_angle

        nodes, x = _lib.quad_nodes(0.501), d["g_param"]
        G = leaf_angle.G_ellipsoidal_approx
        tab = np.stack([G(nodes, x[c]) for c in range(ncol)])
        gat = np.stack([G(s["psi"][c], x[c]) for c in range(ncol)])
        kind = d["g_kind"].copy()
        kind[0] = 6
        cols = batched.Columns(cols.psi, cols.lai, torch.as_tensor(kind, device=DEV), cols.g_param, cols.mla,
                               torch.zeros(ncol, dtype=torch.float64, device=DEV), torch.as_tensor(tab, device=DEV))
        sun = batched.SunSeries(sun.psi, sun.I_dr0, sun.I_df0, torch.as_tensor(gat, device=DEV))
    return cols, bands, sun


def _step_inputs(batched, cols, bands, sun, t):
    c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla,
                        None if sun.g_at_psi is None else sun.g_at_psi[:, t].contiguous(), cols.g_table)
    rows = max(sun.I_dr0.shape[0], bands.leaf_r.shape[0])
    ex = lambda v: v.expand(rows, -1).contiguous()  # noqa: E731
    return c, batched.Bands(ex(sun.I_dr0[:, t]), ex(sun.I_df0[:, t]), ex(bands.leaf_r), ex(bands.leaf_t), ex(bands.soil_r))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_series_slices_bitwise(scheme, uniform):
    """(4) slice [:, t] is the per-step call at that sun state, nt = 3, with a CRT_G_TABLE column; a workspace filled by
    solve_levels_series serves SKIP_PRECOMPUTE."""
    _lib, batched, synth = _mods()
    nt = 3
    for (ncol, nb, nz), table in (((3, 12, 7), True), ((2, 107, 9), False), ((1, 2151, 6), False), ((3, 300, 150), True)):
        cols, bands, sun = _series_case(ncol, nb, nz, nt, uniform=uniform, table=table)
        sens = batched.SensorSet(_dense_weights(nb))
        for lev in _level_sets(nz)[2:]:
            plan = batched.SensorLevelsSeriesPlan(scheme, cols, bands, sun, lev, sens)
            got = {k: v.clone() for k, v in plan().items()}
            torch.cuda.synchronize()
            assert FAMILY.get(scheme, "k_lev_sens") + "_series" in plan.last_kernel() and "k_colsun" in plan.last_kernel(), plan.last_kernel()
            for t in range(nt):
                c, b = _step_inputs(batched, cols, bands, sun, t)
                ref = batched.solve_sensor_levels(scheme, c, b, lev, sens)
                torch.cuda.synchronize()
                for k in KEYS:
                    assert got[k].shape == (ncol, nt, len(lev), sens.nsens)
                    assert torch.equal(got[k][:, t], ref[k]), (scheme, (ncol, nb, nz), lev, k, t)
            # records written by the level series, read by the sensor series
            need = batched.sensor_series_workspace_bytes(scheme, ncol, nz, nb, nt, len(lev), sens.nsens)
            assert need >= batched.levels_series_workspace_bytes(scheme, ncol, nz, nt)
            ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
            batched.LevelsSeriesPlan(scheme, cols, bands, sun, lev, workspace=ws)()
            again = batched.SensorLevelsSeriesPlan(scheme, cols, bands, sun, lev, sens, workspace=ws)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(again[k], got[k]), (scheme, (ncol, nb, nz), lev, k)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_per_step_workspace_of_the_levels_call_serves_skip_precompute(scheme):
    _lib, batched, synth = _mods()
    for ncol, nb, nz in [(2, 107, 9), (1, 2151, 6)]:
        d, cols, bands = _case(ncol, nb, nz, uniform=False)
        sens = batched.SensorSet(_dense_weights(nb))
        lev = (0, nz - 1)
        ref = batched.solve_sensor_levels(scheme, cols, bands, lev, sens)
        ws = torch.full((batched.sensor_workspace_bytes(scheme, ncol, nz, nb, len(lev), sens.nsens),), 0x5A, dtype=torch.uint8, device=DEV)
        batched.LevelsPlan(scheme, cols, bands, lev, workspace=ws)()
        got = batched.SensorLevelsPlan(scheme, cols, bands, lev, sens, workspace=ws)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], ref[k]), (scheme, (ncol, nb, nz), k)
        with pytest.raises(ValueError, match="workspace too small"):
            batched.SensorLevelsPlan(scheme, cols, bands, lev, sens, workspace=ws[:-8])


@pytest.mark.parametrize("series", [False, True], ids=["step", "series"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_output_subsets_guards_and_repeat(scheme, series):
    """(5) NULL outputs are honoured, nothing beyond the given arrays is written, two calls of one plan give the same bits."""
    _lib, batched, synth = _mods()
    for ncol, nb, nz in [(3, 70, 22), (2, 2151, 6)]:
        nt = 2
        cols, bands, sun = _series_case(ncol, nb, nz, nt, uniform=True)
        if not series:
            cols, bands = _step_inputs(batched, cols, bands, sun, 1)
        sens = batched.SensorSet(_dense_weights(nb))
        lev = (0, nz // 2, nz - 1)
        make = (lambda **kw: batched.SensorLevelsSeriesPlan(scheme, cols, bands, sun, lev, sens, **kw)) if series else \
               (lambda **kw: batched.SensorLevelsPlan(scheme, cols, bands, lev, sens, **kw))
        full = {k: v.clone() for k, v in make()().items()}
        shape = (ncol,) + ((nt,) if series else ()) + (len(lev), sens.nsens)
        n, guard, sentinel = int(np.prod(shape)), 4096, -12345.5
        for keys in (("I_df_u",), ("F", "I_dr"), ("I_df_d", "I_df_u", "F")):
            bufs = {k: torch.full((n + 2 * guard,), sentinel, dtype=torch.float64, device=DEV) for k in keys}
            out = {k: v[guard:guard + n].view(shape) for k, v in bufs.items()}
            plan = make(keys=keys, out=out)
            assert [bool(getattr(plan._out, k)) for k in KEYS] == [k in keys for k in KEYS]  # NULL for what is not asked for
            got = plan()
            torch.cuda.synchronize()
            assert set(got) == set(keys)
            first = {k: got[k].clone() for k in keys}
            for k in keys:
                assert torch.equal(got[k], full[k]), (scheme, keys, k)
                assert bool((bufs[k][:guard] == sentinel).all()) and bool((bufs[k][guard + n:] == sentinel).all()), (scheme, keys, k)
                got[k].fill_(sentinel)
            plan()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(got[k], first[k]), (scheme, keys, k)


@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])  # one per kernel family
def test_model_entries(scheme):
    """(7) Model.run_sensors against run() + a NumPy reduction of m.out rows, Model.run_series_sensors against run_series_levels, at the
    bound of (1)."""
    from crt1d_amd import batched
    from crt1d_amd.model import Model

    m = Model(scheme, nlayers=60)
    nz, nb = len(m._p["lai"]), m.nwl
    w = _dense_weights(nb)
    count = batched.SensorSet(w).count
    levels = (0, 7, nz - 1)
    before = float(m._p["psi"])
    res = m.run_sensors(w, levels)
    top = m.run_sensors(batched.SensorSet(w))  # the default levels (0, -1), a ready-made set
    assert float(m._p["psi"]) == before and not m._run_count
    m.run()
    for k in KEYS:
        rows = np.asarray(m.out[k])
        assert res[k].shape == (len(levels), w.shape[0])
        _assert_bound(res[k], rows[list(levels)], w, count, f"run_sensors {scheme} {k}")
        _assert_bound(top[k], rows[[0, nz - 1]], w, count, f"run_sensors {scheme} {k} default levels")
    psis = np.deg2rad([5.0, 40.0, 72.0])
    ser = m.run_series_sensors(psis, w, levels)
    spectra = m.run_series_levels(psis, levels)
    for k in KEYS:
        assert ser[k].shape == (3, len(levels), w.shape[0])
        _assert_bound(ser[k], spectra[k], w, count, f"run_series_sensors {scheme} {k}")
    with pytest.raises(ValueError):
        m.run_sensors(np.ones((2, nb + 1)))


@pytest.mark.parametrize("nb", [107, 2151])
@pytest.mark.parametrize("scheme", ["2s", "zq", "zq_pa"])
def test_graph_capture_and_replay(scheme, nb):
    """(8) one capture and replay of a warmed-up plan gives the same bits (default queue settings); with three slices the finish kernel is
    part of the graph."""
    _lib, batched, synth = _mods()
    d, cols, bands = _case(2, nb, 9, uniform=False)
    sens = batched.SensorSet(_dense_weights(nb))
    plan = batched.SensorLevelsPlan(scheme, cols, bands, (0, 8), sens)
    plan()
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in plan.out.items()}
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
    for k in ref:
        assert torch.equal(plan.out[k], ref[k]), (scheme, k)


def test_plan_argument_checks():
    _lib, batched, synth = _mods()
    d, cols, bands = _case(2, 16, 6, uniform=True)
    sens = batched.SensorSet(np.ones((3, 16)))
    with pytest.raises(ValueError, match="built for nb = 16"):
        batched.SensorLevelsPlan("2s", cols, batched.Bands.from_host(synth.make_columns(2, 17, 6, seed=1), DEV), (0,), sens)
    with pytest.raises(ValueError, match="live on"):
        batched.SensorLevelsPlan("2s", cols, bands, (0,), batched.SensorSet(np.ones((3, 16)), device="cpu"))
    with pytest.raises(ValueError):
        batched.SensorLevelsPlan("2s", cols, bands, (6,), sens)
    with pytest.raises(TypeError):  # the sums are float64 for both storage types
        batched.SensorLevelsPlan("2s", cols, _to(bands, torch.float32), (0,), sens, keys=("F",),
                                 out={"F": torch.empty(2, 1, 3, dtype=torch.float32, device=DEV)})
    with pytest.raises(ValueError):
        batched.SensorLevelsPlan("2s", cols, bands, (0,), sens, keys=("F",), out={"F": torch.empty(2, 1, 4, dtype=torch.float64, device=DEV)})
    with pytest.raises(ValueError, match="lacks"):
        batched.SensorLevelsPlan("2s", cols, bands, (0,), sens, out={"F": torch.empty(2, 1, 3, dtype=torch.float64, device=DEV)})
    s = synth.make_sun_series(synth.make_columns(2, 16, 6, seed=11, uniform_dlai=True), 2, seed=2)
    with pytest.raises(TypeError):  # no f32 form of the sensor series
        batched.SensorLevelsSeriesPlan("2s", cols, _to(bands, torch.float32), batched.SunSeriesF32.from_host(s, DEV), (0,), sens)
