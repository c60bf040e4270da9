"""GPU: spectral inputs on the device (crt_hip_avg_optical_prop_f64, crt_hip_bands_from_spectra_f64, k_spectral_prep).

Parity bar against the reference (fixture g12, tools/gen_spectral_prep_golden.py): relative error <= 1e-12 in every finite element, NaN
exactly where the reference has NaN.  Every term is non-negative (y >= 0, light >= 0, widths > 0), so nothing cancels and the error of a
result is bounded by (number of additions <= nx + nsub ~ 3000) x 2.2e-16 ~ 7e-13 whatever the summation order; NumPy's pairwise ``sum`` is
the one order the kernel does not reproduce.  Shapes the fixture does not hold are compared with the sequential NumPy restatement of
tests/test_spectral_prep_cpu.py (itself within 2.1e-15 of the reference there), under the same bar.

Everything else is bitwise: the contract of the kernel is that a result depends only on its own spectrum, band and light."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_spectral_prep_cpu import LIGHTS, MODES, PARITY_BAR, rel_err, restate

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("parnir", "sp2", "odd", "outside", "nx2", "nx5", "nx9")


def _mods():
    from crt1d_amd import _lib, batched
    from crt1d_amd import spectra as sp

    return _lib, batched, sp


@pytest.fixture(scope="module")
def gold():
    return load_golden("g12_spectral_prep")


def dv(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def same(a, b):
    a, b = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def kw_of(light, g, c):
    """keyword arguments of the two entry points for a light of the fixture"""
    if light.startswith("planck"):
        k = dict(light="planck", T_K=float(light[6:]))
        return k, k
    if light == "table":
        return dict(light="table", light_x=g[f"{c}_xs"], light_y=g[f"{c}_si"][0] + g[f"{c}_si"][1]), dict(light="table")
    return dict(light="uniform"), dict(light="uniform")


def optics(b):
    return torch.stack([b.leaf_r, b.leaf_t, b.soil_r])[:, 0]


@pytest.mark.parametrize("c", CASES)
def test_parity_with_the_reference(gold, c):
    """Both entry points on every edge set x light x x_smear_nb of the fixture; they agree with each other bitwise."""
    _lib, batched, sp = _mods()
    x, y, xs, si, edges = (gold[f"{c}_{k}"] for k in ("x", "y", "xs", "si", "edges"))
    yd, sid = dv(y), dv(si)
    worst = 0.0
    for m, nbm in MODES:
        for light in LIGHTS:
            ref = gold[f"{c}_{light}_{m}"]
            if c not in gold["nan_cases"]:
                assert np.isfinite(ref).all()
            k_avg, k_bands = kw_of(light, gold, c)
            got = sp.avg_optical_prop_batched(x, yd, edges, x_smear_nb=nbm, **k_avg)
            b = batched.Bands.from_spectra(x, yd[0], yd[1], yd[2], xs, sid[0], sid[1], edges, x_smear_nb=nbm, **k_bands)
            torch.cuda.synchronize()
            assert got.shape == (3, edges.size - 1) and b.nb == edges.size - 1
            worst = max(worst, rel_err(got.cpu().numpy(), ref))
            assert same(optics(b), got), (light, m)
            worst = max(worst, rel_err(torch.stack([b.I_dr0, b.I_df0])[:, 0].cpu().numpy(), gold[f"{c}_I"]))
    print(f"{c}: worst relative error against the reference = {worst:.2e}")
    assert worst <= PARITY_BAR


def test_single_spectrum_drop_ins(gold):
    _lib, batched, sp = _mods()
    c = "odd"
    x, y, xs, si, edges = (gold[f"{c}_{k}"] for k in ("x", "y", "xs", "si", "edges"))
    got = sp.smear_avg_optical_prop(x, y[1], edges, light="planck", T_K=3000)
    assert isinstance(got, np.ndarray) and rel_err(got[None], gold[f"{c}_planck3000_d"][1:2]) <= PARITY_BAR
    got = sp.smear_avg_optical_prop(x, y[0], edges, light=(xs, si[0] + si[1]), x_smear_nb=7)
    assert rel_err(got[None], gold[f"{c}_table_7"][0:1]) <= PARITY_BAR
    one = sp.avg_optical_prop(y[2], (edges[2], edges[3]), x=x, light="uniform")
    assert isinstance(one, float) and abs(one - gold[f"{c}_uniform_d"][2, 2]) <= PARITY_BAR * one
    i_dr, i_df, dwl = sp.smear_si_batched(xs, si[0], dv(si[1]), edges)
    assert rel_err(torch.cat([i_dr, i_df]).cpu().numpy(), gold[f"{c}_I"]) <= PARITY_BAR and same(dwl, np.diff(edges))


@pytest.mark.parametrize("c", ["parnir", "sp2", "odd", "nx2", "nx9"])
def test_sub_bin_averages_and_irradiance_are_smear_tuv(gold, c):
    """The sub-bin averages (debug output) are crt_hip_smear_tuv_f64 on the same sub-edges, bit for bit, and the band irradiances are
    smear_tuv x dwl formed in torch."""
    _lib, batched, sp = _mods()
    x, y, xs, si, edges = (gold[f"{c}_{k}"] for k in ("x", "y", "xs", "si", "edges"))
    for m, nbm in MODES:
        lo, hi = gold[f"{c}_sub_{m}"]
        y_sub = torch.full((3, lo.size), -7.0, dtype=torch.float64, device=DEV)
        sp.avg_optical_prop_batched(x, y, edges, light="uniform", x_smear_nb=nbm, y_sub=y_sub)
        assert same(y_sub, sp.smear_tuv_batched(x, y, np.concatenate([lo, hi[-1:]])))
    b = batched.Bands.from_spectra(x, dv(y[0]), dv(y[1]), dv(y[2]), xs, dv(si[0]), dv(si[1]), edges)
    i_dr, i_df, _ = sp.smear_si_batched(xs, si[0], si[1], edges)
    assert same(b.I_dr0, i_dr) and same(b.I_df0, i_df)
    assert same(b.I_dr0, sp.smear_tuv_batched(xs, si[:1], edges) * dv(np.diff(edges)))


def _columns(gold, ncol):
    """ncol columns of per-column spectra on the 2101-point grid (fills the LDS staging): the sample spectra, scaled per column."""
    y, si = gold["parnir_y"], gold["parnir_si"]
    f = 1.0 + 0.003 * np.arange(ncol)[:, None]
    return [dv(y[q] * f / (1 + q)) for q in range(3)], [dv(si[q] * (2.0 - f)) for q in range(2)]


@pytest.mark.parametrize("light", ["table", "planck"])
def test_results_do_not_depend_on_the_batch(gold, light):
    """Column c of an ncol-column call equals the one-column call, shared inputs equal the same spectra tiled, a second call into the
    same memory reproduces the bits, and the two entry points agree (light_group = 3 with one light row per column)."""
    _lib, batched, sp = _mods()
    x, xs, edges = gold["parnir_x"], gold["parnir_xs"], gold["sp2_edges"]
    opt, si = _columns(gold, 70)
    names = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")

    def run(cols):
        return batched.Bands.from_spectra(x, *(t[cols] for t in opt), xs, *(t[cols] for t in si), edges, light=light)

    full = run(slice(0, 70))
    assert full.I_dr0.shape == (70, edges.size - 1)
    for ncol in (1, 2, 3):
        part = run(slice(0, ncol))
        for k in names:
            assert same(getattr(part, k), getattr(full, k)[:ncol]), (ncol, k)
    last = run(slice(69, 70))
    again = run(slice(0, 70))
    for k in names:
        assert same(getattr(last, k), getattr(full, k)[69:]), k
        assert same(getattr(again, k), getattr(full, k)), k
    # shared (stride 0) against tiled: every input shared, then the optics shared and the irradiance per column
    shared = batched.Bands.from_spectra(x, opt[0][4], opt[1][4], opt[2][4], xs, si[0][4], si[1][4], edges, light=light)
    tiled = batched.Bands.from_spectra(x, *(t[4:5].repeat(3, 1) for t in opt), xs, *(t[4:5].repeat(3, 1) for t in si), edges, light=light)
    mixed = batched.Bands.from_spectra(x, opt[0][4], opt[1][4:5].repeat(3, 1), opt[2][4], xs, si[0][4:5].repeat(3, 1), si[1][4], edges, light=light)
    for k in names:
        assert getattr(shared, k).shape == (1, edges.size - 1)
        assert same(getattr(tiled, k), getattr(shared, k).repeat(3, 1)) and same(getattr(mixed, k), getattr(tiled, k)), k
        assert same(getattr(tiled, k)[0], getattr(full, k)[4]), k
    # the first entry on the 3 x 5 spectra of columns 0 .. 4, one light row per column
    y = torch.stack([t[:5] for t in opt], dim=1).reshape(15, -1)
    k_avg = dict(light="table", light_x=xs, light_y=(si[0] + si[1])[:5], light_group=3) if light == "table" else dict(light="planck")
    out = torch.full((15, edges.size - 1), -7.0, dtype=torch.float64, device=DEV)
    got = sp.avg_optical_prop_batched(x, y, edges, out=out, **k_avg)
    assert got is out
    for q, k in enumerate(("leaf_r", "leaf_t", "soil_r")):
        assert same(out.reshape(5, 3, -1)[:, q], getattr(full, k)[:5]), k
    first = out.clone()
    sp.avg_optical_prop_batched(x, y, edges, out=out, **k_avg)
    assert same(out, first)


def test_107_narrow_bands(gold):
    """nb = 107 with one or two sub-bins per band, against the restatement (the fixture's nearest is 91 bands)."""
    _lib, batched, sp = _mods()
    x, y, xs, si = gold["parnir_x"], gold["parnir_y"], gold["parnir_xs"], gold["parnir_si"]
    edges = 0.45 + np.concatenate([[0.0], np.cumsum(np.where(np.arange(107) % 3 == 0, 0.004, 0.0075))])
    counts = sp.sub_bin_counts(x, edges)
    assert edges.size == 108 and set(counts) == {1, 2}
    nodes = _lib.planck_nodes()
    b = {light: batched.Bands.from_spectra(x, dv(y[0]), dv(y[1]), dv(y[2]), xs, dv(si[0]), dv(si[1]), edges, light=light)
         for light in ("uniform", "planck", "table")}
    for light, kw in (("uniform", dict(light="uniform")), ("planck", dict(light="planck", T_K=6000.0, nodes=nodes)),
                      ("table", dict(light="table", table=(xs, si[0] + si[1])))):
        ref, _ = restate(x, y, edges, counts, **kw)
        err = rel_err(optics(b[light]).cpu().numpy(), ref)
        print(f"{light}: {err:.2e}")
        assert err <= PARITY_BAR


def test_largest_item_count_and_one_more(gold):
    """CRT_SPECTRA_MAX_ITEMS sub-bins in two bands (128 passes of the workgroup, a band that spans passes), then one sub-bin more.
    y = a + b x under uniform light: the band average is y at the band's centre.  Bar: (nsub + trapezoids) additions of non-negative
    terms, (32768 + 4) x 2.2e-16 = 7.3e-12, the derivation of the parity bar at this length."""
    _lib, batched, sp = _mods()
    x = np.array([0.4, 0.9, 1.1, 2.0, 2.5])
    y = np.stack([0.1 + 0.2 * x, 0.7 - 0.1 * x])
    edges = np.array([0.5, 1.3, 2.4])
    n = _lib.SPECTRA_MAX_ITEMS // 2
    got = sp.avg_optical_prop_batched(x, y, edges, light="uniform", x_smear_nb=n).cpu().numpy()
    mid = 0.5 * (edges[:-1] + edges[1:])
    ref = np.stack([0.1 + 0.2 * mid, 0.7 - 0.1 * mid])
    err = float(np.max(np.abs(got - ref) / ref))
    print(f"{2 * n} sub-bins: {err:.2e}")
    assert err <= (n + 4) * 2.2e-16
    out = torch.full((2, 2), -7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="status -3"):
        sp.avg_optical_prop_batched(x, y, edges, light="uniform", x_smear_nb=n + 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    xs, si = gold["nx2_xs"], dv(gold["nx2_si"])
    with pytest.raises(RuntimeError, match="status -3"):
        batched.Bands.from_spectra(x, dv(y[0]), dv(y[1]), dv(y[0]), xs, si[0], si[1], edges, x_smear_nb=n + 1)


def test_bands_from_spectra_feed_the_solve(gold):
    """3 columns x 12 bands x 5 levels: solving on Bands.from_spectra equals solving on a Bands made of the same five arrays copied
    through the host, bit for bit -- the layout is the one crt_bands takes."""
    _lib, batched, sp = _mods()
    from crt1d_amd import synth

    d = synth.make_columns(3, 12, 5, seed=3)
    cols = batched.Columns.from_host(d, DEV)
    opt, si = _columns(gold, 3)
    edges = np.linspace(0.4, 2.5, 13)
    b = batched.Bands.from_spectra(gold["parnir_x"], *opt, gold["parnir_xs"], *si, edges)
    assert b.nb == 12 and b.col_stride(3) == 12
    host = {k: getattr(b, k).cpu().numpy().copy() for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")}
    assert all(np.isfinite(v).all() and (v > 0).all() for v in host.values())
    got = batched.solve("2s", cols, b)
    ref = batched.solve("2s", cols, batched.Bands.from_host(host, DEV))
    for k in ref:
        assert same(got[k], ref[k]), k
        assert bool(torch.isfinite(got[k]).all())
