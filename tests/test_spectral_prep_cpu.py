"""CPU: spectral inputs on the device (include/crt1d_hip_spectra.h) -- symbols and binding, argument errors before any launch, the
host-side sub-bin counts against the reference's, the fixed Gauss-Legendre rule of the Planck weight against QUADPACK, and a sequential
NumPy restatement of ``k_spectral_prep`` against the reference's outputs (the GPU tests use it for shapes the fixture does not hold).

Planck rule: relative error of the ``CRT_SPECTRA_NGL`` = 16-point rule against the fixture's ``l_wl_planck_integ`` over every sub-bin
of every edge set, both ``x_smear_nb`` modes, at 6000 K and 3000 K: worst 1.4e-15, the rounding floor (12 points: 1.1e-15); the bar is
1e-13.  The widest sub-bin of the fixture is 0.43 of its centre wavelength ("nx2": 0.9 .. 1.4 um), where an 8-point rule is left with
3.0e-14 -- three times under the bar, no margin for a wider sub-bin or a lower temperature -- so 16 points were chosen.

Restatement against the reference: worst relative error 2.1e-15 over all cases (bar 1e-12, tests/test_gpu_spectral_prep.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHTS = ("uniform", "planck6000", "planck3000", "table")
MODES = (("d", None), ("7", 7))
PLANCK_BAR = 1e-13
PARITY_BAR = 1e-12


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return load_golden("g12_spectral_prep")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_new_symbols_are_exported_and_bound(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_spectra.h")
    assert names == sorted(_lib.SPECTRA_EXPORTS) == ["crt_hip_avg_optical_prop_f64", "crt_hip_bands_from_spectra_f64", "crt_hip_planck_nodes_f64"]
    for n in names:
        f = getattr(lib, n)
        assert f.restype is ctypes.c_int and f.argtypes is not None, n
    assert len(lib.crt_hip_avg_optical_prop_f64.argtypes) == 17 and len(lib.crt_hip_bands_from_spectra_f64.argtypes) == 26
    # the main header, its binding table and the ABI version are what they were
    assert len(_declared("crt1d_hip.h")) == 57 == len(_lib.EXPORTS)
    assert not set(_lib.SPECTRA_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.LEAF_EXPORTS))
    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3
    text = open(os.path.join(ROOT, "include", "crt1d_hip_spectra.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"CRT_LIGHT_(\w+) = (\d+)", text)}
    assert enum == {"UNIFORM": _lib.LIGHT_UNIFORM, "PLANCK": _lib.LIGHT_PLANCK, "TABLE": _lib.LIGHT_TABLE}
    assert enum == {k.upper(): v for k, v in _lib.LIGHT_KINDS.items()}
    for macro, val in (("NGL", _lib.SPECTRA_NGL), ("MAX_NB", _lib.SPECTRA_MAX_NB), ("MAX_ITEMS", _lib.SPECTRA_MAX_ITEMS), ("BLOCK", _lib.SPECTRA_BLOCK)):
        assert int(re.search(rf"#define CRT_SPECTRA_{macro} (\d+)", text).group(1)) == val, macro
    assert _lib.SPECTRA_LDS_BYTES == 160 * 1024 and "#define CRT_SPECTRA_LDS_BYTES (160 * 1024)" in text


def _offsets(counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return off, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_argument_errors_before_any_launch(lib):
    """Fake device pointers: every call below must return before it touches them (no GPU here, nothing to launch on).  ``sub_off`` is
    the one host pointer, and real."""
    from crt1d_amd import _lib

    fake = 0x1000
    good, good_p = _offsets([3, 1, 2, 5])
    T = _lib.LIGHT_TABLE
    ok = dict(x=fake, nx=9, y=fake, nspec=4, edges=fake, nb=4, sub_off=good_p, kind=_lib.LIGHT_PLANCK, T_K=6000.0, lx=fake, nlx=5, ly=fake,
              nlight=2, group=2, out=fake, y_sub=fake)

    def avg(**kw):
        a = {**ok, **kw}
        return lib.crt_hip_avg_optical_prop_f64(a["x"], a["nx"], a["y"], a["nspec"], a["edges"], a["nb"], a["sub_off"], a["kind"], a["T_K"], a["lx"],
                                                a["nlx"], a["ly"], a["nlight"], a["group"], a["out"], a["y_sub"], None)

    okb = dict(x=fake, nx=9, lr=fake, lrs=9, lt=fake, lts=0, sr=fake, srs=9, xs=fake, nxs=4, dr=fake, drs=4, df=fake, dfs=0, ncol=4, edges=fake, nb=4,
               sub_off=good_p, kind=T, T_K=6000.0, o0=fake, o1=fake, o2=fake, o3=fake, o4=fake)

    def bands(**kw):
        a = {**okb, **kw}
        return lib.crt_hip_bands_from_spectra_f64(a["x"], a["nx"], a["lr"], a["lrs"], a["lt"], a["lts"], a["sr"], a["srs"], a["xs"], a["nxs"], a["dr"],
                                                  a["drs"], a["df"], a["dfs"], a["ncol"], a["edges"], a["nb"], a["sub_off"], a["kind"], a["T_K"],
                                                  a["o0"], a["o1"], a["o2"], a["o3"], a["o4"], None)

    first_nonzero = _offsets([3, 1, 2, 5])
    first_nonzero[0][0] = 1
    flat = _offsets([3, 0, 2, 5])       # a band without sub-bins
    falling = _offsets([3, 4, -2, 5])
    shared_bad = [dict(nx=1), dict(nb=-1), dict(edges=None), dict(sub_off=None), dict(sub_off=first_nonzero[1]), dict(sub_off=flat[1]),
                  dict(sub_off=falling[1]), dict(kind=3), dict(kind=-1), dict(kind=_lib.LIGHT_PLANCK, T_K=0.0), dict(kind=_lib.LIGHT_PLANCK, T_K=-5.0),
                  dict(kind=_lib.LIGHT_PLANCK, T_K=float("nan"))]
    for bad in shared_bad + [dict(x=None), dict(y=None), dict(out=None), dict(nspec=-1), dict(kind=T, lx=None), dict(kind=T, ly=None),
                             dict(kind=T, nlx=0), dict(kind=T, nlight=0), dict(kind=T, group=0), dict(kind=T, group=1)]:  # (group 1: 4 rows needed, 2 given)
        assert avg(**bad) == _lib.CRT_ERR_BAD_ARG, bad
    for bad in shared_bad + [dict(x=None), dict(lr=None), dict(lt=None), dict(sr=None), dict(xs=None), dict(dr=None), dict(df=None), dict(o0=None),
                             dict(o1=None), dict(o2=None), dict(o3=None), dict(o4=None), dict(ncol=-1), dict(nxs=1), dict(lrs=8), dict(lts=-9),
                             dict(srs=1), dict(drs=3), dict(dfs=2)]:
        assert bands(**bad) == _lib.CRT_ERR_BAD_ARG, bad
    # nothing to do
    assert avg(nspec=0) == avg(nb=0) == avg(nspec=0, kind=T) == _lib.CRT_OK
    assert avg(nspec=0, y_sub=None, kind=_lib.LIGHT_UNIFORM, lx=None, ly=None, nlx=0, nlight=0, group=0) == _lib.CRT_OK
    assert bands(ncol=0) == bands(nb=0) == _lib.CRT_OK
    # over the limits: too many bands, too many sub-bins, more than one workgroup's LDS
    many = _offsets(np.ones(_lib.SPECTRA_MAX_NB + 1, dtype=np.int64))
    assert avg(nb=_lib.SPECTRA_MAX_NB + 1, sub_off=many[1]) == bands(nb=_lib.SPECTRA_MAX_NB + 1, sub_off=many[1]) == _lib.CRT_ERR_UNSUPPORTED
    long_ = _offsets([_lib.SPECTRA_MAX_ITEMS - 2, 3])
    assert avg(nb=2, sub_off=long_[1]) == bands(nb=2, sub_off=long_[1]) == _lib.CRT_ERR_UNSUPPORTED
    assert avg(nx=10000) == bands(nx=4800, lrs=4800, srs=4800) == bands(nxs=7000, drs=7000) == _lib.CRT_ERR_UNSUPPORTED
    assert avg(kind=T, nlx=10000) == _lib.CRT_ERR_UNSUPPORTED
    # the node query
    assert lib.crt_hip_planck_nodes_f64(None, None) == _lib.CRT_ERR_BAD_ARG


def test_sub_bin_counts_equal_the_reference(gold):
    from crt1d_amd import spectra as sp

    for c in gold["cases"]:
        x, edges = gold[f"{c}_x"], gold[f"{c}_edges"]
        got = sp.sub_bin_counts(x, edges)
        assert got.dtype == np.int64 and np.array_equal(got, gold[f"{c}_nsub"]), c
        assert np.array_equal(sp.sub_bin_counts(x, edges, 7), np.full(edges.size - 1, 7))
    assert np.array_equal(gold["parnir_edges"], [0.4, 0.7, 2.5])
    assert sp.sub_bin_counts(gold["parnir_x"], gold["parnir_edges"])[0] == gold["parnir_nsub"][0]  # the PAR band: (0.7 - 0.4) / 0.005
    assert gold["odd_nsub"][0] == 1  # a band narrower than one sub-bin
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            sp.sub_bin_counts(gold["parnir_x"], gold["parnir_edges"], bad)


# ---- the kernel restated in NumPy, sequentially --------------------------------------------------------------------------------------
def planck(T_K, wl_um):
    h, c, k_B = 6.62607015e-34, 299792458.0, 1.380649e-23
    wl = wl_um * 1e-6
    return (2 * h * c * c) / (wl * wl * wl * wl * wl * (np.exp(h * c / (wl * k_B * T_K)) - 1.0))


def rule_planck(T_K, lo, hi, nodes):
    """int l_wl_planck over [lo, hi] (arrays) by the device's rule."""
    gx, gw = nodes
    acc = np.zeros_like(lo)
    for xi, wi in zip(gx, gw):
        acc = acc + wi * planck(T_K, lo + (hi - lo) * xi)
    return (hi - lo) * acc


def smear_1(x, ys, xl, xu):
    """``_smear_tuv_1`` of the rows of ``ys`` (k_smear_tuv's walk)."""
    area = np.zeros(len(ys))
    k = max(int(np.searchsorted(x[1:], xl, side="left")), 0)
    while k < x.size - 1 and not x[k] > xu:
        a1, a2 = max(x[k], xl), min(x[k + 1], xu)
        slope = (ys[:, k + 1] - ys[:, k]) / (x[k + 1] - x[k])
        area = area + (a2 - a1) * ((ys[:, k] + slope * (a2 - x[k])) + (ys[:, k] + slope * (a1 - x[k]))) / 2
        k += 1
    return area / (xu - xl)


def sub_edges(edges, counts):
    lo, hi = [], []
    for b0, b1, n in zip(edges[:-1], edges[1:], counts):
        step = (b1 - b0) / n
        xe = np.arange(n + 1) * step + b0
        xe[-1] = b1
        lo.append(xe[:-1]), hi.append(xe[1:])
    return np.concatenate(lo), np.concatenate(hi)


def restate(x, ys, edges, counts, light, T_K=None, table=None, nodes=None):
    """(out (nprop, nb), y_sub (nprop, nitem)): sums in ascending sub-bin order, as the kernel forms them."""
    lo, hi = sub_edges(edges, counts)
    with np.errstate(invalid="ignore", divide="ignore"):
        y_sub = np.stack([smear_1(x, ys, a, b) for a, b in zip(lo, hi)], axis=1)
        if light == "uniform":
            lw = np.ones_like(lo)
        elif light == "planck":
            lw = rule_planck(T_K, lo, hi, nodes)
        else:
            lw = np.interp((lo + hi) / 2, table[0], table[1])
        w = (hi - lo) * lw
        out = np.empty((len(ys), len(counts)))
        off = np.concatenate([[0], np.cumsum(counts)])
        for b in range(len(counts)):
            num, den = np.zeros(len(ys)), 0.0
            for s in range(off[b], off[b + 1]):
                num, den = num + y_sub[:, s] * w[s], den + w[s]
            out[:, b] = num / den
    return out, y_sub


def light_args(light, g, c, nodes):
    if light.startswith("planck"):
        return dict(light="planck", T_K=float(light[6:]), nodes=nodes)
    if light == "table":
        return dict(light="table", table=(g[f"{c}_xs"], g[f"{c}_si"][0] + g[f"{c}_si"][1]))
    return dict(light="uniform")


def rel_err(got, ref):
    """Largest relative error over the finite elements of ``ref``; NaN must sit where the reference's NaN sits."""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    ok = np.isfinite(ref)
    den = np.where(ref[ok] == 0, 1.0, np.abs(ref[ok]))
    return float(np.max(np.abs(got[ok] - ref[ok]) / den)) if ok.any() else 0.0


def test_gauss_legendre_nodes(lib):
    from numpy.polynomial.legendre import leggauss

    from crt1d_amd import _lib

    x, w = _lib.planck_nodes()
    gx, gw = leggauss(_lib.SPECTRA_NGL)
    assert x.shape == w.shape == (_lib.SPECTRA_NGL,)
    np.testing.assert_allclose(x, (gx + 1) / 2, rtol=0, atol=2e-16)
    np.testing.assert_allclose(w, gw / 2, rtol=0, atol=4e-15)
    assert abs(w.sum() - 1.0) < 2e-15 and np.all(w > 0) and np.all(np.diff(x) > 0)


def test_planck_rule_meets_the_bar_against_quadpack(lib, gold):
    from crt1d_amd import _lib

    nodes = _lib.planck_nodes()
    worst, widest = 0.0, 0.0
    for c in gold["cases"]:
        for m, _ in MODES:
            lo, hi = gold[f"{c}_sub_{m}"]
            widest = max(widest, float(np.max((hi - lo) / (0.5 * (hi + lo)))))
            for T, ref in zip((6000.0, 3000.0), gold[f"{c}_planck_{m}"]):
                err = np.abs(rule_planck(T, lo, hi, nodes) - ref) / ref
                worst = max(worst, float(err.max()))
                assert err.max() <= PLANCK_BAR, (c, m, T, err.max(), lo[err.argmax()], hi[err.argmax()])
    print(f"worst relative error of the {_lib.SPECTRA_NGL}-point rule: {worst:.2e}; widest sub-bin / centre: {widest:.3f}")
    assert 0.43 <= widest <= 0.44  # the range the header states


def test_restatement_equals_the_reference(lib, gold):
    """The fixture is sound (NaN only where an edge set leaves the data on purpose) and the sequential restatement of the kernel is
    within the parity bar of the reference on every case."""
    from crt1d_amd import _lib

    nodes = _lib.planck_nodes()
    worst = 0.0
    for c in gold["cases"]:
        x, ys, edges = gold[f"{c}_x"], gold[f"{c}_y"], gold[f"{c}_edges"]
        for m, nbm in MODES:
            counts = np.full(edges.size - 1, nbm) if nbm else gold[f"{c}_nsub"]
            lo, hi = sub_edges(edges, counts)
            assert np.array_equal(np.stack([lo, hi]), gold[f"{c}_sub_{m}"]), c  # linspace, restated
            for light in LIGHTS:
                ref = gold[f"{c}_{light}_{m}"]
                if c not in gold["nan_cases"]:
                    assert np.isfinite(ref).all(), (c, light, m)
                got, _ = restate(x, ys, edges, counts, **light_args(light, gold, c, nodes))
                worst = max(worst, rel_err(got, ref))
        si = gold[f"{c}_si"]
        got_I = np.stack([[smear_1(gold[f"{c}_xs"], si[q:q + 1], a, b)[0] * (b - a) for a, b in zip(edges[:-1], edges[1:])] for q in range(2)])
        worst = max(worst, rel_err(got_I, gold[f"{c}_I"]))
    assert np.isnan(gold["nx9_table_d"]).any() and np.isfinite(gold["nx9_uniform_d"]).all()
    print(f"worst relative error of the restatement against the reference: {worst:.2e}")
    assert worst <= PARITY_BAR


def test_python_entry_points_refuse_what_the_device_cannot_do():
    import torch

    from crt1d_amd import batched
    from crt1d_amd import spectra as sp

    x = np.linspace(0.4, 2.5, 30)
    y = np.full(30, 0.2)
    with pytest.raises(NotImplementedError, match="callable"):
        sp.smear_avg_optical_prop(x, y, np.array([0.4, 0.7]), light=lambda xm: np.ones_like(xm))
    with pytest.raises(NotImplementedError, match="callable"):
        sp.avg_optical_prop(y, (0.4, 0.7), x=x, light=np.ones(60))  # per-bin weights: cannot be sent either
    with pytest.raises(NotImplementedError, match="xe="):
        sp.avg_optical_prop(y[:-1], (0.4, 0.7), xe=x)
    with pytest.raises(ValueError):
        sp.avg_optical_prop(y, (0.4, 0.7), x=x, xe=x)
    with pytest.raises(ValueError):
        sp.avg_optical_prop(y, (0.4, 0.7))
    with pytest.raises(ValueError, match="light"):
        sp.smear_avg_optical_prop(x, y, np.array([0.4, 0.7]), light="sun")
    # Bands.from_spectra: the house checks, in the order type, dtype, shape, device -- none of them needs a GPU
    t = lambda n, dtype=torch.float64: torch.full((2, n), 0.3, dtype=dtype)  # noqa: E731
    xs, edges = np.linspace(0.3, 4.0, 12), np.array([0.4, 0.7, 2.5])
    good = [x, t(30), t(30), t(30), xs, t(12), t(12), edges]
    for pos, bad, exc in ((1, y, TypeError), (2, t(30, torch.float32), TypeError), (3, t(29), ValueError), (5, t(30), ValueError),
                          (6, torch.zeros((2, 2, 12), dtype=torch.float64), ValueError), (1, t(30), ValueError)):  # (last: a CPU tensor)
        a = list(good)
        a[pos] = bad
        with pytest.raises(exc):
            batched.Bands.from_spectra(*a)
    with pytest.raises(ValueError, match="light"):
        batched.Bands.from_spectra(*good, light="moon")
