"""CPU: the plate model of leaf optics (include_ext/crt1d_hip_leafmodel.h; crt1d_amd.leaf_model, tests/leaf_model_reference.py).

1. The entry point exists next to unchanged headers, the struct matches the header, every argument error is found before the launch
   (fake device pointers: no VALID call is made here, it would launch).
2. tav against the values of the specification and against an mpmath quadrature of the Fresnel average.
3. The reference itself: the spot values of the specification, N = 1, energy conservation, and its complex-step partials against
   mpmath on the domain grid -- the reference alone must stay inside the bar the device is held to.
4. The ``leaf_model=`` argument errors of the plans that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import leaf_model_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header(name="crt1d_hip_leafmodel.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include_ext", name)).read(), flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.LEAFMODEL_EXPORTS) == ["crt_hip_plate_leaf_f64"]
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    # include_ext/ holds this header and nothing else (tests/test_specfit_series_cpu.py holds include/ to its complete list, which stays
    # what it was): a header added there fails here until it is listed with a table of its own
    ext = os.path.join(ROOT, "include_ext")
    assert sorted(os.path.relpath(os.path.join(d, f), ext) for d, _, files in os.walk(ext) for f in files) == ["crt1d_hip_leafmodel.h"]
    assert not os.path.exists(os.path.join(ROOT, "include", "crt1d_hip_leafmodel.h"))
    m = re.search(r"crt_hip_plate_leaf_f64\s*\((.*?)\)\s*;", _header(), re.S)
    assert len(m.group(1).split(",")) == len(_lib._LEAFMODEL_SIGNATURES["crt_hip_plate_leaf_f64"][1])
    assert "#define CRT_PLATE_MAX_NABS (CRT_SENSJAC_MAX_NTAN - 1)" in _header() and _lib.PLATE_MAX_NABS == 7
    assert float(re.search(r"#define CRT_PLATE_K_MIN (\S+)", _header()).group(1)) == _lib.PLATE_K_MIN == R.K_MIN
    assert float(re.search(r"#define CRT_PLATE_K_MAX (\S+)", _header()).group(1)) == _lib.PLATE_K_MAX == R.K_MAX
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3  # crt1d_hip.h is what it was


def test_struct_layout():
    from crt1d_amd import _lib

    S = _lib.CrtPlateLeafModel
    m = re.search(r"typedef struct crt_plate_leaf_model \{(.*?)\} crt_plate_leaf_model;", _header(), re.S)
    names = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert [f[0] for f in S._fields_] == names
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 4, 8, 16, 24, 32, 40] and ctypes.sizeof(S) == 48


def test_validation_without_gpu(lib):
    """Every one of these is CRT_ERR_BAD_ARG (the last CRT_ERR_UNSUPPORTED) and launches nothing: the pointers are fake."""
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG

    def call(q=FAKE, q_stride=3, leaf_r=FAKE, leaf_t=FAKE, ntan=3, d_r=FAKE, d_t=FAKE, **kw):
        d = dict(ncol=3, nb=8, nabs=2, kspec=FAKE, t_alpha=FAKE, t_90=FAKE, n=FAKE)
        d.update(kw)
        m = _lib.CrtPlateLeafModel(*[d[f[0]] for f in _lib.CrtPlateLeafModel._fields_])
        return lib.crt_hip_plate_leaf_f64(ctypes.byref(m), q, q_stride, leaf_r, leaf_t, ntan, d_r, d_t, None)

    assert lib.crt_hip_plate_leaf_f64(None, FAKE, 3, FAKE, FAKE, 3, FAKE, FAKE, None) == BAD
    for kw in (dict(ncol=0), dict(nb=0), dict(nabs=0), dict(nabs=8), dict(kspec=None), dict(t_alpha=None), dict(t_90=None), dict(n=None),
               dict(q=None), dict(leaf_r=None), dict(leaf_t=None), dict(q_stride=2), dict(d_r=None), dict(d_t=None), dict(ntan=2),
               dict(ntan=_lib.SENSJAC_MAX_NTAN + 1), dict(nabs=7, q_stride=7), dict(nabs=7, q_stride=8, ntan=7)):
        assert call(**kw) == BAD, kw
    assert call(nb=65535 * 64 + 1) == _lib.CRT_ERR_UNSUPPORTED


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def test_tav_spot_values():
    from crt1d_amd.leaf_model import tav

    for f in (tav, R.tav):
        assert abs(float(f(90.0, 1.5)) - 0.90822204066) < 1e-10
        assert abs(float(f(40.0, 1.5)) - 0.95842403571) < 1e-10
        assert abs(float(f(0.5, 1.5)) - 0.96) < 1e-10  # the normal-incidence value 4 n / (n + 1)^2
    n = np.linspace(1.3, 1.6, 7)
    assert np.abs(tav(40.0, n) - R.tav(40.0, n)).max() < 1e-14 and np.abs(tav(90.0, n) - R.tav(90.0, n)).max() < 1e-14  # (two orders of the same sum)
    with pytest.raises(ValueError):
        tav(0.0, 1.5)
    with pytest.raises(ValueError):
        tav(40.0, 1.0)


@pytest.mark.parametrize("n", [1.3, 1.45, 1.6])
def test_tav_is_the_fresnel_average(n):
    """tav(alpha, n) = (2 / sin^2 alpha) int_0^alpha T(theta) sin theta cos theta d theta with T the unpolarised Fresnel transmittance
    of the interface, by mpmath.quad at 30 digits, to 1e-12."""
    import mpmath

    from crt1d_amd.leaf_model import tav

    with mpmath.workdps(30):
        nn = mpmath.mpf(n)

        def T(th):
            c, s2 = mpmath.cos(th), mpmath.sin(th) ** 2
            g = mpmath.sqrt(nn * nn - s2)
            return 1 - (((c - g) / (c + g)) ** 2 + ((nn * nn * c - g) / (nn * nn * c + g)) ** 2) / 2

        for alpha in (40.0, 90.0):
            a = mpmath.radians(alpha)
            avg = 2 * mpmath.quad(lambda th: T(th) * mpmath.sin(th) * mpmath.cos(th), [0, a / 2, a]) / mpmath.sin(a) ** 2
            assert abs(float(avg) - float(tav(alpha, n))) < 1e-12, (alpha, float(avg), float(tav(alpha, n)))


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_reference_spot_values():
    n = 1.45
    ta, t9 = R.tav(40.0, n), R.tav(90.0, n)
    for (N, k), want in (((1.5, 0.01), (0.458351, 0.479601)), ((1.5, 1.0), (0.047526, 0.028030))):
        got = R.plate(N, k, n, ta, t9)
        assert abs(got[0] - want[0]) < 5e-7 and abs(got[1] - want[1]) < 5e-7, (N, k, got)
    Ra, Ta = R.top_plate(0.05, n, ta, t9)[:2]
    assert abs(Ra - 0.301894) < 5e-7 and abs(Ta - 0.519262) < 5e-7
    got = R.plate(1.0, 0.05, n, ta, t9)  # N = 1: no inner plate
    assert abs(got[0] - Ra) < 1e-15 and abs(got[1] - Ta) < 1e-15


def test_reference_conserves_energy():
    q, K, n = R.domain_grid()
    ref = R.reference(q, K, n)
    tot = ref["leaf_r"] + ref["leaf_t"]
    assert np.all(tot < 1.0) and np.all(ref["leaf_r"] > 0.0) and np.all(ref["leaf_t"] > 0.0)
    ta, t9 = R.tav(40.0, n), R.tav(90.0, n)
    last = None
    for k in (1e-2, 1e-4, 1e-6):  # leaf_r + leaf_t -> 1 as k -> 0, from below
        r, t = R.plate(2.0, k, n, ta, t9)
        gap = 1.0 - (r + t)
        assert np.all(gap > 0.0) and (last is None or np.all(gap < 0.02 * last))
        last = gap
    assert np.all(last < 1e-4)


def test_reference_complex_step_against_mpmath():
    """On the domain grid the complex128 partials lie within 1e-11 of the scale (the largest magnitude of that parameter's leaf_r /
    leaf_t partial over the column) of the mpmath ones, and the values within 1e-13.  Measured: 2.1e-12 at worst, at k = 1e-4."""
    q, K, n = R.domain_grid()
    ref = R.reference(q, K, n)
    assert ref["k"].min() == pytest.approx(1e-4) and ref["k"].max() <= 50.0
    scale = np.abs(np.stack([ref["d_leaf_r"], ref["d_leaf_t"]])).max(axis=(0, 3))
    worst = max(float((ref[s] / scale[:, :, None]).max()) for s in ("spread_r", "spread_t"))
    print(f"complex step against mpmath: {worst:.2e} of scale")
    assert worst < 1e-11
    assert np.abs(ref["cs_leaf_r"] - ref["leaf_r"]).max() < 1e-13 and np.abs(ref["cs_leaf_t"] - ref["leaf_t"]).max() < 1e-13


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def test_model_object():
    from crt1d_amd.leaf_model import PlateLeafModel

    K, n = np.ones((2, 5)), np.full(5, 1.4)
    m = PlateLeafModel(K, n, names=("cab", "cw"))
    assert m.params == ("N", "cab", "cw") and (m.nm, m.nabs, m.nb, m.alpha) == (3, 2, 5, 40.0)
    assert PlateLeafModel(K, n).params == ("N", "C0", "C1")
    assert np.abs(m.t_alpha - R.tav(40.0, n)).max() < 1e-14 and np.abs(m.t_90 - R.tav(90.0, n)).max() < 1e-14
    for bad in (dict(kspec=np.ones((8, 5))), dict(kspec=-K), dict(kspec=np.ones((2, 4))), dict(names=("a",)), dict(names=("N", "a")),
                dict(n=np.full(5, 0.9))):
        kw = dict(kspec=K, n=n)
        kw.update(bad)
        with pytest.raises(ValueError):
            PlateLeafModel(kw.pop("kspec"), kw.pop("n"), **kw)


def test_plan_errors_need_no_device():
    from crt1d_amd import batched
    from crt1d_amd.leaf_model import PlateLeafModel

    model = PlateLeafModel(np.ones((2, 8)), np.full(8, 1.4))  # nm = 3
    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    ys = {"I_df_u": np.ones((1, 1, 1))}
    yb = {"I_df_u": np.ones((1, 1, 8))}
    lo, hi = np.array([1.0, 0.0, 0.0, -1.0]), np.array([4.0, 9.0, 9.0, 1.0])  # N, C0, C1, lai
    p0 = np.array([1.5, 1.0, 1.0, 0.0])
    makers = [lambda **kw: batched.RetrievalPlan("2s", None, None, (0,), sens, ys, keys=("I_df_u",), **kw),
              lambda **kw: batched.retrieve("2s", None, None, (0,), sens, ys, keys=("I_df_u",), **kw),
              lambda **kw: batched.SpectralRetrievalPlan("2s", None, None, (0,), yb, keys=("I_df_u",), **kw)]
    for make in makers:
        with pytest.raises(TypeError, match="leaf_model must be a PlateLeafModel"):
            make(leaf_model="prospect", lo=lo, hi=hi, p0=p0)
        for d in ("d_leaf_r", "d_leaf_t"):
            with pytest.raises(ValueError, match="exclude each other"):
                make(leaf_model=model, lo=lo, hi=hi, p0=p0, **{d: np.ones((1, 8))})
        with pytest.raises(ValueError, match="one call takes 8"):
            make(leaf_model=model, lo=lo, hi=hi, p0=p0, d_soil_r=np.ones((6, 8)))
        with pytest.raises(ValueError, match=r"must be \(npar,\) = \(4,\)"):
            make(leaf_model=model, lo=lo[:3], hi=hi, p0=p0)
    for make in makers[:2] + [lambda **kw: batched.SpectralRetrievalPlan("2s", _Cols, _Bands, (0,), yb, keys=("I_df_u",), **kw),
                              lambda **kw: batched.retrieve_spectral("2s", _Cols, _Bands, (0,), yb, keys=("I_df_u",), **kw)]:
        with pytest.raises(ValueError, match="needs lo and hi"):
            make(leaf_model=model, p0=p0)
        with pytest.raises(ValueError, match="needs lo and hi"):
            make(leaf_model=model, lo=lo, p0=p0)
        for k, v in ((0, 0.5), (1, -1e-3), (2, -1.0)):
            bad = lo.copy()
            bad[k] = v
            with pytest.raises(ValueError, match="lo and hi must keep"):
                make(leaf_model=model, lo=bad, hi=hi, p0=p0)
        bad = hi.copy()
        bad[0] = 4.5
        with pytest.raises(ValueError, match=r"keep N inside \[1, 4\]"):
            make(leaf_model=model, lo=lo, hi=bad, p0=p0)
        with pytest.raises(ValueError, match="needs p0"):
            make(leaf_model=model, lo=lo, hi=hi)


class _Cols:  # (what the spectral plans look at before they touch a device: the shapes)
    ncol, nz = 1, 4


class _Bands:
    import torch

    nb, dtype = 8, torch.float64
