"""CPU: the series form of the spectral normal equations (include/series/crt1d_hip_specfit_series.h) has a header and a symbol table of
its own, the complete set of public headers (directories below include/ walked) is held to the tables, the struct matches the header,
every argument error of the entry is found before any launch (fake device pointers, as tests/test_specfit_cpu.py: a valid call stops at
the workspace check), the order of precedence, the schemes that are not served, the LDS limit behind the workspace check, the workspace query against its terms (each taken from an existing query, never
from the new one), and the Python errors that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("series", "crt1d_hip_specfit_series.h")
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf"]
NOT_SERVED = ["n79", "zq", "4s", "zq_pa"]
NAMES = ["crt_hip_spectral_normal_series_f64", "crt_hip_spectral_normal_series_workspace_bytes"]
KEYS = ["I_dr", "I_df_d", "I_df_u", "F"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_series_entry_points_have_a_table_of_their_own(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.SPECFIT_SERIES_EXPORTS) == sorted(_lib._SPECFIT_SERIES_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS)
    for name in names:
        assert hasattr(lib, name)
        for other in others:
            assert name not in other
    for name, (_, argtypes) in _lib._SPECFIT_SERIES_SIGNATURES.items():  # the argument counts of the table are those of the header
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    # the header reuses the structs of the two it includes: it declares one struct
    assert re.findall(r"typedef struct (\w+)", _header()) == ["crt_spec_series_out"]
    assert '#include "crt1d_hip_specfit.h"' in _header() and '#include "crt1d_hip_sensjac_series.h"' in _header()


def test_every_public_header_is_listed(lib):
    """The complete set of public headers, the directories below include/ walked too (the list of tests/test_specfit_cpu.py covers the files
    that lie directly in include/): every header is held to its table, the tables are disjoint, and the library exports every name.  A header
    added anywhere below include/, or a declaration added to one, fails here until it is listed."""
    from crt1d_amd import _lib

    tables = {"crt1d_hip.h": _lib.EXPORTS, "crt1d_hip_leaf.h": _lib.LEAF_EXPORTS, "crt1d_hip_spectra.h": _lib.SPECTRA_EXPORTS,
              "crt1d_hip_sensor.h": _lib.SENSOR_EXPORTS, "crt1d_hip_jac.h": _lib.JAC_EXPORTS, "crt1d_hip_dlai.h": _lib.DLAI_EXPORTS,
              "crt1d_hip_dleaf.h": _lib.DLEAF_EXPORTS, "crt1d_hip_grad.h": _lib.GRAD_EXPORTS, "crt1d_hip_sensjac.h": _lib.SENSJAC_EXPORTS,
              "crt1d_hip_sensjac_series.h": _lib.SENSJAC_SERIES_EXPORTS, "crt1d_hip_retrieve.h": _lib.RETRIEVE_EXPORTS,
              "crt1d_hip_specfit.h": _lib.SPECFIT_EXPORTS, "series/crt1d_hip_specfit_series.h": _lib.SPECFIT_SERIES_EXPORTS}
    inc = os.path.join(ROOT, "include")
    found = sorted(os.path.relpath(os.path.join(d, f), inc).replace(os.sep, "/") for d, _, files in os.walk(inc) for f in files)
    assert found == sorted(tables)  # (nothing but headers lies there, and every one of them is listed)
    seen = set()
    for header, table in tables.items():
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, header)).read(), flags=re.S)
        assert sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text))) == sorted(table), header
        assert len(set(table)) == len(table) and not seen & set(table), header
        seen |= set(table)
        for name in table:
            assert hasattr(lib, name), name
    assert len(seen) == sum(len(t) for t in tables.values()) and len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_struct_layout():
    from crt1d_amd import _lib

    m = re.search(r"typedef struct crt_spec_series_out \{(.*?)\} crt_spec_series_out;", _header(), re.S)
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("double")
            fields += [re.sub(r"[\s*]", "", n) for n in decl[len("double"):].split(",")]
    S = _lib.CrtSpecSeriesOut
    assert [f[0] for f in S._fields_] == fields == ["A", "g", "c2", "A_t", "g_t", "c2_t"] + ["fwd_" + k for k in KEYS]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [8 * i for i in range(10)] and ctypes.sizeof(S) == 80


def _args(nz=20, nb=8, ncol=2, ntan=2, nt=3):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, None, FAKE, FAKE, FAKE, FAKE, None, None)  # no psi: the series does not read it
    b = _lib.CrtBands(nb, nb, None, None, FAKE, FAKE, FAKE)  # no I_dr0 / I_df0 either
    sun = _lib.CrtSunSeries(nt, FAKE, None, nt * nb, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    dirs = _lib.CrtOpticsDirs(ntan, 0, FAKE, FAKE, FAKE)
    tan = _lib.CrtLeafTangentSeries(FAKE, FAKE, None)
    obs = _lib.CrtSpecObs(None, None, FAKE, None, None, None, FAKE, None)  # I_df_u with weights
    out = _lib.CrtSpecSeriesOut(FAKE, FAKE, FAKE, None, None, None, None, None, None, None)
    return c, b, sun, o, dirs, tan, obs, out


def _call(lib, scheme, c, b, sun, o, levels, dirs, lai, tan, obs, out, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_spectral_normal_series_f64(sid, ref(c), ref(b), ref(sun), ref(o), arr, n, ref(dirs), lai, ref(tan), ref(obs), ref(out), ws,
                                                  wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_series_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, U, SHAPE, nz, nb, nt = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, _lib.CRT_ERR_UNSUPPORTED, _lib.CRT_ERR_SHAPE, 20, 8, 3
    c, b, sun, o, dirs, tan, obs, out = _args(nz, nb, nt=nt)

    def call(c=c, b=b, sun=sun, o=o, levels=(0, nz - 1), dirs=dirs, lai=1, tan=tan, obs=obs, out=out, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, sun, o, None if levels is None else list(levels), dirs, lai, tan, obs, out, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    need = lib.crt_hip_spectral_normal_series_workspace_bytes(_lib.SCHEME_IDS[scheme], 2, nz, nb, nt, 2, 1, 4)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS
    # cols->psi and the incoming spectra of bands are not read: set or not, the call is valid
    assert call(c=_lib.CrtColumns(2, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)) == WS
    # the observations and the outputs, as the per-step entry
    for one in range(4):
        assert call(obs=_lib.CrtSpecObs(*[FAKE if i == one else None for i in range(8)])) == WS
    assert call(obs=None) == BAD
    assert call(obs=_lib.CrtSpecObs(*[None] * 8)) == BAD
    assert call(obs=_lib.CrtSpecObs(None, None, None, None, FAKE, FAKE, FAKE, FAKE)) == BAD  # weights without observations
    assert call(out=None) == BAD
    for hole in range(3):  # NULL A, g, c2
        assert call(out=_lib.CrtSpecSeriesOut(*[None if i == hole else FAKE for i in range(3)], *[None] * 7)) == BAD
    assert call(out=_lib.CrtSpecSeriesOut(*[FAKE] * 10)) == WS  # with the per-step sums and fwd
    assert call(out=_lib.CrtSpecSeriesOut(FAKE, FAKE, FAKE, None, None, None, FAKE, FAKE, FAKE, FAKE)) == WS
    for mask in range(1, 7):  # A_t, g_t, c2_t partly set
        part = [FAKE if mask >> i & 1 else None for i in range(3)]
        assert call(out=_lib.CrtSpecSeriesOut(FAKE, FAKE, FAKE, *part, None, None, None, None)) == BAD, mask
    # the parameter axis
    assert call(lai=0, tan=None) == WS
    assert call(dirs=None, tan=None) == WS
    assert call(dirs=None, lai=0) == WS
    assert call(dirs=None, lai=0, tan=None) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN, 0, FAKE, FAKE, FAKE)) == WS  # npar = 10
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN + 1, 0, FAKE, FAKE, FAKE)) == BAD  # npar = 11
    assert call(dirs=_lib.CrtOpticsDirs(-1, 0, FAKE, FAKE, FAKE)) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(2, 0, None, None, None)) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(2, 2 * nb, FAKE, FAKE, FAKE)) == WS  # per column
    assert call(dirs=_lib.CrtOpticsDirs(2, nb, FAKE, FAKE, FAKE)) == BAD  # col_stride neither 0 nor ntan * nb
    # a tangent must be whole
    assert call(tan=_lib.CrtLeafTangentSeries(None, FAKE, None)) == BAD
    assert call(tan=_lib.CrtLeafTangentSeries(FAKE, None, FAKE)) == BAD
    assert call(tan=_lib.CrtLeafTangentSeries(FAKE, FAKE, FAKE)) == WS
    assert call(tan=_lib.CrtLeafTangentSeries(None, None, None)) == BAD
    # the rest of the parameter-axis parse: without a direction (ntan = 0) neither the stride nor the pointers are looked at; any with_lai
    # but 0 counts as set; sizes that are not positive are an argument error
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None)) == WS
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None), lai=0, tan=None) == BAD
    assert call(dirs=None, lai=2, tan=None) == WS
    assert call(c=_lib.CrtColumns(0, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)) == BAD
    assert call(c=_lib.CrtColumns(2, 0, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), levels=(0,)) == BAD
    for one in range(3):  # any single direction array is enough
        assert call(dirs=_lib.CrtOpticsDirs(2, 0, *[FAKE if i == one else None for i in range(3)])) == WS
    assert call(dirs=_lib.CrtOpticsDirs(0, 0, FAKE, FAKE, FAKE), lai=0, tan=None) == BAD
    # whatever the level series rejects about sun
    assert call(sun=None) == BAD
    assert call(sun=_lib.CrtSunSeries(0, FAKE, None, 0, FAKE, FAKE)) == BAD  # nt < 1
    assert call(sun=_lib.CrtSunSeries(nt, None, None, nt * nb, FAKE, FAKE)) == BAD  # no psi
    assert call(sun=_lib.CrtSunSeries(nt, FAKE, None, nt * nb, None, FAKE)) == BAD
    assert call(sun=_lib.CrtSunSeries(nt, FAKE, None, nt * nb, FAKE, None)) == BAD
    assert call(sun=_lib.CrtSunSeries(nt, FAKE, None, nt * nb - 1, FAKE, FAKE)) == BAD  # a stride below one column's series
    assert call(sun=_lib.CrtSunSeries(nt, FAKE, None, 0, FAKE, FAKE)) == WS  # shared spectra
    assert call(c=_lib.CrtColumns(2, nz, None, FAKE, FAKE, FAKE, FAKE, None, FAKE)) == BAD  # a G table without sun->g_at_psi
    assert call(c=_lib.CrtColumns(2, nz, None, FAKE, FAKE, FAKE, FAKE, None, FAKE), sun=_lib.CrtSunSeries(nt, FAKE, FAKE, 0, FAKE, FAKE)) == WS
    # everything the levels entry rejects
    assert call(c=None) == BAD
    assert call(b=None) == BAD
    assert call(levels=None, nsel=1) == BAD
    assert call(nsel=0) == BAD
    c100 = _args(100, nb)[0]
    assert call(c=c100, levels=range(65)) == BAD
    assert call(levels=(3, 2)) == BAD
    assert call(levels=(nz,)) == BAD
    assert call(scheme=42) == BAD
    assert call(o=_lib.CrtOptions(0.501, 5, 0)) == BAD
    assert call(b=_lib.CrtBands(nb, nb - 1, None, None, FAKE, FAKE, FAKE)) == BAD
    assert call(b=_lib.CrtBands(0, 0, None, None, FAKE, FAKE, FAKE)) == BAD
    assert call(b=_lib.CrtBands(nb, nb, None, None, None, FAKE, FAKE)) == BAD  # no leaf_r
    assert call(b=_lib.CrtBands(nb, nb, None, None, FAKE, FAKE, None)) == (WS if scheme == "bl" else BAD)
    # the order of precedence: an argument error before the shape, the shape before the workspace, the workspace before the LDS limit
    c1 = _args(1, nb)[0]
    assert call(c=c1, levels=(0,)) == SHAPE
    assert call(c=c1, levels=(0,), out=None) == BAD
    assert call(c=c1, levels=(0,), sun=None) == BAD
    assert call(c=c1, levels=(0,), ws=FAKE, wsb=1 << 30) == SHAPE
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == WS
    big = 1 << 30
    two = _lib.CrtSpecObs(None, FAKE, FAKE, None, None, None, None, None)
    assert call(c=c100, levels=range(62), ws=FAKE, wsb=0) == WS  # npar = 4, one key: 310 rows fit
    assert call(c=c100, levels=range(63), ws=FAKE, wsb=0) == WS  # 315 rows do not: found after the workspace check
    assert call(c=c100, levels=range(63), ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(31), obs=two, ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(32), obs=two, ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(63), ws=FAKE, wsb=big, out=None) == BAD  # (an argument error is still one)
    # the rows do not grow with nt: 310 rows of 1000 sun states stop at the workspace check (one byte short), 315 rows at the limit
    many = _lib.CrtSunSeries(1000, FAKE, None, 0, FAKE, FAKE)
    need = lib.crt_hip_spectral_normal_series_workspace_bytes(_lib.SCHEME_IDS[scheme], 2, 100, nb, 1000, 62, 1, 4)
    assert 0 < need < big and call(c=c100, levels=range(62), sun=many, ws=FAKE, wsb=need - 1) == WS
    assert call(c=c100, levels=range(63), sun=many, ws=FAKE, wsb=big) == U


@pytest.mark.parametrize("scheme", NOT_SERVED)
def test_series_schemes_not_served(lib, scheme):
    """n79, zq, 4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors."""
    from crt1d_amd import _lib

    c, b, sun, o, dirs, tan, obs, out = _args()
    U, BAD = _lib.CRT_ERR_UNSUPPORTED, _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, sun, o, [0, 19], dirs, 1, tan, obs, out) == U
    assert _call(lib, scheme, c, b, sun, o, [0, 19], dirs, 1, tan, obs, out, ws=FAKE, wsb=1 << 30) == U
    assert _call(lib, scheme, c, b, sun, o, [19, 0], dirs, 1, tan, obs, out) == BAD  # an argument error is still one
    assert _call(lib, scheme, c, b, None, o, [0, 19], dirs, 1, tan, obs, out) == BAD
    assert _call(lib, scheme, c, b, sun, o, [0, 19], dirs, 1, tan, obs, None) == BAD
    assert _call(lib, scheme, _args(1)[0], b, sun, o, [0], dirs, 1, tan, obs, out) == _lib.CRT_ERR_SHAPE


def _slices(nb, nsel, nkey, npar):
    """Band slices of k_spec_normal: the widest of 256, 128, 64 lanes whose nkey * nsel * (npar + 1) rows fit 160 KB less 4 KB."""
    w = 256
    while w >= 64 and nkey * nsel * (npar + 1) * w * 8 > 160 * 1024 - 4096:
        w //= 2
    w = max(w, 64)  # (none fits: the query sizes 64-lane slices, the call refuses)
    return -(-nb // w)


def test_series_workspace_query(lib):
    """records of the level series + the two side records (the differences tests/test_specfit_cpu.py uses) + [ncol][nt][slices][nent],
    the last term also with one slice."""
    from crt1d_amd import _lib

    q = lib.crt_hip_spectral_normal_series_workspace_bytes
    ncol = 5
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            step = lib.crt_hip_workspace_bytes_nb(sid, ncol, nz, nb)
            lai = lib.crt_hip_levels_dlai_workspace_bytes(sid, ncol, nz, nb, 2) - step
            leaf = lib.crt_hip_levels_dleaf_workspace_bytes(sid, ncol, nz, nb, 2) - step
            for nt in (1, 3, 24):
                rec = lib.crt_hip_levels_series_workspace_bytes(sid, ncol, nz, nt)
                assert rec > 0
                for nsel, nkey, npar in ((1, 1, 5), (2, 1, 1), (2, 4, 5), (9, 2, 5), (16, 1, 10), (64, 4, 10)):
                    part = ncol * nt * _slices(nb, nsel, nkey, npar) * ((npar + 1) * (npar + 2) // 2) * 8
                    assert q(sid, ncol, nz, nb, nt, nsel, nkey, npar) == rec + lai + leaf + part, (scheme, nz, nb, nt, nsel, nkey, npar)
    assert _slices(8, 1, 1, 5) == 1 and _slices(300, 1, 1, 5) == 2 and _slices(300, 9, 2, 5) == 3
    for bad in ((42, 5, 20, 8, 3, 2, 1, 4), (-1, 5, 20, 8, 3, 2, 1, 4), (0, 0, 20, 8, 3, 2, 1, 4), (0, 5, 0, 8, 3, 2, 1, 4), (0, 5, 20, 0, 3, 2, 1, 4),
                (0, 5, 20, 8, 0, 2, 1, 4), (0, 5, 20, 8, -1, 2, 1, 4), (0, 5, 20, 8, 3, 0, 1, 4), (0, 5, 20, 8, 3, 65, 1, 4),
                (0, 5, 20, 8, 3, 2, 0, 4), (0, 5, 20, 8, 3, 2, 5, 4), (0, 5, 20, 8, 3, 2, 1, 0), (0, 5, 20, 8, 3, 2, 1, 11)):
        assert q(*bad) == 0, bad


def test_series_python_errors_need_no_device():
    import numpy as np
    import torch

    from crt1d_amd import batched

    def fake(cls, **attrs):
        """An instance of a device-bound dataclass without its constructor (which wants CUDA tensors): the checks that touch no device
        look at its type and at the shapes given here."""
        x = object.__new__(cls)
        for k, v in attrs.items():
            setattr(x, k, v)
        return x

    ncol, nt, nb = 3, 4, 8
    sun = fake(batched.SunSeries, psi=torch.zeros(ncol, nt, dtype=torch.float64))
    sun32 = fake(batched.SunSeriesF32, psi=sun.psi)
    assert sun.nt == nt
    y = {"I_df_u": np.ones((ncol, nt, 1, nb))}
    tan5 = fake(batched.LeafTangentSeries, dg_at_psi=torch.zeros(ncol, nt + 1))

    class FakeCols:
        ncol, nz, device = 3, 6, "nowhere"

    class F64Bands:
        dtype = torch.float64
        nb = 8

    class F32Bands(F64Bands):
        dtype = torch.float32

    series = [lambda scheme, c, b, s, *a, **kw: batched.SpectralNormalSeriesPlan(scheme, c, b, s, *a, **kw),
              lambda scheme, c, b, s, *a, **kw: batched.spectral_normal_series(scheme, c, b, s, *a, **kw)]
    retrievals = [lambda scheme, c, b, s, *a, **kw: batched.SpectralRetrievalPlan(scheme, c, b, *a, sun=s, **kw),
                  lambda scheme, c, b, s, *a, **kw: batched.retrieve_spectral(scheme, c, b, *a, sun=s, **kw)]
    for make in series + retrievals:
        with pytest.raises(TypeError, match="sun must be a SunSeries"):  # a SunSeriesF32
            make("2s", None, None, sun32, (0,), y, keys=("I_df_u",))
        with pytest.raises(TypeError, match="sun must be a SunSeries"):
            make("2s", None, None, np.ones((ncol, nt)), (0,), y, keys=("I_df_u",))
        for scheme in NOT_SERVED:
            with pytest.raises(ValueError, match="has no spectral retrieval"):
                make(scheme, None, None, sun, (0,), y, keys=("I_df_u",))
        with pytest.raises(ValueError, match="unknown scheme"):
            make("nope", None, None, sun, (0,), y, keys=("I_df_u",))
        with pytest.raises(ValueError, match=r"must be \(ncol, nt, nsel, nb\)"):  # a per-step array: a wrong rank here
            make("2s", None, None, sun, (0,), {"I_df_u": np.ones((ncol, 1, nb))}, keys=("I_df_u",))
        with pytest.raises(ValueError, match=r"must share one shape \(ncol, nt, nsel, nb\)"):
            make("2s", None, None, sun, (0,), y, keys=("I_df_u",), inv_sigma={"I_df_u": np.ones((ncol, nt, 1, nb - 1))})
        with pytest.raises(TypeError, match=r"y must be a dict \{key: \(ncol, nt, nsel, nb\)\}"):
            make("2s", None, None, sun, (0,), np.ones((ncol, nt, 1, nb)), keys=("I_df_u",))
        with pytest.raises(TypeError, match="no f32 storage form"):
            make("2s", None, F32Bands(), sun, (0,), y, keys=("I_df_u",))
        for bad in (np.ones((ncol, nt + 1, 1, nb)), np.ones((ncol, nt, 2, nb)), np.ones((ncol - 1, nt, 1, nb)), np.ones((ncol, nt, 1, nb + 1))):
            with pytest.raises(ValueError, match=r"y\['I_df_u'\] must be \(3, 4, 1, 8\)"):
                make("2s", FakeCols(), F64Bands(), sun, (0,), {"I_df_u": bad}, keys=("I_df_u",))
    for make in series:
        with pytest.raises(ValueError, match="the tangent has nt = 5 sun states, the series 4"):
            make("2s", None, None, sun, (0,), y, keys=("I_df_u",), tangent=tan5)
        with pytest.raises(TypeError, match="tangent must be a LeafTangentSeries"):
            make("2s", None, None, sun, (0,), y, keys=("I_df_u",), tangent=fake(batched.LeafTangent))
        with pytest.raises(ValueError, match="no parameter at all"):
            make("2s", None, None, sun, (0,), y, keys=("I_df_u",), lai=False)
    with pytest.raises(ValueError, match="exceeds 312"):  # the rows do not grow with nt: 1 key, 64 levels, npar = 4
        class Deep(FakeCols):
            nz = 100
        batched.SpectralNormalSeriesPlan("2s", Deep(), F64Bands(), sun, tuple(range(64)), {"I_df_u": np.ones((ncol, nt, 64, nb))}, keys=("I_df_u",),
                                         d_leaf_r=np.ones((3, nb)))
