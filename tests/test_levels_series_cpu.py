"""CPU: the sun-angle series of level spectra (crt_hip_levels_series_f64 / _f32) -- symbols, struct layout, the workspace query, every
argument error (each found before any launch, so no device is needed) and the Python boundary's shape / dtype / device checks."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ["2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa"]
NAMES = ("crt_hip_levels_series_workspace_bytes", "crt_hip_levels_series_f64", "crt_hip_levels_series_f32")


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_symbols_exported_and_declared(lib):
    from crt1d_amd import _lib

    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert "#define CRT_ABI_VERSION 3" in text and lib.crt_hip_abi_version() == 3  # symbols were added, nothing changed


def test_sun_series_f32_layout_matches_header(lib):
    from crt1d_amd import _lib

    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    body = text[text.index("typedef struct crt_sun_series_f32 {"):text.index("} crt_sun_series_f32;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|int64_t|const double\*|const float\*)\s+(\w+);", body)
    assert [f[1] for f in fields] == [f[0] for f in _lib.CrtSunSeriesF32._fields_]
    assert [f[0] for f in fields] == ["int32_t", "const double*", "const double*", "int64_t", "const float*", "const float*"]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const double*": ctypes.c_void_p, "const float*": ctypes.c_void_p}
    assert [ctype[f[0]] for f in fields] == [f[1] for f in _lib.CrtSunSeriesF32._fields_]
    # the layout of crt_sun_series: the f32 entry reads it through the same offsets
    assert ctypes.sizeof(_lib.CrtSunSeriesF32) == ctypes.sizeof(_lib.CrtSunSeries) == 8 + 5 * 8
    for f, _ in _lib.CrtSunSeries._fields_:
        assert getattr(_lib.CrtSunSeriesF32, f).offset == getattr(_lib.CrtSunSeries, f).offset, f


def test_workspace_bytes(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_levels_series_workspace_bytes
    for scheme, sid in _lib.SCHEME_IDS.items():
        for ncol, nz in ((1, 5), (10, 60), (7, 100), (3, 130)):
            prev = 0
            for nt in (1, 2, 3, 24, 1000, 70000):
                n = q(sid, ncol, nz, nt)
                assert n > prev, (scheme, ncol, nz, nt)  # monotone in nt
                prev = n
                # no nb in the query: records only, never more than the integrated series asks for at any nb
                for nb in (1, 12, 2151):
                    assert n <= lib.crt_hip_series_workspace_bytes(sid, ncol, nz, nb, nt), (scheme, ncol, nz, nb, nt)
            # exactly [ncol] canopy records + [ncol][nt] sun records: linear in nt
            assert q(sid, ncol, nz, 3) - q(sid, ncol, nz, 2) == q(sid, ncol, nz, 2) - q(sid, ncol, nz, 1)
            assert q(sid, ncol, nz, 1) % 8 == 0
        assert q(sid, 4, 10, 0) == 0 and q(sid, 4, 10, -1) == 0
        assert q(sid, 0, 10, 3) == 0 and q(sid, -2, 10, 3) == 0
        assert q(sid, 4, 0, 3) == 0
    assert q(99, 4, 10, 3) == 0 and q(-1, 4, 10, 3) == 0
    assert len(q.argtypes) == 4  # (scheme, ncol, nz, nt)


class _Call:
    """A well-formed call with fake (never dereferenced) device pointers; tests break one argument at a time."""

    P = 0x10000  # any non-NULL value: every check below happens on the host, before a launch

    def __init__(self, lib, scheme="2s", suffix="f64", ncol=3, nz=7, nb=5, nt=4, levels=(0, 6)):
        from crt1d_amd import _lib

        self._lib, self.lib, self.sid = _lib, lib, _lib.SCHEME_IDS[scheme]
        P = self.P
        self.fn = getattr(lib, f"crt_hip_levels_series_{suffix}")
        self.cols = _lib.CrtColumns(ncol, nz, None, P, P, P, P, None, None)
        self.bands = _lib.CrtBands(nb, nb, None, None, P, P, P)
        self.sun = (_lib.CrtSunSeriesF32 if suffix == "f32" else _lib.CrtSunSeries)(nt, P, None, nt * nb, P, P)
        self.opts = _lib.CrtOptions(0.501, 0, 0)
        self.out = _lib.CrtOutputs(P, P, P, P, None, None, None)
        self.levels = list(levels)
        self.nsel = None
        self.ws = P
        self.ws_bytes = lib.crt_hip_levels_series_workspace_bytes(self.sid, ncol, nz, nt)

    def __call__(self, sun="own", opts="own", levels="own"):
        r = lambda x, own: None if x is None else ctypes.byref(own if isinstance(x, str) else x)  # noqa: E731
        lev = (ctypes.c_int32 * max(len(self.levels), 1))(*self.levels)
        nsel = len(self.levels) if self.nsel is None else self.nsel
        return self.fn(self.sid, ctypes.byref(self.cols), ctypes.byref(self.bands), r(sun, self.sun), r(opts, self.opts),
                       None if levels is None else lev, nsel, ctypes.byref(self.out), self.ws, self.ws_bytes, None)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bad_arguments(lib, scheme, suffix):
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG
    new = lambda **kw: _Call(lib, scheme, suffix, **kw)  # noqa: E731
    # what the integrated series rejects
    assert new()(sun=None) == BAD
    for field in ("psi", "I_dr0", "I_df0"):
        c = new()
        setattr(c.sun, field, None)
        assert c() == BAD, field
    for nt in (0, -3):
        c = new()
        c.sun.nt = nt
        assert c() == BAD
    for stride in (1, 4 * 5 - 1, -20):
        c = new()
        c.sun.col_stride = stride
        assert c() == BAD, stride
    c = new()
    c.cols.g_table = c.P  # a table, but no per-step G(psi)
    assert c() == BAD
    # what the level-subset solve rejects
    assert new()(levels=None) == BAD
    for bad in ((), (-1,), (7,), (3, 3), (4, 2), (0, 6, 6), tuple(range(7)) + (100,)):
        assert new(levels=bad)() == BAD, bad
    c = new()
    c.nsel = 0
    assert c() == BAD
    c = new(nz=200, levels=tuple(range(_lib.MAX_LEVEL_SELECT + 1)))
    assert c() == BAD
    c = new()
    c.out = _lib.CrtOutputs(None, None, None, None, None, None, None)  # nothing asked for
    assert c() == BAD
    for extra in ("x0", "x1", "x2"):
        c = new()
        setattr(c.out, extra, c.P)
        assert c() == BAD, extra
    # ... and the common ones
    for field in ("lai", "g_kind"):
        c = new()
        setattr(c.cols, field, None)
        assert c() == BAD, field
    for field in ("leaf_r", "leaf_t"):
        c = new()
        setattr(c.bands, field, None)
        assert c() == BAD, field
    c = new()
    c.bands.col_stride = 3
    assert c() == BAD
    c = new()
    c.opts.tau_d_method = 7
    assert c() == BAD
    c = new()
    c.opts.tune[_lib.NTUNE - 2] = 1  # reserved key
    assert c() == BAD
    c = new()
    c.opts.tune[8] = 9  # CRT_TUNE_TRI_M takes 8 / 12 / 16
    assert c() == BAD
    if scheme == "2s":
        c = new()
        c.cols.mla = None
        assert c() == BAD
    if scheme == "4s":
        c = new()
        c.opts.mu_s = 1.5
        assert c() == BAD
    if scheme != "bl":
        c = new()
        c.bands.soil_r = None
        assert c() == BAD
    assert new().fn(99, None, None, None, None, None, 1, None, None, 0, None) == BAD
    # a subset of the outputs is fine up to the workspace check (which comes after every argument check)
    c = new()
    c.out = _lib.CrtOutputs(None, None, c.P, None, None, None, None)
    c.ws_bytes -= 1
    assert c() == _lib.CRT_ERR_WORKSPACE


@pytest.mark.parametrize("suffix", ["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_workspace_and_unsupported(lib, scheme, suffix):
    from crt1d_amd import _lib

    c = _Call(lib, scheme, suffix)
    c.ws_bytes -= 1
    assert c() == _lib.CRT_ERR_WORKSPACE
    c = _Call(lib, scheme, suffix)
    c.ws = None
    assert c() == _lib.CRT_ERR_WORKSPACE
    c = _Call(lib, scheme, suffix)  # the per-step workspace is not enough for a series
    c.ws_bytes = lib.crt_hip_workspace_bytes_nb(c.sid, 3, 7, 5)
    assert c() == _lib.CRT_ERR_WORKSPACE
    assert _Call(lib, "n79", suffix, nz=2, levels=(0, 1))() == _lib.CRT_ERR_SHAPE


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_unsupported_shapes_found_before_any_launch(lib, suffix):
    """Shapes no level-series kernel serves are CRT_ERR_UNSUPPORTED from a call with fake pointers: nothing was launched, so nothing -- not
    even the K0 records -- was written."""
    from crt1d_amd import _lib

    U = _lib.CRT_ERR_UNSUPPORTED
    assert _Call(lib, "n79", suffix, nz=3000, levels=(0, 2999))() == U    # n79 serves nz <= 1360
    assert _Call(lib, "zq", suffix, nz=3000, levels=(0, 2999))() == U     # zq nz <= 2271
    assert _Call(lib, "zq_pa", suffix, nz=5000, levels=(0, 4999))() == U  # zq_pa nz <= 4495 with two levels
    assert _Call(lib, "2s", suffix, nz=12000, levels=(0, 11999))() == U   # closed forms: the record must fit in 160 KB of LDS
    assert _Call(lib, "bl", suffix, nz=7000, levels=(0, 6999))() == U
    # t over two grid dimensions times the band slices: 3 slices x 2 > 65535 / ... fits; 40000 slices x 2 does not
    assert _Call(lib, "2s", suffix, ncol=1, nz=7, nb=1024 * 40000, nt=70000)() == U


def test_python_boundary_checks():
    """SunSeriesF32 / LevelsSeriesPlan reject host tensors and wrong dtypes before anything reaches the library."""
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(3, 4, 5, seed=1)
    s = synth.make_sun_series(d, 6, seed=2)
    t = lambda a: torch.as_tensor(a)  # noqa: E731  (host tensors)
    with pytest.raises(ValueError, match="GPU"):
        batched.SunSeriesF32(t(s["psi"]), t(s["I_dr0"]).float(), t(s["I_df0"]).float())
    with pytest.raises(ValueError, match="GPU"):
        batched.SunSeriesF32.from_host(s, "cpu")
    assert issubclass(batched.SunSeriesF32, batched.SunSeries)
    assert batched.SunSeriesF32._c_type is __import__("crt1d_amd")._lib.CrtSunSeriesF32
    for name in ("LevelsSeriesPlan", "solve_levels_series", "spectral_totals_series", "levels_series_workspace_bytes"):
        assert callable(getattr(batched, name)), name
    assert batched.levels_series_workspace_bytes("n79", 3, 20, 4) <= batched.series_workspace_bytes("n79", 3, 20, 9, 4)
    from crt1d_amd.model import Model

    assert callable(Model.run_series_levels)


def test_python_shape_and_dtype_checks_without_a_device(monkeypatch):
    """The rules of SunSeriesF32 and LevelsSeriesPlan's own argument checks, exercised without a device: `_f64` / `_f32` are the only
    places that ask for one."""
    import torch

    from crt1d_amd import batched

    f64, f32 = torch.float64, torch.float32

    def chk(dtype):
        def f(t, name):
            if t.dtype != dtype:
                raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
            return t.contiguous()
        return f

    monkeypatch.setattr(batched, "_f64", chk(f64))
    monkeypatch.setattr(batched, "_f32", chk(f32))
    psi = torch.zeros(3, 6, dtype=f64)
    ok = batched.SunSeriesF32(psi, torch.zeros(3, 6, 4, dtype=f32), torch.zeros(3, 6, 4, dtype=f32))
    assert (ok.ncol, ok.nt, ok.nb, ok.col_stride) == (3, 6, 4, 24)
    assert ok.I_dr0.dtype == f32 and ok.psi.dtype == f64
    sh = batched.SunSeriesF32(psi, torch.zeros(6, 4, dtype=f32), torch.zeros(1, 6, 4, dtype=f32))
    assert sh.col_stride == 0 and sh.slice(1, 3).ncol == 2 and isinstance(sh.slice(1, 3), batched.SunSeriesF32)
    assert isinstance(ok.c_struct(), __import__("crt1d_amd")._lib.CrtSunSeriesF32)
    with pytest.raises(TypeError):
        batched.SunSeriesF32(psi, torch.zeros(3, 6, 4, dtype=f64), torch.zeros(3, 6, 4, dtype=f64))  # float64 spectra
    with pytest.raises(TypeError):
        batched.SunSeries(psi, torch.zeros(3, 6, 4, dtype=f32), torch.zeros(3, 6, 4, dtype=f32))  # SunSeries stays float64
    with pytest.raises(TypeError):
        batched.SunSeriesF32(psi.float(), torch.zeros(3, 6, 4, dtype=f32), torch.zeros(3, 6, 4, dtype=f32))  # psi stays float64
    with pytest.raises(ValueError):
        batched.SunSeriesF32(psi, torch.zeros(3, 5, 4, dtype=f32), torch.zeros(3, 5, 4, dtype=f32))  # nt mismatch
    with pytest.raises(ValueError):
        batched.SunSeriesF32(psi, torch.zeros(3, 6, 4, dtype=f32), torch.zeros(3, 6, 5, dtype=f32))  # nb mismatch
    with pytest.raises(ValueError):
        batched.SunSeriesF32(psi, torch.zeros(3, 6, 4, dtype=f32), torch.zeros(3, 6, 4, dtype=f32), torch.zeros(3, 5, dtype=f64))
    # LevelsSeriesPlan: the checks that precede any use of the columns
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.LevelsSeriesPlan("nope", None, None, ok, (0,))
    with pytest.raises(ValueError, match="method"):
        batched.LevelsSeriesPlan("2s", None, None, ok, (0,), tau_d_method="simpson")
    with pytest.raises(TypeError, match="SunSeries"):
        batched.LevelsSeriesPlan("2s", None, None, {"psi": psi}, (0,))
    for keys in ((), ("I_d",), ("F", "F")):
        with pytest.raises(ValueError, match="keys"):
            batched.LevelsSeriesPlan("2s", None, None, ok, (0,), keys=keys)
    # the integrated series takes float64 spectra only
    with pytest.raises(TypeError, match="float64"):
        batched.IntegratedSeriesPlan("2s", None, None, ok, None)
