"""CPU: the sun-angle series entry (crt_hip_integrated_series_f64) -- symbols, struct layout, every argument error (each found before
any launch, so no device is needed) and the Python boundary's shape / device checks."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for name in ("crt_hip_series_workspace_bytes", "crt_hip_integrated_series_f64"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.crt_hip_abi_version() == 3  # symbols were added, nothing changed


def test_sun_series_layout_matches_header(lib):
    from crt1d_amd import _lib

    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    body = text[text.index("typedef struct crt_sun_series {"):text.index("} crt_sun_series;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|int64_t|const double\*)\s+(\w+);", body)
    assert [f[1] for f in fields] == [f[0] for f in _lib.CrtSunSeries._fields_]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const double*": ctypes.c_void_p}
    assert [ctype[f[0]] for f in fields] == [f[1] for f in _lib.CrtSunSeries._fields_]
    assert ctypes.sizeof(_lib.CrtSunSeries) == 8 + 5 * 8  # nt (+ padding), psi, g_at_psi, col_stride, I_dr0, I_df0
    assert _lib.CrtSunSeries.psi.offset == 8 and _lib.CrtSunSeries.col_stride.offset == 24


def test_workspace_bytes(lib):
    from crt1d_amd import _lib

    for scheme, sid in _lib.SCHEME_IDS.items():
        for ncol, nz, nb in ((1, 5, 4), (10, 60, 12), (7, 100, 300), (3, 130, 1024)):
            prev = 0
            for nt in (1, 2, 3, 24, 1000, 70000):
                n = lib.crt_hip_series_workspace_bytes(sid, ncol, nz, nb, nt)
                assert n > prev, (scheme, ncol, nz, nb, nt)  # monotone in nt
                prev = n
            assert lib.crt_hip_series_workspace_bytes(sid, ncol, nz, nb, 1) >= lib.crt_hip_workspace_bytes_nb(sid, ncol, nz, nb)
        assert lib.crt_hip_series_workspace_bytes(sid, 4, 10, 8, 0) == 0
        assert lib.crt_hip_series_workspace_bytes(sid, 0, 10, 8, 3) == 0
    assert lib.crt_hip_series_workspace_bytes(99, 4, 10, 8, 3) == 0


class _Call:
    """A well-formed call with fake (never dereferenced) device pointers; tests break one argument at a time."""

    P = 0x10000  # any non-NULL value: every check below happens on the host, before a launch

    def __init__(self, lib, scheme="2s", ncol=3, nz=7, nb=5, nt=4, ng=2, profiles=True):
        from crt1d_amd import _lib

        self._lib, self.lib, self.sid = _lib, lib, _lib.SCHEME_IDS[scheme]
        P = self.P
        self.cols = _lib.CrtColumns(ncol, nz, None, P, P, P, P, None, None)
        self.bands = _lib.CrtBands(nb, nb, None, None, P, P, P)
        self.sun = _lib.CrtSunSeries(nt, P, None, nt * nb, P, P)
        self.opts = _lib.CrtOptions(0.501, 0, 0)
        keys = ("aI", "aI_sl", "aI_sh", "totals") + (("aI_dr", "I_dr", "I_df_d", "I_df_u", "F", "I_d") if profiles else ())
        self.out = _lib.CrtBandsumOut(**{k: P for k in keys})
        self.band_w, self.ng, self.ws = P, ng, P
        self.ws_bytes = lib.crt_hip_series_workspace_bytes(self.sid, ncol, nz, nb, nt)

    def __call__(self, sun="own", opts="own"):
        r = lambda x, own: None if x is None else ctypes.byref(own if isinstance(x, str) else x)  # noqa: E731
        return self.lib.crt_hip_integrated_series_f64(self.sid, ctypes.byref(self.cols), ctypes.byref(self.bands), r(sun, self.sun),
                                                      r(opts, self.opts), self.band_w, self.ng, ctypes.byref(self.out), self.ws,
                                                      self.ws_bytes, None)


@pytest.mark.parametrize("scheme", ["2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa"])
def test_bad_arguments(lib, scheme):
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG
    assert _Call(lib, scheme)(sun=None) == BAD
    for field in ("psi", "I_dr0", "I_df0"):
        c = _Call(lib, scheme)
        setattr(c.sun, field, None)
        assert c() == BAD, field
    for nt in (0, -3):
        c = _Call(lib, scheme)
        c.sun.nt = nt
        assert c() == BAD
    for stride in (1, 4 * 5 - 1, -20):
        c = _Call(lib, scheme)
        c.sun.col_stride = stride
        assert c() == BAD, stride
    c = _Call(lib, scheme)
    c.cols.g_table = c.P  # a table, but no per-step G(psi)
    assert c() == BAD
    # ... and what crt_hip_integrated2_f64 rejects
    c = _Call(lib, scheme)
    c.band_w = None
    assert c() == BAD
    for ng in (0, 5):
        c = _Call(lib, scheme)
        c.ng = ng
        assert c() == BAD
    c = _Call(lib, scheme)
    c.out.F = None  # the six optional outputs: all or none
    assert c() == BAD
    c = _Call(lib, scheme)
    c.out.aI_sl = None
    assert c() == BAD
    for field in ("lai", "g_kind"):
        c = _Call(lib, scheme)
        setattr(c.cols, field, None)
        assert c() == BAD, field
    for field in ("leaf_r", "leaf_t"):
        c = _Call(lib, scheme)
        setattr(c.bands, field, None)
        assert c() == BAD, field
    c = _Call(lib, scheme)
    c.bands.col_stride = 3
    assert c() == BAD
    c = _Call(lib, scheme)
    c.opts.tau_d_method = 7
    assert c() == BAD
    c = _Call(lib, scheme)
    c.opts.tune[_lib.NTUNE - 2] = 1  # reserved key
    assert c() == BAD
    c = _Call(lib, scheme)
    c.opts.tune[8] = 9  # CRT_TUNE_TRI_M takes 8 / 12 / 16
    assert c() == BAD
    if scheme == "2s":
        c = _Call(lib, scheme)
        c.cols.mla = None
        assert c() == BAD
    if scheme == "4s":
        c = _Call(lib, scheme)
        c.opts.mu_s = 1.5
        assert c() == BAD
    if scheme != "bl":
        c = _Call(lib, scheme)
        c.bands.soil_r = None
        assert c() == BAD
    assert _Call(lib, "2s").lib.crt_hip_integrated_series_f64(99, None, None, None, None, None, 1, None, None, 0, None) == BAD


@pytest.mark.parametrize("scheme", ["2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa"])
def test_workspace_and_unsupported(lib, scheme):
    from crt1d_amd import _lib

    c = _Call(lib, scheme)
    c.ws_bytes -= 1
    assert c() == _lib.CRT_ERR_WORKSPACE
    c = _Call(lib, scheme)
    c.ws = None
    assert c() == _lib.CRT_ERR_WORKSPACE
    c = _Call(lib, scheme)  # the per-step workspace is not enough for a series
    c.ws_bytes = lib.crt_hip_workspace_bytes_nb(c.sid, 3, 7, 5)
    assert c() == _lib.CRT_ERR_WORKSPACE
    for profiles in (False, True):
        c = _Call(lib, scheme, nb=1025, profiles=profiles)  # found before K0: nothing is launched, so nothing is written
        assert c() == _lib.CRT_ERR_UNSUPPORTED
    assert _Call(lib, "n79", nz=2)() == _lib.CRT_ERR_SHAPE


def test_python_boundary_checks():
    """SunSeries / IntegratedSeriesPlan reject wrong shapes and host tensors with ValueError before anything reaches the library."""
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(3, 4, 5, seed=1)
    s = synth.make_sun_series(d, 6, seed=2)
    assert s["psi"].shape == (3, 6) and s["I_dr0"].shape == (3, 6, 4) and s["I_df0"].shape == (3, 6, 4)
    assert np.all((s["psi"] >= 0) & (s["psi"] <= np.deg2rad(75.0)))
    assert np.all((s["I_dr0"] >= 0) & (s["I_dr0"] <= 10)) and np.all((s["I_df0"] >= 0) & (s["I_df0"] <= 5))
    assert synth.make_sun_series(d, 6, seed=2, shared=True)["I_dr0"].shape == (1, 6, 4)
    d2 = synth.make_columns(3, 4, 5, seed=1)  # make_columns itself is unchanged by the series generator
    assert all(np.array_equal(d[k], d2[k]) for k in d)
    t = lambda a: torch.as_tensor(a)  # noqa: E731  (host tensors)
    with pytest.raises(ValueError, match="GPU"):
        batched.SunSeries(t(s["psi"]), t(s["I_dr0"]), t(s["I_df0"]))
    with pytest.raises(ValueError, match="GPU"):
        batched.SunSeries.from_host(s, "cpu")
    assert batched.series_shapes(3, 6, 5, 2, profiles=True)["I_d"] == (3, 6, 5, 2)
    assert batched.series_shapes(3, 6, 5, 2)["totals"] == (3, 6, 2, 4)
    assert set(batched.series_shapes(3, 6, 5, 2)) == set(batched.bandsum_shapes(3, 5, 2))


def test_python_shape_checks_on_meta_free_path(monkeypatch):
    """The shape rules of SunSeries, exercised without a device: `_f64` is the only place that asks for one."""
    import torch

    from crt1d_amd import batched

    monkeypatch.setattr(batched, "_f64", lambda t, name: t.contiguous())
    psi = torch.zeros(3, 6, dtype=torch.float64)
    ok = batched.SunSeries(psi, torch.zeros(3, 6, 4, dtype=torch.float64), torch.zeros(3, 6, 4, dtype=torch.float64))
    assert (ok.ncol, ok.nt, ok.nb, ok.col_stride) == (3, 6, 4, 24)
    sh = batched.SunSeries(psi, torch.zeros(6, 4, dtype=torch.float64), torch.zeros(1, 6, 4, dtype=torch.float64))
    assert sh.col_stride == 0 and sh.slice(1, 3).ncol == 2
    with pytest.raises(ValueError):
        batched.SunSeries(torch.zeros(3, dtype=torch.float64), torch.zeros(3, 6, 4, dtype=torch.float64), torch.zeros(3, 6, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        batched.SunSeries(psi, torch.zeros(3, 5, 4, dtype=torch.float64), torch.zeros(3, 5, 4, dtype=torch.float64))  # nt mismatch
    with pytest.raises(ValueError):
        batched.SunSeries(psi, torch.zeros(2, 6, 4, dtype=torch.float64), torch.zeros(2, 6, 4, dtype=torch.float64))  # ncol mismatch
    with pytest.raises(ValueError):
        batched.SunSeries(psi, torch.zeros(3, 6, 4, dtype=torch.float64), torch.zeros(3, 6, 5, dtype=torch.float64))  # nb mismatch
    with pytest.raises(ValueError):
        batched.SunSeries(psi, torch.zeros(3, 6, 4, dtype=torch.float64), torch.zeros(3, 6, 4, dtype=torch.float64),
                          torch.zeros(3, 5, dtype=torch.float64))  # g_at_psi shape
