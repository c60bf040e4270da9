"""CPU: the LAI-derivative entry points (include/crt1d_hip_dlai.h) exist next to an unchanged crt1d_hip.h, every argument error and every
unsupported scheme or depth is found before any launch, and the plans' own checks."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf", "n79", "zq"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_dlai_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_dlai.h")
    assert names == sorted(_lib.DLAI_EXPORTS) == ["crt_hip_dtau_d_f64", "crt_hip_levels_dlai_f64", "crt_hip_levels_dlai_workspace_bytes"]
    for name in names:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.JAC_EXPORTS
    # crt1d_hip.h keeps its symbol set and its version
    assert _declared("crt1d_hip.h") == sorted(_lib.EXPORTS) and len(_lib.EXPORTS) == 57
    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3
    text = open(os.path.join(ROOT, "include", "crt1d_hip_dlai.h")).read()
    assert f"#define CRT_DLAI_MAX_NZ_N79 {_lib.DLAI_MAX_NZ['n79']}" in text
    assert f"#define CRT_DLAI_MAX_NZ_ZQ {_lib.DLAI_MAX_NZ['zq']}" in text


def test_dlai_out_layout():
    from crt1d_amd import _lib

    keys = ["I_dr", "I_df_d", "I_df_u", "F"]
    assert ctypes.sizeof(_lib.CrtDlaiOut) == 32
    assert [f[0] for f in _lib.CrtDlaiOut._fields_] == keys
    assert [getattr(_lib.CrtDlaiOut, k).offset for k in keys] == [0, 8, 16, 24]
    text = open(os.path.join(ROOT, "include", "crt1d_hip_dlai.h")).read()
    m = re.search(r"typedef struct crt_dlai_out \{(.*?)\} crt_dlai_out;", text, re.S)
    assert re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == keys


def _args(nz=20, nb=8, ncol=2):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no
    workspace -> CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    out = _lib.CrtDlaiOut(FAKE, FAKE, FAKE, FAKE)
    return c, b, o, out


def _call(lib, scheme, c, b, o, levels, out, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_levels_dlai_f64(sid, ref(c), ref(b), ref(o), arr, n, ref(out), ws, wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_dlai_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, nz, nb = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, 20, 8
    c, b, o, out = _args(nz, nb)

    def call(c=c, b=b, o=o, levels=(0, nz - 1), out=out, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, o, None if levels is None else list(levels), out, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    sid = _lib.SCHEME_IDS[scheme]
    need = lib.crt_hip_levels_dlai_workspace_bytes(sid, 2, nz, nb, 2)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS  # a short workspace
    if scheme in ("bl", "n79", "zq"):  # the K0 records alone do not do: the side records lie behind them
        assert call(ws=FAKE, wsb=lib.crt_hip_workspace_bytes_nb(sid, 2, nz, nb)) == WS
    for one in range(4):  # any single output is enough
        assert call(out=_lib.CrtDlaiOut(*[FAKE if i == one else None for i in range(4)])) == WS
    # the outputs
    assert call(out=None) == BAD
    assert call(out=_lib.CrtDlaiOut(None, None, None, None)) == BAD
    # everything the levels entry rejects
    assert call(c=None) == BAD
    assert call(b=None) == BAD
    assert call(levels=None, nsel=1) == BAD
    assert call(nsel=0) == BAD
    c100 = _args(100, nb)[0]
    assert call(c=c100, levels=range(64)) == WS
    assert call(c=c100, levels=range(65)) == BAD
    assert call(levels=(3, 2)) == BAD
    assert call(levels=(2, 2)) == BAD
    assert call(levels=(-1,)) == BAD
    assert call(levels=(nz,)) == BAD
    assert call(scheme=42) == BAD
    assert call(scheme=-1) == BAD
    assert call(o=_lib.set_tune(_lib.CrtOptions(0.501, 0, 0), {_lib.TUNE_TRI_M: 10})) == BAD
    assert call(o=_lib.CrtOptions(0.501, 5, 0)) == BAD
    assert call(b=_lib.CrtBands(nb, nb - 1, FAKE, FAKE, FAKE, FAKE, FAKE)) == BAD  # col_stride neither 0 nor >= nb
    assert call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, None, FAKE, FAKE)) == BAD  # no leaf_r
    soilless = call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, None))
    assert soilless == (WS if scheme == "bl" else BAD)
    # CRT_ERR_SHAPE as crt_hip_levels_f64: nz < 2; n79: nz < 3
    assert call(c=_args(1, nb)[0], levels=(0,)) == _lib.CRT_ERR_SHAPE
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == (_lib.CRT_ERR_SHAPE if scheme == "n79" else WS)


@pytest.mark.parametrize("scheme", ["4s", "zq_pa"])
def test_dlai_schemes_not_served(lib, scheme):
    """4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors (the precedence of
    crt_hip_levels_jac_f64)."""
    from crt1d_amd import _lib

    c, b, o, out = _args()
    assert _call(lib, scheme, c, b, o, [0, 19], out) == _lib.CRT_ERR_UNSUPPORTED
    assert _call(lib, scheme, c, b, o, [0, 19], out, ws=FAKE, wsb=1 << 30) == _lib.CRT_ERR_UNSUPPORTED
    assert _call(lib, scheme, c, b, o, [19, 0], out) == _lib.CRT_ERR_BAD_ARG  # an argument error is still one
    assert _call(lib, scheme, c, b, o, [0, 19], None) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, None, o, [0, 19], out) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, _lib.CrtBands(8, 8, FAKE, FAKE, None, FAKE, FAKE), o, [0, 19], out, ws=FAKE, wsb=1 << 30) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, _lib.CrtOptions(0.501, 5, 0), [0, 19], out) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, _args(1)[0], b, o, [0], out) == _lib.CRT_ERR_SHAPE


@pytest.mark.parametrize("scheme", ["n79", "zq"])
def test_dlai_depth_limit_without_gpu(lib, scheme):
    """One level past the documented depth: CRT_ERR_UNSUPPORTED before K0 (the fake pointers are never used); at the limit the call
    would launch, so only the workspace check is exercised there.  The limits lie below those of the optics Jacobian: the record part is
    staged twice."""
    from crt1d_amd import _lib

    lim = _lib.DLAI_MAX_NZ[scheme]
    sid = _lib.SCHEME_IDS[scheme]
    for nb in (1, 300):
        c, b, o, out = _args(lim + 1, nb, ncol=1)
        need = lib.crt_hip_levels_dlai_workspace_bytes(sid, 1, lim + 1, nb, 2)
        assert need > 0
        assert _call(lib, scheme, c, b, o, [0, lim], out, ws=FAKE, wsb=need) == _lib.CRT_ERR_UNSUPPORTED
        assert _call(lib, scheme, c, b, o, [0, lim], out) == _lib.CRT_ERR_WORKSPACE  # the workspace comes before the depth
        c, b, o, out = _args(lim, nb, ncol=1)
        assert _call(lib, scheme, c, b, o, [0, lim - 1], out) == _lib.CRT_ERR_WORKSPACE
    assert 150 <= lim < _lib.JAC_MAX_NZ[scheme]


def test_dlai_workspace_query(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_levels_dlai_workspace_bytes
    side = {"bl": lambda nz: nz, "n79": lambda nz: 16 + 3 * nz, "zq": lambda nz: 16 + nz}
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, nb)
            assert rec > 0
            want = rec + 5 * 8 * side.get(scheme, lambda nz: 0)(nz)  # the K0 records, the side records behind them
            assert q(sid, 5, nz, nb, 2) == q(sid, 5, nz, nb, 64) == want
    for bad in ((42, 5, 20, 8, 2), (-1, 5, 20, 8, 2), (0, 0, 20, 8, 2), (0, 5, 0, 8, 2), (0, 5, 20, 0, 2), (0, 5, 20, 8, 0), (0, 5, 20, 8, 65),
                (0, -3, 20, 8, 2)):
        assert q(*bad) == 0, bad


def test_dtau_d_validation_without_gpu(lib):
    from crt1d_amd import _lib

    f = lib.crt_hip_dtau_d_f64
    assert f(None, FAKE, 4, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, None, 4, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, 4, 0, None, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, -1, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, 4, 2, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, 0, 1, FAKE, None) == _lib.CRT_OK  # nothing to do, nothing launched


def test_dlai_plan_python_errors_need_no_device():
    from crt1d_amd import batched

    assert batched.DLAI_KEYS == ("I_dr", "I_df_d", "I_df_u", "F") and batched.DLAI_SCHEMES == tuple(SERVED)
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.LevelsDlaiPlan("nope", None, None, (0,))
    with pytest.raises(ValueError, match="invalid `method`"):
        batched.LevelsDlaiPlan("2s", None, None, (0,), tau_d_method="nope")
    for scheme in ("4s", "zq_pa"):
        with pytest.raises(ValueError, match="has no LAI-derivative kernel"):
            batched.LevelsDlaiPlan(scheme, None, None, (0,))
    for keys in (("x0",), ("F", "F"), (), ("I_d",)):
        with pytest.raises(ValueError, match="keys must be distinct"):
            batched.LevelsDlaiPlan("2s", None, None, (0,), keys=keys)
    for per in ("percent", None, "LOG", 1):
        with pytest.raises(ValueError, match="per must be"):
            batched.LevelsDlaiPlan("2s", None, None, (0,), per=per)
    with pytest.raises(TypeError, match="must be a SensorSet"):
        batched.sensor_dlai("2s", None, None, (0,), np.ones((2, 8)))
    # the one-shot functions keep the promise too: nothing of `cols` is read before the scheme, the method and `per` are checked
    for scheme in ("4s", "zq_pa"):
        with pytest.raises(ValueError, match="has no LAI-derivative kernel"):
            batched.solve_levels_dlai(scheme, None, None, (0,))
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.solve_levels_dlai("nope", None, None, (0,))
    with pytest.raises(ValueError, match="invalid `method`"):
        batched.solve_levels_dlai("n79", None, None, (0,), tau_d_method="nope")
    with pytest.raises(ValueError, match="per must be"):
        batched.solve_levels_dlai("2s", None, None, (0,), per="percent")


def test_sensor_dlai_errors_need_no_device():
    import torch

    from crt1d_amd import batched

    class _Cols:
        ncol, device = 3, torch.device("cpu")

    class _Bands:
        nb = 7

    s = batched.SensorSet(np.ones((2, 8)), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="per must be"):
        batched.sensor_dlai("2s", _Cols, _Bands, (0,), s, per="percent")
    with pytest.raises(ValueError, match="has no LAI-derivative kernel"):
        batched.sensor_dlai("4s", _Cols, _Bands, (0,), s)
    with pytest.raises(ValueError, match="the sensor set was built for nb = 8"):
        batched.sensor_dlai("2s", _Cols, _Bands, (0,), s)
