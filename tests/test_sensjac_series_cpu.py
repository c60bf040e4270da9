"""CPU: the sun-angle series of the sensor Jacobian (include/crt1d_hip_sensjac_series.h).  Its symbols have a table of their own next to
unchanged tables; every status of crt_hip_sensor_jac_series_f64 is found before any launch, in its order of precedence (fake device
pointers, as tests/test_sensjac_cpu.py); the workspace query equals the documented layout; and the Python errors of
SensorJacSeriesPlan / sensor_jacobian_series that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
HEADER = "crt1d_hip_sensjac_series.h"
SERVED = ["2s", "bl", "g77", "bf"]
NOT_SERVED = ["n79", "zq", "4s", "zq_pa"]
NAMES = ["crt_hip_g_dparam_series_f64", "crt_hip_sensor_jac_series_f64", "crt_hip_sensor_jac_series_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _code(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def _declared(header):
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _code(header))))


def test_series_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    assert _declared(HEADER) == sorted(_lib.SENSJAC_SERIES_EXPORTS) == sorted(_lib._SENSJAC_SERIES_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS)
    for name in NAMES:
        assert hasattr(lib, name)
        for other in others:
            assert name not in other
    for name, (_, argtypes) in _lib._SENSJAC_SERIES_SIGNATURES.items():  # the argument counts of the table are those of the header
        m = re.search(name + r"\s*\((.*?)\)\s*;", _code(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    # the other headers keep their symbol sets, crt1d_hip.h its version
    for header, table in (("crt1d_hip.h", _lib.EXPORTS), ("crt1d_hip_sensor.h", _lib.SENSOR_EXPORTS), ("crt1d_hip_dleaf.h", _lib.DLEAF_EXPORTS),
                          ("crt1d_hip_sensjac.h", _lib.SENSJAC_EXPORTS)):
        assert _declared(header) == sorted(table), header
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_tangent_series_struct_layout():
    from crt1d_amd import _lib

    S, names = _lib.CrtLeafTangentSeries, ["dg_table", "dg_at_psi", "dmla"]
    assert ctypes.sizeof(S) == 24 and [f[0] for f in S._fields_] == names
    assert [getattr(S, k).offset for k in names] == [0, 8, 16]
    m = re.search(r"typedef struct crt_leaf_tangent_series \{(.*?)\} crt_leaf_tangent_series;", _code(), re.S)
    assert re.findall(r"\*\s*(\w+);", m.group(1)) == names


def _sens(first, count, w=FAKE):
    from crt1d_amd import _lib

    n = len(first)
    f, k = (ctypes.c_int32 * max(n, 1))(*first), (ctypes.c_int32 * max(n, 1))(*count)
    s = _lib.CrtSensorSet(n, f, k, w)
    s._keep = (f, k)
    return s


def _args(nz=20, nb=8, ncol=2, nt=3, nsens=3, ntan=2):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no workspace ->
    CRT_ERR_WORKSPACE, no launch).  cols.psi / g_at_psi and bands.I_dr0 / I_df0 are NULL: the series entry does not read them."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, None, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, None, None, FAKE, FAKE, FAKE)
    sun = _lib.CrtSunSeries(nt, FAKE, None, nt * nb, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    sens = _sens([0, 2, 0][:nsens], [3, 1, nb][:nsens])
    dirs = _lib.CrtOpticsDirs(ntan, 0, FAKE, FAKE, FAKE)
    out = _lib.CrtSensJacOut(FAKE, FAKE, FAKE, FAKE)
    tan = _lib.CrtLeafTangentSeries(FAKE, FAKE, None)
    return c, b, sun, o, sens, dirs, tan, out


def _call(lib, scheme, c, b, sun, o, levels, sens, dirs, lai, tan, out, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_sensor_jac_series_f64(sid, ref(c), ref(b), ref(sun), ref(o), arr, n, ref(sens), ref(dirs), lai, ref(tan), ref(out), ws,
                                             wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_series_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, U, nz, nb, nt = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, _lib.CRT_ERR_UNSUPPORTED, 20, 8, 3
    c, b, sun, o, sens, dirs, tan, out = _args(nz, nb, nt=nt)
    S, T, D, O = _lib.CrtSunSeries, _lib.CrtLeafTangentSeries, _lib.CrtOpticsDirs, _lib.CrtSensJacOut

    def call(c=c, b=b, sun=sun, o=o, levels=(0, nz - 1), sens=sens, dirs=dirs, lai=1, tan=tan, out=out, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, sun, o, None if levels is None else list(levels), sens, dirs, lai, tan, out, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    sid = _lib.SCHEME_IDS[scheme]
    need = lib.crt_hip_sensor_jac_series_workspace_bytes(sid, 2, nz, nb, nt, 2, 3, 4)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS
    assert call(tan=T(FAKE, FAKE, FAKE)) == WS  # with dmla
    for one in range(4):  # any single output is enough
        assert call(out=O(*[FAKE if i == one else None for i in range(4)])) == WS
    # every parameter column alone, and the parameter axis empty
    assert call(lai=0, tan=None) == WS
    assert call(dirs=None, tan=None) == WS
    assert call(dirs=None, lai=0) == WS
    assert call(dirs=None, lai=0, tan=None) == BAD
    assert call(dirs=D(0, 0, FAKE, FAKE, FAKE), lai=0, tan=None) == BAD
    # the sun series: NULL, nt < 1, and what crt_hip_sensor_levels_series_f64 rejects about it
    assert call(sun=None) == BAD
    assert call(sun=S(0, FAKE, None, 0, FAKE, FAKE)) == BAD
    assert call(sun=S(-1, FAKE, None, 0, FAKE, FAKE)) == BAD
    assert call(sun=S(nt, None, None, nt * nb, FAKE, FAKE)) == BAD
    assert call(sun=S(nt, FAKE, None, nt * nb, None, FAKE)) == BAD
    assert call(sun=S(nt, FAKE, None, nt * nb, FAKE, None)) == BAD
    assert call(sun=S(nt, FAKE, None, nt * nb - 1, FAKE, FAKE)) == BAD  # col_stride neither 0 nor >= nt * nb
    assert call(sun=S(nt, FAKE, None, 0, FAKE, FAKE)) == WS  # shared spectra
    assert call(sun=S(nt, FAKE, FAKE, nt * nb, FAKE, FAKE)) == WS  # with g_at_psi
    ctab = _lib.CrtColumns(2, nz, None, FAKE, FAKE, FAKE, FAKE, None, FAKE)  # G_TABLE columns need sun.g_at_psi
    assert call(c=ctab) == BAD and call(c=ctab, sun=S(nt, FAKE, FAKE, nt * nb, FAKE, FAKE)) == WS
    # a tangent must be whole
    assert call(tan=T(None, FAKE, None)) == BAD
    assert call(tan=T(FAKE, None, FAKE)) == BAD
    assert call(tan=T(None, None, None)) == BAD
    # the rest of the parameter-axis parse: without a direction (ntan = 0) neither the stride nor the pointers are looked at; any with_lai
    # but 0 counts as set; sizes that are not positive are an argument error
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None)) == WS
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None), lai=0, tan=None) == BAD
    assert call(dirs=None, lai=2, tan=None) == WS
    assert call(c=_lib.CrtColumns(0, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)) == BAD
    assert call(c=_lib.CrtColumns(2, 0, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), levels=(0,)) == BAD
    for one in range(3):  # any single direction array is enough
        assert call(dirs=_lib.CrtOpticsDirs(2, 0, *[FAKE if i == one else None for i in range(3)])) == WS
    assert call(dirs=D(-1, 0, FAKE, FAKE, FAKE)) == BAD
    # the directions, the outputs, the sensor set: as crt_hip_sensor_jac_f64
    assert call(dirs=D(2, 0, None, None, None)) == BAD
    assert call(dirs=D(_lib.SENSJAC_MAX_NTAN + 1, 0, FAKE, FAKE, FAKE)) == BAD
    assert call(dirs=D(2, 2 * nb, FAKE, FAKE, FAKE)) == WS  # per column
    assert call(dirs=D(2, nb, FAKE, FAKE, FAKE)) == BAD
    assert call(out=None) == BAD
    assert call(out=O(None, None, None, None)) == BAD
    assert call(sens=None) == BAD
    assert call(sens=_sens([0] * 65, [1] * 65)) == BAD
    assert call(sens=_sens([nb - 1], [2])) == BAD
    assert call(sens=_sens([nb - 1], [1])) == WS
    # everything the levels entry rejects
    assert call(c=None) == BAD
    assert call(b=None) == BAD
    assert call(levels=None, nsel=1) == BAD
    assert call(nsel=0) == BAD
    assert call(levels=(3, 2)) == BAD
    assert call(levels=(nz,)) == BAD
    assert call(scheme=42) == BAD
    assert call(o=_lib.CrtOptions(0.501, 5, 0)) == BAD
    assert call(b=_lib.CrtBands(nb, nb, None, None, None, FAKE, FAKE)) == BAD  # no leaf_r
    soilless = call(b=_lib.CrtBands(nb, nb, None, None, FAKE, FAKE, None))
    assert soilless == (WS if scheme == "bl" else BAD)
    # CRT_ERR_SHAPE after the argument errors, before the workspace: nz < 2
    assert call(c=_args(1, nb)[0], levels=(0,)) == _lib.CRT_ERR_SHAPE
    assert call(c=_args(1, nb)[0], levels=(0,), sun=None) == BAD
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == WS
    # CRT_ERR_UNSUPPORTED after the workspace check: nsel * max(3 npar, 4) staging rows of 64 doubles beyond the LDS.  npar = 4 here: 12 rows
    # per level, 26 levels = 312 rows fit, 27 do not; at 5 parameters 20 levels fit and 21 do not
    c100, big = _args(100, nb)[0], 1 << 30
    assert call(c=c100, levels=range(26), ws=FAKE, wsb=need) == WS
    assert call(c=c100, levels=range(27), ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(27), ws=FAKE, wsb=big) == U
    d3 = D(3, 0, FAKE, FAKE, FAKE)
    assert call(c=c100, levels=range(21), dirs=d3, ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(21), dirs=d3, ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(21), dirs=d3, ws=FAKE, wsb=big, out=None) == BAD  # (an argument error is still one)
    assert call(c=c100, levels=range(21), dirs=d3, ws=FAKE, wsb=big, sun=None) == BAD


@pytest.mark.parametrize("scheme", SERVED)
def test_series_grid_refusals_without_gpu(lib, scheme):
    """Several band slices and an nt for which nslice * ceil(nt / 65535) > 65535: CRT_ERR_UNSUPPORTED behind the workspace check, before any
    launch; likewise a finish grid beyond 2^31 blocks."""
    from crt1d_amd import _lib

    WS, U, sid = _lib.CRT_ERR_WORKSPACE, _lib.CRT_ERR_UNSUPPORTED, _lib.SCHEME_IDS[scheme]
    q = lib.crt_hip_sensor_jac_series_workspace_bytes
    # 2151 bands, 2 levels, 5 parameters: 9 slices of 256 lanes; 9 * ceil(nt / 65535) > 65535 from nt = 7281 * 65535 + 1 on
    nz, nb, nt = 2, 2151, 7281 * 65535 + 1
    c, b, sun, o, sens, dirs, tan, out = _args(nz, nb, ncol=1, nt=nt, nsens=1, ntan=3)
    need = q(sid, 1, nz, nb, nt, 2, 1, 5)
    assert need > 0
    assert _call(lib, scheme, c, b, sun, o, [0, 1], sens, dirs, 1, tan, out, ws=FAKE, wsb=need - 1) == WS
    assert _call(lib, scheme, c, b, sun, o, [0, 1], sens, dirs, 1, tan, out, ws=FAKE, wsb=need) == U
    # 300 bands: 2 slices, the grid fits (2 * 3277 blocks); 64 sensor bands: (nt * 2 * 64 * 5 * 4 + 255) / 256 finish blocks > 2^31 - 1
    nb, nt = 300, 214748365
    c, b, sun, o, _, dirs, tan, out = _args(nz, nb, ncol=1, nt=nt, ntan=3)
    sens = _sens([0] * 64, [nb] * 64)
    need = q(sid, 1, nz, nb, nt, 2, 64, 5)
    assert need > 0
    assert _call(lib, scheme, c, b, sun, o, [0, 1], sens, dirs, 1, tan, out, ws=FAKE, wsb=need - 1) == WS
    assert _call(lib, scheme, c, b, sun, o, [0, 1], sens, dirs, 1, tan, out, ws=FAKE, wsb=need) == U


@pytest.mark.parametrize("scheme", NOT_SERVED)
def test_series_schemes_not_served(lib, scheme):
    """n79, zq, 4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors."""
    from crt1d_amd import _lib

    c, b, sun, o, sens, dirs, tan, out = _args()
    U, BAD = _lib.CRT_ERR_UNSUPPORTED, _lib.CRT_ERR_BAD_ARG
    call = lambda *a, **kw: _call(lib, scheme, *a, **kw)  # noqa: E731
    assert call(c, b, sun, o, [0, 19], sens, dirs, 1, tan, out) == U
    assert call(c, b, sun, o, [0, 19], sens, dirs, 1, tan, out, ws=FAKE, wsb=1 << 30) == U
    assert call(c, b, sun, o, [19, 0], sens, dirs, 1, tan, out) == BAD  # an argument error is still one
    assert call(c, b, None, o, [0, 19], sens, dirs, 1, tan, out) == BAD
    assert call(c, b, _lib.CrtSunSeries(0, FAKE, None, 0, FAKE, FAKE), o, [0, 19], sens, dirs, 1, tan, out) == BAD
    assert call(c, b, sun, o, [0, 19], None, dirs, 1, tan, out) == BAD
    assert call(c, b, sun, o, [0, 19], sens, dirs, 1, tan, None) == BAD
    assert call(c, b, sun, o, [0, 19], sens, None, 0, None, out) == BAD
    assert call(c, b, sun, o, [0, 19], sens, dirs, 1, _lib.CrtLeafTangentSeries(FAKE, None, None), out) == BAD
    assert call(_args(1)[0], b, sun, o, [0], sens, dirs, 1, tan, out) == _lib.CRT_ERR_SHAPE


def _slices(nb, nsel, npar):
    """Band slices of k_sens_jac (tests/test_sensjac_cpu.py): the widest of 256, 128, 64 lanes whose nsel * max(3 npar, 4) staging rows fit
    160 KB less 4 KB; where none fits the query sizes 64-lane slices."""
    w = 256
    while w >= 64 and nsel * max(3 * npar, 4) * w * 8 > 160 * 1024 - 4096:
        w //= 2
    return -(-nb // max(w, 64))


def test_series_workspace_query(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_sensor_jac_series_workspace_bytes
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            step = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, nb)
            lai = lib.crt_hip_levels_dlai_workspace_bytes(sid, 5, nz, nb, 2) - step  # the two side records, as their own entries keep them
            leaf = lib.crt_hip_levels_dleaf_workspace_bytes(sid, 5, nz, nb, 2) - step
            for nt in (1, 7):
                rec = lib.crt_hip_levels_series_workspace_bytes(sid, 5, nz, nt)
                assert rec > 0
                for nsel, nsens, npar in ((2, 13, 5), (2, 1, 1), (9, 5, 5), (16, 5, 5), (64, 3, 10)):
                    ns = _slices(nb, nsel, npar)
                    part = 0 if ns == 1 else 5 * nt * ns * nsel * nsens * npar * 4 * 8
                    assert q(sid, 5, nz, nb, nt, nsel, nsens, npar) == rec + lai + leaf + part, (scheme, nz, nb, nt, nsel, nsens, npar)
    # independent of how npar splits: the query takes npar alone, and the call accepts that size for every split
    sid, nz, nb, nt = _lib.SCHEME_IDS["bl"], 20, 300, 3
    need = q(sid, 2, nz, nb, nt, 2, 3, 3)
    c, b, sun, o, sens, _, tan, out = _args(nz, nb, nt=nt)
    D = _lib.CrtOpticsDirs
    for dirs, lai, tn in ((D(3, 0, FAKE, None, None), 0, None), (D(2, 0, FAKE, None, None), 1, None), (D(1, 0, FAKE, None, None), 1, tan),
                          (D(2, 0, FAKE, None, None), 0, tan)):
        assert _call(lib, "bl", c, b, sun, o, [0, 19], sens, dirs, lai, tn, out, ws=FAKE, wsb=need - 1) == _lib.CRT_ERR_WORKSPACE
    for bad in ((42, 5, 20, 8, 3, 2, 3, 4), (-1, 5, 20, 8, 3, 2, 3, 4), (0, 0, 20, 8, 3, 2, 3, 4), (0, 5, 0, 8, 3, 2, 3, 4), (0, 5, 20, 0, 3, 2, 3, 4),
                (0, 5, 20, 8, 0, 2, 3, 4), (0, 5, 20, 8, -2, 2, 3, 4), (0, 5, 20, 8, 3, 0, 3, 4), (0, 5, 20, 8, 3, 65, 3, 4), (0, -3, 20, 8, 3, 2, 3, 4),
                (0, 5, 20, 8, 3, 2, 0, 4), (0, 5, 20, 8, 3, 2, 65, 4), (0, 5, 20, 8, 3, 2, 3, 0), (0, 5, 20, 8, 3, 2, 3, 11)):
        assert q(*bad) == 0, bad


def _fake(cls, **attrs):
    """An instance of a device-bound dataclass without its constructor (which wants CUDA tensors): what the checks that touch no device
    look at is its type and the shapes given here."""
    x = object.__new__(cls)
    for k, v in attrs.items():
        setattr(x, k, v)
    return x


def test_series_plan_python_errors_need_no_device():
    import numpy as np
    import torch

    from crt1d_amd import batched

    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    sun = _fake(batched.SunSeries, psi=torch.zeros(1, 2, dtype=torch.float64))
    assert sun.nt == 2

    class FakeBands:  # (what the plan looks at before it touches a column or a device)
        dtype = torch.float32

    for make in (batched.SensorJacSeriesPlan, batched.sensor_jacobian_series):
        with pytest.raises(ValueError, match="unknown scheme"):
            make("nope", None, None, sun, (0,), sens)
        for scheme in ("4s", "zq_pa"):
            with pytest.raises(ValueError, match="has no sensor Jacobian"):
                make(scheme, None, None, sun, (0,), sens)
        for scheme in ("2s", "n79"):
            with pytest.raises(TypeError, match="sensors must be a SensorSet"):
                make(scheme, None, None, sun, (0,), np.ones((2, 8)))
            with pytest.raises(TypeError, match="sun must be a SunSeries"):
                make(scheme, None, None, _fake(batched.SunSeriesF32, psi=sun.psi), (0,), sens)
            with pytest.raises(TypeError, match="sun must be a SunSeries"):
                make(scheme, None, None, None, (0,), sens)
            with pytest.raises(TypeError, match="tangent must be a LeafTangentSeries"):
                make(scheme, None, None, sun, (0,), sens, tangent=_fake(batched.LeafTangent))
            with pytest.raises(ValueError, match="nt = 3 sun states, the series 2"):
                make(scheme, None, None, sun, (0,), sens, tangent=_fake(batched.LeafTangentSeries, dg_at_psi=torch.zeros(1, 3)))
            with pytest.raises(ValueError, match="no parameter at all"):
                make(scheme, None, None, sun, (0,), sens, lai=False)
            with pytest.raises(ValueError, match="must share ntan"):
                make(scheme, None, None, sun, (0,), sens, d_leaf_r=np.ones((2, 8)), d_soil_r=np.ones((5, 3, 8)))
    for scheme in ("2s", "zq"):
        with pytest.raises(TypeError, match="no f32 storage form"):
            batched.SensorJacSeriesPlan(scheme, None, FakeBands(), sun, (0,), sens)
    # n79 / zq are composed of per-step plans with workspaces of their own: no workspace, no flags
    for scheme in ("n79", "zq"):
        with pytest.raises(ValueError, match="workspace must be None"):
            batched.SensorJacSeriesPlan(scheme, None, None, sun, (0,), sens, workspace=torch.zeros(8))
        plan = _fake(batched.SensorJacSeriesPlan, scheme=scheme, _composed=True)
        with pytest.raises(ValueError, match="takes no flags"):
            plan(flags=1)
