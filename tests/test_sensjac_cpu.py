"""CPU: the sensor-Jacobian entry points (include/crt1d_hip_sensjac.h) exist next to unchanged headers, the structs match the header,
every argument error, every scheme that is not served, a short workspace and a configuration beyond the LDS are found before any launch
(fake device pointers, as tests/test_grad_cpu.py), the workspace query, and the Python errors of SensorJacPlan / sensor_jacobian /
gauss_newton_step that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf"]
NOT_SERVED = ["n79", "zq", "4s", "zq_pa"]
NAMES = ["crt_hip_sensor_jac_f64", "crt_hip_sensor_jac_workspace_bytes"]
O_KEYS = ["I_dr", "I_df_d", "I_df_u", "F"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "crt1d_hip_sensjac.h")).read()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_sensjac_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_sensjac.h")
    assert names == sorted(_lib.SENSJAC_EXPORTS) == sorted(_lib._SENSJAC_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS)
    for name in names:
        assert hasattr(lib, name)
        for other in others:
            assert name not in other
    # the argument counts of the table are those of the header
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, (_, argtypes) in _lib._SENSJAC_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    assert int(re.search(r"#define CRT_SENSJAC_MAX_NTAN (\d+)", _header()).group(1)) == _lib.SENSJAC_MAX_NTAN == 8
    # the other headers keep their symbol sets, crt1d_hip.h its version
    for header, table in (("crt1d_hip.h", _lib.EXPORTS), ("crt1d_hip_sensor.h", _lib.SENSOR_EXPORTS), ("crt1d_hip_jac.h", _lib.JAC_EXPORTS),
                          ("crt1d_hip_dlai.h", _lib.DLAI_EXPORTS), ("crt1d_hip_dleaf.h", _lib.DLEAF_EXPORTS), ("crt1d_hip_grad.h", _lib.GRAD_EXPORTS)):
        assert _declared(header) == sorted(table), header
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_struct_layouts():
    from crt1d_amd import _lib

    S = _lib.CrtSensJacOut
    assert ctypes.sizeof(S) == 32 and [f[0] for f in S._fields_] == O_KEYS
    assert [getattr(S, k).offset for k in O_KEYS] == [0, 8, 16, 24]
    m = re.search(r"typedef struct crt_sensjac_out \{(.*?)\} crt_sensjac_out;", _header(), re.S)
    assert re.findall(r"\*\s*(\w+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == O_KEYS
    D = _lib.CrtOpticsDirs
    names = ["ntan", "col_stride", "leaf_r", "leaf_t", "soil_r"]
    assert ctypes.sizeof(D) == 40 and [f[0] for f in D._fields_] == names
    assert [getattr(D, k).offset for k in names] == [0, 8, 16, 24, 32]  # (int32, padding, int64, three pointers)
    m = re.search(r"typedef struct crt_optics_dirs \{(.*?)\} crt_optics_dirs;", _header(), re.S)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == names


def _args(nz=20, nb=8, ncol=2, nsens=3, ntan=2):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no
    workspace -> CRT_ERR_WORKSPACE, no launch).  The sensor supports are host arrays: real ones."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    sens = _sens([0, 2, 0][:nsens], [3, 1, nb][:nsens])
    dirs = _lib.CrtOpticsDirs(ntan, 0, FAKE, FAKE, FAKE)
    out = _lib.CrtSensJacOut(FAKE, FAKE, FAKE, FAKE)
    tan = _lib.CrtLeafTangent(FAKE, FAKE, None)
    return c, b, o, sens, dirs, tan, out


def _sens(first, count, w=FAKE):
    from crt1d_amd import _lib

    n = len(first)
    f, k = (ctypes.c_int32 * max(n, 1))(*first), (ctypes.c_int32 * max(n, 1))(*count)
    s = _lib.CrtSensorSet(n, f, k, w)
    s._keep = (f, k)
    return s


def _call(lib, scheme, c, b, o, levels, sens, dirs, lai, tan, out, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_sensor_jac_f64(sid, ref(c), ref(b), ref(o), arr, n, ref(sens), ref(dirs), lai, ref(tan), ref(out), ws, wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_sensjac_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, U, nz, nb = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, _lib.CRT_ERR_UNSUPPORTED, 20, 8
    c, b, o, sens, dirs, tan, out = _args(nz, nb)

    def call(c=c, b=b, o=o, levels=(0, nz - 1), sens=sens, dirs=dirs, lai=1, tan=tan, out=out, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, o, None if levels is None else list(levels), sens, dirs, lai, tan, out, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    sid = _lib.SCHEME_IDS[scheme]
    need = lib.crt_hip_sensor_jac_workspace_bytes(sid, 2, nz, nb, 2, 3, 4)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS  # a short workspace
    assert call(tan=_lib.CrtLeafTangent(FAKE, FAKE, FAKE)) == WS  # with dmla
    for one in range(4):  # any single output is enough
        assert call(out=_lib.CrtSensJacOut(*[FAKE if i == one else None for i in range(4)])) == WS
    # every parameter column alone, and the parameter axis empty
    assert call(lai=0, tan=None) == WS
    assert call(dirs=None, tan=None) == WS
    assert call(dirs=None, lai=0) == WS
    assert call(dirs=_lib.CrtOpticsDirs(0, 0, None, None, None), lai=0) == WS
    assert call(dirs=None, lai=0, tan=None) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(0, 0, FAKE, FAKE, FAKE), lai=0, tan=None) == BAD
    # the directions
    for one in range(3):  # any single direction array is enough
        assert call(dirs=_lib.CrtOpticsDirs(2, 0, *[FAKE if i == one else None for i in range(3)])) == WS
    assert call(dirs=_lib.CrtOpticsDirs(2, 0, None, None, None)) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(-1, 0, FAKE, FAKE, FAKE)) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN, 0, FAKE, FAKE, FAKE)) == WS
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN + 1, 0, FAKE, FAKE, FAKE)) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(2, 2 * nb, FAKE, FAKE, FAKE)) == WS  # per column
    assert call(dirs=_lib.CrtOpticsDirs(2, nb, FAKE, FAKE, FAKE)) == BAD  # col_stride neither 0 nor ntan * nb
    # the outputs
    assert call(out=None) == BAD
    assert call(out=_lib.CrtSensJacOut(None, None, None, None)) == BAD
    # a tangent must be whole
    assert call(tan=_lib.CrtLeafTangent(None, FAKE, None)) == BAD
    assert call(tan=_lib.CrtLeafTangent(FAKE, None, FAKE)) == BAD
    assert call(tan=_lib.CrtLeafTangent(None, None, None)) == BAD
    # the rest of the parameter-axis parse: without a direction (ntan = 0) neither the stride nor the pointers are looked at; any with_lai
    # but 0 counts as set; sizes that are not positive are an argument error
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None)) == WS
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None), lai=0, tan=None) == BAD
    assert call(dirs=None, lai=2, tan=None) == WS
    assert call(c=_lib.CrtColumns(0, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)) == BAD
    assert call(c=_lib.CrtColumns(2, 0, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), levels=(0,)) == BAD
    # the sensor set, as crt_hip_sensor_levels_f64
    assert call(sens=None) == BAD
    assert call(sens=_sens([0], [nb], w=None)) == BAD
    assert call(sens=_lib.CrtSensorSet(1, None, sens.count, FAKE)) == BAD
    assert call(sens=_lib.CrtSensorSet(1, sens.first, None, FAKE)) == BAD
    assert call(sens=_lib.CrtSensorSet(0, sens.first, sens.count, FAKE)) == BAD
    assert call(sens=_sens([0] * 64, [1] * 64)) == WS
    assert call(sens=_sens([0] * 65, [1] * 65)) == BAD
    assert call(sens=_sens([0], [0])) == BAD
    assert call(sens=_sens([-1], [2])) == BAD
    assert call(sens=_sens([nb - 1], [2])) == BAD
    assert call(sens=_sens([nb - 1], [1])) == WS
    # everything the levels entry rejects
    assert call(c=None) == BAD
    assert call(b=None) == BAD
    assert call(levels=None, nsel=1) == BAD
    assert call(nsel=0) == BAD
    c100 = _args(100, nb)[0]
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
    assert call(b=_lib.CrtBands(nb, 0, FAKE, FAKE, FAKE, FAKE, FAKE)) == WS  # shared spectra
    assert call(b=_lib.CrtBands(0, 0, FAKE, FAKE, FAKE, FAKE, FAKE)) == BAD
    assert call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, None, FAKE, FAKE)) == BAD  # no leaf_r
    soilless = call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, None))
    assert soilless == (WS if scheme == "bl" else BAD)
    # CRT_ERR_SHAPE as crt_hip_levels_f64: nz < 2
    assert call(c=_args(1, nb)[0], levels=(0,)) == _lib.CRT_ERR_SHAPE
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == WS
    # CRT_ERR_UNSUPPORTED after the workspace check: nsel * max(3 npar, 4) staging rows of 64 doubles beyond the LDS.  npar = 4 here: 12 rows
    # per level, 26 levels = 312 rows fit, 27 do not; a lone LAI column has 4 rows per level, so all 64 levels fit
    big = 1 << 30
    assert call(c=c100, levels=range(26), ws=FAKE, wsb=need) == WS
    assert call(c=c100, levels=range(27), ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(27), ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(64), ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(27), ws=FAKE, wsb=big, out=None) == BAD  # (an argument error is still one)


@pytest.mark.parametrize("scheme", NOT_SERVED)
def test_sensjac_schemes_not_served(lib, scheme):
    """n79, zq, 4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors."""
    from crt1d_amd import _lib

    c, b, o, sens, dirs, tan, out = _args()
    U, BAD = _lib.CRT_ERR_UNSUPPORTED, _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, o, [0, 19], sens, dirs, 1, tan, out) == U
    assert _call(lib, scheme, c, b, o, [0, 19], sens, dirs, 1, tan, out, ws=FAKE, wsb=1 << 30) == U
    assert _call(lib, scheme, c, b, o, [19, 0], sens, dirs, 1, tan, out) == BAD  # an argument error is still one
    assert _call(lib, scheme, c, b, o, [0, 19], None, dirs, 1, tan, out) == BAD
    assert _call(lib, scheme, c, b, o, [0, 19], sens, dirs, 1, tan, None) == BAD
    assert _call(lib, scheme, c, b, o, [0, 19], sens, None, 0, None, out) == BAD
    assert _call(lib, scheme, c, None, o, [0, 19], sens, dirs, 1, tan, out) == BAD
    assert _call(lib, scheme, c, b, _lib.CrtOptions(0.501, 5, 0), [0, 19], sens, dirs, 1, tan, out) == BAD
    assert _call(lib, scheme, _args(1)[0], b, o, [0], sens, dirs, 1, tan, out) == _lib.CRT_ERR_SHAPE
    if scheme == "n79":
        assert _call(lib, scheme, _args(2)[0], b, o, [0, 1], sens, dirs, 1, tan, out) == _lib.CRT_ERR_SHAPE


def _slices(nb, nsel, npar):
    """(band slices, lanes) of k_sens_jac: the widest of 256, 128, 64 lanes whose nsel * max(3 npar, 4) staging rows fit 160 KB less 4 KB."""
    w = 256
    while w >= 64 and nsel * max(3 * npar, 4) * w * 8 > 160 * 1024 - 4096:
        w //= 2
    w = max(w, 64)  # (none fits: the query sizes 64-lane slices, the call refuses)
    return -(-nb // w)


def test_sensjac_workspace_query(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_sensor_jac_workspace_bytes
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, nb)
            assert rec > 0
            lai = lib.crt_hip_levels_dlai_workspace_bytes(sid, 5, nz, nb, 2) - rec  # the two side records, as their own entries keep them
            leaf = lib.crt_hip_levels_dleaf_workspace_bytes(sid, 5, nz, nb, 2) - rec
            for nsel, nsens, npar in ((2, 13, 5), (2, 1, 1), (9, 5, 5), (16, 5, 5), (64, 3, 10)):
                ns = _slices(nb, nsel, npar)
                part = 0 if ns == 1 else 5 * ns * nsel * nsens * npar * 4 * 8
                assert q(sid, 5, nz, nb, nsel, nsens, npar) == rec + lai + leaf + part, (scheme, nz, nb, nsel, nsens, npar)
    assert _slices(300, 2, 5) == 2 and _slices(300, 9, 5) == 3 and _slices(300, 16, 5) == 5 and _slices(2151, 2, 5) == 9
    for bad in ((42, 5, 20, 8, 2, 3, 4), (-1, 5, 20, 8, 2, 3, 4), (0, 0, 20, 8, 2, 3, 4), (0, 5, 0, 8, 2, 3, 4), (0, 5, 20, 0, 2, 3, 4),
                (0, 5, 20, 8, 0, 3, 4), (0, 5, 20, 8, 65, 3, 4), (0, -3, 20, 8, 2, 3, 4), (0, 5, 20, 8, 2, 0, 4), (0, 5, 20, 8, 2, 65, 4),
                (0, 5, 20, 8, 2, 3, 0), (0, 5, 20, 8, 2, 3, 11)):
        assert q(*bad) == 0, bad


def test_sensjac_plan_python_errors_need_no_device():
    import numpy as np
    import torch

    from crt1d_amd import batched

    assert batched.SENSJAC_SCHEMES == ("2s", "bl", "g77", "bf")
    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    d2, d3 = np.ones((2, 8)), np.ones((5, 3, 8))
    for make in (batched.SensorJacPlan, batched.sensor_jacobian):
        with pytest.raises(ValueError, match="unknown scheme"):
            make("nope", None, None, (0,), sens)
        with pytest.raises(ValueError, match="invalid `method`"):
            make("2s", None, None, (0,), sens, tau_d_method="nope")
        for scheme in ("4s", "zq_pa"):
            with pytest.raises(ValueError, match="has no sensor Jacobian"):
                make(scheme, None, None, (0,), sens)
        for scheme in ("2s", "n79"):
            with pytest.raises(ValueError, match="keys must be distinct"):
                make(scheme, None, None, (0,), sens, keys=("x0",))
            with pytest.raises(TypeError, match="sensors must be a SensorSet"):
                make(scheme, None, None, (0,), np.ones((2, 8)))
            with pytest.raises(TypeError, match="tangent must be a LeafTangent"):
                make(scheme, None, None, (0,), sens, tangent=np.ones(3))
            with pytest.raises(ValueError, match="must share ntan"):  # mismatched ntan
                make(scheme, None, None, (0,), sens, d_leaf_r=d2, d_soil_r=d3)
            with pytest.raises(ValueError, match=r"must be \(ntan, nb\) or \(ncol, ntan, nb\)"):
                make(scheme, None, None, (0,), sens, d_leaf_t=np.ones(8))
            with pytest.raises(ValueError, match="one call takes"):
                make(scheme, None, None, (0,), sens, d_leaf_t=np.ones((9, 8)))
            with pytest.raises(ValueError, match="no parameter at all"):
                make(scheme, None, None, (0,), sens, lai=False)

    class FakeBands:  # (what the plan looks at before it touches a column or a device)
        dtype = torch.float32

    for scheme in ("2s", "zq"):
        with pytest.raises(TypeError, match="no f32 storage form"):
            batched.SensorJacPlan(scheme, None, FakeBands(), (0,), sens)


def test_gauss_newton_step_on_the_host():
    """delta solves (J^T J + damping diag(J^T J)) delta = -J^T r per column; a zero Jacobian column gives delta = 0 there."""
    import numpy as np
    import torch

    from crt1d_amd import batched

    rng = np.random.default_rng(2)
    J = torch.as_tensor(rng.normal(size=(6, 9, 4)) * np.array([1.0, 1e3, 1e-3, 7.0]))
    r = torch.as_tensor(rng.normal(size=(6, 9)))
    for damping in (0.0, 0.5):
        A = torch.einsum("coi,coj->cij", J, J)
        A = A + damping * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        ref = np.stack([np.linalg.solve(A[c].numpy(), -(J[c].T @ r[c]).numpy()) for c in range(6)])
        got = batched.gauss_newton_step(J, r, damping=damping).numpy()
        assert got.shape == (6, 4)
        assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref).max(axis=1, keepdims=True))  # cond(scaled normal matrix) ~ 1e2: far inside
    J0 = J.clone()
    J0[:, :, 2] = 0.0
    got = batched.gauss_newton_step(J0, r)
    keep = [0, 1, 3]
    assert bool((got[:, 2] == 0).all())
    assert torch.allclose(got[:, keep], batched.gauss_newton_step(J0[:, :, keep], r), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="J must be"):
        batched.gauss_newton_step(J, r[:, :3])
    with pytest.raises(ValueError, match="damping"):
        batched.gauss_newton_step(J, r, damping=-1.0)
