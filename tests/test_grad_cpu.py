"""CPU: the gradient entry points (include/crt1d_hip_grad.h) exist next to an unchanged crt1d_hip.h, the structs match the header, every
argument error and every scheme that is not served is found before any launch in the precedence of crt_hip_levels_dleaf_f64 (fake device
pointers, as tests/test_dleaf_cpu.py), the workspace query, and the Python errors of LevelsGradPlan / solve_levels_ad that need no
device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf"]
NOT_SERVED = ["n79", "zq", "4s", "zq_pa"]
NAMES = ["crt_hip_levels_grad_f64", "crt_hip_levels_grad_workspace_bytes"]
W_KEYS = ["I_dr", "I_df_d", "I_df_u", "F"]
O_KEYS = ["leaf_r", "leaf_t", "soil_r", "lai", "leaf"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "crt1d_hip_grad.h")).read()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_grad_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_grad.h")
    assert names == sorted(_lib.GRAD_EXPORTS) == sorted(_lib._GRAD_SIGNATURES) == NAMES
    for name in names:
        assert hasattr(lib, name)
        for other in (_lib.EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS):
            assert name not in other
    # the argument counts of the table are those of the header
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, (_, argtypes) in _lib._GRAD_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    # crt1d_hip.h keeps its symbol set and its version, the other derivative headers their sets
    assert _declared("crt1d_hip.h") == sorted(_lib.EXPORTS) and len(_lib.EXPORTS) == 57
    assert _declared("crt1d_hip_dleaf.h") == sorted(_lib.DLEAF_EXPORTS) and len(_lib.DLEAF_EXPORTS) == 4
    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.parametrize("struct,cname,keys", [("CrtGradWeights", "crt_grad_weights", W_KEYS), ("CrtGradOut", "crt_grad_out", O_KEYS)])
def test_struct_layout(struct, cname, keys):
    from crt1d_amd import _lib

    S = getattr(_lib, struct)
    assert ctypes.sizeof(S) == 8 * len(keys)
    assert [f[0] for f in S._fields_] == keys
    assert [getattr(S, k).offset for k in keys] == [8 * i for i in range(len(keys))]
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), _header(), re.S)
    assert re.findall(r"\*\s*(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == keys


def _args(nz=20, nb=8, ncol=2):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no
    workspace -> CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    w = _lib.CrtGradWeights(FAKE, FAKE, FAKE, FAKE)
    out = _lib.CrtGradOut(FAKE, FAKE, FAKE, FAKE, FAKE)
    tan = _lib.CrtLeafTangent(FAKE, FAKE, None)
    return c, b, o, w, out, tan


def _call(lib, scheme, c, b, o, levels, w, tan, out, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_levels_grad_f64(sid, ref(c), ref(b), ref(o), arr, n, ref(w), ref(tan), ref(out), ws, wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_grad_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, nz, nb = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, 20, 8
    c, b, o, w, out, tan = _args(nz, nb)

    def call(c=c, b=b, o=o, levels=(0, nz - 1), w=w, out=out, tan=tan, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, o, None if levels is None else list(levels), w, tan, out, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    sid = _lib.SCHEME_IDS[scheme]
    need = lib.crt_hip_levels_grad_workspace_bytes(sid, 2, nz, nb, 2)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS  # a short workspace
    assert call(ws=FAKE, wsb=lib.crt_hip_levels_dleaf_workspace_bytes(sid, 2, nz, nb, 2)) == WS  # the leaf-angle entry's does not do
    assert call(tan=_lib.CrtLeafTangent(FAKE, FAKE, FAKE)) == WS  # with dmla
    for one in range(4):  # any single weight is enough
        assert call(w=_lib.CrtGradWeights(*[FAKE if i == one else None for i in range(4)])) == WS
    for one in range(5):  # any single output is enough; only `leaf` needs the tangent
        only = _lib.CrtGradOut(*[FAKE if i == one else None for i in range(5)])
        assert call(out=only) == WS
        assert call(out=only, tan=None) == (BAD if one == 4 else WS)
    # the weights
    assert call(w=None) == BAD
    assert call(w=_lib.CrtGradWeights(None, None, None, None)) == BAD
    # the outputs
    assert call(out=None) == BAD
    assert call(out=_lib.CrtGradOut(None, None, None, None, None)) == BAD
    # `leaf` without a whole tangent
    assert call(tan=None) == BAD
    assert call(tan=_lib.CrtLeafTangent(None, FAKE, None)) == BAD
    assert call(tan=_lib.CrtLeafTangent(FAKE, None, FAKE)) == BAD
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
    assert call(b=_lib.CrtBands(nb, 0, FAKE, FAKE, FAKE, FAKE, FAKE)) == WS  # shared spectra
    assert call(b=_lib.CrtBands(0, 0, FAKE, FAKE, FAKE, FAKE, FAKE)) == BAD
    assert call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, None, FAKE, FAKE)) == BAD  # no leaf_r
    soilless = call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, None))
    assert soilless == (WS if scheme == "bl" else BAD)
    # CRT_ERR_SHAPE as crt_hip_levels_f64: nz < 2
    assert call(c=_args(1, nb)[0], levels=(0,)) == _lib.CRT_ERR_SHAPE
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == WS


@pytest.mark.parametrize("scheme", NOT_SERVED)
def test_grad_schemes_not_served(lib, scheme):
    """n79, zq, 4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors."""
    from crt1d_amd import _lib

    c, b, o, w, out, tan = _args()
    U, BAD = _lib.CRT_ERR_UNSUPPORTED, _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, o, [0, 19], w, tan, out) == U
    assert _call(lib, scheme, c, b, o, [0, 19], w, tan, out, ws=FAKE, wsb=1 << 30) == U
    assert _call(lib, scheme, c, b, o, [19, 0], w, tan, out) == BAD  # an argument error is still one
    assert _call(lib, scheme, c, b, o, [0, 19], None, tan, out) == BAD
    assert _call(lib, scheme, c, b, o, [0, 19], w, tan, None) == BAD
    assert _call(lib, scheme, c, b, o, [0, 19], w, None, out) == BAD
    assert _call(lib, scheme, c, None, o, [0, 19], w, tan, out) == BAD
    assert _call(lib, scheme, c, _lib.CrtBands(8, 8, FAKE, FAKE, None, FAKE, FAKE), o, [0, 19], w, tan, out, ws=FAKE, wsb=1 << 30) == BAD
    assert _call(lib, scheme, c, b, _lib.CrtOptions(0.501, 5, 0), [0, 19], w, tan, out) == BAD
    assert _call(lib, scheme, _args(1)[0], b, o, [0], w, tan, out) == _lib.CRT_ERR_SHAPE
    if scheme == "n79":
        assert _call(lib, scheme, _args(2)[0], b, o, [0, 1], w, tan, out) == _lib.CRT_ERR_SHAPE


def test_grad_workspace_query(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_levels_grad_workspace_bytes
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, nb)
            assert rec > 0
            lai = lib.crt_hip_levels_dlai_workspace_bytes(sid, 5, nz, nb, 2) - rec  # the two side records, as their own entries keep them
            leaf = lib.crt_hip_levels_dleaf_workspace_bytes(sid, 5, nz, nb, 2) - rec
            nslice = -(-nb // 256)
            assert q(sid, 5, nz, nb, 2) == q(sid, 5, nz, nb, 64) == rec + lai + leaf + 5 * nslice * 2 * 8, (scheme, nz, nb)
    bl = _lib.SCHEME_IDS["bl"]
    grow = [q(bl, 5, nz, 8, 2) - lib.crt_hip_workspace_bytes_nb(bl, 5, nz, 8) for nz in (20, 21, 150)]
    assert grow[1] - grow[0] == 5 * 2 * 8 and grow[2] > grow[1]  # bl: both side records hold a vector of nz
    for bad in ((42, 5, 20, 8, 2), (-1, 5, 20, 8, 2), (0, 0, 20, 8, 2), (0, 5, 0, 8, 2), (0, 5, 20, 0, 2), (0, 5, 20, 8, 0), (0, 5, 20, 8, 65),
                (0, -3, 20, 8, 2)):
        assert q(*bad) == 0, bad


def test_grad_plan_python_errors_need_no_device():
    import numpy as np
    import torch

    from crt1d_amd import batched

    assert batched.GRAD_SCHEMES == ("2s", "bl", "g77", "bf")
    assert batched.GRAD_WRT == ("leaf_r", "leaf_t", "soil_r", "lai", "leaf")
    w = {"F": None}
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.LevelsGradPlan("nope", None, None, (0,), w)
    with pytest.raises(ValueError, match="invalid `method`"):
        batched.LevelsGradPlan("2s", None, None, (0,), w, tau_d_method="nope")
    for scheme in ("4s", "zq_pa"):
        with pytest.raises(ValueError, match="has no gradient"):
            batched.LevelsGradPlan(scheme, None, None, (0,), w)
        with pytest.raises(ValueError, match="has no gradient"):
            batched.solve_levels_grad(scheme, None, None, (0,), w)
        with pytest.raises(ValueError, match="has no gradient"):
            batched.solve_levels_ad(scheme, None, None, (0,))
    for scheme in ("2s", "n79"):
        for wrt in (("x0",), ("lai", "lai"), (), ("I_dr",)):
            with pytest.raises(ValueError, match="keys must be distinct"):
                batched.LevelsGradPlan(scheme, None, None, (0,), w, wrt=wrt)
        for bad in (None, {}, {"I_d": None}, [1.0]):
            with pytest.raises(ValueError, match="weights must be a dict"):
                batched.LevelsGradPlan(scheme, None, None, (0,), bad)
            with pytest.raises(ValueError, match="weights must be a dict"):
                batched.solve_levels_grad(scheme, None, None, (0,), bad)
        with pytest.raises(ValueError, match="per must be"):
            batched.LevelsGradPlan(scheme, None, None, (0,), w, per="x")
        with pytest.raises(TypeError, match="tangent must be a LeafTangent"):
            batched.LevelsGradPlan(scheme, None, None, (0,), w, tangent=np.ones(3))
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.solve_levels_ad("nope", None, None, (0,))
    with pytest.raises(ValueError, match="invalid `method`"):
        batched.solve_levels_ad("2s", None, None, (0,), tau_d_method="nope")
    with pytest.raises(ValueError, match="keys must be distinct"):
        batched.solve_levels_ad("2s", None, None, (0,), keys=("I_d",))

    class FakeBands:  # (what solve_levels_ad looks at before it touches a device)
        I_dr0 = torch.ones(3, dtype=torch.float64)
        I_df0 = torch.ones(3, dtype=torch.float64, requires_grad=True)

    with pytest.raises(ValueError, match="I_df0 requires grad"):
        batched.solve_levels_ad("2s", None, FakeBands(), (0,))
