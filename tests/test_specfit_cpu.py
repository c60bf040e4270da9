"""CPU: the spectral-retrieval entry points (include/crt1d_hip_specfit.h) exist next to unchanged headers, the structs match the header,
every argument error of the two launching entries is found before any launch (fake device pointers, as tests/test_retrieve_cpu.py: a
valid call of crt_hip_spectral_normal_f64 stops at the workspace check, no valid call of the step is made), the schemes that are not
served, a configuration beyond the LDS, the workspace query against its formula, and the Python errors that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf"]
NOT_SERVED = ["n79", "zq", "4s", "zq_pa"]
NAMES = ["crt_hip_lm_step_normal_f64", "crt_hip_spectral_normal_f64", "crt_hip_spectral_normal_workspace_bytes"]
KEYS = ["I_dr", "I_df_d", "I_df_u", "F"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header(name="crt1d_hip_specfit.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared(header):
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header(header))))


def test_specfit_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_specfit.h")
    assert names == sorted(_lib.SPECFIT_EXPORTS) == sorted(_lib._SPECFIT_SIGNATURES) == NAMES
    tables = (("crt1d_hip.h", _lib.EXPORTS), ("crt1d_hip_leaf.h", _lib.LEAF_EXPORTS), ("crt1d_hip_spectra.h", _lib.SPECTRA_EXPORTS),
              ("crt1d_hip_sensor.h", _lib.SENSOR_EXPORTS), ("crt1d_hip_jac.h", _lib.JAC_EXPORTS), ("crt1d_hip_dlai.h", _lib.DLAI_EXPORTS),
              ("crt1d_hip_dleaf.h", _lib.DLEAF_EXPORTS), ("crt1d_hip_grad.h", _lib.GRAD_EXPORTS), ("crt1d_hip_sensjac.h", _lib.SENSJAC_EXPORTS),
              ("crt1d_hip_sensjac_series.h", _lib.SENSJAC_SERIES_EXPORTS), ("crt1d_hip_retrieve.h", _lib.RETRIEVE_EXPORTS))
    for name in names:
        assert hasattr(lib, name)
        for _, other in tables:
            assert name not in other
    for name, (_, argtypes) in _lib._SPECFIT_SIGNATURES.items():  # the argument counts of the table are those of the header
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    for header, table in tables:  # the other headers keep their symbol sets, crt1d_hip.h its version
        assert _declared(header) == sorted(table), header
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")) == sorted([h for h, _ in tables] + ["crt1d_hip_specfit.h"])


def _fields(struct):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S)
    names = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return names


def test_struct_layouts():
    from crt1d_amd import _lib

    def layout(S):
        return [f[0] for f in S._fields_], [getattr(S, f[0]).offset for f in S._fields_], ctypes.sizeof(S)

    names, offs, size = layout(_lib.CrtSpecObs)
    assert names == _fields("crt_spec_obs") == ["y_" + k for k in KEYS] + ["inv_sigma_" + k for k in KEYS]
    assert offs == [8 * i for i in range(8)] and size == 64
    names, offs, size = layout(_lib.CrtSpecNormalOut)
    assert names == _fields("crt_spec_normal_out") == ["A", "g", "c2"] + ["fwd_" + k for k in KEYS]
    assert offs == [8 * i for i in range(7)] and size == 56
    names, offs, size = layout(_lib.CrtLmNormalBlock)
    assert names == _fields("crt_lm_normal_block") == ["A", "g", "c2"] and offs == [0, 8, 16] and size == 24


def _args(nz=20, nb=8, ncol=2, ntan=2):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no workspace ->
    CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    dirs = _lib.CrtOpticsDirs(ntan, 0, FAKE, FAKE, FAKE)
    tan = _lib.CrtLeafTangent(FAKE, FAKE, None)
    obs = _lib.CrtSpecObs(None, None, FAKE, None, None, None, FAKE, None)  # I_df_u with weights
    out = _lib.CrtSpecNormalOut(FAKE, FAKE, FAKE, None, None, None, None)
    return c, b, o, dirs, tan, obs, out


def _call(lib, scheme, c, b, o, levels, dirs, lai, tan, obs, out, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_spectral_normal_f64(sid, ref(c), ref(b), ref(o), arr, n, ref(dirs), lai, ref(tan), ref(obs), ref(out), ws, wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_spectral_normal_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, U, nz, nb = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, _lib.CRT_ERR_UNSUPPORTED, 20, 8
    c, b, o, dirs, tan, obs, out = _args(nz, nb)

    def call(c=c, b=b, o=o, levels=(0, nz - 1), dirs=dirs, lai=1, tan=tan, obs=obs, out=out, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, o, None if levels is None else list(levels), dirs, lai, tan, obs, out, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    need = lib.crt_hip_spectral_normal_workspace_bytes(_lib.SCHEME_IDS[scheme], 2, nz, nb, 2, 1, 4)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS
    # the observations: any single key is enough, none is an error; inv_sigma and fwd of a key that is not observed are not looked at
    for one in range(4):
        assert call(obs=_lib.CrtSpecObs(*[FAKE if i == one else None for i in range(8)])) == WS
    assert call(obs=_lib.CrtSpecObs(*[FAKE] * 8)) == WS
    assert call(obs=None) == BAD
    assert call(obs=_lib.CrtSpecObs(*[None] * 8)) == BAD
    assert call(obs=_lib.CrtSpecObs(None, None, None, None, FAKE, FAKE, FAKE, FAKE)) == BAD  # weights without observations
    # the outputs
    assert call(out=None) == BAD
    for hole in range(3):  # NULL A, g, c2
        assert call(out=_lib.CrtSpecNormalOut(*[None if i == hole else FAKE for i in range(3)], None, None, None, None)) == BAD
    assert call(out=_lib.CrtSpecNormalOut(*[FAKE] * 7)) == WS  # with fwd
    # the parameter axis: every column alone, none (npar = 0), ten and eleven
    assert call(lai=0, tan=None) == WS
    assert call(dirs=None, tan=None) == WS
    assert call(dirs=None, lai=0) == WS
    assert call(dirs=None, lai=0, tan=None) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(0, 0, FAKE, FAKE, FAKE), lai=0, tan=None) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN, 0, FAKE, FAKE, FAKE)) == WS  # npar = 10
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN + 1, 0, FAKE, FAKE, FAKE), lai=0) == BAD  # (npar = 10 would need nine directions)
    assert call(dirs=_lib.CrtOpticsDirs(_lib.SENSJAC_MAX_NTAN + 1, 0, FAKE, FAKE, FAKE)) == BAD  # npar = 11
    assert call(dirs=_lib.CrtOpticsDirs(-1, 0, FAKE, FAKE, FAKE)) == BAD
    for one in range(3):  # any single direction array is enough
        assert call(dirs=_lib.CrtOpticsDirs(2, 0, *[FAKE if i == one else None for i in range(3)])) == WS
    assert call(dirs=_lib.CrtOpticsDirs(2, 0, None, None, None)) == BAD
    assert call(dirs=_lib.CrtOpticsDirs(2, 2 * nb, FAKE, FAKE, FAKE)) == WS  # per column
    assert call(dirs=_lib.CrtOpticsDirs(2, nb, FAKE, FAKE, FAKE)) == BAD  # col_stride neither 0 nor ntan * nb
    # a tangent must be whole
    assert call(tan=_lib.CrtLeafTangent(None, FAKE, None)) == BAD
    assert call(tan=_lib.CrtLeafTangent(FAKE, None, FAKE)) == BAD
    assert call(tan=_lib.CrtLeafTangent(FAKE, FAKE, FAKE)) == WS
    assert call(tan=_lib.CrtLeafTangent(None, None, None)) == BAD
    # the rest of the parameter-axis parse: without a direction (ntan = 0) neither the stride nor the pointers are looked at; any with_lai
    # but 0 counts as set; sizes that are not positive are an argument error
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None)) == WS
    assert call(dirs=_lib.CrtOpticsDirs(0, 5, None, None, None), lai=0, tan=None) == BAD
    assert call(dirs=None, lai=2, tan=None) == WS
    assert call(c=_lib.CrtColumns(0, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)) == BAD
    assert call(c=_lib.CrtColumns(2, 0, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), levels=(0,)) == BAD
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
    assert call(o=_lib.CrtOptions(0.501, 5, 0)) == BAD
    assert call(b=_lib.CrtBands(nb, nb - 1, FAKE, FAKE, FAKE, FAKE, FAKE)) == BAD
    assert call(b=_lib.CrtBands(0, 0, FAKE, FAKE, FAKE, FAKE, FAKE)) == BAD
    assert call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, None, FAKE, FAKE)) == BAD  # no leaf_r
    assert call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, None)) == (WS if scheme == "bl" else BAD)
    assert call(c=_args(1, nb)[0], levels=(0,)) == _lib.CRT_ERR_SHAPE
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == WS
    # CRT_ERR_UNSUPPORTED after the workspace check: nkey * nsel * (npar + 1) rows of 64 doubles beyond the LDS.  npar = 4, one key: 5 rows
    # per level, 62 levels = 310 rows fit, 63 = 315 do not; two keys: 31 levels = 310 fit, 32 = 320 do not
    big = 1 << 30
    two = _lib.CrtSpecObs(None, FAKE, FAKE, None, None, None, None, None)
    assert call(c=c100, levels=range(62), ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(63), ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(63), ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(31), obs=two, ws=FAKE, wsb=0) == WS
    assert call(c=c100, levels=range(32), obs=two, ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(64), obs=_lib.CrtSpecObs(*[FAKE] * 8), ws=FAKE, wsb=big) == U
    assert call(c=c100, levels=range(63), ws=FAKE, wsb=big, out=None) == BAD  # (an argument error is still one)


@pytest.mark.parametrize("scheme", NOT_SERVED)
def test_spectral_normal_schemes_not_served(lib, scheme):
    """n79, zq, 4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors."""
    from crt1d_amd import _lib

    c, b, o, dirs, tan, obs, out = _args()
    U, BAD = _lib.CRT_ERR_UNSUPPORTED, _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, o, [0, 19], dirs, 1, tan, obs, out) == U
    assert _call(lib, scheme, c, b, o, [0, 19], dirs, 1, tan, obs, out, ws=FAKE, wsb=1 << 30) == U
    assert _call(lib, scheme, c, b, o, [19, 0], dirs, 1, tan, obs, out) == BAD  # an argument error is still one
    assert _call(lib, scheme, c, b, o, [0, 19], dirs, 1, tan, None, out) == BAD
    assert _call(lib, scheme, c, b, o, [0, 19], dirs, 1, tan, obs, None) == BAD
    assert _call(lib, scheme, c, b, o, [0, 19], None, 0, None, obs, out) == BAD
    assert _call(lib, scheme, _args(1)[0], b, o, [0], dirs, 1, tan, obs, out) == _lib.CRT_ERR_SHAPE


def _slices(nb, nsel, nkey, npar):
    """Band slices of k_spec_normal: the widest of 256, 128, 64 lanes whose nkey * nsel * (npar + 1) rows fit 160 KB less 4 KB."""
    w = 256
    while w >= 64 and nkey * nsel * (npar + 1) * w * 8 > 160 * 1024 - 4096:
        w //= 2
    w = max(w, 64)  # (none fits: the query sizes 64-lane slices, the call refuses)
    return -(-nb // w)


def test_spectral_normal_workspace_query(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_spectral_normal_workspace_bytes
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, nb)
            assert rec > 0
            lai = lib.crt_hip_levels_dlai_workspace_bytes(sid, 5, nz, nb, 2) - rec  # the two side records, as their own entries keep them
            leaf = lib.crt_hip_levels_dleaf_workspace_bytes(sid, 5, nz, nb, 2) - rec
            for nsel, nkey, npar in ((1, 1, 5), (2, 1, 1), (2, 4, 5), (9, 2, 5), (16, 1, 10), (64, 1, 3), (64, 4, 10)):
                ns = _slices(nb, nsel, nkey, npar)
                part = 0 if ns == 1 else 5 * ns * ((npar + 1) * (npar + 2) // 2) * 8
                assert q(sid, 5, nz, nb, nsel, nkey, npar) == rec + lai + leaf + part, (scheme, nz, nb, nsel, nkey, npar)
    assert _slices(300, 1, 1, 5) == 2 and _slices(300, 2, 4, 5) == 2 and _slices(300, 16, 1, 10) == 5 and _slices(2151, 1, 1, 5) == 9
    assert _slices(300, 9, 2, 5) == 3 and _slices(64, 64, 4, 10) == 1
    for bad in ((42, 5, 20, 8, 2, 1, 4), (-1, 5, 20, 8, 2, 1, 4), (0, 0, 20, 8, 2, 1, 4), (0, 5, 0, 8, 2, 1, 4), (0, 5, 20, 0, 2, 1, 4),
                (0, 5, 20, 8, 0, 1, 4), (0, 5, 20, 8, 65, 1, 4), (0, -3, 20, 8, 2, 1, 4), (0, 5, 20, 8, 2, 0, 4), (0, 5, 20, 8, 2, 5, 4),
                (0, 5, 20, 8, 2, 1, 0), (0, 5, 20, 8, 2, 1, 11)):
        assert q(*bad) == 0, bad


def _problem(**kw):
    from crt1d_amd import _lib

    d = dict(ncol=3, npar=5, lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0, lo=None, hi=None, prior=None,
             inv_sigma_prior=None)
    d.update(kw)
    return _lib.CrtLmProblem(*[d[f[0]] for f in _lib.CrtLmProblem._fields_])


def _blocks(*blocks):
    from crt1d_amd import _lib

    return (_lib.CrtLmNormalBlock * max(len(blocks), 1))(*[_lib.CrtLmNormalBlock(*b) for b in blocks])


def test_lm_step_normal_validation_without_gpu(lib):
    """Every one of these is CRT_ERR_BAD_ARG and launches nothing (the pointers are fake: a launch would fault on a GPU machine)."""
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG
    state = _lib.CrtLmState(*[FAKE] * 9)
    good = (FAKE, FAKE, FAKE)
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731

    def call(prob=_problem(), blocks=_blocks(good), nblk=1, st=state):
        return lib.crt_hip_lm_step_normal_f64(ref(prob), blocks, nblk, ref(st), None)

    assert call(prob=None) == BAD
    assert call(blocks=None) == BAD
    assert call(st=None) == BAD
    for npar in (0, -1, _lib.RETRIEVE_MAX_NPAR + 1):
        assert call(prob=_problem(npar=npar)) == BAD
    assert call(prob=_problem(ncol=0)) == BAD
    for nblk in (0, -1, _lib.LM_MAX_BLOCKS + 1):
        assert call(blocks=_blocks(*[good] * 5), nblk=nblk) == BAD
    for hole in range(3):  # NULL A, g, c2
        assert call(blocks=_blocks(tuple(None if i == hole else v for i, v in enumerate(good)))) == BAD
        assert call(blocks=_blocks(good, good, tuple(None if i == hole else v for i, v in enumerate(good))), nblk=3) == BAD
    nan = float("nan")
    for kw in (dict(lam_up=1.0), dict(lam_up=0.5), dict(lam_up=nan), dict(lam_down=0.0), dict(lam_down=-0.1), dict(lam_down=1.5),
               dict(lam_down=nan), dict(xtol=-1e-9), dict(ftol=-1e-9), dict(xtol=nan), dict(ftol=nan), dict(lam_min=-1.0),
               dict(lam_min=2.0, lam_max=1.0), dict(prior=FAKE), dict(inv_sigma_prior=FAKE)):
        assert call(prob=_problem(**kw)) == BAD, kw
    for hole in range(9):  # a NULL state array
        assert call(st=_lib.CrtLmState(*[None if i == hole else FAKE for i in range(9)])) == BAD


def test_spectral_plans_python_errors_need_no_device():
    import numpy as np
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    assert batched.SPECTRAL_RETRIEVE_SCHEMES == ("2s", "bl", "g77", "bf") and batched.SPECFIT_MAX_ROWS == 312
    y = {"I_df_u": np.ones((3, 1, 8))}

    class FakeBands:  # (what the plans look at before they touch a column or a device)
        dtype = torch.float32
        nb = 8

    class FakeCols:
        ncol, nz, device = 3, 6, "nowhere"

    class F64Bands(FakeBands):
        dtype = torch.float64

    for make in (batched.SpectralNormalPlan, batched.spectral_normal, batched.SpectralRetrievalPlan, batched.retrieve_spectral):
        with pytest.raises(ValueError, match="unknown scheme"):
            make("nope", None, None, (0,), y, keys=("I_df_u",))
        for scheme in ("n79", "zq", "4s", "zq_pa"):
            with pytest.raises(ValueError, match="has no spectral retrieval"):
                make(scheme, None, None, (0,), y, keys=("I_df_u",))
        with pytest.raises(ValueError, match="invalid `method`"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), tau_d_method="nope")
        with pytest.raises(ValueError, match="keys must be distinct"):
            make("2s", None, None, (0,), y, keys=("x0",))
        with pytest.raises(ValueError, match="which are not in keys"):
            make("2s", None, None, (0,), y, keys=("F",))
        with pytest.raises(ValueError, match="which are not in keys"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), inv_sigma={"F": np.ones((3, 1, 8))})
        with pytest.raises(ValueError, match="y lacks the keys"):
            make("2s", None, None, (0,), y, keys=("I_df_u", "F"))
        with pytest.raises(TypeError, match="y must be a dict"):
            make("2s", None, None, (0,), np.ones((3, 1, 8)), keys=("I_df_u",))
        with pytest.raises(ValueError, match=r"must be \(ncol, nsel, nb\)"):  # a wrong rank
            make("2s", None, None, (0,), {"I_df_u": np.ones((3, 8))}, keys=("I_df_u",))
        with pytest.raises(ValueError, match="must share one shape"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), inv_sigma={"I_df_u": np.ones((3, 1, 7))})
        with pytest.raises(ValueError, match="one call takes"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), d_leaf_r=np.ones((9, 8)))
        with pytest.raises(TypeError, match="no f32 storage form"):
            make("2s", None, FakeBands(), (0,), y, keys=("I_df_u",))
        for bad in (np.ones((3, 2, 8)), np.ones((2, 1, 8)), np.ones((3, 1, 9))):  # a wrong y shape: against (ncol, nsel, nb) = (3, 1, 8)
            with pytest.raises(ValueError, match=r"y\['I_df_u'\] must be \(3, 1, 8\)"):
                make("2s", FakeCols(), F64Bands(), (0,), {"I_df_u": bad}, keys=("I_df_u",))
    for make in (batched.SpectralNormalPlan, batched.spectral_normal):
        with pytest.raises(ValueError, match="no parameter at all"):  # npar == 0
            make("2s", None, None, (0,), y, keys=("I_df_u",), lai=False)
        with pytest.raises(TypeError, match="tangent must be a LeafTangent"):
            batched.SpectralNormalPlan("2s", None, None, (0,), y, keys=("I_df_u",), tangent=np.ones(3))
    for make in (batched.SpectralRetrievalPlan, batched.retrieve_spectral):
        with pytest.raises(ValueError, match="no parameter at all"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), lai=False, leaf=False)
        for bound in ("lo", "hi"):
            with pytest.raises(ValueError, match=bound + r" must be \(npar,\) = \(4,\)"):
                make("2s", None, None, (0,), y, keys=("I_df_u",), d_leaf_r=np.ones((2, 8)), leaf=True, **{bound: np.zeros(3)})
        with pytest.raises(ValueError, match="lam_up > 1"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), lam_up=1.0)
        with pytest.raises(TypeError, match="unknown options"):
            make("2s", None, None, (0,), y, keys=("I_df_u",), lam_sideways=2.0)
    with pytest.raises(ValueError, match="exceeds 312"):  # 1 key, 64 levels, npar = 4: 320 rows
        class Deep(FakeCols):
            nz = 100
        batched.SpectralNormalPlan("2s", Deep(), F64Bands(), tuple(range(64)), {"I_df_u": np.ones((3, 64, 8))}, keys=("I_df_u",),
                                   d_leaf_r=np.ones((3, 8)))
    for scheme in ("4s", "n79"):
        with pytest.raises(ValueError, match="has no spectral retrieval"):
            Model(scheme, nlayers=6).retrieve_spectral({"I_df_u": np.ones((1, 8))})
