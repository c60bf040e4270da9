"""CPU: the retrieval entry points (include/crt1d_hip_retrieve.h) exist next to unchanged headers, the structs match the header, every
argument error is found before any launch (fake device pointers, as tests/test_sensjac_cpu.py: no VALID call is made here, it would
launch), and the Python errors of RetrievalPlan / retrieve that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NAMES = ["crt_hip_lm_covariance_f64", "crt_hip_lm_step_f64", "crt_hip_retrieve_apply_f64"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header(name="crt1d_hip_retrieve.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared(header):
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header(header))))


def test_retrieve_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_retrieve.h")
    assert names == sorted(_lib.RETRIEVE_EXPORTS) == sorted(_lib._RETRIEVE_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS)
    for name in names:
        assert hasattr(lib, name)
        for other in others:
            assert name not in other
    for name, (_, argtypes) in _lib._RETRIEVE_SIGNATURES.items():  # the argument counts of the table are those of the header
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    assert _lib.RETRIEVE_MAX_NPAR == _lib.SENSJAC_MAX_NTAN + 2 == 10
    assert "#define CRT_RETRIEVE_MAX_NPAR (CRT_SENSJAC_MAX_NTAN + 2)" in _header()
    assert int(re.search(r"#define CRT_LM_MAX_BLOCKS (\d+)", _header()).group(1)) == _lib.LM_MAX_BLOCKS == 4
    enum = re.search(r"enum crt_lm_status \{(.*?)\}", _header(), re.S).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"CRT_(LM_\w+) = (\d+)", enum)) == {
        k: getattr(_lib, k) for k in ("LM_RUNNING", "LM_CONVERGED_X", "LM_CONVERGED_F", "LM_STALLED", "LM_FAILED_START")}
    # the other headers keep their symbol sets, crt1d_hip.h its version
    for header, table in (("crt1d_hip.h", _lib.EXPORTS), ("crt1d_hip_leaf.h", _lib.LEAF_EXPORTS), ("crt1d_hip_spectra.h", _lib.SPECTRA_EXPORTS),
                          ("crt1d_hip_sensor.h", _lib.SENSOR_EXPORTS), ("crt1d_hip_jac.h", _lib.JAC_EXPORTS),
                          ("crt1d_hip_dlai.h", _lib.DLAI_EXPORTS), ("crt1d_hip_dleaf.h", _lib.DLEAF_EXPORTS),
                          ("crt1d_hip_grad.h", _lib.GRAD_EXPORTS), ("crt1d_hip_sensjac.h", _lib.SENSJAC_EXPORTS),
                          ("crt1d_hip_sensjac_series.h", _lib.SENSJAC_SERIES_EXPORTS)):
        assert _declared(header) == sorted(table), header
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


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

    names, offs, size = layout(_lib.CrtRetrieveApply)
    assert names == _fields("crt_retrieve_apply")
    assert offs == [0, 4, 8, 12, 16, 20, 24] + [32 + 8 * i for i in range(11)] and size == 120
    names, offs, size = layout(_lib.CrtLmObs)
    assert names == _fields("crt_lm_obs") and offs == [0, 8, 16, 24, 32] and size == 40  # (int32, padding, four pointers)
    names, offs, size = layout(_lib.CrtLmProblem)
    assert names == _fields("crt_lm_problem") and offs == [0, 4] + [8 + 8 * i for i in range(10)] and size == 88
    names, offs, size = layout(_lib.CrtLmState)
    assert names == _fields("crt_lm_state") and offs == [8 * i for i in range(9)] and size == 72


def _problem(**kw):
    from crt1d_amd import _lib

    d = dict(ncol=3, npar=5, lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0, lo=None, hi=None, prior=None,
             inv_sigma_prior=None)
    d.update(kw)
    return _lib.CrtLmProblem(*[d[f[0]] for f in _lib.CrtLmProblem._fields_])


def _obs(*blocks):
    from crt1d_amd import _lib

    return (_lib.CrtLmObs * max(len(blocks), 1))(*[_lib.CrtLmObs(*b) for b in blocks])


def test_lm_step_validation_without_gpu(lib):
    """Every one of these is CRT_ERR_BAD_ARG and launches nothing (the pointers are fake: a launch would fault on a GPU machine)."""
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG
    state = _lib.CrtLmState(*[FAKE] * 9)
    good = (7, FAKE, FAKE, FAKE, None)
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731

    def call(prob=_problem(), obs=_obs(good), nblk=1, st=state):
        return lib.crt_hip_lm_step_f64(ref(prob), obs, nblk, ref(st), None)

    assert call(prob=None) == BAD
    assert call(obs=None) == BAD
    assert call(st=None) == BAD
    for npar in (0, -1, _lib.RETRIEVE_MAX_NPAR + 1):
        assert call(prob=_problem(npar=npar)) == BAD
    assert call(prob=_problem(ncol=0)) == BAD
    for nblk in (0, -1, _lib.LM_MAX_BLOCKS + 1):
        assert call(obs=_obs(*[good] * 5), nblk=nblk) == BAD
    assert call(obs=_obs((0, FAKE, FAKE, FAKE, None))) == BAD
    assert call(obs=_obs(good, (-3, FAKE, FAKE, FAKE, FAKE)), nblk=2) == BAD
    for hole in (1, 2, 3):  # NULL f, J, y
        assert call(obs=_obs(tuple(None if i == hole else v for i, v in enumerate(good)))) == BAD
        assert call(obs=_obs(good, good, tuple(None if i == hole else v for i, v in enumerate(good))), nblk=3) == BAD
    nan = float("nan")
    for kw in (dict(lam_up=1.0), dict(lam_up=0.5), dict(lam_up=nan), dict(lam_down=0.0), dict(lam_down=-0.1), dict(lam_down=1.5),
               dict(lam_down=nan), dict(xtol=-1e-9), dict(ftol=-1e-9), dict(xtol=nan), dict(ftol=nan), dict(lam_min=-1.0),
               dict(lam_min=2.0, lam_max=1.0), dict(prior=FAKE), dict(inv_sigma_prior=FAKE)):
        assert call(prob=_problem(**kw)) == BAD, kw
    for hole in range(9):  # a NULL state array
        assert call(st=_lib.CrtLmState(*[None if i == hole else FAKE for i in range(9)])) == BAD
    # the covariance entry
    cov = lib.crt_hip_lm_covariance_f64
    assert cov(0, 5, FAKE, FAKE, None) == BAD and cov(3, 0, FAKE, FAKE, None) == BAD and cov(3, 11, FAKE, FAKE, None) == BAD
    assert cov(3, 5, None, FAKE, None) == BAD and cov(3, 5, FAKE, None, None) == BAD


def test_apply_validation_without_gpu(lib):
    from crt1d_amd import _lib

    BAD, nb = _lib.CRT_ERR_BAD_ARG, 8
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731

    def call(dirs=_lib.CrtOpticsDirs(2, 0, FAKE, None, FAKE), **kw):
        d = dict(ncol=3, nz=6, nb=nb, npar=4, i_lai=2, i_leaf=3, base_stride=nb)
        d.update({k: FAKE for k in ("leaf_r0", "leaf_t0", "soil_r0", "lai0", "p", "leaf_r", "leaf_t", "soil_r", "lai_scale", "lai", "g_param")})
        d.update(kw)
        ap = _lib.CrtRetrieveApply(*[d[f[0]] for f in _lib.CrtRetrieveApply._fields_])
        return lib.crt_hip_retrieve_apply_f64(ref(ap), ref(dirs), None)

    assert lib.crt_hip_retrieve_apply_f64(None, None, None) == BAD
    for kw in (dict(ncol=0), dict(nz=0), dict(nb=0), dict(npar=0), dict(npar=11), dict(npar=3), dict(npar=5), dict(i_lai=0), dict(i_lai=3),
               dict(i_lai=-2), dict(i_leaf=2), dict(i_leaf=4), dict(i_lai=-1), dict(i_leaf=-1), dict(i_lai=-1, i_leaf=2, npar=4),
               dict(base_stride=4), dict(leaf_r0=None), dict(leaf_t0=None), dict(p=None), dict(leaf_r=None), dict(leaf_t=None),
               dict(soil_r0=None), dict(soil_r=None), dict(lai0=None), dict(lai=None), dict(lai_scale=None), dict(g_param=None)):
        assert call(**kw) == BAD, kw
    D = _lib.CrtOpticsDirs
    assert call(dirs=D(-1, 0, FAKE, FAKE, FAKE)) == BAD
    assert call(dirs=D(_lib.SENSJAC_MAX_NTAN + 1, 0, FAKE, FAKE, FAKE), npar=10, i_lai=9, i_leaf=-1) == BAD
    assert call(dirs=D(2, 0, None, None, None)) == BAD
    assert call(dirs=D(2, nb, FAKE, FAKE, FAKE)) == BAD  # col_stride neither 0 nor ntan * nb
    assert call(dirs=None) == BAD  # ntan = 0: i_lai = 2 and npar = 4 no longer fit
    assert call(dirs=D(3, 0, FAKE, FAKE, FAKE)) == BAD  # ntan = 3 likewise


def test_retrieval_plan_python_errors_need_no_device():
    import numpy as np
    import torch

    from crt1d_amd import batched

    assert batched.RETRIEVE_SCHEMES == ("2s", "bl", "g77", "bf", "n79", "zq")
    assert (batched.LM_RUNNING, batched.LM_CONVERGED_X, batched.LM_CONVERGED_F, batched.LM_STALLED, batched.LM_FAILED_START) == (0, 1, 2, 3, 4)
    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    y = {"I_df_u": np.ones((1, 1, 1))}

    class FakeBands:  # (what the plan looks at before it touches a column or a device)
        dtype = torch.float32

    for make in (batched.RetrievalPlan, batched.retrieve):
        with pytest.raises(ValueError, match="unknown scheme"):
            make("nope", None, None, (0,), sens, y, keys=("I_df_u",))
        for scheme in ("4s", "zq_pa"):
            with pytest.raises(ValueError, match="has no retrieval"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",))
        for scheme in ("2s", "n79"):
            with pytest.raises(ValueError, match="invalid `method`"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), tau_d_method="nope")
            with pytest.raises(ValueError, match="which are not in keys"):
                make(scheme, None, None, (0,), sens, y, keys=("F",))
            with pytest.raises(ValueError, match="which are not in keys"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), inv_sigma={"F": np.ones((1, 1, 1))})
            with pytest.raises(ValueError, match="y lacks the keys"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u", "F"))
            with pytest.raises(TypeError, match="sensors must be a SensorSet"):
                make(scheme, None, None, (0,), np.ones((2, 8)), y, keys=("I_df_u",))
            for bound in ("lo", "hi"):
                with pytest.raises(ValueError, match=bound + r" must be \(npar,\) = \(4,\)"):
                    make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), d_leaf_r=np.ones((2, 8)), leaf=True, **{bound: np.zeros(3)})
            with pytest.raises(ValueError, match="one call takes"):  # 9 directions: beyond the parameter limit, whatever else is retrieved
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), d_leaf_r=np.ones((9, 8)), leaf=True)
            with pytest.raises(ValueError, match="no parameter at all"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), lai=False)
            with pytest.raises(ValueError, match="lam_up > 1"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), lam_up=1.0)
            with pytest.raises(TypeError, match="unknown options"):
                make(scheme, None, None, (0,), sens, y, keys=("I_df_u",), lam_sideways=2.0)
            with pytest.raises(TypeError, match="no f32 storage form"):
                make(scheme, None, FakeBands(), (0,), sens, y, keys=("I_df_u",))
