"""CPU: the masked entries and the accept decision (include_mask/crt1d_hip_masked.h; ``skip=`` on the inner plans, ``evaluate=`` and
``check_every=`` on the retrieval plans).

1. The header against the ctypes table: names, argument counts (the sibling's plus one), the struct layout; no other table holds the
   names; include_mask/ holds this one header; the 57 names and ABI 3 stay.
2. Every status of the seven entries that is found before a launch, from calls with fake device pointers: a masked entry answers what its
   sibling answers on the same arguments (the precedence is the sibling's), a bad unit is CRT_ERR_BAD_ARG, a NULL mask or a NULL skip is
   the sibling, the schemes without masked kernels are CRT_ERR_UNSUPPORTED behind the argument errors and whatever the workspace.
3. The device-free ValueErrors of ``skip=``, ``skip_unit=``, ``evaluate=`` and ``check_every=``."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf"]
NOT_SERVED = ["n79", "zq", "4s", "zq_pa"]
SIBLING = {"crt_hip_sensor_jac_masked_f64": "crt_hip_sensor_jac_f64",
           "crt_hip_sensor_jac_series_masked_f64": "crt_hip_sensor_jac_series_f64",
           "crt_hip_sensor_levels_masked_f64": "crt_hip_sensor_levels_f64",
           "crt_hip_sensor_levels_series_masked_f64": "crt_hip_sensor_levels_series_f64",
           "crt_hip_spectral_normal_masked_f64": "crt_hip_spectral_normal_f64",
           "crt_hip_spectral_normal_series_masked_f64": "crt_hip_spectral_normal_series_f64"}
NAMES = sorted(list(SIBLING) + ["crt_hip_lm_decide_f64"])


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    raw = open(os.path.join(ROOT, "include_mask", "crt1d_hip_masked.h")).read()
    return re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.MASKED_EXPORTS) == sorted(_lib._MASKED_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS, _lib.LEAFMODEL_EXPORTS, _lib.LUT_EXPORTS, _lib.LUT_POSTERIOR_EXPORTS, _lib.CHAIN_EXPORTS,
              _lib.SHARED_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    tables = {**_lib._SENSOR_SIGNATURES, **_lib._SENSJAC_SIGNATURES, **_lib._SENSJAC_SERIES_SIGNATURES, **_lib._SPECFIT_SIGNATURES,
              **_lib._SPECFIT_SERIES_SIGNATURES}
    for name, (restype, argtypes) in _lib._MASKED_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
        assert restype is ctypes.c_int
        if name in SIBLING:  # the sibling's arguments and a trailing mask
            assert argtypes[:-1] == tables[SIBLING[name]][1] and argtypes[-1] is ctypes.POINTER(_lib.CrtColMask)
            assert re.search(r"const crt_col_mask\*\s*mask\s*$", m.group(1).strip())
    mask = os.path.join(ROOT, "include_mask")
    assert sorted(os.path.relpath(os.path.join(d, f), mask) for d, _, files in os.walk(mask) for f in files) == ["crt1d_hip_masked.h"]
    assert _header().count("typedef struct") == 1
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_struct_layout():
    from crt1d_amd import _lib

    m = re.search(r"typedef struct crt_col_mask \{(.*?)\} crt_col_mask;", _header(), re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "const int32_t* skip; int32_t unit;"
    S = _lib.CrtColMask
    assert [f[0] for f in S._fields_] == ["skip", "unit"] and [f[1] for f in S._fields_] == [ctypes.c_void_p, ctypes.c_int32]
    assert S.skip.offset == 0 and S.unit.offset == 8 and ctypes.sizeof(S) == 16
    assert _lib.LM_RUNNING == 0  # a status array serves as skip


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def _sens(first, count, w=FAKE):
    from crt1d_amd import _lib

    n = len(first)
    f, k = (ctypes.c_int32 * max(n, 1))(*first), (ctypes.c_int32 * max(n, 1))(*count)
    s = _lib.CrtSensorSet(n, f, k, w)
    s._keep = (f, k)
    return s


def _base(ncol=6, nz=20, nb=8, nt=3):
    """The arguments of every entry, with device pointers that are never dereferenced on the host: a valid call gets as far as the
    workspace check (no workspace: CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    return dict(c=_lib.CrtColumns(ncol, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE),
                sun=_lib.CrtSunSeries(nt, FAKE, None, nt * nb, FAKE, FAKE), o=_lib.CrtOptions(0.501, 0, 0), levels=(0, nz - 1),
                sens=_sens([0, 2, 0], [3, 1, nb]), dirs=_lib.CrtOpticsDirs(2, 0, FAKE, FAKE, FAKE), lai=1, tan=_lib.CrtLeafTangent(FAKE, FAKE, None),
                tans=_lib.CrtLeafTangentSeries(FAKE, FAKE, None), sout=_lib.CrtSensorOut(FAKE, FAKE, FAKE, FAKE),
                jout=_lib.CrtSensJacOut(FAKE, FAKE, FAKE, FAKE), obs=_lib.CrtSpecObs(FAKE, None, FAKE, None, FAKE, None, None, None),
                nout=_lib.CrtSpecNormalOut(FAKE, FAKE, FAKE, None, None, None, None),
                nsout=_lib.CrtSpecSeriesOut(FAKE, FAKE, FAKE, None, None, None, None, None, None, None), ws=None, wsb=0)


def _call(lib, name, scheme, a, mask="none"):
    """``name``: a masked entry; mask == "none": its plain sibling on the same arguments."""
    from crt1d_amd import _lib

    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    lev = None if a["levels"] is None else (ctypes.c_int32 * max(len(a["levels"]), 1))(*a["levels"])
    n = 0 if a["levels"] is None else len(a["levels"])
    sid = _lib.SCHEME_IDS[scheme]
    series = "series" in name
    head = (sid, ref(a["c"]), ref(a["b"])) + ((ref(a["sun"]),) if series else ()) + (ref(a["o"]), lev, n)
    if "sensor_levels" in name:
        mid = (ref(a["sens"]), ref(a["sout"]))
    elif "sensor_jac" in name:
        mid = (ref(a["sens"]), ref(a["dirs"]), a["lai"], ref(a["tans"] if series else a["tan"]), ref(a["jout"]))
    else:
        mid = (ref(a["dirs"]), a["lai"], ref(a["tans"] if series else a["tan"]), ref(a["obs"]), ref(a["nsout"] if series else a["nout"]))
    args = head + mid + (a["ws"], a["wsb"], None)
    if isinstance(mask, str):
        return getattr(lib, SIBLING[name])(*args)
    return getattr(lib, name)(*args, ref(mask))


def _variants():
    """name -> changes of the base arguments: valid calls, argument errors of every group, a short workspace."""
    from crt1d_amd import _lib

    return {
        "valid": {}, "workspace": dict(ws=FAKE, wsb=64), "no columns": dict(c=None), "no bands": dict(b=None), "no levels": dict(levels=None),
        "descending levels": dict(levels=(19, 0)), "level beyond nz": dict(levels=(0, 20)),
        "ncol 0": dict(c=_lib.CrtColumns(0, 20, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)),
        "nz 1": dict(c=_lib.CrtColumns(6, 1, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), levels=(0,)),
        "no psi": dict(c=_lib.CrtColumns(6, 20, None, FAKE, FAKE, FAKE, FAKE, None, None)),
        "nb 0": dict(b=_lib.CrtBands(0, 0, FAKE, FAKE, FAKE, FAKE, FAKE)), "no leaf_r": dict(b=_lib.CrtBands(8, 8, FAKE, FAKE, None, FAKE, FAKE)),
        "no sensors": dict(sens=None), "empty support": dict(sens=_sens([0], [0])), "no outputs": dict(sout=None, jout=None, nout=None, nsout=None),
        "empty outputs": dict(sout=_lib.CrtSensorOut(None, None, None, None), jout=_lib.CrtSensJacOut(None, None, None, None),
                              nout=_lib.CrtSpecNormalOut(None, FAKE, FAKE, None, None, None, None),
                              nsout=_lib.CrtSpecSeriesOut(FAKE, None, FAKE, None, None, None, None, None, None, None)),
        "no directions": dict(dirs=_lib.CrtOpticsDirs(2, 0, None, None, None)), "bad stride": dict(dirs=_lib.CrtOpticsDirs(2, 8, FAKE, FAKE, FAKE)),
        "half a tangent": dict(tan=_lib.CrtLeafTangent(None, FAKE, None), tans=_lib.CrtLeafTangentSeries(FAKE, None, None)),
        "no observations": dict(obs=None), "no sun": dict(sun=None), "nt 0": dict(sun=_lib.CrtSunSeries(0, FAKE, None, 0, FAKE, FAKE)),
        "bad option": dict(o=_lib.CrtOptions(0.501, 7, 0)),
    }


@pytest.mark.parametrize("name", sorted(SIBLING))
def test_masked_entries_validate_as_their_siblings(lib, name):
    from crt1d_amd import _lib

    BAD, WS, U = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, _lib.CRT_ERR_UNSUPPORTED
    ok1, ok3, ok6 = _lib.CrtColMask(FAKE, 1), _lib.CrtColMask(FAKE, 3), _lib.CrtColMask(FAKE, 6)
    seen = set()
    for scheme in SERVED:
        for label, change in _variants().items():
            a = dict(_base(), **change)
            want = _call(lib, name, scheme, a)
            seen.add(want)
            for mask in (None, _lib.CrtColMask(None, 0), _lib.CrtColMask(None, -5), ok1, ok3, ok6):  # no mask, no skip (unit not looked at), masks
                assert _call(lib, name, scheme, a, mask) == want, (scheme, label)
            for unit in (0, -1, 4, 5, 7, 12):  # unit < 1 or ncol % unit != 0: an argument error, in front of CRT_ERR_SHAPE / _WORKSPACE
                got = _call(lib, name, scheme, a, _lib.CrtColMask(FAKE, unit))
                assert got == BAD, (scheme, label, unit)
    assert {BAD, WS, _lib.CRT_ERR_SHAPE} <= seen  # the variants reach the three of them
    a = _base()
    assert _call(lib, name, "2s", a) == WS and _call(lib, name, "2s", a, ok3) == WS
    for scheme in NOT_SERVED:  # an argument error is one for every scheme, then the scheme, whatever the workspace
        for mask in (None, ok1, ok3):
            assert _call(lib, name, scheme, a, mask) == U
            assert _call(lib, name, scheme, dict(a, ws=FAKE, wsb=1 << 40), mask) == U
            assert _call(lib, name, scheme, dict(a, levels=(19, 0)), mask) == BAD
            assert _call(lib, name, scheme, dict(a, c=None), mask) == BAD
        assert _call(lib, name, scheme, a, _lib.CrtColMask(FAKE, 4)) == BAD
        assert _call(lib, name, scheme, dict(a, c=_lib.CrtColumns(6, 1, FAKE, FAKE, FAKE, FAKE, FAKE, None, None), levels=(0,)), ok1) == _lib.CRT_ERR_SHAPE


def _problem(ncol=6, npar=3, **kw):
    from crt1d_amd import _lib

    o = dict(lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0, lo=None, hi=None, prior=None, inv_sigma_prior=None)
    o.update(kw)
    return _lib.CrtLmProblem(ncol, npar, *[o[k] for k in ("lam_up", "lam_down", "lam_min", "lam_max", "xtol", "ftol", "lo", "hi", "prior",
                                                           "inv_sigma_prior")])


def test_decide_validation_without_gpu(lib):
    """The argument errors of crt_hip_lm_step_f64, one by one, and the two outputs.  Nothing valid is called: it would launch."""
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    state = _lib.CrtLmState(*[FAKE] * 9)
    obs = lambda n=1, hole=None, nrow=5: (_lib.CrtLmObs * 4)(*[_lib.CrtLmObs(nrow, *[None if hole == (q, i) else FAKE for i in range(4)])  # noqa: E731
                                                               for q in range(min(n, 4))])

    def both(prob="default", blk="default", nblk=1, st=state, skip=FAKE, cost=FAKE, **kw):
        pr = _problem(**kw) if prob == "default" else prob
        b = obs(nblk) if blk == "default" else blk
        d = lib.crt_hip_lm_decide_f64(ref(pr), b, nblk, ref(st), skip, cost, None)
        s = lib.crt_hip_lm_step_f64(ref(pr), b, nblk, ref(st), None)
        return d, s

    cases = [dict(prob=None), dict(blk=None), dict(st=None), dict(ncol=0), dict(npar=0), dict(npar=11), dict(nblk=0), dict(nblk=5),
             dict(blk=obs(1, nrow=0)), dict(blk=obs(2, (1, 0)), nblk=2), dict(blk=obs(1, (0, 1))), dict(blk=obs(1, (0, 2))),
             dict(lam_up=1.0), dict(lam_up=float("nan")), dict(lam_down=0.0), dict(lam_down=1.5), dict(lam_min=-1.0), dict(lam_max=1e-13),
             dict(xtol=-1.0), dict(ftol=float("nan")), dict(prior=FAKE), dict(inv_sigma_prior=FAKE)]
    cases += [dict(st=_lib.CrtLmState(*[None if i == hole else FAKE for i in range(9)])) for hole in range(9)]
    for kw in cases:
        assert both(**kw) == (BAD, BAD), kw
    # the outputs: only the decision has them; and an error of the step wins nothing over them -- both are CRT_ERR_BAD_ARG
    pr, b = _problem(), obs(1)
    assert lib.crt_hip_lm_decide_f64(ref(pr), b, 1, ref(state), None, FAKE, None) == BAD
    assert lib.crt_hip_lm_decide_f64(ref(pr), b, 1, ref(state), FAKE, None, None) == BAD


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_python_errors_need_no_device():
    import torch

    from crt1d_amd import batched

    class Cols:
        ncol, nz, device = 6, 6, "nowhere"

    class Bands:
        dtype, nb = torch.float64, 8

    class Bands32:
        dtype, nb = torch.float32, 8

    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    ys = {"I_df_u": np.ones((6, 1, 8))}
    flags = torch.zeros(6, dtype=torch.int32)
    sun = object.__new__(batched.SunSeries)  # (its tensors would have to live on a device; the checks below come before they are read)
    sun.psi = torch.zeros((6, 2), dtype=torch.float64)
    yt = {"I_df_u": np.ones((6, 2, 1, 8))}
    inner = [lambda scheme="2s", bands=Bands(), **kw: batched.SensorLevelsPlan(scheme, Cols(), bands, (0,), sens, **kw),
             lambda scheme="2s", bands=Bands(), **kw: batched.SensorLevelsSeriesPlan(scheme, Cols(), bands, sun, (0,), sens, **kw),
             lambda scheme="2s", bands=Bands(), **kw: batched.SensorJacPlan(scheme, Cols(), bands, (0,), sens, **kw),
             lambda scheme="2s", bands=Bands(), **kw: batched.SensorJacSeriesPlan(scheme, Cols(), bands, sun, (0,), sens, **kw),
             lambda scheme="2s", bands=Bands(), **kw: batched.SpectralNormalPlan(scheme, Cols(), bands, (0,), ys, keys=("I_df_u",), **kw),
             lambda scheme="2s", bands=Bands(), **kw: batched.SpectralNormalSeriesPlan(scheme, Cols(), bands, sun, (0,), yt, keys=("I_df_u",), **kw)]
    for make in inner:
        for unit in (0, -1, 1.0, True, "1"):
            with pytest.raises(ValueError, match="skip_unit must be an integer >= 1"):
                make(skip=flags, skip_unit=unit)
        with pytest.raises(ValueError, match="skip_unit needs skip="):
            make(skip_unit=3)
        with pytest.raises(ValueError, match="skip must be an int32 torch tensor"):
            make(skip=np.zeros(6, dtype=np.int32))
        with pytest.raises(ValueError, match="skip must be an int32 torch tensor"):
            make(skip=torch.zeros(6, dtype=torch.int64))
        with pytest.raises(ValueError, match="skip_unit = 4 does not divide ncol = 6"):
            make(skip=flags, skip_unit=4)
        with pytest.raises(ValueError, match=r"skip must be a contiguous \(2,\) tensor"):
            make(skip=flags, skip_unit=3)
        with pytest.raises(ValueError, match=r"skip must be a contiguous \(6,\) tensor"):
            make(skip=torch.zeros(12, dtype=torch.int32)[::2])
    for make in inner[:2]:  # the sensor-level plans serve more schemes and float32 bands than the masked entries do
        with pytest.raises(ValueError, match="has no masked kernels"):
            make("n79", skip=flags)
        with pytest.raises(ValueError, match="has no masked kernels"):
            make("4s", skip=flags)
        with pytest.raises(ValueError, match="skip= needs float64 bands"):
            make(bands=Bands32(), skip=flags)
    for make in inner[2:4]:  # the composed Jacobians
        for scheme in ("n79", "zq"):
            with pytest.raises(ValueError, match="is composed of three calls: it takes no skip="):
                make(scheme, skip=flags)

    y1 = {"I_df_u": np.ones((6, 1, 1))}
    sensor = [lambda scheme="2s", **kw: batched.RetrievalPlan(scheme, Cols(), Bands(), (0,), sens, y1, keys=("I_df_u",), **kw),
              lambda scheme="2s", **kw: batched.retrieve(scheme, Cols(), Bands(), (0,), sens, y1, keys=("I_df_u",), **kw)]
    spectral = [lambda scheme="2s", **kw: batched.SpectralRetrievalPlan(scheme, Cols(), Bands(), (0,), ys, keys=("I_df_u",), **kw),
                lambda scheme="2s", **kw: batched.retrieve_spectral(scheme, Cols(), Bands(), (0,), ys, keys=("I_df_u",), **kw)]
    ch = dict(chain=3, inv_sigma_chain=np.ones((2, 1)))
    for make in sensor + spectral:
        for bad in ("none", None, "Running", 1):
            with pytest.raises(ValueError, match="evaluate must be one of"):
                make(evaluate=bad)
    for make in spectral:
        with pytest.raises(ValueError, match="evaluate='accepted' is not served by a spectral plan"):
            make(evaluate="accepted")
        with pytest.raises(ValueError, match="evaluate='accepted' is not served by a spectral plan"):
            make(evaluate="accepted", **ch)
    for make in sensor:
        with pytest.raises(ValueError, match="evaluate='accepted' is not served by a chained plan"):
            make(evaluate="accepted", **ch)
        for scheme in ("n79", "zq"):
            with pytest.raises(ValueError, match="evaluate='accepted' is not served by a composed plan"):
                make(scheme, evaluate="accepted")
            with pytest.raises(ValueError, match="evaluate='running' needs the masked kernels"):
                make(scheme, evaluate="running")
    assert batched.EVALUATE_MODES == ("all", "running", "accepted") and batched.MASKED_SCHEMES == tuple(SERVED)

    plan = object.__new__(batched.RetrievalPlan)  # run() checks check_every before it touches the plan
    for bad in (0, -3, 2.0, True, "4"):
        with pytest.raises(ValueError, match="check_every must be None or an integer >= 1"):
            plan.run(5, check_every=bad)
