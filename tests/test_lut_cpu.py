"""CPU: the look-up-table start of the retrievals (include_lut/crt1d_hip_lut.h; batched.lut_sample, LutTable, LutMatchPlan, ``p0=`` a table).

1. The header against the ctypes table: names, argument counts, struct layouts; the other tables keep their symbols.
2. Every CRT_ERR_BAD_ARG of the entry is found before any launch (fake device pointers); a valid call stops at the workspace check.
3. ``lut_sample``: shape, box, determinism, ``include`` first, the spread of the first 64 points of a 2-D box, infinite bounds.
4. The device-free errors of ``LutTable.build``, ``LutMatchPlan`` and ``p0=table``.
5. tests/lut_reference.py against a brute-force double loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import lut_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NAMES = ["crt_hip_lut_match_f64", "crt_hip_lut_match_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include_lut", "crt1d_hip_lut.h")).read(), flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.LUT_EXPORTS) == sorted(_lib._LUT_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS, _lib.LEAFMODEL_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    for name, (_, argtypes) in _lib._LUT_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    lut = os.path.join(ROOT, "include_lut")  # a directory of its own: include/ and include_ext/ are held to their lists elsewhere
    assert sorted(os.path.relpath(os.path.join(d, f), lut) for d, _, files in os.walk(lut) for f in files) == ["crt1d_hip_lut.h"]
    assert "#define CRT_LUT_MAX_BEST 8" in _header() and _lib.LUT_MAX_BEST == 8
    assert int(re.search(r"#define CRT_LUT_MAX_KSPLIT (\d+)", _header()).group(1)) == _lib.LUT_MAX_KSPLIT
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3  # crt1d_hip.h is what it was


def _fields(struct):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S)
    names = []
    for decl in m.group(1).split(";"):
        decl = re.sub(r"\[\w+\]", "", decl.strip())  # (arrays: the name)
        if decl:
            names += [re.sub(r"[\s*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return names


def test_struct_layouts():
    from crt1d_amd import _lib

    def layout(S):
        return [f[0] for f in S._fields_], [getattr(S, f[0]).offset for f in S._fields_], ctypes.sizeof(S)

    assert _lib.LM_MAX_BLOCKS == 4
    names, offs, size = layout(_lib.CrtLutTable)
    assert names == _fields("crt_lut_table") == ["ncand", "npar", "nblk", "nrow", "q", "m"]
    assert offs == [0, 4, 8, 12, 32, 40] and size == 72
    names, offs, size = layout(_lib.CrtLutObs)
    assert names == _fields("crt_lut_obs") == ["ncol", "y", "inv_sigma", "prior", "inv_sigma_prior"]
    assert offs == [0, 8, 40, 72, 80] and size == 88
    names, offs, size = layout(_lib.CrtLutOut)
    assert names == _fields("crt_lut_out") == ["nbest", "ksplit", "index", "cost", "p"]
    assert offs == [0, 4, 8, 16, 24] and size == 32


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def _args(ncand=100, npar=3, nblk=2, nrow=(5, 7), ncol=10, nbest=2, prior=True):
    from crt1d_amd import _lib

    i4, p4 = ctypes.c_int32 * 4, ctypes.c_void_p * 4
    ptrs = lambda n=nblk: p4(*[FAKE] * n)  # noqa: E731
    t = _lib.CrtLutTable(ncand, npar, nblk, i4(*nrow), FAKE, ptrs())
    o = _lib.CrtLutObs(ncol, ptrs(), ptrs(), FAKE if prior else None, FAKE if prior else None)
    out = _lib.CrtLutOut(nbest, 0, FAKE, FAKE, FAKE)
    return t, o, out


def test_validation_without_gpu(lib):
    """Every one of these is CRT_ERR_BAD_ARG and launches nothing (the pointers are fake: a launch would fault on a GPU machine); a valid
    call gets as far as the workspace check."""
    from crt1d_amd import _lib

    BAD, WS = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    i4, p4 = ctypes.c_int32 * 4, ctypes.c_void_p * 4

    def call(change=None, t=True, o=True, out=True, ws=None, wsb=0, **kw):
        T, O, U = _args(**kw)
        if change:
            change(T, O, U)
        return lib.crt_hip_lut_match_f64(ref(T) if t else None, ref(O) if o else None, ref(U) if out else None, ws, wsb, None)

    def setter(which, field, value):
        def change(T, O, U):
            setattr({"t": T, "o": O, "u": U}[which], field, value)
        return change

    assert call() == WS  # valid: nothing below is rejected for any other reason than the one named
    need = lib.crt_hip_lut_match_workspace_bytes(10, 100, 2)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS and call(ws=None, wsb=need) == WS
    assert call(prior=False) == WS and call(nblk=1, nrow=(1,)) == WS and call(nblk=4, nrow=(1, 2, 3, 4)) == WS
    assert call(setter("o", "inv_sigma", p4())) == WS  # NULL inv_sigma: ones
    assert call(setter("u", "p", None)) == WS  # p is optional
    for n in (1, 8):
        assert call(nbest=n) == WS
    assert call(npar=1) == WS and call(npar=10) == WS and call(ncand=1) == WS and call(ncol=1) == WS
    # NULL structs
    assert call(t=False) == BAD and call(o=False) == BAD and call(out=False) == BAD
    # sizes
    assert call(ncand=0) == BAD and call(ncand=-1) == BAD and call(ncol=0) == BAD
    assert call(npar=0) == BAD and call(npar=11) == BAD
    assert call(nblk=0, nrow=()) == BAD and call(setter("t", "nblk", 5)) == BAD
    assert call(nrow=(5, 0)) == BAD and call(nrow=(-1, 5)) == BAD
    assert call(nbest=0) == BAD and call(nbest=9) == BAD
    assert call(setter("u", "ksplit", -1)) == BAD
    # pointers
    assert call(setter("t", "q", None)) == BAD
    assert call(setter("t", "m", p4(FAKE, None))) == BAD and call(setter("t", "m", p4(None, FAKE))) == BAD
    assert call(setter("o", "y", p4(FAKE, None))) == BAD and call(setter("o", "y", p4())) == BAD
    assert call(setter("u", "index", None)) == BAD and call(setter("u", "cost", None)) == BAD
    assert call(setter("o", "prior", None)) == BAD and call(setter("o", "inv_sigma_prior", None)) == BAD
    # a block beyond nblk is not looked at
    assert call(nblk=1, nrow=(5, 0)) == WS
    del i4


def test_workspace_query(lib):
    q = lib.crt_hip_lut_match_workspace_bytes
    assert q(0, 10, 1) == 0 and q(10, 0, 1) == 0 and q(10, 10, 0) == 0 and q(10, 10, 9) == 0
    # many columns: no K-split, one list per column of 1, 4 or 8 entries of (double, int32)
    ncol = 64 * 1024
    assert q(ncol, 4096, 1) == ncol * 12 and q(ncol, 4096, 3) == ncol * 4 * 12 and q(ncol, 4096, 8) == ncol * 8 * 12
    # one column: as many parts as there are groups of 64 candidates, 256 at most
    assert q(1, 64, 1) == 256 + 4 and q(1, 65, 1) == 256 + 2 * 4 and q(1, 1 << 20, 8) == 256 * 8 * 8 + 256 * 8 * 4
    assert q(1 << 30, 1 << 30, 8) == (1 << 30) * 8 * 12  # 64-bit sizes


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_lut_sample():
    from crt1d_amd import batched

    lo, hi = np.array([1.0, -2.0, 0.0]), np.array([4.0, 3.0, 0.0])  # (a degenerate axis is allowed)
    q = batched.lut_sample(lo, hi, 100)
    assert q.shape == (100, 3) and q.dtype == np.float64 and (q >= lo).all() and (q <= hi).all()
    assert np.array_equal(q, batched.lut_sample(lo, hi, 100)) and np.array_equal(q[:40], batched.lut_sample(lo, hi, 40))
    assert len({tuple(r) for r in q}) == 100
    inc = np.array([[2.0, 0.0, 0.0], [9.0, 9.0, 9.0]])  # taken as they are, first
    qi = batched.lut_sample(lo, hi, 100, include=inc)
    assert qi.shape == (100, 3) and np.array_equal(qi[:2], inc) and np.array_equal(qi[2:], q[:98])
    assert np.array_equal(batched.lut_sample(lo, hi, 3, include=inc[0])[0], inc[0])
    assert np.array_equal(batched.lut_sample(lo, hi, 2, include=inc), inc)
    # the first 64 points of a 2-D box: bases 2 and 3 put 4 +- 2 into each cell of a 4 x 4 grid
    q = batched.lut_sample([0.0, 10.0], [1.0, 30.0], 64)
    cells = np.histogram2d(q[:, 0], (q[:, 1] - 10.0) / 20.0, bins=4, range=[[0, 1], [0, 1]])[0]
    assert cells.sum() == 64 and cells.min() >= 2 and cells.max() <= 6
    for bad_lo, bad_hi in (([0.0, -np.inf], [1.0, 1.0]), ([0.0, 0.0], [1.0, np.inf]), ([np.nan, 0.0], [1.0, 1.0])):
        with pytest.raises(ValueError, match="finite bounds"):
            batched.lut_sample(bad_lo, bad_hi, 8)
    with pytest.raises(ValueError, match="lo must not exceed hi"):
        batched.lut_sample([1.0], [0.0], 8)
    with pytest.raises(ValueError, match=r"must be \(npar,\)"):
        batched.lut_sample(np.zeros(11), np.ones(11), 8)
    with pytest.raises(ValueError, match="include must be"):
        batched.lut_sample(lo, hi, 8, include=np.zeros((1, 2)))
    with pytest.raises(ValueError, match="ncand must be"):
        batched.lut_sample(lo, hi, 1, include=inc)
    with pytest.raises(ValueError, match="ncand must be"):
        batched.lut_sample(lo, hi, 0)


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
class _Cols:  # (what the checks look at before they touch a column or a device)
    ncol, nz, device = 1, 12, "nowhere"


class _Bands:
    import torch

    dtype, nb, _shape = torch.float64, 8, (1, 8)


def _table(params=("lai",), keys=("I_df_u",), shape=(2, 5), spectral=False, K=6):
    import torch

    from crt1d_amd import batched

    n = int(np.prod(shape))
    return batched.LutTable(torch.zeros((K, len(params)), dtype=torch.float64), {k: torch.zeros((K, n), dtype=torch.float64) for k in keys},
                            params=params, keys=keys, shape=shape, scheme="2s", spectral=spectral)


def test_table_build_errors_need_no_device():
    from crt1d_amd import batched

    sensors = batched.SensorSet.from_supports([0, 2], [3, 4], np.ones(7), nb=8, device="cpu")
    q = np.zeros((6, 1))
    build = batched.LutTable.build
    with pytest.raises(ValueError, match="unknown scheme"):
        build("nope", None, None, (0,), q, keys=("F",))
    for scheme in ("n79", "zq", "4s", "zq_pa"):  # no spectral table; with sensors n79 and zq are served
        with pytest.raises(ValueError, match="has no spectral look-up table"):
            build(scheme, None, None, (0,), q, keys=("F",))
    for scheme in ("4s", "zq_pa"):
        with pytest.raises(ValueError, match="has no look-up table"):
            build(scheme, None, None, (0,), q, keys=("F",), sensors=sensors)
    with pytest.raises(ValueError, match="keys must be distinct"):
        build("2s", None, None, (0,), q, keys=("x0",))
    with pytest.raises(ValueError, match="no parameter at all"):
        build("2s", None, None, (0,), q, keys=("F",), lai=False)

    class Three(_Cols):
        ncol = 3

    class ThreeBands(_Bands):
        _shape = (3, 8)

    for sens in (None, sensors):
        with pytest.raises(ValueError, match="ONE template column: cols has 3"):
            build("2s", Three(), _Bands(), (0,), q, keys=("F",), sensors=sens)
        with pytest.raises(ValueError, match="ONE template column: bands has 3"):
            build("2s", _Cols(), ThreeBands(), (0,), q, keys=("F",), sensors=sens)
        with pytest.raises(ValueError, match="ONE template column: sun has 3"):
            build("2s", _Cols(), _Bands(), (0,), q, keys=("F",), sensors=sens, sun=Three())
        for bad in (np.zeros(6), np.zeros((6, 2)), np.zeros((0, 1))):
            with pytest.raises(ValueError, match=r"q must be \(K, npar\)"):
                build("2s", _Cols(), _Bands(), (0,), bad, keys=("F",), sensors=sens)
        with pytest.raises(ValueError, match="q must be finite"):
            build("2s", _Cols(), _Bands(), (0,), np.full((6, 1), np.nan), keys=("F",), sensors=sens)
        with pytest.raises(ValueError, match="chunk must be"):
            build("2s", _Cols(), _Bands(), (0,), q, keys=("F",), sensors=sens, chunk=0)
    with pytest.raises(TypeError, match="sensors must be a SensorSet"):
        build("2s", _Cols(), _Bands(), (0,), q, keys=("F",), sensors=np.ones((2, 8)))


def test_match_plan_errors_need_no_device():
    from crt1d_amd import batched

    t = _table(keys=("I_df_u", "F"))
    y = {"I_df_u": np.zeros((3, 2, 5)), "F": np.zeros((3, 2, 5))}
    for make in (batched.LutMatchPlan, batched.lut_match):
        with pytest.raises(TypeError, match="table must be a LutTable"):
            make(None, y)
        with pytest.raises(TypeError, match="y must be a dict"):
            make(t, np.zeros((3, 2, 5)))
        with pytest.raises(ValueError, match="y lacks the keys"):
            make(t, {"F": y["F"]})
        with pytest.raises(ValueError, match="which are not in keys"):
            make(t, dict(y, I_dr=y["F"]))
        with pytest.raises(ValueError, match="which are not in keys"):
            make(t, y, inv_sigma={"I_dr": y["F"]})
        with pytest.raises(ValueError, match=r"must be \(ncol, nsel, nsens\)"):  # a wrong rank
            make(t, {k: np.zeros((3, 10)) for k in y})
        with pytest.raises(ValueError, match="must share one shape"):
            make(t, dict(y, F=np.zeros((4, 2, 5))))
        with pytest.raises(ValueError, match=r"y\['I_df_u'\] must be \(ncol, nsel, nsens\) = \(ncol, 2, 5\)"):
            make(t, {k: np.zeros((3, 2, 6)) for k in y})
        for nbest in (0, 9):
            with pytest.raises(ValueError, match="nbest must be in 1 .. 8"):
                make(t, y, nbest=nbest)
        with pytest.raises(ValueError, match="ksplit must be"):
            make(t, y, ksplit=-1)
        with pytest.raises(ValueError, match="prior and inv_sigma_prior go together"):
            make(t, y, prior=np.zeros(1))
    ts = _table(keys=("F",), shape=(3, 2, 8), spectral=True)  # a series of spectra
    with pytest.raises(ValueError, match=r"must be \(ncol, nt, nsel, nb\)"):
        batched.LutMatchPlan(ts, {"F": np.zeros((3, 2, 8))})


def test_table_start_errors_need_no_device():
    from crt1d_amd import batched

    sensors = batched.SensorSet.from_supports([0, 2], [3, 4], np.ones(7), nb=8, device="cpu")
    y = {"I_df_u": np.zeros((3, 1, 2))}
    for make in (batched.RetrievalPlan, batched.retrieve):
        with pytest.raises(ValueError, match="the table has the parameters"):
            make("2s", None, None, (0,), sensors, y, keys=("I_df_u",), p0=_table(params=("dir0", "lai")))
        with pytest.raises(ValueError, match="the table has the parameters"):
            make("2s", None, None, (0,), sensors, y, keys=("I_df_u",), leaf=True, p0=_table())
        with pytest.raises(ValueError, match="the table has the keys"):
            make("2s", None, None, (0,), sensors, y, keys=("I_df_u",), p0=_table(keys=("F",)))
        with pytest.raises(ValueError, match="the table holds level spectra"):
            make("2s", None, None, (0,), sensors, y, keys=("I_df_u",), p0=_table(spectral=True))
        with pytest.raises(ValueError, match=r"the table's rows are \(2, 5\) per candidate, y\['I_df_u'\] is \(3, 1, 2\)"):
            make("2s", None, None, (0,), sensors, y, keys=("I_df_u",), p0=_table())
    ys = {"I_df_u": np.zeros((3, 1, 8))}
    for make in (batched.SpectralRetrievalPlan, batched.retrieve_spectral):
        with pytest.raises(ValueError, match="the table has the parameters"):
            make("2s", None, None, (0,), ys, keys=("I_df_u",), p0=_table(params=("leaf",), spectral=True))
        with pytest.raises(ValueError, match="the table has the keys"):
            make("2s", None, None, (0,), ys, keys=("I_df_u",), p0=_table(keys=("I_df_u", "F"), spectral=True))
        with pytest.raises(ValueError, match="the table holds sensor-band sums"):
            make("2s", None, None, (0,), ys, keys=("I_df_u",), p0=_table())
        with pytest.raises(ValueError, match="the table's rows are"):
            make("2s", None, None, (0,), ys, keys=("I_df_u",), p0=_table(shape=(1, 9), spectral=True))


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
def test_reference_against_a_double_loop():
    """3 columns x 5 candidates x 4 rows (two blocks of 3 and 1) and a prior, with a masked row that holds NaN, a NaN table entry, a
    duplicated candidate and a masked prior row: the contracts spelled out entry by entry in Python floats."""
    rng = np.random.default_rng(5)
    ncol, K, npar, rows = 3, 5, 2, (3, 1)
    q = rng.normal(size=(K, npar))
    m = [rng.normal(size=(K, n)) for n in rows]
    y = [rng.normal(size=(ncol, n)) for n in rows]
    w = [rng.uniform(0.5, 2.0, size=(ncol, rows[0])), None]
    prior, wp = rng.normal(size=(ncol, npar)), rng.uniform(0.5, 2.0, size=(ncol, npar))
    q[3], m[0][3], m[1][3] = q[1], m[0][1], m[1][1]  # candidate 3 duplicates candidate 1
    m[0][4, 2] = np.nan  # candidate 4 is eligible for no column
    w[0][1, 2], y[0][1, 2] = 0.0, np.nan  # ... not even for column 1, where the row of its NaN is masked
    wp[2, 0] = 0.0
    cost = np.empty((ncol, K))
    for c in range(ncol):
        for k in range(K):
            s = 0.0
            for b, n in enumerate(rows):
                for o in range(n):
                    ww = 1.0 if w[b] is None else float(w[b][c, o])
                    if ww == 0.0:
                        continue
                    r = (float(m[b][k, o]) - float(y[b][c, o])) * ww if w[b] is not None else float(m[b][k, o]) - float(y[b][c, o])
                    s = s + r * r
            for j in range(npar):
                if float(wp[c, j]) == 0.0:
                    continue
                d = (float(q[k, j]) - float(prior[c, j])) * float(wp[c, j])
                s = s + d * d
            finite = all(np.isfinite(t[k]).all() for t in m) and np.isfinite(q[k]).all()
            cost[c, k] = 0.5 * s if finite else np.nan
    got = R.lut_cost(q, m, y, w, prior, wp)
    assert got.tobytes() == cost.tobytes()
    assert np.isnan(cost[:, 4]).all() and np.isfinite(cost[:, :4]).all()
    for nbest in (1, 3, 8):
        index, best, p = R.lut_match(q, m, y, w, prior, wp, nbest=nbest, p_default=np.full((ncol, npar), 7.0))
        for c in range(ncol):
            order = sorted((k for k in range(K) if cost[c, k] < np.inf), key=lambda k: (cost[c, k], k))[:nbest]
            assert index[c].tolist() == order + [-1] * (nbest - len(order))
            assert best[c].tolist() == [cost[c, k] for k in order] + [np.inf] * (nbest - len(order))
            assert p[c].tolist() == q[order[0]].tolist()
            assert 3 not in order or order.index(1) < order.index(3)  # the duplicate: the lower index first
        assert (index == 4).sum() == 0
    # no eligible candidate: -1, +inf, the default stays
    index, best, p = R.lut_match(q, [np.full_like(m[0], np.nan), m[1]], y, None, nbest=2, p_default=np.full((ncol, npar), 7.0))
    assert (index == -1).all() and (best == np.inf).all() and (p == 7.0).all()
    # a fully masked column: every cost +0, the first candidates in index order
    index, best, _ = R.lut_match(q, m[:1], y[:1], [np.zeros_like(w[0])], nbest=3)
    assert index.tolist() == [[0, 1, 2]] * ncol and best.tobytes() == np.zeros((ncol, 3)).tobytes()
    # the merge of two halves is the whole
    whole = R.lut_select(cost, 3)
    a, b = R.lut_select(cost[:, :2], 3), R.lut_select(cost[:, 2:], 3)
    merged = R.merge_lists(a[0], a[1], np.where(b[0] >= 0, b[0] + 2, -1), b[1], 3)
    assert np.array_equal(merged[0], whole[0]) and merged[1].tobytes() == whole[1].tobytes()
