"""CPU: the look-up-table posterior (include_post/crt1d_hip_lut_posterior.h; batched.LutPosteriorPlan, lut_posterior, ``posterior=True``).

1. The header against the ctypes table: names, argument counts, the struct layout; no other table holds the names; include_post/ holds
   this one header.
2. Every CRT_ERR_BAD_ARG / CRT_ERR_WORKSPACE of the entry is found before any launch (fake device pointers).
3. The workspace query: 0 for refused sizes, monotone in ksplit.
4. The device-free errors of ``LutPosteriorPlan``, ``lut_posterior`` and ``posterior=True`` without a table.
5. tests/lut_posterior_reference.py against a 50-digit mpmath evaluation of the same formulas.
6. The linear-Gaussian grid twin on the reference: mean and covariance equal the analytic posterior."""
import ctypes
import os
import re

import numpy as np
import pytest

import lut_posterior_reference as P
import lut_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NAMES = ["crt_hip_lut_posterior_f64", "crt_hip_lut_posterior_workspace_bytes"]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include_post", "crt1d_hip_lut_posterior.h")).read(), flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.LUT_POSTERIOR_EXPORTS) == sorted(_lib._LUT_POSTERIOR_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS, _lib.LEAFMODEL_EXPORTS, _lib.LUT_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    for name, (_, argtypes) in _lib._LUT_POSTERIOR_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    post = os.path.join(ROOT, "include_post")  # a directory of its own: the other three are held to their lists elsewhere
    assert sorted(os.path.relpath(os.path.join(d, f), post) for d, _, files in os.walk(post) for f in files) == ["crt1d_hip_lut_posterior.h"]
    assert '#include "crt1d_hip_lut.h"' in _header() and _header().count("typedef struct") == 1  # (the match's structs, reused)
    assert len(_lib.EXPORTS) == 57 and len(_lib.LUT_EXPORTS) == 2 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_struct_layout():
    from crt1d_amd import _lib

    m = re.search(r"typedef struct crt_lut_posterior_out \{(.*?)\} crt_lut_posterior_out;", _header(), re.S)
    fields = [re.sub(r"[\s*]", "", re.sub(r"^(const\s+)?\w+\s*\*?", "", d.strip(), count=1)) for d in m.group(1).split(";") if d.strip()]
    S = _lib.CrtLutPosteriorOut
    assert [f[0] for f in S._fields_] == fields == ["temperature", "temperature_col", "ksplit", "index", "cost", "mean", "cov", "wsum", "ess"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64] and ctypes.sizeof(S) == 72
    kinds = [ctypes.c_double, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 6
    assert [f[1] for f in S._fields_] == kinds


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def _args(ncand=100, npar=3, nblk=2, nrow=(5, 7), ncol=10, prior=True, temperature=1.0, ksplit=0):
    from crt1d_amd import _lib

    i4, p4 = ctypes.c_int32 * 4, ctypes.c_void_p * 4
    ptrs = lambda n=nblk: p4(*[FAKE] * n)  # noqa: E731
    t = _lib.CrtLutTable(ncand, npar, nblk, i4(*nrow), FAKE, ptrs())
    o = _lib.CrtLutObs(ncol, ptrs(), ptrs(), FAKE if prior else None, FAKE if prior else None)
    out = _lib.CrtLutPosteriorOut(temperature, None, ksplit, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
    return t, o, out


def test_validation_without_gpu(lib):
    """Every one of these is found before the first launch (the pointers are fake: a launch would fault on a GPU machine); a valid call
    gets as far as the workspace check, and CRT_ERR_BAD_ARG comes before CRT_ERR_WORKSPACE, as in the match."""
    from crt1d_amd import _lib

    BAD, WS = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    p4 = ctypes.c_void_p * 4

    def call(change=None, t=True, o=True, out=True, ws=None, wsb=0, **kw):
        T, O, X = _args(**kw)
        if change:
            change(T, O, X)
        return lib.crt_hip_lut_posterior_f64(ref(T) if t else None, ref(O) if o else None, ref(X) if out else None, ws, wsb, None)

    def setter(which, field, value):
        def change(T, O, X):
            setattr({"t": T, "o": O, "x": X}[which], field, value)
        return change

    assert call() == WS  # valid: nothing below is rejected for any other reason than the one named
    need = lib.crt_hip_lut_posterior_workspace_bytes(10, 100, 3, 0)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS and call(ws=None, wsb=need) == WS
    need2 = lib.crt_hip_lut_posterior_workspace_bytes(10, 100, 3, 1)
    assert need2 < need and call(ws=FAKE, wsb=need2 - 1, ksplit=1) == WS  # the query follows ksplit
    assert call(prior=False) == WS and call(nblk=1, nrow=(1,)) == WS and call(nblk=4, nrow=(1, 2, 3, 4)) == WS
    assert call(setter("o", "inv_sigma", p4())) == WS  # NULL inv_sigma: ones
    assert call(setter("x", "temperature_col", FAKE)) == WS  # optional
    assert call(npar=1) == WS and call(npar=10) == WS and call(ncand=1) == WS and call(ncol=1) == WS
    assert call(ksplit=1) == WS and call(ksplit=1000) == WS  # clamped, not refused
    assert call(temperature=1e-300) == WS and call(temperature=1e300) == WS
    # NULL structs
    assert call(t=False) == BAD and call(o=False) == BAD and call(out=False) == BAD
    # sizes
    assert call(ncand=0) == BAD and call(ncand=-1) == BAD and call(ncol=0) == BAD
    assert call(npar=0) == BAD and call(npar=11) == BAD
    assert call(nblk=0, nrow=()) == BAD and call(setter("t", "nblk", 5)) == BAD
    assert call(nrow=(5, 0)) == BAD and call(nrow=(-1, 5)) == BAD
    assert call(ksplit=-1) == BAD
    # the temperature
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(temperature=bad) == BAD
    # pointers
    assert call(setter("t", "q", None)) == BAD
    assert call(setter("t", "m", p4(FAKE, None))) == BAD and call(setter("t", "m", p4(None, FAKE))) == BAD
    assert call(setter("o", "y", p4(FAKE, None))) == BAD and call(setter("o", "y", p4())) == BAD
    for field in ("index", "cost", "mean", "cov", "wsum", "ess"):
        assert call(setter("x", field, None)) == BAD, field
    assert call(setter("o", "prior", None)) == BAD and call(setter("o", "inv_sigma_prior", None)) == BAD
    # a bad argument wins over a missing workspace, whatever the workspace
    assert call(temperature=0.0, ws=FAKE, wsb=1 << 40) == BAD
    # a block beyond nblk is not looked at
    assert call(nblk=1, nrow=(5, 0)) == WS


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_workspace_query(lib):
    q = lib.crt_hip_lut_posterior_workspace_bytes
    match = lib.crt_hip_lut_match_workspace_bytes
    assert q(0, 10, 1, 0) == 0 and q(10, 0, 1, 0) == 0 and q(10, 10, 0, 0) == 0 and q(10, 10, 11, 0) == 0 and q(10, 10, 1, -1) == 0
    pad = lambda n: (n + 255) & ~255  # noqa: E731
    nacc = lambda npar: 2 + npar + npar * (npar + 1) // 2  # noqa: E731
    # many columns: one part; the partial sums are one (S0, Sq, S1, S2) per lane of every group of 64 columns
    ncol = 64 * 1024
    for npar in (1, 4, 5, 10):
        assert q(ncol, 4096, npar, 0) == pad(match(ncol, 4096, 1)) + ncol * nacc(npar) * 8
    assert q(65, 64, 2, 0) == pad(match(65, 64, 1)) + 128 * nacc(2) * 8  # two groups of columns, one group of candidates
    # one column: automatic = as many parts as there are groups of 64 candidates, 256 at most; an explicit value is honoured and clamped
    one = lambda K, ks: (q(1, K, 3, ks) - pad(match(1, K, 1))) // (64 * nacc(3) * 8)  # noqa: E731
    assert [one(1000, ks) for ks in (0, 1, 2, 3, 7, 16, 17, 256)] == [16, 1, 2, 3, 7, 16, 16, 16]
    assert one(1 << 20, 0) == 256 and one(1 << 20, 1000) == 256 and one(64, 5) == 1 and one(65, 5) == 2
    # an explicit ksplit does not depend on the batch: that is what holds the bits across batch sizes
    parts = lambda n, ks: (q(n, 1000, 3, ks) - pad(match(n, 1000, 1))) // (((n + 63) // 64) * 64 * nacc(3) * 8)  # noqa: E731
    assert [parts(n, 3) for n in (1, 64, 65, 130, 100000)] == [3] * 5
    sizes = [q(130, 5000, 5, ks) for ks in range(1, 80)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]  # monotone in ksplit
    assert q(1 << 30, 1 << 30, 10, 0) == pad(match(1 << 30, 1 << 30, 1)) + (1 << 30) * nacc(10) * 8  # 64-bit sizes


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def _table(params=("lai",), keys=("I_df_u",), shape=(2, 5), spectral=False, K=6):
    import torch

    from crt1d_amd import batched

    n = int(np.prod(shape))
    return batched.LutTable(torch.zeros((K, len(params)), dtype=torch.float64), {k: torch.zeros((K, n), dtype=torch.float64) for k in keys},
                            params=params, keys=keys, shape=shape, scheme="2s", spectral=spectral)


def test_plan_errors_need_no_device():
    import torch

    from crt1d_amd import batched

    t = _table(keys=("I_df_u", "F"))
    y = {"I_df_u": np.zeros((3, 2, 5)), "F": np.zeros((3, 2, 5))}
    for make in (batched.LutPosteriorPlan, batched.lut_posterior):
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
        for ksplit in (-1, 257):
            with pytest.raises(ValueError, match="ksplit must be"):
                make(t, y, ksplit=ksplit)
        with pytest.raises(ValueError, match="prior and inv_sigma_prior go together"):
            make(t, y, prior=np.zeros(1))
        for bad in (0.0, -1.0, float("nan"), float("inf"), 0):
            with pytest.raises(ValueError, match="temperature must be finite and > 0"):
                make(t, y, temperature=bad)
        for bad in ("1", None, True, np.ones(3)):
            with pytest.raises(TypeError, match="temperature must be a number or an"):
                make(t, y, temperature=bad)
        with pytest.raises(ValueError, match="temperature must be a number or a floating-point"):
            make(t, y, temperature=torch.ones((3, 1), dtype=torch.float64))
        with pytest.raises(ValueError, match="temperature must be a number or a floating-point"):
            make(t, y, temperature=torch.ones(3, dtype=torch.int32))
        with pytest.raises(ValueError, match=r"temperature must be a number or \(ncol,\) = \(3,\)"):
            make(t, y, temperature=torch.ones(4, dtype=torch.float64))
        with pytest.raises(TypeError):  # the match's options are not this plan's
            make(t, y, nbest=2)
    ts = _table(keys=("F",), shape=(3, 2, 8), spectral=True)  # a series of spectra
    with pytest.raises(ValueError, match=r"must be \(ncol, nt, nsel, nb\)"):
        batched.LutPosteriorPlan(ts, {"F": np.zeros((3, 2, 8))})


def test_posterior_needs_a_table():
    from crt1d_amd import batched
    from crt1d_amd.model import Model

    sensors = batched.SensorSet.from_supports([0, 2], [3, 4], np.ones(7), nb=8, device="cpu")
    y = {"I_df_u": np.zeros((3, 1, 2))}
    with pytest.raises(ValueError, match="posterior=True needs a look-up table"):
        batched.retrieve("2s", None, None, (0,), sensors, y, keys=("I_df_u",), posterior=True)
    with pytest.raises(ValueError, match="posterior=True needs a look-up table"):
        batched.retrieve("2s", None, None, (0,), sensors, y, keys=("I_df_u",), posterior=True, p0=np.zeros(1))
    with pytest.raises(ValueError, match="posterior=True needs a look-up table"):
        batched.retrieve_spectral("2s", None, None, (0,), {"I_df_u": np.zeros((3, 1, 8))}, keys=("I_df_u",), posterior=True)
    with pytest.raises(ValueError, match="posterior=True needs lut=K"):
        Model.retrieve(None, None, {}, posterior=True)
    with pytest.raises(ValueError, match="posterior=True needs lut=K"):
        Model.retrieve_spectral(None, {}, posterior=True)


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
def test_reference_against_mpmath():
    """K = 7, nrow = 3, npar = 2, two columns (T = 1 and T = 0.25), one ineligible candidate.  The contract fixes cost, a_k and d_ki as
    float64 numbers; from them the weights, the sums and the finish are evaluated with 50 digits.  Bound: 16 u of each result's scale
    (S0, ess, |q[kb]| + A1, A2 + A1 A1)."""
    import mpmath as mp

    mp.mp.dps = 50
    rng = np.random.default_rng(11)
    K, nrow, npar, ncol = 7, 3, 2, 2
    q = rng.normal(size=(K, npar))
    m = [rng.normal(size=(K, nrow))]
    y = [m[0][[2, 5]] + 0.3 * rng.normal(size=(ncol, nrow))]
    w = [rng.uniform(0.5, 2.0, size=(ncol, nrow))]
    m[0][4, 1] = np.nan
    T = np.array([1.0, 0.25])
    ref = P.lut_posterior(q, m, y, w, temperature=T)
    cost = R.lut_cost(q, m, y, w)
    assert (ref["index"] >= 0).all() and (ref["ess"] > 1.0).all()
    for c in range(ncol):
        kb = int(ref["index"][c])
        it = np.float64(1.0) / T[c]
        S0, Sq, S1, S2 = mp.mpf(0), mp.mpf(0), [mp.mpf(0)] * npar, [[mp.mpf(0)] * npar for _ in range(npar)]
        for k in range(K):
            if not cost[c, k] < np.inf:
                assert k == 4
                continue
            wk = mp.exp(-mp.mpf(float((cost[c, k] - cost[c, kb]) * it)))
            d = [mp.mpf(float(q[k, i] - q[kb, i])) for i in range(npar)]
            S0, Sq = S0 + wk, Sq + wk * wk
            S1 = [S1[i] + wk * d[i] for i in range(npar)]
            S2 = [[S2[i][j] + wk * d[i] * d[j] for j in range(npar)] for i in range(npar)]
        assert abs(ref["wsum"][c] - S0) <= 16 * U * S0
        ess = S0 * S0 / Sq
        assert abs(ref["ess"][c] - ess) <= 16 * U * ess
        for i in range(npar):
            mean = mp.mpf(float(q[kb, i])) + S1[i] / S0
            assert abs(ref["mean"][c, i] - mean) <= 16 * U * (abs(q[kb, i]) + ref["A1"][c, i])
            for j in range(npar):
                cov = S2[i][j] / S0 - S1[i] * S1[j] / (S0 * S0)
                assert abs(ref["cov"][c, i, j] - cov) <= 16 * U * (ref["A2"][c, i, j] + ref["A1"][c, i] * ref["A1"][c, j])
    # the same column at both temperatures: the colder one concentrates
    two = P.lut_posterior(q, m, [y[0][[0, 0]]], [w[0][[0, 0]]], temperature=T)
    assert two["ess"][1] < two["ess"][0] and two["index"][0] == two["index"][1]
    # no result: the temperature, or no eligible candidate
    none = P.lut_posterior(q, m, y, w, temperature=np.array([0.0, np.nan]))
    assert (none["index"] == -1).all() and np.isinf(none["cost"]).all() and (none["wsum"] == 0).all() and (none["ess"] == 0).all()
    assert np.isnan(none["mean"]).all() and np.isnan(none["cov"]).all()


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
def test_grid_twin_on_the_reference():
    """Mean and covariance equal the analytic posterior to 1e-10 of the largest posterior standard deviation and of max |C|: the
    discretisation error of a Gaussian of width s summed at spacing h is of order exp(-2 pi^2 (s / h)^2), below 1e-34 at s >= 2 h; the
    box edge is at least 8.7 sigma away (asserted), below 1e-16; rounding is of order K u, about 5e-13.  Measured: 1.5e-15 and 3.6e-16."""
    q, m, y, w, mu, C = P.grid_twin(20)
    assert q.shape == (4225, 2)
    sd = np.sqrt(np.linalg.eigvalsh(C))
    assert abs(sd.min() - 2.0 / 32.0) < 1e-15 and (1.0 - np.abs(mu).max()) / sd.max() >= 8.7
    ref = P.lut_posterior(q, m, y, w)
    err_mean = np.abs(ref["mean"] - mu).max() / sd.max()
    err_cov = np.abs(ref["cov"] - C).max() / np.abs(C).max()
    print(f"grid twin on the reference: mean {err_mean:.2e} of the largest sd, cov {err_cov:.2e} of max |C|, ess {ref['ess'].min():.1f}")
    assert err_mean < 1e-10 and err_cov < 1e-10
    assert (ref["ess"] > 40).all()
