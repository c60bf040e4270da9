"""CPU: the date-by-date retrieval (include_seq/crt1d_hip_lm_seq.h; ``prior_precision=`` on the retrieval plans, ``SequentialPlan``).

1. The header against the ctypes table: names, argument counts, the struct layout; no other table holds the names; include_seq/ holds
   this one header.
2. Every CRT_ERR_BAD_ARG of the three entries is found before any launch (fake device pointers).
3. The device-free errors of the plans, of ``SequentialPlan`` and of ``Model.retrieve_sequential``.
4. tests/lm_seq_reference.py against itself: the product form of the parallel sum against its definition (two inversions, long double)
   and against a 50-digit mpmath evaluation in a stiff case; on a random linear-Gaussian pixel the long-double filter plus
   Rauch-Tung-Striebel sweep equals the dense chain system of tests/lm_chain_reference.py, and the block-tridiagonal solve does too."""
import ctypes
import os
import re

import numpy as np
import pytest

import lm_chain_reference as R
import lm_seq_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NAMES = ["crt_hip_lm_predict_f64", "crt_hip_lm_prior_block_f64", "crt_hip_lm_rts_f64"]
LD = np.longdouble


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include_seq", "crt1d_hip_lm_seq.h")).read(), flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.SEQ_EXPORTS) == sorted(_lib._SEQ_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS, _lib.LEAFMODEL_EXPORTS, _lib.LUT_EXPORTS, _lib.LUT_POSTERIOR_EXPORTS, _lib.CHAIN_EXPORTS,
              _lib.SHARED_EXPORTS, _lib.MASKED_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    for name, (_, argtypes) in _lib._SEQ_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    seq = os.path.join(ROOT, "include_seq")
    assert sorted(os.path.relpath(os.path.join(d, f), seq) for d, _, files in os.walk(seq) for f in files) == ["crt1d_hip_lm_seq.h"]
    assert _header().count("typedef struct") == 1
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_struct_layout():
    from crt1d_amd import _lib

    m = re.search(r"typedef struct crt_lm_prior_full \{(.*?)\} crt_lm_prior_full;", _header(), re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            fields += [re.sub(r"[\s*]", "", f) for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",")]
    S = _lib.CrtLmPriorFull
    assert [f[0] for f in S._fields_] == fields == ["ncol", "npar", "prec_stride", "precision", "mean"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 4, 8, 16, 24] and ctypes.sizeof(S) == 32
    assert [f[1] for f in S._fields_] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def test_validation_without_gpu(lib):
    """The pointers are fake: a launch would fault on a GPU machine, so every call here is one that must be refused.  Each case differs
    from a valid call in the one thing named."""
    from crt1d_amd import _lib

    BAD = _lib.CRT_ERR_BAD_ARG
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731

    def block(pr="default", ncol=4, npar=3, stride=6, prec=FAKE, mean=FAKE, p=FAKE, A=FAKE, g=FAKE, c2=FAKE):
        pr = _lib.CrtLmPriorFull(ncol, npar, stride, prec, mean) if pr == "default" else pr
        return lib.crt_hip_lm_prior_block_f64(ref(pr), p, A, g, c2, None)

    for kw in (dict(pr=None), dict(ncol=0), dict(ncol=-1), dict(npar=0), dict(npar=11, stride=66), dict(stride=3), dict(stride=9), dict(stride=-6),
               dict(prec=None), dict(mean=None), dict(p=None), dict(A=None), dict(g=None), dict(c2=None), dict(stride=6, npar=2)):
        assert block(**kw) == BAD, kw

    def predict(ncol=4, npar=3, A=FAKE, w=FAKE, stride=3, prec=FAKE, info=FAKE):
        return lib.crt_hip_lm_predict_f64(ncol, npar, A, w, stride, prec, info, None)

    for kw in (dict(ncol=0), dict(npar=0), dict(npar=11, stride=11), dict(A=None), dict(w=None), dict(prec=None), dict(info=None), dict(stride=1),
               dict(stride=6), dict(stride=-3)):
        assert predict(**kw) == BAD, kw

    def rts(chain="default", npar=3, npix=2, nd=5, stride=0, w=FAKE, p_f=FAKE, A_f=FAKE, p_s=FAKE, cov=FAKE, info=FAKE):
        ch = _lib.CrtLmChain(npix, nd, stride, w) if chain == "default" else chain
        return lib.crt_hip_lm_rts_f64(ref(ch), npar, p_f, A_f, p_s, cov, info, None)

    for kw in (dict(chain=None), dict(npix=0), dict(nd=0), dict(nd=-1), dict(npar=0), dict(npar=11), dict(stride=3), dict(stride=15), dict(stride=-12),
               dict(w=None), dict(w=None, nd=2), dict(p_f=None), dict(A_f=None), dict(p_s=None), dict(cov=None), dict(info=None),
               dict(nd=1, w=None, info=None), dict(nd=100000, stride=7)):
        assert rts(**kw) == BAD, kw


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_python_errors_need_no_device():
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    class Cols:
        ncol, nz, device = 6, 6, "nowhere"

    class Bands:
        dtype, nb = torch.float64, 8

    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    ys = {"I_df_u": np.ones((6, 1, 8))}
    yr = {"I_df_u": np.ones((6, 1, 1))}
    makes = [lambda **kw: batched.RetrievalPlan("2s", Cols(), Bands(), (0,), sens, yr, keys=("I_df_u",), **kw),
             lambda **kw: batched.retrieve("2s", Cols(), Bands(), (0,), sens, yr, keys=("I_df_u",), **kw),
             lambda **kw: batched.SpectralRetrievalPlan("2s", Cols(), Bands(), (0,), ys, keys=("I_df_u",), **kw),
             lambda **kw: batched.retrieve_spectral("2s", Cols(), Bands(), (0,), ys, keys=("I_df_u",), **kw)]
    d2 = np.ones((2, 8))  # npar = 3: two directions and ln LAI
    m, P = np.zeros(3), np.eye(3)
    for make in makes:
        with pytest.raises(ValueError, match="prior_mean and prior_precision go together"):
            make(d_leaf_r=d2, prior_mean=m)
        with pytest.raises(ValueError, match="prior_mean and prior_precision go together"):
            make(d_leaf_r=d2, prior_precision=P)
        with pytest.raises(ValueError, match="cannot be combined with chain="):
            make(d_leaf_r=d2, prior_mean=m, prior_precision=P, chain=3, inv_sigma_chain=np.ones((2, 3)))
        for bad in (np.zeros(2), np.zeros((5, 3)), np.zeros((3, 3))):
            with pytest.raises(ValueError, match=r"prior_mean must be \(6, 3\) or \(3,\)"):
                make(d_leaf_r=d2, prior_mean=bad, prior_precision=P)
        for bad in (np.zeros(3), np.zeros((6, 3)), np.zeros((5, 3, 3)), np.zeros((6, 2, 3))):
            with pytest.raises(ValueError, match=r"prior_precision must be \(6, 3, 3\) or \(3, 3\)"):
                make(d_leaf_r=d2, prior_mean=m, prior_precision=bad)
    for make in makes[:2]:  # (a spectral plan refuses evaluate="accepted" whatever the prior)
        with pytest.raises(ValueError, match="k_lm_decide.*takes no block"):
            make(d_leaf_r=d2, prior_mean=m, prior_precision=P, evaluate="accepted")
    assert batched._check_full_prior(None, None, 3, "accepted", 6, 3) is False
    assert batched._check_full_prior(np.zeros((6, 3)), torch.zeros((6, 3, 3)), None, "running", Cols(), 3) is True

    seqs = [lambda **kw: batched.SequentialPlan("2s", Cols(), Bands(), (0,), yr, keys=("I_df_u",), sensors=sens, d_leaf_r=d2, **kw),
            lambda **kw: batched.retrieve_sequential("2s", Cols(), Bands(), (0,), ys, keys=("I_df_u",), d_leaf_r=d2, **kw)]
    w = np.ones((2, 3))
    for make in seqs:
        for name, v in (("sun", object()), ("chain", 3), ("shared", ("lai",))):
            with pytest.raises(ValueError, match=name + "= is not served inside a SequentialPlan"):
                make(nd=3, inv_sigma_dyn=w, **{name: v})
        for bad in (0, 1.5, -2):
            with pytest.raises(ValueError, match="an integer >= 1"):
                make(nd=bad, inv_sigma_dyn=w)
        with pytest.raises(ValueError, match="does not divide ncol = 6"):
            make(nd=4, inv_sigma_dyn=np.ones((3, 3)))
        with pytest.raises(ValueError, match="needs inv_sigma_dyn"):
            make(nd=3, inv_sigma_dyn=None)
        for bad in (np.ones((2, 2)), np.ones((3, 3)), np.ones((6, 2, 3)), np.ones(3)):
            with pytest.raises(ValueError, match=r"inv_sigma_dyn must be \(2, 3\) or \(2, 2, 3\)"):
                make(nd=3, inv_sigma_dyn=bad)
        for bad in (-1.0, float("nan"), float("inf")):
            v = np.ones((2, 2, 3))
            v[1, 0, 2] = bad
            with pytest.raises(ValueError, match="finite and >= 0"):
                make(nd=3, inv_sigma_dyn=v)
    assert batched._check_sequential(84, np.ones((83, 10)), 168, dict(d_leaf_r=np.ones((8, 8)), leaf=True)) == (2, 84, 10)  # no limit on nd

    mod = Model("2s", nlayers=6)
    sw = np.ones((2, mod.nwl))
    y = {"I_df_u": np.ones((3, 1, 2))}
    psi = np.deg2rad([10.0, 30.0, 50.0])
    with pytest.raises(ValueError, match="non-empty 1-D series"):
        mod.retrieve_sequential(sw, y, psi[None], np.ones((2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match=r"y_dates\['I_df_u'\] must be \(nd, nsel, nsens\) with nd = 3"):
        mod.retrieve_sequential(sw, {"I_df_u": np.ones((2, 1, 2))}, psi, np.ones((2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match=r"inv_sigma_dyn must be \(2, 1\) or \(1, 2, 1\)"):
        mod.retrieve_sequential(sw, y, psi, np.ones((3, 1)), levels=(-1,))
    with pytest.raises(ValueError, match="for the model's one pixel"):
        mod.retrieve_sequential(sw, y, psi, np.ones((1, 2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match="wrt_leaf must be None or 'param'"):
        mod.retrieve_sequential(sw, y, psi, np.ones((2, 1)), levels=(-1,), wrt_leaf="mla")


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def _spd(rng, n, kappa):
    Qm, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Qm * np.logspace(0.0, -np.log10(kappa), n)) @ Qm.T


def test_prior_block_restatement_against_long_double():
    rng = np.random.default_rng(3)
    for npar in (1, 3, 10):
        P, mean, p = R.pack(_spd(rng, npar, 1e3)), rng.normal(size=npar), rng.normal(size=npar)
        A, g, c2 = Q.prior_block(P, mean, p)
        gl, cl, gb, cb = Q.prior_block_ld(P, mean, p)
        assert A.tobytes() == P.tobytes()
        assert np.all(np.abs(g.astype(LD) - gl) <= (npar + 2) * Q.U * gb) and abs(LD(c2) - cl) <= (2 * npar + 3) * Q.U * cb
    A, g, c2 = Q.prior_block(np.zeros(6), np.array([1.0, -2.0, 3.0]), np.array([-1.0, 5.0, 0.5]))
    assert not np.signbit(g).any() and not np.signbit(c2) and c2 == 0.0 and not g.any()  # a block of +0 is +0, whatever the mean


def test_parallel_sum_product_form():
    """The product W (A + W)^-1 A of the header against the definition (A^-1 + W^-1)^-1: in a mild case against two long-double
    inversions, 1e-15 of the largest entry (kappa <= 1e2, u_ld = 2^-64); in the stiff case of the GPU test (kappa(A) = 1e6, w from 1e-3
    to 1e5) against 50-digit mpmath, entry by entry in the scaled domain s_i s_j |dP_ij| <= 1e-15 max |S P S|, s = 1 / sqrt(diag(A + W)):
    the long-double product form has c u_ld kappa_2(M_scaled) of error there, 2^-11 of what fp64 is allowed."""
    import mpmath as mp

    rng = np.random.default_rng(11)
    for npar in (1, 3, 10):
        A, w = _spd(rng, npar, 1e2), rng.uniform(0.5, 2.0, npar)
        a, b = Q.parallel_sum_ld(R.pack(A), w), Q.parallel_sum_literal_ld(R.pack(A), w)
        assert np.abs(a - b).max() <= 1e-15 * np.abs(b).max()
    mp.mp.dps = 50
    for npar in (1, 5, 10):
        A = R.pack(_spd(rng, npar, 1e6))
        w = np.logspace(-3, 5, npar) if npar > 1 else np.array([1e5])
        Am = Q.unpack(A)
        H = mp.matrix(npar, npar)
        for i in range(npar):
            for j in range(npar):
                H[i, j] = mp.mpf(float(Am[i, j]))
        X = H ** -1
        for k in range(npar):
            X[k, k] += 1 / mp.mpf(float(w[k])) ** 2
        want = X ** -1
        got = Q.parallel_sum_ld(A, w)
        s = 1.0 / np.sqrt(np.diagonal(Am) + w * w)
        err = max(abs(mp.mpf(float(np.float64(got[i, j]))) + mp.mpf(float(got[i, j] - np.float64(got[i, j]))) - want[i, j]) * s[i] * s[j]
                  for i in range(npar) for j in range(npar))
        scale = max(abs(want[i, j]) * s[i] * s[j] for i in range(npar) for j in range(npar))
        assert err <= 1e-15 * scale, (npar, float(err / scale))
    # forget (w_k = 0) and a dead parameter: exactly zero rows and columns, the rest the parallel sum of the rest
    A = _spd(rng, 4, 10.0)
    A[2, :] = A[:, 2] = 0.0
    w = np.array([1.0, 0.0, 0.0, 2.0])
    got = Q.parallel_sum_ld(R.pack(A), w)
    assert not got[1].any() and not got[:, 1].any() and not got[2].any() and not got[:, 2].any()
    sub = Q.parallel_sum_literal_ld(R.pack(A[np.ix_([0, 1, 3], [0, 1, 3])]), np.array([1.0, 1e-30, 2.0]))  # (w -> 0 as a limit)
    assert np.abs(got[np.ix_([0, 3], [0, 3])] - sub[np.ix_([0, 2], [0, 2])]).max() <= 1e-15 * np.abs(sub).max()


def _linear_pixel(rng, nd, npar):
    nrow = 3 * npar
    J = rng.normal(size=(nd, nrow, npar))
    y = rng.normal(size=(nd, nrow))
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    A = R.pack(np.einsum("doi,doj->dij", J, J))
    b = np.einsum("doi,do->di", J, y)
    return A, b, w


@pytest.mark.parametrize("nd,npar", [(1, 1), (1, 3), (1, 10), (2, 1), (2, 3), (2, 10), (7, 1), (7, 3), (7, 10), (84, 10)])
def test_filter_plus_sweep_is_the_chain(nd, npar):
    """y_t = J_t p_t + N(0, I), a random walk between the dates, a full Gaussian prior on date 0: the long-double information filter
    and Rauch-Tung-Striebel sweep against the dense solve and the dense inverse of the chain's (nd npar)^2 system, 1e-15 of the largest
    entry.  The prior of date 0 enters the dense system through A_0 and g_0, which is exactly how the step kernel sees a prior block.
    nd = 84 at npar = 10 is one past the chain kernel's limit: there the inverse is compared on the block columns of the first, a
    middle and the last date (the dense factor is shared), and the block-tridiagonal solve on every date."""
    assert nd <= R.max_nd(npar) or (nd, npar) == (84, 10)
    rng = np.random.default_rng(1000 + 10 * nd + npar)
    A, b, w = _linear_pixel(rng, nd, npar)
    m0, P0 = rng.normal(size=npar), R.pack(_spd(rng, npar, 10.0) * 2.0)
    pf, Af = Q.filter_ld(A, b, w, m0, P0)
    ps, Cs = Q.rts_ld(pf, R.pack(Af), w)
    # the dense system at p = 0: A_0 += P0, g = -(b + P0 m0 on date 0)
    Ad, g = A.copy(), -b.copy()
    Ad[0] = Ad[0] + P0
    g[0] = g[0] - Q.unpack(P0) @ m0
    x, S = Q.block_tridiagonal_ld(Ad, -g, w)
    want = R.solve_ld(Ad, g, np.zeros((nd, npar)), w, 0.0)
    scale = np.abs(want).max()
    assert np.abs(ps - want).max() <= 1e-15 * scale and np.abs(x - want).max() <= 1e-15 * scale
    dates = range(nd) if nd <= 7 else (0, nd // 2, nd - 1)
    cols = Q.dense_columns_ld(Ad, w, dates)
    cscale = max(np.abs(c).max() for c in cols.values())
    for d in dates:
        blk = cols[d][d * npar:(d + 1) * npar]
        assert np.abs(Cs[d] - blk).max() <= 1e-15 * cscale and np.abs(S[d] - blk).max() <= 1e-15 * cscale
    assert np.abs(Cs - S).max() <= 1e-15 * cscale
    if nd <= 7:
        X = R.inverse_ld(Ad, w)
        for d in range(nd):
            assert np.abs(Cs[d] - X[d * npar:(d + 1) * npar, d * npar:(d + 1) * npar]).max() <= 1e-15 * cscale
