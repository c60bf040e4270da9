"""CPU: the Levenberg-Marquardt step on a chain of coupled dates (include_chain/crt1d_hip_lm_chain.h; ``chain=`` on the retrieval plans).

1. The header against the ctypes table: names, argument counts, the struct layout; no other table holds the names; include_chain/ holds
   this one header.
2. Every CRT_ERR_BAD_ARG / CRT_ERR_UNSUPPORTED of the entries is found before any launch (fake device pointers).
3. crt_hip_lm_chain_max_nd equals the header's formula and is 0 for a refused npar; the LDS bytes and the limit are those of
   include_shared/crt1d_hip_lm_shared.h with nothing shared, for every nd up to the limit.
4. The device-free errors of the two plans and of Model.retrieve_chain.
5. tests/lm_chain_reference.py: the long-double dense layer against a 50-digit mpmath solve of the same system.
6. A linear-Gaussian twin: one step at lam = 0 of the reference is the Rauch-Tung-Striebel smoother, mean and marginal covariances."""
import ctypes
import os
import re

import numpy as np
import pytest

import lm_chain_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NAMES = ["crt_hip_lm_chain_covariance_f64", "crt_hip_lm_chain_max_nd", "crt_hip_lm_normal_f64", "crt_hip_lm_step_chain_f64"]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include_chain", "crt1d_hip_lm_chain.h")).read(), flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.CHAIN_EXPORTS) == sorted(_lib._CHAIN_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS, _lib.LEAFMODEL_EXPORTS, _lib.LUT_EXPORTS, _lib.LUT_POSTERIOR_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    for name, (_, argtypes) in _lib._CHAIN_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    chain = os.path.join(ROOT, "include_chain")  # a directory of its own: the other four are held to their lists elsewhere
    assert sorted(os.path.relpath(os.path.join(d, f), chain) for d, _, files in os.walk(chain) for f in files) == ["crt1d_hip_lm_chain.h"]
    assert _header().count("typedef struct") == 1  # (the structs of the step, reused)
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_struct_layout():
    from crt1d_amd import _lib

    m = re.search(r"typedef struct crt_lm_chain \{(.*?)\} crt_lm_chain;", _header(), re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            fields += [re.sub(r"[\s*]", "", f) for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",")]
    S = _lib.CrtLmChain
    assert [f[0] for f in S._fields_] == fields == ["npix", "nd", "dyn_stride", "inv_sigma_dyn"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 4, 8, 16] and ctypes.sizeof(S) == 24
    assert [f[1] for f in S._fields_] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p]
    assert "#define CRT_LM_CHAIN_LDS_LIMIT (160 * 1024)" in _header() and _lib.LM_CHAIN_LDS_LIMIT == 160 * 1024


# ---- 2. / 3. ----------------------------------------------------------------------------------------------------------------------------
def _problem(ncol=6, npar=3, **kw):
    from crt1d_amd import _lib

    o = dict(lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0, lo=None, hi=None, prior=None, inv_sigma_prior=None)
    o.update(kw)
    return _lib.CrtLmProblem(ncol, npar, *[o[k] for k in ("lam_up", "lam_down", "lam_min", "lam_max", "xtol", "ftol", "lo", "hi", "prior",
                                                           "inv_sigma_prior")])


def test_validation_without_gpu(lib):
    """The pointers are fake: a launch would fault on a GPU machine.  The base call has nd one beyond the limit and is otherwise valid:
    it is CRT_ERR_UNSUPPORTED, the last check, so nothing below is rejected for another reason than the one named."""
    from crt1d_amd import _lib

    BAD, UNS = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_UNSUPPORTED
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    npar = 3
    big = lib.crt_hip_lm_chain_max_nd(npar) + 1
    state = _lib.CrtLmState(*[FAKE] * 9)
    blocks = lambda n=1, hole=None: (_lib.CrtLmNormalBlock * 4)(*[_lib.CrtLmNormalBlock(*[None if hole == (q, i) else FAKE for i in range(3)])  # noqa: E731
                                                                  for q in range(min(n, 4))])

    def step(chain="default", prob="default", blk="default", nblk=1, st=state, npix=2, nd=big, stride=0, w=FAKE, **kw):
        ch = _lib.CrtLmChain(npix, nd, stride, w) if chain == "default" else chain
        pr = _problem(ncol=npix * nd, npar=npar, **kw) if prob == "default" else prob
        return lib.crt_hip_lm_step_chain_f64(ref(ch), ref(pr), blocks(nblk) if blk == "default" else blk, nblk, ref(st), None)

    assert step() == UNS and step(stride=(big - 1) * npar) == UNS and step(nblk=4) == UNS and step(npix=1) == UNS
    assert step(prior=FAKE, inv_sigma_prior=FAKE, lo=FAKE, hi=FAKE) == UNS
    assert step(chain=None) == BAD and step(prob=None) == BAD and step(blk=None) == BAD and step(st=None) == BAD
    assert step(npix=0) == BAD and step(nd=0) == BAD and step(nd=-1) == BAD
    assert step(prob=_problem(ncol=2 * big + 1, npar=npar)) == BAD and step(prob=_problem(ncol=big, npar=npar)) == BAD  # ncol != npix * nd
    assert step(stride=1) == BAD and step(stride=big * npar) == BAD and step(stride=-(big - 1) * npar) == BAD
    assert step(w=None) == BAD and step(w=None, nd=2) == BAD
    assert step(prob=_problem(ncol=2, npar=npar), nd=1, w=None, st=None) == BAD  # (nd = 1 needs no weights: it is the NULL state that fails)
    assert step(prob=_problem(ncol=2 * big, npar=0)) == BAD and step(prob=_problem(ncol=2 * big, npar=11)) == BAD
    assert step(nblk=0) == BAD and step(nblk=5) == BAD
    for hole in ((0, 0), (0, 1), (0, 2), (1, 1)):
        assert step(blk=blocks(2, hole), nblk=2) == BAD, hole
    assert step(blk=blocks(2, (1, 1)), nblk=1) == UNS  # a block beyond nblk is not looked at
    for kw in (dict(lam_up=1.0), dict(lam_up=float("nan")), dict(lam_down=0.0), dict(lam_down=1.5), dict(lam_min=-1.0), dict(lam_max=1e-13),
               dict(xtol=-1.0), dict(ftol=float("nan")), dict(prior=FAKE), dict(inv_sigma_prior=FAKE)):
        assert step(**kw) == BAD, kw
    for hole in range(9):
        assert step(st=_lib.CrtLmState(*[None if i == hole else FAKE for i in range(9)])) == BAD
    assert step(stride=1, nd=big + 5) == BAD  # a bad argument wins over the limit

    def cov(chain="default", npar=npar, A=FAKE, out=FAKE, npix=2, nd=big, stride=0, w=FAKE):
        ch = _lib.CrtLmChain(npix, nd, stride, w) if chain == "default" else chain
        return lib.crt_hip_lm_chain_covariance_f64(ref(ch), npar, A, out, None)

    assert cov() == UNS and cov(stride=(big - 1) * npar) == UNS
    assert cov(chain=None) == BAD and cov(A=None) == BAD and cov(out=None) == BAD and cov(npar=0) == BAD and cov(npar=11) == BAD
    assert cov(npix=0) == BAD and cov(nd=0) == BAD and cov(stride=7) == BAD and cov(w=None) == BAD

    good = lambda **kw: _lib.CrtLmObs(kw.get("nrow", 5), kw.get("f", FAKE), kw.get("J", FAKE), kw.get("y", FAKE), kw.get("s", None))  # noqa: E731
    arr = lambda *o: (_lib.CrtLmObs * 4)(*o)  # noqa: E731

    def normal(ncol=4, npar=3, obs=arr(good()), nblk=1, A=FAKE, g=FAKE, c2=FAKE):
        return lib.crt_hip_lm_normal_f64(ncol, npar, obs, nblk, A, g, c2, None)

    assert normal(ncol=0) == BAD and normal(npar=0) == BAD and normal(npar=11) == BAD and normal(obs=None) == BAD
    assert normal(nblk=0) == BAD and normal(nblk=5) == BAD and normal(A=None) == BAD and normal(g=None) == BAD and normal(c2=None) == BAD
    for bad in (good(nrow=0), good(f=None), good(J=None), good(y=None)):
        assert normal(obs=arr(bad)) == BAD and normal(obs=arr(good(), bad), nblk=2) == BAD


def test_max_nd_is_the_formula_of_the_header(lib):
    from crt1d_amd import _lib

    h = open(os.path.join(ROOT, "include_chain", "crt1d_hip_lm_chain.h")).read()
    assert "8 * (nd * (2 npar^2 + 4 npar) + 4 npar^2 + 64)" in h and "8 * ((long long)(nd) * (2 * (npar) * (npar) + 4 * (npar)) + 4 * (npar) * (npar) + 64)" in h
    for npar in range(1, 11):
        nd = lib.crt_hip_lm_chain_max_nd(npar)
        assert nd == R.max_nd(npar) == _lib.lm_chain_max_nd(npar) >= 83
        assert _lib.lm_chain_lds_bytes(nd, npar) <= 160 * 1024 < _lib.lm_chain_lds_bytes(nd + 1, npar)
    assert lib.crt_hip_lm_chain_max_nd(10) == 83 and lib.crt_hip_lm_chain_max_nd(5) == 290
    for npar in (0, -1, 11, 1000):
        assert lib.crt_hip_lm_chain_max_nd(npar) == 0 == _lib.lm_chain_max_nd(npar)


def test_chain_lds_bytes_are_the_shared_bytes_with_nothing_shared(lib):
    """The chain entries launch the shared-parameter kernels with ns = 0 and may size the LDS with either macro: the two byte counts
    (and the macro of the chain's header, written out) agree for every nd an entry accepts, and so do the two limits."""
    from crt1d_amd import _lib

    for npar in range(1, 11):
        limit = lib.crt_hip_lm_chain_max_nd(npar)
        assert limit == lib.crt_hip_lm_shared_max_nd(npar, 0) == _lib.lm_shared_max_nd(npar, 0)
        for nd in range(1, limit + 1):
            want = 8 * (nd * (2 * npar * npar + 4 * npar) + 4 * npar * npar + 64)
            assert _lib.lm_chain_lds_bytes(nd, npar) == _lib.lm_shared_lds_bytes(nd, npar, 0) == want <= 160 * 1024, (nd, npar)


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def test_chain_python_errors_need_no_device():
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    class Cols:
        ncol, nz, device = 6, 6, "nowhere"

    class Bands:
        dtype, nb = torch.float64, 8

    sens = batched.SensorSet.from_supports([0], [2], np.ones(2), device="cpu")
    ys = {"I_df_u": np.ones((6, 1, 8))}
    makes = [lambda **kw: batched.RetrievalPlan("2s", Cols(), Bands(), (0,), sens, {"I_df_u": np.ones((6, 1, 1))}, keys=("I_df_u",), **kw),
             lambda **kw: batched.retrieve("2s", Cols(), Bands(), (0,), sens, {"I_df_u": np.ones((6, 1, 1))}, keys=("I_df_u",), **kw),
             lambda **kw: batched.SpectralRetrievalPlan("2s", Cols(), Bands(), (0,), ys, keys=("I_df_u",), **kw),
             lambda **kw: batched.retrieve_spectral("2s", Cols(), Bands(), (0,), ys, keys=("I_df_u",), **kw)]
    d2 = np.ones((2, 8))  # npar = 3: two directions and ln LAI
    for make in makes:
        with pytest.raises(ValueError, match="does not divide ncol = 6"):
            make(d_leaf_r=d2, chain=4, inv_sigma_chain=np.ones((3, 3)))
        with pytest.raises(ValueError, match="an integer >= 1"):
            make(d_leaf_r=d2, chain=0, inv_sigma_chain=np.ones((1, 3)))
        with pytest.raises(ValueError, match="an integer >= 1"):
            make(d_leaf_r=d2, chain=1.5, inv_sigma_chain=np.ones((1, 3)))
        with pytest.raises(ValueError, match="needs chain="):
            make(d_leaf_r=d2, inv_sigma_chain=np.ones((2, 3)))
        with pytest.raises(ValueError, match="a chain needs inv_sigma_chain"):
            make(d_leaf_r=d2, chain=3)
        for bad in (np.ones((2, 2)), np.ones((3, 3)), np.ones((6, 2, 3)), np.ones((2, 3, 3)), np.ones(3)):
            with pytest.raises(ValueError, match=r"inv_sigma_chain must be \(2, 3\) or \(2, 2, 3\)"):
                make(d_leaf_r=d2, chain=3, inv_sigma_chain=bad)
        for bad in (-1.0, float("nan")):
            w = np.ones((2, 2, 3))
            w[1, 0, 2] = bad
            with pytest.raises(ValueError, match="must be >= 0"):
                make(d_leaf_r=d2, chain=3, inv_sigma_chain=w)
    assert batched._check_chain(None, None, Cols(), 3) is None and batched._check_chain(3, np.zeros((2, 3)), Cols(), 3) == (2, 3)
    assert batched._check_chain(6, torch.ones((1, 5, 3)), 6, 3) == (1, 6) and batched._check_chain(1, np.ones((0, 3)), 6, 3) == (6, 1)

    class Long:
        ncol, nz, device = 84 * 2, 6, "nowhere"

    with pytest.raises(ValueError, match="beyond the 83 the chain kernel serves at npar = 10"):
        batched._check_chain(84, np.ones((83, 10)), Long(), 10)
    with pytest.raises(ValueError, match="beyond the 83"):
        batched.RetrievalPlan("2s", Long(), Bands(), (0,), sens, {"I_df_u": np.ones((168, 1, 1))}, keys=("I_df_u",), d_leaf_r=np.ones((8, 8)), leaf=True,
                              chain=84, inv_sigma_chain=np.ones((83, 10)))

    m = Model("2s", nlayers=6)
    w = np.ones((2, m.nwl))
    y = {"I_df_u": np.ones((3, 1, 2))}
    psi = np.deg2rad([10.0, 30.0, 50.0])
    with pytest.raises(ValueError, match="non-empty 1-D series"):
        m.retrieve_chain(w, y, psi[None], np.ones((2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match=r"y\['I_df_u'\] must be \(nd, nsel, nsens\) with nd = 3"):
        m.retrieve_chain(w, {"I_df_u": np.ones((2, 1, 2))}, psi, np.ones((2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match=r"inv_sigma_chain must be \(2, 1\) or \(1, 2, 1\)"):
        m.retrieve_chain(w, y, psi, np.ones((3, 1)), levels=(-1,))
    with pytest.raises(ValueError, match="for the model's one pixel"):
        m.retrieve_chain(w, y, psi, np.ones((1, 2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match="must be >= 0"):
        m.retrieve_chain(w, y, psi, -np.ones((2, 1)), levels=(-1,))
    with pytest.raises(ValueError, match="wrt_leaf must be None or 'param'"):
        m.retrieve_chain(w, y, psi, np.ones((2, 1)), levels=(-1,), wrt_leaf="mla")


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
def _twin(rng, nd, npar, nrow=None):
    nrow = nrow or 3 * npar
    J = rng.normal(size=(nd, nrow, npar))
    y = rng.normal(size=(nd, nrow))
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    p = 0.3 * rng.normal(size=(nd, npar))
    r = np.einsum("dok,dk->do", J, p) - y
    return J, y, w, p, (R.pack(np.einsum("doi,doj->dij", J, J)), np.einsum("doi,do->di", J, r), np.einsum("do,do->d", r, r))


def test_long_double_layer_against_mpmath():
    """nd = 3, npar = 2, lam = 1e-2: H, G and the damped solve restated in 50-digit arithmetic from the same fp64 inputs.  The long-double
    Cholesky solve of n = 6 unknowns has a relative error of order n^2 u_ld kappa (u_ld = 2^-64, kappa of order 10^2): 1e-15 of the
    largest entry is asserted, six orders below fp64 results it referees."""
    import mpmath as mp

    mp.mp.dps = 50
    nd, npar, lam = 3, 2, 1e-2
    _, _, w, p, (A, g, c2) = _twin(np.random.default_rng(5), nd, npar)
    n = nd * npar
    H, G = mp.zeros(n, n), mp.zeros(n, 1)
    for d in range(nd):
        for i in range(npar):
            G[d * npar + i] = mp.mpf(float(g[d, i]))
            for j in range(npar):
                H[d * npar + i, d * npar + j] = mp.mpf(float(A[d, R.tri(max(i, j), min(i, j))]))
    for d in range(nd - 1):
        for k in range(npar):
            a, b, w2 = d * npar + k, (d + 1) * npar + k, mp.mpf(float(w[d, k])) ** 2
            e = (mp.mpf(float(p[d + 1, k])) - mp.mpf(float(p[d, k]))) * w2
            H[a, a] += w2
            H[b, b] += w2
            H[a, b] -= w2
            H[b, a] -= w2
            G[a] -= e
            G[b] += e
    D = H.copy()
    for r in range(n):
        D[r, r] = H[r, r] * (1 + mp.mpf(lam))
    delta = mp.lu_solve(D, -G)
    got = R.solve_ld(A, g, p, w, lam).reshape(-1)
    scale = max(abs(delta[r]) for r in range(n))
    assert max(abs(mp.mpf(float(np.float64(got[r]))) + mp.mpf(float(got[r] - np.float64(got[r]))) - delta[r]) for r in range(n)) < 1e-15 * scale
    inv = H ** -1
    X = R.inverse_ld(A, w)
    scale = max(abs(inv[r, q]) for r in range(n) for q in range(n))
    err = max(abs(mp.mpf(float(np.float64(X[r, q]))) + mp.mpf(float(X[r, q] - np.float64(X[r, q]))) - inv[r, q]) for r in range(n) for q in range(n))
    assert err < 1e-15 * scale
    cost = (sum(mp.mpf(float(v)) for v in c2) + sum(((mp.mpf(float(p[d + 1, k])) - mp.mpf(float(p[d, k]))) * mp.mpf(float(w[d, k]))) ** 2
                                                     for d in range(nd - 1) for k in range(npar))) / 2
    assert abs(mp.mpf(float(np.float64(R.cost_ld(c2, p, w)))) - cost) < 2e-16 * cost
    assert abs(R.pixel_cost(c2, p, w) - float(cost)) <= 2 * (nd + (nd - 1) * npar) * U * float(cost)
    # and the fp64 restatement of the banded solve agrees with it within the bound the GPU test uses for the kernel
    fp = R.band_solve(A, g, p, w, lam).reshape(-1)
    lo, hi = R.scaled_extremes(A, w, lam)
    assert max(abs(float(fp[r]) - float(delta[r])) for r in range(n)) < (4 * n * (3 * n + 1) + 8 * n) * U * (hi / lo) * float(scale) * 4


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd,npar", [(1, 2), (4, 1), (5, 3)])
def test_one_undamped_step_is_the_rts_smoother(nd, npar):
    """y_d = J_d p_d + N(0, I), p_{d+1} = p_d + N(0, diag(1 / w_d^2)), p_0 ~ N(m0, diag(1 / s0^2)): the per-date prior rows carry the
    prior of date 0 only (inv_sigma_prior = 0 on the other dates).  The posterior is Gaussian, its mode the minimiser of the chain's
    quadratic cost, so ONE step at lam = 0 from anywhere lands on the smoothed mean and the diagonal blocks of H^-1 are the smoothed
    covariances.  Both sides are fp64 solves of systems whose condition is at most kappa_2(H); 1e4 u kappa_2(H) of the largest entry
    is allowed (n <= 15 unknowns, five filter and smoother sweeps of a few matrix products each)."""
    rng = np.random.default_rng(60 + nd + npar)
    J, y, w, p, blocks = _twin(rng, nd, npar)
    m0, s0 = rng.normal(size=npar), rng.uniform(0.5, 2.0, npar)
    prior, isp = np.zeros((nd, npar)), np.zeros((nd, npar))
    prior[0], isp[0] = m0, s0
    prior[1:] = np.nan  # (never read)
    opt = dict(lam_up=10.0, lam_down=0.1, lam_min=0.0, lam_max=1e12, xtol=0.0, ftol=0.0)
    st = R.new_state(p, 0.0)
    st = R.step(st, [blocks], w, opt, prior=prior, isp=isp)
    assert st["naccept"] == 1 and st["lam"] == 0.0 and st["status"] == R.RUNNING
    # Kalman filter, then the Rauch-Tung-Striebel sweep
    m, P = m0.copy(), np.diag(1.0 / s0 ** 2)
    mf, Pf, mp_, Pp = [], [], [], []
    for d in range(nd):
        mp_.append(m.copy()), Pp.append(P.copy())
        S = J[d] @ P @ J[d].T + np.eye(J.shape[1])
        K = P @ J[d].T @ np.linalg.inv(S)
        m = m + K @ (y[d] - J[d] @ m)
        P = P - K @ J[d] @ P
        mf.append(m.copy()), Pf.append(P.copy())
        if d < nd - 1:
            P = P + np.diag(1.0 / w[d] ** 2)
    ms, Ps = [None] * nd, [None] * nd
    ms[-1], Ps[-1] = mf[-1], Pf[-1]
    for d in reversed(range(nd - 1)):
        Gd = Pf[d] @ np.linalg.inv(Pp[d + 1])
        ms[d] = mf[d] + Gd @ (ms[d + 1] - mp_[d + 1])
        Ps[d] = Pf[d] + Gd @ (Ps[d + 1] - Pp[d + 1]) @ Gd.T
    X = R.inverse_ld(st["A"], w).astype(np.float64)
    H = np.linalg.inv(X)
    kappa = np.linalg.cond(H)
    tol = 1e4 * U * kappa
    assert np.abs(st["p_trial"] - np.array(ms)).max() <= tol * np.abs(np.array(ms)).max()
    for d in range(nd):
        blk = X[d * npar:(d + 1) * npar, d * npar:(d + 1) * npar]
        assert np.abs(blk - Ps[d]).max() <= tol * np.abs(Ps[d]).max()
