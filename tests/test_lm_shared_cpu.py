"""CPU: the chained Levenberg-Marquardt step with parameters shared by all dates of a pixel (include_shared/crt1d_hip_lm_shared.h;
``shared=`` on the retrieval plans).

1. The header against the ctypes table: names, argument counts, the struct layout; no other table holds the names; include_shared/ holds
   this one header; the 57 names and ABI 3 stay.
2. Every CRT_ERR_BAD_ARG / CRT_ERR_UNSUPPORTED of the entries is found before any launch (fake device pointers);
   crt_hip_lm_shared_max_nd equals the header's formula, is 0 for a refused npar or ns, and is the chain's limit at ns = 0.
3. The device-free errors of the two plans, the two one-shot functions and Model.retrieve_chain.
4. tests/lm_shared_reference.py: the long-double dense layer against a 50-digit mpmath solve of the same bordered system.
5. A linear-Gaussian twin: one step at lam = 0 of the fp64 restatement is the generalised least-squares solution of the stacked system,
   mean and covariance; the variance of a shared parameter is below its variance from any single date."""
import ctypes
import os
import re

import numpy as np
import pytest

import lm_shared_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NAMES = ["crt_hip_lm_shared_covariance_f64", "crt_hip_lm_shared_max_nd", "crt_hip_lm_step_shared_f64"]
U = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _raw():
    return open(os.path.join(ROOT, "include_shared", "crt1d_hip_lm_shared.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", _header())))
    assert names == sorted(_lib.SHARED_EXPORTS) == sorted(_lib._SHARED_SIGNATURES) == NAMES
    others = (_lib.EXPORTS, _lib.LEAF_EXPORTS, _lib.SPECTRA_EXPORTS, _lib.SENSOR_EXPORTS, _lib.JAC_EXPORTS, _lib.DLAI_EXPORTS, _lib.DLEAF_EXPORTS,
              _lib.GRAD_EXPORTS, _lib.SENSJAC_EXPORTS, _lib.SENSJAC_SERIES_EXPORTS, _lib.RETRIEVE_EXPORTS, _lib.SPECFIT_EXPORTS,
              _lib.SPECFIT_SERIES_EXPORTS, _lib.LEAFMODEL_EXPORTS, _lib.LUT_EXPORTS, _lib.LUT_POSTERIOR_EXPORTS, _lib.CHAIN_EXPORTS)
    for name in names:
        assert hasattr(lib, name) and not any(name in other for other in others)
    for name, (_, argtypes) in _lib._SHARED_SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert len(m.group(1).split(",")) == len(argtypes), name
    shared = os.path.join(ROOT, "include_shared")  # a directory of its own: the other five are held to their lists elsewhere
    assert sorted(os.path.relpath(os.path.join(d, f), shared) for d, _, files in os.walk(shared) for f in files) == ["crt1d_hip_lm_shared.h"]
    assert _header().count("typedef struct") == 1  # (the structs of the chain and of the step, reused)
    assert len(_lib.EXPORTS) == 57 and lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3
    assert len(_lib.CHAIN_EXPORTS) == 4


def test_struct_layout():
    from crt1d_amd import _lib

    m = re.search(r"typedef struct crt_lm_shared \{(.*?)\} crt_lm_shared;", _header(), re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint32_t mask;"
    S = _lib.CrtLmShared
    assert [f[0] for f in S._fields_] == ["mask"] and [f[1] for f in S._fields_] == [ctypes.c_uint32]
    assert S.mask.offset == 0 and ctypes.sizeof(S) == 4


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
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
    npar, mask0 = 3, 0b101
    big = lib.crt_hip_lm_shared_max_nd(npar, 2) + 1
    state = _lib.CrtLmState(*[FAKE] * 9)
    blocks = lambda n=1, hole=None: (_lib.CrtLmNormalBlock * 4)(*[_lib.CrtLmNormalBlock(*[None if hole == (q, i) else FAKE for i in range(3)])  # noqa: E731
                                                                  for q in range(min(n, 4))])

    def step(chain="default", prob="default", blk="default", nblk=1, st=state, npix=2, nd=big, stride=0, w=FAKE, mask=mask0, sh="default", **kw):
        ch = _lib.CrtLmChain(npix, nd, stride, w) if chain == "default" else chain
        pr = _problem(ncol=npix * nd, npar=npar, **kw) if prob == "default" else prob
        shared = _lib.CrtLmShared(mask) if sh == "default" else sh
        return lib.crt_hip_lm_step_shared_f64(ref(ch), ref(shared), ref(pr), blocks(nblk) if blk == "default" else blk, nblk, ref(st), None)

    assert step() == UNS and step(stride=(big - 1) * npar) == UNS and step(nblk=4) == UNS and step(npix=1) == UNS
    assert step(prior=FAKE, inv_sigma_prior=FAKE, lo=FAKE, hi=FAKE) == UNS
    assert step(sh=None) == BAD and step(mask=0b1000) == BAD and step(mask=0b1101) == BAD and step(mask=1 << 31) == BAD
    assert step(mask=0b110) == UNS  # (another set of two)
    for m in (0, 0b1, 0b111):  # the limit depends on ns: one beyond it each time
        assert step(mask=m, nd=lib.crt_hip_lm_shared_max_nd(npar, bin(m).count("1")) + 1) == UNS
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
    assert step(stride=1, nd=big + 5) == BAD and step(mask=0b1000, nd=big + 5) == BAD  # a bad argument wins over the limit

    def cov(chain="default", npar=npar, A=FAKE, out=FAKE, npix=2, nd=big, stride=0, w=FAKE, mask=mask0, sh="default"):
        ch = _lib.CrtLmChain(npix, nd, stride, w) if chain == "default" else chain
        shared = _lib.CrtLmShared(mask) if sh == "default" else sh
        return lib.crt_hip_lm_shared_covariance_f64(ref(ch), ref(shared), npar, A, out, None)

    assert cov() == UNS and cov(stride=(big - 1) * npar) == UNS
    assert cov(chain=None) == BAD and cov(A=None) == BAD and cov(out=None) == BAD and cov(npar=0) == BAD and cov(npar=11) == BAD
    assert cov(npix=0) == BAD and cov(nd=0) == BAD and cov(stride=7) == BAD and cov(w=None) == BAD
    assert cov(sh=None) == BAD and cov(mask=0b1000) == BAD and cov(mask=0b1000, nd=big + 5) == BAD


def test_max_nd_is_the_formula_of_the_header(lib):
    from crt1d_amd import _lib

    h = _raw()
    assert "8 * (nd * (nv ? 2 nv^2 + 4 nv + nv ns : 1) + 4 nv^2 + 64 + 3 ns^2 + 2 nv ns + 4 ns)" in h
    macro = re.search(r"#define CRT_LM_SHARED_LDS_BYTES\(nd, nv, ns\)(.*?)\n\n", _header(), re.S).group(1).replace("\\\n", " ")
    expr = macro.replace("(long long)", "").replace("?", " and (").replace(": 1)", ") or 1)")  # C's a ? b : 1 with b > 0 for a > 0
    for npar in range(1, 11):
        for ns in range(npar + 1):
            nv = npar - ns
            nd = lib.crt_hip_lm_shared_max_nd(npar, ns)
            assert nd == R.max_nd(npar, ns) == _lib.lm_shared_max_nd(npar, ns) >= 83
            assert _lib.lm_shared_lds_bytes(nd, nv, ns) <= 160 * 1024 < _lib.lm_shared_lds_bytes(nd + 1, nv, ns)
            for n in (1, nd):
                assert eval(expr, {}, dict(nd=n, nv=nv, ns=ns)) == _lib.lm_shared_lds_bytes(n, nv, ns) == R.lds_bytes(n, nv, ns)
        assert lib.crt_hip_lm_shared_max_nd(npar, 0) == lib.crt_hip_lm_chain_max_nd(npar)
        assert _lib.lm_shared_lds_bytes(7, npar, 0) == _lib.lm_chain_lds_bytes(7, npar)
    assert lib.crt_hip_lm_shared_max_nd(10, 5) == 212 and "212 at npar = 10, ns = 5" in h
    for npar, ns in ((0, 0), (-1, 0), (11, 0), (1000, 3), (5, -1), (5, 6), (10, 11)):
        assert lib.crt_hip_lm_shared_max_nd(npar, ns) == 0 == _lib.lm_shared_max_nd(npar, ns)


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def test_shared_python_errors_need_no_device():
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
    ch = dict(chain=3, inv_sigma_chain=np.ones((2, 3)))
    for make in makes:
        with pytest.raises(ValueError, match=r"shared names \['soil'\] are not among the parameters \('dir0', 'dir1', 'lai'\)"):
            make(d_leaf_r=d2, shared=("dir0", "soil"), **ch)
        with pytest.raises(ValueError, match="one entry for each of the 3 parameters"):
            make(d_leaf_r=d2, shared=np.array([True, False]), **ch)
        with pytest.raises(ValueError, match="one entry for each of the 3 parameters"):
            make(d_leaf_r=d2, shared=[True, False, True, False], **ch)
        with pytest.raises(ValueError, match="names or a boolean mask"):
            make(d_leaf_r=d2, shared=[0, 1], **ch)
        with pytest.raises(ValueError, match="shared needs chain="):
            make(d_leaf_r=d2, shared=("dir0",))
        with pytest.raises(ValueError, match="does not divide ncol = 6"):  # the chain's own checks still hold
            make(d_leaf_r=d2, shared=("dir0",), chain=4, inv_sigma_chain=np.ones((3, 3)))
    P = ("dir0", "dir1", "lai")
    assert batched._check_shared(None, None, P) is None and batched._check_shared(None, 3, P) is None
    assert batched._check_shared(("lai", "dir0"), 3, P) == 0b101 and batched._check_shared("dir1", 3, P) == 0b010
    assert batched._check_shared(np.array([False, True, True]), 3, P) == 0b110 and batched._check_shared(torch.tensor([True, True, True]), 3, P) == 0b111
    assert batched._check_shared((), 3, P) == 0 and batched._check_shared([False] * 3, 3, P) == 0

    # nd beyond crt_hip_lm_shared_max_nd: 212 at npar = 10 with 5 shared, where the chain alone stops at 83
    class Long:
        ncol, nz, device = 213, 6, "nowhere"

    names = tuple(f"dir{k}" for k in range(5))
    m5 = batched._check_shared(names, 213, names + ("dir5", "dir6", "dir7", "lai", "leaf"))
    assert m5 == 0b11111 and batched._check_chain(212, np.ones((211, 10)), 212, 10, m5) == (1, 212)
    with pytest.raises(ValueError, match="beyond the 83 the chain kernel serves"):
        batched._check_chain(212, np.ones((211, 10)), 212, 10)
    with pytest.raises(ValueError, match="beyond the 212 the shared-parameter kernel serves at npar = 10 with 5 shared"):
        batched._check_chain(213, np.ones((212, 10)), Long(), 10, m5)
    with pytest.raises(ValueError, match="beyond the 212"):
        batched.RetrievalPlan("2s", Long(), Bands(), (0,), sens, {"I_df_u": np.ones((213, 1, 1))}, keys=("I_df_u",), d_leaf_r=np.ones((8, 8)), leaf=True,
                              chain=213, inv_sigma_chain=np.ones((212, 10)), shared=names)
    with pytest.raises(ValueError, match="beyond the 212"):
        batched.retrieve_spectral("2s", Long(), Bands(), (0,), {"I_df_u": np.ones((213, 1, 8))}, keys=("I_df_u",), d_leaf_r=np.ones((8, 8)), leaf=True,
                                  chain=213, inv_sigma_chain=np.ones((212, 10)), shared=names)

    m = Model("2s", nlayers=6)
    w = np.ones((2, m.nwl))
    y = {"I_df_u": np.ones((3, 1, 2))}
    psi = np.deg2rad([10.0, 30.0, 50.0])
    d = {"leaf_r": np.ones((1, m.nwl))}
    with pytest.raises(ValueError, match=r"shared names \['leaf'\] are not among the parameters \('dir0', 'lai'\)"):
        m.retrieve_chain(w, y, psi, np.ones((2, 2)), levels=(-1,), directions=d, shared=("leaf",))
    with pytest.raises(ValueError, match="one entry for each of the 2 parameters"):
        m.retrieve_chain(w, y, psi, np.ones((2, 2)), levels=(-1,), directions=d, shared=[True])
    with pytest.raises(ValueError, match=r"inv_sigma_chain must be \(2, 2\) or \(1, 2, 2\)"):  # (after the shared set was understood)
        m.retrieve_chain(w, y, psi, np.ones((3, 2)), levels=(-1,), directions=d, shared=("dir0",))


# ---- 4. / 5. ----------------------------------------------------------------------------------------------------------------------------
def _twin(rng, nd, npar, mask, nrow=None):
    """A linear twin: J (nd, nrow, npar), y, the weights, a point p whose shared columns agree over the dates, and the sums there."""
    nrow = nrow or 3 * npar
    _, ks = R.split(mask, npar)
    J = rng.normal(size=(nd, nrow, npar))
    y = rng.normal(size=(nd, nrow))
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    w[:, ks] = np.nan  # never read
    p = 0.3 * rng.normal(size=(nd, npar))
    p[:, ks] = p[0, ks]
    r = np.einsum("dok,dk->do", J, p) - y
    return J, y, w, p, (R.pack(np.einsum("doi,doj->dij", J, J)), np.einsum("doi,do->di", J, r), np.einsum("do,do->d", r, r))


def _mp(v):
    import mpmath as mp

    v = LD(v)
    hi = np.float64(v)
    return mp.mpf(float(hi)) + mp.mpf(float(v - hi))


@pytest.mark.parametrize("mask", [0b01, 0b10, 0b11, 0b00])
def test_long_double_layer_against_mpmath(mask):
    """nd = 3, npar = 2, lam = 1e-2: H and G of the header (the varying part, the border, the corner) restated in 50-digit arithmetic from
    the same fp64 inputs, the damped solve, the inverse and the cost.  The long-double Cholesky solve of n <= 6 unknowns has a relative
    error of order n^2 u_ld kappa (u_ld = 2^-64, kappa of order 10^2): 1e-15 of the largest entry is asserted, six orders below the fp64
    results it referees."""
    import mpmath as mp

    mp.mp.dps = 50
    nd, npar, lam = 3, 2, 1e-2
    _, _, w, p, (A, g, c2) = _twin(np.random.default_rng(5 + mask), nd, npar, mask)
    kv, ks = R.split(mask, npar)
    nv, ns = len(kv), len(ks)
    N = nd * nv
    n = N + ns
    pos = lambda d, k: d * nv + kv.index(k) if k in kv else N + ks.index(k)  # noqa: E731
    f = lambda v: mp.mpf(float(v))  # noqa: E731
    H, G = mp.zeros(n, n), mp.zeros(n, 1)
    for d in range(nd):  # every date's A_d and g_d land on the unknowns of (v_d, s): the corner and G_s collect the sums over the dates
        for a in range(npar):
            G[pos(d, a)] += f(g[d, a])
            for b in range(npar):
                H[pos(d, a), pos(d, b)] += f(A[d, R.tri(max(a, b), min(a, b))])
    for d in range(nd - 1):
        for k in kv:
            a, b, w2 = pos(d, k), pos(d + 1, k), f(w[d, k]) ** 2
            e = (f(p[d + 1, k]) - f(p[d, k])) * w2
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
    got = R.solve_ld(A, g, p, w, lam, mask)
    scale = max(abs(delta[r]) for r in range(n))
    assert max(abs(_mp(got[r]) - delta[r]) for r in range(n)) < 1e-15 * scale
    inv = H ** -1
    X = R.inverse_ld(A, w, mask)
    scale = max(abs(inv[r, q]) for r in range(n) for q in range(n))
    assert max(abs(_mp(X[r, q]) - inv[r, q]) for r in range(n) for q in range(n)) < 1e-15 * scale
    for d in range(nd):  # the marginal of (v_d, s) in the original order
        blk = R.marginal(X, d, nd, npar, mask)
        for a in range(npar):
            for b in range(npar):
                assert blk[a, b] == X[pos(d, a), pos(d, b)]
    cost = (sum(f(v) for v in c2) + sum(((f(p[d + 1, k]) - f(p[d, k])) * f(w[d, k])) ** 2 for d in range(nd - 1) for k in kv)) / 2
    assert abs(_mp(R.cost_ld(c2, p, w, mask)) - cost) < 2e-16 * cost
    assert abs(R.pixel_cost(c2, p, w, mask) - float(cost)) <= 2 * (nd + (nd - 1) * nv) * U * float(cost)
    # the fp64 restatement of the bordered solve agrees with it within the bound the GPU test uses for the kernel
    dv, ds = R.bordered_solve(A, g, p, w, lam, mask)
    fp = np.concatenate([dv.reshape(-1), ds])
    _, _, s = R.dense_ld(A, g, p, w, lam, mask)
    x = np.array([float(delta[r]) for r in range(n)]) / s.astype(np.float64)
    bound, s, _, _, _ = R.solve_bound(A, g, p, w, lam, mask, float(np.linalg.norm(x)))
    assert max(abs(float(fp[r]) - float(delta[r])) / (s[r] * bound + U * abs(float(delta[r]))) for r in range(n)) <= 1.0
    if mask == 0:  # and with nothing shared it is the chain's restatement, bit for bit
        import lm_chain_reference as RC

        assert dv.tobytes() == RC.band_solve(A, g, p, w, lam).tobytes()


def _gls(J, y, w, mask):
    """The stacked system in long double: the rows of every date on the columns of (v_d, s), then the random-walk rows
    w_{d,k} (v_{d+1,k} - v_{d,k}) = 0.  -> (theta (n,), (X^T X)^-1 (n, n)), by a long-double Cholesky of the normal equations."""
    nd, nrow, npar = J.shape
    kv, ks = R.split(mask, npar)
    nv, ns = len(kv), len(ks)
    N = nd * nv
    n = N + ns
    rows, rhs = [], []
    for d in range(nd):
        for o in range(nrow):
            row = np.zeros(n, dtype=LD)
            row[d * nv:(d + 1) * nv] = J[d, o, kv]
            row[N:] = J[d, o, ks]
            rows.append(row), rhs.append(LD(y[d, o]))
    for d in range(nd - 1):
        for j, k in enumerate(kv):
            row = np.zeros(n, dtype=LD)
            row[d * nv + j], row[(d + 1) * nv + j] = -LD(w[d, k]), LD(w[d, k])
            rows.append(row), rhs.append(LD(0))
    X, b = np.array(rows, dtype=LD), np.array(rhs, dtype=LD)
    # (X^T X in long double, summed term by term: numpy has no long-double BLAS and its einsum keeps the dtype)
    XtX, Xtb = np.einsum("oi,oj->ij", X, X), np.einsum("oi,o->i", X, b)
    L = R.cholesky_ld(XtX)
    inv = np.stack([R._solve_ld(L, np.eye(n, dtype=LD)[:, r]) for r in range(n)], axis=1)
    return R._solve_ld(L, Xtb), inv


@pytest.mark.parametrize("nd,npar,mask", [(1, 2, 0b01), (4, 1, 0b1), (5, 3, 0b011), (5, 3, 0b100), (3, 5, 0b10101), (4, 3, 0b000), (3, 4, 0b1111)])
def test_one_undamped_step_is_generalised_least_squares(nd, npar, mask):
    """y_d = J_d (v_d, s) + N(0, I), v_{d+1} = v_d + N(0, diag(1 / w_d^2)): the cost of the header is the quadratic form of the stacked
    system, so ONE step at lam = 0 from anywhere lands on its generalised least-squares solution, and the inverse of H is its
    covariance.  The mean: within the bound of the GPU test (solve_bound of the reference: Higham's 4 n (3 n + 1) u kappa_2(M) and the
    roundings of forming M and G), per entry s_r * bound + u (|delta_r| + |p_trial_r|).  The covariance of the long-double layer against
    (X^T X)^-1: within the factor's bound doubled.  And the point of sharing: the variance of a shared parameter is below its variance
    from any single date."""
    rng = np.random.default_rng(600 + 10 * nd + npar + mask)
    J, y, w, p, blocks = _twin(rng, nd, npar, mask)
    kv, ks = R.split(mask, npar)
    nv, ns = len(kv), len(ks)
    n = nd * nv + ns
    opt = dict(lam_up=10.0, lam_down=0.1, lam_min=0.0, lam_max=1e12, xtol=0.0, ftol=0.0)
    st = R.step(R.new_state(p, 0.0), [blocks], w, opt, mask)
    assert st["naccept"] == 1 and st["lam"] == 0.0 and st["status"] == R.RUNNING
    assert all(st["p_trial"][:, k].tobytes() == np.repeat(st["p_trial"][0, k], nd).tobytes() for k in ks)
    theta, cov = _gls(J, y, w, mask)
    want = R.full_delta(theta, nd, npar, mask)
    A, g = st["A"], st["g"]
    _, _, s = R.dense_ld(A, g, p, w, 0.0, mask)
    flat = lambda v: np.concatenate([np.asarray(v)[:, kv].reshape(-1), np.asarray(v)[0, ks]])  # noqa: E731
    delta = flat(want) - flat(p).astype(LD)
    bound, s64, c, lo, hi = R.solve_bound(A, g, p, w, 0.0, mask, float(np.linalg.norm((delta / s).astype(np.float64))))
    err = np.abs(flat(st["p_trial"]).astype(LD) - flat(want)).astype(np.float64)
    allowed = s64 * bound + U * (np.abs(delta.astype(np.float64)) + np.abs(flat(st["p_trial"])))
    assert np.all(err <= allowed), float((err / allowed).max())
    X = R.inverse_ld(A, w, mask)
    cb = 2 * c * U * (hi / lo) / lo * s64[:, None] * s64[None, :]
    assert np.all(np.abs(X - cov).astype(np.float64) <= cb)
    for i, k in enumerate(ks):
        joint = float(X[nd * nv + i, nd * nv + i])
        for d in range(nd if nd > 1 else 0):  # (with one date the joint system IS that date)
            alone = np.linalg.inv(J[d].T @ J[d])[k, k]  # date d alone: (v_d, s) from its own rows
            assert joint < alone, (k, d, joint, alone)
