"""GPU: the date-by-date retrieval (include_seq/crt1d_hip_lm_seq.h) through its C entries, then through the plans.

1. The prior block: bitwise the fp64 restatement of tests/lm_seq_reference.py, within rounding of long double, a column alone.
2. crt_hip_lm_step_normal_f64 fed the block against the same entry with the diagonal prior of crt_lm_problem.
3. crt_hip_lm_predict_f64 against the long-double parallel sum in a stiff case; forget, dead and non-PD columns.
4. crt_hip_lm_rts_f64 against the long-double recursion; a non-PD date; a pixel alone.
5. Filter plus sweep against the dense chain system on a linear-Gaussian problem, also one date past the chain kernel's limit.
6. The plans on the radiative transfer (the twin of tests/test_gpu_lm_chain.py).

THE BOUNDS (u = 2^-53, n = npar, c = 4 n (3 n + 1) + 8 n as derived in tests/test_gpu_lm_chain.py for a scaled Cholesky solve of order n;
Ms the scaled matrix the kernel factorises, s = 1 / sqrt(diag), kappa_2 its condition number).
 predict: P = W M^-1 A.  In the scaled domain S P S = Ws (Ms^-1 As) with Ws = S W S <= I and As = S A S <= Ms, so the backward error of
   the npar solves moves S P S by at most c u kappa_2(Ms) in norm, relative to the norm of what is computed; the last three roundings
   (two products, the mean) are relative to the entry.  Asserted: s_i s_j |dP_ij| <= c u kappa_2(Ms) ||S P S||_2, plus 2^-11 of that for
   the long-double reference (the same product form at u_ld = 2^-64).
 sweep, covariance: date t adds the error of its own inverse, at most 2 c u kappa_2(Ms_t) ||M_t^-1||_2 (the allowance of the chain's
   covariance test), and carries the error of the dates behind it through G C G^T with G = M^-1 W, a contraction in the M-norm.  The
   accumulated bound asserted at date t is  E_t = sum_{t' >= t} 2 c u kappa_2(Ms_t') ||M_t'^-1||_2  (the last date: A_f in place of M).
 sweep, mean: p_s,t = p_f,t + G d.  dG = dM^-1 W gives ||dM^-1||_2 ||W||_2 ||d||_2, the error of p_s,t+1 is carried through G, and the
   npar-term sum and the final addition round: B_t = 2 c u kappa_2 ||M^-1||_2 ||W||_2 ||d||_2 + ||G||_2 B_{t+1} + (n + 2) u (|p_f| + |G| |d|).
Measured on MI355X, largest error / bound: see DESIGN.md 3.31."""
import ctypes

import numpy as np
import pytest

import lm_chain_reference as R
import lm_seq_reference as Q
from test_gpu_lm_chain import Chain, Sums, _dev_sums, _linear_case, _ptr, _series_problem, _solve_bound, _stream
from test_gpu_retrieve import STATE, _same, _t

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def _c(n):
    return 4 * n * (3 * n + 1) + 8 * n


def _lib():
    from crt1d_amd import _lib

    return _lib, _lib.load()


def _out(shape, dtype=None, fill=np.nan):
    import torch

    return torch.full(shape, fill, dtype=dtype or torch.float64, device="cuda")


def prior_block(P, mean, p, expect=0):
    """P (ncol or 1, ntri), mean, p (ncol, npar) on the host -> A, g, c2 on the host."""
    import torch

    L, lib = _lib()
    ncol, npar = mean.shape
    ntri = npar * (npar + 1) // 2
    Pd, md, pd = _t(P), _t(mean), _t(p)
    A, g, c2 = _out((ncol, ntri)), _out((ncol, npar)), _out((ncol,))
    pr = L.CrtLmPriorFull(ncol, npar, 0 if P.shape[0] == 1 and ncol != 1 else ntri, _ptr(Pd), _ptr(md))
    assert lib.crt_hip_lm_prior_block_f64(ctypes.byref(pr), _ptr(pd), _ptr(A), _ptr(g), _ptr(c2), _stream()) == expect
    torch.cuda.synchronize()
    return A.cpu().numpy(), g.cpu().numpy(), c2.cpu().numpy()


def predict(A, w):
    """A (ncol, ntri), w (ncol or 1, npar) -> precision (ncol, ntri), info (ncol,)."""
    import torch

    L, lib = _lib()
    ncol, ntri = A.shape
    npar = w.shape[1]
    Ad, wd = _t(A), _t(w)
    prec, info = _out((ncol, ntri)), _out((ncol,), torch.int32, -1)
    assert lib.crt_hip_lm_predict_f64(ncol, npar, _ptr(Ad), _ptr(wd), 0 if w.shape[0] == 1 and ncol != 1 else npar, _ptr(prec), _ptr(info),
                                      _stream()) == 0
    torch.cuda.synchronize()
    return prec.cpu().numpy(), info.cpu().numpy()


def rts(p_f, A_f, w):
    """p_f (npix, nd, npar), A_f (npix, nd, ntri), w (nd - 1, npar) or (npix, nd - 1, npar) -> p_s, cov_s (npix, nd, npar, npar), info."""
    import torch

    L, lib = _lib()
    npix, nd, npar = p_f.shape
    pd, Ad, wd = _t(p_f), _t(A_f), _t(w) if nd > 1 else None
    p_s, cov, info = _out((npix, nd, npar)), _out((npix, nd, npar, npar)), _out((npix,), torch.int32, -1)
    ch = L.CrtLmChain(npix, nd, 0 if w.ndim == 2 else (nd - 1) * npar, _ptr(wd))
    assert lib.crt_hip_lm_rts_f64(ctypes.byref(ch), npar, _ptr(pd), _ptr(Ad), _ptr(p_s), _ptr(cov), _ptr(info), _stream()) == 0
    torch.cuda.synchronize()
    return p_s.cpu().numpy(), cov.cpu().numpy(), info.cpu().numpy()


def covariance(A):
    import torch

    L, lib = _lib()
    ncol, ntri = A.shape
    npar = int(round((np.sqrt(8 * ntri + 1) - 1) / 2))
    Ad, cov = _t(A), _out((ncol, npar, npar))
    assert lib.crt_hip_lm_covariance_f64(ncol, npar, _ptr(Ad), _ptr(cov), _stream()) == 0
    torch.cuda.synchronize()
    return cov.cpu().numpy()


def _spd(rng, n, kappa):
    Qm, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Qm * np.logspace(0.0, -np.log10(kappa), n)) @ Qm.T


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("ncol", [1, 64, 65, 130])
@pytest.mark.parametrize("npar", [1, 3, 10])
def test_prior_block(npar, ncol, shared):
    rng = np.random.default_rng(100 * npar + ncol + shared)
    P = np.stack([R.pack(_spd(rng, npar, 1e3) * rng.uniform(0.1, 10.0)) for _ in range(1 if shared else ncol)])
    mean, p = rng.normal(size=(ncol, npar)), rng.normal(size=(ncol, npar))
    A, g, c2 = prior_block(P, mean, p)
    for c in range(ncol):
        Pc = P[0 if shared else c]
        Ar, gr, cr = Q.prior_block(Pc, mean[c], p[c])
        assert A[c].tobytes() == Pc.tobytes() == Ar.tobytes() and g[c].tobytes() == gr.tobytes() and c2[c].tobytes() == np.float64(cr).tobytes(), c
        gl, cl, gb, cb = Q.prior_block_ld(Pc, mean[c], p[c])
        assert np.all(np.abs(g[c].astype(LD) - gl) <= (npar + 2) * U * gb) and abs(LD(c2[c]) - cl) <= (2 * npar + 3) * U * cb
    c = 37 if ncol > 37 else 0
    A1, g1, c21 = prior_block(P if shared else P[c:c + 1], mean[c:c + 1], p[c:c + 1])
    assert A1.tobytes() == A[c].tobytes() and g1.tobytes() == g[c].tobytes() and c21.tobytes() == c2[c:c + 1].tobytes()


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npar", [1, 3, 10])
def test_step_with_the_block(npar):
    """[the data's sums, the prior block with P = diag(s^2)] against the data's sums and inv_sigma_prior = s: the same cost up to the
    rounding of npar + 2 more terms on either side, the same A up to one rounding on either side; a block of +0: the plain call's bits."""
    ncol = 65
    rng = np.random.default_rng(200 + npar)
    p0 = 0.1 * rng.normal(size=(ncol, npar))
    sums = _dev_sums(_linear_case(rng, ncol, 1, npar)(p0))
    mean, s = rng.normal(size=(ncol, npar)), rng.uniform(0.5, 2.0, (ncol, npar))
    i, j = np.tril_indices(npar)
    P = np.zeros((ncol, len(i)))
    P[:, i == j] = s * s
    blk = tuple(_t(v) for v in prior_block(P, mean, p0))
    a = Chain(ncol, None, _t(p0)).step(sums + [blk]).snap()
    b = Chain(ncol, None, _t(p0), prior=_t(mean), isp=_t(s)).step(sums).snap()
    assert np.all(a["naccept"] == 1) and np.all(b["naccept"] == 1)
    assert np.all(np.abs(a["cost"] - b["cost"]) <= 2 * (npar + 2) * U * b["cost"])
    assert np.all(np.abs(a["A"] - b["A"]) <= 2 * U * np.abs(b["A"]))
    zero = tuple(_t(v) for v in prior_block(np.zeros((ncol, len(i))), mean, p0))
    assert all(not v.cpu().numpy().any() and not np.signbit(v.cpu().numpy()).any() for v in zero)
    plain = Chain(ncol, None, _t(p0))
    with0 = Chain(ncol, None, _t(p0))
    for it in range(3):
        plain.step(sums)
        with0.step(sums + [zero])
        assert _same(plain.snap(), with0.snap()), it


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
FORGET, DEAD, NOTPD = 3, 5, 7


def _predict_case(npar):
    """65 columns: A random SPD with kappa = 10^[0, 6], w log-spaced over 1e-3 .. 1e5 within a column (npar = 1: over the columns), the
    order shuffled.  Column FORGET has w_k = 0 for one k, column DEAD a dead A_kk = 0 (zero row and column) with w_k = 0, column NOTPD is
    not positive definite (npar = 1: NaN, since a non-positive 1 x 1 matrix with w = 0 is a dead entry, not a failing pivot)."""
    ncol = 65
    rng = np.random.default_rng(300 + npar)
    A = np.stack([_spd(rng, npar, 10.0 ** rng.uniform(0.0, 6.0)) for _ in range(ncol)])
    if npar > 1:
        w = np.stack([rng.permutation(np.logspace(-3, 5, npar)) for _ in range(ncol)])
    else:
        w = np.logspace(-3, 5, ncol)[:, None]
    k = npar // 2
    w[FORGET, k] = 0.0
    w[DEAD, k] = 0.0
    A[DEAD, k, :] = A[DEAD, :, k] = 0.0
    if npar > 1:
        A[NOTPD] = A[NOTPD] + 50.0 * np.abs(A[NOTPD]).max() * (1.0 - np.eye(npar))
        w[NOTPD] = 1e-3
    else:
        A[NOTPD] = np.nan
    return R.pack(A), w, k


def _predict_fraction(npar):
    """The case of the test: every assertion but the last.  -> the largest error / bound"""
    A, w, k = _predict_case(npar)
    ncol = A.shape[0]
    i, j = np.tril_indices(npar)
    got, info = predict(A, w)
    assert list(np.nonzero(info)[0]) == [NOTPD] and info[NOTPD] == 1
    assert not got[NOTPD].any() and not np.signbit(got[NOTPD]).any()
    worst = 0.0
    for c in range(ncol):
        if c == NOTPD:
            continue
        zero = (w[c] == 0.0)
        touched = zero[i] | zero[j]
        assert not got[c][touched].any() and not np.signbit(got[c][touched]).any(), c  # exactly +0
        if zero.all():  # (npar = 1: nothing is handed over at all, which the line above has checked)
            continue
        ref = Q.parallel_sum_ld(A[c], w[c])
        M = Q.unpack(A[c]) + np.diag(w[c] ** 2)
        alive = np.diagonal(M) > 0.0  # what the kernel factorises: everything but a dead entry, a forgotten parameter included
        sub = M[np.ix_(alive, alive)]
        lo, hi = Q.scaled_extremes(sub)
        s = np.ones(npar)
        s[alive] = 1.0 / np.sqrt(np.diagonal(sub))
        Ps = (ref * s[:, None] * s[None, :]).astype(np.float64)
        bound = _c(npar) * U * (hi / lo) * np.linalg.norm(Ps, 2) * (1.0 + 2.0 ** -11)
        assert 0.0 < bound < 1e-6, (c, bound)  # (of the inputs: the bound means something)
        err = (np.abs(Q.unpack(got[c], LD) - ref) * s[:, None] * s[None, :]).astype(np.float64)
        worst = max(worst, float(err.max() / bound))
    return worst


@pytest.mark.parametrize("npar", [1, 5, 10])
def test_predict_against_long_double(npar):
    worst = _predict_fraction(npar)
    print(f"predict npar={npar}: largest error / bound = {worst:.3e}")
    assert worst <= 1.0


def test_predict_shared_weights_and_a_column_alone():
    npar = 5
    A, w, _ = _predict_case(npar)
    got, info = predict(A, w)
    one, i1 = predict(A[37:38], w[37:38])
    assert one.tobytes() == got[37].tobytes() and i1[0] == info[37] == 0
    same, _ = predict(A, w[37:38])  # stride 0: one row of weights for every column
    again, _ = predict(A, np.repeat(w[37:38], A.shape[0], axis=0))
    assert same.tobytes() == again.tobytes()


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def _rts_case(nd, npar, npix):
    """Filtered dates as a filter leaves them: A_f = J^T J of 3 npar rows plus a prior precision of order 1, p_f random; weights in
    [0.5, 2], one set for all pixels where nd + npar is even."""
    rng = np.random.default_rng(400 + 100 * nd + 10 * npar + npix)
    J = rng.normal(size=(npix, nd, 3 * npar, npar))
    A = np.einsum("pdoi,pdoj->pdij", J, J) + np.stack([[_spd(rng, npar, 10.0) for _ in range(nd)] for _ in range(npix)])
    p_f = rng.normal(size=(npix, nd, npar))
    w = rng.uniform(0.5, 2.0, (nd - 1, npar) if (nd + npar) % 2 == 0 else (npix, nd - 1, npar))
    return p_f, R.pack(A), w


def _rts_bounds(p_f, A_f, w, ps_ref, Cs_ref):
    """-> (B (nd, npar), E (nd,)): the accumulated bounds of the module docstring for one pixel, from the reference's own quantities."""
    nd, npar = p_f.shape
    c = _c(npar)
    lo, hi = Q.scaled_extremes(Q.unpack(A_f[-1]))
    E = np.zeros(nd)
    B = np.zeros((nd, npar))
    E[-1] = 2 * c * U * (hi / lo) * np.linalg.norm(np.linalg.inv(Q.unpack(A_f[-1])), 2)
    for t in reversed(range(nd - 1)):
        q = w[t] ** 2
        M = Q.unpack(A_f[t]) + np.diag(q)
        lo, hi = Q.scaled_extremes(M)
        Mi = np.linalg.inv(M)
        own = 2 * c * U * (hi / lo) * np.linalg.norm(Mi, 2)
        E[t] = E[t + 1] + own
        G = Mi * q[None, :]
        d = (ps_ref[t + 1] - p_f[t]).astype(np.float64)
        B[t] = own * q.max() * np.linalg.norm(d) + np.linalg.norm(G, 2) * B[t + 1].max() + (npar + 2) * U * (np.abs(p_f[t]) + np.abs(G) @ np.abs(d))
    return B, E


def _rts_fractions(nd, npar, npix):
    """The case of the test: every assertion but the last two.  -> the largest error / bound of (p_s, cov_s)"""
    p_f, A_f, w = _rts_case(nd, npar, npix)
    p_s, cov, info = rts(p_f, A_f, w)
    assert not info.any() and np.all(np.isfinite(p_s)) and np.all(np.isfinite(cov))
    last = covariance(A_f[:, -1])
    assert cov[:, -1].tobytes() == last.tobytes() and p_s[:, -1].tobytes() == p_f[:, -1].tobytes()
    assert np.array_equal(cov[:, :-1], np.swapaxes(cov[:, :-1], 2, 3))  # (the sweep mirrors; the last date is k_lm_covariance's)
    fp, fc = 0.0, 0.0
    for pix in sorted({0, npix // 2, npix - 1}):
        wp = w if w.ndim == 2 else w[pix]
        ps_ref, Cs_ref = Q.rts_ld(p_f[pix], A_f[pix], wp)
        B, E = _rts_bounds(p_f[pix], A_f[pix], wp, ps_ref, Cs_ref)
        assert E.max() < 1e-6 and B.max() < 1e-6  # (of the inputs: the bounds mean something)
        ec = np.abs(cov[pix].astype(LD) - Cs_ref).astype(np.float64).reshape(nd, -1).max(1)
        fc = max(fc, float((ec / E).max()))
        if nd > 1:
            ep = np.abs(p_s[pix, :-1].astype(LD) - ps_ref[:-1]).astype(np.float64)
            fp = max(fp, float((ep / B[:-1]).max()))
    # a pixel alone gives the bits it has in the batch
    pix = npix // 2
    a_p, a_c, a_i = rts(p_f[pix:pix + 1], A_f[pix:pix + 1], w if w.ndim == 2 else w[pix:pix + 1])
    assert a_p.tobytes() == p_s[pix].tobytes() and a_c.tobytes() == cov[pix].tobytes() and a_i[0] == 0
    return fp, fc


@pytest.mark.parametrize("npix", [1, 65])
@pytest.mark.parametrize("nd,npar", [(1, 10), (2, 1), (7, 3), (12, 5), (84, 10)])
def test_rts_against_long_double(nd, npar, npix):
    """The accumulated bounds E_t (covariance) and B_t (mean) of the module docstring, on the first, the middle and the last pixel.
    nd = 1: cov_s is crt_hip_lm_covariance_f64's bits and p_s = p_f's (asserted for the last date of every case)."""
    fp, fc = _rts_fractions(nd, npar, npix)
    print(f"rts nd={nd} npar={npar} npix={npix}: largest error / bound: p_s {fp:.3e}, cov_s {fc:.3e}")
    assert fp <= 1.0 and fc <= 1.0


@pytest.mark.parametrize("nd,npar", [(2, 1), (7, 3), (12, 5)])
def test_rts_with_a_date_that_is_not_positive_definite(nd, npar):
    """Date t of pixel 1 is spoilt (npar > 1: large off-diagonal entries, a failing pivot; npar = 1: a negative entry, a dead diagonal
    of A + W): info = 1 + t, NaN on the dates <= t, the later dates keep the bits of the clean run; the other pixels are not affected."""
    npix, t = 3, (nd - 2) // 2
    p_f, A_f, w = _rts_case(nd, npar, npix)
    clean_p, clean_c, _ = rts(p_f, A_f, w)
    bad = Q.unpack(A_f[1, t])
    bad = bad + 50.0 * np.abs(bad).max() * (1.0 - np.eye(npar)) if npar > 1 else -10.0 - bad
    A_f[1, t] = R.pack(bad)
    p_s, cov, info = rts(p_f, A_f, w)
    assert list(info) == [0, 1 + t, 0]
    assert np.all(np.isnan(p_s[1, :t + 1])) and np.all(np.isnan(cov[1, :t + 1]))
    assert p_s[1, t + 1:].tobytes() == clean_p[1, t + 1:].tobytes() and cov[1, t + 1:].tobytes() == clean_c[1, t + 1:].tobytes()
    assert p_s[[0, 2]].tobytes() == clean_p[[0, 2]].tobytes() and cov[[0, 2]].tobytes() == clean_c[[0, 2]].tobytes()


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
def _filter_through_the_entries(rng, npix, nd, npar):
    """A linear-Gaussian series through the C entries.  Per date: rows (f = J p, J, y) -> crt_hip_lm_normal_f64; the prior block (date 0:
    a full Gaussian prior of the test's; later: the predicted precision around the previous filtered point); two calls of
    crt_hip_lm_step_normal_f64 at lam = 0 -- the first is accepted and lands on the Gauss-Newton point, the second accepts it --; then
    crt_hip_lm_predict_f64.  -> dict of host arrays: p_f, A_f (stored, prior included), the data part (A_d, g_d at p_f; date 0 with its
    prior), J, y, w, and the residual budget of the two evaluations"""
    nrow = 3 * npar
    J = rng.normal(size=(nd, npix, nrow, npar)) * rng.uniform(0.5, 2.0, npar)
    y = rng.normal(size=(nd, npix, nrow))
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    m0 = rng.normal(size=(npix, npar))
    P0 = np.stack([R.pack(_spd(rng, npar, 10.0) * 2.0) for _ in range(npix)])
    ntri = npar * (npar + 1) // 2
    p_f, A_f = np.zeros((npix, nd, npar)), np.zeros((npix, nd, ntri))
    A_d, g_d, budget = np.zeros((npix, nd, ntri)), np.zeros((npix, nd, npar)), np.zeros((npix, nd, npar))
    mean, prec = m0, P0
    start = 0.1 * rng.normal(size=(npix, npar))
    for t in range(nd):
        st = Chain(npix, None, _t(start), lam0=0.0, lam_min=0.0)
        for call in range(2):
            pt = st.snap()["p_trial"]
            f = np.einsum("cok,ck->co", J[t], pt)
            blocks = [dict(J=_t(J[t]), f=_t(f), y=_t(y[t]), s=None)]
            data = Sums(blocks, npar).out[0]
            blk = tuple(_t(v) for v in prior_block(prec, mean, pt))
            st.step([data, blk])
            budget[:, t] += (nrow + 2) * U * np.einsum("cok,co->ck", np.abs(J[t]), np.abs(f - y[t]))
        got = st.snap()
        assert np.all(got["naccept"] == 2) and np.all(got["lam"] == 0.0) and np.array_equal(got["p"], pt)
        p_f[:, t], A_f[:, t] = got["p"], got["A"]
        A_d[:, t], g_d[:, t] = data[0].cpu().numpy(), data[1].cpu().numpy()
        if t == 0:  # the prior of date 0 belongs to the dense system: the stored sums of both blocks
            A_d[:, 0], g_d[:, 0] = got["A"], got["g"]
        if t < nd - 1:
            prec, info = predict(got["A"], w[t:t + 1])
            assert not info.any()
            mean = start = got["p"]
    return dict(p_f=p_f, A_f=A_f, A_d=A_d, g_d=g_d, w=w, budget=budget)


@pytest.mark.parametrize("nd,npar", [(7, 3), (12, 5), (84, 10)])
def test_filter_and_sweep_equal_the_chain_on_a_linear_problem(nd, npar):
    """p_s against p_f + solve_ld of the dense chain system linearised at p_f (on a linear problem: the minimiser, from any point), the
    diagonal blocks of cov_s against the dense inverse -- within the solve bound and the covariance bound of tests/test_gpu_lm_chain.py
    for the dense system (n = nd npar).  The sums g of the rows are the kernel's: their rounding, (nrow + 2) u |J|^T |r| for each of
    the two evaluations of a date, moves the minimiser by at most ||.||_2 / lambda_min(M) in the scaled system and is added to the
    solve bound.  (84, 10) is one date past what crt_hip_lm_step_chain_f64 serves (asserted); there the dense inverse is formed for the
    block columns of three dates and the long-double block-tridiagonal solve (held to the dense one in the CPU tests) covers the rest."""
    from crt1d_amd import _lib

    npix = 2
    rng = np.random.default_rng(500 + 10 * nd + npar)
    F = _filter_through_the_entries(rng, npix, nd, npar)
    p_s, cov, info = rts(F["p_f"], F["A_f"], F["w"])
    assert not info.any()
    if nd > R.max_nd(npar):
        assert (nd, npar) == (84, 10)
        ch = Chain(npix, nd, _t(F["p_f"].reshape(npix * nd, npar)), w=_t(F["w"]))
        z = np.zeros((npix * nd, 1))
        ch.step(_dev_sums([(F["A_d"].reshape(npix * nd, -1), F["g_d"].reshape(npix * nd, -1), z[:, 0])]), expect=_lib.CRT_ERR_UNSUPPORTED)
    worst_p, worst_c = 0.0, 0.0
    n = nd * npar
    for pix in ((1,) if nd > 12 else range(npix)):
        A, g, p, w = F["A_d"][pix], F["g_d"][pix], F["p_f"][pix], F["w"]
        delta = R.solve_ld(A, g, p, w, 0.0)
        bound = _solve_bound(A, g, p, w, 0.0, delta, p_s[pix])
        lo, hi = R.scaled_extremes(A, w, 0.0)
        _, _, s = R.dense_ld(A, g, p, w, 0.0)
        s = s.astype(np.float64).reshape(nd, npar)
        bound = bound + s * np.linalg.norm(F["budget"][pix] * s) / lo
        assert bound.max() < 1e-6
        err = np.abs(p_s[pix].astype(LD) - p.astype(LD) - delta).astype(np.float64)
        worst_p = max(worst_p, float((err / bound).max()))
        dates = range(nd) if nd <= 12 else (0, nd // 2, nd - 1)
        cols = Q.dense_columns_ld(A, w, dates)
        _, S = Q.block_tridiagonal_ld(A, -g, w)
        for d in range(nd):
            ref = cols[d][d * npar:(d + 1) * npar] if d in cols else S[d]
            cb = 2 * _c(n) * U * (hi / lo) / lo * s[d][:, None] * s[d][None, :]
            assert cb.max() < 1e-6
            worst_c = max(worst_c, float((np.abs(cov[pix, d].astype(LD) - ref).astype(np.float64) / cb).max()))
    print(f"filter + sweep nd={nd} npar={npar}: largest error / bound: p_s {worst_p:.3e}, cov_s {worst_c:.3e}")
    assert worst_p <= 1.0 and worst_c <= 1.0


# ---- 6. the plans on the radiative transfer ------------------------------------------------------------------------------------------------
NSTEP = 15
BOX = 0.4  # the width of the interval the twin's truth is drawn from, (-0.2, 0.2)


def _plan_of(spectral):
    from crt1d_amd import batched

    return batched.SpectralRetrievalPlan if spectral else batched.RetrievalPlan


def _state(plan):
    import torch

    torch.cuda.synchronize()
    return {k: getattr(plan, k).cpu().numpy().copy() for k in STATE}


def _sequential(P, spectral, nd=None, niter=NSTEP, **kw):
    from crt1d_amd import batched

    a = P["args"]
    sensors = {} if spectral else dict(sensors=a[4])
    nd = P["nd"] if nd is None else nd
    w = np.full((nd - 1, 3), 5.0)
    return batched.SequentialPlan(*a[:4], a[-1], nd=nd, inv_sigma_dyn=w, niter=niter, **sensors, **P["kw"], **kw)


@pytest.mark.parametrize("spectral", [False, True])
def test_zero_precision_is_the_plan_without_it_bitwise(spectral):
    """prior_precision = 0 with any finite prior_mean: p, cost, A, g, status (and the rest of the state) after each of 6 steps are the
    bits of the plan without the two arguments, whose closing launch is another one (k_lm_step on rows; the spectral plan: one block)."""
    P = _series_problem(40, spectral)
    ncol = P["npix"] * P["nd"]
    rng = np.random.default_rng(61)
    old = _plan_of(spectral)(*P["args"], **P["kw"])
    new = _plan_of(spectral)(*P["args"], **P["kw"], prior_mean=rng.normal(size=(ncol, 3)), prior_precision=np.zeros((3, 3)))
    for it in range(6):
        assert _same(_state(old.step()), _state(new.step())), it
    assert _state(old)["naccept"].max() >= 3


@pytest.mark.parametrize("spectral", [False, True])
def test_diagonal_precision_is_the_diagonal_prior(spectral):
    """P = diag(s^2) around m against prior = m, inv_sigma_prior = s: one cost function, sums rounded differently.  Both runs end with
    the same status, and their final p differ by far less than either is from the truth: the prior (s = 3 around 0) pulls the
    minimiser off the truth by a distance d_truth of order 1e-2 to 1e-1 (printed), while the two minimisers are the same point up to
    rounding amplified by the condition of the normal matrix; 1e-6 d_truth is asserted, which is 1e10 u d_truth."""
    import torch

    P = _series_problem(40, spectral)
    m, s = np.zeros(3), np.full(3, 3.0)
    diag = _plan_of(spectral)(*P["args"], **P["kw"], prior=m, inv_sigma_prior=s).run(NSTEP)
    full = _plan_of(spectral)(*P["args"], **P["kw"], prior_mean=m, prior_precision=np.diag(s * s)).run(NSTEP)
    torch.cuda.synchronize()
    a, b = diag.result(), full.result()
    pa, pb = a["p"].cpu().numpy(), b["p"].cpu().numpy()
    d_truth = float(np.abs(pa.reshape(P["truth"].shape) - P["truth"]).max())
    d_plans = float(np.abs(pa - pb).max())
    print(f"diagonal against full prior, spectral={spectral}: |p_diag - truth| = {d_truth:.3e}, |p_full - p_diag| = {d_plans:.3e}")
    assert np.array_equal(a["status"].cpu().numpy(), b["status"].cpu().numpy())
    assert d_plans <= 1e-6 * d_truth
    ak = full.averaging_kernel().cpu().numpy()
    cov = full.covariance().cpu().numpy()
    assert np.allclose(ak, np.eye(3) - cov @ np.diag(s * s), rtol=0, atol=1e-12) and np.allclose(full.dfs().cpu().numpy(), np.trace(ak, axis1=1, axis2=2))
    assert np.all(full.dfs().cpu().numpy() < 3.0) and np.all(full.dfs().cpu().numpy() >= 0.0)


@pytest.mark.parametrize("spectral", [False, True])
def test_sequential_plan_with_one_date_is_the_unchained_plan(spectral):
    P = _series_problem(40, spectral)
    ncol = P["npix"] * P["nd"]
    old = _plan_of(spectral)(*P["args"], **P["kw"]).run(6)
    seq = _sequential(P, spectral, nd=1, niter=6).run()
    assert seq.npix == ncol and _same(_state(old), _state(seq.plan))
    r = seq.result()
    assert r["p"].cpu().numpy().tobytes() == old.p.cpu().numpy().tobytes() and r["p"].shape == (ncol, 1, 3) and not r["info"].any()
    assert r["cov"].cpu().numpy().tobytes() == old.covariance().cpu().numpy().tobytes()


@pytest.mark.parametrize("spectral", [False, True])
def test_sequential_plan_on_the_radiative_transfer(spectral):
    """Five dates, the twin of the chained plans (noise-free, date pix % 5 of every pixel fully masked).
    (a) result() is the long-double sweep of the plan's own p_filtered and stored A, within the bounds of section 4;
    (b) a fully masked date t >= 1 has p_filtered bitwise the p of the date before, and where it lies between two observed dates its
        smoothed variances exceed both neighbours';
    (c) both plans solve a zero-residual problem whose minimum is the truth: the smoothed p ends no farther from it than 10 times the
        chained plan's distance, with a floor of 1e-9 of the box the truth is drawn from (the factor covers the different iteration
        paths -- the filter linearises each date at its own filtered point -- not a model difference).  Both distances are printed.
    Measured on MI355X: see DESIGN.md 3.31."""
    import torch

    P = _series_problem(40, spectral)
    npix, nd, masked = P["npix"], P["nd"], P["masked"]
    # The observed rows get inv_sigma = 100 in place of the twin's 1.  At 1 the data precision of a date (of order 5) is below the
    # coupling's (w^2 = 25), so an observed date at the end of a series, with one neighbour, is less certain than a masked one between
    # two; with well-observed dates the gap is the least certain date, which (b) asserts -- on the long-double reference first.
    P["kw"]["inv_sigma"] = {k: 100.0 * v for k, v in P["kw"]["inv_sigma"].items()}
    seq = _sequential(P, spectral).run()
    r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in seq.result().items()}
    torch.cuda.synchronize()
    assert r["p"].shape == (npix, nd, 3) and r["cov"].shape == (npix, nd, 3, 3) and r["cost"].shape == (npix, nd) and r["info"].shape == (npix,)
    assert not r["info"].any() and not r["info_predict"].any() and r["params"] == seq.plan.params
    assert not np.any((r["status"] == R.STALLED) & ~masked) and not np.any(r["status"] == R.FAILED_START)
    A = seq.A.cpu().numpy()
    w = np.full((nd - 1, 3), 5.0)
    for pix in range(npix):
        ps_ref, Cs_ref = Q.rts_ld(r["p_filtered"][pix], A[pix], w)
        B, E = _rts_bounds(r["p_filtered"][pix], A[pix], w, ps_ref, Cs_ref)
        assert np.all(np.abs(r["cov"][pix].astype(LD) - Cs_ref).astype(np.float64).reshape(nd, -1).max(1) <= E), pix
        assert np.all(np.abs(r["p"][pix, :-1].astype(LD) - ps_ref[:-1]).astype(np.float64) <= B[:-1]), pix
        assert r["p"][pix, -1].tobytes() == r["p_filtered"][pix, -1].tobytes()
        t = pix % nd
        if t >= 1:
            assert r["p_filtered"][pix, t].tobytes() == r["p_filtered"][pix, t - 1].tobytes(), pix
        if 1 <= t <= nd - 2:
            var = np.diagonal(Cs_ref, axis1=1, axis2=2).astype(np.float64)
            assert np.all(var[t] > var[t - 1]) and np.all(var[t] > var[t + 1]), pix  # the reference, on the CPU
            var = np.diagonal(r["cov"][pix], axis1=1, axis2=2)
            assert np.all(var[t] > var[t - 1]) and np.all(var[t] > var[t + 1]), pix
    chain = _plan_of(spectral)(*P["args"], **P["kw"], chain=nd, inv_sigma_chain=P["w"]).run(NSTEP).result()["p"].cpu().numpy()
    d_chain, d_seq = float(np.abs(chain - P["truth"]).max()), float(np.abs(r["p"] - P["truth"]).max())
    print(f"noise-free twin, spectral={spectral}: distance from the truth: chain {d_chain:.3e}, filter + sweep {d_seq:.3e}")
    assert d_seq <= max(10.0 * d_chain, 1e-9 * BOX)
    # the filter alone, one date at a time: the same filtered state, the covariance of every date from its own A
    again = _sequential(P, spectral)
    for t in range(nd):
        again.assimilate(t)
    f = again.result()
    assert f["p"].cpu().numpy().tobytes() == r["p_filtered"].tobytes() and f["info"].shape == (npix, nd)
    assert f["cov"].cpu().numpy().tobytes() == covariance(A.reshape(npix * nd, -1)).tobytes()
    part = _sequential(P, spectral)
    for t in range(3):
        part.assimilate(t)
    pr = part.smooth().result()
    assert pr["p"].shape == (npix, 3, 3) and pr["p_filtered"].cpu().numpy().tobytes() == r["p_filtered"][:, :3].tobytes()
    ps3, cov3, _ = rts(r["p_filtered"][:, :3].copy(), A[:, :3].copy(), w[:2])
    assert pr["p"].cpu().numpy().tobytes() == ps3.tobytes() and pr["cov"].cpu().numpy().tobytes() == cov3.tobytes()


def test_a_series_longer_than_the_chain_serves():
    """84 dates at npar = 10 -- eight soil / leaf directions, ln LAI and the leaf-angle parameter --, 2 pixels, a diagonal prior on
    date 0 (which also gives the leaf-angle parameter of a parameterless kind a finite variance to hand on): the sequential plan runs,
    no date fails its start, every hand-over and the sweep report 0; chain = 84 is refused by the constructor, as before."""
    import torch

    from crt1d_amd import batched, synth

    npix, nd, nb, nz = 2, 84, 40, 10
    ncol = npix * nd
    d = synth.make_columns(npix, nb, nz, seed=23)
    rng = np.random.default_rng(231)
    per_date = lambda v: np.repeat(v, nd, axis=0)  # noqa: E731
    psi = np.tile(np.deg2rad(np.linspace(15.0, 65.0, nd)), npix)
    cols = batched.Columns(_t(psi), _t(per_date(d["lai"])), _t(per_date(d["g_kind"])).to(torch.int32), _t(per_date(d["g_param"])),
                           _t(per_date(d["mla"])))
    bands = batched.Bands(*[_t(per_date(d[k])) for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
    x = np.linspace(0.0, 1.0, nb)
    dl = _t(np.stack([0.2 * d["leaf_r"].mean(0) * np.cos(np.pi * k * x) for k in range(4)]))
    ds = _t(np.stack([0.2 * d["soil_r"].mean(0) * np.cos(np.pi * k * x) for k in range(4)]))
    zl, zs = torch.zeros_like(dl), torch.zeros_like(ds)
    dirs = dict(d_leaf_r=torch.cat((dl, zl)), d_soil_r=torch.cat((zs, ds)))
    lev, keys = (0, nz - 1), ("I_df_d", "I_df_u")
    y = {k: 1.01 * v for k, v in batched.solve_levels("2s", cols, bands, lev, keys=keys).items()}
    isp = np.zeros((ncol, 10))
    isp.reshape(npix, nd, 10)[:, 0] = 2.0
    prior = np.zeros((ncol, 10))
    prior[:, 9] = per_date(d["g_param"])  # (the leaf-angle parameter starts at, and is tied to, the column's own)
    kw = dict(keys=keys, lai=True, leaf=True, prior=prior, inv_sigma_prior=isp, lam0=1e-2, **dirs)
    w = np.full((nd - 1, 10), 5.0)
    with pytest.raises(ValueError, match="beyond the 83 the chain kernel serves at npar = 10"):
        batched.SpectralRetrievalPlan("2s", cols, bands, lev, y, **kw, chain=nd, inv_sigma_chain=w)
    seq = batched.SequentialPlan("2s", cols, bands, lev, y, nd=nd, inv_sigma_dyn=w, niter=6, **kw).run()
    r = seq.result()
    torch.cuda.synchronize()
    assert seq.npar == 10 and r["p"].shape == (npix, nd, 10)
    assert not bool((r["status"] == R.FAILED_START).any()) and not bool(r["info"].any()) and not bool(r["info_predict"].any())
    assert bool(torch.isfinite(r["p"]).all()) and bool(torch.isfinite(r["cov"]).all()) and bool((r["naccept"] >= 1).all())


def test_model_retrieve_sequential():
    """Model.retrieve_sequential is the batched sequential plan on the model's one pixel: bitwise; a full prior on date 0 is felt."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=10)
    nb, nd = m.nwl, 3
    psi = np.deg2rad([10.0, 40.0, 65.0])
    w = np.zeros((3, nb))
    w[0, : nb // 2], w[1, nb // 3:], w[2, nb // 2] = 1.0, 0.5, 2.0
    d = (0.3 * np.sin(np.linspace(0.0, 3.0, nb)) * m.copy_p()["leaf_r"])[None]
    y = {"I_df_u": 1.03 * m.run_series_sensors(psi, w, levels=(-1,))["I_df_u"]}  # (nd, 1, 3)
    isg = {"I_df_u": np.ones_like(y["I_df_u"])}
    isg["I_df_u"][1] = 0.0  # a cloudy date
    wdyn = np.full((nd - 1, 2), 3.0)
    got = m.retrieve_sequential(w, y, psi, wdyn, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, inv_sigma=isg)
    assert got["params"] == ("dir0", "lai") and got["p"].shape == (nd, 2) and got["cov"].shape == (nd, 2, 2) and got["cost"].shape == (nd,)
    assert got["info"] == 0 and got["p_filtered"][1].tobytes() == got["p_filtered"][0].tobytes()
    scheme, cols, b, sun = m._series_inputs(psi, None, None, "retrieval")
    rep = lambda v: None if v is None else v.expand(nd, *v.shape[1:]).contiguous()  # noqa: E731
    cols = batched.Columns(psi=sun.psi[0].contiguous(), lai=rep(cols.lai), g_kind=rep(cols.g_kind), g_param=rep(cols.g_param), mla=rep(cols.mla),
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[0].contiguous(), g_table=rep(cols.g_table))
    b = batched.Bands(sun.I_dr0[0].contiguous(), sun.I_df0[0].contiguous(), rep(b.leaf_r), rep(b.leaf_t), rep(b.soil_r))
    ref = batched.retrieve_sequential("2s", cols, b, (-1,), y, nd=nd, inv_sigma_dyn=wdyn, keys=("I_df_u",), sensors=batched.SensorSet(w), niter=8,
                                      d_leaf_r=d, lai=True, inv_sigma=isg)
    torch.cuda.synchronize()
    for k in ("p", "p_filtered", "cost", "status", "naccept", "nreject", "cov", "info"):
        assert got[k].tobytes() == ref[k][0].cpu().numpy().tobytes(), k
    var = np.diagonal(got["cov"], axis1=1, axis2=2)
    assert np.all(np.isfinite(got["cov"])) and np.all(var > 0)
    tight = m.retrieve_sequential(w, y, psi, wdyn, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, inv_sigma=isg,
                                  prior_mean=np.zeros(2), prior_precision=np.array([[1e8, 0.0], [0.0, 1e8]]))
    assert np.abs(tight["p_filtered"][0]).max() < 1e-3 < np.abs(got["p_filtered"][0]).max()  # date 0 held at the prior mean
    one = m.retrieve(w, {"I_df_u": y["I_df_u"][0]}, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8,
                     prior_mean=np.zeros(2), prior_precision=np.array([[1e8, 0.0], [0.0, 1e8]]))
    assert np.abs(one["p"]).max() < 1e-3
