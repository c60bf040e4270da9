"""The reference of the date-by-date retrieval, written from the contract of include_seq/crt1d_hip_lm_seq.h -- not from the kernels.

1. the fp64 restatement of k_lm_prior_block: the sums of a full Gaussian prior in the contract's order, on Python floats;
2. long double (``numpy.longdouble``): the parallel sum (A^-1 + W^-1)^-1 of k_lm_predict -- both as the product the header prescribes
   and literally, by two inversions --, the Rauch-Tung-Striebel recursions of k_lm_rts, an information filter of a linear-Gaussian pixel,
   and a block-tridiagonal solve that gives the smoothed means and marginal covariances straight from the chain's system.

Shapes for ONE column or pixel: packed matrices ``(ntri,)`` (lower triangle row by row), ``p (nd, npar)``, ``A (nd, ntri)``,
``w (nd - 1, npar)``.  The dense layer of tests/lm_chain_reference.py (``system``, ``solve_ld``, ``inverse_ld``) referees the rest."""
import numpy as np

import lm_chain_reference as R

LD = np.longdouble
U = 2.0 ** -53
tri = R.tri
pack = R.pack


def unpack(t, num=np.float64):
    """(ntri,) -> the symmetric (npar, npar)."""
    n = int(round((np.sqrt(8 * len(t) + 1) - 1) / 2))
    M = np.zeros((n, n), dtype=num)
    for i in range(n):
        for j in range(i + 1):
            M[i, j] = M[j, i] = num(t[tri(i, j)])
    return M


# ---- 1. fp64 in the contract's order --------------------------------------------------------------------------------------------------------
def prior_block(P, mean, p):
    """-> (A, g, c2) of one column: d_j = p_j - mean_j; v_i the running sum of S(i, j) d_j, j ascending; c2 the running sum of d_i v_i."""
    n = len(mean)
    d = [float(p[j]) - float(mean[j]) for j in range(n)]
    v = []
    for i in range(n):
        s = 0.0
        for j in range(n):
            s = s + float(P[tri(max(i, j), min(i, j))]) * d[j]
        v.append(s)
    c2 = 0.0
    for i in range(n):
        c2 = c2 + d[i] * v[i]
    return np.array(P, dtype=np.float64), np.array(v), c2


def prior_block_ld(P, mean, p):
    """-> (g, c2, |g| budget, |c2| budget) in long double: the exact-ish sums and the sums of the absolute values of their terms."""
    Pm, d = unpack(P, LD), np.asarray(p, dtype=LD) - np.asarray(mean, dtype=LD)
    terms = Pm * d[None, :]
    g = terms.sum(1)
    q = d[:, None] * terms
    return g, q.sum(), np.abs(terms).sum(1), np.abs(q).sum()


# ---- 2. long double ---------------------------------------------------------------------------------------------------------------------------
def _scaled_factor(E):
    """E (n, n) long double, positive diagonal -> (L, s): the Cholesky factor of (E_ij s_i s_j) and s = 1 / sqrt(diag E)."""
    s = LD(1) / np.sqrt(np.diagonal(E))
    return R.cholesky_ld(E * s[:, None] * s[None, :]), s


def _inverse(E):
    L, s = _scaled_factor(E)
    n = len(E)
    X = np.stack([R._solve_ld(L, np.eye(n, dtype=LD)[:, r]) for r in range(n)], axis=1)
    return X * s[:, None] * s[None, :]


def parallel_sum_ld(A, w):
    """(A^-1 + W^-1)^-1, W = diag(w^2), as the header's product W (A + W)^-1 A, symmetrised; A packed fp64, -> (npar, npar) long double.
    A row and column with w_k == 0 or A_kk + w_k^2 <= 0 is zero."""
    Am, q = unpack(A, LD), np.asarray(w, dtype=LD) ** 2
    n = len(q)
    live = [k for k in range(n) if q[k] != 0 and Am[k, k] + q[k] > 0]
    P = np.zeros((n, n), dtype=LD)
    if not live:
        return P
    dead = [k for k in range(n) if Am[k, k] + q[k] <= 0]
    keep = [k for k in range(n) if k not in dead]  # (a dead parameter is uncoupled from the rest: A_kk = 0 in a semidefinite A)
    Ak, qk = Am[np.ix_(keep, keep)], q[keep]
    L, s = _scaled_factor(Ak + np.diag(qk))
    Y = np.stack([R._solve_ld(L, Ak[:, j] * s) * s for j in range(len(keep))], axis=1)
    Pk = LD(0.5) * (qk[:, None] * Y + (qk[:, None] * Y).T)
    for a, i in enumerate(keep):
        for b, j in enumerate(keep):
            if i in live and j in live:
                P[i, j] = Pk[a, b]
    return P


def parallel_sum_literal_ld(A, w):
    """The same by its definition, two inversions; every w > 0 and A positive definite."""
    return _inverse(_inverse(unpack(A, LD)) + np.diag(LD(1) / np.asarray(w, dtype=LD) ** 2))


def rts_ld(p_f, A_f, w):
    """The backward sweep of the header in long double.  -> (p_s (nd, npar), C_s (nd, npar, npar))"""
    nd, npar = np.shape(p_f)
    pf = np.asarray(p_f, dtype=LD)
    ps, Cs = np.zeros((nd, npar), dtype=LD), np.zeros((nd, npar, npar), dtype=LD)
    ps[-1], Cs[-1] = pf[-1], _inverse(unpack(A_f[-1], LD))
    for t in reversed(range(nd - 1)):
        q = np.asarray(w[t], dtype=LD) ** 2
        Mi = _inverse(unpack(A_f[t], LD) + np.diag(q))
        G = Mi * q[None, :]
        ps[t] = pf[t] + G @ (ps[t + 1] - pf[t])
        Cs[t] = Mi + G @ Cs[t + 1] @ G.T
    return ps, Cs


def filter_ld(A_data, b_data, w, mean0=None, prec0=None):
    """The information filter of a linear-Gaussian pixel in long double.  Date t has the data term 0.5 p^T A_t p - b_t^T p (A_data
    (nd, ntri) packed, b_data (nd, npar)); date 0 may have the prior N(mean0, prec0^-1) (prec0 packed).  -> (p_f (nd, npar), A_f (nd,
    npar, npar)): the filtered means and posterior precisions."""
    nd, npar = np.shape(b_data)
    pf, Af = np.zeros((nd, npar), dtype=LD), np.zeros((nd, npar, npar), dtype=LD)
    Pp = np.zeros((npar, npar), dtype=LD) if prec0 is None else unpack(prec0, LD)
    m = np.zeros(npar, dtype=LD) if mean0 is None else np.asarray(mean0, dtype=LD)
    for t in range(nd):
        Af[t] = unpack(A_data[t], LD) + Pp
        L, s = _scaled_factor(Af[t])
        pf[t] = R._solve_ld(L, (np.asarray(b_data[t], dtype=LD) + Pp @ m) * s) * s
        if t < nd - 1:
            Pp, m = parallel_sum_ld(pack(Af[t]), w[t]), pf[t]
    return pf, Af


def block_tridiagonal_ld(A, b, w):
    """The chain's system H x = rhs solved as what it is, in long double: H_dd = A_d + W_{d-1} + W_d, H_{d,d-1} = -W_{d-1}, rhs = b.
    Forward elimination D_d = H_dd - W_{d-1} D_{d-1}^-1 W_{d-1}, backward substitution, and the diagonal blocks of H^-1 by
    S_d = D_d^-1 + D_d^-1 W_d S_{d+1} W_d D_d^-1.  -> (x (nd, npar), S (nd, npar, npar))"""
    nd, npar = np.shape(b)
    W = [np.diag(np.asarray(w[d], dtype=LD) ** 2) for d in range(nd - 1)]
    Di, z = [], []
    for d in range(nd):
        H = unpack(A[d], LD) + (W[d - 1] if d > 0 else 0) + (W[d] if d < nd - 1 else 0)
        r = np.asarray(b[d], dtype=LD)
        if d > 0:
            H = H - W[d - 1] @ Di[-1] @ W[d - 1]
            r = r + W[d - 1] @ z[-1]
        Di.append(_inverse(H))
        z.append(Di[-1] @ r)
    x, S = np.zeros((nd, npar), dtype=LD), np.zeros((nd, npar, npar), dtype=LD)
    x[-1], S[-1] = z[-1], Di[-1]
    for d in reversed(range(nd - 1)):
        x[d] = z[d] + Di[d] @ W[d] @ x[d + 1]
        S[d] = Di[d] + Di[d] @ W[d] @ S[d + 1] @ W[d] @ Di[d]
    return x, S


def dense_columns_ld(A, w, dates):
    """The block columns ``dates`` of the inverse of the dense chain system (tests/lm_chain_reference.py), without forming all of it:
    {d: (n, npar)} long double."""
    nd, npar = A.shape[0], int(round((np.sqrt(8 * A.shape[1] + 1) - 1) / 2))
    M, _, s = R.dense_ld(A, np.zeros((nd, npar)), np.zeros((nd, npar)), w, 0.0)
    L = R.cholesky_ld(M)
    out = {}
    for d in dates:
        cols = [R._solve_ld(L, np.eye(nd * npar, dtype=LD)[:, d * npar + k] * s) * s for k in range(npar)]
        out[d] = np.stack(cols, axis=1)
    return out


def scaled_extremes(E):
    """(lambda_min, lambda_max) of E scaled to a unit diagonal, fp64 (eigvalsh): kappa_2 of what the kernels factorise."""
    E = np.asarray(E, dtype=np.float64)
    s = 1.0 / np.sqrt(np.diagonal(E))
    ev = np.linalg.eigvalsh(E * s[:, None] * s[None, :])
    return float(ev[0]), float(ev[-1])
