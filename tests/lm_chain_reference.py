"""The reference of the chained Levenberg-Marquardt step, written from the contract of include_chain/crt1d_hip_lm_chain.h -- not from the
kernel.  Two layers, both for ONE pixel (a pixel never sees another):

1. the fp64 restatement: the per-date sums, the pixel cost, the decisions and the banded left-looking solve in the order of the header,
   on Python floats (IEEE doubles, every operation rounded on its own);
2. the long-double layer: the dense (nd npar)^2 system, its solution and its inverse by a dense Cholesky on ``numpy.longdouble``.

Shapes: ``A (nd, ntri)`` packed lower triangles row by row, ``g (nd, npar)``, ``c2 (nd,)``, ``p (nd, npar)``, ``w (nd - 1, npar)``."""
import math

import numpy as np

RUNNING, CONVERGED_X, CONVERGED_F, STALLED, FAILED_START = range(5)
U = 2.0 ** -53
LD = np.longdouble


def tri(i, j):
    return i * (i + 1) // 2 + j


def max_nd(npar):
    """The header's formula: the largest nd whose CRT_LM_CHAIN_LDS_BYTES fit 160 KiB."""
    return (160 * 1024 // 8 - 4 * npar * npar - 64) // (2 * npar * npar + 4 * npar)


# ---- layer 1: fp64 in the contract's order ----------------------------------------------------------------------------------------------
def date_sums(blocks, p_trial, prior=None, isp=None):
    """blocks: [(A, g, c2)] of one pixel -> (A, g, c2): block 0's bits, the blocks 1.. in ascending order, the date's prior rows last."""
    A, g, c2 = (np.array(v, dtype=np.float64) for v in blocks[0])
    nd, npar = g.shape
    A, g, c2 = A.tolist(), g.tolist(), c2.tolist()
    for Ab, gb, cb in blocks[1:]:
        for d in range(nd):
            A[d] = [a + float(b) for a, b in zip(A[d], Ab[d])]
            g[d] = [a + float(b) for a, b in zip(g[d], gb[d])]
            c2[d] = c2[d] + float(cb[d])
    if isp is not None:
        for d in range(nd):
            for k in range(npar):
                s = float(isp[d][k])
                if s == 0.0:
                    continue
                dk = (float(p_trial[d][k]) - float(prior[d][k])) * s
                A[d][tri(k, k)] = A[d][tri(k, k)] + s * s
                g[d][k] = g[d][k] + s * dk
                c2[d] = c2[d] + dk * dk
    return np.array(A), np.array(g), np.array(c2)


def pixel_cost(c2, p, w):
    tot = float(c2[0])
    for d in range(1, len(c2)):
        tot = tot + float(c2[d])
    for d in range(len(c2) - 1):
        for k in range(p.shape[1]):
            e = (float(p[d + 1][k]) - float(p[d][k])) * float(w[d][k])
            tot = tot + e * e
    return 0.5 * tot


def system(A, g, p, w, lam, num=float):
    """-> (M, x, s, dead): the scaled damped matrix (dense, n x n nested lists), the scaled right-hand side and the scales, formed in the
    header's order in the arithmetic of ``num`` (float: fp64; numpy.longdouble: the same formulas, 11 bits more)."""
    nd, npar = g.shape
    n = nd * npar
    one, zero = num(1), num(0)
    wv = lambda d, k: num(w[d][k]) if 0 <= d < nd - 1 else None  # noqa: E731
    h, G = [zero] * n, [zero] * n
    for d in range(nd):
        for k in range(npar):
            r = d * npar + k
            hh, gg, pk = num(A[d][tri(k, k)]), num(g[d][k]), num(p[d][k])
            wl, wr = wv(d - 1, k), wv(d, k)
            if wl is not None:
                hh = hh + wl * wl
                gg = gg + wl * ((pk - num(p[d - 1][k])) * wl)
            if wr is not None:
                hh = hh + wr * wr
                gg = gg - wr * ((num(p[d + 1][k]) - pk) * wr)
            h[r], G[r] = hh, gg
    dead = [bool(v <= 0) for v in h]
    sqrt = math.sqrt if num is float else np.sqrt
    s = [one if dd else one / sqrt(v) for v, dd in zip(h, dead)]
    M = [[zero] * n for _ in range(n)]
    for d in range(nd):
        for i in range(npar):
            r = d * npar + i
            for j in range(i + 1):
                q = d * npar + j
                v = ((h[r] if i == j else num(A[d][tri(i, j)])) * s[r]) * s[q]
                if i == j:
                    v = v + (one if dead[r] else num(lam))
                M[r][q] = M[q][r] = v
            if d > 0:
                wl = num(w[d - 1][i])
                M[r][r - npar] = M[r - npar][r] = ((-(wl * wl)) * s[r]) * s[r - npar]
    x = [(-G[r]) * s[r] for r in range(n)]
    return M, x, s, dead


def band_solve(A, g, p, w, lam):
    """delta (nd, npar) in fp64, every sum in the header's order: the left-looking Cholesky on the band, forward, backward."""
    nd, npar = g.shape
    n = nd * npar
    M, x, s, _ = system(A, g, p, w, lam)
    first = lambda r: max(r // npar - 1, 0) * npar  # noqa: E731  (the first column of the block of the date before r's)
    L = [[0.0] * n for _ in range(n)]
    for q in range(n):
        for r in range(q, min(n, (q // npar + 2) * npar)):
            t = 0.0
            for m in range(first(r), q):
                t = t + L[r][m] * L[q][m]
            L[r][q] = math.sqrt(M[q][q] - t) if r == q else (M[r][q] - t) / L[q][q]
    z = [0.0] * n
    for r in range(n):
        u = 0.0
        for m in range(first(r), r):
            u = u + L[r][m] * z[m]
        z[r] = (x[r] - u) / L[r][r]
    y = [0.0] * n
    for r in reversed(range(n)):
        d = r // npar
        v = 0.0
        for m in list(range((d + 1) * npar, min(n, (d + 2) * npar))) + list(range(r + 1, (d + 1) * npar)):
            v = v + L[m][r] * y[m]
        y[r] = (z[r] - v) / L[r][r]
    return np.array([y[r] * s[r] for r in range(n)]).reshape(nd, npar)


def new_state(p0, lam0):
    p0 = np.array(p0, dtype=np.float64)
    nd, npar = p0.shape
    return dict(p=p0.copy(), p_trial=p0.copy(), cost=math.inf, lam=float(lam0), A=np.zeros((nd, npar * (npar + 1) // 2)),
                g=np.zeros((nd, npar)), status=RUNNING, naccept=0, nreject=0)


def step(state, blocks, w, opt, lo=None, hi=None, prior=None, isp=None):
    """THE STEP of the header for one pixel; ``opt``: lam_up, lam_down, lam_min, lam_max, xtol, ftol.  -> the new state (a copy)."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    if st["status"] != RUNNING:
        return st
    A, g, c2 = date_sums(blocks, st["p_trial"], prior, isp)
    cost_t, cost = pixel_cost(c2, st["p_trial"], w), st["cost"]
    accept = cost_t < cost
    if accept:
        st["p"], st["A"], st["g"] = st["p_trial"].copy(), A, g
        st["lam"] = max(st["lam"] * opt["lam_down"], opt["lam_min"])
        if cost - cost_t < opt["ftol"] * cost_t:
            st["status"] = CONVERGED_F
        st["cost"] = cost_t
        st["naccept"] += 1
    elif cost == math.inf:
        st["status"] = FAILED_START
    else:
        st["lam"] = st["lam"] * opt["lam_up"]
        if st["lam"] > opt["lam_max"]:
            st["status"] = STALLED
        st["nreject"] += 1
    if st["status"] == RUNNING:
        delta = band_solve(st["A"], st["g"], st["p"], w, st["lam"])
        pt = st["p"] + delta
        if lo is not None:
            pt = np.where(pt < lo, lo, pt)
        if hi is not None:
            pt = np.where(pt > hi, hi, pt)
        xtol = opt["xtol"]
        if bool(np.all(np.abs(pt - st["p"]) < xtol * (np.abs(st["p"]) + xtol))):
            st["status"] = CONVERGED_X
        else:
            st["p_trial"] = pt
    if st["status"] != RUNNING:
        st["p_trial"] = st["p"].copy()
    return st


# ---- layer 2: long double, dense ---------------------------------------------------------------------------------------------------------
def cholesky_ld(M):
    n = len(M)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - np.dot(L[j, :j], L[j, :j]))
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def _solve_ld(L, b):
    n = len(b)
    z = np.zeros(n, dtype=LD)
    for r in range(n):
        z[r] = (b[r] - np.dot(L[r, :r], z[:r])) / L[r, r]
    y = np.zeros(n, dtype=LD)
    for r in reversed(range(n)):
        y[r] = (z[r] - np.dot(L[r + 1:, r], y[r + 1:])) / L[r, r]
    return y


def dense_ld(A, g, p, w, lam):
    """-> (M, x, s) as long-double arrays: the dense scaled damped system of the pixel, formed in long double from the fp64 inputs."""
    M, x, s, dead = system(A, g, p, w, lam, num=LD)
    assert not any(dead)
    return np.array(M, dtype=LD), np.array(x, dtype=LD), np.array(s, dtype=LD)


def solve_ld(A, g, p, w, lam):
    """delta (nd, npar) in long double by a dense Cholesky of the whole (nd npar)^2 system."""
    M, x, s = dense_ld(A, g, p, w, lam)
    return (_solve_ld(cholesky_ld(M), x) * s).reshape(np.shape(g))


def inverse_ld(A, w):
    """The inverse of the undamped H, (n, n) long double."""
    nd, npar = A.shape[0], int(round((math.sqrt(8 * A.shape[1] + 1) - 1) / 2))
    M, _, s = dense_ld(A, np.zeros((nd, npar)), np.zeros((nd, npar)), w, 0.0)
    L = cholesky_ld(M)
    n = len(M)
    X = np.stack([_solve_ld(L, np.eye(n, dtype=LD)[:, r]) for r in range(n)], axis=1)
    return X * s[:, None] * s[None, :]


def cost_ld(c2, p, w):
    c2, p, w = (np.asarray(v, dtype=LD) for v in (c2, p, w))
    return LD(0.5) * (c2.sum() + (((p[1:] - p[:-1]) * w) ** 2).sum())


def scaled_extremes(A, w, lam):
    """(lambda_min, lambda_max) of the scaled damped matrix M, in fp64 (eigvalsh): kappa_2(M) = max / min."""
    nd, npar = A.shape[0], int(round((math.sqrt(8 * A.shape[1] + 1) - 1) / 2))
    M, _, _, _ = system(A, np.zeros((nd, npar)), np.zeros((nd, npar)), w, lam)
    ev = np.linalg.eigvalsh(np.array(M))
    return float(ev[0]), float(ev[-1])


def pack(Afull):
    """(..., npar, npar) -> the packed lower triangles (..., ntri)."""
    n = Afull.shape[-1]
    i, j = np.tril_indices(n)
    return Afull[..., i, j]
