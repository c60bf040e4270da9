"""The reference of the chained Levenberg-Marquardt step with shared parameters, written from the contract of include_shared/
crt1d_hip_lm_shared.h -- not from the kernel.  Two layers, both for ONE pixel:

1. the fp64 restatement: the per-date sums, the pixel cost, the decisions and the left-looking solve of the bordered system in the order
   of the header, on Python floats (IEEE doubles, every operation rounded on its own);
2. the long-double layer: the dense n x n system (n = nd nv + ns), its solution and its inverse by a dense Cholesky on
   ``numpy.longdouble``.

Shapes: ``A (nd, ntri)`` packed lower triangles at the full npar, ``g (nd, npar)``, ``c2 (nd,)``, ``p (nd, npar)``, ``w (nd - 1, npar)``
(the columns of shared parameters are never read), ``mask``: bit k set = parameter k shared.  Unknown ordering: (d, j) -> d * nv + j for
the varying parameter kv[j] of date d, then nd * nv + i for the shared parameter ks[i]."""
import math

import numpy as np

from lm_chain_reference import (CONVERGED_F, CONVERGED_X, FAILED_START, LD, RUNNING, STALLED, U, _solve_ld, cholesky_ld, date_sums,  # noqa: F401
                                new_state, pack, tri)

LIMIT = 160 * 1024


def split(mask, npar):
    """-> (kv, ks): the varying and the shared parameter indices, ascending"""
    return [k for k in range(npar) if not mask >> k & 1], [k for k in range(npar) if mask >> k & 1]


def mask_of(bits):
    return sum(1 << k for k, b in enumerate(bits) if b)


def lds_bytes(nd, nv, ns):
    """CRT_LM_SHARED_LDS_BYTES of the header"""
    return 8 * (nd * (2 * nv * nv + 4 * nv + nv * ns if nv else 1) + 4 * nv * nv + 64 + 3 * ns * ns + 2 * nv * ns + 4 * ns)


def max_nd(npar, ns):
    """The header's formula inverted: the largest nd whose LDS fits 160 KiB (the formula is affine in nd)."""
    nv = npar - ns
    fixed, per_date = lds_bytes(0, nv, ns), lds_bytes(1, nv, ns) - lds_bytes(0, nv, ns)
    return (LIMIT - fixed) // per_date


def sym(A_d, a, b):
    return A_d[tri(max(a, b), min(a, b))]


# ---- layer 1: fp64 in the contract's order ----------------------------------------------------------------------------------------------
def pixel_cost(c2, p, w, mask):
    kv, _ = split(mask, p.shape[1])
    tot = float(c2[0])
    for d in range(1, len(c2)):
        tot = tot + float(c2[d])
    for d in range(len(c2) - 1):
        for k in kv:
            e = (float(p[d + 1][k]) - float(p[d][k])) * float(w[d][k])
            tot = tot + e * e
    return 0.5 * tot


def system(A, g, p, w, lam, mask, num=float):
    """-> (M, x, s, dead): the scaled damped matrix (dense, n x n nested lists, the ordering of the header), the scaled right-hand side
    and the scales, formed in the header's order in the arithmetic of ``num``."""
    nd, npar = g.shape
    kv, ks = split(mask, npar)
    nv, ns = len(kv), len(ks)
    N = nd * nv
    n = N + ns
    one, zero = num(1), num(0)
    wv = lambda d, k: num(w[d][k]) if 0 <= d < nd - 1 else None  # noqa: E731
    h, G = [zero] * n, [zero] * n
    for d in range(nd):
        for j, k in enumerate(kv):
            r = d * nv + j
            hh, gg, pk = num(A[d][tri(k, k)]), num(g[d][k]), num(p[d][k])
            wl, wr = wv(d - 1, k), wv(d, k)
            if wl is not None:
                hh = hh + wl * wl
                gg = gg + wl * ((pk - num(p[d - 1][k])) * wl)
            if wr is not None:
                hh = hh + wr * wr
                gg = gg - wr * ((num(p[d + 1][k]) - pk) * wr)
            h[r], G[r] = hh, gg
    for i, k in enumerate(ks):
        hh, gg = num(A[0][tri(k, k)]), num(g[0][k])
        for d in range(1, nd):
            hh = hh + num(A[d][tri(k, k)])
            gg = gg + num(g[d][k])
        h[N + i], G[N + i] = hh, gg
    dead = [bool(v <= 0) for v in h]
    sqrt = math.sqrt if num is float else np.sqrt
    s = [one if dd else one / sqrt(v) for v, dd in zip(h, dead)]
    M = [[zero] * n for _ in range(n)]
    for d in range(nd):
        for i in range(nv):
            r = d * nv + i
            for j in range(i + 1):
                q = d * nv + j
                v = ((h[r] if i == j else num(sym(A[d], kv[i], kv[j]))) * s[r]) * s[q]
                if i == j:
                    v = v + (one if dead[r] else num(lam))
                M[r][q] = M[q][r] = v
            if d > 0:
                wl = num(w[d - 1][kv[i]])
                M[r][r - nv] = M[r - nv][r] = ((-(wl * wl)) * s[r]) * s[r - nv]
        for i in range(ns):
            for j in range(nv):
                r, q = N + i, d * nv + j
                M[r][q] = M[q][r] = (num(sym(A[d], ks[i], kv[j])) * s[r]) * s[q]
    for i in range(ns):
        for l in range(i + 1):
            r, q = N + i, N + l
            if i == l:
                hil = h[r]
            else:
                hil = num(sym(A[0], ks[i], ks[l]))
                for d in range(1, nd):
                    hil = hil + num(sym(A[d], ks[i], ks[l]))
            v = (hil * s[r]) * s[q]
            if i == l:
                v = v + (one if dead[r] else num(lam))
            M[r][q] = M[q][r] = v
    x = [(-G[r]) * s[r] for r in range(n)]
    return M, x, s, dead


def bordered_solve(A, g, p, w, lam, mask):
    """-> (delta_v (nd, nv), delta_s (ns,)) in fp64, every sum in the header's order: the left-looking Cholesky with the structural zeros
    left out, forward, backward (the farthest group of rows first)."""
    nd, npar = g.shape
    kv, ks = split(mask, npar)
    nv, ns = len(kv), len(ks)
    N = nd * nv
    n = N + ns
    M, x, s, _ = system(A, g, p, w, lam, mask)

    def cols(r):  # the columns m <= r where L_rm is structurally non-zero, ascending
        if r >= N:
            return range(0, r + 1)
        return range(max(r // nv - 1, 0) * nv, r + 1)

    L = [[0.0] * n for _ in range(n)]
    for q in range(n):
        for r in range(q, n):
            cr = cols(r)
            if q not in cr:
                continue
            t = 0.0
            for m in cols(q):  # ascending; the columns where both rows are non-zero
                if m < q and m in cr:
                    t = t + L[r][m] * L[q][m]
            L[r][q] = math.sqrt(M[q][q] - t) if r == q else (M[r][q] - t) / L[q][q]
    z = [0.0] * n
    for r in range(n):
        u = 0.0
        for m in cols(r):
            if m < r:
                u = u + L[r][m] * z[m]
        z[r] = (x[r] - u) / L[r][r]
    y = [0.0] * n
    for r in reversed(range(n)):
        if r >= N:
            rows = list(range(r + 1, n))
        else:
            d = r // nv
            rows = list(range(N, n)) + list(range((d + 1) * nv, min(N, (d + 2) * nv))) + list(range(r + 1, (d + 1) * nv))
        v = 0.0
        for m in rows:
            v = v + L[m][r] * y[m]
        y[r] = (z[r] - v) / L[r][r]
    delta = [y[r] * s[r] for r in range(n)]
    return np.array(delta[:N]).reshape(nd, nv), np.array(delta[N:])


def trial_point(p, dv, ds, mask, lo=None, hi=None):
    """p_trial (nd, npar): p + delta on the varying entries, p of date 0 + delta on the shared ones (the same bits on every date), clamped"""
    nd, npar = p.shape
    kv, ks = split(mask, npar)
    pt = np.array(p, dtype=np.float64)
    for j, k in enumerate(kv):
        pt[:, k] = p[:, k] + dv[:, j]
    for i, k in enumerate(ks):
        pt[:, k] = p[0, k] + ds[i]
    if lo is not None:
        pt = np.where(pt < lo, lo, pt)
    if hi is not None:
        pt = np.where(pt > hi, hi, pt)
    return pt


def step(state, blocks, w, opt, mask, lo=None, hi=None, prior=None, isp=None):
    """THE STEP of the header for one pixel; ``opt``: lam_up, lam_down, lam_min, lam_max, xtol, ftol.  -> the new state (a copy)."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    if st["status"] != RUNNING:
        return st
    npar = st["p"].shape[1]
    kv, ks = split(mask, npar)
    A, g, c2 = date_sums(blocks, st["p_trial"], prior, isp)
    cost_t, cost = pixel_cost(c2, st["p_trial"], w, mask), st["cost"]
    accept = cost_t < cost
    if accept:
        p = st["p_trial"].copy()
        p[:, ks] = st["p_trial"][0, ks]
        st["p"], st["A"], st["g"] = p, A, g
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
        dv, ds = bordered_solve(st["A"], st["g"], st["p"], w, st["lam"], mask)
        pt = trial_point(st["p"], dv, ds, mask, lo, hi)
        xtol, p = opt["xtol"], st["p"]
        near = np.abs(pt - p) < xtol * (np.abs(p) + xtol)
        if bool(np.all(near[:, kv])) and bool(np.all(near[0, ks])):  # the n entries: a shared one at p of date 0
            st["status"] = CONVERGED_X
        else:
            st["p_trial"] = pt
    if st["status"] != RUNNING:
        st["p_trial"] = st["p"].copy()
    return st


# ---- layer 2: long double, dense ---------------------------------------------------------------------------------------------------------
def dense_ld(A, g, p, w, lam, mask):
    """-> (M, x, s) as long-double arrays: the dense scaled damped system, formed in long double from the fp64 inputs."""
    M, x, s, dead = system(A, g, p, w, lam, mask, num=LD)
    assert not any(dead)
    return np.array(M, dtype=LD), np.array(x, dtype=LD), np.array(s, dtype=LD)


def solve_ld(A, g, p, w, lam, mask):
    """delta (n,) in long double, the ordering of the header, by a dense Cholesky of the whole system."""
    M, x, s = dense_ld(A, g, p, w, lam, mask)
    return _solve_ld(cholesky_ld(M), x) * s


def inverse_ld(A, w, mask):
    """The inverse of the undamped H, (n, n) long double, the ordering of the header."""
    nd, npar = A.shape[0], int(round((math.sqrt(8 * A.shape[1] + 1) - 1) / 2))
    M, _, s = dense_ld(A, np.zeros((nd, npar)), np.zeros((nd, npar)), w, 0.0, mask)
    L = cholesky_ld(M)
    n = len(M)
    X = np.stack([_solve_ld(L, np.eye(n, dtype=LD)[:, r]) for r in range(n)], axis=1)
    return X * s[:, None] * s[None, :]


def marginal(X, d, nd, npar, mask):
    """The (npar, npar) block of (v_d, s) out of the (n, n) matrix X, in the ORIGINAL parameter order."""
    kv, ks = split(mask, npar)
    nv = len(kv)
    idx = np.empty(npar, dtype=int)
    for j, k in enumerate(kv):
        idx[k] = d * nv + j
    for i, k in enumerate(ks):
        idx[k] = nd * nv + i
    return X[np.ix_(idx, idx)]


def full_delta(delta, nd, npar, mask):
    """(n,) in the header's ordering -> (nd, npar), a shared entry on every date"""
    X = np.asarray(delta)
    kv, ks = split(mask, npar)
    nv = len(kv)
    out = np.zeros((nd, npar), dtype=X.dtype)
    for d in range(nd):
        for j, k in enumerate(kv):
            out[d, k] = X[d * nv + j]
        for i, k in enumerate(ks):
            out[d, k] = X[nd * nv + i]
    return out


def cost_ld(c2, p, w, mask):
    kv, _ = split(mask, np.shape(p)[1])
    c2, p, w = (np.asarray(v, dtype=LD) for v in (c2, p, w))
    return LD(0.5) * (c2.sum() + (((p[1:, kv] - p[:-1, kv]) * w[:, kv]) ** 2).sum())


def scaled_extremes(A, w, lam, mask):
    """(lambda_min, lambda_max) of the scaled damped matrix M, in fp64 (eigvalsh): kappa_2(M) = max / min."""
    nd, npar = A.shape[0], int(round((math.sqrt(8 * A.shape[1] + 1) - 1) / 2))
    M, _, _, _ = system(A, np.zeros((nd, npar)), np.zeros((nd, npar)), w, lam, mask)
    ev = np.linalg.eigvalsh(np.array(M))
    return float(ev[0]), float(ev[-1])


def solve_bound(A, g, p, w, lam, mask, sol_scaled_norm):
    """The bound of the solve in the scaled unknowns x (u = 2^-53, n = nd nv + ns, M the scaled damped matrix):
    (4 n (3 n + 1) + 8 n) u kappa_2(M) ||x||_2 for the backward-stable Cholesky solve (Higham, Thm 10.4 with 10.6) and the at most 8
    roundings an entry of forming a varying entry of M -- a border entry costs 2 (two scalings), a corner entry nd + 2 (nd - 1 sums, two
    scalings, the damping): componentwise (nd + 2) u |M| on those ns rows, in norm at most (nd + 2) sqrt(ns n) u ||M||_2, added as its own
    term -- plus ||beta||_2 / lambda_min for forming b = -G s: beta_r = 6 u (|g| + |w_l e_l| + |w_r e_r|) s_r on a varying row and
    (nd + 1) u (sum_d |g_d|) s_r on a shared row (nd - 1 sums, the sign, the scaling).  -> (the bound on |x^ - x| in the 2-norm, s)"""
    nd, npar = g.shape
    kv, ks = split(mask, npar)
    nv, ns = len(kv), len(ks)
    n = nd * nv + ns
    _, _, s = dense_ld(A, g, p, w, lam, mask)
    s = s.astype(np.float64)
    lo, hi = scaled_extremes(A, w, lam, mask)
    beta = np.zeros(n)
    for d in range(nd):
        for j, k in enumerate(kv):
            t = abs(g[d, k])
            if d > 0:
                t += abs(w[d - 1, k] ** 2 * (p[d, k] - p[d - 1, k]))
            if d < nd - 1:
                t += abs(w[d, k] ** 2 * (p[d + 1, k] - p[d, k]))
            beta[d * nv + j] = 6 * U * t * s[d * nv + j]
    for i, k in enumerate(ks):
        beta[nd * nv + i] = (nd + 1) * U * np.abs(g[:, k]).sum() * s[nd * nv + i]
    c = 4 * n * (3 * n + 1) + 8 * n + (nd + 2) * math.sqrt(ns * n)
    return c * U * (hi / lo) * sol_scaled_norm + np.linalg.norm(beta) / lo, s, c, lo, hi
