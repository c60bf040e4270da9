"""NumPy restatement of the cost and selection contracts of include_lut/crt1d_hip_lut.h, written from the contracts (not from the kernel).

Cost: for column c and candidate k ONE running sum, started at +0 and extended row by row -- the rows of block 0 ascending, then block 1,
.., then the prior rows ascending --, every difference, product and sum a separately rounded float64 operation; a row with inv_sigma == 0
(a prior row with inv_sigma_prior == 0) adds nothing, whatever its y holds; cost = 0.5 * sum.  The table is finite: a candidate with a NaN or
an infinity anywhere in its rows (with a prior: or in its q) is eligible for no column (its cost is NaN here).  The arrays below are
vectorised over (c, k) only: the row loop is the contract's order.

Selection: eligible iff cost < +inf; the nbest smallest eligible candidates under (cost, then index); unfilled slots -1 / +inf;
p[c] = q[index[c][0]], or the default where no candidate is eligible."""
import numpy as np


def lut_cost(q, m, y, inv_sigma=None, prior=None, inv_sigma_prior=None):
    """``q (K, npar)``; ``m``, ``y``: lists of ``(K, nrow_b)`` / ``(ncol, nrow_b)``; ``inv_sigma``: None or a list of the shapes of ``y``
    with None entries for ones; ``prior``, ``inv_sigma_prior`` ``(ncol, npar)`` or both None.  -> ``(ncol, K)``"""
    ncol, K = y[0].shape[0], q.shape[0]
    s = np.zeros((ncol, K))
    with np.errstate(all="ignore"):
        for b in range(len(m)):
            w = None if inv_sigma is None else inv_sigma[b]
            for o in range(m[b].shape[1]):
                r = m[b][None, :, o] - y[b][:, None, o]
                if w is not None:
                    r = r * w[:, None, o]
                add = r * r
                if w is not None:
                    add = np.where(w[:, None, o] == 0.0, 0.0, add)  # (+0 on a sum that is never -0: nothing)
                s = s + add
        if prior is not None:
            for j in range(q.shape[1]):
                d = (q[None, :, j] - prior[:, None, j]) * inv_sigma_prior[:, None, j]
                s = s + np.where(inv_sigma_prior[:, None, j] == 0.0, 0.0, d * d)
        bad = ~np.all([np.isfinite(t).all(axis=1) for t in m], axis=0)
        if prior is not None:
            bad |= ~np.isfinite(q).all(axis=1)
        cost = 0.5 * s
        cost[:, bad] = np.nan
        return cost


def lut_select(cost, nbest):
    """``cost (ncol, K)`` -> ``index (ncol, nbest)`` int32, ``best (ncol, nbest)``"""
    ncol = cost.shape[0]
    index = np.full((ncol, nbest), -1, dtype=np.int32)
    best = np.full((ncol, nbest), np.inf)
    for c in range(ncol):
        elig = np.flatnonzero(cost[c] < np.inf)
        order = elig[np.lexsort((elig, cost[c][elig]))][:nbest]
        index[c, :order.size] = order
        best[c, :order.size] = cost[c][order]
    return index, best


def lut_match(q, m, y, inv_sigma=None, prior=None, inv_sigma_prior=None, nbest=1, p_default=None):
    """-> ``index``, ``cost``, ``p`` of the contracts; ``p_default (ncol, npar)`` (default NaN)."""
    index, best = lut_select(lut_cost(q, m, y, inv_sigma, prior, inv_sigma_prior), nbest)
    p = np.full((y[0].shape[0], q.shape[1]), np.nan) if p_default is None else np.array(p_default, dtype=np.float64)
    has = index[:, 0] >= 0
    p[has] = q[index[has, 0]]
    return index, best, p


def merge_lists(index_a, cost_a, index_b, cost_b, nbest):
    """Two results on disjoint candidate sets (indices already global) -> the result on their union, under the total order."""
    index = np.concatenate([index_a, index_b], axis=1)
    cost = np.concatenate([cost_a, cost_b], axis=1)
    out_i = np.full((index.shape[0], nbest), -1, dtype=np.int32)
    out_c = np.full((index.shape[0], nbest), np.inf)
    for c in range(index.shape[0]):
        ok = np.flatnonzero(index[c] >= 0)
        order = ok[np.lexsort((index[c][ok], cost[c][ok]))][:nbest]
        out_i[c, :order.size] = index[c][order]
        out_c[c, :order.size] = cost[c][order]
    return out_i, out_c
