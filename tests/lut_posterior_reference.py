"""NumPy restatement of the contract of include_post/crt1d_hip_lut_posterior.h, written from the contract (not from the kernel).

The costs are those of tests/lut_reference.lut_cost, bitwise the cost contract; the best candidate is that of lut_select.  For a column
with a best candidate kb and a temperature T that is finite and > 0: it = 1 / T, a_k = (cost_k - cmin) * it and d_ki = q[k][i] - q[kb][i]
are formed in float64 exactly as the contract rounds them; w_k = exp(-a_k) and every sum (S0, Sq, S1, S2 and the absolute sums) are
formed in np.longdouble, so the reference carries none of the kernel's summation error; the finish (m = S1 / S0, mean = q[kb] + m, cov =
S2 / S0 - m m^T, ess = S0^2 / Sq) is float64 on the rounded sums.  An ineligible candidate (cost not < +inf) enters no sum.  A column without
a result: index -1, cost +inf, wsum = ess = 0, mean and cov NaN (the plan's fill).

Besides the six outputs it returns A1_i = sum w |d_i| / S0 and A2_ij = sum w |d_i d_j| / S0, the scales of the rounding bounds."""
import numpy as np

import lut_reference as R


def lut_posterior(q, m, y, inv_sigma=None, prior=None, inv_sigma_prior=None, temperature=1.0):
    """Arguments as ``lut_reference.lut_cost``; ``temperature`` a number or ``(ncol,)``.
    -> dict of ``index (ncol,)`` int32, ``cost``, ``mean (ncol, npar)``, ``cov (ncol, npar, npar)``, ``wsum``, ``ess``, ``A1 (ncol, npar)``,
    ``A2 (ncol, npar, npar)``"""
    cost = R.lut_cost(q, m, y, inv_sigma, prior, inv_sigma_prior)
    index, best = R.lut_select(cost, 1)
    ncol, npar = cost.shape[0], q.shape[1]
    T = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (ncol,))
    out = {"index": index[:, 0].copy(), "cost": best[:, 0].copy(), "mean": np.full((ncol, npar), np.nan),
           "cov": np.full((ncol, npar, npar), np.nan), "wsum": np.zeros(ncol), "ess": np.zeros(ncol), "A1": np.zeros((ncol, npar)),
           "A2": np.zeros((ncol, npar, npar))}
    L = np.longdouble
    for c in range(ncol):
        kb = out["index"][c]
        if kb < 0 or not (np.isfinite(T[c]) and T[c] > 0):
            out["index"][c], out["cost"][c] = -1, np.inf
            continue
        with np.errstate(all="ignore"):
            elig = cost[c] < np.inf
        it = np.float64(1.0) / T[c]
        a = (cost[c][elig] - cost[c][kb]) * it
        d = q[elig] - q[kb]
        w = np.exp(-a.astype(L))
        dl = d.astype(L)
        S0, Sq = w.sum(), (w * w).sum()
        S1 = (w[:, None] * dl).sum(axis=0)
        S2 = np.einsum("k,ki,kj->ij", w, dl, dl)
        out["A1"][c] = (np.einsum("k,ki->i", w, np.abs(dl)) / S0).astype(np.float64)
        out["A2"][c] = (np.einsum("k,ki,kj->ij", w, np.abs(dl), np.abs(dl)) / S0).astype(np.float64)
        s0, sq, s1, s2 = np.float64(S0), np.float64(Sq), S1.astype(np.float64), S2.astype(np.float64)
        mm = s1 / s0
        out["mean"][c] = q[kb] + mm
        out["cov"][c] = s2 / s0 - mm[:, None] * mm[None, :]
        out["ess"][c] = (s0 * s0) / sq
        out["wsum"][c] = s0
    return out


def finish(q_kb, s0, sq, s1, s2):
    """The contract's finish arithmetic in float64, operation by operation: ``s1 (npar,)``, ``s2 (npar, npar)`` symmetric.
    -> mean, cov, ess, wsum"""
    s0, sq = np.float64(s0), np.float64(sq)
    mm = np.asarray(s1, dtype=np.float64) / s0
    return q_kb + mm, np.asarray(s2, dtype=np.float64) / s0 - mm[:, None] * mm[None, :], (s0 * s0) / sq, s0


def bounds(ref, K):
    """The rounding bounds of the header's summation against this reference, first order: every one of the K terms of a sum is rounded
    once when it is formed (twice for S2: t_i, then t_i d_j) and carries fexp's 1 ulp, a running sum of at most K + 8 additions (the
    candidates, the strands, the parts) adds (K + 8) u of the sum of the absolute terms.  -> dict of the absolute bounds of ``wsum``,
    ``mean``, ``cov`` and ``ess``"""
    u = 2.0 ** -53
    n = K + 8
    A1, A2 = ref["A1"], ref["A2"]
    return {"wsum": n * u * ref["wsum"],
            "mean": 2 * n * u * A1 + 2 * u * np.abs(np.nan_to_num(ref["mean"])),
            "cov": 2 * n * u * (A2 + 2 * A1[:, :, None] * A1[:, None, :]),
            "ess": 4 * n * u * ref["ess"]}


def grid_twin(ncol, seed=3):
    """The linear-Gaussian twin on a grid: m = q A^T on the regular 65 x 65 grid of [-1, 1]^2 (spacing h = 1/32), one inv_sigma s for
    all rows chosen so that the smallest posterior standard deviation (the root of the smallest eigenvalue of C = (A^T A)^-1 / s^2) is
    2 h; truths in [-0.3, 0.3]^2, observed with a noise of 0.2 / s.  -> q, m, y, inv_sigma, the analytic means (ncol, 2), C"""
    h = 1.0 / 32.0
    g = np.arange(-32, 33) * h
    q = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    A = np.array([[1.0, 0.1], [0.1, 1.0], [0.5, -0.4], [-0.3, 0.6]])
    G = np.linalg.inv(A.T @ A)
    s = np.sqrt(np.linalg.eigvalsh(G).min()) / (2 * h)
    C = G / s ** 2
    rng = np.random.default_rng(seed)
    truth = rng.uniform(-0.3, 0.3, size=(ncol, 2))
    y = truth @ A.T + (0.2 / s) * rng.normal(size=(ncol, 4))
    mu = y @ A @ G  # (A^T W A)^-1 A^T W y with W = s^2 I
    return q, [q @ A.T], [y], [np.full((ncol, 4), s)], mu, C
