"""GPU: the look-up-table posterior (include_post/crt1d_hip_lut_posterior.h; batched.LutPosteriorPlan, ``plan.lut_posterior()``,
``posterior=True``).

1. The entry against tests/lut_posterior_reference.py on synthetic tables: index and cost bitwise, the sums within the rounding bounds.
2. Exact cases, bitwise: one candidate far better than all others; all table rows identical with q on a dyadic grid.
3. Batch independence at a fixed ksplit, bitwise; agreement across ksplit within the bounds.
4. Columns without a result, and a candidate that enters no sum.
5. The linear-Gaussian grid twin of tests/test_lut_posterior_cpu.py on the device.
6. A bimodal misfit surface: the case a local covariance cannot report.
7. Through RetrievalPlan, SpectralRetrievalPlan and Model.retrieve.
8. Capture into a graph.

Measured on MI355X, the largest fraction of each bound of 1. over its 20 cases: wsum 0.125, mean 0.120, cov 0.076, ess 0.082 (all at
K = 15); the grid twin of 5.: 1.2e-15 and 7.2e-16 against 1e-10."""
import ctypes
import functools

import numpy as np
import pytest

import lut_posterior_reference as P
import lut_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FIELDS = ("index", "cost", "mean", "cov", "wsum", "ess")
SENTINEL = -7.25


def _t(v):
    import torch

    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


def _posterior(q, m, y, w=None, prior=None, wp=None, temperature=1.0, ksplit=0):
    """The C entry on blocks of any row counts.  ``temperature``: a number, or ``(ncol,)`` for temperature_col (the scalar is then 1).
    mean and cov are pre-filled with SENTINEL.  -> dict of NumPy arrays, and the kernel's note"""
    import torch

    from crt1d_amd import _lib

    lib = _lib.load()
    ncol, (K, npar), nblk = y[0].shape[0], q.shape, len(m)
    dq, dm, dy = _t(q), [_t(a) for a in m], [_t(a) for a in y]
    dw = [None if (w is None or a is None) else _t(a) for a in (w or [None] * nblk)]
    dp, dwp = (None, None) if prior is None else (_t(prior), _t(wp))
    tcol = None if np.ndim(temperature) == 0 else _t(np.asarray(temperature, dtype=np.float64))
    new = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")  # noqa: E731
    out = {"index": torch.full((ncol,), -7, dtype=torch.int32, device="cuda"), "cost": new(ncol), "mean": new(ncol, npar),
           "cov": new(ncol, npar, npar), "wsum": new(ncol), "ess": new(ncol)}
    need = lib.crt_hip_lut_posterior_workspace_bytes(ncol, K, npar, ksplit)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    p4 = lambda v: (ctypes.c_void_p * 4)(*[ptr(a) for a in v])  # noqa: E731
    T = _lib.CrtLutTable(K, npar, nblk, (ctypes.c_int32 * 4)(*[a.shape[1] for a in m]), ptr(dq), p4(dm))
    O = _lib.CrtLutObs(ncol, p4(dy), p4(dw), ptr(dp), ptr(dwp))
    X = _lib.CrtLutPosteriorOut(1.0 if tcol is not None else float(temperature), ptr(tcol), ksplit, *[ptr(out[k]) for k in FIELDS])
    st = lib.crt_hip_lut_posterior_f64(ctypes.byref(T), ctypes.byref(O), ctypes.byref(X), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, lib.crt_hip_last_kernel().decode()


def _same(a, b, fields=FIELDS):
    return all(a[k].tobytes() == b[k].tobytes() for k in fields)


def _within(got, ref, K):
    """index and cost bitwise, the rest within the bounds of the reference; -> the largest fraction of each bound"""
    assert got["index"].tobytes() == ref["index"].tobytes() and got["cost"].tobytes() == ref["cost"].tobytes()
    has = ref["index"] >= 0
    bound = P.bounds(ref, K)
    frac = {}
    for k in ("wsum", "mean", "cov", "ess"):
        err, b = np.abs(got[k][has] - ref[k][has]), bound[k][has]
        assert np.all(err <= b), (k, float(np.max(err / np.maximum(b, 1e-300))))
        frac[k] = float(np.max(err[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0
    return frac


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
def _case(ncol, K, rows, npar, prior, temp, seed):
    """A table on a line: m[k] = base + a_k v with the a_k a jittered regular grid of [0, 1] in random order, so that the cost of
    candidate k for a column observing candidate kc is 0.5 |s v|^2 (a_k - a_kc)^2 / T-scaled: cost - cmin spans 0 to about 60 T for a
    column near an end of the line (19 T in the middle), and the neighbours on the grid keep ess above 3 from K = 15 on.  The columns
    observe candidates of the inner 80 % of the line plus noise, with weights that differ by row and column (scaled by sqrt(T) of the
    column, so that the weights exp(-(cost - cmin) / T) see the same spread at every temperature), masked rows that hold NaN, and a weak
    prior.  q is unrelated to the line: the moments are those of a cloud.  -> q, m, y, w, prior, wp, T (a number or (ncol,))"""
    rng = np.random.default_rng(seed)
    n = sum(rows)
    a = (rng.permutation(K) + 0.5 + 0.2 * rng.uniform(-1, 1, K)) / K
    v = rng.choice([-1.0, 1.0], n) * rng.uniform(0.8, 1.2, n)
    base = rng.normal(size=n)
    full = base[None, :] + a[:, None] * v[None, :]
    q = rng.normal(size=(K, npar))
    inner = np.flatnonzero((a > 0.1) & (a < 0.9)) if K > 1 else np.array([0])
    kc = rng.choice(inner, ncol)
    T = {"col": rng.uniform(0.5, 2.0, ncol)}.get(temp, temp)
    s0 = np.sqrt(2 * 75.0 / np.sum(v * v))  # 0.5 |s0 v|^2 = 75
    wfull = s0 * np.sqrt(np.broadcast_to(T, (ncol,)))[:, None] * rng.uniform(0.9, 1.1, (ncol, n))
    yfull = full[kc] + (0.3 / s0) * rng.normal(size=(ncol, n)) / np.sqrt(n)
    if n >= 16:
        hole = rng.uniform(size=(ncol, n)) < 0.1
        wfull[hole], yfull[hole] = 0.0, np.nan
    cut = np.cumsum((0,) + tuple(rows))
    split = lambda t: [np.ascontiguousarray(t[:, i:j]) for i, j in zip(cut[:-1], cut[1:])]  # noqa: E731
    pr = wp = None
    if prior:
        pr, wp = q[kc] + 0.1 * rng.normal(size=(ncol, npar)), rng.uniform(0.05, 0.2, (ncol, npar))
        wp[rng.uniform(size=wp.shape) < 0.3] = 0.0
    return q, split(full), split(yfull), split(wfull), pr, wp, T


CASES = [  # ncol, K, rows, npar, prior, temperature
    (1, 1, (1,), 1, False, 1.0),
    (1, 15, (16,), 4, True, 0.25),
    (63, 15, (17,), 5, False, "col"),
    (63, 64, (40,), 10, True, 1.0),
    (65, 64, (1,), 1, False, 1.0),
    (65, 65, (16,), 4, True, "col"),
    (65, 200, (17, 16, 1), 5, True, 1.0),
    (130, 200, (40,), 10, False, 0.25),
    (130, 1000, (16,), 5, True, 1.0),
    (130, 1000, (1, 17, 40), 10, True, "col"),
    (1, 1000, (17,), 4, False, 1.0),
    (63, 1000, (40, 1, 16), 1, False, 0.25),
    (1, 64, (16, 1, 17), 10, True, 1.0),
    (63, 65, (40,), 4, False, "col"),
    (65, 15, (1,), 10, False, 1.0),
    (130, 15, (17,), 1, True, 1.0),
    (1, 200, (40,), 5, True, "col"),
    (65, 1000, (1,), 4, False, 0.25),
    (130, 65, (16,), 5, False, 1.0),
    (63, 200, (17,), 10, True, 0.25),
]


@pytest.mark.parametrize("ncol,K,rows,npar,prior,temp", CASES)
def test_against_the_reference(ncol, K, rows, npar, prior, temp):
    """ess > 3 is asserted on the reference first (K = 1 has one candidate: ess is 1 there, exactly), and the spread of cost - cmin."""
    q, m, y, w, pr, wp, T = _case(ncol, K, rows, npar, prior, temp, seed=ncol + K + sum(rows) + npar)
    ref = P.lut_posterior(q, m, y, w, pr, wp, temperature=T)
    assert (ref["index"] >= 0).all()
    if K == 1:
        assert (ref["ess"] == 1.0).all()
    else:
        span = np.nanmax(R.lut_cost(q, m, y, w, pr, wp) - ref["cost"][:, None], axis=1) / np.broadcast_to(T, (ncol,))
        assert (ref["ess"] > 3.0).all() and span.min() > 5.0 and span.max() < 120.0, (ref["ess"].min(), span.min(), span.max())
    got, note = _posterior(q, m, y, w, pr, wp, temperature=T)
    assert note.startswith(f"k_lut_moments np={npar} ") and f"nblk={len(rows) + bool(prior)} " in note
    frac = _within(got, ref, K)
    best = R.lut_match(q, m, y, w, pr, wp, nbest=1)
    assert got["index"].tobytes() == best[0][:, 0].tobytes() and got["cost"].tobytes() == best[1][:, 0].tobytes()
    print(f"posterior ncol={ncol} K={K} rows={rows} npar={npar}: fractions of the bounds " + " ".join(f"{k} {v:.3f}" for k, v in frac.items()))
    # the covariance is symmetric to the bit (the lower triangle computed and mirrored)
    assert got["cov"].tobytes() == np.swapaxes(got["cov"], 1, 2).copy().tobytes()


def test_cost_is_the_cost_of_the_match_entry():
    """cost bitwise what the match entry gives on the device, through both plans on one table."""
    import torch

    from crt1d_amd import batched

    q, m, y, w, pr, wp, _ = _case(70, 300, (24,), 3, True, 1.0, seed=4)
    table = batched.LutTable(_t(q), {"I_df_u": _t(m[0])}, params=("dir0", "dir1", "dir2"), keys=("I_df_u",), shape=(1, 24), scheme="2s",
                             spectral=False)
    kw = dict(inv_sigma={"I_df_u": _t(w[0]).reshape(70, 1, 24)}, prior=pr, inv_sigma_prior=wp)
    yk = {"I_df_u": _t(y[0]).reshape(70, 1, 24)}
    match = batched.lut_match(table, yk, **kw)
    tcol = torch.full((70,), 0.5, dtype=torch.float64, device="cuda")
    plan = batched.LutPosteriorPlan(table, yk, **kw, temperature=tcol)
    post = plan()
    torch.cuda.synchronize()
    assert plan.last_kernel().startswith("k_lut_moments np=3 ")
    assert torch.equal(post["index"], match["index"][:, 0]) and post["cost"].cpu().numpy().tobytes() == match["cost"][:, 0].cpu().numpy().tobytes()
    assert post["mean"].shape == (70, 3) and post["cov"].shape == (70, 3, 3) and post["ess"].shape == post["wsum"].shape == (70,)
    ref = P.lut_posterior(q, m, y, w, pr, wp, temperature=0.5)
    _within({k: v.cpu().numpy() for k, v in post.items()}, ref, 300)
    # the scalar temperature is the same arithmetic: bitwise the per-column one
    one = batched.lut_posterior(table, yk, **kw, temperature=0.5)
    torch.cuda.synchronize()
    assert all(torch.equal(one[k], post[k]) for k in FIELDS)
    # the temperature is read where it lies at every call
    tcol[3] = float("nan")
    again = plan()
    torch.cuda.synchronize()
    assert int(again["index"][3]) == -1 and bool(torch.isnan(again["mean"][3]).all()) and bool(torch.isnan(again["cov"][3]).all())
    assert torch.equal(again["mean"][4:], one["mean"][4:])


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_one_candidate_dominates():
    """cost - cmin > 800 for every other candidate: their weights underflow to exactly 0.  mean is bitwise q[kb], cov exactly +0."""
    rng = np.random.default_rng(21)
    ncol, K, n, npar = 70, 200, 16, 5
    q, m = rng.normal(size=(K, npar)), [rng.normal(size=(K, n))]
    kc = rng.integers(0, K, ncol)
    y, w = [m[0][kc] + 1e-6 * rng.normal(size=(ncol, n))], [np.full((ncol, n), 40.0)]
    cost = R.lut_cost(q, m, y, w)
    rest = np.sort(cost, axis=1)
    assert (rest[:, 1] - rest[:, 0] > 800.0).all()
    got, _ = _posterior(q, m, y, w)
    assert got["index"].tolist() == kc.tolist()
    assert got["mean"].tobytes() == q[kc].tobytes()
    assert got["cov"].tobytes() == np.zeros((ncol, npar, npar)).tobytes()  # +0, every bit
    assert got["ess"].tobytes() == np.ones(ncol).tobytes() and got["wsum"].tobytes() == np.ones(ncol).tobytes()


def test_exact_identical_rows():
    """All K = 200 table rows identical, q on a dyadic grid (multiples of 1/64 in [-1, 1]): every weight is exactly 1 and every sum is
    exact in any order.  mean and cov are bitwise the contract's finish arithmetic in NumPy; three ksplit give the same bits."""
    rng = np.random.default_rng(22)
    ncol, K, n, npar = 5, 200, 17, 4
    q = rng.integers(-64, 65, size=(K, npar)) / 64.0
    m = [np.tile(rng.normal(size=(1, n)), (K, 1))]
    y, w = [rng.normal(size=(ncol, n))], [rng.uniform(0.5, 2.0, size=(ncol, n))]
    d = q - q[0]
    s1, s2 = d.sum(axis=0), np.einsum("ki,kj->ij", d, d)
    mean, cov, ess, wsum = P.finish(q[0], float(K), float(K), s1, s2)
    for ksplit in (0, 1, 3):
        got, _ = _posterior(q, m, y, w, temperature=0.25, ksplit=ksplit)
        assert (got["index"] == 0).all() and (got["wsum"] == K).all() and (got["ess"] == K).all() and ess == K and wsum == K
        assert got["mean"].tobytes() == np.tile(mean, (ncol, 1)).tobytes()
        assert got["cov"].tobytes() == np.tile(cov, (ncol, 1, 1)).tobytes()


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    return _case(130, 1000, (13, 1, 40), 5, True, "col", seed=77)


def _take(case, idx):
    q, m, y, w, pr, wp, T = case
    return q, m, [a[idx] for a in y], [a[idx] for a in w], pr[idx], wp[idx], T[idx]


def _run(case, ksplit):
    q, m, y, w, pr, wp, T = case
    return _posterior(q, m, y, w, pr, wp, temperature=T, ksplit=ksplit)[0]


@pytest.mark.parametrize("ksplit", [1, 3])
def test_batch_independence(ksplit):
    """At a fixed explicit ksplit a column's six outputs are bitwise the same alone, at positions 0, 63, 64 and 129 of a batch of 130 and
    after a permutation of the batch, and do not change when another column's observations become NaN or fully masked."""
    case = _batch()
    whole = _run(case, ksplit)
    col = 17
    alone = _run(_take(case, np.array([col])), ksplit)
    assert all(alone[k][0].tobytes() == whole[k][col].tobytes() for k in FIELDS)
    idx = np.arange(130)
    idx[[0, 63, 64, 129]] = col
    placed = _run(_take(case, idx), ksplit)
    for pos in (0, 63, 64, 129):
        assert all(placed[k][pos].tobytes() == alone[k][0].tobytes() for k in FIELDS), pos
    perm = np.random.default_rng(1).permutation(130)
    shuffled = _run(_take(case, perm), ksplit)
    assert all(shuffled[k].tobytes() == whole[k][perm].tobytes() for k in FIELDS)
    q, m, y, w, pr, wp, T = case
    y2, w2 = [a.copy() for a in y], [a.copy() for a in w]
    for b in range(len(y)):
        y2[b][16] = np.nan  # observed NaN: column 16 has no eligible candidate
        w2[b][16] = np.where(w2[b][16] == 0.0, 1.0, w2[b][16])
        y2[b][18], w2[b][18] = np.nan, 0.0  # column 18 fully masked
    other = _run((q, m, y2, w2, pr, wp, T), ksplit)
    keep = np.setdiff1d(np.arange(130), [16, 18])
    assert all(other[k][keep].tobytes() == whole[k][keep].tobytes() for k in FIELDS)
    assert other["index"][16] == -1 and other["index"][18] >= 0


def test_agreement_across_ksplit():
    """Across ksplit in {1, 2, 3, 7} and automatic the sums are formed in different orders: within the bounds of test 1, index and cost
    bitwise."""
    case = _batch()
    q, m, y, w, pr, wp, T = case
    ref = P.lut_posterior(q, m, y, w, pr, wp, temperature=T)
    runs = {ks: _run(case, ks) for ks in (0, 1, 2, 3, 7)}
    for ks, got in runs.items():
        _within(got, ref, 1000)
        assert _same(got, runs[1], ("index", "cost")), ks
    assert _same(runs[0], _run(case, 16)) and _same(runs[0], _run(case, 200))  # automatic is 16 parts here; beyond that it is clamped


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def test_columns_without_a_result():
    """In one batch: a column with an all-NaN observed row and columns with temperature_col 0, -1, NaN and inf get -1, +inf, wsum = ess = 0
    and keep the sentinel in mean and cov; their neighbours are bitwise what they are in the batch without them."""
    q, m, y, w, pr, wp, _ = _case(12, 200, (16, 17), 4, True, 1.0, seed=41)
    T = np.linspace(0.5, 1.5, 12)
    clean, _ = _posterior(q, m, y, w, pr, wp, temperature=T)
    assert (clean["index"] >= 0).all() and not (clean["mean"] == SENTINEL).any()
    T2, y2, w2 = T.copy(), [a.copy() for a in y], [a.copy() for a in w]
    T2[[2, 3, 4, 5]] = [0.0, -1.0, np.nan, np.inf]
    y2[1][7], w2[1][7] = np.nan, 1.0
    got, _ = _posterior(q, m, y2, w2, pr, wp, temperature=T2)
    bad, good = [2, 3, 4, 5, 7], [0, 1, 6, 8, 9, 10, 11]
    assert (got["index"][bad] == -1).all() and (got["cost"][bad] == np.inf).all()
    assert got["wsum"][bad].tobytes() == np.zeros(5).tobytes() and got["ess"][bad].tobytes() == np.zeros(5).tobytes()
    assert (got["mean"][bad] == SENTINEL).all() and (got["cov"][bad] == SENTINEL).all()
    assert all(got[k][good].tobytes() == clean[k][good].tobytes() for k in FIELDS)
    ref = P.lut_posterior(q, m, y2, w2, pr, wp, temperature=T2)
    assert (ref["index"][bad] == -1).all()
    _within(got, ref, 200)
    # a NaN in every table row of one block: no column has a candidate
    m2 = [m[0], m[1].copy()]
    m2[1][:, 3] = np.nan
    none, _ = _posterior(q, m2, y, w, pr, wp, temperature=T)
    assert (none["index"] == -1).all() and np.isinf(none["cost"]).all() and (none["wsum"] == 0).all() and (none["ess"] == 0).all()
    assert (none["mean"] == SENTINEL).all() and (none["cov"] == SENTINEL).all()


def test_plan_keeps_the_nan_fill():
    import torch

    from crt1d_amd import batched

    q, m, y, w, _, _, _ = _case(6, 100, (16,), 3, False, 1.0, seed=42)
    y[0][2] = np.inf
    w[0][2] = 1.0
    table = batched.LutTable(_t(q), {"F": _t(m[0])}, params=("a", "b", "c"), keys=("F",), shape=(1, 16), scheme="2s", spectral=False)
    T = torch.tensor([1.0, 0.0, 1.0, 1.0, -2.0, 1.0], dtype=torch.float64, device="cuda")
    plan = batched.LutPosteriorPlan(table, {"F": _t(y[0]).reshape(6, 1, 16)}, inv_sigma={"F": _t(w[0]).reshape(6, 1, 16)}, temperature=T)
    for _ in range(2):  # (the fill is renewed before every call)
        out = plan()
        torch.cuda.synchronize()
        bad = [1, 2, 4]
        assert out["index"].tolist() == [int(i) if c not in bad else -1 for c, i in enumerate(out["index"].tolist())]
        assert bool(torch.isnan(out["mean"][bad]).all()) and bool(torch.isnan(out["cov"][bad]).all())
        assert bool((out["index"][bad] == -1).all()) and bool(torch.isinf(out["cost"][bad]).all())
        assert bool((out["wsum"][bad] == 0).all()) and bool((out["ess"][bad] == 0).all())
        assert bool(torch.isfinite(out["mean"][[0, 3, 5]]).all()) and bool(torch.isfinite(out["cov"][[0, 3, 5]]).all())


def test_a_nan_candidate_enters_no_sum():
    """One candidate with a NaN in its table row (and, with the prior, in its q): every column's result is bitwise that of the table
    where this candidate lies so far off that its weight underflows to 0 -- the same summation order, a term of exactly +0 -- and within
    the bounds of the reference on the table without it."""
    q, m, y, w, pr, wp, T = _case(70, 200, (16, 17), 4, True, "col", seed=43)
    k = int(np.flatnonzero(np.arange(200) != P.lut_posterior(q, m, y, w, pr, wp, temperature=T)["index"][0])[5])
    qn, mn = q.copy(), [a.copy() for a in m]
    mn[0][k, 2], qn[k, 1] = np.nan, np.nan
    far = [a.copy() for a in m]
    far[0][k] += 1e4
    a, _ = _posterior(qn, mn, y, w, pr, wp, temperature=T)
    b, _ = _posterior(q, far, y, w, pr, wp, temperature=T)
    assert _same(a, b) and np.isfinite(a["mean"]).all() and np.isfinite(a["cov"]).all() and not (a["index"] == k).any()
    keep = np.arange(200) != k
    ref = P.lut_posterior(q[keep], [t[keep] for t in m], y, w, pr, wp, temperature=T)
    ref["index"] = np.where(ref["index"] >= k, ref["index"] + 1, ref["index"]).astype(np.int32)
    _within(a, ref, 200)
    _within(a, P.lut_posterior(qn, mn, y, w, pr, wp, temperature=T), 200)  # the reference on the NaN table itself


# ---- 5. and 6. ----------------------------------------------------------------------------------------------------------------------------
def _grid_table(q, m):
    from crt1d_amd import batched

    return batched.LutTable(_t(q), {"F": _t(m)}, params=("q0", "q1"), keys=("F",), shape=(1, m.shape[1]), scheme="2s", spectral=False)


def test_grid_twin_on_the_device():
    """The linear-Gaussian grid twin of the CPU file with 64 columns: the same bar, 1e-10 of the largest posterior standard deviation and of
    max |C| (discretisation < 1e-34, box edge < 1e-16, rounding of order K u = 5e-13)."""
    import torch

    from crt1d_amd import batched

    q, m, y, w, mu, C = P.grid_twin(64)
    sd = np.sqrt(np.linalg.eigvalsh(C))
    assert (1.0 - np.abs(mu).max()) / sd.max() >= 8.7
    out = batched.lut_posterior(_grid_table(q, m[0]), {"F": _t(y[0]).reshape(64, 1, 4)}, inv_sigma={"F": _t(w[0]).reshape(64, 1, 4)})
    torch.cuda.synchronize()
    err_mean = np.abs(out["mean"].cpu().numpy() - mu).max() / sd.max()
    err_cov = np.abs(out["cov"].cpu().numpy() - C).max() / np.abs(C).max()
    print(f"grid twin on the device: mean {err_mean:.2e} of the largest sd, cov {err_cov:.2e} of max |C|, ess {float(out['ess'].min()):.1f}")
    assert err_mean < 1e-10 and err_cov < 1e-10


def test_bimodal():
    """m(q) = (q0^2, q1) on the 65 x 65 grid of [-1, 1]^2, truth (0.5, 0.1): two basins at q0 = +-0.5 that the observations cannot tell
    apart.  index lands in one of them; the mean lies between them, |mean_0| < 0.05 (the table's symmetry q0 -> -q0 makes it 0 up to
    rounding), and cov_00 is within 2 % of 0.5^2: the distance of the basins, not the width of one.  The 2 % is the width of each mode,
    sigma_0^2, against 0.5^2; inv_sigma = (1 / 0.035, 16) makes sigma_0 = 0.035 <= 0.05 in q0 (d q0^2 / d q0 = 1 at 0.5) and 2 h in q1."""
    import torch

    from crt1d_amd import batched

    g = np.arange(-32, 33) / 32.0
    q = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    m = np.stack([q[:, 0] ** 2, q[:, 1]], axis=1)
    y, w = np.array([[0.25, 0.1]]), np.array([[1.0 / 0.035, 16.0]])
    out = batched.lut_posterior(_grid_table(q, m), {"F": _t(y).reshape(1, 1, 2)}, inv_sigma={"F": _t(w).reshape(1, 1, 2)})
    torch.cuda.synchronize()
    kb = int(out["index"][0])
    mean, cov = out["mean"][0].cpu().numpy(), out["cov"][0].cpu().numpy()
    print(f"bimodal: best q = {q[kb]}, mean = {mean}, cov_00 = {cov[0, 0]:.5f}, sd_1 = {np.sqrt(cov[1, 1]):.4f}, ess = {float(out['ess'][0]):.1f}")
    assert abs(q[kb, 0]) == 0.5 and abs(q[kb, 1] - 0.1) <= 1.0 / 64.0
    assert abs(mean[0]) < 0.05 and abs(mean[1] - 0.1) < 0.01
    assert abs(cov[0, 0] - 0.25) < 0.02 * 0.25
    assert abs(np.sqrt(cov[1, 1]) - 0.0625) < 0.001  # the unimodal direction: the width of the mode


# ---- 7. ---------------------------------------------------------------------------------------------------------------------------------
def _template():
    """One 2s column of 12 bands and 6 levels, 3 sensor bands; ln LAI and one leaf-reflectance direction as the parameters; K = 256."""
    from crt1d_amd import batched, synth

    nb, nz = 12, 6
    d = synth.make_columns(1, nb, nz, seed=5)
    cols = batched.Columns.from_host(d, "cuda:0")
    bands = batched.Bands.from_host(d, "cuda:0")
    dirn = _t(0.3 * d["leaf_r"].mean(axis=0) * np.sin(np.linspace(0.0, 3.0, nb)))[None]
    sw = np.zeros((3, nb))
    for s in range(3):
        sw[s, 4 * s:4 * s + 4] = 1.0
    lo, hi = np.array([-0.2, -0.3]), np.array([0.2, 0.3])
    return dict(cols=cols, bands=bands, dirn=dirn, sensors=batched.SensorSet(sw), lo=lo, hi=hi, q=batched.lut_sample(lo, hi, 256, include=[0.0, 0.0]))


@pytest.mark.parametrize("spectral", [False, True])
def test_through_the_retrieval_plans(spectral):
    import torch

    from crt1d_amd import batched

    T, ncol, keys, levels = _template(), 8, ("I_df_u",), (0, -1)
    axis = dict(d_leaf_r=T["dirn"], lai=True)
    sens = {} if spectral else dict(sensors=T["sensors"])
    table = batched.LutTable.build("2s", T["cols"], T["bands"], levels, T["q"], keys=keys, **sens, **axis)
    assert table.ncand == 256 and table.npar == 2
    rng = np.random.default_rng(8)
    pick = _t(rng.integers(0, 256, ncol))
    y = {"I_df_u": (table.m["I_df_u"][pick] * _t(1.0 + 0.01 * rng.normal(size=(ncol, table.nrow)))).reshape(ncol, *table.shape).contiguous()}
    w = {"I_df_u": (20.0 / table.m["I_df_u"].abs().mean()).item() * torch.ones_like(y["I_df_u"])}
    rep = lambda v: None if v is None else v.expand(ncol, *v.shape[1:]).contiguous()  # noqa: E731
    c = T["cols"]
    cols = batched.Columns(rep(c.psi), rep(c.lai), rep(c.g_kind), rep(c.g_param), rep(c.mla), rep(c.g_at_psi), rep(c.g_table))
    pr = dict(prior=np.array([0.05, -0.1]), inv_sigma_prior=np.array([3.0, 0.0]))
    common = dict(keys=keys, inv_sigma=w, lo=T["lo"], hi=T["hi"], **axis, **pr)
    if spectral:
        make = lambda p0: batched.SpectralRetrievalPlan("2s", cols, T["bands"], levels, y, p0=p0, **common)  # noqa: E731
    else:
        make = lambda p0: batched.RetrievalPlan("2s", cols, T["bands"], levels, T["sensors"], y, p0=p0, **common)  # noqa: E731
    plan = make(table)
    post = plan.lut_posterior()
    torch.cuda.synchronize()
    assert torch.equal(post["index"], plan.lut.index[:, 0])
    assert post["cost"].cpu().numpy().tobytes() == plan.lut.cost[:, 0].cpu().numpy().tobytes()
    assert post["mean"].shape == (ncol, 2) and post["cov"].shape == (ncol, 2, 2) and bool((post["ess"] >= 1.0).all())
    ref = P.lut_posterior(table.q.cpu().numpy(), [table.m["I_df_u"].cpu().numpy()], [y["I_df_u"].reshape(ncol, -1).cpu().numpy()],
                          [w["I_df_u"].reshape(ncol, -1).cpu().numpy()], np.tile(pr["prior"], (ncol, 1)), np.tile(pr["inv_sigma_prior"], (ncol, 1)))
    _within({k: v.cpu().numpy() for k, v in post.items()}, ref, 256)
    inner = plan._post[1]
    assert plan.lut_posterior()["mean"] is post["mean"] and plan._post[1] is inner  # built once, reused
    cold = plan.lut_posterior(temperature=0.25)
    torch.cuda.synchronize()
    assert plan._post[1] is not inner and bool((cold["ess"] <= ref["ess"].max()).all()) and torch.equal(cold["index"], plan.lut.index[:, 0])
    with pytest.raises(ValueError, match="needs a plan started from a look-up table"):
        make(None).lut_posterior()
    # the one-shot form: the three extra keys, the rest bitwise the call without them
    one = batched.retrieve_spectral if spectral else batched.retrieve
    args = ("2s", cols, T["bands"], levels) + (() if spectral else (T["sensors"],)) + (y,)
    a, b = one(*args, niter=3, p0=table, posterior=True, **common), one(*args, niter=3, p0=table, **common)
    torch.cuda.synchronize()
    assert set(a) - set(b) == {"lut_mean", "lut_cov", "lut_ess"}
    assert all(k == "params" or a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in b)
    assert torch.equal(a["lut_mean"], post["mean"]) and torch.equal(a["lut_cov"], post["cov"]) and torch.equal(a["lut_ess"], post["ess"])


def test_model_retrieve_posterior():
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=6)
    nb = m.nwl
    w = np.zeros((3, nb))
    w[0, : nb // 2], w[1, nb // 3:], w[2, nb // 2] = 1.0, 0.5, 2.0
    d = np.random.default_rng(3).uniform(-0.05, 0.05, (1, nb)) * m.copy_p()["leaf_r"]
    y = {"I_df_u": 1.03 * m.run_sensors(w, levels=(-1,))["I_df_u"]}
    lo, hi = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    kw = dict(levels=(-1,), directions={"leaf_r": d}, lai=True, niter=4, lo=lo, hi=hi, lut=256)
    got, plain = m.retrieve(w, y, posterior=True, **kw), m.retrieve(w, y, **kw)
    assert set(got) - set(plain) == {"lut_mean", "lut_cov", "lut_ess"}
    assert got["lut_mean"].shape == (2,) and got["lut_cov"].shape == (2, 2) and got["lut_ess"].shape == () and got["lut_ess"] >= 1.0
    assert (got["lut_mean"] >= lo).all() and (got["lut_mean"] <= hi).all() and np.array_equal(got["lut_cov"], got["lut_cov"].T)
    assert all(k == "params" or got[k].tobytes() == plain[k].tobytes() for k in plain) and got["params"] == plain["params"]
    ys = {"I_df_u": 1.03 * m.run_series_levels(np.atleast_1d(float(m._p["psi"])), (-1,))["I_df_u"][0]}
    kw.pop("lut")
    gs = m.retrieve_spectral(ys, posterior=True, lut=256, **kw)
    ps = m.retrieve_spectral(ys, lut=256, **kw)
    assert gs["lut_mean"].shape == (2,) and gs["lut_cov"].shape == (2, 2) and gs["lut_ess"].shape == ()
    assert all(k == "params" or gs[k].tobytes() == ps[k].tobytes() for k in ps)
    with pytest.raises(ValueError, match="posterior=True needs lut=K"):
        m.retrieve(w, y, posterior=True, **kw)


# ---- 8. ---------------------------------------------------------------------------------------------------------------------------------
def test_capture():
    """The plan call captured into a graph after one eager call, on one stream: the replay is bitwise the eager result, also after the
    observations have changed in place."""
    import torch

    from crt1d_amd import batched

    q, m, y, w, pr, wp, _ = _case(70, 300, (24,), 3, True, 1.0, seed=9)
    table = batched.LutTable(_t(q), {"F": _t(m[0])}, params=("a", "b", "c"), keys=("F",), shape=(1, 24), scheme="2s", spectral=False)
    yk = {"F": _t(y[0]).reshape(70, 1, 24)}
    wk = {"F": _t(w[0]).reshape(70, 1, 24)}
    plan = batched.LutPosteriorPlan(table, yk, inv_sigma=wk, prior=pr, inv_sigma_prior=wp, ksplit=2)
    eager = {k: v.clone() for k, v in plan().items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            plan(s)
    for v in plan().values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(eager[k].cpu().numpy().tobytes() == getattr(plan, k).cpu().numpy().tobytes() for k in FIELDS)
    yk["F"][5], wk["F"][5] = yk["F"][6], wk["F"][6]  # (the plan reads its inputs where they lie: column 5 now observes what column 6 does)
    graph.replay()
    torch.cuda.synchronize()
    after = {k: getattr(plan, k).cpu().numpy() for k in FIELDS}
    again = plan()
    torch.cuda.synchronize()
    assert all(after[k].tobytes() == again[k].cpu().numpy().tobytes() for k in FIELDS)
    assert np.isfinite(after["mean"]).all() and not np.array_equal(after["mean"][5], eager["mean"][5].cpu().numpy())
