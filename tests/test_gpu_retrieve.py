"""GPU: the per-column Levenberg-Marquardt retrieval (include/crt1d_hip_retrieve.h; batched.RetrievalPlan, batched.retrieve,
Model.retrieve).

1. The normal equations of k_lm_step: bitwise a NumPy restatement of the summation order the header documents; batch invariance.
2. The damped solve against batched.gauss_newton_step on host copies, to a bound that follows from the conditioning.
3. The state machine on a linear problem f = M p_trial formed in torch between calls of the step entry alone.
4. k_retrieve_apply: bitwise the torch expression in the stated order.
5. The covariance against numpy.linalg.inv.
6. - 8. The retrieval problems of tests/test_gpu_sensjac.py and tests/test_gpu_sensjac_series.py, restated here, against the host loop of
   sensor_jacobian + solve_sensor_levels + gauss_newton_step (the reference, not the code under test); one composed scheme.
9. Model.retrieve is the batched call.

EPS = 2^-52.  The bound of 2.: the scaled damped matrix has a unit diagonal plus lam, so its eigenvalues lie in [lam, npar + lam]; a
Cholesky solve of an n x n system is backward stable with a constant of a few n eps, so the error relative to max |delta| in the scaled
variables is allowed 32 npar EPS (npar + lam) / lam.  Where lam is (driven to) 0 the ratio (npar + lam) / lam is replaced by the condition
number numpy.linalg.cond reports for the scaled normal matrix of the case."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ELLIPSOIDAL = 3  # leaf_angle.G_ELLIPSOIDAL
STATE = ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")


def _bound(npar, lam=None, cond=None):
    return 32 * npar * EPS * ((npar + lam) / lam if cond is None else cond)


class LM:
    """The step entry on tensors of the test's own: blocks = [dict(f, J, y, s)] of CUDA tensors (s: None = ones)."""

    def __init__(self, blocks, p0, lam0=1e-2, prior=None, isp=None, lo=None, hi=None, **opts):
        import torch

        from crt1d_amd import _lib

        self.lib, self.blocks = _lib.load(), blocks
        ncol, npar = p0.shape
        self.ncol, self.npar = ncol, npar
        f64 = dict(dtype=torch.float64, device="cuda")
        self.p, self.p_trial = p0.clone(), p0.clone()
        self.cost, self.lam = torch.full((ncol,), float("inf"), **f64), torch.full((ncol,), lam0, **f64)
        self.A, self.g = torch.zeros((ncol, npar * (npar + 1) // 2), **f64), torch.zeros((ncol, npar), **f64)
        self.status, self.naccept, self.nreject = (torch.zeros((ncol,), dtype=torch.int32, device="cuda") for _ in range(3))
        o = dict(lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0)
        o.update(opts)
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        self._keep = (prior, isp, lo, hi)
        self._prob = _lib.CrtLmProblem(ncol, npar, o["lam_up"], o["lam_down"], o["lam_min"], o["lam_max"], o["xtol"], o["ftol"], ptr(lo), ptr(hi),
                                       ptr(prior), ptr(isp))
        self._obs = (_lib.CrtLmObs * len(blocks))(*[_lib.CrtLmObs(b["J"].shape[1], ptr(b["f"]), ptr(b["J"]), ptr(b["y"]), ptr(b["s"])) for b in blocks])
        self._state = _lib.CrtLmState(*[ptr(getattr(self, k)) for k in STATE])

    def step(self):
        import torch

        from crt1d_amd import _lib

        st = self.lib.crt_hip_lm_step_f64(ctypes.byref(self._prob), self._obs, len(self.blocks), ctypes.byref(self._state),
                                          torch.cuda.current_stream().cuda_stream)
        assert st == _lib.CRT_OK, st
        return self

    def snap(self):
        import torch

        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in STATE}


def _same(a, b, keys=STATE):
    return all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].tobytes() == b[k].tobytes() for k in keys)


def _t(v):
    import torch

    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


def _pairs(npar):
    """(i, j) of the entries of (A | g | 2 cost): the lower triangle of the (npar + 1) x (npar + 1) matrix of products, row by row."""
    ij = [(i, j) for i in range(npar + 1) for j in range(i + 1)]
    return np.array([i for i, _ in ij]), np.array([j for _, j in ij])


def _normal_ref(blocks, c, npar, p_trial=None, prior=None, isp=None):
    """The header's order for column c in NumPy: one running sum per entry, rows of block 0 ascending, block 1, ..., the prior rows last;
    every product and every sum a separately rounded float64 operation.  -> (A packed, g, cost)"""
    I, Jx = _pairs(npar)
    acc = np.zeros(len(I))
    for b in blocks:
        J, f, y, s = b["J"][c], b["f"][c], b["y"][c], b["s"]
        for o in range(J.shape[0]):
            so = 1.0 if s is None else s[c, o]
            if so == 0.0:
                continue
            v = np.append(J[o] * so, (f[o] - y[o]) * so)
            acc = acc + v[I] * v[Jx]
    if isp is not None:
        for k in range(npar):
            s = isp[c, k]
            if s == 0.0:
                continue
            d = (p_trial[c, k] - prior[c, k]) * s
            v = np.zeros(npar + 1)
            v[k], v[npar] = s, d
            hit = ((I == k) | (I == npar)) & ((Jx == k) | (Jx == npar))  # (k, k), (npar, k), (npar, npar)
            acc = np.where(hit, acc + v[I] * v[Jx], acc)
    ntri = npar * (npar + 1) // 2
    return acc[:ntri], acc[ntri:ntri + npar], 0.5 * acc[-1]


def _split(nrow, nblk):
    if nblk == 1:
        return [nrow]
    if nrow < 3:
        return [1, 1, 1]  # (one row cannot be split: three blocks of one row)
    a = nrow // 3
    return [a, a, nrow - 2 * a]


def _random_blocks(rng, ncol, sizes, npar, holes=True):
    """Host blocks: block 0 with weights of which some are 0 (y and f NaN there, never row 0), block 1 without weights, block 2 weighted."""
    blocks = []
    for q, n in enumerate(sizes):
        J = rng.normal(size=(ncol, n, npar)) * rng.uniform(0.1, 10.0, npar)
        f, y = rng.normal(size=(ncol, n)), rng.normal(size=(ncol, n))
        s = None if q == 1 else rng.uniform(0.5, 2.0, (ncol, n))
        if q == 0 and holes:
            dead = rng.uniform(size=(ncol, n)) < 0.25
            dead[:, 0] = False
            s[dead], y[dead], f[dead] = 0.0, np.nan, np.nan
            J[dead] = np.nan
        blocks.append(dict(J=J, f=f, y=y, s=s))
    return blocks


def _dev(blocks, cols=slice(None)):
    return [{k: None if v is None else _t(v[cols]) for k, v in b.items()} for b in blocks]


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("npar", [1, 5, 10])
@pytest.mark.parametrize("nrow", [1, 13, 64, 65, 200])
def test_normal_equations_bitwise(nrow, npar, nblk):
    """After a first step A, g and cost are bitwise the NumPy restatement of the documented order (rows with inv_sigma = 0 hold NaN and
    are skipped; a prior with one unobserved row comes last); column 3 alone gives the bits it gives inside the batch."""
    ncol = 7
    rng = np.random.default_rng(1000 * nrow + 10 * npar + nblk)
    blocks = _random_blocks(rng, ncol, _split(nrow, nblk), npar)
    p0, prior = rng.normal(size=(ncol, npar)), rng.normal(size=(ncol, npar))
    isp = rng.uniform(0.5, 2.0, (ncol, npar))
    isp[:, npar // 2] = 0.0
    prior[:, npar // 2] = np.nan
    lm = LM(_dev(blocks), _t(p0), prior=_t(prior), isp=_t(isp)).step()
    got = lm.snap()
    assert np.all(got["naccept"] == 1) and np.all(got["status"] == 0) and np.array_equal(got["p"], p0)
    for c in range(ncol):
        A, g, cost = _normal_ref(blocks, c, npar, p0, prior, isp)
        assert A.tobytes() == got["A"][c].tobytes() and g.tobytes() == got["g"][c].tobytes() and cost == got["cost"][c], c
    one = LM(_dev(blocks, slice(3, 4)), _t(p0[3:4]), prior=_t(prior[3:4]), isp=_t(isp[3:4])).step().snap()
    assert all(one[k].tobytes() == got[k][3:4].tobytes() for k in STATE)


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
def _scaled(A):
    sc = 1.0 / np.sqrt(np.diagonal(A, axis1=-2, axis2=-1))
    return A * sc[..., :, None] * sc[..., None, :], sc


@pytest.mark.parametrize("lam", [1e-2, 0.5])
@pytest.mark.parametrize("npar", [1, 5, 10])
def test_solve_against_gauss_newton_step(npar, lam):
    """p_trial - p (p = 0: exactly delta) against gauss_newton_step on host copies of the same weighted J, r and lam, relative to
    max |delta| in the scaled variables, bound 32 npar EPS (npar + lam) / lam; gauss_newton_step itself agrees with numpy.linalg.solve
    within that bound on the same cases.  Measured on MI355X, largest error / bound over the six cases: device against host 3.4e-04, host against
    numpy 6.6e-02 (npar = 1, lam = 0.5)."""
    import torch

    from crt1d_amd import batched

    ncol, nrow = 7, 40
    rng = np.random.default_rng(77 + npar)
    blocks = _random_blocks(rng, ncol, [nrow], npar, holes=False)
    b = blocks[0]
    Jw, r = b["J"] * b["s"][:, :, None], (b["f"] - b["y"]) * b["s"]
    lm = LM(_dev(blocks), _t(np.zeros((ncol, npar))), lam0=lam, lam_down=1.0, lam_min=0.0).step()
    got = lm.snap()
    assert np.all(got["lam"] == lam) and np.all(got["p"] == 0)
    ref = batched.gauss_newton_step(torch.as_tensor(Jw), torch.as_tensor(r), damping=lam).numpy()
    A = np.einsum("coi,coj->cij", Jw, Jw)
    sc = 1.0 / np.sqrt(np.diagonal(A, axis1=1, axis2=2))
    exact = np.stack([np.linalg.solve(A[c] + lam * np.diag(np.diag(A[c])), -(Jw[c].T @ r[c])) for c in range(ncol)])
    scale = np.abs(exact / sc).max(axis=1, keepdims=True)
    bound = _bound(npar, lam)
    e_dev = (np.abs(got["p_trial"] - ref) / sc / scale).max()
    e_host = (np.abs(ref - exact) / sc / scale).max()
    print(f"solve npar={npar} lam={lam}: device-host {e_dev:.3e}, host-numpy {e_host:.3e}, bound {bound:.3e}; ratios {e_dev / bound:.2e} {e_host / bound:.2e}")
    assert e_host <= bound and e_dev <= bound


def test_solve_with_a_dead_parameter():
    """A zero Jacobian column gives delta = 0 there; the other entries equal the solve without that column to the same bound."""
    npar, lam, ncol = 5, 1e-2, 7
    rng = np.random.default_rng(5)
    blocks = _random_blocks(rng, ncol, [40], npar, holes=False)
    blocks[0]["J"][:, :, 2] = 0.0
    keep = [0, 1, 3, 4]
    less = [dict(blocks[0], J=np.ascontiguousarray(blocks[0]["J"][:, :, keep]))]
    full = LM(_dev(blocks), _t(np.zeros((ncol, npar))), lam0=lam, lam_down=1.0).step().snap()
    part = LM(_dev(less), _t(np.zeros((ncol, 4))), lam0=lam, lam_down=1.0).step().snap()
    assert np.all(full["p_trial"][:, 2] == 0)
    d = part["p_trial"]
    Jw = less[0]["J"] * less[0]["s"][:, :, None]
    root = np.sqrt(np.einsum("coi,coi->ci", Jw, Jw))  # 1 / sc: to the scaled variables
    err = np.abs(full["p_trial"][:, keep] - d) * root
    assert np.all(err <= _bound(4, lam) * np.abs(d * root).max(axis=1, keepdims=True))


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def _linear(ncol=6, nrow=30, npar=4, seed=9):
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(ncol, nrow, npar))
    truth = rng.normal(size=(ncol, npar))
    noise = 0.05 * rng.normal(size=(ncol, nrow))
    return M, truth, np.einsum("cok,ck->co", M, truth) + noise


def _linear_lm(M, y, p0=None, **kw):
    import torch

    blk = dict(J=_t(M), f=torch.zeros(M.shape[:2], dtype=torch.float64, device="cuda"), y=_t(y), s=None)
    lm = LM([blk], _t(np.zeros((M.shape[0], M.shape[2])) if p0 is None else p0), **kw)

    def evaluate(offset=0.0):
        blk["f"].copy_(torch.einsum("cok,ck->co", blk["J"], lm.p_trial) + offset)
        return lm

    return lm, evaluate


def test_state_machine_accept_reject_stall():
    M, truth, y = _linear()
    lm, evaluate = _linear_lm(M, y, lam0=1e-2, lam_max=5.0)
    s1 = evaluate().step().snap()  # the first call accepts
    assert np.all(s1["naccept"] == 1) and np.all(s1["nreject"] == 0) and np.all(s1["status"] == 0)
    assert np.all(s1["p"] == 0) and np.all(s1["lam"] == 1e-2 * 0.1) and np.all(np.isfinite(s1["cost"]))
    assert np.any(s1["p_trial"] != s1["p"])
    s2 = evaluate(offset=10.0).step().snap()  # a worse f: nothing of the accepted point moves
    assert _same(s1, s2, ("p", "cost", "A", "g", "naccept", "status"))
    assert np.array_equal(s2["lam"], s1["lam"] * 10.0) and np.all(s2["nreject"] == 1)
    s3 = evaluate(offset=float("nan")).step().snap()  # NaN in f is a rejection
    assert _same(s1, s3, ("p", "cost", "A", "g", "naccept", "status"))
    assert np.array_equal(s3["lam"], s2["lam"] * 10.0) and np.all(s3["nreject"] == 2)
    s4 = evaluate(offset=10.0).step().snap()  # lam = 1e-1 -> 1: not yet beyond lam_max = 5
    assert np.all(s4["status"] == 0) and np.array_equal(s4["lam"], s3["lam"] * 10.0)
    s5 = evaluate(offset=10.0).step().snap()  # lam > lam_max: stalled, the trial point goes back to p
    assert np.all(s5["status"] == 3) and np.array_equal(s5["p_trial"], s5["p"]) and _same(s1, s5, ("p", "cost", "A", "g"))
    for _ in range(3):  # a finished column: no state bit changes any more, whatever is evaluated
        evaluate(offset=-1.0).step()
    assert _same(s5, lm.snap())


def test_state_machine_failed_start():
    M, truth, y = _linear()
    y[2, 5] = np.nan
    lm, evaluate = _linear_lm(M, y)
    s = evaluate().step().snap()
    assert s["status"][2] == 4 and np.all(np.delete(s["status"], 2) == 0)
    assert s["naccept"][2] == 0 and s["nreject"][2] == 0 and np.isinf(s["cost"][2]) and np.array_equal(s["p_trial"][2], s["p"][2])
    evaluate().step()
    t = lm.snap()
    assert all(s[k][2].tobytes() == t[k][2].tobytes() for k in STATE) and np.all(np.delete(t["naccept"], 2) == 2)


@pytest.mark.parametrize("which", ["xtol", "ftol"])
def test_state_machine_tolerances(which):
    M, truth, y = _linear()
    lm, evaluate = _linear_lm(M, y, **{which: 1e-3})
    hist = []
    for _ in range(12):
        hist.append(evaluate().step().snap())
    want = 1 if which == "xtol" else 2
    assert np.all(hist[-1]["status"] == want)
    assert np.array_equal(hist[-1]["p_trial"], hist[-1]["p"])
    done = next(i for i, h in enumerate(hist) if np.all(h["status"] == want))
    assert _same(hist[done], hist[-1])  # (later calls changed nothing)
    assert np.abs(hist[-1]["p"] - truth).max() < 0.2  # (it stopped near the solution of the noisy problem, not anywhere)
    if which == "ftol":
        c = np.stack([h["cost"] for h in hist[: done + 1]])
        assert np.all(c[1:] <= c[:-1])


def test_bounds_clamp():
    M, truth, y = _linear()
    lo, hi = np.array([-0.1, -np.inf, -0.2, 0.0]), np.array([0.1, np.inf, 0.3, 0.05])
    lm, evaluate = _linear_lm(M, y, lo=_t(lo), hi=_t(hi))
    free, free_evaluate = _linear_lm(M, y)
    for _ in range(6):
        evaluate().step()
        free_evaluate().step()
    s, f = lm.snap(), free.snap()
    assert np.all(s["p_trial"] >= lo) and np.all(s["p_trial"] <= hi) and np.all(s["p"] >= lo) and np.all(s["p"] <= hi)
    assert np.any((f["p"] < lo) | (f["p"] > hi))  # (the bounds do cut the unbounded solution off)
    assert np.any(s["p"] == lo) or np.any(s["p"] == hi)  # (a bound is met exactly, not approached)


def test_linear_problem_reaches_lstsq():
    """With the damping driven down (lam0 = 1e-17, lam_min = 0) the step from p0 = 0 is the Gauss-Newton step of a linear problem: the
    accepted result is numpy.linalg.lstsq of the problem with the prior as extra rows, relative to max |p| in the scaled variables, to
    32 npar EPS cond(scaled normal matrix) (lam = 0: the conditioning takes the place of (npar + lam) / lam).  The damping is driven
    down by the option, not by iterating: the problem is noisy, and the acceptance test compares costs, which resolve a parameter change
    near the minimum only to about sqrt(EPS); further iterations are rejected and leave the result alone.  Measured on MI355X: error / bound 2.7e-02."""
    M, truth, y = _linear()
    ncol, nrow, npar = M.shape
    rng = np.random.default_rng(3)
    prior, isp = truth + 0.1 * rng.normal(size=truth.shape), rng.uniform(0.5, 2.0, truth.shape)
    lm, evaluate = _linear_lm(M, y, prior=_t(prior), isp=_t(isp), lam0=1e-17, lam_min=0.0)
    for _ in range(2):
        evaluate().step()
    first = lm.snap()
    for _ in range(3):
        evaluate().step()
    s = lm.snap()
    assert np.all(first["naccept"] == 2) and np.all(s["status"] == 0)
    worst = 0.0
    for c in range(ncol):
        Mc = np.vstack([M[c], np.diag(isp[c])])
        yc = np.concatenate([y[c], isp[c] * prior[c]])
        ref = np.linalg.lstsq(Mc, yc, rcond=None)[0]
        As, sc = _scaled(Mc.T @ Mc)
        err = np.abs(s["p"][c] - ref) / sc / np.abs(ref / sc).max()
        worst = max(worst, err.max() / _bound(npar, cond=np.linalg.cond(As)))
    print(f"linear problem against lstsq: error / bound {worst:.3e}")
    assert worst <= 1.0


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared_base,shared_dirs,null", [(True, True, ()), (False, False, ()), (False, True, ("leaf_t",)), (True, False, ("leaf_r", "soil_r"))])
@pytest.mark.parametrize("nb,nz", [(37, 9), (300, 260)])
def test_apply_bitwise(nb, nz, shared_base, shared_dirs, null):
    import torch

    from crt1d_amd import _lib

    ncol, ntan = 5, 3
    npar = ntan + 2
    rng = np.random.default_rng(nb + 7 * len(null))
    base = {n: _t(rng.uniform(0.05, 0.5, (1 if shared_base else ncol, nb))) for n in ("leaf_r", "leaf_t", "soil_r")}
    dirs = {n: None if n in null else _t(rng.normal(size=(1 if shared_dirs else ncol, ntan, nb))) for n in base}
    lai0, p = _t(rng.uniform(0.0, 5.0, (ncol, nz))), _t(rng.normal(size=(ncol, npar)))
    out = {n: torch.full((ncol, nb), 7.0, dtype=torch.float64, device="cuda") for n in base}
    lai, scale, gp = torch.empty_like(lai0), torch.empty(ncol, dtype=torch.float64, device="cuda"), torch.empty(ncol, dtype=torch.float64, device="cuda")
    ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    ap = _lib.CrtRetrieveApply(ncol, nz, nb, npar, ntan, ntan + 1, 0 if shared_base else nb, ptr(base["leaf_r"]), ptr(base["leaf_t"]),
                               ptr(base["soil_r"]), ptr(lai0), ptr(p), ptr(out["leaf_r"]), ptr(out["leaf_t"]), ptr(out["soil_r"]), ptr(scale),
                               ptr(lai), ptr(gp))
    d = _lib.CrtOpticsDirs(ntan, 0 if shared_dirs else ntan * nb, ptr(dirs["leaf_r"]), ptr(dirs["leaf_t"]), ptr(dirs["soil_r"]))
    st = _lib.load().crt_hip_retrieve_apply_f64(ctypes.byref(ap), ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    assert st == _lib.CRT_OK
    for n in base:
        want = base[n].expand(ncol, nb)
        if dirs[n] is not None:
            want = want + p[:, 0, None] * dirs[n][:, 0] + p[:, 1, None] * dirs[n][:, 1] + p[:, 2, None] * dirs[n][:, 2]
        assert torch.equal(out[n], want), n
    assert torch.equal(lai, lai0 * scale[:, None]) and torch.equal(gp, p[:, ntan + 1])
    ref = torch.exp(p[:, ntan])
    ulp = torch.as_tensor(np.spacing(ref.cpu().numpy())).cuda()
    assert bool(((scale - ref).abs() <= 2 * ulp).all())


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npar", [1, 5, 10])
def test_covariance(npar):
    """The inverse of the stored A against numpy.linalg.inv, in the scaled variables, to 32 npar EPS cond(scaled A); a dead parameter has
    variance +inf and zero covariances, and the rest is the inverse without it."""
    import torch

    from crt1d_amd import _lib

    ncol = 7
    rng = np.random.default_rng(20 + npar)
    blocks = _random_blocks(rng, ncol, [40], npar, holes=False)
    if npar > 1:
        blocks[0]["J"][4, :, 1] = 0.0  # column 4: parameter 1 is dead
    lm = LM(_dev(blocks), _t(np.zeros((ncol, npar)))).step()
    cov = torch.full((ncol, npar, npar), 3.25, dtype=torch.float64, device="cuda")
    st = _lib.load().crt_hip_lm_covariance_f64(ncol, npar, lm.A.data_ptr(), cov.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == _lib.CRT_OK
    got, packed = cov.cpu().numpy(), lm.snap()["A"]
    il = np.tril_indices(npar)
    for c in range(ncol):
        A = np.zeros((npar, npar))
        A[il] = packed[c]
        A = A + np.tril(A, -1).T
        live = [k for k in range(npar) if A[k, k] > 0]
        assert len(live) == (npar - 1 if (c == 4 and npar > 1) else npar)
        for k in set(range(npar)) - set(live):
            assert np.isposinf(got[c, k, k]) and np.all(np.delete(got[c, k], k) == 0) and np.all(np.delete(got[c, :, k], k) == 0)
        A = A[np.ix_(live, live)]
        As, sc = _scaled(A)
        cond = np.linalg.cond(As)
        assert cond < 1e4
        ref = np.linalg.inv(A)
        g = got[c][np.ix_(live, live)]
        unscale = 1.0 / (sc[:, None] * sc[None, :])
        assert np.all(np.abs(g - ref) * unscale <= _bound(len(live), cond=cond) * np.abs(ref * unscale).max()), c


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
NSTEP = 15  # the evaluation of p0 and the 14 iterations of the host loops


def _host_loop(forward, jacobian, p, y, niter=NSTEP - 1):
    """The loop of tests/test_gpu_sensjac.py::_retrieval: gauss_newton_step, torch.where for accept / reject, x clamped to [0.2, 5]."""
    import torch

    from crt1d_amd import batched

    lam = torch.full((p.shape[0],), 1e-2, dtype=torch.float64, device="cuda")
    r = forward(p) - y
    hist = [(r * r).sum(1)]
    for _ in range(niter):
        trial = p + batched.gauss_newton_step(jacobian(p), r, damping=lam)
        trial[:, 2] = trial[:, 2].clamp(0.2, 5.0)
        rt = forward(trial) - y
        better = (rt * rt).sum(1) < hist[-1]
        p = torch.where(better[:, None], trial, p)
        r = torch.where(better[:, None], rt, r)
        lam = torch.where(better, lam / 10, lam * 10)
        hist.append((r * r).sum(1))
    return p, torch.stack(hist).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _problem(scheme="2s"):
    """The problem of tests/test_gpu_sensjac.py::_retrieval: 4 columns, 30 bands, 12 levels, the upwelling sums of 5 sensor bands at the
    top of the canopy; unknowns: one leaf-reflectance coefficient, ln(LAI scale), the ellipsoidal x in [0.2, 5]; noise-free."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nb, nz = 4, 30, 12
    d = synth.make_columns(ncol, nb, nz, seed=5)
    rng = np.random.default_rng(41)
    x_true = _t(rng.uniform(0.7, 2.0, ncol))
    dirn = _t(0.3 * d["leaf_r"].mean(axis=0) * np.sin(np.linspace(0.0, 3.0, nb)))
    truth = torch.stack((_t(rng.uniform(-0.2, 0.2, ncol)), _t(rng.uniform(-0.2, 0.2, ncol)), x_true), dim=1)
    kind = torch.full((ncol,), ELLIPSOIDAL, dtype=torch.int32, device="cuda")
    w = np.zeros((5, nb))
    for s in range(5):
        w[s, 6 * s:6 * s + 8] = np.hanning(10)[1:9][: nb - 6 * s]
    sensors = batched.SensorSet(w)
    lev, keys = (nz - 1,), ("I_df_u",)
    base_cols = batched.Columns(_t(d["psi"]), _t(d["lai"]), kind, torch.full((ncol,), 1.2, dtype=torch.float64, device="cuda"), _t(d["mla"]))
    base_bands = batched.Bands(_t(d["I_dr0"]), _t(d["I_df0"]), _t(d["leaf_r"]), _t(d["leaf_t"]), _t(d["soil_r"]))

    def inputs(p):
        cols = batched.Columns(base_cols.psi, base_cols.lai * torch.exp(p[:, 1])[:, None], kind, p[:, 2].contiguous(), base_cols.mla)
        bands = batched.Bands(base_bands.I_dr0, base_bands.I_df0, base_bands.leaf_r + p[:, 0, None] * dirn, base_bands.leaf_t, base_bands.soil_r)
        return cols, bands

    def forward(p):
        return batched.solve_sensor_levels(scheme, *inputs(p), lev, sensors, keys=keys)["I_df_u"][:, 0].clone()  # (ncol, 5)

    def jacobian(p):
        cols, bands = inputs(p)
        return batched.sensor_jacobian(scheme, cols, bands, lev, sensors, d_leaf_r=dirn[None], tangent=batched.leaf_tangent(cols, "param"),
                                       keys=keys)["I_df_u"][:, 0]  # (ncol, 5, 3)

    y = forward(truth)
    p0 = torch.stack((torch.zeros(ncol, dtype=torch.float64, device="cuda"),) * 2 + (torch.full((ncol,), 1.2, dtype=torch.float64, device="cuda"),), dim=1)
    p_host, hist = _host_loop(forward, jacobian, p0, y)
    torch.cuda.synchronize()
    return dict(cols=base_cols, bands=base_bands, dirn=dirn, truth=truth, sensors=sensors, lev=lev, keys=keys, y=y, p0=p0,
                host_error=float((p_host - truth).abs().max()), host_hist=hist)


def _plan(P, scheme="2s", cols=slice(None), **kw):
    from crt1d_amd import batched

    lo, hi = np.array([-np.inf, -np.inf, 0.2]), np.array([np.inf, np.inf, 5.0])
    c, b = P["cols"], P["bands"]
    if cols != slice(None):
        c, b = c.slice(cols.start, cols.stop), b.slice(cols.start, cols.stop)
    sun = kw.pop("sun", None)
    if sun is not None and cols != slice(None):
        sun = sun.slice(cols.start, cols.stop)
    return batched.RetrievalPlan(scheme, c, b, P["lev"], P["sensors"], {"I_df_u": P["y_plan"][cols] if "y_plan" in P else P["y"][cols, None]},
                                 keys=P["keys"], sun=sun, d_leaf_r=P["dirn"][None], lai=True, leaf=True, p0=P["p0"][cols], lo=lo, hi=hi,
                                 lam0=1e-2, lam_up=10.0, lam_down=0.1, xtol=0.0, ftol=0.0, **kw)


def _plan_state(plan):
    import torch

    torch.cuda.synchronize()
    return {k: getattr(plan, k).cpu().numpy().copy() for k in STATE}


def _run_and_check(P, plan, label):
    """15 single steps: the cost never increases, ends below 1e-12 of the first, and the parameter error is at most 10 x the host
    loop's.  -> the final state"""
    costs = []
    for _ in range(NSTEP):
        costs.append(plan.step().cost.clone())
    state = _plan_state(plan)
    costs = np.stack([c.cpu().numpy() for c in costs])
    err = float(np.abs(state["p"] - P["truth"].cpu().numpy()).max())
    print(f"{label}: parameter error plan {err:.3e}, host loop {P['host_error']:.3e}; cost {costs[0].max():.3e} -> {costs[-1].max():.3e} "
          f"(host loop misfit {P['host_hist'][0].max():.3e} -> {P['host_hist'][-1].max():.3e}); accepted {state['naccept']}, rejected {state['nreject']}")
    assert np.all(costs[1:] <= costs[:-1])
    assert costs[-1].max() < 1e-12 * costs[0].max()
    assert err <= 10 * P["host_error"], (err, P["host_error"])
    return state


def test_retrieval_2s():
    """Measured on MI355X after 15 steps, largest parameter error: plan 1.6e-13, host loop 1.4e-13; largest column cost
    2.9e-01 -> 9.8e-29 (host loop misfit 5.8e-01 -> 7.0e-29).  plan.run(15) after reset() gives the bits of the 15 single steps; columns 0-1 alone the bits they have in the batch."""
    P = _problem()
    plan = _plan(P)
    state = _run_and_check(P, plan, "retrieval 2s")
    assert np.all(state["status"] == 0)
    again = _plan_state(plan.reset().run(NSTEP))
    assert _same(state, again)
    two = _plan_state(_plan(P, cols=slice(0, 2)).run(NSTEP))
    assert all(two[k].tobytes() == state[k][:2].tobytes() for k in STATE)
    res = plan.result()
    assert res["params"] == ("dir0", "lai", "leaf") and np.array_equal(res["p"].cpu().numpy(), state["p"])
    cov = plan.covariance().cpu().numpy()
    assert cov.shape == (4, 3, 3) and np.all(np.isfinite(cov)) and np.all(np.diagonal(cov, axis1=1, axis2=2) > 0)


# ---- 7. ---------------------------------------------------------------------------------------------------------------------------------
ZENITHS = np.deg2rad([22.0, 45.0, 64.0])


@functools.lru_cache(maxsize=None)
def _series_problem():
    """The problem of tests/test_gpu_sensjac_series.py::_retrieval: 2s, 4 columns, 30 bands (15 visible, 15 near-infrared), 12 levels;
    the upwelling sums of two boxcar sensor bands at the top of the canopy at three sun zeniths; the same three unknowns."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nb, nz, nt = 4, 30, 12, len(ZENITHS)
    d = synth.make_columns(ncol, nb, nz, seed=5)
    rng = np.random.default_rng(41)
    vis = np.arange(nb) < nb // 2
    leaf_r = np.where(vis, 0.08, 0.45) * rng.uniform(0.9, 1.1, (ncol, nb))
    leaf_t = np.where(vis, 0.06, 0.42) * rng.uniform(0.9, 1.1, (ncol, nb))
    soil_r = np.where(vis, 0.10, 0.25) * rng.uniform(0.9, 1.1, (ncol, nb))
    lai = np.linspace(1.0, 0.0, nz)[None, :] * rng.uniform(1.5, 3.0, ncol)[:, None]
    dirn = _t(0.3 * leaf_r.mean(axis=0))
    truth = torch.stack((_t(rng.uniform(-0.2, 0.2, ncol)), _t(rng.uniform(-0.15, 0.15, ncol)), _t(rng.uniform(0.8, 1.6, ncol))), dim=1)
    kind = torch.full((ncol,), ELLIPSOIDAL, dtype=torch.int32, device="cuda")
    psi = ZENITHS[None, :] + np.deg2rad(rng.uniform(-2.0, 2.0, (ncol, 1)))
    I_dr0 = d["I_dr0"][:, None, :] * np.cos(psi)[:, :, None]
    I_df0 = np.repeat(d["I_df0"][:, None, :], nt, axis=1)
    sun = batched.SunSeries(_t(psi), _t(I_dr0), _t(I_df0))
    w = np.zeros((2, nb))
    w[0, 2:13], w[1, 17:28] = 1.0, 1.0
    sensors = batched.SensorSet(w)
    lev, keys = (nz - 1,), ("I_df_u",)
    x0 = torch.full((ncol,), 1.2, dtype=torch.float64, device="cuda")
    base_cols = batched.Columns(sun.psi[:, 0].contiguous(), _t(lai), kind, x0, _t(d["mla"]))
    base_bands = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), _t(leaf_r), _t(leaf_t), _t(soil_r))

    def inputs(p):
        cols = batched.Columns(base_cols.psi, base_cols.lai * torch.exp(p[:, 1])[:, None], kind, p[:, 2].contiguous(), base_cols.mla)
        bands = batched.Bands(base_bands.I_dr0, base_bands.I_df0, base_bands.leaf_r + p[:, 0, None] * dirn, base_bands.leaf_t, base_bands.soil_r)
        return cols, bands

    def forward(p):  # (ncol, nt * 2)
        cols, bands = inputs(p)
        return batched.solve_sensor_levels_series("2s", cols, bands, sun, lev, sensors, keys=keys)["I_df_u"].reshape(ncol, nt * 2).clone()

    def jacobian(p):  # (ncol, nt * 2, 3)
        cols, bands = inputs(p)
        J = batched.sensor_jacobian_series("2s", cols, bands, sun, lev, sensors, d_leaf_r=dirn[None],
                                           tangent=batched.leaf_tangent_series(cols, sun, "param"), keys=keys)["I_df_u"]
        return J.reshape(ncol, nt * 2, 3)

    y = forward(truth)
    zero = torch.zeros(ncol, dtype=torch.float64, device="cuda")
    p0 = torch.stack((zero, zero, x0), dim=1)
    p_host, hist = _host_loop(forward, jacobian, p0, y)
    torch.cuda.synchronize()
    return dict(cols=base_cols, bands=base_bands, dirn=dirn, truth=truth, sensors=sensors, lev=lev, keys=keys, y=y, p0=p0, sun=sun,
                y_plan=y.reshape(ncol, nt, 1, 2), host_error=float((p_host - truth).abs().max()), host_hist=hist)


def test_retrieval_series():
    """The same three assertions with sun= a three-state SunSeries, against the host loop on sensor_jacobian_series.  Measured on MI355X
    after 15 steps, largest parameter error: plan 1.1e-14, host loop 8.0e-15; largest column cost 7.8e+00 -> 5.1e-29."""
    P = _series_problem()
    plan = _plan(P, sun=P["sun"])
    state = _run_and_check(P, plan, "retrieval 2s series")
    two = _plan_state(_plan(P, cols=slice(0, 2), sun=P["sun"]).run(NSTEP))
    assert all(two[k].tobytes() == state[k][:2].tobytes() for k in STATE)


# ---- 8. ---------------------------------------------------------------------------------------------------------------------------------
def test_retrieval_composed_n79():
    """n79 through the composed SensorJacPlan, the same small shape: the cost is monotone and the final parameter error within 10 x the
    host loop's.  Measured on MI355X: plan 3.0e-14, host loop 3.2e-14."""
    P = _problem("n79")
    _run_and_check(P, _plan(P, scheme="n79"), "retrieval n79")


# ---- 9. ---------------------------------------------------------------------------------------------------------------------------------
def test_model_retrieve():
    """Model.retrieve is the batched call on the model's own column: bitwise; with psi it runs over a sun-angle series."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=12)
    nb = m.nwl
    w = np.zeros((3, nb))
    w[0, : nb // 2], w[1, nb // 3:], w[2, nb // 2] = 1.0, 0.5, 2.0
    d = np.random.default_rng(3).uniform(-0.05, 0.05, (1, nb)) * m.copy_p()["leaf_r"]
    y = {"I_df_u": 1.03 * m.run_sensors(w, levels=(-1,))["I_df_u"]}
    got = m.retrieve(w, y, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, lo=np.array([-1.0, -1.0]), hi=np.array([1.0, 1.0]))
    assert got["params"] == ("dir0", "lai") and got["p"].shape == (2,) and got["cov"].shape == (2, 2)
    scheme, cols, b, sun = m._series_inputs(np.atleast_1d(float(m._p["psi"])), None, None, "retrieval")
    cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
    b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
    ref = batched.retrieve("2s", cols, b, (-1,), batched.SensorSet(w), {"I_df_u": y["I_df_u"][None]}, keys=("I_df_u",), niter=8, d_leaf_r=d,
                           lai=True, lo=np.array([-1.0, -1.0]), hi=np.array([1.0, 1.0]))
    torch.cuda.synchronize()
    for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
        assert got[k].tobytes() == ref[k][0].cpu().numpy().tobytes(), k
    assert got["cost"] < 0.5 * 0.5 * float(((0.03 / 1.03 * y["I_df_u"]) ** 2).sum())  # (it did lower the cost of the starting point)
    psi = np.deg2rad([10.0, 40.0, 70.0])
    ys = {"I_df_u": 1.03 * m.run_series_sensors(psi, w, levels=(-1,))["I_df_u"]}
    gs = m.retrieve(w, ys, levels=(-1,), directions={"leaf_r": d}, lai=True, psi=psi, niter=8)
    scheme, cols, b, sun = m._series_inputs(psi, None, None, "retrieval")
    rs = batched.retrieve("2s", cols, b, (-1,), batched.SensorSet(w), {"I_df_u": ys["I_df_u"][None]}, keys=("I_df_u",), niter=8, sun=sun,
                          d_leaf_r=d, lai=True)
    torch.cuda.synchronize()
    for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
        assert gs[k].tobytes() == rs[k][0].cpu().numpy().tobytes(), k
    with pytest.raises(ValueError, match="wrt_leaf must be None or 'param'"):
        m.retrieve(w, y, levels=(-1,), wrt_leaf="mla")
