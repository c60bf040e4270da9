"""GPU: the Levenberg-Marquardt step on a chain of coupled dates (include_chain/crt1d_hip_lm_chain.h) through its C entries.

1. Sums from rows: k_lm_normal + crt_hip_lm_step_normal_f64 equals crt_hip_lm_step_f64, every state array byte for byte, three steps.
2. Degenerate chains: nd = 1 equals k_lm_step_normal byte for byte; all-zero weights decouple the dates; a pixel alone equals the pixel
   in a batch of 70; a pixel that is not running is not touched.
3. Decisions: a scripted sequence of supplied sums against the fp64 restatement of tests/lm_chain_reference.py.
4. The solve against the long-double dense solution, within a bound derived below; the cost within 2 m u cost.
5. The covariance against the long-double dense inverse, a date without any observation included; the largest nd at npar = 10.

THE BOUNDS (u = 2^-53, n = nd npar, M the scaled damped matrix, x its solution, s the scales).
 solve: the Cholesky solve is backward stable: (M + dM) x^ = b with ||dM||_2 <= 4 n (3 n + 1) u ||M||_2 (Higham, Accuracy and Stability,
   Thm 10.4 with the norm bound of 10.6), hence ||x^ - x||_2 <= 4 n (3 n + 1) u kappa_2(M) ||x||_2.  Forming M costs at most 8 roundings
   an entry (two squares, two sums, two scalings, the damping, the sign): componentwise 8 u |M|, in norm <= 8 n u ||M||_2, the same kind of
   term.  Forming b = -G s costs 6 roundings on the three terms of G: |db_r| <= 6 u (|g| + |w_l e_l| + |w_r e_r|) s_r =: beta_r, which
   moves x by at most ||beta||_2 / lambda_min(M).  delta = x s and p + delta add u |delta| and u |p_trial|.  So per entry
       |got - ref|_r <= s_r ((4 n (3 n + 1) + 8 n) u kappa_2 ||x||_2 + ||beta||_2 / lambda_min) + u (|delta_r| + |p_trial_r|).
 covariance: the same backward error of the factor moves M^-1 by at most c u kappa_2 ||M^-1||_2, c = 4 n (3 n + 1) + 8 n: that part is
   derived.  The recursion S_d = W^T W + C^T S_{d+1} C adds, per date, three triangular or full npar x npar products whose sums have
   at most 2 npar terms: each computed entry is off by at most gamma_{2 npar} times a product of norms of W, C and S, which are bounded
   by ||L^-1||^2 <= ||M^-1|| and ||C|| <= kappa_2^(1/2), and the error of S_{d+1} is carried on through a contraction (C^T S C <= S_d).
   Summed over the nd dates that is at most nd * 3 * 2 npar u kappa_2 ||M^-1||_2 = 6 n u kappa_2 ||M^-1||_2 to first order, far below c.
   The bound asserted is 2 c u kappa_2 ||M^-1||_2 s_r s_q: the second c is an ALLOWANCE that covers this 6 n term with a wide
   margin, not a sharp derivation of it.
 Measured on MI355X, largest error / bound: see DESIGN.md 3.28."""
import ctypes

import numpy as np
import pytest

import lm_chain_reference as R
from test_gpu_retrieve import LM, STATE, _dev, _random_blocks, _same, _t

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OPTS = dict(lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0)
PER_PIX = ("cost", "lam", "status", "naccept", "nreject")


def _ptr(v):
    return None if v is None else v.data_ptr()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Sums:
    """crt_hip_lm_normal_f64 on the blocks of LM: one crt_lm_normal_block per observation block (or one over all of them)."""

    def __init__(self, blocks, npar, together=False):
        import torch

        from crt1d_amd import _lib

        self.lib = _lib.load()
        ncol = blocks[0]["J"].shape[0]
        groups = [blocks] if together else [[b] for b in blocks]
        f64 = dict(dtype=torch.float64, device="cuda")
        self.out = []
        for grp in groups:
            A, g, c2 = torch.full((ncol, npar * (npar + 1) // 2), np.nan, **f64), torch.full((ncol, npar), np.nan, **f64), torch.full((ncol,), np.nan, **f64)
            obs = (_lib.CrtLmObs * len(grp))(*[_lib.CrtLmObs(b["J"].shape[1], _ptr(b["f"]), _ptr(b["J"]), _ptr(b["y"]), _ptr(b["s"])) for b in grp])
            st = self.lib.crt_hip_lm_normal_f64(ncol, npar, obs, len(grp), _ptr(A), _ptr(g), _ptr(c2), _stream())
            assert st == _lib.CRT_OK, st
            self.out.append((A, g, c2))


class Chain:
    """The chain entries on tensors of the test's own.  sums: [(A, g, c2)] of CUDA tensors per column; nd = None: crt_hip_lm_step_normal_f64."""

    def __init__(self, npix, nd, p0, w=None, lam0=1e-2, prior=None, isp=None, lo=None, hi=None, **opts):
        import torch

        from crt1d_amd import _lib

        self.lib = _lib.load()
        self.chained = nd is not None
        nd = nd or 1
        ncol, npar = p0.shape
        assert ncol == npix * nd
        self.npix, self.nd, self.npar = npix, nd, npar
        f64 = dict(dtype=torch.float64, device="cuda")
        i32 = dict(dtype=torch.int32, device="cuda")
        self.p, self.p_trial = p0.clone(), p0.clone()
        self.cost, self.lam = torch.full((npix,), float("inf"), **f64), torch.full((npix,), lam0, **f64)
        self.A, self.g = torch.zeros((ncol, npar * (npar + 1) // 2), **f64), torch.zeros((ncol, npar), **f64)
        self.status, self.naccept, self.nreject = (torch.zeros((npix,), **i32) for _ in range(3))
        self.cov = torch.full((ncol, npar, npar), np.nan, **f64)
        o = dict(OPTS)
        o.update(opts)
        self.opt = o
        self._keep = (prior, isp, lo, hi, w)
        self._prob = _lib.CrtLmProblem(ncol, npar, o["lam_up"], o["lam_down"], o["lam_min"], o["lam_max"], o["xtol"], o["ftol"], _ptr(lo), _ptr(hi),
                                       _ptr(prior), _ptr(isp))
        self._state = _lib.CrtLmState(*[_ptr(getattr(self, k)) for k in STATE])
        stride = 0 if w is None or w.ndim == 2 else (nd - 1) * npar
        self._chain = _lib.CrtLmChain(npix, nd, stride, _ptr(w))

    def step(self, sums, expect=0):
        from crt1d_amd import _lib

        blk = (_lib.CrtLmNormalBlock * len(sums))(*[_lib.CrtLmNormalBlock(*[_ptr(v) for v in s]) for s in sums])
        if self.chained:
            st = self.lib.crt_hip_lm_step_chain_f64(ctypes.byref(self._chain), ctypes.byref(self._prob), blk, len(sums), ctypes.byref(self._state),
                                                    _stream())
        else:
            st = self.lib.crt_hip_lm_step_normal_f64(ctypes.byref(self._prob), blk, len(sums), ctypes.byref(self._state), _stream())
        assert st == expect, st
        return self

    def covariance(self, expect=0):
        st = self.lib.crt_hip_lm_chain_covariance_f64(ctypes.byref(self._chain), self.npar, _ptr(self.A), _ptr(self.cov), _stream())
        assert st == expect, st
        import torch

        torch.cuda.synchronize()
        return self.cov.cpu().numpy().reshape(self.npix, self.nd, self.npar, self.npar)

    def snap(self):
        import torch

        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in STATE}


def _split(n, nblk):
    return [n] if nblk == 1 else [n - 2 * (n // 3), n // 3, n // 3]


def _extras(rng, ncol, npar):
    prior, isp = rng.normal(size=(ncol, npar)), rng.uniform(0.5, 2.0, (ncol, npar))
    isp[:, npar // 2] = 0.0
    prior[:, npar // 2] = np.nan
    return dict(prior=_t(prior), isp=_t(isp), lo=_t(np.full(npar, -0.7)), hi=_t(np.full(npar, 0.9)))


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("nrow", [3, 65, 200])
def test_sums_from_rows_bitwise(nrow, npar, nblk):
    """Masked rows (NaN under inv_sigma = 0), a prior with one unobserved row, bounds: three steps of k_lm_step against k_lm_normal (one
    block over all the rows, as k_lm_step sums them) + k_lm_step_normal."""
    ncol = 70
    rng = np.random.default_rng(5000 + 100 * nrow + 10 * npar + nblk)
    blocks = _dev(_random_blocks(rng, ncol, _split(nrow, nblk), npar))
    p0, ex = _t(0.1 * rng.normal(size=(ncol, npar))), _extras(rng, ncol, npar)
    a = LM(blocks, p0, **ex)
    b = Chain(ncol, None, p0, **ex)
    for it in range(3):
        a.step()
        b.step(Sums(blocks, npar, together=True).out)
        assert _same(a.snap(), b.snap()), it
    assert a.snap()["naccept"].min() >= 1


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("npix", [1, 3, 70])
def test_single_date_is_step_normal_bitwise(npix, npar, nblk):
    rng = np.random.default_rng(6000 + 100 * npix + 10 * npar + nblk)
    blocks = _dev(_random_blocks(rng, npix, _split(40, nblk), npar))
    sums = Sums(blocks, npar).out
    p0, ex = _t(0.1 * rng.normal(size=(npix, npar))), _extras(rng, npix, npar)
    a, b = Chain(npix, None, p0, **ex), Chain(npix, 1, p0, **ex)
    for it in range(3):
        assert _same(a.step(sums).snap(), b.step(sums).snap()), it


def _linear_case(rng, npix, nd, npar, empty=None, nblk=1, scale=1.0):
    """A linear twin: per column J (3 npar, npar) and y; the sums at p are A = J^T J, g = J^T r, c2 = r^T r (fp64 NumPy), split over nblk
    blocks of rows.  empty: a date index without any observation (all three sums +0); scale: of J.  -> sums_at(p) on the host"""
    ncol, nrow = npix * nd, 3 * npar
    J = rng.normal(size=(ncol, nrow, npar)) * rng.uniform(0.5, 2.0, npar) * scale
    y = rng.normal(size=(ncol, nrow))
    if empty is not None:
        J.reshape(npix, nd, nrow, npar)[:, empty] = 0.0
        y.reshape(npix, nd, nrow)[:, empty] = 0.0
    cuts = np.array_split(np.arange(nrow), nblk)

    def sums_at(p):
        out = []
        for rows in cuts:
            Jb = J[:, rows]
            r = np.einsum("cok,ck->co", Jb, p) - y[:, rows]
            out.append((R.pack(np.einsum("coi,coj->cij", Jb, Jb)), np.einsum("coi,co->ci", Jb, r), np.einsum("co,co->c", r, r)))
        return out

    return sums_at


def _dev_sums(sums):
    return [tuple(_t(v) for v in s) for s in sums]


@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("nd", [2, 3, 7])
def test_zero_weights_decouple(nd, npar):
    """All weights 0, the first call: p_trial of every column is bitwise k_lm_step_normal's for that column, cost[pix] the left-to-right
    sum over the dates of that kernel's cost.  3 blocks, a prior, bounds."""
    npix = 3
    rng = np.random.default_rng(7000 + 10 * nd + npar)
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    sums = _dev_sums(_linear_case(rng, npix, nd, npar, nblk=3)(p0))
    ex = _extras(rng, npix * nd, npar)
    a = Chain(npix * nd, None, _t(p0), **ex).step(sums).snap()
    b = Chain(npix, nd, _t(p0), w=_t(np.zeros((nd - 1, npar))), **ex).step(sums).snap()
    assert a["p_trial"].tobytes() == b["p_trial"].tobytes() and a["A"].tobytes() == b["A"].tobytes() and a["g"].tobytes() == b["g"].tobytes()
    want = a["cost"].reshape(npix, nd)[:, 0].copy()
    for d in range(1, nd):
        want = want + a["cost"].reshape(npix, nd)[:, d]
    assert want.tobytes() == b["cost"].tobytes() and np.all(b["naccept"] == 1) and np.all(b["status"] == 0)


@pytest.mark.parametrize("shared", [True, False])
def test_pixel_alone_equals_pixel_in_batch_and_stopped_pixels_keep_their_bits(shared):
    import torch

    npix, nd, npar, pix = 70, 3, 5, 37
    rng = np.random.default_rng(7100 + shared)
    w = rng.uniform(0.5, 2.0, (nd - 1, npar) if shared else (npix, nd - 1, npar))
    w1 = w if shared else w[pix:pix + 1]
    sums_at = _linear_case(rng, npix, nd, npar, nblk=3)
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    ex = _extras(rng, npix * nd, npar)
    cols = slice(pix * nd, (pix + 1) * nd)
    one = {k: (v[cols] if v.shape[0] == npix * nd else v) for k, v in ex.items()}
    big, small = Chain(npix, nd, _t(p0), w=_t(w), **ex), Chain(1, nd, _t(p0[cols]), w=_t(w1), **one)
    stopped = [5, 64]
    big.status[stopped] = R.CONVERGED_X
    before = big.snap()
    for it in range(3):
        sb = sums_at(big.snap()["p_trial"])
        for s in sb:
            for v in s:
                v.reshape(npix, nd, -1)[stopped] = np.nan  # what a stopped pixel would read
        ss = [tuple(v[cols] for v in s) for s in sb]
        np.testing.assert_array_equal(big.snap()["p_trial"][cols], small.snap()["p_trial"])
        big.step(_dev_sums(sb))
        small.step(_dev_sums(ss))
        a, b = big.snap(), small.snap()
        for k in STATE:
            n = nd if k in ("p", "p_trial", "A", "g") else 1
            assert a[k][pix * n:(pix + 1) * n].tobytes() == b[k].tobytes(), (it, k)
            for q in stopped:
                assert a[k][q * n:(q + 1) * n].tobytes() == before[k][q * n:(q + 1) * n].tobytes(), (it, k, q)
    assert a["naccept"][pix] >= 2
    torch.cuda.synchronize()


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def _run_script(rng, script, nd=3, npar=2, npix=3, nsteps=6, **opts):
    """Steps of the kernel and of the fp64 restatement on the same supplied sums.  script(it, pix, sums) may spoil the sums of a step.
    After every step the decisions are equal and p_trial has the restatement's bits.  -> the snapshots"""
    w = rng.uniform(0.5, 2.0, (npix, nd - 1, npar))
    sums_at = _linear_case(rng, npix, nd, npar)
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    lo, hi = np.full(npar, -5.0), np.full(npar, 5.0)
    ch = Chain(npix, nd, _t(p0), w=_t(w), lo=_t(lo), hi=_t(hi), **opts)
    ref = [R.new_state(p0.reshape(npix, nd, npar)[i], 1e-2) for i in range(npix)]
    history = []
    for it in range(nsteps):
        (A, g, c2), = sums_at(ch.snap()["p_trial"])
        A, g, c2 = A.reshape(npix, nd, -1), g.reshape(npix, nd, -1), c2.reshape(npix, nd)
        for i in range(npix):
            script(it, i, (A[i], g[i], c2[i]))
        ch.step(_dev_sums([(A.reshape(npix * nd, -1), g.reshape(npix * nd, -1), c2.reshape(-1))]))
        got = ch.snap()
        for i in range(npix):
            ref[i] = R.step(ref[i], [(A[i], g[i], c2[i])], w[i], ch.opt, lo, hi)
            for k in PER_PIX:
                assert got[k][i] == ref[i][k] or (k == "cost" and np.isnan(got[k][i]) and np.isnan(ref[i][k])), (it, i, k, got[k][i], ref[i][k])
            for k in ("p", "p_trial", "A", "g"):
                have = got[k].reshape(npix, nd, -1)[i]
                assert have.tobytes() == ref[i][k].tobytes(), (it, i, k)
        history.append(got)
    return history


def test_decisions_accept_reject_failed_start():
    """Step 0 accepted everywhere but pixel 1, whose date 1 is NaN: FAILED_START, no counter moves.  Step 1: pixel 0 is shown a cost 100
    times too large: rejected, lam up, p, cost, A and g kept; pixel 2 is accepted.  Step 2: pixel 0 is accepted again."""
    def script(it, pix, s):
        if pix == 1 and it == 0:
            s[2][1] = np.nan
        if pix == 0 and it == 1:
            s[2][:] *= 100.0

    h = _run_script(np.random.default_rng(81), script, nsteps=3)
    assert list(h[0]["status"]) == [0, R.FAILED_START, 0] and list(h[0]["naccept"]) == [1, 0, 1] and list(h[0]["nreject"]) == [0, 0, 0]
    assert list(h[1]["status"]) == [0, R.FAILED_START, 0] and list(h[1]["naccept"]) == [1, 0, 2] and list(h[1]["nreject"]) == [1, 0, 0]
    assert h[1]["lam"][0] == h[0]["lam"][0] * 10.0 and h[1]["lam"][2] == h[0]["lam"][2] * 0.1 and h[1]["lam"][1] == 1e-2
    assert h[1]["cost"][0] == h[0]["cost"][0] and h[1]["A"][:3].tobytes() == h[0]["A"][:3].tobytes() and np.array_equal(h[1]["p"][:3], h[0]["p"][:3])
    assert not np.array_equal(h[1]["p_trial"][:3], h[0]["p_trial"][:3])  # (a shorter step from the same point)
    assert h[2]["naccept"][0] == 2 and np.isinf(h[2]["cost"][1])


def test_decisions_stalled():
    def script(it, pix, s):
        if it >= 1:
            s[2][:] = 1e30  # never accepted again

    h = _run_script(np.random.default_rng(82), script, nsteps=4, lam_max=0.05)
    assert list(h[1]["status"]) == [0, 0, 0] and list(h[2]["status"]) == [R.STALLED] * 3 and list(h[3]["nreject"]) == [2, 2, 2]
    assert np.array_equal(h[3]["p"], h[3]["p_trial"])


def test_decisions_converged_f():
    h = _run_script(np.random.default_rng(83), lambda *a: None, nsteps=6, ftol=1e-3)
    assert list(h[-1]["status"]) == [R.CONVERGED_F] * 3 and list(h[0]["status"]) == [0, 0, 0] and np.array_equal(h[-1]["p"], h[-1]["p_trial"])


def test_decisions_converged_x():
    h = _run_script(np.random.default_rng(84), lambda *a: None, nsteps=6, xtol=1e-4)
    assert list(h[-1]["status"]) == [R.CONVERGED_X] * 3 and list(h[0]["status"]) == [0, 0, 0] and np.array_equal(h[-1]["p"], h[-1]["p_trial"])


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def _solve_bound(A, g, p, w, lam, delta, p_trial):
    nd, npar = g.shape
    n = nd * npar
    M, x, s = R.dense_ld(A, g, p, w, lam)
    lo, hi = R.scaled_extremes(A, w, lam)
    sol = np.asarray(delta, dtype=np.longdouble).reshape(-1) / s
    beta = np.zeros(n)
    for d in range(nd):
        for k in range(npar):
            t = abs(g[d, k])
            if d > 0:
                t += abs(w[d - 1, k] ** 2 * (p[d, k] - p[d - 1, k]))
            if d < nd - 1:
                t += abs(w[d, k] ** 2 * (p[d + 1, k] - p[d, k]))
            beta[d * npar + k] = 6 * U * t * float(s[d * npar + k])
    scaled = (4 * n * (3 * n + 1) + 8 * n) * U * (hi / lo) * float(np.linalg.norm(sol.astype(np.float64))) + np.linalg.norm(beta) / lo
    return np.asarray(s, dtype=np.float64).reshape(nd, npar) * scaled + U * (np.abs(np.asarray(delta, dtype=np.float64)) + np.abs(p_trial))


@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("nd", [1, 2, 3, 7])
def test_solve_against_long_double_dense(nd, npar, lam):
    assert _solve_fraction(nd, npar, lam) <= 1.0


def _solve_fraction(nd, npar, lam):
    """The case of the test: every assertion but the last.  -> the largest error / bound"""
    npix = 3
    rng = np.random.default_rng(9000 + 100 * nd + 10 * npar + (lam > 0))
    shared = (nd + npar) % 2 == 0
    w = rng.uniform(0.5, 2.0, (nd - 1, npar) if shared else (npix, nd - 1, npar))
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    sums = _linear_case(rng, npix, nd, npar)(p0)
    A, g, c2 = (v.reshape(npix, nd, *v.shape[1:]) for v in sums[0])
    P = p0.reshape(npix, nd, npar)
    wp = lambda i: w if shared else w[i]  # noqa: E731
    refs = [R.solve_ld(A[i], g[i], P[i], wp(i), lam) for i in range(npix)]
    got = Chain(npix, nd, _t(p0), w=_t(w) if nd > 1 else None, lam0=lam, lam_down=1.0, lam_min=0.0).step(_dev_sums(sums)).snap()
    assert np.array_equal(got["p"], p0) and np.all(got["naccept"] == 1) and np.all(got["lam"] == lam)
    worst = 0.0
    for i in range(npix):
        pt = got["p_trial"].reshape(npix, nd, npar)[i]
        bound = _solve_bound(A[i], g[i], P[i], wp(i), lam, refs[i], pt)
        assert bound.max() < 1e-6, bound.max()  # (of the inputs: the bound means something)
        err = np.abs(pt.astype(np.longdouble) - P[i].astype(np.longdouble) - refs[i]).astype(np.float64)
        worst = max(worst, float((err / bound).max()))
        m = nd + (nd - 1) * npar
        want = R.cost_ld(c2[i], P[i], wp(i) if nd > 1 else np.zeros((0, npar)))
        assert abs(np.longdouble(got["cost"][i]) - want) <= 2 * m * U * want
        fp = R.band_solve(A[i], g[i], P[i], wp(i), lam)  # the fp64 restatement gives the kernel's bits
        assert (P[i] + fp).tobytes() == pt.tobytes()
    return worst


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("nd", [1, 2, 3, 7])
def test_covariance_against_long_double_inverse(nd, npar):
    """The diagonal blocks against the long-double dense inverse; npar = 10 has 100 entries a block, more than the 64 lanes, so the
    entry loops of the recursion take a second trip.  Shared weights where nd + npar is even, per-pixel ones otherwise.
    Date 1 of every pixel (nd >= 3) has no observation at all: A = 0 there, its variance comes from the neighbours through the
    coupling and exceeds theirs (asserted on the reference first).  The observed dates are well observed (J scaled by 4: a data
    precision of order 16 x 3 npar against coupling weights^2 <= 4), which is what makes the gap the least certain date."""
    assert _covariance_fraction(nd, npar) <= 1.0


def _covariance_fraction(nd, npar):
    """The case of the test: every assertion but the last.  -> the largest error / bound"""
    npix = 3
    rng = np.random.default_rng(9500 + 10 * nd + npar)
    empty = 1 if nd >= 3 else None
    shared = (nd + npar) % 2 == 0
    w = rng.uniform(0.5, 2.0, (nd - 1, npar) if shared else (npix, nd - 1, npar))
    wp = lambda i: w if shared else w[i]  # noqa: E731
    p0 = np.zeros((npix * nd, npar))
    sums = _linear_case(rng, npix, nd, npar, empty=empty, scale=4.0)(p0)
    A = sums[0][0].reshape(npix, nd, -1)
    ch = Chain(npix, nd, _t(p0), w=_t(w) if nd > 1 else None).step(_dev_sums(sums))
    cov = ch.covariance()
    n, worst = nd * npar, 0.0
    for i in range(npix):
        X = R.inverse_ld(A[i], wp(i))
        lo, hi = R.scaled_extremes(A[i], wp(i), 0.0)
        _, _, s = R.dense_ld(A[i], np.zeros((nd, npar)), np.zeros((nd, npar)), wp(i), 0.0)
        s = s.astype(np.float64)
        for d in range(nd):
            ref = X[d * npar:(d + 1) * npar, d * npar:(d + 1) * npar]
            sd = s[d * npar:(d + 1) * npar]
            bound = 2 * (4 * n * (3 * n + 1) + 8 * n) * U * (hi / lo) / lo * sd[:, None] * sd[None, :]
            assert bound.max() < 1e-6
            err = np.abs(cov[i, d].astype(np.longdouble) - ref).astype(np.float64)
            worst = max(worst, float((err / bound).max()))
            assert np.array_equal(cov[i, d], cov[i, d].T)
        if empty is not None:
            var = np.diagonal(X).astype(np.float64).reshape(nd, npar)
            assert np.all(var[1] > var[0]) and np.all(var[1] > var[2])  # the reference, on the CPU
            got = np.diagonal(cov[i], axis1=1, axis2=2)
            assert np.all(got[1] > got[0]) and np.all(got[1] > got[2])
    return worst


def test_dead_entry_in_the_chain():
    """A parameter without data or coupling on one date: delta = 0 there, variance +inf, zero covariances; the others are unaffected."""
    npix, nd, npar = 1, 3, 2
    rng = np.random.default_rng(9600)
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    w[:, 1] = 0.0
    J = rng.normal(size=(nd, 6, npar))
    J[1, :, 1] = 0.0
    r = rng.normal(size=(nd, 6))
    sums = [(R.pack(np.einsum("coi,coj->cij", J, J)), np.einsum("coi,co->ci", J, r), np.einsum("co,co->c", r, r))]
    ch = Chain(npix, nd, _t(np.zeros((nd, npar))), w=_t(w)).step(_dev_sums(sums))
    got, cov = ch.snap(), ch.covariance()[0]
    assert got["p_trial"][1, 1] == 0.0 and np.all(got["p_trial"][[0, 2], 1] != 0.0) and np.all(np.isfinite(got["p_trial"]))
    assert cov[1, 1, 1] == np.inf and cov[1, 0, 1] == 0.0 and cov[1, 1, 0] == 0.0 and np.all(np.isfinite(cov[[0, 2]])) and np.isfinite(cov[1, 0, 0])


def test_largest_nd_at_npar_10_and_one_more_is_refused():
    from crt1d_amd import _lib

    npar = 10
    lib = _lib.load()
    nd = lib.crt_hip_lm_chain_max_nd(npar)
    assert nd == R.max_nd(npar) == 83
    rng = np.random.default_rng(9700)
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    p0 = 0.1 * rng.normal(size=(2 * nd, npar))
    sums = _linear_case(rng, 2, nd, npar)(p0)
    ch = Chain(2, nd, _t(p0), w=_t(w)).step(_dev_sums(sums))
    got = ch.snap()
    A, g, _ = (v.reshape(2, nd, -1) for v in sums[0])
    fp = R.band_solve(A[1], g[1], p0.reshape(2, nd, npar)[1], w, float(got["lam"][1]))
    assert np.all(got["naccept"] == 1) and (p0.reshape(2, nd, npar)[1] + fp).tobytes() == got["p_trial"].reshape(2, nd, npar)[1].tobytes()
    cov = ch.covariance()
    assert np.all(np.isfinite(cov)) and np.all(np.diagonal(cov, axis1=2, axis2=3) > 0)
    w2 = _t(rng.uniform(0.5, 2.0, (nd, npar)))
    more = Chain(2, nd + 1, _t(np.zeros((2 * (nd + 1), npar))), w=w2)
    before = more.snap()
    more.step(_dev_sums(_linear_case(rng, 2, nd + 1, npar)(np.zeros((2 * (nd + 1), npar)))), expect=_lib.CRT_ERR_UNSUPPORTED)
    more.covariance(expect=_lib.CRT_ERR_UNSUPPORTED)
    assert _same(before, more.snap())


# ---- 6. the plans on the radiative transfer ------------------------------------------------------------------------------------------------
PSI = np.deg2rad([15.0, 30.0, 45.0, 58.0, 68.0])
NSTEP = 15


class _Calls:
    """A recording stand-in for a plan's library handle: the names of the entries called through it, in order."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _series_problem(nb, spectral):
    """2s, 10 levels, 6 pixels x 5 dates at five sun angles (each pixel's canopy replicated, the illumination scaled per date); unknowns:
    the coefficients of two leaf-reflectance directions and ln(LAI scale), the truth constant over the dates; noise-free.  Sensor rows:
    4 bands x 2 levels of the two diffuse fluxes; spectral: those two spectra at the same levels.  Date pix % 5 of every pixel is fully
    masked (inv_sigma = 0, y = NaN); p0 is perturbed differently per date."""
    import torch

    from crt1d_amd import batched, synth

    npix, nd, nz = 6, len(PSI), 10
    ncol = npix * nd
    d = synth.make_columns(npix, nb, nz, seed=17)
    rng = np.random.default_rng(171)
    per_date = lambda v: np.repeat(v, nd, axis=0)  # noqa: E731
    light = per_date(np.ones((npix, 1))) * np.tile(rng.uniform(0.7, 1.3, nd), npix)[:, None]
    cols = batched.Columns(_t(np.tile(PSI, npix)), _t(per_date(d["lai"])), _t(per_date(d["g_kind"])).to(torch.int32),
                           _t(per_date(d["g_param"])), _t(per_date(d["mla"])))
    bands = batched.Bands(_t(per_date(d["I_dr0"]) * light), _t(per_date(d["I_df0"]) * light), _t(per_date(d["leaf_r"])), _t(per_date(d["leaf_t"])),
                          _t(per_date(d["soil_r"])))
    mean = d["leaf_r"].mean(axis=0)
    dirs = _t(np.stack((0.3 * mean * np.sin(np.linspace(0.0, 3.0, nb)), 0.3 * mean * np.cos(np.linspace(0.0, 2.0, nb)))))
    truth = np.repeat(rng.uniform(-0.2, 0.2, (npix, 1, 3)), nd, axis=1)  # (npix, nd, npar)
    lev, keys = (0, nz - 1), ("I_df_d", "I_df_u")
    w = np.zeros((4, nb))
    for s in range(4):
        w[s, 9 * s:9 * s + 10] = np.hanning(12)[1:11]
    sensors = batched.SensorSet(w)
    p = _t(truth.reshape(ncol, 3))
    tc = batched.Columns(cols.psi, cols.lai * torch.exp(p[:, 2])[:, None], cols.g_kind, cols.g_param, cols.mla)
    tb = batched.Bands(bands.I_dr0, bands.I_df0, bands.leaf_r + p[:, 0, None] * dirs[0] + p[:, 1, None] * dirs[1], bands.leaf_t, bands.soil_r)
    if spectral:
        out = batched.solve_levels("2s", tc, tb, lev, keys=keys)
    else:
        out = batched.solve_sensor_levels("2s", tc, tb, lev, sensors, keys=keys)
    y = {k: out[k].clone() for k in keys}
    masked = np.zeros((npix, nd), dtype=bool)
    masked[np.arange(npix), np.arange(npix) % nd] = True
    mask = _t(masked.reshape(ncol))
    inv_sigma = {}
    for k in keys:
        y[k][mask] = float("nan")
        inv_sigma[k] = torch.ones_like(y[k])
        inv_sigma[k][mask] = 0.0
    p0 = rng.uniform(-0.05, 0.05, (ncol, 3))
    common = dict(keys=keys, d_leaf_r=dirs, lai=True, p0=_t(p0), inv_sigma=inv_sigma, lam0=1e-2, xtol=0.0, ftol=0.0)
    args = ("2s", cols, bands, lev) + (() if spectral else (sensors,)) + (y,)
    return dict(args=args, kw=common, truth=truth, p0=p0.reshape(npix, nd, 3), masked=masked, npix=npix, nd=nd,
                w=np.full((nd - 1, 3), 5.0))


@pytest.mark.parametrize("spectral", [False, True])
def test_plans_on_the_radiative_transfer(spectral):
    """Both chained plans end at the truth on every date, the masked one included, within 10 x the distance the unchained plan of the
    same columns reaches on its observed dates; the unchained plan leaves the masked date at p0; the pixel cost never increases.
    Measured on MI355X: see DESIGN.md 3.28."""
    import torch

    from crt1d_amd import batched

    P = _series_problem(40, spectral)
    Plan = batched.SpectralRetrievalPlan if spectral else batched.RetrievalPlan
    npix, nd, m = P["npix"], P["nd"], P["masked"]
    old = Plan(*P["args"], **P["kw"]).run(NSTEP)
    p_old = old.result()["p"].cpu().numpy().reshape(npix, nd, 3)
    dist_old = float(np.abs(p_old - P["truth"])[~m].max())
    assert np.array_equal(p_old[m], P["p0"][m])  # the difference the feature makes: alone, a masked date stays where it started
    plan = Plan(*P["args"], **P["kw"], chain=nd, inv_sigma_chain=P["w"])
    costs = []
    for _ in range(NSTEP):
        costs.append(plan.step().cost.clone())
    res = plan.result()
    torch.cuda.synchronize()
    costs = np.stack([c.cpu().numpy() for c in costs])
    p = res["p"].cpu().numpy()
    dist = float(np.abs(p - P["truth"]).max())
    status = res["status"].cpu().numpy()
    # converged: the cost fell by 12 orders and no pixel gave up (xtol = ftol = 0, so that the distance below is that of the last
    # bits and not that of a tolerance: a pixel then stays RUNNING at its fixed point; the CONVERGED codes are section 3's)
    assert not np.any((status == R.STALLED) | (status == R.FAILED_START)) and np.all(res["naccept"].cpu().numpy() >= 3)
    assert np.all(costs[-1] < 1e-12 * costs[0])
    assert p.shape == (npix, nd, 3) and costs.shape == (NSTEP, npix) and res["status"].shape == (npix,)
    assert np.all(costs[1:] <= costs[:-1])
    assert dist <= 10 * dist_old, (dist, dist_old)
    cov = plan.covariance().cpu().numpy()
    var = np.diagonal(cov, axis1=2, axis2=3)
    assert cov.shape == (npix, nd, 3, 3) and np.all(np.isfinite(cov)) and np.all(var > 0)
    with pytest.raises(ValueError, match="scale=True"):
        plan.covariance(scale=True)
    # a pixel alone gives the bits it has in the batch
    a = P["args"]
    one = Plan(a[0], a[1].slice(nd, 2 * nd), a[2].slice(nd, 2 * nd), *a[3:-1], {k: v[nd:2 * nd] for k, v in a[-1].items()},
               **{**P["kw"], "p0": P["kw"]["p0"][nd:2 * nd], "inv_sigma": {k: v[nd:2 * nd] for k, v in P["kw"]["inv_sigma"].items()}},
               chain=nd, inv_sigma_chain=P["w"]).run(NSTEP).result()
    assert one["p"].cpu().numpy().tobytes() == p[1:2].tobytes() and one["cost"].cpu().numpy().tobytes() == res["cost"][1:2].cpu().numpy().tobytes()


def test_chained_step_is_the_old_launches_with_the_last_replaced_by_two():
    from crt1d_amd import _lib, batched

    P = _series_problem(40, False)
    old = batched.RetrievalPlan(*P["args"], **P["kw"])
    new = batched.RetrievalPlan(*P["args"], **P["kw"], chain=P["nd"], inv_sigma_chain=P["w"])
    old.lib, new.lib = _Calls(old.lib), _Calls(new.lib)
    old.step()
    new.step()
    assert old.lib.names[-1] == "crt_hip_lm_step_f64" and len(old.lib.names) >= 2
    assert new.lib.names == old.lib.names[:-1] + ["crt_hip_lm_normal_f64", "crt_hip_lm_step_chain_f64"]
    assert _lib.load().crt_hip_last_kernel().decode().startswith("k_lm_step_chain nd=5 npar=3 nblk=1")
    spec = _series_problem(40, True)
    plan = batched.SpectralRetrievalPlan(*spec["args"], **spec["kw"], chain=spec["nd"], inv_sigma_chain=spec["w"])
    plan.lib = _Calls(plan.lib)
    plan.step()
    assert plan.lib.names[-1] == "crt_hip_lm_step_chain_f64" and "crt_hip_lm_step_normal_f64" not in plan.lib.names


def test_model_retrieve_chain():
    """Model.retrieve_chain is the batched chained plan on the model's one pixel: bitwise."""
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
    wch = np.full((nd - 1, 2), 3.0)
    got = m.retrieve_chain(w, y, psi, wch, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, inv_sigma=isg)
    assert got["params"] == ("dir0", "lai") and got["p"].shape == (nd, 2) and got["cov"].shape == (nd, 2, 2) and got["cost"].shape == ()
    scheme, cols, b, sun = m._series_inputs(psi, None, None, "retrieval")
    rep = lambda v: None if v is None else v.expand(nd, *v.shape[1:]).contiguous()  # noqa: E731
    cols = batched.Columns(psi=sun.psi[0].contiguous(), lai=rep(cols.lai), g_kind=rep(cols.g_kind), g_param=rep(cols.g_param), mla=rep(cols.mla),
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[0].contiguous(), g_table=rep(cols.g_table))
    b = batched.Bands(sun.I_dr0[0].contiguous(), sun.I_df0[0].contiguous(), rep(b.leaf_r), rep(b.leaf_t), rep(b.soil_r))
    ref = batched.retrieve("2s", cols, b, (-1,), batched.SensorSet(w), y, keys=("I_df_u",), niter=8, d_leaf_r=d, lai=True, inv_sigma=isg,
                           chain=nd, inv_sigma_chain=wch)
    torch.cuda.synchronize()
    for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
        assert got[k].tobytes() == ref[k][0].cpu().numpy().tobytes(), k
    var = np.diagonal(got["cov"], axis1=1, axis2=2)
    assert np.all(np.isfinite(got["cov"])) and np.all(var > 0) and np.all(got["p"][1] != 0.0)  # (the cloudy date moved off its start)
