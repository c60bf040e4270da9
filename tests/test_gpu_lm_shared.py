"""GPU: the chained Levenberg-Marquardt step with parameters shared by all dates of a pixel (include_shared/crt1d_hip_lm_shared.h)
through its C entries, then through the plans.

1. ns = 0: every state array and the covariance of crt_hip_lm_step_shared_f64 / crt_hip_lm_shared_covariance_f64 at mask = 0 AND of
   crt_hip_lm_step_chain_f64 / crt_hip_lm_chain_covariance_f64 are the bytes of tests/golden/lm_chain_bits.npz, after each of three steps:
   what the chain's own kernels gave before the two pairs became one (tools/gen_lm_chain_bits.py, through that commit's library).
2. ns = npar, one block, no prior: p_trial of every date, cost, lam, status are bitwise crt_hip_lm_step_normal_f64 on ONE column fed
   the nd dates' sums as nd blocks.
3. The fp64 restatement of tests/lm_shared_reference.py, bit for bit: general masks, per-pixel and shared weights, a fully masked date,
   dead entries; a pixel alone equals the pixel in a batch of 70; stopped pixels keep their bits.
4. Scripted decisions against the restatement; the shared columns of p and p_trial are bitwise equal over the dates after every call.
5. The solve and the covariance against the long-double dense layer, within the bounds below.
6. The largest nd at npar = 10, ns = 5; one more is refused and nothing is written.
7. - 10. The plans on the radiative transfer, the launch list, Model.retrieve_chain.

THE BOUNDS (u = 2^-53, n = nd nv + ns, M the scaled damped matrix, x its solution, s the scales): R.solve_bound, which is _solve_bound
of tests/test_gpu_lm_chain.py with n = nd nv + ns and the roundings of the border, the corner and the shared gradient added (its
docstring derives them).  Per entry |got - ref|_r <= s_r * bound + u (|delta_r| + |p_trial_r|).
 covariance: the backward error of the factor moves M^-1 by at most c u kappa_2 ||M^-1||_2 with the c of R.solve_bound; the chain's
   recursion adds at most 6 nd nv u kappa_2 ||M^-1||_2 (the chain test's derivation at nv).  The border's own share: per date the
   products R = Y^T - B^T Z, Z = W^T R, Q = Z S^-1 and Q Z^T, each entry a sum of at most max(nv, ns) <= npar terms of factors bounded
   by ||L^-1|| ||Y|| <= kappa_2^(1/2) ||M^-1||^(1/2) and ||S^-1|| <= ||M^-1||: 4 gamma_npar kappa_2 ||M^-1||_2 a date, 4 nd npar u kappa_2
   ||M^-1||_2 in all, and S^-1 = Lc^-T Lc^-1 once, 2 gamma_ns ||M^-1||_2; to first order (6 nd nv + 4 nd npar + 2 ns) u kappa_2 ||M^-1||_2
   <= 10 (n + nd ns) u kappa_2 ||M^-1||_2, far below c >= 12 n^2.  The bound asserted is the chain test's 2 c u kappa_2 ||M^-1||_2 s_r s_q:
   the second c is an ALLOWANCE that covers these terms with a wide margin.
 Measured on MI355X, largest error / bound: see DESIGN.md 3.29."""
import ctypes
import os

import numpy as np
import pytest

import lm_shared_reference as R
from test_gpu_lm_chain import OPTS, PER_PIX, PSI, Chain, _Calls, _dev_sums, _extras, _linear_case, _ptr, _stream  # noqa: F401
from test_gpu_retrieve import STATE, _same, _t

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


class Shared(Chain):
    """The shared entries on tensors of the test's own (Chain of the chain test, with the shared set)."""

    def __init__(self, npix, nd, p0, mask, **kw):
        from crt1d_amd import _lib

        super().__init__(npix, nd, p0, **kw)
        self.mask = mask
        self._shared = _lib.CrtLmShared(mask)

    def step(self, sums, expect=0):
        from crt1d_amd import _lib

        blk = (_lib.CrtLmNormalBlock * len(sums))(*[_lib.CrtLmNormalBlock(*[_ptr(v) for v in s]) for s in sums])
        st = self.lib.crt_hip_lm_step_shared_f64(ctypes.byref(self._chain), ctypes.byref(self._shared), ctypes.byref(self._prob), blk, len(sums),
                                                 ctypes.byref(self._state), _stream())
        assert st == expect, st
        return self

    def covariance(self, expect=0):
        import torch

        st = self.lib.crt_hip_lm_shared_covariance_f64(ctypes.byref(self._chain), ctypes.byref(self._shared), self.npar, _ptr(self.A), _ptr(self.cov),
                                                       _stream())
        assert st == expect, st
        torch.cuda.synchronize()
        return self.cov.cpu().numpy().reshape(self.npix, self.nd, self.npar, self.npar)


def _masks(npar):
    """none, first only, last only, alternating, all (the distinct ones)"""
    alt = sum(1 << k for k in range(0, npar, 2))
    return sorted({0, 1, 1 << (npar - 1), alt, (1 << npar) - 1})


def _agree(p, nd, mask):
    """p (npix * nd, npar) with the shared columns of every pixel set to date 0's"""
    p = p.copy()
    v = p.reshape(-1, nd, p.shape[1])
    ks = R.split(mask, p.shape[1])[1]
    v[:, :, ks] = v[:, :1, ks]
    return p


def _weights(rng, npix, nd, npar, per_pixel):
    return rng.uniform(0.5, 2.0, (npix, nd - 1, npar) if per_pixel else (nd - 1, npar))


CASES = [(nd, npar, mask) for nd in (1, 2, 3, 7) for npar in (1, 2, 5, 10) for mask in _masks(npar)]


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------------
BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_chain_bits.npz")
BITS_CASES = [(nd, npar) for nd in (1, 2, 3, 7) for npar in (1, 2, 5, 10)]


def chain_bits(nd, npar, make):
    """The case of item 1 (tools/gen_lm_chain_bits.py records it through the parent's library): three blocks, a prior with one unobserved
    row, bounds, date 1 without any observation (nd >= 3), per-pixel weights where nd + npar is odd.  make(npix, nd, p0, w=, **extras)
    -> a Chain.  Three steps, each on the sums at its own p_trial.  -> {"<step>/<array>"}: every array of snap() and the covariance."""
    npix = 3
    rng = np.random.default_rng(11000 + 10 * nd + npar)
    w = _weights(rng, npix, nd, npar, (nd + npar) % 2 == 1)
    sums_at = _linear_case(rng, npix, nd, npar, nblk=3, empty=1 if nd >= 3 else None)
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    ex = _extras(rng, npix * nd, npar)
    ch = make(npix, nd, _t(p0), w=_t(w) if nd > 1 else None, **ex)
    out = {}
    for it in range(3):
        snap = ch.step(_dev_sums(sums_at(ch.snap()["p_trial"]))).snap()
        out.update({f"{it}/{k}": snap[k] for k in STATE})
        out[f"{it}/cov"] = ch.covariance()
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(BITS) as f:
        return dict(f)


def test_golden_holds_exactly_the_cases(golden):
    want = {f"nd{nd}_npar{npar}/{it}/{k}" for nd, npar in BITS_CASES for it in range(3) for k in STATE + ("cov",)}
    assert set(golden) == want and len(want) == 16 * 3 * 10


@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("nd", [1, 2, 3, 7])
def test_nothing_shared_is_the_chain_bitwise(nd, npar, golden):
    """Both entries against the bytes the two chain kernels of the commit before the unification left: the chain entry and the shared
    entry at mask = 0 now launch one kernel, so comparing them with each other would compare a kernel with itself."""
    entries = {"chain": Chain, "shared": lambda npix, nd, p0, **kw: Shared(npix, nd, p0, 0, **kw)}
    for name, make in entries.items():
        got = chain_bits(nd, npar, make)
        for key, v in got.items():
            ref = golden[f"nd{nd}_npar{npar}/{key}"]
            assert v.dtype == ref.dtype and v.shape == ref.shape and v.tobytes() == ref.tobytes(), (name, key)
        assert got["2/naccept"].min() >= 2, name


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npar", [1, 2, 5, 10])
@pytest.mark.parametrize("nd", [1, 2, 4])
def test_everything_shared_is_step_normal_on_nd_blocks_bitwise(nd, npar):
    """One block at the chain's level, no prior, bounds: the nd dates' sums of a pixel fed to k_lm_step_normal as nd blocks of ONE column."""
    npix = 3
    rng = np.random.default_rng(12000 + 10 * nd + npar)
    mask = (1 << npar) - 1
    sums_at = _linear_case(rng, npix, nd, npar)
    p1 = 0.1 * rng.normal(size=(npix, npar))
    p0 = np.repeat(p1, nd, axis=0)
    lo, hi = _t(np.full(npar, -0.7)), _t(np.full(npar, 0.9))
    w = _t(np.full((nd - 1, npar), np.nan)) if nd > 1 else None  # (no varying parameter: never read)
    a, b = Chain(npix, None, _t(p1), lo=lo, hi=hi), Shared(npix, nd, _t(p0), mask, w=w, lo=lo, hi=hi)
    for it in range(3):
        pt = b.snap()["p_trial"]
        (A, g, c2), = sums_at(pt)
        per_date = [tuple(np.ascontiguousarray(v.reshape(npix, nd, *v.shape[1:])[:, d]) for v in (A, g, c2)) for d in range(nd)]
        sa, sb = a.step(_dev_sums(per_date)).snap(), b.step(_dev_sums([(A, g, c2)])).snap()
        for k in ("cost", "lam", "status", "naccept", "nreject"):
            assert sa[k].tobytes() == sb[k].tobytes(), (it, k)
        for d in range(nd):
            assert sb["p_trial"].reshape(npix, nd, npar)[:, d].tobytes() == sa["p_trial"].tobytes(), (it, d)
            assert sb["p"].reshape(npix, nd, npar)[:, d].tobytes() == sa["p"].tobytes(), (it, d)
    assert sa["naccept"].min() >= 2


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
def _check_against_restatement(got, ref, npix, nd, where):
    for i in range(npix):
        for k in PER_PIX:
            assert got[k][i] == ref[i][k] or (k == "cost" and np.isnan(got[k][i]) and np.isnan(ref[i][k])), (where, i, k, got[k][i], ref[i][k])
        for k in ("p", "p_trial", "A", "g"):
            assert got[k].reshape(npix, nd, -1)[i].tobytes() == ref[i][k].tobytes(), (where, i, k)


@pytest.mark.parametrize("nd,npar,mask", CASES)
def test_restatement_bit_for_bit(nd, npar, mask):
    """Three blocks, a prior with one unobserved row, bounds, date 1 of every pixel without any observation (nd >= 3); per-pixel weights
    where nd + npar is odd, shared ones otherwise; the start disagrees over the dates on the shared columns (date 0 counts).  Two steps."""
    npix = 3
    rng = np.random.default_rng(13000 + 1000 * nd + 50 * npar + mask % 47)
    per_pixel = (nd + npar) % 2 == 1
    w = _weights(rng, npix, nd, npar, per_pixel)
    sums_at = _linear_case(rng, npix, nd, npar, nblk=3, empty=1 if nd >= 3 else None)
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    ex = _extras(rng, npix * nd, npar)
    host = {k: v.cpu().numpy() for k, v in ex.items()}
    ch = Shared(npix, nd, _t(p0), mask, w=_t(w) if nd > 1 else None, **ex)
    ref = [R.new_state(p0.reshape(npix, nd, npar)[i], 1e-2) for i in range(npix)]
    ks = R.split(mask, npar)[1]
    for it in range(2):
        sums = sums_at(ch.snap()["p_trial"])
        got = ch.step(_dev_sums(sums)).snap()
        for i in range(npix):
            blocks = [tuple(v.reshape(npix, nd, *v.shape[1:])[i] for v in s) for s in sums]
            wi = (w[i] if per_pixel else w) if nd > 1 else np.zeros((0, npar))
            ref[i] = R.step(ref[i], blocks, wi, ch.opt, mask, host["lo"], host["hi"], host["prior"].reshape(npix, nd, npar)[i],
                            host["isp"].reshape(npix, nd, npar)[i])
        _check_against_restatement(got, ref, npix, nd, it)
        for k in ("p", "p_trial"):
            v = got[k].reshape(npix, nd, npar)[:, :, ks]
            assert v.tobytes() == np.repeat(v[:, :1], nd, axis=1).tobytes(), (it, k)
    assert got["naccept"].min() >= 1


def test_dead_entries_in_the_varying_and_in_the_shared_part():
    """Parameter 1 (varying) has neither data nor coupling on date 1; parameter 2 (shared) has no data on any date: delta = 0 there,
    variance +inf, zero covariances; the rest is the restatement's, finite."""
    npix, nd, npar, mask = 1, 3, 4, 0b0101
    rng = np.random.default_rng(13900)
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    w[:, 1] = 0.0
    J = rng.normal(size=(nd, 9, npar))
    J[1, :, 1] = 0.0
    J[:, :, 2] = 0.0
    r = rng.normal(size=(nd, 9))
    sums = [(R.pack(np.einsum("coi,coj->cij", J, J)), np.einsum("coi,co->ci", J, r), np.einsum("co,co->c", r, r))]
    p0 = _agree(0.1 * rng.normal(size=(nd, npar)), nd, mask)
    ch = Shared(npix, nd, _t(p0), mask, w=_t(w)).step(_dev_sums(sums))
    got, cov = ch.snap(), ch.covariance()[0]
    ref = R.step(R.new_state(p0, 1e-2), sums, w, ch.opt, mask)
    _check_against_restatement(got, [ref], 1, nd, "dead")
    pt = got["p_trial"]
    assert pt[1, 1] == p0[1, 1] and np.all(pt[[0, 2], 1] != p0[[0, 2], 1]) and np.all(pt[:, 2] == p0[0, 2]) and np.all(np.isfinite(pt))
    assert np.all(pt[:, 0] != p0[0, 0]) and np.all(pt[:, 3] != p0[:, 3])
    for d in range(nd):
        assert cov[d, 2, 2] == np.inf and np.all(cov[d, 2, [0, 1, 3]] == 0.0) and np.all(cov[d, [0, 1, 3], 2] == 0.0)
        live = [0, 3] if d == 1 else [0, 1, 3]
        assert np.all(np.isfinite(cov[d][np.ix_(live, live)])) and np.all(np.diagonal(cov[d])[live] > 0)
    assert cov[1, 1, 1] == np.inf and np.all(cov[1, 1, [0, 2, 3]] == 0.0) and np.all(cov[1, [0, 2, 3], 1] == 0.0)


@pytest.mark.parametrize("per_pixel", [False, True])
def test_pixel_alone_equals_pixel_in_batch_and_stopped_pixels_keep_their_bits(per_pixel):
    npix, nd, npar, pix, mask = 70, 3, 5, 37, 0b10010
    rng = np.random.default_rng(13950 + per_pixel)
    w = _weights(rng, npix, nd, npar, per_pixel)
    w1 = w[pix:pix + 1] if per_pixel else w
    sums_at = _linear_case(rng, npix, nd, npar, nblk=3)
    p0 = 0.1 * rng.normal(size=(npix * nd, npar))
    ex = _extras(rng, npix * nd, npar)
    cols = slice(pix * nd, (pix + 1) * nd)
    one = {k: (v[cols] if v.shape[0] == npix * nd else v) for k, v in ex.items()}
    big, small = Shared(npix, nd, _t(p0), mask, w=_t(w), **ex), Shared(1, nd, _t(p0[cols]), mask, w=_t(w1), **one)
    stopped = [5, 64]
    big.status[stopped] = R.CONVERGED_X
    before = big.snap()
    for it in range(3):
        sb = sums_at(big.snap()["p_trial"])
        for s in sb:
            for v in s:
                v.reshape(npix, nd, -1)[stopped] = np.nan  # what a stopped pixel would read
        ss = [tuple(v[cols] for v in s) for s in sb]
        big.step(_dev_sums(sb))
        small.step(_dev_sums(ss))
        a, b = big.snap(), small.snap()
        for k in STATE:
            n = nd if k in ("p", "p_trial", "A", "g") else 1
            assert a[k][pix * n:(pix + 1) * n].tobytes() == b[k].tobytes(), (it, k)
            for q in stopped:
                assert a[k][q * n:(q + 1) * n].tobytes() == before[k][q * n:(q + 1) * n].tobytes(), (it, k, q)
    assert a["naccept"][pix] >= 2
    assert big.covariance()[pix].tobytes() == small.covariance()[0].tobytes()


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
def _run_script(rng, script, nd=3, npar=3, mask=0b101, npix=3, nsteps=6, **opts):
    """Steps of the kernel and of the fp64 restatement on the same supplied sums.  script(it, pix, sums) may spoil the sums of a step.
    After every step every state array has the restatement's bits and the shared columns agree over the dates.  -> the snapshots"""
    w = rng.uniform(0.5, 2.0, (npix, nd - 1, npar))
    sums_at = _linear_case(rng, npix, nd, npar)
    p0 = _agree(0.1 * rng.normal(size=(npix * nd, npar)), nd, mask)  # (as the plans start: a pixel that never accepts keeps its p)
    lo, hi = np.full(npar, -5.0), np.full(npar, 5.0)
    ch = Shared(npix, nd, _t(p0), mask, w=_t(w), lo=_t(lo), hi=_t(hi), **opts)
    ref = [R.new_state(p0.reshape(npix, nd, npar)[i], 1e-2) for i in range(npix)]
    ks = R.split(mask, npar)[1]
    history = []
    for it in range(nsteps):
        (A, g, c2), = sums_at(ch.snap()["p_trial"])
        A, g, c2 = A.reshape(npix, nd, -1), g.reshape(npix, nd, -1), c2.reshape(npix, nd)
        for i in range(npix):
            script(it, i, (A[i], g[i], c2[i]))
        ch.step(_dev_sums([(A.reshape(npix * nd, -1), g.reshape(npix * nd, -1), c2.reshape(-1))]))
        got = ch.snap()
        for i in range(npix):
            ref[i] = R.step(ref[i], [(A[i], g[i], c2[i])], w[i], ch.opt, mask, lo, hi)
        _check_against_restatement(got, ref, npix, nd, it)
        for k in ("p", "p_trial"):
            v = got[k].reshape(npix, nd, npar)[:, :, ks]
            assert v.tobytes() == np.repeat(v[:, :1], nd, axis=1).tobytes(), (it, k)
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

    h = _run_script(np.random.default_rng(181), script, nsteps=3)
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

    h = _run_script(np.random.default_rng(182), script, nsteps=4, lam_max=0.05)
    assert list(h[1]["status"]) == [0, 0, 0] and list(h[2]["status"]) == [R.STALLED] * 3 and list(h[3]["nreject"]) == [2, 2, 2]
    assert np.array_equal(h[3]["p"], h[3]["p_trial"])


def test_decisions_converged_f():
    h = _run_script(np.random.default_rng(183), lambda *a: None, nsteps=6, ftol=1e-3)
    assert list(h[-1]["status"]) == [R.CONVERGED_F] * 3 and list(h[0]["status"]) == [0, 0, 0] and np.array_equal(h[-1]["p"], h[-1]["p_trial"])


def test_decisions_converged_x():
    h = _run_script(np.random.default_rng(184), lambda *a: None, nsteps=6, xtol=1e-4)
    assert list(h[-1]["status"]) == [R.CONVERGED_X] * 3 and list(h[0]["status"]) == [0, 0, 0] and np.array_equal(h[-1]["p"], h[-1]["p_trial"])


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
def _flat(v, mask):
    """(nd, npar) -> (n,) in the header's ordering (a shared entry from date 0)"""
    kv, ks = R.split(mask, v.shape[1])
    return np.concatenate([v[:, kv].reshape(-1), v[0, ks]])


def _solve_fraction(nd, npar, mask, lam):
    """The case of the test: every assertion but the last.  -> the largest error / bound"""
    npix = 3
    rng = np.random.default_rng(19000 + 1000 * nd + 50 * npar + mask % 47 + (lam > 0))
    per_pixel = (nd + npar) % 2 == 1
    w = _weights(rng, npix, nd, npar, per_pixel)
    p0 = _agree(0.1 * rng.normal(size=(npix * nd, npar)), nd, mask)
    sums = _linear_case(rng, npix, nd, npar)(p0)
    A, g, c2 = (v.reshape(npix, nd, *v.shape[1:]) for v in sums[0])
    P = p0.reshape(npix, nd, npar)
    wp = lambda i: (w[i] if per_pixel else w) if nd > 1 else np.zeros((0, npar))  # noqa: E731
    got = Shared(npix, nd, _t(p0), mask, w=_t(w) if nd > 1 else None, lam0=lam, lam_down=1.0, lam_min=0.0).step(_dev_sums(sums)).snap()
    assert np.array_equal(got["p"], p0) and np.all(got["naccept"] == 1) and np.all(got["lam"] == lam)
    worst = 0.0
    for i in range(npix):
        ref = R.solve_ld(A[i], g[i], P[i], wp(i), lam, mask)  # (n,), long double
        _, _, s = R.dense_ld(A[i], g[i], P[i], wp(i), lam, mask)
        bound, s64, _, _, _ = R.solve_bound(A[i], g[i], P[i], wp(i), lam, mask, float(np.linalg.norm((ref / s).astype(np.float64))))
        pt = got["p_trial"].reshape(npix, nd, npar)[i]
        allowed = s64 * bound + U * (np.abs(ref.astype(np.float64)) + np.abs(_flat(pt, mask)))
        assert allowed.max() < 1e-6, allowed.max()  # (of the inputs: the bound means something)
        err = np.abs(_flat(pt, mask).astype(LD) - _flat(P[i], mask).astype(LD) - ref).astype(np.float64)
        worst = max(worst, float((err / allowed).max()))
        m = nd + (nd - 1) * (npar - bin(mask).count("1"))
        want = R.cost_ld(c2[i], P[i], wp(i), mask)
        assert abs(LD(got["cost"][i]) - want) <= 2 * m * U * want
    return worst


@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("nd,npar,mask", CASES)
def test_solve_against_long_double_dense(nd, npar, mask, lam):
    assert _solve_fraction(nd, npar, mask, lam) <= 1.0


def _covariance_fraction(nd, npar, mask):
    """The case of the test: every assertion but the last.  -> the largest error / bound"""
    npix = 3
    rng = np.random.default_rng(19500 + 1000 * nd + 50 * npar + mask % 47)
    per_pixel = (nd + npar) % 2 == 1
    w = _weights(rng, npix, nd, npar, per_pixel)
    wp = lambda i: (w[i] if per_pixel else w) if nd > 1 else np.zeros((0, npar))  # noqa: E731
    p0 = np.zeros((npix * nd, npar))
    sums = _linear_case(rng, npix, nd, npar, scale=4.0)(p0)
    A = sums[0][0].reshape(npix, nd, -1)
    ch = Shared(npix, nd, _t(p0), mask, w=_t(w) if nd > 1 else None).step(_dev_sums(sums))
    cov = ch.covariance()
    kv, ks = R.split(mask, npar)
    worst = 0.0
    for i in range(npix):
        X = R.inverse_ld(A[i], wp(i), mask)
        z = np.zeros((nd, npar))
        _, s64, c, lo, hi = R.solve_bound(A[i], z, z, wp(i), 0.0, mask, 0.0)
        S = np.diag(s64)
        for d in range(nd):
            ref = R.marginal(X, d, nd, npar, mask)
            sd = np.diagonal(R.marginal(S, d, nd, npar, mask))
            bound = 2 * c * U * (hi / lo) / lo * sd[:, None] * sd[None, :]
            assert bound.max() < 1e-6
            err = np.abs(cov[i, d].astype(LD) - ref).astype(np.float64)
            worst = max(worst, float((err / bound).max()))
            assert np.array_equal(cov[i, d], cov[i, d].T)
            assert cov[i, d][np.ix_(ks, ks)].tobytes() == cov[i, 0][np.ix_(ks, ks)].tobytes()  # the shared block: the same bits on every date
    return worst


@pytest.mark.parametrize("nd,npar,mask", CASES)
def test_covariance_against_long_double_inverse(nd, npar, mask):
    assert _covariance_fraction(nd, npar, mask) <= 1.0


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
def test_largest_nd_at_npar_10_with_5_shared_and_one_more_is_refused():
    from crt1d_amd import _lib

    npar, mask = 10, 0b0101010101
    lib = _lib.load()
    nd = lib.crt_hip_lm_shared_max_nd(npar, 5)
    assert nd == R.max_nd(npar, 5) == 212
    rng = np.random.default_rng(19700)
    w = rng.uniform(0.5, 2.0, (nd - 1, npar))
    p0 = _agree(0.1 * rng.normal(size=(2 * nd, npar)), nd, mask)
    sums = _linear_case(rng, 2, nd, npar)(p0)
    ch = Shared(2, nd, _t(p0), mask, w=_t(w)).step(_dev_sums(sums))
    got = ch.snap()
    A, g, _ = (v.reshape(2, nd, -1) for v in sums[0])
    P = p0.reshape(2, nd, npar)[1]
    dv, ds = R.bordered_solve(A[1], g[1], P, w, float(got["lam"][1]), mask)
    assert np.all(got["naccept"] == 1) and R.trial_point(P, dv, ds, mask).tobytes() == got["p_trial"].reshape(2, nd, npar)[1].tobytes()
    cov = ch.covariance()
    assert np.all(np.isfinite(cov)) and np.all(np.diagonal(cov, axis1=2, axis2=3) > 0)
    w2 = _t(rng.uniform(0.5, 2.0, (nd, npar)))
    more = Shared(2, nd + 1, _t(np.zeros((2 * (nd + 1), npar))), mask, w=w2)
    before = more.snap()
    cov_before = more.cov.cpu().numpy().tobytes()
    more.step(_dev_sums(_linear_case(rng, 2, nd + 1, npar)(np.zeros((2 * (nd + 1), npar)))), expect=_lib.CRT_ERR_UNSUPPORTED)
    more.covariance(expect=_lib.CRT_ERR_UNSUPPORTED)
    assert _same(before, more.snap()) and more.cov.cpu().numpy().tobytes() == cov_before


# ---- 7. - 10. the plans on the radiative transfer ------------------------------------------------------------------------------------------
NSTEP = 25
SHARED = ("dir0", "dir1")
# The distance from the truth the shared sensor plan reached on MI355X, times 1000: last-bit distances move by orders
# with the summation order.  Never above 1e-6 of the parameter scale (of order 1): a retrieval that failed to separate the unknowns is
# off by 1e-3 or more.
BAR = min(1000 * 3.4e-13, 1e-6)


def _series_problem(nb, spectral):
    """The model of the chain test's _series_problem, restated for shared parameters: 2s, 10 levels, 6 pixels x 5 dates at five sun angles
    (each pixel's canopy replicated, the illumination scaled per date); unknowns: the coefficients of two leaf-reflectance directions
    (the truth constant over the dates) and ln(LAI scale) (the truth different on every date); noise-free.  Sensor rows: ONE band over
    the whole spectrum at two levels of the upward diffuse flux -- two rows a date against three unknowns; spectral: that spectrum at
    the same levels.  The first direction lives in the first half of the spectrum, the second in the second half.  The weights of the
    chain are 0: nothing but the sharing ties the dates."""
    import torch

    from crt1d_amd import batched, synth

    npix, nd, nz = 6, len(PSI), 10
    ncol = npix * nd
    d = synth.make_columns(npix, nb, nz, seed=17)
    rng = np.random.default_rng(271)
    per_date = lambda v: np.repeat(v, nd, axis=0)  # noqa: E731
    light = per_date(np.ones((npix, 1))) * np.tile(rng.uniform(0.7, 1.3, nd), npix)[:, None]
    cols = batched.Columns(_t(np.tile(PSI, npix)), _t(per_date(d["lai"])), _t(per_date(d["g_kind"])).to(torch.int32),
                           _t(per_date(d["g_param"])), _t(per_date(d["mla"])))
    bands = batched.Bands(_t(per_date(d["I_dr0"]) * light), _t(per_date(d["I_df0"]) * light), _t(per_date(d["leaf_r"])), _t(per_date(d["leaf_t"])),
                          _t(per_date(d["soil_r"])))
    mean = d["leaf_r"].mean(axis=0)
    half = np.arange(nb) < nb // 2
    dirs = _t(np.stack((0.3 * mean * half, 0.3 * mean * ~half)))
    truth = np.concatenate([np.repeat(rng.uniform(-0.2, 0.2, (npix, 1, 2)), nd, axis=1), rng.uniform(-0.3, 0.3, (npix, nd, 1))], axis=2)
    lev, keys = (0, nz - 1), ("I_df_u",)
    sensors = batched.SensorSet(np.ones((1, nb)))
    p = _t(truth.reshape(ncol, 3))
    tc = batched.Columns(cols.psi, cols.lai * torch.exp(p[:, 2])[:, None], cols.g_kind, cols.g_param, cols.mla)
    tb = batched.Bands(bands.I_dr0, bands.I_df0, bands.leaf_r + p[:, 0, None] * dirs[0] + p[:, 1, None] * dirs[1], bands.leaf_t, bands.soil_r)
    if spectral:
        out = batched.solve_levels("2s", tc, tb, lev, keys=keys)
    else:
        out = batched.solve_sensor_levels("2s", tc, tb, lev, sensors, keys=keys)
    y = {k: out[k].clone() for k in keys}
    p0 = _agree(rng.uniform(-0.05, 0.05, (ncol, 3)), nd, 0b011)
    common = dict(keys=keys, d_leaf_r=dirs, lai=True, p0=_t(p0), lam0=1e-2, xtol=0.0, ftol=0.0)
    args = ("2s", cols, bands, lev) + (() if spectral else (sensors,)) + (y,)
    return dict(args=args, kw=common, truth=truth, npix=npix, nd=nd, w=np.zeros((nd - 1, 3)), at_truth=(tc, tb), sensors=sensors, lev=lev,
                dirs=dirs, keys=keys)


def _joint_jacobian(P):
    """The Jacobian of a pixel's 2 nd sensor rows with respect to (ln LAI_0 .. ln LAI_{nd-1}, dir0, dir1) at the truth, dense, from one
    SensorJacPlan call.  -> (npix, 2 nd, nd + 2)"""
    import torch

    from crt1d_amd import batched

    tc, tb = P["at_truth"]
    jac = batched.SensorJacPlan("2s", tc, tb, P["lev"], P["sensors"], d_leaf_r=P["dirs"], lai=True, keys=P["keys"])
    jac()
    torch.cuda.synchronize()
    npix, nd = P["npix"], P["nd"]
    J = jac.out[P["keys"][0]].cpu().numpy().reshape(npix, nd, -1, 3)  # (pixel, date, row, (dir0, dir1, lai))
    nrow = J.shape[2]
    full = np.zeros((npix, nd * nrow, nd + 2))
    for d in range(nd):
        full[:, d * nrow:(d + 1) * nrow, d] = J[:, d, :, 2]
        full[:, d * nrow:(d + 1) * nrow, nd:] = J[:, d, :, :2]
    return full


def _run(plan, nstep):
    import torch

    costs = []
    for _ in range(nstep):
        costs.append(plan.step().cost.clone())
    res = plan.result()
    torch.cuda.synchronize()
    return res, np.stack([c.cpu().numpy() for c in costs])


def test_sensor_plan_with_two_rows_a_date_needs_the_sharing():
    """Two rows a date against three unknowns: every date alone is singular, the five dates together with the two directions shared
    are 10 rows against 7 unknowns.  The shared plan ends at the truth on every date; the chained plan without `shared` does not."""
    from crt1d_amd import batched

    P = _series_problem(40, False)
    npix, nd = P["npix"], P["nd"]
    J = _joint_jacobian(P)
    assert J.shape == (npix, 2 * nd, nd + 2)
    sv = np.linalg.svd(J, compute_uv=False)
    kappa = sv[:, 0] / sv[:, -1]
    print("kappa_2 of the joint Jacobian:", kappa)
    assert np.all(sv[:, -1] > 0) and np.all(kappa < 1e8), kappa
    plan = batched.RetrievalPlan(*P["args"], **P["kw"], chain=nd, inv_sigma_chain=P["w"], shared=SHARED)
    assert plan.shared == SHARED
    res, costs = _run(plan, NSTEP)
    p = res["p"].cpu().numpy()
    status = res["status"].cpu().numpy()
    dist = float(np.abs(p - P["truth"]).max())
    print("distance from the truth, shared:", dist, "cost", costs[0].max(), "->", costs[-1].max())
    assert not np.any((status == R.STALLED) | (status == R.FAILED_START))
    assert np.all(costs[1:] <= costs[:-1]) and np.all(costs[-1] < 1e-12 * costs[0])
    assert p.shape == (npix, nd, 3) and p[:, :, :2].tobytes() == np.repeat(p[:, :1, :2], nd, axis=1).tobytes()
    assert dist <= BAR, (dist, BAR)
    cov = plan.covariance().cpu().numpy()
    var = np.diagonal(cov, axis1=2, axis2=3)
    assert cov.shape == (npix, nd, 3, 3) and np.all(np.isfinite(cov)) and np.all(var > 0)
    assert cov[:, :, :2, :2].tobytes() == np.repeat(cov[:, :1, :2, :2], nd, axis=1).tobytes()
    with pytest.raises(ValueError, match="scale=True"):
        plan.covariance(scale=True)
    # the difference the feature makes: the same problem without `shared` has a singular system on every date
    old, _ = _run(batched.RetrievalPlan(*P["args"], **P["kw"], chain=nd, inv_sigma_chain=P["w"]), NSTEP)
    dist_old = np.abs(old["p"].cpu().numpy() - P["truth"]).max(axis=(0, 2))
    print("distance from the truth, not shared, per date:", dist_old)
    assert np.any(dist_old > BAR)
    # a pixel alone gives the bits it has in the batch
    a = P["args"]
    one = batched.RetrievalPlan(a[0], a[1].slice(nd, 2 * nd), a[2].slice(nd, 2 * nd), *a[3:-1], {k: v[nd:2 * nd] for k, v in a[-1].items()},
                                **{**P["kw"], "p0": P["kw"]["p0"][nd:2 * nd]}, chain=nd, inv_sigma_chain=P["w"], shared=SHARED).run(NSTEP).result()
    assert one["p"].cpu().numpy().tobytes() == p[1:2].tobytes() and one["cost"].cpu().numpy().tobytes() == res["cost"][1:2].cpu().numpy().tobytes()


def test_spectral_plan_with_shared_directions():
    """40 bands at two levels: every date alone is determined.  The sharing plan reaches the truth within 10 x the distance the chained
    plan of the same columns reaches (the chain test's own criterion)."""
    from crt1d_amd import batched

    P = _series_problem(40, True)
    npix, nd = P["npix"], P["nd"]
    old, _ = _run(batched.SpectralRetrievalPlan(*P["args"], **P["kw"], chain=nd, inv_sigma_chain=P["w"]), NSTEP)
    dist_old = float(np.abs(old["p"].cpu().numpy() - P["truth"]).max())
    plan = batched.SpectralRetrievalPlan(*P["args"], **P["kw"], chain=nd, inv_sigma_chain=P["w"], shared=np.array([True, True, False]))
    res, costs = _run(plan, NSTEP)
    p, status = res["p"].cpu().numpy(), res["status"].cpu().numpy()
    dist = float(np.abs(p - P["truth"]).max())
    print("distance from the truth, spectral: shared", dist, "chained", dist_old)
    assert not np.any((status == R.STALLED) | (status == R.FAILED_START))
    assert np.all(costs[1:] <= costs[:-1]) and np.all(costs[-1] < 1e-12 * costs[0])
    assert p[:, :, :2].tobytes() == np.repeat(p[:, :1, :2], nd, axis=1).tobytes()
    assert dist <= 10 * dist_old, (dist, dist_old)
    cov = plan.covariance().cpu().numpy()
    assert np.all(np.isfinite(cov)) and np.all(np.diagonal(cov, axis1=2, axis2=3) > 0)
    assert cov[:, :, :2, :2].tobytes() == np.repeat(cov[:, :1, :2, :2], nd, axis=1).tobytes()


def test_shared_step_is_the_chained_launch_list_with_the_last_name_replaced():
    import torch

    from crt1d_amd import _lib, batched

    P = _series_problem(40, False)
    old = batched.RetrievalPlan(*P["args"], **P["kw"], chain=P["nd"], inv_sigma_chain=P["w"])
    new = batched.RetrievalPlan(*P["args"], **P["kw"], chain=P["nd"], inv_sigma_chain=P["w"], shared=SHARED)
    old.lib, new.lib = _Calls(old.lib), _Calls(new.lib)
    old.step()
    new.step()
    assert old.lib.names[-1] == "crt_hip_lm_step_chain_f64" and len(old.lib.names) >= 3
    assert new.lib.names == old.lib.names[:-1] + ["crt_hip_lm_step_shared_f64"]
    assert _lib.load().crt_hip_last_kernel().decode().startswith("k_lm_step_shared nd=5 npar=3 ns=2 nblk=1")
    spec = _series_problem(40, True)
    plan = batched.SpectralRetrievalPlan(*spec["args"], **spec["kw"], chain=spec["nd"], inv_sigma_chain=spec["w"], shared=SHARED)
    plan.lib = _Calls(plan.lib)
    plan.step()
    assert plan.lib.names[-1] == "crt_hip_lm_step_shared_f64" and "crt_hip_lm_step_chain_f64" not in plan.lib.names
    # p0 / reset: the shared entries of the dates after the first are date 0's; the prior of a shared parameter counts once
    p0 = np.random.default_rng(5).uniform(-0.05, 0.05, (P["npix"] * P["nd"], 3))
    kw = {**P["kw"], "p0": _t(p0)}
    prior, isp = np.zeros((P["npix"] * P["nd"], 3)), np.ones((P["npix"] * P["nd"], 3))
    plan = batched.RetrievalPlan(*P["args"], **kw, chain=P["nd"], inv_sigma_chain=P["w"], shared=SHARED, prior=prior, inv_sigma_prior=isp)
    torch.cuda.synchronize()
    want = _agree(p0, P["nd"], 0b011)
    assert plan.p.cpu().numpy().tobytes() == want.tobytes() == plan.p_trial.cpu().numpy().tobytes()
    plan.reset(p0[::-1].copy())
    assert plan.p.cpu().numpy().tobytes() == _agree(p0[::-1].copy(), P["nd"], 0b011).tobytes()
    got = plan.inv_sigma_prior.cpu().numpy().reshape(P["npix"], P["nd"], 3)
    assert np.all(got[:, 0] == 1.0) and np.all(got[:, 1:, :2] == 0.0) and np.all(got[:, 1:, 2] == 1.0)


def test_model_retrieve_chain_with_shared():
    """Model.retrieve_chain(shared=...) is the batched plan on the model's one pixel: bitwise."""
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
    wch = np.full((nd - 1, 2), 3.0)
    got = m.retrieve_chain(w, y, psi, wch, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, shared=("dir0",))
    assert got["params"] == ("dir0", "lai") and got["p"].shape == (nd, 2) and got["cov"].shape == (nd, 2, 2) and got["cost"].shape == ()
    scheme, cols, b, sun = m._series_inputs(psi, None, None, "retrieval")
    rep = lambda v: None if v is None else v.expand(nd, *v.shape[1:]).contiguous()  # noqa: E731
    cols = batched.Columns(psi=sun.psi[0].contiguous(), lai=rep(cols.lai), g_kind=rep(cols.g_kind), g_param=rep(cols.g_param), mla=rep(cols.mla),
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[0].contiguous(), g_table=rep(cols.g_table))
    b = batched.Bands(sun.I_dr0[0].contiguous(), sun.I_df0[0].contiguous(), rep(b.leaf_r), rep(b.leaf_t), rep(b.soil_r))
    ref = batched.retrieve("2s", cols, b, (-1,), batched.SensorSet(w), y, keys=("I_df_u",), niter=8, d_leaf_r=d, lai=True, chain=nd,
                           inv_sigma_chain=wch, shared=[True, False])
    torch.cuda.synchronize()
    for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
        assert got[k].tobytes() == ref[k][0].cpu().numpy().tobytes(), k
    var = np.diagonal(got["cov"], axis1=1, axis2=2)
    assert np.all(np.isfinite(got["cov"])) and np.all(var > 0)
    assert got["p"][:, 0].tobytes() == np.repeat(got["p"][0, 0], nd).tobytes() and len(set(got["p"][:, 1])) == nd
    assert got["cov"][:, 0, 0].tobytes() == np.repeat(got["cov"][0, 0, 0], nd).tobytes()
    plain = m.retrieve_chain(w, y, psi, wch, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8)
    assert len(set(plain["p"][:, 0])) == nd  # (without `shared` every date has its own)
