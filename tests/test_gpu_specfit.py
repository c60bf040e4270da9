"""GPU: the spectral normal equations in one kernel and the step on them (include/crt1d_hip_specfit.h; batched.SpectralNormalPlan,
batched.SpectralRetrievalPlan, batched.retrieve_spectral, Model.retrieve_spectral).

1. fwd against LevelsPlan.  The kernel's primal is the closed form the derivative kernels differentiate; k_lev advances its exponentials
   by recurrence and writes 2s through A / sigma, so the two are not bit-equal.  Asserted: 4 x the largest |diff| / max |X| measured over
   the cases of this file on MI355X (FWD_MEASURED).
2. A, g, c2 against the composition: torch fp64 from the kernel's own fwd, the tangents of LevelsJacPlan, LevelsDlaiPlan and
   LevelsDleafPlan contracted with the directions, and inv_sigma.  The bound is derived (U = 2^-53, gamma_k = k U / (1 - k U)): a direction
   tangent is 3 products and 2 sums (3 roundings at most on a term), w = t s one more, r = (X - y) s two, the product w_i w_j one: at most 9
   roundings on a term, each relative to the absolute values sum_p |X'_p| |d_p| |s| (wa) and |r|; n terms summed in any order add
   n - 1.  Both sides (the kernel, torch) are held to it, so
       |got - ref| <= 2 gamma_{n + 9} S,   S = sum_o wa_i wa_j,   n = the rows of the column (nkey * nsel * nb).
3. Bitwise invariants: batch, another column's mask, c2 and fwd under a different parameter set, A with and without fwd.
4. Masks: NaN under inv_sigma = 0.
5. crt_hip_lm_step_normal_f64 against crt_hip_lm_step_f64, bitwise, and its state machine.
6. Twin retrievals against the host loop of the composition, against RetrievalPlan at nb = 13, and the covariance.
7. Refusals through the C entry."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_retrieve import LM, STATE, _bound, _dev, _random_blocks, _same, _scaled, _t

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLOSED = ("2s", "bl", "g77", "bf")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
JAC_KEYS = ("I_df_d", "I_df_u", "F")
PARAMS = ("leaf_r", "leaf_t", "soil_r")
ELLIPSOIDAL = 3
NBS = (1, 5, 64, 65, 300, 130, 2151)  # 64 / 65 cross a wave; 300: two 256-lane slices; 130: two slices at the 128-lane width (88 rows)
# 1.: the largest |fwd - LevelsPlan| / max |X| over _cases(), measured once on MI355X, per scheme.  bl (bit-equal on ragged columns) and
# g77 differ by the recurrence of k_lev's exponentials; 2s (nb = 300, uniform) and bf (nb = 65, uniform) by the removable singularity k_lev
# divides through (2s: sigma = mu_bar^2 (K_b^2 - h^2); bf: k_d - k_b), 1e-16 / (b - a) in the value, which the closed form of
# jac_schemes.hpp evaluates by phi instead: the figure follows how close a band of the case comes to it.
FWD_MEASURED = {"2s": 1.1e-12, "bl": 2.0e-15, "g77": 2.1e-15, "bf": 7.7e-13}
FWD_TOL = {k: 4 * v for k, v in FWD_MEASURED.items()}


def _gamma(k):
    return k * U / (1 - k * U)


def _config(nb):
    """(ncol, nz, levels, keys, ntan) of a band count: nsel in {1, 2}, one to four keys, 3 directions (nb = 130: 8, the widest axis)."""
    ncol, nz = (2 if nb == 2151 else 3 + nb % 3), 5 + nb % 3
    if nb == 130:
        return ncol, nz, (1, nz - 1), KEYS, 8
    keys = {1: ("I_df_u",), 5: ("I_dr", "F"), 64: ("I_df_u",), 65: ("I_df_d", "I_df_u"), 300: KEYS, 2151: ("I_df_u",)}[nb]
    return ncol, nz, ((0, nz - 1) if nb in (5, 65, 300) else (nz - 1,)), keys, 3


@functools.lru_cache(maxsize=None)
def _inputs(nb, uniform):
    """Device columns with the ellipsoidal leaf-angle class, spectra, the leaf tangent and the directions (per column on uniform columns,
    shared on ragged ones)."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nz, lev, keys, ntan = _config(nb)
    d = dict(synth.make_columns(ncol, nb, nz, seed=100 + nb, uniform_dlai=uniform))
    rng = np.random.default_rng(7 * nb + uniform)
    d["g_kind"] = np.full(ncol, ELLIPSOIDAL, dtype=np.int32)
    d["g_param"] = rng.uniform(0.7, 2.0, ncol)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    dirs = {}
    for k in PARAMS:
        base = d[k] if uniform else d[k].mean(axis=0, keepdims=True)
        dirs[k] = _t(rng.uniform(-1.0, 1.0, (base.shape[0], ntan, nb)) * base[:, None, :])
    torch.cuda.synchronize()
    return cols, bands, tan, dirs


def _dkw(dirs):
    return {"d_" + k: (v[0] if v.shape[0] == 1 else v) for k, v in dirs.items()}


@functools.lru_cache(maxsize=None)
def _reference(scheme, nb, uniform):
    """What the existing plans give, computed once: the level spectra and the tangents, contracted with the directions in torch fp64.
    -> X {key: (ncol, nsel, nb)}, T {key: (ncol, nsel, nb, npar)}, Ta (the same with absolute values)"""
    import torch

    from crt1d_amd import batched

    cols, bands, tan, dirs = _inputs(nb, uniform)
    ncol, nz, lev, keys, ntan = _config(nb)
    X = {k: v.clone() for k, v in batched.solve_levels(scheme, cols, bands, lev).items()}
    J = batched.solve_levels_jac(scheme, cols, bands, lev)
    A = batched.solve_levels_dlai(scheme, cols, bands, lev)
    B = batched.solve_levels_dleaf(scheme, cols, bands, lev, tan)
    T, Ta = {}, {}
    for k in KEYS:
        if k in JAC_KEYS:
            t = sum(J[k][:, :, p, None, :] * dirs[n][:, None, :, :] for p, n in enumerate(PARAMS))  # (ncol, nsel, ntan, nb)
            ta = sum(J[k][:, :, p, None, :].abs() * dirs[n][:, None, :, :].abs() for p, n in enumerate(PARAMS))
        else:
            t = ta = torch.zeros((ncol, len(lev), ntan, nb), dtype=torch.float64, device="cuda")
        T[k] = torch.cat([t.permute(0, 1, 3, 2), A[k][..., None], B[k][..., None]], dim=3)
        Ta[k] = torch.cat([ta.permute(0, 1, 3, 2), A[k][..., None].abs(), B[k][..., None].abs()], dim=3)
    torch.cuda.synchronize()
    return X, T, Ta


@functools.lru_cache(maxsize=None)
def _observations(scheme, nb, uniform):
    """y = the level spectra with 5 % noise, inv_sigma in [0.5, 2] / the key's mean (the last of several keys has none: the NULL path)."""
    ncol, nz, lev, keys, ntan = _config(nb)
    X = _reference(scheme, nb, uniform)[0]
    rng = np.random.default_rng(3 * nb + 11)
    y, s = {}, {}
    for i, k in enumerate(keys):
        x = X[k].cpu().numpy()
        y[k] = _t(x * (1 + 0.05 * rng.normal(size=x.shape)) + 0.01 * np.abs(x).max())
        if i == 0 or i + 1 < len(keys):
            s[k] = _t(rng.uniform(0.5, 2.0, x.shape) / max(np.abs(x).mean(), 1e-3))
    return y, s


def _normal(scheme, nb, uniform, *, y=None, s=None, cols=slice(None), select=None, fwd=True, **kw):
    """One call of a fresh SpectralNormalPlan on the case (or its columns `cols`).  select: 'lai' = the LAI column alone."""
    import torch

    from crt1d_amd import batched

    c, b, tan, dirs = _inputs(nb, uniform)
    ncol, nz, lev, keys, ntan = _config(nb)
    y0, s0 = _observations(scheme, nb, uniform)
    y, s = y0 if y is None else y, s0 if s is None else s
    if cols != slice(None):
        c, b, tan = c.slice(cols.start, cols.stop), b.slice(cols.start, cols.stop), batched.LeafTangent(tan.dg_table[cols].contiguous(), tan.dg_at_psi[cols].contiguous())
        dirs = {k: (v if v.shape[0] == 1 else v[cols].contiguous()) for k, v in dirs.items()}
        y, s = {k: v[cols].contiguous() for k, v in y.items()}, {k: v[cols].contiguous() for k, v in s.items()}
    par = dict(_dkw(dirs), lai=True, tangent=tan) if select is None else dict(lai=True, tangent=None)
    plan = batched.SpectralNormalPlan(scheme, c, b, lev, y, keys=keys, inv_sigma=s, fwd=fwd, **par, **kw)
    out = plan()
    torch.cuda.synchronize()
    res = {k: out[k].clone() for k in ("A", "g", "c2")}
    if fwd:
        res["fwd"] = {k: v.clone() for k, v in out["fwd"].items()}
    return plan, res


@functools.lru_cache(maxsize=None)
def _got(scheme, nb, uniform):
    return _normal(scheme, nb, uniform)


def _compose(scheme, nb, uniform, fwd, y, s, rows=None):
    """The composition in torch fp64 and the derived bound: -> (A (ncol, npar, npar), g, c2), (bA, bg, bc2).  rows {key: bool mask}: the rows
    that are kept (default: all)."""
    import torch

    ncol, nz, lev, keys, ntan = _config(nb)
    _, T, Ta = _reference(scheme, nb, uniform)
    Jw, Ja, r = [], [], []
    for k in keys:
        sk = s[k] if k in s else torch.ones_like(y[k])
        keep = torch.ones_like(sk, dtype=torch.bool) if rows is None else rows[k]
        sk = torch.where(keep, sk, torch.zeros_like(sk))
        Jw.append((T[k] * sk[..., None]).reshape(ncol, -1, ntan + 2))
        Ja.append((Ta[k] * sk.abs()[..., None]).reshape(ncol, -1, ntan + 2))
        r.append(torch.where(keep, (fwd[k] - y[k]) * sk, torch.zeros_like(sk)).reshape(ncol, -1))
    Jw, Ja, r = torch.cat(Jw, 1), torch.cat(Ja, 1), torch.cat(r, 1)
    n = Jw.shape[1]
    g2 = 2 * _gamma(n + 9)
    ref = (torch.einsum("coi,coj->cij", Jw, Jw), torch.einsum("coi,co->ci", Jw, r), (r * r).sum(1))
    bound = (g2 * torch.einsum("coi,coj->cij", Ja, Ja), g2 * torch.einsum("coi,co->ci", Ja, r.abs()), g2 * (r * r).sum(1))
    return ref, bound


def _dense(A, npar):
    import torch

    i, j = torch.tril_indices(npar, npar, device=A.device)
    M = A.new_zeros((A.shape[0], npar, npar))
    M[:, i, j] = A
    M[:, j, i] = A
    return M


def _ratio(got, ref, bound):
    """The largest |got - ref| / bound; an element whose bound is 0 must be met exactly."""
    import torch

    err = (got - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / torch.where(bound == 0, torch.ones_like(bound), bound)).max())


def _cases():
    for scheme in CLOSED:
        for nb in NBS:
            for uniform in (True, False):
                if nb == 2151 and not (uniform ^ (scheme in ("bl", "bf"))):
                    continue  # (the large case once per scheme: uniform for 2s and g77, ragged for bl and bf)
                yield pytest.param(scheme, nb, uniform, id=f"{scheme}-{nb}-{'uniform' if uniform else 'ragged'}")


# ---- 1., 2. -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,nb,uniform", _cases())
def test_fwd_and_normal_equations(scheme, nb, uniform):
    """fwd within FWD_TOL of LevelsPlan relative to the key's largest value; A, g and c2 within the derived bound of the composition.
    Measured on MI355X, the largest |got - ref| / bound over the cases: A 0.087 (bf, nb = 5), g 0.065, c2 0.051; from 64 bands on below
    0.05, from 300 on below 0.006.  bl observed in I_df_u alone (nb = 1, 64, 2151) has no signal: every sum is +0.
    The check of fwd, A, g and c2 against the oracle, not against other kernels: test_gpu_deriv_domain.py::test_spectral_normal_equations."""
    ncol, nz, lev, keys, ntan = _config(nb)
    plan, got = _got(scheme, nb, uniform)
    X = _reference(scheme, nb, uniform)[0]
    y, s = _observations(scheme, nb, uniform)
    worst = 0.0
    for k in keys:
        scale = float(X[k].abs().max())
        if scale == 0.0:  # (bl has no upward stream)
            assert bool((got["fwd"][k] == 0).all())
            continue
        worst = max(worst, float((got["fwd"][k] - X[k]).abs().max()) / scale)
    ref, bound = _compose(scheme, nb, uniform, got["fwd"], y, s)
    npar = ntan + 2
    assert plan.params == tuple(f"dir{k}" for k in range(ntan)) + ("lai", "leaf") and got["A"].shape == (ncol, npar * (npar + 1) // 2)
    ratios = (_ratio(_dense(got["A"], npar), ref[0], bound[0]), _ratio(got["g"], ref[1], bound[1]), _ratio(got["c2"], ref[2], bound[2]))
    print(f"specfit {scheme} nb={nb} {'uniform' if uniform else 'ragged'}: fwd {worst:.3e} of max |X|; error / bound A {ratios[0]:.3e} "
          f"g {ratios[1]:.3e} c2 {ratios[2]:.3e}; {plan.last_kernel()}")
    assert ("k_spec_normal_finish" in plan.last_kernel()) == (nb in (300, 130, 2151))
    assert worst <= FWD_TOL[scheme]
    assert max(ratios) <= 1.0
    if scheme == "bl" and keys == ("I_df_u",):
        assert all(bool((got[k] == 0).all()) for k in ("A", "g", "c2"))
    else:
        assert bool((got["c2"] > 0).all())


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
@pytest.mark.parametrize("nb", [65, 300])
def test_bits(scheme, nb):
    import torch

    ncol, nz, lev, keys, ntan = _config(nb)
    assert ncol == 5 if nb == 65 else ncol == 3
    _, full = _got(scheme, nb, True)
    # a column alone is the column in the batch
    _, one = _normal(scheme, nb, True, cols=slice(1, 2))
    for k in ("A", "g", "c2"):
        assert torch.equal(one[k], full[k][1:2]), k
    for k in keys:
        assert torch.equal(one["fwd"][k], full["fwd"][k][1:2])
    # another column's mask does not reach this one
    y, s = _observations(scheme, nb, True)
    s2 = {k: v.clone() for k, v in s.items()}
    s2[keys[0]][0, :, ::2] = 0.0
    s2[keys[0]][2] = 0.0
    _, masked = _normal(scheme, nb, True, s=s2)
    for k in ("A", "g", "c2"):
        assert torch.equal(masked[k][1], full[k][1]), k
        assert not torch.equal(masked[k][0], full[k][0])
    # c2 and fwd do not depend on which parameters are asked for
    _, lai = _normal(scheme, nb, True, select="lai")
    assert torch.equal(lai["c2"], full["c2"]) and all(torch.equal(lai["fwd"][k], full["fwd"][k]) for k in keys)
    npar = ntan + 2
    assert torch.equal(lai["A"][:, 0], full["A"][:, (npar - 2) * (npar - 1) // 2 + npar - 2])  # (and the LAI diagonal is the same sum)
    assert torch.equal(lai["g"][:, 0], full["g"][:, npar - 2])
    # A does not depend on whether fwd is written
    _, bare = _normal(scheme, nb, True, fwd=False)
    for k in ("A", "g", "c2"):
        assert torch.equal(bare[k], full[k]), k


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", CLOSED)
@pytest.mark.parametrize("nb", [65, 300])
def test_masks(scheme, nb):
    """inv_sigma = 0 on a third of the rows with NaN in their y: finite, bitwise the result with finite garbage there, within the bound of
    2. on the kept rows; a column with every row masked gives zeros."""
    import torch

    ncol, nz, lev, keys, ntan = _config(nb)
    y, s = _observations(scheme, nb, False)
    rng = np.random.default_rng(nb)
    s = {k: (s[k].clone() if k in s else torch.ones_like(y[k])) for k in keys}
    dead = {k: _t(rng.uniform(size=tuple(y[k].shape)) < 1 / 3) for k in keys}
    for k in keys:
        dead[k][ncol - 1] = True  # the last column: nothing observed
        s[k][dead[k]] = 0.0
    y_nan = {k: torch.where(dead[k], torch.full_like(y[k], float("nan")), y[k]) for k in keys}
    y_junk = {k: torch.where(dead[k], torch.full_like(y[k], -7.5e3), y[k]) for k in keys}
    _, a = _normal(scheme, nb, False, y=y_nan, s=s)
    _, b = _normal(scheme, nb, False, y=y_junk, s=s)
    for k in ("A", "g", "c2"):
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
        assert bool((a[k][ncol - 1] == 0).all()) and not bool(torch.signbit(a[k][ncol - 1]).any())
    ref, bound = _compose(scheme, nb, False, a["fwd"], y_junk, s, rows={k: ~dead[k] for k in keys})
    npar = ntan + 2
    assert _ratio(_dense(a["A"], npar), ref[0], bound[0]) <= 1 and _ratio(a["g"], ref[1], bound[1]) <= 1 and _ratio(a["c2"], ref[2], bound[2]) <= 1


# ---- 5. ---------------------------------------------------------------------------------------------------------------------------------
class LMN(LM):
    """The step entry on supplied sums: blocks = [dict(A, g, c2)] of CUDA tensors; the state and the options of test_gpu_retrieve.LM."""

    def __init__(self, sums, p0, **kw):
        from crt1d_amd import _lib

        super().__init__([], p0, **kw)
        self.sums = sums
        self._blk = (_lib.CrtLmNormalBlock * len(sums))(*[_lib.CrtLmNormalBlock(b["A"].data_ptr(), b["g"].data_ptr(), b["c2"].data_ptr()) for b in sums])

    def step(self):
        import torch

        from crt1d_amd import _lib

        st = self.lib.crt_hip_lm_step_normal_f64(ctypes.byref(self._prob), self._blk, len(self.sums), ctypes.byref(self._state),
                                                 torch.cuda.current_stream().cuda_stream)
        assert st == _lib.CRT_OK, st
        return self


def _sums_of(state):
    """The block a first, prior-free call of crt_hip_lm_step_f64 stored: A, g and 2 cost (exact: cost = 0.5 * the sum)."""
    return dict(A=_t(state["A"]), g=_t(state["g"]), c2=_t(2.0 * state["cost"]))


@pytest.mark.parametrize("npar", [1, 5, 10])
def test_step_normal_against_step_bitwise(npar):
    ncol, nrow = 6, 37
    rng = np.random.default_rng(50 + npar)
    blocks = _random_blocks(rng, ncol, [nrow], npar)
    p0 = rng.normal(size=(ncol, npar))
    rows = LM(_dev(blocks), _t(p0)).step().snap()  # the first call is always accepted
    assert np.all(rows["naccept"] == 1)
    sums = LMN([_sums_of(rows)], _t(p0)).step().snap()
    assert _same(rows, sums)
    # with a prior (one row of it unobserved) and with bounds: the prior rows come last in either entry
    prior, isp = rng.normal(size=(ncol, npar)), rng.uniform(0.5, 2.0, (ncol, npar))
    if npar > 1:
        isp[:, npar // 2], prior[:, npar // 2] = 0.0, np.nan
    lo, hi = np.median(p0, axis=0) - 1e-3, np.median(p0, axis=0) + 1e-3  # (tight: trial points are clamped)
    kw = lambda: dict(prior=_t(prior), isp=_t(isp), lo=_t(lo), hi=_t(hi))  # noqa: E731
    a = LM(_dev(blocks), _t(p0), **kw()).step().snap()
    b = LMN([_sums_of(rows)], _t(p0), **kw()).step().snap()
    assert _same(a, b)
    assert np.any(a["p_trial"] == lo) or np.any(a["p_trial"] == hi)
    assert not np.array_equal(a["A"], rows["A"])


def test_step_normal_two_blocks_and_state_machine():
    import torch

    ncol, npar = 6, 4
    rng = np.random.default_rng(8)
    p0 = rng.normal(size=(ncol, npar))
    s1 = LM(_dev(_random_blocks(rng, ncol, [20], npar)), _t(p0)).step().snap()
    s2 = LM(_dev(_random_blocks(rng, ncol, [31], npar)), _t(p0)).step().snap()
    b1, b2 = _sums_of(s1), _sums_of(s2)
    lm = LMN([b1, b2], _t(p0))
    lm.status[4] = 3  # a finished column
    before = lm.snap()
    got = lm.step().snap()
    live = [c for c in range(ncol) if c != 4]
    assert got["A"][live].tobytes() == (s1["A"] + s2["A"])[live].tobytes() and got["g"][live].tobytes() == (s1["g"] + s2["g"])[live].tobytes()
    assert got["cost"][live].tobytes() == (0.5 * (2.0 * s1["cost"] + 2.0 * s2["cost"]))[live].tobytes()
    assert all(got[k][4].tobytes() == before[k][4].tobytes() for k in STATE)  # a column that is not running is not touched
    assert np.all(got["naccept"][live] == 1) and np.all(got["lam"][live] == 1e-2 * 0.1)
    # a rejected trial: a larger c2 leaves p, cost, A and g alone and raises lam
    b1["c2"].mul_(4.0)
    b1["A"].mul_(3.0)
    rej = lm.step().snap()
    assert _same(got, rej, ("p", "cost", "A", "g", "naccept", "status"))
    assert np.array_equal(rej["lam"][live], got["lam"][live] * 10.0) and np.all(rej["nreject"][live] == 1) and rej["nreject"][4] == 0
    assert rej["lam"][4] == before["lam"][4]
    # a NaN c2 on the first call
    b2["c2"][2] = float("nan")
    first = LMN([b1, b2], _t(p0)).step().snap()
    assert first["status"][2] == 4 and np.all(np.delete(first["status"], 2) == 0)
    assert first["naccept"][2] == 0 and first["nreject"][2] == 0 and np.isinf(first["cost"][2]) and np.array_equal(first["p_trial"][2], first["p"][2])
    torch.cuda.synchronize()


# ---- 6. ---------------------------------------------------------------------------------------------------------------------------------
NSTEP = 15


@functools.lru_cache(maxsize=None)
def _twin(scheme, nb=40):
    """A noise-free twin: y from LevelsPlan at a known p*, 3 directions + ln LAI + the ellipsoidal x.  2s: I_df_u at the top.  bl has no upward
    stream, and at the top (L = 0) none of its spectra depends on a parameter: its twin observes I_dr and I_df_d at the ground and at
    mid-canopy instead; its soil direction is dead, so its three directions lie in leaf_r, leaf_t and leaf_r again."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nz = 4, 7
    d = synth.make_columns(ncol, nb, nz, seed=5)
    rng = np.random.default_rng(41)
    wl = np.linspace(0.0, 3.0, nb)
    shapes = np.stack([np.sin(wl) + 1.5, np.cos(2 * wl), wl / 3.0])
    if scheme == "bl":
        dirs = {"d_leaf_r": _t(0.1 * d["leaf_r"].mean(axis=0) * shapes * np.array([1.0, 0.0, 1.0])[:, None]),
                "d_leaf_t": _t(0.1 * d["leaf_t"].mean(axis=0) * shapes * np.array([0.0, 1.0, 0.0])[:, None])}
        lev, keys = (0, nz // 2), ("I_dr", "I_df_d")
    else:
        dirs = {"d_leaf_r": _t(0.1 * d["leaf_r"].mean(axis=0) * shapes * np.array([1.0, 0.0, 0.0])[:, None]),
                "d_leaf_t": _t(0.1 * d["leaf_t"].mean(axis=0) * shapes * np.array([0.0, 1.0, 0.0])[:, None]),
                "d_soil_r": _t(0.1 * d["soil_r"].mean(axis=0) * shapes * np.array([0.0, 0.0, 1.0])[:, None])}
        lev, keys = (nz - 1,), ("I_df_u",)
    truth = torch.cat((_t(rng.uniform(-0.2, 0.2, (ncol, 3))), _t(rng.uniform(-0.2, 0.2, (ncol, 1))), _t(rng.uniform(0.8, 1.8, (ncol, 1)))), dim=1)
    kind = torch.full((ncol,), ELLIPSOIDAL, dtype=torch.int32, device="cuda")
    x0 = torch.full((ncol,), 1.2, dtype=torch.float64, device="cuda")
    base_cols = batched.Columns(_t(d["psi"]), _t(d["lai"]), kind, x0, _t(d["mla"]))
    base_bands = batched.Bands(_t(d["I_dr0"]), _t(d["I_df0"]), _t(d["leaf_r"]), _t(d["leaf_t"]), _t(d["soil_r"]))

    def inputs(p):
        cols = batched.Columns(base_cols.psi, base_cols.lai * torch.exp(p[:, 3])[:, None], kind, p[:, 4].contiguous(), base_cols.mla)
        spec = {}
        for n in PARAMS:
            v = getattr(base_bands, n)
            if "d_" + n in dirs:
                v = v + torch.einsum("ck,kb->cb", p[:, :3], dirs["d_" + n])
            spec[n] = v
        return cols, batched.Bands(base_bands.I_dr0, base_bands.I_df0, spec["leaf_r"], spec["leaf_t"], spec["soil_r"])

    def spectra(p):  # {key: (ncol, nsel, nb)}
        return {k: v.clone() for k, v in batched.solve_levels(scheme, *inputs(p), lev, keys=keys).items()}

    def forward(p):  # (ncol, nrow), rows in the order (key, level, band)
        X = spectra(p)
        return torch.cat([X[k].reshape(ncol, -1) for k in keys], dim=1)

    def jacobian(p):  # (ncol, nrow, 5): the composition
        cols, bands = inputs(p)
        J = batched.solve_levels_jac(scheme, cols, bands, lev)
        A = batched.solve_levels_dlai(scheme, cols, bands, lev)
        B = batched.solve_levels_dleaf(scheme, cols, bands, lev, batched.leaf_tangent(cols, "param"))
        out = []
        for k in keys:
            if k in JAC_KEYS:
                t = sum(J[k][:, :, q, :, None] * dirs["d_" + n].T[None, None] for q, n in enumerate(PARAMS) if "d_" + n in dirs)
            else:
                t = torch.zeros((ncol, len(lev), nb, 3), dtype=torch.float64, device="cuda")
            out.append(torch.cat([t, A[k][..., None], B[k][..., None]], dim=3).reshape(ncol, -1, 5))
        return torch.cat(out, dim=1)

    y = spectra(truth)
    zero = torch.zeros((ncol, 4), dtype=torch.float64, device="cuda")
    p0 = torch.cat((zero, x0[:, None]), dim=1)
    p_host, hist = _host_loop_x(forward, jacobian, p0, torch.cat([y[k].reshape(ncol, -1) for k in keys], dim=1))
    torch.cuda.synchronize()
    return dict(cols=base_cols, bands=base_bands, dirs=dirs, truth=truth, lev=lev, keys=keys, y=y, p0=p0, forward=forward, jacobian=jacobian,
                host_p=p_host, host_error=float((p_host - truth).abs().max()), host_hist=hist)


def _host_loop_x(forward, jacobian, p, y, niter=NSTEP - 1):
    """test_gpu_retrieve._host_loop with the clamp on the last parameter (x in [0.2, 5]) instead of the third."""
    import torch

    from crt1d_amd import batched

    lam = torch.full((p.shape[0],), 1e-2, dtype=torch.float64, device="cuda")
    r = forward(p) - y
    hist = [(r * r).sum(1)]
    for _ in range(niter):
        trial = p + batched.gauss_newton_step(jacobian(p), r, damping=lam)
        trial[:, -1] = trial[:, -1].clamp(0.2, 5.0)
        rt = forward(trial) - y
        better = (rt * rt).sum(1) < hist[-1]
        p = torch.where(better[:, None], trial, p)
        r = torch.where(better[:, None], rt, r)
        lam = torch.where(better, lam / 10, lam * 10)
        hist.append((r * r).sum(1))
    assert bool((lam < 1e12).all())  # (the host loop's status: still running)
    return p, torch.stack(hist).cpu().numpy()


def _twin_plan(P, scheme, **kw):
    from crt1d_amd import batched

    lo, hi = np.array([-np.inf] * 4 + [0.2]), np.array([np.inf] * 4 + [5.0])
    return batched.SpectralRetrievalPlan(scheme, P["cols"], P["bands"], P["lev"], P["y"], keys=P["keys"], **P["dirs"], lai=True, leaf=True,
                                         p0=P["p0"], lo=lo, hi=hi, lam0=1e-2, lam_up=10.0, lam_down=0.1, xtol=0.0, ftol=0.0, **kw)


@pytest.mark.parametrize("scheme", ["2s", "bl"])
def test_twin_retrieval(scheme):
    """From the displaced p0 the plan reaches p*: the cost never increases and ends below 1e-12 of the first; the parameter error is at most
    10 x that of the host loop of the composition after the same number of steps (the rule of tests/test_gpu_retrieve.py: both stop at the
    conditioning of the problem), and the status is the host loop's (running).  run() repeats the single steps bitwise; fitted() is the
    observation to the same accuracy; covariance() is the inverse of the composed J^T J to 32 npar EPS cond(scaled J^T J)^2 (the inverse is
    compared entry by entry in the scaled variables, and the plan's own A sits within 2 gamma S of the composed one).  Measured on MI355X
    after 15 steps, largest parameter error: 2s plan 2.8e-12, host loop 1.7e-12, cost 1.4e-01 -> 2.9e-28; bl plan 6.8e-15, host loop
    7.4e-15, cost 2.2e+00 -> 6.9e-30; covariance error / bound 3.7e-05 and 9.7e-05."""
    import torch

    P = _twin(scheme)
    plan = _twin_plan(P, scheme)
    costs = []
    for _ in range(NSTEP):
        costs.append(plan.step().cost.clone())
    torch.cuda.synchronize()
    state = {k: getattr(plan, k).cpu().numpy().copy() for k in STATE}
    costs = np.stack([c.cpu().numpy() for c in costs])
    truth = P["truth"].cpu().numpy()
    err = float(np.abs(state["p"] - truth).max())
    print(f"twin {scheme}: parameter error plan {err:.3e}, host loop {P['host_error']:.3e}; cost {costs[0].max():.3e} -> {costs[-1].max():.3e} "
          f"(host loop misfit {P['host_hist'][0].max():.3e} -> {P['host_hist'][-1].max():.3e}); accepted {state['naccept']}, rejected {state['nreject']}")
    assert np.all(costs[1:] <= costs[:-1]) and costs[-1].max() < 1e-12 * costs[0].max()
    assert err <= 10 * P["host_error"], (err, P["host_error"])
    assert np.all(state["status"] == 0)
    assert float(np.abs(state["p"] - P["host_p"].cpu().numpy()).max()) <= 11 * P["host_error"]  # (both within their error of p*)
    again = plan.reset().run(NSTEP)
    torch.cuda.synchronize()
    assert all(getattr(again, k).cpu().numpy().tobytes() == state[k].tobytes() for k in STATE)
    res = plan.result()
    assert res["params"] == ("dir0", "dir1", "dir2", "lai", "leaf") and np.array_equal(res["p"].cpu().numpy(), state["p"])
    nrow = len(P["keys"]) * len(P["lev"]) * 40
    assert bool((plan.nobs() == nrow).all())
    fit = plan.fitted()
    for k in P["keys"]:
        assert float((fit[k] - P["y"][k]).abs().max()) <= 1e-9 * float(P["y"][k].abs().max())
    # the covariance against the inverse of the composed normal matrix at the accepted point
    J = P["jacobian"](plan.p.clone()).cpu().numpy()
    cov = plan.covariance().cpu().numpy()
    worst = 0.0
    for c in range(J.shape[0]):
        A = J[c].T @ J[c]
        As, sc = _scaled(A)
        cond = np.linalg.cond(As)
        unscale = 1.0 / (sc[:, None] * sc[None, :])
        ref = np.linalg.inv(A)
        # (the plan's A sits within 2 gamma S of the composed one: a relative perturbation of the scaled matrix far below EPS cond)
        worst = max(worst, float((np.abs(cov[c] - ref) * unscale).max() / (_bound(5, cond=cond) * cond * np.abs(ref * unscale).max())))
    print(f"twin {scheme}: covariance error / bound {worst:.3e}")
    assert worst <= 1.0
    scaled = plan.covariance(scale=True).cpu().numpy()
    chi2 = 2.0 * state["cost"] / (nrow - 5)
    assert np.allclose(scaled, cov * chi2[:, None, None], rtol=1e-12, atol=0)


def test_twin_against_sensor_retrieval():
    """nb = 13: RetrievalPlan with 13 single-band unit-weight sensors is the same problem.  After the first step (the evaluation of p0) the
    stored normal equations agree within the bound of 2. plus what the two forward values may differ by (1.: FWD_TOL max |X| on every
    residual, times the weighted tangent), and the final p agrees as both agree with p*."""
    import torch

    from crt1d_amd import batched

    nb = 13
    P = _twin("2s", nb)
    spec = _twin_plan(P, "2s")
    sens = batched.SensorSet.from_supports(np.arange(nb), np.ones(nb, dtype=np.int64), np.ones(nb), nb=nb)
    lo, hi = np.array([-np.inf] * 4 + [0.2]), np.array([np.inf] * 4 + [5.0])
    rp = batched.RetrievalPlan("2s", P["cols"], P["bands"], P["lev"], sens, {"I_df_u": P["y"]["I_df_u"]}, keys=("I_df_u",), **P["dirs"], lai=True,
                               leaf=True, p0=P["p0"], lo=lo, hi=hi, lam0=1e-2, lam_up=10.0, lam_down=0.1, xtol=0.0, ftol=0.0)
    spec.step()
    rp.step()
    torch.cuda.synchronize()
    J = P["jacobian"](P["p0"])  # (ncol, 13, 5)
    r = P["forward"](P["p0"]) - P["y"]["I_df_u"].reshape(4, -1)
    g2 = 2 * _gamma(nb + 9)
    slack = FWD_TOL["2s"] * max(float(P["y"]["I_df_u"].abs().max()), float(P["forward"](P["p0"]).abs().max()))
    bA = g2 * torch.einsum("coi,coj->cij", J.abs(), J.abs())
    bg = g2 * torch.einsum("coi,co->ci", J.abs(), r.abs()) + slack * J.abs().sum(1)
    bc = g2 * (r * r).sum(1) + 2 * slack * r.abs().sum(1) + nb * slack * slack
    assert _ratio(_dense(spec.A, 5), _dense(rp.A, 5), bA) <= 1 and _ratio(spec.g, rp.g, bg) <= 1
    assert _ratio(2 * spec.cost, 2 * rp.cost, bc) <= 1
    spec.run(NSTEP - 1)
    rp.run(NSTEP - 1)
    torch.cuda.synchronize()
    e_spec, e_rp = float((spec.p - P["truth"]).abs().max()), float((rp.p - P["truth"]).abs().max())
    print(f"nb = 13: parameter error spectral {e_spec:.3e}, sensor plan {e_rp:.3e}, host loop {P['host_error']:.3e}")
    assert e_spec <= 10 * P["host_error"] and e_rp <= 10 * P["host_error"]
    assert float((spec.p - rp.p).abs().max()) <= 20 * P["host_error"]


def test_one_shots_and_model():
    """retrieve_spectral is the plan; Model.retrieve_spectral is the batched call on the model's own column: bitwise."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    P = _twin("2s")
    lo, hi = np.array([-np.inf] * 4 + [0.2]), np.array([np.inf] * 4 + [5.0])
    res = batched.retrieve_spectral("2s", P["cols"], P["bands"], P["lev"], P["y"], keys=P["keys"], niter=6, **P["dirs"], lai=True, leaf=True,
                                    p0=P["p0"], lo=lo, hi=hi)
    plan = _twin_plan(P, "2s").run(6)
    torch.cuda.synchronize()
    assert torch.equal(res["p"], plan.p) and torch.equal(res["cov"], plan.covariance()) and res["params"] == plan.params
    sums = batched.spectral_normal("2s", P["cols"], P["bands"], P["lev"], P["y"], keys=P["keys"], lai=True)
    assert set(sums) == {"A", "g", "c2"} and sums["A"].shape == (4, 1) and bool((sums["c2"] > 0).all())
    m = Model("2s", nlayers=12)
    nb = m.nwl
    d = np.random.default_rng(3).uniform(-0.05, 0.05, (1, nb)) * m.copy_p()["leaf_r"]
    scheme, cols, b, sun = m._series_inputs(np.atleast_1d(float(m._p["psi"])), None, None, "spectral retrieval")
    cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
    b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
    y = {"I_df_u": 1.03 * batched.solve_levels("2s", cols, b, (-1,), keys=("I_df_u",))["I_df_u"][0].cpu().numpy()}
    mask = np.ones_like(y["I_df_u"])
    mask[:, nb // 3: nb // 3 + 4] = 0.0  # a masked window
    y["I_df_u"][:, nb // 3] = np.nan
    got = m.retrieve_spectral(y, levels=(-1,), directions={"leaf_r": d}, lai=True, niter=8, inv_sigma={"I_df_u": mask})
    assert got["params"] == ("dir0", "lai") and got["p"].shape == (2,) and got["cov"].shape == (2, 2) and np.isfinite(got["cost"])
    ref = batched.retrieve_spectral("2s", cols, b, (-1,), {"I_df_u": y["I_df_u"][None]}, keys=("I_df_u",), niter=8, d_leaf_r=d, lai=True,
                                    inv_sigma={"I_df_u": mask[None]})
    torch.cuda.synchronize()
    for k in ("p", "cost", "status", "lam", "naccept", "nreject", "cov"):
        assert got[k].tobytes() == ref[k][0].cpu().numpy().tobytes(), k
    first = 0.5 * float(np.nansum((0.03 / 1.03 * y["I_df_u"] * mask) ** 2))
    assert got["cost"] < 0.5 * first  # (it did lower the cost of the starting point)


# ---- 7. ---------------------------------------------------------------------------------------------------------------------------------
def _c_call(scheme, cols, bands, lev, dirs, tan, y, out, ws):
    import torch

    from crt1d_amd import _lib

    ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    c, b = cols.c_struct(), bands.c_struct(cols.ncol)
    o = _lib.CrtOptions(0.501, 0, 0)
    nb = bands.nb
    ntan = next(iter(dirs.values())).shape[-2]
    D = _lib.CrtOpticsDirs(ntan, 0, *[ptr(dirs.get("d_" + n)) for n in PARAMS])
    obs = _lib.CrtSpecObs(*[ptr(y.get(k)) for k in KEYS], None, None, None, None)
    O = _lib.CrtSpecNormalOut(ptr(out["A"]), ptr(out["g"]), ptr(out["c2"]), None, None, None, None)
    arr = (ctypes.c_int32 * len(lev))(*lev)
    t = tan.c_struct()
    return _lib.load().crt_hip_spectral_normal_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), arr, len(lev),
                                                   ctypes.byref(D), 1, ctypes.byref(t), ctypes.byref(obs), ctypes.byref(O), ws.data_ptr(),
                                                   ws.numel(), torch.cuda.current_stream().cuda_stream), nb


def test_refusals_and_the_lds_limit():
    """n79, zq, 4s, zq_pa: CRT_ERR_UNSUPPORTED with a workspace that would do; one level past the LDS formula likewise, and nothing is
    written; the largest count that fits (2 keys x 26 levels x (5 + 1) = 312 rows) runs and passes the bound of 2."""
    import torch

    from crt1d_amd import _lib, batched, synth

    ncol, nb, nz = 3, 70, 30
    d = dict(synth.make_columns(ncol, nb, nz, seed=77, uniform_dlai=False))
    d["g_kind"] = np.full(ncol, ELLIPSOIDAL, dtype=np.int32)
    d["g_param"] = np.array([0.8, 1.3, 1.9])
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    rng = np.random.default_rng(2)
    dirs = {"d_" + n: _t(rng.uniform(-1.0, 1.0, (3, nb)) * d[n].mean(axis=0)) for n in PARAMS}
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    new = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    out = dict(A=new(ncol, 15), g=new(ncol, 5), c2=new(ncol))
    keys = ("I_df_d", "I_df_u")

    def obs(nsel):
        return {k: new(ncol, nsel, nb) for k in keys}

    for scheme in ("n79", "zq", "4s", "zq_pa"):
        assert _c_call(scheme, cols, bands, (0, nz - 1), dirs, tan, obs(2), out, ws)[0] == _lib.CRT_ERR_UNSUPPORTED
    assert _c_call("2s", cols, bands, tuple(range(27)), dirs, tan, obs(27), out, ws)[0] == _lib.CRT_ERR_UNSUPPORTED  # 324 rows
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in out.values())
    lev = tuple(range(26))  # 312 rows: 64-lane slices, two of them (35 + 35)
    X = batched.solve_levels("2s", cols, bands, lev, keys=keys)
    y = {k: (1.04 * X[k]).contiguous() for k in keys}
    plan = batched.SpectralNormalPlan("2s", cols, bands, lev, y, keys=keys, **dirs, lai=True, tangent=tan, fwd=True)
    got = plan()
    assert "slice=35 + k_spec_normal_finish" in plan.last_kernel()
    J = batched.solve_levels_jac("2s", cols, bands, lev)
    A = batched.solve_levels_dlai("2s", cols, bands, lev)
    B = batched.solve_levels_dleaf("2s", cols, bands, lev, tan)
    Jw, Ja, r = [], [], []
    for k in keys:
        t = sum(J[k][:, :, q, :, None] * dirs["d_" + n].T[None, None] for q, n in enumerate(PARAMS))
        ta = sum(J[k][:, :, q, :, None].abs() * dirs["d_" + n].T[None, None].abs() for q, n in enumerate(PARAMS))
        Jw.append(torch.cat([t, A[k][..., None], B[k][..., None]], dim=3).reshape(ncol, -1, 5))
        Ja.append(torch.cat([ta, A[k][..., None].abs(), B[k][..., None].abs()], dim=3).reshape(ncol, -1, 5))
        r.append((got["fwd"][k] - y[k]).reshape(ncol, -1))
    Jw, Ja, r = torch.cat(Jw, 1), torch.cat(Ja, 1), torch.cat(r, 1)
    g2 = 2 * _gamma(Jw.shape[1] + 9)
    assert _ratio(_dense(got["A"], 5), torch.einsum("coi,coj->cij", Jw, Jw), g2 * torch.einsum("coi,coj->cij", Ja, Ja)) <= 1
    assert _ratio(got["g"], torch.einsum("coi,co->ci", Jw, r), g2 * torch.einsum("coi,co->ci", Ja, r.abs())) <= 1
    assert _ratio(got["c2"], (r * r).sum(1), g2 * (r * r).sum(1)) <= 1
