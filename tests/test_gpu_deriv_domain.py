"""GPU: the closed-form derivative kernels (2s, bl, g77, bf) on the whole supported input domain (tests/domain_cases.py: ten leaf-angle
classes x sun zenith 0.05 .. 89 degrees x total LAI 0.01 .. 12 = 200 columns) against an exact reference: complex-step differentiation
through the NumPy oracle in extended precision (tests/deriv_reference.py, pinned by tests/test_deriv_reference_cpu.py), evaluated with
the device's quadrature rules as check A of tests/test_gpu_domain.py is.

1. Values.  LevelsJacPlan (k_jac) and LevelsDlaiPlan (k_dlai), every level, at 200 x (6, 12), (18, 12), (70, 60), uniform and ragged:
       |J - J_ref| <= tangent_bar x scale      elementwise,
   tangent_bar = 1e-11 + 4 x spread / scale per (column, parameter, band), scale = max |J_ref| over the levels and the four quantities,
   spread = |complex128 - clongdouble| of the reference (deriv_reference.tangent_bar: the forward kernels' 1e-11 plus the widening
   rule of domain_cases.check_scheme for how far two fp64 evaluation orders of the same derivative may differ); for the soil_r tangent
   of 2s plus 1e-14 (I_dr0 + I_df0) (1 + 1 / soil_r) / scale (deriv_reference.conditioning: the cancellation of the partial soil
   tangents under a dense canopy).  No bar comes from a kernel's output.
2. The identity F' = I_dr' / mu + 2 (dn' + up') of the kernels' own outputs at 1e-11 of the reference's scale, on the same batch.
3. The separately written code paths at 200 x (18, 12) ragged, against the reference contracted in np.longdouble:
   LevelsGradPlan (k_grad keeps its own staging) with one random weight set over the four quantities and all levels, gradient with
   respect to the three optics and the LAI scale; SensorJacPlan (sens_jac_body keeps its own pass loops) with three sensor bands, the
   three unit directions and lai=True.  Bound of an output element that is a sum over the rows o of weight_o x tangent_o:
       sum_o |weight_o| tangent_bar_o scale_o  +  2 gamma_n sum_o |weight_o| |tangent_o|,      gamma_n = n U / (1 - n U), U = 2^-53,
   the first term the bar of 1. carried through the sum, the second the summation term as tests/test_gpu_specfit.py derives it: one
   rounding for a product and n - 1 for n terms summed in any order, doubled for the higher-order terms (n = the rows of the sum; for
   a direction column three products and two sums per row, 3 n + 1: tests/test_gpu_sensjac.py).
4. SpectralNormalPlan (k_spec_normal) at 200 x (18, 12) and 200 x (300, 12) ragged -- 300 bands take two band slices and
   k_spec_normal_finish --, four keys, levels (0, nz - 1), the three unit directions and lai=True, inv_sigma as
   test_gpu_specfit._observations builds it (the last key has none).
   fwd against the ORACLE's primal at domain_cases.domain_bars (2s, bf, or base for bl and g77): profile error <= bar and elementwise
   error <= 100 x bar, the two assertions of domain_cases.check_scheme.  (tests/test_gpu_specfit.py compares fwd with LevelsPlan at a
   bar measured from the kernel; this is the check against something that is not a kernel.)
   A, g, c2 against J_ref^T W J_ref, J_ref^T W r_ref and sum r_ref^2 formed in np.longdouble from the reference.  With w_o,i = t_o,i s_o the
   weighted tangent of row o = (key, level, band) and r_o = (X_o - y_o) s_o, a kernel whose tangents are within delta_o,i = tangent_bar
   scale |s_o| of the reference's and whose residual is within rho_o = (fwd bar) (profile maximum) |s_o| forms
       (w_i + e_i) (w_j + e_j) - w_i w_j = e_i w_j + w_i e_j + e_i e_j,      |e_i| <= delta_i,
   so  |A_ij - ref| <= sum_o (delta_i |w_j| + |w_i| delta_j + delta_i delta_j) + 2 gamma_{n + 9} sum_o |w_i| |w_j|,
       |g_i - ref|  <= sum_o (delta_i |r| + |w_i| rho + delta_i rho)           + 2 gamma_{n + 9} sum_o |w_i| |r|,
       |c2 - ref|   <= sum_o (2 |r| rho + rho^2)                               + 2 gamma_{n + 9} sum_o r^2,
   the last term of each line the existing derivation of tests/test_gpu_specfit.py (9 roundings on a term, n rows).

Measured on MI355X (pytest -s prints every case).  1.: worst |J - J_ref| / scale over the six cases, in brackets the largest error / bar:

  scheme   leaf_r            leaf_t            soil_r            LAI scale
  2s       1.4e-07 [0.14]    3.8e-07 [0.14]    9.8e-10 [0.52]    9.1e-14 [0.01]
  bl       1.3e-14 [0.00]    1.3e-14 [0.00]    0 (no soil)       1.4e-15 [0.00]
  g77      3.7e-14 [0.00]    3.7e-14 [0.00]    3.4e-13 [0.03]    1.2e-14 [0.00]
  bf       1.1e-10 [0.02]    9.1e-11 [0.02]    2.1e-15 [0.00]    5.6e-14 [0.01]

  (2s leaf_r, leaf_t: the 1e-7 are the one band of 200x70x60 uniform with sigma = 3e-13, where the reference's spread is 3.8e-4 and the
  bar 1.5e-3; 8.0e-11 on the other five cases.  bf: the bands with k_d next to K_b.  Away from the two singularities every kernel is
  within 1e-12.)
  2s soil_r is the one place where 1e-11 + 4 x spread / scale alone does not hold: 2.3e-10 .. 9.8e-10 of scale, 11 .. 50 x that bar, in
  the columns of total LAI 12 with the sun at 75 degrees from the zenith or lower, in all six cases.  k_jac forms the soil tangent
  as the oracle does, as a difference of partial tangents 1 / soil_r times larger than the result; deriv_reference.conditioning derives the term from the inputs and the
  reference's scale, and with it the worst case sits at 0.52 of the bar.
2.: F' = I_dr' / mu + 2 (dn' + up') to 2.6e-16 of scale in every case.
3.: error / bound  k_grad <= 0.01 for every scheme and parameter;  k_sens_jac 2s 0.22 (F), 0.11 (I_df_u), <= 0.01 else and for bl, g77, bf.
4.: fwd against the oracle, worst profile error [error / bar]: 2s 2.2e-12 [0.11] (300 bands), bl 9.5e-14 [0.01], g77 1.1e-13 [0.01],
    bf 1.6e-12 [0.06]; error / bound of A 0.027, g 0.006 (2s, 18 bands), c2 < 0.001; bl, g77, bf < 0.001.
"""
import functools

import numpy as np
import pytest

import deriv_reference as R
import domain_cases as D
from test_gpu_domain import _case

pytestmark = pytest.mark.gpu

SCHEMES = R.CLOSED
SHAPES = ((6, 12), (18, 12), (70, 60))  # (nb, nz): those of tests/test_gpu_domain.py; nz <= 64, so one call serves every level
JAC_KEYS = ("I_df_d", "I_df_u", "F")
U = 2.0 ** -53
LD = np.longdouble


def _gamma(k):
    return k * U / (1 - k * U)


@functools.lru_cache(maxsize=None)
def _ref(scheme, nb, nz, uniform):
    """(J, spread, scale, bar) of deriv_reference on the domain batch, built once per (scheme, shape, profile) and left unchanged."""
    from oracle import crt_oracle

    d = _case(nb, nz, uniform)[0]
    J, spread, scale = R.reference(crt_oracle, d, scheme)
    for p in R.PARAMS:
        for k in R.KEYS:
            assert np.all(np.isfinite(J[p][k])), (scheme, p, k)  # no column is dropped below
            J[p][k].setflags(write=False)
    return J, spread, scale, R.tangent_bar(spread, scale, R.conditioning(d, scheme, scale))


@functools.lru_cache(maxsize=None)
def _kernels(scheme, nb, nz, uniform):
    """The two derivative plans at every level, on the host: ({key: (ncol, nz, 3, nb)}, {key: (ncol, nz, nb)}, kernel names)."""
    from crt1d_amd import batched

    _, cols, bands, _ = _case(nb, nz, uniform)
    lev = tuple(range(nz))
    jp = batched.LevelsJacPlan(scheme, cols, bands, lev)
    jac = {k: v.cpu().numpy() for k, v in jp().items()}
    jname = jp.last_kernel()
    lp = batched.LevelsDlaiPlan(scheme, cols, bands, lev)
    dlai = {k: v.cpu().numpy() for k, v in lp().items()}
    return jac, dlai, (jname, lp.last_kernel())


def _where(d, cols):
    """Class, zenith and LAI of the columns ``cols``, as tests/test_gpu_domain.py names a failure."""
    return [(D.CLASS_NAMES[d["cls"][c]], D.PSI_DEG[d["ipsi"][c]], D.LAI_TOT[d["ilai"][c]]) for c in cols]


def _tag(scheme, nb, nz, uniform):
    return f"{scheme} 200x{nb}x{nz} {'uniform' if uniform else 'ragged'}"


def _cases():
    for scheme in SCHEMES:
        for nb, nz in SHAPES:
            for uniform in (True, False):
                yield pytest.param(scheme, nb, nz, uniform, id=f"{scheme}-200x{nb}x{nz}-{'uniform' if uniform else 'ragged'}")


# ---- 1. -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,nb,nz,uniform", _cases())
def test_tangents_against_the_reference(scheme, nb, nz, uniform):
    d = _case(nb, nz, uniform)[0]
    J, spread, scale, bar = _ref(scheme, nb, nz, uniform)
    jac, dlai, names = _kernels(scheme, nb, nz, uniform)
    assert names[0].startswith("k_jac<") and names[1].startswith("k_dlai<"), names
    fails, line = [], []
    for p, param in enumerate(R.PARAMS):
        tol = (bar[:, p] * scale[:, p])[:, None, :]  # (ncol, 1, nb)
        den = np.where(scale[:, p] == 0, 1.0, scale[:, p])[:, None, :]
        worst = ratio = 0.0
        for k in (R.KEYS if param == "lai" else JAC_KEYS):
            g = dlai[k] if param == "lai" else jac[k][:, :, p]
            assert g.shape == J[param][k].shape == (D.NCOL, nz, nb) and np.all(np.isfinite(g)), (param, k)
            err = np.abs(g - J[param][k])
            worst = max(worst, float((err / den).max()))
            ratio = max(ratio, float((err / np.where(tol == 0, 1.0, tol)).max()))
            bad = np.unique(np.argwhere(err > tol)[:, 0])
            if bad.size:
                fails.append((param, k, f"{float((err / np.where(tol == 0, 1.0, tol)).max()):.2f} x bar", _where(d, bad[:6])))
        line.append(f"{param} {worst:.1e} [{ratio:.2f}]")
    print(f"\nderiv {_tag(scheme, nb, nz, uniform)}: " + "  ".join(line) + f"   (worst bar {bar.max():.1e})")
    assert not fails, fails


# ---- 2. -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,nb,nz,uniform", _cases())
def test_flux_identity(scheme, nb, nz, uniform):
    d = _case(nb, nz, uniform)[0]
    scale = _ref(scheme, nb, nz, uniform)[2]
    jac, dlai, _ = _kernels(scheme, nb, nz, uniform)
    mu = np.cos(d["psi"])[:, None, None]
    worst = 0.0
    for p, param in enumerate(R.PARAMS):
        if param == "lai":
            resid = np.abs(dlai["F"] - (dlai["I_dr"] / mu + 2 * (dlai["I_df_d"] + dlai["I_df_u"])))
        else:
            resid = np.abs(jac["F"][:, :, p] - 2 * (jac["I_df_d"][:, :, p] + jac["I_df_u"][:, :, p]))
        sc = scale[:, p][:, None, :]
        worst = max(worst, float((resid / np.where(sc == 0, 1.0, sc)).max()))
        bad = np.unique(np.argwhere(resid > 1e-11 * sc)[:, 0])
        assert not bad.size, (param, worst, _where(d, bad[:6]))
    print(f"\nderiv identity {_tag(scheme, nb, nz, uniform)}: {worst:.1e} of scale")


# ---- 3. -----------------------------------------------------------------------------------------------------------------------------------
def _check(name, d, got, ref, bound, tally):
    """Every element of ``got`` within ``bound`` of ``ref`` (np.longdouble); a failure names the columns."""
    err = np.abs(got.astype(LD) - ref)
    assert got.shape == ref.shape == bound.shape and np.all(np.isfinite(got)), name
    tally[name] = float((err / np.where(bound == 0, 1, bound)).max())
    bad = np.unique(np.argwhere(err > bound)[:, 0])
    assert not bad.size, (name, f"{tally[name]:.2f} x bound", _where(d, bad[:6]))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_gradient_kernel(scheme):
    import torch

    from crt1d_amd import batched

    nb, nz, uniform = 18, 12, False
    d, cols, bands, _ = _case(nb, nz, uniform)
    J, _, scale, bar = _ref(scheme, nb, nz, uniform)
    rng = np.random.default_rng(17)
    w = {k: rng.uniform(-1.0, 1.0, (D.NCOL, nz, nb)) for k in R.KEYS}
    plan = batched.LevelsGradPlan(scheme, cols, bands, tuple(range(nz)), {k: torch.as_tensor(v).to(cols.device) for k, v in w.items()},
                                  wrt=("leaf_r", "leaf_t", "soil_r", "lai"))
    got = {k: v.cpu().numpy() for k, v in plan().items()}
    assert plan.last_kernel().startswith(f"k_grad<{scheme}>"), plan.last_kernel()
    tally = {}
    for p, param in enumerate(R.PARAMS):
        ref = sum(w[k].astype(LD) * J[param][k].astype(LD) for k in R.KEYS)  # (ncol, nz, nb)
        mag = sum(np.abs(w[k]).astype(LD) * np.abs(J[param][k]).astype(LD) for k in R.KEYS)
        carried = sum(np.abs(w[k]).astype(LD) for k in R.KEYS) * (bar[:, p] * scale[:, p]).astype(LD)[:, None, :]
        if param == "lai":
            n = len(R.KEYS) * nz * nb
            _check(param, d, got[param], ref.sum((1, 2)), carried.sum((1, 2)) + 2 * _gamma(n) * mag.sum((1, 2)), tally)
        else:
            n = len(R.KEYS) * nz
            _check(param, d, got[param], ref.sum(1), carried.sum(1) + 2 * _gamma(n) * mag.sum(1), tally)
    print(f"\nderiv grad {_tag(scheme, nb, nz, uniform)}: error / bound " + "  ".join(f"{k} {v:.2f}" for k, v in tally.items()))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sensor_jacobian_kernel(scheme):
    import torch

    from crt1d_amd import batched

    nb, nz, uniform = 18, 12, False
    d, cols, bands, _ = _case(nb, nz, uniform)
    J, _, scale, bar = _ref(scheme, nb, nz, uniform)
    first, count = np.array([0, nb // 3, nb // 4]), np.array([nb, 1, nb // 2])  # all bands | one band | an inner support
    sensors = batched.SensorSet.from_supports(first, count, np.random.default_rng(29).uniform(-1.0, 1.0, int(count.sum())), nb=nb)
    W = sensors.dense(nb).astype(LD)  # (nsens, nb)
    eye = np.eye(3)
    dirs = {"d_" + n: torch.as_tensor(np.ascontiguousarray(np.broadcast_to(eye[:, p, None], (3, nb)))).to(cols.device)
            for p, n in enumerate(R.OPTICS)}  # direction j = one unit of R.OPTICS[j] in every band
    plan = batched.SensorJacPlan(scheme, cols, bands, tuple(range(nz)), sensors, lai=True, **dirs)
    got = {k: v.cpu().numpy() for k, v in plan().items()}
    assert plan.params == ("dir0", "dir1", "dir2", "lai") and plan.last_kernel().startswith(f"k_sens_jac<{scheme}>"), plan.last_kernel()
    ncount = np.asarray(count, dtype=LD)[None, None, :]
    tally = {}
    for k in R.KEYS:
        ref, bound = [], []
        for p, param in enumerate(R.PARAMS):
            t = J[param][k].astype(LD)
            n = ncount if param == "lai" else 3 * ncount + 1
            ref.append(np.einsum("crb,sb->crs", t, W))
            bound.append(np.einsum("cb,sb->cs", (bar[:, p] * scale[:, p]).astype(LD), np.abs(W))[:, None, :]
                         + 2 * _gamma(n) * np.einsum("crb,sb->crs", np.abs(t), np.abs(W)))
        _check(k, d, got[k], np.stack(ref, axis=-1), np.stack(bound, axis=-1), tally)
    print(f"\nderiv sensjac {_tag(scheme, nb, nz, uniform)}: error / bound " + "  ".join(f"{k} {v:.2f}" for k, v in tally.items()))


# ---- 4. -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [18, 300])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_spectral_normal_equations(oracle, scheme, nb):
    import torch

    from crt1d_amd import batched

    nz, uniform = 12, False
    d, cols, bands, bars = _case(nb, nz, uniform)
    J, _, scale, bar = _ref(scheme, nb, nz, uniform)
    lev, keys = [0, nz - 1], R.KEYS
    with D.device_rules(oracle):
        full = D.oracle_solve(oracle, d, scheme)
    fbar = np.broadcast_to(bars[scheme] if scheme in ("2s", "bf") else bars["base"], (D.NCOL, nb))
    rng = np.random.default_rng(3 * nb + 11)
    X, y, s, prof = {}, {}, {}, {}
    for i, k in enumerate(keys):  # the observations of test_gpu_specfit._observations, from the oracle's spectra
        X[k] = full[k][:, lev]
        prof[k] = np.abs(full[k]).max(axis=1)  # (ncol, nb): the profile maximum the forward bars refer to
        y[k] = X[k] * (1 + 0.05 * rng.normal(size=X[k].shape)) + 0.01 * np.abs(X[k]).max()
        s[k] = rng.uniform(0.5, 2.0, X[k].shape) / max(np.abs(X[k]).mean(), 1e-3) if i + 1 < len(keys) else None
    eye = np.eye(3)
    dirs = {"d_" + n: torch.as_tensor(np.ascontiguousarray(np.broadcast_to(eye[:, p, None], (3, nb)))).to(cols.device)
            for p, n in enumerate(R.OPTICS)}
    plan = batched.SpectralNormalPlan(scheme, cols, bands, tuple(lev), y, keys=keys, inv_sigma={k: v for k, v in s.items() if v is not None},
                                      lai=True, fwd=True, **dirs)
    out = plan()
    torch.cuda.synchronize()
    assert plan.params == ("dir0", "dir1", "dir2", "lai")
    assert "k_spec_normal" in plan.last_kernel() and ("k_spec_normal_finish" in plan.last_kernel()) == (nb == 300), plan.last_kernel()
    # fwd against the oracle
    worst_f = ratio_f = 0.0
    for k in keys:
        g = out["fwd"][k].cpu().numpy()
        assert g.shape == X[k].shape and np.all(np.isfinite(g)), k
        sc = np.where(prof[k] == 0, 1.0, prof[k])[:, None, :]
        err = np.abs(g - X[k])
        ratio = np.maximum(err / sc / fbar[:, None, :], err / np.maximum(np.abs(X[k]), 1e-9 * sc) / (100 * fbar[:, None, :]))
        worst_f, ratio_f = max(worst_f, float((err / sc).max())), max(ratio_f, float(ratio.max()))
        bad = np.unique(np.argwhere(ratio > 1)[:, 0])
        assert not bad.size, ("fwd", k, f"{float(ratio.max()):.2f} x bar", _where(d, bad[:6]))
    # A, g, c2 against the reference
    Wt, Dl, Rr, Rho = [], [], [], []
    for k in keys:
        sk = (np.ones_like(X[k]) if s[k] is None else s[k]).astype(LD)  # (ncol, 2, nb)
        t = np.stack([J[p][k][:, lev].astype(LD) for p in R.PARAMS], axis=-1)  # (ncol, 2, nb, 4)
        dl = np.stack([(bar[:, p] * scale[:, p]).astype(LD)[:, None, :] * np.abs(sk) for p in range(4)], axis=-1)
        Wt.append((t * sk[..., None]).reshape(D.NCOL, -1, 4))
        Dl.append(dl.reshape(D.NCOL, -1, 4))
        Rr.append(((X[k].astype(LD) - y[k].astype(LD)) * sk).reshape(D.NCOL, -1))
        Rho.append(((fbar * prof[k]).astype(LD)[:, None, :] * np.abs(sk)).reshape(D.NCOL, -1))
    Wt, Dl, Rr, Rho = (np.concatenate(v, axis=1) for v in (Wt, Dl, Rr, Rho))
    Wa, Ra = np.abs(Wt), np.abs(Rr)
    g2 = 2 * _gamma(Wt.shape[1] + 9)
    e = lambda spec, *a: np.einsum(spec, *a)  # noqa: E731
    ref = (e("coi,coj->cij", Wt, Wt), e("coi,co->ci", Wt, Rr), (Rr * Rr).sum(1))
    bound = (e("coi,coj->cij", Dl, Wa) + e("coi,coj->cij", Wa, Dl) + e("coi,coj->cij", Dl, Dl) + g2 * e("coi,coj->cij", Wa, Wa),
             e("coi,co->ci", Dl, Ra) + e("coi,co->ci", Wa, Rho) + e("coi,co->ci", Dl, Rho) + g2 * e("coi,co->ci", Wa, Ra),
             (2 * Ra * Rho + Rho * Rho).sum(1) + g2 * (Rr * Rr).sum(1))
    tally = {}
    got = (plan.dense().cpu().numpy(), out["g"].cpu().numpy(), out["c2"].cpu().numpy())
    for name, g, r, b in zip(("A", "g", "c2"), got, ref, bound):
        _check(name, d, g, r, b, tally)
    print(f"\nderiv specfit {_tag(scheme, nb, nz, uniform)}: fwd {worst_f:.1e} [{ratio_f:.2f}]; error / bound "
          + "  ".join(f"{k} {v:.3f}" for k, v in tally.items()) + f"; {plan.last_kernel()}")
