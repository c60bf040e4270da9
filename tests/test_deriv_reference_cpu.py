"""CPU: the complex-step reference of tests/deriv_reference.py is pinned here before any kernel is compared with it
(tests/test_gpu_deriv_domain.py).  No kernel runs in this file, and no figure below comes from one.

(a) Steps agree.  The tangents at steps 1e-40 and 1e-30 (clongdouble, rounded to float64: what ``reference`` returns) are compared on
    every (column, parameter, band) of a synthetic shape and of two domain batches.  A step-size error (the h^2 f''' / 6 term, 1e-60 of
    the value at the larger step) or an under- or overflow of the imaginary parts would show in every element, whatever its
    conditioning.  Two runs at different steps also differ by their ROUNDING (1e-30 / 1e-40 is no power of two, so the imaginary parts
    round differently), and that is the reference's own error.  Two assertions:
      every band of every scheme
                |t(1e-40) - t(1e-30)| <= 4 ulp x scale + 8 x 2^-11 x (4 x spread + conditioning x scale).
                The bracket is what tangent_bar is widened by: the fp64 rounding level of the closed form there, from the measured
                spread and from the derived soil term of 2s.  deriv_reference says the clongdouble run carries 2^-11 of that level; two
                runs make 2, and 4 more allow for the spread being one sample of the fp64 rounding (one evaluation's maximum over
                levels and keys), which can lie below the level it stands for.  This pins the claim the bar rests on: the reference's
                own error is at most 1/256 of the widening.  Measured: at most 0.25 of the bound for every scheme (that is the ulp
                term; in the rounding term the worst band is 2s soil_r at 200x70x60 uniform, 16.7 x (ulp + 2^-11 spread): its spread
                is a low sample, and the soil term carries it).
      where the form is well conditioned
                <= 4 ulp of float64 at the scale, the plain statement of the check.  The bands are chosen from the oracle's own
                quantities (domain_cases.singular_quantities) before the runs are compared: bl, g77 every band (measured <= 1.0 ulp);
                bf the bands with max(k_d, K_b) / |k_d - K_b| <= 32 (99 %; 0.98 ulp); 2s on the synthetic shape (3, 70, 60) the bands
                with max((mu_bar K_b)^2, b^2) / |sigma| <= 32 (94 %; 0.99 ulp).  2s on the domain batch has the first assertion only:
                with K_b LAI up to 477 its e^{+-h L} products cancel as well, and bands with that ratio below 32 differ by 340 ulp
                (8e-14 of scale).
    Over ALL bands the difference reaches bf 6.3 ulp; 2s 91 ulp on the synthetic shape, 3.3e5 ulp at 200x18x12 ragged and 1.2e9 ulp =
    2.6e-7 of scale at the one band of 200x70x60 uniform whose spread is 3.8e-4.
(b) Primal agrees.  The real part of the complex128 run is the plain oracle's solution within domain_cases.domain_bars (measured:
    <= 2e-12 of the profile maximum; bit-equal for most columns).
(c) Finite difference agrees.  On SHAPES of test_gpu_jac.py, uniform and ragged, the reference (plain rules) is within 1e-8 of scale of
    the Richardson references of test_gpu_jac.py and test_gpu_dlai.py: their own guard.  Those tests form two estimates, at h and at
    h / 2, and guard |estimate(h) - estimate(h / 2)| <= 1e-8; the reference is held to 1e-8 of both.  Measured, worst over the shapes,
    against the estimate at h / at h / 2: 2s 6.8e-9 / 8.6e-9 (both at (3, 70, 60) uniform, where the two estimates themselves differ by
    8.2e-9: the finite difference's rounding noise), bl 4.6e-9 / 2.9e-10, g77 5.7e-9 / 3.6e-10, bf 3.8e-9 / 5.2e-10 (bl, g77, bf: the
    h^4 truncation error of the coarser estimate, a sixteenth of it in the finer); the LAI scale 1.6e-9 / 3.0e-9 (2s), <= 1.1e-10 else.
    The comparison is sensitive to how the extended run treats the per-column constants: with K_b left in float64
    (deriv_reference._columns) the reference lies 1.0e-8 from both estimates at the band of (3, 70, 60) uniform with sigma = -2.9e-5.
(d) Conditions on the domain batch at (18, 12) and (70, 60), both profiles: every reference value finite; bl and g77 spread <= 1e-12 of
    scale; the share of (column, parameter, band) with 4 x spread > 1e-9 of scale <= 0.2 %.  Caps, not measurements.  Measured:

      spread / scale, worst    200x18x12 uniform   200x18x12 ragged   200x70x60 uniform   200x70x60 ragged    share 4 x spread > 1e-9
      2s                       7.4e-09             1.1e-07            3.8e-04             1.5e-07             <= 0.075 %
      bl                       6.4e-15             1.3e-14            1.8e-15             2.5e-15             0
      g77                      3.4e-13             3.6e-14            1.7e-13             1.7e-13             0
      bf                       8.1e-10             4.8e-08            1.7e-07             2.1e-07             <= 0.062 %

    (2s at 200x70x60 uniform: one band of one column -- sigma = 3e-13 there -- carries the 3.8e-4; the next is 2e-7.)
(e) Identities in the reference, to 1e-14 of scale: F' = I_dr' / mu + 2 (dn' + up') for all four parameters, I_dr' = -K_b L I_dr for the
    LAI scale and I_dr' = 0 for the optics.  Measured 4.2e-16 and 4.0e-16.
"""
import functools

import numpy as np
import pytest

import deriv_reference as R
import domain_cases as D

ULP = 2.0 ** -52
OWN_ERROR_MARGIN = 8  # (a): two runs x 4 for the spread being one sample; times 2^-11 of the bar's widening
DOMAIN_SHAPES = ((18, 12), (70, 60))


@functools.lru_cache(maxsize=None)
def _domain(nb, nz, uniform):
    return D.make_domain_columns(nb, nz, uniform)


@functools.lru_cache(maxsize=None)
def _domain_reference(scheme, nb, nz, uniform):
    from oracle import crt_oracle

    return R.reference(crt_oracle, _domain(nb, nz, uniform), scheme)


def _domain_cases():
    for scheme in R.CLOSED:
        for nb, nz in DOMAIN_SHAPES:
            for uniform in (True, False):
                yield pytest.param(scheme, nb, nz, uniform, id=f"{scheme}-200x{nb}x{nz}-{'uniform' if uniform else 'ragged'}")


def _den(scale):
    return np.where(scale == 0, 1.0, scale)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
def _well_conditioned(oracle, d, scheme):
    """(ncol, nb) bool, from the oracle's quantities alone (domain_cases.singular_quantities, what domain_bars is made of): the ratio of
    the largest term of the cancelling difference to the difference is at most 32."""
    q = D.singular_quantities(oracle, d)
    if scheme == "2s":
        return np.maximum(q["mbK"] ** 2, q["b"] ** 2) <= 32 * np.abs(q["sigma"])
    if scheme == "bf":
        return np.maximum(q["k_d"], q["Kb"]) <= 32 * np.abs(q["k_d"] - q["Kb"])
    return np.ones(q["om"].shape, dtype=bool)


@pytest.mark.parametrize("scheme", R.CLOSED)
def test_steps_agree(oracle, scheme):
    from crt1d_amd import synth

    batches = [("synth 3x70x60 ragged", dict(synth.make_columns(3, 70, 60, seed=11, uniform_dlai=False)), True),
               ("domain 200x18x12 ragged", _domain(18, 12, False), scheme != "2s"),
               ("domain 200x70x60 uniform", _domain(70, 60, True), scheme != "2s")]
    for name, d, plain in batches:
        good = _well_conditioned(oracle, d, scheme)
        assert good.mean() >= 0.9, (scheme, name, good.mean())
        with D.device_rules(oracle):
            for p, param in enumerate(R.PARAMS):
                lo, _ = R.complex_step(oracle, d, scheme, param, np.complex128)
                a, _ = R.complex_step(oracle, d, scheme, param, np.clongdouble, 1e-40)
                b, _ = R.complex_step(oracle, d, scheme, param, np.clongdouble, 1e-30)
                scale = np.max([np.abs(a[k]).max(axis=1) for k in R.KEYS], axis=0).astype(np.float64)
                spread = np.max([np.abs(lo[k] - a[k]).max(axis=1) for k in R.KEYS], axis=0).astype(np.float64)
                diff = np.max([np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max(axis=1) for k in R.KEYS], axis=0)
                if scheme == "bl" and param == "soil_r":
                    assert not diff.any() and not scale.any()
                    continue
                ulps = diff / (ULP * _den(scale))
                cond = R.conditioning(d, scheme, np.repeat(scale[:, None], 4, axis=1))[:, p]  # (this parameter's slab)
                widening = (R.tangent_bar(spread, scale, cond) - R.BASE_BAR) * scale  # 4 x spread + cond x scale
                bound = 4 * ULP * scale + OWN_ERROR_MARGIN * 2.0 ** -11 * widening
                print(f"steps {scheme} {param} {name}: {100 * good.mean():.1f} % well conditioned, worst {ulps[good].max():.3f} ulp"
                      f"{'' if plain else ' (4 ulp not asserted)'}; all bands: {ulps.max():.3g} ulp, "
                      f"{float((diff / bound).max()):.2f} of the bound")
                assert np.all(diff <= bound), (scheme, param, name, float((diff / bound).max()))  # every band of every scheme
                if plain:
                    assert np.all(ulps[good] <= 4), (scheme, param, name, float(ulps[good].max()))


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,nb,nz,uniform", _domain_cases())
def test_primal_is_the_oracle(oracle, scheme, nb, nz, uniform):
    d = _domain(nb, nz, uniform)
    ref = D.oracle_solve(oracle, d, scheme)
    bars = D.domain_bars(oracle, d, uniform)
    for param in R.PARAMS:
        _, primal = R.complex_step(oracle, d, scheme, param, np.complex128)
        tally = {}
        fails = D.check_scheme(scheme, primal, ref, bars, tally=tally)
        print(f"primal {scheme} {param} 200x{nb}x{nz}: " + "  ".join(f"{k} {e:.1e} [{r:.2f}]" for k, (e, r) in tally.items()))
        assert not fails, (param, fails[:4])


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
def _fd_cases():
    from test_gpu_jac import SHAPES

    for scheme in R.CLOSED:
        for shape in SHAPES:
            for uniform in (True, False):
                yield pytest.param(scheme, shape, uniform, id=f"{scheme}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}")


@pytest.mark.parametrize("scheme,shape,uniform", _fd_cases())
def test_finite_difference_agrees(oracle, scheme, shape, uniform):
    import test_gpu_dlai
    import test_gpu_jac

    d = test_gpu_jac._host(shape, uniform)
    lev = list(test_gpu_jac._levels(shape[2]))
    J, _, _ = R.reference(oracle, d, scheme, device_rules=False)
    Jh, Jfd, scale = test_gpu_jac._reference(scheme, shape, uniform)  # {key: (ncol, nsel, 3, nb)} at h and at h / 2, (ncol, 1, 3, nb)
    worst = coarse = 0.0
    for k in test_gpu_jac.KEYS:
        for p, param in enumerate(R.OPTICS):
            err = np.abs(J[param][k][:, lev] - Jfd[k][:, :, p])
            worst = max(worst, float((err / _den(scale[:, :, p])).max()))
            coarse = max(coarse, float((np.abs(J[param][k][:, lev] - Jh[k][:, :, p]) / _den(scale[:, :, p])).max()))
            assert np.all(err <= 1e-8 * scale[:, :, p]), (scheme, shape, k, param, worst)
            assert np.all(np.abs(J[param][k][:, lev] - Jh[k][:, :, p]) <= 1e-8 * scale[:, :, p]), (scheme, shape, k, param, coarse)
    for param in R.OPTICS:
        assert not J[param]["I_dr"].any()  # (the finite-difference reference of test_gpu_jac.py has no I_dr slab: it is zero)
    Lh, Lfd, lscale = test_gpu_dlai._reference(scheme, shape, uniform)  # {key: (ncol, nsel, nb)}, (ncol, 1, nb)
    worst_l = coarse_l = 0.0
    for k in R.KEYS:
        err = np.abs(J["lai"][k][:, lev] - Lfd[k])
        worst_l = max(worst_l, float((err / _den(lscale)).max()))
        coarse_l = max(coarse_l, float((np.abs(J["lai"][k][:, lev] - Lh[k]) / _den(lscale)).max()))
        assert np.all(err <= 1e-8 * lscale), (scheme, shape, k, "lai", worst_l)
        assert np.all(np.abs(J["lai"][k][:, lev] - Lh[k]) <= 1e-8 * lscale), (scheme, shape, k, "lai", coarse_l)
    print(f"complex step vs Richardson {scheme} {shape} {'uniform' if uniform else 'ragged'}: optics {worst:.2e} (at h: {coarse:.2e}), "
          f"lai {worst_l:.2e} (at h: {coarse_l:.2e}) of scale")


# ---- (d), (e) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,nb,nz,uniform", _domain_cases())
def test_conditions_and_identities_on_the_domain(oracle, scheme, nb, nz, uniform):
    d = _domain(nb, nz, uniform)
    J, spread, scale = _domain_reference(scheme, nb, nz, uniform)
    for param in R.PARAMS:
        for k in R.KEYS:
            assert np.all(np.isfinite(J[param][k])), (param, k, np.argwhere(~np.isfinite(J[param][k]))[:3])
    assert np.all(np.isfinite(spread)) and np.all(np.isfinite(scale))
    rel = spread / _den(scale)
    share = float(np.mean(4 * rel > 1e-9))
    print(f"reference {scheme} 200x{nb}x{nz} {'uniform' if uniform else 'ragged'}: worst spread / scale {rel.max():.2e} "
          f"({', '.join(f'{n} {rel[:, i].max():.1e}' for i, n in enumerate(R.PARAMS))}); 4 x spread > 1e-9: {100 * share:.3f} %, > 1e-8: "
          f"{100 * float(np.mean(4 * rel > 1e-8)):.3f} %")
    if scheme in ("bl", "g77"):
        assert rel.max() <= 1e-12, rel.max()
    assert share <= 0.002, share
    bar = R.tangent_bar(spread, scale, R.conditioning(d, scheme, scale))
    assert bar.shape == (D.NCOL, 4, nb) and np.all(bar >= R.BASE_BAR) and np.all(np.isfinite(bar))
    # (e)
    mu = np.cos(d["psi"])[:, None, None]
    worst = 0.0
    for p, param in enumerate(R.PARAMS):
        t = J[param]
        resid = np.abs(t["F"] - (t["I_dr"] / mu + 2 * (t["I_df_d"] + t["I_df_u"])))
        worst = max(worst, float((resid / _den(scale[:, p])[:, None, :]).max()))
        assert np.all(resid <= 1e-14 * scale[:, p][:, None, :]), (param, worst)
        if param != "lai":
            assert not t["I_dr"].any()
    oc = oracle.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
    exact = -(oc.K_b()[:, None] * d["lai"])[:, :, None] * D.oracle_solve(oracle, d, scheme)["I_dr"]
    resid = np.abs(J["lai"]["I_dr"] - exact)
    print(f"reference identities {scheme}: F' {worst:.1e}, I_dr' {float((resid / scale[:, 3][:, None, :]).max()):.1e} of scale")
    assert np.all(resid <= 1e-14 * scale[:, 3][:, None, :])
