"""An exact reference for the closed-form derivative kernels (2s, bl, g77, bf): complex-step differentiation through the NumPy oracle,
evaluated in extended precision (tests/test_deriv_reference_cpu.py pins it, tests/test_gpu_deriv_domain.py compares the kernels with it).

The oracle's closed forms are analytic in the leaf and soil optics and in the cumulative LAI, and with the dtype-preserving casts of
oracle/crt_oracle.py they run end to end on complex input.  For a real x and a step h far below the rounding of x,

    f(x + i h) = f(x) + i h f'(x) - h^2 f''(x) / 2 - ...,      Im f(x + i h) / h = f'(x) - h^2 f'''(x) / 6 + ...

With h = 1e-40 the h^2 term is 1e-80 of the value: it is below the last bit of any of the number formats used here, and no difference of
nearby values is formed, so there is no step-size error and no cancellation error.  What is left is the rounding of the evaluation
itself, and that is measured by evaluating twice: in complex128 (fp64 parts, the class of arithmetic the kernels use) and in clongdouble
(the 80-bit type of x86, 64-bit significand, eps = 2^-63 = 1.1e-19).

  * The reference is the clongdouble tangent, cast to float64.
  * The SPREAD |complex128 - clongdouble| is how far an fp64 evaluation of the same derivative, in the oracle's order of operations, is
    from it.  It is ~1e-15 of scale except next to the two removable singularities (2s: sigma -> 0; bf: k_d -> K_b), where the oracle
    divides through the singularity and the fp64 run loses what the division amplifies.
  * The clongdouble run loses the same amplification, from a rounding 2^-11 times as large (eps 2^-63 against 2^-52): the reference's own
    error is 2^-11 of the spread, 1/8192 of the term by which the bar is widened below.  That holds only if the extended run is extended
    throughout: the oracle's per-column K_b is widened before it meets mu_bar (``_columns``).  tests/test_deriv_reference_cpu.py (a)
    asserts it on every band, through two runs at different steps, with a factor 8 for two runs and for the spread being one sample.

n79 and zq are not served: the oracle's tridiagonal path allocates float64 arrays and drops the imaginary part.

The method needs a longdouble that is wider than a double.  Where it is not (eps > 2e-19) this module stops at import by an assertion:
a spread of zero would make every bar 1e-11 without the reference having earned it.
"""
import contextlib

import numpy as np

import domain_cases as D

assert np.finfo(np.longdouble).eps <= 2e-19, (
    "deriv_reference needs the 80-bit longdouble of x86 (eps 1.1e-19); this platform's longdouble has eps "
    f"{np.finfo(np.longdouble).eps:.3g}")

CLOSED = ("2s", "bl", "g77", "bf")
PARAMS = ("leaf_r", "leaf_t", "soil_r", "lai")
OPTICS = PARAMS[:3]
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
STEP = 1e-40
BASE_BAR = 1e-11  # the forward bar of tests/test_gpu_parity.py::test_hip_vs_oracle_synthetic


def _columns(oracle, rtype):
    """``oracle.Columns`` whose K_b() comes back in ``rtype`` (the same values: the float64 K_b, widened).  The oracle forms K_b per
    column in float64, and NumPy evaluates a product of two float64 operands in float64 whatever the spectra's type is.  2s forms
    sigma = (mu_bar K_b)^2 + c^2 - b^2 (_solve_2s.py:85) next to the factors b +- mu_bar K_b: with the square rounded to float64 the
    two are no longer the same function of mu_bar K_b by 1e-16, the removable singularity is no longer removed exactly, and the
    clongdouble tangent is off by ~1e-16 / sigma^2 -- 1.0e-8 at sigma = -2.9e-5 (band 60 of column 0 of the synthetic (3, 70, 60)
    uniform case; tests/test_deriv_reference_cpu.py (c) is the check that sees it).  With K_b widened, mu_bar K_b and its square are
    formed in ``rtype``, and the extended run is extended throughout.  For float64 nothing changes."""

    class Columns(oracle.Columns):
        def K_b(self):
            return super().K_b().astype(rtype)

    return Columns


def complex_step(oracle, d, scheme, param, ctype, step=STEP):
    """({key: tangent}, {key: primal}), each (ncol, nz, nb) over all levels in the real type of ``ctype`` (np.complex128 or
    np.clongdouble): the derivative of the oracle's ``scheme`` on the columns ``d`` (a ``synth.make_columns`` dict) with respect to
    ``param``, per band, and the real part of the same run.

    leaf_r, leaf_t, soil_r: the band's own value, x -> x + i step.  lai: the LAI scale s of tests/test_gpu_dlai.py, lai -> lai (1 + i
    step), the derivative LevelsDlaiPlan(per="log") returns.  bl has no soil: its soil_r slab is zero (and its primal is the plain run)."""
    assert scheme in CLOSED and param in PARAMS and ctype in (np.complex128, np.clongdouble), (scheme, param, ctype)
    rtype = np.float64 if ctype is np.complex128 else np.longdouble
    h = rtype(step)
    names = ("I_dr0", "I_df0", "leaf_r", "leaf_t") + (() if scheme == "bl" else ("soil_r",))
    kw = {k: np.asarray(d[k], dtype=np.float64).astype(ctype) for k in names}
    lai = np.asarray(d["lai"], dtype=np.float64).astype(ctype)
    dead = param not in names and param != "lai"
    if param == "lai":
        lai.imag = lai.real * h
    elif not dead:
        kw[param].imag = h
    cols = _columns(oracle, rtype)(d["psi"], lai, mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
    out = oracle.SOLVERS[scheme](cols, **kw)
    for k in KEYS:
        assert out[k].dtype == ctype, (scheme, k, out[k].dtype)  # the perturbation went through
    primal = {k: np.ascontiguousarray(out[k].real) for k in KEYS}
    if dead:
        return {k: np.zeros_like(primal[k]) for k in KEYS}, primal
    return {k: out[k].imag / h for k in KEYS}, primal


def reference(oracle, d, scheme, device_rules=True):
    """(J, spread, scale) for the columns ``d``:

    J        {param: {key: (ncol, nz, nb) float64}}: the clongdouble tangents, rounded to float64;
    spread   (ncol, 4, nb): max over levels and the four keys of |complex128 tangent - clongdouble tangent|, per parameter of PARAMS;
    scale    (ncol, 4, nb): max over levels and the four keys of |clongdouble tangent|.

    ``device_rules``: evaluated with the device's quadrature rules for mu_bar (2s) and tau_d (bl) in place of the oracle's
    (domain_cases.device_rules), which puts the comparison on the kernel's arithmetic as check A of tests/test_gpu_domain.py does.  The
    nodes and weights are real constants of either evaluation."""
    J, spread, scale = {}, [], []
    with (D.device_rules(oracle) if device_rules else contextlib.nullcontext()):
        for param in PARAMS:
            lo, _ = complex_step(oracle, d, scheme, param, np.complex128)
            hi, _ = complex_step(oracle, d, scheme, param, np.clongdouble)
            J[param] = {k: hi[k].astype(np.float64) for k in KEYS}
            spread.append(np.max([np.abs(lo[k] - hi[k]).max(axis=1) for k in KEYS], axis=0).astype(np.float64))
            scale.append(np.max([np.abs(hi[k]).max(axis=1) for k in KEYS], axis=0).astype(np.float64))
    return J, np.stack(spread, axis=1), np.stack(scale, axis=1)


def conditioning(d, scheme, scale):
    """(ncol, 4, nb): what is added to the bar of a parameter because of how the closed form is conditioned there, as a fraction of
    ``scale``, from the inputs and the reference's scale alone.  Zero but for the soil_r tangent of 2s:

        1e-14 (I_dr0 + I_df0) (1 + 1 / soil_r) / scale

    soil_r enters 2s through u1 = b - c / soil_r, u2 = b - c soil_r and u3 = f + c soil_r (_solve_2s.py:87) only, and every coefficient
    h2 .. h10 is a quotient whose numerator and denominator D1 or D2 carry the same u: h9 = (u2 + mu_bar h) / S1 / D2 with
    D2 = (u2 + mu_bar h) / S1 - (u2 - mu_bar h) S1 is 1 / (1 - (u2 - mu_bar h) / (u2 + mu_bar h) S1^2), S1 = e^{-h LAI}.  Its soil tangent is
    of size S1^2, but it is formed -- by the oracle's complex arithmetic and by the kernels' dual numbers alike -- as the difference of
    the two partial tangents n' / D2 and n D2' / D2^2, each of size |u'| / |u +- mu_bar h|: at most 1 for u2 and u3 (|u'| = c < b), at most
    1 / soil_r for u1 (|u1'| = c / soil_r^2 against |u1| ~ c / soil_r).  The difference keeps their rounding, eps (1 + 1 / soil_r), and the
    streams multiply it by I_dr0 or I_df0 and by e^{-h L} = 1 at the top: an absolute error of a few eps (I_dr0 + I_df0) (1 + 1 / soil_r) in
    a tangent whose scale is the light that reaches the ground and comes back, e^{-h LAI} of the incoming (and none of I_dr0 at a low
    sun).  1e-14, 45 eps, is the constant domain_cases.domain_bars gives the two removable singularities of the forward solve for the
    same reason: two fp64 evaluation orders of a cancelling closed form.

    Size of the term on the domain batch, as a fraction of scale, over the six cases 200 x (6, 12), (18, 12), (70, 60), uniform and ragged:
    total LAI <= 0.1 at most 4.8e-13; LAI 3 at most 1.6e-11 (200x70x60 ragged; <= 5.3e-12 in the other five); LAI 12 median 3e-11,
    maximum per case 1.8e-8 .. 8.3e-8 (the 8.3e-8 at 200x18x12 uniform; 2.9e-8 at 200x18x12 ragged, 4.4e-8 at 200x70x60 uniform).  So the
    bar stays tight up to LAI 3.  At LAI 12 it is an UPPER BOUND and not a tight one: it takes the worst of the partial tangents on
    every band, and under the lowest sun it is up to 2000 x the plain bar -- a relative error of 1e-8 in the soil tangent of such a
    column would pass.  (What the kernels show there is 9.8e-10 at the worst, tests/test_gpu_deriv_domain.py.)
    bl has no soil; in g77 and bf the soil term is a product, soil_r (...) e^{-k_d (LAI - L)}, and nothing cancels."""
    out = np.zeros_like(scale)
    if scheme == "2s":
        out[:, 2] = 1e-14 * (d["I_dr0"] + d["I_df0"]) * (1 + 1 / d["soil_r"]) / np.where(scale[:, 2] == 0, 1.0, scale[:, 2])
    return out


def tangent_bar(spread, scale, cond=0.0):
    """Allowed |J - J_ref| as a fraction of ``scale``, per (column, parameter, band): 1e-11 + 4 x spread / scale + ``cond``
    (``conditioning``).

    1e-11 is the bar the forward kernels are held to (test_hip_vs_oracle_synthetic).  4 x spread is the widening rule
    domain_cases.check_scheme uses for an uncertainty on the reference's side, here: how far two fp64-class evaluation orders of the same
    derivative may differ -- the oracle's own fp64 evaluation is ``spread`` away from the exact value, and a kernel that evaluates the
    same closed form in another order is allowed four times that.  The clongdouble reference's own error is 2^-11 of the spread (module
    docstring), so the bar is not the reference's noise.  Where scale is 0 (bl's soil_r slab) the bar is 1e-11 of nothing: the kernel's
    value must be exactly 0.  Nothing here is taken from a kernel's output."""
    return BASE_BAR + 4 * spread / np.where(scale == 0, 1.0, scale) + cond
