"""The supported input domain of the parity tests, in one place (tests/test_quadrature_domain_cpu.py, tests/test_gpu_domain.py).

``synth.make_columns`` draws ellipsoidal-approx leaves (mla 20-80 degrees), sun zenith 0-75 degrees and total LAI 0.5-8 only.  The batch
built here is the full product of

  CLASSES   ten leaf-angle classes: every closed-form kind of include/crt1d_hip.h, the parameterised ones at both ends of their range
  PSI_DEG   sun zenith from 0.05 degrees (K_b down to 5.6e-4 for vertical leaves) to 89 degrees (1 degree elevation, K_b up to 39.8)
  LAI_TOT   total LAI from 0.01 to 12 (K_b LAI up to 477)

= 200 columns, ordered with the class index fastest so that every workgroup that packs several columns holds several kinds.

Excluded on purpose -- the NumPy oracle itself is not finite there, so there is nothing to compare with:

  * psi = 0 with vertical leaves: G = 0, K_b = 0, and the closed forms of 2s (mu_bar K_b in a denominator) and n79 (1 / (fsha dlai) with
    fsha = 0) divide by zero;
  * psi > 89 degrees: at 89.9 degrees n79's 1 / (fsun dlai) overflows from LAI = 3 on (fsun = e^{-K_b laim} underflows);
  * LAI > 12: the same overflow sets in at 89 degrees (checked at 20).

Inside the product every column is finite in every output of all eight schemes (asserted by tests/test_gpu_domain.py before any
comparison).  Negative values do occur (2s, n79, g77 at K_b LAI >> 1); they are a property of the schemes and are not asserted on.
"""
import contextlib

import numpy as np

# kind ids of include/crt1d_hip.h
HORIZONTAL, SPHERICAL, VERTICAL, ELLIPSOIDAL, ELLIPSOIDAL_APPROX, BONAN = range(6)

# (name, g_kind, g_param)
CLASSES = (
    ("horizontal", HORIZONTAL, 0.0),
    ("spherical", SPHERICAL, 0.0),
    ("vertical", VERTICAL, 0.0),
    ("ellipsoidal_x0.2", ELLIPSOIDAL, 0.2),
    ("ellipsoidal_x1", ELLIPSOIDAL, 1.0),
    ("ellipsoidal_x10", ELLIPSOIDAL, 10.0),
    ("approx_x0.2", ELLIPSOIDAL_APPROX, 0.2),
    ("approx_x10", ELLIPSOIDAL_APPROX, 10.0),
    ("bonan_-0.4", BONAN, -0.4),
    ("bonan_0.6", BONAN, 0.6),
)
CLASS_NAMES = tuple(c[0] for c in CLASSES)
PSI_DEG = (0.05, 30.0, 75.0, 85.0, 89.0)
LAI_TOT = (0.01, 0.1, 3.0, 12.0)
NCOL = len(CLASSES) * len(PSI_DEG) * len(LAI_TOT)
MLA = 57.0


def make_domain_columns(nb, nz, uniform, seed=1):
    """The 200 domain columns as a ``synth.make_columns`` dict (same keys, host arrays), plus the index arrays ``cls``, ``ipsi``, ``ilai``
    (into CLASSES, PSI_DEG, LAI_TOT) of every column.

    Column c = (ilai * len(PSI_DEG) + ipsi) * len(CLASSES) + cls: the class changes fastest.  Optics, irradiances and the shape of the
    cumulative-LAI profile (equal steps, or the generator's ragged power-law profiles) are ``synth.make_columns``'; ``lai`` is rescaled to
    the column's total and ``mla`` is 57 degrees (spherical leaves' mean angle; only 2s reads it)."""
    from crt1d_amd import synth

    d = dict(synth.make_columns(NCOL, nb, nz, seed=seed, uniform_dlai=uniform))
    c = np.arange(NCOL)
    cls = c % len(CLASSES)
    ipsi = (c // len(CLASSES)) % len(PSI_DEG)
    ilai = c // (len(CLASSES) * len(PSI_DEG))
    tot = np.asarray(LAI_TOT)[ilai]
    if uniform:  # as the generator forms it, so that the columns are uniform to the bit the kernels test for
        lai = tot[:, None] * np.linspace(1.0, 0.0, nz)[None, :]
    else:
        lai = d["lai"] * (tot / d["lai"][:, 0])[:, None]
        lai[:, 0] = tot
        lai[:, -1] = 0.0
    d["lai"] = np.ascontiguousarray(lai)
    d["psi"] = np.deg2rad(np.asarray(PSI_DEG))[ipsi]
    d["mla"] = np.full(NCOL, MLA)
    d["g_kind"] = np.array([CLASSES[i][1] for i in cls], dtype=np.int32)
    d["g_param"] = np.array([CLASSES[i][2] for i in cls], dtype=np.float64)
    d["cls"], d["ipsi"], d["ilai"] = cls, ipsi, ilai
    return d


def take_columns(d, idx):
    """The columns ``idx`` of a make_domain_columns dict."""
    n = d["psi"].shape[0]
    return {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------------------
# the device's tau_d rule on the host (csrc/colpre.hip build_host_tables): what tests/test_quadrature_domain_cpu.py measures against
# mpmath, and what the bars below are derived from
DEVICE_EDGES = (0.0, 1e-4, 1e-3, 1e-2, 0.1, 0.6, 1.0)  # PAN_EDGE: panel edges in t = pi/2 - psi, fractions of pi/2


def G_np(kind, x, c, s):
    """G from (cos psi, sin psi) in double precision, the expressions of csrc/crt_internal.hpp G_eval."""
    if kind == HORIZONTAL:
        return c + 0.0
    if kind == SPHERICAL or (kind == ELLIPSOIDAL and x == 1):
        return np.full_like(c, 0.5)
    if kind == VERTICAL:
        return 2 / np.pi * s
    if kind in (ELLIPSOIDAL, ELLIPSOIDAL_APPROX):
        if kind == ELLIPSOIDAL_APPROX:
            p2 = x + 1.774 * (x + 1.182) ** -0.733
        elif x > 1:
            e = np.sqrt(1 - x**-2)
            p2 = x + np.log((1 + e) / (1 - e)) / (2 * e * x)
        else:
            e = np.sqrt(1 - x**2)
            p2 = x + np.arcsin(e) / e
        return np.sqrt(x * x * c * c + s * s) / p2
    assert kind == BONAN
    phi1 = 0.5 - 0.633 * x - 0.330 * x * x
    return phi1 + 0.877 * (1 - 2 * phi1) * c


def device_rule(edges=DEVICE_EDGES):
    """(t, w): nodes in t = pi/2 - psi and weights of the 6 x 16 Gauss-Legendre rule."""
    from numpy.polynomial.legendre import leggauss

    x, w = leggauss(16)
    e = [np.pi / 2 * f for f in edges]
    t = np.concatenate([a + (x + 1) * (b - a) / 2 for a, b in zip(e[:-1], e[1:])])
    wt = np.concatenate([w * (b - a) / 2 for a, b in zip(e[:-1], e[1:])])
    return t, wt


def device_one_minus_tau_d(kind, x, L, rule=None):
    """1 - tau_d(L) by the device's rule: cos psi = sin t at the nodes, which keeps its relative accuracy next to pi/2 (col_record.hpp),
    and -expm1 (no cancellation)."""
    t, wt = device_rule() if rule is None else rule
    c, s = np.sin(t), np.cos(t)
    k = G_np(kind, x, c, s) / c
    return -np.expm1(-np.multiply.outer(np.asarray(L, dtype=np.float64), k)) @ (2 * wt * s * c)


# ------------------------------------------------------------------------------------------------------------------
# comparison with the oracle: bars per (column, band), derived from the oracle's own quantities and from the rules' measured truncation
# error -- never from a kernel's output
RULE_SCHEMES = ("2s", "4s", "bl", "n79", "zq", "zq_pa")  # read mu_bar (2s), G_int_1/2 (4s) or tau_d; g77 and bf use no quadrature


def oracle_solve(oracle, d, scheme):
    cols = oracle.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
    kw = dict(I_dr0=d["I_dr0"], I_df0=d["I_df0"], leaf_r=d["leaf_r"], leaf_t=d["leaf_t"], soil_r=d["soil_r"])
    if scheme == "bl":
        kw.pop("soil_r")
    return oracle.SOLVERS[scheme](cols, **kw)


@contextlib.contextmanager
def device_rules(oracle, edges=DEVICE_EDGES):
    """The oracle with the device's quadrature in place of its own: the 6 x 16 rule for tau_d, 1 - tau_d and mu_bar, 16 instead of 24
    Gauss-Legendre nodes on each side of acos mu_s for G_int_1/2.  (The oracle takes cos psi of psi = pi/2 - t where the device holds
    sin t; next to pi/2 that is an absolute difference of 6e-17 in cos psi, and 3e-17 relative in 1 - tau_d of the thinnest layer.)"""
    from numpy.polynomial.legendre import leggauss

    t, wt = device_rule(edges)
    saved = oracle._PSI_Q, oracle._W_Q, oracle.leggauss
    oracle._PSI_Q, oracle._W_Q = np.pi / 2 - t, wt
    oracle.leggauss = lambda n: leggauss(16 if n == 24 else n)
    try:
        yield
    finally:
        oracle._PSI_Q, oracle._W_Q, oracle.leggauss = saved


def oracle_solve_device_rules(oracle, d, scheme, ref, edges=DEVICE_EDGES):
    """``oracle_solve`` under ``device_rules``; ``ref`` (the plain oracle's solution) is returned for a scheme that uses no quadrature.
    4s (a Python loop per column and band) is solved again only for the columns whose G_int_1/2 differ between the rules by more
    than rounding; the other columns are ``ref``'s."""
    if scheme not in RULE_SCHEMES:
        return ref
    with device_rules(oracle, edges):
        if scheme != "4s":
            return oracle_solve(oracle, d, scheme)
        oc = oracle.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
        gi_dev = oracle.G_integrals(oc, 0.501)
    gi = oracle.G_integrals(oc, 0.501)
    sel = np.flatnonzero((np.abs(gi_dev - gi) > 1e-14 * np.abs(gi)).any(axis=1))
    out = {k: v.copy() for k, v in ref.items()}
    if sel.size:
        with device_rules(oracle, edges):
            sub = oracle_solve(oracle, take_columns(d, sel), scheme)
        for k in out:
            out[k][sel] = sub[k]
    return out


def singular_quantities(oracle, d):
    """What the two removable singularities of the closed forms are made of, per (column, band) [Kb: (ncol, 1)], from the oracle: 2s
    sigma = (mu_bar K_b)^2 + c^2 - b^2 with its terms mbK = mu_bar K_b, b, c (_solve_2s.py:65-85); bf k_d = 0.8 sqrt(1 - omega) against
    K_b (_solve_bf.py:80,95).  One place for ``domain_bars`` and for the tests that choose well-conditioned bands."""
    oc = oracle.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
    Kb = oc.K_b()[:, None]
    om = d["leaf_r"] + d["leaf_t"]
    beta = 0.5 * (om + (d["leaf_r"] - d["leaf_t"]) * np.cos(np.deg2rad(d["mla"]))[:, None] ** 2) / om
    b_, c_ = 1 - (1 - beta) * om, om * beta
    mbK = oracle.mu_bar(oc)[:, None] * Kb
    return {"oc": oc, "Kb": Kb, "om": om, "b": b_, "c": c_, "mbK": mbK, "sigma": mbK ** 2 + c_**2 - b_**2, "k_d": 0.8 * np.sqrt(1 - om)}


def domain_bars(oracle, d, uniform):
    """Allowed error of a kernel against the oracle WITH THE SAME QUADRATURE RULES (``oracle_solve_device_rules``), as a fraction of the
    profile maximum, per (column, band) [or per column, shape (ncol, 1)]:

    "base"     1e-11, the bar of tests/test_gpu_parity.py::test_hip_vs_oracle_synthetic;
    "2s"       1e-11 + 1e-14 / |sigma|, sigma = (mu_bar K_b)^2 + c^2 - b^2 (_solve_2s.py:85): every h_i / sigma term of the closed form is a
               removable singularity there, and two fp64 evaluation orders differ by ~eps / |sigma| (test_invariants_full_size);
    "bf"       1e-11 + 1e-14 / |k_d - K_b|, the same for (e^{-K_b L} - e^{-k_d L}) / (k_d - K_b) (B&F eq. 8, _solve_bf.py:95);
    "4s"       1e-11 + 1e-14 / min_k |1 - lambda_k / kappa|, lambda_k the eigenvalues of the four-stream matrix A (_solve_4s.py:81-95) and
               kappa = K_b: the particular solution -(A + kappa I)^-1 g of the direct-beam source has a pole where an eigenvalue of A equals
               -kappa, cancelled by the homogeneous coefficients -- a removable singularity of the same kind as the two above (in the
               kernel's p'' = B p form: an eigenvalue of B equal to kappa^2).  The batch has one such band: approx x = 10, psi = 30
               degrees at 18 bands, lambda = 0.9723 against kappa = 0.97228, gap 3.8e-7, cond(A + kappa I) = 5.8e6;
    "shade"    added for aI_lsh of g77 and bf, (1 - e^{-K_b L}) x ... as the reference forms it (_solve_g77.py:99, _solve_bf.py:116):
               4 ulp(1) / (1 - e^{-K_b LAI}), ulp(1) = 2^-53 -- e^{-K_b L} is rounded below 1 on both sides (the device's fexp within an
               ulp, as NumPy's), and where K_b LAI << 1 the whole profile of 1 - e^{-K_b L} is made of those roundings (vertical leaves at
               0.05 degrees with LAI 0.01: K_b LAI = 5.6e-6, one ulp is 2e-11 of the profile maximum);
    "n79_aI"   aI_lsl, aI_lsh of n79, (1 - tau_d(dlai)) / dlai: test_hip_vs_oracle_synthetic's 3e-10 on ragged profiles, 1e-11 on uniform.

    Against the plain oracle, whose rules are finer (pinned to mpmath at 2e-15, tests/test_quadrature_domain_cpu.py), ``check_scheme``
    adds 4 x the device rules' truncation error propagated through the scheme: 4 x |oracle with the device's rules - oracle|, per output,
    column and band.  What that error is in the integrals themselves is tabulated per class and layer thickness in
    test_quadrature_domain_cpu.py DEVICE_OMT / DEVICE_REST and DESIGN.md 3.2; it is visible (above 1e-11 in an output) in three places:
    n79's aI_ls* where layers are thinner than 1e-3 (up to 2e-8 at dlai = 3.6e-6); the diffuse fluxes of n79, zq and zq_pa for Bonan
    chi_l = 0.6 leaves in layers of ~2e-4 (2.4e-11: a layer's reflectance is (1 - tau_d) rho, relative error 3.5e-10); and 4s for
    ellipsoidal leaves with x = 0.2 or 10 (3.9e-11: G_int_1/2 by 16 nodes are 5e-12 off)."""
    ncol = d["psi"].shape[0]
    q = singular_quantities(oracle, d)
    oc, Kb, om, sigma, k_d = q["oc"], q["Kb"], q["om"], q["sigma"], q["k_d"]
    G12 = oracle.G_integrals(oc, 0.501)
    mu_1, mu_2, al, be, ga, _, _ = oracle._coef_4s(om, 1.0, G12[:, :1], G12[:, 1:], 0.501)
    G1, G2 = np.broadcast_to(G12[:, :1], om.shape), np.broadcast_to(G12[:, 1:], om.shape)
    A = np.array([[(al - G2) / mu_2, be / mu_2, be / mu_2, al / mu_2],
                  [be / mu_1, (ga - G1) / mu_1, ga / mu_1, be / mu_1],
                  [-be / mu_1, -ga / mu_1, -(ga - G1) / mu_1, -be / mu_1],
                  [-al / mu_2, -be / mu_2, -be / mu_2, -(al - G2) / mu_2]])  # (4, 4, ncol, nb)
    lam = np.linalg.eigvals(np.moveaxis(A, (0, 1), (-2, -1)))  # (ncol, nb, 4): +-lambda pairs, real or imaginary
    gap4 = np.abs(1 + lam / Kb[:, :, None]).min(axis=-1)
    return {
        "base": np.full((ncol, 1), 1e-11),
        "4s": 1e-11 + 1e-14 / gap4,
        "shade": 4 * 2.0**-53 / -np.expm1(-Kb * d["lai"][:, :1]),
        "2s": 1e-11 + 1e-14 / np.abs(sigma),
        "bf": 1e-11 + 1e-14 / np.abs(k_d - Kb),
        "n79_aI": np.full((ncol, 1), 1e-11 if uniform else 3e-10),
    }


def bar_for(scheme, key, bars):
    if scheme in ("g77", "bf") and key == "aI_lsh":
        return bars["bf" if scheme == "bf" else "base"] + bars["shade"]
    if scheme in ("2s", "bf", "4s"):
        return bars[scheme]
    if scheme == "n79" and key.startswith("aI"):
        return bars["n79_aI"]
    return bars["base"]


def column_errors(got, ref):
    """(profile error, elementwise error), each (ncol, nb): conftest.rel_profile_err and rel_elem_err before their maximum over columns
    and bands."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.ndim == 1:  # one value per column (bf's rho_c)
        got, ref = got[:, None, None], ref[:, None, None]
    scale = np.abs(ref).max(axis=1, keepdims=True)
    scale = np.where(scale == 0, 1.0, scale)
    diff = np.abs(got - ref)
    return (diff / scale).max(axis=1), (diff / np.maximum(np.abs(ref), 1e-9 * scale)).max(axis=1)


def check_scheme(scheme, got, ref, bars, rule_ref=None, tally=None):
    """Every output array of ``got`` against ``ref``: finite, profile error <= bar, elementwise error <= 100 x bar (the two assertions of
    test_hip_vs_oracle_synthetic), per (column, band).  ``rule_ref``: ``ref`` is the plain oracle's solution and ``rule_ref`` the one
    with the device's rules; the bar is widened by 4 x their difference (``domain_bars``).  Returns the failures as
    (key, column, error / bar, bar), worst first; ``tally[key]`` gets the worst (profile error, error / bar)."""
    fails = []
    for k in got:  # (the oracle also returns what the reference returns beside the arrays: bf's rho_c)
        g = np.asarray(got[k])
        if not np.all(np.isfinite(g)):
            fails.append((k + ": not finite", int(np.argwhere(~np.isfinite(g))[0][0]), np.inf, 0.0))
            continue
        prof, elem = column_errors(g, ref[k])
        bar = bar_for(scheme, k, bars)
        tol = np.broadcast_to(bar[:, -1:] if prof.shape[1] == 1 else bar, prof.shape)  # (bf's rho_c is the last band's)
        if rule_ref is not None:
            tol = tol + 4 * column_errors(rule_ref[k], ref[k])[0]
        ratio = np.maximum(prof / tol, elem / (100 * tol))
        if tally is not None:
            tally[k] = (float(prof.max()), float(ratio.max()))
        for c, b in np.argwhere(ratio > 1):
            fails.append((k, int(c), float(ratio[c, b]), float(tol[c, b])))
    return sorted(fails, key=lambda f: -f[2])
