"""CPU: the two fixed-node quadrature rules -- the oracle's (oracle/crt_oracle.py _graded_rule) and the device's (csrc/colpre.hip PAN_EDGE,
rebuilt here on the host from crt_hip_quad_nodes) -- against converged mpmath integrals, on every leaf-angle class of
tests/domain_cases.py.

    tau_d(L)     = 2 int_0^{pi/2} e^{-G(psi) L / cos psi} sin psi cos psi dpsi        (common.py:30-37)
    1 - tau_d(L) = 2 int (1 - e^{-G L / cos}) sin cos dpsi: what n79 divides by dlai  (_solve_n79.py:146,154-155)
    mu_bar       = int_0^{pi/2} cos psi sin psi / G(psi) dpsi                         (_solve_2s.py:32)
    G_int_1, 2   = int_0^{mu_s} G(acos m) dm, int_{mu_s}^1                            (_solve_4s.py:148-149), mu_s in {0.501, 0.33998}

L runs over {1e-4, 3e-4, 1e-3, 1e-2, 0.1, 1, 12} and two thinner layers, 1e-6 and 1e-5: a ragged 60-level profile of total LAI 0.01
(tests/test_gpu_domain.py) has layers down to dlai = 3.6e-6.

The mpmath value.  Integrals in t = pi/2 - psi, Gauss-Legendre on pieces split at t = pi/2 10^-k (k = 1 .. 14): the integrand is analytic
on every piece but the innermost, which contributes less than 1e-27.  A value is accepted only if 60 digits with more pieces (k to 16,
and 3 10^-k) move it by less than 1e-20 relative -- asserted (measured: 1.6e-24).  Where a closed form exists (horizontal e^{-L},
spherical 2 E_3(L / 2), Bonan 2 e^{-phi_2 L} E_3(phi_1 L)) the integral also has to reproduce it: to 1e-20, and to 1e-25 at 60 digits.

Measured here (x86-64, glibc, NumPy 2.2); every bar below is one of these figures times the stated factor:

  oracle rule (12 x 24), worst over classes and L      tau_d 1.1e-15   1 - tau_d 6.4e-16   mu_bar 2.0e-16   G_int 4.3e-16
  device rule (6 x 16): table DEVICE_OMT below (1 - tau_d per class and L), DEVICE_REST (tau_d worst over L, mu_bar, G_int)
"""
import numpy as np
import pytest
from numpy.polynomial.legendre import leggauss

import domain_cases as D
from domain_cases import (BONAN, CLASSES, DEVICE_EDGES, ELLIPSOIDAL, ELLIPSOIDAL_APPROX, HORIZONTAL, SPHERICAL, VERTICAL, G_np,
                          device_one_minus_tau_d, device_rule)

L_GRID = (1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 1e-2, 0.1, 1.0, 12.0)
MU_S = (0.501, 0.33998)
T = np.pi / 2


# ------------------------------------------------------------------------------------------------------------------
# mpmath side
def _mp_G(mp, kind, param):
    """G as a function of (cos psi, sin psi) in mpmath arithmetic; leaf_angle.py:118-202.  The decimal constants are taken at their
    double values, as the oracle and the device hold them."""
    x = mp.mpf(param)
    if kind == HORIZONTAL:
        return lambda c, s: c
    if kind == SPHERICAL or (kind == ELLIPSOIDAL and x == 1):
        return lambda c, s: mp.mpf(0.5)
    if kind == VERTICAL:
        return lambda c, s: 2 / mp.pi * s
    if kind == ELLIPSOIDAL:
        if x > 1:
            e = mp.sqrt(1 - x**-2)
            p2 = x + mp.log((1 + e) / (1 - e)) / (2 * e * x)
        else:
            e = mp.sqrt(1 - x**2)
            p2 = x + mp.asin(e) / e
        return lambda c, s: mp.sqrt(x * x * c * c + s * s) / p2
    if kind == ELLIPSOIDAL_APPROX:
        p2 = x + mp.mpf(1.774) * (x + mp.mpf(1.182)) ** mp.mpf(-0.733)
        return lambda c, s: mp.sqrt(x * x * c * c + s * s) / p2
    assert kind == BONAN
    phi1 = mp.mpf(0.5) - mp.mpf(0.633) * x - mp.mpf(0.330) * x**2
    phi2 = mp.mpf(0.877) * (1 - 2 * phi1)
    return lambda c, s: phi1 + phi2 * c


def _mp_closed_tau_d(mp, kind, param, L):
    """tau_d in closed form where there is one, else None."""
    L = mp.mpf(L)
    if kind == HORIZONTAL:
        return mp.exp(-L)
    if kind == SPHERICAL or (kind == ELLIPSOIDAL and param == 1):
        return 2 * mp.expint(3, L / 2)
    if kind == BONAN:
        x = mp.mpf(param)
        phi1 = mp.mpf(0.5) - mp.mpf(0.633) * x - mp.mpf(0.330) * x**2
        phi2 = mp.mpf(0.877) * (1 - 2 * phi1)
        return 2 * mp.exp(-phi2 * L) * mp.expint(3, phi1 * L)
    return None


def _mp_values(dps, kmax, more):
    """{(class, quantity[, L | mu_s]): mpf} at ``dps`` digits; pieces split at pi/2 10^-k, k <= kmax (``more``: also 3 10^-k and 0.6)."""
    import mpmath as mp

    out = {}
    with mp.workdps(dps):
        Tm = mp.pi / 2
        pts = [mp.mpf(0)] + [Tm * mp.mpf(10) ** -k for k in range(kmax, 0, -1)] + [Tm]
        if more:
            pts = sorted(pts + [3 * Tm * mp.mpf(10) ** -k for k in range(1, 9)] + [Tm * mp.mpf("0.6")])
        quad = lambda f, p: mp.quad(f, p, method="gauss-legendre")  # noqa: E731
        for name, kind, param in CLASSES:
            G = _mp_G(mp, kind, param)
            for L in L_GRID:
                Lm = mp.mpf(L)

                def f(t):
                    c, s = mp.sin(t), mp.cos(t)  # cos psi, sin psi
                    return -mp.expm1(-G(c, s) * Lm / c) * c * s

                om = 2 * quad(f, pts)
                out[name, "one_minus_tau_d", L] = om
                out[name, "tau_d", L] = 1 - om  # om >= 1e-7 and tau_d >= 6e-6: at most 8 of the digits cancel

            def fm(t):
                c, s = mp.sin(t), mp.cos(t)
                return c * s / G(c, s)

            out[name, "mu_bar"] = quad(fm, pts)
            for mu_s in MU_S:
                ps = mp.acos(mp.mpf(mu_s))
                h = lambda p: G(mp.cos(p), mp.sin(p)) * mp.sin(p)  # noqa: E731
                out[name, "G_int_1", mu_s] = quad(h, [ps, (ps + Tm) / 2, Tm])
                out[name, "G_int_2", mu_s] = quad(h, [0, ps / 2, ps])
    return out


@pytest.fixture(scope="module")
def mpref():
    """Converged mpmath values as floats, after the convergence and closed-form assertions."""
    import mpmath as mp

    a = _mp_values(30, 14, False)
    b = _mp_values(60, 16, True)
    worst = max(float(abs(a[k] - b[k]) / abs(b[k])) for k in a)
    print(f"mpmath 30 digits vs 60 digits with more pieces: {worst:.1e}")
    assert worst < 1e-20, worst
    with mp.workdps(60):
        for name, kind, param in CLASSES:
            for L in L_GRID:
                cf = _mp_closed_tau_d(mp, kind, param, L)
                if cf is not None:
                    assert abs(a[name, "tau_d", L] - cf) / cf < 1e-20 and abs(b[name, "tau_d", L] - cf) / cf < 1e-25, (name, L)
    return {k: float(v) for k, v in a.items()}


# ------------------------------------------------------------------------------------------------------------------
# the oracle's rule
# bars: largest error measured over classes and L (module docstring), times 4 for another platform's libm.  The three figures below 1e-15
# are the rounding of a 288-term (G_int: 24-term) sum, not truncation; they are taken as 1e-15.
ORACLE_BARS = {"tau_d": 4 * 1.1e-15, "one_minus_tau_d": 4 * 1e-15, "mu_bar": 4 * 1e-15, "G_int": 4 * 1e-15}


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_oracle_rule_vs_mpmath(oracle, mpref):
    """oracle.tau_d, one_minus_tau_d, mu_bar and G_integrals on every class and L.  One tenth of the tightest GPU bar they support is
    1e-12 (tests/test_gpu_parity.py: 1e-11); the rule is three orders inside it."""
    worst = dict.fromkeys(ORACLE_BARS, 0.0)
    for name, kind, param in CLASSES:
        cols = oracle.Columns(np.array([0.3]), np.zeros((1, 3)), g_kind=[kind], g_param=[param])
        L = np.array([L_GRID])
        td, om, mb = oracle.tau_d(cols, L)[0], oracle.one_minus_tau_d(cols, L)[0], oracle.mu_bar(cols)[0]
        err = {
            "tau_d": max(_rel(td[i], mpref[name, "tau_d", Lv]) for i, Lv in enumerate(L_GRID)),
            "one_minus_tau_d": max(_rel(om[i], mpref[name, "one_minus_tau_d", Lv]) for i, Lv in enumerate(L_GRID)),
            "mu_bar": _rel(mb, mpref[name, "mu_bar"]),
            "G_int": max(_rel(oracle.G_integrals(cols, m)[0][k], mpref[name, f"G_int_{k + 1}", m]) for m in MU_S for k in (0, 1)),
        }
        print(f"oracle rule {name:18s} " + "  ".join(f"{q} {e:.1e}" for q, e in err.items()))
        for q, e in err.items():
            worst[q] = max(worst[q], e)
            assert e <= ORACLE_BARS[q], (name, q, e)
    print("oracle rule, worst: " + "  ".join(f"{q} {e:.1e}" for q, e in worst.items()))


# ------------------------------------------------------------------------------------------------------------------
# the device's rule, rebuilt on the host
# Relative error of 1 - tau_d(L) by the device's rule against mpmath, measured; columns = L_GRID.  Entries at rounding level are
# recorded as 1e-15.  The rule resolves the boundary layer at cos psi ~ G(pi/2) L down to its finest panel, [0, 1e-4] pi/2: below
# L ~ 1e-4 / G(pi/2) the error grows to ~1e-7 at L = 1e-6 (and falls again beyond, as G(pi/2)^2 L).
#                      L = 1e-6    1e-5     1e-4     3e-4     1e-3     1e-2     0.1      1        12
DEVICE_OMT = {
    "horizontal":       (1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15),
    "spherical":        (1.0e-07, 8.8e-09, 3.4e-11, 8.5e-14, 7.4e-13, 1.8e-12, 3.0e-13, 4.6e-15, 1e-15),
    "vertical":         (1.2e-07, 3.4e-09, 1.0e-11, 4.5e-13, 1.1e-12, 1.8e-12, 3.2e-13, 2.6e-15, 1e-15),
    "ellipsoidal_x0.2": (1.2e-07, 3.9e-09, 8.6e-12, 4.1e-13, 1.0e-12, 1.8e-12, 2.8e-13, 2.0e-15, 5.9e-15),
    "ellipsoidal_x1":   (1.0e-07, 8.8e-09, 3.4e-11, 8.5e-14, 7.4e-13, 1.8e-12, 3.0e-13, 4.6e-15, 1e-15),
    "ellipsoidal_x10":  (1.6e-08, 1.2e-08, 4.8e-10, 3.2e-11, 2.2e-13, 2.0e-13, 6.8e-14, 1.6e-14, 1e-15),
    "approx_x0.2":      (1.2e-07, 3.9e-09, 8.5e-12, 4.1e-13, 1.0e-12, 1.8e-12, 2.8e-13, 2.2e-15, 5.8e-15),
    "approx_x10":       (1.6e-08, 1.2e-08, 4.8e-10, 3.2e-11, 2.2e-13, 2.0e-13, 6.9e-14, 1.6e-14, 1e-15),
    "bonan_-0.4":       (1.2e-07, 9.9e-10, 1.4e-11, 5.8e-13, 1.2e-12, 1.6e-12, 4.5e-13, 1e-15,   1e-15),
    "bonan_0.6":        (1.3e-11, 7.8e-11, 3.0e-10, 3.5e-10, 9.8e-11, 3.6e-12, 1e-15,   2.5e-15, 1e-15),
}
# (tau_d worst over L_GRID, mu_bar, G_int worst over both intervals and both mu_s), same convention
DEVICE_REST = {
    "horizontal":       (1e-15,   1e-15,   1e-15),
    "spherical":        (1.0e-13, 1e-15,   1e-15),
    "vertical":         (1.2e-13, 1e-15,   1e-15),
    "ellipsoidal_x0.2": (3.6e-13, 2.8e-13, 5.4e-12),
    "ellipsoidal_x1":   (1.0e-13, 1e-15,   1e-15),
    "ellipsoidal_x10":  (1.0e-12, 1.5e-14, 5.1e-12),
    "approx_x0.2":      (3.6e-13, 2.8e-13, 5.4e-12),
    "approx_x10":       (1.0e-12, 1.5e-14, 5.1e-12),
    "bonan_-0.4":       (1.2e-13, 1e-15,   1e-15),
    "bonan_0.6":        (9.2e-14, 1.5e-12, 1e-15),
}


@pytest.fixture(scope="module")
def lib_nodes():
    import os

    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.quad_nodes(0.501), _lib.quad_nodes(0.33998)


def test_device_rule_vs_mpmath(mpref, lib_nodes):
    """What the device's 96 tau_d nodes and 32 G_int nodes can deliver, per class and L: the table of DESIGN.md section 3.2, asserted at
    twice the measured figures so that a change of csrc/colpre.hip PAN_EDGE cannot lose accuracy silently."""
    t, wt = device_rule()
    # the library's nodes are the ones rebuilt here (psi = pi/2 - t; G_int: 16 Gauss-Legendre nodes on each side of acos mu_s)
    np.testing.assert_allclose(lib_nodes[0][:96], T - t, rtol=0, atol=2e-16)
    xg, wg = leggauss(16)
    c, s = np.sin(t), np.cos(t)
    over = []
    for name, kind, x in CLASSES:
        g = G_np(kind, x, c, s)
        k = g / c
        om = device_one_minus_tau_d(kind, x, L_GRID, (t, wt))
        td = np.exp(-np.multiply.outer(np.asarray(L_GRID), k)) @ (2 * wt * s * c)
        e_om = [_rel(om[i], mpref[name, "one_minus_tau_d", L]) for i, L in enumerate(L_GRID)]
        e_td = max(_rel(td[i], mpref[name, "tau_d", L]) for i, L in enumerate(L_GRID))
        e_mb = _rel(np.sum(wt * c * s / g), mpref[name, "mu_bar"])
        e_g = 0.0
        for nodes, mu_s in zip(lib_nodes, MU_S):
            ps = np.arccos(mu_s)
            for i, (lo, hi) in enumerate(((ps, T), (0.0, ps))):
                p = lo + (xg + 1) * (hi - lo) / 2
                np.testing.assert_allclose(np.sort(nodes[96 + 16 * i:112 + 16 * i]), p, rtol=0, atol=4e-16)
                val = np.sum(wg * (hi - lo) / 2 * G_np(kind, x, np.cos(p), np.sin(p)) * np.sin(p))
                e_g = max(e_g, _rel(val, mpref[name, f"G_int_{i + 1}", mu_s]))
        print(f"device rule {name:18s} 1-tau_d " + " ".join(f"{e:.1e}" for e in e_om) + f" | tau_d {e_td:.1e} mu_bar {e_mb:.1e} G_int {e_g:.1e}")
        over += [(name, "1 - tau_d", L, e_om[i]) for i, L in enumerate(L_GRID) if e_om[i] > 2 * DEVICE_OMT[name][i]]
        over += [(name, q, None, e) for q, e, bar in zip(("tau_d", "mu_bar", "G_int"), (e_td, e_mb, e_g), DEVICE_REST[name]) if e > 2 * bar]
    assert not over, over  # (after the whole table is printed)


def test_device_rule_documented_claims():
    """The sentences of csrc/colpre.hip (PAN_EDGE), csrc/col_record.hpp and DESIGN.md 3.2 about the rule, as inequalities over the table."""
    col = {L: i for i, L in enumerate(L_GRID)}
    x10 = ("ellipsoidal_x10", "approx_x10")
    for name, row in DEVICE_OMT.items():
        if name == "bonan_0.6":
            assert row[col[1e-3]] <= 9.8e-11 and row[col[1e-2]] <= 3.6e-12 and max(row[col[0.1]:]) <= 2.3e-12
            assert row[col[3e-4]] <= 3.5e-10 and row[col[1e-4]] <= 3.0e-10
        else:
            assert max(row[col[1e-3]:]) <= 1.8e-12, name
            assert row[col[3e-4]] <= (3.2e-11 if name in x10 else 5.8e-13), name
            assert row[col[1e-4]] <= (4.8e-10 if name in x10 else 3.4e-11), name
        assert row[col[1e-5]] <= 1.2e-8 and row[col[1e-6]] <= 1.2e-7, name
    for name, (td, mb, gi) in DEVICE_REST.items():
        assert td <= 1.0e-12 and gi <= 5.4e-12, name
        assert mb <= (1.5e-12 if name == "bonan_0.6" else 2.8e-13 if name.endswith("x0.2") else 1.5e-14), name


# ------------------------------------------------------------------------------------------------------------------
# would the GPU domain test see a kernel that is subtly wrong?  Shown on the CPU, on the batch and with the assertions of that test
MUTATION_SCHEMES = ("2s", "bl", "n79", "zq")


def test_domain_assertions_catch_a_perturbed_G_and_a_moved_panel_edge(oracle):
    """tests/test_gpu_domain.py holds a kernel's output to two comparisons (domain_cases.check_scheme): against the plain oracle at the
    bars widened by the device rules' truncation error, and against the oracle with the device's rules at the plain bars.  Here the
    'kernel' is the oracle with the device's rules -- which must pass both -- and then the same with a fault planted:
      (a) G of one class (spherical) larger by 1e-9 relative;
      (b) the panel edge next to psi = pi/2 moved from 1e-4 to 4e-4 (of pi/2), and the edge at 0.1 moved to 0.2.
    Each fault must fail BOTH comparisons, in every scheme that can see it, and (a) only in the columns of that class."""
    d = D.make_domain_columns(6, 12, False)
    bars = D.domain_bars(oracle, d, False)
    ref = {s: D.oracle_solve(oracle, d, s) for s in MUTATION_SCHEMES}
    rule_ref = {s: D.oracle_solve_device_rules(oracle, d, s, ref[s]) for s in MUTATION_SCHEMES}

    def both(s, kernel):
        return D.check_scheme(s, kernel, ref[s], bars, rule_ref=rule_ref[s]), D.check_scheme(s, kernel, rule_ref[s], bars)

    for s in MUTATION_SCHEMES:
        assert both(s, rule_ref[s]) == ([], []), s

    closed = oracle._G_closed_form
    oracle._G_closed_form = lambda kind, param, psi: closed(kind, param, psi) * (1 + 1e-9 * (kind == SPHERICAL))
    try:
        bad = {s: D.oracle_solve_device_rules(oracle, d, s, None) for s in MUTATION_SCHEMES}
    finally:
        oracle._G_closed_form = closed
    for s in MUTATION_SCHEMES:
        for fails in both(s, bad[s]):
            print(f"G x (1 + 1e-9), {s}: {len(fails)} (column, band, output) over the bar, worst {fails[0][2]:.1f} x" if fails else f"G, {s}: none")
            assert fails and all(d["g_kind"][c] == SPHERICAL for _, c, _, _ in fails), (s, fails[:3])

    for edges, seen_by in (((0.0, 4e-4) + DEVICE_EDGES[2:], ("n79", "zq")), (DEVICE_EDGES[:4] + (0.2, 0.6, 1.0), MUTATION_SCHEMES)):
        bad = {s: D.oracle_solve_device_rules(oracle, d, s, None, edges) for s in seen_by}
        for s in seen_by:
            for fails in both(s, bad[s]):
                print(f"edges {edges}, {s}: {len(fails)} over the bar, worst {fails[0][2]:.1f} x" if fails else f"edges {edges}, {s}: none")
                assert fails, (edges, s)
