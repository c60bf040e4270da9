"""CPU: the device's rule for tau_d'(L) = d tau_d / dL = -2 int_0^{pi/2} K_b(psi) e^{-K_b(psi) L} sin psi cos psi dpsi (csrc/dlai.hip,
crt_hip_dtau_d_f64: the nodes and weights of tau_d with the integrand factor -K_b e^{-K_b L}), rebuilt on the host from
crt_hip_quad_nodes, against converged mpmath integrals on the ten leaf-angle classes of tests/domain_cases.py and the L grid of
tests/test_quadrature_domain_cpu.py, {1e-6 .. 12}; and the '9sky' form against its nine-term closed sum.

The mpmath value is accepted by the procedure of tests/test_quadrature_domain_cpu.py: Gauss-Legendre in t = pi/2 - psi on pieces split at
t = pi/2 10^-k, 30 digits with k <= 14 against 60 digits with more pieces (k <= 16 and 3 10^-k) to 1e-20 relative (measured 5.1e-30), and
where tau_d has a closed form (horizontal e^{-L}, spherical 2 E_3(L / 2), Bonan 2 e^{-phi_2 L} E_3(phi_1 L)) its derivative is reproduced
to 1e-20, at 60 digits to 1e-25.

Measured (x86-64, glibc, NumPy 2.2): the table DEVICE_DTAU below, asserted at twice its figures.  In t the integrand is
-2 G e^{-G L / sin t} cos t, with the boundary layer of tau_d next to psi = pi/2 (t ~ G(pi/2) L): like 1 - tau_d, tau_d' is good to 3.5e-12
for L in [1e-3, 12] on every class but Bonan chi_l = 0.6 (1.9e-10 at 1e-3, 1.5e-11 at 1e-2), to 7.8e-10 at 1e-4, and loses the layer below that, where it
falls inside the finest panel: 2.5e-8 at 1e-5, 7.1e-8 at 1e-6.  That is the error that (1 - td_j)' = -D_j tau_d'(D_j) of an n79 layer carries,
next to the 1.2e-7 of (1 - td_j) itself at that thickness."""
import numpy as np
import pytest

from domain_cases import BONAN, CLASSES, ELLIPSOIDAL, HORIZONTAL, SPHERICAL, G_np, device_rule
from test_quadrature_domain_cpu import L_GRID, T, _mp_G, _rel

# Relative error of tau_d'(L) by the device's rule against mpmath, measured; columns = L_GRID.  Entries at rounding level are recorded as 1e-15.
#                      L = 1e-6    1e-5     1e-4     3e-4     1e-3     1e-2     0.1      1        12
DEVICE_DTAU = {
    "horizontal":       (1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15),
    "spherical":        (7.1e-08, 1.7e-08, 2.2e-10, 8.6e-13, 1.1e-12, 6.0e-13, 2.3e-12, 1.4e-14, 8.2e-15),
    "vertical":         (5.0e-08, 2.5e-08, 9.1e-11, 2.1e-12, 1.6e-12, 8.1e-13, 2.4e-12, 4.9e-14, 1e-15),
    "ellipsoidal_x0.2": (5.2e-08, 2.5e-08, 1.1e-10, 2.2e-12, 1.5e-12, 6.9e-13, 2.6e-12, 4.5e-14, 1.4e-13),
    "ellipsoidal_x1":   (7.1e-08, 1.7e-08, 2.2e-10, 8.6e-13, 1.1e-12, 6.0e-13, 2.3e-12, 1.4e-14, 8.2e-15),
    "ellipsoidal_x10":  (2.3e-08, 4.3e-09, 7.8e-10, 2.1e-10, 3.5e-12, 2.9e-13, 5.5e-13, 6.1e-13, 7.4e-13),
    "approx_x0.2":      (5.2e-08, 2.5e-08, 1.1e-10, 2.2e-12, 1.5e-12, 6.8e-13, 2.6e-12, 4.5e-14, 1.4e-13),
    "approx_x10":       (2.3e-08, 4.3e-09, 7.8e-10, 2.1e-10, 3.5e-12, 2.9e-13, 5.5e-13, 6.1e-13, 7.4e-13),
    "bonan_-0.4":       (3.4e-08, 2.4e-08, 9.1e-13, 1.3e-12, 1.7e-12, 1.5e-12, 6.9e-13, 8.1e-14, 1.1e-14),
    "bonan_0.6":        (2.4e-11, 1.3e-10, 4.1e-10, 2.9e-10, 1.9e-10, 1.5e-11, 1.1e-14, 2.6e-15, 2.6e-14),
}


def _mp_dtau(dps, kmax, more):
    """{(class, L): mpf tau_d'(L)} at ``dps`` digits; pieces split at pi/2 10^-k, k <= kmax (``more``: also 3 10^-k and 0.6)."""
    import mpmath as mp

    out = {}
    with mp.workdps(dps):
        Tm = mp.pi / 2
        pts = [mp.mpf(0)] + [Tm * mp.mpf(10) ** -k for k in range(kmax, 0, -1)] + [Tm]
        if more:
            pts = sorted(pts + [3 * Tm * mp.mpf(10) ** -k for k in range(1, 9)] + [Tm * mp.mpf("0.6")])
        for name, kind, param in CLASSES:
            G = _mp_G(mp, kind, param)
            for L in L_GRID:
                Lm = mp.mpf(L)

                def f(t):
                    c, s = mp.sin(t), mp.cos(t)  # cos psi, sin psi
                    g = G(c, s)
                    return -g * mp.exp(-g * Lm / c) * s  # -K_b e^{-K_b L} sin cos, K_b = G / cos

                out[name, L] = 2 * mp.quad(f, pts, method="gauss-legendre")
    return out


def _mp_closed_dtau(mp, kind, param, L):
    """tau_d' in closed form where tau_d has one, else None (E_n' = -E_{n-1})."""
    L = mp.mpf(L)
    if kind == HORIZONTAL:
        return -mp.exp(-L)
    if kind == SPHERICAL or (kind == ELLIPSOIDAL and param == 1):
        return -mp.expint(2, L / 2)
    if kind == BONAN:
        x = mp.mpf(param)
        phi1 = mp.mpf(0.5) - mp.mpf(0.633) * x - mp.mpf(0.330) * x**2
        phi2 = mp.mpf(0.877) * (1 - 2 * phi1)
        return -2 * mp.exp(-phi2 * L) * (phi2 * mp.expint(3, phi1 * L) + phi1 * mp.expint(2, phi1 * L))
    return None


@pytest.fixture(scope="module")
def mpref():
    import mpmath as mp

    a = _mp_dtau(30, 14, False)
    b = _mp_dtau(60, 16, True)
    worst = max(float(abs(a[k] - b[k]) / abs(b[k])) for k in a)
    print(f"mpmath 30 digits vs 60 digits with more pieces: {worst:.1e}")
    assert worst < 1e-20, worst
    with mp.workdps(60):
        for name, kind, param in CLASSES:
            for L in L_GRID:
                cf = _mp_closed_dtau(mp, kind, param, L)
                if cf is not None:
                    assert abs((a[name, L] - cf) / cf) < 1e-20 and abs((b[name, L] - cf) / cf) < 1e-25, (name, L)
    return {k: float(v) for k, v in a.items()}


def host_dtau_d_quad(kb_nodes, L):
    """The device's 'quad' rule for tau_d' on the host: K_b at the 96 tau_d nodes -> tau_d'(L)."""
    t, wt = device_rule()
    k = np.asarray(kb_nodes)[:96]
    return -(k * np.exp(-np.multiply.outer(np.asarray(L, dtype=np.float64), k))) @ (2 * wt * np.cos(t) * np.sin(t))


def host_dtau_d_9sky(k9, L):
    """The nine-term closed sum of the '9sky' form (common.py:40-53 with the factor -K_b e^{-K_b L})."""
    psi = np.radians(5.0 + 10.0 * np.arange(9))
    k9 = np.asarray(k9)
    return -(k9 * np.exp(-np.multiply.outer(np.asarray(L, dtype=np.float64), k9))) @ (np.sin(psi) * np.cos(psi)) * (2 * np.radians(10.0))


def test_device_dtau_rule_vs_mpmath(mpref):
    """Per class and L, asserted at twice the measured figures (the convention of the 1 - tau_d table)."""
    from crt1d_amd import _lib

    t, wt = device_rule()
    np.testing.assert_allclose(_lib.quad_nodes(0.501)[:96], T - t, rtol=0, atol=2e-16)
    c, s = np.sin(t), np.cos(t)
    over = []
    for name, kind, x in CLASSES:
        got = host_dtau_d_quad(G_np(kind, x, c, s) / c, L_GRID)
        err = [_rel(got[i], mpref[name, L]) for i, L in enumerate(L_GRID)]
        print(f"device tau_d' rule {name:18s} " + " ".join(f"{e:.1e}" for e in err))
        over += [(name, L, err[i]) for i, L in enumerate(L_GRID) if err[i] > 2 * DEVICE_DTAU[name][i]]
    assert not over, over  # (after the whole table is printed)


def test_9sky_is_its_nine_term_sum():
    """'9sky' has no truncation error to measure: it IS nine terms.  Two ways of forming the sum agree to 1e-14."""
    psi = np.radians(5.0 + 10.0 * np.arange(9))
    for name, kind, x in CLASSES:
        k9 = G_np(kind, x, np.cos(psi), np.sin(psi)) / np.cos(psi)
        got = host_dtau_d_9sky(k9, L_GRID)
        for i, L in enumerate(L_GRID):
            ref = sum(-kk * np.exp(-kk * L) * np.sin(p) * np.cos(p) for kk, p in zip(k9, psi)) * 2 * np.radians(10.0)
            assert abs(got[i] - ref) <= 1e-14 * abs(ref), (name, L)
        # and it is the derivative of the reference's nine-term tau_d: central difference of the closed sum, truncation h^2 K^2 / 6
        h = 1e-5
        td = lambda L: np.exp(-np.multiply.outer(L, k9)) @ (np.sin(psi) * np.cos(psi)) * (2 * np.radians(10.0))  # noqa: E731
        Ls = np.asarray(L_GRID[4:])
        fd = (td(Ls + h) - td(Ls - h)) / (2 * h)
        assert np.all(np.abs(fd - got[4:]) <= 1e-8 * np.abs(got[4:]) + 1e-10), name
