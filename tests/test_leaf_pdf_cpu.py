"""CPU: leaf-inclination PDFs (include/crt1d_hip_leaf.h) -- symbols and binding, argument errors before any launch, the Python ``g_*``
against the reference's values, and the quadrature rule of ``k_g_from_pdf`` restated in NumPy against mpmath.

The last check is what fixes ``CRT_LEAF_NGL``: the bar is ``|G - G_exact| <= 1e-11`` at every target angle (an error d in G moves a flux
by about d LAI / cos(psi) <= 31 d relative, and the tightest parity bar of the project is 3e-10).  Worst error of the 48-point rule over
everything below: 4.5e-13 (planophile at psi = (1 - 6e-6) pi/2, where the upper panel's integrand has a pole at
s = i sqrt(theta_k / psi) next to the panel; 32 points give 1.1e-11, 40 points 1.8e-12)."""
import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PI = np.pi / 2
BAR = 1e-11


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    return _lib.load()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_new_symbols_are_exported_and_bound(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_leaf.h")
    assert names == sorted(_lib.LEAF_EXPORTS) == ["crt_hip_g_from_pdf_f64", "crt_hip_leaf_pdf_nodes_f64"]
    for n in names:
        f = getattr(lib, n)
        assert f.restype is ctypes.c_int and f.argtypes is not None, n
    assert len(lib.crt_hip_g_from_pdf_f64.argtypes) == 10
    # the main header, its binding table and the ABI version are what they were
    assert len(_declared("crt1d_hip.h")) == 57 == len(_lib.EXPORTS)
    assert not set(_lib.LEAF_EXPORTS) & set(_lib.EXPORTS)
    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3
    # the header's constants and the binding's
    text = open(os.path.join(ROOT, "include", "crt1d_hip_leaf.h")).read()
    assert int(re.search(r"#define CRT_LEAF_NGL (\d+)", text).group(1)) == _lib.LEAF_NGL
    assert int(re.search(r"#define CRT_LEAF_NMLA (\d+)", text).group(1)) == _lib.LEAF_NMLA
    from crt1d_amd import leaf_angle as la

    enum = dict(re.findall(r"CRT_LEAF_PDF_(\w+) = (\d+)", text))
    assert {k: int(v) for k, v in enum.items()} == {"SPHERICAL": la.PDF_SPHERICAL, "ELLIPSOIDAL": la.PDF_ELLIPSOIDAL, "TRIG": la.PDF_TRIG}
    assert float(re.search(r"#define CRT_LEAF_X_MIN ([\d.]+)", text).group(1)) == la.PDF_X_MIN
    assert float(re.search(r"#define CRT_LEAF_X_MAX ([\d.]+)", text).group(1)) == la.PDF_X_MAX


def test_argument_errors_before_any_launch(lib):
    """Fake pointers: every call below must return before it touches them (no GPU here, nothing to launch on)."""
    from crt1d_amd import _lib

    fake = 0x1000
    call = lib.crt_hip_g_from_pdf_f64
    ok = dict(kind=fake, param=fake, ncol=4, mu_s=0.501, psi=fake, npsi=2, g_table=fake, g_at_psi=fake, mla=fake)

    def status(**kw):
        a = {**ok, **kw}
        return call(a["kind"], a["param"], a["ncol"], a["mu_s"], a["psi"], a["npsi"], a["g_table"], a["g_at_psi"], a["mla"], None)

    for bad in (dict(kind=None), dict(param=None), dict(g_table=None), dict(ncol=-1), dict(npsi=-1), dict(mu_s=0.0), dict(mu_s=1.0),
                dict(mu_s=float("nan")), dict(psi=None)):
        assert status(**bad) == _lib.CRT_ERR_BAD_ARG, bad
    assert status(ncol=0) == _lib.CRT_OK  # nothing to do
    assert status(ncol=0, g_at_psi=None, mla=None, psi=None, npsi=0) == _lib.CRT_OK
    # the node query: pairs go together
    x = (ctypes.c_double * _lib.LEAF_NGL)()
    assert lib.crt_hip_leaf_pdf_nodes_f64(x, None, None, None) == _lib.CRT_ERR_BAD_ARG
    assert lib.crt_hip_leaf_pdf_nodes_f64(None, None, None, None) == _lib.CRT_OK


def test_leaf_pdf_descriptions():
    from crt1d_amd import leaf_angle as la

    assert la.LeafPDF.planophile() == la.LeafPDF(la.PDF_TRIG, 1, 0) == la.LeafPDF.trig(1.0, 0.0)
    assert la.LeafPDF.spherical().param == (0.0, 0.0) and la.LeafPDF.ellipsoidal(2.5).param == (2.5, 0.0)
    assert la.LeafPDF.plagiophile().param == (0.0, -1.0) and la.LeafPDF.erectophile().param == (-1.0, 0.0)
    assert la.LeafPDF.uniform().kind == la.PDF_TRIG
    for bad in ((7,), (la.PDF_ELLIPSOIDAL, 0.0), (la.PDF_ELLIPSOIDAL, -1.0), (la.PDF_ELLIPSOIDAL, float("nan")), (la.PDF_ELLIPSOIDAL, 0.19), (la.PDF_ELLIPSOIDAL, 10.5), (la.PDF_SPHERICAL, 1.0),
                (la.PDF_TRIG, 1.0), (la.PDF_TRIG, 1.5, 0.0), (la.PDF_TRIG, 0.0, -1.5), (la.PDF_TRIG, 0.0, 1.5), (la.PDF_TRIG, 2.0, 1.0)):
        with pytest.raises(ValueError):
            la.LeafPDF(*bad)
    # the sign test against a dense scan of the PDF itself
    t = np.linspace(0, HALF_PI, 2001)
    rng = np.random.default_rng(5)
    for a, b in np.concatenate([rng.uniform(-2.5, 2.5, (400, 2)), [(1, 0), (-1, 0), (0, -1), (0, 1), (4 / 3, 1 / 3)]]):
        dense = (1 + a * np.cos(2 * t) + b * np.cos(4 * t)).min()
        if abs(dense) > 1e-5:  # (away from the boundary of the admissible set, where the scan's resolution decides)
            assert la.trig_pdf_is_nonnegative(a, b) == (dense > 0), (a, b, dense)


def test_python_pdfs_equal_the_reference():
    from crt1d_amd import leaf_angle as la

    g = load_golden("g11_leaf_pdf")
    theta = g["theta"]
    assert theta.shape == (50,) and list(g["names"]) == ["spherical", "uniform", "planophile", "erectophile", "plagiophile"]
    for i, name in enumerate(g["names"]):
        np.testing.assert_array_equal(getattr(la, "g_" + str(name))(theta), g["g"][i])
        # the device's description of the same PDF
        np.testing.assert_allclose(getattr(la.LeafPDF, str(name))().pdf(theta), g["g"][i], rtol=0, atol=4e-16)
    assert np.isscalar(la.g_uniform(0.3)) and la.g_uniform(0.3) == 2 / np.pi
    assert list(g["x"]) == [0.3, 1.0, 2.5]
    for i, x in enumerate(g["x"]):
        np.testing.assert_array_equal(la.g_ellipsoidal(theta, float(x)), g["g_ell"][i])
        np.testing.assert_array_equal(la.LeafPDF.ellipsoidal(float(x)).pdf(theta), g["g_ell"][i])
    # the reference's mla against the analytic ones it estimates: spherical 1 rad, uniform 45 deg
    assert abs(g["mla"][0] - np.rad2deg(1.0)) < 1e-7 and abs(g["mla"][1] - 45.0) < 1e-7


# ---- the rule of k_g_from_pdf, restated in NumPy from the exported nodes ----------------------------------------------------------
def _ell_l(x):
    if x == 1:
        return 2.0
    if x < 1:
        e = np.sqrt(1 - x * x)
        return x + np.arcsin(e) / e
    e = np.sqrt(1 - x ** -2)
    return x + np.log((1 + e) / (1 - e)) / (2 * e * x)


def rule_pdf(kind, p, st, ct):
    if kind == 0:
        return st
    if kind == 1:
        d = ct * ct + p[0] * p[0] * st * st
        return 2 * p[0] ** 3 / _ell_l(p[0]) * st / (d * d)
    c2 = 2 * ct * ct - 1
    c4 = 2 * c2 * c2 - 1
    return 2 / np.pi * (1 + p[0] * c2 + p[1] * c4)


def rule_G(kind, p, psi, x, w):
    """G at the angles ``psi`` (n,) by the device's rule (leaf_pdf.hip, G_of_pdf), nodes ``x`` and weights ``w`` on the unit interval."""
    psi = np.asarray(psi, dtype=np.float64)[:, None]
    sp, cp = np.sin(psi), np.cos(psi)
    tk = HALF_PI - psi
    th = tk * x
    lo = cp * tk * np.sum(w * rule_pdf(kind, p, np.sin(th), np.cos(th)) * np.cos(th), axis=1, keepdims=True)
    d = psi * x * x
    st, ct = np.sin(tk + d), np.cos(tk + d)
    with np.errstate(invalid="ignore", divide="ignore"):
        ss, cc = st * sp, ct * cp
        u = np.minimum(1.0, np.sin(d) / ss)
        h = np.sqrt(0.5 * u)
        A = cc + 2 / np.pi * (ss * 2 * h * np.sqrt(1 - 0.5 * u) - cc * 2 * np.arcsin(h))
        hi = psi * np.sum(w * 2 * x * rule_pdf(kind, p, st, ct) * A, axis=1, keepdims=True)
    return (lo + np.where(sp > 0, hi, 0.0))[:, 0]


@functools.lru_cache(maxsize=None)
def _projected(multiprecision, f, x, psi):
    """int_0^{pi/2} f(theta) A(psi, theta) dtheta by mpmath's tanh-sinh rule, which copes with the 3/2-power kink as an END point: the
    integration is split at theta_k.  A is written as the issue states it, beta = acos(min(1, cot(theta) cot(psi))).  f: "sin",
    "cos" (cos(x theta)) or "ell" (the ellipsoidal PDF of parameter x).  multiprecision: 25 digits, else mpmath's double context
    (mpmath.fp: the same rule in machine arithmetic, ~100 x faster, for the GPU tests; checked against the other below)."""
    import mpmath

    mp = mpmath.mp if multiprecision else mpmath.fp
    with (mpmath.workdps(25) if multiprecision else contextlib.nullcontext()):
        psi, x = mp.mpf(psi), mp.mpf(x)
        tk, cp, sp = mp.pi / 2 - psi, mp.cos(psi), mp.sin(psi)
        if f == "ell":
            if x == 1:
                l = mp.mpf(2)  # noqa: E741
            elif x < 1:
                e = mp.sqrt(1 - x * x)
                l = x + mp.asin(e) / e  # noqa: E741
            else:
                e = mp.sqrt(1 - x ** -2)
                l = x + mp.log((1 + e) / (1 - e)) / (2 * e * x)  # noqa: E741
            g = lambda t: 2 * x ** 3 * mp.sin(t) / (l * (mp.cos(t) ** 2 + x * x * mp.sin(t) ** 2) ** 2)  # noqa: E731
        else:
            g = mp.sin if f == "sin" else (lambda t: mp.cos(x * t))

        def A(t):
            beta = mp.acos(min(mp.mpf(1), mp.cot(t) * mp.cot(psi)))
            return mp.cos(t) * cp * (1 - 2 * beta / mp.pi) + 2 / mp.pi * mp.sin(t) * sp * mp.sin(beta)

        lo = cp * mp.quad(lambda t: g(t) * mp.cos(t), [0, tk]) if tk > 0 else mp.mpf(0)
        hi = mp.quad(lambda t: g(t) * A(t), [tk, mp.pi / 2]) if psi > 0 else mp.mpf(0)
        return float(lo + hi)


def mp_G(kind, p, psi, multiprecision=True):
    """G(psi) of one PDF at the angles ``psi`` by mpmath.  G is linear in g, so the TRIG kinds share three integrals per angle."""
    psi = [float(s) for s in np.atleast_1d(psi)]
    if kind == 0:
        return np.array([_projected(multiprecision, "sin", 0.0, s) for s in psi])
    if kind == 1:
        return np.array([_projected(multiprecision, "ell", float(p[0]), s) for s in psi])
    c0, c2, c4 = (np.array([_projected(multiprecision, "cos", k, s) for s in psi]) for k in (0.0, 2.0, 4.0))
    return 2 / np.pi * (c0 + p[0] * c2 + p[1] * c4)


KINDS = {
    "spherical": (0, (0.0, 0.0)), "ellipsoidal(0.3)": (1, (0.3, 0.0)), "ellipsoidal(1)": (1, (1.0, 0.0)), "ellipsoidal(2.5)": (1, (2.5, 0.0)),
    "uniform": (2, (0.0, 0.0)), "planophile": (2, (1.0, 0.0)), "erectophile": (2, (-1.0, 0.0)), "plagiophile": (2, (0.0, -1.0)),
}
EXTRA_PSI = np.array([0.0, 1e-3, np.deg2rad(20.0), np.deg2rad(75.0), np.deg2rad(89.99), 0.3, 1.0, 1.4, HALF_PI])  # (the last four: the GPU test's)


def target_angles():
    """All 137 nodes of both mu_s (the 105 that do not depend on mu_s once) and the extra angles."""
    from crt1d_amd import _lib

    a, b = _lib.quad_nodes(0.501), _lib.quad_nodes(0.33998)
    assert np.array_equal(a[:96], b[:96]) and np.array_equal(a[128:], b[128:])
    assert HALF_PI - a.max() < 1e-4 * HALF_PI  # psi next to pi/2 occurs among the nodes
    return np.concatenate([a, b[96:128], EXTRA_PSI])


def test_gauss_legendre_nodes(lib):
    from numpy.polynomial.legendre import leggauss

    from crt1d_amd import _lib

    x, w, xm, wm = _lib.leaf_pdf_nodes()
    for n, (xs, ws) in ((_lib.LEAF_NGL, (x, w)), (_lib.LEAF_NMLA, (xm, wm))):
        gx, gw = leggauss(n)
        assert xs.shape == ws.shape == (n,)
        np.testing.assert_allclose(xs, (gx + 1) / 2, rtol=0, atol=2e-16)
        np.testing.assert_allclose(ws, gw / 2, rtol=0, atol=4e-15)
        assert abs(ws.sum() - 1.0) < 2e-15 and np.all(ws > 0) and np.all(np.diff(xs) > 0)
        assert abs(np.sum(ws * xs ** (2 * n - 1)) - 1 / (2 * n)) < 2e-15  # exact for degree 2 n - 1


@pytest.mark.parametrize("name", list(KINDS))
def test_rule_meets_the_bar_against_mpmath(lib, name):
    from crt1d_amd import _lib
    from crt1d_amd import leaf_angle as la

    kind, p = KINDS[name]
    x, w, _, _ = _lib.leaf_pdf_nodes()
    psi = target_angles()
    got = rule_G(kind, p, psi, x, w)
    ref = mp_G(kind, p, psi)
    err = np.abs(got - ref)
    print(f"{name}: worst |G_rule - G_mpmath| = {err.max():.2e} at psi = {psi[err.argmax()]!r}")
    assert err.max() <= BAR, (name, err.max(), psi[err.argmax()])
    # mpmath itself against the closed forms there are
    if kind == 0:
        assert np.max(np.abs(ref - 0.5)) < 1e-15
    if kind == 1:
        assert np.max(np.abs(ref - la.G_ellipsoidal(psi, p[0]))) < 1e-15
    # psi = 0: int g cos(theta), finite
    assert np.isfinite(got).all()
    # the machine-precision form of the same reference, which the GPU tests use
    assert np.max(np.abs(mp_G(kind, p, psi, multiprecision=False) - ref)) < 1e-13


@pytest.mark.parametrize("xv", [0.2, 10.0])
def test_rule_meets_the_bar_at_the_ends_of_the_x_range(lib, xv):
    """The ellipsoidal x the library accepts, [CRT_LEAF_X_MIN, CRT_LEAF_X_MAX]: the rule against Campbell's exact G (which the test above
    shows to be what mpmath integrates to) at both ends, where the PDF's poles are closest to the panels."""
    from crt1d_amd import _lib
    from crt1d_amd import leaf_angle as la

    assert (la.PDF_X_MIN, la.PDF_X_MAX) == (0.2, 10.0)
    x, w, _, _ = _lib.leaf_pdf_nodes()
    psi = target_angles()
    err = np.abs(rule_G(1, (xv, 0.0), psi, x, w) - la.G_ellipsoidal(psi, xv))
    print(f"x = {xv}: worst |G_rule - G_exact| = {err.max():.2e}")
    assert err.max() <= BAR


def test_rule_limits_and_mla():
    """The projection in its limits (G_horizontal / G_vertical for leaves all at one inclination are the limits of A itself), the hand
    values of the two de Wit classes the GPU test uses, and the one-panel mla rule."""
    from crt1d_amd import _lib

    x, w, xm, wm = _lib.leaf_pdf_nodes()
    # erectophile: G(0) = int (2/pi)(1 - cos 2t) cos t dt = (2/pi)(1 - 1/3) = 4/(3 pi); planophile: G(0) = (2/pi)(1 + 1/3) = 8/(3 pi)
    assert abs(rule_G(2, (-1.0, 0.0), [0.0], x, w)[0] - 4 / (3 * np.pi)) < 1e-15
    assert abs(rule_G(2, (1.0, 0.0), [0.0], x, w)[0] - 8 / (3 * np.pi)) < 1e-15
    # psi = pi/2: G = (2/pi) int g sin t dt: planophile (2/pi)^2 (1 - 1/3), erectophile (2/pi)^2 (1 + 1/3), uniform (2/pi)^2
    for (a, b), val in (((1.0, 0.0), 2 / 3), ((-1.0, 0.0), 4 / 3), ((0.0, 0.0), 1.0)):
        assert abs(rule_G(2, (a, b), [HALF_PI], x, w)[0] - (2 / np.pi) ** 2 * val) < 1e-14
    th = HALF_PI * xm
    g = load_golden("g11_leaf_pdf")
    mla = lambda kind, p: np.rad2deg(HALF_PI * np.sum(wm * th * rule_pdf(kind, p, np.sin(th), np.cos(th))))  # noqa: E731
    assert abs(mla(0, (0, 0)) - np.rad2deg(1.0)) < 1e-12 and abs(mla(2, (0, 0)) - 45.0) < 1e-12
    for name, ref in zip(g["names"], g["mla"]):
        assert abs(mla(*KINDS[str(name)]) - ref) < 1e-7, name  # the reference's quad at its default tolerance
    for xv, ref in zip(g["x"], g["mla_ell"]):
        assert abs(mla(1, (float(xv), 0.0)) - ref) < 1e-7, xv
