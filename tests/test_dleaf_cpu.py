"""CPU: the leaf-angle-derivative entry points (include/crt1d_hip_dleaf.h) exist next to an unchanged crt1d_hip.h, every argument error
and every unsupported scheme or depth is found before any launch, the plans' own checks -- and the device's rules for

    tau_d^th(L) = -2 int_0^{pi/2} K_b'(psi) L e^{-K_b(psi) L} sin psi cos psi dpsi        mu_bar' = -int_0^{pi/2} cos psi sin psi dG / G^2 dpsi

(csrc/dleaf.hip: the nodes and weights of tau_d and mu_bar with the differentiated integrands), rebuilt on the host from
crt_hip_quad_nodes, against converged mpmath integrals on the ten leaf-angle classes of tests/domain_cases.py and the L grid of
tests/test_quadrature_domain_cpu.py, {1e-6 .. 12}.  The direction is dG / d g_param for the parametric classes (Bonan: the unclamped
one-sided derivative at both ends of the clamp) and dG = G (cos psi - 1/4) for the parameterless ones: a relative change of G, so that
dG / G^2 stays integrable where G vanishes (horizontal leaves at pi/2, vertical ones at 0).  The mpmath values are accepted by the procedure of tests/test_dtau_d_quadrature_cpu.py
(30 digits against 60 digits with more pieces, 1e-20).

Measured (x86-64, glibc, NumPy 2.2): the tables DEVICE_DTAU_LEAF and DEVICE_DMUBAR below, asserted at twice their figures, each
relative to the rule's sum of magnitudes.  The integrand of tau_d^th carries the boundary layer of tau_d next to psi = pi/2, so small L
is limited as tau_d' is: 5.5e-11 for L >= 1e-3 on every class but Bonan chi_l = 0.6 (1.3e-7 at 1e-3, 1.1e-8 at 1e-2, where
G(pi/2) = 0.0014 puts the layer inside the finest panel up to L ~ 1e-2), to 3.3e-9 at 3e-4 and 3.6e-7 at L = 1e-6.  mu_bar' is good to
3.0e-11 (ellipsoidal x = 0.2)."""
import ctypes
import os
import re

import numpy as np
import pytest

from domain_cases import BONAN, CLASSES, ELLIPSOIDAL, ELLIPSOIDAL_APPROX, HORIZONTAL, SPHERICAL, G_np, device_rule
from test_quadrature_domain_cpu import L_GRID, T, _mp_G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
SERVED = ["2s", "bl", "g77", "bf", "n79", "zq"]
NAMES = ["crt_hip_dtau_d_dleaf_f64", "crt_hip_g_dparam_f64", "crt_hip_levels_dleaf_f64", "crt_hip_levels_dleaf_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_dleaf_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = _declared("crt1d_hip_dleaf.h")
    assert names == sorted(_lib.DLEAF_EXPORTS) == NAMES
    for name in names:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.JAC_EXPORTS and name not in _lib.DLAI_EXPORTS
    # crt1d_hip.h keeps its symbol set and its version, crt1d_hip_dlai.h its set
    assert _declared("crt1d_hip.h") == sorted(_lib.EXPORTS) and len(_lib.EXPORTS) == 57
    assert _declared("crt1d_hip_dlai.h") == sorted(_lib.DLAI_EXPORTS) and len(_lib.DLAI_EXPORTS) == 3
    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


def test_leaf_tangent_layout():
    from crt1d_amd import _lib

    keys = ["dg_table", "dg_at_psi", "dmla"]
    assert ctypes.sizeof(_lib.CrtLeafTangent) == 24
    assert [f[0] for f in _lib.CrtLeafTangent._fields_] == keys
    assert [getattr(_lib.CrtLeafTangent, k).offset for k in keys] == [0, 8, 16]
    text = open(os.path.join(ROOT, "include", "crt1d_hip_dleaf.h")).read()
    m = re.search(r"typedef struct crt_leaf_tangent \{(.*?)\} crt_leaf_tangent;", text, re.S)
    assert re.findall(r"\*\s*(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == keys


def _args(nz=20, nb=8, ncol=2):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no
    workspace -> CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(ncol, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    out = _lib.CrtDlaiOut(FAKE, FAKE, FAKE, FAKE)
    tan = _lib.CrtLeafTangent(FAKE, FAKE, None)
    return c, b, o, out, tan


def _call(lib, scheme, c, b, o, levels, out, tan, nsel=None, ws=None, wsb=0):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    return lib.crt_hip_levels_dleaf_f64(sid, ref(c), ref(b), ref(o), arr, n, ref(tan), ref(out), ws, wsb, None)


@pytest.mark.parametrize("scheme", SERVED)
def test_dleaf_validation_without_gpu(lib, scheme):
    from crt1d_amd import _lib

    BAD, WS, nz, nb = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, 20, 8
    c, b, o, out, tan = _args(nz, nb)

    def call(c=c, b=b, o=o, levels=(0, nz - 1), out=out, tan=tan, scheme=scheme, nsel=None, **kw):
        return _call(lib, scheme, c, b, o, None if levels is None else list(levels), out, tan, nsel, **kw)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    sid = _lib.SCHEME_IDS[scheme]
    need = lib.crt_hip_levels_dleaf_workspace_bytes(sid, 2, nz, nb, 2)
    assert need > 0 and call(ws=FAKE, wsb=need - 1) == WS  # a short workspace
    assert call(ws=FAKE, wsb=lib.crt_hip_workspace_bytes_nb(sid, 2, nz, nb)) == WS  # the K0 records alone do not do, for any scheme
    assert call(tan=_lib.CrtLeafTangent(FAKE, FAKE, FAKE)) == WS  # with dmla
    for one in range(4):  # any single output is enough
        assert call(out=_lib.CrtDlaiOut(*[FAKE if i == one else None for i in range(4)])) == WS
    # the tangent
    assert call(tan=None) == BAD
    assert call(tan=_lib.CrtLeafTangent(None, FAKE, None)) == BAD
    assert call(tan=_lib.CrtLeafTangent(FAKE, None, FAKE)) == BAD
    # the outputs
    assert call(out=None) == BAD
    assert call(out=_lib.CrtDlaiOut(None, None, None, None)) == BAD
    # everything the levels entry rejects
    assert call(c=None) == BAD
    assert call(b=None) == BAD
    assert call(levels=None, nsel=1) == BAD
    assert call(nsel=0) == BAD
    c100 = _args(100, nb)[0]
    assert call(c=c100, levels=range(64)) == WS
    assert call(c=c100, levels=range(65)) == BAD
    assert call(levels=(3, 2)) == BAD
    assert call(levels=(2, 2)) == BAD
    assert call(levels=(-1,)) == BAD
    assert call(levels=(nz,)) == BAD
    assert call(scheme=42) == BAD
    assert call(scheme=-1) == BAD
    assert call(o=_lib.set_tune(_lib.CrtOptions(0.501, 0, 0), {_lib.TUNE_TRI_M: 10})) == BAD
    assert call(o=_lib.CrtOptions(0.501, 5, 0)) == BAD
    assert call(b=_lib.CrtBands(nb, nb - 1, FAKE, FAKE, FAKE, FAKE, FAKE)) == BAD  # col_stride neither 0 nor >= nb
    assert call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, None, FAKE, FAKE)) == BAD  # no leaf_r
    soilless = call(b=_lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, None))
    assert soilless == (WS if scheme == "bl" else BAD)
    # CRT_ERR_SHAPE as crt_hip_levels_f64: nz < 2; n79: nz < 3
    assert call(c=_args(1, nb)[0], levels=(0,)) == _lib.CRT_ERR_SHAPE
    assert call(c=_args(2, nb)[0], levels=(0, 1)) == (_lib.CRT_ERR_SHAPE if scheme == "n79" else WS)


@pytest.mark.parametrize("scheme", ["4s", "zq_pa"])
def test_dleaf_schemes_not_served(lib, scheme):
    """4s and zq_pa: CRT_ERR_UNSUPPORTED whatever the workspace, after the argument and shape errors (the precedence of
    crt_hip_levels_dlai_f64)."""
    from crt1d_amd import _lib

    c, b, o, out, tan = _args()
    assert _call(lib, scheme, c, b, o, [0, 19], out, tan) == _lib.CRT_ERR_UNSUPPORTED
    assert _call(lib, scheme, c, b, o, [0, 19], out, tan, ws=FAKE, wsb=1 << 30) == _lib.CRT_ERR_UNSUPPORTED
    assert _call(lib, scheme, c, b, o, [19, 0], out, tan) == _lib.CRT_ERR_BAD_ARG  # an argument error is still one
    assert _call(lib, scheme, c, b, o, [0, 19], None, tan) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, o, [0, 19], out, None) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, None, o, [0, 19], out, tan) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, _lib.CrtBands(8, 8, FAKE, FAKE, None, FAKE, FAKE), o, [0, 19], out, tan, ws=FAKE, wsb=1 << 30) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, c, b, _lib.CrtOptions(0.501, 5, 0), [0, 19], out, tan) == _lib.CRT_ERR_BAD_ARG
    assert _call(lib, scheme, _args(1)[0], b, o, [0], out, tan) == _lib.CRT_ERR_SHAPE


@pytest.mark.parametrize("scheme", ["n79", "zq"])
def test_dleaf_depth_limit_without_gpu(lib, scheme):
    """One level past the depth k_dlai_tri serves: CRT_ERR_UNSUPPORTED before K0 (the fake pointers are never used); at the limit the
    call would launch, so only the workspace check is exercised there."""
    from crt1d_amd import _lib

    lim = _lib.DLAI_MAX_NZ[scheme]
    sid = _lib.SCHEME_IDS[scheme]
    for nb in (1, 300):
        c, b, o, out, tan = _args(lim + 1, nb, ncol=1)
        need = lib.crt_hip_levels_dleaf_workspace_bytes(sid, 1, lim + 1, nb, 2)
        assert need > 0
        assert _call(lib, scheme, c, b, o, [0, lim], out, tan, ws=FAKE, wsb=need) == _lib.CRT_ERR_UNSUPPORTED
        assert _call(lib, scheme, c, b, o, [0, lim], out, tan) == _lib.CRT_ERR_WORKSPACE  # the workspace comes before the depth
        c, b, o, out, tan = _args(lim, nb, ncol=1)
        assert _call(lib, scheme, c, b, o, [0, lim - 1], out, tan) == _lib.CRT_ERR_WORKSPACE


def test_dleaf_workspace_query(lib):
    from crt1d_amd import _lib

    q = lib.crt_hip_levels_dleaf_workspace_bytes
    side = {"bl": lambda nz: 16 + nz, "n79": lambda nz: 16 + 3 * nz, "zq": lambda nz: 16 + nz}
    for scheme, sid in _lib.SCHEME_IDS.items():
        for nz, nb in ((20, 8), (150, 300), (3, 2151)):
            rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, nb)
            assert rec > 0
            want = rec + 5 * 8 * side.get(scheme, lambda nz: 16)(nz)  # the K0 records, a side record per column behind them
            assert q(sid, 5, nz, nb, 2) == q(sid, 5, nz, nb, 64) == want
    for bad in ((42, 5, 20, 8, 2), (-1, 5, 20, 8, 2), (0, 0, 20, 8, 2), (0, 5, 0, 8, 2), (0, 5, 20, 0, 2), (0, 5, 20, 8, 0), (0, 5, 20, 8, 65),
                (0, -3, 20, 8, 2)):
        assert q(*bad) == 0, bad


def test_helpers_validation_without_gpu(lib):
    from crt1d_amd import _lib

    f = lib.crt_hip_dtau_d_dleaf_f64
    assert f(None, FAKE, FAKE, 4, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, None, FAKE, 4, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, None, 4, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, FAKE, 4, 0, None, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, FAKE, -1, 0, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, FAKE, 4, 2, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert f(FAKE, FAKE, FAKE, 0, 1, FAKE, None) == _lib.CRT_OK  # nothing to do, nothing launched
    g = lib.crt_hip_g_dparam_f64
    c = _args()[0]
    assert g(None, FAKE, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert g(ctypes.byref(c), None, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert g(ctypes.byref(c), FAKE, None, None) == _lib.CRT_ERR_BAD_ARG
    assert g(ctypes.byref(_lib.CrtColumns(0, 20, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)), FAKE, FAKE, None) == _lib.CRT_ERR_BAD_ARG
    assert g(ctypes.byref(_lib.CrtColumns(2, 20, None, FAKE, FAKE, FAKE, FAKE, None, None)), FAKE, FAKE, None) == _lib.CRT_ERR_BAD_ARG  # no psi
    assert g(ctypes.byref(_lib.CrtColumns(2, 20, FAKE, FAKE, FAKE, None, FAKE, None, None)), FAKE, FAKE, None) == _lib.CRT_ERR_BAD_ARG  # no g_kind


def test_dleaf_plan_python_errors_need_no_device():
    from crt1d_amd import batched

    assert batched.DLEAF_KEYS == ("I_dr", "I_df_d", "I_df_u", "F") and batched.DLEAF_SCHEMES == tuple(SERVED)
    assert batched.LEAF_WRT == ("param", "mla", "a", "b")
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.LevelsDleafPlan("nope", None, None, (0,), None)
    with pytest.raises(ValueError, match="invalid `method`"):
        batched.LevelsDleafPlan("2s", None, None, (0,), None, tau_d_method="nope")
    for scheme in ("4s", "zq_pa"):
        with pytest.raises(ValueError, match="has no leaf-angle-derivative kernel"):
            batched.LevelsDleafPlan(scheme, None, None, (0,), None)
        with pytest.raises(ValueError, match="has no leaf-angle-derivative kernel"):
            batched.solve_levels_dleaf(scheme, None, None, (0,), None)
    for keys in (("x0",), ("F", "F"), (), ("I_d",)):
        with pytest.raises(ValueError, match="keys must be distinct"):
            batched.LevelsDleafPlan("2s", None, None, (0,), None, keys=keys)
    with pytest.raises(TypeError, match="tangent must be a LeafTangent"):
        batched.LevelsDleafPlan("2s", None, None, (0,), np.ones(3))
    with pytest.raises(TypeError, match="must be a SensorSet"):
        batched.sensor_dleaf("2s", None, None, (0,), None, np.ones((2, 8)))
    with pytest.raises(ValueError, match="wrt must be one of"):
        batched.leaf_tangent(None, wrt="x")
    with pytest.raises(ValueError, match="unknown scheme"):
        batched.solve_levels_dleaf("nope", None, None, (0,), None)
    with pytest.raises(ValueError, match="invalid `method`"):
        batched.solve_levels_dleaf("n79", None, None, (0,), None, tau_d_method="nope")


# ------------------------------------------------------------------------------------------------------------------
# the two rules against mpmath


def _ell_den(x, lib=np):
    """(p2, dp2 / dx) of the exact ellipsoidal G: p2 = x + A(u), u = 1 - x^2, A' = (1 / x - A) / (2 u); x = 1: (2, 2 / 3)."""
    if x == 1:
        return (2.0, 2.0 / 3) if lib is np else (lib.mpf(2), lib.mpf(2) / 3)
    if x > 1:
        e = lib.sqrt(1 - x**-2)
        A = lib.log((1 + e) / (1 - e)) / (2 * e * x)
    else:
        e = lib.sqrt(1 - x**2)
        A = (lib.arcsin if lib is np else lib.asin)(e) / e
    return x + A, 1 - 2 * x * (1 / x - A) / (2 * (1 - x * x))


def dG_direction(kind, x, c, s, lib=np):
    """The test's leaf-angle direction of a class (module docstring) from (cos psi, sin psi); ``lib``: numpy or mpmath."""
    if kind == HORIZONTAL:
        return c * (c - 0.25)
    if kind in (ELLIPSOIDAL, ELLIPSOIDAL_APPROX):
        if kind == ELLIPSOIDAL:
            p, dp = _ell_den(x, lib)
        else:
            p, dp = x + 1.774 * (x + 1.182) ** -0.733, 1 - 0.733 * 1.774 * (x + 1.182) ** -1.733  # (the constants at their double values)
        R = lib.sqrt(x * x * c * c + s * s)
        return x * c * c / (R * p) - R * dp / (p * p)
    if kind == BONAN:
        return (-0.633 - 2 * 0.330 * x) * (1 - 2 * 0.877 * c)
    return (0.5 if kind == SPHERICAL else 2 / lib.pi * s) * (c - 0.25)  # spherical, vertical


def _mp_leaf(dps, kmax, more):
    """{(class, L) | (class, "mu_bar"): mpf} at ``dps`` digits; pieces as tests/test_dtau_d_quadrature_cpu.py."""
    import mpmath as mp

    out = {}
    with mp.workdps(dps):
        Tm = mp.pi / 2
        pts = [mp.mpf(0)] + [Tm * mp.mpf(10) ** -k for k in range(kmax, 0, -1)] + [Tm]
        if more:
            pts = sorted(pts + [3 * Tm * mp.mpf(10) ** -k for k in range(1, 9)] + [Tm * mp.mpf("0.6")])
        for name, kind, param in CLASSES:
            G = _mp_G(mp, kind, param)
            x = mp.mpf(param)
            for L in L_GRID:
                Lm = mp.mpf(L)

                def f(t):
                    c, s = mp.sin(t), mp.cos(t)  # cos psi, sin psi
                    return -dG_direction(kind, x, c, s, mp) * Lm * mp.exp(-G(c, s) * Lm / c) * s  # -K' L e^{-K L} sin cos, K = G / cos

                out[name, L] = 2 * mp.quad(f, pts, method="gauss-legendre")

            def fm(t):
                c, s = mp.sin(t), mp.cos(t)
                return -c * s * dG_direction(kind, x, c, s, mp) / G(c, s) ** 2

            out[name, "mu_bar"] = mp.quad(fm, pts, method="gauss-legendre")
    return out


@pytest.fixture(scope="module")
def mpref():
    a = _mp_leaf(30, 14, False)
    b = _mp_leaf(60, 16, True)
    worst = max(float(abs(a[k] - b[k]) / abs(b[k])) for k in a)
    print(f"mpmath 30 digits vs 60 digits with more pieces: {worst:.1e}")
    assert worst < 1e-20, worst
    return {k: float(v) for k, v in a.items()}


def host_dtau_d_dleaf_quad(kb_nodes, dkb_nodes, L):
    """The device's 'quad' rule for tau_d^th on the host: K_b and K_b' at the 96 tau_d nodes -> tau_d^th(L)."""
    t, wt = device_rule()
    k, dk = np.asarray(kb_nodes)[:96], np.asarray(dkb_nodes)[:96]
    L = np.asarray(L, dtype=np.float64)
    return -(np.multiply.outer(L, dk) * np.exp(-np.multiply.outer(L, k))) @ (2 * wt * np.cos(t) * np.sin(t))


def host_dtau_d_dleaf_9sky(k9, dk9, L):
    """The nine-term sum of the '9sky' form (common.py:40-53 with the factor -K_b' L e^{-K_b L})."""
    psi = np.radians(5.0 + 10.0 * np.arange(9))
    L = np.asarray(L, dtype=np.float64)
    return -(np.multiply.outer(L, np.asarray(dk9)) * np.exp(-np.multiply.outer(L, np.asarray(k9)))) @ (np.sin(psi) * np.cos(psi)) * (2 * np.radians(10.0))


def host_dmubar(g, dg):
    """The device's rule for mu_bar' on the host from G and dG at the 96 tau_d nodes."""
    t, wt = device_rule()
    return np.sum(wt * np.sin(t) * np.cos(t) / g * -(dg / g))


# Error of tau_d^th(L) by the device's rule against mpmath, relative to M(L) = 2 sum_q w_q sin cos |Kq'| L e^{-Kq L}, the rule's sum of
# magnitudes: the direction of a normalised G changes sign over psi, so the value itself nearly cancels (ellipsoidal x = 10 at L = 1e-6:
# 2.4e-14 out of M = 6e-9) while the schemes take the error in absolute terms; where the direction keeps its sign M is |tau_d^th|.
# Measured; columns = L_GRID.  Entries at rounding level are recorded as 1e-15.
#                      L = 1e-6    1e-5     1e-4     3e-4     1e-3     1e-2     0.1      1        12
DEVICE_DTAU_LEAF = {
    "horizontal":       (1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15,   1e-15),
    "spherical":        (5.7e-08, 1.4e-08, 1.7e-10, 6.9e-13, 9.0e-13, 5.1e-13, 1.7e-12, 1.8e-14, 7.1e-15),
    "vertical":         (4.9e-08, 2.5e-08, 9.0e-11, 2.1e-12, 1.6e-12, 7.5e-13, 2.2e-12, 2.3e-14, 1e-15),
    "ellipsoidal_x0.2": (4.4e-08, 2.2e-08, 9.2e-11, 2.2e-12, 1.6e-12, 2.5e-13, 1.7e-12, 7.6e-13, 9.6e-12),
    "ellipsoidal_x1":   (9.2e-08, 2.2e-08, 2.8e-10, 1.1e-12, 1.5e-12, 7.9e-13, 3.1e-12, 1.8e-14, 8.7e-15),
    "ellipsoidal_x10":  (3.6e-07, 6.6e-08, 1.2e-08, 3.3e-09, 5.4e-11, 4.6e-12, 9.1e-12, 1.2e-11, 9.2e-12),
    "approx_x0.2":      (4.5e-08, 2.2e-08, 9.5e-11, 2.2e-12, 1.7e-12, 2.6e-13, 1.7e-12, 7.6e-13, 9.6e-12),
    "approx_x10":       (3.6e-07, 6.6e-08, 1.2e-08, 3.3e-09, 5.5e-11, 4.6e-12, 9.2e-12, 1.2e-11, 9.2e-12),
    "bonan_-0.4":       (5.6e-08, 3.9e-08, 1.5e-12, 2.2e-12, 2.9e-12, 2.5e-12, 1.3e-12, 1.4e-13, 1.0e-14),
    "bonan_0.6":        (1.7e-08, 9.4e-08, 2.9e-07, 2.0e-07, 1.3e-07, 1.1e-08, 7.9e-12, 4.2e-12, 3.9e-12),
}
# error of mu_bar' by the device's rule relative to sum_q w_q cos sin |dG_q| / G_q^2, measured (rounding level recorded as 1e-15)
DEVICE_DMUBAR = {"horizontal": 1e-15, "spherical": 1e-15, "vertical": 1e-15, "ellipsoidal_x0.2": 3.0e-11, "ellipsoidal_x1": 1e-15,
                 "ellipsoidal_x10": 4.9e-13, "approx_x0.2": 3.0e-11, "approx_x10": 4.9e-13, "bonan_-0.4": 1e-15, "bonan_0.6": 1.2e-12}


def _nodes_G_dG(kind, x):
    t, _ = device_rule()
    c, s = np.sin(t), np.cos(t)  # cos psi = sin t keeps its accuracy next to pi/2
    return G_np(kind, x, c, s), dG_direction(kind, x, c, s), c


def test_device_leaf_rules_vs_mpmath(mpref):
    """Per class and L, asserted at twice the measured figures (the convention of the tau_d' table)."""
    from crt1d_amd import _lib

    t, _ = device_rule()
    np.testing.assert_allclose(_lib.quad_nodes(0.501)[:96], T - t, rtol=0, atol=2e-16)
    over = []
    for name, kind, x in CLASSES:
        g, dg, c = _nodes_G_dG(kind, x)
        got, mag = host_dtau_d_dleaf_quad(g / c, dg / c, L_GRID), -host_dtau_d_dleaf_quad(g / c, np.abs(dg) / c, L_GRID)
        err = [abs(got[i] - mpref[name, L]) / mag[i] for i, L in enumerate(L_GRID)]
        e_mb = abs(host_dmubar(g, dg) - mpref[name, "mu_bar"]) / -host_dmubar(g, np.abs(dg))
        print(f"device tau_d^th rule {name:18s} " + " ".join(f"{e:.1e}" for e in err) + f" | mu_bar' {e_mb:.1e}")
        over += [(name, L, err[i]) for i, L in enumerate(L_GRID) if err[i] > 2 * DEVICE_DTAU_LEAF[name][i]]
        if e_mb > 2 * DEVICE_DMUBAR[name]:
            over.append((name, "mu_bar'", e_mb))
    assert not over, over  # (after the whole table is printed)


def test_9sky_is_its_nine_term_sum():
    """'9sky' has no truncation error to measure: it IS nine terms.  Two ways of forming the sum agree to 1e-14 of the largest term."""
    psi = np.radians(5.0 + 10.0 * np.arange(9))
    c, s = np.cos(psi), np.sin(psi)
    for name, kind, x in CLASSES:
        k9, dk9 = G_np(kind, x, c, s) / c, dG_direction(kind, x, c, s) / c
        got = host_dtau_d_dleaf_9sky(k9, dk9, L_GRID)
        for i, L in enumerate(L_GRID):
            terms = [-dk * L * np.exp(-kk * L) * np.sin(p) * np.cos(p) * 2 * np.radians(10.0) for kk, dk, p in zip(k9, dk9, psi)]
            assert abs(got[i] - sum(terms)) <= 1e-14 * max(abs(v) for v in terms), (name, L)
