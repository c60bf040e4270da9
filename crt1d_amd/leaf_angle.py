"""
Leaf-angle projection functions G(psi) for the batched canopy-RT path.

Mirrors the ``G_*`` family of the reference (``crt1d/leaf_angle.py:118-202``) but as
*descriptors*: a :class:`GFunction` is callable like the reference's plain functions
(``G_fn(psi)``) and additionally carries ``kind``/``param`` so the HIP column-precompute
kernel can evaluate the same closed form on device instead of receiving a table.

Arbitrary Python callables are still accepted everywhere a ``G_fn`` is expected: the host
wrapper samples them at the library's fixed quadrature nodes (kind ``G_TABLE``).

Device kind ids (must match ``include/crt1d_hip.h``):

== =========================== ==============================================
0  ``G_HORIZONTAL``            cos(psi)                      (ref :118-120)
1  ``G_SPHERICAL``             0.5                           (ref :123-125)
2  ``G_VERTICAL``              2/pi sin(psi)                 (ref :128-130)
3  ``G_ELLIPSOIDAL``           Campbell (1986) exact, x      (ref :133-165)
4  ``G_ELLIPSOIDAL_APPROX``    Campbell (1990) approx, x     (ref :168-180)
5  ``G_ELLIPSOIDAL_APPROX_BONAN`` Ross-Goudriaan, chi_l      (ref :183-202)
6  ``G_TABLE``                 host-sampled callable
== =========================== ==============================================

A canopy may instead be described by its leaf-inclination PDF ``g(theta_l)`` (``g_*`` below, ref ``:31-79``): a :class:`LeafPDF` names
one of the device's PDF kinds, and ``crt_hip_g_from_pdf_f64`` integrates it into the ``G_TABLE`` arrays (and ``mla``, ref ``:82-87``) on
the device, one launch for any number of columns (:func:`crt1d_amd.batched.leaf_pdf_tables`).
"""

import math

import numpy as np

G_HORIZONTAL = 0
G_SPHERICAL = 1
G_VERTICAL = 2
G_ELLIPSOIDAL = 3
G_ELLIPSOIDAL_APPROX = 4
G_ELLIPSOIDAL_APPROX_BONAN = 5
G_TABLE = 6

KIND_NAMES = {
    G_HORIZONTAL: "horizontal",
    G_SPHERICAL: "spherical",
    G_VERTICAL: "vertical",
    G_ELLIPSOIDAL: "ellipsoidal",
    G_ELLIPSOIDAL_APPROX: "ellipsoidal_approx",
    G_ELLIPSOIDAL_APPROX_BONAN: "ellipsoidal_approx_bonan",
    G_TABLE: "table",
}


def _ellipsoidal_denominator(x):
    """Campbell (1986) eq. 6 surface-area ratio term (ref ``leaf_angle.py:155-162``)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.full(x.shape, 2.0)
    gt = x > 1
    lt = x < 1
    if np.any(gt):
        e1 = np.sqrt(1 - x[gt] ** -2)
        out[gt] = x[gt] + np.log((1 + e1) / (1 - e1)) / (2 * e1 * x[gt])
    if np.any(lt):
        e2 = np.sqrt(1 - x[lt] ** 2)
        out[lt] = x[lt] + np.arcsin(e2) / e2
    return out


def eval_G(kind, param, psi):
    """Vectorised G(psi) for parameterised kinds; ``kind``/``param``/``psi`` broadcast.

    Uses the tan-free form sqrt(x^2 cos^2 + sin^2)/p2, algebraically equal to the
    reference's sqrt(x^2 + tan^2)/p2 * cos but finite at psi = pi/2.
    """
    kind = np.asarray(kind)
    param = np.asarray(param, dtype=np.float64)
    psi = np.asarray(psi, dtype=np.float64)
    kind, param, psi = np.broadcast_arrays(kind, param, psi)
    out = np.empty(psi.shape, dtype=np.float64)
    c = np.cos(psi)
    s = np.sin(psi)
    m = kind == G_HORIZONTAL
    out[m] = c[m]
    m = kind == G_SPHERICAL
    out[m] = 0.5
    m = kind == G_VERTICAL
    out[m] = 2 / math.pi * s[m]
    m = kind == G_ELLIPSOIDAL
    if np.any(m):
        x = param[m]
        g = np.sqrt(x * x * c[m] ** 2 + s[m] ** 2) / _ellipsoidal_denominator(x)
        out[m] = np.where(x == 1, 0.5, g)
    m = kind == G_ELLIPSOIDAL_APPROX
    if np.any(m):
        x = param[m]
        p2 = x + 1.774 * (x + 1.182) ** -0.733
        out[m] = np.sqrt(x * x * c[m] ** 2 + s[m] ** 2) / p2
    m = kind == G_ELLIPSOIDAL_APPROX_BONAN
    if np.any(m):
        chil = np.clip(param[m], -0.4, 0.6)
        phi1 = 0.5 - 0.633 * chil - 0.330 * chil**2
        phi2 = 0.877 * (1 - 2 * phi1)
        out[m] = phi1 + phi2 * c[m]
    if np.any(kind == G_TABLE):
        raise ValueError("G_TABLE columns have no closed form; sample the callable instead")
    return out


class GFunction:
    """Callable G(psi) that also tells the device which closed form it is."""

    __slots__ = ("kind", "param")

    def __init__(self, kind, param=0.0):
        if kind not in KIND_NAMES or kind == G_TABLE:
            raise ValueError(f"invalid parameterised G kind {kind!r}")
        self.kind = int(kind)
        self.param = float(param)

    def __call__(self, psi):
        res = eval_G(self.kind, self.param, psi)
        return float(res) if res.ndim == 0 else res

    def __repr__(self):
        return f"GFunction({KIND_NAMES[self.kind]}, param={self.param!r})"


def G_horizontal(psi):
    return GFunction(G_HORIZONTAL)(psi)


def G_spherical(psi):
    return GFunction(G_SPHERICAL)(psi)


def G_vertical(psi):
    return GFunction(G_VERTICAL)(psi)


def G_ellipsoidal(psi, x):
    return GFunction(G_ELLIPSOIDAL, x)(psi)


def G_ellipsoidal_approx(psi, x):
    return GFunction(G_ELLIPSOIDAL_APPROX, x)(psi)


def G_ellipsoidal_approx_bonan(psi, xl):
    return GFunction(G_ELLIPSOIDAL_APPROX_BONAN, xl)(psi)


# tag the plain functions so wrappers can recognise the parameter-free ones by identity
G_horizontal.gfunction = GFunction(G_HORIZONTAL)
G_spherical.gfunction = GFunction(G_SPHERICAL)
G_vertical.gfunction = GFunction(G_VERTICAL)


def mla_to_x_approx(mla):
    """Mean leaf angle (deg) -> ellipsoidal x; Campbell (1990) eq. 16 inverted
    (ref ``leaf_angle.py:222-229``). Vectorised."""
    x = (np.deg2rad(mla) / 9.65) ** (-1.0 / 1.65) - 3.0
    if np.any(np.asarray(x) <= 0):
        raise AssertionError("x > 0 required")
    return x


def x_to_mla_approx(x):
    """Ellipsoidal x -> mean leaf angle (deg); ref ``leaf_angle.py:205-211``."""
    return np.rad2deg(9.65 * (3 + np.asarray(x, dtype=np.float64)) ** (-1.65))


def describe_G(G_fn):
    """Return ``(kind, param)`` for a :class:`GFunction`-like ``G_fn``, else ``None``."""
    g = getattr(G_fn, "gfunction", G_fn)
    if isinstance(g, GFunction):
        return g.kind, g.param
    return None


# ---- leaf-inclination PDFs g(theta_l), theta_l from the horizontal (ref ``leaf_angle.py:31-79``) -----------------------------------
# device kind ids (must match ``include/crt1d_hip_leaf.h``)
PDF_SPHERICAL = 0
PDF_ELLIPSOIDAL = 1
PDF_TRIG = 2

PDF_KIND_NAMES = {PDF_SPHERICAL: "spherical", PDF_ELLIPSOIDAL: "ellipsoidal", PDF_TRIG: "trig"}
# ellipsoidal x the device's fixed rule is validated for (CRT_LEAF_X_MIN / CRT_LEAF_X_MAX; outside, the PDF's poles come too close to
# the panels for 1e-11 in G and the library refuses the column)
PDF_X_MIN, PDF_X_MAX = 0.2, 10.0


def _trig_pdf(theta_l, a, b):
    theta_l = np.asarray(theta_l, dtype=np.float64)
    return 2 / math.pi * (1 + a * np.cos(2 * theta_l) + b * np.cos(4 * theta_l))


def g_spherical(theta_l):
    """PDF of the spherical distribution (ref ``:31-35``)."""
    return np.sin(theta_l)


def g_uniform(theta_l):
    """PDF of the uniform distribution (ref ``:38-42``): 2/pi at every inclination, a float for a scalar argument."""
    flat = np.full(np.shape(theta_l), 2 / math.pi)
    return float(flat) if flat.ndim == 0 else flat


def g_planophile(theta_l):
    """PDF of a mostly horizontal distribution (ref ``:45-47``)."""
    return 2 / math.pi * (1 + np.cos(2 * theta_l))


def g_erectophile(theta_l):
    """PDF of a mostly vertical distribution (ref ``:50-52``)."""
    return 2 / math.pi * (1 - np.cos(2 * theta_l))


def g_plagiophile(theta_l):
    """PDF of a distribution between horizontal and vertical (ref ``:55-57``)."""
    return 2 / math.pi * (1 - np.cos(4 * theta_l))


def g_ellipsoidal(theta_l, x):
    """PDF of the ellipsoidal distribution with parameter ``x`` (ref ``:60-79``; Bonan 2019 eqs. 2.11-14): the normalisation is the
    denominator of Campbell's exact G, ``_ellipsoidal_denominator``."""
    sn, cs = np.sin(theta_l), np.cos(theta_l)
    return 2 * x**3 * sn / (float(_ellipsoidal_denominator(x)) * (cs**2 + x**2 * sn**2) ** 2)


def trig_pdf_is_nonnegative(a, b):
    """Whether ``(2/pi)(1 + a cos 2t + b cos 4t) >= 0`` on [0, pi/2]: with u = cos 2t the quadratic ``1 + a u + b (2 u^2 - 1)`` at both
    ends of [-1, 1] and at its vertex when that is an interior minimum (the library makes the same test)."""
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b)):
        return False
    if not (1 + a + b >= 0 and 1 - a + b >= 0):
        return False
    return not (b > 0 and abs(a) < 4 * b and not 1 - b - a * a / (8 * b) >= 0)


class LeafPDF:
    """A leaf-inclination PDF the device can integrate: ``LeafPDF(kind, *params)`` with ``kind`` one of ``PDF_SPHERICAL`` (no
    parameter), ``PDF_ELLIPSOIDAL`` (``PDF_X_MIN <= x <= PDF_X_MAX``) and ``PDF_TRIG`` (``a, b`` of ``(2/pi)(1 + a cos 2t + b cos 4t)``), or the named
    constructors.  ``pdf(theta_l)`` is g on the host.  As a ``G_fn`` it is callable: ``G(psi)`` comes from the device kernel
    (``crt_hip_g_from_pdf_f64``), for a scalar or an array of angles in one launch, and the solvers and ``Model`` take the device path for
    the whole table instead of sampling the callable on the host.

    Every call -- ``pdf(psi)``, ``mla()``, ``tables()`` -- is one launch that forms the whole 137-angle table, ``mla`` and the caller's
    angles, with the descriptor read-back and the copies to the host (``g_table`` is a required output of the entry): simple, and cheap
    next to a solve, but not free.  Code that needs G at many angles should pass them in one array."""

    __slots__ = ("kind", "param")

    def __init__(self, kind, *params):
        if kind not in PDF_KIND_NAMES:
            raise ValueError(f"invalid leaf-inclination PDF kind {kind!r}")
        want = {PDF_SPHERICAL: 0, PDF_ELLIPSOIDAL: 1, PDF_TRIG: 2}[kind]
        if len(params) != want:
            raise ValueError(f"a {PDF_KIND_NAMES[kind]} PDF takes {want} parameter(s), got {len(params)}")
        params = tuple(float(v) for v in params)
        if kind == PDF_ELLIPSOIDAL and not PDF_X_MIN <= params[0] <= PDF_X_MAX:
            raise ValueError(f"ellipsoidal x must be in [{PDF_X_MIN}, {PDF_X_MAX}], the range the device rule is validated for")
        if kind == PDF_TRIG and not trig_pdf_is_nonnegative(*params):
            raise ValueError(f"(2/pi)(1 + a cos 2t + b cos 4t) with (a, b) = {params} is negative somewhere in [0, pi/2]")
        self.kind = int(kind)
        self.param = (params + (0.0, 0.0))[:2]

    @classmethod
    def spherical(cls):
        return cls(PDF_SPHERICAL)

    @classmethod
    def ellipsoidal(cls, x):
        return cls(PDF_ELLIPSOIDAL, x)

    @classmethod
    def trig(cls, a, b):
        return cls(PDF_TRIG, a, b)

    @classmethod
    def uniform(cls):
        return cls(PDF_TRIG, 0.0, 0.0)

    @classmethod
    def planophile(cls):
        return cls(PDF_TRIG, 1.0, 0.0)

    @classmethod
    def erectophile(cls):
        return cls(PDF_TRIG, -1.0, 0.0)

    @classmethod
    def plagiophile(cls):
        return cls(PDF_TRIG, 0.0, -1.0)

    def pdf(self, theta_l):
        """g(theta_l) on the host."""
        if self.kind == PDF_SPHERICAL:
            return g_spherical(theta_l)
        if self.kind == PDF_ELLIPSOIDAL:
            return g_ellipsoidal(theta_l, self.param[0])
        return _trig_pdf(theta_l, *self.param)

    def tables(self, psi=None, mu_s=0.501):
        """``(g_table (NQ,), g_at_psi (npsi,), mla)`` of this PDF as NumPy values, from one launch with ``ncol = 1``."""
        from . import batched

        ps = None if psi is None else np.ascontiguousarray(np.atleast_1d(np.asarray(psi, dtype=np.float64)).reshape(1, -1))
        g_table, g_at_psi, mla = batched.leaf_pdf_tables([self.kind], [self.param], mu_s=mu_s, psi=ps)
        return g_table[0].cpu().numpy(), g_at_psi[0].cpu().numpy(), float(mla[0])

    def mla(self):
        """Mean leaf inclination angle (degrees), ``mla_from_g`` of the reference (``:82-87``) on the device."""
        return self.tables()[2]

    def __call__(self, psi):
        psi = np.asarray(psi, dtype=np.float64)
        res = self.tables(psi)[1].reshape(psi.shape)
        return float(res) if res.ndim == 0 else res

    def __eq__(self, other):
        return isinstance(other, LeafPDF) and (self.kind, self.param) == (other.kind, other.param)

    def __hash__(self):
        return hash((self.kind, self.param))

    def __repr__(self):
        return f"LeafPDF({PDF_KIND_NAMES[self.kind]}, param={self.param!r})"
