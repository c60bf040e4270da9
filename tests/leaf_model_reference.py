"""The generalised plate model of include_ext/crt1d_hip_leafmodel.h restated in NumPy: the oracle of tests/test_leaf_model_cpu.py and
tests/test_gpu_leaf_model.py (a helper, not a test).  Every function runs on float64, complex128 and mpmath numbers: the arithmetic is
plain ``+ - * /``, and ``exp``, ``log``, ``sqrt`` and the exponential integral ``E1`` are passed in.

``reference(q, K, n)``: values and partials with respect to ``q = (N, C_0 ..)`` by ``mpmath.diff`` at 50 digits, the same partials by
the complex step (h = 1e-30) in complex128 with ``scipy.special.exp1``, and the difference of the two, the *spread*."""
import functools
import math

import numpy as np

K_MIN, K_MAX = 1e-6, 100.0
ALPHA = 40.0


class NP:
    exp, log, sqrt = staticmethod(np.exp), staticmethod(np.log), staticmethod(np.sqrt)

    @staticmethod
    def E1(k):
        from scipy.special import exp1

        return exp1(k)


class MP:
    @staticmethod
    def _mp():
        import mpmath

        return mpmath

    exp = staticmethod(lambda x: MP._mp().exp(x))
    log = staticmethod(lambda x: MP._mp().log(x))
    sqrt = staticmethod(lambda x: MP._mp().sqrt(x))
    E1 = staticmethod(lambda x: MP._mp().e1(x))


def tav(alpha_deg, n, lib=NP, sin=None):
    """Stern 1964 / Allen 1973: the Fresnel transmittance of the interface averaged over the cone of half-angle ``alpha``."""
    if sin is None:
        sin = math.sin(math.radians(alpha_deg))
    n2 = n * n
    np_, nm = n2 + 1, n2 - 1
    A = (n + 1) * (n + 1) / 2
    k = -(n2 - 1) * (n2 - 1) / 4
    s = sin * sin
    b2 = s - np_ / 2
    b1 = 0 * n if alpha_deg == 90 else lib.sqrt(b2 * b2 + k)
    B = b1 - b2
    ts = (k * k / (6 * B * B * B) + k / B - B / 2) - (k * k / (6 * A * A * A) + k / A - A / 2)
    tp1 = -2 * n2 * (B - A) / (np_ * np_)
    tp2 = -2 * n2 * np_ * lib.log(B / A) / (nm * nm)
    tp3 = n2 * (1 / B - 1 / A) / 2
    tp4 = 16 * n2 * n2 * (n2 * n2 + 1) * lib.log((2 * np_ * B - nm * nm) / (2 * np_ * A - nm * nm)) / (np_ * np_ * np_ * nm * nm)
    tp5 = 16 * n2 * n2 * n2 * (1 / (2 * np_ * B - nm * nm) - 1 / (2 * np_ * A - nm * nm)) / (np_ * np_ * np_)
    return (ts + tp1 + tp2 + tp3 + tp4 + tp5) / (2 * s)


def top_plate(k, n, talf, t90, lib=NP):
    """(Ra, Ta, r, t): the top plate under light inside the cone and an inner plate under isotropic light."""
    tau = (1 - k) * lib.exp(-k) + k * k * lib.E1(k)
    ralf = 1 - talf
    t12 = t90
    r12 = 1 - t12
    t21 = t12 / (n * n)
    r21 = 1 - t21
    den = 1 - r21 * r21 * tau * tau
    Ta = talf * tau * t21 / den
    Ra = ralf + r21 * tau * Ta
    t = t12 * tau * t21 / den
    r = r12 + r21 * tau * t
    return Ra, Ta, r, t


def plate(N, k, n, talf, t90, lib=NP):
    """(leaf_r, leaf_t) of ``N`` plates with the plate absorption ``k`` (not clamped here)."""
    Ra, Ta, r, t = top_plate(k, n, talf, t90, lib)
    D = lib.sqrt((1 + r + t) * (1 + r - t) * (1 - r + t) * (1 - r - t))
    a = (1 + r * r - t * t + D) / (2 * r)
    b = (1 - r * r + t * t + D) / (2 * t)
    bN = lib.exp((N - 1) * lib.log(b))
    dn = a * a * bN * bN - 1
    Rs = a * (bN * bN - 1) / dn
    Ts = bN * (a * a - 1) / dn
    return Ra + Ta * Rs * t / (1 - Rs * r), Ta * Ts / (1 - Rs * r)


def plate_k(q, K):
    """``k [ncol][nb]`` of float64 ``q [ncol][nm]``, ``K [nabs][nb]``: the sum in ascending i, then / N, then the clamp."""
    q, K = np.asarray(q, dtype=np.float64), np.asarray(K, dtype=np.float64)
    s = np.zeros((q.shape[0], K.shape[1]))
    for i in range(K.shape[0]):
        s = s + q[:, 1 + i, None] * K[i][None]
    return np.clip(s / q[:, :1], K_MIN, K_MAX)


def chain(q, K, k, dk, dN):
    """The base partials ``dk, dN [ncol][nb]`` -> the partials with respect to ``q``, ``[ncol][nm][nb]``: ``d/dC_i = (K_i / N) d/dk``,
    ``d/dN = dN - (k / N) dk`` (``k`` the clamped value)."""
    q, K = np.asarray(q, dtype=np.float64), np.asarray(K, dtype=np.float64)
    N = q[:, :1]
    return np.stack([dN - (k / N) * dk] + [(K[i][None] / N) * dk for i in range(K.shape[0])], axis=1)


def complex_step(q, K, n, alpha=ALPHA, h=1e-30):
    """complex128: ``(leaf_r, leaf_t, d_leaf_r, d_leaf_t)`` with the base partials by the complex step."""
    q, n = np.asarray(q, dtype=np.float64), np.asarray(n, dtype=np.float64)
    k, N = plate_k(q, K), q[:, :1] * np.ones((1, n.size))
    talf, t90 = tav(alpha, n), tav(90, n)
    rk, tk = plate(N, k + 1j * h, n[None], talf[None], t90[None])
    rN, tN = plate(N + 1j * h, k + 0j, n[None], talf[None], t90[None])
    return (rk.real, tk.real, chain(q, K, k, rk.imag / h, rN.imag / h), chain(q, K, k, tk.imag / h, tN.imag / h))


def _key(*arrays):
    return tuple((a.shape, a.tobytes()) for a in arrays)


_CACHE = {}


def reference(q, K, n, alpha=ALPHA):
    """``dict(leaf_r, leaf_t [ncol][nb], d_leaf_r, d_leaf_t [ncol][nm][nb], spread_r, spread_t [ncol][nm][nb])``: values and partials
    from mpmath at 50 digits (``mpmath.diff`` of the base partials, the chain rule in float64), rounded to float64, and the spread: the
    absolute difference of the complex-step partials from them.  Computed once per set of inputs."""
    import mpmath

    q, K, n = (np.ascontiguousarray(v, dtype=np.float64) for v in (q, K, n))
    key = _key(q, K, n) + (alpha,)
    if key in _CACHE:
        return _CACHE[key]
    k = plate_k(q, K)
    ncol, nb = k.shape
    val = np.zeros((2, ncol, nb))
    base = np.zeros((2, 2, ncol, nb))  # [r | t][dk | dN]
    with mpmath.workdps(50):
        sin = mpmath.sin(mpmath.radians(alpha))
        for b in range(nb):
            nn = mpmath.mpf(float(n[b]))
            talf, t90 = tav(alpha, nn, MP, sin), tav(90, nn, MP, mpmath.mpf(1))
            for c in range(ncol):
                N, kk = mpmath.mpf(float(q[c, 0])), mpmath.mpf(float(k[c, b]))
                v = plate(N, kk, nn, talf, t90, MP)
                for o in range(2):
                    val[o, c, b] = float(v[o])
                    base[o, 0, c, b] = float(mpmath.diff(lambda x: plate(N, x, nn, talf, t90, MP)[o], kk))
                    base[o, 1, c, b] = float(mpmath.diff(lambda x: plate(x, kk, nn, talf, t90, MP)[o], N))
    d_r, d_t = chain(q, K, k, base[0, 0], base[0, 1]), chain(q, K, k, base[1, 0], base[1, 1])
    cs = complex_step(q, K, n, alpha)
    res = dict(leaf_r=val[0], leaf_t=val[1], d_leaf_r=d_r, d_leaf_t=d_t, cs_leaf_r=cs[0], cs_leaf_t=cs[1], cs_d_leaf_r=cs[2],
               cs_d_leaf_t=cs[3], spread_r=np.abs(cs[2] - d_r), spread_t=np.abs(cs[3] - d_t), k=k)
    for v in res.values():
        v.setflags(write=False)
    _CACHE[key] = res
    return res


def domain_grid(seed=3):
    """The grid of the issue: nb = 24, nabs = 2, K_0 = logspace(-4, log10(50)), K_1 = 0.1 K_0 reversed, n = linspace(1.3, 1.6); four
    columns with C = (N, 0) -- k = K_0, band 0 at 1e-4 -- at N = 1, 1.37, 2.5, 3.5 and one column with random C."""
    nb = 24
    K0 = np.logspace(-4, np.log10(50.0), nb)
    K = np.stack([K0, 0.1 * K0[::-1]])
    n = np.linspace(1.3, 1.6, nb)
    rng = np.random.default_rng(seed)
    N = rng.uniform(1.2, 3.0)  # (the random column: k = u_0 K_0 + u_1 K_1 with u in [0.3, 0.9], inside [1e-4, 50])
    q = np.array([[N_, N_, 0.0] for N_ in (1.0, 1.37, 2.5, 3.5)] + [[N, N * rng.uniform(0.3, 0.9), N * rng.uniform(0.3, 0.9)]])
    return q, K, n
