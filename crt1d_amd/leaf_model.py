"""
The generalised plate model of leaf optics (Allen et al. 1969; Stokes' pile of plates; the core of PROSPECT) as the leaf model of the
retrievals: ``include_ext/crt1d_hip_leafmodel.h`` states the model, :func:`crt1d_amd.batched.plate_leaf_optics` evaluates it on the
device, and ``leaf_model=`` of the retrieval plans retrieves its parameters.

What depends on the band alone -- the interface transmittances :func:`tav` -- is computed here, on the host, in NumPy.  The specific
absorption spectra are the user's: no coefficient tables are shipped.
"""

import numpy as np

from . import _lib

N_MIN, N_MAX = 1.0, 4.0  # the domain of the structure parameter (the header: bN^2 stays below 1e265)


def tav(alpha_deg, n):
    """The Fresnel transmittance of a dielectric interface of refractive index ``n`` averaged over the cone of half-angle
    ``alpha_deg`` degrees (Stern 1964; Allen 1973), unpolarised light.  ``n``: a number or an array, > 1; ``0 < alpha_deg <= 90``."""
    n = np.asarray(n, dtype=np.float64)
    if not 0.0 < float(alpha_deg) <= 90.0:
        raise ValueError(f"alpha must lie in (0, 90] degrees, got {alpha_deg}")
    if np.any(n <= 1.0):
        raise ValueError("the refractive index must be > 1")
    n2 = n * n
    npl, nmi = n2 + 1.0, n2 - 1.0
    A = (n + 1.0) ** 2 / 2.0
    k = -(nmi**2) / 4.0
    s = np.sin(np.deg2rad(float(alpha_deg))) ** 2
    b2 = s - npl / 2.0
    b1 = np.zeros_like(n) if float(alpha_deg) == 90.0 else np.sqrt(b2 * b2 + k)
    B = b1 - b2
    ts = (k * k / (6.0 * B**3) + k / B - B / 2.0) - (k * k / (6.0 * A**3) + k / A - A / 2.0)
    tp1 = -2.0 * n2 * (B - A) / npl**2
    tp2 = -2.0 * n2 * npl * np.log(B / A) / nmi**2
    tp3 = n2 * (1.0 / B - 1.0 / A) / 2.0
    tp4 = 16.0 * n2**2 * (n2**2 + 1.0) * np.log((2.0 * npl * B - nmi**2) / (2.0 * npl * A - nmi**2)) / (npl**3 * nmi**2)
    tp5 = 16.0 * n2**3 * (1.0 / (2.0 * npl * B - nmi**2) - 1.0 / (2.0 * npl * A - nmi**2)) / npl**3
    return (ts + tp1 + tp2 + tp3 + tp4 + tp5) / (2.0 * s)


class PlateLeafModel:
    """The per-band part of the plate model: ``kspec (nabs, nb)`` specific absorption spectra (``nabs`` 1 .. 7, ``>= 0``), ``n (nb,)``
    the refractive index, ``alpha`` the half-angle of the cone of the top interface in degrees, ``names`` the absorbers' names (default
    ``"C0", "C1", ..``).  ``params`` names the model's parameters of every column, ``("N", names...)``; ``nm = 1 + nabs`` of them.  The
    host arrays ``kspec, n, t_alpha, t_90`` are kept; the device tensors are made at the first use on a device and kept too."""

    def __init__(self, kspec, n, *, alpha=40.0, names=None):
        kspec = np.ascontiguousarray(kspec, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.float64)
        if kspec.ndim != 2 or n.ndim != 1 or kspec.shape[1] != n.shape[0] or n.shape[0] < 1:
            raise ValueError("kspec must be (nabs, nb) and n (nb,)")
        if not 1 <= kspec.shape[0] <= _lib.PLATE_MAX_NABS:
            raise ValueError(f"nabs = {kspec.shape[0]}; the model takes 1 .. {_lib.PLATE_MAX_NABS} absorbers")
        if not np.all(np.isfinite(kspec)) or np.any(kspec < 0.0):
            raise ValueError("kspec must be finite and >= 0")
        if names is None:
            names = tuple(f"C{i}" for i in range(kspec.shape[0]))
        names = tuple(str(v) for v in names)
        if len(names) != kspec.shape[0] or len(set(names) | {"N"}) != len(names) + 1:
            raise ValueError("names must be nabs distinct names other than 'N'")
        self.kspec, self.n, self.alpha = kspec, n, float(alpha)
        self.t_alpha, self.t_90 = tav(alpha, n), tav(90.0, n)
        self.params = ("N",) + names
        self._dev = {}

    @property
    def nabs(self):
        return self.kspec.shape[0]

    @property
    def nm(self):
        return 1 + self.kspec.shape[0]

    @property
    def nb(self):
        return self.kspec.shape[1]

    def tensors(self, device):
        """``(kspec, t_alpha, t_90, n)`` as float64 tensors on ``device`` (made once per device)."""
        import torch

        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = tuple(torch.as_tensor(v).to(device).contiguous() for v in (self.kspec, self.t_alpha, self.t_90, self.n))
        return self._dev[device]

    def c_struct(self, ncol, device):
        k, ta, t9, n = self.tensors(device)
        return _lib.CrtPlateLeafModel(ncol, self.nb, self.nabs, k.data_ptr(), ta.data_ptr(), t9.data_ptr(), n.data_ptr())

    def check_bounds(self, lo, hi):
        """The bounds of a retrieval on the model's slots: ``N`` inside [1, 4], every content ``>= 0``; else a ValueError."""
        if lo is None or hi is None:
            raise ValueError("a leaf_model needs lo and hi: they keep N inside [1, 4] and the contents >= 0")
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        nm = self.nm
        if lo.ndim != 1 or hi.ndim != 1 or lo.shape[0] < nm or hi.shape[0] < nm:
            raise ValueError(f"lo and hi must cover the {nm} parameters of the leaf model")
        if not (lo[0] >= N_MIN and hi[0] <= N_MAX and lo[0] <= hi[0]):
            raise ValueError(f"lo and hi must keep N inside [{N_MIN:g}, {N_MAX:g}], got [{lo[0]:g}, {hi[0]:g}]")
        if not (np.all(lo[1:nm] >= 0.0) and np.all(hi[1:nm] >= lo[1:nm])):
            raise ValueError(f"lo and hi must keep every content >= 0, got lo = {lo[1:nm]}, hi = {hi[1:nm]}")
