"""Band definitions and band-integration weights (host side; these are O(n_wl) and feed the device epilogue).

Mirrors ``crt1d/spectra.py:22-27`` (``BAND_DEFNS_UM``) and ``:71-126`` (``_x_frac_in_bounds``)."""

import warnings

import numpy as np

BAND_DEFNS_UM = {"PAR": (0.4, 0.7), "NIR": (0.7, 2.5), "UV": (0.01, 0.4), "solar": (0.3, 5.0)}


def x_frac_in_bounds(xe, bounds):
    """Fraction of each bin ``[xe[i], xe[i+1]]`` inside ``bounds`` (weights for summing in-band irradiances)."""
    xe = np.asarray(xe, dtype=float)
    x1, x2 = xe[:-1], xe[1:]
    b1, b2 = bounds[0], bounds[1]
    if (b1 < x1[0] or b2 > x2[-1]) and tuple(bounds) != BAND_DEFNS_UM["solar"]:
        warnings.warn(
            f"`bounds` ({b1:.3g}, {b2:.3g}) extend outside the data range defined by `xe` ({x1[0]:.3g}, {x2[-1]:.3g})"
        )
    inside = (x2 >= b1) & (x1 <= b2)
    dx = x2 - x1
    w = np.ones_like(x1)
    left = x1 < b1
    right = ~left & (x2 > b2)
    w[left] = (x2[left] - b1) / dx[left]
    w[right] = (b2 - x1[right]) / dx[right]
    w[~inside] = 0.0
    return w


# CODATA 2018 exact SI values (what scipy.constants holds; crt1d/spectra.py:10-13 imports them from there)
_H_PLANCK = 6.62607015e-34  # J s
_C_LIGHT = 299792458.0  # m s-1
_N_AVOGADRO = 6.02214076e23  # mol-1


def e_wl_umol(wl_um):
    """J per micromole of photons at wavelength ``wl_um`` (micrometres); ``crt1d/spectra.py:30-39`` (same operation order)."""
    wl = np.asarray(wl_um, dtype=float) * 1e-6
    e_wl_1 = _H_PLANCK * _C_LIGHT / wl
    e_wl_mol = e_wl_1 * _N_AVOGADRO
    return e_wl_mol * 1e-6


def band_weights(wle, names=("PAR", "NIR", "solar"), *, wl=None, pfd=False):
    """Stack of weight vectors ``(len(names), n_wl)`` for the device band-sum epilogue: ``_x_frac_in_bounds`` of each named band
    (``diagnostics.py:71``).  ``pfd=True``: the photon-flux-density variants of ``diagnostics.band(..., calc_PFD=True)``
    (``:92-104``; ``_E_to_PFD_da`` ``:19-36`` multiplies every band by ``1 / e_wl_umol(wl)`` BEFORE the band sum, because photon energy
    depends on wavelength) -- the same sums with the weights divided by ``e_wl_umol(wl)``; ``wl`` = band centres (micrometres), by
    default the mid-points of ``wle``.  W m-2 in, micromol photons m-2 s-1 out."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = np.stack([x_frac_in_bounds(wle, BAND_DEFNS_UM[n]) for n in names])
    if pfd:
        wle = np.asarray(wle, dtype=float)
        wl = 0.5 * (wle[:-1] + wle[1:]) if wl is None else np.asarray(wl, dtype=float)
        w = w * (1.0 / e_wl_umol(wl))[None, :]
    return w


def edges_from_centers_widths(wl, dwl):
    """``wle`` as ``Model._check_inputs`` builds it (``crt1d/model.py:286-287``)."""
    wl, dwl = np.asarray(wl, dtype=float), np.asarray(dwl, dtype=float)
    return np.r_[wl[0] - 0.5 * dwl[0], wl + 0.5 * dwl]


def smear_tuv_batched(x, y, bins, *, out=None):
    """Re-bin ``nspec`` spectra at once on the GPU (``crt_hip_smear_tuv_f64``).

    ``x``: increasing grid ``(nx,)`` shared by all spectra, or ``(nspec, nx)``; ``y``: ``(nspec, nx)``; ``bins``: ``(nbins+1,)``
    edges.  CUDA float64 tensors (host arrays are copied over).  Returns a ``(nspec, nbins)`` CUDA tensor of in-bin
    averages, each the reference's ``_smear_tuv_1`` (``crt1d/spectra.py:221-257``) with identical arithmetic."""
    import ctypes  # noqa: F401
    import torch

    from . import _lib

    lib = _lib.load()
    dev = y.device if isinstance(y, torch.Tensor) and y.is_cuda else torch.device("cuda", torch.cuda.current_device())

    def dv(t):
        return torch.as_tensor(t, dtype=torch.float64).to(dev).contiguous()

    x, y, bins = dv(x), dv(y), dv(bins)
    if y.ndim != 2 or bins.ndim != 1 or bins.numel() < 1:
        raise ValueError("y must be (nspec, nx) and bins (nbins+1,)")
    nspec, nx = y.shape
    if x.shape == (nx,):
        x_stride = 0
    elif x.shape == (nspec, nx):
        x_stride = nx
    else:
        raise ValueError(f"x must be ({nx},) or ({nspec}, {nx}); got {tuple(x.shape)}")
    nbins = bins.numel() - 1
    if out is None:
        out = torch.empty((nspec, nbins), dtype=torch.float64, device=dev)
    elif out.shape != (nspec, nbins) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float64 (nspec, nbins) tensor")
    if nspec == 0 or nbins == 0:
        return out
    with torch.cuda.device(dev):
        st = lib.crt_hip_smear_tuv_f64(x.data_ptr(), x_stride, nx, y.data_ptr(), nspec, bins.data_ptr(), nbins, out.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "crt_hip_smear_tuv_f64")
    return out


def smear_tuv(x, y, bins):
    """Drop-in for ``crt1d.spectra.smear_tuv`` (``crt1d/spectra.py:260-300``): one spectrum, host arrays in and out."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return smear_tuv_batched(x, y[None, :], np.asarray(bins, dtype=np.float64)).cpu().numpy()[0]


def sensor_weights(wle, srf_x, srf_y):
    """Sensor-band weights on the model bands from tabulated spectral responses: ``srf_y`` ``(nsens, nx)`` responses on the grid ``srf_x``
    (``(nx,)`` shared, or ``(nsens, nx)``), ``wle`` the ``(nb + 1,)`` model band edges.  Returns the ``(nsens, nb)`` CUDA tensor of the mean
    of each response over each model band -- :func:`smear_tuv_batched` applied to the responses -- which
    :class:`crt1d_amd.batched.SensorSet` takes as it is (bands a response does not reach get weight 0 and stay outside its support)."""
    y = np.asarray(srf_y, dtype=np.float64) if not hasattr(srf_y, "is_cuda") else srf_y
    if y.ndim != 2:
        raise ValueError("srf_y must be (nsens, nx)")
    if np.ndim(wle) != 1 or np.shape(wle)[0] < 2:
        raise ValueError("wle must hold the nb + 1 band edges")
    return smear_tuv_batched(srf_x, y, wle)


def boxcar_sensor_weights(wle, bounds):
    """Boxcar sensor bands: ``bounds`` ``(nsens, 2)`` wavelength intervals -> ``(nsens, nb)`` NumPy weights, the fraction of each model
    band ``[wle[i], wle[i+1]]`` inside each interval (:func:`x_frac_in_bounds`)."""
    bounds = np.asarray(bounds, dtype=float)
    if bounds.ndim == 1:
        bounds = bounds[None, :]
    if bounds.ndim != 2 or bounds.shape[1] != 2:
        raise ValueError("bounds must be (nsens, 2)")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.stack([x_frac_in_bounds(wle, (b1, b2)) for b1, b2 in bounds])


# ---- light-weighted band optics and band irradiance on the device (include/crt1d_hip_spectra.h) --------------------------------------
def sub_bin_counts(x, edges, x_smear_nb=None):
    """Sub-bins per band as ``avg_optical_prop`` chooses them (``crt1d/spectra.py:185-189``): ``x_smear_nb``, or
    ``ceil((b1 - b0) / max(min dx, 5e-3))`` -- that very expression, in Python floats on the host (``(0.7 - 0.4) / 0.005`` sits next to
    an integer).  ``(nb,)`` int64."""
    import math

    x, edges = np.asarray(x, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    if x.ndim != 1 or x.size < 2 or edges.ndim != 1 or edges.size < 1:
        raise ValueError("x must be (nx >= 2,) and edges (nb+1,)")
    if x_smear_nb is not None:
        if int(x_smear_nb) != x_smear_nb or x_smear_nb < 1:
            raise ValueError("x_smear_nb must be a positive integer")
        return np.full(edges.size - 1, int(x_smear_nb), dtype=np.int64)
    dx_smear = max(np.diff(x).min(), 5e-3)
    return np.array([math.ceil((b1 - b0) / dx_smear) for b0, b1 in zip(edges[:-1], edges[1:])], dtype=np.int64)


def _sub_offsets(x, edges, x_smear_nb):
    """The int32 prefix sums of :func:`sub_bin_counts` the C entries take as a host pointer (kept alive by the caller)."""
    import ctypes

    n = sub_bin_counts(x, edges, x_smear_nb)
    if np.any(n < 1):
        raise ValueError("every band needs at least one sub-bin: edges must increase")
    off = np.concatenate([[0], np.cumsum(n)])
    if off[-1] > np.iinfo(np.int32).max:
        raise RuntimeError("too many sub-bins")
    off = np.ascontiguousarray(off, dtype=np.int32)
    return off, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _host(t):
    """A host float64 copy of a grid (tensor or array-like): the sub-bin counts are formed on the host."""
    import torch

    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _light_kind(light):
    from . import _lib

    if not isinstance(light, str) or light not in _lib.LIGHT_KINDS:
        raise ValueError("invalid choice of `light`: 'planck', 'uniform' or 'table'")
    return _lib.LIGHT_KINDS[light]


def avg_optical_prop_batched(x, y, edges, *, light="planck", T_K=6000, light_x=None, light_y=None, light_group=1, x_smear_nb=None,
                             out=None, y_sub=None):
    """Light-weighted band averages of ``nspec`` spectra in one launch (``crt_hip_avg_optical_prop_f64``): the reference's
    ``smear_avg_optical_prop(x, y[s], edges, light=..., x_smear_nb=...)`` (``crt1d/spectra.py:129-218, 366-390``) for every ``s``.

    ``x`` ``(nx,)`` increasing, shared; ``y`` ``(nspec, nx)``; ``edges`` ``(nb+1,)``; CUDA float64 tensors, or host arrays (copied over).
    ``light``: ``"planck"`` (``T_K``), ``"uniform"``, or ``"table"`` -- ``np.interp(mid-points, light_x, light_y)`` with ``light_x``
    ``(nlx,)`` and ``light_y`` ``(nlx,)`` or ``(nlight, nlx)``; spectrum ``s`` then uses row ``s // light_group`` (row 0 when there is one).
    Returns the ``(nspec, nb)`` CUDA tensor (``out`` if given).  ``y_sub``: an optional ``(nspec, n_sub_bins_total)`` tensor that receives
    the sub-bin averages themselves.  The sub-bin counts come from the host copies of ``x`` and ``edges`` (:func:`sub_bin_counts`)."""
    import torch

    from . import _lib

    lib = _lib.load()
    dev = y.device if isinstance(y, torch.Tensor) and y.is_cuda else torch.device("cuda", torch.cuda.current_device())

    def dv(t):
        return torch.as_tensor(t, dtype=torch.float64).to(dev).contiguous()

    kind = _light_kind(light)
    off, off_p = _sub_offsets(_host(x), _host(edges), x_smear_nb)
    x, y, edges = dv(x), dv(y), dv(edges)
    if y.ndim != 2 or x.ndim != 1 or y.shape[1] != x.shape[0] or edges.ndim != 1:
        raise ValueError("x must be (nx,), y (nspec, nx) and edges (nb+1,)")
    nspec, nx = y.shape
    nb = edges.numel() - 1
    lx = ly = None
    nlx = nlight = 0
    if kind == _lib.LIGHT_TABLE:
        if light_x is None or light_y is None:
            raise ValueError("light='table' needs light_x and light_y")
        lx, ly = dv(light_x), dv(light_y)
        if ly.ndim == 1:
            ly = ly[None, :]
        if lx.ndim != 1 or ly.ndim != 2 or ly.shape[1] != lx.shape[0]:
            raise ValueError("light_x must be (nlx,) and light_y (nlx,) or (nlight, nlx)")
        nlight, nlx = ly.shape
    if out is None:
        out = torch.empty((nspec, nb), dtype=torch.float64, device=dev)
    elif out.shape != (nspec, nb) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float64 (nspec, nb) tensor on the device of y")
    if y_sub is not None and (y_sub.shape != (nspec, int(off[-1])) or y_sub.dtype != torch.float64 or not y_sub.is_contiguous()
                              or y_sub.device != dev):
        raise ValueError(f"y_sub must be a contiguous float64 ({nspec}, {int(off[-1])}) tensor on the device of y")
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        st = lib.crt_hip_avg_optical_prop_f64(x.data_ptr(), nx, y.data_ptr(), nspec, edges.data_ptr(), nb, off_p, kind, float(T_K), p(lx), nlx,
                                              p(ly), nlight, int(light_group), out.data_ptr(), p(y_sub),
                                              torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "crt_hip_avg_optical_prop_f64")
    return out


def _light_args(light, light_kwargs):
    """``light`` of the single-spectrum drop-ins -> keyword arguments of :func:`avg_optical_prop_batched`."""
    if isinstance(light, str):
        if light not in ("planck", "uniform"):
            raise ValueError("invalid choice of `light`")
        extra = set(light_kwargs) - ({"T_K"} if light == "planck" else set())
        if extra:
            raise TypeError(f"unexpected light arguments {sorted(extra)}")
        return dict(light=light, **light_kwargs)
    if isinstance(light, tuple) and len(light) == 2 and not light_kwargs:
        return dict(light="table", light_x=np.asarray(light[0], dtype=np.float64), light_y=np.asarray(light[1], dtype=np.float64))
    raise NotImplementedError(
        "crt1d_amd evaluates the light on the device: `light` must be 'planck', 'uniform' or a (light_x, light_y) pair that is "
        "interpolated linearly at the sub-bin mid-points; an arbitrary callable or an array of per-bin weights cannot be sent there")


def smear_avg_optical_prop(x, y, bins, *, x_smear_nb=None, light="planck", **light_kwargs):
    """Drop-in for ``crt1d.spectra.smear_avg_optical_prop`` (``crt1d/spectra.py:366-390``): one spectrum, host arrays in and out.
    ``light``: ``"planck"`` (``T_K=``), ``"uniform"``, or a ``(light_x, light_y)`` pair standing for the callable
    ``lambda x: np.interp(x, light_x, light_y)``; any other callable raises NotImplementedError (there is no host path)."""
    kw = _light_args(light, light_kwargs)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return avg_optical_prop_batched(x, y[None, :], np.asarray(bins, dtype=np.float64), x_smear_nb=x_smear_nb, **kw).cpu().numpy()[0]


def avg_optical_prop(y, bounds, *, x=None, xe=None, x_smear_nb=None, light="planck", **light_kwargs):
    """Drop-in for ``crt1d.spectra.avg_optical_prop`` (``crt1d/spectra.py:129-218``) in its ``x=`` form: the average of the spectrum
    ``y(x)`` over ``bounds``, a float.  The ``xe=`` form (an already binned spectrum) is not implemented on the device."""
    if xe is not None:
        if x is not None:
            raise ValueError("only provide one of `x` and `xe`.")
        raise NotImplementedError("crt1d_amd implements avg_optical_prop for a spectrum y(x) only: the `xe=` form (already binned) is not available")
    if x is None:
        raise ValueError("`x` or `xe` must be provided!")
    return float(smear_avg_optical_prop(x, y, np.asarray([bounds[0], bounds[1]], dtype=np.float64), x_smear_nb=x_smear_nb, light=light,
                                        **light_kwargs)[0])


def smear_si_batched(x_si, SI_dr, SI_df, edges):
    """Band irradiances of ``smear_si`` (``crt1d/spectra.py:529-573``) for ``ncol`` spectra: ``(I_dr0, I_df0, dwl)`` with
    ``I = smear_tuv(x_si, SI, edges) * dwl``, ``(ncol, nb)`` CUDA tensors and ``dwl = diff(edges)`` ``(nb,)``."""
    import torch

    dev = SI_dr.device if isinstance(SI_dr, torch.Tensor) and SI_dr.is_cuda else torch.device("cuda", torch.cuda.current_device())
    edges = torch.as_tensor(edges, dtype=torch.float64).to(dev).contiguous()
    dwl = edges[1:] - edges[:-1]
    two_d = lambda t: (lambda v: v[None, :] if v.ndim == 1 else v)(torch.as_tensor(t, dtype=torch.float64).to(dev))  # noqa: E731
    return smear_tuv_batched(x_si, two_d(SI_dr), edges) * dwl, smear_tuv_batched(x_si, two_d(SI_df), edges) * dwl, dwl
