"""
Batched (column x band) canopy-RT solves on PyTorch-ROCm tensors.

PyTorch is plumbing here: device memory, streams and (in :mod:`crt1d_amd.dist`)
``torch.distributed``.  All arithmetic happens in the hand-written gfx950 kernels of
``libcrt1d_hip.so``, reached through the C ABI with ``tensor.data_ptr()``.

Shapes: ``ncol`` columns, ``nb`` bands, ``nz`` interface levels.  Outputs are
``(ncol, nz, nb)`` (``(ncol, nz-1, nb)`` for n79's per-leaf-area absorption), bands contiguous --
the reference's ``(nz, nb)`` solver outputs (e.g. ``_solve_2s.py:45-49``) stacked over columns.
"""

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

SCHEMES = tuple(_lib.SCHEME_IDS)

# output keys per scheme, in crt_outputs slot order (I_dr, I_df_d, I_df_u, F, x0, x1, x2)
OUT_KEYS = {
    "2s": ("I_dr", "I_df_d", "I_df_u", "F"),  # _solve_2s.py:158-163
    "4s": ("I_dr", "I_df_d", "I_df_u", "F"),  # _solve_4s.py:293
    "bl": ("I_dr", "I_df_d", "I_df_u", "F"),  # _solve_bl.py:93
    "n79": ("I_dr", "I_df_d", "I_df_u", "F", "aI_lsl", "aI_lsh"),  # _solve_n79.py:157-164
    "zq": ("I_dr", "I_df_d", "I_df_u", "F", "I_df_d_ss", "I_df_u_ss", "F_ss"),  # _solve_zq.py:221-229
    "g77": ("I_dr", "I_df_d", "I_df_u", "F", "aI_lsl", "aI_lsh", "aI_l"),  # _solve_g77.py:127-135
    "bf": ("I_dr", "I_df_d", "I_df_u", "F", "aI_lsl", "aI_lsh", "aI_l"),  # _solve_bf.py:144-153 (+ rho_c host-side)
    "zq_pa": ("I_dr", "I_df_d", "I_df_u", "F"),  # _solve_zq_pa.py:413-418
}
_MID_KEYS = {"n79": ("aI_lsl", "aI_lsh")}  # (ncol, nz-1, nb)


def _tensor(t, name, dtypes):
    """A tensor the kernels read through a bare pointer: a contiguous CUDA tensor whose dtype is one of ``dtypes``."""
    _check_type(t, name, dtypes)
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); crt1d_amd has no CPU path")
    return t.contiguous()


def _check_type(t, name, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d)[len('torch.'):] for d in dtypes)}, got {t.dtype}")


def _f64(t, name):
    return _tensor(t, name, (torch.float64,))


def _f32(t, name):
    return _tensor(t, name, (torch.float32,))


def _fio(t, name):
    """Spectra may be float64 (crt_hip_*_f64) or float32 (crt_hip_*_f32: half the HBM bytes, fp64 arithmetic)."""
    return _tensor(t, name, (torch.float64, torch.float32))


def _host_reader(d, device):
    """``k -> d[k]`` as a tensor on ``device``, ``None`` for an entry that is missing or ``None``: what the ``from_host`` constructors read
    a dict of NumPy arrays with."""
    return lambda k: None if d.get(k) is None else torch.as_tensor(d[k]).to(device)


def _check_profile(t, name, shape, device, dtype=torch.float64):
    """A caller-supplied profile / output array: the C ABI receives a bare pointer, so everything the kernels assume about it
    (dtype, shape, device, contiguity) is checked here."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda or t.device != device:
        raise ValueError(f"{name} must live on {device} (got {t.device})")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


@dataclass
class Columns:
    """Device-resident per-column canopy geometry (what one reference ``Model`` holds)."""

    psi: torch.Tensor  # (ncol,)
    lai: torch.Tensor  # (ncol, nz), index 0 = ground
    g_kind: torch.Tensor  # (ncol,) int32, crt1d_amd.leaf_angle kind ids
    g_param: torch.Tensor  # (ncol,)
    mla: Optional[torch.Tensor] = None  # (ncol,) degrees; 2s only
    g_at_psi: Optional[torch.Tensor] = None  # (ncol,)  G_TABLE columns
    g_table: Optional[torch.Tensor] = None  # (ncol, NQ) G_TABLE columns

    def __post_init__(self):
        self.psi = _f64(self.psi, "psi")
        self.lai = _f64(self.lai, "lai")
        if self.lai.ndim != 2 or self.psi.shape != (self.lai.shape[0],):
            raise ValueError("lai must be (ncol, nz) and psi (ncol,)")
        self.g_param = _f64(self.g_param, "g_param")
        if self.g_kind.dtype != torch.int32 or not self.g_kind.is_cuda:
            raise TypeError("g_kind must be a CUDA int32 tensor")
        self.g_kind = self.g_kind.contiguous()
        for name in ("mla", "g_at_psi"):
            v = getattr(self, name)
            if v is not None:
                v = _f64(v, name)
                if v.shape != self.psi.shape:
                    raise ValueError(f"{name} must be (ncol,)")
                setattr(self, name, v)
        if self.g_table is not None:
            self.g_table = _f64(self.g_table, "g_table")
            if self.g_table.shape != (self.ncol, _lib.NQ):
                raise ValueError(f"g_table must be (ncol, {_lib.NQ})")

    @property
    def ncol(self):
        return self.lai.shape[0]

    @property
    def nz(self):
        return self.lai.shape[1]

    @property
    def device(self):
        return self.lai.device

    def validate(self):
        """The orientation checks ``Model._check_inputs`` makes per column (``crt1d/model.py:244-246``), for the whole
        batch (one device->host sync): lai strictly decreasing with level, lai[:, -1] == 0, 0 <= psi < pi/2."""
        import math

        lai = self.lai
        ok = bool((lai[:, :-1] > lai[:, 1:]).all()) and bool((lai[:, -1] == 0).all())
        if not ok:
            raise AssertionError("lai must decrease strictly from index 0 (ground, total LAI) to 0 at the canopy top")
        if not bool(((self.psi >= 0) & (self.psi < math.pi / 2)).all()):
            raise AssertionError("psi must be in [0, pi/2)")
        if not bool(((self.g_kind >= 0) & (self.g_kind <= 6)).all()):
            raise ValueError("invalid leaf-angle kind")
        self.check_tables()
        return self

    def check_tables(self):
        """Columns of kind G_TABLE dereference ``g_table`` / ``g_at_psi`` on the device: when either is missing make sure no
        column asks for it (one device->host sync, and only in the case where a table is missing)."""
        if getattr(self, "_tables_ok", False):
            return
        if (self.g_table is None or self.g_at_psi is None) and bool((self.g_kind == 6).any()):
            raise ValueError("columns with g_kind = G_TABLE need g_table and g_at_psi")
        self._tables_ok = True  # checked once per object; slices inherit the result (no sync inside a tiled, overlapped loop)

    def slice(self, lo, hi):
        """Columns [lo, hi) as a view (used by the column-sharded multi-GPU path)."""
        g = lambda t: None if t is None else t[lo:hi]  # noqa: E731
        c = Columns(self.psi[lo:hi], self.lai[lo:hi], self.g_kind[lo:hi], self.g_param[lo:hi], g(self.mla),
                    g(self.g_at_psi), g(self.g_table))
        c._tables_ok = getattr(self, "_tables_ok", False)
        return c

    def c_struct(self):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _lib.CrtColumns(self.ncol, self.nz, p(self.psi), p(self.lai), p(self.mla), p(self.g_kind), p(self.g_param),
                               p(self.g_at_psi), p(self.g_table))

    @classmethod
    def from_host(cls, d, device="cuda"):
        """From a dict of NumPy arrays (e.g. :func:`crt1d_amd.synth.make_columns`)."""
        t = _host_reader(d, device)
        return cls(t("psi"), t("lai"), t("g_kind"), t("g_param"), t("mla"), t("g_at_psi"), t("g_table"))

    @classmethod
    def from_leaf_pdf(cls, psi, lai, pdf_kind, pdf_param, mu_s=0.501):
        """Columns described by their leaf-inclination PDFs (:func:`leaf_pdf_tables`): ``g_kind = G_TABLE`` with ``g_table``, ``g_at_psi``
        and ``mla`` (the PDF's mean leaf angle) formed on the device.  ``mu_s`` must be the one the solve is given."""
        psi = _f64(psi, "psi")
        if psi.ndim != 1:
            raise ValueError("psi must be (ncol,)")
        g_table, g_at_psi, mla = leaf_pdf_tables(pdf_kind, pdf_param, mu_s=mu_s, psi=psi)
        kind = torch.full((psi.shape[0],), 6, dtype=torch.int32, device=psi.device)
        return cls(psi, lai, kind, torch.zeros_like(psi), mla, g_at_psi, g_table)


def leaf_pdf_tables(pdf_kind, pdf_param, *, mu_s=0.501, psi=None):
    """G(psi) of ``ncol`` leaf-inclination PDFs in one launch (``crt_hip_g_from_pdf_f64``, include/crt1d_hip_leaf.h).

    ``pdf_kind`` ``(ncol,)``: ``leaf_angle.PDF_*`` ids; ``pdf_param`` ``(ncol, 2)``: ``x`` or ``(a, b)`` (see :class:`crt1d_amd.leaf_angle.LeafPDF`);
    tensors on the GPU, or anything ``torch.as_tensor`` takes (moved there).  ``psi``: ``None``, ``(ncol,)`` -- each column's sun angle -- or
    ``(ncol, nt)``, the sun angles of a series.  Returns CUDA tensors ``g_table (ncol, NQ)`` (G at ``_lib.quad_nodes(mu_s)``),
    ``g_at_psi`` (the shape of ``psi``; ``(ncol, 0)`` without it) and ``mla (ncol,)`` in degrees: ``Columns.g_table / g_at_psi / mla``, and
    for a series ``SunSeries.g_at_psi`` directly.  An unknown kind, ``x <= 0`` or a ``(a, b)`` whose PDF goes negative is a ValueError,
    found by the library before the launch (it reads the descriptors back once: one stream synchronisation)."""
    given = [t for t in (pdf_kind, pdf_param, psi) if isinstance(t, torch.Tensor) and t.is_cuda]
    dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
    # (dtype given to as_tensor: Python floats would otherwise pass through torch's default float32 and x = 0.3 arrive as 0.30000001)
    as_f64 = lambda v: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.float64)).to(device=dev, dtype=torch.float64)  # noqa: E731
    kind = torch.as_tensor(pdf_kind).to(device=dev, dtype=torch.int32).contiguous()
    param = as_f64(pdf_param).contiguous()
    if kind.ndim != 1 or param.shape != (kind.shape[0], 2):
        raise ValueError("pdf_kind must be (ncol,) and pdf_param (ncol, 2)")
    ncol = kind.shape[0]
    if psi is None:
        ps = torch.empty((ncol, 0), dtype=torch.float64, device=dev)
    else:
        ps = as_f64(psi).contiguous()
        if ps.ndim not in (1, 2) or ps.shape[0] != ncol:
            raise ValueError("psi must be (ncol,) or (ncol, nt)")
    npsi = ps.numel() // ncol if ncol else 0
    g_table = torch.empty((ncol, _lib.NQ), dtype=torch.float64, device=dev)
    g_at_psi = torch.empty_like(ps)
    mla = torch.empty((ncol,), dtype=torch.float64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        st = lib.crt_hip_g_from_pdf_f64(kind.data_ptr(), param.data_ptr(), ncol, float(mu_s), ps.data_ptr() if npsi else None, npsi,
                                        g_table.data_ptr(), g_at_psi.data_ptr() if npsi else None, mla.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "crt_hip_g_from_pdf_f64")
    return g_table, g_at_psi, mla


@dataclass
class Bands:
    """Per-(column, band) spectra; each tensor is (ncol, nb), or (nb,)/(1, nb) to share one
    spectrum over all columns (the reference's (n_wl,) plugin inputs)."""

    I_dr0: torch.Tensor
    I_df0: torch.Tensor
    leaf_r: torch.Tensor
    leaf_t: torch.Tensor
    soil_r: Optional[torch.Tensor] = None

    def __post_init__(self):
        shape = None
        self.dtype = None
        for name in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r"):
            v = getattr(self, name)
            if v is None:
                continue
            v = _fio(v, name)
            if self.dtype is None:
                self.dtype = v.dtype
            elif v.dtype != self.dtype:
                raise TypeError("all band arrays must share one dtype")
            if v.ndim == 1:
                v = v[None, :]
            if v.ndim != 2:
                raise ValueError(f"{name} must be (ncol, nb) or (nb,)")
            if shape is None:
                shape = v.shape
            elif v.shape != shape:
                raise ValueError("all band arrays must have the same shape")
            setattr(self, name, v)
        self._shape = shape

    @property
    def nb(self):
        return self._shape[1]

    def col_stride(self, ncol):
        if self._shape[0] == 1 and ncol != 1:
            return 0
        if self._shape[0] != ncol:
            raise ValueError(f"band arrays have {self._shape[0]} rows but there are {ncol} columns")
        return self.nb

    def slice(self, lo, hi):
        if self._shape[0] == 1:
            return self
        g = lambda t: None if t is None else t[lo:hi]  # noqa: E731
        return Bands(self.I_dr0[lo:hi], self.I_df0[lo:hi], self.leaf_r[lo:hi], self.leaf_t[lo:hi], g(self.soil_r))

    def band_slice(self, lo, hi):
        """Bands [lo, hi) of every column (band-sharded multi-GPU path); copies to keep rows contiguous."""
        g = lambda t: None if t is None else t[:, lo:hi].contiguous()  # noqa: E731
        return Bands(g(self.I_dr0), g(self.I_df0), g(self.leaf_r), g(self.leaf_t), g(self.soil_r))

    def c_struct(self, ncol):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _lib.CrtBands(self.nb, self.col_stride(ncol), p(self.I_dr0), p(self.I_df0), p(self.leaf_r), p(self.leaf_t),
                             p(self.soil_r))

    @classmethod
    def from_host(cls, d, device="cuda"):
        t = _host_reader(d, device)
        return cls(t("I_dr0"), t("I_df0"), t("leaf_r"), t("leaf_t"), t("soil_r"))

    @classmethod
    def from_spectra(cls, x_opt, leaf_r, leaf_t, soil_r, x_si, SI_dr, SI_df, edges, *, light="table", T_K=6000, x_smear_nb=None):
        """The five band arrays from raw spectra, in one launch for all columns (``crt_hip_bands_from_spectra_f64``,
        include/crt1d_hip_spectra.h): what the reference prepares with ``smear_avg_optical_prop`` and ``smear_si``
        (``crt1d/spectra.py:129-218, 366-390, 529-573``).

        ``leaf_r``, ``leaf_t``, ``soil_r``: raw optics on the grid ``x_opt (nx,)``; ``SI_dr``, ``SI_df``: spectral irradiance
        (W m-2 um-1) on ``x_si (nxs,)``; each a CUDA float64 tensor ``(ncol, n)``, or ``(n,)`` for one spectrum shared by all columns.
        ``edges (nb+1,)``: band edges.  The grids and ``edges`` may be host arrays (the sub-bin counts are formed on the host from them,
        :func:`crt1d_amd.spectra.sub_bin_counts`).  ``light``: what weights the optics -- ``"table"``: each column's own
        ``SI_dr + SI_df``; ``"planck"`` (``T_K``); ``"uniform"``.  Returns ``Bands`` with ``(ncol, nb)`` arrays (``ncol = 1`` when every
        input is shared)."""
        from . import spectra as sp

        kind = sp._light_kind(light)
        xo_h, xs_h, ed_h = sp._host(x_opt), sp._host(x_si), sp._host(edges)
        if xo_h.ndim != 1 or xs_h.ndim != 1 or ed_h.ndim != 1 or ed_h.size < 1:
            raise ValueError("x_opt must be (nx,), x_si (nxs,) and edges (nb+1,)")
        ncol, dev = None, None
        rows = {}
        given = (("leaf_r", leaf_r, xo_h.size), ("leaf_t", leaf_t, xo_h.size), ("soil_r", soil_r, xo_h.size), ("SI_dr", SI_dr, xs_h.size),
                 ("SI_df", SI_df, xs_h.size))
        for name, t, n in given:  # (type, dtype and shape of every input before the device of any)
            _check_type(t, name, (torch.float64,))
            if t.ndim not in (1, 2) or t.shape[-1] != n:
                raise ValueError(f"{name} must be (ncol, {n}) or ({n},), got {tuple(t.shape)}")
        for name, t, n in given:
            t = _f64(t, name)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise ValueError(f"{name} lives on {t.device} but leaf_r on {dev}")
            if t.ndim == 2:
                if ncol is None:
                    ncol = t.shape[0]
                elif t.shape[0] != ncol:
                    raise ValueError(f"{name} has {t.shape[0]} rows but another input {ncol}")
            rows[name] = t
        ncol = 1 if ncol is None else ncol
        off, off_p = sp._sub_offsets(xo_h, ed_h, x_smear_nb)
        grid = lambda t: torch.as_tensor(t, dtype=torch.float64).to(dev).contiguous()  # noqa: E731
        x_opt, x_si, edges = grid(x_opt), grid(x_si), grid(edges)
        nb = ed_h.size - 1
        out = [torch.empty((ncol, nb), dtype=torch.float64, device=dev) for _ in range(5)]
        args = []
        for name in ("leaf_r", "leaf_t", "soil_r"):
            args += [rows[name].data_ptr(), xo_h.size if rows[name].ndim == 2 else 0]
        args += [x_si.data_ptr(), xs_h.size]
        for name in ("SI_dr", "SI_df"):
            args += [rows[name].data_ptr(), xs_h.size if rows[name].ndim == 2 else 0]
        with torch.cuda.device(dev):
            st = _lib.load().crt_hip_bands_from_spectra_f64(x_opt.data_ptr(), xo_h.size, *args, ncol, edges.data_ptr(), nb, off_p, kind,
                                                            float(T_K), *(o.data_ptr() for o in out),
                                                            torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, "crt_hip_bands_from_spectra_f64")
        return cls(*out)


def _check_band_device(bands, device):
    for name in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r"):
        v = getattr(bands, name)
        if v is not None and v.device != device:
            raise ValueError(f"{name} lives on {v.device} but the columns on {device}")


def _check_workspace(workspace, need, device):
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != device:
        raise ValueError(f"workspace must be a tensor on {device}")
    if not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace too small or not contiguous (need {need} bytes)")
    return workspace


def _outputs(shapes, out, dtype, device, label="out[{!r}]", lacks=False):
    """The output arrays ``{key: shape}``: allocated when ``out`` is ``None``, else the caller's ``out`` with every array checked.
    ``lacks``: a missing key is a ValueError (not a KeyError)."""
    if out is None:
        return {k: torch.empty(sh, dtype=dtype, device=device) for k, sh in shapes.items()}
    for k, sh in shapes.items():
        if lacks and k not in out:
            raise ValueError(f"`out` lacks {k!r}")
        _check_profile(out[k], label.format(k), sh, device, dtype)
    return out


def _band_weights(band_w, nb, device):
    """Band weights ``(nb,)`` or ``(ngroup <= 4, nb)`` as the ``(ngroup, nb)`` float64 tensor on ``device`` the kernels read."""
    band_w = _f64(band_w, "band_w")
    if band_w.ndim == 1:
        band_w = band_w[None, :]
    if band_w.shape[1] != nb or not 1 <= band_w.shape[0] <= 4:
        raise ValueError("band_w must be (ngroup <= 4, nb)")
    if band_w.device != device:
        raise ValueError(f"band_w lives on {band_w.device} but the columns on {device}")
    return band_w


def workspace_bytes(scheme, ncol, nz, nb=1):
    """Device workspace a solve needs; ``nb`` matters for zq_pa only (its computational-grid fluxes live there)."""
    return int(_lib.load().crt_hip_workspace_bytes_nb(_lib.SCHEME_IDS[scheme], ncol, nz, nb))


class _DeviceBuffer:
    """Owner of one buffer of a ``crt_hip_buffer_alloc_set`` allocation; exposes it to torch through
    ``__cuda_array_interface__`` (the tensor made from it keeps this object, and with it the memory, alive)."""

    def __init__(self, ptr, shape, dtype, device):
        self._lib = _lib.load()
        self._ptr = ctypes.c_void_p(ptr)
        self._dev = torch.device(device)
        self.__cuda_array_interface__ = {
            "shape": tuple(int(s) for s in shape), "typestr": {torch.float64: "<f8", torch.float32: "<f4"}[dtype],
            "data": (ptr, False), "version": 2, "strides": None,
        }

    def classes(self):
        buf = ctypes.create_string_buffer(4096)
        _lib.check(self._lib.crt_hip_buffer_describe(self._ptr, buf, len(buf)), "crt_hip_buffer_describe")
        return buf.value.decode()

    def __del__(self):
        if getattr(self, "_ptr", None) is not None and self._ptr.value:
            try:
                torch.cuda.synchronize(self._dev)  # nothing may still be writing into it
                self._lib.crt_hip_buffer_free(self._ptr)
            except Exception:  # interpreter shutdown
                pass
            self._ptr = None


_OWNERS = "_crt_owner"  # attribute under which a tensor made by device_buffers() carries its _DeviceBuffer


def device_buffers(shapes, dtype=torch.float64, device="cuda"):
    """Tensors for ONE output set (arrays a kernel writes in step), placed by ``crt_hip_buffer_alloc_set``: 512 MB physical chunks
    whose memory classes are interleaved across the arrays (include/crt1d_hip.h; csrc/buffers.hip).  Raises if the HIP
    virtual-memory API is unavailable -- callers that can live with any placement catch the error and use ``torch.empty``."""
    lib = _lib.load()
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    itemsize = torch.empty((), dtype=dtype).element_size()
    n = len(shapes)
    sizes = []
    for shape in shapes:
        k = itemsize
        for s in shape:
            k *= int(s)
        sizes.append(max(k, itemsize))
    c_sizes = (ctypes.c_size_t * n)(*sizes)
    c_ptrs = (ctypes.c_void_p * n)()
    with torch.cuda.device(dev):
        _lib.check(lib.crt_hip_buffer_alloc_set(n, c_sizes, c_ptrs), "crt_hip_buffer_alloc_set")
    out = []
    for ptr, shape in zip(c_ptrs, shapes):
        owner = _DeviceBuffer(ptr, shape, dtype, dev)
        t = torch.as_tensor(owner, device=dev)
        setattr(t, _OWNERS, owner)
        out.append(t)
    return out


def device_buffer(shape, dtype=torch.float64, device="cuda"):
    """One tensor from ``crt_hip_buffer_alloc`` (a set of one)."""
    return device_buffers([shape], dtype, device)[0]


def buffer_classes(t):
    """Memory-class letters of the chunks behind a tensor made by :func:`device_buffers` (``None`` for any other tensor)."""
    owner = getattr(t, _OWNERS, None)
    return None if owner is None else owner.classes()


def buffer_stats(device=None):
    """``crt_hip_buffer_stats`` of the current (or given) device as a dict."""
    lib = _lib.load()
    a = (ctypes.c_int64 * 6)()
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        _lib.check(lib.crt_hip_buffer_stats(a), "crt_hip_buffer_stats")
    return dict(zip(("chunks_created", "chunks_released", "probes", "probe_us", "free_chunks", "classes_seen"), [int(v) for v in a]))


def trim_buffers(device=None):
    """Hand the set allocator's pooled chunks of the current (or given) device back to the driver (``crt_hip_buffer_trim``).  The pool
    keeps at most its retention cap anyway (8 GB by default, :func:`set_pool_retention`); call this before a large allocation through
    another allocator (``torch.empty``, RCCL buffers) when every GB counts."""
    lib = _lib.load()
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        _lib.check(lib.crt_hip_buffer_trim(), "crt_hip_buffer_trim")


def set_pool_retention(nbytes):
    """Cap on the memory the set allocator's per-device pools keep after buffers are freed (``crt_hip_buffer_set_retain``;
    default 8 GB, or ``CRT1D_POOL_RETAIN_MB``).  Applied at once to the existing pools."""
    _lib.check(_lib.load().crt_hip_buffer_set_retain(int(nbytes)), "crt_hip_buffer_set_retain")


PLACED_MIN_BYTES = 1 << 30  # below this the whole output set lives in the 256 MB Infinity Cache / a few chunks: plain torch memory


def alloc_outputs(scheme, ncol, nz, nb, device, dtype=torch.float64, placed=False):
    """Output arrays of one scheme.  ``placed=True``: through :func:`device_buffers` (class-interleaved 512 MB chunks) when the
    set is at least ``PLACED_MIN_BYTES``; otherwise (or if the virtual-memory API fails) plain ``torch.empty``."""
    shapes = {}
    for k in OUT_KEYS[scheme]:
        n = nz - 1 if k in _MID_KEYS.get(scheme, ()) else nz
        shapes[k] = (ncol, n, nb)
    item = 8 if dtype == torch.float64 else 4
    total = sum(s[0] * s[1] * s[2] * item for s in shapes.values())
    if placed and total >= PLACED_MIN_BYTES:
        try:
            return dict(zip(shapes, device_buffers(list(shapes.values()), dtype, device)))
        except RuntimeError:
            pass  # placement is a performance feature: any device memory is correct
    try:
        return {k: torch.empty(s, dtype=dtype, device=device) for k, s in shapes.items()}
    except torch.OutOfMemoryError:
        # what the set allocator's pool still holds is invisible to torch's caching allocator: release it and try once more
        trim_buffers(device)
        torch.cuda.empty_cache()
        return {k: torch.empty(s, dtype=dtype, device=device) for k, s in shapes.items()}


MASKED_SCHEMES = ("2s", "bl", "g77", "bf")  # the schemes of include_mask/crt1d_hip_masked.h


def _check_skip(skip, skip_unit, ncol, scheme, bands):
    """The checks of ``skip=`` / ``skip_unit=`` that touch no device (``ncol``: the number of columns, or ``None`` where it is not known
    yet)."""
    if isinstance(skip_unit, bool) or not isinstance(skip_unit, int) or skip_unit < 1:
        raise ValueError(f"skip_unit must be an integer >= 1, got {skip_unit!r}")
    if skip is None:
        if skip_unit != 1:
            raise ValueError("skip_unit needs skip=")
        return
    if scheme not in MASKED_SCHEMES:
        raise ValueError(f"scheme {scheme!r} has no masked kernels (skip=); served: " + ", ".join(MASKED_SCHEMES))
    if bands.dtype != torch.float64:
        raise ValueError("skip= needs float64 bands: the masked entries have no f32 storage form")
    if not isinstance(skip, torch.Tensor) or skip.dtype != torch.int32:
        raise ValueError("skip must be an int32 torch tensor on the columns' device")
    if ncol is None:
        return
    if ncol % skip_unit:
        raise ValueError(f"skip_unit = {skip_unit} does not divide ncol = {ncol}")
    if tuple(skip.shape) != (ncol // skip_unit,) or not skip.is_contiguous():
        raise ValueError(f"skip must be a contiguous ({ncol // skip_unit},) tensor (ncol // skip_unit), got {tuple(skip.shape)}")


class _SolvePlan:
    """What the solve plans share: the checks of scheme, method, geometry and spectra, the argument structs of the C entry, the
    workspace, and the call.  A subclass's ``__init__`` runs ``_check_options`` (and its own checks that need no column) first, then
    ``_bind``, builds ``out`` / ``_out``, and ends with ``_finish``; ``_tail`` gives the entry's arguments between the options and the
    workspace."""

    _bad_scheme = "unknown scheme {!r}; valid: " + ", ".join(SCHEMES)
    _scheme_arg = True  # the entry takes the scheme id first (Plan's per-scheme entries do not)
    _f32_series = False  # a sun series with float32 spectra is served (LevelsSeriesPlan)
    _s = None  # crt_sun_series of the series plans
    _mask = None  # crt_col_mask of a plan made with ``skip=`` (the six maskable plans)
    skip, skip_unit = None, 1
    use_skip = True  # False: the next calls evaluate every column through the plain entry (the mask stays bound)

    def _bind_skip(self, skip, skip_unit, entry):
        """``skip=`` / ``skip_unit=`` of the maskable plans, after ``_bind``: the device check, the struct and the masked entry
        ``entry`` (include_mask/crt1d_hip_masked.h).  The flags are read on the device at every call."""
        _check_skip(skip, skip_unit, self.cols.ncol, self.scheme, self.bands)
        if skip is None:
            return
        if skip.device != self.cols.device:
            raise ValueError(f"skip lives on {skip.device} but the columns on {self.cols.device}")
        self.skip, self.skip_unit = skip, int(skip_unit)
        self._mask = _lib.CrtColMask(skip.data_ptr(), int(skip_unit))
        self._entry_masked = entry
        self._fn_masked = getattr(self.lib, entry)

    def _check_options(self, scheme, tau_d_method):
        if scheme not in _lib.SCHEME_IDS:
            raise ValueError(self._bad_scheme.format(scheme))
        if tau_d_method not in _lib.TAU_D_METHODS:
            raise ValueError("invalid `method`. Valid options are 'quad' and '9sky'.")  # common.py:78

    def _bind(self, scheme, cols, bands, mu_s, tau_d_method, sun=None, tune=None):
        """Check the columns and spectra (for a series: against ``sun``) and build the structs ``_c``, ``_b``, ``_s``, ``_o``."""
        self.lib = _lib.load()
        self.scheme, self.cols, self.bands = scheme, cols, bands
        if scheme == "2s" and cols.mla is None:
            raise ValueError("solve_2s needs `mla`")
        if scheme != "bl" and bands.soil_r is None:
            raise ValueError(f"solve_{scheme} needs `soil_r`")
        if sun is None:
            cols.check_tables()
        else:
            self.sun = sun
            _check_sun(cols, bands, sun, self._f32_series)
            self._s = sun.c_struct()
        _check_band_device(bands, cols.device)
        self._c, self._b = cols.c_struct(), bands.c_struct(cols.ncol)
        self._o = _lib.CrtOptions(float(mu_s), _lib.TAU_D_METHODS[tau_d_method], 0)
        self.set_tune(tune or {})

    def _finish(self, entry, need, workspace):
        self.workspace = _check_workspace(workspace, need, self.cols.device)
        self._wsb = self.workspace.numel() * self.workspace.element_size()
        self._entry = entry
        self._fn = getattr(self.lib, entry)

    def set_tune(self, tune):
        """Measurement aid: per-plan overrides of the kernel-selection heuristics (``crt_options.tune``; keys ``_lib.TUNE_*``,
        documented in include/crt1d_hip.h).  ``{}`` = automatic.  They travel with every call of this plan -- no process-global state."""
        _lib.set_tune(self._o, tune)
        return self

    def last_kernel(self):
        """Name / configuration of the kernel(s) this thread's most recent call launched (``crt_hip_last_kernel``)."""
        return self.lib.crt_hip_last_kernel().decode()

    def __call__(self, stream=None, *, flags=0):
        """Enqueue on ``stream`` (default: torch's current stream).  ``flags``: ``_lib.FLAG_SKIP_PRECOMPUTE`` reuses
        the column records already in the workspace (same geometry, new spectra); ``_lib.FLAG_PRECOMPUTE_ONLY``
        runs only the column precompute."""
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        self._o.flags = int(flags)
        c, b, o = ctypes.byref(self._c), ctypes.byref(self._b), ctypes.byref(self._o)
        head = (c, b, o) if self._s is None else (c, b, ctypes.byref(self._s), o)
        if self._scheme_arg:
            head = (_lib.SCHEME_IDS[self.scheme],) + head
        masked = self._mask is not None and self.use_skip
        fn, entry, mask = (self._fn_masked, self._entry_masked, (ctypes.byref(self._mask),)) if masked else (self._fn, self._entry, ())
        with torch.cuda.device(dev):  # the launch goes to the CURRENT device: make it the one the buffers live on
            st = fn(*head, *self._tail(), self.workspace.data_ptr(), self._wsb, s.cuda_stream, *mask)
        _lib.check(st, entry)
        return self.out


class Plan(_SolvePlan):
    """Pre-validated launch of one scheme on fixed buffers: ``plan()`` enqueues K0 + the solve kernel
    on the current stream with no allocation and no host synchronisation (bench / steady-state use)."""

    _scheme_arg = False

    def __init__(self, scheme, cols: Columns, bands: Bands, *, mu_s=0.501, tau_d_method="quad", out=None, workspace=None,
                 placement="auto", tune=None):
        """``placement``: ``"auto"`` allocates output sets of 1 GB and more through the class-interleaving allocator
        (``crt_hip_buffer_alloc_set``: deterministic ~7 TB/s store mode); ``"none"`` uses ``torch.empty``
        (the store rate then depends on where the driver happens to put the arrays).  Ignored when ``out`` is given.

        ``out``: caller-owned output arrays (contiguous, of the bands' dtype), at any element offset.  One exception: zq_pa with
        float32 storage needs every output array to start on an 8-byte boundary (its kernels store band pairs and it has no
        other path in f32); a float32 array that starts at an odd element of an aligned allocation is a ValueError."""
        self._check_options(scheme, tau_d_method)
        self._bind(scheme, cols, bands, mu_s, tau_d_method, tune=tune)
        ncol, nz, nb = cols.ncol, cols.nz, bands.nb
        if placement not in ("auto", "none"):
            raise ValueError("placement must be 'auto' or 'none'")
        if out is None:
            placed = placement == "auto" and os.environ.get("CRT1D_PLACEMENT", "auto") != "none"
            out = alloc_outputs(scheme, ncol, nz, nb, cols.device, bands.dtype, placed=placed)
        shapes = {k: (ncol, nz - 1 if k in _MID_KEYS.get(scheme, ()) else nz, nb) for k in OUT_KEYS[scheme]}
        _outputs(shapes, out, bands.dtype, cols.device, "output {!r}", lacks=True)
        if scheme == "zq_pa" and bands.dtype == torch.float32:
            for k in shapes:
                if out[k].data_ptr() % 8:
                    raise ValueError(f"output {k!r}: zq_pa with float32 storage needs output arrays that start on an 8-byte boundary")
        if bands.dtype == torch.float32 and scheme not in _lib.F32_SCHEMES:
            raise TypeError(f"scheme {scheme!r} has no f32 storage variant yet")
        self._point_at(out)
        self._finish(f"crt_hip_{scheme}_{_io_suffix(bands)}", workspace_bytes(scheme, ncol, nz, nb), workspace)
        # where the output arrays live: memory-class letters per 512 MB chunk for arrays from the set allocator (None = torch memory)
        cls = {k: buffer_classes(v) for k, v in self.out.items()}
        self.placement_report = {"allocator": "crt_hip_buffer_alloc_set", "classes": cls} if any(cls.values()) else None

    def _point_at(self, out):
        self.out = out
        ptrs = [out[k].data_ptr() for k in OUT_KEYS[self.scheme]]
        ptrs += [None] * (7 - len(ptrs))
        self._out = _lib.CrtOutputs(*ptrs)

    def _tail(self):
        return (ctypes.byref(self._out),)


def solve(scheme, cols: Columns, bands: Bands, *, mu_s=0.501, tau_d_method="quad", out=None, workspace=None, placement="none"):
    """Run ``scheme`` over all (column, band) pairs; returns a dict of ``(ncol, nz, nb)`` CUDA tensors.

    Asynchronous on the current stream, like any torch op.  One-shot calls take their outputs from torch's caching allocator
    (``placement="none"``): allocation then costs microseconds, but output sets of a GB and more land wherever the driver put them and the
    solve kernel runs 10-20 % below what a class-interleaved set allows (0.77-0.83 of the HBM peak instead of 0.87-0.89, DESIGN.md
    section 3.1).  Steady-state users build a :class:`Plan` once (``placement="auto"``: ~2 ms per 512 MB chunk at construction, nothing
    per call) or pass ``placement="auto"`` here when the set is large enough for that to pay.
    """
    with torch.cuda.device(cols.device):
        return Plan(scheme, cols, bands, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace, placement=placement)()


def _io_suffix(bands):
    """Entry-point suffix of the storage type of ``bands``: ``"f64"`` or ``"f32"`` (f32 storage: float spectra / profiles, fp64 arithmetic)."""
    return "f32" if bands.dtype == torch.float32 else "f64"


def _check_epilogue_inputs(cols, bands, sol):
    """The epilogue reads the leaf optics of ``bands`` and the three profiles with ONE element type: float64 bands with float64
    profiles (``crt_hip_absorb*_f64``) or float32 bands with float32 profiles, e.g. the output of an f32 solve
    (``crt_hip_absorb*_f32``).  Mixed precision is a TypeError: a profile read with the wrong element size would run past the end of
    its allocation."""
    _check_band_device(bands, cols.device)
    bands.col_stride(cols.ncol)
    cols.check_tables()
    for k in ("I_dr", "I_df_d", "I_df_u"):
        if k not in sol:
            raise ValueError(f"`sol` lacks {k!r}")
        if isinstance(sol[k], torch.Tensor) and sol[k].dtype != bands.dtype:
            raise TypeError(f"sol[{k!r}] is {sol[k].dtype} but the bands are {bands.dtype}: profiles and bands must share one storage type")
        _check_profile(sol[k], f"sol[{k!r}]", (cols.ncol, cols.nz, bands.nb), cols.device, bands.dtype)


BANDSUM_KEYS = ("aI", "aI_sl", "aI_sh", "totals")
# with ``profiles=True``: the direct-beam part of the absorption and the band-integrated LEVEL profiles of every irradiance variable
# ``diagnostics.band`` reduces (crt1d/diagnostics.py:84-91; the "I..." / "F" variables of ``Model.to_xr``, model.py:421-426)
PROFILE_KEYS = ("aI_dr", "I_dr", "I_df_d", "I_df_u", "F", "I_d")


def bandsum_shapes(ncol, nz, ngroup, profiles=False):
    """Shapes of the integrated outputs, in ``BANDSUM_KEYS`` (+ ``PROFILE_KEYS``) order."""
    sh = {"aI": (ncol, nz - 1, ngroup), "aI_sl": (ncol, nz - 1, ngroup), "aI_sh": (ncol, nz - 1, ngroup), "totals": (ncol, ngroup, 4)}
    if profiles:
        sh["aI_dr"] = (ncol, nz - 1, ngroup)
        for k in PROFILE_KEYS[1:]:
            sh[k] = (ncol, nz, ngroup)
    return sh


def _bandsum_out_struct(out, profiles):
    keys = BANDSUM_KEYS + (PROFILE_KEYS if profiles else ())
    return _lib.CrtBandsumOut(**{k: out[k].data_ptr() for k in keys})


def absorption_from_bandsums(res):
    """The seven entries of the reference's absorption dict (``model.py:637-647``), band-integrated, from a ``profiles=True`` result:
    ``aI_df = aI - aI_dr``, ``aI_df_sl = aI_sl - aI_dr``, ``aI_df_sh = aI_sh`` (``model.py:628-634``)."""
    return {"aI": res["aI"], "aI_dr": res["aI_dr"], "aI_df": res["aI"] - res["aI_dr"], "aI_sl": res["aI_sl"], "aI_sh": res["aI_sh"],
            "aI_df_sl": res["aI_sl"] - res["aI_dr"], "aI_df_sh": res["aI_sh"]}


class BandSumPlan:
    """Pre-validated launch of the epilogue (``crt_hip_absorb_bandsum2_f64``, or ``_f32`` for float32 bands and profiles) on fixed
    buffers: ``plan()`` enqueues the kernel with no allocation and no host synchronisation.  ``out`` may hold caller-owned output
    tensors (e.g. views into one packed message buffer, :class:`crt1d_amd.dist.BandShardPlan`); they are float64 for both storage
    types, and the f32 band sums equal the f64 band sums of the upcast profiles bit for bit."""

    def __init__(self, cols: Columns, bands: Bands, sol, band_w, out=None, profiles=False):
        self.lib = _lib.load()
        ncol, nz, dev = cols.ncol, cols.nz, cols.device
        band_w = _band_weights(band_w, bands.nb, dev)
        ng = band_w.shape[0]
        _check_epilogue_inputs(cols, bands, sol)
        out = _outputs(bandsum_shapes(ncol, nz, ng, profiles), out, torch.float64, dev)
        self.cols, self.bands, self.sol, self.band_w, self.out, self.ng, self.profiles = cols, bands, sol, band_w, out, ng, profiles
        self._c, self._b = cols.c_struct(), bands.c_struct(ncol)
        self._o = _bandsum_out_struct(out, profiles)
        self._entry = f"crt_hip_absorb_bandsum2_{_io_suffix(bands)}"
        self._fn = getattr(self.lib, self._entry)

    def __call__(self, stream=None):
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        sol = self.sol
        with torch.cuda.device(dev):
            st = self._fn(ctypes.byref(self._c), ctypes.byref(self._b), sol["I_dr"].data_ptr(), sol["I_df_d"].data_ptr(),
                          sol["I_df_u"].data_ptr(), self.band_w.data_ptr(), self.ng, ctypes.byref(self._o), s.cuda_stream)
        _lib.check(st, self._entry)
        return self.out


def absorb_bandsum(cols: Columns, bands: Bands, sol, band_w, out=None, profiles=False):
    """Layer absorption (``model.py:573-647``) reduced over bands with weights ``band_w (ngroup, nb)``
    (``diagnostics.py:39-108``).  Returns ``aI, aI_sl, aI_sh`` ``(ncol, nz-1, ngroup)`` and the
    energy-balance terms ``totals (ncol, ngroup, 4)`` = incoming, reflected, transmitted, soil-reflected.
    ``profiles=True`` adds everything else ``diagnostics.band`` returns (``PROFILE_KEYS``): the band-integrated level profiles
    ``I_dr, I_df_d, I_df_u, F, I_d (ncol, nz, ngroup)`` and ``aI_dr (ncol, nz-1, ngroup)`` (:func:`absorption_from_bandsums`).
    Photon-flux variants (``calc_PFD``) are a choice of weights: ``spectra.band_weights(..., wl=..., pfd=True)``.
    ``bands`` and the profiles ``sol`` are both float64 or both float32 (f32 storage); the outputs are float64 either way."""
    return dict(BandSumPlan(cols, bands, sol, band_w, out=out, profiles=profiles)())


class BandSumFinishPlan:
    """Pre-validated launch of ``crt_hip_bandsum_finish_f64`` on fixed ``profiles=True`` band-sum buffers ``out``: re-forms, in place,
    ``aI = aI_sl + aI_sh`` and the level profiles ``F``, ``I_d`` from the level sums ``I_dr, I_df_d, I_df_u`` -- the outputs
    :class:`crt1d_amd.dist.BandShardPlan` does not send, after the all-reduce of the others.  ``F`` and ``I_d`` are the bits the
    epilogue writes for the same sums."""

    def __init__(self, cols: Columns, out):
        self.lib = _lib.load()
        ncol, nz, dev = cols.ncol, cols.nz, cols.device
        ng = out["aI"].shape[-1] if out["aI"].ndim == 3 else 0
        if not 1 <= ng <= 4:
            raise ValueError("out['aI'] must be (ncol, nz-1, ngroup <= 4)")
        for k, sh in bandsum_shapes(ncol, nz, ng, profiles=True).items():
            if k not in ("totals", "aI_dr"):
                _check_profile(out[k], f"out[{k!r}]", sh, dev)
        self.cols, self.out, self.ng = cols, out, ng
        self._c = cols.c_struct()
        self._o = _lib.CrtBandsumOut(**{k: out[k].data_ptr() for k in ("aI", "aI_sl", "aI_sh", "I_dr", "I_df_d", "I_df_u", "F", "I_d")})

    def __call__(self, stream=None):
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.device(dev):
            st = self.lib.crt_hip_bandsum_finish_f64(ctypes.byref(self._c), self.ng, ctypes.byref(self._o), s.cuda_stream)
        _lib.check(st, "crt_hip_bandsum_finish_f64")
        return self.out


def bandsum_finish(cols: Columns, out):
    """``aI``, ``F`` and ``I_d`` of the ``profiles=True`` band sums ``out`` re-formed in place from ``aI_sl, aI_sh, I_dr, I_df_d, I_df_u``
    (:class:`BandSumFinishPlan`); returns ``out``."""
    return BandSumFinishPlan(cols, out)()


ABSORPTION_KEYS = ("aI", "aI_df", "aI_dr", "aI_sh", "aI_sl", "aI_df_sl", "aI_df_sh")  # model.py:637-647


def absorb(cols: Columns, bands: Bands, sol):
    """Per-band layerwise absorption: the reference's ``Model.absorption`` dict (``model.py:573-647``), batched.
    Returns the seven ``(ncol, nz-1, nb)`` arrays plus ``laim``, ``f_slm`` ``(ncol, nz-1)``.
    ``bands`` and ``sol`` are both float64 or both float32; with float32 (f32 storage) the seven per-band arrays are float32 -- the
    fp64 result rounded once -- and ``laim``, ``f_slm`` stay float64."""
    lib = _lib.load()
    ncol, nz, nb = cols.ncol, cols.nz, bands.nb
    dev = cols.device
    _check_epilogue_inputs(cols, bands, sol)
    entry = f"crt_hip_absorb_{_io_suffix(bands)}"
    out = {k: torch.empty((ncol, nz - 1, nb), dtype=bands.dtype, device=dev) for k in ABSORPTION_KEYS}
    laim = torch.empty((ncol, nz - 1), dtype=torch.float64, device=dev)
    f_slm = torch.empty_like(laim)
    ptrs = (ctypes.c_void_p * 7)(*[out[k].data_ptr() for k in ABSORPTION_KEYS])
    c, b = cols.c_struct(), bands.c_struct(ncol)
    with torch.cuda.device(dev):
        st = getattr(lib, entry)(ctypes.byref(c), ctypes.byref(b), sol["I_dr"].data_ptr(), sol["I_df_d"].data_ptr(),
                                 sol["I_df_u"].data_ptr(), ptrs, laim.data_ptr(), f_slm.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, entry)
    out["laim"] = laim
    out["f_slm"] = f_slm
    return out


class IntegratedPlan(_SolvePlan):
    """Fused solve + absorption + band integrals (``crt_hip_integrated2_f64``, or ``_f32`` for float32 bands): no profile ever
    reaches HBM.  Outputs as :func:`absorb_bandsum`: ``aI, aI_sl, aI_sh (ncol, nz-1, ngroup)``, ``totals (ncol, ngroup, 4)``; float64
    for both storage types."""

    _bad_scheme = "scheme {!r} has no integrated kernel"

    def __init__(self, scheme, cols: Columns, bands: Bands, band_w, *, mu_s=0.501, tau_d_method="quad", workspace=None, out=None,
                 profiles=False):
        self._check_options(scheme, tau_d_method)
        self._bind_sums(scheme, cols, bands, band_w, mu_s, tau_d_method, out, profiles)
        self._finish(f"crt_hip_integrated2_{_io_suffix(bands)}", workspace_bytes(scheme, cols.ncol, cols.nz, bands.nb), workspace)

    def _bind_sums(self, scheme, cols, bands, band_w, mu_s, tau_d_method, out, profiles, sun=None):
        """``_bind`` + the band weights and the band-sum outputs (with ``sun``: of every sun state)."""
        self.band_w = _band_weights(band_w, bands.nb, cols.device)
        self._bind(scheme, cols, bands, mu_s, tau_d_method, sun=sun)
        ncol, nz, ng = cols.ncol, cols.nz, self.band_w.shape[0]
        shapes = bandsum_shapes(ncol, nz, ng, profiles) if sun is None else series_shapes(ncol, sun.nt, nz, ng, profiles)
        self.out = _outputs(shapes, out, torch.float64, cols.device)
        self.profiles = profiles
        self._out = _bandsum_out_struct(self.out, profiles)

    def _tail(self):
        return self.band_w.data_ptr(), self.band_w.shape[0], ctypes.byref(self._out)


def solve_integrated(scheme, cols: Columns, bands: Bands, band_w, **kw):
    with torch.cuda.device(cols.device):
        return IntegratedPlan(scheme, cols, bands, band_w, **kw)()


@dataclass
class SunSeries:
    """``nt`` sun states per column on one canopy (``crt_sun_series``): ``psi (ncol, nt)`` solar zenith angles in radians and the
    incoming spectra ``I_dr0``, ``I_df0`` ``(ncol, nt, nb)`` -- or ``(nt, nb)`` / ``(1, nt, nb)`` to share one series of spectra over all
    columns.  ``g_at_psi (ncol, nt)`` = G(psi) for columns of kind G_TABLE.  What the reference passes step by step through
    ``update_p(psi=...)`` and ``I_dr0_all`` / ``I_df0_all``."""

    psi: torch.Tensor
    I_dr0: torch.Tensor
    I_df0: torch.Tensor
    g_at_psi: Optional[torch.Tensor] = None

    _c_type = _lib.CrtSunSeries

    @staticmethod
    def _spectrum(t, name):  # check of I_dr0 / I_df0 (SunSeriesF32: float32)
        return _f64(t, name)

    def __post_init__(self):
        self.psi = _f64(self.psi, "psi")
        if self.psi.ndim != 2 or self.psi.shape[1] < 1:
            raise ValueError("psi must be (ncol, nt) with nt >= 1")
        if self.g_at_psi is not None:
            self.g_at_psi = _f64(self.g_at_psi, "g_at_psi")
            if self.g_at_psi.shape != self.psi.shape:
                raise ValueError("g_at_psi must be (ncol, nt)")
        shape = None
        for name in ("I_dr0", "I_df0"):
            v = self._spectrum(getattr(self, name), name)
            if v.ndim == 2:
                v = v[None]
            if v.ndim != 3 or v.shape[1] != self.nt or v.shape[0] not in (1, self.ncol):
                raise ValueError(f"{name} must be (ncol, nt, nb) or (nt, nb) with ncol = {self.ncol}, nt = {self.nt}")
            if shape is None:
                shape = v.shape
            elif v.shape != shape:
                raise ValueError("I_dr0 and I_df0 must have the same shape")
            setattr(self, name, v)
        for name in ("I_dr0", "I_df0", "g_at_psi"):
            v = getattr(self, name)
            if v is not None and v.device != self.psi.device:
                raise ValueError(f"{name} lives on {v.device} but psi on {self.psi.device}")

    @property
    def ncol(self):
        return self.psi.shape[0]

    @property
    def nt(self):
        return self.psi.shape[1]

    @property
    def nb(self):
        return self.I_dr0.shape[2]

    @property
    def col_stride(self):
        return 0 if (self.I_dr0.shape[0] == 1 and self.ncol != 1) else self.nt * self.nb

    def slice(self, lo, hi):
        """Columns [lo, hi) as a view."""
        g = lambda t: t if t.shape[0] == 1 else t[lo:hi]  # noqa: E731
        return type(self)(self.psi[lo:hi], g(self.I_dr0), g(self.I_df0), None if self.g_at_psi is None else self.g_at_psi[lo:hi])

    def c_struct(self):
        return self._c_type(self.nt, self.psi.data_ptr(), None if self.g_at_psi is None else self.g_at_psi.data_ptr(), self.col_stride,
                                 self.I_dr0.data_ptr(), self.I_df0.data_ptr())

    @classmethod
    def from_host(cls, d, device="cuda"):
        """From a dict of NumPy arrays (:func:`crt1d_amd.synth.make_sun_series`)."""
        t = _host_reader(d, device)
        return cls(t("psi"), t("I_dr0"), t("I_df0"), t("g_at_psi"))


def _check_sun(cols, bands, sun, f32_ok):
    """A sun series against the columns and spectra it is solved with: storage type, ``ncol`` / ``nb``, device, and the tables of
    G_TABLE columns (``cols.psi`` / ``cols.g_at_psi`` are not read, so ``Columns.check_tables`` does not apply: up to two device->host
    syncs, each only where a table is missing)."""
    ncol, nb, dev = cols.ncol, bands.nb, cols.device
    if bands.dtype != sun.I_dr0.dtype:
        if not f32_ok:
            raise TypeError("the sun-angle series has no f32 storage form: bands must be float64")
        want = "SunSeriesF32" if bands.dtype == torch.float32 else "SunSeries"
        raise TypeError(f"{bands.dtype} bands need a {want}: the spectra of sun are {sun.I_dr0.dtype}")
    if sun.ncol != ncol or sun.nb != nb:
        raise ValueError(f"sun must have ncol = {ncol} rows and nb = {nb} bands, got {sun.ncol} and {sun.nb}")
    if sun.psi.device != dev:
        raise ValueError(f"sun lives on {sun.psi.device} but the columns on {dev}")
    if bands.leaf_r is None or bands.leaf_t is None:
        raise ValueError("bands needs leaf_r and leaf_t")
    if (cols.g_table is not None or cols.g_at_psi is not None) and sun.g_at_psi is None and bool((cols.g_kind == 6).any()):
        raise ValueError("columns with g_kind = G_TABLE need sun.g_at_psi (ncol, nt)")
    if cols.g_table is None and bool((cols.g_kind == 6).any()):
        raise ValueError("columns with g_kind = G_TABLE need g_table")


@dataclass
class SunSeriesF32(SunSeries):
    """:class:`SunSeries` with float32 incoming spectra ``I_dr0``, ``I_df0`` (``crt_sun_series_f32``, for float32 :class:`Bands`): half
    the bytes, widened on load; ``psi`` and ``g_at_psi`` stay float64.  Served by :class:`LevelsSeriesPlan` only."""

    _c_type = _lib.CrtSunSeriesF32

    @staticmethod
    def _spectrum(t, name):
        return _f32(t, name)

    @classmethod
    def from_host(cls, d, device="cuda"):
        """From a dict of NumPy arrays (:func:`crt1d_amd.synth.make_sun_series`); the spectra are rounded to float32."""
        t = _host_reader(d, device)
        return cls(t("psi"), t("I_dr0").to(torch.float32), t("I_df0").to(torch.float32), t("g_at_psi"))


def series_workspace_bytes(scheme, ncol, nz, nb, nt):
    """Device workspace of a series call: the canopy records of the columns and the sun records of every (column, t)."""
    return int(_lib.load().crt_hip_series_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nt))


def series_shapes(ncol, nt, nz, ngroup, profiles=False):
    """Shapes of the series outputs: :func:`bandsum_shapes` with ``nt`` inserted at axis 1."""
    return {k: (sh[0], nt) + tuple(sh[1:]) for k, sh in bandsum_shapes(ncol, nz, ngroup, profiles).items()}


class IntegratedSeriesPlan(IntegratedPlan):
    """The outputs of :class:`IntegratedPlan` for ``sun.nt`` sun states of every column in one call
    (``crt_hip_integrated_series_f64``): ``out[k][:, t]`` is bitwise what ``IntegratedPlan`` returns with ``psi = sun.psi[:, t]`` and
    the incoming spectra of step ``t``.  The canopy-only part of the column precompute runs once per column, the sun-dependent part
    once per (column, t).  ``cols.psi``, ``cols.g_at_psi`` and ``bands.I_dr0`` / ``I_df0`` are not read (``bands`` may be built with
    ``None`` for the two).  float64 only."""

    def __init__(self, scheme, cols: Columns, bands: Bands, sun: SunSeries, band_w, *, mu_s=0.501, tau_d_method="quad", workspace=None,
                 out=None, profiles=False):
        self._check_options(scheme, tau_d_method)
        if not isinstance(sun, SunSeries) or isinstance(sun, SunSeriesF32):
            raise TypeError("sun must be a SunSeries (float64 spectra)")
        self._bind_sums(scheme, cols, bands, band_w, mu_s, tau_d_method, out, profiles, sun=sun)
        self._finish("crt_hip_integrated_series_f64", series_workspace_bytes(scheme, cols.ncol, cols.nz, bands.nb, sun.nt), workspace)


def solve_integrated_series(scheme, cols: Columns, bands: Bands, sun: SunSeries, band_w, **kw):
    with torch.cuda.device(cols.device):
        return IntegratedSeriesPlan(scheme, cols, bands, sun, band_w, **kw)()


LEVEL_KEYS = ("I_dr", "I_df_d", "I_df_u", "F")  # the profiles a level-subset solve serves, in crt_outputs slot order


def normalize_levels(levels, nz):
    """The level selection of :class:`LevelsPlan` as a sorted tuple of distinct indices in ``[0, nz)``.  ``levels`` is an int or an
    iterable of ints; negative values count from the top as in NumPy (``-1`` = ``nz - 1``, the canopy top).  ValueError for an empty
    or too long selection (more than ``_lib.MAX_LEVEL_SELECT``), a non-integer, a level outside ``[-nz, nz)`` and a level given twice."""
    import operator

    if hasattr(levels, "tolist"):  # NumPy / torch integers and arrays
        levels = levels.tolist()
    if not hasattr(levels, "__iter__"):
        levels = [levels]
    try:
        raw = [operator.index(v) for v in levels]
    except TypeError as e:
        raise ValueError(f"levels must be integers: {e}") from None
    if not raw:
        raise ValueError("levels is empty: select at least one level")
    out = []
    for v in raw:
        if not -nz <= v < nz:
            raise ValueError(f"level {v} is out of range for nz = {nz} (valid: {-nz} .. {nz - 1})")
        out.append(v + nz if v < 0 else v)
    if len(set(out)) != len(out):
        dup = sorted({v for v in out if out.count(v) > 1})
        raise ValueError(f"level(s) {dup} selected more than once (negative indices count from nz = {nz})")
    if len(out) > _lib.MAX_LEVEL_SELECT:
        raise ValueError(f"{len(out)} levels selected; one call serves at most {_lib.MAX_LEVEL_SELECT}")
    return tuple(sorted(out))


def _level_keys(keys, allowed=LEVEL_KEYS):
    """The profile selection of the level plans as a tuple of distinct names out of ``allowed``."""
    keys = (keys,) if isinstance(keys, str) else tuple(keys)
    if not keys or any(k not in allowed for k in keys) or len(set(keys)) != len(keys):
        raise ValueError(f"keys must be distinct names out of {allowed}, got {keys!r}")
    return keys


class LevelsPlan(_SolvePlan):
    """Pre-validated level-subset solve (``crt_hip_levels_f64``, or ``_f32`` for float32 bands): the spectra of ``keys`` (any of
    ``I_dr, I_df_d, I_df_u, F``) at the levels ``levels`` only, each ``(ncol, nsel, nb)`` in the dtype of ``bands``; row ``r`` is level
    ``self.levels[r]`` (sorted, negatives resolved: :func:`normalize_levels`).  Every row is bitwise the row of :func:`solve`'s profile
    for the same inputs; the other levels are never written (at 60 levels and two selected, 3 % of the bytes)."""

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, *, keys=LEVEL_KEYS, mu_s=0.501, tau_d_method="quad", out=None,
                 workspace=None):
        self._check_options(scheme, tau_d_method)
        self._bind_levels(scheme, cols, bands, levels, _level_keys(keys), mu_s, tau_d_method, out)
        self._finish(f"crt_hip_levels_{_io_suffix(bands)}", workspace_bytes(scheme, cols.ncol, cols.nz, bands.nb), workspace)

    def _bind_levels(self, scheme, cols, bands, levels, keys, mu_s, tau_d_method, out, sun=None):
        """``_bind`` + the level list ``_lev`` and the outputs of ``keys`` (with ``sun``: of every sun state), NULL in ``_out`` for the rest."""
        self.levels, self.keys = normalize_levels(levels, cols.nz), keys
        self._bind(scheme, cols, bands, mu_s, tau_d_method, sun=sun)
        shape = (cols.ncol,) + (() if sun is None else (sun.nt,)) + (len(self.levels), bands.nb)
        out = _outputs({k: shape for k in keys}, out, bands.dtype, cols.device, "output {!r}", lacks=True)
        self.out = {k: out[k] for k in keys}
        self._out = _lib.CrtOutputs(*[out[k].data_ptr() if k in keys else None for k in LEVEL_KEYS], None, None, None)
        self._lev = (ctypes.c_int32 * len(self.levels))(*self.levels)

    def _tail(self):
        return self._lev, len(self.levels), ctypes.byref(self._out)


def solve_levels(scheme, cols: Columns, bands: Bands, levels, **kw):
    """One-shot :class:`LevelsPlan`: ``{key: (ncol, nsel, nb)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    with torch.cuda.device(cols.device):
        return LevelsPlan(scheme, cols, bands, levels, **kw)()


def spectral_totals(scheme, cols: Columns, bands: Bands, **kw):
    """The per-band terms of the reference's energy balance (``compare_ebal``, diagnostics.py:510-522) before their band integral:
    ``(ncol, nb, 4)`` float64 with, in the order of ``totals``, the incoming ``I_d[top]``, reflected ``I_df_u[top]``, transmitted
    ``I_d[0]`` and soil-reflected ``I_df_u[0]`` spectra (``I_d = I_dr + I_df_d``), from one level-subset solve at the ground and the top.
    Contracted with band weights ``w`` (``torch.einsum("cbq,gb->cgq", t, w)``) it gives :class:`IntegratedPlan`'s ``totals``.  The
    canopy albedo spectrum is ``t[..., 1] / t[..., 0]``, the canopy transmittance ``t[..., 2] / t[..., 0]``.  ``kw`` as for
    :class:`LevelsPlan` (``levels`` and ``keys`` are fixed here)."""
    nz = cols.nz
    r = solve_levels(scheme, cols, bands, (0, nz - 1), keys=("I_dr", "I_df_d", "I_df_u"), **kw)
    dr, dn, up = (r[k].to(torch.float64) for k in ("I_dr", "I_df_d", "I_df_u"))
    i_d = dr + dn
    return torch.stack((i_d[:, 1], up[:, 1], i_d[:, 0], up[:, 0]), dim=-1)


def levels_series_workspace_bytes(scheme, ncol, nz, nt):
    """Device workspace of a :class:`LevelsSeriesPlan` call: the canopy records of the columns and the sun records of every (column, t).
    Never larger than :func:`series_workspace_bytes`, and laid out the same way: one buffer of that size serves both series plans."""
    return int(_lib.load().crt_hip_levels_series_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nt))


class LevelsSeriesPlan(LevelsPlan):
    """The outputs of :class:`LevelsPlan` for ``sun.nt`` sun states of every column in one call (``crt_hip_levels_series_f64``, or
    ``_f32`` for float32 bands and a :class:`SunSeriesF32`): the spectra of ``keys`` at the levels ``levels``, each
    ``(ncol, nt, nsel, nb)`` in the dtype of ``bands``.  ``out[k][:, t]`` is bitwise what ``LevelsPlan`` returns with
    ``psi = sun.psi[:, t]`` and the incoming spectra of step ``t`` -- hence bitwise rows of :func:`solve` of that step.  The canopy-only part
    of the column precompute runs once per column, the sun-dependent part once per (column, t).  ``cols.psi``, ``cols.g_at_psi`` and
    ``bands.I_dr0`` / ``I_df0`` are not read (``bands`` may be built with ``None`` for the two).  Any ``nb``."""

    _f32_series = True

    def __init__(self, scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, *, keys=LEVEL_KEYS, mu_s=0.501, tau_d_method="quad",
                 out=None, workspace=None):
        self._check_options(scheme, tau_d_method)
        if not isinstance(sun, SunSeries):
            raise TypeError("sun must be a SunSeries or a SunSeriesF32")
        self._bind_levels(scheme, cols, bands, levels, _level_keys(keys), mu_s, tau_d_method, out, sun=sun)
        self._finish(f"crt_hip_levels_series_{_io_suffix(bands)}", levels_series_workspace_bytes(scheme, cols.ncol, cols.nz, sun.nt), workspace)


def solve_levels_series(scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, **kw):
    """One-shot :class:`LevelsSeriesPlan`: ``{key: (ncol, nt, nsel, nb)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    with torch.cuda.device(cols.device):
        return LevelsSeriesPlan(scheme, cols, bands, sun, levels, **kw)()


def spectral_totals_series(scheme, cols: Columns, bands: Bands, sun: SunSeries, **kw):
    """:func:`spectral_totals` with a time axis: ``(ncol, nt, nb, 4)`` float64 -- incoming ``I_d[top]``, reflected ``I_df_u[top]``,
    transmitted ``I_d[0]`` and soil-reflected ``I_df_u[0]`` spectra of every sun state -- from one level-series call at the ground and the
    top.  Slice ``[:, t]`` is bitwise :func:`spectral_totals` of step ``t``.  ``kw`` as for :class:`LevelsSeriesPlan`."""
    nz = cols.nz
    r = solve_levels_series(scheme, cols, bands, sun, (0, nz - 1), keys=("I_dr", "I_df_d", "I_df_u"), **kw)
    dr, dn, up = (r[k].to(torch.float64) for k in ("I_dr", "I_df_d", "I_df_u"))
    i_d = dr + dn
    return torch.stack((i_d[:, :, 1], up[:, :, 1], i_d[:, :, 0], up[:, :, 0]), dim=-1)


# ---- sensor-band outputs (include/crt1d_hip_sensor.h) -------------------------------------------------------------------------------


class SensorSet:
    """The spectral responses of ``nsens <= _lib.MAX_SENSOR_BANDS`` sensor bands on the ``nb`` model bands, as the sensor plans read them
    (``crt_sensor_set``): per sensor band the support ``[first, first + count)`` and its weights, packed one support after the other.

    ``SensorSet(weights)``: dense ``(nsens, nb)`` weights (NumPy array or tensor); the support of a row is the span from its first to its
    last nonzero weight -- zeros inside the span are kept, the zeros outside are never multiplied.  An all-zero row is a ValueError.
    :meth:`from_supports` takes the supports as they are.  ``first`` / ``count`` live on the host (``np.int32``), ``w`` is the packed
    float64 tensor on ``device`` (default: the current GPU)."""

    def __init__(self, weights, device=None):
        import numpy as np

        dev = weights.device if isinstance(weights, torch.Tensor) and weights.is_cuda else device
        w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights
        w = np.asarray(w, dtype=np.float64)
        if w.ndim == 1:
            w = w[None, :]
        if w.ndim != 2 or w.shape[1] < 1:
            raise ValueError("weights must be (nsens, nb)")
        self._check_nsens(w.shape[0])
        first, count, packed = [], [], []
        for s, row in enumerate(w):
            nzr = np.flatnonzero(row)
            if nzr.size == 0:
                raise ValueError(f"sensor band {s} has no nonzero weight")
            first.append(int(nzr[0]))
            count.append(int(nzr[-1]) - int(nzr[0]) + 1)
            packed.append(row[nzr[0]:nzr[-1] + 1])
        self._set(w.shape[1], first, count, np.concatenate(packed), dev)

    @staticmethod
    def _check_nsens(nsens):
        if not 1 <= nsens <= _lib.MAX_SENSOR_BANDS:
            raise ValueError(f"{nsens} sensor bands; one set holds 1 .. {_lib.MAX_SENSOR_BANDS}")

    def _set(self, nb, first, count, packed, device):
        import numpy as np

        self.nb = None if nb is None else int(nb)
        self.first = np.ascontiguousarray(first, dtype=np.int32)
        self.count = np.ascontiguousarray(count, dtype=np.int32)
        self.nsens = int(self.first.size)
        if device is None:  # the current GPU; without one the set stays on the host (and no plan takes it)
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        if isinstance(packed, torch.Tensor):
            self.w = _f64(packed, "packed_w")
            if not self.w.is_cuda:
                self.w = self.w.to(device)
        else:
            self.w = torch.as_tensor(np.ascontiguousarray(packed, dtype=np.float64)).to(device)

    @classmethod
    def from_supports(cls, first, count, packed_w, nb=None, device=None):
        """``first``, ``count``: ``(nsens,)`` ints (``count >= 1``, ``first >= 0``; supports may overlap, in any order); ``packed_w``: the
        ``sum(count)`` weights, those of sensor band ``s`` at ``off[s] .. off[s] + count[s]`` with ``off`` the exclusive prefix sum of
        ``count``.  ``nb``: the model band count, when known (a plan checks the supports against its bands either way)."""
        import numpy as np

        first, count = np.atleast_1d(np.asarray(first)), np.atleast_1d(np.asarray(count))
        if first.ndim != 1 or first.shape != count.shape or not (np.issubdtype(first.dtype, np.integer) and np.issubdtype(count.dtype, np.integer)):
            raise ValueError("first and count must be integer arrays of one shape (nsens,)")
        cls._check_nsens(first.size)
        if (count < 1).any() or (first < 0).any():
            raise ValueError("every support needs count >= 1 and first >= 0")
        if nb is not None and (first.astype(np.int64) + count > nb).any():
            raise ValueError(f"a support reaches beyond nb = {nb}")
        n = int(count.astype(np.int64).sum())
        if (packed_w.numel() if isinstance(packed_w, torch.Tensor) else np.size(packed_w)) != n or np.ndim(packed_w) != 1:
            raise ValueError(f"packed_w must hold sum(count) = {n} weights in one dimension")
        self = cls.__new__(cls)
        self._set(nb, first, count, packed_w, device)
        return self

    @property
    def offsets(self):
        """Exclusive prefix sum of ``count``: where the weights of each sensor band start in ``w``."""
        import numpy as np

        return np.concatenate(([0], np.cumsum(self.count[:-1], dtype=np.int64)))

    def dense(self, nb=None):
        """The ``(nsens, nb)`` NumPy array of the weights (zeros outside the supports)."""
        import numpy as np

        nb = self.nb if nb is None else nb
        if nb is None:
            raise ValueError("nb is not known: pass it")
        w, out = self.w.cpu().numpy(), np.zeros((self.nsens, nb))
        for s, (f, n, o) in enumerate(zip(self.first, self.count, self.offsets)):
            out[s, f:f + n] = w[o:o + n]
        return out

    def check(self, nb, device):
        """The checks of a plan: the supports lie in ``[0, nb)`` and the weights on ``device``."""
        if self.nb is not None and self.nb != nb:
            raise ValueError(f"the sensor set was built for nb = {self.nb} bands, the spectra have {nb}")
        if int((self.first.astype("int64") + self.count).max()) > nb:
            raise ValueError(f"a sensor support reaches beyond nb = {nb}")
        if self.w.device != device:
            raise ValueError(f"the sensor weights live on {self.w.device} but the columns on {device}")

    def c_struct(self):
        P = ctypes.POINTER(ctypes.c_int32)
        return _lib.CrtSensorSet(self.nsens, self.first.ctypes.data_as(P), self.count.ctypes.data_as(P), self.w.data_ptr())


def sensor_workspace_bytes(scheme, ncol, nz, nb, nsel, nsens):
    """Device workspace of a :class:`SensorLevelsPlan` call: the records of :func:`workspace_bytes` and, with several band slices, the
    partial sums behind them."""
    return int(_lib.load().crt_hip_sensor_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nsel, nsens))


def sensor_series_workspace_bytes(scheme, ncol, nz, nb, nt, nsel, nsens):
    """Device workspace of a :class:`SensorLevelsSeriesPlan` call: the records of :func:`levels_series_workspace_bytes`, then partial sums."""
    return int(_lib.load().crt_hip_sensor_series_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nt, nsel, nsens))


class SensorLevelsPlan(_SolvePlan):
    """Pre-validated sensor-band solve (``crt_hip_sensor_levels_f64``, or ``_f32`` for float32 bands): ``out[k][c, r, s]`` is the sum over
    the support of sensor band ``s`` of ``w_s[b] * X[c, levels[r], b]`` for ``X`` in ``keys`` (any of ``I_dr, I_df_d, I_df_u, F``), each
    ``(ncol, nsel, nsens)`` float64 for both storage types.  ``X`` is the row :class:`LevelsPlan` gives; it is reduced inside the level
    kernel and never written.  The summation order depends on the scheme, ``nz``, ``nb``, ``nsel`` and the sensor set only: a column's
    sums are bitwise the same alone or in any batch."""

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, *, keys=LEVEL_KEYS, mu_s=0.501, tau_d_method="quad",
                 out=None, workspace=None, skip=None, skip_unit=1):
        self._check_options(scheme, tau_d_method)
        _check_skip(skip, skip_unit, getattr(cols, "ncol", None), scheme, bands)
        self._bind_sensors(scheme, cols, bands, levels, sensors, _level_keys(keys), mu_s, tau_d_method, out)
        need = sensor_workspace_bytes(scheme, cols.ncol, cols.nz, bands.nb, len(self.levels), sensors.nsens)
        self._finish(f"crt_hip_sensor_levels_{_io_suffix(bands)}", need, workspace)
        self._bind_skip(skip, skip_unit, "crt_hip_sensor_levels_masked_f64")

    def _bind_sensors(self, scheme, cols, bands, levels, sensors, keys, mu_s, tau_d_method, out, sun=None):
        """``_bind`` + the level list, the sensor set and the outputs of ``keys`` (with ``sun``: of every sun state), NULL for the rest."""
        if not isinstance(sensors, SensorSet):
            raise TypeError("sensors must be a SensorSet")
        self.levels, self.keys, self.sensors = normalize_levels(levels, cols.nz), keys, sensors
        sensors.check(bands.nb, cols.device)
        self._bind(scheme, cols, bands, mu_s, tau_d_method, sun=sun)
        shape = (cols.ncol,) + (() if sun is None else (sun.nt,)) + (len(self.levels), sensors.nsens)
        out = _outputs({k: shape for k in keys}, out, torch.float64, cols.device, "output {!r}", lacks=True)
        self.out = {k: out[k] for k in keys}
        self._out = _lib.CrtSensorOut(*[out[k].data_ptr() if k in keys else None for k in LEVEL_KEYS])
        self._lev = (ctypes.c_int32 * len(self.levels))(*self.levels)
        self._sens = sensors.c_struct()

    def _tail(self):
        return self._lev, len(self.levels), ctypes.byref(self._sens), ctypes.byref(self._out)


def solve_sensor_levels(scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, **kw):
    """One-shot :class:`SensorLevelsPlan`: ``{key: (ncol, nsel, nsens)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    with torch.cuda.device(cols.device):
        return SensorLevelsPlan(scheme, cols, bands, levels, sensors, **kw)()


class SensorLevelsSeriesPlan(SensorLevelsPlan):
    """The outputs of :class:`SensorLevelsPlan` for ``sun.nt`` sun states of every column in one call
    (``crt_hip_sensor_levels_series_f64``): each ``(ncol, nt, nsel, nsens)`` float64, ``out[k][:, t]`` bitwise what
    :class:`SensorLevelsPlan` returns with ``psi = sun.psi[:, t]`` and the incoming spectra of step ``t``.  Reads and ignores the inputs
    :class:`LevelsSeriesPlan` does.  float64 bands only."""

    def __init__(self, scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, sensors: SensorSet, *, keys=LEVEL_KEYS, mu_s=0.501,
                 tau_d_method="quad", out=None, workspace=None, skip=None, skip_unit=1):
        self._check_options(scheme, tau_d_method)
        keys = _level_keys(keys)
        _check_skip(skip, skip_unit, getattr(cols, "ncol", None), scheme, bands)
        if not isinstance(sun, SunSeries) or isinstance(sun, SunSeriesF32):
            raise TypeError("sun must be a SunSeries (float64 spectra)")
        self._bind_sensors(scheme, cols, bands, levels, sensors, keys, mu_s, tau_d_method, out, sun=sun)
        need = sensor_series_workspace_bytes(scheme, cols.ncol, cols.nz, bands.nb, sun.nt, len(self.levels), sensors.nsens)
        self._finish("crt_hip_sensor_levels_series_f64", need, workspace)
        self._bind_skip(skip, skip_unit, "crt_hip_sensor_levels_series_masked_f64")


def solve_sensor_levels_series(scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, sensors: SensorSet, **kw):
    """One-shot :class:`SensorLevelsSeriesPlan`: ``{key: (ncol, nt, nsel, nsens)}``."""
    with torch.cuda.device(cols.device):
        return SensorLevelsSeriesPlan(scheme, cols, bands, sun, levels, sensors, **kw)()


def sensor_albedo(scheme, cols: Columns, bands: Bands, sensors: SensorSet, **kw):
    """The canopy albedo in every sensor band, ``(ncol, nsens)`` float64: the sensor-weighted upwelling over the sensor-weighted incoming
    irradiance at the canopy top, ``sum(w I_df_u) / sum(w (I_dr + I_df_d))``, from one sensor-band call at ``levels = (nz - 1,)``.  ``kw`` as
    for :class:`SensorLevelsPlan` (``keys`` is fixed here)."""
    r = solve_sensor_levels(scheme, cols, bands, (cols.nz - 1,), sensors, keys=("I_dr", "I_df_d", "I_df_u"), **kw)
    return r["I_df_u"][:, 0] / (r["I_dr"][:, 0] + r["I_df_d"][:, 0])


# ---- derivatives of the level spectra: what the Jacobian, the LAI derivative and the leaf-angle derivative share -------------------------


def _levels_deriv_workspace_bytes(query, scheme, ncol, nz, nb, nsel):
    return int(getattr(_lib.load(), query)(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nsel))


class _LevelsDerivPlan(_SolvePlan):
    """What the three derivative plans share: one construction sequence and one argument tail.  A subclass names its C entry
    (``_entry_name``), its workspace query (``_ws_query``), its output struct (``_out_struct``, a name of ``_lib``) with the keys of its
    slots (``_all_keys``), the schemes it serves (``_schemes``) and how its messages call it (``_no_kernel``, ``_what``); its own arguments
    go through ``_check_extras(**kw)`` (what needs neither a column nor a device) and ``_bind_extras(cols, **extras)``."""

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, *, keys=None, mu_s=0.501, tau_d_method="quad", out=None, workspace=None,
                 **extras):
        keys = self._check_static(scheme, tau_d_method, keys, **extras)
        if bands.dtype != torch.float64:
            raise TypeError(f"the {self._what} has no f32 storage form: bands must be float64")
        self._bind_extras(cols, **extras)
        self.levels, self.keys = normalize_levels(levels, cols.nz), keys
        self._bind(scheme, cols, bands, mu_s, tau_d_method)
        shape = (cols.ncol, len(self.levels), *self._mid, bands.nb)
        out = _outputs({k: shape for k in keys}, out, torch.float64, cols.device, "output {!r}", lacks=True)
        self.out = {k: out[k] for k in keys}
        self._out = getattr(_lib, self._out_struct)(*[out[k].data_ptr() if k in keys else None for k in self._all_keys])
        self._lev = (ctypes.c_int32 * len(self.levels))(*self.levels)
        need = _levels_deriv_workspace_bytes(self._ws_query, scheme, cols.ncol, cols.nz, bands.nb, len(self.levels))
        self._finish(self._entry_name, need, workspace)

    @classmethod
    def _check_static(cls, scheme, tau_d_method="quad", keys=None, **kw):
        """The checks that need neither a column nor a device: scheme, method, keys, the plan's own arguments.  -> keys"""
        cls._check_options(cls, scheme, tau_d_method)
        if scheme not in cls._schemes:
            raise ValueError(cls._no_kernel.format(scheme))
        keys = _level_keys(cls._all_keys if keys is None else keys, cls._all_keys)
        cls._check_extras(**kw)
        return keys

    _mid = ()  # output axes between the levels and the bands
    _check_extras = staticmethod(lambda **_: None)
    _bind_extras = staticmethod(lambda cols: None)

    def _tail(self):
        return self._lev, len(self.levels), ctypes.byref(self._out)


def _sensor_contract(sensors, cols, bands, spec, before, solve):
    """What ``sensor_jvp``, ``sensor_dlai`` and ``sensor_dleaf`` share: the SensorSet check, ``before()`` (the caller's checks that touch no
    device), ``sensors.check``, the derivative ``solve() -> {key: array}`` and the contraction ``spec`` of every array with the set's dense
    weights, in torch on the device."""
    if not isinstance(sensors, SensorSet):
        raise TypeError("sensors must be a SensorSet")
    before()
    sensors.check(bands.nb, cols.device)
    d = solve()
    w = torch.as_tensor(sensors.dense(bands.nb)).to(cols.device)
    return {k: torch.einsum(spec, v, w) for k, v in d.items()}


# ---- optical-property Jacobians of the level spectra (include/crt1d_hip_jac.h) --------------------------------------------------------

JAC_PARAMS = ("leaf_r", "leaf_t", "soil_r")  # the parameter axis of every Jacobian, in this order
JAC_KEYS = ("I_df_d", "I_df_u", "F")  # I_dr does not depend on the optics
JAC_SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")


def levels_jac_workspace_bytes(scheme, ncol, nz, nb, nsel):
    """Device workspace of a :class:`LevelsJacPlan` call: the records of :func:`workspace_bytes`, at the same offsets."""
    return _levels_deriv_workspace_bytes("crt_hip_levels_jac_workspace_bytes", scheme, ncol, nz, nb, nsel)


class LevelsJacPlan(_LevelsDerivPlan):
    """Pre-validated Jacobian of the level spectra (``crt_hip_levels_jac_f64``): ``out[k][c, r, p, b]`` is the exact derivative of
    ``X[c, levels[r], b]`` (``X`` in ``keys``, any of ``I_df_d, I_df_u, F``: what :class:`LevelsPlan` returns) with respect to parameter
    ``JAC_PARAMS[p]`` of the SAME column and band -- bands are independent, so this diagonal is the whole Jacobian.  Each array is
    ``(ncol, nsel, 3, nb)`` float64.  One K0 and one kernel; no finite differences.  Schemes: ``JAC_SCHEMES`` (``4s`` and ``zq_pa`` are a
    ValueError; n79 / zq beyond ``_lib.JAC_MAX_NZ`` levels a RuntimeError from the call).  bl has no soil and no upward stream: those slabs
    are zeros.  A column's result is bitwise the same alone or in any batch, for any subset of ``keys`` and of ``levels``."""

    _entry_name, _ws_query, _out_struct = "crt_hip_levels_jac_f64", "crt_hip_levels_jac_workspace_bytes", "CrtJacOut"
    _all_keys, _schemes, _what = JAC_KEYS, JAC_SCHEMES, "Jacobian"
    _no_kernel = "scheme {!r} has no Jacobian kernel; served: " + ", ".join(JAC_SCHEMES)
    _mid = (_lib.JAC_NPARAM,)


def solve_levels_jac(scheme, cols: Columns, bands: Bands, levels, **kw):
    """One-shot :class:`LevelsJacPlan`: ``{key: (ncol, nsel, 3, nb)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    with torch.cuda.device(cols.device):
        return LevelsJacPlan(scheme, cols, bands, levels, **kw)()


def _jvp_direction(d, name, ncol, nb, device):
    """A direction ``(ntan, nb)`` or ``(ncol, ntan, nb)`` (``None``: zeros) as a float64 tensor on ``device`` that broadcasts over columns."""
    if d is None:
        return None
    d = torch.as_tensor(d, dtype=torch.float64)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3 or d.shape[2] != nb or d.shape[0] not in (1, ncol):
        raise ValueError(f"`{name}` must be (ntan, nb) or (ncol, ntan, nb) with nb = {nb}, ncol = {ncol}")
    return d.to(device)


def sensor_jvp(scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, d_leaf_r, d_leaf_t, d_soil_r, **kw):
    """The derivative of :class:`SensorLevelsPlan`'s sums along ``ntan`` directions of a leaf or soil model's parameter space: per key
    ``(ncol, nsel, nsens, ntan)`` with ``out[c, r, s, k] = sum_b w_s[b] * sum_p J_p[c, r, b] * d_p[c, k, b]``.  ``d_leaf_r``, ``d_leaf_t``,
    ``d_soil_r``: ``(ntan, nb)`` (the same directions for every column) or ``(ncol, ntan, nb)``, the derivatives of the three spectra with
    respect to the model's parameters; ``None`` stands for zeros.  The Jacobian ``J`` comes from one :class:`LevelsJacPlan` call
    (``kw`` goes there); the contraction runs in torch on the device."""
    dirs = {}  # parameter index -> direction

    def check_directions():
        for p, (n, d) in enumerate(zip(JAC_PARAMS, (d_leaf_r, d_leaf_t, d_soil_r))):
            if (d := _jvp_direction(d, "d_" + n, cols.ncol, bands.nb, cols.device)) is not None:
                dirs[p] = d
        if not dirs:
            raise ValueError("at least one direction must be given")
        if len({d.shape[1] for d in dirs.values()}) != 1:
            raise ValueError("the directions must share ntan")

    def tangents():
        out = {}
        for k, J in solve_levels_jac(scheme, cols, bands, levels, **kw).items():
            for p, d in dirs.items():
                term = J[:, :, p, None, :] * d[:, None, :, :]  # (ncol, nsel, ntan, nb)
                out[k] = out[k] + term if k in out else term
        return out

    return _sensor_contract(sensors, cols, bands, "crkb,sb->crsk", check_directions, tangents)


# ---- LAI derivative of the level spectra (include/crt1d_hip_dlai.h) --------------------------------------------------------------------

DLAI_KEYS = LEVEL_KEYS  # every level quantity depends on the LAI, I_dr included
DLAI_SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")
DLAI_PER = ("log", "lai")


def _dlai_per(per):
    if per not in DLAI_PER:
        raise ValueError(f"per must be 'log' (dX / d ln LAI) or 'lai' (dX / d LAI), got {per!r}")
    return per


def levels_dlai_workspace_bytes(scheme, ncol, nz, nb, nsel):
    """Device workspace of a :class:`LevelsDlaiPlan` call: the records of :func:`workspace_bytes` at the same offsets, then the side
    records (the tangents of the record entries; bl, n79, zq)."""
    return _levels_deriv_workspace_bytes("crt_hip_levels_dlai_workspace_bytes", scheme, ncol, nz, nb, nsel)


class LevelsDlaiPlan(_LevelsDerivPlan):
    """Pre-validated derivative of the level spectra with respect to the leaf area index (``crt_hip_levels_dlai_f64``).  Every column's
    cumulative LAI profile is scaled as ``lai(s) = s * lai`` (the vertical distribution stays fixed); ``out[k][c, r, b]`` is the exact
    derivative of ``X[c, levels[r], b]`` (``X`` in ``keys``, any of ``I_dr, I_df_d, I_df_u, F``: what :class:`LevelsPlan` returns) at
    ``s = 1``, each ``(ncol, nsel, nb)`` float64.  ``per="log"``: ``dX / ds = dX / d ln(LAI)``; ``per="lai"``: divided by the column's total
    LAI ``lai[c, 0]`` on the device, ``dX / dLAI``.  One column precompute and one kernel; no finite differences.  Schemes:
    ``DLAI_SCHEMES`` (``4s`` and ``zq_pa`` are a ValueError; n79 / zq beyond ``_lib.DLAI_MAX_NZ`` levels a RuntimeError from the call).
    ``FLAG_SKIP_PRECOMPUTE`` is valid only on a workspace a call of this plan's entry has filled (the side records).  A column's result
    is bitwise the same alone or in any batch, for any subset of ``keys`` and of ``levels``."""

    _entry_name, _ws_query, _out_struct = "crt_hip_levels_dlai_f64", "crt_hip_levels_dlai_workspace_bytes", "CrtDlaiOut"
    _all_keys, _schemes, _what = DLAI_KEYS, DLAI_SCHEMES, "LAI derivative"
    _no_kernel = "scheme {!r} has no LAI-derivative kernel; served: " + ", ".join(DLAI_SCHEMES)

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, *, keys=DLAI_KEYS, per="log", mu_s=0.501, tau_d_method="quad",
                 out=None, workspace=None):
        super().__init__(scheme, cols, bands, levels, keys=keys, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace, per=per)

    @staticmethod
    def _check_extras(per="log", **_):
        _dlai_per(per)

    def _bind_extras(self, cols, per):
        self.per = per
        self._lai_total = cols.lai[:, 0].contiguous()[:, None, None] if per == "lai" else None

    def __call__(self, stream=None, *, flags=0):
        out = super().__call__(stream, flags=flags)
        if self._lai_total is not None and not flags & _lib.FLAG_PRECOMPUTE_ONLY:
            s = torch.cuda.current_stream(self.cols.device) if stream is None else stream
            with torch.cuda.stream(s):
                for v in out.values():
                    v.div_(self._lai_total)
        return out


def solve_levels_dlai(scheme, cols: Columns, bands: Bands, levels, **kw):
    """One-shot :class:`LevelsDlaiPlan`: ``{key: (ncol, nsel, nb)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    LevelsDlaiPlan._check_static(scheme, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return LevelsDlaiPlan(scheme, cols, bands, levels, **kw)()


def sensor_dlai(scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, **kw):
    """The LAI derivative of :class:`SensorLevelsPlan`'s sums: per key ``(ncol, nsel, nsens)`` with
    ``out[c, r, s] = sum_b w_s[b] * dX[c, r, b]``.  ``dX`` comes from one :class:`LevelsDlaiPlan` call (``kw`` goes there, ``per``
    included); the contraction with the sensor set's dense weights runs in torch on the device, as in :func:`sensor_jvp`."""
    return _sensor_contract(sensors, cols, bands, "crb,sb->crs", lambda: LevelsDlaiPlan._check_static(scheme, **kw),
                            lambda: solve_levels_dlai(scheme, cols, bands, levels, **kw))


# ---- leaf-angle derivative of the level spectra (include/crt1d_hip_dleaf.h) -------------------------------------------------------------

DLEAF_KEYS = LEVEL_KEYS
DLEAF_SCHEMES = DLAI_SCHEMES
LEAF_WRT = ("param", "mla", "a", "b")


@dataclass
class LeafTangent:
    """A leaf-angle direction of every column (``crt_leaf_tangent``): the tangent of G at ``_lib.quad_nodes()`` and at the sun angle, and
    of the mean leaf angle in degrees (2s reads it; ``None``: zeros)."""

    dg_table: torch.Tensor  # (ncol, NQ)
    dg_at_psi: torch.Tensor  # (ncol,)
    dmla: Optional[torch.Tensor] = None  # (ncol,) degrees

    def __post_init__(self):
        self.dg_table = _f64(self.dg_table, "dg_table")
        self.dg_at_psi = _f64(self.dg_at_psi, "dg_at_psi")
        if self.dg_table.ndim != 2 or self.dg_table.shape[1] != _lib.NQ or self.dg_at_psi.shape != (self.dg_table.shape[0],):
            raise ValueError(f"dg_table must be (ncol, {_lib.NQ}) and dg_at_psi (ncol,)")
        if self.dmla is not None:
            self.dmla = _f64(self.dmla, "dmla")
            if self.dmla.shape != self.dg_at_psi.shape:
                raise ValueError("dmla must be (ncol,)")

    def slice(self, lo, hi):
        return LeafTangent(self.dg_table[lo:hi], self.dg_at_psi[lo:hi], None if self.dmla is None else self.dmla[lo:hi])

    def c_struct(self):
        return _lib.CrtLeafTangent(self.dg_table.data_ptr(), self.dg_at_psi.data_ptr(), None if self.dmla is None else self.dmla.data_ptr())


def g_dparam(cols: Columns):
    """``dG / d g_param`` of every column in one launch (``crt_hip_g_dparam_f64``): ``(dg_table (ncol, NQ), dg_at_psi (ncol,))`` at
    ``_lib.quad_nodes(0.501)`` and at ``cols.psi``; zeros for the parameterless kinds and for ``G_TABLE`` columns."""
    dev = cols.device
    dg_table = torch.empty((cols.ncol, _lib.NQ), dtype=torch.float64, device=dev)
    dg_at_psi = torch.empty((cols.ncol,), dtype=torch.float64, device=dev)
    c = cols.c_struct()
    with torch.cuda.device(dev):
        st = _lib.load().crt_hip_g_dparam_f64(ctypes.byref(c), dg_table.data_ptr(), dg_at_psi.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "crt_hip_g_dparam_f64")
    return dg_table, dg_at_psi


def leaf_tangent(cols: Columns, wrt="param"):
    """The :class:`LeafTangent` of a unit step of one leaf-angle parameter of every column.

    ``"param"``: ``g_param`` (the ellipsoidal ``x``, Bonan's ``chi_l``) by :func:`g_dparam`, ``dmla = 0``.
    ``"mla"``: the mean leaf angle in degrees of ellipsoidal columns whose ``x`` is tied to it by ``leaf_angle.mla_to_x_approx``:
    :func:`g_dparam` times ``dx / dmla = -(x + 3) / (1.65 mla)``, with ``dmla = 1``.
    ``"a"``, ``"b"``: the coefficients of ``LeafPDF.trig(a, b)`` columns.  G and the mean leaf angle are linear in the PDF, so the
    tangent is the difference of two :func:`leaf_pdf_tables` results (``trig(1, 0)`` resp. ``trig(0, 1)`` against ``trig(0, 0)``), exact to
    rounding and the same for every ``(a, b)``."""
    if wrt not in LEAF_WRT:
        raise ValueError(f"wrt must be one of {LEAF_WRT}, got {wrt!r}")
    if wrt in ("a", "b"):
        from .leaf_angle import PDF_TRIG

        kind = torch.full((cols.ncol,), PDF_TRIG, dtype=torch.int32, device=cols.device)
        step = torch.zeros((cols.ncol, 2), dtype=torch.float64, device=cols.device)
        t0, p0, m0 = leaf_pdf_tables(kind, step, psi=cols.psi)
        step[:, 0 if wrt == "a" else 1] = 1.0
        t1, p1, m1 = leaf_pdf_tables(kind, step, psi=cols.psi)
        return LeafTangent(t1 - t0, p1 - p0, m1 - m0)
    dg_table, dg_at_psi = g_dparam(cols)
    if wrt == "param":
        return LeafTangent(dg_table, dg_at_psi)
    if cols.mla is None:
        raise ValueError("wrt='mla' needs cols.mla")
    dx = -(cols.g_param + 3.0) / (1.65 * cols.mla)
    return LeafTangent(dg_table * dx[:, None], dg_at_psi * dx, torch.ones_like(cols.mla))


def levels_dleaf_workspace_bytes(scheme, ncol, nz, nb, nsel):
    """Device workspace of a :class:`LevelsDleafPlan` call: the records of :func:`workspace_bytes` at the same offsets, then a side
    record per column (the tangents of the record entries)."""
    return _levels_deriv_workspace_bytes("crt_hip_levels_dleaf_workspace_bytes", scheme, ncol, nz, nb, nsel)


class LevelsDleafPlan(_LevelsDerivPlan):
    """Pre-validated derivative of the level spectra along a leaf-angle direction (``crt_hip_levels_dleaf_f64``): ``out[k][c, r, b]`` is
    the exact derivative of ``X[c, levels[r], b]`` (``X`` in ``keys``, any of ``I_dr, I_df_d, I_df_u, F``: what :class:`LevelsPlan`
    returns) along ``tangent`` (:class:`LeafTangent`, e.g. from :func:`leaf_tangent`), each ``(ncol, nsel, nb)`` float64; the sun angle,
    the LAI and the optics are fixed.  One column precompute, one side precompute and one kernel; no finite differences.  Schemes:
    ``DLEAF_SCHEMES`` (``4s`` and ``zq_pa`` are a ValueError; n79 / zq beyond ``_lib.DLAI_MAX_NZ`` levels a RuntimeError from the call).
    ``FLAG_SKIP_PRECOMPUTE`` is valid only on a workspace a call of this plan has filled.  A column's result is bitwise the same alone
    or in any batch, for any subset of ``keys`` and of ``levels``."""

    _entry_name, _ws_query, _out_struct = "crt_hip_levels_dleaf_f64", "crt_hip_levels_dleaf_workspace_bytes", "CrtDlaiOut"
    _all_keys, _schemes, _what = DLEAF_KEYS, DLEAF_SCHEMES, "leaf-angle derivative"
    _no_kernel = "scheme {!r} has no leaf-angle-derivative kernel; served: " + ", ".join(DLEAF_SCHEMES)

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, tangent: LeafTangent, *, keys=DLEAF_KEYS, mu_s=0.501,
                 tau_d_method="quad", out=None, workspace=None):
        super().__init__(scheme, cols, bands, levels, keys=keys, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace,
                         tangent=tangent)

    @staticmethod
    def _check_extras(**kw):  # (the one-shot functions check ahead without the tangent)
        if "tangent" in kw and not isinstance(kw["tangent"], LeafTangent):
            raise TypeError("tangent must be a LeafTangent")

    def _bind_extras(self, cols, tangent):
        if tangent.dg_table.shape[0] != cols.ncol or tangent.dg_table.device != cols.device:
            raise ValueError("the tangent must have the columns' ncol and device")
        self.tangent, self._tan = tangent, tangent.c_struct()

    def _tail(self):
        return self._lev, len(self.levels), ctypes.byref(self._tan), ctypes.byref(self._out)


def solve_levels_dleaf(scheme, cols: Columns, bands: Bands, levels, tangent: LeafTangent, **kw):
    """One-shot :class:`LevelsDleafPlan`: ``{key: (ncol, nsel, nb)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    LevelsDleafPlan._check_static(scheme, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return LevelsDleafPlan(scheme, cols, bands, levels, tangent, **kw)()


def sensor_dleaf(scheme, cols: Columns, bands: Bands, levels, tangent: LeafTangent, sensors: SensorSet, **kw):
    """The leaf-angle derivative of :class:`SensorLevelsPlan`'s sums: per key ``(ncol, nsel, nsens)`` with
    ``out[c, r, s] = sum_b w_s[b] * dX[c, r, b]``.  ``dX`` comes from one :class:`LevelsDleafPlan` call (``kw`` goes there); the
    contraction with the sensor set's dense weights runs in torch on the device, as in :func:`sensor_dlai`."""
    return _sensor_contract(sensors, cols, bands, "crb,sb->crs", lambda: LevelsDleafPlan._check_static(scheme, **kw),
                            lambda: solve_levels_dleaf(scheme, cols, bands, levels, tangent, **kw))


# ---- gradient of a weighted sum of the level spectra (include/crt1d_hip_grad.h) -----------------------------------------------------------

GRAD_SCHEMES = ("2s", "bl", "g77", "bf")  # the schemes k_grad serves; LevelsGradPlan composes the three plans above for n79 and zq
GRAD_WRT = JAC_PARAMS + ("lai", "leaf")


def levels_grad_workspace_bytes(scheme, ncol, nz, nb, nsel):
    """Device workspace of a :class:`LevelsGradPlan` call of a scheme of ``GRAD_SCHEMES``: the records of :func:`workspace_bytes` at the
    same offsets, the side records of the LAI and of the leaf-angle derivative, and the slice sums of ``lai`` and ``leaf``."""
    return _levels_deriv_workspace_bytes("crt_hip_levels_grad_workspace_bytes", scheme, ncol, nz, nb, nsel)


def _grad_weights(weights, shape=None, device=None):
    """The weights of :class:`LevelsGradPlan` as ``{key: tensor}`` in the order of ``LEVEL_KEYS``; with ``shape``: each checked as a
    caller-supplied array the kernel reads through a bare pointer."""
    if not isinstance(weights, dict) or not weights or any(k not in LEVEL_KEYS for k in weights):
        raise ValueError(f"weights must be a dict of (ncol, nsel, nb) tensors under keys out of {LEVEL_KEYS}")
    if shape is None:
        return weights
    return {k: _check_profile(weights[k], f"weights[{k!r}]", shape, device) for k in LEVEL_KEYS if k in weights}


class LevelsGradPlan(_LevelsDerivPlan):
    """Pre-validated gradient of the scalar ``sum_X sum(weights[X] * X)`` of the level spectra ``X[c, levels[r], b]`` (what
    :class:`LevelsPlan` returns; ``weights``: ``{key: (ncol, nsel, nb)}`` float64, any of ``I_dr, I_df_d, I_df_u, F`` -- in a retrieval
    ``d loss / d X``) with respect to ``wrt``, any of ``GRAD_WRT``:

    ``leaf_r``, ``leaf_t``, ``soil_r``  ``(ncol, nb)``: band by band, each row a column's own response (shared ``(nb,)`` spectra: their
    gradient is the sum over the rows); ``lai``  ``(ncol,)``: per ``ln LAI`` at a fixed leaf-area profile (``per="lai"``: per LAI), the
    convention of :class:`LevelsDlaiPlan`; ``leaf``  ``(ncol,)``: along ``tangent`` (a :class:`LeafTangent`; ``None``:
    ``leaf_tangent(cols, "param")``).

    It is the contraction of what :class:`LevelsJacPlan`, :class:`LevelsDlaiPlan` and :class:`LevelsDleafPlan` return with the weights.
    For ``GRAD_SCHEMES`` one column precompute and ONE kernel form it (``crt_hip_levels_grad_f64``) from the same tangent bits without
    writing a derivative array; for n79 and zq the plan runs those three plans and contracts in torch: the same result dict.  ``4s`` and
    ``zq_pa`` are a ValueError.  The weights are read at every call: update them in place.  There is no gradient with respect to
    ``I_dr0`` / ``I_df0`` (the spectra are linear in them).  A column's result is bitwise the same alone or in any batch and for any
    subset of ``wrt``."""

    _entry_name, _ws_query, _out_struct = "crt_hip_levels_grad_f64", "crt_hip_levels_grad_workspace_bytes", "CrtGradOut"
    _all_keys, _schemes, _what = GRAD_WRT, DLAI_SCHEMES, "gradient"
    _no_kernel = "scheme {!r} has no gradient; served: " + ", ".join(DLAI_SCHEMES)

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, weights, *, wrt=GRAD_WRT, tangent=None, per="log", mu_s=0.501,
                 tau_d_method="quad", out=None, workspace=None):
        wrt = self._check_static(scheme, tau_d_method, wrt, weights=weights, tangent=tangent, per=per)
        if bands.dtype != torch.float64:
            raise TypeError(f"the {self._what} has no f32 storage form: bands must be float64")
        self.levels, self.keys, self.per = normalize_levels(levels, cols.nz), wrt, per
        self._kw = dict(mu_s=mu_s, tau_d_method=tau_d_method)
        self._bind(scheme, cols, bands, mu_s, tau_d_method)
        ncol, nsel, nb, dev = cols.ncol, len(self.levels), bands.nb, cols.device
        self.weights = _grad_weights(weights, (ncol, nsel, nb), dev)
        if "leaf" in wrt:
            tangent = leaf_tangent(cols, "param") if tangent is None else tangent
            if tangent.dg_table.shape[0] != ncol or tangent.dg_table.device != dev:
                raise ValueError("the tangent must have the columns' ncol and device")
        self.tangent = tangent if "leaf" in wrt else None
        out = _outputs({k: (ncol, nb) if k in JAC_PARAMS else (ncol,) for k in wrt}, out, torch.float64, dev, "output {!r}", lacks=True)
        self.out = {k: out[k] for k in wrt}
        self._lai_total = cols.lai[:, 0].contiguous() if per == "lai" and "lai" in wrt else None
        self._lev = (ctypes.c_int32 * nsel)(*self.levels)
        self._composed = scheme not in GRAD_SCHEMES
        if self._composed:
            self._compose(workspace)
            return
        self._w = _lib.CrtGradWeights(*[self.weights[k].data_ptr() if k in self.weights else None for k in LEVEL_KEYS])
        self._tan = None if self.tangent is None else self.tangent.c_struct()
        self._out = _lib.CrtGradOut(*[out[k].data_ptr() if k in wrt else None for k in GRAD_WRT])
        self._finish(self._entry_name, levels_grad_workspace_bytes(scheme, ncol, cols.nz, nb, nsel), workspace)

    @staticmethod
    def _check_extras(weights=None, tangent=None, per="log", **_):
        _grad_weights(weights)
        _dlai_per(per)
        if tangent is not None and not isinstance(tangent, LeafTangent):
            raise TypeError("tangent must be a LeafTangent")

    def _tail(self):
        return (self._lev, len(self.levels), ctypes.byref(self._w), None if self._tan is None else ctypes.byref(self._tan),
                ctypes.byref(self._out))

    def _compose(self, workspace):
        """n79, zq: the plans whose outputs the call contracts (only those ``wrt`` and the weights need)."""
        if workspace is not None:
            raise ValueError(f"the gradient of {self.scheme} runs three plans with workspaces of their own: workspace must be None")
        kw = self._kw
        a = (self.scheme, self.cols, self.bands, self.levels)
        jk = tuple(k for k in JAC_KEYS if k in self.weights)
        lk = tuple(self.weights)
        self._plans = {}
        if jk and any(k in JAC_PARAMS for k in self.keys):
            self._plans["jac"] = LevelsJacPlan(*a, keys=jk, **kw)
        if "lai" in self.keys:
            self._plans["lai"] = LevelsDlaiPlan(*a, keys=lk, **kw)
        if "leaf" in self.keys:
            self._plans["leaf"] = LevelsDleafPlan(*a, self.tangent, keys=lk, **kw)

    def last_kernel(self):
        """n79, zq: the reports of the plans of this plan's most recent call, joined by `` | ``."""
        return self._report if self._composed else super().last_kernel()

    def __call__(self, stream=None, *, flags=0):
        s = torch.cuda.current_stream(self.cols.device) if stream is None else stream
        if not self._composed:
            out = super().__call__(stream, flags=flags)
        else:
            out = self.out
            d, reports = {}, []
            for n, p in self._plans.items():
                d[n] = p(stream, flags=flags)
                reports.append(p.last_kernel())
            self._report = " | ".join(reports)
            if not flags & _lib.FLAG_PRECOMPUTE_ONLY:
                with torch.cuda.stream(s):
                    for k in self.keys:
                        if k in JAC_PARAMS:
                            out[k].zero_()
                            for x, J in d.get("jac", {}).items():
                                out[k] += (self.weights[x] * J[:, :, JAC_PARAMS.index(k), :]).sum(1)
                        else:
                            out[k].zero_()
                            for x, D in d[k].items():
                                out[k] += (self.weights[x] * D).sum((1, 2))
        if self._lai_total is not None and not flags & _lib.FLAG_PRECOMPUTE_ONLY:
            with torch.cuda.stream(s):
                out["lai"].div_(self._lai_total)
        return out


def solve_levels_grad(scheme, cols: Columns, bands: Bands, levels, weights, **kw):
    """One-shot :class:`LevelsGradPlan`: ``{name: (ncol, nb) | (ncol,)}`` for the names ``wrt``."""
    LevelsGradPlan._check_static(scheme, kw.get("tau_d_method", "quad"), kw.get("wrt", GRAD_WRT), weights=weights,
                                 tangent=kw.get("tangent"), per=kw.get("per", "log"))  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return LevelsGradPlan(scheme, cols, bands, levels, weights, **kw)()


# ---- what the inverse-problem plans share: the parameter axis and the checks that need no device (the retrieval core: _LmPlan) ----------


def _need_sun_series(sun):
    if not isinstance(sun, SunSeries) or isinstance(sun, SunSeriesF32):
        raise TypeError("sun must be a SunSeries (float64 spectra)")


def _need_f64_bands(bands, what):
    if bands is not None and bands.dtype != torch.float64:  # (None: a check ahead of the columns)
        raise TypeError(f"the {what} has no f32 storage form: bands must be float64")


def _check_tangent(tangent, sun=None, series=False):
    """``tangent``: None or a :class:`LeafTangent`; ``series``: ``sun`` a float64 :class:`SunSeries`, ``tangent`` a :class:`LeafTangentSeries`
    of its ``nt``."""
    if series:
        _need_sun_series(sun)
    kind = LeafTangentSeries if series else LeafTangent
    if tangent is not None and not isinstance(tangent, kind):
        raise TypeError(f"tangent must be a {kind.__name__}")
    if series and tangent is not None and tangent.nt != sun.nt:
        raise ValueError(f"the tangent has nt = {tangent.nt} sun states, the series {sun.nt}")


def _check_obs(y, inv_sigma, keys, axes, rank=None):
    """The observation dicts of a retrieval against ``keys``; ``axes``: how the messages call the arrays' shape.  ``rank``: their number of
    axes, where the shapes can be looked at already (the spectral plans: arrays of the user's) -- they must share one shape then."""
    import numpy as np

    shapes = set()
    for name, d in (("y", y), ("inv_sigma", inv_sigma)):
        if d is None and name == "inv_sigma":
            continue
        if not isinstance(d, dict):
            raise TypeError(f"{name} must be a dict {{key: {axes}}}")
        if extra := [k for k in d if k not in keys]:
            raise ValueError(f"{name} has the keys {extra}, which are not in keys = {keys}")
        for k, v in d.items() if rank else ():
            shape = tuple(v.shape) if hasattr(v, "shape") else np.shape(v)
            if len(shape) != rank:
                raise ValueError(f"{name}[{k!r}] must be {axes}, got {shape}")
            shapes.add(shape)
    if missing := [k for k in keys if k not in y]:
        raise ValueError(f"y lacks the keys {missing} of keys = {keys}")
    if len(shapes) > 1:
        raise ValueError(f"the arrays of y and inv_sigma must share one shape {axes}, got {sorted(shapes)}")


def _per_col(v, name, ncol, npar, device):
    """``(ncol, npar)`` or ``(npar,)`` -> a contiguous float64 ``(ncol, npar)`` on ``device``."""
    v = torch.as_tensor(v, dtype=torch.float64).to(device)
    if v.ndim == 1:
        v = v[None]
    if v.ndim != 2 or v.shape[1] != npar or v.shape[0] not in (1, ncol):
        raise ValueError(f"{name} must be (ncol, npar) or (npar,) with ncol = {ncol}, npar = {npar}")
    return v.expand(ncol, -1).contiguous()


class _ParamAxis:
    """The parameter axis of the inverse-problem plans: the ``ntan`` directions ``d_leaf_r / d_leaf_t / d_soil_r`` (``"dir0"``, ...; with a
    ``leaf_model``: its ``nm`` parameters by name, then the ``ns`` soil directions), then ``"lai"``, then ``"leaf"`` (``leaf=True`` or a
    ``tangent``).  The constructor is the static half: nothing but the user's arguments -> ``ntan``, ``npar``, ``params``.  :meth:`bind`
    is the bound half: the direction tensors, the tangent, and the C structs the entries and ``k_retrieve_apply`` read."""

    def __init__(self, d_leaf_r=None, d_leaf_t=None, d_soil_r=None, lai=True, leaf=False, leaf_model=None, tangent=None):
        self.given = {n: d for n, d in zip(JAC_PARAMS, (d_leaf_r, d_leaf_t, d_soil_r)) if d is not None}
        if leaf_model is None:
            self.ntan, names = _sensjac_ntan(d_leaf_r, d_leaf_t, d_soil_r), ()
        else:
            self.ntan, names = _leaf_model_ntan(leaf_model, d_leaf_r, d_leaf_t, d_soil_r), leaf_model.params
        self.lai, self.leaf, self.tangent = bool(lai), bool(leaf) or tangent is not None, tangent
        self.params = (names + tuple(f"dir{k}" for k in range(self.ntan - len(names))) + (("lai",) if self.lai else ())
                       + (("leaf",) if self.leaf else ()))
        self.npar = len(self.params)
        if self.npar == 0:
            raise ValueError("no parameter at all: give a direction, lai=True or a leaf-angle parameter (leaf=True, a tangent)")

    def bind(self, ncol, nb, device):
        """-> self, with ``dirs`` (the directions given, contiguous float64 on ``device``, per column where one of them is), the tangent
        checked against the columns, and ``c_dirs`` / ``c_tan``, the ``CrtOpticsDirs`` and the tangent's C struct (None where there is
        none).  The axis keeps every tensor whose address they hold.  (Not for an axis with a ``leaf_model``: :class:`_PlateLeafBinding`.)"""
        dirs = {n: _jvp_direction(d, "d_" + n, ncol, nb, device) for n, d in self.given.items()}
        per_col = any(d.shape[0] != 1 for d in dirs.values()) and ncol != 1
        self.dirs = {n: (d.expand(ncol, -1, -1) if per_col else d).contiguous() for n, d in dirs.items()}
        t = self.tangent
        if t is not None and (t.dg_table.shape[0] != ncol or t.dg_table.device != device):
            raise ValueError("the tangent must have the columns' ncol and device")
        self.c_dirs = None
        if self.ntan:
            self.c_dirs = _lib.CrtOpticsDirs(self.ntan, self.ntan * nb if per_col else 0,
                                             *[self.dirs[n].data_ptr() if n in self.dirs else None for n in JAC_PARAMS])
        self.c_tan = None if t is None else t.c_struct()
        return self


# ---- Jacobian of the sensor-band sums (include/crt1d_hip_sensjac.h) -----------------------------------------------------------------------

SENSJAC_SCHEMES = GRAD_SCHEMES  # the schemes k_sens_jac serves; SensorJacPlan composes sensor_jvp, sensor_dlai and sensor_dleaf for n79 and zq


def sensor_jac_workspace_bytes(scheme, ncol, nz, nb, nsel, nsens, npar):
    """Device workspace of a :class:`SensorJacPlan` call of a scheme of ``SENSJAC_SCHEMES``: the records of :func:`workspace_bytes` at the
    same offsets, the side records of the LAI and of the leaf-angle derivative, and the slice partial sums."""
    return int(_lib.load().crt_hip_sensor_jac_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nsel, nsens, npar))


def _sensjac_ntan(d_leaf_r=None, d_leaf_t=None, d_soil_r=None):
    """``ntan`` of the directions of a :class:`SensorJacPlan` from their shapes alone (no device): 0 with none given."""
    import numpy as np

    ntan = set()
    for n, d in zip(JAC_PARAMS, (d_leaf_r, d_leaf_t, d_soil_r)):
        if d is None:
            continue
        shape = tuple(d.shape) if hasattr(d, "shape") else np.shape(d)
        if len(shape) not in (2, 3):
            raise ValueError(f"`d_{n}` must be (ntan, nb) or (ncol, ntan, nb)")
        ntan.add(int(shape[-2]))
    if len(ntan) > 1:
        raise ValueError("the directions must share ntan")
    ntan = ntan.pop() if ntan else 0
    if not 0 <= ntan <= _lib.SENSJAC_MAX_NTAN:
        raise ValueError(f"ntan = {ntan}; one call takes 1 .. {_lib.SENSJAC_MAX_NTAN} directions")
    return ntan


class SensorJacPlan(_LevelsDerivPlan):
    """Pre-validated Jacobian of the sums of :class:`SensorLevelsPlan` with respect to a parameter vector of every column
    (``crt_hip_sensor_jac_f64``): ``out[k][c, r, s, j]`` is the derivative of ``sum_b w_s[b] * X[c, levels[r], b]`` (``X`` in ``keys``, any
    of ``I_dr, I_df_d, I_df_u, F``) with respect to parameter ``params[j]``, each ``(ncol, nsel, nsens, npar)`` float64.  The parameters, in
    this order: ``ntan`` directions of a leaf or soil model, given as in :func:`sensor_jvp` (``d_leaf_r``, ``d_leaf_t``, ``d_soil_r``:
    ``(ntan, nb)`` or ``(ncol, ntan, nb)``, ``None`` = zeros; ``"dir0"``, ``"dir1"``, ...); ``"lai"`` (``lai=True``): per ``ln LAI`` at a
    fixed leaf-area profile, the convention of :class:`LevelsDlaiPlan`; ``"leaf"``: along ``tangent`` (a :class:`LeafTangent`; ``None``:
    no such column).

    It is what :func:`sensor_jvp`, :func:`sensor_dlai` and :func:`sensor_dleaf` return, side by side.  For ``SENSJAC_SCHEMES`` one column
    precompute and ONE kernel form it from the same tangent bits without writing a derivative array; for n79 and zq the plan calls those
    three functions: the same result dict.  ``4s`` and ``zq_pa`` are a ValueError.  The directions are read at every call: update them
    in place.  ``I_dr`` does not depend on the optics (zeros in its direction columns); bl has no soil and no upward stream.  The
    workspace also holds what a :class:`SensorLevelsPlan` of the same shape needs: that plan, called on ``plan.workspace`` with
    ``FLAG_SKIP_PRECOMPUTE`` after this one, gives the forward sums without a second column precompute.  A column's result is bitwise
    the same alone or in any batch, for any subset of ``keys``, and a parameter column's bits do not depend on which others exist.

    ``skip=``: an int32 tensor ``(ncol // skip_unit,)`` on the columns' device, read on the device at every call
    (``crt_hip_sensor_jac_masked_f64``): column ``c`` is left alone -- its outputs and its slice sums in the workspace keep their bits --
    iff ``skip[c // skip_unit] != 0``; an evaluated column has the bits of the plan without ``skip``.  The column precompute runs on
    every column.  ``plan.use_skip = False`` makes the next calls evaluate everything.  Not with the composed n79 / zq plans.
    :class:`SensorLevelsPlan`, :class:`SpectralNormalPlan` and the three series plans take the same two keywords."""

    _entry_name, _ws_query, _out_struct = "crt_hip_sensor_jac_f64", "crt_hip_sensor_jac_workspace_bytes", "CrtSensJacOut"
    _all_keys, _schemes, _what = LEVEL_KEYS, DLAI_SCHEMES, "sensor Jacobian"
    _no_kernel = "scheme {!r} has no sensor Jacobian; served: " + ", ".join(DLAI_SCHEMES)

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, *, d_leaf_r=None, d_leaf_t=None, d_soil_r=None,
                 lai=True, tangent=None, keys=LEVEL_KEYS, mu_s=0.501, tau_d_method="quad", out=None, workspace=None, skip=None, skip_unit=1):
        self._build(None, scheme, cols, bands, levels, sensors, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t, d_soil_r=d_soil_r, lai=lai, tangent=tangent,
                    keys=keys, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace, skip=skip, skip_unit=skip_unit)

    _entry_masked_name = "crt_hip_sensor_jac_masked_f64"
    _series = False  # SensorJacSeriesPlan: a sun-angle series in front of the levels, outputs with a sun-state axis

    @classmethod
    def _static(cls, scheme, cols, bands, levels, sensors, **kw):
        """The constructor's arguments (``kw``: its keywords) -> (keys, the parameter axis): every check that needs neither a column nor
        a device."""
        return cls._static_of(None, scheme, bands, sensors, **kw)

    @classmethod
    def _static_of(cls, sun, scheme, bands, sensors, *, d_leaf_r=None, d_leaf_t=None, d_soil_r=None, lai=True, tangent=None, keys=LEVEL_KEYS,
                   mu_s=0.501, tau_d_method="quad", out=None, workspace=None, skip=None, skip_unit=1, ncol=None):
        keys = cls._check_static(scheme, tau_d_method, keys, sensors=sensors, tangent=tangent, sun=sun)
        if skip is not None and scheme not in SENSJAC_SCHEMES:
            raise ValueError(f"the sensor Jacobian of {scheme} is composed of three calls: it takes no skip=")
        _check_skip(skip, skip_unit, ncol, scheme, bands)
        axis = _ParamAxis(d_leaf_r, d_leaf_t, d_soil_r, lai, tangent=tangent)
        if scheme not in SENSJAC_SCHEMES and workspace is not None:
            raise ValueError(f"the sensor Jacobian of {scheme} runs plans with workspaces of their own: workspace must be None")
        _need_f64_bands(bands, cls._what)
        return keys, axis

    @classmethod
    def _check_extras(cls, sensors=None, tangent=None, sun=None):
        if not isinstance(sensors, SensorSet):
            raise TypeError("sensors must be a SensorSet")
        _check_tangent(tangent, sun, cls._series)

    def _build(self, sun, scheme, cols, bands, levels, sensors, *, mu_s, tau_d_method, out, workspace, **kw):
        """The construction of this plan (``sun`` None) and of :class:`SensorJacSeriesPlan`."""
        skip, skip_unit = kw.get("skip"), kw.get("skip_unit", 1)
        keys, axis = self._static_of(sun, scheme, bands, sensors, tau_d_method=tau_d_method, workspace=workspace, ncol=getattr(cols, "ncol", None), **kw)
        series = {} if sun is None else {"sun": sun}
        self._composed = scheme not in SENSJAC_SCHEMES
        self.levels, self.keys, self.sensors = normalize_levels(levels, cols.nz), keys, sensors
        self._kw = dict(mu_s=mu_s, tau_d_method=tau_d_method)
        sensors.check(bands.nb, cols.device)
        self._bind(scheme, cols, bands, mu_s, tau_d_method, **series)
        ncol, nsel, nb, dev = cols.ncol, len(self.levels), bands.nb, cols.device
        nts = () if sun is None else (sun.nt,)
        self._axis = axis.bind(ncol, nb, dev)  # (the composed plans too: a retrieval takes its apply-directions from here)
        self.dirs, self.tangent, self.ntan, self.params = axis.dirs, axis.tangent, axis.ntan, axis.params
        self._dirs, self._tan = axis.c_dirs, axis.c_tan
        npar = axis.npar
        out = _outputs({k: (ncol, *nts, nsel, sensors.nsens, npar) for k in keys}, out, torch.float64, dev, "output {!r}", lacks=True)
        self.out = {k: out[k] for k in keys}
        self._lev = (ctypes.c_int32 * nsel)(*self.levels)
        if self._composed:
            self._report = ""
            return
        self._sens = sensors.c_struct()
        self._out = _lib.CrtSensJacOut(*[out[k].data_ptr() if k in keys else None for k in LEVEL_KEYS])
        if sun is None:
            need = max(sensor_jac_workspace_bytes(scheme, ncol, cols.nz, nb, nsel, sensors.nsens, npar),
                       sensor_workspace_bytes(scheme, ncol, cols.nz, nb, nsel, sensors.nsens))
        else:
            need = max(sensor_jac_series_workspace_bytes(scheme, ncol, cols.nz, nb, sun.nt, nsel, sensors.nsens, npar),
                       sensor_series_workspace_bytes(scheme, ncol, cols.nz, nb, sun.nt, nsel, sensors.nsens))
        self._finish(self._entry_name, need, workspace)
        self._bind_skip(skip, skip_unit, self._entry_masked_name)

    def _tail(self):
        ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
        return (self._lev, len(self.levels), ctypes.byref(self._sens), ref(self._dirs), int("lai" in self.params), ref(self._tan),
                ctypes.byref(self._out))

    def last_kernel(self):
        """n79, zq: the reports of the calls of this plan's most recent call, joined by `` | ``."""
        return self._report if self._composed else super().last_kernel()

    def __call__(self, stream=None, *, flags=0):
        if not self._composed:
            return super().__call__(stream, flags=flags)
        if flags:
            raise ValueError(f"the sensor Jacobian of {self.scheme} is composed of three calls: it takes no flags")
        s = torch.cuda.current_stream(self.cols.device) if stream is None else stream
        a, reports, ntan = (self.scheme, self.cols, self.bands, self.levels), [], self.ntan
        last = lambda: reports.append(self.lib.crt_hip_last_kernel().decode())  # noqa: E731
        with torch.cuda.stream(s):
            for v in self.out.values():
                v.zero_()
            jk = tuple(k for k in JAC_KEYS if k in self.keys)
            if ntan and jk:
                d = sensor_jvp(*a, self.sensors, *[self.dirs.get(n) for n in JAC_PARAMS], keys=jk, **self._kw)
                last()
                for k, v in d.items():
                    self.out[k][..., :ntan] = v
            if "lai" in self.params:
                d = sensor_dlai(*a, self.sensors, keys=self.keys, **self._kw)
                last()
                for k, v in d.items():
                    self.out[k][..., ntan] = v
            if "leaf" in self.params:
                d = sensor_dleaf(*a, self.tangent, self.sensors, keys=self.keys, **self._kw)
                last()
                for k, v in d.items():
                    self.out[k][..., len(self.params) - 1] = v
        self._report = " | ".join(reports)
        return self.out


def sensor_jacobian(scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, **kw):
    """One-shot :class:`SensorJacPlan`: ``{key: (ncol, nsel, nsens, npar)}`` at the sorted levels ``normalize_levels(levels, nz)``."""
    SensorJacPlan._static(scheme, cols, bands, levels, sensors, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return SensorJacPlan(scheme, cols, bands, levels, sensors, **kw)()


# ---- the sensor Jacobian over a sun-angle series (include/crt1d_hip_sensjac_series.h) -----------------------------------------------------


@dataclass
class LeafTangentSeries:
    """A :class:`LeafTangent` for the ``nt`` sun states of a :class:`SunSeries` (``crt_leaf_tangent_series``): ``dg_table (ncol, NQ)`` and
    ``dmla (ncol,)`` do not follow the sun; ``dg_at_psi (ncol, nt)`` is the tangent of G at ``sun.psi``."""

    dg_table: torch.Tensor  # (ncol, NQ)
    dg_at_psi: torch.Tensor  # (ncol, nt)
    dmla: Optional[torch.Tensor] = None  # (ncol,) degrees

    def __post_init__(self):
        self.dg_table = _f64(self.dg_table, "dg_table")
        self.dg_at_psi = _f64(self.dg_at_psi, "dg_at_psi")
        ncol = self.dg_table.shape[0]
        if (self.dg_table.ndim != 2 or self.dg_table.shape[1] != _lib.NQ or self.dg_at_psi.ndim != 2 or self.dg_at_psi.shape[0] != ncol
                or self.dg_at_psi.shape[1] < 1):
            raise ValueError(f"dg_table must be (ncol, {_lib.NQ}) and dg_at_psi (ncol, nt) with nt >= 1")
        if self.dmla is not None:
            self.dmla = _f64(self.dmla, "dmla")
            if self.dmla.shape != (ncol,):
                raise ValueError("dmla must be (ncol,)")

    @property
    def nt(self):
        return self.dg_at_psi.shape[1]

    def step(self, t):
        """The :class:`LeafTangent` of sun state ``t``."""
        return LeafTangent(self.dg_table, self.dg_at_psi[:, t].contiguous(), self.dmla)

    def slice(self, lo, hi):
        return LeafTangentSeries(self.dg_table[lo:hi], self.dg_at_psi[lo:hi], None if self.dmla is None else self.dmla[lo:hi])

    def c_struct(self):
        return _lib.CrtLeafTangentSeries(self.dg_table.data_ptr(), self.dg_at_psi.data_ptr(), None if self.dmla is None else self.dmla.data_ptr())


def g_dparam_series(cols: Columns, sun: SunSeries):
    """:func:`g_dparam` with the sun-angle entry at every ``sun.psi[c, t]`` (``crt_hip_g_dparam_series_f64``): ``(dg_table (ncol, NQ),
    dg_at_psi (ncol, nt))``, bitwise what :func:`g_dparam` gives for columns whose ``psi`` is ``sun.psi[:, t]``.  ``cols.psi`` is not read."""
    dev = cols.device
    if sun.ncol != cols.ncol or sun.psi.device != dev:
        raise ValueError("sun must have the columns' ncol and device")
    dg_table = torch.empty((cols.ncol, _lib.NQ), dtype=torch.float64, device=dev)
    dg_at_psi = torch.empty((cols.ncol, sun.nt), dtype=torch.float64, device=dev)
    c, sn = cols.c_struct(), sun.c_struct()
    with torch.cuda.device(dev):
        st = _lib.load().crt_hip_g_dparam_series_f64(ctypes.byref(c), ctypes.byref(sn), dg_table.data_ptr(), dg_at_psi.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "crt_hip_g_dparam_series_f64")
    return dg_table, dg_at_psi


def leaf_tangent_series(cols: Columns, sun: SunSeries, wrt="param"):
    """:func:`leaf_tangent` for every sun state of ``sun``: a :class:`LeafTangentSeries` whose ``.step(t)`` is bitwise
    ``leaf_tangent`` of columns with ``psi = sun.psi[:, t]``.  Same four ``wrt``."""
    if wrt not in LEAF_WRT:
        raise ValueError(f"wrt must be one of {LEAF_WRT}, got {wrt!r}")
    if wrt in ("a", "b"):
        from .leaf_angle import PDF_TRIG

        kind = torch.full((cols.ncol,), PDF_TRIG, dtype=torch.int32, device=cols.device)
        step = torch.zeros((cols.ncol, 2), dtype=torch.float64, device=cols.device)
        t0, p0, m0 = leaf_pdf_tables(kind, step, psi=sun.psi)
        step[:, 0 if wrt == "a" else 1] = 1.0
        t1, p1, m1 = leaf_pdf_tables(kind, step, psi=sun.psi)
        return LeafTangentSeries(t1 - t0, p1 - p0, m1 - m0)
    dg_table, dg_at_psi = g_dparam_series(cols, sun)
    if wrt == "param":
        return LeafTangentSeries(dg_table, dg_at_psi)
    if cols.mla is None:
        raise ValueError("wrt='mla' needs cols.mla")
    dx = -(cols.g_param + 3.0) / (1.65 * cols.mla)
    return LeafTangentSeries(dg_table * dx[:, None], dg_at_psi * dx[:, None], torch.ones_like(cols.mla))


def sensor_jac_series_workspace_bytes(scheme, ncol, nz, nb, nt, nsel, nsens, npar):
    """Device workspace of a :class:`SensorJacSeriesPlan` call of a scheme of ``SENSJAC_SCHEMES``: the records of
    :func:`levels_series_workspace_bytes` at the same offsets, the side records of the LAI and of the leaf-angle derivative, and the slice
    partial sums of every (column, t)."""
    return int(_lib.load().crt_hip_sensor_jac_series_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nt, nsel, nsens, npar))


class SensorJacSeriesPlan(SensorJacPlan):
    """The Jacobian of :class:`SensorJacPlan` for the ``sun.nt`` sun states of every column in one call
    (``crt_hip_sensor_jac_series_f64``): each output ``(ncol, nt, nsel, nsens, npar)`` float64, the Jacobian of the sums of
    :class:`SensorLevelsSeriesPlan` with respect to ONE parameter vector per column (``.params`` as in :class:`SensorJacPlan`).
    ``out[k][:, t]`` is bitwise what :class:`SensorJacPlan` returns with ``psi = sun.psi[:, t]`` (``g_at_psi`` likewise), the incoming
    spectra of step ``t`` and ``tangent.step(t)``; ``cols.psi``, ``cols.g_at_psi`` and ``bands.I_dr0 / I_df0`` are not read.  ``sun``: a
    float64 :class:`SunSeries`; ``tangent``: a :class:`LeafTangentSeries` of the same ``nt`` (e.g. :func:`leaf_tangent_series`) or ``None``.

    For ``SENSJAC_SCHEMES`` the canopy part of the column precompute and the side precomputes run once per column, the sun records, one
    Jacobian kernel and (several band slices) one finish kernel serve every (column, t).  The workspace also holds what a
    :class:`SensorLevelsSeriesPlan` of the same shape needs: that plan, called on ``plan.workspace`` with ``FLAG_SKIP_PRECOMPUTE`` after
    this one, gives the forward sums of the residual.  For n79 and zq the plan loops the composed path of :class:`SensorJacPlan` over ``t``
    (no workspace, no flags); ``4s`` and ``zq_pa`` are a ValueError.  For :func:`gauss_newton_step`:
    ``J.reshape(ncol, nt * nsel * nsens, npar)``."""

    _entry_name, _series = "crt_hip_sensor_jac_series_f64", True
    _entry_masked_name = "crt_hip_sensor_jac_series_masked_f64"

    def __init__(self, scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, sensors: SensorSet, *, d_leaf_r=None, d_leaf_t=None,
                 d_soil_r=None, lai=True, tangent=None, keys=LEVEL_KEYS, mu_s=0.501, tau_d_method="quad", out=None, workspace=None, skip=None,
                 skip_unit=1):
        self._build(sun, scheme, cols, bands, levels, sensors, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t, d_soil_r=d_soil_r, lai=lai, tangent=tangent,
                    keys=keys, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace, skip=skip, skip_unit=skip_unit)

    @classmethod
    def _static(cls, scheme, cols, bands, sun, levels, sensors, **kw):
        return cls._static_of(sun, scheme, bands, sensors, **kw)

    def __call__(self, stream=None, *, flags=0):
        if not self._composed:
            return _SolvePlan.__call__(self, stream, flags=flags)
        if flags:
            raise ValueError(f"the sensor Jacobian of {self.scheme} is composed of three calls per sun state: it takes no flags")
        s = torch.cuda.current_stream(self.cols.device) if stream is None else stream
        sun, reports = self.sun, []
        with torch.cuda.stream(s):
            for t in range(sun.nt):
                plan = SensorJacPlan(self.scheme, _step_columns(self.cols, sun, t), _step_bands(self.bands, sun, t), self.levels, self.sensors,
                                     **{"d_" + n: d for n, d in self.dirs.items()}, lai="lai" in self.params,
                                     tangent=None if self.tangent is None else self.tangent.step(t), keys=self.keys, **self._kw)
                for k, v in plan().items():
                    self.out[k][:, t] = v
                reports.append(plan.last_kernel())
        self._report = " | ".join(reports)
        return self.out


def _step_columns(cols, sun, t):
    """``cols`` with the sun of step ``t`` of ``sun`` (views; the sun angles as contiguous copies)."""
    return Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla,
                   None if sun.g_at_psi is None else sun.g_at_psi[:, t].contiguous(), cols.g_table)


def _step_bands(bands, sun, t):
    """``bands`` with the incoming spectra of step ``t`` of ``sun`` (shared rows expanded where only one side is per column)."""
    rows = max(sun.I_dr0.shape[0], bands.leaf_r.shape[0])
    g = lambda v: None if v is None else v.expand(rows, -1).contiguous()  # noqa: E731
    return Bands(g(sun.I_dr0[:, t]), g(sun.I_df0[:, t]), g(bands.leaf_r), g(bands.leaf_t), g(bands.soil_r))


def sensor_jacobian_series(scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, sensors: SensorSet, **kw):
    """One-shot :class:`SensorJacSeriesPlan`: ``{key: (ncol, nt, nsel, nsens, npar)}`` at the sorted levels."""
    SensorJacSeriesPlan._static(scheme, cols, bands, sun, levels, sensors, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return SensorJacSeriesPlan(scheme, cols, bands, sun, levels, sensors, **kw)()


def gauss_newton_step(J, r, *, damping=0.0):
    """One damped Gauss-Newton (Levenberg-Marquardt) step of every column: ``J`` ``(ncol, nobs, npar)``, ``r`` ``(ncol, nobs)`` ->
    ``delta`` ``(ncol, npar)``, the solution of ``(J^T J + damping * diag(J^T J)) delta = -J^T r`` (``damping``: a number, or ``(ncol,)`` for a
    damping of every column's own).  A series Jacobian ``(ncol, nt, nsel, nsens, npar)`` of :class:`SensorJacSeriesPlan` needs nothing
    more: ``J.reshape(ncol, nt * nsel * nsens, npar)``.  Plain torch on the tensors' device: the
    normal equations, scaled to a unit diagonal, are solved by a Cholesky factorisation written as ``npar`` vector steps over the
    columns (no pivoting is needed, no solver library is called).  A parameter whose Jacobian column is zero gets ``delta = 0``.  A
    convenience for a handful of parameters, not a hot path."""
    if J.ndim != 3 or r.shape != J.shape[:2]:
        raise ValueError("J must be (ncol, nobs, npar) and r (ncol, nobs)")
    lam = torch.as_tensor(damping, dtype=J.dtype, device=J.device)
    if lam.ndim > 1 or (lam.ndim == 1 and lam.shape[0] != J.shape[0]) or bool((lam < 0).any()):
        raise ValueError("damping must be a number or (ncol,), >= 0")
    A = torch.einsum("coi,coj->cij", J, J)
    g = torch.einsum("coi,co->ci", J, r)
    n = A.shape[1]
    diag = torch.diagonal(A, dim1=1, dim2=2)
    dead = diag <= 0
    sc = torch.where(dead, torch.ones_like(diag), diag).rsqrt()
    A = A * sc[:, :, None] * sc[:, None, :]
    A = A + torch.diag_embed(torch.where(dead, torch.ones_like(diag), lam.reshape(-1, 1).expand_as(diag)))
    y = -g * sc
    L = torch.zeros_like(A)
    for j in range(n):  # A = L L^T, column by column
        d = (A[:, j, j] - (L[:, j, :j] ** 2).sum(1)).sqrt()
        L[:, j, j] = d
        if j + 1 < n:
            L[:, j + 1:, j] = (A[:, j + 1:, j] - torch.einsum("cik,ck->ci", L[:, j + 1:, :j], L[:, j, :j])) / d[:, None]
    z = torch.zeros_like(y)
    for j in range(n):  # L z = y
        z[:, j] = (y[:, j] - (L[:, j, :j] * z[:, :j]).sum(1)) / L[:, j, j]
    x = torch.zeros_like(y)
    for j in reversed(range(n)):  # L^T x = z
        x[:, j] = (z[:, j] - (L[:, j + 1:, j] * x[:, j + 1:]).sum(1)) / L[:, j, j]
    return x * sc


# ---- the per-column Levenberg-Marquardt retrieval (include/crt1d_hip_retrieve.h) ---------------------------------------------------------

LM_RUNNING, LM_CONVERGED_X, LM_CONVERGED_F = _lib.LM_RUNNING, _lib.LM_CONVERGED_X, _lib.LM_CONVERGED_F
LM_STALLED, LM_FAILED_START = _lib.LM_STALLED, _lib.LM_FAILED_START
RETRIEVE_SCHEMES = DLAI_SCHEMES  # 2s, bl, g77, bf on the kernels; n79 and zq through the composed SensorJacPlan
LM_OPTIONS = dict(lam0=1e-2, lam_up=10.0, lam_down=0.1, lam_min=1e-12, lam_max=1e12, xtol=0.0, ftol=0.0)


def _lm_options(lo, hi, npar, opts):
    """The bounds and Levenberg-Marquardt options of a retrieval plan, checked without a device.  -> LM options"""
    import numpy as np

    for name, v in (("lo", lo), ("hi", hi)):
        if v is not None and tuple(np.shape(v)) != (npar,):
            raise ValueError(f"{name} must be (npar,) = ({npar},), got {tuple(np.shape(v))}")
    if unknown := [k for k in opts if k not in LM_OPTIONS]:
        raise TypeError(f"unknown options {unknown}; the Levenberg-Marquardt options are {tuple(LM_OPTIONS)}")
    o = {k: float(opts.get(k, v)) for k, v in LM_OPTIONS.items()}
    if not (o["lam0"] > 0 and o["lam_up"] > 1 and 0 < o["lam_down"] <= 1 and 0 <= o["lam_min"] <= o["lam_max"] and o["xtol"] >= 0 and o["ftol"] >= 0):
        raise ValueError("the options need lam0 > 0, lam_up > 1, 0 < lam_down <= 1, 0 <= lam_min <= lam_max, xtol >= 0 and ftol >= 0")
    return o


def _check_start(leaf_model, lo, hi, p0, prior, inv_sigma_prior):
    """The starting point and the prior of a retrieval, as far as no device is needed."""
    if leaf_model is not None:
        _leaf_model_start(leaf_model, lo, hi, p0)
    if (prior is None) != (inv_sigma_prior is None):
        raise ValueError("prior and inv_sigma_prior go together")


def pack_lower(P):
    """``(..., npar, npar)`` -> the lower triangles row by row ``(..., npar (npar + 1) / 2)``, the layout of ``crt_lm_state.A`` and of
    ``plan.prior_precision``; the upper triangle is not read."""
    i, j = torch.tril_indices(P.shape[-1], P.shape[-1])
    return P[..., i.to(P.device), j.to(P.device)].contiguous()


def unpack_lower(T, npar):
    """The inverse of :func:`pack_lower`: ``(..., ntri)`` -> the symmetric ``(..., npar, npar)``."""
    i, j = (v.to(T.device) for v in torch.tril_indices(npar, npar))
    P = T.new_zeros(T.shape[:-1] + (npar, npar))
    P[..., i, j] = T
    P[..., j, i] = T
    return P


def _check_full_prior(prior_mean, prior_precision, chain, evaluate, ncol, npar):
    """``prior_mean=`` / ``prior_precision=`` of a retrieval plan with ``ncol`` columns (or: of the :class:`Columns` ``ncol``), as far as
    no device is needed.  -> whether the plan has a full Gaussian prior"""
    import numpy as np

    if prior_mean is None and prior_precision is None:
        return False
    if prior_mean is None or prior_precision is None:
        raise ValueError("prior_mean and prior_precision go together: a full Gaussian prior needs its mean and its precision matrix")
    if chain is not None:
        raise ValueError("prior_precision cannot be combined with chain=: the chained step takes no full prior block (a date-by-date "
                         "series with a full prior is a SequentialPlan)")
    if evaluate == "accepted":
        raise ValueError("prior_precision cannot be combined with evaluate='accepted': the decision kernel (k_lm_decide) takes no block of "
                         "sums, so its cost would lack the prior; use evaluate='running'")
    ncol = ncol if isinstance(ncol, int) else ncol.ncol
    shape = lambda v: tuple(v.shape) if hasattr(v, "shape") else np.shape(v)  # noqa: E731
    if shape(prior_mean) not in ((npar,), (ncol, npar)):
        raise ValueError(f"prior_mean must be {(ncol, npar)} or {(npar,)}, got {shape(prior_mean)}")
    if shape(prior_precision) not in ((npar, npar), (ncol, npar, npar)):
        raise ValueError(f"prior_precision must be {(ncol, npar, npar)} or {(npar, npar)}, got {shape(prior_precision)}")
    return True


def _check_shared(shared, chain, params, p0=None):
    """``shared=`` of a retrieval plan whose parameter axis is ``params``, as far as no device is needed: a sequence of names out of
    ``params`` or a boolean mask ``(npar,)``.  -> None (no shared set) or the mask of ``crt_lm_shared`` (bit ``k``: parameter ``k``)"""
    import numpy as np

    if shared is None:
        return None
    if chain is None:
        raise ValueError("shared needs chain= the number of dates: the parameters are shared by the dates of a pixel")
    npar = len(params)
    if isinstance(shared, str):
        shared = (shared,)
    items = list(shared.tolist() if isinstance(shared, (np.ndarray, torch.Tensor)) else shared)
    if all(isinstance(v, str) for v in items):  # (an empty sequence: no name, nothing shared)
        unknown = [v for v in items if v not in params]
        if unknown:
            raise ValueError(f"shared names {unknown} are not among the parameters {tuple(params)}")
        bits = [n in items for n in params]
    elif all(isinstance(v, (bool, np.bool_)) for v in items):
        if len(items) != npar:
            raise ValueError(f"a shared mask must have one entry for each of the {npar} parameters {tuple(params)}, got {len(items)}")
        bits = [bool(v) for v in items]
    else:
        raise ValueError("shared must be a sequence of parameter names or a boolean mask (npar,)")
    if isinstance(p0, LutTable):
        raise ValueError("a look-up-table start (p0= a LutTable) cannot be combined with shared: the dates' best candidates disagree on "
                         "the shared parameters")
    return sum(1 << k for k, b in enumerate(bits) if b)


def _check_chain(chain, inv_sigma_chain, ncol, npar, shared=None):
    """``chain=nd`` and ``inv_sigma_chain=`` of a retrieval plan with ``ncol`` columns (or: of the :class:`Columns` ``ncol``), as far as no
    device is needed; ``shared``: the mask :func:`_check_shared` gave, which sets the limit on ``nd``.  -> None (no chain) or (npix, nd)"""
    if chain is None:
        if inv_sigma_chain is not None:
            raise ValueError("inv_sigma_chain needs chain= the number of dates")
        return None
    nd = int(chain)
    if nd != chain or nd < 1:
        raise ValueError(f"chain must be the number of dates, an integer >= 1, got {chain!r}")
    ncol = ncol if isinstance(ncol, int) else ncol.ncol
    if ncol % nd:
        raise ValueError(f"chain = {nd} dates does not divide ncol = {ncol}: the columns are (pixel, date) pairs, pixel-major")
    ns = 0 if shared is None else bin(shared).count("1")
    limit = _lib.lm_shared_max_nd(npar, ns)
    if nd > limit and shared is None:
        raise ValueError(f"chain = {nd} dates is beyond the {limit} the chain kernel serves at npar = {npar}")
    if nd > limit:
        raise ValueError(f"chain = {nd} dates is beyond the {limit} the shared-parameter kernel serves at npar = {npar} with {ns} shared")
    npix = ncol // nd
    if inv_sigma_chain is None:
        raise ValueError("a chain needs inv_sigma_chain (nd - 1, npar) or (npix, nd - 1, npar)")
    w = torch.as_tensor(inv_sigma_chain)
    if tuple(w.shape) not in ((nd - 1, npar), (npix, nd - 1, npar)):
        raise ValueError(f"inv_sigma_chain must be {(nd - 1, npar)} or {(npix, nd - 1, npar)}, got {tuple(w.shape)}")
    if not bool((w >= 0).all()):  # (false for NaN)
        raise ValueError("inv_sigma_chain must be >= 0 (0: not coupled across that gap) and not NaN")
    return npix, nd


EVALUATE_MODES = ("all", "running", "accepted")


def _check_evaluate(evaluate, scheme, chain, spectral):
    """``evaluate=`` of the retrieval plans (no device): ``"all"`` -- every column at every step, the plan as it always was; ``"running"`` --
    the masked entries of include_mask/crt1d_hip_masked.h skip the columns (with a chain: the pixels) that have stopped; ``"accepted"`` --
    the forward sums first, ``crt_hip_lm_decide_f64``, then the Jacobian only where the trial point will be accepted."""
    if evaluate not in EVALUATE_MODES:
        raise ValueError(f"evaluate must be one of {EVALUATE_MODES}, got {evaluate!r}")
    if evaluate == "all":
        return
    if evaluate == "accepted":
        if spectral:
            raise ValueError("evaluate='accepted' is not served by a spectral plan: the cost comes out of the kernel that forms the normal "
                             "equations (a cost-only first pass does not exist); use evaluate='running'")
        if chain is not None:
            raise ValueError("evaluate='accepted' is not served by a chained plan: acceptance is per pixel and includes the coupling terms; "
                             "use evaluate='running'")
        if scheme not in SENSJAC_SCHEMES:
            raise ValueError(f"evaluate='accepted' is not served by a composed plan: the sensor Jacobian of {scheme} is three calls without a "
                             "mask")
    if scheme not in MASKED_SCHEMES:
        raise ValueError(f"evaluate={evaluate!r} needs the masked kernels; scheme {scheme!r} has none (served: " + ", ".join(MASKED_SCHEMES) + ")")


class _LmPlan:
    """What :class:`RetrievalPlan` and :class:`SpectralRetrievalPlan` share: the base and the working :class:`Columns` / :class:`Bands`, the
    leaf-angle tangent, the leaf-model binding, the bounds, the prior, the starting point and the Levenberg-Marquardt state, the structs
    of ``k_retrieve_apply`` and of the step kernels, and the first launches of an evaluation.  A subclass supplies ``_inner`` -- its inner
    plan or plans, bound to the working tensors, and its observation structs -- and ``step``, which closes an evaluation with its C
    call."""

    _owns_sums = True  # a chained plan allocates its block of per-column sums; False: the subclass's _inner binds ``_blk`` to its own

    def _construct(self, keys, axis, o, scheme, cols, bands, levels, sun, p0, lo, hi, prior, inv_sigma_prior, leaf_model, chain=None,
                   inv_sigma_chain=None, shared=None, evaluate="all", prior_mean=None, prior_precision=None, **inner):
        self.lib = _lib.load()
        self.scheme, self.keys, self.sun, self.options = scheme, keys, sun, o
        ncol, nz, nb, dev = cols.ncol, cols.nz, bands.nb, cols.device
        npar, ntan, lai, leaf = axis.npar, axis.ntan, axis.lai, axis.leaf
        f64 = dict(dtype=torch.float64, device=dev)
        new = lambda *shape: torch.zeros(shape, **f64)  # noqa: E731
        # the status of every unit (column; with a chain: pixel) first: with evaluate != "all" it is the skip flags of the inner plans
        self.evaluate, self.nsteps = evaluate, 0
        self.nd = None if chain is None else int(chain)
        nunit = self.npix = ncol if chain is None else ncol // self.nd
        i32 = dict(dtype=torch.int32, device=dev)
        self.status, self.naccept, self.nreject = (torch.zeros((nunit,), **i32) for _ in range(3))
        self._skip = {} if evaluate == "all" else dict(skip=self.status, skip_unit=self.nd or 1)
        if evaluate == "accepted":  # what crt_hip_lm_decide_f64 writes: the Jacobian's own skip flags and the trial cost
            self.skip_jac, self.cost_t = torch.ones((ncol,), **i32), new(ncol)
        # the base state and the working inputs k_retrieve_apply overwrites
        self.base_cols, self.base_bands = cols, bands
        self._base_stride = bands.col_stride(ncol)
        rows = lambda v: None if v is None else v.expand(ncol, -1).contiguous()  # noqa: E731
        self.bands = Bands(rows(bands.I_dr0), rows(bands.I_df0), new(ncol, nb), new(ncol, nb), None if bands.soil_r is None else new(ncol, nb))
        self.cols = Columns(cols.psi, cols.lai.clone(), cols.g_kind, cols.g_param.clone(), cols.mla, cols.g_at_psi, cols.g_table)
        self.lai_scale = torch.ones((ncol,), **f64)
        # the leaf-angle tangent, refilled in place at every evaluation
        self.tangent = None
        if leaf:
            self.tangent = (LeafTangent(new(ncol, _lib.NQ), new(ncol)) if sun is None
                            else LeafTangentSeries(new(ncol, _lib.NQ), new(ncol, sun.nt)))
        # the leaf model: the plan owns the per-column directions k_plate_leaf writes and the inner plan reads
        self.leaf_model = leaf_model
        self._leaf = None if leaf_model is None else _PlateLeafBinding(leaf_model, axis, ncol, nb, dev)
        dirs = axis.given if self._leaf is None else self._leaf.dirs
        held = self._inner(scheme, levels, sun, **inner, **{"d_" + n: d for n, d in dirs.items()}, lai=lai, tangent=self.tangent, keys=keys)
        self.params, self.levels, self.npar, self.ntan = axis.params, held.levels, npar, ntan
        self._dirs = held._dirs  # what k_retrieve_apply adds to the base spectra: the inner plan's directions
        if self._leaf is not None:
            self._leaf.bound_to(held)
            self._dirs = self._leaf.apply_dirs
        self.lo = None if lo is None else torch.as_tensor(lo, dtype=torch.float64).to(dev).contiguous()
        self.hi = None if hi is None else torch.as_tensor(hi, dtype=torch.float64).to(dev).contiguous()
        self.prior = None if prior is None else _per_col(prior, "prior", ncol, npar, dev)
        self.inv_sigma_prior = None if prior is None else _per_col(inv_sigma_prior, "inv_sigma_prior", ncol, npar, dev)
        # the parameters all dates of a pixel share: the prior of such a parameter counts once, through date 0's row
        mask = _check_shared(shared, chain, axis.params, p0)
        self.shared = None if mask is None else tuple(n for k, n in enumerate(axis.params) if mask >> k & 1)
        self._shared = None if mask is None else _lib.CrtLmShared(mask)
        self._shared_idx = None if mask is None else torch.tensor([k for k in range(npar) if mask >> k & 1], dtype=torch.int64, device=dev)
        if mask is not None and self.inv_sigma_prior is not None and self._shared_idx.numel():
            self.inv_sigma_prior = self.inv_sigma_prior.clone()
            self.inv_sigma_prior.view(-1, int(chain), npar)[:, 1:, self._shared_idx] = 0.0
        table = p0 if isinstance(p0, LutTable) else None
        if table is not None:  # a column without an eligible candidate gets table.p_default, else the default start (a leaf model has none: q[0])
            if table.q.device != dev:
                raise ValueError(f"the table lives on {table.q.device} but the columns on {dev}")
            p0 = table.p_default if table.p_default is not None else None if leaf_model is None else table.q[0]
        if p0 is None:
            p0 = new(ncol, npar)
            if leaf:
                p0[:, npar - 1] = cols.g_param
        self._p0 = _per_col(p0, "p0", ncol, npar, dev).clone()
        # the state
        ntri = npar * (npar + 1) // 2
        # (a chain of nd dates: the columns are (pixel, date) pairs, p, p_trial, A and g stay per column, the rest is per pixel)
        self.p, self.p_trial, self.cost, self.lam = new(ncol, npar), new(ncol, npar), new(nunit), new(nunit)
        self.A, self.g = new(ncol, ntri), new(ncol, npar)
        self.cov = new(ncol, npar, npar)
        # the structs of the entries: k_retrieve_apply at the trial point (_ap) and at the accepted point (_ap_p)
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        b, w, c = bands, self.bands, self.cols
        apply = lambda p: _lib.CrtRetrieveApply(ncol, nz, nb, npar, ntan if lai else -1, ntan + lai if leaf else -1,  # noqa: E731
                                                self._base_stride, ptr(b.leaf_r), ptr(b.leaf_t), ptr(b.soil_r), ptr(cols.lai), ptr(p),
                                                ptr(w.leaf_r), ptr(w.leaf_t), ptr(w.soil_r), ptr(self.lai_scale), ptr(c.lai), ptr(c.g_param))
        self._ap, self._ap_p = apply(self.p_trial), apply(self.p)
        self._prob = _lib.CrtLmProblem(ncol, npar, o["lam_up"], o["lam_down"], o["lam_min"], o["lam_max"], o["xtol"], o["ftol"], ptr(self.lo),
                                       ptr(self.hi), ptr(self.prior), ptr(self.inv_sigma_prior))
        self._state = _lib.CrtLmState(*[ptr(v) for v in (self.p, self.p_trial, self.cost, self.lam, self.A, self.g, self.status, self.naccept,
                                                          self.nreject)])
        self._c = c.c_struct()
        self._s = None if sun is None else sun.c_struct()
        if chain is not None:  # the coupling weights, and the block of per-column sums of a plan that has none of its own
            w = self.inv_sigma_chain = torch.as_tensor(inv_sigma_chain, dtype=torch.float64).to(dev).contiguous()
            self._chain = _lib.CrtLmChain(nunit, self.nd, 0 if w.ndim == 2 else (self.nd - 1) * npar, ptr(w) if self.nd > 1 else None)
            if self._owns_sums:
                self.sums = (new(ncol, ntri), new(ncol, npar), new(ncol))
                self._blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[v.data_ptr() for v in self.sums]))
        # the full Gaussian prior (include_seq/crt1d_hip_lm_seq.h): its mean and packed precision, owned by the plan and bound by pointer,
        # the block of sums k_lm_prior_block writes, and the two blocks the closing call reads: the data's sums, then the prior's
        self._pf = None
        if _check_full_prior(prior_mean, prior_precision, chain, evaluate, ncol, npar):
            self.prior_mean = _per_col(prior_mean, "prior_mean", ncol, npar, dev).clone()
            P = torch.as_tensor(prior_precision, dtype=torch.float64).to(dev)
            self.prior_precision = pack_lower(P.expand(ncol, npar, npar)).clone()
            if self._owns_sums:
                self.sums = (new(ncol, ntri), new(ncol, npar), new(ncol))
                self._blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[v.data_ptr() for v in self.sums]))
            self.prior_sums = (new(ncol, ntri), new(ncol, npar), new(ncol))
            self._blk2 = (_lib.CrtLmNormalBlock * 2)(self._blk[0], _lib.CrtLmNormalBlock(*[v.data_ptr() for v in self.prior_sums]))
            self._pf = _lib.CrtLmPriorFull(ncol, npar, ntri, self.prior_precision.data_ptr(), self.prior_mean.data_ptr())
        # the look-up-table start: the best candidate of every column on the plan's own observations and prior
        self.lut = None if table is None else LutMatchPlan(table, self.y, inv_sigma=self.inv_sigma or None, prior=self.prior,
                                                           inv_sigma_prior=self.inv_sigma_prior, p_default=self._p0)
        self._post = None  # (temperature, the LutPosteriorPlan of lut_posterior())
        self.reset()

    def _evaluate(self, ap, s):
        """The launches every evaluation starts with, on stream ``s``: the working inputs from the parameters behind ``ap``, the leaf model,
        the tangent refill.  (The caller has entered ``torch.cuda.device``.)"""
        lib, ref, h = self.lib, ctypes.byref, s.cuda_stream
        _lib.check(lib.crt_hip_retrieve_apply_f64(ref(ap), None if self._dirs is None else ref(self._dirs), h), "crt_hip_retrieve_apply_f64")
        if self._leaf is not None:
            self._leaf.launch(lib, ap.p, self.npar, self.bands, h)
        t = self.tangent
        if t is not None and self.sun is None:
            _lib.check(lib.crt_hip_g_dparam_f64(ref(self._c), t.dg_table.data_ptr(), t.dg_at_psi.data_ptr(), h), "crt_hip_g_dparam_f64")
        elif t is not None:
            _lib.check(lib.crt_hip_g_dparam_series_f64(ref(self._c), ref(self._s), t.dg_table.data_ptr(), t.dg_at_psi.data_ptr(), h),
                       "crt_hip_g_dparam_series_f64")

    def _step_chain(self, s):
        """The closing call of a chained ``step()``: ``crt_hip_lm_step_chain_f64`` (with ``shared``: ``crt_hip_lm_step_shared_f64``; one
        kernel behind both) on the plan's one block of sums."""
        if self._shared is not None:
            _lib.check(self.lib.crt_hip_lm_step_shared_f64(ctypes.byref(self._chain), ctypes.byref(self._shared), ctypes.byref(self._prob),
                                                           self._blk, 1, ctypes.byref(self._state), s.cuda_stream), "crt_hip_lm_step_shared_f64")
            return
        _lib.check(self.lib.crt_hip_lm_step_chain_f64(ctypes.byref(self._chain), ctypes.byref(self._prob), self._blk, 1, ctypes.byref(self._state),
                                                      s.cuda_stream), "crt_hip_lm_step_chain_f64")

    def _step_full_prior(self, s):
        """The closing calls of a ``step()`` with ``prior_precision``: ``crt_hip_lm_prior_block_f64`` at the trial point, then
        ``crt_hip_lm_step_normal_f64`` on the two blocks -- the sums of the data, the sums of the prior."""
        h = s.cuda_stream
        _lib.check(self.lib.crt_hip_lm_prior_block_f64(ctypes.byref(self._pf), self.p_trial.data_ptr(), *[v.data_ptr() for v in self.prior_sums], h),
                   "crt_hip_lm_prior_block_f64")
        _lib.check(self.lib.crt_hip_lm_step_normal_f64(ctypes.byref(self._prob), self._blk2, 2, ctypes.byref(self._state), h),
                   "crt_hip_lm_step_normal_f64")

    def averaging_kernel(self, stream=None):
        """``(ncol, npar, npar)``: ``I - cov @ (P + diag(inv_sigma_prior^2))`` with ``cov`` of :meth:`covariance` and ``P`` the full prior
        precision -- the sensitivity of the retrieved state to the true one (the identity where the data decide, zero where the prior
        does; the identity without any prior).  Plain torch on :meth:`covariance`; not for a chained plan (ValueError)."""
        if self.nd is not None:
            raise ValueError("averaging_kernel() is not defined for a chained plan: the prior of a date includes its neighbours")
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        cov = self.covariance(stream=s)
        with torch.cuda.stream(s):
            H = torch.zeros_like(cov) if self._pf is None else unpack_lower(self.prior_precision, self.npar)
            if self.inv_sigma_prior is not None:
                H = H + torch.diag_embed(self.inv_sigma_prior * self.inv_sigma_prior)
            return torch.eye(self.npar, dtype=cov.dtype, device=dev) - cov @ H

    def dfs(self, stream=None):
        """``(ncol,)``: the degrees of freedom for signal, the trace of :meth:`averaging_kernel`."""
        return torch.diagonal(self.averaging_kernel(stream), dim1=1, dim2=2).sum(1)

    def reset(self, p0=None):
        """Restart the state at ``p0`` (default: the plan's starting point): ``p = p_trial = p0``, ``cost = +inf``, ``lam = lam0``.  A plan
        made with ``p0=`` a :class:`LutTable` and restarted without ``p0`` runs its match (``plan.lut``) on the current stream and starts
        every column at its best candidate; the host is not synchronised."""
        if p0 is not None:
            v = torch.as_tensor(p0, dtype=torch.float64).to(self.p.device)
            self._p0.copy_(v.expand_as(self._p0))
        elif self.lut is not None:
            self._p0.copy_(self.lut()["p"])
        if self._shared is not None and self._shared_idx.numel():  # a shared parameter starts at date 0's value on every date
            v = self._p0.view(self.npix, self.nd, self.npar)
            v[:, 1:, self._shared_idx] = v[:, :1, self._shared_idx]
        self.p.copy_(self._p0)
        self.p_trial.copy_(self._p0)
        self.cost.fill_(float("inf"))
        self.lam.fill_(self.options["lam0"])
        for v in (self.A, self.g, self.status, self.naccept, self.nreject):
            v.zero_()
        self.nsteps = 0
        return self

    def lut_posterior(self, temperature=1.0, stream=None):
        """The Bayesian look-up-table estimate of a plan started with ``p0=`` a :class:`LutTable`: a :class:`LutPosteriorPlan` on the plan's
        own ``y``, ``inv_sigma`` and prior (built at the first call, reused while ``temperature`` stays the same number or tensor), called on
        ``stream``; its dict.  It reads the observations, not the state of the iteration.  ValueError without a table."""
        if self.lut is None:
            raise ValueError("lut_posterior() needs a plan started from a look-up table: p0= a LutTable")
        held = None if self._post is None else self._post[0]
        tensors = isinstance(temperature, torch.Tensor) or isinstance(held, torch.Tensor)
        if self._post is None or not (held is temperature or (not tensors and held == temperature)):
            self._post = (temperature, LutPosteriorPlan(self.lut.table, self.y, inv_sigma=self.inv_sigma or None, prior=self.prior,
                                                        inv_sigma_prior=self.inv_sigma_prior, temperature=temperature))
        return self._post[1](stream)

    def running(self):
        """The number of units (columns; with a chain: pixels) that are still running, a 0-d int64 tensor on the device, formed on the
        current stream; the host is not synchronised."""
        return (self.status == 0).sum()

    def run(self, niter, stream=None, check_every=None):
        """``niter`` steps with no host synchronisation in between.  ``check_every=k``: the count of :meth:`running` is read after every
        ``k`` steps -- the one host synchronisation the caller asks for -- and the loop ends once it is 0; a unit that has stopped is not
        touched by a step, so the state is bitwise that of all ``niter`` steps.  ``plan.nsteps`` counts the steps since the last
        :meth:`reset`."""
        if check_every is not None and (isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1):
            raise ValueError(f"check_every must be None or an integer >= 1, got {check_every!r}")
        dev = self.cols.device
        for i in range(int(niter)):
            self.step(stream)
            if check_every is not None and (i + 1) % check_every == 0:
                with torch.cuda.stream(torch.cuda.current_stream(dev) if stream is None else stream):
                    left = int(self.running())
                if left == 0:
                    break
        return self

    def result(self):
        """Copies of ``p``, ``cost``, ``status`` (``LM_*``), ``lam``, ``naccept``, ``nreject``, and ``params``, the names of the columns of ``p``."""
        r = {k: getattr(self, k).clone() for k in ("p", "cost", "status", "lam", "naccept", "nreject")}
        if self.nd is not None:  # p (npix, nd, npar); cost, status, lam and the counters per pixel
            r["p"] = r["p"].reshape(self.npix, self.nd, self.npar)
        r["params"] = self.params
        return r

    def nobs(self):
        """``(ncol,)``: the rows every column is observed in (``inv_sigma != 0``), the rows of the prior included."""
        n = torch.zeros_like(self.cost) if self.nd is None else self.p.new_zeros(self.p.shape[0])
        for k in self.keys:
            n += float(self.nrow) if k not in self.inv_sigma else (self.inv_sigma[k] != 0).reshape(n.shape[0], -1).sum(1)
        if self.inv_sigma_prior is not None:
            n += (self.inv_sigma_prior != 0).sum(1)
        return n

    def covariance(self, scale=False, stream=None):
        """The posterior covariance ``(ncol, npar, npar)``: the inverse of the undamped normal matrix at the accepted point
        (``crt_hip_lm_covariance_f64``); a dead parameter has variance ``+inf`` and zero covariances.  ``scale=True`` multiplies by the
        reduced chi-square ``2 cost / (nobs - npar)`` (for observations without error estimates).  With a chain: ``(npix, nd, npar,
        npar)``, the smoothed marginal covariance of every date (``crt_hip_lm_chain_covariance_f64``: the diagonal blocks of the inverse
        of the pixel's block-tridiagonal matrix); ``scale=True`` is a ValueError then -- the coupling is a prior with a stated sigma.
        With ``shared``: ``crt_hip_lm_shared_covariance_f64``, for every date the marginal covariance of its varying parameters and the
        shared ones in the plan's parameter order; the shared-shared block has the same bits on every date."""
        if self.nd is not None and scale:
            raise ValueError("covariance(scale=True) has no meaning with a chain: the coupling is a prior with a stated sigma")
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        if self.nd is not None and self._shared is not None:
            with torch.cuda.device(dev):
                _lib.check(self.lib.crt_hip_lm_shared_covariance_f64(ctypes.byref(self._chain), ctypes.byref(self._shared), self.npar,
                                                                     self.A.data_ptr(), self.cov.data_ptr(), s.cuda_stream),
                           "crt_hip_lm_shared_covariance_f64")
            return self.cov.reshape(self.npix, self.nd, self.npar, self.npar).clone()
        if self.nd is not None:
            with torch.cuda.device(dev):
                _lib.check(self.lib.crt_hip_lm_chain_covariance_f64(ctypes.byref(self._chain), self.npar, self.A.data_ptr(), self.cov.data_ptr(),
                                                                    s.cuda_stream), "crt_hip_lm_chain_covariance_f64")
            return self.cov.reshape(self.npix, self.nd, self.npar, self.npar).clone()
        with torch.cuda.device(dev):
            _lib.check(self.lib.crt_hip_lm_covariance_f64(self.p.shape[0], self.npar, self.A.data_ptr(), self.cov.data_ptr(), s.cuda_stream),
                       "crt_hip_lm_covariance_f64")
        if not scale:
            return self.cov.clone()
        with torch.cuda.stream(s):
            return self.cov * (2.0 * self.cost / (self.nobs() - self.npar))[:, None, None]


class RetrievalPlan(_LmPlan):
    """A Levenberg-Marquardt retrieval of a parameter vector of every column from sensor-band observations, with the whole loop on the
    device (include/crt1d_hip_retrieve.h): no host synchronisation between steps, no allocation after construction.

    ``cols``, ``bands`` (with ``sun``: a :class:`SunSeries` that supplies the sun angles and the incoming spectra) are the base state;
    ``y[k]`` are the observations of the sums :class:`SensorLevelsPlan` (``sun``: :class:`SensorLevelsSeriesPlan`) gives for ``keys``,
    each ``(ncol, [nt,] nsel, nsens)``; ``inv_sigma[k]`` their weights (``None`` / a missing key: ones; an entry 0: not observed, its
    ``y`` may be NaN).  The parameters, in the order of ``SensorJacPlan.params``: the coefficients of the ``ntan`` directions
    ``d_leaf_r / d_leaf_t / d_soil_r`` added to the base spectra; ``"lai"`` (``lai=True``): the log of a scale of the base LAI profile;
    ``"leaf"`` (``leaf=True``): the column's ``g_param`` itself (``wrt="param"`` of :func:`leaf_tangent`; ``mla`` stays fixed).  For the
    parameterless leaf-angle kinds and ``G_TABLE`` columns ``dG`` is zero: the parameter is dead there and stays where it started.
    ``p0 (ncol, npar)`` or ``(npar,)``: the starting point (default: zeros, and ``cols.g_param`` for ``"leaf"``); ``lo``, ``hi`` ``(npar,)``:
    bounds, which also keep the optics physical -- nothing else clamps them; ``prior``, ``inv_sigma_prior`` ``(ncol, npar)`` or ``(npar,)``:
    a Gaussian prior.  ``lam0`` and the options ``lam_up, lam_down, lam_min, lam_max, xtol, ftol`` are those of the header.

    :meth:`step` is five launches in a row: ``k_retrieve_apply`` writes the working :class:`Columns` / :class:`Bands` from the trial
    point; ``crt_hip_g_dparam_f64`` refills the leaf-angle tangent; the :class:`SensorJacPlan` (``sun``: :class:`SensorJacSeriesPlan`)
    bound to the working tensors; the forward sums on its workspace with ``FLAG_SKIP_PRECOMPUTE``; ``k_lm_step``.  The first step
    evaluates ``p0`` and is always accepted.  n79 and zq run the composed Jacobian plan (workspaces and allocations of its own) and the
    forward plan with its own precompute; ``4s`` and ``zq_pa`` are a ValueError.  A column's state is bitwise the same alone or in any
    batch.  float64 only.

    ``leaf_model``: a :class:`crt1d_amd.leaf_model.PlateLeafModel` -- the leaf spectra are the plate model's, and its ``nm`` parameters
    ``leaf_model.params`` = ``("N", contents...)`` are retrieved in place of coefficients of leaf directions.  The parameter axis is then
    the model's parameters, the ``ns`` soil directions ``d_soil_r`` (``"dir0"``, ...), ``"lai"``, ``"leaf"``, with ``nm + ns <= 8``;
    ``d_leaf_r`` / ``d_leaf_t`` are a ValueError; ``lo`` / ``hi`` are required and must keep ``N`` inside [1, 4] and every content
    ``>= 0``; ``p0`` is required; ``bands.leaf_r / leaf_t`` are not used.  The plan owns per-column direction arrays of ``nm + ns`` rows
    (``3 x ncol x (nm + ns) x nb x 8`` bytes), and :meth:`step` is one launch more: ``k_retrieve_apply`` with the leaf directions left out,
    then ``crt_hip_plate_leaf_f64`` on the same parameter array, which writes the working leaf spectra and the model's partials into
    the leaf rows, then the launches above.

    ``chain=nd`` with ``inv_sigma_chain`` ``(nd - 1, npar)`` or ``(npix, nd - 1, npar)``: a time series (include_chain/
    crt1d_hip_lm_chain.h).  The ``ncol = npix * nd`` columns are (pixel, date) pairs, pixel-major; ``cols``, ``bands``, ``y``, ``sun``,
    ``leaf_model`` and ``p0`` keep their per-column meaning, so every date has its own ``psi`` and illumination; the parameter vectors of
    consecutive dates of a pixel are coupled by a random-walk prior with the weights ``inv_sigma_chain`` (``(p_{d+1} - p_d) *
    inv_sigma_chain[d]`` is a residual; 0: not coupled; fold the time gap in).  A date whose rows are all masked gets its value from
    its neighbours.  The last launch of :meth:`step` becomes two: ``k_lm_normal`` writes the sums ``k_lm_step`` would have formed,
    ``crt_hip_lm_step_chain_f64`` accepts or rejects, damps and solves the block-tridiagonal system of every pixel.  ``result()`` then gives
    ``p (npix, nd, npar)`` and per-pixel ``cost``, ``status``, ``lam`` and counters, ``covariance()`` the smoothed marginal covariances
    ``(npix, nd, npar, npar)``.  ``chain=None``: the plan as it always was, call for call.

    ``shared=`` (needs ``chain=``): the parameters that are constants of a pixel over its ``nd`` dates -- a sequence of names out of
    ``plan.params`` (``"lai"``, ``"leaf"``, ``"dir0"``.. or leaf-model names) or a boolean mask ``(npar,)`` (include_shared/
    crt1d_hip_lm_shared.h).  Such a parameter is ONE unknown of the pixel: the system has ``nd * nv + ns`` unknowns, the block-tridiagonal
    matrix bordered by ``ns`` dense rows, and the closing call is ``crt_hip_lm_step_shared_f64`` in place of ``crt_hip_lm_step_chain_f64`` (the number of
    launches is unchanged).  ``result()["p"]`` stays ``(npix, nd, npar)`` with the shared columns bitwise equal over the dates;
    ``inv_sigma_chain`` keeps its shape, its entries of shared parameters are not read.  ``p0`` / ``reset(p0)``: the shared entries of
    the dates after the first are overwritten with date 0's.  ``prior`` / ``inv_sigma_prior``: for a shared parameter the plan keeps date
    0's row and zeroes ``inv_sigma_prior`` on the other dates, so that the prior counts once.  ``p0=`` a :class:`LutTable` together with
    ``shared`` is a ValueError.  ``shared=None``: the chained plan, call for call.

    ``prior_mean`` ``(ncol, npar)`` or ``(npar,)`` with ``prior_precision`` ``(ncol, npar, npar)`` or ``(npar, npar)`` (only the lower
    triangle is read): a Gaussian prior with a FULL precision matrix (include_seq/crt1d_hip_lm_seq.h), independent of ``prior`` /
    ``inv_sigma_prior`` and added to them -- a covariance another retrieval produced (``covariance()``, ``lut_posterior()["cov"]``),
    inverted, or a trait-database prior with correlated parameters.  The plan keeps ``plan.prior_mean (ncol, npar)`` and
    ``plan.prior_precision (ncol, ntri)`` (the packed lower triangles of :func:`pack_lower`), bound by pointer: both may be updated in
    place between steps.  The last launch of :meth:`step` becomes three: ``k_lm_normal`` writes the sums of the data,
    ``crt_hip_lm_prior_block_f64`` the sums of the prior at the trial point, ``crt_hip_lm_step_normal_f64`` decides on the two blocks; the
    stored ``A`` then includes the prior, so ``covariance()`` is the posterior covariance.  With or without ``sun``, ``leaf_model`` and
    ``evaluate="running"``; together with ``chain=`` or ``evaluate="accepted"``, or one of the two without the other: a ValueError.
    ``p0=`` a :class:`LutTable` stays allowed, but the match and ``lut_posterior()`` see the diagonal prior only: ``plan.lut.cost`` is
    then not the first step's cost.  :meth:`averaging_kernel` and :meth:`dfs` give the averaging kernel and the degrees of freedom for
    signal.  Without the two arguments the plan is what it was, launch for launch."""

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, y, *, keys, sun=None, d_leaf_r=None, d_leaf_t=None,
                 d_soil_r=None, lai=True, leaf=False, p0=None, lo=None, hi=None, inv_sigma=None, prior=None, inv_sigma_prior=None,
                 leaf_model=None, chain=None, inv_sigma_chain=None, shared=None, evaluate="all", prior_mean=None, prior_precision=None,
                 mu_s=0.501, tau_d_method="quad", **options):
        static = self._static(scheme, cols, bands, levels, sensors, y, keys=keys, sun=sun, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t,
                              d_soil_r=d_soil_r, lai=lai, leaf=leaf, p0=p0, lo=lo, hi=hi, inv_sigma=inv_sigma, prior=prior,
                              inv_sigma_prior=inv_sigma_prior, leaf_model=leaf_model, chain=chain, inv_sigma_chain=inv_sigma_chain,
                              shared=shared, evaluate=evaluate, prior_mean=prior_mean, prior_precision=prior_precision,
                              tau_d_method=tau_d_method, **options)
        self._construct(*static, scheme, cols, bands, levels, sun, p0, lo, hi, prior, inv_sigma_prior, leaf_model, chain=chain,
                        inv_sigma_chain=inv_sigma_chain, shared=shared, evaluate=evaluate, prior_mean=prior_mean,
                        prior_precision=prior_precision, sensors=sensors, y=y, inv_sigma=inv_sigma, mu_s=mu_s, tau_d_method=tau_d_method)

    @classmethod
    def _static(cls, scheme, cols, bands, levels, sensors, y, *, keys, sun=None, d_leaf_r=None, d_leaf_t=None, d_soil_r=None, lai=True,
                leaf=False, p0=None, lo=None, hi=None, inv_sigma=None, prior=None, inv_sigma_prior=None, leaf_model=None, chain=None,
                inv_sigma_chain=None, shared=None, evaluate="all", prior_mean=None, prior_precision=None, mu_s=0.501, tau_d_method="quad",
                **options):
        """The constructor's arguments -> (keys, the parameter axis, the LM options): every check that needs neither a column nor a
        device."""
        _SolvePlan._check_options(_SolvePlan, scheme, tau_d_method)
        if scheme not in RETRIEVE_SCHEMES:
            raise ValueError(f"scheme {scheme!r} has no retrieval; served: " + ", ".join(RETRIEVE_SCHEMES))
        _check_evaluate(evaluate, scheme, chain, False)
        keys = _level_keys(keys)
        if not isinstance(sensors, SensorSet):
            raise TypeError("sensors must be a SensorSet")
        if sun is not None:
            _need_sun_series(sun)
        _check_obs(y, inv_sigma, keys, "(ncol, [nt,] nsel, nsens)")
        axis = _ParamAxis(d_leaf_r, d_leaf_t, d_soil_r, lai, leaf, leaf_model)
        o = _lm_options(lo, hi, axis.npar, options)
        _need_f64_bands(bands, "retrieval")
        _check_start(leaf_model, lo, hi, p0, prior, inv_sigma_prior)
        if isinstance(p0, LutTable):
            _check_lut_start(p0, axis.params, keys, False, y)
        _check_chain(chain, inv_sigma_chain, cols, axis.npar, _check_shared(shared, chain, axis.params, p0))
        _check_full_prior(prior_mean, prior_precision, chain, evaluate, cols, axis.npar)
        return keys, axis, o

    def _inner(self, scheme, levels, sun, sensors, y, inv_sigma, keys, mu_s, tau_d_method, **axis):
        """The Jacobian plan and the forward plan on its workspace, the observations against the forward sums.  -> the Jacobian plan"""
        f = dict(keys=keys, mu_s=mu_s, tau_d_method=tau_d_method)
        a = (scheme, self.cols, self.bands) + (() if sun is None else (sun,)) + (levels, sensors)
        jskip = self._skip if self.evaluate != "accepted" else dict(skip=self.skip_jac, skip_unit=1)
        self.jac = (SensorJacPlan if sun is None else SensorJacSeriesPlan)(*a, **axis, **f, **jskip)
        self.fwd = (SensorLevelsPlan if sun is None else SensorLevelsSeriesPlan)(*a, **f, workspace=getattr(self.jac, "workspace", None), **self._skip)
        self._fwd_flags = 0 if self.jac._composed else _lib.FLAG_SKIP_PRECOMPUTE
        shape = tuple(self.fwd.out[keys[0]].shape)
        self.nrow = int(torch.Size(shape[1:]).numel())

        def obs(v, name):
            v = torch.as_tensor(v, dtype=torch.float64).to(self.cols.device).contiguous()
            if tuple(v.shape) != shape:
                raise ValueError(f"{name} must be {shape}, got {tuple(v.shape)}")
            return v

        self.y = {k: obs(y[k], f"y[{k!r}]") for k in keys}
        self.inv_sigma = {k: obs(inv_sigma[k], f"inv_sigma[{k!r}]") for k in keys if inv_sigma is not None and k in inv_sigma}
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        self._obs = (_lib.CrtLmObs * len(keys))(*[
            _lib.CrtLmObs(self.nrow, ptr(self.fwd.out[k]), ptr(self.jac.out[k]), ptr(self.y[k]), ptr(self.inv_sigma.get(k))) for k in keys])
        return self.jac

    def step(self, stream=None):
        """One iteration on ``stream`` (default: torch's current stream): apply, tangent, Jacobian, forward sums, ``k_lm_step``."""
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        self.nsteps += 1
        with torch.cuda.device(dev):
            self._evaluate(self._ap, s)
            if self.evaluate == "accepted":
                # the forward sums with their own precompute where the column runs, the decision k_lm_step will take, then the Jacobian
                # (with the precompute again: the forward plan's slice sums lie on its side records) where the trial point is accepted
                self.fwd(s, flags=0)
                _lib.check(self.lib.crt_hip_lm_decide_f64(ctypes.byref(self._prob), self._obs, len(self.keys), ctypes.byref(self._state),
                                                          self.skip_jac.data_ptr(), self.cost_t.data_ptr(), s.cuda_stream), "crt_hip_lm_decide_f64")
                self.jac(s)
            else:
                self.jac(s)
                self.fwd(s, flags=self._fwd_flags)
            if self.nd is not None:  # the last launch replaced by two: the sums of k_lm_step written out, then the step of every pixel
                _lib.check(self.lib.crt_hip_lm_normal_f64(self.p.shape[0], self.npar, self._obs, len(self.keys), *[v.data_ptr() for v in self.sums],
                                                          s.cuda_stream), "crt_hip_lm_normal_f64")
                self._step_chain(s)
                return self
            if self._pf is not None:  # the last launch replaced by three: the sums of k_lm_step written out, the prior's, the step on both
                _lib.check(self.lib.crt_hip_lm_normal_f64(self.p.shape[0], self.npar, self._obs, len(self.keys), *[v.data_ptr() for v in self.sums],
                                                          s.cuda_stream), "crt_hip_lm_normal_f64")
                self._step_full_prior(s)
                return self
            _lib.check(self.lib.crt_hip_lm_step_f64(ctypes.byref(self._prob), self._obs, len(self.keys), ctypes.byref(self._state), s.cuda_stream),
                       "crt_hip_lm_step_f64")
        return self



def retrieve(scheme, cols: Columns, bands: Bands, levels, sensors: SensorSet, y, *, keys, niter=20, posterior=False, **kw):
    """One-shot :class:`RetrievalPlan`: ``niter`` steps from ``p0``; what ``plan.result()`` returns, and ``"cov"``, ``plan.covariance()``.
    ``posterior=True`` (``p0`` a :class:`LutTable`, else ValueError) adds ``"lut_mean"``, ``"lut_cov"`` and ``"lut_ess"``, what
    ``plan.lut_posterior()`` gives."""
    if posterior and not isinstance(kw.get("p0"), LutTable):
        raise ValueError("posterior=True needs a look-up table: p0= a LutTable (Model: lut=K)")
    RetrievalPlan._static(scheme, cols, bands, levels, sensors, y, keys=keys, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        plan = RetrievalPlan(scheme, cols, bands, levels, sensors, y, keys=keys, **kw).run(niter)
        res = plan.result()
        res["cov"] = plan.covariance()
        if posterior:
            post = plan.lut_posterior()
            res.update({"lut_" + k: post[k].clone() for k in ("mean", "cov", "ess")})
    return res



# ---- the retrieval from the level spectra themselves (include/crt1d_hip_specfit.h) -------------------------------------------------------

SPECTRAL_RETRIEVE_SCHEMES = ("2s", "bl", "g77", "bf")  # the schemes k_spec_normal serves; n79 and zq stay composable by hand
SPECFIT_MAX_ROWS = 312  # nkey * nsel * (npar + 1) at most: the LDS limit of the header


def spectral_normal_workspace_bytes(scheme, ncol, nz, nb, nsel, nkey, npar):
    """Device workspace of a :class:`SpectralNormalPlan` call: the records of :func:`workspace_bytes` at the same offsets, the side
    records of the LAI and of the leaf-angle derivative, and the slice sums."""
    return int(_lib.load().crt_hip_spectral_normal_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nsel, nkey, npar))


def _spectral_static(scheme, y, keys, inv_sigma, tau_d_method, bands, sun, **axis):
    """The checks of the spectral plans that touch no device (``sun``: the series forms, whose arrays carry a sun-state axis; ``axis``: the
    arguments of :class:`_ParamAxis`).  -> (keys in ``LEVEL_KEYS`` order, the parameter axis)"""
    _SolvePlan._check_options(_SolvePlan, scheme, tau_d_method)
    if scheme not in SPECTRAL_RETRIEVE_SCHEMES:
        raise ValueError(f"scheme {scheme!r} has no spectral retrieval; served: " + ", ".join(SPECTRAL_RETRIEVE_SCHEMES))
    if sun is not None:
        _need_sun_series(sun)
    keys = _level_keys(keys)
    keys = tuple(k for k in LEVEL_KEYS if k in keys)
    _check_obs(y, inv_sigma, keys, "(ncol, nsel, nb)" if sun is None else "(ncol, nt, nsel, nb)", 3 if sun is None else 4)
    axis = _ParamAxis(**axis)
    _need_f64_bands(bands, "spectral retrieval")
    return keys, axis


def _spectral_shapes(cols, bands, levels, y, inv_sigma, nkey, npar, sun=None):
    """The shapes of the observations against ``(ncol, nsel, nb)`` (``sun``: ``(ncol, nt, nsel, nb)``) and the LDS limit; still no
    device.  -> the normalized levels"""
    levels = normalize_levels(levels, cols.nz)
    shape = (cols.ncol, *(() if sun is None else (sun.nt,)), len(levels), bands.nb)
    for name, d in (("y", y), ("inv_sigma", inv_sigma or {})):
        for k, v in d.items():
            if tuple(v.shape) != shape:
                raise ValueError(f"{name}[{k!r}] must be {shape}, got {tuple(v.shape)}")
    if nkey * len(levels) * (npar + 1) > SPECFIT_MAX_ROWS:
        raise ValueError(f"nkey * nsel * (npar + 1) = {nkey * len(levels) * (npar + 1)} exceeds {SPECFIT_MAX_ROWS}: select fewer levels or keys")
    return levels


class SpectralNormalPlan(_LevelsDerivPlan):
    """Pre-validated normal equations of the per-band misfit of the level spectra (``crt_hip_spectral_normal_f64``): with ``X`` the
    spectra of ``keys`` at ``levels``, ``r = (X - y) * inv_sigma`` and ``J`` their Jacobian with respect to the parameters of
    :class:`SensorJacPlan` (``d_leaf_r / d_leaf_t / d_soil_r``, ``lai``, ``tangent``; ``params`` names them), one column precompute and
    ONE kernel give ``out["A"] (ncol, npar (npar + 1) / 2)`` -- the lower triangle of ``J^T W J`` row by row --, ``out["g"] (ncol, npar)``
    ``= J^T W r`` and ``out["c2"] (ncol,)`` ``= sum r^2``.  Neither ``J`` nor a derivative array is written.  ``y[k]``, ``inv_sigma[k]``:
    ``(ncol, nsel, nb)`` (``inv_sigma`` ``None`` / a missing key: ones; an entry 0: the row is skipped, its ``y`` may be NaN); tensors on
    the columns' device are read where they lie at every call.  ``fwd=True`` also keeps ``out["fwd"][k] (ncol, nsel, nb)``, the model
    spectrum, written while ``plan.write_fwd`` is true.  A column's result is bitwise the same alone or in any batch and does not
    depend on another column's ``inv_sigma``; ``c2`` and ``fwd`` do not depend on which parameters exist.  ``SPECTRAL_RETRIEVE_SCHEMES``
    only; ``nkey * nsel * (npar + 1) <= SPECFIT_MAX_ROWS``."""

    _entry_name, _ws_query = "crt_hip_spectral_normal_f64", "crt_hip_spectral_normal_workspace_bytes"
    _all_keys, _schemes, _what = LEVEL_KEYS, SPECTRAL_RETRIEVE_SCHEMES, "spectral retrieval"

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, y, *, keys, inv_sigma=None, d_leaf_r=None, d_leaf_t=None, d_soil_r=None,
                 lai=True, tangent=None, fwd=False, mu_s=0.501, tau_d_method="quad", out=None, workspace=None, skip=None, skip_unit=1):
        self._build(None, scheme, cols, bands, levels, y, keys=keys, inv_sigma=inv_sigma, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t, d_soil_r=d_soil_r,
                    lai=lai, tangent=tangent, fwd=fwd, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace, skip=skip,
                    skip_unit=skip_unit)

    _entry_masked_name = "crt_hip_spectral_normal_masked_f64"
    _series = False  # SpectralNormalSeriesPlan: a sun-angle series in front of the levels, arrays with a sun-state axis

    @classmethod
    def _static(cls, scheme, cols, bands, levels, y, **kw):
        """The constructor's arguments (``kw``: its keywords) -> (keys in ``LEVEL_KEYS`` order, the parameter axis, the normalized
        levels): every check that needs no device."""
        return cls._static_of(None, scheme, cols, bands, levels, y, **kw)

    @classmethod
    def _static_of(cls, sun, scheme, cols, bands, levels, y, *, keys, inv_sigma=None, d_leaf_r=None, d_leaf_t=None, d_soil_r=None, lai=True,
                   tangent=None, per_step=False, fwd=False, mu_s=0.501, tau_d_method="quad", out=None, workspace=None, skip=None, skip_unit=1):
        _check_tangent(tangent, sun, cls._series)
        keys, axis = _spectral_static(scheme, y, keys, inv_sigma, tau_d_method, bands, sun, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t,
                                      d_soil_r=d_soil_r, lai=lai, tangent=tangent)
        _check_skip(skip, skip_unit, getattr(cols, "ncol", None), scheme, bands)
        return keys, axis, _spectral_shapes(cols, bands, levels, y, inv_sigma, len(keys), axis.npar, sun)

    def _build(self, sun, scheme, cols, bands, levels, y, *, inv_sigma, fwd, mu_s, tau_d_method, out, workspace, per_step=False, **kw):
        """The construction of this plan (``sun`` None) and of :class:`SpectralNormalSeriesPlan`."""
        skip, skip_unit = kw.get("skip"), kw.get("skip_unit", 1)
        keys, axis, self.levels = self._static_of(sun, scheme, cols, bands, levels, y, inv_sigma=inv_sigma, tau_d_method=tau_d_method, **kw)
        series = {} if sun is None else {"sun": sun}
        self.keys = keys
        ncol, nsel, nb, dev = cols.ncol, len(self.levels), bands.nb, cols.device
        nts = () if sun is None else (sun.nt,)
        shape = (ncol, *nts, nsel, nb)
        self._bind(scheme, cols, bands, mu_s, tau_d_method, **series)
        obs = lambda v: torch.as_tensor(v, dtype=torch.float64).to(dev).contiguous()  # noqa: E731
        self.y = {k: obs(y[k]) for k in keys}
        self.inv_sigma = {k: obs(inv_sigma[k]) for k in keys if inv_sigma is not None and k in inv_sigma}
        self._axis = axis.bind(ncol, nb, dev)
        self.dirs, self.tangent, self.ntan, self.npar, self.params = axis.dirs, axis.tangent, axis.ntan, axis.npar, axis.params
        self._dirs, self._tan = axis.c_dirs, axis.c_tan
        npar = axis.npar
        ntri = npar * (npar + 1) // 2
        shapes = {"A": (ncol, ntri), "g": (ncol, npar), "c2": (ncol,)}
        if per_step:
            shapes.update({"A_t": (ncol, *nts, ntri), "g_t": (ncol, *nts, npar), "c2_t": (ncol, *nts)})
        o = _outputs(shapes, out, torch.float64, dev, "output {!r}", lacks=True)
        self.out = {k: o[k] for k in shapes}
        self.write_fwd = bool(fwd)
        if fwd:
            self.out["fwd"] = {k: torch.empty(shape, dtype=torch.float64, device=dev) for k in keys}
        ptr = lambda d, k: d[k].data_ptr() if k in d else None  # noqa: E731
        self._obs = _lib.CrtSpecObs(*[ptr(self.y, k) for k in LEVEL_KEYS], *[ptr(self.inv_sigma, k) for k in LEVEL_KEYS])
        sums = [self.out[k].data_ptr() for k in ("A", "g", "c2")]
        struct = _lib.CrtSpecNormalOut
        if sun is not None:
            struct = _lib.CrtSpecSeriesOut
            sums += [ptr(self.out, k) for k in ("A_t", "g_t", "c2_t")]
        self._out_sums = struct(*sums, None, None, None, None)
        self._out_fwd = struct(*sums, *[ptr(self.out.get("fwd", {}), k) for k in LEVEL_KEYS])
        self._lev = (ctypes.c_int32 * nsel)(*self.levels)
        if sun is None:
            need = spectral_normal_workspace_bytes(scheme, ncol, cols.nz, nb, nsel, len(keys), npar)
        else:
            need = spectral_normal_series_workspace_bytes(scheme, ncol, cols.nz, nb, sun.nt, nsel, len(keys), npar)
        self._finish(self._entry_name, need, workspace)
        self._bind_skip(skip, skip_unit, self._entry_masked_name)

    def _tail(self):
        ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
        return (self._lev, len(self.levels), ref(self._dirs), int("lai" in self.params), ref(self._tan), ctypes.byref(self._obs),
                ctypes.byref(self._out_fwd if self.write_fwd else self._out_sums))

    def dense(self):
        """``out["A"]`` as the full symmetric matrices ``(ncol, npar, npar)`` (a new tensor)."""
        n = self.npar
        i, j = torch.tril_indices(n, n, device=self.out["A"].device)
        A = self.out["A"].new_zeros((self.out["A"].shape[0], n, n))
        A[:, i, j] = self.out["A"]
        A[:, j, i] = self.out["A"]
        return A


def spectral_normal(scheme, cols: Columns, bands: Bands, levels, y, *, keys, **kw):
    """One-shot :class:`SpectralNormalPlan`: ``{"A", "g", "c2"}`` (and ``"fwd"`` with ``fwd=True``) at the sorted levels."""
    SpectralNormalPlan._static(scheme, cols, bands, levels, y, keys=keys, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return SpectralNormalPlan(scheme, cols, bands, levels, y, keys=keys, **kw)()


def spectral_normal_series_workspace_bytes(scheme, ncol, nz, nb, nt, nsel, nkey, npar):
    """Device workspace of a :class:`SpectralNormalSeriesPlan` call: the records of :func:`levels_series_workspace_bytes` at the same
    offsets, the side records of the LAI and of the leaf-angle derivative, and the slice sums of every (column, t)."""
    return int(_lib.load().crt_hip_spectral_normal_series_workspace_bytes(_lib.SCHEME_IDS[scheme], ncol, nz, nb, nt, nsel, nkey, npar))


class SpectralNormalSeriesPlan(SpectralNormalPlan):
    """The normal equations of :class:`SpectralNormalPlan` for the ``sun.nt`` sun states of every column, summed over the sun states, in
    one call (``crt_hip_spectral_normal_series_f64``): ``y[k]``, ``inv_sigma[k]`` are ``(ncol, nt, nsel, nb)``, the parameter vector, the
    directions and the canopy are shared over ``t``, and ``out["A"]``, ``out["g"]``, ``out["c2"]`` are the sums a retrieval from a diurnal
    course consumes -- ONE block of ``crt_hip_lm_step_normal_f64`` whatever ``nt``.  ``per_step=True`` also keeps ``out["A_t"] (ncol, nt,
    ntri)``, ``out["g_t"] (ncol, nt, npar)`` and ``out["c2_t"] (ncol, nt)``; ``fwd=True`` ``out["fwd"][k] (ncol, nt, nsel, nb)``.  Slice
    ``[:, t]`` of those is bitwise what :class:`SpectralNormalPlan` gives with ``psi = sun.psi[:, t]`` (``g_at_psi`` likewise), the incoming
    spectra of step ``t``, ``tangent.step(t)`` and the observations of step ``t``; the sums are bitwise the left-to-right sum of the slices
    over ``t``.  An ``inv_sigma`` of 0 masks a band of a sun state (its ``y`` may be NaN); a sun state masked completely contributes ``+0``.
    ``cols.psi``, ``cols.g_at_psi`` and ``bands.I_dr0 / I_df0`` are not read.  ``sun``: a float64 :class:`SunSeries`; ``tangent``: a
    :class:`LeafTangentSeries` of the same ``nt`` or ``None``.  The canopy part of the column precompute and the side precomputes run once
    per column; the workspace starts with the records of a :class:`LevelsSeriesPlan`, which can run on it with ``FLAG_SKIP_PRECOMPUTE``."""

    _entry_name, _ws_query, _series = "crt_hip_spectral_normal_series_f64", "crt_hip_spectral_normal_series_workspace_bytes", True
    _entry_masked_name = "crt_hip_spectral_normal_series_masked_f64"

    def __init__(self, scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, y, *, keys, inv_sigma=None, d_leaf_r=None, d_leaf_t=None,
                 d_soil_r=None, lai=True, tangent=None, per_step=False, fwd=False, mu_s=0.501, tau_d_method="quad", out=None, workspace=None,
                 skip=None, skip_unit=1):
        self._build(sun, scheme, cols, bands, levels, y, keys=keys, inv_sigma=inv_sigma, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t, d_soil_r=d_soil_r,
                    lai=lai, tangent=tangent, per_step=per_step, fwd=fwd, mu_s=mu_s, tau_d_method=tau_d_method, out=out, workspace=workspace,
                    skip=skip, skip_unit=skip_unit)

    @classmethod
    def _static(cls, scheme, cols, bands, sun, levels, y, **kw):
        return cls._static_of(sun, scheme, cols, bands, levels, y, **kw)


def spectral_normal_series(scheme, cols: Columns, bands: Bands, sun: SunSeries, levels, y, *, keys, **kw):
    """One-shot :class:`SpectralNormalSeriesPlan`: ``{"A", "g", "c2"}`` (``per_step=True``: and ``"A_t", "g_t", "c2_t"``; ``fwd=True``: and
    ``"fwd"``) at the sorted levels."""
    SpectralNormalSeriesPlan._static(scheme, cols, bands, sun, levels, y, keys=keys, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        return SpectralNormalSeriesPlan(scheme, cols, bands, sun, levels, y, keys=keys, **kw)()


class SpectralRetrievalPlan(_LmPlan):
    """:class:`RetrievalPlan` without the sensors: a Levenberg-Marquardt retrieval of a parameter vector of every column from the level
    spectra themselves, band by band (include/crt1d_hip_specfit.h), with the whole loop on the device.  ``y[k] (ncol, nsel, nb)`` are
    the observed spectra of ``keys`` at ``levels`` (what :class:`LevelsPlan` gives), ``inv_sigma[k]`` their weights (``None`` / a missing
    key: ones; an entry 0: not observed -- a masked band --, its ``y`` may be NaN).  The parameters, ``p0``, ``lo``, ``hi``, ``prior``,
    ``inv_sigma_prior`` and the options are those of :class:`RetrievalPlan`.

    :meth:`step` is four launches in a row: ``k_retrieve_apply`` writes the working :class:`Columns` / :class:`Bands` from the trial
    point; ``crt_hip_g_dparam_f64`` refills the leaf-angle tangent; the :class:`SpectralNormalPlan` bound to the working tensors forms
    ``A``, ``g`` and ``c2``; ``crt_hip_lm_step_normal_f64`` decides.  Nothing the size of the spectrum is written, nothing is
    allocated after construction and the host is never synchronised.  ``SPECTRAL_RETRIEVE_SCHEMES`` only; float64 only.

    ``sun``: a float64 :class:`SunSeries` -- the diurnal course of a tower spectrometer, which separates LAI from the leaf angle: ``y[k]``,
    ``inv_sigma[k]`` are ``(ncol, nt, nsel, nb)``, ONE parameter vector fits every sun state, and the four launches become
    ``k_retrieve_apply``, ``crt_hip_g_dparam_series_f64`` into a :class:`LeafTangentSeries`, the :class:`SpectralNormalSeriesPlan` and
    ``crt_hip_lm_step_normal_f64`` with its one block.  ``cols.psi`` and ``bands.I_dr0 / I_df0`` are not read then.

    ``leaf_model``: as for :class:`RetrievalPlan` -- the parameters of a :class:`crt1d_amd.leaf_model.PlateLeafModel`, then the soil
    directions, ``"lai"``, ``"leaf"``; one launch more per :meth:`step` (and per :meth:`fitted`), ``crt_hip_plate_leaf_f64`` behind
    ``k_retrieve_apply``, with or without ``sun``.

    ``chain=nd``, ``inv_sigma_chain``: as for :class:`RetrievalPlan` -- the columns are (pixel, date) pairs and the closing call is
    ``crt_hip_lm_step_chain_f64`` on the block the normal plan wrote.  ``shared=``: as for :class:`RetrievalPlan` -- the closing call is
    ``crt_hip_lm_step_shared_f64``.

    ``evaluate="running"``: as for :class:`RetrievalPlan` -- the normal plan goes through its masked entry with ``status`` as the skip
    flags; :meth:`fitted` still evaluates every column.  ``"accepted"`` is a ValueError: the cost comes out of the kernel that forms the
    normal equations.

    ``prior_mean``, ``prior_precision``: as for :class:`RetrievalPlan` -- a Gaussian prior with a full precision matrix; the closing
    call becomes ``crt_hip_lm_prior_block_f64`` and ``crt_hip_lm_step_normal_f64`` on two blocks, the normal plan's sums and the
    prior's.  The match of a ``p0=`` :class:`LutTable` and ``lut_posterior()`` see the diagonal prior only."""

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, y, *, keys, inv_sigma=None, d_leaf_r=None, d_leaf_t=None, d_soil_r=None,
                 lai=True, leaf=False, p0=None, lo=None, hi=None, prior=None, inv_sigma_prior=None, sun=None, leaf_model=None, chain=None,
                 inv_sigma_chain=None, shared=None, evaluate="all", prior_mean=None, prior_precision=None, mu_s=0.501, tau_d_method="quad",
                 **options):
        keys, axis, o, levels = self._static(scheme, cols, bands, levels, y, keys=keys, inv_sigma=inv_sigma, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t,
                                             d_soil_r=d_soil_r, lai=lai, leaf=leaf, p0=p0, lo=lo, hi=hi, prior=prior,
                                             inv_sigma_prior=inv_sigma_prior, sun=sun, leaf_model=leaf_model, chain=chain,
                                             inv_sigma_chain=inv_sigma_chain, shared=shared, evaluate=evaluate, prior_mean=prior_mean,
                                             prior_precision=prior_precision, tau_d_method=tau_d_method, **options)
        self._construct(keys, axis, o, scheme, cols, bands, levels, sun, p0, lo, hi, prior, inv_sigma_prior, leaf_model, chain=chain,
                        inv_sigma_chain=inv_sigma_chain, shared=shared, evaluate=evaluate, prior_mean=prior_mean,
                        prior_precision=prior_precision, y=y, inv_sigma=inv_sigma, mu_s=mu_s, tau_d_method=tau_d_method)

    @classmethod
    def _static(cls, scheme, cols, bands, levels, y, *, keys, inv_sigma=None, d_leaf_r=None, d_leaf_t=None, d_soil_r=None, lai=True, leaf=False,
                p0=None, lo=None, hi=None, prior=None, inv_sigma_prior=None, sun=None, leaf_model=None, chain=None, inv_sigma_chain=None,
                shared=None, evaluate="all", prior_mean=None, prior_precision=None, mu_s=0.501, tau_d_method="quad", **options):
        """The constructor's arguments -> (keys in ``LEVEL_KEYS`` order, the parameter axis, the LM options, the normalized levels): every
        check that needs no device."""
        if evaluate not in EVALUATE_MODES:
            raise ValueError(f"evaluate must be one of {EVALUATE_MODES}, got {evaluate!r}")
        keys, axis = _spectral_static(scheme, y, keys, inv_sigma, tau_d_method, bands, sun, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t,
                                      d_soil_r=d_soil_r, lai=lai, leaf=leaf, leaf_model=leaf_model)
        o = _lm_options(lo, hi, axis.npar, options)
        _check_start(leaf_model, lo, hi, p0, prior, inv_sigma_prior)
        if isinstance(p0, LutTable):
            _check_lut_start(p0, axis.params, keys, True, y)
        _check_evaluate(evaluate, scheme, chain, True)
        levels = _spectral_shapes(cols, bands, levels, y, inv_sigma, len(keys), axis.npar, sun)
        _check_chain(chain, inv_sigma_chain, cols, axis.npar, _check_shared(shared, chain, axis.params, p0))
        _check_full_prior(prior_mean, prior_precision, chain, evaluate, cols, axis.npar)
        return keys, axis, o, levels

    _owns_sums = False  # (the normal plan's A, g and c2 are the block)

    def _inner(self, scheme, levels, sun, y, **kw):
        """The normal plan on the working tensors, which holds the observations (``fwd`` kept for :meth:`fitted`, not written by a step)."""
        a = (scheme, self.cols, self.bands) + (() if sun is None else (sun,)) + (levels, y)
        self.normal = (SpectralNormalPlan if sun is None else SpectralNormalSeriesPlan)(*a, fwd=True, **kw, **self._skip)
        self.normal.write_fwd = False
        self.y, self.inv_sigma = self.normal.y, self.normal.inv_sigma
        self.nrow = (1 if sun is None else sun.nt) * len(self.normal.levels) * self.bands.nb
        self._blk = (_lib.CrtLmNormalBlock * 1)(_lib.CrtLmNormalBlock(*[self.normal.out[k].data_ptr() for k in ("A", "g", "c2")]))
        return self.normal

    def step(self, stream=None):
        """One iteration on ``stream`` (default: torch's current stream): apply, tangent, normal equations, ``k_lm_step_normal``."""
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        self.nsteps += 1
        with torch.cuda.device(dev):
            self._evaluate(self._ap, s)
            self.normal(s)
            if self.nd is not None:  # the step of every pixel on the block the normal plan wrote
                self._step_chain(s)
                return self
            if self._pf is not None:  # two launches in place of the last: the sums of the prior, the step on both blocks
                self._step_full_prior(s)
                return self
            _lib.check(self.lib.crt_hip_lm_step_normal_f64(ctypes.byref(self._prob), self._blk, 1, ctypes.byref(self._state), s.cuda_stream),
                       "crt_hip_lm_step_normal_f64")
        return self

    def fitted(self, stream=None):
        """``{key: (ncol, [nt,] nsel, nb)}``: the model spectra at the accepted point ``p``, by one more evaluation there (copies).  The working
        inputs are left at ``p``; the next :meth:`step` applies its trial point again."""
        dev = self.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.device(dev):
            self.normal.write_fwd, self.normal.use_skip = True, False  # (every column, whatever ``evaluate``)
            try:
                self._evaluate(self._ap_p, s)
                self.normal(s)
            finally:
                self.normal.write_fwd, self.normal.use_skip = False, True
            with torch.cuda.stream(s):
                return {k: v.clone() for k, v in self.normal.out["fwd"].items()}


def retrieve_spectral(scheme, cols: Columns, bands: Bands, levels, y, *, keys, niter=20, posterior=False, **kw):
    """One-shot :class:`SpectralRetrievalPlan`: ``niter`` steps from ``p0``; what ``plan.result()`` returns, and ``"cov"``,
    ``plan.covariance()``.  ``posterior=True`` (``p0`` a :class:`LutTable`, else ValueError) adds ``"lut_mean"``, ``"lut_cov"`` and
    ``"lut_ess"``, what ``plan.lut_posterior()`` gives."""
    if posterior and not isinstance(kw.get("p0"), LutTable):
        raise ValueError("posterior=True needs a look-up table: p0= a LutTable (Model: lut=K)")
    SpectralRetrievalPlan._static(scheme, cols, bands, levels, y, keys=keys, **kw)  # (before any device is touched)
    with torch.cuda.device(cols.device):
        plan = SpectralRetrievalPlan(scheme, cols, bands, levels, y, keys=keys, **kw).run(niter)
        res = plan.result()
        res["cov"] = plan.covariance()
        if posterior:
            post = plan.lut_posterior()
            res.update({"lut_" + k: post[k].clone() for k in ("mean", "cov", "ess")})
    return res


# ---- the date-by-date retrieval: filter and Rauch-Tung-Striebel sweep (include_seq/crt1d_hip_lm_seq.h) -------------------------------------


def _check_sequential(nd, inv_sigma_dyn, ncol, plan_kwargs):
    """The arguments of a :class:`SequentialPlan` over ``ncol`` columns (or: over the :class:`Columns` ``ncol``), as far as no device is
    needed.  -> (npix, nd, npar)"""
    for name in ("sun", "chain", "shared"):
        if plan_kwargs.get(name) is not None:
            raise ValueError(f"{name}= is not served inside a SequentialPlan: every date is one unchained column of the inner plan")
    n = int(nd)
    if n != nd or n < 1:
        raise ValueError(f"nd must be the number of dates, an integer >= 1, got {nd!r}")
    ncol = ncol if isinstance(ncol, int) else ncol.ncol
    if ncol % n:
        raise ValueError(f"nd = {n} dates does not divide ncol = {ncol}: the columns are (pixel, date) pairs, pixel-major")
    npix = ncol // n
    for name in ("d_leaf_r", "d_leaf_t", "d_soil_r"):
        d = plan_kwargs.get(name)
        if d is not None and len(tuple(d.shape) if hasattr(d, "shape") else ()) == 3:
            raise ValueError(f"{name} per column is not served inside a SequentialPlan: give (ntan, nb), shared by all dates")
    axis = _ParamAxis(*[plan_kwargs.get(k) for k in ("d_leaf_r", "d_leaf_t", "d_soil_r")], plan_kwargs.get("lai", True),
                      plan_kwargs.get("leaf", False), plan_kwargs.get("leaf_model"))
    npar = axis.npar
    if inv_sigma_dyn is None:
        raise ValueError("a SequentialPlan needs inv_sigma_dyn (nd - 1, npar) or (npix, nd - 1, npar)")
    w = torch.as_tensor(inv_sigma_dyn)
    if tuple(w.shape) not in ((n - 1, npar), (npix, n - 1, npar)):
        raise ValueError(f"inv_sigma_dyn must be {(n - 1, npar)} or {(npix, n - 1, npar)}, got {tuple(w.shape)}")
    if not bool(((w >= 0) & (w < float("inf"))).all()):  # (false for NaN)
        raise ValueError("inv_sigma_dyn must be finite and >= 0 (0: nothing is handed over across that gap)")
    return npix, n, npar


class SequentialPlan:
    """The time series of a :class:`RetrievalPlan` with ``chain=nd``, solved date by date: a forward filter that retrieves one date at a
    time with the previous date's posterior as a full Gaussian prior, and a backward Rauch-Tung-Striebel sweep over the filtered dates
    (include_seq/crt1d_hip_lm_seq.h).  The on-chip state is that of ONE date: any ``nd`` is served, where the chained step ends at
    ``lm_chain_max_nd(npar)`` dates; and a new acquisition costs one date's retrieval, not a re-solve of the series.

    ``cols``, ``bands``, ``y``, ``inv_sigma``, ``p0``, ``prior``, ``inv_sigma_prior`` are per (pixel, date) column, pixel-major, exactly
    the inputs of a ``chain=nd`` plan; ``inv_sigma_dyn`` ``(nd - 1, npar)`` or ``(npix, nd - 1, npar)``, finite and ``>= 0``, has the
    meaning of ``inv_sigma_chain`` (0: nothing is handed over across that gap).  ``sensors`` given: the inner plan is an unchained
    :class:`RetrievalPlan` on ``npix`` columns; ``sensors=None``: a :class:`SpectralRetrievalPlan`.  ``plan_kwargs`` go to it (``keys``,
    directions ``(ntan, nb)``, ``lai``, ``leaf``, ``leaf_model``, ``lo``, ``hi``, the options, ``evaluate="running"``); ``sun=``,
    ``chain=`` and ``shared=`` are a ValueError.  ``prior_mean`` / ``prior_precision`` ``(npix, ..)`` apply to date 0 only.

    :meth:`assimilate` ``(t)``: the strided slices of date ``t`` are copied into the inner plan's bound tensors; for ``t > 0``
    ``crt_hip_lm_predict_f64`` pushes the stored ``A`` of date ``t - 1`` through the gap into the inner plan's ``prior_precision``, ``p``
    of date ``t - 1`` becomes ``prior_mean`` and the start; ``reset`` and ``niter`` steps; the state goes into the history arrays.
    :meth:`run` is ``assimilate(0 .. nd - 1)`` and the sweep (``crt_hip_lm_rts_f64``), with no host synchronisation anywhere.  For data
    that arrive later call :meth:`assimilate` one date at a time -- the strided inputs may be filled in place before the call -- and
    :meth:`smooth` for the sweep over the dates assimilated so far.

    On a linear problem filter plus sweep is the chained solve.  On a nonlinear one the filter linearises every date once, at its own
    filtered point, while the chain iterates all dates jointly: the two agree where every date (with the prior it inherits) determines
    the parameters; where only the whole series does, a date can settle in another minimum and hand it on -- use ``chain=`` there."""

    def __init__(self, scheme, cols: Columns, bands: Bands, levels, y, *, nd, inv_sigma_dyn, keys, sensors=None, niter=10, **plan_kwargs):
        npix, nd, npar = _check_sequential(nd, inv_sigma_dyn, cols, plan_kwargs)
        if isinstance(niter, bool) or int(niter) != niter or niter < 1:
            raise ValueError(f"niter must be an integer >= 1, got {niter!r}")
        if not isinstance(y, dict):
            raise TypeError("y must be a dict {key: (ncol, ...)}")
        self.npix, self.nd, self.npar, self.niter = npix, nd, npar, int(niter)
        dev, ncol = cols.device, cols.ncol
        kw = dict(plan_kwargs)
        per_date = lambda v: v.view(npix, nd, *v.shape[1:])  # noqa: E731
        full = lambda v, name: self._full(v, name, ncol, dev)  # noqa: E731
        Y = {k: full(v, f"y[{k!r}]") for k, v in y.items()}
        S = {k: full(v, f"inv_sigma[{k!r}]") for k, v in (kw.pop("inv_sigma", None) or {}).items()}
        pri = {k: _per_col(kw.pop(k), k, ncol, npar, dev) for k in ("prior", "inv_sigma_prior") if kw.get(k) is not None}
        for k in ("prior", "inv_sigma_prior"):
            kw.pop(k, None)
        p0 = kw.pop("p0", None)
        self._lut = isinstance(p0, LutTable)
        self._p0 = None if p0 is None or self._lut else per_date(_per_col(p0, "p0", ncol, npar, dev))
        pm, pp = kw.pop("prior_mean", None), kw.pop("prior_precision", None)
        self._own_prior = _check_full_prior(pm, pp, None, kw.get("evaluate", "all"), npix, npar)
        first = lambda v: None if v is None else per_date(v)[:, 0].clone()  # noqa: E731
        cfields = ("psi", "lai", "g_kind", "g_param", "mla", "g_at_psi", "g_table")
        c0 = Columns(*[first(getattr(cols, f)) for f in cfields])
        c0._tables_ok = getattr(cols, "_tables_ok", False)
        bfields = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")
        shared_bands = bands.col_stride(ncol) == 0
        b0 = bands if shared_bands else Bands(*[first(getattr(bands, f)) for f in bfields])
        inner_kw = dict(kw, keys=keys, inv_sigma={k: first(v) for k, v in S.items()} or None,
                        p0=p0 if self._lut else None if self._p0 is None else self._p0[:, 0].clone(),
                        prior_mean=pm if self._own_prior else torch.zeros((npix, npar), dtype=torch.float64, device=dev),
                        prior_precision=pp if self._own_prior else torch.zeros((npar, npar), dtype=torch.float64, device=dev),
                        **{k: first(v) for k, v in pri.items()})
        y0 = {k: first(v) for k, v in Y.items()}
        with torch.cuda.device(dev):
            if sensors is None:
                self.plan = SpectralRetrievalPlan(scheme, c0, b0, levels, y0, **inner_kw)
            else:
                self.plan = RetrievalPlan(scheme, c0, b0, levels, sensors, y0, **inner_kw)
        plan = self.plan
        self.params, self.lib = plan.params, plan.lib
        # what assimilate(t) copies: (the inner plan's bound tensor, the caller's array viewed (npix, nd, ...))
        feeds = []

        def feed(dsts, src):
            seen = set()
            for d in dsts:
                if d is not None and d.data_ptr() not in seen:
                    seen.add(d.data_ptr())
                    feeds.append((d, per_date(src)))

        for f in cfields:
            if getattr(cols, f) is not None:
                feed((getattr(plan.base_cols, f), getattr(plan.cols, f)), getattr(cols, f))
        if not shared_bands:
            for f in bfields:
                if getattr(bands, f) is not None:
                    feed((getattr(plan.base_bands, f),) + ((getattr(plan.bands, f),) if f in ("I_dr0", "I_df0") else ()), getattr(bands, f))
        for k in plan.keys:
            feed((plan.y[k],), Y[k])
            if k in S:
                feed((plan.inv_sigma[k],), S[k])
        for k, v in pri.items():
            feed((getattr(plan, k),), v)
        self._feeds = feeds
        self._start0 = plan._p0.clone()
        self._pm0 = plan.prior_mean.clone() if self._own_prior else None
        self._pp0 = plan.prior_precision.clone() if self._own_prior else None
        w = torch.as_tensor(inv_sigma_dyn, dtype=torch.float64).to(dev).contiguous()
        self.inv_sigma_dyn = w
        self._w3 = w if w.ndim == 3 else w[None]  # (npix or 1, nd - 1, npar)
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        ntri = npar * (npar + 1) // 2
        self._wgap, self._Aprev = torch.zeros((npix, npar), **f64), torch.zeros((npix, ntri), **f64)
        self._info1 = torch.zeros((npix,), **i32)
        self.p_filtered, self.A = torch.zeros((npix, nd, npar), **f64), torch.zeros((npix, nd, ntri), **f64)
        self.cost = torch.zeros((npix, nd), **f64)
        self.status, self.naccept, self.nreject, self.info_predict = (torch.zeros((npix, nd), **i32) for _ in range(4))
        self.p_smoothed, self.cov = torch.zeros((npix, nd, npar), **f64), torch.zeros((npix, nd, npar, npar), **f64)
        self.info_smooth = torch.zeros((npix,), **i32)
        self.ndone, self.nsmoothed = 0, 0

    @staticmethod
    def _full(v, name, ncol, dev):
        v = torch.as_tensor(v, dtype=torch.float64).to(dev).contiguous()
        if v.ndim < 1 or v.shape[0] != ncol:
            raise ValueError(f"{name} must have ncol = {ncol} leading rows, one per (pixel, date) column, got {tuple(v.shape)}")
        return v

    def assimilate(self, t, stream=None):
        """The filter step of date ``t`` (``t == 0``, or the date after the last one assimilated) on ``stream``; no host synchronisation."""
        if not 0 <= t < self.nd or t > self.ndone:
            raise ValueError(f"assimilate({t}): the next date is {self.ndone} of nd = {self.nd} (or 0, to start over)")
        plan, dev = self.plan, self.plan.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.device(dev), torch.cuda.stream(s):
            for dst, src in self._feeds:
                dst.copy_(src[:, t])
            if t > 0:  # the posterior of the date before, through the gap: the prior of this date
                self._wgap.copy_(self._w3[:, t - 1].expand_as(self._wgap))
                self._Aprev.copy_(self.A[:, t - 1])
                _lib.check(self.lib.crt_hip_lm_predict_f64(self.npix, self.npar, self._Aprev.data_ptr(), self._wgap.data_ptr(), self.npar,
                                                           plan.prior_precision.data_ptr(), self._info1.data_ptr(), s.cuda_stream),
                           "crt_hip_lm_predict_f64")
                self.info_predict[:, t].copy_(self._info1)
                plan.prior_mean.copy_(self.p_filtered[:, t - 1])
                plan.reset(self.p_filtered[:, t - 1])
            else:
                self.info_predict[:, 0].zero_()
                if self._own_prior:
                    plan.prior_mean.copy_(self._pm0)
                    plan.prior_precision.copy_(self._pp0)
                else:
                    plan.prior_precision.zero_()
                if self._lut:
                    plan.reset()
                else:
                    plan.reset(self._start0 if self._p0 is None else self._p0[:, 0])
                if not self._own_prior:
                    plan.prior_mean.copy_(plan.p)
            for _ in range(self.niter):
                plan.step(s)
            for hist, v in ((self.p_filtered, plan.p), (self.A, plan.A), (self.cost, plan.cost), (self.status, plan.status),
                            (self.naccept, plan.naccept), (self.nreject, plan.nreject)):
                hist[:, t].copy_(v)
        self.ndone, self.nsmoothed = t + 1, 0
        return self

    def smooth(self, stream=None):
        """The backward sweep (``crt_hip_lm_rts_f64``) over the dates assimilated so far; fewer than ``nd``: on compact copies."""
        m = self.ndone
        if m < 1:
            raise ValueError("smooth() needs at least one assimilated date")
        dev = self.plan.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.device(dev), torch.cuda.stream(s):
            whole = m == self.nd
            cut = lambda v, n=m: v if whole else v[:, :n].contiguous()  # noqa: E731
            p_f, A_f, w = cut(self.p_filtered), cut(self.A), cut(self._w3, m - 1)
            p_s, cov = (self.p_smoothed, self.cov) if whole else (torch.empty_like(p_f), self.cov.new_empty((self.npix, m, self.npar, self.npar)))
            chain = _lib.CrtLmChain(self.npix, m, 0 if w.shape[0] == 1 and self.npix != 1 or m == 1 else (m - 1) * self.npar,
                                    w.data_ptr() if m > 1 else None)
            _lib.check(self.lib.crt_hip_lm_rts_f64(ctypes.byref(chain), self.npar, p_f.data_ptr(), A_f.data_ptr(), p_s.data_ptr(), cov.data_ptr(),
                                                   self.info_smooth.data_ptr(), s.cuda_stream), "crt_hip_lm_rts_f64")
            if not whole:
                self.p_smoothed[:, :m].copy_(p_s)
                self.cov[:, :m].copy_(cov)
        self.nsmoothed = m
        return self

    def run(self, smooth=True, stream=None):
        """``assimilate(0 .. nd - 1)``, then the sweep (``smooth=False``: the filter only)."""
        for t in range(self.nd):
            self.assimilate(t, stream)
        return self.smooth(stream) if smooth else self

    def result(self, stream=None):
        """Copies over the ``m`` dates assimilated so far: ``p (npix, m, npar)`` -- smoothed if the sweep ran over them, else filtered --,
        ``p_filtered``, ``cov (npix, m, npar, npar)`` -- smoothed, else the inverse of every date's stored ``A``
        (``crt_hip_lm_covariance_f64``) --, ``cost``, ``status``, ``naccept``, ``nreject`` ``(npix, m)``; ``info``: ``(npix,)`` of the sweep
        (0, or 1 + the last date it could not pass) if it ran, else ``(npix, m)`` of the hand-overs (1: the date started without a
        prior); ``info_predict`` always; ``params``."""
        m, dev = self.ndone, self.plan.cols.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        smoothed = self.nsmoothed == m and m > 0
        with torch.cuda.device(dev), torch.cuda.stream(s):
            r = {k: getattr(self, k)[:, :m].clone() for k in ("p_filtered", "cost", "status", "naccept", "nreject", "info_predict")}
            if smoothed:
                r["p"], r["cov"], r["info"] = self.p_smoothed[:, :m].clone(), self.cov[:, :m].clone(), self.info_smooth.clone()
            else:
                A = self.A[:, :m].contiguous()
                cov = self.cov.new_empty((self.npix, m, self.npar, self.npar))
                if m:
                    _lib.check(self.lib.crt_hip_lm_covariance_f64(self.npix * m, self.npar, A.data_ptr(), cov.data_ptr(), s.cuda_stream),
                               "crt_hip_lm_covariance_f64")
                r["p"], r["cov"], r["info"] = r["p_filtered"].clone(), cov, r["info_predict"].clone()
        r["params"] = self.params
        return r


def retrieve_sequential(scheme, cols: Columns, bands: Bands, levels, y, *, nd, inv_sigma_dyn, keys, sensors=None, niter=10, smooth=True, **kw):
    """One-shot :class:`SequentialPlan`: the filter over the ``nd`` dates, the sweep (``smooth=False``: not), ``plan.result()``."""
    _check_sequential(nd, inv_sigma_dyn, cols, kw)  # (before any device is touched)
    return SequentialPlan(scheme, cols, bands, levels, y, nd=nd, inv_sigma_dyn=inv_sigma_dyn, keys=keys, sensors=sensors, niter=niter,
                          **kw).run(smooth).result()


class _LevelsAD(torch.autograd.Function):
    """``solve_levels`` with a backward pass: one :class:`LevelsGradPlan` call on the incoming ``d loss / d X``."""

    @staticmethod
    def forward(ctx, st, leaf_r, leaf_t, soil_r, lai_scale, g_param):
        ctx.st = st
        out = LevelsPlan(st["scheme"], st["cols"], st["bands"], st["levels"], keys=st["keys"], **st["kw"])()
        return tuple(out[k] for k in st["keys"])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        st = ctx.st
        names = ("leaf_r", "leaf_t", "soil_r", "lai", "leaf")
        need = ctx.needs_input_grad[1:]
        wrt = tuple(n for n, w in zip(names, need) if w)
        if not wrt:
            return (None,) * 6
        weights = {k: g.contiguous() for k, g in zip(st["keys"], grads)}
        g = LevelsGradPlan(st["scheme"], st["cols"], st["bands"], st["levels"], weights, wrt=wrt, **st["kw"])()
        res = []
        for n, t in zip(names, (st["bands"].leaf_r, st["bands"].leaf_t, st["bands"].soil_r, st["lai_scale"], st["cols"].g_param)):
            if n not in wrt:
                res.append(None)
            elif n in JAC_PARAMS:  # one spectrum shared by all columns: the sum of the columns' own responses
                res.append(g[n].sum(0, keepdim=True) if t.shape[0] == 1 and g[n].shape[0] != 1 else g[n])
            elif n == "lai":  # d / d lai_scale = (d / d ln LAI) / lai_scale
                res.append(g[n] / t)
            else:
                res.append(g[n])
        return (None, *res)


def solve_levels_ad(scheme, cols: Columns, bands: Bands, levels, *, keys=LEVEL_KEYS, lai_scale=None, mu_s=0.501, tau_d_method="quad"):
    """:func:`solve_levels` attached to torch's autograd graph: ``{key: (ncol, nsel, nb)}`` whose ``.backward()`` fills ``.grad`` of
    whichever of ``bands.leaf_r``, ``bands.leaf_t``, ``bands.soil_r``, ``lai_scale`` and ``cols.g_param`` require grad.

    ``lai_scale`` ``(ncol,)``: the solve runs on ``cols.lai * lai_scale[:, None]`` (``None``: on ``cols.lai``, bitwise
    :func:`solve_levels`).  The backward pass is one :class:`LevelsGradPlan` call on the incoming gradients (``GRAD_SCHEMES``: one
    kernel; n79, zq: composed), once-differentiable.  Shared ``(nb,)`` spectra receive the sum over the columns, ``lai_scale`` receives
    ``lai / lai_scale``, ``cols.g_param`` the gradient along ``leaf_tangent(cols, "param")``.  Spectra that require grad must be float64.
    There is no gradient with respect to ``I_dr0`` / ``I_df0``: a ValueError where they require grad, as is ``4s`` / ``zq_pa``."""
    LevelsGradPlan._check_options(LevelsGradPlan, scheme, tau_d_method)
    if scheme not in LevelsGradPlan._schemes:
        raise ValueError(LevelsGradPlan._no_kernel.format(scheme))
    keys = _level_keys(keys)
    for n in ("I_dr0", "I_df0"):
        if getattr(bands, n).requires_grad:
            raise ValueError(f"bands.{n} requires grad, but the level spectra have no gradient kernel with respect to it (they are linear in it)")
    if bands.dtype != torch.float64:
        raise TypeError("solve_levels_ad has no f32 storage form: bands must be float64")
    cols_f = cols
    if lai_scale is not None:
        lai_scale = _f64(lai_scale, "lai_scale")
        if lai_scale.shape != (cols.ncol,):
            raise ValueError("lai_scale must be (ncol,)")
        cols_f = Columns(cols.psi, cols.lai.detach() * lai_scale.detach()[:, None], cols.g_kind, cols.g_param, cols.mla, cols.g_at_psi, cols.g_table)
    st = dict(scheme=scheme, cols=cols_f, bands=bands, levels=normalize_levels(levels, cols.nz), keys=keys, lai_scale=lai_scale,
              kw=dict(mu_s=mu_s, tau_d_method=tau_d_method))
    with torch.cuda.device(cols.device):
        out = _LevelsAD.apply(st, bands.leaf_r, bands.leaf_t, bands.soil_r, lai_scale, cols.g_param)
    return dict(zip(keys, out))


# ---- the generalised plate model of leaf optics (include_ext/crt1d_hip_leafmodel.h) ---------------------------------------------------------

PLATE_LEAF_KEYS = ("leaf_r", "leaf_t", "d_leaf_r", "d_leaf_t")


def _plate_leaf_static(model, q, partials, out):
    """The checks of :func:`plate_leaf_optics` that touch no device.  -> ntan of the partial arrays"""
    from .leaf_model import PlateLeafModel

    if not isinstance(model, PlateLeafModel):
        raise TypeError("model must be a PlateLeafModel")
    _check_type(q, "q", (torch.float64,))
    if q.ndim != 2 or q.shape[1] != model.nm or q.shape[0] < 1:
        raise ValueError(f"q must be (ncol, nm) = (ncol, {model.nm}): {model.params}")
    ntan = model.nm
    if partials and out is not None and "d_leaf_r" in out:
        ntan = int(out["d_leaf_r"].shape[1]) if out["d_leaf_r"].ndim == 3 else -1
        if not model.nm <= ntan <= _lib.SENSJAC_MAX_NTAN:
            raise ValueError(f"the partial arrays must be (ncol, ntan, nb) with {model.nm} <= ntan <= {_lib.SENSJAC_MAX_NTAN}")
    return ntan


def plate_leaf_optics(model, q, *, partials=False, out=None, stream=None):
    """The plate model on the device (``crt_hip_plate_leaf_f64``, one launch): ``q (ncol, nm)`` float64 on the GPU, its columns named
    ``model.params`` = ``("N", contents...)`` -> ``(leaf_r, leaf_t)``, each ``(ncol, nb)``; ``partials=True``: ``(leaf_r, leaf_t,
    d_leaf_r, d_leaf_t)`` with the partial derivatives ``(ncol, nm, nb)`` in the order of ``model.params`` -- per-column directions
    as the Jacobian plans read them.  ``out``: a dict of arrays to write into under the keys ``PLATE_LEAF_KEYS``; its partial arrays
    may have ``ntan >= nm`` rows, of which the rows beyond ``nm`` are not touched.  ``N`` in [1, 4], contents ``>= 0``; ``k`` is clamped
    to [1e-6, 100] (the header).  A column's result is bitwise the same alone or in any batch, with or without the partials."""
    ntan = _plate_leaf_static(model, q, partials, out)
    q = _f64(q, "q")
    ncol, nb, dev = q.shape[0], model.nb, q.device
    shapes = {"leaf_r": (ncol, nb), "leaf_t": (ncol, nb)}
    if partials:
        shapes.update({"d_leaf_r": (ncol, ntan, nb), "d_leaf_t": (ncol, ntan, nb)})
    o = _outputs(shapes, out, torch.float64, dev, "out[{!r}]", lacks=True)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev) if stream is None else stream
        m = model.c_struct(ncol, dev)
        d = [o[k].data_ptr() if partials else None for k in ("d_leaf_r", "d_leaf_t")]
        _lib.check(_lib.load().crt_hip_plate_leaf_f64(ctypes.byref(m), q.data_ptr(), model.nm, o["leaf_r"].data_ptr(), o["leaf_t"].data_ptr(),
                                                       ntan if partials else 0, *d, s.cuda_stream), "crt_hip_plate_leaf_f64")
    return tuple(o[k] for k in shapes)


class _PlateLeafAD(torch.autograd.Function):
    """``plate_leaf_optics`` with a backward pass: the incoming gradients contracted with the stored partials."""

    @staticmethod
    def forward(ctx, model, q):
        leaf_r, leaf_t, d_r, d_t = plate_leaf_optics(model, q.detach(), partials=True)
        ctx.save_for_backward(d_r, d_t)
        return leaf_r, leaf_t

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_r, g_t):
        d_r, d_t = ctx.saved_tensors
        return None, torch.einsum("cb,cjb->cj", g_r, d_r) + torch.einsum("cb,cjb->cj", g_t, d_t)


def plate_leaf_ad(model, q):
    """:func:`plate_leaf_optics` attached to torch's autograd graph: ``(leaf_r, leaf_t)`` whose ``.backward()`` fills ``q.grad`` with
    the incoming gradients contracted with the model's partials (once-differentiable).  With :func:`solve_levels_ad` behind it -- a
    :class:`Bands` of these spectra -- a torch optimiser fits ``q`` directly."""
    _plate_leaf_static(model, q, False, None)
    with torch.cuda.device(q.device):
        return _PlateLeafAD.apply(model, q)


def _leaf_model_ntan(leaf_model, d_leaf_r, d_leaf_t, d_soil_r):
    """``ntan = nm + ns`` of a retrieval with a leaf model: the model's parameters, then the ``ns`` soil directions.  No device."""
    from .leaf_model import PlateLeafModel

    if not isinstance(leaf_model, PlateLeafModel):
        raise TypeError("leaf_model must be a PlateLeafModel")
    if d_leaf_r is not None or d_leaf_t is not None:
        raise ValueError("d_leaf_r / d_leaf_t and leaf_model exclude each other: the model writes the leaf directions")
    ns = _sensjac_ntan(None, None, d_soil_r)
    if leaf_model.nm + ns > _lib.SENSJAC_MAX_NTAN:
        raise ValueError(f"nm + ns = {leaf_model.nm} + {ns} model parameters and soil directions; one call takes {_lib.SENSJAC_MAX_NTAN}")
    return leaf_model.nm + ns


def _leaf_model_start(leaf_model, lo, hi, p0):
    """The bounds and the starting point a leaf model needs.  No device."""
    leaf_model.check_bounds(lo, hi)
    if p0 is None:
        raise ValueError("a leaf_model needs p0: the model has no default starting point")


class _PlateLeafBinding:
    """What a retrieval plan owns for its ``leaf_model``: the per-column direction arrays ``(ncol, ntan, nb)`` with ``ntan = nm + ns``
    -- leaf rows ``0 .. nm - 1`` written by ``k_plate_leaf`` at every evaluation and ``nm ..`` zero, soil rows ``0 .. nm - 1`` zero and
    ``nm ..`` the user's directions -- and the launch that writes the working leaf spectra and those rows from a parameter array."""

    def __init__(self, model, axis, ncol, nb, device):
        """``axis``: the plan's :class:`_ParamAxis` (static half), which knows ``ntan`` and the user's soil directions."""
        if model.nb != nb:
            raise ValueError(f"the leaf model has {model.nb} bands, the bands {nb}")
        self.model, self.nm, self.ns, self.ntan = model, model.nm, axis.ntan - model.nm, axis.ntan
        ns = self.ns
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=device)  # noqa: E731
        self.d_leaf_r, self.d_leaf_t = new(ncol, self.ntan, nb), new(ncol, self.ntan, nb)
        self.d_soil_r = None
        if ns:
            self.d_soil_r = new(ncol, self.ntan, nb)
            self.d_soil_r[:, self.nm:] = _jvp_direction(axis.given["soil_r"], "d_soil_r", ncol, nb, device)
        self.dirs = {"leaf_r": self.d_leaf_r, "leaf_t": self.d_leaf_t, **({"soil_r": self.d_soil_r} if ns else {})}  # the inner plan's
        # what k_retrieve_apply reads: no leaf directions (the base spectra are copied), the soil directions or, with none, a shared zero
        # array -- an axis of its own, which keeps that array
        self._apply = _ParamAxis(d_soil_r=self.d_soil_r if ns else new(self.ntan, nb), lai=False).bind(ncol, nb, device)
        self.apply_dirs = self._apply.c_dirs
        self._m = model.c_struct(ncol, device)
        self._keep = model.tensors(device)

    def bound_to(self, plan):
        """The inner Jacobian / normal plan must read the arrays this binding writes."""
        for n in ("leaf_r", "leaf_t"):
            assert plan.dirs[n].data_ptr() == getattr(self, "d_" + n).data_ptr()

    def launch(self, lib, p_ptr, npar, bands, h):
        _lib.check(lib.crt_hip_plate_leaf_f64(ctypes.byref(self._m), p_ptr, npar, bands.leaf_r.data_ptr(), bands.leaf_t.data_ptr(), self.ntan,
                                              self.d_leaf_r.data_ptr(), self.d_leaf_t.data_ptr(), h), "crt_hip_plate_leaf_f64")


# ---- the look-up-table start of the retrievals (include_lut/crt1d_hip_lut.h) --------------------------------------------------------------

LUT_MAX_BEST = _lib.LUT_MAX_BEST
_HALTON_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29)  # one per parameter, RETRIEVE_MAX_NPAR of them


def lut_sample(lo, hi, ncand, *, include=None):
    """``ncand`` candidate parameter vectors in the box ``[lo, hi]`` (each ``(npar,)``, finite): a NumPy array ``(ncand, npar)`` float64.
    The rows of ``include`` (``(n, npar)`` or ``(npar,)``, e.g. the default starting point; taken as they are) come first; the rest is
    the Halton sequence (bases 2, 3, 5, ..; from its index 1) scaled to the box -- deterministic, no random-number generator."""
    import numpy as np

    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.ndim != 1 or lo.shape != hi.shape or not 1 <= lo.shape[0] <= _lib.RETRIEVE_MAX_NPAR:
        raise ValueError(f"lo and hi must be (npar,) with npar in 1 .. {_lib.RETRIEVE_MAX_NPAR}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("a look-up table needs finite bounds lo and hi")
    if (lo > hi).any():
        raise ValueError("lo must not exceed hi")
    npar = lo.shape[0]
    inc = np.empty((0, npar)) if include is None else np.atleast_2d(np.asarray(include, dtype=np.float64))
    if inc.ndim != 2 or inc.shape[1] != npar:
        raise ValueError(f"include must be (n, npar) or (npar,) with npar = {npar}")
    n = int(ncand) - inc.shape[0]
    if int(ncand) < 1 or n < 0:
        raise ValueError("ncand must be >= 1 and at least the number of rows of include")
    u = np.empty((n, npar))
    for j in range(npar):
        b, f, r, k = _HALTON_BASES[j], 1.0, np.zeros(n), np.arange(1, n + 1)
        while k.any():  # the radical inverse of the index in base b
            f /= b
            r += f * (k % b)
            k //= b
        u[:, j] = r
    return np.concatenate([inc, np.clip(lo + u * (hi - lo), lo, hi)])


def _table_axes(spectral, series):
    return "(ncol, " + ("nt, " if series else "") + ("nsel, nb)" if spectral else "nsel, nsens)")


class LutTable:
    """A look-up table of a retrieval: the model evaluated once at ``K`` candidate parameter vectors on ONE template canopy.  ``q (K,
    npar)`` the candidates and ``m[key] (K, nrow)`` the model's values (device tensors), ``params`` the names of the columns of ``q``,
    ``keys``, ``nrow``, ``shape`` (what ``nrow`` flattens: ``([nt,] nsel, nsens)`` or ``([nt,] nsel, nb)``), ``scheme`` and ``spectral``
    (the rows are level spectra, not sensor-band sums).  Made by :meth:`build`; matched by :class:`LutMatchPlan`; taken as ``p0=`` by
    :class:`RetrievalPlan` and :class:`SpectralRetrievalPlan`."""

    def __init__(self, q, m, *, params, keys, shape, scheme, spectral, p_default=None):
        self.q, self.m, self.params, self.keys, self.shape = q, m, tuple(params), tuple(keys), tuple(shape)
        self.p_default = p_default  # where a plan started from this table puts a column without an eligible candidate (None: the plan's)
        self.scheme, self.spectral = scheme, bool(spectral)
        self.nrow = int(torch.Size(self.shape).numel())

    @property
    def ncand(self):
        return self.q.shape[0]

    @property
    def npar(self):
        return self.q.shape[1]

    @classmethod
    def _static(cls, scheme, cols, bands, levels, q, *, keys, sensors=None, sun=None, d_leaf_r=None, d_leaf_t=None, d_soil_r=None, lai=True,
                leaf=False, leaf_model=None, mu_s=0.501, tau_d_method="quad", chunk=None):
        """The arguments of :meth:`build` -> (keys, the parameter axis, the candidates as a host array, the chunk): every check that needs
        no device, through the ``_static`` of the plan the table is for."""
        import numpy as np

        spectral = sensors is None
        _SolvePlan._check_options(_SolvePlan, scheme, tau_d_method)
        served = SPECTRAL_RETRIEVE_SCHEMES if spectral else RETRIEVE_SCHEMES
        if scheme not in served:
            raise ValueError(f"scheme {scheme!r} has no {'spectral ' if spectral else ''}look-up table; served: " + ", ".join(served))
        keys = _level_keys(keys)
        axis_kw = dict(d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t, d_soil_r=d_soil_r, lai=lai, leaf=leaf, leaf_model=leaf_model)
        axis = _ParamAxis(**axis_kw)
        for what, n in (("cols", getattr(cols, "ncol", 1)), ("bands", getattr(bands, "_shape", (1,))[0]), ("sun", getattr(sun, "ncol", 1))):
            if n != 1:
                raise ValueError(f"a look-up table is built on ONE template column: {what} has {n}")
        qh = np.asarray(q.detach().cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float64)
        if qh.ndim != 2 or qh.shape[0] < 1 or qh.shape[1] != axis.npar:
            raise ValueError(f"q must be (K, npar) with K >= 1 and npar = {axis.npar} for the parameters {axis.params}, got {qh.shape}")
        if not np.isfinite(qh).all():
            raise ValueError("q must be finite")
        if chunk is not None and int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        chunk = min(qh.shape[0], 1024 if chunk is None else int(chunk))
        start = dict(p0=qh[:1], lo=qh.min(0), hi=qh.max(0))  # (the candidates' own box: a leaf model checks N and the contents on it)
        if spectral:
            fake = {k: np.broadcast_to(0.0, (1,) * (3 if sun is None else 4)) for k in keys}
            keys, axis = _spectral_static(scheme, fake, keys, None, tau_d_method, bands, sun, **axis_kw)
            _check_start(leaf_model, start["lo"], start["hi"], start["p0"], None, None)
        else:
            keys, axis, _ = RetrievalPlan._static(scheme, cols, bands, levels, sensors, dict.fromkeys(keys), keys=keys, sun=sun, **axis_kw,
                                                  **start, tau_d_method=tau_d_method)
        return keys, axis, qh, chunk

    @classmethod
    def build(cls, scheme, cols: Columns, bands: Bands, levels, q, *, keys, sensors=None, sun=None, d_leaf_r=None, d_leaf_t=None,
              d_soil_r=None, lai=True, leaf=False, leaf_model=None, mu_s=0.501, tau_d_method="quad", chunk=None):
        """Evaluate the model at the candidates ``q (K, npar)`` (e.g. :func:`lut_sample`) on the template ``cols``, ``bands``, ``sun``: ONE
        column each -- anything else is a ValueError.  All columns later matched against the table share that template (sun angle or
        series, base LAI profile, base spectra, illumination) and differ in their observations; several classes of columns are several
        tables.  With ``sensors`` the rows are the sensor-band sums a :class:`RetrievalPlan` compares (``RETRIEVE_SCHEMES``); without, the
        level spectra of ``SpectralRetrievalPlan.fitted()`` (``SPECTRAL_RETRIEVE_SCHEMES``).  The parameter axis (``d_*``, ``lai``,
        ``leaf``, ``leaf_model``) is that of the plans.  There is no second apply path: the matching retrieval plan is built on the
        template replicated to ``chunk`` columns (default ``min(K, 1024)``) and restarted at every chunk of ``q``; row ``k`` is bitwise what
        that plan evaluates at ``q[k]`` alone, for any ``chunk``."""
        kw = dict(keys=keys, sensors=sensors, sun=sun, d_leaf_r=d_leaf_r, d_leaf_t=d_leaf_t, d_soil_r=d_soil_r, lai=lai, leaf=leaf,
                  leaf_model=leaf_model, mu_s=mu_s, tau_d_method=tau_d_method)
        keys, axis, qh, chunk = cls._static(scheme, cols, bands, levels, q, chunk=chunk, **kw)
        spectral, dev, K = sensors is None, cols.device, qh.shape[0]
        rep = lambda v: None if v is None else v.expand(chunk, *v.shape[1:]).contiguous()  # noqa: E731
        tcols = Columns(rep(cols.psi), rep(cols.lai), rep(cols.g_kind), rep(cols.g_param), rep(cols.mla), rep(cols.g_at_psi), rep(cols.g_table))
        tsun = None if sun is None else type(sun)(rep(sun.psi), sun.I_dr0, sun.I_df0, rep(sun.g_at_psi))
        kw.pop("sensors")
        kw["sun"] = tsun
        with torch.cuda.device(dev):
            qd = torch.as_tensor(qh, device=dev).contiguous()
            start = dict(p0=qd[:1], lo=qh.min(0), hi=qh.max(0)) if leaf_model is not None else {}
            # zero observations of the plans' shapes: the table rows do not depend on them
            nts, nsel = () if sun is None else (sun.nt,), len(normalize_levels(levels, cols.nz))
            zeros = lambda n: {k: torch.zeros((chunk, *nts, nsel, n), dtype=torch.float64, device=dev) for k in keys}  # noqa: E731
            if spectral:
                plan = SpectralRetrievalPlan(scheme, tcols, bands, levels, zeros(bands.nb), **kw, **start)
            else:
                plan = RetrievalPlan(scheme, tcols, bands, levels, sensors, zeros(sensors.nsens), **kw, **start)
            s = torch.cuda.current_stream(dev)
            m = None
            for i0 in range(0, K, chunk):
                n = min(chunk, K - i0)
                qc = qd[i0:i0 + n] if n == chunk else torch.cat([qd[i0:], qd[-1:].expand(chunk - n, -1)])  # (padded with the last row)
                plan.reset(p0=qc)
                if spectral:
                    vals = plan.fitted(s)
                else:
                    plan._evaluate(plan._ap, s)
                    plan.fwd(s, flags=0)  # (its own precompute)
                    vals = plan.fwd.out
                if m is None:
                    shape = tuple(vals[keys[0]].shape[1:])
                    m = {k: torch.empty((K, int(torch.Size(shape).numel())), dtype=torch.float64, device=dev) for k in keys}
                for k in keys:
                    m[k][i0:i0 + n] = vals[k].reshape(chunk, -1)[:n]
        return cls(qd, m, params=axis.params, keys=keys, shape=shape, scheme=scheme, spectral=spectral)


def _check_lut_start(table, params, keys, spectral, y):
    """A :class:`LutTable` given as ``p0`` against the plan it starts: the parameter axis, the keys, the kind, and its rows against the
    observations ``y`` (whose shape the plan holds to its own).  No device."""
    import numpy as np

    if tuple(table.params) != tuple(params):
        raise ValueError(f"the table has the parameters {table.params}, the plan {tuple(params)}")
    if tuple(table.keys) != tuple(keys):
        raise ValueError(f"the table has the keys {table.keys}, the plan {tuple(keys)}")
    if table.spectral != spectral:
        kinds = ("level spectra (built without sensors)", "sensor-band sums (built with sensors)")
        raise ValueError(f"the table holds {kinds[not table.spectral]}, the plan compares {kinds[not spectral]}")
    for k in keys:
        if tuple(np.shape(y[k])[1:]) != table.shape:
            raise ValueError(f"the table's rows are {table.shape} per candidate, y[{k!r}] is {tuple(np.shape(y[k]))}")


class _LutObsPlan:
    """What the plans on a :class:`LutTable` share: the device-free checks of the table and the observations, and the structs
    ``crt_lut_table`` / ``crt_lut_obs`` bound to the tensors."""

    @staticmethod
    def _check_table(table, y, inv_sigma):
        """-> how the messages call the observations' shape"""
        if not isinstance(table, LutTable):
            raise TypeError("table must be a LutTable")
        if len(table.keys) > _lib.LM_MAX_BLOCKS:
            raise ValueError(f"a match takes {_lib.LM_MAX_BLOCKS} keys at most")
        axes = _table_axes(table.spectral, len(table.shape) == 3)
        _check_obs(y, inv_sigma, table.keys, axes, 1 + len(table.shape))
        return axes

    @staticmethod
    def _check_rest(table, y, inv_sigma, prior, inv_sigma_prior, ksplit, axes):
        import numpy as np

        if not 0 <= int(ksplit) <= _lib.LUT_MAX_KSPLIT:
            raise ValueError(f"ksplit must be in 0 .. {_lib.LUT_MAX_KSPLIT}, got {ksplit}")
        if (prior is None) != (inv_sigma_prior is None):
            raise ValueError("prior and inv_sigma_prior go together")
        for name, d in (("y", y), ("inv_sigma", inv_sigma or {})):
            for k, v in d.items():
                shape = tuple(v.shape) if hasattr(v, "shape") else np.shape(v)
                if shape[1:] != table.shape or shape[0] < 1:
                    raise ValueError(f"{name}[{k!r}] must be {axes} = (ncol, {str(table.shape)[1:-1]}), got {shape}")

    def _bind(self, table, y, inv_sigma, prior, inv_sigma_prior, axes):
        """The observations on the table's device and the two input structs."""
        self.lib, self.table = _lib.load(), table
        dev, keys, npar = table.q.device, table.keys, table.npar

        def obs(v, name, ncol=None):
            v = torch.as_tensor(v, dtype=torch.float64).to(dev).contiguous()
            if tuple(v.shape[1:]) != table.shape or v.ndim < 2 or (ncol is not None and v.shape[0] != ncol) or v.shape[0] < 1:
                raise ValueError(f"{name} must be {axes} = ({'ncol' if ncol is None else ncol}, {str(table.shape)[1:-1]}), got {tuple(v.shape)}")
            return v

        self.y = {keys[0]: obs(y[keys[0]], f"y[{keys[0]!r}]")}
        ncol = self.ncol = self.y[keys[0]].shape[0]
        self.y.update({k: obs(y[k], f"y[{k!r}]", ncol) for k in keys[1:]})
        self.inv_sigma = {k: obs(inv_sigma[k], f"inv_sigma[{k!r}]", ncol) for k in keys if inv_sigma is not None and k in inv_sigma}
        self.prior = None if prior is None else _per_col(prior, "prior", ncol, npar, dev)
        self.inv_sigma_prior = None if prior is None else _per_col(inv_sigma_prior, "inv_sigma_prior", ncol, npar, dev)
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        pad = lambda v: v + [None] * (_lib.LM_MAX_BLOCKS - len(v))  # noqa: E731
        nblk = len(keys)
        self._t = _lib.CrtLutTable(table.ncand, npar, nblk, (ctypes.c_int32 * _lib.LM_MAX_BLOCKS)(*[table.nrow] * nblk),
                                   ptr(table.q), (ctypes.c_void_p * _lib.LM_MAX_BLOCKS)(*pad([ptr(table.m[k]) for k in keys])))
        self._o = _lib.CrtLutObs(ncol, (ctypes.c_void_p * _lib.LM_MAX_BLOCKS)(*pad([ptr(self.y[k]) for k in keys])),
                                 (ctypes.c_void_p * _lib.LM_MAX_BLOCKS)(*pad([ptr(self.inv_sigma.get(k)) for k in keys])),
                                 ptr(self.prior), ptr(self.inv_sigma_prior))

    def last_kernel(self):
        return self.lib.crt_hip_last_kernel().decode()


class LutMatchPlan(_LutObsPlan):
    """The best ``nbest`` candidates of a :class:`LutTable` for every column, in one kernel pass (``crt_hip_lut_match_f64``): the weighted
    misfit of the observations ``y[k] (ncol, *table.shape)`` (``inv_sigma[k]`` the same shape; ``None`` / a missing key: ones; an entry 0:
    not observed, its ``y`` may be NaN) and the prior ``prior`` / ``inv_sigma_prior`` (``(ncol, npar)`` or ``(npar,)``, both or neither)
    against every table row, under the cost contract of the Levenberg-Marquardt step, with the selection fused: neither the costs ``ncol x
    K`` nor the residuals are written.  Everything is bound at construction and the workspace allocated once; tensors on the table's
    device are read where they lie at every call.  ``plan()`` is one C call and returns ``{"index" (ncol, nbest) int32, "cost" (ncol,
    nbest), "p" (ncol, npar)}``: the candidates in ascending (cost, index), ``-1`` / ``+inf`` where fewer than ``nbest`` have a cost below
    ``+inf``, and ``p = q[index[:, 0]]`` -- filled at every call with ``p_default`` (``(ncol, npar)`` or ``(npar,)``; default NaN) first,
    which a column without any eligible candidate keeps.  ``ksplit``: how many workgroups share the candidates of 64 columns (0: automatic);
    it changes no bit of the result."""

    def __init__(self, table, y, *, inv_sigma=None, prior=None, inv_sigma_prior=None, nbest=1, p_default=None, ksplit=0):
        axes = self._static(table, y, inv_sigma=inv_sigma, prior=prior, inv_sigma_prior=inv_sigma_prior, nbest=nbest, ksplit=ksplit)
        self.nbest = int(nbest)
        self._bind(table, y, inv_sigma, prior, inv_sigma_prior, axes)
        dev, npar, ncol = table.q.device, table.npar, self.ncol
        self.index = torch.full((ncol, self.nbest), -1, dtype=torch.int32, device=dev)
        self.cost = torch.full((ncol, self.nbest), float("inf"), dtype=torch.float64, device=dev)
        fill = torch.full((npar,), float("nan"), dtype=torch.float64) if p_default is None else p_default
        self._p_default = _per_col(fill, "p_default", ncol, npar, dev).clone()
        self.p = self._p_default.clone()
        need = int(self.lib.crt_hip_lut_match_workspace_bytes(ncol, table.ncand, self.nbest))
        self.workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        self._out = _lib.CrtLutOut(self.nbest, int(ksplit), self.index.data_ptr(), self.cost.data_ptr(), self.p.data_ptr())

    @staticmethod
    def _static(table, y, *, inv_sigma=None, prior=None, inv_sigma_prior=None, nbest=1, p_default=None, ksplit=0):
        """Every check that needs no device.  -> how the messages call the observations' shape"""
        axes = _LutObsPlan._check_table(table, y, inv_sigma)
        if not 1 <= int(nbest) <= LUT_MAX_BEST:
            raise ValueError(f"nbest must be in 1 .. {LUT_MAX_BEST}, got {nbest}")
        _LutObsPlan._check_rest(table, y, inv_sigma, prior, inv_sigma_prior, ksplit, axes)
        return axes

    def __call__(self, stream=None):
        dev = self.table.q.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.device(dev):
            with torch.cuda.stream(s):
                self.p.copy_(self._p_default)  # (a column that has lost its last eligible candidate since the call before falls back)
            _lib.check(self.lib.crt_hip_lut_match_f64(ctypes.byref(self._t), ctypes.byref(self._o), ctypes.byref(self._out),
                                                      self.workspace.data_ptr(), self.workspace.numel(), s.cuda_stream), "crt_hip_lut_match_f64")
        return {"index": self.index, "cost": self.cost, "p": self.p}


def lut_match(table, y, **kw):
    """One-shot :class:`LutMatchPlan`: ``{"index", "cost", "p"}``."""
    LutMatchPlan._static(table, y, **kw)  # (before any device is touched)
    with torch.cuda.device(table.q.device):
        return LutMatchPlan(table, y, **kw)()


class LutPosteriorPlan(_LutObsPlan):
    """The Bayesian look-up-table estimate of every column (``crt_hip_lut_posterior_f64``, include_post/crt1d_hip_lut_posterior.h): the
    mean and the covariance of the ``K`` candidates of a :class:`LutTable` weighted by ``exp(-(cost - cmin) / temperature)``, with the
    effective sample size -- a value with a global uncertainty where the Levenberg-Marquardt covariance describes one basin.  ``table``,
    ``y``, ``inv_sigma``, ``prior``, ``inv_sigma_prior`` as for :class:`LutMatchPlan` (the cost is the same, bit for bit).
    ``temperature``: a float (finite, > 0) or an ``(ncol,)`` tensor; a column whose value is not finite or not > 0 gets no result.  With
    costs that are half sums of squared residuals in units of the noise, 1 is the Gaussian likelihood.  ``ksplit``: the parts the candidates
    are summed in (0: automatic, a function of ``ncol`` and ``K``); the sums are formed in a fixed order for a given ``ksplit``, so a fixed
    value keeps a column's bits across batch sizes, and different values agree within rounding.  ``plan()`` is one C call and returns
    ``{"mean" (ncol, npar), "cov" (ncol, npar, npar), "ess" (ncol,), "wsum" (ncol,), "index" (ncol,) int32, "cost" (ncol,)}``: ``index`` /
    ``cost`` the best candidate (what ``lut_match`` gives), ``wsum`` the sum of the weights (the best one's is 1) and ``ess = wsum^2 / sum
    w^2`` the effective number of candidates behind the estimate -- a few means the table is too coarse for the noise.  ``mean`` and
    ``cov`` are filled with NaN before every call; a column without an eligible candidate keeps that fill and gets ``index -1``, ``cost
    +inf``, ``wsum = ess = 0``.

    A temperature taken from the best cost (e.g. the reduced chi-square) needs no host synchronisation::

        best = lut_match(table, y, inv_sigma=w)["cost"][:, 0]
        post = lut_posterior(table, y, inv_sigma=w, temperature=torch.clamp(2.0 * best / nobs, min=1.0))
    """

    def __init__(self, table, y, *, inv_sigma=None, prior=None, inv_sigma_prior=None, temperature=1.0, ksplit=0):
        axes = self._static(table, y, inv_sigma=inv_sigma, prior=prior, inv_sigma_prior=inv_sigma_prior, temperature=temperature,
                            ksplit=ksplit)
        self._bind(table, y, inv_sigma, prior, inv_sigma_prior, axes)
        dev, npar, ncol = table.q.device, table.npar, self.ncol
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        self.index = torch.full((ncol,), -1, dtype=torch.int32, device=dev)
        self.cost, self.mean, self.cov, self.wsum, self.ess = new(ncol), new(ncol, npar), new(ncol, npar, npar), new(ncol), new(ncol)
        self.temperature = None
        if isinstance(temperature, torch.Tensor):  # ((ncol,): _static)
            self.temperature = temperature.to(device=dev, dtype=torch.float64).contiguous()
        need = int(self.lib.crt_hip_lut_posterior_workspace_bytes(ncol, table.ncand, npar, int(ksplit)))
        self.workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        self._out = _lib.CrtLutPosteriorOut(1.0 if self.temperature is not None else float(temperature),
                                            None if self.temperature is None else self.temperature.data_ptr(), int(ksplit),
                                            *[v.data_ptr() for v in (self.index, self.cost, self.mean, self.cov, self.wsum, self.ess)])

    @staticmethod
    def _static(table, y, *, inv_sigma=None, prior=None, inv_sigma_prior=None, temperature=1.0, ksplit=0):
        """Every check that needs no device.  -> how the messages call the observations' shape"""
        import math

        axes = _LutObsPlan._check_table(table, y, inv_sigma)
        if isinstance(temperature, torch.Tensor):
            if temperature.ndim != 1 or not temperature.dtype.is_floating_point:
                raise ValueError(f"temperature must be a number or a floating-point (ncol,) tensor, got {tuple(temperature.shape)}")
        elif isinstance(temperature, bool) or not isinstance(temperature, (int, float)):
            raise TypeError("temperature must be a number or an (ncol,) tensor")
        elif not (math.isfinite(temperature) and temperature > 0):
            raise ValueError(f"temperature must be finite and > 0, got {temperature}")
        _LutObsPlan._check_rest(table, y, inv_sigma, prior, inv_sigma_prior, ksplit, axes)
        ncol = y[table.keys[0]].shape[0]
        if isinstance(temperature, torch.Tensor) and temperature.shape[0] != ncol:
            raise ValueError(f"temperature must be a number or (ncol,) = ({ncol},), got {tuple(temperature.shape)}")
        return axes

    def __call__(self, stream=None):
        dev = self.table.q.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.device(dev):
            with torch.cuda.stream(s):
                self.mean.fill_(float("nan"))
                self.cov.fill_(float("nan"))
            _lib.check(self.lib.crt_hip_lut_posterior_f64(ctypes.byref(self._t), ctypes.byref(self._o), ctypes.byref(self._out),
                                                          self.workspace.data_ptr(), self.workspace.numel(), s.cuda_stream),
                       "crt_hip_lut_posterior_f64")
        return {k: getattr(self, k) for k in ("mean", "cov", "ess", "wsum", "index", "cost")}


def lut_posterior(table, y, **kw):
    """One-shot :class:`LutPosteriorPlan`: ``{"mean", "cov", "ess", "wsum", "index", "cost"}``."""
    LutPosteriorPlan._static(table, y, **kw)  # (before any device is touched)
    with torch.cuda.device(table.q.device):
        return LutPosteriorPlan(table, y, **kw)()
