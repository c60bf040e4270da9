"""
``Model`` -- the reference's convenience driver (``crt1d/model.py:49-447``) on top of the MI355X solvers.

Same entry points and bookkeeping for the hot path: ``Model(scheme, nlayers, **p)``, ``update_p``,
``assign_scheme``, ``run(**solver_options)`` (``model.py:296-320``), ``calc_absorption()``
(``model.py:327-336,573-647``), ``out`` / ``out_extra`` / ``absorption``.  ``to_dataset()`` returns the reference's
output dataset as a plain container (``to_xr()`` converts it when xarray is installed); plots are out of scope.

Multi-column use (the reference's ``run_sensitivity`` is a ``NotImplementedError`` stub, ``model.py:650-664``):
:func:`run_columns` solves many independent canopies in one launch.
"""

import copy
import pprint
import traceback
import warnings

import numpy as np

from . import canopy
from .canopy import CANOPY_DESCRIPTION_KEYS, CanopyDescription
from .cases import load_default_case
from .solvers import AVAILABLE_SCHEMES, RET_KEYS_ALL_SCHEMES
from .variables import VMD

__all__ = ("Model", "Dataset", "run_columns")

_FALLBACK_SCHEME = "2s"
_SOLUTION_VARS = ("I_dr", "I_df_d", "I_df_u", "F")
_SCHEME_SUFFIX = "_scheme"


class Model:
    """One canopy, one scheme: holds the case, runs the scheme's solver on the GPU, keeps the results.

    State: ``_p`` (inputs + what :func:`crt1d_amd.canopy.derive` adds), ``scheme`` (registry entry), ``out`` (the four contract
    profiles), ``out_extra`` (everything else the scheme returned, keys suffixed ``_scheme``), ``absorption``."""

    required_input_keys = canopy.INPUT_KEYS
    _schemes = AVAILABLE_SCHEMES
    vmd = VMD

    def __init__(self, scheme="2s", nlayers=60, **p_kwargs):
        self.nlayers = nlayers
        self.p_default = load_default_case(nlayers=nlayers)
        self._p = copy.deepcopy(self.p_default)
        self._run_count = 0
        self.out, self.out_extra, self.absorption = {}, {}, None
        self.assign_scheme(scheme)
        self._check_inputs()  # the default case; a failing update below then has something valid to fall back to
        if p_kwargs:
            self.update_p(**p_kwargs)

    # ---- the case ---------------------------------------------------------------------------
    @property
    def p(self):
        """Not the parameters: a reminder (the reference does the same, ``model.py:108-116``), since edits to a returned dict
        would bypass validation."""
        print("Please update parameters using `.update_p()`! Changes to `.p` will not be stored!\n"
              "Extract (copy) the parameters using `.copy_p()` or summarize using `.print_p()`.")

    def copy_p(self):
        return copy.deepcopy(self._p)

    def print_p(self):
        with np.printoptions(precision=3, threshold=7):
            pprint.pprint(self._p, indent=1)

    @property
    def cd(self):
        return CanopyDescription(*(self._p[k] for k in CANOPY_DESCRIPTION_KEYS))

    def __repr__(self):
        return f"Model(scheme={self.scheme['name']!r}, psi={self._p['psi']:.4g})"

    def assign_scheme(self, scheme_name, *, verbose=False):
        """Select a registered scheme by ID.  An unknown ID is reported on stdout and replaced by '2s' (``model.py:157-168``)."""
        entry = AVAILABLE_SCHEMES.get(scheme_name)
        if entry is None:
            print(f"{scheme_name!r} is not a valid scheme name/ID!\nThe valid ones are: {', '.join(AVAILABLE_SCHEMES)}.\n"
                  "Defaulting to Dickinson-Sellers two-stream.\n")
            entry = AVAILABLE_SCHEMES[_FALLBACK_SCHEME]
        elif verbose:
            rule = "=" * 40
            print(f"\n\n{rule}\nscheme: {entry['name']}\n{'-' * 40}")
        self.scheme = entry
        return self

    def update_p(self, **kwargs):
        """Replace inputs.  All-or-nothing: the candidate case is validated as a whole and adopted only if that succeeds, otherwise
        a warning carries the traceback and the previous case stays (``model.py:173-203``).  Non-input keys are skipped with a
        warning."""
        accepted = {}
        for name, value in kwargs.items():
            if name in canopy.INPUT_KEYS:
                accepted[name] = value
            else:
                warnings.warn(f"{name!r} is not intended as an input and will be ignored")
        candidate = {**self._p, **accepted}
        try:
            candidate.update(canopy.derive(candidate))
        except Exception:
            warnings.warn(f"Updating parameters failed. Full traceback:\n\n{traceback.format_exc()}\nReverting.")
        else:
            self._adopt(candidate)
        return self

    def update_spectra(self, ds):
        """Inputs from a spectra container with ``I_dr, I_df, wl, dwl, tl, rl, rs`` (an ``xarray.Dataset`` in the reference, any
        mapping of arrays here)."""
        take = lambda k: np.asarray(getattr(ds[k], "values", ds[k]))  # noqa: E731
        renamed = {"I_dr0_all": "I_dr", "I_df0_all": "I_df", "wl": "wl", "dwl": "dwl", "leaf_t": "tl", "leaf_r": "rl", "soil_r": "rs",
                   "wl_leafsoil": "wl"}
        return self.update_p(**{ours: take(theirs) for ours, theirs in renamed.items()})

    def _adopt(self, case):
        self._p = case
        self.nlev, self.nwl = canopy.sizes(case)

    def _check_inputs(self):
        """(Re)derive ``lai_tot, lai_eff, dlai, zm, dz, mu, wle, K_b_fn, G, K_b`` from the inputs; raises on an unsolvable case
        (``model.py:222-294``)."""
        self._adopt({**self._p, **canopy.derive(self._p)})

    # ---- solve ------------------------------------------------------------------------------
    def run(self, **extra_solver_kwargs):
        """Call the scheme's solver with the arguments its signature names (``model.py:296-320``)."""
        self._check_inputs()
        solver, argnames = self.scheme["solver"], self.scheme["args"]
        returned = solver(**{name: self._p[name] for name in argnames}, **extra_solver_kwargs)
        for name, value in returned.items():
            if name in RET_KEYS_ALL_SCHEMES:
                self.out[name] = value
            else:
                self.out_extra[name + _SCHEME_SUFFIX] = value
        self._run_count += 1
        return self

    @property
    def out_all(self):
        return {**self.out, **self.out_extra}

    def _need_run(self, purpose):
        if not self._run_count:
            raise Exception(f"Must run the model {purpose}.")

    def calc_absorption(self):
        """Layerwise absorption (``model.py:573-647``), computed by the device epilogue kernel."""
        self._need_run("first")
        import torch

        from . import batched
        from .leaf_angle import G_TABLE, describe_G

        p = self._p
        dev = torch.device("cuda", torch.cuda.current_device())
        t = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
        d = describe_G(p["G_fn"])
        kind, param = d if d is not None else (G_TABLE, 0.0)
        cols = batched.Columns(
            psi=t(p["psi"]), lai=t(p["lai"])[None, :], g_kind=torch.tensor([kind], dtype=torch.int32, device=dev), g_param=t(param),
            g_at_psi=t(p["G"]),
        )
        bands = batched.Bands(t(p["I_dr0_all"]), t(p["I_df0_all"]), t(p["leaf_r"]), t(p["leaf_t"]), t(p["soil_r"]))
        sol = {k: t(self.out[k])[None] for k in ("I_dr", "I_df_d", "I_df_u")}
        res = batched.absorb(cols, bands, sol)
        ab = {k: v[0].cpu().numpy() for k, v in res.items()}
        if not np.allclose(ab["aI_sl"] + ab["aI_sh"], ab["aI"]):  # the reference's sanity check, model.py:635
            raise AssertionError("sunlit + shaded absorption does not add up to the total")
        self.absorption = ab
        return self

    def _series_inputs(self, psi, I_dr0_all, I_df0_all, what):
        """``(scheme, cols, bands, sun)`` of a sun-angle series on this canopy (``ncol = 1``): the psi series and the spectra validated and
        broadcast to ``(nt, n_wl)``, the leaf-angle description sampled per step.  ``what`` names the kernel in the error of a scheme
        without one ("integrated" / "level")."""
        import torch

        from . import _lib, batched
        from .solvers.common import _describe, _sample

        self._check_inputs()
        p = self._p
        psi = np.atleast_1d(np.asarray(psi, dtype=np.float64))
        if psi.ndim != 1 or psi.size < 1:
            raise ValueError("`psi` must be a non-empty 1-D series of solar zenith angles")
        if not np.all((psi >= 0) & (psi < np.pi / 2)):
            raise ValueError("psi must be in [0, pi/2)")
        nt, nb = psi.size, self.nwl
        series = []
        for name, v in (("I_dr0_all", I_dr0_all), ("I_df0_all", I_df0_all)):
            v = np.asarray(p[name] if v is None else v, dtype=np.float64)
            if v.shape not in ((nb,), (nt, nb)):
                raise ValueError(f"`{name}` must be (n_wl,) or (nt, n_wl) = ({nt}, {nb})")
            series.append(np.ascontiguousarray(np.broadcast_to(v, (nt, nb))))
        scheme = self.scheme["name"] if self.scheme.get("name") in _lib.SCHEME_IDS else self.scheme.get("short_name")
        if scheme not in _lib.SCHEME_IDS:
            raise ValueError(f"scheme {scheme!r} has no {what} kernel")
        mu_s = 0.501  # the solvers' defaults, as `run()` without options
        G_fn, K_b_fn = p.get("G_fn"), p.get("K_b_fn")
        g = _describe(float(psi[0]), K_b_fn, G_fn, mu_s)
        g_at = None
        if g["g_table"] is not None:  # a callable: sampled at the quadrature nodes once, G_fn(psi_t) per step
            g_at = _sample(G_fn, psi) if G_fn is not None else _sample(K_b_fn, psi) * np.cos(psi)
        dev = torch.device("cuda", torch.cuda.current_device())
        t = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
        cols = batched.Columns(
            psi=t(psi[:1]), lai=t(p["lai"])[None, :], g_kind=torch.tensor([g["g_kind"]], dtype=torch.int32, device=dev),
            g_param=t(g["g_param"]), mla=None if p.get("mla") is None else t(float(p["mla"])),
            g_at_psi=None if g_at is None else t(g_at[:1]), g_table=None if g["g_table"] is None else t(g["g_table"])[None, :],
        )
        b = batched.Bands(None, None, t(p["leaf_r"]), t(p["leaf_t"]), t(p["soil_r"]))
        sun = batched.SunSeries(t(psi)[None, :], t(series[0])[None], t(series[1])[None], None if g_at is None else t(g_at)[None, :])
        return scheme, cols, b, sun

    def run_series(self, psi, I_dr0_all=None, I_df0_all=None, bands=("PAR", "NIR", "solar"), calc_PFD=False):
        """The band-integrated outputs of this canopy for a series of sun states in ONE device call
        (:class:`crt1d_amd.batched.IntegratedSeriesPlan`, ``ncol = 1``): what the loop

            for t: m.update_p(psi=psi[t], I_dr0_all=..., I_df0_all=...); m.run(); m.calc_absorption(); diagnostics.band(m.to_dataset(), ...)

        returns, stacked over a leading time axis.  ``psi``: ``(nt,)`` radians; ``I_dr0_all``, ``I_df0_all``: ``(nt, n_wl)``, ``(n_wl,)``
        or ``None`` (the case's own spectra at every step).  Returns ``{band_name: {variable: array}}`` with the level profiles
        ``I_dr, I_df_d, I_df_u, F, I_d`` ``(nt, nz)`` and the seven absorption entries ``(nt, nz-1)``; ``calc_PFD=True`` adds the
        photon-flux variants under the reference's names (``I`` -> ``PFD``).  The model's own state (``psi``, ``out``) is not changed."""
        import torch

        from . import _lib, batched, spectra

        scheme, cols, b, sun = self._series_inputs(psi, I_dr0_all, I_df0_all, "integrated")
        p = self._p
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(cols.device)  # noqa: E731
        names = list(bands)
        wle = np.asarray(p["wle"], dtype=float)
        weights = [(n, "", w) for n, w in zip(names, spectra.band_weights(wle, names))]
        if calc_PFD:
            weights += [(n, "PFD", w) for n, w in zip(names, spectra.band_weights(wle, names, wl=np.asarray(p["wl"], dtype=float), pfd=True))]
        res = {n: {} for n in names}
        ws = None
        for i in range(0, len(weights), 4):  # at most four band groups per call; later calls reuse the records
            chunk = weights[i:i + 4]
            plan = batched.IntegratedSeriesPlan(scheme, cols, b, sun, t(np.stack([w for _, _, w in chunk])), profiles=True, workspace=ws)
            out = {k: v[0].cpu().numpy() for k, v in plan(flags=0 if ws is None else _lib.FLAG_SKIP_PRECOMPUTE).items()}
            ws = plan.workspace
            for gi, (n, kindw, _) in enumerate(chunk):
                one = {k: out[k][..., gi] for k in ("I_dr", "I_df_d", "I_df_u", "F", "I_d")}
                one.update(batched.absorption_from_bandsums({k: out[k][..., gi] for k in ("aI", "aI_dr", "aI_sl", "aI_sh")}))
                for k, v in one.items():
                    res[n][k.replace("I", "PFD") if kindw else k] = v
        return res

    def run_series_levels(self, psi, levels, I_dr0_all=None, I_df0_all=None):
        """The spectra at a few levels of this canopy for a series of sun states in ONE device call
        (:class:`crt1d_amd.batched.LevelsSeriesPlan`, ``ncol = 1``): rows ``levels`` of what the loop

            for t: m.update_p(psi=psi[t], I_dr0_all=..., I_df0_all=...); m.run()

        leaves in ``m.out``, stacked over a leading time axis -- the diurnal course of the spectral albedo
        ``I_df_u[-1] / (I_dr[-1] + I_df_d[-1])``, of the spectrum at the ground or at a sensor height.  ``psi``, ``I_dr0_all``,
        ``I_df0_all`` as for :meth:`run_series`; ``levels`` as for :func:`crt1d_amd.batched.normalize_levels` (an int or ints, negatives
        from the top; returned rows are in ascending level order).  Returns ``{"I_dr", "I_df_d", "I_df_u", "F"}`` as NumPy arrays
        ``(nt, nsel, n_wl)``.  The model's own state (``psi``, ``out``) is not changed."""
        from . import batched

        scheme, cols, b, sun = self._series_inputs(psi, I_dr0_all, I_df0_all, "level")
        out = batched.solve_levels_series(scheme, cols, b, sun, levels)
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    @staticmethod
    def _sensor_set(weights, nb):
        from . import batched

        if isinstance(weights, batched.SensorSet):
            return weights
        w = weights.cpu().numpy() if hasattr(weights, "cpu") else np.asarray(weights, dtype=np.float64)
        if w.ndim == 1:
            w = w[None, :]
        if w.ndim != 2 or w.shape[1] != nb:
            raise ValueError(f"`weights` must be (nsens, n_wl) = (nsens, {nb})")
        return batched.SensorSet(w)

    def run_series_sensors(self, psi, weights, levels=(0, -1), I_dr0_all=None, I_df0_all=None):
        """:meth:`run_series_levels` folded with spectral responses in the same device call
        (:class:`crt1d_amd.batched.SensorLevelsSeriesPlan`, ``ncol = 1``): ``weights`` is a dense ``(nsens, n_wl)`` array (for instance
        :func:`crt1d_amd.spectra.sensor_weights`) or a :class:`crt1d_amd.batched.SensorSet`.  Returns ``{"I_dr", "I_df_d", "I_df_u", "F"}``
        as NumPy arrays ``(nt, nsel, nsens)``: the sensor-weighted sums of the rows ``levels``.  The model's own state is not changed."""
        from . import batched

        scheme, cols, b, sun = self._series_inputs(psi, I_dr0_all, I_df0_all, "level")
        out = batched.solve_sensor_levels_series(scheme, cols, b, sun, levels, self._sensor_set(weights, self.nwl))
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    def run_sensors(self, weights, levels=(0, -1)):
        """The sensor-band sums of the rows ``levels`` of what :meth:`run` leaves in ``m.out``, at the model's own sun state and spectra
        (:class:`crt1d_amd.batched.SensorLevelsPlan`): ``{"I_dr", "I_df_d", "I_df_u", "F"}`` as NumPy arrays ``(nsel, nsens)``.
        ``weights`` as for :meth:`run_series_sensors`.  The model's own state (``out``) is not changed."""
        import torch

        from . import batched

        self._check_inputs()
        p = self._p
        scheme, cols, b, sun = self._series_inputs(np.atleast_1d(float(p["psi"])), None, None, "level")
        cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                               g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
        b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        out = batched.solve_sensor_levels(scheme, cols, b, levels, self._sensor_set(weights, self.nwl))
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    def run_jacobian(self, levels=None):
        """The exact derivative of the rows ``levels`` (default: the ground and the top) of ``I_df_d, I_df_u, F`` with respect to this
        case's ``leaf_r``, ``leaf_t`` and ``soil_r`` spectra, band by band (:class:`crt1d_amd.batched.LevelsJacPlan`): NumPy arrays
        ``(nsel, 3, n_wl)`` per key, the parameter axis in the order of ``batched.JAC_PARAMS``.  ValueError for a scheme without a
        Jacobian kernel (``4s``, ``zq_pa``).  The model's own state (``out``) is not changed."""
        from . import batched

        self._check_inputs()
        p = self._p
        scheme, cols, b, sun = self._series_inputs(np.atleast_1d(float(p["psi"])), None, None, "Jacobian")
        if scheme not in batched.JAC_SCHEMES:
            raise ValueError(f"scheme {scheme!r} has no Jacobian kernel")
        cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                               g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
        b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        out = batched.solve_levels_jac(scheme, cols, b, (0, -1) if levels is None else levels)
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    def run_gradient(self, weights, levels=None, wrt=("leaf_r", "leaf_t", "soil_r", "lai", "leaf")):
        """The gradient of the scalar ``sum_X sum(weights[X] * X)`` of the rows ``levels`` (default: the ground and the top) of
        ``I_dr, I_df_d, I_df_u, F`` -- ``weights``: ``{key: (nsel, n_wl)}``, in a retrieval ``d loss / d X`` -- with respect to the names
        ``wrt`` (:class:`crt1d_amd.batched.LevelsGradPlan`): ``leaf_r``, ``leaf_t``, ``soil_r`` as NumPy arrays ``(n_wl,)``, ``lai`` (per
        ``ln LAI``) and ``leaf`` (per unit of this case's leaf-angle parameter) as floats.  ValueError for ``4s`` and ``zq_pa``.  The
        model's own state (``out``) is not changed."""
        import torch

        from . import batched

        self._check_inputs()
        p = self._p
        scheme, cols, b, sun = self._series_inputs(np.atleast_1d(float(p["psi"])), None, None, "gradient")
        if scheme not in batched.LevelsGradPlan._schemes:
            raise ValueError(batched.LevelsGradPlan._no_kernel.format(scheme))
        if not isinstance(weights, dict):
            raise ValueError("weights must be a dict of (nsel, n_wl) arrays")
        cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                               g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
        b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        w = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)[None]).to(cols.device) for k, v in weights.items()}
        out = batched.solve_levels_grad(scheme, cols, b, (0, -1) if levels is None else levels, w, wrt=wrt)
        return {k: v[0].cpu().numpy() if v.ndim == 2 else float(v[0]) for k, v in out.items()}

    def run_lai_sensitivity(self, levels=None, per="log"):
        """The exact derivative of the rows ``levels`` (default: the ground and the top) of ``I_dr, I_df_d, I_df_u, F`` with respect to
        this case's leaf area index at a fixed leaf-area profile (:class:`crt1d_amd.batched.LevelsDlaiPlan`): NumPy arrays
        ``(nsel, n_wl)`` per key.  ``per="log"``: ``dX / d ln(LAI)``; ``per="lai"``: ``dX / dLAI``.  ValueError for a scheme without the
        kernel (``4s``, ``zq_pa``) and for any other ``per``.  The model's own state (``out``) is not changed."""
        from . import batched

        self._check_inputs()
        p = self._p
        scheme, cols, b, sun = self._series_inputs(np.atleast_1d(float(p["psi"])), None, None, "LAI sensitivity")
        if scheme not in batched.DLAI_SCHEMES:
            raise ValueError(f"scheme {scheme!r} has no LAI-derivative kernel")
        cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                               g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
        b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        out = batched.solve_levels_dlai(scheme, cols, b, (0, -1) if levels is None else levels, per=per)
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    def run_leaf_angle_sensitivity(self, levels=None, wrt="param"):
        """The exact derivative of the rows ``levels`` (default: the ground and the top) of ``I_dr, I_df_d, I_df_u, F`` with respect to
        one leaf-angle parameter of this case (:class:`crt1d_amd.batched.LevelsDleafPlan` along ``batched.leaf_tangent(cols, wrt)``;
        ``wrt``: ``"param"``, ``"mla"``, ``"a"``, ``"b"``): NumPy arrays ``(nsel, n_wl)`` per key.  ValueError for a scheme without the
        kernel (``4s``, ``zq_pa``) and for any other ``wrt``.  The model's own state (``out``) is not changed."""
        from . import batched

        self._check_inputs()
        p = self._p
        scheme, cols, b, sun = self._series_inputs(np.atleast_1d(float(p["psi"])), None, None, "leaf-angle sensitivity")
        if scheme not in batched.DLEAF_SCHEMES:
            raise ValueError(f"scheme {scheme!r} has no leaf-angle-derivative kernel")
        if wrt not in batched.LEAF_WRT:
            raise ValueError(f"wrt must be one of {batched.LEAF_WRT}, got {wrt!r}")
        cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                               g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
        b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        out = batched.solve_levels_dleaf(scheme, cols, b, (0, -1) if levels is None else levels, batched.leaf_tangent(cols, wrt))
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    def run_sensor_jacobian(self, weights, levels=(0, -1), directions=None, lai=True, wrt_leaf=None):
        """The Jacobian of what :meth:`run_sensors` returns with respect to a parameter vector of this case
        (:class:`crt1d_amd.batched.SensorJacPlan`, ``ncol = 1``).  ``directions``: ``{"leaf_r" | "leaf_t" | "soil_r": (ntan, n_wl)}``, the
        derivatives of the spectra with respect to ``ntan`` parameters of a leaf or soil model (``None``: no such columns); ``lai``: a
        column per ``ln LAI``; ``wrt_leaf``: a leaf-angle parameter (``"param"``, ``"mla"``, ``"a"``, ``"b"``; ``None``: no such column).
        Returns ``{"I_dr", "I_df_d", "I_df_u", "F"}`` as NumPy arrays ``(nsel, nsens, npar)`` and ``"params"``, the names of the columns
        (``"dir0"``, ..., ``"lai"``, ``"leaf"``).  ValueError for ``4s`` and ``zq_pa``.  The model's own state (``out``) is not changed."""
        from . import batched

        self._check_inputs()
        p = self._p
        scheme, cols, b, sun = self._series_inputs(np.atleast_1d(float(p["psi"])), None, None, "sensor Jacobian")
        if scheme not in batched.SensorJacPlan._schemes:
            raise ValueError(batched.SensorJacPlan._no_kernel.format(scheme))
        directions = {} if directions is None else dict(directions)
        if any(k not in batched.JAC_PARAMS for k in directions):
            raise ValueError(f"directions must be a dict of (ntan, n_wl) arrays under keys out of {batched.JAC_PARAMS}")
        if wrt_leaf is not None and wrt_leaf not in batched.LEAF_WRT:
            raise ValueError(f"wrt_leaf must be None or one of {batched.LEAF_WRT}, got {wrt_leaf!r}")
        cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                               g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
        b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        d = {"d_" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in directions.items()}
        with batched.torch.cuda.device(cols.device):
            plan = batched.SensorJacPlan(scheme, cols, b, levels, self._sensor_set(weights, self.nwl), lai=lai,
                                         tangent=None if wrt_leaf is None else batched.leaf_tangent(cols, wrt_leaf), **d)
            out = plan()
        res = {k: v[0].cpu().numpy() for k, v in out.items()}
        res["params"] = plan.params
        return res

    def run_series_sensor_jacobian(self, psi, weights, levels=(0, -1), directions=None, lai=True, wrt_leaf=None, I_dr0_all=None,
                                   I_df0_all=None):
        """The Jacobian of what :meth:`run_series_sensors` returns with respect to ONE parameter vector of this case, for every sun state
        in one device call (:class:`crt1d_amd.batched.SensorJacSeriesPlan`, ``ncol = 1``).  ``psi``, ``I_dr0_all``, ``I_df0_all`` as for
        :meth:`run_series_sensors`; ``weights``, ``levels``, ``directions``, ``lai``, ``wrt_leaf`` as for :meth:`run_sensor_jacobian`.
        Returns ``{"I_dr", "I_df_d", "I_df_u", "F"}`` as NumPy arrays ``(nt, nsel, nsens, npar)`` and ``"params"``.  ValueError for ``4s``
        and ``zq_pa``.  The model's own state is not changed."""
        from . import batched

        scheme, cols, b, sun = self._series_inputs(psi, I_dr0_all, I_df0_all, "sensor Jacobian")
        if scheme not in batched.SensorJacSeriesPlan._schemes:
            raise ValueError(batched.SensorJacSeriesPlan._no_kernel.format(scheme))
        directions = {} if directions is None else dict(directions)
        if any(k not in batched.JAC_PARAMS for k in directions):
            raise ValueError(f"directions must be a dict of (ntan, n_wl) arrays under keys out of {batched.JAC_PARAMS}")
        if wrt_leaf is not None and wrt_leaf not in batched.LEAF_WRT:
            raise ValueError(f"wrt_leaf must be None or one of {batched.LEAF_WRT}, got {wrt_leaf!r}")
        d = {"d_" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in directions.items()}
        with batched.torch.cuda.device(cols.device):
            plan = batched.SensorJacSeriesPlan(scheme, cols, b, sun, levels, self._sensor_set(weights, self.nwl), lai=lai,
                                               tangent=None if wrt_leaf is None else batched.leaf_tangent_series(cols, sun, wrt_leaf), **d)
            out = plan()
        res = {k: v[0].cpu().numpy() for k, v in out.items()}
        res["params"] = plan.params
        return res

    @staticmethod
    def _lut_table(lut, lm_options, scheme, cols, b, levels, *, keys, sensors, sun, lai, leaf, **d):
        """The look-up table of ``lut=K``: K candidates of :func:`crt1d_amd.batched.lut_sample` in ``[lo, hi]``, the default start (or the
        ``p0`` given) first, evaluated on this model's own column."""
        from . import batched

        lo, hi, p0, leaf_model = (lm_options.get(k) for k in ("lo", "hi", "p0", "leaf_model"))
        if lo is None or hi is None:
            raise ValueError("lut= needs finite bounds lo and hi")
        if p0 is None and leaf_model is None:
            p0 = np.zeros(np.shape(lo))
            if leaf:
                p0[-1] = float(cols.g_param[0])
        q = batched.lut_sample(lo, hi, int(lut), include=None if p0 is None else np.asarray(p0, dtype=np.float64).reshape(1, -1))
        opts = {k: lm_options[k] for k in ("mu_s", "tau_d_method") if k in lm_options}
        table = batched.LutTable.build(scheme, cols, b, levels, q, keys=keys, sensors=sensors, sun=sun, lai=lai, leaf=leaf,
                                       leaf_model=leaf_model, **d, **opts)
        table.p_default = None if lm_options.get("p0") is None else p0  # (the caller's p0 stays the start without an eligible candidate)
        return table

    def retrieve(self, weights, y, levels=(0, -1), directions=None, lai=True, wrt_leaf=None, psi=None, niter=20, lut=None, posterior=False,
                 **lm_options):
        """A Levenberg-Marquardt retrieval of a parameter vector of this case from sensor-band observations
        (:class:`crt1d_amd.batched.RetrievalPlan`, ``ncol = 1``).  ``y``: ``{key: (nsel, nsens)}`` for keys out of ``"I_dr", "I_df_d",
        "I_df_u", "F"``, the observed values of what :meth:`run_sensors` returns; with ``psi`` (a series of sun angles) ``{key: (nt, nsel,
        nsens)}``, what :meth:`run_series_sensors` returns.  ``weights``, ``levels``, ``directions``, ``lai`` as for
        :meth:`run_sensor_jacobian`; ``wrt_leaf``: ``None`` or ``"param"`` (``g_param`` itself is retrieved).  ``lm_options``: ``p0``, ``lo``,
        ``hi``, ``prior``, ``inv_sigma_prior`` (each ``(npar,)``), ``prior_mean (npar,)`` with ``prior_precision (npar, npar)`` (a Gaussian
        prior with a full precision matrix, added to the diagonal one), ``inv_sigma`` (as ``y``), ``I_dr0_all`` / ``I_df0_all`` (with ``psi``) and
        the options of the plan.  Returns NumPy arrays ``p (npar,)``, ``cost``, ``status``, ``lam``, ``naccept``, ``nreject``,
        ``cov (npar, npar)`` and ``"params"``.  ValueError for ``4s`` and ``zq_pa``.  The model's own state is not changed.
        ``leaf_model=`` (a :class:`crt1d_amd.leaf_model.PlateLeafModel` on this model's wavelengths, among ``lm_options``) retrieves the
        plate model's parameters instead of leaf directions: ``directions`` may then hold ``"soil_r"`` only, and ``p0``, ``lo``, ``hi``
        are required.  ``lut=K``: a look-up-table start -- ``K`` candidates sampled in ``[lo, hi]`` (finite bounds required; the
        default start, or the ``p0`` given, is one of them, and where no candidate has a finite cost the retrieval starts there) are evaluated on this column (:class:`crt1d_amd.batched.LutTable`) and the
        retrieval starts from the best of them; ``lut=None``: the call as it always was.  ``posterior=True`` (with ``lut=``, else ValueError)
        adds the Bayesian look-up-table estimate over those candidates (:class:`crt1d_amd.batched.LutPosteriorPlan`, temperature 1):
        ``lut_mean (npar,)``, ``lut_cov (npar, npar)`` and ``lut_ess``, the effective number of candidates behind it."""
        from . import batched

        if posterior and lut is None:
            raise ValueError("posterior=True needs lut=K: the estimate is taken over the candidates of the look-up table")

        series = psi is not None
        spectra = [lm_options.pop(k, None) for k in ("I_dr0_all", "I_df0_all")]
        one = np.atleast_1d(float(self._p["psi"]))
        scheme, cols, b, sun = self._series_inputs(psi if series else one, *(spectra if series else (None, None)), "retrieval")
        directions = {} if directions is None else dict(directions)
        if any(k not in batched.JAC_PARAMS for k in directions):
            raise ValueError(f"directions must be a dict of (ntan, n_wl) arrays under keys out of {batched.JAC_PARAMS}")
        if wrt_leaf not in (None, "param"):
            raise ValueError(f"wrt_leaf must be None or 'param', got {wrt_leaf!r}")
        if not series:
            cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                                   g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
            b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        d = {"d_" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in directions.items()}
        keys = tuple(k for k in batched.LEVEL_KEYS if k in y)
        lead = lambda v: {k: np.asarray(a, dtype=np.float64)[None] for k, a in v.items()}  # noqa: E731
        if lm_options.get("inv_sigma") is not None:
            lm_options["inv_sigma"] = lead(lm_options["inv_sigma"])
        sensors = self._sensor_set(weights, self.nwl)
        if lut is not None:
            lm_options["p0"] = self._lut_table(lut, lm_options, scheme, cols, b, levels, keys=keys or tuple(y), sensors=sensors,
                                               sun=sun if series else None, lai=lai, leaf=wrt_leaf is not None, **d)
        res = batched.retrieve(scheme, cols, b, levels, sensors, lead(y), keys=keys or tuple(y), niter=niter,
                               sun=sun if series else None, lai=lai, leaf=wrt_leaf is not None, posterior=posterior, **d,
                               **lm_options)
        out = {k: v[0].cpu().numpy() for k, v in res.items() if k != "params"}
        out["params"] = res["params"]
        return out

    def retrieve_chain(self, weights, y, psi, inv_sigma_chain, levels=(0, -1), directions=None, lai=True, wrt_leaf=None, niter=20,
                       shared=None, **lm_options):
        """:meth:`retrieve` of this one canopy observed on ``nd`` dates, the dates coupled by a random-walk prior
        (:class:`crt1d_amd.batched.RetrievalPlan` with ``chain=nd``: one pixel, the column replicated ``nd`` times).  ``psi (nd,)``: the sun
        angle of every date; ``y``: ``{key: (nd, nsel, nsens)}``; ``inv_sigma_chain (nd - 1, npar)``: the coupling weights of the gaps
        between consecutive dates (0: not coupled; the time gap folded in).  ``lm_options``: ``p0``, ``prior``, ``inv_sigma_prior`` (each
        ``(nd, npar)`` or ``(npar,)``), ``lo``, ``hi`` ``(npar,)``, ``inv_sigma`` (as ``y``; a fully masked date is a cloudy one),
        ``I_dr0_all`` / ``I_df0_all`` ``(n_wl,)`` or ``(nd, n_wl)`` and the options of the plan.  Returns NumPy arrays ``p (nd, npar)``, the
        pixel's ``cost``, ``status``, ``lam``, ``naccept``, ``nreject``, the smoothed marginal covariances ``cov (nd, npar, npar)`` and
        ``"params"``.  ``shared``: the parameters that are constants of the canopy over the dates, names out of ``"params"`` or a boolean mask
        (``shared=`` of the plan): one unknown each instead of one per date.  The model's own state is not changed."""
        from . import batched

        psi = np.atleast_1d(np.asarray(psi, dtype=np.float64))
        if psi.ndim != 1 or psi.size < 1:
            raise ValueError("`psi` must be a non-empty 1-D series of solar zenith angles, one per date")
        nd = psi.size
        directions = {} if directions is None else dict(directions)
        if any(k not in batched.JAC_PARAMS for k in directions):
            raise ValueError(f"directions must be a dict of (ntan, n_wl) arrays under keys out of {batched.JAC_PARAMS}")
        if wrt_leaf not in (None, "param"):
            raise ValueError(f"wrt_leaf must be None or 'param', got {wrt_leaf!r}")
        d = {"d_" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in directions.items()}
        for k, v in y.items():
            if np.ndim(v) != 3 or np.shape(v)[0] != nd:
                raise ValueError(f"y[{k!r}] must be (nd, nsel, nsens) with nd = {nd} dates, got {np.shape(v)}")
        axis = batched._ParamAxis(d.get("d_leaf_r"), d.get("d_leaf_t"), d.get("d_soil_r"), lai, wrt_leaf is not None,
                                  lm_options.get("leaf_model"))
        npar = axis.npar
        mask = batched._check_shared(shared, nd, axis.params, lm_options.get("p0"))
        batched._check_chain(nd, inv_sigma_chain, nd, npar, mask)  # (before any device is touched)
        if np.ndim(inv_sigma_chain) != 2:
            raise ValueError(f"inv_sigma_chain must be (nd - 1, npar) = {(nd - 1, npar)} for the model's one pixel")
        spectra = [lm_options.pop(k, None) for k in ("I_dr0_all", "I_df0_all")]
        scheme, cols, b, sun = self._series_inputs(psi, *spectra, "retrieval")
        rep = lambda v: None if v is None else v.expand(nd, *v.shape[1:]).contiguous()  # noqa: E731  (the one column on every date)
        cols = batched.Columns(psi=sun.psi[0].contiguous(), lai=rep(cols.lai), g_kind=rep(cols.g_kind), g_param=rep(cols.g_param),
                               mla=rep(cols.mla), g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[0].contiguous(),
                               g_table=rep(cols.g_table))
        b = batched.Bands(sun.I_dr0[0].contiguous(), sun.I_df0[0].contiguous(), rep(b.leaf_r), rep(b.leaf_t), rep(b.soil_r))
        keys = tuple(k for k in batched.LEVEL_KEYS if k in y)
        f64 = lambda v: {k: np.asarray(a, dtype=np.float64) for k, a in v.items()}  # noqa: E731
        if lm_options.get("inv_sigma") is not None:
            lm_options["inv_sigma"] = f64(lm_options["inv_sigma"])
        res = batched.retrieve(scheme, cols, b, levels, self._sensor_set(weights, self.nwl), f64(y), keys=keys or tuple(y), niter=niter,
                               lai=lai, leaf=wrt_leaf is not None, chain=nd, inv_sigma_chain=inv_sigma_chain,
                               **({} if shared is None else {"shared": shared}), **d, **lm_options)
        out = {k: v[0].cpu().numpy() for k, v in res.items() if k != "params"}
        out["params"] = res["params"]
        return out

    def retrieve_sequential(self, weights, y_dates, psi_dates, inv_sigma_dyn, levels=(0, -1), directions=None, lai=True, wrt_leaf=None,
                            niter=10, smooth=True, **lm_options):
        """:meth:`retrieve_chain` solved date by date (:class:`crt1d_amd.batched.SequentialPlan`: one pixel, the column replicated ``nd``
        times): a forward filter that hands the posterior of a date to the next one as a full Gaussian prior, then a backward
        Rauch-Tung-Striebel sweep; any number of dates.  ``psi_dates (nd,)``; ``y_dates``: ``{key: (nd, nsel, nsens)}``; ``inv_sigma_dyn
        (nd - 1, npar)``: the random-walk weights of the gaps (the meaning of ``inv_sigma_chain``); ``niter``: the steps of every date.
        ``lm_options``: ``p0``, ``prior``, ``inv_sigma_prior`` (each ``(nd, npar)`` or ``(npar,)``), ``prior_mean (npar,)`` /
        ``prior_precision (npar, npar)`` (date 0 only), ``lo``, ``hi``, ``inv_sigma`` (as ``y_dates``), ``I_dr0_all`` / ``I_df0_all`` and
        the options of the plan.  Returns NumPy arrays ``p (nd, npar)`` (smoothed; ``smooth=False``: filtered), ``p_filtered``, ``cov (nd,
        npar, npar)``, ``cost``, ``status``, ``naccept``, ``nreject`` ``(nd,)``, ``info``, ``info_predict`` and ``"params"``.  The model's
        own state is not changed."""
        from . import batched

        psi = np.atleast_1d(np.asarray(psi_dates, dtype=np.float64))
        if psi.ndim != 1 or psi.size < 1:
            raise ValueError("`psi_dates` must be a non-empty 1-D series of solar zenith angles, one per date")
        nd = psi.size
        directions = {} if directions is None else dict(directions)
        if any(k not in batched.JAC_PARAMS for k in directions):
            raise ValueError(f"directions must be a dict of (ntan, n_wl) arrays under keys out of {batched.JAC_PARAMS}")
        if wrt_leaf not in (None, "param"):
            raise ValueError(f"wrt_leaf must be None or 'param', got {wrt_leaf!r}")
        d = {"d_" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in directions.items()}
        for k, v in y_dates.items():
            if np.ndim(v) != 3 or np.shape(v)[0] != nd:
                raise ValueError(f"y_dates[{k!r}] must be (nd, nsel, nsens) with nd = {nd} dates, got {np.shape(v)}")
        kw = dict(lm_options, lai=lai, leaf=wrt_leaf is not None, **d)
        spectra = [kw.pop(k, None) for k in ("I_dr0_all", "I_df0_all")]
        batched._check_sequential(nd, inv_sigma_dyn, nd, kw)  # (before any device is touched)
        if np.ndim(inv_sigma_dyn) != 2:
            raise ValueError(f"inv_sigma_dyn must be (nd - 1, npar) for the model's one pixel, got {np.shape(inv_sigma_dyn)}")
        scheme, cols, b, sun = self._series_inputs(psi, *spectra, "retrieval")
        rep = lambda v: None if v is None else v.expand(nd, *v.shape[1:]).contiguous()  # noqa: E731  (the one column on every date)
        cols = batched.Columns(psi=sun.psi[0].contiguous(), lai=rep(cols.lai), g_kind=rep(cols.g_kind), g_param=rep(cols.g_param),
                               mla=rep(cols.mla), g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[0].contiguous(),
                               g_table=rep(cols.g_table))
        b = batched.Bands(sun.I_dr0[0].contiguous(), sun.I_df0[0].contiguous(), rep(b.leaf_r), rep(b.leaf_t), rep(b.soil_r))
        keys = tuple(k for k in batched.LEVEL_KEYS if k in y_dates)
        f64 = lambda v: {k: np.asarray(a, dtype=np.float64) for k, a in v.items()}  # noqa: E731
        if kw.get("inv_sigma") is not None:
            kw["inv_sigma"] = f64(kw["inv_sigma"])
        res = batched.retrieve_sequential(scheme, cols, b, levels, f64(y_dates), nd=nd, inv_sigma_dyn=inv_sigma_dyn, keys=keys or tuple(y_dates),
                                          sensors=self._sensor_set(weights, self.nwl), niter=niter, smooth=smooth, **kw)
        out = {k: v[0].cpu().numpy() for k, v in res.items() if k != "params"}
        out["params"] = res["params"]
        return out

    def retrieve_spectral(self, y, levels=(-1,), directions=None, lai=True, wrt_leaf=None, niter=20, psi=None, I_dr0_all=None,
                          I_df0_all=None, lut=None, posterior=False, **lm_options):
        """:meth:`retrieve` from the level spectra themselves, band by band (:class:`crt1d_amd.batched.SpectralRetrievalPlan`,
        ``ncol = 1``): ``y``: ``{key: (nsel, n_wl)}`` for keys out of ``"I_dr", "I_df_d", "I_df_u", "F"``, the observed spectra at
        ``levels`` (default: the canopy top); with ``psi`` (a series of sun angles, and ``I_dr0_all`` / ``I_df0_all`` as for
        :meth:`run_series`) ``{key: (nt, nsel, n_wl)}``, the spectra of every sun state, fitted by ONE parameter vector
        (:class:`crt1d_amd.batched.SpectralNormalSeriesPlan`).  ``directions``, ``lai``, ``wrt_leaf`` as for :meth:`retrieve`.
        ``lm_options``: ``p0``, ``lo``, ``hi``, ``prior``, ``inv_sigma_prior`` (each ``(npar,)``), ``prior_mean`` / ``prior_precision`` (as for
        :meth:`retrieve`), ``inv_sigma`` (as ``y``; 0 masks a band) and the options of the plan.  Returns what :meth:`retrieve` returns.  ValueError for the schemes outside
        ``batched.SPECTRAL_RETRIEVE_SCHEMES``.  The model's own state is not changed.  ``leaf_model=``, ``lut=`` and ``posterior=`` as for :meth:`retrieve`."""
        from . import batched

        if posterior and lut is None:
            raise ValueError("posterior=True needs lut=K: the estimate is taken over the candidates of the look-up table")

        from . import _lib

        name = self.scheme["name"] if self.scheme.get("name") in _lib.SCHEME_IDS else self.scheme.get("short_name")
        if name not in batched.SPECTRAL_RETRIEVE_SCHEMES:  # (before any device is touched)
            raise ValueError(f"scheme {name!r} has no spectral retrieval; served: " + ", ".join(batched.SPECTRAL_RETRIEVE_SCHEMES))
        series = psi is not None
        one = np.atleast_1d(float(self._p["psi"]))
        scheme, cols, b, sun = self._series_inputs(psi if series else one, *((I_dr0_all, I_df0_all) if series else (None, None)),
                                                   "spectral retrieval")
        directions = {} if directions is None else dict(directions)
        if any(k not in batched.JAC_PARAMS for k in directions):
            raise ValueError(f"directions must be a dict of (ntan, n_wl) arrays under keys out of {batched.JAC_PARAMS}")
        if wrt_leaf not in (None, "param"):
            raise ValueError(f"wrt_leaf must be None or 'param', got {wrt_leaf!r}")
        if not series:
            cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                                   g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
            b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
        else:
            lm_options["sun"] = sun
        d = {"d_" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in directions.items()}
        keys = tuple(k for k in batched.LEVEL_KEYS if k in y)
        lead = lambda v: {k: np.asarray(a, dtype=np.float64)[None] for k, a in v.items()}  # noqa: E731
        if lm_options.get("inv_sigma") is not None:
            lm_options["inv_sigma"] = lead(lm_options["inv_sigma"])
        if lut is not None:
            lm_options["p0"] = self._lut_table(lut, lm_options, scheme, cols, b, levels, keys=keys or tuple(y), sensors=None,
                                               sun=lm_options.get("sun"), lai=lai, leaf=wrt_leaf is not None, **d)
        res = batched.retrieve_spectral(scheme, cols, b, levels, lead(y), keys=keys or tuple(y), niter=niter, lai=lai,
                                        leaf=wrt_leaf is not None, posterior=posterior, **d, **lm_options)
        out = {k: v[0].cpu().numpy() for k, v in res.items() if k != "params"}
        out["params"] = res["params"]
        return out

    # ---- output container -------------------------------------------------------------------
    def _scheme_absorption_vars(self, nz):
        """The scheme's own absorption outputs (``aI*_scheme``): on levels or on layers, by their leading size."""
        from .variables import da_attrs

        for name, arr in self.out_extra.items():
            if not name.startswith("aI"):
                continue
            dims = {nz: ("z", "wl"), nz - 1: ("zm", "wl")}.get(arr.shape[0])
            if dims is None:
                raise ValueError("Scheme absorption output has too many or too few levels.")
            base = name[: -len(_SCHEME_SUFFIX)]
            try:
                yield name, (dims, arr, da_attrs(base))
            except KeyError:
                raise Exception(f"Scheme absorbance variable {base} not found in vmd.") from None

    def to_dataset(self, *, info=""):
        """The reference's output dataset (``model.py:338-447``) as a plain :class:`Dataset`: same coordinates (``z, wl, zm,
        wle``), data variables (solution, ``I_d``, grid, absorption, scheme extras named ``aI*_scheme``, geometry scalars),
        dims, attributes and global attributes.  No xarray needed; :meth:`to_xr` converts when it is installed."""
        from . import __version__
        from .variables import dv_tuple

        self._need_run("before creating the dataset")
        p, out = self._p, self.out
        values = {name: out[name] for name in _SOLUTION_VARS}
        values["I_d"] = out["I_dr"] + out["I_df_d"]
        values.update({name: np.asarray(p[name]) for name in ("dwl", "lai", "dlai")})
        values.update(self.absorption or {})  # standard absorption calculations (layer in-out)
        data_vars = {name: dv_tuple(name, v) for name, v in values.items()}
        data_vars.update(self._scheme_absorption_vars(np.asarray(p["z"]).size))
        scalars = {"psi": p["psi"], "sza": np.rad2deg(p["psi"]), "G": p["G"], "K_b": p["K_b"]}
        data_vars.update({name: dv_tuple(name, v) for name, v in scalars.items()})
        coords = {name: dv_tuple(name, np.asarray(p[name])) for name in ("z", "wl", "zm", "wle")}
        attrs = {"info": info, "crt1d_version": __version__}
        attrs.update({f"scheme_{k}": self.scheme[k] for k in ("name", "long_name", "short_name")})
        return Dataset(coords, data_vars, attrs)

    def to_xr(self, *, info=""):
        """``xarray.Dataset`` of the run (``model.py:338-447``); needs xarray, which the hot path itself does not."""
        return self.to_dataset(info=info).to_xarray()


class Dataset:
    """Minimal labelled container: ``coords`` / ``data_vars`` map a name to ``(dims, array, attrs)``; ``attrs`` are global."""

    def __init__(self, coords, data_vars, attrs):
        self.coords, self.data_vars, self.attrs = dict(coords), dict(data_vars), dict(attrs)
        sizes = {k: np.shape(v[1])[0] for k, v in self.coords.items()}
        for name, (dims, arr, _) in self.data_vars.items():
            if tuple(sizes[d] for d in dims) != np.shape(arr):
                raise ValueError(f"{name}: shape {np.shape(arr)} does not match dims {dims} {sizes}")
        self.sizes = sizes

    def __getitem__(self, name):
        return (self.data_vars[name] if name in self.data_vars else self.coords[name])[1]

    def __contains__(self, name):
        return name in self.data_vars or name in self.coords

    def keys(self):
        return list(self.coords) + list(self.data_vars)

    def to_xarray(self):
        try:
            import xarray as xr
        except ImportError as e:
            raise ImportError("xarray is not installed; use the Dataset returned by Model.to_dataset() directly") from e
        return xr.Dataset(coords=self.coords, data_vars=self.data_vars, attrs=self.attrs)


def run_columns(scheme, columns, **solver_options):
    """Solve many canopies at once.

    ``columns``: dict of host arrays as produced by :func:`crt1d_amd.synth.make_columns`
    (``psi (ncol,)``, ``lai (ncol,nz)``, ``mla``, ``g_kind``, ``g_param``, per-(column, band) spectra).
    Returns a dict of ``(ncol, nz, nb)`` CUDA tensors (no host copy)."""
    from . import batched

    cols = batched.Columns.from_host(columns)
    bands = batched.Bands.from_host(columns)
    return batched.solve(scheme, cols, bands, **solver_options)
