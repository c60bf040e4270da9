"""
ctypes binding of ``libcrt1d_hip.so`` (C ABI declared in ``include/crt1d_hip.h``).

There is deliberately NO fallback: if the HIP library is missing every solver raises.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRT1D_HIP_LIB: measurement aid only -- an alternative build of the SAME library (tools/build_variant.sh) for in-round A/B runs
LIB_PATH = os.environ.get("CRT1D_HIP_LIB") or os.path.join(_HERE, "libcrt1d_hip.so")

# enum crt_scheme
SCHEME_IDS = {"2s": 0, "4s": 1, "n79": 2, "zq": 3, "bl": 4, "g77": 5, "bf": 6, "zq_pa": 7}
F32_SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
TAU_D_METHODS = {"quad": 0, "9sky": 1}
NQ_TAU, NQ_G4, NQ_9SKY = 96, 32, 9
NQ = NQ_TAU + NQ_G4 + NQ_9SKY

FLAG_SKIP_PRECOMPUTE = 1
FLAG_PRECOMPUTE_ONLY = 2
FLAG_DIRECT_STORES = 4

# crt_hip_levels_*: most levels one call serves (CRT_MAX_LEVEL_SELECT)
MAX_LEVEL_SELECT = 64

CRT_OK = 0
CRT_ERR_BAD_ARG = -1
CRT_ERR_WORKSPACE = -2
CRT_ERR_UNSUPPORTED = -3
CRT_ERR_LAUNCH = -4
CRT_ERR_SHAPE = -5

_vp = ctypes.c_void_p


class CrtColumns(ctypes.Structure):
    _fields_ = [
        ("ncol", ctypes.c_int32),
        ("nz", ctypes.c_int32),
        ("psi", _vp),
        ("lai", _vp),
        ("mla", _vp),
        ("g_kind", _vp),
        ("g_param", _vp),
        ("g_at_psi", _vp),
        ("g_table", _vp),
    ]


class CrtBands(ctypes.Structure):
    _fields_ = [
        ("nb", ctypes.c_int32),
        ("col_stride", ctypes.c_int64),
        ("I_dr0", _vp),
        ("I_df0", _vp),
        ("leaf_r", _vp),
        ("leaf_t", _vp),
        ("soil_r", _vp),
    ]


class CrtSunSeries(ctypes.Structure):
    """crt_sun_series: nt sun states (psi, g_at_psi, I_dr0, I_df0) per column for crt_hip_integrated_series_f64."""

    _fields_ = [
        ("nt", ctypes.c_int32),
        ("psi", _vp),
        ("g_at_psi", _vp),
        ("col_stride", ctypes.c_int64),
        ("I_dr0", _vp),
        ("I_df0", _vp),
    ]


class CrtSunSeriesF32(CrtSunSeries):
    """crt_sun_series_f32: the layout of crt_sun_series with float I_dr0 / I_df0 behind the pointers (crt_hip_levels_series_f32)."""


NTUNE = 16

# crt_options.tune: keys (enum crt_tune_key; what each one selects is documented there) and the named values of some of them.
# 0 is automatic for every key; 7 and 14 are reserved.
TUNE_TILE_LDS = 0
TUNE_TILE_T = 1
TUNE_TILE_FLAGS = 2
TUNE_CLOSED_STORE_WAVES = 3
TUNE_CLOSED_PIPE_T = 4
TUNE_PACK = 5
TUNE_PACK_COMPUTE_WAVES = 6
TUNE_TRI_M = 8
TUNE_TRI_T = 9
TUNE_TRI_FAMILY = 10
TUNE_TRI_STORE_WAVES = 11
TUNE_MIN_TILE_NB = 12
TUNE_FLAT_FLUSH = 13
TUNE_K0_SEPARATE = 15
# TUNE_TILE_FLAGS bits (enum crt_tune_tile_flag)
TILE_FLAG_SYNC_BARRIERS = 1
TILE_FLAG_GENERIC_FLUSH = 2
TILE_FLAG_NO_PIPELINE = 4
TILE_FLAG_NO_GENERIC_PIPELINE = 8
TILE_FLAG_FOUR_PAIR_STORE = 16
# TUNE_PACK values (enum crt_tune_pack)
PACK_OFF = 1
PACK_FORCE = 2
# TUNE_TRI_FAMILY values (enum crt_tune_tri_family); zq_pa reads 1 as its two-kernel path
TRI_FAMILY_NO_PIPELINE = 1
TRI_FAMILY_DOUBLE_BUFFERED = 2
TRI_FAMILY_REG_STAGED = 3
TRI_FAMILY_GENERIC_PIPELINE = 4
TRI_FAMILY_ZQPA_TWO_KERNEL = 1
TRI_FAMILY_ZQPA_PIPE = 5
TRI_FAMILY_ZQPA_PIPE2_DB = 6
TRI_FAMILY_ZQPA_PIPE2_RS = 7
# TUNE_FLAT_FLUSH values (enum crt_tune_flat_flush)
FLAT_FLUSH_OFF = 1
FLAT_FLUSH_PART_LINE = 2
FLAT_FLUSH_WHOLE_LINE = 3


class CrtOptions(ctypes.Structure):
    _fields_ = [("mu_s", ctypes.c_double), ("tau_d_method", ctypes.c_int32), ("flags", ctypes.c_int32), ("tune", ctypes.c_int32 * NTUNE)]


def set_tune(opts, tune):
    """Write the overrides ``{key: value}`` (keys ``TUNE_*``) into ``opts.tune``; keys not given are 0 (automatic).  A key outside
    ``range(NTUNE)`` is a ValueError; the values are checked by the library, at the call."""
    for k in tune:
        if not isinstance(k, int) or not 0 <= k < NTUNE:
            raise ValueError(f"unknown crt_options.tune key {k!r}: keys are the TUNE_* constants, 0 .. {NTUNE - 1}")
    for k in range(NTUNE):
        opts.tune[k] = int(tune.get(k, 0))
    return opts


class CrtOutputs(ctypes.Structure):
    _fields_ = [(k, _vp) for k in ("I_dr", "I_df_d", "I_df_u", "F", "x0", "x1", "x2")]


class CrtBandsumOut(ctypes.Structure):
    """``crt_bandsum_out``: layer-absorption band sums (+ ``totals``), and -- optional, all six or none -- the direct-beam part and the
    band-integrated level profiles of every irradiance variable ``diagnostics.band`` reduces."""

    _fields_ = [(k, _vp) for k in ("aI", "aI_sl", "aI_sh", "totals", "aI_dr", "I_dr", "I_df_d", "I_df_u", "F", "I_d")]


ABI_VERSION = 3


def _signatures():
    """``name -> (restype, argtypes)`` of every symbol of the C ABI (include/crt1d_hip.h): the one table :func:`load` applies and
    ``EXPORTS`` lists.  The f32 structs share the layouts of the f64 ones, so both storage types of an entry take the same ``argtypes``
    (except the sun series, whose two struct types are kept apart).  ``argtypes`` ``None``: left unset."""
    P = ctypes.POINTER
    i, i32, i64, sz, dbl, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double, ctypes.c_int
    cols, bands, opts, outs, sums = P(CrtColumns), P(CrtBands), P(CrtOptions), P(CrtOutputs), P(CrtBandsumOut)
    solve = [cols, bands, opts, outs, _vp, sz, _vp]
    t = {
        "crt_hip_abi_version": (i, None),
        "crt_hip_strerror": (ctypes.c_char_p, [i]),
        "crt_hip_workspace_bytes": (sz, [i, i32, i32]),
        "crt_hip_workspace_bytes_nb": (sz, [i, i32, i32, i32]),
        "crt_hip_series_workspace_bytes": (sz, [i, i32, i32, i32, i32]),
        "crt_hip_levels_series_workspace_bytes": (sz, [i, i32, i32, i32]),
        "crt_hip_quad_nodes": (ok, [dbl, P(dbl)]),
        "crt_hip_integrated_series_f64": (ok, [i, cols, bands, P(CrtSunSeries), opts, _vp, i32, sums, _vp, sz, _vp]),
    }
    for suffix, sun_t in (("f64", CrtSunSeries), ("f32", CrtSunSeriesF32)):
        t[f"crt_hip_solve_{suffix}"] = (ok, [i] + solve)
        for s in SCHEME_IDS if suffix == "f64" else F32_SCHEMES:
            t[f"crt_hip_{s}_{suffix}"] = (ok, solve)
        t[f"crt_hip_absorb_{suffix}"] = (ok, [cols, bands, _vp, _vp, _vp, P(_vp), _vp, _vp, _vp])
        t[f"crt_hip_absorb_bandsum_{suffix}"] = (ok, [cols, bands, _vp, _vp, _vp, _vp, i32, _vp, _vp, _vp, _vp, _vp])
        t[f"crt_hip_absorb_bandsum2_{suffix}"] = (ok, [cols, bands, _vp, _vp, _vp, _vp, i32, sums, _vp])
        t[f"crt_hip_integrated_{suffix}"] = (ok, [i, cols, bands, opts, _vp, i32, _vp, _vp, _vp, _vp, _vp, sz, _vp])
        t[f"crt_hip_integrated2_{suffix}"] = (ok, [i, cols, bands, opts, _vp, i32, sums, _vp, sz, _vp])
        t[f"crt_hip_levels_{suffix}"] = (ok, [i, cols, bands, opts, P(i32), i32, outs, _vp, sz, _vp])
        t[f"crt_hip_levels_series_{suffix}"] = (ok, [i, cols, bands, P(sun_t), opts, P(i32), i32, outs, _vp, sz, _vp])
    t.update({
        "crt_hip_bandsum_finish_f64": (ok, [cols, i32, sums, _vp]),
        "crt_hip_band_reduce_f64": (ok, [_vp, i64, i32, _vp, i32, _vp, _vp]),
        "crt_hip_tau_d_f64": (ok, [_vp, _vp, i64, i32, _vp, _vp]),
        "crt_hip_smear_tuv_f64": (ok, [_vp, i64, i32, _vp, i32, _vp, i32, _vp, _vp]),
        "crt_hip_lai_beta_f64": (ok, [_vp, _vp, _vp, i32, i32, _vp, _vp, _vp, _vp]),
        "crt_hip_buffer_alloc_set": (ok, [i32, P(sz), P(_vp)]),
        "crt_hip_buffer_alloc": (ok, [sz, P(_vp)]),
        "crt_hip_buffer_free": (ok, [_vp]),
        "crt_hip_buffer_trim": (ok, []),
        "crt_hip_buffer_set_retain": (ok, [sz]),
        "crt_hip_buffer_describe": (ok, [_vp, ctypes.c_char_p, sz]),
        "crt_hip_buffer_stats": (ok, [P(i64)]),
        "crt_hip_last_kernel": (ctypes.c_char_p, []),
        "crt_hip_probe_fill_f64": (ok, [_vp, sz, dbl, _vp]),
        "crt_hip_probe_copy_f64": (ok, [_vp, _vp, sz, _vp]),
        "crt_hip_probe_store_set_f64": (ok, [P(_vp), i32, i64, i64, i32, dbl, _vp]),
        "crt_hip_probe_math_f64": (ok, [_vp, sz, _vp, _vp, _vp, _vp]),
    })
    return t


_SIGNATURES = _signatures()
EXPORTS = list(_SIGNATURES)

# leaf-inclination PDFs (include/crt1d_hip_leaf.h): the same library, a header and a table of their own -- EXPORTS stays the symbol set of
# include/crt1d_hip.h.  (The PDF kind ids are leaf_angle.PDF_*.)
LEAF_NGL, LEAF_NMLA = 48, 64


def _leaf_signatures():
    dp, i32, dbl, ok = ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_double, ctypes.c_int
    return {
        "crt_hip_leaf_pdf_nodes_f64": (ok, [dp, dp, dp, dp]),
        "crt_hip_g_from_pdf_f64": (ok, [_vp, _vp, i32, dbl, _vp, i32, _vp, _vp, _vp, _vp]),
    }


_LEAF_SIGNATURES = _leaf_signatures()
LEAF_EXPORTS = list(_LEAF_SIGNATURES)

# spectral inputs (include/crt1d_hip_spectra.h): raw spectra -> Bands, again a header and a table of their own
LIGHT_UNIFORM, LIGHT_PLANCK, LIGHT_TABLE = 0, 1, 2  # enum crt_light
LIGHT_KINDS = {"uniform": LIGHT_UNIFORM, "planck": LIGHT_PLANCK, "table": LIGHT_TABLE}
SPECTRA_NGL = 16
SPECTRA_MAX_NB = 512
SPECTRA_MAX_ITEMS = 65536
SPECTRA_BLOCK = 512
SPECTRA_LDS_BYTES = 160 * 1024


def _spectra_signatures():
    dp, ip, i32, i64, dbl, ok = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_int
    return {
        "crt_hip_planck_nodes_f64": (ok, [dp, dp]),
        "crt_hip_avg_optical_prop_f64": (ok, [_vp, i32, _vp, i32, _vp, i32, ip, i32, dbl, _vp, i32, _vp, i32, i32, _vp, _vp, _vp]),
        "crt_hip_bands_from_spectra_f64": (ok, [_vp, i32, _vp, i64, _vp, i64, _vp, i64, _vp, i32, _vp, i64, _vp, i64, i32, _vp, i32, ip, i32, dbl,
                                                _vp, _vp, _vp, _vp, _vp, _vp]),
    }


_SPECTRA_SIGNATURES = _spectra_signatures()
SPECTRA_EXPORTS = list(_SPECTRA_SIGNATURES)

# sensor-band outputs (include/crt1d_hip_sensor.h): level spectra folded with spectral responses, a header and a table of their own
MAX_SENSOR_BANDS = 64  # CRT_MAX_SENSOR_BANDS


class CrtSensorSet(ctypes.Structure):
    """``crt_sensor_set``: ``first`` / ``count`` are HOST arrays, ``w`` the packed DEVICE weights."""

    _fields_ = [("nsens", ctypes.c_int32), ("first", ctypes.POINTER(ctypes.c_int32)), ("count", ctypes.POINTER(ctypes.c_int32)), ("w", _vp)]


class CrtSensorOut(ctypes.Structure):
    _fields_ = [(k, _vp) for k in ("I_dr", "I_df_d", "I_df_u", "F")]


def _sensor_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    cols, bands, opts = P(CrtColumns), P(CrtBands), P(CrtOptions)
    tail = [opts, P(i32), i32, P(CrtSensorSet), P(CrtSensorOut), _vp, sz, _vp]
    return {
        "crt_hip_sensor_workspace_bytes": (sz, [i, i32, i32, i32, i32, i32]),
        "crt_hip_sensor_levels_f64": (ok, [i, cols, bands] + tail),
        "crt_hip_sensor_levels_f32": (ok, [i, cols, bands] + tail),
        "crt_hip_sensor_series_workspace_bytes": (sz, [i, i32, i32, i32, i32, i32, i32]),
        "crt_hip_sensor_levels_series_f64": (ok, [i, cols, bands, P(CrtSunSeries)] + tail),
    }


_SENSOR_SIGNATURES = _sensor_signatures()
SENSOR_EXPORTS = list(_SENSOR_SIGNATURES)

# optical-property Jacobians of the level spectra (include/crt1d_hip_jac.h), again a header and a table of their own.  This and the two
# derivative entries below run one host path in the library (api.hip: levels_deriv_impl) and one plan base (batched._LevelsDerivPlan).
JAC_NPARAM = 3  # CRT_JAC_NPARAM: leaf_r, leaf_t, soil_r
JAC_MAX_NZ = {"n79": 1076, "zq": 1200}  # CRT_JAC_MAX_NZ_N79, CRT_JAC_MAX_NZ_ZQ


class CrtJacOut(ctypes.Structure):
    _fields_ = [(k, _vp) for k in ("I_df_d", "I_df_u", "F")]


def _jac_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_levels_jac_workspace_bytes": (sz, [i, i32, i32, i32, i32]),
        "crt_hip_levels_jac_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtOptions), P(i32), i32, P(CrtJacOut), _vp, sz, _vp]),
    }


_JAC_SIGNATURES = _jac_signatures()
JAC_EXPORTS = list(_JAC_SIGNATURES)

# LAI derivative of the level spectra (include/crt1d_hip_dlai.h), again a header and a table of their own
DLAI_MAX_NZ = {"n79": 928, "zq": 1135}  # CRT_DLAI_MAX_NZ_N79, CRT_DLAI_MAX_NZ_ZQ


class CrtDlaiOut(ctypes.Structure):
    _fields_ = [(k, _vp) for k in ("I_dr", "I_df_d", "I_df_u", "F")]


def _dlai_signatures():
    P = ctypes.POINTER
    i, i32, i64, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_levels_dlai_workspace_bytes": (sz, [i, i32, i32, i32, i32]),
        "crt_hip_levels_dlai_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtOptions), P(i32), i32, P(CrtDlaiOut), _vp, sz, _vp]),
        "crt_hip_dtau_d_f64": (ok, [_vp, _vp, i64, i32, _vp, _vp]),
    }


_DLAI_SIGNATURES = _dlai_signatures()
DLAI_EXPORTS = list(_DLAI_SIGNATURES)

# leaf-angle derivative of the level spectra (include/crt1d_hip_dleaf.h), again a header and a table of their own; the outputs are a
# CrtDlaiOut, the depth limits DLAI_MAX_NZ


class CrtLeafTangent(ctypes.Structure):
    """``crt_leaf_tangent``: device pointers; ``dmla`` may be NULL (zeros)."""

    _fields_ = [(k, _vp) for k in ("dg_table", "dg_at_psi", "dmla")]


def _dleaf_signatures():
    P = ctypes.POINTER
    i, i32, i64, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_levels_dleaf_workspace_bytes": (sz, [i, i32, i32, i32, i32]),
        "crt_hip_levels_dleaf_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtOptions), P(i32), i32, P(CrtLeafTangent), P(CrtDlaiOut), _vp, sz,
                                          _vp]),
        "crt_hip_g_dparam_f64": (ok, [P(CrtColumns), _vp, _vp, _vp]),
        "crt_hip_dtau_d_dleaf_f64": (ok, [_vp, _vp, _vp, i64, i32, _vp, _vp]),
    }


_DLEAF_SIGNATURES = _dleaf_signatures()
DLEAF_EXPORTS = list(_DLEAF_SIGNATURES)

# gradient of a weighted sum of the level spectra (include/crt1d_hip_grad.h), again a header and a table of their own: the three
# derivatives above contracted with one set of weights in one kernel; the closed forms only


class CrtGradWeights(ctypes.Structure):
    """``crt_grad_weights``: d loss / d X at the selected levels, each ``[ncol][nsel][nb]`` or NULL."""

    _fields_ = [(k, _vp) for k in ("I_dr", "I_df_d", "I_df_u", "F")]


class CrtGradOut(ctypes.Structure):
    """``crt_grad_out``: the optics gradients ``[ncol][nb]``, ``lai`` and ``leaf`` ``[ncol]``; NULL = not formed."""

    _fields_ = [(k, _vp) for k in ("leaf_r", "leaf_t", "soil_r", "lai", "leaf")]


def _grad_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_levels_grad_workspace_bytes": (sz, [i, i32, i32, i32, i32]),
        "crt_hip_levels_grad_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtOptions), P(i32), i32, P(CrtGradWeights), P(CrtLeafTangent),
                                         P(CrtGradOut), _vp, sz, _vp]),
    }


_GRAD_SIGNATURES = _grad_signatures()
GRAD_EXPORTS = list(_GRAD_SIGNATURES)

# Jacobian of the sensor-band sums (include/crt1d_hip_sensjac.h), again a header and a table of their own: the three derivatives above
# folded with a sensor set in one kernel; the closed forms only
SENSJAC_MAX_NTAN = 8  # CRT_SENSJAC_MAX_NTAN


class CrtOpticsDirs(ctypes.Structure):
    """``crt_optics_dirs``: ``ntan`` directions in (leaf_r, leaf_t, soil_r), each ``[ncol or 1][ntan][nb]`` on the device or NULL (zeros)."""

    _fields_ = [("ntan", ctypes.c_int32), ("col_stride", ctypes.c_int64), ("leaf_r", _vp), ("leaf_t", _vp), ("soil_r", _vp)]


class CrtSensJacOut(ctypes.Structure):
    """``crt_sensjac_out``: each ``[ncol][nsel][nsens][npar]`` or NULL."""

    _fields_ = [(k, _vp) for k in ("I_dr", "I_df_d", "I_df_u", "F")]


def _sensjac_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_sensor_jac_workspace_bytes": (sz, [i, i32, i32, i32, i32, i32, i32]),
        "crt_hip_sensor_jac_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtOptions), P(i32), i32, P(CrtSensorSet), P(CrtOpticsDirs), i,
                                        P(CrtLeafTangent), P(CrtSensJacOut), _vp, sz, _vp]),
    }


_SENSJAC_SIGNATURES = _sensjac_signatures()
SENSJAC_EXPORTS = list(_SENSJAC_SIGNATURES)

# the sun-angle series of that Jacobian (include/crt1d_hip_sensjac_series.h), again a header and a table of their own


class CrtLeafTangentSeries(ctypes.Structure):
    """``crt_leaf_tangent_series``: device pointers; ``dg_at_psi`` is ``[ncol][nt]``, ``dmla`` may be NULL (zeros)."""

    _fields_ = [(k, _vp) for k in ("dg_table", "dg_at_psi", "dmla")]


def _sensjac_series_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_sensor_jac_series_workspace_bytes": (sz, [i, i32, i32, i32, i32, i32, i32, i32]),
        "crt_hip_sensor_jac_series_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtSunSeries), P(CrtOptions), P(i32), i32, P(CrtSensorSet),
                                               P(CrtOpticsDirs), i, P(CrtLeafTangentSeries), P(CrtSensJacOut), _vp, sz, _vp]),
        "crt_hip_g_dparam_series_f64": (ok, [P(CrtColumns), P(CrtSunSeries), _vp, _vp, _vp]),
    }


_SENSJAC_SERIES_SIGNATURES = _sensjac_series_signatures()
SENSJAC_SERIES_EXPORTS = list(_SENSJAC_SERIES_SIGNATURES)

# the per-column Levenberg-Marquardt retrieval on those Jacobians (include/crt1d_hip_retrieve.h), again a header and a table of their own
RETRIEVE_MAX_NPAR = SENSJAC_MAX_NTAN + 2  # CRT_RETRIEVE_MAX_NPAR
LM_MAX_BLOCKS = 4  # CRT_LM_MAX_BLOCKS
LM_RUNNING, LM_CONVERGED_X, LM_CONVERGED_F, LM_STALLED, LM_FAILED_START = range(5)  # enum crt_lm_status


class CrtRetrieveApply(ctypes.Structure):
    """``crt_retrieve_apply``: the base inputs, the parameter vector and the working arrays ``k_retrieve_apply`` writes."""

    _fields_ = ([(k, ctypes.c_int32) for k in ("ncol", "nz", "nb", "npar", "i_lai", "i_leaf")] + [("base_stride", ctypes.c_int64)]
                + [(k, _vp) for k in ("leaf_r0", "leaf_t0", "soil_r0", "lai0", "p", "leaf_r", "leaf_t", "soil_r", "lai_scale", "lai", "g_param")])


class CrtLmObs(ctypes.Structure):
    """``crt_lm_obs``: one block of observations, ``f`` / ``y`` / ``inv_sigma`` ``[ncol][nrow]``, ``J`` ``[ncol][nrow][npar]``."""

    _fields_ = [("nrow", ctypes.c_int32)] + [(k, _vp) for k in ("f", "J", "y", "inv_sigma")]


class CrtLmProblem(ctypes.Structure):
    """``crt_lm_problem``: the sizes, the options of the algorithm, the bounds ``[npar]`` and the prior ``[ncol][npar]``."""

    _fields_ = ([("ncol", ctypes.c_int32), ("npar", ctypes.c_int32)]
                + [(k, ctypes.c_double) for k in ("lam_up", "lam_down", "lam_min", "lam_max", "xtol", "ftol")]
                + [(k, _vp) for k in ("lo", "hi", "prior", "inv_sigma_prior")])


class CrtLmState(ctypes.Structure):
    """``crt_lm_state``: the caller-owned per-column state of the Levenberg-Marquardt loop."""

    _fields_ = [(k, _vp) for k in ("p", "p_trial", "cost", "lam", "A", "g", "status", "naccept", "nreject")]


def _retrieve_signatures():
    P = ctypes.POINTER
    i32, ok = ctypes.c_int32, ctypes.c_int
    return {
        "crt_hip_retrieve_apply_f64": (ok, [P(CrtRetrieveApply), P(CrtOpticsDirs), _vp]),
        "crt_hip_lm_step_f64": (ok, [P(CrtLmProblem), P(CrtLmObs), i32, P(CrtLmState), _vp]),
        "crt_hip_lm_covariance_f64": (ok, [i32, i32, _vp, _vp, _vp]),
    }


_RETRIEVE_SIGNATURES = _retrieve_signatures()
RETRIEVE_EXPORTS = list(_RETRIEVE_SIGNATURES)

# the retrieval from the level spectra themselves (include/crt1d_hip_specfit.h), again a header and a table of their own: the normal
# equations of the per-band misfit in one kernel and the step that consumes such sums; the closed forms only


class CrtSpecObs(ctypes.Structure):
    """``crt_spec_obs``: the observed level spectra and their weights, each ``[ncol][nsel][nb]`` on the device; a NULL ``y_*``: the key is
    not observed, a NULL ``inv_sigma_*``: ones."""

    _fields_ = [(p + k, _vp) for p in ("y_", "inv_sigma_") for k in ("I_dr", "I_df_d", "I_df_u", "F")]


class CrtSpecNormalOut(ctypes.Structure):
    """``crt_spec_normal_out``: ``A [ncol][npar (npar + 1) / 2]``, ``g [ncol][npar]``, ``c2 [ncol]`` and the optional model spectra."""

    _fields_ = [(k, _vp) for k in ("A", "g", "c2", "fwd_I_dr", "fwd_I_df_d", "fwd_I_df_u", "fwd_F")]


class CrtLmNormalBlock(ctypes.Structure):
    """``crt_lm_normal_block``: the sums ``A``, ``g``, ``c2`` of one evaluation at the trial point."""

    _fields_ = [(k, _vp) for k in ("A", "g", "c2")]


def _specfit_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_spectral_normal_workspace_bytes": (sz, [i, i32, i32, i32, i32, i32, i32]),
        "crt_hip_spectral_normal_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtOptions), P(i32), i32, P(CrtOpticsDirs), i, P(CrtLeafTangent),
                                             P(CrtSpecObs), P(CrtSpecNormalOut), _vp, sz, _vp]),
        "crt_hip_lm_step_normal_f64": (ok, [P(CrtLmProblem), P(CrtLmNormalBlock), i32, P(CrtLmState), _vp]),
    }


_SPECFIT_SIGNATURES = _specfit_signatures()
SPECFIT_EXPORTS = list(_SPECFIT_SIGNATURES)

# those normal equations over a sun-angle series (include/series/crt1d_hip_specfit_series.h); again a table of its own


class CrtSpecSeriesOut(ctypes.Structure):
    """``crt_spec_series_out``: the sums over the sun states ``A [ncol][ntri]``, ``g [ncol][npar]``, ``c2 [ncol]``; the optional sums of
    every sun state ``A_t / g_t / c2_t`` (``[ncol][nt]...``, all NULL or all set); the optional model spectra ``[ncol][nt][nsel][nb]``."""

    _fields_ = [(k, _vp) for k in ("A", "g", "c2", "A_t", "g_t", "c2_t", "fwd_I_dr", "fwd_I_df_d", "fwd_I_df_u", "fwd_F")]


def _specfit_series_signatures():
    P = ctypes.POINTER
    i, i32, sz, ok = ctypes.c_int, ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_spectral_normal_series_workspace_bytes": (sz, [i, i32, i32, i32, i32, i32, i32, i32]),
        "crt_hip_spectral_normal_series_f64": (ok, [i, P(CrtColumns), P(CrtBands), P(CrtSunSeries), P(CrtOptions), P(i32), i32,
                                                    P(CrtOpticsDirs), i, P(CrtLeafTangentSeries), P(CrtSpecObs), P(CrtSpecSeriesOut), _vp, sz,
                                                    _vp]),
    }


_SPECFIT_SERIES_SIGNATURES = _specfit_series_signatures()
SPECFIT_SERIES_EXPORTS = list(_SPECFIT_SERIES_SIGNATURES)

# the generalised plate model of leaf optics (include_ext/crt1d_hip_leafmodel.h): the leaf model behind the leaf directions of a retrieval;
# again a header and a table of their own
PLATE_MAX_NABS = SENSJAC_MAX_NTAN - 1  # CRT_PLATE_MAX_NABS
PLATE_K_MIN, PLATE_K_MAX = 1e-6, 100.0  # CRT_PLATE_K_MIN, CRT_PLATE_K_MAX


class CrtPlateLeafModel(ctypes.Structure):
    """``crt_plate_leaf_model``: the sizes and the per-band spectra of the model, device pointers."""

    _fields_ = [(k, ctypes.c_int32) for k in ("ncol", "nb", "nabs")] + [(k, _vp) for k in ("kspec", "t_alpha", "t_90", "n")]


def _leafmodel_signatures():
    i32, i64, ok = ctypes.c_int32, ctypes.c_int64, ctypes.c_int
    return {"crt_hip_plate_leaf_f64": (ok, [ctypes.POINTER(CrtPlateLeafModel), _vp, i64, _vp, _vp, i32, _vp, _vp, _vp])}


_LEAFMODEL_SIGNATURES = _leafmodel_signatures()
LEAFMODEL_EXPORTS = list(_LEAFMODEL_SIGNATURES)

# the look-up-table start of a retrieval (include_lut/crt1d_hip_lut.h): the fused misfit of the observations against a table of model
# evaluations with the selection of the best candidates; again a header and a table of their own
LUT_MAX_BEST = 8  # CRT_LUT_MAX_BEST
LUT_MAX_KSPLIT = 256  # CRT_LUT_MAX_KSPLIT


class CrtLutTable(ctypes.Structure):
    """``crt_lut_table``: ``q [K][npar]`` and ``m[b] [K][nrow_b]`` on the device."""

    _fields_ = [("ncand", ctypes.c_int32), ("npar", ctypes.c_int32), ("nblk", ctypes.c_int32), ("nrow", ctypes.c_int32 * LM_MAX_BLOCKS),
                ("q", _vp), ("m", _vp * LM_MAX_BLOCKS)]


class CrtLutObs(ctypes.Structure):
    """``crt_lut_obs``: ``y[b]``, ``inv_sigma[b]`` (or NULL) ``[ncol][nrow_b]``; ``prior``, ``inv_sigma_prior`` ``[ncol][npar]`` or both NULL."""

    _fields_ = [("ncol", ctypes.c_int32), ("y", _vp * LM_MAX_BLOCKS), ("inv_sigma", _vp * LM_MAX_BLOCKS), ("prior", _vp),
                ("inv_sigma_prior", _vp)]


class CrtLutOut(ctypes.Structure):
    """``crt_lut_out``: ``index [ncol][nbest]`` int32, ``cost [ncol][nbest]``, ``p [ncol][npar]`` or NULL; ``ksplit`` 0 = automatic."""

    _fields_ = [("nbest", ctypes.c_int32), ("ksplit", ctypes.c_int32), ("index", _vp), ("cost", _vp), ("p", _vp)]


def _lut_signatures():
    P = ctypes.POINTER
    i32, sz, ok = ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_lut_match_workspace_bytes": (sz, [i32, i32, i32]),
        "crt_hip_lut_match_f64": (ok, [P(CrtLutTable), P(CrtLutObs), P(CrtLutOut), _vp, sz, _vp]),
    }


_LUT_SIGNATURES = _lut_signatures()
LUT_EXPORTS = list(_LUT_SIGNATURES)

# the look-up-table posterior (include_post/crt1d_hip_lut_posterior.h): the likelihood-weighted mean and covariance of the table's candidates;
# the structs of the match, and again a header and a table of their own


class CrtLutPosteriorOut(ctypes.Structure):
    """``crt_lut_posterior_out``: ``temperature`` (finite, > 0), ``temperature_col [ncol]`` or NULL, ``ksplit`` 0 = automatic; ``index
    [ncol]`` int32, ``cost [ncol]``, ``mean [ncol][npar]``, ``cov [ncol][npar][npar]``, ``wsum [ncol]``, ``ess [ncol]``."""

    _fields_ = [("temperature", ctypes.c_double), ("temperature_col", _vp), ("ksplit", ctypes.c_int32), ("index", _vp), ("cost", _vp),
                ("mean", _vp), ("cov", _vp), ("wsum", _vp), ("ess", _vp)]


def _lut_posterior_signatures():
    P = ctypes.POINTER
    i32, sz, ok = ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
    return {
        "crt_hip_lut_posterior_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "crt_hip_lut_posterior_f64": (ok, [P(CrtLutTable), P(CrtLutObs), P(CrtLutPosteriorOut), _vp, sz, _vp]),
    }


_LUT_POSTERIOR_SIGNATURES = _lut_posterior_signatures()
LUT_POSTERIOR_EXPORTS = list(_LUT_POSTERIOR_SIGNATURES)

# the Levenberg-Marquardt step on a chain of coupled dates (include_chain/crt1d_hip_lm_chain.h): the sums from sensor rows, the step of a
# pixel's nd dates under a random-walk prior, the smoothed marginal covariances; the structs of the step, a header and a table of their own

LM_CHAIN_LDS_LIMIT = 160 * 1024  # CRT_LM_CHAIN_LDS_LIMIT


def lm_chain_lds_bytes(nd, npar):
    """``CRT_LM_CHAIN_LDS_BYTES(nd, npar)``: the dynamic LDS of one pixel of the chain entries, which is that of the shared-parameter
    kernels with nothing shared."""
    return lm_shared_lds_bytes(nd, npar, 0)


def lm_chain_max_nd(npar):
    """``crt_hip_lm_chain_max_nd``: the largest ``nd`` whose LDS fits the limit; 0 for a refused ``npar``.  No library is loaded."""
    return lm_shared_max_nd(npar, 0)


class CrtLmChain(ctypes.Structure):
    """``crt_lm_chain``: ``npix``, ``nd``; ``dyn_stride`` 0 or ``(nd - 1) * npar``; ``inv_sigma_dyn [npix or 1][nd - 1][npar]``."""

    _fields_ = [("npix", ctypes.c_int32), ("nd", ctypes.c_int32), ("dyn_stride", ctypes.c_int64), ("inv_sigma_dyn", _vp)]


def _chain_signatures():
    P = ctypes.POINTER
    i32, ok = ctypes.c_int32, ctypes.c_int
    return {
        "crt_hip_lm_normal_f64": (ok, [i32, i32, P(CrtLmObs), i32, _vp, _vp, _vp, _vp]),
        "crt_hip_lm_step_chain_f64": (ok, [P(CrtLmChain), P(CrtLmProblem), P(CrtLmNormalBlock), i32, P(CrtLmState), _vp]),
        "crt_hip_lm_chain_covariance_f64": (ok, [P(CrtLmChain), i32, _vp, _vp, _vp]),
        "crt_hip_lm_chain_max_nd": (i32, [i32]),
    }


_CHAIN_SIGNATURES = _chain_signatures()
CHAIN_EXPORTS = list(_CHAIN_SIGNATURES)

# the chained step with parameters shared by all dates of a pixel (include_shared/crt1d_hip_lm_shared.h): the step on the arrowhead system
# and the marginal covariances of (v_d, s); the structs of the chain, a header and a table of their own


def lm_shared_lds_bytes(nd, nv, ns):
    """``CRT_LM_SHARED_LDS_BYTES(nd, nv, ns)``: the dynamic LDS of one pixel of the shared-parameter kernels."""
    per_date = 2 * nv * nv + 4 * nv + nv * ns if nv else 1
    return 8 * (nd * per_date + 4 * nv * nv + 64 + 3 * ns * ns + 2 * nv * ns + 4 * ns)


def lm_shared_max_nd(npar, ns):
    """``crt_hip_lm_shared_max_nd``: the largest ``nd`` whose LDS fits the limit; 0 for a refused ``npar`` or ``ns``.  No library is
    loaded."""
    if not 1 <= npar <= RETRIEVE_MAX_NPAR or not 0 <= ns <= npar:
        return 0
    nv = npar - ns
    per_date = 2 * nv * nv + 4 * nv + nv * ns if nv else 1
    return (LM_CHAIN_LDS_LIMIT // 8 - (4 * nv * nv + 64 + 3 * ns * ns + 2 * nv * ns + 4 * ns)) // per_date


class CrtLmShared(ctypes.Structure):
    """``crt_lm_shared``: ``mask``, bit ``k`` set means parameter ``k`` is shared by all dates of a pixel."""

    _fields_ = [("mask", ctypes.c_uint32)]


def _shared_signatures():
    P = ctypes.POINTER
    i32, ok = ctypes.c_int32, ctypes.c_int
    return {
        "crt_hip_lm_step_shared_f64": (ok, [P(CrtLmChain), P(CrtLmShared), P(CrtLmProblem), P(CrtLmNormalBlock), i32, P(CrtLmState), _vp]),
        "crt_hip_lm_shared_covariance_f64": (ok, [P(CrtLmChain), P(CrtLmShared), i32, _vp, _vp, _vp]),
        "crt_hip_lm_shared_max_nd": (i32, [i32, i32]),
    }


_SHARED_SIGNATURES = _shared_signatures()
SHARED_EXPORTS = list(_SHARED_SIGNATURES)

# the entries a Levenberg-Marquardt loop evaluates its columns with, behind a per-column skip flag, and the decision that lets the Jacobian
# run only where the trial point will be accepted (include_mask/crt1d_hip_masked.h); again a header and a table of their own


class CrtColMask(ctypes.Structure):
    """``crt_col_mask``: ``skip`` int32 ``[ncol / unit]`` on the device, column ``c`` is skipped iff ``skip[c // unit] != 0``."""

    _fields_ = [("skip", _vp), ("unit", ctypes.c_int32)]


def _masked_signatures():
    P = ctypes.POINTER
    i32, ok, M = ctypes.c_int32, ctypes.c_int, P(CrtColMask)
    sib = lambda table, name: table[name][1]  # noqa: E731  (the sibling's arguments, then the mask)
    return {
        "crt_hip_sensor_jac_masked_f64": (ok, sib(_SENSJAC_SIGNATURES, "crt_hip_sensor_jac_f64") + [M]),
        "crt_hip_sensor_jac_series_masked_f64": (ok, sib(_SENSJAC_SERIES_SIGNATURES, "crt_hip_sensor_jac_series_f64") + [M]),
        "crt_hip_sensor_levels_masked_f64": (ok, sib(_SENSOR_SIGNATURES, "crt_hip_sensor_levels_f64") + [M]),
        "crt_hip_sensor_levels_series_masked_f64": (ok, sib(_SENSOR_SIGNATURES, "crt_hip_sensor_levels_series_f64") + [M]),
        "crt_hip_spectral_normal_masked_f64": (ok, sib(_SPECFIT_SIGNATURES, "crt_hip_spectral_normal_f64") + [M]),
        "crt_hip_spectral_normal_series_masked_f64": (ok, sib(_SPECFIT_SERIES_SIGNATURES, "crt_hip_spectral_normal_series_f64") + [M]),
        "crt_hip_lm_decide_f64": (ok, [P(CrtLmProblem), P(CrtLmObs), i32, P(CrtLmState), _vp, _vp, _vp]),
    }


_MASKED_SIGNATURES = _masked_signatures()
MASKED_EXPORTS = list(_MASKED_SIGNATURES)

# the date-by-date form of the time-series retrieval (include_seq/crt1d_hip_lm_seq.h): the sums of a Gaussian prior with a full precision
# matrix, the hand-over of a date's posterior through one random-walk gap, the backward Rauch-Tung-Striebel sweep; the chain's struct, a
# header and a table of their own


class CrtLmPriorFull(ctypes.Structure):
    """``crt_lm_prior_full``: ``ncol``, ``npar``; ``prec_stride`` 0 or ``npar (npar + 1) / 2``; ``precision [ncol or 1][ntri]`` packed
    lower triangles, ``mean [ncol][npar]``."""

    _fields_ = [("ncol", ctypes.c_int32), ("npar", ctypes.c_int32), ("prec_stride", ctypes.c_int64), ("precision", _vp), ("mean", _vp)]


def _seq_signatures():
    P = ctypes.POINTER
    i32, i64, ok = ctypes.c_int32, ctypes.c_int64, ctypes.c_int
    return {
        "crt_hip_lm_prior_block_f64": (ok, [P(CrtLmPriorFull), _vp, _vp, _vp, _vp, _vp]),
        "crt_hip_lm_predict_f64": (ok, [i32, i32, _vp, _vp, i64, _vp, _vp, _vp]),
        "crt_hip_lm_rts_f64": (ok, [P(CrtLmChain), i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    }


_SEQ_SIGNATURES = _seq_signatures()
SEQ_EXPORTS = list(_SEQ_SIGNATURES)

_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle; raises :class:`HipLibraryMissing` if not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} not found: the HIP kernels are not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C crt1d_amd/csrc`). "
            "crt1d_amd has no CPU fallback."
        )
    # torch first: it brings its own libamdhip64.so.7; ours must bind to the same runtime instance
    import torch  # noqa: F401

    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**_SIGNATURES, **_LEAF_SIGNATURES, **_SPECTRA_SIGNATURES, **_SENSOR_SIGNATURES, **_JAC_SIGNATURES,
                                      **_DLAI_SIGNATURES, **_DLEAF_SIGNATURES, **_GRAD_SIGNATURES, **_SENSJAC_SIGNATURES,
                                      **_SENSJAC_SERIES_SIGNATURES, **_RETRIEVE_SIGNATURES, **_SPECFIT_SIGNATURES,
                                      **_SPECFIT_SERIES_SIGNATURES, **_LEAFMODEL_SIGNATURES, **_LUT_SIGNATURES, **_LUT_POSTERIOR_SIGNATURES,
                                      **_CHAIN_SIGNATURES, **_SHARED_SIGNATURES, **_MASKED_SIGNATURES, **_SEQ_SIGNATURES}.items():
        f = getattr(lib, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    if lib.crt_hip_abi_version() != ABI_VERSION:
        raise HipLibraryMissing(f"{LIB_PATH}: ABI version mismatch, rebuild")
    _lib = lib
    return lib


def strerror(status):
    return load().crt_hip_strerror(int(status)).decode()


def check(status, what):
    """Translate a C-ABI status into the reference's exception conventions
    (AssertionError for shape/orientation, ValueError for bad options)."""
    if status == CRT_OK:
        return
    msg = f"{what}: {strerror(status)} (status {status})"
    if status == CRT_ERR_SHAPE:
        raise AssertionError(msg)
    if status == CRT_ERR_BAD_ARG:
        raise ValueError(msg)
    raise RuntimeError(msg)


def quad_nodes(mu_s=0.501):
    """Zenith angles (radians) at which a sampled ``G_fn`` table must be given; (NQ,) float64."""
    import numpy as np

    buf = (ctypes.c_double * NQ)()
    check(load().crt_hip_quad_nodes(float(mu_s), buf), "crt_hip_quad_nodes")
    return np.frombuffer(buf, dtype=np.float64).copy()


def leaf_pdf_nodes():
    """The Gauss-Legendre rules of ``crt_hip_g_from_pdf_f64`` on the unit interval: ``(x, w, x_mla, w_mla)``, the ``LEAF_NGL``-point rule
    of each panel of G(psi) and the ``LEAF_NMLA``-point rule of the mean leaf angle (include/crt1d_hip_leaf.h)."""
    import numpy as np

    x, w = (ctypes.c_double * LEAF_NGL)(), (ctypes.c_double * LEAF_NGL)()
    xm, wm = (ctypes.c_double * LEAF_NMLA)(), (ctypes.c_double * LEAF_NMLA)()
    check(load().crt_hip_leaf_pdf_nodes_f64(x, w, xm, wm), "crt_hip_leaf_pdf_nodes_f64")
    return tuple(np.frombuffer(b, dtype=np.float64).copy() for b in (x, w, xm, wm))


def planck_nodes():
    """The ``SPECTRA_NGL``-point Gauss-Legendre rule on the unit interval that ``CRT_LIGHT_PLANCK`` integrates the Planck radiance over a
    sub-bin with: ``(x, w)`` (include/crt1d_hip_spectra.h)."""
    import numpy as np

    x, w = (ctypes.c_double * SPECTRA_NGL)(), (ctypes.c_double * SPECTRA_NGL)()
    check(load().crt_hip_planck_nodes_f64(x, w), "crt_hip_planck_nodes_f64")
    return np.frombuffer(x, dtype=np.float64).copy(), np.frombuffer(w, dtype=np.float64).copy()
