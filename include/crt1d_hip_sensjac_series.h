/*
 * crt1d_hip_sensjac_series.h -- the Jacobian of crt1d_hip_sensjac.h over a sun-angle series: d(sensor-band sums) / d(parameters) for nt sun
 * states (psi, I_dr0, I_df0) of every column on one canopy with one parameter vector, in one call.  What a retrieval from a diurnal course
 * consumes: [nt * nobs] x [npar] per column.  The canopy part of the column precompute and the side precomputes of the LAI and the
 * leaf-angle derivative run once per column, not once per sun state; the sun records, the Jacobian kernel and the finish kernel serve
 * every (column, t).
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol sets of
 * the other headers and CRT_ABI_VERSION stay what they are.
 *
 * OUTPUT.  out.X is [ncol][nt][nsel][nsens][npar], the parameter axis of crt_hip_sensor_jac_f64: ntan directions, then ln LAI, then the
 * leaf angle.
 *
 * SLICE CONTRACT.  Slice [:, t] is BITWISE what crt_hip_sensor_jac_f64 writes with cols->psi[c] = sun->psi[c][t] (g_at_psi likewise),
 * the incoming spectra of step t and a crt_leaf_tangent whose dg_at_psi[c] is dg_at_psi[c][t] of the series tangent.  cols->psi,
 * cols->g_at_psi and bands->I_dr0 / I_df0 are not read, as in the other series entries.  The directions do not depend on the sun: they are
 * shared over t.  The summation contract of crt1d_hip_sensjac.h holds for every (column, t): same band slices, same lanes, same order.
 *
 * SCHEMES.  2s, bl, g77, bf.  n79, zq, 4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 */
#ifndef CRT1D_HIP_SENSJAC_SERIES_H
#define CRT1D_HIP_SENSJAC_SERIES_H

#include "crt1d_hip_sensjac.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_leaf_tangent_series { /* crt_leaf_tangent with the sun-angle entry per sun state */
  const double* dg_table;                /* [ncol][CRT_NQ] */
  const double* dg_at_psi;               /* [ncol][nt]: dG at sun->psi[c][t] */
  const double* dmla;                    /* [ncol] or NULL */
} crt_leaf_tangent_series;

/*
 * Workspace, in this order: the records of crt_hip_levels_series_workspace_bytes(scheme, ncol, nz, nt) FIRST and at the same offsets
 * (canopy records, then sun records) -- a crt_hip_sensor_levels_series_f64 call can run afterwards on the same workspace with
 * CRT_FLAG_SKIP_PRECOMPUTE and gives the forward sums of the residual, bitwise those of a stand-alone call (its own partial sums lie behind
 * the records: the workspace must hold crt_hip_sensor_series_workspace_bytes too, and the side records below are overwritten where there
 * are several band slices, so run this entry with the precompute again afterwards); the side records of the LAI derivative
 * [ncol][bl: nz | else 0]; those of the leaf-angle derivative [ncol][bl: 16 + nz | else 16]; the slice partial sums
 * [ncol][nt][band slices][nsel][nsens][npar][4], only with several slices.  The same for every subset of the outputs and for every split of
 * npar.  0 for an invalid scheme, a non-positive size, nt < 1, nsel outside 1..CRT_MAX_LEVEL_SELECT, nsens outside 1..CRT_MAX_SENSOR_BANDS,
 * npar outside 1..CRT_SENSJAC_MAX_NTAN + 2, or a size beyond size_t.
 */
size_t crt_hip_sensor_jac_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt, int32_t nsel, int32_t nsens,
                                                 int32_t npar);

/*
 * Arguments as crt_hip_sensor_jac_f64, with `sun` as in crt_hip_sensor_levels_series_f64 and the series form of the tangent.  Kernels:
 * k_colpre<canopy> + k_colsun, the side precomputes the requested columns need (k_dlai_side: LAI of bl; k_dleaf_side<canopy>: leaf angle;
 * once per column), k_sens_jac_series -- one workgroup per (column, band slice, sun state) -- and, with several band slices,
 * k_sens_jac_finish; crt_hip_last_kernel names them, the series kernel with nt=.  The leaf-angle side record does not follow the sun: the
 * series kernel forms K_b' = dg_at_psi[c][t] / cos psi[c][t] itself, by the division k_dleaf_side uses.  Asynchronous on `stream`, no
 * allocation, no synchronisation, capturable into a hipGraph after the first call.  opts->flags: CRT_FLAG_PRECOMPUTE_ONLY runs the column
 * and the side precomputes; CRT_FLAG_SKIP_PRECOMPUTE skips them all (valid only on a workspace that a call of THIS entry has filled with
 * the same sun angles, the same tangent and the same parameter columns).
 *
 * Status, all found before any launch and with nothing written, in this order of precedence:
 *  - CRT_ERR_BAD_ARG: everything crt_hip_sensor_jac_f64 reports as such (its cols->psi and bands->I_dr0 / I_df0 excepted); NULL sun,
 *    nt < 1, whatever crt_hip_sensor_levels_series_f64 rejects about sun; tangent without dg_table or dg_at_psi.
 *  - CRT_ERR_SHAPE: nz < 2.
 *  - CRT_ERR_UNSUPPORTED: n79, zq, 4s, zq_pa, whatever the workspace.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_sensor_jac_series_workspace_bytes.
 *  - CRT_ERR_UNSUPPORTED: nsel * max(3 npar, 4) > 312 (the staging rows do not fit the LDS); a grid that does not fit
 *    (band slices * ceil(nt / 65535) > 65535); a finish grid beyond 2^31 blocks.
 */
int crt_hip_sensor_jac_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                  const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                  const crt_optics_dirs* dirs, int with_lai, const crt_leaf_tangent_series* tangent,
                                  const crt_sensjac_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);

/*
 * crt_hip_g_dparam_f64 with the sun-angle lane evaluated for every sun state: dg_table [ncol][CRT_NQ] is bitwise that entry's, and
 * dg_at_psi[c][t] bitwise what it writes for psi = sun->psi[c][t].  Reads sun->nt and sun->psi only.  CRT_ERR_BAD_ARG: a NULL pointer,
 * ncol < 1, nt < 1, NULL g_kind;  CRT_ERR_UNSUPPORTED: nt beyond the grid (55 + 65534 * 192 sun states per column).
 */
int crt_hip_g_dparam_series_f64(const crt_columns* cols, const crt_sun_series* sun, double* dg_table /*[ncol][CRT_NQ]*/,
                                double* dg_at_psi /*[ncol][nt]*/, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_SENSJAC_SERIES_H */
