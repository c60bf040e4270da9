/*
 * crt1d_hip_specfit_series.h -- the spectral normal equations of crt1d_hip_specfit.h over a sun-angle series: A = J^T W J, g = J^T W r and
 * c2 = sum r^2 of the per-band misfit of the level spectra of nt sun states (psi, I_dr0, I_df0) of every column, on one canopy with one
 * parameter vector, summed over the sun states, in one call.  What a retrieval from the diurnal course of a tower spectrometer consumes:
 * from one sun angle the LAI and the leaf-angle parameter are barely separable, the course separates them.  The canopy part of the column
 * precompute and the side precomputes of the LAI and of the leaf-angle derivative run once per column, not once per sun state; the sun
 * records, the kernel and the finish kernel serve every (column, t).  crt_hip_lm_step_normal_f64 takes the sums as ONE block, whatever nt.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), a header and a symbol table of its own.  It
 * lies in include/series/ and is included as "series/crt1d_hip_specfit_series.h" with include/ on the include path; it belongs to the
 * public interface like the headers beside crt1d_hip.h (the complete list, directories included: tests/test_specfit_series_cpu.py).
 *
 * ARRAYS.  obs->y_* and obs->inv_sigma_* are [ncol][nt][nsel][nb]; an inv_sigma of 0 masks a band of a sun state, whose y may be NaN; a
 * sun state that is masked completely (the night) is legal and contributes +0.  The parameter vector, the directions of crt_optics_dirs
 * and the canopy are shared over t, as in crt_hip_sensor_jac_series_f64.  cols->psi, cols->g_at_psi and bands->I_dr0 / I_df0 are not read.
 *
 * SLICE CONTRACT.  A_t[:, t], g_t[:, t], c2_t[:, t] and fwd[:, t] are BITWISE what crt_hip_spectral_normal_f64 writes with
 * cols->psi[c] = sun->psi[c][t] (g_at_psi likewise), the incoming spectra of step t, a crt_leaf_tangent whose dg_at_psi[c] is
 * dg_at_psi[c][t] of the series tangent, and the observations of step t.  Same band slices, same lanes, same order: the summation contract
 * of crt1d_hip_specfit.h holds for every (column, t).
 *
 * SUM CONTRACT.  A, g, c2 are bitwise the left-to-right sum over t of those slices, starting from the bits of t = 0 (one sun state: its
 * bits).  For nt <= CRT_LM_MAX_BLOCKS this is bitwise what k_lm_step_normal forms from nt per-step blocks.
 *
 * ORDER.  No atomics.  The order of every sum is a function of (nb, nsel, the observed keys, npar, the slice width, nt) only -- never of
 * ncol, the column index or any mask.
 *
 * SCHEMES.  2s, bl, g77, bf.  n79, zq, 4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 */
#ifndef CRT1D_HIP_SPECFIT_SERIES_H
#define CRT1D_HIP_SPECFIT_SERIES_H

#include "crt1d_hip_sensjac_series.h"
#include "crt1d_hip_specfit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_spec_series_out {
  double *A, *g, *c2;          /* [ncol][ntri], [ncol][npar], [ncol]: summed over t; all three required */
  double *A_t, *g_t, *c2_t;    /* [ncol][nt][ntri], [ncol][nt][npar], [ncol][nt]: per sun state; all NULL or all set */
  double *fwd_I_dr, *fwd_I_df_d, *fwd_I_df_u, *fwd_F;   /* [ncol][nt][nsel][nb] or NULL, observed keys only */
} crt_spec_series_out;

/*
 * Workspace, in this order: the records of crt_hip_levels_series_workspace_bytes(scheme, ncol, nz, nt) FIRST and at the same offsets (canopy
 * records, then sun records) -- a crt_hip_levels_series_f64 call with CRT_FLAG_SKIP_PRECOMPUTE can run on the same workspace --; the two
 * side records as crt_hip_sensor_jac_series_workspace_bytes lays them out ([ncol][bl: nz | else 0], then [ncol][bl: 16 + nz | else 16]);
 * the partial sums [ncol][nt][S][(npar + 1)(npar + 2) / 2] with S = ceil(nb / width) band slices.  The partial sums are always there: the
 * sum over t goes through them even with one slice.  0 for what crt_hip_spectral_normal_workspace_bytes or
 * crt_hip_levels_series_workspace_bytes return 0 for (an invalid scheme, a non-positive size, nsel outside 1..CRT_MAX_LEVEL_SELECT, nkey
 * outside 1..4, npar outside 1..CRT_RETRIEVE_MAX_NPAR), for nt < 1 and for a size beyond size_t.
 */
size_t crt_hip_spectral_normal_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt,
                                                      int32_t nsel, int32_t nkey, int32_t npar);

/*
 * Arguments as crt_hip_spectral_normal_f64, with `sun` and the series tangent as in crt_hip_sensor_jac_series_f64.  Kernels:
 * k_colpre<canopy> + k_colsun, the side precomputes the requested columns need (k_dlai_side: LAI of bl; k_dleaf_side<canopy>: leaf angle;
 * once per column), k_spec_normal_series -- one workgroup per (column, band slice, sun state) -- and k_spec_normal_series_finish;
 * crt_hip_last_kernel names the two, the first with nt=.  The leaf-angle side record does not follow the sun: the series kernel forms
 * K_b' = dg_at_psi[c][t] / cos psi[c][t] itself, by the division k_dleaf_side uses.  Asynchronous on `stream`, no allocation, no
 * synchronisation, capturable into a hipGraph after the first call.  opts->flags: CRT_FLAG_PRECOMPUTE_ONLY runs the column and the side
 * precomputes; CRT_FLAG_SKIP_PRECOMPUTE skips them all (valid only on a workspace that a call of THIS entry has filled with the same sun
 * angles, the same tangent and the same parameter columns).
 *
 * Status, all found before any launch and with nothing written, in this order of precedence:
 *  - CRT_ERR_BAD_ARG: everything crt_hip_spectral_normal_f64 reports as such (its cols->psi and bands->I_dr0 / I_df0 excepted); NULL sun,
 *    nt < 1, whatever crt_hip_levels_series_f64 rejects about sun; tangent without dg_table or dg_at_psi; A_t, g_t, c2_t partly set.
 *  - CRT_ERR_SHAPE: nz < 2.
 *  - CRT_ERR_UNSUPPORTED: n79, zq, 4s, zq_pa, whatever the workspace.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_spectral_normal_series_workspace_bytes.
 *  - CRT_ERR_UNSUPPORTED: nkey * nsel * (npar + 1) > 312 (the LDS LIMIT of crt1d_hip_specfit.h: the rows do not grow with nt); a grid that
 *    does not fit (band slices * ceil(nt / 65535) > 65535); a finish grid beyond 2^31 blocks.
 */
int crt_hip_spectral_normal_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                       const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs,
                                       int with_lai, const crt_leaf_tangent_series* tangent, const crt_spec_obs* obs,
                                       const crt_spec_series_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_SPECFIT_SERIES_H */
