/*
 * crt1d_hip_masked.h -- the entries a Levenberg-Marquardt loop evaluates its columns with, behind a per-column skip flag, and the decision
 * that lets the Jacobian run only where the trial point will be accepted.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h, of every other extension header and CRT_ABI_VERSION stay what they are.  Every struct but crt_col_mask is the sibling's.
 *
 * THE MASK.  Column c is skipped iff skip[c / unit] != 0.  unit is 1, or nd where the columns are (pixel, date) pairs of a chain
 * (crt1d_hip_lm_chain.h) and the flags are per pixel.  The status array of a crt_lm_state serves directly as skip: CRT_LM_RUNNING == 0.
 * The mask is written by an earlier kernel on the same stream; stream order is the only visibility relied on -- no fence, no atomic.  It
 * is read at every call: a captured hipGraph replays with whatever the array holds then.
 *
 * THE SIX MASKED ENTRIES.  Each takes the arguments of its plain sibling and a trailing mask:
 *
 *  - every workgroup of a skipped column returns before it reads any input of that column and before any barrier.  The test is uniform
 *    for the workgroup: the column is the workgroup's first grid coordinate on the per-step grids and on the series grids alike.
 *  - a skipped column's entries of every output (the model spectra `fwd_*` and the per-step sums A_t / g_t / c2_t of the spectral entries
 *    included) and of the slice partial sums in the workspace keep their bits.  The finish kernels (k_sens_finish, k_sens_jac_finish,
 *    k_spec_normal_finish, k_spec_normal_series_finish) have a masked form with one test per thread: an element of a skipped column is
 *    neither read nor written.
 *  - an evaluated column's outputs are bitwise those of the plain entry, in any mix of skipped and evaluated neighbours: it runs the
 *    body its sibling runs, and no column reads another's data.
 *  - mask == NULL or mask->skip == NULL: the launches and the bits of the plain entry, and its crt_hip_last_kernel report (unit is not
 *    looked at).  With a mask the report names the masked kernels: k_lev_sens_masked, k_lev_sens_series_masked, k_sens_jac_masked,
 *    k_sens_jac_series_masked, k_spec_normal_masked, k_spec_normal_series_masked and their *_finish_masked.
 *  - K0 and the side precomputes (k_colpre, k_colsun, k_dlai_side, k_dleaf_side) run UNMASKED, on every column: they are 0.03-0.1 ms of a
 *    1.2-1.9 ms step, and a record that is always current keeps CRT_FLAG_SKIP_PRECOMPUTE valid for whatever runs next on the workspace.
 *  - schemes: 2s, bl, g77 and bf, float64.  n79, zq, 4s and zq_pa are CRT_ERR_UNSUPPORTED -- for the two sensor-level entries too, whose
 *    siblings serve them -- after the argument errors (CRT_ERR_BAD_ARG, CRT_ERR_SHAPE) and whatever the workspace, the place the sensor
 *    Jacobian gives them.
 *  - status: the sibling's, in the sibling's order of precedence.  In addition, with a non-NULL skip, unit < 1 or ncol % unit != 0 is
 *    CRT_ERR_BAD_ARG.  Everything is found before any launch.
 *  - asynchronous on `stream`, no allocation, no synchronisation, capturable into a hipGraph after the first call.  Workspace: the
 *    sibling's query.
 *
 * The masked kernels are instantiations of their own beside the plain ones, with the mask as their LAST kernel argument: the plain
 * kernels keep their argument layout and their device code.
 */
#ifndef CRT1D_HIP_MASKED_H
#define CRT1D_HIP_MASKED_H

#include "crt1d_hip.h"
#include "crt1d_hip_retrieve.h"
#include "crt1d_hip_sensjac_series.h"
#include "crt1d_hip_specfit.h"
#include "series/crt1d_hip_specfit_series.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_col_mask {
  const int32_t* skip; /* [ncol / unit] on the device; column c is skipped iff skip[c / unit] != 0 */
  int32_t unit;        /* >= 1, divides ncol */
} crt_col_mask;

int crt_hip_sensor_jac_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                                  int32_t nsel, const crt_sensor_set* sensors, const crt_optics_dirs* dirs, int with_lai,
                                  const crt_leaf_tangent* tangent, const crt_sensjac_out* out, void* workspace, size_t workspace_bytes,
                                  crt_stream_t stream, const crt_col_mask* mask);

int crt_hip_sensor_jac_series_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                         const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                         const crt_optics_dirs* dirs, int with_lai, const crt_leaf_tangent_series* tangent,
                                         const crt_sensjac_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                                         const crt_col_mask* mask);

int crt_hip_sensor_levels_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                                     int32_t nsel, const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace,
                                     size_t workspace_bytes, crt_stream_t stream, const crt_col_mask* mask);

int crt_hip_sensor_levels_series_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                            const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                            const crt_sensor_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                                            const crt_col_mask* mask);

int crt_hip_spectral_normal_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                                       const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs, int with_lai,
                                       const crt_leaf_tangent* tangent, const crt_spec_obs* obs, const crt_spec_normal_out* out, void* workspace,
                                       size_t workspace_bytes, crt_stream_t stream, const crt_col_mask* mask);

int crt_hip_spectral_normal_series_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                              const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs,
                                              int with_lai, const crt_leaf_tangent_series* tangent, const crt_spec_obs* obs,
                                              const crt_spec_series_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                                              const crt_col_mask* mask);

/*
 * k_lm_decide, one launch: what crt_hip_lm_step_f64 will decide on the same inputs, without the Jacobian.  It reads f, y, inv_sigma,
 * p_trial, the prior, cost and status; it never reads J (obs[].J must still be non-NULL: the argument errors are those of the step) and
 * writes no state.  For a column with status == CRT_LM_RUNNING:
 *   cost_t[c]   = the cost of THE STEP, item 1 (crt1d_hip_retrieve.h), under its summation contract -- the running sum of r_o * r_o over
 *                 the rows of block 0, 1, ... in ascending order, then d_k * d_k over the prior rows, times 0.5 -- formed by the device
 *                 functions k_lm_step stages its residuals and extends its cost entry with: the same bits;
 *   skip_jac[c] = !(cost_t[c] < cost[c])  (NaN: 1; cost == +inf, the first step: 0 for a finite cost_t).
 * A column that is not running: skip_jac[c] = 1 and cost_t[c] keeps its bits.  So a following crt_hip_lm_step_f64 accepts exactly the
 * columns with skip_jac == 0, and J is needed for no other column: a rejected trial point leaves p, cost, A and g with their bits.
 * CRT_ERR_BAD_ARG: everything crt_hip_lm_step_f64 rejects; NULL skip_jac or cost_t.  obs: HOST array, copied by value.
 */
int crt_hip_lm_decide_f64(const crt_lm_problem* prob, const crt_lm_obs* obs, int32_t nblk, const crt_lm_state* state,
                          int32_t* skip_jac /*[ncol]*/, double* cost_t /*[ncol]*/, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_MASKED_H */
