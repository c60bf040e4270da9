/*
 * crt1d_hip_specfit.h -- a per-column Levenberg-Marquardt retrieval from the level spectra themselves, band by band: what an imaging
 * spectrometer with hundreds of contiguous bands observes.  The step of crt1d_hip_retrieve.h never needs the Jacobian
 * [nsel * nb][npar] of such a fit, only A = J^T W J, g = J^T W r and the cost of every column; k_spec_normal forms them where the
 * tangents are formed, as crt_hip_levels_grad_f64 and crt_hip_sensor_jac_f64 contract theirs, and crt_hip_lm_step_normal_f64 is the
 * step on such sums.  A retrieval is k_retrieve_apply -> the tangent refill -> k_spec_normal -> k_lm_step_normal: nothing the size of
 * the spectrum is written (the optional model spectrum `fwd` excepted).
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol sets of
 * the other headers and CRT_ABI_VERSION stay what they are.  Both launching entries are asynchronous on `stream`, allocate nothing, never
 * synchronise, use no atomics, find every argument error before any launch and are capturable into a hipGraph.
 *
 * PARAMETER AXIS.  That of crt_hip_sensor_jac_f64: npar = ntan + (with_lai != 0) + (tangent != NULL), 1 .. CRT_RETRIEVE_MAX_NPAR: the
 * coefficients of the ntan directions of a crt_optics_dirs, then ln LAI, then the leaf-angle direction.
 *
 * THE SUMS.  With X[c][r][b] the model spectrum of an observed key at level levels[r] and X'_i its derivative along parameter i (exactly
 * what crt_hip_levels_jac_f64 contracted with the directions in the order leaf_r, leaf_t, soil_r, crt_hip_levels_dlai_f64 and
 * crt_hip_levels_dleaf_f64 give: the kernel instantiates the per-band maths those kernels instantiate), a row o = (key, r, b) with
 * s = inv_sigma[key][c][r][b] (NULL: 1) forms, each rounded on its own,
 *     w_i = X'_i * s,   r = (X - y) * s
 * and then adds the products w_i * w_j to A_ij (j <= i), w_i * r to g_i and r * r to c2.  A row with s == 0 is skipped altogether: its y
 * may be NaN.  I_dr does not depend on the optics (its w_i are zero along the directions); bl has no soil and no upward stream.
 * X -- and with it r, c2 and fwd -- comes from one primal evaluation of its own and has the same bits whichever parameters are asked for
 * and whether or not fwd is written; it is the closed form the derivative kernels differentiate, which differs from what
 * crt_hip_levels_f64 writes by a few rounding errors (that kernel advances its exponentials by recurrence).
 *
 * SCHEMES.  2s, bl, g77, bf -- the closed forms.  n79, zq, 4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 *
 * LDS LIMIT.  A lane keeps (npar + 1) doubles of every (observed key, level) in LDS: nkey * nsel * (npar + 1) rows of one double per lane.
 * A workgroup owns one column and one slice of `per` consecutive bands; the slice is the widest of 256, 128, 64 lanes whose rows fit the
 * workgroup's 160 KB less 4 KB, and the bands are divided evenly over ceil(nb / width) slices.  A configuration fits iff
 *     nkey * nsel * (npar + 1) <= 312
 * (nkey = the observed keys); beyond it the call is CRT_ERR_UNSUPPORTED.
 *
 * SUMMATION CONTRACT.  No atomics.  The order of every sum is a function of (nb, nsel, the observed keys, npar, the slice width) only --
 * never of ncol, the column index, another column's inv_sigma, or whether fwd is written.  Lane l of a slice owns band slice * per + l.
 * Every one of the (npar + 1)(npar + 2) / 2 entries of (A | g | c2) -- the lower triangle of the (npar + 1) x (npar + 1) matrix of products of
 * (w_0 .. w_{npar-1}, r), row by row -- is formed on its own: the lane adds its products to a sum that starts at +0 in the order (key in the
 * order I_dr, I_df_d, I_df_u, F; level ascending), a skipped row adding a product of zeros, which changes no bit; the 64 lane sums of a wave
 * are added by a butterfly (partners at distance 32, 16, 8, 4, 2, 1), the wave sums in ascending wave order, and, where there are
 * several slices, the slice sums in ascending slice order, starting from slice 0's bits.  A lane without a band contributes +0.
 * Products and sums are separately rounded fp64 operations.
 */
#ifndef CRT1D_HIP_SPECFIT_H
#define CRT1D_HIP_SPECFIT_H

#include "crt1d_hip.h"
#include "crt1d_hip_dleaf.h"
#include "crt1d_hip_retrieve.h"
#include "crt1d_hip_sensjac.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_spec_obs { /* the observed level spectra, each [ncol][nsel][nb] */
  const double *y_I_dr, *y_I_df_d, *y_I_df_u, *y_F; /* NULL: the key is not observed; at least one */
  const double *inv_sigma_I_dr, *inv_sigma_I_df_d, *inv_sigma_I_df_u, *inv_sigma_F; /* NULL: ones; 0: the row is skipped */
} crt_spec_obs;

typedef struct crt_spec_normal_out {
  double* A;  /* [ncol][npar (npar + 1) / 2] the lower triangle row by row, as in crt_lm_state */
  double* g;  /* [ncol][npar] */
  double* c2; /* [ncol] sum of r^2, without the factor 1/2 */
  double *fwd_I_dr, *fwd_I_df_d, *fwd_I_df_u, *fwd_F; /* optional: the model spectrum X [ncol][nsel][nb]; NULL: not written */
} crt_spec_normal_out;

typedef struct crt_lm_normal_block { /* the sums of one evaluation at p_trial */
  const double* A;  /* [ncol][npar (npar + 1) / 2] */
  const double* g;  /* [ncol][npar] */
  const double* c2; /* [ncol] */
} crt_lm_normal_block;

/*
 * Workspace: the column records of crt_hip_levels_f64 at the offsets of crt_hip_workspace_bytes_nb come FIRST (a
 * CRT_FLAG_SKIP_PRECOMPUTE call of another entry can share them), then the side records of crt_hip_levels_dlai_f64 and
 * crt_hip_levels_dleaf_f64 as in crt_hip_sensor_jac_workspace_bytes, then, with S = ceil(nb / width) > 1 band slices, the slice sums
 * [ncol][S][(npar + 1)(npar + 2) / 2].  nkey: the number of observed keys.  0 for an invalid scheme, a non-positive size, nsel outside
 * 1..CRT_MAX_LEVEL_SELECT, nkey outside 1..4 or npar outside 1..CRT_RETRIEVE_MAX_NPAR.
 */
size_t crt_hip_spectral_normal_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel, int32_t nkey, int32_t npar);

/*
 * cols, bands, opts, levels, nsel, dirs, with_lai, tangent, workspace: as crt_hip_sensor_jac_f64 (levels: HOST array copied by value;
 * dirs NULL stands for ntan = 0; opts->flags as there).  K0, the side precomputes the requested columns need, k_spec_normal and, with
 * several band slices, k_spec_normal_finish; crt_hip_last_kernel names them.
 *
 * Status, all found before any launch, in the order of precedence of crt_hip_sensor_jac_f64:
 *  - CRT_ERR_BAD_ARG: NULL obs, no key observed; NULL out, out->A, out->g or out->c2; ntan outside 0..CRT_SENSJAC_MAX_NTAN, ntan > 0 with
 *    all three direction pointers NULL, col_stride neither 0 nor ntan * nb; npar == 0; tangent without dg_table or dg_at_psi; everything
 *    crt_hip_levels_f64 rejects.
 *  - CRT_ERR_SHAPE: as crt_hip_levels_f64 (nz < 2).
 *  - CRT_ERR_UNSUPPORTED: n79, zq, 4s, zq_pa, whatever the workspace.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_spectral_normal_workspace_bytes.
 *  - CRT_ERR_UNSUPPORTED: nkey * nsel * (npar + 1) > 312 (the LDS LIMIT above); more than 65535 band slices.  Nothing is written.
 */
int crt_hip_spectral_normal_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                                int32_t nsel, const crt_optics_dirs* dirs, int with_lai, const crt_leaf_tangent* tangent,
                                const crt_spec_obs* obs, const crt_spec_normal_out* out, void* workspace, size_t workspace_bytes,
                                crt_stream_t stream);

/*
 * k_lm_step_normal, one launch: THE STEP of crt1d_hip_retrieve.h for every column, except that no rows are read: the caller supplies the
 * sums of the trial point as nblk blocks (HOST array, copied by value), e.g. what crt_hip_spectral_normal_f64 wrote.  Every entry of
 * (A | g | c2) starts from block 0's bits and the blocks 1, 2, ... are added in ascending order, then the prior rows in ascending k exactly
 * as k_lm_step adds them to its running sums; cost_t = 0.5 * c2.  Accepted: the summed A and g become the state's; rejected: they are
 * dropped.  Everything else -- one wave per column, a column that is not running is not touched, the status codes, the solve -- is
 * k_lm_step's: fed with the sums k_lm_step formed from rows, every state array gets k_lm_step's bits.  crt_hip_lm_covariance_f64 works on the
 * state unchanged.
 * CRT_ERR_BAD_ARG: NULL prob, blocks or state; ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; nblk outside 1..CRT_LM_MAX_BLOCKS; a block
 * with NULL A, g or c2; the option and state checks of crt_hip_lm_step_f64.
 */
int crt_hip_lm_step_normal_f64(const crt_lm_problem* prob, const crt_lm_normal_block* blocks, int32_t nblk, const crt_lm_state* state,
                               crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_SPECFIT_H */
