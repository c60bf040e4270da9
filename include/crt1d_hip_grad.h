/*
 * crt1d_hip_grad.h -- the gradient of a weighted sum of the level spectra of crt_hip_levels_f64 with respect to the optics, the leaf area
 * index and a leaf-angle direction: the three derivatives of crt1d_hip_jac.h, crt1d_hip_dlai.h and crt1d_hip_dleaf.h contracted with one
 * set of weights inside one kernel, behind one column precompute.  This is what a retrieval that minimises a scalar misfit needs:
 * with w.X[c][r][b] = d loss / d X[c][levels[r]][b] the outputs are d loss / d (leaf_r, leaf_t, soil_r, ln LAI, leaf-angle parameter).
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 * With X' denoting exactly what crt_hip_levels_jac_f64, crt_hip_levels_dlai_f64 and crt_hip_levels_dleaf_f64 write for the same inputs
 * (the same tangent bits: the kernel instantiates the per-band maths those kernels instantiate),
 *
 *   out.q[c][b]  = sum_X sum_r w.X[c][r][b] dX[c][levels[r]][b] / dq[c][b]        q = leaf_r, leaf_t, soil_r;  X = I_df_d, I_df_u, F
 *   out.lai[c]   = sum_X sum_r sum_b w.X[c][r][b] dX[c][levels[r]][b] / d ln LAI  X = I_dr, I_df_d, I_df_u, F
 *   out.leaf[c]  = the same sum along `tangent`
 *
 * I_dr does not depend on the optics: w.I_dr enters lai and leaf only.  bl has no soil and no upward stream: its soil_r is written as
 * zeros and its w.I_df_u is not read.  With bands->col_stride == 0 (one set of spectra for all columns) the optics outputs are still
 * [ncol][nb]: each row is that column's own response, and the gradient of the shared spectrum is their sum over columns.  The outputs are
 * linear in I_dr0 and I_df0; gradients with respect to those are not formed.
 *
 * SCHEMES.  2s, bl, g77, bf -- the closed forms.  n79, zq, 4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 *
 * DETERMINISM.  No atomics.  A lane is a band and adds its terms in the order (level, quantity); the sums over bands of lai and leaf are
 * a fixed-order wave and workgroup sum, then the band slices in ascending order.  A column's result is bitwise the same alone or in any
 * batch, and for any subset of the requested outputs.
 */
#ifndef CRT1D_HIP_GRAD_H
#define CRT1D_HIP_GRAD_H

#include "crt1d_hip.h"
#include "crt1d_hip_dleaf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_grad_weights {
  const double* I_dr;   /* each [ncol][nsel][nb] or NULL; at least one */
  const double* I_df_d;
  const double* I_df_u;
  const double* F;
} crt_grad_weights;

typedef struct crt_grad_out {
  double* leaf_r; /* each [ncol][nb] or NULL */
  double* leaf_t;
  double* soil_r;
  double* lai;    /* [ncol] or NULL: per ln LAI, the convention of crt_hip_levels_dlai_f64 */
  double* leaf;   /* [ncol] or NULL: along `tangent`, which must then be given */
} crt_grad_out;   /* at least one */

/*
 * Workspace: the column records of crt_hip_levels_f64 at the offsets of crt_hip_workspace_bytes_nb, then the side records of
 * crt_hip_levels_dlai_f64 [ncol][bl: nz | else 0], those of crt_hip_levels_dleaf_f64 [ncol][bl: 16 + nz | else 16], and the partial sums
 * [ncol][band slices][2] of lai and leaf (a slice holds at most 256 bands).  The same for every subset of the outputs.  0 for an
 * invalid scheme, a non-positive size or nsel outside 1..CRT_MAX_LEVEL_SELECT.
 */
size_t crt_hip_levels_grad_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel);

/*
 * cols, bands, opts, levels, nsel: as crt_hip_levels_f64 (levels: HOST array copied by value; CRT_G_TABLE columns included).  K0, the
 * side precomputes the requested outputs need (k_dlai_side: lai of bl; k_dleaf_side: leaf), k_grad and, with several band slices and
 * lai or leaf requested, k_grad_finish; crt_hip_last_kernel names them.  Asynchronous on `stream`, no allocation, no synchronisation,
 * capturable into a hipGraph after the first call.  opts->flags: CRT_FLAG_PRECOMPUTE_ONLY runs K0 and the side precomputes;
 * CRT_FLAG_SKIP_PRECOMPUTE skips them all, so it is valid only on a workspace that a call of THIS entry has filled with the same tangent
 * and the same outputs requested.
 *
 * Status, all found before any launch, in the order of precedence of crt_hip_levels_dleaf_f64:
 *  - CRT_ERR_BAD_ARG: NULL w, all four weights NULL; NULL out, all five outputs NULL; out->leaf without tangent, dg_table or dg_at_psi;
 *    everything crt_hip_levels_f64 rejects.
 *  - CRT_ERR_SHAPE: as crt_hip_levels_f64 (nz < 2; n79: nz < 3).
 *  - CRT_ERR_UNSUPPORTED: n79, zq, 4s, zq_pa, whatever the workspace; more than 65535 band slices.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_levels_grad_workspace_bytes.
 */
int crt_hip_levels_grad_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                            int32_t nsel, const crt_grad_weights* w, const crt_leaf_tangent* tangent, const crt_grad_out* out,
                            void* workspace, size_t workspace_bytes, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_GRAD_H */
