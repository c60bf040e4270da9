/*
 * crt1d_hip_jac.h -- optical-property Jacobians of the level spectra of crt_hip_levels_f64: the exact derivative of every selected row
 * with respect to the leaf reflectance, the leaf transmittance and the soil reflectance of its own band, by forward-mode differentiation
 * inside the kernel.  Bands are independent, so the Jacobian is diagonal in the band: three numbers per output element.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 *   out.X[c][r][p][b] = d X[c][levels[r]][b] / d q_p[c][b],     q_0 = leaf_r, q_1 = leaf_t, q_2 = soil_r   (CRT_JAC_NPARAM = 3)
 *
 * X is the quantity crt_hip_levels_f64 forms for that row.  With bands->col_stride == 0 the spectra are shared by the columns; the
 * derivative is still each column's own response to ITS value of the parameter.  I_dr does not depend on the optics (no output for
 * it), and every output is linear in I_dr0 and I_df0 (no Jacobian needed for those).
 *
 * Schemes: 2s, bl, g77, bf (closed forms, each selected level evaluated directly from L_j and e^{-K_b L_j} of the column record: a row's
 * bits do not depend on which other levels are selected) and n79, zq (the tangent of the tridiagonal solve, carried through the
 * block-eliminated sweep).  bl has no soil and no upward stream: its p = 2 slabs and its I_df_u slabs are written as zeros.
 * 4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch, nothing written: the tangent of 4s's pivoted 4 x 4 eigen-solve and of zq_pa's
 * regrid-and-interpolate are a follow-up.
 *
 * DETERMINISM.  No atomics, no reduction across lanes: a column's result is bitwise the same alone or in any batch, and for any subset
 * of the outputs and of the levels.
 */
#ifndef CRT1D_HIP_JAC_H
#define CRT1D_HIP_JAC_H

#include "crt1d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_JAC_NPARAM 3
/* largest nz the tridiagonal Jacobian kernel keeps in its workgroup's 160 KB of LDS (sweep state of every fourth level, 16 lanes) */
#define CRT_JAC_MAX_NZ_N79 1076
#define CRT_JAC_MAX_NZ_ZQ 1200

typedef struct crt_jac_out {
  double *I_df_d, *I_df_u, *F; /* each [ncol][nsel][3][nb] or NULL; at least one */
} crt_jac_out;

/*
 * Workspace: the column records of crt_hip_levels_f64 (crt_hip_workspace_bytes_nb) at the same offsets -- a workspace filled by that call
 * can be reused here with CRT_FLAG_SKIP_PRECOMPUTE, and the other way round -- and nothing behind them.  0 for an invalid scheme, a
 * non-positive size or nsel outside 1..CRT_MAX_LEVEL_SELECT.
 */
size_t crt_hip_levels_jac_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel);

/*
 * cols, bands, opts, levels, nsel: as crt_hip_levels_f64 (levels: HOST array copied by value; CRT_G_TABLE columns and both tau_d_methods
 * of n79 included).  opts->flags: CRT_FLAG_SKIP_PRECOMPUTE and CRT_FLAG_PRECOMPUTE_ONLY as everywhere.  K0 + one kernel (k_jac or
 * k_jac_tri, named by crt_hip_last_kernel); asynchronous on `stream`, no allocation, no synchronisation, capturable into a hipGraph after
 * the first call.
 *
 * Status, all found before any launch, in this order of precedence (CRT_ERR_BAD_ARG and CRT_ERR_SHAPE first, for every scheme; then the
 * schemes that are not served, whatever the workspace; then the workspace; then the depth):
 *  - CRT_ERR_BAD_ARG: NULL out, all three outputs NULL, everything crt_hip_levels_f64 rejects.
 *  - CRT_ERR_UNSUPPORTED: 4s, zq_pa; n79 with nz > CRT_JAC_MAX_NZ_N79, zq with nz > CRT_JAC_MAX_NZ_ZQ (the band slice of a workgroup
 *    narrows from 64 to 32 to 16 lanes as nz grows: n79 up to 304 levels and zq up to 311 run whole waves; every nb is served); more than 65535 band slices.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_levels_jac_workspace_bytes.
 *  - CRT_ERR_SHAPE: as crt_hip_levels_f64 (nz < 2; n79: nz < 3).
 */
int crt_hip_levels_jac_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                           int32_t nsel, const crt_jac_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_JAC_H */
