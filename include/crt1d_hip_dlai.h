/*
 * crt1d_hip_dlai.h -- the derivative of the level spectra of crt_hip_levels_f64 with respect to the leaf area index, by forward-mode
 * differentiation inside the kernel: one column precompute, one kernel, no finite differences and no step size.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 * Every column's cumulative LAI profile is scaled as lai(s) = s * lai -- the vertical distribution stays fixed -- and the output is the
 * derivative at s = 1:
 *
 *   out.X[c][r][b] = d X[c][levels[r]][b] / d s |_(s=1),     X = I_dr, I_df_d, I_df_u, F
 *
 * i.e. dX / d ln(LAI_total); dX / dLAI_total is out / lai[c][0].  X is the quantity crt_hip_levels_f64 forms for that row:
 * I_dr' = -K_b L_j I_dr and F' = I_dr' / mu + 2 (I_df_d' + I_df_u').  K_b, mu, mu_bar, the G integrals and the optics do not depend on s.
 *
 * Schemes: 2s, g77, bf (closed forms; L_j, the total LAI and e^{-K_b L_j} of the column record are seeded with their tangents L_j, LT
 * and -K_b L_j e^{-K_b L_j}), bl (the same, and the sky term I_df0 tau_d(L_j) brings I_df0 L_j tau_d'(L_j)), n79 and zq (the tangent of the
 * tridiagonal solve with the record entries (1 - td_j), (1 - tb_j), tbcum resp. tau_d(dlai_mean), e^{-K_b dlai_mean}, e^{-K_b L_j} carrying
 * theirs).  bl, n79 and zq need tau_d'(x) = d tau_d / dx = -2 int K_b(psi) e^{-K_b(psi) x} sin psi cos psi dpsi: a small kernel behind K0
 * writes the s-tangent of every record entry the scheme's kernel reads as a SIDE RECORD behind the K0 records, from cols->lai and the
 * column's K_b at the nodes K0 uses (CRT_G_TABLE columns included), level by level: a row does not depend on which other levels are
 * selected.  bl has no upward stream: its I_df_u is written as zeros.  4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 *
 * DETERMINISM.  No atomics, no reduction across lanes: a column's result is bitwise the same alone or in any batch, and for any subset
 * of the outputs and of the levels.
 */
#ifndef CRT1D_HIP_DLAI_H
#define CRT1D_HIP_DLAI_H

#include "crt1d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest nz the tridiagonal kernel keeps in its workgroup's 160 KB of LDS: the record entries it reads as value and tangent, and the
 * sweep state of every fourth level, 16 lanes */
#define CRT_DLAI_MAX_NZ_N79 928
#define CRT_DLAI_MAX_NZ_ZQ 1135

typedef struct crt_dlai_out {
  double *I_dr, *I_df_d, *I_df_u, *F; /* each [ncol][nsel][nb] or NULL; at least one */
} crt_dlai_out;

/*
 * Workspace: the column records of crt_hip_levels_f64 at the offsets of crt_hip_workspace_bytes_nb, and the side records
 * [ncol][bl: nz | n79: 16 + 3 nz | zq: 16 + nz | else 0] behind them.  0 for an invalid scheme, a non-positive size or nsel outside
 * 1..CRT_MAX_LEVEL_SELECT.
 */
size_t crt_hip_levels_dlai_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel);

/*
 * cols, bands, opts, levels, nsel: as crt_hip_levels_f64 (levels: HOST array copied by value; CRT_G_TABLE columns and both tau_d_methods
 * of n79 included).  K0, the side precompute (bl, n79, zq) and one kernel (k_dlai or k_dlai_tri, named by crt_hip_last_kernel);
 * asynchronous on `stream`, no allocation, no synchronisation, capturable into a hipGraph after the first call.
 * opts->flags: CRT_FLAG_PRECOMPUTE_ONLY runs K0 and the side precompute; CRT_FLAG_SKIP_PRECOMPUTE skips BOTH, so it is valid only on a
 * workspace that a call of THIS entry has filled (the records of crt_hip_levels_f64 alone lack the side records).
 *
 * Status, all found before any launch, in this order of precedence (CRT_ERR_BAD_ARG and CRT_ERR_SHAPE first, for every scheme; then the
 * schemes that are not served, whatever the workspace; then the workspace; then the depth):
 *  - CRT_ERR_BAD_ARG: NULL out, all four outputs NULL, everything crt_hip_levels_f64 rejects.
 *  - CRT_ERR_UNSUPPORTED: 4s, zq_pa; n79 with nz > CRT_DLAI_MAX_NZ_N79, zq with nz > CRT_DLAI_MAX_NZ_ZQ (the band slice of a workgroup
 *    narrows from 64 to 32 to 16 lanes as nz grows: n79 up to 292 levels and zq up to 307 run whole waves, n79 up to 536 and zq up to
 *    599 run 32 lanes; every nb is served); more than 65535 band slices.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_levels_dlai_workspace_bytes.
 *  - CRT_ERR_SHAPE: as crt_hip_levels_f64 (nz < 2; n79: nz < 3).
 */
int crt_hip_levels_dlai_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                            int32_t nsel, const crt_dlai_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);

/*
 * tau_d'(L) = d tau_d / dL for n arbitrary LAI values from K_b sampled at the library's nodes: the sibling of crt_hip_tau_d_f64, same
 * arguments.  CRT_TAU_D_QUAD: the nodes and weights of the tau_d rule with the integrand factor -K_b e^{-K_b L}; CRT_TAU_D_9SKY: the
 * reference's nine angles and weights with the same factor.
 */
int crt_hip_dtau_d_f64(const double* kb_nodes, const double* L, int64_t n, int32_t method, double* out, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_DLAI_H */
