/*
 * crt1d_hip_dleaf.h -- the derivative of the level spectra of crt_hip_levels_f64 along a direction of the leaf-angle distribution, by
 * forward-mode differentiation inside the kernel: one column precompute, one side precompute, one kernel, no finite differences and no
 * step size.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 * A LEAF-ANGLE DIRECTION of a column is a tangent of its G function and, for 2s, of its mean leaf angle (crt_leaf_tangent): dG at the
 * library's CRT_NQ nodes in the order of crt_hip_quad_nodes, dG at the sun angle, and dmla in degrees.  One representation serves every
 * G kind, closed-form and CRT_G_TABLE columns alike; crt_hip_g_dparam_f64 fills it with dG / d g_param for the parametric kinds.
 *
 *   out.X[c][r][b] = d X[c][levels[r]][b] along that direction,     X = I_dr, I_df_d, I_df_u, F
 *
 * with X the quantity crt_hip_levels_f64 forms for that row.  The sun angle, lai and the optics are fixed.  Tangents of the column
 * record (Kq = G_q / cos psi_q at the tau_d nodes, mu = cos psi_sun):
 *
 *   K_b' = dG(psi_sun) / mu         Kq' = dG_q / cos psi_q         mu_bar' = -sum_q w_q cos sin dG_q / G_q^2   (the order of mu_bar's sum)
 *   cos2' = -2 cos(m) sin(m) (pi / 180) dmla,  m = radians(mla)    (e^{-K_b L_j})' = -K_b' L_j e^{-K_b L_j}
 *   tau_d^th(x) = -2 sum_q w_q sin cos Kq' x e^{-Kq x}             ('9sky': the nine-angle sum with the same factor)
 *
 * 2s, g77, bf: closed forms whose header scalars K_b, mu_bar, cos^2 and whose beam fractions carry the tangent; bl the same, and the
 * sky term I_df0 tau_d(L_j) brings I_df0 tau_d^th(L_j); n79: (1 - td_j)' = -tau_d^th(D_j), (1 - tb_j)' = K_b' D_j tb_j, tbcum' as
 * e^{-K_b L_j}; zq: tau_d(dm)' = tau_d^th(dm), (e^{-K_b dm})' = -K_b' dm e^{-K_b dm}.  Then I_dr' = I_dr0 (e^{-K_b L_j})' and
 * F' = I_dr' / mu + 2 (I_df_d' + I_df_u').  A small kernel behind K0 writes the tangent of every record entry the scheme's kernel reads
 * as a SIDE RECORD behind the K0 records, level by level.  n79 and zq run the tridiagonal kernel of crt1d_hip_dlai.h on that side
 * record, so its depth limits CRT_DLAI_MAX_NZ_N79 / CRT_DLAI_MAX_NZ_ZQ and lane narrowing hold here.  bl has no upward stream: its
 * I_df_u is written as zeros.  4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 *
 * DETERMINISM.  No atomics; the one reduction (mu_bar') is a fixed-order wave sum: a column's result is bitwise the same alone or in any
 * batch, and for any subset of the outputs and of the levels.
 */
#ifndef CRT1D_HIP_DLEAF_H
#define CRT1D_HIP_DLEAF_H

#include "crt1d_hip.h"
#include "crt1d_hip_dlai.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_leaf_tangent {
  const double* dg_table;  /* [ncol][CRT_NQ] dG at the angles of crt_hip_quad_nodes(); the CRT_NQ_G4 entries are not read */
  const double* dg_at_psi; /* [ncol] dG at the sun angle cols->psi[c] */
  const double* dmla;      /* [ncol] tangent of the mean leaf angle in degrees (2s), or NULL = 0 */
} crt_leaf_tangent;

/*
 * Workspace: the column records of crt_hip_levels_f64 at the offsets of crt_hip_workspace_bytes_nb, and the side records
 * [ncol][2s, g77, bf: 16 | bl: 16 + nz | n79: 16 + 3 nz | zq: 16 + nz] behind them.  0 for an invalid scheme, a non-positive size or
 * nsel outside 1..CRT_MAX_LEVEL_SELECT.
 */
size_t crt_hip_levels_dleaf_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel);

/*
 * cols, bands, opts, levels, nsel: as crt_hip_levels_f64 (levels: HOST array copied by value; CRT_G_TABLE columns and both tau_d_methods
 * of n79 included); out: the four arrays of crt_dlai_out, each [ncol][nsel][nb] or NULL, at least one.  K0, the side precompute and one
 * kernel (k_dleaf or k_dlai_tri, named by crt_hip_last_kernel); asynchronous on `stream`, no allocation, no synchronisation, capturable
 * into a hipGraph after the first call.  opts->flags: CRT_FLAG_PRECOMPUTE_ONLY runs K0 and the side precompute;
 * CRT_FLAG_SKIP_PRECOMPUTE skips BOTH, so it is valid only on a workspace that a call of THIS entry has filled with the same tangent.
 *
 * Status, all found before any launch, in this order of precedence (CRT_ERR_BAD_ARG and CRT_ERR_SHAPE first, for every scheme; then the
 * schemes that are not served, whatever the workspace; then the workspace; then the depth):
 *  - CRT_ERR_BAD_ARG: NULL tangent, dg_table or dg_at_psi; NULL out, all four outputs NULL; everything crt_hip_levels_f64 rejects.
 *  - CRT_ERR_UNSUPPORTED: 4s, zq_pa; n79 with nz > CRT_DLAI_MAX_NZ_N79, zq with nz > CRT_DLAI_MAX_NZ_ZQ; more than 65535 band slices.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_levels_dleaf_workspace_bytes.
 *  - CRT_ERR_SHAPE: as crt_hip_levels_f64 (nz < 2; n79: nz < 3).
 */
int crt_hip_levels_dleaf_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                             int32_t nsel, const crt_leaf_tangent* tangent, const crt_dlai_out* out, void* workspace,
                             size_t workspace_bytes, crt_stream_t stream);

/*
 * dG / d g_param of every column in one launch: dg_table[ncol][CRT_NQ] at the angles of crt_hip_quad_nodes(0.501, .) (the CRT_NQ_G4
 * nodes depend on mu_s; they serve 4s only, which has no derivative kernel) and dg_at_psi[ncol] at cols->psi[c].
 * CRT_G_ELLIPSOIDAL: the exact form with the derivative of its normalisation, by a series in 1 - x^2 next to x = 1 (smooth through it);
 * CRT_G_ELLIPSOIDAL_APPROX; CRT_G_ELLIPSOIDAL_APPROX_BONAN: zero outside the clamp -0.4 < chi_l < 0.6.  Parameterless kinds and
 * CRT_G_TABLE columns get zeros.  Reads cols->ncol, psi, g_kind, g_param.
 */
int crt_hip_g_dparam_f64(const crt_columns* cols, double* dg_table, double* dg_at_psi, crt_stream_t stream);

/*
 * tau_d^th(L) = -2 sum_q w_q sin cos Kq' L e^{-Kq L} for n arbitrary LAI values, the sibling of crt_hip_dtau_d_f64: kb_nodes[CRT_NQ] and
 * dkb_nodes[CRT_NQ] are K_b and its tangent at the angles of crt_hip_quad_nodes() (device memory, like L and out).
 */
int crt_hip_dtau_d_dleaf_f64(const double* kb_nodes, const double* dkb_nodes, const double* L, int64_t n, int32_t method, double* out,
                             crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_DLEAF_H */
