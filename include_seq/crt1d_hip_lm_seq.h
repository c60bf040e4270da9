/*
 * crt1d_hip_lm_seq.h -- the date-by-date (sequential) form of the time-series retrieval of crt1d_hip_lm_chain.h: a Gaussian prior with a
 * FULL precision matrix as one more block of sums of the Levenberg-Marquardt step, the hand-over of one date's posterior as the next
 * date's prior through one random-walk gap, and the backward Rauch-Tung-Striebel (RTS) sweep over the filtered dates.  Three launching
 * entries: k_lm_prior_block, k_lm_predict, k_lm_rts.  The on-chip state of each is O(npar^2) per column or pixel whatever nd is: there
 * is no limit on the length of a series.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol sets of
 * the other headers and CRT_ABI_VERSION stay what they are.  The entries are asynchronous on `stream`, allocate nothing, never
 * synchronise, use no atomics, find every argument error before any launch and are capturable into a hipGraph.
 *
 * NOTATION.  ntri = npar (npar + 1) / 2.  A packed matrix is the lower triangle row by row, as crt_lm_state.A: entry (i, j), j <= i, at
 * i (i + 1) / 2 + j; the upper triangle is implied.  S(i, j) below reads entry (max(i, j), min(i, j)) of such a triangle.  Every product,
 * sum, quotient and square root named below is one separately rounded fp64 operation (no fused multiply-add); "a running sum" starts
 * at +0 and adds its terms one by one in the order stated.  Every order is a function of npar only, never of ncol, npix, nd or the
 * index of the column: the result of a column (of a pixel for k_lm_rts) is bitwise the same alone or in any batch.
 *
 * THE SCALED CHOLESKY of a packed matrix E (the one of crt_hip_lm_step_f64 and crt_hip_lm_covariance_f64, with lam = 0):
 *     dead_k = E_kk <= 0;  s_k = dead_k ? 1 : 1 / sqrt(E_kk);  Ms_ij = (E_ij * s_i) * s_j (+ 1 on the diagonal of a dead k), j <= i;
 *     L_jj = sqrt(Ms_jj - t_jj), L_ij = (Ms_ij - t_ij) / L_jj with t_ij the running sum of L_ik * L_jk, k = 0 .. j - 1.
 * A PIVOT is Ms_jj - t_jj; it "fails" when L_jj is not a finite number > 0.  solve(b) is the forward substitution z_j = (b_j - u_j) /
 * L_jj, u_j the running sum of L_jk * z_k, k ascending, then the backward one x_j = (z_j - v_j) / L_jj, v_j the running sum of
 * L_kj * x_k, k = j + 1 .. npar - 1 ascending.
 */
#ifndef CRT1D_HIP_LM_SEQ_H
#define CRT1D_HIP_LM_SEQ_H

#include "crt1d_hip.h"
#include "crt1d_hip_retrieve.h"
#include "crt1d_hip_lm_chain.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_lm_prior_full {
  int32_t ncol, npar;      /* ncol >= 1; npar in 1..CRT_RETRIEVE_MAX_NPAR */
  int64_t prec_stride;     /* 0: one matrix for every column; else npar (npar + 1) / 2 */
  const double* precision; /* [ncol or 1][ntri] packed; the upper triangle is implied */
  const double* mean;      /* [ncol][npar] */
} crt_lm_prior_full;

/*
 * k_lm_prior_block, one launch, one wave per column: the sums of the Gaussian prior N(mean, precision^-1) at the trial point, as one
 * crt_lm_normal_block.  With P the column's precision:
 *     d_j = p_trial_j - mean_j;
 *     v_i = the running sum of S(i, j) * d_j, j = 0 .. npar - 1;
 *     A   = the bits of P (ntri entries);   g_i = v_i;   c2 = the running sum of d_i * v_i, i = 0 .. npar - 1.
 * Fed to crt_hip_lm_step_normal_f64 as one more block it adds 0.5 (p - m)^T P (p - m) to the cost and P to the stored normal matrix, so
 * that crt_hip_lm_covariance_f64 on the state is the posterior covariance, prior included.  A block of +0 (precision all +0, any finite
 * mean) adds +0 to every sum.
 * CRT_ERR_BAD_ARG: NULL pr, precision, mean, p_trial, A, g or c2; ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; prec_stride neither 0
 * nor ntri.
 */
int crt_hip_lm_prior_block_f64(const crt_lm_prior_full* pr, const double* p_trial, double* A, double* g, double* c2, crt_stream_t stream);

/*
 * k_lm_predict, one launch, one wave per column: the posterior precision A [ncol][ntri] of one date pushed through one random-walk gap
 * with the weights w = inv_sigma_dyn [ncol or 1][npar] (dyn_stride npar or 0; finite, >= 0; the meaning of crt_lm_chain's):
 *     precision = (A^-1 + W^-1)^-1,   W = diag(w_k * w_k),
 * formed as the PRODUCT W M^-1 A with M = A + W, never as the difference W - W M^-1 W (which loses the digits of w^2 / A for a stiff
 * parameter):
 *     q_k = w_k * w_k;  E = A with E_kk = A_kk + q_k;  the scaled Cholesky of E;
 *     column j of Y = M^-1 A:  b_k = S_A(k, j) * s_k;  x = solve(b);  Y_kj = x_k * s_k;
 *     precision_ij = 0.5 * (q_i * Y_ij + q_j * Y_ji),  j <= i.
 * Entries that are zero whatever the roundings say: row and column k of a parameter with w_k == 0 ("forget": nothing is handed over)
 * and of a dead k (E_kk <= 0) are +0.  If a pivot fails the column's precision is all +0 and info = 1: the next date starts without a
 * prior instead of with NaN.  Otherwise info = 0.  precision may not alias A.
 * CRT_ERR_BAD_ARG: ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; NULL A, inv_sigma_dyn, precision or info; dyn_stride neither 0 nor
 * npar.
 */
int crt_hip_lm_predict_f64(int32_t ncol, int32_t npar, const double* A, const double* inv_sigma_dyn, int64_t dyn_stride, double* precision,
                           int32_t* info, crt_stream_t stream);

/*
 * k_lm_rts, one launch, one wave per pixel: the backward sweep over the filtered dates of every pixel.  chain: npix, nd >= 1 (ANY nd:
 * there is no CRT_ERR_UNSUPPORTED on length), dyn_stride, inv_sigma_dyn [npix or 1][nd - 1][npar]; columns pixel-major, c = pix * nd + t.
 * p_f [npix * nd][npar] and A_f [npix * nd][ntri]: the filtered estimate and its posterior precision (the stored normal matrix of the
 * date's retrieval, its prior block included).  p_s [npix * nd][npar], cov_s [npix * nd][npar][npar], info [npix].
 *
 * Last date: p_s = the bits of p_f; cov_s what crt_hip_lm_covariance_f64 gives for that A_f, bit for bit (the scaled Cholesky of A_f,
 * column j by solve(e_j): cov_kj = (x_k * s_k) * s_j; a dead k or j: +inf on the diagonal, 0 elsewhere).  C = cov_s of that date.
 * For t = nd - 2 .. 0, with w the weights of the gap between t and t + 1, C = cov_s of t + 1 (all npar^2 entries) and p+ = p_s of t + 1:
 *     q_k = w_k * w_k;  E = A_f,t with E_kk = A_kk + q_k;  the scaled Cholesky of E;
 *     column j of M^-1:  x = solve(e_j);  Mi_kj = (x_k * s_k) * s_j;            G_kj = Mi_kj * q_j            (G = M^-1 W)
 *     d_j = p+_j - p_f,t,j;   p_s,t,i = p_f,t,i + (the running sum of G_ij * d_j, j ascending)
 *     T_ik = the running sum of G_ij * C_jk, j ascending;
 *     cov_s,t,ik = cov_s,t,ki = Mi_ik + (the running sum of T_ij * G_kj, j ascending),  k <= i.
 * Both updates add positive semidefinite terms; no covariance is subtracted from another.  The memory of a pixel on chip is that of one
 * date; the date loop reads p_f, A_f and the weights of one date at a time.
 * FAILURE.  Going backward, the first date t <= nd - 2 at which E has a dead diagonal or a failing pivot, or C (of t + 1) is not finite
 * (a dead entry of the last date makes it so): info = 1 + t, p_s and cov_s are NaN on all dates <= t and what was written for the later
 * dates stays valid.  Otherwise info = 0.
 * CRT_ERR_BAD_ARG: NULL chain, npix < 1, nd < 1, dyn_stride neither 0 nor (nd - 1) * npar, nd > 1 with NULL weights; npar outside
 * 1..CRT_RETRIEVE_MAX_NPAR; NULL p_f, A_f, p_s, cov_s or info.
 */
int crt_hip_lm_rts_f64(const crt_lm_chain* chain, int32_t npar, const double* p_f, const double* A_f, double* p_s, double* cov_s,
                       int32_t* info, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LM_SEQ_H */
