/*
 * crt1d_hip_lm_chain.h -- the Levenberg-Marquardt step of crt1d_hip_retrieve.h for a time series: the nd dates of a pixel are nd columns
 * whose parameter vectors are coupled by a random-walk prior, so that the normal matrix of a pixel is block tridiagonal (nd blocks of
 * npar x npar, diagonal off-diagonal blocks).  Three launching entries: the sums of k_lm_step from sensor rows, written instead of
 * consumed (k_lm_normal); the step of a whole pixel on such sums (k_lm_step_chain); and the smoothed marginal covariances
 * (k_lm_chain_covariance).  The radiative transfer is not in here: a (pixel, date) pair is a column of every other entry, with its own
 * psi and illumination, and the caller evaluates all npix * nd columns as it does for the unchained step.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol sets of
 * the other headers and CRT_ABI_VERSION stay what they are.  The launching entries are asynchronous on `stream`, allocate nothing, never
 * synchronise, use no atomics, find every argument error before any launch and are capturable into a hipGraph.
 *
 * THE PROBLEM.  ncol = npix * nd columns, pixel-major: c = pix * nd + d.  The unknowns of a pixel are p_0 .. p_{nd-1}, each npar long,
 * npar in 1..CRT_RETRIEVE_MAX_NPAR.  inv_sigma_dyn [npix or 1][nd - 1][npar] (dyn_stride = (nd - 1) * npar or 0) holds the coupling
 * weights w_{d,k} of the gap between the dates d and d + 1; an entry 0 leaves the parameter uncoupled across that gap; the caller folds
 * the time gap into the weight.  Per pixel
 *     cost = 0.5 * (sum_d c2_d + sum_{d < nd-1} sum_k e_{d,k}^2),   e_{d,k} = (p_{d+1,k} - p_{d,k}) * w_{d,k}.
 * c2_d, A_d and g_d are the sums of date d, every entry formed exactly as k_lm_step_normal forms it: block 0's bits, then the blocks 1..
 * in ascending order, then that date's prior rows in ascending k (prob->prior / inv_sigma_prior are per column, hence per date).  The
 * pixel sum starts from c2_0's bits and adds c2_1, c2_2, ... in ascending order; the coupling terms follow with d ascending, then k
 * ascending; each e, each e * e and each sum is a separately rounded fp64 operation; cost = 0.5 * that sum.
 *
 * With coupling the normal matrix H and the gradient G of a pixel are (a neighbour that does not exist adds nothing)
 *     H_(d,k),(d,k)   = (A_d,kk + w_{d-1,k}^2) + w_{d,k}^2          (each square rounded first)
 *     H_(d,k),(d-1,k) = -(w_{d-1,k}^2)                              (the off-diagonal blocks are diagonal)
 *     G_d,k           = (g_d,k + w_{d-1,k} * e_{d-1,k}) - w_{d,k} * e_{d,k}
 * formed at solve time from the stored per-date A and g and the ACCEPTED p: the state keeps the data part only (the per-date prior
 * included).
 *
 * THE STEP is that of crt1d_hip_retrieve.h taken per pixel.  For a pixel with status == CRT_LM_RUNNING:
 *  1. cost_t as above at p_trial.  Accepted iff cost_t < cost (false for NaN); not accepted with cost == +inf: CRT_LM_FAILED_START (one
 *     NaN date fails the pixel; no counter moves).
 *     accepted: p = p_trial, A_d and g_d of every date become the state's; lam = max(lam * lam_down, lam_min); CRT_LM_CONVERGED_F if
 *       cost - cost_t < ftol * cost_t; cost = cost_t; ++naccept.
 *     rejected: p, cost, A, g keep their bits; lam = lam * lam_up; CRT_LM_STALLED once lam > lam_max; ++nreject.
 *  2. Still running: (H + lam diag H) delta = -G by a Cholesky without pivoting of the scaled matrix, n = nd * npar, row index
 *     r = d * npar + k:  s_r = 1 / sqrt(H_rr), a dead entry (H_rr <= 0) has s_r = 1;  M_rq = (H_rq * s_r) * s_q + (dead ? 1 : lam) [r == q];
 *     L_rq = (M_rq - t_rq) / L_qq and L_qq = sqrt(M_qq - t_qq), where t_rq is ONE running sum that starts at +0 and adds L_rm * L_qm for
 *     m ascending from the first column of the block of the date before r's (of r's own date for date 0) up to q - 1 -- the only columns
 *     where both rows can be non-zero; u and v below run over the same band.  That is the dense left-looking factorisation of
 *     scaled_cholesky restricted to the band; it is carried out as a block Cholesky along the chain: the sub-diagonal block B_d (rows of
 *     date d, columns of date d - 1) by npar lanes, one row each; the npar^2 sums B_d B_d^T one per lane; then below each pivot one lane
 *     per row.
 *     x_r = (-G_r) * s_r;  forward: z_r = (x_r - u_r) / L_rr with u_r one running sum from +0 over L_rm * z_m, m ascending as above;
 *     backward: y_r = (z_r - v_r) / L_rr with v_r one running sum from +0 over the rows m of the NEXT date's block ascending
 *     (L_mr * y_m), then over the rows m > k of the own block ascending;  delta_r = y_r * s_r.
 *     p_trial_r = clamp(p_r + delta_r, lo_k, hi_k); CRT_LM_CONVERGED_X if |p_trial_r - p_r| < xtol * (|p_r| + xtol) for every one of the
 *     nd * npar entries.
 *  3. A pixel that stops running in this call gets p_trial = p on every date.  A pixel that is not running on entry is not touched.
 * With nd == 1 every state array gets k_lm_step_normal's bits.  With all weights 0 the blocks decouple: the first call leaves
 * p_trial[c] bitwise what k_lm_step_normal leaves for the column c alone and cost[pix] the left-to-right sum over the dates of that
 * kernel's cost.
 *
 * STATE.  p, p_trial, A, g stay per column ([ncol] x what crt_lm_state says), so p_trial is directly what k_retrieve_apply reads;
 * cost, lam, status, naccept, nreject are [npix].
 *
 * SUMMATION CONTRACT.  No atomics.  One wave owns one pixel.  Every sum above has a fixed order that is a function of (nd, npar, nblk)
 * only, never of npix or the pixel index: a pixel's state is bitwise the same alone or in any batch.
 *
 * LDS LIMIT.  The factor blocks, the sub-diagonal blocks, the right-hand side, the scales and the diagonal of H live in dynamic LDS:
 *     CRT_LM_CHAIN_LDS_BYTES(nd, npar) = 8 * (nd * (2 npar^2 + 4 npar) + 4 npar^2 + 64)   <=   CRT_LM_CHAIN_LDS_LIMIT = 160 KiB,
 * so crt_hip_lm_chain_max_nd(npar) = (160 * 1024 / 8 - 4 npar^2 - 64) / (2 npar^2 + 4 npar), rounded down: 83 at npar = 10, 290 at 5.
 */
#ifndef CRT1D_HIP_LM_CHAIN_H
#define CRT1D_HIP_LM_CHAIN_H

#include "crt1d_hip.h"
#include "crt1d_hip_retrieve.h"
#include "crt1d_hip_specfit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_LM_CHAIN_LDS_LIMIT (160 * 1024)
#define CRT_LM_CHAIN_LDS_BYTES(nd, npar) \
  (8 * ((long long)(nd) * (2 * (npar) * (npar) + 4 * (npar)) + 4 * (npar) * (npar) + 64))

typedef struct crt_lm_chain {
  int32_t npix, nd;            /* >= 1 each; the problem's ncol == npix * nd */
  int64_t dyn_stride;          /* 0: the same weights for every pixel; else (nd - 1) * npar */
  const double* inv_sigma_dyn; /* [npix or 1][nd - 1][npar], >= 0; may be NULL where nd == 1 */
} crt_lm_chain;

/*
 * k_lm_normal, one launch: for every column the sums k_lm_step forms over the rows of its nblk observation blocks (obs: HOST array,
 * copied by value), in that kernel's order and rounding (the SUMMATION CONTRACT of crt1d_hip_retrieve.h), WITHOUT the prior rows, written
 * as one crt_lm_normal_block: A [ncol][npar (npar + 1) / 2], g [ncol][npar], c2 [ncol] (the sum of r^2, without the factor 1/2).  Fed into
 * crt_hip_lm_step_normal_f64 with the same problem, every state array gets crt_hip_lm_step_f64's bits.
 * CRT_ERR_BAD_ARG: ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; NULL obs; nblk outside 1..CRT_LM_MAX_BLOCKS; a block with nrow < 1 or
 * NULL f, J or y; NULL A, g or c2.
 */
int crt_hip_lm_normal_f64(int32_t ncol, int32_t npar, const crt_lm_obs* obs, int32_t nblk, double* A, double* g, double* c2,
                          crt_stream_t stream);

/*
 * k_lm_step_chain, one launch: THE STEP above for every pixel.  blocks: HOST array of nblk blocks of per-column sums, copied by value.
 * state: p, p_trial, A, g per column; cost, lam, status, naccept, nreject per pixel.
 * CRT_ERR_BAD_ARG: everything crt_hip_lm_step_normal_f64 rejects; NULL chain; npix < 1; nd < 1; prob->ncol != npix * nd; dyn_stride
 * neither 0 nor (nd - 1) * npar; nd > 1 with NULL inv_sigma_dyn.
 * CRT_ERR_UNSUPPORTED: nd > crt_hip_lm_chain_max_nd(npar).
 */
int crt_hip_lm_step_chain_f64(const crt_lm_chain* chain, const crt_lm_problem* prob, const crt_lm_normal_block* blocks, int32_t nblk,
                              const crt_lm_state* state, crt_stream_t stream);

/*
 * k_lm_chain_covariance, one launch: cov [npix * nd][npar][npar], the diagonal blocks of the inverse of the undamped H of every pixel --
 * the smoothed marginal covariance of every date -- from the stored A [npix * nd][npar (npar + 1) / 2] and the weights: the block factors
 * of the step with lam = 0, then the backward recursion  S_d = W_d^T W_d + C_d^T S_{d+1} C_d,  W_d = L_d^-1,  C_d = B_{d+1} W_d
 * (S_{nd-1} = W^T W), unscaled by s.  A dead entry gets variance +inf and zero covariances.  The status of a pixel is not looked at.
 * CRT_ERR_BAD_ARG: NULL chain, npix or nd < 1, a bad stride, nd > 1 with NULL weights; npar outside 1..CRT_RETRIEVE_MAX_NPAR; NULL A or cov.
 * CRT_ERR_UNSUPPORTED: nd > crt_hip_lm_chain_max_nd(npar).
 */
int crt_hip_lm_chain_covariance_f64(const crt_lm_chain* chain, int32_t npar, const double* A, double* cov, crt_stream_t stream);

/* The largest nd the LDS LIMIT serves at this npar; 0 for npar outside 1..CRT_RETRIEVE_MAX_NPAR.  No device is touched. */
int32_t crt_hip_lm_chain_max_nd(int32_t npar);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LM_CHAIN_H */
