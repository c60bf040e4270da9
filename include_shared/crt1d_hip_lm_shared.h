/*
 * crt1d_hip_lm_shared.h -- the chained Levenberg-Marquardt step of crt1d_hip_lm_chain.h with parameters that all nd dates of a pixel
 * share: one unknown instead of nd copies tied by a stiff random walk.  The normal matrix of a pixel is the chain's block-tridiagonal
 * matrix (at the nv varying parameters per date) bordered by ns dense rows, an arrowhead.  Two launching entries: the step of a whole
 * pixel (k_lm_step_shared) and the marginal covariances of (v_d, s) for every date (k_lm_shared_covariance).  The sums come from
 * crt_hip_lm_normal_f64 or the spectral normal entries, as for the chain; k_retrieve_apply reads p_trial unchanged.
 *
 * An extension of crt1d_hip.h: same library, same conventions, separate header so that the symbol sets of the other headers and
 * CRT_ABI_VERSION stay what they are.  The launching entries are asynchronous on `stream`, allocate nothing, never synchronise, use no
 * atomics, find every argument error before any launch and are capturable into a hipGraph.
 *
 * SHARED SET.  crt_lm_shared.mask: bit k set means parameter k (0 <= k < npar) is shared.  ns = popcount(mask), 0 <= ns <= npar,
 * nv = npar - ns.  k_0 < k_1 < .. are the shared indices ("s_i" is parameter k_i), kv_0 < kv_1 < .. the varying ones.
 *
 * UNKNOWNS of a pixel, in this order: v_0 .. v_{nd-1}, the nv varying parameters of each date with k ascending; then s, the ns shared
 * ones with k ascending.  n = nd * nv + ns.  Row index r = d * nv + j for the varying parameter kv_j of date d, r = nd * nv + i for s_i.
 *
 * STATE.  As in the chain: p, p_trial, A, g are [ncol] (ncol = npix * nd, c = pix * nd + d), A and g at the full npar of every date;
 * cost, lam, status, naccept, nreject are [npix].  The value of a shared parameter is READ from date 0 of the pixel (p[pix * nd][k]).
 * It is WRITTEN with the same bits to all nd dates of p_trial, and on acceptance p[d][k] = p_trial[0][k] for every date d.  The kernel
 * does not check that the caller's copies agree (the caller evaluated date d at p_trial[d]).
 *
 * COST.  The chain's cost with the coupling terms over varying k only:
 *     cost = 0.5 * (sum_d c2_d + sum_{d < nd-1} sum_{k varying} e_{d,k}^2),   e_{d,k} = (p_{d+1,k} - p_{d,k}) * w_{d,k},
 * c2_d, A_d, g_d per date exactly as the chain forms them (block 0's bits, the blocks 1.. ascending, then that date's prior rows in
 * ascending k, shared k included: a prior on a shared parameter given on several dates counts several times).  The pixel sum starts from
 * c2_0's bits, adds c2_1, c2_2, ..., then the coupling terms with d ascending, then k ascending, shared k skipped; e, e * e and every sum
 * are separately rounded.  inv_sigma_dyn keeps its layout [npix or 1][nd - 1][npar]; the entries of shared k are not read.
 *
 * NORMAL MATRIX AND GRADIENT.
 *     varying part: the chain's H and G restricted to the varying indices (the same formulas, the same roundings);
 *     border:       H_(s_i),(d,j)  = A_d[k_i, kv_j]                 the stored bits
 *     corner:       H_(s_i),(s_l)  = sum_d A_d[k_i, k_l]
 *     gradient:     G_(s_i)        = sum_d g_d[k_i]
 * each of the two sums starts from date 0's bits and adds the dates 1, 2, .. in ascending order.
 *
 * THE STEP is the chain's per pixel, word for word: accept iff cost_t < cost; CRT_LM_FAILED_START; the lam updates; ftol; CRT_LM_STALLED;
 * a pixel that stops gets p_trial = p on every date (a plain copy); a pixel not running on entry is not touched.  CRT_LM_CONVERGED_X
 * looks at all n entries (a shared entry at p of date 0).  p_trial_r = clamp(p_r + delta_r, lo_k, hi_k).
 *
 * THE SOLVE runs on the n x n system: s_r = 1 / sqrt(H_rr), a dead entry (H_rr <= 0) has s_r = 1;
 * M_rq = (H_rq * s_r) * s_q + (dead ? 1 : lam) [r == q] for q <= r (so a border entry is (A * s_(s_i)) * s_(d,j)); x_r = (-G_r) * s_r.
 * The factorisation is the dense left-looking Cholesky of scaled_cholesky in the ordering above, L_rq = (M_rq - t_rq) / L_qq,
 * L_qq = sqrt(M_qq - t_qq), where every t_rq is ONE running sum from +0 of L_rm * L_qm over ascending m < q with the structurally zero
 * terms left out.  L_rm is structurally non-zero
 *     for a varying row r of date d:  m in the block of date d - 1 (date 0: none) or in the own block, m <= r;
 *     for a border row:               every m <= r.
 * So for a border row r = s_i:
 *     q = (d, j):  m runs over the nv columns of date d - 1 (none for d = 0), then the columns (d, 0) .. (d, j - 1);
 *     q = s_l:     m runs over all nd * nv varying columns, d ascending then j ascending, then the corner columns s_0 .. s_{l-1}.
 * Forward: z_r = (x_r - u_r) / L_rr, u_r one running sum from +0 of L_rm * z_m over ascending m < r, non-zeros as above (a border row:
 * all nd * nv varying columns, then the corner columns before it).
 * Backward: y_r = (z_r - v_r) / L_rr, v_r one running sum from +0 of L_mr * y_m over the rows m > r that are structurally non-zero in
 * column r, the farthest group first: for a varying r = (d, j) the border rows s_0 .. s_{ns-1}, then the rows of date d + 1's block
 * ascending, then the rows m > j of the own block ascending (the chain's order, which takes the next date before the own block; with
 * ns = 0 nothing else is possible if the chain's bits are to be kept); for a border row the corner rows m > r ascending.
 * delta_r = y_r * s_r.
 *
 * IDENTITIES.  With ns == 0 every state array and the covariance have the bits of crt_hip_lm_step_chain_f64 /
 * crt_hip_lm_chain_covariance_f64.  With ns == npar, one block and no prior, p_trial of every date, cost, lam and status have the bits
 * crt_hip_lm_step_normal_f64 leaves on ONE column fed the nd dates' sums as nd blocks.
 *
 * SUMMATION CONTRACT.  No atomics.  One wave owns one pixel.  Every order is a function of (nd, npar, mask, nblk) only: a pixel's state is
 * bitwise the same alone or in any batch.
 *
 * LDS LIMIT.  The chain's carve-up at nv, the border factor Y [nd][ns][nv], three ns x ns corner arrays, two nv x ns work arrays and four
 * vectors of ns live in dynamic LDS.  A date without a varying parameter still keeps its c2, one double:
 *     CRT_LM_SHARED_LDS_BYTES(nd, nv, ns) = 8 * (nd * (nv ? 2 nv^2 + 4 nv + nv ns : 1) + 4 nv^2 + 64 + 3 ns^2 + 2 nv ns + 4 ns)
 *                                        <=   CRT_LM_CHAIN_LDS_LIMIT = 160 KiB,
 * and crt_hip_lm_shared_max_nd(npar, ns) is that inverted, rounded down: 212 at npar = 10, ns = 5; with ns = 0 the chain's limit.
 */
#ifndef CRT1D_HIP_LM_SHARED_H
#define CRT1D_HIP_LM_SHARED_H

#include "crt1d_hip_lm_chain.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_LM_SHARED_LDS_BYTES(nd, nv, ns)                                                                                \
  (8 * ((long long)(nd) * ((nv) ? 2 * (nv) * (nv) + 4 * (nv) + (nv) * (ns) : 1) + 4 * (nv) * (nv) + 64 + 3 * (ns) * (ns) + \
        2 * (nv) * (ns) + 4 * (ns)))

typedef struct crt_lm_shared {
  uint32_t mask; /* bit k set: parameter k is shared by all dates of a pixel; no bit at or above npar */
} crt_lm_shared;

/*
 * k_lm_step_shared, one launch: THE STEP above for every pixel.  Arguments as crt_hip_lm_step_chain_f64, plus the shared set.
 * CRT_ERR_BAD_ARG: everything crt_hip_lm_step_chain_f64 rejects; NULL shared; a mask bit at or above npar.
 * CRT_ERR_UNSUPPORTED: nd > crt_hip_lm_shared_max_nd(npar, ns).
 */
int crt_hip_lm_step_shared_f64(const crt_lm_chain* chain, const crt_lm_shared* shared, const crt_lm_problem* prob,
                               const crt_lm_normal_block* blocks, int32_t nblk, const crt_lm_state* state, crt_stream_t stream);

/*
 * k_lm_shared_covariance, one launch: cov [npix * nd][npar][npar] in the ORIGINAL parameter order: for date d the marginal covariance of
 * (v_d, s) from the inverse of the undamped H (the factors of the step with lam = 0): the chain's recursion for (T^-1)_dd plus
 * Z_d S^-1 Z_d^T, the cross block -Z_d S^-1 and S^-1, with T the varying part, Z = T^-1 B^T, B the border and S the Schur complement of
 * the corner; unscaled by s.  The shared-shared block has the same bits on every date.  A dead entry gets variance +inf and zero
 * covariances.  The status of a pixel is not looked at.
 * CRT_ERR_BAD_ARG: what crt_hip_lm_chain_covariance_f64 rejects; NULL shared; a mask bit at or above npar.
 * CRT_ERR_UNSUPPORTED: nd > crt_hip_lm_shared_max_nd(npar, ns).
 */
int crt_hip_lm_shared_covariance_f64(const crt_lm_chain* chain, const crt_lm_shared* shared, int32_t npar, const double* A, double* cov,
                                     crt_stream_t stream);

/* The largest nd the LDS LIMIT serves; 0 for npar outside 1..CRT_RETRIEVE_MAX_NPAR or ns outside 0..npar.  No device is touched. */
int32_t crt_hip_lm_shared_max_nd(int32_t npar, int32_t ns);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LM_SHARED_H */
