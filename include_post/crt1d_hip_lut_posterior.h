/*
 * crt1d_hip_lut_posterior.h -- the Bayesian look-up-table estimate on the device: for every column the mean and the covariance of the K
 * candidates of a table weighted by exp(-cost / T), with the effective sample size, without ever writing the ncol x K costs.  Where the
 * Levenberg-Marquardt covariance describes one basin of the misfit surface, this one describes the whole box the table samples.
 *
 * An extension of crt1d_hip_lut.h: same library, same structs (crt_lut_table, crt_lut_obs, unchanged), same conventions; a header of its
 * own so that the symbol sets of the other headers and CRT_ABI_VERSION stay what they are.  The entry is asynchronous on `stream`,
 * allocates nothing, never synchronises, uses no atomics, finds every argument error before any launch and is capturable into a hipGraph
 * after the first call.
 *
 * For column c, with cost[c][k] bit for bit the cost of the COST CONTRACT of crt1d_hip_lut.h:
 *
 * BEST CANDIDATE.  kb and cmin = cost[c][kb] are the best candidate under the SELECTION CONTRACT of crt1d_hip_lut.h: the total order
 * (cost, index), eligible iff cost < +inf.  They are what crt_hip_lut_match_f64 gives with nbest = 1.
 *
 * NO RESULT.  A column without an eligible candidate gets index = -1, cost = +inf, wsum = 0, ess = 0; its mean and cov keep their bits.
 *
 * TEMPERATURE.  T is the scalar `temperature` (finite and > 0, else CRT_ERR_BAD_ARG), overridden per column by temperature_col[c] where
 * that array is given.  A column whose temperature_col value is not finite or not > 0 is a column without an eligible candidate.
 *
 * WEIGHT.  it = 1.0 / T (IEEE division, once per column); a_k = (cost_k - cmin) * it, the difference and the product rounded separately;
 * w_k = fexp(-a_k), the library's exponential (<= 1 ulp; it underflows to exactly 0).  An ineligible candidate has w_k = 0 by selection,
 * not by multiplication: its q may be non-finite when a prior is present, and it enters no sum.
 *
 * CENTRED MOMENTS, centred on the best candidate so that nothing large cancels:
 *   d_i = q[k][i] - q[kb][i];  t_i = w_k * d_i;
 *   S0 += w_k;  Sq += w_k * w_k;  S1_i += t_i;  S2_ij += t_i * d_j for i >= j.
 * Every product and every sum is rounded separately.
 *
 * SUMMATION ORDER.  K is divided into parts exactly as k_lut_match divides it: groups of 64 candidates, the groups
 * [p * ngroups / ksplit, (p + 1) * ngroups / ksplit) in part p.  Inside a part candidate k belongs to strand (k mod 64) / 16.  There is
 * ONE running sum per (part, strand, entry), from +0, extended in ascending k.  The four strands of a part are added in the order 0, 1,
 * 2, 3; then the parts are added in ascending order.  The order is a function of (K, the effective ksplit, npar) only -- never of ncol,
 * the column index or another column's data.
 *
 * KSPLIT.  ksplit = 0 chooses as the match does (enough workgroups for the device when there are few columns: a function of ncol and K);
 * an explicit value is honoured, clamped to the number of groups of 64 candidates and to CRT_LUT_MAX_KSPLIT.  The workspace query takes
 * ksplit, so a fixed value holds the bits of a column across batch sizes.  Across DIFFERENT ksplit the sums are formed in different
 * orders and the results agree within rounding only (index and cost are bitwise the same) -- unlike the match, whose result is
 * ksplit-free.
 *
 * FINISH.  One lane per column, IEEE division and multiplication, each operation rounded once, in this order:
 *   m_i = S1_i / S0;  mean_i = q[kb][i] + m_i;  cov_ij = S2_ij / S0 - m_i * m_j (the lower triangle computed and mirrored);
 *   ess = (S0 * S0) / Sq;  wsum = S0.
 * (S0 >= 1: the best candidate's weight is exactly 1.)
 *
 * BIT-NEUTRAL SKIPPING.  A weight that underflows to exactly 0 adds +0 everywhere and changes no bit, so k_lut_moments skips the moment
 * arithmetic of a candidate whose weight is 0 in all 64 lanes of the wave.
 *
 * MAPPING.  Three passes.  (1) crt_hip_lut_match_f64 with nbest = 1 writes index and cost.  (2) k_lut_moments, on the skeleton of
 * k_lut_match: lane = column, a workgroup of four waves owns 64 columns and one part, the rows stream through LDS CRT_LUT_ROWS at a
 * time, each wave forms the costs of its 16 candidates of a group of 64 -- the same four fp64 instructions per row, hence the same bits
 * -- and extends its strand's sums, which live in registers; at the end of the part the strands are added through LDS and written to
 * the workspace.  (3) k_lut_moments_finish adds the parts and does the finish arithmetic.
 */
#ifndef CRT1D_HIP_LUT_POSTERIOR_H
#define CRT1D_HIP_LUT_POSTERIOR_H

#include "crt1d_hip_lut.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crt_lut_posterior_out {
  double temperature;            /* finite, > 0 */
  const double* temperature_col; /* [ncol] or NULL */
  int32_t ksplit;                /* 0: automatic */
  int32_t* index;                /* [ncol]   best candidate, -1 without one */
  double* cost;                  /* [ncol]   its cost, +inf without one */
  double* mean;                  /* [ncol][npar] */
  double* cov;                   /* [ncol][npar][npar] */
  double* wsum;                  /* [ncol] */
  double* ess;                   /* [ncol] */
} crt_lut_posterior_out;

/* The workspace of a call: that of the match and the partial sums of the parts.  0 for sizes the entry refuses (ncol or ncand < 1, npar
 * outside 1..CRT_RETRIEVE_MAX_NPAR, ksplit < 0).  Monotone in ksplit. */
size_t crt_hip_lut_posterior_workspace_bytes(int32_t ncol, int32_t ncand, int32_t npar, int32_t ksplit);

/*
 * crt_hip_lut_match_f64 (nbest = 1), k_lut_moments, k_lut_moments_finish: four launches.
 * CRT_ERR_BAD_ARG: NULL table, obs or out; ncand or ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; nblk outside 1..CRT_LM_MAX_BLOCKS; a
 * block b < nblk with nrow < 1 or NULL m or y; NULL q; one of prior / inv_sigma_prior NULL and the other not; temperature not finite or
 * not > 0; ksplit < 0; NULL index, cost, mean, cov, wsum or ess.  CRT_ERR_WORKSPACE: NULL workspace, or workspace_bytes below
 * crt_hip_lut_posterior_workspace_bytes(ncol, ncand, npar, ksplit).  As in the match, nothing is refused on size.
 */
int crt_hip_lut_posterior_f64(const crt_lut_table* table, const crt_lut_obs* obs, const crt_lut_posterior_out* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LUT_POSTERIOR_H */
