/*
 * crt1d_hip_lut.h -- the look-up-table start of a retrieval on the device: the weighted misfit of the observation vectors of ncol
 * columns against the K rows of a table of model evaluations, fused with the selection of the M best candidates of every column
 * (k_lut_match, then the tiny k_lut_merge).  Neither the ncol x K costs nor the ncol x K x nrow residuals are ever written.  The table
 * itself is made by the forward entries of the other headers: this header knows nothing of radiative transfer.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol sets of
 * the other headers and CRT_ABI_VERSION stay what they are.  The entry is asynchronous on `stream`, allocates nothing, never synchronises,
 * uses no atomics, finds every argument error before any launch and is capturable into a hipGraph.
 *
 * THE TEMPLATE ASSUMPTION.  One table is one template canopy evaluated at K parameter vectors q[k]; every column matched against it
 * shares that template and differs in its observations (and its prior).  Several classes of columns: several tables, several calls.
 *
 * COST CONTRACT (that of crt1d_hip_retrieve.h, so that cost[c][k] is bit for bit the cost_t of k_lm_step at p_trial = q[k] when the
 * table rows are bit for bit the forward sums there).  For column c and candidate k there is ONE running sum.  It starts at +0 and is
 * extended in this order: the rows of block 0 in ascending order, then those of block 1, ..., then the prior rows in ascending j.
 *   an observation row o of block b:  r = (m_b[k][o] - y_b[c][o]) * inv_sigma_b[c][o]   (rounded; inv_sigma_b NULL: r = m - y)
 *                                     sum = sum + r * r                                 (the product and the sum rounded separately)
 *     A row with inv_sigma == 0 adds nothing: its y may be NaN.
 *   a prior row j:                    d = (q[k][j] - prior[c][j]) * inv_sigma_prior[c][j];  sum = sum + d * d;
 *     skipped where inv_sigma_prior == 0.
 *   cost = 0.5 * sum.
 * The table is finite: a candidate with a NaN or an infinity in one of its m_b[k][.] (with a prior: or in q[k][.]) is eligible for no
 * column, whether the row it stands in is observed or not.
 * The order is a function of (nrow_0.., npar) only -- never of ncol, K, the column index or how the kernel tiles K.
 *
 * SELECTION CONTRACT.  A candidate is eligible iff cost < +inf (NaN and +inf are not).  index[c][0 .. M-1] are the M smallest eligible
 * candidates under the total order (cost, then index): ties go to the lower index.  cost[c][i] holds their costs.  Unfilled slots (fewer
 * than M eligible candidates, K < M included) get index -1 and cost +inf.  p[c] = q[index[c][0]]; a column without an eligible candidate
 * keeps the bits of its p[c]: the caller's default stays there.  Being defined by a total order, the result does not depend on how K is
 * split over waves, workgroups or passes, nor on `ksplit`.
 *
 * MAPPING.  Lane = column, candidates wave-uniform.  A workgroup of four waves owns 64 columns and takes 64 candidates at a time, 16 per
 * wave, each lane with 16 running sums in registers; the rows stream past in ascending order, CRT_LUT_ROWS at a time: the columns'
 * (y, inv_sigma) and the 64 table rows are staged in LDS by coalesced loads (a masked row as y = 0, inv_sigma = 0, whose square is +0 for a finite
 * table entry: the inner loop is the four fp64 instructions of the contract without a branch), and the table entries are
 * read back as LDS broadcasts.  Every lane keeps its M best sorted in registers, visits its candidates in ascending order and inserts on
 * strict <; the four lists are merged through LDS under the total order.  K is split over `ksplit` workgroups per 64 columns when there are
 * few columns; k_lut_merge merges the partial lists in the workspace and writes index, cost and p.
 */
#ifndef CRT1D_HIP_LUT_H
#define CRT1D_HIP_LUT_H

#include "crt1d_hip.h"
#include "crt1d_hip_retrieve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_LUT_MAX_BEST 8
#define CRT_LUT_MAX_KSPLIT 256
#define CRT_LUT_ROWS 16

typedef struct crt_lut_table { /* K model evaluations on one template; device pointers */
  int32_t ncand;           /* K >= 1 */
  int32_t npar;            /* 1 .. CRT_RETRIEVE_MAX_NPAR */
  int32_t nblk;            /* 1 .. CRT_LM_MAX_BLOCKS */
  int32_t nrow[CRT_LM_MAX_BLOCKS]; /* each >= 1 for b < nblk */
  const double* q;         /* [K][npar] the parameter vectors */
  const double* m[CRT_LM_MAX_BLOCKS]; /* m[b]: [K][nrow_b] the model's values of block b */
} crt_lut_table;

typedef struct crt_lut_obs { /* the observations of ncol columns; device pointers */
  int32_t ncol;            /* >= 1 */
  const double* y[CRT_LM_MAX_BLOCKS];         /* y[b]: [ncol][nrow_b] */
  const double* inv_sigma[CRT_LM_MAX_BLOCKS]; /* [ncol][nrow_b] or NULL (= ones); 0 = the row is not observed */
  const double* prior;           /* each [ncol][npar]; both or neither */
  const double* inv_sigma_prior;
} crt_lut_obs;

typedef struct crt_lut_out {
  int32_t nbest;           /* M, 1 .. CRT_LUT_MAX_BEST */
  int32_t ksplit;          /* 0: automatic; else the workgroups K is split over per 64 columns, clamped to what the automatic choice is
                              (the workspace is sized for that).  Changes no bit of the result. */
  int32_t* index;          /* [ncol][M] */
  double* cost;            /* [ncol][M] */
  double* p;               /* [ncol][npar] or NULL */
} crt_lut_out;

/* The workspace of a call: the partial lists of the K-split.  0 for sizes the entry refuses. */
size_t crt_hip_lut_match_workspace_bytes(int32_t ncol, int32_t ncand, int32_t nbest);

/*
 * k_lut_match and k_lut_merge, two launches.
 * CRT_ERR_BAD_ARG: NULL table, obs or out; ncand or ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; nblk outside 1..CRT_LM_MAX_BLOCKS; a
 * block b < nblk with nrow < 1 or NULL m or y; NULL q; one of prior / inv_sigma_prior NULL and the other not; nbest outside
 * 1..CRT_LUT_MAX_BEST; ksplit < 0; NULL index or cost.  CRT_ERR_WORKSPACE: NULL workspace, or workspace_bytes below
 * crt_hip_lut_match_workspace_bytes(ncol, ncand, nbest).  Nothing is refused on size: every offset is formed in 64 bits and the
 * groups of 64 columns lie on two grid dimensions, so any int32 ncol, K and nrow launch.
 */
int crt_hip_lut_match_f64(const crt_lut_table* table, const crt_lut_obs* obs, const crt_lut_out* out, void* workspace,
                          size_t workspace_bytes, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LUT_H */
