/*
 * crt1d_hip_retrieve.h -- a per-column Levenberg-Marquardt retrieval on the device: what consumes the sensor-band sums of
 * crt1d_hip_sensor.h and their Jacobian of crt1d_hip_sensjac.h.  Three entries: the parameter vector of every column applied to the
 * solver inputs (k_retrieve_apply), one Levenberg-Marquardt step of every column (k_lm_step) and the posterior covariance
 * (k_lm_covariance).  The radiative transfer itself is not in here: between the apply and the step the caller runs
 * crt_hip_sensor_jac_f64 and crt_hip_sensor_levels_f64 (or their series forms) on the arrays the apply wrote.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.  All three entries are asynchronous on `stream`, allocate nothing, never
 * synchronise, find every argument error before any launch and are capturable into a hipGraph.
 *
 * PARAMETER AXIS.  npar = ntan + (i_lai >= 0) + (i_leaf >= 0), 1 .. CRT_RETRIEVE_MAX_NPAR, in the order of crt_hip_sensor_jac_f64: the
 * coefficients of the ntan directions of a crt_optics_dirs, then the log of a scale of the column's LAI profile, then the column's
 * g_param itself.
 *
 * THE STEP.  The caller evaluates the forward sums f and the Jacobian J at the TRIAL point p_trial; the step decides whether the trial
 * point becomes the accepted point p, keeps the normal equations of the accepted point, and forms the next trial point from them.  For
 * a column with status == CRT_LM_RUNNING (o runs over the rows of all observation blocks):
 *
 *  1. r_o = (f_o - y_o) * inv_sigma_o;  cost_t = 0.5 * (sum_o r_o^2 + sum_k ((p_trial_k - prior_k) * inv_sigma_prior_k)^2).  A row with
 *     inv_sigma == 0 is skipped altogether (its f, y and J may be NaN); so is a prior row with inv_sigma_prior == 0.
 *  2. Accepted iff cost_t < cost (false for NaN).  cost starts at +inf: the first call is accepted unless cost_t is not finite, which
 *     gives status = CRT_LM_FAILED_START (no counter moves).
 *     accepted: p = p_trial;  A_ij = sum_o (J_oi * inv_sigma_o) * (J_oj * inv_sigma_o),  g_i = sum_o (J_oi * inv_sigma_o) * r_o, the
 *       prior rows (J = inv_sigma_prior_k e_k) last;  lam = max(lam * lam_down, lam_min);  status = CRT_LM_CONVERGED_F if
 *       cost - cost_t < ftol * cost_t (strict: ftol = 0 disables it);  cost = cost_t;  ++naccept.
 *     rejected: p, cost, A and g keep their bits;  lam = lam * lam_up;  status = CRT_LM_STALLED once lam > lam_max;  ++nreject.
 *  3. Still running: (A + lam * diag(A)) delta = -g, solved as batched.gauss_newton_step does it: with s_k = 1 / sqrt(A_kk), the matrix
 *     (A_ij * s_i) * s_j + lam [i == j] is factorised by a Cholesky without pivoting and delta_k = x_k * s_k; a dead parameter (A_kk <= 0)
 *     has s_k = 1 and a unit diagonal, hence delta_k = 0.  p_trial_k = clamp(p_k + delta_k, lo_k, hi_k) (NaN stays NaN), and
 *     status = CRT_LM_CONVERGED_X if |p_trial_k - p_k| < xtol * (|p_k| + xtol) for every k (strict: xtol = 0 disables it).
 *  4. A column that stops running in this call gets p_trial = p.  A column that is not running on entry is not touched: every state
 *     array keeps its bits.  The caller keeps evaluating it at its result.
 *
 * SUMMATION CONTRACT.  No atomics.  One wave owns one column; one lane owns one entry of (A | g | 2 cost) (npar = 10: 66 entries, lanes 0
 * and 1 own two).  Every entry is one running sum, started at +0 and extended by one product at a time in this order: the rows of block 0
 * in ascending order, then those of block 1, ..., then the prior rows in ascending k.  Skipped rows add nothing.  The order is a function
 * of (nrow_0.., npar) only -- never of ncol, the column index or the column's status.  Every product and every sum is a separately rounded
 * fp64 operation: w_oi = J_oi * inv_sigma_o and r_o are rounded first (inv_sigma NULL: w_oi = J_oi, r_o = f_o - y_o), then the products
 * w_oi * w_oj, w_oi * r_o and r_o * r_o; the prior row k adds inv_sigma_prior_k * inv_sigma_prior_k to A_kk,
 * inv_sigma_prior_k * d_k to g_k and d_k * d_k to 2 cost, d_k = (p_trial_k - prior_k) * inv_sigma_prior_k.  cost_t = 0.5 * that sum.
 */
#ifndef CRT1D_HIP_RETRIEVE_H
#define CRT1D_HIP_RETRIEVE_H

#include "crt1d_hip.h"
#include "crt1d_hip_sensjac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_RETRIEVE_MAX_NPAR (CRT_SENSJAC_MAX_NTAN + 2)
#define CRT_LM_MAX_BLOCKS 4

enum crt_lm_status {
  CRT_LM_RUNNING = 0,
  CRT_LM_CONVERGED_X = 1,  /* the step fell below xtol */
  CRT_LM_CONVERGED_F = 2,  /* an accepted step lowered the cost by less than ftol * cost */
  CRT_LM_STALLED = 3,      /* the damping passed lam_max */
  CRT_LM_FAILED_START = 4  /* the cost at the starting point is not finite */
};

typedef struct crt_retrieve_apply { /* parameters -> solver inputs */
  int32_t ncol, nz, nb, npar;
  int32_t i_lai;           /* index of ln(LAI scale) in p: ntan, or -1 for none */
  int32_t i_leaf;          /* index of g_param in p: ntan + (i_lai >= 0), or -1 for none */
  int64_t base_stride;     /* 0: the same base spectra for every column; else nb */
  const double* leaf_r0;   /* each [ncol or 1][nb] */
  const double* leaf_t0;
  const double* soil_r0;   /* NULL together with soil_r (bl) */
  const double* lai0;      /* [ncol][nz]; read where i_lai >= 0 */
  const double* p;         /* [ncol][npar] */
  double* leaf_r;          /* each [ncol][nb] */
  double* leaf_t;
  double* soil_r;
  double* lai_scale;       /* [ncol]; written where i_lai >= 0 */
  double* lai;             /* [ncol][nz]; written where i_lai >= 0 */
  double* g_param;         /* [ncol]; written where i_leaf >= 0 */
} crt_retrieve_apply;

typedef struct crt_lm_obs { /* one block of observations: one output key of a Jacobian plan, read where it lies */
  int32_t nrow;            /* >= 1 */
  const double* f;         /* [ncol][nrow] forward sums at p_trial */
  const double* J;         /* [ncol][nrow][npar] */
  const double* y;         /* [ncol][nrow] observations */
  const double* inv_sigma; /* [ncol][nrow] or NULL (= ones); 0 = the row is not observed */
} crt_lm_obs;

typedef struct crt_lm_problem {
  int32_t ncol, npar;
  double lam_up;                 /* > 1 */
  double lam_down;               /* in (0, 1] */
  double lam_min, lam_max;       /* 0 <= lam_min <= lam_max */
  double xtol, ftol;             /* >= 0 */
  const double* lo;              /* each [npar] or NULL (unbounded) */
  const double* hi;
  const double* prior;           /* each [ncol][npar]; both or neither */
  const double* inv_sigma_prior;
} crt_lm_problem;

typedef struct crt_lm_state { /* caller-owned, per column */
  double* p;         /* [ncol][npar] the accepted parameters */
  double* p_trial;   /* [ncol][npar] the trial point */
  double* cost;      /* [ncol] the accepted cost; starts at +inf */
  double* lam;       /* [ncol] the damping */
  double* A;         /* [ncol][npar (npar + 1) / 2] the lower triangle of the normal matrix at p, row by row */
  double* g;         /* [ncol][npar] its right-hand side J^T r */
  int32_t* status;   /* [ncol] enum crt_lm_status */
  int32_t* naccept;  /* [ncol] */
  int32_t* nreject;  /* [ncol] */
} crt_lm_state;

/*
 * k_retrieve_apply, one launch:
 *   leaf_r[c][b] = leaf_r0[c or 0][b] + p[c][0] * d.leaf_r[c or 0][0][b] + p[c][1] * d.leaf_r[c or 0][1][b] + ...   (ascending k, products
 *   and sums separately rounded; a NULL direction array is left out: a copy of the base), leaf_t and soil_r likewise;
 *   lai_scale[c] = exp(p[c][i_lai]);  lai[c][z] = lai0[c][z] * lai_scale[c];  g_param[c] = p[c][i_leaf].
 * Nothing is clamped or validated.  dirs: NULL stands for ntan = 0.
 * CRT_ERR_BAD_ARG: NULL ap; ncol, nz or nb < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; ntan outside 0..CRT_SENSJAC_MAX_NTAN, ntan > 0 with
 * all three direction pointers NULL, dirs->col_stride neither 0 nor ntan * nb; i_lai neither -1 nor ntan; i_leaf neither -1 nor
 * ntan + (i_lai >= 0); npar != ntan + (i_lai >= 0) + (i_leaf >= 0); base_stride neither 0 nor nb; NULL leaf_r0, leaf_t0, p, leaf_r or
 * leaf_t; one of soil_r0 / soil_r NULL and the other not; i_lai >= 0 with NULL lai0, lai or lai_scale; i_leaf >= 0 with NULL g_param.
 */
int crt_hip_retrieve_apply_f64(const crt_retrieve_apply* ap, const crt_optics_dirs* dirs, crt_stream_t stream);

/*
 * k_lm_step, one launch: THE STEP above for every column.  obs: HOST array of nblk blocks, copied by value.
 * CRT_ERR_BAD_ARG: NULL prob, obs or state; ncol < 1; npar outside 1..CRT_RETRIEVE_MAX_NPAR; nblk outside 1..CRT_LM_MAX_BLOCKS; a block with
 * nrow < 1 or NULL f, J or y; lam_up <= 1; lam_down outside (0, 1]; lam_min < 0 or lam_max < lam_min; xtol or ftol < 0 (NaN fails every
 * one of these); one of prior / inv_sigma_prior NULL and the other not; a NULL state array.
 */
int crt_hip_lm_step_f64(const crt_lm_problem* prob, const crt_lm_obs* obs, int32_t nblk, const crt_lm_state* state, crt_stream_t stream);

/*
 * k_lm_covariance, one launch: cov[c] = inverse of the stored, undamped A[c], [ncol][npar][npar], by the scaled Cholesky of the step.  A
 * dead parameter (A_kk <= 0) gets variance +inf and zero covariances.
 * CRT_ERR_BAD_ARG: ncol < 1, npar outside 1..CRT_RETRIEVE_MAX_NPAR, NULL A or cov.
 */
int crt_hip_lm_covariance_f64(int32_t ncol, int32_t npar, const double* A, double* cov, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_RETRIEVE_H */
