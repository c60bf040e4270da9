// What the Levenberg-Marquardt units (retrieve.hip, specfit.hip, lm_chain.hip) share: the packed-triangle indexing, a block of supplied
// sums (A | g | c2), the scaled Cholesky of one column by one lane, and on the host the argument checks of a problem with its state and of
// a chain.  Everything is internal to a unit (the unnamed namespace): a kernel that uses a function has it inlined, with the roundings of
// the text here (-ffp-contract=off).
#pragma once
#include "crt1d_hip_lm_chain.h"
#include "crt_internal.hpp"

namespace crt {
namespace {

constexpr int MAXP = CRT_RETRIEVE_MAX_NPAR;  // 10

__device__ inline int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i
__device__ inline int symtri(int a, int b) { return a >= b ? tri(a, b) : tri(b, a); }

// entry e of a lower triangle stored row by row -> (i, j), j <= i
__device__ inline void tri_pair(int e, int& i, int& j) {
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

// the sums of one block of observations, supplied instead of rows: A [ncol][ntri], g [ncol][npar], c2 [ncol]
struct SumBlock {
  const double *A, *g, *c2;
};

// entry e of (A | g | c2) of column c in a block
__device__ __forceinline__ double block_entry(const SumBlock& B, long long c, int e, int ntri, int npar) {
  return e < ntri ? B.A[c * ntri + e] : e < ntri + npar ? B.g[c * npar + e - ntri] : B.c2[c];
}

// By ONE lane, on LDS: sc[k] = 1 / sqrt(A_kk) (dead: 1); M = (A_ij sc_i) sc_j + (dead ? 1 : lam) [i == j], lower triangle, replaced by its
// Cholesky factor (left-looking, as batched.gauss_newton_step).  ent: the packed lower triangle of A.
__device__ inline void scaled_cholesky(const double* ent, int n, double lam, double* M, double* sc, bool* dead) {
  for (int k = 0; k < n; ++k) {
    const double d = ent[tri(k, k)];
    dead[k] = d <= 0.0;
    sc[k] = dead[k] ? 1.0 : 1.0 / sqrt(d);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double m = (ent[tri(i, j)] * sc[i]) * sc[j];
      if (i == j) m = m + (dead[i] ? 1.0 : lam);
      M[i * MAXP + j] = m;
    }
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = 0; k < j; ++k) s = s + M[j * MAXP + k] * M[j * MAXP + k];
    const double d = sqrt(M[j * MAXP + j] - s);
    M[j * MAXP + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double t = 0.0;
      for (int k = 0; k < j; ++k) t = t + M[i * MAXP + k] * M[j * MAXP + k];
      M[i * MAXP + j] = (M[i * MAXP + j] - t) / d;
    }
  }
}

// L L^T x = x in place (x: LDS, n entries)
__device__ inline void cholesky_solve(const double* M, int n, double* x) {
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = 0; k < j; ++k) s = s + M[j * MAXP + k] * x[k];
    x[j] = (x[j] - s) / M[j * MAXP + j];
  }
  for (int j = n - 1; j >= 0; --j) {
    double s = 0.0;
    for (int k = j + 1; k < n; ++k) s = s + M[k * MAXP + j] * x[k];
    x[j] = (x[j] - s) / M[j * MAXP + j];
  }
}

// ---- host: the argument checks the step entries share (every failure is CRT_ERR_BAD_ARG) ----

inline bool lm_problem_ok(const crt_lm_problem* prob, int32_t nblk, const crt_lm_state* state) {
  if (!prob || !state) return false;
  if (prob->ncol < 1 || prob->npar < 1 || prob->npar > CRT_RETRIEVE_MAX_NPAR || nblk < 1 || nblk > CRT_LM_MAX_BLOCKS) return false;
  if (!(prob->lam_up > 1.0) || !(prob->lam_down > 0.0 && prob->lam_down <= 1.0)) return false;
  if (!(prob->lam_min >= 0.0) || !(prob->lam_max >= prob->lam_min) || !(prob->xtol >= 0.0) || !(prob->ftol >= 0.0)) return false;
  if (!prob->prior != !prob->inv_sigma_prior) return false;
  return state->p && state->p_trial && state->cost && state->lam && state->A && state->g && state->status && state->naccept &&
         state->nreject;
}

inline bool chain_ok(const crt_lm_chain* ch, int npar) {
  if (!ch || ch->npix < 1 || ch->nd < 1) return false;
  if (ch->dyn_stride != 0 && ch->dyn_stride != (int64_t)(ch->nd - 1) * npar) return false;
  return ch->nd == 1 || ch->inv_sigma_dyn;
}

}  // namespace
}  // namespace crt
