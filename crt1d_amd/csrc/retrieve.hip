// The per-column Levenberg-Marquardt retrieval (include/crt1d_hip_retrieve.h): the three kernels and their C entries.
//
//  k_retrieve_apply  the parameter vector of every column applied to the working spectra, LAI profile and g_param
//  k_lm_step         one wave per column: the normal equations at the trial point in the fixed order of the header, accept / reject,
//                    the damped scaled Cholesky solve and the next trial point
//  k_lm_covariance   one wave per column: the inverse of the stored normal matrix by the same scaled Cholesky
//
// No kernel here reads or writes outside [ncol] x its own row lengths: every index is bounded by a loop over the sizes the entry checked.
#include "crt1d_hip_masked.h"
#include "crt1d_hip_retrieve.h"
#include "crt_internal.hpp"
#include "lm_common.hpp"

namespace crt {
namespace {

constexpr int MAXA = MAXP + 1;                         // a row of (w_o0 .. w_o,npar-1, r_o)
constexpr int MAXENT = MAXA * (MAXA + 1) / 2;          // 66 entries of (A | g | 2 cost)
constexpr int LM_WAVE = 64;                            // one wave per column; also the rows staged at a time
constexpr int APPLY_BLOCK = 256;

struct ApplyArgs {
  int nz, nb, npar, ntan, i_lai, i_leaf;
  long long base_stride, dir_stride;
  const double* base[3];
  const double* dir[3];
  double* out[3];
  const double *lai0, *p;
  double *lai_scale, *lai, *g_param;
};

__global__ __launch_bounds__(APPLY_BLOCK) void k_retrieve_apply(ApplyArgs a) {
  const long long c = blockIdx.x;
  const int i = blockIdx.y * APPLY_BLOCK + threadIdx.x;
  const double* const pc = a.p + c * a.npar;
  if (i < a.nb) {
    for (int q = 0; q < 3; ++q) {
      if (!a.out[q]) continue;
      double x = a.base[q][c * a.base_stride + i];
      if (a.dir[q]) {
        const double* const d = a.dir[q] + c * a.dir_stride + i;
        for (int k = 0; k < a.ntan; ++k) x = x + pc[k] * d[(long long)k * a.nb];
      }
      a.out[q][c * a.nb + i] = x;
    }
  }
  if (a.i_lai >= 0) {
    const double sc = exp(pc[a.i_lai]);
    if (i == 0) a.lai_scale[c] = sc;
    if (i < a.nz) a.lai[c * a.nz + i] = a.lai0[c * a.nz + i] * sc;
  }
  if (a.i_leaf >= 0 && i == 0) a.g_param[c] = pc[a.i_leaf];
}

struct LmBlock {
  const double *f, *J, *y, *is;
  int nrow;
};

struct LmArgs {
  LmBlock blk[CRT_LM_MAX_BLOCKS];
  int nblk, npar;
  double lam_up, lam_down, lam_min, lam_max, xtol, ftol;
  const double *lo, *hi, *prior, *isp;
  crt_lm_state st;
};

// What THE STEP, item 1, is made of -- shared by k_lm_step and k_lm_decide (include_mask/crt1d_hip_masked.h), so that the cost the two form
// is one computation: the weight of a row, its weighted residual (a skipped row: +0) and one extension of a running sum by one product.
// Every operation is a separately rounded fp64 one (-ffp-contract=off).  The weighted residual of a prior row, one subtraction and one
// product, is written out in both kernels: behind a function of its own it moved k_lm_step's device code, which is held to what it was.
__device__ __forceinline__ double lm_row_weight(const LmBlock& B, long long o) { return B.is ? B.is[o] : 1.0; }
__device__ __forceinline__ double lm_row_residual(const LmBlock& B, long long o, double s) { return s != 0.0 ? (B.f[o] - B.y[o]) * s : 0.0; }
__device__ __forceinline__ double lm_extend(double acc, double x, double y) { return acc + x * y; }

__global__ __launch_bounds__(LM_WAVE) void k_lm_step(LmArgs a) {
  __shared__ double v[LM_WAVE * MAXA];  // the staged rows (w_o0 .. w_o,npar-1, r_o)
  __shared__ double sflag[LM_WAVE];     // inv_sigma of the staged rows; 0 = skipped (staged as a row of +0)
  __shared__ double ent[MAXENT + 2];    // (A | g | 2 cost)
  __shared__ double M[MAXP * MAXP];
  __shared__ double sc[MAXP], dl[MAXP];
  __shared__ bool dead[MAXP];
  const long long c = blockIdx.x;
  const int lane = threadIdx.x;
  const crt_lm_state& S = a.st;
  if (S.status[c] != CRT_LM_RUNNING) return;  // (the whole wave, before any barrier)
  const int npar = a.npar, na = npar + 1, ntri = npar * (npar + 1) / 2, nent = na * (na + 1) / 2;
  const int e0 = lane, e1 = lane + LM_WAVE;
  const bool has0 = e0 < nent, has1 = e1 < nent;
  int i0 = 0, j0 = 0, i1 = 0, j1 = 0;
  if (has0) tri_pair(e0, i0, j0);
  if (has1) tri_pair(e1, i1, j1);
  double acc0 = 0.0, acc1 = 0.0;
  for (int q = 0; q < a.nblk; ++q) {
    const LmBlock& B = a.blk[q];
    const long long row0 = c * B.nrow;
    for (int base = 0; base < B.nrow; base += LM_WAVE) {
      const int n = min(LM_WAVE, B.nrow - base);
      __syncthreads();  // the previous rows are consumed
      double s = 0.0;
      if (lane < n) {
        const long long o = row0 + base + lane;
        s = lm_row_weight(B, o);
        v[lane * na + npar] = lm_row_residual(B, o, s);
      }
      sflag[lane] = s;
      __syncthreads();
      const double* const Jc = B.J + (row0 + base) * npar;
      for (int idx = lane; idx < n * npar; idx += LM_WAVE) {
        const int row = idx / npar, k = idx - row * npar;
        const double sr = sflag[row];
        v[row * na + k] = sr != 0.0 ? Jc[idx] * sr : 0.0;
      }
      __syncthreads();
      // A skipped row is staged as +0: its products are +0, and a running sum that started at +0 is never -0, so adding them changes
      // no bit -- the loop has no branch on the row and its LDS reads run ahead of the adds.
#pragma unroll 4
      for (int o = 0; o < n; ++o) {
        const double* const r = v + o * na;
        acc0 = lm_extend(acc0, r[i0], r[j0]);
        acc1 = lm_extend(acc1, r[i1], r[j1]);
      }
    }
  }
  if (a.isp) {
    for (int k = 0; k < npar; ++k) {
      const double s = a.isp[c * npar + k];
      if (s == 0.0) continue;
      const double d = (S.p_trial[c * npar + k] - a.prior[c * npar + k]) * s;
      if (has0) {
        if (i0 == k && j0 == k) acc0 = acc0 + s * s;
        else if (i0 == npar && j0 == k) acc0 = acc0 + s * d;
        else if (i0 == npar && j0 == npar) acc0 = lm_extend(acc0, d, d);
      }
      if (has1) {
        if (i1 == k && j1 == k) acc1 = acc1 + s * s;
        else if (i1 == npar && j1 == k) acc1 = acc1 + s * d;
        else if (i1 == npar && j1 == npar) acc1 = lm_extend(acc1, d, d);
      }
    }
  }
  __syncthreads();
  if (has0) ent[e0] = acc0;
  if (has1) ent[e1] = acc1;
  __syncthreads();

  // ---- accept / reject: every lane takes the same decisions from the same values ----
  const double cost_t = 0.5 * ent[nent - 1];
  const double cost = S.cost[c];
  double lam = S.lam[c];
  int status = CRT_LM_RUNNING;
  const bool accept = cost_t < cost;
  double new_cost = cost;
  if (accept) {
    if (lane < npar) S.p[c * npar + lane] = S.p_trial[c * npar + lane];
    if (has0 && e0 < ntri) S.A[c * ntri + e0] = acc0;
    if (has0 && e0 >= ntri && e0 < ntri + npar) S.g[c * npar + e0 - ntri] = acc0;
    if (has1 && e1 < ntri + npar) S.g[c * npar + e1 - ntri] = acc1;  // (e1 >= 64 > ntri)
    lam = fmax(lam * a.lam_down, a.lam_min);
    if (cost - cost_t < a.ftol * cost_t) status = CRT_LM_CONVERGED_F;
    new_cost = cost_t;
  } else if (cost == INFINITY) {
    status = CRT_LM_FAILED_START;
  } else {
    lam = lam * a.lam_up;
    if (lam > a.lam_max) status = CRT_LM_STALLED;
    __syncthreads();
    if (has0 && e0 < ntri) ent[e0] = S.A[c * ntri + e0];
    if (has0 && e0 >= ntri && e0 < ntri + npar) ent[e0] = S.g[c * npar + e0 - ntri];
    if (has1 && e1 < ntri + npar) ent[e1] = S.g[c * npar + e1 - ntri];
    __syncthreads();
  }

  // ---- the next trial point ----
  bool conv_x = false;
  double pk = 0.0, pt = 0.0;
  if (status == CRT_LM_RUNNING) {
    if (lane == 0) {
      scaled_cholesky(ent, npar, lam, M, sc, dead);
      for (int k = 0; k < npar; ++k) dl[k] = -ent[ntri + k] * sc[k];
      cholesky_solve(M, npar, dl);
      for (int k = 0; k < npar; ++k) dl[k] = dl[k] * sc[k];
    }
    __syncthreads();
    bool far = false;
    if (lane < npar) {
      pk = S.p[c * npar + lane];  // (written by this lane where the step was accepted)
      pt = pk + dl[lane];
      if (a.lo && pt < a.lo[lane]) pt = a.lo[lane];
      if (a.hi && pt > a.hi[lane]) pt = a.hi[lane];
      far = !(fabs(pt - pk) < a.xtol * (fabs(pk) + a.xtol));
    }
    conv_x = !__any(far);
    if (conv_x) status = CRT_LM_CONVERGED_X;
  } else if (lane < npar) {
    pk = S.p[c * npar + lane];
  }
  if (lane < npar) S.p_trial[c * npar + lane] = status == CRT_LM_RUNNING ? pt : pk;
  if (lane == 0) {
    S.cost[c] = new_cost;
    S.lam[c] = lam;
    S.status[c] = status;
    if (accept) S.naccept[c] += 1;
    else if (status != CRT_LM_FAILED_START) S.nreject[c] += 1;
  }
}

// crt_hip_lm_decide_f64 (include_mask/crt1d_hip_masked.h): the cost entry of k_lm_step alone -- the running sum of r_o * r_o over the rows
// of block 0, 1, ... in ascending order, then d_k * d_k over the prior rows, extended by the functions k_lm_step extends it with -- and
// the decision k_lm_step will take from it.  One wave per column; every lane forms the same sum from the residuals staged in LDS, lane 0
// stores.  J is never read, no state is written; a column that is not running is skipped and its cost_t keeps its bits.
__global__ __launch_bounds__(LM_WAVE) void k_lm_decide(LmArgs a, int32_t* __restrict__ skip_jac, double* __restrict__ cost_t) {
  __shared__ double rr[LM_WAVE];  // the weighted residuals of the staged rows (a skipped row: +0)
  const long long c = blockIdx.x;
  const int lane = threadIdx.x, npar = a.npar;
  if (a.st.status[c] != CRT_LM_RUNNING) {  // (the whole wave, before any barrier)
    if (lane == 0) skip_jac[c] = 1;
    return;
  }
  double acc = 0.0;
  for (int q = 0; q < a.nblk; ++q) {
    const LmBlock& B = a.blk[q];
    const long long row0 = c * B.nrow;
    for (int base = 0; base < B.nrow; base += LM_WAVE) {
      const int n = min(LM_WAVE, B.nrow - base);
      __syncthreads();  // the previous rows are consumed
      if (lane < n) {
        const long long o = row0 + base + lane;
        rr[lane] = lm_row_residual(B, o, lm_row_weight(B, o));
      }
      __syncthreads();
      for (int o = 0; o < n; ++o) acc = lm_extend(acc, rr[o], rr[o]);
    }
  }
  if (a.isp) {
    for (int k = 0; k < npar; ++k) {
      const double s = a.isp[c * npar + k];
      if (s == 0.0) continue;
      const double d = (a.st.p_trial[c * npar + k] - a.prior[c * npar + k]) * s;  // (k_lm_step's line: see above)
      acc = lm_extend(acc, d, d);
    }
  }
  if (lane == 0) {
    const double ct = 0.5 * acc;
    cost_t[c] = ct;
    skip_jac[c] = ct < a.st.cost[c] ? 0 : 1;  // (NaN: skip)
  }
}

__global__ __launch_bounds__(LM_WAVE) void k_lm_covariance(int npar, const double* __restrict__ A, double* __restrict__ cov) {
  __shared__ double ent[MAXP * (MAXP + 1) / 2];
  __shared__ double M[MAXP * MAXP];
  __shared__ double X[MAXP * MAXP];
  __shared__ double sc[MAXP];
  __shared__ bool dead[MAXP];
  const long long c = blockIdx.x;
  const int lane = threadIdx.x, ntri = npar * (npar + 1) / 2;
  if (lane < ntri) ent[lane] = A[c * ntri + lane];
  __syncthreads();
  if (lane == 0) scaled_cholesky(ent, npar, 0.0, M, sc, dead);
  __syncthreads();
  if (lane < npar) {
    double* const x = X + lane * MAXP;  // column `lane` of the inverse of the scaled matrix
    for (int k = 0; k < npar; ++k) x[k] = k == lane ? 1.0 : 0.0;
    cholesky_solve(M, npar, x);
    for (int k = 0; k < npar; ++k) {
      double z = (x[k] * sc[k]) * sc[lane];
      if (dead[k] || dead[lane]) z = k == lane ? INFINITY : 0.0;
      cov[(c * npar + lane) * npar + k] = z;
    }
  }
}

bool dirs_ok(const crt_optics_dirs* d, int nb) {
  if (!d) return true;
  if (d->ntan < 0 || d->ntan > CRT_SENSJAC_MAX_NTAN) return false;
  if (d->ntan == 0) return true;
  if (!d->leaf_r && !d->leaf_t && !d->soil_r) return false;
  return d->col_stride == 0 || d->col_stride == (int64_t)d->ntan * nb;
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int crt_hip_retrieve_apply_f64(const crt_retrieve_apply* ap, const crt_optics_dirs* dirs, crt_stream_t stream) {
  if (!ap || ap->ncol < 1 || ap->nz < 1 || ap->nb < 1 || ap->npar < 1 || ap->npar > CRT_RETRIEVE_MAX_NPAR) return CRT_ERR_BAD_ARG;
  if (!dirs_ok(dirs, ap->nb)) return CRT_ERR_BAD_ARG;
  const int ntan = dirs ? dirs->ntan : 0;
  const int has_lai = ap->i_lai >= 0, has_leaf = ap->i_leaf >= 0;
  if (ap->i_lai != -1 && ap->i_lai != ntan) return CRT_ERR_BAD_ARG;
  if (ap->i_leaf != -1 && ap->i_leaf != ntan + has_lai) return CRT_ERR_BAD_ARG;
  if (ap->npar != ntan + has_lai + has_leaf) return CRT_ERR_BAD_ARG;
  if (ap->base_stride != 0 && ap->base_stride != ap->nb) return CRT_ERR_BAD_ARG;
  if (!ap->leaf_r0 || !ap->leaf_t0 || !ap->p || !ap->leaf_r || !ap->leaf_t || !ap->soil_r0 != !ap->soil_r) return CRT_ERR_BAD_ARG;
  if (has_lai && (!ap->lai0 || !ap->lai || !ap->lai_scale)) return CRT_ERR_BAD_ARG;
  if (has_leaf && !ap->g_param) return CRT_ERR_BAD_ARG;
  ApplyArgs a;
  a.nz = ap->nz, a.nb = ap->nb, a.npar = ap->npar, a.ntan = ntan, a.i_lai = has_lai ? ap->i_lai : -1, a.i_leaf = has_leaf ? ap->i_leaf : -1;
  a.base_stride = ap->base_stride;
  a.dir_stride = ntan ? dirs->col_stride : 0;
  a.base[0] = ap->leaf_r0, a.base[1] = ap->leaf_t0, a.base[2] = ap->soil_r0;
  a.dir[0] = ntan ? dirs->leaf_r : nullptr, a.dir[1] = ntan ? dirs->leaf_t : nullptr, a.dir[2] = ntan ? dirs->soil_r : nullptr;
  a.out[0] = ap->leaf_r, a.out[1] = ap->leaf_t, a.out[2] = ap->soil_r;
  a.lai0 = ap->lai0, a.p = ap->p, a.lai_scale = ap->lai_scale, a.lai = ap->lai, a.g_param = ap->g_param;
  const int span = ap->nb > ap->nz ? ap->nb : ap->nz;
  const long long ny = ((long long)span + APPLY_BLOCK - 1) / APPLY_BLOCK;
  if (ny > 65535) return CRT_ERR_UNSUPPORTED;
  const int st = launch_kernel(k_retrieve_apply, dim3(ap->ncol, (unsigned)ny), APPLY_BLOCK, 0, static_cast<hipStream_t>(stream), a);
  if (st == CRT_OK) note_kernel("k_retrieve_apply ntan=%d lai=%d leaf=%d", ntan, has_lai, has_leaf);
  return st;
}

// the argument checks of crt_hip_lm_step_f64 and the kernel's argument block (crt_hip_lm_decide_f64 shares both)
static int lm_step_args(const crt_lm_problem* prob, const crt_lm_obs* obs, int32_t nblk, const crt_lm_state* state, LmArgs& a) {
  if (!obs || !lm_problem_ok(prob, nblk, state)) return CRT_ERR_BAD_ARG;
  a = {};
  for (int q = 0; q < nblk; ++q) {
    if (obs[q].nrow < 1 || !obs[q].f || !obs[q].J || !obs[q].y) return CRT_ERR_BAD_ARG;
    a.blk[q] = LmBlock{obs[q].f, obs[q].J, obs[q].y, obs[q].inv_sigma, obs[q].nrow};
  }
  a.nblk = nblk, a.npar = prob->npar;
  a.lam_up = prob->lam_up, a.lam_down = prob->lam_down, a.lam_min = prob->lam_min, a.lam_max = prob->lam_max;
  a.xtol = prob->xtol, a.ftol = prob->ftol;
  a.lo = prob->lo, a.hi = prob->hi, a.prior = prob->prior, a.isp = prob->inv_sigma_prior;
  a.st = *state;
  return CRT_OK;
}

int crt_hip_lm_step_f64(const crt_lm_problem* prob, const crt_lm_obs* obs, int32_t nblk, const crt_lm_state* state, crt_stream_t stream) {
  LmArgs a;
  if (const int st = lm_step_args(prob, obs, nblk, state, a)) return st;
  const int st = launch_kernel(k_lm_step, dim3(prob->ncol), LM_WAVE, 0, static_cast<hipStream_t>(stream), a);
  if (st == CRT_OK) note_kernel("k_lm_step npar=%d nblk=%d", prob->npar, nblk);
  return st;
}

int crt_hip_lm_decide_f64(const crt_lm_problem* prob, const crt_lm_obs* obs, int32_t nblk, const crt_lm_state* state, int32_t* skip_jac,
                          double* cost_t, crt_stream_t stream) {
  LmArgs a;
  if (const int st = lm_step_args(prob, obs, nblk, state, a)) return st;
  if (!skip_jac || !cost_t) return CRT_ERR_BAD_ARG;
  const int st = launch_kernel(k_lm_decide, dim3(prob->ncol), LM_WAVE, 0, static_cast<hipStream_t>(stream), a, skip_jac, cost_t);
  if (st == CRT_OK) note_kernel("k_lm_decide npar=%d nblk=%d", prob->npar, nblk);
  return st;
}

int crt_hip_lm_covariance_f64(int32_t ncol, int32_t npar, const double* A, double* cov, crt_stream_t stream) {
  if (ncol < 1 || npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || !A || !cov) return CRT_ERR_BAD_ARG;
  const int st = launch_kernel(k_lm_covariance, dim3(ncol), LM_WAVE, 0, static_cast<hipStream_t>(stream), (int)npar, A, cov);
  if (st == CRT_OK) note_kernel("k_lm_covariance npar=%d", npar);
  return st;
}

}  // extern "C"
