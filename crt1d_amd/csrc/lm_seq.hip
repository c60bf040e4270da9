// The date-by-date form of the time-series retrieval (include_seq/crt1d_hip_lm_seq.h): the three kernels and their C entries.
//
//  k_lm_prior_block  one wave per column: the sums (A | g | c2) of a Gaussian prior with a full precision matrix at the trial point
//  k_lm_predict      one wave per column: the posterior precision of a date through one random-walk gap, (A^-1 + W^-1)^-1 = W (A + W)^-1 A
//  k_lm_rts          one wave per pixel: the backward Rauch-Tung-Striebel sweep, date by date, with one date's matrices in LDS
//
// All three follow k_lm_covariance (retrieve.hip): the small matrices live in static LDS, ONE lane factorises (scaled_cholesky of
// lm_common.hpp, lam = 0), the npar right-hand sides of a solve go one per lane, the npar^2 entries of a product one per lane (two trips
// at npar > 8).  No per-lane arrays, no scratch, no dynamic LDS: nothing on chip depends on nd.
//
// Bounds: a column index c < ncol (c < npix * nd in k_lm_rts) times a row length plus an index below that row length, in 64 bits; every
// LDS index is i * MAXP + j with i, j < npar <= MAXP or a packed index < ntri <= 55.
#include "crt1d_hip_lm_seq.h"
#include "crt_internal.hpp"
#include "lm_common.hpp"

namespace crt {
namespace {

constexpr int WAVE = 64;
constexpr int MAXTRI = MAXP * (MAXP + 1) / 2;

// every pivot of the factor scaled_cholesky left in M is a finite number > 0 (a NaN anywhere in a row reaches that row's pivot)
__device__ inline bool pivots_ok(const double* M, int n) {
  bool ok = true;
  for (int j = 0; j < n; ++j) {
    const double d = M[j * MAXP + j];
    ok = ok && d > 0.0 && d < INFINITY;
  }
  return ok;
}

// k_lm_covariance's body on LDS, restated (sharing it through a header would have to leave that kernel's device code identical): column
// `lane` of the inverse of the matrix whose scaled factor is M; X: the work array, out: [npar][npar], out[lane][k]
__device__ inline void inverse_column(const double* M, const double* sc, const bool* dead, int npar, int lane, double* X, double* out) {
  double* const x = X + lane * MAXP;
  for (int k = 0; k < npar; ++k) x[k] = k == lane ? 1.0 : 0.0;
  cholesky_solve(M, npar, x);
  for (int k = 0; k < npar; ++k) {
    double z = (x[k] * sc[k]) * sc[lane];
    if (dead[k] || dead[lane]) z = k == lane ? INFINITY : 0.0;
    out[lane * npar + k] = z;
  }
}

__global__ __launch_bounds__(WAVE) void k_lm_prior_block(int npar, long long prec_stride, const double* __restrict__ prec,
                                                         const double* __restrict__ mean, const double* __restrict__ p_trial,
                                                         double* __restrict__ A, double* __restrict__ g, double* __restrict__ c2) {
  __shared__ double P[MAXTRI];
  __shared__ double d[MAXP];
  __shared__ double v[MAXP];
  const long long c = blockIdx.x;
  const int lane = threadIdx.x, ntri = npar * (npar + 1) / 2;
  if (lane < ntri) {
    const double e = prec[c * prec_stride + lane];
    P[lane] = e;
    A[c * ntri + lane] = e;
  }
  if (lane < npar) d[lane] = p_trial[c * npar + lane] - mean[c * npar + lane];
  __syncthreads();
  if (lane < npar) {
    double s = 0.0;
    for (int j = 0; j < npar; ++j) s = s + P[symtri(lane, j)] * d[j];
    v[lane] = s;
    g[c * npar + lane] = s;
  }
  __syncthreads();
  if (lane == 0) {
    double s = 0.0;
    for (int i = 0; i < npar; ++i) s = s + d[i] * v[i];
    c2[c] = s;
  }
}

__global__ __launch_bounds__(WAVE) void k_lm_predict(int npar, long long dyn_stride, const double* __restrict__ A,
                                                     const double* __restrict__ wdyn, double* __restrict__ prec, int* __restrict__ info) {
  __shared__ double ent[MAXTRI];  // A, then E = A + W
  __shared__ double a0[MAXTRI];   // A
  __shared__ double M[MAXP * MAXP];
  __shared__ double Y[MAXP * MAXP];  // Y[j * MAXP + k] = Y_kj: column j by lane j
  __shared__ double sc[MAXP];
  __shared__ double q[MAXP];
  __shared__ bool dead[MAXP];
  __shared__ int okflag;
  const long long c = blockIdx.x;
  const int lane = threadIdx.x, ntri = npar * (npar + 1) / 2;
  if (lane < ntri) {
    const double e = A[c * ntri + lane];
    a0[lane] = e, ent[lane] = e;
  }
  __syncthreads();
  if (lane < npar) {
    const double w = wdyn[c * dyn_stride + lane];
    const double qq = w * w;
    q[lane] = qq;
    ent[tri(lane, lane)] = a0[tri(lane, lane)] + qq;
  }
  __syncthreads();
  if (lane == 0) {
    scaled_cholesky(ent, npar, 0.0, M, sc, dead);
    okflag = pivots_ok(M, npar) ? 1 : 0;
  }
  __syncthreads();
  const bool ok = okflag != 0;  // (uniform)
  if (ok && lane < npar) {
    double* const x = Y + lane * MAXP;
    for (int k = 0; k < npar; ++k) x[k] = a0[symtri(k, lane)] * sc[k];
    cholesky_solve(M, npar, x);
    for (int k = 0; k < npar; ++k) x[k] = x[k] * sc[k];
  }
  __syncthreads();
  if (lane < ntri) {
    int i, j;
    tri_pair(lane, i, j);
    double z = 0.0;
    if (ok && q[i] != 0.0 && q[j] != 0.0 && !dead[i] && !dead[j]) z = 0.5 * (q[i] * Y[j * MAXP + i] + q[j] * Y[i * MAXP + j]);
    prec[c * ntri + lane] = z;
  }
  if (lane == 0) info[c] = ok ? 0 : 1;
}

__global__ __launch_bounds__(WAVE) void k_lm_rts(int nd, int npar, long long dyn_stride, const double* __restrict__ wdyn,
                                                 const double* __restrict__ p_f, const double* __restrict__ A_f, double* __restrict__ p_s,
                                                 double* __restrict__ cov_s, int* __restrict__ info) {
  __shared__ double ent[MAXTRI];
  __shared__ double M[MAXP * MAXP];
  __shared__ double X[MAXP * MAXP];
  __shared__ double Mi[MAXP * MAXP];  // [npar][npar]: Mi[j * npar + k] = (M^-1)_kj, column j by lane j
  __shared__ double G[MAXP * MAXP];   // [npar][npar] row-major: G[i * npar + j]
  __shared__ double C[MAXP * MAXP];   // [npar][npar]: cov_s of the date after
  __shared__ double T[MAXP * MAXP];
  __shared__ double sc[MAXP];
  __shared__ double q[MAXP];
  __shared__ double dp[MAXP];
  __shared__ double pf[MAXP];
  __shared__ bool dead[MAXP];
  __shared__ int okflag;
  const long long pix = blockIdx.x, c0 = pix * nd;
  const int lane = threadIdx.x, ntri = npar * (npar + 1) / 2, npp = npar * npar;
  const double* const wp = wdyn ? wdyn + pix * dyn_stride : nullptr;  // (read only where nd > 1; the entry refused NULL there)

  // ---- the last date: k_lm_covariance on A_f, p_s = p_f ----
  {
    const long long c = c0 + nd - 1;
    if (lane < ntri) ent[lane] = A_f[c * ntri + lane];
    double pl = 0.0;
    if (lane < npar) pl = p_f[c * npar + lane];
    __syncthreads();
    if (lane == 0) scaled_cholesky(ent, npar, 0.0, M, sc, dead);
    __syncthreads();
    if (lane < npar) {
      inverse_column(M, sc, dead, npar, lane, X, C);
      p_s[c * npar + lane] = pl;
      pf[lane] = pl;  // p_s of the date after, for the first step back
    }
    __syncthreads();
    for (int e = lane; e < npp; e += WAVE) cov_s[c * npp + e] = C[e];
  }
  bool cbad = false;
  for (int e = lane; e < npp; e += WAVE) cbad = cbad || !(fabs(C[e]) < INFINITY);
  cbad = __any(cbad);

  // ---- backward; the loads of date t are issued one date ahead of their use ----
  double a_n = 0.0, p_n = 0.0, w_n = 0.0;
  if (nd > 1) {
    const long long c = c0 + nd - 2;
    if (lane < ntri) a_n = A_f[c * ntri + lane];
    if (lane < npar) p_n = p_f[c * npar + lane], w_n = wp[(long long)(nd - 2) * npar + lane];
  }
  int failed = 0;
  for (int t = nd - 2; t >= 0; --t) {
    const long long c = c0 + t;
    __syncthreads();  // the date after is consumed (pf held its p_s)
    if (lane < ntri) ent[lane] = a_n;
    double pt = p_n;
    if (lane < npar) {
      dp[lane] = pf[lane] - p_n;  // p_s,t+1 - p_f,t
      q[lane] = w_n * w_n;
    }
    if (t > 0) {
      if (lane < ntri) a_n = A_f[(c - 1) * ntri + lane];
      if (lane < npar) p_n = p_f[(c - 1) * npar + lane], w_n = wp[(long long)(t - 1) * npar + lane];
    }
    __syncthreads();
    if (lane < npar) ent[tri(lane, lane)] = ent[tri(lane, lane)] + q[lane];
    __syncthreads();
    if (lane == 0) {
      scaled_cholesky(ent, npar, 0.0, M, sc, dead);
      bool ok = pivots_ok(M, npar);
      for (int k = 0; k < npar; ++k) ok = ok && !dead[k];
      okflag = ok ? 1 : 0;
    }
    __syncthreads();
    if (cbad || okflag == 0) {  // (uniform)
      failed = 1 + t;
      break;
    }
    if (lane < npar) {
      inverse_column(M, sc, dead, npar, lane, X, Mi);
      for (int k = 0; k < npar; ++k) G[k * npar + lane] = Mi[lane * npar + k] * q[lane];
    }
    __syncthreads();
    if (lane < npar) {
      double s = 0.0;
      for (int j = 0; j < npar; ++j) s = s + G[lane * npar + j] * dp[j];
      const double ps = pt + s;
      p_s[c * npar + lane] = ps;
      pf[lane] = ps;  // (dp was formed from the old value before the barriers above)
    }
    for (int e = lane; e < npp; e += WAVE) {
      const int i = e / npar, k = e - i * npar;
      double s = 0.0;
      for (int j = 0; j < npar; ++j) s = s + G[i * npar + j] * C[j * npar + k];
      T[e] = s;
    }
    __syncthreads();
    double z0 = 0.0, z1 = 0.0;  // the entries lane and lane + 64 of the new C (read the old one above, written after the barrier)
    for (int e = lane, r = 0; e < npp; e += WAVE, ++r) {
      const int i = e / npar, k = e - i * npar;
      const int hi = i >= k ? i : k, lo = i >= k ? k : i;
      double s = 0.0;
      for (int j = 0; j < npar; ++j) s = s + T[hi * npar + j] * G[lo * npar + j];
      const double z = Mi[lo * npar + hi] + s;
      if (r == 0) z0 = z;
      else z1 = z;
    }
    __syncthreads();
    bool bad = false;
    for (int e = lane, r = 0; e < npp; e += WAVE, ++r) {
      const double z = r == 0 ? z0 : z1;
      C[e] = z;
      cov_s[c * npp + e] = z;
      bad = bad || !(fabs(z) < INFINITY);
    }
    cbad = __any(bad);
  }
  if (failed) {
    const double nan = __builtin_nan("");
    const long long np = (long long)failed * npar, nc = (long long)failed * npp;
    for (long long e = lane; e < np; e += WAVE) p_s[c0 * npar + e] = nan;
    for (long long e = lane; e < nc; e += WAVE) cov_s[c0 * npp + e] = nan;
  }
  if (lane == 0) info[pix] = failed;
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int crt_hip_lm_prior_block_f64(const crt_lm_prior_full* pr, const double* p_trial, double* A, double* g, double* c2, crt_stream_t stream) {
  if (!pr || pr->ncol < 1 || pr->npar < 1 || pr->npar > CRT_RETRIEVE_MAX_NPAR || !pr->precision || !pr->mean) return CRT_ERR_BAD_ARG;
  const int ntri = pr->npar * (pr->npar + 1) / 2;
  if ((pr->prec_stride != 0 && pr->prec_stride != ntri) || !p_trial || !A || !g || !c2) return CRT_ERR_BAD_ARG;
  const int st = launch_kernel(k_lm_prior_block, dim3(pr->ncol), WAVE, 0, static_cast<hipStream_t>(stream), (int)pr->npar,
                               (long long)pr->prec_stride, pr->precision, pr->mean, p_trial, A, g, c2);
  if (st == CRT_OK) note_kernel("k_lm_prior_block npar=%d", pr->npar);
  return st;
}

int crt_hip_lm_predict_f64(int32_t ncol, int32_t npar, const double* A, const double* inv_sigma_dyn, int64_t dyn_stride, double* precision,
                           int32_t* info, crt_stream_t stream) {
  if (ncol < 1 || npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || !A || !inv_sigma_dyn || !precision || !info) return CRT_ERR_BAD_ARG;
  if (dyn_stride != 0 && dyn_stride != npar) return CRT_ERR_BAD_ARG;
  const int st = launch_kernel(k_lm_predict, dim3(ncol), WAVE, 0, static_cast<hipStream_t>(stream), (int)npar, (long long)dyn_stride, A,
                               inv_sigma_dyn, precision, info);
  if (st == CRT_OK) note_kernel("k_lm_predict npar=%d", npar);
  return st;
}

int crt_hip_lm_rts_f64(const crt_lm_chain* chain, int32_t npar, const double* p_f, const double* A_f, double* p_s, double* cov_s,
                       int32_t* info, crt_stream_t stream) {
  if (npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || !chain_ok(chain, npar) || !p_f || !A_f || !p_s || !cov_s || !info) return CRT_ERR_BAD_ARG;
  const int st = launch_kernel(k_lm_rts, dim3(chain->npix), WAVE, 0, static_cast<hipStream_t>(stream), (int)chain->nd, (int)npar,
                               (long long)chain->dyn_stride, chain->nd > 1 ? chain->inv_sigma_dyn : nullptr, p_f, A_f, p_s, cov_s, info);
  if (st == CRT_OK) note_kernel("k_lm_rts nd=%d npar=%d", chain->nd, npar);
  return st;
}

}  // extern "C"
