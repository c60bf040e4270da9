// The Levenberg-Marquardt step on a chain of coupled dates (include_chain/crt1d_hip_lm_chain.h): the three kernels and their C entries.
//
//  k_lm_normal            one wave per column: the sums of k_lm_step (retrieve.hip) over the observation rows, written instead of consumed
//  k_lm_step_chain        one wave per pixel: the per-date sums as k_lm_step_normal (specfit.hip) forms them, the pixel's cost with the
//                         random-walk terms, accept / reject, the block Cholesky of the damped, scaled block-tridiagonal normal matrix
//                         along the chain, the two substitutions and the next trial point of every date
//  k_lm_chain_covariance  one wave per pixel: the same block factors with lam = 0 and the backward recursion for the diagonal blocks
//                         of the inverse
//
// The work of a date's block is spread over the lanes (one row of the sub-diagonal solve, one entry of B B^T, one row below a pivot per
// lane); every entry still is one running sum in ascending column order, so the order of the header holds and a single date gives
// scaled_cholesky's bits.  All per-date storage is dynamic LDS sized by (nd, npar): no per-lane arrays, no scratch.
//
// Bounds: every global index is c * (row length) + (index < row length) with c < npix * nd, every LDS index lies inside the carve-up
// of chain_lds() whose size the entry checked against the limit.
#include "crt1d_hip_lm_chain.h"
#include "crt_internal.hpp"

namespace crt {
namespace {

constexpr int MAXP = CRT_RETRIEVE_MAX_NPAR;    // 10
constexpr int MAXA = MAXP + 1;                 // a row of (w_o0 .. w_o,npar-1, r_o)
constexpr int WAVE = 64;                       // one wave per column (k_lm_normal) or per pixel; also the rows staged at a time

__device__ inline int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// entry e of a lower triangle stored row by row -> (i, j), j <= i
__device__ inline void tri_pair(int e, int& i, int& j) {
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

// ------------------------------------------------------------------------------------------
// the sums from rows.  The row loop is k_lm_step's, restated: sharing it through a header would have to leave that kernel's device code
// identical, and its loop is interleaved with that kernel's own staging buffers and barriers.  Same staging, same order, same roundings.

struct RowBlock {
  const double *f, *J, *y, *is;
  int nrow;
};

struct NormalArgs {
  RowBlock blk[CRT_LM_MAX_BLOCKS];
  int nblk, npar;
  double *A, *g, *c2;
};

__global__ __launch_bounds__(WAVE) void k_lm_normal(NormalArgs a) {
  __shared__ double v[WAVE * MAXA];  // the staged rows (w_o0 .. w_o,npar-1, r_o)
  __shared__ double sflag[WAVE];     // inv_sigma of the staged rows; 0 = skipped (staged as a row of +0)
  const long long c = blockIdx.x;
  const int lane = threadIdx.x;
  const int npar = a.npar, na = npar + 1, ntri = npar * (npar + 1) / 2, nent = na * (na + 1) / 2;
  const int e0 = lane, e1 = lane + WAVE;
  const bool has0 = e0 < nent, has1 = e1 < nent;
  int i0 = 0, j0 = 0, i1 = 0, j1 = 0;
  if (has0) tri_pair(e0, i0, j0);
  if (has1) tri_pair(e1, i1, j1);
  double acc0 = 0.0, acc1 = 0.0;
  for (int q = 0; q < a.nblk; ++q) {
    const RowBlock& B = a.blk[q];
    const long long row0 = c * B.nrow;
    for (int base = 0; base < B.nrow; base += WAVE) {
      const int n = min(WAVE, B.nrow - base);
      __syncthreads();  // the previous rows are consumed
      double s = 0.0;
      if (lane < n) {
        const long long o = row0 + base + lane;
        s = B.is ? B.is[o] : 1.0;
        v[lane * na + npar] = s != 0.0 ? (B.f[o] - B.y[o]) * s : 0.0;
      }
      sflag[lane] = s;
      __syncthreads();
      const double* const Jc = B.J + (row0 + base) * npar;
      for (int idx = lane; idx < n * npar; idx += WAVE) {
        const int row = idx / npar, k = idx - row * npar;
        const double sr = sflag[row];
        v[row * na + k] = sr != 0.0 ? Jc[idx] * sr : 0.0;
      }
      __syncthreads();
      // (a skipped row is staged as +0 and adds products of +0 to sums that started at +0: no bit changes, as in k_lm_step)
#pragma unroll 4
      for (int o = 0; o < n; ++o) {
        const double* const r = v + o * na;
        acc0 = acc0 + r[i0] * r[j0];
        acc1 = acc1 + r[i1] * r[j1];
      }
    }
  }
  if (has0) {
    if (e0 < ntri) a.A[c * ntri + e0] = acc0;
    else if (e0 < ntri + npar) a.g[c * npar + e0 - ntri] = acc0;
    else a.c2[c] = acc0;
  }
  if (has1) {  // (e1 >= 64 > ntri)
    if (e1 < ntri + npar) a.g[c * npar + e1 - ntri] = acc1;
    else a.c2[c] = acc1;
  }
}

// ------------------------------------------------------------------------------------------
// the chain

struct SumBlock {
  const double *A, *g, *c2;
};

struct ChainArgs {
  SumBlock blk[CRT_LM_MAX_BLOCKS];
  int nblk, npar, nd;
  long long dyn_stride;
  const double* wdyn;
  double lam_up, lam_down, lam_min, lam_max, xtol, ftol;
  const double *lo, *hi, *prior, *isp;
  crt_lm_state st;
};

// the dynamic LDS of a pixel, in doubles: CRT_LM_CHAIN_LDS_BYTES / 8
struct ChainLds {
  double* L;   // [nd][npar][npar] the diagonal blocks of M, replaced by their factors (lower triangle)
  double* B;   // [nd][npar][npar] the sub-diagonal blocks (rows of date d, columns of date d - 1; block 0 unused)
  double* x;   // [nd][npar] the right-hand side, replaced by the solution; before that the c2 of the dates
  double* sc;  // [nd][npar] the scales
  double* w;   // [nd][npar] the weights of the gap behind date d (the last row +0)
  double* h;   // [nd][npar] the diagonal of H; after the solve the trial point
  double* T;   // [npar][npar] the running sums B B^T a diagonal block starts from
  double *W, *C, *S;  // each [npar][npar]: the covariance recursion
};

__device__ inline ChainLds chain_lds(double* sh, int nd, int npar) {
  const int np2 = npar * npar, nv = nd * npar;
  ChainLds m;
  m.L = sh, m.B = m.L + nd * np2, m.x = m.B + nd * np2, m.sc = m.x + nv, m.w = m.sc + nv, m.h = m.w + nv;
  m.T = m.h + nv, m.W = m.T + np2, m.C = m.W + np2, m.S = m.C + np2;
  return m;
}

__device__ __forceinline__ double block_entry(const SumBlock& B, long long c, int e, int ntri, int npar) {
  return e < ntri ? B.A[c * ntri + e] : e < ntri + npar ? B.g[c * npar + e - ntri] : B.c2[c];
}

// Entry e of (A | g | c2) of column c as k_lm_step_normal forms it: block 0's bits, the blocks 1.. in ascending order, then the prior rows
// in ascending k -- of which an entry of A or g sees at most one.
__device__ inline double date_entry(const ChainArgs& a, long long c, int e, int ntri, int npar) {
  double acc = block_entry(a.blk[0], c, e, ntri, npar);
  for (int q = 1; q < a.nblk; ++q) acc = acc + block_entry(a.blk[q], c, e, ntri, npar);
  if (!a.isp) return acc;
  const double* const isp = a.isp + c * npar;
  const double* const pr = a.prior + c * npar;
  const double* const pt = a.st.p_trial + c * npar;
  if (e < ntri) {
    int i, j;
    tri_pair(e, i, j);
    if (i == j && isp[i] != 0.0) acc = acc + isp[i] * isp[i];
  } else if (e < ntri + npar) {
    const int k = e - ntri;
    const double s = isp[k];
    if (s != 0.0) acc = acc + s * ((pt[k] - pr[k]) * s);
  } else {
    for (int k = 0; k < npar; ++k) {
      const double s = isp[k];
      if (s == 0.0) continue;
      const double d = (pt[k] - pr[k]) * s;
      acc = acc + d * d;
    }
  }
  return acc;
}

// h = diag H, the scales and the weights of every (date, parameter).  A: the packed triangles of the pixel's nd dates; wp: its weights.
__device__ inline void chain_scales(const ChainLds& m, const double* A, const double* wp, int nd, int npar, int lane) {
  const int ntri = npar * (npar + 1) / 2;
  for (int r = lane; r < nd * npar; r += WAVE) {
    const int d = r / npar, k = r - d * npar;
    double h = A[(long long)d * ntri + tri(k, k)];
    if (d > 0) {
      const double wl = wp[(d - 1) * npar + k];
      h = h + wl * wl;
    }
    double wr = 0.0;
    if (d < nd - 1) {
      wr = wp[d * npar + k];
      h = h + wr * wr;
    }
    m.h[r] = h, m.w[r] = wr;
    m.sc[r] = h <= 0.0 ? 1.0 : 1.0 / sqrt(h);
  }
}

// M = (H_rq s_r) s_q + (dead ? 1 : lam) [r == q]: the lower triangles of the diagonal blocks into L, the (diagonal) sub-diagonal blocks into B
__device__ inline void chain_matrix(const ChainLds& m, const double* A, int nd, int npar, double lam, int lane) {
  const int ntri = npar * (npar + 1) / 2, np2 = npar * npar;
  for (int idx = lane; idx < nd * np2; idx += WAVE) {
    const int d = idx / np2, e = idx - d * np2, i = e / npar, j = e - i * npar;
    double v = 0.0, b = 0.0;
    if (j <= i) {
      const double hij = i == j ? m.h[d * npar + i] : A[(long long)d * ntri + tri(i, j)];
      v = (hij * m.sc[d * npar + i]) * m.sc[d * npar + j];
      if (i == j) v = v + (hij <= 0.0 ? 1.0 : lam);
    }
    if (d > 0 && i == j) {
      const double wl = m.w[(d - 1) * npar + i];
      b = ((-(wl * wl)) * m.sc[d * npar + i]) * m.sc[(d - 1) * npar + i];
    }
    m.L[idx] = v, m.B[idx] = b;
  }
}

// The block Cholesky along the chain, in place.  Per date: B_d L_{d-1}^T = M_{d,d-1} by npar lanes, one row each; T = B_d B_d^T, one entry
// per lane; then the left-looking factorisation of the diagonal block, whose running sums start from T: the pivot by its own lane, the
// rows below it one per lane.  (Uniform trip counts: every lane reaches every barrier.)
__device__ inline void chain_factor(const ChainLds& m, int nd, int npar, int lane) {
  const int np2 = npar * npar;
  for (int d = 0; d < nd; ++d) {
    double* const L = m.L + d * np2;
    double* const B = m.B + d * np2;
    if (d > 0) {
      const double* const Lp = L - np2;
      if (lane < npar) {
        double* const row = B + lane * npar;
        for (int k = 0; k < npar; ++k) {
          double t = 0.0;
          for (int q = 0; q < k; ++q) t = t + row[q] * Lp[k * npar + q];
          row[k] = (row[k] - t) / Lp[k * npar + k];
        }
      }
      __syncthreads();
    }
    for (int e = lane; e < np2; e += WAVE) {
      const int i = e / npar, j = e - i * npar;
      double t = 0.0;
      if (d > 0 && j <= i)
        for (int k = 0; k < npar; ++k) t = t + B[i * npar + k] * B[j * npar + k];
      m.T[e] = t;
    }
    __syncthreads();
    for (int j = 0; j < npar; ++j) {
      if (lane == j) {
        double s = m.T[j * npar + j];
        for (int k = 0; k < j; ++k) s = s + L[j * npar + k] * L[j * npar + k];
        L[j * npar + j] = sqrt(L[j * npar + j] - s);
      }
      __syncthreads();
      if (lane > j && lane < npar) {
        double t = m.T[lane * npar + j];
        for (int k = 0; k < j; ++k) t = t + L[lane * npar + k] * L[j * npar + k];
        L[lane * npar + j] = (L[lane * npar + j] - t) / L[j * npar + j];
      }
      __syncthreads();
    }
  }
}

// L L^T x = x in place.  Forward: lane j keeps the running sum of row j (the previous date's columns, then the own columns as they become
// known).  Backward: the next date's rows first, one running sum per lane, then the own rows k > j in ascending order by the lane of j.
__device__ inline void chain_solve(const ChainLds& m, int nd, int npar, int lane) {
  const int np2 = npar * npar;
  for (int d = 0; d < nd; ++d) {
    const double* const L = m.L + d * np2;
    const double* const B = m.B + d * np2;
    double* const x = m.x + d * npar;
    double s = 0.0;
    if (lane < npar && d > 0)
      for (int k = 0; k < npar; ++k) s = s + B[lane * npar + k] * x[k - npar];
    for (int k = 0; k < npar; ++k) {
      if (lane == k) x[k] = (x[k] - s) / L[k * npar + k];
      __syncthreads();
      if (lane > k && lane < npar) s = s + L[lane * npar + k] * x[k];
    }
  }
  for (int d = nd - 1; d >= 0; --d) {
    const double* const L = m.L + d * np2;
    double* const x = m.x + d * npar;
    double s = 0.0;
    if (lane < npar && d < nd - 1) {
      const double* const Bn = m.B + (d + 1) * np2;
      for (int k = 0; k < npar; ++k) s = s + Bn[k * npar + lane] * x[npar + k];
    }
    for (int j = npar - 1; j >= 0; --j) {
      if (lane == j) {
        double t = s;
        for (int k = j + 1; k < npar; ++k) t = t + L[k * npar + j] * x[k];
        x[j] = (x[j] - t) / L[j * npar + j];
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(WAVE) void k_lm_step_chain(ChainArgs a) {
  extern __shared__ double sh[];
  const long long pix = blockIdx.x;
  const int lane = threadIdx.x;
  const crt_lm_state& S = a.st;
  if (S.status[pix] != CRT_LM_RUNNING) return;  // (the whole wave, before any barrier)
  const int npar = a.npar, nd = a.nd, nv = nd * npar, ntri = npar * (npar + 1) / 2, nsum = ntri + npar;
  const long long c0 = pix * nd;
  const ChainLds m = chain_lds(sh, nd, npar);
  const double* const wp = a.wdyn ? a.wdyn + pix * a.dyn_stride : nullptr;  // (read only where nd > 1; the entry refused NULL there)
  double* const P = S.p + c0 * npar;
  double* const PT = S.p_trial + c0 * npar;

  // ---- the cost at the trial point: c2 of every date, one per lane, and the coupling terms e * e, one per lane, into LDS; then ONE lane
  // adds them in the order of the header (e, e * e and every sum rounded on their own, as there) and the wave reads the result ----
  for (int d = lane; d < nd; d += WAVE) m.x[d] = date_entry(a, c0 + d, nsum, ntri, npar);
  for (int r = lane; r < nv - npar; r += WAVE) {  // r = d * npar + k, d < nd - 1 (wp is read only here and below: nd > 1)
    const double e = (PT[r + npar] - PT[r]) * wp[r];
    m.sc[r] = e * e;
  }
  __syncthreads();
  if (lane == 0) {
    double tot = m.x[0];
    for (int d = 1; d < nd; ++d) tot = tot + m.x[d];
    for (int r = 0; r < nv - npar; ++r) tot = tot + m.sc[r];
    m.T[0] = 0.5 * tot;
  }
  __syncthreads();
  const double cost_t = m.T[0];
  const double cost = S.cost[pix];
  double lam = S.lam[pix];
  int status = CRT_LM_RUNNING;
  const bool accept = cost_t < cost;
  double new_cost = cost;
  if (accept) {
    for (int r = lane; r < nv; r += WAVE) P[r] = PT[r];
    for (int idx = lane; idx < nd * nsum; idx += WAVE) {
      const int d = idx / nsum, e = idx - d * nsum;
      const double v = date_entry(a, c0 + d, e, ntri, npar);
      if (e < ntri) S.A[(c0 + d) * ntri + e] = v;
      else S.g[(c0 + d) * npar + e - ntri] = v;
    }
    lam = fmax(lam * a.lam_down, a.lam_min);
    if (cost - cost_t < a.ftol * cost_t) status = CRT_LM_CONVERGED_F;
    new_cost = cost_t;
  } else if (cost == INFINITY) {
    status = CRT_LM_FAILED_START;
  } else {
    lam = lam * a.lam_up;
    if (lam > a.lam_max) status = CRT_LM_STALLED;
  }
  __syncthreads();  // the c2 are consumed; what the wave wrote of p, A and g is visible to all its lanes

  // ---- the next trial point: H and G from the stored A, g and the accepted p ----
  if (status == CRT_LM_RUNNING) {
    const double* const A = S.A + c0 * ntri;
    const double* const G = S.g + c0 * npar;
    chain_scales(m, A, wp, nd, npar, lane);
    __syncthreads();
    for (int r = lane; r < nv; r += WAVE) {
      const int d = r / npar;
      const double pk = P[r];
      double gr = G[r];
      if (d > 0) {
        const double wl = m.w[r - npar];
        gr = gr + wl * ((pk - P[r - npar]) * wl);
      }
      if (d < nd - 1) {
        const double wr = m.w[r];
        gr = gr - wr * ((P[r + npar] - pk) * wr);
      }
      m.x[r] = -gr * m.sc[r];
    }
    chain_matrix(m, A, nd, npar, lam, lane);
    __syncthreads();
    chain_factor(m, nd, npar, lane);
    chain_solve(m, nd, npar, lane);
    bool far = false;
    for (int r = lane; r < nv; r += WAVE) {
      const int k = r % npar;
      const double pk = P[r];
      double pt = pk + m.x[r] * m.sc[r];
      if (a.lo && pt < a.lo[k]) pt = a.lo[k];
      if (a.hi && pt > a.hi[k]) pt = a.hi[k];
      far = far || !(fabs(pt - pk) < a.xtol * (fabs(pk) + a.xtol));
      m.h[r] = pt;
    }
    if (!__any(far)) status = CRT_LM_CONVERGED_X;
  }
  for (int r = lane; r < nv; r += WAVE) PT[r] = status == CRT_LM_RUNNING ? m.h[r] : P[r];  // (m.h[r]: written by this lane)
  if (lane == 0) {
    S.cost[pix] = new_cost;
    S.lam[pix] = lam;
    S.status[pix] = status;
    if (accept) S.naccept[pix] += 1;
    else if (status != CRT_LM_FAILED_START) S.nreject[pix] += 1;
  }
}

__global__ __launch_bounds__(WAVE) void k_lm_chain_covariance(int nd, int npar, long long dyn_stride, const double* __restrict__ wdyn,
                                                              const double* __restrict__ Aall, double* __restrict__ cov) {
  extern __shared__ double sh[];
  const long long pix = blockIdx.x;
  const int lane = threadIdx.x, np2 = npar * npar, ntri = npar * (npar + 1) / 2;
  const long long c0 = pix * nd;
  const ChainLds m = chain_lds(sh, nd, npar);
  const double* const wp = wdyn ? wdyn + pix * dyn_stride : nullptr;
  const double* const A = Aall + c0 * ntri;
  chain_scales(m, A, wp, nd, npar, lane);
  __syncthreads();
  chain_matrix(m, A, nd, npar, 0.0, lane);
  __syncthreads();
  chain_factor(m, nd, npar, lane);
  for (int d = nd - 1; d >= 0; --d) {
    const double* const L = m.L + d * np2;
    const bool last = d == nd - 1;
    if (lane < npar) {  // column `lane` of W = L^-1
      const int j = lane;
      for (int i = 0; i < j; ++i) m.W[i * npar + j] = 0.0;
      m.W[j * npar + j] = 1.0 / L[j * npar + j];
      for (int i = j + 1; i < npar; ++i) {
        double t = 0.0;
        for (int k = j; k < i; ++k) t = t + L[i * npar + k] * m.W[k * npar + j];
        m.W[i * npar + j] = -t / L[i * npar + i];
      }
    }
    __syncthreads();
    if (!last) {
      const double* const Bn = m.B + (d + 1) * np2;
      for (int e = lane; e < np2; e += WAVE) {  // C = B_{d+1} W
        const int i = e / npar, j = e - i * npar;
        double t = 0.0;
        for (int k = 0; k < npar; ++k) t = t + Bn[i * npar + k] * m.W[k * npar + j];
        m.C[e] = t;
      }
      __syncthreads();
      for (int e = lane; e < np2; e += WAVE) {  // T = S_{d+1} C
        const int i = e / npar, j = e - i * npar;
        double t = 0.0;
        for (int k = 0; k < npar; ++k) t = t + m.S[i * npar + k] * m.C[k * npar + j];
        m.T[e] = t;
      }
      __syncthreads();
    }
    for (int e = lane; e < np2; e += WAVE) {  // S_d = W^T W + C^T T: the lower triangle, mirrored
      const int i = e / npar, j = e - i * npar;
      if (j > i) continue;
      double t = 0.0;
      for (int k = 0; k < npar; ++k) t = t + m.W[k * npar + i] * m.W[k * npar + j];
      if (!last)
        for (int k = 0; k < npar; ++k) t = t + m.C[k * npar + i] * m.T[k * npar + j];
      m.S[i * npar + j] = t, m.S[j * npar + i] = t;
      const int ri = d * npar + i, rj = d * npar + j;
      double z = (t * m.sc[ri]) * m.sc[rj];
      if (m.h[ri] <= 0.0 || m.h[rj] <= 0.0) z = i == j ? INFINITY : 0.0;
      double* const out = cov + (c0 + d) * np2;
      out[i * npar + j] = z, out[j * npar + i] = z;
    }
    __syncthreads();
  }
}

bool chain_ok(const crt_lm_chain* ch, int npar) {
  if (!ch || ch->npix < 1 || ch->nd < 1) return false;
  if (ch->dyn_stride != 0 && ch->dyn_stride != (int64_t)(ch->nd - 1) * npar) return false;
  return ch->nd == 1 || ch->inv_sigma_dyn;
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int32_t crt_hip_lm_chain_max_nd(int32_t npar) {
  if (npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR) return 0;
  return (int32_t)((CRT_LM_CHAIN_LDS_LIMIT / 8 - 4 * npar * npar - 64) / (2 * npar * npar + 4 * npar));
}

int crt_hip_lm_normal_f64(int32_t ncol, int32_t npar, const crt_lm_obs* obs, int32_t nblk, double* A, double* g, double* c2,
                          crt_stream_t stream) {
  if (ncol < 1 || npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || !obs || nblk < 1 || nblk > CRT_LM_MAX_BLOCKS || !A || !g || !c2)
    return CRT_ERR_BAD_ARG;
  NormalArgs a = {};
  for (int q = 0; q < nblk; ++q) {
    if (obs[q].nrow < 1 || !obs[q].f || !obs[q].J || !obs[q].y) return CRT_ERR_BAD_ARG;
    a.blk[q] = RowBlock{obs[q].f, obs[q].J, obs[q].y, obs[q].inv_sigma, obs[q].nrow};
  }
  a.nblk = nblk, a.npar = npar, a.A = A, a.g = g, a.c2 = c2;
  const int st = launch_kernel(k_lm_normal, dim3(ncol), WAVE, 0, static_cast<hipStream_t>(stream), a);
  if (st == CRT_OK) note_kernel("k_lm_normal npar=%d nblk=%d", npar, nblk);
  return st;
}

int crt_hip_lm_step_chain_f64(const crt_lm_chain* chain, const crt_lm_problem* prob, const crt_lm_normal_block* blocks, int32_t nblk,
                              const crt_lm_state* state, crt_stream_t stream) {
  if (!chain || !prob || !blocks || !state) return CRT_ERR_BAD_ARG;
  if (prob->ncol < 1 || prob->npar < 1 || prob->npar > CRT_RETRIEVE_MAX_NPAR || nblk < 1 || nblk > CRT_LM_MAX_BLOCKS) return CRT_ERR_BAD_ARG;
  if (!(prob->lam_up > 1.0) || !(prob->lam_down > 0.0 && prob->lam_down <= 1.0)) return CRT_ERR_BAD_ARG;
  if (!(prob->lam_min >= 0.0) || !(prob->lam_max >= prob->lam_min) || !(prob->xtol >= 0.0) || !(prob->ftol >= 0.0)) return CRT_ERR_BAD_ARG;
  if (!prob->prior != !prob->inv_sigma_prior) return CRT_ERR_BAD_ARG;
  if (!state->p || !state->p_trial || !state->cost || !state->lam || !state->A || !state->g || !state->status || !state->naccept ||
      !state->nreject)
    return CRT_ERR_BAD_ARG;
  if (!chain_ok(chain, prob->npar) || (int64_t)chain->npix * chain->nd != prob->ncol) return CRT_ERR_BAD_ARG;
  ChainArgs a = {};
  for (int q = 0; q < nblk; ++q) {
    if (!blocks[q].A || !blocks[q].g || !blocks[q].c2) return CRT_ERR_BAD_ARG;
    a.blk[q] = SumBlock{blocks[q].A, blocks[q].g, blocks[q].c2};
  }
  if (chain->nd > crt_hip_lm_chain_max_nd(prob->npar)) return CRT_ERR_UNSUPPORTED;
  a.nblk = nblk, a.npar = prob->npar, a.nd = chain->nd;
  a.dyn_stride = chain->dyn_stride, a.wdyn = chain->nd > 1 ? chain->inv_sigma_dyn : nullptr;
  a.lam_up = prob->lam_up, a.lam_down = prob->lam_down, a.lam_min = prob->lam_min, a.lam_max = prob->lam_max;
  a.xtol = prob->xtol, a.ftol = prob->ftol;
  a.lo = prob->lo, a.hi = prob->hi, a.prior = prob->prior, a.isp = prob->inv_sigma_prior;
  a.st = *state;
  const size_t sh = (size_t)CRT_LM_CHAIN_LDS_BYTES(chain->nd, prob->npar);
  const int st = launch_kernel(k_lm_step_chain, dim3(chain->npix), WAVE, sh, static_cast<hipStream_t>(stream), a);
  if (st == CRT_OK) note_kernel("k_lm_step_chain nd=%d npar=%d nblk=%d", chain->nd, prob->npar, nblk);
  return st;
}

int crt_hip_lm_chain_covariance_f64(const crt_lm_chain* chain, int32_t npar, const double* A, double* cov, crt_stream_t stream) {
  if (npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || !A || !cov || !chain_ok(chain, npar)) return CRT_ERR_BAD_ARG;
  if (chain->nd > crt_hip_lm_chain_max_nd(npar)) return CRT_ERR_UNSUPPORTED;
  const size_t sh = (size_t)CRT_LM_CHAIN_LDS_BYTES(chain->nd, npar);
  const int st = launch_kernel(k_lm_chain_covariance, dim3(chain->npix), WAVE, sh, static_cast<hipStream_t>(stream), (int)chain->nd, (int)npar,
                               (long long)chain->dyn_stride, chain->nd > 1 ? chain->inv_sigma_dyn : nullptr, A, cov);
  if (st == CRT_OK) note_kernel("k_lm_chain_covariance nd=%d npar=%d", chain->nd, npar);
  return st;
}

}  // extern "C"
