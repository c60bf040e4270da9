// The Levenberg-Marquardt step on a chain of coupled dates, with or without parameters shared by all dates of a pixel
// (include_chain/crt1d_hip_lm_chain.h, include_shared/crt1d_hip_lm_shared.h): the three kernels and the C entries of both headers.
//
//  k_lm_normal             one wave per column: the sums of k_lm_step (retrieve.hip) over the observation rows, written instead of consumed
//  k_lm_step_shared        one wave per pixel: the per-date sums as k_lm_step_normal (specfit.hip) forms them, the pixel's cost with the
//                          random-walk terms, accept / reject, the factorisation of the damped, scaled arrowhead system -- the block
//                          Cholesky along the chain at the nv varying parameters, the ns border rows eliminated along the chain, the
//                          ns x ns Schur complement factorised at the end --, the substitutions and the next trial point of every date
//  k_lm_shared_covariance  one wave per pixel: the same factors with lam = 0, the backward recursion for the diagonal blocks of the
//                          inverse plus the border terms
//
// ONE kernel pair serves both headers.  crt_hip_lm_step_chain_f64 / crt_hip_lm_chain_covariance_f64 launch it with an empty shared set
// (mask = 0, nv = npar, ns = 0): the index map is the identity, every border loop has a trip count of zero, and what is left is the block
// Cholesky of the block-tridiagonal matrix whose bits tests/golden/lm_chain_bits.npz pins.  The labels "k_lm_step_chain ..." and
// "k_lm_chain_covariance ..." those two entries leave in the launch report name the entry, not a kernel of their own.
//
// The work of a date's block is spread over the lanes (one row of the sub-diagonal solve, one entry of B B^T, one row below a pivot per
// lane); every entry still is one running sum in ascending column order, so the order of the headers holds and a single date without a
// border gives scaled_cholesky's bits.  All per-date storage is dynamic LDS sized by (nd, nv, ns): no per-lane arrays, no scratch.
//
// Phases of a date d in the factorisation (no barrier is there for the border alone):
//   A  one row per lane: the rows of B_d against L_{d-1}^T and, on ns more lanes, the rows of the border block Y_{d-1} against the same
//      factor, each entry's running sum resumed from what phase B of the date before stored in R
//   B  one entry per lane: T = B_d B_d^T; R = Y_{d-1} B_d^T (the head of Y_d's running sums); the corner sums += Y_{d-1} Y_{d-1}^T
//   C  the left-looking factorisation of the diagonal block
// and after the last date the rows of Y_{nd-1}, the last corner update and the corner's factorisation by one lane, as scaled_cholesky.
//
// Bounds: every global index is c * (row length) + (index < row length) with c < npix * nd, every LDS index lies inside the carve-up of
// shared_lds() whose size the entry checked against the limit; kv / ks hold parameter indices < npar <= 10.
#include "crt1d_hip_lm_shared.h"
#include "crt_internal.hpp"
#include "lm_common.hpp"

namespace crt {
namespace {

constexpr int MAXA = MAXP + 1;                 // a row of (w_o0 .. w_o,npar-1, r_o)
constexpr int WAVE = 64;                       // one wave per column (k_lm_normal) or per pixel; also the rows staged at a time

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
// the chain: nv varying parameters per date, ns shared ones (the chain entries: ns = 0)

struct SharedArgs {
  SumBlock blk[CRT_LM_MAX_BLOCKS];
  int nblk, npar, nd, nv, ns;
  unsigned mask;
  long long dyn_stride;
  const double* wdyn;
  double lam_up, lam_down, lam_min, lam_max, xtol, ftol;
  const double *lo, *hi, *prior, *isp;
  crt_lm_state st;
};

// the dynamic LDS of a pixel, in doubles: CRT_LM_SHARED_LDS_BYTES / 8
struct SharedLds {
  double *L, *B;            // [nd][nv][nv] the diagonal blocks of M, replaced by their factors, and the sub-diagonal blocks (block 0 unused)
  double *x, *sc, *w, *h;   // [nd][nv] (x: [nd] where nv == 0, the c2 of the dates)
  double *T, *W, *C, *S;    // [nv][nv]
  double* misc;             // [64]: the cost, then the index maps
  double* Y;                // [nd][ns][nv] the border blocks, replaced by their factors (covariance: by Z_d, transposed)
  double *K, *KT, *Ki;      // [ns][ns] the corner (replaced by its factor), its running sums (covariance: the factor's inverse), S^-1
  double *R, *Q;            // [ns][nv] the heads of Y's running sums (covariance: [nv][ns] work arrays)
  double *xs, *ss, *hs, *ps;  // [ns] right-hand side / solution, scales, diagonal of H, trial values
  int *kv, *ks;             // the varying and the shared parameter indices, ascending
};

__device__ inline SharedLds shared_lds(double* sh, int nd, int nv, int ns) {
  const int np2 = nv * nv, nt = nd * nv;
  SharedLds m;
  m.L = sh, m.B = m.L + nd * np2, m.x = m.B + nd * np2, m.sc = m.x + (nv ? nt : nd), m.w = m.sc + nt, m.h = m.w + nt;
  m.T = m.h + nt, m.W = m.T + np2, m.C = m.W + np2, m.S = m.C + np2, m.misc = m.S + np2;
  m.Y = m.misc + 64, m.K = m.Y + nt * ns, m.KT = m.K + ns * ns, m.Ki = m.KT + ns * ns;
  m.R = m.Ki + ns * ns, m.Q = m.R + nv * ns, m.xs = m.Q + nv * ns, m.ss = m.xs + ns, m.hs = m.ss + ns, m.ps = m.hs + ns;
  m.kv = reinterpret_cast<int*>(m.misc + 8), m.ks = m.kv + CRT_RETRIEVE_MAX_NPAR;
  return m;
}

__device__ inline void index_maps(const SharedLds& m, unsigned mask, int npar, int lane) {
  if (lane < npar) {
    const int below = __popc(mask & ((1u << lane) - 1u));
    if ((mask >> lane) & 1u) m.ks[below] = lane;
    else m.kv[lane - below] = lane;
  }
}

// Entry e of (A | g | c2) of column c as k_lm_step_normal forms it: block 0's bits, the blocks 1.. in ascending order, then the prior rows
// in ascending k -- of which an entry of A or g sees at most one.
__device__ inline double date_entry(const SharedArgs& a, long long c, int e, int ntri, int npar) {
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

// h = diag H, the scales and the weights: per (date, varying parameter) with the coupling weights, the sums over the dates for the shared ones
__device__ inline void shared_scales(const SharedLds& m, const double* A, const double* wp, int nd, int npar, int nv, int ns, int lane) {
  const int ntri = npar * (npar + 1) / 2;
  for (int r = lane; r < nd * nv; r += WAVE) {
    const int d = r / nv, k = m.kv[r - d * nv];
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
  if (lane < ns) {
    const int k = m.ks[lane];
    double h = A[tri(k, k)];
    for (int d = 1; d < nd; ++d) h = h + A[(long long)d * ntri + tri(k, k)];
    m.hs[lane] = h;
    m.ss[lane] = h <= 0.0 ? 1.0 : 1.0 / sqrt(h);
  }
}

// M = (H_rq s_r) s_q + (dead ? 1 : lam) [r == q]: the diagonal and sub-diagonal blocks of the varying part into L and B, the border into Y, the corner into K (KT = +0)
__device__ inline void shared_matrix(const SharedLds& m, const double* A, int nd, int npar, int nv, int ns, double lam, int lane) {
  const int ntri = npar * (npar + 1) / 2, np2 = nv * nv, nyv = ns * nv;
  for (int idx = lane; idx < nd * np2; idx += WAVE) {
    const int d = idx / np2, e = idx - d * np2, i = e / nv, j = e - i * nv;
    double v = 0.0, b = 0.0;
    if (j <= i) {
      const double hij = i == j ? m.h[d * nv + i] : A[(long long)d * ntri + tri(m.kv[i], m.kv[j])];
      v = (hij * m.sc[d * nv + i]) * m.sc[d * nv + j];
      if (i == j) v = v + (hij <= 0.0 ? 1.0 : lam);
    }
    if (d > 0 && i == j) {
      const double wl = m.w[(d - 1) * nv + i];
      b = ((-(wl * wl)) * m.sc[d * nv + i]) * m.sc[(d - 1) * nv + i];
    }
    m.L[idx] = v, m.B[idx] = b;
  }
  for (int idx = lane; idx < nd * nyv; idx += WAVE) {
    const int d = idx / nyv, e = idx - d * nyv, i = e / nv, j = e - i * nv;
    m.Y[idx] = (A[(long long)d * ntri + symtri(m.ks[i], m.kv[j])] * m.ss[i]) * m.sc[d * nv + j];
  }
  for (int e = lane; e < ns * ns; e += WAVE) {
    const int i = e / ns, l = e - i * ns;
    double v = 0.0;
    if (l <= i) {
      double hil = m.hs[i];
      if (i != l) {
        const int t = tri(m.ks[i], m.ks[l]);
        hil = A[t];
        for (int d = 1; d < nd; ++d) hil = hil + A[(long long)d * ntri + t];
      }
      v = (hil * m.ss[i]) * m.ss[l];
      if (i == l) v = v + (hil <= 0.0 ? 1.0 : lam);
    }
    m.K[e] = v, m.KT[e] = 0.0;
  }
}

// corner sums += Y Y^T of one date, one entry per lane
__device__ inline void corner_update(const SharedLds& m, const double* Y, int nv, int ns, int lane) {
  for (int e = lane; e < ns * ns; e += WAVE) {
    const int i = e / ns, l = e - i * ns;
    if (l > i) continue;
    double t = m.KT[e];
    for (int k = 0; k < nv; ++k) t = t + Y[i * nv + k] * Y[l * nv + k];
    m.KT[e] = t;
  }
}

// The factorisation of the arrowhead, in place (the phases of the file header).  (Uniform trip counts: every lane reaches every barrier.)
__device__ inline void shared_factor(const SharedLds& m, int nd, int nv, int ns, int lane) {
  const int np2 = nv * nv, nyv = ns * nv;
  if (nv > 0) {
    for (int d = 0; d <= nd; ++d) {  // (d == nd: only the rows of the last border block and the last corner update)
      double* const L = m.L + d * np2;
      double* const B = m.B + d * np2;
      double* const Yp = m.Y + (d - 1) * nyv;  // (read for d > 0 only)
      if (d > 0) {
        const double* const Lp = L - np2;
        const bool isb = lane < nv && d < nd, isy = lane >= nv && lane < nv + ns;
        if (isb || isy) {
          double* const row = isb ? B + lane * nv : Yp + (lane - nv) * nv;
          const double* const r0 = m.R + (isy ? (lane - nv) * nv : 0);
          for (int k = 0; k < nv; ++k) {
            double t = isy ? r0[k] : 0.0;
            for (int q = 0; q < k; ++q) t = t + row[q] * Lp[k * nv + q];
            row[k] = (row[k] - t) / Lp[k * nv + k];
          }
        }
        __syncthreads();
      }
      if (d < nd) {
        for (int e = lane; e < np2; e += WAVE) {
          const int i = e / nv, j = e - i * nv;
          double t = 0.0;
          if (d > 0 && j <= i)
            for (int k = 0; k < nv; ++k) t = t + B[i * nv + k] * B[j * nv + k];
          m.T[e] = t;
        }
        for (int e = lane; e < nyv; e += WAVE) {
          const int i = e / nv, j = e - i * nv;
          double t = 0.0;
          if (d > 0)
            for (int k = 0; k < nv; ++k) t = t + Yp[i * nv + k] * B[j * nv + k];
          m.R[e] = t;
        }
      }
      if (d > 0) corner_update(m, Yp, nv, ns, lane);
      __syncthreads();
      if (d == nd) break;
      for (int j = 0; j < nv; ++j) {
        if (lane == j) {
          double s = m.T[j * nv + j];
          for (int k = 0; k < j; ++k) s = s + L[j * nv + k] * L[j * nv + k];
          L[j * nv + j] = sqrt(L[j * nv + j] - s);
        }
        __syncthreads();
        if (lane > j && lane < nv) {
          double t = m.T[lane * nv + j];
          for (int k = 0; k < j; ++k) t = t + L[lane * nv + k] * L[j * nv + k];
          L[lane * nv + j] = (L[lane * nv + j] - t) / L[j * nv + j];
        }
        __syncthreads();
      }
    }
  }
  if (lane == 0) {  // the corner: scaled_cholesky's loop, every running sum resumed from the border's
    for (int j = 0; j < ns; ++j) {
      double s = m.KT[j * ns + j];
      for (int k = 0; k < j; ++k) s = s + m.K[j * ns + k] * m.K[j * ns + k];
      const double dj = sqrt(m.K[j * ns + j] - s);
      m.K[j * ns + j] = dj;
      for (int i = j + 1; i < ns; ++i) {
        double t = m.KT[i * ns + j];
        for (int k = 0; k < j; ++k) t = t + m.K[i * ns + k] * m.K[j * ns + k];
        m.K[i * ns + j] = (m.K[i * ns + j] - t) / dj;
      }
    }
  }
  __syncthreads();
}

// L L^T x = x in place on (x, xs), in the order of the header
__device__ inline void shared_solve(const SharedLds& m, int nd, int nv, int ns, int lane) {
  const int np2 = nv * nv, nyv = ns * nv;
  if (nv > 0)
    for (int d = 0; d < nd; ++d) {
      const double* const L = m.L + d * np2;
      const double* const B = m.B + d * np2;
      double* const x = m.x + d * nv;
      double s = 0.0;
      if (lane < nv && d > 0)
        for (int k = 0; k < nv; ++k) s = s + B[lane * nv + k] * x[k - nv];
      for (int k = 0; k < nv; ++k) {
        if (lane == k) x[k] = (x[k] - s) / L[k * nv + k];
        __syncthreads();
        if (lane > k && lane < nv) s = s + L[lane * nv + k] * x[k];
      }
    }
  if (lane < ns) {  // the head of u of a border row: all varying columns, d ascending then j ascending
    double u = 0.0;
    for (int d = 0; d < nd; ++d) {
      const double* const Y = m.Y + d * nyv + lane * nv;
      for (int j = 0; j < nv; ++j) u = u + Y[j] * m.x[d * nv + j];
    }
    m.ps[lane] = u;
  }
  __syncthreads();
  if (lane == 0) {
    for (int i = 0; i < ns; ++i) {
      double s = m.ps[i];
      for (int k = 0; k < i; ++k) s = s + m.K[i * ns + k] * m.xs[k];
      m.xs[i] = (m.xs[i] - s) / m.K[i * ns + i];
    }
    for (int i = ns - 1; i >= 0; --i) {
      double s = 0.0;
      for (int k = i + 1; k < ns; ++k) s = s + m.K[k * ns + i] * m.xs[k];
      m.xs[i] = (m.xs[i] - s) / m.K[i * ns + i];
    }
  }
  __syncthreads();
  if (nv > 0)
    for (int d = nd - 1; d >= 0; --d) {
      const double* const L = m.L + d * np2;
      const double* const Y = m.Y + d * nyv;
      double* const x = m.x + d * nv;
      double s = 0.0;
      if (lane < nv) {
        for (int i = 0; i < ns; ++i) s = s + Y[i * nv + lane] * m.xs[i];
        if (d < nd - 1) {
          const double* const Bn = m.B + (d + 1) * np2;
          for (int k = 0; k < nv; ++k) s = s + Bn[k * nv + lane] * x[nv + k];
        }
      }
      for (int j = nv - 1; j >= 0; --j) {
        if (lane == j) {
          double t = s;
          for (int k = j + 1; k < nv; ++k) t = t + L[k * nv + j] * x[k];
          x[j] = (x[j] - t) / L[j * nv + j];
        }
        __syncthreads();
      }
    }
}

__global__ __launch_bounds__(WAVE) void k_lm_step_shared(SharedArgs a) {
  extern __shared__ double sh[];
  const long long pix = blockIdx.x;
  const int lane = threadIdx.x;
  const crt_lm_state& S = a.st;
  if (S.status[pix] != CRT_LM_RUNNING) return;  // (the whole wave, before any barrier)
  const int npar = a.npar, nd = a.nd, nv = a.nv, ns = a.ns, nt = nd * nv, ntri = npar * (npar + 1) / 2, nsum = ntri + npar;
  const unsigned mask = a.mask;
  const long long c0 = pix * nd;
  const SharedLds m = shared_lds(sh, nd, nv, ns);
  const double* const wp = a.wdyn ? a.wdyn + pix * a.dyn_stride : nullptr;  // (read only where nd > 1; the entry refused NULL there)
  double* const P = S.p + c0 * npar;
  double* const PT = S.p_trial + c0 * npar;
  index_maps(m, mask, npar, lane);
  __syncthreads();

  // ---- the cost at the trial point: the c2 and the e * e into LDS, then ONE lane adds them in the header's order ----
  for (int d = lane; d < nd; d += WAVE) m.x[d] = date_entry(a, c0 + d, nsum, ntri, npar);
  for (int r = lane; r < nt - nv; r += WAVE) {  // r = d * nv + j, d < nd - 1
    const int d = r / nv, o = d * npar + m.kv[r - d * nv];
    const double e = (PT[o + npar] - PT[o]) * wp[o];
    m.sc[r] = e * e;
  }
  __syncthreads();
  if (lane == 0) {
    double tot = m.x[0];
    for (int d = 1; d < nd; ++d) tot = tot + m.x[d];
    for (int r = 0; r < nt - nv; ++r) tot = tot + m.sc[r];
    m.misc[0] = 0.5 * tot;
  }
  __syncthreads();
  const double cost_t = m.misc[0];
  const double cost = S.cost[pix];
  double lam = S.lam[pix];
  int status = CRT_LM_RUNNING;
  const bool accept = cost_t < cost;
  double new_cost = cost;
  if (accept) {
    for (int r = lane; r < nd * npar; r += WAVE) {
      const int k = r % npar;
      P[r] = PT[(mask >> k) & 1u ? k : r];  // a shared parameter: date 0's bits on every date
    }
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
    shared_scales(m, A, wp, nd, npar, nv, ns, lane);
    __syncthreads();
    for (int r = lane; r < nt; r += WAVE) {
      const int d = r / nv, o = d * npar + m.kv[r - d * nv];
      const double pk = P[o];
      double gr = G[o];
      if (d > 0) {
        const double wl = m.w[r - nv];
        gr = gr + wl * ((pk - P[o - npar]) * wl);
      }
      if (d < nd - 1) {
        const double wr = m.w[r];
        gr = gr - wr * ((P[o + npar] - pk) * wr);
      }
      m.x[r] = -gr * m.sc[r];
    }
    if (lane < ns) {
      const int k = m.ks[lane];
      double gr = G[k];
      for (int d = 1; d < nd; ++d) gr = gr + G[d * npar + k];
      m.xs[lane] = -gr * m.ss[lane];
    }
    shared_matrix(m, A, nd, npar, nv, ns, lam, lane);
    __syncthreads();
    shared_factor(m, nd, nv, ns, lane);
    shared_solve(m, nd, nv, ns, lane);
    bool far = false;
    for (int r = lane; r < nt; r += WAVE) {
      const int d = r / nv, k = m.kv[r - d * nv];
      const double pk = P[d * npar + k];
      double pt = pk + m.x[r] * m.sc[r];
      if (a.lo && pt < a.lo[k]) pt = a.lo[k];
      if (a.hi && pt > a.hi[k]) pt = a.hi[k];
      far = far || !(fabs(pt - pk) < a.xtol * (fabs(pk) + a.xtol));
      m.h[r] = pt;
    }
    if (lane < ns) {
      const int k = m.ks[lane];
      const double pk = P[k];
      double pt = pk + m.xs[lane] * m.ss[lane];
      if (a.lo && pt < a.lo[k]) pt = a.lo[k];
      if (a.hi && pt > a.hi[k]) pt = a.hi[k];
      far = far || !(fabs(pt - pk) < a.xtol * (fabs(pk) + a.xtol));
      m.ps[lane] = pt;
    }
    if (!__any(far)) status = CRT_LM_CONVERGED_X;
    __syncthreads();  // the trial values are read by other lanes than wrote them
  }
  for (int r = lane; r < nd * npar; r += WAVE) {
    const int d = r / npar, k = r - d * npar, below = __popc(mask & ((1u << k) - 1u));
    double v = P[r];
    if (status == CRT_LM_RUNNING) v = (mask >> k) & 1u ? m.ps[below] : m.h[d * nv + k - below];
    PT[r] = v;
  }
  if (lane == 0) {
    S.cost[pix] = new_cost;
    S.lam[pix] = lam;
    S.status[pix] = status;
    if (accept) S.naccept[pix] += 1;
    else if (status != CRT_LM_FAILED_START) S.nreject[pix] += 1;
  }
}

__global__ __launch_bounds__(WAVE) void k_lm_shared_covariance(int nd, int npar, int nv, int ns, unsigned mask, long long dyn_stride,
                                                               const double* __restrict__ wdyn, const double* __restrict__ Aall,
                                                               double* __restrict__ cov) {
  extern __shared__ double sh[];
  const long long pix = blockIdx.x;
  const int lane = threadIdx.x, np2 = nv * nv, nyv = ns * nv, ntri = npar * (npar + 1) / 2, npp = npar * npar;
  const long long c0 = pix * nd;
  const SharedLds m = shared_lds(sh, nd, nv, ns);
  const double* const wp = wdyn ? wdyn + pix * dyn_stride : nullptr;
  const double* const A = Aall + c0 * ntri;
  index_maps(m, mask, npar, lane);
  __syncthreads();
  shared_scales(m, A, wp, nd, npar, nv, ns, lane);
  __syncthreads();
  shared_matrix(m, A, nd, npar, nv, ns, 0.0, lane);
  __syncthreads();
  shared_factor(m, nd, nv, ns, lane);
  // S^-1 = Lc^-T Lc^-1: the columns of Lc^-1 into KT, one per lane, then one entry of Ki per lane
  if (lane < ns) {
    const int j = lane;
    for (int i = 0; i < j; ++i) m.KT[i * ns + j] = 0.0;
    m.KT[j * ns + j] = 1.0 / m.K[j * ns + j];
    for (int i = j + 1; i < ns; ++i) {
      double t = 0.0;
      for (int k = j; k < i; ++k) t = t + m.K[i * ns + k] * m.KT[k * ns + j];
      m.KT[i * ns + j] = -t / m.K[i * ns + i];
    }
  }
  __syncthreads();
  for (int e = lane; e < ns * ns; e += WAVE) {
    const int i = e / ns, l = e - i * ns;
    double t = 0.0;
    for (int k = 0; k < ns; ++k) t = t + m.KT[k * ns + i] * m.KT[k * ns + l];
    m.Ki[e] = t;
  }
  __syncthreads();
  for (int d = nd - 1; d >= 0; --d) {
    double* const out = cov + (c0 + d) * npp;
    for (int e = lane; e < ns * ns; e += WAVE) {  // the shared-shared block: the same bits on every date
      const int i = e / ns, l = e - i * ns;
      if (l > i) continue;  // the lower triangle, mirrored: the two scalings do not commute in the last bit
      double z = (m.Ki[e] * m.ss[i]) * m.ss[l];
      if (m.hs[i] <= 0.0 || m.hs[l] <= 0.0) z = i == l ? INFINITY : 0.0;
      out[m.ks[i] * npar + m.ks[l]] = z, out[m.ks[l] * npar + m.ks[i]] = z;
    }
    if (nv == 0) continue;
    const double* const L = m.L + d * np2;
    const double* const Bn = m.B + (d + 1) * np2;  // (read for !last only)
    double* const Yd = m.Y + d * nyv;              // Y_d [ns][nv], replaced by Z_d transposed: Z_d[j][i] at Yd[i * nv + j]
    const double* const Yn = Yd + nyv;
    const bool last = d == nd - 1;
    if (lane < nv) {  // column `lane` of W = L^-1
      const int j = lane;
      for (int i = 0; i < j; ++i) m.W[i * nv + j] = 0.0;
      m.W[j * nv + j] = 1.0 / L[j * nv + j];
      for (int i = j + 1; i < nv; ++i) {
        double t = 0.0;
        for (int k = j; k < i; ++k) t = t + L[i * nv + k] * m.W[k * nv + j];
        m.W[i * nv + j] = -t / L[i * nv + i];
      }
    }
    for (int e = lane; e < nyv; e += WAVE) {  // R = Y_d^T - B_{d+1}^T Z_{d+1}, [nv][ns]
      const int j = e / ns, i = e - j * ns;
      double t = 0.0;
      if (!last)
        for (int k = 0; k < nv; ++k) t = t + Bn[k * nv + j] * Yn[i * nv + k];
      m.R[e] = Yd[i * nv + j] - t;
    }
    __syncthreads();
    if (!last)
      for (int e = lane; e < np2; e += WAVE) {  // C = B_{d+1} W
        const int i = e / nv, j = e - i * nv;
        double t = 0.0;
        for (int k = 0; k < nv; ++k) t = t + Bn[i * nv + k] * m.W[k * nv + j];
        m.C[e] = t;
      }
    for (int e = lane; e < nyv; e += WAVE) {  // Z_d = W^T R
      const int j = e / ns, i = e - j * ns;
      double t = 0.0;
      for (int k = 0; k < nv; ++k) t = t + m.W[k * nv + j] * m.R[k * ns + i];
      Yd[i * nv + j] = t;
    }
    __syncthreads();
    if (!last)
      for (int e = lane; e < np2; e += WAVE) {  // T = S_{d+1} C
        const int i = e / nv, j = e - i * nv;
        double t = 0.0;
        for (int k = 0; k < nv; ++k) t = t + m.S[i * nv + k] * m.C[k * nv + j];
        m.T[e] = t;
      }
    for (int e = lane; e < nyv; e += WAVE) {  // Q = Z_d S^-1, [nv][ns]
      const int j = e / ns, i = e - j * ns;
      double t = 0.0;
      for (int l = 0; l < ns; ++l) t = t + Yd[l * nv + j] * m.Ki[l * ns + i];
      m.Q[e] = t;
    }
    __syncthreads();
    for (int e = lane; e < np2; e += WAVE) {  // S_d = W^T W + C^T T, the recursion of the block-tridiagonal part; the output adds Q Z_d^T
      const int i = e / nv, j = e - i * nv;
      if (j > i) continue;
      double t = 0.0;
      for (int k = 0; k < nv; ++k) t = t + m.W[k * nv + i] * m.W[k * nv + j];
      if (!last)
        for (int k = 0; k < nv; ++k) t = t + m.C[k * nv + i] * m.T[k * nv + j];
      m.S[i * nv + j] = t, m.S[j * nv + i] = t;
      for (int l = 0; l < ns; ++l) t = t + m.Q[i * ns + l] * Yd[l * nv + j];
      const int ri = d * nv + i, rj = d * nv + j;
      double z = (t * m.sc[ri]) * m.sc[rj];
      if (m.h[ri] <= 0.0 || m.h[rj] <= 0.0) z = i == j ? INFINITY : 0.0;
      const int ki = m.kv[i], kj = m.kv[j];
      out[ki * npar + kj] = z, out[kj * npar + ki] = z;
    }
    for (int e = lane; e < nyv; e += WAVE) {  // the cross block -Z_d S^-1
      const int j = e / ns, i = e - j * ns;
      double z = ((-m.Q[e]) * m.sc[d * nv + j]) * m.ss[i];
      if (m.h[d * nv + j] <= 0.0 || m.hs[i] <= 0.0) z = 0.0;
      const int kj = m.kv[j], ki = m.ks[i];
      out[kj * npar + ki] = z, out[ki * npar + kj] = z;
    }
    __syncthreads();
  }
}

// The argument checks of the two step entries and the kernel's argument block; mask: the shared set (the chain entry: 0).  A bad
// argument wins over the limit.
int step_args(const crt_lm_chain* chain, unsigned mask, const crt_lm_problem* prob, const crt_lm_normal_block* blocks, int32_t nblk,
              const crt_lm_state* state, SharedArgs& a) {
  if (!chain || !blocks || !lm_problem_ok(prob, nblk, state)) return CRT_ERR_BAD_ARG;
  if (!chain_ok(chain, prob->npar) || (int64_t)chain->npix * chain->nd != prob->ncol) return CRT_ERR_BAD_ARG;
  if ((mask >> prob->npar) != 0u) return CRT_ERR_BAD_ARG;  // (npar <= 10 < 32)
  a = {};
  for (int q = 0; q < nblk; ++q) {
    if (!blocks[q].A || !blocks[q].g || !blocks[q].c2) return CRT_ERR_BAD_ARG;
    a.blk[q] = SumBlock{blocks[q].A, blocks[q].g, blocks[q].c2};
  }
  const int ns = __builtin_popcount(mask);
  if (chain->nd > crt_hip_lm_shared_max_nd(prob->npar, ns)) return CRT_ERR_UNSUPPORTED;
  a.nblk = nblk, a.npar = prob->npar, a.nd = chain->nd, a.nv = prob->npar - ns, a.ns = ns, a.mask = mask;
  a.dyn_stride = chain->dyn_stride, a.wdyn = chain->nd > 1 ? chain->inv_sigma_dyn : nullptr;
  a.lam_up = prob->lam_up, a.lam_down = prob->lam_down, a.lam_min = prob->lam_min, a.lam_max = prob->lam_max;
  a.xtol = prob->xtol, a.ftol = prob->ftol;
  a.lo = prob->lo, a.hi = prob->hi, a.prior = prob->prior, a.isp = prob->inv_sigma_prior;
  a.st = *state;
  return CRT_OK;
}

int launch_step(const SharedArgs& a, int npix, crt_stream_t stream) {
  const size_t sh = (size_t)CRT_LM_SHARED_LDS_BYTES(a.nd, a.nv, a.ns);
  return launch_kernel(k_lm_step_shared, dim3(npix), WAVE, sh, static_cast<hipStream_t>(stream), a);
}

// the checks of the two covariance entries and the launch; mask as above
int launch_covariance(const crt_lm_chain* chain, unsigned mask, int32_t npar, const double* A, double* cov, crt_stream_t stream) {
  if (npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || !A || !cov || !chain_ok(chain, npar) || (mask >> npar) != 0u) return CRT_ERR_BAD_ARG;
  const int ns = __builtin_popcount(mask), nv = npar - ns;
  if (chain->nd > crt_hip_lm_shared_max_nd(npar, ns)) return CRT_ERR_UNSUPPORTED;
  const size_t sh = (size_t)CRT_LM_SHARED_LDS_BYTES(chain->nd, nv, ns);
  return launch_kernel(k_lm_shared_covariance, dim3(chain->npix), WAVE, sh, static_cast<hipStream_t>(stream), (int)chain->nd, (int)npar, nv,
                       ns, mask, (long long)chain->dyn_stride, chain->nd > 1 ? chain->inv_sigma_dyn : nullptr, A, cov);
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int32_t crt_hip_lm_shared_max_nd(int32_t npar, int32_t ns) {
  if (npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || ns < 0 || ns > npar) return 0;
  const int nv = npar - ns;
  const int fixed = 4 * nv * nv + 64 + 3 * ns * ns + 2 * nv * ns + 4 * ns;
  const int per_date = nv ? 2 * nv * nv + 4 * nv + nv * ns : 1;
  return (int32_t)((CRT_LM_CHAIN_LDS_LIMIT / 8 - fixed) / per_date);
}

int32_t crt_hip_lm_chain_max_nd(int32_t npar) { return crt_hip_lm_shared_max_nd(npar, 0); }

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
  SharedArgs a;
  if (const int st = step_args(chain, 0u, prob, blocks, nblk, state, a)) return st;
  const int st = launch_step(a, chain->npix, stream);
  if (st == CRT_OK) note_kernel("k_lm_step_chain nd=%d npar=%d nblk=%d", chain->nd, prob->npar, nblk);
  return st;
}

int crt_hip_lm_chain_covariance_f64(const crt_lm_chain* chain, int32_t npar, const double* A, double* cov, crt_stream_t stream) {
  const int st = launch_covariance(chain, 0u, npar, A, cov, stream);
  if (st == CRT_OK) note_kernel("k_lm_chain_covariance nd=%d npar=%d", chain->nd, npar);
  return st;
}

int crt_hip_lm_step_shared_f64(const crt_lm_chain* chain, const crt_lm_shared* shared, const crt_lm_problem* prob,
                               const crt_lm_normal_block* blocks, int32_t nblk, const crt_lm_state* state, crt_stream_t stream) {
  SharedArgs a;
  if (!shared) return CRT_ERR_BAD_ARG;
  if (const int st = step_args(chain, shared->mask, prob, blocks, nblk, state, a)) return st;
  const int st = launch_step(a, chain->npix, stream);
  if (st == CRT_OK) note_kernel("k_lm_step_shared nd=%d npar=%d ns=%d nblk=%d", chain->nd, prob->npar, a.ns, nblk);
  return st;
}

int crt_hip_lm_shared_covariance_f64(const crt_lm_chain* chain, const crt_lm_shared* shared, int32_t npar, const double* A, double* cov,
                                     crt_stream_t stream) {
  if (!shared) return CRT_ERR_BAD_ARG;
  const int st = launch_covariance(chain, shared->mask, npar, A, cov, stream);
  if (st == CRT_OK) note_kernel("k_lm_shared_covariance nd=%d npar=%d ns=%d", chain->nd, npar, __builtin_popcount(shared->mask));
  return st;
}

}  // extern "C"
