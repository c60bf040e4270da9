// The look-up-table posterior (include_post/crt1d_hip_lut_posterior.h): the likelihood-weighted mean and covariance of the table's
// candidates for every column.
//
//  pass 1                 crt_hip_lut_match_f64 with nbest = 1: the best candidate kb and its cost cmin of every column
//  k_lut_moments          lane = column, candidates wave-uniform, on the skeleton of k_lut_match: a workgroup owns 64 columns and one part of
//                         the K-split, takes 64 candidates at a time (16 per wave, one running cost sum each per lane) and streams the rows
//                         through LDS CRT_LUT_ROWS at a time; after the rows of a tile every wave forms the weights of its 16 candidates and
//                         extends its strand's sums S0, Sq, S1, S2 in registers; the four strands are added through LDS in strand order and
//                         written to the workspace
//  k_lut_moments_finish   one lane per column: the parts added in ascending order, then the finish arithmetic of the header
//
// Bounds: every global index is (column < ncol) * nrow + (row < nrow) or (candidate < K) * nrow + (row < nrow), in 64 bits; a column or a
// candidate beyond the end is staged as zeros and gets the weight 0; q[k] is read only for a candidate some lane weights (k < K then) and
// q[kb] only where 0 <= kb (< K: the match wrote it).  The workspace index is ((group of 64 columns * ksplit + part) * NACC + entry) * 64 +
// lane with part < ksplit and entry < NACC: what crt_hip_lut_posterior_workspace_bytes sizes.  The LDS indices are bounded by the constants.
#include "crt1d_hip_lut_posterior.h"
#include "crt_internal.hpp"

namespace crt {
namespace {

// the tiling of k_lut_match (lut.hip), which the cost bits do not depend on and the summation order of the header is written for
constexpr int LUT_COLS = 64;
constexpr int LUT_WAVES = 4;
constexpr int LUT_TILE = 16;
constexpr int LUT_SUPER = LUT_WAVES * LUT_TILE;
constexpr int LUT_THREADS = LUT_WAVES * 64;
constexpr int LUT_RC = CRT_LUT_ROWS;
constexpr int LUT_YS = LUT_COLS + 1;  // the padded row strides of the staged arrays (lut.hip: 64 puts a staging wave into one bank pair)
constexpr int LUT_TS = LUT_COLS + 2;
constexpr int LUT_STAGE = LUT_RC * (2 * LUT_YS + LUT_TS);
constexpr int LUT_TARGET_WG = 1024;
constexpr int LUT_MAXBLK = CRT_LM_MAX_BLOCKS + 1;
constexpr long long LUT_GRID_X = 1 << 20;

constexpr int nacc(int np) { return 2 + np + np * (np + 1) / 2; }  // S0, Sq, S1[np], S2[np (np + 1) / 2]

struct PostBlk {
  const double *m, *y, *is;
  int nrow;
};

struct MomentArgs {
  PostBlk blk[LUT_MAXBLK];
  int nblk, ncol, ncand, ksplit, once;
  const double* q;      // [K][npar]
  const int* index;     // [ncol] kb, of pass 1
  const double* cost;   // [ncol] cmin
  double temperature;
  const double* temperature_col;
  double* part;         // [ntile][ksplit][NACC][64]
};

struct FinishArgs {
  int ncol, ksplit;
  const double* q;
  const double* part;
  double temperature;
  const double* temperature_col;
  int* index;
  double *cost, *mean, *cov, *wsum, *ess;
};

__device__ inline bool good_temperature(double t) { return t > 0.0 && t < INFINITY; }

template <int NP>
__global__ __launch_bounds__(LUT_THREADS) void k_lut_moments(MomentArgs a) {
  constexpr int NA = nacc(NP), NTRI = NP * (NP + 1) / 2;
  constexpr int NLDS = LUT_STAGE > NA * LUT_COLS ? LUT_STAGE : NA * LUT_COLS;  // 24.5 KiB; 33.5 KiB at NP = 10
  __shared__ __attribute__((aligned(16))) double lds[NLDS];
  double* const tb = lds;                        // [row][candidate of the 64], rows LUT_TS apart
  double* const ys = tb + LUT_RC * LUT_TS;       // [row][column], rows LUT_YS apart: y, 0 where masked
  double* const ss = ys + LUT_RC * LUT_YS;       // inv_sigma, 0 where masked
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long tile = (long long)blockIdx.z * LUT_GRID_X + blockIdx.x, c0 = tile * LUT_COLS;
  if (c0 >= a.ncol) return;  // (the whole workgroup, before any barrier: the last slice of grid.z is not full)
  const int split = blockIdx.y;
  const long long nsuper = ((long long)a.ncand + LUT_SUPER - 1) / LUT_SUPER;
  const long long st0 = split * nsuper / a.ksplit, st1 = (split + 1) * nsuper / a.ksplit;
  // this lane's column: the centre of the moments and the scale of the weights
  const long long c = c0 + lane;
  int kb = -1;
  double cmin = 0.0, it = 0.0, qb[NP];
  if (c < a.ncol) {
    const double T = a.temperature_col ? a.temperature_col[c] : a.temperature;
    if (good_temperature(T)) kb = a.index[c], cmin = a.cost[c], it = 1.0 / T;
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) qb[i] = kb >= 0 ? a.q[(long long)kb * NP + i] : 0.0;
  double s0 = 0.0, sq = 0.0, s1[NP], s2[NTRI];
#pragma unroll
  for (int i = 0; i < NP; ++i) s1[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NTRI; ++i) s2[i] = 0.0;
  for (long long st = st0; st < st1; ++st) {
    const long long kbase = st * LUT_SUPER;
    double acc[LUT_TILE];
#pragma unroll
    for (int j = 0; j < LUT_TILE; ++j) acc[j] = 0.0;
    for (int q = 0; q < a.nblk; ++q) {
      const PostBlk B = a.blk[q];
      for (int o0 = 0; o0 < B.nrow; o0 += LUT_RC) {
        const int n = min(LUT_RC, B.nrow - o0);
        __syncthreads();  // the previous rows are consumed
        if (!a.once || st == st0) {
          for (int idx = tid; idx < LUT_COLS * n; idx += LUT_THREADS) {
            const int cl = idx / n, o = idx - cl * n;
            const long long cc = c0 + cl;
            double s = 0.0, y = 0.0;
            if (cc < a.ncol) {
              const long long g = cc * B.nrow + o0 + o;
              s = B.is ? B.is[g] : 1.0;
              if (s != 0.0) y = B.y[g];
              else s = 0.0;
            }
            ys[o * LUT_YS + cl] = y, ss[o * LUT_YS + cl] = s;
          }
        }
        for (int idx = tid; idx < LUT_SUPER * n; idx += LUT_THREADS) {
          const int kk = idx / n, o = idx - kk * n;
          const long long k = kbase + kk;
          tb[o * LUT_TS + kk] = k < a.ncand ? B.m[k * B.nrow + o0 + o] : 0.0;
        }
        __syncthreads();
        // the cost loop of k_lut_match, instruction for instruction: a masked row is staged as (0, 0) and adds +0
        const double* const tw = tb + w * LUT_TILE;
#pragma unroll 2
        for (int o = 0; o < n; ++o) {
          const double y = ys[o * LUT_YS + lane], s = ss[o * LUT_YS + lane];
#pragma unroll
          for (int j = 0; j < LUT_TILE; ++j) {
            const double r = (tw[o * LUT_TS + j] - y) * s;
            acc[j] = acc[j] + r * r;
          }
        }
      }
    }
    // this wave's 16 candidates, in ascending order, onto its strand's sums
#pragma unroll
    for (int j = 0; j < LUT_TILE; ++j) {
      const long long k = kbase + w * LUT_TILE + j;
      const double cost = 0.5 * acc[j];
      const bool elig = k < a.ncand && kb >= 0 && cost < INFINITY;
      const double wk = elig ? fexp(-((cost - cmin) * it)) : 0.0;
      if (__builtin_amdgcn_ballot_w64(wk != 0.0) == 0) continue;  // +0 everywhere: no bit changes (wave-uniform)
      s0 = s0 + wk;
      sq = sq + wk * wk;
      const double* const qk = a.q + k * NP;  // wave-uniform
      double d[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) d[i] = elig ? qk[i] - qb[i] : 0.0;  // (an ineligible lane: no sum sees this candidate's q)
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const double t = wk * d[i];
        s1[i] = s1[i] + t;
#pragma unroll
        for (int l = 0; l <= i; ++l) s2[i * (i + 1) / 2 + l] = s2[i * (i + 1) / 2 + l] + t * d[l];
      }
    }
  }
  // the four strands in the order 0, 1, 2, 3 through LDS; the last one writes the part
  double* const out = a.part + ((tile * a.ksplit + split) * NA) * LUT_COLS + lane;
  __syncthreads();  // the staged rows are consumed
  for (int s = 0; s < LUT_WAVES; ++s) {
    if (w == s) {
      double* const l = lds + lane;
      if (s > 0) {
        s0 = l[0] + s0, sq = l[LUT_COLS] + sq;
#pragma unroll
        for (int i = 0; i < NP; ++i) s1[i] = l[(2 + i) * LUT_COLS] + s1[i];
#pragma unroll
        for (int i = 0; i < NTRI; ++i) s2[i] = l[(2 + NP + i) * LUT_COLS] + s2[i];
      }
      double* const dst = s == LUT_WAVES - 1 ? out : l;
      dst[0] = s0, dst[LUT_COLS] = sq;
#pragma unroll
      for (int i = 0; i < NP; ++i) dst[(2 + i) * LUT_COLS] = s1[i];
#pragma unroll
      for (int i = 0; i < NTRI; ++i) dst[(2 + NP + i) * LUT_COLS] = s2[i];
    }
    __syncthreads();
  }
}

template <int NP>
__global__ __launch_bounds__(LUT_COLS) void k_lut_moments_finish(FinishArgs a) {
  constexpr int NA = nacc(NP), NTRI = NP * (NP + 1) / 2;
  const long long tile = (long long)blockIdx.z * LUT_GRID_X + blockIdx.x, c = tile * LUT_COLS + threadIdx.x;
  if (c >= a.ncol) return;
  const int kb = a.index[c];
  if (kb < 0 || !good_temperature(a.temperature_col ? a.temperature_col[c] : a.temperature)) {
    a.index[c] = -1, a.cost[c] = INFINITY, a.wsum[c] = 0.0, a.ess[c] = 0.0;  // mean and cov keep their bits
    return;
  }
  const double* part = a.part + (tile * a.ksplit * NA) * LUT_COLS + threadIdx.x;
  double s[NA];
#pragma unroll
  for (int e = 0; e < NA; ++e) s[e] = part[e * LUT_COLS];
  for (int p = 1; p < a.ksplit; ++p) {
    part += NA * LUT_COLS;
#pragma unroll
    for (int e = 0; e < NA; ++e) s[e] = s[e] + part[e * LUT_COLS];
  }
  const double s0 = s[0];
  double m[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    m[i] = s[2 + i] / s0;
    a.mean[c * NP + i] = a.q[(long long)kb * NP + i] + m[i];
  }
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int l = 0; l <= i; ++l) {
      const double v = s[2 + NP + i * (i + 1) / 2 + l] / s0 - m[i] * m[l];
      a.cov[(c * NP + i) * NP + l] = v, a.cov[(c * NP + l) * NP + i] = v;
    }
  static_assert(NTRI == NA - 2 - NP, "S2 is the rest of the entries");
  a.ess[c] = (s0 * s0) / s[1];
  a.wsum[c] = s0;
}

long long ngroups(int ncand) { return ((long long)ncand + LUT_SUPER - 1) / LUT_SUPER; }
long long ntiles(int ncol) { return ((long long)ncol + LUT_COLS - 1) / LUT_COLS; }

// The parts of a call.  0: the automatic choice of the match (enough workgroups for the device when there are few columns); an explicit
// value is honoured.  Never more than there are groups of 64 candidates, nor than CRT_LUT_MAX_KSPLIT.
int effective_ksplit(int ncol, int ncand, int ksplit) {
  long long ks = ksplit > 0 ? ksplit : (LUT_TARGET_WG + ntiles(ncol) - 1) / ntiles(ncol);
  if (ks > ngroups(ncand)) ks = ngroups(ncand);
  if (ks > CRT_LUT_MAX_KSPLIT) ks = CRT_LUT_MAX_KSPLIT;
  return ks < 1 ? 1 : (int)ks;
}

size_t match_bytes(int ncol, int ncand) { return (crt_hip_lut_match_workspace_bytes(ncol, ncand, 1) + 255) & ~(size_t)255; }

template <int NP>
int launch_moments(const MomentArgs& a, const FinishArgs& f, hipStream_t s) {
  const long long ntile = ntiles(a.ncol);
  const unsigned gx = (unsigned)(ntile < LUT_GRID_X ? ntile : LUT_GRID_X), gz = (unsigned)((ntile + LUT_GRID_X - 1) / LUT_GRID_X);
  const int st = launch_kernel(k_lut_moments<NP>, dim3(gx, (unsigned)a.ksplit, gz), LUT_THREADS, 0, s, a);
  if (st != CRT_OK) return st;
  return launch_kernel(k_lut_moments_finish<NP>, dim3(gx, 1, gz), LUT_COLS, 0, s, f);
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

size_t crt_hip_lut_posterior_workspace_bytes(int32_t ncol, int32_t ncand, int32_t npar, int32_t ksplit) {
  if (ncol < 1 || ncand < 1 || npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR || ksplit < 0) return 0;
  return match_bytes(ncol, ncand) + (size_t)ntiles(ncol) * effective_ksplit(ncol, ncand, ksplit) * nacc(npar) * LUT_COLS * sizeof(double);
}

int crt_hip_lut_posterior_f64(const crt_lut_table* table, const crt_lut_obs* obs, const crt_lut_posterior_out* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream) {
  if (!table || !obs || !out) return CRT_ERR_BAD_ARG;
  if (table->ncand < 1 || obs->ncol < 1 || table->npar < 1 || table->npar > CRT_RETRIEVE_MAX_NPAR) return CRT_ERR_BAD_ARG;
  if (table->nblk < 1 || table->nblk > CRT_LM_MAX_BLOCKS || !table->q) return CRT_ERR_BAD_ARG;
  if (!(out->temperature > 0.0 && out->temperature < INFINITY) || out->ksplit < 0) return CRT_ERR_BAD_ARG;
  if (!out->index || !out->cost || !out->mean || !out->cov || !out->wsum || !out->ess) return CRT_ERR_BAD_ARG;
  if (!obs->prior != !obs->inv_sigma_prior) return CRT_ERR_BAD_ARG;
  MomentArgs a = {};
  long long nchunk = 0;
  for (int b = 0; b < table->nblk; ++b) {
    if (table->nrow[b] < 1 || !table->m[b] || !obs->y[b]) return CRT_ERR_BAD_ARG;
    a.blk[b] = PostBlk{table->m[b], obs->y[b], obs->inv_sigma[b], table->nrow[b]};
    nchunk += ((long long)table->nrow[b] + LUT_RC - 1) / LUT_RC;
  }
  a.nblk = table->nblk;
  if (obs->prior) {
    a.blk[a.nblk++] = PostBlk{table->q, obs->prior, obs->inv_sigma_prior, table->npar};
    nchunk += 1;
  }
  const size_t need = crt_hip_lut_posterior_workspace_bytes(obs->ncol, table->ncand, table->npar, out->ksplit);
  if (!workspace || workspace_bytes < need) return CRT_ERR_WORKSPACE;
  // pass 1: the best candidate and its cost, by the match itself (its result does not depend on its own K-split)
  const size_t mbytes = match_bytes(obs->ncol, table->ncand);
  const crt_lut_out best = {1, 0, out->index, out->cost, nullptr};
  int st = crt_hip_lut_match_f64(table, obs, &best, workspace, mbytes, stream);
  if (st != CRT_OK) return st;
  a.ncol = obs->ncol, a.ncand = table->ncand;
  a.ksplit = effective_ksplit(a.ncol, a.ncand, out->ksplit);
  a.once = nchunk == 1;  // the columns' rows fit the LDS: staged once per workgroup, not once per 64 candidates
  a.q = table->q, a.index = out->index, a.cost = out->cost;
  a.temperature = out->temperature, a.temperature_col = out->temperature_col;
  a.part = reinterpret_cast<double*>(static_cast<char*>(workspace) + mbytes);
  const FinishArgs f = {a.ncol, a.ksplit, a.q, a.part, a.temperature, a.temperature_col, out->index, out->cost, out->mean, out->cov,
                        out->wsum, out->ess};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (table->npar) {
    case 1: st = launch_moments<1>(a, f, s); break;
    case 2: st = launch_moments<2>(a, f, s); break;
    case 3: st = launch_moments<3>(a, f, s); break;
    case 4: st = launch_moments<4>(a, f, s); break;
    case 5: st = launch_moments<5>(a, f, s); break;
    case 6: st = launch_moments<6>(a, f, s); break;
    case 7: st = launch_moments<7>(a, f, s); break;
    case 8: st = launch_moments<8>(a, f, s); break;
    case 9: st = launch_moments<9>(a, f, s); break;
    default: st = launch_moments<10>(a, f, s); break;
  }
  static_assert(CRT_RETRIEVE_MAX_NPAR == 10, "one instantiation per npar");
  if (st == CRT_OK) note_kernel("k_lut_moments np=%d ksplit=%d nblk=%d once=%d", table->npar, a.ksplit, a.nblk, a.once);
  return st;
}

}  // extern "C"
