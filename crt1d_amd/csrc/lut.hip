// The look-up-table start of a retrieval (include_lut/crt1d_hip_lut.h): the fused misfit-and-selection kernel, the merge of its partial
// lists and their C entry.
//
//  k_lut_match   lane = column, candidates wave-uniform: a workgroup owns 64 columns and one part of the K-split, takes 64 candidates at
//                a time (16 per wave, one running sum each per lane), streams the rows through LDS CRT_LUT_ROWS at a time and keeps the M
//                best of every column sorted in registers; the four waves' lists are merged through LDS into the workspace
//  k_lut_merge   one lane per column: the partial lists of the K-split merged under the total order (cost, index); writes index, cost, p
//
// Bounds: every global index is (column < ncol) * nrow + (row < nrow) or (candidate < K) * nrow + (row < nrow), in 64 bits; a column or a
// candidate beyond the end is staged as zeros and never selected or written.  The LDS indices are bounded by the constants below.
#include "crt1d_hip_lut.h"
#include "crt_internal.hpp"

namespace crt {
namespace {

constexpr int LUT_COLS = 64;                       // columns of a workgroup: one per lane
constexpr int LUT_WAVES = 4;
constexpr int LUT_TILE = 16;                       // candidates of a wave at a time: 16 running sums, 32 VGPRs
constexpr int LUT_SUPER = LUT_WAVES * LUT_TILE;    // candidates of a workgroup at a time
constexpr int LUT_THREADS = LUT_WAVES * 64;
constexpr int LUT_RC = CRT_LUT_ROWS;               // rows staged at a time
// Row strides of the staged arrays, in doubles.  The staging threads run along the rows of one column (coalesced global loads), so their
// LDS stores are a row stride apart: 64 would put them all into one bank pair (measured: 55 % of the LDS-array cycles were bank
// conflicts); 65 and 66 (a multiple of two keeps the 16-byte broadcast reads aligned) spread them.
constexpr int LUT_YS = LUT_COLS + 1;
constexpr int LUT_TS = LUT_COLS + 2;
constexpr int LUT_TARGET_WG = 1024;                // workgroups wanted on the device: four per CU
constexpr int LUT_MAXBLK = CRT_LM_MAX_BLOCKS + 1;  // the prior rows are one more block: table q, observation prior, weight inv_sigma_prior
constexpr int MERGE_BLOCK = 64;
constexpr long long LUT_GRID_X = 1 << 20;          // workgroups along grid.x; the groups of 64 columns beyond that go along grid.z

struct LutBlk {
  const double *m, *y, *is;
  int nrow;
};

struct LutArgs {
  LutBlk blk[LUT_MAXBLK];
  int nblk, ncol, ncand, ksplit, once;
  double* wcost;  // [ncol][ksplit][MB]
  int* widx;
};

struct MergeArgs {
  int ncol, ksplit, nbest, npar;
  const double* wcost;
  const int* widx;
  const double* q;
  int* index;
  double *cost, *p;
};

__device__ inline bool before(double ca, int ia, double cb, int ib) { return ca < cb || (ca == cb && ia < ib); }

// The MB best (cost, index) of one column, sorted, in registers.  An empty slot is (+inf, -1).
template <int MB>
struct Best {
  double c[MB];
  int i[MB];
  __device__ inline void init() {
#pragma unroll
    for (int j = 0; j < MB; ++j) c[j] = INFINITY, i[j] = -1;
  }
  // Candidates that arrive in ascending index: strict <, so an equal cost stays behind those already there.  (cost < c[MB-1] <= +inf: an
  // ineligible candidate never enters.)
  __device__ inline void push(double cost, int idx) {
    if (!(cost < c[MB - 1])) return;
#pragma unroll
    for (int j = MB - 1; j >= 0; --j) {
      if (j > 0 && cost < c[j - 1]) c[j] = c[j - 1], i[j] = i[j - 1];
      else if (cost < c[j]) c[j] = cost, i[j] = idx;
    }
  }
  // Entries in any order, under the total order (cost, index).  idx >= 0 and cost < +inf.
  __device__ inline void push_ordered(double cost, int idx) {
    if (!before(cost, idx, c[MB - 1], i[MB - 1])) return;
#pragma unroll
    for (int j = MB - 1; j >= 0; --j) {
      if (j > 0 && before(cost, idx, c[j - 1], i[j - 1])) c[j] = c[j - 1], i[j] = i[j - 1];
      else if (before(cost, idx, c[j], i[j])) c[j] = cost, i[j] = idx;
    }
  }
};

template <int MB>
__global__ __launch_bounds__(LUT_THREADS) void k_lut_match(LutArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[LUT_RC * (2 * LUT_YS + LUT_TS)];  // 24.5 KiB
  double* const tb = lds;                        // [row][candidate of the 64], rows LUT_TS apart
  double* const ys = tb + LUT_RC * LUT_TS;       // [row][column], rows LUT_YS apart: y, 0 where masked
  double* const ss = ys + LUT_RC * LUT_YS;       // inv_sigma, 0 where masked
  static_assert(LUT_RC * (2 * LUT_YS + LUT_TS) >= LUT_WAVES * CRT_LUT_MAX_BEST * LUT_COLS * 3 / 2, "the lists of the four waves fit");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long c0 = ((long long)blockIdx.z * LUT_GRID_X + blockIdx.x) * LUT_COLS;
  if (c0 >= a.ncol) return;  // (the whole workgroup, before any barrier: the last slice of grid.z is not full)
  const int split = blockIdx.y;
  const long long nsuper = ((long long)a.ncand + LUT_SUPER - 1) / LUT_SUPER;
  const long long st0 = split * nsuper / a.ksplit, st1 = (split + 1) * nsuper / a.ksplit;
  Best<MB> best;
  best.init();
  for (long long st = st0; st < st1; ++st) {
    const long long kbase = st * LUT_SUPER;
    double acc[LUT_TILE];
#pragma unroll
    for (int j = 0; j < LUT_TILE; ++j) acc[j] = 0.0;
    for (int q = 0; q < a.nblk; ++q) {
      const LutBlk B = a.blk[q];
      for (int o0 = 0; o0 < B.nrow; o0 += LUT_RC) {
        const int n = min(LUT_RC, B.nrow - o0);
        __syncthreads();  // the previous rows are consumed
        if (!a.once || st == st0) {
          for (int idx = tid; idx < LUT_COLS * n; idx += LUT_THREADS) {
            const int cl = idx / n, o = idx - cl * n;
            const long long c = c0 + cl;
            double s = 0.0, y = 0.0;
            if (c < a.ncol) {
              const long long g = c * B.nrow + o0 + o;
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
        // A masked row is staged as y = 0, inv_sigma = 0: r = (m - 0) * 0 is +-0 for a finite table entry and r * r is +0; a running sum
        // that started at +0 is never -0, so adding it changes no bit, and the loop has no branch.  A table entry that is not finite gives
        // NaN there as on a row that counts: such a candidate is eligible for no column.
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
#pragma unroll
    for (int j = 0; j < LUT_TILE; ++j) {
      const long long k = kbase + w * LUT_TILE + j;
      if (k < a.ncand) best.push(0.5 * acc[j], (int)k);
    }
  }
  // the four waves' lists -> one, under the total order (a wave's candidates are not all below the next wave's)
  double* const lc = lds;
  int* const li = reinterpret_cast<int*>(lds + LUT_WAVES * MB * LUT_COLS);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < MB; ++j) lc[(w * MB + j) * LUT_COLS + lane] = best.c[j], li[(w * MB + j) * LUT_COLS + lane] = best.i[j];
  __syncthreads();
  const long long c = c0 + lane;
  if (w == 0 && c < a.ncol) {
    Best<MB> tot;
    tot.init();
    for (int e = 0; e < LUT_WAVES * MB; ++e) {
      const int ie = li[e * LUT_COLS + lane];
      if (ie >= 0) tot.push_ordered(lc[e * LUT_COLS + lane], ie);
    }
    const long long base = (c * a.ksplit + split) * MB;
#pragma unroll
    for (int j = 0; j < MB; ++j) a.wcost[base + j] = tot.c[j], a.widx[base + j] = tot.i[j];
  }
}

template <int MB>
__global__ __launch_bounds__(MERGE_BLOCK) void k_lut_merge(MergeArgs a) {
  const long long c = ((long long)blockIdx.z * LUT_GRID_X + blockIdx.x) * MERGE_BLOCK + threadIdx.x;
  if (c >= a.ncol) return;
  Best<MB> tot;
  tot.init();
  const long long base = c * a.ksplit * MB;
  for (long long e = 0; e < (long long)a.ksplit * MB; ++e) {
    const int ie = a.widx[base + e];
    if (ie >= 0) tot.push_ordered(a.wcost[base + e], ie);
  }
#pragma unroll
  for (int j = 0; j < MB; ++j)
    if (j < a.nbest) a.index[c * a.nbest + j] = tot.i[j], a.cost[c * a.nbest + j] = tot.c[j];
  if (a.p && tot.i[0] >= 0)
    for (int k = 0; k < a.npar; ++k) a.p[c * a.npar + k] = a.q[(long long)tot.i[0] * a.npar + k];
}

// the list length the kernels are instantiated for
int list_len(int nbest) { return nbest <= 1 ? 1 : nbest <= 4 ? 4 : 8; }

// The K-split: enough workgroups for the device when there are few columns, never more than there are groups of 64 candidates.
int auto_ksplit(int ncol, int ncand) {
  const long long ntile = ((long long)ncol + LUT_COLS - 1) / LUT_COLS, nsuper = ((long long)ncand + LUT_SUPER - 1) / LUT_SUPER;
  long long ks = (LUT_TARGET_WG + ntile - 1) / ntile;
  if (ks > nsuper) ks = nsuper;
  if (ks > CRT_LUT_MAX_KSPLIT) ks = CRT_LUT_MAX_KSPLIT;
  return ks < 1 ? 1 : (int)ks;
}

size_t part_cost_bytes(int ncol, int ks, int mb) { return (((size_t)ncol * ks * mb * sizeof(double)) + 255) & ~(size_t)255; }

template <int MB>
int launch_lut(const LutArgs& a, const MergeArgs& g, hipStream_t s) {
  // groups of 64 columns on (grid.x, grid.z): any int32 ncol stays inside the limits of a grid (2^31 / 64 groups = 32 slices of 2^20)
  const long long ntile = ((long long)a.ncol + LUT_COLS - 1) / LUT_COLS;
  const unsigned gx = (unsigned)(ntile < LUT_GRID_X ? ntile : LUT_GRID_X), gz = (unsigned)((ntile + LUT_GRID_X - 1) / LUT_GRID_X);
  int st = launch_kernel(k_lut_match<MB>, dim3(gx, (unsigned)a.ksplit, gz), LUT_THREADS, 0, s, a);
  if (st != CRT_OK) return st;
  static_assert(MERGE_BLOCK == LUT_COLS, "the merge kernel runs on the same groups of columns");
  return launch_kernel(k_lut_merge<MB>, dim3(gx, 1, gz), MERGE_BLOCK, 0, s, g);
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

size_t crt_hip_lut_match_workspace_bytes(int32_t ncol, int32_t ncand, int32_t nbest) {
  if (ncol < 1 || ncand < 1 || nbest < 1 || nbest > CRT_LUT_MAX_BEST) return 0;
  const int ks = auto_ksplit(ncol, ncand), mb = list_len(nbest);
  return part_cost_bytes(ncol, ks, mb) + (size_t)ncol * ks * mb * sizeof(int32_t);
}

int crt_hip_lut_match_f64(const crt_lut_table* table, const crt_lut_obs* obs, const crt_lut_out* out, void* workspace,
                          size_t workspace_bytes, crt_stream_t stream) {
  if (!table || !obs || !out) return CRT_ERR_BAD_ARG;
  if (table->ncand < 1 || obs->ncol < 1 || table->npar < 1 || table->npar > CRT_RETRIEVE_MAX_NPAR) return CRT_ERR_BAD_ARG;
  if (table->nblk < 1 || table->nblk > CRT_LM_MAX_BLOCKS || !table->q) return CRT_ERR_BAD_ARG;
  if (out->nbest < 1 || out->nbest > CRT_LUT_MAX_BEST || out->ksplit < 0 || !out->index || !out->cost) return CRT_ERR_BAD_ARG;
  if (!obs->prior != !obs->inv_sigma_prior) return CRT_ERR_BAD_ARG;
  LutArgs a = {};
  long long nchunk = 0;
  for (int b = 0; b < table->nblk; ++b) {
    if (table->nrow[b] < 1 || !table->m[b] || !obs->y[b]) return CRT_ERR_BAD_ARG;
    a.blk[b] = LutBlk{table->m[b], obs->y[b], obs->inv_sigma[b], table->nrow[b]};
    nchunk += ((long long)table->nrow[b] + LUT_RC - 1) / LUT_RC;
  }
  a.nblk = table->nblk;
  if (obs->prior) {
    a.blk[a.nblk++] = LutBlk{table->q, obs->prior, obs->inv_sigma_prior, table->npar};
    nchunk += 1;
  }
  const size_t need = crt_hip_lut_match_workspace_bytes(obs->ncol, table->ncand, out->nbest);
  if (!workspace || workspace_bytes < need) return CRT_ERR_WORKSPACE;
  const int cap = auto_ksplit(obs->ncol, table->ncand), mb = list_len(out->nbest);
  a.ncol = obs->ncol, a.ncand = table->ncand;
  a.ksplit = out->ksplit == 0 || out->ksplit > cap ? cap : out->ksplit;
  a.once = nchunk == 1;  // the columns' rows fit the LDS: staged once per workgroup, not once per 64 candidates
  a.wcost = static_cast<double*>(workspace);
  a.widx = reinterpret_cast<int*>(static_cast<char*>(workspace) + part_cost_bytes(a.ncol, a.ksplit, mb));
  MergeArgs g = {a.ncol, a.ksplit, out->nbest, table->npar, a.wcost, a.widx, table->q, out->index, out->cost, out->p};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int st = mb == 1 ? launch_lut<1>(a, g, s) : mb == 4 ? launch_lut<4>(a, g, s) : launch_lut<8>(a, g, s);
  if (st == CRT_OK) note_kernel("k_lut_match mb=%d ksplit=%d nblk=%d once=%d", mb, a.ksplit, a.nblk, a.once);
  return st;
}

}  // extern "C"
