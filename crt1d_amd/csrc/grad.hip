// Gradient of a weighted sum of the level spectra (include/crt1d_hip_grad.h): the optics Jacobian (jac.hip), the LAI derivative
// (dlai.hip) and the leaf-angle derivative (dleaf.hip) contracted with the weights w.X[c][r][b] = d loss / d X[c][levels[r]][b] where
// they are formed, for the closed forms 2s, bl, g77, bf.  Reverse mode by forward passes: the parameters are few (three per band, two
// per column), so the adjoint is at most five forward-mode passes whose tangents are multiplied by the weights and added instead of
// stored -- eleven derivative arrays and the contraction that reads them back are never written.
//
//  k_grad         k_jac's mapping without the parameter axis: lane <-> band, a workgroup owns one column and one band slice; the header
//                 with its leaf-angle tangents and the selected record entries are staged in LDS once.  A lane loads its band once and runs
//                 the passes one after the other, ONE tangent at a time (jac.hip: three at once would triple the ~40 live doubles of the 2s
//                 constants), each the pass of deriv_passes.hpp that the kernel it replaces calls -- one piece of code, so the same
//                 tangent bits (-ffp-contract=off):
//                   p = 0, 1, 2   pass_optics<Sch::J>        seed 1 in leaf_r, leaf_t, soil_r      (k_jac)
//                   LAI           pass_record<Sch::D>        L_j' = L_j, LT' = LT                  (k_dlai; bl: + I_df0 L_j tau_d'(L_j))
//                   leaf angle    pass_record<Sch::F, LEAF>  the header tangents of k_dleaf_side   (k_dleaf; bl: + I_df0 tau_d^th(L_j))
//                 A pass whose output is NULL is skipped.  Within a pass the lane adds w.X * X' in the order (level, quantity), quantities
//                 whose weight is NULL left out.  Optics: a plain store of consecutive bands.  LAI, leaf angle: the lanes' sums are added
//                 over the wave by a butterfly (every lane ends with the same bits), over the waves in ascending order by thread 0.
//  k_grad_finish  several band slices: a thread per column adds the slice sums in ascending order.
// No atomics anywhere: a column's result does not depend on the batch, and an output's bits do not depend on which others are asked for.
#include "deriv_passes.hpp"
#include "launch_forms.hpp"

namespace crt {
namespace {

struct G2s : Sch2s {};
struct GBl : SchBl {};
template <bool BF>
struct GG77 : SchG77<BF> {};

// acc += sum_X w.X[o] X' for the tangents of one row: dI = I_dr', dn = I_df_d', up = I_df_u', dF = F'.  UP: the scheme has an upward stream
// (bl: w.I_df_u is not read)
template <bool UP>
__device__ __forceinline__ void grad_add(double& acc, const GradArgs& ga, long long o, bool with_dr, double dI, double dn, double up, double dF) {
  if (with_dr && ga.w[0]) acc += ga.w[0][o] * dI;
  if (ga.w[1]) acc += ga.w[1][o] * dn;
  if (UP && ga.w[2]) acc += ga.w[2][o] * up;
  if (ga.w[3]) acc += ga.w[3][o] * dF;
}

// the sum of v over the workgroup in a fixed order, valid in thread 0 (every thread calls): butterfly over the wave, then wave 0, 1, ...
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  __syncthreads();  // (red is used again)
  return s;
}

template <class G, bool BL>
__global__ __launch_bounds__(GRAD_BLOCK) void k_grad(SolveArgs a, LevArgs la, GradArgs ga, int per) {
  using SJ = typename G::J;
  __shared__ double hd[HDR_TAN + REC_HDR];  // k_dleaf's layout: header | e^{-K_b LT} at the ground | ... | the header's leaf-angle tangents
  __shared__ double lvL[CRT_MAX_LEVEL_SELECT], lvE[CRT_MAX_LEVEL_SELECT], lvTs[CRT_MAX_LEVEL_SELECT], lvTh[CRT_MAX_LEVEL_SELECT];
  __shared__ double red[GRAD_BLOCK / 64];
  const int c = blockIdx.x, nz = a.nz, nb = a.nb, nsel = la.nsel, tid = threadIdx.x;
  const int b = blockIdx.y * per + tid;
  const bool live = tid < per && b < nb;
  // its own staging, the tangents of both record derivatives at once: through a shared function k_grad<bl> took 8 more SGPRs
  const double* rec = a.ws + (long long)c * a.reclen;
  const double* sdl = ga.side_leaf + (long long)c * (REC_HDR + (BL ? nz : 0));
  if (tid < REC_HDR) {
    hd[tid] = rec[tid];
    hd[HDR_TAN + tid] = ga.leaf ? sdl[tid] : 0.0;
  }
  if (tid == REC_HDR) hd[REC_HDR] = rec[REC_HDR + nz];  // e^{-K_b L} at the ground
  for (int r = tid; r < nsel; r += blockDim.x) {
    const int j = la.lev[r];
    lvL[r] = rec[REC_HDR + j];
    lvE[r] = rec[REC_HDR + nz + j];
    if constexpr (BL) {
      lvTs[r] = ga.lai ? ga.side_lai[(long long)c * nz + j] : 0.0;  // L_j tau_d'(L_j)
      lvTh[r] = ga.leaf ? sdl[REC_HDR + j] : 0.0;                   // tau_d^th(L_j)
    }
  }
  __syncthreads();
  const double invmu = hd[S_INVMU];
  const long long o0 = (long long)c * nsel * nb + b;  // row r of the weights: + r nb
  DBand in = {};
  if (live) in = load_dband(a, c, b, SJ::SOIL);

  // ---- the optics, one parameter at a time (k_jac) ----
  if (live) {
    for (int p = 0; p < CRT_JAC_NPARAM; ++p) {
      if (!ga.o[p]) continue;
      double acc = 0.0;
      if (SJ::SOIL || p != 2)  // (bl has no soil: zeros)
        pass_optics<SJ>(hd, lvL, lvE, nsel, seed_band(in, p), [&](int r, Du dn, Du up) {
          grad_add<SJ::SOIL>(acc, ga, o0 + (long long)r * nb, false, 0.0, dn.d, up.d, 2 * (up.d + dn.d));  // F' as jac_store
        });
      ga.o[p][(long long)c * nb + b] = acc;
    }
  }
  const int nslice = gridDim.y;
  double* const dst = nslice == 1 ? nullptr : ga.part + ((long long)c * nslice + blockIdx.y) * 2;

  // ---- the LAI (k_dlai) ----
  if (ga.lai) {
    double acc = 0.0;
    if (live)
      pass_record<typename G::D, BL, false>(hd, lvL, lvE, lvTs, nsel, in, [&](int r, double dI, Du dn, Du up) {
        grad_add<SJ::SOIL>(acc, ga, o0 + (long long)r * nb, true, dI, dn.d, up.d, flux_tan(dI, invmu, dn, up));
      });
    const double s = block_sum(acc, red);
    if (tid == 0) (dst ? dst[0] : ga.lai[c]) = s;
  }

  // ---- the leaf angles (k_dleaf) ----
  if (ga.leaf) {
    double acc = 0.0;
    if (live)
      pass_record<typename G::F, BL, true>(hd, lvL, lvE, lvTh, nsel, in, [&](int r, double dI, Du dn, Du up) {
        grad_add<SJ::SOIL>(acc, ga, o0 + (long long)r * nb, true, dI, dn.d, up.d, flux_tan(dI, invmu, dn, up));
      });
    const double s = block_sum(acc, red);
    if (tid == 0) (dst ? dst[1] : ga.leaf[c]) = s;
  }
}

__global__ __launch_bounds__(256) void k_grad_finish(int ncol, int nslice, const double* __restrict__ part, double* __restrict__ lai,
                                                      double* __restrict__ leaf) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double* p = part + (long long)c * nslice * 2;
  if (lai) {
    double s = p[0];
    for (int i = 1; i < nslice; ++i) s += p[2 * i];
    lai[c] = s;
  }
  if (leaf) {
    double s = p[1];
    for (int i = 1; i < nslice; ++i) s += p[2 * i + 1];
    leaf[c] = s;
  }
}

template <class G, bool BL = false>
int launch_grad_closed(const SolveArgs& a, const LevArgs& la, const GradArgs& ga, hipStream_t s, bool probe) {
  const LevSlices ls = lev_slices(a.nb, GRAD_BLOCK);
  if (ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  int st = launch_kernel(k_grad<G, BL>, dim3(a.ncol, ls.nslice), ls.nthr, 0, s, a, la, ga, ls.per);
  const bool fin = ls.nslice > 1 && (ga.lai || ga.leaf);
  if (st == CRT_OK && fin) st = launch_kernel(k_grad_finish, dim3((a.ncol + 255) / 256), 256, 0, s, a.ncol, ls.nslice, ga.part, ga.lai, ga.leaf);
  if (st == CRT_OK) note_kernel("k_grad<%s> nsel=%d slice=%d%s", G::J::NAME, la.nsel, ls.per, fin ? " + k_grad_finish" : "");
  return st;
}

}  // namespace

int launch_grad(int scheme, const SolveArgs& a, const LevArgs& la, const GradArgs& ga, hipStream_t s, bool probe) {
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_grad_closed<G2s>(a, la, ga, s, probe);
    case CRT_SCHEME_BL: return launch_grad_closed<GBl, true>(a, la, ga, s, probe);
    case CRT_SCHEME_G77: return launch_grad_closed<GG77<false>>(a, la, ga, s, probe);
    case CRT_SCHEME_BF: return launch_grad_closed<GG77<true>>(a, la, ga, s, probe);
    default: return CRT_ERR_UNSUPPORTED;
  }
}

}  // namespace crt
