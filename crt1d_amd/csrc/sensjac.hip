// Jacobian of the sensor-band sums (include/crt1d_hip_sensjac.h): the optics Jacobian (jac.hip) along ntan directions, the LAI derivative
// (dlai.hip) and the leaf-angle derivative (dleaf.hip) folded with the spectral responses of a sensor set where they are formed, for the
// closed forms 2s, bl, g77, bf.  Only [ncol][nsel][nsens][npar] sums leave the workgroup: the eleven derivative arrays of the composition,
// the (ncol, nsel, ntan, nb) intermediate and the dense weights are never written or read.
//
//  k_sens_jac         k_grad's mapping: lane <-> band, a workgroup owns one column and one band slice; the header with its leaf-angle
//                     tangents and the selected record entries are staged in LDS once, a lane loads its band once and runs the passes one
//                     after the other, ONE tangent at a time (grad.hip), each with the jac_schemes.hpp instantiation k_grad uses -- the same
//                     tangent bits (-ffp-contract=off).  Where k_grad multiplies a tangent by a weight and adds, a lane here leaves the
//                     tangent in its entry of the staging rows [nsel][R][lanes] in LDS; three phases share the rows:
//                       directions   rows (k, q), q = I_df_d, I_df_u, F: the unit-seed passes p = leaf_r, leaf_t, soil_r add X'_p d_p[k][b]
//                                    in this order (a NULL direction array and bl's soil are left out) -- a lane touches its own entries
//                                    only, so the three passes need no barrier
//                       LAI          rows q = I_dr, I_df_d, I_df_u, F
//                       leaf angle   the same
//                     and each phase ends with ONE barrier and sens_fold_rows (crt_internal.hpp): a wave per (level, sensor band,
//                     parameter) over the support inside the slice, sens_row's order.  R = max(3 ntan, 4).
//  k_sens_jac_series  the same body (sens_jac_body) for the sun states of a series (include/crt1d_hip_sensjac_series.h): a workgroup owns one
//                     (column, band slice, sun state) on the grid of lev_series_grid; the header, the selected entries of L_j and
//                     e^{-K_b L_j} and the ground entry are read straight from the canopy record of the column and the sun record of
//                     (column, t) -- the record is not assembled, the static LDS is that of k_sens_jac -- and K_b' of the leaf-angle pass
//                     is formed here, dG(psi_t) / cos psi_t, the side record being the sun-independent one of k_dleaf_side<canopy>.
//                     Same slices, lanes and R as k_sens_jac (sensjac_slices): slice [:, t] of the output has the per-step bits.
//  k_sens_jac_finish  several band slices: a thread per output element adds the slice sums in ascending order (k_sens_finish's rule);
//                     the series: ncol * nt "columns" v = c * nt + t.
// No atomics anywhere: a column's result does not depend on the batch, and an output's bits do not depend on which others are asked for
// (every quantity is staged and folded; a NULL output is only not written).
#include "deriv_passes.hpp"
#include "launch_forms.hpp"

namespace crt {
namespace {

struct S2s : Sch2s {};
struct SBl : SchBl {};
template <bool BF>
struct SG77 : SchG77<BF> {};

// Where the body below finds the band-independent entries of its (column, sun state): the header scalar i, the LAI L_j and the beam
// fraction e^{-K_b L_j} of level j (j = 0: the ground), and the tangent of header scalar i along the leaf-angle direction.
struct RecStep {  // the record k_colpre wrote; sdl: the side record of k_dleaf_side
  const double* rec;
  int nz;
  __device__ __forceinline__ double hdr(int i) const { return rec[i]; }
  __device__ __forceinline__ double L(int j) const { return rec[REC_HDR + j]; }
  __device__ __forceinline__ double E(int j) const { return rec[REC_HDR + nz + j]; }
  __device__ __forceinline__ double dhdr(const double* sdl, int i) const { return sdl[i]; }
};
// The canopy record of the column and the sun record of (column, t) (SeriesArgs, crt_internal.hpp), each entry read where it lies -- the
// record is not assembled.  sdl: the side record of k_dleaf_side<canopy>, which leaves out the one tangent that follows the sun:
// K_b' = dG(psi_t) / cos psi_t, the division k_dleaf_side does.
struct RecSeries {
  const double *can, *sun;
  const double* dgp;  // dG at psi of (column, t); read with a leaf-angle column only
  int scheme, nz;
  __device__ __forceinline__ double hdr(int i) const {
    int si = -1;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (sun_hdr_slot(k) == i) si = k;
    return si >= 0 ? sun[si] : can[i];
  }
  __device__ __forceinline__ double vec(int vc, int j) const {
    const int sv = rec_vec_sun(scheme, vc);
    return sv >= 0 ? sun[SUN_HDR + sv * nz + j] : can[REC_HDR + vc * nz + j];
  }
  __device__ __forceinline__ double L(int j) const { return vec(0, j); }
  __device__ __forceinline__ double E(int j) const { return vec(1, j); }
  __device__ __forceinline__ double dhdr(const double* sdl, int i) const { return i == S_KB ? *dgp / hdr(S_MU) : sdl[i]; }
};

// The work of one workgroup: column c, band slice `slice` of nslice, sums indexed by v (the column; series: c * nt + t).  `a` carries the
// spectra of v at the column's index.
template <class G, bool BL, class Rec>
__device__ __forceinline__ void sens_jac_body(const SolveArgs& a, const LevArgs& la, const SensJacArgs& ja, int per, int R, int c, int slice,
                                              int nslice, long long v, const Rec rc, double* rows) {
  using SJ = typename G::J;
  __shared__ double hd[HDR_TAN + REC_HDR];  // k_dleaf's layout: header | e^{-K_b LT} at the ground | ... | the header's leaf-angle tangents
  __shared__ double lvL[CRT_MAX_LEVEL_SELECT], lvE[CRT_MAX_LEVEL_SELECT], lvTs[CRT_MAX_LEVEL_SELECT], lvTh[CRT_MAX_LEVEL_SELECT];
  const int nz = a.nz, nb = a.nb, nsel = la.nsel, tid = threadIdx.x, nthr = blockDim.x;
  const int b = slice * per + tid;
  const bool live = tid < per && b < nb;
  const int ntan = ja.ntan, npar = ntan + ja.lai + ja.leaf;
  // (staging and pass loops are this body's own, not those of deriv_passes.hpp: DESIGN 3.20)
  const double* sdl = ja.side_leaf + (long long)c * (REC_HDR + (BL ? nz : 0));
  if (tid < REC_HDR) {
    hd[tid] = rc.hdr(tid);
    hd[HDR_TAN + tid] = ja.leaf ? rc.dhdr(sdl, tid) : 0.0;
  }
  if (tid == REC_HDR) hd[REC_HDR] = rc.E(0);  // e^{-K_b L} at the ground
  for (int r = tid; r < nsel; r += nthr) {
    const int j = la.lev[r];
    lvL[r] = rc.L(j);
    lvE[r] = rc.E(j);
    if constexpr (BL) {
      lvTs[r] = ja.lai ? ja.side_lai[(long long)c * nz + j] : 0.0;  // L_j tau_d'(L_j)
      lvTh[r] = ja.leaf ? sdl[REC_HDR + j] : 0.0;                   // tau_d^th(L_j)
    }
  }
  __syncthreads();
  const double invmu = hd[S_INVMU];
  DBand in = {};
  if (live) in = load_dband(a, c, b, SJ::SOIL);
  double* const my = rows + tid;  // row i of level r: my[(r R + i) nthr]

  // ---- the directions: the optics one parameter at a time (k_jac), each tangent times the lane's band of every direction ----
  if (ntan > 0) {
    if (live) {
      bool first = true;  // (uniform)
      for (int p = 0; p < CRT_JAC_NPARAM; ++p) {
        if (!ja.d[p] || (!SJ::SOIL && p == 2)) continue;  // (bl has no soil)
        const double* dp = ja.d[p] + (long long)c * ja.dstride + b;
        double d[CRT_SENSJAC_MAX_NTAN];
#pragma unroll
        for (int k = 0; k < CRT_SENSJAC_MAX_NTAN; ++k) d[k] = k < ntan ? dp[(long long)k * nb] : 0.0;
        SJ st;
        st.init(hd, seed_band(in, p), hd[REC_HDR]);
        for (int r = 0; r < nsel; ++r) {
          Du dn, up;
          st.level(lvL[r], lvE[r], dn, up);
          const double x[3] = {dn.d, up.d, 2 * (up.d + dn.d)};  // F' as jac_store
          double* const y = my + (size_t)r * R * nthr;
#pragma unroll
          for (int k = 0; k < CRT_SENSJAC_MAX_NTAN; ++k)
            if (k < ntan) {
#pragma unroll
              for (int q = 0; q < 3; ++q) {
                const double t = x[q] * d[k];
                double* const e = y + (size_t)(3 * k + q) * nthr;
                *e = first ? t : *e + t;
              }
            }
        }
        first = false;
      }
      if (first)  // (bl with directions in soil_r alone: zeros)
        for (int r = 0; r < nsel; ++r)
          for (int i = 0; i < 3 * ntan; ++i) my[((size_t)r * R + i) * nthr] = 0.0;
    }
    __syncthreads();
    sens_fold_rows<3>(ja.sn, rows, R, 0, ntan, 0, npar, slice, per, nb, nslice, v, nsel);
    __syncthreads();
  }

  // ---- the LAI (k_dlai) ----
  if (ja.lai) {
    if (live) {
      const double K = hd[S_KB];
      typename G::D st;
      st.init(hd, in, Du{hd[REC_HDR], -(K * hd[S_LT]) * hd[REC_HDR]});
      for (int r = 0; r < nsel; ++r) {
        const double L = lvL[r];
        const Du eK = Du{lvE[r], -(K * L) * lvE[r]};
        Du dn, up;
        st.level(Du{L, L}, eK, dn, up);
        if constexpr (BL) dn.d += in.I_df0 * lvTs[r];  // the sky term I_df0 tau_d(L_j)
        const double dI = in.I_dr0 * eK.d;
        double* const y = my + (size_t)r * R * nthr;
        y[0] = dI;
        y[nthr] = dn.d;
        y[2 * nthr] = up.d;
        y[3 * nthr] = __builtin_fma(dI, invmu, 2 * (up.d + dn.d));  // F' as dlai_store
      }
    }
    __syncthreads();
    sens_fold_rows<4>(ja.sn, rows, R, 0, 1, ntan, npar, slice, per, nb, nslice, v, nsel);
    __syncthreads();
  }

  // ---- the leaf angles (k_dleaf) ----
  if (ja.leaf) {
    if (live) {
      const double dK = hd[HDR_TAN + S_KB];
      typename G::F st;
      st.init(hd, in, Du{hd[REC_HDR], -(dK * hd[S_LT]) * hd[REC_HDR]});
      for (int r = 0; r < nsel; ++r) {
        const double L = lvL[r];
        const Du eK = Du{lvE[r], -(dK * L) * lvE[r]};
        Du dn, up;
        st.level(L, eK, dn, up);
        if constexpr (BL) dn.d += in.I_df0 * lvTh[r];  // the sky term I_df0 tau_d(L_j)
        const double dI = in.I_dr0 * eK.d;
        double* const y = my + (size_t)r * R * nthr;
        y[0] = dI;
        y[nthr] = dn.d;
        y[2 * nthr] = up.d;
        y[3 * nthr] = __builtin_fma(dI, invmu, 2 * (up.d + dn.d));
      }
    }
    __syncthreads();
    sens_fold_rows<4>(ja.sn, rows, R, 0, 1, ntan + ja.lai, npar, slice, per, nb, nslice, v, nsel);
  }
}

template <class G, bool BL>
__global__ __launch_bounds__(SENSJAC_BLOCK) void k_sens_jac(SolveArgs a, LevArgs la, SensJacArgs ja, int per, int R) {
  extern __shared__ double rows[];  // [nsel][R][blockDim.x]
  const int c = blockIdx.x;
  sens_jac_body<G, BL>(a, la, ja, per, R, c, blockIdx.y, gridDim.y, c, RecStep{a.ws + (long long)c * a.reclen, a.nz}, rows);
}

// The sun-angle series (include/crt1d_hip_sensjac_series.h): one workgroup per (column, band slice, sun state) on the grid of
// lev_series_grid; the spectra of (column, t) as in series_lev_step.  The same body on the same slices: slice [:, t] has the per-step bits.
template <class G, bool BL>
__global__ __launch_bounds__(SENSJAC_BLOCK) void k_sens_jac_series(SolveArgs a, LevArgs la, SensJacArgs ja, SeriesArgs sr,
                                                                   const double* __restrict__ dg_at_psi, int per, int R, int nslice) {
  extern __shared__ double rows[];  // [nsel][R][blockDim.x]
  const int c = blockIdx.x;
  const int zt = blockIdx.z / nslice, slice = blockIdx.z - zt * nslice;
  const long long tl = (long long)zt * gridDim.y + blockIdx.y;
  if (tl >= sr.nt) return;  // (whole workgroup, before any barrier)
  const long long v = (long long)c * sr.nt + tl;
  const long long din = (long long)c * sr.col_stride + tl * a.nb - (long long)c * a.col_stride;
  a.I_dr0 = static_cast<const double*>(sr.I_dr0) + din;
  a.I_df0 = static_cast<const double*>(sr.I_df0) + din;
  const RecSeries rc = {sr.can + (long long)c * sr.canlen, sr.sun + v * sr.sunlen, dg_at_psi + v, sr.scheme, sr.nz};
  sens_jac_body<G, BL>(a, la, ja, per, R, c, slice, nslice, v, rc, rows);
}

// One thread per output element (c, r, s, par, q): the partial sums of the slices that meet the support of sensor band s, added in
// ascending slice order -- the slices sens_fold_rows skipped are skipped here, so nothing unwritten is read.  MASKED: an element of a
// skipped column (v / nt) keeps its bits, and its slice sums are not read.
template <bool MASKED>
__device__ __forceinline__ void sens_jac_finish_body(const SensArgs& sn, long long ncol, int nslice, int per, int nb, int nsel, int npar, ColMask m,
                                                     int nt) {
  const int nsens = sn.nsens;
  const long long n = ncol * nsel * nsens * npar * 4;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int q = (int)(i % 4);
  const int par = (int)((i / 4) % npar);
  const int s = (int)((i / (4LL * npar)) % nsens);
  const int r = (int)((i / (4LL * npar * nsens)) % nsel);
  const long long v = i / (4LL * npar * nsens * nsel);
  if constexpr (MASKED)
    if (col_skipped(m, (int)(v / nt))) return;
  double* const o = sn.o[q];
  if (!o) return;
  const int f = sn.first[s], e = f + sn.count[s];
  double z = 0.0;
  bool any = false;
  for (int sl = 0; sl < nslice; ++sl) {
    const int lo_s = sl * per, hi_s = min(lo_s + per, nb);
    if (max(f, lo_s) >= min(e, hi_s)) continue;
    const double p = sn.part[((((v * nslice + sl) * nsel + r) * nsens + s) * npar + par) * 4 + q];
    z = any ? z + p : p;
    any = true;
  }
  o[((v * nsel + r) * nsens + s) * npar + par] = z;
}

__global__ __launch_bounds__(256) void k_sens_jac_finish(SensArgs sn, long long ncol, int nslice, int per, int nb, int nsel, int npar) {
  sens_jac_finish_body<false>(sn, ncol, nslice, per, nb, nsel, npar, ColMask{}, 1);
}

// ---- the masked forms (include_mask/crt1d_hip_masked.h): every workgroup of a skipped column returns before it reads anything of the
// column and before any barrier (the test is workgroup-uniform: the column is blockIdx.x on both grids); an evaluated column runs the body
// of its plain sibling, so its bits are the sibling's.
template <class G, bool BL>
__global__ __launch_bounds__(SENSJAC_BLOCK) void k_sens_jac_masked(SolveArgs a, LevArgs la, SensJacArgs ja, int per, int R, ColMask m) {
  extern __shared__ double rows[];  // [nsel][R][blockDim.x]
  const int c = blockIdx.x;
  if (col_skipped(m, c)) return;
  sens_jac_body<G, BL>(a, la, ja, per, R, c, blockIdx.y, gridDim.y, c, RecStep{a.ws + (long long)c * a.reclen, a.nz}, rows);
}

template <class G, bool BL>
__global__ __launch_bounds__(SENSJAC_BLOCK) void k_sens_jac_series_masked(SolveArgs a, LevArgs la, SensJacArgs ja, SeriesArgs sr,
                                                                          const double* __restrict__ dg_at_psi, int per, int R, int nslice,
                                                                          ColMask m) {
  extern __shared__ double rows[];  // [nsel][R][blockDim.x]
  const int c = blockIdx.x;
  if (col_skipped(m, c)) return;
  const int zt = blockIdx.z / nslice, slice = blockIdx.z - zt * nslice;
  const long long tl = (long long)zt * gridDim.y + blockIdx.y;
  if (tl >= sr.nt) return;  // (whole workgroup, before any barrier)
  const long long v = (long long)c * sr.nt + tl;
  const long long din = (long long)c * sr.col_stride + tl * a.nb - (long long)c * a.col_stride;
  a.I_dr0 = static_cast<const double*>(sr.I_dr0) + din;
  a.I_df0 = static_cast<const double*>(sr.I_df0) + din;
  const RecSeries rc = {sr.can + (long long)c * sr.canlen, sr.sun + v * sr.sunlen, dg_at_psi + v, sr.scheme, sr.nz};
  sens_jac_body<G, BL>(a, la, ja, per, R, c, slice, nslice, v, rc, rows);
}

__global__ __launch_bounds__(256) void k_sens_jac_finish_masked(SensArgs sn, long long ncol, int nslice, int per, int nb, int nsel, int npar,
                                                                int nt, ColMask m) {
  sens_jac_finish_body<true>(sn, ncol, nslice, per, nb, nsel, npar, m, nt);
}

// sr: nullptr = the per-step kernel; else the series kernel on the same slices (dg_at_psi [ncol][nt]: the series tangent, or nullptr)
template <class G, bool BL = false>
int launch_sens_jac_closed(const SolveArgs& a, const LevArgs& la, const SensJacArgs& ja, hipStream_t s, bool probe, const SeriesArgs* sr,
                           const double* dg_at_psi, ColMask m) {
  const int npar = ja.ntan + ja.lai + ja.leaf, nsens = ja.sn.nsens;
  const LevSlices ls = sensjac_slices(a.nb, la.nsel, npar);
  if (ls.nslice == 0 || ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  dim3 grid(a.ncol, ls.nslice);
  if (sr && !lev_series_grid(a.ncol, sr->nt, ls.nslice, &grid)) return CRT_ERR_UNSUPPORTED;
  const long long nv = (long long)a.ncol * (sr ? sr->nt : 1);
  const long long nfin = (nv * la.nsel * nsens * npar * 4 + 255) / 256;
  if (ls.nslice > 1 && nfin > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const int R = sensjac_rows(ja.ntan);
  const size_t sh = (size_t)la.nsel * R * ls.nthr * sizeof(double);  // (<= the bound of sensjac_slices: ntan <= npar)
  const bool fin = ls.nslice > 1;
  int st;
  if (m.skip) {
    st = sr ? launch_kernel(k_sens_jac_series_masked<G, BL>, grid, ls.nthr, sh, s, a, la, ja, *sr, dg_at_psi, ls.per, R, ls.nslice, m)
            : launch_kernel(k_sens_jac_masked<G, BL>, grid, ls.nthr, sh, s, a, la, ja, ls.per, R, m);
    if (st == CRT_OK && fin)
      st = launch_kernel(k_sens_jac_finish_masked, dim3((unsigned)nfin), 256, 0, s, ja.sn, nv, ls.nslice, ls.per, a.nb, la.nsel, npar,
                         sr ? sr->nt : 1, m);
  } else {
    st = sr ? launch_kernel(k_sens_jac_series<G, BL>, grid, ls.nthr, sh, s, a, la, ja, *sr, dg_at_psi, ls.per, R, ls.nslice)
            : launch_kernel(k_sens_jac<G, BL>, grid, ls.nthr, sh, s, a, la, ja, ls.per, R);
    if (st == CRT_OK && fin)
      st = launch_kernel(k_sens_jac_finish, dim3((unsigned)nfin), 256, 0, s, ja.sn, nv, ls.nslice, ls.per, a.nb, la.nsel, npar);
  }
  if (st == CRT_OK) {
    const char* const f = !fin ? "" : m.skip ? " + k_sens_jac_finish_masked" : " + k_sens_jac_finish";
    const char* const mk = m.skip ? "_masked" : "";
    if (sr)
      note_kernel("k_sens_jac_series%s<%s> nt=%d nsel=%d nsens=%d npar=%d slice=%d%s", mk, G::J::NAME, sr->nt, la.nsel, nsens, npar, ls.per, f);
    else
      note_kernel("k_sens_jac%s<%s> nsel=%d nsens=%d npar=%d slice=%d%s", mk, G::J::NAME, la.nsel, nsens, npar, ls.per, f);
  }
  return st;
}

}  // namespace

int launch_sens_jac(int scheme, const SolveArgs& a, const LevArgs& la, const SensJacArgs& ja, hipStream_t s, bool probe, const SeriesArgs* sr,
                    const double* dg_at_psi, ColMask m) {
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_sens_jac_closed<S2s>(a, la, ja, s, probe, sr, dg_at_psi, m);
    case CRT_SCHEME_BL: return launch_sens_jac_closed<SBl, true>(a, la, ja, s, probe, sr, dg_at_psi, m);
    case CRT_SCHEME_G77: return launch_sens_jac_closed<SG77<false>>(a, la, ja, s, probe, sr, dg_at_psi, m);
    case CRT_SCHEME_BF: return launch_sens_jac_closed<SG77<true>>(a, la, ja, s, probe, sr, dg_at_psi, m);
    default: return CRT_ERR_UNSUPPORTED;
  }
}

}  // namespace crt
