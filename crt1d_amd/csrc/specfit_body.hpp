// The work of one workgroup of the spectral normal equations, shared by k_spec_normal (specfit.hip) and k_spec_normal_series
// (specfit_series.hip): the staging, the passes of deriv_passes.hpp, the weights and the one-entry-at-a-time contraction, written once over
// a record accessor, as sens_jac_body (sensjac.hip) is over RecStep / RecSeries.  The accessors below are COPIES of those two with the one
// entry this body needs on top (tau_d(L_j), bl's primal sky term): sensjac.hip keeps its own, so that its device code stays what it is.
#pragma once
#include "deriv_passes.hpp"
#include "specfit.hpp"

namespace crt {

// Where the body finds the band-independent entries of its (column, sun state): the header scalar i, the LAI L_j, the beam fraction
// e^{-K_b L_j} and (bl) tau_d(L_j) of level j (j = 0: the ground), and the tangent of header scalar i along the leaf-angle direction.
struct SpecRecStep {  // the record k_colpre wrote; sdl: the side record of k_dleaf_side
  const double* rec;
  int nz;
  __device__ __forceinline__ double hdr(int i) const { return rec[i]; }
  __device__ __forceinline__ double L(int j) const { return rec[REC_HDR + j]; }
  __device__ __forceinline__ double E(int j) const { return rec[REC_HDR + nz + j]; }
  __device__ __forceinline__ double Td(int j) const { return rec[REC_HDR + 2 * nz + j]; }
  __device__ __forceinline__ double dhdr(const double* sdl, int i) const { return sdl[i]; }
};
// The canopy record of the column and the sun record of (column, t) (SeriesArgs, crt_internal.hpp), each entry read where it lies.  sdl: the
// side record of k_dleaf_side<canopy>, which leaves out the one tangent that follows the sun: K_b' = dG(psi_t) / cos psi_t, the division
// k_dleaf_side does.
struct SpecRecSeries {
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
  __device__ __forceinline__ double Td(int j) const { return vec(2, j); }
  __device__ __forceinline__ double dhdr(const double* sdl, int i) const { return i == S_KB ? *dgp / hdr(S_MU) : sdl[i]; }
};

// the sum of v over the workgroup in a fixed order, valid in thread 0 (every thread calls): butterfly over the wave, then wave 0, 1, ...
// (grad.hip's block_sum)
__device__ __forceinline__ double spec_block_sum(double v, double* red) {
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

// Column c, band slice `slice`, observations and fwd indexed by v (the column; series: c * nt + t).  `a` carries the spectra of v at the
// column's index.  Thread 0 stores the (npar + 1)(npar + 2) / 2 sums of this slice to sp.part[v nslice + slice]; PART false (the per-step
// kernel: nslice is its gridDim.y, nslice_part is not looked at) and one slice: straight to sp.A / g / c2 of v.  The slot is formed behind
// the passes, so that nothing of it is live across them: the passes sit at the limit of the scalar registers.
template <class G, bool BL, bool PART, class Rec, class V>
__device__ __forceinline__ void spec_normal_body(const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, int per, int c, int slice,
                                                 const V v, const Rec rc, int nslice_part) {
  using SJ = typename G::J;
  extern __shared__ double rows[];          // [nkey][nsel][npar + 1][blockDim.x]
  __shared__ double hd[HDR_TAN + REC_HDR];  // k_dleaf's layout: header | e^{-K_b LT} at the ground | ... | the header's leaf-angle tangents
  __shared__ double lvL[CRT_MAX_LEVEL_SELECT], lvE[CRT_MAX_LEVEL_SELECT], lvTs[CRT_MAX_LEVEL_SELECT], lvTh[CRT_MAX_LEVEL_SELECT];
  __shared__ double lvTd[CRT_MAX_LEVEL_SELECT];  // bl: tau_d(L_j), the sky term of the primal
  __shared__ double red[SPEC_BLOCK / 64];
  const int nz = a.nz, nb = a.nb, nsel = la.nsel, tid = threadIdx.x, nthr = blockDim.x;
  const int b = slice * per + tid;
  const bool live = tid < per && b < nb;
  const int ntan = sp.ntan, npar = ntan + sp.lai + sp.leaf, na = npar + 1;
  // k_grad's staging: the tangents of both record derivatives at once
  const double* sdl = sp.side_leaf + (long long)c * (REC_HDR + (BL ? nz : 0));
  if (tid < REC_HDR) {
    hd[tid] = rc.hdr(tid);
    hd[HDR_TAN + tid] = sp.leaf ? rc.dhdr(sdl, tid) : 0.0;
  }
  if (tid == REC_HDR) hd[REC_HDR] = rc.E(0);  // e^{-K_b L} at the ground
  for (int r = tid; r < nsel; r += nthr) {
    const int j = la.lev[r];
    lvL[r] = rc.L(j);
    lvE[r] = rc.E(j);
    if constexpr (BL) {
      lvTs[r] = sp.lai ? sp.side_lai[(long long)c * nz + j] : 0.0;  // L_j tau_d'(L_j)
      lvTh[r] = sp.leaf ? sdl[REC_HDR + j] : 0.0;                   // tau_d^th(L_j)
      lvTd[r] = rc.Td(j);
    }
  }
  __syncthreads();
  const double invmu = hd[S_INVMU];
  const long long o0 = (long long)v * nsel * nb + b;  // row r of the observations: + r nb
  double* const my = rows + tid;           // entry i of (key kq, level r): my[((kq nsel + r) na + i) nthr]
  const size_t lev = (size_t)na * nthr, key = lev * nsel;

  if (live) {
    const DBand in = load_dband(a, c, b, SJ::SOIL);

    // ---- the primal: the closed form the passes below differentiate, no parameter seeded ----
    pass_optics<SJ>(hd, lvL, lvE, nsel, seed_band(in, -1), [&](int r, Du dn, Du up) {
      const double idr = in.I_dr0 * lvE[r];
      double d = dn.v;
      if constexpr (BL) d = in.I_df0 * lvTd[r] + d;  // the sky term I_df0 tau_d(L_j)
      const double x[4] = {idr, d, up.v, __builtin_fma(idr, invmu, 2 * (up.v + d))};
      double* y = my + r * lev + (size_t)npar * nthr;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (sp.y[q]) {
          *y = x[q];
          if (sp.fwd[q]) sp.fwd[q][o0 + (long long)r * nb] = x[q];
          y += key;
        }
    });

    // ---- the directions: the optics one parameter at a time (k_jac), each tangent times the lane's band of every direction ----
    if (ntan > 0) {
      bool first = true;  // (uniform)
      for (int p = 0; p < CRT_JAC_NPARAM; ++p) {
        if (!sp.d[p] || (!SJ::SOIL && p == 2)) continue;  // (bl has no soil)
        const double* dp = sp.d[p] + (long long)c * sp.dstride + b;
        double d[CRT_SENSJAC_MAX_NTAN];
#pragma unroll
        for (int k = 0; k < CRT_SENSJAC_MAX_NTAN; ++k) d[k] = k < ntan ? dp[(long long)k * nb] : 0.0;
        pass_optics<SJ>(hd, lvL, lvE, nsel, seed_band(in, p), [&](int r, Du dn, Du up) {
          const double x[4] = {0.0, dn.d, up.d, 2 * (up.d + dn.d)};  // F' as jac_store; I_dr does not depend on the optics
          double* y = my + r * lev;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (sp.y[q]) {
#pragma unroll
              for (int k = 0; k < CRT_SENSJAC_MAX_NTAN; ++k)
                if (k < ntan) {
                  double* const e = y + (size_t)k * nthr;
                  if (q == 0) {
                    if (first) *e = 0.0;
                  } else {
                    const double t = x[q] * d[k];
                    *e = first ? t : *e + t;
                  }
                }
              y += key;
            }
        });
        first = false;
      }
      if (first)  // (bl with directions in soil_r alone: zeros)
        for (int t = 0; t < sp.nkey * nsel; ++t)
          for (int k = 0; k < ntan; ++k) my[t * lev + (size_t)k * nthr] = 0.0;
    }

    // ---- the LAI (k_dlai) ----
    if (sp.lai)
      pass_record<typename G::D, BL, false>(hd, lvL, lvE, lvTs, nsel, in, [&](int r, double dI, Du dn, Du up) {
        const double x[4] = {dI, dn.d, up.d, flux_tan(dI, invmu, dn, up)};
        double* y = my + r * lev + (size_t)ntan * nthr;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (sp.y[q]) {
            *y = x[q];
            y += key;
          }
      });

    // ---- the leaf angles (k_dleaf) ----
    if (sp.leaf)
      pass_record<typename G::F, BL, true>(hd, lvL, lvE, lvTh, nsel, in, [&](int r, double dI, Du dn, Du up) {
        const double x[4] = {dI, dn.d, up.d, flux_tan(dI, invmu, dn, up)};
        double* y = my + r * lev + (size_t)(ntan + sp.lai) * nthr;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (sp.y[q]) {
            *y = x[q];
            y += key;
          }
      });

    // ---- the weights: w_i = X'_i s and r = (X - y) s, each rounded once; a skipped row becomes a row of +0 ----
    for (int r = 0; r < nsel; ++r) {
      const long long o = o0 + (long long)r * nb;
      double* y = my + r * lev;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (sp.y[q]) {
          const double s = sp.is[q] ? sp.is[q][o] : 1.0;
          if (s != 0.0) {
            for (int i = 0; i < npar; ++i) y[(size_t)i * nthr] = y[(size_t)i * nthr] * s;
            y[(size_t)npar * nthr] = (y[(size_t)npar * nthr] - sp.y[q][o]) * s;
          } else {
            for (int i = 0; i <= npar; ++i) y[(size_t)i * nthr] = 0.0;
          }
          y += key;
        }
    }
  }

  // ---- (A | g | c2), one entry at a time: the products of a lane in the order (key, level), then the lanes ----
  const int ntri = npar * (npar + 1) / 2, nent = na * (na + 1) / 2, nrow = sp.nkey * nsel;
  const int nslice = PART ? nslice_part : (int)gridDim.y;  // (the per-step grid: read here, behind the passes)
  double* const dst = !PART && nslice == 1 ? nullptr : sp.part + ((long long)v * nslice + slice) * nent;
  int i = 0, j = 0;
  for (int e = 0; e < nent; ++e) {
    double acc = 0.0;
    if (live) {
      const double *yi = my + (size_t)i * nthr, *yj = my + (size_t)j * nthr;
      for (int t = 0; t < nrow; ++t) acc = acc + yi[t * lev] * yj[t * lev];
    }
    const double s = spec_block_sum(acc, red);
    if (tid == 0) {
      if (dst) dst[e] = s;
      else if (e < ntri) sp.A[(long long)v * ntri + e] = s;
      else if (e < ntri + npar) sp.g[(long long)v * npar + e - ntri] = s;
      else sp.c2[v] = s;
    }
    if (++j > i) {
      ++i;
      j = 0;
    }
  }
}

}  // namespace crt
