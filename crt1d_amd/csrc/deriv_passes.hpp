// What the closed-form (2s, bl, g77, bf) derivative kernels share, written once: k_jac (jac.hip), k_dlai (dlai.hip), k_dleaf (dleaf.hip)
// and k_grad (grad.hip) are a staging step, a band load and pass calls with a sink for the tangents of a row.  sens_jac_body (sensjac.hip)
// uses the scheme triples and seed_band and keeps its own staging and pass loops: on the shared ones k_sens_jac_series<2s> and <bf> ran
// slower.
//   Sch2s / SchBl / SchG77   the three jac_schemes.hpp instantiations of a scheme: optics pass | LAI pass | leaf-angle pass
//   stage_record             the staging of k_jac, k_dlai and k_dleaf; k_grad, which stages the tangents of both record derivatives
//                            at once, keeps its own lines
//   pass_optics              one seeded optical parameter: sink(r, dn', up')
//   pass_record              the LAI or the leaf angles: sink(r, I_dr', dn', up'); F' of the row by flux_tan, where it is asked for
// A pass is the same operations on the same inputs in every kernel that calls it (-ffp-contract=off), so k_grad has the tangent bits
// of the single-derivative kernels by construction.
#pragma once
#include "jac_schemes.hpp"

namespace crt {
namespace {

struct Sch2s {
  using J = J2sT<Du, double>;
  using D = J2sT<double, Du>;
  using F = J2sT<double, Du, Du>;
};
struct SchBl {
  using J = JBlT<Du, double>;
  using D = JBlT<double, Du>;
  using F = JBlT<double, Du, Du>;
};
template <bool BF>
struct SchG77 {
  using J = JG77T<BF, Du, double>;
  using D = JG77T<BF, double, Du>;
  using F = JG77T<BF, double, Du, Du>;
};

// the band of load_dband with parameter p seeded (uniform)
__device__ __forceinline__ JBandT<Du> seed_band(const DBand& in, int p) {
  return JBandT<Du>{in.I_dr0, in.I_df0, Du{in.r, p == 0 ? 1.0 : 0.0}, Du{in.t, p == 1 ? 1.0 : 0.0}, Du{in.s, p == 2 ? 1.0 : 0.0}};
}

// Staging for the single-derivative kernels (k_jac, k_dlai, k_dleaf), every thread of the workgroup; ends with the barrier.  `rec`: the
// column's record.  hd: the header | e^{-K_b LT} at the ground and, with TAN, the header's leaf-angle tangents at HDR_TAN (hdr<Du>);
// lvL, lvE: L_j and e^{-K_b L_j} of the selected levels; BL: lvT, bl's tau_d tangents.  `side`: the column's side record -- with TAN that
// of k_dleaf_side (header tangents, then bl's tau_d^th(L_j)), else bl's [nz] vector L_j tau_d'(L_j) of k_dlai_side.  The LDS arrays are
// the kernel's own declarations, so its static LDS stays what it was.
template <bool TAN, bool BL>
__device__ __forceinline__ void stage_record(const double* rec, int nz, const LevArgs& la, const double* side, double* hd, double* lvL, double* lvE,
                                             double* lvT) {
  const int tid = threadIdx.x;
  if (tid < REC_HDR) {
    hd[tid] = rec[tid];
    if constexpr (TAN) hd[HDR_TAN + tid] = side[tid];
  }
  if (tid == REC_HDR) hd[REC_HDR] = rec[REC_HDR + nz];  // e^{-K_b L} at the ground
  for (int r = tid; r < la.nsel; r += blockDim.x) {
    const int j = la.lev[r];
    lvL[r] = rec[REC_HDR + j];
    lvE[r] = rec[REC_HDR + nz + j];
    if constexpr (BL) lvT[r] = side[(TAN ? REC_HDR : 0) + j];
  }
  __syncthreads();
}

// One optical parameter, seeded in `band`: the band constants are differentiated once, then every selected level is evaluated on its own.
template <class SJ, class Sink>
__device__ __forceinline__ void pass_optics(const double* hd, const double* lvL, const double* lvE, int nsel, const JBandT<Du>& band, Sink&& sink) {
  SJ st;
  st.init(hd, band, hd[REC_HDR]);
  for (int r = 0; r < nsel; ++r) {
    Du dn, up;
    st.level(lvL[r], lvE[r], dn, up);
    sink(r, dn, up);
  }
}

// The record's tangent: the LAI (S = Sch::D: L_j' = L_j, LT' = LT, K = K_b) or, LEAF, the leaf angles (S = Sch::F: the header tangents,
// K = K_b'); either way (e^{-K_b L_j})' = -K L_j e^{-K_b L_j}.  lvT: bl's tau_d tangents of this derivative.
template <class S, bool BL, bool LEAF, class Sink>
__device__ __forceinline__ void pass_record(const double* hd, const double* lvL, const double* lvE, const double* lvT, int nsel, const DBand& in,
                                            Sink&& sink) {
  const double K = hd[(LEAF ? HDR_TAN : 0) + S_KB];
  S st;
  st.init(hd, in, Du{hd[REC_HDR], -(K * hd[S_LT]) * hd[REC_HDR]});
  for (int r = 0; r < nsel; ++r) {
    const double L = lvL[r];
    const Du eK = Du{lvE[r], -(K * L) * lvE[r]};
    Du dn, up;
    if constexpr (LEAF)
      st.level(L, eK, dn, up);
    else
      st.level(Du{L, L}, eK, dn, up);
    if constexpr (BL) dn.d += in.I_df0 * lvT[r];  // the sky term I_df0 tau_d(L_j)
    sink(r, in.I_dr0 * eK.d, dn, up);
  }
}

}  // namespace
}  // namespace crt
