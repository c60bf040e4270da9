// Spectral normal equations (include/crt1d_hip_specfit.h; kernels in specfit.hip): what api.hip (the entry, on levels_deriv_impl) and
// specfit.hip (the launcher) share.  A header of its own: crt_internal.hpp stays what it is.
#pragma once
#include "crt1d_hip_specfit.h"
#include "crt_internal.hpp"

namespace crt {

struct SpecArgs {
  const double* y[4];       // observations of I_dr, I_df_d, I_df_u, F: [ncol][nsel][nb] or NULL (not observed)
  const double* is[4];      // their inv_sigma or NULL (ones)
  double* fwd[4];           // the model spectrum [ncol][nsel][nb] or NULL
  double *A, *g, *c2;       // [ncol][ntri], [ncol][npar], [ncol]
  double* part;             // [ncol][nslice][nent]: the slice sums (several band slices)
  const double* d[3];       // directions in leaf_r, leaf_t, soil_r: [ncol or 1][ntan][nb] or NULL
  long long dstride;        // 0 or ntan * nb
  int ntan, lai, leaf;      // parameter columns: ntan directions, ln LAI (0 / 1), the leaf angle (0 / 1)
  int nkey;                 // observed keys
  const double* side_lai;   // side records of k_dlai_side  (read for bl with `lai`)
  const double* side_leaf;  // side records of k_dleaf_side (read with `leaf`)
};
constexpr int SPEC_BLOCK = 256;           // bands per slice at most
constexpr size_t SPEC_STATIC_LDS = 4096;  // allowance for the kernel's static LDS (header, tangents, level entries, wave sums: 2976 bytes)
constexpr int spec_nent(int npar) { return (npar + 1) * (npar + 2) / 2; }  // entries of (A | g | c2)
// LDS rows of one double per lane: (w_0 .. w_{npar-1}, r) of every (observed key, level)
constexpr size_t spec_rows(int nsel, int nkey, int npar) { return (size_t)nsel * nkey * (npar + 1); }
// the widest of 256, 128, 64 lanes whose rows fit; nslice = 0: none
inline LevSlices spec_slices(int nb, int nsel, int nkey, int npar) {
  int wmax = SPEC_BLOCK;
  while (wmax >= 64 && spec_rows(nsel, nkey, npar) * wmax * sizeof(double) > 160 * 1024 - SPEC_STATIC_LDS) wmax >>= 1;
  if (wmax < 64) return LevSlices{0, 0, 0};
  return lev_slices(nb, wmax);
}
static_assert(312 * 64 * sizeof(double) <= 160 * 1024 - SPEC_STATIC_LDS && 313 * 64 * sizeof(double) > 160 * 1024 - SPEC_STATIC_LDS,
              "the limit crt1d_hip_specfit.h states");
// bytes of the slice sums behind the side records (0 with one slice; where no slice width fits, those of 64-lane slices: the call refuses)
inline size_t spec_part_bytes(int ncol, int nb, int nsel, int nkey, int npar) {
  LevSlices ls = spec_slices(nb, nsel, nkey, npar);
  if (ls.nslice == 0) ls = lev_slices(nb, 64);
  if (ls.nslice <= 1) return 0;
  return (size_t)ncol * (size_t)ls.nslice * spec_nent(npar) * sizeof(double);
}
// probe: return the status (CRT_OK / CRT_ERR_UNSUPPORTED) of the configuration without launching anything
// m (skip != nullptr): the masked kernels of include_mask/crt1d_hip_masked.h
int launch_spec_normal(int scheme, const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, hipStream_t s, bool probe, ColMask m = {});

// The sun-angle series (include/series/crt1d_hip_specfit_series.h; kernels in specfit_series.hip).  sp: y / is / fwd are indexed by
// c * nt + t, A / g / c2 are the sums over t, part is [ncol][nt][nslice][nent] and ALWAYS there: the sum over t goes through it.
struct SpecSeriesOut {
  double *A_t, *g_t, *c2_t;  // [ncol][nt][ntri], [ncol][nt][npar], [ncol][nt], or all NULL
};
// bytes of the slice sums of every (column, t), one slice included; SIZE_MAX: beyond size_t
inline size_t spec_series_part_bytes(int ncol, int nb, int nsel, int nkey, int npar, int nt) {
  LevSlices ls = spec_slices(nb, nsel, nkey, npar);
  if (ls.nslice == 0) ls = lev_slices(nb, 64);
  const size_t per = (size_t)ls.nslice * spec_nent(npar) * sizeof(double), nv = (size_t)ncol * (size_t)nt;
  return nv > SIZE_MAX / per ? SIZE_MAX : nv * per;
}
// a.ws / sr.can hold canopy records, side_leaf comes from launch_dleaf_side(.., canopy = true), dg_at_psi is [ncol][nt] (or nullptr)
int launch_spec_normal_series(int scheme, const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, const SpecSeriesOut& so,
                              const SeriesArgs& sr, const double* dg_at_psi, hipStream_t s, bool probe, ColMask m = {});

}  // namespace crt
