// Argument blocks and launchers of the absorption + band-sum epilogue (epilogue.hip).  api.hip validates a call, fills a block and
// calls a launcher; which kernel serves a shape is decided in epilogue.hip alone.
#pragma once

#include "crt_internal.hpp"

namespace crt {

constexpr int MAXG = 4;
typedef double d2 __attribute__((ext_vector_type(2)));

// TIO = double | float: element type of the spectra and profiles the epilogue reads (crt_hip_absorb_bandsum*_f64 / _f32).  Every load
// converts to double at once; band_w, the geometry, the arithmetic and all band-sum outputs are fp64 for both.
template <typename TIO>
struct EpiArgsT {
  int ncol, nb, nz, ngroup;
  long long col_stride;
  const double* psi;
  const double* lai;
  const int32_t* g_kind;
  const double* g_param;
  const double* g_at_psi;
  const TIO* leaf_r;
  const TIO* leaf_t;
  const TIO* I_dr;
  const TIO* I_df_d;
  const TIO* I_df_u;
  const double* band_w;
  double* aI;
  double* aI_sl;
  double* aI_sh;
  double* totals;
  // optional (crt_bandsum_out), all six or none: the direct-beam part of the absorption [ncol][nz-1][ngroup], and the band-integrated
  // LEVEL profiles [ncol][nz][ngroup] of every irradiance variable diagnostics.band sums (diagnostics.py:84-91): I_dr, I_df_d, I_df_u, F, I_d
  double* aI_dr;
  double* L_dr;
  double* L_dn;
  double* L_up;
  double* L_F;
  double* L_Id;
};

// Per-band layer absorption (k_absorb, k_absorb_tile).  TIO = double | float: the three input profiles, the leaf optics and the seven
// outputs (crt_hip_absorb_f64 / _f32).  The arithmetic is fp64 for both: a float output is the fp64 value rounded once.  laim and f_slm are fp64.
template <typename TIO>
struct AbsArgsT {
  int ncol, nb, nz;
  long long col_stride;
  const double* psi;
  const double* lai;
  const int32_t* g_kind;
  const double* g_param;
  const double* g_at_psi;
  const TIO* leaf_r;
  const TIO* leaf_t;
  const TIO* I_dr;
  const TIO* I_df_d;
  const TIO* I_df_u;
  TIO* o[7];  // aI, aI_df, aI_dr, aI_sh, aI_sl, aI_df_sl, aI_df_sh
  double* laim;
  double* f_slm;
};

// k_bandsum_finish (crt_hip_bandsum_finish_f64)
struct FinishArgs {
  int ncol, nz, ngroup;
  const double* psi;
  const double* aI_sl;
  const double* aI_sh;
  const double* L_dr;
  const double* L_dn;
  const double* L_up;
  double* aI;
  double* L_F;
  double* L_Id;
};

// Each takes a filled, validated argument block, picks the kernel for its shape and alignment and returns CRT_OK or CRT_ERR_LAUNCH (TIO: double, float).
template <typename TIO>
int launch_bandsum(const EpiArgsT<TIO>& a, hipStream_t s);
template <typename TIO>
int launch_absorb(const AbsArgsT<TIO>& a, hipStream_t s);
int launch_bandsum_finish(const FinishArgs& a, hipStream_t s);
int launch_band_reduce(const double* X, long long nrow, int nb, const double* band_w, int ngroup, double* out, hipStream_t s);

}  // namespace crt
