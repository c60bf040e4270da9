// Spectral normal equations over a sun-angle series (include/series/crt1d_hip_specfit_series.h): A = J^T W J, g = J^T W r and c2 = sum r^2
// of the per-band misfit of the level spectra of nt sun states of every column, on one canopy with one parameter vector, summed over t.
//
//  k_spec_normal_series         the body of k_spec_normal (spec_normal_body, specfit_body.hpp) for one (column, band slice, sun state) on
//                               the grid of lev_series_grid; the header, the selected entries of L_j, e^{-K_b L_j} and tau_d(L_j) and the
//                               ground entry are read straight from the canopy record of the column and the sun record of (column, t), and
//                               K_b' of the leaf-angle pass is formed here, dG(psi_t) / cos psi_t (SpecRecSeries) -- the relation
//                               k_sens_jac_series has to k_sens_jac.  Same slices (spec_slices), lanes, LDS rows and order as k_spec_normal:
//                               the sums of (column, t) have the per-step bits.  Thread 0 writes them to part[(c nt + t) nslice + slice].
//  k_spec_normal_series_finish  a thread per (column, entry): for t = 0, 1, ... the slice sums in ascending slice order, starting from slice
//                               0's bits (k_spec_normal_finish's rule) -- stored to A_t / g_t / c2_t where asked for --, and the total over t
//                               in ascending t, starting from t = 0's bits: what k_lm_step_normal forms from nt blocks.
// No atomics, no cross-column reads: a column's result does not depend on the batch or on another column's mask.
#include "specfit_body.hpp"

namespace crt {
namespace {

struct Q2s : Sch2s {};
struct QBl : SchBl {};
template <bool BF>
struct QG77 : SchG77<BF> {};

// One workgroup per (column, band slice, sun state); the spectra of (column, t) as in series_lev_step.
template <class G, bool BL>
__global__ __launch_bounds__(SPEC_BLOCK) void k_spec_normal_series(SolveArgs a, LevArgs la, SpecArgs sp, SeriesArgs sr,
                                                                   const double* __restrict__ dg_at_psi, int per, int nslice) {
  const int c = blockIdx.x;
  const int zt = blockIdx.z / nslice, slice = blockIdx.z - zt * nslice;
  const long long tl = (long long)zt * gridDim.y + blockIdx.y;
  if (tl >= sr.nt) return;  // (whole workgroup, before any barrier)
  const long long v = (long long)c * sr.nt + tl;
  const long long din = (long long)c * sr.col_stride + tl * a.nb - (long long)c * a.col_stride;
  a.I_dr0 = static_cast<const double*>(sr.I_dr0) + din;
  a.I_df0 = static_cast<const double*>(sr.I_df0) + din;
  const double* dgp = dg_at_psi ? dg_at_psi + v : nullptr;  // (no leaf-angle column: no tangent, nothing to point into)
  const SpecRecSeries rc = {sr.can + (long long)c * sr.canlen, sr.sun + v * sr.sunlen, dgp, sr.scheme, sr.nz};
  spec_normal_body<G, BL, true>(a, la, sp, per, c, slice, v, rc, nslice);
}

// One thread per (column, entry): s_t = the slice sums of (column, t) in ascending slice order, the total = s_0 + s_1 + ... in this order.
// MASKED: an entry of a skipped column keeps its bits (the per-step sums too), and its slice sums are not read.
template <bool MASKED>
__device__ __forceinline__ void spec_series_finish_body(long long ncol, int nt, int nslice, int npar, const double* __restrict__ part,
                                                        double* __restrict__ A, double* __restrict__ g, double* __restrict__ c2,
                                                        const SpecSeriesOut& so, ColMask m) {
  const int ntri = npar * (npar + 1) / 2, nent = (npar + 1) * (npar + 2) / 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncol * nent) return;
  const long long c = i / nent;
  if constexpr (MASKED)
    if (col_skipped(m, (int)c)) return;
  const int e = (int)(i - c * nent);
  double tot = 0.0;
  for (int t = 0; t < nt; ++t) {
    const long long v = c * nt + t;
    const double* p = part + v * nslice * nent + e;
    double s = p[0];
    for (int sl = 1; sl < nslice; ++sl) s += p[(long long)sl * nent];
    if (so.A_t) {
      if (e < ntri) so.A_t[v * ntri + e] = s;
      else if (e < ntri + npar) so.g_t[v * npar + e - ntri] = s;
      else so.c2_t[v] = s;
    }
    tot = t == 0 ? s : tot + s;
  }
  if (e < ntri) A[c * ntri + e] = tot;
  else if (e < ntri + npar) g[c * npar + e - ntri] = tot;
  else c2[c] = tot;
}

__global__ __launch_bounds__(256) void k_spec_normal_series_finish(long long ncol, int nt, int nslice, int npar, const double* __restrict__ part,
                                                                    double* __restrict__ A, double* __restrict__ g, double* __restrict__ c2,
                                                                    SpecSeriesOut so) {
  spec_series_finish_body<false>(ncol, nt, nslice, npar, part, A, g, c2, so, ColMask{});
}

// ---- the masked forms (include_mask/crt1d_hip_masked.h): every workgroup of a skipped column returns before it reads anything of the
// column and before any barrier (the column is blockIdx.x, known before the sun state is decoded); an evaluated column runs the body of its
// plain sibling.
template <class G, bool BL>
__global__ __launch_bounds__(SPEC_BLOCK) void k_spec_normal_series_masked(SolveArgs a, LevArgs la, SpecArgs sp, SeriesArgs sr,
                                                                          const double* __restrict__ dg_at_psi, int per, int nslice, ColMask m) {
  const int c = blockIdx.x;
  if (col_skipped(m, c)) return;
  const int zt = blockIdx.z / nslice, slice = blockIdx.z - zt * nslice;
  const long long tl = (long long)zt * gridDim.y + blockIdx.y;
  if (tl >= sr.nt) return;  // (whole workgroup, before any barrier)
  const long long v = (long long)c * sr.nt + tl;
  const long long din = (long long)c * sr.col_stride + tl * a.nb - (long long)c * a.col_stride;
  a.I_dr0 = static_cast<const double*>(sr.I_dr0) + din;
  a.I_df0 = static_cast<const double*>(sr.I_df0) + din;
  const double* dgp = dg_at_psi ? dg_at_psi + v : nullptr;
  const SpecRecSeries rc = {sr.can + (long long)c * sr.canlen, sr.sun + v * sr.sunlen, dgp, sr.scheme, sr.nz};
  spec_normal_body<G, BL, true>(a, la, sp, per, c, slice, v, rc, nslice);
}

__global__ __launch_bounds__(256) void k_spec_normal_series_finish_masked(long long ncol, int nt, int nslice, int npar,
                                                                           const double* __restrict__ part, double* __restrict__ A,
                                                                           double* __restrict__ g, double* __restrict__ c2, SpecSeriesOut so,
                                                                           ColMask m) {
  spec_series_finish_body<true>(ncol, nt, nslice, npar, part, A, g, c2, so, m);
}

template <class G, bool BL = false>
int launch_spec_series_closed(const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, const SpecSeriesOut& so, const SeriesArgs& sr,
                              const double* dg_at_psi, hipStream_t s, bool probe, ColMask m) {
  const int npar = sp.ntan + sp.lai + sp.leaf;
  const LevSlices ls = spec_slices(a.nb, la.nsel, sp.nkey, npar);
  if (ls.nslice == 0 || ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  dim3 grid;
  if (!lev_series_grid(a.ncol, sr.nt, ls.nslice, &grid)) return CRT_ERR_UNSUPPORTED;
  const long long nfin = ((long long)a.ncol * spec_nent(npar) + 255) / 256;
  if (nfin > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const size_t sh = spec_rows(la.nsel, sp.nkey, npar) * ls.nthr * sizeof(double);  // (<= the bound of spec_slices)
  int st;
  if (m.skip) {
    st = launch_kernel(k_spec_normal_series_masked<G, BL>, grid, ls.nthr, sh, s, a, la, sp, sr, dg_at_psi, ls.per, ls.nslice, m);
    if (st == CRT_OK)
      st = launch_kernel(k_spec_normal_series_finish_masked, dim3((unsigned)nfin), 256, 0, s, (long long)a.ncol, sr.nt, ls.nslice, npar, sp.part,
                         sp.A, sp.g, sp.c2, so, m);
  } else {
    st = launch_kernel(k_spec_normal_series<G, BL>, grid, ls.nthr, sh, s, a, la, sp, sr, dg_at_psi, ls.per, ls.nslice);
    if (st == CRT_OK)
      st = launch_kernel(k_spec_normal_series_finish, dim3((unsigned)nfin), 256, 0, s, (long long)a.ncol, sr.nt, ls.nslice, npar, sp.part, sp.A,
                         sp.g, sp.c2, so);
  }
  if (st == CRT_OK) {
    const char* const mk = m.skip ? "_masked" : "";
    note_kernel("k_spec_normal_series%s<%s> nt=%d nsel=%d nkey=%d npar=%d slice=%d + k_spec_normal_series_finish%s", mk, G::J::NAME, sr.nt,
                la.nsel, sp.nkey, npar, ls.per, mk);
  }
  return st;
}

}  // namespace

int launch_spec_normal_series(int scheme, const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, const SpecSeriesOut& so,
                              const SeriesArgs& sr, const double* dg_at_psi, hipStream_t s, bool probe, ColMask m) {
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_spec_series_closed<Q2s>(a, la, sp, so, sr, dg_at_psi, s, probe, m);
    case CRT_SCHEME_BL: return launch_spec_series_closed<QBl, true>(a, la, sp, so, sr, dg_at_psi, s, probe, m);
    case CRT_SCHEME_G77: return launch_spec_series_closed<QG77<false>>(a, la, sp, so, sr, dg_at_psi, s, probe, m);
    case CRT_SCHEME_BF: return launch_spec_series_closed<QG77<true>>(a, la, sp, so, sr, dg_at_psi, s, probe, m);
    default: return CRT_ERR_UNSUPPORTED;
  }
}

}  // namespace crt
