// Spectral inputs on the device (include/crt1d_hip_spectra.h): raw 1 nm leaf / soil spectra and the incoming spectral irradiance of every
// column become the five arrays of `crt_bands` in one launch -- the light-weighted band averages of crt1d/spectra.py:129-218
// (`avg_optical_prop`, looped over the bands by `smear_avg_optical_prop`, :366-390) and the re-binned irradiance of `smear_si` (:529-573).
//
// One workgroup per column.  The kernel is read-side: 8 (3 nx + 2 nxs) bytes per column in, 40 nb out, so the column's spectra and the
// shared grids are staged into LDS once, by 16-byte loads (non-temporal where all rows of a group are per-column: every byte is used once), and everything
// after that runs out of LDS:
//
//   items   the flattened (band, sub-bin) list of the optics, then the nb irradiance bins; CRT_SPECTRA_BLOCK items per pass, one per
//           thread.  An optics item runs `_smear_tuv_1` (k_smear_tuv's search and trapezoid walk, prep.hip) over its sub-bin for all the
//           column's properties in one walk -- they share x, the sub-bin and the search -- and parks  y_sub w  and  w  in LDS.
//   sums    one lane per (quantity, band) adds the parked values of its band in ascending sub-bin order onto its running sum (LDS, carried
//           from pass to pass).  That order is the contract: a result is the same bits for any ncol, pass split or input sharing.
//   out     sum(y_sub w) / sum(w), bands contiguous.
//
// The Planck weight is  int l_wl_planck  over the sub-bin by a fixed CRT_SPECTRA_NGL-point Gauss-Legendre rule in place of QUADPACK
// (crt1d/spectra.py:42-68); the nodes ride in the kernel arguments, as does sub_off.
#include <hip/hip_runtime.h>
#include <math.h>

#include "crt1d_hip_spectra.h"
#include "crt_internal.hpp"

namespace crt {
namespace {

constexpr int SP_BLOCK = CRT_SPECTRA_BLOCK;
constexpr int SP_NGL = CRT_SPECTRA_NGL;
constexpr int SP_MAXPROP = 3;

struct SpecArgs {
  int nprop, nx, nb, nxs, nlx;    // nxs: irradiance grid (0: no irradiance outputs); nlx: light table of the first entry (else 0)
  int light_kind, light_group, nlight;
  double T_K;
  const double* x;                // [nx]
  const double* y[SP_MAXPROP];    // column c at y[q] + c * ystride[q]
  long long ystride[SP_MAXPROP];
  const double* x_si;             // [nxs]
  const double* si[2];            // SI_dr, SI_df
  long long sistride[2];
  const double* light_x;          // [nlx]
  const double* light_y;          // [nlight][nlx]
  const double* edges;            // [nb + 1]
  double* out[SP_MAXPROP];        // [ncol][nb]
  double* I_out[2];               // [ncol][nb]
  double* y_sub;                  // [ncol][sub_off[nb]] of property 0, or nullptr
  double glx[SP_NGL], glw[SP_NGL];
  int32_t sub_off[CRT_SPECTRA_MAX_NB + 1];
};
static_assert(sizeof(SpecArgs) <= 4096, "kernel arguments");

typedef double dbl2 __attribute__((ext_vector_type(2)));

// NR rows of n doubles each from global memory into LDS, in one branch-free loop so that a thread has a load of every row in flight
// before it waits for the first.  Per row: one scalar to reach 16-byte alignment (a row of odd length starts on an odd double in every
// other column), 16-byte loads, up to three scalars at the end.  Row 0 is a shared grid (plain loads: every workgroup re-reads it from
// cache); NT: rows 1 .. NR-1 are per-column rows, loaded non-temporally (every byte is used once).
template <int NR, bool NT>
__device__ inline void stage(const double* const (&g)[NR], double* const (&l)[NR], int n) {
  const int tid = threadIdx.x;
  int head[NR];
  const dbl2* g2[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    head[q] = ((uintptr_t)g[q] & 8) ? 1 : 0;
    g2[q] = reinterpret_cast<const dbl2*>(g[q] + head[q]);
  }
  const int m = (n - 1) >> 1;  // head + 2 i + 1 <= n - 1 for every i < m, whatever the head
#pragma unroll 2
  for (int i = tid; i < m; i += SP_BLOCK) {
    dbl2 v[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      if (NT && q > 0)
        v[q] = __builtin_nontemporal_load(g2[q] + i);
      else
        v[q] = g2[q][i];
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      l[q][head[q] + 2 * i] = v[q].x;
      l[q][head[q] + 2 * i + 1] = v[q].y;
    }
  }
  // what the pairs leave: element 0 under a head, and the last one to three
  if (tid < 4) {
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const int j = tid == 3 ? 0 : head[q] + 2 * m + tid;
      if (tid == 3 ? head[q] == 1 : j < n) l[q][j] = g[q][j];
    }
  }
}

// `_smear_tuv_1` for NP spectra on one grid (LDS), the operations of k_smear_tuv in its order; area / (xu - xl) into res
template <int NP>
__device__ inline void smear_bin(const double* xs, const double* ys, int ystep, int np, int nx, double xl, double xu, double* res) {
  int lo = 0, hi = nx - 1;  // first k in [0, nx-1) with x[k+1] >= xl
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xs[mid + 1] < xl)
      lo = mid + 1;
    else
      hi = mid;
  }
  double area[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) area[q] = 0.0;
  for (int k = lo; k < nx - 1; ++k) {
    const double x0 = xs[k], x1 = xs[k + 1];
    if (x1 < xl) continue;
    if (x0 > xu) break;
    const double a1 = fmax(x0, xl);
    const double a2 = fmin(x1, xu);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      if (q < np) {
        const double y0 = ys[q * ystep + k];
        const double slope = (ys[q * ystep + k + 1] - y0) / (x1 - x0);
        const double b1 = y0 + slope * (a1 - x0);
        const double b2 = y0 + slope * (a2 - x0);
        area[q] = area[q] + (a2 - a1) * (b2 + b1) / 2;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) res[q] = area[q] / (xu - xl);
}

// l_wl_planck(T_K, wl_um), crt1d/spectra.py:42-53
__device__ inline double planck(double T_K, double wl_um) {
  constexpr double h = 6.62607015e-34, c = 299792458.0, k_B = 1.380649e-23;
  const double wl = wl_um * 1e-6;
  return (2 * h * c * c) / (wl * wl * wl * wl * wl * (exp(h * c / (wl * k_B * T_K)) - 1.0));
}

// np.interp(xv, lx, ly) with ly = l0 (+ l1): clamped outside, the slope form inside
__device__ inline double interp_light(const double* lx, const double* l0, const double* l1, int n, double xv) {
  auto ly = [&](int j) { return l1 ? l0[j] + l1[j] : l0[j]; };
  if (xv > lx[n - 1]) return ly(n - 1);
  if (xv < lx[0]) return ly(0);
  int lo = 0, hi = n - 1;  // last j with lx[j] <= xv
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lx[mid] <= xv)
      lo = mid;
    else
      hi = mid - 1;
  }
  if (lo == n - 1 || lx[lo] == xv) return ly(lo);
  const double f0 = ly(lo), f1 = ly(lo + 1);
  const double slope = (f1 - f0) / (lx[lo + 1] - lx[lo]);
  return slope * (xv - lx[lo]) + f0;
}

__global__ __launch_bounds__(SP_BLOCK) void k_spectral_prep(const SpecArgs a) {
  extern __shared__ __align__(16) double lds[];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int nx = a.nx, nb = a.nb, np = a.nprop, nq = np + 1, nxs = a.nxs, nlx = a.nlx;
  double* xs = lds;                     // [nx]
  double* ys = xs + nx;                 // [np][nx]
  double* xsi = ys + np * nx;           // [nxs]
  double* sis = xsi + nxs;              // [2][nxs]
  double* lxs = sis + 2 * nxs;          // [nlx]
  double* lys = lxs + nlx;              // [nlx]
  double* ed = lys + nlx;               // [nb + 1]
  double* sums = ed + (nb + 1);         // [nq][nb], the denominators last
  double* park = sums + nq * nb;        // [nq][SP_BLOCK]
  int* off = reinterpret_cast<int*>(park + nq * SP_BLOCK);  // [nb + 1]

  if (np == SP_MAXPROP) {
    const double* const g[4] = {a.x, a.y[0] + (long long)c * a.ystride[0], a.y[1] + (long long)c * a.ystride[1], a.y[2] + (long long)c * a.ystride[2]};
    double* const l[4] = {xs, ys, ys + nx, ys + 2 * nx};
    if (a.ystride[0] && a.ystride[1] && a.ystride[2])
      stage<4, true>(g, l, nx);
    else
      stage<4, false>(g, l, nx);
  } else {  // (the first entry: one spectrum per workgroup)
    const double* const g[2] = {a.x, a.y[0] + (long long)c * a.ystride[0]};
    double* const l[2] = {xs, ys};
    stage<2, true>(g, l, nx);
  }
  if (nxs) {
    const double* const g[3] = {a.x_si, a.si[0] + (long long)c * a.sistride[0], a.si[1] + (long long)c * a.sistride[1]};
    double* const l[3] = {xsi, sis, sis + nxs};
    if (a.sistride[0] && a.sistride[1])
      stage<3, true>(g, l, nxs);
    else
      stage<3, false>(g, l, nxs);
  }
  if (nlx) {
    const double* const g[2] = {a.light_x, a.light_y + (long long)(a.nlight == 1 ? 0 : c / a.light_group) * nlx};
    double* const l[2] = {lxs, lys};
    stage<2, false>(g, l, nlx);
  }
  for (int i = tid; i <= nb; i += SP_BLOCK) {
    ed[i] = a.edges[i];
    off[i] = a.sub_off[i];
  }
  for (int i = tid; i < nq * nb; i += SP_BLOCK) sums[i] = 0.0;
  __syncthreads();

  // the light table of CRT_LIGHT_TABLE: the first entry's own, or the column's SI_dr + SI_df on x_si
  const double* tlx = nlx ? lxs : xsi;
  const double* tl0 = nlx ? lys : sis;
  const double* tl1 = nlx ? nullptr : sis + nxs;
  const int tn = nlx ? nlx : nxs;

  const int nopt = off[nb], nitem = nopt + (nxs ? nb : 0);
  for (int c0 = 0; c0 < nitem; c0 += SP_BLOCK) {
    const int idx = c0 + tid;
    if (idx < nopt) {
      int lo = 0, hi = nb - 1;  // the band of item idx: last b with off[b] <= idx
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= idx)
          lo = mid;
        else
          hi = mid - 1;
      }
      const int b = lo, s = idx - off[b], nsub = off[b + 1] - off[b];
      // numpy.linspace(start, stop, nsub + 1): arange * step + start, last element forced to stop
      const double start = ed[b], stop = ed[b + 1];
      const double step = (stop - start) / (double)nsub;
      const double xl = (double)s * step + start;
      const double xu = (s + 1 == nsub) ? stop : (double)(s + 1) * step + start;
      double ysub[SP_MAXPROP];
      smear_bin<SP_MAXPROP>(xs, ys, nx, np, nx, xl, xu, ysub);
      double light = 1.0;
      if (a.light_kind == CRT_LIGHT_PLANCK) {
        double acc = 0.0;
        for (int i = 0; i < SP_NGL; ++i) acc = acc + a.glw[i] * planck(a.T_K, xl + (xu - xl) * a.glx[i]);
        light = (xu - xl) * acc;
      } else if (a.light_kind == CRT_LIGHT_TABLE) {
        light = interp_light(tlx, tl0, tl1, tn, (xl + xu) / 2);
      }
      const double w = (xu - xl) * light;
#pragma unroll
      for (int q = 0; q < SP_MAXPROP; ++q)
        if (q < np) park[q * SP_BLOCK + tid] = ysub[q] * w;
      park[np * SP_BLOCK + tid] = w;
      if (a.y_sub) a.y_sub[(long long)c * nopt + idx] = ysub[0];
    } else if (idx < nitem) {
      const int b = idx - nopt;
      double v[2];
      smear_bin<2>(xsi, sis, nxs, 2, nxs, ed[b], ed[b + 1], v);
      const double dwl = ed[b + 1] - ed[b];
      a.I_out[0][(long long)c * nb + b] = v[0] * dwl;
      a.I_out[1][(long long)c * nb + b] = v[1] * dwl;
    }
    __syncthreads();
    for (int p = tid; p < nq * nb; p += SP_BLOCK) {
      const int q = p / nb, b = p - q * nb;
      const int lo = max(off[b], c0), hi = min(off[b + 1], c0 + SP_BLOCK);
      if (lo < hi) {
        double acc = sums[p];
        const double* pk = park + q * SP_BLOCK - c0;
        for (int s = lo; s < hi; ++s) acc = acc + pk[s];
        sums[p] = acc;
      }
    }
    __syncthreads();
  }
  for (int p = tid; p < np * nb; p += SP_BLOCK) {
    const int q = p / nb, b = p - q * nb;
    a.out[q][(long long)c * nb + b] = sums[p] / sums[np * nb + b];
  }
}

struct Rule {
  double x[SP_NGL], w[SP_NGL];
};

const Rule& planck_rule() {
  static const Rule r = [] {
    Rule t;
    gauss_unit(SP_NGL, t.x, t.w);
    return t;
  }();
  return r;
}

// the checks both entries share; fills the fields they share.  CRT_OK with *nothing = true: nothing to do.
int bind_common(SpecArgs& a, int nprop, int nx, int ncol, const double* edges, int nb, const int32_t* sub_off, int light_kind, double T_K,
                int nxs, int nlx, bool* nothing) {
  *nothing = false;
  if (!edges || !sub_off || nx < 2 || ncol < 0 || nb < 0) return CRT_ERR_BAD_ARG;
  if (light_kind != CRT_LIGHT_UNIFORM && light_kind != CRT_LIGHT_PLANCK && light_kind != CRT_LIGHT_TABLE) return CRT_ERR_BAD_ARG;
  if (light_kind == CRT_LIGHT_PLANCK && !(T_K > 0.0)) return CRT_ERR_BAD_ARG;
  if (sub_off[0] != 0) return CRT_ERR_BAD_ARG;
  for (int i = 0; i < nb; ++i)
    if (sub_off[i + 1] <= sub_off[i]) return CRT_ERR_BAD_ARG;
  if (ncol == 0 || nb == 0) {
    *nothing = true;
    return CRT_OK;
  }
  if (nb > CRT_SPECTRA_MAX_NB || sub_off[nb] > CRT_SPECTRA_MAX_ITEMS) return CRT_ERR_UNSUPPORTED;
  a.nprop = nprop, a.nx = nx, a.nb = nb, a.nxs = nxs, a.nlx = nlx;
  a.light_kind = light_kind, a.light_group = 1, a.nlight = 1;
  a.T_K = T_K;
  a.edges = edges;
  a.x_si = nullptr, a.si[0] = a.si[1] = nullptr, a.sistride[0] = a.sistride[1] = 0;
  a.light_x = a.light_y = nullptr;
  a.I_out[0] = a.I_out[1] = nullptr;
  a.y_sub = nullptr;
  for (int q = 0; q < SP_MAXPROP; ++q) a.y[q] = nullptr, a.ystride[q] = 0, a.out[q] = nullptr;
  const Rule& r = planck_rule();
  for (int i = 0; i < SP_NGL; ++i) a.glx[i] = r.x[i], a.glw[i] = r.w[i];
  for (int i = 0; i <= nb; ++i) a.sub_off[i] = sub_off[i];
  return CRT_OK;
}

// LDS of one workgroup, the formula of the header
long long lds_doubles(const SpecArgs& a) {
  return (long long)a.nx * (1 + a.nprop) + 3LL * a.nxs + 2LL * a.nlx + (long long)(a.nprop + 1) * (a.nb + SP_BLOCK) + 2LL * (a.nb + 1);
}

int launch(const SpecArgs& a, int ncol, hipStream_t s) {
  const long long bytes = 8 * lds_doubles(a);
  if (bytes > CRT_SPECTRA_LDS_BYTES) return CRT_ERR_UNSUPPORTED;
  return launch_kernel(k_spectral_prep, dim3((unsigned)ncol), SP_BLOCK, (size_t)bytes, s, a);
}

bool stride_ok(int64_t stride, int n) { return stride == 0 || stride >= n; }

}  // namespace
}  // namespace crt

extern "C" {

int crt_hip_planck_nodes_f64(double* x, double* w) {
  if (!x || !w) return CRT_ERR_BAD_ARG;
  const crt::Rule& r = crt::planck_rule();
  for (int i = 0; i < crt::SP_NGL; ++i) x[i] = r.x[i], w[i] = r.w[i];
  return CRT_OK;
}

int crt_hip_avg_optical_prop_f64(const double* x, int32_t nx, const double* y, int32_t nspec, const double* edges, int32_t nb,
                                 const int32_t* sub_off, int32_t light_kind, double T_K, const double* light_x, int32_t nlx,
                                 const double* light_y, int32_t nlight, int32_t light_group, double* out, double* y_sub,
                                 crt_stream_t stream) {
  using namespace crt;
  if (!x || !y || !out) return CRT_ERR_BAD_ARG;
  const bool table = light_kind == CRT_LIGHT_TABLE;
  if (table) {
    if (!light_x || !light_y || nlx < 1 || nlight < 1 || light_group < 1) return CRT_ERR_BAD_ARG;
    if (nlight != 1 && nspec > 0 && (nspec - 1) / light_group >= nlight) return CRT_ERR_BAD_ARG;
  }
  SpecArgs a;
  bool nothing;
  const int st = bind_common(a, 1, nx, nspec, edges, nb, sub_off, light_kind, T_K, 0, table ? nlx : 0, &nothing);
  if (st != CRT_OK || nothing) return st;
  a.x = x;
  a.y[0] = y, a.ystride[0] = nx, a.out[0] = out;
  a.y_sub = y_sub;
  if (table) a.light_x = light_x, a.light_y = light_y, a.nlight = nlight, a.light_group = light_group;
  return launch(a, nspec, static_cast<hipStream_t>(stream));
}

int crt_hip_bands_from_spectra_f64(const double* x_opt, int32_t nx, const double* leaf_r, int64_t leaf_r_stride, const double* leaf_t,
                                   int64_t leaf_t_stride, const double* soil_r, int64_t soil_r_stride, const double* x_si, int32_t nxs,
                                   const double* SI_dr, int64_t si_dr_stride, const double* SI_df, int64_t si_df_stride, int32_t ncol,
                                   const double* edges, int32_t nb, const int32_t* sub_off, int32_t light_kind, double T_K, double* I_dr0,
                                   double* I_df0, double* leaf_r_out, double* leaf_t_out, double* soil_r_out, crt_stream_t stream) {
  using namespace crt;
  if (!x_opt || !leaf_r || !leaf_t || !soil_r || !x_si || !SI_dr || !SI_df) return CRT_ERR_BAD_ARG;
  if (!I_dr0 || !I_df0 || !leaf_r_out || !leaf_t_out || !soil_r_out) return CRT_ERR_BAD_ARG;
  if (nxs < 2 || nx < 2) return CRT_ERR_BAD_ARG;
  if (!stride_ok(leaf_r_stride, nx) || !stride_ok(leaf_t_stride, nx) || !stride_ok(soil_r_stride, nx) || !stride_ok(si_dr_stride, nxs) ||
      !stride_ok(si_df_stride, nxs))
    return CRT_ERR_BAD_ARG;
  SpecArgs a;
  bool nothing;
  const int st = bind_common(a, 3, nx, ncol, edges, nb, sub_off, light_kind, T_K, nxs, 0, &nothing);
  if (st != CRT_OK || nothing) return st;
  a.x = x_opt;
  a.y[0] = leaf_r, a.y[1] = leaf_t, a.y[2] = soil_r;
  a.ystride[0] = leaf_r_stride, a.ystride[1] = leaf_t_stride, a.ystride[2] = soil_r_stride;
  a.out[0] = leaf_r_out, a.out[1] = leaf_t_out, a.out[2] = soil_r_out;
  a.x_si = x_si;
  a.si[0] = SI_dr, a.si[1] = SI_df;
  a.sistride[0] = si_dr_stride, a.sistride[1] = si_df_stride;
  a.I_out[0] = I_dr0, a.I_out[1] = I_df0;
  return launch(a, ncol, static_cast<hipStream_t>(stream));
}

}  // extern "C"
