// The generalised plate model of leaf optics (include_ext/crt1d_hip_leafmodel.h): k_plate_leaf and its C entry.
//
// One lane per (column, band), bands along the lanes: blockIdx.x is the column, so its q = (N, C_0, ..) is wave-uniform, every spectrum
// load and every store is coalesced, and the kernel writes (2 + 2 nm) doubles per lane.  A workgroup is four waves -- 2 KB of every
// output row come from one CU, which is what the stores of rows that are no multiple of 128 B want (nb = 2151: 0.15 against 0.18 ms
// with one-wave workgroups) -- unless more than an eighth of such a grid's waves would own no band (nb = 300: three of eight), where
// it is one wave.  No lane's result depends on the choice.  Nothing is read or written outside [ncol] x [nb] (x rows 0 .. nm - 1 of a
// column's ntan): the only guard needed is band < nb.
#include "crt1d_hip_leafmodel.h"
#include "jac_schemes.hpp"

namespace crt {
namespace {

constexpr int PL_WAVE = 64, PL_BLOCK = 256;
constexpr int PL_MAXABS = CRT_PLATE_MAX_NABS;
constexpr int E1_NSER = 20;  // k < 1: the last term is below 1 / (20 * 20!) = 2e-20
constexpr int E1_NCF = 96;   // k >= 1: the truncation error at k = 1, where it is largest, is 1e-15 of e^k E1
constexpr double EULER_GAMMA = 0.57721566490153286061;

struct PlateArgs {
  int nb, nabs, ntan;
  long long q_stride;
  const double *kspec, *t_alpha, *t_90, *n, *q;
  double *leaf_r, *leaf_t, *d_leaf_r, *d_leaf_t;
};

struct E1Series {  // c[m] = (-1)^m / (m m!)
  double c[E1_NSER + 1];
  constexpr E1Series() : c{} {
    double f = 1.0;
    for (int m = 1; m <= E1_NSER; ++m) {
      f *= m;
      c[m] = ((m & 1) ? -1.0 : 1.0) / (m * f);
    }
  }
};

// E1(k) for 0 < k < 1: -gamma - ln k - sum_{m=1..20} (-k)^m / (m m!), the sum by Horner
__device__ __forceinline__ double e1_series(double k) {
  constexpr E1Series ser;
  double s = 0.0;
#pragma unroll
  for (int m = E1_NSER; m >= 1; --m) s = __builtin_fma(s, k, ser.c[m]);
  return (-EULER_GAMMA - log(k)) - s * k;
}

// e^k E1(k) for k >= 1: the continued fraction 1 / (k + 1 - 1 / (k + 3 - 4 / (k + 5 - ..))) cut after E1_NCF terms and evaluated from
// its tail as a ratio P / Q (f_m = b_m - m^2 / f_{m+1} = (b_m P - m^2 Q) / P), so that the loop has no division.  P grows like
// prod (k + 2 m): both are scaled by an exact power of two every 32 terms.
__device__ __forceinline__ double e1_scaled_cf(double k) {
  double P = k + (2 * E1_NCF + 1), Q = 1.0;
#pragma unroll
  for (int m = E1_NCF; m >= 1; --m) {
    const double Pn = __builtin_fma(k + (2 * m - 1), P, -((double)(m * m) * Q));  // three operations a term
    Q = P;
    P = Pn;
    if ((m & 31) == 1 && m != 1) {
      P = P * 0x1p-240;
      Q = Q * 0x1p-240;
    }
  }
  return Q * fast_rcp(P);
}

__device__ __forceinline__ Du dlog(Du a) { return Du{log(a.v), a.d * fast_rcp(a.v)}; }

// Stokes' pile of N - 1 inner plates (r, t; a, bN from them) under the top plate (Ra, Ta)
__device__ __forceinline__ void pile(Du Ra, Du Ta, Du r, Du t, Du a, Du bN, Du& leaf_r, Du& leaf_t) {
  const Du bN2 = bN * bN, a2 = a * a;
  const Du dn = a2 * bN2 - 1.0;
  const Du Rs = a * (bN2 - 1.0) / dn;
  const Du Ts = bN * (a2 - 1.0) / dn;
  const Du den = 1.0 - Rs * r;
  leaf_r = Ra + Ta * Rs * t / den;
  leaf_t = Ta * Ts / den;
}

__global__ __launch_bounds__(PL_BLOCK) void k_plate_leaf(PlateArgs A) {
  const long long c = blockIdx.x;
  const int band = blockIdx.y * blockDim.x + threadIdx.x;
  if (band >= A.nb) return;
  const double* const q = A.q + c * A.q_stride;  // wave-uniform
  const double N = q[0], invN = fast_rcp(N);
  double s = 0.0;
  for (int i = 0; i < A.nabs; ++i) s = s + q[1 + i] * A.kspec[(long long)i * A.nb + band];
  double k = s * invN;
  k = k < CRT_PLATE_K_MIN ? CRT_PLATE_K_MIN : (k > CRT_PLATE_K_MAX ? CRT_PLATE_K_MAX : k);  // (NaN stays NaN)

  // the plate transmittance and its derivative; each form of E1 only where a lane of the wave needs it
  const double em = fexp(-k);
  const bool small = k < 1.0;
  double e1s = 0.0, e1l = 0.0;
  if (__any(small)) e1s = e1_series(k);
  if (__any(!small)) e1l = em * e1_scaled_cf(k);
  const double E1 = small ? e1s : e1l;
  const Du tau{(1.0 - k) * em + (k * k) * E1, (2.0 * k) * E1 - 2.0 * em};

  // interfaces and single plates, d / dk carried
  const double nn = A.n[band], talf = A.t_alpha[band], t12 = A.t_90[band];
  const double ralf = 1.0 - talf, r12 = 1.0 - t12, t21 = t12 * fast_rcp(nn * nn), r21 = 1.0 - t21;
  const Du den = 1.0 - (r21 * r21) * (tau * tau);
  const Du Ta = (talf * t21) * tau / den;
  const Du Ra = ralf + r21 * (tau * Ta);
  const Du t = (t12 * t21) * tau / den;
  const Du r = r12 + r21 * (tau * t);
  const Du D = dsqrt((1.0 + r + t) * (1.0 + r - t) * (1.0 - r + t) * (1.0 - r - t));
  const Du r2 = r * r, t2 = t * t;
  const Du a = (1.0 + r2 - t2 + D) / (2.0 * r);
  const Du b = (1.0 - r2 + t2 + D) / (2.0 * t);
  const Du lnb = dlog(b);
  const double bNv = fexp((N - 1.0) * lnb.v);

  Du Lr, Lt;
  pile(Ra, Ta, r, t, a, Du{bNv, bNv * ((N - 1.0) * lnb.d)}, Lr, Lt);  // d / dk at fixed N
  const long long o = c * A.nb + band;
  A.leaf_r[o] = Lr.v;
  A.leaf_t[o] = Lt.v;
  if (!A.d_leaf_r) return;
  Du Nr, Nt;
  pile(mk(Ra.v), mk(Ta.v), mk(r.v), mk(t.v), mk(a.v), Du{bNv, bNv * lnb.v}, Nr, Nt);  // d / dN at fixed k: through bN alone
  const long long row = (long long)A.nb;
  double* const dr = A.d_leaf_r + c * A.ntan * row + band;
  double* const dt = A.d_leaf_t + c * A.ntan * row + band;
  const double kn = k * invN;
  dr[0] = Nr.d - kn * Lr.d;
  dt[0] = Nt.d - kn * Lt.d;
  for (int i = 0; i < A.nabs; ++i) {
    const double f = A.kspec[(long long)i * A.nb + band] * invN;
    dr[(1 + i) * row] = f * Lr.d;
    dt[(1 + i) * row] = f * Lt.d;
  }
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" int crt_hip_plate_leaf_f64(const crt_plate_leaf_model* m, const double* q, int64_t q_stride, double* leaf_r, double* leaf_t,
                                      int32_t ntan, double* d_leaf_r, double* d_leaf_t, crt_stream_t stream) {
  if (!m || m->ncol < 1 || m->nb < 1 || m->nabs < 1 || m->nabs > PL_MAXABS) return CRT_ERR_BAD_ARG;
  if (!m->kspec || !m->t_alpha || !m->t_90 || !m->n || !q || !leaf_r || !leaf_t) return CRT_ERR_BAD_ARG;
  const int nm = 1 + m->nabs;
  if (q_stride < nm || !d_leaf_r != !d_leaf_t) return CRT_ERR_BAD_ARG;
  if (d_leaf_r && (ntan < nm || ntan > CRT_SENSJAC_MAX_NTAN)) return CRT_ERR_BAD_ARG;
  const long long waves = ((long long)m->nb + PL_WAVE - 1) / PL_WAVE, wide = ((long long)m->nb + PL_BLOCK - 1) / PL_BLOCK;
  const int nthr = (wide * 4 - waves) * 8 <= wide * 4 ? PL_BLOCK : PL_WAVE;
  const long long ny = nthr == PL_BLOCK ? wide : waves;
  if (waves > 65535) return CRT_ERR_UNSUPPORTED;
  PlateArgs a;
  a.nb = m->nb, a.nabs = m->nabs, a.ntan = d_leaf_r ? ntan : 0, a.q_stride = q_stride;
  a.kspec = m->kspec, a.t_alpha = m->t_alpha, a.t_90 = m->t_90, a.n = m->n, a.q = q;
  a.leaf_r = leaf_r, a.leaf_t = leaf_t, a.d_leaf_r = d_leaf_r, a.d_leaf_t = d_leaf_t;
  const int st = launch_kernel(k_plate_leaf, dim3(m->ncol, (unsigned)ny), nthr, 0, static_cast<hipStream_t>(stream), a);
  if (st == CRT_OK) note_kernel("k_plate_leaf nabs=%d partials=%d block=%d", m->nabs, d_leaf_r ? 1 : 0, nthr);
  return st;
}
