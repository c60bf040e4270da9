// Leaf-inclination PDFs on the device (include/crt1d_hip_leaf.h): the front end of K0 for canopies described by g(theta_l) instead of a
// closed-form G(psi).  One launch turns (pdf_kind, pdf_param) of every column into the G table at the library's quadrature angles, G at the
// caller's angles and the mean leaf angle -- the three arrays a CRT_G_TABLE column brings (crt1d/leaf_angle.py:31-87; the reference has no
// G(psi) for the de Wit classes at all).
//
//   G(psi) = int_0^{pi/2} g(theta) A(psi, theta) dtheta
//   A      = cos(theta) cos(psi) (1 - 2 beta / pi) + (2 / pi) sin(theta) sin(psi) sin(beta),   beta = acos(min(1, cot(theta) cot(psi)))
//
// beta = 0 on [0, theta_k], theta_k = pi/2 - psi, and A ~ (theta - theta_k)^{3/2} above it: the two panels are integrated separately with
// the same NGL-point Gauss-Legendre rule, the upper one in s with theta = theta_k + psi s^2 (beta is s times a function of s^2, the Jacobian
// 2 psi s: the integrand is smooth in s).  cot(theta) cot(psi) is never formed: with d = theta - theta_k = psi s^2
//   1 - cot(theta) cot(psi) = -cos(theta + psi) / (sin(theta) sin(psi)) = sin(d) / (sin(theta) sin(psi)) =: u,
// exact to rounding where the difference from 1 would cancel, and beta = 2 asin(sqrt(u / 2)), sin(beta) = 2 sqrt(u / 2) sqrt(1 - u / 2).
// psi = 0 has no upper panel (u would be 0 / 0): G = int g cos(theta).  NGL = 48 is the smallest multiple of 8 that keeps ten times the
// margin to the 1e-11 bar of DESIGN.md 3.11 (worst case: uniform / planophile at psi = (1 - 6e-6) pi/2, where u = d / (theta_k + d) has a
// pole at s = i sqrt(theta_k / psi) next to the panel; tests/test_leaf_pdf_cpu.py).
#include <hip/hip_runtime.h>
#include <math.h>

#include <mutex>
#include <vector>

#include "crt1d_hip_leaf.h"
#include "crt_internal.hpp"

namespace crt {
namespace {

constexpr int NGL_G = CRT_LEAF_NGL;
constexpr int NGL_M = CRT_LEAF_NMLA;
constexpr int LEAF_BLOCK = 192;  // three waves: the 137 nodes and up to 55 caller angles in one pass
constexpr double HALF_PI = 1.57079632679489661923;
constexpr double TWO_OVER_PI = 0.63661977236758134308;

struct LeafRule {
  double x[NGL_G], w[NGL_G];    // unit interval
  double xm[NGL_M], wm[NGL_M];
};

__constant__ LeafRule lr;

struct LeafArgs {
  int ncol, npsi;               // npsi: caller angles per column that are evaluated (0 when g_at_psi is NULL)
  const int32_t* kind;
  const double* param;          // [ncol][2]
  const double* psi;            // [ncol][npsi]
  double* g_table;              // [ncol][CRT_NQ]
  double* g_at_psi;             // [ncol][npsi]
  double* mla;                  // [ncol] or nullptr
  double node_psi[CRT_NQ];      // crt_hip_quad_nodes(mu_s): the same bits a host-sampled table is taken at
};

// one column's PDF: g(theta) from sin / cos of theta
struct Pdf {
  int kind;
  double p0, p1, scale;  // ELLIPSOIDAL: x^2, -, 2 x^3 / l;  TRIG: a, b, 2 / pi
};

__device__ inline Pdf pdf_of(int kind, double a, double b) {
  Pdf f;
  f.kind = kind;
  f.p0 = a;
  f.p1 = b;
  f.scale = TWO_OVER_PI;
  if (kind == CRT_LEAF_PDF_ELLIPSOIDAL) {
    const double l = a == 1.0 ? 2.0 : ellipsoidal_p2(a);  // leaf_angle.py:66-73, the normalisation of G_ellipsoidal
    f.p0 = a * a;
    f.scale = 2.0 * a * a * a / l;
  }
  return f;
}

__device__ inline double pdf_eval(const Pdf& f, double st, double ct) {
  switch (f.kind) {
    case CRT_LEAF_PDF_SPHERICAL: return st;
    case CRT_LEAF_PDF_ELLIPSOIDAL: {
      const double d = ct * ct + f.p0 * st * st;
      return f.scale * st / (d * d);
    }
    default: {
      const double c2 = 2.0 * ct * ct - 1.0;
      const double c4 = 2.0 * c2 * c2 - 1.0;
      return f.scale * (1.0 + f.p0 * c2 + f.p1 * c4);
    }
  }
}

__device__ inline double G_of_pdf(const Pdf& f, double psi) {
  double sp, cp;
  sincos(psi, &sp, &cp);
  const double tk = HALF_PI - psi;
  double lo = 0.0, hi = 0.0;
  for (int i = 0; i < NGL_G; ++i) {
    double st, ct;
    sincos(tk * lr.x[i], &st, &ct);
    lo += lr.w[i] * pdf_eval(f, st, ct) * ct;
  }
  lo *= cp * tk;
  if (sp > 0.0) {
    for (int i = 0; i < NGL_G; ++i) {
      const double s = lr.x[i];
      const double d = psi * s * s;
      double st, ct;
      sincos(tk + d, &st, &ct);
      const double ss = st * sp, cc = ct * cp;
      const double u = fmin(1.0, sin(d) / ss);
      const double h = sqrt(0.5 * u);
      const double beta = 2.0 * asin(h);
      const double sb = 2.0 * h * sqrt(1.0 - 0.5 * u);
      const double A = cc + TWO_OVER_PI * (ss * sb - cc * beta);
      hi += lr.w[i] * (2.0 * s) * pdf_eval(f, st, ct) * A;
    }
    hi *= psi;
  }
  return lo + hi;
}

// One workgroup per column, one thread per target angle (the CRT_NQ nodes, then the column's npsi angles; the workgroup loops when there
// are more targets than its 192 threads).  Wave 0 forms mla first, one node of its rule per lane.
__global__ __launch_bounds__(LEAF_BLOCK) void k_g_from_pdf(const LeafArgs a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const Pdf f = pdf_of(a.kind[c], a.param[2 * (long long)c], a.param[2 * (long long)c + 1]);
  if (a.mla && tid < NGL_M) {
    const double th = HALF_PI * lr.xm[tid];
    double st, ct;
    sincos(th, &st, &ct);
    const double m = wave_sum_all(lr.wm[tid] * th * pdf_eval(f, st, ct));
    if (tid == 0) a.mla[c] = HALF_PI * m * (180.0 / 3.14159265358979323846);
  }
  const int ntarget = CRT_NQ + a.npsi;
  for (int t = tid; t < ntarget; t += LEAF_BLOCK) {
    if (t < CRT_NQ) {
      a.g_table[(long long)c * CRT_NQ + t] = G_of_pdf(f, a.node_psi[t]);
    } else {
      const long long o = (long long)c * a.npsi + (t - CRT_NQ);
      a.g_at_psi[o] = G_of_pdf(f, a.psi[o]);
    }
  }
}

LeafRule h_lr;
std::once_flag h_lr_once;
std::mutex lr_mu;
bool lr_inited[64];

const LeafRule& host_rule() {
  std::call_once(h_lr_once, [] {
    gauss_unit(NGL_G, h_lr.x, h_lr.w);
    gauss_unit(NGL_M, h_lr.xm, h_lr.wm);
  });
  return h_lr;
}

// the rule in constant memory, once per device (like init_quadrature: a synchronising upload on the first call)
int init_leaf_rule(hipStream_t s) {
  const LeafRule& h = host_rule();
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return CRT_ERR_LAUNCH;
  if (dev < 0 || dev >= 64) return CRT_ERR_UNSUPPORTED;
  std::lock_guard<std::mutex> lk(lr_mu);
  if (!lr_inited[dev]) {
    if (hipMemcpyToSymbolAsync(HIP_SYMBOL(lr), &h, sizeof(LeafRule), 0, hipMemcpyHostToDevice, s) != hipSuccess) return CRT_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return CRT_ERR_LAUNCH;
    lr_inited[dev] = true;
  }
  return CRT_OK;
}

// (2/pi)(1 + a u + b (2 u^2 - 1)) >= 0 for u = cos(2 theta) in [-1, 1]: both ends, and the vertex when it is an interior minimum
bool trig_pdf_ok(double a, double b) {
  if (!std::isfinite(a) || !std::isfinite(b)) return false;
  if (!(1.0 + a + b >= 0.0) || !(1.0 - a + b >= 0.0)) return false;
  if (b > 0.0 && fabs(a) < 4.0 * b && !(1.0 - b - a * a / (8.0 * b) >= 0.0)) return false;
  return true;
}

bool pdf_ok(int kind, double p0, double p1) {
  switch (kind) {
    case CRT_LEAF_PDF_SPHERICAL: return true;
    case CRT_LEAF_PDF_ELLIPSOIDAL: return p0 >= CRT_LEAF_X_MIN && p0 <= CRT_LEAF_X_MAX;  // (false for NaN)
    case CRT_LEAF_PDF_TRIG: return trig_pdf_ok(p0, p1);
    default: return false;
  }
}

}  // namespace
}  // namespace crt

extern "C" {

int crt_hip_leaf_pdf_nodes_f64(double* x, double* w, double* x_mla, double* w_mla) {
  if (!!x != !!w || !!x_mla != !!w_mla) return CRT_ERR_BAD_ARG;
  const crt::LeafRule& h = crt::host_rule();
  for (int i = 0; x && i < crt::NGL_G; ++i) x[i] = h.x[i], w[i] = h.w[i];
  for (int i = 0; x_mla && i < crt::NGL_M; ++i) x_mla[i] = h.xm[i], w_mla[i] = h.wm[i];
  return CRT_OK;
}

int crt_hip_g_from_pdf_f64(const int32_t* pdf_kind, const double* pdf_param, int32_t ncol, double mu_s, const double* psi, int32_t npsi,
                           double* g_table, double* g_at_psi, double* mla, crt_stream_t stream) {
  using namespace crt;
  if (!pdf_kind || !pdf_param || !g_table) return CRT_ERR_BAD_ARG;
  if (ncol < 0 || npsi < 0 || !(mu_s > 0.0 && mu_s < 1.0)) return CRT_ERR_BAD_ARG;
  if (npsi > 0 && !psi) return CRT_ERR_BAD_ARG;
  if (ncol == 0) return CRT_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the descriptors, read back and checked before anything is launched
  std::vector<int32_t> hk((size_t)ncol);
  std::vector<double> hp((size_t)ncol * 2);
  if (hipMemcpyAsync(hk.data(), pdf_kind, hk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(hp.data(), pdf_param, hp.size() * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return CRT_ERR_LAUNCH;
  for (int c = 0; c < ncol; ++c)
    if (!pdf_ok(hk[c], hp[2 * (size_t)c], hp[2 * (size_t)c + 1])) return CRT_ERR_BAD_ARG;
  const int st = init_leaf_rule(s);
  if (st != CRT_OK) return st;
  LeafArgs a;
  a.ncol = ncol;
  a.npsi = g_at_psi ? npsi : 0;
  a.kind = pdf_kind;
  a.param = pdf_param;
  a.psi = psi;
  a.g_table = g_table;
  a.g_at_psi = g_at_psi;
  a.mla = mla;
  host_quad_nodes(mu_s, a.node_psi);
  return launch_kernel(k_g_from_pdf, dim3((unsigned)ncol), LEAF_BLOCK, 0, s, a);
}

}  // extern "C"
