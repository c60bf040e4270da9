// K0: per-column precompute for the batched canopy-RT solvers (gfx950).
//
// Everything the reference computes once per `solve_*` call before its band loop -- K_b, mu_bar,
// the G integrals, tau_d of every layer/level, exp(-K_b lai) -- is band-independent, so it is
// computed once per column here (one 128-thread workgroup per column) and written as a small
// record into the caller's workspace; the solve kernels stage it into LDS.  The 2s record is
// formed by the functions of col_record.hpp, which the 2s k_pipe also calls to build its
// column's record itself (solve_closed.hip).
//
// The reference evaluates its integrals with adaptive QUADPACK (scipy.integrate.quad) over
// arbitrary Python callables.  On device the integrals use FIXED nodes (col_record.hpp):
//   * tau_d and mu_bar: 6 panels x 16-point Gauss-Legendre on psi in [0, pi/2], panel edges at decades of pi/2 - psi toward
//       pi/2 where exp(-G L / cos psi) has its essential singularity: tau_d <= 1e-12 relative, mu_bar <= 1.5e-12, and 1 - tau_d
//       <= 2.3e-12 for L in [1e-3, 12] on every leaf-angle class but one -- the figures per class and L are at PAN_EDGE below
//       (the reference's own quad error is up to ~3e-8 in tau_d).
//   * G_int_1, G_int_2: 16-point Gauss-Legendre each, in psi (dm = -sin psi dpsi).
//   * '9sky': the reference's own 9 fixed angles                 (common.py:40-53)
#include <math.h>

#include <mutex>

#include "col_record.hpp"

namespace crt {

namespace {

constexpr int NPAN = 6;
// Panel edges in t = pi/2 - psi, as fractions of pi/2: decades towards psi = pi/2, where e^{-G L / cos psi} has its boundary layer (at
// cos psi ~ G(pi/2) L), and a split of the wide end, where 1/G of an ellipsoidal distribution with small x has its own structure at
// psi -> 0 (mu_bar).  The geometric 4x grading of rounds 1-2 gave 1e-8 in 1 - tau_d at L = 3e-4 -- n79 divides 1 - tau_d(dlai) by dlai,
// and its per-leaf-area absorption on fine ragged grids was the one output that saw it -- and 8e-10 in mu_bar at x = 0.2.
//
// What the rule delivers is measured by tests/test_quadrature_domain_cpu.py (the rule rebuilt on the host from crt_hip_quad_nodes,
// against converged 30-digit mpmath integrals) and asserted there at twice these figures; the table per class and L is in DESIGN 3.2.
// Classes: horizontal, spherical, vertical, ellipsoidal and ellipsoidal-approx with x in [0.2, 10], Bonan with chi_l in [-0.4, 0.6].
// Relative error of 1 - tau_d(L):
//   L in [1e-3, 12]   <= 1.8e-12 on every class but Bonan chi_l = 0.6 (G(pi/2) = 0.0014: 9.8e-11 at 1e-3, 3.6e-12 at 1e-2)
//   L = 3e-4          <= 5.8e-13, but 3.2e-11 for x = 10 and 3.5e-10 for Bonan chi_l = 0.6
//   L = 1e-4          <= 3.4e-11, but 4.8e-10 for x = 10 and 3.0e-10 for Bonan chi_l = 0.6
//   L < 1e-4          the layer at cos psi ~ G(pi/2) L falls inside the finest panel, [0, 1e-4] pi/2: 1.2e-8 at 1e-5, 1.2e-7 at 1e-6
//                     (in tau_d itself that is 1e-13)
// tau_d <= 1.0e-12 and mu_bar <= 1.5e-12 (Bonan chi_l = 0.6; 2.8e-13 at x = 0.2, 1.5e-14 elsewhere) for L in [1e-6, 12].  The edges came
// from a scan over ellipsoidal-approx x in {0.2, 0.3, 0.96, 3} only, where 1 - tau_d <= 2.3e-12 for L in [3e-4, 20].  No other six
// edges on a half-decade grid hold 2.3e-12 from 3e-4 on all ten classes (best: 6.9e-12, with mu_bar at 1.3e-10), so the edges stay
// (they are what crt_hip_quad_nodes exports: ABI) and the claim is stated per class.
constexpr double PAN_EDGE[NPAN + 1] = {0.0, 1e-4, 1e-3, 1e-2, 0.1, 0.6, 1.0};
static_assert(NPAN * NGL == NQT, "tau_d rule size");
static_assert(2 * NGL == NQG, "4s rule size");

QuadConst h_qc;
std::once_flag h_once;
bool dev_inited[64] = {};
std::mutex dev_mu;

// Gauss-Legendre nodes/weights on [-1, 1] by Newton iteration on P_n
void gauss_legendre(int n, double* x, double* w) {
  for (int i = 0; i < n; ++i) {
    double z = cos(M_PI * (i + 0.75) / (n + 0.5));
    double pp = 0;
    for (int it = 0; it < 100; ++it) {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 1; j <= n; ++j) {
        double p3 = p2;
        p2 = p1;
        p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
      }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      double dz = p1 / pp;
      z -= dz;
      if (fabs(dz) < 1e-16) break;
    }
    // ascending order
    x[n - 1 - i] = z;
    w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
  }
}

void build_host_tables() {
  gauss_legendre(NGL, h_qc.gx, h_qc.gw);
  const double T = M_PI / 2;
  // panel edges in t = pi/2 - psi
  double edge[NPAN + 1];
  for (int k = 0; k <= NPAN; ++k) edge[k] = T * PAN_EDGE[k];
  int q = 0;
  for (int k = 0; k < NPAN; ++k) {
    const double a = edge[k], b = edge[k + 1];
    for (int i = 0; i < NGL; ++i, ++q) {
      const double t = a + (h_qc.gx[i] + 1.0) * (b - a) / 2;
      const double psi = T - t;
      h_qc.psi[q] = psi;
      // cos(pi/2 - t) = sin t: keeps full relative accuracy next to pi/2
      h_qc.cs[q] = sin(t);
      h_qc.sn[q] = cos(t);
      h_qc.w[q] = h_qc.gw[i] * (b - a) / 2;
      h_qc.w2sc[q] = 2.0 * h_qc.w[q] * h_qc.sn[q] * h_qc.cs[q];
    }
  }
  for (int i = 0; i < CRT_NQ_9SKY; ++i) {
    const double psi = (5.0 + 10.0 * i) * (M_PI / 180.0);  // math.radians(sza), common.py:46-48
    h_qc.cs9[i] = cos(psi);
    h_qc.sn9[i] = sin(psi);
    h_qc.sc9[i] = sin(psi) * cos(psi);
  }
}

// 4s nodes: interval 0 = psi in [acos(mu_s), pi/2] (m in [0, mu_s]), interval 1 = [0, acos(mu_s)]
__host__ __device__ inline void g4_interval(double mu_s, int iv, double& lo, double& hi) {
  const double ps = acos(mu_s);
  if (iv == 0) {
    lo = ps;
    hi = 1.57079632679489661923;
  } else {
    lo = 0.0;
    hi = ps;
  }
}

constexpr int K0_BLOCK = 128;
constexpr int BL_UNIF_MAX_NZ = 512;
constexpr int BL_CHUNK = 16;
static_assert(K0_BLOCK == 8 * BL_CHUNK && CRT_NQ_TAU % 8 == 0, "bl chunk reduction layout");

__device__ inline double tau_d_quad(const double* kq, double L) {
  double s = 0.0;
  for (int q = 0; q < NQT; ++q) s += qc.w2sc[q] * fexp(-kq[q] * L);
  return s;
}

// 1 - tau_d(L) = 2 int (1 - e^{-K_b(psi) L}) sin cos dpsi  (the weights 2 w sin cos integrate to one): every term by expm1, so that the
// result keeps its RELATIVE accuracy at small L, where tau_d -> 1.  n79 divides (1 - tau_d(dlai)) by dlai afterwards (_solve_n79.py:146,
// 154-155): formed as 1 - tau_d the ~3e-13 by which two quadrature rules differ in tau_d became ~2e-8 at dlai ~ 3e-4 (round 2).
__device__ inline double one_minus_tau_d_quad(const double* kq, double L) {
  double s = 0.0;
  for (int q = 0; q < NQT; ++q) s -= qc.w2sc[q] * fexpm1(-kq[q] * L);
  return s;
}

__device__ inline double tau_d_9sky(const double* k9, double L) {
  double s = 0.0;
  for (int i = 0; i < CRT_NQ_9SKY; ++i) s += fexp(-k9[i] * L) * qc.sc9[i];
  return s * (2.0 * 0.17453292519943295);  // * 2 radians(10), common.py:51
}

// zq_pa: linear interpolation of the interface fluxes back to cumulative LAI L (:357-362, np.interp semantics) on the computational
// interfaces xi[0 .. M]: interface index (0 = ground) of the node above L, and the weight
struct ZqPaInterp {
  double k, w;
};
__device__ inline ZqPaInterp zqpa_interp(const double* xi, int M, double L) {
  int lo = 0;
  for (int i = 1; i < M; ++i)
    if (xi[i] <= L) lo = i;
  const double x0 = xi[lo], x1 = xi[lo + 1];
  double w = (L - x0) / (x1 - x0);
  if (L >= x1) w = 1.0;  // at or beyond the last node: np.interp returns fp[-1]
  return {(double)(M - lo), w};
}
// zq_pa: beam fraction seen by computational layer li = j+1 (:164-168): f_sl[li] = exp(-K_b xi[M+1-li])
__device__ inline double zqpa_fsl(double Kb, const double* xi, int M, int j) { return (j < M) ? fexp(-Kb * xi[M - j]) : 0.0; }

// n79: 1 - td of a layer of thickness dl
__device__ inline double n79_omtd(int method, const double* k9, const double* kq, double dl) {
  return (method == CRT_TAU_D_9SKY) ? 1.0 - tau_d_9sky(k9, dl) : one_minus_tau_d_quad(kq, dl);  // 1 - td, :53
}
// n79: what follows the sun in the layer between L = lai[j] and Ln = lai[j+1]: 1 - tb, fs / (fs dlai), 1 / (fs dlai), (1 - fs) / ((1 - fs) dlai)
struct N79Sun {
  double omtb, fsisl, isl, fhish;
};
__device__ inline N79Sun n79_sun(double Kb, double L, double Ln, bool unif, double dlu) {
  const double dl = L - Ln;                                // :40
  const double omtb = -fexpm1(-Kb * (unif ? dlu : dl));    // 1 - tb, :45
  const double fs = fexp(-Kb * ((L + Ln) / 2));            // :57-58
  const double isl = 1.0 / (fs * dl);                      // :154
  const double ish = 1.0 / ((1.0 - fs) * dl);              // :155
  return {omtb, fs * isl, isl, (1.0 - fs) * ish};
}

// CAN (sun-angle series, SeriesArgs in crt_internal.hpp): the canopy record only -- every entry that does not follow the sun, in the
// record's own layout with a stride of can_len, the sun's slots left as placeholders for k_colsun's records, and for zq_pa the cumulative
// LAI of the computational interfaces behind it.  The per-step kernel is k_colpre<false>.
template <bool CAN>
__global__ __launch_bounds__(K0_BLOCK) void k_colpre(ColArgs a) {
  __shared__ double kq[NQT];    // K_b(psi_q) = G/cos at the tau_d nodes
  __shared__ double pmb[NQT];   // mu_bar terms, later tau_d(dlai_mean) terms
  __shared__ double pg[NQG];    // G-integral terms
  __shared__ double k9[CRT_NQ_9SKY];
  __shared__ double sh_kb, sh_dlm, sh_dl, sh_tdu;
  __shared__ int sh_unif;
  __shared__ double xis[104];  // zq_pa: cumulative LAI of the computational interfaces
  // bl only (dynamic, so that the other schemes keep 16 workgroups per CU): the 96 quadrature terms of 16 levels, the sums
  // over groups of 12 nodes, tau_d of every level
  extern __shared__ double bl_lds[];
  double* bl_terms = bl_lds;
  double* bl_gsum = bl_terms + NQT * (BL_CHUNK + 1);
  double* bl_td = bl_gsum + 8 * BL_CHUNK;

  const int c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nz = a.nz;
  const ColIn in = col_in(a, c);  // (the angle-independent part of G once per thread)
  const int kind = in.kind;
  const double param = in.param, gden = in.gden;
  const double* tab = in.tab;
  const double* lai = in.lai;
  const int reclen = CAN ? can_len(a.scheme, nz) : rec_len(a.scheme, nz);
  double* rec = a.ws + (long long)c * reclen;

  for (int q = tid; q < NQT; q += K0_BLOCK) col_node(in, q, kq[q], pmb[q]);
  if (a.scheme == CRT_SCHEME_4S && tid < NQG) {
    const int iv = tid / NGL, i = tid % NGL;
    double lo, hi;
    g4_interval(a.mu_s, iv, lo, hi);
    const double p = lo + (qc.gx[i] + 1.0) * (hi - lo) / 2;
    const double g = tab ? tab[NQT + tid] : G_eval(kind, param, gden, cos(p), sin(p));
    pg[tid] = qc.gw[i] * (hi - lo) / 2 * g * sin(p);
  }
  if (tid < CRT_NQ_9SKY) k9[tid] = col_node9(in, tid);
  __syncthreads();

  // ---- header: wave 0, reductions by shuffles ----
  if (wave == 0) {
    ColSun sun;
    if constexpr (CAN) {  // placeholders in the sun's header slots (k_colsun's record supplies them): cos psi = 1, G = 0, K_b = 0
      sun.cs = 1.0;
      sun.G = 0.0;
      sun.Kb = 0.0;
    } else {
      sun = col_sun(a, c, in);
    }
    const ColDl dls = col_dl(in, nz, lane);
    const double Kb = sun.Kb;
    double mubar = 0.0, g1 = 0.0, g2 = 0.0, dlm = 0.0;
    if (a.scheme == CRT_SCHEME_2S) mubar = col_mubar(pmb[lane], lane < NQT - 64 ? pmb[64 + lane] : 0.0, lane);
    if (a.scheme == CRT_SCHEME_4S) {
      g1 = wave_sum64(lane < NGL ? pg[lane] : 0.0);
      g2 = wave_sum64(lane < NGL ? pg[NGL + lane] : 0.0);
    }
    if (a.scheme == CRT_SCHEME_ZQ) dlm = fabs(wave_sum64(dls.dsum) / wave_sum64(dls.dcnt));
    if (lane == 0) {
      const double tpsi = a.scheme == CRT_SCHEME_ZQ && !CAN ? fexp(-Kb * dlm) : 0.0;  // _solve_zq.py:52
      const double cos2 = a.scheme == CRT_SCHEME_2S ? col_cos2(a.mla[c]) : 0.0;
      col_header(rec, sun, dls, mubar, g1, g2, dlm, tpsi, cos2, lai[0], nz);
      sh_kb = Kb;
      sh_dlm = dlm;
      sh_dl = dls.dl;
      sh_unif = dls.unif ? 1 : 0;
    }
  }
  __syncthreads();
  const double Kb = sh_kb;
  if (a.scheme == CRT_SCHEME_ZQ_PA) {
    // computational grid of M equal layers (_solve_zq_pa.py:94-100): tau_d(LAI/M) (:176), exp(-K_b LAI/M) (:174)
    const int M = zqpa_M(nz);
    const double Lm = lai[0] / M;
    for (int q = tid; q < NQT; q += K0_BLOCK) pmb[q] = qc.w2sc[q] * fexp(-kq[q] * Lm);
    __syncthreads();
    if (wave == 0) {
      const double t = wave_sum64(pmb[lane] + (lane < NQT - 64 ? pmb[64 + lane] : 0.0));
      if (lane == 0) {
        rec[S_TAUI] = t;
        if constexpr (!CAN) rec[S_TPSI] = fexp(-Kb * Lm);
        // xi[i] = cumulative LAI of computational interface i from the top, built by repeated addition as np.cumsum
        // does (_solve_zq_pa.py:159): xi[0] = 0, xi[i] = xi[i-1] + Lm
        double sacc = 0.0;
        xis[0] = 0.0;
        for (int i = 1; i <= M; ++i) {
          sacc += Lm;
          xis[i] = sacc;
        }
        if constexpr (CAN)
          for (int i = 0; i <= M; ++i) rec[rec_len(a.scheme, nz) + i] = xis[i];
      }
    }
    __syncthreads();
  }
  if (a.scheme == CRT_SCHEME_ZQ) {
    // tau_i = tau_d(dlai_mean), always 'quad' (_solve_zq.py:51): one node per thread, then the same tree reduction
    const double dlm = sh_dlm;
    for (int q = tid; q < NQT; q += K0_BLOCK) pmb[q] = qc.w2sc[q] * fexp(-kq[q] * dlm);
    __syncthreads();
    if (wave == 0) {
      const double t = wave_sum64(pmb[lane] + (lane < NQT - 64 ? pmb[64 + lane] : 0.0));
      if (lane == 0) rec[S_TAUI] = t;
    }
  }

  // n79 on an equal-dLAI column (S_UNIF): one layer transmittance pair (tb, td) serves every layer, so tau_d is
  // evaluated once, one node per thread, instead of once per level; the solve kernels rely on the three layer
  // vectors (tb, td, 1/(1-td)) being constant when S_UNIF is set (TriN79U, tri_schemes.hpp).
  const bool n79u = a.scheme == CRT_SCHEME_N79 && sh_unif != 0 && nz >= 3;
  if (n79u) {
    const double dl = sh_dl;
    // (sh_tdu holds 1 - tau_d: see one_minus_tau_d_quad; '9sky' has no such form -- its nine weights do not sum to one -- and is 1 - tau_d
    //  as the reference computes it)
    if (a.tau_d_method == CRT_TAU_D_9SKY) {
      if (tid == 0) sh_tdu = 1.0 - tau_d_9sky(k9, dl);
    } else {
      for (int q = tid; q < NQT; q += K0_BLOCK) pmb[q] = -qc.w2sc[q] * fexpm1(-kq[q] * dl);
      __syncthreads();
      if (wave == 0) {
        const double t = wave_sum64(pmb[lane] + (lane < NQT - 64 ? pmb[64 + lane] : 0.0));
        if (lane == 0) sh_tdu = t;
      }
    }
    __syncthreads();
  }
  // bl on an equal-dLAI column: tau_d is needed at every level L_j = (nz-1-j) dl.  Instead of 96 exponentials per level
  // (the kernel's whole cost: 5760 fp64 exps per column), thread q carries E_q^m = exp(-K_q dl)^m down the levels by one
  // multiplication per level (drift <= nz ulp).  The 96 terms of a level are summed through LDS, 16 levels at a time:
  // thread q writes its 16 terms (row stride 17: conflict-free both ways), thread (g, jj) adds the 12 nodes of group g for
  // level jj, the first 16 threads add the 8 group sums.  (A wave reduction per level -- 60 x DPP -- cost as much as the
  // exponentials it replaced.)
  const bool blu = a.scheme == CRT_SCHEME_BL && sh_unif != 0 && nz <= BL_UNIF_MAX_NZ;
  if (blu) {
    const double dl = sh_dl;
    const bool on = tid < NQT;
    const double E = on ? fexp(-kq[on ? tid : 0] * dl) : 0.0;
    const double w = on ? qc.w2sc[tid] : 0.0;
    double P = 1.0;  // level nz-1: L = 0
    for (int jtop = nz - 1; jtop >= 0; jtop -= BL_CHUNK) {  // levels jtop, jtop-1, ... (chunk position jj <-> level jtop - jj)
      if (on) {
#pragma unroll
        for (int jj = 0; jj < BL_CHUNK; ++jj) {
          bl_terms[tid * (BL_CHUNK + 1) + jj] = w * P;
          P *= E;
        }
      }
      __syncthreads();
      {
        const int jj = tid & (BL_CHUNK - 1), g = tid / BL_CHUNK;  // 128 threads = 8 groups x 16 levels
        double acc = 0.0;
        for (int q = g * (NQT / 8); q < (g + 1) * (NQT / 8); ++q) acc += bl_terms[q * (BL_CHUNK + 1) + jj];
        bl_gsum[g * BL_CHUNK + jj] = acc;
      }
      __syncthreads();
      if (tid < BL_CHUNK && jtop - tid >= 0) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += bl_gsum[g * BL_CHUNK + tid];
        bl_td[jtop - tid] = t;
      }
      // (bl_terms / bl_gsum are rewritten only after the next chunk's first barrier resp. after its second one)
      __syncthreads();
    }
  }
  double* v = rec + REC_HDR;
  for (int j = tid; j < nz; j += K0_BLOCK) {
    const double L = lai[j];
    if constexpr (CAN) {
      switch (a.scheme) {
        case CRT_SCHEME_ZQ:
          break;
        case CRT_SCHEME_ZQ_PA: {
          const int M = zqpa_M(nz);
          const ZqPaInterp ip = zqpa_interp(xis, M, L);
          v[2 * nz + j] = ip.k;
          v[3 * nz + j] = ip.w;
          break;
        }
        case CRT_SCHEME_BL:
          v[j] = L;
          v[2 * nz + j] = blu ? bl_td[j] : tau_d_quad(kq, L);  // _solve_bl.py:35-37
          break;
        case CRT_SCHEME_N79: {
          double omtd = 1;  // 1 - td
          if (j + 1 < nz) omtd = n79u ? sh_tdu : n79_omtd(a.tau_d_method, k9, kq, L - lai[j + 1]);
          v[2 * nz + j] = omtd;
          v[6 * nz + j] = 1.0 / omtd;
          break;
        }
        default:
          v[j] = L;
          break;
      }
      continue;
    }
    const double ekl = col_ekl(Kb, L);
    switch (a.scheme) {
      case CRT_SCHEME_ZQ:
        v[j] = ekl;
        break;
      case CRT_SCHEME_ZQ_PA: {
        const int M = zqpa_M(nz);
        // beam fraction seen by computational layer li = j+1 (:164-168): f_sl[li] = exp(-K_b xi[M+1-li])
        v[j] = zqpa_fsl(Kb, xis, M, j);
        v[nz + j] = ekl;
        const ZqPaInterp ip = zqpa_interp(xis, M, L);
        v[2 * nz + j] = ip.k;
        v[3 * nz + j] = ip.w;
        break;
      }
      case CRT_SCHEME_BL:
        v[j] = L;
        v[nz + j] = ekl;
        v[2 * nz + j] = blu ? bl_td[j] : tau_d_quad(kq, L);  // _solve_bl.py:35-37
        break;
      case CRT_SCHEME_N79: {
        v[j] = ekl;  // tbcum  _solve_n79.py:46
        double omtd = 1;  // 1 - td
        N79Sun ns = {1, 0, 0, 0};
        if (j + 1 < nz) {
          const double Ln = lai[j + 1];
          omtd = n79u ? sh_tdu : n79_omtd(a.tau_d_method, k9, kq, L - Ln);
          ns = n79_sun(Kb, L, Ln, n79u, sh_dl);
        }
        // what the level loops multiply by, formed once per column (tri_schemes.hpp, TriN79): 1 - tb, 1 - td, fs / (fs dlai), 1 / (fs dlai),
        // (1 - fs) / ((1 - fs) dlai), 1 / (1 - td)
        v[nz + j] = ns.omtb;
        v[2 * nz + j] = omtd;
        v[3 * nz + j] = ns.fsisl;
        v[4 * nz + j] = ns.isl;
        v[5 * nz + j] = ns.fhish;
        v[6 * nz + j] = 1.0 / omtd;  // refld = (1 - td) rho  ->  1/refld = (1/rho) * this
        break;
      }
      default:  // 2s, 4s, g77, bf
        v[j] = L;
        v[nz + j] = ekl;
        break;
    }
  }
}

// The sun record of (column, t) (SeriesArgs, crt_internal.hpp): what k_colpre forms from K_b = G(psi) / cos psi, by the same functions.  One
// wave per record.  a.psi / a.g_at_psi are [ncol][nt]; a.ws holds the canopy records (dlai statistics, zq_pa's interfaces).
__global__ __launch_bounds__(64) void k_colsun(ColArgs a, int nt, long long nitem, double* __restrict__ sunrec) {
  const long long v = blockIdx.x;
  if (v >= nitem) return;
  const int c = (int)(v / nt), lane = threadIdx.x, nz = a.nz;
  const ColIn in = col_in(a, c);
  const double* can = a.ws + (long long)c * can_len(a.scheme, nz);
  const double* lai = in.lai;
  ColArgs at = a;  // col_sun reads psi[c], g_at_psi[c]: point them at state t of this column
  at.psi = a.psi + (v - c);
  at.g_at_psi = a.g_at_psi ? a.g_at_psi + (v - c) : nullptr;
  const ColSun sun = col_sun(at, c, in);
  const double Kb = sun.Kb;
  double* rec = sunrec + v * sun_len(a.scheme, nz);
  if (lane == 0) {
    double tpsi = 0.0;
    if (a.scheme == CRT_SCHEME_ZQ) tpsi = fexp(-Kb * can[S_DLM]);                     // _solve_zq.py:52
    if (a.scheme == CRT_SCHEME_ZQ_PA) tpsi = fexp(-Kb * (lai[0] / zqpa_M(nz)));       // _solve_zq_pa.py:174
    rec[0] = Kb;
    rec[1] = sun.cs;
    rec[2] = sun.G;
    rec[3] = 1.0 / sun.cs;
    rec[4] = tpsi;
    rec[5] = rec[6] = rec[7] = 0.0;
  }
  double* sv = rec + SUN_HDR;
  const bool n79u = a.scheme == CRT_SCHEME_N79 && can[S_UNIF] != 0.0 && nz >= 3;
  const double dlu = can[S_DL];
  const double* xis = can + rec_len(a.scheme, nz);
  for (int j = lane; j < nz; j += 64) {
    const double L = lai[j];
    const double ekl = col_ekl(Kb, L);
    switch (a.scheme) {
      case CRT_SCHEME_ZQ_PA:
        sv[j] = zqpa_fsl(Kb, xis, zqpa_M(nz), j);
        sv[nz + j] = ekl;
        break;
      case CRT_SCHEME_N79: {
        N79Sun ns = {1, 0, 0, 0};
        if (j + 1 < nz) ns = n79_sun(Kb, L, lai[j + 1], n79u, dlu);
        sv[j] = ekl;
        sv[nz + j] = ns.omtb;
        sv[2 * nz + j] = ns.fsisl;
        sv[3 * nz + j] = ns.isl;
        sv[4 * nz + j] = ns.fhish;
        break;
      }
      default:
        sv[j] = ekl;
        break;
    }
  }
}

// tau_d for arbitrary LAI values from K_b sampled at the library's nodes (common.py:30-87 `tau_df_fn`)
__global__ __launch_bounds__(256) void k_tau_d(const double* __restrict__ kb_nodes, const double* __restrict__ L, long long n, int method,
                                                double* __restrict__ out) {
  __shared__ double kq[NQT];
  __shared__ double k9[CRT_NQ_9SKY];
  for (int q = threadIdx.x; q < NQT; q += blockDim.x) kq[q] = kb_nodes[q];
  if (threadIdx.x < CRT_NQ_9SKY) k9[threadIdx.x] = kb_nodes[NQT + NQG + threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = method == CRT_TAU_D_9SKY ? tau_d_9sky(k9, L[i]) : tau_d_quad(kq, L[i]);
}

}  // namespace

int launch_tau_d(const double* kb_nodes, const double* L, long long n, int method, double* out, hipStream_t s) {
  const int st = init_quadrature(s);
  if (st != CRT_OK) return st;
  const long long nblk = (n + 255) / 256;
  if (nblk > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_tau_d, dim3((unsigned)nblk), dim3(256), 0, s, kb_nodes, L, n, method, out);
  return hipGetLastError() == hipSuccess ? CRT_OK : CRT_ERR_LAUNCH;
}

void host_quad_nodes(double mu_s, double* psi_nodes) {
  std::call_once(h_once, build_host_tables);
  for (int q = 0; q < NQT; ++q) psi_nodes[q] = h_qc.psi[q];
  for (int t = 0; t < NQG; ++t) {
    double lo, hi;
    g4_interval(mu_s, t / NGL, lo, hi);
    psi_nodes[NQT + t] = lo + (h_qc.gx[t % NGL] + 1.0) * (hi - lo) / 2;
  }
  for (int i = 0; i < CRT_NQ_9SKY; ++i) psi_nodes[NQT + NQG + i] = (5.0 + 10.0 * i) * (M_PI / 180.0);
}

int init_quadrature(hipStream_t s) {
  std::call_once(h_once, build_host_tables);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return CRT_ERR_LAUNCH;
  if (dev < 0 || dev >= 64) return CRT_ERR_UNSUPPORTED;
  std::lock_guard<std::mutex> lk(dev_mu);
  if (!dev_inited[dev]) {
    // first call on this device only; not capturable into a hipGraph (documented in DESIGN.md).  Every unit whose kernels read the
    // tables has its own copy (col_record.hpp): this one (k_colpre, k_tau_d), solve_closed.hip (the 2s k_pipe's record prologue), dlai.hip and dleaf.hip.
    for (auto upload : {upload_qc, upload_quad_closed, upload_quad_dlai, upload_quad_dleaf})
      if (upload(h_qc, s) != CRT_OK) return CRT_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return CRT_ERR_LAUNCH;
    dev_inited[dev] = true;
  }
  return CRT_OK;
}

int launch_colpre(const ColArgs& a, hipStream_t s) {
  int st = init_quadrature(s);
  if (st != CRT_OK) return st;
  const size_t dyn = a.scheme == CRT_SCHEME_BL ? (NQT * (BL_CHUNK + 1) + 8 * BL_CHUNK + BL_UNIF_MAX_NZ) * sizeof(double) : 0;
  hipLaunchKernelGGL(k_colpre<false>, dim3(a.ncol), dim3(K0_BLOCK), dyn, s, a);
  return hipGetLastError() == hipSuccess ? CRT_OK : CRT_ERR_LAUNCH;
}

int launch_colpre_series(const ColArgs& a, int nt, double* sun, hipStream_t s) {
  int st = init_quadrature(s);
  if (st != CRT_OK) return st;
  const long long nitem = (long long)a.ncol * nt;
  if (nitem > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  const size_t dyn = a.scheme == CRT_SCHEME_BL ? (NQT * (BL_CHUNK + 1) + 8 * BL_CHUNK + BL_UNIF_MAX_NZ) * sizeof(double) : 0;
  hipLaunchKernelGGL(k_colpre<true>, dim3(a.ncol), dim3(K0_BLOCK), dyn, s, a);
  if (hipGetLastError() != hipSuccess) return CRT_ERR_LAUNCH;
  hipLaunchKernelGGL(k_colsun, dim3((unsigned)nitem), dim3(64), 0, s, a, nt, nitem, sun);
  return hipGetLastError() == hipSuccess ? CRT_OK : CRT_ERR_LAUNCH;
}

}  // namespace crt
