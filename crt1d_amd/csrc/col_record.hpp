// The band-independent column record (K0) as __device__ functions, shared by k_colpre (colpre.hip) and by the 2s k_pipe that builds its
// column's record itself (solve_closed.hip).  Both kernels call THESE functions, so there is one copy of the arithmetic and a
// record formed in either kernel has the same bits (the tests compare workspaces byte for byte).  Every function body switches
// floating-point contraction off itself: what an expression rounds to does not depend on the build flags or on where it is inlined.
//
// Quadrature (the reference evaluates its integrals with adaptive QUADPACK, scipy.integrate.quad; on device they use FIXED nodes):
//   * tau_d(L) = 2 int_0^{pi/2} exp(-K_b(psi) L) sin cos dpsi   (common.py:30-37)
//     mu_bar   =   int_0^{pi/2} cos sin / G(psi) dpsi           (_solve_2s.py:32)
//       6 panels x 16-point Gauss-Legendre on psi in [0, pi/2] (panel edges and measured accuracy per leaf-angle class and L: colpre.hip
//       PAN_EDGE; tau_d <= 1e-12, mu_bar <= 1.5e-12, 1 - tau_d <= 2.3e-12 for L >= 0.1 on every class, larger below)
//   * G_int_1 = int_0^{mu_s} G(acos m) dm,  G_int_2 = int_{mu_s}^1   (_solve_4s.py:148-149): 16-point Gauss-Legendre each, in psi
//   * '9sky': the reference's own 9 fixed angles                 (common.py:40-53)
// A CRT_G_TABLE column brings G sampled at exactly these nodes (crt_hip_quad_nodes).
#pragma once
#include <math.h>

#include "crt_internal.hpp"

namespace crt {

constexpr int NQT = CRT_NQ_TAU;
constexpr int NQG = CRT_NQ_G4;
constexpr int NGL = 16;

// node tables, built on the host once (colpre.hip) and uploaded to every translation unit's copy of `qc` (init_quadrature)
struct QuadConst {
  double psi[NQT], cs[NQT], sn[NQT];
  double w[NQT];     // plain weights in psi
  double w2sc[NQT];  // 2 w sin cos  (tau_d weights)
  double gx[NGL], gw[NGL];
  double cs9[CRT_NQ_9SKY], sn9[CRT_NQ_9SKY], sc9[CRT_NQ_9SKY];
};

// copies of the tables in the other units that read them (solve_closed.hip, dlai.hip, dleaf.hip); called by init_quadrature once per device
int upload_quad_closed(const QuadConst& h, hipStream_t s);
int upload_quad_dlai(const QuadConst& h, hipStream_t s);  // dlai.hip (the side precompute, k_dtau_d)
int upload_quad_dleaf(const QuadConst& h, hipStream_t s);  // dleaf.hip (the side precompute, k_g_dparam, k_dtau_d_dleaf)

namespace {

__constant__ QuadConst qc;  // internal linkage: one copy per translation unit

// the tables into this unit's copy (what a unit's upload_quad_* above is; colpre.hip for its own)
inline int upload_qc(const QuadConst& h, hipStream_t s) {
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(qc), &h, sizeof(QuadConst), 0, hipMemcpyHostToDevice, s) == hipSuccess ? (int)CRT_OK : (int)CRT_ERR_LAUNCH;
}

__device__ __forceinline__ double wave_sum64(double v) {  // fixed tree order -> bitwise reproducible
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// per-column inputs of the record
struct ColIn {
  int kind;
  double param, gden;  // G parameter, angle-independent part of G
  const double* tab;   // CRT_G_TABLE: G at the nodes, else nullptr
  const double* lai;
};

__device__ __forceinline__ ColIn col_in(const ColArgs& a, int c) {
#pragma clang fp contract(off)
  ColIn in;
  in.kind = a.g_kind[c];
  in.param = a.g_param ? a.g_param[c] : 0.0;
  in.tab = (in.kind == CRT_G_TABLE) ? a.g_table + (long long)c * CRT_NQ : nullptr;
  in.lai = a.lai + (long long)c * a.nz;
  in.gden = in.tab ? 0.0 : G_den(in.kind, in.param);
  return in;
}

// tau_d node q: K_b(psi_q) = G / cos and the mu_bar term w cos sin / G
__device__ __forceinline__ void col_node(const ColIn& in, int q, double& kq, double& pmb) {
#pragma clang fp contract(off)
  const double g = in.tab ? in.tab[q] : G_eval(in.kind, in.param, in.gden, qc.cs[q], qc.sn[q]);
  kq = g / qc.cs[q];
  pmb = qc.w[q] * qc.cs[q] * qc.sn[q] / g;
}

// sky angle i of the '9sky' rule: K_b = G / cos
__device__ __forceinline__ double col_node9(const ColIn& in, int i) {
#pragma clang fp contract(off)
  const double g = in.tab ? in.tab[NQT + NQG + i] : G_eval(in.kind, in.param, in.gden, qc.cs9[i], qc.sn9[i]);
  return g / qc.cs9[i];
}

// mu_bar from the node terms: lane l adds terms l and 64 + l, then the fixed-order wave sum (call with all 64 lanes of one wave)
__device__ __forceinline__ double col_mubar(double t_lo, double t_hi, int lane) {
#pragma clang fp contract(off)
  return wave_sum64(t_lo + (lane < NQT - 64 ? t_hi : 0.0));
}

// geometry of the sun: cos psi, G(psi), K_b = G / cos psi
struct ColSun {
  double cs, G, Kb;
};

__device__ __forceinline__ ColSun col_sun(const ColArgs& a, int c, const ColIn& in) {
#pragma clang fp contract(off)
  ColSun s;
  const double psi = a.psi[c];
  s.cs = cos(psi);
  const double sn = sin(psi);
  s.G = in.tab ? a.g_at_psi[c] : G_eval(in.kind, in.param, in.gden, s.cs, sn);
  s.Kb = s.G / s.cs;
  return s;
}

// the dlai statistics of a column (call with all 64 lanes of one wave): uniform-dlai detection (lets the solve kernels advance
// exponentials by recurrence) and, for zq, the sum and count of the non-zero diff(lai) of this lane's levels (_solve_zq.py:30,50)
struct ColDl {
  double dl, dsum, dcnt;
  bool unif;
};

__device__ __forceinline__ ColDl col_dl(const ColIn& in, int nz, int lane) {
#pragma clang fp contract(off)
  const double* lai = in.lai;
  const double dl = (lai[0] - lai[nz - 1]) / (nz - 1);
  const double tol = 4.0 * 2.220446049250313e-16 * fabs(lai[0]);
  bool ok = dl > 0.0;
  double dsum = 0.0, dcnt = 0.0;
  for (int j = lane; j + 1 < nz; j += 64) {
    const double d = lai[j] - lai[j + 1];
    ok = ok && fabs(d - dl) <= tol;
    if (d != 0.0) {
      dsum -= d;  // diff(lai) = lai[j+1] - lai[j]
      dcnt += 1.0;
    }
  }
  ColDl r;
  r.dl = dl;
  r.dsum = dsum;
  r.dcnt = dcnt;
  r.unif = __all(ok);
  return r;
}

// cos^2(radians(mla))   _solve_2s.py:28,68
__device__ __forceinline__ double col_cos2(double mla) {
#pragma clang fp contract(off)
  const double cm = cos(mla * (M_PI / 180.0));
  return cm * cm;
}

// the 16-double header (RecScalar); the scheme-specific entries come in as arguments (0 where the scheme has none)
__device__ __forceinline__ void col_header(double* rec, const ColSun& s, const ColDl& d, double mubar, double g1, double g2, double dlm, double tpsi,
                                  double cos2, double lt, int nz) {
#pragma clang fp contract(off)
  rec[S_KB] = s.Kb;
  rec[S_MU] = s.cs;
  rec[S_G] = s.G;
  rec[S_MUBAR] = mubar;
  rec[S_GINT1] = g1;
  rec[S_GINT2] = g2;
  rec[S_DLM] = dlm;
  rec[S_TAUI] = 0.0;
  rec[S_TPSI] = tpsi;
  rec[S_COS2] = cos2;
  rec[S_LT] = lt;
  rec[S_INVMU] = 1.0 / s.cs;
  rec[S_UNIF] = d.unif ? 1.0 : 0.0;
  rec[S_DL] = d.dl;
  rec[S_M] = (double)zqpa_M(nz);
  rec[15] = 0.0;
}

// exp(-K_b L_j): the beam fraction of level j (second vector of the 2s, 4s, bl, g77 and bf records)
__device__ __forceinline__ double col_ekl(double Kb, double L) {
#pragma clang fp contract(off)
  return fexp(-Kb * L);
}

// The whole 2s record of column c, formed by one workgroup of nthr >= 128 threads straight into `rec` (LDS) and into the column's slot of
// the workspace -- the bits k_colpre writes there, so that a later CRT_FLAG_SKIP_PRECOMPUTE call finds what it would have found.  No
// barrier of its own (the caller's next __syncthreads publishes `rec`): wave 0 forms the header, each of its lanes evaluating the two
// mu_bar terms that k_colpre's wave 0 reads from LDS (lane l: nodes l and 64 + l), so the wave sum adds the same values in the same
// order; the other waves form the level vectors, each with its own (identical) K_b.
__device__ __forceinline__ void col_record_2s(const ColArgs& a, int c, double* rec, int tid, int nthr) {
#pragma clang fp contract(off)
  const ColIn in = col_in(a, c);
  const int nz = a.nz;
  double* ws = a.ws + (long long)c * rec_len(CRT_SCHEME_2S, nz);
  if (tid < 64) {
    const int lane = tid;
    const ColSun sun = col_sun(a, c, in);
    const ColDl dls = col_dl(in, nz, lane);
    double kq, t_lo, t_hi = 0.0;
    col_node(in, lane, kq, t_lo);
    if (lane < NQT - 64) col_node(in, 64 + lane, kq, t_hi);
    const double mubar = col_mubar(t_lo, t_hi, lane);
    if (lane == 0) {
      const double cos2 = col_cos2(a.mla[c]);
      col_header(rec, sun, dls, mubar, 0.0, 0.0, 0.0, 0.0, cos2, in.lai[0], nz);
      col_header(ws, sun, dls, mubar, 0.0, 0.0, 0.0, 0.0, cos2, in.lai[0], nz);
    }
  } else if (tid - 64 < nz) {
    const double Kb = col_sun(a, c, in).Kb;
    for (int j = tid - 64; j < nz; j += nthr - 64) {
      const double L = in.lai[j];
      const double ekl = col_ekl(Kb, L);
      rec[REC_HDR + j] = L;
      rec[REC_HDR + nz + j] = ekl;
      ws[REC_HDR + j] = L;
      ws[REC_HDR + nz + j] = ekl;
    }
  }
}

}  // namespace
}  // namespace crt
