// Optical-property Jacobians of the level spectra (include/crt1d_hip_jac.h): d X[levels[r]][b] / d (leaf_r, leaf_t, soil_r)[b] for
// X = I_df_d, I_df_u, F, by forward-mode differentiation.  The per-band maths of the schemes is restated here on Du, a value with ONE
// tangent; the scheme objects of the solve kernels (Sch2s, TriZq, ...) are not touched.
//
// Work decomposition: lane <-> band, and the parameter index p is a GRID dimension (blockIdx.z), so a lane carries one tangent (three would
// triple the ~40 live doubles of the 2s constants) and its seed (1 in the parameter's slot) is workgroup-uniform.  A wave stores 64
// consecutive bands of one [p] slab of out.X[c][r][p][b]: 512 contiguous bytes.  A workgroup owns one column and one band slice.
//
//  k_jac      2s, bl, g77, bf: the band constants are differentiated once, then every selected level is evaluated directly from L_j and
//             e^{-K_b L_j} of the column record (no level walk, no uniform-dLAI recurrence): O(nsel), and a row's bits do not depend on
//             the other levels.  LDS: the record header and the selected entries of its vectors.
//  k_jac_tri  n79, zq: the tridiagonal system is block-eliminated as in the solve kernels (the pair (e, f) of level k, up_k = f_k - e_k dn_k),
//             here in plain (not projective) form on Du: e carries the matrix, f the right-hand side, so their tangents ARE the solve
//             A x' = d' - A' x with the same matrix.  The forward sweep leaves (e, f) of every FOURTH level in LDS; the back substitution
//             recomputes the three levels in between into registers, block by block.  8 bytes per level and lane: a whole wave up to
//             nz = 304 (n79) / 311 (zq), then 32 and 16 lanes per workgroup (jac_tri_lanes).  One wave per workgroup, every lane in its own LDS column: no
//             barrier after the record is staged.  The reference's quirks are kept: n79's first downward row uses layer
//             index 1, zq one dlai_mean for every layer.
#include "crt_internal.hpp"

namespace crt {
namespace {

// ------------------------------------------------------------------------------------------
// value + one tangent.  The build runs with -ffp-contract=off: every operation below rounds separately, in every kernel.
struct Du {
  double v, d;
};
__device__ __forceinline__ Du mk(double v) { return Du{v, 0.0}; }
__device__ __forceinline__ Du operator-(Du a) { return Du{-a.v, -a.d}; }
__device__ __forceinline__ Du operator+(Du a, Du b) { return Du{a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Du operator+(Du a, double b) { return Du{a.v + b, a.d}; }
__device__ __forceinline__ Du operator+(double a, Du b) { return Du{a + b.v, b.d}; }
__device__ __forceinline__ Du operator-(Du a, Du b) { return Du{a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Du operator-(Du a, double b) { return Du{a.v - b, a.d}; }
__device__ __forceinline__ Du operator-(double a, Du b) { return Du{a - b.v, -b.d}; }
__device__ __forceinline__ Du operator*(Du a, Du b) { return Du{a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Du operator*(Du a, double b) { return Du{a.v * b, a.d * b}; }
__device__ __forceinline__ Du operator*(double a, Du b) { return Du{a * b.v, a * b.d}; }
// one reciprocal (fast_rcp: <= 1 ulp, no IEEE fix-up sequence): a / b = a (1 / b), (a / b)' = (a' - (a / b) b') / b
__device__ __forceinline__ Du operator/(Du a, Du b) {
  const double ib = fast_rcp(b.v), v = a.v * ib;
  return Du{v, (a.d - v * b.d) * ib};
}
__device__ __forceinline__ Du operator/(double a, Du b) {
  const double ib = fast_rcp(b.v), v = a * ib;
  return Du{v, -(v * b.d) * ib};
}
__device__ __forceinline__ Du operator/(Du a, double b) {
  const double ib = fast_rcp(b);
  return Du{a.v * ib, a.d * ib};
}
__device__ __forceinline__ Du dsqrt(Du a) {
  const double s = sqrt(a.v);
  return Du{s, a.d * (0.5 * fast_rcp(s))};
}
__device__ __forceinline__ Du dexp(Du a) {
  const double e = fexp(a.v);
  return Du{e, e * a.d};
}

// phi(x) = (e^x - 1) / x, the divided difference of the exponential: (e^{-a L} - e^{-b L}) / (b - a) = L e^{-b L} phi((b - a) L) stays
// exact to rounding where a scheme's two extinction coefficients meet (2s: K_b = h; bf: k_b = k_d), a removable singularity that the
// textbook forms divide through -- harmless at 1e-16 / (b - a) in the value, but 1e-16 / (b - a)^2 in the tangent.  phi' = (e^x - phi) / x
// cancels near 0 in turn: both come from their series below |x| = 1/2 (19 terms: 0.5^19 / 20! < 1e-24).
__device__ inline Du dphi(Du x) {
  const double v = x.v;
  double p, dp;
  if (fabs(v) < 0.5) {
    constexpr double rf[19] = {1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880, 1.0 / 3628800,
                               1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0, 1.0 / 1307674368000.0,
                               1.0 / 20922789888000.0, 1.0 / 355687428096000.0, 1.0 / 6402373705728000.0, 1.0 / 121645100408832000.0};  // 1 / (n + 1)!
    p = 0.0;
    dp = 0.0;
#pragma unroll
    for (int n = 18; n >= 0; --n) p = p * v + rf[n];        // sum x^n / (n + 1)!
#pragma unroll
    for (int n = 18; n >= 1; --n) dp = dp * v + n * rf[n];  // sum n x^(n-1) / (n + 1)!
  } else {
    const double e = fexp(v), iv = fast_rcp(v);
    p = (e - 1.0) * iv;
    dp = (e - p) * iv;
  }
  return Du{p, dp * x.d};
}

// the spectra of one (column, band), the three parameters seeded for parameter p (uniform)
struct JBand {
  double I_dr0, I_df0;
  Du r, t, s;
};
__device__ __forceinline__ JBand load_jband(const SolveArgs& a, int c, int b, int p, bool soil) {
  const long long i = (long long)c * a.col_stride + b;
  JBand in;
  in.I_dr0 = static_cast<const double*>(a.I_dr0)[i];
  in.I_df0 = static_cast<const double*>(a.I_df0)[i];
  in.r = Du{static_cast<const double*>(a.leaf_r)[i], p == 0 ? 1.0 : 0.0};
  in.t = Du{static_cast<const double*>(a.leaf_t)[i], p == 1 ? 1.0 : 0.0};
  in.s = Du{soil ? static_cast<const double*>(a.soil_r)[i] : 0.0, p == 2 ? 1.0 : 0.0};
  return in;
}

// ------------------------------------------------------------------------------------------
// closed forms.  init(hdr, band, A0): hdr = the record header, A0 = e^{-K_b L} at the ground; level(L, eK, dn, up): the two diffuse
// streams at a level with cumulative LAI L and beam fraction eK = e^{-K_b L}.

// 2s  Dickinson-Sellers two-stream (crt1d/solvers/_solve_2s.py:54-156)
struct J2s {
  static constexpr const char* NAME = "2s";
  static constexpr bool SOIL = true;
  // up/dn = A E(L) + B e^{-hL} + C e^{+hL} with E(L) = (e^{-K_b L} - e^{-hL}) / sigma, sigma = mu_bar^2 (K_b^2 - h^2) (:85).  The reference
  // writes A / sigma e^{-K_b L} and folds -A / sigma into B and C; here sigma is never divided by: with delta = K_b - h,
  //   E(L) = -e^{-hL} (L / mu_bar) phi(-delta L) g,   g = 1 / (mu_bar (K_b + h)),
  // and the sigma-proportional parts of the reference's h2, h3, h5, h6 (:99-120) are taken out the same way through
  // S2 - S1 = -delta LT S1 phi(-delta LT)  (S1 = e^{-h LT}, S2 = e^{-K_b LT}).  Same function, no removable singularity at K_b = h.
  Du h, delta, Au, Bu, Cu, Ad, Bd, Cd;
  double imb;
  __device__ inline void init(const double* hd, const JBand& in, double) {
    const double K = hd[S_KB], mu = hd[S_MU], mb = hd[S_MUBAR], cos2 = hd[S_COS2], LT = hd[S_LT];
    const Du al = in.r, ta = in.t, rs = in.s;
    const Du om = al + ta;                                              // :65
    const Du beta = 0.5 * (om + (al - ta) * cos2) / om;                 // :68
    const Du a_s = om * (0.5 * (1 - mu * log((mu + 1) / mu)));          // :73
    const double mbK = mb * K;
    const Du beta0 = (1 + mbK) / (om * mbK) * a_s;                      // :76
    const Du b = 1 - (1 - beta) * om;                                   // :80
    const Du c = om * beta;
    const Du d = om * mbK * beta0;
    const Du f = om * mbK * (1 - beta0);
    h = dsqrt(b * b - c * c) / mb;
    const Du u1 = b - c / rs;                                           // :87
    const Du u2 = b - c * rs;
    const Du u3 = f + c * rs;
    const Du S1 = dexp(-(h * LT));
    const double S2 = fexp(-K * LT);
    const Du mh = mb * h;
    const Du p1 = b + mh, p2 = b - mh, p3 = b + mbK, p4 = b - mbK;
    const Du iS1 = 1.0 / S1;
    const Du D1 = p1 * (u1 - mh) * iS1 - p2 * (u1 + mh) * S1;           // :96
    const Du D2 = (u2 + mh) * iS1 - (u2 - mh) * S1;
    const Du iD1 = 1.0 / D1, iD2 = 1.0 / D2;
    delta = K - h;
    imb = 1.0 / mb;
    const Du g = 1.0 / (mb * (K + h));
    const Du phiT = dphi(-(delta * LT));
    const Du h1g = (-(d * p4) - c * f) * g;                             // h1 :99, h1 / sigma = h1 g / (mu_bar delta)
    const Du h4g = (-(f * p3) - c * d) * g;                             // h4 :108 (Sellers 1996)
    const Du w = (u1 + mbK) * (LT * imb) * phiT;
    const Du h2 = iD1 * (d * (u1 - mh) * iS1 - p2 * (d - c) * S2 + h1g * (p2 * S1 * (1 - w) - (u1 - mh) * iS1));
    const Du h3 = -(iD1 * (d * (u1 + mh) * S1 - p1 * (d - c) * S2 + h1g * S1 * (p1 - (u1 + mh) - p1 * w)));
    const Du h6 = iD2 * (u3 * S2 + h4g * S1 * (1 + (u2 - mbK) * (LT * imb) * phiT));
    const Du h5 = -h6;
    const Du h7 = c * iD1 * (u1 - mh) * iS1;
    const Du h8 = -(c * iD1 * (u1 + mh) * S1);
    const Du h9 = iD2 * (u2 + mh) * iS1;
    const Du h10 = -(iD2 * (u2 - mh) * S1);                             // :120
    Au = in.I_dr0 * h1g;
    Bu = in.I_dr0 * h2 + in.I_df0 * h7;
    Cu = in.I_dr0 * h3 + in.I_df0 * h8;
    Ad = in.I_dr0 * h4g;
    Bd = in.I_dr0 * h5 + in.I_df0 * h9;
    Cd = in.I_dr0 * h6 + in.I_df0 * h10;
  }
  __device__ inline void level(double L, double, Du& dn, Du& up) const {
    const Du em = dexp(-(h * L));
    const Du ep = 1.0 / em;
    const Du E = -(em * (L * imb) * dphi(-(delta * L)));
    up = Au * E + Bu * em + Cu * ep;                                    // :125-135
    dn = Ad * E + Bd * em + Cd * ep;
  }
};

// bl  Beer-Lambert (crt1d/solvers/_solve_bl.py:51-90): no soil, no upward stream; the sky-diffuse term I_df0 tau_d(L) has no tangent
struct JBl {
  static constexpr const char* NAME = "bl";
  static constexpr bool SOIL = false;
  Du Kg;
  double I_dr0;
  __device__ inline void init(const double* hd, const JBand& in, double) {
    Kg = hd[S_KB] * dsqrt(1 - (in.t + in.r));                           // :58-62
    I_dr0 = in.I_dr0;
  }
  __device__ inline void level(double L, double eK, Du& dn, Du& up) const {
    const Du tg = dexp(-(Kg * L));                                      // :65
    dn = 0.5 * (I_dr0 * (tg - eK));                                     // :70,74,79
    up = mk(0.0);                                                       // :87
  }
};

// g77 Goudriaan 1977 (crt1d/solvers/_solve_g77.py:48-124) and bf Bodin & Franklin (crt1d/solvers/_solve_bf.py:60-140)
template <bool BF>
struct JG77 {
  static constexpr const char* NAME = BF ? "bf" : "g77";
  static constexpr bool SOIL = true;
  double kb, LT, I_dr0, I_df0;
  Du r, t, kp, kd, omr, oms, gnd;
  __device__ inline void init(const double* hd, const JBand& in, double A0) {
    kb = hd[S_KB];
    LT = hd[S_LT];
    const double mu = hd[S_MU];
    I_dr0 = in.I_dr0;
    I_df0 = in.I_df0;
    r = in.r;
    t = in.t;
    oms = 1 - (in.r + in.t);                                            // g77:57
    kp = dsqrt(oms);                                                    // :59
    const Du rho_c = ((1 - kp) / (1 + kp)) * (2 / (1 + 1.6 * mu));      // :66
    omr = BF ? mk(1.0) : 1 - rho_c;                                     // bf:84 drops (1 - rho_c)
    kd = 0.8 * kp;                                                      // :69
    const Du ed0 = dexp(-(kd * LT));
    const Du Idf0 = I_df0 * omr * ed0;
    Du Iscd0;
    if (BF)
      Iscd0 = I_dr0 * t * (LT * ed0 * dphi((kd - kb) * LT));            // bf:95, (A0 - ed0) / (kd - kb) by dphi
    else
      Iscd0 = 0.5 * (I_dr0 * omr * dexp(-(kp * (kb * LT))) - I_dr0 * oms * A0);
    gnd = in.s * (I_dr0 * A0 + Idf0 + Iscd0);                           // g77:95, bf:112
  }
  __device__ inline void level(double L, double Asl, Du& dn, Du& up) const {
    const Du ed = dexp(-(kd * L));
    const Du er = dexp(-(kd * (LT - L)));
    const Du Idf = I_df0 * omr * ed;                                    // g77:73 / bf:84
    Du Iscd, Iscu;
    if (BF) {
      const Du ex = dexp(kd * L - (kb + kd) * LT);
      Iscd = I_dr0 * t * (L * ed * dphi((kd - kb) * L));                // bf:95, (Asl - ed) / (kd - kb) by dphi
      Iscu = I_dr0 * r * ((Asl - ex) / (kd + kb));                      // bf:99-103
    } else {
      const Du ex = dexp(-(kp * (kb * L)));
      const Du Isc = I_dr0 * omr * ex - I_dr0 * oms * Asl;              // g77:84-86
      Iscd = 0.5 * Isc;
      Iscu = Iscd;
    }
    dn = Iscd + Idf;                                                    // :115
    up = Iscu + gnd * er;                                               // :116, :95
  }
};

__device__ __forceinline__ void jac_store(const JacArgs& jo, long long o, Du dn, Du up) {
  if (jo.o[0]) jo.o[0][o] = dn.d;
  if (jo.o[1]) jo.o[1][o] = up.d;
  if (jo.o[2]) jo.o[2][o] = 2 * (up.d + dn.d);  // F = I_dr / mu + 2 (up + dn), and I_dr does not depend on the optics
}

constexpr int JAC_BLOCK = 256;

template <class S>
__global__ __launch_bounds__(JAC_BLOCK) void k_jac(SolveArgs a, LevArgs la, JacArgs jo, int per) {
  __shared__ double hd[REC_HDR + 2];
  __shared__ double lvL[CRT_MAX_LEVEL_SELECT], lvE[CRT_MAX_LEVEL_SELECT];
  const int c = blockIdx.x, p = blockIdx.z, nz = a.nz, nb = a.nb, nsel = la.nsel, tid = threadIdx.x;
  const int b = blockIdx.y * per + tid;
  const bool live = tid < per && b < nb;
  const long long o0 = ((long long)c * nsel * CRT_JAC_NPARAM + p) * nb + b;  // row r: + r * 3 nb
  if (!S::SOIL && p == 2) {  // (uniform) no soil in this scheme
    if (live)
      for (int r = 0; r < nsel; ++r) jac_store(jo, o0 + (long long)r * CRT_JAC_NPARAM * nb, mk(0.0), mk(0.0));
    return;
  }
  const double* rec = a.ws + (long long)c * a.reclen;
  if (tid < REC_HDR) hd[tid] = rec[tid];
  if (tid == REC_HDR) hd[REC_HDR] = rec[REC_HDR + nz];  // e^{-K_b L} at the ground
  for (int r = tid; r < nsel; r += blockDim.x) {
    const int j = la.lev[r];
    lvL[r] = rec[REC_HDR + j];
    lvE[r] = rec[REC_HDR + nz + j];
  }
  __syncthreads();
  if (!live) return;
  S st;
  st.init(hd, load_jband(a, c, b, p, S::SOIL), hd[REC_HDR]);
  for (int r = 0; r < nsel; ++r) {
    Du dn, up;
    st.level(lvL[r], lvE[r], dn, up);
    jac_store(jo, o0 + (long long)r * CRT_JAC_NPARAM * nb, dn, up);
  }
}

// ------------------------------------------------------------------------------------------
// tridiagonal schemes.  State of level k: (e_k, f_k) with up_k = f_k - e_k dn_k.
//   init(rec, band, nz);  first(e, f): level 0;  advance(k, e, f): level k -> k + 1;  top(e, f): the top row (sets the back state);
//   back(k, e, f, dn, up): level k from level k + 1 and (e_k, f_k), gives the outputs of level k.
//   nstates(nz): levels that carry a state;  TOP_OUT: top() belongs to an output level (nz - 1)

// n79 (crt1d/solvers/_solve_n79.py:70-155).  Record vectors: [0] tbcum = e^{-K_b lai}, [1] 1 - tb, [2] 1 - td.
struct JN79 {
  static constexpr const char* NAME = "n79";
  static constexpr int ID = CRT_SCHEME_N79;
  static constexpr int NVEC = 3;
  static constexpr bool TOP_OUT = true;
  __host__ __device__ static inline int nstates(int nz) { return nz; }
  const double* rec;
  int nz;
  double swb, swd;
  Du rho, tau, alb, irho;
  Du dn, up;  // level k + 1 of the back substitution

  __device__ inline void init(const double* rec_, const JBand& in, int nz_) {
    rec = rec_;
    nz = nz_;
    swb = in.I_dr0;
    swd = in.I_df0;
    rho = in.r;
    tau = in.t;
    alb = in.s;
    irho = 1.0 / rho;
  }
  // layer scattering coefficients (:85-88 / :102-105): r = trand / refld, s = refld - trand^2 / refld;  1 / refld = (1 / rho) (1 / (1 - td_j)):
  // the band's reciprocal, formed once, times a plain reciprocal
  __device__ inline void layer(int j, Du& r, Du& s) const {
    const double omt = rec[REC_HDR + 2 * nz + j];
    const Du refld = omt * rho;
    const Du trand = omt * tau + (1 - omt);
    r = trand * (irho * fast_rcp(omt));
    s = refld - trand * r;
  }
  __device__ inline void first(Du& e, Du& f) const {  // row 0: soil, upward (:79-82)
    e = -alb;
    f = (swb * rec[REC_HDR]) * alb;
  }
  // the odd row of level k (layer m; the first downward row uses layer index 1, :85-92) and the even row of level k + 1 (layer k):
  //   A = 1 + s_m e,  D = A - r_k r_m,   e' = -s_k A / D,   f' = (d_even A + r_k (d_odd + s_m f)) / D
  __device__ inline void advance(int k, Du& e, Du& f) const {
    const double* tbcum = rec + REC_HDR;
    const double* omtb = tbcum + nz;
    const int m = k == 0 ? 1 : k;
    Du rm, sm, r, s;
    layer(m, rm, sm);
    if (k == 0) {
      layer(0, r, s);
    } else {
      r = rm;
      s = sm;
    }
    const double src = swb * tbcum[k + 1];
    const Du d_odd = (src * omtb[m]) * (tau - rho * rm);   // (:92, :119)
    const Du d_even = (src * omtb[k]) * (rho - tau * r);   // (:109, :129)
    const Du A = 1 + sm * e;
    const Du iD = 1.0 / (A - r * rm);
    f = (d_even * A + r * (d_odd + sm * f)) * iD;
    e = -(s * A) * iD;
  }
  __device__ inline void top(Du e, Du f) {  // dn = sky diffuse (:132-135)
    dn = mk(swd);
    up = f - e * dn;
  }
  // dn_k from the upward equation of level k + 1 (layer k):  -r dn_k + up_{k+1} - s dn_{k+1} = d_even   (s < 0: no cancellation)
  __device__ inline void back(int k, Du e, Du f, bool, Du& odn, Du& oup) {
    Du r, s;
    layer(k, r, s);
    const double src = swb * rec[REC_HDR + k + 1] * rec[REC_HDR + nz + k];
    const Du d_even = src * (rho - tau * r);
    dn = (up - s * dn - d_even) / r;
    up = f - e * dn;
    odn = dn;
    oup = up;
  }
};

// zq (crt1d/solvers/_solve_zq.py:74-219).  State k <-> SWu0[k] = f_k - e_k SWd0[k], k = 0 .. m (m = nz); output level k < m.
struct JZq {
  static constexpr const char* NAME = "zq";
  static constexpr int ID = CRT_SCHEME_ZQ;
  static constexpr int NVEC = 1;
  static constexpr bool TOP_OUT = false;
  __host__ __device__ static inline int nstates(int nz) { return nz + 1; }
  const double* rec;
  int m;
  double I_dr0, I_df0;
  Du rho, fwd, q, cu, cd;
  Du dint, fq, a1, c1, fdh, iden;  // interior layers (1 < li < m): 1 - q^2, q fwd, (1 - q^2)^2, (1 - q^2) cu, fwd / (1 - q^2), 1 / (1 - q^2)
  Du xd, xu;  // SWd0, SWu0 of the level above

  __device__ inline void init(const double* rec_, const JBand& in, int nz_) {
    rec = rec_;
    m = nz_;
    I_dr0 = in.I_dr0;
    I_df0 = in.I_df0;
    const Du bL = in.r, tL = in.t;
    rho = in.s;
    const double mu = rec[S_MU], t = rec[S_TAUI], t_psi = rec[S_TPSI];
    const Du sum = bL + tL;
    const Du oma = sum;                                                       // 1 - aL, aL = 1 - (bL + tL)  :87
    const Du isum = 1.0 / sum;
    const Du r_i = 2.0 / 3 * (bL * isum) + 1.0 / 3 * (tL * isum);             // eq. 23 :40-43
    const Du r_psi = 0.5 + 0.3334 * ((bL - tL) * isum) * mu;                  // eq. 22 :35-38
    fwd = t + (1 - t) * oma * (1 - r_i);                                      // :116
    q = r_i * oma * (1 - t);
    cu = r_psi * (1 - t_psi) * oma;                                           // :139
    cd = (1 - t_psi) * oma * (1 - r_psi);                                     // :142
    dint = 1 - q * q;
    fq = q * fwd;
    a1 = dint * dint;
    c1 = dint * cu;
    iden = 1.0 / dint;
    fdh = fwd * iden;
  }
  // ground "layer": r = 1, t = 0, a = 1 - rho (:106-108) -> q_lo of the lowest layer is rho; the ghost layer above the top: q_hi = 0
  __device__ inline Du qlo_of(int li) const { return li == 1 ? rho : q; }
  __device__ inline Du qhi_of(int li) const { return li == m ? mk(0.0) : q; }
  __device__ inline void first(Du& e, Du& f) const {  // row 0: x0 = rho S_0 (:115,136)
    e = mk(0.0);
    f = rho * (I_dr0 * rec[REC_HDR]);
  }
  // rows 2li-1 (sub -fwd, dia -qlo fwd, sup dlo; :116-118, rhs :137-139) and 2li (sub dhi, dia -qhi fwd, sup -fwd; :119-121, rhs :140-142):
  //   B = fwd (e - qlo),  D = qhi fwd B + dhi dlo,   e' = fwd B / D,   f' = (dhi (C1 + fwd f) - C2 B) / D,   C1 = dlo cu S, C2 = dhi cd S
  // Interior layers have qlo = qhi = q, dlo = dhi = 1 - q^2: everything but B, D and the two updates is a band constant (the branch is uniform).
  __device__ inline void advance(int k, Du& e, Du& f) const {
    const int li = k + 1;
    const double S = I_dr0 * rec[REC_HDR + li - 1];  // :130
    if (li > 1 && li < m) {
      const Du B = fwd * (e - q);
      const Du iD = 1.0 / (fq * B + a1);
      f = (dint * iD) * (S * (c1 - cd * B) + fwd * f);
      e = fwd * B * iD;
      return;
    }
    const Du qlo = qlo_of(li), qhi = qhi_of(li);
    const Du dlo = 1 - qlo * q;  // :118
    const Du dhi = 1 - q * qhi;  // :119
    const Du B = fwd * (e - qlo);
    const Du iD = 1.0 / (qhi * fwd * B + dhi * dlo);
    const Du C1 = dlo * cu * S, C2 = dhi * cd * S;
    f = (dhi * (C1 + fwd * f) - C2 * B) * iD;
    e = fwd * B * iD;
  }
  __device__ inline void top(Du e, Du f) {  // x[2m+1] = I_df0 (:122,143)
    xd = mk(I_df0);
    xu = f - e * xd;
  }
  // SWd0[li-1] from row 2li:  dhi x_{2li-1} - qhi fwd x_{2li} - fwd x_{2li+1} = C2;  then, for a selected level only (`want`, uniform), the
  // multiple-scattering correction, eqs. 24/25 (:180-187)
  __device__ inline void back(int k, Du e, Du f, bool want, Du& odn, Du& oup) {
    const int li = k + 1;
    const double S = I_dr0 * rec[REC_HDR + k];
    Du xdl, xul;
    if (li > 1 && li < m) {
      xdl = cd * S + fdh * (q * xu + xd);
      xul = f - e * xdl;
      if (want) {
        odn = (xd + q * xul) * iden;
        oup = (xul + q * xd) * iden;
      }
    } else {
      const Du qlo = qlo_of(li), qhi = qhi_of(li);
      const Du dhi = 1 - q * qhi;
      xdl = (dhi * cd * S + fwd * (qhi * xu + xd)) / dhi;
      xul = f - e * xdl;
      if (want) {
        const Du id = 1.0 / (1 - qlo * q);
        odn = (xd + q * xul) * id;
        oup = (xul + qlo * xd) * id;
      }
    }
    xd = xdl;
    xu = xul;
  }
};

// LDS: the first nrec doubles of the record | the states of every JAC_TRI_CP-th level [ncp][4][W]
template <class S>
__global__ __launch_bounds__(64) void k_jac_tri(SolveArgs a, LevArgs la, JacArgs jo, int W, int nrec, int off_cp) {
  extern __shared__ double lds[];
  const int c = blockIdx.x, p = blockIdx.z, nz = a.nz, nb = a.nb, nsel = la.nsel, lane = threadIdx.x;
  {
    const double* rec = a.ws + (long long)c * a.reclen;
    for (int i = lane; i < nrec; i += 64) lds[i] = rec[i];
  }
  __syncthreads();
  const int b = blockIdx.y * W + lane;
  if (lane >= W || b >= nb) return;  // (no barrier below)
  double* const cp = lds + off_cp + lane;
  auto put = [&](int k2, Du e, Du f) {
    double* q = cp + (long long)k2 * 4 * W;
    q[0] = e.v;
    q[W] = e.d;
    q[2 * W] = f.v;
    q[3 * W] = f.d;
  };
  auto get = [&](int k2, Du& e, Du& f) {
    const double* q = cp + (long long)k2 * 4 * W;
    e = Du{q[0], q[W]};
    f = Du{q[2 * W], q[3 * W]};
  };
  S st;
  st.init(lds, load_jband(a, c, b, p, true), nz);
  const int nst = S::nstates(nz);
  Du e, f;
  st.first(e, f);
  put(0, e, f);
  for (int k = 0; k + 1 < nst; ++k) {
    st.advance(k, e, f);
    if ((k + 1) % JAC_TRI_CP == 0) put((k + 1) / JAC_TRI_CP, e, f);
  }
  st.top(e, f);
  const long long o0 = ((long long)c * nsel * CRT_JAC_NPARAM + p) * nb + b;
  int r = nsel - 1;  // rows are written from the top down
  if constexpr (S::TOP_OUT) {
    if (la.lev[r] == nz - 1) {
      jac_store(jo, o0 + (long long)r * CRT_JAC_NPARAM * nb, st.dn, st.up);
      --r;
    }
  }
  // back substitution over levels nst - 2 .. 0 in blocks of JAC_TRI_CP: the states of a block are recomputed from its kept one into registers
  // (static indices: the loops are unrolled), then consumed from the top of the block down.  Stops below the lowest selected level.
  for (int kb = ((nst - 2) / JAC_TRI_CP) * JAC_TRI_CP; kb >= 0 && r >= 0; kb -= JAC_TRI_CP) {
    const int hi = min(kb + JAC_TRI_CP - 1, nst - 2);
    Du E[JAC_TRI_CP], F[JAC_TRI_CP];
    get(kb / JAC_TRI_CP, E[0], F[0]);
#pragma unroll
    for (int i = 1; i < JAC_TRI_CP; ++i) {
      E[i] = E[i - 1];
      F[i] = F[i - 1];
      if (kb + i <= hi) st.advance(kb + i - 1, E[i], F[i]);
    }
#pragma unroll
    for (int i = JAC_TRI_CP - 1; i >= 0; --i) {
      const int k = kb + i;
      if (k <= hi && r >= 0) {
        const bool want = la.lev[r] == k;
        Du dn, up;
        st.back(k, E[i], F[i], want, dn, up);
        if (want) {
          jac_store(jo, o0 + (long long)r * CRT_JAC_NPARAM * nb, dn, up);
          --r;
        }
      }
    }
  }
}

template <class S>
int launch_jac_closed(const SolveArgs& a, const LevArgs& la, const JacArgs& jo, hipStream_t s, bool probe) {
  const LevSlices ls = lev_slices(a.nb, JAC_BLOCK);
  if (ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const int st = launch_kernel(k_jac<S>, dim3(a.ncol, ls.nslice, CRT_JAC_NPARAM), ls.nthr, 0, s, a, la, jo, ls.per);
  if (st == CRT_OK) note_kernel("k_jac<%s> nsel=%d slice=%d", S::NAME, la.nsel, ls.per);
  return st;
}

template <class S>
int launch_jac_tri(const SolveArgs& a, const LevArgs& la, const JacArgs& jo, hipStream_t s, bool probe) {
  constexpr int scheme = S::ID;
  const int W = jac_tri_lanes(scheme, a.nz);
  if (W == 0) return CRT_ERR_UNSUPPORTED;
  const long long nslice = ((long long)a.nb + W - 1) / W;
  if (nslice > 65535) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const int nrec = jac_tri_nrec(scheme, a.nz), off_cp = (nrec + 1) & ~1;
  const int st = launch_kernel(k_jac_tri<S>, dim3(a.ncol, (unsigned)nslice, CRT_JAC_NPARAM), 64, jac_tri_lds_bytes(scheme, a.nz, W), s, a, la,
                               jo, W, nrec, off_cp);
  if (st == CRT_OK) note_kernel("k_jac_tri<%s> nsel=%d slice=%d", S::NAME, la.nsel, W);
  return st;
}

}  // namespace

int launch_jac(int scheme, const SolveArgs& a, const LevArgs& la, const JacArgs& jo, hipStream_t s, bool probe) {
  static_assert(JN79::NVEC == 3 && JZq::NVEC == 1, "jac_tri_nrec");
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_jac_closed<J2s>(a, la, jo, s, probe);
    case CRT_SCHEME_BL: return launch_jac_closed<JBl>(a, la, jo, s, probe);
    case CRT_SCHEME_G77: return launch_jac_closed<JG77<false>>(a, la, jo, s, probe);
    case CRT_SCHEME_BF: return launch_jac_closed<JG77<true>>(a, la, jo, s, probe);
    case CRT_SCHEME_N79: return launch_jac_tri<JN79>(a, la, jo, s, probe);
    case CRT_SCHEME_ZQ: return launch_jac_tri<JZq>(a, la, jo, s, probe);
    default: return CRT_ERR_UNSUPPORTED;
  }
}

}  // namespace crt
