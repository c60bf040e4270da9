// The per-band maths of the schemes on Du, a value with ONE tangent, written once for the three forward-mode kernel families:
//   jac.hip   d / d (leaf_r, leaf_t, soil_r):  the optics carry the tangent (P = Du), the column record is plain (R = double);
//             zq excepted, which keeps its own struct there (its kernel is held to the code it had)
//   dlai.hip  d / d s of lai(s) = s lai:       the optics are plain (P = double), the record entries carry the tangent (R = Du)
//   dleaf.hip d along a leaf-angle direction:  as dlai.hip, and the header scalars K_b, mu_bar, cos^2 of the closed forms carry one too
//             (H = Du) while the LAI entries L_j, LT do not (LaiT)
// Every local is `auto`: an expression has the type its operands give it, so that with (P, R) = (Du, double) each line is the operation
// the optics Jacobian has always performed.  The scheme objects of the solve kernels (Sch2s, TriZq, ...) are not touched.
#pragma once
#include "crt_internal.hpp"

namespace crt {
namespace {

// ------------------------------------------------------------------------------------------
// value + one tangent.  The build runs with -ffp-contract=off: every operation below rounds separately, in every kernel.
struct Du {
  double v, d;
};
__device__ __forceinline__ Du mk(double v) { return Du{v, 0.0}; }
__device__ __forceinline__ Du to_du(Du a) { return a; }
__device__ __forceinline__ Du to_du(double a) { return Du{a, 0.0}; }
// a cumulative LAI of the record as R: lai(s) = s lai, so its tangent is itself
template <class R>
__device__ __forceinline__ R seed_lai(double L) {
  if constexpr (std::is_same_v<R, Du>)
    return Du{L, L};
  else
    return L;
}
// the type of the LAI entries L_j, LT: they scale with s (R) but do not depend on the leaf angles
template <class R, class H>
using LaiT = std::conditional_t<std::is_same_v<H, Du>, double, R>;
// what depends on the optics (P) or on the header scalars (H)
template <class P, class H>
using PorH = std::conditional_t<std::is_same_v<P, Du> || std::is_same_v<H, Du>, Du, double>;
// header scalar i as H; H = Du: the tangent lies HDR_TAN doubles behind the value (the kernel stages both)
constexpr int HDR_TAN = 2 * REC_HDR;
template <class H>
__device__ __forceinline__ H hdr(const double* hd, int i) {
  if constexpr (std::is_same_v<H, Du>)
    return Du{hd[i], hd[HDR_TAN + i]};
  else
    return hd[i];
}
template <class T>
__device__ __forceinline__ T cst(double v) {
  if constexpr (std::is_same_v<T, Du>)
    return Du{v, 0.0};
  else
    return v;
}
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
__device__ __forceinline__ double dsqrt(double a) { return sqrt(a); }
__device__ __forceinline__ Du dexp(Du a) {
  const double e = fexp(a.v);
  return Du{e, e * a.d};
}
__device__ __forceinline__ double dexp(double a) { return fexp(a); }
// 1 / x of a record entry
__device__ __forceinline__ double rinv(double a) { return fast_rcp(a); }
__device__ __forceinline__ Du rinv(Du a) { return 1.0 / a; }

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

// the spectra of one (column, band); P = Du: the three optical parameters seeded by the caller
template <class P>
struct JBandT {
  double I_dr0, I_df0;
  P r, t, s;
};

// the leading doubles of a column record as values of type R; R = Du: the value from the record, the tangent from `t` (same layout)
template <class R>
struct RecV;
template <>
struct RecV<double> {
  const double* v;
  __device__ __forceinline__ double operator[](int i) const { return v[i]; }
  __device__ __forceinline__ RecV operator+(int n) const { return RecV{v + n}; }
};
template <>
struct RecV<Du> {
  const double* v;
  const double* t;
  __device__ __forceinline__ Du operator[](int i) const { return Du{v[i], t[i]}; }
  __device__ __forceinline__ RecV operator+(int n) const { return RecV{v + n, t + n}; }
};

// ------------------------------------------------------------------------------------------
// closed forms.  init(hdr, band, A0): hdr = the record header, A0 = e^{-K_b LT} at the ground; level(L, eK, dn, up):
// the two diffuse streams at a level with cumulative LAI L and beam fraction eK = e^{-K_b L}.

// 2s  Dickinson-Sellers two-stream (crt1d/solvers/_solve_2s.py:54-156)
template <class P, class R, class H = double>
struct J2sT {
  using LT_t = LaiT<R, H>;
  static constexpr const char* NAME = "2s";
  static constexpr bool SOIL = true;
  // up/dn = A E(L) + B e^{-hL} + C e^{+hL} with E(L) = (e^{-K_b L} - e^{-hL}) / sigma, sigma = mu_bar^2 (K_b^2 - h^2) (:85).  The reference
  // writes A / sigma e^{-K_b L} and folds -A / sigma into B and C; here sigma is never divided by: with delta = K_b - h,
  //   E(L) = -e^{-hL} (L / mu_bar) phi(-delta L) g,   g = 1 / (mu_bar (K_b + h)),
  // and the sigma-proportional parts of the reference's h2, h3, h5, h6 (:99-120) are taken out the same way through
  // S2 - S1 = -delta LT S1 phi(-delta LT)  (S1 = e^{-h LT}, S2 = e^{-K_b LT}).  Same function, no removable singularity at K_b = h.
  PorH<P, H> h, delta, Au, Ad;
  Du Bu, Cu, Bd, Cd;
  H imb;
  __device__ inline void init(const double* hd, const JBandT<P>& in, R) {
    const H K = hdr<H>(hd, S_KB);
    const double mu = hd[S_MU];
    const H mb = hdr<H>(hd, S_MUBAR), cos2 = hdr<H>(hd, S_COS2);
    const LT_t LT = seed_lai<LT_t>(hd[S_LT]);
    const auto al = in.r, ta = in.t, rs = in.s;
    const auto om = al + ta;                                              // :65
    const auto beta = 0.5 * (om + (al - ta) * cos2) / om;                 // :68
    const auto a_s = om * (0.5 * (1 - mu * log((mu + 1) / mu)));          // :73
    const auto mbK = mb * K;
    const auto beta0 = (1 + mbK) / (om * mbK) * a_s;                      // :76
    const auto b = 1 - (1 - beta) * om;                                   // :80
    const auto c = om * beta;
    const auto d = om * mbK * beta0;
    const auto f = om * mbK * (1 - beta0);
    h = dsqrt(b * b - c * c) / mb;
    const auto u1 = b - c / rs;                                           // :87
    const auto u2 = b - c * rs;
    const auto u3 = f + c * rs;
    const Du S1 = dexp(-(h * LT));
    const auto S2 = dexp(-K * LT);
    const auto mh = mb * h;
    const auto p1 = b + mh, p2 = b - mh, p3 = b + mbK, p4 = b - mbK;
    const Du iS1 = 1.0 / S1;
    const Du D1 = p1 * (u1 - mh) * iS1 - p2 * (u1 + mh) * S1;           // :96
    const Du D2 = (u2 + mh) * iS1 - (u2 - mh) * S1;
    const Du iD1 = 1.0 / D1, iD2 = 1.0 / D2;
    delta = K - h;
    imb = 1.0 / mb;
    const auto g = 1.0 / (mb * (K + h));
    const Du phiT = dphi(-(delta * LT));
    const auto h1g = (-(d * p4) - c * f) * g;                             // h1 :99, h1 / sigma = h1 g / (mu_bar delta)
    const auto h4g = (-(f * p3) - c * d) * g;                             // h4 :108 (Sellers 1996)
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
  __device__ inline void level(LT_t L, R, Du& dn, Du& up) const {
    const Du em = dexp(-(h * L));
    const Du ep = 1.0 / em;
    const Du E = -(em * (L * imb) * dphi(-(delta * L)));
    up = Au * E + Bu * em + Cu * ep;                                    // :125-135
    dn = Ad * E + Bd * em + Cd * ep;
  }
};

// bl  Beer-Lambert (crt1d/solvers/_solve_bl.py:51-90): no soil, no upward stream; the sky-diffuse term I_df0 tau_d(L) has no tangent
// with respect to the optics (the LAI derivative adds its own, dlai.hip)
template <class P, class R, class H = double>
struct JBlT {
  static constexpr const char* NAME = "bl";
  static constexpr bool SOIL = false;
  PorH<P, H> Kg;
  double I_dr0;
  __device__ inline void init(const double* hd, const JBandT<P>& in, R) {
    Kg = hdr<H>(hd, S_KB) * dsqrt(1 - (in.t + in.r));                   // :58-62
    I_dr0 = in.I_dr0;
  }
  __device__ inline void level(LaiT<R, H> L, R eK, Du& dn, Du& up) const {
    const Du tg = dexp(-(Kg * L));                                      // :65
    dn = 0.5 * (I_dr0 * (tg - eK));                                     // :70,74,79
    up = mk(0.0);                                                       // :87
  }
};

// g77 Goudriaan 1977 (crt1d/solvers/_solve_g77.py:48-124) and bf Bodin & Franklin (crt1d/solvers/_solve_bf.py:60-140)
template <bool BF, class P, class R, class H = double>
struct JG77T {
  static constexpr const char* NAME = BF ? "bf" : "g77";
  static constexpr bool SOIL = true;
  using LT_t = LaiT<R, H>;
  H kb;
  double I_dr0, I_df0;
  LT_t LT;
  P r, t, kp, kd, omr, oms;
  Du gnd;
  __device__ inline void init(const double* hd, const JBandT<P>& in, R A0) {
    kb = hdr<H>(hd, S_KB);
    LT = seed_lai<LT_t>(hd[S_LT]);
    const double mu = hd[S_MU];
    I_dr0 = in.I_dr0;
    I_df0 = in.I_df0;
    r = in.r;
    t = in.t;
    oms = 1 - (in.r + in.t);                                            // g77:57
    kp = dsqrt(oms);                                                    // :59
    const auto rho_c = ((1 - kp) / (1 + kp)) * (2 / (1 + 1.6 * mu));      // :66
    omr = BF ? cst<P>(1.0) : 1 - rho_c;                                 // bf:84 drops (1 - rho_c)
    kd = 0.8 * kp;                                                      // :69
    const Du ed0 = to_du(dexp(-(kd * LT)));
    const Du Idf0 = I_df0 * omr * ed0;
    Du Iscd0;
    if (BF)
      Iscd0 = I_dr0 * t * (LT * ed0 * dphi((kd - kb) * LT));            // bf:95, (A0 - ed0) / (kd - kb) by dphi
    else
      Iscd0 = 0.5 * (I_dr0 * omr * dexp(-(kp * (kb * LT))) - I_dr0 * oms * A0);
    gnd = in.s * (I_dr0 * A0 + Idf0 + Iscd0);                           // g77:95, bf:112
  }
  __device__ inline void level(LT_t L, R Asl, Du& dn, Du& up) const {
    const Du ed = to_du(dexp(-(kd * L)));
    const Du er = to_du(dexp(-(kd * (LT - L))));
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

// ------------------------------------------------------------------------------------------
// tridiagonal schemes.  State of level k: (e_k, f_k) with up_k = f_k - e_k dn_k.
//   init(rec, band, nz);  first(e, f): level 0;  advance(k, e, f): level k -> k + 1;  top(e, f): the top row (sets the back state);
//   back(k, e, f, dn, up): level k from level k + 1 and (e_k, f_k), gives the outputs of level k.
//   nstates(nz): levels that carry a state;  TOP_OUT: top() belongs to an output level (nz - 1)

// n79 (crt1d/solvers/_solve_n79.py:70-155).  Record vectors: [0] tbcum = e^{-K_b lai}, [1] 1 - tb, [2] 1 - td.
template <class P, class R>
struct JN79T {
  static constexpr const char* NAME = "n79";
  static constexpr int ID = CRT_SCHEME_N79;
  static constexpr int NVEC = 3;
  static constexpr bool TOP_OUT = true;
  __host__ __device__ static inline int nstates(int nz) { return nz; }
  RecV<R> rec;
  int nz;
  double swb, swd;
  P rho, tau, alb, irho;
  Du dn, up;  // level k + 1 of the back substitution

  __device__ inline void init(RecV<R> rec_, const JBandT<P>& in, int nz_) {
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
    const auto omt = rec[REC_HDR + 2 * nz + j];
    const Du refld = omt * rho;
    const Du trand = omt * tau + (1 - omt);
    r = trand * (irho * rinv(omt));
    s = refld - trand * r;
  }
  __device__ inline void first(Du& e, Du& f) const {  // row 0: soil, upward (:79-82)
    e = to_du(-alb);
    f = (swb * rec[REC_HDR]) * alb;
  }
  // the odd row of level k (layer m; the first downward row uses layer index 1, :85-92) and the even row of level k + 1 (layer k):
  //   A = 1 + s_m e,  D = A - r_k r_m,   e' = -s_k A / D,   f' = (d_even A + r_k (d_odd + s_m f)) / D
  __device__ inline void advance(int k, Du& e, Du& f) const {
    const auto tbcum = rec + REC_HDR;
    const auto omtb = tbcum + nz;
    const int m = k == 0 ? 1 : k;
    Du rm, sm, r, s;
    layer(m, rm, sm);
    if (k == 0) {
      layer(0, r, s);
    } else {
      r = rm;
      s = sm;
    }
    const auto src = swb * tbcum[k + 1];
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
    const auto src = swb * rec[REC_HDR + k + 1] * rec[REC_HDR + nz + k];
    const Du d_even = src * (rho - tau * r);
    dn = (up - s * dn - d_even) / r;
    up = f - e * dn;
    odn = dn;
    oup = up;
  }
};

// zq (crt1d/solvers/_solve_zq.py:74-219).  State k <-> SWu0[k] = f_k - e_k SWd0[k], k = 0 .. m (m = nz); output level k < m.
template <class P, class R>
struct JZqT {
  static constexpr const char* NAME = "zq";
  static constexpr int ID = CRT_SCHEME_ZQ;
  static constexpr int NVEC = 1;
  static constexpr bool TOP_OUT = false;
  __host__ __device__ static inline int nstates(int nz) { return nz + 1; }
  RecV<R> rec;
  int m;
  double I_dr0, I_df0;
  P rho;
  Du fwd, q, cu, cd;
  Du dint, fq, a1, c1, fdh, iden;  // interior layers (1 < li < m): 1 - q^2, q fwd, (1 - q^2)^2, (1 - q^2) cu, fwd / (1 - q^2), 1 / (1 - q^2)
  Du xd, xu;  // SWd0, SWu0 of the level above

  __device__ inline void init(RecV<R> rec_, const JBandT<P>& in, int nz_) {
    rec = rec_;
    m = nz_;
    I_dr0 = in.I_dr0;
    I_df0 = in.I_df0;
    const auto bL = in.r, tL = in.t;
    rho = in.s;
    const double mu = rec.v[S_MU];
    const auto t = rec[S_TAUI], t_psi = rec[S_TPSI];
    const auto sum = bL + tL;
    const auto oma = sum;                                                       // 1 - aL, aL = 1 - (bL + tL)  :87
    const auto isum = 1.0 / sum;
    const auto r_i = 2.0 / 3 * (bL * isum) + 1.0 / 3 * (tL * isum);             // eq. 23 :40-43
    const auto r_psi = 0.5 + 0.3334 * ((bL - tL) * isum) * mu;                  // eq. 22 :35-38
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
  __device__ inline Du qlo_of(int li) const { return li == 1 ? to_du(rho) : q; }
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
    const auto S = I_dr0 * rec[REC_HDR + li - 1];  // :130
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
    const auto S = I_dr0 * rec[REC_HDR + k];
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

// ------------------------------------------------------------------------------------------
// shared by the kernels whose optics are plain and whose outputs are the four level quantities (dlai.hip, dleaf.hip)
using DBand = JBandT<double>;

__device__ __forceinline__ DBand load_dband(const SolveArgs& a, int c, int b, bool soil) {
  const long long i = (long long)c * a.col_stride + b;
  DBand in;
  in.I_dr0 = static_cast<const double*>(a.I_dr0)[i];
  in.I_df0 = static_cast<const double*>(a.I_df0)[i];
  in.r = static_cast<const double*>(a.leaf_r)[i];
  in.t = static_cast<const double*>(a.leaf_t)[i];
  in.s = soil ? static_cast<const double*>(a.soil_r)[i] : 0.0;
  return in;
}

// F' of a row of the LAI or leaf-angle derivative: F = I_dr / mu + 2 (up + dn); dI = I_dr' of the row, I_dr0 (e^{-K_b L_j})'
__device__ __forceinline__ double flux_tan(double dI, double invmu, Du dn, Du up) { return __builtin_fma(dI, invmu, 2 * (up.d + dn.d)); }

__device__ __forceinline__ void dlai_store(const DlaiArgs& da, long long o, double dI, double invmu, Du dn, Du up) {
  if (da.o[0]) da.o[0][o] = dI;
  if (da.o[1]) da.o[1][o] = dn.d;
  if (da.o[2]) da.o[2][o] = up.d;
  if (da.o[3]) da.o[3][o] = flux_tan(dI, invmu, dn, up);
}

}  // namespace
}  // namespace crt
