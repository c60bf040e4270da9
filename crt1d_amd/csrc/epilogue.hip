// The absorption and band-sum epilogue: its kernels and the launchers that choose among them (declared in epilogue.hpp; api.hip
// validates the calls and fills the argument blocks).
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "epilogue.hpp"
#include "launch_forms.hpp"

namespace crt {
namespace {

// ------------------------------------------------------------------------------------------
// Epilogue: model.py:573-647 (_calc_absorption) fused with diagnostics.py:39-108 (band sums).
//
// k_absorb_bandsum: ONE streaming pass over the three profiles.  Workgroup = column, thread = band (NBT bands per thread when
// nb > 1024); the previous level's values stay in registers, so every profile byte is read exactly once (round 1 gave a
// (column, layer) to each wave and read rows k and k+1: every row twice, 0.27 of the HBM roofline).  Per level only TWO
// band sums per group are needed, because the sunlit/shaded split uses band-independent factors (as in the integrated
// kernels, crt_internal.hpp):
//     A_g(k) = sum_b w_g[b] aI(k, b),   D_g(k) = sum_b w_g[b] (1 - r - t)[b] I_dr(k+1, b)
//     aI_dr = (1 - e^{-K_b dlai_k}) D,  aI_df = A - aI_dr,  aI_sl = aI_df f_sl(k) + aI_dr,  aI_sh = aI_df (1 - f_sl(k))
// Wave sums by DPP (wave_sum_lane63), one LDS slot per wave and level; the levels are processed in chunks of BS_CH whose loads
// are all issued before the arithmetic (24 rows in flight per thread), a double-buffered partial-sum area needs one LDS-only
// barrier per chunk, and the first BS_CH * ngroup threads turn the partials of the previous chunk into outputs.
constexpr int BS_CH = 8;

// K_b = G(psi) / cos(psi) of column c of an argument block.  Only what the column's kind of G needs is read: g_at_psi for a tabulated G,
// else g_param, which may be absent.
template <class A>
__device__ inline double column_kb(const A& a, int c) {
  const double psi = a.psi[c];
  const int kind = a.g_kind[c];
  const double G = (kind == CRT_G_TABLE) ? a.g_at_psi[c] : G_closed(kind, a.g_param ? a.g_param[c] : 0.0, cos(psi), sin(psi));
  return G / cos(psi);
}
// ... and of a column whose values a kernel holds in registers already
__device__ __forceinline__ double column_kb(int kind, double g_param, double g_at_psi, double psi) {
  const double G = (kind == CRT_G_TABLE) ? g_at_psi : G_closed(kind, g_param, cos(psi), sin(psi));
  return G / cos(psi);
}

// level outputs from the three level sums: F = I_dr / mu + 2 I_df_u + 2 I_df_d is linear in the profiles (every scheme forms its F this
// way, e.g. _solve_2s.py:156), so its band sum is the same combination of the band sums; I_d = I_dr + I_df_d (model.py:425).
// SUMS = false stores F and I_d only (k_bandsum_finish: the three sums are its inputs), from the very same expressions.
template <bool SUMS = true, class A>
__device__ inline void store_level_profiles(const A& a, long long o, double R, double Dn, double Up, double invmu, bool accumulate) {
  if (accumulate) {
    if constexpr (SUMS) {
      a.L_dr[o] += R;
      a.L_dn[o] += Dn;
      a.L_up[o] += Up;
    }
    a.L_F[o] += R * invmu + 2 * (Up + Dn);
    a.L_Id[o] += R + Dn;
  } else {
    if constexpr (SUMS) {
      __builtin_nontemporal_store(R, a.L_dr + o);
      __builtin_nontemporal_store(Dn, a.L_dn + o);
      __builtin_nontemporal_store(Up, a.L_up + o);
    }
    __builtin_nontemporal_store(R * invmu + 2 * (Up + Dn), a.L_F + o);
    __builtin_nontemporal_store(R + Dn, a.L_Id + o);
  }
}

template <typename TIO, int MAXT, bool PROF>
__global__ __launch_bounds__(MAXT) void k_absorb_bandsum(EpiArgsT<TIO> a, int b0, int nbs, int accumulate) {
  // bands [b0, b0 + nbs) of every row (nbs <= blockDim.x <= 1024; spectra wider than 1024 bands take several launches, the
  // later ones adding to the outputs of the first)
  extern __shared__ double lds[];
  const int c = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  const int nz = a.nz, nb = a.nb, ng = a.ngroup;
  const double psi = a.psi[c];
  const double Kb = column_kb(a, c);
  const double* __restrict__ lai = a.lai + (long long)c * nz;
  const long long cb = (long long)c * nz * nb + b0;
  const TIO* __restrict__ R = a.I_dr + cb;
  const TIO* __restrict__ D = a.I_df_d + cb;
  const TIO* __restrict__ U = a.I_df_u + cb;
  // LDS: part[2][BS_CH][nwave][NV][MAXG] (NV = 2 sums per level and group: A, D; PROF: + the level sums of I_dr, I_df_d, I_df_u),
  // ends[nwave][4][MAXG], PROF: lev0[nwave][3][MAXG] (the level sums of row 0)
  constexpr int NV = PROF ? 5 : 2;
  double* part = lds;
  double* ends = lds + 2 * BS_CH * nwave * NV * MAXG;
  double* lev0 = ends + nwave * 4 * MAXG;
  const int pstride = nwave * NV * MAXG;  // doubles per level slot
  const double invmu = 1.0 / cos(psi);

  const bool act = tid < nbs;
  const int bi = act ? tid : 0;
  double w[MAXG], wa[MAXG];
  {
    const long long ib = (long long)c * a.col_stride + b0 + bi;
    const double la = act ? 1 - ((double)a.leaf_r[ib] + (double)a.leaf_t[ib]) : 0.0;  // :584
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      w[g] = (g < ng && act) ? a.band_w[(long long)g * nb + b0 + bi] : 0.0;
      wa[g] = w[g] * la;
    }
  }
  double r0 = R[bi], d0 = D[bi], u0 = U[bi];
  if constexpr (PROF) {  // level sums of row 0
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < ng) {
        const double t0 = wave_sum_lane63(w[g] * r0), t1 = wave_sum_lane63(w[g] * d0), t2 = wave_sum_lane63(w[g] * u0);
        if (lane == 63) {
          lev0[(wave * 3 + 0) * MAXG + g] = t0;
          lev0[(wave * 3 + 1) * MAXG + g] = t1;
          lev0[(wave * 3 + 2) * MAXG + g] = t2;
        }
      }
  }
  // energy-balance terms at the ground (diagnostics.py:476-530): transmitted I_d[0], soil-reflected I_df_u[0]
  if (a.totals) {
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < ng) {
        const double t2 = wave_sum_lane63(w[g] * (r0 + d0)), t3 = wave_sum_lane63(w[g] * u0);
        if (lane == 63) {
          ends[(wave * 4 + 2) * MAXG + g] = t2;
          ends[(wave * 4 + 3) * MAXG + g] = t3;
        }
      }
  }

  auto finish_chunk = [&](int k0, int nlev, int buf) {  // first BS_CH * ng threads: partials of levels k0 .. k0+nlev-1 -> outputs
    if (tid < BS_CH * ng) {
      const int t = tid / ng, g = tid - t * ng;
      if (t < nlev) {
        const int k = k0 + t;
        const double* p = part + (buf * BS_CH + t) * pstride;
        double A = 0.0, Dg = 0.0;
        for (int wv = 0; wv < nwave; ++wv) {
          A += p[(wv * NV + 0) * MAXG + g];
          Dg += p[(wv * NV + 1) * MAXG + g];
        }
        const double dl = lai[k] - lai[k + 1];                      // model.py:248
        const double fsl = exp(-Kb * ((lai[k] + lai[k + 1]) / 2));  // :601-602
        const double adr = (1 - exp(-Kb * dl)) * Dg;                // :617-621
        const double adf = A - adr;                                 // :628
        const long long o = ((long long)c * (nz - 1) + k) * ng + g;
        if (accumulate) {
          a.aI[o] += A;
          a.aI_sl[o] += adf * fsl + adr;
          a.aI_sh[o] += adf * (1 - fsl);
        } else {
          a.aI[o] = A;
          a.aI_sl[o] = adf * fsl + adr;                             // :631-633
          a.aI_sh[o] = adf * (1 - fsl);
        }
        if constexpr (PROF) {
          if (accumulate) a.aI_dr[o] += adr; else a.aI_dr[o] = adr;
          double sR = 0.0, sD = 0.0, sU = 0.0;
          for (int wv = 0; wv < nwave; ++wv) {
            sR += p[(wv * NV + 2) * MAXG + g];
            sD += p[(wv * NV + 3) * MAXG + g];
            sU += p[(wv * NV + 4) * MAXG + g];
          }
          store_level_profiles(a, ((long long)c * nz + k + 1) * ng + g, sR, sD, sU, invmu, accumulate != 0);  // level k + 1
        }
      }
    }
  };

  int buf = 0, prev_k0 = -1, prev_n = 0;
  for (int k0 = 0; k0 < nz - 1; k0 += BS_CH) {
    const int nlev = min(BS_CH, nz - 1 - k0);
    // all loads of the chunk first: rows k0+1 .. k0+nlev of the three profiles
    double r1[BS_CH], d1[BS_CH], u1[BS_CH];
#pragma unroll
    for (int t = 0; t < BS_CH; ++t)
      if (t < nlev) {
        const long long row = (long long)(k0 + t + 1) * nb + bi;
        r1[t] = __builtin_nontemporal_load(R + row);
        d1[t] = __builtin_nontemporal_load(D + row);
        u1[t] = __builtin_nontemporal_load(U + row);
      }
    if (prev_k0 >= 0) finish_chunk(prev_k0, prev_n, buf ^ 1);  // the previous chunk's outputs while this chunk's loads are in flight
#pragma unroll
    for (int t = 0; t < BS_CH; ++t)
      if (t < nlev) {
        const double av = r1[t] - r0 + d1[t] - d0 + u0 - u1[t];  // :609
#pragma unroll
        for (int g = 0; g < MAXG; ++g)
          if (g < ng) {
            const double ta = wave_sum_lane63(w[g] * av), td = wave_sum_lane63(wa[g] * r1[t]);
            double* p = part + (buf * BS_CH + t) * pstride;
            if (lane == 63) {
              p[(wave * NV + 0) * MAXG + g] = ta;
              p[(wave * NV + 1) * MAXG + g] = td;
            }
            if constexpr (PROF) {
              const double s0 = wave_sum_lane63(w[g] * r1[t]), s1 = wave_sum_lane63(w[g] * d1[t]), s2 = wave_sum_lane63(w[g] * u1[t]);
              if (lane == 63) {
                p[(wave * NV + 2) * MAXG + g] = s0;
                p[(wave * NV + 3) * MAXG + g] = s1;
                p[(wave * NV + 4) * MAXG + g] = s2;
              }
            }
          }
        r0 = r1[t];
        d0 = d1[t];
        u0 = u1[t];
      }
    lds_barrier();  // chunk complete (and every thread is past its reads of the other buffer)
    prev_k0 = k0;
    prev_n = nlev;
    buf ^= 1;
  }
  // canopy top: incoming I_d[top], reflected I_df_u[top] (r0, d0, u0 now hold level nz-1)
  if (a.totals) {
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < ng) {
        const double t0 = wave_sum_lane63(w[g] * (r0 + d0)), t1 = wave_sum_lane63(w[g] * u0);
        if (lane == 63) {
          ends[(wave * 4 + 0) * MAXG + g] = t0;
          ends[(wave * 4 + 1) * MAXG + g] = t1;
        }
      }
  }
  if (prev_k0 >= 0) finish_chunk(prev_k0, prev_n, buf ^ 1);
  if (a.totals || PROF) {
    lds_barrier();
    if (a.totals && tid < ng * 4) {
      const int g = tid >> 2, q = tid & 3;
      double t = 0.0;
      for (int wv = 0; wv < nwave; ++wv) t += ends[(wv * 4 + q) * MAXG + g];
      double* o = a.totals + ((long long)c * ng + g) * 4 + q;
      *o = accumulate ? *o + t : t;
    }
    if constexpr (PROF) {
      if (tid < ng) {  // level 0
        double sR = 0.0, sD = 0.0, sU = 0.0;
        for (int wv = 0; wv < nwave; ++wv) {
          sR += lev0[(wv * 3 + 0) * MAXG + tid];
          sD += lev0[(wv * 3 + 1) * MAXG + tid];
          sU += lev0[(wv * 3 + 2) * MAXG + tid];
        }
        store_level_profiles(a, (long long)c * nz * ng + tid, sR, sD, sU, invmu, accumulate != 0);
      }
    }
  }
}

// The per-column tail of the band-sum kernels below: raw band sums A_g(k), D_g(k) (LDS) -> the level outputs, lanes over (level, group).
// `factors(k, fsl, ab)` gives the level factors f_sl(k) and 1 - e^{-K_b dlai_k} of layer k: ExpFactors forms them here; a kernel that has
// formed them already hands them over.
// Streaming stores: the outputs are not read again by this kernel (1e5 x 38 x 100: 2.05 -> 1.91 ms).
struct ExpFactors {
  const double* __restrict__ lai;
  double Kb;
  __device__ void operator()(int k, double& fsl, double& ab) const {
    fsl = exp(-Kb * ((lai[k] + lai[k + 1]) / 2));  // model.py:601-602
    ab = 1 - exp(-Kb * (lai[k] - lai[k + 1]));     // :617-621
  }
};
template <int NGT, bool PROF = false, class EA, class F>
__device__ inline void bandsum_finish(const EA& a, int c, const double* raw, const double* ends, F factors, int l, int nlanes,
                                      const double* lev = nullptr) {
  const int ng = a.ngroup, nl = a.nz - 1;
  const long long ob = (long long)c * nl * ng;
  for (int i = l; i < nl * ng; i += nlanes) {
    const int k = i / ng, g = i - k * ng;
    const double A = raw[(k * NGT + g) * 2], Dg = raw[(k * NGT + g) * 2 + 1];
    double fsl, ab;
    factors(k, fsl, ab);
    const double adr = ab * Dg;  // :617-621
    const double adf = A - adr;  // :628
    __builtin_nontemporal_store(A, a.aI + ob + i);
    __builtin_nontemporal_store(adf * fsl + adr, a.aI_sl + ob + i);  // :631-633
    __builtin_nontemporal_store(adf * (1 - fsl), a.aI_sh + ob + i);
    if constexpr (PROF) __builtin_nontemporal_store(adr, a.aI_dr + ob + i);
  }
  if constexpr (PROF) {  // band-integrated level profiles (diagnostics.py:81): lev = [nz][NGT][3] level sums of I_dr, I_df_d, I_df_u
    const double invmu = 1.0 / cos(a.psi[c]);
    const long long lb = (long long)c * a.nz * ng;
    for (int i = l; i < a.nz * ng; i += nlanes) {
      const int j = i / ng, g = i - j * ng;
      const double* q = lev + (j * NGT + g) * 3;
      store_level_profiles(a, lb + i, q[0], q[1], q[2], invmu, false);
    }
  }
  if (a.totals && l < 4 * ng) {  // incoming, reflected, transmitted, soil-reflected
    const int g = l >> 2, q = l & 3;
    a.totals[((long long)c * ng + g) * 4 + q] = ends[(q < 2 ? 2 * NGT : 0) + 2 * g + (q & 1)];
  }
}

// LDS of one column of k_absorb_bandsum_w / _h, in doubles: raw[nl][ngt][2] (A_g(k), D_g(k)) from 0, ends[2][ngt][2] (ground, then top:
// I_d, I_df_u), and with the level profiles lev[nz][ngt][3] (level sums of I_dr, I_df_d, I_df_u).  The kernels carve it up and the
// launchers size it from here.
struct ColLds { int ends, lev, total; };
__host__ __device__ constexpr ColLds col_lds(int ngt, int nz, bool prof) {
  const int ends = 2 * ngt * (nz - 1), lev = ends + 4 * ngt;
  return {ends, lev, lev + (prof ? 3 * ngt * nz : 0)};
}

// What k_absorb_bandsum_w and k_absorb_bandsum_h share: a column's bands spread over LANES lanes (lane l owns bands l, l + LANES, ...:
// NBT of them), the levels taken in chunks of CH, the band sums formed by `sum` (WaveSum over a wave, HalfSum over each half).
// Plain `inline`, not forced: the regular inliner takes every one of them into its kernel (no call is left in the code object) and gives
// the registers of the kernels' former own copies within 3; forced inlining cost up to 36 registers and k_absorb_bandsum_w<double, 6, 1, 4>
// with profiles a wave per SIMD.
struct WaveSum {
  template <int N>
  __device__ void operator()(const double (&v)[N], double* dst, int nvalid, int lane) const { wave_sum_store(v, dst, nvalid, lane); }
};
struct HalfSum {
  template <int N>
  __device__ void operator()(const double (&v)[N], double* dst, int nvalid, int lane) const { half_sum_store(v, dst, nvalid, lane); }
};
template <int NBT, int NGT>
struct BandLane {  // a lane's bands: index, weights (NGT >= ngroup: weight registers for the groups in use only), 1 - r - t, the level below
  int bi[NBT];
  double w[NBT][NGT], la[NBT], r0[NBT], d0[NBT], u0[NBT];
};
template <int CH, int NBT>
struct Chunk {  // CH levels of the three profiles
  double r[CH][NBT], d[CH][NBT], u[CH][NBT];
};
// the column head: weights, leaf optics and row 0 of column c
template <int LANES, typename TIO, int NBT, int NGT>
__device__ inline void band_head(BandLane<NBT, NGT>& s, const EpiArgsT<TIO>& a, int c, int l, const TIO* __restrict__ R,
                                          const TIO* __restrict__ D, const TIO* __restrict__ U) {
  const int nb = a.nb, ng = a.ngroup;
#pragma unroll
  for (int i = 0; i < NBT; ++i) {
    const int b = l + LANES * i;
    const bool act = b < nb;
    s.bi[i] = act ? b : 0;
    const long long ib = (long long)c * a.col_stride + s.bi[i];
    s.la[i] = act ? 1 - ((double)a.leaf_r[ib] + (double)a.leaf_t[ib]) : 0.0;  // :584
#pragma unroll
    for (int g = 0; g < NGT; ++g) s.w[i][g] = (g < ng && act) ? a.band_w[(long long)g * nb + s.bi[i]] : 0.0;
    s.r0[i] = R[s.bi[i]];
    s.d0[i] = D[s.bi[i]];
    s.u0[i] = U[s.bi[i]];
  }
}
// sum_b w (I_dr + I_df_d), sum_b w I_df_u of the level held in r0, d0, u0
template <class Sum, int NBT, int NGT>
__device__ inline void band_end_terms(const BandLane<NBT, NGT>& s, Sum sum, double* dst, int lane) {
  double v[2 * NGT];
#pragma unroll
  for (int g = 0; g < NGT; ++g) {
    v[2 * g] = v[2 * g + 1] = 0.0;
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
      v[2 * g] += s.w[i][g] * (s.r0[i] + s.d0[i]);
      v[2 * g + 1] += s.w[i][g] * s.u0[i];
    }
  }
  sum(v, dst, 2 * NGT, lane);
}
// sum_b w I_dr, sum_b w I_df_d, sum_b w I_df_u of one row (r, d, u) for every group: v[3 g + 0 .. 2]; zeros for a row that is not `on`
template <int NBT, int NGT>
__device__ inline void level_sums(const double (&w)[NBT][NGT], const double (&r)[NBT], const double (&d)[NBT], const double (&u)[NBT], double* v,
                                  bool on = true) {
#pragma unroll
  for (int g = 0; g < NGT; ++g) {
    v[3 * g] = v[3 * g + 1] = v[3 * g + 2] = 0.0;
#pragma unroll
    for (int i = 0; on && i < NBT; ++i) {
      v[3 * g] += w[i][g] * r[i];
      v[3 * g + 1] += w[i][g] * d[i];
      v[3 * g + 2] += w[i][g] * u[i];
    }
  }
}
// a chunk = CH levels from k0 + 1: `band_fetch` issues its loads, `band_reduce` forms the level terms and the band sums and moves on
template <typename TIO, int CH, int NBT, int NGT>
__device__ inline void band_fetch(const BandLane<NBT, NGT>& s, Chunk<CH, NBT>& x, const TIO* __restrict__ R, const TIO* __restrict__ D,
                                           const TIO* __restrict__ U, int nb, int nl, int k0) {
  const int nlev = min(CH, nl - k0);
#pragma unroll
  for (int t = 0; t < CH; ++t)
    if (t < nlev) {
      const unsigned row = (unsigned)(k0 + t + 1) * (unsigned)nb;  // nz * nb < 2^31 (checked by the launcher)
#pragma unroll
      for (int i = 0; i < NBT; ++i) {
        const unsigned off = row + (unsigned)s.bi[i];
        x.r[t][i] = __builtin_nontemporal_load(R + off);
        x.d[t][i] = __builtin_nontemporal_load(D + off);
        x.u[t][i] = __builtin_nontemporal_load(U + off);
      }
    }
}
template <class Sum, int CH, int NBT, int NGT>
__device__ inline void band_reduce(BandLane<NBT, NGT>& s, const Chunk<CH, NBT>& x, Sum sum, double* raw, int nl, int k0, int lane) {
  const int nlev = min(CH, nl - k0);
  double v[CH * NGT * 2];  // [t][g][A, D]
#pragma unroll
  for (int t = 0; t < CH; ++t) {
#pragma unroll
    for (int g = 0; g < NGT; ++g) v[(t * NGT + g) * 2] = v[(t * NGT + g) * 2 + 1] = 0.0;
    if (t < nlev) {
#pragma unroll
      for (int i = 0; i < NBT; ++i) {
        const double av = x.r[t][i] - s.r0[i] + x.d[t][i] - s.d0[i] + s.u0[i] - x.u[t][i];  // :609
        const double ar = s.la[i] * x.r[t][i];                                              // :617-621 without the level factor
#pragma unroll
        for (int g = 0; g < NGT; ++g) {
          v[(t * NGT + g) * 2] += s.w[i][g] * av;
          v[(t * NGT + g) * 2 + 1] += s.w[i][g] * ar;
        }
        s.r0[i] = x.r[t][i];
        s.d0[i] = x.d[t][i];
        s.u0[i] = x.u[t][i];
      }
    }
  }
  sum(v, raw + (size_t)k0 * NGT * 2, nlev * NGT * 2, lane);
}

// k_absorb_bandsum_w: the same pass with ONE WAVE PER COLUMN (nb <= 512): lane l owns bands l, l + 64, ... (NBT of them), so
// the cross-band reduction of a level costs one set of lane exchanges per COLUMN instead of one per wave of a multi-wave
// workgroup -- the kernel above spends most of its instructions there (2 ngroup reductions x 18 VALU instructions x 5 waves per
// level at nb = 300: VALU-bound at 2.1 TB/s, measured) -- and the exchanges themselves reduce FOUR values at a time (wave_sum4,
// crt_internal.hpp: 5 instructions per value instead of 18).  No barriers, no cross-wave traffic: the waves of a workgroup are
// independent columns.  The raw band sums A_g(k), D_g(k) go to LDS; at the end the lanes turn them into the level outputs
// (level factors f_sl(k), 1 - e^{-K_b dlai_k} evaluated there, lanes over levels) and write them coalesced.
template <typename TIO, int NBT, int CH, int NGT, bool PF = false, bool PROF = false>
__global__ __launch_bounds__(256) void k_absorb_bandsum_w(EpiArgsT<TIO> a, int wpb, int per_wave) {
  extern __shared__ double lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // wave-uniform column index in a scalar register: the profile pointers below then are scalar bases, and every load is
  // "scalar base + one 32-bit lane offset" shared by the three arrays (15 offset registers instead of 90 address registers)
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + wave);
  if (c >= a.ncol) return;  // (no workgroup barrier anywhere in this kernel)
  const int nz = a.nz, nb = a.nb, nl = nz - 1;
  const ColLds L = col_lds(NGT, nz, PROF);
  double* raw = lds + (size_t)wave * per_wave;
  double* ends = raw + L.ends;
  double* lev = raw + L.lev;
  const long long cb = (long long)c * nz * nb;
  const TIO* __restrict__ R = a.I_dr + cb;
  const TIO* __restrict__ D = a.I_df_d + cb;
  const TIO* __restrict__ U = a.I_df_u + cb;
  BandLane<NBT, NGT> s;
  band_head<64>(s, a, c, lane, R, D, U);
  const double Kb = column_kb(a, c);  // now, not in the tail: three dependent round trips with nothing else of the wave in flight there
  if (a.totals) band_end_terms(s, WaveSum{}, ends, lane);  // ground: transmitted I_d[0], soil-reflected I_df_u[0]  (diagnostics.py:476-530)
  if constexpr (PROF) {  // level sums of row 0
    double v[3 * NGT];
    level_sums(s.w, s.r0, s.d0, s.u0, v);
    wave_sum_store(v, lev, 3 * NGT, lane);
  }
  auto fetch = [&](int k0, Chunk<CH, NBT>& x) { band_fetch(s, x, R, D, U, nb, nl, k0); };
  auto reduce = [&](int k0, const Chunk<CH, NBT>& x) {
    band_reduce(s, x, WaveSum{}, raw, nl, k0, lane);
    if constexpr (PROF) {  // the level sums of rows k0 + 1 .. k0 + nlev
      const int nlev = min(CH, nl - k0);
      double v3[CH * NGT * 3];
#pragma unroll
      for (int t = 0; t < CH; ++t) level_sums(s.w, x.r[t], x.d[t], x.u[t], v3 + t * NGT * 3, t < nlev);
      wave_sum_store(v3, lev + (size_t)(k0 + 1) * NGT * 3, nlev * NGT * 3, lane);
    }
  };
  if constexpr (PF) {
    // narrow spectra (one band per lane): a chunk is only CH rows of nb * 8 bytes per array, too little in flight to cover the
    // HBM latency at the occupancy the registers allow -> the next chunk's loads are issued before this chunk is reduced
    Chunk<CH, NBT> xa, xb;
    fetch(0, xa);
    for (int k0 = 0; k0 < nl; k0 += 2 * CH) {
      if (k0 + CH < nl) fetch(k0 + CH, xb);
      reduce(k0, xa);
      if (k0 + CH < nl) {
        if (k0 + 2 * CH < nl) fetch(k0 + 2 * CH, xa);
        reduce(k0 + CH, xb);
      }
    }
  } else {
    for (int k0 = 0; k0 < nl; k0 += CH) {
      Chunk<CH, NBT> x;
      fetch(k0, x);
      reduce(k0, x);
    }
  }
  if (a.totals) band_end_terms(s, WaveSum{}, ends + 2 * NGT, lane);  // canopy top: incoming I_d[top], reflected I_df_u[top]
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave: LDS operations complete in order; make the sums visible to all lanes
  bandsum_finish<NGT, PROF>(a, c, raw, ends, ExpFactors{a.lai + (long long)c * nz, Kb}, lane, 64, lev);
}

// k_absorb_bandsum_l: narrow spectra (32 < nb <= 48, even; nz <= 257): one wave per column, the lanes over LAYERS.
//   * lanes over layers: in the kernel above a narrow spectrum leaves lanes idle and still pays the full cross-lane reduction per
//     level.  Here a slab of LS + 1 = 17 consecutive rows of the three profiles is staged in LDS as the flat copy of its global run
//     (16-byte loads into registers -- issued one slab ahead, in flight while the previous slab is reduced -- then 16-byte LDS
//     writes) and lane (t = lane & 15, p = lane >> 4) sums layer k0 + t over the bands p, p + 4, ... serially; what is left of the
//     reduction is the sum over the four p, four values per set of six lane swaps.
//     Rows are nbp = nb or nb + 2 doubles apart in LDS, whichever is 2 (mod 4): the 16 layers of a read fall into 16 bank groups.
//   * the head and the tail of a column have nothing in flight to hide behind, so they are kept short: everything the column needs
//     (first slab, LAI levels, leaf optics, geometry) is requested in one go, the level factors (two exponentials per layer) are
//     formed while the second slab is in flight, and the tail is LDS reads, three multiply-adds and streaming stores.
//     Measured per column at 1e5 x 38 x 100 before that (wall_clock64 stamps): first slab after 7.7 us (three dependent round
//     trips), 3.3 us per further slab, then 2.2 + 2.6 + 0.9 us (last reduction, tail arithmetic, store acknowledgement).
//     (A persistent form -- waves walking columns w, w + G, ... with the next column's first slab prefetched -- was tried: the
//     loop-carried state costs 316 registers, one wave per SIMD, 3.3 ms instead of 2.0; capped at 256 it spills, 2.3 ms.)
//   * float storage (TIO = float): the same pieces of two bands, 8 bytes per lane, widened to d2 as they go to LDS.  A column of
//     nz * nb floats starts on an 8-byte boundary only (nz * nb is even, not a multiple of four), and the layer sums must keep the fp64
//     kernel's order (f32 band sums are the f64 band sums of the upcast profiles, bit for bit).
constexpr int LAYER_LS = 16;  // layers per slab
// LDS of k_absorb_bandsum_l, in doubles: slab[3][LS + 1][nbp] from 0 (ss = one array's slab), wts[ngt + 1][nbp] (the groups' band weights,
// then 1 - (leaf_r + leaf_t) of the column), raw[nl][ngt][2] (A_g(k), D_g(k)), ends[2][ngt][2], lai[nz], lvl[nl][2] (f_sl(k),
// 1 - e^{-K_b dlai_k}).  The kernel carves it up and the launcher sizes it from here.
struct LayerLds { int ss, wts, raw, ends, lai, lvl, total; };
__host__ __device__ constexpr LayerLds layer_lds(int ngt, int nz, int nbp) {
  const int nl = nz - 1, ss = (LAYER_LS + 1) * nbp;
  const int wts = 3 * ss, raw = wts + (ngt + 1) * nbp, ends = raw + 2 * ngt * nl, lai = ends + 4 * ngt, lvl = lai + nz;
  return {ss, wts, raw, ends, lai, lvl, lvl + 2 * nl};
}

template <typename TIO, int NGT>
__global__ __launch_bounds__(64) void k_absorb_bandsum_l(EpiArgsT<TIO> a, int nbp) {
  typedef TIO tio2 __attribute__((ext_vector_type(2)));  // one piece: two bands of a row
  constexpr int LS = LAYER_LS, NP = 4, NLD = 9;  // NLD 16-byte loads per lane cover 17 rows of <= 64 bands: 17 * 32 <= 9 * 64
  constexpr int NLAI = 5;                        // LAI levels per lane: nz <= 64 * 4 + 1 (the launcher checks)
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int nz = a.nz, nb = a.nb, ng = a.ngroup, nl = nz - 1, nb2 = nb >> 1;
  const LayerLds L = layer_lds(NGT, nz, nbp);
  const int SS = L.ss;
  double* slab = lds;
  double* wts = lds + L.wts;
  double* raw = lds + L.raw;
  double* ends = lds + L.ends;
  double* lai_s = lds + L.lai;
  double* lvl = lds + L.lvl;
  // where this lane's i-th 16-byte piece of a slab goes in LDS (the same for every slab): piece lane + 64 i of the flat run
  int dst[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int idx = lane + 64 * i;
    const int row = idx / nb2;
    dst[i] = row * nbp + 2 * (idx - row * nb2);
  }
  const int t = lane & 15, p = lane >> 4;
  const int slot = wave_sum4_slot(p);
  const bool band_lane = lane < nb;
  // registers of the slab in flight, and of the column it opens (only loaded with a column's first slab)
  tio2 sr[NLD], sd[NLD], su[NLD];
  double c_lr = 0.0, c_lt = 0.0, c_lai[NLAI], c_psi = 0.0, c_gp = 0.0, c_ga = 0.0;
  int c_kind = 0;
  const int c = blockIdx.x;
  auto fetch = [&](int k0) {
    const long long cb2 = (long long)c * nz * nb2;
    const tio2* __restrict__ R2 = reinterpret_cast<const tio2*>(a.I_dr) + cb2;
    const tio2* __restrict__ D2 = reinterpret_cast<const tio2*>(a.I_df_d) + cb2;
    const tio2* __restrict__ U2 = reinterpret_cast<const tio2*>(a.I_df_u) + cb2;
    const int n2 = (min(LS, nl - k0) + 1) * nb2;
    const unsigned base = (unsigned)k0 * (unsigned)nb2;  // nz * nb < 2^31 (checked by the launcher)
#pragma unroll
    for (int i = 0; i < NLD; ++i)
      if (lane + 64 * i < n2) {
        sr[i] = __builtin_nontemporal_load(R2 + base + lane + 64 * i);
        sd[i] = __builtin_nontemporal_load(D2 + base + lane + 64 * i);
        su[i] = __builtin_nontemporal_load(U2 + base + lane + 64 * i);
      }
    if (k0 == 0) {
      const long long ib = (long long)c * a.col_stride + (band_lane ? lane : 0);
      c_lr = a.leaf_r[ib];
      c_lt = a.leaf_t[ib];
#pragma unroll
      for (int j = 0; j < NLAI; ++j) c_lai[j] = a.lai[(long long)c * nz + min(lane + 64 * j, nz - 1)];
      c_psi = a.psi[c];
      c_kind = a.g_kind[c];
      c_gp = a.g_param ? a.g_param[c] : 0.0;
      c_ga = a.g_at_psi ? a.g_at_psi[c] : 0.0;
    }
  };
  auto end_terms = [&](int row, double* out) {  // sum_b w (I_dr + I_df_d), sum_b w I_df_u of slab row `row`
    double v[2 * NGT];
    const int o = row * nbp + (band_lane ? lane : 0);
    const double rd = band_lane ? slab[o] + slab[SS + o] : 0.0, uu = band_lane ? slab[2 * SS + o] : 0.0;
#pragma unroll
    for (int g = 0; g < NGT; ++g) {
      const double wg = wts[g * nbp + (band_lane ? lane : 0)];
      v[2 * g] = wg * rd;
      v[2 * g + 1] = wg * uu;
    }
    wave_sum_store(v, out, 2 * NGT, lane);
  };
  fetch(0);  // first: everything below queues up behind it
  {  // band weights: all requested at once (a load inside `g < ng ? ... : 0` is waited for before the next one is issued)
    double wv[NGT];
#pragma unroll
    for (int g = 0; g < NGT; ++g) wv[g] = a.band_w[(long long)min(g, ng - 1) * nb + (band_lane ? lane : 0)];
    if (band_lane) {
#pragma unroll
      for (int g = 0; g < NGT; ++g) wts[g * nbp + lane] = g < ng ? wv[g] : 0.0;
    }
  }
  for (int k0 = 0; k0 < nl; k0 += LS) {
    const int nr = min(LS, nl - k0);
    {  // the slab in flight -> LDS
      const int n2 = (nr + 1) * nb2;
#pragma unroll
      for (int i = 0; i < NLD; ++i)
        if (lane + 64 * i < n2) {
          *reinterpret_cast<d2*>(slab + dst[i]) = __builtin_convertvector(sr[i], d2);
          *reinterpret_cast<d2*>(slab + SS + dst[i]) = __builtin_convertvector(sd[i], d2);
          *reinterpret_cast<d2*>(slab + 2 * SS + dst[i]) = __builtin_convertvector(su[i], d2);
        }
    }
    if (k0 == 0) {  // ... and the column it opens
      if (band_lane) wts[NGT * nbp + lane] = 1 - (c_lr + c_lt);  // :584
#pragma unroll
      for (int j = 0; j < NLAI; ++j)
        if (lane + 64 * j < nz) lai_s[lane + 64 * j] = c_lai[j];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave: LDS operations complete in order; the slab is visible to all lanes
    if (k0 + LS < nl) fetch(k0 + LS);  // the next slab is in flight while this one is reduced
    if (k0 == 0) {  // level factors of the column (model.py:601-602, 617-621), lanes over layers
      const double Kb = column_kb(c_kind, c_gp, c_ga, c_psi);
      for (int k = lane; k < nl; k += 64) {
        const double l0 = lai_s[k], l1 = lai_s[k + 1];
        lvl[2 * k] = exp(-Kb * ((l0 + l1) / 2));
        lvl[2 * k + 1] = 1 - exp(-Kb * (l0 - l1));
      }
      if (a.totals) end_terms(0, ends);  // ground: transmitted I_d[0], soil-reflected I_df_u[0]  (diagnostics.py:476-530)
    }
    double v[2 * NGT];
#pragma unroll
    for (int j = 0; j < 2 * NGT; ++j) v[j] = 0.0;
    if (t < nr) {
      const double* r0p = slab + t * nbp;
      for (int b = p; b < nb; b += NP) {
        const double r0 = r0p[b], r1 = r0p[nbp + b];
        const double d0 = r0p[SS + b], d1 = r0p[SS + nbp + b];
        const double u0 = r0p[2 * SS + b], u1 = r0p[2 * SS + nbp + b];
        const double av = r1 - r0 + d1 - d0 + u0 - u1;  // :609
        const double ar = wts[NGT * nbp + b] * r1;       // :617-621 without the level factor
#pragma unroll
        for (int g = 0; g < NGT; ++g) {
          const double wg = wts[g * nbp + b];
          v[2 * g] += wg * av;
          v[2 * g + 1] += wg * ar;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < (2 * NGT + 3) / 4; ++j) {  // sum over the four p: afterwards DPP row p holds value 4 j + slot of its layer
      const double z = swap_add16(swap_add32(v[4 * j], 4 * j + 1 < 2 * NGT ? v[4 * j + 1] : 0.0),
                                  swap_add32(4 * j + 2 < 2 * NGT ? v[4 * j + 2] : 0.0, 4 * j + 3 < 2 * NGT ? v[4 * j + 3] : 0.0));
      if (t < nr && 4 * j + slot < 2 * NGT) raw[(k0 + t) * NGT * 2 + 4 * j + slot] = z;
    }
    if (k0 + LS >= nl) {  // the column is complete
      if (a.totals) end_terms(nr, ends + 2 * NGT);  // canopy top: incoming I_d[top], reflected I_df_u[top]
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      bandsum_finish<NGT>(a, c, raw, ends, [lvl](int k, double& fsl, double& ab) { fsl = lvl[2 * k], ab = lvl[2 * k + 1]; }, lane, 64);
    }
  }
}

// k_absorb_bandsum_h: very narrow spectra (nb <= 32): a column per HALF wave (lane l of a
// half owns band l), so a wave instruction serves two columns instead of leaving half of the lanes idle;
// the reductions stay inside the halves (half_sum2).  Otherwise the same pass.
template <typename TIO, int NBT, int CH, int NGT>
__global__ __launch_bounds__(256) void k_absorb_bandsum_h(EpiArgsT<TIO> a, int wpb, int per_col) {
  extern __shared__ double lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int c0 = 2 * (blockIdx.x * wpb + wave);
  if (c0 >= a.ncol) return;  // wave-uniform; no workgroup barrier in this kernel
  const bool colok = c0 + half < a.ncol;
  const int c = colok ? c0 + half : c0;  // a missing second column repeats the first and writes nothing
  const int nz = a.nz, nb = a.nb, nl = nz - 1;
  double* raw = lds + (size_t)(2 * wave + half) * per_col;
  double* ends = raw + col_lds(NGT, nz, false).ends;
  const long long cb = (long long)c * nz * nb;
  const TIO* __restrict__ R = a.I_dr + cb;
  const TIO* __restrict__ D = a.I_df_d + cb;
  const TIO* __restrict__ U = a.I_df_u + cb;
  BandLane<NBT, NGT> s;
  band_head<32>(s, a, c, l, R, D, U);
  if (a.totals) band_end_terms(s, HalfSum{}, ends, lane);
  for (int k0 = 0; k0 < nl; k0 += CH) {
    Chunk<CH, NBT> x;
    band_fetch(s, x, R, D, U, nb, nl, k0);
    band_reduce(s, x, HalfSum{}, raw, nl, k0, lane);
  }
  if (a.totals) band_end_terms(s, HalfSum{}, ends + 2 * NGT, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (!colok) return;
  bandsum_finish<NGT>(a, c, raw, ends, ExpFactors{a.lai + (long long)c * nz, column_kb(a, c)}, l, 32);
}

// ------------------------------------------------------------------------------------------
// crt_hip_bandsum_finish_f64: the band-sum outputs that are NOT all-reduced by the band partition (crt1d_amd/dist.py), re-formed in
// one pass from the reduced ones: aI = aI_sl + aI_sh (model.py:633-635), and per level F and I_d from the level sums of I_dr, I_df_d,
// I_df_u through store_level_profiles with invmu = 1 / cos(psi) as the epilogue forms it -- so F and I_d are the bits the epilogue
// writes for the same sums.  One wave per column (invmu once per column), lanes over (level, group): every access is coalesced; the
// outputs are not read again here (streaming stores).  Waves stride over the columns.
constexpr int FIN_WPB = 4;

__global__ __launch_bounds__(64 * FIN_WPB) void k_bandsum_finish(FinishArgs a) {
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * FIN_WPB;
  const int nl = (a.nz - 1) * a.ngroup, nv = a.nz * a.ngroup;
  for (int c = __builtin_amdgcn_readfirstlane(blockIdx.x * FIN_WPB + (threadIdx.x >> 6)); c < a.ncol; c += nwaves) {
    const double invmu = 1.0 / cos(a.psi[c]);  // as k_absorb_bandsum / bandsum_finish
    const long long ol = (long long)c * nl, ov = (long long)c * nv;
    for (int i = lane; i < nl; i += 64)
      __builtin_nontemporal_store(__builtin_nontemporal_load(a.aI_sl + ol + i) + __builtin_nontemporal_load(a.aI_sh + ol + i), a.aI + ol + i);
    for (int i = lane; i < nv; i += 64) {
      const double R = __builtin_nontemporal_load(a.L_dr + ov + i), Dn = __builtin_nontemporal_load(a.L_dn + ov + i),
                   Up = __builtin_nontemporal_load(a.L_up + ov + i);
      store_level_profiles<false>(a, ov + i, R, Dn, Up, invmu, false);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Per-band layer absorption, model.py:573-647: the seven (nz-1, nb) arrays + laim, f_slm of the reference's
// `Model.absorption` dict (AbsArgsT, epilogue.hpp).  One workgroup per column, lanes over bands, previous level kept in registers.
template <typename TIO>
__global__ __launch_bounds__(256) void k_absorb(AbsArgsT<TIO> a) {
  const int c = blockIdx.x;
  const int nz = a.nz, nb = a.nb;
  const double Kb = column_kb(a, c);
  const double* lai = a.lai + (long long)c * nz;
  const long long cb = (long long)c * nz * nb;
  const long long cm = (long long)c * (nz - 1) * nb;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const double leaf_a = 1 - ((double)a.leaf_r[(long long)c * a.col_stride + b] + (double)a.leaf_t[(long long)c * a.col_stride + b]);  // :584
    double r0 = a.I_dr[cb + b], d0 = a.I_df_d[cb + b], u0 = a.I_df_u[cb + b];
    for (int k = 0; k < nz - 1; ++k) {
      const long long i1 = cb + (long long)(k + 1) * nb + b;
      const double r1 = a.I_dr[i1], d1 = a.I_df_d[i1], u1 = a.I_df_u[i1];
      const double dl = lai[k] - lai[k + 1];
      const double fsl = exp(-Kb * ((lai[k] + lai[k + 1]) / 2));   // :601-602
      const double av = r1 - r0 + d1 - d0 + u0 - u1;               // :609
      const double adr = r1 * (1 - exp(-Kb * dl)) * leaf_a;        // :617-621
      const double adf = av - adr;                                 // :628
      const double adfsl = adf * fsl, adfsh = adf * (1 - fsl);     // :631-632
      const long long o = cm + (long long)k * nb + b;
      a.o[0][o] = av;
      a.o[1][o] = adf;
      a.o[2][o] = adr;
      a.o[3][o] = adfsh;
      a.o[4][o] = adfsl + adr;
      a.o[5][o] = adfsl;
      a.o[6][o] = adfsh;
      if (b == 0) {
        a.laim[(long long)c * (nz - 1) + k] = (lai[k] + lai[k + 1]) / 2;
        a.f_slm[(long long)c * (nz - 1) + k] = fsl;
      }
      r0 = r1;
      d0 = d1;
      u0 = u1;
    }
  }
}

// k_absorb_tile (nb a multiple of V = 16 / sizeof(TIO): 2 doubles or 4 floats; 16-byte aligned arrays): a column's seven outputs are each
// ONE contiguous run of (nz-1) nb elements, so
// the kernel walks the flat element index with 16 bytes per lane -- every wave store is a contiguous, line-aligned 1 KiB whatever nb
// is (with lanes on bands a 300-band row starts and ends inside a 128-B line: 0.50 of the HBM peak).  The three input profiles go
// through an LDS ring of T + 1 rows: each round loads T new rows (one contiguous run per array, 16 bytes per lane), the row on top
// of the previous round stays where it is, so every input byte is read exactly once.  Level factors and (1 - r - t) come from LDS.
// The ring keeps the inputs as stored (TIO); the float form widens a piece to fp64 before any arithmetic.
// LDS of k_absorb_tile: fsl[nl] from 0, absd[nl], la[nb] (offsets in doubles), then the ring [3][T + 1][nb] of TIO; bytes(T, sizeof(TIO))
// is the whole.  The kernel carves it up and the launcher sizes it -- and chooses T -- from here.
struct TileLds {
  int absd, la, ring, nb;
  __host__ __device__ constexpr size_t bytes(int T, size_t tio) const { return ring * sizeof(double) + (size_t)3 * (T + 1) * nb * tio; }
};
__host__ __device__ constexpr TileLds tile_lds(int nz, int nb) { return {nz - 1, 2 * (nz - 1), 2 * (nz - 1) + nb, nb}; }

template <typename TIO>
__global__ __launch_bounds__(256) void k_absorb_tile(AbsArgsT<TIO> a, int T) {
  constexpr int V = 16 / sizeof(TIO), VS = V == 2 ? 1 : 2;  // elements per 16-byte piece, log2
  typedef TIO vio __attribute__((ext_vector_type(V)));
  typedef double dv __attribute__((ext_vector_type(V)));                  // a piece widened to fp64
  typedef double dv16 __attribute__((ext_vector_type(V), aligned(16)));  // ... as it lies in la[] (16-byte aligned for both V)
  extern __shared__ double lds[];
  const int c = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int nz = a.nz, nb = a.nb, nl = nz - 1, nb2 = nb >> VS, NS = T + 1;  // nb2: pieces per row
  const TileLds L = tile_lds(nz, nb);
  double* fsl = lds;
  double* absd = lds + L.absd;
  double* la = lds + L.la;
  vio* ring = reinterpret_cast<vio*>(lds + L.ring);  // [3][NS][nb2]
  const double Kb = column_kb(a, c);
  const double* lai = a.lai + (long long)c * nz;
  for (int k = tid; k < nl; k += nthr) {
    const double lm = (lai[k] + lai[k + 1]) / 2;       // model.py:601
    const double f = exp(-Kb * lm);                    // :602
    fsl[k] = f;
    absd[k] = 1 - exp(-Kb * (lai[k] - lai[k + 1]));    // :619
    a.laim[(long long)c * nl + k] = lm;
    a.f_slm[(long long)c * nl + k] = f;
  }
  for (int b = tid; b < nb; b += nthr)
    la[b] = 1 - ((double)a.leaf_r[(long long)c * a.col_stride + b] + (double)a.leaf_t[(long long)c * a.col_stride + b]);  // :584
  const long long cb = (long long)c * nz * nb, cm = (long long)c * nl * nb;
  const vio* R2 = reinterpret_cast<const vio*>(a.I_dr + cb);
  const vio* D2 = reinterpret_cast<const vio*>(a.I_df_d + cb);
  const vio* U2 = reinterpret_cast<const vio*>(a.I_df_u + cb);
  const int dt = nthr / nb2, dp = nthr - dt * nb2;       // one round of the workgroup advances (dt rows, dp pairs)
  const int t00 = tid / nb2, p00 = tid - t00 * nb2;
  // row 0 of the column into slot 0
  for (int p = tid; p < nb2; p += nthr) {
    ring[p] = R2[p];
    ring[NS * nb2 + p] = D2[p];
    ring[2 * NS * nb2 + p] = U2[p];
  }
  int base = 0;  // ring slot of the row below the current chunk (level k0)
  for (int k0 = 0; k0 < nl; k0 += T) {
    const int nlev = min(T, nl - k0), n2 = nlev * nb2;
    // rows k0+1 .. k0+nlev -> slots base+1 .. base+nlev (mod NS): one contiguous run of nlev * nb elements per array
    {
      const long long g0 = (long long)(k0 + 1) * nb2;
      int t = t00, p = p00;
      for (int i2 = tid; i2 < n2; i2 += nthr) {
        int slot = base + 1 + t;
        if (slot >= NS) slot -= NS;
        const int li = slot * nb2 + p;
        ring[li] = __builtin_nontemporal_load(R2 + g0 + i2);
        ring[NS * nb2 + li] = __builtin_nontemporal_load(D2 + g0 + i2);
        ring[2 * NS * nb2 + li] = __builtin_nontemporal_load(U2 + g0 + i2);
        p += dp;
        t += dt;
        if (p >= nb2) {
          p -= nb2;
          ++t;
        }
      }
    }
    __syncthreads();
    {
      int t = t00, p = p00;
      const long long o0 = (cm >> VS) + (long long)k0 * nb2;
      for (int i2 = tid; i2 < n2; i2 += nthr) {
        int s0 = base + t;
        if (s0 >= NS) s0 -= NS;
        int s1 = s0 + 1;
        if (s1 >= NS) s1 -= NS;
        const int l0 = s0 * nb2 + p, l1 = s1 * nb2 + p;
        const long long o = o0 + i2;
        // a piece widened to fp64 first (no change for doubles), then :609-632 on its V bands at once; narrowed again as it is stored
        const dv r0 = __builtin_convertvector(ring[l0], dv), r1 = __builtin_convertvector(ring[l1], dv);
        const dv d0 = __builtin_convertvector(ring[NS * nb2 + l0], dv), d1 = __builtin_convertvector(ring[NS * nb2 + l1], dv);
        const dv u0 = __builtin_convertvector(ring[2 * NS * nb2 + l0], dv), u1 = __builtin_convertvector(ring[2 * NS * nb2 + l1], dv);
        const double f = fsl[k0 + t], ab = absd[k0 + t];
        const dv l = *reinterpret_cast<const dv16*>(la + V * p);
        const dv av = r1 - r0 + d1 - d0 + u0 - u1;      // :609
        const dv adr = r1 * ab * l;                     // :617-621
        const dv adf = av - adr;                        // :628
        const dv dsl = adf * f, dsh = adf * (1 - f);    // :631-632
        const dv sl = dsl + adr;
        __builtin_nontemporal_store(__builtin_convertvector(av, vio), reinterpret_cast<vio*>(a.o[0]) + o);
        __builtin_nontemporal_store(__builtin_convertvector(adf, vio), reinterpret_cast<vio*>(a.o[1]) + o);
        __builtin_nontemporal_store(__builtin_convertvector(adr, vio), reinterpret_cast<vio*>(a.o[2]) + o);
        __builtin_nontemporal_store(__builtin_convertvector(dsh, vio), reinterpret_cast<vio*>(a.o[3]) + o);
        __builtin_nontemporal_store(__builtin_convertvector(sl, vio), reinterpret_cast<vio*>(a.o[4]) + o);
        __builtin_nontemporal_store(__builtin_convertvector(dsl, vio), reinterpret_cast<vio*>(a.o[5]) + o);
        __builtin_nontemporal_store(__builtin_convertvector(dsh, vio), reinterpret_cast<vio*>(a.o[6]) + o);
        p += dp;
        t += dt;
        if (p >= nb2) {
          p -= nb2;
          ++t;
        }
      }
    }
    base += nlev;
    if (base >= NS) base -= NS;
    lds_barrier();  // all reads of this chunk's slots are done before the next round overwrites them (LDS only: the stores keep flowing)
  }
}

// out[row][g] = sum_b w[g][b] X[row][b]: diagnostics.band's reduction (diagnostics.py:81) for ANY variable with a trailing wavelength
// axis -- one wave per row, lanes over bands, four group totals per set of lane exchanges (wave_sum4)
__global__ __launch_bounds__(256) void k_band_reduce(const double* __restrict__ X, long long nrow, int nb, const double* __restrict__ w, int ng,
                                                     double* __restrict__ out) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= nrow) return;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const double* x = X + row * nb;
  for (int b = lane; b < nb; b += 64) {
    const double v = x[b];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (g < ng) acc[g] += w[(long long)g * nb + b] * v;
  }
  const double z = wave_sum4(acc[0], acc[1], acc[2], acc[3]);
  const int g = wave_sum4_slot(lane >> 4);
  if ((lane & 15) == 0 && g < ng) out[row * ng + g] = z;
}



// ngroup -> NGT, the number of groups a kernel keeps weight registers for: calls f(std::integral_constant<int, NGT>{})
template <class F>
int with_ngt(int ngroup, F f) {
  if (ngroup == 1) return f(std::integral_constant<int, 1>{});
  if (ngroup <= 3) return f(std::integral_constant<int, 3>{});
  return f(std::integral_constant<int, 4>{});
}

// bands per lane -> NBT of k_absorb_bandsum_w: calls f(std::integral_constant<int, NBT>{}); and CH, the levels per chunk at that NBT.  The
// chunk lengths are the measured ones; with the level profiles they are shorter: the extra sums live in registers too.
template <class F>
int with_nbt(int nbt, F f) {
  switch (nbt) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}
constexpr int wave_ch(int nbt, bool prof) { return prof ? (nbt <= 5 ? 2 : 1) : (nbt <= 3 ? 4 : 2); }

// bands [b0, b0 + nbs) of every row by k_absorb_bandsum, in workgroups of nthr threads
template <typename TIO, bool PROF>
int launch_band_slice(const EpiArgsT<TIO>& a, int b0, int nbs, int nthr, hipStream_t s) {
  const int nwave = nthr / 64;
  const size_t sh = ((size_t)2 * BS_CH * nwave * (PROF ? 5 : 2) * MAXG + (size_t)nwave * (4 + (PROF ? 3 : 0)) * MAXG) * sizeof(double);
  const dim3 grid(a.ncol);
  return with_bound(nthr, [&](auto B) { return launch_kernel(k_absorb_bandsum<TIO, B(), PROF>, grid, nthr, sh, s, a, b0, nbs, (int)(b0 > 0)); });
}

}  // namespace

// The launchers of both storage types (TIO = element type of the profiles and leaf optics): the kernel choice depends on the shape and on
// alignment only, so an f32 call takes the form -- and the summation order -- of the f64 call on the upcast profiles.
template <typename TIO>
int launch_bandsum(const EpiArgsT<TIO>& a, hipStream_t s) {
  const bool prof = a.aI_dr != nullptr;  // the six optional outputs come all together or not at all (api.hip checks)
  const bool idx32 = (long long)a.nz * a.nb < (1ll << 31);  // the one-wave kernels index a column with 32 bits
  const int ngt = with_ngt(a.ngroup, [](auto n) { return (int)decltype(n)::value; });
  // measured (tools/epilogue_bench.py): nb = 20: 1.15 ms per wave-column vs 0.85 ms per half-wave-column; nb = 38: 1.11 vs 1.26 (the second band
  // slot of a half is nearly empty and doubles the per-band work) -> halves only up to 32 bands
  // k_absorb_bandsum_l moves pieces of two bands (16 bytes of double, 8 of float): the profiles must be aligned to one piece
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(a.I_dr) | reinterpret_cast<uintptr_t>(a.I_df_d) | reinterpret_cast<uintptr_t>(a.I_df_u)) &
                          (2 * sizeof(TIO) - 1)) == 0;
  // measured (tools/bandsum_shapes.py, 9.1 GB of profiles): lanes over layers vs lanes over bands (one band per lane, next chunk prefetched):
  //   1e5 x 34 x 100: 1.69 vs 1.83 ms;  1e5 x 38 x 100: 1.89 vs 2.09;  1e5 x 48 x 80: 1.85 vs 1.88;  1e5 x 64 x 60: 2.02 vs 1.66 -> up to 48 bands
  // (with the level profiles requested the band-lane kernels below serve every width: they hold each level's values in registers anyway)
  if (!prof && a.nb > 32 && a.nb <= 48 && a.nb % 2 == 0 && aligned16 && a.nz <= 257 && idx32) {  // lanes over layers
    const int nbp = (a.nb % 4 == 2) ? a.nb : a.nb + 2;
    const size_t sh = (size_t)layer_lds(ngt, a.nz, nbp).total * sizeof(double);
    if (sh <= 64 * 1024)
      return with_ngt(a.ngroup, [&](auto n) { return launch_kernel(k_absorb_bandsum_l<TIO, decltype(n)::value>, dim3(a.ncol), 64, sh, s, a, nbp); });
  }
  if (!prof && a.nb <= 32 && idx32) {  // a column per half wave
    const int per_col = col_lds(ngt, a.nz, false).total;
    int wpb = 4;
    while (wpb > 1 && (size_t)2 * wpb * per_col * sizeof(double) > 60 * 1024) wpb >>= 1;
    const size_t sh = (size_t)2 * wpb * per_col * sizeof(double);
    if (sh <= 64 * 1024) {
      const dim3 grid((a.ncol + 2 * wpb - 1) / (2 * wpb));
      return with_ngt(a.ngroup, [&](auto n) {
        return launch_kernel(k_absorb_bandsum_h<TIO, 1, 4, decltype(n)::value>, grid, 64 * wpb, sh, s, a, wpb, per_col);
      });
    }
  }
  if (a.nb <= 512 && idx32) {  // one wave per column
    const int per_wave = col_lds(ngt, a.nz, prof).total;
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * per_wave * sizeof(double) > 60 * 1024) wpb >>= 1;
    const size_t sh = (size_t)wpb * per_wave * sizeof(double);
    if (sh <= 64 * 1024) {
      const dim3 grid((a.ncol + wpb - 1) / wpb);
      return with_ngt(a.ngroup, [&](auto n) {
        return with_nbt((a.nb + 63) / 64, [&](auto nbt) {
          constexpr int NGT = decltype(n)::value, NBT = decltype(nbt)::value;
          if (prof) return launch_kernel(k_absorb_bandsum_w<TIO, NBT, wave_ch(NBT, true), NGT, false, true>, grid, 64 * wpb, sh, s, a, wpb, per_wave);
          // one band per lane: the next chunk prefetched (PF, see the kernel)
          return launch_kernel(k_absorb_bandsum_w<TIO, NBT, wave_ch(NBT, false), NGT, NBT == 1>, grid, 64 * wpb, sh, s, a, wpb, per_wave);
        });
      });
    }
  }
  for (int b0 = 0; b0 < a.nb; b0 += 1024) {  // one launch per 1024 bands (the usual case: one), the later ones adding to the first
    const int nbs = std::min(1024, a.nb - b0);
    const int nthr = ((nbs + 63) / 64) * 64;
    const int st = prof ? launch_band_slice<TIO, true>(a, b0, nbs, nthr, s) : launch_band_slice<TIO, false>(a, b0, nbs, nthr, s);
    if (st != CRT_OK) return st;
  }
  return CRT_OK;
}
template int launch_bandsum<double>(const EpiArgsT<double>&, hipStream_t);
template int launch_bandsum<float>(const EpiArgsT<float>&, hipStream_t);

template <typename TIO>
int launch_absorb(const AbsArgsT<TIO>& a, hipStream_t s) {
  constexpr int V = 16 / sizeof(TIO);  // elements per 16-byte piece of k_absorb_tile
  bool flat = a.nb % V == 0 && a.col_stride % V == 0 && (long long)a.nz * a.nb < (1ll << 31);
  const void* ptrs[] = {a.I_dr, a.I_df_d, a.I_df_u, a.o[0], a.o[1], a.o[2], a.o[3], a.o[4], a.o[5], a.o[6]};
  for (const void* q : ptrs)
    if (reinterpret_cast<uintptr_t>(q) & 15) flat = false;
  // ring of T + 1 rows of the three inputs (TIO): T rows per round, as many as keep the workgroup at ~40 KB of LDS (4 per CU).  The
  // per-band outputs involve no reduction, so the float form may take the longer rounds its 4-byte rows allow.
  const TileLds L = tile_lds(a.nz, a.nb);
  const size_t fixed = (size_t)L.ring * sizeof(double);  // what lies before the ring
  int T = (int)((40 * 1024 - std::min<size_t>(fixed, 40 * 1024)) / (3 * (size_t)a.nb * sizeof(TIO))) - 1;
  T = std::max(1, std::min(T, std::min(16, a.nz - 1)));
  const size_t sh = L.bytes(T, sizeof(TIO));
  if (flat && a.nb >= V && sh <= 64 * 1024) return launch_kernel(k_absorb_tile<TIO>, dim3(a.ncol), 256, sh, s, a, T);
  return launch_kernel(k_absorb<TIO>, dim3(a.ncol), 256, 0, s, a);
}
template int launch_absorb<double>(const AbsArgsT<double>&, hipStream_t);
template int launch_absorb<float>(const AbsArgsT<float>&, hipStream_t);

int launch_bandsum_finish(const FinishArgs& a, hipStream_t s) {
  // 8192 workgroups of four waves fill every CU at full occupancy; more columns than waves are strided
  const int nblk = (int)std::min<long long>(((long long)a.ncol + FIN_WPB - 1) / FIN_WPB, 8192);
  return launch_kernel(k_bandsum_finish, dim3(nblk), 64 * FIN_WPB, 0, s, a);
}

int launch_band_reduce(const double* X, long long nrow, int nb, const double* band_w, int ngroup, double* out, hipStream_t s) {
  return launch_kernel(k_band_reduce, dim3((unsigned)((nrow + 3) / 4)), 256, 0, s, X, nrow, nb, band_w, ngroup, out);  // a wave per row
}

}  // namespace crt
