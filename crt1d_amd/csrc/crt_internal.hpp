// Internal declarations shared by the gfx950 kernels of libcrt1d_hip.so.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "crt1d_hip.h"
#include "crt1d_hip_dlai.h"
#include "crt1d_hip_dleaf.h"
#include "crt1d_hip_grad.h"
#include "crt1d_hip_jac.h"
#include "crt1d_hip_sensjac.h"
#include "crt1d_hip_sensjac_series.h"
#include "crt1d_hip_sensor.h"

namespace crt {

// ------------------------------------------------------------------------------------------
// Per-column record written by the column-precompute kernel (K0) into the caller's workspace
// and staged into LDS by every solve kernel: a 16-double header + nvec vectors of nz doubles.
//
//   header: band-independent scalars the reference computes before its band loop
//   vectors (by scheme):
//     2s, 4s, g77, bf : lai, ekl = exp(-K_b lai)
//     bl              : lai, ekl, tau_d(lai_j)                       (_solve_bl.py:31-37)
//     n79             : tbcum = ekl, 1 - tb, 1 - td, fracsun/(fracsun dlai), 1/(fracsun dlai), fracsha/(fracsha dlai), 1/(1 - td)
//                                                                     (_solve_n79.py:40-59)
//     zq              : ekl                                           (_solve_zq.py:130)
//     zq_pa           : beam fraction on the M computational layers, ekl, interpolation index, weight
//                                                                     (_solve_zq_pa.py:159-168,357-362)
enum RecScalar {
  S_KB = 0,     // K_b = G(psi)/cos(psi)              model.py:291-293
  S_MU = 1,     // cos(psi)
  S_G = 2,      // G(psi)
  S_MUBAR = 3,  // int cos sin / G                     _solve_2s.py:32
  S_GINT1 = 4,  // int_0^{mu_s} G(acos m) dm           _solve_4s.py:148
  S_GINT2 = 5,  // int_{mu_s}^1                        _solve_4s.py:149
  S_DLM = 6,    // |mean(dlai[dlai != 0])|             _solve_zq.py:50
  S_TAUI = 7,   // tau_d(dlai_mean)                    _solve_zq.py:51
  S_TPSI = 8,   // exp(-K_b dlai_mean)                 _solve_zq.py:52
  S_COS2 = 9,   // cos^2(radians(mla))                 _solve_2s.py:28,68
  S_LT = 10,    // lai[0], total LAI
  S_INVMU = 11, // 1/cos(psi)
  S_UNIF = 12,  // 1.0 when every dlai_j equals S_DL to within 4 ulp of LAI (all reference LAI generators), else 0.0
  S_DL = 13,    // (lai[0] - lai[nz-1]) / (nz - 1)
  S_M = 14,     // zq_pa: number of computational layers min(100, nz)   _solve_zq_pa.py:95
  REC_HDR = 16
};

__host__ __device__ inline int rec_nvec(int scheme) {
  switch (scheme) {
    case CRT_SCHEME_BL: return 3;
    case CRT_SCHEME_N79: return 7;
    case CRT_SCHEME_ZQ_PA: return 4;
    case CRT_SCHEME_ZQ: return 1;
    default: return 2;
  }
}
__host__ __device__ inline int rec_len(int scheme, int nz) { return REC_HDR + rec_nvec(scheme) * nz; }

// ------------------------------------------------------------------------------------------
// kernel argument blocks (passed by value)
struct ColArgs {
  int ncol, nz, scheme, tau_d_method;
  double mu_s;
  const double* psi;
  const double* lai;
  const double* mla;
  const int32_t* g_kind;
  const double* g_param;
  const double* g_at_psi;
  const double* g_table;
  double* ws;  // [ncol][rec_len]
};

// Kernel-selection overrides of one call: crt_options.tune with a field per key (include/crt1d_hip.h, enum crt_tune_key), validated by
// check_solve (api.hip).  0 = automatic everywhere.
struct Tune {
  int32_t tile_lds, tile_t, tile_flags, closed_store_waves, closed_pipe_t, pack, pack_compute_waves, reserved7;
  int32_t tri_m, tri_t, tri_family, tri_store_waves, min_tile_nb, flat_flush, reserved14, k0_separate;
  // smallest nb that takes the tile / pipeline kernels: CRT_TUNE_MIN_TILE_NB, or the launcher's own default when that is 0
  int min_nb(int launcher_default) const { return min_tile_nb > 0 ? min_tile_nb : launcher_default; }
};
// the fields lie in key order, so that SolveArgs keeps the layout it had with int tune[CRT_NTUNE] (and the kernels their ISA)
static_assert(sizeof(Tune) == CRT_NTUNE * sizeof(int32_t), "Tune is crt_options.tune");
static_assert(offsetof(Tune, tile_lds) == 4 * CRT_TUNE_TILE_LDS && offsetof(Tune, tile_t) == 4 * CRT_TUNE_TILE_T &&
                  offsetof(Tune, tile_flags) == 4 * CRT_TUNE_TILE_FLAGS &&
                  offsetof(Tune, closed_store_waves) == 4 * CRT_TUNE_CLOSED_STORE_WAVES &&
                  offsetof(Tune, closed_pipe_t) == 4 * CRT_TUNE_CLOSED_PIPE_T && offsetof(Tune, pack) == 4 * CRT_TUNE_PACK &&
                  offsetof(Tune, pack_compute_waves) == 4 * CRT_TUNE_PACK_COMPUTE_WAVES &&
                  offsetof(Tune, tri_m) == 4 * CRT_TUNE_TRI_M && offsetof(Tune, tri_t) == 4 * CRT_TUNE_TRI_T &&
                  offsetof(Tune, tri_family) == 4 * CRT_TUNE_TRI_FAMILY && offsetof(Tune, tri_store_waves) == 4 * CRT_TUNE_TRI_STORE_WAVES &&
                  offsetof(Tune, min_tile_nb) == 4 * CRT_TUNE_MIN_TILE_NB && offsetof(Tune, flat_flush) == 4 * CRT_TUNE_FLAT_FLUSH &&
                  offsetof(Tune, k0_separate) == 4 * CRT_TUNE_K0_SEPARATE,
              "every field of Tune lies at its key");

// Spectra and output profiles are stored as TIO = double (crt_hip_*_f64) or float (crt_hip_*_f32); the per-column
// geometry, the K0 records and ALL arithmetic are fp64 in both cases (the f32 entry points halve the HBM bytes, they
// do not lower the precision of the solve: results are the fp64 results rounded once to fp32).
struct SolveArgs {
  int ncol, nb, nz, reclen;
  long long col_stride;
  const double* ws;  // K0 records
  const void* I_dr0;
  const void* I_df0;
  const void* leaf_r;
  const void* leaf_t;
  const void* soil_r;
  void* o[7];  // I_dr, I_df_d, I_df_u, F, x0, x1, x2
  double mu_s;
  int f32;     // 0: TIO = double, 1: TIO = float
  Tune tune;   // this call's kernel-selection overrides
};

// name of the solve kernel the last launch_* call of this thread chose (crt_hip_last_kernel; reporting only)
void note_kernel(const char* fmt, ...);
const char* last_kernel();

template <typename TIO>
__device__ inline double ldio(const void* p, long long i) {
  return (double)reinterpret_cast<const TIO*>(p)[i];
}
template <typename TIO>
__device__ inline TIO* outp(void* p) {
  return reinterpret_cast<TIO*>(p);
}

// ------------------------------------------------------------------------------------------
// G(psi) closed forms on device (crt1d/leaf_angle.py:118-202); `cs`, `sn` = cos/sin(psi).
// Ellipsoidal forms use sqrt(x^2 cos^2 + sin^2)/p2 == sqrt(x^2 + tan^2)/p2 * cos, finite at pi/2.
__device__ inline double ellipsoidal_p2(double x) {
  if (x > 1.0) {
    double e = sqrt(1.0 - 1.0 / (x * x));
    return x + log((1.0 + e) / (1.0 - e)) / (2.0 * e * x);
  }
  double e = sqrt(1.0 - x * x);
  return x + asin(e) / e;
}

// G(psi) = G_eval(kind, param, G_den(kind, param), cos psi, sin psi).  G_den is the part that does not depend on the angle
// (the ellipsoidal normalisations); K0 evaluates it once per thread and G_eval at each of its quadrature nodes.
// x^-0.733 as exp(-0.733 log x): ~3 ulp instead of pow's < 1 ulp, a third of its instructions (K0 is bound by exactly these).
__device__ inline double G_den(int kind, double param) {
  switch (kind) {
    case CRT_G_ELLIPSOIDAL: return param == 1.0 ? 0.0 : ellipsoidal_p2(param);
    case CRT_G_ELLIPSOIDAL_APPROX: return param + 1.774 * exp(-0.733 * log(param + 1.182));
    default: return 0.0;
  }
}

__device__ inline double G_eval(int kind, double param, double den, double cs, double sn) {
  switch (kind) {
    case CRT_G_HORIZONTAL: return cs;
    case CRT_G_SPHERICAL: return 0.5;
    case CRT_G_VERTICAL: return 0.63661977236758134308 * sn;  // 2/pi
    case CRT_G_ELLIPSOIDAL: {
      if (param == 1.0) return 0.5;
      return sqrt(param * param * cs * cs + sn * sn) / den;
    }
    case CRT_G_ELLIPSOIDAL_APPROX: return sqrt(param * param * cs * cs + sn * sn) / den;
    case CRT_G_ELLIPSOIDAL_APPROX_BONAN: {
      double chil = fmin(fmax(param, -0.4), 0.6);
      double phi1 = 0.5 - 0.633 * chil - 0.330 * chil * chil;
      double phi2 = 0.877 * (1.0 - 2.0 * phi1);
      return phi1 + phi2 * cs;
    }
    default: return 0.0 / 0.0;
  }
}

__device__ inline double G_closed(int kind, double param, double cs, double sn) {
  return G_eval(kind, param, G_den(kind, param), cs, sn);
}

// ------------------------------------------------------------------------------------------
// Work decomposition of every solve kernel: one lane owns VEC adjacent bands of one column and
// sweeps the canopy levels; consecutive lanes own consecutive bands, so each per-level store of a
// wave is one contiguous 512-B (VEC=1) or 1-KiB (VEC=2) segment of the band-contiguous output.
// A block covers BLOCK consecutive (column, band-group) items, i.e. at most
// (BLOCK-1)/nbv + 2 columns, whose K0 records are contiguous in the workspace and are staged
// into LDS with one coalesced copy.
struct Item {
  int c;          // column
  int b;          // first band
  int c_first;    // first column of this block
  bool active;
};

template <int BLOCK, int VEC>
__device__ inline Item locate(int ncol, int nb) {
  const int nbv = nb / VEC;
  const long long first = (long long)blockIdx.x * BLOCK;
  const long long item = first + threadIdx.x;
  Item it;
  it.c_first = (int)(first / nbv);
  it.active = item < (long long)ncol * nbv;
  const long long itc = it.active ? item : first;
  it.c = (int)(itc / nbv);
  it.b = (int)(itc - (long long)it.c * nbv) * VEC;
  return it;
}

// copy the block's column records global -> LDS (USE_LDS) and return this lane's record base
template <int BLOCK, int VEC, bool USE_LDS>
__device__ inline const double* stage_records(const SolveArgs& a, const Item& it, double* lds) {
  if constexpr (USE_LDS) {
    const int nbv = a.nb / VEC;
    const long long first = (long long)blockIdx.x * BLOCK;
    long long last = first + BLOCK - 1;
    const long long total = (long long)a.ncol * nbv;
    if (last >= total) last = total - 1;
    const int c_last = (int)(last / nbv);
    const int n = (c_last - it.c_first + 1) * a.reclen;
    const double* src = a.ws + (long long)it.c_first * a.reclen;
    for (int i = threadIdx.x; i < n; i += BLOCK) lds[i] = src[i];
    __syncthreads();
    return lds + (it.c - it.c_first) * a.reclen;
  } else {
    return a.ws + (long long)it.c * a.reclen;
  }
}

// streaming (write-once) stores: outputs are never re-read by the kernel
template <typename TIO, int VEC>
__device__ inline void store_stream(TIO* p, const double (&v)[VEC]) {
  if constexpr (VEC == 1) {
    __builtin_nontemporal_store((TIO)v[0], p);
  } else {
    typedef TIO vt __attribute__((ext_vector_type(2)));
    vt t;
    t.x = (TIO)v[0];
    t.y = (TIO)v[1];
    __builtin_nontemporal_store(t, reinterpret_cast<vt*>(p));
  }
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also emits s_waitcnt vmcnt(0), i.e.
// every wave would drain its outstanding global stores (a full HBM write round trip) twice per tile;
// the tile protocol only needs the LDS writes/reads of the other waves to have completed.
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// 1/x for normal, positive-or-negative x well inside the exponent range: hardware seed + two Newton steps
// (<= 1 ulp; skips the scaling / fix-up of the IEEE division sequence, ~5 instructions instead of ~10)
__device__ inline double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
  return r;
}

// ------------------------------------------------------------------------------------------
// Polynomial steps with the coefficient in a SCALAR register.  hipcc (ROCm 7.2) turns a Horner step fma(acc, r, C) whose constant it keeps
// in a VGPR into v_mov_b64 tmp, C + v_fmac_f64 tmp, acc, r -- two issue slots per step (ISA of k_pipe<4s>, round 3: ocml's exp was 35
// VALU instructions, 11 of them such copies).  v_fma_f64 takes one SGPR pair as a source, so the step is ONE instruction when the
// constant is pinned to scalar registers; the asm is not volatile, the compiler still schedules and interleaves it freely.
__device__ __forceinline__ double fma_vvs(double a, double b, double c_uniform) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c_uniform));
  return d;
}
__device__ __forceinline__ double fma_vsv(double a, double c_uniform, double b) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(c_uniform), "v"(b));
  return d;
}
__device__ __forceinline__ double mul_vs(double a, double c_uniform) {
  double d;
  asm("v_mul_f64 %0, %1, %2" : "=v"(d) : "v"(a), "s"(c_uniform));
  return d;
}

// e^x in 18 VALU instructions, <= 1 ulp: k = rint(x log2 e), r = x - k ln2 (two-term Cody-Waite, exact first product for |k| < 2^20),
// e^r = 1 + r + r^2 q(r) with q the degree-9 interpolant of (e^r - 1 - r) / r^2 at the Chebyshev nodes of [-ln2/2, ln2/2] (coefficients
// computed for this file with mpmath at 60 digits and rounded to double: 1.6e-17 relative in exact arithmetic), scaled by v_ldexp_f64 --
// which underflows to 0 and overflows to inf by itself, so no range checks.  NaN in, NaN out.
__device__ __forceinline__ double fexp(double x) {
  const double k = __builtin_rint(mul_vs(x, 1.44269504088896338700e+00));
  double r = fma_vsv(k, -6.93147180369123816490e-01, x);
  r = fma_vsv(k, -1.90821492927058770002e-10, r);
  double q = fma_vvs(r, 0x1.af389ecfc4b9cp-26, 0x1.28917c89a43a7p-22);
  q = fma_vvs(q, r, 0x1.71de0db2f6b19p-19);
  q = fma_vvs(q, r, 0x1.a019b9149a41cp-16);
  q = fma_vvs(q, r, 0x1.a01a01a7c2efep-13);
  q = fma_vvs(q, r, 0x1.6c16c17889ef1p-10);
  q = fma_vvs(q, r, 0x1.11111111109b5p-7);
  q = fma_vvs(q, r, 0x1.5555555553d68p-5);
  q = fma_vvs(q, r, 0x1.5555555555556p-3);
  q = fma_vvs(q, r, 0x1.0000000000001p-1);
  q = __builtin_fma(q, r, 1.0);
  q = __builtin_fma(q, r, 1.0);
  return __builtin_ldexp(q, (int)k);
}

// e^x - 1 without the cancellation of fexp(x) - 1 at small |x|: inside the reduced range (|x| <= ln2 / 2, k = 0) e^x - 1 = x + x^2 q(x) with the
// SAME polynomial q as fexp -- relative error ~1e-16 down to x -> 0 -- and fexp(x) - 1 beyond, where e^x is <= 0.71 or >= 1.41.
// Used where a quantity of the form 1 - e^{-k L} is divided by L afterwards (n79's per-leaf-area absorption at small dlai).
__device__ __forceinline__ double fexpm1(double x) {
  if (__builtin_fabs(x) > 0.34657359027997264) return fexp(x) - 1.0;
  double q = fma_vvs(x, 0x1.af389ecfc4b9cp-26, 0x1.28917c89a43a7p-22);
  q = fma_vvs(q, x, 0x1.71de0db2f6b19p-19);
  q = fma_vvs(q, x, 0x1.a019b9149a41cp-16);
  q = fma_vvs(q, x, 0x1.a01a01a7c2efep-13);
  q = fma_vvs(q, x, 0x1.6c16c17889ef1p-10);
  q = fma_vvs(q, x, 0x1.11111111109b5p-7);
  q = fma_vvs(q, x, 0x1.5555555553d68p-5);
  q = fma_vvs(q, x, 0x1.5555555555556p-3);
  q = fma_vvs(q, x, 0x1.0000000000001p-1);
  return __builtin_fma(x * x, q, x);
}

// sin and cos of a moderate argument (|th| < ~1e6) in ~35 instructions: two-term Cody-Waite reduction by pi/2 (the first product is
// exact in the FMA for |th| < 2^20, the reduced argument is good to ~1.2e-16 absolute) and the minimax polynomials of fdlibm's
// __kernel_sin / __kernel_cos on [-pi/4, pi/4].  Absolute error <= ~2e-16: the oscillatory modes of the four-stream scheme need
// nothing better (ocml's sincos carries a Payne-Hanek path and double-double reduction: ~200 instructions).
__device__ inline void fast_sincos(double th, double& sn, double& cs) {
  const double k = __builtin_rint(mul_vs(th, 0.63661977236758134308));
  double r = fma_vsv(k, -1.57079632679489655800e+00, th);
  r = fma_vsv(k, -6.12323399573676603587e-17, r);
  const double z = r * r;
  double ps = fma_vvs(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = fma_vvs(z, ps, 2.75573137070700676789e-06);
  ps = fma_vvs(z, ps, -1.98412698298579493134e-04);
  ps = fma_vvs(z, ps, 8.33333333332248946124e-03);
  ps = fma_vvs(z, ps, -1.66666666666666324348e-01);
  const double sr = __builtin_fma(z * r, ps, r);
  double pc = fma_vvs(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = fma_vvs(z, pc, -2.75573143513906633035e-07);
  pc = fma_vvs(z, pc, 2.48015872894767294178e-05);
  pc = fma_vvs(z, pc, -1.38888888888741095749e-03);
  pc = fma_vvs(z, pc, 4.16666666666666019037e-02);
  const double cr = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
  const int n = (int)k;
  const bool swap = (n & 1) != 0;
  const double ss = swap ? cr : sr, cc = swap ? sr : cr;
  sn = (n & 2) ? -ss : ss;
  cs = ((n + 1) & 2) ? -cc : cc;
}

// Levels at which the per-level exponentials are re-evaluated exactly when a column has uniform dlai; in between
// they advance by one multiplication (e^{-h(L - dl)} = e^{-hL} e^{h dl}).  At most 7 products since the last exact
// value -> <= 8 ulp; the rule depends on j only, so every kernel variant produces the same bits.
__device__ inline bool exact_level(int j) { return (j & 7) == 0; }

// ------------------------------------------------------------------------------------------
// Integrated-output path (no profiles written): per column and band group g (weights w_g[b], diagnostics.py:81)
//   Phi_g(j) = sum_b w_g[b] (I_dr + I_df_d - I_df_u)(j, b)            net downward flux at level j
//   aI_g(k)  = Phi_g(k+1) - Phi_g(k)                                  == sum_b w_g[b] aI(k, b)      (model.py:609)
//   aI_dr    = (1 - e^{-K_b dlai_k}) e^{-K_b lai_{k+1}} sum_b w_g[b] (1 - r - t)[b] I_dr0[b]       (model.py:617-621;
//              I_dr factorises into band x level, so this needs ONE reduction per column)
//   aI_sl = (aI - aI_dr) f_sl(k) + aI_dr,  aI_sh = (aI - aI_dr)(1 - f_sl(k))                       (model.py:628-634)
// so only ngroup values per level are reduced across the bands (wave shuffles + one LDS pass per column).
constexpr int INT_MAXG = 4;

struct IntArgs {
  const double* lai;     // [ncol][nz]
  const double* band_w;  // [ngroup][nb]
  int ngroup;
  double* aI;            // [ncol][nz-1][ngroup]
  double* aI_sl;
  double* aI_sh;
  double* totals;        // [ncol][ngroup][4]: incoming, reflected, transmitted, soil-reflected (may be NULL)
  // optional, all or none (crt_bandsum_out): direct-beam part of the absorption [ncol][nz-1][ngroup] and the band-integrated level
  // profiles [ncol][nz][ngroup] of I_dr, I_df_d, I_df_u, F, I_d (diagnostics.py:84-91)
  double* aI_dr;
  double* L_dr;
  double* L_dn;
  double* L_up;
  double* L_F;
  double* L_Id;
};

// Sum over each 16-lane DPP row, result in every lane of the row: 4 steps of (2 x v_mov_b32 dpp + v_add_f64), pure VALU
// (a __shfl_xor butterfly over the whole wave goes through ds_bpermute: LDS-crossbar latency on every step, measured
// 1.6 ms per 3e6 solves for the integrated 2s kernel against 1.0 ms for the kernel that writes full profiles).
template <int CTRL>
__device__ inline double dpp_add(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
__device__ inline double row_sum16(double v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  return v;
}
// ... plus row_bcast15 / row_bcast31: the wave total ends up in lane 63 (only that lane is valid)
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_add_rows(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
__device__ inline double wave_sum_lane63(double v) {
  v = row_sum16(v);
  v = dpp_add_rows<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v = dpp_add_rows<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
  return v;
}
// FOUR per-lane values -> their four wave totals in ONE register: the lanes of DPP row 0 end up with sum(a), row 1 with sum(c),
// row 2 with sum(b), row 3 with sum(d).  v_permlane32_swap / v_permlane16_swap (gfx950) exchange half-waves / odd-even rows between
// two registers, so each swap + add halves the number of registers while summing across the halves; one row_sum16 finishes all
// four at once: 2 x 3 + 3 + 12 = 21 VALU instructions for four totals, against 4 x 18 for four wave_sum_lane63.
__device__ inline double swap_add32(double x, double y) {
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(y), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ inline double swap_add16(double x, double y) {
  const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(y), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ inline double wave_sum4(double a, double b, double c, double d) {
  return row_sum16(swap_add16(swap_add32(a, b), swap_add32(c, d)));
}
// index (0..3 = a, b, c, d) of the value whose total a lane of DPP row `row` holds after wave_sum4
__device__ inline int wave_sum4_slot(int row) { return ((row & 1) << 1) | (row >> 1); }
// wave totals of v[0..N) written to dst[0..nvalid) (LDS or global) by the first lane of each row, four values per pass
template <int N>
__device__ inline void wave_sum_store(const double (&v)[N], double* dst, int nvalid, int lane) {
  const int slot = wave_sum4_slot(lane >> 4);
#pragma unroll
  for (int j = 0; j < (N + 3) / 4; ++j) {
    const double z = wave_sum4(v[4 * j], 4 * j + 1 < N ? v[4 * j + 1] : 0.0, 4 * j + 2 < N ? v[4 * j + 2] : 0.0, 4 * j + 3 < N ? v[4 * j + 3] : 0.0);
    const int idx = 4 * j + slot;
    if ((lane & 15) == 0 && idx < nvalid) dst[idx] = z;
  }
}

// TWO per-lane values -> their totals over each HALF of the wave (lanes 0-31 / 32-63), for kernels that give a column to each
// half: lanes of DPP row 0 end up with sum(x) over the lower half, row 1 with sum(y) over the lower half, rows 2 / 3 the same for the
// upper half.  3 + 12 = 15 VALU instructions for two values of two columns.
__device__ inline double half_sum2(double x, double y) { return row_sum16(swap_add16(x, y)); }
template <int N>
__device__ inline void half_sum_store(const double (&v)[N], double* dst, int nvalid, int lane) {  // dst: this lane's half's area
  const int which = (lane >> 4) & 1;
#pragma unroll
  for (int j = 0; j < (N + 1) / 2; ++j) {
    const double z = half_sum2(v[2 * j], 2 * j + 1 < N ? v[2 * j + 1] : 0.0);
    const int idx = 2 * j + which;
    if ((lane & 15) == 0 && idx < nvalid) dst[idx] = z;
  }
}

__device__ inline double wave_sum_all(double v) {  // sum over the 64 lanes (used once per column only)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// LDS layout of the partial sums: nslot = waves (ROWS = false: wave totals, 6 DPP steps per value) or 4 * waves
// (ROWS = true: one partial per 16-lane row, 4 DPP steps per value, 4x the LDS):
//   part[(j * nslot + slot) * INT_MAXG + g];  ends[((e * nslot + slot) * 2 + q) * INT_MAXG + g] with e = 0 ground / 1 top,
//   q = 0 (I_dr + I_df_d) / 1 (I_df_u);  pdr[wave * INT_MAXG + g]
struct IntLds {
  double* part;
  double* ends;
  double* pdr;
  double* lev;   // PROF: [nz][nwave][2][INT_MAXG] wave sums of w I_df_d, w I_df_u per level
  double* pi0;   // PROF: [nwave][INT_MAXG] wave sums of w I_dr0 (I_dr factorises into band x level)
};
// carve the integrated kernels' LDS area (after the record) into its parts
__device__ inline IntLds int_lds_carve(double* base, int nz, int nwave, bool prof) {
  IntLds L;
  L.part = base;
  L.ends = L.part + (size_t)nz * nwave * INT_MAXG;
  L.pdr = L.ends + (size_t)2 * nwave * 2 * INT_MAXG;
  L.lev = L.pdr + (size_t)nwave * INT_MAXG;
  L.pi0 = L.lev + (prof ? (size_t)nz * nwave * 2 * INT_MAXG : 0);
  return L;
}

template <bool ROWS, bool PROF = false>
__device__ inline void int_accumulate(const IntLds& L, int nwave, int wave, int lane, int nz, int j, int ng, const double (&w)[INT_MAXG],
                                      bool active, double idr, double dn, double up) {
  if constexpr (!ROWS) {
    if constexpr (PROF) {  // the level sums of the two diffuse streams (the direct beam's follow from one sum per column)
      const int g2 = wave_sum4_slot(lane >> 4);
      const double dd = active ? dn : 0.0, uu = active ? up : 0.0;
      const double zd = wave_sum4(w[0] * dd, w[1] * dd, w[2] * dd, w[3] * dd);
      const double zu = wave_sum4(w[0] * uu, w[1] * uu, w[2] * uu, w[3] * uu);
      if ((lane & 15) == 0 && g2 < ng) {
        L.lev[((j * nwave + wave) * 2 + 0) * INT_MAXG + g2] = zd;
        L.lev[((j * nwave + wave) * 2 + 1) * INT_MAXG + g2] = zu;
      }
    }
    // wave totals of all (up to four) band groups with ONE wave_sum4: 21 VALU instructions per level instead of 18 per group
    // (w[g] = 0 for g >= ngroup and for inactive lanes)
    const int g = wave_sum4_slot(lane >> 4);
    const bool writer = (lane & 15) == 0 && g < ng;
    const double net = active ? idr + dn - up : 0.0;
    const double z = wave_sum4(w[0] * net, w[1] * net, w[2] * net, w[3] * net);
    if (writer) L.part[(j * nwave + wave) * INT_MAXG + g] = z;
    if (j == 0 || j == nz - 1) {
      const int e = j == 0 ? 0 : 1;
      const double dd = active ? idr + dn : 0.0, uu = active ? up : 0.0;
      const double z0 = wave_sum4(w[0] * dd, w[1] * dd, w[2] * dd, w[3] * dd);
      const double z1 = wave_sum4(w[0] * uu, w[1] * uu, w[2] * uu, w[3] * uu);
      if (writer) {
        L.ends[((e * nwave + wave) * 2 + 0) * INT_MAXG + g] = z0;
        L.ends[((e * nwave + wave) * 2 + 1) * INT_MAXG + g] = z1;
      }
    }
    return;
  }
  const int nslot = ROWS ? nwave * 4 : nwave;
  const int slot = ROWS ? wave * 4 + (lane >> 4) : wave;
  const bool writer = ROWS ? (lane & 15) == 0 : lane == 63;
  auto red = [](double v) { return ROWS ? row_sum16(v) : wave_sum_lane63(v); };
  const double net = active ? idr + dn - up : 0.0;
#pragma unroll
  for (int g = 0; g < INT_MAXG; ++g)
    if (g < ng) {
      const double t = red(w[g] * net);
      if (writer) L.part[(j * nslot + slot) * INT_MAXG + g] = t;
    }
  if (j == 0 || j == nz - 1) {
    const int e = j == 0 ? 0 : 1;
#pragma unroll
    for (int g = 0; g < INT_MAXG; ++g)
      if (g < ng) {
        const double t0 = red(active ? w[g] * (idr + dn) : 0.0);
        const double t1 = red(active ? w[g] * up : 0.0);
        if (writer) {
          L.ends[((e * nslot + slot) * 2 + 0) * INT_MAXG + g] = t0;
          L.ends[((e * nslot + slot) * 2 + 1) * INT_MAXG + g] = t1;
        }
      }
  }
}

// after the sweep (call with all threads of the workgroup): combine the partials and write the column's outputs
template <bool ROWS, bool PROF = false>
__device__ inline void int_finish(const IntLds& L, const IntArgs& ia, int nwave, int nz, int c, double Kb, double invmu = 0.0) {
  __syncthreads();
  if constexpr (PROF) {
    const int ngp = ia.ngroup;
    for (int i = threadIdx.x; i < nz * ngp; i += blockDim.x) {
      const int j = i / ngp, g = i - j * ngp;
      double p0 = 0.0, sD = 0.0, sU = 0.0;
      for (int wv = 0; wv < nwave; ++wv) {
        p0 += L.pi0[wv * INT_MAXG + g];
        sD += L.lev[((j * nwave + wv) * 2 + 0) * INT_MAXG + g];
        sU += L.lev[((j * nwave + wv) * 2 + 1) * INT_MAXG + g];
      }
      const double sR = exp(-Kb * ia.lai[(long long)c * nz + j]) * p0;  // sum_b w I_dr0[b] e^{-K_b lai_j}
      const long long o = ((long long)c * nz + j) * ngp + g;
      ia.L_dr[o] = sR;
      ia.L_dn[o] = sD;
      ia.L_up[o] = sU;
      ia.L_F[o] = sR * invmu + 2 * (sU + sD);
      ia.L_Id[o] = sR + sD;
    }
  }
  const int ng = ia.ngroup, nrow = ROWS ? nwave * 4 : nwave;
  const double* lai = ia.lai + (long long)c * nz;
  for (int i = threadIdx.x; i < (nz - 1) * ng; i += blockDim.x) {
    const int k = i / ng, g = i - k * ng;
    double p0 = 0.0, p1 = 0.0, pd = 0.0;
    for (int r = 0; r < nrow; ++r) {
      p0 += L.part[(k * nrow + r) * INT_MAXG + g];
      p1 += L.part[((k + 1) * nrow + r) * INT_MAXG + g];
    }
    for (int wv = 0; wv < nwave; ++wv) pd += L.pdr[wv * INT_MAXG + g];
    const double dl = lai[k] - lai[k + 1];
    const double fsl = exp(-Kb * ((lai[k] + lai[k + 1]) / 2));       // model.py:601-602
    const double adr = (1 - exp(-Kb * dl)) * exp(-Kb * lai[k + 1]) * pd;  // :617-621
    const double a = p1 - p0;                                          // :609
    const double adf = a - adr;
    const long long o = ((long long)c * (nz - 1) + k) * ng + g;
    ia.aI[o] = a;
    ia.aI_sl[o] = adf * fsl + adr;
    ia.aI_sh[o] = adf * (1 - fsl);
    if constexpr (PROF) ia.aI_dr[o] = adr;
  }
  if (ia.totals) {
    for (int i = threadIdx.x; i < ng * 4; i += blockDim.x) {
      const int g = i >> 2, q = i & 3;  // incoming (top, I_d), reflected (top, up), transmitted (ground, I_d), soil-reflected
      const int e = q < 2 ? 1 : 0, which = q & 1;
      double t = 0.0;
      for (int r = 0; r < nrow; ++r) t += L.ends[((e * nrow + r) * 2 + which) * INT_MAXG + g];
      ia.totals[((long long)c * ng + g) * 4 + q] = t;
    }
  }
}

__host__ __device__ inline size_t int_lds_doubles(int nz, int nwave, bool rows = false, bool prof = false) {
  const size_t nslot = rows ? (size_t)nwave * 4 : (size_t)nwave;
  return (size_t)nz * nslot * INT_MAXG + 2 * nslot * 2 * INT_MAXG + (size_t)nwave * INT_MAXG +
         (prof ? (size_t)nz * nwave * 2 * INT_MAXG + (size_t)nwave * INT_MAXG : 0);
}

// ------------------------------------------------------------------------------------------
// Sun-angle series (crt_hip_integrated_series_f64): nt sun states (psi, I_dr0, I_df0) per column on one canopy.  The workspace holds
//   canopy records  [ncol][canlen]     the K0 record with every entry that does not follow the sun (the sun's slots are placeholders),
//                                      canlen = rec_len (+ SER_XI for zq_pa: the cumulative LAI of its computational interfaces)
//   sun records     [ncol * nt][sunlen] SUN_HDR scalars (K_b, cos psi, G, 1 / cos psi, tau_psi) + sun_nvec(scheme) vectors of nz doubles
// written by k_colpre<canopy> (one workgroup per column) and k_colsun (one wave per (column, t)).  A series kernel assembles the record of
// its (column, t) in LDS from the two (series_step): the scheme objects read the record k_colpre would have written for that sun
// state.  What the series shares is K0 alone: on the solve side a workgroup serves one sun state, as in the per-step kernels.
constexpr int SUN_HDR = 8;
constexpr int SER_XI = 104;
__host__ __device__ inline int sun_nvec(int scheme) {
  switch (scheme) {
    case CRT_SCHEME_N79: return 5;
    case CRT_SCHEME_ZQ_PA: return 2;
    default: return 1;
  }
}
// record vector that sun vector sv fills
__host__ __device__ inline int sun_vec_slot(int scheme, int sv) {
  switch (scheme) {
    case CRT_SCHEME_N79: return sv < 2 ? sv : sv + 1;  // ekl, 1 - tb | fracsun / (fracsun dlai), 1 / (fracsun dlai), fracsha / (fracsha dlai)
    case CRT_SCHEME_ZQ: return 0;                       // ekl
    case CRT_SCHEME_ZQ_PA: return sv;                   // beam fraction of the computational layers, ekl
    default: return 1;                                  // ekl (2s, 4s, bl, g77, bf)
  }
}
__host__ __device__ inline int sun_len(int scheme, int nz) { return SUN_HDR + sun_nvec(scheme) * nz; }
__host__ __device__ inline int can_len(int scheme, int nz) { return rec_len(scheme, nz) + (scheme == CRT_SCHEME_ZQ_PA ? SER_XI : 0); }
// header slot of sun scalar i < 5
__device__ inline int sun_hdr_slot(int i) { return i == 0 ? S_KB : i == 1 ? S_MU : i == 2 ? S_G : i == 3 ? S_INVMU : S_TPSI; }

// sun vector that fills record vector `vec`, or -1 for a canopy vector (the inverse of sun_vec_slot)
__host__ __device__ inline int rec_vec_sun(int scheme, int vec) {
  switch (scheme) {
    case CRT_SCHEME_N79: return vec < 2 ? vec : (vec >= 3 && vec <= 5) ? vec - 1 : -1;
    case CRT_SCHEME_ZQ: return vec == 0 ? 0 : -1;
    case CRT_SCHEME_ZQ_PA: return vec < 2 ? vec : -1;
    default: return vec == 1 ? 0 : -1;
  }
}

struct SeriesArgs {
  int nt, scheme, nz;    // sun states per column, scheme, caller's nz
  int canlen, sunlen;
  const double* can;     // canopy records
  const double* sun;     // sun records
  long long col_stride;  // of I_dr0 / I_df0 (crt_sun_series)
  const void* I_dr0;     // double (crt_sun_series) or float (crt_sun_series_f32: the level series with f32 storage)
  const void* I_df0;
};

// sun-record form of K0 (colpre.hip): ca.psi / ca.g_at_psi are [ncol][nt], ca.ws the canopy records, `sun` the sun records
int launch_colpre_series(const ColArgs& ca, int nt, double* sun, hipStream_t s);

// Grid of a series kernel: one workgroup per (column, t).  The column is blockIdx.x, as in the per-step kernels; t = blockIdx.z * gridDim.y +
// blockIdx.y, so that any nt fits (65535 x 65535 states per column).
inline dim3 series_grid(int ncol, int nt) {
  const unsigned gy = nt < 65535 ? (unsigned)nt : 65535u;
  return dim3((unsigned)ncol, gy, (unsigned)((nt + (long long)gy - 1) / gy));
}

// n-point Gauss-Legendre on (0, 1): Newton on P_n from the Chebyshev guess, the usual recurrence; ~1e-16
inline void gauss_unit(int n, double* x, double* w) {
  for (int i = 0; i < (n + 1) / 2; ++i) {
    double z = cos(3.14159265358979323846 * (i + 0.75) / (n + 0.5)), pp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 0; j < n; ++j) {
        const double p3 = p2;
        p2 = p1;
        p1 = ((2.0 * j + 1.0) * z * p2 - j * p3) / (j + 1.0);
      }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      const double dz = p1 / pp;
      z -= dz;
      if (fabs(dz) < 1e-16) break;
    }
    const double wt = 2.0 / ((1.0 - z * z) * pp * pp);
    x[i] = 0.5 * (1.0 - z);
    x[n - 1 - i] = 0.5 * (1.0 + z);
    w[i] = w[n - 1 - i] = 0.5 * wt;
  }
}

// set the dynamic-LDS attribute where needed, launch, check: the one launch sequence (the caller reports the kernel when this returns CRT_OK)
template <class K, class... Args>
inline int launch_kernel(K kern, dim3 grid, int nthr, size_t sh, hipStream_t s, Args... args) {
  if (sh > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh) != hipSuccess)
    return (int)CRT_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, grid, dim3(nthr), sh, s, args...);
  return hipGetLastError() == hipSuccess ? (int)CRT_OK : (int)CRT_ERR_LAUNCH;
}

// The record of sun state v = c * nt + t of column c in lds[0 .. reclen): each header slot and each vector from the canopy record or from
// the sun record, in one pass, and the barrier behind it (call with every thread of the workgroup).
__device__ __forceinline__ void series_assemble(const SeriesArgs& sr, int reclen, int c, long long v, double* lds) {
  const int tid = threadIdx.x, nthr = blockDim.x, nz = sr.nz;
  {
    const double* can = sr.can + (long long)c * sr.canlen;
    const double* sun = sr.sun + v * sr.sunlen;
    if (tid < REC_HDR) {
      int si = -1;
#pragma unroll
      for (int i = 0; i < 5; ++i)
        if (sun_hdr_slot(i) == tid) si = i;
      lds[tid] = si >= 0 ? sun[si] : can[tid];
    }
    const int nvec = (reclen - REC_HDR) / nz;
    for (int vec = 0; vec < nvec; ++vec) {
      const int sv = rec_vec_sun(sr.scheme, vec);
      const double* src = sv >= 0 ? sun + SUN_HDR + sv * nz : can + REC_HDR + vec * nz;
      for (int j = tid; j < nz; j += nthr) lds[REC_HDR + vec * nz + j] = src[j];
    }
  }
  __syncthreads();
}

// One sun state of one column per workgroup.  Assembles the record of (column, t) in lds[0 .. reclen) (series_assemble) and calls
// `body(a_t, ia_t)`, the per-step kernel's body, with argument
// blocks whose spectra and output pointers are shifted so that the body's own indexing by the COLUMN reaches I_dr0 / I_df0 of (column, t)
// and slice [column][t] of every output.  The shifts are workgroup-uniform; there is no loop over sun states, so the body keeps the
// registers it has in the per-step kernel.
template <class Body>
__device__ __forceinline__ void series_step(const SolveArgs& a, const IntArgs& ia, const SeriesArgs& sr, double* lds, Body body) {
  const int c = blockIdx.x, nz = sr.nz, ng = ia.ngroup;
  const long long tl = (long long)blockIdx.z * gridDim.y + blockIdx.y;
  if (tl >= sr.nt) return;  // (whole workgroup, before any barrier)
  const int t = (int)tl;
  const long long v = (long long)c * sr.nt + t;
  series_assemble(sr, a.reclen, c, v, lds);
  SolveArgs at = a;
  IntArgs it = ia;
  const long long din = (long long)c * sr.col_stride + (long long)t * a.nb - (long long)c * a.col_stride;
  at.I_dr0 = static_cast<const double*>(sr.I_dr0) + din;
  at.I_df0 = static_cast<const double*>(sr.I_df0) + din;
  const long long sh = v - c, sa = sh * (nz - 1) * ng, sl = sh * nz * ng;
  it.aI += sa;
  it.aI_sl += sa;
  it.aI_sh += sa;
  if (it.totals) it.totals += sh * ng * 4;
  if (it.L_dr) {
    it.aI_dr += sa;
    it.L_dr += sl;
    it.L_dn += sl;
    it.L_up += sl;
    it.L_F += sl;
    it.L_Id += sl;
  }
  body(at, it);
}

// sr: nullptr = the per-step kernel; else the series kernel of the same form (same LDS layout, same choice of M / sums)
int launch_closed_int(int scheme, const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr = nullptr);
int launch_tridiag_int(int scheme, const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr = nullptr);

// ------------------------------------------------------------------------------------------
// Level-subset outputs (crt_hip_levels_*): rows lev[0..nsel) of I_dr, I_df_d, I_df_u, F, each [ncol][nsel][nb] or NULL.  The levels
// travel by value in the kernel arguments (strictly ascending, validated by the entry point).  A workgroup owns one column and one
// slice of `per` bands (grid: ncol x nslice), one lane per band: nothing is reduced across bands, so any nb works.
struct LevArgs {
  void* o[4];
  int nsel;
  int32_t lev[CRT_MAX_LEVEL_SELECT];
};

struct LevSlices {
  int nslice, per, nthr;  // workgroups per column, bands per workgroup, lanes per workgroup (multiple of 64, >= per)
};
// balanced band slices of at most wmax lanes
inline LevSlices lev_slices(int nb, int wmax) {
  LevSlices ls;
  ls.nslice = (nb + wmax - 1) / wmax;
  ls.per = (nb + ls.nslice - 1) / ls.nslice;
  ls.nthr = ((ls.per + 63) / 64) * 64;
  return ls;
}

// Level-subset outputs over a sun-angle series (crt_hip_levels_series_*): one workgroup per (column, band slice, sun state).  The column is
// blockIdx.x as in the per-step level kernels; t = (blockIdx.z / nslice) * gridDim.y + blockIdx.y and the band slice blockIdx.z % nslice, so
// that any nt fits as long as nslice * ceil(nt / 65535) <= 65535.
inline bool lev_series_grid(int ncol, int nt, int nslice, dim3* grid) {
  const unsigned gy = nt < 65535 ? (unsigned)nt : 65535u;
  const long long gz = (long long)nslice * ((nt + (long long)gy - 1) / gy);
  if (gz > 65535) return false;
  *grid = dim3((unsigned)ncol, gy, (unsigned)gz);
  return true;
}

// Assembles the record of (column, t) in lds[0 .. reclen) and calls `body(a_t, slice, oshift)`, the per-step level kernel's body: a_t has
// its spectra shifted so that the body's indexing by the COLUMN reaches I_dr0 / I_df0 of (column, t) (TIO elements: the series spectra have
// the storage type of the call), and oshift (elements) moves its [column][nsel][nb] output index to slice [column][t].  Both are
// workgroup-uniform.  LevArgs is passed on untouched: its level list stays in the kernel arguments.
template <typename TIO, class Body>
__device__ __forceinline__ void series_lev_step(const SolveArgs& a, const LevArgs& la, const SeriesArgs& sr, int nslice, double* lds, Body body) {
  const int c = blockIdx.x;
  const int zt = blockIdx.z / nslice, slice = blockIdx.z - zt * nslice;
  const long long tl = (long long)zt * gridDim.y + blockIdx.y;
  if (tl >= sr.nt) return;  // (whole workgroup, before any barrier)
  const int t = (int)tl;
  const long long v = (long long)c * sr.nt + t;
  series_assemble(sr, a.reclen, c, v, lds);
  SolveArgs at = a;
  const long long din = (long long)c * sr.col_stride + (long long)t * a.nb - (long long)c * a.col_stride;
  at.I_dr0 = static_cast<const TIO*>(sr.I_dr0) + din;
  at.I_df0 = static_cast<const TIO*>(sr.I_df0) + din;
  if constexpr (std::is_invocable_v<Body, const SolveArgs&, int, long long, long long>)
    body(at, slice, (v - c) * la.nsel * a.nb, v);  // (the sensor forms index their sums by v)
  else
    body(at, slice, (v - c) * la.nsel * a.nb);
}

// ------------------------------------------------------------------------------------------
// Sensor-band outputs (crt_hip_sensor_levels_*, include/crt1d_hip_sensor.h): the level kernels with every selected row folded with a set
// of spectral response functions before anything leaves the workgroup.  The supports travel by value, as the levels do.
struct SensArgs {
  double* o[4];       // I_dr, I_df_d, I_df_u, F: [nv][nsel][nsens] or NULL (nv = ncol, series: ncol * nt)
  const double* w;    // packed weights: those of sensor band s at w[off[s] .. off[s] + count[s])
  double* part;       // partial sums [nv][nslice][nsel][4][nsens] (several band slices only)
  int nsens;
  int nq;             // outputs asked for; qs[k] = index (0..3) of the k-th of them: only those are staged, multiplied and summed
  int32_t qs[4];
  int32_t first[CRT_MAX_SENSOR_BANDS], count[CRT_MAX_SENSOR_BANDS], off[CRT_MAX_SENSOR_BANDS];
};
// The column mask of the masked entries (include_mask/crt1d_hip_masked.h): column c is skipped iff skip[c / unit] != 0.  It travels as
// the LAST argument of the masked kernel instantiations only -- the argument blocks of the plain kernels keep their layout -- and is
// read once per workgroup (per thread in the finish kernels), before anything of the column.  skip == nullptr on the host: no mask, the
// plain kernels are launched.
struct ColMask {
  const int32_t* skip;
  int unit;
};
__device__ __forceinline__ bool col_skipped(const ColMask& m, int c) { return m.skip[c / m.unit] != 0; }

// what a sensor call adds to a level launch; nslice: the band slices the launcher chose (written by a probe too); mask: the masked entries
struct SensLaunch {
  SensArgs sn;
  int nslice;
  ColMask mask;
  bool closed_only;  // the call comes from a masked entry: 2s, bl, g77 and bf only (api.hip refuses the rest before any launch)
};
constexpr int SENS_STAGE = 4;  // LDS doubles per lane of the staging row

// One finished row r of the workgroup's (column or (column, t)) v and band slice `slice` = bands [slice * per, min(slice * per + per, nb)):
// every lane stages its value of each output asked for (0 from a lane that owns no band of the slice), then wave w reduces the sensor bands
// w, w + nwave, ... whose support meets the slice -- lane l adds the products of the bands lo + l, lo + l + 64, ... in ascending order,
// wave_sum4 adds the 64 lane sums of up to four arrays -- and writes the sums (one slice) or the slice's partial sums.  The order depends
// on the slice bounds and the support only; the total of an array does not depend on which other arrays share the wave_sum4.  Call with
// every thread of the workgroup (two barriers).
__device__ __forceinline__ void sens_row(const SensArgs& sn, double* stage, const double (&v)[4], bool live, int slice, int per, int nb,
                                         int nslice, long long vcol, int nsel, int r) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  {
    int k = 0;  // (uniform)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (sn.o[q]) stage[k++ * nthr + tid] = live ? v[q] : 0.0;
  }
  __syncthreads();
  const int lo_s = slice * per, hi_s = min(lo_s + per, nb);
  const int lane = tid & 63, nsens = sn.nsens, nq = sn.nq;
  const int k = wave_sum4_slot(lane >> 4);
  for (int s = tid >> 6; s < nsens; s += nthr >> 6) {  // (wave-uniform)
    const int f = sn.first[s];
    const int lo = max(f, lo_s), hi = min(f + sn.count[s], hi_s);
    if (lo >= hi) continue;
    const double* w = sn.w + (sn.off[s] - f);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = lo + lane; i < hi; i += 64) {
      const double wi = w[i];
      const double* x = stage + (i - lo_s);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nq) acc[j] += wi * x[j * nthr];
    }
    const double z = wave_sum4(acc[0], acc[1], acc[2], acc[3]);
    if ((lane & 15) == 0 && k < nq) {
      const int q = sn.qs[k];
      if (nslice == 1)
        sn.o[q][(vcol * nsel + r) * nsens + s] = z;
      else
        sn.part[(((vcol * nslice + slice) * nsel + r) * 4 + q) * nsens + s] = z;
    }
  }
  __syncthreads();
}

// The fold of sens_row for rows that already lie in LDS (k_sens_jac, sensjac.hip): `rows` = [nsel][R][nthr] doubles, lane <-> band of the
// slice; group g < ng of level r is the NR <= 4 consecutive rows row0 + g NR .. and belongs to parameter par0 + g.  Wave w serves the items
// (r, s, g) w, w + nwave, ...: lane l adds the products w_s[b] * row[b] of the bands lo + l, lo + l + 64, ... in ascending order, wave_sum4
// adds the 64 lane sums of the group's rows -- sens_row's order, whatever the split of the items over the waves.  A group of NR = 3 rows
// holds quantities 1..3 (I_df_d, I_df_u, F); quantity 0 (I_dr) is then the sum of zeros.  The sums go to sn.o[q][((v nsel + r) nsens + s) npar
// + par] (one slice; a NULL output is not written) or to sn.part[((((v nslice + slice) nsel + r) nsens + s) npar + par) 4 + q].  Call with
// every thread of the workgroup, between two barriers of the caller's.
template <int NR>
__device__ __forceinline__ void sens_fold_rows(const SensArgs& sn, const double* rows, int R, int row0, int ng, int par0, int npar, int slice,
                                               int per, int nb, int nslice, long long v, int nsel) {
  static_assert(NR == 3 || NR == 4, "three diffuse quantities or all four");
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, nsens = sn.nsens;
  const int lo_s = slice * per, hi_s = min(lo_s + per, nb);
  const int q = wave_sum4_slot(lane >> 4);
  const int nitem = nsel * nsens * ng;
  for (int it = tid >> 6; it < nitem; it += nthr >> 6) {  // (wave-uniform)
    const int g = it % ng, s = (it / ng) % nsens, r = it / (ng * nsens);
    const int f = sn.first[s];
    const int lo = max(f, lo_s), hi = min(f + sn.count[s], hi_s);
    if (lo >= hi) continue;
    const double* w = sn.w + (sn.off[s] - f);
    const double* x = rows + ((size_t)r * R + row0 + g * NR) * nthr - lo_s;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = lo + lane; i < hi; i += 64) {
      const double wi = w[i];
#pragma unroll
      for (int j = 0; j < NR; ++j) acc[4 - NR + j] += wi * x[(size_t)j * nthr + i];
    }
    const double z = wave_sum4(acc[0], acc[1], acc[2], acc[3]);
    if ((lane & 15) == 0) {
      const int par = par0 + g;
      if (nslice == 1) {
        if (sn.o[q]) sn.o[q][((v * nsel + r) * nsens + s) * npar + par] = z;
      } else {
        sn.part[((((v * nslice + slice) * nsel + r) * nsens + s) * npar + par) * 4 + q] = z;
      }
    }
  }
}

// Widest balanced band slices (lev_slices, at most 1024 lanes, halved down to 64) whose LDS `bytes(nthr)` fits `cap`; nslice = 0: none fits.
template <class F>
inline LevSlices lev_slices_fit(int nb, size_t cap, F bytes) {
  int wmax = 1024;
  while (wmax >= 64 && bytes(wmax) > cap) wmax >>= 1;
  if (wmax < 64) return LevSlices{0, 0, 0};
  return lev_slices(nb, wmax);
}

// What every sensor launcher does around its kernel.  sens_probe: records the slice count for the workspace query and refuses (before
// any launch) a finish grid beyond 2^31 blocks; sens_finish: the finish kernel where several slices ran.
inline int sens_probe(SensLaunch* sl, const LevSlices& ls, long long nv, int nsel) {
  sl->nslice = ls.nslice;
  if (ls.nslice > 1 && nv * nsel * 4 * sl->sn.nsens / 256 >= 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  return CRT_OK;
}
// mask (skip != nullptr): the masked finish kernel; nt: the sun states per column (the mask is indexed by the column v / nt)
int launch_sens_finish(const SensArgs& sn, long long nv, int nslice, int per, int nb, int nsel, hipStream_t s, ColMask mask = {}, int nt = 1);
inline int sens_finish(const SensLaunch* sl, const LevSlices& ls, long long nv, int nb, int nsel, hipStream_t s, int nt = 1) {
  return ls.nslice > 1 ? launch_sens_finish(sl->sn, nv, ls.nslice, ls.per, nb, nsel, s, sl->mask, nt) : (int)CRT_OK;
}

// (launch_sens_finish, sensor.hip: adds the slice partial sums of sens_row in ascending slice order; nv = ncol, series: ncol * nt)

// sr: nullptr = the per-step kernel; else the series kernel of the same form (same slices, same LDS layout, same M).  probe: choose the
// configuration and return its status (CRT_OK / CRT_ERR_UNSUPPORTED) without launching anything.  sl: nullptr = the level spectra; else the
// sensor-band form of the same kernel (la.o unused), followed by the finish kernel where several slices ran.
int launch_closed_lev(int scheme, const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr = nullptr, bool probe = false,
                      SensLaunch* sl = nullptr);
int launch_tridiag_lev(int scheme, const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr = nullptr, bool probe = false,
                       SensLaunch* sl = nullptr);
int launch_zqpa_lev(const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr = nullptr, bool probe = false,
                    SensLaunch* sl = nullptr);
int launch_tri_lev_n79_f64(const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr, bool probe, SensLaunch* sl);
int launch_tri_lev_n79_f32(const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr, bool probe, SensLaunch* sl);
int launch_tri_lev_zq_f64(const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr, bool probe, SensLaunch* sl);
int launch_tri_lev_zq_f32(const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr, bool probe, SensLaunch* sl);

// ------------------------------------------------------------------------------------------
// Optical-property Jacobians of the level spectra (crt_hip_levels_jac_f64, include/crt1d_hip_jac.h; kernels in jac.hip)
struct JacArgs {
  double* o[3];  // d I_df_d, d I_df_u, d F: [ncol][nsel][3][nb] or NULL
};
// n79 / zq (k_jac_tri, k_dlai_tri): the leading doubles of the record the kernel stages (header + the vectors it reads) and the level states it
// keeps (every JAC_TRI_CP-th one, 4 doubles per lane each).  tri_cp_lds_bytes: its LDS bytes with W lanes per workgroup and `copies` of the
// staged record part -- 1: the values (k_jac_tri); 2: values | tangents of the side record (k_dlai_tri) -- and tri_cp_lanes: the widest W out
// of 64, 32, 16 that fits 160 KB (0: none)
constexpr int JAC_TRI_CP = 4;
constexpr int jac_tri_nrec(int scheme, int nz) { return REC_HDR + (scheme == CRT_SCHEME_N79 ? 3 : 1) * nz; }
constexpr size_t tri_cp_lds_bytes(int scheme, int nz, int W, int copies) {
  const size_t nst = scheme == CRT_SCHEME_N79 ? (size_t)nz : (size_t)nz + 1, ncp = (nst + JAC_TRI_CP - 1) / JAC_TRI_CP;
  return (copies * (((size_t)jac_tri_nrec(scheme, nz) + 1) & ~(size_t)1) + ncp * 4 * W) * sizeof(double);
}
constexpr int tri_cp_lanes(int scheme, int nz, int copies) {
  for (int W = 64; W >= 16; W >>= 1)
    if (tri_cp_lds_bytes(scheme, nz, W, copies) <= 160 * 1024) return W;
  return 0;
}
static_assert(tri_cp_lanes(CRT_SCHEME_N79, CRT_JAC_MAX_NZ_N79, 1) == 16 && tri_cp_lanes(CRT_SCHEME_N79, CRT_JAC_MAX_NZ_N79 + 1, 1) == 0 &&
                  tri_cp_lanes(CRT_SCHEME_ZQ, CRT_JAC_MAX_NZ_ZQ, 1) == 16 && tri_cp_lanes(CRT_SCHEME_ZQ, CRT_JAC_MAX_NZ_ZQ + 1, 1) == 0,
              "the depth limits of crt1d_hip_jac.h are those of the LDS layout");
static_assert(tri_cp_lanes(CRT_SCHEME_N79, 304, 1) == 64 && tri_cp_lanes(CRT_SCHEME_N79, 305, 1) == 32 && tri_cp_lanes(CRT_SCHEME_ZQ, 311, 1) == 64 &&
                  tri_cp_lanes(CRT_SCHEME_ZQ, 312, 1) == 32,
              "whole waves up to 304 (n79) / 311 (zq) levels, as crt1d_hip_jac.h says");
static_assert(tri_cp_lanes(CRT_SCHEME_N79, CRT_DLAI_MAX_NZ_N79, 2) == 16 && tri_cp_lanes(CRT_SCHEME_N79, CRT_DLAI_MAX_NZ_N79 + 1, 2) == 0 &&
                  tri_cp_lanes(CRT_SCHEME_ZQ, CRT_DLAI_MAX_NZ_ZQ, 2) == 16 && tri_cp_lanes(CRT_SCHEME_ZQ, CRT_DLAI_MAX_NZ_ZQ + 1, 2) == 0,
              "the depth limits of crt1d_hip_dlai.h are those of the LDS layout");
static_assert(tri_cp_lanes(CRT_SCHEME_N79, 292, 2) == 64 && tri_cp_lanes(CRT_SCHEME_N79, 293, 2) == 32 && tri_cp_lanes(CRT_SCHEME_N79, 536, 2) == 32 &&
                  tri_cp_lanes(CRT_SCHEME_N79, 537, 2) == 16 && tri_cp_lanes(CRT_SCHEME_ZQ, 307, 2) == 64 && tri_cp_lanes(CRT_SCHEME_ZQ, 308, 2) == 32 &&
                  tri_cp_lanes(CRT_SCHEME_ZQ, 599, 2) == 32 && tri_cp_lanes(CRT_SCHEME_ZQ, 600, 2) == 16,
              "the lane-narrowing thresholds crt1d_hip_dlai.h states");
// probe: return the status (CRT_OK / CRT_ERR_UNSUPPORTED) of the configuration without launching anything
int launch_jac(int scheme, const SolveArgs& a, const LevArgs& la, const JacArgs& jo, hipStream_t s, bool probe);

// ------------------------------------------------------------------------------------------
// LAI derivative of the level spectra (crt_hip_levels_dlai_f64, include/crt1d_hip_dlai.h; kernels in dlai.hip)
struct DlaiArgs {
  double* o[4];        // d I_dr, d I_df_d, d I_df_u, d F: [ncol][nsel][nb] or NULL
  const double* side;  // side records [ncol][dlai_side_len]: the s-tangent of the record entries the kernel reads
};
// doubles of a column's side record: bl the tangent of its tau_d vector; n79 / zq the tangent of every entry of the record part the
// tridiagonal kernel stages, in the record's own layout (header included); 2s, g77, bf none (their tangents follow from the record itself)
constexpr int dlai_side_len(int scheme, int nz) {
  return scheme == CRT_SCHEME_BL ? nz : (scheme == CRT_SCHEME_N79 || scheme == CRT_SCHEME_ZQ) ? jac_tri_nrec(scheme, nz) : 0;
}
// the side precompute (after K0, same stream); the derivative kernel (probe: the status of the configuration, nothing launched); tau_d'
int launch_dlai_side(const ColArgs& ca, double* side, hipStream_t s);
int launch_dlai(int scheme, const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe);
int launch_dtau_d(const double* kb_nodes, const double* L, long long n, int method, double* out, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Leaf-angle derivative of the level spectra (crt_hip_levels_dleaf_f64, include/crt1d_hip_dleaf.h; kernels in dleaf.hip, n79 / zq through
// launch_dlai on the side record written here)
struct DleafTan {
  const double* dg_table;   // [ncol][CRT_NQ]
  const double* dg_at_psi;  // [ncol]
  const double* dmla;       // [ncol] or nullptr
};
// doubles of a column's side record: the tangent of the header and of every vector entry the scheme's kernel reads, in the layout of the
// record part that kernel stages (bl: its tau_d vector alone follows the header)
constexpr int dleaf_side_len(int scheme, int nz) {
  return scheme == CRT_SCHEME_BL ? REC_HDR + nz : (scheme == CRT_SCHEME_N79 || scheme == CRT_SCHEME_ZQ) ? jac_tri_nrec(scheme, nz) : REC_HDR;
}
static_assert(dleaf_side_len(CRT_SCHEME_N79, 7) == dlai_side_len(CRT_SCHEME_N79, 7) && dleaf_side_len(CRT_SCHEME_ZQ, 7) == dlai_side_len(CRT_SCHEME_ZQ, 7),
              "k_dlai_tri reads either side record");
// canopy (2s, bl, g77, bf; the sun-angle series of the sensor Jacobian): on canopy records, without the one entry that follows the sun --
// the header tangent K_b' is written as 0 and tn.dg_at_psi is not read
int launch_dleaf_side(const ColArgs& ca, const DleafTan& tn, double* side, hipStream_t s, bool canopy = false);
int launch_dleaf(int scheme, const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe);
// psi / dg_at_psi: [ncol][nt]
int launch_g_dparam(int ncol, const double* psi, const int32_t* g_kind, const double* g_param, double* dg_table, double* dg_at_psi, hipStream_t s,
                    int nt = 1);
int launch_dtau_d_dleaf(const double* kb_nodes, const double* dkb_nodes, const double* L, long long n, int method, double* out, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Gradient of a weighted sum of the level spectra (crt_hip_levels_grad_f64, include/crt1d_hip_grad.h; kernels in grad.hip): 2s, bl, g77, bf
struct GradArgs {
  const double* w[4];       // d loss / d (I_dr, I_df_d, I_df_u, F): [ncol][nsel][nb] or NULL
  double* o[3];             // d loss / d (leaf_r, leaf_t, soil_r): [ncol][nb] or NULL
  double* lai;              // [ncol] or NULL
  double* leaf;             // [ncol] or NULL
  const double* side_lai;   // side records of k_dlai_side [ncol][dlai_side_len]   (read for bl with `lai`)
  const double* side_leaf;  // side records of k_dleaf_side [ncol][dleaf_side_len] (read with `leaf`)
  double* part;             // [ncol][nslice][2]: the slice sums of lai, leaf (several band slices)
};
constexpr int GRAD_BLOCK = 256;  // bands per slice at most
// doubles behind the K0 records: both side records of every column (the dlai ones first), then the slice sums
constexpr int grad_side_len(int scheme, int nz) { return dlai_side_len(scheme, nz) + dleaf_side_len(scheme, nz); }
inline size_t grad_part_bytes(int ncol, int nb) { return (size_t)ncol * (size_t)lev_slices(nb, GRAD_BLOCK).nslice * 2 * sizeof(double); }
int launch_grad(int scheme, const SolveArgs& a, const LevArgs& la, const GradArgs& ga, hipStream_t s, bool probe);

// ------------------------------------------------------------------------------------------
// Jacobian of the sensor-band sums (crt_hip_sensor_jac_f64, include/crt1d_hip_sensjac.h; kernels in sensjac.hip): 2s, bl, g77, bf
struct SensJacArgs {
  SensArgs sn;              // o: [ncol][nsel][nsens][npar] or NULL; part: [ncol][nslice][nsel][nsens][npar][4]; nq / qs unused
  const double* d[3];       // directions in leaf_r, leaf_t, soil_r: [ncol or 1][ntan][nb] or NULL
  long long dstride;        // 0 or ntan * nb
  int ntan, lai, leaf;      // parameter columns: ntan directions, ln LAI (0 / 1), the leaf angle (0 / 1)
  const double* side_lai;   // side records of k_dlai_side  (read for bl with `lai`)
  const double* side_leaf;  // side records of k_dleaf_side (read with `leaf`)
};
constexpr int SENSJAC_BLOCK = 256;          // bands per slice at most
constexpr size_t SENSJAC_STATIC_LDS = 4096;  // allowance for the kernel's static LDS (header, tangents, level entries: 2432 bytes)
// staging rows per level: three per direction (I_df_d, I_df_u, F), or the four of the LAI / leaf-angle pass, which reuse the same area.
// The slices follow from npar alone (every parameter taken for a direction), so that the workspace query needs no more than npar.
constexpr int sensjac_rows(int ndir) { return 3 * ndir > 4 ? 3 * ndir : 4; }
// the widest of 256, 128, 64 lanes whose staging rows fit; nslice = 0: none
inline LevSlices sensjac_slices(int nb, int nsel, int npar) {
  int wmax = SENSJAC_BLOCK;
  while (wmax >= 64 && (size_t)nsel * sensjac_rows(npar) * wmax * sizeof(double) > 160 * 1024 - SENSJAC_STATIC_LDS) wmax >>= 1;
  if (wmax < 64) return LevSlices{0, 0, 0};
  return lev_slices(nb, wmax);
}
// bytes of the slice sums behind the side records (0 with one slice; where no slice width fits, those of 64-lane slices: the call refuses)
// nt: the sun states of a series ([ncol][nt][nslice]...); SIZE_MAX: beyond size_t
inline size_t sensjac_part_bytes(int ncol, int nb, int nsel, int nsens, int npar, int nt = 1) {
  LevSlices ls = sensjac_slices(nb, nsel, npar);
  if (ls.nslice == 0) ls = lev_slices(nb, 64);
  if (ls.nslice <= 1) return 0;
  const size_t per = (size_t)ls.nslice * nsel * nsens * npar * 4 * sizeof(double), nv = (size_t)ncol * (size_t)nt;
  return nv > SIZE_MAX / per ? SIZE_MAX : nv * per;
}
// sr: nullptr = k_sens_jac; else k_sens_jac_series on the same slices (crt1d_hip_sensjac_series.h): a.ws / sr->can hold canopy records,
// sn.o / sn.part are indexed by c * nt + t, side_leaf comes from launch_dleaf_side(.., canopy = true) and dg_at_psi is [ncol][nt]
int launch_sens_jac(int scheme, const SolveArgs& a, const LevArgs& la, const SensJacArgs& ja, hipStream_t s, bool probe,
                    const SeriesArgs* sr = nullptr, const double* dg_at_psi = nullptr, ColMask mask = {});

// launchers implemented in the .hip files
int launch_colpre(const ColArgs& a, hipStream_t s);
// k0: column records still to be formed (2s: by the k_pipe prologue when k_pipe is picked; otherwise k_colpre runs first), or nullptr
int launch_closed(int scheme, const SolveArgs& a, hipStream_t s, int force, const ColArgs* k0);
int launch_tridiag(int scheme, const SolveArgs& a, hipStream_t s, int force);
int init_quadrature(hipStream_t s);
int launch_tau_d(const double* kb_nodes, const double* L, long long n, int method, double* out, hipStream_t s);
int launch_tridiag_tile(int scheme, const SolveArgs& a, hipStream_t s, bool& done);
// per-(scheme, storage type) instantiation units: tri_inst.hip compiled four times
int launch_tri_tile_n79_f64(const SolveArgs& a, hipStream_t s, bool& done);
int launch_tri_tile_n79_f32(const SolveArgs& a, hipStream_t s, bool& done);
int launch_tri_tile_zq_f64(const SolveArgs& a, hipStream_t s, bool& done);
int launch_tri_tile_zq_f32(const SolveArgs& a, hipStream_t s, bool& done);
int launch_tri_int_n79_f64(const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr);
int launch_tri_int_n79_f32(const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr);
int launch_tri_int_zq_f64(const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr);
int launch_tri_int_zq_f32(const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr);
int launch_zqpa(const SolveArgs& a, double* scratch, hipStream_t s);
int launch_zqpa_int(const SolveArgs& a, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr = nullptr);  // integrated outputs, no scratch (tri_zqpa.hip)
int launch_zqpa_wave(const SolveArgs& g, hipStream_t s);  // per-wave fallback of the computational-grid solve
__host__ __device__ inline int zqpa_M(int nz) { return nz < 100 ? nz : 100; }
void host_quad_nodes(double mu_s, double* psi_nodes);

}  // namespace crt
