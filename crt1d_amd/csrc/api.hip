// C-ABI entry points of libcrt1d_hip.so (see include/crt1d_hip.h): argument validation, filling the argument blocks of the launchers
// (the solve files; epilogue.hip for absorption and band sums), and the four bandwidth and math probes, which belong to no other file.
#include <math.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "crt1d_hip_masked.h"
#include "epilogue.hpp"
#include "series/crt1d_hip_specfit_series.h"
#include "specfit.hpp"

namespace crt {
namespace {

// ------------------------------------------------------------------------------------------
// probes.  Device math first; then bandwidth: plain 16-B-per-lane streaming fill / copy, grid-stride
__global__ __launch_bounds__(256) void k_probe_math(const double* x, size_t n, double* e, double* sn, double* cs) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  e[i] = fexp(x[i]);
  double s_, c_;
  fast_sincos(x[i], s_, c_);
  sn[i] = s_;
  cs[i] = c_;
}

__global__ __launch_bounds__(256) void k_fill(d2* dst, size_t n2, double v) {
  d2 t;
  t.x = v;
  t.y = v;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256)
    __builtin_nontemporal_store(t, dst + i);
}

__global__ __launch_bounds__(256) void k_copy(d2* dst, const d2* src, size_t n2) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

// store-pattern probe: what the solve kernels' flush does and nothing else -- workgroup c writes, for column c of EVERY array of the
// set, run after run of `run` doubles (T levels x nb bands) with 16-byte streaming stores, all arrays in step.  Run on a Plan's own
// output set it measures the store rate that placement allows (the linear fill above writes one array, i.e. one memory class, at a time).
struct StoreSetArgs {
  double* p[8];
  int na;
  long long ncol, col;  // columns, doubles per column
  int run;              // doubles per run (a multiple of 2)
};
__global__ __launch_bounds__(192) void k_store_set(StoreSetArgs a, double v) {
  d2 t;
  t.x = v;
  t.y = v;
  const long long c = blockIdx.x;
  const long long base = c * a.col;
  for (long long r0 = 0; r0 < a.col; r0 += a.run) {
    const int n2 = (int)(min((long long)a.run, a.col - r0) >> 1);
    for (int k = 0; k < a.na; ++k) {
      d2* dst = reinterpret_cast<d2*>(a.p[k] + base + r0);
      for (int i = threadIdx.x; i < n2; i += 192) __builtin_nontemporal_store(t, dst + i);
    }
  }
}

bool scheme_ok(int s) { return s >= 0 && s < CRT_NUM_SCHEMES; }

}  // namespace
}  // namespace crt

using namespace crt;

// The optional outputs of a crt_bandsum_out come all together or not at all -- the direct-beam part of the absorption + the five level
// profiles: 6 or 0, or -1 for a part of them (CRT_ERR_BAD_ARG).
static int bandsum_nopt(const crt_bandsum_out& o) {
  const int n = (o.aI_dr != nullptr) + (o.I_dr != nullptr) + (o.I_df_d != nullptr) + (o.I_df_u != nullptr) + (o.F != nullptr) + (o.I_d != nullptr);
  return n == 0 || n == 6 ? n : -1;
}

// the crt_bandsum_out of the entries that take the four mandatory outputs as arguments
static crt_bandsum_out bandsum_out4(double* aI, double* aI_sl, double* aI_sh, double* totals) {
  crt_bandsum_out o = {};
  o.aI = aI;
  o.aI_sl = aI_sl;
  o.aI_sh = aI_sh;
  o.totals = totals;
  return o;
}

template <typename TIO>
static int bandsum_impl(const crt_columns* cols, int32_t nb, int64_t col_stride, const TIO* leaf_r, const TIO* leaf_t, const TIO* I_dr,
                        const TIO* I_df_d, const TIO* I_df_u, const double* band_w, int32_t ngroup, const crt_bandsum_out* out,
                        crt_stream_t stream) {
  if (!cols || !I_dr || !I_df_d || !I_df_u || !band_w || !out || !out->aI || !out->aI_sl || !out->aI_sh) return CRT_ERR_BAD_ARG;
  if (bandsum_nopt(*out) < 0) return CRT_ERR_BAD_ARG;
  if (cols->ncol <= 0 || cols->nz < 2 || nb <= 0 || ngroup <= 0 || ngroup > MAXG) return CRT_ERR_BAD_ARG;
  if (!cols->psi || !cols->lai || !cols->g_kind || !leaf_r || !leaf_t) return CRT_ERR_BAD_ARG;
  EpiArgsT<TIO> a;
  a.ncol = cols->ncol;
  a.nb = nb;
  a.nz = cols->nz;
  a.ngroup = ngroup;
  a.col_stride = col_stride;
  a.psi = cols->psi;
  a.lai = cols->lai;
  a.g_kind = cols->g_kind;
  a.g_param = cols->g_param;
  a.g_at_psi = cols->g_at_psi;
  a.leaf_r = leaf_r;
  a.leaf_t = leaf_t;
  a.I_dr = I_dr;
  a.I_df_d = I_df_d;
  a.I_df_u = I_df_u;
  a.band_w = band_w;
  a.aI = out->aI;
  a.aI_sl = out->aI_sl;
  a.aI_sh = out->aI_sh;
  a.totals = out->totals;
  a.aI_dr = out->aI_dr;
  a.L_dr = out->I_dr;
  a.L_dn = out->I_df_d;
  a.L_up = out->I_df_u;
  a.L_F = out->F;
  a.L_Id = out->I_d;
  return launch_bandsum(a, static_cast<hipStream_t>(stream));
}

template <typename TIO>
static int absorb_impl(const crt_columns* cols, int32_t nb, int64_t col_stride, const TIO* leaf_r, const TIO* leaf_t, const TIO* I_dr,
                       const TIO* I_df_d, const TIO* I_df_u, TIO* const* out7, double* laim, double* f_slm, crt_stream_t stream) {
  if (!cols || !I_dr || !I_df_d || !I_df_u || !out7 || !laim || !f_slm) return CRT_ERR_BAD_ARG;
  if (cols->ncol <= 0 || cols->nz < 2 || nb <= 0) return CRT_ERR_BAD_ARG;
  if (!cols->psi || !cols->lai || !cols->g_kind || !leaf_r || !leaf_t) return CRT_ERR_BAD_ARG;
  AbsArgsT<TIO> a;
  a.ncol = cols->ncol;
  a.nb = nb;
  a.nz = cols->nz;
  a.col_stride = col_stride;
  a.psi = cols->psi;
  a.lai = cols->lai;
  a.g_kind = cols->g_kind;
  a.g_param = cols->g_param;
  a.g_at_psi = cols->g_at_psi;
  a.leaf_r = leaf_r;
  a.leaf_t = leaf_t;
  a.I_dr = I_dr;
  a.I_df_d = I_df_d;
  a.I_df_u = I_df_u;
  for (int i = 0; i < 7; ++i) {
    if (!out7[i]) return CRT_ERR_BAD_ARG;
    a.o[i] = out7[i];
  }
  a.laim = laim;
  a.f_slm = f_slm;
  return launch_absorb(a, static_cast<hipStream_t>(stream));
}

extern "C" {

int crt_hip_abi_version(void) { return CRT_ABI_VERSION; }

const char* crt_hip_strerror(int st) {
  switch (st) {
    case CRT_OK: return "ok";
    case CRT_ERR_BAD_ARG: return "bad argument (null pointer, non-positive size or invalid option)";
    case CRT_ERR_WORKSPACE: return "workspace too small (see crt_hip_workspace_bytes)";
    case CRT_ERR_UNSUPPORTED: return "shape not supported by the gfx950 kernels (nz too large for LDS, or grid overflow)";
    case CRT_ERR_LAUNCH: return "HIP runtime / launch error";
    case CRT_ERR_SHAPE: return "shape violates a reference assertion";
    default: return "unknown status";
  }
}

size_t crt_hip_workspace_bytes(int scheme, int32_t ncol, int32_t nz) {
  if (!scheme_ok(scheme) || ncol <= 0 || nz <= 0) return 0;
  return (size_t)ncol * (size_t)rec_len(scheme, nz) * sizeof(double);
}

size_t crt_hip_workspace_bytes_nb(int scheme, int32_t ncol, int32_t nz, int32_t nb) {
  size_t n = crt_hip_workspace_bytes(scheme, ncol, nz);
  if (n == 0 || nb <= 0) return 0;
  if (scheme == CRT_SCHEME_ZQ_PA) n += 2 * (size_t)ncol * (size_t)zqpa_M(nz) * (size_t)nb * sizeof(double);
  return n;
}

// the records of a series: canopy records [ncol][can_len] -- or `base` bytes where that is more -- then the sun records [ncol * nt][sun_len];
// 0 for a size beyond size_t (arguments checked by the caller)
static size_t series_record_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nt, size_t base) {
  const size_t can = std::max(base, (size_t)ncol * (size_t)can_len(scheme, nz) * sizeof(double));
  const size_t per = (size_t)sun_len(scheme, nz) * sizeof(double);
  const size_t nsun = (size_t)ncol * (size_t)nt;
  return nsun > (SIZE_MAX - can) / per ? 0 : can + nsun * per;
}

size_t crt_hip_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt) {
  // Layout: canopy records [ncol][can_len] from the start, the sun records [ncol * nt][sun_len] right behind them.  The size is at least
  // the per-step workspace (so that one buffer serves both entries): where that is larger than the canopy records (zq_pa's scratch share
  // for its grid fluxes, which no integrated kernel uses), the difference is unused padding at the end.
  const size_t base = crt_hip_workspace_bytes_nb(scheme, ncol, nz, nb);
  return base == 0 || nt < 1 ? 0 : series_record_bytes(scheme, ncol, nz, nt, base);
}

size_t crt_hip_levels_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nt) {
  // the records of crt_hip_series_workspace_bytes at the same offsets, and nothing behind them: no nb
  return !scheme_ok(scheme) || ncol <= 0 || nz <= 0 || nt < 1 ? 0 : series_record_bytes(scheme, ncol, nz, nt, 0);
}

int crt_hip_quad_nodes(double mu_s, double* psi_nodes) {
  if (!psi_nodes || !(mu_s > 0.0 && mu_s < 1.0)) return CRT_ERR_BAD_ARG;
  host_quad_nodes(mu_s, psi_nodes);
  return CRT_OK;
}

// options of one solve call, resolved from crt_options (or the defaults when it is NULL) by check_solve
struct SolveOpts {
  double mu_s = 0.501;
  int method = CRT_TAU_D_QUAD, flags = 0;
  int32_t tune[CRT_NTUNE] = {};
};

static bool is_tri(int scheme) { return scheme == CRT_SCHEME_N79 || scheme == CRT_SCHEME_ZQ; }

// the level-subset and the integrated launcher of the scheme's kernel family: zq_pa, n79 / zq, the closed forms
static int launch_family_lev(int scheme, const SolveArgs& sa, const LevArgs& la, hipStream_t s, const SeriesArgs* sr, bool probe, SensLaunch* sl) {
  if (scheme == CRT_SCHEME_ZQ_PA) return launch_zqpa_lev(sa, la, s, sr, probe, sl);
  return is_tri(scheme) ? launch_tridiag_lev(scheme, sa, la, s, sr, probe, sl) : launch_closed_lev(scheme, sa, la, s, sr, probe, sl);
}
static int launch_family_int(int scheme, const SolveArgs& sa, const IntArgs& ia, hipStream_t s, const SeriesArgs* sr) {
  if (scheme == CRT_SCHEME_ZQ_PA) return launch_zqpa_int(sa, ia, s, sr);
  return is_tri(scheme) ? launch_tridiag_int(scheme, sa, ia, s, sr) : launch_closed_int(scheme, sa, ia, s, sr);
}

// Every argument check of a solve, in the order that decides which status a call with several faults gets; fills `o`.
// integ / lev / ser: the integrated outputs, the level subset, the sun-angle series of the call (each NULL when it has none).
static int check_solve(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const crt_outputs* out,
                       const void* workspace, size_t workspace_bytes, const IntArgs* integ, const LevArgs* lev, const crt_sun_series* ser,
                       SolveOpts& o, size_t extra_ws = 0) {  // extra_ws: what the call keeps behind the records (sensor partial sums)
  if (!scheme_ok(scheme) || !cols || !bands || !out) return CRT_ERR_BAD_ARG;
  const int ncol = cols->ncol, nz = cols->nz, nb = bands->nb;
  if (ncol <= 0 || nz <= 0 || nb <= 0) return CRT_ERR_BAD_ARG;
  if (!cols->lai || !cols->g_kind) return CRT_ERR_BAD_ARG;
  if (scheme == CRT_SCHEME_2S && !cols->mla) return CRT_ERR_BAD_ARG;
  if (!bands->leaf_r || !bands->leaf_t) return CRT_ERR_BAD_ARG;
  if (ser) {  // sun-angle series (integrated outputs or level spectra): the sun and the incoming spectra come from `ser`, not from cols / bands
    if ((!integ && !lev) || !ser->psi || !ser->I_dr0 || !ser->I_df0 || ser->nt < 1) return CRT_ERR_BAD_ARG;
    if (ser->col_stride != 0 && ser->col_stride < (int64_t)ser->nt * nb) return CRT_ERR_BAD_ARG;
    if (cols->g_table && !ser->g_at_psi) return CRT_ERR_BAD_ARG;
  } else if (!cols->psi || !bands->I_dr0 || !bands->I_df0) {
    return CRT_ERR_BAD_ARG;
  }
  if (scheme != CRT_SCHEME_BL && !bands->soil_r) return CRT_ERR_BAD_ARG;
  if (bands->col_stride != 0 && bands->col_stride < nb) return CRT_ERR_BAD_ARG;
  if (!integ && !lev) {
    if (!out->I_dr || !out->I_df_d || !out->I_df_u || !out->F) return CRT_ERR_BAD_ARG;
    const int nextra = scheme == CRT_SCHEME_N79 ? 2 : (scheme == CRT_SCHEME_ZQ || scheme == CRT_SCHEME_G77 || scheme == CRT_SCHEME_BF) ? 3 : 0;
    if (nextra >= 1 && !out->x0) return CRT_ERR_BAD_ARG;
    if (nextra >= 2 && !out->x1) return CRT_ERR_BAD_ARG;
    if (nextra >= 3 && !out->x2) return CRT_ERR_BAD_ARG;
  }
  if (nz < 2) return CRT_ERR_SHAPE;
  if (scheme == CRT_SCHEME_N79 && nz < 3) return CRT_ERR_SHAPE;  // td[1]/tb[1] of _solve_n79.py:85-92
  if (opts) {
    o.mu_s = opts->mu_s;
    o.method = opts->tau_d_method;
    o.flags = opts->flags;
    std::memcpy(o.tune, opts->tune, sizeof o.tune);
  }
  {  // crt_options.tune is a measurement aid, but it is part of the ABI: values out of range are rejected here, before any launch,
     // instead of reaching the kernel configurations.  A key takes 0 (automatic) or lo, lo + step, ... up to hi; a key absent from the
     // table is reserved and stays 0.
    static const struct { int key, lo, hi, step; } accepted[] = {
        {CRT_TUNE_TILE_LDS, 1, 160 * 1024, 1},           {CRT_TUNE_TILE_T, 1, 64, 1},
        {CRT_TUNE_TILE_FLAGS, 1, 255, 1},                {CRT_TUNE_CLOSED_STORE_WAVES, 1, 12, 1},
        {CRT_TUNE_CLOSED_PIPE_T, 1, 32, 1},              {CRT_TUNE_PACK, CRT_PACK_OFF, CRT_PACK_FORCE, 1},
        {CRT_TUNE_PACK_COMPUTE_WAVES, 1, 4, 1},          {CRT_TUNE_TRI_M, 8, 16, 4},
        {CRT_TUNE_TRI_T, 4, 12, 4},                      {CRT_TUNE_TRI_FAMILY, 1, CRT_TRI_FAMILY_ZQPA_PIPE2_RS, 1},
        {CRT_TUNE_TRI_STORE_WAVES, 1, 12, 1},            {CRT_TUNE_MIN_TILE_NB, 1, 1024, 1},
        {CRT_TUNE_FLAT_FLUSH, CRT_FLAT_FLUSH_OFF, CRT_FLAT_FLUSH_WHOLE_LINE, 1}, {CRT_TUNE_K0_SEPARATE, 1, 1, 1}};
    bool known[CRT_NTUNE] = {};
    for (const auto& r : accepted) {
      const int v = o.tune[r.key];
      known[r.key] = true;
      if (v != 0 && (v < r.lo || v > r.hi || (v - r.lo) % r.step != 0)) return CRT_ERR_BAD_ARG;
    }
    for (int i = 0; i < CRT_NTUNE; ++i)
      if (!known[i] && o.tune[i] != 0) return CRT_ERR_BAD_ARG;
  }
  if (scheme == CRT_SCHEME_4S && !(o.mu_s > 0.0 && o.mu_s < 1.0)) return CRT_ERR_BAD_ARG;
  if (o.method != CRT_TAU_D_QUAD && o.method != CRT_TAU_D_9SKY) return CRT_ERR_BAD_ARG;  // ValueError, common.py:78
  const size_t need = !ser ? crt_hip_workspace_bytes_nb(scheme, ncol, nz, nb)
                      : lev ? crt_hip_levels_series_workspace_bytes(scheme, ncol, nz, ser->nt)
                            : crt_hip_series_workspace_bytes(scheme, ncol, nz, nb, ser->nt);
  if (need == 0 || extra_ws > SIZE_MAX - need) return CRT_ERR_UNSUPPORTED;  // (series: a size beyond size_t)
  if (!workspace || workspace_bytes < need + extra_ws) return CRT_ERR_WORKSPACE;
  if (ser && integ && nb > 1024) return CRT_ERR_UNSUPPORTED;  // as the per-step entry, but before K0 has written anything
  if (ser && lev && (long long)ncol * ser->nt > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;  // (column, t) is a 32-bit index in K0
  return CRT_OK;
}

// the K0 and solve argument blocks of a checked call, for the per-step and the series dispatch alike
static void build_args(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_outputs* out, void* workspace, int f32,
                       const SolveOpts& o, ColArgs& ca, SolveArgs& sa) {
  ca = {cols->ncol, cols->nz, scheme, o.method, o.mu_s, cols->psi, cols->lai, cols->mla, cols->g_kind, cols->g_param, cols->g_at_psi,
        cols->g_table, static_cast<double*>(workspace)};
  sa = {};
  sa.ncol = cols->ncol;
  sa.nb = bands->nb;
  sa.nz = cols->nz;
  sa.reclen = rec_len(scheme, cols->nz);
  sa.col_stride = bands->col_stride;
  sa.ws = static_cast<const double*>(workspace);
  sa.I_dr0 = bands->I_dr0;
  sa.I_df0 = bands->I_df0;
  sa.leaf_r = bands->leaf_r;
  sa.leaf_t = bands->leaf_t;
  sa.soil_r = bands->soil_r;
  void* const o7[7] = {out->I_dr, out->I_df_d, out->I_df_u, out->F, out->x0, out->x1, out->x2};
  std::memcpy(sa.o, o7, sizeof sa.o);
  sa.mu_s = o.mu_s;
  sa.f32 = f32;
  std::memcpy(&sa.tune, o.tune, sizeof sa.tune);
}

// the records and the incoming spectra of a sun-angle series, as the series kernels read them: canopy records [ncol][can_len] at sa.ws, then
// sun records [ncol * nt][sun_len] (SeriesArgs, crt_internal.hpp)
static SeriesArgs series_args(int scheme, const SolveArgs& sa, const crt_sun_series* ser) {
  return {ser->nt, scheme, sa.nz, can_len(scheme, sa.nz), sun_len(scheme, sa.nz), sa.ws, sa.ws + (size_t)sa.ncol * can_len(scheme, sa.nz),
          ser->col_stride, ser->I_dr0, ser->I_df0};
}

// sun-angle series: K0 per column and per (column, t), then one series kernel (integrated outputs or level spectra)
static int dispatch_series(int scheme, ColArgs ca, SolveArgs sa, int flags, const IntArgs* integ, const LevArgs* lev, const crt_sun_series* ser,
                           hipStream_t s, SensLaunch* sl) {
  double* const sunrec = ca.ws + (size_t)ca.ncol * can_len(scheme, ca.nz);
  ca.psi = ser->psi;
  ca.g_at_psi = ser->g_at_psi;
  sa.I_dr0 = sa.I_df0 = nullptr;  // the spectra come from `sr`
  const SeriesArgs sr = series_args(scheme, sa, ser);
  if (lev)  // every shape the level series cannot serve is found here, before K0 has written anything
    if (const int st = launch_family_lev(scheme, sa, *lev, s, &sr, true, sl)) return st;
  const int st = (flags & CRT_FLAG_SKIP_PRECOMPUTE) ? init_quadrature(s) : launch_colpre_series(ca, ser->nt, sunrec, s);
  if (st != CRT_OK) return st;
  if (flags & CRT_FLAG_PRECOMPUTE_ONLY) {
    note_kernel("k_colpre<canopy> + k_colsun nt=%d", ser->nt);
    return CRT_OK;
  }
  return lev ? launch_family_lev(scheme, sa, *lev, s, &sr, false, sl) : launch_family_int(scheme, sa, *integ, s, &sr);
}

// The K0 step of a per-step call: k_colpre, unless the caller keeps the records of an earlier call (CRT_FLAG_SKIP_PRECOMPUTE) or the solve
// kernel forms them itself (k0_in_solve: only the quadrature constants are set up).
static int k0_step(const ColArgs& ca, int flags, bool k0_in_solve, hipStream_t s) {
  if (k0_in_solve) return init_quadrature(s);
  return (flags & CRT_FLAG_SKIP_PRECOMPUTE) ? (int)CRT_OK : launch_colpre(ca, s);
}

// one sun state per column: K0, then the profile, integrated or level-subset kernel of the scheme
static int dispatch_step(int scheme, const ColArgs& ca, const SolveArgs& sa, int flags, const IntArgs* integ, const LevArgs* lev, hipStream_t s,
                         SensLaunch* sl) {
  if (sl)  // sensor-band outputs: a shape their staging does not fit is found here, before K0 has written anything
    if (const int st = launch_family_lev(scheme, sa, *lev, s, nullptr, true, sl)) return st;
  // 2s profiles: the closed-form launcher forms the records inside k_pipe when it picks that kernel (one launch per call), and runs
  // k_colpre in front of any other kernel.  SKIP_PRECOMPUTE / PRECOMPUTE_ONLY and CRT_TUNE_K0_SEPARATE keep k_colpre as a kernel of its own.
  const bool k0_in_solve = scheme == CRT_SCHEME_2S && !integ && !lev && !(flags & (CRT_FLAG_SKIP_PRECOMPUTE | CRT_FLAG_PRECOMPUTE_ONLY)) &&
                           sa.tune.k0_separate == 0;
  if (const int st = k0_step(ca, flags, k0_in_solve, s)) return st;
  if (flags & CRT_FLAG_PRECOMPUTE_ONLY) return CRT_OK;
  if (integ) return launch_family_int(scheme, sa, *integ, s, nullptr);
  if (lev) return launch_family_lev(scheme, sa, *lev, s, nullptr, false, sl);
  if (scheme == CRT_SCHEME_ZQ_PA) return launch_zqpa(sa, ca.ws + (size_t)sa.ncol * sa.reclen, s);
  const int force = (flags & CRT_FLAG_DIRECT_STORES) ? 1 : 0;
  return is_tri(scheme) ? launch_tridiag(scheme, sa, s, force) : launch_closed(scheme, sa, s, force, k0_in_solve ? &ca : nullptr);
}

static int solve_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                      const crt_outputs* out, void* workspace, size_t workspace_bytes, crt_stream_t stream, int f32,
                      const IntArgs* integ = nullptr, const LevArgs* lev = nullptr, const crt_sun_series* ser = nullptr,
                      SensLaunch* sl = nullptr, size_t extra_ws = 0) {
  SolveOpts o;
  const int chk = check_solve(scheme, cols, bands, opts, out, workspace, workspace_bytes, integ, lev, ser, o, extra_ws);
  if (sl && sl->closed_only) {  // a masked entry: an argument error is one for every scheme, then the scheme, whatever the workspace
    if (chk == CRT_ERR_BAD_ARG || chk == CRT_ERR_SHAPE) return chk;
    if (scheme != CRT_SCHEME_2S && scheme != CRT_SCHEME_BL && scheme != CRT_SCHEME_G77 && scheme != CRT_SCHEME_BF) return CRT_ERR_UNSUPPORTED;
  }
  if (chk != CRT_OK) return chk;
  ColArgs ca;
  SolveArgs sa;
  build_args(scheme, cols, bands, out, workspace, f32, o, ca, sa);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return ser ? dispatch_series(scheme, ca, sa, o.flags, integ, lev, ser, s, sl) : dispatch_step(scheme, ca, sa, o.flags, integ, lev, s, sl);
}

int crt_hip_solve_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                      const crt_outputs* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  return solve_impl(scheme, cols, bands, opts, out, workspace, workspace_bytes, stream, 0);
}

// the f32 structs have the layout of the f64 ones (pointers + sizes); only the element type behind the pointers differs
int crt_hip_solve_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts,
                      const crt_outputs_f32* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  static_assert(sizeof(crt_bands_f32) == sizeof(crt_bands) && sizeof(crt_outputs_f32) == sizeof(crt_outputs), "layout");
  return solve_impl(scheme, cols, reinterpret_cast<const crt_bands*>(bands), opts, reinterpret_cast<const crt_outputs*>(out), workspace,
                    workspace_bytes, stream, 1);
}

#define CRT_ENTRY(tag, id)                                                                                                                    \
  int crt_hip_##tag##_f64(const crt_columns* c, const crt_bands* b, const crt_options* o, const crt_outputs* out, void* ws, size_t wsb,         \
                          crt_stream_t s) {                                                                                                     \
    return crt_hip_solve_f64(id, c, b, o, out, ws, wsb, s);                                                                                     \
  }                                                                                                                                             \
  int crt_hip_##tag##_f32(const crt_columns* c, const crt_bands_f32* b, const crt_options* o, const crt_outputs_f32* out, void* ws, size_t wsb, \
                          crt_stream_t s) {                                                                                                     \
    return crt_hip_solve_f32(id, c, b, o, out, ws, wsb, s);                                                                                     \
  }
CRT_ENTRY(2s, CRT_SCHEME_2S)
CRT_ENTRY(4s, CRT_SCHEME_4S)
CRT_ENTRY(n79, CRT_SCHEME_N79)
CRT_ENTRY(zq, CRT_SCHEME_ZQ)
CRT_ENTRY(bl, CRT_SCHEME_BL)
CRT_ENTRY(g77, CRT_SCHEME_G77)
CRT_ENTRY(bf, CRT_SCHEME_BF)
CRT_ENTRY(zq_pa, CRT_SCHEME_ZQ_PA)
#undef CRT_ENTRY

int crt_hip_absorb_bandsum2_f64(const crt_columns* cols, const crt_bands* bands, const double* I_dr, const double* I_df_d,
                                const double* I_df_u, const double* band_w, int32_t ngroup, const crt_bandsum_out* out, crt_stream_t stream) {
  if (!bands) return CRT_ERR_BAD_ARG;
  return bandsum_impl<double>(cols, bands->nb, bands->col_stride, bands->leaf_r, bands->leaf_t, I_dr, I_df_d, I_df_u, band_w, ngroup, out,
                              stream);
}

int crt_hip_absorb_bandsum2_f32(const crt_columns* cols, const crt_bands_f32* bands, const float* I_dr, const float* I_df_d,
                                const float* I_df_u, const double* band_w, int32_t ngroup, const crt_bandsum_out* out, crt_stream_t stream) {
  if (!bands) return CRT_ERR_BAD_ARG;
  return bandsum_impl<float>(cols, bands->nb, bands->col_stride, bands->leaf_r, bands->leaf_t, I_dr, I_df_d, I_df_u, band_w, ngroup, out,
                             stream);
}

int crt_hip_absorb_bandsum_f64(const crt_columns* cols, const crt_bands* bands, const double* I_dr, const double* I_df_d,
                               const double* I_df_u, const double* band_w, int32_t ngroup, double* aI, double* aI_sl,
                               double* aI_sh, double* totals, crt_stream_t stream) {
  const crt_bandsum_out o = bandsum_out4(aI, aI_sl, aI_sh, totals);
  return crt_hip_absorb_bandsum2_f64(cols, bands, I_dr, I_df_d, I_df_u, band_w, ngroup, &o, stream);
}

int crt_hip_absorb_bandsum_f32(const crt_columns* cols, const crt_bands_f32* bands, const float* I_dr, const float* I_df_d,
                               const float* I_df_u, const double* band_w, int32_t ngroup, double* aI, double* aI_sl,
                               double* aI_sh, double* totals, crt_stream_t stream) {
  const crt_bandsum_out o = bandsum_out4(aI, aI_sl, aI_sh, totals);
  return crt_hip_absorb_bandsum2_f32(cols, bands, I_dr, I_df_d, I_df_u, band_w, ngroup, &o, stream);
}

// f32: crt_bands_f32 has the layout of crt_bands (crt_hip_solve_f32); the fused kernels read the spectra as TIO = float
static int integrated_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const double* band_w,
                           int32_t ngroup, const crt_bandsum_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream, int f32,
                           const crt_sun_series* ser = nullptr) {
  if (!band_w || !out || !out->aI || !out->aI_sl || !out->aI_sh || ngroup <= 0 || ngroup > INT_MAXG || !cols) return CRT_ERR_BAD_ARG;
  if (bandsum_nopt(*out) < 0) return CRT_ERR_BAD_ARG;
  IntArgs ia;
  ia.lai = cols->lai;
  ia.band_w = band_w;
  ia.ngroup = ngroup;
  ia.aI = out->aI;
  ia.aI_sl = out->aI_sl;
  ia.aI_sh = out->aI_sh;
  ia.totals = out->totals;
  ia.aI_dr = out->aI_dr;
  ia.L_dr = out->I_dr;
  ia.L_dn = out->I_df_d;
  ia.L_up = out->I_df_u;
  ia.L_F = out->F;
  ia.L_Id = out->I_d;
  crt_outputs none = {};
  return solve_impl(scheme, cols, bands, opts, &none, workspace, workspace_bytes, stream, f32, &ia, nullptr, ser);
}

int crt_hip_integrated_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                  const crt_options* opts, const double* band_w, int32_t ngroup, const crt_bandsum_out* out, void* workspace,
                                  size_t workspace_bytes, crt_stream_t stream) {
  if (!sun) return CRT_ERR_BAD_ARG;
  return integrated_impl(scheme, cols, bands, opts, band_w, ngroup, out, workspace, workspace_bytes, stream, 0, sun);
}

int crt_hip_integrated2_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                            const double* band_w, int32_t ngroup, const crt_bandsum_out* out, void* workspace, size_t workspace_bytes,
                            crt_stream_t stream) {
  return integrated_impl(scheme, cols, bands, opts, band_w, ngroup, out, workspace, workspace_bytes, stream, 0);
}

int crt_hip_integrated2_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts,
                            const double* band_w, int32_t ngroup, const crt_bandsum_out* out, void* workspace, size_t workspace_bytes,
                            crt_stream_t stream) {
  return integrated_impl(scheme, cols, reinterpret_cast<const crt_bands*>(bands), opts, band_w, ngroup, out, workspace, workspace_bytes,
                         stream, 1);
}

int crt_hip_integrated_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                           const double* band_w, int32_t ngroup, double* aI, double* aI_sl, double* aI_sh, double* totals,
                           void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  const crt_bandsum_out o = bandsum_out4(aI, aI_sl, aI_sh, totals);
  return crt_hip_integrated2_f64(scheme, cols, bands, opts, band_w, ngroup, &o, workspace, workspace_bytes, stream);
}

int crt_hip_integrated_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts,
                           const double* band_w, int32_t ngroup, double* aI, double* aI_sl, double* aI_sh, double* totals,
                           void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  const crt_bandsum_out o = bandsum_out4(aI, aI_sl, aI_sh, totals);
  return crt_hip_integrated2_f32(scheme, cols, bands, opts, band_w, ngroup, &o, workspace, workspace_bytes, stream);
}

// the level list of a call into la.nsel / la.lev: 1 .. CRT_MAX_LEVEL_SELECT levels of the column, strictly ascending (no duplicates)
static int parse_levels(const crt_columns* cols, const int32_t* levels, int32_t nsel, LevArgs& la) {
  if (nsel < 1 || nsel > CRT_MAX_LEVEL_SELECT) return CRT_ERR_BAD_ARG;
  la.nsel = nsel;
  for (int r = 0; r < nsel; ++r) {
    if (levels[r] < 0 || levels[r] >= cols->nz || (r > 0 && levels[r] <= levels[r - 1])) return CRT_ERR_BAD_ARG;
    la.lev[r] = levels[r];
  }
  return CRT_OK;
}

// f32: crt_bands_f32 / crt_outputs_f32 have the layouts of crt_bands / crt_outputs (crt_hip_solve_f32).  Every argument error is found here
// or in solve_impl's checks, before any launch.
static int levels_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                       int32_t nsel, const crt_outputs* out, void* workspace, size_t workspace_bytes, crt_stream_t stream, int f32,
                       const crt_sun_series* ser = nullptr, SensLaunch* sl = nullptr, size_t extra_ws = 0) {
  if (!scheme_ok(scheme) || !cols || !levels || !out) return CRT_ERR_BAD_ARG;
  if (out->x0 || out->x1 || out->x2) return CRT_ERR_BAD_ARG;
  if (!sl && !out->I_dr && !out->I_df_d && !out->I_df_u && !out->F) return CRT_ERR_BAD_ARG;  // (a sensor call has its outputs in sl)
  LevArgs la = {};
  la.o[0] = out->I_dr;
  la.o[1] = out->I_df_d;
  la.o[2] = out->I_df_u;
  la.o[3] = out->F;
  if (const int st = parse_levels(cols, levels, nsel, la)) return st;
  crt_outputs none = {};
  return solve_impl(scheme, cols, bands, opts, &none, workspace, workspace_bytes, stream, f32, nullptr, &la, ser, sl, extra_ws);
}

// crt_sun_series_f32 has the layout of crt_sun_series (the element type behind I_dr0 / I_df0 differs: SeriesArgs carries them untyped)
int crt_hip_levels_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun, const crt_options* opts,
                              const int32_t* levels, int32_t nsel, const crt_outputs* out, void* workspace, size_t workspace_bytes,
                              crt_stream_t stream) {
  if (!sun) return CRT_ERR_BAD_ARG;
  return levels_impl(scheme, cols, bands, opts, levels, nsel, out, workspace, workspace_bytes, stream, 0, sun);
}

int crt_hip_levels_series_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_sun_series_f32* sun,
                              const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_outputs_f32* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream) {
  static_assert(sizeof(crt_sun_series_f32) == sizeof(crt_sun_series) && offsetof(crt_sun_series_f32, I_dr0) == offsetof(crt_sun_series, I_dr0) &&
                    offsetof(crt_sun_series_f32, I_df0) == offsetof(crt_sun_series, I_df0) &&
                    offsetof(crt_sun_series_f32, col_stride) == offsetof(crt_sun_series, col_stride),
                "layout");
  if (!sun) return CRT_ERR_BAD_ARG;
  return levels_impl(scheme, cols, reinterpret_cast<const crt_bands*>(bands), opts, levels, nsel, reinterpret_cast<const crt_outputs*>(out),
                     workspace, workspace_bytes, stream, 1, reinterpret_cast<const crt_sun_series*>(sun));
}

int crt_hip_levels_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                       int32_t nsel, const crt_outputs* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  return levels_impl(scheme, cols, bands, opts, levels, nsel, out, workspace, workspace_bytes, stream, 0);
}

int crt_hip_levels_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts, const int32_t* levels,
                       int32_t nsel, const crt_outputs_f32* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  return levels_impl(scheme, cols, reinterpret_cast<const crt_bands*>(bands), opts, levels, nsel, reinterpret_cast<const crt_outputs*>(out),
                     workspace, workspace_bytes, stream, 1);
}

// ------------------------------------------------------------------------------------------
// Sensor-band outputs (include/crt1d_hip_sensor.h): crt_hip_levels_* with the sensor form of the level kernel.

// bytes of the partial sums [ncol * nt][nslice][nsel][4][nsens] behind the records: 0 with one band slice, and 0 where the shape is not
// served (the call then reports it) or the size is beyond size_t
static size_t sens_partial_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt, int32_t nsel, int32_t nsens) {
  if (!scheme_ok(scheme) || ncol <= 0 || nz <= 0 || nb <= 0 || nt < 1 || nsel < 1 || nsel > CRT_MAX_LEVEL_SELECT || nsens < 1 ||
      nsens > CRT_MAX_SENSOR_BANDS)
    return 0;
  SolveArgs sa = {};
  sa.ncol = ncol;
  sa.nb = nb;
  sa.nz = nz;
  sa.reclen = rec_len(scheme, nz);
  LevArgs la = {};
  la.nsel = nsel;
  SensLaunch sl = {};
  if (launch_family_lev(scheme, sa, la, nullptr, nullptr, true, &sl) != CRT_OK || sl.nslice <= 1) return 0;
  const size_t per = (size_t)sl.nslice * (size_t)nsel * 4 * (size_t)nsens * sizeof(double);
  const size_t nv = (size_t)ncol * (size_t)nt;
  return nv > SIZE_MAX / per ? 0 : nv * per;
}

size_t crt_hip_sensor_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel, int32_t nsens) {
  const size_t rec = crt_hip_workspace_bytes_nb(scheme, ncol, nz, nb);
  return rec == 0 ? 0 : rec + sens_partial_bytes(scheme, ncol, nz, nb, 1, nsel, nsens);
}

size_t crt_hip_sensor_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt, int32_t nsel, int32_t nsens) {
  const size_t rec = crt_hip_levels_series_workspace_bytes(scheme, ncol, nz, nt);
  return rec == 0 || nb <= 0 ? 0 : rec + sens_partial_bytes(scheme, ncol, nz, nb, nt, nsel, nsens);
}

// The column mask of a masked entry (include_mask/crt1d_hip_masked.h).  NULL or a NULL skip: no mask, the plain launches.  ok: false for
// unit < 1 or ncol % unit != 0 (a NULL cols is the sibling's error).
struct MaskArg {
  ColMask m;
  bool ok;
};
static MaskArg parse_mask(const crt_col_mask* mask, const crt_columns* cols) {
  if (!mask || !mask->skip) return {{}, true};
  if (mask->unit < 1 || (cols && cols->ncol > 0 && cols->ncol % mask->unit != 0)) return {{}, false};
  return {{mask->skip, mask->unit}, true};
}
// masked: the call comes from a masked entry, which serves 2s, bl, g77 and bf only (mask: its mask, or NULL)
static int sensor_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels, int32_t nsel,
                       const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                       int f32, const crt_sun_series* ser = nullptr, bool masked = false, const crt_col_mask* mask = nullptr) {
  if (!scheme_ok(scheme) || !cols || !bands || !sensors || !out) return CRT_ERR_BAD_ARG;
  const MaskArg ma = parse_mask(mask, cols);
  if (!ma.ok) return CRT_ERR_BAD_ARG;
  if (!sensors->first || !sensors->count || !sensors->w) return CRT_ERR_BAD_ARG;
  const int nsens = sensors->nsens, nb = bands->nb;
  if (nsens < 1 || nsens > CRT_MAX_SENSOR_BANDS || nb <= 0) return CRT_ERR_BAD_ARG;
  if (!out->I_dr && !out->I_df_d && !out->I_df_u && !out->F) return CRT_ERR_BAD_ARG;
  SensLaunch sl = {};
  sl.mask = ma.m;
  sl.closed_only = masked;
  SensArgs& sn = sl.sn;
  sn.o[0] = out->I_dr;
  sn.o[1] = out->I_df_d;
  sn.o[2] = out->I_df_u;
  sn.o[3] = out->F;
  sn.w = sensors->w;
  sn.nsens = nsens;
  for (int q = 0; q < 4; ++q)
    if (sn.o[q]) sn.qs[sn.nq++] = q;
  int64_t off = 0;
  for (int k = 0; k < nsens; ++k) {
    const int32_t f = sensors->first[k], n = sensors->count[k];
    if (n < 1 || f < 0 || (int64_t)f + n > nb) return CRT_ERR_BAD_ARG;
    sn.first[k] = f;
    sn.count[k] = n;
    sn.off[k] = (int32_t)off;
    off += n;  // (<= 64 nb: no overflow)
  }
  if (off > 0x7fffffffLL) return CRT_ERR_BAD_ARG;
  const int nt = ser ? ser->nt : 1;
  size_t rec = 0, extra = 0;
  if (cols->ncol > 0 && cols->nz > 0 && nt >= 1) {
    rec = ser ? crt_hip_levels_series_workspace_bytes(scheme, cols->ncol, cols->nz, nt) : crt_hip_workspace_bytes_nb(scheme, cols->ncol, cols->nz, nb);
    if (nsel >= 1 && nsel <= CRT_MAX_LEVEL_SELECT) extra = sens_partial_bytes(scheme, cols->ncol, cols->nz, nb, nt, nsel, nsens);
  }
  sn.part = workspace ? reinterpret_cast<double*>(static_cast<char*>(workspace) + rec) : nullptr;
  const crt_outputs lev_out = {};  // no level spectra: LevArgs.o stays NULL, the sums go where `sl` says
  return levels_impl(scheme, cols, bands, opts, levels, nsel, &lev_out, workspace, workspace_bytes, stream, f32, ser, &sl, extra);
}

int crt_hip_sensor_levels_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                              int32_t nsel, const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream) {
  return sensor_impl(scheme, cols, bands, opts, levels, nsel, sensors, out, workspace, workspace_bytes, stream, 0);
}

int crt_hip_sensor_levels_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts, const int32_t* levels,
                              int32_t nsel, const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream) {
  return sensor_impl(scheme, cols, reinterpret_cast<const crt_bands*>(bands), opts, levels, nsel, sensors, out, workspace, workspace_bytes,
                     stream, 1);
}

int crt_hip_sensor_levels_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                     const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                     const crt_sensor_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  if (!sun) return CRT_ERR_BAD_ARG;
  return sensor_impl(scheme, cols, bands, opts, levels, nsel, sensors, out, workspace, workspace_bytes, stream, 0, sun);
}

// ------------------------------------------------------------------------------------------
// Derivatives of the level spectra: the optics Jacobian (include/crt1d_hip_jac.h), the LAI derivative (crt1d_hip_dlai.h), the leaf-angle
// derivative (crt1d_hip_dleaf.h).  One host path, levels_deriv_impl: the checks of crt_hip_levels_f64, K0, the entry's side precompute into
// the side records [ncol][side_len(scheme, nz)] behind the K0 records, one derivative kernel.  An entry says what differs.

using SideLen = int (*)(int scheme, int nz);  // doubles of a column's side record; nullptr: the entry keeps none (jac)

static size_t side_bytes(SideLen len, int scheme, int32_t ncol, int32_t nz) {
  return len ? (size_t)ncol * (size_t)len(scheme, nz) * sizeof(double) : 0;
}

// the K0 records at the offsets of crt_hip_workspace_bytes_nb, then the side records
static size_t levels_deriv_workspace_bytes(SideLen len, int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel) {
  if (nsel < 1 || nsel > CRT_MAX_LEVEL_SELECT) return 0;
  const size_t rec = crt_hip_workspace_bytes_nb(scheme, ncol, nz, nb);
  return rec == 0 ? 0 : rec + side_bytes(len, scheme, ncol, nz);
}

}  // extern "C": closed around the one template (C++ linkage)

// args_ok: the entry's own pointers are there (an output at least).  pre_report: what a CRT_FLAG_PRECOMPUTE_ONLY call reports where the
// scheme has a side record ("k_colpre" where it has none; an entry without side_len leaves K0's report).
// launch(sa, la, side, s, probe): the entry's derivative kernel;  side_pre(ca, side, s): its side precompute, after K0 on the same stream
// (the gradient runs two, into two side records one behind the other).  closed_only: n79 and zq are not served either;  tail_bytes: what the
// entry keeps behind the side records (the gradient's slice sums).
// ser (crt1d_hip_sensjac_series.h): the records are those of a level series -- canopy records at `workspace`, then the sun records, the side
// records behind both -- K0 is launch_colpre_series, and pre_report is reported as it stands; tail_bytes SIZE_MAX: a size beyond size_t.
template <class Launch, class SidePre>
static int levels_deriv_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                             int32_t nsel, void* workspace, size_t workspace_bytes, crt_stream_t stream, bool args_ok, SideLen side_len,
                             const char* pre_report, Launch launch, SidePre side_pre, bool closed_only = false, size_t tail_bytes = 0,
                             const crt_sun_series* ser = nullptr) {
  if (!scheme_ok(scheme) || !cols || !levels || !args_ok) return CRT_ERR_BAD_ARG;
  LevArgs la = {};
  if (const int st = parse_levels(cols, levels, nsel, la)) return st;
  SolveOpts o;
  const crt_outputs none = {};
  const bool sized = cols->ncol > 0 && cols->nz > 0;
  const size_t sides = sized ? side_bytes(side_len, scheme, cols->ncol, cols->nz) : 0;
  const int chk = check_solve(scheme, cols, bands, opts, &none, workspace, workspace_bytes, nullptr, &la, ser, o,
                              !sized ? 0 : tail_bytes > SIZE_MAX - sides ? SIZE_MAX : sides + tail_bytes);
  if (chk == CRT_ERR_BAD_ARG || chk == CRT_ERR_SHAPE) return chk;  // an argument error is one for every scheme
  if (scheme == CRT_SCHEME_4S || scheme == CRT_SCHEME_ZQ_PA) return CRT_ERR_UNSUPPORTED;  // whatever the workspace (a follow-up: crt1d_hip_jac.h)
  if (closed_only && is_tri(scheme)) return CRT_ERR_UNSUPPORTED;                          // (the gradient: crt1d_hip_grad.h)
  if (chk != CRT_OK) return chk;
  ColArgs ca;
  SolveArgs sa;
  build_args(scheme, cols, bands, &none, workspace, 0, o, ca, sa);
  const size_t rec = ser ? crt_hip_levels_series_workspace_bytes(scheme, cols->ncol, cols->nz, ser->nt)
                         : crt_hip_workspace_bytes_nb(scheme, cols->ncol, cols->nz, bands->nb);
  double* const side = reinterpret_cast<double*>(static_cast<char*>(workspace) + rec);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int st = launch(sa, la, side, s, true)) return st;  // a shape that is not served: before K0 has written anything
  if (ser) {
    ca.psi = ser->psi;
    ca.g_at_psi = ser->g_at_psi;
    double* const sunrec = ca.ws + (size_t)ca.ncol * can_len(scheme, ca.nz);
    if (const int st = (o.flags & CRT_FLAG_SKIP_PRECOMPUTE) ? init_quadrature(s) : launch_colpre_series(ca, ser->nt, sunrec, s)) return st;
  } else if (const int st = k0_step(ca, o.flags, false, s)) {
    return st;
  }
  if (!(o.flags & CRT_FLAG_SKIP_PRECOMPUTE))
    if (const int st = side_pre(ca, side, s)) return st;
  if (o.flags & CRT_FLAG_PRECOMPUTE_ONLY) {
    if (side_len) note_kernel("%s", ser || side_len(scheme, cols->nz) ? pre_report : "k_colpre");
    return CRT_OK;
  }
  return launch(sa, la, side, s, false);
}

// a leaf-angle tangent of either C struct (crt_leaf_tangent, crt_leaf_tangent_series: the same three names); NULL: an empty one
template <class Tangent>
static DleafTan dleaf_tan(const Tangent* t) {
  return t ? DleafTan{t->dg_table, t->dg_at_psi, t->dmla} : DleafTan{};
}

// The parameter axis of the entries that take a parameter vector (crt1d_hip_sensjac.h): ntan directions of the optics, then ln LAI, then the
// leaf angle.  ok: the directions are usable, the tangent is NULL or whole, and there is a parameter at all.
struct ParamAxis {
  int ntan, lai, leaf;
  const double* d[3];
  int64_t dstride;
  bool ok;
  int npar() const { return ntan + lai + leaf; }
  template <class KernelArgs>  // SensJacArgs, SpecArgs: the same five names
  void put(KernelArgs& a) const {
    a.ntan = ntan, a.lai = lai, a.leaf = leaf, a.dstride = dstride;
    std::memcpy(a.d, d, sizeof d);
  }
};

static ParamAxis parse_axis(const crt_bands* bands, const crt_optics_dirs* dirs, int with_lai, const DleafTan* tangent) {
  ParamAxis p = {dirs ? dirs->ntan : 0, with_lai ? 1 : 0, tangent ? 1 : 0, {}, 0, false};
  p.ok = bands && bands->nb > 0 && p.ntan >= 0 && p.ntan <= CRT_SENSJAC_MAX_NTAN && (p.ntan == 0 || dirs->leaf_r || dirs->leaf_t || dirs->soil_r) &&
         (p.ntan == 0 || dirs->col_stride == 0 || dirs->col_stride == (int64_t)p.ntan * bands->nb) &&
         (!tangent || (tangent->dg_table && tangent->dg_at_psi)) && p.npar() >= 1;
  if (p.ok && p.ntan > 0) {
    const double* const d[3] = {dirs->leaf_r, dirs->leaf_t, dirs->soil_r};
    std::memcpy(p.d, d, sizeof d);
    p.dstride = dirs->col_stride;
  }
  return p;
}

// The side records of the gradient, the sensor Jacobian and the spectral entries, behind the K0 records: the LAI ones [ncol][dlai_side_len]
// (filled where ln LAI is a parameter and the scheme keeps one), the leaf-angle ones [ncol][dleaf_side_len] (filled where the leaf angle is one),
// then the entry's slice sums.  Called as the side precompute of levels_deriv_impl; `report` is what a CRT_FLAG_PRECOMPUTE_ONLY call reports.
struct SideRecords {
  int scheme;
  bool sized, lai, leaf, series;  // sized: the sizes are positive (they are an argument error of the shared path otherwise: no tail then)
  DleafTan tan;
  char report[112];

  SideRecords(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* ser, bool args_ok, bool want_lai, bool want_leaf,
              const DleafTan& tan)
      : scheme(scheme), series(ser != nullptr), tan(tan) {
    sized = args_ok && cols && bands && cols->ncol > 0 && cols->nz > 0 && bands->nb > 0 && (!ser || ser->nt >= 1);
    lai = sized && want_lai && dlai_side_len(scheme, cols->nz) > 0;
    leaf = args_ok && want_leaf;
    char k0[48] = "k_colpre";
    if (ser) std::snprintf(k0, sizeof k0, "k_colpre<canopy> + k_colsun nt=%d", ser->nt);
    std::snprintf(report, sizeof report, "%s%s%s", k0, lai ? " + k_dlai_side" : "", !leaf ? "" : ser ? " + k_dleaf_side<canopy>" : " + k_dleaf_side");
  }
  const double* side_leaf(const double* side, const SolveArgs& sa) const { return side + (size_t)sa.ncol * dlai_side_len(scheme, sa.nz); }
  double* part(const double* side, const SolveArgs& sa) const { return const_cast<double*>(side) + (size_t)sa.ncol * grad_side_len(scheme, sa.nz); }
  int operator()(const ColArgs& ca, double* side, hipStream_t s) const {
    if (lai)
      if (const int st = launch_dlai_side(ca, side, s)) return st;
    return leaf ? launch_dleaf_side(ca, tan, side + (size_t)ca.ncol * dlai_side_len(scheme, ca.nz), s, series) : (int)CRT_OK;
  }
};

extern "C" {

size_t crt_hip_levels_jac_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel) {
  return levels_deriv_workspace_bytes(nullptr, scheme, ncol, nz, nb, nsel);  // the records; the kernels keep nothing behind them
}

int crt_hip_levels_jac_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                           int32_t nsel, const crt_jac_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  return levels_deriv_impl(
      scheme, cols, bands, opts, levels, nsel, workspace, workspace_bytes, stream, out && (out->I_df_d || out->I_df_u || out->F), nullptr, nullptr,
      [&](const SolveArgs& sa, const LevArgs& la, const double*, hipStream_t s, bool probe) {
        return launch_jac(scheme, sa, la, JacArgs{{out->I_df_d, out->I_df_u, out->F}}, s, probe);
      },
      [](const ColArgs&, double*, hipStream_t) { return (int)CRT_OK; });
}

// the LAI and the leaf-angle derivative share crt_dlai_out and DlaiArgs
static bool dlai_out_ok(const crt_dlai_out* out) { return out && (out->I_dr || out->I_df_d || out->I_df_u || out->F); }
static DlaiArgs dlai_args(const crt_dlai_out* out, const double* side) { return {{out->I_dr, out->I_df_d, out->I_df_u, out->F}, side}; }

size_t crt_hip_levels_dlai_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel) {
  return levels_deriv_workspace_bytes(dlai_side_len, scheme, ncol, nz, nb, nsel);
}

int crt_hip_levels_dlai_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                            int32_t nsel, const crt_dlai_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  return levels_deriv_impl(
      scheme, cols, bands, opts, levels, nsel, workspace, workspace_bytes, stream, dlai_out_ok(out), dlai_side_len, "k_colpre + k_dlai_side",
      [&](const SolveArgs& sa, const LevArgs& la, const double* side, hipStream_t s, bool probe) {
        return launch_dlai(scheme, sa, la, dlai_args(out, side), s, probe);
      },
      [](const ColArgs& ca, double* side, hipStream_t s) { return launch_dlai_side(ca, side, s); });
}

int crt_hip_dtau_d_f64(const double* kb_nodes, const double* L, int64_t n, int32_t method, double* out, crt_stream_t stream) {
  if (!kb_nodes || !L || !out || n < 0) return CRT_ERR_BAD_ARG;
  if (method != CRT_TAU_D_QUAD && method != CRT_TAU_D_9SKY) return CRT_ERR_BAD_ARG;
  if (n == 0) return CRT_OK;
  return crt::launch_dtau_d(kb_nodes, L, (long long)n, method, out, static_cast<hipStream_t>(stream));
}

size_t crt_hip_levels_dleaf_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel) {
  return levels_deriv_workspace_bytes(dleaf_side_len, scheme, ncol, nz, nb, nsel);
}

// (n79 / zq: k_dlai_tri of dlai.hip on the side record written here)
int crt_hip_levels_dleaf_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                             int32_t nsel, const crt_leaf_tangent* tangent, const crt_dlai_out* out, void* workspace,
                             size_t workspace_bytes, crt_stream_t stream) {
  return levels_deriv_impl(
      scheme, cols, bands, opts, levels, nsel, workspace, workspace_bytes, stream,
      tangent && tangent->dg_table && tangent->dg_at_psi && dlai_out_ok(out), dleaf_side_len, "k_colpre + k_dleaf_side",
      [&](const SolveArgs& sa, const LevArgs& la, const double* side, hipStream_t s, bool probe) {
        return launch_dleaf(scheme, sa, la, dlai_args(out, side), s, probe);
      },
      [&](const ColArgs& ca, double* side, hipStream_t s) {
        return launch_dleaf_side(ca, dleaf_tan(tangent), side, s);
      });
}

int crt_hip_g_dparam_f64(const crt_columns* cols, double* dg_table, double* dg_at_psi, crt_stream_t stream) {
  if (!cols || !dg_table || !dg_at_psi || !cols->psi || !cols->g_kind || cols->ncol <= 0) return CRT_ERR_BAD_ARG;
  return crt::launch_g_dparam(cols->ncol, cols->psi, cols->g_kind, cols->g_param, dg_table, dg_at_psi, static_cast<hipStream_t>(stream));
}

int crt_hip_dtau_d_dleaf_f64(const double* kb_nodes, const double* dkb_nodes, const double* L, int64_t n, int32_t method, double* out,
                             crt_stream_t stream) {
  if (!kb_nodes || !dkb_nodes || !L || !out || n < 0) return CRT_ERR_BAD_ARG;
  if (method != CRT_TAU_D_QUAD && method != CRT_TAU_D_9SKY) return CRT_ERR_BAD_ARG;
  if (n == 0) return CRT_OK;
  return crt::launch_dtau_d_dleaf(kb_nodes, dkb_nodes, L, (long long)n, method, out, static_cast<hipStream_t>(stream));
}

// the gradient of a weighted sum of the level spectra (crt1d_hip_grad.h): both side records (the dlai ones first), then the slice sums
size_t crt_hip_levels_grad_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel) {
  const size_t rec = levels_deriv_workspace_bytes(grad_side_len, scheme, ncol, nz, nb, nsel);
  return rec == 0 ? 0 : rec + grad_part_bytes(ncol, nb);
}

int crt_hip_levels_grad_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                            int32_t nsel, const crt_grad_weights* w, const crt_leaf_tangent* tangent, const crt_grad_out* out,
                            void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  const bool args_ok = w && (w->I_dr || w->I_df_d || w->I_df_u || w->F) && out &&
                       (out->leaf_r || out->leaf_t || out->soil_r || out->lai || out->leaf) &&
                       (!out->leaf || (tangent && tangent->dg_table && tangent->dg_at_psi));
  const SideRecords rec(scheme, cols, bands, nullptr, args_ok, args_ok && out->lai, args_ok && out->leaf, dleaf_tan(tangent));
  return levels_deriv_impl(
      scheme, cols, bands, opts, levels, nsel, workspace, workspace_bytes, stream, args_ok, grad_side_len, rec.report,
      [&](const SolveArgs& sa, const LevArgs& la, const double* side, hipStream_t s, bool probe) {
        return launch_grad(scheme, sa, la,
                           GradArgs{{w->I_dr, w->I_df_d, w->I_df_u, w->F}, {out->leaf_r, out->leaf_t, out->soil_r}, out->lai, out->leaf, side,
                                    rec.side_leaf(side, sa), rec.part(side, sa)},
                           s, probe);
      },
      rec, true, rec.sized ? grad_part_bytes(cols->ncol, bands->nb) : 0);
}

// the Jacobian of the sensor-band sums (crt1d_hip_sensjac.h): the workspace of the gradient with the slice sums of k_sens_jac as its tail
size_t crt_hip_sensor_jac_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel, int32_t nsens, int32_t npar) {
  if (nsens < 1 || nsens > CRT_MAX_SENSOR_BANDS || npar < 1 || npar > CRT_SENSJAC_MAX_NTAN + 2) return 0;
  const size_t rec = levels_deriv_workspace_bytes(grad_side_len, scheme, ncol, nz, nb, nsel);
  return rec == 0 ? 0 : rec + sensjac_part_bytes(ncol, nb, nsel, nsens, npar);
}

// both forms of the sensor Jacobian; ser: the sun-angle series (crt1d_hip_sensjac_series.h), whose tangent carries dg_at_psi as [ncol][nt]
static int sensor_jac_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* ser, bool series,
                           const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                           const crt_optics_dirs* dirs, int with_lai, const DleafTan* tangent, const crt_sensjac_out* out, void* workspace,
                           size_t workspace_bytes, crt_stream_t stream, const crt_col_mask* mask = nullptr) {
  const MaskArg ma = parse_mask(mask, cols);
  SensJacArgs ja = {};
  SensArgs& sn = ja.sn;
  const ParamAxis axis = parse_axis(bands, dirs, with_lai, tangent);
  axis.put(ja);
  bool args_ok = sensors && sensors->first && sensors->count && sensors->w && sensors->nsens >= 1 && sensors->nsens <= CRT_MAX_SENSOR_BANDS &&
                 out && (out->I_dr || out->I_df_d || out->I_df_u || out->F) && axis.ok && (!series || ser) && ma.ok;
  if (args_ok) {
    const int nb = bands->nb;
    sn.o[0] = out->I_dr;
    sn.o[1] = out->I_df_d;
    sn.o[2] = out->I_df_u;
    sn.o[3] = out->F;
    sn.w = sensors->w;
    sn.nsens = sensors->nsens;
    int64_t off = 0;
    for (int k = 0; k < sn.nsens && args_ok; ++k) {
      const int32_t f = sensors->first[k], n = sensors->count[k];
      if (n < 1 || f < 0 || (int64_t)f + n > nb) args_ok = false;
      sn.first[k] = f;
      sn.count[k] = n;
      sn.off[k] = (int32_t)off;
      off += n;  // (<= 64 nb: no overflow)
    }
    if (off > 0x7fffffffLL) args_ok = false;
  }
  const SideRecords rec(scheme, cols, bands, ser, args_ok, axis.lai, axis.leaf, tangent ? *tangent : DleafTan{});
  const bool sel_ok = nsel >= 1 && nsel <= CRT_MAX_LEVEL_SELECT;
  return levels_deriv_impl(
      scheme, cols, bands, opts, levels, nsel, workspace, workspace_bytes, stream, args_ok, grad_side_len, rec.report,
      [&](const SolveArgs& sa, const LevArgs& la, const double* side, hipStream_t s, bool probe) {
        ja.side_lai = side;
        ja.side_leaf = rec.side_leaf(side, sa);
        sn.part = rec.part(side, sa);
        if (!ser) return launch_sens_jac(scheme, sa, la, ja, s, probe, nullptr, nullptr, ma.m);
        const SeriesArgs sr = series_args(scheme, sa, ser);
        return launch_sens_jac(scheme, sa, la, ja, s, probe, &sr, tangent ? tangent->dg_at_psi : nullptr, ma.m);
      },
      rec, true, rec.sized && sel_ok ? sensjac_part_bytes(cols->ncol, bands->nb, nsel, sn.nsens, axis.npar(), ser ? ser->nt : 1) : 0, ser);
}

int crt_hip_sensor_jac_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                           int32_t nsel, const crt_sensor_set* sensors, const crt_optics_dirs* dirs, int with_lai,
                           const crt_leaf_tangent* tangent, const crt_sensjac_out* out, void* workspace, size_t workspace_bytes,
                           crt_stream_t stream) {
  const DleafTan tn = dleaf_tan(tangent);
  return sensor_jac_impl(scheme, cols, bands, nullptr, false, opts, levels, nsel, sensors, dirs, with_lai, tangent ? &tn : nullptr, out, workspace,
                         workspace_bytes, stream);
}

// the sun-angle series of the two (crt1d_hip_sensjac_series.h): the records of a level series, the side records, the slice sums of every (column, t)
size_t crt_hip_sensor_jac_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt, int32_t nsel, int32_t nsens,
                                                 int32_t npar) {
  if (nsel < 1 || nsel > CRT_MAX_LEVEL_SELECT || nsens < 1 || nsens > CRT_MAX_SENSOR_BANDS || npar < 1 || npar > CRT_SENSJAC_MAX_NTAN + 2 || nb <= 0)
    return 0;
  const size_t rec = crt_hip_levels_series_workspace_bytes(scheme, ncol, nz, nt);
  if (rec == 0) return 0;
  const size_t sides = side_bytes(grad_side_len, scheme, ncol, nz), part = sensjac_part_bytes(ncol, nb, nsel, nsens, npar, nt);
  return part > SIZE_MAX - rec - sides ? 0 : rec + sides + part;
}

int crt_hip_sensor_jac_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun, const crt_options* opts,
                                  const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors, const crt_optics_dirs* dirs, int with_lai,
                                  const crt_leaf_tangent_series* tangent, const crt_sensjac_out* out, void* workspace, size_t workspace_bytes,
                                  crt_stream_t stream) {
  const DleafTan tn = dleaf_tan(tangent);
  return sensor_jac_impl(scheme, cols, bands, sun, true, opts, levels, nsel, sensors, dirs, with_lai, tangent ? &tn : nullptr, out, workspace,
                         workspace_bytes, stream);
}

int crt_hip_g_dparam_series_f64(const crt_columns* cols, const crt_sun_series* sun, double* dg_table, double* dg_at_psi, crt_stream_t stream) {
  if (!cols || !sun || !dg_table || !dg_at_psi || !sun->psi || sun->nt < 1 || !cols->g_kind || cols->ncol <= 0) return CRT_ERR_BAD_ARG;
  return crt::launch_g_dparam(cols->ncol, sun->psi, cols->g_kind, cols->g_param, dg_table, dg_at_psi, static_cast<hipStream_t>(stream), sun->nt);
}

// the normal equations of the per-band misfit (crt1d_hip_specfit.h): the workspace of the sensor Jacobian with the slice sums of k_spec_normal as
// its tail
size_t crt_hip_spectral_normal_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel, int32_t nkey, int32_t npar) {
  if (nkey < 1 || nkey > 4 || npar < 1 || npar > CRT_RETRIEVE_MAX_NPAR) return 0;
  const size_t rec = levels_deriv_workspace_bytes(grad_side_len, scheme, ncol, nz, nb, nsel);
  return rec == 0 ? 0 : rec + spec_part_bytes(ncol, nb, nsel, nkey, npar);
}

// the sun-angle series of it (series/crt1d_hip_specfit_series.h): the records of a level series, the side records, the slice sums of every
// (column, t) -- always there: the sum over t goes through them
size_t crt_hip_spectral_normal_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt, int32_t nsel, int32_t nkey,
                                                      int32_t npar) {
  if (crt_hip_spectral_normal_workspace_bytes(scheme, ncol, nz, nb, nsel, nkey, npar) == 0) return 0;
  const size_t rec = crt_hip_levels_series_workspace_bytes(scheme, ncol, nz, nt);
  if (rec == 0) return 0;
  const size_t sides = side_bytes(grad_side_len, scheme, ncol, nz), part = spec_series_part_bytes(ncol, nb, nsel, nkey, npar, nt);
  return part > SIZE_MAX - rec - sides ? 0 : rec + sides + part;
}

// Both forms of the normal equations; ser: the sun-angle series, whose tangent carries dg_at_psi as [ncol][nt] and whose `out` may keep the
// per-step sums A_t / g_t / c2_t (all three or none).  The per-step entry hands its outputs over in the series struct, those three NULL.
static int spectral_normal_impl(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* ser, bool series,
                                const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs, int with_lai,
                                const DleafTan* tangent, const crt_spec_obs* obs, const crt_spec_series_out* out, void* workspace,
                                size_t workspace_bytes, crt_stream_t stream, const crt_col_mask* mask = nullptr) {
  const MaskArg ma = parse_mask(mask, cols);
  SpecArgs sp = {};
  const ParamAxis axis = parse_axis(bands, dirs, with_lai, tangent);
  axis.put(sp);
  const int per_t = out ? (out->A_t != nullptr) + (out->g_t != nullptr) + (out->c2_t != nullptr) : 0;
  bool args_ok = obs && out && out->A && out->g && out->c2 && (per_t == 0 || per_t == 3) && axis.ok && (!series || ser) && ma.ok;
  if (args_ok) {
    const double* const y[4] = {obs->y_I_dr, obs->y_I_df_d, obs->y_I_df_u, obs->y_F};
    const double* const is[4] = {obs->inv_sigma_I_dr, obs->inv_sigma_I_df_d, obs->inv_sigma_I_df_u, obs->inv_sigma_F};
    double* const fwd[4] = {out->fwd_I_dr, out->fwd_I_df_d, out->fwd_I_df_u, out->fwd_F};
    for (int q = 0; q < 4; ++q) {
      if (!y[q]) continue;  // (not observed: its inv_sigma and fwd are not looked at)
      sp.y[q] = y[q];
      sp.is[q] = is[q];
      sp.fwd[q] = fwd[q];
      ++sp.nkey;
    }
    sp.A = out->A, sp.g = out->g, sp.c2 = out->c2;
    args_ok = sp.nkey >= 1;
  }
  const SpecSeriesOut so = args_ok ? SpecSeriesOut{out->A_t, out->g_t, out->c2_t} : SpecSeriesOut{};
  const SideRecords rec(scheme, cols, bands, ser, args_ok, axis.lai, axis.leaf, tangent ? *tangent : DleafTan{});
  const bool tail = rec.sized && nsel >= 1 && nsel <= CRT_MAX_LEVEL_SELECT;
  const int npar = axis.npar();
  return levels_deriv_impl(
      scheme, cols, bands, opts, levels, nsel, workspace, workspace_bytes, stream, args_ok, grad_side_len, rec.report,
      [&](const SolveArgs& sa, const LevArgs& la, const double* side, hipStream_t s, bool probe) {
        sp.side_lai = side;
        sp.side_leaf = rec.side_leaf(side, sa);
        sp.part = rec.part(side, sa);
        if (!ser) return launch_spec_normal(scheme, sa, la, sp, s, probe, ma.m);
        return launch_spec_normal_series(scheme, sa, la, sp, so, series_args(scheme, sa, ser), tangent ? tangent->dg_at_psi : nullptr, s, probe,
                                         ma.m);
      },
      rec, true,
      !tail  ? 0
      : !ser ? spec_part_bytes(cols->ncol, bands->nb, nsel, sp.nkey, npar)
             : spec_series_part_bytes(cols->ncol, bands->nb, nsel, sp.nkey, npar, ser->nt),
      ser);
}

int crt_hip_spectral_normal_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                                int32_t nsel, const crt_optics_dirs* dirs, int with_lai, const crt_leaf_tangent* tangent,
                                const crt_spec_obs* obs, const crt_spec_normal_out* out, void* workspace, size_t workspace_bytes,
                                crt_stream_t stream) {
  const crt_spec_series_out so = out ? crt_spec_series_out{out->A, out->g, out->c2, nullptr, nullptr, nullptr, out->fwd_I_dr, out->fwd_I_df_d,
                                                           out->fwd_I_df_u, out->fwd_F}
                                     : crt_spec_series_out{};
  const DleafTan tn = dleaf_tan(tangent);
  return spectral_normal_impl(scheme, cols, bands, nullptr, false, opts, levels, nsel, dirs, with_lai, tangent ? &tn : nullptr, obs, out ? &so : nullptr,
                              workspace, workspace_bytes, stream);
}

int crt_hip_spectral_normal_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                       const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs,
                                       int with_lai, const crt_leaf_tangent_series* tangent, const crt_spec_obs* obs,
                                       const crt_spec_series_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream) {
  const DleafTan tn = dleaf_tan(tangent);
  return spectral_normal_impl(scheme, cols, bands, sun, true, opts, levels, nsel, dirs, with_lai, tangent ? &tn : nullptr, obs, out, workspace,
                              workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------
// The masked entries (include_mask/crt1d_hip_masked.h): each is its sibling's host path with the mask handed to the launcher.

int crt_hip_sensor_levels_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                                     int32_t nsel, const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace,
                                     size_t workspace_bytes, crt_stream_t stream, const crt_col_mask* mask) {
  return sensor_impl(scheme, cols, bands, opts, levels, nsel, sensors, out, workspace, workspace_bytes, stream, 0, nullptr, true, mask);
}

int crt_hip_sensor_levels_series_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                            const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                            const crt_sensor_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                                            const crt_col_mask* mask) {
  if (!sun) return CRT_ERR_BAD_ARG;
  return sensor_impl(scheme, cols, bands, opts, levels, nsel, sensors, out, workspace, workspace_bytes, stream, 0, sun, true, mask);
}

int crt_hip_sensor_jac_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                                  int32_t nsel, const crt_sensor_set* sensors, const crt_optics_dirs* dirs, int with_lai,
                                  const crt_leaf_tangent* tangent, const crt_sensjac_out* out, void* workspace, size_t workspace_bytes,
                                  crt_stream_t stream, const crt_col_mask* mask) {
  const DleafTan tn = dleaf_tan(tangent);
  return sensor_jac_impl(scheme, cols, bands, nullptr, false, opts, levels, nsel, sensors, dirs, with_lai, tangent ? &tn : nullptr, out, workspace,
                         workspace_bytes, stream, mask);
}

int crt_hip_sensor_jac_series_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                         const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                         const crt_optics_dirs* dirs, int with_lai, const crt_leaf_tangent_series* tangent,
                                         const crt_sensjac_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                                         const crt_col_mask* mask) {
  const DleafTan tn = dleaf_tan(tangent);
  return sensor_jac_impl(scheme, cols, bands, sun, true, opts, levels, nsel, sensors, dirs, with_lai, tangent ? &tn : nullptr, out, workspace,
                         workspace_bytes, stream, mask);
}

int crt_hip_spectral_normal_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                                       const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs, int with_lai,
                                       const crt_leaf_tangent* tangent, const crt_spec_obs* obs, const crt_spec_normal_out* out, void* workspace,
                                       size_t workspace_bytes, crt_stream_t stream, const crt_col_mask* mask) {
  const crt_spec_series_out so = out ? crt_spec_series_out{out->A, out->g, out->c2, nullptr, nullptr, nullptr, out->fwd_I_dr, out->fwd_I_df_d,
                                                           out->fwd_I_df_u, out->fwd_F}
                                     : crt_spec_series_out{};
  const DleafTan tn = dleaf_tan(tangent);
  return spectral_normal_impl(scheme, cols, bands, nullptr, false, opts, levels, nsel, dirs, with_lai, tangent ? &tn : nullptr, obs, out ? &so : nullptr,
                              workspace, workspace_bytes, stream, mask);
}

int crt_hip_spectral_normal_series_masked_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                              const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_optics_dirs* dirs,
                                              int with_lai, const crt_leaf_tangent_series* tangent, const crt_spec_obs* obs,
                                              const crt_spec_series_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream,
                                              const crt_col_mask* mask) {
  const DleafTan tn = dleaf_tan(tangent);
  return spectral_normal_impl(scheme, cols, bands, sun, true, opts, levels, nsel, dirs, with_lai, tangent ? &tn : nullptr, obs, out, workspace,
                              workspace_bytes, stream, mask);
}

int crt_hip_bandsum_finish_f64(const crt_columns* cols, int32_t ngroup, const crt_bandsum_out* out, crt_stream_t stream) {
  if (!cols || !out || !cols->psi || ngroup <= 0 || ngroup > INT_MAXG) return CRT_ERR_BAD_ARG;
  if (!out->aI || !out->aI_sl || !out->aI_sh || !out->I_dr || !out->I_df_d || !out->I_df_u || !out->F || !out->I_d) return CRT_ERR_BAD_ARG;
  if (cols->ncol <= 0 || cols->nz < 2) return CRT_ERR_BAD_ARG;
  if ((long long)cols->nz * ngroup > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;  // a column's (level, group) index is 32-bit
  FinishArgs a;
  a.ncol = cols->ncol;
  a.nz = cols->nz;
  a.ngroup = ngroup;
  a.psi = cols->psi;
  a.aI_sl = out->aI_sl;
  a.aI_sh = out->aI_sh;
  a.L_dr = out->I_dr;
  a.L_dn = out->I_df_d;
  a.L_up = out->I_df_u;
  a.aI = out->aI;
  a.L_F = out->F;
  a.L_Id = out->I_d;
  return launch_bandsum_finish(a, static_cast<hipStream_t>(stream));
}

int crt_hip_band_reduce_f64(const double* X, int64_t nrow, int32_t nb, const double* band_w, int32_t ngroup, double* out, crt_stream_t stream) {
  if (!X || !band_w || !out || nrow < 0 || nb <= 0 || ngroup <= 0 || ngroup > 4) return CRT_ERR_BAD_ARG;
  if (nrow == 0) return CRT_OK;
  if ((nrow + 3) / 4 > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;  // a wave per row, four per workgroup: the grid is 32-bit
  return launch_band_reduce(X, (long long)nrow, nb, band_w, ngroup, out, static_cast<hipStream_t>(stream));
}

int crt_hip_absorb_f64(const crt_columns* cols, const crt_bands* bands, const double* I_dr, const double* I_df_d,
                       const double* I_df_u, double* const* out7, double* laim, double* f_slm, crt_stream_t stream) {
  if (!bands) return CRT_ERR_BAD_ARG;
  return absorb_impl<double>(cols, bands->nb, bands->col_stride, bands->leaf_r, bands->leaf_t, I_dr, I_df_d, I_df_u, out7, laim, f_slm, stream);
}

int crt_hip_absorb_f32(const crt_columns* cols, const crt_bands_f32* bands, const float* I_dr, const float* I_df_d,
                       const float* I_df_u, float* const* out7, double* laim, double* f_slm, crt_stream_t stream) {
  if (!bands) return CRT_ERR_BAD_ARG;
  return absorb_impl<float>(cols, bands->nb, bands->col_stride, bands->leaf_r, bands->leaf_t, I_dr, I_df_d, I_df_u, out7, laim, f_slm, stream);
}

int crt_hip_tau_d_f64(const double* kb_nodes, const double* L, int64_t n, int32_t method, double* out, crt_stream_t stream) {
  if (!kb_nodes || !L || !out || n < 0) return CRT_ERR_BAD_ARG;
  if (method != CRT_TAU_D_QUAD && method != CRT_TAU_D_9SKY) return CRT_ERR_BAD_ARG;  // ValueError, common.py:78
  if (n == 0) return CRT_OK;
  return crt::launch_tau_d(kb_nodes, L, (long long)n, method, out, static_cast<hipStream_t>(stream));
}

const char* crt_hip_last_kernel(void) { return last_kernel(); }

// The fill probe is a YARDSTICK, not a ceiling: a linear fill writes one narrow window of memory at a time, i.e. into one class
// of physical memory (csrc/buffers.hip), and is subject to the same single-class limit as the column pattern -- 6.2-6.6 TB/s with
// this 256-workgroup grid, 4.2-4.5 TB/s with 2048 workgroups (tools/chunk_probe.hip: the wider window of the larger grid is worse,
// so the grid was NOT enlarged) -- while the solve kernels' pattern reaches 7.0 TB/s into a class-balanced set of arrays.
int crt_hip_probe_fill_f64(double* dst, size_t n, double value, crt_stream_t stream) {
  if (!dst || n == 0 || (n & 1) || (reinterpret_cast<uintptr_t>(dst) & 15)) return CRT_ERR_BAD_ARG;
  return launch_kernel(k_fill, dim3(256), 256, 0, static_cast<hipStream_t>(stream), reinterpret_cast<d2*>(dst), n / 2, value);
}

int crt_hip_probe_store_set_f64(double* const* arrays, int32_t narrays, int64_t ncol, int64_t col_doubles, int32_t run_doubles, double value,
                                crt_stream_t stream) {
  if (!arrays || narrays < 1 || narrays > 8 || ncol < 1 || ncol > 0x7fffffff || col_doubles < 2 || (col_doubles & 1) || run_doubles < 2 ||
      (run_doubles & 1))
    return CRT_ERR_BAD_ARG;
  StoreSetArgs a;
  for (int i = 0; i < narrays; ++i) {
    if (!arrays[i] || (reinterpret_cast<uintptr_t>(arrays[i]) & 15)) return CRT_ERR_BAD_ARG;
    a.p[i] = arrays[i];
  }
  a.na = narrays;
  a.ncol = ncol;
  a.col = col_doubles;
  a.run = run_doubles;
  return launch_kernel(k_store_set, dim3((unsigned)ncol), 192, 0, static_cast<hipStream_t>(stream), a, value);
}

// the device math the kernels use instead of ocml's exp / sincos (crt_internal.hpp: fexp, fast_sincos), exposed so that a test can
// bound their error in ulps over the arguments the schemes produce
int crt_hip_probe_math_f64(const double* x, size_t n, double* e, double* sn, double* cs, crt_stream_t stream) {
  if (!x || !e || !sn || !cs || n == 0 || n > 0x7fffffffull * 256) return CRT_ERR_BAD_ARG;
  return launch_kernel(k_probe_math, dim3((unsigned)((n + 255) / 256)), 256, 0, static_cast<hipStream_t>(stream), x, n, e, sn, cs);
}

int crt_hip_probe_copy_f64(double* dst, const double* src, size_t n, crt_stream_t stream) {
  if (!dst || !src || n == 0 || (n & 1) || ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15))
    return CRT_ERR_BAD_ARG;
  return launch_kernel(k_copy, dim3(2048), 256, 0, static_cast<hipStream_t>(stream), reinterpret_cast<d2*>(dst), reinterpret_cast<const d2*>(src),
                       n / 2);
}

}  // extern "C"
