// Host side of the solve launchers (no device code): the launch-bound dispatch, the "next form while unsupported" chain, and ONE launch
// sequence per output form -- level subsets (per step, series, sensor, sensor series) and integrated sums (per step, series) -- which the
// three kernel families (closed forms: solve_closed.hip; n79 / zq: tri_tile_impl.hpp; zq_pa: tri_zqpa.hip) fill in with a small description
// each.  A new output form is a new sequence here plus one `launch` branch per family; a new family is a new description.  The level
// derivatives (jac.hip, dlai.hip, dleaf.hip) have one sequence per kernel shape at the end.
#pragma once
#include <cstdio>

#include "crt_internal.hpp"

namespace crt {

// thread count -> the launch bound of the kernel instantiation that serves it, as a compile-time constant:
//   with_bound(nthr, [&](auto B) { return go(k_x<S, TIO, B()>); })
template <int N>
using Bound = std::integral_constant<int, N>;
template <class F>
inline auto with_bound(int nthr, F f) {
  if (nthr <= 256) return f(Bound<256>{});
  if (nthr <= 512) return f(Bound<512>{});
  return f(Bound<1024>{});
}
// the pipeline kernels (compute waves + store waves) have no 256 form
template <class F>
inline auto with_pipe_bound(int nthr, F f) {
  return nthr <= 512 ? f(Bound<512>{}) : f(Bound<1024>{});
}

// the attempts in the order written, each a callable returning a status: the first status that is not CRT_ERR_UNSUPPORTED, else the last
template <class F, class... Rest>
inline int first_supported(F f, Rest... rest) {
  const int st = f();
  if constexpr (sizeof...(Rest) > 0)
    if (st == CRT_ERR_UNSUPPORTED) return first_supported(rest...);
  return st;
}

constexpr size_t MAX_WG_LDS = 160 * 1024;

// ------------------------------------------------------------------------------------------
// Level subsets.  What a family's `launch` and `note` see of the launch the sequence below has configured:
struct LevLaunch {
  const LevArgs& la;
  hipStream_t s;
  const SeriesArgs* sr;  // series forms, else nullptr
  const SensLaunch* sl;  // sensor forms, else nullptr
  LevSlices ls;
  size_t sh;             // LDS bytes
  bool in_lds;           // false: the record is read from the workspace (sh does not fit; per-step form of a family with HBM_RECORD)
  dim3 grid;
};

// A family description F has
//   static constexpr bool FIT          the band slices are narrowed until lds_bytes fits (lev_slices_fit); else lev_slices(nb, 1024)
//   static constexpr bool HBM_RECORD   the per-step kernel has a form that reads the record from the workspace when it exceeds the LDS
//   size_t lds_bytes(int nthr, bool sens) const
//   template <int MAXT, bool SER, bool SENS, bool IN_LDS> int launch(const LevLaunch&) const      launch_kernel of its kernel, with its
//                                                                                                 trailing arguments (IN_LDS = L.in_lds)
//   void note(const LevLaunch&) const                                                its report (lev_note)
// Order: slices, LDS, series grid, sens_probe (records the slice count: the workspace query is a probe), probe return -- nothing is
// launched in probe mode --, kernel, sens_finish, report.  Every refusal is CRT_ERR_UNSUPPORTED.  The sensor series has no f32 form.
template <typename TIO, class F>
int launch_lev_form(const F& f, const SolveArgs& a, const LevArgs& la, hipStream_t s, const SeriesArgs* sr, bool probe, SensLaunch* sl) {
  const bool sens = sl != nullptr;
  LevLaunch L{la, s, sr, sl, {}, 0, true, {}};
  if constexpr (F::FIT)
    L.ls = lev_slices_fit(a.nb, MAX_WG_LDS, [&](int nthr) { return f.lds_bytes(nthr, sens); });
  else
    L.ls = lev_slices(a.nb, 1024);
  const LevSlices& ls = L.ls;
  if (ls.nslice == 0 || ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  L.sh = f.lds_bytes(ls.nthr, sens);
  L.in_lds = L.sh <= MAX_WG_LDS;
  if (!L.in_lds && (sens || sr || !F::HBM_RECORD)) return CRT_ERR_UNSUPPORTED;  // (the series has no assembled record in the workspace)
  L.grid = dim3(a.ncol, ls.nslice);
  if (sr && ((sens && sizeof(TIO) != 8) || !lev_series_grid(a.ncol, sr->nt, ls.nslice, &L.grid))) return CRT_ERR_UNSUPPORTED;
  const long long nv = (long long)a.ncol * (sr ? sr->nt : 1);
  if (sens)
    if (const int st = sens_probe(sl, ls, nv, la.nsel)) return st;
  if (probe) return CRT_OK;
  // (the form outside, the launch bound inside: the kernels are instantiated form by form, which is their order in the code object)
  auto go = [&](auto SER, auto SENS, auto IN_LDS) {
    return with_bound(ls.nthr, [&](auto B) { return f.template launch<B(), decltype(SER)::value, decltype(SENS)::value, decltype(IN_LDS)::value>(L); });
  };
  constexpr std::true_type Y{};
  constexpr std::false_type N{};
  int st = CRT_ERR_UNSUPPORTED;
  if (sens && sr) {
    if constexpr (sizeof(TIO) == 8) st = go(Y, Y, Y);
  } else if (sens) {
    st = go(N, Y, Y);
  } else if (sr) {
    st = go(Y, N, Y);
  } else {
    st = !L.in_lds ? go(N, N, N) : go(N, N, Y);
  }
  if (st == CRT_OK && sens) st = sens_finish(sl, ls, nv, a.nb, la.nsel, s, sr ? sr->nt : 1);
  if (st == CRT_OK) f.note(L);  // (only a launch that succeeded is reported)
  return st;
}

// the report of a level launch: kernel `kern`<`name`>, `mid` = the family's own fields (" M=8", " M=8 grid=100", "")
inline void lev_note(const LevLaunch& L, const char* kern, const char* name, bool f32, const char* mid) {
  const char* pre = L.sr ? "k_colpre<canopy> + k_colsun + " : "";
  const char* io = f32 ? " f32" : "";
  const int nsel = L.la.nsel, per = L.ls.per;
  if (L.sl)
    note_kernel("%s%s_sens%s%s<%s>%s%s nsel=%d nsens=%d slice=%d%s", pre, kern, L.sr ? "_series" : "", L.sl->mask.skip ? "_masked" : "", name, io,
                mid, nsel, L.sl->sn.nsens, per, L.ls.nslice <= 1 ? "" : L.sl->mask.skip ? " + k_sens_finish_masked" : " + k_sens_finish");
  else if (L.sr)
    note_kernel("%s%s_series<%s>%s%s nsel=%d slice=%d nt=%d", pre, kern, name, io, mid, nsel, per, L.sr->nt);
  else
    note_kernel("%s<%s>%s%s nsel=%d slice=%d%s", kern, name, io, mid, nsel, per, L.in_lds ? "" : " record in HBM");
}

// ------------------------------------------------------------------------------------------
// Integrated sums: one workgroup of nthr lanes per column (series: per (column, sun state)).
struct IntLaunch {
  const IntArgs& ia;
  hipStream_t s;
  const SeriesArgs* sr;  // series form, else nullptr
  int nthr;
  size_t sh;
  dim3 grid;
  bool prof;             // the level profiles are asked for
};

// A family description F has
//   size_t lds_bytes(int nthr, bool prof) const
//   template <int MAXT, bool SER, bool PROF> int launch(const IntLaunch&) const      launch_kernel of its kernel, with its trailing arguments
//   void note(const IntLaunch&) const
// The series has no f32 form.
template <typename TIO, class F>
int launch_int_form(const F& f, const SolveArgs& a, const IntArgs& ia, hipStream_t s, int nthr, const SeriesArgs* sr) {
  IntLaunch L{ia, s, sr, nthr, 0, sr ? series_grid(a.ncol, sr->nt) : dim3(a.ncol), ia.L_dr != nullptr};
  L.sh = f.lds_bytes(nthr, L.prof);
  if (L.sh > MAX_WG_LDS || (sr && sizeof(TIO) != 8)) return CRT_ERR_UNSUPPORTED;
  // (series and profiles outside, the launch bound inside: the kernels' order in the code object)
  auto go = [&](auto SER, auto PROF) { return with_bound(nthr, [&](auto B) { return f.template launch<B(), decltype(SER)::value, decltype(PROF)::value>(L); }); };
  constexpr std::true_type Y{};
  constexpr std::false_type N{};
  int st = CRT_ERR_UNSUPPORTED;
  if (sr) {
    if constexpr (sizeof(TIO) == 8) st = L.prof ? go(Y, Y) : go(Y, N);
  } else {
    st = L.prof ? go(N, Y) : go(N, N);
  }
  if (st == CRT_OK) f.note(L);  // (only a launch that succeeded is reported)
  return st;
}

// ------------------------------------------------------------------------------------------
// Level derivatives (jac.hip, dlai.hip, dleaf.hip): lane <-> band, a workgroup owns one column and one band slice, gz is the grid's third
// extent (the Jacobian's parameter axis, else 1).  `out` is the kernel's output block (JacArgs, DlaiArgs); the report is
// "kname<sname> nsel= slice=".  probe: the status of the configuration (CRT_OK / CRT_ERR_UNSUPPORTED), nothing launched.

// closed forms: balanced slices of at most `block` lanes; kernel arguments (a, la, out, slice width)
template <class K, class Out>
int launch_deriv_closed(K kern, const char* kname, const char* sname, int block, unsigned gz, const SolveArgs& a, const LevArgs& la,
                        const Out& out, hipStream_t s, bool probe) {
  const LevSlices ls = lev_slices(a.nb, block);
  if (ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const int st = launch_kernel(kern, dim3(a.ncol, ls.nslice, gz), ls.nthr, 0, s, a, la, out, ls.per);
  if (st == CRT_OK) note_kernel("%s<%s> nsel=%d slice=%d", kname, sname, la.nsel, ls.per);
  return st;
}

// n79 / zq: one wave per workgroup with W = tri_cp_lanes(scheme, nz, copies) lanes at work; kernel arguments (a, la, out, W, the staged
// record doubles, their even-rounded count = the offset of what follows them in LDS)
template <class K, class Out>
int launch_deriv_tri(K kern, const char* kname, const char* sname, int scheme, int copies, unsigned gz, const SolveArgs& a, const LevArgs& la,
                     const Out& out, hipStream_t s, bool probe) {
  const int W = tri_cp_lanes(scheme, a.nz, copies);
  if (W == 0) return CRT_ERR_UNSUPPORTED;
  const long long nslice = ((long long)a.nb + W - 1) / W;
  if (nslice > 65535) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const int nrec = jac_tri_nrec(scheme, a.nz), off = (nrec + 1) & ~1;
  const int st = launch_kernel(kern, dim3(a.ncol, (unsigned)nslice, gz), 64, tri_cp_lds_bytes(scheme, a.nz, W, copies), s, a, la, out, W, nrec, off);
  if (st == CRT_OK) note_kernel("%s<%s> nsel=%d slice=%d", kname, sname, la.nsel, W);
  return st;
}

// tau_d' and its kin: one thread per LAI value, 256 per workgroup, once the quadrature tables are on the device; `args`: the kernel's
template <class K, class... Args>
int launch_per_lai(K kern, long long n, hipStream_t s, Args... args) {
  const int st = init_quadrature(s);
  if (st != CRT_OK) return st;
  const long long nblk = (n + 255) / 256;
  if (nblk > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  return launch_kernel(kern, dim3((unsigned)nblk), 256, 0, s, args...);
}

}  // namespace crt
