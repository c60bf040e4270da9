// Spectral normal equations and the step on them (include/crt1d_hip_specfit.h): A = J^T W J, g = J^T W r and c2 = sum r^2 of the per-band
// misfit of the level spectra, for the closed forms 2s, bl, g77, bf.  The optics Jacobian (jac.hip) along ntan directions, the LAI
// derivative (dlai.hip) and the leaf-angle derivative (dleaf.hip) are contracted where they are formed: the Jacobian [nsel * nb][npar] of a
// column, the eleven derivative arrays behind it and the level spectra are never written.
//
//  k_spec_normal         (its body: spec_normal_body of specfit_body.hpp, shared with k_spec_normal_series of specfit_series.hip)
//                        k_grad's mapping: lane <-> band, a workgroup owns one column and one band slice; the header with its leaf-angle
//                        tangents and the selected record entries are staged in LDS once, a lane loads its band once and runs the passes of
//                        deriv_passes.hpp one after the other, ONE tangent at a time -- the tangent bits of the single-derivative kernels
//                        (-ffp-contract=off).  A lane keeps (w_0 .. w_{npar-1}, r) of every (observed key, level) in LDS entries that only
//                        it reads and writes, rows [nkey][nsel][npar + 1][lanes] -- no barrier between the passes:
//                          primal       pass_optics<Sch::J> with no seed: X into the r entry (and to fwd); the ONE place X comes from, so r,
//                                       c2 and fwd do not depend on which parameters exist (the unused tangents are dead code)
//                          directions   the unit-seed passes p = leaf_r, leaf_t, soil_r add X'_p d_p[k][b] in this order (k_sens_jac's order)
//                          LAI          pass_record<Sch::D>
//                          leaf angle   pass_record<Sch::F, LEAF>
//                          weights      w_i = X'_i s, r = (X - y) s; a row with s == 0 becomes a row of +0
//                        Then the (npar + 1)(npar + 2) / 2 entries of (A | g | c2) one at a time: the lane adds its products over (key, level),
//                        spec_block_sum (grad.hip's block_sum: butterfly, then the waves in ascending order) adds the lanes, thread 0 stores.  The 66 sums
//                        of npar = 10 are never live together: no accumulator sits in a register across a pass.
//  k_spec_normal_finish  several band slices: a thread per (column, entry) adds the slice sums in ascending order (k_grad_finish's rule).
//  k_lm_step_normal      k_lm_step (retrieve.hip) with the sums supplied instead of rows.  The scaled Cholesky and the solve are the ones
//                        retrieve.hip uses (lm_common.hpp).
// No atomics anywhere: a column's result does not depend on the batch or on another column's mask.
#include "lm_common.hpp"
#include "specfit_body.hpp"

namespace crt {
namespace {

struct P2s : Sch2s {};
struct PBl : SchBl {};
template <bool BF>
struct PG77 : SchG77<BF> {};

constexpr int MAXA = MAXP + 1;                  // (w_0 .. w_{npar-1}, r)
constexpr int MAXENT = MAXA * (MAXA + 1) / 2;   // 66 entries of (A | g | c2)
constexpr int LM_WAVE = 64;                     // one wave per column

// The body (specfit_body.hpp) on the record k_colpre wrote: one column and one band slice per workgroup.
template <class G, bool BL>
__global__ __launch_bounds__(SPEC_BLOCK) void k_spec_normal(SolveArgs a, LevArgs la, SpecArgs sp, int per) {
  const int c = blockIdx.x;
  spec_normal_body<G, BL, false>(a, la, sp, per, c, blockIdx.y, c, SpecRecStep{a.ws + (long long)c * a.reclen, a.nz}, 0);
}

// One thread per (column, entry): the slice sums in ascending slice order, starting from slice 0's bits.  MASKED: an entry of a skipped
// column keeps its bits, and its slice sums are not read.
template <bool MASKED>
__device__ __forceinline__ void spec_finish_body(long long ncol, int nslice, int npar, const double* __restrict__ part, double* __restrict__ A,
                                                 double* __restrict__ g, double* __restrict__ c2, ColMask m) {
  const int ntri = npar * (npar + 1) / 2, nent = (npar + 1) * (npar + 2) / 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncol * nent) return;
  const long long c = i / nent;
  if constexpr (MASKED)
    if (col_skipped(m, (int)c)) return;
  const int e = (int)(i - c * nent);
  const double* p = part + c * nslice * nent + e;
  double s = p[0];
  for (int sl = 1; sl < nslice; ++sl) s += p[(long long)sl * nent];
  if (e < ntri) A[c * ntri + e] = s;
  else if (e < ntri + npar) g[c * npar + e - ntri] = s;
  else c2[c] = s;
}

__global__ __launch_bounds__(256) void k_spec_normal_finish(long long ncol, int nslice, int npar, const double* __restrict__ part,
                                                             double* __restrict__ A, double* __restrict__ g, double* __restrict__ c2) {
  spec_finish_body<false>(ncol, nslice, npar, part, A, g, c2, ColMask{});
}

// ---- the masked forms (include_mask/crt1d_hip_masked.h): every workgroup of a skipped column returns before it reads anything of the
// column and before any barrier; an evaluated column runs the body of its plain sibling.
template <class G, bool BL>
__global__ __launch_bounds__(SPEC_BLOCK) void k_spec_normal_masked(SolveArgs a, LevArgs la, SpecArgs sp, int per, ColMask m) {
  const int c = blockIdx.x;
  if (col_skipped(m, c)) return;
  spec_normal_body<G, BL, false>(a, la, sp, per, c, blockIdx.y, c, SpecRecStep{a.ws + (long long)c * a.reclen, a.nz}, 0);
}

__global__ __launch_bounds__(256) void k_spec_normal_finish_masked(long long ncol, int nslice, int npar, const double* __restrict__ part,
                                                                    double* __restrict__ A, double* __restrict__ g, double* __restrict__ c2,
                                                                    ColMask m) {
  spec_finish_body<true>(ncol, nslice, npar, part, A, g, c2, m);
}

template <class G, bool BL = false>
int launch_spec_closed(const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, hipStream_t s, bool probe, ColMask m) {
  const int npar = sp.ntan + sp.lai + sp.leaf;
  const LevSlices ls = spec_slices(a.nb, la.nsel, sp.nkey, npar);
  if (ls.nslice == 0 || ls.nslice > 65535) return CRT_ERR_UNSUPPORTED;
  if (probe) return CRT_OK;
  const size_t sh = spec_rows(la.nsel, sp.nkey, npar) * ls.nthr * sizeof(double);  // (<= the bound of spec_slices)
  const bool fin = ls.nslice > 1;
  const long long n = (long long)a.ncol * spec_nent(npar);  // (< 2^31 * 66: the grid fits)
  const dim3 gfin((unsigned)((n + 255) / 256));
  int st;
  if (m.skip) {
    st = launch_kernel(k_spec_normal_masked<G, BL>, dim3(a.ncol, ls.nslice), ls.nthr, sh, s, a, la, sp, ls.per, m);
    if (st == CRT_OK && fin)
      st = launch_kernel(k_spec_normal_finish_masked, gfin, 256, 0, s, (long long)a.ncol, ls.nslice, npar, sp.part, sp.A, sp.g, sp.c2, m);
  } else {
    st = launch_kernel(k_spec_normal<G, BL>, dim3(a.ncol, ls.nslice), ls.nthr, sh, s, a, la, sp, ls.per);
    if (st == CRT_OK && fin)
      st = launch_kernel(k_spec_normal_finish, gfin, 256, 0, s, (long long)a.ncol, ls.nslice, npar, sp.part, sp.A, sp.g, sp.c2);
  }
  if (st == CRT_OK)
    note_kernel("k_spec_normal%s<%s> nsel=%d nkey=%d npar=%d slice=%d%s", m.skip ? "_masked" : "", G::J::NAME, la.nsel, sp.nkey, npar, ls.per,
                !fin ? "" : m.skip ? " + k_spec_normal_finish_masked" : " + k_spec_normal_finish");
  return st;
}

// ------------------------------------------------------------------------------------------
// the step on supplied sums: k_lm_step of retrieve.hip, line by line, with the row loop replaced by the block loads

struct LmNormalArgs {
  SumBlock blk[CRT_LM_MAX_BLOCKS];
  int nblk, npar;
  double lam_up, lam_down, lam_min, lam_max, xtol, ftol;
  const double *lo, *hi, *prior, *isp;
  crt_lm_state st;
};

__global__ __launch_bounds__(LM_WAVE) void k_lm_step_normal(LmNormalArgs a) {
  __shared__ double ent[MAXENT + 2];  // (A | g | 2 cost)
  __shared__ double M[MAXP * MAXP];
  __shared__ double sc[MAXP], dl[MAXP];
  __shared__ bool dead[MAXP];
  const long long c = blockIdx.x;
  const int lane = threadIdx.x;
  const crt_lm_state& S = a.st;
  if (S.status[c] != CRT_LM_RUNNING) return;  // (the whole wave, before any barrier)
  const int npar = a.npar, na = npar + 1, ntri = npar * (npar + 1) / 2, nent = na * (na + 1) / 2;
  const int e0 = lane, e1 = lane + LM_WAVE;
  const bool has0 = e0 < nent, has1 = e1 < nent;
  int i0 = 0, j0 = 0, i1 = 0, j1 = 0;
  if (has0) tri_pair(e0, i0, j0);
  if (has1) tri_pair(e1, i1, j1);
  double acc0 = 0.0, acc1 = 0.0;
  if (has0) acc0 = block_entry(a.blk[0], c, e0, ntri, npar);
  if (has1) acc1 = block_entry(a.blk[0], c, e1, ntri, npar);
  for (int q = 1; q < a.nblk; ++q) {
    if (has0) acc0 = acc0 + block_entry(a.blk[q], c, e0, ntri, npar);
    if (has1) acc1 = acc1 + block_entry(a.blk[q], c, e1, ntri, npar);
  }
  if (a.isp) {
    for (int k = 0; k < npar; ++k) {
      const double s = a.isp[c * npar + k];
      if (s == 0.0) continue;
      const double d = (S.p_trial[c * npar + k] - a.prior[c * npar + k]) * s;
      if (has0) {
        if (i0 == k && j0 == k) acc0 = acc0 + s * s;
        else if (i0 == npar && j0 == k) acc0 = acc0 + s * d;
        else if (i0 == npar && j0 == npar) acc0 = acc0 + d * d;
      }
      if (has1) {
        if (i1 == k && j1 == k) acc1 = acc1 + s * s;
        else if (i1 == npar && j1 == k) acc1 = acc1 + s * d;
        else if (i1 == npar && j1 == npar) acc1 = acc1 + d * d;
      }
    }
  }
  if (has0) ent[e0] = acc0;
  if (has1) ent[e1] = acc1;
  __syncthreads();

  // ---- accept / reject: every lane takes the same decisions from the same values ----
  const double cost_t = 0.5 * ent[nent - 1];
  const double cost = S.cost[c];
  double lam = S.lam[c];
  int status = CRT_LM_RUNNING;
  const bool accept = cost_t < cost;
  double new_cost = cost;
  if (accept) {
    if (lane < npar) S.p[c * npar + lane] = S.p_trial[c * npar + lane];
    if (has0 && e0 < ntri) S.A[c * ntri + e0] = acc0;
    if (has0 && e0 >= ntri && e0 < ntri + npar) S.g[c * npar + e0 - ntri] = acc0;
    if (has1 && e1 < ntri + npar) S.g[c * npar + e1 - ntri] = acc1;  // (e1 >= 64 > ntri)
    lam = fmax(lam * a.lam_down, a.lam_min);
    if (cost - cost_t < a.ftol * cost_t) status = CRT_LM_CONVERGED_F;
    new_cost = cost_t;
  } else if (cost == INFINITY) {
    status = CRT_LM_FAILED_START;
  } else {
    lam = lam * a.lam_up;
    if (lam > a.lam_max) status = CRT_LM_STALLED;
    __syncthreads();
    if (has0 && e0 < ntri) ent[e0] = S.A[c * ntri + e0];
    if (has0 && e0 >= ntri && e0 < ntri + npar) ent[e0] = S.g[c * npar + e0 - ntri];
    if (has1 && e1 < ntri + npar) ent[e1] = S.g[c * npar + e1 - ntri];
    __syncthreads();
  }

  // ---- the next trial point ----
  bool conv_x = false;
  double pk = 0.0, pt = 0.0;
  if (status == CRT_LM_RUNNING) {
    if (lane == 0) {
      scaled_cholesky(ent, npar, lam, M, sc, dead);
      for (int k = 0; k < npar; ++k) dl[k] = -ent[ntri + k] * sc[k];
      cholesky_solve(M, npar, dl);
      for (int k = 0; k < npar; ++k) dl[k] = dl[k] * sc[k];
    }
    __syncthreads();
    bool far = false;
    if (lane < npar) {
      pk = S.p[c * npar + lane];  // (written by this lane where the step was accepted)
      pt = pk + dl[lane];
      if (a.lo && pt < a.lo[lane]) pt = a.lo[lane];
      if (a.hi && pt > a.hi[lane]) pt = a.hi[lane];
      far = !(fabs(pt - pk) < a.xtol * (fabs(pk) + a.xtol));
    }
    conv_x = !__any(far);
    if (conv_x) status = CRT_LM_CONVERGED_X;
  } else if (lane < npar) {
    pk = S.p[c * npar + lane];
  }
  if (lane < npar) S.p_trial[c * npar + lane] = status == CRT_LM_RUNNING ? pt : pk;
  if (lane == 0) {
    S.cost[c] = new_cost;
    S.lam[c] = lam;
    S.status[c] = status;
    if (accept) S.naccept[c] += 1;
    else if (status != CRT_LM_FAILED_START) S.nreject[c] += 1;
  }
}

}  // namespace

int launch_spec_normal(int scheme, const SolveArgs& a, const LevArgs& la, const SpecArgs& sp, hipStream_t s, bool probe, ColMask m) {
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_spec_closed<P2s>(a, la, sp, s, probe, m);
    case CRT_SCHEME_BL: return launch_spec_closed<PBl, true>(a, la, sp, s, probe, m);
    case CRT_SCHEME_G77: return launch_spec_closed<PG77<false>>(a, la, sp, s, probe, m);
    case CRT_SCHEME_BF: return launch_spec_closed<PG77<true>>(a, la, sp, s, probe, m);
    default: return CRT_ERR_UNSUPPORTED;
  }
}

}  // namespace crt

using namespace crt;

extern "C" {

int crt_hip_lm_step_normal_f64(const crt_lm_problem* prob, const crt_lm_normal_block* blocks, int32_t nblk, const crt_lm_state* state,
                               crt_stream_t stream) {
  if (!blocks || !lm_problem_ok(prob, nblk, state)) return CRT_ERR_BAD_ARG;
  LmNormalArgs a = {};
  for (int q = 0; q < nblk; ++q) {
    if (!blocks[q].A || !blocks[q].g || !blocks[q].c2) return CRT_ERR_BAD_ARG;
    a.blk[q] = SumBlock{blocks[q].A, blocks[q].g, blocks[q].c2};
  }
  a.nblk = nblk, a.npar = prob->npar;
  a.lam_up = prob->lam_up, a.lam_down = prob->lam_down, a.lam_min = prob->lam_min, a.lam_max = prob->lam_max;
  a.xtol = prob->xtol, a.ftol = prob->ftol;
  a.lo = prob->lo, a.hi = prob->hi, a.prior = prob->prior, a.isp = prob->inv_sigma_prior;
  a.st = *state;
  const int st = launch_kernel(k_lm_step_normal, dim3(prob->ncol), LM_WAVE, 0, static_cast<hipStream_t>(stream), a);
  if (st == CRT_OK) note_kernel("k_lm_step_normal npar=%d nblk=%d", prob->npar, nblk);
  return st;
}

}  // extern "C"
