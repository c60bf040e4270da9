// Leaf-angle derivative of the level spectra (include/crt1d_hip_dleaf.h): d X[levels[r]][b] along a tangent (dG at the nodes, dG at the
// sun angle, dmla) of the column's leaf-angle distribution, for X = I_dr, I_df_d, I_df_u, F, by forward-mode differentiation.  The
// per-band maths is that of jac_schemes.hpp: the optics and the LAI entries are plain doubles, the beam fractions and -- unlike the LAI
// derivative -- the header scalars K_b, mu_bar, cos^2 carry the tangent (H = Du).
//
// What depends on the direction (mu, L_j and the optics do not), with Kq = G_q / cos psi_q at the tau_d nodes:
//   K_b' = dG(psi_sun) / mu      Kq' = dG_q / cos psi_q      mu_bar' = sum_q (w_q cos sin / G_q) (-dG_q / G_q)      cos2' = -2 cos m sin m (pi / 180) dmla
//   (e^{-K_b L_j})' = -K_b' L_j e^{-K_b L_j}                  tau_d^th(x) = -2 sum_q w_q sin cos Kq' x e^{-Kq x}
//   bl    the sky term I_df0 tau_d(L_j) brings I_df0 tau_d^th(L_j)
//   n79   (1 - td_j)' = -tau_d^th(D_j),  (1 - tb_j)' = K_b' D_j tb_j,  tbcum_j' as e^{-K_b L_j}     (D_j the layer's dLAI; uniform columns: S_DL)
//   zq    S_TAUI' = tau_d^th(dm),  S_TPSI' = -K_b' dm S_TPSI,  rec[REC_HDR + j]' as e^{-K_b L_j}
//
//  k_dleaf_side  every scheme: one workgroup per column, after K0.  Kq by col_node, the function K0 uses (CRT_G_TABLE columns included), Kq'
//                and the mu_bar' terms in LDS; the mu_bar' sum in col_mubar's order; every level on its own.  Writes the side record:
//                the tangent of the header and of the vectors the scheme's kernel reads (dleaf_side_len, crt_internal.hpp).
//  k_dleaf       2s, bl, g77, bf: k_dlai's mapping (lane <-> band, a workgroup owns one column and one band slice, plain stores of
//                consecutive bands), O(nsel).
//  n79, zq       k_dlai_tri (dlai.hip) through launch_dlai, on this side record: it takes every record entry as value | tangent and reads
//                no header scalar but zq's plain mu.
//  k_g_dparam    dG / d g_param of the parametric kinds at the nodes and at the sun angle (a series: at every sun angle of the column)
//  k_dtau_d_dleaf  tau_d^th for arbitrary L.
#include "col_record.hpp"
#include "deriv_passes.hpp"
#include "launch_forms.hpp"

namespace crt {
namespace {

struct F2s : Sch2s::F {};
struct FBl : SchBl::F {};
template <bool BF>
struct FG77 : SchG77<BF>::F {};

// tau_d^th on the rules of tau_d_quad / tau_d_9sky (colpre.hip): the integrand factor e^{-K L} becomes -K' L e^{-K L}
__device__ inline double dtau_leaf_quad(const double* kq, const double* dkq, double L) {
  double s = 0.0;
  for (int q = 0; q < NQT; ++q) s -= qc.w2sc[q] * ((dkq[q] * L) * fexp(-kq[q] * L));
  return s;
}
__device__ inline double dtau_leaf_9sky(const double* k9, const double* dk9, double L) {
  double s = 0.0;
  for (int i = 0; i < CRT_NQ_9SKY; ++i) s -= ((dk9[i] * L) * fexp(-k9[i] * L)) * qc.sc9[i];
  return s * (2.0 * 0.17453292519943295);  // * 2 radians(10), common.py:51
}

constexpr int SIDE_BLOCK = 128;

// CAN (2s, bl, g77, bf; the sun-angle series of the sensor Jacobian, sensjac.hip): a.ws holds canopy records, and the one entry that follows
// the sun, the header tangent K_b', is left 0 -- neither the sun's slots of the record nor tn.dg_at_psi are read.
template <bool CAN>
__global__ __launch_bounds__(SIDE_BLOCK) void k_dleaf_side(ColArgs a, DleafTan tn, double* __restrict__ side) {
  __shared__ double kq[NQT], dkq[NQT], pm[NQT];
  __shared__ double k9[CRT_NQ_9SKY], dk9[CRT_NQ_9SKY];
  __shared__ double dmb;
  const int c = blockIdx.x, tid = threadIdx.x, nz = a.nz;
  const ColIn in = col_in(a, c);
  const double* dg = tn.dg_table + (long long)c * CRT_NQ;
  for (int q = tid; q < NQT; q += SIDE_BLOCK) {
    double pmb;
    col_node(in, q, kq[q], pmb);
    dkq[q] = dg[q] / qc.cs[q];
    pm[q] = pmb * -(dkq[q] / kq[q]);  // -dG_q / G_q = -Kq' / Kq
  }
  if (tid < CRT_NQ_9SKY) {  // as k_colpre
    k9[tid] = col_node9(in, tid);
    dk9[tid] = dg[NQT + NQG + tid] / qc.cs9[tid];
  }
  __syncthreads();
  if (tid < 64 && a.scheme == CRT_SCHEME_2S) {  // wave 0, whole: col_mubar's order
    const double s = col_mubar(pm[tid], tid < NQT - 64 ? pm[64 + tid] : 0.0, tid);
    if (tid == 0) dmb = s;
  }
  __syncthreads();
  const double* rec = a.ws + (long long)c * (CAN ? can_len(a.scheme, nz) : rec_len(a.scheme, nz));
  const double* lai = in.lai;
  double* sd = side + (long long)c * dleaf_side_len(a.scheme, nz);
  double dK = 0.0;
  if constexpr (!CAN) dK = tn.dg_at_psi[c] / rec[S_MU];
  if (tid < REC_HDR) {
    double t = 0.0;
    if (tid == S_KB) t = dK;
    if (a.scheme == CRT_SCHEME_2S) {
      if (tid == S_MUBAR) t = dmb;
      if (tid == S_COS2 && tn.dmla) {
        const double m = a.mla[c] * (M_PI / 180.0);
        t = -2.0 * cos(m) * sin(m) * ((M_PI / 180.0) * tn.dmla[c]);
      }
    }
    if (a.scheme == CRT_SCHEME_ZQ) {
      const double dm = rec[S_DLM];
      if (tid == S_TAUI) t = dtau_leaf_quad(kq, dkq, dm);  // always 'quad', _solve_zq.py:51
      if (tid == S_TPSI) t = -(dK * dm) * rec[S_TPSI];
    }
    sd[tid] = t;
  }
  double* v = sd + REC_HDR;
  if (a.scheme == CRT_SCHEME_BL) {
    for (int j = tid; j < nz; j += SIDE_BLOCK) v[j] = dtau_leaf_quad(kq, dkq, lai[j]);  // always 'quad', _solve_bl.py:35-37
    return;
  }
  if (CAN || (a.scheme != CRT_SCHEME_N79 && a.scheme != CRT_SCHEME_ZQ)) return;  // 2s, g77, bf: the header alone
  const double Kb = rec[S_KB];
  const bool n79u = a.scheme == CRT_SCHEME_N79 && rec[S_UNIF] != 0.0 && nz >= 3;  // one (tb, td) serves every layer (k_colpre)
  const double dlu = rec[S_DL];
  for (int j = tid; j < nz; j += SIDE_BLOCK) {
    v[j] = -(dK * lai[j]) * rec[REC_HDR + j];  // e^{-K_b L_j}: n79's tbcum, zq's beam fraction
    if (a.scheme != CRT_SCHEME_N79) continue;
    double tb = 0.0, td = 0.0;  // the top level carries no layer: 1 - tb = 1 - td = 1
    if (j + 1 < nz) {
      const double D = n79u ? dlu : lai[j] - lai[j + 1];
      tb = (dK * D) * fexp(-Kb * D);
      td = -(a.tau_d_method == CRT_TAU_D_9SKY ? dtau_leaf_9sky(k9, dk9, D) : dtau_leaf_quad(kq, dkq, D));
    }
    v[nz + j] = tb;
    v[2 * nz + j] = td;
  }
}

__global__ __launch_bounds__(256) void k_dtau_d_dleaf(const double* __restrict__ kb_nodes, const double* __restrict__ dkb_nodes,
                                                       const double* __restrict__ L, long long n, int method, double* __restrict__ out) {
  __shared__ double kq[NQT], dkq[NQT];
  __shared__ double k9[CRT_NQ_9SKY], dk9[CRT_NQ_9SKY];
  for (int q = threadIdx.x; q < NQT; q += blockDim.x) {
    kq[q] = kb_nodes[q];
    dkq[q] = dkb_nodes[q];
  }
  if (threadIdx.x < CRT_NQ_9SKY) {
    k9[threadIdx.x] = kb_nodes[NQT + NQG + threadIdx.x];
    dk9[threadIdx.x] = dkb_nodes[NQT + NQG + threadIdx.x];
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = method == CRT_TAU_D_9SKY ? dtau_leaf_9sky(k9, dk9, L[i]) : dtau_leaf_quad(kq, dkq, L[i]);
}

// ------------------------------------------------------------------------------------------
// dG / d g_param.  The ellipsoidal normalisation (ellipsoidal_p2) is p2(x) = x + A(u), u = 1 - x^2, with
//   A(u) = asin(sqrt u) / sqrt u  (x < 1)  =  asinh(sqrt -u) / sqrt -u  (x > 1)  =  sum_n a_n u^n,   a_n = a_{n-1} (2n - 1)^2 / (2n (2n + 1)),
// one analytic function of u: A' = (1 / x - A) / (2 u) away from u = 0, the series (24 terms: 0.125^24 < 2e-22) for |u| < 1/8 -- the
// quotient form loses 1e-16 / u there and is 0 / 0 at x = 1, where the derivative itself is smooth (p2 = 2, p2' = 2 / 3).
struct Den {
  double p, dp;  // the angle-independent denominator of G and its derivative
};
__device__ inline Den ell_den(double x) {
  const double u = (1.0 - x) * (1.0 + x);
  double A, dA;
  if (fabs(u) < 0.125) {
    double a = 1.0, un = 1.0;
    A = 1.0;
    dA = 0.0;
    for (int n = 1; n <= 24; ++n) {
      a *= ((2.0 * n - 1.0) * (2.0 * n - 1.0)) / ((2.0 * n) * (2.0 * n + 1.0));
      dA += (n * a) * un;
      un *= u;
      A += a * un;
    }
  } else {
    A = ellipsoidal_p2(x) - x;
    dA = (1.0 / x - A) / (2.0 * u);
  }
  return Den{x + A, 1.0 - 2.0 * x * dA};
}

__device__ inline double dG_dparam(int kind, double x, double cs, double sn) {
  switch (kind) {
    case CRT_G_ELLIPSOIDAL:
    case CRT_G_ELLIPSOIDAL_APPROX: {
      Den d;
      if (kind == CRT_G_ELLIPSOIDAL) {
        d = ell_den(x);
      } else {
        d.p = G_den(kind, x);
        d.dp = 1.0 - (0.733 * 1.774) * exp(-1.733 * log(x + 1.182));
      }
      const double R = sqrt(x * x * cs * cs + sn * sn);
      return (x * cs * cs) / (R * d.p) - (R * d.dp) / (d.p * d.p);
    }
    case CRT_G_ELLIPSOIDAL_APPROX_BONAN: {
      if (!(x > -0.4 && x < 0.6)) return 0.0;  // G_eval clamps chi_l
      const double dphi1 = -0.633 - 0.660 * x;
      return dphi1 * (1.0 - (2.0 * 0.877) * cs);  // phi2' = -2 0.877 phi1'
    }
    default: return 0.0;
  }
}

constexpr int GDP_BLOCK = 192;
static_assert(CRT_NQ + 1 <= GDP_BLOCK, "a thread per node and one for the sun");
constexpr int GDP_SUN0 = GDP_BLOCK - CRT_NQ;  // sun states served by the block of the nodes

// psi / dg_at_psi: [ncol][nt].  Block y = 0 of a column: a thread per node, the others the sun states 0 .. GDP_SUN0; block y >= 1: the sun
// states GDP_SUN0 + (y - 1) GDP_BLOCK + tid (a series with more than GDP_SUN0 states).
__global__ __launch_bounds__(GDP_BLOCK) void k_g_dparam(int ncol, int nt, const double* __restrict__ psi, const int32_t* __restrict__ g_kind,
                                                         const double* __restrict__ g_param, double* __restrict__ dg_table,
                                                         double* __restrict__ dg_at_psi) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long t = blockIdx.y == 0 ? tid - CRT_NQ : GDP_SUN0 + (long long)(blockIdx.y - 1) * GDP_BLOCK + tid;
  const bool node = blockIdx.y == 0 && tid < CRT_NQ;
  if (!node && t >= nt) return;
  const int kind = g_kind[c];
  const double x = g_param ? g_param[c] : 0.0;
  double cs, sn;
  if (!node) {
    const double p = psi[(long long)c * nt + t];
    cs = cos(p);
    sn = sin(p);
  } else if (tid < NQT) {
    cs = qc.cs[tid];
    sn = qc.sn[tid];
  } else if (tid < NQT + NQG) {  // the nodes of crt_hip_quad_nodes(0.501, .) (colpre.hip, g4_interval)
    const int g = tid - NQT;
    const double ps = acos(0.501);
    const double lo = g < NGL ? ps : 0.0, hi = g < NGL ? 1.57079632679489661923 : ps;
    const double p = lo + (qc.gx[g % NGL] + 1.0) * (hi - lo) / 2;
    cs = cos(p);
    sn = sin(p);
  } else {
    cs = qc.cs9[tid - NQT - NQG];
    sn = qc.sn9[tid - NQT - NQG];
  }
  const double d = dG_dparam(kind, x, cs, sn);
  if (node)
    dg_table[(long long)c * CRT_NQ + tid] = d;
  else
    dg_at_psi[(long long)c * nt + t] = d;
}

// ------------------------------------------------------------------------------------------
constexpr int DLEAF_BLOCK = 256;

// hd: the record header | e^{-K_b LT} at the ground | ... | the header's tangents at HDR_TAN (jac_schemes.hpp, hdr<Du>)
template <class S, bool BL>
__global__ __launch_bounds__(DLEAF_BLOCK) void k_dleaf(SolveArgs a, LevArgs la, DlaiArgs da, int per) {
  __shared__ double hd[HDR_TAN + REC_HDR];
  __shared__ double lvL[CRT_MAX_LEVEL_SELECT], lvE[CRT_MAX_LEVEL_SELECT], lvT[CRT_MAX_LEVEL_SELECT];
  const int c = blockIdx.x, nz = a.nz, nb = a.nb, nsel = la.nsel, tid = threadIdx.x;
  const int b = blockIdx.y * per + tid;
  const bool live = tid < per && b < nb;
  stage_record<true, BL>(a.ws + (long long)c * a.reclen, nz, la, da.side + (long long)c * (REC_HDR + (BL ? nz : 0)), hd, lvL, lvE, lvT);
  if (!live) return;
  const double invmu = hd[S_INVMU];
  const long long o0 = (long long)c * nsel * nb + b;  // row r: + r nb
  pass_record<S, BL, true>(hd, lvL, lvE, lvT, nsel, load_dband(a, c, b, S::SOIL),
                           [&](int r, double dI, Du dn, Du up) { dlai_store(da, o0 + (long long)r * nb, dI, invmu, dn, up); });
}

template <class S, bool BL = false>
int launch_dleaf_closed(const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe) {
  return launch_deriv_closed(k_dleaf<S, BL>, "k_dleaf", S::NAME, DLEAF_BLOCK, 1, a, la, da, s, probe);
}

}  // namespace

int launch_dleaf(int scheme, const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe) {
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_dleaf_closed<F2s>(a, la, da, s, probe);
    case CRT_SCHEME_BL: return launch_dleaf_closed<FBl, true>(a, la, da, s, probe);
    case CRT_SCHEME_G77: return launch_dleaf_closed<FG77<false>>(a, la, da, s, probe);
    case CRT_SCHEME_BF: return launch_dleaf_closed<FG77<true>>(a, la, da, s, probe);
    case CRT_SCHEME_N79:
    case CRT_SCHEME_ZQ: return launch_dlai(scheme, a, la, da, s, probe);  // k_dlai_tri on this side record (same layout)
    default: return CRT_ERR_UNSUPPORTED;
  }
}

// after K0 on the same stream (the quadrature tables are uploaded by then)
int launch_dleaf_side(const ColArgs& ca, const DleafTan& tn, double* side, hipStream_t s, bool canopy) {
  if (canopy) return launch_kernel(k_dleaf_side<true>, dim3(ca.ncol), SIDE_BLOCK, 0, s, ca, tn, side);
  return launch_kernel(k_dleaf_side<false>, dim3(ca.ncol), SIDE_BLOCK, 0, s, ca, tn, side);
}

int launch_g_dparam(int ncol, const double* psi, const int32_t* g_kind, const double* g_param, double* dg_table, double* dg_at_psi,
                    hipStream_t s, int nt) {
  const long long ny = 1 + (nt > GDP_SUN0 ? ((long long)nt - GDP_SUN0 + GDP_BLOCK - 1) / GDP_BLOCK : 0);
  if (ny > 65535) return CRT_ERR_UNSUPPORTED;
  const int st = init_quadrature(s);
  if (st != CRT_OK) return st;
  return launch_kernel(k_g_dparam, dim3(ncol, (unsigned)ny), GDP_BLOCK, 0, s, ncol, nt, psi, g_kind, g_param, dg_table, dg_at_psi);
}

int launch_dtau_d_dleaf(const double* kb_nodes, const double* dkb_nodes, const double* L, long long n, int method, double* out,
                        hipStream_t s) {
  return launch_per_lai(k_dtau_d_dleaf, n, s, kb_nodes, dkb_nodes, L, n, method, out);
}

int upload_quad_dleaf(const QuadConst& h, hipStream_t s) { return upload_qc(h, s); }

}  // namespace crt
