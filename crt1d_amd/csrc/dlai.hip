// LAI derivative of the level spectra (include/crt1d_hip_dlai.h): d X[levels[r]][b] / d s at s = 1 of lai(s) = s lai, for X = I_dr, I_df_d,
// I_df_u, F, by forward-mode differentiation.  The per-band maths is that of jac_schemes.hpp with the roles swapped: the optics are plain
// doubles, the entries of the column record carry the tangent.
//
// What depends on s (nothing else does: K_b, mu, mu_bar, the G integrals, cos^2 and the optics are functions of the angles alone):
//   L_j' = L_j, LT' = LT                          (e^{-K_b L_j})' = -K_b L_j e^{-K_b L_j}
//   bl    (tau_d(L_j))' = L_j tau_d'(L_j)
//   n79   (1 - td_j)' = -D_j tau_d'(D_j),  (1 - tb_j)' = K_b D_j tb_j,  tbcum_j' as e^{-K_b L_j}     (D_j the layer's dLAI; uniform columns: S_DL)
//   zq    dm' = dm,  S_TAUI' = dm tau_d'(dm),  S_TPSI' = -K_b dm S_TPSI,  rec[REC_HDR + j]' as e^{-K_b L_j}   (dm = S_DLM, the one mean dLAI)
// with tau_d'(x) = -2 int K_b(psi) e^{-K_b(psi) x} sin psi cos psi dpsi on the nodes and weights of tau_d ('quad') or the nine sky angles.
//
//  k_dlai_side  bl, n79, zq: one workgroup per column, after K0.  K_b at the tau_d nodes by col_node, the function K0 uses (CRT_G_TABLE
//               columns included), K_b(psi_sun) and the dLAI statistics from the record K0 has just written; every level on its own.
//               Writes the side record (DlaiArgs, crt_internal.hpp) behind the K0 records.
//  k_dlai       2s, bl, g77, bf: k_jac's mapping without the parameter axis (lane <-> band, a workgroup owns one column and one band slice,
//               plain stores of consecutive bands); L_j, LT, e^{-K_b L_j} are seeded from the record itself, O(nsel).
//  k_dlai_tri   n79, zq: k_jac_tri's checkpoint-every-fourth-level sweep with the record entries as Du: the staged record part is in LDS
//               twice (values | tangents of the side record), so the lanes narrow earlier (tri_cp_lanes with two copies).
#include "col_record.hpp"
#include "deriv_passes.hpp"
#include "launch_forms.hpp"

namespace crt {
namespace {

struct D2s : Sch2s::D {};
struct DBl : SchBl::D {};
template <bool BF>
struct DG77 : SchG77<BF>::D {};
struct DN79 : JN79T<double, Du> {};
struct DZq : JZqT<double, Du> {};

// ------------------------------------------------------------------------------------------
// tau_d' on the rules of tau_d_quad / tau_d_9sky (colpre.hip): the integrand factor e^{-K_b L} becomes -K_b e^{-K_b L}
__device__ inline double dtau_d_quad(const double* kq, double L) {
  double s = 0.0;
  for (int q = 0; q < NQT; ++q) s -= qc.w2sc[q] * (kq[q] * fexp(-kq[q] * L));
  return s;
}
__device__ inline double dtau_d_9sky(const double* k9, double L) {
  double s = 0.0;
  for (int i = 0; i < CRT_NQ_9SKY; ++i) s -= (k9[i] * fexp(-k9[i] * L)) * qc.sc9[i];
  return s * (2.0 * 0.17453292519943295);  // * 2 radians(10), common.py:51
}

constexpr int SIDE_BLOCK = 128;

__global__ __launch_bounds__(SIDE_BLOCK) void k_dlai_side(ColArgs a, double* __restrict__ side) {
  __shared__ double kq[NQT];
  __shared__ double k9[CRT_NQ_9SKY];
  const int c = blockIdx.x, tid = threadIdx.x, nz = a.nz;
  const ColIn in = col_in(a, c);
  for (int q = tid; q < NQT; q += SIDE_BLOCK) {
    double pmb;
    col_node(in, q, kq[q], pmb);
  }
  if (tid < CRT_NQ_9SKY) k9[tid] = col_node9(in, tid);  // as k_colpre
  __syncthreads();
  const double* rec = a.ws + (long long)c * rec_len(a.scheme, nz);
  const double* lai = in.lai;
  double* sd = side + (long long)c * dlai_side_len(a.scheme, nz);
  const double Kb = rec[S_KB];
  if (a.scheme == CRT_SCHEME_BL) {
    for (int j = tid; j < nz; j += SIDE_BLOCK) sd[j] = lai[j] * dtau_d_quad(kq, lai[j]);  // always 'quad', _solve_bl.py:35-37
    return;
  }
  if (tid < REC_HDR) {
    double t = 0.0;
    if (tid == S_LT) t = rec[S_LT];
    if (a.scheme == CRT_SCHEME_ZQ) {
      const double dm = rec[S_DLM];
      if (tid == S_DLM) t = dm;
      if (tid == S_TAUI) t = dm * dtau_d_quad(kq, dm);  // always 'quad', _solve_zq.py:51
      if (tid == S_TPSI) t = -(Kb * dm) * rec[S_TPSI];
    }
    sd[tid] = t;
  }
  double* v = sd + REC_HDR;
  const bool n79u = a.scheme == CRT_SCHEME_N79 && rec[S_UNIF] != 0.0 && nz >= 3;  // one (tb, td) serves every layer (k_colpre)
  const double dlu = rec[S_DL];
  for (int j = tid; j < nz; j += SIDE_BLOCK) {
    v[j] = -(Kb * lai[j]) * rec[REC_HDR + j];  // e^{-K_b L_j}: n79's tbcum, zq's beam fraction
    if (a.scheme != CRT_SCHEME_N79) continue;
    double tb = 0.0, td = 0.0;  // the top level carries no layer: 1 - tb = 1 - td = 1
    if (j + 1 < nz) {
      const double D = n79u ? dlu : lai[j] - lai[j + 1];
      tb = (Kb * D) * fexp(-Kb * D);
      td = -D * (a.tau_d_method == CRT_TAU_D_9SKY ? dtau_d_9sky(k9, D) : dtau_d_quad(kq, D));
    }
    v[nz + j] = tb;
    v[2 * nz + j] = td;
  }
}

__global__ __launch_bounds__(256) void k_dtau_d(const double* __restrict__ kb_nodes, const double* __restrict__ L, long long n, int method,
                                                 double* __restrict__ out) {
  __shared__ double kq[NQT];
  __shared__ double k9[CRT_NQ_9SKY];
  for (int q = threadIdx.x; q < NQT; q += blockDim.x) kq[q] = kb_nodes[q];
  if (threadIdx.x < CRT_NQ_9SKY) k9[threadIdx.x] = kb_nodes[NQT + NQG + threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = method == CRT_TAU_D_9SKY ? dtau_d_9sky(k9, L[i]) : dtau_d_quad(kq, L[i]);
}

// ------------------------------------------------------------------------------------------
constexpr int DLAI_BLOCK = 256;

template <class S, bool BL>
__global__ __launch_bounds__(DLAI_BLOCK) void k_dlai(SolveArgs a, LevArgs la, DlaiArgs da, int per) {
  __shared__ double hd[REC_HDR + 2];
  __shared__ double lvL[CRT_MAX_LEVEL_SELECT], lvE[CRT_MAX_LEVEL_SELECT], lvT[CRT_MAX_LEVEL_SELECT];
  const int c = blockIdx.x, nz = a.nz, nb = a.nb, nsel = la.nsel, tid = threadIdx.x;
  const int b = blockIdx.y * per + tid;
  const bool live = tid < per && b < nb;
  stage_record<false, BL>(a.ws + (long long)c * a.reclen, nz, la, BL ? da.side + (long long)c * nz : nullptr, hd, lvL, lvE, lvT);
  if (!live) return;
  const double invmu = hd[S_INVMU];
  const long long o0 = (long long)c * nsel * nb + b;  // row r: + r nb
  pass_record<S, BL, false>(hd, lvL, lvE, lvT, nsel, load_dband(a, c, b, S::SOIL),
                            [&](int r, double dI, Du dn, Du up) { dlai_store(da, o0 + (long long)r * nb, dI, invmu, dn, up); });
}

// LDS: the first nrec doubles of the record | their tangents (side record) | the states of every JAC_TRI_CP-th level [ncp][4][W]
template <class S>
__global__ __launch_bounds__(64) void k_dlai_tri(SolveArgs a, LevArgs la, DlaiArgs da, int W, int nrec, int off_t) {
  extern __shared__ double lds[];
  const int c = blockIdx.x, nz = a.nz, nb = a.nb, nsel = la.nsel, lane = threadIdx.x;
  {
    const double* rec = a.ws + (long long)c * a.reclen;
    const double* sd = da.side + (long long)c * nrec;
    for (int i = lane; i < nrec; i += 64) {
      lds[i] = rec[i];
      lds[off_t + i] = sd[i];
    }
  }
  __syncthreads();
  const int b = blockIdx.y * W + lane;
  if (lane >= W || b >= nb) return;  // (no barrier below)
  double* const cp = lds + 2 * off_t + lane;
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
  const DBand in = load_dband(a, c, b, true);
  const double invmu = lds[S_INVMU];
  const double* const dekl = lds + off_t + REC_HDR;  // (e^{-K_b L_j})': the first vector of both records
  S st;
  st.init(RecV<Du>{lds, lds + off_t}, in, nz);
  const int nst = S::nstates(nz);
  Du e, f;
  st.first(e, f);
  put(0, e, f);
  for (int k = 0; k + 1 < nst; ++k) {
    st.advance(k, e, f);
    if ((k + 1) % JAC_TRI_CP == 0) put((k + 1) / JAC_TRI_CP, e, f);
  }
  st.top(e, f);
  const long long o0 = (long long)c * nsel * nb + b;
  int r = nsel - 1;  // rows are written from the top down
  if constexpr (S::TOP_OUT) {
    if (la.lev[r] == nz - 1) {
      dlai_store(da, o0 + (long long)r * nb, in.I_dr0 * dekl[nz - 1], invmu, st.dn, st.up);
      --r;
    }
  }
  // back substitution as in k_jac_tri: blocks of JAC_TRI_CP levels recomputed from their kept state, consumed from the top down
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
          dlai_store(da, o0 + (long long)r * nb, in.I_dr0 * dekl[k], invmu, dn, up);
          --r;
        }
      }
    }
  }
}

template <class S, bool BL = false>
int launch_dlai_closed(const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe) {
  return launch_deriv_closed(k_dlai<S, BL>, "k_dlai", S::NAME, DLAI_BLOCK, 1, a, la, da, s, probe);
}
template <class S>
int launch_dlai_tri(const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe) {
  return launch_deriv_tri(k_dlai_tri<S>, "k_dlai_tri", S::NAME, S::ID, 2, 1, a, la, da, s, probe);
}

}  // namespace

int launch_dlai(int scheme, const SolveArgs& a, const LevArgs& la, const DlaiArgs& da, hipStream_t s, bool probe) {
  static_assert(DN79::NVEC == 3 && DZq::NVEC == 1, "jac_tri_nrec");
  switch (scheme) {
    case CRT_SCHEME_2S: return launch_dlai_closed<D2s>(a, la, da, s, probe);
    case CRT_SCHEME_BL: return launch_dlai_closed<DBl, true>(a, la, da, s, probe);
    case CRT_SCHEME_G77: return launch_dlai_closed<DG77<false>>(a, la, da, s, probe);
    case CRT_SCHEME_BF: return launch_dlai_closed<DG77<true>>(a, la, da, s, probe);
    case CRT_SCHEME_N79: return launch_dlai_tri<DN79>(a, la, da, s, probe);
    case CRT_SCHEME_ZQ: return launch_dlai_tri<DZq>(a, la, da, s, probe);
    default: return CRT_ERR_UNSUPPORTED;
  }
}

// after K0 on the same stream (the quadrature tables are uploaded by then); 2s, g77, bf have no side record
int launch_dlai_side(const ColArgs& ca, double* side, hipStream_t s) {
  if (dlai_side_len(ca.scheme, ca.nz) == 0) return CRT_OK;
  return launch_kernel(k_dlai_side, dim3(ca.ncol), SIDE_BLOCK, 0, s, ca, side);
}

int launch_dtau_d(const double* kb_nodes, const double* L, long long n, int method, double* out, hipStream_t s) {
  return launch_per_lai(k_dtau_d, n, s, kb_nodes, L, n, method, out);
}

int upload_quad_dlai(const QuadConst& h, hipStream_t s) { return upload_qc(h, s); }

}  // namespace crt
