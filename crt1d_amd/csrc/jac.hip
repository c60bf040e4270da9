// Optical-property Jacobians of the level spectra (include/crt1d_hip_jac.h): d X[levels[r]][b] / d (leaf_r, leaf_t, soil_r)[b] for
// X = I_df_d, I_df_u, F, by forward-mode differentiation.  The per-band maths of the schemes on Du, a value with ONE
// tangent, is in jac_schemes.hpp (shared with the LAI derivative, dlai.hip); the scheme objects of the solve kernels are not touched.
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
//             nz = 304 (n79) / 311 (zq), then 32 and 16 lanes per workgroup (tri_cp_lanes).  One wave per workgroup, every lane in its own LDS column: no
//             barrier after the record is staged.  The reference's quirks are kept: n79's first downward row uses layer
//             index 1, zq one dlai_mean for every layer.
#include "deriv_passes.hpp"
#include "launch_forms.hpp"

namespace crt {
namespace {

// the scheme objects of jac_schemes.hpp with the optics as Du and the column record as plain doubles
using JBand = JBandT<Du>;
struct J2s : Sch2s::J {};
struct JBl : SchBl::J {};
template <bool BF>
struct JG77 : SchG77<BF>::J {};
struct JN79 : JN79T<Du, double> {};

// the spectra of one (column, band), the three parameters seeded for parameter p (uniform)
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
  stage_record<false, false>(a.ws + (long long)c * a.reclen, nz, la, nullptr, hd, lvL, lvE, nullptr);
  if (!live) return;
  pass_optics<S>(hd, lvL, lvE, nsel, load_jband(a, c, b, p, S::SOIL),
                 [&](int r, Du dn, Du up) { jac_store(jo, o0 + (long long)r * CRT_JAC_NPARAM * nb, dn, up); });
}

// ------------------------------------------------------------------------------------------
// tridiagonal schemes (JN79: jac_schemes.hpp).  State of level k: (e_k, f_k) with up_k = f_k - e_k dn_k.

// JZq keeps its own copy of JZqT<Du, double>: instantiated from the template, k_jac_tri<JZq> came out with other register names and one
// commuted v_add_f64 (the same bits, not the same code); the kernels of this file are held to the code they had (tools/device_code_diff.py).
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

  __device__ inline void init(RecV<double> rec_, const JBand& in, int nz_) {
    rec = rec_.v;
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
  st.init(RecV<double>{lds}, load_jband(a, c, b, p, true), nz);
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
  return launch_deriv_closed(k_jac<S>, "k_jac", S::NAME, JAC_BLOCK, CRT_JAC_NPARAM, a, la, jo, s, probe);
}
template <class S>
int launch_jac_tri(const SolveArgs& a, const LevArgs& la, const JacArgs& jo, hipStream_t s, bool probe) {
  return launch_deriv_tri(k_jac_tri<S>, "k_jac_tri", S::NAME, S::ID, 1, CRT_JAC_NPARAM, a, la, jo, s, probe);
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
