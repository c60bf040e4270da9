/*
 * crt1d_hip_leafmodel.h -- the generalised plate model of leaf optics (Allen et al. 1969; Stokes' pile of plates; the core of PROSPECT)
 * on the device: a structure parameter N and the contents C_i of nabs absorbers of every column -> leaf_r, leaf_t of every band and their
 * partial derivatives with respect to (N, C_0, ..), written as the per-column directions of a crt_optics_dirs.  It is the leaf model
 * behind the "directions of a leaf model" of crt1d_hip_sensjac.h: a retrieval is k_retrieve_apply (leaf directions NULL) -> k_plate_leaf
 * on the same parameter array -> the tangent refill -> the Jacobian or normal-equation call -> the step, with no host round trip.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol sets of
 * the other headers and CRT_ABI_VERSION stay what they are.  The entry is asynchronous on `stream`, allocates nothing, never synchronises,
 * uses no atomics, finds every argument error before the launch and is capturable into a hipGraph.
 *
 * THE MODEL.  Per band b: the refractive index n, the interface transmittances t_alpha = tav(alpha, n) and t_90 = tav(90 deg, n) (the
 * Fresnel transmittance averaged over a cone, Stern 1964 / Allen 1973: functions of the band alone, computed by the caller) and the
 * specific absorption spectra K_i.  Per column: q = (N, C_0 .. C_{nabs-1}); nm = 1 + nabs.
 *
 *     k     = (C_0 K_0[b] + C_1 K_1[b] + ...) / N      (ascending i), then clamped to [CRT_PLATE_K_MIN, CRT_PLATE_K_MAX] = [1e-6, 100]
 *     tau   = (1 - k) e^-k + k^2 E1(k);                 dtau/dk = 2 k E1(k) - 2 e^-k
 *     talf  = t_alpha;  ralf = 1 - talf;  t12 = t_90;  r12 = 1 - t12;  t21 = t12 / n^2;  r21 = 1 - t21
 *     den   = 1 - r21^2 tau^2
 *     Ta    = talf tau t21 / den;   Ra = ralf + r21 tau Ta         (the top plate, light inside the cone)
 *     t     = t12  tau t21 / den;   r  = r12  + r21 tau t          (an inner plate, isotropic light)
 *     D     = sqrt((1 + r + t)(1 + r - t)(1 - r + t)(1 - r - t))
 *     a     = (1 + r^2 - t^2 + D) / (2 r);   b = (1 - r^2 + t^2 + D) / (2 t)
 *     bN    = exp((N - 1) ln b);   dn = a^2 bN^2 - 1;   Rs = a (bN^2 - 1) / dn;   Ts = bN (a^2 - 1) / dn
 *     leaf_r = Ra + Ta Rs t / (1 - Rs r);   leaf_t = Ta Ts / (1 - Rs r)
 *
 * E1, the exponential integral, has a fixed number of operations: for k < 1 the series -gamma - ln k - sum_{m=1..20} (-k)^m / (m m!), from
 * 1 on e^-k times 96 terms of the continued fraction 1 / (k + 1 - 1 / (k + 3 - 4 / (k + 5 - ..))), evaluated from its tail without a
 * division; a wave evaluates a form only where one of its lanes needs it, and every lane selects by its own k.
 *
 * THE PARTIALS.  d/dk at fixed N and d/dN at fixed k (which enters through bN alone) by forward mode through the lines above; then
 *     d/dC_i = (K_i[b] / N) d/dk,     d/dN (total) = d/dN - (k / N) d/dk        (k: the clamped value).
 * Where k was clamped, the value and the two base partials are those AT the clamp and the chain factors are applied all the same, so that
 * a Levenberg-Marquardt step can still move off the clamp.
 *
 * DOMAIN.  N in [1, 4], which with k <= 100 keeps bN^2 below 1e265; K_i >= 0, C_i >= 0.  The accuracy of the partials is stated for k in
 * [1e-4, 50]; below 1e-4 the same formulas lose accuracy as r + t -> 1 (a removable singularity of Stokes' formulas, D -> 0): about 1e-9 of
 * their scale at k = 1e-6, which is why the floor sits there.  The results are finite for every k >= 0.  Nothing is validated on the
 * device: a NaN in q gives NaN.
 *
 * ORDER.  One lane owns one (column, band); bands run along the lanes, so every load of a spectrum and every store is coalesced, and the
 * column's q is wave-uniform.  Every sum has the fixed order above: a column's outputs are bitwise the same alone or in any batch, with or
 * without the partials, and for any ntan.
 */
#ifndef CRT1D_HIP_LEAFMODEL_H
#define CRT1D_HIP_LEAFMODEL_H

#include "crt1d_hip.h"
#include "crt1d_hip_sensjac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_PLATE_MAX_NABS (CRT_SENSJAC_MAX_NTAN - 1)
#define CRT_PLATE_K_MIN 1e-6
#define CRT_PLATE_K_MAX 100.0

typedef struct crt_plate_leaf_model { /* device pointers */
  int32_t ncol, nb;
  int32_t nabs;          /* 1 .. CRT_PLATE_MAX_NABS */
  const double* kspec;   /* [nabs][nb] specific absorption spectra, shared by all columns */
  const double* t_alpha; /* [nb] tav(alpha, n) */
  const double* t_90;    /* [nb] tav(90 deg, n) */
  const double* n;       /* [nb] refractive index */
} crt_plate_leaf_model;

/*
 * k_plate_leaf, one launch.  q: [ncol][q_stride], of which row c's first nm = 1 + nabs entries (N, C_0, ..) are read -- a retrieval passes
 * its parameter array [ncol][npar] with q_stride = npar.  leaf_r, leaf_t: [ncol][nb].  d_leaf_r, d_leaf_t: both NULL (no partials), or
 * both [ncol][ntan][nb] with nm <= ntan <= CRT_SENSJAC_MAX_NTAN: rows 0 .. nm - 1 of every column receive the partials in the order
 * N, C_0, ..; the rows beyond are not touched.
 * CRT_ERR_BAD_ARG: NULL m; ncol or nb < 1; nabs outside 1..CRT_PLATE_MAX_NABS; a NULL spectrum of the model; NULL q, leaf_r or leaf_t;
 * q_stride < nm; one of d_leaf_r / d_leaf_t NULL and the other not; with them, ntan outside nm..CRT_SENSJAC_MAX_NTAN.
 * CRT_ERR_UNSUPPORTED: nb beyond 65535 * 64.
 */
int crt_hip_plate_leaf_f64(const crt_plate_leaf_model* m, const double* q, int64_t q_stride, double* leaf_r, double* leaf_t, int32_t ntan,
                           double* d_leaf_r, double* d_leaf_t, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LEAFMODEL_H */
