/*
 * crt1d_hip_leaf.h -- leaf-inclination PDFs g(theta_l) on the device: the G(psi) table, G at the caller's angles and the mean leaf angle
 * of every column in one launch (crt1d/leaf_angle.py:31-87: `g_spherical`, `g_uniform`, `g_planophile`, `g_erectophile`,
 * `g_plagiophile`, `g_ellipsoidal`, `mla_from_g`).  The outputs have the layout `crt_columns` (g_table, g_at_psi, mla) and
 * `crt_sun_series` (g_at_psi) take: a column described by its PDF runs as a CRT_G_TABLE column, no solve kernel knows about PDFs.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, fp64, status codes), separate header so that the symbol
 * set of crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 *   G(psi) = int_0^{pi/2} g(theta) A(psi, theta) dtheta,
 *   A      = cos(theta) cos(psi) (1 - 2 beta / pi) + (2 / pi) sin(theta) sin(psi) sin(beta),   beta = acos(min(1, cot(theta) cot(psi)))
 *
 * (Warren Wilson's projection of a leaf inclined by theta, azimuth uniform; beta = 0 where theta + psi <= pi/2).  A has a 3/2-power kink
 * at theta_k = pi/2 - psi, so [0, theta_k] and [theta_k, pi/2] are integrated separately, each with the CRT_LEAF_NGL-point Gauss-Legendre
 * rule; the upper panel in s, theta = theta_k + psi s^2, which makes its integrand smooth.
 */
#ifndef CRT1D_HIP_LEAF_H
#define CRT1D_HIP_LEAF_H

#include "crt1d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* leaf-inclination PDFs g(theta), theta = leaf inclination from the horizontal, on [0, pi/2] */
enum crt_leaf_pdf {
  CRT_LEAF_PDF_SPHERICAL = 0,   /* sin(theta)                                                     no parameter     :31-35 */
  CRT_LEAF_PDF_ELLIPSOIDAL = 1, /* 2 x^3 sin / (l (cos^2 + x^2 sin^2)^2), all three branches of l param[0] = x      :60-79 */
  CRT_LEAF_PDF_TRIG = 2         /* (2/pi)(1 + a cos(2 theta) + b cos(4 theta))                    param = (a, b)   :38-57 */
};                              /* TRIG: uniform (0, 0), planophile (1, 0), erectophile (-1, 0), plagiophile (0, -1) */

/* Ellipsoidal x the fixed rule is validated for: |G - G_exact| <= 1e-11 holds for CRT_LEAF_X_MIN <= x <= CRT_LEAF_X_MAX (worst 1.7e-14 at
 * 0.2, 4.7e-14 at 10).  Outside, the poles of the PDF at theta = pi/2 +- i atanh(x) (x < 1), +- i atanh(1/x) (x > 1) come too close to the
 * panels (7e-10 at x = 0.1 and at x = 20), so such a column is CRT_ERR_BAD_ARG instead of a silently worse table. */
#define CRT_LEAF_X_MIN 0.2
#define CRT_LEAF_X_MAX 10.0

#define CRT_LEAF_NGL 48  /* Gauss-Legendre points of each of the two panels of G(psi) */
#define CRT_LEAF_NMLA 64 /* Gauss-Legendre points of the one panel of mla = deg(int theta g dtheta) */

/* host: the two rules on the unit interval, x in (0, 1), sum(w) = 1.  G: lower panel theta = theta_k x, weight theta_k w; upper panel
 * theta = theta_k + psi x^2, weight 2 psi x w.  mla: theta = (pi/2) x_mla, weight (pi/2) w_mla.  Either pair may be NULL. */
int crt_hip_leaf_pdf_nodes_f64(double* x, double* w, double* x_mla, double* w_mla);

/* pdf_kind[ncol] (crt_leaf_pdf), pdf_param[ncol][2], psi[ncol][npsi] (radians, 0 <= psi <= pi/2; NULL when npsi = 0) ->
 *   g_table[ncol][CRT_NQ]  G at the angles of crt_hip_quad_nodes(mu_s)
 *   g_at_psi[ncol][npsi]   G at the caller's angles (may be NULL: not computed)
 *   mla[ncol]              mean leaf inclination, degrees (may be NULL: not computed)
 * One kernel, asynchronous on `stream` -- after the descriptors have been validated: pdf_kind / pdf_param are read back to the host
 * (20 bytes per column; this synchronises `stream` once, so the call cannot be captured into a graph) and an unknown kind, x outside
 * [CRT_LEAF_X_MIN, CRT_LEAF_X_MAX] (x <= 0 and NaN included) or a TRIG pair whose PDF is negative somewhere in [0, pi/2] is CRT_ERR_BAD_ARG, like a NULL required pointer, ncol < 0,
 * npsi < 0 or mu_s outside (0, 1): found before the launch, nothing is written.  ncol = 0 is CRT_OK and does nothing. */
int crt_hip_g_from_pdf_f64(const int32_t* pdf_kind, const double* pdf_param, int32_t ncol, double mu_s, const double* psi, int32_t npsi,
                           double* g_table, double* g_at_psi, double* mla, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_LEAF_H */
