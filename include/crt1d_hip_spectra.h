/*
 * crt1d_hip_spectra.h -- spectral inputs on the device: raw spectra in, the five arrays of `crt_bands` out, in one launch for all columns
 * (crt1d/spectra.py:129-218 `avg_optical_prop`, :366-390 `smear_avg_optical_prop`, :529-573 `smear_si`, :42-68 `l_wl_planck[_integ]`).
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, fp64, status codes), separate header so that the symbol
 * set of crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 * A band [edges[i], edges[i+1]] is cut into nsub[i] = sub_off[i+1] - sub_off[i] equal sub-bins (the caller counts them: the reference's
 * ceil((b1 - b0) / max(min dx, 5e-3)) is evaluated in Python floats, crt1d_amd.spectra.sub_bin_counts), and per band
 *
 *   xe    = linspace(edges[i], edges[i+1], nsub + 1)            arange * step + start, last element forced to the stop
 *   y_sub = _smear_tuv_1(x, y, (xe[s], xe[s+1]))                the arithmetic and order of crt_hip_smear_tuv_f64
 *   w     = (xe[s+1] - xe[s]) * light(s)
 *   out   = (sum_s y_sub w) / (sum_s w)                         both sums in ascending s, by one lane
 *
 * so a result depends on nothing but its own spectrum, band and light: not on ncol, the launch geometry or shared / per-column inputs.
 *
 * `sub_off` is a HOST pointer (nb + 1 int32 prefix sums, sub_off[0] = 0, strictly increasing): it is checked on the host and travels to
 * the kernel inside the kernel arguments, which is what bounds nb by CRT_SPECTRA_MAX_NB.  Nothing is allocated, nothing synchronises.
 */
#ifndef CRT1D_HIP_SPECTRA_H
#define CRT1D_HIP_SPECTRA_H

#include "crt1d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the light that weights a sub-bin */
enum crt_light {
  CRT_LIGHT_UNIFORM = 0, /* 1 */
  CRT_LIGHT_PLANCK = 1,  /* int l_wl_planck(T_K, .) over the sub-bin, CRT_SPECTRA_NGL-point Gauss-Legendre; T_K > 0 */
  CRT_LIGHT_TABLE = 2    /* np.interp(mid-point of the sub-bin, light_x, light_y), clamped outside light_x */
};

#define CRT_SPECTRA_NGL 16          /* Gauss-Legendre points of the Planck integral over one sub-bin */
#define CRT_SPECTRA_MAX_NB 512      /* bands per call (sub_off rides in the kernel arguments) */
#define CRT_SPECTRA_MAX_ITEMS 65536 /* sub_off[nb]: sub-bins of all bands of one spectrum together */
/* One workgroup holds its column's raw spectra and the shared grids in LDS.  In doubles:
 *   nx (1 + nprop) + 3 nxs + 2 nlx + (nprop + 1)(nb + CRT_SPECTRA_BLOCK) + 2 (nb + 1)  <=  CRT_SPECTRA_LDS_BYTES / 8
 * (nprop = 1 / nxs = 0 for crt_hip_avg_optical_prop_f64, nprop = 3 / nlx = 0 for crt_hip_bands_from_spectra_f64); e.g. nx = 2151 with
 * nxs = 2151 and nb = 512 fits.  Anything larger is CRT_ERR_UNSUPPORTED. */
#define CRT_SPECTRA_BLOCK 512
#define CRT_SPECTRA_LDS_BYTES (160 * 1024)

/* host: the Planck rule on the unit interval, x in (0, 1), sum(w) = 1:  int_a^b f = (b - a) sum_i w[i] f(a + (b - a) x[i]), ascending i,
 * f(wl_um) = 2 h c^2 / (wl^5 (exp(h c / (wl k_B T_K)) - 1)), wl = wl_um 1e-6 (CODATA 2018 exact h, c, k_B).  Validated (relative error
 * <= 1e-13 against QUADPACK, tests/test_spectral_prep_cpu.py) for sub-bins no wider than 0.43 of their centre wavelength at
 * T_K >= 3000; the nearest singularity of f is wl = 0, so wider sub-bins converge more slowly. */
int crt_hip_planck_nodes_f64(double* x, double* w);

/* Batched `smear_avg_optical_prop(x, y, edges, light=...)`:  x[nx] (increasing, shared), y[nspec][nx], edges[nb+1] -> out[nspec][nb].
 *   light_kind  crt_light.  TABLE: light_x[nlx] (increasing), light_y[nlight][nlx]; spectrum s uses row s / light_group, or row 0 when
 *               nlight = 1.  The table arguments are ignored for the other kinds (may be NULL / 0).
 *   y_sub       optional [nspec][sub_off[nb]]: the sub-bin averages themselves (NULL: not written).
 * CRT_ERR_BAD_ARG, found before any launch (nothing is written): a NULL required pointer, nx < 2, nspec < 0, nb < 0, sub_off[0] != 0 or
 * sub_off not strictly increasing, an unknown light kind, PLANCK with T_K <= 0 or NaN, TABLE with nlx < 1, nlight < 1, light_group < 1 or
 * fewer rows than (nspec - 1) / light_group + 1 (unless nlight = 1).  nspec = 0 or nb = 0: CRT_OK, nothing written.  Over the limits
 * above: CRT_ERR_UNSUPPORTED, before any launch.  One kernel, asynchronous on `stream`. */
int crt_hip_avg_optical_prop_f64(const double* x, int32_t nx, const double* y, int32_t nspec, const double* edges, int32_t nb,
                                 const int32_t* sub_off, int32_t light_kind, double T_K, const double* light_x, int32_t nlx,
                                 const double* light_y, int32_t nlight, int32_t light_group, double* out, double* y_sub,
                                 crt_stream_t stream);

/* The input side of one `crt_bands` in one launch.
 *   x_opt[nx]; leaf_r, leaf_t, soil_r: raw optics, column c at ptr + c * stride, stride = nx or more, or 0 (one spectrum for all columns)
 *   x_si[nxs]; SI_dr, SI_df: spectral irradiance (W m-2 um-1), the same way with si_*_stride
 *   -> I_dr0, I_df0, leaf_r_out, leaf_t_out, soil_r_out: [ncol][nb] each (col_stride = nb)
 *   I_*0 = smear_tuv(x_si, SI_*, edges) * (edges[i+1] - edges[i])   (`smear_si`);  the optics as in crt_hip_avg_optical_prop_f64, where
 *   with CRT_LIGHT_TABLE the light of column c is its own SI_dr + SI_df on x_si.
 * Errors as above (nxs < 2 and a stride that is neither 0 nor >= the row length are CRT_ERR_BAD_ARG too); ncol = 0 or nb = 0: CRT_OK. */
int crt_hip_bands_from_spectra_f64(const double* x_opt, int32_t nx, const double* leaf_r, int64_t leaf_r_stride, const double* leaf_t,
                                   int64_t leaf_t_stride, const double* soil_r, int64_t soil_r_stride, const double* x_si, int32_t nxs,
                                   const double* SI_dr, int64_t si_dr_stride, const double* SI_df, int64_t si_df_stride, int32_t ncol,
                                   const double* edges, int32_t nb, const int32_t* sub_off, int32_t light_kind, double T_K, double* I_dr0,
                                   double* I_df0, double* leaf_r_out, double* leaf_t_out, double* soil_r_out, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_SPECTRA_H */
