/*
 * crt1d_hip_sensjac.h -- the Jacobian of the sensor-band sums of crt_hip_sensor_levels_f64 with respect to a parameter vector of every
 * column: ntan directions of a leaf / soil model in (leaf_r, leaf_t, soil_r), ln LAI and a leaf-angle direction.  The three derivatives
 * of crt1d_hip_jac.h, crt1d_hip_dlai.h and crt1d_hip_dleaf.h folded with the spectral responses of crt1d_hip_sensor.h inside one kernel,
 * behind one column precompute: only [ncol][nsel][nsens][npar] sums leave the workgroup, no derivative array is written.  This is what a
 * per-column Gauss-Newton or Levenberg-Marquardt solver consumes: [nobs] x [npar] per column.
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 * PARAMETER AXIS.  npar = ntan + (with_lai != 0) + (tangent != NULL), at least 1: the ntan directions, then ln LAI, then the leaf angle.
 *
 * With X' denoting exactly what crt_hip_levels_jac_f64, crt_hip_levels_dlai_f64 and crt_hip_levels_dleaf_f64 write for the same inputs
 * (the same tangent bits: the kernel instantiates the per-band maths those kernels instantiate, as crt_hip_levels_grad_f64 does),
 *
 *   out.X[c][r][s][k]     = sum_{b in support(s)} w_s[b] * sum_p dX[c][levels[r]][b] / dq_p[c][b] * d_p[c][k][b]    k < ntan
 *   out.X[c][r][s][lai]   = sum_b w_s[b] * dX[c][levels[r]][b] / d ln LAI
 *   out.X[c][r][s][leaf]  = sum_b w_s[b] * dX[c][levels[r]][b] along `tangent`
 *
 * I_dr does not depend on the optics: its direction columns are written as zeros.  bl has no soil and no upward stream: soil_r
 * contributes nothing and its I_df_u array is written as zeros.
 *
 * SCHEMES.  2s, bl, g77, bf -- the closed forms.  n79, zq, 4s and zq_pa are CRT_ERR_UNSUPPORTED before any launch.
 *
 * SUMMATION CONTRACT.  No atomics.  The order of every sum is a function of (scheme, nz, nb, nsel, the sensor set, ntan, which parameter
 * columns exist) only -- never of ncol, the column index, or which of the four outputs are NULL.  A workgroup owns one column and one
 * slice of `per` consecutive bands (per <= 256; halved down to 64 where nsel * max(3 npar, 4) rows of per doubles do not fit the LDS).  A lane
 * is a band: for a direction k it adds the products X'_p * d_p[k][b] in the order p = leaf_r, leaf_t, soil_r (a NULL direction array is
 * left out) into its entry of a staging row.  Then, per (level, sensor band, parameter), lane l of one wave adds the products
 * w_s[b] * row[b] of the bands lo + l, lo + l + 64, ... in ascending order (lo = the first band of the support inside the slice), the 64
 * lane sums are added by a fixed exchange tree, and the slice sums are added in ascending slice order -- the order of
 * crt_hip_sensor_levels_f64.  Products and sums are separately rounded fp64 operations.
 */
#ifndef CRT1D_HIP_SENSJAC_H
#define CRT1D_HIP_SENSJAC_H

#include "crt1d_hip.h"
#include "crt1d_hip_dleaf.h"
#include "crt1d_hip_sensor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_SENSJAC_MAX_NTAN 8

typedef struct crt_optics_dirs { /* ntan directions of a leaf / soil model in (leaf_r, leaf_t, soil_r) */
  int32_t ntan;                  /* 0 .. CRT_SENSJAC_MAX_NTAN */
  int64_t col_stride;            /* 0: the same directions for every column; else ntan * nb */
  const double* leaf_r;          /* each [ncol or 1][ntan][nb] or NULL (= zeros); ntan > 0 needs at least one */
  const double* leaf_t;
  const double* soil_r;
} crt_optics_dirs;

typedef struct crt_sensjac_out {
  double *I_dr, *I_df_d, *I_df_u, *F; /* each [ncol][nsel][nsens][npar] or NULL; at least one */
} crt_sensjac_out;

/*
 * Workspace: the column records of crt_hip_levels_f64 at the offsets of crt_hip_workspace_bytes_nb come FIRST -- a
 * crt_hip_sensor_levels_f64 call can run afterwards on the same workspace with CRT_FLAG_SKIP_PRECOMPUTE and gives the forward sums of the
 * residual without a second column precompute (its own partial sums lie behind the records: the workspace must hold
 * crt_hip_sensor_workspace_bytes too, and the side records below are overwritten where there are several band slices, so run this entry
 * with the precompute again afterwards).  Then the side records of crt_hip_levels_dlai_f64 [ncol][bl: nz | else 0], those of
 * crt_hip_levels_dleaf_f64 [ncol][bl: 16 + nz | else 16], and the slice partial sums [ncol][band slices][nsel][nsens][npar][4].  The same
 * for every subset of the outputs and for every split of npar into directions, LAI and leaf angle.  0 for an invalid scheme, a
 * non-positive size, nsel outside 1..CRT_MAX_LEVEL_SELECT, nsens outside 1..CRT_MAX_SENSOR_BANDS or npar outside
 * 1..CRT_SENSJAC_MAX_NTAN + 2.
 */
size_t crt_hip_sensor_jac_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel, int32_t nsens, int32_t npar);

/*
 * cols, bands, opts, levels, nsel: as crt_hip_levels_f64 (levels: HOST array copied by value; CRT_G_TABLE columns included); sensors: as
 * crt_hip_sensor_levels_f64 (first / count travel by value); dirs: NULL stands for ntan = 0; with_lai: nonzero = the ln LAI column;
 * tangent: NULL = no leaf-angle column.  K0, the side precomputes the requested columns need (k_dlai_side: LAI of bl; k_dleaf_side: leaf
 * angle), k_sens_jac and, with several band slices, k_sens_jac_finish; crt_hip_last_kernel names them.  Asynchronous on `stream`, no
 * allocation, no synchronisation, capturable into a hipGraph after the first call.  opts->flags: CRT_FLAG_PRECOMPUTE_ONLY runs K0 and the
 * side precomputes; CRT_FLAG_SKIP_PRECOMPUTE skips them all, so it is valid only on a workspace that a call of THIS entry has filled with
 * the same tangent and the same parameter columns.
 *
 * Status, all found before any launch, in the order of precedence of crt_hip_levels_grad_f64:
 *  - CRT_ERR_BAD_ARG: NULL sensors / first / count / w, nsens outside 1..CRT_MAX_SENSOR_BANDS, count < 1, first < 0 or first + count > nb;
 *    ntan outside 0..CRT_SENSJAC_MAX_NTAN, ntan > 0 with all three direction pointers NULL, col_stride neither 0 nor ntan * nb; npar == 0;
 *    tangent without dg_table or dg_at_psi; NULL out, all four outputs NULL; everything crt_hip_levels_f64 rejects.
 *  - CRT_ERR_SHAPE: as crt_hip_levels_f64 (nz < 2).
 *  - CRT_ERR_UNSUPPORTED: n79, zq, 4s, zq_pa, whatever the workspace.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_sensor_jac_workspace_bytes.
 *  - CRT_ERR_UNSUPPORTED: the staging rows, nsel * max(3 npar, 4) doubles per lane, do not fit the workgroup's 160 KB of LDS even at a
 *    64-lane slice (nsel * max(3 npar, 4) <= 312 fits); more than 65535 band slices.  Nothing is written.
 */
int crt_hip_sensor_jac_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                           int32_t nsel, const crt_sensor_set* sensors, const crt_optics_dirs* dirs, int with_lai,
                           const crt_leaf_tangent* tangent, const crt_sensjac_out* out, void* workspace, size_t workspace_bytes,
                           crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_SENSJAC_H */
