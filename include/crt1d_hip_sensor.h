/*
 * crt1d_hip_sensor.h -- sensor-band outputs: the level spectra of crt_hip_levels_* folded with a set of spectral response functions
 * inside the level kernels, so that only [ncol][nsel][nsens] sums leave the workgroup (13 Sentinel-2 bands out of 2151 model bands: 165
 * times fewer bytes than the spectra, which are never written).
 *
 * An extension of crt1d_hip.h: same library, same conventions (device pointers, status codes), separate header so that the symbol set of
 * crt1d_hip.h and CRT_ABI_VERSION stay what they are.
 *
 *   out.X[c][r][s] = sum over b in [first[s], first[s] + count[s]) of w_s[b - first[s]] * X[c][levels[r]][b]
 *
 * X is the value the level kernel of crt_hip_levels_f64 forms for that row (same scheme objects, same level walk); only bands inside the
 * support of a sensor band are touched.
 *
 * SUMMATION CONTRACT.  The order of the sum is a function of (scheme, nz, nb, nsel, the sensor set) only -- never of ncol, the column index
 * or the launch: a column's result is bitwise the same alone or in any batch, and every series slice [:, t] is bitwise the per-step call at
 * that sun state.  No atomics.  The order: a workgroup owns one column and one slice of `per` consecutive bands (per <= 1024; nb > 1024 is
 * cut into ceil(nb / 1024) balanced slices, and n79 / zq / zq_pa narrow the slices further where their LDS demands it); within a slice,
 * lane l of one wave adds the products of the bands lo + l, lo + l + 64, ... in ascending order (lo = the first band of the support inside
 * the slice), the 64 lane sums are added by a fixed exchange tree, and the slice sums are added in ascending slice order.  Products and
 * sums are separately rounded fp64 operations.  Only the outputs that are not NULL are staged, multiplied and summed; which of them are NULL
 * changes neither the slices nor the order: a call for a subset of the outputs gives the bits of the call for all four.
 */
#ifndef CRT1D_HIP_SENSOR_H
#define CRT1D_HIP_SENSOR_H

#include "crt1d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_MAX_SENSOR_BANDS 64

typedef struct crt_sensor_set {
  int32_t nsens;        /* 1 .. CRT_MAX_SENSOR_BANDS */
  const int32_t* first; /* HOST [nsens]: first model band of the support of sensor band s */
  const int32_t* count; /* HOST [nsens]: >= 1 bands, first + count <= nb; supports may overlap, any order */
  const double* w;      /* DEVICE, packed: the weights of sensor s are w[off[s] .. off[s] + count[s]), off = exclusive prefix sum of count */
} crt_sensor_set;

typedef struct crt_sensor_out {
  double *I_dr, *I_df_d, *I_df_u, *F; /* each [ncol][nsel][nsens] (series: [ncol][nt][nsel][nsens]) or NULL; at least one */
} crt_sensor_out;

/*
 * Workspace: the column records of crt_hip_levels_* (crt_hip_workspace_bytes_nb) at the same offsets -- a workspace filled by that call can
 * be reused here with CRT_FLAG_SKIP_PRECOMPUTE -- and, where the call runs more than one band slice, the partial sums
 * [ncol][nslice][nsel][4][nsens] behind them.  0 for an invalid scheme or a non-positive size.
 */
size_t crt_hip_sensor_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nsel, int32_t nsens);

/*
 * cols, bands, opts, levels, nsel: as crt_hip_levels_f64 / _f32 (levels: HOST array copied by value).  sensors->first / count travel by
 * value in the kernel arguments too: the call stays capturable into a hipGraph.  opts->flags: CRT_FLAG_SKIP_PRECOMPUTE and
 * CRT_FLAG_PRECOMPUTE_ONLY as everywhere.  The _f32 entry widens the float spectra on load; everything after that is the f64 code, and
 * the sums are DOUBLE.  K0 + one level kernel, + one finish kernel where there are several band slices; asynchronous on `stream`.
 *
 * Status, all found before any launch:
 *  - CRT_ERR_BAD_ARG: NULL sensors / first / count / w / out; nsens outside 1..CRT_MAX_SENSOR_BANDS; count < 1, first < 0 or
 *    first + count > nb; all four outputs NULL; everything crt_hip_levels_* rejects.
 *  - CRT_ERR_WORKSPACE: workspace below crt_hip_sensor_workspace_bytes.
 *  - CRT_ERR_UNSUPPORTED: the staging row (4 doubles per lane) does not fit the workgroup's 160 KB of LDS next to what the level kernel
 *    keeps there; nothing is written.  Limits, tighter than those of crt_hip_levels_*: the closed-form schemes need the column record and the
 *    staging row in LDS together (crt_hip_levels_* falls back to the record in HBM there); n79 / zq / zq_pa need one
 *    64-band slice with its checkpoints (zq_pa: and its kept rows) and the staging row to fit.
 */
int crt_hip_sensor_levels_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                              int32_t nsel, const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream);
int crt_hip_sensor_levels_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts, const int32_t* levels,
                              int32_t nsel, const crt_sensor_set* sensors, const crt_sensor_out* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream);

/*
 * Sun-angle series: the product with crt_hip_levels_series_f64 -- same `sun`, the same inputs read and the same ones ignored, K0 shared
 * (once per column, once per (column, t)).  out: [ncol][nt][nsel][nsens]; slice [:, t] is BITWISE what crt_hip_sensor_levels_f64 writes at
 * that sun state.  Workspace: the records of crt_hip_levels_series_workspace_bytes at the same offsets, the partial sums
 * [ncol][nt][nslice][nsel][4][nsens] behind them.  Shape limits: those of crt_hip_levels_series_f64 and of crt_hip_sensor_levels_f64.
 * float64 only.
 */
size_t crt_hip_sensor_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt, int32_t nsel, int32_t nsens);
int crt_hip_sensor_levels_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                     const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_sensor_set* sensors,
                                     const crt_sensor_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_SENSOR_H */
