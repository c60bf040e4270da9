/*
 * crt1d_hip.h -- C ABI of the MI355X (gfx950) batched 1-D canopy radiative-transfer path.
 *
 * One call = one scheme over a batch of (column x band) solves.  The entry points replace,
 * for the batched case, the reference's keyword-only plugin functions
 *
 *   solve_2s   crt1d/solvers/_solve_2s.py:11-163     ->  crt_hip_2s_f64
 *   solve_4s   crt1d/solvers/_solve_4s.py:8-293      ->  crt_hip_4s_f64
 *   solve_n79  crt1d/solvers/_solve_n79.py:11-164    ->  crt_hip_n79_f64
 *   solve_zq   crt1d/solvers/_solve_zq.py:13-229     ->  crt_hip_zq_f64
 *   solve_bl   crt1d/solvers/_solve_bl.py:9-93       ->  crt_hip_bl_f64
 *   solve_g77  crt1d/solvers/_solve_g77.py:7-135     ->  crt_hip_g77_f64
 *   solve_bf   crt1d/solvers/_solve_bf.py:7-154      ->  crt_hip_bf_f64
 *   solve_zq_pa crt1d/solvers/_solve_zq_pa.py:24-418 ->  crt_hip_zq_pa_f64
 *
 * which `Model.run` dispatches to at crt1d/model.py:305-310.  Every scheme also has an f32 storage entry (crt_hip_<scheme>_f32),
 * and f32 storage reaches the epilogue (crt_hip_absorb_f32, crt_hip_absorb_bandsum{,2}_f32) and the fused integrated path
 * (crt_hip_integrated{,2}_f32): float spectra and profiles, fp64 arithmetic and band sums.  The reference has no FFI of
 * its own (pure Python); INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - plain pointers + sizes; all data pointers are DEVICE pointers (HBM), fp64, caller-owned.
 *    Nothing is allocated or freed by the library; launches are asynchronous on `stream`.
 *  - `lai` is cumulative leaf-area index from the canopy top: index 0 = ground (total LAI),
 *    index nz-1 = canopy top (0), strictly as crt1d/variables.yml:73-86 / model.py:244-246.
 *  - per-(column, band) inputs: element (c, b) at p[c * col_stride + b]; col_stride = 0
 *    broadcasts one spectrum over all columns.
 *  - outputs are [ncol][nz or nz-1][nb], bands contiguous (the reference's (nz, nb) C-order
 *    arrays, stacked over columns).
 *  - return value: 0 on success, negative crt_status otherwise (the Python wrapper maps these
 *    to the reference's exception types: AssertionError / ValueError).
 *  - thread-safety: re-entrant -- no mutable process-global state on the solve path (kernel-selection overrides travel in
 *    crt_options.tune; the quadrature tables are uploaded once per device under a lock); concurrent calls must use distinct
 *    streams + workspaces.  The buffer allocator (crt_hip_buffer_*) serialises on one mutex.
 */
#ifndef CRT1D_HIP_H
#define CRT1D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_ABI_VERSION 3

/* leaf-angle G(psi) kinds: crt1d/leaf_angle.py:118-202 */
enum crt_g_kind {
  CRT_G_HORIZONTAL = 0,              /* cos(psi)                       :118-120 */
  CRT_G_SPHERICAL = 1,               /* 0.5                            :123-125 */
  CRT_G_VERTICAL = 2,                /* 2/pi sin(psi)                  :128-130 */
  CRT_G_ELLIPSOIDAL = 3,             /* Campbell 1986, param = x       :133-165 */
  CRT_G_ELLIPSOIDAL_APPROX = 4,      /* Campbell 1990, param = x       :168-180 */
  CRT_G_ELLIPSOIDAL_APPROX_BONAN = 5,/* Ross-Goudriaan, param = chi_l  :183-202 */
  CRT_G_TABLE = 6                    /* caller-sampled callable (K_b_fn / G_fn of the plugin API) */
};

/* fixed quadrature nodes at which a CRT_G_TABLE column supplies G(psi) */
#define CRT_NQ_TAU 96  /* graded composite Gauss-Legendre on [0, pi/2]: tau_d (common.py:30-37), mu_bar (_solve_2s.py:32) */
#define CRT_NQ_G4 32   /* 2 x 16 Gauss-Legendre in psi for G_int_1/2 (_solve_4s.py:148-149); depend on mu_s */
#define CRT_NQ_9SKY 9  /* 5,15,...,85 deg (common.py:46) */
#define CRT_NQ (CRT_NQ_TAU + CRT_NQ_G4 + CRT_NQ_9SKY)

enum crt_scheme {
  CRT_SCHEME_2S = 0, CRT_SCHEME_4S = 1, CRT_SCHEME_N79 = 2, CRT_SCHEME_ZQ = 3,
  CRT_SCHEME_BL = 4, CRT_SCHEME_G77 = 5, CRT_SCHEME_BF = 6, CRT_SCHEME_ZQ_PA = 7, CRT_NUM_SCHEMES = 8
};

enum crt_tau_d_method { CRT_TAU_D_QUAD = 0, CRT_TAU_D_9SKY = 1 }; /* _solve_n79.py:19, common.py:72-78 */

enum crt_status {
  CRT_OK = 0,
  CRT_ERR_BAD_ARG = -1,      /* null pointer, non-positive size, bad enum  -> ValueError      */
  CRT_ERR_WORKSPACE = -2,    /* workspace smaller than crt_hip_workspace_bytes()              */
  CRT_ERR_UNSUPPORTED = -3,  /* shape outside what the kernels handle (e.g. nz too large for LDS) */
  CRT_ERR_LAUNCH = -4,       /* HIP launch / runtime error                                    */
  CRT_ERR_SHAPE = -5         /* shape violates a reference assertion (e.g. nz < 3 for n79) -> AssertionError */
};

typedef void* crt_stream_t; /* hipStream_t */

/* per-column canopy geometry (what one reference `Model` instance holds; model.py:68-116) */
typedef struct crt_columns {
  int32_t ncol;
  int32_t nz;             /* interface levels ("nlayers" of the reference) */
  const double* psi;      /* [ncol] solar zenith angle, radians */
  const double* lai;      /* [ncol][nz] cumulative LAI, index 0 = ground */
  const double* mla;      /* [ncol] mean leaf angle, degrees; 2s only (may be NULL otherwise) */
  const int32_t* g_kind;  /* [ncol] crt_g_kind */
  const double* g_param;  /* [ncol] x or chi_l (ignored for parameter-free kinds) */
  const double* g_at_psi; /* [ncol] G(psi[c]); read only for CRT_G_TABLE columns (may be NULL otherwise) */
  const double* g_table;  /* [ncol][CRT_NQ] G at crt_hip_quad_nodes(); CRT_G_TABLE columns only (may be NULL) */
} crt_columns;

/* per-(column, band) spectra: the (n_wl,) plugin inputs I_dr0_all, I_df0_all, leaf_r, leaf_t, soil_r */
typedef struct crt_bands {
  int32_t nb;
  int64_t col_stride;     /* nb (or larger) for per-column spectra, 0 = same spectrum for every column */
  const double* I_dr0;
  const double* I_df0;
  const double* leaf_r;
  const double* leaf_t;
  const double* soil_r;   /* not read by bl */
} crt_bands;

/* crt_options.flags */
#define CRT_FLAG_SKIP_PRECOMPUTE 1 /* workspace already holds the column records of an earlier call with the
                                      same scheme/columns/options (only the spectra changed): skip kernel K0 */
#define CRT_FLAG_PRECOMPUTE_ONLY 2 /* run K0 only (fills the workspace), no solve kernel */
#define CRT_FLAG_DIRECT_STORES 4   /* measurement aid: use the direct-store solve kernel even where the LDS-tiled,
                                      line-aligned one applies (same results, different store pattern) */

/* crt_options.tune: keys.  Every value is 0 = automatic (the launcher's own heuristic); any other value outside the range given
 * here is CRT_ERR_BAD_ARG, checked before any launch.  "Closed forms" are 2s, 4s, bl, g77 and bf; the tridiagonal schemes are n79
 * and zq; zq_pa has launchers of its own and hands the same overrides to the grid solve of its two-kernel path.  Keys 7 and 14 are
 * reserved and must stay 0. */
enum crt_tune_key {
  CRT_TUNE_TILE_LDS = 0,           /* closed forms: LDS bytes a tile may take per workgroup, <= 160 KiB */
  CRT_TUNE_TILE_T = 1,             /* closed forms: levels per k_tile tile, <= 64 */
  CRT_TUNE_TILE_FLAGS = 2,         /* bit set of crt_tune_tile_flag, <= 255 */
  CRT_TUNE_CLOSED_STORE_WAVES = 3, /* closed forms: store waves of k_pipe / k_pipe_pack, <= 12 */
  CRT_TUNE_CLOSED_PIPE_T = 4,      /* closed forms: levels per k_pipe / k_pipe_pack tile, <= 32 */
  CRT_TUNE_PACK = 5,               /* several columns per compute wave (k_pipe_pack, packed k_tri_pipe): crt_tune_pack */
  CRT_TUNE_PACK_COMPUTE_WAVES = 6, /* compute waves of one pack, <= 4 */
  CRT_TUNE_TRI_M = 8,              /* tridiagonal and zq_pa: rows per segment M, 8 / 12 / 16 */
  CRT_TUNE_TRI_T = 9,              /* tridiagonal: levels per tile T, 4 / 8 / 12; read only with CRT_TUNE_TRI_M (0 there: 4) */
  CRT_TUNE_TRI_FAMILY = 10,        /* tridiagonal and zq_pa: kernel family, crt_tune_tri_family */
  CRT_TUNE_TRI_STORE_WAVES = 11,   /* tridiagonal and zq_pa: store waves of the pipelines, <= 12 */
  CRT_TUNE_MIN_TILE_NB = 12,       /* smallest nb that takes the tile / pipeline kernels, <= 1024 (0: 4 for the closed forms, 10 for
                                      the tridiagonal schemes, 16 for zq_pa's single-kernel forms, 1 for its grid solve) */
  CRT_TUNE_FLAT_FLUSH = 13,        /* flat flush of rows that are not pair-aligned (odd nb): crt_tune_flat_flush */
  CRT_TUNE_K0_SEPARATE = 15        /* 2s: 1 = k_colpre in front of k_pipe instead of the record prologue inside it */
};
#define CRT_NTUNE 16

/* CRT_TUNE_TILE_FLAGS bits */
enum crt_tune_tile_flag {
  CRT_TILE_FLAG_SYNC_BARRIERS = 1,       /* k_tile: full __syncthreads() barriers */
  CRT_TILE_FLAG_GENERIC_FLUSH = 2,       /* closed forms: generic flush instead of the fused one */
  CRT_TILE_FLAG_NO_PIPELINE = 4,         /* closed forms: no k_pipe (k_tile instead) */
  CRT_TILE_FLAG_NO_GENERIC_PIPELINE = 8, /* closed forms: no generic-flush k_pipe */
  CRT_TILE_FLAG_FOUR_PAIR_STORE = 16     /* tridiagonal, narrow spectra: the four-pair instead of the two-pair register-staged store role */
};

/* CRT_TUNE_PACK values */
enum crt_tune_pack {
  CRT_PACK_OFF = 1,  /* one column per workgroup */
  CRT_PACK_FORCE = 2 /* closed forms: pack also above 32 bands (up to 128) */
};

/* CRT_TUNE_TRI_FAMILY values (any of them, like CRT_TUNE_TRI_M, also keeps n79 and zq from packing columns).  1 reads as NO_PIPELINE
 * for n79 and zq and as ZQPA_TWO_KERNEL for zq_pa, whose grid solve then reads it as NO_PIPELINE. */
enum crt_tune_tri_family {
  CRT_TRI_FAMILY_NO_PIPELINE = 1,      /* k_tri_tile */
  CRT_TRI_FAMILY_DOUBLE_BUFFERED = 2,  /* double-buffered k_tri_pipe only */
  CRT_TRI_FAMILY_REG_STAGED = 3,       /* register-staged k_tri_pipe only */
  CRT_TRI_FAMILY_GENERIC_PIPELINE = 4, /* generic-flush k_tri_pipe wherever the fused flush does not apply, for any nb */
  CRT_TRI_FAMILY_ZQPA_TWO_KERNEL = 1,  /* zq_pa: grid solve into workspace scratch + k_zqpa_interp (f64 only) */
  CRT_TRI_FAMILY_ZQPA_PIPE = 5,        /* zq_pa: k_zqpa_pipe (interpolation in the store waves) */
  CRT_TRI_FAMILY_ZQPA_PIPE2_DB = 6,    /* zq_pa: double-buffered k_zqpa_pipe2 (interpolation in the compute lanes) */
  CRT_TRI_FAMILY_ZQPA_PIPE2_RS = 7     /* zq_pa: register-staged k_zqpa_pipe2 */
};

/* CRT_TUNE_FLAT_FLUSH values (0: whole lines for zq and zq_pa, part lines for n79) */
enum crt_tune_flat_flush {
  CRT_FLAT_FLUSH_OFF = 1,       /* per-array generic flush instead */
  CRT_FLAT_FLUSH_PART_LINE = 2,
  CRT_FLAT_FLUSH_WHOLE_LINE = 3
};

typedef struct crt_options {
  double mu_s;            /* 4s: cosine of the dividing angle, default 0.501 (_solve_4s.py:9) */
  int32_t tau_d_method;   /* n79: crt_tau_d_method, default CRT_TAU_D_QUAD (_solve_n79.py:19) */
  int32_t flags;          /* CRT_FLAG_* */
  int32_t tune[CRT_NTUNE];/* measurement aid, all zero in production: per-CALL overrides of the kernel-selection heuristics,
                             indexed by crt_tune_key.  Part of the call's arguments, so there is no process-global tuning state:
                             calls with different settings may run concurrently */
} crt_options;

/* outputs; each [ncol][nz][nb] unless noted.  Unused slots may be NULL. */
typedef struct crt_outputs {
  double* I_dr;
  double* I_df_d;
  double* I_df_u;
  double* F;
  double* x0; /* n79: aI_lsl [ncol][nz-1][nb] | zq: I_df_d_ss | g77, bf: aI_lsl */
  double* x1; /* n79: aI_lsh [ncol][nz-1][nb] | zq: I_df_u_ss | g77, bf: aI_lsh */
  double* x2; /*                                zq: F_ss      | g77, bf: aI_l   */
} crt_outputs;

/* f32 storage variants: spectra read and profiles written as float (half the HBM bytes).  Geometry (crt_columns), the
 * workspace and ALL arithmetic stay fp64: results are the fp64 results rounded once to fp32.  They reach every step after the
 * solve as well: the epilogue (crt_hip_absorb_f32, crt_hip_absorb_bandsum{,2}_f32) and the fused integrated path
 * (crt_hip_integrated{,2}_f32), whose band sums and other reduced outputs stay fp64. */
typedef struct crt_bands_f32 {
  int32_t nb;
  int64_t col_stride;
  const float* I_dr0;
  const float* I_df0;
  const float* leaf_r;
  const float* leaf_t;
  const float* soil_r;
} crt_bands_f32;

typedef struct crt_outputs_f32 {
  float* I_dr;
  float* I_df_d;
  float* I_df_u;
  float* F;
  float* x0;
  float* x1;
  float* x2;
} crt_outputs_f32;

int crt_hip_abi_version(void);
const char* crt_hip_strerror(int status);

/* bytes of device workspace a solve of `scheme` needs for (ncol, nz) */
size_t crt_hip_workspace_bytes(int scheme, int32_t ncol, int32_t nz);

/* same, for schemes whose workspace also depends on the number of bands (zq_pa keeps its computational-grid fluxes
 * there: 2 * ncol * min(100, nz) * nb doubles); equals crt_hip_workspace_bytes for every other scheme */
size_t crt_hip_workspace_bytes_nb(int scheme, int32_t ncol, int32_t nz, int32_t nb);

/* host: fill psi_nodes[CRT_NQ] with the zenith angles (radians) at which g_table is sampled */
int crt_hip_quad_nodes(double mu_s, double* psi_nodes);

/* generic entry (scheme = crt_scheme) and the per-scheme entry points */
int crt_hip_solve_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                      const crt_outputs* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);
int crt_hip_2s_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_4s_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_n79_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_zq_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_bl_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_g77_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_bf_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);
int crt_hip_zq_pa_f64(const crt_columns*, const crt_bands*, const crt_options*, const crt_outputs*, void*, size_t, crt_stream_t);

int crt_hip_solve_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts,
                      const crt_outputs_f32* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);
int crt_hip_2s_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
int crt_hip_4s_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
int crt_hip_n79_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
int crt_hip_zq_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
int crt_hip_bl_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
int crt_hip_g77_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
int crt_hip_bf_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);
/* zq_pa with f32 storage runs in the single-kernel form only: nb >= 16 (even or odd: the reference's default 107 bands are covered)
 * and as many bands as its LDS holds -- 832 at a dozen levels, about 600 from 60 levels up -- else CRT_ERR_UNSUPPORTED.  Its four output arrays must start on an 8-byte boundary (a float array may not start at an
 * odd element of an aligned allocation), else CRT_ERR_UNSUPPORTED: every form stores band pairs, and there is no two-kernel
 * fallback in f32.  The f64 entry accepts any 8-byte aligned outputs (misaligned ones take the two-kernel path). */
int crt_hip_zq_pa_f32(const crt_columns*, const crt_bands_f32*, const crt_options*, const crt_outputs_f32*, void*, size_t, crt_stream_t);

/*
 * Epilogue (model.py:573-647 `_calc_absorption` + diagnostics.py:39-108 `band`): layer absorption
 * from the three irradiance profiles, reduced over bands with `ngroup` weight vectors
 * (spectra.py:71-126 `_x_frac_in_bounds`).  Outputs, each [ncol][nz-1][ngroup]:
 *   aI (total), aI_sl (sunlit), aI_sh (shaded); and totals [ncol][ngroup][4]:
 *   incoming I_d[top], reflected I_df_u[top], transmitted I_d[ground], soil-reflected I_df_u[ground]
 *   (the terms of diagnostics.py:476-530 `compare_ebal`).  band_w is [ngroup][nb].
 */
int crt_hip_absorb_bandsum_f64(const crt_columns* cols, const crt_bands* bands, const double* I_dr, const double* I_df_d,
                               const double* I_df_u, const double* band_w, int32_t ngroup, double* aI, double* aI_sl,
                               double* aI_sh, double* totals, crt_stream_t stream);
/* f32 storage: bands->leaf_r / leaf_t and the three profiles I_dr, I_df_d, I_df_u are float; band_w and every output stay double.
 * Loads widen to double at once and the kernel choice depends on the shape only, so the outputs are the bits
 * crt_hip_absorb_bandsum_f64 gives for the same values upcast. */
int crt_hip_absorb_bandsum_f32(const crt_columns* cols, const crt_bands_f32* bands, const float* I_dr, const float* I_df_d,
                               const float* I_df_u, const double* band_w, int32_t ngroup, double* aI, double* aI_sl,
                               double* aI_sh, double* totals, crt_stream_t stream);

/*
 * The complete output of diagnostics.band (crt1d/diagnostics.py:39-108) for up to four band groups at once: besides the layer
 * absorption sums above, the band-integrated LEVEL profiles of every irradiance variable band() reduces (:84-91; the variables of
 * Model.to_xr, model.py:421-426): I_dr, I_df_d, I_df_u, F and I_d = I_dr + I_df_d, each [ncol][nz][ngroup]
 *     X_g(z) = sum_b band_w[g][b] X(z, b)                                            (diagnostics.py:81)
 * and aI_dr [ncol][nz-1][ngroup], the direct-beam part of the absorbed irradiance, from which the remaining entries of the
 * reference's absorption dict follow exactly: aI_df = aI - aI_dr, aI_df_sl = aI_sl - aI_dr, aI_df_sh = aI_sh (model.py:628-634).
 * calc_PFD=True (:92-104, _E_to_PFD_da :19-36) is a choice of WEIGHTS: band_w[g][b] / e_wl_umol(wl[b]) gives the photon-flux variants.
 * The six optional pointers are given all together or all NULL (then this is crt_hip_absorb_bandsum_f64); totals may be NULL.
 */
typedef struct crt_bandsum_out {
  double* aI;      /* [ncol][nz-1][ngroup] */
  double* aI_sl;
  double* aI_sh;
  double* totals;  /* [ncol][ngroup][4] or NULL */
  double* aI_dr;   /* [ncol][nz-1][ngroup] or NULL */
  double* I_dr;    /* [ncol][nz][ngroup] or NULL */
  double* I_df_d;
  double* I_df_u;
  double* F;
  double* I_d;
} crt_bandsum_out;
int crt_hip_absorb_bandsum2_f64(const crt_columns* cols, const crt_bands* bands, const double* I_dr, const double* I_df_d,
                                const double* I_df_u, const double* band_w, int32_t ngroup, const crt_bandsum_out* out, crt_stream_t stream);
/* f32 storage: float leaf optics and profiles, double band_w and crt_bandsum_out (bitwise equal to the f64 call on upcast values) */
int crt_hip_absorb_bandsum2_f32(const crt_columns* cols, const crt_bands_f32* bands, const float* I_dr, const float* I_df_d,
                                const float* I_df_u, const double* band_w, int32_t ngroup, const crt_bandsum_out* out, crt_stream_t stream);
/* ... and the same complete output from the fused solve + epilogue (crt_hip_integrated_f64): no profile is written to memory, the
 * level sums the kernel forms anyway are kept instead of thrown away. */
int crt_hip_integrated2_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const double* band_w,
                            int32_t ngroup, const crt_bandsum_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);
/* f32 storage: the five spectra of crt_bands_f32 are float; band_w, the workspace and crt_bandsum_out stay double.  All eight schemes,
 * nb <= 1024 (else CRT_ERR_UNSUPPORTED); crt_hip_last_kernel names the float instantiation with an " f32" tag. */
int crt_hip_integrated2_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts, const double* band_w,
                            int32_t ngroup, const crt_bandsum_out* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);
/*
 * Sun-angle series: the complete output of crt_hip_integrated2_f64 for `nt` sun states of every column in ONE call -- the same canopy
 * (lai, leaf angle, leaf and soil optics) under many sun positions psi and incoming spectra I_dr0, I_df0: what the reference does with
 * `update_p(psi=...)` + `run()` in a loop over a day or a season (model.py:118-176, 295-331).
 *
 *  - cols->psi, cols->g_at_psi, bands->I_dr0, bands->I_df0 are NOT read and may be NULL; everything else in crt_columns / crt_bands
 *    (leaf_r, leaf_t, soil_r and their own col_stride) keeps its meaning and is constant over the series.
 *  - every array of crt_bandsum_out gains a time axis after the column axis: aI, aI_sl, aI_sh, aI_dr [ncol][nt][nz-1][ngroup];
 *    I_dr, I_df_d, I_df_u, F, I_d [ncol][nt][nz][ngroup]; totals [ncol][nt][ngroup][4].  Optional pointers as crt_hip_integrated2_f64.
 *  - CONTRACT: for every t, slice [:, t] of every output is BITWISE what crt_hip_integrated2_f64 writes for the same columns with
 *    psi = sun.psi[:, t], g_at_psi = sun.g_at_psi[:, t], I_dr0 = sun.I_dr0[:, t], I_df0 = sun.I_df0[:, t].  All eight schemes, nb <= 1024
 *    (beyond: CRT_ERR_UNSUPPORTED, nothing written).  The series kernels run the per-step kernels' bodies on the same records and pick
 *    between their forms (zq_pa: net-flux or separate sums, M = 8 / 12) by the same rule, which depends on nz, nb and the requested
 *    outputs only.
 *  - what is shared: the column precompute (K0), and nothing else.  Per column, once per call (k_colpre<canopy>): the K_b node table,
 *    every tau_d / 1 - tau_d quadrature, mu_bar, G_int_1/2, the dLAI analysis, zq_pa's grid and interpolation record.  Per (column, t)
 *    (k_colsun): K_b, cos psi, G, tau_psi and the vectors built from exp(-K_b lai).  The workspace holds [ncol] canopy records and
 *    [ncol][nt] sun records.  The solve side shares nothing between sun states: one workgroup per (column, t) assembles its record from
 *    the two and runs the per-step kernel's body; leaf_r, leaf_t, soil_r are read again for every state (a kernel that walked the
 *    states of a column with the optics in registers was measured slower than the per-step loop and dropped).
 *  - CRT_FLAG_PRECOMPUTE_ONLY fills the workspace (both kinds of record) and launches no solve; CRT_FLAG_SKIP_PRECOMPUTE: the workspace
 *    holds the records of an earlier series call with the same scheme, columns, options and sun.psi (only the spectra changed).
 *  - CRT_ERR_BAD_ARG before any launch: NULL sun, sun->psi, I_dr0 or I_df0; nt < 1; col_stride neither 0 nor >= nt * nb; g_at_psi NULL
 *    while cols->g_table is given; everything crt_hip_integrated2_f64 rejects.  CRT_ERR_WORKSPACE below crt_hip_series_workspace_bytes
 *    (which is 0 for sizes it cannot express).  Any nt: t is spread over two grid dimensions (65535 x 65535 states per column); ncol * nt < 2^31.
 *  - capturable into a hipGraph after the first call per device; crt_hip_last_kernel names the K0 forms and the series kernel.
 */
typedef struct crt_sun_series {
  int32_t nt;               /* sun states per column, >= 1 */
  const double* psi;        /* [ncol][nt] solar zenith angle, radians */
  const double* g_at_psi;   /* [ncol][nt] G(psi[c][t]); read for CRT_G_TABLE columns only (else may be NULL) */
  int64_t col_stride;       /* of I_dr0 / I_df0: nt*nb (or larger) per column, 0 = one series for every column */
  const double* I_dr0;      /* element (c, t, b) at p[c*col_stride + t*nb + b] */
  const double* I_df0;
} crt_sun_series;

size_t crt_hip_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nb, int32_t nt);
int crt_hip_integrated_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun,
                                  const crt_options* opts, const double* band_w, int32_t ngroup, const crt_bandsum_out* out,
                                  void* workspace, size_t workspace_bytes, crt_stream_t stream);
/* The outputs of crt_bandsum_out that follow from the others, re-formed in place in one pass (after the band sums of partial spectra
 * have been added up, e.g. by an all-reduce that carried only aI_sl, aI_sh and the level sums I_dr, I_df_d, I_df_u):
 *     aI = aI_sl + aI_sh,   F = I_dr / cos(psi) + 2 (I_df_u + I_df_d),   I_d = I_dr + I_df_d
 * F and I_d are bitwise what crt_hip_absorb_bandsum2_* (nb <= 1024; wider spectra add F in pieces) / crt_hip_integrated2_* write for
 * the same level sums.  Reads cols->psi (ncol, nz),
 * aI_sl, aI_sh, I_dr, I_df_d, I_df_u; writes aI, F, I_d; aI_dr and totals are ignored.  ngroup 1..4. */
int crt_hip_bandsum_finish_f64(const crt_columns* cols, int32_t ngroup, const crt_bandsum_out* out, crt_stream_t stream);

/*
 * Fused solve + epilogue: the integrated outputs of crt_hip_absorb_bandsum_f64 (same shapes and meaning) straight from
 * the inputs, WITHOUT writing any profile to memory (bytes per solve drop from ~2 kB to ~40 B; the variant SURVEY.md
 * section 8(d) asks to report separately).  Schemes: 2s, 4s, bl, g77, bf, n79, zq, zq_pa; nb <= 1024.
 */
int crt_hip_integrated_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts,
                           const double* band_w, int32_t ngroup, double* aI, double* aI_sl, double* aI_sh, double* totals,
                           void* workspace, size_t workspace_bytes, crt_stream_t stream);
/* f32 storage: float spectra (crt_bands_f32); band_w, aI, aI_sl, aI_sh, totals and the workspace stay double */
int crt_hip_integrated_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts,
                           const double* band_w, int32_t ngroup, double* aI, double* aI_sl, double* aI_sh, double* totals,
                           void* workspace, size_t workspace_bytes, crt_stream_t stream);

/*
 * Level-subset solve: the SPECTRA of the four contract profiles at a few chosen levels, without writing the other levels.  These are
 * the per-band terms of the reference's compare_ebal (crt1d/diagnostics.py:510-522) before their band integral -- top-of-canopy
 * reflectance I_df_u[nz-1], ground-level transmission I_dr[0] + I_df_d[0], spectra at sensor heights -- and the rows
 * levels[r] of the I_dr, I_df_d, I_df_u, F arrays of the solver return dicts (_solve_2s.py:158-163, _solve_4s.py:293,
 * _solve_n79.py:157-164, _solve_zq.py:221-229, _solve_bl.py:93, _solve_g77.py:127-135, _solve_bf.py:144-153, _solve_zq_pa.py:413-418).
 *
 *  - levels: HOST array of nsel level indices, 1 <= nsel <= CRT_MAX_LEVEL_SELECT, strictly ascending, each in [0, nz).  Copied by value
 *    into the kernel arguments: the caller's array may go away once the call returns, and the launch is capturable into a hipGraph.
 *  - out: I_dr, I_df_d, I_df_u, F, each [ncol][nsel][nb] (bands contiguous; row r = level levels[r]) or NULL when not wanted; at least
 *    one of the four is given.  x0, x1, x2 must be NULL (the scheme-specific extras are not served).
 *  - every row is BITWISE the row levels[r] that crt_hip_solve_f64 / _f32 writes for the same inputs (same scheme objects, same
 *    arithmetic), for all eight schemes; the f32 entry writes those rows rounded once to float, also where the f32 profile path of
 *    zq_pa is CRT_ERR_UNSUPPORTED.
 *  - workspace and opts as for crt_hip_solve_f64 (crt_hip_workspace_bytes_nb; CRT_FLAG_SKIP_PRECOMPUTE, CRT_FLAG_PRECOMPUTE_ONLY keep
 *    their meaning; tune is validated, its keys do not apply).
 *  - CRT_ERR_BAD_ARG before any launch for null, unsorted, duplicate or out-of-range levels, nsel outside 1..CRT_MAX_LEVEL_SELECT, all
 *    four outputs NULL or an extra non-NULL.  Any nb.  Shape limit: the K0 record and the checkpoints of the tridiagonal sweep (zq_pa:
 *    on its grid of min(100, nz) rows, plus the grid rows the selected levels read) must fit in LDS for a 64-band slice -- n79 serves
 *    nz <= 1360, zq nz <= 2271, zq_pa nz <= 1487 (64 levels) to 4495 (two levels) -- else CRT_ERR_UNSUPPORTED with nothing written.
 *    The closed forms (2s, 4s, bl, g77, bf) serve every nz.
 */
#define CRT_MAX_LEVEL_SELECT 64
int crt_hip_levels_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_options* opts, const int32_t* levels,
                       int32_t nsel, const crt_outputs* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);
int crt_hip_levels_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_options* opts, const int32_t* levels,
                       int32_t nsel, const crt_outputs_f32* out, void* workspace, size_t workspace_bytes, crt_stream_t stream);

/*
 * Sun-angle series of level spectra: what crt_hip_levels_f64 / _f32 writes, for `nt` sun states of every column in ONE call -- the diurnal
 * or seasonal course of the spectral albedo I_df_u[nz-1] / I_d[nz-1], of the spectrum transmitted to the ground or of the spectrum at a
 * sensor height: the per-band terms of compare_ebal (crt1d/diagnostics.py:510-522) per time step of the reference's `update_p(psi=...)` +
 * `run()` loop.  The product of the two entries above: inputs as crt_hip_integrated_series_f64, levels and outputs as crt_hip_levels_*.
 *
 *  - cols->psi, cols->g_at_psi, bands->I_dr0, bands->I_df0 are NOT read and may be NULL.  The sun states come from `sun`, element
 *    (c, t, b) of I_dr0 / I_df0 at p[c*col_stride + t*nb + b]; col_stride = 0 broadcasts one series over all columns.  The f32 entry takes
 *    crt_sun_series_f32: float I_dr0 / I_df0 (widened on load, as the spectra of crt_bands_f32); psi and g_at_psi stay double.
 *  - levels: as crt_hip_levels_f64 (HOST array copied by value, 1 <= nsel <= CRT_MAX_LEVEL_SELECT, strictly ascending, each in [0, nz)).
 *  - out: I_dr, I_df_d, I_df_u, F, each [ncol][nt][nsel][nb] or NULL; at least one of the four is given; x0, x1, x2 must be NULL.
 *  - CONTRACT: for every t, slice [:, t] of every output is BITWISE what crt_hip_levels_f64 (resp. _f32) writes for the same columns with
 *    psi = sun.psi[:, t], g_at_psi = sun.g_at_psi[:, t], I_dr0 = sun.I_dr0[:, t], I_df0 = sun.I_df0[:, t]: all eight schemes, uniform and
 *    ragged dLAI, CRT_G_TABLE columns; hence, through the contract of crt_hip_levels_*, bitwise a row of the full solve of that step.  The
 *    series kernels run the per-step level kernels' bodies (same scheme objects, same level walk) on the same records, with the same band
 *    slices and the same choice of M.
 *  - what is shared: the column precompute (K0), as in crt_hip_integrated_series_f64 (k_colpre<canopy> once per column, k_colsun once per
 *    (column, t)).  One workgroup per (column, band slice, t) assembles its record in LDS from the two and runs the per-step body.
 *  - workspace: [ncol] canopy records and [ncol][nt] sun records, nothing else (zq_pa's level kernel sweeps its grid in LDS), so
 *    crt_hip_levels_series_workspace_bytes takes no nb.  It is 0 for a bad scheme, non-positive sizes or a size beyond size_t.
 *    The record layouts of the two series entries COINCIDE (canopy records from the start, the sun records right behind them): a workspace
 *    filled by crt_hip_integrated_series_f64 for the same scheme, columns, options and sun.psi may be used here with
 *    CRT_FLAG_SKIP_PRECOMPUTE, and the other way round; crt_hip_series_workspace_bytes is never smaller than this query, so a buffer of that
 *    size serves both entries.
 *  - CRT_FLAG_PRECOMPUTE_ONLY fills the workspace (both kinds of record) and launches no level kernel; CRT_FLAG_SKIP_PRECOMPUTE: the
 *    workspace holds the records of an earlier series call with the same scheme, columns, options and sun.psi (only the spectra changed).
 *  - any nb (band slices as crt_hip_levels_*).  Shape limits: every (nz, nsel) that crt_hip_levels_* serves with its record in LDS -- n79
 *    nz <= 1360, zq nz <= 2271, zq_pa nz <= 1487 (64 levels) to 4495 (two levels); a closed-form column (2s, 4s, bl, g77, bf) whose K0
 *    record exceeds 160 KB (nz > ~10000; bl ~6800) is CRT_ERR_UNSUPPORTED here: the per-step kernel reads such a record from the
 *    workspace, the series has no assembled record there.  Any nt with ncol * nt < 2^31 and nslice * ceil(nt / 65535) <= 65535 (the grid
 *    is ncol x min(nt, 65535) x nslice * ceil(nt / 65535)).  Every CRT_ERR_UNSUPPORTED is found before K0 runs: neither outputs nor
 *    workspace are touched.
 *  - CRT_ERR_BAD_ARG before any launch: NULL sun, sun->psi, I_dr0 or I_df0; nt < 1; col_stride neither 0 nor >= nt * nb; g_at_psi NULL
 *    while cols->g_table is given; bad, unsorted or duplicate levels; all four outputs NULL; a non-NULL extra output; an out-of-range tune
 *    value; everything else crt_hip_levels_* rejects.  CRT_ERR_WORKSPACE below crt_hip_levels_series_workspace_bytes.
 *  - capturable into a hipGraph after the first call per device; crt_hip_last_kernel names the K0 forms and the series level kernel
 *    (k_lev_series<...>, k_tri_lev_series<...>, k_zqpa_lev_series<...>).
 */
typedef struct crt_sun_series_f32 {
  int32_t nt;               /* sun states per column, >= 1 */
  const double* psi;        /* [ncol][nt] solar zenith angle, radians */
  const double* g_at_psi;   /* [ncol][nt] G(psi[c][t]); read for CRT_G_TABLE columns only (else may be NULL) */
  int64_t col_stride;       /* of I_dr0 / I_df0: nt*nb (or larger) per column, 0 = one series for every column */
  const float* I_dr0;       /* element (c, t, b) at p[c*col_stride + t*nb + b] */
  const float* I_df0;
} crt_sun_series_f32;

size_t crt_hip_levels_series_workspace_bytes(int scheme, int32_t ncol, int32_t nz, int32_t nt);
int crt_hip_levels_series_f64(int scheme, const crt_columns* cols, const crt_bands* bands, const crt_sun_series* sun, const crt_options* opts,
                              const int32_t* levels, int32_t nsel, const crt_outputs* out, void* workspace, size_t workspace_bytes,
                              crt_stream_t stream);
int crt_hip_levels_series_f32(int scheme, const crt_columns* cols, const crt_bands_f32* bands, const crt_sun_series_f32* sun,
                              const crt_options* opts, const int32_t* levels, int32_t nsel, const crt_outputs_f32* out, void* workspace,
                              size_t workspace_bytes, crt_stream_t stream);

/*
 * diagnostics.band's reduction for ANY variable with a trailing wavelength axis (diagnostics.py:81, `(da * w).sum(dim="wl")`):
 * out[row][g] = sum_b band_w[g][b] X[row][b], X = [nrow][nb], band_w = [ngroup <= 4][nb], out = [nrow][ngroup].  Used by
 * crt1d_amd.diagnostics.band for the variables of a single Model's dataset (incl. the schemes' own aI_*_scheme outputs); the batched
 * path uses crt_hip_absorb_bandsum2_f64 / crt_hip_integrated2_f64.
 */
int crt_hip_band_reduce_f64(const double* X, int64_t nrow, int32_t nb, const double* band_w, int32_t ngroup, double* out, crt_stream_t stream);

/*
 * Per-band layer absorption (model.py:573-647 `_calc_absorption`): out7 = {aI, aI_df, aI_dr, aI_sh, aI_sl, aI_df_sl,
 * aI_df_sh}, each [ncol][nz-1][nb]; laim, f_slm [ncol][nz-1].
 */
int crt_hip_absorb_f64(const crt_columns* cols, const crt_bands* bands, const double* I_dr, const double* I_df_d,
                       const double* I_df_u, double* const* out7, double* laim, double* f_slm, crt_stream_t stream);
/* f32 storage: float leaf optics, profiles and out7 (each output is the fp64 value rounded once); laim and f_slm stay double */
int crt_hip_absorb_f32(const crt_columns* cols, const crt_bands_f32* bands, const float* I_dr, const float* I_df_d, const float* I_df_u,
                       float* const* out7, double* laim, double* f_slm, crt_stream_t stream);

/*
 * tau_d(L) = 2 int_0^{pi/2} exp(-K_b(psi) L) sin(psi) cos(psi) dpsi for n values of L: crt1d/solvers/common.py:56-87 `tau_df_fn`
 * (`_tau_df_fn_scalar` :30-37 with the library's fixed 96-node rule instead of QUADPACK, `_tau_df_fn_scalar_9sky` :40-53
 * unchanged).  kb_nodes[CRT_NQ] = K_b at the angles of crt_hip_quad_nodes() (device memory, like L and out).  The solvers get the
 * same numbers from their K0 kernel; this entry point serves callers of `tau_df_fn` / `K_df_fn` (:90-95).
 */
int crt_hip_tau_d_f64(const double* kb_nodes, const double* L, int64_t n, int32_t method, double* out, crt_stream_t stream);

/*
 * Input side, batched.
 *
 * crt_hip_smear_tuv_f64 replaces crt1d/spectra.py:260-300 `smear_tuv(x, y, bins)` (per-bin kernel `_smear_tuv_1`,
 * spectra.py:221-257): out[s][i] = trapezoidal integral of y_s(x) over [bins[i], bins[i+1]] (clipped to the x range)
 * divided by the bin width.  x: increasing grid, [nx] shared by all spectra (x_stride = 0) or [nspec][x_stride];
 * y: [nspec][nx]; bins: [nbins + 1]; out: [nspec][nbins].  Same floating-point operations, same order as the reference.
 *
 * crt_hip_lai_beta_f64 replaces crt1d/leaf_area.py:42-93 `distribute_lai_beta(h_c, LAI, n, h_min=0.5)` for ncol canopies:
 * lai, z (and lad unless NULL) are [ncol][nz]; h_c, LAI, h_min are [ncol] (h_min NULL = 0.5 everywhere).  lai is
 * bit-identical to the reference (numpy.linspace arithmetic); z and lad agree to ~1e-14 (Beta ppf by Newton iteration on
 * the closed form of I_x(a, 3) instead of scipy's inverse).
 */
int crt_hip_smear_tuv_f64(const double* x, int64_t x_stride, int32_t nx, const double* y, int32_t nspec, const double* bins,
                          int32_t nbins, double* out, crt_stream_t stream);
int crt_hip_lai_beta_f64(const double* h_c, const double* LAI, const double* h_min, int32_t ncol, int32_t nz, double* lai, double* z,
                         double* lad, crt_stream_t stream);

/*
 * Device buffers for the output profiles, with a deterministic placement in HBM (optional; any device pointer works with the
 * solve entry points).  On MI355X the store pattern of the solve kernels runs at ~5.5 TB/s when all the memory written at one
 * time lies in one "class" of physical memory and at ~7 TB/s when it is spread over two or three (csrc/buffers.hip explains the
 * measurement).  crt_hip_buffer_alloc_set allocates the n arrays of one output set from 512 MB physical chunks (HIP
 * virtual-memory API), classifies every new chunk with a ~1 ms probe, and interleaves the classes across the arrays so that a
 * kernel sweeping all n arrays in step always writes a balanced mix.  ptrs[a] receives a device pointer to at least bytes[a]
 * bytes (2 MB aligned).  Buffers belong to the current device; free each with crt_hip_buffer_free after all work that uses it
 * has completed.  Its chunks return to a per-device pool that keeps at most a RETENTION CAP (8 GB by default; environment
 * CRT1D_POOL_RETAIN_MB, or crt_hip_buffer_set_retain(bytes), which also applies the new cap at once): what exceeds the cap goes back
 * to the driver inside crt_hip_buffer_free, so freeing a large set makes its memory available to every other allocator again;
 * crt_hip_buffer_trim hands back the rest.  Looking for chunks of other classes ("exploration") transiently takes at most half of the
 * memory that stays free beside the request (<= 96 GB), and is abandoned for good on a device that shows a single class.
 * Synchronous (like hipMalloc): runs short probe kernels on a private stream and waits for them -- not capturable into a hipGraph,
 * so allocate (and construct plans) outside stream capture.  No counterpart in the reference (NumPy owns its arrays).
 * crt_hip_buffer_alloc = a set of one.
 * crt_hip_buffer_describe writes one letter per chunk of a buffer (X / Y / Z = class, ? = ambiguous) into buf;
 * crt_hip_buffer_stats fills {chunks created, chunks released, probes run, probe microseconds, free chunks, classes seen}.
 */
int crt_hip_buffer_alloc_set(int32_t n, const size_t* bytes, void** ptrs);
int crt_hip_buffer_alloc(size_t bytes, void** ptr);
int crt_hip_buffer_free(void* ptr);
int crt_hip_buffer_trim(void);
int crt_hip_buffer_set_retain(size_t bytes);
int crt_hip_buffer_describe(const void* ptr, char* buf, size_t n);
int crt_hip_buffer_stats(int64_t* out6);

/* name and configuration of the solve kernel chosen by the calling thread's most recent solve / integrated call
 * (e.g. "k_pipe<2s,f64> T=8 store_waves=3 lds=81536"); reporting only, valid until the thread's next call */
const char* crt_hip_last_kernel(void);

/* bandwidth probes used by bench.py to report a measured HBM ceiling next to the 8 TB/s spec */
int crt_hip_probe_fill_f64(double* dst, size_t n, double value, crt_stream_t stream);
int crt_hip_probe_copy_f64(double* dst, const double* src, size_t n, crt_stream_t stream);
/* The device math the solve kernels use in place of libm: e[i] = exp(x[i]) (18 instructions, <= 1 ulp), sn / cs[i] = sin / cos(x[i])
 * (two-term Cody-Waite reduction, absolute error ~2e-16 for |x| < 1e6; the oscillatory modes of solve_4s).  Diagnostic: lets a test
 * bound their error against the host's libm, which is what the reference's numpy.exp calls (_solve_2s.py:125-131). */
int crt_hip_probe_math_f64(const double* x, size_t n, double* e, double* sn, double* cs, crt_stream_t stream);
/* The flush of the solve kernels alone: workgroup c writes column c (col_doubles doubles) of all `narrays` arrays in step, run_doubles at a
 * time (T levels x nb bands), with 16-byte streaming stores.  On a set from crt_hip_buffer_alloc_set it measures the store rate that
 * placement allows; it OVERWRITES the arrays with `value`.  No counterpart in the reference. */
int crt_hip_probe_store_set_f64(double* const* arrays, int32_t narrays, int64_t ncol, int64_t col_doubles, int32_t run_doubles, double value,
                                crt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRT1D_HIP_H */
