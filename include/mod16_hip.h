/*
 * mod16_hip.h -- C ABI of libmod16hip.so, the MI355X (gfx950) engine behind the
 * MOD16 forward run.
 *
 * The reference (arthur-e/MOD16 v1.2.0) is pure Python/numpy and has no FFI of
 * its own; the boundary this library replaces is the body of
 *     MOD16.evapotranspiration()            reference mod16/__init__.py:675-793
 * and the sub-methods it calls (:795-1258, :1261-1397), plus the per-pixel
 * parameter gather `bplut[key][pft_map]` that precedes it for multi-class
 * rasters (reference mod16/utils.py:81-117 + forward-run notebook cell 32).
 * The Python class `mod16_amd.MOD16` binds these entry points with ctypes
 * (see INTEGRATION.md for the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - plain C types only; no exceptions cross the ABI; every call returns
 *     MOD16_OK (0) or a negative MOD16_ERR_* code; mod16_last_error() has text;
 *   - the library never frees or retains caller memory;
 *   - `where` says whether the data pointers are HOST (pageable or pinned
 *     memory; the call stages tiles through the GPU and is synchronous) or
 *     DEVICE (zero-copy, asynchronous on `stream`, a hipStream_t or NULL);
 *     HOST calls of at most MOD16_SMALL_PIXELS pixels (environment, default
 *     65536, 0 = never; mod16_et_*, mod16_et_raw_*, mod16_method_*,
 *     mod16_et_static_*) issue no copy commands: the kernel reads its inputs
 *     from a page-locked buffer of the ctx and writes its outputs there (one
 *     launch, one synchronisation; same kernels, same results -- with ONE
 *     exception: a MOD16_MATH_MIXED call whose pixel count is no multiple of
 *     four computes its last, incomplete vector through the pipeline here and
 *     with the float64 (FAST) arithmetic on the staged path: those up to three
 *     pixels agree to the mixed form's tolerance, not bit for bit), and a class
 *     code >= 13 is found before anything is launched;
 *   - DEVICE launches of one ctx share its diagnostics workspace: on ONE stream
 *     they are ordered anyway and nothing is added between them; the first
 *     launch a ctx makes on a second stream waits for the device once, and
 *     from then on every launch records an event the next one on another
 *     stream waits for (a stream may be destroyed by its owner at any time:
 *     the library never touches a stream it is not launching on). That one
 *     wait is hipDeviceSynchronize(): other contexts of the process stall with
 *     it, and it fails (MOD16_ERR_HIP) while another thread captures a stream
 *     in hipStreamCaptureModeGlobal -- a program that does either gives every
 *     stream its own ctx, or launches once on each stream before it starts
 *     capturing;
 *   - a launch that did not process its whole raster (kStatusIncomplete, see
 *     mod16_check_status) is found by the kernels that run BEHIND the pipeline
 *     kernel: the guard's pass (every guarded launch) or the diagnostics sum
 *     (MOD16_DOMAIN_TRUSTED launches) -- a trusted launch without diagnostics
 *     is not checked;
 *   - a ctx serialises the calls made on it (every entry point holds the ctx's
 *     mutex), so sharing one between host threads is safe; for concurrency use
 *     one ctx per host thread and GPU (each owns its staging slabs, streams,
 *     BPLUT copy and workspace).
 */
#ifndef MOD16_HIP_H
#define MOD16_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOD16_ABI_VERSION 16

#if defined(__GNUC__)
#define MOD16_API __attribute__((visibility("default")))
#else
#define MOD16_API
#endif

/* MOD16.evapotranspiration() argument order, mod16/__init__.py:675-682 */
#define MOD16_N_DRIVERS 14
enum mod16_driver {
    MOD16_LW_NET_DAY = 0, MOD16_LW_NET_NIGHT, MOD16_SW_RAD_DAY,
    MOD16_SW_RAD_NIGHT, MOD16_SW_ALBEDO, MOD16_TEMP_DAY, MOD16_TEMP_NIGHT,
    MOD16_TEMP_ANNUAL, MOD16_TMIN, MOD16_VPD_DAY, MOD16_VPD_NIGHT,
    MOD16_PRESSURE, MOD16_FPAR, MOD16_LAI
};

/* MOD16.required_parameters order, mod16/__init__.py:152-155 */
#define MOD16_N_PARAMS 11
enum mod16_param {
    MOD16_TMIN_CLOSE = 0, MOD16_TMIN_OPEN, MOD16_VPD_OPEN, MOD16_VPD_CLOSE,
    MOD16_GL_SH, MOD16_GL_WV, MOD16_G_CUTICULAR, MOD16_CSL, MOD16_RBL_MIN,
    MOD16_RBL_MAX, MOD16_BETA
};

/* restore_bplut() arrays have 13 entries indexed by PFT code (utils.py:104) */
#define MOD16_N_CLASSES 13

/* order of the optional component outputs (`separate=True`, :789-790) */
#define MOD16_N_COMPONENTS 6
enum mod16_component {
    MOD16_CANOPY_DAY = 0, MOD16_SOIL_DAY, MOD16_TRANS_DAY,
    MOD16_CANOPY_NIGHT, MOD16_SOIL_NIGHT, MOD16_TRANS_NIGHT
};

enum mod16_status {
    MOD16_OK = 0,
    MOD16_ERR_ARG = -1,          /* NULL / misaligned / inconsistent argument */
    MOD16_ERR_HIP = -2,          /* a HIP runtime call failed                 */
    MOD16_ERR_CLASS_RANGE = -3,  /* a class code >= 13 (numpy: IndexError)    */
    MOD16_ERR_NOMEM = -4,
    MOD16_ERR_NO_DEVICE = -5,    /* no usable gfx950 device                   */
    MOD16_ERR_NO_BPLUT = -6      /* class raster given before a BPLUT was set */
};

enum mod16_where { MOD16_HOST = 0, MOD16_DEVICE = 1 };

/* flags of mod16_et_*
 *
 * MOD16_MATH_FAST rearranges the smooth arithmetic (conductances instead of resistances,
 * shared per-period terms, table exp / log) and keeps every comparison of the reference:
 * within 1e-9 of the reference-order kernel, NaN and exact-zero masks identical. Its own
 * domain is finite drivers of physical sign and magnitude (NaN anywhere, zeros and the usual
 * fill values in the radiation / albedo / VPD / fPAR / LAI fields included). A pixel outside
 * it is detected in the kernel (csrc/mod16_physics.hpp, fast_out_of_domain) and computed in the
 * reference's operation order instead. The test, exactly:
 *     |A_day| = |sw_rad_day (1 - albedo) + lw_net_day|, |lw_net_night|,
 *     |sw_rad_night (1 - albedo) + lw_net_night|, |fPAR|, |LAI|, |pressure|, |VPD day|,
 *     |VPD night| at or above 1e50 (or infinite);  pressure below 1 Pa (zero, negative);
 *     a day or night temperature at or outside 36 K .. 1332 K (35.85 K is the pole of the
 *     saturation formula, from 1332.4 K the latent heat is negative).
 * NaN operands never flag a pixel. With this the DEFAULT arithmetic returned what the
 * reference returns on every input class tested: a ladder of 56 magnitudes in each driver,
 * 1.2 M random pairs and a storm of independently special drivers (tests/fuzz_domain.py),
 * signalling-NaN patterns next to an infinity (tests/test_gpu_guard.py), NaN / zero / inf
 * masks included. The raw-driver forms test the raw fields instead: |specific humidity| < 1
 * kg/kg, |surface pressure| < 1e50 Pa, an elevation between -2000 m and 12000 m (the interval on
 * which the fast form evaluates air pressure as a polynomial, 3.7e-14 relative; MIXED: |z| < 25 km),
 * the radiation terms as above, and day / night temperatures between 190 K and 360 K (-83 C ..
 * +87 C, FAST and MIXED): on that interval the two saturation formulas of the path -- MOD16.vpd's
 * 610.7 exp(17.38 tc / (239 + tc)) and svp's 610.8 exp(17.27 tc / (237.3 + tc)) -- share one
 * exponential (their exponents differ by |delta| < 0.043, exp(delta) is a short polynomial; round 5).
 * MOD16_MATH_EXACT is the reference's operation order throughout. */
#define MOD16_MATH_FAST   0u  /* strength-reduced arithmetic (default)          */
#define MOD16_MATH_EXACT  1u  /* reference operation order, IEEE divide/pow     */
#define MOD16_MATH_MIXED  2u  /* float32 rasters: float64 where it decides a mask or
                                 feeds the humidity terms, packed float32 elsewhere
                                 (dense class rasters; other shapes run FAST). Its domain
                                 is physical drivers (|lw|, |sw|, |albedo|, |vpd|, |fpar|,
                                 |lai|, |tmin| < 1e5, 1e3 <= pressure < 1e7 Pa, 90 K < T < 1332 K);
                                 pixels outside it are computed in the reference's order,
                                 float64, like FAST's. Values whose wet-canopy or bare-soil
                                 numerator cancels below 1/320 of its terms relative to the
                                 period's total (one pixel in 700 of the synthetic grid) are
                                 computed again with the FAST form's float64 arithmetic behind
                                 the pipeline kernel (round 6): against that arithmetic no value
                                 of the global grid is off by more than 2.0e-4 of itself. With
                                 MOD16_DOMAIN_TRUSTED nothing is revisited, that tail included */
/* The caller vouches that every driver lies inside the domain above (quality-controlled or
 * NaN-masked rasters): the totals form of the production pipeline (dense class raster,
 * outputs day + night; mod16_et_*, mod16_et_diag_*, mod16_et_tiled_*, their graphs) then runs
 * the instance without the domain test and without the dispatch that revisits flagged pixels
 * (-1.6 % kernel time on the float64 global grid, round 5; MIXED: -7 %, of which 5 % are the
 * cancellation budgets of round 6: profiles/r06_mixed_cancel_threshold.txt). A pixel outside the domain then
 * gets whatever the rearranged arithmetic gives. Other forms and shapes ignore the flag. */
#define MOD16_DOMAIN_TRUSTED 4u

typedef struct mod16_ctx mod16_ctx;

MOD16_API int mod16_version(void);
MOD16_API const char* mod16_strerror(int status);
/* text of the last failure on this ctx ("" if none); valid until next call */
MOD16_API const char* mod16_last_error(const mod16_ctx* ctx);

MOD16_API int mod16_device_count(int* count);
MOD16_API int mod16_create(int device, mod16_ctx** out);
MOD16_API int mod16_destroy(mod16_ctx* ctx);

/*
 * Biome-properties look-up table: `lut` is a host array [13][11] of float64,
 * row = PFT code, column = enum mod16_param; rows of invalid classes hold NaN
 * (what restore_bplut() leaves at 0 and 11, utils.py:104-116). Replaces the
 * reference's per-pixel gather `params_dict[key][pft_map]`.
 */
MOD16_API int mod16_set_bplut_f64(mod16_ctx* ctx, const double* lut);

/*
 * The forward run over n pixels: replaces MOD16.evapotranspiration()
 * (mod16/__init__.py:675-793) and everything below it.
 *
 *   cls      uint8 class raster [n], or NULL. With a class raster the
 *            parameters come from the BPLUT (set beforehand); a code >= 13
 *            makes the call (HOST) or mod16_check_status() (DEVICE) return
 *            MOD16_ERR_CLASS_RANGE and yields NaN for that pixel.
 *   drivers  the 14 driver arrays, order enum mod16_driver.
 *   dstride  element stride of each driver: 1 = dense array of n elements,
 *            0 = one value broadcast to every pixel (numpy scalar).
 *   params   used only when cls == NULL: the 11 parameters, each dense
 *            (pstride 1, per-pixel `params_dict[key][pft_map]` arrays) or a
 *            broadcast scalar (pstride 0, the single-PFT MOD16(params) case).
 *   out_day, out_night   [n] totals in kg m-2 s-1 (:792); may be NULL if
 *            only components are wanted.
 *   out_sep  NULL, or 6 arrays [n] in enum mod16_component order (any entry
 *            may be NULL) -- the `separate=True` outputs (:790).
 *   flags    MOD16_MATH_*.
 */
MOD16_API int mod16_et_f64(mod16_ctx* ctx, const uint8_t* cls,
                 const double* const* drivers, const int64_t* dstride,
                 const double* const* params, const int64_t* pstride,
                 int64_t n, double* out_day, double* out_night,
                 double* const* out_sep, unsigned flags, int where,
                 void* stream);

/*
 * The same with the reference's 2-level broadcasting: its callers pass (N,)
 * arrays -- one value per site: pressure, temp_annual, the per-site parameters
 * `params_dict[key][pft_map]` -- against (T, N) drivers (mod16/__init__.py:180-181,
 * forward-run notebook cell 17), and numpy broadcasts them. Here every input
 * carries a broadcast kind instead of a 0 / 1 stride and nothing is made dense:
 * with the (T, N) raster flattened to n = T * inner pixels (inner = N),
 *
 *     MOD16_BC_SCALAR  one value                     element 0
 *     MOD16_BC_DENSE   [n]                           element i
 *     MOD16_BC_ROW     [inner]   an (N,) array       element i % inner
 *     MOD16_BC_COL     [n/inner] a (T, 1) array      element i / inner
 *
 * `cls_kind` is the kind of the class raster (a per-site PFT vector is a ROW).
 * A call with a ROW or COL input runs the one-pixel-per-thread kernel (in HOST
 * mode the small arrays are uploaded whole, once); without one it is mod16_et_*.
 */
enum mod16_broadcast { MOD16_BC_SCALAR = 0, MOD16_BC_DENSE = 1, MOD16_BC_ROW = 2, MOD16_BC_COL = 3 };
MOD16_API int mod16_et2_f64(mod16_ctx* ctx, const uint8_t* cls, int cls_kind,
                  const double* const* drivers, const int64_t* dkind,
                  const double* const* params, const int64_t* pkind,
                  int64_t inner, int64_t n, double* out_day, double* out_night,
                  double* const* out_sep, unsigned flags, int where, void* stream);
MOD16_API int mod16_et2_f32(mod16_ctx* ctx, const uint8_t* cls, int cls_kind,
                  const float* const* drivers, const int64_t* dkind,
                  const float* const* params, const int64_t* pkind,
                  int64_t inner, int64_t n, float* out_day, float* out_night,
                  float* const* out_sep, unsigned flags, int where, void* stream);

/* float32 data: MOD16_MATH_FAST widens to float64 on load, computes in float64 and
 * rounds once on store; MOD16_MATH_EXACT keeps float32 arithmetic in the reference's
 * operation order (what numpy does for the reference on float32 inputs);
 * MOD16_MATH_MIXED (dense class rasters: totals, components, potential ET, raw drivers): float64 for
 * the humidity terms (and for the radiation balance next to its clamps), packed float32
 * for the rest, every
 * decision behind a NaN or an exact zero made as in FAST; same masks as FAST, median
 * relative difference 1e-7, absolute difference below 1e-6 of the largest value,
 * 1.5x faster */
MOD16_API int mod16_et_f32(mod16_ctx* ctx, const uint8_t* cls,
                 const float* const* drivers, const int64_t* dstride,
                 const float* const* params, const int64_t* pstride,
                 int64_t n, float* out_day, float* out_night,
                 float* const* out_sep, unsigned flags, int where,
                 void* stream);

/*
 * HOST mode with diagnostics, and the unit the multi-GPU entry points of the Python layer deal
 * out. The numpy entry points (MOD16.evapotranspiration(), mod16/__init__.py:675-793, and
 * evapotranspiration_raster) stage host arrays through the GPU in tiles of
 * mod16_host_tile_pixels() pixels. mod16_et_hdiag_* is mod16_et_* with where = MOD16_HOST and
 * both totals, plus ONE diagnostics vector per staged tile: tile_diag is a HOST array
 * [ceil(n / mod16_host_tile_pixels())][8] (layout of mod16_reduce_diag_*), row t reduced on the
 * device, in a fixed order, from the outputs of pixels [t * tile, (t + 1) * tile) while they are
 * still there. Because a tile's row depends on that tile alone, a raster cut at tile boundaries
 * and dealt over several contexts / GPUs (one host thread per ctx, each writing its rows of the
 * one array) gives the same rows -- and, folded in tile order with mod16_fold_diag_host, the same
 * diagnostics bit for bit -- as the undivided call, whatever the number of GPUs (SURVEY.md 8e:
 * "tiles of the global grid shard embarrassingly", here for the PCIe-bound HOST paths, one link
 * per GPU, no collective).
 */
MOD16_API int64_t mod16_host_tile_pixels(void);
MOD16_API int mod16_et_hdiag_f64(mod16_ctx* ctx, const uint8_t* cls,
                       const double* const* drivers, const int64_t* dstride,
                       const double* const* params, const int64_t* pstride,
                       int64_t n, double* out_day, double* out_night,
                       unsigned flags, double* tile_diag);
MOD16_API int mod16_et_hdiag_f32(mod16_ctx* ctx, const uint8_t* cls,
                       const float* const* drivers, const int64_t* dstride,
                       const float* const* params, const int64_t* pstride,
                       int64_t n, float* out_day, float* out_night,
                       unsigned flags, double* tile_diag);
/* diag[8] = parts[0] (+) parts[1] (+) ... in the order given: sums and counts [0..5] added,
 * maxima [6..7] maximised (host arrays; the rule of mod16_fold_diag). Needs no ctx. */
MOD16_API int mod16_fold_diag_host(const double* parts, int64_t count, double* diag);

/*
 * Forward run that also returns potential ET: as
 * mod16_et_* (out_day / out_night may be NULL), plus pet_day / pet_night [n]
 * in kg m-2 s-1 = wet-canopy evaporation + saturated-soil evaporation +
 * unsaturated-soil evaporation without the soil-moisture constraint +
 * Priestley-Taylor potential transpiration (reference README.md:404-424;
 * MOD16.potential_soil_evaporation :449-544, MOD16.potential_transpiration
 * :546-602 with alpha = 1.26, evaporation_wet_canopy :866-961).
 */
MOD16_API int mod16_et_pet_f64(mod16_ctx* ctx, const uint8_t* cls,
                     const double* const* drivers, const int64_t* dstride,
                     const double* const* params, const int64_t* pstride,
                     int64_t n, double* out_day, double* out_night,
                     double* pet_day, double* pet_night, unsigned flags,
                     int where, void* stream);
MOD16_API int mod16_et_pet_f32(mod16_ctx* ctx, const uint8_t* cls,
                     const float* const* drivers, const int64_t* dstride,
                     const float* const* params, const int64_t* pstride,
                     int64_t n, float* out_day, float* out_night,
                     float* pet_day, float* pet_night, unsigned flags,
                     int where, void* stream);

/*
 * Forward run on raw drivers: the pre-processing the
 * reference does in front of the forward run (mod16/calibration.py:380-423) is
 * folded into the pixel kernel --
 *   vpd_day   = MOD16.vpd(qv10m_day, ps_day, temp_day)            :604-644
 *   vpd_night = max(MOD16.vpd(qv10m_night, ps_night, temp_night), 0)   calibration.py:398-401
 *   pressure  = MOD16.air_pressure(elevation)                      :414-447
 *   fpar = fpar_pct / 100, lai = lai_x10 / 10                      calibration.py:422-423
 * with fPAR / LAI given as the MODIS uint8 encodings (codes >= 249 = fill ->
 * NaN). `raw` holds 14 arrays in enum mod16_raw_driver order (rstride 0/1 as
 * elsewhere); cls + BPLUT give the parameters. Outputs: out_day / out_night
 * [kg m-2 s-1] and/or, with `day_hours` (hours of daylight per pixel, hstride
 * 0/1), out_total8 = (day h + night (24 - h)) * 8 * 3600 [kg m-2 (8 d)-1], the
 * MOD16A2 unit (reference tests/verification/verify2.py:113-115).
 */
#define MOD16_N_RAW_DRIVERS 14
enum mod16_raw_driver {
    MOD16_RAW_LW_NET_DAY = 0, MOD16_RAW_LW_NET_NIGHT, MOD16_RAW_SW_RAD_DAY,
    MOD16_RAW_SW_RAD_NIGHT, MOD16_RAW_SW_ALBEDO, MOD16_RAW_TEMP_DAY,
    MOD16_RAW_TEMP_NIGHT, MOD16_RAW_TEMP_ANNUAL, MOD16_RAW_TMIN,
    MOD16_RAW_QV10M_DAY, MOD16_RAW_QV10M_NIGHT, MOD16_RAW_PS_DAY,
    MOD16_RAW_PS_NIGHT, MOD16_RAW_ELEVATION
};
MOD16_API int mod16_et_raw_f64(mod16_ctx* ctx, const uint8_t* cls,
                     const double* const* raw, const int64_t* rstride,
                     const uint8_t* fpar_pct, const uint8_t* lai_x10,
                     const double* day_hours, int64_t hstride, int64_t n,
                     double* out_day, double* out_night, double* out_total8,
                     unsigned flags, int where, void* stream);
MOD16_API int mod16_et_raw_f32(mod16_ctx* ctx, const uint8_t* cls,
                     const float* const* raw, const int64_t* rstride,
                     const uint8_t* fpar_pct, const uint8_t* lai_x10,
                     const float* day_hours, int64_t hstride, int64_t n,
                     float* out_day, float* out_night, float* out_total8,
                     unsigned flags, int where, void* stream);

/*
 * Forward run and diagnostics in one pass, DEVICE pointers only: as
 * mod16_et_* with a class raster (BPLUT parameters) and both totals, plus the
 * diagnostics vector of mod16_reduce_diag_* written to ddiag (device, 8
 * doubles). On the production path (dense 16-byte-aligned drivers, n a
 * multiple of the vector width) the outputs are reduced while still in
 * registers, so the extra 16 B/pixel read of a separate reduction is saved;
 * otherwise the call runs the forward run and then the reduction. The sums
 * are deterministic for a given n and device. Asynchronous on `stream`.
 */
MOD16_API int mod16_et_diag_f64(mod16_ctx* ctx, const uint8_t* cls,
                      const double* const* drivers, const int64_t* dstride,
                      int64_t n, double* out_day, double* out_night,
                      unsigned flags, double* ddiag, void* stream);
MOD16_API int mod16_et_diag_f32(mod16_ctx* ctx, const uint8_t* cls,
                      const float* const* drivers, const int64_t* dstride,
                      int64_t n, float* out_day, float* out_night,
                      unsigned flags, double* ddiag, void* stream);

/*
 * mod16_et_diag_* for a raster that is processed again and again (one call per
 * time step of a series): the launch sequence -- ticket-counter reset, pipeline
 * kernel, staged fixed-order sum of the diagnostics -- is captured once into a
 * HIP graph and replayed by mod16_graph_launch on any stream. All pointers are
 * DEVICE pointers and must stay valid and in place; the raster's contents may
 * change between launches. Replays of one graph must be ordered (one stream, or
 * events); deferred errors surface through mod16_check_status as usual.
 * A graph belongs to the context it was captured with -- its kernels read the
 * context's parameter and exp / log tables and report into its status word:
 * destroy the graph first. Once the context is gone, mod16_graph_launch and
 * mod16_time_graph return MOD16_ERR_ARG (nothing is launched);
 * mod16_graph_destroy still frees the graph, in either order.
 */
typedef struct mod16_graph mod16_graph;
MOD16_API int mod16_graph_et_diag_f64(mod16_ctx* ctx, const uint8_t* cls,
                      const double* const* drivers, const int64_t* dstride,
                      int64_t n, double* out_day, double* out_night,
                      unsigned flags, double* ddiag, mod16_graph** out);
MOD16_API int mod16_graph_et_diag_f32(mod16_ctx* ctx, const uint8_t* cls,
                      const float* const* drivers, const int64_t* dstride,
                      int64_t n, float* out_day, float* out_night,
                      unsigned flags, double* ddiag, mod16_graph** out);
MOD16_API int mod16_graph_launch(mod16_graph* graph, void* stream);
MOD16_API int mod16_graph_destroy(mod16_graph* graph);

/*
 * The sub-methods of the reference's class surface (mod16/__init__.py:384-673,
 * :795-1258, :1261-1397), reference operation order. `method` selects one;
 * `in` holds MOD16_METHOD_MAX_IN pointers in the order of the reference
 * signature (table below), NULL = optional argument not given (then computed as
 * the reference does); istride 0 = broadcast scalar, 1 = dense; `params` as in
 * mod16_et_* (may be NULL for the static / module-level methods); `out` holds 2
 * pointers (second NULL unless the method returns a pair); `alpha` is used by
 * POT_TRANSPIRATION only, `tiny` (the reference's argument of that name,
 * :869, :1157; default 1e-7) by EVAP_WET_CANOPY and TRANSPIRATION_*. `where` as
 * in mod16_et_*.
 *
 *   SVP                 temp_k                                     :1340
 *   SVP_SLOPE           temp_k, s?                                 :1370
 *   LHV                 temp_k                                     :121
 *   PSYCHROMETRIC       pressure, temp_k                           :1261
 *   RADIATION_NET       sw_rad, sw_albedo, temp_k                  :1293
 *   AIR_DENSITY         temp_k, pressure, rhumidity                :384
 *   AIR_PRESSURE        elevation_m                                :414
 *   VPD                 qv10m, pressure, tmean                     :604
 *   RHUMIDITY           temp_k, vpd                                :646
 *   POT_SOIL_EVAP       pressure, temp_k, vpd, fpar, rad_soil, r_corr?, lhv?, rh?, f_wet? -> (sat, unsat)  :449
 *   POT_TRANSPIRATION   lw_net, sw_rad, sw_albedo, pressure, temp_k, vpd, fpar, rh?, f_wet?       :546
 *   EVAP_SOIL           pressure, temp_k, vpd, fpar, rad_soil, r_corr?, lhv?, rh?, f_wet?         :795
 *   EVAP_WET_CANOPY     pressure, temp_k, vpd, lai, fpar, rad_canopy, lhv?, rh?, f_wet?           :866
 *   RADIATION_SOIL      lw_d, lw_n, sw_d, sw_n, albedo, t_d, t_n, t_annual, fpar -> (day, night)  :963
 *   SOIL_HEAT_FLUX      rad_net_day, rad_net_night, t_d, t_n, t_annual -> (day, night)            :1055
 *   SURFACE_CONDUCTANCE tmin, vpd_day                              :1121
 *   TRANSPIRATION_DAY / _NIGHT  pressure, temp_k, vpd, lai, fpar, rad_canopy, tmin, r_corr?, lhv?, rh?, f_wet?  :1152
 */
#define MOD16_METHOD_MAX_IN 13
enum mod16_method {
    MOD16_M_SVP = 0, MOD16_M_SVP_SLOPE, MOD16_M_LHV, MOD16_M_PSYCHROMETRIC,
    MOD16_M_RADIATION_NET, MOD16_M_AIR_DENSITY, MOD16_M_AIR_PRESSURE, MOD16_M_VPD,
    MOD16_M_RHUMIDITY, MOD16_M_POT_SOIL_EVAP, MOD16_M_POT_TRANSPIRATION,
    MOD16_M_EVAP_SOIL, MOD16_M_EVAP_WET_CANOPY, MOD16_M_RADIATION_SOIL,
    MOD16_M_SOIL_HEAT_FLUX, MOD16_M_SURFACE_CONDUCTANCE,
    MOD16_M_TRANSPIRATION_DAY, MOD16_M_TRANSPIRATION_NIGHT, MOD16_M_COUNT
};
MOD16_API int mod16_method_f64(mod16_ctx* ctx, int method,
                     const double* const* in, const int64_t* istride,
                     const double* const* params, const int64_t* pstride,
                     int64_t n, double* const* out, double alpha, double tiny,
                     int where, void* stream);
MOD16_API int mod16_method_f32(mod16_ctx* ctx, int method,
                     const float* const* in, const int64_t* istride,
                     const float* const* params, const int64_t* pstride,
                     int64_t n, float* const* out, float alpha, float tiny,
                     int where, void* stream);

/*
 * The vectorised calibration path MOD16._evapotranspiration (reference
 * mod16/__init__.py:195-382; MOD16._et :162-193 is out_day + out_night):
 * latent heat flux [W m-2] for day and night, reference operation order. It
 * is a different algorithm from mod16_et_* (other clamps, tmin_open in the
 * soil-heat-flux condition, transpiration switched for the whole array on
 * any(g_surf > 0)). `rcorr` = NULL or two arrays (day, night), the reference's
 * `r_corr_list`; `tiny` is the reference's argument of that name (:199,
 * default 1e-7); strides as elsewhere. HOST or DEVICE; synchronous in HOST.
 */
MOD16_API int mod16_et_static_f64(mod16_ctx* ctx, const double* const* drivers,
                        const int64_t* dstride, const double* const* params,
                        const int64_t* pstride, const double* const* rcorr,
                        const int64_t* rstride, int64_t n, double* out_day,
                        double* out_night, double tiny, int where, void* stream);
MOD16_API int mod16_et_static_f32(mod16_ctx* ctx, const float* const* drivers,
                        const int64_t* dstride, const float* const* params,
                        const int64_t* pstride, const float* const* rcorr,
                        const int64_t* rstride, int64_t n, float* out_day,
                        float* out_night, float tiny, int where, void* stream);

/*
 * The calibration path batched over parameter vectors:
 * MOD16._evapotranspiration / MOD16._et (reference mod16/__init__.py:162-382)
 * for `ndraw` parameter vectors over the same n pixels in one call -- what the
 * reference's MCMC sampler (calibration.py:907) and Sobol analysis
 * (sensitivity.py:95) evaluate draw by draw. `params` is [ndraw][11] row-major
 * in mod16_param order; outputs are [ndraw][n] row-major, each may be NULL:
 * out_day / out_night [W m-2] and out_total = day + night (MOD16._et). With
 * flags = MOD16_MATH_EXACT row d is bit-identical to mod16_et_static_* called
 * with the scalars params[d] (r_corr computed, `rcorr` = NULL); MOD16_MATH_FAST
 * uses the strength-reduced arithmetic of the forward run (float64 throughout,
 * within 1e-9 of EXACT, same NaN and zero masks, several times faster); pixels outside that
 * arithmetic's domain (the test of MOD16_MATH_FAST above, on the drivers) are left out by the
 * FAST kernels and computed in the reference's operation order behind them, so FAST returns
 * what EXACT returns for them (here also |VPD| >= 1e18 Pa: this path does not clamp the relative
 * humidity from above, mod16/__init__.py:280-281). With `observed` [n] (and optional
 * `weights` [n]) the call also reduces each draw to
 *     sse[d]   = sum_i (weights[i] * (out_total[d][i] - observed[i]))^2
 *     count[d] = number of pairs used (NaN pairs are skipped),
 * both float64 [ndraw], summed in a fixed order (deterministic); the caller
 * forms its objective (e.g. RMSD = sqrt(sse / count)) from them. In DEVICE mode
 * out_total must be given when sse is (it is the workspace). HOST: synchronous.
 */
MOD16_API int mod16_et_static_batch_f64(mod16_ctx* ctx, const double* const* drivers,
                        const int64_t* dstride, int64_t n, const double* params,
                        int64_t ndraw, double* out_day, double* out_night,
                        double* out_total, const double* observed,
                        const double* weights, double* sse, double* count,
                        unsigned flags, int where, void* stream);
MOD16_API int mod16_et_static_batch_f32(mod16_ctx* ctx, const float* const* drivers,
                        const int64_t* dstride, int64_t n, const float* params,
                        int64_t ndraw, float* out_day, float* out_night,
                        float* out_total, const float* observed,
                        const float* weights, double* sse, double* count,
                        unsigned flags, int where, void* stream);

/*
 * The same problem RESIDENT on the device: what the reference's MCMC sampler
 * (calibration.py:907-909) and Sobol analysis (sensitivity.py:94-96) actually do is evaluate
 * MOD16._et thousands of times on the SAME drivers with new parameter vectors.
 * mod16_static_batch_bind_* takes the 14 drivers (dstride 0 / 1 as above), the observations
 * and optional weights once -- where = MOD16_HOST: copied to the device; MOD16_DEVICE: the
 * caller's device arrays are used in place and must outlive the object -- marks the pixels
 * outside the FAST domain, and sizes a workspace for up to `max_draws` parameter vectors.
 *   mod16_static_batch_objective  params [ndraw][11] (HOST, the problem's data type) ->
 *       sse[ndraw], count[ndraw] (HOST float64, as defined above). One evaluation = the
 *       parameters up (ndraw x 88 bytes), ONE graph launch, 16 bytes per draw down; nothing of
 *       size [ndraw][n] exists: the residuals are reduced where they are computed, in a fixed
 *       order (lanes, waves, blocks: the result does not depend on the schedule). The
 *       reference's whole-array branch any(g_surf > 0) (mod16/__init__.py:343-348) is resolved
 *       inside the same launch sequence: every draw is evaluated with transpiration while the
 *       blocks report whether any pixel has g_surf > 0, and the (normally zero) draws without it
 *       are evaluated again without. flags = MOD16_MATH_EXACT at bind time: the kernels of the
 *       unbound call on the resident drivers (bit-identical sums to mod16_et_static_batch_*).
 *   mod16_static_batch_rows       the [ndraw][n] rows (HOST; day / night / total, any may be
 *       NULL): the unbound call's kernels on the resident drivers -- bit-identical rows.
 *   mod16_static_batch_info       n, max_draws and the number of pixels outside the FAST domain.
 *   mod16_static_batch_time       mean milliseconds of the GPU part of the last objective
 *       call's evaluation, plain or fold (graph replays bracketed by HIP events).
 * Calls on one object are serialised by its ctx's mutex. Synchronous.
 *
 * where = MOD16_DEVICE: the object works on a private stream and the interface takes none, so the
 * caller's arrays must be COMPLETE when mod16_static_batch_bind_* is called (synchronise the stream
 * that produced them first) and must not change while the object lives -- the pixels outside the
 * FAST domain are listed once, at bind time, from the values found then. Device memory that cannot
 * be had is MOD16_ERR_NOMEM (bind: resident copies, workspace for max_draws parameter vectors -- about
 * 190 bytes per draw; objective: the per-block partials, 20 bytes x draws x ceil(n / 256), sized for
 * the draws actually evaluated and grown on demand -- a problem bound for max_draws = 4096 that is
 * evaluated 256 draws at a time holds a sixteenth of what 4096 would take; EXACT problems: none).
 */
typedef struct mod16_batch mod16_batch;
MOD16_API int mod16_static_batch_bind_f64(mod16_ctx* ctx, const double* const* drivers,
                        const int64_t* dstride, int64_t n, const double* observed,
                        const double* weights, int64_t max_draws, unsigned flags, int where,
                        mod16_batch** out);
MOD16_API int mod16_static_batch_bind_f32(mod16_ctx* ctx, const float* const* drivers,
                        const int64_t* dstride, int64_t n, const float* observed,
                        const float* weights, int64_t max_draws, unsigned flags, int where,
                        mod16_batch** out);
MOD16_API int mod16_static_batch_objective(mod16_batch* problem, const void* params, int64_t ndraw,
                        double* sse, double* count);
MOD16_API int mod16_static_batch_rows(mod16_batch* problem, const void* params, int64_t ndraw,
                        void* out_day, void* out_night, void* out_total);
MOD16_API int mod16_static_batch_info(const mod16_batch* problem, int64_t* n, int64_t* max_draws,
                        int64_t* n_outside_domain);
MOD16_API int mod16_static_batch_time(mod16_batch* problem, int launches, float* ms);
MOD16_API int mod16_static_batch_destroy(mod16_batch* problem);

/*
 * k-fold cross-validation on a resident problem (ABI 8; mod16_amd/calibration.py). Every pixel
 * (site-day) carries a fold label in 0 .. nfolds - 1, 2 <= nfolds <= 255, each value used at least
 * once; every draw of a fold call carries a code f | (MOD16_FOLD_HELDOUT or 0):
 *   TRAIN (bit clear)   the draw sees the pixels whose label != f,
 *   HELDOUT             the draw sees the pixels whose label == f.
 * A pixel the draw does not see adds nothing to its (sse, count). The reference's whole-array
 * branch any(g_surf > 0) ranges over the seen pixels whose observation is a number (its k-fold path
 * drops the rows with a NaN observation, calibration.py:896-901): a fold draw returns what
 * mod16_et_static_batch_* (MOD16_MATH_FAST) returns on the compacted seen rows, up to summation
 * order. Plain calls on the problem are unchanged, bit for bit, labels or not.
 *   mod16_static_batch_set_folds        labels [n] (HOST). Once per problem, before any sampler
 *       exists on it; the problem must be float64, MOD16_MATH_FAST, bound with observations.
 *   mod16_static_batch_objective_folds  as mod16_static_batch_objective, code [ndraw] (HOST): folds
 *       and modes may differ between the draws of one call. Plain and fold calls keep a captured
 *       graph each.
 * Anything else is MOD16_ERR_ARG with a message (mod16_last_error).
 */
#define MOD16_FOLD_HELDOUT 0x100
MOD16_API int mod16_static_batch_set_folds(mod16_batch* problem, const uint8_t* labels, int nfolds);
MOD16_API int mod16_static_batch_objective_folds(mod16_batch* problem, const void* params, int64_t ndraw,
                        const int32_t* code, double* sse, double* count);

/*
 * The annual-precipitation constraint on a resident problem (ABI 9; the reference's constrain_by_map,
 * mod16/calibration.py:776-796). The problem is T days x N sites, pixel t N + s; day t belongs to
 * year year_index[t] in 0 .. Y - 1; annual_precip [Y][N] in mm per year; lhv [T][N] in J kg-1. For a
 * parameter row with le = the row's ET in W m-2 (every pixel, observed or not):
 *   mass = max(le 86400 / lhv, 0), tot[y][s] = its sum over the days of year y,
 *   over = max(tot - annual_precip, 0), penalty = -100 mean(over^2) / sum(annual_precip)
 * both max keeping a NaN: penalty <= 0, or NaN. float64, sums in a fixed order (the same bits on every
 * launch), no array of size draws x n.
 *   mod16_static_batch_set_annual        once per problem, before any objective call or sampler: a
 *       float64 MOD16_MATH_FAST problem bound from MOD16_HOST arrays with observations, without
 *       folds, n = T N; every year index used; annual_precip finite with a sum > 0; lhv finite and
 *       > 0. The resident copies are laid out anew, site-year by site-year, each padded to a multiple
 *       of 64 pixels (so device memory grows by up to 63 pixels per site-year, plus 8 bytes per
 *       pixel); n of mod16_static_batch_info, the rows of mod16_static_batch_rows and the (sse,
 *       count) of mod16_static_batch_objective stay the caller's (sse up to summation order).
 *   mod16_static_batch_objective_annual  as mod16_static_batch_objective, and penalty [ndraw]; one
 *       graph launch, its own cached graph.
 * Not combined with folds (the reference's own combination cannot run: its closure indexes a (T,)
 * mask into ravelled, compacted rows). Anything else is MOD16_ERR_ARG with a message; memory that
 * cannot be had is MOD16_ERR_NOMEM and leaves the problem as it was.
 */
MOD16_API int mod16_static_batch_set_annual(mod16_batch* problem, int64_t T, int64_t N, const int32_t* year_index,
                        int Y, const double* annual_precip, const double* lhv);
MOD16_API int mod16_static_batch_objective_annual(mod16_batch* problem, const void* params, int64_t ndraw,
                        double* sse, double* count, double* penalty);

/*
 * DE-MCMC-Z calibration sampler (ABI 7; mod16_amd/calibration.py): independent chains of PyMC's
 * DEMetropolisZ -- the project's restatement of it, stated in full at the top of
 * mod16_amd/csrc/mod16_mcmc.hpp -- over the free parameters of a RESIDENT problem
 * (mod16_static_batch_bind_f64), with proposals, priors, the likelihood, the Metropolis decision,
 * tuning and the history in device memory. One lane per chain; K = `segment` steps (propose ->
 * the problem's objective launches -> accept, on the problem's stream, a single chain of nodes) are
 * captured as one graph and replayed; the step counter lives on the device, so every replay is the
 * same graph. Steps that do not fill a K run as one more graph of the remainder.
 *
 *   mod16_mcmc_create   problem: float64, bound with MOD16_MATH_FAST and with observations;
 *       spec->chains <= the problem's max_draws. x0: NULL (every chain starts at the priors'
 *       support points: Uniform the midpoint, LogNormal exp(mu + s^2/2), Triangular (a + b + c) / 3)
 *       or [chains][nfree] x-values inside the supports. Evaluates the initial log posterior;
 *       one that is not finite is MOD16_ERR_ARG.
 *   mod16_mcmc_run      `steps` more steps of every chain (synchronous). ms, if not NULL: the GPU
 *       time of the graphs (HIP events).
 *   mod16_mcmc_read     steps [t0, t0 + count) of the trace, each output optional:
 *       x, y [count][chains][nfree] (x-values, sampler y-values), loglik, logpost [count][chains],
 *       accepted [count][chains] (0 / 1); and the current per-chain scaling, lamb [chains] and the
 *       number of steps taken so far. t0 + count <= steps taken.
 *   mod16_mcmc_destroy  frees the sampler; destroy every sampler of a problem before the problem.
 *   mod16_mcmc_create_groups  (ABI 8) cross-validation in one sampler: spec->chains chains for each
 *       of the `ngroups` distinct folds fold[g] of a problem with labels (mod16_static_batch_set_folds),
 *       chains x ngroups <= max_draws. Chain j of group g is chain g * chains + j of x0, of the trace
 *       and of every per-chain output; it evaluates its objective with the TRAIN code fold[g], and its
 *       random stream is the plain sampler's with seed (seed + fold[g]) mod 2^64 and chain index j
 *       (mod16_mcmc.hpp) -- so its draws do not depend on which other groups run alongside.
 * Checks (MOD16_ERR_ARG): 1 <= nfree <= 11 distinct columns; Uniform / Triangular lower < upper,
 * lower <= c <= upper, LogNormal sigma > 0, all finite; tune_target 0 (none), 1 (scaling), 2 (lamb);
 * tune_interval >= 1; tune_steps >= 0; 0 <= tune_drop_fraction < 1; objective 0 (rmsd:
 * loglik = -sqrt(sse / count)) or 1 (gaussian: -sse / 2); lamb, scaling finite; segment 0 (64) or
 * 1 .. 1024. Device memory: about 8 (2 nfree + 2) + 1 bytes per chain and step taken (history and
 * trace, grown by each run -- the graphs are captured again then), plus the objective's workspace
 * for `chains` draws; what cannot be had is MOD16_ERR_NOMEM. Calls hold the problem's ctx mutex.
 * spec->constraints (ABI 9): MOD16_CONSTRAINT_ANNUAL_PRECIP on a problem with
 * mod16_static_batch_set_annual adds the row's penalty to the log-likelihood of either objective (the
 * trace's loglik includes it; a NaN penalty rejects the step, and an initial point with one is
 * MOD16_ERR_ARG); the sampler's graphs then hold the constrained launches. With folds
 * (mod16_mcmc_create_groups), on a problem without the constraint, or with unknown bits:
 * MOD16_ERR_ARG. 0 is a sampler without constraint, on any problem.
 */
#define MOD16_CONSTRAINT_ANNUAL_PRECIP 1
enum mod16_prior { MOD16_PRIOR_UNIFORM = 0, MOD16_PRIOR_LOGNORMAL = 1, MOD16_PRIOR_TRIANGULAR = 2 };
typedef struct mod16_mcmc_spec {
    int32_t chains;
    int32_t nfree;
    int32_t index[11];          /* column of free parameter i (mod16_param order), ascending */
    int32_t family[11];         /* enum mod16_prior */
    double p0[11], p1[11], p2[11];   /* (lower, upper, -) / (mu, sigma, -) / (lower, upper, c) */
    double fixed[11];           /* the parameter row; free columns are ignored */
    double lamb, scaling;
    int32_t tune_target;
    int32_t tune_interval;
    int64_t tune_steps;
    double tune_drop_fraction;
    int32_t objective;
    int32_t segment;
    uint64_t seed;
    int32_t constraints;        /* (ABI 9) bits of MOD16_CONSTRAINT_*; 0: none */
    int32_t reserved_;          /* 0 */
} mod16_mcmc_spec;
typedef struct mod16_mcmc mod16_mcmc;
MOD16_API int mod16_mcmc_create(mod16_batch* problem, const mod16_mcmc_spec* spec, const double* x0,
                                mod16_mcmc** out);
MOD16_API int mod16_mcmc_create_groups(mod16_batch* problem, const mod16_mcmc_spec* spec, int ngroups,
                                       const int32_t* fold, const double* x0, mod16_mcmc** out);
MOD16_API int mod16_mcmc_run(mod16_mcmc* sampler, int64_t steps, float* ms);
MOD16_API int mod16_mcmc_read(mod16_mcmc* sampler, int64_t t0, int64_t count, double* x, double* y,
                              double* loglik, double* logpost, uint8_t* accepted, double* scaling,
                              double* lamb, int64_t* steps_taken);
MOD16_API int mod16_mcmc_destroy(mod16_mcmc* sampler);

/*
 * Waits for the ctx's outstanding work on `stream` and reports deferred
 * errors of DEVICE-mode calls (MOD16_ERR_CLASS_RANGE, MOD16_ERR_HIP).
 */
MOD16_API int mod16_check_status(mod16_ctx* ctx, void* stream);

/*
 * Diagnostics of a (day, night) result pair [n] (device pointers): a
 * deterministic two-level tree sum in fixed order. diag (host, 8 doubles) =
 * { sum_day, sum_night, n_finite_day, n_finite_night, n_nan_day, n_nan_night,
 *   max_day, max_night }, NaN pixels skipped as np.nansum would. Synchronous.
 * ddiag (device, 8 doubles, may be NULL) receives the same vector
 * asynchronously for an RCCL all-reduce without a host round trip; pass
 * diag == NULL to stay asynchronous.
 */
MOD16_API int mod16_reduce_diag_f64(mod16_ctx* ctx, const double* day,
                          const double* night, int64_t n, double* diag,
                          double* ddiag, void* stream);
MOD16_API int mod16_reduce_diag_f32(mod16_ctx* ctx, const float* day,
                          const float* night, int64_t n, double* diag,
                          double* ddiag, void* stream);

/*
 * On-device synthetic driver fields: fills the class
 * raster and the 14 dense driver arrays (device pointers, n elements each)
 * for global pixel indices [pixel_offset, pixel_offset + n) of time step
 * `step` from a counter-based generator keyed on (seed, step, variable,
 * pixel), so any tiling of a raster over any number of GPUs sees the same
 * field. Asynchronous on `stream`.
 */
MOD16_API int mod16_synth_f64(mod16_ctx* ctx, uint64_t seed, int64_t step,
                    int64_t pixel_offset, int64_t n, uint8_t* cls,
                    double* const* drivers, void* stream);
MOD16_API int mod16_synth_f32(mod16_ctx* ctx, uint64_t seed, int64_t step,
                    int64_t pixel_offset, int64_t n, uint8_t* cls,
                    float* const* drivers, void* stream);

/*
 * Timing aid for bench.py: runs `launches` back-to-back launches of the
 * DEVICE-mode f64/f32 forward run on `stream`, bracketed by HIP events on
 * that stream, and returns the mean milliseconds per launch in *ms.
 * Arguments as mod16_et_f64 / mod16_et_f32 (is_f32 selects), where = DEVICE;
 * with ddiag != NULL the launches are those of mod16_et_diag_*.
 */
MOD16_API int mod16_time_et(mod16_ctx* ctx, int is_f32, const uint8_t* cls,
                  const void* const* drivers, const int64_t* dstride,
                  const void* const* params, const int64_t* pstride,
                  int64_t n, void* out_day, void* out_night,
                  void* const* out_sep, unsigned flags, double* ddiag,
                  int launches, void* stream, float* ms);

/*
 * Tiled rasters: the engine's own layout for rasters that stay resident on the
 * device (DEVICE pointers only). The reference passes 16 separate arrays
 * (14 drivers, day, night); streamed side by side they lie GiB apart in HBM and
 * the 14-read + 2-write mix reaches 5.7 TB/s. Cut into tiles of `tile` pixels
 * and interleaved -- [tile][field][tile pixels], every array keeps its own base
 * pointer and reads as a 2-D strided view -- the same bytes stream at 6.5 TB/s
 * (tools/probe_layout.hip, tile = 32-64 KiB per field). Pixel i of an array:
 *
 *     base[(i / tile) * row + (i % tile)]
 *
 * `tile` is a power of two (>= 8 KiB per field); `driver_row`, `out_row` are in
 * elements and apply to every driver / output array, `cls_row` in bytes to the
 * class raster; rows are multiples of the 16-byte vector width, bases 16-byte
 * aligned, n a multiple of the vector width (the storage is padded to whole
 * tiles by whoever allocates it). tile = 0 in mod16_synth_tiled_* means plain
 * arrays. mod16_et_tiled_* = mod16_et_diag_* on that layout (ddiag may be NULL;
 * MOD16_MATH_FAST or, float32, MOD16_MATH_MIXED); mod16_graph_et_tiled_* captures
 * it for replay with mod16_graph_launch. Host arrays reach the layout with 2-D
 * copies (hipMemcpy2DAsync, width = tile, destination pitch = row).
 * Limits of one pipeline launch (any layout; MOD16_ERR_ARG beyond them): 2^30
 * pieces of 64 vectors -- 1.4e11 float64 or 2.7e11 float32 pixels, three orders of
 * magnitude above what 288 GB hold -- and rows below 2^32 elements: the kernel
 * keeps its piece numbers and tile offsets in single 32-bit scalar registers.
 */
typedef struct mod16_layout {
    int64_t tile;        /* pixels per tile */
    int64_t driver_row;  /* elements between successive tiles of a driver array */
    int64_t out_row;     /* elements between successive tiles of an output array */
    int64_t cls_row;     /* bytes between successive tiles of the class raster */
} mod16_layout;
MOD16_API int mod16_et_tiled_f64(mod16_ctx* ctx, const mod16_layout* layout,
                       const uint8_t* cls, const double* const* drivers, int64_t n,
                       double* out_day, double* out_night, unsigned flags,
                       double* ddiag, void* stream);
MOD16_API int mod16_et_tiled_f32(mod16_ctx* ctx, const mod16_layout* layout,
                       const uint8_t* cls, const float* const* drivers, int64_t n,
                       float* out_day, float* out_night, unsigned flags,
                       double* ddiag, void* stream);
MOD16_API int mod16_graph_et_tiled_f64(mod16_ctx* ctx, const mod16_layout* layout,
                       const uint8_t* cls, const double* const* drivers, int64_t n,
                       double* out_day, double* out_night, unsigned flags,
                       double* ddiag, mod16_graph** out);
MOD16_API int mod16_graph_et_tiled_f32(mod16_ctx* ctx, const mod16_layout* layout,
                       const uint8_t* cls, const float* const* drivers, int64_t n,
                       float* out_day, float* out_night, unsigned flags,
                       double* ddiag, mod16_graph** out);
MOD16_API int mod16_synth_tiled_f64(mod16_ctx* ctx, const mod16_layout* layout,
                       uint64_t seed, int64_t step, int64_t pixel_offset, int64_t n,
                       uint8_t* cls, double* const* drivers, void* stream);
MOD16_API int mod16_synth_tiled_f32(mod16_ctx* ctx, const mod16_layout* layout,
                       uint64_t seed, int64_t step, int64_t pixel_offset, int64_t n,
                       uint8_t* cls, float* const* drivers, void* stream);

/*
 * The other forms of the forward run on a tiled raster -- what mod16_et_pet_*,
 * mod16_et_* with out_sep and mod16_et_raw_* compute on plain arrays, on the
 * layout above (device pointers, MOD16_MATH_FAST or, float32, MOD16_MATH_MIXED;
 * asynchronous on `stream`). `wide`: the form's driver arrays (driver_row applies to
 * each), `bytes`: its byte rasters (cls_row applies to each), `outs`: its outputs
 * (out_row applies to each); every array of the form is required:
 *
 *   form                          wide                      bytes                     outs
 *   MOD16_FORM_TOTALS             14 drivers                cls                       day, night
 *   MOD16_FORM_PET                14 drivers                cls                       day, night, pet day, pet night
 *   MOD16_FORM_COMPONENTS         14 drivers                cls                       canopy, soil, transpiration (day), then (night)
 *   MOD16_FORM_TOTALS_COMPONENTS  14 drivers                cls                       day, night, then the six components
 *   MOD16_FORM_RAW                14 raw (mod16_raw_driver) cls, fpar_pct, lai_x10    day, night
 *   MOD16_FORM_RAW_TOTAL8         14 raw                    cls, fpar_pct, lai_x10    day, night, total8 (day_hours: one value)
 *   MOD16_FORM_RAW_TOTAL8_HOURS   14 raw + hours of daylight cls, fpar_pct, lai_x10   day, night, total8
 *
 * mod16_form_shape() returns the three counts of a form.
 */
enum mod16_form {
    MOD16_FORM_TOTALS = 0, MOD16_FORM_PET, MOD16_FORM_COMPONENTS, MOD16_FORM_TOTALS_COMPONENTS,
    MOD16_FORM_RAW, MOD16_FORM_RAW_TOTAL8, MOD16_FORM_RAW_TOTAL8_HOURS
};
MOD16_API int mod16_form_shape(int form, int* n_wide, int* n_bytes, int* n_out);
MOD16_API int mod16_et_form_tiled_f64(mod16_ctx* ctx, const mod16_layout* layout, int form,
                       const uint8_t* const* bytes, const double* const* wide,
                       double* const* outs, double day_hours, int64_t n,
                       unsigned flags, void* stream);
MOD16_API int mod16_et_form_tiled_f32(mod16_ctx* ctx, const mod16_layout* layout, int form,
                       const uint8_t* const* bytes, const float* const* wide,
                       float* const* outs, double day_hours, int64_t n,
                       unsigned flags, void* stream);

/* mod16_time_et for a tiled raster: `launches` back-to-back direct (not captured)
 * launches of mod16_et_tiled_*, HIP events on `stream`, mean milliseconds per launch.
 * For steps shorter than a graph replay's fixed cost (a 1200 x 1200 tile) this is
 * the faster way to issue them, and how bench.py times configs[1]. */
MOD16_API int mod16_time_et_tiled(mod16_ctx* ctx, int is_f32, const mod16_layout* layout,
                       const uint8_t* cls, const void* const* drivers, int64_t n,
                       void* out_day, void* out_night, unsigned flags, double* ddiag,
                       int launches, void* stream, float* ms);

/* Mean milliseconds per replay of a captured step: `launches` back-to-back
 * mod16_graph_launch calls bracketed by HIP events on `stream`. Synchronous. */
MOD16_API int mod16_time_graph(mod16_graph* graph, int launches, void* stream, float* ms);

/*
 * Page-locked host memory for the arrays a HOST-mode call writes its results to.
 * The reference returns freshly allocated arrays (mod16/__init__.py:789-793); a
 * device-to-host copy into fresh pageable memory is bound by the kernel's
 * page-fault rate (13 GB/s measured), into page-locked memory by PCIe (57 GB/s).
 * The Python layer keeps a bounded pool of such blocks behind the numpy arrays
 * it returns. Not tied to a ctx; thread-safe.
 */
MOD16_API int mod16_host_alloc(int64_t bytes, void** out);
MOD16_API int mod16_host_free(void* p);

/*
 * Measurement aid for bench.py ("roofline vs measured
 * copy bandwidth"): allocates two device buffers of `bytes`, times a one-shot
 * 16-byte-per-lane copy kernel `reps` times with HIP events and returns the
 * best rate, (bytes read + bytes written) / time, in GB/s. Synchronous.
 */
MOD16_API int mod16_measure_copy(mod16_ctx* ctx, int64_t bytes, int reps, float* gbps);

/*
 * Identity of this build: a hex digest of the library's sources and compiler flags, put in
 * by mod16_amd/csrc/build.py. profiles/ records of a kernel (HBM traffic from the PMC passes)
 * carry it, and bench.py reports such a record only for the build it was measured on.
 */
MOD16_API const char* mod16_build_id(void);

/*
 * The rank-order fold behind the all-gather of the diagnostics vectors: `gathered`
 * is [world][8] float64 on the device (rank r's vector at row r), `diag` [8] receives sums and
 * counts [0..5] added in rank order (rank 0 + rank 1 + ...: the same bits on every rank and
 * from run to run) and the maxima [6..7]. One small kernel, asynchronous on `stream`.
 */
MOD16_API int mod16_fold_diag(mod16_ctx* ctx, const double* gathered, int world, double* diag,
                              void* stream);

/*
 * Parameter rasters -> class raster (round 6). The reference's multi-class idiom gathers the BPLUT
 * per pixel -- MOD16({k: bplut[k][pft_map]}), mod16/utils.py:81-117 and notebook cell 32 -- and hands
 * evapotranspiration() eleven parameter rasters that hold, pixel for pixel, one of at most 13 rows.
 * mod16_classify_* turns DEVICE rasters of that kind back into a class raster: params[11] (order of
 * MOD16.required_parameters) with pstride 1 (a raster of n values) or 0 (one value); `rows` a HOST
 * array [nrows][11] of candidate rows, 1 <= nrows <= 13; every pixel whose eleven values equal a row
 * bit for bit (a NaN row matches itself) gets that row's index in cls[n] (device). *unmatched
 * receives -1 if every pixel matched, else the smallest index of a pixel that matched no row (the
 * caller adds that pixel's row and calls again, or gives up: the rasters are not a gather of <= 13
 * rows). Waits for `stream`. What the Python layer does with it: MOD16.evapotranspiration on device
 * tensors with per-pixel parameter tensors takes the production pipeline (14 drivers + 1 byte per
 * pixel) instead of the plain kernel (25 arrays).
 */
MOD16_API int mod16_classify_f64(mod16_ctx* ctx, const double* const* params, const int64_t* pstride,
                                 int64_t n, const double* rows, int nrows, uint8_t* cls,
                                 int64_t* unmatched, void* stream);
MOD16_API int mod16_classify_f32(mod16_ctx* ctx, const float* const* params, const int64_t* pstride,
                                 int64_t n, const float* rows, int nrows, uint8_t* cls,
                                 int64_t* unmatched, void* stream);

/*
 * Sobol sensitivity analysis (ABI 6; mod16_amd/sensitivity.py): what the reference's
 * sensitivity.py does with SALib, on the device. float64 only. The arithmetic -- the Sobol
 * sequence, the Saltelli row layout, the indices and the bootstrap's index generator -- is stated
 * in full at the top of mod16_amd/csrc/mod16_sobol.hpp; in short:
 *   - the sequence is the unscrambled Sobol sequence of scipy.stats.qmc.Sobol(2d, scramble=False,
 *     bits=32) (Joe-Kuo direction numbers, 32 dimensions committed as constants), point skip + j for
 *     base sample j; a value is lo + (hi - lo) * u (no contraction);
 *   - a base sample has R = 2d + 2 rows (second_order) or d + 2: A, AB^(1..d), [BA^(1..d)], B --
 *     SALib's documented layout (not checked against SALib itself);
 *   - idx_out and std_out are [S1 d | ST d | S2 d*d] (S2[j][k] for j < k, NaN elsewhere and without
 *     second order); std_out is the standard deviation (ddof 1) of each index over `resamples`
 *     bootstrap resamples of the n base samples (multiply by the normal quantile for a confidence
 *     half-width); NaN in y propagates.
 * Checks (MOD16_ERR_ARG): 1 <= d <= 14; n a power of two, n <= 2^26; lo < hi, both finite;
 * 0 <= skip, skip + n <= 2^32; vary[d] distinct driver indices (enum mod16_driver);
 * 0 <= resamples <= 2^20. Device memory that cannot be had is MOD16_ERR_NOMEM.
 * where = MOD16_HOST: the arrays are host memory, the call is synchronous; MOD16_DEVICE: device
 * memory, asynchronous on `stream`.
 *
 *   mod16_sobol_sample_f64   the sample: out[n*R][d] row-major (the rows SALib's sample() returns).
 *   mod16_sobol_rows_f64     sample, MOD16._et and output in one kernel: y[n][R] = day + night
 *       (W m-2) of each row, evaluated as MOD16._et(params, *row) with scalars -- the reference's
 *       operation order (MOD16_MATH_EXACT), and the whole-array switch any(g_surf > 0) decided per
 *       row. Driver vary[s] takes column s of the sample; the others take base[14] (all 14 given,
 *       mod16_driver order); params[11] in mod16_param order. Nothing but y is written.
 *   mod16_sobol_analyze_f64  y[n][R] -> indices and bootstrap spreads; `normalize`: y is first
 *       standardised over all n*R values (SALib's step). Sums are in a fixed order, without
 *       floating-point atomics: two calls give the same bits. Device memory: about
 *       8 * ((resamples + 1) * (nchunks * m(m+1)/2 + 2d + d^2)) bytes of workspace (m = 3 + 2d with
 *       second order, 3 + d without; nchunks about 1024 / (resamples + 1)), plus y in HOST mode.
 */
MOD16_API int mod16_sobol_sample_f64(mod16_ctx* ctx, int d, const double* lo, const double* hi,
                                     int64_t n, int64_t skip, int second_order, double* out,
                                     int where, void* stream);
MOD16_API int mod16_sobol_rows_f64(mod16_ctx* ctx, const double* params, const double* base,
                                   const int* vary, const double* lo, const double* hi, int d,
                                   int64_t n, int64_t skip, int second_order, double* y, int where,
                                   void* stream);
MOD16_API int mod16_sobol_analyze_f64(mod16_ctx* ctx, const double* y, int d, int64_t n,
                                      int second_order, int normalize, int resamples, uint64_t seed,
                                      double* idx_out, double* std_out, int where, void* stream);

/*
 * Ensemble forward run (ABI 10; mod16_amd.evapotranspiration_ensemble, RasterEngine.ensemble):
 * MOD16.evapotranspiration for `members` parameter tables over one raster, reduced per pixel to
 * the mean and the spread over the members. One kernel reads each pixel's drivers and class once,
 * evaluates every member (the pixel's class picks its row in every table) and writes five arrays;
 * nothing of size members x n exists, there are no atomics, two calls give the same bits.
 *
 *   function                 what it does
 *   mod16_ensemble_create    tables[members][13][11] (HOST, float64, mod16_param column order) ->
 *                            an ensemble on the ctx's device: the derived tables of
 *                            mod16_set_bplut_f64, one per member, uploaded once (2 KiB each).
 *                            MOD16_ERR_ARG unless 1 <= members <= 65536:
 *                            "mod16_ensemble_create: members must be between 1 and 65536"
 *   mod16_ensemble_destroy   frees it (NULL is fine); the ctx may be gone already
 *   mod16_et_ensemble_f64    cls[n], drivers[14] with dstride[14] = 0 (broadcast scalar) / 1 (dense),
 *   mod16_et_ensemble_f32    as mod16_et_*; out[5], all required, each [n]:
 *                              out[0] mean_day    mean over the members of the day total
 *                              out[1] mean_night  ... of the night total
 *                              out[2] std_day     standard deviation (ddof = 0) of the day total
 *                              out[3] std_night   ... of the night total
 *                              out[4] std_total   ... of day + night (its mean is out[0] + out[1])
 *
 *   flags   MOD16_MATH_FAST (default): every member with the FAST float64 arithmetic, the part of it
 *           that depends on the drivers alone computed once per pixel; pixels outside its domain
 *           (the test of MOD16_MATH_FAST above) have ALL their members computed in the reference's
 *           operation order. MOD16_MATH_EXACT: every pixel that way. Refused (MOD16_ERR_ARG):
 *           "MOD16_MATH_MIXED is not available for the ensemble run" and
 *           "MOD16_DOMAIN_TRUSTED is not available for the ensemble run".
 *   float32 data: float64 arithmetic and accumulation under either flag, one rounding on store.
 *   sums    sequential in member order, float64, one pass, shifted by member 0: identical tables give
 *           a spread of exactly 0 and the mean of a one-member ensemble, bit for bit.
 *   NaN     a member's NaN (classes without parameters, a NaN driver, a NaN row in ONE table) makes
 *           that period's mean and spread and std_total NaN; an infinite member value leaves them
 *           non-finite (which non-finite value is not specified).
 *   class   a code >= 13 gives NaN and MOD16_ERR_CLASS_RANGE -- from the call with where =
 *           MOD16_HOST, from mod16_check_status after a MOD16_DEVICE call.
 *   where   MOD16_DEVICE: device pointers, asynchronous on `stream`; MOD16_HOST: host arrays, the
 *           shared staging path of the other pixel-wise families (small calls copy-free, larger ones
 *           in tiles of mod16_host_tile_pixels()), synchronous; the same kernel, the same bits.
 */
typedef struct mod16_ensemble mod16_ensemble;
MOD16_API int mod16_ensemble_create(mod16_ctx* ctx, const double* tables, int64_t members,
                                    mod16_ensemble** out);
MOD16_API int mod16_ensemble_destroy(mod16_ensemble* ensemble);
MOD16_API int mod16_et_ensemble_f64(mod16_ctx* ctx, const mod16_ensemble* ensemble, const uint8_t* cls,
                                    const double* const* drivers, const int64_t* dstride, int64_t n,
                                    double* const* out, unsigned flags, int where, void* stream);
MOD16_API int mod16_et_ensemble_f32(mod16_ctx* ctx, const mod16_ensemble* ensemble, const uint8_t* cls,
                                    const float* const* drivers, const int64_t* dstride, int64_t n,
                                    float* const* out, unsigned flags, int where, void* stream);

/*
 * Per-member outputs and per-pixel quantiles of the ensemble run (ABI 11;
 * mod16_amd.evapotranspiration_ensemble_quantiles, EnsembleRun.quantiles / .run_members). The
 * definition of the quantiles is the numpy statement mod16_amd.calibration.ensemble_quantile (numpy's
 * default 'linear' method): with h = q (members - 1) in float64, lo = floor(h), frac = h - lo and s the
 * members in ascending order, a = s[lo], b = s[min(lo + 1, members - 1)], the value is a where
 * frac == 0 or a == b, else a + frac (b - a) (multiply, then add; no contraction).
 *
 *   function                          what it does
 *   mod16_et_ensemble_members_f64     every member's day and night total: day[m * pitch + i],
 *   mod16_et_ensemble_members_f32     night[m * pitch + i] for member m and pixel i, pitch >= n
 *                                     ("mod16_et_ensemble_members: pitch must be at least n").
 *                                     MOD16_DEVICE only: device pointers, asynchronous on `stream`.
 *                                     Row m holds the bits mean_day / mean_night of the one-member
 *                                     ensemble of table m have.
 *   mod16_et_ensemble_quantiles_f64   nq quantiles q[0..nq) (HOST doubles) of three series per pixel:
 *   mod16_et_ensemble_quantiles_f32   the day total, the night total, and day + night (summed per
 *                                     member in float64 before ordering). out[3 * nq], series-major,
 *                                     all required, each [n]: out[k] day at q[k], out[nq + k] night,
 *                                     out[2 nq + k] total.
 *
 *   slab        The member values of P pixels at a time pass through a stream-ordered temporary of
 *               members x P x 2 doubles (never members x n): P = slab_bytes / (16 members) rounded down
 *               to a multiple of 256, at least 256, at most n rounded up to one. slab_bytes = 0: 128 MiB;
 *               a slab below one 256-pixel batch is raised to one; slab_bytes < 0 is MOD16_ERR_ARG
 *               ("mod16_et_ensemble_quantiles: slab_bytes must not be negative"). The result does not
 *               depend on it. MOD16_HOST: one slab per staging slot, on that slot's stream.
 *   selection   one pixel per lane, the pixel's members ordered in LDS by a bitonic network (exact
 *               order statistics, no atomics, two calls give the same bits); LDS is static, one
 *               instance per capacity of 16, 32, 64, 128, 256 members (8 ... 128 KiB).
 *   float32     member values, their sum, the ordering and the interpolation in float64, one rounding
 *               on store.
 *   NaN         a NaN member makes all nq values of that pixel and series NaN. Infinite members follow
 *               the rule above: equal infinities stay, a position that falls on a finite member gives
 *               that member, an interpolation between -inf and a finite value or +inf is NaN.
 *   flags, class, where (quantiles)   as mod16_et_ensemble_*.
 *   refused (MOD16_ERR_ARG)
 *               "mod16_et_ensemble_quantiles: nq must be between 1 and 8"
 *               "mod16_et_ensemble_quantiles: every q must lie in [0, 1] and not be NaN"
 *               "mod16_et_ensemble_quantiles: more than 256 members" (mod16_ensemble_create itself
 *               takes up to 65536; the other calls serve them)
 *               "MOD16_MATH_MIXED is not available for the ensemble run" and
 *               "MOD16_DOMAIN_TRUSTED is not available for the ensemble run" (both calls)
 *               "the ensemble was created on another device than this context's" (both calls)
 */
MOD16_API int mod16_et_ensemble_members_f64(mod16_ctx* ctx, const mod16_ensemble* ensemble, const uint8_t* cls,
                                            const double* const* drivers, const int64_t* dstride, int64_t n,
                                            double* day, double* night, int64_t pitch, unsigned flags,
                                            void* stream);
MOD16_API int mod16_et_ensemble_members_f32(mod16_ctx* ctx, const mod16_ensemble* ensemble, const uint8_t* cls,
                                            const float* const* drivers, const int64_t* dstride, int64_t n,
                                            float* day, float* night, int64_t pitch, unsigned flags,
                                            void* stream);
MOD16_API int mod16_et_ensemble_quantiles_f64(mod16_ctx* ctx, const mod16_ensemble* ensemble, const uint8_t* cls,
                                              const double* const* drivers, const int64_t* dstride, int64_t n,
                                              const double* q, int nq, double* const* out, int64_t slab_bytes,
                                              unsigned flags, int where, void* stream);
MOD16_API int mod16_et_ensemble_quantiles_f32(mod16_ctx* ctx, const mod16_ensemble* ensemble, const uint8_t* cls,
                                              const float* const* drivers, const int64_t* dstride, int64_t n,
                                              const double* q, int nq, float* const* out, int64_t slab_bytes,
                                              unsigned flags, int where, void* stream);

/*
 * Multi-day ET composites (ABI 12; mod16_amd.evapotranspiration_composite, RasterEngine.composite):
 * per-pixel period totals [kg m-2 per period] of MOD16.evapotranspiration over `days` days of
 * drivers in one launch -- MOD16A2 is the 8-day sum of daily ET, MOD16A3 the annual one. The
 * definition is the numpy statement mod16_amd/composite.py (daily_total, composite_reduce):
 *
 *   periods     K = days (1 ... 4096), L = period_days >= 1: period p covers days [p L, min((p + 1) L, K));
 *               P = ceil(K / L) periods, the last may be short.
 *   arrays      each of the 14 drivers, and day_hours (hours of daylight), has a pixel stride (1: one
 *               value per pixel; 0: one value, constant in time), a divisor every >= 1 and a time
 *               stride in elements: day t reads time slab t / every, which starts time_stride
 *               elements behind the previous one; ceil(K / every) slabs. An array with one slab
 *               (every >= K) is constant and its time stride is not looked at.
 *   daily total v_t = (day_t * h_t * 3600.0) + (night_t * (24.0 - h_t) * 3600.0), left to right, no
 *               contraction; day_t / night_t are what mod16_et_* gives for day t's drivers [kg m-2 s-1];
 *               with out_pet the same formula on the potential-ET pair of mod16_et_pet_*.
 *   result      day t is valid where v_t is not NaN; count_p = valid days of period p (uint16);
 *               sum_p = the float64 sum in day order of the valid v_t, from +0.0 (infinities take
 *               part); the result is NaN where count_p < min_valid (1 ... L), else sum_p, or with
 *               rescale = 1 sum_p * ((double)len_p / (double)count_p). ET and PET have their own counts.
 *   outputs     out_et[p * out_pitch + i] for period p and pixel i, out_pitch >= n; optional out_pet
 *               likewise; optional count_et / count_pet (uint16, the same pitch in elements;
 *               count_pet needs out_pet).
 *   float32     inputs widened, arithmetic and accumulation in float64, one rounding on store.
 *   flags       MOD16_MATH_FAST (0) or MOD16_MATH_EXACT; the fast instance tests every pixel-day
 *               against the domain of its arithmetic and a second kernel behind it recomputes the
 *               periods of the pixels with a flagged day (the flagged days in the reference's
 *               operation order): the daily values have the bits of mod16_et_* / mod16_et_pet_*
 *               with the same flags on that day's drivers. No atomics on results, no workspace:
 *               two calls give the same bits.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream` (mod16_check_status reports a
 *               class code >= 13). MOD16_HOST: host pointers; pixel tiles are staged through the
 *               context's slabs -- every time slab of every array, one copy per slab and tile -- with
 *               the tile cut so that a slot's slab fits stage_bytes (0: 128 MiB; at least one batch of
 *               256 pixels is taken). The result does not depend on stage_bytes.
 *               A year of daily float64 drivers (days = 368, 3900 slabs and periods) gets tiles of 4096
 *               pixels from the default; more stage_bytes, larger copies.
 *               every >= days means one slab; it is used as days.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_et_composite: ...")
 *               "days must be between 1 and 4096", "period_days must be at least 1",
 *               "min_valid must be between 1 and period_days", "rescale must be 0 or 1",
 *               "pixel stride must be 0 or 1", "every must be at least 1",
 *               "time stride must not be negative",
 *               "a broadcast scalar (pixel stride 0) is constant in time: its every must be at least days",
 *               "time stride of an array with several slabs must be at least n",
 *               "out_pitch must be at least n", "count_pet needs out_pet",
 *               "stage_bytes must not be negative", a NULL array, n < 0, an unknown flag,
 *               "MOD16_MATH_MIXED is not available for the composite run" and
 *               "MOD16_DOMAIN_TRUSTED is not available for the composite run".
 *               n = 0 is MOD16_OK.
 */
typedef struct mod16_composite_spec {
    int64_t n;                                   /* pixels */
    int32_t days, period_days, min_valid, rescale;
    int64_t pixel_stride[MOD16_N_DRIVERS];       /* 0 or 1 */
    int64_t time_stride[MOD16_N_DRIVERS];        /* elements between two time slabs */
    int32_t every[MOD16_N_DRIVERS];              /* day t reads slab t / every */
    int64_t hours_pixel_stride, hours_time_stride;   /* the same three for day_hours */
    int32_t hours_every;
    int32_t reserved_;
} mod16_composite_spec;
MOD16_API int mod16_et_composite_f64(mod16_ctx* ctx, const mod16_composite_spec* spec, const uint8_t* cls,
                                     const double* const* drivers, const double* day_hours, double* out_et,
                                     double* out_pet, uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch,
                                     unsigned flags, int where, void* stream, int64_t stage_bytes);
MOD16_API int mod16_et_composite_f32(mod16_ctx* ctx, const mod16_composite_spec* spec, const uint8_t* cls,
                                     const float* const* drivers, const float* day_hours, float* out_et,
                                     float* out_pet, uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch,
                                     unsigned flags, int where, void* stream, int64_t stage_bytes);

/*
 * QC-driven temporal gap filling of byte series (ABI 13; mod16_amd.gapfill_series,
 * RasterEngine.gapfill): the step between MOD15A2H granules and the fPAR / LAI series the raw and
 * composite entry points take. One launch fills the annual profile of every pixel of one to three
 * fields. The definition is the numpy statement mod16_amd/gapfill.py (reliable, fill_series, encode):
 *
 *   inputs      fields[f][t * in_pitch + i]: the code of field f, slab t (0 ... slabs - 1, slabs
 *               1 ... 4096), pixel i; optional qc[t * qc_pitch + i], one QC byte shared by the fields;
 *               optional good256[q]: non-zero where QC byte q is acceptable (NULL: the package's
 *               default for MOD15A2H's FparLai_QC -- MODLAND good, no dead detector, cloud state clear
 *               or assumed clear, main algorithm with or without saturation: the codes 0, 2, 24, 26, 32,
 *               34, 56, 58); optional fallback[f][i] (the array, or any of its entries, may be NULL).
 *   reliable    slab t of pixel i is reliable for field f where its code is < 249 and, with qc,
 *               good256[qc] holds: each field has its own reliability.
 *   result      per field, pixel and slab t, with i the last reliable slab <= t (code a) and j the
 *               first reliable slab >= t (code b), an exact rational num / den and a source byte:
 *                 0 observed      t reliable: code / 1
 *                 1 interpolated  i and j exist, j - i - 1 <= max_gap: (a (j - t) + b (t - i)) / (j - i)
 *                 2 held          only one of them exists and is at most max_gap slabs away: its code / 1
 *                 3 fallback      none of these and fallback[f][pixel] < 249: that code / 1
 *                 4 unfilled      otherwise
 *               max_gap = -1: no limit.
 *   outputs     out[f][t * out_pitch + i], of out_type: MOD16_GAPFILL_U8 (2 num + den) / (2 den) in
 *               integers, round half up, 255 where unfilled; MOD16_GAPFILL_F32 / _F64
 *               (T)(((double)num / (double)den) * scale[f]), NaN where unfilled (scale is not looked at
 *               for uint8). Optional source[(f * slabs + t) * source_pitch + i], the source byte.
 *               Every element [t][0, n) is written exactly once; [t][n, pitch) is not touched.
 *               Pointers may have any byte alignment and the pitches any value >= n (in elements);
 *               rows aligned to 16 bytes take vector accesses. No workspace, no atomics: two calls
 *               give the same bits.
 *   where       MOD16_DEVICE: device pointers (good256 too), asynchronous on `stream`. MOD16_HOST:
 *               host pointers; pixel tiles are staged through the context's slabs, every slab of
 *               every array one copy per tile, the tile cut so that a slot fits stage_bytes (0: 128
 *               MiB; at least 256 pixels). The result does not depend on stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_gapfill: ...")
 *               NULL spec, fields, out or one of their first nfields entries; n < 0; "slabs must be
 *               between 1 and 4096"; "nfields must be between 1 and 3"; an unknown out_type; "max_gap
 *               must be -1 (none) or at least 0"; a pitch below n; a scale that is not finite;
 *               `where` other than the two modes; "an output overlaps an input or another output" (in
 *               place is refused, not supported). n = 0 is MOD16_OK.
 */
enum mod16_gapfill_out { MOD16_GAPFILL_U8 = 0, MOD16_GAPFILL_F32 = 1, MOD16_GAPFILL_F64 = 2 };
typedef struct mod16_gapfill_spec {
    int64_t n;                                   /* pixels */
    int32_t slabs, nfields, out_type, max_gap;   /* max_gap: -1 = none */
    double scale[3];                             /* per field, float outputs only */
    int64_t in_pitch, qc_pitch, out_pitch, source_pitch;   /* elements between two slabs */
} mod16_gapfill_spec;
MOD16_API int mod16_gapfill_u8(mod16_ctx* ctx, const mod16_gapfill_spec* spec, const uint8_t* const* fields,
                               const uint8_t* qc, const uint8_t* good256, const uint8_t* const* fallback,
                               void* const* out, uint8_t* source, int where, void* stream, size_t stage_bytes);

/*
 * Hourly reanalysis aggregated into day / night drivers (added under ABI 16, new symbols only;
 * mod16_amd.aggregate_daynight, RasterEngine.daynight): the step in front of the downscaled composite --
 * hourly planes of T10M, QV10M, PS, SWGDN and LWGNT in, the coarse planes mod16_et_composite_downscaled_*
 * takes out. One launch reads every hourly value once. The definition is the numpy statement
 * mod16_amd/daynight.py (day_weights, sw_weights, split_field, aggregate); the split is this package's
 * definition, not a transcription of the operational MOD16 preprocessing:
 *
 *   inputs      fields[5] = t, qv, ps, sw, lw (an entry may be NULL where no requested output needs it):
 *               fields[f][s * in_plane + r * in_pitch + c], step s = d * steps_per_day + k (days 1 ... 4096,
 *               steps_per_day H 1 ... 48, step k covers the UTC hours [k delta, (k + 1) delta), delta = 24 /
 *               H), row r, column c of a rows x cols grid. NaN is the missing value. The tables are HOST
 *               pointers (float64) in both modes: half_day[days][rows] (0 ... 12 hours), noon[days] (0 ...
 *               24), offset[cols] (longitude / 15, -12 ... 12).
 *   weight      per step and cell, w in [0, 1]. MOD16_DAYNIGHT_SOLAR: a = ((noon - half_day) - offset) / delta,
 *               b = ((noon + half_day) - offset) / delta, w = min(sum over m in (-H, 0, +H), in that order, of
 *               max(min(k + 1, b + m) - max(k, a + m), 0), 1). MOD16_DAYNIGHT_SW: 1.0 where sw > threshold,
 *               else 0.0, NaN where sw is NaN (sw is then needed by every output).
 *   result      per day and cell in float64, sums sequential in k from 0.0, products rounded before they are
 *               added (no contraction): sum_w = sum w, sum_n = sum (1 - w); per field X mean = (sum X) / H,
 *               day = (sum w X) / sum_w where sum_w > 0 else mean, night = (sum (1 - w) X) / sum_n where
 *               sum_n > 0 else mean (polar night and polar day stay finite).
 *   outputs     out[10] (NULL: skip), out[o][d * out_plane + r * out_pitch + c] of out_type, each value
 *               rounded once: 0 lw_net_day, 1 lw_net_night, 2 sw_rad_day, 3 temp_day, 4 temp_night, 5 tmin
 *               (min over k of t, NaN if any step is NaN), 6 vpd_day = vpd(qv_day, ps_day, t_day) as
 *               mod16_method_* computes MOD16.vpd in float64, 7 vpd_night (the same of the night values,
 *               negative values 0), 8 day_hours = delta sum_w, 9 temp_mean (mean of t). temp_annual[r *
 *               out_pitch + c] (NULL: skip) = (sum over d of temp_mean, float64, sequential in d) / days.
 *               sw_rad_night is not produced (callers pass 0.0). Every requested element [d][r][0, cols)
 *               is written exactly once; padding is not touched. Pointers may have any element alignment,
 *               in_pitch / out_pitch any value >= cols and in_plane / out_plane any value >= (rows - 1)
 *               pitch + cols, in elements; where bases, pitches and plane strides are multiples of two
 *               elements the kernel takes vector accesses, with the same bits. No atomics: two calls
 *               give the same bits. temp_annual takes 8 bytes of stream-ordered device memory per cell
 *               and day of the launch for the unrounded daily means.
 *   where       MOD16_DEVICE: device pointers (the tables stay host pointers: they are checked, then
 *               uploaded on `stream`), asynchronous on `stream`. MOD16_HOST: host pointers; chunks of whole
 *               days are staged through the context's slabs, stage_bytes / (bytes of a day's inputs and
 *               outputs) days at a time (0: 128 MiB; at least one day). The result does not depend on
 *               stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_daynight: ...")
 *               NULL spec, fields or out; "an output is requested whose field is NULL"; "no output is
 *               requested"; rows or cols outside 0 ... 2^30, days outside 0 ... 4096, steps_per_day outside
 *               1 ... 48; a pitch below cols or a plane stride below a plane; a NULL table or a table value
 *               out of its range or not finite (MOD16_DAYNIGHT_SOLAR); a threshold that is not finite
 *               (MOD16_DAYNIGHT_SW); an unknown mode, out_type or `where`; "an output overlaps an input or
 *               another output". Zero days or zero cells is MOD16_OK.
 */
enum mod16_daynight_mode { MOD16_DAYNIGHT_SOLAR = 0, MOD16_DAYNIGHT_SW = 1 };
enum mod16_daynight_out { MOD16_DAYNIGHT_F32 = 0, MOD16_DAYNIGHT_F64 = 1 };
typedef struct mod16_daynight_spec {
    int64_t rows, cols;                  /* the grid: latitude rows, longitude columns */
    int32_t days, steps_per_day;
    int32_t mode, out_type;
    double threshold;                    /* MOD16_DAYNIGHT_SW */
    int64_t in_pitch, in_plane;          /* elements between two rows / two steps of a field */
    int64_t out_pitch, out_plane;        /* ... between two rows / two days of an output (temp_annual: out_pitch) */
} mod16_daynight_spec;
MOD16_API int mod16_daynight_f32(mod16_ctx* ctx, const mod16_daynight_spec* spec, const float* const* fields,
                                 const double* half_day, const double* noon, const double* offset, void* const* out,
                                 void* temp_annual, int where, void* stream, size_t stage_bytes);
MOD16_API int mod16_daynight_f64(mod16_ctx* ctx, const mod16_daynight_spec* spec, const double* const* fields,
                                 const double* half_day, const double* noon, const double* offset, void* const* out,
                                 void* temp_annual, int where, void* stream, size_t stage_bytes);

/*
 * Per-pixel Mann-Kendall test and Theil-Sen slope over a stack of composites (added under ABI 16, new
 * symbols only; mod16_amd.trend_series, RasterEngine.trend): is the annual ET of a pixel rising, by how
 * much per unit of time, and is the rise significant. One launch reads every value once and orders the
 * pairwise slopes of a pixel in LDS. The definition is the numpy statement mod16_amd/trend.py
 * (pixel_trend), which the outputs equal bit for bit:
 *
 *   inputs      values[y * time_stride + i], step y of `steps` (2 ... 64), pixel i of n (0 ... 2^30),
 *               float32 (widened to float64: exact) or float64; NaN and the infinities are missing.
 *               times[steps]: a HOST pointer (float64) in both modes, finite and strictly increasing.
 *               Per pixel the valid steps v, their number m, M = m (m - 1) / 2.
 *   result      in float64, every operation rounded on its own (no contraction): S = sum over valid
 *               pairs a < b of sign(x[b] - x[a]); the M slopes (x[b] - x[a]) / (t[b] - t[a]) + 0.0 in
 *               ascending order q[0 ... M); the median rule med(k values) = the middle one for odd k, (lo
 *               + hi) * 0.5 of the two middle ones for even k; slope = med(q); intercept = med(x[v] + 0.0)
 *               - slope * med(t[v]); V18 = m (m - 1)(2 m + 5) - sum over groups of g equal valid values of g
 *               (g - 1)(2 g + 5); sigma = sqrt(V18 / 18.0); z = 0.0 where S = 0 or V18 = 0, else (S -
 *               sign(S)) / sigma. With zq > 0 (the normal quantile of 1 - alpha / 2): C = zq sigma,
 *               slope_hi = q[min(rint((M + C) / 2), M - 1)], slope_lo = q[max(rint((M - C) / 2) - 1, 0)],
 *               rint to even. Where m < min_valid: S = 0 and the five floats are NaN.
 *   outputs     out[5] = slope, intercept, slope_lo, slope_hi, z (float64[n]), s (int32[n]), count
 *               (uint8[n], m); a NULL entry (or out NULL) is skipped, every requested element is written
 *               exactly once. Pointers may have any element alignment, time_stride any value >= n. No
 *               atomics: two calls give the same bits. A stack laid out (steps, P, n) -- one trend per
 *               8-day period -- is the same call with P n pixels.
 *   where       MOD16_DEVICE: device pointers (times stays a host pointer: checked, then uploaded on
 *               `stream` into stream-ordered memory), asynchronous on `stream`. MOD16_HOST: host pointers;
 *               ranges of pixels, all `steps` rows of a range, are staged through the context's slabs,
 *               a slab of at most stage_bytes (0: 128 MiB; at least 256 pixels). The result does not
 *               depend on stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_trend: ...")
 *               NULL spec, values or times; "no output is requested"; n outside 0 ... 2^30, steps outside
 *               2 ... 64 (mod16_trend_max_steps()); time_stride below n; times not finite, not strictly
 *               increasing, or with a span that is not finite; min_valid outside 2 ... steps; zq negative
 *               or not finite; slope_lo or slope_hi given with zq = 0; an unknown `where`; "an output
 *               overlaps an input or another output". n = 0 is MOD16_OK.
 */
typedef struct mod16_trend_spec {
    int64_t n;                           /* pixels */
    int32_t steps;                       /* Y: values per pixel */
    int32_t min_valid;                   /* fewer valid values: no trend */
    int64_t time_stride;                 /* elements between two steps of `values` */
    double zq;                           /* 0: no interval */
} mod16_trend_spec;
MOD16_API int mod16_trend_max_steps(void);
MOD16_API int mod16_trend_f32(mod16_ctx* ctx, const mod16_trend_spec* spec, const float* values, const double* times,
                              double* const* out, int32_t* s, uint8_t* count, int where, void* stream,
                              size_t stage_bytes);
MOD16_API int mod16_trend_f64(mod16_ctx* ctx, const mod16_trend_spec* spec, const double* values, const double* times,
                              double* const* out, int32_t* s, uint8_t* count, int where, void* stream,
                              size_t stage_bytes);

/*
 * Per-pixel climatology, standardized anomalies and percentile ranks over a record of composites (added
 * under ABI 16, new symbols only; mod16_amd.anomaly_series, RasterEngine.anomaly): how unusual is this
 * 8-day period of this year against the same period of the baseline years. One launch reads the record
 * and writes every result once. The definition is the numpy statement mod16_amd/anomaly.py (anomaly),
 * which the outputs equal bit for bit:
 *
 *   inputs      num[s * in_stride + i], slab s = y * periods + p of years * periods (years outermost),
 *               pixel i of n (0 ... 2^30), float32 (widened to float64: exact) or float64; den likewise
 *               or NULL -- with den the quantity is the ratio, ET / PET say. years 2 ... 64, periods
 *               1 ... 366, years * periods <= 4096, window W 1 ... min(periods, 16)
 *               (mod16_anomaly_max_window()).
 *   result      in float64, every operation rounded on its own (no contraction). r[s]: missing for
 *               s < W - 1, else a = +0.0, a = a + num[k] for k = s - W + 1 ... s in that order, b
 *               likewise from den, r = a / b (r = a without den), valid where r is finite and (with den)
 *               0 < b < inf. Per period p over the baseline years base_first ... base_end - 1 in year order:
 *               m valid values, sum from +0.0, mean = sum / m, ss the sum from +0.0 of the rounded
 *               squares of r - mean, std = sqrt(ss / (m - 1)); mean and std NaN where m < min_valid.
 *               Per slab of every year: z = (r - mean) / std where r is valid, m >= min_valid and std
 *               is finite and > 0, else NaN; pct = (lt + 0.5 eq) / m with lt / eq the valid baseline
 *               values of the period below / equal to r, NaN where r is missing or m < min_valid.
 *   outputs     z, pct: [years * periods] rows out_stride apart, of the input type (float32: the
 *               float64 result rounded once); mean, std (float64) and count (uint8, m):
 *               [periods] rows clim_stride apart. A NULL output is skipped and not written; every
 *               requested element is written exactly once. Pointers may have any element alignment,
 *               the strides any value >= n. No atomics: two calls give the same bits.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream`. MOD16_HOST: host pointers;
 *               ranges of pixels, all rows of a range, are staged through the context's slabs, a slab
 *               of at most stage_bytes (0: 128 MiB; at least 256 pixels). The result does not depend on
 *               stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_anomaly: ...")
 *               NULL spec or num; "no output is requested"; n outside 0 ... 2^30; periods outside
 *               1 ... 366; years outside 2 ... 64; years * periods above 4096; window outside
 *               1 ... min(periods, 16); a baseline outside 0 <= base_first < base_end <= years or shorter
 *               than 2 years; min_valid outside 2 ... base_end - base_first; a stride of a given array
 *               below n; an unknown `where`; "an output overlaps an input or another output". n = 0 is
 *               MOD16_OK.
 */
typedef struct mod16_anomaly_spec {
    int64_t n;                           /* pixels */
    int32_t years, periods;              /* Y, P: the record has Y * P slabs, years outermost */
    int32_t window;                      /* W: periods summed into a value */
    int32_t base_first, base_end;        /* the baseline years */
    int32_t min_valid;                   /* fewer valid baseline values: no climatology */
    int64_t in_stride;                   /* elements between two slabs of num and den */
    int64_t out_stride;                  /* ... of z and pct */
    int64_t clim_stride;                 /* ... between two periods of mean, std and count */
} mod16_anomaly_spec;
MOD16_API int mod16_anomaly_max_window(void);
MOD16_API int mod16_anomaly_f32(mod16_ctx* ctx, const mod16_anomaly_spec* spec, const float* num, const float* den,
                                float* z, float* pct, double* mean, double* std, uint8_t* count, int where,
                                void* stream, size_t stage_bytes);
MOD16_API int mod16_anomaly_f64(mod16_ctx* ctx, const mod16_anomaly_spec* spec, const double* num, const double* den,
                                double* z, double* pct, double* mean, double* std, uint8_t* count, int where,
                                void* stream, size_t stage_bytes);

/*
 * Upscaling (added under ABI 16, new symbols only; mod16_amd.upscale_fields / upscale_classes,
 * RasterEngine.upscale_grid): the area-weighted mean of the valid fine pixels of every cell of a coarse
 * grid, with the valid fraction and count, and the dominant class of a class raster per cell. The
 * definition is the numpy statement mod16_amd/upscale.py (aggregate, majority), which the outputs
 * equal bit for bit.
 *
 *   geometry    a rows x cols fine raster over coarse_rows x coarse_cols cells (each 1 ... 2^30). The
 *               fine rows of coarse row i are row_first[i] + 0 ... row_count[i] - 1, the fine columns of
 *               coarse column j are col_first[j] + 0 ... col_count[j] - 1 -- with wrap_cols (a global
 *               longitude axis) modulo cols: one run may pass the last column. A count may be 0 (an
 *               empty cell). mod16_amd.upscale.cell_table / cell_runs derive the tables from positions.
 *               area[rows] (or NULL: 1.0) is the weight of a pixel of that fine row, cos(latitude) say.
 *               mod16_upscale_create copies the tables to the device; the handle belongs to the context's
 *               device and is freed with mod16_upscale_destroy (NULL is fine).
 *   refused by mod16_upscale_create (MOD16_ERR_ARG, "mod16_upscale_create: ...")
 *               NULL spec, tables or handle pointer; an extent outside 1 ... 2^30; wrap_cols not 0 or 1;
 *               a count below 0 or above its axis; a run of pixels that starts outside its axis or
 *               (rows; columns without wrap_cols) ends behind it; two runs of one axis that share a
 *               fine index; the largest row_count times the largest col_count at or above 2^31; an area
 *               that is not positive and finite.
 *   mean        values[k * layer_stride + r * row_stride + c], k of `layers` (1 ... 65535), float32
 *               (widened to float64: exact) or float64; row_stride >= cols, layer_stride at least a
 *               plane. Per layer and cell, every operation rounded on its own (no contraction): num =
 *               den = tot = +0.0, cnt = 0; per row r of the cell in run order s = +0.0, m = 0, per column
 *               in run order s = s + x and m += 1 where x is not NaN; then num = num + area[r] * s, den =
 *               den + area[r] * m, tot = tot + area[r] * col_count[j], cnt += m. fraction = den / tot (0.0
 *               for a cell without pixels); mean = num / den where cnt >= 1 and den >= min_fraction * tot,
 *               else NaN; count = cnt.
 *   outputs     mean, fraction (the input type; float32: the float64 result rounded once) and count
 *               (int32): [layers][coarse_rows][coarse_cols], each with its own layer and row stride (row
 *               stride >= coarse_cols, layer stride at least a plane). A NULL output is skipped and not
 *               written; every requested element is written exactly once. No atomics: two calls give
 *               the same bits.
 *   classes     cls[r * row_stride + c] uint8; bit c of `valid` set: code c (below 32) counts. Per cell
 *               the code with the most pixels, the LOWEST code on a tie, 255 where no pixel counts ->
 *               out_cls (uint8); out_share (float32) = float32(double(winner's pixels) / double(row_count
 *               * col_count)), 0 where none counts. Either output may be NULL, not both.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream`. MOD16_HOST: host pointers;
 *               bands of whole coarse rows -- their fine rows are one range of rows of the raster -- are
 *               staged through the context's slabs, a slab of at most stage_bytes (0: 128 MiB); where the
 *               layers of one coarse row exceed that, the layers are cut first; one coarse row of one
 *               layer goes through whatever the budget. The result does not depend on stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_upscale: ..." / "mod16_upscale_classes: ...")
 *               NULL grid or input; a grid of another device; "no output is requested"; layers outside
 *               1 ... 65535; a row stride below the row, a layer stride below the plane; min_fraction
 *               outside [0, 1] or NaN; an unknown `where`; stage_bytes out of range; "an output overlaps
 *               an input or another output".
 */
typedef struct mod16_upscale mod16_upscale;
typedef struct mod16_upscale_spec {
    int64_t rows, cols;                  /* the fine raster */
    int64_t coarse_rows, coarse_cols;    /* the coarse grid */
    int32_t wrap_cols;                   /* 1: the column runs are cyclic */
    int32_t reserved_;                   /* 0 */
} mod16_upscale_spec;
MOD16_API int mod16_upscale_create(mod16_ctx* ctx, const mod16_upscale_spec* spec, const int32_t* row_first,
                                   const int32_t* row_count, const int32_t* col_first, const int32_t* col_count,
                                   const double* area, mod16_upscale** out);
MOD16_API int mod16_upscale_destroy(mod16_upscale* grid);
MOD16_API int mod16_upscale_f32(mod16_ctx* ctx, const mod16_upscale* grid, const float* values, int32_t layers,
                                int64_t layer_stride, int64_t row_stride, double min_fraction, float* mean,
                                int64_t mean_layer_stride, int64_t mean_row_stride, float* fraction,
                                int64_t fraction_layer_stride, int64_t fraction_row_stride, int32_t* count,
                                int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                size_t stage_bytes);
MOD16_API int mod16_upscale_f64(mod16_ctx* ctx, const mod16_upscale* grid, const double* values, int32_t layers,
                                int64_t layer_stride, int64_t row_stride, double min_fraction, double* mean,
                                int64_t mean_layer_stride, int64_t mean_row_stride, double* fraction,
                                int64_t fraction_layer_stride, int64_t fraction_row_stride, int32_t* count,
                                int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                size_t stage_bytes);
MOD16_API int mod16_upscale_classes(mod16_ctx* ctx, const mod16_upscale* grid, const uint8_t* cls, int64_t row_stride,
                                    uint32_t valid, uint8_t* out_cls, int64_t cls_row_stride, float* out_share,
                                    int64_t share_row_stride, int where, void* stream, size_t stage_bytes);

/*
 * Upscaling from rasters with row-affine columns -- MODIS sinusoidal tiles -- and mergeable cell sums
 * (added under ABI 16, new symbols only; RasterEngine.upscale_grid(col_affine=...), UpscaleGrid.sums,
 * mod16_amd.upscale_sums, mod16_amd.upscale.merge). The definition is mod16_amd/upscale.py
 * (cell_table_rows, aggregate_rows, sums_rows, majority_rows), which the outputs equal bit for bit.
 *
 *   geometry    the rows as above (row_first, row_count). The column position of pixel (r, c) is
 *               col_origin[r] + col_scale[r] * c in units of coarse cells (one multiplication, one
 *               addition, each rounded; mod16_amd.downscale.sinusoidal_positions), and the pixel belongs
 *               to the cell mod16_amd.upscale.cell_table gives that position: without wrap_cols i0 =
 *               floor(pos), f = pos - i0, cell = i0 + (f >= 0.5), none outside [0, coarse_cols); with
 *               wrap_cols p = pos - floor(pos / W) W (0 where that is not in [0, W)), cell = (floor(p) +
 *               (f >= 0.5)) mod W. col_first[rows], col_count[rows] (both NULL: every column): only the
 *               columns col_first[r] ... col_first[r] + col_count[r] - 1 of fine row r can belong to a
 *               cell, the others are not read (the on-globe pixels of an edge tile:
 *               mod16_amd.downscale.sinusoidal_columns). The column run of a cell in a fine row is found
 *               on the device from the row's two float64; the cell's pixels in that row are col_count[j]
 *               of the statement above, and out_share divides by their sum over the cell's rows.
 *               The handle is a mod16_upscale like any other: mod16_upscale_f32 / _f64 / _classes and
 *               the sums take it, mod16_upscale_destroy frees it.
 *   refused by mod16_upscale_create_rows (MOD16_ERR_ARG, "mod16_upscale_create_rows: ...")
 *               NULL spec, row tables, col_origin, col_scale or handle pointer; one of col_first and
 *               col_count NULL alone; an extent outside 1 ... 2^30; wrap_cols not 0 or 1; bad row runs
 *               (as mod16_upscale_create); col_origin, col_scale or col_origin + col_scale (cols - 1) not
 *               finite; a column range outside [0, cols); with wrap_cols a row of n = col_count > 1
 *               columns with abs(col_scale) * (n - 1) > coarse_cols - 2 (it may lap the periodic axis:
 *               narrow the range or cut the raster; sufficient for one run of columns per cell and
 *               row); the largest row_count times the largest col_count at or above 2^31; a bad area.
 *   sums        mod16_upscale_sums_f32 / _f64, for handles of both kinds: num, den, tot (float64 whatever
 *               the input type) and count (int32) of the statement above, before the divisions --
 *               what a tile contributes to cells it covers in part; add the sums of several tiles in
 *               a fixed order and divide once (mod16_amd.upscale.merge). Each output
 *               [layers][coarse_rows][coarse_cols] with its own layer and row stride; a NULL output is
 *               skipped, at least one is required. where, stage_bytes and the refusals
 *               ("mod16_upscale_sums: ...") are those of mod16_upscale_f32.
 */
MOD16_API int mod16_upscale_create_rows(mod16_ctx* ctx, const mod16_upscale_spec* spec, const int32_t* row_first,
                                        const int32_t* row_count, const double* col_origin, const double* col_scale,
                                        const int32_t* col_first, const int32_t* col_count, const double* area,
                                        mod16_upscale** out);
MOD16_API int mod16_upscale_sums_f32(mod16_ctx* ctx, const mod16_upscale* grid, const float* values, int32_t layers,
                                     int64_t layer_stride, int64_t row_stride, double* num, int64_t num_layer_stride,
                                     int64_t num_row_stride, double* den, int64_t den_layer_stride, int64_t den_row_stride,
                                     double* tot, int64_t tot_layer_stride, int64_t tot_row_stride, int32_t* count,
                                     int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                     size_t stage_bytes);
MOD16_API int mod16_upscale_sums_f64(mod16_ctx* ctx, const mod16_upscale* grid, const double* values, int32_t layers,
                                     int64_t layer_stride, int64_t row_stride, double* num, int64_t num_layer_stride,
                                     int64_t num_row_stride, double* den, int64_t den_layer_stride, int64_t den_row_stride,
                                     double* tot, int64_t tot_layer_stride, int64_t tot_row_stride, int32_t* count,
                                     int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                     size_t stage_bytes);

/*
 * Downscaled forward run (ABI 14; mod16_amd.evapotranspiration_downscaled,
 * RasterEngine.downscale_grid): ET day and night for a contiguous range of pixels of a rows x cols
 * fine raster, each of the 14 drivers a scalar, a fine array or a COARSE coarse_rows x coarse_cols
 * array (reanalysis meteorology) interpolated per pixel inside the kernel -- the interpolated values
 * never touch memory. The definition is the numpy statement mod16_amd/downscale.py (corner_tables,
 * interpolate):
 *
 *   geometry    row_pos[rows], col_pos[cols] (HOST pointers, float64): the position of every fine row
 *               / column in units of coarse cells, cell centres at the integers. Rectilinear grids
 *               (row-affine columns: below). Per axis and entry, two cells and two weights:
 *                 held edge (rows; columns with wrap_cols = 0): p = min(max(pos, 0), size - 1),
 *                   i0 = floor(p), f = p - i0, i1 = min(i0 + 1, size - 1);
 *                 wrap_cols = 1 (the longitude axis of a global grid): p = pos - floor(pos / size) size,
 *                   0 where that is not in [0, size); i0 = floor(p), f = p - i0, i1 = (i0 + 1) % size;
 *                 w1 (the far cell's weight; w0 = 1.0 - w1): MOD16_DOWNSCALE_NEAREST 1.0 where
 *                   f >= 0.5, else 0.0; _BILINEAR f; _COS4 b / (a + b), a = cos(pi/2 f)^4,
 *                   b = cos(pi/2 (1 - f))^4, and 0.0 where f == 0 -- a separable form of the cosine-to-the-fourth distance
 *                   weighting, not the great-circle form of the operational algorithm.
 *               mod16_downscale_create computes the tables on the host (cos and pow of the C
 *               library); mod16_downscale_create_tables takes tables the caller computed (the Python
 *               layer passes numpy's, so that device results carry the bits of the numpy definition
 *               whatever the two cosines round to) and checks them: indices inside the coarse grid,
 *               finite weights. The handle owns device copies of the tables.
 *   value       corners in the order (row i0, col i0), (i0, i1), (i1, i0), (i1, i1); a corner's weight
 *               is wr * wc, its term w * v where w != 0 and +0.0 where w == 0 (a corner without weight
 *               cannot poison a pixel), the value ((t00 + t01) + t10) + t11 in float64, left to right,
 *               no contraction. A NaN corner with weight gives NaN; nothing is renormalised.
 *   run         kinds[k]: 0 a scalar (one value), 1 a fine array, 2 a coarse array. Fine arrays, cls
 *               and the outputs are addressed from the range's first pixel (element 0 is pixel
 *               first_pixel of the raster, row-major); coarse arrays are whole
 *               [coarse_rows][coarse_pitch] planes, coarse_pitch >= coarse_cols in elements. The
 *               pixel's ET is what mod16_et_* gives on the interpolated drivers, bit for bit, with the
 *               same flags. float32: inputs widened, interpolation and arithmetic in float64, one
 *               rounding on store.
 *   flags       MOD16_MATH_FAST (0) or MOD16_MATH_EXACT; the fast instance tests every interpolated
 *               pixel against the domain of its arithmetic and a second kernel behind it recomputes
 *               the flagged pixels in the reference's operation order. No atomics on results, no
 *               workspace: two calls give the same bits.
 *   fields      mod16_downscale_fields_*: out[f * out_pitch + i] = the interpolated field f (1 <= F
 *               <= 16 coarse planes) at pixel first_pixel + i, rounded once to T; [n, out_pitch) of a
 *               row is not touched.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream` (mod16_check_status reports a
 *               class code >= 13). MOD16_HOST: host pointers; the coarse planes are uploaded once per
 *               call, the fine arrays, class raster and outputs are staged tile by tile
 *               (mod16_host_tile_pixels() pixels). The result does not depend on the tiling.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_downscale_create: ...",
 *            "mod16_et_downscaled: ...", "mod16_downscale_fields: ...")
 *               a NULL argument; rows, cols, coarse_rows, coarse_cols outside 1 ... 2^30; wrap_cols
 *               other than 0 or 1; an unknown method; a position that is not finite; a table index
 *               outside the coarse grid or a weight that is not finite; a kind other than 0, 1, 2;
 *               "coarse_pitch must be at least coarse_cols"; "the pixel range [first_pixel,
 *               first_pixel + n) leaves the raster"; "out_pitch must be at least n"; "F must be between
 *               1 and 16"; a grid of another device; an unknown flag; "MOD16_MATH_MIXED is not
 *               available for the downscaled run" and "MOD16_DOMAIN_TRUSTED is not available for the
 *               downscaled run". n = 0 is MOD16_OK.
 *
 * Row-affine columns (additive in ABI 16; mod16_amd.downscale.corner_tables_rows, sinusoidal_positions;
 * `col_affine` of the Python layer): a second geometry of the same handle for fine grids whose column
 * mapping depends on the row -- MODIS sinusoidal tiles, where the longitude of column c is
 * x / (R cos(lat_row)). The column position of pixel (r, c) is
 *
 *     col_pos(r, c) = col_origin[r] + col_scale[r] * c        (one multiplication, one addition, each rounded)
 *
 *   geometry    mod16_downscale_create_rows(row_pos[rows], col_origin[rows], col_scale[rows]) computes the
 *               row tables on the host as mod16_downscale_create does; mod16_downscale_create_rows_tables
 *               takes the caller's row tables as mod16_downscale_create_tables does. The handle owns
 *               device copies of the row tables and of the two float64 per row; the column cell pair and
 *               its weights are formed per pixel inside the kernel by the formulas of "geometry" above
 *               (wrap_cols and method of the spec govern them), in float64 with multiply, add, a correctly
 *               rounded division, floor and compare, no contraction: the bits of the numpy definition.
 *   use         mod16_et_downscaled_*, mod16_downscale_fields_* and mod16_et_composite_downscaled_* accept
 *               a handle of either geometry and pick their kernel instances by it; everything said of
 *               them above and below holds unchanged (ranges, pitches, HOST and DEVICE).
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_downscale_create: ...")
 *               a NULL argument; the spec as above; MOD16_DOWNSCALE_COS4 (its weights need a cosine, which
 *               the device would not reproduce bit for bit); a row position that is not finite, a row
 *               table index outside the coarse grid or a weight that is not finite; a row r whose
 *               col_origin[r], col_scale[r] or col_origin[r] + col_scale[r] * (cols - 1) is not finite
 *               (finite end points make every position of the row finite). Whatever the arithmetic
 *               gives, the kernels clamp the computed cell index into [0, coarse_cols).
 */
enum mod16_downscale_method { MOD16_DOWNSCALE_NEAREST = 0, MOD16_DOWNSCALE_BILINEAR = 1, MOD16_DOWNSCALE_COS4 = 2 };
typedef struct mod16_downscale_spec {
    int64_t rows, cols;                          /* the fine raster */
    int64_t coarse_rows, coarse_cols;            /* the coarse grid */
    int32_t wrap_cols;                           /* 1: the column axis of the coarse grid is periodic */
    int32_t method;                              /* enum mod16_downscale_method */
} mod16_downscale_spec;
typedef struct mod16_downscale mod16_downscale;
MOD16_API int mod16_downscale_create(mod16_ctx* ctx, const mod16_downscale_spec* spec, const double* row_pos,
                                     const double* col_pos, mod16_downscale** grid);
MOD16_API int mod16_downscale_create_tables(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* row_i0,
                                            const int32_t* row_i1, const double* row_w0, const double* row_w1,
                                            const int32_t* col_i0, const int32_t* col_i1, const double* col_w0,
                                            const double* col_w1, mod16_downscale** grid);
MOD16_API int mod16_downscale_create_rows(mod16_ctx* ctx, const mod16_downscale_spec* spec, const double* row_pos,
                                          const double* col_origin, const double* col_scale, mod16_downscale** grid);
MOD16_API int mod16_downscale_create_rows_tables(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* row_i0,
                                                 const int32_t* row_i1, const double* row_w0, const double* row_w1,
                                                 const double* col_origin, const double* col_scale,
                                                 mod16_downscale** grid);
MOD16_API int mod16_downscale_destroy(mod16_downscale* grid);
MOD16_API int mod16_et_downscaled_f64(mod16_ctx* ctx, const mod16_downscale* grid, const uint8_t* cls,
                                      const double* const* drivers, const int32_t* kinds, int64_t coarse_pitch,
                                      int64_t first_pixel, int64_t n, double* out_day, double* out_night,
                                      unsigned flags, int where, void* stream);
MOD16_API int mod16_et_downscaled_f32(mod16_ctx* ctx, const mod16_downscale* grid, const uint8_t* cls,
                                      const float* const* drivers, const int32_t* kinds, int64_t coarse_pitch,
                                      int64_t first_pixel, int64_t n, float* out_day, float* out_night,
                                      unsigned flags, int where, void* stream);
MOD16_API int mod16_downscale_fields_f64(mod16_ctx* ctx, const mod16_downscale* grid, const double* const* fields,
                                         int nfields, int64_t coarse_pitch, int64_t first_pixel, int64_t n,
                                         double* out, int64_t out_pitch, int where, void* stream);
MOD16_API int mod16_downscale_fields_f32(mod16_ctx* ctx, const mod16_downscale* grid, const float* const* fields,
                                         int nfields, int64_t coarse_pitch, int64_t first_pixel, int64_t n,
                                         float* out, int64_t out_pitch, int where, void* stream);

/*
 * Zonal statistics (ABI 15; mod16_amd.zonal_statistics, RasterEngine.zonal): exact weighted totals per
 * zone and layer -- ET in km3 per basin, country, biome or climate-grid cell -- in one pass over the
 * raster, with sums that do not depend on the order of arrival: one launch, a call staged in tiles,
 * several calls that accumulate tile after tile and the sum of several devices' partial results give
 * the same words. The definition is the numpy statement mod16_amd/zonal.py (classify, quantise,
 * accumulate):
 *
 *   inputs      values[k * value_pitch + i]: layer k (0 ... layers - 1), pixel i; zones[i] of zone_type
 *               (MOD16_ZONE_U8 / _U16 / _I32); a weight w per pixel by weight_kind:
 *               MOD16_ZONAL_WEIGHT_NONE w = 1 (weights is not looked at); _ROW weights is float64, one
 *               entry per raster row, and pixel i takes weights[(first_pixel + i) / cols] (the area of
 *               a latitude row; the vector must reach the row of the last pixel); _PIXEL weights[i]
 *               of the values' type. float32 inputs are widened; all arithmetic is float64.
 *   bounds      0 < wmax <= 2^ew and 0 < xmax <= 2^ex (ew, ex the smallest such exponents when the
 *               call comes from the Python layer). The three sums carry F0 = 62 - ew, F1 = 62 - ew - ex
 *               and F2 = 62 - ew - 2 ex fractional bits.
 *   per pixel and layer, in this order
 *               a zone id outside [0, nzones): ignored; x NaN or w NaN: ignored (masked);
 *               !(|x| <= xmax) or !(0 <= w <= wmax): rejected += 1, nothing else (infinities land
 *               here); otherwise count += 1 and, for t = w, w x, (w x) x (one rounded multiply each),
 *               q = (int64)rint(ldexp(t, F)) (|q| <= 2^62), hi += q >> 32, lo += q & 0xffffffff; the
 *               min and max words take key(x), the bits of the double with the low 63 flipped where
 *               the sign is set (an order-preserving int64; -0.0 < +0.0).
 *   acc         int64 [layers][nzones][10]: count, rejected, w_hi, w_lo, wx_hi, wx_lo, wxx_hi, wxx_lo,
 *               min_key, max_key. The call ADDS into it: the caller starts it with min_key =
 *               INT64_MAX, max_key = INT64_MIN, the rest 0. A sum is (hi * 2^32 + lo) / 2^F. Valid
 *               while a zone and layer holds fewer than 2^31 valid pixels over everything accumulated
 *               into it (every lo word then stays below 2^63). Two accumulators with the same
 *               exponents add word by word (min / max of the last two).
 *   kernel      a lane merges runs of equal zone id in registers; up to mod16_zonal_lds_zones() zones
 *               a block accumulates in an LDS table with 64-bit LDS integer atomics and flushes the
 *               entries it touched with global 64-bit integer atomics; above that the runs go straight
 *               to the accumulator, those of a wave's neighbouring lanes that hold the same zone merged
 *               first -- right for any zone map, slow for one without runs. No float atomics anywhere:
 *               the words of two calls are identical.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream`; stage_bytes is not looked at.
 *               MOD16_HOST: host pointers; values, zones and per-pixel weights are staged tile by tile
 *               through the context's slabs, the tile cut so that a slot fits stage_bytes (0: 128 MiB;
 *               at least 256 pixels); acc is uploaded once, added into by every tile and downloaded
 *               once; the per-row weights are uploaded once. The result does not depend on stage_bytes.
 *   bounds pre-pass
 *               mod16_zonal_bounds_*: *xmax = max |x| over the finite values of all layers (0 if
 *               none), *wmax = max w over the finite weights >= 0 of the pixels' range (1 without
 *               weights), by integer maxima of the bit patterns; synchronous in both modes. Looks at
 *               n, layers, weight_kind, cols, first_pixel and value_pitch of the spec only.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_zonal: ...", "mod16_zonal_bounds: ...")
 *               a NULL argument; n < 0 or n > 2^30; layers outside 1 ... 65535; nzones outside 1 ...
 *               2^24; an unknown zone_type, weight_kind or `where`; per-row weights with cols < 1 or
 *               first_pixel outside 0 ... 2^50; value_pitch < n; exponents for which an F leaves
 *               [-900, 900]; bounds that are not positive or exceed 2^ew / 2^ex; "acc overlaps an
 *               input". Memory that cannot be had is MOD16_ERR_NOMEM. n = 0 is MOD16_OK and leaves
 *               acc untouched.
 */
enum mod16_zone_type { MOD16_ZONE_U8 = 0, MOD16_ZONE_U16 = 1, MOD16_ZONE_I32 = 2 };
enum mod16_zonal_weight { MOD16_ZONAL_WEIGHT_NONE = 0, MOD16_ZONAL_WEIGHT_ROW = 1, MOD16_ZONAL_WEIGHT_PIXEL = 2 };
typedef struct mod16_zonal_spec {
    int64_t n;                                   /* pixels */
    int32_t layers, nzones;
    int32_t zone_type, weight_kind;              /* enum mod16_zone_type, enum mod16_zonal_weight */
    int64_t cols, first_pixel;                   /* per-row weights: raster columns, raster index of pixel 0 */
    int64_t value_pitch;                         /* elements between two layers */
    int32_t ew, ex;                              /* wmax <= 2^ew, xmax <= 2^ex */
    double wmax, xmax;                           /* what a pixel is tested against */
} mod16_zonal_spec;
MOD16_API int mod16_zonal_f64(mod16_ctx* ctx, const mod16_zonal_spec* spec, const double* values, const void* zones,
                              const void* weights, int64_t* acc, int where, void* stream, size_t stage_bytes);
MOD16_API int mod16_zonal_f32(mod16_ctx* ctx, const mod16_zonal_spec* spec, const float* values, const void* zones,
                              const void* weights, int64_t* acc, int where, void* stream, size_t stage_bytes);
MOD16_API int mod16_zonal_bounds_f64(mod16_ctx* ctx, const mod16_zonal_spec* spec, const double* values,
                                     const void* weights, double* wmax, double* xmax, int where, void* stream,
                                     size_t stage_bytes);
MOD16_API int mod16_zonal_bounds_f32(mod16_ctx* ctx, const mod16_zonal_spec* spec, const float* values,
                                     const void* weights, double* wmax, double* xmax, int where, void* stream,
                                     size_t stage_bytes);
MOD16_API int mod16_zonal_lds_zones(void);

/*
 * Zonal histograms and exact zonal quantiles (added under ABI 16, new symbols only; mod16_amd.zonal_histogram,
 * mod16_amd.zonal_quantiles, RasterEngine.zonal_histogram / zonal_selection / zonal_quantiles): per zone and layer the histogram
 * of the values and exact order statistics -- the median and the spread of ET per biome, basin or
 * country -- from int64 tables that 64-bit integer adds fill, so that, as for mod16_zonal_*, one
 * launch, a call staged in tiles, calls that accumulate part after part and the sum of several
 * devices' tables give the same words. The definition is the numpy statement mod16_amd/zonalq.py
 * (histogram, digits, select):
 *
 *   inputs      values, zones, weights, zone_type, weight_kind, cols, first_pixel, value_pitch: as in
 *               mod16_zonal_spec. width: 32 (float32) or 64 (float64), the bits of the values' type.
 *   per pixel and layer
 *               a zone id outside [0, nzones): skipped; x NaN or w NaN: skipped; !(0 <= w <= wmax):
 *               skipped (infinite x takes part). The weight word is 1 (MOD16_ZONAL_WEIGHT_NONE) or qw =
 *               (int64)rint(ldexp(w, 31 - ew)) <= 2^31, 0 < wmax <= 2^ew; a weight below 2^(ew - 32)
 *               quantises to 0 and counts for nothing. The key is the order-preserving unsigned image
 *               of the value in its own width: the bits, all flipped where the sign is set, else the
 *               sign bit set (-0.0 < +0.0).
 *   MOD16_ZONAL_HIST_UNIFORM
 *               hist is int64 [layers][nzones][bins + 2], 1 <= bins <= 4094: word 0 the under bin (x <
 *               lo), word bins + 1 the over bin (!(x < hi)), else word min(bins, 1 + (int)floor((x -
 *               lo) * scale)) with x widened to float64, the subtraction and the multiply rounded once
 *               each (no fused multiply-add); scale = bins / (hi - lo) is the caller's.
 *   MOD16_ZONAL_HIST_DIGIT
 *               hist is int64 [layers][nzones][slots][2^bits], 4 <= bits <= 12, 1 <= slots <= 16,
 *               0 <= level < ceil(width / bits). Level 0 counts the top `bits` bits of every valid
 *               pixel's key into slot 0 only (prefix is not looked at). On a level l >= 1 a pixel is
 *               counted into every slot s for which the top l * bits bits of its key equal
 *               prefix[layer][zone][s], under the next min(bits, width - l * bits) bits of its key.
 *   hist        the call ADDS into it (the caller starts it with zeros). Valid while a zone and layer
 *               holds fewer than 2^31 valid pixels over everything added into it. Two tables of the
 *               same call shape add word by word.
 *   mod16_zonal_select
 *               closes a level of the digit form for every (layer, zone, slot). Level 0: W = the sum
 *               of hist[layer][zone][0][*] goes to weight[layer][zone], and the target of slot s is
 *               max(1, ceil(q_mant[s] * W / 2^q_exp[s])) in 128-bit integers (0 <= q_mant < 2^53, the
 *               quantile q = q_mant / 2^q_exp in [0, 1] exactly: m, e = frexp(q), q_mant = m 2^53,
 *               q_exp = 53 - e; q_mant and q_exp are host arrays of `slots` entries in both modes);
 *               W = 0 leaves remaining = 0, which marks "no value". Every level: the first bin whose
 *               running sum reaches remaining (level 0: the target; slot s reads slot 0's row) is
 *               appended to prefix, and remaining drops by the sum before that bin. After the last
 *               level the prefix is the key of the answer: out_values (of the values' type,
 *               [layers][nzones][slots]) takes the value, NaN where remaining is 0 -- the smallest
 *               value of the zone whose cumulative weight word reaches the target, the weighted
 *               inverted-CDF quantile, an exact order statistic. The caller zeroes hist between levels.
 *   kernel      zonal_kernel's traversal; tables of up to mod16_zonal_hist_lds_bytes() bytes (per
 *               layer: nzones * slots * 2^bits words, one slot on level 0; nzones * (bins + 2)) are
 *               filled in LDS with 64-bit LDS integer adds and flushed, the words that are not zero,
 *               with global 64-bit integer atomic adds; larger ones take the adds in global memory.
 *               A lane merges runs of equal table word in registers. No float atomics.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream` (no host synchronisation between
 *               the levels). MOD16_HOST: host pointers; mod16_zonal_hist_* stage values, zones and
 *               per-pixel weights tile by tile as mod16_zonal_* do, the table goes up once, every tile
 *               adds into it, and it comes down once: the result does not depend on stage_bytes;
 *               mod16_zonal_select runs the same integer loop on the CPU, with no device work.
 *   refused (MOD16_ERR_ARG, before any device work and before an output is touched; "mod16_zonal_hist:
 *   ...", "mod16_zonal_select: ...")
 *               everything mod16_zonal_* refuses; an unknown mode; a width that is not that of the
 *               values; bins, bits, slots or level out of range; lo, hi or scale not finite, hi <= lo,
 *               scale <= 0; a NULL prefix on a level above 0; "the table overlaps an input";
 *               mod16_zonal_select: a quantile outside [0, 1], a missing q_mant, q_exp or weight on
 *               level 0, a missing out_values on the last level, an output on the table. n = 0 is
 *               MOD16_OK and leaves hist untouched.
 */
enum mod16_zonal_hist_mode { MOD16_ZONAL_HIST_UNIFORM = 0, MOD16_ZONAL_HIST_DIGIT = 1 };
typedef struct mod16_zonal_hist_spec {
    int64_t n;                                   /* pixels */
    int32_t layers, nzones;
    int32_t zone_type, weight_kind;              /* enum mod16_zone_type, enum mod16_zonal_weight */
    int64_t cols, first_pixel;                   /* per-row weights: raster columns, raster index of pixel 0 */
    int64_t value_pitch;                         /* elements between two layers */
    int32_t ew, mode;                            /* wmax <= 2^ew; enum mod16_zonal_hist_mode */
    double wmax;                                 /* what a weight is tested against */
    int32_t bins, width;                         /* uniform: bins; both: 32 or 64, the bits of a value */
    double lo, hi, scale;                        /* uniform: the range and bins / (hi - lo) */
    int32_t bits, level, slots, reserved;        /* digit: bits per level, the level, slots per zone */
} mod16_zonal_hist_spec;
MOD16_API int mod16_zonal_hist_f64(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const double* values,
                                   const void* zones, const void* weights, const uint64_t* prefix, int64_t* hist,
                                   int where, void* stream, size_t stage_bytes);
MOD16_API int mod16_zonal_hist_f32(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const float* values,
                                   const void* zones, const void* weights, const uint64_t* prefix, int64_t* hist,
                                   int where, void* stream, size_t stage_bytes);
MOD16_API int mod16_zonal_select(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const int64_t* hist,
                                 const int64_t* q_mant, const int32_t* q_exp, int64_t* remaining, uint64_t* prefix,
                                 void* out_values, int64_t* weight, int where, void* stream);
MOD16_API int mod16_zonal_hist_lds_bytes(void);

/*
 * Composites over coarse-grid meteorology (ABI 16; mod16_amd.evapotranspiration_composite_downscaled,
 * DownscaleGrid.composite): the period totals of mod16_et_composite_* for a contiguous range of pixels
 * of a grid handle's fine raster, with any of the 15 arrays (the 14 drivers and day_hours) a series
 * of COARSE planes interpolated per pixel inside the kernel -- a year of daily reanalysis stays on its
 * own grid, the interpolated values never touch memory. No new numerics: the result is what
 * mod16_et_composite_* gives on the arrays the "value" rule of mod16_et_downscaled_* materialises
 * slab by slab, bit for bit (counts included), with the same flags.
 *
 *   spec        `composite`: as for mod16_et_composite_* -- n is the number of pixels of the range;
 *               fine arrays, cls and the outputs are addressed from the range's first pixel (element 0
 *               is pixel first_pixel of the raster, row-major). coarse_mask: bit k set = driver k is
 *               coarse, bit 14 = day_hours (they are a function of latitude and day). A coarse array
 *               is ceil(days / every) planes [coarse_rows][coarse_pitch], time_stride elements apart
 *               (one plane where every >= days: constant in time); its pixel stride is not looked at.
 *               All coarse arrays share the grid and coarse_pitch >= coarse_cols; each has its own time
 *               stride. A NaN cell makes the interpolant NaN where it has weight: that day is not
 *               counted (see "result" of mod16_et_composite_*); nothing is renormalised.
 *   float32     coarse and fine values widened; interpolation, pixel function and accumulation in
 *               float64; one rounding on store.
 *   flags       MOD16_MATH_FAST (0) or MOD16_MATH_EXACT; guarded as mod16_et_composite_*: a second
 *               kernel recomputes all periods of the pixels with a flagged day. No atomics on results,
 *               no workspace: two calls give the same bits.
 *   where       MOD16_DEVICE: device pointers, asynchronous on `stream` (mod16_check_status reports a
 *               class code >= 13). MOD16_HOST: host pointers; the coarse series are uploaded whole,
 *               once per call, before the first pixel tile (MOD16_ERR_NOMEM where there is no room:
 *               11 x 365 planes of 361 x 576 float64 are 6.7 GB); the fine arrays, the class raster
 *               and the outputs go through the tile staging of mod16_et_composite_* (stage_bytes as
 *               there), each tile launched with its own first pixel. The result does not depend on
 *               stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work; "mod16_et_composite_downscaled: ...")
 *               everything mod16_et_composite_* refuses, with its texts (a coarse array's pixel stride
 *               apart); "the grid was created on another device than this context's"; "the pixel
 *               range [first_pixel, first_pixel + n) leaves the raster"; "coarse_mask has a bit above
 *               14"; "coarse_pitch must be at least coarse_cols"; "a coarse plane with its pitch must
 *               hold at most 2^31 - 1 elements" (this entry only: the kernel's cell offsets are
 *               32-bit); "time stride of a coarse array with several slabs must be at least a plane"
 *               ((coarse_rows - 1) coarse_pitch + coarse_cols elements); a NULL grid or spec;
 *               "MOD16_MATH_MIXED is not available for the composite run" and "MOD16_DOMAIN_TRUSTED is
 *               not available for the composite run". n = 0 is MOD16_OK.
 */
typedef struct mod16_composite_downscaled_spec {
    mod16_composite_spec composite;              /* n: the pixels of the range */
    uint32_t coarse_mask;                        /* bit k: driver k is coarse; bit 14: day_hours */
    uint32_t reserved_;
    int64_t coarse_pitch;                        /* elements between two rows of a coarse plane */
    int64_t first_pixel;                         /* the range's first pixel in the raster */
} mod16_composite_downscaled_spec;
MOD16_API int mod16_et_composite_downscaled_f64(mod16_ctx* ctx, const mod16_downscale* grid,
                                                const mod16_composite_downscaled_spec* spec, const uint8_t* cls,
                                                const double* const* drivers, const double* day_hours, double* out_et,
                                                double* out_pet, uint16_t* count_et, uint16_t* count_pet,
                                                int64_t out_pitch, unsigned flags, int where, void* stream,
                                                int64_t stage_bytes);
MOD16_API int mod16_et_composite_downscaled_f32(mod16_ctx* ctx, const mod16_downscale* grid,
                                                const mod16_composite_downscaled_spec* spec, const uint8_t* cls,
                                                const float* const* drivers, const float* day_hours, float* out_et,
                                                float* out_pet, uint16_t* count_et, uint16_t* count_pet,
                                                int64_t out_pitch, unsigned flags, int where, void* stream,
                                                int64_t stage_bytes);

/*
 * Whittaker smoothing of 8-day series, weighted by QC (added under ABI 16, new symbols only;
 * mod16_amd.smooth_series, RasterEngine.smooth): the step behind -- or instead of -- mod16_gapfill_u8.
 * One launch smooths the profile of every pixel. The definition is the numpy statement
 * mod16_amd/smooth.py (weights_of, penalty_bands, factor, solve, encode):
 *
 *   inputs      values[t * in_pitch + i], slab t (0 ... slabs - 1, slabs 1 ... mod16_smooth_max_slabs()
 *               = 4096), pixel i: uint8 codes (missing where >= 249), float32 or float64 (missing where
 *               not finite). weight_mode MOD16_SMOOTH_WEIGHT_NONE: w = 1, `weights` is NULL;
 *               _STACK: `weights` is float32 [t * weight_pitch + i], the slab is missing unless w is
 *               finite and > 0; _QC: `weights` is a uint8 QC layer of that layout and w =
 *               qc_weight256[qc] (256 float64, finite and >= 0; NULL: 1.0 for the codes mod16_gapfill_u8
 *               accepts by default, else 0.0), the slab is missing where that is 0. A missing slab has
 *               w = 0 and y = 0. count = the slabs with w > 0.
 *   result      per pixel, in float64 and without contraction, with a0, a1, a2 the diagonals of D'D (D:
 *               the difference matrix of `order` 1 or 2; all zero where slabs <= order), terms with an
 *               index below 0 being 0.0:
 *                 d[i] = ((w[i] + lam*a0[i]) - (c[i-1]*c[i-1])*d[i-1]) - (e[i-2]*e[i-2])*d[i-2]
 *                 c[i] = (lam*a1[i] - (d[i-1]*c[i-1])*e[i-1]) / d[i]
 *                 e[i] = (lam*a2[i]) / d[i]
 *                 f[i] = (w[i]*y[i] - c[i-1]*f[i-1]) - e[i-2]*f[i-2]             i ascending
 *                 z[i] = (f[i]/d[i] - c[i]*z[i+1]) - e[i]*z[i+2]                 i descending
 *               then `envelope` (0 ... 8) times: y[t] = z[t] where w[t] > 0 and z[t] > y[t], and f, z
 *               again with the same d, c, e.
 *   outputs     out[t * out_pitch + i] of out_type: MOD16_SMOOTH_F32 / _F64 (T)(z * scale),
 *               MOD16_SMOOTH_U8 clip(floor(z + 0.5), 0, 248); a pixel with count < min_valid (min_valid >=
 *               order) is unsmoothed: NaN, or 255, in every slab. mod16_smooth_u8 takes any out_type (scale
 *               is looked at for its float outputs only), mod16_smooth_f32 / _f64 their own. Optional
 *               count[i], uint16. Every element [t][0, n) is written exactly once; [t][n, pitch) is not
 *               touched. Pointers may have any alignment of their type and the pitches any value >= n
 *               (in elements). No atomics: two calls give the same bits.
 *   workspace   the columns c, e, f/d (then z) and, with an envelope, y and d of the pixels in flight live
 *               in one block of device memory the context owns (at most 256 MiB, allocated on first use,
 *               kept); launches of one context on several streams are ordered one behind the other.
 *   where       MOD16_DEVICE: device pointers (qc_weight256 too), asynchronous on `stream`. MOD16_HOST:
 *               host pointers; pixel tiles are staged through the context's slabs as for
 *               mod16_gapfill_u8 (stage_bytes as there). The result does not depend on stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work and before an output is touched; "mod16_smooth: ...")
 *               NULL spec, values or out; n < 0; "slabs must be between 1 and 4096"; "order must be 1 or
 *               2"; "envelope must be between 0 and 8"; "min_valid must be at least the order"; "lam must
 *               be finite and > 0"; an unknown out_type or one the entry point does not give; an unknown
 *               weight_mode; weights given without a mode or a mode without weights; qc_weight256
 *               without MOD16_SMOOTH_WEIGHT_QC, or (HOST) with an entry that is not finite or negative; a
 *               scale that is not finite; a pitch below n; `where` other than the two modes; "an output
 *               overlaps an input or another output". n = 0 is MOD16_OK.
 */
enum mod16_smooth_out { MOD16_SMOOTH_U8 = 0, MOD16_SMOOTH_F32 = 1, MOD16_SMOOTH_F64 = 2 };
enum mod16_smooth_weight { MOD16_SMOOTH_WEIGHT_NONE = 0, MOD16_SMOOTH_WEIGHT_STACK = 1, MOD16_SMOOTH_WEIGHT_QC = 2 };
typedef struct mod16_smooth_spec {
    int64_t n;                                   /* pixels */
    int32_t slabs, order, envelope, min_valid;
    int32_t weight_mode, out_type;               /* enum mod16_smooth_weight, enum mod16_smooth_out */
    double lam, scale;                           /* scale: float outputs of uint8 values only */
    int64_t in_pitch, weight_pitch, out_pitch;   /* elements between two slabs */
} mod16_smooth_spec;
MOD16_API int mod16_smooth_u8(mod16_ctx* ctx, const mod16_smooth_spec* spec, const uint8_t* values, const void* weights,
                              const double* qc_weight256, void* out, uint16_t* count, int where, void* stream,
                              size_t stage_bytes);
MOD16_API int mod16_smooth_f32(mod16_ctx* ctx, const mod16_smooth_spec* spec, const float* values, const void* weights,
                               const double* qc_weight256, void* out, uint16_t* count, int where, void* stream,
                               size_t stage_bytes);
MOD16_API int mod16_smooth_f64(mod16_ctx* ctx, const mod16_smooth_spec* spec, const double* values, const void* weights,
                               const double* qc_weight256, void* out, uint16_t* count, int where, void* stream,
                               size_t stage_bytes);
MOD16_API int mod16_smooth_max_slabs(void);

/*
 * Per-pixel weighted least squares over a stack, with shared and per-pixel terms (added under ABI 16, new
 * symbols only; mod16_amd.regress_series, RasterEngine.regress): y = X b fitted for every pixel in one
 * launch -- a harmonic model plus trend over a long 8-day record, an OLS trend, ET regressed on
 * precipitation, net radiation and VPD stacks. The definition is the numpy statement
 * mod16_amd/regress.py (accumulate, factor, solve, residual_sums, inverse_diagonal):
 *
 *   inputs      values[i * value_pitch + p], step i (0 ... steps - 1, steps 1 ... mod16_regress_max_steps()
 *               = 4096), pixel p, float32 or float64 (widened to float64; missing where not finite).
 *               The predictors of a sample are x[0 .. P - 1], P = ks + kp between 1 and
 *               mod16_regress_max_terms() = 8: first the ks columns design[i * ks + a] (float64, the same
 *               for every pixel, finite), then the kp per-pixel stacks terms[k][i * term_pitch + p] of the
 *               values' type. weights: NULL (w = 1) or float32 [i * weight_pitch + p]. A sample is valid
 *               where y and every per-pixel term are finite and the weight is finite and > 0; count = the
 *               valid samples.
 *   result      per pixel, in float64 and without contraction, the valid samples in ascending i:
 *                 wx[a] = w * x[a];  h[a] += wx[a] * y;  G[a][b] += wx[a] * x[b] (b >= a);  Sw += w;  Sy += w * y
 *               G = L diag(d) L' without pivoting, column by column (k = 0 .. j - 1):
 *                 d[j]    = (G[j][j] - (L[j][0] * L[j][0]) * d[0]) - ...
 *                 L[i][j] = ((G[j][i] - (L[i][0] * L[j][0]) * d[0]) - ...) / d[j]
 *               the pixel is degenerate if a test d[j] > 2^-40 * G[j][j] fails (a NaN fails it);
 *                 z[i] = (h[i] - L[i][0] * z[0]) - ...;  c[i] = z[i] / d[i];  b[i] = (c[i] - L[i+1][i] * b[i+1]) - ...
 *               and over the samples again: f = (x[0] * b[0] + x[1] * b[1]) + ..., r = y - f,
 *                 rss += w * (r * r);  tss += w * ((y - Sy / Sw) * (y - Sy / Sw))
 *               r2 = 1 - rss / tss, sigma2 = rss / (count - P), se[j] = sqrt(sigma2 * inv[j]) with inv the
 *               diagonal of the inverse of L diag(d) L' (regress.py: inverse_diagonal). Nothing is
 *               special-cased: count == P gives what 0 / 0 or x / 0 gives.
 *   outputs     coef[j * coef_pitch + p]; optional se[j * se_pitch + p], rss[p], tss[p], r2[p] (float64),
 *               count[p] (uint16) and series[i * series_pitch + p] in the values' type:
 *               MOD16_REGRESS_SERIES_RESIDUALS r, NaN where the sample is not valid; _FITTED f wherever every
 *               per-pixel term of the step is finite (with ks = P: every step). Where count < min_valid
 *               (min_valid >= P) or the pixel is degenerate every float output is NaN; count is kept.
 *               Every element [.][0, n) is written exactly once; [.][n, pitch) is not touched. Pointers may
 *               have any alignment of their type and the pitches any value >= n (in elements). No atomics:
 *               two calls give the same bits.
 *   where       MOD16_DEVICE: device pointers (design too; `terms` itself is a host array of kp device
 *               pointers), asynchronous on `stream`. MOD16_HOST: host pointers; pixel tiles are staged
 *               through the context's slabs as for mod16_smooth_*, the design is uploaded whole to memory
 *               the context owns (stage_bytes as there). The result does not depend on stage_bytes.
 *   refused (MOD16_ERR_ARG, before any device work and before an output is touched; "mod16_regress: ...")
 *               NULL spec, values or coef; n < 0; "steps must be between 1 and 4096"; ks or kp negative or
 *               ks + kp outside 1 ... 8; design given without ks or ks without design, likewise terms and
 *               kp; a NULL term; "min_valid must be at least ks + kp"; an unknown series mode, or a series
 *               output without a mode or a mode without the output; a pitch below n; (HOST) "design must be
 *               finite"; `where` other than the two modes; "an output overlaps an input or another
 *               output". n = 0 is MOD16_OK.
 */
enum mod16_regress_series { MOD16_REGRESS_SERIES_NONE = 0, MOD16_REGRESS_SERIES_RESIDUALS = 1, MOD16_REGRESS_SERIES_FITTED = 2 };
typedef struct mod16_regress_spec {
    int64_t n;                                   /* pixels */
    int32_t steps, ks, kp, min_valid;
    int32_t series, flags;                       /* enum mod16_regress_series; flags: 0 */
    int64_t value_pitch, term_pitch, weight_pitch;   /* elements between two steps */
    int64_t coef_pitch, se_pitch, series_pitch;      /* elements between two coefficients, two steps */
} mod16_regress_spec;
MOD16_API int mod16_regress_f32(mod16_ctx* ctx, const mod16_regress_spec* spec, const float* values, const double* design,
                                const float* const* terms, const float* weights, double* coef, double* se, double* rss,
                                double* tss, double* r2, uint16_t* count, float* series, int where, void* stream,
                                size_t stage_bytes);
MOD16_API int mod16_regress_f64(mod16_ctx* ctx, const mod16_regress_spec* spec, const double* values, const double* design,
                                const double* const* terms, const float* weights, double* coef, double* se, double* rss,
                                double* tss, double* r2, uint16_t* count, double* series, int where, void* stream,
                                size_t stage_bytes);
MOD16_API int mod16_regress_max_steps(void);
MOD16_API int mod16_regress_max_terms(void);

#ifdef __cplusplus
}
#endif
#endif /* MOD16_HIP_H */
