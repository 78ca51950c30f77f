// libmod16hip.so -- multi-day ET composites over coarse-grid meteorology: mod16_et_composite_downscaled_* (the period totals of mod16_et_composite_* with any of the 15 arrays a series of coarse planes interpolated per pixel inside the kernel)
#include "composite_call.hpp"
#include "downscale_grid.hpp"
#include "../mod16_composite_downscale.hpp"

// the kernels of one geometry (G: DsGrid or DsRowsGrid)
template <typename T, typename G> struct CdKernels {
    template <bool FAST, bool PET> static auto main() { return &cd_kernel<T, FAST, PET, G>; }
    template <bool PET> static auto redo() { return &cd_redo_kernel<T, PET, G>; }
};

// All pointers are device pointers here. The handle's geometry picks the instances.
template <typename T>
static int launch_composite_downscaled(mod16_ctx* ctx, const mod16_downscale* grid, const CompArgs<T>& a, uint32_t coarse,
                                       int64_t cpitch, int64_t first, bool pet, unsigned flags, hipStream_t st) {
    return ds_dispatch(grid, [&](const auto& g) {
        using G = std::decay_t<decltype(g)>;
        CdArgs<T, G> b;
        memset(&b, 0, sizeof b);
        b.c = comp_with_tables(ctx, a);
        b.coarse = coarse;
        b.g = g;
        b.cpitch = cpitch;
        b.first = first;
        return comp_launch<CdKernels<T, G>>(ctx, b, a.n, pet, flags, st);
    });
}

// HOST mode: the coarse series resident, planes and rows back to back; everything else as
// composite.hip stages it
template <typename T>
static int composite_downscaled_host(mod16_ctx* ctx, const mod16_downscale* grid, const CompCall<T>& h, int64_t cpitch,
                                     int64_t first, unsigned flags) {
    const T* series[kCompArrays];
    const T* dev[kCompArrays];
    for (int k = 0; k < kCompArrays; ++k) series[k] = ((h.coarse >> k) & 1u) ? h.a.arr[k] : nullptr;
    const int rc = upload_coarse<T>(ctx, grid, series, h.slabs, h.a.tstride, cpitch, kCompArrays, "coarse series", dev);
    if (rc != MOD16_OK) return rc;
    const int64_t W = grid->spec.coarse_cols;
    return comp_host<T>(ctx, h, dev, grid->spec.coarse_rows * W, [&](const CompArgs<T>& d, const HostTile& t) {
        return launch_composite_downscaled<T>(ctx, grid, d, h.coarse, W, first + t.off, h.pet, flags, t.st);
    });
}

template <typename T>
static int composite_downscaled_entry(mod16_ctx* ctx, const mod16_downscale* grid,
                                      const mod16_composite_downscaled_spec* dspec, const uint8_t* cls,
                                      const T* const* drivers, const T* day_hours, T* out_et, T* out_pet,
                                      uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch, unsigned flags,
                                      int where, void* stream, int64_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    const char* const prefix = "mod16_et_composite_downscaled: ";
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, prefix, what); };
    if (!grid || !dspec || !cls || !drivers || !day_hours || !out_et)
        return bad("NULL grid, spec, class raster, drivers, day_hours or out_et");
    const mod16_composite_spec* spec = &dspec->composite;
    int rc = comp_check_spec(ctx, prefix, spec, out_pet, count_pet, out_pitch, flags, where, stage_bytes);
    if (rc != MOD16_OK) return rc;
    if (grid->device != ctx->device) return bad("the grid was created on another device than this context's");
    const int64_t total = grid->spec.rows * grid->spec.cols;
    const int64_t first = dspec->first_pixel;
    if (first < 0 || first > total || spec->n > total - first)
        return bad("the pixel range [first_pixel, first_pixel + n) leaves the raster");
    if (dspec->coarse_mask >> kCompArrays) return bad("coarse_mask has a bit above 14 (the hours of daylight)");
    const int64_t H = grid->spec.coarse_rows, W = grid->spec.coarse_cols;
    int64_t span = 0;              // the elements of a coarse plane, from its first to its last cell
    if (dspec->coarse_mask) {
        if (dspec->coarse_pitch < W) return bad("coarse_pitch must be at least coarse_cols");
        // ((H - 1) pitch + W, both factors below 2^62 / 2^30: no overflow before the comparison)
        if (dspec->coarse_pitch > std::numeric_limits<int32_t>::max() ||
            (span = (H - 1) * dspec->coarse_pitch + W) > std::numeric_limits<int32_t>::max())
            return bad("a coarse plane with its pitch must hold at most 2^31 - 1 elements");
    }
    CompCall<T> c;
    memset(&c, 0, sizeof c);
    rc = comp_check_arrays<T>(ctx, prefix, spec, drivers, day_hours, dspec->coarse_mask, span, c);
    if (rc != MOD16_OK) return rc;
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, prefix, "mod16_set_bplut_f64 was not called");
    if (spec->n == 0) return MOD16_OK;
    comp_fill<T>(c, spec, cls, out_et, out_pet, count_et, count_pet, out_pitch, stage_bytes);
    const int64_t cpitch = dspec->coarse_mask ? dspec->coarse_pitch : W;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE)
        return launch_composite_downscaled<T>(ctx, grid, c.a, c.coarse, cpitch, first, c.pet, flags, static_cast<hipStream_t>(stream));
    return composite_downscaled_host<T>(ctx, grid, c, cpitch, first, flags);
}

extern "C" int mod16_et_composite_downscaled_f64(mod16_ctx* ctx, const mod16_downscale* grid,
                                                 const mod16_composite_downscaled_spec* spec, const uint8_t* cls,
                                                 const double* const* drivers, const double* day_hours, double* out_et,
                                                 double* out_pet, uint16_t* count_et, uint16_t* count_pet,
                                                 int64_t out_pitch, unsigned flags, int where, void* stream,
                                                 int64_t stage_bytes) {
    MOD16_LOCK(ctx);
    return composite_downscaled_entry<double>(ctx, grid, spec, cls, drivers, day_hours, out_et, out_pet, count_et,
                                              count_pet, out_pitch, flags, where, stream, stage_bytes);
}
extern "C" int mod16_et_composite_downscaled_f32(mod16_ctx* ctx, const mod16_downscale* grid,
                                                 const mod16_composite_downscaled_spec* spec, const uint8_t* cls,
                                                 const float* const* drivers, const float* day_hours, float* out_et,
                                                 float* out_pet, uint16_t* count_et, uint16_t* count_pet,
                                                 int64_t out_pitch, unsigned flags, int where, void* stream,
                                                 int64_t stage_bytes) {
    MOD16_LOCK(ctx);
    return composite_downscaled_entry<float>(ctx, grid, spec, cls, drivers, day_hours, out_et, out_pet, count_et,
                                             count_pet, out_pitch, flags, where, stream, stage_bytes);
}
