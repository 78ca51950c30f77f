// libmod16hip.so -- multi-day ET composites: mod16_et_composite_* (per-pixel period totals of ET, and potential ET, over K days of drivers in one launch)
#include "composite_call.hpp"

template <typename T> struct CompKernels {
    template <bool FAST, bool PET> static auto main() { return &comp_kernel<T, FAST, PET>; }
    template <bool PET> static auto redo() { return &comp_redo_kernel<T, PET>; }
};

// All pointers are device pointers here.
template <typename T>
static int launch_composite(mod16_ctx* ctx, const CompArgs<T>& a, bool pet, unsigned flags, hipStream_t st) {
    return comp_launch<CompKernels<T>>(ctx, comp_with_tables(ctx, a), a.n, pet, flags, st);
}

template <typename T>
static int composite_entry(mod16_ctx* ctx, const mod16_composite_spec* spec, const uint8_t* cls,
                           const T* const* drivers, const T* day_hours, T* out_et, T* out_pet,
                           uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch, unsigned flags,
                           int where, void* stream, int64_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    const char* const prefix = "mod16_et_composite: ";
    if (!spec || !cls || !drivers || !day_hours || !out_et)
        return fail(ctx, MOD16_ERR_ARG, prefix, "NULL spec, class raster, drivers, day_hours or out_et");
    int rc = comp_check_spec(ctx, prefix, spec, out_pet, count_pet, out_pitch, flags, where, stage_bytes);
    if (rc != MOD16_OK) return rc;
    CompCall<T> c;
    memset(&c, 0, sizeof c);
    rc = comp_check_arrays<T>(ctx, prefix, spec, drivers, day_hours, 0u, 0, c);
    if (rc != MOD16_OK) return rc;
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, prefix, "mod16_set_bplut_f64 was not called");
    if (spec->n == 0) return MOD16_OK;
    comp_fill<T>(c, spec, cls, out_et, out_pet, count_et, count_pet, out_pitch, stage_bytes);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_composite<T>(ctx, c.a, c.pet, flags, static_cast<hipStream_t>(stream));
    return comp_host<T>(ctx, c, nullptr, 0, [&](const CompArgs<T>& d, const HostTile& t) {
        return launch_composite<T>(ctx, d, c.pet, flags, t.st);
    });
}

extern "C" int mod16_et_composite_f64(mod16_ctx* ctx, const mod16_composite_spec* spec, const uint8_t* cls,
                                      const double* const* drivers, const double* day_hours, double* out_et,
                                      double* out_pet, uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch,
                                      unsigned flags, int where, void* stream, int64_t stage_bytes) {
    MOD16_LOCK(ctx);
    return composite_entry<double>(ctx, spec, cls, drivers, day_hours, out_et, out_pet, count_et, count_pet,
                                   out_pitch, flags, where, stream, stage_bytes);
}
extern "C" int mod16_et_composite_f32(mod16_ctx* ctx, const mod16_composite_spec* spec, const uint8_t* cls,
                                      const float* const* drivers, const float* day_hours, float* out_et,
                                      float* out_pet, uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch,
                                      unsigned flags, int where, void* stream, int64_t stage_bytes) {
    MOD16_LOCK(ctx);
    return composite_entry<float>(ctx, spec, cls, drivers, day_hours, out_et, out_pet, count_et, count_pet,
                                  out_pitch, flags, where, stream, stage_bytes);
}
