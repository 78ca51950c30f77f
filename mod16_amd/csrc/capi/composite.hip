// libmod16hip.so -- multi-day ET composites: mod16_et_composite_* (per-pixel period totals of ET, and potential ET, over K days of drivers in one launch)
#include "host.hpp"
#include "../mod16_composite.hpp"

// What the entry point has checked: the kernels' arguments (device pointers, or host pointers in
// front of the staging path), the potential-ET outputs wanted or not, the periods.
template <typename T> struct CompCall {
    CompArgs<T> a;
    bool pet;
    int periods;
    int slabs[kCompArrays];        // time slabs of every array: ceil(days / every)
    int64_t stage_bytes;
};

// All pointers are device pointers here.
template <typename T>
static int launch_composite(mod16_ctx* ctx, CompArgs<T> a, bool pet, unsigned flags, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    a.lut64 = ctx->lut64.as<double>();
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    const int64_t nbatch = (a.n + kBlock - 1) / kBlock;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t)ctx->cus * 8));
    if (flags & MOD16_MATH_EXACT) {
        if (pet) hipLaunchKernelGGL((comp_kernel<T, false, true>), dim3(grid), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((comp_kernel<T, false, false>), dim3(grid), dim3(kBlock), 0, st, a);
    } else if (pet) {
        hipLaunchKernelGGL((comp_kernel<T, true, true>), dim3(grid), dim3(kBlock), 0, st, a);
        // pixels with a day outside the domain of the fast arithmetic: the kernel above left a mark
        // in period 0 of their out_et, this one computes all their periods
        hipLaunchKernelGGL((comp_redo_kernel<T, true>), dim3(grid), dim3(kBlock), 0, st, a);
    } else {
        hipLaunchKernelGGL((comp_kernel<T, true, false>), dim3(grid), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL((comp_redo_kernel<T, false>), dim3(grid), dim3(kBlock), 0, st, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: every time slab of the 15 arrays, the periods of the outputs and counts, the class
// raster -- through the shared staging path, the tile cut so that a slot's slab fits stage_bytes
template <typename T>
static int composite_host(mod16_ctx* ctx, const CompCall<T>& h, unsigned flags) {
    const CompArgs<T>& a = h.a;
    const int64_t n = a.n;
    const int P = h.periods;
    HostPlan p(sizeof(T));
    for (int k = 0; k < kCompArrays; ++k) {
        if ((a.dense >> k) & 1u) p.add(kIn, a.arr[k], false, h.slabs[k], a.tstride[k]);
        else p.add(kScalar, a.arr[k]);
    }
    p.add(kOut, a.out_et, false, P, a.out_pitch);
    p.add(kOut, a.out_pet, false, a.out_pet ? P : 1, a.out_pitch);
    p.add(kOut, a.cnt_et, false, a.cnt_et ? P : 1, a.cnt_pitch, sizeof(uint16_t));
    p.add(kOut, a.cnt_pet, false, a.cnt_pet ? P : 1, a.cnt_pitch, sizeof(uint16_t));
    p.add(kIn, a.cls, true);
    p.cls = a.cls;
    // a slab holds the rows back to back (whole tiles of 256 pixels: no rounding), the stagger once per
    // array, the class bytes: a year of daily drivers (some 3900 rows of float64) still gets tiles of
    // 4096 pixels out of the default 128 MiB
    const int64_t fixed = (int64_t)p.nwide * (int64_t)kStagger + 512;
    const int64_t per_pixel = (int64_t)p.wide_rows * (int64_t)sizeof(T) + 1;
    int64_t tile = (h.stage_bytes - fixed) / per_pixel / kBlock * kBlock;
    tile = std::max<int64_t>(kBlock, std::min<int64_t>(tile, kTilePixels));
    auto launch = [&](const HostTile& t) {
        CompArgs<T> d = a;
        d.n = t.m;
        for (int k = 0; k < kCompArrays; ++k) {
            d.arr[k] = static_cast<const T*>(t.dev[k]);
            d.tstride[k] = ((a.dense >> k) & 1u) ? (int64_t)(t.row_bytes / sizeof(T)) : 0;
        }
        d.out_et = static_cast<T*>(t.dev[kCompArrays]);
        d.out_pet = static_cast<T*>(t.dev[kCompArrays + 1]);
        d.cnt_et = static_cast<uint16_t*>(t.dev[kCompArrays + 2]);
        d.cnt_pet = static_cast<uint16_t*>(t.dev[kCompArrays + 3]);
        d.cls = static_cast<const uint8_t*>(t.dev[kCompArrays + 4]);
        d.out_pitch = (int64_t)(t.row_bytes / sizeof(T));
        d.cnt_pitch = (int64_t)(t.row_bytes / sizeof(uint16_t));
        return launch_composite<T>(ctx, d, h.pet, flags, t.st);
    };
    // (pipeline = false: these kernels use none of the stream pipeline's workspace; the status word --
    // a class code >= 13 -- is read back here)
    const int rc = host_tiled(ctx, p, n, ctx->host_threads, false, launch, nullptr, tile);
    return rc == MOD16_OK ? read_status(ctx, ctx->streams[0]) : rc;
}

template <typename T>
static int composite_entry(mod16_ctx* ctx, const mod16_composite_spec* spec, const uint8_t* cls,
                           const T* const* drivers, const T* day_hours, T* out_et, T* out_pet,
                           uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch, unsigned flags,
                           int where, void* stream, int64_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_et_composite: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!spec || !cls || !drivers || !day_hours || !out_et) return bad("NULL spec, class raster, drivers, day_hours or out_et");
    if (spec->n < 0) return bad("n < 0");
    if (flags & MOD16_MATH_MIXED)
        return bad("MOD16_MATH_MIXED is not available for the composite run (MOD16_MATH_FAST or MOD16_MATH_EXACT)");
    if (flags & MOD16_DOMAIN_TRUSTED)
        return bad("MOD16_DOMAIN_TRUSTED is not available for the composite run (every launch is guarded)");
    if (flags & ~(unsigned)MOD16_MATH_EXACT) return bad("unknown flag");
    if (spec->days < 1 || spec->days > kCompMaxDays) return bad("days must be between 1 and 4096");
    if (spec->period_days < 1) return bad("period_days must be at least 1");
    if (spec->min_valid < 1 || spec->min_valid > spec->period_days) return bad("min_valid must be between 1 and period_days");
    if (spec->rescale != 0 && spec->rescale != 1) return bad("rescale must be 0 or 1");
    if (count_pet && !out_pet) return bad("count_pet needs out_pet");
    if (out_pitch < spec->n) return bad("out_pitch must be at least n");
    if (stage_bytes < 0) return bad("stage_bytes must not be negative");
    if (where != MOD16_DEVICE && where != MOD16_HOST) return bad("`where` must be MOD16_HOST or MOD16_DEVICE");
    CompCall<T> c;
    memset(&c, 0, sizeof c);
    for (int k = 0; k < kCompArrays; ++k) {
        const bool hours = k == kCompHours;
        const T* ptr = hours ? day_hours : drivers[k];
        const int64_t ps = hours ? spec->hours_pixel_stride : spec->pixel_stride[k];
        const int64_t ts = hours ? spec->hours_time_stride : spec->time_stride[k];
        const int ev = hours ? spec->hours_every : spec->every[k];
        if (!ptr) return bad("NULL driver array");
        if (ps != 0 && ps != 1) return bad("pixel stride must be 0 or 1");
        if (ev < 1) return bad("every must be at least 1");
        if (ts < 0) return bad("time stride must not be negative");
        const int evc = std::min(ev, spec->days);      // (every >= days is one slab: no overflow in the sum below)
        c.slabs[k] = (spec->days + evc - 1) / evc;
        if (ps == 0 && c.slabs[k] != 1) return bad("a broadcast scalar (pixel stride 0) is constant in time: its every must be at least days");
        if (ps == 1 && c.slabs[k] > 1 && ts < spec->n) return bad("time stride of an array with several slabs must be at least n");
        c.a.arr[k] = ptr;
        c.a.tstride[k] = c.slabs[k] > 1 ? ts : 0;
        c.a.every[k] = evc;
        if (ps == 1) c.a.dense |= 1u << k;
    }
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, "mod16_et_composite: mod16_set_bplut_f64 was not called");
    if (spec->n == 0) return MOD16_OK;
    c.a.cls = cls;
    c.a.out_et = out_et;
    c.a.out_pet = out_pet;
    c.a.cnt_et = count_et;
    c.a.cnt_pet = count_pet;
    c.a.out_pitch = c.a.cnt_pitch = out_pitch;
    c.a.n = spec->n;
    c.a.days = spec->days;
    c.a.period_days = spec->period_days;
    c.a.min_valid = spec->min_valid;
    c.a.rescale = spec->rescale;
    c.pet = out_pet != nullptr;
    c.periods = (spec->days + spec->period_days - 1) / spec->period_days;
    c.stage_bytes = stage_bytes ? stage_bytes : (int64_t)128 << 20;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_composite<T>(ctx, c.a, c.pet, flags, static_cast<hipStream_t>(stream));
    return composite_host<T>(ctx, c, flags);
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
