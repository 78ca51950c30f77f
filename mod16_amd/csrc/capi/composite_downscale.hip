// libmod16hip.so -- multi-day ET composites over coarse-grid meteorology: mod16_et_composite_downscaled_* (the period totals of mod16_et_composite_* with any of the 15 arrays a series of coarse planes interpolated per pixel inside the kernel)
#include "downscale_grid.hpp"
#include "../mod16_composite_downscale.hpp"

// What the entry point has checked: the kernels' arguments (device pointers, or host pointers in
// front of the staging path), the potential-ET outputs wanted or not, the periods.
template <typename T> struct CdCall {
    CdArgs<T> a;
    bool pet;
    int periods;
    int slabs[kCompArrays];        // time slabs of every array: ceil(days / every)
    int64_t stage_bytes;
};

// the kernels of one geometry (G: DsGrid or DsRowsGrid)
template <typename T, typename G>
static void launch_composite_downscaled_on(const CdArgs<T>& a, const G& g, int blocks, bool pet, unsigned flags, hipStream_t st) {
    CdArgs<T, G> b;
    memset(&b, 0, sizeof b);
    b.c = a.c;
    b.coarse = a.coarse;
    b.g = g;
    b.cpitch = a.cpitch;
    b.first = a.first;
    if (flags & MOD16_MATH_EXACT) {
        if (pet) hipLaunchKernelGGL((cd_kernel<T, false, true, G>), dim3(blocks), dim3(kBlock), 0, st, b);
        else hipLaunchKernelGGL((cd_kernel<T, false, false, G>), dim3(blocks), dim3(kBlock), 0, st, b);
    } else if (pet) {
        hipLaunchKernelGGL((cd_kernel<T, true, true, G>), dim3(blocks), dim3(kBlock), 0, st, b);
        // pixels with a day outside the domain of the fast arithmetic: the kernel above left a mark
        // in period 0 of their out_et, this one computes all their periods
        hipLaunchKernelGGL((cd_redo_kernel<T, true, G>), dim3(blocks), dim3(kBlock), 0, st, b);
    } else {
        hipLaunchKernelGGL((cd_kernel<T, true, false, G>), dim3(blocks), dim3(kBlock), 0, st, b);
        hipLaunchKernelGGL((cd_redo_kernel<T, false, G>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
}

// All pointers are device pointers here. The handle's geometry picks the instances.
template <typename T>
static int launch_composite_downscaled(mod16_ctx* ctx, const mod16_downscale* grid, CdArgs<T> a, bool pet, unsigned flags,
                                       hipStream_t st) {
    if (a.c.n <= 0) return MOD16_OK;
    a.c.lut64 = ctx->lut64.as<double>();
    a.c.tab = ctx->tab64.as<double>();
    a.c.status = ctx->status.as<unsigned>();
    const int64_t nbatch = (a.c.n + kBlock - 1) / kBlock;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t)ctx->cus * 8));
    if (grid->affine) launch_composite_downscaled_on<T, DsRowsGrid>(a, grid->gr, blocks, pet, flags, st);
    else launch_composite_downscaled_on<T, DsGrid>(a, grid->g, blocks, pet, flags, st);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: every coarse series of the call uploaded whole, once, planes and rows back to back
// (pitch = coarse_cols, time stride = a plane), into the context's buffer for resident inputs;
// dev[k] receives the address of its first plane
template <typename T>
static int cd_upload_series(mod16_ctx* ctx, const mod16_downscale* grid, const CdCall<T>& h, const T** dev) {
    const CdArgs<T>& a = h.a;
    const size_t H = (size_t)grid->spec.coarse_rows, W = (size_t)grid->spec.coarse_cols;
    size_t total = 256;
    for (int k = 0; k < kCompArrays; ++k)
        if ((a.coarse >> k) & 1u) total += align256(H * W * sizeof(T) * (size_t)h.slabs[k]);
    int rc = ctx->bc_buf.reserve(ctx, total, "HOST mode: device memory for the coarse series");
    if (rc != MOD16_OK) return rc;
    char* cur = ctx->bc_buf.as<char>();
    for (int k = 0; k < kCompArrays; ++k) {
        dev[k] = nullptr;
        if (!((a.coarse >> k) & 1u)) continue;
        // (one copy per plane where its rows lie back to back, else one per row)
        const bool packed = (size_t)a.cpitch == W;
        for (int s = 0; s < h.slabs[k]; ++s) {
            const T* plane = a.c.arr[k] + (int64_t)s * a.c.tstride[k];
            char* to = cur + (size_t)s * H * W * sizeof(T);
            const size_t rows = packed ? 1 : H, row_bytes = (packed ? H : 1) * W * sizeof(T);
            for (size_t r = 0; r < rows; ++r)
                if (hipMemcpy(to + r * W * sizeof(T), plane + r * (size_t)a.cpitch, row_bytes, hipMemcpyHostToDevice) != hipSuccess)
                    return fail(ctx, MOD16_ERR_HIP, "HOST mode: upload of a coarse plane failed");
        }
        dev[k] = reinterpret_cast<const T*>(cur);
        cur += align256(H * W * sizeof(T) * (size_t)h.slabs[k]);
    }
    return MOD16_OK;
}

// HOST mode: the coarse series resident; every time slab of the fine arrays, the periods of the
// outputs and counts, the class raster through the shared staging path as composite.hip stages them,
// the tile cut so that a slot's slab fits stage_bytes; HostTile::off gives a tile's first pixel
template <typename T>
static int composite_downscaled_host(mod16_ctx* ctx, const mod16_downscale* grid, const CdCall<T>& h, unsigned flags) {
    const CdArgs<T>& a = h.a;
    const int P = h.periods;
    const T* dev[kCompArrays];
    int rc = cd_upload_series<T>(ctx, grid, h, dev);
    if (rc != MOD16_OK) return rc;
    HostPlan p(sizeof(T));
    for (int k = 0; k < kCompArrays; ++k) {
        if ((a.coarse >> k) & 1u) {
            p.add(kResident, a.c.arr[k]);
            p.a[k].dev = const_cast<T*>(dev[k]);
        } else if ((a.c.dense >> k) & 1u) {
            p.add(kIn, a.c.arr[k], false, h.slabs[k], a.c.tstride[k]);
        } else {
            p.add(kScalar, a.c.arr[k]);
        }
    }
    p.add(kOut, a.c.out_et, false, P, a.c.out_pitch);
    p.add(kOut, a.c.out_pet, false, a.c.out_pet ? P : 1, a.c.out_pitch);
    p.add(kOut, a.c.cnt_et, false, a.c.cnt_et ? P : 1, a.c.cnt_pitch, sizeof(uint16_t));
    p.add(kOut, a.c.cnt_pet, false, a.c.cnt_pet ? P : 1, a.c.cnt_pitch, sizeof(uint16_t));
    p.add(kIn, a.c.cls, true);
    p.cls = a.c.cls;
    const int64_t fixed = (int64_t)p.nwide * (int64_t)kStagger + 512;
    const int64_t per_pixel = (int64_t)p.wide_rows * (int64_t)sizeof(T) + 1;
    int64_t tile = (h.stage_bytes - fixed) / per_pixel / kBlock * kBlock;
    tile = std::max<int64_t>(kBlock, std::min<int64_t>(tile, kTilePixels));
    const int64_t plane = grid->spec.coarse_rows * grid->spec.coarse_cols;
    auto launch = [&](const HostTile& t) {
        CdArgs<T> d = a;
        d.c.n = t.m;
        d.first = a.first + t.off;
        d.cpitch = grid->spec.coarse_cols;
        for (int k = 0; k < kCompArrays; ++k) {
            d.c.arr[k] = static_cast<const T*>(t.dev[k]);
            if ((a.coarse >> k) & 1u) d.c.tstride[k] = h.slabs[k] > 1 ? plane : 0;
            else d.c.tstride[k] = ((a.c.dense >> k) & 1u) ? (int64_t)(t.row_bytes / sizeof(T)) : 0;
        }
        d.c.out_et = static_cast<T*>(t.dev[kCompArrays]);
        d.c.out_pet = static_cast<T*>(t.dev[kCompArrays + 1]);
        d.c.cnt_et = static_cast<uint16_t*>(t.dev[kCompArrays + 2]);
        d.c.cnt_pet = static_cast<uint16_t*>(t.dev[kCompArrays + 3]);
        d.c.cls = static_cast<const uint8_t*>(t.dev[kCompArrays + 4]);
        d.c.out_pitch = (int64_t)(t.row_bytes / sizeof(T));
        d.c.cnt_pitch = (int64_t)(t.row_bytes / sizeof(uint16_t));
        return launch_composite_downscaled<T>(ctx, grid, d, h.pet, flags, t.st);
    };
    // (pipeline = false: these kernels use none of the stream pipeline's workspace; the status word --
    // a class code >= 13 -- is read back here)
    rc = host_tiled(ctx, p, a.c.n, ctx->host_threads, false, launch, nullptr, tile);
    return rc == MOD16_OK ? read_status(ctx, ctx->streams[0]) : rc;
}

template <typename T>
static int composite_downscaled_entry(mod16_ctx* ctx, const mod16_downscale* grid,
                                      const mod16_composite_downscaled_spec* dspec, const uint8_t* cls,
                                      const T* const* drivers, const T* day_hours, T* out_et, T* out_pet,
                                      uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch, unsigned flags,
                                      int where, void* stream, int64_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) {
        char msg[240];
        snprintf(msg, sizeof msg, "mod16_et_composite_downscaled: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!grid || !dspec || !cls || !drivers || !day_hours || !out_et)
        return bad("NULL grid, spec, class raster, drivers, day_hours or out_et");
    const mod16_composite_spec* spec = &dspec->composite;
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
    CdCall<T> c;
    memset(&c, 0, sizeof c);
    for (int k = 0; k < kCompArrays; ++k) {
        const bool hours = k == kCompHours;
        const bool coarse = (dspec->coarse_mask >> k) & 1u;
        const T* ptr = hours ? day_hours : drivers[k];
        const int64_t ps = hours ? spec->hours_pixel_stride : spec->pixel_stride[k];
        const int64_t ts = hours ? spec->hours_time_stride : spec->time_stride[k];
        const int ev = hours ? spec->hours_every : spec->every[k];
        if (!ptr) return bad("NULL driver array");
        if (!coarse && ps != 0 && ps != 1) return bad("pixel stride must be 0 or 1");
        if (ev < 1) return bad("every must be at least 1");
        if (ts < 0) return bad("time stride must not be negative");
        const int evc = std::min(ev, spec->days);      // (every >= days is one slab: no overflow in the sum below)
        c.slabs[k] = (spec->days + evc - 1) / evc;
        if (coarse) {
            if (c.slabs[k] > 1 && ts < span)
                return bad("time stride of a coarse array with several slabs must be at least a plane ((coarse_rows - 1) coarse_pitch + coarse_cols)");
            c.a.coarse |= 1u << k;
        } else {
            if (ps == 0 && c.slabs[k] != 1) return bad("a broadcast scalar (pixel stride 0) is constant in time: its every must be at least days");
            if (ps == 1 && c.slabs[k] > 1 && ts < spec->n) return bad("time stride of an array with several slabs must be at least n");
            if (ps == 1) c.a.c.dense |= 1u << k;
        }
        c.a.c.arr[k] = ptr;
        c.a.c.tstride[k] = c.slabs[k] > 1 ? ts : 0;
        c.a.c.every[k] = evc;
    }
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, "mod16_et_composite_downscaled: mod16_set_bplut_f64 was not called");
    if (spec->n == 0) return MOD16_OK;
    c.a.cpitch = dspec->coarse_mask ? dspec->coarse_pitch : W;
    c.a.first = first;
    c.a.c.cls = cls;
    c.a.c.out_et = out_et;
    c.a.c.out_pet = out_pet;
    c.a.c.cnt_et = count_et;
    c.a.c.cnt_pet = count_pet;
    c.a.c.out_pitch = c.a.c.cnt_pitch = out_pitch;
    c.a.c.n = spec->n;
    c.a.c.days = spec->days;
    c.a.c.period_days = spec->period_days;
    c.a.c.min_valid = spec->min_valid;
    c.a.c.rescale = spec->rescale;
    c.pet = out_pet != nullptr;
    c.periods = (spec->days + spec->period_days - 1) / spec->period_days;
    c.stage_bytes = stage_bytes ? stage_bytes : (int64_t)128 << 20;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE)
        return launch_composite_downscaled<T>(ctx, grid, c.a, c.pet, flags, static_cast<hipStream_t>(stream));
    return composite_downscaled_host<T>(ctx, grid, c, flags);
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
