// libmod16hip.so, host side: what the composite families share -- mod16_et_composite_* (composite.hip)
// and mod16_et_composite_downscaled_* (composite_downscale.hip): the checks of the spec and of the
// 15 arrays, the checked call, its HOST mode, the ladder of kernel instances. A family adds its own
// checks, its kernels and, where it has coarse arrays, their upload.
#pragma once
#include "host.hpp"
#include "../mod16_composite.hpp"

// What the entry point has checked: the kernels' arguments (device pointers, or host pointers in
// front of the staging path), the potential-ET outputs wanted or not, the periods.
template <typename T> struct CompCall {
    CompArgs<T> a;
    uint32_t coarse;               // bit k set: array k is a series of coarse planes (composite.hip: none)
    bool pet;
    int periods;
    int slabs[kCompArrays];        // time slabs of every array: ceil(days / every)
    int64_t stage_bytes;
};

// the spec, the flags and the scalar arguments of a call
static int comp_check_spec(mod16_ctx* ctx, const char* prefix, const mod16_composite_spec* spec, const void* out_pet,
                           const void* count_pet, int64_t out_pitch, unsigned flags, int where, int64_t stage_bytes) {
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, prefix, what); };
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
    if (const char* what = check_where(where)) return bad(what);
    return MOD16_OK;
}

// The 15 arrays of a call -> c.a.arr, tstride, every, dense, c.coarse, c.slabs. coarse_mask: the
// arrays that are series of coarse planes; span: the elements of such a plane, from its first to
// its last cell.
template <typename T>
static int comp_check_arrays(mod16_ctx* ctx, const char* prefix, const mod16_composite_spec* spec, const T* const* drivers,
                             const T* day_hours, uint32_t coarse_mask, int64_t span, CompCall<T>& c) {
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, prefix, what); };
    for (int k = 0; k < kCompArrays; ++k) {
        const bool hours = k == kCompHours;
        const bool coarse = (coarse_mask >> k) & 1u;
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
            c.coarse |= 1u << k;
        } else {
            if (ps == 0 && c.slabs[k] != 1) return bad("a broadcast scalar (pixel stride 0) is constant in time: its every must be at least days");
            if (ps == 1 && c.slabs[k] > 1 && ts < spec->n) return bad("time stride of an array with several slabs must be at least n");
            if (ps == 1) c.a.dense |= 1u << k;
        }
        c.a.arr[k] = ptr;
        c.a.tstride[k] = c.slabs[k] > 1 ? ts : 0;
        c.a.every[k] = evc;
    }
    return MOD16_OK;
}

// the class raster, the outputs, the periods, the size of a staged tile
template <typename T>
static void comp_fill(CompCall<T>& c, const mod16_composite_spec* spec, const uint8_t* cls, T* out_et, T* out_pet,
                      uint16_t* count_et, uint16_t* count_pet, int64_t out_pitch, int64_t stage_bytes) {
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
    c.stage_bytes = stage_budget((size_t)stage_bytes);
}

// The kernels of a family for arguments `a` (all pointers are device pointers here). K names them:
// K::template main<FAST, PET>() and K::template redo<PET>().
template <typename K, typename A>
static int comp_launch(mod16_ctx* ctx, const A& a, int64_t n, bool pet, unsigned flags, hipStream_t st) {
    if (n <= 0) return MOD16_OK;
    const int blocks = batch_blocks(ctx, n);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, st, a); };
    if (flags & MOD16_MATH_EXACT) {
        if (pet) go(K::template main<false, true>());
        else go(K::template main<false, false>());
    } else if (pet) {
        go(K::template main<true, true>());
        // pixels with a day outside the domain of the fast arithmetic: the kernel above left a mark
        // in period 0 of their out_et, this one computes all their periods
        go(K::template redo<true>());
    } else {
        go(K::template main<true, false>());
        go(K::template redo<false>());
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// the context's tables and status word in the arguments of a launch
template <typename T> static CompArgs<T> comp_with_tables(const mod16_ctx* ctx, CompArgs<T> a) {
    a.lut64 = ctx->lut64.as<double>();
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    return a;
}

// HOST mode: every time slab of the 15 arrays, the periods of the outputs and counts, the class
// raster -- through the shared staging path, the tile cut so that a slot's slab fits stage_bytes.
// resident[k]: the device copy of coarse array k, which its family has uploaded whole (plane: the
// elements between two of its planes there); launch(d, t): tile t's kernels on the arguments d,
// HostTile::off its first pixel in the call.
template <typename T, typename Launch>
static int comp_host(mod16_ctx* ctx, const CompCall<T>& h, const T* const* resident, int64_t plane, Launch&& launch) {
    const CompArgs<T>& a = h.a;
    const int P = h.periods;
    HostPlan p(sizeof(T));
    for (int k = 0; k < kCompArrays; ++k) {
        if ((h.coarse >> k) & 1u) {
            p.add(kResident, a.arr[k]);
            p.a[k].dev = const_cast<T*>(resident[k]);
        } else if ((a.dense >> k) & 1u) {
            p.add(kIn, a.arr[k], false, h.slabs[k], a.tstride[k]);
        } else {
            p.add(kScalar, a.arr[k]);
        }
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
    const int64_t tile = stage_tile(p, sizeof(T), h.stage_bytes);
    auto on_tile = [&](const HostTile& t) {
        CompArgs<T> d = a;
        d.n = t.m;
        const int64_t row = (int64_t)(t.row_bytes / sizeof(T));
        for (int k = 0; k < kCompArrays; ++k) {
            d.arr[k] = static_cast<const T*>(t.dev[k]);
            if ((h.coarse >> k) & 1u) d.tstride[k] = h.slabs[k] > 1 ? plane : 0;
            else d.tstride[k] = ((a.dense >> k) & 1u) ? row : 0;
        }
        d.out_et = static_cast<T*>(t.dev[kCompArrays]);
        d.out_pet = static_cast<T*>(t.dev[kCompArrays + 1]);
        d.cnt_et = static_cast<uint16_t*>(t.dev[kCompArrays + 2]);
        d.cnt_pet = static_cast<uint16_t*>(t.dev[kCompArrays + 3]);
        d.cls = static_cast<const uint8_t*>(t.dev[kCompArrays + 4]);
        d.out_pitch = row;
        d.cnt_pitch = (int64_t)(t.row_bytes / sizeof(uint16_t));
        return launch(d, t);
    };
    // (pipeline = false: these kernels use none of the stream pipeline's workspace; the status word --
    // a class code >= 13 -- is read back here)
    const int rc = host_tiled(ctx, p, a.n, ctx->host_threads, false, on_tile, nullptr, tile);
    return rc == MOD16_OK ? read_status(ctx, ctx->streams[0]) : rc;
}
