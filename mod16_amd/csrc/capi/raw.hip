// libmod16hip.so -- raw reanalysis drivers (N1): mod16_et_raw_*
#include "host.hpp"
#include "../mod16_methods.hpp"

// ----------------------------------------------------- raw drivers (N1)
template <typename T>
static int raw_entry(mod16_ctx* ctx, const uint8_t* cls, const T* const* raw,
                     const int64_t* rstride, const uint8_t* fpar_pct, const uint8_t* lai_x10,
                     const T* day_hours, int64_t hstride, int64_t n, T* out_day, T* out_night,
                     T* out_total8, unsigned flags, int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    if (!cls || !raw || !rstride || !fpar_pct || !lai_x10 || n < 0)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_raw: NULL argument or n < 0");
    if (!out_day && !out_night && !out_total8) return fail(ctx, MOD16_ERR_ARG, "mod16_et_raw: no output array given");
    if (out_total8 && !day_hours) return fail(ctx, MOD16_ERR_ARG, "mod16_et_raw: out_total8 needs day_hours");
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, "mod16_et_raw: mod16_set_bplut_f64 was not called");
    RawArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) {
        if (!raw[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_raw: NULL driver array");
        a.drv[k] = raw[k];
        if (rstride[k]) a.dense_drv |= 1u << k;
    }
    a.fpar_pct = fpar_pct;
    a.lai_x10 = lai_x10;
    a.cls = cls;
    a.day_hours = out_total8 ? day_hours : nullptr;
    a.dense_hours = hstride ? 1u : 0u;
    a.out[0] = out_day;
    a.out[1] = out_night;
    a.out[2] = out_total8;
    a.n = n;
    a.lut = ctx_lut<T>(ctx);
    a.lut64 = ctx->lut64.as<double>();
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    if (n == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool fast = (flags & MOD16_MATH_EXACT) == 0;
    // d holds device pointers. Dense, 16-byte-aligned rasters run their vector
    // body on the production pipeline (et_stream_kernel); the ragged tail and
    // every other shape run the plain kernel. host_hours: the scalar hours of
    // daylight when it is known on the host (HOST mode).
    auto launch = [&](const RawArgs<T>& d, hipStream_t st, const T* host_hours) -> int {
        constexpr int V = VecOf<T>::v;
        auto al = [](const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; };
        bool ok = fast && ctx->use_dma && d.dense_drv == 0x3fffu && d.out[0] && d.out[1];
        for (int k = 0; k < 14 && ok; ++k) ok = al(d.drv[k], 16);
        ok = ok && al(d.fpar_pct, V) && al(d.lai_x10, V) && al(d.cls, V) && al(d.out[0], 16) && al(d.out[1], 16);
        int mode = kStreamRaw;
        if (ok && d.out[2]) {
            ok = al(d.out[2], 16);
            if (d.dense_hours) { mode = kStreamRawTotalHours; ok = ok && al(d.day_hours, 16); }
            else if (host_hours) mode = kStreamRawTotal;
            else ok = false;
        }
        const int64_t nbody = ok ? (d.n / V) * V : 0;
        if (nbody) {
            StreamArgs<T> s;
            memset(&s, 0, sizeof s);
            for (int k = 0; k < 14; ++k) s.wide[k] = d.drv[k];
            s.wide[14] = d.day_hours;
            s.bytes[0] = d.cls; s.bytes[1] = d.fpar_pct; s.bytes[2] = d.lai_x10;
            for (int k = 0; k < 3; ++k) s.out[k] = d.out[k];
            s.hours = host_hours ? (double)*host_hours : 0.0;
            s.n = nbody;
            int rc = MOD16_OK;
            bool mixed = false;
            if constexpr (std::is_same<T, float>::value) {
                mixed = (flags & MOD16_MATH_MIXED) != 0;
                if (mixed)
                    rc = mode == kStreamRaw ? launch_stream<T, kStreamRawMixed>(ctx, s, st)
                         : mode == kStreamRawTotal ? launch_stream<T, kStreamRawTotalMixed>(ctx, s, st)
                                                   : launch_stream<T, kStreamRawTotalHoursMixed>(ctx, s, st);
            }
            if (!mixed)
                rc = mode == kStreamRaw ? launch_stream<T, kStreamRaw>(ctx, s, st)
                     : mode == kStreamRawTotal ? launch_stream<T, kStreamRawTotal>(ctx, s, st)
                                               : launch_stream<T, kStreamRawTotalHours>(ctx, s, st);
            if (rc != MOD16_OK) return rc;
        }
        if (nbody < d.n) {
            RawArgs<T> t = d;
            for (int k = 0; k < 14; ++k) if ((t.dense_drv >> k) & 1u) t.drv[k] += nbody;
            t.fpar_pct += nbody; t.lai_x10 += nbody; t.cls += nbody;
            if (t.day_hours && t.dense_hours) t.day_hours += nbody;
            for (int k = 0; k < 3; ++k) if (t.out[k]) t.out[k] += nbody;
            t.n = d.n - nbody;
            const int grid = grid_for(ctx, t.n);
            if (fast) hipLaunchKernelGGL((et_raw_kernel<T, true>), dim3(grid), dim3(kBlock), 0, st, t);
            else hipLaunchKernelGGL((et_raw_kernel<T, false>), dim3(grid), dim3(kBlock), 0, st, t);
        }
        return MOD16_OK;
    };
    if (where == MOD16_DEVICE) {
        int rc = launch(a, static_cast<hipStream_t>(stream), nullptr);
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipGetLastError());
        return MOD16_OK;
    }
    if (where != MOD16_HOST) return fail(ctx, MOD16_ERR_ARG, "mod16_et_raw: bad `where`");
    // HOST mode: 14 drivers, day_hours, 3 outputs (T each), then the fPAR, LAI and class bytes
    HostPlan p(sizeof(T));
    for (int k = 0; k < 14; ++k) p.add(((a.dense_drv >> k) & 1u) ? kIn : kScalar, a.drv[k]);
    p.add(a.dense_hours ? kIn : kScalar, a.day_hours);
    for (int k = 0; k < 3; ++k) p.add(kOut, a.out[k]);
    p.add(kIn, fpar_pct, true);
    p.add(kIn, lai_x10, true);
    p.add(kIn, cls, true);
    p.cls = cls;
    const T* host_hours = (a.day_hours && !a.dense_hours) ? a.day_hours : nullptr;
    auto launch_tile = [&](const HostTile& t) {
        RawArgs<T> d = a;
        d.n = t.m;
        for (int k = 0; k < 14; ++k) d.drv[k] = static_cast<const T*>(t.dev[k]);
        d.day_hours = static_cast<const T*>(t.dev[14]);
        for (int k = 0; k < 3; ++k) d.out[k] = static_cast<T*>(t.dev[15 + k]);
        d.fpar_pct = static_cast<const uint8_t*>(t.dev[18]);
        d.lai_x10 = static_cast<const uint8_t*>(t.dev[19]);
        d.cls = static_cast<const uint8_t*>(t.dev[20]);
        return launch(d, t.st, host_hours);
    };
    if (n <= ctx->small_pixels) {
        const int rc = host_small(ctx, p, n, true, launch_tile);
        if (rc != kSmallUnavailable) return rc;
    }
    return host_tiled(ctx, p, n, ctx->host_threads, true, launch_tile);
}

extern "C" int mod16_et_raw_f64(mod16_ctx* ctx, const uint8_t* cls, const double* const* raw,
                                const int64_t* rstride, const uint8_t* fpar_pct,
                                const uint8_t* lai_x10, const double* day_hours, int64_t hstride,
                                int64_t n, double* out_day, double* out_night, double* out_total8,
                                unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return raw_entry<double>(ctx, cls, raw, rstride, fpar_pct, lai_x10, day_hours, hstride, n,
                             out_day, out_night, out_total8, flags, where, stream);
}
extern "C" int mod16_et_raw_f32(mod16_ctx* ctx, const uint8_t* cls, const float* const* raw,
                                const int64_t* rstride, const uint8_t* fpar_pct,
                                const uint8_t* lai_x10, const float* day_hours, int64_t hstride,
                                int64_t n, float* out_day, float* out_night, float* out_total8,
                                unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return raw_entry<float>(ctx, cls, raw, rstride, fpar_pct, lai_x10, day_hours, hstride, n,
                            out_day, out_night, out_total8, flags, where, stream);
}
