// libmod16hip.so -- zonal statistics: mod16_zonal_f64 / _f32 (exact weighted sums per zone and layer into a (K, Z, 10) int64 accumulator, order-independent by construction), mod16_zonal_bounds_f64 / _f32 (the bounds pre-pass), mod16_zonal_lds_zones
#include "zonal_common.hpp"

// All pointers are device pointers here; a.n > 0.
template <typename T>
static int launch_zonal(mod16_ctx* ctx, ZonalArgs a, const mod16_zonal_spec& s, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    a.wide = zonal_wide<T>(a, s);
    const int64_t blocks = ((a.n + V - 1) / V + kBlock - 1) / kBlock;
    auto grid = [&](int per_cu) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)ctx->cus * per_cu)), (unsigned)s.layers); };
    zonal_dispatch(s.zone_type, s.weight_kind, [&](auto zt, auto wk) {
        using ZT = decltype(zt);
        constexpr int WK = decltype(wk)::value;
        if (a.nzones <= kZonalLdsSmall)
            hipLaunchKernelGGL((zonal_kernel<T, ZT, WK, kZonalLdsSmall>), grid(4), dim3(kBlock), 0, st, a);
        else if (a.nzones <= kZonalLdsZones)
            hipLaunchKernelGGL((zonal_kernel<T, ZT, WK, kZonalLdsZones>), grid(2), dim3(kBlock), 0, st, a);
        else
            hipLaunchKernelGGL((zonal_kernel<T, ZT, WK, 0>), grid(4), dim3(kBlock), 0, st, a);
    });
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

template <typename T>
static int launch_zonal_bounds(mod16_ctx* ctx, const ZonalArgs& a, int wk, int layers, hipStream_t st) {
    const int64_t most = std::max(a.n, wk == MOD16_ZONAL_WEIGHT_ROW ? a.rows : (int64_t)0);
    const dim3 grid((unsigned)batch_blocks(ctx, most), (unsigned)layers);
    if (wk == MOD16_ZONAL_WEIGHT_NONE) hipLaunchKernelGGL((zonal_bounds_kernel<T, kZonalWeightNone>), grid, dim3(kBlock), 0, st, a);
    else if (wk == MOD16_ZONAL_WEIGHT_ROW) hipLaunchKernelGGL((zonal_bounds_kernel<T, kZonalWeightRow>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((zonal_bounds_kernel<T, kZonalWeightPixel>), grid, dim3(kBlock), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// what both entry points check of a spec; -> NULL, or what is wrong
static const char* zonal_check_spec(const mod16_zonal_spec* s, bool bounds_only) {
    if (s->n < 0 || s->n > (int64_t(1) << 30)) return "n must be between 0 and 2^30";
    if (s->layers < 1 || s->layers > 65535) return "layers must be between 1 and 65535";
    if (const char* what = zonal_check_geometry(s)) return what;
    if (bounds_only) return nullptr;
    if (s->nzones < 1 || s->nzones > (1 << 24)) return "nzones must be between 1 and 2^24";
    if (const char* what = zonal_check_zone_type(s->zone_type)) return what;
    // (in 64 bits: the exponents are the caller's)
    const int64_t f0 = 62 - (int64_t)s->ew, f1 = f0 - s->ex, f2 = f1 - s->ex;
    if (std::max({f0, f1, f2}) > 900 || std::min({f0, f1, f2}) < -900)
        return "the exponents ew and ex put a fixed-point scale outside 2^-900 ... 2^900";
    if (!(s->wmax > 0.0) || !(s->xmax > 0.0) || !(s->wmax <= std::ldexp(1.0, s->ew)) || !(s->xmax <= std::ldexp(1.0, s->ex)))
        return "the bounds must satisfy 0 < wmax <= 2^ew and 0 < xmax <= 2^ex";
    return nullptr;
}

template <typename T>
static int zonal_entry(mod16_ctx* ctx, const mod16_zonal_spec* spec, const T* values, const void* zones,
                       const void* weights, int64_t* acc, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_zonal: ", what); };
    if (!spec || !values || !zones || !acc) return bad("NULL spec, values, zones or acc");
    if (const char* what = zonal_check_spec(spec, false)) return bad(what);
    if (spec->weight_kind != MOD16_ZONAL_WEIGHT_NONE && !weights) return bad("NULL weights");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    if (spec->n == 0) return MOD16_OK;
    const int64_t words = (int64_t)kZonalWords * spec->layers * spec->nzones;
    {
        const Extent out = extent(acc, words, sizeof(int64_t));
        Extent ins[3];
        if (overlaps(&out, 1, ins, zonal_input_extents(*spec, values, zones, weights, ins))) return bad("acc overlaps an input");
    }
    ZonalArgs a;
    memset(&a, 0, sizeof a);
    zonal_fill_geometry(a, *spec, values, zones, weights);
    a.acc = reinterpret_cast<long long*>(acc);
    a.wmax = spec->wmax;
    a.xmax = spec->xmax;
    a.f[0] = 62 - spec->ew;
    a.f[1] = a.f[0] - spec->ex;
    a.f[2] = a.f[1] - spec->ex;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_zonal<T>(ctx, a, *spec, static_cast<hipStream_t>(stream));
    return zonal_host_tiled<T>(ctx, *spec, a, acc, sizeof(int64_t) * (size_t)words, "mod16_zonal: device memory for the accumulator",
                               "mod16_zonal: device memory for the per-row weights", stage_budget(stage_bytes),
                               [&](const ZonalGeom& g, void* dacc, hipStream_t st) {
                                   ZonalArgs d = a;
                                   static_cast<ZonalGeom&>(d) = g;
                                   d.acc = static_cast<long long*>(dacc);
                                   return launch_zonal<T>(ctx, d, *spec, st);
                               });
}

template <typename T>
static int zonal_bounds_entry(mod16_ctx* ctx, const mod16_zonal_spec* spec, const T* values, const void* weights,
                              double* wmax, double* xmax, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_zonal_bounds: ", what); };
    if (!spec || !values || !wmax || !xmax) return bad("NULL spec, values, wmax or xmax");
    if (const char* what = zonal_check_spec(spec, true)) return bad(what);
    const int wk = spec->weight_kind;
    if (wk != MOD16_ZONAL_WEIGHT_NONE && !weights) return bad("NULL weights");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    *wmax = wk == MOD16_ZONAL_WEIGHT_NONE ? 1.0 : 0.0;
    *xmax = 0.0;
    if (spec->n == 0) return MOD16_OK;
    ZonalArgs a;
    memset(&a, 0, sizeof a);
    a.values = values;
    a.weights = weights;
    a.n = spec->n;
    a.pitch = spec->value_pitch;
    int64_t r0 = 0, r1 = 0;
    if (wk == MOD16_ZONAL_WEIGHT_ROW) zonal_rows(*spec, &r0, &r1);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevMem top;
    int rc = top.alloc(ctx, 2 * sizeof(unsigned long long), "mod16_zonal_bounds: device memory for the two maxima");
    if (rc != MOD16_OK) return rc;
    a.bounds = top.as<unsigned long long>();
    unsigned long long bits[2] = {0, 0};
    double host_w = 0.0;
    if (where == MOD16_DEVICE) {
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (wk == MOD16_ZONAL_WEIGHT_ROW) {
            a.weights = static_cast<const double*>(weights) + r0;
            a.rows = r1 - r0 + 1;
        }
        HIPCHK(ctx, hipMemsetAsync(top.get(), 0, sizeof bits, st));
        rc = launch_zonal_bounds<T>(ctx, a, wk, spec->layers, st);
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpyAsync(bits, top.get(), sizeof bits, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    } else {
        // the per-row weights are a host vector: their maximum is taken here
        if (wk == MOD16_ZONAL_WEIGHT_ROW)
            for (int64_t r = r0; r <= r1; ++r) {
                const double w = static_cast<const double*>(weights)[r];
                if (w >= 0.0 && std::isfinite(w) && w > host_w) host_w = w;
            }
        HIPCHK(ctx, hipMemset(top.get(), 0, sizeof bits));
        HostPlan p((int)sizeof(T));
        p.add(kIn, values, false, spec->layers, spec->value_pitch);
        p.add(kIn, wk == MOD16_ZONAL_WEIGHT_PIXEL ? weights : nullptr, false);
        const int tile_wk = wk == MOD16_ZONAL_WEIGHT_PIXEL ? wk : MOD16_ZONAL_WEIGHT_NONE;
        auto launch = [&](const HostTile& t) {
            ZonalArgs d = a;
            d.n = t.m;
            d.values = t.dev[0];
            d.pitch = (int64_t)(t.row_bytes / sizeof(T));
            d.weights = t.dev[1];
            return launch_zonal_bounds<T>(ctx, d, tile_wk, spec->layers, t.st);
        };
        rc = host_tiled(ctx, p, spec->n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(T), stage_budget(stage_bytes)));
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(bits, top.get(), sizeof bits, hipMemcpyDeviceToHost));
    }
    double dev_w, dev_x;
    memcpy(&dev_w, &bits[0], sizeof dev_w);
    memcpy(&dev_x, &bits[1], sizeof dev_x);
    if (wk != MOD16_ZONAL_WEIGHT_NONE) *wmax = std::max(dev_w, host_w);
    *xmax = dev_x;
    return MOD16_OK;
}

extern "C" int mod16_zonal_f64(mod16_ctx* ctx, const mod16_zonal_spec* spec, const double* values, const void* zones,
                               const void* weights, int64_t* acc, int where, void* stream, size_t stage_bytes) {
    return zonal_entry<double>(ctx, spec, values, zones, weights, acc, where, stream, stage_bytes);
}
extern "C" int mod16_zonal_f32(mod16_ctx* ctx, const mod16_zonal_spec* spec, const float* values, const void* zones,
                               const void* weights, int64_t* acc, int where, void* stream, size_t stage_bytes) {
    return zonal_entry<float>(ctx, spec, values, zones, weights, acc, where, stream, stage_bytes);
}
extern "C" int mod16_zonal_bounds_f64(mod16_ctx* ctx, const mod16_zonal_spec* spec, const double* values, const void* weights,
                                      double* wmax, double* xmax, int where, void* stream, size_t stage_bytes) {
    return zonal_bounds_entry<double>(ctx, spec, values, weights, wmax, xmax, where, stream, stage_bytes);
}
extern "C" int mod16_zonal_bounds_f32(mod16_ctx* ctx, const mod16_zonal_spec* spec, const float* values, const void* weights,
                                      double* wmax, double* xmax, int where, void* stream, size_t stage_bytes) {
    return zonal_bounds_entry<float>(ctx, spec, values, weights, wmax, xmax, where, stream, stage_bytes);
}
extern "C" int mod16_zonal_lds_zones(void) { return kZonalLdsZones; }
