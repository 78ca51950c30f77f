// libmod16hip.so -- zonal statistics: mod16_zonal_f64 / _f32 (exact weighted sums per zone and layer into a (K, Z, 10) int64 accumulator, order-independent by construction), mod16_zonal_bounds_f64 / _f32 (the bounds pre-pass), mod16_zonal_lds_zones
#include "host.hpp"
#include "../mod16_zonal.hpp"

namespace {
size_t zonal_zone_size(int zone_type) { return zone_type == MOD16_ZONE_U8 ? 1 : zone_type == MOD16_ZONE_U16 ? 2 : 4; }

bool zonal_aligned(const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

// first and last raster row of the pixels [first_pixel, first_pixel + n)
void zonal_rows(const mod16_zonal_spec& s, int64_t first, int64_t n, int64_t* r0, int64_t* r1) {
    *r0 = first / s.cols;
    *r1 = (first + n - 1) / s.cols;
}
}  // namespace

template <typename T, typename ZT, int WK>
static void zonal_launch_lz(const ZonalArgs& a, int cus, int layers, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t blocks = ((a.n + V - 1) / V + kBlock - 1) / kBlock;
    auto grid = [&](int per_cu) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)cus * per_cu)), (unsigned)layers); };
    if (a.nzones <= kZonalLdsSmall)
        hipLaunchKernelGGL((zonal_kernel<T, ZT, WK, kZonalLdsSmall>), grid(4), dim3(kBlock), 0, st, a);
    else if (a.nzones <= kZonalLdsZones)
        hipLaunchKernelGGL((zonal_kernel<T, ZT, WK, kZonalLdsZones>), grid(2), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((zonal_kernel<T, ZT, WK, 0>), grid(4), dim3(kBlock), 0, st, a);
}
template <typename T, typename ZT>
static void zonal_launch_wk(const ZonalArgs& a, int wk, int cus, int layers, hipStream_t st) {
    if (wk == MOD16_ZONAL_WEIGHT_NONE) zonal_launch_lz<T, ZT, kZonalWeightNone>(a, cus, layers, st);
    else if (wk == MOD16_ZONAL_WEIGHT_ROW) zonal_launch_lz<T, ZT, kZonalWeightRow>(a, cus, layers, st);
    else zonal_launch_lz<T, ZT, kZonalWeightPixel>(a, cus, layers, st);
}

// All pointers are device pointers here; a.n > 0.
template <typename T>
static int launch_zonal(mod16_ctx* ctx, ZonalArgs a, const mod16_zonal_spec& s, hipStream_t st) {
    constexpr size_t V = 16 / sizeof(T);
    a.wide = zonal_aligned(a.values, 16) && (s.layers == 1 || (size_t)a.pitch % V == 0) &&
             zonal_aligned(a.zones, V * zonal_zone_size(s.zone_type)) &&
             (s.weight_kind != MOD16_ZONAL_WEIGHT_PIXEL || zonal_aligned(a.weights, 16));
    if (s.zone_type == MOD16_ZONE_U8) zonal_launch_wk<T, uint8_t>(a, s.weight_kind, ctx->cus, s.layers, st);
    else if (s.zone_type == MOD16_ZONE_U16) zonal_launch_wk<T, uint16_t>(a, s.weight_kind, ctx->cus, s.layers, st);
    else zonal_launch_wk<T, int32_t>(a, s.weight_kind, ctx->cus, s.layers, st);
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

// HOST mode: values (one row per layer), zone ids and per-pixel weights staged tile by tile through
// the shared staging path; the accumulator uploaded once, added into by the tiles of every slot's
// stream (integer atomics: the order does not show) and downloaded once; the per-row weights the
// range touches uploaded once.
template <typename T>
static int zonal_host(mod16_ctx* ctx, const mod16_zonal_spec& s, ZonalArgs a, int64_t* acc, int64_t stage_bytes) {
    const size_t zsz = zonal_zone_size(s.zone_type);
    const size_t acc_bytes = sizeof(int64_t) * kZonalWords * (size_t)s.layers * (size_t)s.nzones;
    DevMem dacc, drow;
    int rc = dacc.alloc(ctx, acc_bytes, "mod16_zonal: device memory for the accumulator");
    if (rc != MOD16_OK) return rc;
    const double* host_row = static_cast<const double*>(a.weights);
    if (s.weight_kind == MOD16_ZONAL_WEIGHT_ROW) {
        int64_t r0, r1;
        zonal_rows(s, s.first_pixel, s.n, &r0, &r1);
        rc = drow.alloc(ctx, sizeof(double) * (size_t)(r1 - r0 + 1), "mod16_zonal: device memory for the per-row weights");
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(drow.get(), host_row + r0, sizeof(double) * (size_t)(r1 - r0 + 1), hipMemcpyHostToDevice));
        a.row0 = r0;
    }
    HIPCHK(ctx, hipMemcpy(dacc.get(), acc, acc_bytes, hipMemcpyHostToDevice));
    HostPlan p((int)sizeof(T));
    const bool pixel_w = s.weight_kind == MOD16_ZONAL_WEIGHT_PIXEL;
    p.add(kIn, a.values, false, s.layers, s.value_pitch);                       // 0
    p.add(kIn, pixel_w ? a.weights : nullptr, false);                            // 1
    if (zsz == 1) p.add(kIn, a.zones, true);                                     // 2: a byte row
    else p.add(kIn, a.zones, false, 1, 0, (int)zsz);                             // 2: in a T-sized place
    auto launch = [&](const HostTile& t) {
        ZonalArgs d = a;
        d.n = t.m;
        d.values = t.dev[0];
        d.pitch = (int64_t)(t.row_bytes / sizeof(T));
        d.zones = t.dev[2];
        d.weights = pixel_w ? t.dev[1] : drow.get();
        d.first_pixel = s.first_pixel + t.off;
        d.acc = dacc.as<long long>();
        return launch_zonal<T>(ctx, d, s, t.st);
    };
    rc = host_tiled(ctx, p, s.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(T), stage_bytes));
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipMemcpy(acc, dacc.get(), acc_bytes, hipMemcpyDeviceToHost));
    return MOD16_OK;
}

// what both entry points check of a spec; -> NULL, or what is wrong
static const char* zonal_check_spec(const mod16_zonal_spec* s, bool bounds_only) {
    if (s->n < 0 || s->n > (int64_t(1) << 30)) return "n must be between 0 and 2^30";
    if (s->layers < 1 || s->layers > 65535) return "layers must be between 1 and 65535";
    if (s->weight_kind != MOD16_ZONAL_WEIGHT_NONE && s->weight_kind != MOD16_ZONAL_WEIGHT_ROW && s->weight_kind != MOD16_ZONAL_WEIGHT_PIXEL)
        return "weight_kind must be MOD16_ZONAL_WEIGHT_NONE, MOD16_ZONAL_WEIGHT_ROW or MOD16_ZONAL_WEIGHT_PIXEL";
    if (s->weight_kind == MOD16_ZONAL_WEIGHT_ROW && s->cols < 1) return "per-row weights need cols >= 1";
    if (s->weight_kind == MOD16_ZONAL_WEIGHT_ROW && (s->first_pixel < 0 || s->first_pixel > (int64_t(1) << 50)))
        return "first_pixel must be between 0 and 2^50";
    if (s->value_pitch < s->n) return "value_pitch must be at least n";
    if (bounds_only) return nullptr;
    if (s->nzones < 1 || s->nzones > (1 << 24)) return "nzones must be between 1 and 2^24";
    if (s->zone_type != MOD16_ZONE_U8 && s->zone_type != MOD16_ZONE_U16 && s->zone_type != MOD16_ZONE_I32)
        return "zone_type must be MOD16_ZONE_U8, MOD16_ZONE_U16 or MOD16_ZONE_I32";
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
    const int64_t n = spec->n;
    if (n == 0) return MOD16_OK;
    {
        const Extent out = extent(acc, (int64_t)kZonalWords * spec->layers * spec->nzones, sizeof(int64_t));
        Extent ins[3];
        int ni = 0;
        ins[ni++] = extent(values, 1, 0, spec->layers, spec->value_pitch, n, sizeof(T));
        ins[ni++] = extent(zones, n, zonal_zone_size(spec->zone_type));
        if (spec->weight_kind == MOD16_ZONAL_WEIGHT_PIXEL) ins[ni++] = extent(weights, n, sizeof(T));
        if (spec->weight_kind == MOD16_ZONAL_WEIGHT_ROW) {
            int64_t r0, r1;
            zonal_rows(*spec, spec->first_pixel, n, &r0, &r1);
            ins[ni++] = extent(static_cast<const double*>(weights) + r0, r1 - r0 + 1, sizeof(double));
        }
        if (overlaps(&out, 1, ins, ni)) return bad("acc overlaps an input");
    }
    ZonalArgs a;
    memset(&a, 0, sizeof a);
    a.values = values;
    a.zones = zones;
    a.weights = weights;
    a.acc = reinterpret_cast<long long*>(acc);
    a.n = n;
    a.pitch = spec->value_pitch;
    a.cols = spec->weight_kind == MOD16_ZONAL_WEIGHT_ROW ? spec->cols : 1;
    a.inv_cols = 1.0 / (double)a.cols;
    a.first_pixel = spec->weight_kind == MOD16_ZONAL_WEIGHT_ROW ? spec->first_pixel : 0;
    a.wmax = spec->wmax;
    a.xmax = spec->xmax;
    a.nzones = spec->nzones;
    a.f[0] = 62 - spec->ew;
    a.f[1] = a.f[0] - spec->ex;
    a.f[2] = a.f[1] - spec->ex;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_zonal<T>(ctx, a, *spec, static_cast<hipStream_t>(stream));
    return zonal_host<T>(ctx, *spec, a, acc, stage_budget(stage_bytes));
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
    if (wk == MOD16_ZONAL_WEIGHT_ROW) zonal_rows(*spec, spec->first_pixel, spec->n, &r0, &r1);
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
