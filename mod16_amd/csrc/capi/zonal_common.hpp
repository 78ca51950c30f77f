// libmod16hip.so, host side -- what mod16_zonal_* (zonal.hip) and mod16_zonal_hist_* (zonalq.hip) share:
// their specs begin with the same geometry fields (n ... value_pitch) and their kernels walk the same
// ZonalGeom (mod16_zonal.hpp), so the rules about that geometry -- its checks, the extents of its
// inputs, the alignment that allows vector access, the (zone type, weight kind) instance, the HOST
// mode -- stand here once, as templates over the spec.
#pragma once
#include <type_traits>

#include "host.hpp"
#include "../mod16_zonal.hpp"

static size_t zonal_zone_size(int zone_type) { return zone_type == MOD16_ZONE_U8 ? 1 : zone_type == MOD16_ZONE_U16 ? 2 : 4; }

static bool zonal_aligned(const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

// first and last raster row of the call's pixels [first_pixel, first_pixel + n)
template <typename Spec>
static void zonal_rows(const Spec& s, int64_t* r0, int64_t* r1) {
    *r0 = s.first_pixel / s.cols;
    *r1 = (s.first_pixel + s.n - 1) / s.cols;
}

// ZonalGeom::wide of device pointers: every row of values, zone ids and per-pixel weights starts a 16-byte vector
template <typename T, typename Spec>
static bool zonal_wide(const ZonalGeom& g, const Spec& s) {
    constexpr size_t V = 16 / sizeof(T);
    return zonal_aligned(g.values, 16) && (s.layers == 1 || (size_t)g.pitch % V == 0) &&
           zonal_aligned(g.zones, V * zonal_zone_size(s.zone_type)) &&
           (s.weight_kind != MOD16_ZONAL_WEIGHT_PIXEL || zonal_aligned(g.weights, 16));
}

// calls f(ZT(), std::integral_constant<int, WK>()) with the kernels' template arguments for a spec's zone type and weight kind
template <typename F>
static void zonal_dispatch(int zone_type, int weight_kind, F&& f) {
    auto weights = [&](auto zt) {
        if (weight_kind == MOD16_ZONAL_WEIGHT_NONE) f(zt, std::integral_constant<int, kZonalWeightNone>());
        else if (weight_kind == MOD16_ZONAL_WEIGHT_ROW) f(zt, std::integral_constant<int, kZonalWeightRow>());
        else f(zt, std::integral_constant<int, kZonalWeightPixel>());
    };
    if (zone_type == MOD16_ZONE_U8) weights(uint8_t());
    else if (zone_type == MOD16_ZONE_U16) weights(uint16_t());
    else weights(int32_t());
}

// what every entry point checks of the geometry behind n and layers; -> NULL, or what is wrong
template <typename Spec>
static const char* zonal_check_geometry(const Spec* s) {
    if (s->weight_kind != MOD16_ZONAL_WEIGHT_NONE && s->weight_kind != MOD16_ZONAL_WEIGHT_ROW && s->weight_kind != MOD16_ZONAL_WEIGHT_PIXEL)
        return "weight_kind must be MOD16_ZONAL_WEIGHT_NONE, MOD16_ZONAL_WEIGHT_ROW or MOD16_ZONAL_WEIGHT_PIXEL";
    if (s->weight_kind == MOD16_ZONAL_WEIGHT_ROW && s->cols < 1) return "per-row weights need cols >= 1";
    if (s->weight_kind == MOD16_ZONAL_WEIGHT_ROW && (s->first_pixel < 0 || s->first_pixel > (int64_t(1) << 50)))
        return "first_pixel must be between 0 and 2^50";
    if (s->value_pitch < s->n) return "value_pitch must be at least n";
    return nullptr;
}
static const char* zonal_check_zone_type(int zone_type) {
    if (zone_type != MOD16_ZONE_U8 && zone_type != MOD16_ZONE_U16 && zone_type != MOD16_ZONE_I32)
        return "zone_type must be MOD16_ZONE_U8, MOD16_ZONE_U16 or MOD16_ZONE_I32";
    return nullptr;
}

// the extents of a call's inputs (n > 0), for the overlap check, into ins[]; -> how many (at most 3)
template <typename T, typename Spec>
static int zonal_input_extents(const Spec& s, const T* values, const void* zones, const void* weights, Extent* ins) {
    int ni = 0;
    ins[ni++] = extent(values, 1, 0, s.layers, s.value_pitch, s.n, sizeof(T));
    ins[ni++] = extent(zones, s.n, zonal_zone_size(s.zone_type));
    if (s.weight_kind == MOD16_ZONAL_WEIGHT_PIXEL) ins[ni++] = extent(weights, s.n, sizeof(T));
    if (s.weight_kind == MOD16_ZONAL_WEIGHT_ROW) {
        int64_t r0, r1;
        zonal_rows(s, &r0, &r1);
        ins[ni++] = extent(static_cast<const double*>(weights) + r0, r1 - r0 + 1, sizeof(double));
    }
    return ni;
}

// the geometry of a checked spec and its arrays (a zeroed g: row0 = 0, wide = 0)
template <typename Spec>
static void zonal_fill_geometry(ZonalGeom& g, const Spec& s, const void* values, const void* zones, const void* weights) {
    g.values = values;
    g.zones = zones;
    g.weights = weights;
    g.n = s.n;
    g.pitch = s.value_pitch;
    g.cols = s.weight_kind == MOD16_ZONAL_WEIGHT_ROW ? s.cols : 1;
    g.inv_cols = 1.0 / (double)g.cols;
    g.first_pixel = s.weight_kind == MOD16_ZONAL_WEIGHT_ROW ? s.first_pixel : 0;
    g.nzones = s.nzones;
}

// HOST mode of both families: values (one row per layer), zone ids and per-pixel weights staged tile by
// tile through the shared staging path; the table (`bytes` at `table`: the accumulator, a histogram)
// uploaded once, added into by the tiles of every slot's stream (integer atomics: the order does not
// show) and downloaded once; the per-row weights the range touches uploaded once. tile(g, dtable, st)
// enqueues one tile: g is the tile's geometry in device pointers, dtable the table's device copy.
// no_table, no_rows: what to say where the device memory for the table or the per-row weights cannot be had.
template <typename T, typename Spec, typename Tile>
static int zonal_host_tiled(mod16_ctx* ctx, const Spec& s, ZonalGeom g, void* table, size_t bytes, const char* no_table,
                            const char* no_rows, int64_t stage_bytes, Tile&& tile) {
    DevMem dtable, drow;
    int rc = dtable.alloc(ctx, bytes, no_table);
    if (rc != MOD16_OK) return rc;
    if (s.weight_kind == MOD16_ZONAL_WEIGHT_ROW) {
        int64_t r0, r1;
        zonal_rows(s, &r0, &r1);
        const size_t row_bytes = sizeof(double) * (size_t)(r1 - r0 + 1);
        rc = drow.alloc(ctx, row_bytes, no_rows);
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(drow.get(), static_cast<const double*>(g.weights) + r0, row_bytes, hipMemcpyHostToDevice));
        g.row0 = r0;
    }
    HIPCHK(ctx, hipMemcpy(dtable.get(), table, bytes, hipMemcpyHostToDevice));
    const size_t zsz = zonal_zone_size(s.zone_type);
    const bool pixel_w = s.weight_kind == MOD16_ZONAL_WEIGHT_PIXEL;
    HostPlan p((int)sizeof(T));
    p.add(kIn, g.values, false, s.layers, s.value_pitch);                       // 0
    p.add(kIn, pixel_w ? g.weights : nullptr, false);                            // 1
    if (zsz == 1) p.add(kIn, g.zones, true);                                     // 2: a byte row
    else p.add(kIn, g.zones, false, 1, 0, (int)zsz);                             // 2: in a T-sized place
    auto launch = [&](const HostTile& t) {
        ZonalGeom d = g;
        d.n = t.m;
        d.values = t.dev[0];
        d.pitch = (int64_t)(t.row_bytes / sizeof(T));
        d.zones = t.dev[2];
        d.weights = pixel_w ? t.dev[1] : drow.get();
        d.first_pixel = g.first_pixel + t.off;
        return tile(d, dtable.get(), t.st);
    };
    rc = host_tiled(ctx, p, s.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(T), stage_bytes));
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipMemcpy(table, dtable.get(), bytes, hipMemcpyDeviceToHost));
    return MOD16_OK;
}
