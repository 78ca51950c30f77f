// libmod16hip.so -- zonal histograms and exact zonal quantiles: mod16_zonal_hist_f64 / _f32 (the uniform histogram, or one level's digit histogram under the prefix filter, ADDED into an int64 table), mod16_zonal_select (closes a level: target, prefix scan, the next prefix, the value at the end), mod16_zonal_hist_lds_bytes
#include "host.hpp"
#include "../mod16_zonalq.hpp"

namespace {
size_t zonalq_zone_size(int zone_type) { return zone_type == MOD16_ZONE_U8 ? 1 : zone_type == MOD16_ZONE_U16 ? 2 : 4; }
bool zonalq_aligned(const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }
void zonalq_rows(const mod16_zonal_hist_spec& s, int64_t* r0, int64_t* r1) {
    *r0 = s.first_pixel / s.cols;
    *r1 = (s.first_pixel + s.n - 1) / s.cols;
}
int zonalq_levels(const mod16_zonal_hist_spec& s) { return (s.width + s.bits - 1) / s.bits; }
// words per zone and slot, slots of the table in memory, words of the whole table
int64_t zonalq_nb(const mod16_zonal_hist_spec& s) { return s.mode == MOD16_ZONAL_HIST_UNIFORM ? (int64_t)s.bins + 2 : (int64_t)1 << s.bits; }
int64_t zonalq_slots(const mod16_zonal_hist_spec& s) { return s.mode == MOD16_ZONAL_HIST_UNIFORM ? 1 : s.slots; }
int64_t zonalq_words(const mod16_zonal_hist_spec& s) { return (int64_t)s.layers * s.nzones * zonalq_slots(s) * zonalq_nb(s); }
}  // namespace

template <typename T, typename ZT, int WK, int MODE>
static void zonalq_launch_lw(const ZonalHistArgs& a, int cus, int layers, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t blocks = ((a.n + V - 1) / V + kBlock - 1) / kBlock;
    // a block flushes its whole table: with many layers each takes fewer, longer blocks
    auto grid = [&](int per_cu) {
        const int64_t want = ((int64_t)cus * per_cu * 2 + layers - 1) / layers;
        return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, want)), (unsigned)layers);
    };
    const int64_t words = (int64_t)a.nzones * a.seff * a.nb;
    if (words <= kZonalqLdsSmall)
        hipLaunchKernelGGL((zonal_hist_kernel<T, ZT, WK, MODE, kZonalqLdsSmall>), grid(5), dim3(kBlock), 0, st, a);
    else if (words <= kZonalqLdsWords)
        hipLaunchKernelGGL((zonal_hist_kernel<T, ZT, WK, MODE, kZonalqLdsWords>), grid(2), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((zonal_hist_kernel<T, ZT, WK, MODE, 0>), grid(4), dim3(kBlock), 0, st, a);
}
template <typename T, typename ZT, int WK>
static void zonalq_launch_mode(const ZonalHistArgs& a, int mode, int cus, int layers, hipStream_t st) {
    if (mode == MOD16_ZONAL_HIST_UNIFORM) zonalq_launch_lw<T, ZT, WK, kZonalqUniform>(a, cus, layers, st);
    else zonalq_launch_lw<T, ZT, WK, kZonalqDigit>(a, cus, layers, st);
}
template <typename T, typename ZT>
static void zonalq_launch_wk(const ZonalHistArgs& a, int wk, int mode, int cus, int layers, hipStream_t st) {
    if (wk == MOD16_ZONAL_WEIGHT_NONE) zonalq_launch_mode<T, ZT, kZonalWeightNone>(a, mode, cus, layers, st);
    else if (wk == MOD16_ZONAL_WEIGHT_ROW) zonalq_launch_mode<T, ZT, kZonalWeightRow>(a, mode, cus, layers, st);
    else zonalq_launch_mode<T, ZT, kZonalWeightPixel>(a, mode, cus, layers, st);
}

// All pointers are device pointers here; a.n > 0.
template <typename T>
static int launch_zonal_hist(mod16_ctx* ctx, ZonalHistArgs a, const mod16_zonal_hist_spec& s, hipStream_t st) {
    constexpr size_t V = 16 / sizeof(T);
    a.wide = zonalq_aligned(a.values, 16) && (s.layers == 1 || (size_t)a.pitch % V == 0) &&
             zonalq_aligned(a.zones, V * zonalq_zone_size(s.zone_type)) &&
             (s.weight_kind != MOD16_ZONAL_WEIGHT_PIXEL || zonalq_aligned(a.weights, 16));
    if (s.zone_type == MOD16_ZONE_U8) zonalq_launch_wk<T, uint8_t>(a, s.weight_kind, s.mode, ctx->cus, s.layers, st);
    else if (s.zone_type == MOD16_ZONE_U16) zonalq_launch_wk<T, uint16_t>(a, s.weight_kind, s.mode, ctx->cus, s.layers, st);
    else zonalq_launch_wk<T, int32_t>(a, s.weight_kind, s.mode, ctx->cus, s.layers, st);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: as zonal_host -- values, zone ids and per-pixel weights staged tile by tile; the table
// uploaded once, added into by the tiles of every slot's stream (integer atomics: the order does not
// show) and downloaded once; the prefixes and the per-row weights the range touches uploaded once.
template <typename T>
static int zonal_hist_host(mod16_ctx* ctx, const mod16_zonal_hist_spec& s, ZonalHistArgs a, const uint64_t* prefix,
                           int64_t* hist, int64_t stage_bytes) {
    const size_t zsz = zonalq_zone_size(s.zone_type);
    const size_t hist_bytes = sizeof(int64_t) * (size_t)zonalq_words(s);
    DevMem dhist, drow, dpre;
    int rc = dhist.alloc(ctx, hist_bytes, "mod16_zonal_hist: device memory for the table");
    if (rc != MOD16_OK) return rc;
    if (s.weight_kind == MOD16_ZONAL_WEIGHT_ROW) {
        int64_t r0, r1;
        zonalq_rows(s, &r0, &r1);
        const size_t bytes = sizeof(double) * (size_t)(r1 - r0 + 1);
        rc = drow.alloc(ctx, bytes, "mod16_zonal_hist: device memory for the per-row weights");
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(drow.get(), static_cast<const double*>(a.weights) + r0, bytes, hipMemcpyHostToDevice));
        a.row0 = r0;
    }
    if (prefix) {
        const size_t bytes = sizeof(uint64_t) * (size_t)s.layers * (size_t)s.nzones * (size_t)s.slots;
        rc = dpre.alloc(ctx, bytes, "mod16_zonal_hist: device memory for the prefixes");
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(dpre.get(), prefix, bytes, hipMemcpyHostToDevice));
        a.prefix = dpre.as<unsigned long long>();
    }
    HIPCHK(ctx, hipMemcpy(dhist.get(), hist, hist_bytes, hipMemcpyHostToDevice));
    HostPlan p((int)sizeof(T));
    const bool pixel_w = s.weight_kind == MOD16_ZONAL_WEIGHT_PIXEL;
    p.add(kIn, a.values, false, s.layers, s.value_pitch);                       // 0
    p.add(kIn, pixel_w ? a.weights : nullptr, false);                            // 1
    if (zsz == 1) p.add(kIn, a.zones, true);                                     // 2: a byte row
    else p.add(kIn, a.zones, false, 1, 0, (int)zsz);                             // 2: in a T-sized place
    auto launch = [&](const HostTile& t) {
        ZonalHistArgs d = a;
        d.n = t.m;
        d.values = t.dev[0];
        d.pitch = (int64_t)(t.row_bytes / sizeof(T));
        d.zones = t.dev[2];
        d.weights = pixel_w ? t.dev[1] : drow.get();
        d.first_pixel = a.first_pixel + t.off;
        d.hist = dhist.as<unsigned long long>();
        return launch_zonal_hist<T>(ctx, d, s, t.st);
    };
    rc = host_tiled(ctx, p, s.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(T), stage_bytes));
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipMemcpy(hist, dhist.get(), hist_bytes, hipMemcpyDeviceToHost));
    return MOD16_OK;
}

// what the table's shape depends on: checked by mod16_zonal_hist_* and mod16_zonal_select; -> NULL, or what is wrong
static const char* zonal_hist_check_table(const mod16_zonal_hist_spec* s) {
    if (s->layers < 1 || s->layers > 65535) return "layers must be between 1 and 65535";
    if (s->nzones < 1 || s->nzones > (1 << 24)) return "nzones must be between 1 and 2^24";
    if (s->mode != MOD16_ZONAL_HIST_UNIFORM && s->mode != MOD16_ZONAL_HIST_DIGIT)
        return "mode must be MOD16_ZONAL_HIST_UNIFORM or MOD16_ZONAL_HIST_DIGIT";
    if (s->width != 32 && s->width != 64) return "width must be 32 or 64";
    if (s->mode == MOD16_ZONAL_HIST_UNIFORM) {
        if (s->bins < 1 || s->bins > 4094) return "bins must be between 1 and 4094";
        if (!std::isfinite(s->lo) || !std::isfinite(s->hi) || !(s->lo < s->hi)) return "lo and hi must be finite with lo < hi";
        if (!std::isfinite(s->scale) || !(s->scale > 0.0)) return "scale must be finite and positive";
    } else {
        if (s->bits < 4 || s->bits > 12) return "bits must be between 4 and 12";
        if (s->slots < 1 || s->slots > kZonalqMaxSlots) return "slots must be between 1 and 16";
        if (s->level < 0 || s->level >= zonalq_levels(*s)) return "level must be between 0 and ceil(width / bits) - 1";
    }
    if (zonalq_words(*s) > (int64_t(1) << 40)) return "the table would hold more than 2^40 words";
    return nullptr;
}

static const char* zonal_hist_check_spec(const mod16_zonal_hist_spec* s) {
    if (s->n < 0 || s->n > (int64_t(1) << 30)) return "n must be between 0 and 2^30";
    if (const char* what = zonal_hist_check_table(s)) return what;
    if (s->weight_kind != MOD16_ZONAL_WEIGHT_NONE && s->weight_kind != MOD16_ZONAL_WEIGHT_ROW && s->weight_kind != MOD16_ZONAL_WEIGHT_PIXEL)
        return "weight_kind must be MOD16_ZONAL_WEIGHT_NONE, MOD16_ZONAL_WEIGHT_ROW or MOD16_ZONAL_WEIGHT_PIXEL";
    if (s->weight_kind == MOD16_ZONAL_WEIGHT_ROW && s->cols < 1) return "per-row weights need cols >= 1";
    if (s->weight_kind == MOD16_ZONAL_WEIGHT_ROW && (s->first_pixel < 0 || s->first_pixel > (int64_t(1) << 50)))
        return "first_pixel must be between 0 and 2^50";
    if (s->value_pitch < s->n) return "value_pitch must be at least n";
    if (s->zone_type != MOD16_ZONE_U8 && s->zone_type != MOD16_ZONE_U16 && s->zone_type != MOD16_ZONE_I32)
        return "zone_type must be MOD16_ZONE_U8, MOD16_ZONE_U16 or MOD16_ZONE_I32";
    const int64_t f = 31 - (int64_t)s->ew;                 // (in 64 bits: the exponent is the caller's)
    if (f > 900 || f < -900) return "the exponent ew puts the weight scale outside 2^-900 ... 2^900";
    if (!(s->wmax > 0.0) || !(s->wmax <= std::ldexp(1.0, s->ew))) return "the bound must satisfy 0 < wmax <= 2^ew";
    return nullptr;
}

template <typename T>
static int zonal_hist_entry(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const T* values, const void* zones,
                            const void* weights, const uint64_t* prefix, int64_t* hist, int where, void* stream,
                            size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_zonal_hist: ", what); };
    if (!spec || !values || !zones || !hist) return bad("NULL spec, values, zones or hist");
    if (const char* what = zonal_hist_check_spec(spec)) return bad(what);
    if (spec->width != (int)(8 * sizeof(T))) return bad("width must be the bits of the values' type");
    if (spec->weight_kind != MOD16_ZONAL_WEIGHT_NONE && !weights) return bad("NULL weights");
    const bool filtered = spec->mode == MOD16_ZONAL_HIST_DIGIT && spec->level > 0;
    if (filtered && !prefix) return bad("NULL prefix on a level above 0");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int64_t n = spec->n;
    if (n == 0) return MOD16_OK;
    {
        const Extent out = extent(hist, zonalq_words(*spec), sizeof(int64_t));
        Extent ins[4];
        int ni = 0;
        ins[ni++] = extent(values, 1, 0, spec->layers, spec->value_pitch, n, sizeof(T));
        ins[ni++] = extent(zones, n, zonalq_zone_size(spec->zone_type));
        if (spec->weight_kind == MOD16_ZONAL_WEIGHT_PIXEL) ins[ni++] = extent(weights, n, sizeof(T));
        if (spec->weight_kind == MOD16_ZONAL_WEIGHT_ROW) {
            int64_t r0, r1;
            zonalq_rows(*spec, &r0, &r1);
            ins[ni++] = extent(static_cast<const double*>(weights) + r0, r1 - r0 + 1, sizeof(double));
        }
        if (filtered) ins[ni++] = extent(prefix, (int64_t)spec->layers * spec->nzones * spec->slots, sizeof(uint64_t));
        if (overlaps(&out, 1, ins, ni)) return bad("the table overlaps an input");
    }
    ZonalHistArgs a;
    memset(&a, 0, sizeof a);
    a.values = values;
    a.zones = zones;
    a.weights = weights;
    a.prefix = filtered ? reinterpret_cast<const unsigned long long*>(prefix) : nullptr;
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    a.n = n;
    a.pitch = spec->value_pitch;
    a.cols = spec->weight_kind == MOD16_ZONAL_WEIGHT_ROW ? spec->cols : 1;
    a.inv_cols = 1.0 / (double)a.cols;
    a.first_pixel = spec->weight_kind == MOD16_ZONAL_WEIGHT_ROW ? spec->first_pixel : 0;
    a.wmax = spec->wmax;
    a.wexp = 31 - spec->ew;
    a.nzones = spec->nzones;
    a.nb = (int)zonalq_nb(*spec);
    a.slots = (int)zonalq_slots(*spec);
    a.seff = filtered ? spec->slots : 1;
    a.top = 64;
    if (spec->mode == MOD16_ZONAL_HIST_UNIFORM) {
        a.bins = spec->bins;
        a.lo = spec->lo;
        a.hi = spec->hi;
        a.scale = spec->scale;
    } else {
        const int used = spec->level * spec->bits;
        const int d = std::min(spec->bits, spec->width - used);
        if (filtered) a.top = spec->width - used;
        a.low = spec->width - used - d;
        a.mask = (1 << d) - 1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_zonal_hist<T>(ctx, a, *spec, static_cast<hipStream_t>(stream));
    return zonal_hist_host<T>(ctx, *spec, a, filtered ? prefix : nullptr, hist, stage_budget(stage_bytes));
}

// the loop of zonal_select_kernel on the CPU (HOST mode: no device work)
static void zonal_select_host(const ZonalSelectArgs& a, int width) {
    for (int64_t r = 0; r < a.rows; ++r) {
        const int64_t zrow = r / a.slots;
        const int s = (int)(r - zrow * a.slots);
        const unsigned long long* const row = a.hist + (zrow * a.slots + (a.level == 0 ? 0 : s)) * a.nb;
        unsigned long long want;
        if (a.level == 0) {
            unsigned long long total = 0;
            for (int b = 0; b < a.used; ++b) total += row[b];
            want = total ? zonalq_target(a.q_mant[s], a.q_exp[s], total) : 0;
            if (s == 0) a.weight[zrow] = (long long)total;
            a.remaining[r] = 0;
            a.prefix[r] = 0;
        } else {
            want = (unsigned long long)a.remaining[r];
        }
        unsigned long long run = 0;
        int b = 0;
        bool found = false;
        if (want != 0)
            for (; b < a.used; ++b) {
                if (run + row[b] >= want) { found = true; break; }
                run += row[b];
            }
        if (found) {
            a.prefix[r] = (a.prefix[r] << a.dbits) | (unsigned long long)b;
            a.remaining[r] = (long long)(want - run);
        } else {
            a.remaining[r] = 0;
        }
        if (!a.last) continue;
        if (width == 64) {
            const unsigned long long k = a.prefix[r];
            const unsigned long long bits = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
            double v;
            memcpy(&v, &bits, sizeof v);
            static_cast<double*>(a.values)[r] = found ? v : std::nan("");
        } else {
            const uint32_t k = (uint32_t)a.prefix[r];
            const uint32_t bits = k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu);
            float v;
            memcpy(&v, &bits, sizeof v);
            static_cast<float*>(a.values)[r] = found ? v : std::nanf("");
        }
    }
}

extern "C" int mod16_zonal_hist_f64(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const double* values, const void* zones,
                                    const void* weights, const uint64_t* prefix, int64_t* hist, int where, void* stream,
                                    size_t stage_bytes) {
    return zonal_hist_entry<double>(ctx, spec, values, zones, weights, prefix, hist, where, stream, stage_bytes);
}
extern "C" int mod16_zonal_hist_f32(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const float* values, const void* zones,
                                    const void* weights, const uint64_t* prefix, int64_t* hist, int where, void* stream,
                                    size_t stage_bytes) {
    return zonal_hist_entry<float>(ctx, spec, values, zones, weights, prefix, hist, where, stream, stage_bytes);
}

extern "C" int mod16_zonal_select(mod16_ctx* ctx, const mod16_zonal_hist_spec* spec, const int64_t* hist, const int64_t* q_mant,
                                  const int32_t* q_exp, int64_t* remaining, uint64_t* prefix, void* out_values, int64_t* weight,
                                  int where, void* stream) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_zonal_select: ", what); };
    if (!spec || !hist || !remaining || !prefix) return bad("NULL spec, hist, remaining or prefix");
    if (const char* what = zonal_hist_check_table(spec)) return bad(what);
    if (spec->mode != MOD16_ZONAL_HIST_DIGIT) return bad("mode must be MOD16_ZONAL_HIST_DIGIT");
    const bool last = spec->level == zonalq_levels(*spec) - 1;
    if (spec->level == 0 && (!q_mant || !q_exp || !weight)) return bad("level 0 needs q_mant, q_exp and weight");
    if (last && !out_values) return bad("the last level needs out_values");
    if (const char* what = check_where(where)) return bad(what);
    ZonalSelectArgs a;
    memset(&a, 0, sizeof a);
    if (spec->level == 0)
        for (int s = 0; s < spec->slots; ++s) {
            // q = M / 2^E in [0, 1]: M < 2^53 and E >= 52 (E < 52 would put q above 1)
            if (q_mant[s] < 0 || q_mant[s] >= (int64_t(1) << 53) || q_exp[s] < 52 || q_exp[s] > 1200)
                return bad("a quantile must be M / 2^E with 0 <= M < 2^53 and 52 <= E <= 1200");
            if (q_exp[s] == 52 && q_mant[s] > (int64_t(1) << 52)) return bad("a quantile lies above 1");
            a.q_mant[s] = (unsigned long long)q_mant[s];
            a.q_exp[s] = q_exp[s];
        }
    const int64_t rows = (int64_t)spec->layers * spec->nzones * spec->slots;
    {
        const Extent in = extent(hist, zonalq_words(*spec), sizeof(int64_t));
        Extent outs[4];
        int no = 0;
        outs[no++] = extent(remaining, rows, sizeof(int64_t));
        outs[no++] = extent(prefix, rows, sizeof(uint64_t));
        if (last) outs[no++] = extent(out_values, rows, (size_t)spec->width / 8);
        if (spec->level == 0) outs[no++] = extent(weight, rows / spec->slots, sizeof(int64_t));
        if (overlaps(outs, no, &in, 1)) return bad("an output overlaps the table or another output");
    }
    const int used = spec->level * spec->bits;
    a.hist = reinterpret_cast<const unsigned long long*>(hist);
    a.remaining = reinterpret_cast<long long*>(remaining);
    a.prefix = reinterpret_cast<unsigned long long*>(prefix);
    a.values = out_values;
    a.weight = reinterpret_cast<long long*>(weight);
    a.rows = rows;
    a.slots = spec->slots;
    a.nb = 1 << spec->bits;
    a.dbits = std::min(spec->bits, spec->width - used);
    a.used = 1 << a.dbits;
    a.level = spec->level;
    a.last = last ? 1 : 0;
    if (where == MOD16_HOST) {
        zonal_select_host(a, spec->width);
        return MOD16_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t)ctx->cus * 32)));
    if (spec->width == 64) hipLaunchKernelGGL((zonal_select_kernel<double>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((zonal_select_kernel<float>), grid, dim3(kBlock), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

extern "C" int mod16_zonal_hist_lds_bytes(void) { return kZonalqLdsWords * (int)sizeof(int64_t); }
