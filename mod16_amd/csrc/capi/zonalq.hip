// libmod16hip.so -- zonal histograms and exact zonal quantiles: mod16_zonal_hist_f64 / _f32 (the uniform histogram, or one level's digit histogram under the prefix filter, ADDED into an int64 table), mod16_zonal_select (closes a level: target, prefix scan, the next prefix, the value at the end), mod16_zonal_hist_lds_bytes
#include "zonal_common.hpp"
#include "../mod16_zonalq.hpp"

namespace {
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

// All pointers are device pointers here; a.n > 0.
template <typename T>
static int launch_zonal_hist(mod16_ctx* ctx, ZonalHistArgs a, const mod16_zonal_hist_spec& s, hipStream_t st) {
    a.wide = zonal_wide<T>(a, s);
    zonal_dispatch(s.zone_type, s.weight_kind, [&](auto zt, auto wk) {
        using ZT = decltype(zt);
        constexpr int WK = decltype(wk)::value;
        if (s.mode == MOD16_ZONAL_HIST_UNIFORM) zonalq_launch_lw<T, ZT, WK, kZonalqUniform>(a, ctx->cus, s.layers, st);
        else zonalq_launch_lw<T, ZT, WK, kZonalqDigit>(a, ctx->cus, s.layers, st);
    });
    HIPCHK(ctx, hipGetLastError());
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
    if (const char* what = zonal_check_geometry(s)) return what;
    if (const char* what = zonal_check_zone_type(s->zone_type)) return what;
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
    if (spec->n == 0) return MOD16_OK;
    const int64_t nprefix = filtered ? (int64_t)spec->layers * spec->nzones * spec->slots : 0;
    {
        const Extent out = extent(hist, zonalq_words(*spec), sizeof(int64_t));
        Extent ins[4];
        int ni = zonal_input_extents(*spec, values, zones, weights, ins);
        if (filtered) ins[ni++] = extent(prefix, nprefix, sizeof(uint64_t));
        if (overlaps(&out, 1, ins, ni)) return bad("the table overlaps an input");
    }
    ZonalHistArgs a;
    memset(&a, 0, sizeof a);
    zonal_fill_geometry(a, *spec, values, zones, weights);
    a.prefix = filtered ? reinterpret_cast<const unsigned long long*>(prefix) : nullptr;
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    a.wmax = spec->wmax;
    a.wexp = 31 - spec->ew;
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
    // HOST mode: as mod16_zonal_* (zonal_host_tiled); the prefixes go up once, before the table
    DevMem dpre;
    if (filtered) {
        const size_t bytes = sizeof(uint64_t) * (size_t)nprefix;
        const int rc = dpre.alloc(ctx, bytes, "mod16_zonal_hist: device memory for the prefixes");
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(dpre.get(), prefix, bytes, hipMemcpyHostToDevice));
        a.prefix = dpre.as<unsigned long long>();
    }
    return zonal_host_tiled<T>(ctx, *spec, a, hist, sizeof(int64_t) * (size_t)zonalq_words(*spec),
                               "mod16_zonal_hist: device memory for the table",
                               "mod16_zonal_hist: device memory for the per-row weights", stage_budget(stage_bytes),
                               [&](const ZonalGeom& g, void* dhist, hipStream_t st) {
                                   ZonalHistArgs d = a;
                                   static_cast<ZonalGeom&>(d) = g;
                                   d.hist = static_cast<unsigned long long*>(dhist);
                                   return launch_zonal_hist<T>(ctx, d, *spec, st);
                               });
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
