// Stand-alone driver of tests/test_zonalq_host_asan.py: the HOST mode of mod16_zonal_hist_* and of
// mod16_zonal_select -- the library's own host code under AddressSanitizer +
// UndefinedBehaviorSanitizer, linked against the HIP stand-in of tests/host_asan (device memory = host
// heap filled with 0xA5, a launch = its shape check; the histogram kernels have no shadow there). Every
// host array sits between guard bytes; 1237 pixels in tiles of 256, of 512 and in one tile; K = 3
// layers with a value pitch above n; all three zone types; all three weight kinds with cols = 67 and
// first_pixel = 5; uniform mode and digit mode on level 0 and on a level with prefixes. No kernel runs,
// so the table comes back as it went up: the round trip is checked word for word. The CPU selection
// loop really runs: a hand-made table is selected level by level, float32 with 11 bits (3 levels, the
// last of 10 bits) and float64 with 12 bits (6 levels, the last of 4), and the values are checked. Pass:
// no sanitizer report, no guard byte touched, nothing left allocated, every refusal returned before an
// output is touched.
#include <cmath>

#define HARNESS_NAME "host_asan_zonalq"
#include "harness.hpp"

constexpr int64_t kN = 1237, kCols = 67, kFirst = 5;
constexpr int kLayers = 3, kZones = 40, kSlots = 3, kBits = 8, kBins = 50;
constexpr unsigned char kTableByte = 0x17;

static bool all(Guarded& g, unsigned char v) {
    for (size_t i = 0; i < g.bytes; ++i)
        if (g.data()[i] != v) return false;
    return true;
}

static mod16_zonal_hist_spec base_spec(int zone_type, int weight_kind, int mode, int level, int width) {
    mod16_zonal_hist_spec s;
    memset(&s, 0, sizeof s);
    s.n = kN;
    s.layers = kLayers;
    s.nzones = kZones;
    s.zone_type = zone_type;
    s.weight_kind = weight_kind;
    s.cols = kCols;
    s.first_pixel = kFirst;
    s.value_pitch = kN + 19;
    s.ew = 18;
    s.wmax = 2.5e5;
    s.mode = mode;
    s.width = width;
    s.bins = kBins;
    s.lo = -1.0;
    s.hi = 9.0;
    s.scale = kBins / 10.0;
    s.bits = kBits;
    s.level = level;
    s.slots = kSlots;
    return s;
}

static size_t table_words(const mod16_zonal_hist_spec& s) {
    return s.mode == MOD16_ZONAL_HIST_UNIFORM ? (size_t)s.layers * s.nzones * (s.bins + 2)
                                              : (size_t)s.layers * s.nzones * s.slots * ((size_t)1 << s.bits);
}

template <typename T>
static int hist_call(mod16_ctx* ctx, const mod16_zonal_hist_spec& s, const void* v, const void* z, const void* w, const void* pre,
                     void* hist, int where, size_t stage) {
    if (sizeof(T) == 8)
        return mod16_zonal_hist_f64(ctx, &s, static_cast<const double*>(v), z, w, static_cast<const uint64_t*>(pre),
                                    static_cast<int64_t*>(hist), where, nullptr, stage);
    return mod16_zonal_hist_f32(ctx, &s, static_cast<const float*>(v), z, w, static_cast<const uint64_t*>(pre),
                                static_cast<int64_t*>(hist), where, nullptr, stage);
}

template <typename T>
static void run(mod16_ctx* ctx, const char* what) {
    const int zone_types[] = {MOD16_ZONE_U8, MOD16_ZONE_U16, MOD16_ZONE_I32};
    const size_t zone_size[] = {1, 2, 4};
    const int modes[][2] = {{MOD16_ZONAL_HIST_UNIFORM, 0}, {MOD16_ZONAL_HIST_DIGIT, 0}, {MOD16_ZONAL_HIST_DIGIT, 2}};
    for (int zt = 0; zt < 3; ++zt)
        for (int wk = 0; wk < 3; ++wk)
            for (const auto& m : modes) {
                const mod16_zonal_hist_spec spec = base_spec(zone_types[zt], wk, m[0], m[1], 8 * (int)sizeof(T));
                Guarded values(((size_t)(kLayers - 1) * spec.value_pitch + kN) * sizeof(T), 0);
                Guarded zones((size_t)kN * zone_size[zt], 0);
                const int64_t rows = (kFirst + kN - 1) / kCols + 1;
                Guarded weights(wk == MOD16_ZONAL_WEIGHT_ROW ? (size_t)rows * sizeof(double) : (size_t)kN * sizeof(T), 0);
                Guarded prefix((size_t)kLayers * kZones * kSlots * sizeof(uint64_t), 0);
                // the slab of a slot: as for mod16_zonal_* (tests/host_asan/zonal.cpp)
                const int nwide = 2 + (zt ? 1 : 0), wide_rows = kLayers + 1 + (zt ? 1 : 0), byte_rows = zt ? 0 : 1;
                const size_t fixed = (size_t)nwide * 33 * 1024 + 512, per_pixel = (size_t)wide_rows * sizeof(T) + byte_rows;
                // tiles of 256 and of 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
                const size_t stages[] = {fixed + 300 * per_pixel, fixed + 600 * per_pixel, 0};
                for (size_t stage : stages) {
                    Guarded hist(table_words(spec) * sizeof(int64_t), kTableByte);
                    const void* w = wk == MOD16_ZONAL_WEIGHT_NONE ? nullptr : weights.data();
                    const int rc = hist_call<T>(ctx, spec, values.data(), zones.data(), w, m[1] ? prefix.data() : nullptr,
                                                hist.data(), MOD16_HOST, stage);
                    if (rc != MOD16_OK) {
                        fprintf(stderr, "host_asan_zonalq: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                        exit(1);
                    }
                    EXPECT(hist.guards_intact() && all(hist, kTableByte));      // (no kernel ran: the table's round trip)
                }
                EXPECT(values.guards_intact() && zones.guards_intact() && weights.guards_intact() && prefix.guards_intact());
            }
    printf("host_asan_zonalq: %s done\n", what);
}

// The CPU selection loop on a hand-made table: one layer, two zones, three slots. Zone 0 holds the
// keys of `vals` with the weight words `wts`; zone 1 is empty. The table of each level is built here
// from the keys (what the kernel would have counted) and closed by mod16_zonal_select in HOST mode.
template <typename T, typename U>
static void select_run(mod16_ctx* ctx, int bits, const char* what) {
    const int width = 8 * (int)sizeof(T), levels = (width + bits - 1) / bits, nb = 1 << bits;
    const T vals[] = {(T)-INFINITY, (T)-2.5, (T)-0.0, (T)0.0, (T)1.0, std::nextafter((T)1.0, (T)2.0), (T)7.25, (T)INFINITY};
    const int64_t wts[] = {1, 2, 3, 1, 5, 5, 2, 1};                          // W = 20
    const int nv = 8;
    U keys[8];
    for (int i = 0; i < nv; ++i) {
        U b;
        memcpy(&b, &vals[i], sizeof b);
        keys[i] = (b >> (width - 1)) ? (U)~b : (U)(b | ((U)1 << (width - 1)));
    }
    // q = 0 -> target 1 -> -inf; q = 0.5 -> target 10 -> 1.0 (cumulative 1 3 6 7 12); q = 1 -> target 20 -> +inf
    const int64_t q_mant[kSlots] = {0, int64_t(1) << 52, int64_t(1) << 52};
    const int32_t q_exp[kSlots] = {53, 53, 52};
    mod16_zonal_hist_spec spec = base_spec(MOD16_ZONE_U8, MOD16_ZONAL_WEIGHT_NONE, MOD16_ZONAL_HIST_DIGIT, 0, width);
    spec.layers = 1;
    spec.nzones = 2;
    spec.bits = bits;
    Guarded hist((size_t)2 * kSlots * nb * sizeof(int64_t), 0);
    Guarded remaining((size_t)2 * kSlots * sizeof(int64_t), kFresh), prefix((size_t)2 * kSlots * sizeof(uint64_t), kFresh);
    Guarded out((size_t)2 * kSlots * sizeof(T), kFresh), weight(2 * sizeof(int64_t), kFresh);
    for (int level = 0; level < levels; ++level) {
        spec.level = level;
        const int used = level * bits, d = bits < width - used ? bits : width - used;
        memset(hist.data(), 0, hist.bytes);
        int64_t* h = hist.as<int64_t>();
        for (int s = 0; s < (level ? kSlots : 1); ++s)
            for (int i = 0; i < nv; ++i) {
                const uint64_t key = (uint64_t)keys[i];
                if (level && (key >> (width - used)) != prefix.as<uint64_t>()[s]) continue;
                h[(size_t)s * nb + ((key >> (width - used - d)) & (((uint64_t)1 << d) - 1))] += wts[i];
            }
        const bool last = level == levels - 1;
        const int rc = mod16_zonal_select(ctx, &spec, h, level ? nullptr : q_mant, level ? nullptr : q_exp, remaining.as<int64_t>(),
                                          prefix.as<uint64_t>(), last ? out.data() : nullptr, level ? nullptr : weight.as<int64_t>(),
                                          MOD16_HOST, nullptr);
        if (rc != MOD16_OK) {
            fprintf(stderr, "host_asan_zonalq: %s level %d: status %d: %s\n", what, level, rc, mod16_last_error(ctx));
            exit(1);
        }
    }
    EXPECT(hist.guards_intact() && remaining.guards_intact() && prefix.guards_intact() && out.guards_intact() && weight.guards_intact());
    EXPECT(weight.as<int64_t>()[0] == 20 && weight.as<int64_t>()[1] == 0);
    const T expect[kSlots] = {(T)-INFINITY, (T)1.0, (T)INFINITY};
    for (int s = 0; s < kSlots; ++s) {
        EXPECT(memcmp(&out.as<T>()[s], &expect[s], sizeof(T)) == 0);
        EXPECT(prefix.as<uint64_t>()[s] == (uint64_t)keys[s == 0 ? 0 : s == 1 ? 4 : 7]);
        EXPECT(remaining.as<int64_t>()[s] >= 1);
        EXPECT(std::isnan(out.as<T>()[kSlots + s]) && remaining.as<int64_t>()[kSlots + s] == 0);      // the empty zone
    }
    printf("host_asan_zonalq: %s done\n", what);
}

// refused before any device work, the table untouched; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const mod16_zonal_hist_spec uni = base_spec(MOD16_ZONE_I32, MOD16_ZONAL_WEIGHT_PIXEL, MOD16_ZONAL_HIST_UNIFORM, 0, 64);
    const mod16_zonal_hist_spec dig = base_spec(MOD16_ZONE_I32, MOD16_ZONAL_WEIGHT_PIXEL, MOD16_ZONAL_HIST_DIGIT, 1, 64);
    Guarded values(((size_t)(kLayers - 1) * uni.value_pitch + kN) * sizeof(double), 0);
    Guarded zones((size_t)kN * 4, 0), weights((size_t)kN * sizeof(double), 0);
    Guarded prefix((size_t)kLayers * kZones * kSlots * sizeof(uint64_t), 0);
    Guarded hist(table_words(dig) * sizeof(int64_t), kTableByte);
    const double* v = reinterpret_cast<const double*>(values.data());
    int64_t* h = hist.as<int64_t>();
    auto call = [&](const mod16_zonal_hist_spec& s, const void* vv, const void* zz, const void* ww, const void* pp, void* hh, int where) {
        const int rc = hist_call<double>(ctx, s, vv, zz, ww, pp, hh, where, 0);
        if (rc == MOD16_ERR_ARG) EXPECT(strncmp(mod16_last_error(ctx), "mod16_zonal_hist: ", 18) == 0);
        return rc;
    };
    auto bad = [&](const mod16_zonal_hist_spec& s) { return call(s, v, zones.data(), weights.data(), prefix.data(), h, MOD16_HOST) == MOD16_ERR_ARG; };
    EXPECT(mod16_zonal_hist_f64(ctx, nullptr, v, zones.data(), weights.data(), nullptr, h, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(call(uni, nullptr, zones.data(), weights.data(), nullptr, h, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(uni, v, nullptr, weights.data(), nullptr, h, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(uni, v, zones.data(), nullptr, nullptr, h, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(uni, v, zones.data(), weights.data(), nullptr, nullptr, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(dig, v, zones.data(), weights.data(), nullptr, h, MOD16_HOST) == MOD16_ERR_ARG);      // level 1 without prefixes
    EXPECT(call(uni, v, zones.data(), weights.data(), nullptr, h, 7) == MOD16_ERR_ARG);
    // everything mod16_zonal_* refuses
    mod16_zonal_hist_spec s = uni;
    s.n = -1; EXPECT(bad(s));
    s = uni; s.n = (int64_t(1) << 30) + 1; s.value_pitch = s.n; EXPECT(bad(s));
    s = uni; s.layers = 0; EXPECT(bad(s));
    s = uni; s.layers = 65536; EXPECT(bad(s));
    s = uni; s.nzones = 0; EXPECT(bad(s));
    s = uni; s.nzones = (1 << 24) + 1; EXPECT(bad(s));
    s = uni; s.zone_type = 3; EXPECT(bad(s));
    s = uni; s.weight_kind = 3; EXPECT(bad(s));
    s = uni; s.weight_kind = MOD16_ZONAL_WEIGHT_ROW; s.cols = 0; EXPECT(bad(s));
    s = uni; s.weight_kind = MOD16_ZONAL_WEIGHT_ROW; s.first_pixel = -1; EXPECT(bad(s));
    s = uni; s.value_pitch = kN - 1; EXPECT(bad(s));
    s = uni; s.ew = 963; s.wmax = 1.0; EXPECT(bad(s));
    s = uni; s.ew = INT32_MIN; EXPECT(bad(s));
    s = uni; s.wmax = 3e5; EXPECT(bad(s));
    s = uni; s.wmax = std::nan(""); EXPECT(bad(s));
    s = uni; s.wmax = 0.0; EXPECT(bad(s));
    // the histogram's own
    s = uni; s.mode = 2; EXPECT(bad(s));
    s = uni; s.width = 32; EXPECT(bad(s));                   // float64 values
    s = uni; s.width = 16; EXPECT(bad(s));
    s = uni; s.bins = 0; EXPECT(bad(s));
    s = uni; s.bins = 4095; EXPECT(bad(s));
    s = uni; s.lo = std::nan(""); EXPECT(bad(s));
    s = uni; s.hi = INFINITY; EXPECT(bad(s));
    s = uni; s.hi = s.lo; EXPECT(bad(s));
    s = uni; s.hi = s.lo - 1.0; EXPECT(bad(s));
    s = uni; s.scale = INFINITY; EXPECT(bad(s));
    s = uni; s.scale = std::nan(""); EXPECT(bad(s));
    s = uni; s.scale = 0.0; EXPECT(bad(s));
    s = dig; s.bits = 3; EXPECT(bad(s));
    s = dig; s.bits = 13; EXPECT(bad(s));
    s = dig; s.slots = 0; EXPECT(bad(s));
    s = dig; s.slots = 17; EXPECT(bad(s));
    s = dig; s.level = -1; EXPECT(bad(s));
    s = dig; s.level = 8; EXPECT(bad(s));                    // 64 / 8 levels: 0 ... 7
    // a table on the values, on the zone ids, on the weights, on the prefixes
    EXPECT(call(uni, v, zones.data(), weights.data(), nullptr, const_cast<double*>(v) + 1, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "overlaps") != nullptr);
    EXPECT(call(uni, v, h, weights.data(), nullptr, h, MOD16_DEVICE) == MOD16_ERR_ARG);
    EXPECT(call(uni, v, zones.data(), h + 7, nullptr, h, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(dig, v, zones.data(), weights.data(), h + 3, h, MOD16_HOST) == MOD16_ERR_ARG);
    // mod16_zonal_select
    Guarded remaining((size_t)kLayers * kZones * kSlots * sizeof(int64_t), kFresh), out((size_t)kLayers * kZones * kSlots * sizeof(double), kFresh);
    Guarded weight((size_t)kLayers * kZones * sizeof(int64_t), kFresh);
    int64_t mant[kSlots] = {0, int64_t(1) << 52, int64_t(1) << 52};
    int32_t expo[kSlots] = {53, 53, 52};
    auto sel = [&](const mod16_zonal_hist_spec& sp, const int64_t* hh, const int64_t* mm, const int32_t* ee, int64_t* rr, uint64_t* pp,
                   void* oo, int64_t* ww, int where) {
        const int rc = mod16_zonal_select(ctx, &sp, hh, mm, ee, rr, pp, oo, ww, where, nullptr);
        if (rc == MOD16_ERR_ARG) EXPECT(strncmp(mod16_last_error(ctx), "mod16_zonal_select: ", 20) == 0);
        return rc == MOD16_ERR_ARG;
    };
    int64_t* r = remaining.as<int64_t>();
    uint64_t* p = prefix.as<uint64_t>();
    mod16_zonal_hist_spec l0 = dig, l7 = dig;
    l0.level = 0;
    l7.level = 7;
    EXPECT(mod16_zonal_select(ctx, nullptr, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(sel(l0, nullptr, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    EXPECT(sel(l0, h, mant, expo, nullptr, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    EXPECT(sel(l0, h, mant, expo, r, nullptr, nullptr, weight.as<int64_t>(), MOD16_HOST));
    EXPECT(sel(l0, h, nullptr, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    EXPECT(sel(l0, h, mant, nullptr, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    EXPECT(sel(l0, h, mant, expo, r, p, nullptr, nullptr, MOD16_HOST));
    EXPECT(sel(l7, h, nullptr, nullptr, r, p, nullptr, nullptr, MOD16_HOST));          // the last level writes values
    EXPECT(sel(uni, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));   // no selection over a uniform table
    EXPECT(sel(l0, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), 7));
    s = l0; s.bits = 13; EXPECT(sel(s, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    s = l0; s.slots = 17; EXPECT(sel(s, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    s = l0; s.level = 8; EXPECT(sel(s, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    mant[1] = -1; EXPECT(sel(l0, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    mant[1] = int64_t(1) << 53; EXPECT(sel(l0, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));
    mant[1] = int64_t(1) << 52; expo[1] = 51; EXPECT(sel(l0, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));     // q = 2
    mant[1] = (int64_t(1) << 52) + 1; expo[1] = 52; EXPECT(sel(l0, h, mant, expo, r, p, nullptr, weight.as<int64_t>(), MOD16_HOST));   // just above 1
    mant[1] = int64_t(1) << 52; expo[1] = 53;
    EXPECT(sel(l0, h, mant, expo, h + 5, p, nullptr, weight.as<int64_t>(), MOD16_HOST));      // remaining on the table
    EXPECT(sel(l0, h, mant, expo, r, p, nullptr, r + 1, MOD16_HOST));                          // weight on remaining
    s = uni; s.n = 0; EXPECT(call(s, v, zones.data(), weights.data(), nullptr, h, MOD16_HOST) == MOD16_OK);
    EXPECT(hist.guards_intact() && all(hist, kTableByte));
    EXPECT(remaining.guards_intact() && all(remaining, kFresh) && out.guards_intact() && all(out, kFresh));
    EXPECT(weight.guards_intact() && all(weight, kFresh) && prefix.guards_intact() && all(prefix, 0));
    EXPECT(values.guards_intact() && all(values, 0) && zones.guards_intact() && weights.guards_intact());
    EXPECT(mod16_zonal_hist_lds_bytes() >= 13 * 3 * 256 * 8 && 2 * mod16_zonal_hist_lds_bytes() <= 160 * 1024);
    printf("host_asan_zonalq: refusals done\n");
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    run<double>(ctx, "float64");
    run<float>(ctx, "float32");
    select_run<float, uint32_t>(ctx, 11, "select float32");
    select_run<double, uint64_t>(ctx, 12, "select float64");
    refusals(ctx);
    harness_finish(ctx);
    return 0;
}
