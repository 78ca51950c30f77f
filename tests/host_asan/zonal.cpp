// Stand-alone driver of tests/test_zonal_host_asan.py: the HOST mode of mod16_zonal_* and
// mod16_zonal_bounds_* -- the library's own host code under AddressSanitizer +
// UndefinedBehaviorSanitizer, linked against the HIP stand-in of tests/host_asan (device memory = host
// heap filled with 0xA5, a launch = its shape check; the zonal kernels have no shadow there). Every
// host array sits between guard bytes; 1237 pixels in tiles of 256, of 512 and in one tile; K = 3
// layers with a value pitch above n; all three zone types; all three weight kinds with cols = 67 and
// first_pixel = 5. No kernel runs, so the accumulator comes back as it went up: the round trip is
// checked word for word. Pass: no sanitizer report, no guard byte touched, nothing left allocated,
// every refusal returned before acc is touched.
#include <cmath>

#define HARNESS_NAME "host_asan_zonal"
#include "harness.hpp"

constexpr int64_t kN = 1237, kCols = 67, kFirst = 5;
constexpr int kLayers = 3, kZones = 40;
constexpr unsigned char kAccByte = 0x17;

static bool all(Guarded& g, unsigned char v) {
    for (size_t i = 0; i < g.bytes; ++i)
        if (g.data()[i] != v) return false;
    return true;
}

static mod16_zonal_spec base_spec(int zone_type, int weight_kind) {
    mod16_zonal_spec s;
    memset(&s, 0, sizeof s);
    s.n = kN;
    s.layers = kLayers;
    s.nzones = kZones;
    s.zone_type = zone_type;
    s.weight_kind = weight_kind;
    s.cols = kCols;
    s.first_pixel = kFirst;
    s.value_pitch = kN + 19;
    s.ew = 18; s.ex = 6;
    s.wmax = 2.5e5; s.xmax = 50.0;
    return s;
}

template <typename T>
static void run(mod16_ctx* ctx, const char* what) {
    const int zone_types[] = {MOD16_ZONE_U8, MOD16_ZONE_U16, MOD16_ZONE_I32};
    const size_t zone_size[] = {1, 2, 4};
    for (int zt = 0; zt < 3; ++zt)
        for (int wk = 0; wk < 3; ++wk) {
            const mod16_zonal_spec spec = base_spec(zone_types[zt], wk);
            Guarded values(((size_t)(kLayers - 1) * spec.value_pitch + kN) * sizeof(T), 0);
            Guarded zones((size_t)kN * zone_size[zt], 0);
            const int64_t rows = (kFirst + kN - 1) / kCols + 1;
            Guarded weights(wk == MOD16_ZONAL_WEIGHT_ROW ? (size_t)rows * sizeof(double) : (size_t)kN * sizeof(T), 0);
            // the slab of a slot: the values' rows, the weights' place and (2 / 4-byte ids) the zones' as
            // T-sized rows, uint8 ids as a byte row
            const int nwide = 2 + (zt ? 1 : 0), wide_rows = kLayers + 1 + (zt ? 1 : 0), byte_rows = zt ? 0 : 1;
            const size_t fixed = (size_t)nwide * 33 * 1024 + 512, per_pixel = (size_t)wide_rows * sizeof(T) + byte_rows;
            // tiles of 256 and of 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
            const size_t stages[] = {fixed + 300 * per_pixel, fixed + 600 * per_pixel, 0};
            for (size_t stage : stages) {
                Guarded acc((size_t)kLayers * kZones * 10 * sizeof(int64_t), kAccByte);
                const void* w = wk == MOD16_ZONAL_WEIGHT_NONE ? nullptr : weights.data();
                int rc;
                double wmax = -1.0, xmax = -1.0;
                if (sizeof(T) == 8) {
                    rc = mod16_zonal_f64(ctx, &spec, reinterpret_cast<const double*>(values.data()), zones.data(), w,
                                         reinterpret_cast<int64_t*>(acc.data()), MOD16_HOST, nullptr, stage);
                    if (rc == MOD16_OK)
                        rc = mod16_zonal_bounds_f64(ctx, &spec, reinterpret_cast<const double*>(values.data()), w, &wmax, &xmax,
                                                    MOD16_HOST, nullptr, stage);
                } else {
                    rc = mod16_zonal_f32(ctx, &spec, reinterpret_cast<const float*>(values.data()), zones.data(), w,
                                         reinterpret_cast<int64_t*>(acc.data()), MOD16_HOST, nullptr, stage);
                    if (rc == MOD16_OK)
                        rc = mod16_zonal_bounds_f32(ctx, &spec, reinterpret_cast<const float*>(values.data()), w, &wmax, &xmax,
                                                    MOD16_HOST, nullptr, stage);
                }
                if (rc != MOD16_OK) {
                    fprintf(stderr, "host_asan_zonal: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                    exit(1);
                }
                // (no kernel ran: the accumulator's round trip, and the maxima the stand-in's zeroed words give)
                EXPECT(acc.guards_intact() && all(acc, kAccByte));
                EXPECT(xmax == 0.0 && wmax == (wk == MOD16_ZONAL_WEIGHT_NONE ? 1.0 : 0.0));
            }
            EXPECT(values.guards_intact() && zones.guards_intact() && weights.guards_intact());
        }
    printf("host_asan_zonal: %s done\n", what);
}

// refused before any device work, acc untouched; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const mod16_zonal_spec spec = base_spec(MOD16_ZONE_I32, MOD16_ZONAL_WEIGHT_PIXEL);
    Guarded values(((size_t)(kLayers - 1) * spec.value_pitch + kN) * sizeof(double), 0);
    Guarded zones((size_t)kN * 4, 0), weights((size_t)kN * sizeof(double), 0);
    Guarded acc((size_t)kLayers * kZones * 10 * sizeof(int64_t), kAccByte);
    const double* v = reinterpret_cast<const double*>(values.data());
    int64_t* a = reinterpret_cast<int64_t*>(acc.data());
    auto call = [&](const mod16_zonal_spec& s, const double* vv, const void* zz, const void* ww, int64_t* aa, int where) {
        const int rc = mod16_zonal_f64(ctx, &s, vv, zz, ww, aa, where, nullptr, 0);
        if (rc == MOD16_ERR_ARG) EXPECT(strstr(mod16_last_error(ctx), "mod16_zonal: ") != nullptr);
        return rc;
    };
    EXPECT(mod16_zonal_f64(ctx, nullptr, v, zones.data(), weights.data(), a, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(call(spec, nullptr, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, v, nullptr, weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, v, zones.data(), nullptr, a, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, v, zones.data(), weights.data(), nullptr, MOD16_HOST) == MOD16_ERR_ARG);
    mod16_zonal_spec s = spec;
    s.n = -1; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.n = (int64_t(1) << 30) + 1; s.value_pitch = s.n; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.layers = 0; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.layers = 65536; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.nzones = 0; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.nzones = (1 << 24) + 1; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.zone_type = 3; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.weight_kind = 3; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, v, zones.data(), weights.data(), a, 7) == MOD16_ERR_ARG);
    s = spec; s.weight_kind = MOD16_ZONAL_WEIGHT_ROW; s.cols = 0; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.weight_kind = MOD16_ZONAL_WEIGHT_ROW; s.first_pixel = -1; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.value_pitch = kN - 1; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.ew = 963; s.wmax = 1.0; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.ex = -500; s.xmax = 1e-200; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.ew = INT32_MIN; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.wmax = 3e5; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.xmax = std::nan(""); EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.xmax = 0.0; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_ERR_ARG);
    // an accumulator on the values, on the zone ids, on the weights
    EXPECT(call(spec, v, zones.data(), weights.data(), reinterpret_cast<int64_t*>(values.data()) + 1, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "overlaps") != nullptr);
    EXPECT(call(spec, v, zones.data(), a + 7, a, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, v, a, weights.data(), a, MOD16_DEVICE) == MOD16_ERR_ARG);
    double wmax = 0.0, xmax = 0.0;
    s = spec; s.layers = 0;
    EXPECT(mod16_zonal_bounds_f64(ctx, &s, v, weights.data(), &wmax, &xmax, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "mod16_zonal_bounds: ") != nullptr);
    EXPECT(mod16_zonal_bounds_f64(ctx, &spec, v, weights.data(), nullptr, &xmax, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(mod16_zonal_bounds_f64(ctx, &spec, v, nullptr, &wmax, &xmax, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.n = 0; EXPECT(call(s, v, zones.data(), weights.data(), a, MOD16_HOST) == MOD16_OK);
    EXPECT(acc.guards_intact() && all(acc, kAccByte));
    EXPECT(values.guards_intact() && all(values, 0) && zones.guards_intact() && weights.guards_intact());
    EXPECT(mod16_zonal_lds_zones() >= 256);
    printf("host_asan_zonal: refusals done\n");
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    run<double>(ctx, "float64");
    run<float>(ctx, "float32");
    refusals(ctx);
    harness_finish(ctx);
    return 0;
}
