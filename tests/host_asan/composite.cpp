// Stand-alone driver of tests/test_composite_host_asan.py: the HOST mode of mod16_et_composite_* --
// the library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the
// HIP stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape
// check; the composite kernels have no shadow there). Every host array sits between guard bytes;
// the sizes make the tiles ragged and the last period short. Pass: no sanitizer report, every output
// element overwritten, no guard byte and no padding byte of a pitched output touched.
#include <algorithm>

#define HARNESS_NAME "host_asan_composite"
#include "harness.hpp"

template <typename T> static Guarded input(size_t count, T value) {
    Guarded g(count * sizeof(T), 0);
    for (size_t i = 0; i < count; ++i) g.as<T>()[i] = value;
    return g;
}

template <typename T>
static void run(mod16_ctx* ctx, int (*fn)(mod16_ctx*, const mod16_composite_spec*, const uint8_t*, const T* const*, const T*, T*, T*,
                                          uint16_t*, uint16_t*, int64_t, unsigned, int, void*, int64_t),
                const char* what) {
    const int64_t n = 1237, pitch = n + 19;
    const int K = 11, L = 4, P = 3;                   // periods of 4, 4 and 3 days
    mod16_composite_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.n = n;
    spec.days = K;
    spec.period_days = L;
    spec.min_valid = 2;
    spec.rescale = 1;
    std::vector<Guarded> in;
    const T* drivers[MOD16_N_DRIVERS];
    in.reserve(MOD16_N_DRIVERS + 1);
    for (int k = 0; k < MOD16_N_DRIVERS; ++k) {
        int slabs;
        if (k == MOD16_SW_RAD_NIGHT) {                // a broadcast scalar
            spec.pixel_stride[k] = 0; spec.time_stride[k] = 0; spec.every[k] = K; slabs = 1;
            in.push_back(input<T>(1, (T)0));
        } else if (k == MOD16_TEMP_ANNUAL || k == MOD16_PRESSURE) {      // constant in time
            spec.pixel_stride[k] = 1; spec.time_stride[k] = 0; spec.every[k] = 4096; slabs = 1;
            in.push_back(input<T>((size_t)n, (T)1.5));
        } else if (k == MOD16_SW_ALBEDO || k == MOD16_FPAR || k == MOD16_LAI) {   // 4-day slabs, pitched
            spec.pixel_stride[k] = 1; spec.time_stride[k] = pitch; spec.every[k] = 4; slabs = 3;
            in.push_back(input<T>((size_t)(slabs - 1) * pitch + n, (T)1.5));
        } else {                                      // daily, back to back
            spec.pixel_stride[k] = 1; spec.time_stride[k] = n; spec.every[k] = 1; slabs = K;
            in.push_back(input<T>((size_t)slabs * n, (T)1.5));
        }
        drivers[k] = in.back().template as<T>();
    }
    spec.hours_pixel_stride = 1; spec.hours_time_stride = n; spec.hours_every = 1;
    Guarded hours = input<T>((size_t)K * n, (T)12);
    Guarded cls = input<uint8_t>((size_t)n, (uint8_t)1);
    const size_t out_count = (size_t)(P - 1) * pitch + n;
    // 20 arrays, 19 of them T-sized (33 KiB of stagger each), in 111 slab rows of inputs (the scalar keeps
    // a place) and 12 of outputs (6 without the optional ones): these stage sizes give tiles of 256 and
    // 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
    const int64_t stages[] = {(int64_t)19 * 33 * 1024 + 512 + 300 * (123 * (int64_t)sizeof(T) + 1),
                              (int64_t)19 * 33 * 1024 + 512 + 600 * (123 * (int64_t)sizeof(T) + 1), 0};
    for (int64_t stage : stages)
        for (int all = 0; all < 2; ++all) {
            Guarded et(out_count * sizeof(T), kFresh), pet(out_count * sizeof(T), kFresh);
            Guarded cet(out_count * 2, kFresh), cpet(out_count * 2, kFresh);
            const int rc = fn(ctx, &spec, cls.as<uint8_t>(), drivers, hours.as<T>(), et.as<T>(), all ? pet.as<T>() : nullptr,
                              all ? cet.as<uint16_t>() : nullptr, all ? cpet.as<uint16_t>() : nullptr, pitch,
                              all ? MOD16_MATH_EXACT : MOD16_MATH_FAST, MOD16_HOST, nullptr, stage);
            if (rc != MOD16_OK) {
                fprintf(stderr, "host_asan_composite: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                exit(1);
            }
            check_written(et, P, pitch, n, sizeof(T), true, "out_et");
            check_written(pet, P, pitch, n, sizeof(T), all != 0, "out_pet");
            check_written(cet, P, pitch, n, 2, all != 0, "count_et");
            check_written(cpet, P, pitch, n, 2, all != 0, "count_pet");
        }
    for (Guarded& g : in) EXPECT(g.guards_intact());
    EXPECT(hours.guards_intact() && cls.guards_intact());
    // refused before any device work; n = 0 is fine
    Guarded et(out_count * sizeof(T), kFresh);
    auto call = [&](const mod16_composite_spec& s, int64_t op, unsigned flags, uint16_t* cpet, int64_t stage) {
        return fn(ctx, &s, cls.as<uint8_t>(), drivers, hours.as<T>(), et.as<T>(), nullptr, nullptr, cpet, op, flags, MOD16_HOST, nullptr, stage);
    };
    uint16_t dummy = 0;
    mod16_composite_spec s = spec;
    s.days = 0; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.days = 4097; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.period_days = 0; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.min_valid = L + 1; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.rescale = 2; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.every[MOD16_FPAR] = 0; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.pixel_stride[MOD16_LAI] = 2; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.time_stride[MOD16_LAI] = n - 1; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.every[MOD16_SW_RAD_NIGHT] = 1; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    s = spec; s.hours_every = 0; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(call(spec, n - 1, 0, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(call(spec, pitch, MOD16_MATH_MIXED, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(call(spec, pitch, MOD16_DOMAIN_TRUSTED, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(call(spec, pitch, 0, &dummy, 0) == MOD16_ERR_ARG);
    EXPECT(call(spec, pitch, 0, nullptr, -1) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "stage_bytes") != nullptr);
    s = spec; s.n = 0; EXPECT(call(s, pitch, 0, nullptr, 0) == MOD16_OK);
    check_written(et, P, pitch, n, sizeof(T), false, "out_et of the refused calls");
    printf("host_asan_composite: %s done\n", what);
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    double lut[MOD16_N_CLASSES * MOD16_N_PARAMS];
    for (int i = 0; i < MOD16_N_CLASSES * MOD16_N_PARAMS; ++i) lut[i] = 1.0 + i;
    EXPECT(mod16_set_bplut_f64(ctx, lut) == MOD16_OK);
    run<double>(ctx, mod16_et_composite_f64, "float64");
    run<float>(ctx, mod16_et_composite_f32, "float32");
    harness_finish(ctx);
    return 0;
}
