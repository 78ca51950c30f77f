// Stand-alone driver of tests/test_composite_downscale_host_asan.py: the HOST mode of
// mod16_et_composite_downscaled_* -- the library's own host code under AddressSanitizer +
// UndefinedBehaviorSanitizer, linked against the HIP stand-in of tests/host_asan (device memory = host
// heap filled with 0xA5, a launch = its shape check; these kernels have no shadow there). Every host
// array sits between guard bytes and is exactly as large as the call may read: a coarse series ends
// with the W elements of its last plane's last row. Pass: no sanitizer report, every output element
// overwritten, no guard byte and no padding byte of a pitched output touched, nothing left allocated.
//   1237 pixels from pixel 777 of a 60 x 47 raster (not row-aligned), K = 11 days in periods of 4:
//   the reanalysis drivers coarse -- daily planes with a row pitch of W + 3 and a time stride of a
//   plane + 5, temp_annual one plane, pressure in two slabs -- the hours coarse too, albedo / fPAR / LAI
//   fine in pitched 4-day slabs; several stage_bytes (5 tiles, 3 tiles, one), with and without the
//   optional outputs; every refusal; n = 0; the coarse upload without memory.
#include <algorithm>

#define HARNESS_NAME "host_asan_composite_downscale"
#include "harness.hpp"

constexpr int64_t R = 60, C = 47, H = 5, W = 7, kPitch = W + 3;
constexpr int64_t kSpan = (H - 1) * kPitch + W;       // a plane, from its first to its last cell
constexpr int64_t kTime = kSpan + 5;                  // between two planes

template <typename T> static Guarded input(size_t count, T value) {
    Guarded g(count * sizeof(T), 0);
    for (size_t i = 0; i < count; ++i) g.as<T>()[i] = value;
    return g;
}

static mod16_downscale* make_grid(mod16_ctx* ctx) {
    mod16_downscale_spec spec = {R, C, H, W, 1, MOD16_DOWNSCALE_COS4};
    std::vector<double> row_pos((size_t)R), col_pos((size_t)C);
    for (int64_t r = 0; r < R; ++r) row_pos[r] = -0.8 + (H + 0.6) * (double)r / (double)R;
    for (int64_t c = 0; c < C; ++c) col_pos[c] = -9.3 + (3.0 * W) * (double)c / (double)C;
    mod16_downscale* grid = nullptr;
    EXPECT(mod16_downscale_create(ctx, &spec, row_pos.data(), col_pos.data(), &grid) == MOD16_OK && grid);
    return grid;
}

template <typename T>
static void run(mod16_ctx* ctx, mod16_ctx* other,
                int (*fn)(mod16_ctx*, const mod16_downscale*, const mod16_composite_downscaled_spec*, const uint8_t*,
                          const T* const*, const T*, T*, T*, uint16_t*, uint16_t*, int64_t, unsigned, int, void*, int64_t),
                const char* what) {
    const int64_t first = 777, n = 1237, pitch = n + 19;
    const int K = 11, L = 4, P = 3;                   // periods of 4, 4 and 3 days
    mod16_downscale* grid = make_grid(ctx);
    mod16_composite_downscaled_spec spec;
    memset(&spec, 0, sizeof spec);
    mod16_composite_spec& cs = spec.composite;
    cs.n = n;
    cs.days = K;
    cs.period_days = L;
    cs.min_valid = 2;
    cs.rescale = 1;
    spec.coarse_pitch = kPitch;
    spec.first_pixel = first;
    std::vector<Guarded> in;
    const T* drivers[MOD16_N_DRIVERS];
    in.reserve(MOD16_N_DRIVERS + 1);
    for (int k = 0; k < MOD16_N_DRIVERS; ++k) {
        if (k == MOD16_SW_ALBEDO || k == MOD16_FPAR || k == MOD16_LAI) {     // fine, 4-day slabs, pitched
            cs.pixel_stride[k] = 1; cs.time_stride[k] = pitch; cs.every[k] = 4;
            in.push_back(input<T>((size_t)2 * pitch + n, (T)1.5));
        } else if (k == MOD16_SW_RAD_NIGHT) {                                // a broadcast scalar
            cs.pixel_stride[k] = 0; cs.time_stride[k] = 0; cs.every[k] = K;
            in.push_back(input<T>(1, (T)0));
        } else {                                                             // coarse
            spec.coarse_mask |= 1u << k;
            cs.pixel_stride[k] = 7;                                          // (not looked at)
            const int slabs = k == MOD16_TEMP_ANNUAL ? 1 : k == MOD16_PRESSURE ? 2 : K;
            cs.every[k] = k == MOD16_TEMP_ANNUAL ? 4096 : k == MOD16_PRESSURE ? 6 : 1;
            cs.time_stride[k] = slabs > 1 ? kTime : 0;
            in.push_back(input<T>((size_t)((slabs - 1) * kTime + kSpan), (T)1.5));
        }
        drivers[k] = in.back().template as<T>();
    }
    spec.coarse_mask |= 1u << 14;                                            // the hours: coarse, daily
    cs.hours_pixel_stride = 0; cs.hours_time_stride = kTime; cs.hours_every = 1;
    Guarded hours = input<T>((size_t)((K - 1) * kTime + kSpan), (T)12);
    Guarded cls = input<uint8_t>((size_t)n, (uint8_t)1);
    const size_t out_count = (size_t)(P - 1) * pitch + n;
    // 20 arrays of the plan, 19 of them T-sized (33 KiB of stagger each), in 9 + 1 + 11 slab rows of
    // inputs (a scalar and a resident array keep a place) and 12 of outputs: these stage sizes give tiles
    // of 256 and 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
    const int64_t stages[] = {(int64_t)19 * 33 * 1024 + 512 + 300 * (33 * (int64_t)sizeof(T) + 1),
                              (int64_t)19 * 33 * 1024 + 512 + 600 * (33 * (int64_t)sizeof(T) + 1), 0};
    for (int64_t stage : stages)
        for (int all = 0; all < 2; ++all) {
            Guarded et(out_count * sizeof(T), kFresh), pet(out_count * sizeof(T), kFresh);
            Guarded cet(out_count * 2, kFresh), cpet(out_count * 2, kFresh);
            const int rc = fn(ctx, grid, &spec, cls.as<uint8_t>(), drivers, hours.as<T>(), et.as<T>(), all ? pet.as<T>() : nullptr,
                              all ? cet.as<uint16_t>() : nullptr, all ? cpet.as<uint16_t>() : nullptr, pitch,
                              all ? MOD16_MATH_EXACT : MOD16_MATH_FAST, MOD16_HOST, nullptr, stage);
            if (rc != MOD16_OK) {
                fprintf(stderr, "host_asan_composite_downscale: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
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
    auto call = [&](const mod16_composite_downscaled_spec& s, int64_t op, unsigned flags, uint16_t* cpet, int64_t stage,
                    const mod16_downscale* g, int where = MOD16_HOST, mod16_ctx* c = nullptr) {
        return fn(c ? c : ctx, g, &s, cls.as<uint8_t>(), drivers, hours.as<T>(), et.as<T>(), nullptr, nullptr, cpet, op, flags,
                  where, nullptr, stage);
    };
    uint16_t dummy = 0;
    mod16_composite_downscaled_spec s = spec;
#define REFUSED(change, text)                                              \
    do {                                                                   \
        s = spec;                                                          \
        change;                                                            \
        EXPECT(refused(ctx, call(s, pitch, 0, nullptr, 0, grid), "mod16_et_composite_downscaled: ", text)); \
    } while (0)
    // what the composite refuses
    REFUSED(s.composite.n = -1, "n < 0");
    REFUSED(s.composite.days = 0, "days must be between 1 and 4096");
    REFUSED(s.composite.days = 4097, "days must be between 1 and 4096");
    REFUSED(s.composite.period_days = 0, "period_days must be at least 1");
    REFUSED(s.composite.min_valid = L + 1, "min_valid must be between 1 and period_days");
    REFUSED(s.composite.rescale = 2, "rescale must be 0 or 1");
    REFUSED(s.composite.every[MOD16_FPAR] = 0, "every must be at least 1");
    REFUSED(s.composite.pixel_stride[MOD16_LAI] = 2, "pixel stride must be 0 or 1");
    REFUSED(s.composite.time_stride[MOD16_LAI] = n - 1, "time stride of an array with several slabs must be at least n");
    REFUSED(s.composite.time_stride[MOD16_TMIN] = -1, "time stride must not be negative");
    REFUSED(s.composite.every[MOD16_SW_RAD_NIGHT] = 1, "a broadcast scalar");
    REFUSED(s.composite.hours_every = 0, "every must be at least 1");
    // what is this entry's own
    REFUSED(s.composite.time_stride[MOD16_TEMP_DAY] = kSpan - 1, "time stride of a coarse array with several slabs must be at least a plane");
    REFUSED(s.composite.hours_time_stride = kSpan - 1, "time stride of a coarse array");
    REFUSED(s.coarse_pitch = W - 1, "coarse_pitch must be at least coarse_cols");
    REFUSED(s.coarse_pitch = ((int64_t)1 << 31) / (H - 1), "a coarse plane with its pitch must hold at most 2^31 - 1 elements");
    REFUSED(s.coarse_pitch = (int64_t)1 << 40, "a coarse plane with its pitch must hold at most 2^31 - 1 elements");
    REFUSED(s.coarse_mask |= 1u << 15, "coarse_mask has a bit above 14");
    REFUSED(s.first_pixel = -1, "leaves the raster");
    REFUSED(s.first_pixel = R * C - n + 1, "leaves the raster");
    REFUSED(s.first_pixel = R * C + 1; s.composite.n = 0, "leaves the raster");
#undef REFUSED
    EXPECT(call(spec, n - 1, 0, nullptr, 0, grid) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "out_pitch must be at least n"));
    EXPECT(call(spec, pitch, MOD16_MATH_MIXED, nullptr, 0, grid) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "MOD16_MATH_MIXED is not available"));
    EXPECT(call(spec, pitch, MOD16_DOMAIN_TRUSTED, nullptr, 0, grid) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "MOD16_DOMAIN_TRUSTED is not available"));
    EXPECT(call(spec, pitch, 64, nullptr, 0, grid) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "unknown flag"));
    EXPECT(call(spec, pitch, 0, &dummy, 0, grid) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "count_pet needs out_pet"));
    EXPECT(call(spec, pitch, 0, nullptr, -1, grid) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "stage_bytes must not be negative"));
    EXPECT(call(spec, pitch, 0, nullptr, 0, grid, 7) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "`where` must be"));
    EXPECT(call(spec, pitch, 0, nullptr, 0, nullptr) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "NULL grid"));
    EXPECT(fn(ctx, grid, nullptr, cls.as<uint8_t>(), drivers, hours.as<T>(), et.as<T>(), nullptr, nullptr, nullptr, pitch, 0, MOD16_HOST,
              nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(fn(ctx, grid, &spec, cls.as<uint8_t>(), drivers, nullptr, et.as<T>(), nullptr, nullptr, nullptr, pitch, 0, MOD16_HOST,
              nullptr, 0) == MOD16_ERR_ARG);
    const T* hole[MOD16_N_DRIVERS];
    memcpy(hole, drivers, sizeof hole);
    hole[MOD16_VPD_DAY] = nullptr;
    EXPECT(fn(ctx, grid, &spec, cls.as<uint8_t>(), hole, hours.as<T>(), et.as<T>(), nullptr, nullptr, nullptr, pitch, 0, MOD16_HOST,
              nullptr, 0) == MOD16_ERR_ARG && strstr(mod16_last_error(ctx), "NULL driver array"));
    EXPECT(fn(nullptr, grid, &spec, cls.as<uint8_t>(), drivers, hours.as<T>(), et.as<T>(), nullptr, nullptr, nullptr, pitch, 0,
              MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    // a context without a parameter table
    EXPECT(call(spec, pitch, 0, nullptr, 0, grid, MOD16_HOST, other) == MOD16_ERR_NO_BPLUT);
    // n = 0 is fine, wherever the (empty) range starts
    s = spec; s.composite.n = 0; EXPECT(call(s, pitch, 0, nullptr, 0, grid) == MOD16_OK);
    s.first_pixel = R * C; EXPECT(call(s, pitch, 0, nullptr, 0, grid) == MOD16_OK);
    check_written(et, P, pitch, n, sizeof(T), false, "out_et of the refused calls");
    EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
    printf("host_asan_composite_downscale: %s done\n", what);
}

// the coarse upload finds no memory: MOD16_ERR_NOMEM, no output touched, and the next call works
static void no_room(mod16_ctx* ctx) {
    mod16_downscale* grid = make_grid(ctx);
    const int64_t n = 300;
    const int K = 5;
    mod16_composite_downscaled_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.composite.n = n;
    spec.composite.days = K;
    spec.composite.period_days = K;
    spec.composite.min_valid = 1;
    spec.coarse_pitch = W;
    spec.coarse_mask = 1u << MOD16_TEMP_DAY;
    Guarded scalar = input<double>(1, 1.5), planes = input<double>((size_t)(K * H * W), 280.0), cls = input<uint8_t>((size_t)n, (uint8_t)1);
    const double* drivers[MOD16_N_DRIVERS];
    for (int k = 0; k < MOD16_N_DRIVERS; ++k) {
        drivers[k] = k == MOD16_TEMP_DAY ? planes.as<double>() : scalar.as<double>();
        spec.composite.every[k] = k == MOD16_TEMP_DAY ? 1 : K;
        spec.composite.time_stride[k] = k == MOD16_TEMP_DAY ? H * W : 0;
    }
    spec.composite.hours_every = K;
    Guarded et((size_t)n * sizeof(double), kFresh);
    mod16_stub_fail_malloc(1);
    EXPECT(mod16_et_composite_downscaled_f64(ctx, grid, &spec, cls.as<uint8_t>(), drivers, scalar.as<double>(), et.as<double>(), nullptr,
                                             nullptr, nullptr, n, 0, MOD16_HOST, nullptr, 0) == MOD16_ERR_NOMEM);
    EXPECT(strstr(mod16_last_error(ctx), "coarse series") != nullptr);
    check_written(et, 1, n, n, sizeof(double), false, "out_et without memory");
    mod16_stub_fail_malloc(0);
    EXPECT(mod16_et_composite_downscaled_f64(ctx, grid, &spec, cls.as<uint8_t>(), drivers, scalar.as<double>(), et.as<double>(), nullptr,
                                             nullptr, nullptr, n, 0, MOD16_HOST, nullptr, 0) == MOD16_OK);
    check_written(et, 1, n, n, sizeof(double), true, "out_et after it");
    EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
    printf("host_asan_composite_downscale: no room done\n");
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    mod16_ctx* bare = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    EXPECT(mod16_create(0, &bare) == MOD16_OK && bare);
    double lut[MOD16_N_CLASSES * MOD16_N_PARAMS];
    for (int i = 0; i < MOD16_N_CLASSES * MOD16_N_PARAMS; ++i) lut[i] = 1.0 + i;
    EXPECT(mod16_set_bplut_f64(ctx, lut) == MOD16_OK);
    no_room(ctx);
    run<double>(ctx, bare, mod16_et_composite_downscaled_f64, "float64");
    run<float>(ctx, bare, mod16_et_composite_downscaled_f32, "float32");
    EXPECT(mod16_destroy(bare) == MOD16_OK);
    harness_finish(ctx);
    return 0;
}
