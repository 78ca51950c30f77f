// Stand-alone driver of tests/test_downscale_host_asan.py: the HOST mode of mod16_et_downscaled_* and
// mod16_downscale_fields_*, and the host-side corner tables of mod16_downscale_create -- the library's
// own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP stand-in
// of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check; the
// downscale kernels have no shadow there). Every output sits between guard bytes; every input is a
// heap block of exactly its size, so that a read past its end is a sanitizer report. Pass: no
// report, every output element of the small calls overwritten, no guard byte touched, nothing left
// allocated.
//   small    1237 pixels from pixel 777 of a 60 x 47 raster (not row-aligned), one
//            tile, real memory: coarse planes with a row pitch of W + 3 whose last row ends with its W
//            elements, scalars, fine arrays
//   ragged   2 x 2^21 + 1237 pixels from pixel 777 of a 2100 x 2000 raster: three tiles, the last
//            ragged. A slot's slab is above the stand-in's 64 MiB, so its copies are range-checked on
//            the device side and skipped (hip_stub.hip): the outputs keep their fill
//   fields   3 fields over 3 000 001 pixels: the tile is cut so that a slab stays within 32 MiB -- real
//            memory, three tiles, the last ragged, a pitched output
#include <algorithm>
#include <cmath>

#define HARNESS_NAME "host_asan_downscale"
#include "harness.hpp"

constexpr int64_t H = 5, W = 7, kPitch = W + 3;

static mod16_downscale* make_grid(mod16_ctx* ctx, int64_t R, int64_t C, int method, int wrap) {
    mod16_downscale_spec spec = {R, C, H, W, wrap, method};
    std::vector<double> row_pos((size_t)R), col_pos((size_t)C);
    for (int64_t r = 0; r < R; ++r) row_pos[r] = -0.8 + (H + 0.6) * (double)r / (double)R;
    for (int64_t c = 0; c < C; ++c) col_pos[c] = -9.3 + (3.0 * W) * (double)c / (double)C;
    mod16_downscale* grid = nullptr;
    const int rc = mod16_downscale_create(ctx, &spec, row_pos.data(), col_pos.data(), &grid);
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_downscale: create: status %d: %s\n", rc, mod16_last_error(ctx));
        exit(1);
    }
    return grid;
}

template <typename T> struct Calls {
    int (*run)(mod16_ctx*, const mod16_downscale*, const uint8_t*, const T* const*, const int32_t*, int64_t, int64_t, int64_t,
               T*, T*, unsigned, int, void*);
    int (*fields)(mod16_ctx*, const mod16_downscale*, const T* const*, int, int64_t, int64_t, int64_t, T*, int64_t, int, void*);
};

template <typename T>
static void run_case(mod16_ctx* ctx, const Calls<T>& fn, int64_t R, int64_t C, int64_t first, int64_t n, bool written,
                     unsigned flags, const char* what) {
    mod16_downscale* grid = make_grid(ctx, R, C, MOD16_DOWNSCALE_COS4, 1);
    const size_t plane = (size_t)((H - 1) * kPitch + W);           // the last row ends with its W elements
    std::vector<std::vector<T>> in;
    const T* drivers[MOD16_N_DRIVERS];
    int32_t kinds[MOD16_N_DRIVERS];
    for (int k = 0; k < MOD16_N_DRIVERS; ++k) {
        const bool fine = k == MOD16_SW_ALBEDO || k == MOD16_FPAR || k == MOD16_LAI;
        kinds[k] = k == MOD16_SW_RAD_NIGHT ? 0 : fine ? 1 : 2;
        in.emplace_back(kinds[k] == 0 ? 1 : fine ? (size_t)n : plane, (T)1.5);
        in.back().shrink_to_fit();
        drivers[k] = in.back().data();
    }
    std::vector<uint8_t> cls((size_t)n, (uint8_t)1);
    Guarded day((size_t)n * sizeof(T)), night((size_t)n * sizeof(T));
    const int rc = fn.run(ctx, grid, cls.data(), drivers, kinds, kPitch, first, n, day.as<T>(), night.as<T>(), flags,
                          MOD16_HOST, nullptr);
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_downscale: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
        exit(1);
    }
    check_written(day, 1, n, n, sizeof(T), written, "out_day");
    check_written(night, 1, n, n, sizeof(T), written, "out_night");
    // refused before any device work (the outputs keep what they hold); n = 0 is fine
    Guarded keep(64 * sizeof(T));
    auto call = [&](const int32_t* kd, int64_t pitch, int64_t f, int64_t m, unsigned fl, int where) {
        return fn.run(ctx, grid, cls.data(), drivers, kd, pitch, f, m, keep.as<T>(), keep.as<T>(), fl, where, nullptr);
    };
    int32_t bad_kinds[MOD16_N_DRIVERS];
    memcpy(bad_kinds, kinds, sizeof kinds);
    bad_kinds[MOD16_LAI] = 3;
    EXPECT(call(bad_kinds, kPitch, first, 1, 0, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, W - 1, first, 1, 0, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, kPitch, -1, 1, 0, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, kPitch, R * C - 3, 4, 0, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, kPitch, first, -1, 0, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, kPitch, first, 1, MOD16_MATH_MIXED, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, kPitch, first, 1, MOD16_DOMAIN_TRUSTED, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(kinds, kPitch, first, 1, 0, 7) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "mod16_et_downscaled") != nullptr);
    EXPECT(call(kinds, kPitch, R * C, 0, 0, MOD16_HOST) == MOD16_OK);
    check_written(keep, 1, 64, 64, sizeof(T), false, "outputs of the refused calls");
    EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
    printf("host_asan_downscale: %s done\n", what);
}

template <typename T>
static void fields_case(mod16_ctx* ctx, const Calls<T>& fn, const char* what) {
    const int64_t R = 1733, C = 1741, first = 777, n = 3000001, pitch = n + 19;
    const int F = 3;
    mod16_downscale* grid = make_grid(ctx, R, C, MOD16_DOWNSCALE_BILINEAR, 0);
    const size_t plane = (size_t)((H - 1) * kPitch + W);
    std::vector<std::vector<T>> in;
    const T* fields[F];
    for (int f = 0; f < F; ++f) {
        in.emplace_back(plane, (T)280);
        in.back().shrink_to_fit();
        fields[f] = in.back().data();
    }
    Guarded out(((size_t)(F - 1) * pitch + n) * sizeof(T));
    const int rc = fn.fields(ctx, grid, fields, F, kPitch, first, n, out.as<T>(), pitch, MOD16_HOST, nullptr);
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_downscale: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
        exit(1);
    }
    check_written(out, F, pitch, n, sizeof(T), true, "fields");
    Guarded keep(64 * sizeof(T));
    EXPECT(fn.fields(ctx, grid, fields, 0, kPitch, first, 8, keep.as<T>(), 8, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.fields(ctx, grid, fields, 17, kPitch, first, 8, keep.as<T>(), 8, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.fields(ctx, grid, fields, F, W - 1, first, 8, keep.as<T>(), 8, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.fields(ctx, grid, fields, F, kPitch, first, 8, keep.as<T>(), 7, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.fields(ctx, grid, fields, F, kPitch, R * C - 7, 8, keep.as<T>(), 8, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.fields(ctx, grid, fields, F, kPitch, first, 0, keep.as<T>(), 0, MOD16_HOST, nullptr) == MOD16_OK);
    check_written(keep, 1, 64, 64, sizeof(T), false, "output of the refused calls");
    EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
    printf("host_asan_downscale: %s done\n", what);
}

static void create_errors(mod16_ctx* ctx) {
    mod16_downscale* grid = nullptr;
    std::vector<double> rows(9, 0.5), cols(11, 0.5);
    mod16_downscale_spec spec = {9, 11, H, W, 0, MOD16_DOWNSCALE_BILINEAR};
    mod16_downscale_spec s = spec;
    s.rows = 0; EXPECT(mod16_downscale_create(ctx, &s, rows.data(), cols.data(), &grid) == MOD16_ERR_ARG && !grid);
    s = spec; s.coarse_cols = ((int64_t)1 << 30) + 1; EXPECT(mod16_downscale_create(ctx, &s, rows.data(), cols.data(), &grid) == MOD16_ERR_ARG);
    s = spec; s.method = 3; EXPECT(mod16_downscale_create(ctx, &s, rows.data(), cols.data(), &grid) == MOD16_ERR_ARG);
    s = spec; s.wrap_cols = 2; EXPECT(mod16_downscale_create(ctx, &s, rows.data(), cols.data(), &grid) == MOD16_ERR_ARG);
    EXPECT(mod16_downscale_create(ctx, &spec, nullptr, cols.data(), &grid) == MOD16_ERR_ARG);
    rows[4] = NAN;
    EXPECT(mod16_downscale_create(ctx, &spec, rows.data(), cols.data(), &grid) == MOD16_ERR_ARG && !grid);
    rows[4] = 1e300;              // far outside: held at the last row; wrapped: some cell of the axis
    cols[3] = -1e300;
    for (int wrap = 0; wrap < 2; ++wrap)
        for (int method = 0; method < 3; ++method) {
            s = spec; s.wrap_cols = wrap; s.method = method;
            EXPECT(mod16_downscale_create(ctx, &s, rows.data(), cols.data(), &grid) == MOD16_OK && grid);
            EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
        }
    // tables the caller computed: an index outside the coarse grid is refused
    std::vector<int32_t> ri0(9, 0), ri1(9, 1), ci0(11, 0), ci1(11, 1);
    std::vector<double> rw0(9, 0.5), rw1(9, 0.5), cw0(11, 0.5), cw1(11, 0.5);
    EXPECT(mod16_downscale_create_tables(ctx, &spec, ri0.data(), ri1.data(), rw0.data(), rw1.data(), ci0.data(), ci1.data(),
                                         cw0.data(), cw1.data(), &grid) == MOD16_OK && grid);
    EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
    ci1[10] = (int32_t)W;
    EXPECT(mod16_downscale_create_tables(ctx, &spec, ri0.data(), ri1.data(), rw0.data(), rw1.data(), ci0.data(), ci1.data(),
                                         cw0.data(), cw1.data(), &grid) == MOD16_ERR_ARG && !grid);
    ci1[10] = 1; ri0[0] = -1;
    EXPECT(mod16_downscale_create_tables(ctx, &spec, ri0.data(), ri1.data(), rw0.data(), rw1.data(), ci0.data(), ci1.data(),
                                         cw0.data(), cw1.data(), &grid) == MOD16_ERR_ARG && !grid);
    ri0[0] = 0; rw1[2] = INFINITY;
    EXPECT(mod16_downscale_create_tables(ctx, &spec, ri0.data(), ri1.data(), rw0.data(), rw1.data(), ci0.data(), ci1.data(),
                                         cw0.data(), cw1.data(), &grid) == MOD16_ERR_ARG && !grid);
    printf("host_asan_downscale: create done\n");
}

// (the context's slabs only grow: the case whose slab is address space without memory comes last,
// and each data type has a context of its own)
template <typename T> static void all_cases(const Calls<T>& fn, const char* name, bool first) {
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    double lut[MOD16_N_CLASSES * MOD16_N_PARAMS];
    for (int i = 0; i < MOD16_N_CLASSES * MOD16_N_PARAMS; ++i) lut[i] = 1.0 + i;
    EXPECT(mod16_set_bplut_f64(ctx, lut) == MOD16_OK);
    if (first) create_errors(ctx);
    char what[64];
    snprintf(what, sizeof what, "%s small", name);
    run_case<T>(ctx, fn, 60, 47, 777, 1237, true, MOD16_MATH_FAST, what);
    snprintf(what, sizeof what, "%s fields", name);
    fields_case<T>(ctx, fn, what);
    snprintf(what, sizeof what, "%s ragged", name);
    run_case<T>(ctx, fn, 2100, 2000, 777, 2 * ((int64_t)1 << 21) + 1237, false, MOD16_MATH_EXACT, what);
    EXPECT(mod16_destroy(ctx) == MOD16_OK);
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    all_cases<double>(Calls<double>{mod16_et_downscaled_f64, mod16_downscale_fields_f64}, "float64", true);
    all_cases<float>(Calls<float>{mod16_et_downscaled_f32, mod16_downscale_fields_f32}, "float32", false);
    harness_finish(nullptr);
    return 0;
}
