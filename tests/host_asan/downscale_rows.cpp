// Stand-alone driver of tests/test_downscale_rows_host_asan.py: the row-affine column geometry of the
// downscaled families (mod16_downscale_create_rows, mod16_downscale_create_rows_tables) and the HOST
// mode of mod16_et_downscaled_*, mod16_downscale_fields_* and mod16_et_composite_downscaled_* on such
// a handle -- the library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked
// against the HIP stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch =
// its shape check; the downscale kernels have no shadow there, the stand-in records their names).
// col_origin and col_scale are heap blocks of exactly rows x 8 bytes, so that a read past their end
// is a sanitizer report; every output sits between guard bytes. All ranges start inside a row (pixel
// 777 of a 60 x 47 raster) and end ragged (1237 pixels). Pass: no report, every output element
// overwritten, no guard byte and no padding touched, every refusal before an output is touched,
// nothing left allocated.
#include <cmath>

#define HARNESS_NAME "host_asan_downscale_rows"
#include "harness.hpp"

constexpr int64_t R = 60, C = 47, H = 5, W = 7, kPitch = W + 3;
constexpr int64_t kSpan = (H - 1) * kPitch + W, kTime = kSpan + 5;      // a plane, and the distance between two
constexpr int64_t kFirst = 777, kN = 1237;

// a heap block of exactly `count` elements
template <typename T> struct Exact {
    T* p;
    explicit Exact(size_t count, T v) : p(static_cast<T*>(malloc(count * sizeof(T)))) {
        EXPECT(p);
        for (size_t i = 0; i < count; ++i) p[i] = v;
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

// the geometry of a sinusoidal-like raster: the scale grows towards both ends of the rows, one row
// stands still, one runs east to west
struct Geometry {
    Exact<double> row_pos, origin, scale;
    Geometry() : row_pos(R, 0.0), origin(R, 0.0), scale(R, 0.0) {
        for (int64_t r = 0; r < R; ++r) {
            row_pos.p[r] = -0.8 + (H + 0.6) * (double)r / (double)R;
            const double lat = (70.0 - 140.0 * (double)r / (double)(R - 1)) * 3.141592653589793 / 180.0;
            scale.p[r] = r == 5 ? 0.0 : (r == 6 ? -0.41 : 0.41) / std::cos(lat);
            origin.p[r] = 3.0 - scale.p[r] * 23;
        }
    }
};

static mod16_downscale* make_grid(mod16_ctx* ctx, const Geometry& g, int method, int wrap, bool own_tables) {
    mod16_downscale_spec spec = {R, C, H, W, wrap, method};
    mod16_downscale* grid = nullptr;
    int rc;
    if (own_tables) {
        Exact<int32_t> i0(R, 0), i1(R, 0);
        Exact<double> w0(R, 1.0), w1(R, 0.0);
        for (int64_t r = 0; r < R; ++r) {
            i0.p[r] = (int32_t)(r % H);
            i1.p[r] = (int32_t)((r + 1) % H);
            w0.p[r] = 0.25;
            w1.p[r] = 0.75;
        }
        rc = mod16_downscale_create_rows_tables(ctx, &spec, i0.p, i1.p, w0.p, w1.p, g.origin.p, g.scale.p, &grid);
    } else {
        rc = mod16_downscale_create_rows(ctx, &spec, g.row_pos.p, g.origin.p, g.scale.p, &grid);
    }
    if (rc != MOD16_OK || !grid) {
        fprintf(stderr, "host_asan_downscale_rows: create: status %d: %s\n", rc, mod16_last_error(ctx));
        exit(1);
    }
    return grid;
}

static void create_errors(mod16_ctx* ctx, const Geometry& g) {
    mod16_downscale* grid = nullptr;
    mod16_downscale_spec spec = {R, C, H, W, 1, MOD16_DOWNSCALE_BILINEAR};
    Exact<int32_t> i0(R, 0), i1(R, 1);
    Exact<double> w0(R, 0.5), w1(R, 0.5);
    auto rows = [&](const mod16_downscale_spec& s, const double* rp, const double* o, const double* sc) {
        grid = reinterpret_cast<mod16_downscale*>(&spec);      // must come back NULL
        const int rc = mod16_downscale_create_rows(ctx, &s, rp, o, sc, &grid);
        EXPECT(rc == MOD16_OK || !grid);
        return rc;
    };
    auto tables = [&](const mod16_downscale_spec& s, const int32_t* a, const double* w, const double* o, const double* sc) {
        grid = reinterpret_cast<mod16_downscale*>(&spec);
        const int rc = mod16_downscale_create_rows_tables(ctx, &s, a, i1.p, w, w1.p, o, sc, &grid);
        EXPECT(rc == MOD16_OK || !grid);
        return rc;
    };
#define REFUSED(call, text) EXPECT(refused(ctx, (call), "mod16_downscale_create: ", text))
    mod16_downscale_spec s = spec;
    // the spec, cos4 among it
    s.method = MOD16_DOWNSCALE_COS4;
    REFUSED(rows(s, g.row_pos.p, g.origin.p, g.scale.p), "MOD16_DOWNSCALE_COS4 is not available");
    REFUSED(tables(s, i0.p, w0.p, g.origin.p, g.scale.p), "MOD16_DOWNSCALE_COS4 is not available");
    s = spec; s.method = 3;
    REFUSED(rows(s, g.row_pos.p, g.origin.p, g.scale.p), "unknown method");
    s = spec; s.rows = 0;
    REFUSED(rows(s, g.row_pos.p, g.origin.p, g.scale.p), "rows and cols");
    s = spec; s.wrap_cols = 2;
    REFUSED(tables(s, i0.p, w0.p, g.origin.p, g.scale.p), "wrap_cols");
    // NULLs
    REFUSED(rows(spec, nullptr, g.origin.p, g.scale.p), "NULL argument");
    REFUSED(rows(spec, g.row_pos.p, nullptr, g.scale.p), "NULL argument");
    REFUSED(rows(spec, g.row_pos.p, g.origin.p, nullptr), "NULL argument");
    REFUSED(tables(spec, nullptr, w0.p, g.origin.p, g.scale.p), "NULL argument");
    REFUSED(tables(spec, i0.p, nullptr, g.origin.p, g.scale.p), "NULL argument");
    REFUSED(tables(spec, i0.p, w0.p, nullptr, g.scale.p), "NULL argument");
    REFUSED(tables(spec, i0.p, w0.p, g.origin.p, nullptr), "NULL argument");
    EXPECT(mod16_downscale_create_rows(ctx, &spec, g.row_pos.p, g.origin.p, g.scale.p, nullptr) == MOD16_ERR_ARG);
    EXPECT(mod16_downscale_create_rows(ctx, nullptr, g.row_pos.p, g.origin.p, g.scale.p, &grid) == MOD16_ERR_ARG && !grid);
    EXPECT(mod16_downscale_create_rows(nullptr, &spec, g.row_pos.p, g.origin.p, g.scale.p, &grid) == MOD16_ERR_ARG);
    EXPECT(mod16_downscale_create_rows_tables(nullptr, &spec, i0.p, i1.p, w0.p, w1.p, g.origin.p, g.scale.p, &grid) == MOD16_ERR_ARG);
    // the geometry: the last row's entry is looked at too
    {
        Exact<double> o(R, 1.0), sc(R, 0.5), rp(R, 0.5);
        o.p[R - 1] = NAN;
        REFUSED(rows(spec, g.row_pos.p, o.p, g.scale.p), "col_origin holds a value that is not finite");
        REFUSED(tables(spec, i0.p, w0.p, o.p, g.scale.p), "col_origin holds a value that is not finite");
        o.p[R - 1] = -INFINITY;
        REFUSED(rows(spec, g.row_pos.p, o.p, g.scale.p), "col_origin holds a value that is not finite");
        sc.p[R - 1] = INFINITY;
        REFUSED(rows(spec, g.row_pos.p, g.origin.p, sc.p), "col_scale holds a value that is not finite");
        sc.p[R - 1] = NAN;
        REFUSED(tables(spec, i0.p, w0.p, g.origin.p, sc.p), "col_scale holds a value that is not finite");
        sc.p[R - 1] = 1e307;                 // finite, and 46 of them are not
        REFUSED(rows(spec, g.row_pos.p, g.origin.p, sc.p), "col_origin + col_scale * (cols - 1) is not finite");
        REFUSED(tables(spec, i0.p, w0.p, g.origin.p, sc.p), "col_origin + col_scale * (cols - 1) is not finite");
        sc.p[R - 1] = 1e300;                 // huge and finite: accepted, clamped or wrapped on the device
        o.p[R - 1] = -1e300;
        EXPECT(rows(spec, g.row_pos.p, o.p, sc.p) == MOD16_OK && grid);
        EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
        rp.p[3] = NAN;
        REFUSED(rows(spec, rp.p, g.origin.p, g.scale.p), "row_pos holds a value that is not finite");
    }
    // the row tables
    i0.p[R - 1] = (int32_t)H;
    REFUSED(tables(spec, i0.p, w0.p, g.origin.p, g.scale.p), "a row table holds an index outside the coarse grid");
    i0.p[R - 1] = 0;
    w0.p[0] = NAN;
    REFUSED(tables(spec, i0.p, w0.p, g.origin.p, g.scale.p), "a row table holds");
    w0.p[0] = 0.5;
    EXPECT(tables(spec, i0.p, w0.p, g.origin.p, g.scale.p) == MOD16_OK && grid);
    EXPECT(mod16_downscale_destroy(grid) == MOD16_OK);
#undef REFUSED
    printf("host_asan_downscale_rows: create done\n");
}

template <typename T> struct Calls {
    int (*run)(mod16_ctx*, const mod16_downscale*, const uint8_t*, const T* const*, const int32_t*, int64_t, int64_t, int64_t,
               T*, T*, unsigned, int, void*);
    int (*fields)(mod16_ctx*, const mod16_downscale*, const T* const*, int, int64_t, int64_t, int64_t, T*, int64_t, int, void*);
    int (*composite)(mod16_ctx*, const mod16_downscale*, const mod16_composite_downscaled_spec*, const uint8_t*,
                     const T* const*, const T*, T*, T*, uint16_t*, uint16_t*, int64_t, unsigned, int, void*, int64_t);
};

template <typename T>
static void run_case(mod16_ctx* ctx, const Calls<T>& fn, mod16_downscale* grid, unsigned flags) {
    std::vector<Exact<T>*> in;
    const T* drivers[MOD16_N_DRIVERS];
    int32_t kinds[MOD16_N_DRIVERS];
    for (int k = 0; k < MOD16_N_DRIVERS; ++k) {
        const bool fine = k == MOD16_SW_ALBEDO || k == MOD16_FPAR || k == MOD16_LAI;
        kinds[k] = k == MOD16_SW_RAD_NIGHT ? 0 : fine ? 1 : 2;
        in.push_back(new Exact<T>(kinds[k] == 0 ? 1 : fine ? (size_t)kN : (size_t)kSpan, (T)1.5));
        drivers[k] = in.back()->p;
    }
    Exact<uint8_t> cls((size_t)kN, (uint8_t)1);
    Guarded day((size_t)kN * sizeof(T)), night((size_t)kN * sizeof(T));
    const int rc = fn.run(ctx, grid, cls.p, drivers, kinds, kPitch, kFirst, kN, day.as<T>(), night.as<T>(), flags, MOD16_HOST, nullptr);
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_downscale_rows: run: status %d: %s\n", rc, mod16_last_error(ctx));
        exit(1);
    }
    check_written(day, 1, kN, kN, sizeof(T), true, "out_day");
    check_written(night, 1, kN, kN, sizeof(T), true, "out_night");
    Guarded keep(64 * sizeof(T));
    EXPECT(fn.run(ctx, grid, cls.p, drivers, kinds, kPitch, R * C - 3, 4, keep.as<T>(), keep.as<T>(), flags, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.run(ctx, grid, cls.p, drivers, kinds, W - 1, kFirst, 1, keep.as<T>(), keep.as<T>(), flags, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.run(ctx, grid, cls.p, drivers, kinds, kPitch, R * C, 0, keep.as<T>(), keep.as<T>(), flags, MOD16_HOST, nullptr) == MOD16_OK);
    check_written(keep, 1, 64, 64, sizeof(T), false, "outputs of the refused calls");
    for (auto* e : in) delete e;
}

template <typename T>
static void fields_case(mod16_ctx* ctx, const Calls<T>& fn, mod16_downscale* grid) {
    const int F = 3;
    const int64_t pitch = kN + 19;
    std::vector<Exact<T>*> in;
    const T* fields[F];
    for (int f = 0; f < F; ++f) {
        in.push_back(new Exact<T>((size_t)kSpan, (T)280));
        fields[f] = in.back()->p;
    }
    Guarded out(((size_t)(F - 1) * pitch + kN) * sizeof(T));
    const int rc = fn.fields(ctx, grid, fields, F, kPitch, kFirst, kN, out.as<T>(), pitch, MOD16_HOST, nullptr);
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_downscale_rows: fields: status %d: %s\n", rc, mod16_last_error(ctx));
        exit(1);
    }
    check_written(out, F, pitch, kN, sizeof(T), true, "fields");
    Guarded keep(64 * sizeof(T));
    EXPECT(fn.fields(ctx, grid, fields, F, kPitch, R * C - 7, 8, keep.as<T>(), 8, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    EXPECT(fn.fields(ctx, grid, fields, F, kPitch, kFirst, 8, keep.as<T>(), 7, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    check_written(keep, 1, 64, 64, sizeof(T), false, "output of the refused calls");
    for (auto* e : in) delete e;
}

template <typename T>
static void composite_case(mod16_ctx* ctx, const Calls<T>& fn, mod16_downscale* grid, bool all, unsigned flags) {
    const int64_t pitch = kN + 19;
    const int K = 11, L = 4, P = 3;                   // periods of 4, 4 and 3 days
    mod16_composite_downscaled_spec spec;
    memset(&spec, 0, sizeof spec);
    mod16_composite_spec& cs = spec.composite;
    cs.n = kN;
    cs.days = K;
    cs.period_days = L;
    cs.min_valid = 2;
    cs.rescale = 1;
    spec.coarse_pitch = kPitch;
    spec.first_pixel = kFirst;
    std::vector<Exact<T>*> in;
    const T* drivers[MOD16_N_DRIVERS];
    for (int k = 0; k < MOD16_N_DRIVERS; ++k) {
        if (k == MOD16_SW_ALBEDO || k == MOD16_FPAR || k == MOD16_LAI) {     // fine, 4-day slabs, pitched
            cs.pixel_stride[k] = 1; cs.time_stride[k] = pitch; cs.every[k] = 4;
            in.push_back(new Exact<T>((size_t)2 * pitch + kN, (T)1.5));
        } else if (k == MOD16_SW_RAD_NIGHT) {                                // a broadcast scalar
            cs.pixel_stride[k] = 0; cs.time_stride[k] = 0; cs.every[k] = K;
            in.push_back(new Exact<T>(1, (T)0));
        } else {                                                             // coarse
            spec.coarse_mask |= 1u << k;
            const int slabs = k == MOD16_TEMP_ANNUAL ? 1 : k == MOD16_PRESSURE ? 2 : K;
            cs.every[k] = k == MOD16_TEMP_ANNUAL ? 4096 : k == MOD16_PRESSURE ? 6 : 1;
            cs.time_stride[k] = slabs > 1 ? kTime : 0;
            in.push_back(new Exact<T>((size_t)((slabs - 1) * kTime + kSpan), (T)1.5));
        }
        drivers[k] = in.back()->p;
    }
    spec.coarse_mask |= 1u << 14;                                            // the hours: coarse, daily
    cs.hours_pixel_stride = 0; cs.hours_time_stride = kTime; cs.hours_every = 1;
    Exact<T> hours((size_t)((K - 1) * kTime + kSpan), (T)12);
    Exact<uint8_t> cls((size_t)kN, (uint8_t)1);
    const size_t count = (size_t)(P - 1) * pitch + kN;
    Guarded et(count * sizeof(T)), pet(count * sizeof(T)), cet(count * 2), cpet(count * 2);
    // a stage size that cuts the range into tiles of 512 pixels (the last ragged), then the default
    const int64_t stages[] = {(int64_t)19 * 33 * 1024 + 512 + 600 * (33 * (int64_t)sizeof(T) + 1), 0};
    for (int64_t stage : stages) {
        const int rc = fn.composite(ctx, grid, &spec, cls.p, drivers, hours.p, et.as<T>(), all ? pet.as<T>() : nullptr,
                                    all ? cet.as<uint16_t>() : nullptr, all ? cpet.as<uint16_t>() : nullptr, pitch, flags,
                                    MOD16_HOST, nullptr, stage);
        if (rc != MOD16_OK) {
            fprintf(stderr, "host_asan_downscale_rows: composite: status %d: %s\n", rc, mod16_last_error(ctx));
            exit(1);
        }
        check_written(et, P, pitch, kN, sizeof(T), true, "out_et");
        check_written(pet, P, pitch, kN, sizeof(T), all, "out_pet");
        check_written(cet, P, pitch, kN, 2, all, "count_et");
        check_written(cpet, P, pitch, kN, 2, all, "count_pet");
    }
    Guarded keep(64 * sizeof(T));
    mod16_composite_downscaled_spec s = spec;
    s.first_pixel = R * C - kN + 1;
    EXPECT(fn.composite(ctx, grid, &s, cls.p, drivers, hours.p, keep.as<T>(), nullptr, nullptr, nullptr, pitch, flags, MOD16_HOST,
                        nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "leaves the raster") != nullptr);
    check_written(keep, 1, 64, 64, sizeof(T), false, "output of the refused call");
    for (auto* e : in) delete e;
}

template <typename T> static void all_cases(const Calls<T>& fn, const char* name, bool first) {
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    double lut[MOD16_N_CLASSES * MOD16_N_PARAMS];
    for (int i = 0; i < MOD16_N_CLASSES * MOD16_N_PARAMS; ++i) lut[i] = 1.0 + i;
    EXPECT(mod16_set_bplut_f64(ctx, lut) == MOD16_OK);
    Geometry g;
    if (first) create_errors(ctx, g);
    // both create functions, both methods, both wrap values
    mod16_downscale* a = make_grid(ctx, g, MOD16_DOWNSCALE_BILINEAR, 1, false);
    mod16_downscale* b = make_grid(ctx, g, MOD16_DOWNSCALE_NEAREST, 0, true);
    run_case<T>(ctx, fn, a, MOD16_MATH_FAST);
    run_case<T>(ctx, fn, b, MOD16_MATH_EXACT);
    printf("host_asan_downscale_rows: %s run done\n", name);
    fields_case<T>(ctx, fn, a);
    fields_case<T>(ctx, fn, b);
    printf("host_asan_downscale_rows: %s fields done\n", name);
    composite_case<T>(ctx, fn, a, false, MOD16_MATH_FAST);
    composite_case<T>(ctx, fn, a, true, MOD16_MATH_FAST);
    composite_case<T>(ctx, fn, b, false, MOD16_MATH_EXACT);
    composite_case<T>(ctx, fn, b, true, MOD16_MATH_EXACT);
    printf("host_asan_downscale_rows: %s composite done\n", name);
    EXPECT(mod16_downscale_destroy(a) == MOD16_OK);
    EXPECT(mod16_downscale_destroy(b) == MOD16_OK);
    EXPECT(mod16_destroy(ctx) == MOD16_OK);
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    all_cases<double>(Calls<double>{mod16_et_downscaled_f64, mod16_downscale_fields_f64, mod16_et_composite_downscaled_f64}, "float64", true);
    all_cases<float>(Calls<float>{mod16_et_downscaled_f32, mod16_downscale_fields_f32, mod16_et_composite_downscaled_f32}, "float32", false);
    harness_finish(nullptr);
    return 0;
}
