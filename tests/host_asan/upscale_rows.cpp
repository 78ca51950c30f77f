// Stand-alone driver of tests/test_upscale_rows_host_asan.py: mod16_upscale_create_rows and the HOST mode of
// mod16_upscale_f32 / _f64 / _classes / _sums_f32 / _sums_f64 on a rows handle (row-affine columns) -- the
// library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP
// stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check; the
// upscale kernels have no shadow there). Every host array sits between guard bytes. Geometries: 37 fine rows
// over 5 coarse rows (runs of 7, 8, 7, 8, 7) increasing and decreasing, with a margin of rows outside and an
// empty coarse row, 70 columns over 9 cells at scales of both signs, with and without wrap_cols, with and
// without column ranges (an empty one among them) and area; K = 1 and 3 layers; three stage_bytes (one coarse
// row of one layer per pass, a band of two coarse rows, one band), dense arrays and arrays whose row and layer
// strides exceed the row and the plane, all outputs and a subset, both types. Pass: no sanitizer report,
// every requested output element overwritten, no guard byte and no element between the rows or the layers
// touched, nothing left allocated.
#include <cmath>

#define HARNESS_NAME "host_asan_upscale_rows"
#include "harness.hpp"

struct Axis {
    std::vector<int32_t> first, count;
    int64_t n;          // fine indices
};

// runs of the given lengths one after the other from `margin`; reversed: the last cell first
static Axis axis(std::vector<int32_t> lengths, int64_t margin, bool reversed) {
    Axis a;
    a.first.resize(lengths.size());
    a.count = lengths;
    int64_t at = margin;
    for (size_t k = 0; k < lengths.size(); ++k) {
        const size_t c = reversed ? lengths.size() - 1 - k : k;
        a.first[c] = lengths[c] ? (int32_t)at : 0;
        at += lengths[c];
    }
    a.n = at + margin;
    return a;
}

static void* ptr(Shaped* g) { return g ? static_cast<void*>(g->data()) : nullptr; }
static int64_t plane(Shaped* g) { return g ? g->plane : 0; }
static int64_t pitch(Shaped* g) { return g ? g->pitch : 0; }

template <typename T>
static int mean_call(mod16_ctx* ctx, const mod16_upscale* grid, const void* values, int32_t layers, int64_t ls, int64_t rs, double mf,
                     Shaped* mean, Shaped* fraction, Shaped* count, int where, size_t stage) {
    if (sizeof(T) == 4)
        return mod16_upscale_f32(ctx, grid, static_cast<const float*>(values), layers, ls, rs, mf, static_cast<float*>(ptr(mean)), plane(mean),
                                 pitch(mean), static_cast<float*>(ptr(fraction)), plane(fraction), pitch(fraction),
                                 static_cast<int32_t*>(ptr(count)), plane(count), pitch(count), where, nullptr, stage);
    return mod16_upscale_f64(ctx, grid, static_cast<const double*>(values), layers, ls, rs, mf, static_cast<double*>(ptr(mean)), plane(mean),
                             pitch(mean), static_cast<double*>(ptr(fraction)), plane(fraction), pitch(fraction),
                             static_cast<int32_t*>(ptr(count)), plane(count), pitch(count), where, nullptr, stage);
}

template <typename T>
static int sums_call(mod16_ctx* ctx, const mod16_upscale* grid, const void* values, int32_t layers, int64_t ls, int64_t rs, Shaped* num,
                     Shaped* den, Shaped* tot, Shaped* count, int where, size_t stage) {
    auto d = [](Shaped* g) { return static_cast<double*>(ptr(g)); };
    if (sizeof(T) == 4)
        return mod16_upscale_sums_f32(ctx, grid, static_cast<const float*>(values), layers, ls, rs, d(num), plane(num), pitch(num), d(den),
                                      plane(den), pitch(den), d(tot), plane(tot), pitch(tot), static_cast<int32_t*>(ptr(count)),
                                      plane(count), pitch(count), where, nullptr, stage);
    return mod16_upscale_sums_f64(ctx, grid, static_cast<const double*>(values), layers, ls, rs, d(num), plane(num), pitch(num), d(den),
                                  plane(den), pitch(den), d(tot), plane(tot), pitch(tot), static_cast<int32_t*>(ptr(count)),
                                  plane(count), pitch(count), where, nullptr, stage);
}

static void ok(mod16_ctx* ctx, int rc, const char* what) {
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_upscale_rows: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
        exit(1);
    }
}

template <typename T>
static void run(mod16_ctx* ctx, const char* what) {
    const std::vector<int32_t> row_lengths[] = {{7, 8, 7, 8, 7}, {7, 0, 8, 7}};
    for (int geom = 0; geom < 4; ++geom) {
        const Axis rows = axis(row_lengths[geom / 2], geom >= 2 ? 3 : 0, geom % 2 == 1);
        const int64_t R = rows.n, C = 70, H = (int64_t)rows.count.size(), W = 9;
        const bool wrap = geom % 2 == 1, ranges = geom != 0;
        std::vector<double> area((size_t)R, 0.5), origin((size_t)R), scale((size_t)R);
        std::vector<int32_t> col_first((size_t)R), col_count((size_t)R);
        for (int64_t r = 0; r < R; ++r) {
            scale[r] = (r % 3 == 2 ? -1.0 : 1.0) * (0.05 + 0.01 * (double)(r % 5));      // 0.05 ... 0.09: 69 columns stay below W - 2 = 7
            origin[r] = scale[r] < 0 ? 8.0 : -0.5 + 0.25 * (double)(r % 4);
            col_first[r] = (int32_t)(r % 7);
            col_count[r] = r == 4 ? 0 : (int32_t)(C - r % 7 - r % 3);
        }
        mod16_upscale_spec spec;
        memset(&spec, 0, sizeof spec);
        spec.rows = R; spec.cols = C; spec.coarse_rows = H; spec.coarse_cols = W; spec.wrap_cols = wrap;
        mod16_upscale* grid = nullptr;
        ok(ctx, mod16_upscale_create_rows(ctx, &spec, rows.first.data(), rows.count.data(), origin.data(), scale.data(),
                                          ranges ? col_first.data() : nullptr, ranges ? col_count.data() : nullptr,
                                          geom >= 2 ? area.data() : nullptr, &grid), "create_rows");
        EXPECT(grid);
        for (int32_t K : {1, 3})
            for (int pitched = 0; pitched < 2; ++pitched)
                for (int all = 0; all < 2; ++all) {
                    const int64_t rs = pitched ? C + 5 : C, ls = pitched ? R * rs + 9 : R * C;
                    const int64_t ors = pitched ? W + 3 : W, ols = pitched ? H * ors + 7 : H * W;
                    Shaped values(K, ls, R, rs, C, sizeof(T), 0);
                    // one layer of the tallest coarse row: its 8 fine rows and its row of the four outputs, each in whole 256-byte lines
                    const size_t coarse_row = 8 * (size_t)C * sizeof(T) + 4 * 256;
                    const size_t stages[] = {1, (size_t)K * 2 * coarse_row + 1536, 0};
                    for (size_t stage : stages) {
                        Shaped mean(K, ols, H, ors, W, sizeof(T), kFresh), fraction(K, ols, H, ors, W, sizeof(T), kFresh);
                        Shaped count(K, ols, H, ors, W, 4, kFresh);
                        ok(ctx, mean_call<T>(ctx, grid, values.data(), K, ls, rs, 0.5, &mean, all ? &fraction : nullptr, all ? &count : nullptr,
                                             MOD16_HOST, stage), what);
                        mean.check(true, "mean");
                        fraction.check(all != 0, "fraction");
                        count.check(all != 0, "count");
                        Shaped num(K, ols, H, ors, W, 8, kFresh), den(K, ols, H, ors, W, 8, kFresh), tot(K, ols, H, ors, W, 8, kFresh);
                        Shaped cnt(K, ols, H, ors, W, 4, kFresh);
                        ok(ctx, sums_call<T>(ctx, grid, values.data(), K, ls, rs, all ? &num : nullptr, &den, all ? &tot : nullptr,
                                             all ? &cnt : nullptr, MOD16_HOST, stage), "sums");
                        num.check(all != 0, "num");
                        den.check(true, "den");
                        tot.check(all != 0, "tot");
                        cnt.check(all != 0, "count of the sums");
                    }
                    EXPECT(values.guards_intact());
                }
        if (sizeof(T) == 4) {                              // the class raster once per geometry
            for (int pitched = 0; pitched < 2; ++pitched) {
                const int64_t rs = pitched ? C + 5 : C, ors = pitched ? W + 3 : W;
                Shaped cls(1, R * rs, R, rs, C, 1, 0);
                for (size_t stage : {(size_t)1, (size_t)(2 * (8 * C + 2 * 256) + 1024), (size_t)0}) {
                    Shaped out_cls(1, H * ors, H, ors, W, 1, kFresh), share(1, H * ors, H, ors, W, 4, kFresh);
                    ok(ctx, mod16_upscale_classes(ctx, grid, cls.as<uint8_t>(), rs, 0x1fffu,
                                                  out_cls.as<uint8_t>(), ors,
                                                  pitched ? nullptr : share.as<float>(), ors, MOD16_HOST, nullptr, stage),
                       "classes");
                    out_cls.check(true, "out_cls");
                    share.check(!pitched, "out_share");
                }
                EXPECT(cls.guards_intact());
            }
        }
        EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    }
    // the sums of a rectilinear handle go through the same band loop with four outputs
    {
        const Axis rows = axis({7, 8, 7}, 1, false), cols = axis({8, 8, 8, 8, 8, 8, 8, 8, 6}, 0, false);
        const int64_t R = rows.n, C = cols.n, H = 3, W = 9;
        mod16_upscale_spec spec;
        memset(&spec, 0, sizeof spec);
        spec.rows = R; spec.cols = C; spec.coarse_rows = H; spec.coarse_cols = W;
        mod16_upscale* grid = nullptr;
        ok(ctx, mod16_upscale_create(ctx, &spec, rows.first.data(), rows.count.data(), cols.first.data(), cols.count.data(), nullptr, &grid),
           "create");
        Shaped values(2, R * C, R, C, C, sizeof(T), 0);
        for (size_t stage : {(size_t)1, (size_t)0}) {
            Shaped num(2, H * W + 7, H, W + 3, W, 8, kFresh), den(2, H * W, H, W, W, 8, kFresh), cnt(2, H * W, H, W, W, 4, kFresh);
            ok(ctx, sums_call<T>(ctx, grid, values.data(), 2, R * C, C, &num, &den, nullptr, &cnt, MOD16_HOST, stage), "rectilinear sums");
            num.check(true, "num");
            den.check(true, "den");
            cnt.check(true, "count of the sums");
        }
        EXPECT(values.guards_intact());
        EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    }
    printf("host_asan_upscale_rows: %s done\n", what);
}

// refused before any device work
static void refusals(mod16_ctx* ctx) {
    const int64_t R = 4, C = 9, H = 2, W = 5;
    const std::vector<int32_t> rf = {0, 2}, rc = {2, 2};
    const std::vector<double> origin = {0.0, 0.5, 1.0, 4.0}, scale = {0.25, 0.25, -0.25, 0.125};
    const std::vector<int32_t> cf = {0, 1, 2, 3}, cc = {9, 8, 7, 0};
    mod16_upscale_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.rows = R; spec.cols = C; spec.coarse_rows = H; spec.coarse_cols = W; spec.wrap_cols = 1;
    mod16_upscale* grid = nullptr;
    auto create = [&](const mod16_upscale_spec& sp, const std::vector<int32_t>& f, const std::vector<int32_t>& n, const std::vector<double>& o,
                      const std::vector<double>& s, const std::vector<int32_t>& first, const std::vector<int32_t>& count, const double* area) {
        grid = reinterpret_cast<mod16_upscale*>(&spec);
        return mod16_upscale_create_rows(ctx, &sp, f.data(), n.data(), o.data(), s.data(), first.data(), count.data(), area, &grid);
    };
    auto refused = [&](int code, const char* prefix, const char* part) { return ::refused(ctx, code, prefix, part); };
    const char* const cr = "mod16_upscale_create_rows: ";
    grid = reinterpret_cast<mod16_upscale*>(&spec);
    EXPECT(refused(mod16_upscale_create_rows(ctx, nullptr, rf.data(), rc.data(), origin.data(), scale.data(), nullptr, nullptr, nullptr, &grid), cr, "NULL argument"));
    EXPECT(grid == nullptr);
    EXPECT(refused(mod16_upscale_create_rows(ctx, &spec, rf.data(), nullptr, origin.data(), scale.data(), nullptr, nullptr, nullptr, &grid), cr, "NULL argument"));
    EXPECT(refused(mod16_upscale_create_rows(ctx, &spec, rf.data(), rc.data(), nullptr, scale.data(), nullptr, nullptr, nullptr, &grid), cr, "NULL argument"));
    EXPECT(refused(mod16_upscale_create_rows(ctx, &spec, rf.data(), rc.data(), origin.data(), nullptr, nullptr, nullptr, nullptr, &grid), cr, "NULL argument"));
    EXPECT(refused(mod16_upscale_create_rows(ctx, &spec, rf.data(), rc.data(), origin.data(), scale.data(), nullptr, nullptr, nullptr, nullptr), cr, "NULL argument"));
    EXPECT(refused(mod16_upscale_create_rows(ctx, &spec, rf.data(), rc.data(), origin.data(), scale.data(), cf.data(), nullptr, nullptr, &grid), cr, "both be given or both be NULL"));
    EXPECT(refused(mod16_upscale_create_rows(ctx, &spec, rf.data(), rc.data(), origin.data(), scale.data(), nullptr, cc.data(), nullptr, &grid), cr, "both be given or both be NULL"));
    mod16_upscale_spec sp = spec;
    sp.rows = 0; EXPECT(refused(create(sp, rf, rc, origin, scale, cf, cc, nullptr), cr, "rows and cols must be"));
    sp = spec; sp.coarse_cols = (int64_t(1) << 30) + 1; EXPECT(refused(create(sp, rf, rc, origin, scale, cf, cc, nullptr), cr, "coarse_rows and coarse_cols must be"));
    sp = spec; sp.wrap_cols = 2; EXPECT(refused(create(sp, rf, rc, origin, scale, cf, cc, nullptr), cr, "wrap_cols"));
    EXPECT(refused(create(spec, rf, {2, 5}, origin, scale, cf, cc, nullptr), cr, "a count lies outside"));
    EXPECT(refused(create(spec, {0, 3}, rc, origin, scale, cf, cc, nullptr), cr, "a run leaves its axis"));
    EXPECT(refused(create(spec, {0, 1}, rc, origin, scale, cf, cc, nullptr), cr, "share a fine index"));
    {
        const double nan = std::nan(""), inf = (double)INFINITY;
        for (double v : {nan, inf, -inf}) {
            EXPECT(refused(create(spec, rf, rc, {0.0, v, 1.0, 4.0}, scale, cf, cc, nullptr), cr, "must be finite"));
            EXPECT(refused(create(spec, rf, rc, origin, {0.25, 0.25, v, 0.125}, cf, cc, nullptr), cr, "must be finite"));
        }
        EXPECT(refused(create(spec, rf, rc, {0.0, 1e308, 1.0, 4.0}, {0.25, 1e308, 0.25, 0.125}, cf, {9, 1, 7, 0}, nullptr), cr, "must be finite"));   // the far end
        for (double v : {0.0, -1.0, nan, inf}) {
            const double area[4] = {1.0, 1.0, v, 1.0};
            EXPECT(refused(create(spec, rf, rc, origin, scale, cf, cc, area), cr, "area must be positive and finite"));
        }
    }
    EXPECT(refused(create(spec, rf, rc, origin, scale, {0, -1, 2, 3}, cc, nullptr), cr, "a column range leaves its row"));
    EXPECT(refused(create(spec, rf, rc, origin, scale, cf, {9, 8, -1, 0}, nullptr), cr, "a column range leaves its row"));
    EXPECT(refused(create(spec, rf, rc, origin, scale, cf, {9, 9, 7, 0}, nullptr), cr, "a column range leaves its row"));
    EXPECT(refused(create(spec, rf, rc, origin, {0.25, 0.5, -0.25, 0.125}, cf, cc, nullptr), cr, "may lap the periodic axis"));      // 0.5 * 7 > 3
    sp = spec; sp.wrap_cols = 0;
    ok(ctx, create(sp, rf, rc, origin, {0.25, 0.5, -0.25, 0.125}, cf, cc, nullptr), "the same row without wrap_cols");
    EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    ok(ctx, create(spec, rf, rc, origin, {0.25, 400.0, -0.25, 0.125}, cf, {9, 1, 7, 0}, nullptr), "one column at any scale");
    EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    {   // 2^16 rows x 2^15 columns: 2^31 pixels
        mod16_upscale_spec big = spec;
        big.rows = 1 << 16; big.cols = 1 << 15; big.coarse_rows = big.coarse_cols = 1; big.wrap_cols = 0;
        const std::vector<double> zero((size_t)big.rows, 0.0);
        grid = reinterpret_cast<mod16_upscale*>(&spec);
        EXPECT(refused(mod16_upscale_create_rows(ctx, &big, std::vector<int32_t>{0}.data(), std::vector<int32_t>{1 << 16}.data(), zero.data(),
                                                 zero.data(), nullptr, nullptr, nullptr, &grid), cr, "fewer than 2^31 pixels"));
        EXPECT(grid == nullptr);
    }
    ok(ctx, create(spec, rf, rc, origin, scale, cf, cc, nullptr), "create_rows");
    EXPECT(grid && grid != reinterpret_cast<mod16_upscale*>(&spec));

    const int32_t K = 2;
    Shaped values(K, R * C, R, C, C, 8, 0), num(K, H * W, H, W, W, 8, kFresh), den(K, H * W, H, W, W, 8, kFresh), tot(K, H * W, H, W, W, 8, kFresh);
    Shaped count(K, H * W, H, W, W, 4, kFresh), mean(K, H * W, H, W, W, 8, kFresh);
    const char* const us = "mod16_upscale_sums: ";
    auto go = [&](const mod16_upscale* g, const void* v, int32_t layers, int64_t ls, int64_t rs, int where, size_t stage) {
        return sums_call<double>(ctx, g, v, layers, ls, rs, &num, &den, &tot, &count, where, stage);
    };
    EXPECT(refused(go(nullptr, values.data(), K, R * C, C, MOD16_HOST, 0), us, "NULL grid or values"));
    EXPECT(refused(go(grid, nullptr, K, R * C, C, MOD16_DEVICE, 0), us, "NULL grid or values"));
    EXPECT(refused(sums_call<double>(ctx, grid, values.data(), K, R * C, C, nullptr, nullptr, nullptr, nullptr, MOD16_HOST, 0), us, "no output is requested"));
    EXPECT(refused(go(grid, values.data(), 0, R * C, C, MOD16_HOST, 0), us, "layers must be between 1 and 65535"));
    EXPECT(refused(go(grid, values.data(), K, R * C, C - 1, MOD16_HOST, 0), us, "a row stride is below"));
    EXPECT(refused(go(grid, values.data(), K, R * C - 1, C, MOD16_DEVICE, 0), us, "a layer stride is below a plane"));
    EXPECT(refused(go(grid, values.data(), K, R * C, int64_t(1) << 60, MOD16_HOST, 0), us, "out of range"));
    EXPECT(refused(go(grid, values.data(), K, R * C, C, 7, 0), us, "`where` must be"));
    EXPECT(refused(go(grid, values.data(), K, R * C, C, MOD16_HOST, ~size_t(0)), us, "stage_bytes"));
    {
        Shaped narrow(K, H * W, H, W - 1, W - 1, 8, kFresh);
        EXPECT(refused(sums_call<double>(ctx, grid, values.data(), K, R * C, C, nullptr, nullptr, &narrow, nullptr, MOD16_HOST, 0), us, "a row stride is below"));
        narrow.check(false, "the narrow tot");
        EXPECT(refused(mod16_upscale_sums_f64(ctx, grid, values.as<double>(), K, R * C, C, values.as<double>() + 5,
                                              H * W, W, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, MOD16_HOST, nullptr, 0), us, "overlaps"));
        EXPECT(refused(mod16_upscale_sums_f64(ctx, grid, values.as<double>(), K, R * C, C, num.as<double>(), H * W, W,
                                              nullptr, 0, 0, num.as<double>() + K * H * W - 1, H * W, W, nullptr, 0, 0, MOD16_DEVICE,
                                              nullptr, 0), us, "overlaps"));
    }
    // the entry points of the mean and the classes refuse on a rows handle as on any other
    const char* const up = "mod16_upscale: ";
    EXPECT(refused(mean_call<double>(ctx, grid, values.data(), K, R * C, C, 1.5, &mean, nullptr, nullptr, MOD16_HOST, 0), up, "min_fraction"));
    EXPECT(refused(mean_call<double>(ctx, grid, values.data(), K, R * C, C, 0.0, nullptr, nullptr, nullptr, MOD16_HOST, 0), up, "no output is requested"));
    EXPECT(refused(mod16_upscale_f64(ctx, grid, values.as<double>(), K, R * C, C, 0.0, values.as<double>() + 5, H * W, W,
                                     nullptr, 0, 0, nullptr, 0, 0, MOD16_HOST, nullptr, 0), up, "overlaps"));
    const char* const uc = "mod16_upscale_classes: ";
    Shaped cls(1, R * C, R, C, C, 1, 0), out_cls(1, H * W, H, W, W, 1, kFresh);
    EXPECT(refused(mod16_upscale_classes(ctx, grid, cls.as<uint8_t>(), C - 1, 0x1fffu, out_cls.as<uint8_t>(), W,
                                         nullptr, 0, MOD16_HOST, nullptr, 0), uc, "a row stride is below"));
    EXPECT(refused(mod16_upscale_classes(ctx, grid, cls.as<uint8_t>(), C, 0x1fffu, cls.as<uint8_t>() + 3, W,
                                         nullptr, 0, MOD16_HOST, nullptr, 0), uc, "overlaps"));
    num.check(false, "num of the refused calls");
    den.check(false, "den of the refused calls");
    tot.check(false, "tot of the refused calls");
    count.check(false, "count of the refused calls");
    mean.check(false, "mean of the refused calls");
    out_cls.check(false, "out_cls of the refused calls");
    EXPECT(values.guards_intact() && cls.guards_intact());
    EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    printf("host_asan_upscale_rows: refusals done\n");
}

int main() {
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    run<float>(ctx, "float32");
    run<double>(ctx, "float64");
    refusals(ctx);
    harness_finish(ctx);
    return 0;
}
