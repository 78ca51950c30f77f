// Stand-alone driver of tests/test_upscale_host_asan.py: mod16_upscale_create / _destroy and the HOST mode of
// mod16_upscale_f32 / _f64 / _classes -- the library's own host code under AddressSanitizer +
// UndefinedBehaviorSanitizer, linked against the HIP stand-in of tests/host_asan (device memory = host heap
// filled with 0xA5, a launch = its shape check; the upscale kernels have no shadow there). Every host array
// sits between guard bytes. Geometries: 37 fine rows over 5 coarse rows (runs of 7, 8, 7, 8, 7) increasing
// and decreasing, with a margin of rows outside and an empty coarse row, 70 columns over 9 cells with the
// cell that straddles the end of the axis; K = 1 and 3 layers; three stage_bytes (one coarse row of one
// layer per pass, a band of two coarse rows, one band), dense arrays and arrays whose row and layer strides
// exceed the row and the plane, all outputs and a subset, both types, with and without area. Pass: no
// sanitizer report, every requested output element overwritten, no guard byte and no element between the
// rows or the layers touched, nothing left allocated.
#include <cmath>

#define HARNESS_NAME "host_asan_upscale"
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

template <typename T>
static int call(mod16_ctx* ctx, const mod16_upscale* grid, const void* values, int32_t layers, int64_t ls, int64_t rs, double mf,
                Shaped* mean, Shaped* fraction, Shaped* count, int where, size_t stage) {
    auto p = [](Shaped* g) { return g ? g->data() : nullptr; };
    auto l = [](Shaped* g) { return g ? g->plane : 0; };
    auto r = [](Shaped* g) { return g ? g->pitch : 0; };
    if (sizeof(T) == 4)
        return mod16_upscale_f32(ctx, grid, static_cast<const float*>(values), layers, ls, rs, mf, reinterpret_cast<float*>(p(mean)), l(mean),
                                 r(mean), reinterpret_cast<float*>(p(fraction)), l(fraction), r(fraction),
                                 reinterpret_cast<int32_t*>(p(count)), l(count), r(count), where, nullptr, stage);
    return mod16_upscale_f64(ctx, grid, static_cast<const double*>(values), layers, ls, rs, mf, reinterpret_cast<double*>(p(mean)), l(mean),
                             r(mean), reinterpret_cast<double*>(p(fraction)), l(fraction), r(fraction),
                             reinterpret_cast<int32_t*>(p(count)), l(count), r(count), where, nullptr, stage);
}

static void ok(mod16_ctx* ctx, int rc, const char* what) {
    if (rc != MOD16_OK) {
        fprintf(stderr, "host_asan_upscale: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
        exit(1);
    }
}

template <typename T>
static void run(mod16_ctx* ctx, const char* what) {
    const std::vector<int32_t> row_lengths[] = {{7, 8, 7, 8, 7}, {7, 0, 8, 7}};
    for (int geom = 0; geom < 4; ++geom) {
        const Axis rows = axis(row_lengths[geom / 2], geom >= 2 ? 3 : 0, geom % 2 == 1);
        Axis cols = axis({8, 8, 8, 8, 8, 8, 8, 8, 6}, 0, false);
        if (geom % 2) {                                    // the columns rolled by 3: cell 0 is 67, 68, 69, 0 ... 4
            for (auto& f : cols.first) f = (int32_t)((f + cols.n - 3) % cols.n);
        }
        const int64_t R = rows.n, C = cols.n, H = (int64_t)rows.count.size(), W = (int64_t)cols.count.size();
        std::vector<double> area((size_t)R, 0.5);
        mod16_upscale_spec spec;
        memset(&spec, 0, sizeof spec);
        spec.rows = R; spec.cols = C; spec.coarse_rows = H; spec.coarse_cols = W; spec.wrap_cols = geom % 2;
        mod16_upscale* grid = nullptr;
        ok(ctx, mod16_upscale_create(ctx, &spec, rows.first.data(), rows.count.data(), cols.first.data(), cols.count.data(),
                                     geom >= 2 ? area.data() : nullptr, &grid), "create");
        EXPECT(grid);
        for (int32_t K : {1, 3})
            for (int pitched = 0; pitched < 2; ++pitched)
                for (int all = 0; all < 2; ++all) {
                    const int64_t rs = pitched ? C + 5 : C, ls = pitched ? R * rs + 9 : R * C;
                    const int64_t ors = pitched ? W + 3 : W, ols = pitched ? H * ors + 7 : H * W;
                    Shaped values(K, ls, R, rs, C, sizeof(T), 0);
                    // one layer of the tallest coarse row: its 8 fine rows and its row of the three outputs, each in whole 256-byte lines
                    const size_t coarse_row = 8 * (size_t)C * sizeof(T) + 3 * 256;
                    const size_t stages[] = {1, (size_t)K * 2 * coarse_row + 1280, 0};
                    for (size_t stage : stages) {
                        Shaped mean(K, ols, H, ors, W, sizeof(T), kFresh), fraction(K, ols, H, ors, W, sizeof(T), kFresh);
                        Shaped count(K, ols, H, ors, W, 4, kFresh);
                        ok(ctx, call<T>(ctx, grid, values.data(), K, ls, rs, 0.5, &mean, all ? &fraction : nullptr, all ? &count : nullptr,
                                        MOD16_HOST, stage), what);
                        mean.check(true, "mean");
                        fraction.check(all != 0, "fraction");
                        count.check(all != 0, "count");
                    }
                    EXPECT(values.guards_intact());
                }
        if (sizeof(T) == 4) {                              // the class raster once per geometry
            for (int pitched = 0; pitched < 2; ++pitched) {
                const int64_t rs = pitched ? C + 5 : C, ors = pitched ? W + 3 : W;
                Shaped cls(1, R * rs, R, rs, C, 1, 0);
                for (size_t stage : {(size_t)1, (size_t)(2 * (8 * C + 2 * 256) + 1024), (size_t)0}) {
                    Shaped out_cls(1, H * ors, H, ors, W, 1, kFresh), share(1, H * ors, H, ors, W, 4, kFresh);
                    ok(ctx, mod16_upscale_classes(ctx, grid, cls.data(), rs, 0x1fffu, out_cls.data(), ors,
                                                  pitched ? nullptr : reinterpret_cast<float*>(share.data()), ors, MOD16_HOST, nullptr, stage),
                       "classes");
                    out_cls.check(true, "out_cls");
                    share.check(!pitched, "out_share");
                }
                EXPECT(cls.guards_intact());
            }
        }
        EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    }
    printf("host_asan_upscale: %s done\n", what);
}

// refused before any device work
static void refusals(mod16_ctx* ctx) {
    const Axis rows = axis({2, 2}, 0, false), cols = axis({3, 3, 3}, 0, false);
    const int64_t R = 4, C = 9, H = 2, W = 3;
    mod16_upscale_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.rows = R; spec.cols = C; spec.coarse_rows = H; spec.coarse_cols = W;
    mod16_upscale* grid = reinterpret_cast<mod16_upscale*>(&spec);
    auto create = [&](const mod16_upscale_spec& sp, const std::vector<int32_t>& rf, const std::vector<int32_t>& rc,
                      const std::vector<int32_t>& cf, const std::vector<int32_t>& cc, const double* area) {
        grid = reinterpret_cast<mod16_upscale*>(&spec);
        return mod16_upscale_create(ctx, &sp, rf.data(), rc.data(), cf.data(), cc.data(), area, &grid);
    };
    auto refused = [&](int rc, const char* prefix, const char* part) { return ::refused(ctx, rc, prefix, part); };
    const char* const cr = "mod16_upscale_create: ";
    mod16_upscale_spec sp = spec;
    EXPECT(refused(mod16_upscale_create(ctx, nullptr, rows.first.data(), rows.count.data(), cols.first.data(), cols.count.data(), nullptr, &grid), cr, "NULL argument"));
    EXPECT(grid == nullptr);
    EXPECT(refused(mod16_upscale_create(ctx, &spec, rows.first.data(), nullptr, cols.first.data(), cols.count.data(), nullptr, &grid), cr, "NULL argument"));
    EXPECT(refused(mod16_upscale_create(ctx, &spec, rows.first.data(), rows.count.data(), cols.first.data(), cols.count.data(), nullptr, nullptr), cr, "NULL argument"));
    sp = spec; sp.rows = 0; EXPECT(refused(create(sp, rows.first, rows.count, cols.first, cols.count, nullptr), cr, "rows and cols must be"));
    sp = spec; sp.cols = (int64_t(1) << 30) + 1; EXPECT(refused(create(sp, rows.first, rows.count, cols.first, cols.count, nullptr), cr, "rows and cols must be"));
    sp = spec; sp.coarse_rows = 0; EXPECT(refused(create(sp, rows.first, rows.count, cols.first, cols.count, nullptr), cr, "coarse_rows and coarse_cols must be"));
    sp = spec; sp.wrap_cols = 2; EXPECT(refused(create(sp, rows.first, rows.count, cols.first, cols.count, nullptr), cr, "wrap_cols"));
    EXPECT(refused(create(spec, rows.first, {2, -1}, cols.first, cols.count, nullptr), cr, "a count lies outside"));
    EXPECT(refused(create(spec, rows.first, {2, 5}, cols.first, cols.count, nullptr), cr, "a count lies outside"));
    EXPECT(refused(create(spec, {0, 4}, rows.count, cols.first, cols.count, nullptr), cr, "a run leaves its axis"));
    EXPECT(refused(create(spec, {0, -1}, rows.count, cols.first, cols.count, nullptr), cr, "a run leaves its axis"));
    EXPECT(refused(create(spec, {0, 3}, rows.count, cols.first, cols.count, nullptr), cr, "a run leaves its axis"));
    EXPECT(refused(create(spec, rows.first, rows.count, {0, 3, 7}, cols.count, nullptr), cr, "a run leaves its axis"));       // cyclic without wrap_cols
    EXPECT(refused(create(spec, {0, 1}, rows.count, cols.first, cols.count, nullptr), cr, "share a fine index"));
    sp = spec; sp.wrap_cols = 1;
    EXPECT(refused(create(sp, rows.first, rows.count, {0, 3, 7}, {3, 3, 3}, nullptr), cr, "share a fine index"));          // 7, 8, 0 meets 0, 1, 2
    EXPECT(grid == nullptr);
    {
        const double nan = std::nan("");
        for (double v : {0.0, -1.0, nan, (double)INFINITY}) {
            const double area[4] = {1.0, 1.0, v, 1.0};
            EXPECT(refused(create(spec, rows.first, rows.count, cols.first, cols.count, area), cr, "area must be positive and finite"));
        }
    }
    {   // 2^16 rows x 2^15 columns in one cell: 2^31 pixels
        mod16_upscale_spec big = spec;
        big.rows = 1 << 16; big.cols = 1 << 15; big.coarse_rows = big.coarse_cols = 1;
        EXPECT(refused(create(big, {0}, {1 << 16}, {0}, {1 << 15}, nullptr), cr, "fewer than 2^31 pixels"));
    }
    ok(ctx, create(spec, rows.first, rows.count, cols.first, cols.count, nullptr), "create");
    EXPECT(grid && grid != reinterpret_cast<mod16_upscale*>(&spec));

    const int32_t K = 2;
    Shaped values(K, R * C, R, C, C, 8, 0), mean(K, H * W, H, W, W, 8, kFresh), fraction(K, H * W, H, W, W, 8, kFresh);
    Shaped count(K, H * W, H, W, W, 4, kFresh);
    const char* const up = "mod16_upscale: ";
    auto go = [&](const mod16_upscale* g, const void* v, int32_t layers, int64_t ls, int64_t rs, double mf, int where, size_t stage) {
        return call<double>(ctx, g, v, layers, ls, rs, mf, &mean, &fraction, &count, where, stage);
    };
    EXPECT(refused(go(nullptr, values.data(), K, R * C, C, 0.0, MOD16_HOST, 0), up, "NULL grid or values"));
    EXPECT(refused(go(grid, nullptr, K, R * C, C, 0.0, MOD16_DEVICE, 0), up, "NULL grid or values"));
    EXPECT(refused(call<double>(ctx, grid, values.data(), K, R * C, C, 0.0, nullptr, nullptr, nullptr, MOD16_HOST, 0), up, "no output is requested"));
    EXPECT(refused(go(grid, values.data(), 0, R * C, C, 0.0, MOD16_HOST, 0), up, "layers must be between 1 and 65535"));
    EXPECT(refused(go(grid, values.data(), 65536, R * C, C, 0.0, MOD16_HOST, 0), up, "layers must be between 1 and 65535"));
    for (double mf : {-0.5, 1.5, std::nan("")}) EXPECT(refused(go(grid, values.data(), K, R * C, C, mf, MOD16_HOST, 0), up, "min_fraction"));
    EXPECT(refused(go(grid, values.data(), K, R * C, C - 1, 0.0, MOD16_HOST, 0), up, "a row stride is below"));
    EXPECT(refused(go(grid, values.data(), K, R * C - 1, C, 0.0, MOD16_DEVICE, 0), up, "a layer stride is below a plane"));
    EXPECT(refused(go(grid, values.data(), K, R * C, int64_t(1) << 60, 0.0, MOD16_HOST, 0), up, "out of range"));
    EXPECT(refused(go(grid, values.data(), K, int64_t(1) << 60, C, 0.0, MOD16_HOST, 0), up, "out of range"));
    EXPECT(refused(go(grid, values.data(), K, R * C, C, 0.0, 7, 0), up, "`where` must be"));
    EXPECT(refused(go(grid, values.data(), K, R * C, C, 0.0, MOD16_HOST, ~size_t(0)), up, "stage_bytes"));
    {
        Shaped narrow(K, H * W, H, W - 1, W - 1, 8, kFresh);
        EXPECT(refused(call<double>(ctx, grid, values.data(), K, R * C, C, 0.0, &narrow, nullptr, nullptr, MOD16_HOST, 0), up, "a row stride is below"));
        narrow.check(false, "the narrow mean");
        // an output on the input, two outputs on each other
        EXPECT(refused(mod16_upscale_f64(ctx, grid, reinterpret_cast<const double*>(values.data()), K, R * C, C, 0.0,
                                         reinterpret_cast<double*>(values.data()) + 5, H * W, W, nullptr, 0, 0, nullptr, 0, 0, MOD16_HOST, nullptr, 0),
                       up, "overlaps"));
        EXPECT(refused(mod16_upscale_f64(ctx, grid, reinterpret_cast<const double*>(values.data()), K, R * C, C, 0.0,
                                         reinterpret_cast<double*>(mean.data()), H * W, W, reinterpret_cast<double*>(mean.data()) + K * H * W - 1, H * W, W,
                                         nullptr, 0, 0, MOD16_DEVICE, nullptr, 0),
                       up, "overlaps"));
    }
    const char* const uc = "mod16_upscale_classes: ";
    Shaped cls(1, R * C, R, C, C, 1, 0), out_cls(1, H * W, H, W, W, 1, kFresh), share(1, H * W, H, W, W, 4, kFresh);
    auto classes = [&](const mod16_upscale* g, const void* c, int64_t rs, void* oc, int64_t ors, void* os, int where, size_t stage) {
        return mod16_upscale_classes(ctx, g, static_cast<const uint8_t*>(c), rs, 0x1fffu, static_cast<uint8_t*>(oc), ors,
                                     static_cast<float*>(os), W, where, nullptr, stage);
    };
    EXPECT(refused(classes(nullptr, cls.data(), C, out_cls.data(), W, share.data(), MOD16_HOST, 0), uc, "NULL grid or class raster"));
    EXPECT(refused(classes(grid, nullptr, C, out_cls.data(), W, share.data(), MOD16_HOST, 0), uc, "NULL grid or class raster"));
    EXPECT(refused(classes(grid, cls.data(), C, nullptr, W, nullptr, MOD16_HOST, 0), uc, "no output is requested"));
    EXPECT(refused(classes(grid, cls.data(), C - 1, out_cls.data(), W, share.data(), MOD16_HOST, 0), uc, "a row stride is below"));
    EXPECT(refused(classes(grid, cls.data(), C, out_cls.data(), W - 1, share.data(), MOD16_DEVICE, 0), uc, "a row stride is below"));
    EXPECT(refused(classes(grid, cls.data(), C, out_cls.data(), W, share.data(), 3, 0), uc, "`where` must be"));
    EXPECT(refused(classes(grid, cls.data(), C, out_cls.data(), W, share.data(), MOD16_HOST, ~size_t(0)), uc, "stage_bytes"));
    EXPECT(refused(classes(grid, cls.data(), C, cls.data() + 3, W, share.data(), MOD16_HOST, 0), uc, "overlaps"));
    mean.check(false, "mean of the refused calls");
    fraction.check(false, "fraction of the refused calls");
    count.check(false, "count of the refused calls");
    out_cls.check(false, "out_cls of the refused calls");
    share.check(false, "out_share of the refused calls");
    EXPECT(values.guards_intact() && cls.guards_intact());
    EXPECT(mod16_upscale_destroy(grid) == MOD16_OK);
    EXPECT(mod16_upscale_destroy(nullptr) == MOD16_OK);
    printf("host_asan_upscale: refusals done\n");
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
