// Stand-alone driver of tests/test_regress_host_asan.py: the HOST mode of mod16_regress_f32 / _f64 -- the
// library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP
// stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check;
// the regression kernels have no shadow there). Every host array sits between guard bytes; 1237 pixels in
// tiles of 256, of 512 and in one tile; T = 5 and T = 1; both value types; (Ks, Kp) = (2, 0), (0, 2) and
// (1, 3); weights, the standard errors and the two series modes on and off; every array with a pitch of
// its own. Pass: no sanitizer report, every output element overwritten, no guard byte and no padding
// byte of a pitched output touched, nothing left allocated.
#include <algorithm>
#include <cmath>
#include <limits>

#define HARNESS_NAME "host_asan_regress"
#include "harness.hpp"

template <typename IN>
static int call(mod16_ctx* ctx, const mod16_regress_spec* spec, const void* values, const double* design, const void* const* terms,
                const float* weights, double* coef, double* se, double* rss, double* tss, double* r2, uint16_t* count,
                void* series, int where, size_t stage) {
    if (sizeof(IN) == 4)
        return mod16_regress_f32(ctx, spec, static_cast<const float*>(values), design, reinterpret_cast<const float* const*>(terms),
                                 weights, coef, se, rss, tss, r2, count, static_cast<float*>(series), where, nullptr, stage);
    return mod16_regress_f64(ctx, spec, static_cast<const double*>(values), design, reinterpret_cast<const double* const*>(terms),
                             weights, coef, se, rss, tss, r2, count, static_cast<double*>(series), where, nullptr, stage);
}

// the launches the calls of run() must have made: one per tile of 256, of 512 and of all 1237 pixels (5 + 3 + 1 a
// configuration); main prints the sum and tests/test_regress_host_asan.py holds the stand-in's count against it
static long g_expected_launches = 0;

template <typename IN>
static void run(mod16_ctx* ctx, int T, int ks, int kp, const char* what) {
    const int64_t n = 1237, vpitch = n + 19, tpitch = n + 11, wpitch = n + 3, cpitch = n + 7, spitch = n + 5, rpitch = n + 13;
    const int P = ks + kp;
    std::vector<double> design((size_t)T * std::max(ks, 1), 0.25);
    for (int weighted = 0; weighted < 2; ++weighted)
        for (int with_se = 0; with_se < 2; ++with_se)
            for (int mode = 0; mode < 3; ++mode) {       // no series, residuals, fitted
                mod16_regress_spec spec;
                memset(&spec, 0, sizeof spec);
                spec.n = n; spec.steps = T; spec.ks = ks; spec.kp = kp; spec.min_valid = P + (mode ? 1 : 0);
                spec.series = mode;
                spec.value_pitch = vpitch; spec.term_pitch = tpitch; spec.weight_pitch = wpitch;
                spec.coef_pitch = cpitch; spec.se_pitch = spitch; spec.series_pitch = rpitch;
                Guarded in(span(T, vpitch, n, sizeof(IN)), 0), w(span(T, wpitch, n, 4), 0);
                std::vector<Guarded> terms;
                std::vector<const void*> tptr;
                for (int k = 0; k < kp; ++k) terms.emplace_back(span(T, tpitch, n, sizeof(IN)), 0);
                for (int k = 0; k < kp; ++k) tptr.push_back(terms[k].data());
                // the slab of a slot: 9 + kp arrays apart by the stagger; per pixel the rows, each in a float64-sized place
                const int wide_rows = P + (with_se ? P : 1) + 4 + (mode ? T : 1) + T * (1 + kp) + (weighted ? T : 1);
                const size_t fixed = (size_t)(9 + kp) * 33 * 1024 + 512, per_pixel = (size_t)wide_rows * 8;
                // tiles of 256 and of 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
                const size_t stages[] = {fixed + 300 * per_pixel, fixed + 600 * per_pixel, 0};
                const int64_t tiles[] = {256, 512, n};
                for (int k = 0; k < 3; ++k) {
                    const size_t stage = stages[k];
                    g_expected_launches += (long)((n + tiles[k] - 1) / tiles[k]);
                    Guarded coef(span(P, cpitch, n, 8), kFresh), se(span(P, spitch, n, 8), kFresh);
                    Guarded rss((size_t)n * 8, kFresh), tss((size_t)n * 8, kFresh), r2((size_t)n * 8, kFresh);
                    Guarded count((size_t)n * 2, kFresh), series(span(T, rpitch, n, sizeof(IN)), kFresh);
                    const int rc = call<IN>(ctx, &spec, in.data(), ks ? design.data() : nullptr, kp ? tptr.data() : nullptr,
                                            weighted ? w.as<float>() : nullptr, coef.as<double>(), with_se ? se.as<double>() : nullptr,
                                            rss.as<double>(), tss.as<double>(), r2.as<double>(), count.as<uint16_t>(),
                                            mode ? series.data() : nullptr, MOD16_HOST, stage);
                    if (rc != MOD16_OK) {
                        fprintf(stderr, "host_asan_regress: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                        exit(1);
                    }
                    check_written(coef, P, cpitch, n, 8, true, "coef");
                    check_written(se, P, spitch, n, 8, with_se != 0, "se");
                    check_written(rss, 8, true, "rss");
                    check_written(tss, 8, true, "tss");
                    check_written(r2, 8, true, "r2");
                    check_written(count, 2, true, "count");
                    check_written(series, T, rpitch, n, sizeof(IN), mode != 0, "series");
                }
                EXPECT(in.guards_intact() && w.guards_intact());
                for (auto& t : terms) EXPECT(t.guards_intact());
            }
    printf("host_asan_regress: %s, %d steps, %d + %d terms done\n", what, T, ks, kp);
}

// refused before any device work and before an output is touched; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const int64_t n = 300;
    const int T = 4;
    const char* pre = "mod16_regress: ";
    Guarded v(span(T, n, n, 8), 0), t0(span(T, n, n, 8), 0), wf(span(T, n, n, 4), 0);
    Guarded coef(span(2, n, n, 8), kFresh), se(span(2, n, n, 8), kFresh), rss((size_t)n * 8, kFresh), cnt((size_t)n * 2, kFresh);
    Guarded series(span(T, n, n, 8), kFresh);
    std::vector<double> design((size_t)T, 1.0);
    const double* terms[1] = {t0.as<double>()};
    const double* none[1] = {nullptr};
    mod16_regress_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.n = n; spec.steps = T; spec.ks = 1; spec.kp = 1; spec.min_valid = 3; spec.series = MOD16_REGRESS_SERIES_RESIDUALS;
    spec.value_pitch = spec.term_pitch = spec.weight_pitch = spec.coef_pitch = spec.se_pitch = spec.series_pitch = n;
    auto f64 = [&](const mod16_regress_spec& s, const void* values, const double* d, const double* const* t, const void* w, void* c,
                   void* e, void* r, void* k, void* ser, int where) {
        return mod16_regress_f64(ctx, &s, static_cast<const double*>(values), d, t, static_cast<const float*>(w),
                                 static_cast<double*>(c), static_cast<double*>(e), static_cast<double*>(r), nullptr, nullptr,
                                 static_cast<uint16_t*>(k), static_cast<double*>(ser), where, nullptr, 0);
    };
    auto usual = [&](const mod16_regress_spec& s) {
        return f64(s, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), series.data(), MOD16_HOST);
    };
    mod16_regress_spec s = spec;
    EXPECT(mod16_regress_f64(nullptr, &spec, v.as<double>(), design.data(), terms, nullptr, coef.as<double>(), nullptr, nullptr, nullptr,
                             nullptr, nullptr, series.as<double>(), MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(refused(ctx, mod16_regress_f64(ctx, nullptr, v.as<double>(), design.data(), terms, nullptr, coef.as<double>(), nullptr, nullptr,
                                          nullptr, nullptr, nullptr, series.as<double>(), MOD16_HOST, nullptr, 0), pre, "NULL"));
    EXPECT(refused(ctx, f64(spec, nullptr, design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), series.data(), MOD16_HOST), pre, "NULL"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), nullptr, se.data(), rss.data(), cnt.data(), series.data(), MOD16_HOST), pre, "NULL"));
    s.n = -1; EXPECT(refused(ctx, usual(s), pre, "n < 0"));
    s = spec; s.steps = 0; EXPECT(refused(ctx, usual(s), pre, "steps"));
    s = spec; s.steps = mod16_regress_max_steps() + 1; EXPECT(refused(ctx, usual(s), pre, "steps"));
    s = spec; s.ks = -1; EXPECT(refused(ctx, usual(s), pre, "ks and kp"));
    s = spec; s.ks = 8; EXPECT(refused(ctx, usual(s), pre, "ks and kp"));
    s = spec; s.ks = 0; s.kp = 0; EXPECT(refused(ctx, usual(s), pre, "ks and kp"));
    s = spec; s.kp = mod16_regress_max_terms() + 1; s.ks = 0; EXPECT(refused(ctx, usual(s), pre, "ks and kp"));
    s = spec; s.ks = 0; s.min_valid = 1; EXPECT(refused(ctx, usual(s), pre, "design"));          // a design without ks
    EXPECT(refused(ctx, f64(spec, v.data(), nullptr, terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), series.data(), MOD16_HOST), pre, "design"));
    s = spec; s.kp = 0; s.min_valid = 1; EXPECT(refused(ctx, usual(s), pre, "terms"));           // terms without kp
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), nullptr, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), series.data(), MOD16_HOST), pre, "terms"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), none, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), series.data(), MOD16_HOST), pre, "NULL pointer"));
    s = spec; s.min_valid = 1; EXPECT(refused(ctx, usual(s), pre, "min_valid"));
    s = spec; s.series = 3; EXPECT(refused(ctx, usual(s), pre, "series must be"));
    s = spec; s.series = MOD16_REGRESS_SERIES_NONE; EXPECT(refused(ctx, usual(s), pre, "series output"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), nullptr, MOD16_HOST), pre, "series output"));
    s = spec; s.value_pitch = n - 1; EXPECT(refused(ctx, usual(s), pre, "value_pitch"));
    s = spec; s.term_pitch = n - 1; EXPECT(refused(ctx, usual(s), pre, "term_pitch"));
    s = spec; s.weight_pitch = n - 1; EXPECT(refused(ctx, usual(s), pre, "weight_pitch"));
    s = spec; s.coef_pitch = n - 1; EXPECT(refused(ctx, usual(s), pre, "coef_pitch"));
    s = spec; s.se_pitch = n - 1; EXPECT(refused(ctx, usual(s), pre, "se_pitch"));
    s = spec; s.series_pitch = n - 1; EXPECT(refused(ctx, usual(s), pre, "series_pitch"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), series.data(), 7), pre, "where"));
    design[2] = std::nan("");
    EXPECT(refused(ctx, usual(spec), pre, "design must be finite"));
    design[2] = std::numeric_limits<double>::infinity();
    EXPECT(refused(ctx, usual(spec), pre, "design must be finite"));
    design[2] = 1.0;
    // in place; the series on a term, on the weights, on the design; the counts on the coefficients; se on coef
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), v.data(), MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), cnt.data(), t0.data() + 8, MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), wf.data(), se.data(), rss.data(), cnt.data(), series.data(), MOD16_DEVICE), pre, "overlaps"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), design.data(), cnt.data(), series.data(), MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), se.data(), rss.data(), coef.data() + 16, series.data(), MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, f64(spec, v.data(), design.data(), terms, wf.data(), coef.data(), coef.data() + 8 * n, rss.data(), cnt.data(), series.data(), MOD16_HOST), pre, "overlaps"));
    s = spec; s.n = 0; EXPECT(usual(s) == MOD16_OK);
    check_written(coef, 2, n, n, 8, false, "coef of the refused calls");
    check_written(se, 2, n, n, 8, false, "se of the refused calls");
    check_written(rss, 8, false, "rss of the refused calls");
    check_written(cnt, 2, false, "count of the refused calls");
    check_written(series, T, n, n, 8, false, "series of the refused calls");
    EXPECT(v.guards_intact() && t0.guards_intact() && wf.guards_intact());
    printf("host_asan_regress: refusals done\n");
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    EXPECT(mod16_regress_max_steps() >= 1104 && mod16_regress_max_terms() == 8);
    const int steps[] = {5, 1};
    const int splits[][2] = {{2, 0}, {0, 2}, {1, 3}};
    for (int T : steps)
        for (auto& split : splits) {
            run<float>(ctx, T, split[0], split[1], "float32");
            run<double>(ctx, T, split[0], split[1], "float64");
        }
    refusals(ctx);
    printf("host_asan_regress: expected launches %ld\n", g_expected_launches);
    harness_finish(ctx);
    return 0;
}
