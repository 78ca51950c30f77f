// Stand-alone driver of tests/test_trend_host_asan.py: the HOST mode of mod16_trend_f32 / _f64 -- the
// library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP
// stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check;
// the trend kernels have no shadow there). Every host array sits between guard bytes; n = 37 and 300
// pixels, Y = 5 and 33 steps, three stage_bytes (the smallest range of pixels: 256 + 44 at n = 300, a
// slab cut from the bytes of a range's rows, one chunk), a dense stack and one with time_stride > n,
// all outputs and a subset, both input types. Pass: no sanitizer report, every requested output
// element overwritten, no guard byte and no byte between the rows touched, nothing left allocated.
#include <cmath>
#include <limits>

#define HARNESS_NAME "host_asan_trend"
#include "harness.hpp"

constexpr int kOutputs = 5;

template <typename IN>
static int call(mod16_ctx* ctx, const mod16_trend_spec* spec, const void* values, const double* times, double* const* out,
                int32_t* s, uint8_t* count, int where, size_t stage) {
    if (sizeof(IN) == 4)
        return mod16_trend_f32(ctx, spec, static_cast<const float*>(values), times, out, s, count, where, nullptr, stage);
    return mod16_trend_f64(ctx, spec, static_cast<const double*>(values), times, out, s, count, where, nullptr, stage);
}

template <typename IN>
static void run(mod16_ctx* ctx, const char* what) {
    const int64_t sizes[] = {37, 300};
    const int steps[] = {5, 33};
    for (int64_t n : sizes)
        for (int Y : steps)
            for (int pitched = 0; pitched < 2; ++pitched)
                for (int all = 0; all < 2; ++all) {       // every output / slope, z and count alone
                    mod16_trend_spec spec;
                    memset(&spec, 0, sizeof spec);
                    spec.n = n; spec.steps = Y; spec.min_valid = 4;
                    spec.time_stride = pitched ? n + 5 : n;
                    spec.zq = all ? 1.96 : 0.0;
                    std::vector<double> times(Y);
                    for (int y = 0; y < Y; ++y) times[y] = 2001.0 + y;
                    Guarded in((size_t)((Y - 1) * spec.time_stride + n) * sizeof(IN), 0);
                    const bool want[kOutputs] = {true, all != 0, all != 0, all != 0, true};
                    // a slot's slab: 33 KiB per staged array and 512 bytes, then per pixel the rows of 8 bytes and the count
                    const size_t fixed = 7 * 33 * 1024 + 512, per_pixel = (size_t)(6 + Y) * 8 + 1;
                    const size_t stages[] = {1, fixed + per_pixel * 280, 0};
                    for (size_t stage : stages) {
                        std::vector<Guarded> out;
                        out.reserve(kOutputs);
                        double* outs[kOutputs] = {};
                        for (int o = 0; o < kOutputs; ++o)
                            if (want[o]) {
                                out.emplace_back((size_t)n * 8, kFresh);
                                outs[o] = reinterpret_cast<double*>(out.back().data());
                            }
                        Guarded s((size_t)n * 4, kFresh), count((size_t)n, kFresh);
                        const int rc = call<IN>(ctx, &spec, in.data(), times.data(), outs, all ? reinterpret_cast<int32_t*>(s.data()) : nullptr,
                                                count.data(), MOD16_HOST, stage);
                        if (rc != MOD16_OK) {
                            fprintf(stderr, "host_asan_trend: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                            exit(1);
                        }
                        for (Guarded& g : out) check_written(g, 8, true, "out");
                        check_written(s, 4, all != 0, "s");
                        check_written(count, 1, true, "count");
                    }
                    EXPECT(in.guards_intact());
                }
    printf("host_asan_trend: %s done\n", what);
}

// refused before any device work; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const int64_t n = 12;
    const int Y = 6;
    Guarded x((size_t)Y * n * 8, 0), o0((size_t)n * 8, kFresh), o1((size_t)n * 8, kFresh), sv((size_t)n * 4, kFresh), cv((size_t)n, kFresh);
    std::vector<double> times(Y);
    for (int y = 0; y < Y; ++y) times[y] = y;
    double* outs[kOutputs] = {reinterpret_cast<double*>(o0.data()), nullptr, nullptr, nullptr, reinterpret_cast<double*>(o1.data())};
    int32_t* s = reinterpret_cast<int32_t*>(sv.data());
    uint8_t* count = cv.data();
    mod16_trend_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.n = n; spec.steps = Y; spec.min_valid = 4; spec.time_stride = n; spec.zq = 0.0;
    auto go = [&](const mod16_trend_spec& sp, double* const* o, int where) {
        return call<double>(ctx, &sp, x.data(), times.data(), o, s, count, where, 0);
    };
    auto refused = [&](int rc, const char* part) { return ::refused(ctx, rc, "mod16_trend: ", part); };
    const double inf = std::numeric_limits<double>::infinity();
    mod16_trend_spec sp = spec;
    EXPECT(refused(call<double>(ctx, nullptr, x.data(), times.data(), outs, s, count, MOD16_HOST, 0), "NULL spec"));
    EXPECT(refused(call<double>(ctx, &spec, nullptr, times.data(), outs, s, count, MOD16_HOST, 0), "NULL spec, values or times"));
    EXPECT(refused(call<float>(ctx, &spec, x.data(), nullptr, outs, s, count, MOD16_HOST, 0), "NULL spec, values or times"));
    {
        double* none[kOutputs] = {};
        EXPECT(refused(call<double>(ctx, &spec, x.data(), times.data(), none, nullptr, nullptr, MOD16_HOST, 0), "no output is requested"));
        EXPECT(refused(call<double>(ctx, &spec, x.data(), times.data(), nullptr, nullptr, nullptr, MOD16_DEVICE, 0), "no output is requested"));
    }
    sp = spec; sp.n = -1; EXPECT(refused(go(sp, outs, MOD16_HOST), "n must be between 0 and 2^30"));
    sp = spec; sp.n = (int64_t(1) << 30) + 1; sp.time_stride = sp.n; EXPECT(refused(go(sp, outs, MOD16_HOST), "n must be between 0 and 2^30"));
    sp = spec; sp.steps = 1; EXPECT(refused(go(sp, outs, MOD16_HOST), "steps must be between 2 and 64"));
    sp = spec; sp.steps = 65; EXPECT(refused(go(sp, outs, MOD16_HOST), "steps must be between 2 and 64"));
    sp = spec; sp.time_stride = n - 1; EXPECT(refused(go(sp, outs, MOD16_HOST), "time_stride must be at least n"));
    times[2] = std::nan(""); EXPECT(refused(go(spec, outs, MOD16_HOST), "times must be finite")); times[2] = 2.0;
    times[5] = inf; EXPECT(refused(go(spec, outs, MOD16_DEVICE), "times must be finite")); times[5] = 5.0;
    times[3] = 2.0; EXPECT(refused(go(spec, outs, MOD16_HOST), "strictly increasing")); times[3] = 3.0;
    times[0] = -1.5e308; times[5] = 1.5e308; EXPECT(refused(go(spec, outs, MOD16_HOST), "span of times")); times[0] = 0.0; times[5] = 5.0;
    sp = spec; sp.min_valid = 1; EXPECT(refused(go(sp, outs, MOD16_HOST), "min_valid must be between 2 and steps"));
    sp = spec; sp.min_valid = Y + 1; EXPECT(refused(go(sp, outs, MOD16_HOST), "min_valid must be between 2 and steps"));
    sp = spec; sp.zq = -1.0; EXPECT(refused(go(sp, outs, MOD16_HOST), "zq must be finite and not negative"));
    sp = spec; sp.zq = inf; EXPECT(refused(go(sp, outs, MOD16_HOST), "zq must be finite and not negative"));
    sp = spec; sp.zq = std::nan(""); EXPECT(refused(go(sp, outs, MOD16_HOST), "zq must be finite and not negative"));
    {
        double* with_lo[kOutputs] = {outs[0], nullptr, outs[4], nullptr, nullptr};
        EXPECT(refused(go(spec, with_lo, MOD16_HOST), "need zq > 0"));
        double* with_hi[kOutputs] = {outs[0], nullptr, nullptr, outs[4], nullptr};
        EXPECT(refused(go(spec, with_hi, MOD16_DEVICE), "need zq > 0"));
    }
    EXPECT(refused(go(spec, outs, 7), "`where` must be"));
    EXPECT(refused(call<double>(ctx, &spec, x.data(), times.data(), outs, s, count, MOD16_HOST, ~size_t(0)), "stage_bytes"));
    {   // an output on the input, two outputs on each other, s on an output, count on the times
        double* on_in[kOutputs] = {reinterpret_cast<double*>(x.data()) + 3 * n, nullptr, nullptr, nullptr, nullptr};
        EXPECT(refused(go(spec, on_in, MOD16_HOST), "overlaps"));
        EXPECT(refused(go(spec, on_in, MOD16_DEVICE), "overlaps"));
        double* twice[kOutputs] = {outs[0], outs[0] + n - 1, nullptr, nullptr, nullptr};
        EXPECT(refused(go(spec, twice, MOD16_HOST), "overlaps"));
        EXPECT(refused(call<double>(ctx, &spec, x.data(), times.data(), outs, reinterpret_cast<int32_t*>(o1.data()), count, MOD16_HOST, 0), "overlaps"));
        EXPECT(refused(call<double>(ctx, &spec, x.data(), times.data(), outs, s, reinterpret_cast<uint8_t*>(times.data()), MOD16_HOST, 0), "overlaps"));
    }
    sp = spec; sp.n = 0; sp.time_stride = 0; EXPECT(go(sp, outs, MOD16_HOST) == MOD16_OK);
    EXPECT(go(sp, outs, MOD16_DEVICE) == MOD16_OK);
    EXPECT(mod16_trend_max_steps() == 64);
    check_written(o0, 8, false, "out[0] of the refused calls");
    check_written(o1, 8, false, "out[4] of the refused calls");
    check_written(sv, 4, false, "s of the refused calls");
    check_written(cv, 1, false, "count of the refused calls");
    EXPECT(x.guards_intact());
    printf("host_asan_trend: refusals done\n");
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
