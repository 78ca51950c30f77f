// Stand-alone driver of tests/test_anomaly_host_asan.py: the HOST mode of mod16_anomaly_f32 / _f64 -- the
// library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP
// stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check;
// the anomaly kernels have no shadow there). Every host array sits between guard bytes; n = 37 and 300
// pixels, (Y, P, W) = (3, 5, 2) and (33, 2, 1), with and without den, three stage_bytes (the smallest
// range of pixels: 256 + 44 at n = 300, a slab cut from the bytes of a range's rows, one chunk), dense
// arrays and arrays with strides > n, all outputs and a subset, both types. Pass: no sanitizer report,
// every requested output element overwritten, no guard byte and no byte between the rows touched,
// nothing left allocated.
#include <cmath>

#define HARNESS_NAME "host_asan_anomaly"
#include "harness.hpp"

template <typename IN>
static int call(mod16_ctx* ctx, const mod16_anomaly_spec* spec, const void* num, const void* den, void* z, void* pct,
                void* mean, void* sdev, void* count, int where, size_t stage) {
    if (sizeof(IN) == 4)
        return mod16_anomaly_f32(ctx, spec, static_cast<const float*>(num), static_cast<const float*>(den), static_cast<float*>(z),
                                 static_cast<float*>(pct), static_cast<double*>(mean), static_cast<double*>(sdev),
                                 static_cast<uint8_t*>(count), where, nullptr, stage);
    return mod16_anomaly_f64(ctx, spec, static_cast<const double*>(num), static_cast<const double*>(den), static_cast<double*>(z),
                             static_cast<double*>(pct), static_cast<double*>(mean), static_cast<double*>(sdev),
                             static_cast<uint8_t*>(count), where, nullptr, stage);
}

template <typename IN>
static void run(mod16_ctx* ctx, const char* what) {
    const int64_t sizes[] = {37, 300};
    const int shapes[][3] = {{3, 5, 2}, {33, 2, 1}};          // Y, P, W
    for (int64_t n : sizes)
        for (const auto& ypw : shapes)
            for (int ratio = 0; ratio < 2; ++ratio)
                for (int pitched = 0; pitched < 2; ++pitched)
                    for (int all = 0; all < 2; ++all) {       // every output / z, std and count alone
                        const int Y = ypw[0], P = ypw[1], S = Y * P;
                        mod16_anomaly_spec spec;
                        memset(&spec, 0, sizeof spec);
                        spec.n = n; spec.years = Y; spec.periods = P; spec.window = ypw[2];
                        spec.base_first = Y > 3 ? 1 : 0; spec.base_end = Y > 3 ? Y - 1 : Y; spec.min_valid = 2;
                        spec.in_stride = pitched ? n + 5 : n;
                        spec.out_stride = pitched ? n + 3 : n;
                        spec.clim_stride = pitched ? n + 7 : n;
                        Shaped num(S, spec.in_stride, n, sizeof(IN), 0), den(S, spec.in_stride, n, sizeof(IN), 0);
                        // a slot's slab: 33 KiB per staged array and 512 bytes, then per pixel the rows of 8 bytes and the counts
                        const size_t fixed = 6 * 33 * 1024 + 512, per_pixel = (size_t)(4 * S + 2 * P) * 8 + P;
                        const size_t stages[] = {1, fixed + per_pixel * 280, 0};
                        for (size_t stage : stages) {
                            Shaped z(S, spec.out_stride, n, sizeof(IN), kFresh), pct(S, spec.out_stride, n, sizeof(IN), kFresh);
                            Shaped mean(P, spec.clim_stride, n, 8, kFresh), sdev(P, spec.clim_stride, n, 8, kFresh);
                            Shaped count(P, spec.clim_stride, n, 1, kFresh);
                            const int rc = call<IN>(ctx, &spec, num.data(), ratio ? den.data() : nullptr, z.data(), all ? pct.data() : nullptr,
                                                    all ? mean.data() : nullptr, sdev.data(), count.data(), MOD16_HOST, stage);
                            if (rc != MOD16_OK) {
                                fprintf(stderr, "host_asan_anomaly: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                                exit(1);
                            }
                            z.check(true, "z");
                            pct.check(all != 0, "pct");
                            mean.check(all != 0, "mean");
                            sdev.check(true, "std");
                            count.check(true, "count");
                        }
                        EXPECT(num.guards_intact() && den.guards_intact());
                    }
    printf("host_asan_anomaly: %s done\n", what);
}

// refused before any device work; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const int64_t n = 12;
    const int Y = 6, P = 4, S = Y * P;
    Shaped num(S, n, n, 8, 0), den(S, n, n, 8, 0), z(S, n, n, 8, kFresh), pct(S, n, n, 8, kFresh);
    Shaped mean(P, n, n, 8, kFresh), sdev(P, n, n, 8, kFresh), count(P, n, n, 1, kFresh);
    mod16_anomaly_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.n = n; spec.years = Y; spec.periods = P; spec.window = 2; spec.base_first = 1; spec.base_end = 5; spec.min_valid = 3;
    spec.in_stride = spec.out_stride = spec.clim_stride = n;
    auto go = [&](const mod16_anomaly_spec& sp, int where) {
        return call<double>(ctx, &sp, num.data(), den.data(), z.data(), pct.data(), mean.data(), sdev.data(), count.data(), where, 0);
    };
    auto refused = [&](int rc, const char* part) { return ::refused(ctx, rc, "mod16_anomaly: ", part); };
    mod16_anomaly_spec sp = spec;
    EXPECT(refused(call<double>(ctx, nullptr, num.data(), nullptr, z.data(), nullptr, nullptr, nullptr, nullptr, MOD16_HOST, 0), "NULL spec or num"));
    EXPECT(refused(call<float>(ctx, &spec, nullptr, den.data(), z.data(), nullptr, nullptr, nullptr, nullptr, MOD16_DEVICE, 0), "NULL spec or num"));
    EXPECT(refused(call<double>(ctx, &spec, num.data(), den.data(), nullptr, nullptr, nullptr, nullptr, nullptr, MOD16_HOST, 0), "no output is requested"));
    sp = spec; sp.n = -1; EXPECT(refused(go(sp, MOD16_HOST), "n must be between 0 and 2^30"));
    sp = spec; sp.n = (int64_t(1) << 30) + 1; sp.in_stride = sp.out_stride = sp.clim_stride = sp.n;
    EXPECT(refused(go(sp, MOD16_HOST), "n must be between 0 and 2^30"));
    sp = spec; sp.periods = 0; EXPECT(refused(go(sp, MOD16_HOST), "periods must be between 1 and 366"));
    sp = spec; sp.periods = 367; EXPECT(refused(go(sp, MOD16_DEVICE), "periods must be between 1 and 366"));
    sp = spec; sp.years = 1; EXPECT(refused(go(sp, MOD16_HOST), "years must be between 2 and 64"));
    sp = spec; sp.years = 65; EXPECT(refused(go(sp, MOD16_HOST), "years must be between 2 and 64"));
    sp = spec; sp.years = 64; sp.periods = 65; EXPECT(refused(go(sp, MOD16_HOST), "years * periods must be at most 4096"));
    sp = spec; sp.window = 0; EXPECT(refused(go(sp, MOD16_HOST), "window must be between 1 and min(periods, 16)"));
    sp = spec; sp.window = P + 1; EXPECT(refused(go(sp, MOD16_HOST), "window must be between 1 and min(periods, 16)"));
    sp = spec; sp.years = 2; sp.periods = 20; sp.base_first = 0; sp.base_end = 2; sp.min_valid = 2; sp.window = 17;
    EXPECT(refused(go(sp, MOD16_HOST), "window must be between 1 and min(periods, 16)"));
    sp = spec; sp.base_first = -1; EXPECT(refused(go(sp, MOD16_HOST), "the baseline must satisfy"));
    sp = spec; sp.base_first = 5; EXPECT(refused(go(sp, MOD16_HOST), "the baseline must satisfy"));
    sp = spec; sp.base_end = Y + 1; EXPECT(refused(go(sp, MOD16_HOST), "the baseline must satisfy"));
    sp = spec; sp.base_first = 4; sp.min_valid = 2; EXPECT(refused(go(sp, MOD16_HOST), "the baseline needs at least 2 years"));
    sp = spec; sp.min_valid = 1; EXPECT(refused(go(sp, MOD16_HOST), "min_valid must be between 2 and the baseline length"));
    sp = spec; sp.min_valid = 5; EXPECT(refused(go(sp, MOD16_HOST), "min_valid must be between 2 and the baseline length"));
    sp = spec; sp.in_stride = n - 1; EXPECT(refused(go(sp, MOD16_HOST), "in_stride must be at least n"));
    sp = spec; sp.out_stride = n - 1; EXPECT(refused(go(sp, MOD16_HOST), "out_stride must be at least n"));
    sp = spec; sp.clim_stride = 0; EXPECT(refused(go(sp, MOD16_DEVICE), "clim_stride must be at least n"));
    EXPECT(refused(go(spec, 7), "`where` must be"));
    EXPECT(refused(call<double>(ctx, &spec, num.data(), den.data(), z.data(), nullptr, nullptr, nullptr, nullptr, MOD16_HOST, ~size_t(0)), "stage_bytes"));
    {   // an output on an input, two outputs on each other, the counts on the mean
        double* in_num = reinterpret_cast<double*>(num.data()) + 3 * n;
        EXPECT(refused(call<double>(ctx, &spec, num.data(), den.data(), z.data(), nullptr, in_num, nullptr, nullptr, MOD16_HOST, 0), "overlaps"));
        EXPECT(refused(call<double>(ctx, &spec, num.data(), den.data(), den.data(), nullptr, nullptr, nullptr, nullptr, MOD16_DEVICE, 0), "overlaps"));
        EXPECT(refused(call<double>(ctx, &spec, num.data(), nullptr, z.data(), reinterpret_cast<double*>(z.data()) + n * S - 1, nullptr, nullptr, nullptr, MOD16_HOST, 0), "overlaps"));
        EXPECT(refused(call<double>(ctx, &spec, num.data(), nullptr, nullptr, nullptr, mean.data(), sdev.data(), mean.data() + 8 * n, MOD16_HOST, 0), "overlaps"));
    }
    sp = spec; sp.n = 0; sp.in_stride = sp.out_stride = sp.clim_stride = 0;
    EXPECT(go(sp, MOD16_HOST) == MOD16_OK);
    EXPECT(go(sp, MOD16_DEVICE) == MOD16_OK);
    EXPECT(mod16_anomaly_max_window() == 16);
    z.check(false, "z of the refused calls");
    pct.check(false, "pct of the refused calls");
    mean.check(false, "mean of the refused calls");
    sdev.check(false, "std of the refused calls");
    count.check(false, "count of the refused calls");
    EXPECT(num.guards_intact() && den.guards_intact());
    printf("host_asan_anomaly: refusals done\n");
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
