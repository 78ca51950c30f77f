// Stand-alone driver of tests/test_daynight_host_asan.py: the HOST mode of mod16_daynight_f32 / _f64 --
// the library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the
// HIP stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape
// check; the day / night kernels have no shadow there). Every host array sits between guard bytes;
// D = 5 days in chunks of 2 (ragged), of 1 and in one chunk; dense and pitched fields and outputs; all
// outputs and a few of them; both modes, both input and both output types. Pass: no sanitizer report,
// every requested output element overwritten, no guard byte and no padding byte touched, nothing left
// allocated.
#include <algorithm>
#include <cmath>

#define HARNESS_NAME "host_asan_daynight"
#include "harness.hpp"

constexpr int kFields = 5, kOutputs = 10;

template <typename IN>
static int call(mod16_ctx* ctx, const mod16_daynight_spec* spec, const void* const* fields, const double* half,
                const double* noon, const double* offset, void* const* out, void* annual, int where, size_t stage) {
    if (sizeof(IN) == 4)
        return mod16_daynight_f32(ctx, spec, reinterpret_cast<const float* const*>(fields), half, noon, offset, out, annual, where, nullptr, stage);
    return mod16_daynight_f64(ctx, spec, reinterpret_cast<const double* const*>(fields), half, noon, offset, out, annual, where, nullptr, stage);
}

template <typename IN>
static void run(mod16_ctx* ctx, int out_type, const char* what) {
    const int64_t R = 7, W = 37;
    const int D = 5, H = 3;
    const size_t isz = sizeof(IN), osz = out_type == MOD16_DAYNIGHT_F32 ? 4 : 8;
    std::vector<double> half((size_t)D * R, 6.0), noon(D, 12.0), offset(W, 0.0);
    for (int64_t c = 0; c < W; ++c) offset[c] = -12.0 + 24.0 * (double)c / (double)W;
    for (int pitched = 0; pitched < 2; ++pitched)
        for (int mode = 0; mode < 2; ++mode)
            for (int all = 0; all < 2; ++all) {         // every output / temp_day, day_hours and temp_annual alone
                mod16_daynight_spec spec;
                memset(&spec, 0, sizeof spec);
                spec.rows = R; spec.cols = W; spec.days = D; spec.steps_per_day = H;
                spec.mode = mode ? MOD16_DAYNIGHT_SW : MOD16_DAYNIGHT_SOLAR;
                spec.out_type = out_type;
                spec.threshold = 1.0;
                spec.in_pitch = pitched ? W + 3 : W;
                spec.in_plane = pitched ? R * spec.in_pitch + 5 : R * W;
                spec.out_pitch = pitched ? W + 7 : W;
                spec.out_plane = pitched ? R * spec.out_pitch + 2 : R * W;
                // the fields a call needs: all of them, or t (and sw in its mode)
                bool need[kFields] = {true, all != 0, all != 0, all != 0 || mode != 0, all != 0};
                bool want[kOutputs];
                for (int o = 0; o < kOutputs; ++o) want[o] = all || o == 3 || o == 8;
                std::vector<Guarded> in;
                in.reserve(kFields);
                const void* fields[kFields] = {};
                int nf = 0, no = 0;
                for (int f = 0; f < kFields; ++f)
                    if (need[f]) {
                        in.emplace_back(span((int64_t)D * H, spec.in_plane, R, spec.in_pitch, W, isz), (unsigned char)0);
                        fields[f] = in.back().data();
                        ++nf;
                    }
                for (int o = 0; o < kOutputs; ++o) no += want[o];
                const size_t per_day = (size_t)nf * H * R * W * isz + (size_t)no * R * W * osz;
                // chunks of 2 days (2, 2, 1), of 1 day (a slot smaller than a day: the minimum), one chunk
                const size_t stages[] = {2 * per_day + per_day / 2, per_day / 3, 0};
                for (size_t stage : stages) {
                    std::vector<Guarded> out;
                    out.reserve(kOutputs);
                    void* outs[kOutputs] = {};
                    for (int o = 0; o < kOutputs; ++o)
                        if (want[o]) {
                            out.emplace_back(span(D, spec.out_plane, R, spec.out_pitch, W, osz), kFresh);
                            outs[o] = out.back().data();
                        }
                    Guarded annual(span(1, 0, R, spec.out_pitch, W, osz), kFresh);
                    const int rc = call<IN>(ctx, &spec, fields, half.data(), noon.data(), offset.data(), outs, annual.data(), MOD16_HOST, stage);
                    if (rc != MOD16_OK) {
                        fprintf(stderr, "host_asan_daynight: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                        exit(1);
                    }
                    for (Guarded& g : out) check_written(g, D, spec.out_plane, R, spec.out_pitch, W, osz, true, "out");
                    check_written(annual, 1, R * spec.out_pitch, R, spec.out_pitch, W, osz, true, "temp_annual");
                }
                for (Guarded& g : in) EXPECT(g.guards_intact());
            }
    printf("host_asan_daynight: %s done\n", what);
}

// refused before any device work; zero days and zero cells are fine
static void refusals(mod16_ctx* ctx) {
    const int64_t R = 4, W = 6;
    const int D = 3, H = 2;
    Guarded t(span(D * H, R * W, R, W, W, 4), 0), sw(span(D * H, R * W, R, W, W, 4), 0);
    Guarded o0(span(D, R * W, R, W, W, 8), kFresh), o1(span(D, R * W, R, W, W, 8), kFresh), ann(span(1, 0, R, W, W, 8), kFresh);
    std::vector<double> half((size_t)D * R, 6.0), noon(D, 12.0), offset(W, 0.0);
    const void* fields[kFields] = {t.data(), nullptr, nullptr, sw.data(), nullptr};
    void* outs[kOutputs] = {};
    outs[3] = o0.data();        // temp_day
    outs[2] = o1.data();        // sw_rad_day
    mod16_daynight_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.rows = R; spec.cols = W; spec.days = D; spec.steps_per_day = H;
    spec.mode = MOD16_DAYNIGHT_SOLAR; spec.out_type = MOD16_DAYNIGHT_F64;
    spec.in_pitch = spec.out_pitch = W;
    spec.in_plane = spec.out_plane = R * W;
    auto go = [&](const mod16_daynight_spec& s, const void* const* f, void* const* o, void* a, int where) {
        return call<float>(ctx, &s, f, half.data(), noon.data(), offset.data(), o, a, where, 0);
    };
    auto refused = [&](int rc, const char* part) { return ::refused(ctx, rc, "mod16_daynight: ", part); };
    mod16_daynight_spec s = spec;
    EXPECT(refused(call<float>(ctx, nullptr, fields, half.data(), noon.data(), offset.data(), outs, ann.data(), MOD16_HOST, 0), "NULL spec"));
    EXPECT(refused(go(spec, nullptr, outs, ann.data(), MOD16_HOST), "NULL fields or out"));
    EXPECT(refused(go(spec, fields, nullptr, ann.data(), MOD16_HOST), "NULL fields or out"));
    {   // a requested output whose field is NULL: lw_net_day without lw, temp_annual without t, anything in 'sw' mode without sw
        void* lw[kOutputs] = {};
        lw[0] = o0.data();
        EXPECT(refused(go(spec, fields, lw, nullptr, MOD16_HOST), "whose field is NULL"));
        const void* no_t[kFields] = {nullptr, nullptr, nullptr, sw.data(), nullptr};
        void* only_sw[kOutputs] = {};
        only_sw[2] = o1.data();
        EXPECT(refused(go(spec, no_t, only_sw, ann.data(), MOD16_HOST), "the field t is NULL"));
        const void* no_sw[kFields] = {t.data(), nullptr, nullptr, nullptr, nullptr};
        void* only_t[kOutputs] = {};
        only_t[3] = o0.data();
        s = spec; s.mode = MOD16_DAYNIGHT_SW; s.threshold = 1.0;
        EXPECT(refused(go(s, no_sw, only_t, nullptr, MOD16_HOST), "whose field is NULL"));
        void* none[kOutputs] = {};
        EXPECT(refused(go(spec, fields, none, nullptr, MOD16_HOST), "no output is requested"));
    }
    s = spec; s.rows = -1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "rows and cols"));
    s = spec; s.cols = (int64_t(1) << 30) + 1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "rows and cols"));
    s = spec; s.days = -1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "days must be between 0 and 4096"));
    s = spec; s.days = 4097; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "days must be between 0 and 4096"));
    s = spec; s.steps_per_day = 0; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "steps_per_day must be between 1 and 48"));
    s = spec; s.steps_per_day = 49; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "steps_per_day must be between 1 and 48"));
    s = spec; s.in_pitch = W - 1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "must be at least cols"));
    s = spec; s.out_pitch = W - 1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "must be at least cols"));
    s = spec; s.in_plane = R * W - 1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "at least a plane"));
    s = spec; s.out_plane = R * W - 1; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "at least a plane"));
    s = spec; s.mode = 2; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "mode must be"));
    s = spec; s.out_type = 2; EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "out_type must be"));
    EXPECT(refused(go(spec, fields, outs, ann.data(), 7), "`where` must be"));
    // table values out of range or not finite, a NULL table
    half[5] = 12.5; EXPECT(refused(go(spec, fields, outs, ann.data(), MOD16_HOST), "half_day holds")); half[5] = 6.0;
    half[2] = std::nan(""); EXPECT(refused(go(spec, fields, outs, ann.data(), MOD16_DEVICE), "half_day holds")); half[2] = 6.0;
    noon[1] = -0.5; EXPECT(refused(go(spec, fields, outs, ann.data(), MOD16_HOST), "noon holds")); noon[1] = 12.0;
    offset[3] = 12.01; EXPECT(refused(go(spec, fields, outs, ann.data(), MOD16_HOST), "offset holds")); offset[3] = 0.0;
    EXPECT(refused(call<float>(ctx, &spec, fields, nullptr, noon.data(), offset.data(), outs, ann.data(), MOD16_HOST, 0), "needs half_day, noon and offset"));
    s = spec; s.mode = MOD16_DAYNIGHT_SW; s.threshold = std::nan("");
    EXPECT(refused(go(s, fields, outs, ann.data(), MOD16_HOST), "threshold must be finite"));
    // an output on an input, two outputs on each other, temp_annual on an output
    {
        void* on_in[kOutputs] = {};
        on_in[3] = t.data();
        EXPECT(refused(go(spec, fields, on_in, nullptr, MOD16_HOST), "overlaps"));
        void* twice[kOutputs] = {};
        twice[3] = o0.data();
        twice[2] = o0.data() + 8 * W;
        s = spec; s.days = 1;
        EXPECT(refused(go(s, fields, twice, nullptr, MOD16_HOST), "overlaps"));
        EXPECT(refused(go(spec, fields, outs, o1.data() + 16, MOD16_HOST), "overlaps"));
        EXPECT(refused(go(spec, fields, outs, o0.data(), MOD16_DEVICE), "overlaps"));
    }
    s = spec; s.days = 0; EXPECT(go(s, fields, outs, ann.data(), MOD16_HOST) == MOD16_OK);
    s = spec; s.rows = 0; s.in_plane = s.out_plane = 0; EXPECT(go(s, fields, outs, ann.data(), MOD16_HOST) == MOD16_OK);
    s = spec; s.cols = 0; EXPECT(go(s, fields, outs, ann.data(), MOD16_DEVICE) == MOD16_OK);
    check_written(o0, D, R * W, R, W, W, 8, false, "out[3] of the refused calls");
    check_written(o1, D, R * W, R, W, W, 8, false, "out[2] of the refused calls");
    check_written(ann, 1, R * W, R, W, W, 8, false, "temp_annual of the refused calls");
    EXPECT(t.guards_intact() && sw.guards_intact());
    printf("host_asan_daynight: refusals done\n");
}

int main() {
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    run<float>(ctx, MOD16_DAYNIGHT_F32, "float32 -> float32");
    run<float>(ctx, MOD16_DAYNIGHT_F64, "float32 -> float64");
    run<double>(ctx, MOD16_DAYNIGHT_F32, "float64 -> float32");
    run<double>(ctx, MOD16_DAYNIGHT_F64, "float64 -> float64");
    refusals(ctx);
    harness_finish(ctx);
    return 0;
}
