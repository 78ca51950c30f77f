// libmod16hip.so -- per-pixel Mann-Kendall / Theil-Sen trends over a stack of composites: mod16_trend_f32 / _f64 (count, S, z, slope, intercept and the slope's interval of every pixel in one launch), mod16_trend_max_steps
#include "host.hpp"
#include "../mod16_trend.hpp"

namespace {
constexpr int64_t kTrendMaxPixels = int64_t(1) << 30;
}  // namespace

// All pointers are device pointers here (the times too).
template <typename IN, int CAP>
static void launch_trend_cap(const TrendArgs& a, hipStream_t st) {
    constexpr int P = kTrendSlots / CAP;      // pixels of a block
    const int64_t blocks = (a.n + P - 1) / P;     // n <= 2^30, P >= 2
    hipLaunchKernelGGL((trend_kernel<IN, CAP>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
}

template <typename IN>
static int launch_trend(mod16_ctx* ctx, const TrendArgs& a, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    switch (trend_capacity(a.steps)) {
        case 16: launch_trend_cap<IN, 16>(a, st); break;
        case 32: launch_trend_cap<IN, 32>(a, st); break;
        case 64: launch_trend_cap<IN, 64>(a, st); break;
        case 128: launch_trend_cap<IN, 128>(a, st); break;
        case 256: launch_trend_cap<IN, 256>(a, st); break;
        case 512: launch_trend_cap<IN, 512>(a, st); break;
        case 1024: launch_trend_cap<IN, 1024>(a, st); break;
        case 2048: launch_trend_cap<IN, 2048>(a, st); break;
        default: return fail(ctx, MOD16_ERR_ARG, "mod16_trend: internal: no kernel for this number of steps");
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: ranges of pixels through the shared staging path -- the five float64 outputs and S (an
// int32 in a float64-sized place), then all `steps` rows of the range's values, the counts as bytes;
// the tile cut so that a slot's slab fits stage_bytes. a.times is the device copy.
template <typename IN>
static int trend_host(mod16_ctx* ctx, const TrendArgs& a, int64_t stage_bytes) {
    HostPlan p((int)sizeof(double));
    for (int o = 0; o < kTrendOutputs; ++o) p.add(kOut, a.out[o]);
    p.add(kOut, a.s, false, 1, 0, (int)sizeof(int32_t));
    p.add(kIn, a.values, false, a.steps, a.time_stride, (int)sizeof(IN));
    p.add(kOut, a.count, true);
    auto launch = [&](const HostTile& t) {
        TrendArgs d = a;
        d.n = t.m;
        for (int o = 0; o < kTrendOutputs; ++o) d.out[o] = static_cast<double*>(t.dev[o]);
        d.s = static_cast<int32_t*>(t.dev[kTrendOutputs]);
        d.values = t.dev[kTrendOutputs + 1];
        d.count = static_cast<uint8_t*>(t.dev[kTrendOutputs + 2]);
        d.time_stride = (int64_t)(t.row_bytes / sizeof(IN));
        return launch_trend<IN>(ctx, d, t.st);
    };
    return host_tiled(ctx, p, a.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(double), stage_bytes));
}

template <typename IN>
static int trend_entry(mod16_ctx* ctx, const mod16_trend_spec* spec, const IN* values, const double* times,
                       double* const* out, int32_t* s, uint8_t* count, int where, void* stream, size_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_trend: ", what); };
    if (!spec || !values || !times) return bad("NULL spec, values or times");
    bool any = s || count;
    for (int o = 0; out && o < kTrendOutputs; ++o) any = any || out[o];
    if (!any) return bad("no output is requested");
    if (spec->n < 0 || spec->n > kTrendMaxPixels) return bad("n must be between 0 and 2^30");
    if (spec->steps < 2 || spec->steps > kTrendMaxSteps) return bad("steps must be between 2 and 64");
    if (spec->time_stride < spec->n) return bad("time_stride must be at least n");
    const int Y = spec->steps;
    for (int y = 0; y < Y; ++y) {
        if (!std::isfinite(times[y])) return bad("times must be finite");
        if (y && !(times[y] > times[y - 1])) return bad("times must be strictly increasing");
    }
    if (!std::isfinite(times[Y - 1] - times[0])) return bad("the span of times must be finite");
    if (spec->min_valid < 2 || spec->min_valid > Y) return bad("min_valid must be between 2 and steps");
    if (!(spec->zq >= 0.0) || !std::isfinite(spec->zq)) return bad("zq must be finite and not negative");
    if (spec->zq == 0.0 && out && (out[kTrendLo] || out[kTrendHi])) return bad("slope_lo and slope_hi need zq > 0");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int64_t n = spec->n;
    if (n == 0) return MOD16_OK;
    // no output may share a byte with the input or with another output
    {
        Extent ins[2], outs[kTrendOutputs + 2];
        int ni = 0, no = 0;
        ins[ni++] = extent(values, 1, 0, Y, spec->time_stride, n, sizeof(IN));
        if (where == MOD16_HOST) ins[ni++] = extent(times, Y, 8);
        for (int o = 0; out && o < kTrendOutputs; ++o)
            if (out[o]) outs[no++] = extent(out[o], n, 8);
        if (s) outs[no++] = extent(s, n, 4);
        if (count) outs[no++] = extent(count, n, 1);
        if (overlaps(outs, no, ins, ni)) return bad("an output overlaps an input or another output");
    }
    TrendArgs a;
    memset(&a, 0, sizeof a);
    a.values = values;
    for (int o = 0; out && o < kTrendOutputs; ++o) a.out[o] = out[o];
    a.s = s;
    a.count = count;
    a.n = n;
    a.time_stride = spec->time_stride;
    a.zq = spec->zq;
    a.steps = Y;
    a.min_valid = spec->min_valid;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool host = where == MOD16_HOST;
    if (host) HIPCHK(ctx, ctx->streams[0].ensure());
    hipStream_t st = host ? (hipStream_t)ctx->streams[0] : static_cast<hipStream_t>(stream);
    // the times as a device copy in stream-ordered memory; HOST mode runs its tiles on several streams: they start behind the upload
    AsyncMem dtimes(st);
    int rc = dtimes.alloc(ctx, (size_t)Y * 8, "mod16_trend: device memory for the times");
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(dtimes.p, times, (size_t)Y * 8, hipMemcpyHostToDevice, st));
    a.times = static_cast<const double*>(dtimes.p);
    if (!host) return launch_trend<IN>(ctx, a, st);
    HIPCHK(ctx, hipStreamSynchronize(st));
    return trend_host<IN>(ctx, a, stage_budget(stage_bytes));
}

extern "C" int mod16_trend_max_steps(void) { return kTrendMaxSteps; }

extern "C" int mod16_trend_f32(mod16_ctx* ctx, const mod16_trend_spec* spec, const float* values, const double* times,
                               double* const* out, int32_t* s, uint8_t* count, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    return trend_entry<float>(ctx, spec, values, times, out, s, count, where, stream, stage_bytes);
}
extern "C" int mod16_trend_f64(mod16_ctx* ctx, const mod16_trend_spec* spec, const double* values, const double* times,
                               double* const* out, int32_t* s, uint8_t* count, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    return trend_entry<double>(ctx, spec, values, times, out, s, count, where, stream, stage_bytes);
}
