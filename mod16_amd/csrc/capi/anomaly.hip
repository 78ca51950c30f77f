// libmod16hip.so -- per-pixel climatology, standardized anomalies and percentile ranks over a record of composites: mod16_anomaly_f32 / _f64 (the windowed value or ratio of every slab, the mean, standard deviation and valid count of every period over the baseline years, z and the mid-rank percentile of every slab in one launch), mod16_anomaly_max_window
#include "host.hpp"
#include "../mod16_anomaly.hpp"

namespace {
constexpr int64_t kAnomalyMaxPixels = int64_t(1) << 30;
constexpr int64_t kAnomalyFill = 4096;        // blocks that fill the device: P is cut into chunks up to here
}  // namespace

// All pointers are device pointers here.
template <typename IN>
static int launch_anomaly(mod16_ctx* ctx, AnomalyArgs a, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    constexpr int LANES = kAnomalyLanes;
    const unsigned lds = (unsigned)anomaly_lds_bytes(a.years);        // years <= 64: at most 64 KiB
    a.pixel_blocks = (a.n + LANES - 1) / LANES;                       // n <= 2^30: at most 2^23
    // the periods of a block: all of them once the pixels alone fill the device (a period's window then
    // re-reads what the same lane read a period earlier), fewer for a small raster
    const int64_t chunks = std::min<int64_t>(a.periods, (kAnomalyFill + a.pixel_blocks - 1) / a.pixel_blocks);
    a.chunk = (int)((a.periods + chunks - 1) / chunks);
    const int64_t blocks = a.pixel_blocks * ((a.periods + a.chunk - 1) / a.chunk);   // below 2^23 + 4096
    if (a.den)
        hipLaunchKernelGGL((anomaly_kernel<IN, true>), dim3((unsigned)blocks), dim3(LANES), lds, st, a);
    else
        hipLaunchKernelGGL((anomaly_kernel<IN, false>), dim3((unsigned)blocks), dim3(LANES), lds, st, a);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: ranges of pixels through the shared staging path -- all S rows of a range for num, den, z
// and pct (IN in a float64-sized place), P rows for mean and std, P byte rows for the counts; the tile
// cut so that a slot's slab fits stage_bytes.
template <typename IN>
static int anomaly_host(mod16_ctx* ctx, const AnomalyArgs& a, int64_t stage_bytes) {
    const int S = a.years * a.periods, P = a.periods;
    HostPlan p((int)sizeof(double));
    p.add(kIn, a.num, false, S, a.in_stride, (int)sizeof(IN));
    p.add(kIn, a.den, false, S, a.in_stride, (int)sizeof(IN));
    p.add(kOut, a.z, false, S, a.out_stride, (int)sizeof(IN));
    p.add(kOut, a.pct, false, S, a.out_stride, (int)sizeof(IN));
    p.add(kOut, a.mean, false, P, a.clim_stride);
    p.add(kOut, a.std, false, P, a.clim_stride);
    p.add(kOut, a.count, true, P, a.clim_stride);
    auto launch = [&](const HostTile& t) {
        AnomalyArgs d = a;
        d.n = t.m;
        d.num = t.dev[0];
        d.den = t.dev[1];
        d.z = t.dev[2];
        d.pct = t.dev[3];
        d.mean = static_cast<double*>(t.dev[4]);
        d.std = static_cast<double*>(t.dev[5]);
        d.count = static_cast<uint8_t*>(t.dev[6]);
        d.in_stride = d.out_stride = (int64_t)(t.row_bytes / sizeof(IN));
        d.clim_stride = (int64_t)(t.row_bytes / sizeof(double));
        d.count_stride = (int64_t)t.byte_row_bytes;
        return launch_anomaly<IN>(ctx, d, t.st);
    };
    return host_tiled(ctx, p, a.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(double), stage_bytes));
}

template <typename IN>
static int anomaly_entry(mod16_ctx* ctx, const mod16_anomaly_spec* spec, const IN* num, const IN* den, IN* z, IN* pct,
                         double* mean, double* sdev, uint8_t* count, int where, void* stream, size_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_anomaly: ", what); };
    if (!spec || !num) return bad("NULL spec or num");
    if (!z && !pct && !mean && !sdev && !count) return bad("no output is requested");
    if (spec->n < 0 || spec->n > kAnomalyMaxPixels) return bad("n must be between 0 and 2^30");
    if (spec->periods < 1 || spec->periods > kAnomalyMaxPeriods) return bad("periods must be between 1 and 366");
    if (spec->years < 2 || spec->years > kAnomalyMaxYears) return bad("years must be between 2 and 64");
    if (spec->years * spec->periods > kAnomalyMaxSlabs) return bad("years * periods must be at most 4096");
    if (spec->window < 1 || spec->window > std::min<int>(spec->periods, kAnomalyMaxWindow))
        return bad("window must be between 1 and min(periods, 16)");
    if (spec->base_first < 0 || spec->base_first >= spec->base_end || spec->base_end > spec->years)
        return bad("the baseline must satisfy 0 <= base_first < base_end <= years");
    if (spec->base_end - spec->base_first < 2) return bad("the baseline needs at least 2 years");
    if (spec->min_valid < 2 || spec->min_valid > spec->base_end - spec->base_first)
        return bad("min_valid must be between 2 and the baseline length");
    if (spec->in_stride < spec->n) return bad("in_stride must be at least n");
    if ((z || pct) && spec->out_stride < spec->n) return bad("out_stride must be at least n");
    if ((mean || sdev || count) && spec->clim_stride < spec->n) return bad("clim_stride must be at least n");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int64_t n = spec->n;
    if (n == 0) return MOD16_OK;
    const int S = spec->years * spec->periods, P = spec->periods;
    // no output may share a byte with an input or with another output
    {
        Extent ins[2], outs[5];
        int ni = 0, no = 0;
        ins[ni++] = extent(num, 1, 0, S, spec->in_stride, n, sizeof(IN));
        if (den) ins[ni++] = extent(den, 1, 0, S, spec->in_stride, n, sizeof(IN));
        if (z) outs[no++] = extent(z, 1, 0, S, spec->out_stride, n, sizeof(IN));
        if (pct) outs[no++] = extent(pct, 1, 0, S, spec->out_stride, n, sizeof(IN));
        if (mean) outs[no++] = extent(mean, 1, 0, P, spec->clim_stride, n, 8);
        if (sdev) outs[no++] = extent(sdev, 1, 0, P, spec->clim_stride, n, 8);
        if (count) outs[no++] = extent(count, 1, 0, P, spec->clim_stride, n, 1);
        if (overlaps(outs, no, ins, ni)) return bad("an output overlaps an input or another output");
    }
    AnomalyArgs a;
    memset(&a, 0, sizeof a);
    a.num = num;
    a.den = den;
    a.z = z;
    a.pct = pct;
    a.mean = mean;
    a.std = sdev;
    a.count = count;
    a.n = n;
    a.in_stride = spec->in_stride;
    a.out_stride = spec->out_stride;
    a.clim_stride = a.count_stride = spec->clim_stride;
    a.years = spec->years;
    a.periods = P;
    a.window = spec->window;
    a.base_first = spec->base_first;
    a.base_end = spec->base_end;
    a.min_valid = spec->min_valid;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_anomaly<IN>(ctx, a, static_cast<hipStream_t>(stream));
    return anomaly_host<IN>(ctx, a, stage_budget(stage_bytes));
}

extern "C" int mod16_anomaly_max_window(void) { return kAnomalyMaxWindow; }

extern "C" int mod16_anomaly_f32(mod16_ctx* ctx, const mod16_anomaly_spec* spec, const float* num, const float* den, float* z,
                                 float* pct, double* mean, double* sdev, uint8_t* count, int where, void* stream,
                                 size_t stage_bytes) {
    MOD16_LOCK(ctx);
    return anomaly_entry<float>(ctx, spec, num, den, z, pct, mean, sdev, count, where, stream, stage_bytes);
}
extern "C" int mod16_anomaly_f64(mod16_ctx* ctx, const mod16_anomaly_spec* spec, const double* num, const double* den, double* z,
                                 double* pct, double* mean, double* sdev, uint8_t* count, int where, void* stream,
                                 size_t stage_bytes) {
    MOD16_LOCK(ctx);
    return anomaly_entry<double>(ctx, spec, num, den, z, pct, mean, sdev, count, where, stream, stage_bytes);
}
