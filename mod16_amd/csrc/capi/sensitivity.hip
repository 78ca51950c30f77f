// libmod16hip.so -- the Sobol sensitivity analysis: mod16_sobol_sample_f64, mod16_sobol_rows_f64,
// mod16_sobol_analyze_f64 (kernels: mod16_sobol.hpp)
#include "internal.hpp"
#include "../mod16_sobol.hpp"

namespace {
constexpr int64_t kSobolMaxN = int64_t(1) << 26;
constexpr int kSobolMaxResamples = 1 << 20;
constexpr int kSobolGramBlocks = 1024;   // target blocks of the Gram kernel (chunks x (resamples + 1))

int sobol_rows_per_sample(int d, int second_order) { return second_order ? 2 * d + 2 : d + 2; }

// the checks shared by the three entry points (MOD16_ERR_ARG with a message, or MOD16_OK)
int sobol_check(mod16_ctx* ctx, const char* fn, int d, int64_t n, int where) {
    char msg[160];
    if (d < 1 || d > kSobolMaxD) {
        snprintf(msg, sizeof msg, "%s: d must be 1 .. %d", fn, kSobolMaxD);
        ctx->err = msg;
        return MOD16_ERR_ARG;
    }
    if (n < 1 || n > kSobolMaxN || (n & (n - 1))) {
        snprintf(msg, sizeof msg, "%s: n must be a power of two, at most 2^26", fn);
        ctx->err = msg;
        return MOD16_ERR_ARG;
    }
    if (where != MOD16_HOST && where != MOD16_DEVICE) {
        snprintf(msg, sizeof msg, "%s: bad `where`", fn);
        ctx->err = msg;
        return MOD16_ERR_ARG;
    }
    return MOD16_OK;
}

int sobol_check_bounds(mod16_ctx* ctx, const char* fn, int d, const double* lo, const double* hi,
                       int64_t n, int64_t skip) {
    char msg[160];
    if (!lo || !hi) {
        snprintf(msg, sizeof msg, "%s: lo and hi are required", fn);
        ctx->err = msg;
        return MOD16_ERR_ARG;
    }
    for (int k = 0; k < d; ++k)
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(lo[k] < hi[k])) {
            snprintf(msg, sizeof msg, "%s: bounds %d: lo < hi, both finite", fn, k);
            ctx->err = msg;
            return MOD16_ERR_ARG;
        }
    if (skip < 0 || skip > (int64_t(1) << 32) - n) {
        snprintf(msg, sizeof msg, "%s: 0 <= skip and skip + n <= 2^32", fn);
        ctx->err = msg;
        return MOD16_ERR_ARG;
    }
    return MOD16_OK;
}

int sobol_grid(int64_t work) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((work + kSobolBlock - 1) / kSobolBlock, int64_t(1) << 20));
}

// runs `launch(device_out, stream)` into the caller's device array (DEVICE) or into a device
// buffer that is copied to the caller's host array behind it (HOST, synchronous)
template <typename F>
int sobol_to(mod16_ctx* ctx, double* out, size_t bytes, int where, void* stream, F launch) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) {
        hipStream_t st = static_cast<hipStream_t>(stream);
        launch(out, st);
        HIPCHK(ctx, hipGetLastError());
        return MOD16_OK;
    }
    HIPCHK(ctx, ctx->streams[0].ensure());
    hipStream_t st = ctx->streams[0];
    DevMem dev;
    int rc = dev.alloc(ctx, bytes, "mod16_sobol: device memory for the output");
    if (rc != MOD16_OK) return rc;
    launch(dev.as<double>(), st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dev.get(), bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    HIPCHK(ctx, e);
    return MOD16_OK;
}
}  // namespace

extern "C" int mod16_sobol_sample_f64(mod16_ctx* ctx, int d, const double* lo, const double* hi,
                                      int64_t n, int64_t skip, int second_order, double* out,
                                      int where, void* stream) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    const char* fn = "mod16_sobol_sample_f64";
    int rc = sobol_check(ctx, fn, d, n, where);
    if (rc == MOD16_OK) rc = sobol_check_bounds(ctx, fn, d, lo, hi, n, skip);
    if (rc != MOD16_OK) return rc;
    if (!out) return fail(ctx, MOD16_ERR_ARG, "mod16_sobol_sample_f64: out is required");
    SobolSampleArgs a;
    for (int k = 0; k < kSobolMaxD; ++k) {
        a.lo[k] = k < d ? lo[k] : 0.0;
        a.hi[k] = k < d ? hi[k] : 1.0;
    }
    a.d = d;
    a.R = sobol_rows_per_sample(d, second_order);
    a.n = n;
    a.skip = (uint64_t)skip;
    const int64_t total = n * a.R * d;
    return sobol_to(ctx, out, sizeof(double) * (size_t)total, where, stream, [&](double* dst, hipStream_t st) {
        a.out = dst;
        hipLaunchKernelGGL(sobol_sample_kernel, dim3(sobol_grid(total)), dim3(kSobolBlock), 0, st, a);
    });
}

extern "C" int mod16_sobol_rows_f64(mod16_ctx* ctx, const double* params, const double* base,
                                    const int* vary, const double* lo, const double* hi, int d,
                                    int64_t n, int64_t skip, int second_order, double* y, int where,
                                    void* stream) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    const char* fn = "mod16_sobol_rows_f64";
    int rc = sobol_check(ctx, fn, d, n, where);
    if (rc == MOD16_OK) rc = sobol_check_bounds(ctx, fn, d, lo, hi, n, skip);
    if (rc != MOD16_OK) return rc;
    if (!params || !base || !vary || !y) return fail(ctx, MOD16_ERR_ARG, "mod16_sobol_rows_f64: params, base, vary and y are required");
    SobolRowsArgs a;
    for (int k = 0; k < 14; ++k) {
        a.slot[k] = -1;
        a.base[k] = base[k];
    }
    for (int s = 0; s < d; ++s) {
        if (vary[s] < 0 || vary[s] >= 14 || a.slot[vary[s]] >= 0)
            return fail(ctx, MOD16_ERR_ARG, "mod16_sobol_rows_f64: vary holds distinct driver indices 0 .. 13");
        a.slot[vary[s]] = s;
    }
    for (int k = 0; k < 11; ++k) a.params[k] = params[k];
    for (int k = 0; k < kSobolMaxD; ++k) {
        a.lo[k] = k < d ? lo[k] : 0.0;
        a.hi[k] = k < d ? hi[k] : 1.0;
    }
    a.d = d;
    a.R = sobol_rows_per_sample(d, second_order);
    a.n = n;
    a.skip = (uint64_t)skip;
    const int64_t total = n * a.R;
    return sobol_to(ctx, y, sizeof(double) * (size_t)total, where, stream, [&](double* dst, hipStream_t st) {
        a.y = dst;
        hipLaunchKernelGGL(sobol_rows_kernel, dim3(sobol_grid(total)), dim3(kSobolBlock), 0, st, a);
    });
}

extern "C" int mod16_sobol_analyze_f64(mod16_ctx* ctx, const double* y, int d, int64_t n,
                                       int second_order, int normalize, int resamples, uint64_t seed,
                                       double* idx_out, double* std_out, int where, void* stream) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    int rc = sobol_check(ctx, "mod16_sobol_analyze_f64", d, n, where);
    if (rc != MOD16_OK) return rc;
    if (!y || !idx_out || !std_out) return fail(ctx, MOD16_ERR_ARG, "mod16_sobol_analyze_f64: y, idx_out and std_out are required");
    if (resamples < 0 || resamples > kSobolMaxResamples)
        return fail(ctx, MOD16_ERR_ARG, "mod16_sobol_analyze_f64: resamples must be 0 .. 2^20");
    SobolAnalyzeArgs a;
    a.n = n;
    a.d = d;
    a.R = sobol_rows_per_sample(d, second_order);
    a.m = 3 + d + (second_order ? d : 0);
    a.nent = a.m * (a.m + 1) / 2;
    a.nidx = 2 * d + d * d;
    a.resamples = resamples;
    a.seed_mixed = sobol_mix(seed);
    // chunks of the draws: about kSobolGramBlocks blocks in all, whatever the device
    const int64_t steps = (n + kSobolGramDraws - 1) / kSobolGramDraws;
    const int64_t want = std::max<int64_t>(1, kSobolGramBlocks / (resamples + 1));
    const int64_t per = (steps + std::min(want, steps) - 1) / std::min(want, steps);
    a.chunk = per * kSobolGramDraws;
    a.nchunks = (int)((n + a.chunk - 1) / a.chunk);

    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (where == MOD16_HOST) {
        HIPCHK(ctx, ctx->streams[0].ensure());
        st = ctx->streams[0];
    }
    // one workspace: [Y (HOST only)] stats | sum partials | Gram partials | indices | outputs
    double* ydev = nullptr;
    auto layout = [&](void* base) {
        Carver c(base);
        if (where == MOD16_HOST) ydev = c.take<double>(sizeof(double) * (size_t)n * a.R);
        a.stats = c.take<double>(sizeof(double) * 4);
        a.sum_partial = c.take<double>(sizeof(double) * kSobolSumBlocks);
        a.gram = c.take<double>(sizeof(double) * (size_t)(resamples + 1) * a.nchunks * a.nent);
        a.idx = c.take<double>(sizeof(double) * (size_t)(resamples + 1) * a.nidx);
        a.out = c.take<double>(sizeof(double) * 2 * a.nidx);
        return c.used;
    };
    AsyncMem ws(st);
    rc = ws.alloc(ctx, layout(nullptr), "mod16_sobol_analyze_f64: device memory for the workspace");
    if (rc != MOD16_OK) return rc;
    layout(ws.p);
    a.y = ydev ? ydev : y;

    hipError_t e = hipSuccess;
    if (ydev) e = hipMemcpyAsync(ydev, y, sizeof(double) * (size_t)n * a.R, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const dim3 blk(kSobolBlock), sums(kSobolSumBlocks), one(1);
        if (normalize) {
            hipLaunchKernelGGL(sobol_sum_kernel<0>, sums, blk, 0, st, a);
            hipLaunchKernelGGL(sobol_stats_kernel<0>, one, blk, 0, st, a);
            hipLaunchKernelGGL(sobol_sum_kernel<2>, sums, blk, 0, st, a);
            hipLaunchKernelGGL(sobol_stats_kernel<2>, one, blk, 0, st, a);
        } else {
            hipLaunchKernelGGL(sobol_sum_kernel<1>, sums, blk, 0, st, a);
            hipLaunchKernelGGL(sobol_stats_kernel<1>, one, blk, 0, st, a);
        }
        hipLaunchKernelGGL(sobol_gram_kernel, dim3(a.nchunks, resamples + 1), blk, 0, st, a);
        hipLaunchKernelGGL(sobol_indices_kernel, dim3(resamples + 1), blk, 0, st, a);
        hipLaunchKernelGGL(sobol_conf_kernel, one, blk, 0, st, a);
        e = hipGetLastError();
    }
    const hipMemcpyKind kind = where == MOD16_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (e == hipSuccess) e = hipMemcpyAsync(idx_out, a.out, sizeof(double) * a.nidx, kind, st);
    if (e == hipSuccess) e = hipMemcpyAsync(std_out, a.out + a.nidx, sizeof(double) * a.nidx, kind, st);
    ws.release();
    if (e == hipSuccess && where == MOD16_HOST) e = hipStreamSynchronize(st);
    HIPCHK(ctx, e);
    return MOD16_OK;
}
