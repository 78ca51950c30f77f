// libmod16hip.so -- the vectorised calibration path (N2): mod16_et_static_*, mod16_et_static_batch_*, mod16_static_batch_*
#include "batch.hpp"
#include "host.hpp"

// ------------------------------------------- vectorised calibration path (N2)
// HOST-mode workspace of the calibration entry points, kept in the context between calls (a
// calibration loop repeats the same shape thousands of times): it only grows; above kBatchKeepBytes
// it is given back after the call.
constexpr size_t kBatchKeepBytes = size_t(8) << 30;
static const char kBatchWhat[] = "mod16_et_static*: device memory for the calibration workspace";
static void batch_trim(mod16_ctx* ctx) {
    if (ctx->batch_buf.bytes() > kBatchKeepBytes) ctx->batch_buf.release();
}

// The 14 drivers (dense [n], or one element each) from host memory into slots 0 .. 13 of `per_arr`
// bytes at `base`, on `st`; dev[k]: where driver k went. The first copy that fails is returned.
template <typename T, typename P>
static hipError_t upload_drivers(const T* const* drv, uint32_t dense, int64_t n, void* base, size_t per_arr, hipStream_t st, P* dev) {
    for (int k = 0; k < 14; ++k) {
        T* dp = reinterpret_cast<T*>(static_cast<char*>(base) + per_arr * k);
        dev[k] = dp;
        hipError_t e = hipMemcpyAsync(dp, drv[k], sizeof(T) * (((dense >> k) & 1u) ? n : 1), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
static int static_entry(mod16_ctx* ctx, const T* const* drivers, const int64_t* dstride,
                        const T* const* params, const int64_t* pstride, const T* const* rcorr,
                        const int64_t* rstride, int64_t n, T* out_day, T* out_night, T tiny,
                        int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    if (!drivers || !dstride || !params || !pstride || !out_day || !out_night || n < 0)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_static: bad argument");
    StaticArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static: NULL driver");
        a.drv[k] = drivers[k];
        if (dstride[k]) a.dense_drv |= 1u << k;
    }
    for (int k = 0; k < 11; ++k) {
        if (!params[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static: NULL parameter");
        a.par[k] = params[k];
        if (pstride[k]) a.dense_par |= 1u << k;
    }
    if (rcorr) {
        if (!rcorr[0] || !rcorr[1] || !rstride) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static: r_corr_list needs two arrays");
        for (int k = 0; k < 2; ++k) {
            a.rc[k] = rcorr[k];
            if (rstride[k]) a.dense_rc |= 1u << k;
        }
    }
    a.out[0] = out_day;
    a.out[1] = out_night;
    a.n = n;
    a.tiny = tiny;
    if (n == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->static_flag) {
        int rc = ctx->static_flag.alloc(ctx, sizeof(unsigned), "mod16_et_static: device memory for the flag word");
        if (rc != MOD16_OK) return rc;
    }
    a.flag = ctx->static_flag.as<unsigned>();
    const int grid = batch_blocks(ctx, n);
    // the flag word cleared, any(g_surf > 0) over the whole array, then the pixels
    auto enqueue = [&](const StaticArgs<T>& d, hipStream_t st) -> hipError_t {
        hipError_t e = hipMemsetAsync(d.flag, 0, sizeof(unsigned), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((static_flag_kernel<T>), dim3(grid), dim3(kBlock), 0, st, d);
        hipLaunchKernelGGL((static_kernel<T>), dim3(grid), dim3(kBlock), 0, st, d);
        return hipSuccess;
    };
    if (where == MOD16_DEVICE) {
        HIPCHK(ctx, enqueue(a, static_cast<hipStream_t>(stream)));
        HIPCHK(ctx, hipGetLastError());
        return MOD16_OK;
    }
    if (where != MOD16_HOST) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static: bad `where`");
    constexpr int kArr = 14 + 11 + 2 + 2;
    if (n <= ctx->small_pixels) {
        // what a sampler calls once per draw (a few sites x a year): no allocation, no copy commands --
        // the two kernels read the page-locked buffer and write their outputs there
        HostPlan p(sizeof(T));
        for (int k = 0; k < 14; ++k) p.add(((a.dense_drv >> k) & 1u) ? kIn : kScalar, a.drv[k]);
        for (int k = 0; k < 11; ++k) p.add(((a.dense_par >> k) & 1u) ? kIn : kScalar, a.par[k]);
        for (int k = 0; k < 2; ++k) p.add(((a.dense_rc >> k) & 1u) ? kIn : kScalar, a.rc[k]);   // (absent: NULL)
        for (int k = 0; k < 2; ++k) p.add(kOut, a.out[k]);
        const int rc = host_small(ctx, p, n, false, [&](const HostTile& t) {
            StaticArgs<T> d = a;
            for (int k = 0; k < 14; ++k) d.drv[k] = static_cast<const T*>(t.dev[k]);
            for (int k = 0; k < 11; ++k) d.par[k] = static_cast<const T*>(t.dev[14 + k]);
            for (int k = 0; k < 2; ++k) d.rc[k] = static_cast<const T*>(t.dev[25 + k]);
            for (int k = 0; k < 2; ++k) d.out[k] = static_cast<T*>(t.dev[27 + k]);
            HIPCHK(ctx, enqueue(d, t.st));
            return MOD16_OK;
        });
        if (rc != kSmallUnavailable) return rc;
    }
    // HOST: the whole-array branch needs every pixel before any output, so the
    // inputs are made resident once (calibration-sized arrays, not rasters)
    const size_t per_arr = align256((size_t)n * sizeof(T));
    // the workspace the context keeps between calibration calls (mod16_et_static_batch_* shares it;
    // until round 5 this entry point allocated and freed its own on every call)
    int rcw = ctx->batch_buf.reserve(ctx, per_arr * kArr, kBatchWhat);
    if (rcw != MOD16_OK) return rcw;
    HIPCHK(ctx, ctx->streams[0].ensure());
    hipStream_t st = ctx->streams[0];
    char* base = ctx->batch_buf.as<char>();
    StaticArgs<T> d = a;
    int slot = 14;
    int rc_status = upload_drivers(a.drv, a.dense_drv, n, base, per_arr, st, d.drv) == hipSuccess ? MOD16_OK : MOD16_ERR_HIP;
    auto up = [&](const T* src, bool dense) -> const T* {
        T* dp = reinterpret_cast<T*>(base + per_arr * slot++);
        hipError_t e = hipMemcpyAsync(dp, src, sizeof(T) * (dense ? n : 1), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) rc_status = MOD16_ERR_HIP;
        return dp;
    };
    for (int k = 0; k < 11; ++k) d.par[k] = up(a.par[k], (a.dense_par >> k) & 1u);
    for (int k = 0; k < 2; ++k) d.rc[k] = a.rc[k] ? up(a.rc[k], (a.dense_rc >> k) & 1u) : nullptr;
    slot = 27;
    d.out[0] = reinterpret_cast<T*>(base + per_arr * slot++);
    d.out[1] = reinterpret_cast<T*>(base + per_arr * slot++);
    if (rc_status == MOD16_OK) {
        if (enqueue(d, st) != hipSuccess || hipGetLastError() != hipSuccess) rc_status = MOD16_ERR_HIP;
        if (hipMemcpyAsync(out_day, d.out[0], sizeof(T) * n, hipMemcpyDeviceToHost, st) != hipSuccess) rc_status = MOD16_ERR_HIP;
        if (hipMemcpyAsync(out_night, d.out[1], sizeof(T) * n, hipMemcpyDeviceToHost, st) != hipSuccess) rc_status = MOD16_ERR_HIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc_status = MOD16_ERR_HIP;
    batch_trim(ctx);
    if (rc_status != MOD16_OK) ctx->err = "mod16_et_static: HIP call failed";
    return rc_status;
}

extern "C" int mod16_et_static_f64(mod16_ctx* ctx, const double* const* drivers,
                                   const int64_t* dstride, const double* const* params,
                                   const int64_t* pstride, const double* const* rcorr,
                                   const int64_t* rstride, int64_t n, double* out_day,
                                   double* out_night, double tiny, int where, void* stream) {
    MOD16_LOCK(ctx);
    return static_entry<double>(ctx, drivers, dstride, params, pstride, rcorr, rstride, n, out_day, out_night, tiny, where, stream);
}
extern "C" int mod16_et_static_f32(mod16_ctx* ctx, const float* const* drivers,
                                   const int64_t* dstride, const float* const* params,
                                   const int64_t* pstride, const float* const* rcorr,
                                   const int64_t* rstride, int64_t n, float* out_day,
                                   float* out_night, float tiny, int where, void* stream) {
    MOD16_LOCK(ctx);
    return static_entry<float>(ctx, drivers, dstride, params, pstride, rcorr, rstride, n, out_day, out_night, tiny, where, stream);
}

// ---------------------- calibration path batched over parameter vectors (N2)
__global__ void zero_u32_kernel(unsigned* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// The device-side pass of the batched calibration path over device pointers: d.drv / d.params /
// d.out are set; rows [ndraw][n] into d.out, and with dsse the objective from d.out[2]. FAST: the
// pixels outside the domain of the strength-reduced arithmetic (dskip, [n] bytes of workspace) are
// left out by the FAST kernels and computed in the reference's operation order behind them.
template <typename T>
static int static_batch_rows(mod16_ctx* ctx, StaticBatchArgs<T> d, int64_t ndraw, const T* dobs, const T* dw,
                             double* dsse, double* dcnt, unsigned* dflags, uint8_t* dskip, unsigned flags,
                             hipStream_t st, bool skip_ready = false) {
    const int64_t n = d.n;
    d.flags = dflags;
    d.tab = ctx->tab64.as<double>();
    d.ndraw = ndraw;
    const bool fast = (flags & MOD16_MATH_EXACT) == 0;
    d.skip = fast ? dskip : nullptr;
    hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)((ndraw + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dflags, ndraw);
    const int gx = batch_blocks(ctx, n);
    if (fast && !skip_ready)
        hipLaunchKernelGGL((static_domain_kernel<T>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d, dskip);
    for (int64_t d0 = 0; d0 < ndraw; d0 += 32768 * (int64_t)kBatchDraws) {
        const unsigned gy = (unsigned)((std::min<int64_t>(32768 * (int64_t)kBatchDraws, ndraw - d0) + kBatchDraws - 1) / kBatchDraws);
        d.draw0 = d0;
        if (fast) {
            hipLaunchKernelGGL((static_batch_flag_fast_kernel<T>), dim3(gx, gy), dim3(kBlock), 0, st, d);
            hipLaunchKernelGGL((static_batch_flag_skipped_kernel<T>), dim3(gx, gy), dim3(kBlock), 0, st, d);
            hipLaunchKernelGGL((static_batch_fast_kernel<T>), dim3(gx, gy), dim3(kBlock), 0, st, d);
            hipLaunchKernelGGL((static_batch_redo_rows_kernel<T>), dim3(gx, gy), dim3(kBlock), 0, st, d);
        } else {
            hipLaunchKernelGGL((static_batch_flag_kernel<T>), dim3(gx, gy), dim3(kBlock), 0, st, d);
            hipLaunchKernelGGL((static_batch_kernel<T>), dim3(gx, gy), dim3(kBlock), 0, st, d);
        }
    }
    if (dsse)
        hipLaunchKernelGGL((static_batch_sse_kernel<T>), dim3((unsigned)ndraw), dim3(kBlock), 0, st,
                           d.out[2], dobs, dw, n, dsse, dcnt);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

template <typename T>
static int static_batch_entry(mod16_ctx* ctx, const T* const* drivers, const int64_t* dstride,
                              int64_t n, const T* params, int64_t ndraw, T* out_day, T* out_night,
                              T* out_total, const T* observed, const T* weights, double* sse,
                              double* count, unsigned flags, int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    if (!drivers || !dstride || !params || n < 0 || ndraw < 0)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: bad argument");
    if (!out_day && !out_night && !out_total && !sse)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: no output requested");
    if ((sse != nullptr) != (count != nullptr) || (sse && !observed))
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: sse needs count and observed");
    if (where == MOD16_DEVICE && sse && !out_total)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: sse on device pointers needs out_total as workspace");
    StaticBatchArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: NULL driver");
        if (dstride[k] != 0 && dstride[k] != 1) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: driver stride must be 0 or 1");
        a.drv[k] = drivers[k];
        if (dstride[k]) a.dense_drv |= 1u << k;
    }
    a.n = n;
    if (n == 0 || ndraw == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ndraw > 0x7fffffff) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: too many draws");
    if (where == MOD16_DEVICE) {
        hipStream_t st = static_cast<hipStream_t>(stream);
        // flags and the domain mask: per-call allocations freed on the stream (asynchronous)
        AsyncMem dflags(st), dskip(st);
        const char* what = "mod16_et_static_batch: device memory for the flags and the domain mask";
        int rc = dflags.alloc(ctx, sizeof(unsigned) * ndraw, what);
        if (rc == MOD16_OK) rc = dskip.alloc(ctx, (size_t)n, what);
        if (rc != MOD16_OK) return rc;
        a.params = params;
        a.out[0] = out_day; a.out[1] = out_night; a.out[2] = out_total;
        return static_batch_rows<T>(ctx, a, ndraw, observed, weights, sse, count, static_cast<unsigned*>(dflags.p),
                                    static_cast<uint8_t*>(dskip.p), flags, st);
    }
    if (where != MOD16_HOST) return fail(ctx, MOD16_ERR_ARG, "mod16_et_static_batch: bad `where`");
    // HOST: drivers / parameters resident once, outputs [ndraw][n] come back
    HIPCHK(ctx, ctx->streams[0].ensure());
    hipStream_t st = ctx->streams[0];
    const size_t per_arr = align256((size_t)n * sizeof(T)), per_out = align256((size_t)n * (size_t)ndraw * sizeof(T));
    const bool want[3] = {out_day != nullptr, out_night != nullptr, out_total != nullptr || sse != nullptr};
    T* const host_out[3] = {out_day, out_night, out_total};
    const size_t par_b = (size_t)ndraw * 11 * sizeof(T), red_b = (size_t)ndraw * sizeof(double), flag_b = (size_t)ndraw * sizeof(unsigned);
    const size_t total = per_arr * 16 + align256(par_b) + 2 * align256(red_b) + align256(flag_b) + align256((size_t)n) +
                         per_out * ((int)want[0] + (int)want[1] + (int)want[2]);
    // workspace kept in the context between calls (a calibration loop repeats the same
    // shape thousands of times -- better still: mod16_static_batch_bind_*); it only grows, up to
    // kBatchKeepBytes it is kept
    {
        int rcw = ctx->batch_buf.reserve(ctx, total, kBatchWhat);
        if (rcw != MOD16_OK) return rcw;
    }
    int rc = MOD16_OK;
    auto chk = [&](hipError_t e) { if (e != hipSuccess && rc == MOD16_OK) { rc = MOD16_ERR_HIP; ctx->err = hipGetErrorString(e); } };
    Carver c(ctx->batch_buf.get());
    StaticBatchArgs<T> d = a;
    chk(upload_drivers(a.drv, a.dense_drv, n, c.take<char>(per_arr * 14), per_arr, st, d.drv));
    T* dobs = c.take<T>(per_arr);
    T* dw = c.take<T>(per_arr);
    if (sse) chk(hipMemcpyAsync(dobs, observed, sizeof(T) * n, hipMemcpyHostToDevice, st));
    if (sse && weights) chk(hipMemcpyAsync(dw, weights, sizeof(T) * n, hipMemcpyHostToDevice, st));
    T* dpar = c.take<T>(par_b);
    chk(hipMemcpyAsync(dpar, params, par_b, hipMemcpyHostToDevice, st));
    d.params = dpar;
    double* dsse = c.take<double>(red_b);
    double* dcnt = c.take<double>(red_b);
    unsigned* dflags = c.take<unsigned>(flag_b);
    uint8_t* dskip = c.take<uint8_t>((size_t)n);
    for (int k = 0; k < 3; ++k) d.out[k] = want[k] ? c.take<T>(per_out) : nullptr;
    if (rc == MOD16_OK)
        rc = static_batch_rows<T>(ctx, d, ndraw, dobs, (sse && weights) ? dw : nullptr, sse ? dsse : nullptr, dcnt,
                                  dflags, dskip, flags, st);
    if (rc == MOD16_OK) {
        for (int k = 0; k < 3; ++k)
            if (host_out[k]) chk(hipMemcpyAsync(host_out[k], d.out[k], sizeof(T) * n * ndraw, hipMemcpyDeviceToHost, st));
        if (sse) {
            chk(hipMemcpyAsync(sse, dsse, sizeof(double) * ndraw, hipMemcpyDeviceToHost, st));
            chk(hipMemcpyAsync(count, dcnt, sizeof(double) * ndraw, hipMemcpyDeviceToHost, st));
        }
    }
    chk(hipStreamSynchronize(st));
    batch_trim(ctx);
    return rc;
}

extern "C" int mod16_et_static_batch_f64(mod16_ctx* ctx, const double* const* drivers,
                                         const int64_t* dstride, int64_t n, const double* params,
                                         int64_t ndraw, double* out_day, double* out_night,
                                         double* out_total, const double* observed,
                                         const double* weights, double* sse, double* count,
                                         unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return static_batch_entry<double>(ctx, drivers, dstride, n, params, ndraw, out_day, out_night,
                                      out_total, observed, weights, sse, count, flags, where, stream);
}
extern "C" int mod16_et_static_batch_f32(mod16_ctx* ctx, const float* const* drivers,
                                         const int64_t* dstride, int64_t n, const float* params,
                                         int64_t ndraw, float* out_day, float* out_night,
                                         float* out_total, const float* observed,
                                         const float* weights, double* sse, double* count,
                                         unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return static_batch_entry<float>(ctx, drivers, dstride, n, params, ndraw, out_day, out_night,
                                     out_total, observed, weights, sse, count, flags, where, stream);
}

// the problem's cached objective graphs (plain, fold and constrained)
static void batch_drop_graphs(mod16_batch* b) {
    b->graph.drop();
    b->fgraph.drop();
    b->agraph.drop();
    b->last = nullptr;
}

extern "C" int mod16_static_batch_destroy(mod16_batch* b) {
    if (!b) return MOD16_OK;
    (void)hipSetDevice(b->device);
    if (b->st) (void)hipStreamSynchronize(b->st);
    delete b;
    return MOD16_OK;
}

template <typename T>
static StaticBatchArgs<T> batch_args(const mod16_batch* b) {
    StaticBatchArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) a.drv[k] = static_cast<const T*>(b->drv[k]);
    a.dense_drv = b->dense_drv;
    a.n = b->n;
    a.params = static_cast<const T*>(b->own.params);
    return a;
}

template <typename T>
static int batch_bind(mod16_ctx* ctx, const T* const* drivers, const int64_t* dstride, int64_t n,
                      const T* observed, const T* weights, int64_t max_draws, unsigned flags, int where,
                      mod16_batch** out) {
    if (!ctx || !out) return MOD16_ERR_ARG;
    *out = nullptr;
    // (a launch evaluates 32 draws per block row: 65535 rows at most)
    if (!drivers || !dstride || n <= 0 || max_draws <= 0 || max_draws > (int64_t)65535 * kObjDraws)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_bind: NULL drivers, n <= 0 or max_draws outside 1 .. 2097120");
    if (weights && !observed) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_bind: weights need observed");
    if (where != MOD16_HOST && where != MOD16_DEVICE) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_bind: bad `where`");
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_bind: NULL driver");
        if (dstride[k] != 0 && dstride[k] != 1) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_bind: driver stride must be 0 or 1");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_batch* b = new (std::nothrow) mod16_batch;
    if (!b) return MOD16_ERR_NOMEM;
    b->ctx = ctx;
    b->device = ctx->device;
    b->f32 = std::is_same<T, float>::value;
    b->flags = flags;
    b->n = b->n_user = n;
    b->max_draws = max_draws;
    b->gx = (int)((n + kBlock - 1) / kBlock);
    int rc = [&]() -> int {
        HIPCHK(ctx, b->st.ensure());
        const size_t per_arr = align256((size_t)n * sizeof(T));
        for (int k = 0; k < 14; ++k) if (dstride[k]) b->dense_drv |= 1u << k;
        int r;
        if (where == MOD16_HOST) {
            r = b->owned.alloc(ctx, per_arr * 16, "mod16_static_batch_bind: device memory for the resident drivers");
            if (r != MOD16_OK) return r;
            char* base = b->owned.as<char>();
            HIPCHK(ctx, upload_drivers(drivers, b->dense_drv, n, base, per_arr, b->st, b->drv));
            if (observed) {
                HIPCHK(ctx, hipMemcpyAsync(base + per_arr * 14, observed, sizeof(T) * n, hipMemcpyHostToDevice, b->st));
                b->obs = base + per_arr * 14;
            }
            if (weights) {
                HIPCHK(ctx, hipMemcpyAsync(base + per_arr * 15, weights, sizeof(T) * n, hipMemcpyHostToDevice, b->st));
                b->wts = base + per_arr * 15;
            }
        } else {
            for (int k = 0; k < 14; ++k) b->drv[k] = drivers[k];
            b->obs = observed;
            b->wts = weights;
        }
        // evaluation workspace: the per-draw part for max_draws (the per-block part: batch_eval_ws)
        const int64_t D = max_draws;
        const size_t per_draw = eval_layout_draws(D, sizeof(T), nullptr, nullptr);
        r = b->ws.alloc(ctx, per_draw + align256((size_t)D * sizeof(unsigned)), "mod16_static_batch_bind: device memory for the evaluation workspace");
        if (r != MOD16_OK) return r;
        eval_layout_draws(D, sizeof(T), b->ws.get(), &b->own);
        b->dflags = reinterpret_cast<unsigned*>(b->ws.as<char>() + per_draw);
        const char* pinned = "mod16_static_batch_bind: page-locked memory for the parameters and the results";
        r = b->hparams.alloc(ctx, (size_t)D * 11 * sizeof(T), pinned);
        if (r == MOD16_OK) r = b->hout.alloc(ctx, (size_t)D * 16, pinned);
        // the pixels outside the domain of the FAST arithmetic: marked once, listed in ascending order
        if (r == MOD16_OK) r = b->skip.alloc(ctx, (size_t)n, "mod16_static_batch_bind: device memory for the domain mask");
        if (r != MOD16_OK) return r;
        StaticBatchArgs<T> a = batch_args<T>(b);
        hipLaunchKernelGGL((static_domain_kernel<T>), dim3((unsigned)b->gx), dim3(kBlock), 0, b->st, a, b->skip.as<uint8_t>());
        HIPCHK(ctx, hipGetLastError());
        std::vector<uint8_t> mask((size_t)n);
        HIPCHK(ctx, hipMemcpyAsync(mask.data(), b->skip.get(), (size_t)n, hipMemcpyDeviceToHost, b->st));
        HIPCHK(ctx, hipStreamSynchronize(b->st));
        std::vector<int64_t> list;
        for (int64_t i = 0; i < n; ++i) if (mask[(size_t)i]) list.push_back(i);
        b->nlist = (int64_t)list.size();
        if (b->nlist) {
            r = b->list.alloc(ctx, sizeof(int64_t) * list.size(), "mod16_static_batch_bind: device memory for the list of pixels outside the domain");
            if (r != MOD16_OK) return r;
            HIPCHK(ctx, hipMemcpy(b->list.get(), list.data(), sizeof(int64_t) * list.size(), hipMemcpyHostToDevice));
        }
        return MOD16_OK;
    }();
    if (rc != MOD16_OK) {
        mod16_static_batch_destroy(b);
        return rc;
    }
    *out = b;
    return MOD16_OK;
}

extern "C" int mod16_static_batch_bind_f64(mod16_ctx* ctx, const double* const* drivers, const int64_t* dstride,
                                           int64_t n, const double* observed, const double* weights,
                                           int64_t max_draws, unsigned flags, int where, mod16_batch** out) {
    MOD16_LOCK(ctx);
    return batch_bind<double>(ctx, drivers, dstride, n, observed, weights, max_draws, flags, where, out);
}
extern "C" int mod16_static_batch_bind_f32(mod16_ctx* ctx, const float* const* drivers, const int64_t* dstride,
                                           int64_t n, const float* observed, const float* weights,
                                           int64_t max_draws, unsigned flags, int where, mod16_batch** out) {
    MOD16_LOCK(ctx);
    return batch_bind<float>(ctx, drivers, dstride, n, observed, weights, max_draws, flags, where, out);
}

extern "C" int mod16_static_batch_info(const mod16_batch* b, int64_t* n, int64_t* max_draws, int64_t* n_outside_domain) {
    if (!b) return MOD16_ERR_ARG;
    if (n) *n = b->n_user;
    if (max_draws) *max_draws = b->max_draws;
    if (n_outside_domain) *n_outside_domain = b->nlist;
    return MOD16_OK;
}

// The per-block partials and flags of the FAST objective for `ndraw` draws (grown to the next power
// of two, at most max_draws; a captured graph holds the old addresses: dropped with them).
static int batch_eval_ws(mod16_batch* b, int64_t ndraw) {
    if (ndraw <= b->eval_draws) return MOD16_OK;
    mod16_ctx* ctx = b->ctx;
    int64_t want = 64;
    while (want < ndraw) want *= 2;
    want = std::min(want, b->max_draws);
    batch_drop_graphs(b);
    HIPCHK(ctx, hipStreamSynchronize(b->st));
    b->eval_draws = 0;
    int rc = b->eval_ws.reserve(ctx, eval_layout_blocks(want, b->gx, nullptr, nullptr, b->G != 0),
                                "mod16_static_batch_objective: device memory for the per-block partials of this many draws");
    if (rc != MOD16_OK) return rc;
    eval_layout_blocks(want, b->gx, b->eval_ws.get(), &b->own, b->G != 0);
    b->eval_draws = want;
    return MOD16_OK;
}

// code: NULL (plain draws) or the fold code of every draw (mod16_static_batch_objective_folds, checked);
// penalty: NULL, or where the constraint's penalty of every draw goes (mod16_static_batch_objective_annual)
template <typename T>
static int batch_objective(mod16_batch* b, const T* params, int64_t ndraw, const int32_t* code, double* sse, double* count,
                           double* penalty = nullptr) {
    mod16_ctx* ctx = b->ctx;
    if (!params || !sse || !count || ndraw < 0 || ndraw > b->max_draws)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_objective: NULL argument or more draws than the problem was bound for");
    if (!b->obs) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_objective: the problem was bound without observations");
    if (ndraw == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(b->device));
    memcpy(b->hparams.get(), params, sizeof(T) * (size_t)ndraw * 11);
    HIPCHK(ctx, hipMemcpyAsync(b->own.params, b->hparams.get(), sizeof(T) * (size_t)ndraw * 11, hipMemcpyHostToDevice, b->st));
    if (code) {
        memcpy(b->hcode.get(), code, sizeof(int32_t) * (size_t)ndraw);
        HIPCHK(ctx, hipMemcpyAsync(b->dcode.get(), b->hcode.get(), sizeof(int32_t) * (size_t)ndraw, hipMemcpyHostToDevice, b->st));
    }
    if (b->flags & MOD16_MATH_EXACT) {
        // reference order: rows into a workspace, then the residuals' sums (the kernels of the unbound call)
        int rc = b->rows.reserve(ctx, sizeof(T) * (size_t)ndraw * (size_t)b->n, "mod16_static_batch_objective: device memory for the [ndraw][n] rows");
        if (rc != MOD16_OK) return rc;
        StaticBatchArgs<T> a = batch_args<T>(b);
        a.out[2] = b->rows.as<T>();
        rc = static_batch_rows<T>(ctx, a, ndraw, static_cast<const T*>(b->obs), static_cast<const T*>(b->wts), b->own.sse, b->own.cnt,
                                  b->dflags, b->skip.as<uint8_t>(), b->flags, b->st, true);
        if (rc != MOD16_OK) return rc;
    } else {
        int rc = batch_eval_ws(b, ndraw);
        if (rc != MOD16_OK) return rc;
        CachedGraph& g = penalty ? b->agraph : code ? b->fgraph : b->graph;     // (each kind of call keeps a graph)
        if (g.key != ndraw) {                   // (re)capture: the kernels' arguments hold the number of draws
            if (b->last == &g) b->last = nullptr;
            EvalWs w = b->own;
            w.code = code ? b->dcode.as<int32_t>() : nullptr;
            if (!penalty) w.mass = nullptr;
            rc = g.capture(ctx, b->st, ndraw, [&] { batch_objective_launches<T>(b, w, ndraw); });
            if (rc != MOD16_OK) return rc;
        }
        HIPCHK(ctx, hipGraphLaunch(g.exec, b->st));
        b->last = &g;
    }
    double* hout = b->hout.as<double>();
    HIPCHK(ctx, hipMemcpyAsync(hout, b->own.sse, sizeof(double) * (size_t)ndraw, hipMemcpyDeviceToHost, b->st));
    HIPCHK(ctx, hipMemcpyAsync(hout + b->max_draws, b->own.cnt, sizeof(double) * (size_t)ndraw, hipMemcpyDeviceToHost, b->st));
    if (penalty)
        HIPCHK(ctx, hipMemcpyAsync(hout + 2 * b->max_draws, b->own.penalty, sizeof(double) * (size_t)ndraw, hipMemcpyDeviceToHost, b->st));
    HIPCHK(ctx, hipStreamSynchronize(b->st));
    memcpy(sse, hout, sizeof(double) * (size_t)ndraw);
    memcpy(count, hout + b->max_draws, sizeof(double) * (size_t)ndraw);
    if (penalty) memcpy(penalty, hout + 2 * b->max_draws, sizeof(double) * (size_t)ndraw);
    return MOD16_OK;
}

extern "C" int mod16_static_batch_objective(mod16_batch* b, const void* params, int64_t ndraw, double* sse, double* count) {
    if (!b) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    return b->f32 ? batch_objective<float>(b, static_cast<const float*>(params), ndraw, nullptr, sse, count)
                  : batch_objective<double>(b, static_cast<const double*>(params), ndraw, nullptr, sse, count);
}

// ---- cross-validation: fold labels per pixel, fold codes per draw
extern "C" int mod16_static_batch_set_folds(mod16_batch* b, const uint8_t* labels, int nfolds) {
    if (!b) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    mod16_ctx* ctx = b->ctx;
    if (b->f32 || (b->flags & MOD16_MATH_EXACT) || !b->obs)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: folds need a float64 MOD16_MATH_FAST problem bound with observations");
    if (b->label) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: the problem already has folds");
    if (b->G) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: the problem has the annual-precipitation constraint (not combined with folds)");
    if (b->samplers) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: a sampler exists on the problem");
    if (!labels || nfolds < 2 || nfolds > 255)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: NULL labels or nfolds outside 2 .. 255");
    std::vector<int64_t> seen((size_t)nfolds, 0);
    for (int64_t i = 0; i < b->n; ++i) {
        if (labels[i] >= nfolds) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: a label outside 0 .. nfolds - 1");
        ++seen[labels[i]];
    }
    for (int f = 0; f < nfolds; ++f)
        if (!seen[(size_t)f]) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_folds: a fold without any pixel");
    HIPCHK(ctx, hipSetDevice(b->device));
    // everything new is made first; the problem takes it once nothing can fail any more
    DevMem label, dcode;
    PinnedMem hcode;
    const char* what = "mod16_static_batch_set_folds: memory for the labels and the codes";
    int rc = label.alloc(ctx, (size_t)b->n, what);
    if (rc == MOD16_OK) rc = dcode.alloc(ctx, sizeof(int32_t) * (size_t)b->max_draws, what);
    if (rc == MOD16_OK) rc = hcode.alloc(ctx, sizeof(int32_t) * (size_t)b->max_draws, what);
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(label.get(), labels, (size_t)b->n, hipMemcpyHostToDevice, b->st));
    HIPCHK(ctx, hipStreamSynchronize(b->st));
    b->label = std::move(label);
    b->dcode = std::move(dcode);
    b->hcode = std::move(hcode);
    b->nfolds = nfolds;
    return MOD16_OK;
}

extern "C" int mod16_static_batch_objective_folds(mod16_batch* b, const void* params, int64_t ndraw, const int32_t* code,
                                                  double* sse, double* count) {
    if (!b) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    mod16_ctx* ctx = b->ctx;
    if (!b->label) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_objective_folds: the problem has no folds (mod16_static_batch_set_folds)");
    if (ndraw < 0 || ndraw > b->max_draws || (!code && ndraw > 0))
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_objective_folds: NULL codes or more draws than the problem was bound for");
    for (int64_t d = 0; d < ndraw; ++d)
        if ((code[d] & ~(0xff | MOD16_FOLD_HELDOUT)) || (code[d] & 0xff) >= b->nfolds)
            return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_objective_folds: a code that is not fold | MOD16_FOLD_HELDOUT with fold < nfolds");
    return batch_objective<double>(b, static_cast<const double*>(params), ndraw, code, sse, count);
}

// ---- the annual-precipitation constraint: the problem laid out site-year-major (mod16_methods.hpp,
// above static_annual_redo_kernel), the limits and the scale 86400 / lhv resident
extern "C" int mod16_static_batch_set_annual(mod16_batch* b, int64_t T, int64_t N, const int32_t* year_index, int Y,
                                             const double* annual_precip, const double* lhv) {
    if (!b) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    mod16_ctx* ctx = b->ctx;
    if (b->f32 || (b->flags & MOD16_MATH_EXACT) || !b->obs || !b->owned)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: the constraint needs a float64 MOD16_MATH_FAST problem bound from HOST arrays with observations");
    if (b->G) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: the problem already has the constraint");
    if (b->label) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: the problem has folds (not combined with the constraint)");
    if (b->samplers) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: a sampler exists on the problem");
    const int64_t n = b->n;
    if (!year_index || !annual_precip || !lhv || T < 1 || N < 1 || T > n || N > n || T * N != n)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: NULL argument, or T x N is not the problem's n");
    if (Y < 1 || (int64_t)Y > T || (int64_t)Y * N > (int64_t)1 << 28)
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: Y outside 1 .. T, or more than 2^28 site-years");
    std::vector<int64_t> days((size_t)Y, 0), rank((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        if (year_index[t] < 0 || year_index[t] >= Y)
            return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: a year index outside 0 .. Y - 1");
        rank[(size_t)t] = days[(size_t)year_index[t]]++;
    }
    for (int y = 0; y < Y; ++y)
        if (!days[(size_t)y]) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: a year without any day");
    const int G = (int)(Y * N);
    double S = 0.0;
    for (int g = 0; g < G; ++g) {
        if (!std::isfinite(annual_precip[g])) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: annual_precip must be finite");
        S += annual_precip[g];
    }
    if (!(S > 0.0) || !std::isfinite(S)) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: the sum of annual_precip must be > 0 and finite");
    for (int64_t i = 0; i < n; ++i)
        if (!(lhv[i] > 0.0) || !std::isfinite(lhv[i])) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: lhv must be finite and > 0");
    // the layout: site-year g = y N + s holds its days in order, then copies of its last day up to a
    // multiple of 64 (src < 0: padding, -(pixel + 1))
    std::vector<int64_t> gstart((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) gstart[(size_t)g + 1] = gstart[(size_t)g] + (days[(size_t)(g / N)] + 63) / 64 * 64;
    const int64_t ni = gstart[(size_t)G];
    if (ni / 64 > 0x7fffffff) return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_set_annual: too many pixels");
    std::vector<int64_t> src, pos;
    std::vector<double> in, out;
    std::vector<uint8_t> mask_in, mask;
    std::vector<int64_t> list, lstart((size_t)G + 1, 0);
    std::vector<int32_t> wstart((size_t)G + 1);
    try {
        src.assign((size_t)ni, -1);
        pos.resize((size_t)n);
        in.resize((size_t)n);
        out.resize((size_t)ni);
        mask_in.resize((size_t)n);
        mask.resize((size_t)ni);
    } catch (const std::bad_alloc&) {
        return fail(ctx, MOD16_ERR_NOMEM, "mod16_static_batch_set_annual: host memory for the reordering");
    }
    for (int64_t t = 0; t < T; ++t)
        for (int64_t s = 0; s < N; ++s) {
            const int64_t g = (int64_t)year_index[t] * N + s, k = gstart[(size_t)g] + rank[(size_t)t];
            src[(size_t)k] = t * N + s;
            pos[(size_t)(t * N + s)] = k;
        }
    for (int g = 0; g < G; ++g) {
        const int64_t real = days[(size_t)(g / N)], k0 = gstart[(size_t)g];
        for (int64_t k = k0 + real; k < gstart[(size_t)g + 1]; ++k) src[(size_t)k] = -(src[(size_t)(k0 + real - 1)] + 1);
        wstart[(size_t)g] = (int32_t)(k0 / 64);
    }
    wstart[(size_t)G] = (int32_t)(ni / 64);
    auto from = [&](int64_t k) { const int64_t v = src[(size_t)k]; return (size_t)(v < 0 ? -(v + 1) : v); };
    HIPCHK(ctx, hipSetDevice(b->device));
    HIPCHK(ctx, hipStreamSynchronize(b->st));
    // Build, then commit: everything the constraint adds or replaces is made in `fresh`; a failure
    // returns (and frees it), success moves it into the problem in one place.
    BatchArrays fresh;
    fresh.n = ni;
    fresh.gx = (int)((ni + kBlock - 1) / kBlock);
    fresh.G = G;
    fresh.S = S;
    const size_t per_new = align256((size_t)ni * sizeof(double));
    const int64_t D = b->max_draws;
    const size_t per_draw = eval_layout_draws(D, sizeof(double), nullptr, nullptr, G);
    const char* what = "mod16_static_batch_set_annual: memory for the reordered problem";
    int rc = fresh.owned.alloc(ctx, per_new * 17, what);
    if (rc != MOD16_OK) return rc;
    char* base = fresh.owned.as<char>();
    for (int k = 0; k < 16; ++k) {
        const void* cur = k < 14 ? b->drv[k] : k == 14 ? b->obs : b->wts;
        if (k < 14) fresh.drv[k] = base + per_new * k;
        if (!cur) continue;
        const bool dense = k >= 14 || ((b->dense_drv >> k) & 1u);
        HIPCHK(ctx, hipMemcpy(in.data(), cur, sizeof(double) * (size_t)(dense ? n : 1), hipMemcpyDeviceToHost));
        if (dense)
            for (int64_t j = 0; j < ni; ++j)
                out[(size_t)j] = (k == 14 && src[(size_t)j] < 0) ? std::numeric_limits<double>::quiet_NaN() : in[from(j)];
        else
            out[0] = in[0];
        HIPCHK(ctx, hipMemcpy(base + per_new * k, out.data(), sizeof(double) * (size_t)(dense ? ni : 1), hipMemcpyHostToDevice));
    }
    fresh.obs = base + per_new * 14;
    fresh.wts = b->wts ? base + per_new * 15 : nullptr;
    fresh.scale = reinterpret_cast<const double*>(base + per_new * 16);
    for (int64_t j = 0; j < ni; ++j) out[(size_t)j] = src[(size_t)j] < 0 ? 0.0 : 86400.0 / lhv[from(j)];
    HIPCHK(ctx, hipMemcpy(base + per_new * 16, out.data(), sizeof(double) * (size_t)ni, hipMemcpyHostToDevice));
    // the domain mask goes with its pixels; the list and each site-year's part of it
    HIPCHK(ctx, hipMemcpy(mask_in.data(), b->skip.get(), (size_t)n, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < ni; ++j) {
        mask[(size_t)j] = mask_in[from(j)];
        if (mask[(size_t)j]) list.push_back(j);
    }
    for (int g = 0, u = 0; g <= G; ++g) {
        while ((size_t)u < list.size() && list[(size_t)u] < gstart[(size_t)g]) ++u;
        lstart[(size_t)g] = u;
    }
    fresh.nlist = (int64_t)list.size();
    rc = fresh.skip.alloc(ctx, (size_t)ni, what);
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipMemcpy(fresh.skip.get(), mask.data(), (size_t)ni, hipMemcpyHostToDevice));
    if (!list.empty()) {
        rc = fresh.list.alloc(ctx, sizeof(int64_t) * list.size(), what);
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipMemcpy(fresh.list.get(), list.data(), sizeof(int64_t) * list.size(), hipMemcpyHostToDevice));
    }
    auto carve = [&](void* at) {
        Carver tc(at);
        fresh.wstart = tc.take<int32_t>(sizeof(int32_t) * ((size_t)G + 1));
        fresh.limit = tc.take<double>(sizeof(double) * (size_t)G);
        fresh.lstart = tc.take<int64_t>(sizeof(int64_t) * ((size_t)G + 1));
        fresh.pos = tc.take<int64_t>(sizeof(int64_t) * (size_t)n);
        return tc.used;
    };
    rc = fresh.annual.alloc(ctx, carve(nullptr), what);
    if (rc == MOD16_OK) rc = fresh.ws.alloc(ctx, per_draw + align256((size_t)D * sizeof(unsigned)), what);
    if (rc == MOD16_OK) rc = fresh.hout.alloc(ctx, (size_t)D * 24, what);
    if (rc != MOD16_OK) return rc;
    carve(fresh.annual.get());
    HIPCHK(ctx, hipMemcpy(fresh.wstart, wstart.data(), sizeof(int32_t) * ((size_t)G + 1), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(fresh.limit, annual_precip, sizeof(double) * (size_t)G, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(fresh.lstart, lstart.data(), sizeof(int64_t) * ((size_t)G + 1), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(fresh.pos, pos.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice));
    eval_layout_draws(D, sizeof(double), fresh.ws.get(), &fresh.own, G);
    fresh.dflags = reinterpret_cast<unsigned*>(fresh.ws.as<char>() + per_draw);
    // commit: the graphs and the per-block workspace held the old geometry; the old arrays go with the assignment
    batch_drop_graphs(b);
    b->eval_ws.release();
    b->eval_draws = 0;
    static_cast<BatchArrays&>(*b) = std::move(fresh);
    return MOD16_OK;
}

extern "C" int mod16_static_batch_objective_annual(mod16_batch* b, const void* params, int64_t ndraw, double* sse, double* count,
                                                   double* penalty) {
    if (!b) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    if (!b->G) return fail(b->ctx, MOD16_ERR_ARG, "mod16_static_batch_objective_annual: the problem has no constraint (mod16_static_batch_set_annual)");
    if (!penalty) return fail(b->ctx, MOD16_ERR_ARG, "mod16_static_batch_objective_annual: NULL penalty");
    return batch_objective<double>(b, static_cast<const double*>(params), ndraw, nullptr, sse, count, penalty);
}

// rows [ndraw][n] (host) of the bound problem: the kernels of the unbound call on the resident drivers
template <typename T>
static int batch_rows(mod16_batch* b, const T* params, int64_t ndraw, T* out_day, T* out_night, T* out_total) {
    mod16_ctx* ctx = b->ctx;
    if (!params || ndraw < 0 || ndraw > b->max_draws || (!out_day && !out_night && !out_total))
        return fail(ctx, MOD16_ERR_ARG, "mod16_static_batch_rows: NULL argument, no output or more draws than the problem was bound for");
    if (ndraw == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(b->device));
    T* const host_out[3] = {out_day, out_night, out_total};
    // (a problem laid out site-year-major, b->pos: the rows of the resident pixels, then the caller's gathered from them)
    const size_t per_out = sizeof(T) * (size_t)ndraw * (size_t)b->n, per_user = sizeof(T) * (size_t)ndraw * (size_t)b->n_user;
    int rc = b->rows.reserve(ctx, (align256(per_out) + (b->pos ? align256(per_user) : 0)) *
                                      ((out_day != nullptr) + (out_night != nullptr) + (out_total != nullptr)),
                             "mod16_static_batch_rows: device memory for the [ndraw][n] rows");
    if (rc != MOD16_OK) return rc;
    memcpy(b->hparams.get(), params, sizeof(T) * (size_t)ndraw * 11);
    HIPCHK(ctx, hipMemcpyAsync(b->own.params, b->hparams.get(), sizeof(T) * (size_t)ndraw * 11, hipMemcpyHostToDevice, b->st));
    StaticBatchArgs<T> a = batch_args<T>(b);
    Carver c(b->rows.get());
    for (int k = 0; k < 3; ++k)
        if (host_out[k]) a.out[k] = c.take<T>(per_out);
    rc = static_batch_rows<T>(ctx, a, ndraw, nullptr, nullptr, nullptr, nullptr, b->dflags, b->skip.as<uint8_t>(), b->flags, b->st, true);
    if (rc != MOD16_OK) return rc;
    if (b->pos) {
        const int64_t total = ndraw * b->n_user;
        const unsigned gg = (unsigned)std::min<int64_t>((total + kBlock - 1) / kBlock, (int64_t)b->ctx->cus * 64);
        for (int k = 0; k < 3; ++k)
            if (host_out[k]) {
                T* user = c.take<T>(per_user);
                hipLaunchKernelGGL((static_rows_gather_kernel<T>), dim3(gg), dim3(kBlock), 0, b->st, (const T*)a.out[k], b->pos, b->n,
                                   b->n_user, ndraw, user);
                a.out[k] = user;
            }
        HIPCHK(ctx, hipGetLastError());
    }
    for (int k = 0; k < 3; ++k)
        if (host_out[k]) HIPCHK(ctx, hipMemcpyAsync(host_out[k], a.out[k], per_user, hipMemcpyDeviceToHost, b->st));
    HIPCHK(ctx, hipStreamSynchronize(b->st));
    return MOD16_OK;
}

extern "C" int mod16_static_batch_rows(mod16_batch* b, const void* params, int64_t ndraw, void* out_day, void* out_night,
                                       void* out_total) {
    if (!b) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    return b->f32 ? batch_rows<float>(b, static_cast<const float*>(params), ndraw, static_cast<float*>(out_day),
                                      static_cast<float*>(out_night), static_cast<float*>(out_total))
                  : batch_rows<double>(b, static_cast<const double*>(params), ndraw, static_cast<double*>(out_day),
                                       static_cast<double*>(out_night), static_cast<double*>(out_total));
}

// mean milliseconds of the GPU part of an objective evaluation (replays of the graph of the last
// objective call, plain or fold, on the problem's stream, HIP events): what bench.py puts next to the
// wall-clock rate of the call
extern "C" int mod16_static_batch_time(mod16_batch* b, int launches, float* ms) {
    if (!b || !ms || launches <= 0 || !b->last) return MOD16_ERR_ARG;
    MOD16_LOCK(b->ctx);
    if (hipSetDevice(b->device) != hipSuccess) return MOD16_ERR_HIP;
    EventTimer timer;
    bool ok = timer.start(b->st) == hipSuccess;
    for (int i = 0; i < launches && ok; ++i) ok = hipGraphLaunch(b->last->exec, b->st) == hipSuccess;
    float t = 0.f;
    if (!ok || timer.stop_ms(b->st, &t) != MOD16_OK) return MOD16_ERR_HIP;
    *ms = t / (float)launches;
    return MOD16_OK;
}
