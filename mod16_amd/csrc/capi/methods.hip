// libmod16hip.so -- the class-surface sub-methods (mod16_method_*)
#include "host.hpp"
#include "../mod16_methods.hpp"

// ------------------------------------------------------- class-surface methods
template <typename T>
static int method_entry(mod16_ctx* ctx, int method, const T* const* in, const int64_t* istride,
                        const T* const* params, const int64_t* pstride, int64_t n,
                        T* const* out, T alpha, T tiny, int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    if (method < 0 || method >= MOD16_M_COUNT || !in || !istride || !out || !out[0] || n < 0)
        return fail(ctx, MOD16_ERR_ARG, "mod16_method: bad argument");
    MethodArgs<T> a;
    memset(&a, 0, sizeof a);
    a.method = method;
    a.alpha = alpha;
    a.tiny = tiny;
    a.n = n;
    static const T nan_param = std::numeric_limits<T>::quiet_NaN();
    for (int k = 0; k < kMethodMaxIn; ++k) {
        a.in[k] = in[k];
        if (in[k]) {
            a.present_in |= 1u << k;
            if (istride[k]) a.dense_in |= 1u << k;
        }
    }
    for (int k = 0; k < 11; ++k) {
        a.par[k] = params ? params[k] : nullptr;
        if (a.par[k] && pstride && pstride[k]) a.dense_par |= 1u << k;
    }
    a.out[0] = out[0];
    a.out[1] = out[1];
    if (n == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    auto launch = [&](const MethodArgs<T>& d, hipStream_t st) {
        hipLaunchKernelGGL((method_kernel<T>), dim3(batch_blocks(ctx, d.n)), dim3(kBlock), 0, st, d);
    };
    if (where == MOD16_DEVICE) {
        // absent parameters read as NaN scalars from the ctx scratch
        T hs[11];
        for (int k = 0; k < 11; ++k) hs[k] = nan_param;
        hipStream_t st = static_cast<hipStream_t>(stream);
        bool need = false;
        for (int k = 0; k < 11; ++k) if (!a.par[k]) need = true;
        if (need) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->scalars.get(), hs, sizeof hs, hipMemcpyHostToDevice, st));
            for (int k = 0; k < 11; ++k) if (!a.par[k]) a.par[k] = ctx->scalars.as<const T>() + k;
        }
        launch(a, st);
        HIPCHK(ctx, hipGetLastError());
        return MOD16_OK;
    }
    if (where != MOD16_HOST) return fail(ctx, MOD16_ERR_ARG, "mod16_method: bad `where`");
    // HOST mode: the inputs (absent: NULL), the parameters (absent: NaN scalars), 2 outputs
    HostPlan p(sizeof(T));
    static_assert(sizeof(double) * (kMethodMaxIn + 11) <= 256, "scalars of a method call fit the scalar block");
    for (int k = 0; k < kMethodMaxIn; ++k) p.add(((a.dense_in >> k) & 1u) ? kIn : kScalar, a.in[k]);
    for (int k = 0; k < 11; ++k) p.add(((a.dense_par >> k) & 1u) ? kIn : kScalar, a.par[k] ? a.par[k] : &nan_param);
    for (int k = 0; k < 2; ++k) p.add(kOut, a.out[k]);
    auto launch_tile = [&](const HostTile& t) {
        MethodArgs<T> d = a;
        d.n = t.m;
        for (int k = 0; k < kMethodMaxIn; ++k) d.in[k] = static_cast<const T*>(t.dev[k]);
        for (int k = 0; k < 11; ++k) d.par[k] = static_cast<const T*>(t.dev[kMethodMaxIn + k]);
        for (int k = 0; k < 2; ++k) d.out[k] = static_cast<T*>(t.dev[kMethodMaxIn + 11 + k]);
        launch(d, t.st);
        return MOD16_OK;
    };
    if (n <= ctx->small_pixels) {
        const int rc = host_small(ctx, p, n, false, launch_tile);
        if (rc != kSmallUnavailable) return rc;
    }
    return host_tiled(ctx, p, n, 1, false, launch_tile);     // (one slot: no double buffering)
}

extern "C" int mod16_method_f64(mod16_ctx* ctx, int method, const double* const* in,
                                const int64_t* istride, const double* const* params,
                                const int64_t* pstride, int64_t n, double* const* out,
                                double alpha, double tiny, int where, void* stream) {
    MOD16_LOCK(ctx);
    return method_entry<double>(ctx, method, in, istride, params, pstride, n, out, alpha, tiny, where, stream);
}
extern "C" int mod16_method_f32(mod16_ctx* ctx, int method, const float* const* in,
                                const int64_t* istride, const float* const* params,
                                const int64_t* pstride, int64_t n, float* const* out, float alpha,
                                float tiny, int where, void* stream) {
    MOD16_LOCK(ctx);
    return method_entry<float>(ctx, method, in, istride, params, pstride, n, out, alpha, tiny, where, stream);
}
