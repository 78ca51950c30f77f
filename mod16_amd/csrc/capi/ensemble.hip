// libmod16hip.so -- the ensemble forward run: mod16_ensemble_create / _destroy, mod16_et_ensemble_* (per-pixel mean and spread of ET over D parameter tables)
#include "host.hpp"
#include "../mod16_ensemble.hpp"

// D parameter tables on the device, each in the layout the kernels index by class code.
struct mod16_ensemble {
    int device = 0;
    int64_t members = 0;
    DevMem tables;               // device double [members][MOD16_LUT_ROWS][kLutCols]
};

extern "C" int mod16_ensemble_destroy(mod16_ensemble* ens) {
    if (!ens) return MOD16_OK;
    (void)hipSetDevice(ens->device);
    delete ens;
    return MOD16_OK;
}

extern "C" int mod16_ensemble_create(mod16_ctx* ctx, const double* tables, int64_t members, mod16_ensemble** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    if (!tables || !out) return fail(ctx, MOD16_ERR_ARG, "mod16_ensemble_create: NULL argument");
    if (members < 1 || members > kEnsMaxMembers)
        return fail(ctx, MOD16_ERR_ARG, "mod16_ensemble_create: members must be between 1 and 65536");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_ensemble* ens = new (std::nothrow) mod16_ensemble;
    if (!ens) return MOD16_ERR_NOMEM;
    ens->device = ctx->device;
    ens->members = members;
    std::vector<double> host((size_t)members * kEnsTable);
    for (int64_t m = 0; m < members; ++m)
        derive_lut(tables + (size_t)m * MOD16_N_CLASSES * MOD16_N_PARAMS, host.data() + (size_t)m * kEnsTable);
    int rc = ens->tables.alloc(ctx, host.size() * sizeof(double), "mod16_ensemble_create: device memory for the members' tables");
    if (rc == MOD16_OK && hipMemcpy(ens->tables.get(), host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(ctx, MOD16_ERR_HIP, "mod16_ensemble_create: upload of the members' tables failed");
    if (rc != MOD16_OK) {
        mod16_ensemble_destroy(ens);
        return rc;
    }
    *out = ens;
    return MOD16_OK;
}

// All pointers are device pointers here (or the page-locked buffer of the small calls).
template <typename T>
static int launch_ensemble(mod16_ctx* ctx, const mod16_ensemble* ens, EnsArgs<T> a, unsigned flags, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    a.tables = ens->tables.as<double>();
    a.members = (int)ens->members;
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    const int64_t nbatch = (a.n + kBlock - 1) / kBlock;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t)ctx->cus * 8));
    if (flags & MOD16_MATH_EXACT) hipLaunchKernelGGL((ens_kernel<T, false>), dim3(grid), dim3(kBlock), 0, st, a);
    else {
        hipLaunchKernelGGL((ens_kernel<T, true>), dim3(grid), dim3(kBlock), 0, st, a);
        // pixels outside the domain of the fast arithmetic: the kernel above left a mark in their
        // std_total, this one computes them in the reference's operation order
        hipLaunchKernelGGL((ens_redo_kernel<T>), dim3(grid), dim3(kBlock), 0, st, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: 14 drivers, the 5 outputs, the class raster -- through the shared staging path
template <typename T>
static int ensemble_host(mod16_ctx* ctx, const mod16_ensemble* ens, const EnsArgs<T>& h, unsigned flags) {
    const int64_t n = h.n;
    if (n == 0) return MOD16_OK;
    HostPlan p(sizeof(T));
    for (int k = 0; k < 14; ++k) p.add(((h.dense_drv >> k) & 1u) ? kIn : kScalar, h.drv[k]);
    for (int k = 0; k < kEnsOut; ++k) p.add(kOut, h.out[k]);
    p.add(kIn, h.cls, true);
    p.cls = h.cls;
    auto launch = [&](const HostTile& t) {
        EnsArgs<T> d = h;
        d.n = t.m;
        for (int k = 0; k < 14; ++k) d.drv[k] = static_cast<const T*>(t.dev[k]);
        for (int k = 0; k < kEnsOut; ++k) d.out[k] = static_cast<T*>(t.dev[14 + k]);
        d.cls = static_cast<const uint8_t*>(t.dev[14 + kEnsOut]);
        return launch_ensemble<T>(ctx, ens, d, flags, t.st);
    };
    if (n <= ctx->small_pixels) {
        const int rc = host_small(ctx, p, n, false, launch);    // (one pixel per thread: no padding to whole vectors)
        if (rc != kSmallUnavailable) return rc;
    }
    return host_tiled(ctx, p, n, ctx->host_threads, true, launch);
}

template <typename T>
static int ensemble_entry(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls, const T* const* drivers,
                          const int64_t* dstride, int64_t n, T* const* out, unsigned flags, int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    if (!ens || !cls || !drivers || !dstride || !out || n < 0)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: NULL ensemble, class raster, drivers, strides or outputs, or n < 0");
    if (flags & MOD16_MATH_MIXED)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: MOD16_MATH_MIXED is not available for the ensemble run (MOD16_MATH_FAST or MOD16_MATH_EXACT)");
    if (flags & MOD16_DOMAIN_TRUSTED)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: MOD16_DOMAIN_TRUSTED is not available for the ensemble run (every launch is guarded)");
    if (flags & ~(unsigned)MOD16_MATH_EXACT) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: unknown flag");
    if (ens->device != ctx->device)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: the ensemble was created on another device than this context's");
    EnsArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: NULL driver array");
        if (dstride[k] != 0 && dstride[k] != 1) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: driver stride must be 0 or 1");
        a.drv[k] = drivers[k];
        if (dstride[k] == 1) a.dense_drv |= 1u << k;
    }
    for (int k = 0; k < kEnsOut; ++k) {
        if (!out[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: all five output arrays are required");
        a.out[k] = out[k];
    }
    a.cls = cls;
    a.n = n;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_ensemble<T>(ctx, ens, a, flags, static_cast<hipStream_t>(stream));
    if (where == MOD16_HOST) return ensemble_host<T>(ctx, ens, a, flags);
    return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble: `where` must be MOD16_HOST or MOD16_DEVICE");
}

extern "C" int mod16_et_ensemble_f64(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls,
                                     const double* const* drivers, const int64_t* dstride, int64_t n,
                                     double* const* out, unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return ensemble_entry<double>(ctx, ens, cls, drivers, dstride, n, out, flags, where, stream);
}
extern "C" int mod16_et_ensemble_f32(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls,
                                     const float* const* drivers, const int64_t* dstride, int64_t n,
                                     float* const* out, unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return ensemble_entry<float>(ctx, ens, cls, drivers, dstride, n, out, flags, where, stream);
}
