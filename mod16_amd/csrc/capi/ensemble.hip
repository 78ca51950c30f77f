// libmod16hip.so -- the ensemble forward run: mod16_ensemble_create / _destroy, mod16_et_ensemble_* (per-pixel mean and spread of ET over D parameter tables), mod16_et_ensemble_members_* (every member's totals), mod16_et_ensemble_quantiles_* (per-pixel quantiles over the members)
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
    const int grid = batch_blocks(ctx, a.n);
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

// ---- per-member outputs and per-pixel quantiles (ABI 11)

// The member kernel (and, behind the fast one, the kernel of the flagged pixels) for a.n pixels.
template <typename T, typename O>
static void launch_members(mod16_ctx* ctx, const mod16_ensemble* ens, EnsMemArgs<T, O> a, unsigned flags, hipStream_t st) {
    a.tables = ens->tables.as<double>();
    a.members = (int)ens->members;
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    const int grid = batch_blocks(ctx, a.n);
    if (flags & MOD16_MATH_EXACT) hipLaunchKernelGGL((ens_members_kernel<T, O, false>), dim3(grid), dim3(kBlock), 0, st, a);
    else {
        hipLaunchKernelGGL((ens_members_kernel<T, O, true>), dim3(grid), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL((ens_members_redo_kernel<T, O>), dim3(grid), dim3(kBlock), 0, st, a);
    }
}

template <typename T, int CAP>
static void launch_select_cap(const EnsSelArgs<T>& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.n + kEnsSelLanes - 1) / kEnsSelLanes);
    hipLaunchKernelGGL((ens_select_kernel<T, CAP>), dim3(grid), dim3(kEnsSelLanes), 0, st, a);
}
// the instance of the smallest capacity (16, 32, 64, 128, 256 members) that holds the ensemble
template <typename T>
static void launch_select(const EnsSelArgs<T>& a, hipStream_t st) {
    if (a.members <= 16) launch_select_cap<T, 16>(a, st);
    else if (a.members <= 32) launch_select_cap<T, 32>(a, st);
    else if (a.members <= 64) launch_select_cap<T, 64>(a, st);
    else if (a.members <= 128) launch_select_cap<T, 128>(a, st);
    else launch_select_cap<T, 256>(a, st);
}

// What the entry point has checked: drivers, class raster, positions, outputs (device pointers, or
// host pointers in front of the staging path).
template <typename T> struct EnsQuantCall {
    EnsMemArgs<T, double> mem;     // drv, cls, n, dense_drv
    EnsSelArgs<T> sel;             // lo, frac, nq, out
    int64_t slab_bytes;
};

// Chunks of P pixels through one slab of members x P x 2 doubles, a stream-ordered temporary of the
// call, reused in stream order: member kernel, redo kernel, selection, next chunk.
template <typename T>
static int launch_quantiles(mod16_ctx* ctx, const mod16_ensemble* ens, const EnsQuantCall<T>& q, unsigned flags, hipStream_t st) {
    const int64_t n = q.mem.n, D = ens->members;
    if (n <= 0) return MOD16_OK;
    int64_t P = std::max<int64_t>(256, q.slab_bytes / (16 * D) / 256 * 256);
    P = std::min(P, (n + 255) / 256 * 256);
    AsyncMem slab(st);
    int rc = slab.alloc(ctx, (size_t)P * D * 16, "mod16_et_ensemble_quantiles: device memory for the slab of member values");
    if (rc != MOD16_OK) return rc;
    double* day = static_cast<double*>(slab.p);
    double* night = day + P * D;
    for (int64_t off = 0; off < n; off += P) {
        EnsMemArgs<T, double> m = q.mem;
        EnsSelArgs<T> s = q.sel;
        m.n = s.n = std::min(P, n - off);
        for (int k = 0; k < 14; ++k)
            if ((m.dense_drv >> k) & 1u) m.drv[k] += off;
        m.cls += off;
        m.day = day;
        m.night = night;
        m.pitch = P;
        s.day = day;
        s.night = night;
        s.pitch = P;
        s.members = (int)D;
        for (int k = 0; k < 3 * s.nq; ++k) s.out[k] += off;
        launch_members<T, double>(ctx, ens, m, flags, st);
        launch_select<T>(s, st);
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: 14 drivers, the 3 nq outputs, the class raster -- through the shared staging path; each
// tile's callback has its own slab on its own stream
template <typename T>
static int quantiles_host(mod16_ctx* ctx, const mod16_ensemble* ens, const EnsQuantCall<T>& h, unsigned flags) {
    const int64_t n = h.mem.n;
    if (n == 0) return MOD16_OK;
    const int nout = 3 * h.sel.nq;
    HostPlan p(sizeof(T));
    for (int k = 0; k < 14; ++k) p.add(((h.mem.dense_drv >> k) & 1u) ? kIn : kScalar, h.mem.drv[k]);
    for (int k = 0; k < nout; ++k) p.add(kOut, h.sel.out[k]);
    p.add(kIn, h.mem.cls, true);
    p.cls = h.mem.cls;
    auto launch = [&](const HostTile& t) {
        EnsQuantCall<T> d = h;
        d.mem.n = t.m;
        for (int k = 0; k < 14; ++k) d.mem.drv[k] = static_cast<const T*>(t.dev[k]);
        for (int k = 0; k < nout; ++k) d.sel.out[k] = static_cast<T*>(t.dev[14 + k]);
        d.mem.cls = static_cast<const uint8_t*>(t.dev[14 + nout]);
        return launch_quantiles<T>(ctx, ens, d, flags, t.st);
    };
    if (n <= ctx->small_pixels) {
        const int rc = host_small(ctx, p, n, false, launch);
        if (rc != kSmallUnavailable) return rc;
    }
    return host_tiled(ctx, p, n, ctx->host_threads, true, launch);
}

// The checks the member and the quantile calls share with the ensemble run; fills drv, cls, n.
template <typename T, typename O>
static int members_args(mod16_ctx* ctx, const char* name, const mod16_ensemble* ens, const uint8_t* cls,
                        const T* const* drivers, const int64_t* dstride, int64_t n, unsigned flags, EnsMemArgs<T, O>& a) {
    char msg[160];
    auto bad = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", name, what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!ens || !cls || !drivers || !dstride || n < 0) return bad("NULL ensemble, class raster, drivers or strides, or n < 0");
    if (flags & MOD16_MATH_MIXED)
        return bad("MOD16_MATH_MIXED is not available for the ensemble run (MOD16_MATH_FAST or MOD16_MATH_EXACT)");
    if (flags & MOD16_DOMAIN_TRUSTED)
        return bad("MOD16_DOMAIN_TRUSTED is not available for the ensemble run (every launch is guarded)");
    if (flags & ~(unsigned)MOD16_MATH_EXACT) return bad("unknown flag");
    if (ens->device != ctx->device) return bad("the ensemble was created on another device than this context's");
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return bad("NULL driver array");
        if (dstride[k] != 0 && dstride[k] != 1) return bad("driver stride must be 0 or 1");
        a.drv[k] = drivers[k];
        if (dstride[k] == 1) a.dense_drv |= 1u << k;
    }
    a.cls = cls;
    a.n = n;
    return MOD16_OK;
}

template <typename T>
static int members_entry(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls, const T* const* drivers,
                         const int64_t* dstride, int64_t n, T* day, T* night, int64_t pitch, unsigned flags, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    EnsMemArgs<T, T> a;
    int rc = members_args<T, T>(ctx, "mod16_et_ensemble_members", ens, cls, drivers, dstride, n, flags, a);
    if (rc != MOD16_OK) return rc;
    if (!day || !night) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_members: both output arrays are required");
    if (pitch < n) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_members: pitch must be at least n");
    if (n == 0) return MOD16_OK;
    a.day = day;
    a.night = night;
    a.pitch = pitch;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    launch_members<T, T>(ctx, ens, a, flags, static_cast<hipStream_t>(stream));
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

template <typename T>
static int quantiles_entry(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls, const T* const* drivers,
                           const int64_t* dstride, int64_t n, const double* q, int nq, T* const* out,
                           int64_t slab_bytes, unsigned flags, int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    EnsQuantCall<T> c;
    memset(&c.sel, 0, sizeof c.sel);
    int rc = members_args<T, double>(ctx, "mod16_et_ensemble_quantiles", ens, cls, drivers, dstride, n, flags, c.mem);
    if (rc != MOD16_OK) return rc;
    if (nq < 1 || nq > kEnsMaxQuantiles) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: nq must be between 1 and 8");
    if (!q || !out) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: NULL q or outputs");
    if (ens->members > kEnsSelMaxMembers)
        return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: more than 256 members");
    if (slab_bytes < 0) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: slab_bytes must not be negative");
    for (int k = 0; k < nq; ++k) {
        if (!(q[k] >= 0.0 && q[k] <= 1.0))
            return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: every q must lie in [0, 1] and not be NaN");
        // mod16_amd.calibration.quantile_positions: one float64 multiply, floor, the remainder
        const double h = q[k] * (double)(ens->members - 1);
        const double lo = std::floor(h);
        c.sel.lo[k] = (int)lo;
        c.sel.frac[k] = h - lo;
    }
    c.sel.nq = nq;
    for (int k = 0; k < 3 * nq; ++k) {
        if (!out[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: all 3 * nq output arrays are required");
        c.sel.out[k] = out[k];
    }
    c.slab_bytes = slab_bytes ? slab_bytes : (int64_t)128 << 20;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_quantiles<T>(ctx, ens, c, flags, static_cast<hipStream_t>(stream));
    if (where == MOD16_HOST) return quantiles_host<T>(ctx, ens, c, flags);
    return fail(ctx, MOD16_ERR_ARG, "mod16_et_ensemble_quantiles: `where` must be MOD16_HOST or MOD16_DEVICE");
}

extern "C" int mod16_et_ensemble_members_f64(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls,
                                             const double* const* drivers, const int64_t* dstride, int64_t n,
                                             double* day, double* night, int64_t pitch, unsigned flags, void* stream) {
    MOD16_LOCK(ctx);
    return members_entry<double>(ctx, ens, cls, drivers, dstride, n, day, night, pitch, flags, stream);
}
extern "C" int mod16_et_ensemble_members_f32(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls,
                                             const float* const* drivers, const int64_t* dstride, int64_t n,
                                             float* day, float* night, int64_t pitch, unsigned flags, void* stream) {
    MOD16_LOCK(ctx);
    return members_entry<float>(ctx, ens, cls, drivers, dstride, n, day, night, pitch, flags, stream);
}
extern "C" int mod16_et_ensemble_quantiles_f64(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls,
                                               const double* const* drivers, const int64_t* dstride, int64_t n,
                                               const double* q, int nq, double* const* out, int64_t slab_bytes,
                                               unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return quantiles_entry<double>(ctx, ens, cls, drivers, dstride, n, q, nq, out, slab_bytes, flags, where, stream);
}
extern "C" int mod16_et_ensemble_quantiles_f32(mod16_ctx* ctx, const mod16_ensemble* ens, const uint8_t* cls,
                                               const float* const* drivers, const int64_t* dstride, int64_t n,
                                               const double* q, int nq, float* const* out, int64_t slab_bytes,
                                               unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return quantiles_entry<float>(ctx, ens, cls, drivers, dstride, n, q, nq, out, slab_bytes, flags, where, stream);
}
