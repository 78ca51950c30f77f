// libmod16hip.so -- the downscaled forward run: mod16_downscale_create / _create_tables / _create_rows / _create_rows_tables / _destroy (the geometry of a fine raster over a coarse grid), mod16_et_downscaled_* (ET with coarse drivers interpolated per pixel inside the kernel), mod16_downscale_fields_* (the interpolated fields alone)
#include "downscale_grid.hpp"

namespace {
constexpr int64_t kDsMaxExtent = int64_t(1) << 30;
enum { kDsScalar = 0, kDsFine = 1, kDsCoarse = 2 };

struct DsAxis {
    std::vector<int32_t> i0, i1;
    std::vector<double> w0, w1;
};

// downscale.corner_tables, formula for formula -> false: a position that is not finite
bool ds_axis_tables(const double* pos, int64_t count, int64_t size, bool wrap, int method, DsAxis& t) {
    t.i0.resize(count); t.i1.resize(count); t.w0.resize(count); t.w1.resize(count);
    const double sz = (double)size;
    for (int64_t k = 0; k < count; ++k) {
        if (!std::isfinite(pos[k])) return false;
        double p;
        int64_t a, b;
        if (wrap) {
            p = pos[k] - std::floor(pos[k] / sz) * sz;
            if (p >= sz || p < 0.0) p = 0.0;
            a = (int64_t)std::floor(p);
            b = (a + 1) % size;
        } else {
            p = std::min(std::max(pos[k], 0.0), (double)(size - 1));
            a = (int64_t)std::floor(p);
            b = std::min(a + 1, size - 1);
        }
        const double f = p - (double)a;
        double w1;
        if (method == MOD16_DOWNSCALE_NEAREST) w1 = f >= 0.5 ? 1.0 : 0.0;
        else if (method == MOD16_DOWNSCALE_BILINEAR) w1 = f;
        else {
            const double half_pi = 3.141592653589793 / 2;
            const double ca = std::pow(std::cos(half_pi * f), 4.0);
            const double cb = std::pow(std::cos(half_pi * (1.0 - f)), 4.0);
            w1 = f == 0.0 ? 0.0 : cb / (ca + cb);        // (cos(pi/2) is 6e-17 in float64, not 0)
        }
        t.i0[k] = (int32_t)a;
        t.i1[k] = (int32_t)b;
        t.w1[k] = w1;
        t.w0[k] = 1.0 - w1;
    }
    return true;
}

const char* ds_check_spec(const mod16_downscale_spec* s) {
    if (!s) return "NULL spec";
    if (s->rows < 1 || s->rows > kDsMaxExtent || s->cols < 1 || s->cols > kDsMaxExtent)
        return "rows and cols must be between 1 and 2^30";
    if (s->coarse_rows < 1 || s->coarse_rows > kDsMaxExtent || s->coarse_cols < 1 || s->coarse_cols > kDsMaxExtent)
        return "coarse_rows and coarse_cols must be between 1 and 2^30";
    if (s->wrap_cols != 0 && s->wrap_cols != 1) return "wrap_cols must be 0 or 1";
    if (s->method != MOD16_DOWNSCALE_NEAREST && s->method != MOD16_DOWNSCALE_BILINEAR && s->method != MOD16_DOWNSCALE_COS4)
        return "unknown method";
    return nullptr;
}

// every index inside its axis, every weight finite: what the kernels rely on
bool ds_tables_valid(const int32_t* i0, const int32_t* i1, const double* w0, const double* w1, int64_t count, int64_t size) {
    for (int64_t k = 0; k < count; ++k)
        if (i0[k] < 0 || i0[k] >= size || i1[k] < 0 || i1[k] >= size || !std::isfinite(w0[k]) || !std::isfinite(w1[k]))
            return false;
    return true;
}
}  // namespace

extern "C" int mod16_downscale_destroy(mod16_downscale* grid) {
    if (!grid) return MOD16_OK;
    (void)hipSetDevice(grid->device);
    delete grid;
    return MOD16_OK;
}

// validated host tables -> a handle with their device copies
static int ds_build(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* const* ri, const double* const* rw,
                    const int32_t* const* ci, const double* const* cw, mod16_downscale** out) {
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_create: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    const int64_t R = spec->rows, C = spec->cols;
    if (!ds_tables_valid(ri[0], ri[1], rw[0], rw[1], R, spec->coarse_rows))
        return bad("a row table holds an index outside the coarse grid or a weight that is not finite");
    if (!ds_tables_valid(ci[0], ci[1], cw[0], cw[1], C, spec->coarse_cols))
        return bad("a column table holds an index outside the coarse grid or a weight that is not finite");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_downscale* g = new (std::nothrow) mod16_downscale;
    if (!g) return MOD16_ERR_NOMEM;
    g->device = ctx->device;
    g->spec = *spec;
    const size_t ib = align256((size_t)R * sizeof(int32_t)), wb = align256((size_t)R * sizeof(double));
    const size_t jb = align256((size_t)C * sizeof(int32_t)), vb = align256((size_t)C * sizeof(double));
    int rc = g->tables.alloc(ctx, 2 * (ib + wb + jb + vb), "mod16_downscale_create: device memory for the corner tables");
    if (rc == MOD16_OK) {
        char* base = g->tables.as<char>();
        char* at[8] = {base, base + ib, base + 2 * ib, base + 2 * ib + wb,
                       base + 2 * (ib + wb), base + 2 * (ib + wb) + jb, base + 2 * (ib + wb + jb), base + 2 * (ib + wb + jb) + vb};
        const void* src[8] = {ri[0], ri[1], rw[0], rw[1], ci[0], ci[1], cw[0], cw[1]};
        const size_t bytes[8] = {(size_t)R * 4, (size_t)R * 4, (size_t)R * 8, (size_t)R * 8,
                                 (size_t)C * 4, (size_t)C * 4, (size_t)C * 8, (size_t)C * 8};
        for (int k = 0; k < 8 && rc == MOD16_OK; ++k)
            if (hipMemcpy(at[k], src[k], bytes[k], hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ctx, MOD16_ERR_HIP, "mod16_downscale_create: upload of the corner tables failed");
        g->g.ri0 = reinterpret_cast<const int32_t*>(at[0]);
        g->g.ri1 = reinterpret_cast<const int32_t*>(at[1]);
        g->g.rw0 = reinterpret_cast<const double*>(at[2]);
        g->g.rw1 = reinterpret_cast<const double*>(at[3]);
        g->g.ci0 = reinterpret_cast<const int32_t*>(at[4]);
        g->g.ci1 = reinterpret_cast<const int32_t*>(at[5]);
        g->g.cw0 = reinterpret_cast<const double*>(at[6]);
        g->g.cw1 = reinterpret_cast<const double*>(at[7]);
        g->g.cols = (int32_t)C;
    }
    if (rc != MOD16_OK) {
        mod16_downscale_destroy(g);
        return rc;
    }
    *out = g;
    return MOD16_OK;
}

extern "C" int mod16_downscale_create(mod16_ctx* ctx, const mod16_downscale_spec* spec, const double* row_pos,
                                      const double* col_pos, mod16_downscale** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_create: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!row_pos || !col_pos || !out) return bad("NULL argument");
    if (const char* what = ds_check_spec(spec)) return bad(what);
    DsAxis r, c;
    if (!ds_axis_tables(row_pos, spec->rows, spec->coarse_rows, false, spec->method, r)) return bad("row_pos holds a value that is not finite");
    if (!ds_axis_tables(col_pos, spec->cols, spec->coarse_cols, spec->wrap_cols != 0, spec->method, c))
        return bad("col_pos holds a value that is not finite");
    const int32_t* ri[2] = {r.i0.data(), r.i1.data()};
    const double* rw[2] = {r.w0.data(), r.w1.data()};
    const int32_t* ci[2] = {c.i0.data(), c.i1.data()};
    const double* cw[2] = {c.w0.data(), c.w1.data()};
    return ds_build(ctx, spec, ri, rw, ci, cw, out);
}

extern "C" int mod16_downscale_create_tables(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* row_i0,
                                             const int32_t* row_i1, const double* row_w0, const double* row_w1,
                                             const int32_t* col_i0, const int32_t* col_i1, const double* col_w0,
                                             const double* col_w1, mod16_downscale** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    if (!row_i0 || !row_i1 || !row_w0 || !row_w1 || !col_i0 || !col_i1 || !col_w0 || !col_w1 || !out)
        return fail(ctx, MOD16_ERR_ARG, "mod16_downscale_create: NULL argument");
    if (const char* what = ds_check_spec(spec)) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_create: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    }
    const int32_t* ri[2] = {row_i0, row_i1};
    const double* rw[2] = {row_w0, row_w1};
    const int32_t* ci[2] = {col_i0, col_i1};
    const double* cw[2] = {col_w0, col_w1};
    return ds_build(ctx, spec, ri, rw, ci, cw, out);
}

// The row-affine geometry: validated row tables and per-row (origin, scale) -> a handle with their
// device copies. Every check runs before any device work.
static int ds_build_rows(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* const* ri, const double* const* rw,
                         const double* origin, const double* scale, mod16_downscale** out) {
#pragma clang fp contract(off)
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_create: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    const int64_t R = spec->rows, C = spec->cols;
    if (!ds_tables_valid(ri[0], ri[1], rw[0], rw[1], R, spec->coarse_rows))
        return bad("a row table holds an index outside the coarse grid or a weight that is not finite");
    const double far = (double)(C - 1);
    for (int64_t r = 0; r < R; ++r) {
        if (!std::isfinite(origin[r])) return bad("col_origin holds a value that is not finite");
        if (!std::isfinite(scale[r])) return bad("col_scale holds a value that is not finite");
        const double step = scale[r] * far;
        const double end = origin[r] + step;
        if (!std::isfinite(end)) return bad("col_origin + col_scale * (cols - 1) is not finite in some row");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_downscale* g = new (std::nothrow) mod16_downscale;
    if (!g) return MOD16_ERR_NOMEM;
    g->device = ctx->device;
    g->spec = *spec;
    g->affine = true;
    const size_t ib = align256((size_t)R * sizeof(int32_t)), wb = align256((size_t)R * sizeof(double));
    int rc = g->tables.alloc(ctx, 2 * ib + 4 * wb, "mod16_downscale_create: device memory for the corner tables");
    if (rc == MOD16_OK) {
        char* base = g->tables.as<char>();
        char* at[6] = {base, base + ib, base + 2 * ib, base + 2 * ib + wb, base + 2 * ib + 2 * wb, base + 2 * ib + 3 * wb};
        const void* src[6] = {ri[0], ri[1], rw[0], rw[1], origin, scale};
        const size_t bytes[6] = {(size_t)R * 4, (size_t)R * 4, (size_t)R * 8, (size_t)R * 8, (size_t)R * 8, (size_t)R * 8};
        for (int k = 0; k < 6 && rc == MOD16_OK; ++k)
            if (hipMemcpy(at[k], src[k], bytes[k], hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ctx, MOD16_ERR_HIP, "mod16_downscale_create: upload of the corner tables failed");
        g->gr.ri0 = reinterpret_cast<const int32_t*>(at[0]);
        g->gr.ri1 = reinterpret_cast<const int32_t*>(at[1]);
        g->gr.rw0 = reinterpret_cast<const double*>(at[2]);
        g->gr.rw1 = reinterpret_cast<const double*>(at[3]);
        g->gr.origin = reinterpret_cast<const double*>(at[4]);
        g->gr.scale = reinterpret_cast<const double*>(at[5]);
        g->gr.cols = (int32_t)C;
        g->gr.width = (int32_t)spec->coarse_cols;
        g->gr.wrap = spec->wrap_cols != 0;
        g->gr.nearest = spec->method == MOD16_DOWNSCALE_NEAREST;
    }
    if (rc != MOD16_OK) {
        mod16_downscale_destroy(g);
        return rc;
    }
    *out = g;
    return MOD16_OK;
}

// the spec of a row-affine grid: as ds_check_spec, and no 'cos4' (its weights need a cosine; the
// device forms this geometry's column weights with multiply, add, divide, floor and compare)
static const char* ds_check_spec_rows(const mod16_downscale_spec* s) {
    if (const char* what = ds_check_spec(s)) return what;
    if (s->method == MOD16_DOWNSCALE_COS4)
        return "MOD16_DOWNSCALE_COS4 is not available with row-affine columns (MOD16_DOWNSCALE_NEAREST or MOD16_DOWNSCALE_BILINEAR)";
    return nullptr;
}

extern "C" int mod16_downscale_create_rows(mod16_ctx* ctx, const mod16_downscale_spec* spec, const double* row_pos,
                                           const double* col_origin, const double* col_scale, mod16_downscale** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_create: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!row_pos || !col_origin || !col_scale || !out) return bad("NULL argument");
    if (const char* what = ds_check_spec_rows(spec)) return bad(what);
    DsAxis r;
    if (!ds_axis_tables(row_pos, spec->rows, spec->coarse_rows, false, spec->method, r)) return bad("row_pos holds a value that is not finite");
    const int32_t* ri[2] = {r.i0.data(), r.i1.data()};
    const double* rw[2] = {r.w0.data(), r.w1.data()};
    return ds_build_rows(ctx, spec, ri, rw, col_origin, col_scale, out);
}

extern "C" int mod16_downscale_create_rows_tables(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* row_i0,
                                                  const int32_t* row_i1, const double* row_w0, const double* row_w1,
                                                  const double* col_origin, const double* col_scale,
                                                  mod16_downscale** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    if (!row_i0 || !row_i1 || !row_w0 || !row_w1 || !col_origin || !col_scale || !out)
        return fail(ctx, MOD16_ERR_ARG, "mod16_downscale_create: NULL argument");
    if (const char* what = ds_check_spec_rows(spec)) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_create: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    }
    const int32_t* ri[2] = {row_i0, row_i1};
    const double* rw[2] = {row_w0, row_w1};
    return ds_build_rows(ctx, spec, ri, rw, col_origin, col_scale, out);
}

static int ds_grid_size(const mod16_ctx* ctx, int64_t n) {
    const int64_t nbatch = (n + kBlock - 1) / kBlock;
    return (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t)ctx->cus * 8));
}

// the kernels of one geometry (G: DsGrid or DsRowsGrid)
template <typename T, typename G>
static void launch_downscaled_on(const DsArgs<T, G>& a, int blocks, unsigned flags, hipStream_t st) {
    if (flags & MOD16_MATH_EXACT) hipLaunchKernelGGL((ds_kernel<T, false, G>), dim3(blocks), dim3(kBlock), 0, st, a);
    else {
        hipLaunchKernelGGL((ds_kernel<T, true, G>), dim3(blocks), dim3(kBlock), 0, st, a);
        // pixels outside the domain of the fast arithmetic: the kernel above left a mark in their
        // out_night, this one computes them in the reference's operation order
        hipLaunchKernelGGL((ds_redo_kernel<T, G>), dim3(blocks), dim3(kBlock), 0, st, a);
    }
}

// All pointers are device pointers here. The handle's geometry picks the instances.
template <typename T>
static int launch_downscaled(mod16_ctx* ctx, const mod16_downscale* grid, DsArgs<T> a, unsigned flags, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    a.lut64 = ctx->lut64.as<double>();
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    const int blocks = ds_grid_size(ctx, a.n);
    if (grid->affine) launch_downscaled_on<T, DsRowsGrid>(ds_with_grid<T, DsRowsGrid>(a, grid->gr), blocks, flags, st);
    else launch_downscaled_on<T, DsGrid>(ds_with_grid<T, DsGrid>(a, grid->g), blocks, flags, st);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

template <typename T>
static int launch_fields(mod16_ctx* ctx, const mod16_downscale* grid, DsFieldArgs<T> a, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    const int blocks = ds_grid_size(ctx, a.n);
    if (grid->affine) {
        DsFieldArgs<T, DsRowsGrid> b;
        memset(&b, 0, sizeof b);
        for (int f = 0; f < kDsMaxFields; ++f) b.field[f] = a.field[f];
        b.out = a.out;
        b.nfields = a.nfields;
        b.g = grid->gr;
        b.cpitch = a.cpitch;
        b.first = a.first;
        b.n = a.n;
        b.out_pitch = a.out_pitch;
        hipLaunchKernelGGL((ds_fields_kernel<T, DsRowsGrid>), dim3(blocks), dim3(kBlock), 0, st, b);
    } else {
        a.g = grid->g;
        hipLaunchKernelGGL((ds_fields_kernel<T>), dim3(blocks), dim3(kBlock), 0, st, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: `count` coarse planes of the call uploaded whole, once, rows back to back (pitch =
// coarse_cols), into the context's buffer for resident inputs; dev[k] receives their addresses
template <typename T>
static int ds_upload_planes(mod16_ctx* ctx, const mod16_downscale* grid, const T* const* host, int count, int64_t cpitch,
                            const T** dev) {
    const size_t H = (size_t)grid->spec.coarse_rows, W = (size_t)grid->spec.coarse_cols;
    const size_t plane = align256(H * W * sizeof(T));
    int rc = ctx->bc_buf.reserve(ctx, 256 + plane * (size_t)count, "HOST mode: device memory for the coarse planes");
    if (rc != MOD16_OK) return rc;
    char* cur = ctx->bc_buf.as<char>();
    for (int k = 0; k < count; ++k) {
        dev[k] = nullptr;
        if (!host[k]) continue;
        // (one copy where the rows lie back to back, else one per row: a plane has a few hundred)
        const size_t rows = (size_t)cpitch == W ? 1 : H, row_bytes = ((size_t)cpitch == W ? H : 1) * W * sizeof(T);
        for (size_t r = 0; r < rows; ++r)
            if (hipMemcpy(cur + r * W * sizeof(T), host[k] + r * (size_t)cpitch, row_bytes, hipMemcpyHostToDevice) != hipSuccess)
                return fail(ctx, MOD16_ERR_HIP, "HOST mode: upload of a coarse plane failed");
        dev[k] = reinterpret_cast<const T*>(cur);
        cur += plane;
    }
    return MOD16_OK;
}

// HOST mode of the run: the coarse planes resident, the fine arrays, the class raster and the two
// outputs tile by tile through the shared staging path; HostTile::off gives a tile's first pixel
template <typename T>
static int downscaled_host(mod16_ctx* ctx, const mod16_downscale* grid, const DsArgs<T>& h, unsigned flags) {
    const T* planes[14];
    const T* dev[14];
    for (int k = 0; k < 14; ++k) planes[k] = ((h.coarse >> k) & 1u) ? h.drv[k] : nullptr;
    int rc = ds_upload_planes<T>(ctx, grid, planes, 14, h.cpitch, dev);
    if (rc != MOD16_OK) return rc;
    HostPlan p(sizeof(T));
    for (int k = 0; k < 14; ++k) {
        const bool coarse = (h.coarse >> k) & 1u;
        p.add(coarse ? kResident : ((h.dense >> k) & 1u) ? kIn : kScalar, h.drv[k]);
        if (coarse) p.a[k].dev = const_cast<T*>(dev[k]);
    }
    p.add(kOut, h.out_day);
    p.add(kOut, h.out_night);
    p.add(kIn, h.cls, true);
    p.cls = h.cls;
    auto launch = [&](const HostTile& t) {
        DsArgs<T> d = h;
        d.n = t.m;
        d.first = h.first + t.off;
        d.cpitch = grid->spec.coarse_cols;
        for (int k = 0; k < 14; ++k) d.drv[k] = static_cast<const T*>(t.dev[k]);
        d.out_day = static_cast<T*>(t.dev[14]);
        d.out_night = static_cast<T*>(t.dev[15]);
        d.cls = static_cast<const uint8_t*>(t.dev[16]);
        return launch_downscaled<T>(ctx, grid, d, flags, t.st);
    };
    // (pipeline = false: these kernels use none of the stream pipeline's workspace; the status word --
    // a class code >= 13 -- is read back here)
    rc = host_tiled(ctx, p, h.n, ctx->host_threads, false, launch);
    return rc == MOD16_OK ? read_status(ctx, ctx->streams[0]) : rc;
}

template <typename T>
static int downscaled_entry(mod16_ctx* ctx, const mod16_downscale* grid, const uint8_t* cls, const T* const* drivers,
                            const int32_t* kinds, int64_t coarse_pitch, int64_t first_pixel, int64_t n, T* out_day,
                            T* out_night, unsigned flags, int where, void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_et_downscaled: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!grid || !cls || !drivers || !kinds || !out_day || !out_night) return bad("NULL grid, class raster, drivers, kinds or outputs");
    if (flags & MOD16_MATH_MIXED)
        return bad("MOD16_MATH_MIXED is not available for the downscaled run (MOD16_MATH_FAST or MOD16_MATH_EXACT)");
    if (flags & MOD16_DOMAIN_TRUSTED)
        return bad("MOD16_DOMAIN_TRUSTED is not available for the downscaled run (every launch is guarded)");
    if (flags & ~(unsigned)MOD16_MATH_EXACT) return bad("unknown flag");
    if (where != MOD16_DEVICE && where != MOD16_HOST) return bad("`where` must be MOD16_HOST or MOD16_DEVICE");
    if (grid->device != ctx->device) return bad("the grid was created on another device than this context's");
    const int64_t total = grid->spec.rows * grid->spec.cols;
    if (n < 0 || first_pixel < 0 || first_pixel > total || n > total - first_pixel)
        return bad("the pixel range [first_pixel, first_pixel + n) leaves the raster");
    DsArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return bad("NULL driver array");
        if (kinds[k] != kDsScalar && kinds[k] != kDsFine && kinds[k] != kDsCoarse) return bad("a driver's kind must be 0 (scalar), 1 (fine) or 2 (coarse)");
        a.drv[k] = drivers[k];
        if (kinds[k] == kDsFine) a.dense |= 1u << k;
        if (kinds[k] == kDsCoarse) a.coarse |= 1u << k;
    }
    if (a.coarse && coarse_pitch < grid->spec.coarse_cols) return bad("coarse_pitch must be at least coarse_cols");
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, "mod16_et_downscaled: mod16_set_bplut_f64 was not called");
    if (n == 0) return MOD16_OK;
    a.cpitch = coarse_pitch;
    a.first = first_pixel;
    a.n = n;
    a.cls = cls;
    a.out_day = out_day;
    a.out_night = out_night;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_downscaled<T>(ctx, grid, a, flags, static_cast<hipStream_t>(stream));
    return downscaled_host<T>(ctx, grid, a, flags);
}

extern "C" int mod16_et_downscaled_f64(mod16_ctx* ctx, const mod16_downscale* grid, const uint8_t* cls,
                                       const double* const* drivers, const int32_t* kinds, int64_t coarse_pitch,
                                       int64_t first_pixel, int64_t n, double* out_day, double* out_night,
                                       unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return downscaled_entry<double>(ctx, grid, cls, drivers, kinds, coarse_pitch, first_pixel, n, out_day, out_night,
                                    flags, where, stream);
}
extern "C" int mod16_et_downscaled_f32(mod16_ctx* ctx, const mod16_downscale* grid, const uint8_t* cls,
                                       const float* const* drivers, const int32_t* kinds, int64_t coarse_pitch,
                                       int64_t first_pixel, int64_t n, float* out_day, float* out_night,
                                       unsigned flags, int where, void* stream) {
    MOD16_LOCK(ctx);
    return downscaled_entry<float>(ctx, grid, cls, drivers, kinds, coarse_pitch, first_pixel, n, out_day, out_night,
                                   flags, where, stream);
}

// HOST mode of the fields: the planes resident, the F output rows tile by tile
template <typename T>
static int fields_host(mod16_ctx* ctx, const mod16_downscale* grid, const DsFieldArgs<T>& h, const T* const* fields) {
    const T* dev[kDsMaxFields];
    int rc = ds_upload_planes<T>(ctx, grid, fields, h.nfields, h.cpitch, dev);
    if (rc != MOD16_OK) return rc;
    HostPlan p(sizeof(T));
    p.add(kOut, h.out, false, h.nfields, h.out_pitch);
    // a slot's slab holds the F rows of a tile: cut the tile so that it stays within 32 MiB
    int64_t tile = ((int64_t)32 << 20) / ((int64_t)h.nfields * (int64_t)sizeof(T)) / kBlock * kBlock;
    tile = std::max<int64_t>(kBlock, std::min<int64_t>(tile, kTilePixels));
    auto launch = [&](const HostTile& t) {
        DsFieldArgs<T> d = h;
        d.n = t.m;
        d.first = h.first + t.off;
        d.cpitch = grid->spec.coarse_cols;
        for (int f = 0; f < h.nfields; ++f) d.field[f] = dev[f];
        d.out = static_cast<T*>(t.dev[0]);
        d.out_pitch = (int64_t)(t.row_bytes / sizeof(T));
        return launch_fields<T>(ctx, grid, d, t.st);
    };
    return host_tiled(ctx, p, h.n, ctx->host_threads, false, launch, nullptr, tile);
}

template <typename T>
static int fields_entry(mod16_ctx* ctx, const mod16_downscale* grid, const T* const* fields, int nfields,
                        int64_t coarse_pitch, int64_t first_pixel, int64_t n, T* out, int64_t out_pitch, int where,
                        void* stream) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) {
        char msg[200];
        snprintf(msg, sizeof msg, "mod16_downscale_fields: %s", what);
        return fail(ctx, MOD16_ERR_ARG, msg);
    };
    if (!grid || !fields || !out) return bad("NULL grid, fields or out");
    if (nfields < 1 || nfields > kDsMaxFields) return bad("F must be between 1 and 16");
    if (where != MOD16_DEVICE && where != MOD16_HOST) return bad("`where` must be MOD16_HOST or MOD16_DEVICE");
    if (grid->device != ctx->device) return bad("the grid was created on another device than this context's");
    const int64_t total = grid->spec.rows * grid->spec.cols;
    if (n < 0 || first_pixel < 0 || first_pixel > total || n > total - first_pixel)
        return bad("the pixel range [first_pixel, first_pixel + n) leaves the raster");
    if (coarse_pitch < grid->spec.coarse_cols) return bad("coarse_pitch must be at least coarse_cols");
    if (out_pitch < n) return bad("out_pitch must be at least n");
    DsFieldArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int f = 0; f < nfields; ++f) {
        if (!fields[f]) return bad("NULL field");
        a.field[f] = fields[f];
    }
    if (n == 0) return MOD16_OK;
    a.out = out;
    a.nfields = nfields;
    a.cpitch = coarse_pitch;
    a.first = first_pixel;
    a.n = n;
    a.out_pitch = out_pitch;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_fields<T>(ctx, grid, a, static_cast<hipStream_t>(stream));
    return fields_host<T>(ctx, grid, a, fields);
}

extern "C" int mod16_downscale_fields_f64(mod16_ctx* ctx, const mod16_downscale* grid, const double* const* fields,
                                          int nfields, int64_t coarse_pitch, int64_t first_pixel, int64_t n,
                                          double* out, int64_t out_pitch, int where, void* stream) {
    MOD16_LOCK(ctx);
    return fields_entry<double>(ctx, grid, fields, nfields, coarse_pitch, first_pixel, n, out, out_pitch, where, stream);
}
extern "C" int mod16_downscale_fields_f32(mod16_ctx* ctx, const mod16_downscale* grid, const float* const* fields,
                                          int nfields, int64_t coarse_pitch, int64_t first_pixel, int64_t n,
                                          float* out, int64_t out_pitch, int where, void* stream) {
    MOD16_LOCK(ctx);
    return fields_entry<float>(ctx, grid, fields, nfields, coarse_pitch, first_pixel, n, out, out_pitch, where, stream);
}
