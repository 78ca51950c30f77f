// libmod16hip.so -- the downscaled forward run: mod16_downscale_create / _create_tables / _create_rows / _create_rows_tables / _destroy (the geometry of a fine raster over a coarse grid), mod16_et_downscaled_* (ET with coarse drivers interpolated per pixel inside the kernel), mod16_downscale_fields_* (the interpolated fields alone)
#include "downscale_grid.hpp"

namespace {
constexpr int64_t kDsMaxExtent = int64_t(1) << 30;
enum { kDsScalar = 0, kDsFine = 1, kDsCoarse = 2 };

// an axis' corner tables: the caller's, or a DsAxis' own
struct DsTables {
    const int32_t* i0;
    const int32_t* i1;
    const double* w0;
    const double* w1;
};

struct DsAxis {
    std::vector<int32_t> i0, i1;
    std::vector<double> w0, w1;
    DsTables view() const { return DsTables{i0.data(), i1.data(), w0.data(), w1.data()}; }
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

// every index inside its axis, every weight finite: what the kernels rely on
bool ds_tables_valid(const DsTables& t, int64_t count, int64_t size) {
    for (int64_t k = 0; k < count; ++k)
        if (t.i0[k] < 0 || t.i0[k] >= size || t.i1[k] < 0 || t.i1[k] >= size || !std::isfinite(t.w0[k]) || !std::isfinite(t.w1[k]))
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

static int ds_bad(mod16_ctx* ctx, const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_downscale_create: ", what); }

// What every create entry point begins with: *out cleared, its pointer arguments present (`given`),
// the spec. A row-affine grid has no 'cos4' (its weights need a cosine; the device forms this
// geometry's column weights with multiply, add, divide, floor and compare).
static int ds_create_begin(mod16_ctx* ctx, const mod16_downscale_spec* s, bool affine, bool given, mod16_downscale** out) {
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    if (!given || !out) return ds_bad(ctx, "NULL argument");
    if (!s) return ds_bad(ctx, "NULL spec");
    if (s->rows < 1 || s->rows > kDsMaxExtent || s->cols < 1 || s->cols > kDsMaxExtent)
        return ds_bad(ctx, "rows and cols must be between 1 and 2^30");
    if (s->coarse_rows < 1 || s->coarse_rows > kDsMaxExtent || s->coarse_cols < 1 || s->coarse_cols > kDsMaxExtent)
        return ds_bad(ctx, "coarse_rows and coarse_cols must be between 1 and 2^30");
    if (s->wrap_cols != 0 && s->wrap_cols != 1) return ds_bad(ctx, "wrap_cols must be 0 or 1");
    if (s->method != MOD16_DOWNSCALE_NEAREST && s->method != MOD16_DOWNSCALE_BILINEAR && s->method != MOD16_DOWNSCALE_COS4)
        return ds_bad(ctx, "unknown method");
    if (affine && s->method == MOD16_DOWNSCALE_COS4)
        return ds_bad(ctx, "MOD16_DOWNSCALE_COS4 is not available with row-affine columns (MOD16_DOWNSCALE_NEAREST or MOD16_DOWNSCALE_BILINEAR)");
    return MOD16_OK;
}

// The row tables and the columns' geometry -- their tables (cols), or the per-row (origin, scale) of
// row-affine columns (cols NULL) -- validated, then a handle with their device copies. Every check
// runs before any device work.
static int ds_build(mod16_ctx* ctx, const mod16_downscale_spec* spec, const DsTables& rows, const DsTables* cols,
                    const double* origin, const double* scale, mod16_downscale** out) {
    const int64_t R = spec->rows, C = spec->cols;
    if (!ds_tables_valid(rows, R, spec->coarse_rows))
        return ds_bad(ctx, "a row table holds an index outside the coarse grid or a weight that is not finite");
    if (cols) {
        if (!ds_tables_valid(*cols, C, spec->coarse_cols))
            return ds_bad(ctx, "a column table holds an index outside the coarse grid or a weight that is not finite");
    } else {
#pragma clang fp contract(off)
        const double far = (double)(C - 1);
        for (int64_t r = 0; r < R; ++r) {
            if (!std::isfinite(origin[r])) return ds_bad(ctx, "col_origin holds a value that is not finite");
            if (!std::isfinite(scale[r])) return ds_bad(ctx, "col_scale holds a value that is not finite");
            const double step = scale[r] * far;
            const double end = origin[r] + step;
            if (!std::isfinite(end)) return ds_bad(ctx, "col_origin + col_scale * (cols - 1) is not finite in some row");
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_downscale* g = new (std::nothrow) mod16_downscale;
    if (!g) return MOD16_ERR_NOMEM;
    g->device = ctx->device;
    g->spec = *spec;
    g->affine = !cols;
    // The device block: the arrays in this order, each in whole 256-byte lines. Walked once without
    // a block for its size, once with it for the uploads and the views into it.
    struct Piece { const void* src; size_t bytes; };
    const size_t ib = (size_t)R * sizeof(int32_t), wb = (size_t)R * sizeof(double);
    const size_t jb = (size_t)C * sizeof(int32_t), vb = (size_t)C * sizeof(double);
    const Piece tables[8] = {{rows.i0, ib}, {rows.i1, ib}, {rows.w0, wb}, {rows.w1, wb},
                             {cols ? cols->i0 : nullptr, jb}, {cols ? cols->i1 : nullptr, jb},
                             {cols ? cols->w0 : nullptr, vb}, {cols ? cols->w1 : nullptr, vb}};
    const Piece affine[6] = {{rows.i0, ib}, {rows.i1, ib}, {rows.w0, wb}, {rows.w1, wb}, {origin, wb}, {scale, wb}};
    const Piece* pieces = cols ? tables : affine;
    const int count = cols ? 8 : 6;
    Carver size;
    for (int k = 0; k < count; ++k) size.take<char>(pieces[k].bytes);
    int rc = g->tables.alloc(ctx, size.used, "mod16_downscale_create: device memory for the corner tables");
    if (rc == MOD16_OK) {
        Carver block(g->tables.get());
        const char* at[8];
        for (int k = 0; k < count; ++k) {
            at[k] = block.take<char>(pieces[k].bytes);
            if (rc == MOD16_OK && hipMemcpy(const_cast<char*>(at[k]), pieces[k].src, pieces[k].bytes, hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ctx, MOD16_ERR_HIP, "mod16_downscale_create: upload of the corner tables failed");
        }
        auto i32 = [&](int k) { return reinterpret_cast<const int32_t*>(at[k]); };
        auto f64 = [&](int k) { return reinterpret_cast<const double*>(at[k]); };
        if (cols) {
            g->g = DsGrid{i32(0), i32(1), f64(2), f64(3), i32(4), i32(5), f64(6), f64(7), (int32_t)C};
        } else {
            g->gr = DsRowsGrid{i32(0), i32(1), f64(2), f64(3), f64(4), f64(5), (int32_t)C, (int32_t)spec->coarse_cols,
                               spec->wrap_cols != 0, spec->method == MOD16_DOWNSCALE_NEAREST};
        }
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
    if (int rc = ds_create_begin(ctx, spec, false, row_pos && col_pos, out)) return rc;
    DsAxis r, c;
    if (!ds_axis_tables(row_pos, spec->rows, spec->coarse_rows, false, spec->method, r)) return ds_bad(ctx, "row_pos holds a value that is not finite");
    if (!ds_axis_tables(col_pos, spec->cols, spec->coarse_cols, spec->wrap_cols != 0, spec->method, c))
        return ds_bad(ctx, "col_pos holds a value that is not finite");
    const DsTables cols = c.view();
    return ds_build(ctx, spec, r.view(), &cols, nullptr, nullptr, out);
}

extern "C" int mod16_downscale_create_tables(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* row_i0,
                                             const int32_t* row_i1, const double* row_w0, const double* row_w1,
                                             const int32_t* col_i0, const int32_t* col_i1, const double* col_w0,
                                             const double* col_w1, mod16_downscale** out) {
    MOD16_LOCK(ctx);
    const bool given = row_i0 && row_i1 && row_w0 && row_w1 && col_i0 && col_i1 && col_w0 && col_w1;
    if (int rc = ds_create_begin(ctx, spec, false, given, out)) return rc;
    const DsTables cols = {col_i0, col_i1, col_w0, col_w1};
    return ds_build(ctx, spec, DsTables{row_i0, row_i1, row_w0, row_w1}, &cols, nullptr, nullptr, out);
}

extern "C" int mod16_downscale_create_rows(mod16_ctx* ctx, const mod16_downscale_spec* spec, const double* row_pos,
                                           const double* col_origin, const double* col_scale, mod16_downscale** out) {
    MOD16_LOCK(ctx);
    if (int rc = ds_create_begin(ctx, spec, true, row_pos && col_origin && col_scale, out)) return rc;
    DsAxis r;
    if (!ds_axis_tables(row_pos, spec->rows, spec->coarse_rows, false, spec->method, r)) return ds_bad(ctx, "row_pos holds a value that is not finite");
    return ds_build(ctx, spec, r.view(), nullptr, col_origin, col_scale, out);
}

extern "C" int mod16_downscale_create_rows_tables(mod16_ctx* ctx, const mod16_downscale_spec* spec, const int32_t* row_i0,
                                                  const int32_t* row_i1, const double* row_w0, const double* row_w1,
                                                  const double* col_origin, const double* col_scale,
                                                  mod16_downscale** out) {
    MOD16_LOCK(ctx);
    if (int rc = ds_create_begin(ctx, spec, true, row_i0 && row_i1 && row_w0 && row_w1 && col_origin && col_scale, out)) return rc;
    return ds_build(ctx, spec, DsTables{row_i0, row_i1, row_w0, row_w1}, nullptr, col_origin, col_scale, out);
}

// The arguments of a launch of the run with the handle's geometry in place (G: DsGrid or DsRowsGrid).
// DsArgs keeps the geometry between its other members, member by member: with `g` behind them, as in
// DsFieldArgs and CdArgs, ds_redo_kernel<double, DsRowsGrid> takes 193 vector registers for 191.
template <typename T, typename G> static DsArgs<T, G> ds_with_grid(const DsArgs<T>& a, const G& g) {
    DsArgs<T, G> b;
    memset(&b, 0, sizeof b);
    for (int k = 0; k < 14; ++k) b.drv[k] = a.drv[k];
    b.dense = a.dense;
    b.coarse = a.coarse;
    b.g = g;
    b.cpitch = a.cpitch;
    b.first = a.first;
    b.n = a.n;
    b.cls = a.cls;
    b.lut64 = a.lut64;
    b.tab = a.tab;
    b.out_day = a.out_day;
    b.out_night = a.out_night;
    b.status = a.status;
    return b;
}

// All pointers are device pointers here. The handle's geometry picks the instances.
template <typename T>
static int launch_downscaled(mod16_ctx* ctx, const mod16_downscale* grid, DsArgs<T> a, unsigned flags, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    a.lut64 = ctx->lut64.as<double>();
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    const int blocks = batch_blocks(ctx, a.n);
    ds_dispatch(grid, [&](const auto& g) {
        using G = std::decay_t<decltype(g)>;
        const DsArgs<T, G> b = ds_with_grid<T, G>(a, g);
        if (flags & MOD16_MATH_EXACT) hipLaunchKernelGGL((ds_kernel<T, false, G>), dim3(blocks), dim3(kBlock), 0, st, b);
        else {
            hipLaunchKernelGGL((ds_kernel<T, true, G>), dim3(blocks), dim3(kBlock), 0, st, b);
            // pixels outside the domain of the fast arithmetic: the kernel above left a mark in their
            // out_night, this one computes them in the reference's operation order
            hipLaunchKernelGGL((ds_redo_kernel<T, G>), dim3(blocks), dim3(kBlock), 0, st, b);
        }
    });
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

template <typename T>
static int launch_fields(mod16_ctx* ctx, const mod16_downscale* grid, const DsFields<T>& a, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    ds_dispatch(grid, [&](const auto& g) {
        using G = std::decay_t<decltype(g)>;
        const DsFieldArgs<T, G> b = {a, g};
        hipLaunchKernelGGL((ds_fields_kernel<T, G>), dim3(batch_blocks(ctx, a.n)), dim3(kBlock), 0, st, b);
    });
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode of the run: the coarse planes resident, the fine arrays, the class raster and the two
// outputs tile by tile through the shared staging path; HostTile::off gives a tile's first pixel
template <typename T>
static int downscaled_host(mod16_ctx* ctx, const mod16_downscale* grid, const DsArgs<T>& h, unsigned flags) {
    const T* planes[14];
    const T* dev[14];
    for (int k = 0; k < 14; ++k) planes[k] = ((h.coarse >> k) & 1u) ? h.drv[k] : nullptr;
    int rc = upload_coarse<T>(ctx, grid, planes, nullptr, nullptr, h.cpitch, 14, "coarse planes", dev);
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
    const char* const prefix = "mod16_et_downscaled: ";
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, prefix, what); };
    if (!grid || !cls || !drivers || !kinds || !out_day || !out_night) return bad("NULL grid, class raster, drivers, kinds or outputs");
    if (flags & MOD16_MATH_MIXED)
        return bad("MOD16_MATH_MIXED is not available for the downscaled run (MOD16_MATH_FAST or MOD16_MATH_EXACT)");
    if (flags & MOD16_DOMAIN_TRUSTED)
        return bad("MOD16_DOMAIN_TRUSTED is not available for the downscaled run (every launch is guarded)");
    if (flags & ~(unsigned)MOD16_MATH_EXACT) return bad("unknown flag");
    if (const char* what = check_where(where)) return bad(what);
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
    if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, prefix, "mod16_set_bplut_f64 was not called");
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
static int fields_host(mod16_ctx* ctx, const mod16_downscale* grid, const DsFields<T>& h) {
    const T* dev[kDsMaxFields];
    int rc = upload_coarse<T>(ctx, grid, h.field, nullptr, nullptr, h.cpitch, h.nfields, "coarse planes", dev);
    if (rc != MOD16_OK) return rc;
    HostPlan p(sizeof(T));
    p.add(kOut, h.out, false, h.nfields, h.out_pitch);
    // a slot's slab holds the F rows of a tile: cut the tile so that it stays within 32 MiB
    int64_t tile = ((int64_t)32 << 20) / ((int64_t)h.nfields * (int64_t)sizeof(T)) / kBlock * kBlock;
    tile = std::max<int64_t>(kBlock, std::min<int64_t>(tile, kTilePixels));
    auto launch = [&](const HostTile& t) {
        DsFields<T> d = h;
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
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_downscale_fields: ", what); };
    if (!grid || !fields || !out) return bad("NULL grid, fields or out");
    if (nfields < 1 || nfields > kDsMaxFields) return bad("F must be between 1 and 16");
    if (const char* what = check_where(where)) return bad(what);
    if (grid->device != ctx->device) return bad("the grid was created on another device than this context's");
    const int64_t total = grid->spec.rows * grid->spec.cols;
    if (n < 0 || first_pixel < 0 || first_pixel > total || n > total - first_pixel)
        return bad("the pixel range [first_pixel, first_pixel + n) leaves the raster");
    if (coarse_pitch < grid->spec.coarse_cols) return bad("coarse_pitch must be at least coarse_cols");
    if (out_pitch < n) return bad("out_pitch must be at least n");
    DsFields<T> a;
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
    return fields_host<T>(ctx, grid, a);
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
