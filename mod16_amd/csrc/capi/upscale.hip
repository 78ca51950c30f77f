// libmod16hip.so -- upscaling: mod16_upscale_create / _create_rows / _destroy (the runs of a coarse grid's cells in a fine raster; row-affine columns: the rows' runs and two float64 per fine row), mod16_upscale_sums_f32 / _f64 (the sums before the divisions), mod16_upscale_f32 / _f64 (per layer and cell the area-weighted mean of the valid fine pixels, the valid fraction and the count), mod16_upscale_classes (the dominant class per cell)
#include "host.hpp"
#include "../mod16_upscale.hpp"

namespace {
constexpr int64_t kUpMaxExtent = int64_t(1) << 30;
constexpr int kUpMaxLayers = 65535;
constexpr int64_t kUpMaxBlocks = (int64_t(1) << 31) - 1;
}  // namespace

// The four run tables (and the area weights) on the device, with what the host needs of them: the row
// runs for the bands of the HOST mode.
struct mod16_upscale {
    int device = 0;
    mod16_upscale_spec spec = {};
    DevMem tables;               // row_first, row_count (int32 [H]), col_first, col_count (int32 [W]), area (double [R]) or nothing;
                                 // by_rows: row_first, row_count, origin, scale (double [R]), col_first, col_count (int32 [R]) or nothing, area
    UpGeom g = {};               // views into `tables`; the launch fills in what depends on it
    bool by_rows = false;        // row-affine columns (mod16_upscale_create_rows): g.col_first / g.col_count are NULL, rg holds the rows'
    UpRowsGeom rg = {};
    std::vector<int32_t> row_first, row_count;
};

extern "C" int mod16_upscale_destroy(mod16_upscale* grid) {
    if (!grid) return MOD16_OK;
    (void)hipSetDevice(grid->device);
    delete grid;
    return MOD16_OK;
}

static int up_bad(mod16_ctx* ctx, const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_upscale_create: ", what); }

// -> NULL, or what is wrong with the runs of one axis of n fine indices (upscale.check_runs); *largest: the longest run
static const char* up_check_runs(const int32_t* first, const int32_t* count, int64_t size, int64_t n, bool wrap, int64_t* largest) {
    std::vector<std::pair<int64_t, int64_t>> runs;
    *largest = 0;
    for (int64_t k = 0; k < size; ++k) {
        const int64_t f = first[k], c = count[k];
        if (c < 0 || c > n) return "a count lies outside 0 ... the extent of its axis";
        if (c == 0) continue;
        if (f < 0 || f >= n || (!wrap && f + c > n)) return "a run leaves its axis";
        *largest = std::max(*largest, c);
        runs.emplace_back(f, f + c);
    }
    std::sort(runs.begin(), runs.end());
    for (size_t k = 1; k < runs.size(); ++k)
        if (runs[k].first < runs[k - 1].second) return "two runs of one axis share a fine index";
    if (!runs.empty() && runs.back().second - n > runs.front().first) return "two runs of one axis share a fine index";
    return nullptr;
}

extern "C" int mod16_upscale_create(mod16_ctx* ctx, const mod16_upscale_spec* s, const int32_t* row_first,
                                    const int32_t* row_count, const int32_t* col_first, const int32_t* col_count,
                                    const double* area, mod16_upscale** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    if (out) *out = nullptr;
    if (!s || !row_first || !row_count || !col_first || !col_count || !out) return up_bad(ctx, "NULL argument");
    if (s->rows < 1 || s->rows > kUpMaxExtent || s->cols < 1 || s->cols > kUpMaxExtent)
        return up_bad(ctx, "rows and cols must be between 1 and 2^30");
    if (s->coarse_rows < 1 || s->coarse_rows > kUpMaxExtent || s->coarse_cols < 1 || s->coarse_cols > kUpMaxExtent)
        return up_bad(ctx, "coarse_rows and coarse_cols must be between 1 and 2^30");
    if (s->wrap_cols != 0 && s->wrap_cols != 1) return up_bad(ctx, "wrap_cols must be 0 or 1");
    const int64_t R = s->rows, C = s->cols, H = s->coarse_rows, W = s->coarse_cols;
    int64_t tallest = 0, widest = 0;
    if (const char* what = up_check_runs(row_first, row_count, H, R, false, &tallest)) return up_bad(ctx, what);
    if (const char* what = up_check_runs(col_first, col_count, W, C, s->wrap_cols != 0, &widest)) return up_bad(ctx, what);
    if (tallest * widest >= (int64_t(1) << 31)) return up_bad(ctx, "a cell must hold fewer than 2^31 pixels (row_count * col_count)");
    if (area)
        for (int64_t r = 0; r < R; ++r)
            if (!(std::isfinite(area[r]) && area[r] > 0.0)) return up_bad(ctx, "area must be positive and finite");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_upscale* g = new (std::nothrow) mod16_upscale;
    if (!g) return MOD16_ERR_NOMEM;
    g->device = ctx->device;
    g->spec = *s;
    g->row_first.assign(row_first, row_first + H);
    g->row_count.assign(row_count, row_count + H);
    struct Piece { const void* src; size_t bytes; };
    const Piece pieces[5] = {{row_first, (size_t)H * 4}, {row_count, (size_t)H * 4}, {col_first, (size_t)W * 4},
                             {col_count, (size_t)W * 4}, {area, area ? (size_t)R * 8 : 0}};
    Carver size;
    for (const Piece& p : pieces) size.take<char>(p.bytes);
    int rc = g->tables.alloc(ctx, size.used + 256, "mod16_upscale_create: device memory for the run tables");
    if (rc == MOD16_OK) {
        Carver block(g->tables.get());
        const char* at[5];
        for (int k = 0; k < 5; ++k) {
            at[k] = block.take<char>(pieces[k].bytes);
            if (rc == MOD16_OK && pieces[k].bytes &&
                hipMemcpy(const_cast<char*>(at[k]), pieces[k].src, pieces[k].bytes, hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ctx, MOD16_ERR_HIP, "mod16_upscale_create: upload of the run tables failed");
        }
        auto i32 = [&](int k) { return reinterpret_cast<const int32_t*>(at[k]); };
        g->g.row_first = i32(0);
        g->g.row_count = i32(1);
        g->g.col_first = i32(2);
        g->g.col_count = i32(3);
        g->g.area = area ? reinterpret_cast<const double*>(at[4]) : nullptr;
        g->g.cols = C;
        g->g.coarse_cols = (int32_t)W;
    }
    if (rc != MOD16_OK) {
        mod16_upscale_destroy(g);
        return rc;
    }
    *out = g;
    return MOD16_OK;
}

extern "C" int mod16_upscale_create_rows(mod16_ctx* ctx, const mod16_upscale_spec* s, const int32_t* row_first,
                                         const int32_t* row_count, const double* col_origin, const double* col_scale,
                                         const int32_t* col_first, const int32_t* col_count, const double* area,
                                         mod16_upscale** out) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_upscale_create_rows: ", what); };
    if (out) *out = nullptr;
    if (!s || !row_first || !row_count || !col_origin || !col_scale || !out) return bad("NULL argument");
    if ((col_first == nullptr) != (col_count == nullptr)) return bad("col_first and col_count must both be given or both be NULL");
    if (s->rows < 1 || s->rows > kUpMaxExtent || s->cols < 1 || s->cols > kUpMaxExtent)
        return bad("rows and cols must be between 1 and 2^30");
    if (s->coarse_rows < 1 || s->coarse_rows > kUpMaxExtent || s->coarse_cols < 1 || s->coarse_cols > kUpMaxExtent)
        return bad("coarse_rows and coarse_cols must be between 1 and 2^30");
    if (s->wrap_cols != 0 && s->wrap_cols != 1) return bad("wrap_cols must be 0 or 1");
    const int64_t R = s->rows, C = s->cols, H = s->coarse_rows, W = s->coarse_cols;
    int64_t tallest = 0, widest = 0;
    if (const char* what = up_check_runs(row_first, row_count, H, R, false, &tallest)) return bad(what);
    for (int64_t r = 0; r < R; ++r) {
        const double far = col_origin[r] + col_scale[r] * (double)(C - 1);
        if (!(std::isfinite(col_origin[r]) && std::isfinite(col_scale[r]) && std::isfinite(far)))
            return bad("col_origin, col_scale and col_origin + col_scale * (cols - 1) must be finite in every row");
        const int64_t f = col_first ? col_first[r] : 0, n = col_first ? col_count[r] : C;
        if (f < 0 || n < 0 || f + n > C) return bad("a column range leaves its row (0 <= first, 0 <= count, first + count <= cols)");
        // sufficient for one run of consecutive columns per cell and fine row (upscale.check_rows)
        if (s->wrap_cols && n > 1 && !(std::fabs(col_scale[r]) * (double)(n - 1) <= (double)(W - 2)))
            return bad("a fine row may lap the periodic axis (abs(col_scale) * (columns - 1) > coarse_cols - 2): give a narrower column range or cut the raster");
        widest = std::max(widest, n);
    }
    if (tallest * widest >= (int64_t(1) << 31)) return bad("a cell must hold fewer than 2^31 pixels (row_count * col_count)");
    if (area)
        for (int64_t r = 0; r < R; ++r)
            if (!(std::isfinite(area[r]) && area[r] > 0.0)) return bad("area must be positive and finite");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mod16_upscale* g = new (std::nothrow) mod16_upscale;
    if (!g) return MOD16_ERR_NOMEM;
    g->device = ctx->device;
    g->spec = *s;
    g->by_rows = true;
    g->row_first.assign(row_first, row_first + H);
    g->row_count.assign(row_count, row_count + H);
    struct Piece { const void* src; size_t bytes; };
    const Piece pieces[7] = {{col_origin, (size_t)R * 8}, {col_scale, (size_t)R * 8}, {area, area ? (size_t)R * 8 : 0},
                             {row_first, (size_t)H * 4}, {row_count, (size_t)H * 4},
                             {col_first, col_first ? (size_t)R * 4 : 0}, {col_count, col_first ? (size_t)R * 4 : 0}};
    Carver size;
    for (const Piece& p : pieces) size.take<char>(p.bytes);
    int rc = g->tables.alloc(ctx, size.used + 256, "mod16_upscale_create_rows: device memory for the tables");
    if (rc == MOD16_OK) {
        Carver block(g->tables.get());
        const char* at[7];
        for (int k = 0; k < 7; ++k) {
            at[k] = block.take<char>(pieces[k].bytes);
            if (rc == MOD16_OK && pieces[k].bytes &&
                hipMemcpy(const_cast<char*>(at[k]), pieces[k].src, pieces[k].bytes, hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ctx, MOD16_ERR_HIP, "mod16_upscale_create_rows: upload of the tables failed");
        }
        auto i32 = [&](int k) { return reinterpret_cast<const int32_t*>(at[k]); };
        auto f64 = [&](int k) { return reinterpret_cast<const double*>(at[k]); };
        g->rg.origin = f64(0);
        g->rg.scale = f64(1);
        g->g.area = area ? f64(2) : nullptr;
        g->g.row_first = i32(3);
        g->g.row_count = i32(4);
        g->rg.col_first = col_first ? i32(5) : nullptr;
        g->rg.col_count = col_first ? i32(6) : nullptr;
        g->rg.wrap = s->wrap_cols;
        g->g.col_first = g->g.col_count = nullptr;
        g->g.cols = C;
        g->g.coarse_cols = (int32_t)W;
    }
    if (rc != MOD16_OK) {
        mod16_upscale_destroy(g);
        return rc;
    }
    *out = g;
    return MOD16_OK;
}

// The lanes of a block = the cells of its span: 256, halved down to a wave while the launch would leave
// the device short of blocks (8 per CU); -> the geometry of a launch over `cell_rows` coarse rows from
// `cell_row_first`, whose input starts at fine row `row_base`
static UpGeom up_launch_geom(const mod16_ctx* ctx, const mod16_upscale* grid, int64_t layers, int32_t cell_row_first,
                             int32_t cell_rows, int64_t row_base, int* lanes, int64_t* blocks) {
    UpGeom g = grid->g;
    const int64_t W = g.coarse_cols;
    int l = kUpMaxLanes;
    auto count = [&](int n) { return layers * (int64_t)cell_rows * ((W + n - 1) / n); };
    while (l > 64 && (W <= l / 2 || count(l) < (int64_t)ctx->cus * 8)) l /= 2;
    g.spans = (int32_t)((W + l - 1) / l);
    g.cell_row_first = cell_row_first;
    g.cell_rows = cell_rows;
    g.row_base = row_base;
    *lanes = l;
    *blocks = count(l);
    return g;
}

template <typename T, bool ROWS, bool SUMS>
static void launch_upscale_ext(const UpArgs<T>& a, const UpRowsGeom& rg, const UpSumArgs& sm, int lanes, int64_t blocks, hipStream_t st) {
    if (lanes == 64) hipLaunchKernelGGL((upscale_ext_kernel<T, 64, ROWS, SUMS>), dim3((unsigned)blocks), dim3(64), 0, st, a, rg, sm);
    else if (lanes == 128) hipLaunchKernelGGL((upscale_ext_kernel<T, 128, ROWS, SUMS>), dim3((unsigned)blocks), dim3(128), 0, st, a, rg, sm);
    else hipLaunchKernelGGL((upscale_ext_kernel<T, 256, ROWS, SUMS>), dim3((unsigned)blocks), dim3(256), 0, st, a, rg, sm);
}

// All pointers are device pointers here; a.g holds the launch's rows (up_launch_geom). sm: the outputs of
// a sums call, or NULL (mean, fraction and count); the grid's geometry picks the walk.
template <typename T>
static int launch_upscale(mod16_ctx* ctx, const mod16_upscale* grid, const UpArgs<T>& a, const UpSumArgs* sm, int lanes,
                          int64_t blocks, hipStream_t st) {
    if (blocks <= 0) return MOD16_OK;
    if (grid->by_rows || sm) {
        const UpSumArgs none = {};
        if (grid->by_rows && sm) launch_upscale_ext<T, true, true>(a, grid->rg, *sm, lanes, blocks, st);
        else if (grid->by_rows) launch_upscale_ext<T, true, false>(a, grid->rg, none, lanes, blocks, st);
        else launch_upscale_ext<T, false, true>(a, grid->rg, *sm, lanes, blocks, st);
        HIPCHK(ctx, hipGetLastError());
        return MOD16_OK;
    }
    if (lanes == 64) hipLaunchKernelGGL((upscale_kernel<T, 64>), dim3((unsigned)blocks), dim3(64), 0, st, a);
    else if (lanes == 128) hipLaunchKernelGGL((upscale_kernel<T, 128>), dim3((unsigned)blocks), dim3(128), 0, st, a);
    else hipLaunchKernelGGL((upscale_kernel<T, 256>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}
static int launch_upscale_classes(mod16_ctx* ctx, const mod16_upscale* grid, const UpClassArgs& a, int lanes, int64_t blocks,
                                  hipStream_t st) {
    if (blocks <= 0) return MOD16_OK;
    if (grid->by_rows) {
        if (lanes == 64) hipLaunchKernelGGL(upscale_classes_rows_kernel<64>, dim3((unsigned)blocks), dim3(64), 0, st, a, grid->rg);
        else if (lanes == 128) hipLaunchKernelGGL(upscale_classes_rows_kernel<128>, dim3((unsigned)blocks), dim3(128), 0, st, a, grid->rg);
        else hipLaunchKernelGGL(upscale_classes_rows_kernel<256>, dim3((unsigned)blocks), dim3(256), 0, st, a, grid->rg);
        HIPCHK(ctx, hipGetLastError());
        return MOD16_OK;
    }
    if (lanes == 64) hipLaunchKernelGGL(upscale_classes_kernel<64>, dim3((unsigned)blocks), dim3(64), 0, st, a);
    else if (lanes == 128) hipLaunchKernelGGL(upscale_classes_kernel<128>, dim3((unsigned)blocks), dim3(128), 0, st, a);
    else hipLaunchKernelGGL(upscale_classes_kernel<256>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// ---- HOST mode. The inputs and outputs of a range have different sizes, so the family has its own loop
// through the context's first slab and stream: bands of whole coarse rows (the fine rows of a band are
// the one range of rows from the lowest to the highest row any of its cells has), the layers cut first
// where those of one coarse row exceed the budget.
struct UpHostArray { char* host; int64_t layer_stride, row_stride; size_t elem; };    // strides in elements
struct UpBand {
    int32_t i0, rows;            // the band's coarse rows
    int64_t r0, fine_rows;       // its fine rows
    int32_t k0, layers;          // its layers
    char* in;                    // device: [layers][fine_rows][cols]
    char* out[4];                // device: [layers][rows][coarse_cols] each, NULL for an absent output
    hipStream_t st;
};

// rows `n` elements long: one copy where they lie back to back on both sides, else one per row
static int up_copy_rows(mod16_ctx* ctx, char* dst, int64_t dst_pitch, const char* src, int64_t src_pitch, int64_t rows,
                        int64_t n, size_t elem, hipMemcpyKind kind, hipStream_t st) {
    if (rows <= 0 || n <= 0) return MOD16_OK;
    if (dst_pitch == n && src_pitch == n) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)(rows * n) * elem, kind, st));
        return MOD16_OK;
    }
    for (int64_t r = 0; r < rows; ++r)
        HIPCHK(ctx, hipMemcpyAsync(dst + (size_t)(r * dst_pitch) * elem, src + (size_t)(r * src_pitch) * elem, (size_t)n * elem, kind, st));
    return MOD16_OK;
}

template <typename Launch>
static int up_host_bands(mod16_ctx* ctx, const mod16_upscale* grid, int K, const UpHostArray& in, const UpHostArray* outs,
                         int nout, int64_t stage_bytes, Launch&& launch) {
    const int64_t C = grid->spec.cols, H = grid->spec.coarse_rows, W = grid->spec.coarse_cols;
    int64_t out_row = 0;                               // bytes of a coarse row of one layer in the outputs
    for (int o = 0; o < nout; ++o)
        if (outs[o].host) out_row += (int64_t)align256((size_t)W * outs[o].elem);
    const int64_t slack = 256 * (int64_t)(nout + 2);
    // the fine rows [lo, hi) of the coarse rows [i0, i1); hi == lo: none of them has a pixel
    auto range = [&](int64_t i0, int64_t i1, int64_t* lo, int64_t* hi) {
        *lo = std::numeric_limits<int64_t>::max();
        *hi = 0;
        for (int64_t i = i0; i < i1; ++i)
            if (grid->row_count[i] > 0) {
                *lo = std::min<int64_t>(*lo, grid->row_first[i]);
                *hi = std::max<int64_t>(*hi, (int64_t)grid->row_first[i] + grid->row_count[i]);
            }
        if (*hi == 0) *lo = 0;
    };
    auto bytes = [&](int64_t i0, int64_t i1, int64_t layers) {
        int64_t lo, hi;
        range(i0, i1, &lo, &hi);
        return layers * ((hi - lo) * C * (int64_t)in.elem + (i1 - i0) * out_row) + slack;
    };
    // layers of a pass: all, or as many as fit with the tallest coarse row
    int64_t tallest = 0;
    for (int64_t i = 0; i < H; ++i) tallest = std::max(tallest, bytes(i, i + 1, 1) - slack);
    const int64_t KL = std::max<int64_t>(1, std::min<int64_t>(K, (stage_bytes - slack) / std::max<int64_t>(tallest, 1)));
    for (int64_t k0 = 0; k0 < K; k0 += KL) {
        const int64_t kl = std::min<int64_t>(KL, K - k0);
        for (int64_t i0 = 0; i0 < H;) {
            int64_t i1 = i0 + 1;
            while (i1 < H && bytes(i0, i1 + 1, kl) <= stage_bytes) ++i1;
            int64_t lo, hi;
            range(i0, i1, &lo, &hi);
            int rc = reserve_slabs(ctx, (size_t)bytes(i0, i1, kl), 1);
            if (rc != MOD16_OK) return rc;
            Carver slab(ctx->slab[0].get());
            UpBand b;
            b.i0 = (int32_t)i0; b.rows = (int32_t)(i1 - i0);
            b.r0 = lo; b.fine_rows = hi - lo;
            b.k0 = (int32_t)k0; b.layers = (int32_t)kl;
            b.st = ctx->streams[0];
            b.in = slab.take<char>((size_t)(kl * b.fine_rows * C) * in.elem);
            for (int o = 0; o < 4; ++o)
                b.out[o] = o < nout && outs[o].host ? slab.take<char>((size_t)(kl * b.rows * W) * outs[o].elem) : nullptr;
            for (int64_t k = 0; k < kl; ++k) {
                rc = up_copy_rows(ctx, b.in + (size_t)(k * b.fine_rows * C) * in.elem, C,
                                  in.host + (size_t)((k0 + k) * in.layer_stride + lo * in.row_stride) * in.elem, in.row_stride,
                                  b.fine_rows, C, in.elem, hipMemcpyHostToDevice, b.st);
                if (rc != MOD16_OK) return rc;
            }
            rc = launch(b);
            if (rc != MOD16_OK) return rc;
            for (int o = 0; o < nout; ++o)
                for (int64_t k = 0; b.out[o] && k < kl; ++k) {
                    rc = up_copy_rows(ctx, outs[o].host + (size_t)((k0 + k) * outs[o].layer_stride + i0 * outs[o].row_stride) * outs[o].elem,
                                      outs[o].row_stride, b.out[o] + (size_t)(k * b.rows * W) * outs[o].elem, W, b.rows, W,
                                      outs[o].elem, hipMemcpyDeviceToHost, b.st);
                    if (rc != MOD16_OK) return rc;
                }
            HIPCHK(ctx, hipStreamSynchronize(b.st));       // the slab is free again
            i0 = i1;
        }
    }
    return MOD16_OK;
}

// what the entry points check of an [layers][rows][n] array: -> NULL or what is wrong
static const char* up_check_strides(int64_t layers, int64_t rows, int64_t n, int64_t layer_stride, int64_t row_stride) {
    const int64_t most = int64_t(1) << 56;             // elements an array may span: its extent in bytes fits an int64
    if (row_stride < n) return "a row stride is below the length of a row";
    if (row_stride > most / rows) return "a row stride is out of range";
    if (layers > 1 && layer_stride < (rows - 1) * row_stride + n) return "a layer stride is below a plane";
    if (layers > 1 && layer_stride > most / layers) return "a layer stride is out of range";
    return nullptr;
}

// one output of a call: [layers][coarse_rows][coarse_cols] with its strides in elements
struct UpOut { void* p; int64_t ls, rs; size_t elem; };

// mod16_upscale_f32 / _f64 (outs: mean, fraction, count) and mod16_upscale_sums_f32 / _f64 (sums: outs are
// num, den, tot, count)
template <typename T>
static int upscale_entry(mod16_ctx* ctx, const char* name, const mod16_upscale* grid, const T* values, int32_t layers,
                         int64_t layer_stride, int64_t row_stride, double min_fraction, bool sums, const UpOut* o, int where,
                         void* stream, size_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, name, what); };
    const int nout = sums ? 4 : 3;
    if (!grid || !values) return bad("NULL grid or values");
    if (grid->device != ctx->device) return bad("the grid was created on another device than this context's");
    bool any = false;
    for (int k = 0; k < nout; ++k) any = any || o[k].p;
    if (!any) return bad("no output is requested");
    if (layers < 1 || layers > kUpMaxLayers) return bad("layers must be between 1 and 65535");
    if (!(min_fraction >= 0.0 && min_fraction <= 1.0)) return bad("min_fraction must lie in [0, 1]");
    const int64_t R = grid->spec.rows, C = grid->spec.cols, H = grid->spec.coarse_rows, W = grid->spec.coarse_cols;
    if (const char* what = up_check_strides(layers, R, C, layer_stride, row_stride)) return bad(what);
    for (int k = 0; k < nout; ++k)
        if (o[k].p) if (const char* what = up_check_strides(layers, H, W, o[k].ls, o[k].rs)) return bad(what);
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    if ((int64_t)layers * H * ((W + 63) / 64) > kUpMaxBlocks) return bad("layers * coarse_rows * ceil(coarse_cols / 64) must stay below 2^31");
    {
        Extent ins[1], outs[4];
        int no = 0;
        ins[0] = extent(values, layers, layer_stride, R, row_stride, C, sizeof(T));
        for (int k = 0; k < nout; ++k)
            if (o[k].p) outs[no++] = extent(o[k].p, layers, o[k].ls, H, o[k].rs, W, o[k].elem);
        if (overlaps(outs, no, ins, 1)) return bad("an output overlaps an input or another output");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    UpArgs<T> a;
    memset(&a, 0, sizeof a);
    a.min_fraction = min_fraction;
    UpSumArgs sm = {};
    // the outputs into the kernels' arguments: p[k] with layer stride ls[k] and row stride rs[k]
    auto place = [&](UpArgs<T>& d, UpSumArgs& m, void* const* p, const int64_t* ls, const int64_t* rs) {
        if (sums) {
            m.num = static_cast<double*>(p[0]); m.num_layer = ls[0]; m.num_row = rs[0];
            m.den = static_cast<double*>(p[1]); m.den_layer = ls[1]; m.den_row = rs[1];
            m.tot = static_cast<double*>(p[2]); m.tot_layer = ls[2]; m.tot_row = rs[2];
        } else {
            d.mean = static_cast<T*>(p[0]); d.mean_layer = ls[0]; d.mean_row = rs[0];
            d.fraction = static_cast<T*>(p[1]); d.fraction_layer = ls[1]; d.fraction_row = rs[1];
        }
        d.count = static_cast<int32_t*>(p[nout - 1]); d.count_layer = ls[nout - 1]; d.count_row = rs[nout - 1];
    };
    int lanes = 0;
    int64_t blocks = 0;
    if (where == MOD16_DEVICE) {
        a.g = up_launch_geom(ctx, grid, layers, 0, (int32_t)H, 0, &lanes, &blocks);
        a.values = values; a.layer_stride = layer_stride; a.row_stride = row_stride;
        void* p[4];
        int64_t ls[4], rs[4];
        for (int k = 0; k < nout; ++k) { p[k] = o[k].p; ls[k] = o[k].ls; rs[k] = o[k].rs; }
        place(a, sm, p, ls, rs);
        return launch_upscale<T>(ctx, grid, a, sums ? &sm : nullptr, lanes, blocks, static_cast<hipStream_t>(stream));
    }
    const UpHostArray in = {reinterpret_cast<char*>(const_cast<T*>(values)), layer_stride, row_stride, sizeof(T)};
    UpHostArray outs[4];
    for (int k = 0; k < nout; ++k) outs[k] = UpHostArray{static_cast<char*>(o[k].p), o[k].ls, o[k].rs, o[k].elem};
    return up_host_bands(ctx, grid, layers, in, outs, nout, stage_budget(stage_bytes), [&](const UpBand& b) {
        UpArgs<T> d = a;
        UpSumArgs m = {};
        int l = 0;
        int64_t n = 0;
        d.g = up_launch_geom(ctx, grid, b.layers, b.i0, b.rows, b.r0, &l, &n);
        d.values = reinterpret_cast<const T*>(b.in);
        d.row_stride = C;
        d.layer_stride = b.fine_rows * C;
        void* p[4];
        int64_t ls[4], rs[4];
        for (int k = 0; k < nout; ++k) { p[k] = b.out[k]; ls[k] = (int64_t)b.rows * W; rs[k] = W; }
        place(d, m, p, ls, rs);
        return launch_upscale<T>(ctx, grid, d, sums ? &m : nullptr, l, n, b.st);
    });
}

extern "C" int mod16_upscale_f32(mod16_ctx* ctx, const mod16_upscale* grid, const float* values, int32_t layers,
                                 int64_t layer_stride, int64_t row_stride, double min_fraction, float* mean,
                                 int64_t mean_layer_stride, int64_t mean_row_stride, float* fraction,
                                 int64_t fraction_layer_stride, int64_t fraction_row_stride, int32_t* count,
                                 int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                 size_t stage_bytes) {
    MOD16_LOCK(ctx);
    const UpOut outs[3] = {{mean, mean_layer_stride, mean_row_stride, sizeof(float)},
                           {fraction, fraction_layer_stride, fraction_row_stride, sizeof(float)},
                           {count, count_layer_stride, count_row_stride, sizeof(int32_t)}};
    return upscale_entry<float>(ctx, "mod16_upscale: ", grid, values, layers, layer_stride, row_stride, min_fraction, false, outs,
                             where, stream, stage_bytes);
}
extern "C" int mod16_upscale_f64(mod16_ctx* ctx, const mod16_upscale* grid, const double* values, int32_t layers,
                                 int64_t layer_stride, int64_t row_stride, double min_fraction, double* mean,
                                 int64_t mean_layer_stride, int64_t mean_row_stride, double* fraction,
                                 int64_t fraction_layer_stride, int64_t fraction_row_stride, int32_t* count,
                                 int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                 size_t stage_bytes) {
    MOD16_LOCK(ctx);
    const UpOut outs[3] = {{mean, mean_layer_stride, mean_row_stride, sizeof(double)},
                           {fraction, fraction_layer_stride, fraction_row_stride, sizeof(double)},
                           {count, count_layer_stride, count_row_stride, sizeof(int32_t)}};
    return upscale_entry<double>(ctx, "mod16_upscale: ", grid, values, layers, layer_stride, row_stride, min_fraction, false, outs,
                             where, stream, stage_bytes);
}

extern "C" int mod16_upscale_classes(mod16_ctx* ctx, const mod16_upscale* grid, const uint8_t* cls, int64_t row_stride,
                                     uint32_t valid, uint8_t* out_cls, int64_t cls_row_stride, float* out_share,
                                     int64_t share_row_stride, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_upscale_classes: ", what); };
    if (!grid || !cls) return bad("NULL grid or class raster");
    if (grid->device != ctx->device) return bad("the grid was created on another device than this context's");
    if (!out_cls && !out_share) return bad("no output is requested");
    const int64_t R = grid->spec.rows, C = grid->spec.cols, H = grid->spec.coarse_rows, W = grid->spec.coarse_cols;
    if (const char* what = up_check_strides(1, R, C, 0, row_stride)) return bad(what);
    if (out_cls) if (const char* what = up_check_strides(1, H, W, 0, cls_row_stride)) return bad(what);
    if (out_share) if (const char* what = up_check_strides(1, H, W, 0, share_row_stride)) return bad(what);
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    if (H * ((W + 63) / 64) > kUpMaxBlocks) return bad("coarse_rows * ceil(coarse_cols / 64) must stay below 2^31");
    {
        Extent ins[1], outs[2];
        int no = 0;
        ins[0] = extent(cls, 1, 0, R, row_stride, C, 1);
        if (out_cls) outs[no++] = extent(out_cls, 1, 0, H, cls_row_stride, W, 1);
        if (out_share) outs[no++] = extent(out_share, 1, 0, H, share_row_stride, W, sizeof(float));
        if (overlaps(outs, no, ins, 1)) return bad("an output overlaps an input or another output");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    UpClassArgs a;
    memset(&a, 0, sizeof a);
    a.valid = valid;
    int lanes = 0;
    int64_t blocks = 0;
    if (where == MOD16_DEVICE) {
        a.g = up_launch_geom(ctx, grid, 1, 0, (int32_t)H, 0, &lanes, &blocks);
        a.cls = cls; a.row_stride = row_stride;
        a.out_cls = out_cls; a.cls_row = cls_row_stride;
        a.out_share = out_share; a.share_row = share_row_stride;
        return launch_upscale_classes(ctx, grid, a, lanes, blocks, static_cast<hipStream_t>(stream));
    }
    const UpHostArray in = {reinterpret_cast<char*>(const_cast<uint8_t*>(cls)), 0, row_stride, 1};
    const UpHostArray outs[2] = {{reinterpret_cast<char*>(out_cls), 0, cls_row_stride, 1},
                                 {reinterpret_cast<char*>(out_share), 0, share_row_stride, sizeof(float)}};
    return up_host_bands(ctx, grid, 1, in, outs, 2, stage_budget(stage_bytes), [&](const UpBand& b) {
        UpClassArgs d = a;
        int l = 0;
        int64_t n = 0;
        d.g = up_launch_geom(ctx, grid, 1, b.i0, b.rows, b.r0, &l, &n);
        d.cls = reinterpret_cast<const uint8_t*>(b.in);
        d.row_stride = C;
        d.out_cls = reinterpret_cast<uint8_t*>(b.out[0]);
        d.out_share = reinterpret_cast<float*>(b.out[1]);
        d.cls_row = d.share_row = W;
        return launch_upscale_classes(ctx, grid, d, l, n, b.st);
    });
}

extern "C" int mod16_upscale_sums_f32(mod16_ctx* ctx, const mod16_upscale* grid, const float* values, int32_t layers,
                                      int64_t layer_stride, int64_t row_stride, double* num, int64_t num_layer_stride,
                                      int64_t num_row_stride, double* den, int64_t den_layer_stride, int64_t den_row_stride,
                                      double* tot, int64_t tot_layer_stride, int64_t tot_row_stride, int32_t* count,
                                      int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                      size_t stage_bytes) {
    MOD16_LOCK(ctx);
    const UpOut outs[4] = {{num, num_layer_stride, num_row_stride, sizeof(double)}, {den, den_layer_stride, den_row_stride, sizeof(double)},
                           {tot, tot_layer_stride, tot_row_stride, sizeof(double)}, {count, count_layer_stride, count_row_stride, sizeof(int32_t)}};
    return upscale_entry<float>(ctx, "mod16_upscale_sums: ", grid, values, layers, layer_stride, row_stride, 0.0, true, outs, where,
                                stream, stage_bytes);
}
extern "C" int mod16_upscale_sums_f64(mod16_ctx* ctx, const mod16_upscale* grid, const double* values, int32_t layers,
                                      int64_t layer_stride, int64_t row_stride, double* num, int64_t num_layer_stride,
                                      int64_t num_row_stride, double* den, int64_t den_layer_stride, int64_t den_row_stride,
                                      double* tot, int64_t tot_layer_stride, int64_t tot_row_stride, int32_t* count,
                                      int64_t count_layer_stride, int64_t count_row_stride, int where, void* stream,
                                      size_t stage_bytes) {
    MOD16_LOCK(ctx);
    const UpOut outs[4] = {{num, num_layer_stride, num_row_stride, sizeof(double)}, {den, den_layer_stride, den_row_stride, sizeof(double)},
                           {tot, tot_layer_stride, tot_row_stride, sizeof(double)}, {count, count_layer_stride, count_row_stride, sizeof(int32_t)}};
    return upscale_entry<double>(ctx, "mod16_upscale_sums: ", grid, values, layers, layer_stride, row_stride, 0.0, true, outs, where,
                                 stream, stage_bytes);
}
