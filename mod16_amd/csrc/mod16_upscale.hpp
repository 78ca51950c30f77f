// Upscaling: area-weighted means of the valid fine pixels of every cell of a coarse grid, and the
// dominant class per cell: the kernels of mod16_upscale_f32 / _f64 and mod16_upscale_classes. The
// definition is the numpy statement mod16_amd/upscale.py (aggregate, majority); this file follows it
// step for step, and every float operation it names is one correctly rounded float64 operation here
// (no contraction in the functions that do arithmetic).
//
// Geometry: four int32 tables. The fine rows of coarse row i are row_first[i] + 0 ... row_count[i] - 1,
// the fine columns of coarse column j are col_first[j] + 0 ... col_count[j] - 1, cyclic (mod cols) on a
// periodic column axis: a cell's pixels are a rectangle of the raster, so there is no cell-id raster,
// and since a cell has one owner there are no atomics.
//
// Shape: a block takes one layer, one coarse row and a span of LANES (64, 128 or 256: a template
// parameter, the launch picks it) consecutive coarse columns; a lane owns one cell. Per fine row of the
// coarse row the block brings the columns of its span into LDS kUpSpan = 2048 elements at a time, whatever
// its size -- consecutive lanes load consecutive columns: every value leaves HBM once, in coalesced
// loads, kUpSpan / LANES = 32, 16 or 8 of them per lane into registers, none behind a branch -- and every
// lane adds the part of its run that lies in the chunk, in run order, carrying (s, m) from chunk to
// chunk: a run longer than kUpSpan (a 1 x 2500 strip) is the same sequence of additions as a short one.
// The loads of the NEXT chunk (of this fine row or the first of the next) are issued right after the
// barrier that publishes the current one, so they are in flight while the lanes walk: the registers are
// stored to LDS at the top of the next round. At the end of a fine row the lane folds (s, m) into (num,
// den, tot, cnt) with the row's area weight, as the definition does. The columns are walked in
// "unrolled" coordinates u = col_first ... col_first + col_count - 1, the column being u or u - cols: the
// cyclic run of the cell that straddles the date line is one range like any other.
// The chunks of a span: where the runs of its cells lie back to back (every regular grid), chunk after
// chunk from the lowest column of the span to the highest; where they leave gaps (the span with the
// straddling cell; tables that are not monotone), the next chunk starts at the lowest column any lane
// still has to read (one block-wide minimum per chunk), so that a gap costs no load.
// Bank conflicts: lanes read LDS col_count elements apart, and an even distance would put 2, 4, ...
// lanes of a 32-lane group on one bank (12 apart: 4-way; 16 apart: 16-way; 32 or 64 apart: all 32).
// Element e lies at e + (e >> 5): one pad element per 32, which moves every 32nd element one bank on.
// Counted with the bank rule for 4-byte and 8-byte reads alike: a power of two up to 32 becomes conflict-free,
// 6, 12 and 24 apart 2-way, and the worst distance up to 75 is 3-way (60, 75); the price is that an odd
// distance, conflict-free unpadded, becomes 2-way.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mod16 {

constexpr int kUpMaxLanes = 256;                     // lanes of a block at the most = cells of its span (64, 128 or 256)
constexpr int kUpSpan = 2048;                        // elements of a fine row a block holds in LDS -- and its lanes in registers -- at a time:
                                                     // 8, 16 or 32 loads per lane in flight
constexpr int kUpTile = kUpSpan + kUpSpan / 32;      // ... with one pad element per 32
constexpr int kUpCodes = 32;                         // class codes that can count
constexpr int kUpNoClass = 255;

struct UpGeom {
    const int32_t* row_first;            // [coarse_rows]
    const int32_t* row_count;
    const int32_t* col_first;            // [coarse_cols]
    const int32_t* col_count;
    const double* area;                  // [rows]: the weight of a pixel of that fine row, or NULL (1.0)
    int64_t cols;                        // fine columns
    int64_t row_base;                    // the fine row the input's row 0 is (HOST mode: a band of rows)
    int32_t coarse_cols;
    int32_t spans;                       // blocks along a coarse row: ceil(coarse_cols / LANES)
    int32_t cell_row_first;              // the coarse rows of this launch; the outputs' row 0 is the first
    int32_t cell_rows;
};

template <typename T> struct UpArgs {
    UpGeom g;
    const T* values;                     // [layers][rows][cols], strides below
    int64_t layer_stride, row_stride;
    double min_fraction;
    T* mean;                             // [layers][cell_rows][coarse_cols] each, or NULL
    T* fraction;
    int32_t* count;
    int64_t mean_layer, mean_row, fraction_layer, fraction_row, count_layer, count_row;
};

struct UpClassArgs {
    UpGeom g;
    const uint8_t* cls;                  // [rows][cols]
    int64_t row_stride;
    uint32_t valid;                      // bit c: code c counts
    uint8_t* out_cls;                    // [cell_rows][coarse_cols] each, or NULL
    float* out_share;
    int64_t cls_row, share_row;
};

__device__ __forceinline__ int up_pad(int e) { return e + (e >> 5); }
__device__ __forceinline__ int64_t up_min(int64_t x, int64_t y) { return x < y ? x : y; }
__device__ __forceinline__ int64_t up_max(int64_t x, int64_t y) { return x > y ? x : y; }

// the smallest v of the block (every lane gets it); red: one element per wave, free on return
__device__ __forceinline__ int64_t up_block_min(int64_t v, int64_t* red) {
    for (int off = 32; off; off >>= 1) v = up_min(v, (int64_t)__shfl_xor((long long)v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t r = red[0];
    for (unsigned w = 1; w < blockDim.x / 64; ++w) r = up_min(r, red[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ int64_t up_block_sum(int64_t v, int64_t* red) {
    for (int off = 32; off; off >>= 1) v += (int64_t)__shfl_xor((long long)v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t r = red[0];
    for (unsigned w = 1; w < blockDim.x / 64; ++w) r += red[w];
    __syncthreads();
    return r;
}

// The walk both kernels share: for every fine row of coarse row i, in run order, acc.value(x) for every
// pixel of this lane's cell (coarse column j0 + threadIdx.x) in run order, then acc.row(r). src: the
// plane, its row 0 the fine row g.row_base. Every lane of the block calls this (the barriers).
template <typename T, int LANES, typename Acc>
__device__ __forceinline__ void upscale_walk(const UpGeom& g, const T* src, int64_t row_stride, int i, int j0, T* tile,
                                             int64_t* red, Acc& acc) {
    constexpr int lanes = LANES, LOADS = kUpSpan / LANES;       // a chunk is kUpSpan elements whatever the block's size
    const int tid = (int)threadIdx.x;
    const int j = j0 + tid;
    const int64_t none = INT64_MAX;
    const int64_t n = j < g.coarse_cols ? g.col_count[j] : 0;
    const int64_t a = n ? g.col_first[j] : 0, b = a + n;       // this lane's run in unrolled columns
    const int64_t lo = up_block_min(n ? a : none, red);
    if (lo == none) {                                           // no cell of the span has a pixel
        for (int t = 0; t < g.row_count[i]; ++t) acc.row((int64_t)g.row_first[i] + t);
        return;
    }
    const int64_t hi = -up_block_min(n ? -b : none, red);
    // back to back: no column of [lo, hi) lies outside every run (the runs are disjoint: the host checks)
    const bool dense = up_block_sum(n, red) == hi - lo;
    const int nrows = g.row_count[i];
    if (nrows <= 0) return;
    constexpr int chunk = kUpSpan;                              // what the lanes hold in registers
    const int64_t r0 = (int64_t)g.row_first[i] - g.row_base;
    T v[LOADS];
    // the loads of the chunk [u, u + len) of fine row t, LOADS per lane, none behind a branch: an element
    // behind the chunk re-reads the chunk's last
    auto load = [&](int t, int64_t u, int len) {
        const T* row = src + (r0 + t) * row_stride;
#pragma unroll
        for (int q = 0; q < LOADS; ++q) {
            int64_t c = u + min(q * lanes + tid, len - 1);
            if (c >= g.cols) c -= g.cols;
            v[q] = row[c];
        }
    };
    // where the chunk behind column `from` of a row starts. Gaps: at the lowest column any lane still has to
    // read (block-uniform, and below hi while from < hi: the lane whose run ends at hi still has one)
    auto start = [&](int64_t from) { return dense ? from : up_block_min(b > from ? up_max(a, from) : none, red); };
    int t = 0;
    int64_t u = start(lo);
    int len = (int)up_min((int64_t)chunk, hi - u);
    load(t, u, len);
    for (;;) {
#pragma unroll
        for (int q = 0; q < LOADS; ++q) {
            const int e = q * lanes + tid;
            if (e < len) tile[up_pad(e)] = v[q];
        }
        __syncthreads();
        // the next chunk's loads are in flight while this one is walked
        const bool row_ends = u + len >= hi;
        const int t2 = row_ends ? t + 1 : t;
        const bool more = t2 < nrows;
        int64_t u2 = 0;
        int len2 = 0;
        if (more) {                                             // (block-uniform)
            u2 = start(row_ends ? lo : u + len);
            len2 = (int)up_min((int64_t)chunk, hi - u2);
            load(t2, u2, len2);
        }
        const int s0 = (int)(up_max(a, u) - u), s1 = (int)(up_min(b, u + len) - u);   // s1 <= s0: nothing of this run
        for (int e = s0; e < s1; ++e) acc.value(tile[up_pad(e)]);
        if (row_ends) acc.row((int64_t)g.row_first[i] + t);
        if (!more) break;
        __syncthreads();                                        // the tile is free again
        t = t2;
        u = u2;
        len = len2;
    }
}

// (block b of the grid: span b % spans, coarse row (b / spans) % cell_rows of the launch, layer beyond)
struct UpBlock { int span, il, layer; };
__device__ __forceinline__ UpBlock up_block(const UpGeom& g) {
    const unsigned b = blockIdx.x, t = b / (unsigned)g.spans;
    return UpBlock{(int)(b % (unsigned)g.spans), (int)(t % (unsigned)g.cell_rows), (int)(t / (unsigned)g.cell_rows)};
}

struct UpMeanAcc {
    const double* area;
    double ccf;                          // float(col_count[j])
    double num = 0.0, den = 0.0, tot = 0.0, s = 0.0;
    int cnt = 0, m = 0;
    __device__ __forceinline__ void value(double x) {
#pragma clang fp contract(off)
        if (x == x) {
            s = s + x;
            ++m;
        }
    }
    __device__ __forceinline__ void row(int64_t r) {
#pragma clang fp contract(off)
        const double w = area ? area[r] : 1.0;
        const double ws = w * s, wm = w * (double)m, wc = w * ccf;
        num = num + ws;
        den = den + wm;
        tot = tot + wc;
        cnt += m;
        s = 0.0;
        m = 0;
    }
};

template <typename T, int LANES>
__global__ __launch_bounds__(LANES) void upscale_kernel(UpArgs<T> a) {
#pragma clang fp contract(off)
    __shared__ T tile[kUpTile];
    __shared__ int64_t red[kUpMaxLanes / 64];
    const UpGeom& g = a.g;
    const UpBlock blk = up_block(g);
    const int i = g.cell_row_first + blk.il, j0 = blk.span * LANES, j = j0 + (int)threadIdx.x;
    UpMeanAcc acc;
    acc.area = g.area;
    acc.ccf = j < g.coarse_cols ? (double)g.col_count[j] : 0.0;
    upscale_walk<T, LANES>(g, a.values + (int64_t)blk.layer * a.layer_stride, a.row_stride, i, j0, tile, red, acc);
    if (j >= g.coarse_cols) return;
    const double fraction = acc.tot > 0.0 ? acc.den / acc.tot : 0.0;
    const double need = a.min_fraction * acc.tot;
    const double mean = acc.cnt >= 1 && acc.den >= need ? acc.num / acc.den : __builtin_nan("");
    if (a.mean) a.mean[(int64_t)blk.layer * a.mean_layer + (int64_t)blk.il * a.mean_row + j] = (T)mean;
    if (a.fraction) a.fraction[(int64_t)blk.layer * a.fraction_layer + (int64_t)blk.il * a.fraction_row + j] = (T)fraction;
    if (a.count) a.count[(int64_t)blk.layer * a.count_layer + (int64_t)blk.il * a.count_row + j] = acc.cnt;
}

// the counters of a lane: a column of LDS, code c of lane l at c * LANES + l (a run-time index into
// registers would become scratch memory); only the lane itself reads and writes its column
struct UpClassAcc {
    unsigned* col;
    unsigned valid;
    int lanes;
    __device__ __forceinline__ void value(uint8_t x) {
        if (x < kUpCodes && ((valid >> x) & 1u)) col[(int)x * lanes] += 1u;
    }
    __device__ __forceinline__ void row(int64_t) {}
};

template <int LANES>
__global__ __launch_bounds__(LANES) void upscale_classes_kernel(UpClassArgs a) {
    __shared__ uint8_t tile[kUpTile];
    __shared__ unsigned counters[kUpCodes * LANES];
    __shared__ int64_t red[kUpMaxLanes / 64];
    const UpGeom& g = a.g;
    const UpBlock blk = up_block(g);
    constexpr int lanes = LANES;
    const int i = g.cell_row_first + blk.il, j0 = blk.span * lanes, j = j0 + (int)threadIdx.x;
    UpClassAcc acc{counters + threadIdx.x, a.valid, lanes};
    for (int c = 0; c < kUpCodes; ++c) acc.col[c * lanes] = 0u;
    upscale_walk<uint8_t, LANES>(g, a.cls, a.row_stride, i, j0, tile, red, acc);
    if (j >= g.coarse_cols) return;
    unsigned best = 0u;
    int winner = kUpNoClass;
    for (int c = 0; c < kUpCodes; ++c) {                  // a later code needs MORE pixels: the lowest code wins a tie
        const unsigned v = acc.col[c * lanes];
        if (v > best) {
            best = v;
            winner = c;
        }
    }
    const double pixels = (double)g.row_count[i] * (double)g.col_count[j];
    const float share = best ? (float)((double)best / pixels) : 0.0f;
    if (a.out_cls) a.out_cls[(int64_t)blk.il * a.cls_row + j] = (uint8_t)winner;
    if (a.out_share) a.out_share[(int64_t)blk.il * a.share_row + j] = share;
}

// ---- Row-affine columns (a sinusoidal tile; mod16_amd/upscale.py: cell_table_rows, aggregate_rows,
// majority_rows). The rows keep their run tables; the column position of pixel (r, c) is origin[r] +
// scale[r] * c, so the column run [a, b) of a cell differs from fine row to fine row and every lane finds
// its own from the two float64 of the row. up_cell alone decides which cell a pixel belongs to; the runs
// are where it changes value, found by bisection over the row's column range [first, first + n): within
// a row the host accepted (upscale.check_rows) up_cell is monotone in c -- without wrap in the unclipped
// index, with wrap as the cyclic offset from the cell of the row's first pixel, which does not lap -- in
// the direction of the scale's sign. A lane bisects for its `a`; its `b` is the `a` of the lane that owns
// the next cell in that direction (an LDS exchange), bisected only where that lane is in another block.
// Every search has at most 31 steps (n <= 2^30) and ends inside [first, first + n], whatever the
// arithmetic gave: no float result steers an address unclamped. The cost is per (fine row, cell); the walk
// has no up_cell and no division per pixel.
struct UpRowsGeom {
    const double* origin;                // [rows] position of column 0 in units of coarse cells
    const double* scale;                 // [rows] coarse cells per fine column
    const int32_t* col_first;            // [rows] the columns of a fine row that can belong to a cell, or NULL: all
    const int32_t* col_count;
    int32_t wrap;                        // 1: the coarse column axis is periodic
};

struct UpSumArgs {                       // the outputs of the sums kernels ([layers][cell_rows][coarse_cols] each, or NULL)
    double* num;
    double* den;
    double* tot;
    int64_t num_layer, num_row, den_layer, den_row, tot_layer, tot_row;
};

// upscale.cell_table on origin + scale * c, operation for operation (no contraction). wrap: the cell in
// [0, W); the quotient of pos / W is the correctly rounded IEEE division, as in ds_corners(DsRowsGrid).
// No wrap: the UNCLIPPED cell clip(floor(pos), -2, W + 1) + (f >= 0.5) in [-2, W + 2]: a value outside
// [0, W) is cell_table's -1 (no cell), and no lane looks for one.
__device__ __forceinline__ int up_cell(double origin, double scale, int c, int W, bool wrap) {
#pragma clang fp contract(off)
    const double step = scale * (double)c;
    const double pos = origin + step;
    const double size = (double)W;
    if (wrap) {
        const double turns = floor(pos / size) * size;
        double p = pos - turns;
        p = (p >= 0.0 && p < size) ? p : 0.0;
        const double fl = floor(p);
        const double f = p - fl;
        int cell = (int)fl + (f >= 0.5 ? 1 : 0);
        cell = cell >= W ? cell - W : cell;
        return cell < 0 ? 0 : (cell > W - 1 ? W - 1 : cell);         // (never taken: index safety)
    }
    const double fl = floor(pos);
    const double f = pos - fl;
    return (int)fmin(fmax(fl, -2.0), size + 1.0) + (f >= 0.5 ? 1 : 0);
}

// the runs of one fine row in a block: this lane's [a, b), the block's [lo, hi) (lo == INT_MAX: no lane
// has a pixel) and whether the runs lie back to back in it
struct UpRowRun { int a, b, lo, hi; bool dense; };

template <int LANES>
__device__ __forceinline__ UpRowRun up_find_runs(const UpGeom& g, const UpRowsGeom& rg, int64_t r, int j, int* bnd, int64_t* red) {
    const int W = g.coarse_cols, C = (int)g.cols, tid = (int)threadIdx.x;
    const bool wrap = rg.wrap != 0;
    const double origin = rg.origin[r], scale = rg.scale[r];
    int first = rg.col_first ? rg.col_first[r] : 0, n = rg.col_count ? rg.col_count[r] : C;
    first = first < 0 ? 0 : (first > C ? C : first);                  // (the host has checked the range: index safety)
    n = n < 0 ? 0 : (n > C - first ? C - first : n);
    const int end = first + n;
    UpRowRun run{end, end, INT32_MAX, 0, true};
    if (n == 0) return run;                                           // (block-uniform)
    const int sgn = scale < 0.0 ? -1 : 1;
    const int k0 = wrap ? up_cell(origin, scale, first, W, true) : 0;
    // the key of a cell: non-decreasing in c along the row
    auto key = [&](int cell) {
        int k = sgn * (cell - k0);
        return wrap && k < 0 ? k + W : k;
    };
    // the first column of [first, end) whose key is at least `want`, `end` where there is none
    auto search = [&](int want) {
        int lo = first, hi = end;
        for (int step = 0; step < 31 && lo < hi; ++step) {
            const int mid = lo + ((hi - lo) >> 1);
            if (key(up_cell(origin, scale, mid, W, wrap)) >= want) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    };
    const bool mine = j < W;
    const int want = key(j);
    const int a = mine ? search(want) : end;
    bnd[tid] = a;
    __syncthreads();
    const int nb = tid + sgn, jn = j + sgn;
    int b = end;
    if (mine && !(wrap && want + 1 >= W)) b = (nb >= 0 && nb < LANES && jn >= 0 && jn < W) ? bnd[nb] : search(want + 1);
    run.a = a;
    run.b = b < a ? a : b;
    const int cnt = run.b - run.a;
    const int64_t none = INT64_MAX;
    const int64_t lo = up_block_min(cnt ? (int64_t)run.a : none, red);      // (its barriers also free bnd)
    if (lo == none) return run;
    run.lo = (int)lo;
    run.hi = (int)-up_block_min(cnt ? -(int64_t)run.b : none, red);
    run.dense = up_block_sum(cnt, red) == (int64_t)run.hi - run.lo;
    return run;
}

// upscale_walk with the runs per fine row: for every fine row of coarse row i in run order, acc.value(x)
// for the pixels of this lane's run in increasing c, then acc.count(pixels of the run) and acc.row(r). The
// runs of the NEXT row that has a pixel in this span are found while the loads of the current chunk are in
// flight, so that the first chunk of that row can be issued right after the barrier, like any other next
// chunk. A fine row without a pixel in the span costs no load (and no acc.row: it would add +0.0 to every
// sum, which changes none of them). -> the pixels of the lane's cell. Every lane of the block calls this.
template <typename T, int LANES, typename Acc>
__device__ __forceinline__ int upscale_walk_rows(const UpGeom& g, const UpRowsGeom& rg, const T* src, int64_t row_stride,
                                                 int i, int j0, T* tile, int64_t* red, int* bnd, Acc& acc) {
    constexpr int lanes = LANES, LOADS = kUpSpan / LANES, chunk = kUpSpan;
    const int tid = (int)threadIdx.x;
    const int j = j0 + tid;
    const int nrows = g.row_count[i];
    const int64_t rf = g.row_first[i], r0 = rf - g.row_base;
    int pixels = 0;
    UpRowRun cur{0, 0, INT32_MAX, 0, true}, nxt = cur;
    // the next fine row from `t` on that has a pixel in the span (nrows: none)
    auto seek = [&](int t, UpRowRun& run) {
        for (; t < nrows; ++t) {
            run = up_find_runs<LANES>(g, rg, rf + t, j, bnd, red);
            if (run.lo != INT32_MAX) break;
        }
        return t;
    };
    int t = seek(0, cur);
    if (t >= nrows) return 0;
    T v[LOADS];
    auto load = [&](int row, int u, int len) {
        const T* p = src + (r0 + row) * row_stride + u;
#pragma unroll
        for (int q = 0; q < LOADS; ++q) v[q] = p[min(q * lanes + tid, len - 1)];
    };
    const int64_t none = INT64_MAX;
    auto start = [&](const UpRowRun& run, int from) {
        return run.dense ? from : (int)up_block_min(run.b > from ? (int64_t)max(run.a, from) : none, red);
    };
    int u = start(cur, cur.lo);
    int len = min(chunk, cur.hi - u);
    load(t, u, len);
    int tn = 0;
    bool sought = false;
    for (;;) {
        if (!sought) {                                          // (block-uniform) while the loads are in flight
            tn = seek(t + 1, nxt);
            sought = true;
        }
#pragma unroll
        for (int q = 0; q < LOADS; ++q) {
            const int e = q * lanes + tid;
            if (e < len) tile[up_pad(e)] = v[q];
        }
        __syncthreads();
        const bool row_ends = u + len >= cur.hi;
        const bool more = row_ends ? tn < nrows : true;
        int u2 = 0, len2 = 0;
        if (more) {                                             // (block-uniform)
            u2 = row_ends ? start(nxt, nxt.lo) : start(cur, u + len);
            len2 = min(chunk, (row_ends ? nxt.hi : cur.hi) - u2);
            load(row_ends ? tn : t, u2, len2);
        }
        const int s0 = max(cur.a, u) - u, s1 = min(cur.b, u + len) - u;      // s1 <= s0: nothing of this run
        for (int e = s0; e < s1; ++e) acc.value(tile[up_pad(e)]);
        if (row_ends) {
            acc.count(cur.b - cur.a);
            acc.row(rf + t);
            pixels += cur.b - cur.a;
        }
        if (!more) break;
        __syncthreads();                                        // the tile is free again
        if (row_ends) {
            cur = nxt;
            t = tn;
            sought = false;
        }
        u = u2;
        len = len2;
    }
    return pixels;
}

// UpMeanAcc with the pixel count of the lane's run set per fine row
struct UpRowsMeanAcc : UpMeanAcc {
    __device__ __forceinline__ void count(int n) { ccf = (double)n; }
};
struct UpRowsClassAcc : UpClassAcc {
    __device__ __forceinline__ void count(int) {}
};

// The mean kernel of the row-affine geometry (ROWS) and the sums kernels of both geometries (SUMS: num,
// den, tot and count instead of mean, fraction and count): upscale_kernel with another walk and / or
// other stores. (ROWS = false, SUMS = false is upscale_kernel itself and is not instantiated.)
template <typename T, int LANES, bool ROWS, bool SUMS>
__global__ __launch_bounds__(LANES) void upscale_ext_kernel(UpArgs<T> a, UpRowsGeom rg, UpSumArgs sm) {
#pragma clang fp contract(off)
    __shared__ T tile[kUpTile];
    __shared__ int64_t red[kUpMaxLanes / 64];
    __shared__ int bnd[ROWS ? LANES : 1];
    const UpGeom& g = a.g;
    const UpBlock blk = up_block(g);
    const int i = g.cell_row_first + blk.il, j0 = blk.span * LANES, j = j0 + (int)threadIdx.x;
    UpRowsMeanAcc acc;
    acc.area = g.area;
    const T* src = a.values + (int64_t)blk.layer * a.layer_stride;
    if constexpr (ROWS) {
        acc.ccf = 0.0;
        upscale_walk_rows<T, LANES>(g, rg, src, a.row_stride, i, j0, tile, red, bnd, acc);
    } else {
        acc.ccf = j < g.coarse_cols ? (double)g.col_count[j] : 0.0;
        upscale_walk<T, LANES>(g, src, a.row_stride, i, j0, tile, red, acc);
    }
    if (j >= g.coarse_cols) return;
    if constexpr (SUMS) {
        if (sm.num) sm.num[(int64_t)blk.layer * sm.num_layer + (int64_t)blk.il * sm.num_row + j] = acc.num;
        if (sm.den) sm.den[(int64_t)blk.layer * sm.den_layer + (int64_t)blk.il * sm.den_row + j] = acc.den;
        if (sm.tot) sm.tot[(int64_t)blk.layer * sm.tot_layer + (int64_t)blk.il * sm.tot_row + j] = acc.tot;
    } else {
        const double fraction = acc.tot > 0.0 ? acc.den / acc.tot : 0.0;
        const double need = a.min_fraction * acc.tot;
        const double mean = acc.cnt >= 1 && acc.den >= need ? acc.num / acc.den : __builtin_nan("");
        if (a.mean) a.mean[(int64_t)blk.layer * a.mean_layer + (int64_t)blk.il * a.mean_row + j] = (T)mean;
        if (a.fraction) a.fraction[(int64_t)blk.layer * a.fraction_layer + (int64_t)blk.il * a.fraction_row + j] = (T)fraction;
    }
    if (a.count) a.count[(int64_t)blk.layer * a.count_layer + (int64_t)blk.il * a.count_row + j] = acc.cnt;
}

template <int LANES>
__global__ __launch_bounds__(LANES) void upscale_classes_rows_kernel(UpClassArgs a, UpRowsGeom rg) {
    __shared__ uint8_t tile[kUpTile];
    __shared__ unsigned counters[kUpCodes * LANES];
    __shared__ int64_t red[kUpMaxLanes / 64];
    __shared__ int bnd[LANES];
    const UpGeom& g = a.g;
    const UpBlock blk = up_block(g);
    constexpr int lanes = LANES;
    const int i = g.cell_row_first + blk.il, j0 = blk.span * lanes, j = j0 + (int)threadIdx.x;
    UpRowsClassAcc acc{{counters + threadIdx.x, a.valid, lanes}};
    for (int c = 0; c < kUpCodes; ++c) acc.col[c * lanes] = 0u;
    const int cell = upscale_walk_rows<uint8_t, LANES>(g, rg, a.cls, a.row_stride, i, j0, tile, red, bnd, acc);
    if (j >= g.coarse_cols) return;
    unsigned best = 0u;
    int winner = kUpNoClass;
    for (int c = 0; c < kUpCodes; ++c) {                  // a later code needs MORE pixels: the lowest code wins a tie
        const unsigned v = acc.col[c * lanes];
        if (v > best) {
            best = v;
            winner = c;
        }
    }
    const double pixels = (double)cell;
    const float share = best ? (float)((double)best / pixels) : 0.0f;
    if (a.out_cls) a.out_cls[(int64_t)blk.il * a.cls_row + j] = (uint8_t)winner;
    if (a.out_share) a.out_share[(int64_t)blk.il * a.share_row + j] = share;
}

}  // namespace mod16
