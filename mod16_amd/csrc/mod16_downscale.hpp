// Downscaled forward run (gfx950): ET day and night for a contiguous range of pixels of an R x C
// fine raster whose drivers are scalars, fine arrays or COARSE H x W arrays interpolated per pixel
// inside the kernel -- mod16_et_downscaled_*; mod16_downscale_fields_* writes the interpolated fields
// alone. The definition is the numpy statement mod16_amd/downscale.py (corner_tables, interpolate);
// ds_interp follows interpolate operation for operation, and the interpolated values never touch
// memory.
//
// One lane per pixel, the block and grid shapes of ens_kernel. The pixel index becomes (r, c) by one
// 64-bit division per batch of 256 pixels (block-uniform) and a 32-bit division per lane; the lane
// reads its row's and its column's table entry (two cell indices, two weights: computed and
// validated on the host, mod16_downscale_create), forms the four corner weights and offsets once,
// and gathers four cells of every coarse driver. Consecutive pixels of a row share the row entry
// and almost always the column pair, so a wave's 4 x 64 addresses of one driver fall into a
// handful of cache lines: the coarse planes (a few hundred thousand values) are read through the
// vector cache, plain gathers -- no LDS stage (a batch spans several rows of any width: its cells
// are no rectangle known in advance), no repacked copy (the planes are the caller's, whole).
// Which drivers are coarse is a mask in the arguments, tested by wave-uniform branches: a dense
// driver costs one load, a coarse one four. All loads of a pixel are issued in front of the
// interpolation arithmetic. Values and arithmetic are float64 whatever T is; float32 storage
// widens, computes in float64 and rounds once on store.
//
// Domain guard: as in the ensemble and composite families. fast_out_of_domain(x) on the
// interpolated pixel; a flagged pixel gets a NaN with a payload of its own (DsMark) in out_night and
// ds_redo_kernel, launched behind ds_kernel, recomputes it with et_pixel_exact. No atomics on
// results, no workspace: two launches give the same bits, and no output keeps the mark.
//
// Index safety: every coarse index comes from the handle's tables (validated against H and W on
// the host), every fine index from the pixel range (validated against R x C); no driver value
// steers an address. In the row-affine geometry (DsRowsGrid) the column pair is computed by the
// lane from the row's (origin, scale), which the host has validated as finite with a finite far
// end, so every position is finite. The argument does not lean on that: the clamped position is
// the result of min / max against 0 and W - 1, the wrapped one is replaced by 0 unless
// 0 <= p < W holds (a comparison that a NaN fails), and the converted cell index is clamped to
// [0, W - 1] as an integer once more, so no computed value, NaN and infinity included, steers an
// address outside [0, W); i1 is formed from i0 by integer arithmetic alone.
#pragma once
#include "mod16_composite.hpp"

namespace mod16 {

constexpr int kDsMaxFields = 16;         // fields of one ds_fields_kernel launch

// The corner tables of a grid handle on the device, and the fine raster's width
struct DsGrid {
    const int32_t* ri0;      // [R] near and far coarse row of every fine row
    const int32_t* ri1;
    const double* rw0;       // [R] their weights
    const double* rw1;
    const int32_t* ci0;      // [C] the same per fine column
    const int32_t* ci1;
    const double* cw0;
    const double* cw1;
    int32_t cols;            // C
};

// The row-affine geometry (mod16_amd/downscale.py: corner_tables_rows): the rows keep their tables,
// the column position of pixel (r, c) is origin[r] + scale[r] * c and its cell pair and weights are
// formed by the lane (sinusoidal tiles: the longitude of a column depends on the row)
struct DsRowsGrid {
    const int32_t* ri0;      // [R] as in DsGrid
    const int32_t* ri1;
    const double* rw0;
    const double* rw1;
    const double* origin;    // [R] position of column 0 in units of coarse cells
    const double* scale;     // [R] coarse cells per fine column
    int32_t cols;            // C
    int32_t width;           // W: the coarse grid's columns
    int32_t wrap;            // 1: the coarse column axis is periodic
    int32_t nearest;         // 1: 'nearest', 0: 'bilinear'
};

template <typename T, typename G = DsGrid> struct DsArgs {
    const T* drv[14];               // scalar: one value; fine: from the range's first pixel; coarse: a whole plane
    uint32_t dense;                 // bit k set: driver k is a fine array
    uint32_t coarse;                // bit k set: driver k is a coarse plane
    G g;
    int64_t cpitch;                 // elements between two rows of a coarse plane
    int64_t first, n;               // the pixel range [first, first + n) of the raster
    const uint8_t* cls;
    const double* lut64;            // device [MOD16_LUT_ROWS][kLutCols]
    const double* tab;              // exp / log tables of FastMath<double>
    T* out_day;
    T* out_night;
    unsigned* status;
};

// What a launch of the fields is given apart from the geometry (CdArgs has the same shape: `c`, then `g`)
template <typename T> struct DsFields {
    const T* field[kDsMaxFields];   // coarse planes
    T* out;                         // [nfields][out_pitch]
    int nfields;
    int64_t cpitch, first, n, out_pitch;
};
template <typename T, typename G = DsGrid> struct DsFieldArgs {
    DsFields<T> c;
    G g;                            // DsGrid (column tables) or DsRowsGrid (row-affine columns)
};

// What ds_kernel leaves in out_night of a pixel outside the domain of the fast arithmetic (a quiet
// NaN, payload "d05ca")
template <typename T> struct DsMark;
template <> struct DsMark<double> {
    static constexpr unsigned long long bits = 0x7ff80000000d05caull;
    static __device__ __forceinline__ double value() { return __longlong_as_double((long long)bits); }
    static __device__ __forceinline__ bool is(double v) { return (unsigned long long)__double_as_longlong(v) == bits; }
};
template <> struct DsMark<float> {
    static constexpr unsigned bits = 0x7fcd05cau;
    static __device__ __forceinline__ float value() { return __uint_as_float(bits); }
    static __device__ __forceinline__ bool is(float v) { return __float_as_uint(v) == bits; }
};

// A pixel's four corners: offsets into a coarse plane and weights, in the order (row i0, col i0),
// (i0, i1), (i1, i0), (i1, i1)
struct DsCorners {
    int64_t o[4];
    double w[4];
};

// (r, c) of pixel `first + b * 256 + lane`: row0 / col0 are the batch's first pixel (one 64-bit
// division per batch, block-uniform), the lane adds its carry with a 32-bit division
// (col0 + lane < 2^30 + 256)
__device__ __forceinline__ DsCorners ds_corners(const DsGrid& g, int64_t cpitch, int64_t row0, uint32_t col0, uint32_t lane) {
#pragma clang fp contract(off)
    const uint32_t cc = col0 + lane;
    const uint32_t q = cc / (uint32_t)g.cols;
    const uint32_t c = cc - q * (uint32_t)g.cols;
    const int64_t r = row0 + q;
    const int64_t r0 = (int64_t)g.ri0[r] * cpitch, r1 = (int64_t)g.ri1[r] * cpitch;
    const int64_t c0 = g.ci0[c], c1 = g.ci1[c];
    const double wr0 = g.rw0[r], wr1 = g.rw1[r], wc0 = g.cw0[c], wc1 = g.cw1[c];
    DsCorners k;
    k.o[0] = r0 + c0;
    k.o[1] = r0 + c1;
    k.o[2] = r1 + c0;
    k.o[3] = r1 + c1;
    k.w[0] = wr0 * wc0;
    k.w[1] = wr0 * wc1;
    k.w[2] = wr1 * wc0;
    k.w[3] = wr1 * wc1;
    return k;
}

// The same in the row-affine geometry: the row's table entry as above, the column pair and its
// weights from the row's (origin, scale) -- downscale.corner_tables on origin + scale * c, operation
// for operation, no contraction: one multiplication and one addition (each rounded), clamp or wrap
// (the quotient of pos / W is the correctly rounded one: the compiler's IEEE float64 division),
// floor, f, the far cell, w1, w0 = 1.0 - w1. `wrap` and `nearest` are wave-uniform. Some fifteen
// float64 operations per pixel (the division's refinement steps among them), once per pixel and
// outside every day loop.
__device__ __forceinline__ DsCorners ds_corners(const DsRowsGrid& g, int64_t cpitch, int64_t row0, uint32_t col0, uint32_t lane) {
#pragma clang fp contract(off)
    const uint32_t cc = col0 + lane;
    const uint32_t q = cc / (uint32_t)g.cols;
    const uint32_t c = cc - q * (uint32_t)g.cols;
    const int64_t r = row0 + q;
    const int64_t r0 = (int64_t)g.ri0[r] * cpitch, r1 = (int64_t)g.ri1[r] * cpitch;
    const double wr0 = g.rw0[r], wr1 = g.rw1[r];
    const double step = g.scale[r] * (double)c;
    const double pos = g.origin[r] + step;
    const int32_t W = g.width;
    const double size = (double)W;
    double p;
    if (g.wrap) {
        const double turns = floor(pos / size) * size;
        p = pos - turns;
        p = (p >= 0.0 && p < size) ? p : 0.0;        // (a NaN fails the comparison and lands on 0 too)
    } else {
        p = fmin(fmax(pos, 0.0), (double)(W - 1));
    }
    const double fl = floor(p);
    const double f = p - fl;
    int32_t i0 = (int32_t)fl;
    i0 = i0 < 0 ? 0 : (i0 > W - 1 ? W - 1 : i0);         // (never taken for a validated handle: index safety)
    const int32_t i1 = g.wrap ? (i0 + 1 == W ? 0 : i0 + 1) : (i0 + 1 < W - 1 ? i0 + 1 : W - 1);
    const double wc1 = g.nearest ? (f >= 0.5 ? 1.0 : 0.0) : f;
    const double wc0 = 1.0 - wc1;
    const int64_t c0 = i0, c1 = i1;
    DsCorners k;
    k.o[0] = r0 + c0;
    k.o[1] = r0 + c1;
    k.o[2] = r1 + c0;
    k.o[3] = r1 + c1;
    k.w[0] = wr0 * wc0;
    k.w[1] = wr0 * wc1;
    k.w[2] = wr1 * wc0;
    k.w[3] = wr1 * wc1;
    return k;
}

// downscale.interpolate for one pixel from its four cell values: a corner without weight gives
// +0.0 whatever its cell holds; left to right, no contraction
__device__ __forceinline__ double ds_interp(const DsCorners& k, double v00, double v01, double v10, double v11) {
#pragma clang fp contract(off)
    const double t00 = (k.w[0] != 0.0) ? k.w[0] * v00 : 0.0;
    const double t01 = (k.w[1] != 0.0) ? k.w[1] * v01 : 0.0;
    const double t10 = (k.w[2] != 0.0) ? k.w[2] * v10 : 0.0;
    const double t11 = (k.w[3] != 0.0) ? k.w[3] * v11 : 0.0;
    return ((t00 + t01) + t10) + t11;
}

// a period's total from its components, as the step kernels add them (:792): no contraction
__device__ __forceinline__ double ds_total(double canopy, double soil, double trans) {
#pragma clang fp contract(off)
    return (canopy + soil) + trans;
}

// The 14 driver values of pixel i of the range (its corners in k): every load first, in the storage
// type, under wave-uniform branches; the arithmetic behind them
template <typename T, typename G>
__device__ __forceinline__ PixelIn<double> ds_pixel(const DsArgs<T, G>& a, int64_t i, const DsCorners& k) {
    T raw[14][4];
#pragma unroll
    for (int d = 0; d < 14; ++d) {
        if ((a.coarse >> d) & 1u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[d][j] = a.drv[d][k.o[j]];
        } else {
            raw[d][0] = a.drv[d][((a.dense >> d) & 1u) ? i : 0];
            raw[d][1] = raw[d][2] = raw[d][3] = (T)0;
        }
    }
    double v[14];
#pragma unroll
    for (int d = 0; d < 14; ++d) {
        if ((a.coarse >> d) & 1u)
            v[d] = ds_interp(k, (double)raw[d][0], (double)raw[d][1], (double)raw[d][2], (double)raw[d][3]);
        else
            v[d] = (double)raw[d][0];
    }
    return PixelIn<double>{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13]};
}

// 256-thread blocks over batches of 256 pixels; the batch loop is block-uniform, the threads past
// the range's end compute on its last pixel and store nothing. G: the geometry, DsGrid (column
// tables) or DsRowsGrid (row-affine columns).
template <typename T, bool FAST, typename G = DsGrid>
__global__ void __launch_bounds__(kBlock, FAST ? 2 : 1) ds_kernel(const DsArgs<T, G> a) {
    constexpr int kTab = FAST ? FastMath<double>::kTabDoubles : 1;
    __shared__ __attribute__((aligned(16))) double lut[MOD16_LUT_ROWS * kLutCols];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    if constexpr (FAST) {
        ignore_signalling_nans();                  // the domain guard's NaN-ignoring chain
        for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.tab[i];
    }
    for (int i = threadIdx.x; i < MOD16_LUT_ROWS * kLutCols; i += kBlock) lut[i] = a.lut64[i];
    __syncthreads();
    const int64_t nbatch = (a.n + kBlock - 1) / kBlock;
    const int64_t last = a.first + a.n - 1;
    const int64_t last_row = last / a.g.cols;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i0 = b * kBlock + threadIdx.x;
        const bool live = i0 < a.n;
        const int64_t i = live ? i0 : a.n - 1;
        DsCorners k;
        if (live) {
            const int64_t p0 = a.first + b * kBlock;       // the batch's first pixel in the raster
            const int64_t row0 = p0 / a.g.cols;
            k = ds_corners(a.g, a.cpitch, row0, (uint32_t)(p0 - row0 * a.g.cols), threadIdx.x);
        } else {
            k = ds_corners(a.g, a.cpitch, last_row, (uint32_t)(last - last_row * a.g.cols), 0u);
        }
        unsigned c = a.cls[i];
        if (c >= 13u) {   // numpy would raise IndexError: flag it, give NaN
            atomicOr(a.status, kStatusClassRange);
            c = 13u;
        }
        const PixelIn<double> x = ds_pixel(a, i, k);
        const ClassPar<double> p = comp_params(lut + c);
        if constexpr (FAST) {
            const bool bad = fast_out_of_domain(x);
            const PixelOut<double> o = et_pixel_fast<double, false>(x, p, tab);
            if (live) {
                // a pixel outside the domain of the strength-reduced arithmetic leaves the mark for
                // ds_redo_kernel, which runs behind this kernel (mod16_physics.hpp, "domain guard")
                if (bad) {
                    a.out_night[i] = DsMark<T>::value();
                } else {
                    a.out_day[i] = (T)ds_total(o.canopy_d, o.soil_d, o.trans_d);
                    a.out_night[i] = (T)ds_total(o.canopy_n, o.soil_n, o.trans_n);
                }
            }
        } else {
            const PixelOut<double> o = et_pixel_exact<double, false, true>(x, p);
            if (live) {
                a.out_day[i] = (T)ds_total(o.canopy_d, o.soil_d, o.trans_d);
                a.out_night[i] = (T)ds_total(o.canopy_n, o.soil_n, o.trans_n);
            }
        }
    }
}

// Behind ds_kernel<T, true>: the marked pixels in the reference's operation order.
template <typename T, typename G = DsGrid>
__global__ void __launch_bounds__(kBlock, 1) ds_redo_kernel(const DsArgs<T, G> a) {
    __shared__ __attribute__((aligned(16))) double lut[MOD16_LUT_ROWS * kLutCols];
    for (int i = threadIdx.x; i < MOD16_LUT_ROWS * kLutCols; i += kBlock) lut[i] = a.lut64[i];
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += step) {
        if (!DsMark<T>::is(a.out_night[i])) continue;
        const int64_t g = a.first + i;
        const int64_t row = g / a.g.cols;
        const DsCorners k = ds_corners(a.g, a.cpitch, row, (uint32_t)(g - row * a.g.cols), 0u);
        unsigned c = a.cls[i];
        c = c >= 13u ? 13u : c;        // (ds_kernel has flagged it)
        const PixelIn<double> x = ds_pixel(a, i, k);
        const PixelOut<double> o = et_pixel_exact<double, false, true>(x, comp_params(lut + c));
        a.out_day[i] = (T)ds_total(o.canopy_d, o.soil_d, o.trans_d);
        a.out_night[i] = (T)ds_total(o.canopy_n, o.soil_n, o.trans_n);
    }
}

// The interpolated fields alone: out[f][i] for the pixels of the range, through ds_interp.
template <typename T, typename G = DsGrid>
__global__ void __launch_bounds__(kBlock) ds_fields_kernel(const DsFieldArgs<T, G> a) {
    const int64_t nbatch = (a.c.n + kBlock - 1) / kBlock;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i = b * kBlock + threadIdx.x;
        if (i >= a.c.n) continue;
        const int64_t p0 = a.c.first + b * kBlock;
        const int64_t row0 = p0 / a.g.cols;
        const DsCorners k = ds_corners(a.g, a.c.cpitch, row0, (uint32_t)(p0 - row0 * a.g.cols), threadIdx.x);
#pragma nounroll
        for (int f = 0; f < a.c.nfields; ++f) {
            const T* src = a.c.field[f];
            const double v = ds_interp(k, (double)src[k.o[0]], (double)src[k.o[1]], (double)src[k.o[2]], (double)src[k.o[3]]);
            a.c.out[(int64_t)f * a.c.out_pitch + i] = (T)v;
        }
    }
}

}  // namespace mod16
