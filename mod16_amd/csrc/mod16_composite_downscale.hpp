// Multi-day ET composites over coarse-grid meteorology (gfx950): the period totals of
// mod16_composite.hpp for a contiguous range of pixels of an R x C fine raster, each of the 15 arrays
// a scalar, a fine array or a COARSE series of H x W planes interpolated per pixel inside the kernel
// -- mod16_et_composite_downscaled_*. No new numerics: the result is what comp_kernel gives on the
// arrays downscale.interpolate materialises slab by slab, bit for bit (ds_interp, the pixel
// functions, comp_totals, CompAcc and comp_store are the ones of the two families).
//
// One lane per pixel, batches of 256; the batch, period and day loops are block-uniform. A lane
// forms its four corners once per pixel (ds_corners: 32-bit cell offsets that all coarse arrays
// share, four weights: 12 registers) and walks the days. Every array has ONE scalar base -- the
// plane, or the fine slab, of the day's time slab: base + slab x time stride, wave-uniform -- so
// comp_kernel's 15 per-lane pointers are gone (30 registers); a fine array adds the lane's pixel,
// a coarse one the lane's four cell offsets.
//   fine array    its value of day t + 1 is issued in front of day t's arithmetic and waits in a
//                 register behind it, as in comp_kernel;
//   coarse array  four gathers per turn of its slab index. 15 x 4 raw values cannot wait across
//                 the day's arithmetic (88 registers for the eleven reanalysis drivers in float64),
//                 so they are issued at the DAY BOUNDARY, when the pixel function's temporaries are
//                 dead, in groups of kCdGroup arrays: a group's gathers first, then its
//                 interpolations straight into cur[] (all 15 at once took 410 registers, groups of
//                 eight 290, of four 256, of three 249 in the float64 instance with potential ET).
//                 The second wave per SIMD computes meanwhile.
// The reference-order instance loads everything at the day boundary.
//
// Domain guard: as in the composite family. A pixel with a flagged day gets CompMark in period 0 of
// out_et and cd_redo_kernel, launched behind cd_kernel, computes all its periods: a flagged day by
// et_pixel_exact, every other day by et_pixel_fast. No atomics on results, no workspace: two launches
// give the same bits, and no output keeps the mark.
//
// Index safety: as in ds_kernel. Coarse indices come from the handle's tables (validated against H
// and W on the host; (H - 1) x pitch + W <= 2^31 - 1 for this entry), time offsets from validated
// strides and `every`, fine indices from the pixel range (validated against R x C); no driver value
// steers an address. In the row-affine geometry the lane computes its column pair; ds_corners
// (DsRowsGrid) clamps the cell index to [0, W - 1] whatever the arithmetic gave, a NaN included, so
// the narrowed offsets stay inside the plane the entry point has measured.
#pragma once
#include "mod16_downscale.hpp"

namespace mod16 {

constexpr int kCdGroup = 3;         // coarse arrays whose cells are in flight together at a day boundary

template <typename T, typename G = DsGrid> struct CdArgs {
    CompArgs<T> c;                  // arr[k]: scalar: one value; fine: from the range's first pixel (`dense`);
                                    // coarse: the plane of time slab 0 -- tstride[k] elements between two planes
    uint32_t coarse;                // bit k set: array k is a series of coarse planes (bit 14: the hours)
    G g;                            // DsGrid (column tables) or DsRowsGrid (row-affine columns)
    int64_t cpitch;                 // elements between two rows of a coarse plane
    int64_t first;                  // the range's first pixel in the raster
};

// ds_corners with the offsets narrowed to 32 bits (the entry point refuses larger planes)
struct CdCorners {
    uint32_t o[4];
    double w[4];
};

// the corners of pixel `pixel + lane` of the raster (one 64-bit division: block-uniform where
// `pixel` is a batch's first, the lane adds its carry: ds_corners)
template <typename G>
__device__ __forceinline__ CdCorners cd_corners(const G& g, int64_t cpitch, int64_t pixel, uint32_t lane) {
    const int64_t row0 = pixel / g.cols;
    const DsCorners k = ds_corners(g, cpitch, row0, (uint32_t)(pixel - row0 * g.cols), lane);
    CdCorners c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c.o[j] = (uint32_t)k.o[j];
        c.w[j] = k.w[j];
    }
    return c;
}

// ds_interp of four cells in the storage type
template <typename T>
__device__ __forceinline__ double cd_interp(const CdCorners& c, const T (&h)[4]) {
    DsCorners k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k.o[j] = 0;
        k.w[j] = c.w[j];
    }
    return ds_interp(k, (double)h[0], (double)h[1], (double)h[2], (double)h[3]);
}

// The coarse arrays [K0, K1) named in `which` (wave-uniform) from their current planes: every gather
// first, then the interpolations into cur[]
template <typename T, int K0, int K1>
__device__ __forceinline__ void cd_gather(const T* const (&base)[kCompArrays], uint32_t which, const CdCorners& cn,
                                          double (&cur)[kCompArrays]) {
    T cell[K1 - K0][4];
#pragma unroll
    for (int k = K0; k < K1; ++k)
        if ((which >> k) & 1u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cell[k - K0][j] = base[k][cn.o[j]];
        }
#pragma unroll
    for (int k = K0; k < K1; ++k)
        if ((which >> k) & 1u) cur[k] = cd_interp<T>(cn, cell[k - K0]);
}

// ... group by group (kCdGroup arrays: what a group's cells take must fit beside cur[], the
// fine arrays' prefetch and the class parameters)
template <typename T, int K0 = 0>
__device__ __forceinline__ void cd_gather_all(const T* const (&base)[kCompArrays], uint32_t which, const CdCorners& cn,
                                              double (&cur)[kCompArrays]) {
    constexpr int K1 = K0 + kCdGroup < kCompArrays ? K0 + kCdGroup : kCompArrays;
    cd_gather<T, K0, K1>(base, which, cn, cur);
    if constexpr (K1 < kCompArrays) cd_gather_all<T, K1>(base, which, cn, cur);
}

// Once per day. The lane's pixel and cell offsets are what every address of the day loop is formed
// from: left to itself the compiler forms the 15 fine and the 4 widened coarse offsets once per
// pixel and keeps them -- comp_kernel's per-lane pointers again, 38 vector registers. Likewise it
// reads all 15 time strides and divisors (45 scalar registers) in front of the loops and then
// parks them, with the bases and count-downs they crowd out, in lanes of vector registers: 336
// scalar spills and 3 vector ones in the float64 fast instance with potential ET, against 187 and
// none with the tables read where an array turns (a scalar load from the kernel's arguments). An
// empty statement that "writes" the five offsets, and a zero the compiler cannot see through that
// the fast instances add to the tables' indices, keep both where they are used.
__device__ __forceinline__ int cd_keep_in_loop(int64_t& i, CdCorners& cn) {
    int zero = 0;
    asm volatile("" : "+v"(i), "+v"(cn.o[0]), "+v"(cn.o[1]), "+v"(cn.o[2]), "+v"(cn.o[3]), "+s"(zero));
    return zero;
}

// 256-thread blocks over batches of 256 pixels; the threads past the range's end compute on its last
// pixel and store nothing. Launch bounds as comp_kernel's.
template <typename T, bool FAST, bool PET, typename G = DsGrid>
__global__ void __launch_bounds__(kBlock, FAST ? 2 : 1) cd_kernel(const CdArgs<T, G> a) {
    constexpr int kTab = FAST ? FastMath<double>::kTabDoubles : 1;
    __shared__ __attribute__((aligned(16))) double lut[MOD16_LUT_ROWS * kLutCols];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    if constexpr (FAST) {
        ignore_signalling_nans();                  // the domain guard's NaN-ignoring chain
        for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.c.tab[i];
    }
    for (int i = threadIdx.x; i < MOD16_LUT_ROWS * kLutCols; i += kBlock) lut[i] = a.c.lut64[i];
    __syncthreads();
    const int K = a.c.days, L = a.c.period_days;
    const int64_t n = a.c.n;
    const int64_t nbatch = (n + kBlock - 1) / kBlock;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i0 = b * kBlock + threadIdx.x;
        const bool live = i0 < n;
        int64_t i = live ? i0 : n - 1;
        CdCorners cn = live ? cd_corners(a.g, a.cpitch, a.first + b * kBlock, threadIdx.x)
                            : cd_corners(a.g, a.cpitch, a.first + n - 1, 0u);
        unsigned c = a.c.cls[i];
        if (c >= 13u) {   // numpy would raise IndexError: flag it, give NaN
            atomicOr(a.c.status, kStatusClassRange);
            c = 13u;
        }
        // day 0's values; base[k]: the array's current time slab, left[k]: days until it changes (wave-uniform)
        const T* base[kCompArrays];
        double cur[kCompArrays];
        int left[kCompArrays];
#pragma unroll
        for (int k = 0; k < kCompArrays; ++k) {
            base[k] = a.c.arr[k];
            left[k] = a.c.every[k];
            if (!((a.coarse >> k) & 1u)) cur[k] = (double)base[k][((a.c.dense >> k) & 1u) ? i : 0];
        }
        cd_gather_all<T>(base, a.coarse, cn, cur);
        bool bad = false;
        int t = 0, period = 0;
        if constexpr (FAST) {
            const ClassPar<double> p = comp_params(lut + c);
            T nxt[kCompArrays];        // the fine arrays' next values, in the storage type
#pragma nounroll
            for (int t0 = 0; t0 < K; t0 += L, ++period) {
                const int len = (K - t0 < L) ? K - t0 : L;
                CompAcc et, pet;
                et.reset();
                pet.reset();
#pragma nounroll
                for (int d = 0; d < len; ++d, ++t) {
                    const int z = cd_keep_in_loop(i, cn);
                    // day t + 1: every turning array's base moves; a fine array's value is issued here,
                    // in front of day t's arithmetic
                    const bool more = t + 1 < K;
                    uint32_t turn = 0;
#pragma unroll
                    for (int k = 0; k < kCompArrays; ++k) {
                        if ((--left[k] == 0) & more) {
                            turn |= 1u << k;
                            base[k] += a.c.tstride[k + z];
                            left[k] = a.c.every[k + z];
                            if (!((a.coarse >> k) & 1u)) nxt[k] = base[k][((a.c.dense >> k) & 1u) ? i : 0];
                        }
                    }
                    const PixelIn<double> x = comp_pixel(cur);
                    bad |= fast_out_of_domain(x);
                    const PixelOut<double> o = et_pixel_fast<double, PET>(x, p, tab);
                    double v_et, v_pet;
                    comp_totals<PET>(o, cur[kCompHours], v_et, v_pet);
                    et.add(v_et);
                    if constexpr (PET) pet.add(v_pet);
                    // the day boundary: the turning coarse arrays' cells, then the fine arrays' values
                    cd_gather_all<T>(base, turn & a.coarse, cn, cur);
#pragma unroll
                    for (int k = 0; k < kCompArrays; ++k)
                        if (((turn & ~a.coarse) >> k) & 1u) cur[k] = (double)nxt[k];
                }
                if (live & !bad) comp_store<T, PET>(a.c, i, period, len, et, pet);
            }
            // a day outside the domain of the strength-reduced arithmetic: the mark for
            // cd_redo_kernel, which runs behind this kernel (mod16_physics.hpp, "domain guard")
            if (live & bad) a.c.out_et[i] = CompMark<T>::value();
        } else {
#pragma nounroll
            for (int t0 = 0; t0 < K; t0 += L, ++period) {
                const int len = (K - t0 < L) ? K - t0 : L;
                CompAcc et, pet;
                et.reset();
                pet.reset();
#pragma nounroll
                for (int d = 0; d < len; ++d, ++t) {
                    cd_keep_in_loop(i, cn);
                    const PixelIn<double> x = comp_pixel(cur);
                    const PixelOut<double> o = et_pixel_exact<double, PET, true>(x, comp_params(lut + c));
                    double v_et, v_pet;
                    comp_totals<PET>(o, cur[kCompHours], v_et, v_pet);
                    et.add(v_et);
                    if constexpr (PET) pet.add(v_pet);
                    const bool more = t + 1 < K;
                    uint32_t turn = 0;
#pragma unroll
                    for (int k = 0; k < kCompArrays; ++k)
                        if ((--left[k] == 0) & more) {
                            turn |= 1u << k;
                            base[k] += a.c.tstride[k];
                            left[k] = a.c.every[k];
                            if (!((a.coarse >> k) & 1u)) cur[k] = (double)base[k][((a.c.dense >> k) & 1u) ? i : 0];
                        }
                    cd_gather_all<T>(base, turn & a.coarse, cn, cur);
                }
                if (live) comp_store<T, PET>(a.c, i, period, len, et, pet);
            }
        }
    }
}

// Behind cd_kernel<T, true, PET>: all periods of the marked pixels; a day outside the domain in the
// reference's operation order, every other day by the fast pixel function.
template <typename T, bool PET, typename G = DsGrid>
__global__ void __launch_bounds__(kBlock, 1) cd_redo_kernel(const CdArgs<T, G> a) {
    constexpr int kTab = FastMath<double>::kTabDoubles;
    __shared__ __attribute__((aligned(16))) double lut[MOD16_LUT_ROWS * kLutCols];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    ignore_signalling_nans();
    for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.c.tab[i];
    for (int i = threadIdx.x; i < MOD16_LUT_ROWS * kLutCols; i += kBlock) lut[i] = a.c.lut64[i];
    __syncthreads();
    const int K = a.c.days, L = a.c.period_days;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.c.n; i += step) {
        if (!CompMark<T>::is(a.c.out_et[i])) continue;
        const CdCorners cn = cd_corners(a.g, a.cpitch, a.first + i, 0u);
        unsigned c = a.c.cls[i];
        c = c >= 13u ? 13u : c;        // (cd_kernel has flagged it)
        int period = 0;
#pragma nounroll
        for (int t0 = 0; t0 < K; t0 += L, ++period) {
            const int len = (K - t0 < L) ? K - t0 : L;
            CompAcc et, pet;
            et.reset();
            pet.reset();
#pragma nounroll
            for (int t = t0; t < t0 + len; ++t) {
                double v[kCompArrays];
#pragma unroll
                for (int k = 0; k < kCompArrays; ++k) {
                    const T* base = a.c.arr[k] + (int64_t)(t / a.c.every[k]) * a.c.tstride[k];
                    if ((a.coarse >> k) & 1u) {
                        T h[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) h[j] = base[cn.o[j]];
                        v[k] = cd_interp<T>(cn, h);
                    } else {
                        v[k] = (double)base[((a.c.dense >> k) & 1u) ? i : 0];
                    }
                }
                const PixelIn<double> x = comp_pixel(v);
                const ClassPar<double> p = comp_params(lut + c);
                PixelOut<double> o;
                if (fast_out_of_domain(x)) o = et_pixel_exact<double, PET, true>(x, p);
                else o = et_pixel_fast<double, PET>(x, p, tab);
                double v_et, v_pet;
                comp_totals<PET>(o, v[kCompHours], v_et, v_pet);
                et.add(v_et);
                if constexpr (PET) pet.add(v_pet);
            }
            comp_store<T, PET>(a.c, i, period, len, et, pet);
        }
    }
}

}  // namespace mod16
