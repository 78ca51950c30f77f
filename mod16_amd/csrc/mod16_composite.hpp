// Multi-day ET composites (gfx950): per-pixel period totals of MOD16.evapotranspiration over K days
// of drivers in one launch -- mod16_et_composite_*. The definition is the numpy statement
// mod16_amd/composite.py (daily_total, composite_reduce); this follows it operation for operation.
//
// One lane per pixel, the block and grid shapes of ens_kernel. A pixel's class parameters come from
// the derived table in LDS once; the lane then walks the days of every period: each of the 15 arrays
// (14 drivers and the hours of daylight) has a divisor `every`, day t reads its time slab t / every,
// and a value is loaded again only on the day its slab index changes (a count-down per array in
// scalar registers: the day loop is wave-uniform). Day t + 1's changing values are issued before day
// t is computed. Every day calls et_pixel_fast<double, PET> (MOD16_MATH_EXACT: et_pixel_exact) as the
// step kernels do, forms the daily total v = (day h 3600) + (night (24 - h) 3600) and adds it to the
// period's sum if it is not NaN; one value (and one count) per pixel and period is stored.
// float32 storage: inputs widened, arithmetic and accumulation in float64, one rounding on store.
//
// Domain guard: fast_out_of_domain(x_t) per pixel-day. A pixel with any flagged day gets no result
// from comp_kernel but a NaN with a payload of its own (CompMark) in period 0 of out_et, and
// comp_redo_kernel, launched behind it as ens_redo_kernel is, computes all periods of every marked
// pixel: a flagged day by et_pixel_exact, every other day by et_pixel_fast -- what the step engine
// does per pixel-day, so the bits are those of a loop over single steps. No atomics on results, no
// workspace, nothing shared between launches: two launches give the same bits. A pixel whose own
// period-0 result carried the payload by coincidence would merely be computed twice.
#pragma once
#include "mod16_kernels.hpp"

namespace mod16 {

constexpr int kCompArrays = 15;          // the 14 drivers and, last, the hours of daylight
constexpr int kCompHours = 14;
constexpr int kCompMaxDays = 4096;

template <typename T> struct CompArgs {
    const T* arr[kCompArrays];
    int64_t tstride[kCompArrays];   // elements between two time slabs
    int every[kCompArrays];         // day t reads slab t / every
    uint32_t dense;                 // bit k set: array k has one value per pixel, else one value per slab
    const uint8_t* cls;
    const double* lut64;            // device [MOD16_LUT_ROWS][kLutCols]
    const double* tab;              // exp / log tables of FastMath<double>
    T* out_et;                      // [periods][out_pitch]
    T* out_pet;                     // PET instances only
    uint16_t* cnt_et;               // [periods][cnt_pitch], or NULL
    uint16_t* cnt_pet;
    int64_t out_pitch, cnt_pitch, n;
    int days, period_days, min_valid, rescale;
    unsigned* status;
};

// What comp_kernel leaves in period 0 of out_et for a pixel with a day outside the domain of the
// fast arithmetic (a quiet NaN, payload "c0351")
template <typename T> struct CompMark;
template <> struct CompMark<double> {
    static constexpr unsigned long long bits = 0x7ff80000000c0351ull;
    static __device__ __forceinline__ double value() { return __longlong_as_double((long long)bits); }
    static __device__ __forceinline__ bool is(double v) { return (unsigned long long)__double_as_longlong(v) == bits; }
};
template <> struct CompMark<float> {
    static constexpr unsigned bits = 0x7fcc0351u;
    static __device__ __forceinline__ float value() { return __uint_as_float(bits); }
    static __device__ __forceinline__ bool is(float v) { return __float_as_uint(v) == bits; }
};

// composite.daily_total: left to right, no contraction
__device__ __forceinline__ double comp_daily(double day, double night, double h) {
#pragma clang fp contract(off)
    return (day * h * 3600.0) + (night * (24.0 - h) * 3600.0);
}

// composite.composite_reduce for one pixel and one series (ET or PET)
struct CompAcc {
    double sum;
    unsigned cnt;
    __device__ __forceinline__ void reset() { sum = 0.0; cnt = 0u; }
    __device__ __forceinline__ void add(double v) {
#pragma clang fp contract(off)
        const bool ok = v == v;
        sum = ok ? sum + v : sum;
        cnt += ok ? 1u : 0u;
    }
    __device__ __forceinline__ double result(int len, int min_valid, int rescale) const {
#pragma clang fp contract(off)
        double r = sum;
        if (rescale) r = sum * ((double)len / (double)(cnt ? cnt : 1u));
        return ((int)cnt < min_valid) ? __builtin_nan("") : r;
    }
};

// the class's column of the derived table (LDS)
__device__ __forceinline__ ClassPar<double> comp_params(const double* l) {
    ClassPar<double> p;
    p.tmin_close = l[0 * kLutCols];
    p.tmin_open = l[1 * kLutCols];
    p.vpd_open = l[2 * kLutCols];
    p.vpd_close = l[3 * kLutCols];
    p.gl_sh = l[4 * kLutCols];
    p.gl_wv = l[5 * kLutCols];
    p.g_cut = l[6 * kLutCols];
    p.csl = l[7 * kLutCols];
    p.rbl_min = l[8 * kLutCols];
    p.rbl_max = l[9 * kLutCols];
    p.beta = l[10 * kLutCols];
    p.inv_dtmin = l[11 * kLutCols];
    p.inv_dvpd = l[12 * kLutCols];
    p.rbl_slope = l[13 * kLutCols];
    p.inv_beta = l[14 * kLutCols];
    return p;
}

__device__ __forceinline__ PixelIn<double> comp_pixel(const double (&v)[kCompArrays]) {
    return PixelIn<double>{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13]};
}

// the day's ET (and potential ET) totals from the pixel function's components
template <bool PET>
__device__ __forceinline__ void comp_totals(const PixelOut<double>& o, double h, double& et, double& pet) {
#pragma clang fp contract(off)
    et = comp_daily((o.canopy_d + o.soil_d) + o.trans_d, (o.canopy_n + o.soil_n) + o.trans_n, h);
    pet = PET ? comp_daily(o.pet_d, o.pet_n, h) : 0.0;
}

template <typename T, bool PET>
__device__ __forceinline__ void comp_store(const CompArgs<T>& a, int64_t i, int period, int len,
                                           const CompAcc& et, const CompAcc& pet) {
    a.out_et[(int64_t)period * a.out_pitch + i] = (T)et.result(len, a.min_valid, a.rescale);
    if (a.cnt_et) a.cnt_et[(int64_t)period * a.cnt_pitch + i] = (uint16_t)et.cnt;
    if constexpr (PET) {
        a.out_pet[(int64_t)period * a.out_pitch + i] = (T)pet.result(len, a.min_valid, a.rescale);
        if (a.cnt_pet) a.cnt_pet[(int64_t)period * a.cnt_pitch + i] = (uint16_t)pet.cnt;
    }
}

// 256-thread blocks over batches of 256 pixels; the batch, period and day loops are block-uniform,
// the threads past the raster's end compute on its last pixel and store nothing.
// FAST: the class parameters and day t + 1's values stay in registers across day t (two waves per
// SIMD). The reference-order instance reads its parameters from LDS every day, loads a changing value
// behind the day's arithmetic and calls the pixel function in its SERIAL form (one component at a
// time: 253 vector registers with potential ET; the plain form took 256 and 36 accumulator registers).
// (The reference-order instances ask for one block per CU only; that they fit two waves per SIMD today
// -- 253 registers with potential ET -- is incidental, three registers more would halve it.)
template <typename T, bool FAST, bool PET>
__global__ void __launch_bounds__(kBlock, FAST ? 2 : 1) comp_kernel(const CompArgs<T> a) {
    constexpr int kTab = FAST ? FastMath<double>::kTabDoubles : 1;
    __shared__ __attribute__((aligned(16))) double lut[MOD16_LUT_ROWS * kLutCols];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    if constexpr (FAST) {
        ignore_signalling_nans();                  // the domain guard's NaN-ignoring chain
        for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.tab[i];
    }
    for (int i = threadIdx.x; i < MOD16_LUT_ROWS * kLutCols; i += kBlock) lut[i] = a.lut64[i];
    __syncthreads();
    const int K = a.days, L = a.period_days;
    const int64_t nbatch = (a.n + kBlock - 1) / kBlock;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i0 = b * kBlock + threadIdx.x;
        const bool live = i0 < a.n;
        const int64_t i = live ? i0 : a.n - 1;
        unsigned c = a.cls[i];
        if (c >= 13u) {   // numpy would raise IndexError: flag it, give NaN
            atomicOr(a.status, kStatusClassRange);
            c = 13u;
        }
        // day 0's values; left[k]: days until array k's slab index changes (wave-uniform)
        const T* at[kCompArrays];
        double cur[kCompArrays];
        int left[kCompArrays];
#pragma unroll
        for (int k = 0; k < kCompArrays; ++k) {
            at[k] = a.arr[k] + (((a.dense >> k) & 1u) ? i : 0);
            cur[k] = (double)*at[k];
            left[k] = a.every[k];
        }
        bool bad = false;
        int t = 0, period = 0;
        if constexpr (FAST) {
            const ClassPar<double> p = comp_params(lut + c);
            T nxt[kCompArrays];        // in the storage type: widening here would wait for each load at once
            // day 0's values have arrived before the day loop begins (vmcnt(0)): inside it the only
            // loads in flight are day t + 1's, and the only wait for them sits behind day t's arithmetic
            __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma nounroll
            for (int t0 = 0; t0 < K; t0 += L, ++period) {
                const int len = (K - t0 < L) ? K - t0 : L;
                CompAcc et, pet;
                et.reset();
                pet.reset();
#pragma nounroll
                for (int d = 0; d < len; ++d, ++t) {
                    // day t + 1's changing values, issued in front of day t's arithmetic
                    const bool more = t + 1 < K;
                    bool turn[kCompArrays];
#pragma unroll
                    for (int k = 0; k < kCompArrays; ++k) {
                        turn[k] = (--left[k] == 0) & more;
                        if (turn[k]) {
                            at[k] += a.tstride[k];
                            nxt[k] = *at[k];
                            left[k] = a.every[k];
                        }
                    }
                    const PixelIn<double> x = comp_pixel(cur);
                    bad |= fast_out_of_domain(x);
                    const PixelOut<double> o = et_pixel_fast<double, PET>(x, p, tab);
                    double v_et, v_pet;
                    comp_totals<PET>(o, cur[kCompHours], v_et, v_pet);
                    et.add(v_et);
                    if constexpr (PET) pet.add(v_pet);
#pragma unroll
                    for (int k = 0; k < kCompArrays; ++k)
                        if (turn[k]) cur[k] = (double)nxt[k];
                }
                if (live & !bad) comp_store<T, PET>(a, i, period, len, et, pet);
            }
            // a day outside the domain of the strength-reduced arithmetic: the mark for
            // comp_redo_kernel, which runs behind this kernel (mod16_physics.hpp, "domain guard")
            if (live & bad) a.out_et[i] = CompMark<T>::value();
        } else {
#pragma nounroll
            for (int t0 = 0; t0 < K; t0 += L, ++period) {
                const int len = (K - t0 < L) ? K - t0 : L;
                CompAcc et, pet;
                et.reset();
                pet.reset();
#pragma nounroll
                for (int d = 0; d < len; ++d, ++t) {
                    const PixelIn<double> x = comp_pixel(cur);
                    const PixelOut<double> o = et_pixel_exact<double, PET, true>(x, comp_params(lut + c));
                    double v_et, v_pet;
                    comp_totals<PET>(o, cur[kCompHours], v_et, v_pet);
                    et.add(v_et);
                    if constexpr (PET) pet.add(v_pet);
                    const bool more = t + 1 < K;
#pragma unroll
                    for (int k = 0; k < kCompArrays; ++k)
                        if ((--left[k] == 0) & more) {
                            at[k] += a.tstride[k];
                            cur[k] = (double)*at[k];
                            left[k] = a.every[k];
                        }
                }
                if (live) comp_store<T, PET>(a, i, period, len, et, pet);
            }
        }
    }
}

// Behind comp_kernel<T, true, PET>: all periods of the marked pixels; a day outside the domain in
// the reference's operation order, every other day by the fast pixel function.
template <typename T, bool PET>
__global__ void __launch_bounds__(kBlock, 1) comp_redo_kernel(const CompArgs<T> a) {
    constexpr int kTab = FastMath<double>::kTabDoubles;
    __shared__ __attribute__((aligned(16))) double lut[MOD16_LUT_ROWS * kLutCols];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    ignore_signalling_nans();
    for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.tab[i];
    for (int i = threadIdx.x; i < MOD16_LUT_ROWS * kLutCols; i += kBlock) lut[i] = a.lut64[i];
    __syncthreads();
    const int K = a.days, L = a.period_days;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += step) {
        if (!CompMark<T>::is(a.out_et[i])) continue;
        unsigned c = a.cls[i];
        c = c >= 13u ? 13u : c;        // (comp_kernel has flagged it)
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
                for (int k = 0; k < kCompArrays; ++k)
                    v[k] = (double)a.arr[k][(int64_t)(t / a.every[k]) * a.tstride[k] + (((a.dense >> k) & 1u) ? i : 0)];
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
            comp_store<T, PET>(a, i, period, len, et, pet);
        }
    }
}

}  // namespace mod16
