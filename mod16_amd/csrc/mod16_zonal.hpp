// Zonal statistics -- exact weighted sums per zone and layer: the kernels of mod16_zonal_* and
// mod16_zonal_bounds_*. The definition is the numpy statement mod16_amd/zonal.py (classify, quantise,
// accumulate); this file follows it step for step.
//
// Why integers: every term (w, w x, w x x) is quantised ONCE to a 62-bit fixed point whose scale the
// call fixes (F0 = 62 - ew, F1 = 62 - ew - ex, F2 = 62 - ew - 2 ex fractional bits for bounds wmax <=
// 2^ew, xmax <= 2^ex) and accumulated with 64-bit integer adds. Integer addition is associative: the
// words do not depend on the order in which lanes, blocks, tiles, calls or devices arrive, which a
// float atomic cannot promise. A term |q| <= 2^62 is kept as qh = q >> 32 (|qh| <= 2^30) and ql = q &
// 0xffffffff, summed in separate int64 words, so neither a lane's registers nor a table entry can
// overflow: the accumulator is valid while a zone and layer holds fewer than 2^31 valid pixels over
// everything accumulated into it (every lo word then stays below 2^63).
//
// Shape: blockIdx.y is the layer; the x grid is a small multiple of the CU count. A block owns one
// contiguous range of 16-byte vectors and strides through it, consecutive lanes on consecutive
// vectors (a lane reads 16 bytes of values, the matching zone ids and, per pixel, weights per step;
// rows that are not 16-byte aligned, and a ragged last vector, take scalar accesses). A lane merges
// runs of equal zone id in registers -- basins and countries are spatially coherent, a lane's next
// vector lies 256 vectors further along the same range -- and touches shared state only where its
// zone changes and at its end:
//   LZ > 0   (nzones <= LZ) the block's LDS table [nzones][10] with 64-bit LDS integer atomics (add,
//            min, max); at its end the block flushes the words that left their identity to the
//            global accumulator with global 64-bit integer atomics.
//   LZ == 0  (more zones than the LDS holds) the runs go straight to the global accumulator, those of
//            a wave's neighbouring lanes that hold the same zone merged first (zonal_flush_wave): one
//            set of atomics per zone a wave's 128 or 256 consecutive pixels meet. Right for any zone
//            map, but a map without runs pays up to ten global atomics per pixel.
// kZonalLdsZones is chosen so that two blocks fit a CU's 160 KiB of LDS (2 x 1000 x 80 bytes); maps of
// up to kZonalLdsSmall zones (a class raster) take an instance with a 5 KiB table and full occupancy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mod16 {

constexpr int kZonalWords = 10;
constexpr int kZonalLdsZones = 1000;     // mod16_zonal_lds_zones()
constexpr int kZonalLdsSmall = 64;
enum { kZonalCount = 0, kZonalRejected = 1, kZonalSums = 2, kZonalMin = 8, kZonalMax = 9 };
enum { kZonalWeightNone = 0, kZonalWeightRow = 1, kZonalWeightPixel = 2 };     // enum mod16_zonal_weight
constexpr long long kZonalKeyMax = 0x7fffffffffffffffLL;
constexpr long long kZonalKeyMin = -kZonalKeyMax - 1;

// what the kernels of both zonal families (this file, mod16_zonalq.hpp) read of a call: the pixels, their
// zones and weights; zonal_traverse walks them
struct ZonalGeom {
    const void* values;      // [layers][pitch] of T
    const void* zones;       // [n] of ZT
    const void* weights;     // per row: double, entry r is raster row row0 + r; per pixel: [n] of T
    int64_t n, pitch, cols, first_pixel, row0;
    double inv_cols;
    int nzones;
    int wide;                // every row allows vector access
};

struct ZonalArgs : ZonalGeom {
    long long* acc;          // [layers][nzones][10]
    unsigned long long* bounds;   // zonal_bounds_kernel: the bits of max w, max |x|
    int64_t rows;            // zonal_bounds_kernel, per-row weights: the entries of `weights` the range touches
    double wmax, xmax;
    int f[3];                // fractional bits of w, w x, w x x
};

template <typename E, int N> struct alignas(sizeof(E) * N) ZonalVec { E v[N]; };

// the state of a lane's current run: one zone's words, hi and lo apart
struct ZonalRun {
    int zone;
    unsigned count, rejected;
    long long hi[3];
    unsigned long long lo[3];
    long long kmin, kmax;
};
__device__ __forceinline__ void zonal_reset(ZonalRun& r, int zone) {
    r.zone = zone;
    r.count = r.rejected = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) { r.hi[j] = 0; r.lo[j] = 0; }
    r.kmin = kZonalKeyMax;
    r.kmax = kZonalKeyMin;
}

template <bool LDS> __device__ __forceinline__ void zonal_add(long long* p, long long v) {
    if (v == 0) return;
    if constexpr (LDS) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void zonal_min(long long* p, long long v) {
    if constexpr (LDS) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void zonal_max(long long* p, long long v) {
    if constexpr (LDS) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a run into its zone's entry of `table` (the block's LDS table, or the layer's part of the accumulator)
template <bool LDS> __device__ __forceinline__ void zonal_flush(const ZonalRun& r, long long* table) {
    if (r.zone < 0 || (r.count | r.rejected) == 0) return;
    long long* e = table + (int64_t)r.zone * kZonalWords;
    zonal_add<LDS>(e + kZonalRejected, (long long)r.rejected);
    if (r.count == 0) return;
    zonal_add<LDS>(e + kZonalCount, (long long)r.count);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        zonal_add<LDS>(e + kZonalSums + 2 * j, r.hi[j]);
        zonal_add<LDS>(e + kZonalSums + 2 * j + 1, (long long)r.lo[j]);
    }
    zonal_min<LDS>(e + kZonalMin, r.kmin);
    zonal_max<LDS>(e + kZonalMax, r.kmax);
}

// q = rint(t 2^F) as qh = q >> 32 and ql = q & 0xffffffff, without a 64-bit conversion: with r the
// rounded value (an integer, |r| <= 2^62), h = floor(r / 2^32) is exact and fits an int, and l = r - h
// 2^32 is exact and lies in [0, 2^32)
__device__ __forceinline__ void zonal_quantise(double t, int F, long long& hi, unsigned long long& lo) {
    const double r = __builtin_rint(__builtin_ldexp(t, F));
    const double h = __builtin_floor(r * (1.0 / 4294967296.0));
    const double l = __builtin_fma(h, -4294967296.0, r);
    hi += (long long)(int)h;
    lo += (unsigned long long)(unsigned)l;
}

// the order-preserving int64 image of a double: the bits, the low 63 flipped where the sign is set
__device__ __forceinline__ long long zonal_key(double x) {
    const long long b = __double_as_longlong(x);
    return b ^ ((b >> 63) & kZonalKeyMax);
}

// The runs of a wave's lanes into `table` (the accumulator: global atomics are the scarce resource
// here), merged first: lanes that hold the SAME zone next to each other -- a wave's vectors are
// consecutive pixels, so they usually fall into two or three zones -- form a segment, the segment's
// words are summed by a doubling scan over the lanes, and its first lane alone issues the atomics.
// Called by all 64 lanes of a wave together; `want`: this lane's run is to go. Segments are numbered
// by their heads, so a map like A B A makes three of them: right for any zone map.
__device__ __forceinline__ void zonal_flush_wave(const ZonalRun& r, bool want, long long* table) {
    const int lane = (int)(threadIdx.x & 63u);
    const bool live = want && r.zone >= 0 && (r.count | r.rejected) != 0;
    ZonalRun m = r;
    if (!live) zonal_reset(m, -1 - lane);          // (a zone of its own: never merged, never flushed)
    const int prev = __shfl_up(m.zone, 1);
    const bool head = lane == 0 || prev != m.zone;
    const unsigned long long heads = __ballot(head);
    const int seg = __popcll(heads & (~0ull >> (63 - lane)));
#pragma unroll
    for (int off = 1; off < 64; off *= 2) {
        const bool take = __shfl_down(seg, off) == seg && lane + off < 64;
        const unsigned count = __shfl_down(m.count, off), rejected = __shfl_down(m.rejected, off);
        const long long kmin = __shfl_down(m.kmin, off), kmax = __shfl_down(m.kmax, off);
        if (take) {
            m.count += count;
            m.rejected += rejected;
            m.kmin = kmin < m.kmin ? kmin : m.kmin;
            m.kmax = kmax > m.kmax ? kmax : m.kmax;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long hi = __shfl_down(m.hi[j], off);
            const unsigned long long lo = __shfl_down(m.lo[j], off);
            if (take) { m.hi[j] += hi; m.lo[j] += lo; }
        }
    }
    if (head && live) zonal_flush<false>(m, table);
}

// one pixel: steps 1 to 4 of the definition. `in`: the lane has this pixel (the accumulator path
// calls this with all lanes of a wave together, so that their runs can leave merged)
template <bool LDS>
__device__ __forceinline__ void zonal_pixel(ZonalRun& r, bool in, int64_t z, double x, double w, const ZonalArgs& a, long long* table) {
    const bool live = in && z >= 0 && z < (int64_t)a.nzones && !(x != x || w != w);
    const bool change = live && (int)z != r.zone;
    if constexpr (LDS) {
        if (change) zonal_flush<true>(r, table);
    } else {
        const bool need = change && (r.count | r.rejected) != 0;
        if (__any(need)) zonal_flush_wave(r, need, table);
    }
    if (change) zonal_reset(r, (int)z);
    if (!live) return;
    if (!(__builtin_fabs(x) <= a.xmax) || !(w >= 0.0 && w <= a.wmax)) {
        ++r.rejected;
        return;
    }
    ++r.count;
    const double b = w * x;
    const double c = b * x;
    zonal_quantise(w, a.f[0], r.hi[0], r.lo[0]);
    zonal_quantise(b, a.f[1], r.hi[1], r.lo[1]);
    zonal_quantise(c, a.f[2], r.hi[2], r.lo[2]);
    const long long k = zonal_key(x);
    r.kmin = k < r.kmin ? k : r.kmin;
    r.kmax = k > r.kmax ? k : r.kmax;
}

// row and column of raster pixel g (0 <= g < 2^52): the quotient from a float64 estimate, put right
// by its remainder
__device__ __forceinline__ void zonal_row(int64_t g, int64_t cols, double inv_cols, int64_t& row, int64_t& col) {
    row = (int64_t)((double)g * inv_cols);
    col = g - row * cols;
    if (col < 0) { --row; col += cols; }
    if (col >= cols) { ++row; col -= cols; }
}

// The traversal of both families: blockIdx.y is the layer; the block owns one contiguous range of
// 16-byte vectors and strides through it, consecutive lanes on consecutive vectors, every lane of the
// block with the same number of trips (a lane past the range has nv = 0: `step` may use wave-wide
// operations). Per trip the lane loads its V = 16 / sizeof(T) values, zone ids and (per pixel)
// weights -- as vectors where g.wide and the vector is whole, else element by element, 0 past the
// range -- and calls step(nv, x, z, weight): the pixels k < nv count, and weight(k) is pixel k's weight
// as a double. `step` asks for it once per pixel, k = 0 ... V - 1 in this order: per row it is one
// lookup where the vector begins and one more wherever a row ends inside it, a walk that moves on.
template <typename T, typename ZT, int WK, typename Step>
__device__ __forceinline__ void zonal_traverse(const ZonalGeom& g, Step&& step) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* const vrow = static_cast<const T*>(g.values) + (int64_t)blockIdx.y * g.pitch;
    const ZT* const zrow = static_cast<const ZT*>(g.zones);
    const int64_t nvec = (g.n + V - 1) / V;
    const int64_t per = (nvec + gridDim.x - 1) / gridDim.x;
    const int64_t v0 = (int64_t)blockIdx.x * per;
    const int64_t v1 = v0 + per < nvec ? v0 + per : nvec;
    for (int64_t vb = v0; vb < v1; vb += kBlock) {
        const int64_t v = vb + threadIdx.x;
        const int64_t p0 = v * V;
        const int nv = v >= v1 ? 0 : g.n - p0 < V ? (int)(g.n - p0) : V;
        T x[V];
        ZT z[V];
        [[maybe_unused]] T wp[V];
        if (nv == V && g.wide) {
            const ZonalVec<T, V> xv = *reinterpret_cast<const ZonalVec<T, V>*>(vrow + p0);
            const ZonalVec<ZT, V> zv = *reinterpret_cast<const ZonalVec<ZT, V>*>(zrow + p0);
#pragma unroll
            for (int k = 0; k < V; ++k) { x[k] = xv.v[k]; z[k] = zv.v[k]; }
            if constexpr (WK == kZonalWeightPixel) {
                const ZonalVec<T, V> wv = *reinterpret_cast<const ZonalVec<T, V>*>(static_cast<const T*>(g.weights) + p0);
#pragma unroll
                for (int k = 0; k < V; ++k) wp[k] = wv.v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const bool in = k < nv;
                x[k] = in ? vrow[p0 + k] : (T)0;
                z[k] = in ? zrow[p0 + k] : (ZT)0;
                if constexpr (WK == kZonalWeightPixel) wp[k] = in ? static_cast<const T*>(g.weights)[p0 + k] : (T)0;
            }
        }
        [[maybe_unused]] int64_t row = 0, col = 0;
        [[maybe_unused]] double wr = 1.0;
        if constexpr (WK == kZonalWeightRow) {
            if (nv > 0) {
                zonal_row(g.first_pixel + p0, g.cols, g.inv_cols, row, col);
                wr = static_cast<const double*>(g.weights)[row - g.row0];
            }
        }
        step(nv, x, z, [&](int k) {
            if constexpr (WK == kZonalWeightRow) {
                if (k > 0 && k < nv && ++col == g.cols) {
                    col = 0;
                    ++row;
                    wr = static_cast<const double*>(g.weights)[row - g.row0];
                }
                return wr;
            } else if constexpr (WK == kZonalWeightPixel) {
                return (double)wp[k];
            } else {
                return 1.0;
            }
        });
    }
}

template <typename T, typename ZT, int WK, int LZ>
__global__ __launch_bounds__(kBlock) void zonal_kernel(ZonalArgs a) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr bool LDS = LZ > 0;
    __shared__ long long lds[LDS ? LZ * kZonalWords : 1];
    const int nwords = a.nzones * kZonalWords;
    long long* const layer_acc = a.acc + (int64_t)blockIdx.y * a.nzones * kZonalWords;
    long long* const table = LDS ? lds : layer_acc;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < nwords; i += kBlock) {
            const int j = i % kZonalWords;
            lds[i] = j == kZonalMin ? kZonalKeyMax : j == kZonalMax ? kZonalKeyMin : 0;
        }
        __syncthreads();
    }
    ZonalRun run;
    zonal_reset(run, -1);
    zonal_traverse<T, ZT, WK>(a, [&](int nv, const T (&x)[V], const ZT (&z)[V], auto&& weight) {
#pragma unroll
        for (int k = 0; k < V; ++k) zonal_pixel<LDS>(run, k < nv, (int64_t)z[k], (double)x[k], weight(k), a, table);
    });
    if constexpr (LDS) zonal_flush<true>(run, table);
    else zonal_flush_wave(run, true, table);
    if constexpr (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nwords; i += kBlock) {
            const int j = i % kZonalWords;
            const long long word = lds[i];
            if (j == kZonalMin) { if (word != kZonalKeyMax) zonal_min<false>(layer_acc + i, word); }
            else if (j == kZonalMax) { if (word != kZonalKeyMin) zonal_max<false>(layer_acc + i, word); }
            else zonal_add<false>(layer_acc + i, word);
        }
    }
}

// max |x| over the finite values of every layer and max w over the finite weights >= 0, as integer
// maxima of the bit patterns (non-negative doubles order as their bits do): associative, so two
// calls give the same bounds. a.bounds[0]: w, [1]: |x|; both start at 0.
template <typename T, int WK>
__global__ __launch_bounds__(kBlock) void zonal_bounds_kernel(ZonalArgs a) {
    __shared__ unsigned long long top[2];
    if (threadIdx.x < 2) top[threadIdx.x] = 0;
    __syncthreads();
    const T* const vrow = static_cast<const T*>(a.values) + (int64_t)blockIdx.y * a.pitch;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const double inf = __builtin_inf();
    double mx = 0.0, mw = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
        const double x = __builtin_fabs((double)vrow[i]);
        if (x < inf && x > mx) mx = x;
        if constexpr (WK == kZonalWeightPixel) {
            if (blockIdx.y == 0) {
                const double w = (double)static_cast<const T*>(a.weights)[i];
                if (w >= 0.0 && w < inf && w > mw) mw = w;
            }
        }
    }
    if constexpr (WK == kZonalWeightRow) {
        if (blockIdx.y == 0)
            for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.rows; r += stride) {
                const double w = static_cast<const double*>(a.weights)[r];
                if (w >= 0.0 && w < inf && w > mw) mw = w;
            }
    }
    if (mw > 0.0) __hip_atomic_fetch_max(&top[0], (unsigned long long)__double_as_longlong(mw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (mx > 0.0) __hip_atomic_fetch_max(&top[1], (unsigned long long)__double_as_longlong(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (threadIdx.x < 2 && top[threadIdx.x])
        __hip_atomic_fetch_max(a.bounds + threadIdx.x, top[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace mod16
