// Zonal histograms and exact zonal quantiles per zone and layer: the kernels of mod16_zonal_hist_* and
// mod16_zonal_select. The definition is the numpy statement mod16_amd/zonalq.py (histogram, digits,
// select); this file follows it step for step.
//
// Why integers: a table is made of int64 words that 64-bit integer adds fill -- 1 per valid pixel, or
// the weight quantised ONCE to qw = rint(w 2^(31 - ew)) <= 2^31 -- so, as in mod16_zonal.hpp, the
// words do not depend on the order in which lanes, blocks, tiles, calls or devices arrive. A quantile
// is found by radix selection over histograms of the order-preserving key, most significant digit
// first: an exact order statistic. A word is valid while a zone and layer holds fewer than 2^31
// valid pixels over everything added into it.
//
// zonal_hist_kernel walks a ZonalGeom as zonal_traverse does (mod16_zonal.hpp: the block's range of
// 16-byte vectors, the loads, the per-row weight walk) but keeps a loop of its own: as a step of
// zonal_traverse its float64 histogram into a global table (2025 zones, 46 layers of 5.76 M pixels)
// took 8.5846 ms against 8.5778 ms, 0.0068 ms more where this loop's own repeats spread over 0.0065 ms
// (profiles/zonal_shared_traversal_speed.txt). A change to the walk is made in both. Per valid pixel
// the lane forms the uniform bin (UNIFORM; explicit round-once subtraction and multiply) or the key's
// digit (DIGIT; at a level >= 1 under the prefix filter of up to `slots` slots of its zone) and adds
// its weight word to one table word per matching slot. A lane merges runs of equal table word in
// registers before it adds (one run: the slots of a vector's pixels are visited slot by slot, so the
// pixels of a vector that share a word leave as one add).
//   LW > 0   the block's LDS table of nzones * S_eff * nb words (S_eff = 1 on level 0 and in uniform
//            mode) with 64-bit LDS integer adds (ds_add_u64); at its end the block flushes the words
//            that are not zero with global 64-bit integer atomic adds.
//   LW == 0  the adds go straight to the table in global memory.
// kZonalqLdsWords (9984 words = 79 872 bytes: 13 zones x 3 slots x 256 bins exactly) and the 256
// prefixes a block keeps in LDS make 81 920 bytes, so that two blocks share a CU's 160 KiB; tables of
// up to kZonalqLdsSmall words (13 zones x 258 words of a uniform histogram, level 0 of a class map) take
// an instance with a 28 KiB table and five blocks per CU. No float atomics, no compare-and-swap loops.
//
// zonal_select_kernel closes a level: per (k, z, s) one block sums the row (level 0: forms the target
// from the total, in 128-bit integers), prefix-scans the bins in integers and writes `remaining` and
// `prefix`; after the last level it writes the value.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mod16_zonal.hpp"

namespace mod16 {

constexpr int kZonalqLdsWords = 9984;        // mod16_zonal_hist_lds_bytes() / 8
constexpr int kZonalqLdsSmall = 3584;
constexpr int kZonalqLdsPrefix = 256;        // prefixes of a layer a block keeps in LDS
constexpr int kZonalqMaxSlots = 16;
enum { kZonalqUniform = 0, kZonalqDigit = 1 };       // enum mod16_zonal_hist_mode

struct ZonalHistArgs : ZonalGeom {
    const unsigned long long* prefix;   // [layers][nzones][slots]; level >= 1
    unsigned long long* hist;           // [layers][nzones][slots][nb] (digit) or [layers][nzones][nb] (uniform)
    double wmax, lo, hi, scale;
    int wexp;                // 31 - ew
    int nb;                  // words per zone and slot: 2^bits, or bins + 2
    int bins;
    int slots;               // slots of the table in memory
    int seff;                // slots that take part: 1 on level 0 and in uniform mode
    int top;                 // digit mode: key >> top is compared with the prefix (level >= 1; 64 on level 0: no filter)
    int low, mask;           // digit = (key >> low) & mask
};

// the order-preserving unsigned image of a value in its own width
__device__ __forceinline__ unsigned long long zonalq_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned long long zonalq_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (unsigned long long)(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}
__device__ __forceinline__ double zonalq_unkey(unsigned long long k, double) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull)));
}
__device__ __forceinline__ float zonalq_unkey(unsigned long long k, float) {
    const unsigned b = (unsigned)k;
    return __uint_as_float(b ^ ((b >> 31) ? 0x80000000u : 0xffffffffu));
}

template <bool LDS> __device__ __forceinline__ void zonalq_add(unsigned long long* p, unsigned long long v) {
    if constexpr (LDS) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a lane's current run: one table word and what is to be added to it
struct ZonalqRun {
    int64_t word;
    unsigned long long sum;
};
template <bool LDS> __device__ __forceinline__ void zonalq_put(ZonalqRun& r, int64_t word, unsigned long long qw, unsigned long long* table) {
    if (word != r.word) {
        if (r.sum) zonalq_add<LDS>(table + r.word, r.sum);
        r.word = word;
        r.sum = 0;
    }
    r.sum += qw;
}

template <typename T, typename ZT, int WK, int MODE, int LW>
__global__ __launch_bounds__(kBlock) void zonal_hist_kernel(ZonalHistArgs a) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr bool LDS = LW > 0;
    __shared__ unsigned long long lds[LDS ? LW : 1];
    __shared__ unsigned long long lpre[MODE == kZonalqDigit ? kZonalqLdsPrefix : 1];
    // the table a lane adds into has seff slots per zone in LDS, a.slots in memory
    const int tslots = LDS ? a.seff : a.slots;
    const int nwords = a.nzones * a.seff * a.nb;                   // (LDS: at most LW, the host side saw to it)
    unsigned long long* const layer_hist = a.hist + (int64_t)blockIdx.y * a.nzones * (MODE == kZonalqDigit ? a.slots : 1) * a.nb;
    unsigned long long* const table = LDS ? lds : layer_hist;
    const bool filter = MODE == kZonalqDigit && a.top < 64;
    const int npre = a.nzones * a.slots;
    const bool pre_lds = filter && npre <= kZonalqLdsPrefix;
    const unsigned long long* const gpre = filter ? a.prefix + (int64_t)blockIdx.y * npre : nullptr;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < nwords; i += kBlock) lds[i] = 0;
    }
    if constexpr (MODE == kZonalqDigit) {
        if (pre_lds)
            for (int i = threadIdx.x; i < npre; i += kBlock) lpre[i] = gpre[i];
    }
    __syncthreads();
    const unsigned long long* const pre = pre_lds ? lpre : gpre;
    const T* const vrow = static_cast<const T*>(a.values) + (int64_t)blockIdx.y * a.pitch;
    const ZT* const zrow = static_cast<const ZT*>(a.zones);
    const int64_t nvec = (a.n + V - 1) / V;
    const int64_t per = (nvec + gridDim.x - 1) / gridDim.x;
    const int64_t v0 = (int64_t)blockIdx.x * per;
    const int64_t v1 = v0 + per < nvec ? v0 + per : nvec;
    ZonalqRun run;
    run.word = 0;
    run.sum = 0;
    for (int64_t vb = v0; vb < v1; vb += kBlock) {
        const int64_t v = vb + threadIdx.x;
        const int64_t p0 = v * V;
        const int nv = v >= v1 ? 0 : a.n - p0 < V ? (int)(a.n - p0) : V;
        T x[V];
        ZT z[V];
        [[maybe_unused]] T wp[V];
        if (nv == V && a.wide) {
            const ZonalVec<T, V> xv = *reinterpret_cast<const ZonalVec<T, V>*>(vrow + p0);
            const ZonalVec<ZT, V> zv = *reinterpret_cast<const ZonalVec<ZT, V>*>(zrow + p0);
#pragma unroll
            for (int k = 0; k < V; ++k) { x[k] = xv.v[k]; z[k] = zv.v[k]; }
            if constexpr (WK == kZonalWeightPixel) {
                const ZonalVec<T, V> wv = *reinterpret_cast<const ZonalVec<T, V>*>(static_cast<const T*>(a.weights) + p0);
#pragma unroll
                for (int k = 0; k < V; ++k) wp[k] = wv.v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const bool in = k < nv;
                x[k] = in ? vrow[p0 + k] : (T)0;
                z[k] = in ? zrow[p0 + k] : (ZT)0;
                if constexpr (WK == kZonalWeightPixel) wp[k] = in ? static_cast<const T*>(a.weights)[p0 + k] : (T)0;
            }
        }
        [[maybe_unused]] int64_t row = 0, col = 0;
        [[maybe_unused]] double wr = 1.0;
        if constexpr (WK == kZonalWeightRow) {
            if (nv > 0) {
                zonal_row(a.first_pixel + p0, a.cols, a.inv_cols, row, col);
                wr = static_cast<const double*>(a.weights)[row - a.row0];
            }
        }
        // per pixel: its zone (-1: the pixel does not count), its weight word, its bin or digit, its key's top
        int zone[V], bin[V];
        unsigned long long qw[V];
        [[maybe_unused]] unsigned long long top[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            double w = 1.0;
            if constexpr (WK == kZonalWeightRow) {
                if (k > 0 && k < nv && ++col == a.cols) {
                    col = 0;
                    ++row;
                    wr = static_cast<const double*>(a.weights)[row - a.row0];
                }
                w = wr;
            } else if constexpr (WK == kZonalWeightPixel) {
                w = (double)wp[k];
            }
            const int64_t zk = (int64_t)z[k];
            bool live = k < nv && zk >= 0 && zk < (int64_t)a.nzones && !(x[k] != x[k]);
            if constexpr (WK != kZonalWeightNone) {
                live = live && w >= 0.0 && w <= a.wmax;           // (a NaN weight fails both)
                qw[k] = live ? (unsigned long long)(long long)__builtin_rint(__builtin_ldexp(w, a.wexp)) : 0;
                live = live && qw[k] != 0;                        // (a word of 0 changes nothing)
            } else {
                qw[k] = 1;
            }
            zone[k] = live ? (int)zk : -1;
            if constexpr (MODE == kZonalqUniform) {
                const double xd = (double)x[k];
                int b;
                if (xd < a.lo) b = 0;
                else if (!(xd < a.hi)) b = a.bins + 1;
                else {
                    const double t = __dmul_rn(__dsub_rn(xd, a.lo), a.scale);
                    b = 1 + (int)__builtin_floor(t);
                    b = b > a.bins ? a.bins : b;
                }
                bin[k] = b;
            } else {
                const unsigned long long key = zonalq_key(x[k]);
                bin[k] = (int)((key >> a.low) & (unsigned long long)a.mask);
                top[k] = filter ? key >> a.top : 0;
            }
        }
        if (!filter) {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (zone[k] >= 0) zonalq_put<LDS>(run, ((int64_t)zone[k] * tslots) * a.nb + bin[k], qw[k], table);
        } else {
            if constexpr (MODE == kZonalqDigit) {
                for (int s = 0; s < a.slots; ++s) {
#pragma unroll
                    for (int k = 0; k < V; ++k)
                        if (zone[k] >= 0 && pre[zone[k] * a.slots + s] == top[k])
                            zonalq_put<LDS>(run, ((int64_t)zone[k] * tslots + s) * a.nb + bin[k], qw[k], table);
                }
            }
        }
    }
    if (run.sum) zonalq_add<LDS>(table + run.word, run.sum);
    if constexpr (LDS) {
        __syncthreads();
        // (LDS tables have seff slots; level 0 and uniform mode: slot 0 of the a.slots in memory)
        const int mslots = MODE == kZonalqDigit ? a.slots : 1;
        const int per_zone = a.seff * a.nb;
        for (int i = threadIdx.x; i < nwords; i += kBlock) {
            const unsigned long long word = lds[i];
            if (word == 0) continue;
            const int zz = i / per_zone, rest = i - zz * per_zone;     // rest = s * nb + bin, s < seff <= mslots
            zonalq_add<false>(layer_hist + (int64_t)zz * mslots * a.nb + rest, word);
        }
    }
}

struct ZonalSelectArgs {
    const unsigned long long* hist;   // [rows / slots][slots][nb]
    long long* remaining;             // [rows]
    unsigned long long* prefix;       // [rows]
    void* values;                     // [rows] of T; written after the last level
    long long* weight;                // [rows / slots]; written on level 0
    int64_t rows;                     // layers * nzones * slots
    int slots, nb, used;              // used: the bins of this level, 2^d
    int dbits;                        // d
    int level, last;
    unsigned long long q_mant[kZonalqMaxSlots];
    int q_exp[kZonalqMaxSlots];
};

// max(1, ceil(M W / 2^E)) for W > 0 (M < 2^53, W < 2^62: the product is below 2^115)
__host__ __device__ inline unsigned long long zonalq_target(unsigned long long M, int E, unsigned long long W) {
    const unsigned __int128 P = (unsigned __int128)M * W;
    unsigned long long t;
    if (E >= 128) t = P != 0;
    else if (E <= 0) t = (unsigned long long)P;                    // (E >= 52 for every q in [0, 1])
    else {
        const unsigned __int128 q = P >> E;
        t = (unsigned long long)q + ((q << E) != P);
    }
    return t < 1 ? 1 : t;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void zonal_select_kernel(ZonalSelectArgs a) {
    __shared__ unsigned long long part[kBlock];
    const int chunk = (a.used + kBlock - 1) / kBlock;              // bins of a thread, consecutive
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const int64_t zrow = r / a.slots;
        const int s = (int)(r - zrow * a.slots);
        const unsigned long long* const row = a.hist + (zrow * a.slots + (a.level == 0 ? 0 : s)) * a.nb;
        const int b0 = (int)threadIdx.x * chunk;
        const int b1 = b0 + chunk < a.used ? b0 + chunk : a.used;
        // (read before the barriers below: the thread that finds the bin overwrites it)
        const unsigned long long left = a.level == 0 ? 0 : (unsigned long long)a.remaining[r];
        unsigned long long mine = 0;
        for (int b = b0; b < b1; ++b) mine += row[b];
        part[threadIdx.x] = mine;
        __syncthreads();
        // inclusive scan of the threads' sums (integers: any order of the adds gives these words)
        for (int off = 1; off < kBlock; off *= 2) {
            const unsigned long long other = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += other;
            __syncthreads();
        }
        const unsigned long long total = part[kBlock - 1];
        unsigned long long want;
        if (a.level == 0) {
            want = total ? zonalq_target(a.q_mant[s], a.q_exp[s], total) : 0;
            if (s == 0 && threadIdx.x == 0) a.weight[zrow] = (long long)total;
        } else {
            want = left;
        }
        const unsigned long long before = part[threadIdx.x] - mine;
        if (want != 0 && before < want && want <= part[threadIdx.x]) {       // exactly one thread
            unsigned long long run = before;
            int b = b0;
            for (; b < b1 - 1; ++b) {
                if (run + row[b] >= want) break;
                run += row[b];
            }
            const unsigned long long pre = a.level == 0 ? 0 : a.prefix[r];
            const unsigned long long key = (pre << a.dbits) | (unsigned long long)b;
            a.remaining[r] = (long long)(want - run);
            a.prefix[r] = key;
            if (a.last) static_cast<T*>(a.values)[r] = zonalq_unkey(key, T());
        }
        if (threadIdx.x == 0 && (want == 0 || want > total)) {      // an empty zone (or a table short of its target): no value
            if (a.level == 0) { a.remaining[r] = 0; a.prefix[r] = 0; }
            if (a.last) static_cast<T*>(a.values)[r] = (T)__builtin_nan("");
            if (want > total) a.remaining[r] = 0;
        }
        __syncthreads();
    }
}

}  // namespace mod16
