// Whittaker smoothing of 8-day series, weighted by QC: the kernel of mod16_smooth_u8 / _f32 / _f64. The
// definition is the numpy statement mod16_amd/smooth.py (weights_of, factor, solve, encode); this file
// follows it operation for operation, in float64 and without contraction, so the outputs are its bits.
//
// Shape: time is the strided axis, a lane owns one pixel (a wave's loads and stores of a slab are one
// contiguous run of 64 elements) and walks the slabs in wave-uniform loops: once ascending (the
// factorisation d, c, e and the forward substitution g = f / d), once descending (z), and per envelope
// round once more each way (the lift of y, then the two substitutions with the stored d, c, e). A
// pixel's recurrences carry the two previous slabs in registers: no per-lane array, no scratch.
//
// Between the passes a pixel's columns live in a workspace of the context, laid out [column][S][lanes]:
// lane l of the launch owns element l of every row, so every access of a wave is one 512-byte run. The
// columns are c, e and g (z takes g's place in the backward pass of every round but the last) and, with
// an envelope, y and d. The launch has at most `lanes` lanes -- as many as the workspace budget holds
// columns for -- and a lane takes the pixels l, l + lanes, ...: the workspace does not grow with n. (An
// LDS column per lane, 24 bytes per slab, would hold S = 46 for 148 lanes of a CU at most and S = 138
// for fewer than a wave: one path for every S. Measured: DESIGN.md 8q -- the columns' traffic is what
// bounds the kernel.)
// The last backward pass writes the output, every element exactly once; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace mod16 {

constexpr int kSmoothMaxSlabs = 4096;
constexpr int kSmoothMaxEnvelope = 8;
constexpr int kSmoothFill = 249;     // uint8 codes from here on are fill values
enum { kSmoothColC = 0, kSmoothColE = 1, kSmoothColG = 2, kSmoothColY = 3, kSmoothColD = 4 };
// columns of the workspace a call needs
inline int smooth_columns(int envelope) { return envelope > 0 ? 5 : 3; }

struct SmoothArgs {
    const void* in;             // [S][in_pitch] of IN
    const float* weights;       // [S][w_pitch], or NULL
    const uint8_t* qc;          // [S][w_pitch], or NULL
    const double* qc_weight;    // 256 doubles on the device, or NULL: 1.0 where good_bits holds
    void* out;                  // [S][out_pitch] of OUT
    uint16_t* count;            // [n], or NULL
    double* ws;                 // [columns][S][lanes]
    int64_t n, in_pitch, w_pitch, out_pitch, lanes;
    double lam, scale;
    uint32_t good_bits[8];      // the default table as 256 bits (bit q of word q / 32)
    int slabs, order, envelope, min_valid;
};

// the diagonals of D'D at row i, `off` columns to the right (mod16_amd/smooth.py: penalty_bands): row r
// of D holds k[0 .. order] in the columns r .. r + order
__host__ __device__ __forceinline__ double smooth_band(int i, int S, int order, int off) {
    const int k0 = order == 2 ? 1 : -1, k1 = order == 2 ? -2 : 1, k2 = order == 2 ? 1 : 0;
    const int rows = S - order;
    const int prod[3] = {off == 0 ? k0 * k0 : off == 1 ? k0 * k1 : k0 * k2,
                         off == 0 ? k1 * k1 : off == 1 ? k1 * k2 : 0,
                         off == 0 ? k2 * k2 : 0};
    int s = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (i - j >= 0 && i - j < rows) s += prod[j];
    return (double)s;
}

__host__ __device__ __forceinline__ bool smooth_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

template <typename OUT> __host__ __device__ __forceinline__ OUT smooth_encode(double z, double scale) {
#pragma clang fp contract(off)
    return (OUT)(z * scale);
}
template <> __host__ __device__ __forceinline__ uint8_t smooth_encode<uint8_t>(double z, double) {
#pragma clang fp contract(off)
    double r = __builtin_floor(z + 0.5);
    r = r < 0.0 ? 0.0 : r;
    r = r > 248.0 ? 248.0 : r;
    return (uint8_t)(int)r;
}
template <typename OUT> __host__ __device__ __forceinline__ OUT smooth_missing() { return (OUT)__builtin_nan(""); }
template <> __host__ __device__ __forceinline__ uint8_t smooth_missing<uint8_t>() { return 255; }

// One pixel: p of the call, whose columns are element `slot` of every row of the workspace. `tab`: the
// 256 QC weights.
template <typename IN, typename OUT>
__host__ __device__ __forceinline__ void smooth_pixel(const SmoothArgs& a, int64_t p, int64_t slot, const double* tab) {
#pragma clang fp contract(off)
    const int S = a.slabs, order = a.order;
    const double lam = a.lam;
    const IN* const in = static_cast<const IN*>(a.in) + p;
    OUT* const out = static_cast<OUT*>(a.out) + p;
    double* const ws = a.ws + slot;
    const int64_t L = a.lanes;
    auto col = [&](int k, int t) -> double& { return ws[((int64_t)k * S + t) * L]; };
    // (y, w) of slab t: 0.0 both where the slab is missing
    auto load = [&](int t, double& y, double& w) {
        const IN v = in[(int64_t)t * a.in_pitch];
        bool have;
        y = (double)v;
        if constexpr (std::is_same<IN, uint8_t>::value) have = v < kSmoothFill;
        else have = smooth_finite(y);
        if (a.weights) w = (double)a.weights[(int64_t)t * a.w_pitch + p];
        else if (a.qc) w = tab[a.qc[(int64_t)t * a.w_pitch + p]];
        else w = 1.0;
        have = have && smooth_finite(w) && w > 0.0;
        y = have ? y : 0.0;
        w = have ? w : 0.0;
    };
    const bool env = a.envelope > 0;

    // the factorisation and the first forward substitution
    int count = 0;
    {
        double d1 = 0.0, d2 = 0.0, c1 = 0.0, e1 = 0.0, e2 = 0.0, f1 = 0.0, f2 = 0.0;
        for (int i = 0; i < S; ++i) {
            double y, w;
            load(i, y, w);
            count += w > 0.0 ? 1 : 0;
            const double d = ((w + lam * smooth_band(i, S, order, 0)) - (c1 * c1) * d1) - (e2 * e2) * d2;
            const double c = (lam * smooth_band(i, S, order, 1) - (d1 * c1) * e1) / d;
            const double e = (lam * smooth_band(i, S, order, 2)) / d;
            const double f = (w * y - c1 * f1) - e2 * f2;
            col(kSmoothColC, i) = c;
            col(kSmoothColE, i) = e;
            col(kSmoothColG, i) = f / d;
            if (env) {
                col(kSmoothColY, i) = y;
                col(kSmoothColD, i) = d;
            }
            d2 = d1; d1 = d; c1 = c; e2 = e1; e1 = e; f2 = f1; f1 = f;
        }
    }
    if (a.count) a.count[p] = (uint16_t)count;
    if (count < a.min_valid) {          // unsmoothed
        for (int i = 0; i < S; ++i) out[(int64_t)i * a.out_pitch] = smooth_missing<OUT>();
        return;
    }
    for (int round = 0;; ++round) {
        const bool last = round == a.envelope;
        double z1 = 0.0, z2 = 0.0;
        for (int i = S - 1; i >= 0; --i) {
            const double z = (col(kSmoothColG, i) - col(kSmoothColC, i) * z1) - col(kSmoothColE, i) * z2;
            if (last) out[(int64_t)i * a.out_pitch] = smooth_encode<OUT>(z, a.scale);
            else col(kSmoothColG, i) = z;
            z2 = z1; z1 = z;
        }
        if (last) break;
        // the lift towards the upper envelope, and the forward substitution of the next round
        double c1 = 0.0, e1 = 0.0, e2 = 0.0, f1 = 0.0, f2 = 0.0;
        for (int i = 0; i < S; ++i) {
            double unused, w;
            load(i, unused, w);
            const double z = col(kSmoothColG, i);
            double y = col(kSmoothColY, i);
            if (w > 0.0 && z > y) {
                y = z;
                col(kSmoothColY, i) = y;
            }
            const double f = (w * y - c1 * f1) - e2 * f2;
            col(kSmoothColG, i) = f / col(kSmoothColD, i);
            c1 = col(kSmoothColC, i);
            e2 = e1; e1 = col(kSmoothColE, i);
            f2 = f1; f1 = f;
        }
    }
}

template <typename IN, typename OUT>
__global__ __launch_bounds__(kBlock) void smooth_kernel(SmoothArgs a) {
    __shared__ double tab[256];
    if (a.qc) {
        const int q = threadIdx.x;
        double w;
        if (a.qc_weight) {
            w = a.qc_weight[q];
        } else {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if ((q >> 5) == k) word = a.good_bits[k];
            w = (word >> (q & 31)) & 1u ? 1.0 : 0.0;
        }
        tab[q] = w;
    }
    __syncthreads();
    const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t p = slot; p < a.n; p += a.lanes) smooth_pixel<IN, OUT>(a, p, slot, tab);
}

}  // namespace mod16
