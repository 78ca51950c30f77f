// Per-pixel Mann-Kendall test and Theil-Sen slope over a stack of Y values (annual composites): the
// kernel of mod16_trend_f32 / _f64. The definition is the numpy statement mod16_amd/trend.py
// (pixel_trend); this file follows it step for step, and every float operation it names is one
// correctly rounded float64 operation here (no contraction anywhere in this file).
//
// Shape: the Y (Y - 1) / 2 pairwise slopes of a pixel are ordered in LDS. The host picks a capacity
// CAP, the power of two from 16 to 2048 that holds the pairs of the call's Y, and with it the layout:
// a lane owns kTrendOwn = 16 of a pixel's CAP slots, so L = CAP / 16 lanes share a pixel (1 lane at
// Y <= 6, 128 lanes -- two waves -- at Y >= 46) and a block of 256 lanes holds P = 4096 / CAP pixels
// (256 ... 2): 32 KiB of slopes per block at every capacity, plus one pad slot per 16 (below).
//
//   1  the block's P x Y values are read once, rows of P consecutive pixels, widened to float64 and
//      stored in LDS with -0.0 turned into 0.0 (equal values become indistinguishable);
//   2  per valid value (its lanes take the values round robin): how many valid values are equal to
//      it -- the tie term is the sum over values of (e - 1)(2 e + 5) -- and its rank among them,
//      which finds the one or two middle values of x and of t without ordering them;
//   3  the pair loop: slot i = u L + lane holds the pair (a, b), i = b (b - 1) / 2 + a -- sign and
//      slope (x[b] - x[a]) / (t[b] - t[a]) + 0.0 -- or +inf where a value is missing or behind the
//      last pair: a pixel with fewer valid years finds its own M slopes in front of the padding;
//   4  a bitonic network over the CAP slots: the strides below 16 of every merge run inside a lane's
//      own 16 slots in registers (one LDS read and one write per slot for four or, at the start, ten
//      stages), the strides from 16 up exchange through LDS, 8 pairs per lane and stage;
//   5  the pixel's first lane reads the ranks it needs and stores the outputs.
//
// LDS: slot p of a pixel lives at p + p / 16 (doubles), so the 16-slot runs of neighbouring lanes
// start 34 dwords apart: ds_read_b64 (banks of (a / 4) mod 64 per 32 lanes) and ds_write_b64 ((a / 4)
// mod 32 per 16 lanes) of step 4's register passes are conflict-free, as are the exchange stages
// (consecutive lanes, consecutive slots). No atomics: sums over a pixel's lanes go through
// cross-lane shuffles and, for two waves, one LDS slot each. Every lane reaches every barrier (no
// early return; pixels behind n load NaN and store nothing).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mod16 {

constexpr int kTrendMaxSteps = 64;
constexpr int kTrendOwn = 16;                 // slots of the network a lane owns
constexpr int kTrendMinCap = 16, kTrendMaxCap = 2048;
constexpr int kTrendSlots = 4096;             // slots of a block at every capacity
enum { kTrendSlope = 0, kTrendIntercept = 1, kTrendLo = 2, kTrendHi = 3, kTrendZ = 4, kTrendOutputs = 5 };

struct TrendArgs {
    const void* values;                  // [steps][time_stride] of IN
    const double* times;                 // [steps], on the device
    double* out[kTrendOutputs];          // [n] or NULL
    int32_t* s;                          // [n] or NULL
    uint8_t* count;                      // [n] or NULL
    int64_t n, time_stride;
    double zq;                           // 0: no interval
    int steps, min_valid;
};

// the most steps whose pairs fit a capacity (6, 8, 11, 16, 23, 32, 45, 64)
constexpr int trend_steps_of(int cap) {
    int y = 2;
    while ((y + 1) * y / 2 <= cap) ++y;
    return y;
}
// the capacity of a call: the power of two from kTrendMinCap that holds steps (steps - 1) / 2 pairs
inline int trend_capacity(int steps) {
    int cap = kTrendMinCap;
    while (cap < steps * (steps - 1) / 2) cap *= 2;
    return cap;
}

__device__ __forceinline__ bool trend_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }
__device__ __forceinline__ int trend_slot(int p) { return p + (p >> 4); }

// lo to a, hi to b (ascending) or the other way round; there is no NaN among the slopes
__device__ __forceinline__ void trend_cmpx(double& a, double& b, bool asc) {
    const bool sw = (a > b) == asc;
    const double x = sw ? b : a, y = sw ? a : b;
    a = x;
    b = y;
}
// one stage of stride J over a lane's 16 slots, in merges of size K: slot i goes up where bit K of i is
// clear (K < 16: the run lies inside the lane's slots), the whole lane goes `up` or down (K = 16 and wider)
template <int K, int J> __device__ __forceinline__ void trend_stage(double (&v)[kTrendOwn], bool up) {
#pragma unroll
    for (int i = 0; i < kTrendOwn; ++i)
        if ((i & J) == 0) trend_cmpx(v[i], v[i | J], K < kTrendOwn ? (i & K) == 0 : up);
}
// the 16 slots of a lane as the bitonic network orders them: runs of 2, 4, 8 alternate, the 16 go `up`
__device__ __forceinline__ void trend_sort16(double (&v)[kTrendOwn], bool up) {
    trend_stage<2, 1>(v, up);
    trend_stage<4, 2>(v, up); trend_stage<4, 1>(v, up);
    trend_stage<8, 4>(v, up); trend_stage<8, 2>(v, up); trend_stage<8, 1>(v, up);
    trend_stage<16, 8>(v, up); trend_stage<16, 4>(v, up); trend_stage<16, 2>(v, up); trend_stage<16, 1>(v, up);
}
// the last four stages of a wider merge
__device__ __forceinline__ void trend_merge16(double (&v)[kTrendOwn], bool up) {
    trend_stage<16, 8>(v, up); trend_stage<16, 4>(v, up); trend_stage<16, 2>(v, up); trend_stage<16, 1>(v, up);
}

// the sum of v over the L lanes of a pixel, in its first lane (L <= 64: lanes of one wave; 128: two
// waves and `two`, a slot per wave)
template <int L> __device__ __forceinline__ int trend_team_sum(int v, int* two) {
    constexpr int W = L < 64 ? L : 64;
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if constexpr (L > 64) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) two[wave] = v;
        __syncthreads();
        v = two[wave & ~1] + two[wave | 1];
        __syncthreads();
    }
    return v;
}

// the median rule: the middle one of k ascending values, or the mean of the two middle ones
__device__ __forceinline__ double trend_middle(double lo, double hi, int k) {
#pragma clang fp contract(off)
    return (k & 1) ? lo : (lo + hi) * 0.5;
}

template <typename IN, int CAP>
__global__ __launch_bounds__(kBlock) void trend_kernel(TrendArgs a) {
#pragma clang fp contract(off)
    constexpr int L = CAP / kTrendOwn;            // lanes of a pixel
    constexpr int P = kBlock / L;                 // pixels of a block
    constexpr int YM = trend_steps_of(CAP);
    constexpr int ROW = CAP + CAP / kTrendOwn;    // a pixel's slots and their pads
    static_assert(P * CAP == kTrendSlots && L * P == kBlock && L <= 128, "the layout of a block");
    __shared__ double slopes[P * ROW];
    __shared__ double xs[YM * P];                 // value y of pixel q at y P + q
    __shared__ double ts[kTrendMaxSteps];
    __shared__ double mid[P * 4];                 // per pixel: the middle values of x (lo, hi) and of t
    __shared__ int two[kBlock / 64];

    const int tid = threadIdx.x;
    const int Y = a.steps;
    const double inf = __builtin_inf();

    // 1: rows of P consecutive pixels, L rows at a time
    if (tid < Y) ts[tid] = a.times[tid];
    {
        const int p = tid % P;
        const int64_t pix = (int64_t)blockIdx.x * P + p;
        const IN* src = static_cast<const IN*>(a.values) + pix;
        for (int y = tid / P; y < Y; y += L) {
            double x = __builtin_nan("");
            if (pix < a.n) x = (double)src[(int64_t)y * a.time_stride];
            xs[y * P + p] = x + 0.0;
        }
    }
    __syncthreads();

    const int q = tid / L, lane = tid % L;        // this lane's pixel and its place among the pixel's lanes
    const int64_t pix = (int64_t)blockIdx.x * P + q;
    double* const row = slopes + q * ROW;

    // 2: equal values and ranks; every lane counts the pixel's valid values on the way
    int m = 0, tie = 0;
    for (int y = 0; y < Y; ++y) m += trend_finite(xs[y * P + q]);
    for (int i = lane; i < Y; i += L) {
        const double xi = xs[i * P + q];
        if (!trend_finite(xi)) continue;
        int below = 0, equal = 0, before = 0;
        for (int y = 0; y < Y; ++y) {
            const double xy = xs[y * P + q];
            const bool ok = trend_finite(xy);
            below += ok && (xy < xi || (xy == xi && y < i));
            equal += ok && xy == xi;
            before += ok && y < i;
        }
        tie += (equal - 1) * (2 * equal + 5);
        if (below == (m - 1) / 2) mid[q * 4 + 0] = xi;
        if (below == m / 2) mid[q * 4 + 1] = xi;
        if (before == (m - 1) / 2) mid[q * 4 + 2] = ts[i];
        if (before == m / 2) mid[q * 4 + 3] = ts[i];
    }

    // 3: the pairs
    const int pairs = Y * (Y - 1) / 2;
    int sgn = 0;
#pragma unroll 1
    for (int u = 0; u < kTrendOwn; ++u) {
        const int i = u * L + lane;
        double slope = inf;
        if (i < pairs) {
            // i = b (b - 1) / 2 + a with a < b: b from the root, put right by one where the estimate is off
            int b = (int)((1.0f + __fsqrt_rn((float)(8 * i + 1))) * 0.5f);
            if (b * (b - 1) / 2 > i) --b;
            if ((b + 1) * b / 2 <= i) ++b;
            const int lo = i - b * (b - 1) / 2;
            const double xa = xs[lo * P + q], xb = xs[b * P + q];
            if (trend_finite(xa) && trend_finite(xb)) {
                const double d = xb - xa;
                sgn += (d > 0.0) - (d < 0.0);
                slope = d / (ts[b] - ts[lo]) + 0.0;
            }
        }
        row[trend_slot(i)] = slope;
    }
    sgn = trend_team_sum<L>(sgn, two);
    tie = trend_team_sum<L>(tie, two);
    __syncthreads();

    // 4: the network
    double v[kTrendOwn];
    double* const own = row + lane * (kTrendOwn + 1);
#pragma unroll
    for (int i = 0; i < kTrendOwn; ++i) v[i] = own[i];
    trend_sort16(v, ((lane * kTrendOwn) & kTrendOwn) == 0);
#pragma unroll
    for (int i = 0; i < kTrendOwn; ++i) own[i] = v[i];
    for (int k = 2 * kTrendOwn; k <= CAP; k <<= 1) {
        for (int j = k >> 1; j >= kTrendOwn; j >>= 1) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kTrendOwn / 2; ++u) {
                const int i = u * L + lane;                       // pair i of the stage: slots p and p + j
                const int p = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                double x = row[trend_slot(p)], y = row[trend_slot(p + j)];
                trend_cmpx(x, y, (p & k) == 0);
                row[trend_slot(p)] = x;
                row[trend_slot(p + j)] = y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kTrendOwn; ++i) v[i] = own[i];
        trend_merge16(v, ((lane * kTrendOwn) & k) == 0);
#pragma unroll
        for (int i = 0; i < kTrendOwn; ++i) own[i] = v[i];
    }
    __syncthreads();

    // 5: the outputs, by the pixel's first lane
    if (lane != 0 || pix >= a.n) return;
    const double nan = __builtin_nan("");
    double slope = nan, intercept = nan, slo = nan, shi = nan, z = nan;
    int s = 0;
    if (m >= a.min_valid) {
        const int M = m * (m - 1) / 2;
        s = sgn;
        slope = trend_middle(row[trend_slot((M - 1) / 2)], row[trend_slot(M / 2)], M);
        const double mx = trend_middle(mid[q * 4 + 0], mid[q * 4 + 1], m);
        const double mt = trend_middle(mid[q * 4 + 2], mid[q * 4 + 3], m);
        const double product = slope * mt;
        intercept = mx - product;
        const int v18 = m * (m - 1) * (2 * m + 5) - tie;
        const double sigma = __builtin_sqrt((double)v18 / 18.0);
        z = (s == 0 || v18 == 0) ? 0.0 : (double)(s - (s > 0 ? 1 : -1)) / sigma;
        if (a.zq != 0.0) {
            const double c = a.zq * sigma;
            const double hi = __builtin_fmin(__builtin_rint(((double)M + c) / 2.0), (double)(M - 1));
            const double lo = __builtin_fmax(__builtin_rint(((double)M - c) / 2.0) - 1.0, 0.0);
            shi = row[trend_slot((int)hi)];
            slo = row[trend_slot((int)lo)];
        }
    }
    if (a.out[kTrendSlope]) a.out[kTrendSlope][pix] = slope;
    if (a.out[kTrendIntercept]) a.out[kTrendIntercept][pix] = intercept;
    if (a.out[kTrendLo]) a.out[kTrendLo][pix] = slo;
    if (a.out[kTrendHi]) a.out[kTrendHi][pix] = shi;
    if (a.out[kTrendZ]) a.out[kTrendZ][pix] = z;
    if (a.s) a.s[pix] = s;
    if (a.count) a.count[pix] = (uint8_t)m;
}

}  // namespace mod16
