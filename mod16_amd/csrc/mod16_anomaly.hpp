// Per-pixel climatology, standardized anomalies and percentile ranks over a record of Y years x P
// periods of composites: the kernel of mod16_anomaly_f32 / _f64. The definition is the numpy statement
// mod16_amd/anomaly.py (anomaly); this file follows it step for step, and every float operation it
// names is one correctly rounded float64 operation here (no contraction anywhere in this file).
//
// Shape: a lane owns one pixel and walks a run of periods; per (pixel, period) the Y windowed values
// r live in LDS as a column, value y of lane l at y * LANES + l (8-byte elements, lane-major:
// ds_read_b64 / ds_write_b64 of consecutive lanes touch consecutive banks, no conflict, no padding).
// Registers cannot hold r behind a run-time year index; LDS can. A lane reads and writes its own
// column only, so the kernel has no barrier and no atomics. A block has kAnomalyLanes = 128 lanes and
// exactly Y rows of dynamic LDS, Y KiB (64 KiB at the most): LDS is what bounds the occupancy, and a CU
// (160 KiB) holds 160 / Y blocks -- 6 blocks, 12 waves at Y = 24; 2 blocks at Y = 64.
//
//   1  r of kAnomalyBatch = 8 years at a time: the window's W loads per array and year are issued
//      term by term for the eight years together (sixteen independent loads in flight per lane),
//      summed from the oldest term as the definition does -- there is no sliding update -- then
//      divided; r or NaN goes to LDS, m and sum accumulate over the baseline years;
//   2  ss from LDS, over the baseline years;
//   3  per year z and, where asked for, the rank from an inner loop over the baseline column in LDS
//      (the counts are integers: pct is exact up to its one division).
//
// Grid: block b takes pixels (b % pixel_blocks) * LANES ... and the periods of chunk b / pixel_blocks;
// the host cuts P into chunks only as far as it takes to fill the device, so the W - 1 earlier slabs
// a period re-reads were read by the same lane one period earlier (L2 / Infinity Cache, not HBM).
// Consecutive lanes take consecutive pixels: every global access is coalesced along the pixel axis.
// Pixels behind n take NaN for every term and store nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mod16 {

constexpr int kAnomalyMaxWindow = 16;
constexpr int kAnomalyMaxYears = 64;
constexpr int kAnomalyMaxPeriods = 366;
constexpr int kAnomalyMaxSlabs = 4096;
constexpr int kAnomalyBatch = 8;              // years whose loads are in flight together
constexpr int kAnomalyLanes = 128;            // lanes, and pixels, of a block

struct AnomalyArgs {
    const void* num;                     // [years * periods][in_stride] of IN
    const void* den;                     // likewise, or NULL
    void* z;                             // [years * periods][out_stride] of IN, or NULL
    void* pct;                           // likewise
    double* mean;                        // [periods][clim_stride], or NULL
    double* std;                         // likewise
    uint8_t* count;                      // [periods][count_stride], or NULL
    int64_t n, in_stride, out_stride, clim_stride, count_stride;
    int64_t pixel_blocks;                // blocks along the pixel axis
    int years, periods, window, base_first, base_end, min_valid;
    int chunk;                           // periods of a block
};

// the dynamic LDS of a block: its lanes' columns of `years` values
inline size_t anomaly_lds_bytes(int years) { return (size_t)years * kAnomalyLanes * sizeof(double); }

__device__ __forceinline__ bool anomaly_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

template <typename IN, bool DEN>
__global__ __launch_bounds__(kAnomalyLanes) void anomaly_kernel(AnomalyArgs a) {
#pragma clang fp contract(off)
    constexpr int LANES = kAnomalyLanes;
    constexpr int B = kAnomalyBatch;
    static_assert(kAnomalyMaxYears * LANES * 8 <= 65536, "the columns of a block");
    extern __shared__ double anomaly_col[];       // [years][LANES]

    const int lane = threadIdx.x;
    const int64_t pb = (int64_t)blockIdx.x % a.pixel_blocks;
    const int chunk = (int)((int64_t)blockIdx.x / a.pixel_blocks);
    const int64_t pix = pb * LANES + lane;
    const bool live = pix < a.n;
    const int Y = a.years, P = a.periods, W = a.window;
    const int p_end = min(P, (chunk + 1) * a.chunk);
    const double nan = __builtin_nan("");
    const int64_t pix_in = live ? pix : a.n - 1;  // a pixel behind n reads the last pixel, and drops it
    const IN* const num = static_cast<const IN*>(a.num) + pix_in;
    const IN* const den = DEN ? static_cast<const IN*>(a.den) + pix_in : nullptr;
    IN* const zo = static_cast<IN*>(a.z);
    IN* const po = static_cast<IN*>(a.pct);
    double* const r = anomaly_col + lane;

    for (int p = chunk * a.chunk; p < p_end; ++p) {
        // 1: the windowed values, B years at a time
        int m = 0;
        double sum = 0.0;
        for (int y0 = 0; y0 < Y; y0 += B) {
            double s1[B], s2[B];
            int slab[B];
            bool have[B];
#pragma unroll
            for (int j = 0; j < B; ++j) {
                s1[j] = 0.0;
                s2[j] = 0.0;
                // slab (y0 + j) P + p has its W terms: every slab but the first W - 1 of the record
                slab[j] = min(y0 + j, Y - 1) * P + p;
                have[j] = live && y0 + j < Y && slab[j] >= W - 1;
            }
            for (int k = W - 1; k >= 0; --k) {             // the oldest term first
                // no load sits behind a branch, so the 2 B loads of a term are in flight together: one
                // that has no term reads a slab of the record all the same (a year behind the last
                // reads the last year's, a term in front of the record slab 0) and becomes NaN
                IN t1[B], t2[B];
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const int64_t at = (int64_t)max(slab[j] - k, 0) * a.in_stride;
                    t1[j] = num[at];
                    if (DEN) t2[j] = den[at];
                }
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    s1[j] = s1[j] + (have[j] ? (double)t1[j] : nan);
                    if (DEN) s2[j] = s2[j] + (have[j] ? (double)t2[j] : nan);
                }
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const double v = DEN ? s1[j] / s2[j] : s1[j];
                const bool ok = anomaly_finite(v) && (!DEN || (s2[j] > 0.0 && s2[j] < __builtin_inf()));
                if (y0 + j < Y) r[(y0 + j) * LANES] = ok ? v : nan;
                if (ok && y0 + j >= a.base_first && y0 + j < a.base_end) {   // base_end <= Y
                    ++m;
                    sum = sum + v;
                }
            }
        }
        // 2: the moments of the baseline
        const double mean = sum / (double)m;
        double ss = 0.0;
        for (int y = a.base_first; y < a.base_end; ++y) {
            const double v = r[y * LANES];
            if (v == v) {
                const double e = v - mean;
                const double sq = e * e;
                ss = ss + sq;
            }
        }
        const double sd = __builtin_sqrt(ss / (double)(m - 1));
        const bool enough = m >= a.min_valid;
        if (live) {
            if (a.mean) a.mean[(int64_t)p * a.clim_stride + pix] = enough ? mean : nan;
            if (a.std) a.std[(int64_t)p * a.clim_stride + pix] = enough ? sd : nan;
            if (a.count) a.count[(int64_t)p * a.count_stride + pix] = (uint8_t)m;
        }
        // 3: the anomaly and the rank of every year
        if (!zo && !po) continue;
        const bool scored = enough && anomaly_finite(sd) && sd > 0.0;
        const double mf = (double)m;
        for (int y = 0; y < Y; ++y) {
            const double v = r[y * LANES];
            const bool ok = v == v;
            const int64_t at = (int64_t)(y * P + p) * a.out_stride + pix;
            if (zo) {
                const double z = ok && scored ? (v - mean) / sd : nan;
                if (live) zo[at] = (IN)z;
            }
            if (po) {
                int lt = 0, eq = 0;
                for (int u = a.base_first; ok && enough && u < a.base_end; ++u) {
                    const double w = r[u * LANES];         // a missing value is NaN: neither below nor equal
                    lt += w < v;
                    eq += w == v;
                }
                const double half = 0.5 * (double)eq;
                const double rank = ok && enough ? ((double)lt + half) / mf : nan;
                if (live) po[at] = (IN)rank;
            }
        }
    }
}

}  // namespace mod16
