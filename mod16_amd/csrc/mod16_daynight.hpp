// Hourly reanalysis aggregated into day / night drivers: the kernels of mod16_daynight_f32 / _f64.
// The definition is the numpy statement mod16_amd/daynight.py (day_weights, sw_weights, split_field,
// aggregate); this file follows it operation for operation, contraction off.
//
// Shape: time is the strided axis, cells the contiguous one. A lane owns kDnPx = 2 consecutive cells
// of one row (one 8-byte load per float32 field and step, 16 bytes stored per float64 output plane)
// and a chunk of consecutive days (grid: cell tiles x day chunks, so a small grid with many days
// still fills the device). Per day it forms sunrise and sunset in UTC steps once per cell ('solar'
// mode: two divisions), walks the H steps in a wave-uniform loop -- the weight of a step is made in
// registers from min / max / add and never stored -- and keeps per cell sum_w, sum_n, three sums per
// field and tmin: 18 float64 accumulators, 20 with the day's a and b, 80 registers for the lane's two
// cells and 162 for the kernel: three waves per SIMD. (Four cells per lane need 280 registers: the
// compiler parks 24 of them in the accumulator file, which tests/test_abi.py forbids, and one wave
// per SIMD would hold fewer bytes in flight than three waves of half the width.) Every hourly value
// is read once, every requested output element [d][r][0, W) written exactly once; no workspace, no
// atomics.
//
// temp_annual needs the daily means of ALL days in day order: where it is wanted the kernel also
// leaves the day's float64 mean of t in a dense workspace plane (8 bytes per cell-day), and
// daynight_annual_kernel, a lane per cell, adds those planes sequentially -- across the day chunks of
// HOST mode through a float64 plane (first / last).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mod16_kernels.hpp"

namespace mod16 {

constexpr int kDnPx = 2;
static_assert(kDnPx == 2, "dn_load / dn_store move two cells");
constexpr int kDnMaxSteps = 48;
constexpr int kDnMaxDays = 4096;
constexpr int kDnMinChunk = 4;     // days per lane at least (where the call has them): the row and column setup amortised
enum { kDnT = 0, kDnQv, kDnPs, kDnSw, kDnLw, kDnFields };
enum { kDnLwDay = 0, kDnLwNight, kDnSwDay, kDnTDay, kDnTNight, kDnTmin, kDnVpdDay, kDnVpdNight, kDnHours, kDnTMean, kDnOutputs };
enum { kDnWideIn = 1, kDnWideOut = 2 };    // DnArgs::wide: bases, pitches and plane strides are multiples of the vector size (two elements)
enum { kDnModeSolar = 0, kDnModeSw = 1 };

struct DnArgs {
    const void* field[kDnFields];   // [days * steps][rows][in_pitch] of IN, or NULL
    void* out[kDnOutputs];          // [days][rows][out_pitch] of OUT, or NULL
    const double* half_day;         // [days][rows]    ('solar')
    const double* noon;             // [days]
    const double* offset;           // [cols]
    double* mean64;                 // [days][rows * cols]: the unrounded daily mean of t for temp_annual, or NULL
    int64_t in_pitch, in_plane, out_pitch, out_plane;
    int64_t lanes_per_row;
    double delta, hd, threshold;    // 24 / H, H, 'sw' mode's threshold
    int rows, cols, days, steps, mode, wide, chunk;
};

struct DnAnnualArgs {
    const double* mean64;           // [days][rows * cols]
    double* acc;                    // [rows * cols]: the running sum between two chunks (NULL: first and last)
    void* out;                      // [rows][out_pitch] of OUT (last)
    int64_t out_pitch;
    double total_days;
    int rows, cols, days, first, last;
};

// a lane's two cells of one step, widened: one vector load, or the first nv alone
__device__ __forceinline__ void dn_load(const float* p, bool wide, int nv, double (&x)[kDnPx]) {
    if (wide) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        x[0] = (double)v.x; x[1] = (double)v.y;
    } else {
#pragma unroll
        for (int j = 0; j < kDnPx; ++j) x[j] = j < nv ? (double)p[j] : 0.0;
    }
}
__device__ __forceinline__ void dn_load(const double* p, bool wide, int nv, double (&x)[kDnPx]) {
    if (wide) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        x[0] = v.x; x[1] = v.y;
    } else {
#pragma unroll
        for (int j = 0; j < kDnPx; ++j) x[j] = j < nv ? p[j] : 0.0;
    }
}
// ... and of one output plane, each value rounded once
__device__ __forceinline__ void dn_store(float* p, bool wide, int nv, const double (&v)[kDnPx]) {
    if (wide) {
        *reinterpret_cast<float2*>(p) = make_float2((float)v[0], (float)v[1]);
    } else {
#pragma unroll
        for (int j = 0; j < kDnPx; ++j)
            if (j < nv) p[j] = (float)v[j];
    }
}
__device__ __forceinline__ void dn_store(double* p, bool wide, int nv, const double (&v)[kDnPx]) {
    if (wide) {
        *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    } else {
#pragma unroll
        for (int j = 0; j < kDnPx; ++j)
            if (j < nv) p[j] = v[j];
    }
}

// one window of day_weights: max(min(k + 1, b + m) - max(k, a + m), 0)
__device__ __forceinline__ double dn_window(double k0, double k1, double a, double b, double m) {
#pragma clang fp contract(off)
    return fmax(fmin(k1, b + m) - fmax(k0, a + m), 0.0);
}

template <typename IN, typename OUT>
__global__ __launch_bounds__(kBlock) void daynight_kernel(DnArgs a) {
#pragma clang fp contract(off)
    constexpr int PX = kDnPx;
    const int64_t lane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (lane >= a.lanes_per_row * (int64_t)a.rows) return;
    const int r = (int)(lane / a.lanes_per_row);
    const int c0 = (int)(lane - (int64_t)r * a.lanes_per_row) * PX;
    const int nv = a.cols - c0 < PX ? a.cols - c0 : PX;
    const bool win = nv == PX && (a.wide & kDnWideIn);
    const bool wout = nv == PX && (a.wide & kDnWideOut);
    const bool solar = a.mode == kDnModeSolar;
    const int H = a.steps;
    const double hd = a.hd, delta = a.delta;
    const int d0 = (int)blockIdx.y * a.chunk;
    const int d1 = d0 + a.chunk < a.days ? d0 + a.chunk : a.days;
    const IN* const fld[kDnFields] = {static_cast<const IN*>(a.field[0]), static_cast<const IN*>(a.field[1]),
                                      static_cast<const IN*>(a.field[2]), static_cast<const IN*>(a.field[3]),
                                      static_cast<const IN*>(a.field[4])};
    double off[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) off[j] = (solar && j < nv) ? a.offset[c0 + j] : 0.0;

    for (int d = d0; d < d1; ++d) {
        double sa[PX], sb[PX];          // sunrise and sunset in UTC steps
#pragma unroll
        for (int j = 0; j < PX; ++j) sa[j] = sb[j] = 0.0;
        if (solar) {
            const double half = a.half_day[(int64_t)d * a.rows + r], noon = a.noon[d];
            const double lo = noon - half, hi = noon + half;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                sa[j] = (lo - off[j]) / delta;
                sb[j] = (hi - off[j]) / delta;
            }
        }
        double sum_w[PX], sum_n[PX], sx[kDnFields][PX], swx[kDnFields][PX], snx[kDnFields][PX], tmin[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            sum_w[j] = sum_n[j] = 0.0;
            tmin[j] = __builtin_inf();
#pragma unroll
            for (int f = 0; f < kDnFields; ++f) sx[f][j] = swx[f][j] = snx[f][j] = 0.0;
        }
        int64_t at = (int64_t)d * H * a.in_plane + (int64_t)r * a.in_pitch + c0;
        for (int k = 0; k < H; ++k) {
            double x[kDnFields][PX];
#pragma unroll
            for (int f = 0; f < kDnFields; ++f) {
                if (fld[f]) {
                    dn_load(fld[f] + at, win, nv, x[f]);
                } else {
#pragma unroll
                    for (int j = 0; j < PX; ++j) x[f][j] = 0.0;
                }
            }
            at += a.in_plane;
            const double k0 = (double)k, k1 = k0 + 1.0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                double w;
                if (solar) {
                    const double t0 = dn_window(k0, k1, sa[j], sb[j], -hd);
                    const double t1 = dn_window(k0, k1, sa[j], sb[j], 0.0);
                    const double t2 = dn_window(k0, k1, sa[j], sb[j], hd);
                    w = fmin((t0 + t1) + t2, 1.0);
                } else {
                    const double s = x[kDnSw][j];
                    w = s != s ? s : (s > a.threshold ? 1.0 : 0.0);
                }
                const double u = 1.0 - w;
                sum_w[j] = sum_w[j] + w;
                sum_n[j] = sum_n[j] + u;
#pragma unroll
                for (int f = 0; f < kDnFields; ++f) {
                    const double v = x[f][j];
                    const double pw = w * v, pn = u * v;
                    sx[f][j] = sx[f][j] + v;
                    swx[f][j] = swx[f][j] + pw;
                    snx[f][j] = snx[f][j] + pn;
                }
                const double t = x[kDnT][j];
                tmin[j] = (t < tmin[j] || t != t) ? t : tmin[j];     // (a NaN stays: nothing is < NaN)
            }
        }
        // the day's values
        const int64_t oat = (int64_t)d * a.out_plane + (int64_t)r * a.out_pitch + c0;
        double day[kDnFields][PX], night[kDnFields][PX], mean[kDnFields][PX], v[PX];
#pragma unroll
        for (int f = 0; f < kDnFields; ++f)
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                mean[f][j] = sx[f][j] / hd;
                day[f][j] = sum_w[j] > 0.0 ? swx[f][j] / sum_w[j] : mean[f][j];
                night[f][j] = sum_n[j] > 0.0 ? snx[f][j] / sum_n[j] : mean[f][j];
            }
        auto put = [&](int o, const double (&val)[PX]) {
            if (a.out[o]) dn_store(static_cast<OUT*>(a.out[o]) + oat, wout, nv, val);
        };
        put(kDnLwDay, day[kDnLw]);
        put(kDnLwNight, night[kDnLw]);
        put(kDnSwDay, day[kDnSw]);
        put(kDnTDay, day[kDnT]);
        put(kDnTNight, night[kDnT]);
        put(kDnTmin, tmin);
        put(kDnTMean, mean[kDnT]);
        if (a.mean64) {
            double* const m = a.mean64 + ((int64_t)d * a.rows + r) * a.cols + c0;
#pragma unroll
            for (int j = 0; j < PX; ++j)
                if (j < nv) m[j] = mean[kDnT][j];
        }
        if (a.out[kDnHours]) {
#pragma unroll
            for (int j = 0; j < PX; ++j) v[j] = delta * sum_w[j];
            put(kDnHours, v);
        }
        if (a.out[kDnVpdDay]) {
#pragma unroll
            for (int j = 0; j < PX; ++j) v[j] = vpd_exact<double>(day[kDnQv][j], day[kDnPs][j], day[kDnT][j]);
            put(kDnVpdDay, v);
        }
        if (a.out[kDnVpdNight]) {
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const double q = vpd_exact<double>(night[kDnQv][j], night[kDnPs][j], night[kDnT][j]);
                v[j] = q < 0.0 ? 0.0 : q;
            }
            put(kDnVpdNight, v);
        }
    }
}

// temp_annual: (sum over d of the day's mean of t) / D per cell, sequential in d; eight planes' loads
// at a time in flight, added in day order
template <typename OUT>
__global__ __launch_bounds__(kBlock) void daynight_annual_kernel(DnAnnualArgs a) {
#pragma clang fp contract(off)
    const int64_t cells = (int64_t)a.rows * a.cols;
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= cells) return;
    const double* p = a.mean64 + cell;
    double acc = a.first ? 0.0 : a.acc[cell];
    int d = 0;
    for (; d + 8 <= a.days; d += 8) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i * cells];
        p += 8 * cells;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = acc + v[i];
    }
    for (; d < a.days; ++d) {
        acc = acc + *p;
        p += cells;
    }
    if (a.last) {
        const int64_t r = cell / a.cols, c = cell - r * a.cols;
        static_cast<OUT*>(a.out)[r * a.out_pitch + c] = (OUT)(acc / a.total_days);
    } else {
        a.acc[cell] = acc;
    }
}

}  // namespace mod16
