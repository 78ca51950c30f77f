// Per-pixel weighted least squares over a stack, shared and per-pixel terms: the kernel of
// mod16_regress_f32 / _f64. The definition is the numpy statement mod16_amd/regress.py (accumulate,
// factor, solve, residual_sums, inverse_diagonal); this file follows it operation for operation, in
// float64 and without contraction, so the outputs are its bits.
//
// Shape: time is the strided axis and a lane owns one pixel, so a wave's load of a slab of the values,
// of a per-pixel term or of the weights is one contiguous run of 64 elements. The lane's whole state is
// the upper triangle of the P x P Gram matrix, the right-hand side and two sums -- P (P + 1) / 2 + P + 2
// doubles, 46 at P = 8 -- in registers: the kernel is instantiated per P and every index into that state
// is a constant after unrolling (no per-lane array in memory, no scratch). The factorisation L diag(d) L'
// overwrites the triangle in place (L[i][j] where G[j][i] was, d[j] on the diagonal); the solution
// overwrites the right-hand side.
//
// The shared design row of a step is the same for every lane of every wave: its address depends on the
// step alone, so it is read through uniform (scalar) loads, Ks doubles per step and wave, and held in
// scalar registers. Staging it in LDS instead would take T x Ks x 8 bytes -- up to 256 KiB, more than the
// 160 KiB there are -- in chunks with a barrier per chunk, and would put it in vector registers, which
// the Gram state needs; the scalar cache and the L2 serve a row that every wave reads in the same order.
//
// Two streaming passes over the stacks, both from HBM: pass 1 accumulates, pass 2 forms the fitted value,
// the residual and the two sums of squares (and writes the series output). Per pixel-step that is 2 x
// (1 + Kp) values and 2 weights read and one series value written: DESIGN.md 8r counts the bytes. The raw
// values of step i + 1 are loaded before the arithmetic of step i is done (P (P + 3) / 2 multiply-adds,
// 44 at P = 8), so the loads are in flight behind it -- the concern mod16_daynight.hpp documents.
// Every output element of a pixel is written exactly once, by its lane; a lane past n does nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mod16 {

constexpr int kRegressMaxSteps = 4096;
constexpr int kRegressMaxTerms = 8;
enum { kRegressSeriesNone = 0, kRegressSeriesResiduals = 1, kRegressSeriesFitted = 2 };

struct RegressArgs {
    const void* values;                  // [T][v_pitch] of IN
    const double* design;                // [T][ks], on the device; NULL where ks = 0
    const void* cols[kRegressMaxTerms];  // cols[a] for a >= ks: the per-pixel term a - ks, [T][t_pitch] of IN; NULL below
    const float* weights;                // [T][w_pitch], or NULL
    double* coef;                        // [P][coef_pitch]
    double* se;                          // [P][se_pitch], or NULL
    double* rss;                         // [n] each, or NULL
    double* tss;
    double* r2;
    uint16_t* count;                     // [n], or NULL
    void* series;                        // [T][s_pitch] of IN, or NULL
    int64_t n, v_pitch, t_pitch, w_pitch, coef_pitch, se_pitch, s_pitch;
    int steps, ks, min_valid, series_mode;
};

__host__ __device__ __forceinline__ bool regress_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }
// where G[a][b], b >= a, sits in the packed upper triangle of a P x P matrix
template <int P> __host__ __device__ constexpr int regress_at(int a, int b) { return a * P - a * (a - 1) / 2 + (b - a); }

// what a lane loads of one step: the value, the per-pixel terms (0 below ks) and the weight, as stored
template <typename IN, int P> struct RegressRaw {
    IN y;
    IN t[P];
    float w;
};

template <typename IN, int P>
__host__ __device__ __forceinline__ void regress_load(const RegressArgs& a, int64_t p, int i, RegressRaw<IN, P>& r) {
    r.y = static_cast<const IN*>(a.values)[(int64_t)i * a.v_pitch + p];
#pragma unroll
    for (int c = 0; c < P; ++c) r.t[c] = c >= a.ks ? static_cast<const IN*>(a.cols[c])[(int64_t)i * a.t_pitch + p] : (IN)0;
    r.w = a.weights ? a.weights[(int64_t)i * a.w_pitch + p] : 1.0f;
}

// y, x[0 .. P - 1] and w of step i in float64; -> have_terms (every per-pixel term finite); valid: the
// sample counts
template <typename IN, int P>
__host__ __device__ __forceinline__ bool regress_sample(const RegressArgs& a, int i, const RegressRaw<IN, P>& r, double& y,
                                                        double (&x)[P], double& w, bool& valid) {
    // the design row: P uniform loads issued together and waited for once (a column past ks - 1 reads the
    // last one again and is not used), no branch per column
    double row[P];
    if (a.ks > 0) {
        const double* const shared = a.design + (int64_t)i * a.ks;
#pragma unroll
        for (int c = 0; c < P; ++c) row[c] = shared[c < a.ks ? c : a.ks - 1];
    }
    bool have = true;
    y = (double)r.y;
#pragma unroll
    for (int c = 0; c < P; ++c) {
        if (c < a.ks) {
            x[c] = row[c];
        } else {
            x[c] = (double)r.t[c];
            have = have && regress_finite(x[c]);
        }
    }
    w = (double)r.w;
    valid = regress_finite(y) && have && regress_finite(w) && w > 0.0;
    return have;
}

template <typename IN, int P>
__host__ __device__ __forceinline__ void regress_pixel(const RegressArgs& a, int64_t p) {
#pragma clang fp contract(off)
    constexpr int NG = P * (P + 1) / 2;
    const int T = a.steps;
    const double nan = __builtin_nan("");
    double G[NG], h[P];
#pragma unroll
    for (int k = 0; k < NG; ++k) G[k] = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) h[k] = 0.0;
    double Sw = 0.0, Sy = 0.0;
    int count = 0;

    // pass 1: the Gram matrix, the right-hand side and the two sums; the next step's loads first
    RegressRaw<IN, P> cur, next;
    regress_load<IN, P>(a, p, 0, cur);
    for (int i = 0; i < T; ++i) {
        regress_load<IN, P>(a, p, i + 1 < T ? i + 1 : i, next);
        double y, w, x[P];
        bool valid;
        regress_sample<IN, P>(a, i, cur, y, x, w, valid);
        if (valid) {      // (a branch, not selects: the lanes of the samples left out are masked off)
            count += 1;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const double wx = w * x[c];
                h[c] = h[c] + wx * y;
#pragma unroll
                for (int b = c; b < P; ++b) G[regress_at<P>(c, b)] = G[regress_at<P>(c, b)] + wx * x[b];
            }
            Sw = Sw + w;
            Sy = Sy + w * y;
        }
        cur = next;
    }

    // G = L diag(d) L' in place, no pivoting: L[i][j] takes the place of G[j][i], d[j] that of G[j][j]
    bool degenerate = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double gjj = G[regress_at<P>(j, j)];
        double dj = gjj;
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - (G[regress_at<P>(k, j)] * G[regress_at<P>(k, j)]) * G[regress_at<P>(k, k)];
        degenerate = degenerate || !(dj > 0x1p-40 * gjj);
#pragma unroll
        for (int i = j + 1; i < P; ++i) {
            double s = G[regress_at<P>(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - (G[regress_at<P>(k, i)] * G[regress_at<P>(k, j)]) * G[regress_at<P>(k, k)];
            G[regress_at<P>(j, i)] = s / dj;
        }
        G[regress_at<P>(j, j)] = dj;
    }
    // L z = h, c = z / d, L' b = c: b takes the place of h
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double s = h[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - G[regress_at<P>(k, i)] * h[k];
        h[i] = s;
    }
#pragma unroll
    for (int i = 0; i < P; ++i) h[i] = h[i] / G[regress_at<P>(i, i)];
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        double s = h[i];
#pragma unroll
        for (int k = i + 1; k < P; ++k) s = s - G[regress_at<P>(i, k)] * h[k];
        h[i] = s;
    }
    const bool empty = count < a.min_valid || degenerate;

    // pass 2: fitted values, residuals, the two sums of squares, the series
    const double ybar = Sy / Sw;
    double rss = 0.0, tss = 0.0;
    IN* const series = static_cast<IN*>(a.series);
    regress_load<IN, P>(a, p, 0, cur);
    for (int i = 0; i < T; ++i) {
        regress_load<IN, P>(a, p, i + 1 < T ? i + 1 : i, next);
        double y, w, x[P];
        bool valid;
        const bool have = regress_sample<IN, P>(a, i, cur, y, x, w, valid);
        double f = x[0] * h[0];
#pragma unroll
        for (int c = 1; c < P; ++c) f = f + x[c] * h[c];
        const double r = y - f;
        const double dy = y - ybar;
        if (valid) {
            rss = rss + w * (r * r);
            tss = tss + w * (dy * dy);
        }
        if (series) {
            const bool residuals = a.series_mode == kRegressSeriesResiduals;
            const bool keep = (residuals ? valid : have) && !empty;
            series[(int64_t)i * a.s_pitch + p] = (IN)(keep ? (residuals ? r : f) : nan);
        }
        cur = next;
    }

#pragma unroll
    for (int j = 0; j < P; ++j) a.coef[(int64_t)j * a.coef_pitch + p] = empty ? nan : h[j];
    if (a.rss) a.rss[p] = empty ? nan : rss;
    if (a.tss) a.tss[p] = empty ? nan : tss;
    if (a.r2) a.r2[p] = empty ? nan : 1.0 - rss / tss;
    if (a.count) a.count[p] = (uint16_t)count;
    if (a.se) {
        const double sigma2 = rss / (double)(count - P);
        // column j of M, the inverse of the unit triangle L, and with it entry j of the inverse's diagonal
#pragma unroll
        for (int j = 0; j < P; ++j) {
            double M[P];
            M[j] = 1.0;
#pragma unroll
            for (int i = j + 1; i < P; ++i) {
                double s = G[regress_at<P>(j, i)];
#pragma unroll
                for (int k = j + 1; k < i; ++k) s = s + G[regress_at<P>(k, i)] * M[k];
                M[i] = -s;
            }
            double t = (M[j] * M[j]) / G[regress_at<P>(j, j)];
#pragma unroll
            for (int k = j + 1; k < P; ++k) t = t + (M[k] * M[k]) / G[regress_at<P>(k, k)];
            a.se[(int64_t)j * a.se_pitch + p] = empty ? nan : __builtin_sqrt(sigma2 * t);
        }
    }
}

template <typename IN, int P>
__global__ __launch_bounds__(kBlock) void regress_kernel(RegressArgs a) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p < a.n) regress_pixel<IN, P>(a, p);
}

}  // namespace mod16
