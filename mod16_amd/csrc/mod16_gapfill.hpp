// QC-driven temporal gap filling of byte series (8-day fPAR / LAI codes): the kernel of
// mod16_gapfill_u8. The definition is the numpy statement mod16_amd/gapfill.py (reliable,
// fill_series, encode); this file follows it case for case.
//
// Shape: time is the strided axis. A lane owns PX consecutive pixels (16 for uint8 output, 8 for
// float32, 4 for float64: 16 input bytes per lane where the output is as narrow as the input, and no
// more than 32 output bytes per lane and slab where it is wider, so that a wave's stores of one slab
// stay one contiguous run) and walks the slabs ONCE, in a wave-uniform loop. Per field and pixel it
// carries the last reliable slab and its code. At a reliable slab t it stores slab t; where a gap
// closes there (the pixel's previous slab was not reliable) it goes back and stores the slabs of the
// gap -- interpolated, held in front of the first reliable slab, fallback or unfilled beyond max_gap.
// One more, virtual, slab behind the last closes the trailing gaps the same way. Every output element
// is written exactly once, no input byte is read twice; no workspace, no atomics, no second pass.
//
// Cost of the common case: the reliability of the 4 pixels of a dword is worked out on the dword (the
// fill codes >= 249 by carry-free byte arithmetic, the QC table as 256 bytes of LDS), the state of a
// lane whose pixels are all reliable and were so one slab earlier is one register per field (`base`),
// and its store is one vector store. Gaps are closed by ONE loop per field over the elements of the
// gaps that end at this slab (the pixels are the set bits of a mask, a pixel's registers are picked by
// a chain of selects: no dynamically indexed array, no scratch); the uint8 interpolation steps
// quotient and remainder from slab to slab instead of dividing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mod16 {

constexpr int kGapMaxFields = 3;
constexpr int kGapMaxSlabs = 4096;
constexpr int kGapFill = 249;        // codes from here on are fill values (MOD15A2H; include/mod16_hip.h)
enum { kGapWideIn = 1, kGapWideOut = 2, kGapWideSrc = 4 };   // GapArgs::wide: rows that allow vector access
enum { kGapObserved = 0, kGapInterpolated = 1, kGapHeld = 2, kGapFallback = 3, kGapUnfilled = 4 };

struct GapArgs {
    const uint8_t* field[kGapMaxFields];     // [S][in_pitch]
    const uint8_t* qc;                       // [S][qc_pitch] or NULL
    const uint8_t* good;                     // 256 bytes on the device, or NULL: good_bits
    const uint8_t* fallback[kGapMaxFields];  // [n] or NULL
    void* out[kGapMaxFields];                // [S][out_pitch] of OUT
    uint8_t* source;                         // [NF][S][src_pitch] or NULL
    int64_t n, in_pitch, qc_pitch, out_pitch, src_pitch;
    double scale[kGapMaxFields];
    uint32_t good_bits[8];                   // the table as 256 bits (bit q of word q / 32)
    int slabs;
    int max_gap;                             // "none" arrives as kGapMaxSlabs + 1
    int wide;                                // kGapWide*: pointer and pitch are multiples of the vector size
};

template <typename OUT> struct GapPx;
template <> struct GapPx<uint8_t> { static constexpr int v = 16; };
template <> struct GapPx<float> { static constexpr int v = 8; };
template <> struct GapPx<double> { static constexpr int v = 4; };

// one rounding per value: integers for uint8 (round half up), one float64 division and one
// multiplication for the floats (no contraction possible between the two), then the cast
template <typename OUT> __device__ __forceinline__ OUT gap_encode(int num, int den, double scale) {
    const double q = den == 1 ? (double)num : (double)num / (double)den;
    return (OUT)(q * scale);
}
template <> __device__ __forceinline__ uint8_t gap_encode<uint8_t>(int num, int den, double) {
    return (uint8_t)((2u * (unsigned)num + (unsigned)den) / (2u * (unsigned)den));
}
template <typename OUT> __device__ __forceinline__ OUT gap_missing() { return (OUT)__builtin_nan(""); }
template <> __device__ __forceinline__ uint8_t gap_missing<uint8_t>() { return 255; }

// PX bytes of a row as dwords: one vector load, or byte loads of the first nv
template <int W> __device__ __forceinline__ void gap_load(const uint8_t* p, bool wide, int nv, uint32_t (&x)[W]) {
    if (wide) {
        if constexpr (W == 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else if constexpr (W == 2) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            x[0] = v.x; x[1] = v.y;
        } else {
            x[0] = *reinterpret_cast<const uint32_t*>(p);
        }
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) x[w] = 0;
#pragma unroll
        for (int k = 0; k < 4 * W; ++k)
            if (k < nv) x[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
    }
}

// the codes of a lane's PX pixels (all observed) as one run of vector stores
template <int W> __device__ __forceinline__ void gap_store_wide(uint8_t* p, const uint32_t (&x)[W], double) {
    if constexpr (W == 4) *reinterpret_cast<uint4*>(p) = make_uint4(x[0], x[1], x[2], x[3]);
    else if constexpr (W == 2) *reinterpret_cast<uint2*>(p) = make_uint2(x[0], x[1]);
    else *reinterpret_cast<uint32_t*>(p) = x[0];
}
template <int W> __device__ __forceinline__ void gap_store_wide(float* p, const uint32_t (&x)[W], double scale) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        float4 v;
        v.x = gap_encode<float>((int)(x[w] & 255u), 1, scale);
        v.y = gap_encode<float>((int)((x[w] >> 8) & 255u), 1, scale);
        v.z = gap_encode<float>((int)((x[w] >> 16) & 255u), 1, scale);
        v.w = gap_encode<float>((int)(x[w] >> 24), 1, scale);
        reinterpret_cast<float4*>(p)[w] = v;
    }
}
template <int W> __device__ __forceinline__ void gap_store_wide(double* p, const uint32_t (&x)[W], double scale) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        double2 lo, hi;
        lo.x = gap_encode<double>((int)(x[w] & 255u), 1, scale);
        lo.y = gap_encode<double>((int)((x[w] >> 8) & 255u), 1, scale);
        hi.x = gap_encode<double>((int)((x[w] >> 16) & 255u), 1, scale);
        hi.y = gap_encode<double>((int)(x[w] >> 24), 1, scale);
        reinterpret_cast<double2*>(p)[2 * w] = lo;
        reinterpret_cast<double2*>(p)[2 * w + 1] = hi;
    }
}

// 0x80 in every byte of x that holds a fill code (>= 249 = 0x80 + 121): the low seven bits plus 7
// carry into bit 7, never into the next byte
__device__ __forceinline__ uint32_t gap_fill_flags(uint32_t x) {
    return x & ((x & 0x7F7F7F7Fu) + 0x07070707u) & 0x80808080u;
}
// the four 0x80 flags of a dword as bits 0..3 (the products' other terms land below bit 24, one bit each)
__device__ __forceinline__ uint32_t gap_flag_bits(uint32_t r) {
    return (((r >> 7) & 0x01010101u) * 0x01020408u) >> 24;
}

template <typename OUT, int NF>
__global__ __launch_bounds__(kBlock) void gapfill_kernel(GapArgs a) {
    constexpr int PX = GapPx<OUT>::v, W = PX / 4;
    constexpr uint32_t kAll = (1u << PX) - 1u;
    // the QC table: 0x80 where the byte is good
    __shared__ uint32_t tab32[64];
    uint8_t* tab = reinterpret_cast<uint8_t*>(tab32);
    {
        const int q = threadIdx.x;
        bool g;
        if (a.good) {
            g = a.good[q] != 0;
        } else {
            uint32_t word = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w)
                if ((q >> 5) == w) word = a.good_bits[w];
            g = (word >> (q & 31)) & 1u;
        }
        tab[q] = g ? 0x80 : 0;
    }
    __syncthreads();
    const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * PX;
    if (p0 >= a.n) return;
    const int nv = a.n - p0 < PX ? (int)(a.n - p0) : PX;
    const uint32_t valid = kAll >> (PX - nv);
    const bool win = nv == PX && (a.wide & kGapWideIn);
    const bool wout = nv == PX && (a.wide & kGapWideOut);
    const bool wsrc = nv == PX && (a.wide & kGapWideSrc);
    const int S = a.slabs, mg = a.max_gap;

    int iv[NF][PX];            // last reliable slab of a pixel, where it is behind base[f]
    int base[NF];              // ... and a slab at which ALL pixels of the lane were reliable
    uint32_t code[NF][W];      // the code at that slab
    uint32_t open[NF];         // pixels whose previous slab was not reliable
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        base[f] = -1;
        open[f] = 0;
#pragma unroll
        for (int k = 0; k < PX; ++k) iv[f][k] = -1;
#pragma unroll
        for (int w = 0; w < W; ++w) code[f][w] = 0;
    }

    for (int t = 0; t <= S; ++t) {           // t = S: the virtual slab that closes the trailing gaps
        uint32_t x[NF][W], gm[W];
#pragma unroll
        for (int w = 0; w < W; ++w) gm[w] = 0x80808080u;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int w = 0; w < W; ++w) x[f][w] = 0;
        if (t < S) {
#pragma unroll
            for (int f = 0; f < NF; ++f) gap_load<W>(a.field[f] + (int64_t)t * a.in_pitch + p0, win, nv, x[f]);
            if (a.qc) {
                uint32_t q[W];
                gap_load<W>(a.qc + (int64_t)t * a.qc_pitch + p0, win, nv, q);
#pragma unroll
                for (int w = 0; w < W; ++w)
                    gm[w] = (uint32_t)tab[q[w] & 255u] | (uint32_t)tab[(q[w] >> 8) & 255u] << 8 |
                            (uint32_t)tab[(q[w] >> 16) & 255u] << 16 | (uint32_t)tab[q[w] >> 24] << 24;
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            OUT* const orow = static_cast<OUT*>(a.out[f]) + (int64_t)t * a.out_pitch + p0;
            uint8_t* const srow = a.source ? a.source + ((int64_t)f * S + t) * a.src_pitch + p0 : nullptr;
            uint32_t rel[W], relbits = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                rel[w] = gm[w] & ~gap_fill_flags(x[f][w]);
                relbits |= gap_flag_bits(rel[w]) << (4 * w);
            }
            relbits = t < S ? relbits & valid : valid;

            // close the gaps that end here: slabs i + 1 .. t - 1 of every pixel of `pend`. ONE loop over
            // the elements of all these gaps (a trip emits one element, and takes the next pixel first where the
            // last one's gap is done), so a lane's trips are its own elements, not the longest gap times the most gaps
            uint32_t pend = relbits & open[f];
            const bool right = t < S;
            int s = t, i = 0, av = 0, bv = 0, fb = 255, mode = 3;
            [[maybe_unused]] int q = 0, r = 0, stepq = 0, stepr = 0, d2 = 2;
            OUT* o = nullptr;
            uint8_t* so = nullptr;
            while (true) {
                if (s >= t) {
                    if (!pend) break;
                    const int k = __ffs(pend) - 1;
                    pend &= pend - 1;
                    uint32_t cw = 0, xw = 0;
                    i = -1;
#pragma unroll
                    for (int kk = 0; kk < PX; ++kk)
                        if (k == kk) i = iv[f][kk];
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if ((k >> 2) == w) { cw = code[f][w]; xw = x[f][w]; }
                    i = i > base[f] ? i : base[f];
                    av = (cw >> ((k & 3) * 8)) & 255u;
                    bv = (xw >> ((k & 3) * 8)) & 255u;
                    fb = a.fallback[f] ? (int)a.fallback[f][p0 + k] : 255;
                    // 0 interpolated, 1 held from the left, 2 held from the right, 3 neither
                    mode = i >= 0 ? (right ? (t - i - 1 <= mg ? 0 : 3) : 1) : (right ? 2 : 3);
                    s = i + 1;
                    o = static_cast<OUT*>(a.out[f]) + (int64_t)s * a.out_pitch + p0 + k;
                    if (a.source) so = a.source + ((int64_t)f * S + s) * a.src_pitch + p0 + k;
                    if constexpr (sizeof(OUT) == 1) {
                        // (2 num_s + den) / (2 den) for s = i + 1 ...: from s to s + 1 the dividend grows by
                        // 2 (b - a); quotient and remainder are stepped, the step's own quotient comes
                        // from a float estimate put right by its remainder (|b - a| <= 248: exact)
                        const int den = t - i, diff = 2 * (bv - av);
                        d2 = 2 * den;
                        stepq = (int)floorf((float)diff * __frcp_rn((float)d2));
                        stepr = diff - stepq * d2;
                        if (stepr < 0) { stepr += d2; --stepq; }
                        if (stepr >= d2) { stepr -= d2; ++stepq; }
                        q = av;
                        r = den;
                    }
                }                   // (a gap holds at least one slab: s < t here)
                int num = 0, den = 1, src = kGapFallback;
                if constexpr (sizeof(OUT) == 1) {
                    r += stepr;
                    q += stepq;
                    if (r >= d2) { r -= d2; ++q; }
                }
                if (mode == 0) {
                    src = kGapInterpolated;
                    if constexpr (sizeof(OUT) == 1) {
                        num = q;
                    } else {
                        num = av * (t - s) + bv * (s - i);
                        den = t - i;
                    }
                } else if (mode == 1 ? s - i <= mg : (mode == 2 && t - s <= mg)) {
                    num = mode == 1 ? av : bv;
                    src = kGapHeld;
                } else if (fb < kGapFill) {
                    num = fb;
                } else {
                    src = kGapUnfilled;
                }
                *o = src == kGapUnfilled ? gap_missing<OUT>() : gap_encode<OUT>(num, den, a.scale[f]);
                o += a.out_pitch;
                if (a.source) { *so = (uint8_t)src; so += a.src_pitch; }
                ++s;
            }
            if (t == S) continue;

            // slab t itself, where it is reliable
            if (relbits == kAll && wout) {
                gap_store_wide<W>(orow, x[f], a.scale[f]);
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if ((relbits >> k) & 1u) orow[k] = gap_encode<OUT>((int)((x[f][k >> 2] >> ((k & 3) * 8)) & 255u), 1, a.scale[f]);
            }
            if (srow) {
                if (relbits == kAll && wsrc) {
                    uint32_t zero[W];
#pragma unroll
                    for (int w = 0; w < W; ++w) zero[w] = 0;
                    gap_store_wide<W>(srow, zero, 0.0);
                } else {
#pragma unroll
                    for (int k = 0; k < PX; ++k)
                        if ((relbits >> k) & 1u) srow[k] = kGapObserved;
                }
            }
            // the state behind slab t
            if (relbits == kAll) {
                base[f] = t;
#pragma unroll
                for (int w = 0; w < W; ++w) code[f][w] = x[f][w];
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if ((relbits >> k) & 1u) iv[f][k] = t;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t m = (rel[w] >> 7) * 255u;
                    code[f][w] = (code[f][w] & ~m) | (x[f][w] & m);
                }
            }
            open[f] = valid & ~relbits;
        }
    }
}

}  // namespace mod16
