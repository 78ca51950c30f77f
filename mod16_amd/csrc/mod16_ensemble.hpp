// Ensemble forward run (gfx950): MOD16.evapotranspiration for D parameter tables over one raster,
// reduced per pixel to the mean and the spread over the members -- mod16_et_ensemble_*.
//
// A pixel's drivers and class are read ONCE; what the FAST pixel function (et_pixel_fast /
// period_fast, mod16_physics.hpp) computes from the drivers alone -- the saturation exponential,
// three reciprocals, t^-1.75, the air density, the slope of the curve, log(rh), the latent heat,
// both outcomes of the soil-heat-flux condition -- is prepared once per pixel (EnsPixel, 2 x
// EnsPeriod) and stays in registers; the member loop evaluates the rest (ens_period_eval: the
// operations of period_fast that touch a parameter, in its order, so a member's value has the bits
// et_pixel_fast gives for that table). The members' derived tables ([MOD16_LUT_ROWS][kLutCols]
// float64 each, the layout of the single-table kernels) pass through LDS in chunks of kEnsChunk.
//
// Accumulation: sequential in member order, float64, one pass, shifted by member 0 (d = x_m - x_0,
// then sum d and sum d^2): identical members give d = 0 exactly, so std = 0 and mean = x_0 + 0. A
// NaN member value makes d NaN and with it the mean and both spreads of that period. No atomics, no
// D x n intermediate: two launches give the same bits.
//
// Domain guard: fast_out_of_domain(x) depends on the drivers only; a flagged pixel has ALL its
// members computed by et_pixel_exact<double> in a second kernel behind this one (ens_redo_kernel,
// tables from global memory; the pattern of et_stream_redo_kernel / static_obj_redo_kernel). Inline,
// behind the member loop, the reference-order branch (232 vector registers on its own) met the fast
// path's constants, which the compiler keeps in vector registers across the batch loop: 256
// registers and 6 spilled. The flag travels in the output itself: the fast kernel writes NO result
// for a flagged pixel but a NaN with a payload of its own (EnsMark) into std_total, and the second
// kernel computes every pixel whose std_total carries it -- 8 bytes (4) per pixel read again, no
// workspace, nothing shared between launches on different streams. A pixel whose own result had that
// payload by coincidence would merely be computed in the reference's order (its NaN stays a NaN).
// MOD16_MATH_EXACT sends every pixel through et_pixel_exact (ens_kernel<T, false>). float32 storage:
// float64 arithmetic and accumulation, one rounding on store, in both instances.
#pragma once
#include "mod16_kernels.hpp"

namespace mod16 {

constexpr int kEnsChunk = 16;                               // members per LDS stage: 32 KiB
constexpr int kEnsTable = MOD16_LUT_ROWS * kLutCols;        // doubles of one member's derived table
constexpr int64_t kEnsMaxMembers = 65536;
constexpr int kEnsOut = 5;                                  // mean day, mean night, std day, std night, std total

template <typename T> struct EnsArgs {
    const T* drv[14];
    const uint8_t* cls;
    const double* tables;      // device [members][MOD16_LUT_ROWS][kLutCols]
    const double* tab;         // exp / log tables of FastMath<double>
    T* out[kEnsOut];
    int64_t n;
    int members;
    unsigned* status;
    uint32_t dense_drv;        // bit k set: driver k is a dense array, else a broadcast scalar
};

// What one period (day / night) of a pixel contributes to every member: period_fast's values that
// depend on the drivers only, and its products of them.
struct EnsPeriod {
    double vpd, logrh, fwet, omw, s, slhv, inv_rcorr, g_rr;
    double rf;          // (rho Cp vpd) fpar
    double rcfv_omf;    // (rho Cp vpd) (1 - fpar)
    double sx_can;      // s (fpar A)            wet canopy
    double sx_tr;       // s max(fpar A, 0)      transpiration, :1251
    double s_rs[2];     // s x radiation received by the soil without / with soil heat flux
    bool dry;           // rh < 0.7
};
struct EnsPixel {
    EnsPeriod d, n;
    double k_p, lai, tm, t_ann;
    bool base_cond, lai_pos, lai_tiny;
};

__device__ __forceinline__ EnsPeriod ens_period_prep(const PixelIn<double>& x, double p_rel, double p_mbar_k,
                                                     double omf, const double* tb, double t, double vpd,
                                                     double rad_net, const double (&rs)[2]) {
#pragma clang fp contract(off)
    typedef FastMath<double> M;
    EnsPeriod c;
    c.vpd = vpd;
    // -- humidity, :646-673 and :763-764 (period_fast, the same operations)
    double tc = t - K<double>::t0;
    double d_es = tc + 237.3;
    double ta = tc + 239.0;
    double dd = d_es * ta;
    double r_both = M::rcp(dd);
    double r_es = r_both * ta, rta = r_both * d_es;
    double e_es = M::exp_tab5s((17.27 * tc) * r_es, tb);
    double esat = (1e3 * 0.6108) * e_es;
    double avp = esat - vpd;
    double resat = M::rcp(esat);
    double rh = avp * resat;
    rh = M::fma_unit(__builtin_fma(-rh, esat, avp), resat, rh);    // :670-673, as period_fast has it
    rh = __builtin_fma(avp, 0.0, rh);
    double rh2 = rh * rh;
    c.dry = rh < 0.7;                                              // :764 (NaN compares false)
    c.fwet = c.dry ? 0.0 : rh2 * rh2;
    c.omw = 1.0 - c.fwet;
    // -- slope of the SVP curve, latent heat
    c.s = ((17.38 * 239.0) * esat) * (rta * rta);
    double lhv = M::fma_kk(tc, -0.002361e6, 2.501e6);
    c.slhv = c.s * lhv;
    // -- 1 / r_corr, 1 / T
    double rt;
    c.inv_rcorr = p_rel * M::pow_m1p75_rcp(t, rt);
    // -- air density and radiative conductance
    double nn = __builtin_fma(-rh, M::fma_kk(tc, 0.252 * 1013.0, -2.0582 * 1013.0), p_mbar_k);
    double rho_cp = nn * rt;
    double t2 = t * t;
    c.g_rr = (K<double>::sigma4 * (t2 * t2)) * M::rcp(nn);
    double rcfv = rho_cp * vpd;
    c.rf = rcfv * x.fpar;
    c.rcfv_omf = rcfv * omf;
    c.sx_can = c.s * (x.fpar * rad_net);
    double rad_c = x.fpar * rad_net;
    rad_c = (rad_c < 0.0) ? 0.0 : rad_c;                           // :1251
    c.sx_tr = c.s * rad_c;
    c.s_rs[0] = c.s * rs[0];
    c.s_rs[1] = c.s * rs[1];
    // -- rh ** (vpd / beta), :861: the logarithm here, the exponential per member
    c.logrh = M::log_tab1(rh, tb);
    return c;
}

__device__ __forceinline__ EnsPixel ens_pixel_prep(const PixelIn<double>& x, const double* tb) {
#pragma clang fp contract(off)
    EnsPixel c;
    const double oma = 1.0 - x.alb, omf = 1.0 - x.fpar;
    const double a_d = __builtin_fma(x.sw_d, oma, x.lw_d), a_n = x.lw_n;
    // soil heat flux, :963-1119: the condition's parameter-dependent part (t_ann >= 273.15 +
    // tmin_close) is applied per member, both outcomes are prepared (as StaticPixel::rs_d[2])
    c.base_cond = (x.t_ann < 273.15 + 25.0) & ((x.t_d - x.t_n) >= 5.0);
    c.t_ann = x.t_ann;
    const double cap_d = 0.39 * a_d, cap_n = 0.39 * a_n;
    double rs_d[2], rs_n[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double g_d = k ? __builtin_fma(4.73, x.t_d - 273.15, -20.87) : 0.0;
        g_d = (__builtin_fabs(g_d) > __builtin_fabs(cap_d)) ? cap_d : g_d;
        double g_n = k ? __builtin_fma(4.73, x.t_n - 273.15, -20.87) : 0.0;
        g_n = (__builtin_fabs(g_n) > __builtin_fabs(cap_n)) ? cap_n : g_n;
        g_d = ((a_d - g_d < 0.0) & (a_d > 0.0)) ? a_d : g_d;
        g_n = ((a_d > 0.0) & ((a_n - g_n) < (-0.5 * a_d))) ? __builtin_fma(0.5, a_d, a_n) : g_n;
        rs_d[k] = omf * (a_d - g_d);
        rs_n[k] = omf * (a_n - g_n);
    }
    const double p_rel = x.pa * 0.2050207779207528;                // 293.15^1.75 / 101300
    c.k_p = x.pa * (1013.0 / 0.622);
    const double p_mbar_k = x.pa * (1013.0 * 0.348444 / 100.0);
    c.lai = x.lai;
    c.lai_tiny = x.lai <= 1e-7;
    c.lai_pos = x.lai > 0.0;
    c.tm = x.tmin - 273.15;
    c.d = ens_period_prep(x, p_rel, p_mbar_k, omf, tb, x.t_d, x.vpd_d, a_d, rs_d);
    const double rn_n = __builtin_fma(x.sw_n, oma, x.lw_n);
    c.n = ens_period_prep(x, p_rel, p_mbar_k, omf, tb, x.t_n, x.vpd_n, rn_n, rs_n);
    return c;
}

// One member's parameters for one pixel: its class's column of the member's table, and the terms
// et_pixel_fast derives from them per pixel.
struct EnsMember {
    double vpd_open, inv_dvpd, rbl_min, drbl, inv_beta, gl_sh, g_cut, csl_mt, glsh_lai, glwv_lai;
    bool cond;
};
__device__ __forceinline__ EnsMember ens_member(const EnsPixel& px, const double* l) {
#pragma clang fp contract(off)
    EnsMember m;
    const double tmin_close = l[0 * kLutCols];
    m.vpd_open = l[2 * kLutCols];
    m.gl_sh = l[4 * kLutCols];
    const double gl_wv = l[5 * kLutCols];
    m.g_cut = l[6 * kLutCols];
    const double csl = l[7 * kLutCols];
    m.rbl_min = l[8 * kLutCols];
    const double rbl_max = l[9 * kLutCols];
    const double inv_dtmin = l[11 * kLutCols];
    m.inv_dvpd = l[12 * kLutCols];
    m.inv_beta = l[14 * kLutCols];
    m.cond = px.base_cond & (px.t_ann >= (273.15 + tmin_close));   // :1103-1107
    m.glsh_lai = m.gl_sh * px.lai;
    m.glwv_lai = gl_wv * px.lai;
    m.drbl = rbl_max - m.rbl_min;
    typedef FastMath<double> M;
    m.csl_mt = csl * M::nan_from(M::mul_unit(px.tm - tmin_close, inv_dtmin), px.tm);   // as et_pixel_fast has it
    return m;
}

// (canopy + soil) + transpiration of one period for one member: period_fast from `vramp` on
template <bool DAY>
__device__ __forceinline__ double ens_period_eval(const EnsPixel& px, const EnsPeriod& c, const EnsMember& m,
                                                  const double* tb) {
#pragma clang fp contract(off)
    typedef FastMath<double> M;
    const double tiny = 1e-7;
    const double vramp = M::mul_unit(c.vpd - m.vpd_open, m.inv_dvpd);
    double canopy, soil, trans;
    {   // wet canopy, :866-961
        const double g_e = m.glwv_lai * c.fwet;
        const double g_a = __builtin_fma(m.glsh_lai, c.fwet, c.g_rr);
        const double numer = c.fwet * __builtin_fma(c.rf, g_a, c.sx_can);
        const double den = __builtin_fma(c.slhv, g_e, px.k_p * g_a);
        const double evap = (numer * g_e) * M::rcp_quotient(den);
        canopy = ((numer < 0.0) | c.dry | px.lai_tiny) ? 0.0 : evap;
    }
    {   // bare soil, :449-544 and :795-864
        const double r0 = __builtin_fma(vramp, m.drbl, m.rbl_min);
        const double r_tot = r0 * c.inv_rcorr;
        const double w = __builtin_fma(r_tot, c.g_rr, 1.0);
        const double s_rs = m.cond ? c.s_rs[1] : c.s_rs[0];
        const double num = __builtin_fma(s_rs, r_tot, c.rcfv_omf * w);
        const double den = r_tot * __builtin_fma(px.k_p, w, c.slhv);
        const double q = num * M::rcp_quotient(den);
        // pow01_tab1(rh, vpd / beta) with its logarithm taken once per period
        const double yc = M::vmin_k(c.vpd * m.inv_beta, 1e300);
        const double pw = M::exp_tab4s(M::vmax_k(yc * c.logrh, -746.0), tb);
        const double e = q * __builtin_fma(c.omw, pw, c.fwet);
        soil = (q < 0.0) ? 0.0 : e;
    }
    {   // transpiration, :1152-1258
        double g_s = 0.0;
        if (DAY) g_s = (m.csl_mt * (1.0 - vramp)) * c.inv_rcorr;
        const double gsc = __builtin_fma(m.g_cut, c.inv_rcorr, g_s);
        const double g_bl = m.glsh_lai * c.omw;
        const double p1 = g_bl * gsc;
        const double s1 = __builtin_fma(m.glsh_lai, c.omw, gsc);
        const bool open = px.lai_pos & (c.omw > 0.0);
        const bool shut = !open | (p1 <= tiny * s1);
        const double g_d = m.gl_sh + c.g_rr;
        const double num = (c.omw * __builtin_fma(c.rf, g_d, c.sx_tr)) * p1;
        const double den = __builtin_fma(c.slhv, p1, px.k_p * __builtin_fma(g_d, s1, p1));
        const double tr = num * M::rcp_quotient(den);
        trans = shut ? 0.0 : tr;
    }
    return (canopy + soil) + trans;                                // mod16/__init__.py:792
}

// The running sums of one pixel, shifted by member 0.
struct EnsAcc {
    double d0, n0, sd, sd2, sn, sn2, st, st2;
    __device__ __forceinline__ void reset() { d0 = n0 = sd = sd2 = sn = sn2 = st = st2 = 0.0; }
    __device__ __forceinline__ void add(bool first, double day, double night) {
#pragma clang fp contract(off)
        d0 = first ? day : d0;
        n0 = first ? night : n0;
        const double dd = day - d0, dn = night - n0, dt = (day + night) - (d0 + n0);
        sd += dd;
        sd2 = __builtin_fma(dd, dd, sd2);
        sn += dn;
        sn2 = __builtin_fma(dn, dn, sn2);
        st += dt;
        st2 = __builtin_fma(dt, dt, st2);
    }
    // np.std, ddof = 0: sqrt((sum d^2 - (sum d)^2 / D) / D); a NaN stays (it compares false)
    static __device__ __forceinline__ double spread(double s, double s2, double D) {
#pragma clang fp contract(off)
        double var = (s2 - (s * s) / D) / D;
        var = (var < 0.0) ? 0.0 : var;
        return __builtin_sqrt(var);
    }
    template <typename T> __device__ __forceinline__ void store(const EnsArgs<T>& a, int64_t i) const {
#pragma clang fp contract(off)
        const double D = (double)a.members;
        a.out[0][i] = (T)(d0 + sd / D);
        a.out[1][i] = (T)(n0 + sn / D);
        a.out[2][i] = (T)spread(sd, sd2, D);
        a.out[3][i] = (T)spread(sn, sn2, D);
        a.out[4][i] = (T)spread(st, st2, D);
    }
};

// Every member of one pixel in the reference's operation order, tables from global memory.
__device__ __forceinline__ void ens_exact_members(const PixelIn<double>& x, unsigned c, const double* __restrict__ tables,
                                                  int members, EnsAcc& acc) {
    acc.reset();
#pragma nounroll
    for (int m = 0; m < members; ++m) {
        const double* l = tables + (int64_t)m * kEnsTable + c;
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
        const PixelOut<double> o = et_pixel_exact<double, false, true>(x, p);
        acc.add(m == 0, (o.canopy_d + o.soil_d) + o.trans_d, (o.canopy_n + o.soil_n) + o.trans_n);
    }
}

// What the fast kernel leaves in std_total of a pixel outside its domain (a quiet NaN, payload "e5b1e")
template <typename T> struct EnsMark;
template <> struct EnsMark<double> {
    static constexpr unsigned long long bits = 0x7ff80000000e5b1eull;
    static __device__ __forceinline__ double value() { return __longlong_as_double((long long)bits); }
    static __device__ __forceinline__ bool is(double v) { return (unsigned long long)__double_as_longlong(v) == bits; }
};
template <> struct EnsMark<float> {
    static constexpr unsigned bits = 0x7fce5b1eu;
    static __device__ __forceinline__ float value() { return __uint_as_float(bits); }
    static __device__ __forceinline__ bool is(float v) { return __float_as_uint(v) == bits; }
};

// One pixel per thread, 256-thread blocks over batches of 256 pixels; the batch loop and the
// member loop are block-uniform (the table stage sits between two barriers), the threads past the
// raster's end compute on its last pixel and store nothing.
template <typename T, bool FAST>
__global__ void __launch_bounds__(kBlock, 2) ens_kernel(const EnsArgs<T> a) {
    constexpr int kTab = FAST ? FastMath<double>::kTabDoubles : 1;
    constexpr int kLds = FAST ? kEnsChunk * kEnsTable : 1;
    __shared__ __attribute__((aligned(16))) double lut[kLds];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    const int D = a.members;
    const bool resident = D <= kEnsChunk;         // the whole ensemble fits one stage: staged once
    auto stage = [&](int m0, int count) {
        const double* src = a.tables + (int64_t)m0 * kEnsTable;
        for (int i = threadIdx.x; i < count * kEnsTable; i += kBlock) lut[i] = src[i];
    };
    if constexpr (FAST) {
        ignore_signalling_nans();                  // the domain guard's NaN-ignoring chain
        for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.tab[i];
        if (resident) stage(0, D);
        __syncthreads();
    }
    const int64_t nbatch = (a.n + kBlock - 1) / kBlock;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i0 = b * kBlock + threadIdx.x;
        const bool live = i0 < a.n;
        const int64_t i = live ? i0 : a.n - 1;
        auto drv = [&](int k) -> double { return (double)a.drv[k][((a.dense_drv >> k) & 1u) ? i : 0]; };
        auto pixel = [&]() {
            return PixelIn<double>{drv(0), drv(1), drv(2), drv(3), drv(4), drv(5), drv(6),
                                   drv(7), drv(8), drv(9), drv(10), drv(11), drv(12), drv(13)};
        };
        unsigned c = a.cls[i];
        if (c >= 13u) {   // numpy would raise IndexError: flag it, give NaN
            atomicOr(a.status, kStatusClassRange);
            c = 13u;
        }
        EnsAcc acc;
        if constexpr (FAST) {
            bool bad;
            EnsPixel px;
            {
                const PixelIn<double> x = pixel();
                bad = fast_out_of_domain(x);
                px = ens_pixel_prep(x, tab);
            }
            acc.reset();
#pragma nounroll
            for (int m0 = 0; m0 < D; m0 += kEnsChunk) {
                const int mc = (D - m0 < kEnsChunk) ? D - m0 : kEnsChunk;
                if (!resident) {
                    __syncthreads();               // every thread is done with the previous chunk
                    stage(m0, mc);
                    __syncthreads();
                }
#pragma nounroll
                for (int k = 0; k < mc; ++k) {
                    const EnsMember m = ens_member(px, lut + k * kEnsTable + c);
                    const double day = ens_period_eval<true>(px, px.d, m, tab);
                    const double night = ens_period_eval<false>(px, px.n, m, tab);
                    acc.add((m0 | k) == 0, day, night);
                }
            }
            // a pixel outside the domain of the strength-reduced arithmetic leaves the mark for
            // ens_redo_kernel, which runs behind this kernel (mod16_physics.hpp, "domain guard")
            if (live) {
                if (bad) a.out[kEnsOut - 1][i] = EnsMark<T>::value();
                else acc.store(a, i);
            }
        } else {
            ens_exact_members(pixel(), c, a.tables, D, acc);
            if (live) acc.store(a, i);
        }
    }
}

// Behind ens_kernel<T, true>: the marked pixels, every member in the reference's operation order.
template <typename T>
__global__ void __launch_bounds__(kBlock, 1) ens_redo_kernel(const EnsArgs<T> a) {
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += step) {
        if (!EnsMark<T>::is(a.out[kEnsOut - 1][i])) continue;
        auto drv = [&](int k) -> double { return (double)a.drv[k][((a.dense_drv >> k) & 1u) ? i : 0]; };
        const PixelIn<double> x = {drv(0), drv(1), drv(2), drv(3), drv(4), drv(5), drv(6),
                                   drv(7), drv(8), drv(9), drv(10), drv(11), drv(12), drv(13)};
        unsigned c = a.cls[i];
        c = c >= 13u ? 13u : c;        // (ens_kernel has flagged it)
        EnsAcc acc;
        ens_exact_members(x, c, a.tables, a.members, acc);
        acc.store(a, i);
    }
}

// ---------------------------------------------------------------------------------------------
// Per-member outputs and per-pixel quantiles (mod16_et_ensemble_members_*, _quantiles_*).
//
// ens_members_kernel is ens_kernel's body with another sink: instead of EnsAcc::add it stores day_m
// and night_m to [m * pitch + i] -- a sibling, not an instance of a shared template, so that
// ens_kernel keeps its code and its registers. O is the type of the member arrays: T for the public
// ones, double for the slab of the quantile run (float drivers, double slab). The domain guard keeps
// its shape: the fast kernel writes NO member of a flagged pixel but an EnsMark<O> into member 0's
// day value, ens_members_redo_kernel behind it computes all members of every marked pixel in the
// reference's order.
//
// ens_select_kernel orders a pixel's members and interpolates the quantiles
// (mod16_amd.calibration.ensemble_quantile is its definition). One pixel per lane, one wave per
// block; the pixel's column lives in LDS as doubles laid out [m][lane] (consecutive lanes on
// consecutive pixels: every global load is coalesced, every LDS access conflict-free), padded with
// +inf to the capacity CAP (a power of two, 16 ... 256: 8 ... 128 KiB, static). The order is a bitonic
// network -- data-independent, so the lanes of the wave stay together -- blocked through registers 16
// elements at a time: runs of 16 are sorted in registers straight from the slab, every later merge
// does its strides >= 16 in LDS and its strides 8, 4, 2, 1 on 16 registers. A lane touches its own
// column only: no barrier. The three series (day, night, day + night formed on load) use the same
// LDS one after the other. A NaN member is replaced by +inf on load and carried as a flag.

template <typename T, typename O> struct EnsMemArgs {
    const T* drv[14];
    const uint8_t* cls;
    const double* tables;
    const double* tab;
    O* day;                    // [members][pitch]
    O* night;
    int64_t pitch;
    int64_t n;
    int members;
    unsigned* status;
    uint32_t dense_drv;
};

template <typename T, typename O>
__device__ __forceinline__ void ens_exact_members_store(const PixelIn<double>& x, unsigned c,
                                                        const EnsMemArgs<T, O>& a, int64_t i, bool live) {
#pragma nounroll
    for (int m = 0; m < a.members; ++m) {
        const double* l = a.tables + (int64_t)m * kEnsTable + c;
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
        const PixelOut<double> o = et_pixel_exact<double, false, true>(x, p);
        if (live) {
            a.day[(int64_t)m * a.pitch + i] = (O)((o.canopy_d + o.soil_d) + o.trans_d);
            a.night[(int64_t)m * a.pitch + i] = (O)((o.canopy_n + o.soil_n) + o.trans_n);
        }
    }
}

template <typename T, typename O, bool FAST>
__global__ void __launch_bounds__(kBlock, 2) ens_members_kernel(const EnsMemArgs<T, O> a) {
    constexpr int kTab = FAST ? FastMath<double>::kTabDoubles : 1;
    constexpr int kLds = FAST ? kEnsChunk * kEnsTable : 1;
    __shared__ __attribute__((aligned(16))) double lut[kLds];
    __shared__ __attribute__((aligned(16))) double tab[kTab];
    const int D = a.members;
    const bool resident = D <= kEnsChunk;
    auto stage = [&](int m0, int count) {
        const double* src = a.tables + (int64_t)m0 * kEnsTable;
        for (int i = threadIdx.x; i < count * kEnsTable; i += kBlock) lut[i] = src[i];
    };
    if constexpr (FAST) {
        ignore_signalling_nans();
        for (int i = threadIdx.x; i < kTab; i += kBlock) tab[i] = a.tab[i];
        if (resident) stage(0, D);
        __syncthreads();
    }
    const int64_t nbatch = (a.n + kBlock - 1) / kBlock;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t i0 = b * kBlock + threadIdx.x;
        const bool live = i0 < a.n;
        const int64_t i = live ? i0 : a.n - 1;
        auto drv = [&](int k) -> double { return (double)a.drv[k][((a.dense_drv >> k) & 1u) ? i : 0]; };
        auto pixel = [&]() {
            return PixelIn<double>{drv(0), drv(1), drv(2), drv(3), drv(4), drv(5), drv(6),
                                   drv(7), drv(8), drv(9), drv(10), drv(11), drv(12), drv(13)};
        };
        unsigned c = a.cls[i];
        if (c >= 13u) {
            atomicOr(a.status, kStatusClassRange);
            c = 13u;
        }
        if constexpr (FAST) {
            bool keep;
            EnsPixel px;
            {
                const PixelIn<double> x = pixel();
                keep = live & !fast_out_of_domain(x);
                px = ens_pixel_prep(x, tab);
            }
            O* day = a.day + i;
            O* night = a.night + i;
#pragma nounroll
            for (int m0 = 0; m0 < D; m0 += kEnsChunk) {
                const int mc = (D - m0 < kEnsChunk) ? D - m0 : kEnsChunk;
                if (!resident) {
                    __syncthreads();
                    stage(m0, mc);
                    __syncthreads();
                }
#pragma nounroll
                for (int k = 0; k < mc; ++k) {
                    const EnsMember m = ens_member(px, lut + k * kEnsTable + c);
                    const double d = ens_period_eval<true>(px, px.d, m, tab);
                    const double g = ens_period_eval<false>(px, px.n, m, tab);
                    if (keep) {
                        *day = (O)d;
                        *night = (O)g;
                    }
                    day += a.pitch;
                    night += a.pitch;
                }
            }
            // outside the domain of the strength-reduced arithmetic: the mark for the kernel behind
            if (live & !keep) a.day[i] = EnsMark<O>::value();
        } else {
            ens_exact_members_store(pixel(), c, a, i, live);
        }
    }
}

// Behind ens_members_kernel<T, O, true>: every member of the marked pixels in the reference's order.
template <typename T, typename O>
__global__ void __launch_bounds__(kBlock, 1) ens_members_redo_kernel(const EnsMemArgs<T, O> a) {
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += step) {
        if (!EnsMark<O>::is(a.day[i])) continue;
        auto drv = [&](int k) -> double { return (double)a.drv[k][((a.dense_drv >> k) & 1u) ? i : 0]; };
        const PixelIn<double> x = {drv(0), drv(1), drv(2), drv(3), drv(4), drv(5), drv(6),
                                   drv(7), drv(8), drv(9), drv(10), drv(11), drv(12), drv(13)};
        unsigned c = a.cls[i];
        c = c >= 13u ? 13u : c;
        ens_exact_members_store(x, c, a, i, true);
    }
}

constexpr int kEnsMaxQuantiles = 8;
constexpr int kEnsSelMaxMembers = 256;     // the largest column the selection holds in LDS
constexpr int kEnsSelLanes = 64;           // one wave per block, one pixel per lane
constexpr int kEnsSelRun = 16;             // elements a lane orders in registers per LDS pass

template <typename T> struct EnsSelArgs {
    const double* day;         // the slab: [members][pitch]
    const double* night;
    int64_t pitch;
    int64_t n;                 // pixels of this chunk
    int members;
    int nq;
    int lo[kEnsMaxQuantiles];          // quantile_positions(q, members), computed on the host
    double frac[kEnsMaxQuantiles];
    T* out[3 * kEnsMaxQuantiles];      // series-major: day, night, total; nq each
};

__device__ __forceinline__ void ens_cmpx(double& a, double& b) {    // a <= b afterwards
    const bool sw = b < a;
    const double lo = sw ? b : a, hi = sw ? a : b;
    a = lo;
    b = hi;
}
// bitonic merge of 16 registers whose two halves ... are bitonic already: strides 8, 4, 2, 1
__device__ __forceinline__ void ens_merge16(double (&v)[kEnsSelRun]) {
#pragma unroll
    for (int j = kEnsSelRun / 2; j >= 1; j >>= 1)
#pragma unroll
        for (int i = 0; i < kEnsSelRun; ++i)
            if ((i & j) == 0) ens_cmpx(v[i], v[i | j]);
}
// ascending order of 16 registers: the bitonic network, directions resolved at compile time
__device__ __forceinline__ void ens_sort16(double (&v)[kEnsSelRun]) {
#pragma unroll
    for (int k = 2; k <= kEnsSelRun; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1)
#pragma unroll
            for (int i = 0; i < kEnsSelRun; ++i)
                if ((i & j) == 0) {
                    if ((i & k) == 0 || k == kEnsSelRun) ens_cmpx(v[i], v[i | j]);
                    else ens_cmpx(v[i | j], v[i]);
                }
}

template <typename T, int CAP>
__global__ void __launch_bounds__(kEnsSelLanes) ens_select_kernel(const EnsSelArgs<T> a) {
    static_assert(CAP >= kEnsSelRun && CAP <= kEnsSelMaxMembers && (CAP & (CAP - 1)) == 0, "capacity");
    constexpr int L = kEnsSelLanes, R = kEnsSelRun;
    __shared__ __attribute__((aligned(16))) double col[CAP * L];
    const int lane = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * L + lane;
    const bool live = i0 < a.n;
    const int64_t i = live ? i0 : a.n - 1;
    const int D = a.members;
    const double inf = __builtin_inf();
    double* mine = col + lane;
#pragma nounroll
    for (int series = 0; series < 3; ++series) {
        bool nan = false;
        // runs of 16 straight from the slab, ordered in registers; run r ascending for even r,
        // descending for odd r: pairs of runs are bitonic
#pragma nounroll
        for (int r = 0; r < CAP / R; ++r) {
            double v[R];
#pragma unroll
            for (int e = 0; e < R; ++e) {
                const int m = r * R + e;
                double x = inf;
                if (m < D) {
                    const int64_t at = (int64_t)m * a.pitch + i;
                    x = series == 0 ? a.day[at] : series == 1 ? a.night[at] : a.day[at] + a.night[at];
                }
                nan |= x != x;
                v[e] = (x != x) ? inf : x;
            }
            ens_sort16(v);
            const bool up = (r & 1) == 0 || CAP == R;
#pragma unroll
            for (int e = 0; e < R; ++e) mine[(r * R + (up ? e : R - 1 - e)) * L] = v[e];
        }
        // merges of 32, 64, ... CAP: strides >= 16 in LDS, the rest on registers
#pragma nounroll
        for (int k = 2 * R; k <= CAP; k <<= 1) {
#pragma nounroll
            for (int j = k >> 1; j >= R; j >>= 1) {
#pragma nounroll
                for (int p = 0; p < CAP / 2; ++p) {
                    const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));     // bit j clear
                    const int hi = lo | j;
                    const bool up = (lo & k) == 0 || k == CAP;
                    double x = mine[lo * L], y = mine[hi * L];
                    if (up) ens_cmpx(x, y);
                    else ens_cmpx(y, x);
                    mine[lo * L] = x;
                    mine[hi * L] = y;
                }
            }
#pragma nounroll
            for (int r = 0; r < CAP / R; ++r) {
                double v[R];
#pragma unroll
                for (int e = 0; e < R; ++e) v[e] = mine[(r * R + e) * L];
                ens_merge16(v);
                const bool up = ((r * R) & k) == 0 || k == CAP;
#pragma unroll
                for (int e = 0; e < R; ++e) mine[(r * R + (up ? e : R - 1 - e)) * L] = v[e];
            }
        }
        // the order statistics and their interpolation: ensemble_quantile, operation for operation
#pragma nounroll
        for (int q = 0; q < a.nq; ++q) {
#pragma clang fp contract(off)
            const int lo = a.lo[q];
            const int hi = (lo + 1 < D) ? lo + 1 : D - 1;
            const double frac = a.frac[q];
            const double x = mine[lo * L], y = mine[hi * L];
            const double t = frac * (y - x);
            double val = (frac == 0.0 || x == y) ? x : x + t;
            val = nan ? __builtin_nan("") : val;
            if (live) a.out[series * a.nq + q][i] = (T)val;
        }
    }
}

}  // namespace mod16
