// gfx950 kernels of the DE-MCMC-Z sampler (mod16_mcmc_*, capi/mcmc.hip; mod16_amd/calibration.py):
// the chains of a calibration of MOD16 parameters against a tower record, kept on the device. One
// lane per chain; a step is propose -> the resident problem's objective (capi/batch.hpp) -> accept,
// and K steps are captured as one graph. float64 only.
//
// This is the project's own restatement of PyMC's DEMetropolisZ (ter Braak & Vrugt 2008) as the
// reference uses it through mod17's StochasticSampler; neither is available to check against.
//
// Parameters. Free parameter i (0 <= i < d, in MOD16.required_parameters order) has a prior; its
// family and the transform between the sampler's y and the model's x:
//     Uniform(a, b)        x = a + (b - a) s(y)     log p(y) = -y - 2 softplus(-y)
//     LogNormal(mu, s)     x = exp(y)               log p(y) = (-log s - H) - (y - mu)^2 / (2 s s)
//     Triangular(a, c, b)  x = a + (b - a) s(y)     log p(y) = ((log f(x) + log(b - a)) - y) - 2 softplus(-y)
// with s(y) = 1 / (1 + exp(-y)), softplus(z) = log1p(exp(z)) (z for z > 36), H = 0x1.d67f1c864beb4p-1
// (1/2 log 2 pi), f(x) = 2 (x - a) / ((b - a)(c - a)) for x < c, else 2 (b - x) / ((b - a)(b - c));
// log f = -inf where f is not > 0 (c = a and c = b both work). The log-densities include the
// Jacobian; they are summed over i in order, then the log-likelihood is added. Every expression is
// evaluated left to right as written, with contraction off. The initial y of an x is log x
// (LogNormal) or log(p / (1 - p)) with p = (x - a) / (b - a).
//
// Log-likelihood of the row's weighted (sse, count) (static_obj_final_kernel): objective 0 (rmsd)
// -sqrt(sse / count); objective 1 (gaussian) -0.5 sse. With the annual-precipitation constraint
// (spec.constraints bit 0, a problem with mod16_static_batch_set_annual) the row's penalty
// (static_annual_final_kernel, <= 0 or NaN) is added to either: loglik = objective + penalty. A NaN
// penalty makes the log posterior NaN: rule 6 rejects the step.
//
// Random stream (mix: splitmix64's finaliser, the sobol_mix of mod16_sobol.hpp):
//     r(c, t, k) = mix(mix(mix(seed) ^ c) ^ ((t << 6) | k))      chain c, step t (0-based, tuning
//                                                                 included), slot k < 64
// Groups (mod16_mcmc_create_groups: `chains` chains for each listed fold f_g, one graph): chain j of
// group g is global chain g chains + j, and its stream is the plain sampler's with seed
// (seed + f_g) mod 2^64 and chain index j:
//     r = mix(mix(mix(seed + f_g) ^ j) ^ ((t << 6) | k))
// The key mix(mix(seed + f_g) ^ j) of every chain is made on the host (a plain sampler: one group,
// f = 0). Group g's chains evaluate their objective with the fold code f_g (TRAIN).
//     unit(z) = (z >> 11) 2^-53;  index(z, m) = floor(z m / 2^64) (the high half of the product)
// Slots: 0 .. d-1 proposal noise; 16 the first history index, 17, 18, ... the second, redrawn on
// the next slot while it equals the first (after slot 47: first + 1 mod m); 63 the Metropolis uniform.
//
// One step t of chain c (PyMC DEMetropolisZ.astep):
//   1. tuning: if tune_target != none and 0 < t < tune_steps and t % tune_interval == 0, scaling (or
//      lamb) *= factor(accepted / tune_interval) -- < 0.001: 0.1, < 0.05: 0.5, < 0.2: 0.9, > 0.95: 10,
//      > 0.75: 2, > 0.5: 1.1, else 1 (PyMC's tune()) -- and the accepted count restarts at 0;
//   2. noise e_i = (2 unit(r(c, t, i)) - 1) scaling;
//   3. the history window [lo, t): entry j is the state after step j; lo = 0 while t < tune_steps,
//      floor(tune_drop_fraction tune_steps) after (PyMC's stop_tuning drops that many entries);
//   4. m = t - lo; m >= 2: y' = (y + lamb (z1 - z2)) + e with z1, z2 the entries lo + index(.., m);
//      otherwise y' = y + e;
//   5. logp(y') through the objective (x-row: the free x-values and the fixed values);
//   6. accept iff mr = logp(y') - logp(y) is finite and log((( r(c, t, 63) >> 11) + 0.5) 2^-53) < mr;
//   7. append the resulting state (y, x, log-likelihood, log-posterior, accepted) at step t.
#pragma once
#include <stdint.h>
#include "mod16_kernels.hpp"

namespace mod16 {

constexpr int kMcmcMaxD = 11;
constexpr int kMcmcSlotI1 = 16, kMcmcSlotLast = 47, kMcmcSlotU = 63;
enum { kPriorUniform = 0, kPriorLogNormal = 1, kPriorTriangular = 2 };

struct McmcArgs {
    int chains, d;
    int idx[kMcmcMaxD];                 // column of free parameter i
    int fam[kMcmcMaxD];
    double p0[kMcmcMaxD], p1[kMcmcMaxD], p2[kMcmcMaxD];     // (a, b, -) / (mu, s, -) / (a, b, c)
    double fixed[11];                   // the row's values; the free columns are overwritten
    int tune_target, tune_interval;     // 0 none, 1 scaling, 2 lamb
    int64_t tune_steps, drop_lo;
    int objective;                      // 0 rmsd, 1 gaussian
    const uint64_t* key;                // [chains] the chain's stream key (see "Groups")
    double scaling0, lamb0;
    // state, [d][chains] or [chains]
    double *y, *yp, *xc;
    double *logp, *loglik, *lprior_p, *scaling, *lamb;
    int* acc;
    int64_t* t;
    // history and trace, [step][chains][d] or [step][chains]
    double *hist, *xtr, *tr_ll, *tr_lp;
    uint8_t* tr_acc;
    // the objective's rows [chains][11] and its result [chains]
    double* params;
    const double *sse, *cnt;
    const double* penalty;              // [chains] the constraint's penalty of the row, NULL: no constraint
};

// (mod16_sobol.hpp's kernels are not included here: its sobol_mix, restated)
__host__ __device__ __forceinline__ uint64_t mcmc_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t mcmc_rand(uint64_t chain_key, int64_t t, int k) {
    return mcmc_mix(chain_key ^ (((uint64_t)t << 6) | (uint64_t)k));
}
__host__ __device__ __forceinline__ double mcmc_tune_factor(double rate) {
    if (rate < 0.001) return 0.1;
    if (rate < 0.05) return 0.5;
    if (rate < 0.2) return 0.9;
    if (rate > 0.95) return 10.0;
    if (rate > 0.75) return 2.0;
    if (rate > 0.5) return 1.1;
    return 1.0;
}
__device__ __forceinline__ double mcmc_unit(uint64_t z) { return (double)(z >> 11) * 0x1p-53; }
__device__ __forceinline__ int64_t mcmc_index(uint64_t z, int64_t m) { return (int64_t)__umul64hi(z, (uint64_t)m); }

__device__ inline double mcmc_softplus(double z) {
#pragma clang fp contract(off)
    return z > 36.0 ? z : log1p(exp(z));
}
__device__ inline double mcmc_x_of(int fam, double a, double b, double y) {
#pragma clang fp contract(off)
    if (fam == kPriorLogNormal) return exp(y);
    const double s = 1.0 / (1.0 + exp(-y));
    return a + (b - a) * s;
}
__device__ inline double mcmc_y_of(int fam, double a, double b, double x) {
#pragma clang fp contract(off)
    if (fam == kPriorLogNormal) return log(x);
    const double p = (x - a) / (b - a);
    return log(p / (1.0 - p));
}
// log p(y), the Jacobian included (x = mcmc_x_of(y))
__device__ inline double mcmc_log_prior(int fam, double p0, double p1, double p2, double y, double x) {
#pragma clang fp contract(off)
    if (fam == kPriorLogNormal) {
        const double u = y - p0;
        return (-log(p1) - 0x1.d67f1c864beb4p-1) - (u * u) / (2.0 * p1 * p1);
    }
    const double logistic = -y - 2.0 * mcmc_softplus(-y);
    if (fam == kPriorUniform) return logistic;
    const double a = p0, b = p1, c = p2;
    const double f = x < c ? 2.0 * (x - a) / ((b - a) * (c - a)) : 2.0 * (b - x) / ((b - a) * (b - c));
    const double lf = f > 0.0 ? log(f) : -__builtin_inf();
    return ((lf + log(b - a)) - y) - 2.0 * mcmc_softplus(-y);
}

// the fixed columns, then the x-value and log-prior of y' (a.yp) of chain c: the row the objective reads
__device__ inline void mcmc_row(const McmcArgs& a, int c) {
#pragma clang fp contract(off)
    double* row = a.params + (int64_t)c * 11;
    for (int k = 0; k < 11; ++k) row[k] = a.fixed[k];
    double lp = 0.0;
    for (int i = 0; i < a.d; ++i) {
        const double y = a.yp[(int64_t)i * a.chains + c];
        const double x = mcmc_x_of(a.fam[i], a.p0[i], a.p1[i], y);
        row[a.idx[i]] = x;
        lp += mcmc_log_prior(a.fam[i], a.p0[i], a.p1[i], a.p2[i], y, x);
    }
    a.lprior_p[c] = lp;
}

__device__ inline double mcmc_loglik(const McmcArgs& a, int c) {
#pragma clang fp contract(off)
    const double sse = a.sse[c], cnt = a.cnt[c];
    const double ll = a.objective == 0 ? -sqrt(sse / cnt) : -0.5 * sse;
    return a.penalty ? ll + a.penalty[c] : ll;
}

// the initial point: x0 [chains][d] -> y, its row (the objective runs behind this kernel)
__global__ void __launch_bounds__(kBlock) mcmc_init_kernel(const McmcArgs a, const double* x0) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= a.chains) return;
    for (int i = 0; i < a.d; ++i)
        a.yp[(int64_t)i * a.chains + c] = mcmc_y_of(a.fam[i], a.p0[i], a.p1[i], x0[(int64_t)c * a.d + i]);
    mcmc_row(a, c);
}
// ... and its log posterior: the chain's state at t = 0
__global__ void __launch_bounds__(kBlock) mcmc_init_accept_kernel(const McmcArgs a) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= a.chains) return;
    const double ll = mcmc_loglik(a, c);
    for (int i = 0; i < a.d; ++i) {
        a.y[(int64_t)i * a.chains + c] = a.yp[(int64_t)i * a.chains + c];
        a.xc[(int64_t)i * a.chains + c] = a.params[(int64_t)c * 11 + a.idx[i]];
    }
    a.loglik[c] = ll;
    a.logp[c] = a.lprior_p[c] + ll;
    a.scaling[c] = a.scaling0;
    a.lamb[c] = a.lamb0;
    a.acc[c] = 0;
    a.t[c] = 0;
}

// steps 1-4 (and the row of step 5)
__global__ void __launch_bounds__(kBlock) mcmc_propose_kernel(const McmcArgs a) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= a.chains) return;
    const int64_t t = a.t[c];
    double sc = a.scaling[c], lb = a.lamb[c];
    if (a.tune_target && t > 0 && t < a.tune_steps && t % a.tune_interval == 0) {
        const double f = mcmc_tune_factor((double)a.acc[c] / (double)a.tune_interval);
        if (a.tune_target == 1) sc = sc * f;
        else lb = lb * f;
        a.scaling[c] = sc;
        a.lamb[c] = lb;
        a.acc[c] = 0;
    }
    const uint64_t key = a.key[c];
    const int64_t lo = t < a.tune_steps ? 0 : a.drop_lo;
    const int64_t m = t - lo;
    const double *z1 = nullptr, *z2 = nullptr;
    if (m >= 2) {
        const int64_t i1 = mcmc_index(mcmc_rand(key, t, kMcmcSlotI1), m);
        int k = kMcmcSlotI1 + 1;
        int64_t i2 = mcmc_index(mcmc_rand(key, t, k), m);
        while (i2 == i1 && k < kMcmcSlotLast) i2 = mcmc_index(mcmc_rand(key, t, ++k), m);
        if (i2 == i1) i2 = (i1 + 1) % m;
        z1 = a.hist + ((lo + i1) * a.chains + c) * a.d;
        z2 = a.hist + ((lo + i2) * a.chains + c) * a.d;
    }
    for (int i = 0; i < a.d; ++i) {
        const double e = (2.0 * mcmc_unit(mcmc_rand(key, t, i)) - 1.0) * sc;
        const double y = a.y[(int64_t)i * a.chains + c];
        double yp;
        if (z1) {
            const double dz = lb * (z1[i] - z2[i]);
            yp = (y + dz) + e;
        } else {
            yp = y + e;
        }
        a.yp[(int64_t)i * a.chains + c] = yp;
    }
    mcmc_row(a, c);
}

// steps 6-7
__global__ void __launch_bounds__(kBlock) mcmc_accept_kernel(const McmcArgs a) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= a.chains) return;
    const int64_t t = a.t[c];
    const uint64_t key = a.key[c];
    const double ll = mcmc_loglik(a, c);
    const double lp = a.lprior_p[c] + ll;
    const double mr = lp - a.logp[c];
    const double lu = log(((double)(mcmc_rand(key, t, kMcmcSlotU) >> 11) + 0.5) * 0x1p-53);
    const bool take = isfinite(mr) && lu < mr;
    if (take) {
        for (int i = 0; i < a.d; ++i) {
            a.y[(int64_t)i * a.chains + c] = a.yp[(int64_t)i * a.chains + c];
            a.xc[(int64_t)i * a.chains + c] = a.params[(int64_t)c * 11 + a.idx[i]];
        }
        a.logp[c] = lp;
        a.loglik[c] = ll;
        a.acc[c] += 1;
    }
    const int64_t o = t * a.chains + c;
    for (int i = 0; i < a.d; ++i) {
        a.hist[o * a.d + i] = a.y[(int64_t)i * a.chains + c];
        a.xtr[o * a.d + i] = a.xc[(int64_t)i * a.chains + c];
    }
    a.tr_ll[o] = a.loglik[c];
    a.tr_lp[o] = a.logp[c];
    a.tr_acc[o] = take ? 1 : 0;
    a.t[c] = t + 1;
}

}  // namespace mod16
