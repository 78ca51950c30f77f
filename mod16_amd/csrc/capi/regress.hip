// libmod16hip.so -- per-pixel weighted least squares over a stack, shared and per-pixel terms: mod16_regress_f32 / _f64 (coefficients, standard errors, sums of squares, R^2, counts and the residual or fitted series of every pixel in one launch), mod16_regress_max_steps / _max_terms
#include "host.hpp"
#include "../mod16_regress.hpp"

// All pointers are device pointers here (the design too).
template <typename IN>
static int launch_regress(mod16_ctx* ctx, const RegressArgs& a, int terms, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock)), block(kBlock);
    switch (terms) {
        case 1: hipLaunchKernelGGL((regress_kernel<IN, 1>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((regress_kernel<IN, 2>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((regress_kernel<IN, 3>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((regress_kernel<IN, 4>), grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL((regress_kernel<IN, 5>), grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL((regress_kernel<IN, 6>), grid, block, 0, st, a); break;
        case 7: hipLaunchKernelGGL((regress_kernel<IN, 7>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((regress_kernel<IN, 8>), grid, block, 0, st, a); break;
        default: return fail(ctx, MOD16_ERR_ARG, "mod16_regress: internal: no kernel for this number of terms");
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

// HOST mode: the outputs (coef and se as P slabs, the three sums and the counts as one, the series as T),
// then the T slabs of the values, of every per-pixel term and of the weights, through the shared staging
// path; the tile cut so that a slot's slab fits stage_bytes. Every array sits in float64-sized places.
// The design goes whole to a block of device memory the context owns.
template <typename IN>
static int regress_host(mod16_ctx* ctx, const RegressArgs& a, int kp, int64_t stage_bytes) {
    const int T = a.steps, P = a.ks + kp;
    enum { kCoef = 0, kSe, kRss, kTss, kR2, kCount, kSeries, kValues, kTerms };
    HostPlan p((int)sizeof(double));
    p.add(kOut, a.coef, false, P, a.coef_pitch);
    p.add(kOut, a.se, false, a.se ? P : 1, a.se_pitch);
    p.add(kOut, a.rss);
    p.add(kOut, a.tss);
    p.add(kOut, a.r2);
    p.add(kOut, a.count, false, 1, 0, (int)sizeof(uint16_t));
    p.add(kOut, a.series, false, a.series ? T : 1, a.s_pitch, (int)sizeof(IN));
    p.add(kIn, a.values, false, T, a.v_pitch, (int)sizeof(IN));
    for (int k = 0; k < kp; ++k) p.add(kIn, a.cols[a.ks + k], false, T, a.t_pitch, (int)sizeof(IN));
    p.add(kIn, a.weights, false, a.weights ? T : 1, a.w_pitch, (int)sizeof(float));
    if (a.ks) {
        const size_t bytes = (size_t)T * a.ks * sizeof(double);
        if (ctx->regress_design.bytes() < bytes) {
            if (ctx->regress_design) ctx->retired.push_back(std::move(ctx->regress_design));
            int rc = ctx->regress_design.alloc(ctx, bytes, "mod16_regress: device memory for the design");
            if (rc != MOD16_OK) return rc;
        }
        HIPCHK(ctx, hipMemcpy(ctx->regress_design.get(), a.design, bytes, hipMemcpyHostToDevice));
    }
    auto launch = [&](const HostTile& t) {
        RegressArgs d = a;
        d.n = t.m;
        d.design = a.ks ? ctx->regress_design.as<double>() : nullptr;
        d.coef = static_cast<double*>(t.dev[kCoef]);
        d.se = static_cast<double*>(t.dev[kSe]);
        d.rss = static_cast<double*>(t.dev[kRss]);
        d.tss = static_cast<double*>(t.dev[kTss]);
        d.r2 = static_cast<double*>(t.dev[kR2]);
        d.count = static_cast<uint16_t*>(t.dev[kCount]);
        d.series = t.dev[kSeries];
        d.values = t.dev[kValues];
        for (int k = 0; k < kp; ++k) d.cols[a.ks + k] = t.dev[kTerms + k];
        d.weights = static_cast<const float*>(t.dev[kTerms + kp]);
        d.coef_pitch = d.se_pitch = (int64_t)(t.row_bytes / sizeof(double));
        d.v_pitch = d.t_pitch = d.s_pitch = (int64_t)(t.row_bytes / sizeof(IN));
        d.w_pitch = (int64_t)(t.row_bytes / sizeof(float));
        return launch_regress<IN>(ctx, d, P, t.st);
    };
    return host_tiled(ctx, p, a.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, sizeof(double), stage_bytes));
}

template <typename IN>
static int regress_entry(mod16_ctx* ctx, const mod16_regress_spec* spec, const IN* values, const double* design,
                         const IN* const* terms, const float* weights, double* coef, double* se, double* rss, double* tss,
                         double* r2, uint16_t* count, IN* series, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_regress: ", what); };
    if (!spec || !values || !coef) return bad("NULL spec, values or coef");
    if (spec->n < 0) return bad("n < 0");
    if (spec->steps < 1 || spec->steps > kRegressMaxSteps) return bad("steps must be between 1 and 4096");
    const int ks = spec->ks, kp = spec->kp;
    if (ks < 0 || kp < 0 || ks > kRegressMaxTerms || kp > kRegressMaxTerms || ks + kp < 1 || ks + kp > kRegressMaxTerms)
        return bad("ks and kp must not be negative and ks + kp must be between 1 and 8");
    const int P = ks + kp, T = spec->steps;
    if ((ks > 0) != (design != nullptr)) return bad("design must be given exactly where ks > 0");
    if ((kp > 0) != (terms != nullptr)) return bad("terms must be given exactly where kp > 0");
    for (int k = 0; k < kp; ++k)
        if (!terms[k]) return bad("terms holds a NULL pointer");
    if (spec->min_valid < P) return bad("min_valid must be at least ks + kp");
    const int mode = spec->series;
    if (mode != MOD16_REGRESS_SERIES_NONE && mode != MOD16_REGRESS_SERIES_RESIDUALS && mode != MOD16_REGRESS_SERIES_FITTED)
        return bad("series must be MOD16_REGRESS_SERIES_NONE, MOD16_REGRESS_SERIES_RESIDUALS or MOD16_REGRESS_SERIES_FITTED");
    if ((mode == MOD16_REGRESS_SERIES_NONE) != (series == nullptr)) return bad("a series output must be given exactly where spec->series asks for one");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int64_t n = spec->n;
    if (spec->value_pitch < n) return bad("value_pitch must be at least n");
    if (kp && spec->term_pitch < n) return bad("term_pitch must be at least n");
    if (weights && spec->weight_pitch < n) return bad("weight_pitch must be at least n");
    if (spec->coef_pitch < n) return bad("coef_pitch must be at least n");
    if (se && spec->se_pitch < n) return bad("se_pitch must be at least n");
    if (series && spec->series_pitch < n) return bad("series_pitch must be at least n");
    if (design && where == MOD16_HOST)
        for (int64_t k = 0; k < (int64_t)T * ks; ++k)
            if (!std::isfinite(design[k])) return bad("design must be finite");
    if (n == 0) return MOD16_OK;
    // in place is refused: no output may share a byte with an input or with another output
    {
        Extent ins[kRegressMaxTerms + 3], outs[7];
        int ni = 0, no = 0;
        ins[ni++] = extent(values, 1, 0, T, spec->value_pitch, n, sizeof(IN));
        if (design) ins[ni++] = extent(design, (int64_t)T * ks, sizeof(double));
        for (int k = 0; k < kp; ++k) ins[ni++] = extent(terms[k], 1, 0, T, spec->term_pitch, n, sizeof(IN));
        if (weights) ins[ni++] = extent(weights, 1, 0, T, spec->weight_pitch, n, sizeof(float));
        outs[no++] = extent(coef, 1, 0, P, spec->coef_pitch, n, sizeof(double));
        if (se) outs[no++] = extent(se, 1, 0, P, spec->se_pitch, n, sizeof(double));
        if (rss) outs[no++] = extent(rss, n, sizeof(double));
        if (tss) outs[no++] = extent(tss, n, sizeof(double));
        if (r2) outs[no++] = extent(r2, n, sizeof(double));
        if (count) outs[no++] = extent(count, n, sizeof(uint16_t));
        if (series) outs[no++] = extent(series, 1, 0, T, spec->series_pitch, n, sizeof(IN));
        if (overlaps(outs, no, ins, ni)) return bad("an output overlaps an input or another output");
    }
    RegressArgs a;
    memset(&a, 0, sizeof a);
    a.values = values;
    a.design = design;
    for (int k = 0; k < kp; ++k) a.cols[ks + k] = terms[k];
    a.weights = weights;
    a.coef = coef;
    a.se = se;
    a.rss = rss;
    a.tss = tss;
    a.r2 = r2;
    a.count = count;
    a.series = series;
    a.n = n;
    a.v_pitch = spec->value_pitch;
    a.t_pitch = kp ? spec->term_pitch : 0;
    a.w_pitch = weights ? spec->weight_pitch : 0;
    a.coef_pitch = spec->coef_pitch;
    a.se_pitch = se ? spec->se_pitch : 0;
    a.s_pitch = series ? spec->series_pitch : 0;
    a.steps = T;
    a.ks = ks;
    a.min_valid = spec->min_valid;
    a.series_mode = mode;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_regress<IN>(ctx, a, P, static_cast<hipStream_t>(stream));
    return regress_host<IN>(ctx, a, kp, stage_budget(stage_bytes));
}

extern "C" int mod16_regress_f32(mod16_ctx* ctx, const mod16_regress_spec* spec, const float* values, const double* design,
                                 const float* const* terms, const float* weights, double* coef, double* se, double* rss,
                                 double* tss, double* r2, uint16_t* count, float* series, int where, void* stream,
                                 size_t stage_bytes) {
    return regress_entry<float>(ctx, spec, values, design, terms, weights, coef, se, rss, tss, r2, count, series, where, stream,
                                stage_bytes);
}
extern "C" int mod16_regress_f64(mod16_ctx* ctx, const mod16_regress_spec* spec, const double* values, const double* design,
                                 const double* const* terms, const float* weights, double* coef, double* se, double* rss,
                                 double* tss, double* r2, uint16_t* count, double* series, int where, void* stream,
                                 size_t stage_bytes) {
    return regress_entry<double>(ctx, spec, values, design, terms, weights, coef, se, rss, tss, r2, count, series, where, stream,
                                 stage_bytes);
}
extern "C" int mod16_regress_max_steps(void) { return kRegressMaxSteps; }
extern "C" int mod16_regress_max_terms(void) { return kRegressMaxTerms; }
