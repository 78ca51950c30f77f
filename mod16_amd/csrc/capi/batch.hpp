// libmod16hip.so, host side: the resident calibration problem (mod16_batch) and the launches of one
// FAST objective evaluation on it -- shared by the problem's own entry points (calibration.hip) and
// the sampler that captures them into its graphs (mcmc.hip).
#pragma once
#include "internal.hpp"
#include "../mod16_methods.hpp"

// The evaluation workspace of the FAST objective: the parameter rows it reads and everything it
// writes. The problem owns one (mod16_batch::own); a sampler (capi/mcmc.hip) owns its own, so that a
// larger objective() call, which regrows the problem's per-block part, never pulls memory from under a
// graph the sampler has captured.
struct EvalWs {
    void* params = nullptr;             // [ndraw][11] of the data type
    double *par16 = nullptr, *partial = nullptr, *redo = nullptr, *sse = nullptr, *cnt = nullptr;
    unsigned *any_gs = nullptr, *any_draw = nullptr;
    const int32_t* code = nullptr;      // [ndraw] fold code per draw (the FOLD kernels); NULL: plain draws
    // the annual-precipitation constraint (mod16_static_batch_set_annual); mass NULL: plain draws
    double *mass = nullptr, *rmass = nullptr, *penalty = nullptr;
};
// Its two parts inside an allocation at `base` (NULL: sizes only), with the extents the kernels of
// mod16_methods.hpp index. Per draw (`el`: bytes of the data type): params [draws][11], par16
// [draws][kPar16], sse / cnt / any_draw [draws], redo [draws][5], and for a problem with G site-years
// (G = 0: none) penalty [draws], rmass [draws][G][2] ...
static size_t eval_layout_draws(int64_t draws, size_t el, void* base, EvalWs* w, int G = 0) {
    EvalWs sizes_only;
    if (!w) w = &sizes_only;
    Carver c(base);
    const size_t D = (size_t)draws;
    w->params = c.take<char>(D * 11 * el);
    w->par16 = c.take<double>(D * kPar16 * sizeof(double));
    w->sse = c.take<double>(D * sizeof(double));
    w->cnt = c.take<double>(D * sizeof(double));
    w->redo = c.take<double>(D * 5 * sizeof(double));
    w->any_draw = c.take<unsigned>(D * sizeof(unsigned));
    if (G) {
        w->penalty = c.take<double>(D * sizeof(double));
        w->rmass = c.take<double>(D * (size_t)G * 2 * sizeof(double));
    }
    return c.used;
}
// ... and per block of kBlock pixels: partial [gx][draws][2], any_gs [gx][draws] (draws x blocks x 20
// bytes: 3.2 GB at 4096 draws x 10 M pixels, so the problem sizes this part for the draws an
// evaluation actually brings, not for max_draws; an EXACT problem never has it); `annual`: and per wave
// of 64 pixels mass [gx * kBlock / 64][draws]
static size_t eval_layout_blocks(int64_t draws, int gx, void* base, EvalWs* w, bool annual = false) {
    EvalWs sizes_only;
    if (!w) w = &sizes_only;
    Carver c(base);
    const size_t cells = (size_t)draws * (size_t)gx;
    w->partial = c.take<double>(cells * 2 * sizeof(double));
    w->any_gs = c.take<unsigned>(cells * sizeof(unsigned));
    if (annual) w->mass = c.take<double>(cells * (kBlock / 64) * sizeof(double));
    return c.used;
}

// The resident arrays and what is sized by them: bind fills one, and mod16_static_batch_set_annual
// builds a second one (the same pixels laid out site-year-major) and moves it into the problem whole.
struct BatchArrays {
    int64_t n = 0;                      // the resident arrays' pixels (with the constraint: padding included)
    int gx = 0;
    DevMem owned;                       // the resident copies (HOST bind); empty when the caller's device arrays are used
    const void* drv[14] = {};           // views: into `owned`, or the caller's
    const void* obs = nullptr;          // ...
    const void* wts = nullptr;
    DevMem skip;                        // uint8 [n]: 1 = outside the FAST domain
    DevMem list;                        // int64: those pixels, ascending
    int64_t nlist = 0;
    DevMem ws;                          // the per-draw part of `own` for max_draws draws, and dflags
    EvalWs own;                         // views into `ws` and (the per-block part) into mod16_batch::eval_ws
    unsigned* dflags = nullptr;         // [max_draws]: the rows kernels' any(g_surf > 0) words; a view into `ws`
    PinnedMem hout;                     // pinned double [2][max_draws] ([3]: with the constraint)
    // the annual-precipitation constraint (mod16_static_batch_set_annual): the resident arrays are laid
    // out site-year-major, every site-year padded to whole waves (the kernels' comment in
    // mod16_methods.hpp); G = 0: none
    int G = 0;                          // site-years, g = year * sites + site
    double S = 0.0;                     // sum of the limits
    DevMem annual;                      // one allocation: the tables below
    const double* scale = nullptr;      // [n] 86400 / lhv, 0 = padding; a view into `owned`
    int32_t* wstart = nullptr;          // [G + 1] first wave of each site-year; views into `annual` ...
    double* limit = nullptr;            // [G] annual_precip
    int64_t* lstart = nullptr;          // [G + 1] first entry of `list` of each site-year
    int64_t* pos = nullptr;             // [n_user] where the caller's pixel lies
};

// ---- the calibration problem RESIDENT on the device (mod16_static_batch_bind_*): drivers,
// observations and weights go up once; an evaluation is parameters up, one graph launch (kernels
// only), (sse, count) down.
// Ownership: members go in reverse order of declaration, then the BatchArrays -- the stream first
// (mod16_static_batch_destroy has synchronized it), then the graphs, then the memory they point into.
struct mod16_batch : BatchArrays {
    mod16_ctx* ctx = nullptr;           // a view: the context outlives its problems
    int device = 0;
    bool f32 = false;
    unsigned flags = 0;
    int64_t max_draws = 0;
    int64_t n_user = 0;                 // the caller's n (mod16_static_batch_info, the rows)
    uint32_t dense_drv = 0;
    DevMem eval_ws;                     // the per-block part of `own` for eval_draws draws (grown on demand: batch_eval_ws)
    int64_t eval_draws = 0;
    DevMem rows;                        // [ndraw][n] x up to 3: rows workspace, allocated when first asked for; only grows
    PinnedMem hparams;                  // pinned staging
    // cross-validation (mod16_static_batch_set_folds): a fold label per pixel, resident; the fold
    // objective's codes and its own cached graph (plain and fold calls never share one: the launches
    // differ in kernels and in the codes' address)
    DevMem label;                       // uint8 [n], empty: no folds
    int nfolds = 0;
    DevMem dcode;                       // int32 [max_draws] device
    PinnedMem hcode;                    // int32 [max_draws] pinned staging
    CachedGraph graph, fgraph, agraph;  // the plain, the fold and the constrained objective, key = draws
    CachedGraph* last = nullptr;        // the one the last objective call launched (mod16_static_batch_time); a view
    int samplers = 0;                   // samplers alive on the problem (capi/mcmc.hip)
    Stream st;
};

// w.code set: the FOLD instances (the problem's labels, the draws' fold codes); otherwise the plain ones.
// (Folds exist on float64 problems only: kFold keeps float32 FOLD instances out of the library.)
// w.mass set (never together with w.code): the ANNUAL instances and the penalty's two kernels.
template <typename T>
static void batch_objective_launches(const mod16_batch* b, const EvalWs& w, int64_t ndraw) {
    constexpr bool kFold = std::is_same<T, double>::value;
    const bool fold = kFold && w.code != nullptr;
    const bool annual = kFold && !fold && w.mass != nullptr;
    hipStream_t st = b->st;
    const unsigned gd = (unsigned)((ndraw + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((static_obj_params_kernel<T>), dim3(gd), dim3(kBlock), 0, st, static_cast<const T*>(w.params), ndraw, w.par16);
    StaticObjArgs<T> a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 14; ++k) a.drv[k] = static_cast<const T*>(b->drv[k]);
    a.dense_drv = b->dense_drv;
    a.n = b->n;
    a.observed = static_cast<const T*>(b->obs);
    a.weights = static_cast<const T*>(b->wts);
    a.skip = b->nlist ? b->skip.as<uint8_t>() : nullptr;
    a.par16 = w.par16;
    a.tab = b->ctx->tab64.as<double>();
    a.ndraw = ndraw;
    a.any_draw = w.any_draw;
    a.partial = w.partial;
    a.any_gs = w.any_gs;
    a.code = w.code;
    a.label = fold ? b->label.as<uint8_t>() : nullptr;
    a.scale = annual ? b->scale : nullptr;
    a.mass = annual ? w.mass : nullptr;
    const dim3 grid((unsigned)b->gx, (unsigned)((ndraw + kObjDraws - 1) / kObjDraws));
    if (fold) hipLaunchKernelGGL((static_obj_kernel<T, true, kFold>), grid, dim3(kBlock), 0, st, a);
    else if (annual) hipLaunchKernelGGL((static_obj_kernel<T, true, false, kFold>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((static_obj_kernel<T, true>), grid, dim3(kBlock), 0, st, a);
    if (b->nlist) {
        StaticObjRedoArgs<T> r;
        memset(&r, 0, sizeof r);
        for (int k = 0; k < 14; ++k) r.drv[k] = static_cast<const T*>(b->drv[k]);
        r.dense_drv = b->dense_drv;
        r.params = static_cast<const T*>(w.params);
        r.observed = a.observed;
        r.weights = a.weights;
        r.list = b->list.as<int64_t>();
        r.nlist = b->nlist;
        r.redo = w.redo;
        r.code = w.code;
        r.label = a.label;
        if (fold) hipLaunchKernelGGL((static_obj_redo_kernel<T, kFold>), dim3((unsigned)ndraw), dim3(kBlock), 0, st, r);
        else hipLaunchKernelGGL((static_obj_redo_kernel<T>), dim3((unsigned)ndraw), dim3(kBlock), 0, st, r);
        if constexpr (kFold) if (annual) {      // (float64 only, as the ANNUAL instances)
            StaticAnnualRedoArgs<T> m;
            memset(&m, 0, sizeof m);
            for (int k = 0; k < 14; ++k) m.drv[k] = r.drv[k];
            m.dense_drv = r.dense_drv;
            m.params = r.params;
            m.scale = b->scale;
            m.list = b->list.as<int64_t>();
            m.lstart = b->lstart;
            m.G = b->G;
            m.rmass = w.rmass;
            hipLaunchKernelGGL((static_annual_redo_kernel<T>), dim3((unsigned)ndraw), dim3(kBlock), 0, st, m);
        }
    }
    const double* redo = b->nlist ? w.redo : nullptr;
    const unsigned gr = (unsigned)((ndraw + kObjPerBlock - 1) / kObjPerBlock);
    hipLaunchKernelGGL(static_obj_any_kernel, dim3(gr), dim3(kBlock), 0, st, w.any_gs, redo, ndraw, b->gx, w.any_draw);
    if (fold) hipLaunchKernelGGL((static_obj_kernel<T, false, kFold>), grid, dim3(kBlock), 0, st, a);
    else if (annual) hipLaunchKernelGGL((static_obj_kernel<T, false, false, kFold>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((static_obj_kernel<T, false>), grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(static_obj_final_kernel, dim3(gr), dim3(kBlock), 0, st, w.partial, redo, w.any_draw, ndraw, b->gx,
                       w.sse, w.cnt);
    if (annual)
        hipLaunchKernelGGL(static_annual_final_kernel, dim3(gr), dim3(kBlock), 0, st, w.mass, b->nlist ? w.rmass : nullptr,
                           w.any_draw, b->wstart, b->limit, b->G, b->S, ndraw, w.penalty);
}

