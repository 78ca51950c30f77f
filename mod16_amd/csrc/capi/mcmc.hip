// libmod16hip.so -- the DE-MCMC-Z sampler on a resident problem: mod16_mcmc_* (kernels and the
// arithmetic: ../mod16_mcmc.hpp)
#include "batch.hpp"
#include "../mod16_mcmc.hpp"

constexpr int kMcmcSegment = 64;          // steps per captured graph unless the spec says otherwise

// (Members go in reverse order of declaration: the graphs before the memory their nodes point into;
// they run on the problem's stream, which mod16_mcmc_destroy synchronizes first.)
struct mod16_mcmc {
    mod16_batch* b = nullptr;             // a view: the problem outlives its samplers
    McmcArgs a;                           // the kernels' arguments: views into the allocations below
    DevMem state;                         // y, yp, xc, logp ... t: one allocation
    DevMem eval;                          // the objective's workspace for `chains` draws (EvalWs)
    EvalWs w;                             // views into `eval`
    DevMem trace;                         // hist, xtr, tr_ll, tr_lp, tr_acc for `cap` steps
    int64_t cap = 0, steps = 0;
    int segment = kMcmcSegment;
    CachedGraph full, rem;                // `segment` steps, and the last run's remainder; key = steps
    bool broken = false;                  // a run failed: the device step counters and `steps` may disagree
    bool counted = false;                 // in the problem's count of samplers
};

static void mcmc_drop_graphs(mod16_mcmc* m) {
    m->full.drop();
    m->rem.drop();
}

extern "C" int mod16_mcmc_destroy(mod16_mcmc* m) {
    if (!m) return MOD16_OK;
    MOD16_LOCK(m->b->ctx);
    (void)hipSetDevice(m->b->device);
    (void)hipStreamSynchronize(m->b->st);
    if (m->counted) --m->b->samplers;
    delete m;
    return MOD16_OK;
}

// the trace arrays of `cap` steps inside one allocation at `base` (NULL: sizes only)
static size_t mcmc_trace_layout(const McmcArgs& a, int64_t cap, char* base, McmcArgs* out) {
    const size_t per_x = align256((size_t)cap * a.chains * a.d * 8), per_s = align256((size_t)cap * a.chains * 8),
                 per_b = align256((size_t)cap * a.chains);
    if (out) {
        out->hist = reinterpret_cast<double*>(base);
        out->xtr = reinterpret_cast<double*>(base + per_x);
        out->tr_ll = reinterpret_cast<double*>(base + 2 * per_x);
        out->tr_lp = reinterpret_cast<double*>(base + 2 * per_x + per_s);
        out->tr_acc = reinterpret_cast<uint8_t*>(base + 2 * per_x + 2 * per_s);
    }
    return 2 * per_x + 2 * per_s + per_b;
}

// room for `need` steps: a larger allocation, the steps taken copied over, the graphs (which hold the
// old addresses) dropped
static int mcmc_reserve(mod16_mcmc* m, int64_t need) {
    if (need <= m->cap) return MOD16_OK;
    mod16_ctx* ctx = m->b->ctx;
    DevMem nt;
    int rc = nt.alloc(ctx, mcmc_trace_layout(m->a, need, nullptr, nullptr), "mod16_mcmc_run: device memory for the history and trace of this many steps");
    if (rc != MOD16_OK) return rc;
    McmcArgs na = m->a;
    mcmc_trace_layout(m->a, need, nt.as<char>(), &na);
    HIPCHK(ctx, hipStreamSynchronize(m->b->st));
    if (m->steps) {
        const size_t nx = (size_t)m->steps * m->a.chains * m->a.d * 8, ns = (size_t)m->steps * m->a.chains;
        HIPCHK(ctx, hipMemcpy(na.hist, m->a.hist, nx, hipMemcpyDeviceToDevice));
        HIPCHK(ctx, hipMemcpy(na.xtr, m->a.xtr, nx, hipMemcpyDeviceToDevice));
        HIPCHK(ctx, hipMemcpy(na.tr_ll, m->a.tr_ll, ns * 8, hipMemcpyDeviceToDevice));
        HIPCHK(ctx, hipMemcpy(na.tr_lp, m->a.tr_lp, ns * 8, hipMemcpyDeviceToDevice));
        HIPCHK(ctx, hipMemcpy(na.tr_acc, m->a.tr_acc, ns, hipMemcpyDeviceToDevice));
    }
    mcmc_drop_graphs(m);
    m->trace = std::move(nt);
    m->a = na;
    m->cap = need;
    return MOD16_OK;
}

// `steps` steps as one graph on the problem's stream: propose -> objective -> accept, a single chain
static int mcmc_capture(mod16_mcmc* m, int64_t steps, CachedGraph* g) {
    mod16_batch* b = m->b;
    const unsigned gc = (unsigned)((m->a.chains + kBlock - 1) / kBlock);
    return g->capture(b->ctx, b->st, steps, [&] {
        for (int64_t s = 0; s < steps; ++s) {
            hipLaunchKernelGGL(mcmc_propose_kernel, dim3(gc), dim3(kBlock), 0, b->st, m->a);
            batch_objective_launches<double>(b, m->w, m->a.chains);
            hipLaunchKernelGGL(mcmc_accept_kernel, dim3(gc), dim3(kBlock), 0, b->st, m->a);
        }
    });
}

static int mcmc_check_spec(mod16_ctx* ctx, const mod16_batch* b, const mod16_mcmc_spec* s, int ngroups, const int32_t* fold) {
    if (b->f32 || (b->flags & MOD16_MATH_EXACT) || !b->obs)
        return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: the problem must be float64, MOD16_MATH_FAST and bound with observations");
    if (fold) {
        if (!b->label) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create_groups: the problem has no folds (mod16_static_batch_set_folds)");
        if (ngroups < 1 || ngroups > b->nfolds) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create_groups: ngroups outside 1 .. nfolds");
        for (int g = 0; g < ngroups; ++g) {
            if (fold[g] < 0 || fold[g] >= b->nfolds) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create_groups: a fold outside 0 .. nfolds - 1");
            for (int h = 0; h < g; ++h)
                if (fold[h] == fold[g]) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create_groups: a fold listed twice");
        }
    }
    if (s->constraints & ~MOD16_CONSTRAINT_ANNUAL_PRECIP)
        return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: unknown bits in constraints");
    if (s->constraints && (fold || !b->G))
        return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: the annual-precipitation constraint needs a problem that has it (mod16_static_batch_set_annual) and no folds");
    if (s->chains < 1 || (int64_t)s->chains * ngroups > b->max_draws)
        return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: chains (x groups) outside 1 .. the problem's max_draws");
    if (s->nfree < 1 || s->nfree > kMcmcMaxD) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: nfree outside 1 .. 11");
    for (int i = 0; i < s->nfree; ++i) {
        if (s->index[i] < 0 || s->index[i] > 10 || (i && s->index[i] <= s->index[i - 1]))
            return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: free columns must be ascending in 0 .. 10");
        const double p0 = s->p0[i], p1 = s->p1[i], p2 = s->p2[i];
        bool ok;
        switch (s->family[i]) {
        case MOD16_PRIOR_UNIFORM: ok = std::isfinite(p0) && std::isfinite(p1) && p0 < p1; break;
        case MOD16_PRIOR_LOGNORMAL: ok = std::isfinite(p0) && std::isfinite(p1) && p1 > 0.0; break;
        case MOD16_PRIOR_TRIANGULAR:
            ok = std::isfinite(p0) && std::isfinite(p1) && std::isfinite(p2) && p0 < p1 && p0 <= p2 && p2 <= p1; break;
        default: ok = false;
        }
        if (!ok) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: bad prior (family, lower < upper, lower <= c <= upper, sigma > 0)");
    }
    if (s->tune_target < 0 || s->tune_target > 2 || s->tune_interval < 1 || s->tune_steps < 0 ||
        !(s->tune_drop_fraction >= 0.0 && s->tune_drop_fraction < 1.0) || s->objective < 0 || s->objective > 1 ||
        !std::isfinite(s->lamb) || !std::isfinite(s->scaling) || s->segment < 0 || s->segment > 1024)
        return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: bad tuning, objective, lamb, scaling or segment");
    return MOD16_OK;
}

// ngroups groups of spec->chains chains; fold: NULL (a plain sampler, one group) or the groups' folds
static int mcmc_create(mod16_batch* b, const mod16_mcmc_spec* s, int ngroups, const int32_t* fold, const double* x0,
                       mod16_mcmc** out) {
    mod16_ctx* ctx = b->ctx;
    int rc = mcmc_check_spec(ctx, b, s, ngroups, fold);
    if (rc != MOD16_OK) return rc;
    const int C = s->chains * ngroups, d = s->nfree;
    // the chains' stream keys and fold codes (mod16_mcmc.hpp, "Groups")
    std::vector<uint64_t> keys((size_t)C);
    std::vector<int32_t> codes((size_t)C);
    for (int g = 0; g < ngroups; ++g)
        for (int j = 0; j < s->chains; ++j) {
            const int32_t f = fold ? fold[g] : 0;
            keys[(size_t)g * s->chains + j] = mcmc_mix(mcmc_mix(s->seed + (uint64_t)f) ^ (uint64_t)j);
            codes[(size_t)g * s->chains + j] = f;
        }
    // the initial x-values, [C][d]: the caller's (inside the supports) or the support points
    std::vector<double> init((size_t)C * d);
    for (int c = 0; c < C; ++c)
        for (int i = 0; i < d; ++i) {
            const double p0 = s->p0[i], p1 = s->p1[i], p2 = s->p2[i];
            double x;
            if (x0) {
                x = x0[(size_t)c * d + i];
                const bool in = s->family[i] == MOD16_PRIOR_LOGNORMAL ? (x > 0.0 && std::isfinite(x)) : (x > p0 && x < p1);
                if (!in) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: an initial value outside its prior's support");
            } else if (s->family[i] == MOD16_PRIOR_UNIFORM) {
                x = p0 + (p1 - p0) / 2.0;
            } else if (s->family[i] == MOD16_PRIOR_LOGNORMAL) {
                x = std::exp(p0 + p1 * p1 / 2.0);
            } else {
                x = (p0 + p1 + p2) / 3.0;
            }
            init[(size_t)c * d + i] = x;
        }
    HIPCHK(ctx, hipSetDevice(b->device));
    mod16_mcmc* m = new (std::nothrow) mod16_mcmc;
    if (!m) return MOD16_ERR_NOMEM;
    m->b = b;
    ++b->samplers;
    m->counted = true;
    m->segment = s->segment ? s->segment : kMcmcSegment;
    McmcArgs& a = m->a;
    memset(&a, 0, sizeof a);
    a.chains = C;
    a.d = d;
    for (int i = 0; i < d; ++i) {
        a.idx[i] = s->index[i];
        a.fam[i] = s->family[i];
        a.p0[i] = s->p0[i];
        a.p1[i] = s->p1[i];
        a.p2[i] = s->p2[i];
    }
    for (int k = 0; k < 11; ++k) a.fixed[k] = s->fixed[k];
    a.tune_target = s->tune_target;
    a.tune_interval = s->tune_interval;
    a.tune_steps = s->tune_steps;
    a.drop_lo = (int64_t)std::floor(s->tune_drop_fraction * (double)s->tune_steps);
    a.objective = s->objective;
    a.scaling0 = s->scaling;
    a.lamb0 = s->lamb;
    rc = [&]() -> int {
        // per-chain state: sized with a NULL base, then placed
        uint64_t* dkey = nullptr;
        double* dx0 = nullptr;
        auto state = [&](void* base) {
            Carver c(base);
            const size_t sd = (size_t)C * d * 8, s1 = (size_t)C * 8;
            a.y = c.take<double>(sd);
            a.yp = c.take<double>(sd);
            a.xc = c.take<double>(sd);
            a.logp = c.take<double>(s1);
            a.loglik = c.take<double>(s1);
            a.lprior_p = c.take<double>(s1);
            a.scaling = c.take<double>(s1);
            a.lamb = c.take<double>(s1);
            a.t = c.take<int64_t>(s1);
            a.key = dkey = c.take<uint64_t>(s1);
            dx0 = c.take<double>(init.size() * 8);
            a.acc = c.take<int>((size_t)C * 4);
            return c.used;
        };
        int r = m->state.alloc(ctx, state(nullptr), "mod16_mcmc_create: device memory for the chains' state");
        if (r != MOD16_OK) return r;
        state(m->state.get());
        // the objective's workspace for C draws, both parts: the sampler's own (see EvalWs); behind it
        // the groups' TRAIN codes, constant for the sampler's life and read by its graphs
        // (with the constraint: its per-draw and per-wave parts too, so the graphs run the ANNUAL launches)
        const bool annual = (s->constraints & MOD16_CONSTRAINT_ANNUAL_PRECIP) != 0;
        const int G = annual ? b->G : 0;
        const size_t per_draw = eval_layout_draws(C, 8, nullptr, nullptr, G), per_block = eval_layout_blocks(C, b->gx, nullptr, nullptr, annual);
        r = m->eval.alloc(ctx, per_draw + per_block + (fold ? align256((size_t)C * 4) : 0), "mod16_mcmc_create: device memory for the objective's workspace");
        if (r != MOD16_OK) return r;
        char* ev = m->eval.as<char>();
        eval_layout_draws(C, 8, ev, &m->w, G);
        eval_layout_blocks(C, b->gx, ev + per_draw, &m->w, annual);
        a.penalty = m->w.penalty;
        a.params = static_cast<double*>(m->w.params);
        a.sse = m->w.sse;
        a.cnt = m->w.cnt;
        hipStream_t st = b->st;
        HIPCHK(ctx, hipMemcpyAsync(dkey, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, st));
        if (fold) {
            int32_t* dcode = reinterpret_cast<int32_t*>(ev + per_draw + per_block);
            HIPCHK(ctx, hipMemcpyAsync(dcode, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, st));
            m->w.code = dcode;
        }
        // the initial point and its log posterior
        const unsigned gc = (unsigned)((C + kBlock - 1) / kBlock);
        HIPCHK(ctx, hipMemcpyAsync(dx0, init.data(), init.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mcmc_init_kernel, dim3(gc), dim3(kBlock), 0, st, a, (const double*)dx0);
        batch_objective_launches<double>(b, m->w, C);
        hipLaunchKernelGGL(mcmc_init_accept_kernel, dim3(gc), dim3(kBlock), 0, st, a);
        HIPCHK(ctx, hipGetLastError());
        std::vector<double> lp((size_t)C);
        HIPCHK(ctx, hipMemcpyAsync(lp.data(), a.logp, (size_t)C * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int c = 0; c < C; ++c)
            if (!std::isfinite(lp[(size_t)c]))
                return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_create: the initial log posterior is not finite");
        return MOD16_OK;
    }();
    if (rc != MOD16_OK) {
        mod16_mcmc_destroy(m);
        return rc;
    }
    *out = m;
    return MOD16_OK;
}

extern "C" int mod16_mcmc_create(mod16_batch* b, const mod16_mcmc_spec* spec, const double* x0, mod16_mcmc** out) {
    if (!b || !spec || !out) return MOD16_ERR_ARG;
    *out = nullptr;
    MOD16_LOCK(b->ctx);
    return mcmc_create(b, spec, 1, nullptr, x0, out);
}

extern "C" int mod16_mcmc_create_groups(mod16_batch* b, const mod16_mcmc_spec* spec, int ngroups, const int32_t* fold,
                                        const double* x0, mod16_mcmc** out) {
    if (!b || !spec || !fold || !out) return MOD16_ERR_ARG;
    *out = nullptr;
    MOD16_LOCK(b->ctx);
    return mcmc_create(b, spec, ngroups, fold, x0, out);
}

static int mcmc_run(mod16_mcmc* m, int64_t steps, float* ms) {
    mod16_batch* b = m->b;
    mod16_ctx* ctx = b->ctx;
    if (steps < 0 || steps > ((int64_t)1 << 40)) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_run: steps outside 0 .. 2^40");
    if (m->broken) return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_run: an earlier run of this sampler failed");
    if (ms) *ms = 0.f;
    if (steps == 0) return MOD16_OK;
    HIPCHK(ctx, hipSetDevice(b->device));
    int rc = mcmc_reserve(m, m->steps + steps);
    if (rc != MOD16_OK) return rc;
    const int64_t K = m->segment, full = steps / K, rem = steps % K;
    if (full && m->full.key != K) rc = mcmc_capture(m, K, &m->full);
    if (rc == MOD16_OK && rem && m->rem.key != rem) rc = mcmc_capture(m, rem, &m->rem);
    if (rc != MOD16_OK) return rc;
    EventTimer timer;
    if (ms) HIPCHK(ctx, timer.start(b->st));
    bool ok = true;
    for (int64_t i = 0; i < full && ok; ++i) ok = hipGraphLaunch(m->full.exec, b->st) == hipSuccess;
    if (rem && ok) ok = hipGraphLaunch(m->rem.exec, b->st) == hipSuccess;
    if (ms && ok) ok = timer.stop_ms(b->st, ms) == MOD16_OK;
    ok = hipStreamSynchronize(b->st) == hipSuccess && ok;
    if (!ok) {
        m->broken = true;
        return fail(ctx, MOD16_ERR_HIP, "mod16_mcmc_run: a graph launch failed");
    }
    m->steps += steps;
    return MOD16_OK;
}

extern "C" int mod16_mcmc_run(mod16_mcmc* m, int64_t steps, float* ms) {
    if (!m) return MOD16_ERR_ARG;
    MOD16_LOCK(m->b->ctx);
    return mcmc_run(m, steps, ms);
}

static int mcmc_read(mod16_mcmc* m, int64_t t0, int64_t count, double* x, double* y, double* loglik, double* logpost,
                     uint8_t* accepted, double* scaling, double* lamb, int64_t* steps_taken) {
    mod16_ctx* ctx = m->b->ctx;
    if (t0 < 0 || count < 0 || t0 + count > m->steps)
        return fail(ctx, MOD16_ERR_ARG, "mod16_mcmc_read: steps outside those taken");
    HIPCHK(ctx, hipSetDevice(m->b->device));
    hipStream_t st = m->b->st;
    const McmcArgs& a = m->a;
    const size_t nx = (size_t)count * a.chains * a.d, ns = (size_t)count * a.chains;
    const size_t ox = (size_t)t0 * a.chains * a.d, os = (size_t)t0 * a.chains;
    if (count) {
        if (x) HIPCHK(ctx, hipMemcpyAsync(x, a.xtr + ox, nx * 8, hipMemcpyDeviceToHost, st));
        if (y) HIPCHK(ctx, hipMemcpyAsync(y, a.hist + ox, nx * 8, hipMemcpyDeviceToHost, st));
        if (loglik) HIPCHK(ctx, hipMemcpyAsync(loglik, a.tr_ll + os, ns * 8, hipMemcpyDeviceToHost, st));
        if (logpost) HIPCHK(ctx, hipMemcpyAsync(logpost, a.tr_lp + os, ns * 8, hipMemcpyDeviceToHost, st));
        if (accepted) HIPCHK(ctx, hipMemcpyAsync(accepted, a.tr_acc + os, ns, hipMemcpyDeviceToHost, st));
    }
    if (scaling) HIPCHK(ctx, hipMemcpyAsync(scaling, a.scaling, (size_t)a.chains * 8, hipMemcpyDeviceToHost, st));
    if (lamb) HIPCHK(ctx, hipMemcpyAsync(lamb, a.lamb, (size_t)a.chains * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (steps_taken) *steps_taken = m->steps;
    return MOD16_OK;
}

extern "C" int mod16_mcmc_read(mod16_mcmc* m, int64_t t0, int64_t count, double* x, double* y, double* loglik,
                               double* logpost, uint8_t* accepted, double* scaling, double* lamb, int64_t* steps_taken) {
    if (!m) return MOD16_ERR_ARG;
    MOD16_LOCK(m->b->ctx);
    return mcmc_read(m, t0, count, x, y, loglik, logpost, accepted, scaling, lamb, steps_taken);
}
