"""The DE-MCMC-Z sampler on the GPU (mod16_amd.calibration): draw-for-draw parity with a numpy
restatement of the same sampler driven by problem.objective(), segments and interleaved calls,
prior recovery with a constant likelihood, a one-parameter posterior against quadrature, the
stored log-likelihoods against the objective, seeds, and the refusals that need a bound problem.
All seeds are fixed; the thresholds were set before the first run."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = {'tmin_close': -8.0, 'tmin_open': 8.0, 'vpd_open': 650.0, 'vpd_close': 4000.0, 'gl_sh': 0.04,
     'gl_wv': 0.04, 'g_cuticular': 1e-5, 'csl': 0.005, 'rbl_min': 20.0, 'rbl_max': 500.0, 'beta': 250.0}
PRIOR5 = {'vpd_close': {'lower': 1000.0, 'upper': 8000.0},
          'gl_sh': {'mu': -3.45, 'sigma': 0.71},
          'csl': {'mu': -5.5, 'sigma': 0.8},
          'rbl_min': {'lower': 10.0, 'upper': 1000.0, 'c': 10.0},       # c = lower
          'rbl_max': {'lower': 100.0, 'upper': 1000.0, 'c': 1000.0}}    # c = upper
SIGMA_OBS = 5.0


@pytest.fixture(scope='module')
def m16():
    import mod16_amd
    from mod16_amd import calibration
    return mod16_amd, calibration


def tower(mod16_amd, n, seed=3, sigma=SIGMA_OBS):
    from oracle import synth
    _, drv = synth.drivers((1, n), seed=seed, special=False)
    drv = [np.asarray(v, np.float64).ravel() for v in drv]
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    rng = np.random.default_rng(seed)
    obs = mod16_amd.MOD16._et(pvec, *drv) + rng.normal(0, sigma, n)
    obs[rng.random(n) < 0.05] = np.nan
    return drv, obs


def bind(mod16_amd, drv, obs, max_draws, weights=None, **kw):
    w = np.full(obs.shape, 1.0 / SIGMA_OBS) if weights is None else weights
    return mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=w, max_draws=max_draws, **kw)


# ---------------------------------------------------------------- the numpy restatement
def numpy_sampler(cal, problem, prior, fixed_row, chains, tune, tune_interval, draws, tune_target,
                  objective, seed, scaling=1e-3, drop=0.9):
    names = [k for k in cal.PARAM_NAMES if k in prior]
    idx = [cal.PARAM_NAMES.index(k) for k in names]
    fp = [cal.prior_family(prior[k]) for k in names]
    d = len(names)
    lamb0 = 2.38 / math.sqrt(2 * d)

    def evaluate(Y):
        rows = np.repeat(np.asarray(fixed_row, np.float64)[None], chains, axis=0)
        lpr = np.zeros(chains)
        for i in range(d):
            x = cal.x_of_y(fp[i][0], fp[i][1], Y[:, i])
            rows[:, idx[i]] = x
            lpr = lpr + cal.log_prior(fp[i][0], fp[i][1], Y[:, i])
        sse, cnt = problem.objective(rows)
        with np.errstate(invalid='ignore', divide='ignore'):
            ll = -np.sqrt(sse / cnt) if objective == 'rmsd' else -0.5 * sse
        return lpr + ll, ll, rows

    x0 = np.array([cal.support_point(f, p) for f, p in fp])
    Y = np.array([[cal.y_of_x(f, p, x0[i]) for i, (f, p) in enumerate(fp)]] * chains)
    lp, ll, rows = evaluate(Y)
    X = rows[:, idx].copy()
    sc = np.full(chains, scaling)
    lb = np.full(chains, lamb0)
    acc_since = np.zeros(chains, int)
    hist = []
    out = {'x': [], 'll': [], 'lp': [], 'acc': []}
    lo_after = int(math.floor(drop * tune))
    keys = [cal.mix(cal.mix(seed) ^ c) for c in range(chains)]
    r = lambda c, t, k: cal.mix(keys[c] ^ ((t << 6) | k))
    for t in range(tune + draws):
        Yp = np.empty_like(Y)
        for c in range(chains):
            if tune_target and 0 < t < tune and t % tune_interval == 0:
                f = cal.tune_factor(acc_since[c] / float(tune_interval))
                if tune_target == 'scaling':
                    sc[c] = sc[c] * f
                else:
                    lb[c] = lb[c] * f
                acc_since[c] = 0
            eps = np.array([(2.0 * cal.unit(r(c, t, i)) - 1.0) * sc[c] for i in range(d)])
            lo = 0 if t < tune else lo_after
            m = t - lo
            if m >= 2:
                i1 = cal.index(r(c, t, 16), m)
                k = 17
                i2 = cal.index(r(c, t, k), m)
                while i2 == i1 and k < 47:
                    k += 1
                    i2 = cal.index(r(c, t, k), m)
                if i2 == i1:
                    i2 = (i1 + 1) % m
                z1, z2 = hist[lo + i1][c], hist[lo + i2][c]
                Yp[c] = (Y[c] + lb[c] * (z1 - z2)) + eps
            else:
                Yp[c] = Y[c] + eps
        lpn, lln, rowsn = evaluate(Yp)
        acc = np.zeros(chains, bool)
        for c in range(chains):
            mr = lpn[c] - lp[c]
            u = math.log(((r(c, t, 63) >> 11) + 0.5) * 2.0 ** -53)
            if np.isfinite(mr) and u < mr:
                acc[c] = True
                Y[c], lp[c], ll[c], X[c] = Yp[c], lpn[c], lln[c], rowsn[c, idx]
                acc_since[c] += 1
        hist.append(Y.copy())
        if t >= tune:
            out['x'].append(X.copy())
            out['ll'].append(ll.copy())
            out['lp'].append(lp.copy())
            out['acc'].append(acc)
    res = {k: np.array(v) for k, v in out.items()}
    res['scaling'], res['lamb'] = sc, lb
    res['names'] = names
    return res


def fixed_row_of(cal, prior, fixed=None):
    row = np.array([P[k] for k in cal.PARAM_NAMES])
    for k, v in (fixed or {}).items():
        row[cal.PARAM_NAMES.index(k)] = v
    return row


# ---------------------------------------------------------------- 1. restatement parity
@pytest.mark.parametrize('tune_target', ['scaling', 'lambda'])
@pytest.mark.parametrize('objective', ['rmsd', 'gaussian'])
def test_chains_match_the_numpy_restatement(m16, tune_target, objective):
    mod16_amd, cal = m16
    drv, obs = tower(mod16_amd, 400)
    problem = bind(mod16_amd, drv, obs, 4)
    s = cal.DEMetropolisZ(problem, P, PRIOR5, chains=4, tune=300, tune_interval=50,
                          tune_target=tune_target, objective=objective, seed=11)
    tr = s.sample(300)
    ref = numpy_sampler(cal, problem, PRIOR5, fixed_row_of(cal, PRIOR5), 4, 300, 50, 300,
                        tune_target, objective, 11)
    assert tr.names == ref['names']
    assert np.array_equal(tr.accepted, ref['acc'].T)
    assert 0 < tr.accepted.sum() < tr.accepted.size
    for i, name in enumerate(tr.names):
        np.testing.assert_allclose(tr.samples[name], ref['x'][:, :, i].T, rtol=1e-12, atol=0)
    np.testing.assert_allclose(tr.log_posterior, ref['lp'].T, rtol=1e-12, atol=0)
    assert np.array_equal(tr.scaling, ref['scaling'])
    assert np.array_equal(tr.lamb, ref['lamb'])
    s.close()


# ---------------------------------------------------------------- 2. segments and interleaving
def _bits(tr):
    return [tr.log_likelihood, tr.log_posterior, tr.accepted, tr.scaling, tr.lamb] + \
           [tr.samples[k] for k in tr.names]


def test_segments_and_interleaved_objective_calls_change_nothing(m16):
    mod16_amd, cal = m16
    drv, obs = tower(mod16_amd, 400)
    problem = bind(mod16_amd, drv, obs, 256)
    rows = np.repeat(np.array([P[k] for k in cal.PARAM_NAMES])[None], 256, axis=0)
    problem.objective(rows[:4])
    kw = dict(chains=4, tune=100, tune_interval=25, seed=5, segment=16)
    a = cal.DEMetropolisZ(problem, P, PRIOR5, **kw)
    a1 = a.sample(150)
    problem.objective(rows)              # more draws: the problem regrows its own workspace
    a2 = a.sample(150)
    b = cal.DEMetropolisZ(problem, P, PRIOR5, **kw).sample(300)
    for x, y, z in zip(_bits(a1), _bits(a2), _bits(b)):
        if x.ndim == 2:
            assert np.array_equal(np.concatenate([x, y], axis=1), z)
    for y, z in zip(_bits(a2)[3:5], _bits(b)[3:5]):
        assert np.array_equal(y, z)


# ---------------------------------------------------------------- 3. prior recovery
def test_constant_likelihood_recovers_the_prior(m16):
    mod16_amd, cal = m16
    from scipy import stats
    drv, obs = tower(mod16_amd, 200)
    problem = bind(mod16_amd, drv, obs, 2048, weights=np.zeros(obs.shape))
    prior = dict(PRIOR5, beta={'lower': 0.0, 'upper': 1000.0})
    s = cal.DEMetropolisZ(problem, P, prior, chains=2048, tune=1000, seed=2)
    tr = s.sample(1000)
    assert np.all(tr.log_likelihood == 0.0)
    dists = {'vpd_close': stats.uniform(1000.0, 7000.0), 'beta': stats.uniform(0.0, 1000.0),
             'gl_sh': stats.lognorm(s=0.71, scale=math.exp(-3.45)),
             'csl': stats.lognorm(s=0.8, scale=math.exp(-5.5)),
             'rbl_min': stats.triang(c=0.0, loc=10.0, scale=990.0),
             'rbl_max': stats.triang(c=1.0, loc=100.0, scale=900.0)}
    for name, dist in dists.items():
        last = tr.samples[name][:, -1]
        p = stats.kstest(last, dist.cdf).pvalue
        assert p > 1e-3, (name, p)
    s.close()


# ---------------------------------------------------------------- 4. posterior against quadrature
def test_one_parameter_posterior_matches_quadrature(m16):
    mod16_amd, cal = m16
    from scipy import stats
    drv, obs = tower(mod16_amd, 60, seed=9, sigma=20.0)
    problem = bind(mod16_amd, drv, obs, 1024, weights=np.full(obs.shape, 1.0 / 20.0))
    prior = {'csl': {'mu': -5.5, 'sigma': 0.8}}
    fam, pp = cal.prior_family(prior['csl'])
    row = np.array([P[k] for k in cal.PARAM_NAMES])
    j = cal.PARAM_NAMES.index('csl')

    def logpost(y):
        out = np.empty(y.size)
        for k0 in range(0, y.size, problem.max_draws):
            yy = y[k0:k0 + problem.max_draws]
            rows = np.repeat(row[None], yy.size, axis=0)
            rows[:, j] = cal.x_of_y(fam, pp, yy)
            sse, _ = problem.objective(rows)
            out[k0:k0 + yy.size] = cal.log_prior(fam, pp, yy) - 0.5 * sse
        return out

    coarse = np.linspace(pp[0] - 6 * pp[1], pp[0] + 6 * pp[1], 4001)
    lc = logpost(coarse)
    keep = coarse[lc > lc.max() - 60.0]
    step = coarse[1] - coarse[0]
    grid = np.linspace(keep.min() - 2 * step, keep.max() + 2 * step, 4001)
    lg = logpost(grid)
    dens = np.exp(lg - lg.max())
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(grid))])
    cdf /= cdf[-1]
    trap = lambda f: float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(grid)))
    mass = dens / trap(dens)
    xg = np.exp(grid)
    mean_x = trap(mass * xg)
    sd_x = math.sqrt(trap(mass * (xg - mean_x) ** 2))
    s = cal.DEMetropolisZ(problem, P, prior, chains=1024, tune=1000, objective='gaussian', seed=4)
    last = s.sample(1000).samples['csl'][:, -1]
    se = sd_x / math.sqrt(last.size)
    assert abs(last.mean() - mean_x) < 4 * se, (last.mean(), mean_x, se)
    p = stats.kstest(np.log(last), lambda v: np.interp(v, grid, cdf)).pvalue
    assert p > 1e-3, p
    s.close()


# ---------------------------------------------------------------- 5. fixed values, stored likelihoods
def test_stored_log_likelihood_is_the_objective_of_the_stored_rows(m16):
    mod16_amd, cal = m16
    drv, obs = tower(mod16_amd, 400)
    problem = bind(mod16_amd, drv, obs, 8)
    fixed = {'beta': 300.0, 'gl_wv': 0.03}
    s = cal.DEMetropolisZ(problem, P, PRIOR5, fixed=fixed, chains=8, tune=200, seed=21)
    tr = s.sample(200)
    row = fixed_row_of(cal, PRIOR5, fixed)
    for k in (0, 57, 199):
        rows = np.repeat(row[None], 8, axis=0)
        for name in tr.names:
            rows[:, cal.PARAM_NAMES.index(name)] = tr.samples[name][:, k]
        sse, cnt = problem.objective(rows)
        assert np.array_equal(tr.log_likelihood[:, k], -np.sqrt(sse / cnt))
    # the free x-values inside their supports; fixed parameters are not in the trace
    assert set(tr.names) == set(PRIOR5)
    assert np.all((tr.samples['vpd_close'] > 1000) & (tr.samples['vpd_close'] < 8000))
    assert np.all((tr.samples['rbl_min'] >= 10) & (tr.samples['rbl_min'] <= 1000))
    assert np.all(tr.samples['csl'] > 0)
    assert np.all(np.isfinite(tr.log_posterior)) and tr.rhat().keys() == set(PRIOR5)
    s.close()


# ---------------------------------------------------------------- 6. seeds
def test_seeds(m16):
    mod16_amd, cal = m16
    drv, obs = tower(mod16_amd, 400)
    problem = bind(mod16_amd, drv, obs, 4)
    run = lambda seed: cal.DEMetropolisZ(problem, P, PRIOR5, chains=4, tune=100, seed=seed).sample(100)
    a, b, c = run(8), run(8), run(9)
    for x, y in zip(_bits(a), _bits(b)):
        assert np.array_equal(x, y)
    assert not np.array_equal(a.samples['csl'], c.samples['csl'])
    # the chains of one run differ from each other
    assert not np.array_equal(a.samples['csl'][0], a.samples['csl'][1])


# ---------------------------------------------------------------- 7. refusals
def test_refusals_that_need_a_bound_problem(m16):
    mod16_amd, cal = m16
    from mod16_amd import _lib
    drv, obs = tower(mod16_amd, 200)
    exact = bind(mod16_amd, drv, obs, 4, math=_lib.MATH_EXACT)
    with pytest.raises(ValueError, match='MATH_FAST'):
        cal.DEMetropolisZ(exact, P, PRIOR5, chains=4)
    f32 = mod16_amd.MOD16._et_bind(*[v.astype(np.float32) for v in drv], observed=obs.astype(np.float32),
                                   max_draws=4)
    with pytest.raises(ValueError, match='float64'):
        cal.DEMetropolisZ(f32, P, PRIOR5, chains=4)
    good = bind(mod16_amd, drv, obs, 4)
    with pytest.raises(ValueError, match='max_draws'):
        cal.DEMetropolisZ(good, P, PRIOR5, chains=5)
    # the C entry point refuses the same on its own
    spec = _lib.McmcSpec()
    spec.chains, spec.nfree = 4, 1
    spec.index[0], spec.family[0], spec.p0[0], spec.p1[0] = 7, _lib.PRIOR_LOGNORMAL, -5.5, 0.8
    for j, k in enumerate(cal.PARAM_NAMES):
        spec.fixed[j] = P[k]
    spec.lamb, spec.scaling, spec.tune_interval = 1.0, 1e-3, 100
    h = C.c_void_p()
    lib = good._ctx.lib
    for prob in (exact, f32):
        assert lib.mod16_mcmc_create(prob._handle, C.byref(spec), None, C.byref(h)) == _lib.ERR_ARG
        assert not h.value
    spec.chains = 5
    assert lib.mod16_mcmc_create(good._handle, C.byref(spec), None, C.byref(h)) == _lib.ERR_ARG
    # a non-finite initial log posterior (no observation is a number: count = 0)
    nan_obs = bind(mod16_amd, drv, np.full(obs.shape, np.nan), 4)
    with pytest.raises(ValueError, match='not finite'):
        cal.DEMetropolisZ(nan_obs, P, PRIOR5, chains=4)
