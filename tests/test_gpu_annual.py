"""The annual-precipitation constraint on the GPU (MOD16._et_bind(..., annual_precip=...),
problem.penalty / objective(..., penalty=True), DEMetropolisZ(..., constraints=...)): the device
penalty against the numpy restatement on the problem's own rows and on EXACT rows, (sse, count)
against an unconstrained problem, NaN and never-binding limits, identical bits between launches, the
constrained sampler, and the refusals of the C entry points. Towers of T = 3 x 365 days x N = 7
sites from oracle.synth, the days of the three years (labelled 2004, 2001, 2009) shuffled, so no
site-year is a multiple of 64 days or contiguous; six site-days lie outside the FAST domain (a
pressure below 1 Pa). All seeds are fixed; the thresholds were set before the first run."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = {'tmin_close': -8.0, 'tmin_open': 8.0, 'vpd_open': 650.0, 'vpd_close': 4000.0, 'gl_sh': 0.04,
     'gl_wv': 0.04, 'g_cuticular': 1e-5, 'csl': 0.005, 'rbl_min': 20.0, 'rbl_max': 500.0, 'beta': 250.0}
PRIOR3 = {'vpd_close': {'lower': 1000.0, 'upper': 8000.0},
          'gl_sh': {'mu': -3.45, 'sigma': 0.71},
          'rbl_max': {'lower': 100.0, 'upper': 1000.0, 'c': 1000.0}}
SIGMA_OBS = 5.0
T, N = 3 * 365, 7


@pytest.fixture(scope='module')
def m16():
    import mod16_amd
    from mod16_amd import calibration
    return mod16_amd, calibration


def tower(mod16_amd, seed=3, planted=6):
    """(drivers (T, N) each, observed, weights, years, lhv, the planted parameters' annual totals (Y, N))"""
    from oracle import synth
    _, drv = synth.drivers((T, N), seed=seed, special=False)
    drv = [np.broadcast_to(np.asarray(v, np.float64), (T, N)).copy() for v in drv]
    rng = np.random.default_rng(seed)
    out = rng.choice(T * N, planted, replace=False)
    drv[11].reshape(-1)[out] = 0.5          # pressure below 1 Pa: outside the FAST domain (reference order)
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    le = mod16_amd.MOD16._et(pvec, *drv)
    obs = le + rng.normal(0, SIGMA_OBS, (T, N))
    obs[rng.random((T, N)) < 0.05] = np.nan
    w = rng.uniform(0.5, 1.5, (T, N)) / SIGMA_OBS
    years = rng.permutation(np.repeat([2004, 2001, 2009], 365))
    lhv = mod16_amd.latent_heat_vaporization((drv[5] + drv[6]) / 2)
    mass = np.maximum(le * 86400.0 / lhv, 0.0)
    tot = np.stack([mass[years == y].sum(axis=0) for y in np.unique(years)])
    return drv, obs, w, years, lhv, tot


def binding_limits(tot, seed=11):
    return np.random.default_rng(seed).uniform(0.6, 0.9, tot.shape) * tot


def draws(cal, rng, D):
    base = np.array([P[k] for k in cal.PARAM_NAMES])
    rows = np.repeat(base[None], D, axis=0)
    rows[:, 3] = rng.uniform(1500, 7000, D)        # vpd_close
    rows[:, 4] = rng.uniform(0.01, 0.1, D)         # gl_sh
    rows[:, 9] = rng.uniform(200, 900, D)          # rbl_max
    return rows


def bind(mod16_amd, drv, obs, w, max_draws, **kw):
    return mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=w, max_draws=max_draws, **kw)


# ---------------------------------------------------------------- 3. the penalty
def test_penalty_matches_the_restatement_on_the_rows(m16):
    """rtol 1e-9 against the restatement on problem.rows(): the same FAST bits per pixel, only the
    order of the sums and the form of the division (le x (86400 / lhv)) differ -- the tolerance the
    project uses for such sums. Against EXACT rows rtol 1e-7: 1e-9 per pixel x the cancellation of
    the clipped difference (<= 10, asserted below on the reference values) x 2 for the square, with
    margin."""
    mod16_amd, cal = m16
    from mod16_amd import _lib
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    limit = binding_limits(tot)
    prob = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, limit))
    assert prob.has_annual and prob.n == T * N and prob.shape == (T, N) and prob.n_outside_domain == 6
    n_info = C.c_int64(0)
    prob._ctx.check(prob._ctx.lib.mod16_static_batch_info(prob._handle, C.byref(n_info), None, None))
    assert n_info.value == T * N
    np.testing.assert_array_equal(prob.lhv, lhv)
    params = draws(cal, np.random.default_rng(5), 40)
    rows = prob.rows(params)
    assert rows.shape == (40, T, N)
    ref = cal.annual_precip_penalty(rows, years, lhv, limit)
    # the inputs: most site-years bind, and the summed clipped differences cancel by less than 10
    mass = np.maximum(rows * 86400.0 / lhv, 0.0)
    tots = np.stack([mass[:, years == y].sum(axis=1) for y in np.unique(years)], axis=1)
    over = np.maximum(tots - limit, 0.0)
    assert ((over > 0).mean(axis=(1, 2)) > 0.5).all() and (ref < 0).all()
    assert ((over * tots).sum(axis=(1, 2)) / (over ** 2).sum(axis=(1, 2)) <= 10.0).all()
    pen = prob.penalty(params)
    print('penalty: max relative difference to the restatement on the rows', np.abs(pen / ref - 1).max())
    np.testing.assert_allclose(pen, ref, rtol=1e-9, atol=0)
    exact = mod16_amd.MOD16._et_batch(params, *drv, math=_lib.MATH_EXACT)
    ref_exact = cal.annual_precip_penalty(exact, years, lhv, limit)
    print('penalty: max relative difference to the restatement on EXACT rows', np.abs(pen / ref_exact - 1).max())
    np.testing.assert_allclose(pen, ref_exact, rtol=1e-7, atol=0)
    # the rows are the caller's, in the caller's order: those of a problem without the constraint
    plain = bind(mod16_amd, drv, obs, w, 64)
    assert np.array_equal(rows, plain.rows(params), equal_nan=True)
    day, night = prob.rows(params[:3], separate=True)
    day0, night0 = plain.rows(params[:3], separate=True)
    assert np.array_equal(day, day0, equal_nan=True) and np.array_equal(night, night0, equal_nan=True)
    # fewer draws than a row of 32, and one
    np.testing.assert_allclose(prob.penalty(params[:5]), ref[:5], rtol=1e-9, atol=0)
    np.testing.assert_allclose(prob.penalty(params[7:8]), ref[7:8], rtol=1e-9, atol=0)
    plain.close()
    prob.close()


# ---------------------------------------------------------------- 4. sse, count
def test_sse_and_count_are_those_of_the_unconstrained_problem(m16):
    mod16_amd, cal = m16
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    prob = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, binding_limits(tot)))
    plain = bind(mod16_amd, drv, obs, w, 64)
    params = draws(cal, np.random.default_rng(6), 40)
    s0, c0 = plain.objective(params)
    s1, c1, pen = prob.objective(params, penalty=True)
    s2, c2 = prob.objective(params)
    assert np.array_equal(c1, c0) and np.array_equal(c2, c0) and c0.min() > 0.9 * T * N
    np.testing.assert_allclose(s1, s0, rtol=1e-9, atol=0)
    np.testing.assert_allclose(s2, s0, rtol=1e-9, atol=0)
    assert np.array_equal(s1, s2)                   # the same reduction in both instances
    assert np.array_equal(pen, prob.penalty(params))
    # interleaved plain and constrained calls keep a graph each
    s3, c3, pen3 = prob.objective(params, penalty=True)
    assert np.array_equal(s3, s1) and np.array_equal(c3, c1) and np.array_equal(pen3, pen)
    with pytest.raises(ValueError, match='annual_precip'):
        plain.objective(params, penalty=True)
    plain.close()
    prob.close()


# ---------------------------------------------------------------- 5. NaN, limits that never bind
def test_nan_driver_and_limits_that_never_bind(m16):
    mod16_amd, cal = m16
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    params = draws(cal, np.random.default_rng(7), 40)
    loose = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, np.full(tot.shape, 1e12)))
    pen = loose.penalty(params)
    assert np.all(pen == 0.0)
    loose.close()
    drv[9][400, 2] = np.nan                         # vpd_day of one day of one site
    prob = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, binding_limits(tot)))
    plain = bind(mod16_amd, drv, obs, w, 64)
    s0, c0 = plain.objective(params)
    s1, c1, pen = prob.objective(params, penalty=True)
    assert np.isnan(pen).all()
    assert np.array_equal(c1, c0)
    np.testing.assert_allclose(s1, s0, rtol=1e-9, atol=0)
    assert np.isnan(cal.annual_precip_penalty(prob.rows(params[:2]), years, prob.lhv, prob.annual_precip)).all()
    plain.close()
    prob.close()


# ---------------------------------------------------------------- 6. the same bits on every launch
def test_two_launches_return_identical_bits(m16):
    mod16_amd, cal = m16
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    prob = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, binding_limits(tot)))
    params = draws(cal, np.random.default_rng(8), 40)
    a = prob.objective(params, penalty=True)
    b = prob.objective(params, penalty=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    again = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, binding_limits(tot)))
    for x, y in zip(a, again.objective(params, penalty=True)):
        assert x.tobytes() == y.tobytes()
    again.close()
    prob.close()


# ---------------------------------------------------------------- 7. the sampler
def _bits(tr):
    return [tr.log_likelihood, tr.log_posterior, tr.accepted, tr.scaling, tr.lamb] + \
        [tr.samples[k] for k in tr.names]


def test_sampler_with_limits_that_never_bind_is_the_plain_sampler(m16):
    mod16_amd, cal = m16
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    prob = bind(mod16_amd, drv, obs, w, 8, annual_precip=(years, np.full(tot.shape, 1e12)))
    run = lambda c: cal.DEMetropolisZ(prob, P, PRIOR3, chains=4, tune=150, seed=31, constraints=c).sample(150)
    a, b = run(True), run(None)
    assert a.accepted.any()
    for x, y in zip(_bits(a), _bits(b)):
        assert x.tobytes() == y.tobytes()
    prob.close()


def test_constrained_sampler(m16):
    mod16_amd, cal = m16
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    prob = bind(mod16_amd, drv, obs, w, 64, annual_precip=(years, binding_limits(tot)))
    con = cal.DEMetropolisZ(prob, P, PRIOR3, chains=4, tune=500, seed=17, constraints=('annual_precipitation',))
    assert con.constraints == ('annual_precipitation',)
    tr = con.sample(1500)
    # (b) the stored log-likelihood is the objective of the stored rows plus their penalty: bit for
    # bit, as tests/test_gpu_calibration.py holds the plain sampler to -sqrt(sse / count)
    for k in (0, 57, 1499):
        rows = con.rows(np.stack([tr.samples[name][:, k] for name in tr.names], axis=-1))
        sse, cnt, pen = prob.objective(rows, penalty=True)
        assert np.array_equal(tr.log_likelihood[:, k], -np.sqrt(sse / cnt) + pen)
    assert np.all(np.isfinite(tr.log_posterior)) and tr.accepted.any()
    # (c) the constraint pulls the chains toward parameters that evaporate less than the limits
    free = cal.DEMetropolisZ(prob, P, PRIOR3, chains=4, tune=500, seed=17)
    assert free.constraints == ()
    tr0 = free.sample(1500)
    pen_con, pen_free = con.penalty(tr), free.penalty(tr0)
    assert pen_con.shape == pen_free.shape == (4, 1500)
    assert np.array_equal(con.penalty(tr, burn=1000, thin=7), pen_con[:, 1000::7])
    print('mean penalty: constrained', pen_con.mean(), 'unconstrained', pen_free.mean())
    assert pen_free.mean() < pen_con.mean() <= 0.0
    con.close()
    free.close()
    prob.close()


def test_initial_point_with_a_nan_penalty_is_refused(m16):
    mod16_amd, cal = m16
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    drv[9][400, 2] = np.nan
    prob = bind(mod16_amd, drv, obs, w, 8, annual_precip=(years, binding_limits(tot)))
    with pytest.raises(ValueError, match='not finite'):
        cal.DEMetropolisZ(prob, P, PRIOR3, chains=4, constraints=True)
    s = cal.DEMetropolisZ(prob, P, PRIOR3, chains=4, tune=10)      # without the constraint the same point is fine
    s.close()
    prob.close()


# ---------------------------------------------------------------- 8. refusals of the C entry points
def test_c_level_refusals(m16):
    mod16_amd, cal = m16
    import torch
    from mod16_amd import _lib
    drv, obs, w, years, lhv, tot = tower(mod16_amd)
    limit = np.ascontiguousarray(binding_limits(tot))
    index = np.ascontiguousarray(np.unique(years, return_inverse=True)[1].reshape(T), np.int32)
    lhv = np.ascontiguousarray(lhv)

    def set_annual(prob, t=T, n=N, index=index, limit=limit, lhv=lhv):
        status = prob._ctx.lib.mod16_static_batch_set_annual(prob._handle, t, n, index.ctypes.data, limit.shape[0],
                                                             limit.ctypes.data, lhv.ctypes.data)
        return status, prob._ctx.lib.mod16_last_error(prob._ctx.handle).decode()

    def refused(result, word):
        status, message = result
        assert status == _lib.ERR_ARG and word in message, (status, message)

    plain = bind(mod16_amd, drv, obs, w, 8)
    lib = plain._ctx.lib
    # arguments that do not fit
    refused(set_annual(plain, t=T - 1), 'T x N')
    refused(set_annual(plain, index=np.where(index == 2, 1, index).astype(np.int32)), 'year without')
    refused(set_annual(plain, index=np.where(index == 2, 3, index).astype(np.int32)), 'year index')
    refused(set_annual(plain, limit=np.where(np.eye(3, N) > 0, np.nan, limit)), 'finite')
    refused(set_annual(plain, limit=-limit), 'sum')
    refused(set_annual(plain, lhv=np.where(np.eye(T, N) > 0, 0.0, lhv)), 'lhv')
    # the constraints bit on a problem without the constraint
    spec = _lib.McmcSpec()
    spec.chains, spec.nfree = 4, 1
    spec.index[0], spec.family[0], spec.p0[0], spec.p1[0] = 4, _lib.PRIOR_LOGNORMAL, -3.45, 0.71
    for j, k in enumerate(cal.PARAM_NAMES):
        spec.fixed[j] = P[k]
    spec.lamb, spec.scaling, spec.tune_interval = 1.0, 1e-3, 100
    spec.constraints = _lib.CONSTRAINT_ANNUAL_PRECIP
    h = C.c_void_p()
    refused((lib.mod16_mcmc_create(plain._handle, C.byref(spec), None, C.byref(h)),
             lib.mod16_last_error(plain._ctx.handle).decode()), 'constraint')
    assert not h.value
    spec.constraints = 2
    refused((lib.mod16_mcmc_create(plain._handle, C.byref(spec), None, C.byref(h)),
             lib.mod16_last_error(plain._ctx.handle).decode()), 'unknown bits')
    pen = np.zeros(4)
    refused((lib.mod16_static_batch_objective_annual(plain._handle, pen.ctypes.data, 0, pen.ctypes.data, pen.ctypes.data,
                                                     pen.ctypes.data),
             lib.mod16_last_error(plain._ctx.handle).decode()), 'no constraint')
    # after a sampler exists
    s = cal.DEMetropolisZ(plain, P, PRIOR3, chains=4, tune=10)
    refused(set_annual(plain), 'sampler')
    s.close()
    # twice
    assert set_annual(plain)[0] == 0
    refused(set_annual(plain), 'already')
    sse, cnt = plain.objective(draws(cal, np.random.default_rng(1), 3))       # the problem works after all that
    assert np.all(cnt > 0) and np.all(np.isfinite(sse))
    plain.close()
    # a problem with folds, and folds on a problem with the constraint
    folded = bind(mod16_amd, drv, obs, w, 8, folds=3)
    refused(set_annual(folded), 'folds')
    folded.close()
    con = bind(mod16_amd, drv, obs, w, 8, annual_precip=(years, limit))
    labels = np.ascontiguousarray(np.arange(T * N) % 3, np.uint8)
    refused((lib.mod16_static_batch_set_folds(con._handle, labels.ctypes.data, 3),
             lib.mod16_last_error(con._ctx.handle).decode()), 'constraint')
    con.close()
    # float32 and EXACT problems
    f32 = mod16_amd.MOD16._et_bind(*[v.astype(np.float32) for v in drv], observed=obs.astype(np.float32), max_draws=8)
    refused(set_annual(f32), 'float64')
    f32.close()
    exact = bind(mod16_amd, drv, obs, w, 8, math=_lib.MATH_EXACT)
    refused(set_annual(exact), 'MOD16_MATH_FAST')
    exact.close()
    # a DEVICE bind: the caller's arrays are not the library's to lay out anew
    dev = [torch.from_numpy(np.ascontiguousarray(v).reshape(-1)).cuda() for v in drv + [obs, w]]
    torch.cuda.synchronize()
    handle = C.c_void_p()
    ctx = _lib.context(0)
    ctx.check(lib.mod16_static_batch_bind_f64(ctx.handle, _lib.ptr_array([d.data_ptr() for d in dev[:14]]),
                                              _lib.i64_array([1] * 14), T * N, dev[14].data_ptr(), dev[15].data_ptr(),
                                              8, _lib.MATH_FAST, _lib.DEVICE, C.byref(handle)))
    status = lib.mod16_static_batch_set_annual(handle, T, N, index.ctypes.data, 3, limit.ctypes.data, lhv.ctypes.data)
    message = lib.mod16_last_error(ctx.handle).decode()
    lib.mod16_static_batch_destroy(handle)
    assert status == _lib.ERR_ARG and 'HOST' in message, (status, message)
