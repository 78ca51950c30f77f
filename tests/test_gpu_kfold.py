"""k-fold cross-validation on the GPU (MOD16._et_bind(..., folds=...), problem.objective(...,
folds=..., heldout=...), DEMetropolisZ(..., folds=...)): fold objectives against plain problems
whose complementary observations are NaN, the whole-array switch over the admitted rows with a
number observed, every fold's chains against the plain sampler with seed + f, held-out scoring,
plain calls unchanged by labels, and the refusals. Towers as tests/test_gpu_calibration.py builds
them, with a few site-days outside the FAST domain (a pressure below 1 Pa) so that the redo path is
hit. All seeds are fixed; the thresholds were set before the first run."""
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


@pytest.fixture(scope='module')
def m16():
    import mod16_amd
    from mod16_amd import calibration
    return mod16_amd, calibration


def tower(mod16_amd, n, seed=3, planted=6, sigma=SIGMA_OBS):
    from oracle import synth
    _, drv = synth.drivers((1, n), seed=seed, special=False)
    drv = [np.asarray(v, np.float64).ravel().copy() for v in drv]
    rng = np.random.default_rng(seed)
    out = rng.choice(n, planted, replace=False)
    drv[11][out] = 0.5                  # pressure below 1 Pa: outside the FAST domain (reference order)
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    obs = mod16_amd.MOD16._et(pvec, *drv) + rng.normal(0, sigma, n)
    obs[rng.random(n) < 0.05] = np.nan
    w = rng.uniform(0.5, 1.5, n) / sigma
    return drv, obs, w, out


def draws(cal, rng, D):
    base = np.array([P[k] for k in cal.PARAM_NAMES])
    rows = np.repeat(base[None], D, axis=0)
    rows[:, 3] = rng.uniform(1500, 7000, D)        # vpd_close
    rows[:, 4] = rng.uniform(0.01, 0.1, D)         # gl_sh
    rows[:, 9] = rng.uniform(200, 900, D)          # rbl_max
    return rows


def bind(mod16_amd, drv, obs, w, max_draws, **kw):
    return mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=w, max_draws=max_draws, **kw)


def masked(obs, labels, f, heldout):
    '''The observations a plain problem needs to see what fold code (f, heldout) admits.'''
    o = obs.copy()
    o[(labels == f) != heldout] = np.nan
    return o


# ---------------------------------------------------------------- objective
def test_fold_objectives_equal_plain_problems_with_the_complement_masked(m16):
    mod16_amd, cal = m16
    n, K, D = 1500, 4, 40                          # 6 blocks, two rows of 32 draws
    drv, obs, w, out = tower(mod16_amd, n)
    lab = cal.kfold_labels(n, K, seed=1)
    prob = bind(mod16_amd, drv, obs, w, 64, folds=lab)
    assert prob.nfolds == K and np.array_equal(prob.labels, lab)
    assert prob.n_outside_domain == out.size
    rng = np.random.default_rng(5)
    params = draws(cal, rng, D)
    folds = rng.integers(0, K, D)
    for heldout in (False, True):
        sse, cnt = prob.objective(params, folds=folds, heldout=heldout)
        for f in range(K):
            plain = bind(mod16_amd, drv, masked(obs, lab, f, heldout), w, 64)
            s2, c2 = plain.objective(params)
            sel = folds == f
            assert sel.any()
            assert np.array_equal(cnt[sel], c2[sel]), (f, heldout)
            assert np.array_equal(sse[sel], s2[sel]), (f, heldout)
            plain.close()
    # one fold for every draw (an int), and the counts add up to the plain problem's
    s_all, c_all = prob.objective(params)
    for f in range(K):
        _, ct = prob.objective(params, folds=f)
        _, ch = prob.objective(params, folds=f, heldout=True)
        assert np.array_equal(ct + ch, c_all)


def test_switch_ranges_over_the_admitted_rows_with_an_observation(m16):
    """Fold 0 holds the warm site-days; folds 1 and 2 are cold (tmin far below tmin_close: g_surf = 0)
    except two warm rows of fold 1 whose observation is NaN, one of them outside the FAST domain. A
    TRAIN draw of fold 0 and a HELDOUT draw of fold 1 see no g_surf > 0 on an admitted, observed row:
    no transpiration, as _et_batch on the compacted rows -- unlike the NaN-masked problem."""
    mod16_amd, cal = m16
    n = 900
    drv, obs, w, out = tower(mod16_amd, n, seed=8, planted=0)
    lab = np.repeat(np.arange(3), n // 3).astype(np.uint8)
    np.random.default_rng(2).shuffle(lab)
    cold = lab != 0
    drv[8][cold] = 200.0
    f1 = np.flatnonzero(lab == 1)
    warm_nan = f1[:2]
    drv[8][warm_nan] = 295.0
    drv[11][warm_nan[1]] = 0.5
    obs = obs.copy()
    obs[warm_nan] = np.nan
    prob = bind(mod16_amd, drv, obs, w, 8, folds=lab)
    assert prob.n_outside_domain == 1
    params = draws(cal, np.random.default_rng(4), 6)
    L = mod16_amd._lib
    for f, heldout in ((0, False), (1, True), (2, True), (0, True)):
        sse, cnt = prob.objective(params, folds=f, heldout=heldout)
        rows = ((lab == f) == heldout) & ~np.isnan(obs)
        with np.errstate(all='ignore'):
            s_e, c_e = mod16_amd.MOD16._et_batch(params, *[d[rows] for d in drv], observed=obs[rows],
                                                 weights=w[rows], math=L.MATH_FAST)
        assert np.array_equal(cnt, c_e), (f, heldout)
        np.testing.assert_allclose(sse, s_e, rtol=1e-9, atol=0)
        plain = bind(mod16_amd, drv, masked(obs, lab, f, heldout), w, 8)
        s_m, c_m = plain.objective(params)
        assert np.array_equal(c_m, cnt)
        if f != 0 or not heldout:      # the switch is off here, but on for the masked problem
            assert not np.allclose(s_m, sse, rtol=1e-6), (f, heldout)
        else:                          # fold 0 is warm: both have transpiration
            assert np.array_equal(s_m, sse)
        plain.close()


def test_plain_calls_do_not_see_labels(m16):
    mod16_amd, cal = m16
    n = 1200
    drv, obs, w, _ = tower(mod16_amd, n, seed=12)
    lab = cal.kfold_labels(n, 5, seed=3)
    with_l = bind(mod16_amd, drv, obs, w, 48, folds=lab)
    without = bind(mod16_amd, drv, obs, w, 48)
    params = draws(cal, np.random.default_rng(6), 48)
    ref = without.objective(params)
    first = with_l.objective(params)
    with_l.objective(params, folds=np.arange(48) % 5)
    between = with_l.objective(params)
    with_l.objective(params[:20], folds=2, heldout=True)
    last = with_l.objective(params)
    for got in (first, between, last):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # and a fold call after plain calls of another size
    a = with_l.objective(params[:20], folds=2, heldout=True)
    with_l.objective(params[:7])
    b = with_l.objective(params[:20], folds=2, heldout=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- sampler
def test_every_folds_chains_are_the_plain_sampler_of_its_masked_problem(m16):
    mod16_amd, cal = m16
    n, K, chains, seed = 1000, 3, 3, 21
    drv, obs, w, _ = tower(mod16_amd, n, seed=5)
    lab = cal.kfold_labels(n, K, seed=7)
    prob = bind(mod16_amd, drv, obs, w, K * chains, folds=lab)
    kw = dict(chains=chains, tune=40, tune_interval=10, seed=seed, segment=16)
    s = cal.DEMetropolisZ(prob, P, PRIOR3, folds=True, **kw)
    assert s.folds == [0, 1, 2] and s.total_chains == 9
    tr = s.sample(30)                               # 70 steps: 4 graphs of 16 and a remainder of 6
    tr2 = s.sample(11)                              # a second remainder
    assert isinstance(tr, cal.KFoldTrace) and tr.chains == 9
    assert tr.chain_fold.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    for f in range(K):
        plain_prob = bind(mod16_amd, drv, masked(obs, lab, f, False), w, chains)
        p = cal.DEMetropolisZ(plain_prob, P, PRIOR3, **dict(kw, seed=seed + f))
        pt, pt2 = p.sample(30), p.sample(11)
        for got, want in ((tr.fold(f), pt), (tr2.fold(f), pt2)):
            assert type(got) is cal.Trace
            assert np.array_equal(got.accepted, want.accepted), f
            assert np.array_equal(got.log_likelihood, want.log_likelihood), f
            assert np.array_equal(got.log_posterior, want.log_posterior), f
            for name in got.names:
                assert np.array_equal(got.samples[name], want.samples[name]), (f, name)
            assert np.array_equal(got.scaling, want.scaling)
        assert 0 < pt.accepted.sum() < pt.accepted.size
        p.close()
        plain_prob.close()
    # one fold alone is the same chains as inside the full run
    s.close()
    one = cal.DEMetropolisZ(prob, P, PRIOR3, folds=[1], **kw)
    t1 = one.sample(30)
    assert t1.chain_fold.tolist() == [1, 1, 1]
    for name in t1.names:
        assert np.array_equal(t1.fold(1).samples[name], tr.fold(1).samples[name])
    rh = tr.rhat()
    assert sorted(rh) == [0, 1, 2] and sorted(rh[0]) == sorted(tr.names)


def test_heldout_scores_equal_the_objective_and_land_near_the_noise(m16, tmp_path):
    mod16_amd, cal = m16
    n, K, chains = 4000, 4, 3
    drv, obs, _, _ = tower(mod16_amd, n, seed=17, planted=0)     # (no 1e5-size values: RMSD near the noise)
    w = np.full(n, 1.0 / SIGMA_OBS)                 # weighted residuals ~ N(0, 1): RMSD near 1
    prob = bind(mod16_amd, drv, obs, w, 10, folds=K)    # max_draws 10: several launches of mixed folds
    truth = [P[k] for k in PRIOR3]
    # (the gaussian likelihood: -RMSD is too flat to pull the chains off the prior in 260 steps)
    s = cal.DEMetropolisZ(prob, P, PRIOR3, chains=chains, tune=200, tune_interval=50, seed=2,
                          folds=[0, 2, 3], initial=np.array([truth] * chains), objective='gaussian')
    tr = s.sample(60)
    res = s.heldout(tr, burn=10, thin=5)
    assert sorted(res) == [0, 2, 3]
    for f, r in res.items():
        post = tr.fold(f).posterior(10, 5)
        assert r['rmsd'].shape == (chains, 10)
        rows = s.rows(np.stack([post[k] for k in s.names], axis=-1).reshape(-1, s.d))
        sse, cnt = np.concatenate([prob.objective(rows[a:a + 10], folds=f, heldout=True)
                                   for a in range(0, rows.shape[0], 10)], axis=1)
        assert np.array_equal(r['sse'].ravel(), sse) and np.array_equal(r['count'].ravel(), cnt)
        assert (cnt == np.sum((prob.labels == f) & ~np.isnan(obs))).all()
        ms, mc = prob.objective(s.rows(r['mean']), folds=f, heldout=True)
        assert r['mean_rmsd'] == np.sqrt(ms[0] / mc[0])
        assert 0.85 < r['mean_rmsd'] < 1.2, (f, r['mean_rmsd'])
    path = str(tmp_path / 'kfold.npz')
    tr.to_npz(path)
    z = np.load(path)
    assert np.array_equal(z['labels'], prob.labels) and z['chain_fold'].tolist() == [0] * 3 + [2] * 3 + [3] * 3
    ti = z['test_indices']
    assert ti.shape == (K, np.bincount(prob.labels).max()) and ti.dtype == np.int64
    for f in range(K):
        row = ti[f][ti[f] >= 0]
        assert np.array_equal(row, np.flatnonzero(prob.labels == f)) and (ti[f][row.size:] == -1).all()


# ---------------------------------------------------------------- refusals
def test_refusals(m16):
    mod16_amd, cal = m16
    L = mod16_amd._lib
    n = 300
    drv, obs, w, _ = tower(mod16_amd, n, seed=4, planted=0)
    lab = cal.kfold_labels(n, 3)
    for bad in (np.where(lab == 2, 3, lab), lab[:-1], np.zeros(n, np.int64), lab.astype(float), 1, 256):
        with pytest.raises(ValueError):
            bind(mod16_amd, drv, obs, w, 8, folds=bad)
    with pytest.raises(ValueError, match='float64'):
        bind(mod16_amd, drv, obs, w, 8, folds=lab, math=L.MATH_EXACT)
    with pytest.raises(ValueError, match='float64'):
        bind(mod16_amd, [d.astype(np.float32) for d in drv], obs.astype(np.float32), w.astype(np.float32), 8,
             folds=lab)
    prob = bind(mod16_amd, drv, obs, w, 8, folds=lab)
    lib, ctx = prob._ctx.lib, prob._ctx
    lab_c = np.ascontiguousarray(lab)

    def c_refused(status, what):
        assert status == L.ERR_ARG
        assert what in lib.mod16_last_error(ctx.handle).decode()
    c_refused(lib.mod16_static_batch_set_folds(prob._handle, lab_c.ctypes.data, 3), 'already')
    params = draws(cal, np.random.default_rng(1), 4)
    with pytest.raises(ValueError):
        prob.objective(params, folds=3)
    with pytest.raises(ValueError):
        prob.objective(params, folds=[0, 1])
    with pytest.raises(ValueError):
        prob.objective(params, heldout=True)
    code = np.array([0, 1, 2, 3], np.int32)
    sse, cnt = np.zeros(4), np.zeros(4)
    c_refused(lib.mod16_static_batch_objective_folds(prob._handle, params.ctypes.data, 4, code.ctypes.data,
                                                     sse.ctypes.data, cnt.ctypes.data), 'code')
    with pytest.raises(ValueError, match='max_draws'):
        cal.DEMetropolisZ(prob, P, PRIOR3, chains=3, folds=True)         # 9 > 8
    for folds in ([0, 0], [3], []):
        with pytest.raises(ValueError):
            cal.DEMetropolisZ(prob, P, PRIOR3, chains=2, folds=folds)
    # a problem without labels
    plain = bind(mod16_amd, drv, obs, w, 8)
    with pytest.raises(ValueError, match='folds'):
        plain.objective(params, folds=0)
    with pytest.raises(ValueError, match='folds'):
        cal.DEMetropolisZ(plain, P, PRIOR3, chains=2, folds=True)
    spec = L.McmcSpec()
    spec.chains, spec.nfree, spec.index[0], spec.family[0] = 2, 1, 3, L.PRIOR_UNIFORM
    spec.p0[0], spec.p1[0] = 1000.0, 8000.0
    for j, k in enumerate(cal.PARAM_NAMES):
        spec.fixed[j] = P[k]
    spec.lamb, spec.scaling, spec.tune_interval = 1.0, 1e-3, 100
    fold = np.array([0], np.int32)
    out = C.c_void_p()
    c_refused(lib.mod16_mcmc_create_groups(plain._handle, C.byref(spec), 1, fold.ctypes.data, None, C.byref(out)),
              'no folds')
    c_refused(lib.mod16_static_batch_objective_folds(plain._handle, params.ctypes.data, 4, code.ctypes.data,
                                                     sse.ctypes.data, cnt.ctypes.data), 'no folds')
    # labels after a sampler exists
    s = cal.DEMetropolisZ(plain, P, PRIOR3, chains=2)
    c_refused(lib.mod16_static_batch_set_folds(plain._handle, lab_c.ctypes.data, 3), 'sampler')
    s.close()
    # EXACT and float32 problems refuse folds in the library too
    exact = bind(mod16_amd, drv, obs, w, 8, math=L.MATH_EXACT)
    c_refused(lib.mod16_static_batch_set_folds(exact._handle, lab_c.ctypes.data, 3), 'float64')
    f32 = bind(mod16_amd, [d.astype(np.float32) for d in drv], obs.astype(np.float32), w.astype(np.float32), 8)
    c_refused(lib.mod16_static_batch_set_folds(f32._handle, lab_c.ctypes.data, 3), 'float64')
    bad = lab_c.copy()
    bad[0] = 3
    fresh = bind(mod16_amd, drv, obs, w, 8)
    c_refused(lib.mod16_static_batch_set_folds(fresh._handle, bad.ctypes.data, 3), 'label outside')
    c_refused(lib.mod16_static_batch_set_folds(fresh._handle, lab_c.ctypes.data, 4), 'without any pixel')
    c_refused(lib.mod16_static_batch_set_folds(fresh._handle, lab_c.ctypes.data, 1), 'nfolds')
