"""The Sobol sensitivity analysis on the GPU (mod16_amd.sensitivity): the device sample is scipy's
unscrambled Sobol sequence in the Saltelli layout bit for bit, the fused rows kernel is
MOD16._et row by row, the indices and their bootstrap are the arithmetic stated in
mod16_amd/csrc/mod16_sobol.hpp, and the parameters mode scores rows as MOD16._et_batch does."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import mod16_oracle as oracle

pytestmark = pytest.mark.gpu

BOUNDS = json.load(open(os.path.join(GOLDEN, 'sensitivity_bounds.json')))
DRIVERS = BOUNDS['drivers']
PARAMS = BOUNDS['parameters']
# MOD16 Collection 6.1-like parameters (the reference's drivers mode uses the BPLUT's mean)
P = dict(tmin_close=-8.0, tmin_open=8.0, vpd_open=650.0, vpd_close=3000.0, gl_sh=0.01, gl_wv=0.01,
         g_cuticular=1e-5, csl=2.4e-3, rbl_min=60.0, rbl_max=90.0, beta=250.0)


@pytest.fixture(scope='module')
def m16():
    import mod16_amd
    from mod16_amd import sensitivity
    return mod16_amd, sensitivity


def np_saltelli(bounds, n, second_order=True, skip=0):
    from scipy.stats import qmc
    lo = np.array([b[0] for b in bounds.values()], np.float64)
    hi = np.array([b[1] for b in bounds.values()], np.float64)
    d = lo.size
    eng = qmc.Sobol(2 * d, scramble=False, bits=32)
    if skip:
        eng.fast_forward(skip)
    u = eng.random(n)
    A = lo + (hi - lo) * u[:, :d]
    B = lo + (hi - lo) * u[:, d:]
    R = 2 * d + 2 if second_order else d + 2
    out = np.empty((n, R, d))
    out[:, 0] = A
    for i in range(d):
        out[:, 1 + i] = A
        out[:, 1 + i, i] = B[:, i]
        if second_order:
            out[:, 1 + d + i] = B
            out[:, 1 + d + i, i] = A[:, i]
    out[:, R - 1] = B
    return out.reshape(n * R, d)


def np_indices(Y, d, second_order=True, normalize=True, rows=None):
    """The header's arithmetic in numpy; `rows` = base samples to use (a bootstrap draw)."""
    R = 2 * d + 2 if second_order else d + 2
    Y = np.asarray(Y, np.float64).reshape(-1, R)
    if normalize:
        Y = (Y - Y.mean()) / Y.std()
    if rows is not None:
        Y = Y[rows]
    fA, fB = Y[:, 0], Y[:, R - 1]
    V = np.var(np.concatenate([fA, fB]))
    S1 = np.array([np.mean(fB * (Y[:, 1 + i] - fA)) / V for i in range(d)])
    ST = np.array([0.5 * np.mean((fA - Y[:, 1 + i]) ** 2) / V for i in range(d)])
    S2 = np.full((d, d), np.nan)
    if second_order:
        for j in range(d):
            for k in range(j + 1, d):
                S2[j, k] = np.mean(Y[:, 1 + d + j] * Y[:, 1 + k] - fA * fB) / V - S1[j] - S1[k]
    return S1, ST, S2


def mix(z):
    z = np.asarray(z, np.uint64)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def np_draws(seed, r, n):
    k = np.arange(n, dtype=np.uint64)
    with np.errstate(over='ignore'):
        return (mix(mix(np.uint64(seed)) ^ ((np.uint64(r) << np.uint64(32)) | k)) & np.uint64(n - 1)).astype(np.int64)


def ishigami(X):
    a, b = 7.0, 0.1
    return np.sin(X[:, 0]) + a * np.sin(X[:, 1]) ** 2 + b * X[:, 2] ** 4 * np.sin(X[:, 0])


# ---------------------------------------------------------------- 1. the sample
@pytest.mark.parametrize('d', [3, 11, 14])
@pytest.mark.parametrize('skip', [0, 1024])
@pytest.mark.parametrize('second_order', [True, False])
def test_sample_is_scipys_sequence_in_saltelli_layout(m16, d, skip, second_order):
    _, sens = m16
    names = list(DRIVERS)[:d] if d <= 14 else None
    bounds = {k: DRIVERS[k] for k in names}
    got = sens.saltelli_sample(bounds, 256, second_order=second_order, skip=skip)
    want = np_saltelli(bounds, 256, second_order, skip)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 2. the rows kernel
def _rows_case(m16, bounds, fixed, n=256):
    mod16_amd, sens = m16
    res, Y = sens.sobol_drivers(P, bounds, n=n, fixed=fixed, resamples=10, return_outputs=True)
    X = sens.saltelli_sample(bounds, n)
    full = np.empty((X.shape[0], 14))
    for c, name in enumerate(mod16_amd.DRIVER_NAMES):
        full[:, c] = X[:, list(bounds).index(name)] if name in bounds else fixed[name]
    return Y, full


def test_rows_equal_the_oracle_and_the_gpu_et_row_by_row(m16):
    mod16_amd, _ = m16
    Y, full = _rows_case(m16, DRIVERS, None)
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    want = np.array([oracle.et_static(pvec, *row) for row in full])
    assert np.array_equal(np.isnan(Y), np.isnan(want))
    ok = np.isfinite(want)
    assert np.max(np.abs(Y[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))) < 1e-11
    # 200 rows bit for bit against MOD16._et on the GPU, both branches of the g_surf switch
    rc = oracle.r_correction(full[:, 11], full[:, 5])
    gs = np.array([oracle.surface_conductance(P, row[8], row[9]) for row in full]) / rc
    on, off = np.flatnonzero(gs > 0), np.flatnonzero(~(gs > 0))
    assert on.size and off.size
    pick = np.concatenate([on[:100], off[:100]])
    for w in pick:
        assert np.array_equal(Y[w], mod16_amd.MOD16._et(pvec, *full[w]), equal_nan=True), w


def test_rows_with_a_driver_subset_and_the_others_fixed(m16):
    mod16_amd, _ = m16
    bounds = {k: DRIVERS[k] for k in ('vpd_day', 'lai', 'tmin')}
    fixed = {k: 0.5 * (lo + hi) for k, (lo, hi) in DRIVERS.items() if k not in bounds}
    Y, full = _rows_case(m16, bounds, fixed)
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    want = np.array([oracle.et_static(pvec, *row) for row in full])
    ok = np.isfinite(want)
    assert np.max(np.abs(Y[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))) < 1e-11
    for w in range(0, full.shape[0], max(1, full.shape[0] // 200)):
        assert np.array_equal(Y[w], mod16_amd.MOD16._et(pvec, *full[w]), equal_nan=True), w


# ---------------------------------------------------------------- 3. the indices
def _y(m16, d, n, second_order=True, seed=3):
    _, sens = m16
    bounds = {'x%d' % k: (-np.pi, np.pi) for k in range(d)}
    X = sens.saltelli_sample(bounds, n, second_order=second_order)
    rng = np.random.default_rng(seed)
    w = rng.random(d) * 3
    return 50.0 + X @ w + np.sin(X[:, 0]) * X[:, -1] ** 2 + 0.1 * rng.standard_normal(X.shape[0])


@pytest.mark.parametrize('normalize', [False, True])
def test_indices_equal_the_stated_arithmetic_and_scipy(m16, normalize):
    from scipy.stats import sobol_indices
    _, sens = m16
    d, n = 5, 1024
    Y = _y(m16, d, n)
    res = sens.sobol_analyze(Y, d, normalize=normalize, resamples=10)
    S1, ST, S2 = np_indices(Y, d, normalize=normalize)
    assert np.allclose(res['S1'], S1, rtol=1e-9, atol=1e-12)
    assert np.allclose(res['ST'], ST, rtol=1e-9, atol=1e-12)
    assert np.allclose(res['S2'], S2, rtol=1e-9, atol=1e-12, equal_nan=True)
    # scipy on the same (normalised) Y: ST is scipy's; scipy's S1 centres f_A, f_B, f_AB by the mean
    # of f_A and f_B first (Sobol & Levitan), the stated arithmetic (SALib's) does not -- the two
    # differ by exactly c * mean(f_AB - f_A) / V
    R = 2 * d + 2
    Yn = Y.reshape(n, R)
    if normalize:
        Yn = (Yn - Yn.mean()) / Yn.std()
    fA, fB, fAB = Yn[:, 0], Yn[:, R - 1], Yn[:, 1:1 + d].T
    sp = sobol_indices(func={'f_A': fA[None], 'f_B': fB[None], 'f_AB': fAB[:, None]}, n=n)
    assert np.allclose(res['ST'], sp.total_order, rtol=1e-9, atol=1e-12)
    c = np.mean(np.concatenate([fA, fB]))
    V = np.var(np.concatenate([fA, fB]))
    assert np.allclose(res['S1'] - c * np.mean(fAB - fA, axis=1) / V, sp.first_order, rtol=1e-9, atol=1e-12)


def test_ishigami_indices(m16):
    _, sens = m16
    bounds = {'x1': (-np.pi, np.pi), 'x2': (-np.pi, np.pi), 'x3': (-np.pi, np.pi)}
    X = sens.saltelli_sample(bounds, 2 ** 16)
    res = sens.sobol_analyze(ishigami(X), 3, resamples=10)
    a, b = 7.0, 0.1
    v1 = 0.5 * (1 + b * np.pi ** 4 / 5) ** 2
    v2 = a ** 2 / 8
    v13 = b ** 2 * np.pi ** 8 * (1 / 18 - 1 / 50)
    v = v1 + v2 + v13
    assert np.allclose(res['S1'], [v1 / v, v2 / v, 0.0], atol=0.01)
    assert np.allclose(res['ST'], [(v1 + v13) / v, v2 / v, v13 / v], atol=0.01)


# ---------------------------------------------------------------- 4. the bootstrap
def test_bootstrap_equals_its_numpy_restatement_and_is_deterministic(m16):
    import statistics
    _, sens = m16
    d, n, B, seed = 4, 512, 40, 12345
    Y = _y(m16, d, n)
    res = sens.sobol_analyze(Y, d, resamples=B, seed=seed)
    boots = [np_indices(Y, d, rows=np_draws(seed, r, n)) for r in range(B)]
    z = statistics.NormalDist().inv_cdf(0.975)
    for k, name in enumerate(('S1', 'ST', 'S2')):
        want = z * np.std(np.array([bt[k] for bt in boots]), axis=0, ddof=1)
        assert np.allclose(res[name + '_conf'], want, rtol=1e-9, atol=1e-14, equal_nan=True), name
    again = sens.sobol_analyze(Y, d, resamples=B, seed=seed)
    for key in res:
        assert np.array_equal(res[key], again[key], equal_nan=True)
    other = sens.sobol_analyze(Y, d, resamples=B, seed=seed + 1)
    assert not np.array_equal(res['S1_conf'], other['S1_conf'])
    assert np.array_equal(res['S1'], other['S1'])


def test_nan_in_y_propagates(m16):
    _, sens = m16
    d, n = 3, 64
    Y = _y(m16, d, n)
    Y[5] = np.nan
    res = sens.sobol_analyze(Y, d, resamples=5)
    assert np.all(np.isnan(res['S1'])) and np.all(np.isnan(res['ST_conf']))


# ---------------------------------------------------------------- 5. the parameters mode
@pytest.mark.parametrize('metric', ['nse', 'nnse', 'rmsd'])
def test_parameters_mode_scores_rows_as_et_batch(m16, metric):
    mod16_amd, sens = m16
    from oracle import synth
    _, drv = synth.drivers((1, 300), seed=7, special=False)
    drv = [np.asarray(v, np.float64).ravel() for v in drv]
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    rng = np.random.default_rng(1)
    obs = mod16_amd.MOD16._et(pvec, *drv) + rng.normal(0, 5, drv[0].size)
    obs[rng.random(obs.size) < 0.1] = np.nan
    bounds = dict(PARAMS) if metric == 'nnse' else {k: PARAMS[k] for k in ('gl_sh', 'csl', 'beta')}
    res, Y = sens.sobol_parameters(drv, obs, bounds, n=16, params=P, metric=metric, max_draws=100,
                                   resamples=10, return_outputs=True)
    X = sens.saltelli_sample(bounds, 16)
    full = np.repeat(np.array(pvec)[None], X.shape[0], axis=0)
    names = list(mod16_amd.MOD16.required_parameters)
    full[:, [names.index(k) for k in bounds]] = X
    sse, count = mod16_amd.MOD16._et_batch(full, *drv, observed=obs)
    assert np.array_equal(Y, sens.skill(sse, count, obs, metric), equal_nan=True)
    assert set(res) == {'S1', 'S1_conf', 'ST', 'ST_conf', 'S2', 'S2_conf'}


# ---------------------------------------------------------------- 6. at size
def test_drivers_mode_at_2_20_base_samples(m16):
    _, sens = m16
    fixed = None
    small = sens.sobol_drivers(P, DRIVERS, n=2 ** 12, fixed=fixed)
    big = sens.sobol_drivers(P, DRIVERS, n=2 ** 20, fixed=fixed)
    for key in ('S1', 'ST', 'S1_conf', 'ST_conf'):
        assert np.all(np.isfinite(big[key])), key
    ratio = np.median(big['ST_conf'] / small['ST_conf'])
    assert 1 / 32 <= ratio <= 1 / 8, ratio
