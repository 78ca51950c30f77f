"""The numpy statement of the per-pixel quantiles over the members of an ensemble run
(mod16_amd.calibration.quantile_positions / ensemble_quantile): the definition the selection kernel of
mod16_et_ensemble_quantiles_* follows. No GPU.

Tolerance against np.quantile(..., axis=0) on finite members: 4 * 2^-52 * max_m |x_m|. numpy's 'linear'
method evaluates the same a + frac (b - a) in another association (its lerp switches to b - (b - a)(1 -
frac) for frac >= 0.5): each form has two roundings of values no larger than 2 max|x_m|, so they differ
by at most 4 ulp of max|x_m|; measured 3.3e-16 max|x_m|."""
import numpy as np
import pytest

from mod16_amd.calibration import ensemble_quantile, quantile_positions

Q6 = (0, 0.05, 1 / 3, 0.5, 0.95, 1)
EPS = 2.0 ** -52


def test_positions():
    lo, frac = quantile_positions((0, 1), 33)
    assert lo.dtype == np.int64 and frac.dtype == np.float64
    assert lo.tolist() == [0, 32] and frac.tolist() == [0.0, 0.0]
    lo, frac = quantile_positions(0.5, 4)              # a scalar is a 1-tuple
    assert lo.shape == (1,) and lo[0] == 1 and frac[0] == 0.5
    lo, frac = quantile_positions(Q6, 1)               # one member: every position is member 0
    assert (lo == 0).all() and (frac == 0).all()
    for D in (2, 5, 17, 256):
        lo, frac = quantile_positions(Q6, D)
        h = np.array(Q6, np.float64) * (D - 1)         # one float64 multiply
        assert np.array_equal(lo, np.floor(h).astype(np.int64)) and np.array_equal(frac, h - np.floor(h))
        assert (lo >= 0).all() and (lo <= D - 1).all() and (frac >= 0).all() and (frac < 1).all()


@pytest.mark.parametrize('q', [(), tuple([0.5] * 9), -1e-9, 1 + 1e-9, np.nan, (0.5, np.nan), np.inf,
                               [[0.1, 0.2]]])
def test_positions_refusals(q):
    with pytest.raises(ValueError):
        quantile_positions(q, 5)


def test_eight_quantiles_are_accepted():
    lo, frac = quantile_positions(np.linspace(0, 1, 8), 5)
    assert lo.shape == frac.shape == (8,)
    with pytest.raises(ValueError):
        quantile_positions(0.5, 0)


@pytest.mark.parametrize('D', [1, 2, 5, 16, 17, 33, 64, 256])
def test_against_numpy(D):
    rng = np.random.default_rng(100 + D)
    x = rng.normal(0, 1, (D, 2000)) * 10.0 ** rng.integers(-8, 3, 2000)
    x[:, 100:300] *= rng.uniform(0, 1, (D, 200)) < 0.5              # blocks of exact zeros
    x[:, 300:350] = 0.0
    if D > 1:                                                        # duplicated rows: ties
        x[D // 2, 400:900] = x[0, 400:900]
        x[D - 1, 600:1200] = x[0, 600:1200]
    got = ensemble_quantile(x, Q6)
    want = np.quantile(x, Q6, axis=0)
    assert got.shape == want.shape == (6, 2000) and got.dtype == np.float64
    scale = np.abs(x).max(axis=0)
    err = np.abs(got - want)
    rel = err[:, scale > 0] / scale[scale > 0]
    print('D = %d: max |statement - np.quantile| / max|x_m| = %.3e' % (D, rel.max()))
    assert (err <= 4 * EPS * scale).all()
    assert (got[:, scale == 0] == 0).all()
    assert np.array_equal(got[0], x.min(axis=0)) and np.array_equal(got[-1], x.max(axis=0))
    assert (np.diff(got, axis=0) >= 0).all()
    # a trailing shape is kept
    assert np.array_equal(ensemble_quantile(x.reshape(D, 40, 50), Q6), got.reshape(6, 40, 50))
    assert np.array_equal(ensemble_quantile(x, 0.5)[0], got[3])


def test_nan_rule():
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1, (5, 64))
    x[3, 10] = np.nan
    x[:, 20] = np.nan
    x[0, 30] = np.nan
    got = ensemble_quantile(x, Q6)
    nan = np.zeros(64, bool)
    nan[[10, 20, 30]] = True
    assert np.isnan(got[:, nan]).all() and np.isfinite(got[:, ~nan]).all()
    keep = np.quantile(x[:, ~nan], Q6, axis=0)
    assert np.allclose(got[:, ~nan], keep, rtol=0, atol=4 * EPS * np.abs(x[:, ~nan]).max())


def test_infinite_members():
    inf = np.inf
    # equal infinities stay
    x = np.array([[inf], [inf], [inf]])
    assert (ensemble_quantile(x, Q6) == inf).all()
    assert (ensemble_quantile(-x, Q6) == -inf).all()
    # a position exactly on a finite member is that member: D = 5, q = 0.5 -> s[2]
    x = np.array([[-inf], [1.0], [2.0], [3.0], [inf]])
    got = ensemble_quantile(x, (0, 0.25, 0.5, 0.75, 1))[:, 0]
    assert got.tolist() == [-inf, 1.0, 2.0, 3.0, inf]
    # between a finite member and +inf: +inf; between -inf and anything else: inf - inf = NaN
    got = ensemble_quantile(x, (0.9, 0.1))[:, 0]
    assert got[0] == inf and np.isnan(got[1])
    # ties of infinities at the top: a == b
    x = np.array([[0.0], [inf], [inf]])
    assert ensemble_quantile(x, 0.75)[0, 0] == inf
