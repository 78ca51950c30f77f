"""The DE-MCMC-Z calibration sampler (mod16_amd.calibration) without a GPU: the prior YAML loader
against the reference's construction, family inference and the refusals that need no device, the
y-space log densities against scipy.stats, PyMC's tune() table and the random stream."""
import math
import os

import numpy as np
import pytest
import yaml
from scipy import stats
from scipy.special import log_expit

from conftest import GOLDEN

from mod16_amd import calibration as cal

PRIOR_YAML = os.path.join(GOLDEN, 'mcmc_prior_20240423.yaml')
ROW = dict(zip(cal.PARAM_NAMES, [-8.0, 8.0, 650.0, 4000.0, 0.04, 0.02, 1e-5, 0.005, 20.0, 500.0, 250.0]))


def reference_prior(path, pft):
    # calibration.py:923-931, restated literally
    with open(path, 'r') as file:
        prior = yaml.safe_load(file)
    prior_params = list(filter(lambda p: p in prior.keys(), cal.PARAM_NAMES))
    return dict([(p, dict([(k, v[pft]) for k, v in prior[p].items()])) for p in prior_params])


@pytest.mark.parametrize('pft', [0, 1, 2, 5, 7, 10, 11, 12])
def test_load_prior_matches_the_references_construction(pft):
    got = cal.load_prior(PRIOR_YAML, pft)
    want = reference_prior(PRIOR_YAML, pft)
    assert got == want
    assert list(got) == list(want)


def test_family_inference_on_the_shipped_prior():
    prior = cal.load_prior(PRIOR_YAML, 7)
    fams = {k: cal.prior_family(v)[0] for k, v in prior.items()}
    assert fams == {'vpd_close': 'uniform', 'gl_sh': 'lognormal', 'gl_wv': 'lognormal',
                    'g_cuticular': 'lognormal', 'csl': 'lognormal', 'rbl_min': 'triangular',
                    'rbl_max': 'triangular', 'beta': 'uniform'}
    assert cal.prior_family(prior['rbl_min'])[1] == (10.0, 1000.0, 10.0)      # c = lower
    assert cal.prior_family(prior['rbl_max'])[1] == (100.0, 1000.0, 1000.0)   # c = upper


@pytest.mark.parametrize('spec', [
    {'lower': 1.0}, {'mu': 0.0}, {'lower': 0, 'upper': 1, 'sigma': 1}, {'lower': 2.0, 'upper': 1.0},
    {'lower': 1.0, 'upper': 1.0}, {'mu': 0.0, 'sigma': 0.0}, {'mu': 0.0, 'sigma': -1.0},
    {'lower': 0.0, 'upper': 1.0, 'c': 1.5}, {'lower': 0.0, 'upper': 1.0, 'c': -0.1},
    {'lower': None, 'upper': 1.0}, {'mu': float('nan'), 'sigma': 1.0}])
def test_bad_priors_are_refused(spec):
    with pytest.raises(ValueError):
        cal.prior_family(spec)


class _Problem(object):
    '''What the sampler reads of a bound problem before any device call.'''
    dtype = np.float64
    math = 0
    has_observed = True
    max_draws = 64


def test_refusals_before_any_device_call():
    prior = {'csl': {'mu': -5.5, 'sigma': 0.8}}
    p = _Problem()
    with pytest.raises(ValueError, match='unknown'):
        cal.DEMetropolisZ(p, ROW, {'nope': {'lower': 0, 'upper': 1}})
    with pytest.raises(ValueError, match='unknown'):
        cal.DEMetropolisZ(p, ROW, prior, fixed={'betta': 250})
    with pytest.raises(ValueError, match='unknown'):
        cal.DEMetropolisZ(p, dict(ROW, extra=1.0), prior)
    with pytest.raises(ValueError):
        cal.DEMetropolisZ(p, list(ROW.values())[:10], prior)
    # neither free nor fixed: a NaN beta without a prior or a fixed value (the reference puts in 250)
    with pytest.raises(ValueError, match='neither'):
        cal.DEMetropolisZ(p, dict(ROW, beta=float('nan')), prior)
    with pytest.raises(ValueError, match='neither'):
        cal.DEMetropolisZ(p, dict(ROW, gl_sh=None), prior)
    # fixed overrides params and removes the parameter from the free set: nothing free is an error
    with pytest.raises(ValueError, match='no free'):
        cal.DEMetropolisZ(p, ROW, prior, fixed={'csl': 0.004})
    with pytest.raises(ValueError, match='finite'):
        cal.DEMetropolisZ(p, ROW, prior, fixed={'beta': float('nan')})
    # bad bounds
    for bad in ({'csl': {'lower': 2.0, 'upper': 1.0}}, {'csl': {'mu': 0.0, 'sigma': 0.0}},
                {'rbl_min': {'lower': 10.0, 'upper': 1000.0, 'c': 1001.0}}):
        with pytest.raises(ValueError):
            cal.DEMetropolisZ(p, ROW, bad)
    with pytest.raises(ValueError, match='objective'):
        cal.DEMetropolisZ(p, ROW, prior, objective='nse')
    with pytest.raises(ValueError, match='tune_target'):
        cal.DEMetropolisZ(p, ROW, prior, tune_target='sigma')
    with pytest.raises(ValueError, match='max_draws'):
        cal.DEMetropolisZ(p, ROW, prior, chains=65)
    q = _Problem()
    q.dtype = np.float32
    with pytest.raises(ValueError, match='float64'):
        cal.DEMetropolisZ(q, ROW, prior)
    q = _Problem()
    q.math = 1
    with pytest.raises(ValueError, match='MATH_FAST'):
        cal.DEMetropolisZ(q, ROW, prior)
    q = _Problem()
    q.has_observed = False
    with pytest.raises(ValueError, match='observed'):
        cal.DEMetropolisZ(q, ROW, prior)


def _ys():
    return np.concatenate([np.linspace(-30, 30, 601), [-700.0, -40.0, 40.0, 700.0]])


def test_uniform_log_density_is_scipys_plus_the_jacobian():
    a, b = 1000.0, 8000.0
    y = np.linspace(-30, 30, 601)
    x = cal.x_of_y('uniform', (a, b, 0.0), y)
    jac = np.log(b - a) + log_expit(y) + log_expit(-y)       # log |dx/dy|
    want = stats.uniform(loc=a, scale=b - a).logpdf(np.clip(x, a, b)) + jac
    ok = (x > a) & (x < b)
    assert np.allclose(cal.log_prior('uniform', (a, b, 0.0), y)[ok], want[ok], rtol=1e-9, atol=1e-9)
    assert np.all(np.isfinite(cal.log_prior('uniform', (a, b, 0.0), _ys())))


def test_lognormal_log_density_is_scipys_plus_the_jacobian():
    mu, s = -5.5, 0.8
    y = np.linspace(-12, 1, 531)
    x = np.exp(y)
    want = stats.lognorm(s=s, scale=np.exp(mu)).logpdf(x) + y      # log |dx/dy| = y
    assert np.allclose(cal.log_prior('lognormal', (mu, s, 0.0), y), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('abc', [(100.0, 1000.0, 400.0), (10.0, 1000.0, 10.0), (100.0, 1000.0, 1000.0)])
def test_triangular_log_density_is_scipys_plus_the_jacobian_at_both_edges(abc):
    a, b, c = abc
    p = (a, b, c)
    y = np.linspace(-15, 15, 301)      # (further out scipy's 1 - (x - a) / (b - a) cancels)
    x = cal.x_of_y('triangular', p, y)
    jac = np.log(b - a) + log_expit(y) + log_expit(-y)       # log |dx/dy|
    want = stats.triang(c=(c - a) / (b - a), loc=a, scale=b - a).logpdf(x) + jac
    got = cal.log_prior('triangular', p, y)
    ok = np.isfinite(want) & (x > a) & (x < b)
    assert ok.sum() > 250
    assert np.allclose(got[ok], want[ok], rtol=1e-8, atol=1e-8)
    # where the density is 0 or undefined (x at the bound opposite c): -inf, never NaN
    assert not np.any(np.isnan(cal.log_prior('triangular', p, _ys())))


def test_tune_factor_table_at_every_boundary():
    table = [(0.0, 0.1), (0.000999, 0.1), (0.001, 0.5), (0.0499, 0.5), (0.05, 0.9), (0.1999, 0.9),
             (0.2, 1.0), (0.5, 1.0), (0.5001, 1.1), (0.75, 1.1), (0.7501, 2.0), (0.95, 2.0),
             (0.9501, 10.0), (1.0, 10.0)]
    for rate, factor in table:
        assert cal.tune_factor(rate) == factor, rate


def test_random_stream_reproduces_splitmix64():
    def mix(z):
        z = np.uint64(z)
        with np.errstate(over='ignore'):
            z ^= z >> np.uint64(30)
            z *= np.uint64(0xbf58476d1ce4e5b9)
            z ^= z >> np.uint64(27)
            z *= np.uint64(0x94d049bb133111eb)
            z ^= z >> np.uint64(31)
        return int(z)
    # splitmix64's first output of seed 0 is mix(0x9e3779b97f4a7c15)
    assert cal.mix(0x9e3779b97f4a7c15) == 0xe220a8397b1dcdaf
    for seed, c, t, k in [(0, 0, 0, 0), (1, 3, 999, 63), (2 ** 64 - 1, 1023, 123456, 17), (7, 2, 5, 16)]:
        want = mix(mix(mix(seed) ^ c) ^ ((t << 6) | k))
        assert cal.stream(seed, c, t, k) == want
    z = cal.stream(0, 0, 0, 0)
    assert cal.unit(z) == (z >> 11) * 2.0 ** -53 and 0.0 <= cal.unit(z) < 1.0
    assert cal.index(z, 1000) == (z * 1000) // 2 ** 64 and 0 <= cal.index(z, 1000) < 1000
    assert cal.index(2 ** 64 - 1, 7) == 6


def test_default_initial_point_and_lamb():
    assert cal.support_point('uniform', (0.0, 1000.0, 0.0)) == 500.0
    assert cal.support_point('lognormal', (-5.5, 0.8, 0.0)) == math.exp(-5.5 + 0.32)
    assert cal.support_point('triangular', (10.0, 1000.0, 10.0)) == 1020.0 / 3.0
    for fam, p in (('uniform', (0.0, 1000.0, 0.0)), ('triangular', (100.0, 1000.0, 400.0))):
        x = cal.support_point(fam, p)
        assert cal.x_of_y(fam, p, cal.y_of_x(fam, p, x)) == pytest.approx(x, rel=1e-14)
