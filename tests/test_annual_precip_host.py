"""The annual-precipitation constraint, host side (no GPU): calibration.annual_precip_penalty against
what the reference's own constrain_by_map returned (tests/golden/f10_annual_precip.npz, written by
tests/golden/make_annual_precip.py), and the refusals of MOD16._et_bind(..., annual_precip=...) and
DEMetropolisZ(..., constraints=...) that are made before any device call."""
import numpy as np
import pytest


@pytest.fixture(scope='module')
def cal():
    from mod16_amd import calibration
    return calibration


def test_penalty_restatement_matches_the_reference_function(golden, cal):
    """rtol 1e-11: the restatement differs from the reference only in the order of its <= 366-term and
    Y N-term float64 sums (relative 366 x 2^-53 < 1e-13 each), times the cancellation factor <= 10 of
    the clipped difference (the fixture keeps every limit outside +-10 % of its total), squared."""
    f = golden('f10_annual_precip')
    le, years, lhv = f['le'], f['years'], f['lhv']
    none = cal.annual_precip_penalty(le, years, lhv, f['annual_precip_none'])
    assert none == 0.0 and f['expected_none'] == 0.0                     # exactly: no site-year over its limit
    quarter = cal.annual_precip_penalty(le, years, lhv, f['annual_precip_quarter'])
    assert f['expected_quarter'] < -1.0
    np.testing.assert_allclose(quarter, f['expected_quarter'], rtol=1e-11, atol=0)
    le_nan = le.copy()
    le_nan[tuple(f['nan_at'])] = np.nan
    assert np.isnan(f['expected_nan'])
    assert np.isnan(cal.annual_precip_penalty(le_nan, years, lhv, f['annual_precip_quarter']))
    # a stack of predictions: one penalty each
    both = cal.annual_precip_penalty(np.stack([le, le_nan, 0.5 * le]), years, lhv, f['annual_precip_quarter'])
    assert both.shape == (3,) and both[0] == quarter and np.isnan(both[1]) and quarter < both[2] <= 0.0
    with pytest.raises(ValueError):
        cal.annual_precip_penalty(le, years[:-1], lhv, f['annual_precip_quarter'])
    with pytest.raises(ValueError):
        cal.annual_precip_penalty(le, years, lhv, f['annual_precip_quarter'][:2])


def _bind(dtype=np.float64, shape=(730, 3), **kw):
    import mod16_amd
    drv = [np.full(shape, 1.0, dtype) for _ in range(14)]
    kw.setdefault('observed', np.zeros(shape, dtype))
    return mod16_amd.MOD16._et_bind(*drv, **kw)


YEARS = np.repeat([2001, 2004], 365)
LIMIT = np.full((2, 3), 700.0)


@pytest.mark.parametrize('case, kw', [
    ('years of the wrong length', dict(annual_precip=(YEARS[:-1], LIMIT))),
    ('years that are not integers', dict(annual_precip=(YEARS.astype(float), LIMIT))),
    ('a year with no row', dict(annual_precip=(np.repeat([2001, 2004, 2005, 2006], [365, 363, 1, 1]), LIMIT))),
    ('a row with no year', dict(annual_precip=(YEARS, np.full((3, 3), 700.0)))),
    ('the wrong number of sites', dict(annual_precip=(YEARS, np.full((2, 4), 700.0)))),
    ('a NaN limit', dict(annual_precip=(YEARS, np.where(np.eye(2, 3) > 0, np.nan, LIMIT)))),
    ('an infinite limit', dict(annual_precip=(YEARS, np.where(np.eye(2, 3) > 0, np.inf, LIMIT)))),
    ('limits that sum to zero', dict(annual_precip=(YEARS, np.zeros((2, 3))))),
    ('not a pair', dict(annual_precip=LIMIT)),
    ('float32', dict(annual_precip=(YEARS, LIMIT), dtype=np.float32)),
    ('EXACT', dict(annual_precip=(YEARS, LIMIT), math=1)),
    ('no observations', dict(annual_precip=(YEARS, LIMIT), observed=None)),
    ('folds', dict(annual_precip=(YEARS, LIMIT), folds=3)),
    ('a flat problem', dict(annual_precip=(YEARS, np.full((2, 1), 700.0)), shape=(730,))),
])
def test_bind_refuses_on_the_host(case, kw):
    """ValueError before any device call: on a machine without a GPU reaching the device raises
    Mod16Error instead, on one with a GPU the bind would succeed."""
    from mod16_amd import _lib
    assert _lib.MATH_EXACT == 1
    with pytest.raises(ValueError):
        _bind(**kw)


class _Problem(object):
    dtype = np.float64
    math = 0
    has_observed = True
    max_draws = 64
    nfolds = 0
    has_annual = False


def test_sampler_refuses_constraints_on_the_host(cal):
    P = dict.fromkeys(cal.PARAM_NAMES, 1.0)
    prior = {'gl_sh': {'mu': -3.45, 'sigma': 0.71}}
    with pytest.raises(ValueError, match='annual_precip'):
        cal.DEMetropolisZ(_Problem(), P, prior, constraints=True)
    with pytest.raises(ValueError, match='unknown constraint'):
        cal.DEMetropolisZ(_Problem(), P, prior, constraints=('annual_rain',))
    folded = _Problem()
    folded.nfolds, folded.has_annual = 3, True
    with pytest.raises(ValueError, match='folds'):
        cal.DEMetropolisZ(folded, P, prior, constraints=('annual_precipitation',), folds=True)
    assert cal.CONSTRAINTS == ('annual_precipitation',)
