"""The Sobol sensitivity analysis (mod16_amd.sensitivity) without a GPU: the committed direction
table is scipy's, arguments are refused before anything reaches the device, and without an MI355X
every entry point raises instead of computing on the CPU."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mod16_amd
from mod16_amd import _lib
from mod16_amd import sensitivity as sens

BOUNDS = json.load(open(os.path.join(GOLDEN, 'sensitivity_bounds.json')))
DRIVERS = BOUNDS['drivers']
PARAMS = BOUNDS['parameters']
MEAN_PARAMS = {k: 0.5 * (lo + hi) for k, (lo, hi) in PARAMS.items()}


def test_committed_direction_table_is_scipys():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import make_sobol_table
    finally:
        sys.path.pop(0)
    table = make_sobol_table.committed()
    assert len(table) == 32 and all(len(row) == 32 for row in table)
    assert table == make_sobol_table.derive()


def test_direction_table_reproduces_scipys_points():
    """The header's construction (XOR over the set bits of gray(i)), restated on the committed table."""
    from scipy.stats import qmc
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import make_sobol_table
    finally:
        sys.path.pop(0)
    V = np.array(make_sobol_table.committed(), np.uint64)
    eng = qmc.Sobol(32, scramble=False, bits=32)
    eng.fast_forward(1000)
    want = eng.random(64)
    for row, i in enumerate(range(1000, 1064)):
        g = i ^ (i >> 1)
        x = np.zeros(32, np.uint64)
        for b in range(32):
            if (g >> b) & 1:
                x ^= V[:, b]
        assert np.array_equal(x * 2.0 ** -32, want[row])


@pytest.mark.parametrize('n', [0, 3, 1000, 2 ** 27])
def test_n_must_be_a_power_of_two(n):
    with pytest.raises(ValueError, match='power of two'):
        sens.saltelli_sample({'a': (0, 1)}, n)
    with pytest.raises(ValueError, match='power of two'):
        sens.sobol_drivers(MEAN_PARAMS, DRIVERS, n=n)
    with pytest.raises(ValueError, match='power of two'):
        sens.sobol_analyze(np.broadcast_to(0.0, (4 * n,)), 1)


@pytest.mark.parametrize('pair', [(1, 1), (2, 1), (0, np.inf), (np.nan, 1)])
def test_bounds_need_lo_below_hi_both_finite(pair):
    with pytest.raises(ValueError, match='lo < hi'):
        sens.saltelli_sample({'a': (0, 1), 'b': pair}, 8)
    with pytest.raises(ValueError, match='lo < hi'):
        sens.sobol_drivers(MEAN_PARAMS, dict(DRIVERS, fpar=pair), n=8)


def test_unknown_names_are_refused():
    with pytest.raises(ValueError, match='unknown'):
        sens.sobol_drivers(MEAN_PARAMS, {'lai': (0, 1), 'lia': (0, 1)}, n=8, fixed=DRIVERS)
    with pytest.raises(ValueError, match='unknown'):
        sens.sobol_parameters([1.0] * 14, 1.0, {'beta': (0, 1), 'gamma': (0, 1)}, n=8,
                              params=MEAN_PARAMS)


@pytest.mark.parametrize('d', [0, 15])
def test_between_one_and_fourteen_variables(d):
    bounds = {'x%d' % k: (0, 1) for k in range(d)}
    with pytest.raises(ValueError, match='between 1 and 14'):
        sens.saltelli_sample(bounds, 8)
    with pytest.raises(ValueError, match='between 1 and 14'):
        sens.sobol_analyze(np.zeros(64), d)


def test_drivers_missing_from_fixed():
    with pytest.raises(ValueError, match='neither in bounds nor in fixed'):
        sens.sobol_drivers(MEAN_PARAMS, {'lai': (0.1, 5)}, n=8, fixed={'fpar': 0.5})
    with pytest.raises(ValueError, match='neither in bounds nor in params'):
        sens.sobol_parameters([1.0] * 14, 1.0, {'beta': (0, 1)}, n=8)


def test_y_must_hold_whole_base_samples():
    with pytest.raises(ValueError, match='multiple'):
        sens.sobol_analyze(np.zeros(8 * 5 + 1), 2)
    with pytest.raises(ValueError, match='metric'):
        sens.sobol_parameters([1.0] * 14, 1.0, {'beta': (0, 1)}, n=8, params=MEAN_PARAMS, metric='r2')


def test_skill_metrics():
    obs = np.array([1.0, 2.0, np.nan, 4.0])
    sse, count = np.array([0.5, 2.0]), np.array([3.0, 3.0])
    den = np.nansum((obs - np.nanmean(obs)) ** 2)
    assert np.array_equal(sens.skill(sse, count, obs, 'nse'), 1 - sse / den)
    assert np.array_equal(sens.skill(sse, count, obs, 'nnse'), 1 / (2 - (1 - sse / den)))
    assert np.array_equal(sens.skill(sse, count, obs, 'rmsd'), np.sqrt(sse / count))


def test_no_device_no_cpu_fallback():
    if _lib.device_count() > 0:
        pytest.skip('a GPU is present')
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        sens.saltelli_sample({'a': (0, 1)}, 8)
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        sens.sobol_analyze(np.random.default_rng(0).random(8 * 6), 2)
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        sens.sobol_drivers(MEAN_PARAMS, DRIVERS, n=8)
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        sens.sobol_parameters([np.ones(4)] * 14, np.ones(4), PARAMS, n=8)
    assert mod16_amd.sensitivity is sens
