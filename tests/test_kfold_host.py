"""k-fold cross-validation (mod16_amd.calibration) without a GPU: kfold_labels against the
reference's slicing restated on the same permutation (calibration.py:859-869), its refusals, the
groups' random stream, the reference-shaped test_indices, the host-side refusals of bad labels, and
the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from mod16_amd import MOD16, _lib
from mod16_amd import calibration as cal


def reference_folds(indices, k_folds):
    # calibration.py:863-869, restated literally on a given permutation
    fold_idx = np.array([indices.size // k_folds] * k_folds) * np.arange(0, k_folds)
    fold_idx = list(map(list, zip(fold_idx, fold_idx + indices.size // k_folds)))
    fold_idx[-1][-1] = indices.max()
    return [indices[start:end] for start, end in fold_idx]


@pytest.mark.parametrize('n, k', [(10, 2), (11, 3), (1000, 5), (1003, 7), (5, 5), (300, 255)])
def test_labels_sizes_and_coverage(n, k):
    lab = cal.kfold_labels(n, k)
    assert lab.shape == (n,) and lab.dtype == np.uint8
    sizes = np.bincount(lab, minlength=k)
    assert sizes.size == k and sizes.sum() == n
    assert (sizes[:-1] == n // k).all()
    assert sizes[-1] == n - (k - 1) * (n // k)       # the last slice takes the remainder


def test_labels_are_seeded():
    assert np.array_equal(cal.kfold_labels(500, 5, seed=3), cal.kfold_labels(500, 5, seed=3))
    assert not np.array_equal(cal.kfold_labels(500, 5, seed=3), cal.kfold_labels(500, 5, seed=4))
    assert np.array_equal(cal.kfold_labels(500, 5), cal.kfold_labels(500, 5, seed=0))


@pytest.mark.parametrize('n, k', [(10, 2), (11, 3), (1000, 5), (1003, 7), (64, 8)])
def test_labels_equal_the_references_slices_but_the_final_row(n, k):
    perm = np.random.default_rng(9).permutation(n)
    lab = cal.kfold_labels(n, k, seed=9)
    ref = reference_folds(perm, k)
    for f in range(k):
        assert (lab[ref[f]] == f).all()
    # the reference ends its last slice at n - 1, exclusive: the last shuffled row is held out by
    # no fold there; here it belongs to the last fold, and every other row agrees
    assert sum(r.size for r in ref) == n - 1
    assert lab[perm[-1]] == k - 1
    unref = np.setdiff1d(np.arange(n), np.concatenate(ref))
    assert unref.tolist() == [perm[-1]]


@pytest.mark.parametrize('n, k', [(10, 1), (10, 0), (10, -2), (300, 256), (4, 5)])
def test_bad_k_is_refused(n, k):
    with pytest.raises(ValueError):
        cal.kfold_labels(n, k)


def test_group_stream_is_the_plain_stream_of_seed_plus_fold():
    M = (1 << 64) - 1
    for seed, f, j, t, k in [(0, 0, 0, 0, 0), (11, 2, 1, 999, 63), (M, 3, 5, 7, 16), (M - 1, 4, 0, 1, 1)]:
        want = cal.mix(cal.mix(cal.mix((seed + f) & M) ^ j) ^ ((t << 6) | k))
        assert cal.group_stream(seed, f, j, t, k) == want == cal.stream((seed + f) & M, j, t, k)
    # group 0 of fold 0 is the plain sampler's chain j
    assert cal.group_stream(5, 0, 2, 3, 4) == cal.stream(5, 2, 3, 4)


def test_test_indices_are_reference_shaped_and_padded():
    lab = np.array([0, 1, 2, 0, 1, 0, 2, 2, 2], np.uint8)
    ti = cal.test_indices(lab, 3)
    assert ti.dtype == np.int64 and ti.shape == (3, 4)
    assert ti[0].tolist() == [0, 3, 5, -1]
    assert ti[1].tolist() == [1, 4, -1, -1]
    assert ti[2].tolist() == [2, 6, 7, 8]


def test_bad_labels_are_refused_on_the_host():
    """The label checks of _et_bind run before any device call (so they raise ValueError even
    here, without a GPU)."""
    drv = [np.ones(6)] * 14
    obs = np.ones(6)
    for folds in ([0, 1, 2, 0, 1], [0, 1, 3, 0, 1, 0], [0, 0, 0, 0, 0, 0], [-1, 0, 1, 0, 1, 0],
                  np.array([0.0, 1, 0, 1, 0, 1]), 1, 7, 256):
        with pytest.raises(ValueError):
            MOD16._et_bind(*drv, observed=obs, folds=folds)
    for kw in ({'math': _lib.MATH_EXACT}, {'observed': None}):
        args = dict(observed=obs, folds=2)
        args.update(kw)
        with pytest.raises(ValueError):
            MOD16._et_bind(*drv, **args)
    with pytest.raises(ValueError):
        MOD16._et_bind(*[np.ones(6, np.float32)] * 14, observed=obs.astype(np.float32), folds=2)


def test_new_symbols_are_in_the_header():
    text = open(os.path.join(ROOT, 'include', 'mod16_hip.h')).read()
    for name in ('mod16_static_batch_set_folds', 'mod16_static_batch_objective_folds', 'mod16_mcmc_create_groups'):
        assert re.search(r'MOD16_API\s+int\s+%s\s*\(' % name, text), name
        assert name in _lib.PROTOTYPES
    assert re.search(r'#define MOD16_FOLD_HELDOUT 0x100\b', text) and _lib.FOLD_HELDOUT == 0x100
    assert _lib.ABI_VERSION >= 8


def test_sampler_folds_argument_is_checked_on_the_host():
    """DEMetropolisZ(..., folds=...) refuses anything but True / False / a list of distinct folds in
    range with ValueError, before any device call (a stand-in problem: no GPU is reached)."""
    from types import SimpleNamespace
    prob = SimpleNamespace(dtype=np.float64, math=_lib.MATH_FAST, has_observed=True, max_draws=8, nfolds=3)
    prior = {'vpd_close': {'lower': 1000.0, 'upper': 8000.0}}
    row = dict(zip(cal.PARAM_NAMES, [-8.0, 8.0, 650.0, 4000.0, 0.04, 0.02, 1e-5, 0.005, 20.0, 500.0, 250.0]))
    for folds in (2, 0, np.int64(1), 1.5, 'all', [0.5, 1.0], [[0, 1]], [0, 0], [3], [-1], []):
        with pytest.raises(ValueError):
            cal.DEMetropolisZ(prob, row, prior, chains=2, folds=folds)
    for folds in (True, np.True_):             # every fold: 3 x 3 chains > max_draws = 8
        with pytest.raises(ValueError, match='3 fold'):
            cal.DEMetropolisZ(prob, row, prior, chains=3, folds=folds)
    with pytest.raises(ValueError, match='bound with folds'):
        cal.DEMetropolisZ(SimpleNamespace(**dict(vars(prob), nfolds=0)), row, prior, chains=2, folds=[0])
