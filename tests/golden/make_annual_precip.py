#!/usr/bin/env python3
"""Writes tests/golden/f10_annual_precip.npz: inputs and outputs of the reference's annual-precipitation
constraint, `constrain_by_map`, a closure defined inside `CalibrationAPI.tune` of the reference's
mod16/calibration.py. That module cannot be imported where pymc and h5py are absent, so the
function's node is lifted out of the parsed file with `ast`, compiled against numpy alone and
called. Nothing of the reference's text is kept: the fixture holds numbers only.

    python tests/golden/make_annual_precip.py /path/to/reference/mod16/calibration.py

Three cases on one (T, N) = (1096, 3) array of predictions (years 2003, 2004 -- a leap year -- and
2007, so the labels are not contiguous; about a fifth of the predictions negative):
  none     every limit 1.5 x its site-year's total: the penalty is exactly (minus) zero
  quarter  two of the nine limits 0.7 x their total, the others 1.3 x: every limit stays outside
           +-10 % of its total, so the clipped difference has a cancellation factor <= 10
  nan      the limits of `quarter`, one prediction NaN: the penalty is NaN
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def lift(path, name='constrain_by_map'):
    tree = ast.parse(open(path).read())
    nodes = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(nodes) == 1, 'expected one %s in %s' % (name, path)
    module = ast.Module(body=[nodes[0]], type_ignores=[])
    scope = {'np': np}
    exec(compile(ast.fix_missing_locations(module), path, 'exec'), scope)
    return scope[name]


def main():
    fn = lift(sys.argv[1])
    rng = np.random.default_rng(20240610)
    years = np.concatenate([np.full(365, 2003), np.full(366, 2004), np.full(365, 2007)])
    T, N = years.size, 3
    le = rng.normal(70.0, 80.0, (T, N))
    lhv = 2.501e6 - 2361.0 * rng.uniform(-5.0, 30.0, (T, N))
    mass = np.maximum(le * 86400.0 / lhv, 0.0)
    tot = np.stack([mass[years == y].sum(axis=0) for y in np.unique(years)])
    factor = np.full(tot.shape, 1.3)
    factor[0, 1] = factor[2, 2] = 0.7
    limits = {'none': 1.5 * tot, 'quarter': factor * tot}
    nan_at = np.array([500, 1])
    le_nan = le.copy()
    le_nan[tuple(nan_at)] = np.nan
    out = {'years': years, 'le': le, 'lhv': lhv, 'nan_at': nan_at,
           'annual_precip_none': limits['none'], 'annual_precip_quarter': limits['quarter'],
           'expected_none': np.float64(fn(le.copy(), years, lhv, limits['none'])),
           'expected_quarter': np.float64(fn(le.copy(), years, lhv, limits['quarter'])),
           'expected_nan': np.float64(fn(le_nan, years, lhv, limits['quarter']))}
    assert out['expected_none'] == 0 and out['expected_quarter'] < 0 and np.isnan(out['expected_nan'])
    np.savez(os.path.join(HERE, 'f10_annual_precip.npz'), **out)
    print({k: (v.shape if v.ndim else float(v)) for k, v in out.items()})


if __name__ == '__main__':
    main()
