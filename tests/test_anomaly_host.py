"""The numpy definition of the per-pixel climatology, standardized anomaly and percentile rank
(mod16_amd/anomaly.py), on the CPU: known answers worked by hand, numpy's own reductions, the bit-level
properties the definition promises (scaling by a power of two, one rounding for float32 input, the
default baseline), every argument check, and the ABI pieces that need no device. The device result is
held to this definition bit for bit by tests/test_gpu_anomaly.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mod16_amd import anomaly as an

HEADER = os.path.join(ROOT, 'include', 'mod16_hip.h')
ALL = an.OUTPUT_NAMES


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_two_years_one_period_by_hand():
    x0, x1 = 3.0, 7.5
    res = an.anomaly(np.array([[x0], [x1]]), periods=1, min_valid=2, outputs=ALL)
    mean = (x0 + x1) / 2.0
    e0, e1 = x0 - mean, x1 - mean
    std = np.sqrt((e0 * e0 + e1 * e1) / 1.0)
    assert res.mean[0, 0] == mean and res.std[0, 0] == std and res.count[0, 0] == 2
    assert abs(std - abs(x1 - x0) / np.sqrt(2.0)) <= 2 ** -50 * std
    assert res.z[0, 0] == e0 / std and res.z[1, 0] == e1 / std
    assert abs(res.z[0, 0] + 1 / np.sqrt(2.0)) < 1e-15 and abs(res.z[1, 0] - 1 / np.sqrt(2.0)) < 1e-15
    assert res.pct[0, 0] == 0.25 and res.pct[1, 0] == 0.75
    assert res.z.dtype == np.float64 and res.mean.dtype == np.float64 and res.count.dtype == np.uint8


def test_constant_pixel():
    Y, P = 6, 3
    res = an.anomaly(np.full((Y * P, 2), 7.25), np.full((Y * P, 2), 29.0), periods=P, outputs=ALL)
    assert (res.std == 0.0).all() and (res.mean == 0.25).all() and (res.count == Y).all()
    assert np.isnan(res.z).all() and (res.pct == 0.5).all()


def test_ties_give_multiples_of_half_a_rank():
    Y = 7
    x = np.array([2.0, 1.0, 2.0, 3.0, 1.0, 2.0, 5.0])[:, None]
    res = an.anomaly(x, periods=1, outputs=('pct', 'count'))
    m = int(res.count[0, 0])
    assert m == Y
    # below / equal: 2.0 -> 2 / 3, 1.0 -> 0 / 2, 3.0 -> 5 / 1, 5.0 -> 6 / 1
    want = {2.0: (2 + 1.5) / 7, 1.0: (0 + 1.0) / 7, 3.0: (5 + 0.5) / 7, 5.0: (6 + 0.5) / 7}
    assert [res.pct[y, 0] for y in range(Y)] == [want[float(v)] for v in x[:, 0]]
    steps = res.pct[:, 0] * m / 0.5
    assert np.array_equal(steps, np.rint(steps))
    assert res.z is None and res.mean is None and res.std is None


def test_window_runs_across_the_year_boundary_and_its_first_slabs_are_missing():
    Y, P, W = 3, 4, 3
    rng = np.random.default_rng(1)
    num = rng.uniform(1, 2, (Y * P, 1))
    den = rng.uniform(2, 3, (Y * P, 1))
    r = an.windowed(num, den, W)
    assert np.isnan(r[:W - 1]).all() and np.isfinite(r[W - 1:]).all()
    s = 1 * P + 0                                    # period 0 of year 1: two terms from year 0
    assert r[s, 0] == ((0.0 + num[s - 2, 0]) + num[s - 1, 0] + num[s, 0]) / ((0.0 + den[s - 2, 0]) + den[s - 1, 0] + den[s, 0])
    res = an.anomaly(num, den, periods=P, window=W, min_valid=2, outputs=ALL)
    assert np.isnan(res.z[:W - 1]).all() and np.isnan(res.pct[:W - 1]).all()
    assert list(res.count[:, 0]) == [2, 2, 3, 3]          # periods 0 and 1 lose year 0
    assert np.isfinite(res.z[W - 1:]).all()
    alone = an.anomaly(num, periods=P, window=W, min_valid=2, outputs=('mean',))
    rr = an.windowed(num, None, W)
    assert rr[s, 0] == num[s - 2, 0] + num[s - 1, 0] + num[s, 0]
    assert alone.mean[2, 0] == ((rr[2, 0] + rr[6, 0]) + rr[10, 0]) / 3.0


def test_one_nan_removes_exactly_window_values():
    Y, P, W = 4, 5, 3
    num = np.random.default_rng(2).uniform(1, 2, (Y * P, 1))
    num[8, 0] = np.nan
    r = an.windowed(num, None, W)
    missing = np.flatnonzero(np.isnan(r[:, 0]))
    assert list(missing) == [0, 1, 8, 9, 10]


@pytest.mark.parametrize('what', ['den == 0', 'den < 0', 'num = inf', 'den = inf', 'num = nan'])
def test_missing_cases(what):
    Y, P = 5, 2
    rng = np.random.default_rng(3)
    num = rng.uniform(1, 2, (Y * P, 1))
    den = rng.uniform(2, 3, (Y * P, 1))
    s = 2 * P + 1
    if what == 'den == 0':
        den[s] = 0.0
    elif what == 'den < 0':
        den[s] = -3.0
    elif what == 'num = inf':
        num[s] = np.inf
    elif what == 'den = inf':
        den[s] = np.inf                              # the ratio would be the finite 0.0: b < inf keeps it out
    else:
        num[s] = np.nan
    res = an.anomaly(num, den, periods=P, outputs=ALL)
    assert res.count[1, 0] == Y - 1 and res.count[0, 0] == Y
    assert np.isnan(res.z[s, 0]) and np.isnan(res.pct[s, 0])
    others = [y * P + 1 for y in range(Y) if y != 2]
    assert np.isfinite(res.z[others]).all() and np.isfinite(res.pct[others]).all()
    r = an.windowed(num, den, 1)
    keep = r[others, 0]
    assert res.mean[1, 0] == sum_in_order(keep) / 4.0


def sum_in_order(v):
    s = np.float64(0.0)
    for e in v:
        s = s + e
    return s


def test_an_overflowing_window_sum_is_missing():
    num = np.full((4, 1), 1.0)
    num[2:] = np.finfo(np.float64).max
    res = an.anomaly(num, periods=2, window=2, min_valid=2, outputs=('count',))
    assert list(res.count[:, 0]) == [1, 1]              # slab 0: no window; slab 3: max + max overflows


def test_a_year_outside_the_baseline_still_gets_z_and_pct():
    Y, P = 8, 2
    x = np.random.default_rng(4).uniform(1, 2, (Y * P, 3))
    x[7 * P:] += 10.0                                # the last year lies far above the baseline
    res = an.anomaly(x, periods=P, baseline=(1, 6), outputs=ALL)
    assert (res.count == 5).all()
    assert np.isfinite(res.z).all() and np.isfinite(res.pct).all()
    assert (res.pct[7 * P:] == 1.0).all() and (res.z[7 * P:] > 5).all()       # eq = 0 outside: lt / m = 1
    inside = an.anomaly(x[P:6 * P], periods=P, outputs=ALL)
    assert same(inside.mean, res.mean) and same(inside.std, res.std)
    assert same(inside.z, res.z[P:6 * P]) and same(inside.pct, res.pct[P:6 * P])


def test_too_few_valid_values_give_nan_but_a_count():
    Y, P = 5, 1
    x = np.arange(1.0, 6.0)[:, None].repeat(2, 1)
    x[:3, 1] = np.nan
    res = an.anomaly(x, periods=P, min_valid=3, outputs=ALL)
    assert list(res.count[0]) == [5, 2]
    assert np.isfinite(res.mean[0, 0]) and np.isnan(res.mean[0, 1]) and np.isnan(res.std[0, 1])
    assert np.isnan(res.z[:, 1]).all() and np.isnan(res.pct[:, 1]).all()


@pytest.mark.parametrize('Y', [8, 24, 64])
def test_against_numpys_own_reductions(Y):
    """window = 1, nothing missing: mean and std against np.mean / np.std(ddof=1) over the year axis.
    Relative tolerance 1e-12: two orders of magnitude above the two-pass algorithm's rounding bound of
    about Y * 2^-53 (7e-15 at Y = 64), so only a wrong formula can exceed it."""
    P, n = 5, 40
    x = np.random.default_rng(Y).uniform(0.2, 1.2, (Y * P, n))
    res = an.anomaly(x, periods=P, outputs=ALL)
    cube = x.reshape(Y, P, n)
    mean, std = np.mean(cube, axis=0), np.std(cube, axis=0, ddof=1)
    assert (res.count == Y).all()
    assert np.max(np.abs(res.mean - mean) / np.abs(mean)) < 1e-12
    assert np.max(np.abs(res.std - std) / std) < 1e-12


def recipe(Y, P, n, seed):
    rng = np.random.default_rng(seed)
    S = Y * P
    num = rng.gamma(4.0, 5.0, (S, n))
    den = num + rng.gamma(4.0, 8.0, (S, n))
    num[:, 1::2] = np.round(num[:, 1::2])
    den[:, 1::2] = np.round(den[:, 1::2]) + 1
    num[rng.uniform(0, 1, (S, n)) < 0.1] = np.nan
    return num, den


@pytest.mark.parametrize('W,base', [(1, None), (4, (2, 10))])
def test_scaling_by_a_power_of_two_changes_no_bit(W, base):
    Y, P, n = 12, 5, 60
    num, den = recipe(Y, P, n, 5)
    ref = an.anomaly(num, den, periods=P, window=W, baseline=base, outputs=('z', 'pct'))
    assert np.isfinite(ref.z).mean() > 0.4
    for f in (8.0, 0.25):
        got = an.anomaly(num * f, den * f, periods=P, window=W, baseline=base, outputs=('z', 'pct'))
        assert same(got.z, ref.z) and same(got.pct, ref.pct)
    alone = an.anomaly(num, periods=P, window=W, baseline=base, outputs=('z', 'pct'))
    for f in (8.0, 0.25):
        got = an.anomaly(num * f, periods=P, window=W, baseline=base, outputs=('z', 'pct'))
        assert same(got.z, alone.z) and same(got.pct, alone.pct)


def test_float32_input_is_the_float64_definition_rounded_once():
    Y, P, n = 9, 3, 50
    num, den = recipe(Y, P, n, 6)
    f, g = num.astype(np.float32), den.astype(np.float32)
    got = an.anomaly(f, g, periods=P, window=2, outputs=ALL)
    wide = an.anomaly(f.astype(np.float64), g.astype(np.float64), periods=P, window=2, outputs=ALL)
    assert got.z.dtype == np.float32 and got.pct.dtype == np.float32
    assert same(got.z, wide.z.astype(np.float32)) and same(got.pct, wide.pct.astype(np.float32))
    assert same(got.mean, wide.mean) and same(got.std, wide.std) and np.array_equal(got.count, wide.count)


def test_the_full_baseline_is_the_default_and_cubes_keep_their_shape():
    Y, P = 6, 4
    num, den = recipe(Y, P, 30, 7)
    a = an.anomaly(num, den, periods=P, outputs=ALL)
    b = an.anomaly(num, den, periods=P, baseline=(0, Y), outputs=ALL)
    assert all(same(p, q) for p, q in zip(a, b))
    c = an.anomaly(num.reshape(Y * P, 5, 6), den.reshape(Y * P, 5, 6), periods=P, outputs=ALL)
    assert c.z.shape == (Y * P, 5, 6) and c.mean.shape == (P, 5, 6) and c.count.shape == (P, 5, 6)
    assert all(same(p.reshape(q.shape), q) for p, q in zip(c, a))
    assert an.anomaly(num, periods=P).z is not None          # every output by default


@pytest.mark.parametrize('shape,kwargs', [
    ((), dict(periods=1)),
    ((10, 3), dict(periods=0)),
    ((10, 3), dict(periods=367)),
    ((10, 3), dict(periods=2.0)),
    ((10, 3), dict(periods=True)),
    ((10, 3), dict(periods=3)),                      # S is no multiple of P
    ((5, 3), dict(periods=5)),                       # Y = 1
    ((65 * 2, 3), dict(periods=2)),                  # Y = 65
    ((64 * 65, 3), dict(periods=65)),                # S = 4160 > 4096
    ((10, 3), dict(periods=5, window=0)),
    ((10, 3), dict(periods=5, window=6)),            # above P
    ((40, 3), dict(periods=20, window=17)),          # above 16
    ((10, 3), dict(periods=5, window=1.5)),
    ((20, 3), dict(periods=5, baseline=(0, 5))),     # y1 > Y
    ((20, 3), dict(periods=5, baseline=(-1, 3))),
    ((20, 3), dict(periods=5, baseline=(2, 2))),
    ((20, 3), dict(periods=5, baseline=(3, 2))),
    ((20, 3), dict(periods=5, baseline=(1, 2))),     # one year
    ((20, 3), dict(periods=5, baseline=3)),
    ((20, 3), dict(periods=5, baseline=(0, 2.5))),
    ((20, 3), dict(periods=5, min_valid=1)),
    ((20, 3), dict(periods=5, min_valid=5)),         # above Y = 4
    ((20, 3), dict(periods=5, baseline=(1, 3), min_valid=3)),
    ((20, 3), dict(periods=5, min_valid=2.0)),
])
def test_check_call_refuses(shape, kwargs):
    with pytest.raises(ValueError):
        an.check_call(shape, **kwargs)


def test_check_call_returns_and_the_other_checks():
    assert an.check_call((20, 4, 5), 5) == (4, 5, (4, 5), 1, (0, 4), 3)
    assert an.check_call((20,), np.int64(5), 5, (1, 4), 2) == (4, 5, (), 5, (1, 4), 2)
    assert an.check_call((64 * 64, 1), 64, 16) [0] == 64
    assert an.check_dtype('float32') == np.float32 and an.check_dtype(np.float64, np.float64) == np.float64
    for bad in (np.float16, np.int32, 'complex128'):
        with pytest.raises(ValueError):
            an.check_dtype(bad)
    with pytest.raises(ValueError):
        an.check_dtype(np.float32, np.float64)
    assert an.check_outputs(('pct', 'z')) == ('z', 'pct') and an.check_outputs('count') == ('count',)
    for bad in ((), ('z', 'z'), ('zscore',)):
        with pytest.raises(ValueError):
            an.check_outputs(bad)
    x = np.ones((20, 3))
    with pytest.raises(ValueError):
        an.anomaly(x, np.ones((20, 4)), periods=5)
    with pytest.raises(ValueError):
        an.anomaly(x, np.ones((20, 3), np.float32), periods=5)
    with pytest.raises(ValueError):
        an.anomaly(x)                                # periods must be given
    with pytest.raises(ValueError):
        an.anomaly(x.astype(np.int32), periods=5)


def header_struct(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, flags=re.S).group(1)
    types = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), types[ctype]) for n in names.split(',')]
    return fields


def test_abi_symbols_spec_layout_and_capacity():
    import mod16_amd
    from mod16_amd import _lib
    text = open(HEADER).read()
    names = ('mod16_anomaly_f32', 'mod16_anomaly_f64', 'mod16_anomaly_max_window')
    for name in names:
        assert re.search(r'MOD16_API int %s\(' % name, text) and name in _lib.PROTOTYPES
    for name in names[:2]:
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == 12
        assert args[1] is ctypes.POINTER(_lib.AnomalySpec) and args[11] is ctypes.c_size_t
    fields = header_struct('mod16_anomaly_spec')
    assert fields == list(_lib.AnomalySpec._fields_)

    class Twin(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(_lib.AnomalySpec) == ctypes.sizeof(Twin) == 56
    assert callable(_lib.Context.anomaly) and callable(mod16_amd.anomaly_series)
    lib = _lib.load()
    assert lib.mod16_anomaly_max_window() == 16 == an.MAX_WINDOW
    for name in names[:2]:
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
        # a NULL context (and with it a NULL spec) is refused before anything is looked at
        assert getattr(lib, name)(None, None, None, None, None, None, None, None, None, 0, None, 0) == _lib.ERR_ARG


def test_the_numpy_entry_point_checks_before_it_needs_a_device():
    import mod16_amd
    x = np.ones((20, 3))
    for kwargs in (dict(periods=3), dict(periods=5, window=6), dict(periods=5, baseline=(0, 9)),
                   dict(periods=5, min_valid=1), dict(periods=5, outputs=('zz',)), dict(periods=5, stage_bytes=-1), dict()):
        with pytest.raises(ValueError):
            mod16_amd.anomaly_series(x, **kwargs)
    with pytest.raises(ValueError):
        mod16_amd.anomaly_series(x.astype(np.float16), periods=5)
    with pytest.raises(ValueError):
        mod16_amd.anomaly_series(x, np.ones((20, 4)), periods=5)
    empty = mod16_amd.anomaly_series(np.ones((20, 0)), periods=5, outputs=('z', 'count'))
    assert empty.z.shape == (20, 0) and empty.count.shape == (5, 0) and empty.pct is None
