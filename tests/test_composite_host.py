"""mod16_amd.composite -- the numpy definition of the multi-day composites (slab_index, daily_total,
composite_reduce) against explicit Python loops over scalars, and the argument checks of the
composite calls, all without a device: nothing here loads the library."""
import math

import numpy as np
import pytest

from mod16_amd import composite as cp


def loop_reduce(daily, L, min_valid, rescale):
    """composite_reduce, one Python float at a time."""
    K, n = daily.shape
    P = -(-K // L)
    total = np.empty((P, n))
    count = np.empty((P, n), np.uint16)
    for i in range(n):
        for p in range(P):
            lo, hi = p * L, min((p + 1) * L, K)
            s, c = 0.0, 0
            for t in range(lo, hi):
                v = float(daily[t, i])
                if not math.isnan(v):
                    s = s + v
                    c += 1
            if c < min_valid:
                r = math.nan
            elif rescale:
                r = s * (float(hi - lo) / float(c))
            else:
                r = s
            total[p, i] = r
            count[p, i] = c
    return total, count


def series(K, n, seed, nan_fraction=0.2):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 5.0, (K, n)) * 10.0 ** rng.integers(-3, 3, (K, n))
    d[rng.uniform(0, 1, (K, n)) < nan_fraction] = np.nan
    d[:, 0] = np.nan                      # a pixel without a valid day
    d[:, 1] = rng.uniform(0, 1, K)        # a pixel without a missing one
    if K >= 2:
        d[0, 2], d[1, 2] = np.inf, -np.inf    # inf - inf: NaN as a SUM, though both days are valid
    d[:, 3] = -0.0                        # +0.0 + -0.0 = +0.0
    return d


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


@pytest.mark.parametrize('K,L', [(19, 8), (16, 8), (8, 8), (1, 1), (5, 7), (23, 1), (11, 3)])
@pytest.mark.parametrize('min_valid,rescale', [(1, False), (1, True), (3, False), (3, True)])
def test_composite_reduce_is_the_sequential_loop(K, L, min_valid, rescale):
    if min_valid > L:
        with pytest.raises(ValueError, match='min_valid'):
            cp.composite_reduce(series(K, 5, 1), L, min_valid, rescale)
        return
    d = series(K, 29, seed=K * 100 + L)
    total, count = cp.composite_reduce(d, L, min_valid, rescale)
    want_total, want_count = loop_reduce(d, L, min_valid, rescale)
    P = -(-K // L)
    assert total.shape == (P, 29) and total.dtype == np.float64
    assert count.shape == (P, 29) and count.dtype == np.uint16
    assert np.array_equal(count, want_count)
    assert same(total, want_total)
    # the partial last period counts its own days only
    last = K - (P - 1) * L
    assert count[-1].max() <= last and count[-1, 1] == last
    assert np.isnan(total[:, 0]).all() and (count[:, 0] == 0).all()
    kept = count[:, 3] >= min_valid
    assert (total[kept, 3] == 0).all() and not np.signbit(total[kept, 3]).any() and np.isnan(total[~kept, 3]).all()
    if K >= 2 and L >= 2:
        assert np.isnan(total[0, 2]) and count[0, 2] >= 2      # inf + -inf, both days counted


def test_composite_reduce_keeps_leading_shape_and_rescales_by_length_over_count():
    d = np.array([[1.0, np.nan], [2.0, 4.0], [np.nan, np.nan], [8.0, np.nan], [16.0, 1.0]]).reshape(5, 1, 2)
    total, count = cp.composite_reduce(d, 4)
    assert total.shape == (2, 1, 2) and count.shape == (2, 1, 2)
    assert total[:, 0].tolist() == [[11.0, 4.0], [16.0, 1.0]]
    assert count[:, 0].tolist() == [[3, 1], [1, 1]]
    scaled, _ = cp.composite_reduce(d, 4, rescale=True)
    assert scaled[:, 0].tolist() == [[11.0 * (4.0 / 3.0), 4.0 * (4.0 / 1.0)], [16.0, 1.0]]
    strict, _ = cp.composite_reduce(d, 4, min_valid=2)
    assert np.isnan(strict[0, 0, 1]) and strict[0, 0, 0] == 11.0 and np.isnan(strict[1]).all()


def test_daily_total_is_left_to_right_in_float64():
    rng = np.random.default_rng(5)
    day = rng.uniform(0, 1e-4, 200)
    night = rng.uniform(0, 1e-5, 200)
    hours = rng.uniform(6, 18, 200)
    got = cp.daily_total(day, night, hours)
    want = np.array([((float(d) * float(h)) * 3600.0) + ((float(g) * (24.0 - float(h))) * 3600.0)
                     for d, g, h in zip(day, night, hours)])
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # float32 inputs are widened before the arithmetic, not after
    d32, g32, h32 = day.astype(np.float32), night.astype(np.float32), hours.astype(np.float32)
    got32 = cp.daily_total(d32, g32, h32)
    want32 = cp.daily_total(d32.astype(np.float64), g32.astype(np.float64), h32.astype(np.float64))
    assert got32.dtype == np.float64 and np.array_equal(got32.view(np.uint64), want32.view(np.uint64))
    assert np.isnan(cp.daily_total(np.nan, 1.0, 12.0)) and np.isnan(cp.daily_total(1.0, 1.0, np.nan))
    assert cp.daily_total(1.0, 0.0, 24.0) == 86400.0


def test_slab_index_and_counts():
    for every in (1, 2, 7, 8, 19, 4096):
        for t in range(0, 40):
            want = 0
            while (want + 1) * every <= t:
                want += 1
            assert cp.slab_index(t, every) == want
        for days in (1, 7, 8, 9, 19, 368):
            assert cp.slab_count(days, every) == cp.slab_index(days - 1, every) + 1
    assert cp.period_bounds(19, 8) == [(0, 8), (8, 16), (16, 19)]
    assert cp.period_bounds(8, 8) == [(0, 8)]
    assert cp.check_periods(4096, 365, 365) == (4096, 365, 365, 12)


@pytest.mark.parametrize('call', [
    lambda: cp.slab_index(-1, 8),
    lambda: cp.slab_index(3, 0),
    lambda: cp.slab_index(3.0, 8),
    lambda: cp.slab_count(0, 8),
    lambda: cp.check_periods(0, 8),
    lambda: cp.check_periods(4097, 8),
    lambda: cp.check_periods(19, 0),
    lambda: cp.check_periods(19, 8, 0),
    lambda: cp.check_periods(19, 8, 9),
    lambda: cp.check_periods(19.5, 8),
    lambda: cp.check_periods(19, 8, True),
    lambda: cp.check_every({'fpar': 0}),
    lambda: cp.check_every({'fpar': 8.0}),
    lambda: cp.check_every({'fpar': 2 ** 31}),
    lambda: cp.check_every({'ndvi': 8}),
    lambda: cp.check_every([8] * 15),
    lambda: cp.check_slabs('fpar', 2, 19, 8),
    lambda: cp.check_slabs('temp_day', 18, 19, 1),
    lambda: cp.composite_reduce(np.float64(1.0), 8),
    lambda: cp.composite_reduce(np.zeros((0, 4)), 8),
    lambda: cp.composite_reduce(np.zeros((4, 4)), 8, min_valid=9),
])
def test_validation_raises_value_error(call):
    with pytest.raises(ValueError):
        call()


def test_check_every_fills_in_the_daily_default():
    full = cp.check_every(None)
    assert tuple(full) == cp.ARRAY_NAMES and set(full.values()) == {1}
    full = cp.check_every({'fpar': 8, 'lai': np.int64(8), 'day_hours': 2})
    assert full['fpar'] == 8 and full['lai'] == 8 and full['day_hours'] == 2 and full['temp_day'] == 1
    assert len(cp.ARRAY_NAMES) == 15 and cp.ARRAY_NAMES[-1] == 'day_hours'
    cp.check_slabs('fpar', 3, 19, 8)
    assert cp.check_every({'pressure': 2 ** 31 - 1})['pressure'] == 2 ** 31 - 1


def test_numpy_entry_point_checks_its_arguments_before_any_device_call():
    """evapotranspiration_composite raises ValueError for every bad argument with no device present:
    the checks come before the context is created."""
    import mod16_amd
    import mod16
    assert mod16.evapotranspiration_composite is mod16_amd.evapotranspiration_composite
    n, K = 6, 19
    table = np.ones((13, 11))
    cls = np.ones(n, np.uint8)
    daily = np.ones((K, n))
    base = [daily] * 4 + [np.ones((3, n))] + [daily] * 2 + [np.ones(n)] + [daily] * 3 + [1e5, np.ones((3, n)), np.ones((3, n))]
    every = {'sw_albedo': 8, 'fpar': 8, 'lai': 8}
    call = mod16_amd.evapotranspiration_composite

    def bad(match, drivers=base, hours=daily, **kw):
        kw.setdefault('every', every)
        with pytest.raises(ValueError, match=match):
            call(table, cls, *drivers, hours, **kw)
    bad('time slabs', every=None)                                   # the 8-day arrays have 3 slabs, not 19
    bad('time slabs', days=20)
    bad('days must be between', days=0)
    bad('period_days', period_days=0)
    bad('min_valid', min_valid=9)
    bad('min_valid', min_valid=0)
    bad('not one of', every={'ndvi': 8})
    bad('between 1 and', every={'fpar': 0})
    bad('expected a scalar', drivers=[np.ones((K, n + 1))] + base[1:])
    bad('expected a scalar', drivers=[np.ones((2, K, n))] + base[1:])
    bad('expected a scalar', hours=np.ones(n + 1))
    bad('MATH_FAST or MATH_EXACT', math=2)
    bad('MATH_FAST or MATH_EXACT', math=4)
    bad('stage_bytes', stage_bytes=-1)
    bad('out must hold', out=[np.empty((3, n))])
    bad('out\\[1\\]', out=[np.empty((3, n)), np.empty((3, n))])      # the count is uint16
    bad('out\\[0\\]', out=[np.empty((2, n)), np.empty((3, n), np.uint16)])
    bad('days is required', drivers=[1.0] * 4 + [base[4]] + [1.0] * 7 + base[12:], hours=12.0)


def test_numpy_entry_point_marshals_scalars_slabs_and_constants(monkeypatch):
    """What evapotranspiration_composite hands to the library, seen by a stand-in context: a scalar is
    one value with pixel stride 0 and a divisor of `days`, an array of the pixel shape is constant, an
    array with a time axis has its slabs n elements apart and its own divisor."""
    import mod16_amd
    from mod16_amd import _lib
    seen = {}

    class Ctx(object):
        def set_bplut(self, table):
            seen['table'] = table

        def composite(self, dtype, n, days, period_days, cls, arrays, pixel_stride, time_stride, every, *outs, **kw):
            seen.update(dtype=dtype, n=n, days=days, period_days=period_days, arrays=arrays, pixel_stride=pixel_stride,
                        time_stride=time_stride, every=every, outs=outs, kw=kw)
    monkeypatch.setattr(_lib, 'context', lambda device=0: Ctx())
    n, K = 6, 19
    daily = np.ones((K, 2, 3), np.float32)
    slow = np.ones((3, 2, 3), np.float32)
    const = np.ones((2, 3), np.float32)
    drivers = [daily] * 3 + [0.0, slow] + [daily] * 2 + [const] + [daily] * 3 + [const, slow, slow]
    et, count = mod16_amd.evapotranspiration_composite(np.ones((13, 11)), np.ones((2, 3), np.uint8), *drivers, daily,
                                                       every={'sw_albedo': 8, 'fpar': 8, 'lai': 8}, min_valid=2, rescale=True)
    assert et.shape == (3, 2, 3) and et.dtype == np.float32 and count.shape == (3, 2, 3) and count.dtype == np.uint16
    assert (seen['n'], seen['days'], seen['period_days']) == (n, K, 8) and seen['dtype'] == np.float32
    assert seen['pixel_stride'] == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert seen['time_stride'] == [n, n, n, 0, n, n, n, 0, n, n, n, 0, n, n, n]
    assert seen['every'] == [1, 1, 1, K, 8, 1, 1, K, 1, 1, 1, K, 8, 8, 1]
    assert seen['outs'][:4] == (et.ctypes.data, None, count.ctypes.data, None) and seen['outs'][4] == n
    assert seen['kw']['min_valid'] == 2 and seen['kw']['rescale'] is True and seen['kw']['where'] == _lib.HOST
