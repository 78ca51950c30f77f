'''
Multi-day ET composites: the definition, in numpy, of what ``mod16_et_composite_*`` computes
(``RasterEngine.composite``, ``mod16_amd.evapotranspiration_composite``), and the argument checks
of those calls. Host only: nothing here touches the library or a device; the kernel
(``csrc/mod16_composite.hpp``) follows ``daily_total`` and ``composite_reduce`` operation for
operation.

``K`` days are cut into periods of ``L`` days: period ``p`` covers days ``[p L, min((p + 1) L, K))``,
there are ``P = ceil(K / L)`` periods and the last may be short. MOD16A2 is ``L = 8``, MOD16A3
``L = K`` = the days of the year. Each of the 14 drivers, and the hours of daylight, has a divisor
``every >= 1``: day ``t`` reads the array's time slab ``t // every`` (1: daily values, 8: what 8-day
fPAR / LAI / albedo have); an array without a time axis is constant.
'''
import numpy as np

#: the arrays of a composite call that may have a time axis, in argument order
ARRAY_NAMES = (
    'lw_net_day', 'lw_net_night', 'sw_rad_day', 'sw_rad_night', 'sw_albedo',
    'temp_day', 'temp_night', 'temp_annual', 'tmin', 'vpd_day', 'vpd_night',
    'pressure', 'fpar', 'lai', 'day_hours')
MAX_DAYS = 4096
MAX_EVERY = 2 ** 31 - 1        # the library's field is an int32; a divisor of `days` or more means constant


def _as_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (what, value))
    return int(value)


def check_periods(days, period_days, min_valid=1):
    '''-> ``(K, L, min_valid, P)`` as ints; ValueError unless ``1 <= K <= 4096``, ``L >= 1`` and
    ``1 <= min_valid <= L``.'''
    K = _as_int(days, 'days')
    L = _as_int(period_days, 'period_days')
    mv = _as_int(min_valid, 'min_valid')
    if K < 1 or K > MAX_DAYS:
        raise ValueError('days must be between 1 and %d, got %d' % (MAX_DAYS, K))
    if L < 1:
        raise ValueError('period_days must be at least 1, got %d' % L)
    if mv < 1 or mv > L:
        raise ValueError('min_valid must be between 1 and period_days (%d), got %d' % (L, mv))
    return K, L, mv, -(-K // L)


def period_bounds(days, period_days):
    '''The ``P`` pairs ``(first day, one past the last day)`` of the periods.'''
    K, L, _, P = check_periods(days, period_days)
    return [(p * L, min((p + 1) * L, K)) for p in range(P)]


def check_every(every):
    '''``every`` of a composite call -> a dict with one divisor per name of ``ARRAY_NAMES``: None
    (all daily) or a mapping of some of the names to integers >= 1; ValueError otherwise.'''
    full = dict.fromkeys(ARRAY_NAMES, 1)
    if every is None:
        return full
    if not hasattr(every, 'items'):
        raise ValueError('every must be None or a mapping of array names to divisors')
    for name, value in every.items():
        if name not in full:
            raise ValueError('every names %r, which is not one of %s' % (name, ', '.join(ARRAY_NAMES)))
        value = _as_int(value, 'every[%r]' % name)
        if value < 1 or value > MAX_EVERY:
            raise ValueError('every[%r] must be between 1 and %d, got %d' % (name, MAX_EVERY, value))
        full[name] = value
    return full


def slab_count(days, every):
    '''Time slabs an array with divisor ``every`` holds for ``days`` days: ``ceil(days / every)``.'''
    days, every = _as_int(days, 'days'), _as_int(every, 'every')
    if days < 1 or every < 1:
        raise ValueError('days and every must be at least 1')
    return -(-days // every)


def slab_index(t, every):
    '''The time slab day ``t`` reads of an array with divisor ``every``: ``t // every``.'''
    t, every = _as_int(t, 't'), _as_int(every, 'every')
    if t < 0:
        raise ValueError('t must not be negative, got %d' % t)
    if every < 1:
        raise ValueError('every must be at least 1, got %d' % every)
    return t // every


def check_slabs(name, slabs, days, every):
    '''An array with a time axis of ``slabs`` entries fits ``days`` days at its divisor, or ValueError.'''
    want = slab_count(days, every)
    if int(slabs) != want:
        raise ValueError('%s has %d time slabs, expected ceil(days / every) = ceil(%d / %d) = %d'
                         % (name, slabs, days, every, want))


def daily_total(day, night, hours):
    '''One day's total [kg m-2 d-1] from the day and night rates [kg m-2 s-1] and the hours of
    daylight: ``(day * hours * 3600.0) + (night * (24.0 - hours) * 3600.0)``, left to right in
    float64 (narrower inputs are widened first).'''
    day = np.asarray(day, np.float64)
    night = np.asarray(night, np.float64)
    hours = np.asarray(hours, np.float64)
    with np.errstate(all='ignore'):
        return (day * hours * 3600.0) + (night * (24.0 - hours) * 3600.0)


def composite_reduce(daily, period_days, min_valid=1, rescale=False):
    '''Period totals of a series of daily totals.

    ``daily``: ``(K,) + shape``, one ``daily_total`` per day. A day is valid where its value is not
    NaN. Per period: ``count`` = its valid days; ``sum`` = the float64 sum of the valid values taken
    in day order from ``+0.0`` (infinities take part as numpy's arithmetic has them); the result is
    NaN where ``count < min_valid``, else ``sum``, or with ``rescale`` ``sum * (float(len) /
    float(count))`` with ``len`` the period's days -- the total of a period with missing days
    brought to its full length.

    Returns ``(total, count)``: float64 and uint16, each ``(P,) + shape``.'''
    daily = np.asarray(daily, np.float64)
    if daily.ndim < 1:
        raise ValueError('daily must have a leading time axis')
    K, L, mv, P = check_periods(daily.shape[0], period_days, min_valid)
    shape = daily.shape[1:]
    total = np.empty((P,) + shape, np.float64)
    count = np.empty((P,) + shape, np.uint16)
    with np.errstate(all='ignore'):
        for p, (lo, hi) in enumerate(period_bounds(K, L)):
            s = np.zeros(shape, np.float64)
            c = np.zeros(shape, np.uint16)
            for t in range(lo, hi):
                v = daily[t]
                ok = ~np.isnan(v)
                s = np.where(ok, s + v, s)
                c = c + ok.astype(np.uint16)
            res = s
            if rescale:
                res = s * (np.float64(hi - lo) / np.maximum(c, 1).astype(np.float64))
            total[p] = np.where(c < mv, np.nan, res)
            count[p] = c
    return total, count
