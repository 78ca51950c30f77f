'''
Per-pixel Mann-Kendall test and Theil-Sen slope over a stack of composites: the numpy statement of
what ``mod16_trend_f32`` / ``mod16_trend_f64`` compute (``RasterEngine.trend``,
``mod16_amd.trend_series``), and the argument checks of those calls. Host only: nothing here touches
the library or a device; the kernel (``csrc/mod16_trend.hpp``) follows ``pixel_trend`` step for step and
gives its bits.

Per pixel, with ``x`` the ``Y`` values (float32 is widened to float64 first: exact), ``t`` the times,
``v = isfinite(x)`` the valid steps (NaN and the infinities are missing), ``m = v.sum()`` and
``M = m (m - 1) / 2``; all arithmetic is float64, every operation rounded on its own:

- ``count = m``; where ``m < min_valid``: ``s = 0`` and the five floats are NaN.
- ``s``: the sum over valid pairs ``a < b`` of ``sign(x[b] - x[a])``.
- the slopes ``(x[b] - x[a]) / (t[b] - t[a]) + 0.0`` of the valid pairs in ascending order, ``q``
  (``+ 0.0`` turns -0.0 into 0.0: equal slopes are indistinguishable, so the order statistics do not
  depend on how ties are ordered).
- the median rule ``middle``: of ``k`` ascending values the middle one for odd ``k``, ``(lo + hi) * 0.5``
  of the two middle ones for even ``k``.
- ``slope = middle(q)``; ``intercept = middle(sort(x[v] + 0.0)) - slope * middle(t[v])``, the product
  rounded before the subtraction.
- ``V18 = m (m - 1)(2 m + 5) - sum over groups of g equal valid values of g (g - 1)(2 g + 5)`` (an
  integer), ``sigma = sqrt(V18 / 18.0)``; ``z = 0.0`` where ``s == 0`` or ``V18 == 0``, else
  ``(s - sign(s)) / sigma``.
- with ``alpha``: ``zq = NormalDist().inv_cdf(1 - alpha / 2)``, ``C = zq * sigma``,
  ``slope_hi = q[min(rint((M + C) / 2), M - 1)]``, ``slope_lo = q[max(rint((M - C) / 2) - 1, 0)]``
  (``rint`` rounds half to even); without: not produced.

Nothing is special-cased beyond this: two huge values whose difference overflows give what IEEE
arithmetic gives. ``slope`` and ``intercept`` have the bits of ``scipy.stats.theilslopes(x[v], t[v])``,
and the interval the ranks it picks (tests/test_trend_host.py).
'''
import collections
import statistics

import numpy as np

MAX_STEPS = 64                                     # mod16_trend_max_steps()
FLOAT_NAMES = ('slope', 'intercept', 'slope_lo', 'slope_hi', 'z')     # the order of the C ABI's out[5]
Trend = collections.namedtuple('Trend', ('slope', 'intercept', 'slope_lo', 'slope_hi', 's', 'z', 'count'))


def check_call(shape, times=None, min_valid=4, alpha=None):
    '''The checks ``trend_series``, ``RasterEngine.trend`` and ``trend`` share, on the shape of
    ``values`` alone: -> ``(Y, pixel shape, times as a contiguous float64 array, min_valid, zq)``;
    ``zq`` is 0.0 without ``alpha``.'''
    shape = tuple(int(e) for e in shape)
    if len(shape) < 1 or not 2 <= shape[0] <= MAX_STEPS:
        raise ValueError('values must have shape (Y,) + pixel shape with 2 <= Y <= %d, got %r' % (MAX_STEPS, shape))
    Y = shape[0]
    if times is None:
        t = np.arange(Y, dtype=np.float64)
    else:
        t = np.ascontiguousarray(times, dtype=np.float64)
        if t.shape != (Y,):
            raise ValueError('times must have shape (%d,), got %r' % (Y, t.shape))
        if not np.isfinite(t).all():
            raise ValueError('times must be finite')
        if not (np.diff(t) > 0).all():
            raise ValueError('times must be strictly increasing')
        with np.errstate(over='ignore'):
            if not np.isfinite(t[-1] - t[0]):
                raise ValueError('the span of times must be finite')
    if isinstance(min_valid, bool) or int(min_valid) != min_valid or not 2 <= int(min_valid) <= Y:
        raise ValueError('min_valid must be an integer between 2 and Y = %d, got %r' % (Y, min_valid))
    zq = 0.0
    if alpha is not None:
        if not 0.0 < float(alpha) <= 0.5:
            raise ValueError('alpha must be None or a level in (0, 0.5], got %r' % (alpha,))
        zq = statistics.NormalDist().inv_cdf(1.0 - float(alpha) / 2.0)
    return Y, shape[1:], t, int(min_valid), zq


def output_table(shape, zq):
    '''What a call produces, in the order of ``Trend``: name -> ``(shape, numpy dtype)``, every field
    of the pixel ``shape``; float64 but for ``s`` (int32) and ``count`` (uint8); no ``slope_lo`` /
    ``slope_hi`` where ``zq`` is 0.0 (no ``alpha``).'''
    kinds = dict(s=np.int32, count=np.uint8)
    return {k: (tuple(shape), np.dtype(kinds.get(k, np.float64))) for k in Trend._fields
            if zq or k not in ('slope_lo', 'slope_hi')}


def check_dtype(dtype):
    '''-> the numpy dtype of ``values``: float32 or float64, nothing else.'''
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('values must be float32 or float64, got %s' % dtype)
    return dtype


def middle(a):
    '''The median rule, of an ascending array of at least one value.'''
    k = len(a)
    lo, hi = a[(k - 1) // 2], a[k // 2]
    return lo if k % 2 else (lo + hi) * 0.5


def pixel_trend(x, t, min_valid, zq):
    '''One pixel: ``x`` and ``t`` float64 ``(Y,)`` -> ``(slope, intercept, slope_lo, slope_hi, s, z,
    count)``; ``zq`` 0.0: the interval is NaN.'''
    nan = np.float64(np.nan)
    v = np.isfinite(x)
    m = int(v.sum())
    if m < min_valid:
        return nan, nan, nan, nan, 0, nan, m
    xv, tv = x[v] + 0.0, t[v]
    a, b = np.triu_indices(m, 1)
    with np.errstate(over='ignore', invalid='ignore'):
        d = xv[b] - xv[a]
        s = int(np.sign(d).sum())
        q = np.sort(d / (tv[b] - tv[a]) + 0.0)
        M = m * (m - 1) // 2
        slope = middle(q)
        product = slope * middle(tv)
        intercept = middle(np.sort(xv)) - product
        groups = np.unique(xv, return_counts=True)[1].astype(np.int64)
        v18 = m * (m - 1) * (2 * m + 5) - int((groups * (groups - 1) * (2 * groups + 5)).sum())
        sigma = np.sqrt(np.float64(v18) / 18.0)
        z = np.float64(0.0) if s == 0 or v18 == 0 else np.float64(s - (1 if s > 0 else -1)) / sigma
        lo = hi = nan
        if zq:
            c = np.float64(zq) * sigma
            hi = q[int(min(np.rint((np.float64(M) + c) / 2.0), np.float64(M - 1)))]
            lo = q[int(max(np.rint((np.float64(M) - c) / 2.0) - 1.0, np.float64(0.0)))]
    return slope, intercept, lo, hi, s, z, m


def trend(values, times=None, min_valid=4, alpha=None):
    '''The definition over a stack: ``values`` ``(Y,) + shape``, float32 or float64 -> ``Trend`` of
    arrays of ``shape`` (float64; ``s`` int32, ``count`` uint8; ``slope_lo`` / ``slope_hi`` None
    without ``alpha``). A loop over the pixels: this is the statement the device result is compared
    with, not a fast path.'''
    values = np.asarray(values)
    check_dtype(values.dtype)
    Y, shape, t, min_valid, zq = check_call(values.shape, times, min_valid, alpha)
    n = int(np.prod(shape, dtype=np.int64))
    x = values.reshape(Y, n).astype(np.float64)
    res = {k: np.empty(n, dt) for k, (_, dt) in output_table((n,), 1.0).items()}
    for i in range(n):
        for k, v in zip(Trend._fields, pixel_trend(x[:, i], t, min_valid, zq)):
            res[k][i] = v
    return Trend(*[res[k].reshape(shape) if k in output_table(shape, zq) else None for k in Trend._fields])
