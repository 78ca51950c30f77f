'''
Per-pixel climatology, standardized anomalies and percentile ranks over a record of composites: the
numpy statement of what ``mod16_anomaly_f32`` / ``mod16_anomaly_f64`` compute (``RasterEngine.anomaly``,
``mod16_amd.anomaly_series``), and the argument checks of those calls. Host only: nothing here touches
the library or a device; the kernel (``csrc/mod16_anomaly.hpp``) follows ``anomaly`` step for step and
gives its bits.

The record is ``S = Y P`` slabs in time order, years outermost: slab ``s = y P + p`` is period ``p`` of
year ``y``. Per pixel, with ``num`` (and ``den``, for a ratio such as ET / PET) widened to float64
first (exact); all arithmetic is float64, every operation rounded on its own:

- the windowed value ``r[s]``: missing for ``s < W - 1``; otherwise ``a = +0.0``, then ``a = a +
  num[k]`` for ``k = s - W + 1 ... s`` in that order, ``b`` likewise from ``den``; ``r = a / b``, or
  ``r = a`` without ``den``. ``r[s]`` is valid where ``isfinite(r)`` and, with ``den``, ``0 < b < inf``;
  everything else is missing. (NaN or an infinity anywhere in the window, PET <= 0 and an overflowing
  sum all land in "missing": by IEEE arithmetic alone but for a finite ``a`` over an infinite ``b``,
  whose ratio 0.0 only the upper bound on ``b`` keeps out.)
- the climatology of period ``p`` over the baseline years ``y0 ... y1 - 1`` in year order: ``m`` the
  number of valid ``r[y P + p]``, ``sum`` their sequential sum from ``+0.0``, ``mean = sum / float(m)``,
  ``ss`` the sequential sum from ``+0.0`` of ``e * e`` with ``e = r - mean`` (the product rounded, then
  added), ``std = sqrt(ss / float(m - 1))``. ``count[p] = m``; ``mean[p]`` and ``std[p]`` are NaN where
  ``m < min_valid``.
- per slab ``s = y P + p`` of every year, inside the baseline or not: ``z[s] = (r[s] - mean) / std``
  where ``r[s]`` is valid, ``m >= min_valid``, ``std`` is finite and ``std > 0``, else NaN;
  ``pct[s] = (float(lt) + 0.5 * float(eq)) / float(m)`` with ``lt`` the number of valid baseline
  values of period ``p`` below ``r[s]`` and ``eq`` the number equal to it (the mid-rank empirical
  distribution; a baseline year counts itself in ``eq``), NaN where ``r[s]`` is missing or
  ``m < min_valid``.

``z`` and ``pct`` take the dtype of ``num`` (float32: the float64 result rounded once); ``mean`` and
``std`` are float64, ``count`` uint8. Scaling ``num`` and ``den`` by one power of two, or ``num`` alone
without ``den``, changes no bit of ``z`` and ``pct`` (tests/test_anomaly_host.py).
'''
import collections

import numpy as np

MAX_WINDOW = 16                                    # mod16_anomaly_max_window()
MAX_PERIODS = 366
MAX_YEARS = 64
MAX_SLABS = 4096                                   # the composite's MAX_DAYS
OUTPUT_NAMES = ('z', 'pct', 'mean', 'std', 'count')
Anomaly = collections.namedtuple('Anomaly', OUTPUT_NAMES)


def _integer(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (what, v))
    return int(v)


def check_call(shape, periods, window=1, baseline=None, min_valid=3):
    '''The checks ``anomaly_series``, ``RasterEngine.anomaly`` and ``anomaly`` share, on the shape of
    ``num`` alone: -> ``(Y, P, pixel shape, W, (y0, y1), min_valid)``.'''
    shape = tuple(int(e) for e in shape)
    if periods is None:
        raise ValueError('periods must be given')
    P = _integer(periods, 'periods')
    if not 1 <= P <= MAX_PERIODS:
        raise ValueError('periods must be between 1 and %d, got %d' % (MAX_PERIODS, P))
    if len(shape) < 1 or shape[0] % P or not 2 * P <= shape[0] <= MAX_YEARS * P:
        raise ValueError('num must have shape (S,) + pixel shape with S = Y * periods and 2 <= Y <= %d, got %r with '
                         'periods = %d' % (MAX_YEARS, shape, P))
    if shape[0] > MAX_SLABS:
        raise ValueError('num must have at most %d slabs, got %d' % (MAX_SLABS, shape[0]))
    Y = shape[0] // P
    W = _integer(window, 'window')
    if not 1 <= W <= min(P, MAX_WINDOW):
        raise ValueError('window must be between 1 and min(periods, %d) = %d, got %d' % (MAX_WINDOW, min(P, MAX_WINDOW), W))
    if baseline is None:
        y0, y1 = 0, Y
    else:
        try:
            y0, y1 = baseline
        except (TypeError, ValueError):
            raise ValueError('baseline must be None or a pair (y0, y1), got %r' % (baseline,))
        y0, y1 = _integer(y0, 'baseline[0]'), _integer(y1, 'baseline[1]')
    if not 0 <= y0 < y1 <= Y:
        raise ValueError('baseline must satisfy 0 <= y0 < y1 <= Y = %d, got %r' % (Y, (y0, y1)))
    if y1 - y0 < 2:
        raise ValueError('the baseline needs at least 2 years, got %r' % ((y0, y1),))
    mv = _integer(min_valid, 'min_valid')
    if not 2 <= mv <= y1 - y0:
        raise ValueError('min_valid must be between 2 and the baseline length %d, got %d' % (y1 - y0, mv))
    return Y, P, shape[1:], W, (y0, y1), mv


def check_dtype(dtype, den_dtype=None):
    '''-> the numpy dtype of ``num``: float32 or float64, nothing else; ``den`` must have the same.'''
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('num must be float32 or float64, got %s' % dtype)
    if den_dtype is not None and np.dtype(den_dtype) != dtype:
        raise ValueError('den must have the dtype of num (%s), got %s' % (dtype, np.dtype(den_dtype)))
    return dtype


def check_den_shape(shape, den_shape):
    if tuple(den_shape) != tuple(shape):
        raise ValueError('den must have the shape of num %r, got %r' % (tuple(shape), tuple(den_shape)))


def output_table(names, S, P, shape, dtype):
    '''What a call produces, in the order of ``OUTPUT_NAMES``: name -> ``(shape, numpy dtype)`` for the
    requested ``names``, with ``shape`` the pixel shape and ``dtype`` that of ``num``.'''
    kinds = dict(z=(S, dtype), pct=(S, dtype), mean=(P, np.float64), std=(P, np.float64), count=(P, np.uint8))
    return {k: ((kinds[k][0],) + tuple(shape), np.dtype(kinds[k][1])) for k in OUTPUT_NAMES if k in names}


def check_outputs(outputs):
    '''-> the requested names in the order of ``OUTPUT_NAMES``; at least one, no unknown one, none twice.'''
    if isinstance(outputs, str):
        outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or len(set(outputs)) != len(outputs) or any(k not in OUTPUT_NAMES for k in outputs):
        raise ValueError('outputs must name one or more of %s, each once, got %r' % (', '.join(OUTPUT_NAMES), outputs))
    return tuple(k for k in OUTPUT_NAMES if k in outputs)


def windowed(x, d, W):
    '''``r`` of the module docstring: ``x`` (and ``d`` or None) float64 ``(S, n)`` -> ``(S, n)``, NaN
    where missing.'''
    S, n = x.shape
    r = np.full((S, n), np.nan)
    with np.errstate(all='ignore'):
        for s in range(W - 1, S):
            a = np.zeros(n)
            b = np.zeros(n)
            for k in range(s - W + 1, s + 1):
                a = a + x[k]
                if d is not None:
                    b = b + d[k]
            v = a / b if d is not None else a
            ok = np.isfinite(v) & (b > 0) & (b < np.inf) if d is not None else np.isfinite(v)
            r[s] = np.where(ok, v, np.nan)
    return r


def anomaly(num, den=None, periods=None, window=1, baseline=None, min_valid=3, outputs=OUTPUT_NAMES):
    '''The definition over a record: ``num`` (and ``den`` or None) ``(S,) + shape``, float32 or float64
    -> ``Anomaly(z, pct, mean, std, count)``: ``z`` / ``pct`` ``(S,) + shape`` in the dtype of ``num``,
    ``mean`` / ``std`` ``(P,) + shape`` float64, ``count`` ``(P,) + shape`` uint8; None for what
    ``outputs`` does not name. Vectorised over the pixels, Python loops over time: this is the
    statement the device result is compared with, not a fast path.'''
    num = np.asarray(num)
    if den is not None:
        den = np.asarray(den)
        check_den_shape(num.shape, den.shape)
    dtype = check_dtype(num.dtype, None if den is None else den.dtype)
    Y, P, shape, W, (y0, y1), min_valid = check_call(num.shape, periods, window, baseline, min_valid)
    outputs = check_outputs(outputs)
    S = Y * P
    n = int(np.prod(shape, dtype=np.int64))
    x = num.reshape(S, n).astype(np.float64)
    d = None if den is None else den.reshape(S, n).astype(np.float64)
    r = windowed(x, d, W).reshape(Y, P, n)
    ok = ~np.isnan(r)                              # a valid r is finite
    z = np.full((Y, P, n), np.nan)
    pct = np.full((Y, P, n), np.nan)
    with np.errstate(all='ignore'):
        m = np.zeros((P, n), np.int64)
        total = np.zeros((P, n))
        for y in range(y0, y1):
            total = np.where(ok[y], total + r[y], total)
            m += ok[y]
        mf = m.astype(np.float64)
        mean = total / mf
        ss = np.zeros((P, n))
        for y in range(y0, y1):
            e = r[y] - mean
            ss = np.where(ok[y], ss + e * e, ss)
        std = np.sqrt(ss / (m - 1).astype(np.float64))
        enough = m >= min_valid
        for y in range(Y):
            v = r[y]
            lt = np.zeros((P, n), np.int64)
            eq = np.zeros((P, n), np.int64)
            for u in range(y0, y1):
                lt += r[u] < v                     # a missing value compares false either way
                eq += r[u] == v
            good = ok[y] & enough
            z[y] = np.where(good & np.isfinite(std) & (std > 0), (v - mean) / std, np.nan)
            pct[y] = np.where(good, (lt.astype(np.float64) + 0.5 * eq.astype(np.float64)) / mf, np.nan)
    res = dict(z=z, pct=pct, mean=np.where(enough, mean, np.nan), std=np.where(enough, std, np.nan), count=m)
    table = output_table(outputs, S, P, shape, dtype)
    return Anomaly(*[res[k].reshape(table[k][0]).astype(table[k][1]) if k in table else None for k in OUTPUT_NAMES])
