'''
Per-pixel weighted least squares over a stack, with shared and per-pixel terms: the definition, in
numpy, of what ``mod16_regress_f32`` / ``mod16_regress_f64`` compute (``RasterEngine.regress``,
``mod16_amd.regress_series``), and the argument checks of those calls. Host only: nothing here touches
the library or a device; the kernel (``csrc/mod16_regress.hpp``) follows ``accumulate``, ``factor``,
``solve``, ``residual_sums`` and ``inverse_diagonal`` operation for operation, in float64 and without
contraction, so the outputs are its bits.

A pixel has ``T`` samples ``y[i]`` (float32 is widened to float64 first: exact; a value that is not
finite is missing) and ``P = Ks + Kp`` predictors per sample, ``x[i][0 .. P - 1]``: first the ``Ks``
columns of ``design`` (``(T, Ks)`` float64, the same for every pixel: intercept, time, harmonics),
then the ``Kp`` per-pixel ``terms`` in the order given (stacks of ``values``' shape and dtype). ``w[i]``
is 1.0, or a float32 weight that counts where it is finite and > 0. Sample ``i`` is *valid* where
``y[i]``, every per-pixel term and the weight qualify; ``count`` is the number of valid samples.

All arithmetic is float64, every operation rounded on its own; the parentheses are the order of the
operations, a sum written ``(.. - t0) - t1 ...`` runs over its index ascending, and a term whose index
lies outside its range is absent. ``G`` is kept as its upper triangle, ``G[a][b]`` with ``b >= a``.
All accumulators start at 0.0 and the valid samples are taken in ascending ``i``:

    wx[a]   = w * x[a]                                        # pass 1, a = 0 .. P - 1
    h[a]    = h[a] + wx[a] * y
    G[a][b] = G[a][b] + wx[a] * x[b]                          # b = a .. P - 1
    Sw      = Sw + w
    Sy      = Sy + w * y

``G = L diag(d) L'`` without pivoting, column by column, ``j`` ascending, ``k`` running over ``0 .. j - 1``:

    d[j]    = (G[j][j] - (L[j][0] * L[j][0]) * d[0]) - (L[j][1] * L[j][1]) * d[1] ...
    L[i][j] = ((G[j][i] - (L[i][0] * L[j][0]) * d[0]) - (L[i][1] * L[j][1]) * d[1] ...) / d[j]      # i = j + 1 .. P - 1

The pixel is *degenerate* if for some ``j`` the test ``d[j] > 2**-40 * G[j][j]`` fails (a NaN fails
it): the pivot has lost more than 40 of its 52 bits to cancellation, or the column is zero. Then

    z[i]    = (h[i] - L[i][0] * z[0]) - L[i][1] * z[1] ...                 # i ascending, k = 0 .. i - 1
    c[i]    = z[i] / d[i]
    b[i]    = (c[i] - L[i + 1][i] * b[i + 1]) - L[i + 2][i] * b[i + 2] ...   # i descending, k = i + 1 .. P - 1

and over the samples again, ``ybar = Sy / Sw``:

    f       = (x[0] * b[0] + x[1] * b[1]) + x[2] * b[2] ...   # pass 2 (P = 1: x[0] * b[0])
    r       = y - f
    rss     = rss + w * (r * r)                               # valid samples only, ascending i
    tss     = tss + w * ((y - ybar) * (y - ybar))

    r2      = 1.0 - rss / tss
    sigma2  = rss / float64(count - P)

With ``stderr``, ``M`` being the inverse of the unit triangle ``L`` (``M[j][j] = 1.0``):

    M[i][j] = -((L[i][j] + L[i][j + 1] * M[j + 1][j]) + L[i][j + 2] * M[j + 2][j] ...)     # i = j + 1 .. P - 1, k = j + 1 .. i - 1
    inv[j]  = ((M[j][j] * M[j][j]) / d[j] + (M[j + 1][j] * M[j + 1][j]) / d[j + 1]) + ...   # k = j .. P - 1
    se[j]   = sqrt(sigma2 * inv[j])

Nothing is special-cased: ``count == P`` gives what ``0 / 0`` or ``x / 0`` gives, a constant ``y`` what
``rss / 0`` gives. Where ``count < min_valid`` or the pixel is degenerate every float output is NaN;
``count`` is kept.

The series output is in ``values``' dtype. ``'residuals'`` is ``r``, NaN where the sample is not
valid. ``'fitted'`` is ``f`` wherever every per-pixel term of the slab is finite, whether or not ``y``
or the weight is valid (with a shared-only design that is every slab: the model-based fill), NaN
elsewhere. The series is NaN everywhere for an empty or degenerate pixel.

The normal equations square the condition number of ``X``. ``harmonic_design`` centres and scales
its trend columns for that reason; uncentred columns (a year column 2000 ... 2023 next to an
intercept) are the caller's risk: they pass the pivot test and lose the digits the squaring costs.
'''
import collections

import numpy as np

MAX_STEPS = 4096                                   # mod16_regress_max_steps()
MAX_TERMS = 8                                      # mod16_regress_max_terms(): P = Ks + Kp at most
SERIES = {None: 0, 'residuals': 1, 'fitted': 2}    # enum mod16_regress_series
PIVOT_RATIO = 2.0 ** -40
Regression = collections.namedtuple('Regression', ('coef', 'stderr', 'rss', 'tss', 'r2', 'count', 'series'))


def _as_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (what, value))
    return int(value)


def check_dtype(dtype):
    '''-> the numpy dtype of ``values``: float32 or float64, nothing else.'''
    try:
        dtype = np.dtype(dtype)
    except TypeError:
        raise ValueError('values must be float32 or float64, got %r' % (dtype,))
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('values must be float32 or float64, got %s' % dtype)
    return dtype


def check_design(design, T):
    '''``design`` -> a C-contiguous ``(T, Ks)`` float64 array (None: ``(T, 0)``); ValueError unless it
    has that shape with ``Ks <= 8`` and is finite.'''
    if design is None:
        return np.zeros((T, 0), np.float64)
    try:
        d = np.ascontiguousarray(design, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('design must be numeric')
    if d.ndim != 2 or d.shape[0] != T:
        raise ValueError('design must have shape (%d, Ks), got %r' % (T, d.shape))
    if d.shape[1] > MAX_TERMS:
        raise ValueError('design has at most %d columns, got %d' % (MAX_TERMS, d.shape[1]))
    if not np.isfinite(d).all():
        raise ValueError('design must be finite')
    return d


def check_call(shape, dtype, design_shape=None, term_shapes=(), term_dtypes=(), weights_shape=None, min_valid=None,
               stderr=False, series=None):
    '''The argument checks of every regression call, on shapes and scalars only (no array is read;
    ``check_design`` reads the design).

    ``shape``: ``(T,) + pixel shape`` with ``1 <= T <= 4096``; ``dtype``: float32 or float64;
    ``design_shape``: None or ``(T, Ks)`` with ``Ks <= 8``; ``term_shapes`` / ``term_dtypes``: those of
    the ``Kp <= 8`` per-pixel terms, each equal to ``values``'; ``P = Ks + Kp`` between 1 and 8;
    ``weights_shape``: None or ``shape``; ``min_valid``: None (``P + 1``) or an int >= ``P``;
    ``series``: None, ``'residuals'`` or ``'fitted'``.

    Returns ``(T, pixel shape, Ks, Kp, min_valid, stderr, series code)``; ValueError otherwise.'''
    shape = tuple(int(e) for e in shape)
    if len(shape) < 1:
        raise ValueError('values must have a leading time axis')
    T = shape[0]
    if T < 1 or T > MAX_STEPS:
        raise ValueError('the time axis must have between 1 and %d steps, got %d' % (MAX_STEPS, T))
    dtype = check_dtype(dtype)
    Ks = 0
    if design_shape is not None:
        design_shape = tuple(design_shape)
        if len(design_shape) != 2 or design_shape[0] != T:
            raise ValueError('design must have shape (%d, Ks), got %r' % (T, design_shape))
        Ks = int(design_shape[1])
    term_shapes, term_dtypes = list(term_shapes), list(term_dtypes)
    Kp = len(term_shapes)
    if len(term_dtypes) != Kp:
        raise ValueError('every term needs a shape and a dtype')
    P = Ks + Kp
    if P < 1 or P > MAX_TERMS or Ks > MAX_TERMS:
        raise ValueError('between 1 and %d terms (design columns + per-pixel terms), got %d + %d'
                         % (MAX_TERMS, Ks, Kp))
    for k, (s, d) in enumerate(zip(term_shapes, term_dtypes)):
        if tuple(s) != shape:
            raise ValueError('terms[%d] must have the shape of values %r, got %r' % (k, shape, tuple(s)))
        try:
            same = np.dtype(d) == dtype
        except TypeError:
            same = False
        if not same:
            raise ValueError('terms[%d] must have the dtype of values (%s), got %s' % (k, dtype, d))
    if weights_shape is not None and tuple(weights_shape) != shape:
        raise ValueError('weights must have the shape of values %r, got %r' % (shape, tuple(weights_shape)))
    if min_valid is None:
        min_valid = P + 1
    min_valid = _as_int(min_valid, 'min_valid')
    if min_valid < P:
        raise ValueError('min_valid must be at least the number of terms (%d), got %d' % (P, min_valid))
    min_valid = min(min_valid, MAX_STEPS + 1)
    if not (series is None or isinstance(series, str)) or series not in SERIES:
        raise ValueError("series must be None, 'residuals' or 'fitted', got %r" % (series,))
    return T, shape[1:], Ks, Kp, min_valid, bool(stderr), SERIES[series]


def output_table(shape, T, P, dtype, stderr=False, series=0):
    '''What a call produces, in the order of ``Regression``: name -> ``(shape, numpy dtype)`` for the
    pixel ``shape``: ``coef`` (and ``stderr``) ``(P,) + shape``, ``rss``, ``tss``, ``r2`` of ``shape``,
    all float64; ``count`` uint16; ``series`` ``(T,) + shape`` in ``dtype``. No ``stderr`` / ``series``
    where they are not asked for.'''
    shape = tuple(shape)
    table = {'coef': ((P,) + shape, np.dtype(np.float64))}
    if stderr:
        table['stderr'] = ((P,) + shape, np.dtype(np.float64))
    for k in ('rss', 'tss', 'r2'):
        table[k] = (shape, np.dtype(np.float64))
    table['count'] = (shape, np.dtype(np.uint16))
    if series:
        table['series'] = ((T,) + shape, np.dtype(dtype))
    return table


def harmonic_design(times, period, harmonics=2, trend=1):
    '''A ``(T, 1 + trend + 2 * harmonics)`` float64 design for ``times`` (``(T,)``, finite): column 0
    is ones; then the powers ``1 ... trend`` of ``u = (t - mid) / half`` with ``mid = (t[0] + t[-1]) /
    2`` and ``half = (t[-1] - t[0]) / 2`` (1.0 where that is 0), so ``u`` runs over [-1, 1]; then for
    ``k = 1 ... harmonics`` ``cos(2 pi k t / period)`` and ``sin(2 pi k t / period)``. The seasonal
    amplitude of harmonic ``k`` is ``hypot(b_cos, b_sin)`` and its phase ``arctan2(b_sin, b_cos)``.

    Centred and scaled like this the columns stay close to orthogonal: a 40 - 80 % gappy 8-day record
    of 24 years (``T = 1104``) has a condition number of about 2. A raw time column (years 2000 ...
    2023) next to the intercept has one of about 1e5, which the normal equations square: uncentred
    columns are the caller's risk.'''
    t = np.ascontiguousarray(times, dtype=np.float64)
    if t.ndim != 1 or t.size < 1 or not np.isfinite(t).all():
        raise ValueError('times must be a finite (T,) sequence')
    harmonics, trend = _as_int(harmonics, 'harmonics'), _as_int(trend, 'trend')
    if harmonics < 0 or trend < 0:
        raise ValueError('harmonics and trend must not be negative')
    if not (np.ndim(period) == 0 and np.isfinite(period) and period > 0):
        raise ValueError('period must be one finite number > 0, got %r' % (period,))
    mid, half = (t[0] + t[-1]) / 2.0, (t[-1] - t[0]) / 2.0
    u = (t - mid) / (half if half != 0 else 1.0)
    cols = [np.ones_like(t)] + [u ** p for p in range(1, trend + 1)]
    for k in range(1, harmonics + 1):
        arg = 2.0 * np.pi * k * t / float(period)
        cols += [np.cos(arg), np.sin(arg)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def samples(values, design, terms=(), weights=None):
    '''``(y, x, w, valid, have_terms)`` of the module text for ``values`` ``(T,) + shape``: ``y`` and
    ``w`` float64 of that shape, ``x`` a list of ``P`` arrays (a shared column is ``(T,) + (1,) *
    len(shape)``: it broadcasts), ``valid`` and ``have_terms`` (every per-pixel term finite) bool.'''
    values = np.asarray(values)
    y = values.astype(np.float64)
    tail = (1,) * (values.ndim - 1)
    x = [design[:, a].reshape((-1,) + tail) for a in range(design.shape[1])]
    have_terms = np.ones(values.shape, bool)
    for t in terms:
        t = np.asarray(t).astype(np.float64)
        have_terms &= np.isfinite(t)
        x.append(t)
    valid = np.isfinite(y) & have_terms
    if weights is None:
        w = np.ones(values.shape, np.float64)
    else:
        w = np.asarray(weights)
        if w.dtype != np.float32:
            raise ValueError('weights must be float32, got %s' % w.dtype)
        w = w.astype(np.float64)
        with np.errstate(invalid='ignore'):
            valid &= np.isfinite(w) & (w > 0)
    return y, x, w, valid, have_terms


def accumulate(y, x, w, valid):
    '''Pass 1: ``(G, h, Sw, Sy)``; ``G`` a dict ``(a, b) -> array`` over ``b >= a``, ``h`` a list. A loop
    over the samples of elementwise float64 operations over the pixels; a sample that is not valid
    leaves every accumulator as it is.'''
    P, T = len(x), y.shape[0]
    zero = np.zeros(y.shape[1:], np.float64)
    G = {(a, b): zero for a in range(P) for b in range(a, P)}
    h = [zero] * P
    Sw = Sy = zero
    with np.errstate(all='ignore'):
        for i in range(T):
            v, wi, yi = valid[i], w[i], y[i]
            xi = [np.broadcast_to(c[i], yi.shape) for c in x]
            for a in range(P):
                wx = wi * xi[a]
                h[a] = np.where(v, h[a] + wx * yi, h[a])
                for b in range(a, P):
                    G[a, b] = np.where(v, G[a, b] + wx * xi[b], G[a, b])
            Sw = np.where(v, Sw + wi, Sw)
            Sy = np.where(v, Sy + wi * yi, Sy)
    return G, h, Sw, Sy


def factor(G, P):
    '''``(L, d, degenerate)`` of the module text: ``L`` a dict ``(i, j) -> array`` over ``i > j``.'''
    L, d = {}, [None] * P
    degenerate = False
    with np.errstate(all='ignore'):
        for j in range(P):
            dj = G[j, j]
            for k in range(j):
                dj = dj - (L[j, k] * L[j, k]) * d[k]
            d[j] = dj
            degenerate = degenerate | ~(dj > PIVOT_RATIO * G[j, j])
            for i in range(j + 1, P):
                s = G[j, i]
                for k in range(j):
                    s = s - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = s / dj
    return L, d, degenerate


def solve(L, d, h):
    '''``b`` of the module text: the forward substitution, the division, the backward substitution.'''
    P = len(d)
    b = [None] * P
    with np.errstate(all='ignore'):
        for i in range(P):
            s = h[i]
            for k in range(i):
                s = s - L[i, k] * b[k]
            b[i] = s                       # z
        for i in range(P):
            b[i] = b[i] / d[i]             # c
        for i in range(P - 1, -1, -1):
            s = b[i]
            for k in range(i + 1, P):
                s = s - L[k, i] * b[k]
            b[i] = s
    return b


def fitted_values(xi, b):
    '''``f`` of one sample: ``(x[0] * b[0] + x[1] * b[1]) + ...``, left to right.'''
    f = xi[0] * b[0]
    for a in range(1, len(b)):
        f = f + xi[a] * b[a]
    return f


def residual_sums(y, x, w, valid, b, Sw, Sy):
    '''Pass 2: ``(rss, tss, f, r)``, ``f`` and ``r`` of ``y``'s shape (every sample, valid or not).'''
    T = y.shape[0]
    zero = np.zeros(y.shape[1:], np.float64)
    rss = tss = zero
    f, r = np.empty_like(y), np.empty_like(y)
    with np.errstate(all='ignore'):
        ybar = Sy / Sw
        for i in range(T):
            v, wi, yi = valid[i], w[i], y[i]
            fi = fitted_values([np.broadcast_to(c[i], yi.shape) for c in x], b)
            ri = yi - fi
            rss = np.where(v, rss + wi * (ri * ri), rss)
            tss = np.where(v, tss + wi * ((yi - ybar) * (yi - ybar)), tss)
            f[i], r[i] = fi, ri
    return rss, tss, f, r


def inverse_diagonal(L, d):
    '''``inv`` of the module text: the diagonal of the inverse of ``L diag(d) L'``.'''
    P = len(d)
    inv = [None] * P
    with np.errstate(all='ignore'):
        for j in range(P):
            M = {j: np.ones_like(d[j])}
            for i in range(j + 1, P):
                s = L[i, j]
                for k in range(j + 1, i):
                    s = s + L[i, k] * M[k]
                M[i] = -s
            t = (M[j] * M[j]) / d[j]
            for k in range(j + 1, P):
                t = t + (M[k] * M[k]) / d[k]
            inv[j] = t
    return inv


def regress(values, design=None, terms=(), weights=None, min_valid=None, stderr=False, series=None):
    '''The definition: ``Regression(coef, stderr, rss, tss, r2, count, series)`` of ``values`` (``(T,) +
    pixel shape``); the arguments are those of ``mod16_amd.regress_series``. ``coef`` and ``stderr``
    are ``(P,) + shape``; float64 but for ``count`` (uint16) and ``series`` (``values``' dtype);
    ``stderr`` / ``series`` are None where they are not asked for.'''
    values = np.asarray(values)
    terms = [np.asarray(t) for t in terms]
    T, shape, Ks, Kp, min_valid, stderr, code = check_call(
        values.shape, values.dtype, None if design is None else np.shape(design), [t.shape for t in terms],
        [t.dtype for t in terms], None if weights is None else np.shape(weights), min_valid, stderr, series)
    design = check_design(design, T)
    P = Ks + Kp
    y, x, w, valid, have_terms = samples(values, design, terms, weights)
    count = valid.sum(axis=0)
    G, h, Sw, Sy = accumulate(y, x, w, valid)
    L, d, degenerate = factor(G, P)
    b = solve(L, d, h)
    rss, tss, f, r = residual_sums(y, x, w, valid, b, Sw, Sy)
    empty = (count < min_valid) | degenerate
    nan = np.float64(np.nan)
    with np.errstate(all='ignore'):
        r2 = 1.0 - rss / tss
        sigma2 = rss / (count - P).astype(np.float64)
        se = None
        if stderr:
            inv = inverse_diagonal(L, d)
            se = np.stack([np.where(empty, nan, np.sqrt(sigma2 * inv[j])) for j in range(P)])
    out = None
    if code:
        keep = (valid if code == SERIES['residuals'] else have_terms) & ~empty
        with np.errstate(all='ignore'):
            out = np.where(keep, r if code == SERIES['residuals'] else f, nan).astype(values.dtype)
    coef = np.stack([np.where(empty, nan, np.broadcast_to(b[j], shape)) for j in range(P)])
    return Regression(coef, se, np.where(empty, nan, rss), np.where(empty, nan, tss), np.where(empty, nan, r2),
                      count.astype(np.uint16), out)
