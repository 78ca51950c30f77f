'''
Whittaker smoothing of 8-day fPAR / LAI series, weighted by QC: the definition, in numpy, of what
``mod16_smooth_u8`` / ``_f32`` / ``_f64`` compute (``RasterEngine.smooth``,
``mod16_amd.smooth_series``), and the argument checks of those calls. Host only: nothing here touches
the library or a device; the kernel (``csrc/mod16_smooth.hpp``) follows ``factor``, ``solve`` and
``encode`` operation for operation, in float64 and without contraction.

A series is ``(S, n)`` values: uint8 codes as MOD15A2H distributes them (codes >= 249 are fill values)
or float32 / float64 (not finite: missing). Per pixel the smoother (Eilers 2003) solves ``(W + lam
D'D) z = W y`` with ``D`` the difference matrix of ``order`` 1 or 2 and ``W`` the diagonal of the
slabs' weights. The weights are 1, or a float32 stack ``weights`` (a slab counts where its weight is
finite and > 0), or a table looked up by the product's QC byte, ``qc_weight[qc]``. The default table is
1.0 where ``mod16_amd.gapfill.default_good()`` holds and 0.0 elsewhere; the usual graded table for
MOD15A2H -- main algorithm 1, main algorithm with saturation 0.5, back-up retrievals 0 -- is

    >>> q = np.arange(256)
    >>> usable = ((q & 1) == 0) & ((q & 4) == 0) & np.isin((q >> 3) & 3, (0, 3))
    >>> qc_weight = np.where(usable, np.select([(q >> 5) == 0, (q >> 5) == 1], [1.0, 0.5], 0.0), 0.0)

A slab without a value or without a weight > 0 is *missing*: ``w = 0`` and ``y = 0``; the smoother
interpolates it. ``count`` is the number of slabs with ``w > 0``.

The system is pentadiagonal. With ``a0, a1, a2`` the diagonals of ``D'D`` (``penalty_bands``: small
integers) it is factored as ``L diag(d) L'``, ``c`` and ``e`` being the two sub-diagonals of ``L``;
terms with an index below 0 are 0.0 and the parentheses are the order of the operations:

    d[i] = ((w[i] + lam*a0[i]) - (c[i-1]*c[i-1])*d[i-1]) - (e[i-2]*e[i-2])*d[i-2]
    c[i] = (lam*a1[i] - (d[i-1]*c[i-1])*e[i-1]) / d[i]
    e[i] = (lam*a2[i]) / d[i]
    f[i] = (w[i]*y[i] - c[i-1]*f[i-1]) - e[i-2]*f[i-2]            # i ascending
    z[i] = (f[i]/d[i] - c[i]*z[i+1]) - e[i]*z[i+2]                # i descending, terms past S - 1 are 0.0

``envelope = k`` repeats k times: ``y[t] = z[t]`` where ``w[t] > 0`` and ``z[t] > y[t]``, then the two
substitutions again with the same ``d, c, e`` -- the fit climbs towards the upper envelope, because
cloud and aerosol bias fPAR and LAI low. A pixel with ``count < min_valid`` is *unsmoothed*: NaN (255
for uint8 output) in every slab.
'''
import numpy as np

from .gapfill import FILL, default_good

MAX_SLABS = 4096
MAX_ENVELOPE = 8
IN_TYPES = ('uint8', 'float32', 'float64')
OUT_TYPES = {'uint8': 0, 'float32': 1, 'float64': 2}       # enum mod16_smooth_out
WEIGHT_NONE, WEIGHT_STACK, WEIGHT_QC = 0, 1, 2              # enum mod16_smooth_weight
_DIFF = {1: (-1.0, 1.0), 2: (1.0, -2.0, 1.0)}


def default_qc_weight():
    '''The 256-entry float64 table of the default: 1.0 where ``gapfill.default_good()`` holds.'''
    return default_good().astype(np.float64)


def _as_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (what, value))
    return int(value)


def _as_order(order):
    order = _as_int(order, 'order')
    if order not in _DIFF:
        raise ValueError('order must be 1 or 2, got %d' % order)
    return order


def penalty_bands(S, order):
    '''``(a0, a1, a2)``: the main, first and second diagonal of ``D'D`` as ``(S,)`` float64 arrays,
    ``D`` being the ``order``-th difference matrix of ``S - order`` rows (no row, all zero, where ``S
    <= order``); ``a1[i]`` is the entry ``(i, i + 1)``, ``a2[i]`` the entry ``(i, i + 2)``, zero where
    that lies outside the matrix.'''
    order = _as_order(order)
    k = _DIFF[order]
    rows = max(int(S) - order, 0)
    i = np.arange(int(S))
    bands = []
    for off in range(3):
        a = np.zeros(int(S), np.float64)
        for j in range(len(k) - off):             # row r = i - j holds k[j] in column i, k[j + off] in i + off
            a += np.where((i - j >= 0) & (i - j < rows), k[j] * k[j + off], 0.0)
        bands.append(a)
    return tuple(bands)


def check_qc_weight(qc_weight):
    '''``qc_weight`` -> a (256,) float64 table (None: the default); ValueError unless it has 256
    entries, all finite and >= 0.'''
    if qc_weight is None:
        return default_qc_weight()
    table = np.asarray(qc_weight)
    if table.shape != (256,):
        raise ValueError('qc_weight must have 256 entries (one per QC byte), got shape %r' % (table.shape,))
    try:
        table = table.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError('qc_weight must be numeric, got %s' % table.dtype)
    if not (np.isfinite(table).all() and (table >= 0).all()):
        raise ValueError('qc_weight must be finite and not negative')
    return table


def check_call(shape, in_dtype, weights_shape=None, qc_shape=None, qc_weight=None, lam=None, order=2,
               envelope=0, min_valid=3, dtype=None, scale=None):
    '''The argument checks of every smoothing call, on shapes and scalars only (no array is read).

    ``shape``: ``(S,) + pixel shape`` with ``1 <= S <= 4096``; ``in_dtype``: uint8, float32 or
    float64; ``weights_shape`` / ``qc_shape``: None or the same shape, at most one of them;
    ``qc_weight``: None or 256 finite numbers >= 0, with ``qc`` only; ``lam``: one finite number >
    0; ``order``: 1 or 2; ``envelope``: an int in 0 ... 8; ``min_valid``: an int >= ``order``;
    ``dtype``: None (the input's type), or for uint8 input 'uint8', 'float32' or 'float64'; ``scale``:
    None or one finite number, uint8 input with float output only.

    Returns ``(S, pixel shape, weight mode, table or None, lam, order, envelope, min_valid, dtype name,
    scale)``; ValueError otherwise.'''
    shape = tuple(shape)
    if len(shape) < 1:
        raise ValueError('values must have a leading time axis')
    S = shape[0]
    if S < 1 or S > MAX_SLABS:
        raise ValueError('the time axis must have between 1 and %d slabs, got %d' % (MAX_SLABS, S))
    try:
        in_name = np.dtype(in_dtype).name
    except TypeError:
        in_name = None
    if in_name not in IN_TYPES:
        raise ValueError('values must be uint8, float32 or float64, got %s' % (in_dtype,))
    if weights_shape is not None and qc_shape is not None:
        raise ValueError('weights and qc exclude each other')
    if weights_shape is not None and tuple(weights_shape) != shape:
        raise ValueError('weights must have the shape of values %r, got %r' % (shape, tuple(weights_shape)))
    if qc_shape is not None and tuple(qc_shape) != shape:
        raise ValueError('qc must have the shape of values %r, got %r' % (shape, tuple(qc_shape)))
    if qc_weight is not None and qc_shape is None:
        raise ValueError('qc_weight needs a qc layer')
    mode = WEIGHT_STACK if weights_shape is not None else WEIGHT_QC if qc_shape is not None else WEIGHT_NONE
    table = check_qc_weight(qc_weight) if mode == WEIGHT_QC else None
    if lam is None or isinstance(lam, (bool, np.bool_)) or np.ndim(lam) != 0:
        raise ValueError('lam must be one finite number > 0, got %r' % (lam,))
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        raise ValueError('lam must be one finite number > 0, got %r' % (lam,))
    if not (np.isfinite(lam) and lam > 0):
        raise ValueError('lam must be one finite number > 0, got %r' % (lam,))
    order = _as_order(order)
    envelope = _as_int(envelope, 'envelope')
    if not 0 <= envelope <= MAX_ENVELOPE:
        raise ValueError('envelope must be between 0 and %d, got %d' % (MAX_ENVELOPE, envelope))
    min_valid = _as_int(min_valid, 'min_valid')
    if min_valid < order:
        raise ValueError('min_valid must be at least the order (%d), got %d' % (order, min_valid))
    min_valid = min(min_valid, MAX_SLABS + 1)
    if dtype is None:
        name = in_name
    else:
        try:
            name = np.dtype(dtype).name
        except TypeError:
            name = None
        if name not in OUT_TYPES:
            raise ValueError("dtype must be 'uint8', 'float32' or 'float64', got %r" % (dtype,))
    if in_name != 'uint8' and name != in_name:
        raise ValueError('%s values return their own type, got dtype %r' % (in_name, dtype))
    if scale is None:
        scale = 1.0
    else:
        if in_name != 'uint8' or name == 'uint8':
            raise ValueError('scale applies to uint8 values with float output only')
        if isinstance(scale, (bool, np.bool_)) or np.ndim(scale) != 0 or not np.isfinite(scale):
            raise ValueError('scale must be one finite number, got %r' % (scale,))
        scale = float(scale)
    return S, shape[1:], mode, table, lam, order, envelope, min_valid, name, scale


def weights_of(values, weights=None, qc=None, qc_weight=None):
    '''``(y, w)``: the values and weights of every slab as float64 arrays of ``values``' shape; 0.0
    in both where the slab is missing -- a fill code (>= 249) or a value that is not finite, a weight
    that is not finite or not > 0.'''
    values = np.asarray(values)
    if values.dtype.name not in IN_TYPES:
        raise ValueError('values must be uint8, float32 or float64, got %s' % values.dtype)
    if weights is not None and qc is not None:
        raise ValueError('weights and qc exclude each other')
    if values.dtype == np.uint8:
        have = values < FILL
    else:
        have = np.isfinite(values)
    y = values.astype(np.float64)
    if weights is not None:
        w = np.asarray(weights, np.float32).astype(np.float64)
    elif qc is not None:
        w = check_qc_weight(qc_weight)[np.asarray(qc, np.uint8)]
    else:
        w = np.ones(values.shape, np.float64)
    if w.shape != values.shape:
        raise ValueError('the weights must have the shape of values %r, got %r' % (values.shape, w.shape))
    with np.errstate(invalid='ignore'):
        have = have & np.isfinite(w) & (w > 0)
    return np.where(have, y, 0.0), np.where(have, w, 0.0)


def factor(w, lam, order):
    '''``(d, c, e)`` of the module text for weights ``w`` of shape ``(S,) + pixel shape``: a loop over
    the slabs of elementwise float64 operations over the pixels. (A pixel with fewer than ``order``
    weighted slabs has a singular system: its ``d`` reaches 0 and the columns behind it hold NaN or
    infinity, without a warning; such a pixel is unsmoothed.)'''
    w = np.asarray(w, np.float64)
    lam = np.float64(lam)
    S = w.shape[0]
    a0, a1, a2 = penalty_bands(S, order)
    d, c, e = np.empty_like(w), np.empty_like(w), np.empty_like(w)
    zero = np.zeros(w.shape[1:], np.float64)
    d1 = d2 = c1 = e1 = e2 = zero
    with np.errstate(all='ignore'):
        for i in range(S):
            di = ((w[i] + lam * a0[i]) - (c1 * c1) * d1) - (e2 * e2) * d2
            ci = (lam * a1[i] - (d1 * c1) * e1) / di
            ei = (lam * a2[i]) / di
            d[i], c[i], e[i] = di, ci, ei
            d2, d1, c1, e2, e1 = d1, di, ci, e1, ei
    return d, c, e


def solve(d, c, e, w, y):
    '''``z`` of the module text: the forward and the backward substitution, slab by slab.'''
    S = d.shape[0]
    zero = np.zeros(d.shape[1:], np.float64)
    g = np.empty_like(d)
    z = np.empty_like(d)
    with np.errstate(all='ignore'):
        f1 = f2 = c1 = e1 = e2 = zero
        for i in range(S):
            fi = (w[i] * y[i] - c1 * f1) - e2 * f2
            g[i] = fi / d[i]
            f2, f1, c1, e2, e1 = f1, fi, c[i], e1, e[i]
        z1 = z2 = zero
        for i in range(S - 1, -1, -1):
            zi = (g[i] - c[i] * z1) - e[i] * z2
            z[i] = zi
            z2, z1 = z1, zi
    return z


def smooth_values(y, w, lam, order=2, envelope=0):
    '''``z``, float64, for every pixel (``min_valid`` is ``encode``'s): the factorisation, the two
    substitutions, and ``envelope`` times the lift of ``y`` and the substitutions again.'''
    y = np.array(y, np.float64)
    w = np.asarray(w, np.float64)
    d, c, e = factor(w, lam, order)
    z = solve(d, c, e, w, y)
    for _ in range(int(envelope)):
        with np.errstate(invalid='ignore'):
            lift = (w > 0) & (z > y)
        y = np.where(lift, z, y)
        z = solve(d, c, e, w, y)
    return z


def encode(z, count, min_valid=3, dtype='float64', scale=1.0):
    '''``z`` in an output type: ``T(z * scale)`` for float32 / float64, ``clip(floor(z + 0.5), 0, 248)``
    for uint8; NaN / 255 in every slab of a pixel with ``count < min_valid``.'''
    z = np.asarray(z, np.float64)
    name = np.dtype(dtype).name
    if name not in OUT_TYPES:
        raise ValueError("dtype must be 'uint8', 'float32' or 'float64', got %r" % (dtype,))
    unsmoothed = np.broadcast_to(np.asarray(count) < min_valid, z.shape)
    with np.errstate(all='ignore'):
        if name == 'uint8':
            codes = np.clip(np.floor(np.where(unsmoothed, 0.0, z) + 0.5), 0.0, 248.0)
            return np.where(unsmoothed, 255, codes.astype(np.int64)).astype(np.uint8)
        return np.where(unsmoothed, np.nan, z * np.float64(scale)).astype(name)


def smooth(values, weights=None, qc=None, qc_weight=None, lam=None, order=2, envelope=0, min_valid=3,
           dtype=None, scale=None, count=False):
    '''The definition: the smoothed series of ``values`` (``(S,) + pixel shape``) in ``dtype``, and
    with ``count`` a pair ``(smoothed, count)``, ``count`` being the uint16 number of weighted slabs
    of every pixel. The arguments are those of ``mod16_amd.smooth_series``.'''
    values = np.asarray(values)
    S, shape, mode, table, lam, order, envelope, min_valid, name, scale = check_call(
        values.shape, values.dtype, None if weights is None else np.shape(weights),
        None if qc is None else np.shape(qc), qc_weight, lam, order, envelope, min_valid, dtype, scale)
    y, w = weights_of(values, weights, qc, table)
    cnt = (w > 0).sum(axis=0).astype(np.uint16)
    out = encode(smooth_values(y, w, lam, order, envelope), cnt, min_valid, name, scale)
    return (out, cnt) if count else out
