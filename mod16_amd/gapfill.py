'''
QC-driven temporal gap filling of 8-day fPAR / LAI series: the definition, in numpy, of what
``mod16_gapfill_u8`` computes (``RasterEngine.gapfill``, ``mod16_amd.gapfill_series``), and the
argument checks of those calls. Host only: nothing here touches the library or a device; the kernel
(``csrc/mod16_gapfill.hpp``) follows ``fill_series`` and ``encode`` case for case.

A series is ``(S, n)`` uint8 codes as MOD15A2H distributes them (fPAR in percent, LAI x 10; codes
>= 249 are fill values), optionally with the product's ``FparLai_QC`` layer. Slab ``t`` of a pixel is
*reliable* for a field where the field's code is < 249 and, with a QC layer, ``good[qc]`` holds.
With ``i`` the last reliable slab <= t (code ``a``) and ``j`` the first reliable slab >= t (code
``b``), every slab gets an exact rational ``num / den`` and a source byte:

====  ============  ===================================================  =================================
 0    observed      t reliable                                           code / 1
 1    interpolated  i and j exist, ``j - i - 1 <= max_gap`` (or None)    (a (j - t) + b (t - i)) / (j - i)
 2    held          only one side exists, at most ``max_gap`` away       that code / 1
 3    fallback      none of these, ``fallback`` given with a code < 249  fallback code / 1
 4    unfilled      otherwise                                            none
====  ============  ===================================================  =================================

``MOD15_GOOD`` is the package's default QC table, chosen from the bit table of the MOD15A2H user
guide: bit 0 = 0 (MODLAND: good quality), bit 2 = 0 (no dead detector), bits 3-4 = 0 or 3 (cloud
state clear, or assumed clear), bits 5-7 = 0 or 1 (main algorithm, with or without saturation) --
the eight codes 0, 2, 24, 26, 32, 34, 56, 58. It is this package's choice, not a transcription of
the operational MOD16 code; pass another ``good`` table for another policy (or another product).
'''
import numpy as np

FILL = 249                  # codes from here on are fill values
MAX_SLABS = 4096
MAX_FIELDS = 3
OBSERVED, INTERPOLATED, HELD, FALLBACK, UNFILLED = range(5)
OUT_TYPES = {'uint8': 0, 'float32': 1, 'float64': 2}       # enum mod16_gapfill_out


def default_good():
    '''The 256-entry boolean table of acceptable ``FparLai_QC`` bytes (see the module text).'''
    q = np.arange(256)
    cloud = (q >> 3) & 3
    return ((q & 1) == 0) & ((q & 4) == 0) & ((cloud == 0) | (cloud == 3)) & ((q >> 5) <= 1)


#: the codes of ``default_good()``
MOD15_GOOD = tuple(int(q) for q in np.flatnonzero(default_good()))


def _as_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (what, value))
    return int(value)


def check_good(good):
    '''``good`` -> a (256,) boolean table (None: the default); ValueError unless it has 256 entries.'''
    if good is None:
        return default_good()
    good = np.asarray(good)
    if good.shape != (256,):
        raise ValueError('good must have 256 entries (one per QC byte), got shape %r' % (good.shape,))
    return good.astype(bool)


def check_series(shapes, qc_shape=None, good=None, max_gap=None, fallback_shapes=None, dtype='uint8',
                 scale=None):
    '''The argument checks of every gap-filling call, on shapes only (no array is read).

    ``shapes``: the shapes of the one to three fields, each ``(S,) + pixel shape`` with ``1 <= S <=
    4096``; ``qc_shape``: None or the same shape; ``fallback_shapes``: None or one pixel shape (or
    None) per field; ``max_gap``: None or an int >= 0; ``dtype``: 'uint8', 'float32' or 'float64';
    ``scale``: None, one number (one field) or one per field, float output only.

    Returns ``(S, pixel shape, good table, max_gap as the library takes it (-1: none), dtype name,
    scales)``; ValueError otherwise.'''
    shapes = [tuple(s) for s in shapes]
    if not 1 <= len(shapes) <= MAX_FIELDS:
        raise ValueError('between 1 and %d fields, got %d' % (MAX_FIELDS, len(shapes)))
    first = shapes[0]
    if len(first) < 1:
        raise ValueError('a field must have a leading time axis')
    S = first[0]
    if S < 1 or S > MAX_SLABS:
        raise ValueError('the time axis must have between 1 and %d slabs, got %d' % (MAX_SLABS, S))
    for s in shapes[1:]:
        if s != first:
            raise ValueError('the fields must share one shape, got %r and %r' % (first, s))
    if qc_shape is not None and tuple(qc_shape) != first:
        raise ValueError('qc must have the shape of the fields %r, got %r' % (first, tuple(qc_shape)))
    if fallback_shapes is not None:
        fallback_shapes = list(fallback_shapes)
        if len(fallback_shapes) != len(shapes):
            raise ValueError('fallback must hold one array per field (%d), got %d' % (len(shapes), len(fallback_shapes)))
        for s in fallback_shapes:
            if s is not None and tuple(s) != first[1:]:
                raise ValueError('a fallback must have the pixel shape %r, got %r' % (first[1:], tuple(s)))
    table = check_good(good)
    if max_gap is None:
        mg = -1
    else:
        mg = _as_int(max_gap, 'max_gap')
        if mg < 0:
            raise ValueError('max_gap must be None or at least 0, got %d' % mg)
        mg = min(mg, MAX_SLABS + 1)
    try:
        name = np.dtype(dtype).name
    except TypeError:
        name = None
    if name not in OUT_TYPES:
        raise ValueError("dtype must be 'uint8', 'float32' or 'float64', got %r" % (dtype,))
    if name == 'uint8':
        if scale is not None:
            raise ValueError('scale applies to float output only (uint8 output keeps the codes)')
        scales = [1.0] * len(shapes)
    else:
        if scale is None:
            scales = [1.0] * len(shapes)
        elif np.ndim(scale) == 0:
            scales = [float(scale)] * len(shapes)
        else:
            scales = [float(v) for v in scale]
        if len(scales) != len(shapes) or not all(np.isfinite(scales)):
            raise ValueError('scale must be one finite number per field, got %r' % (scale,))
    return S, first[1:], table, mg, name, scales


def reliable(values, qc=None, good=None):
    '''Where a field's slabs are reliable: the code is < 249 and, with ``qc``, ``good[qc]`` holds.'''
    values = np.asarray(values)
    rel = values < FILL
    if qc is not None:
        rel = rel & check_good(good)[np.asarray(qc, np.uint8)]
    return rel


def fill_series(values, reliable, max_gap=None, fallback=None):
    '''One field's filled series as exact rationals.

    ``values``: ``(S,) + shape`` codes; ``reliable``: booleans of that shape; ``fallback``: None or
    ``shape`` codes. Returns ``(num, den, source)``: int64, int64 and uint8 of ``values``' shape;
    ``num`` is 0 and ``den`` 1 where ``source`` is 4 (unfilled).'''
    values = np.asarray(values)
    rel = np.asarray(reliable, bool)
    if values.ndim < 1 or rel.shape != values.shape:
        raise ValueError('values and reliable must share a shape with a leading time axis')
    S = values.shape[0]
    v = values.astype(np.int64)
    t = np.arange(S, dtype=np.int64).reshape((S,) + (1,) * (values.ndim - 1))
    none_i, none_j = -1, S
    i = np.maximum.accumulate(np.where(rel, t, none_i), axis=0)
    j = np.minimum.accumulate(np.where(rel, t, none_j)[::-1], axis=0)[::-1]
    left, right = i > none_i, j < none_j
    a = np.take_along_axis(v, np.clip(i, 0, S - 1), axis=0)
    b = np.take_along_axis(v, np.clip(j, 0, S - 1), axis=0)
    limit = S + 1 if max_gap is None else int(max_gap)
    interp = left & right & ~rel & (j - i - 1 <= limit)
    held_l = left & ~right & (t - i <= limit)
    held_r = right & ~left & (j - t <= limit)
    num = np.zeros(values.shape, np.int64)
    den = np.ones(values.shape, np.int64)
    source = np.full(values.shape, UNFILLED, np.uint8)
    if fallback is not None:
        fb = np.broadcast_to(np.asarray(fallback).astype(np.int64), values.shape)
        ok = fb < FILL
        num = np.where(ok, fb, num)
        source = np.where(ok, np.uint8(FALLBACK), source)
    num = np.where(held_l, a, np.where(held_r, b, num))
    source = np.where(held_l | held_r, np.uint8(HELD), source)
    num = np.where(interp, a * (j - t) + b * (t - i), num)
    den = np.where(interp, j - i, den)
    source = np.where(interp, np.uint8(INTERPOLATED), source)
    num = np.where(rel, v, num)
    den = np.where(rel, 1, den)
    source = np.where(rel, np.uint8(OBSERVED), source).astype(np.uint8)
    return num, den, source


def encode(num, den, source, dtype='uint8', scale=1.0):
    '''The rationals of ``fill_series`` in an output type, each value rounded once: uint8 is ``(2 num
    + den) // (2 den)`` (round half up, in integers; 255 where unfilled); float32 / float64 is
    ``T((float64(num) / float64(den)) * scale)`` (NaN where unfilled).'''
    num = np.asarray(num, np.int64)
    den = np.asarray(den, np.int64)
    missing = np.asarray(source) == UNFILLED
    name = np.dtype(dtype).name
    if name == 'uint8':
        return np.where(missing, 255, (2 * num + den) // (2 * den)).astype(np.uint8)
    if name not in OUT_TYPES:
        raise ValueError("dtype must be 'uint8', 'float32' or 'float64', got %r" % (dtype,))
    value = (num.astype(np.float64) / den.astype(np.float64)) * np.float64(scale)
    return np.where(missing, np.nan, value).astype(dtype)
