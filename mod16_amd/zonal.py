'''
Zonal statistics -- exact area-weighted totals per zone and layer: the definition, in numpy, of what
``mod16_zonal_*`` computes (``RasterEngine.zonal``, ``mod16_amd.zonal_statistics``), and the result
type of those calls. Host only: nothing here touches the library or a device; the kernel
(``csrc/mod16_zonal.hpp``) follows ``accumulate`` step for step.

The sums are order-independent by construction. Every term is quantised ONCE to a 62-bit fixed
point whose scale is fixed per call by two bounds, ``wmax`` (weights) and ``xmax`` (values), and
accumulated with 64-bit integer adds: integer addition is associative, so one launch, a call staged
in 300 tiles, several calls that accumulate tile after tile and the ``merge`` of several devices'
partial results all give the same words.

``exponent(b)`` is the smallest integer ``e`` with ``b <= 2**e``; a call carries ``ew =
exponent(wmax)`` and ``ex = exponent(xmax)``, and its three sums have ``F0 = 62 - ew``, ``F1 = 62 -
ew - ex`` and ``F2 = 62 - ew - 2 ex`` fractional bits (``F0 + F2 == 2 F1``).

Per pixel and layer, all arithmetic in float64 (float32 inputs are widened first), in this order:

1. a zone id outside ``[0, Z)``: the pixel is ignored;
2. ``x`` NaN or ``w`` NaN: the pixel is ignored (masked);
3. ``not (abs(x) <= xmax)`` or ``not (0 <= w <= wmax)``: ``rejected += 1`` and nothing else
   (infinities land here);
4. otherwise ``count += 1``; the terms ``a = w``, ``b = w * x``, ``c = b * x`` (one rounded multiply
   each); ``q = int64(rint(ldexp(t, F)))`` (``|q| <= 2**62``), split into ``qh = q >> 32``
   (arithmetic) and ``ql = q & 0xffffffff``; ``hi += qh`` and ``lo += ql``; ``min_key`` and
   ``max_key`` take ``key(x)``, the order-preserving int64 image of the double (``-0.0 < +0.0``).

The accumulator is ``(K, Z, 10)`` int64 -- ``WORDS``: count, rejected, w_hi, w_lo, wx_hi, wx_lo,
wxx_hi, wxx_lo, min_key, max_key. A call ADDS into the accumulator it is given.

Limit: the accumulator is valid while a zone and layer has fewer than 2**31 valid pixels over
everything accumulated into it, so that every ``lo`` word stays below 2**63.
'''
import math
from fractions import Fraction

import numpy as np

WORDS = ('count', 'rejected', 'w_hi', 'w_lo', 'wx_hi', 'wx_lo', 'wxx_hi', 'wxx_lo', 'min_key', 'max_key')
NWORDS = len(WORDS)
COUNT, REJECTED, W_HI, W_LO, WX_HI, WX_LO, WXX_HI, WXX_LO, MIN_KEY, MAX_KEY = range(NWORDS)
INT64_MAX = np.iinfo(np.int64).max
INT64_MIN = np.iinfo(np.int64).min
ZONE_U8, ZONE_U16, ZONE_I32 = 0, 1, 2              # enum mod16_zone_type
ZONE_TYPES = {'uint8': ZONE_U8, 'uint16': ZONE_U16, 'int32': ZONE_I32}
WEIGHT_NONE, WEIGHT_ROW, WEIGHT_PIXEL = 0, 1, 2    # enum mod16_zonal_weight
MAX_PIXELS = 1 << 30
MAX_LAYERS = 65535
MAX_ZONES = 1 << 24
F_LIMIT = 900                                      # every F of a call lies in [-900, 900]
_LOW63 = np.int64(INT64_MAX)


def exponent(b):
    '''The smallest integer ``e`` with ``b <= 2**e`` (``b`` > 0 and finite).'''
    b = float(b)
    if not (b > 0.0) or math.isinf(b):
        raise ValueError('a bound must be positive and finite, got %r' % (b,))
    m, e = math.frexp(b)
    return e - 1 if m == 0.5 else e


def fractional_bits(ew, ex):
    '''``(F0, F1, F2)`` of a call with the exponents ``ew`` and ``ex``.'''
    return 62 - ew, 62 - ew - ex, 62 - ew - 2 * ex


def check_bounds(bounds):
    '''``(wmax, xmax)`` -> ``(wmax, xmax, ew, ex)``; ValueError unless both are positive and finite
    and every F stays inside [-900, 900].'''
    try:
        wmax, xmax = (float(v) for v in bounds)
    except (TypeError, ValueError):
        raise ValueError('bounds must be a pair (wmax, xmax), got %r' % (bounds,))
    ew, ex = exponent(wmax), exponent(xmax)
    if any(abs(f) > F_LIMIT for f in fractional_bits(ew, ex)):
        raise ValueError('bounds %r are out of range: a fixed-point scale leaves 2**-900 ... 2**900' % ((wmax, xmax),))
    return wmax, xmax, ew, ex


def check_nzones(nzones):
    '''-> ``nzones`` as an int; ValueError unless it is an integer (no bool) in ``[1, MAX_ZONES]``.'''
    if isinstance(nzones, (bool, np.bool_)) or not isinstance(nzones, (int, np.integer)) or not 1 <= nzones <= MAX_ZONES:
        raise ValueError('nzones must be an integer between 1 and 2**24, got %r' % (nzones,))
    return int(nzones)


def check_acc_bounds(bounds):
    '''A call that adds into ``acc=`` cannot find its own bounds: ValueError where ``bounds`` is None.'''
    if bounds is None:
        raise ValueError('acc= needs explicit bounds: their exponents are the scale of the accumulator')


def key(x):
    '''The order-preserving int64 image of float64 values: the bits, with the low 63 bits flipped
    where the sign bit is set (so ``key(-0.0) < key(+0.0)``).'''
    bits = np.asarray(x, np.float64).view(np.int64)
    return bits ^ ((bits >> 63) & _LOW63)


def unkey(k):
    '''The inverse of ``key``.'''
    k = np.asarray(k, np.int64)
    return (k ^ ((k >> 63) & _LOW63)).view(np.float64)


def empty(layers, nzones):
    '''A fresh ``(layers, nzones, 10)`` accumulator: the min word INT64_MAX, the max word INT64_MIN,
    the rest 0.'''
    acc = np.zeros((int(layers), int(nzones), NWORDS), np.int64)
    acc[..., MIN_KEY] = INT64_MAX
    acc[..., MAX_KEY] = INT64_MIN
    return acc


def merge(a, b):
    '''The accumulator of everything accumulated into ``a`` or ``b``: the first eight words added,
    min and max of the last two.'''
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape != b.shape or a.shape[-1:] != (NWORDS,):
        raise ValueError('accumulators must share a shape (..., 10), got %r and %r' % (a.shape, b.shape))
    out = a + b
    out[..., MIN_KEY] = np.minimum(a[..., MIN_KEY], b[..., MIN_KEY])
    out[..., MAX_KEY] = np.maximum(a[..., MAX_KEY], b[..., MAX_KEY])
    return out


def pixel_weights(n, dtype, weights=None, cols=None, first_pixel=0):
    '''The float64 weight of each of ``n`` pixels: 1 (``weights`` None), ``weights[(first_pixel + p)
    // cols]`` (with ``cols``: one float64 weight per raster row), or ``weights[p]`` widened.'''
    if weights is None:
        return np.ones(n, np.float64)
    if cols is not None:
        rows = (int(first_pixel) + np.arange(n, dtype=np.int64)) // int(cols)
        return np.asarray(weights, np.float64)[rows]
    w = np.asarray(weights)
    if w.shape != (n,):
        raise ValueError('per-pixel weights must have shape (%d,), got %r' % (n, w.shape))
    return w.astype(dtype).astype(np.float64)


def quantise(t, F):
    '''``int64(rint(ldexp(t, F)))`` and its split ``(q >> 32, q & 0xffffffff)``.'''
    q = np.rint(np.ldexp(np.asarray(t, np.float64), F)).astype(np.int64)
    return q, q >> 32, q & np.int64(0xffffffff)


def classify(x, w, zones, nzones, wmax, xmax):
    '''``(valid, rejected)`` masks of one layer's pixels (steps 1 to 3 of the module text).'''
    z = np.asarray(zones).astype(np.int64)
    inside = (z >= 0) & (z < nzones)
    with np.errstate(invalid='ignore'):
        live = inside & ~(np.isnan(x) | np.isnan(w))
        ok = (np.abs(x) <= xmax) & (w >= 0.0) & (w <= wmax)
    return live & ok, live & ~ok


def accumulate(values, zones, nzones, weights=None, cols=None, first_pixel=0, bounds=(1.0, 1.0), acc=None):
    '''The numpy statement of a zonal call. ``values``: ``(K, n)`` float32 or float64; ``zones``:
    ``(n,)`` integers; ``weights``: None, a float64 vector per raster row (with ``cols``; pixel ``p``
    takes ``weights[(first_pixel + p) // cols]``) or ``(n,)`` of the values' dtype; ``bounds``:
    ``(wmax, xmax)``. Adds into ``acc`` (a copy of it; default ``empty(K, nzones)``) and returns it.'''
    values = np.asarray(values)
    if values.ndim != 2 or values.dtype not in (np.float32, np.float64):
        raise ValueError('values must be (K, n) float32 or float64')
    K, n = values.shape
    zones = np.asarray(zones)
    if zones.shape != (n,) or zones.dtype.kind not in 'iu':
        raise ValueError('zones must be (%d,) integers' % n)
    Z = int(nzones)
    wmax, xmax, ew, ex = check_bounds(bounds)
    F = fractional_bits(ew, ex)
    acc = empty(K, Z) if acc is None else np.array(acc, np.int64)
    if acc.shape != (K, Z, NWORDS):
        raise ValueError('acc must have shape %r, got %r' % ((K, Z, NWORDS), acc.shape))
    w = pixel_weights(n, values.dtype, weights, cols, first_pixel)
    z = zones.astype(np.int64)
    for k in range(K):
        x = values[k].astype(np.float64)
        valid, rejected = classify(x, w, z, Z, wmax, xmax)
        np.add.at(acc[k, :, REJECTED], z[rejected], 1)
        zv, xv, a = z[valid], x[valid], w[valid]
        np.add.at(acc[k, :, COUNT], zv, 1)
        b = a * xv
        c = b * xv
        for j, t in enumerate((a, b, c)):
            _, qh, ql = quantise(t, F[j])
            np.add.at(acc[k, :, W_HI + 2 * j], zv, qh)
            np.add.at(acc[k, :, W_LO + 2 * j], zv, ql)
        kx = key(xv)
        np.minimum.at(acc[k, :, MIN_KEY], zv, kx)
        np.maximum.at(acc[k, :, MAX_KEY], zv, kx)
    return acc


def to_float(hi, lo, F):
    '''A hi / lo pair as float64: the carry normalised (``hi += lo >> 32``, ``lo &= 0xffffffff``),
    then ``ldexp(float64(hi) * 4294967296.0 + float64(lo), -F)``.'''
    hi = np.asarray(hi, np.int64) + (np.asarray(lo, np.int64) >> 32)
    lo = np.asarray(lo, np.int64) & np.int64(0xffffffff)
    return np.ldexp(hi.astype(np.float64) * 4294967296.0 + lo.astype(np.float64), -int(F))


def to_int(hi, lo):
    '''A hi / lo pair as an exact Python integer, ``(hi << 32) + lo``.'''
    return (int(hi) << 32) + int(lo)


class ZonalResult(object):
    '''The accumulator of a zonal call and the exponents of its bounds: ``words`` ``(K, Z, 10)``
    int64, ``ew``, ``ex``. Every statistic is derived from the words on the host, ``(K, Z)`` each
    (``(Z,)`` when the values had no layer axis and ``squeeze`` is set).'''

    def __init__(self, words, ew, ex, squeeze=False):
        words = np.asarray(words, np.int64)
        if words.ndim != 3 or words.shape[2] != NWORDS:
            raise ValueError('words must have shape (K, Z, 10), got %r' % (words.shape,))
        self.words = words
        self.ew, self.ex = int(ew), int(ex)
        self.squeeze = bool(squeeze)

    @classmethod
    def from_tensor(cls, acc, ew=None, ex=None):
        '''Downloads the accumulator tensor ``RasterEngine.zonal`` returned (waits for it); ``ew``
        and ``ex`` default to the exponents that call recorded on the tensor.'''
        if ew is None or ex is None:
            ew, ex = acc.exponents
        return cls(acc.detach().cpu().numpy(), ew, ex)

    def _out(self, a):
        return a[0] if self.squeeze else a

    @property
    def count(self):
        return self._out(self.words[..., COUNT].copy())

    @property
    def rejected(self):
        return self._out(self.words[..., REJECTED].copy())

    def _sum(self, j):
        F = fractional_bits(self.ew, self.ex)[j]
        return self._out(to_float(self.words[..., W_HI + 2 * j], self.words[..., W_LO + 2 * j], F))

    @property
    def sum_w(self):
        return self._sum(0)

    @property
    def sum_wx(self):
        return self._sum(1)

    @property
    def sum_wxx(self):
        return self._sum(2)

    @property
    def mean(self):
        sw, swx = self.sum_w, self.sum_wx
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(sw == 0, np.nan, swx / np.where(sw == 0, 1.0, sw))

    @property
    def var(self):
        '''The weighted population variance, exactly from Python integers: ``(Q2 Q0 - Q1 Q1) / Q0**2
        * 4**ex`` rounded once (the scales cancel: ``F0 + F2 == 2 F1``); NaN where ``sum_w == 0``.'''
        flat = self.words.reshape(-1, NWORDS)
        out = np.full(len(flat), np.nan)
        scale = Fraction(4) ** self.ex
        for i, wd in enumerate(flat):
            q0 = to_int(wd[W_HI], wd[W_LO])
            if q0 == 0:
                continue
            q1 = to_int(wd[WX_HI], wd[WX_LO])
            q2 = to_int(wd[WXX_HI], wd[WXX_LO])
            out[i] = float(Fraction(q2 * q0 - q1 * q1, q0 * q0) * scale)
        return self._out(out.reshape(self.words.shape[:2]))

    @property
    def std(self):
        return np.sqrt(np.maximum(self.var, 0.0))

    def _extreme(self, word):
        return self._out(np.where(self.words[..., COUNT] == 0, np.nan, unkey(self.words[..., word])))

    @property
    def min(self):
        return self._extreme(MIN_KEY)

    @property
    def max(self):
        return self._extreme(MAX_KEY)

    def merge(self, other):
        '''The result of everything accumulated into either; ValueError when the exponents differ.'''
        if (self.ew, self.ex) != (other.ew, other.ex):
            raise ValueError('results with the exponents %r and %r cannot be merged'
                             % ((self.ew, self.ex), (other.ew, other.ex)))
        return ZonalResult(merge(self.words, other.words), self.ew, self.ex, self.squeeze)
