'''
Zonal histograms and exact zonal quantiles per zone and layer: the definition, in numpy and Python
integers, of what ``mod16_zonal_hist_*`` and ``mod16_zonal_select`` compute
(``RasterEngine.zonal_histogram``, ``.zonal_selection``, ``.zonal_quantiles``,
``mod16_amd.zonal_histogram``, ``mod16_amd.zonal_quantiles``), and the result types of those calls.
Host only: nothing here touches the library or a device; the kernels (``csrc/mod16_zonalq.hpp``)
follow ``histogram``, ``digits`` and ``select`` step for step.

Every table is made of int64 words that integer adds fill, as in ``mod16_amd.zonal``: the words do
not depend on the order in which the pixels arrive, so one call, a call staged in tiles, calls that
accumulate part after part and the sum of several devices' tables are the same words. A quantile is
found by radix selection over histograms of the order-preserving key of the value, most significant
digit first: an exact order statistic, a value of the raster, never an interpolation.

Per pixel and layer:

1. a zone id outside ``[0, Z)``: the pixel is skipped;
2. ``x`` NaN or ``w`` NaN: skipped (masked);
3. ``not (0 <= w <= wmax)``: skipped. Infinite ``x`` takes part: it orders like any key, and in a
   uniform histogram it lands in the under or over bin;
4. the weight word is 1 without weights, else ``qw = int64(rint(ldexp(w, 31 - ew)))`` with ``ew =
   exponent(wmax)``, so ``qw <= 2**31``. A weight below ``2**(ew - 32)`` quantises to 0: such a pixel
   counts for nothing (a weight of exactly ``2**(ew - 32)`` rounds to even, 0, as well);
5. the key is the order-preserving unsigned image of the value in its own width ``Wd`` (32 for
   float32, 64 for float64): the bits, all flipped where the sign is set, else the sign bit set
   (``-0.0 < +0.0``).

Limit, as in ``zonal``: a word is valid while a zone and layer holds fewer than 2**31 valid pixels
over everything added into it.

Uniform histogram, ``(K, Z, bins + 2)``: word 0 is the under bin, word ``bins + 1`` the over bin. With
``x`` widened to float64 and ``scale = bins / (hi - lo)`` formed once: ``x < lo`` goes under, ``not (x <
hi)`` over, else the bin is ``1 + int(floor((x - lo) * scale))`` -- the subtraction and the multiply
rounded once each, no fused multiply-add -- clamped to ``bins`` against rounding at the top edge.

Digit histogram of level ``l``, ``(K, Z, S, B)`` with ``B = 2**bits``: level 0 counts the top ``bits``
bits of every valid pixel's key into slot 0 only; at a level ``l >= 1`` a pixel is counted into every
slot ``s`` for which the top ``l * bits`` bits of its key equal ``prefix[k, z, s]``, under its digit, the
next ``min(bits, Wd - l * bits)`` bits. There are ``levels = ceil(Wd / bits)`` levels.

Target of a quantile ``q``, the exact rational of its double: ``m, e = frexp(q)``, ``M = int(m * 2**53)``,
``E = 53 - e``; with ``W`` the total weight word of the zone and layer, ``target = max(1, ceil(M * W /
2**E))`` in Python integers. The quantile is the smallest value ``v`` of the zone whose cumulative
weight word over ``x <= v`` reaches the target: the weighted inverted-CDF quantile. ``W == 0`` gives NaN.
'''
import math

import numpy as np

from . import zonal as _z

MIN_BITS, MAX_BITS = 4, 12
MAX_BINS = 4094
MAX_SLOTS = 16
MODE_UNIFORM, MODE_DIGIT = 0, 1                    # enum mod16_zonal_hist_mode
DEFAULT_BITS = 8
DEFAULT_Q = (0.05, 0.5, 0.95)


def width(dtype):
    '''``Wd``: 32 for float32, 64 for float64; ValueError for anything else.'''
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return 32
    if dtype == np.float64:
        return 64
    raise ValueError('values must be float32 or float64, got %s' % dtype)


def check_bits(bits):
    '''-> ``bits`` as an int; ValueError unless it is an integer in ``[4, 12]``.'''
    if isinstance(bits, (bool, np.bool_)) or not isinstance(bits, (int, np.integer)) or not MIN_BITS <= bits <= MAX_BITS:
        raise ValueError('bits must be an integer between %d and %d, got %r' % (MIN_BITS, MAX_BITS, bits))
    return int(bits)


def check_bins(bins):
    '''-> ``bins`` as an int; ValueError unless it is an integer in ``[1, 4094]``.'''
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= MAX_BINS:
        raise ValueError('bins must be an integer between 1 and %d, got %r' % (MAX_BINS, bins))
    return int(bins)


def check_range(bins, lo, hi):
    '''-> ``(lo, hi, scale)`` as floats, ``scale = bins / (hi - lo)``; ValueError unless ``lo < hi``,
    both finite, and the scale is finite and positive.'''
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError('the range must be a pair of numbers, got %r' % ((lo, hi),))
    if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
        raise ValueError('the range must be finite with lo < hi, got %r' % ((lo, hi),))
    span = hi - lo
    scale = bins / span if span > 0.0 and math.isfinite(span) else math.inf
    if not math.isfinite(scale) or not scale > 0.0:
        raise ValueError('the range %r gives no finite bin scale' % ((lo, hi),))
    return lo, hi, scale


def check_wmax(wmax):
    '''-> ``(wmax, ew)``; ValueError unless ``wmax`` is positive and finite and ``31 - ew`` stays inside
    [-900, 900].'''
    wmax = float(wmax)
    ew = _z.exponent(wmax)
    if abs(31 - ew) > _z.F_LIMIT:
        raise ValueError('wmax %r is out of range: the weight scale leaves 2**-900 ... 2**900' % (wmax,))
    return wmax, ew


def check_acc_wmax(wmax):
    '''A call that adds into ``acc=`` cannot find its own bound: ValueError where ``wmax`` is None.'''
    if wmax is None:
        raise ValueError('acc= needs an explicit wmax: its exponent is the scale of the table')


def levels(wd, bits):
    '''``ceil(Wd / bits)``.'''
    return -(-int(wd) // int(bits))


def check_level(level, wd, bits):
    if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, np.integer)) or not 0 <= level < levels(wd, bits):
        raise ValueError('level must be an integer between 0 and %d, got %r' % (levels(wd, bits) - 1, level))
    return int(level)


def ukey(x):
    '''The order-preserving unsigned image of float values in their own width, as uint64: for
    float64 ``zonal.key`` with the sign bit flipped, for float32 the same rule on 32 bits.'''
    x = np.asarray(x)
    if width(x.dtype) == 64:
        return _z.key(x).view(np.uint64) ^ np.uint64(1 << 63)
    b = x.view(np.uint32)
    return (b ^ np.where(b >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))).astype(np.uint64)


def unukey(k, dtype):
    '''The inverse of ``ukey``: values of ``dtype`` from their unsigned keys.'''
    k = np.asarray(k, np.uint64)
    if width(dtype) == 64:
        return _z.unkey((k ^ np.uint64(1 << 63)).view(np.int64))
    b = k.astype(np.uint32)
    return (b ^ np.where(b >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xffffffff))).view(np.float32)


def weight_words(w, wmax, ew, weighted):
    '''``(valid, qw)`` of float64 weights: step 3 and 4 of the module text.'''
    with np.errstate(invalid='ignore'):
        ok = (w >= 0.0) & (w <= wmax)
    if not weighted:
        return ok, np.ones(len(w), np.int64)
    qw = np.zeros(len(w), np.int64)
    qw[ok] = np.rint(np.ldexp(w[ok], 31 - ew)).astype(np.int64)
    return ok, qw


def _inputs(values, zones, nzones, weights, cols, first_pixel, wmax):
    values = np.asarray(values)
    if values.ndim != 2:
        raise ValueError('values must be (K, n) float32 or float64')
    wd = width(values.dtype)
    K, n = values.shape
    zones = np.asarray(zones)
    if zones.shape != (n,) or zones.dtype.kind not in 'iu':
        raise ValueError('zones must be (%d,) integers' % n)
    Z = _z.check_nzones(nzones)
    if weights is None:
        wmax, ew = 1.0, 31                # (a word is a count: word * 2**(ew - 31))
    else:
        if wmax is None:
            raise ValueError('weights need wmax')
        wmax, ew = check_wmax(wmax)
    w = _z.pixel_weights(n, values.dtype, weights, cols, first_pixel)
    z = zones.astype(np.int64)
    inside = (z >= 0) & (z < Z)
    ok, qw = weight_words(w, wmax, ew, weights is not None)
    live = inside & ok & ~np.isnan(w)
    return values, wd, K, n, Z, z, live, qw, ew


def histogram(values, zones, nzones, bins, lo, hi, weights=None, cols=None, first_pixel=0, wmax=None, acc=None):
    '''The uniform histogram of the module text. ``values``: ``(K, n)`` float32 or float64; ``zones``:
    ``(n,)`` integers; ``weights``, ``cols``, ``first_pixel``: as in ``zonal.accumulate``, with ``wmax``
    their bound. Adds into ``acc`` (a copy of it; default zeros) and returns the ``(K, Z, bins + 2)``
    int64 table.'''
    bins = check_bins(bins)
    lo, hi, scale = check_range(bins, lo, hi)
    values, wd, K, n, Z, z, live, qw, ew = _inputs(values, zones, nzones, weights, cols, first_pixel, wmax)
    acc = np.zeros((K, Z, bins + 2), np.int64) if acc is None else np.array(acc, np.int64)
    if acc.shape != (K, Z, bins + 2):
        raise ValueError('acc must have shape %r, got %r' % ((K, Z, bins + 2), acc.shape))
    for k in range(K):
        x = values[k].astype(np.float64)
        m = live & ~np.isnan(x)
        xv = x[m]
        with np.errstate(invalid='ignore', over='ignore'):
            under, over = xv < lo, ~(xv < hi)
            mid = ~(under | over)
            b = np.zeros(len(xv), np.int64)
            b[over] = bins + 1
            t = (xv[mid] - lo) * scale
            b[mid] = np.minimum(1 + np.floor(t).astype(np.int64), bins)
        np.add.at(acc[k], (z[m], b), qw[m])
    return acc


def digits(values, zones, nzones, level, bits, prefix=None, weights=None, cols=None, first_pixel=0, wmax=None,
           slots=None, acc=None):
    '''The digit histogram of level ``level`` of the module text. ``prefix``: ``(K, Z, S)`` uint64, the
    top ``level * bits`` bits of the keys that count (not looked at on level 0, where ``slots`` may give
    S instead; default 1). Adds into ``acc`` (a copy; default zeros) and returns the ``(K, Z, S, 2**bits)``
    int64 table.'''
    bits = check_bits(bits)
    values, wd, K, n, Z, z, live, qw, ew = _inputs(values, zones, nzones, weights, cols, first_pixel, wmax)
    level = check_level(level, wd, bits)
    if prefix is not None:
        prefix = np.asarray(prefix)
        if prefix.ndim != 3 or prefix.shape[:2] != (K, Z) or prefix.dtype != np.uint64:
            raise ValueError('prefix must be (%d, %d, S) uint64' % (K, Z))
        S = prefix.shape[2]
    elif level == 0:
        S = 1 if slots is None else int(slots)
    else:
        raise ValueError('level %d needs the prefixes of the level before' % level)
    if not 1 <= S <= MAX_SLOTS:
        raise ValueError('between 1 and %d slots, got %d' % (MAX_SLOTS, S))
    B = 1 << bits
    acc = np.zeros((K, Z, S, B), np.int64) if acc is None else np.array(acc, np.int64)
    if acc.shape != (K, Z, S, B):
        raise ValueError('acc must have shape %r, got %r' % ((K, Z, S, B), acc.shape))
    used = level * bits
    d = min(bits, wd - used)
    low = np.uint64(wd - used - d)
    for k in range(K):
        m = live & ~np.isnan(values[k])
        key, zv, qv = ukey(values[k][m]), z[m], qw[m]
        digit = ((key >> low) & np.uint64((1 << d) - 1)).astype(np.int64)
        if level == 0:
            np.add.at(acc[k, :, 0], (zv, digit), qv)
            continue
        top = key >> np.uint64(wd - used)
        for s in range(S):
            hit = top == prefix[k, zv, s]
            np.add.at(acc[k, :, s], (zv[hit], digit[hit]), qv[hit])
    return acc


def check_q(q):
    '''-> the quantiles as a tuple of floats; ValueError unless each lies in ``[0, 1]`` (NaN does
    not) and there are between 1 and 16 of them.'''
    try:
        qs = tuple(float(v) for v in np.atleast_1d(np.asarray(q, np.float64)))
    except (TypeError, ValueError):
        raise ValueError('q must be a number or a sequence of numbers, got %r' % (q,))
    if not 1 <= len(qs) <= MAX_SLOTS:
        raise ValueError('between 1 and %d quantiles, got %d' % (MAX_SLOTS, len(qs)))
    for v in qs:
        if not 0.0 <= v <= 1.0:
            raise ValueError('a quantile must lie in [0, 1], got %r' % (v,))
    return qs


def rational(q):
    '''``(M, E)`` with ``q == M / 2**E`` exactly: ``m, e = frexp(q)``, ``M = int(m * 2**53)``, ``E = 53 - e``.'''
    m, e = math.frexp(q)
    return int(m * 2 ** 53), 53 - e


def target(q, W):
    '''``max(1, ceil(M * W / 2**E))`` in Python integers; 0 marks ``W == 0`` (no quantile).'''
    W = int(W)
    if W == 0:
        return 0
    M, E = rational(q)
    return max(1, -((-M * W) >> E))


def targets(q, total):
    '''``(K, Z, S)`` int64 targets of the quantiles ``q`` for the ``(K, Z)`` totals of level 0.'''
    qs = check_q(q)
    total = np.asarray(total, np.int64)
    out = np.zeros(total.shape + (len(qs),), np.int64)
    for idx in np.ndindex(total.shape):
        for s, v in enumerate(qs):
            out[idx + (s,)] = target(v, total[idx])
    return out


def select(hist, remaining, prefix, level, bits, wd=32):
    '''Closes a level: per ``(k, z, s)`` the first bin of ``hist[k, z, s]`` (level 0: of ``hist[k, z, 0]``)
    whose running sum reaches ``remaining[k, z, s]``; ``remaining`` drops by the sum before that bin and
    the bin is appended to the prefix. ``remaining == 0`` (an empty zone) stays as it is. Returns the new
    ``(remaining, prefix)``; after the last level the prefix is the key of the answer.'''
    bits = check_bits(bits)
    level = check_level(level, wd, bits)
    hist = np.asarray(hist, np.int64)
    remaining = np.array(remaining, np.int64)
    prefix = np.array(prefix, np.uint64)
    if hist.ndim != 4 or hist.shape[3] != 1 << bits or remaining.shape != hist.shape[:3] or prefix.shape != hist.shape[:3]:
        raise ValueError('hist must be (K, Z, S, %d) and remaining and prefix (K, Z, S)' % (1 << bits))
    d = min(bits, wd - level * bits)
    rows = hist[:, :, :1] if level == 0 else hist
    run = np.cumsum(rows[..., :1 << d], axis=-1)                       # (int64: a row sums to less than 2**62)
    live = remaining > 0
    short = live & (run[..., -1] < remaining)
    if short.any():
        k, z, s = (int(v) for v in np.argwhere(short)[0])
        raise ValueError('the histogram of layer %d, zone %d, slot %d holds less than its target' % (k, z, s))
    run = np.broadcast_to(run, remaining.shape + run.shape[-1:])      # (level 0: every slot reads slot 0's row)
    b = (run >= remaining[..., None]).argmax(axis=-1)                  # the first bin that reaches it
    here = np.take_along_axis(np.broadcast_to(rows[..., :1 << d], run.shape), b[..., None], axis=-1)[..., 0]
    before = np.take_along_axis(run, b[..., None], axis=-1)[..., 0] - here
    remaining = np.where(live, remaining - before, remaining)
    prefix = np.where(live, (prefix << np.uint64(d)) | b.astype(np.uint64), prefix)
    return remaining, prefix


class ZonalQuantiles(object):
    '''``values`` ``(K, Z, S)`` in the rasters' dtype (NaN where a zone and layer holds no weight),
    ``weight`` ``(K, Z)`` int64 (the total weight word: the count without weights), ``q`` and ``ew``
    (``weight * 2**(ew - 31)`` is the sum of the weights as they were quantised; 31 without weights).'''

    def __init__(self, values, weight, q=None, ew=31, squeeze=False):
        self.values = np.asarray(values)
        self.weight = np.asarray(weight, np.int64)
        if self.values.ndim != 3 or self.weight.shape != self.values.shape[:2]:
            raise ValueError('values must be (K, Z, S) and weight (K, Z)')
        self.q = None if q is None else tuple(q)
        self.ew = int(ew)
        if squeeze:
            self.values, self.weight = self.values[0], self.weight[0]


def finish(prefix, remaining, dtype):
    '''The values of a finished selection: ``unukey(prefix)``, NaN where ``remaining == 0``.'''
    out = unukey(prefix, dtype).copy()
    out[np.asarray(remaining) == 0] = np.nan
    return out


def quantiles(values, zones, nzones, q=DEFAULT_Q, weights=None, cols=None, first_pixel=0, wmax=None, bits=DEFAULT_BITS):
    '''The loop over the levels: -> ``ZonalQuantiles``.'''
    qs = check_q(q)
    bits = check_bits(bits)
    values = np.asarray(values)
    wd = width(values.dtype)
    kw = dict(weights=weights, cols=cols, first_pixel=first_pixel, wmax=wmax)
    hist = digits(values, zones, nzones, 0, bits, slots=len(qs), **kw)
    weight = hist[:, :, 0].sum(axis=-1)
    remaining = targets(qs, weight)
    prefix = np.zeros(remaining.shape, np.uint64)
    for level in range(levels(wd, bits)):
        if level:
            hist = digits(values, zones, nzones, level, bits, prefix, **kw)
        remaining, prefix = select(hist, remaining, prefix, level, bits, wd)
    ew = 31 if weights is None else check_wmax(wmax)[1]
    return ZonalQuantiles(finish(prefix, remaining, values.dtype), weight, qs, ew)


class ZonalHistogram(object):
    '''The table of a uniform zonal histogram and what fixes its meaning: ``words`` ``(K, Z, bins + 2)``
    int64, ``lo``, ``hi``, ``bins``, ``ew`` (a word times ``2**(ew - 31)`` is a sum of weights; without
    weights ``ew`` is 31 and a word is a count).'''

    def __init__(self, words, lo, hi, ew=31, squeeze=False):
        words = np.asarray(words, np.int64)
        if words.ndim != 3 or words.shape[2] < 3:
            raise ValueError('words must have shape (K, Z, bins + 2), got %r' % (words.shape,))
        self.words = words
        self.bins = words.shape[2] - 2
        self.lo, self.hi, _ = check_range(self.bins, lo, hi)
        self.ew = int(ew)
        self.squeeze = bool(squeeze)

    def _out(self, a):
        return a[0] if self.squeeze else a

    @property
    def edges(self):
        '''The ``bins + 1`` edges ``lo + i * (hi - lo) / bins`` (the last one is ``hi``).'''
        e = self.lo + np.arange(self.bins + 1) * ((self.hi - self.lo) / self.bins)
        e[-1] = self.hi
        return e

    @property
    def under(self):
        return self._out(self.words[..., 0].copy())

    @property
    def over(self):
        return self._out(self.words[..., -1].copy())

    @property
    def counts(self):
        return self._out(self.words[..., 1:-1].copy())

    def merge(self, other):
        '''The histogram of everything added into either; ValueError unless range, bins and ``ew`` agree.'''
        mine, theirs = (self.lo, self.hi, self.bins, self.ew), (other.lo, other.hi, other.bins, other.ew)
        if mine != theirs or self.words.shape != other.words.shape:
            raise ValueError('histograms over %r and %r cannot be merged' % (mine, theirs))
        return ZonalHistogram(self.words + other.words, self.lo, self.hi, self.ew, self.squeeze)
