"""The definition of the zonal histograms and exact zonal quantiles (mod16_amd/zonalq.py) held to
things that do not share its code: a per-pixel Python loop (stable sort by key, cumulative sum in
Python integers, the exact rational target), np.quantile(..., method='inverted_cdf') for unit weights
and dyadic q (for other q numpy rounds q * n in floating point and may pick the neighbour: 0.1 * 10),
and np.histogram on integer-valued data with integer edges. No library, no device."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from mod16_amd import zonal as Z
from mod16_amd import zonalq as Q

DTYPES = (np.float32, np.float64)
BITS = (4, 8, 11, 12)
QS = (0.0, 5e-324, 0.1, 0.25, 0.5, 0.75, 1 - 2.0 ** -53, 1.0)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def key_of(x, dtype):
    '''The order-preserving unsigned key of one value, from its bytes (not the module's code).'''
    if dtype == np.float32:
        b, = struct.unpack('<I', struct.pack('<f', x))
        return b ^ 0xffffffff if b >> 31 else b | 0x80000000
    b, = struct.unpack('<Q', struct.pack('<d', x))
    return b ^ 0xffffffffffffffff if b >> 63 else b | (1 << 63)


def brute(values, zones, nzones, qs, w=None, wmax=None):
    '''Per pixel, in Python: -> (values (K, Z, S), weight (K, Z)).'''
    K, n = values.shape
    dtype = values.dtype.type
    ew = None if w is None else Z.exponent(wmax)
    out = np.full((K, nzones, len(qs)), np.nan, values.dtype)
    weight = np.zeros((K, nzones), np.int64)
    for k in range(K):
        per = [[] for _ in range(nzones)]
        for i in range(n):
            z, x = int(zones[i]), values[k, i]
            if not 0 <= z < nzones or x != x:
                continue
            if w is None:
                qw = 1
            else:
                wi = float(w[i])
                if wi != wi or not 0.0 <= wi <= wmax:
                    continue
                qw = int(Fraction(wi) * Fraction(2) ** (31 - ew) + Fraction(1, 2))        # round half ...
                if Fraction(wi) * Fraction(2) ** (31 - ew) + Fraction(1, 2) == qw and qw % 2:
                    qw -= 1                                                                # ... to even
            per[z].append((key_of(x, dtype), x, qw))
        for z in range(nzones):
            items = sorted(per[z], key=lambda t: t[0])
            W = sum(t[2] for t in items)
            weight[k, z] = W
            if W == 0:
                continue
            for s, q in enumerate(qs):
                target = max(1, math.ceil(Fraction(q) * W))
                run = 0
                for _, x, qw in items:
                    run += qw
                    if run >= target:
                        out[k, z, s] = x
                        break
    return out, weight


def raster(rng, dtype, K, n, nzones, special=True):
    x = rng.normal(3.0, 2.0, (K, n)).astype(dtype)
    x[rng.random((K, n)) < 0.05] = np.nan
    if special and n >= 16:
        x[0, :8] = [0.0, -0.0, np.inf, -np.inf, 0.0, -0.0, 1.0, np.nextafter(dtype(1.0), dtype(2.0))]
    zones = rng.integers(-1, nzones + 1, n).astype(np.int32)          # (-1 and nzones: out of range)
    return x, zones


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('bits', BITS)
def test_quantiles_equal_the_per_pixel_loop(dtype, bits):
    rng = np.random.default_rng(bits * 7 + np.dtype(dtype).itemsize)
    x, zones = raster(rng, dtype, 2, 300, 5)
    zones[zones == 3] = 0                                    # zone 3 is empty
    x[:, zones == 4] = np.nan                                # zone 4 is all NaN
    ref, wref = brute(x, zones, 5, QS)
    got = Q.quantiles(x, zones, 5, QS, bits=bits)
    assert np.array_equal(bits_of(got.values), bits_of(ref)) and np.array_equal(got.weight, wref)
    assert np.isnan(got.values[:, 3:]).all() and (got.weight[:, 3:] == 0).all()
    assert got.values.dtype == dtype and got.q == QS and got.ew == 31


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('bits', (8, 11))
def test_weighted_quantiles_equal_the_per_pixel_loop(dtype, bits):
    rng = np.random.default_rng(11 + bits)
    n, nzones = 260, 3
    x, zones = raster(rng, dtype, 2, n, nzones)
    wmax = 3.0e5
    ew = Z.exponent(wmax)
    w = rng.uniform(0.0, wmax, n)
    w[:10] = [0.0, wmax, 2.0 ** (ew - 33), 2.0 ** (ew - 32), 1.5 * 2.0 ** (ew - 32), np.nan, -1.0, wmax * 1.0001, np.inf, 2.0 ** (ew - 31)]
    w = w.astype(dtype)
    ref, wref = brute(x, zones, nzones, QS, w.astype(np.float64), wmax)
    got = Q.quantiles(x, zones, nzones, QS, weights=w, wmax=wmax, bits=bits)
    assert np.array_equal(bits_of(got.values), bits_of(ref)) and np.array_equal(got.weight, wref)
    assert got.ew == ew
    # per-row weights: the same numbers through the (first_pixel + p) // cols rule
    cols, first = 7, 4
    per_row = rng.integers(0, 2 ** 31 + 1, (first + n - 1) // cols + 1).astype(np.float64)     # ew = 31: the word is the weight
    per_row[:2] = [2.0 ** 31, 0.0]
    ref, wref = brute(x, zones, nzones, QS, per_row[(first + np.arange(n)) // cols], 2.0 ** 31)
    got = Q.quantiles(x, zones, nzones, QS, weights=per_row, cols=cols, first_pixel=first, wmax=2.0 ** 31, bits=bits)
    assert np.array_equal(bits_of(got.values), bits_of(ref)) and np.array_equal(got.weight, wref)


@pytest.mark.parametrize('dtype', DTYPES)
def test_quantiles_equal_numpy_inverted_cdf_for_dyadic_q(dtype):
    rng = np.random.default_rng(5)
    x, zones = raster(rng, dtype, 3, 500, 4, special=False)
    qs = (0.0, 0.125, 0.25, 0.5, 0.75, 0.875, 1.0)
    for bits in BITS:
        got = Q.quantiles(x, zones, 4, qs, bits=bits)
        for k in range(3):
            for z in range(4):
                v = x[k][(zones == z) & ~np.isnan(x[k])]
                ref = np.quantile(v, qs, method='inverted_cdf').astype(dtype)
                assert np.array_equal(bits_of(got.values[k, z]), bits_of(ref)), (bits, k, z)
                assert got.weight[k, z] == len(v)


@pytest.mark.parametrize('dtype', DTYPES)
def test_edge_rasters(dtype):
    one, two = dtype(1.0), np.nextafter(dtype(1.0), dtype(2.0))
    zones = np.zeros(9, np.int32)
    for bits in BITS:
        # a constant raster
        got = Q.quantiles(np.full((1, 9), 2.5, dtype), zones, 1, QS, bits=bits)
        assert (got.values == dtype(2.5)).all() and got.weight[0, 0] == 9
        # two values that differ in the last key bit only
        x = np.array([[one, two, one, two, two, one, two, one, two]], dtype)
        got = Q.quantiles(x, zones, 1, (0.0, 4 / 9, 0.5, 1.0), bits=bits)
        assert np.array_equal(bits_of(got.values[0, 0]), bits_of(np.array([one, one, two, two], dtype)))
        # signed zeros and infinities order as -inf < -0.0 < +0.0 < +inf
        x = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, np.nan, np.nan, np.nan, np.nan]], dtype)
        got = Q.quantiles(x, zones, 1, (0.0, 0.5, 0.75, 1.0), bits=bits)
        assert np.array_equal(bits_of(got.values[0, 0]), bits_of(np.array([-np.inf, -0.0, 0.0, np.inf], dtype)))
    # ids out of range count for nothing; an empty and an all-NaN zone give NaN and weight 0
    x = np.array([[1.0, 2.0, np.nan, 4.0]], dtype)
    got = Q.quantiles(x, np.array([-1, 5, 2, 0]), 4, 0.5)
    assert got.weight.tolist() == [[1, 0, 0, 0]] and got.values[0, 0, 0] == 4.0 and np.isnan(got.values[0, 1:]).all()


def test_weights_of_zero_of_wmax_and_below_the_quantum():
    x = np.array([[1.0, 2.0, 3.0, 4.0]], np.float64)
    zones = np.zeros(4, np.int32)
    wmax = 8.0                                             # ew = 3: the quantum is 2**-28, half of it 2**-29
    got = Q.quantiles(x, zones, 1, (0.0, 1.0), weights=np.array([0.0, 2.0 ** -30, wmax, 2.0 ** -29 * 0.99]), wmax=wmax)
    assert got.weight[0, 0] == 2 ** 31 and got.values[0, 0].tolist() == [3.0, 3.0]
    got = Q.quantiles(x, zones, 1, (0.0, 1.0), weights=np.array([2.0 ** -28, 0.0, 0.0, wmax * 2]), wmax=wmax)
    assert got.weight[0, 0] == 1 and got.values[0, 0].tolist() == [1.0, 1.0]


def test_target_is_the_exact_rational():
    assert Q.rational(0.0) == (0, 53) and Q.rational(1.0) == (2 ** 52, 52) and Q.rational(0.5) == (2 ** 52, 53)
    for q in QS + (0.3, 1e-300, 2.0 ** -1074 * 3):
        M, E = Q.rational(q)
        assert Fraction(M, 2 ** E) == Fraction(q)
        for W in (1, 2, 3, 10, 2 ** 31, 2 ** 62 - 1, 12345678901234567):
            assert Q.target(q, W) == max(1, math.ceil(Fraction(q) * W)), (q, W)
    assert Q.target(0.5, 0) == 0
    assert Q.target(0.1, 10) == 2           # 0.1 as a double lies above 1 / 10: the exact rule, not numpy's


@pytest.mark.parametrize('dtype', DTYPES)
def test_histogram_equals_numpy_on_integer_data(dtype):
    rng = np.random.default_rng(3)
    n, nzones = 800, 3
    x = rng.integers(-5, 45, (2, n)).astype(dtype)
    zones = rng.integers(0, nzones, n).astype(np.uint8)
    for bins, lo, hi in ((1, 0, 40), (40, 0, 40), (20, 0, 40), (8, -4, 44)):
        words = Q.histogram(x, zones, nzones, bins, lo, hi)
        assert words.shape == (2, nzones, bins + 2) and words.dtype == np.int64
        for k in range(2):
            for z in range(nzones):
                v = x[k][zones == z].astype(np.float64)
                ref, edges = np.histogram(v[(v >= lo) & (v < hi)], bins=bins, range=(lo, hi))
                assert np.array_equal(words[k, z, 1:-1], ref)
                assert words[k, z, 0] == (v < lo).sum() and words[k, z, -1] == (v >= hi).sum()
    h = Q.ZonalHistogram(words, lo, hi)
    assert np.array_equal(h.edges, edges) and h.bins == 8 and h.ew == 31
    assert np.array_equal(h.counts, words[..., 1:-1]) and np.array_equal(h.under, words[..., 0]) and np.array_equal(h.over, words[..., -1])


def test_histogram_special_values_and_the_top_edge():
    x = np.array([[np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, np.nextafter(1.0, 0.0), 0.3]], np.float64)
    zones = np.zeros(8, np.int32)
    words = Q.histogram(x, zones, 1, 3, 0.0, 1.0)
    # -inf under; +inf and 1.0 over; the value just under hi clamps into the last bin; both zeros in bin 1
    assert words[0, 0].tolist() == [1, 3, 0, 1, 2]
    words = Q.histogram(x, zones, 1, 3, 0.0, 1.0, weights=np.full(8, 0.5), wmax=1.0)
    assert words[0, 0].tolist() == [2 ** 30, 3 * 2 ** 30, 0, 2 ** 30, 2 ** 31]


@pytest.mark.parametrize('dtype', DTYPES)
def test_merging_and_accumulating_equal_one_call(dtype):
    rng = np.random.default_rng(9)
    n, nzones = 400, 4
    x, zones = raster(rng, dtype, 2, n, nzones)
    w = rng.uniform(0, 9.0, n).astype(dtype)
    kw = dict(wmax=9.0)
    cut = 151
    whole = Q.histogram(x, zones, nzones, 16, -2.0, 8.0, weights=w, **kw)
    a = Q.histogram(x[:, :cut], zones[:cut], nzones, 16, -2.0, 8.0, weights=w[:cut], **kw)
    b = Q.histogram(x[:, cut:], zones[cut:], nzones, 16, -2.0, 8.0, weights=w[cut:], **kw)
    both = Q.histogram(x[:, cut:], zones[cut:], nzones, 16, -2.0, 8.0, weights=w[cut:], acc=a, **kw)
    assert np.array_equal(whole, a + b) and np.array_equal(whole, both)
    ha, hb = Q.ZonalHistogram(a, -2.0, 8.0, 4), Q.ZonalHistogram(b, -2.0, 8.0, 4)
    assert np.array_equal(ha.merge(hb).words, whole)
    with pytest.raises(ValueError):
        ha.merge(Q.ZonalHistogram(b, -2.0, 8.0, 5))
    with pytest.raises(ValueError):
        ha.merge(Q.ZonalHistogram(b, -2.0, 9.0, 4))
    # the levels of a selection: the digit tables of the parts add up to the whole's, level by level
    qs, bits, wd = (0.1, 0.5), 11, Q.width(dtype)
    rem = pre = None
    for level in range(Q.levels(wd, bits)):
        hw = Q.digits(x, zones, nzones, level, bits, pre, weights=w, slots=2, **kw)
        pa = Q.digits(x[:, :cut], zones[:cut], nzones, level, bits, pre, weights=w[:cut], slots=2, **kw)
        pb = Q.digits(x[:, cut:], zones[cut:], nzones, level, bits, pre, weights=w[cut:], slots=2, acc=pa, **kw)
        assert np.array_equal(hw, pb)
        if level == 0:
            assert (hw[:, :, 1] == 0).all()                 # level 0 counts into slot 0 only
            rem, pre = Q.targets(qs, hw[:, :, 0].sum(-1)), np.zeros((2, nzones, 2), np.uint64)
        rem, pre = Q.select(hw, rem, pre, level, bits, wd)
    ref = Q.quantiles(x, zones, nzones, qs, weights=w, bits=bits, **kw)
    assert np.array_equal(bits_of(Q.finish(pre, rem, dtype)), bits_of(ref.values))
    # first_pixel: a part of a raster with per-row weights is the part of the whole
    rows = rng.uniform(0, 9.0, n // 10 + 1)
    whole = Q.histogram(x, zones, nzones, 16, -2.0, 8.0, weights=rows, cols=10, **kw)
    a = Q.histogram(x[:, :cut], zones[:cut], nzones, 16, -2.0, 8.0, weights=rows, cols=10, **kw)
    both = Q.histogram(x[:, cut:], zones[cut:], nzones, 16, -2.0, 8.0, weights=rows, cols=10, first_pixel=cut, acc=a, **kw)
    assert np.array_equal(whole, both)


def test_every_value_error():
    x = np.zeros((1, 4), np.float32)
    zones = np.zeros(4, np.int32)
    for q in (-0.1, 1.0000001, np.nan, [0.5, 2.0], [], [0.5] * 17, 'a'):
        with pytest.raises(ValueError):
            Q.quantiles(x, zones, 1, q)
    for bits in (3, 13, 8.0, True):
        with pytest.raises(ValueError):
            Q.quantiles(x, zones, 1, 0.5, bits=bits)
    for bins in (0, 4095, 2.0, False):
        with pytest.raises(ValueError):
            Q.histogram(x, zones, 1, bins, 0.0, 1.0)
    for lo, hi in ((0.0, 0.0), (1.0, 0.0), (np.nan, 1.0), (0.0, np.inf), (-np.inf, 0.0), (-1.7e308, 1.7e308), (0.0, 5e-324)):
        with pytest.raises(ValueError):
            Q.histogram(x, zones, 1, 4, lo, hi)
    with pytest.raises(ValueError):
        Q.histogram(x.astype(np.float16), zones, 1, 4, 0.0, 1.0)
    with pytest.raises(ValueError):
        Q.histogram(x[0], zones, 1, 4, 0.0, 1.0)                          # no layer axis
    with pytest.raises(ValueError):
        Q.histogram(x, zones[:3], 1, 4, 0.0, 1.0)
    with pytest.raises(ValueError):
        Q.histogram(x, zones.astype(np.float32), 1, 4, 0.0, 1.0)
    with pytest.raises(ValueError):
        Q.histogram(x, zones, 0, 4, 0.0, 1.0)
    with pytest.raises(ValueError):
        Q.histogram(x, zones, 1, 4, 0.0, 1.0, acc=np.zeros((1, 1, 5), np.int64))
    with pytest.raises(ValueError):
        Q.histogram(x, zones, 1, 4, 0.0, 1.0, weights=np.ones(4, np.float32))        # weights need wmax
    for wmax in (0.0, -1.0, np.inf, np.nan, 2.0 ** 1000):
        with pytest.raises(ValueError):
            Q.histogram(x, zones, 1, 4, 0.0, 1.0, weights=np.ones(4, np.float32), wmax=wmax)
    with pytest.raises(ValueError):
        Q.histogram(x, zones, 1, 4, 0.0, 1.0, weights=np.ones(3, np.float32), wmax=1.0)
    for level in (-1, 4, 1.0):
        with pytest.raises(ValueError):
            Q.digits(x, zones, 1, level, 8, np.zeros((1, 1, 1), np.uint64))
    with pytest.raises(ValueError):
        Q.digits(x, zones, 1, 1, 8)                                       # a level above 0 needs prefixes
    with pytest.raises(ValueError):
        Q.digits(x, zones, 1, 1, 8, np.zeros((1, 1, 1), np.int64))
    with pytest.raises(ValueError):
        Q.digits(x, zones, 1, 1, 8, np.zeros((1, 2, 1), np.uint64))
    with pytest.raises(ValueError):
        Q.digits(x, zones, 1, 0, 8, slots=17)
    with pytest.raises(ValueError):
        Q.digits(x, zones, 1, 0, 8, acc=np.zeros((1, 1, 1, 255), np.int64))
    with pytest.raises(ValueError):
        Q.select(np.zeros((1, 1, 1, 255), np.int64), np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), 0, 8)
    with pytest.raises(ValueError):
        Q.select(np.zeros((1, 1, 1, 256), np.int64), np.ones((1, 1, 1)), np.zeros((1, 1, 1)), 0, 8)   # less than its target
    with pytest.raises(ValueError):
        Q.check_acc_wmax(None)
    with pytest.raises(ValueError):
        Q.ZonalHistogram(np.zeros((1, 1, 2), np.int64), 0.0, 1.0)
    with pytest.raises(ValueError):
        Q.ZonalQuantiles(np.zeros((1, 1, 1)), np.zeros((2, 1)))
    assert Q.levels(32, 11) == 3 and Q.levels(64, 11) == 6 and Q.levels(32, 12) == 3 and Q.levels(64, 12) == 6
