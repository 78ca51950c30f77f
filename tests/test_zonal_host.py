"""The numpy definition of the zonal statistics (mod16_amd/zonal.py) against Python big integers
and exact rationals, and the argument checks of the Python layer. No GPU: the GPU tests
(tests/test_gpu_zonal.py) hold the kernels to `zonal.accumulate` word for word.

Every bound here is derived, none is measured: a quantised term differs from its float64 term by at
most half a unit of 2**-F, and F = 62 - e where 2**e bounds the term, so n terms are within n *
2**(e - 63) of their exact sum; `to_float` adds one rounding of the result (hi stays below 2**53 here,
so its conversion and hi * 2**32 are exact and only the sum with lo rounds: half an ulp)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from mod16_amd import zonal as zs

K_HOST = 2
N_HOST = 20000
Z_HOST = 7


def recipe(n=N_HOST, layers=K_HOST, nzones=Z_HOST, seed=11, dtype=np.float64):
    """(values (K, n), zones (n,) int32 drawn from 0 .. Z + 1, per-pixel weights near 2e5): gamma
    values, 5 % NaN, every 17th negative."""
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, 1.5, size=(layers, n))
    x[rng.random((layers, n)) < 0.05] = np.nan
    x[:, ::17] *= -1.0
    w = 2e5 * (1.0 + 0.1 * rng.random(n))
    z = rng.integers(0, nzones + 2, size=n).astype(np.int32)
    return x.astype(dtype), z, w.astype(dtype)


def big_sums(x, z, w, nzones, bounds):
    """Per layer and zone: (count, [Q0, Q1, Q2] as Python integers, [exact rational sums of the
    float64 terms], [the terms' exponent bounds]) by a scalar loop."""
    wmax, xmax, ew, ex = zs.check_bounds(bounds)
    F = zs.fractional_bits(ew, ex)
    out = {}
    for k in range(x.shape[0]):
        for zone in range(nzones):
            out[k, zone] = [0, [0, 0, 0], [Fraction(0)] * 3]
        for i in range(x.shape[1]):
            xi, wi, zi = float(x[k, i]), float(w[i]), int(z[i])
            if not 0 <= zi < nzones or math.isnan(xi) or math.isnan(wi):
                continue
            if not abs(xi) <= xmax or not 0 <= wi <= wmax:
                continue
            terms = (wi, wi * xi, (wi * xi) * xi)
            e = out[k, zi]
            e[0] += 1
            for j, t in enumerate(terms):
                e[1][j] += int(np.rint(np.ldexp(np.float64(t), F[j])))
                e[2][j] = e[2][j] + Fraction(t)
    return out, F, (ew, ew + ex, ew + 2 * ex)


@pytest.fixture(scope='module')
def checked():
    x, z, w = recipe()
    bounds = (2.5e5, 64.0)
    acc = zs.accumulate(x, z, Z_HOST, weights=w, bounds=bounds)
    return x, z, w, bounds, acc, big_sums(x, z, w, Z_HOST, bounds)


def test_exponent_at_and_around_powers_of_two():
    for e in (-1074, -1022, -3, 0, 1, 10, 62, 1023):
        b = math.ldexp(1.0, e)
        assert zs.exponent(b) == e
        assert 2.0 ** zs.exponent(b) >= b
        if e > -1074:
            assert zs.exponent(np.nextafter(b, 0.0)) == e
        if e < 1023:
            assert zs.exponent(np.nextafter(b, np.inf)) == e + 1
    assert zs.exponent(3.0) == 2 and zs.exponent(0.75) == 0 and zs.exponent(2e5) == 18
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            zs.exponent(bad)
    assert zs.fractional_bits(18, 6) == (44, 38, 32)
    f = zs.fractional_bits(-5, 9)
    assert f[0] + f[2] == 2 * f[1]


def test_accumulate_equals_big_integer_sums(checked):
    x, z, w, bounds, acc, (sums, F, _) = checked
    assert acc.shape == (K_HOST, Z_HOST, 10) and acc.dtype == np.int64
    for (k, zone), (count, Q, _) in sums.items():
        wd = acc[k, zone]
        assert wd[zs.COUNT] == count > 1000
        for j in range(3):
            assert zs.to_int(wd[zs.W_HI + 2 * j], wd[zs.W_LO + 2 * j]) == Q[j]
            assert 0 <= wd[zs.W_LO + 2 * j] < count << 32
    assert not acc[..., zs.REJECTED].any()


def test_to_float_is_within_the_derived_bound_of_the_exact_sums(checked):
    x, z, w, bounds, acc, (sums, F, E) = checked
    res = zs.ZonalResult(acc, zs.exponent(bounds[0]), zs.exponent(bounds[1]))
    got = (res.sum_w, res.sum_wx, res.sum_wxx)
    for (k, zone), (count, _, exact) in sums.items():
        for j in range(3):
            value = float(got[j][k, zone])
            bound = Fraction(count) * Fraction(2) ** (E[j] - 63) + Fraction(math.ulp(value)) / 2
            assert abs(Fraction(value) - exact[j]) <= bound, (k, zone, j)


def test_variance_is_the_exact_rational_of_the_quantised_terms_rounded_once(checked):
    x, z, w, bounds, acc, (sums, F, _) = checked
    ex = zs.exponent(bounds[1])
    res = zs.ZonalResult(acc, zs.exponent(bounds[0]), ex)
    var, std, mean = res.var, res.std, res.mean
    for (k, zone), (count, Q, _) in sums.items():
        # sum q2 / 2^F2 / (sum q0 / 2^F0) - (sum q1 / 2^F1 / (sum q0 / 2^F0))^2
        s0, s1, s2 = (Fraction(Q[j]) / Fraction(2) ** F[j] for j in range(3))
        exact = s2 / s0 - (s1 / s0) ** 2
        assert var[k, zone] == float(exact)
        assert std[k, zone] == math.sqrt(float(exact))
        assert mean[k, zone] == res.sum_wx[k, zone] / res.sum_w[k, zone]
    none = zs.ZonalResult(zs.empty(1, 3), 0, 0)
    assert np.isnan(none.var).all() and np.isnan(none.mean).all() and np.isnan(none.min).all()


def test_merge_of_two_halves_is_the_whole(checked):
    x, z, w, bounds, acc, _ = checked
    h = N_HOST // 2 + 3
    a = zs.accumulate(x[:, :h], z[:h], Z_HOST, weights=w[:h], bounds=bounds)
    b = zs.accumulate(x[:, h:], z[h:], Z_HOST, weights=w[h:], bounds=bounds)
    assert np.array_equal(zs.merge(a, b), acc)
    assert np.array_equal(zs.accumulate(x[:, h:], z[h:], Z_HOST, weights=w[h:], bounds=bounds, acc=a), acc)
    ra, rb = zs.ZonalResult(a, 18, 6), zs.ZonalResult(b, 18, 6)
    assert np.array_equal(ra.merge(rb).words, acc)
    with pytest.raises(ValueError, match='exponents'):
        ra.merge(zs.ZonalResult(b, 18, 7))
    # per-row weights: a sub-range that starts in the middle of a row addresses the same rows
    row_w = np.linspace(1.0, 2.0, 400)
    whole = zs.accumulate(x, z, Z_HOST, weights=row_w, cols=67, bounds=(2.0, 64.0))
    first = zs.accumulate(x[:, :h], z[:h], Z_HOST, weights=row_w, cols=67, bounds=(2.0, 64.0))
    both = zs.accumulate(x[:, h:], z[h:], Z_HOST, weights=row_w, cols=67, first_pixel=h, bounds=(2.0, 64.0), acc=first)
    assert np.array_equal(both, whole)


def test_masked_rejected_and_ignored_pixels_leave_the_words_the_definition_names():
    fresh = zs.empty(1, 2)
    bounds = (2.0, 8.0)

    def run(x, w, zone=0):
        return zs.accumulate(np.array([[x]], np.float64), np.array([zone], np.int32), 2,
                             weights=np.array([w], np.float64), bounds=bounds)
    for x, w, zone in ((1.0, 1.0, 2), (1.0, 1.0, -1), (np.nan, 1.0, 0), (1.0, np.nan, 0), (np.nan, np.inf, 0),
                       (np.inf, np.nan, 0)):
        assert np.array_equal(run(x, w, zone), fresh), (x, w, zone)          # ignored, masked
    for x, w in ((np.nextafter(8.0, 9.0), 1.0), (np.inf, 1.0), (-np.inf, 1.0), (1.0, np.nextafter(2.0, 3.0)),
                 (1.0, np.inf), (1.0, -1e-300), (1.0, -np.inf)):
        want = fresh.copy()
        want[0, 0, zs.REJECTED] = 1
        assert np.array_equal(run(x, w), want), (x, w)                       # rejected
    # valid at the bounds themselves: the largest terms, q = 2^62 where the bounds are powers of two
    got = run(-8.0, 2.0, zone=1)
    want = fresh.copy()
    want[0, 1] = [1, 0, 2 ** 30, 0, -2 ** 30, 0, 2 ** 30, 0, zs.key(-8.0), zs.key(-8.0)]
    assert np.array_equal(got, want)
    got = run(0.0, 0.0)              # w = 0 is valid: counted, no weight
    assert got[0, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    got = zs.accumulate(np.array([[0.0, -0.0]]), np.array([0, 0]), 2, bounds=bounds)
    assert got[0, 0, zs.MIN_KEY] == -1 and got[0, 0, zs.MAX_KEY] == 0         # -0.0 < +0.0
    res = zs.ZonalResult(got, 1, 3)
    assert math.copysign(1.0, res.min[0, 0]) == -1.0 and math.copysign(1.0, res.max[0, 0]) == 1.0
    # a negative term splits into an arithmetic hi and a non-negative lo
    q, qh, ql = zs.quantise(np.array([-1.0]), 0)
    assert (q[0], qh[0], ql[0]) == (-1, -1, 0xffffffff)
    assert zs.to_float(np.int64(-1), np.int64(0xffffffff), 0) == -1.0


def test_key_orders_doubles():
    tiny = 5e-324
    v = np.array([-np.inf, -np.finfo(np.float64).max, -1.0, -2.2250738585072014e-308, -tiny, -0.0, 0.0, tiny,
                  2.2250738585072014e-308, 1.0, np.finfo(np.float64).max, np.inf])
    k = zs.key(v)
    assert k.dtype == np.int64 and (np.diff(k) > 0).all()
    assert np.array_equal(zs.unkey(k).view(np.int64), v.view(np.int64))
    rng = np.random.default_rng(3)
    r = np.sort(rng.standard_normal(1000) * 10.0 ** rng.integers(-300, 300, 1000))
    assert (np.diff(zs.key(r)) >= 0).all()


def test_value_errors_of_the_python_layer():
    import mod16_amd
    x, z, w = recipe(n=6 * 7, layers=2)
    x2, z2 = x.reshape(2, 6, 7), z.reshape(6, 7)
    call = mod16_amd.zonal_statistics
    with pytest.raises(ValueError, match='float32 or float64'):
        call(np.zeros((2, 6, 7), np.int32), z2)
    with pytest.raises(ValueError, match='integers'):
        call(x2, z2.astype(np.float32))
    with pytest.raises(ValueError, match='shape of zones'):
        call(x2[:, :5], z2)
    with pytest.raises(ValueError, match='nzones'):
        call(x2, z2, nzones=0)
    with pytest.raises(ValueError, match='nzones'):
        call(x2, z2, nzones=2 ** 24 + 1)
    with pytest.raises(ValueError, match='int32'):
        call(x2, z2.astype(np.int64) + 2 ** 40, nzones=4)
    with pytest.raises(ValueError, match='area'):
        call(x2, z2, nzones=4, area=np.ones(5))
    with pytest.raises(ValueError, match='area'):
        call(x2, z2, nzones=4, area=np.ones((6, 7), bool))
    with pytest.raises(ValueError, match='stage_bytes'):
        call(x2, z2, nzones=4, bounds=(1.0, 64.0), stage_bytes=-1)
    for bad in ((0.0, 1.0), (1.0, np.inf), (1.0, np.nan), (-1.0, 1.0), 5.0, (1e-300, 1.0), (1.0, 1e200)):
        with pytest.raises(ValueError, match='bound'):
            call(x2, z2, nzones=4, bounds=bad)
    acc = zs.ZonalResult(zs.empty(2, 4), 0, 6)
    with pytest.raises(ValueError, match='explicit bounds'):
        call(x2, z2, nzones=4, acc=acc)
    with pytest.raises(ValueError, match='exponents'):
        call(x2, z2, nzones=4, acc=acc, bounds=(1.0, 65.0))
    with pytest.raises(ValueError, match='words'):
        call(x2, z2, nzones=5, acc=acc, bounds=(1.0, 64.0))
    with pytest.raises(ValueError, match='ZonalResult'):
        call(x2, z2, nzones=4, acc=zs.empty(2, 4), bounds=(1.0, 64.0))
    with pytest.raises(ValueError):
        zs.accumulate(x, z.astype(np.float64), 4)
    with pytest.raises(ValueError):
        zs.accumulate(x, z, 4, acc=zs.empty(2, 5))
    with pytest.raises(ValueError):
        zs.merge(zs.empty(2, 4), zs.empty(2, 5))


def test_without_a_device_the_public_call_fails_loudly():
    import mod16_amd
    from mod16_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a GPU is present')
    x, z, _ = recipe(n=64, layers=1)
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        mod16_amd.zonal_statistics(x, z, nzones=Z_HOST, bounds=(1.0, 64.0))
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        mod16_amd.zonal_statistics(x, z, nzones=Z_HOST)
