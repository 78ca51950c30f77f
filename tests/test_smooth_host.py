"""The definition of the Whittaker smoother (mod16_amd/smooth.py: penalty_bands, weights_of, factor,
solve, smooth_values, encode, check_call) without a GPU and without the library: numpy only.

(a) against a scalar loop over pixels and slabs in plain Python floats with the same order of
    operations: bit for bit;
(b) against the dense solve of W + lam D'D (np.linalg.solve) on S in {1, 2, 3, 4, 5, 7, 23, 46, 138},
    both orders, lam in {0.5, 10, 1600, 1e5}, weights drawn from {0, 0.5, 1} with 40 % zeros, 400
    pixels each, for every pixel with count >= order: 1e-7 relative to max(1, max |z|) -- the
    recurrence measured 3.4e-9 against this solve at lam = 1e5, the bound leaves a factor of 30 for
    another BLAS -- and every d > 0 there;
(c) properties: lam -> tiny returns y, a line is reproduced by order 2, the envelope lifts and its
    pull on a planted low outlier shrinks monotonically, the uint8 encoding;
(d) every refusal of check_call with its message;
(e) smooth_series through a recording stand-in of the context."""
import math

import numpy as np
import pytest

import mod16_amd
from mod16_amd import _lib, smooth as sm
from test_entry_points_host import Ctx, Recorder
from test_gapfill_host import recipe, same_bits

GRADED = np.zeros(256)
for _q in range(256):
    if not (_q & 1) and not (_q & 4) and ((_q >> 3) & 3) in (0, 3):
        GRADED[_q] = {0: 1.0, 1: 0.5}.get(_q >> 5, 0.0)


# ---- (a) the scalar loop
def scalar_bands(S, order):
    D = [[0] * S for _ in range(max(S - order, 0))]
    for r in range(len(D)):
        for j, k in enumerate((-1, 1) if order == 1 else (1, -2, 1)):
            D[r][r + j] = k
    A = [[sum(D[r][i] * D[r][j] for r in range(len(D))) for j in range(S)] for i in range(S)]
    a0 = [float(A[i][i]) for i in range(S)]
    a1 = [float(A[i][i + 1]) if i + 1 < S else 0.0 for i in range(S)]
    a2 = [float(A[i][i + 2]) if i + 2 < S else 0.0 for i in range(S)]
    return a0, a1, a2


def div(a, b):
    """IEEE division of Python floats: no ZeroDivisionError."""
    with np.errstate(all='ignore'):
        return float(np.float64(a) / np.float64(b))


def scalar_pixel(y, w, lam, order, envelope):
    """One pixel, slab by slab in Python floats -> (z, d, count)."""
    S = len(y)
    a0, a1, a2 = scalar_bands(S, order)
    d, c, e = [0.0] * S, [0.0] * S, [0.0] * S

    def at(x, i):
        return x[i] if 0 <= i < S else 0.0
    for i in range(S):
        d[i] = ((w[i] + lam * a0[i]) - (at(c, i - 1) * at(c, i - 1)) * at(d, i - 1)) - (at(e, i - 2) * at(e, i - 2)) * at(d, i - 2)
        c[i] = div(lam * a1[i] - (at(d, i - 1) * at(c, i - 1)) * at(e, i - 1), d[i])
        e[i] = div(lam * a2[i], d[i])
    y = list(y)
    for rnd in range(envelope + 1):
        f, z = [0.0] * S, [0.0] * S
        for i in range(S):
            f[i] = (w[i] * y[i] - at(c, i - 1) * at(f, i - 1)) - at(e, i - 2) * at(f, i - 2)
        for i in range(S - 1, -1, -1):
            z[i] = (div(f[i], d[i]) - c[i] * at(z, i + 1)) - e[i] * at(z, i + 2)
        if rnd < envelope:
            y = [z[t] if w[t] > 0 and z[t] > y[t] else y[t] for t in range(S)]
    return z, d, sum(1 for x in w if x > 0)


def scalar_weights(values, weights, qc, table):
    S, n = values.shape
    y = [[0.0] * n for _ in range(S)]
    w = [[0.0] * n for _ in range(S)]
    for t in range(S):
        for p in range(n):
            v = values[t, p]
            have = v < 249 if values.dtype == np.uint8 else math.isfinite(float(v))
            wt = 1.0 if weights is None and qc is None else float(weights[t, p]) if weights is not None else float(table[qc[t, p]])
            if have and math.isfinite(wt) and wt > 0:
                y[t][p], w[t][p] = float(v), wt
    return y, w


def scalar_encode(z, count, min_valid, dtype, scale):
    if count < min_valid:
        return [255 if dtype == 'uint8' else np.nan] * len(z)
    if dtype == 'uint8':
        return [int(min(max(math.floor(v + 0.5), 0), 248)) for v in z]
    return [np.dtype(dtype).type(v * scale) for v in z]


def stack_weights(S, n, seed=1):
    """float32 weights with everything weights_of must drop: 0, NaN, negative, infinite."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0.5, 1, np.nan, -1, np.inf], np.float32), (S, n), p=[.2, .3, .3, .1, .05, .05])


@pytest.mark.parametrize('mode', ['none', 'stack', 'qc'])
@pytest.mark.parametrize('order,lam,envelope', [(1, 0.5, 0), (2, 1600.0, 0), (2, 10.0, 2), (1, 1600.0, 3)])
def test_definition_equals_the_scalar_loop(order, lam, envelope, mode):
    S, n = 23, 120
    values, qc, _ = recipe(S, n)
    kw = {'none': {}, 'stack': dict(weights=stack_weights(S, n)), 'qc': dict(qc=qc, qc_weight=GRADED)}[mode]
    for vin, dtype, scale in ((values, 'uint8', None), (values, 'float32', 0.01),
                              (np.where(values >= 249, np.nan, values * 0.37), 'float64', None)):
        got, cnt = sm.smooth(vin, lam=lam, order=order, envelope=envelope, min_valid=3, dtype=dtype, scale=scale,
                             count=True, **kw)
        y, w = scalar_weights(vin, kw.get('weights'), kw.get('qc'), GRADED)
        want = np.empty((S, n), dtype)
        for p in range(n):
            z, d, count = scalar_pixel([y[t][p] for t in range(S)], [w[t][p] for t in range(S)], lam, order, envelope)
            assert count == cnt[p]
            want[:, p] = scalar_encode(z, count, 3, dtype, scale or 1.0)
        assert same_bits(got, want), (dtype, mode)
    assert cnt.dtype == np.uint16 and (cnt >= 3).any()
    if mode == 'qc':            # (the recipe's planted pixels: never, and only once, reliable)
        assert (cnt < 3).any()


@pytest.mark.parametrize('S', [1, 2, 3, 4, 5])
def test_short_series_equal_the_scalar_loop(S):
    values, qc, _ = recipe(S, 64, seed=3)
    for order in (1, 2):
        got, cnt = sm.smooth(values, qc=qc, lam=10.0, order=order, envelope=1, min_valid=order, dtype='float64', count=True)
        y, w = scalar_weights(values, None, qc, sm.default_qc_weight())
        for p in range(64):
            z, d, count = scalar_pixel([y[t][p] for t in range(S)], [w[t][p] for t in range(S)], 10.0, order, 1)
            want = np.array(scalar_encode(z, count, order, 'float64', 1.0), np.float64)
            assert same_bits(got[:, p].copy(), want), (order, p)
        a0, a1, a2 = sm.penalty_bands(S, order)
        assert (a0.tolist(), a1.tolist(), a2.tolist()) == tuple(scalar_bands(S, order))
        if S <= order:
            assert not a0.any() and not a1.any() and not a2.any()


def test_penalty_bands_are_the_diagonals():
    assert [b.tolist() for b in sm.penalty_bands(6, 2)] == [[1, 5, 6, 6, 5, 1], [-2, -4, -4, -4, -2, 0], [1, 1, 1, 1, 0, 0]]
    assert [b.tolist() for b in sm.penalty_bands(4, 1)] == [[1, 2, 2, 1], [-1, -1, -1, 0], [0, 0, 0, 0]]
    assert [b.tolist() for b in sm.penalty_bands(3, 2)] == [[1, 4, 1], [-2, -2, 0], [1, 0, 0]]
    for S in (7, 46):
        for order in (1, 2):
            assert tuple(b.tolist() for b in sm.penalty_bands(S, order)) == tuple(scalar_bands(S, order))


# ---- (b) the dense solve
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('S', [1, 2, 3, 4, 5, 7, 23, 46, 138])
def test_definition_against_the_dense_solve(S, order):
    n = 400
    D = np.diff(np.eye(S), order, axis=0) if S > order else np.zeros((0, S))
    P = D.T @ D
    for k, lam in enumerate((0.5, 10.0, 1600.0, 1e5)):
        rng = np.random.default_rng(1000 * S + 10 * order + k)
        w = rng.choice([0.0, 0.5, 1.0], (S, n), p=[0.4, 0.3, 0.3])
        y = np.where(w > 0, rng.uniform(0, 100, (S, n)), 0.0)
        z = sm.smooth_values(y, w, lam, order)
        d, c, e = sm.factor(w, lam, order)
        solvable = np.flatnonzero((w > 0).sum(axis=0) >= order)
        assert solvable.size > (n // 2 if S > 2 else 20) or S < order      # (S < order: no pixel has `order` slabs)
        assert (d[:, solvable] > 0).all()
        worst = 0.0
        for p in solvable:
            ref = np.linalg.solve(np.diag(w[:, p]) + lam * P, w[:, p] * y[:, p])
            worst = max(worst, np.abs(ref - z[:, p]).max() / max(1.0, np.abs(ref).max()))
        print('S %d order %d lam %g: %.2e' % (S, order, lam, worst))
        assert worst <= 1e-7, (lam, worst)


# ---- (c) properties
def test_tiny_lam_returns_the_values():
    rng = np.random.default_rng(5)
    y = rng.uniform(0, 100, (46, 50))
    for order in (1, 2):
        z = sm.smooth_values(y, np.ones_like(y), 1e-13, order)
        assert np.abs(z - y).max() <= 1e-9


def test_order_two_reproduces_a_line():
    t = np.arange(46, dtype=np.float64)[:, None]
    y = 3.0 + 0.25 * t + np.zeros((46, 4))
    w = np.ones_like(y)
    w[5:9, 1] = 0.0          # ... through gaps, which are interpolated
    w[40:, 2] = 0.0
    for lam in (0.5, 10.0, 1600.0, 1e5):
        z = sm.smooth_values(np.where(w > 0, y, 0.0), w, lam, 2)
        assert np.abs(z - y).max() <= 1e-7 * 15.0, lam       # (the bound of the dense solve, relative to max |z|)


def test_envelope_lifts_towards_the_upper_envelope():
    S, dip = 46, 20
    t = np.arange(S)
    clean = 40.0 + 30.0 * np.sin(np.pi * t / (S - 1))
    y = clean.copy()
    y[dip] -= 35.0                       # one planted low outlier
    y = y[:, None]
    w = np.ones_like(y)
    w[30:33] = 0.0
    weighted = w[:, 0] > 0
    for order in (1, 2):
        fits = [sm.smooth_values(y, w, 10.0, order, k)[:, 0] for k in range(5)]
        pull = [clean[dip] - f[dip] for f in fits]
        for k in range(1, 5):
            assert 0 < pull[k] < pull[k - 1], (order, k)
        assert pull[4] < 0.5 * pull[0]
        # Order 1: W + lam D'D is a Stieltjes matrix, its inverse has no negative entry, so a fit never
        # falls anywhere when y is lifted. Order 2 has no such theorem: its equivalent kernel (Silverman 1984:
        # exp(-|u| / sqrt 2) sin(|u| / sqrt 2 + pi / 4) / 2, u in units of lam^(1/4) = 1.8 slabs) is positive
        # up to |u| = 3.3, i.e. 5.9 slabs, and has side lobes of at most 4.3 % of its peak: the fit rises
        # within two slabs of the dip and falls nowhere by more than 5 % of the 35 the dip can be lifted by.
        if order == 1:
            for k in range(1, 5):
                assert (fits[k][weighted] >= fits[0][weighted]).all()
                assert (fits[k][weighted] >= fits[k - 1][weighted]).all()
        else:
            near = weighted & (np.abs(t - dip) <= 2)
            for k in range(1, 5):
                assert (fits[k][near] >= fits[0][near]).all()
                assert (fits[k][weighted] >= fits[0][weighted] - 0.05 * 35.0).all()


def test_uint8_encoding_rounds_half_up_and_clips():
    z = np.array([[-3.0], [-0.5], [-0.500001], [0.49999], [0.5], [1.5], [2.5], [247.5], [248.4], [248.5], [300.0]])
    codes = sm.encode(z, np.array([11]), 3, 'uint8')
    assert codes.dtype == np.uint8 and codes.ravel().tolist() == [0, 0, 0, 0, 1, 2, 3, 248, 248, 248, 248]
    assert sm.encode(z, np.array([2]), 3, 'uint8').ravel().tolist() == [255] * 11
    f = sm.encode(z, np.array([11]), 3, 'float32', 0.1)
    assert f.dtype == np.float32 and f[5, 0] == np.float32(1.5 * 0.1)
    assert np.isnan(sm.encode(z, np.array([2]), 3, 'float64')).all()
    with pytest.raises(ValueError):
        sm.encode(z, np.array([11]), 3, 'int16')


def test_weights_of_marks_the_missing_slabs():
    v = np.array([[5], [249], [7], [8]], np.uint8)
    y, w = sm.weights_of(v)
    assert y.ravel().tolist() == [5, 0, 7, 8] and w.ravel().tolist() == [1, 0, 1, 1]
    y, w = sm.weights_of(v, weights=np.array([[0.5], [1], [np.nan], [-2]], np.float32))
    assert y.ravel().tolist() == [5, 0, 0, 0] and w.ravel().tolist() == [0.5, 0, 0, 0]
    y, w = sm.weights_of(v, qc=np.array([[0], [0], [32], [1]], np.uint8), qc_weight=GRADED)
    assert y.ravel().tolist() == [5, 0, 7, 0] and w.ravel().tolist() == [1, 0, 0.5, 0]
    # the default table is gapfill's default of acceptable bytes
    from mod16_amd import gapfill as gf
    assert np.array_equal(sm.default_qc_weight(), gf.default_good().astype(np.float64))
    y, w = sm.weights_of(np.array([[1.5], [np.inf], [np.nan]], np.float32))
    assert y.ravel().tolist() == [1.5, 0, 0] and w.ravel().tolist() == [1, 0, 0]
    with pytest.raises(ValueError):
        sm.weights_of(v.astype(np.int16))
    with pytest.raises(ValueError):
        sm.weights_of(v, weights=np.ones((4, 1), np.float32), qc=np.zeros((4, 1), np.uint8))


# ---- (d) the refusals
def test_check_call_accepts_and_returns():
    ok = (23, 600)
    S, shape, mode, table, lam, order, env, mv, name, scale = sm.check_call(ok, np.uint8, qc_shape=ok, lam=10)
    assert (S, shape, mode, lam, order, env, mv, name, scale) == (23, (600,), sm.WEIGHT_QC, 10.0, 2, 0, 3, 'uint8', 1.0)
    assert table.shape == (256,) and table.sum() == 8
    got = sm.check_call((4096, 2, 3), 'float32', weights_shape=(4096, 2, 3), lam=0.5, order=1, envelope=8, min_valid=1)
    assert got[:3] == (4096, (2, 3), sm.WEIGHT_STACK) and got[3] is None and got[8] == 'float32'
    assert sm.check_call(ok, np.uint8, lam=1.0, dtype='float64', scale=0.01)[8:] == ('float64', 0.01)
    assert sm.check_call(ok, np.float64, lam=1.0, dtype='float64')[2] == sm.WEIGHT_NONE
    assert sm.MAX_SLABS == 4096 and sm.MAX_SLABS >= 3 * 46


@pytest.mark.parametrize('kw,message', [
    (dict(shape=()), 'values must have a leading time axis'),
    (dict(shape=(0, 600)), 'the time axis must have between 1 and 4096 slabs, got 0'),
    (dict(shape=(4097, 600)), 'the time axis must have between 1 and 4096 slabs, got 4097'),
    (dict(in_dtype=np.int16), 'values must be uint8, float32 or float64'),
    (dict(in_dtype='nonsense'), 'values must be uint8, float32 or float64'),
    (dict(weights_shape=(23, 600), qc_shape=(23, 600)), 'weights and qc exclude each other'),
    (dict(weights_shape=(23, 601)), r'weights must have the shape of values \(23, 600\), got \(23, 601\)'),
    (dict(qc_shape=(22, 600)), r'qc must have the shape of values \(23, 600\), got \(22, 600\)'),
    (dict(qc_weight=np.ones(256)), 'qc_weight needs a qc layer'),
    (dict(qc_shape=(23, 600), qc_weight=np.ones(255)), r'qc_weight must have 256 entries \(one per QC byte\)'),
    (dict(qc_shape=(23, 600), qc_weight=np.ones((2, 128))), 'qc_weight must have 256 entries'),
    (dict(qc_shape=(23, 600), qc_weight=np.full(256, np.nan)), 'qc_weight must be finite and not negative'),
    (dict(qc_shape=(23, 600), qc_weight=np.full(256, -1.0)), 'qc_weight must be finite and not negative'),
    (dict(qc_shape=(23, 600), qc_weight=np.array(['x'] * 256)), 'qc_weight must be numeric'),
    (dict(lam=None), 'lam must be one finite number > 0, got None'),
    (dict(lam=0), 'lam must be one finite number > 0'),
    (dict(lam=-1.0), 'lam must be one finite number > 0'),
    (dict(lam=float('nan')), 'lam must be one finite number > 0'),
    (dict(lam=float('inf')), 'lam must be one finite number > 0'),
    (dict(lam=np.ones(3)), 'lam must be one finite number > 0'),
    (dict(lam='much'), 'lam must be one finite number > 0'),
    (dict(lam=True), 'lam must be one finite number > 0'),
    (dict(order=0), 'order must be 1 or 2, got 0'),
    (dict(order=3), 'order must be 1 or 2, got 3'),
    (dict(order=2.0), 'order must be an integer'),
    (dict(envelope=-1), 'envelope must be between 0 and 8, got -1'),
    (dict(envelope=9), 'envelope must be between 0 and 8, got 9'),
    (dict(envelope=1.5), 'envelope must be an integer'),
    (dict(envelope=True), 'envelope must be an integer'),
    (dict(min_valid=1), r'min_valid must be at least the order \(2\), got 1'),
    (dict(order=1, min_valid=0), r'min_valid must be at least the order \(1\), got 0'),
    (dict(min_valid=3.0), 'min_valid must be an integer'),
    (dict(dtype='int16'), "dtype must be 'uint8', 'float32' or 'float64'"),
    (dict(dtype='nonsense'), "dtype must be 'uint8', 'float32' or 'float64'"),
    (dict(in_dtype=np.float32, dtype='uint8'), 'float32 values return their own type'),
    (dict(in_dtype=np.float32, dtype='float64'), 'float32 values return their own type'),
    (dict(in_dtype=np.float64, dtype='float32'), 'float64 values return their own type'),
    (dict(scale=0.01), 'scale applies to uint8 values with float output only'),
    (dict(dtype='uint8', scale=0.01), 'scale applies to uint8 values with float output only'),
    (dict(in_dtype=np.float32, scale=0.01), 'scale applies to uint8 values with float output only'),
    (dict(dtype='float32', scale=float('nan')), 'scale must be one finite number'),
    (dict(dtype='float32', scale=(0.01, 0.1)), 'scale must be one finite number'),
])
def test_check_call_refuses(kw, message):
    base = dict(shape=(23, 600), in_dtype=np.uint8, lam=10.0)
    base.update(kw)
    with pytest.raises(ValueError, match=message):
        sm.check_call(**base)


def test_the_package_entry_point_checks_before_any_device_work():
    v = np.zeros((3, 8), np.uint8)
    with pytest.raises(ValueError, match='lam'):
        mod16_amd.smooth_series(v)
    with pytest.raises(ValueError, match='order'):
        mod16_amd.smooth_series(v, lam=1.0, order=3)
    with pytest.raises(ValueError, match='weights must be float32'):
        mod16_amd.smooth_series(v, weights=np.ones((3, 8)), lam=1.0)
    with pytest.raises(ValueError, match='qc must be uint8'):
        mod16_amd.smooth_series(v, qc=np.zeros((3, 8), np.int16), lam=1.0)
    with pytest.raises(ValueError, match='stage_bytes'):
        mod16_amd.smooth_series(v, lam=1.0, stage_bytes=-1)
    with pytest.raises(ValueError, match='out must hold 2 arrays'):
        mod16_amd.smooth_series(v, lam=1.0, count=True, out=np.empty((3, 8), np.uint8))
    with pytest.raises(ValueError, match=r'out\[0\] must be a writeable C-contiguous uint8 array'):
        mod16_amd.smooth_series(v, lam=1.0, out=np.empty((3, 8), np.float32))
    with pytest.raises(ValueError, match=r'out\[1\] must be a writeable C-contiguous uint16 array'):
        mod16_amd.smooth_series(v, lam=1.0, count=True, out=(np.empty((3, 8), np.uint8), np.empty((3, 8), np.uint16)))
    import mod16
    assert mod16.smooth_series is mod16_amd.smooth_series
    # nothing to do is done without a device as well
    out, cnt = mod16_amd.smooth_series(np.zeros((3, 0), np.float32), lam=1.0, count=True)
    assert out.shape == (3, 0) and out.dtype == np.float32 and cnt.shape == (0,) and cnt.dtype == np.uint16


# ---- (e) smooth_series through a recording stand-in
class SmoothCtx(Ctx):
    def smooth(self, in_dtype, out_type, n, slabs, values, weights, qc_weight, out, count, in_pitch, weight_pitch,
               out_pitch, lam, order=2, envelope=0, min_valid=3, weight_mode=0, scale=1.0, where=_lib.HOST, stream=None,
               stage_bytes=None):
        import ctypes as C
        self.rec.log('smooth', in_dtype=np.dtype(in_dtype), out_type=out_type, n=n, slabs=slabs, values=values,
                     weights=weights, qc_weight=None if qc_weight is None else list((C.c_double * 256).from_address(qc_weight)),
                     out=out, count=count, pitches=(in_pitch, weight_pitch, out_pitch), lam=lam, order=order,
                     envelope=envelope, min_valid=min_valid, weight_mode=weight_mode, scale=scale, where=where,
                     stream=stream, stage_bytes=stage_bytes)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(1 << 20)
    monkeypatch.setattr(_lib, 'context', lambda device=0: SmoothCtx(r, device))
    return r


def test_smooth_series_flattens_the_pixels(rec):
    S, shape, n = 3, (2, 3), 6
    codes = np.arange(S * n, dtype=np.uint8).reshape((S,) + shape)
    qc = np.zeros((S,) + shape, np.uint8)
    out, cnt = mod16_amd.smooth_series(codes, qc=qc, qc_weight=GRADED, lam=1600, order=1, envelope=2, min_valid=2,
                                       dtype='float32', scale=0.01, count=True, device=1, stage_bytes=1 << 16)
    assert type(out) is np.ndarray and out.shape == (S,) + shape and out.dtype == np.float32
    assert cnt.shape == shape and cnt.dtype == np.uint16
    (name, seen), = rec.take()[None]
    assert name == 'smooth'
    assert seen['in_dtype'] == np.uint8 and seen['out_type'] == sm.OUT_TYPES['float32'] == _lib.SMOOTH_F32
    assert (seen['n'], seen['slabs'], seen['pitches']) == (n, S, (n, n, n))
    assert (seen['lam'], seen['order'], seen['envelope'], seen['min_valid'], seen['scale']) == (1600.0, 1, 2, 2, 0.01)
    assert seen['weight_mode'] == _lib.SMOOTH_WEIGHT_QC == sm.WEIGHT_QC and seen['qc_weight'] == GRADED.tolist()
    assert seen['out'] == out.ctypes.data and seen['count'] == cnt.ctypes.data
    assert seen['values'] == codes.ctypes.data and seen['weights'] == qc.ctypes.data      # (contiguous: not copied)
    assert (seen['where'], seen['stream'], seen['stage_bytes']) == (_lib.HOST, None, 1 << 16)


def test_smooth_series_modes_defaults_and_out(rec):
    S, n = 4, 5
    vals = np.linspace(0, 1, S * n, dtype=np.float64).reshape(S, n)
    w = np.ones((S, n), np.float32)
    mine = np.empty((S, n), np.float64)
    got = mod16_amd.smooth_series(vals, weights=w, lam=0.5, out=mine)
    assert got is mine
    (name, seen), = rec.take()[None]
    assert seen['in_dtype'] == np.float64 and seen['out_type'] == _lib.SMOOTH_F64 and seen['out'] == mine.ctypes.data
    assert seen['weight_mode'] == _lib.SMOOTH_WEIGHT_STACK and seen['weights'] == w.ctypes.data and seen['qc_weight'] is None
    assert (seen['order'], seen['envelope'], seen['min_valid'], seen['scale'], seen['count']) == (2, 0, 3, 1.0, None)
    assert seen['stage_bytes'] is None
    # no weights; the default QC table is the library's own (no table travels); uint8 in gives uint8 out
    codes = np.zeros((S, n), np.uint8)
    assert mod16_amd.smooth_series(codes, lam=2).dtype == np.uint8
    (name, seen), = rec.take()[None]
    assert seen['weight_mode'] == _lib.SMOOTH_WEIGHT_NONE and seen['weights'] is None and seen['out_type'] == _lib.SMOOTH_U8
    mod16_amd.smooth_series(codes, qc=codes, lam=2)
    (name, seen), = rec.take()[None]
    assert seen['weight_mode'] == _lib.SMOOTH_WEIGHT_QC and seen['qc_weight'] is None
    # a strided input is made contiguous, an empty one makes no call
    mod16_amd.smooth_series(np.zeros((S, 2 * n), np.float32)[:, ::2], lam=2)
    (name, seen), = rec.take()[None]
    assert seen['pitches'] == (n, n, n) and seen['in_dtype'] == np.float32
    mod16_amd.smooth_series(np.zeros((S, 0), np.float32), lam=2)
    assert rec.take() == {}
