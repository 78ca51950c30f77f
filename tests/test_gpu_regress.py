"""GPU tests of the per-pixel least squares (mod16_regress_f32 / _f64: RasterEngine.regress,
mod16_amd.regress_series) against its numpy definition (mod16_amd/regress.py, itself held to a scalar
loop and to numpy.linalg.lstsq by tests/test_regress_host.py). Every output must be EQUAL to the
definition -- the counts value for value, the floats bit for bit (NaN is any NaN): the kernel performs
the definition's float64 operations in its order, so there is no tolerance.

Shapes: n in 1, 63, 64, 65, 257, 1237 (a lane short of a wave, a wave, one over, a block and a lane, five
blocks the last with 213 lanes) and T in 1, P - 1, P, P + 1, 3, 46 and 130, for P in 1, 2, 5, 8 split into
(P, 0), (0, P) and (1, P - 1) shared and per-pixel terms. The kernel reads the design through uniform
loads step by step: it has no staging chunk to straddle. Weights, the share of missing values, stderr
and the series mode cycle over the shapes so that every value of each meets every P; four edge pixels
(all missing; count = min_valid - 1; count = min_valid; a term that is exactly constant next to the
intercept, where the split has both) are planted at lanes 0, 63, 64 and n - 1, rotating with the shape.
The other edge pixels of tests/test_regress_host.py have tests of their own, each kind at all four lanes:
an uncentred year column next to the intercept (kept), count == P with min_valid = P (T = 1 with P = 1
among the shapes) and weights of 0, -1, NaN and inf."""
import functools

import numpy as np
import pytest

from mod16_amd import regress as R

pytestmark = pytest.mark.gpu

SPLITS = sorted({(P, ks, P - ks) for P in (1, 2, 5, 8) for ks in (P, 0, 1)})
SIZES = (1, 63, 64, 65, 257, 1237)
SERIES = (None, 'residuals', 'fitted')


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    return torch, mod16_amd, _lib


@functools.lru_cache(maxsize=None)
def engine():
    from mod16_amd.raster import RasterEngine
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    return RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250), dtype='float64')


def make_inputs(n, T, Ks, Kp, dtype, weighted, missing, seed, rotate=0):
    """-> (values, design or None, terms, weights or None, min_valid), with the planted edge pixels."""
    rng = np.random.default_rng(seed)
    P = Ks + Kp
    min_valid = P + 1
    design = None
    if Ks:
        t = np.arange(T, dtype=np.float64)
        design = np.stack([np.ones(T)] + [np.cos(0.37 * k * t + k) + 0.05 * rng.standard_normal(T) for k in range(1, Ks)], axis=1)
    terms = [(rng.standard_normal((T, n)) + 0.5 * k).astype(dtype) for k in range(Kp)]
    values = (3.0 * rng.standard_normal((T, n)) + 10.0).astype(dtype)
    values[rng.random((T, n)) < missing] = np.nan
    values[rng.random((T, n)) < 0.01] = np.inf
    for t in terms:
        t[rng.random((T, n)) < missing / 6] = np.nan
    weights = None
    if weighted:
        weights = rng.choice(np.array([0, 0.5, 1, 0.25, 2.5, np.nan, -1, np.inf], np.float32), (T, n),
                             p=[.08, .25, .3, .15, .1, .05, .05, .02])
    lanes = [p for p in dict.fromkeys((0, 63, 64, n - 1)) if p < n]
    for k, p in enumerate(lanes):
        kind = (k + rotate) % 4
        col = (2.0 + np.sin(np.arange(T) * 0.9) + 0.1 * rng.standard_normal(T)).astype(dtype)
        for t in terms:
            t[:, p] = rng.standard_normal(T).astype(dtype)
        if weights is not None:
            weights[:, p] = 1.0
        if kind == 0:
            col[:] = np.nan
        elif kind == 1:
            col[max(min_valid - 1, 0):] = np.nan
        elif kind == 2:
            col[min_valid:] = np.nan
        elif Ks and Kp:
            terms[0][:, p] = dtype(3.7)              # exactly constant next to the intercept: degenerate
        else:
            col[::2] = np.inf
        values[:, p] = col
    return values, design, terms, weights, min_valid


def bits_equal(g, w):
    g, w = np.asarray(g), np.asarray(w)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype.kind != 'f':
        return np.array_equal(g, w)
    nan = np.isnan(g)
    return np.array_equal(nan, np.isnan(w)) and g[~nan].tobytes() == w[~nan].tobytes()


def assert_equal(got, want, what):
    for name, g, w in zip(R.Regression._fields, got, want):
        if w is None:
            assert g is None, '%s: %s was not asked for' % (what, name)
            continue
        if not bits_equal(g, w):
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape and g.dtype == w.dtype, '%s: %s is %s %r, want %s %r' % (what, name, g.dtype, g.shape, w.dtype, w.shape)
            both = ~(np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64)))
            bad = np.argwhere((g != w) & both)
            raise AssertionError('%s: %s differs in %d elements, first at %r: %r, want %r'
                                 % (what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def to_host(torch, t):
    if t is None:
        return None
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def run_device(torch, values, design, terms, weights, **kw):
    eng = engine()
    res = eng.regress(values if isinstance(values, torch.Tensor) else dev(torch, values), design,
                      [t if isinstance(t, torch.Tensor) else dev(torch, t) for t in terms],
                      None if weights is None else weights if isinstance(weights, torch.Tensor) else dev(torch, weights), **kw)
    eng.check()
    return R.Regression(*[to_host(torch, t) for t in res])


@pytest.mark.parametrize('P,Ks,Kp', SPLITS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_equals_the_definition(env, dtype, P, Ks, Kp):
    torch = env[0]
    steps = sorted({T for T in (1, P - 1, P, P + 1, 3, 46) if T >= 1})
    shapes = [(n, T) for n in SIZES for T in steps] + [(257, 130)]
    seen = set()
    for k, (n, T) in enumerate(shapes):
        k += P + Ks                                  # (the cycles start elsewhere for every split)
        weighted, missing = bool(k % 2), (0.1, 0.6)[(k // 2) % 2]
        series, stderr = SERIES[(k // 4) % 3], bool((k // 12) % 2)
        seen.add((weighted, missing, stderr, series))
        values, design, terms, weights, min_valid = make_inputs(n, T, Ks, Kp, dtype, weighted, missing, 1000 * P + 10 * Ks + k, k)
        want = R.regress(values, design, terms, weights, stderr=stderr, series=series)
        got = run_device(torch, values, design, terms, weights, stderr=stderr, series=series)
        assert_equal(got, want, 'n = %d, T = %d, weights %r, missing %.1f, stderr %r, series %r' % (n, T, weighted, missing, stderr, series))
        if T == 46 and n == 1237 and missing < 0.5:
            fitted = np.isfinite(want.coef).all(axis=0)
            assert fitted.sum() > n // 2 and not fitted.all()
    assert len(seen) == 24                           # every combination of the four switches was met


@pytest.mark.parametrize('P,Ks,Kp', [(2, 2, 0), (5, 1, 4), (8, 0, 8)])
def test_min_valid_equal_to_the_terms(env, P, Ks, Kp):
    """count == P with min_valid = P: the exact fit, and a stderr that is what IEEE gives for rss / 0."""
    torch = env[0]
    values, design, terms, weights, _ = make_inputs(257, P + 3, Ks, Kp, np.float64, True, 0.3, 77, 0)
    values[:P, 5] = np.arange(1.0, P + 1.0) ** 2
    values[P:, 5] = np.nan
    rng = np.random.default_rng(5)
    for t in terms:
        t[:, 5] = rng.standard_normal(P + 3)
    weights[:, 5] = 1.0
    want = R.regress(values, design, terms, weights, min_valid=P, stderr=True, series='residuals')
    got = run_device(torch, values, design, terms, weights, min_valid=P, stderr=True, series='residuals')
    assert_equal(got, want, 'min_valid = P = %d' % P)
    assert want.count[5] == P and np.isfinite(want.coef[:, 5]).all() and not np.isfinite(want.stderr[:, 5]).any()


EDGE_LANES = (0, 63, 64)          # and n - 1


def plant_edges(kind, n, T, P, Ks, Kp, dtype, seed):
    """A stack whose pixels at lanes 0, 63, 64 and n - 1 all are the edge pixel `kind` of
    tests/test_regress_host.py; the other pixels are ordinary. -> (values, design, terms, weights, the lanes)."""
    values, design, terms, weights, _ = make_inputs(n, T, Ks, Kp, dtype, True, 0.2, seed, 0)
    rng = np.random.default_rng(seed + 1)
    lanes = [p for p in dict.fromkeys(EDGE_LANES + (n - 1,)) if p < n]
    step = np.arange(T)
    for p in lanes:
        values[:, p] = (2.0 + 0.3 * step + np.sin(0.9 * step) + 0.1 * rng.standard_normal(T)).astype(dtype)
        for t in terms:
            t[:, p] = rng.standard_normal(T).astype(dtype)
        weights[:, p] = 1.0
        if kind == 'years':                   # an uncentred year column next to the intercept: kept, not degenerate
            terms[0][:, p] = (2000.0 + step).astype(dtype)
        elif kind == 'exact':                 # count == P
            values[P:, p] = np.nan
        elif kind == 'weights':               # 0, negative, NaN and inf weights: those samples are left out
            weights[:, p] = np.resize(np.array([1, 0, 0.5, -1, 2, np.nan, 1, np.inf], np.float32), T)
    return values, design, terms, weights, lanes


@pytest.mark.parametrize('n', [65, 257, 1237])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_year_column_next_to_an_intercept_is_kept(env, dtype, n):
    """The host test's ill-conditioned pixel on the device: a per-pixel term 2000 + i next to the intercept has
    a pivot ratio of about 1e-5, far above 2^-40: finite, and the definition's bits."""
    torch = env[0]
    values, design, terms, weights, lanes = plant_edges('years', n, 24, 2, 1, 1, dtype, 41)
    want = R.regress(values, design, terms, weights, stderr=True, series='fitted')
    got = run_device(torch, values, design, terms, weights, stderr=True, series='fitted')
    assert_equal(got, want, 'year column, n = %d' % n)
    assert list(want.count[lanes]) == [24] * len(lanes)
    assert np.isfinite(got.coef[:, lanes]).all() and np.isfinite(got.stderr[:, lanes]).all() and np.isfinite(got.r2[lanes]).all()
    assert np.allclose(got.coef[1, lanes], 0.3, atol=0.1)


@pytest.mark.parametrize('T,P,Ks,Kp', [(1, 1, 1, 0), (1, 1, 0, 1), (2, 2, 1, 1), (9, 5, 1, 4), (11, 8, 8, 0), (8, 8, 0, 8)])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_count_equal_to_the_terms_at_the_wave_edges(env, dtype, T, P, Ks, Kp):
    """count == P with min_valid = P at lanes 0, 63, 64 and n - 1, T = 1 with P = 1 among the shapes: the exact
    fit, and for stderr what IEEE gives for rss / 0."""
    torch = env[0]
    for n in (65, 1237):
        values, design, terms, weights, lanes = plant_edges('exact', n, T, P, Ks, Kp, dtype, 43 + T)
        want = R.regress(values, design, terms, weights, min_valid=P, stderr=True, series='residuals')
        got = run_device(torch, values, design, terms, weights, min_valid=P, stderr=True, series='residuals')
        assert_equal(got, want, 'count == P = %d, T = %d, n = %d' % (P, T, n))
        assert list(want.count[lanes]) == [P] * len(lanes)
        assert np.isfinite(got.coef[:, lanes]).all() and not np.isfinite(got.stderr[:, lanes]).any()
    if T == 1 and Ks == 1:
        assert np.array_equal(got.coef[0, lanes], values[0, lanes].astype(np.float64))       # design 1.0: b = y


@pytest.mark.parametrize('P,Ks,Kp', [(2, 2, 0), (5, 1, 4), (8, 0, 8)])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_bad_weights_at_the_wave_edges(env, dtype, P, Ks, Kp):
    """Weights of 0, -1, NaN and inf at lanes 0, 63, 64 and n - 1: those samples do not count."""
    torch = env[0]
    T = 32
    for n in (65, 1237):
        values, design, terms, weights, lanes = plant_edges('weights', n, T, P, Ks, Kp, dtype, 47)
        want = R.regress(values, design, terms, weights, stderr=True, series='residuals')
        got = run_device(torch, values, design, terms, weights, stderr=True, series='residuals')
        assert_equal(got, want, 'bad weights, n = %d' % n)
        assert list(got.count[lanes]) == [16] * len(lanes)
        bad = ~(np.isfinite(weights[:, lanes[0]]) & (weights[:, lanes[0]] > 0))
        assert bad.sum() == 16 and np.isnan(got.series[bad][:, lanes]).all() and np.isfinite(got.series[~bad][:, lanes]).all()
        assert np.isfinite(got.coef[:, lanes]).all()


def test_no_pixels(env):
    torch = env[0]
    res = engine().regress(torch.empty((9, 0), dtype=torch.float32, device='cuda'), np.ones((9, 2)), stderr=True, series='fitted')
    assert tuple(res.coef.shape) == (2, 0) and tuple(res.series.shape) == (9, 0) and res.series.dtype == torch.float32
    assert tuple(res.count.shape) == (0,) and res.count.dtype == torch.uint16


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('offset', [1, 3])
def test_views_at_odd_offsets_and_pitches(env, dtype, offset):
    """Every tensor a view that starts 1 or 3 elements into a larger buffer, each stack with a pitch of its
    own; the padding of the outputs is pre-filled and unchanged afterwards."""
    torch = env[0]
    n, T, Ks, Kp = 321, 11, 2, 2
    P = Ks + Kp
    values, design, terms, weights, _ = make_inputs(n, T, Ks, Kp, np.dtype(dtype).type, True, 0.2, 31, 1)

    def view(dt, rows, pitch):
        elem = torch.empty((), dtype=dt).element_size()
        buf = torch.full(((rows * pitch + 8) * elem,), 0xA5, dtype=torch.uint8, device='cuda').view(dt)
        return buf, buf[offset:offset + rows * pitch].view(rows, pitch)[:, :n]

    def filled(src, dt, pitch):
        v = view(dt, src.shape[0], pitch)[1]
        v.copy_(dev(torch, src))
        return v
    tdt = getattr(torch, dtype)
    vv = filled(values, tdt, n + 5)
    tv = [filled(t, tdt, n + 9) for t in terms]
    wv = filled(weights, torch.float32, n + 2)
    outs, bufs = {}, {}
    for name, (dt, rows, pitch) in dict(coef=(torch.float64, P, n + 3), stderr=(torch.float64, P, n + 7),
                                        series=(tdt, T, n + 4)).items():
        bufs[name], outs[name] = view(dt, rows, pitch)
        bufs[name] = (bufs[name], rows, pitch)
    for name, dt in dict(rss=torch.float64, tss=torch.float64, r2=torch.float64, count=torch.uint16).items():
        elem = torch.empty((), dtype=dt).element_size()
        buf = torch.full(((n + 8) * elem,), 0xA5, dtype=torch.uint8, device='cuda').view(dt)
        bufs[name], outs[name] = (buf, 1, n), buf[offset:offset + n]
    want = R.regress(values, design, terms, weights, stderr=True, series='residuals')
    got = run_device(torch, vv, design, tv, wv, stderr=True, series='residuals', out=outs)
    assert_equal(got, want, 'views at offset %d' % offset)
    for name, (buf, rows, pitch) in bufs.items():
        raw = buf.view(torch.uint8).cpu().numpy()
        e = buf.element_size()
        mask = np.ones(raw.size, bool)
        for r in range(rows):
            lo = (offset + r * pitch) * e
            mask[lo:lo + n * e] = False
        assert (raw[mask] == 0xA5).all(), name


@pytest.mark.parametrize('dtype,Ks,Kp', [(np.float32, 2, 0), (np.float64, 1, 3), (np.float32, 0, 2)])
def test_host_mode_equals_device_mode_across_tiles(env, dtype, Ks, Kp):
    """numpy in / numpy out through the staged tiles: a stage_bytes that cuts 1237 pixels into tiles of 256
    (four and a short fifth), one that gives 512 (two and a short third), and the default (one tile)."""
    torch, mod16_amd = env[0], env[1]
    n, T = 1237, 7
    P = Ks + Kp
    values, design, terms, weights, _ = make_inputs(n, T, Ks, Kp, dtype, True, 0.3, 91, 2)
    for stderr, series, w in ((True, 'fitted', weights), (False, None, None), (True, 'residuals', weights)):
        want = R.regress(values, design, terms, w, stderr=stderr, series=series)
        device = run_device(torch, values, design, terms, w, stderr=stderr, series=series)
        assert_equal(device, want, 'DEVICE')
        nwide = 9 + Kp
        wide_rows = P + (P if stderr else 1) + 4 + (T if series else 1) + T * (1 + Kp) + (T if w is not None else 1)
        fixed, per_pixel = nwide * 33 * 1024 + 512, wide_rows * 8
        for pixels in (300, 600, None):
            stage = None if pixels is None else fixed + pixels * per_pixel
            got = mod16_amd.regress_series(values, design, terms, w, stderr=stderr, series=series, stage_bytes=stage)
            assert_equal(got, device, 'HOST, stage for %r pixels' % pixels)


def test_regress_series_on_a_pixel_shape_and_out(env):
    mod16_amd = env[1]
    T, shape = 12, (7, 13)
    values, design, terms, weights, _ = make_inputs(91, T, 2, 1, np.float32, True, 0.2, 3, 3)
    full = (T,) + shape
    want = R.regress(values, design, terms, weights, stderr=True, series='fitted')
    out = {k: np.empty(s, dt) for k, (s, dt) in R.output_table(shape, T, 3, np.float32, True, 2).items()}
    got = mod16_amd.regress_series(values.reshape(full), design, [terms[0].reshape(full)], weights.reshape(full), stderr=True,
                                   series='fitted', out=out)
    assert got.coef is out['coef'] and got.series is out['series'] and got.coef.shape == (3,) + shape
    assert_equal(R.Regression(*[None if g is None else g.reshape(w.shape) for g, w in zip(got, want)]), want, 'pixel shape')
    with pytest.raises(ValueError, match='out must hold exactly'):
        mod16_amd.regress_series(values, design, terms, weights, out={'coef': out['coef']})
    with pytest.raises(ValueError, match='weights must be float32'):
        mod16_amd.regress_series(values, design, terms, weights.astype(np.float64))
    with pytest.raises(ValueError, match='design must be finite'):
        mod16_amd.regress_series(values, np.full((T, 2), np.nan), terms)


def test_design_as_an_array_and_as_a_tensor(env):
    torch = env[0]
    values, design, terms, weights, _ = make_inputs(513, 46, 5, 1, np.float32, False, 0.4, 17, 0)
    want = R.regress(values, design, terms, stderr=True, series='fitted')
    from_array = run_device(torch, values, design, terms, None, stderr=True, series='fitted')
    from_tensor = run_device(torch, values, dev(torch, design), terms, None, stderr=True, series='fitted')
    assert_equal(from_array, want, 'design as an array')
    assert_equal(from_tensor, from_array, 'design as a tensor')


def test_tensor_refusals(env):
    torch = env[0]
    eng = engine()
    n, T = 300, 9
    values, design, terms, weights, _ = make_inputs(n, T, 2, 1, np.float32, True, 0.2, 5, 0)
    v, t0, w = dev(torch, values), dev(torch, terms[0]), dev(torch, weights)
    with pytest.raises(TypeError, match='values must be a float32 or float64 tensor'):
        eng.regress(v.to(torch.int32), design)
    with pytest.raises(TypeError, match='values must be'):
        eng.regress(v.cpu(), design)                                          # the wrong device
    with pytest.raises(TypeError, match=r'terms\[0\] must be a float32 tensor'):
        eng.regress(v, design, [t0.double()])
    with pytest.raises(TypeError, match=r'terms\[0\] must be'):
        eng.regress(v, design, [t0.cpu()])
    with pytest.raises(TypeError, match='weights must be a float32 tensor'):
        eng.regress(v, design, [t0], w.double())
    with pytest.raises(TypeError, match='design must be a float64 tensor'):
        eng.regress(v, dev(torch, design).float())
    with pytest.raises(TypeError, match=r"out\['coef'\] must be a float64 tensor"):
        eng.regress(v, design, out=dict(coef=torch.empty((2, n), dtype=torch.float32, device='cuda'),
                                        **{k: torch.empty((n,), dtype=torch.float64, device='cuda') for k in ('rss', 'tss', 'r2')},
                                        count=torch.empty((n,), dtype=torch.uint16, device='cuda')))
    with pytest.raises(ValueError, match='out must hold exactly'):
        eng.regress(v, design, out=dict(coef=torch.empty((2, n), dtype=torch.float64, device='cuda')))
    with pytest.raises(ValueError, match='unit stride in pixels'):
        eng.regress(dev(torch, np.ascontiguousarray(values.T)).t(), design)
    with pytest.raises(ValueError, match='unit stride in pixels'):
        eng.regress(v, design, [dev(torch, np.ascontiguousarray(terms[0].T)).t()])
    with pytest.raises(ValueError, match='stride in time must be at least'):
        eng.regress(v[0].expand(T, n), design)
    with pytest.raises(ValueError, match='design must be contiguous'):
        eng.regress(v, dev(torch, np.ascontiguousarray(design.T)).t())
    with pytest.raises(ValueError, match=r'values must be a \(T, n\) tensor'):
        eng.regress(v.view(T, 3, n // 3), design)
    with pytest.raises(ValueError, match='the terms must share one stride in time'):
        big = torch.zeros((T, n + 4), dtype=torch.float32, device='cuda')
        eng.regress(v, None, [t0, big[:, :n]])
    with pytest.raises(ValueError, match='between 1 and 8 terms'):
        eng.regress(v)
    with pytest.raises(ValueError, match='min_valid'):
        eng.regress(v, design, min_valid=1)

    def outs(**given):
        table = R.output_table((n,), T, 2, np.float32, False, 1)
        made = {k: torch.empty(s, dtype=getattr(torch, dt.name), device='cuda') for k, (s, dt) in table.items()}
        made.update(given)
        return made
    with pytest.raises(ValueError, match='overlaps'):
        eng.regress(v, design, series='residuals', out=outs(series=v))          # in place
    with pytest.raises(ValueError, match='overlaps'):
        eng.regress(v, design, weights=w, series='residuals', out=outs(series=w))
    stack = torch.zeros(T * n + n, dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):                          # one row of overlap
        eng.regress(stack[:T * n].view(T, n), design, series='fitted', out=outs(series=stack[n:].view(T, n)))
    pair = torch.empty((2, n), dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):                          # an output on another output
        eng.regress(v, design, series='residuals', out=outs(coef=pair, rss=pair[1]))
    eng.check()
