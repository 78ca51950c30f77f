"""GPU tests of the per-pixel trend (mod16_trend_f32 / _f64: RasterEngine.trend, mod16_amd.trend_series)
against its numpy definition (mod16_amd/trend.py, itself held to known answers, its properties and
scipy by tests/test_trend_host.py). Every output must have the BITS of the definition: NaN at the same
pixels, everything else equal as uint64 / as integers. The definition is float64 arithmetic of
correctly rounded operations and order statistics, so there is no tolerance.

Y in (2, 3, 5, 6, 7, 17, 23, 24, 32, 33, 45, 46, 64): the pairs Y (Y - 1) / 2 lie on both sides of every
capacity of the ordering network, 16 ... 2048 (1 | 3 | 10 15 | 21 | 136 253 | 276 496 | 528 990 | 1035
2016), so every layout runs, from one lane to 128 lanes per pixel. n in (1, 63, 65, 257, 1000): one
pixel, less and more than a wave, a ragged last block at every capacity (a block holds 2 ... 256
pixels), several blocks. The stack of a Y is made once for 1000 pixels and its definition computed
once; the smaller n are its first pixels (pixels are independent), whose launches differ.

Per pixel, from a seeded generator: its own share of NaN (0 ... 100 %: the valid count runs from 0 to
Y within one launch, on both sides of min_valid), values rounded to multiples of 20 in half of the
pixels (heavy ties), an all-equal pixel, a pixel with both infinities, two pixels of -0.0, 0.0 and +-1."""
import functools

import numpy as np
import pytest

from mod16_amd import trend as tr
import parity

pytestmark = pytest.mark.gpu

STEPS = (2, 3, 5, 6, 7, 17, 23, 24, 32, 33, 45, 46, 64)
SIZES = (1, 63, 65, 257, 1000)
N = max(SIZES)
FIELDS = tr.Trend._fields


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    return torch, mod16_amd


@functools.lru_cache(maxsize=None)
def engine():
    from mod16_amd.raster import RasterEngine
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    return RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250), dtype='float64')


@functools.lru_cache(maxsize=None)
def times(Y, irregular=True):
    if not irregular:
        return None
    t = 2000.0 + np.cumsum(np.random.default_rng(Y).uniform(0.25, 1.75, Y))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def stack(Y, dtype):
    """(Y, N) values, read-only; the recipe of the module docstring."""
    rng = np.random.default_rng(1000 + Y)
    x = rng.normal(500.0, 60.0, (Y, N)) + 2.0 * np.arange(Y)[:, None]
    x[:, 1::2] = np.round(x[:, 1::2] / 20.0) * 20.0
    share = rng.uniform(-0.1, 1.1, N)
    share[:8] = (0.0, 0.2, 0.0, 0.0, 0.0, 0.0, 0.3, 1.0)
    x[rng.uniform(0, 1, (Y, N)) < share] = np.nan
    x[:, 3] = 512.25                                           # all equal
    x[0, 4], x[Y - 1, 4] = np.inf, -np.inf                     # the infinities are missing
    x[:, 5] = rng.choice([-0.0, 0.0], Y)
    x[:, 6] = np.where(np.isnan(x[:, 6]), np.nan, rng.choice([-0.0, 0.0, 1.0, -1.0], Y))
    x = x.astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def definition(Y, dtype):
    """Of the whole stack: irregular times, min_valid 4 (Y below 4: Y), the 95 % interval."""
    want = tr.trend(stack(Y, dtype), times(Y), min(4, Y), 0.05)
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


def first(want, n):
    return tr.Trend(*[None if a is None else a[:n] for a in want])


def host(res):
    return tr.Trend(*[None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for a in res])


def assert_same(got, want, what):
    got = host(got)
    for name, g, w in zip(FIELDS, got, want):
        if w is None:
            assert g is None, '%s: %s was produced' % (what, name)
            continue
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, '%s: %s' % (what, name)
        if w.dtype.kind == 'f':
            assert parity.same_bits(g, w), '%s: %s differs at %d of %d pixels' % (
                what, name, int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum()), w.size)
        else:
            assert np.array_equal(g, w), '%s: %s differs at %d of %d pixels' % (what, name, int((g != w).sum()), w.size)


def on_device(torch, x):
    return torch.from_numpy(np.array(x)).to(engine()._dev())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('Y', STEPS)
def test_every_capacity_and_size_has_the_bits_of_the_definition(env, Y, dtype):
    torch, _ = env
    eng = engine()
    want = definition(Y, dtype)
    assert want.count.min() == 0 and want.count.max() == Y          # the valid count spans 0 ... Y
    x = on_device(torch, stack(Y, dtype))
    for n in SIZES:
        got = eng.trend(x[:, :n], times(Y), min(4, Y), 0.05)         # a view: the stride in time stays N
        eng.check()
        assert_same(got, first(want, n), 'Y = %d, n = %d' % (Y, n))
    assert int(want.count[3]) == Y and want.s[3] == 0 and want.z[3] == 0.0 and want.slope[3] == 0.0
    assert int(want.count[4]) == Y - 2


@pytest.mark.parametrize('alpha', [None, 0.5])
@pytest.mark.parametrize('Y', [5, 24, 46])
def test_default_times_other_levels_and_min_valid(env, Y, alpha):
    torch, _ = env
    eng = engine()
    part = stack(Y, 'float64')[:, :257].copy()
    x = on_device(torch, part)
    for mv in (2, Y):
        want = tr.trend(part, None, mv, alpha)
        got = eng.trend(x, min_valid=mv, alpha=alpha)
        eng.check()
        assert_same(got, want, 'Y = %d, alpha = %r, min_valid = %d' % (Y, alpha, mv))
        assert (got.slope_lo is None) == (alpha is None)


def test_output_subsets_of_the_c_abi(env):
    """S alone; slope and z without the interval; count alone: what is not requested is not written."""
    torch, mod16_amd = env
    from mod16_amd import _lib
    eng = engine()
    Y, n = 24, 257
    want = first(definition(Y, 'float64'), n)
    x = on_device(torch, stack(Y, 'float64')[:, :n].copy())
    t = np.ascontiguousarray(times(Y))
    dev = eng._dev()
    f = {k: torch.full((n,), -7.0, dtype=torch.float64, device=dev) for k in tr.FLOAT_NAMES}
    s = torch.full((n,), -7, dtype=torch.int32, device=dev)
    c = torch.full((n,), 200, dtype=torch.uint8, device=dev)

    def call(floats, s_, c_, zq):
        eng.ctx.trend(np.dtype('float64'), n, Y, x.data_ptr(), t, [f[k].data_ptr() if k in floats else None for k in tr.FLOAT_NAMES],
                      None if s_ is None else s_.data_ptr(), None if c_ is None else c_.data_ptr(), time_stride=n,
                      min_valid=4, zq=zq, where=_lib.DEVICE, stream=eng._stream())
        eng.check()
    call((), s, None, 0.0)
    assert np.array_equal(s.cpu().numpy(), want.s)
    assert all(bool((f[k] == -7.0).all()) for k in f) and bool((c == 200).all())
    call(('slope', 'z'), None, None, 0.0)
    assert parity.same_bits(f['slope'].cpu().numpy(), want.slope) and parity.same_bits(f['z'].cpu().numpy(), want.z)
    assert all(bool((f[k] == -7.0).all()) for k in ('intercept', 'slope_lo', 'slope_hi')) and bool((c == 200).all())
    call((), None, c, 1.5)
    assert np.array_equal(c.cpu().numpy(), want.count)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_strided_stack_at_an_odd_offset_on_another_stream(env, dtype):
    torch, _ = env
    eng = engine()
    Y, n = 33, 65
    want = first(definition(Y, dtype), n)
    buf = torch.full((Y * (n + 3) + 1,), float('nan'), dtype=getattr(torch, dtype), device=eng._dev())
    x = buf[1:].view(Y, n + 3)[:, :n]
    x.copy_(on_device(torch, stack(Y, dtype)[:, :n].copy()))
    outs = {}
    bufs = {}
    for k in FIELDS:
        kind = torch.int32 if k == 's' else torch.uint8 if k == 'count' else torch.float64
        bufs[k] = torch.zeros((n + 1,), dtype=kind, device=eng._dev())
        outs[k] = bufs[k][1:]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = eng.trend(x, times(Y), 4, 0.05, out=outs)
    side.synchronize()
    eng.check()
    assert all(got[i] is outs[k] for i, k in enumerate(FIELDS))
    assert_same(got, want, 'strided, %s' % dtype)
    assert all(float(b[0]) == 0 for b in bufs.values())
    on_input = buf[:n * (8 // buf.element_size())].view(torch.float64)           # n float64 on the first rows of x
    with pytest.raises(ValueError, match='overlaps'):
        eng.trend(x, times(Y), 4, 0.05, out=dict(outs, slope=on_input))


@pytest.mark.parametrize('dtype,Y', [('float32', 46), ('float64', 7)])
def test_host_mode_any_stage_bytes_and_both_entry_points_agree(env, dtype, Y):
    torch, mod16_amd = env
    want = definition(Y, dtype)
    x = stack(Y, dtype)
    fixed, per_pixel = 7 * 33 * 1024 + 512, (6 + Y) * 8 + 1
    for stage in (1, fixed + 600 * per_pixel, None):          # ranges of 256 pixels, of 512, one range
        got = mod16_amd.trend_series(x, times(Y), min(4, Y), 0.05, stage_bytes=stage)
        assert_same(got, want, 'HOST mode, stage_bytes = %r' % stage)
    cube = mod16_amd.trend_series(x.reshape(Y, 8, 125), times(Y), min(4, Y), 0.05)      # (Y, P, n): P n pixels
    assert cube.slope.shape == (8, 125)
    assert_same(tr.Trend(*[a.reshape(-1) for a in cube]), want, 'a (Y, 8, 125) stack')
    dev = engine().trend(on_device(torch, x), times(Y), min(4, Y), 0.05)
    engine().check()
    assert_same(dev, want, 'RasterEngine.trend')


def test_two_calls_give_the_same_bits(env):
    torch, _ = env
    eng = engine()
    x = on_device(torch, stack(64, 'float32'))
    a = host(eng.trend(x, times(64), 4, 0.05))
    b = host(eng.trend(x, times(64), 4, 0.05))
    eng.check()
    for name, p, q in zip(FIELDS, a, b):
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), name


def test_annual_composites_feed_the_trend_on_the_device(env):
    """Four annual totals of RasterEngine.composite over a 2 x 50 raster, written into the rows of one
    stack and fed straight into RasterEngine.trend: the definition on the downloaded composites."""
    torch, _ = env
    from oracle import synth
    eng = engine()
    years, days, n = 4, 16, 2 * 50
    dev = eng._dev()
    totals = torch.empty((years, n), dtype=torch.float64, device=dev)
    valid = torch.empty((years, n), dtype=torch.uint16, device=dev)
    for y in range(years):
        cls, drivers = synth.drivers((days, n), seed=300 + y, special=False)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        c = torch.from_numpy(np.ascontiguousarray(synth.drivers((1, n), seed=300, special=False)[0][0])).to(dev)
        hours = put(np.random.default_rng(y).uniform(6, 18, (days, n)))
        eng.composite(c, [put(d) for d in drivers], hours, days, period_days=days, out=[totals[y:y + 1], valid[y:y + 1]])
    got = eng.trend(totals, times=[2001.0, 2002.0, 2003.0, 2004.0], min_valid=3, alpha=0.05)
    eng.check()
    stacked = totals.cpu().numpy()
    assert np.isfinite(stacked).sum() > 3 * n
    assert_same(got, tr.trend(stacked, [2001.0, 2002.0, 2003.0, 2004.0], 3, 0.05), 'composites')
