"""GPU tests of the per-pixel climatology, standardized anomaly and percentile rank (mod16_anomaly_f32 /
_f64: RasterEngine.anomaly, mod16_amd.anomaly_series) against the numpy definition (mod16_amd/anomaly.py,
itself held to known answers, numpy's reductions and its bit-level properties by
tests/test_anomaly_host.py). Every output must have the BITS of the definition: NaN at the same places,
everything else equal as integers. The definition is float64 arithmetic of correctly rounded
operations in a fixed order and integer counts, so there is no tolerance.

Y in (2, 3, 16, 17, 24, 32, 33, 64): whole and ragged batches of the eight years the kernel loads
together, the fewest years, and the most (the largest LDS column a block can have, 64 KiB; 33 years is
the first size at which a compute unit holds fewer than five blocks). P in (1, 5), one case of Y = 2
with P = 366 and one of Y = 24 with P = 46; windows 1, 2, 4 and min(P, 16) where P allows (they run
across the year boundary, and the first W - 1 slabs of the record are missing); the baseline leaves a
year out at both ends where Y >= 4. Up to 300 pixels every block has one period; 2100 and 12000 pixels
make a block walk several.
n in (1, 63, 65, 257, 300): one pixel, both sides of a wave, a ragged last block, several blocks. The
record of a (Y, P) is made once for 300 pixels and its definition computed once per window; the
smaller n are its first pixels (pixels are independent), whose launches differ.

Per pixel, from a seeded generator: num is gamma(4, 5), den is num + gamma(4, 8), both rounded to
integers in every second pixel (heavy ties); its own share of NaN (0 ... 100 %: the valid count runs
from 0 to the baseline length within one launch, on both sides of min_valid); a constant pixel; a pixel
with den = 0, den < 0, num = inf and den = inf; a pixel of -0.0 and +0.0."""
import functools

import numpy as np
import pytest

from mod16_amd import anomaly as an
import parity

pytestmark = pytest.mark.gpu

YEARS = (2, 3, 16, 17, 24, 32, 33, 64)
SHAPES = [(Y, P) for Y in YEARS for P in (1, 5)] + [(2, 366), (24, 46)]
SIZES = (1, 63, 65, 257, 300)
N = max(SIZES)
ALL = an.OUTPUT_NAMES


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


def windows(P):
    return tuple(sorted({w for w in (1, 2, 4, min(P, 16)) if w <= P}))


def baseline(Y):
    return (1, Y - 1) if Y >= 4 else None


def min_valid(Y):
    return 3 if Y >= 5 else 2


@functools.lru_cache(maxsize=None)
def record(Y, P, dtype):
    """(num, den), each (Y P, N), read-only; the recipe of the module docstring."""
    rng = np.random.default_rng(1000 * Y + P)
    S = Y * P
    num = rng.gamma(4.0, 5.0, (S, N))
    den = num + rng.gamma(4.0, 8.0, (S, N))
    num[:, 1::2] = np.round(num[:, 1::2])
    den[:, 1::2] = np.round(den[:, 1::2]) + 1.0
    share = rng.uniform(-0.1, 1.1, N)
    share[:8] = (0.0, 0.2, 0.0, 0.0, 0.0, 0.0, 0.3, 1.0)
    num[rng.uniform(0, 1, (S, N)) < share] = np.nan
    num[:, 3], den[:, 3] = 7.25, 29.0                          # constant
    den[0, 4], den[S - 1, 4] = 0.0, -3.0                       # every kind of missing value in one pixel
    if S >= 4:
        num[1, 4], den[2, 4] = np.inf, np.inf
    num[:, 5] = rng.choice([-0.0, 0.0], S)
    num, den = num.astype(dtype), den.astype(dtype)
    num.setflags(write=False)
    den.setflags(write=False)
    return num, den


@functools.lru_cache(maxsize=None)
def definition(Y, P, W, dtype, ratio=True):
    num, den = record(Y, P, dtype)
    want = an.anomaly(num, den if ratio else None, periods=P, window=W, baseline=baseline(Y), min_valid=min_valid(Y), outputs=ALL)
    for a in want:
        a.setflags(write=False)
    return want


def first(want, n):
    return an.Anomaly(*[None if a is None else a[:, :n] for a in want])


def host(res):
    return an.Anomaly(*[None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for a in res])


def assert_same(got, want, what):
    got = host(got)
    for name, g, w in zip(ALL, got, want):
        if w is None:
            assert g is None, '%s: %s was produced' % (what, name)
            continue
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, '%s: %s' % (what, name)
        if w.dtype.kind == 'f':
            assert parity.same_bits(g, w), '%s: %s differs at %d of %d places' % (
                what, name, int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum()), w.size)
        else:
            assert np.array_equal(g, w), '%s: %s differs at %d of %d places' % (what, name, int((g != w).sum()), w.size)


def on_device(torch, x):
    return torch.from_numpy(np.array(x)).to(engine()._dev())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('Y,P', SHAPES)
def test_every_capacity_window_and_size_has_the_bits_of_the_definition(env, Y, P, dtype):
    torch, _ = env
    eng = engine()
    num, den = (on_device(torch, a) for a in record(Y, P, dtype))
    y0, y1 = baseline(Y) or (0, Y)
    for W in windows(P):
        want = definition(Y, P, W, dtype)
        if W == 1:
            assert want.count.min() == 0 and want.count.max() == y1 - y0     # the valid count spans 0 ... the baseline
            assert (want.count[:, 3] == y1 - y0).all() and (want.std[:, 3] == 0).all() and np.isnan(want.z[:, 3]).all()
            assert (want.pct[:, 3] == 0.5).all()
        for n in SIZES:
            got = eng.anomaly(num[:, :n], den[:, :n], periods=P, window=W, baseline=baseline(Y), min_valid=min_valid(Y),
                              outputs=ALL)                          # views: the stride in time stays N
            eng.check()
            assert_same(got, first(want, n), 'Y = %d, P = %d, W = %d, n = %d' % (Y, P, W, n))
    if Y * P >= 64:
        share = np.isfinite(definition(Y, P, 1, dtype).z).mean()
        assert 0.3 < share < 0.7, share                             # about half the z are finite


@pytest.mark.parametrize('Y,P,copies,W', [(2, 366, 7, 4), (2, 366, 40, 16), (24, 46, 40, 4)])
def test_a_block_walks_several_periods_once_the_pixels_fill_the_device(env, Y, P, copies, W):
    """The launch cuts P into one period per block until 4096 blocks exist; 2100 and 12000 pixels of
    P = 366 make a block walk 2 and 9 periods in turn, 12000 pixels of P = 46 two, its column and moments
    started anew for each. The record is the 300-pixel one side by side `copies` times (pixels are
    independent)."""
    torch, _ = env
    eng = engine()
    dtype = 'float32'
    once = definition(Y, P, W, dtype)
    num, den = (on_device(torch, np.tile(a, (1, copies))) for a in record(Y, P, dtype))
    got = eng.anomaly(num, den, periods=P, window=W, baseline=baseline(Y), min_valid=min_valid(Y), outputs=ALL)
    eng.check()
    assert_same(got, an.Anomaly(*[np.tile(a, (1, copies)) for a in once]), '%d pixels, W = %d' % (copies * N, W))


@pytest.mark.parametrize('Y,P,W', [(3, 5, 2), (24, 5, 1), (33, 5, 4), (64, 1, 1)])
def test_without_den_the_quantity_is_the_window_sum(env, Y, P, W):
    torch, _ = env
    eng = engine()
    for dtype in ('float32', 'float64'):
        want = definition(Y, P, W, dtype, ratio=False)
        num = on_device(torch, record(Y, P, dtype)[0])
        got = eng.anomaly(num, periods=P, window=W, baseline=baseline(Y), min_valid=min_valid(Y), outputs=ALL)
        eng.check()
        assert_same(got, want, 'no den, Y = %d, P = %d, W = %d, %s' % (Y, P, W, dtype))


def test_defaults_and_min_valid_up_to_the_baseline_length(env):
    torch, _ = env
    eng = engine()
    Y, P = 17, 5
    part = [a[:, :257].copy() for a in record(Y, P, 'float64')]
    num, den = (on_device(torch, a) for a in part)
    got = eng.anomaly(num, den, periods=P)
    eng.check()
    assert got.pct is None and got.mean is None and got.std is None and got.count is None
    assert_same(got, an.anomaly(part[0], part[1], periods=P, outputs=('z',)), 'defaults')
    for mv in (2, Y):
        got = eng.anomaly(num, den, periods=P, window=3, min_valid=mv, outputs=('pct', 'z', 'count'))
        eng.check()
        assert_same(got, an.anomaly(part[0], part[1], periods=P, window=3, min_valid=mv, outputs=('z', 'pct', 'count')),
                    'min_valid = %d' % mv)


def test_output_subsets_of_the_c_abi(env):
    """z alone; pct and count; mean and std: what is not requested keeps its sentinel."""
    torch, mod16_amd = env
    from mod16_amd import _lib
    eng = engine()
    Y, P, W, n = 24, 5, 2, 257
    want = first(definition(Y, P, W, 'float64'), n)
    num, den = (on_device(torch, a[:, :n].copy()) for a in record(Y, P, 'float64'))
    dev = eng._dev()
    buf = dict(z=torch.full((Y * P, n), -7.0, dtype=torch.float64, device=dev),
               pct=torch.full((Y * P, n), -7.0, dtype=torch.float64, device=dev),
               mean=torch.full((P, n), -7.0, dtype=torch.float64, device=dev),
               std=torch.full((P, n), -7.0, dtype=torch.float64, device=dev),
               count=torch.full((P, n), 200, dtype=torch.uint8, device=dev))
    sentinel = dict(z=-7.0, pct=-7.0, mean=-7.0, std=-7.0, count=200)
    y0, y1 = baseline(Y)

    def call(names):
        eng.ctx.anomaly(np.dtype('float64'), n, Y, P, num.data_ptr(), den.data_ptr(),
                        *[buf[k].data_ptr() if k in names else None for k in ALL], window=W, base_first=y0, base_end=y1,
                        min_valid=min_valid(Y), where=_lib.DEVICE, stream=eng._stream())
        eng.check()

    done = set()
    for names in (('z',), ('pct', 'count'), ('mean', 'std')):
        call(names)
        done |= set(names)
        for k in ALL:
            if k in done:
                got = buf[k].cpu().numpy()
                ok = parity.same_bits(got, getattr(want, k)) if k != 'count' else np.array_equal(got, want.count)
                assert ok, (names, k)
            else:
                assert bool((buf[k] == sentinel[k]).all()), (names, k)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_strided_arrays_at_an_odd_offset_on_another_stream(env, dtype):
    torch, _ = env
    eng = engine()
    Y, P, W, n = 33, 5, 4, 65
    S = Y * P
    want = first(definition(Y, P, W, dtype), n)
    tdtype = getattr(torch, dtype)
    dev = eng._dev()

    def strided(rows, kind, fill, pad=3):
        """(buffer, its (rows, n) view one element in, rows n + pad apart)"""
        b = torch.full((rows * (n + pad) + 1,), fill, dtype=kind, device=dev)
        return b, b[1:].view(rows, n + pad)[:, :n]

    nbuf, num = strided(S, tdtype, float('nan'))
    dbuf, den = strided(S, tdtype, float('nan'))
    for view, a in zip((num, den), record(Y, P, dtype)):
        view.copy_(on_device(torch, a[:, :n].copy()))
    kinds = dict(z=(S, tdtype), pct=(S, tdtype), mean=(P, torch.float64), std=(P, torch.float64), count=(P, torch.uint8))
    bufs, outs = {}, {}
    for k, (rows, kind) in kinds.items():
        bufs[k], outs[k] = strided(rows, kind, 0, pad=5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = eng.anomaly(num, den, periods=P, window=W, baseline=baseline(Y), min_valid=min_valid(Y), outputs=ALL, out=outs)
    side.synchronize()
    eng.check()
    assert all(got[i] is outs[k] for i, k in enumerate(ALL))
    assert_same(got, want, 'strided, %s' % dtype)
    for k, (rows, kind) in kinds.items():                          # the guard elements: in front and between the rows
        assert float(bufs[k][0]) == 0
        assert bool((bufs[k][1:].view(rows, n + 5)[:, n:] == 0).all()), k
    on_input = nbuf[:P * n * (8 // nbuf.element_size())].view(torch.float64).view(P, n)      # on the first rows of num
    with pytest.raises(ValueError, match='overlaps'):
        eng.anomaly(num, den, periods=P, outputs=('mean',), out=dict(mean=on_input))
    with pytest.raises(ValueError, match='overlaps'):
        eng.anomaly(num, den, periods=P, outputs=('z', 'pct'), out=dict(z=outs['z'], pct=outs['z']))
    with pytest.raises(ValueError, match='overlaps'):
        eng.anomaly(num, num, periods=P, outputs=('z',), out=dict(z=num))


@pytest.mark.parametrize('dtype,Y,P,W', [('float32', 24, 5, 4), ('float64', 3, 5, 1)])
def test_host_mode_any_stage_bytes_and_both_entry_points_agree(env, dtype, Y, P, W):
    torch, mod16_amd = env
    S = Y * P
    once = definition(Y, P, W, dtype)
    want = an.Anomaly(*[np.concatenate([a, a], axis=1) for a in once])          # 600 pixels: pixels are independent
    num, den = (np.concatenate([a, a], axis=1) for a in record(Y, P, dtype))
    kw = dict(periods=P, window=W, baseline=baseline(Y), min_valid=min_valid(Y), outputs=ALL)
    fixed, per_pixel = 6 * 33 * 1024 + 512, (4 * S + 2 * P) * 8 + P
    for stage in (1, fixed + 520 * per_pixel, None):          # ranges of 256 pixels (three), of 512 (two), one range
        got = mod16_amd.anomaly_series(num, den, stage_bytes=stage, **kw)
        assert_same(got, want, 'HOST mode, stage_bytes = %r' % stage)
    some = mod16_amd.anomaly_series(num, None, periods=P, window=W, outputs=('pct', 'std'), stage_bytes=1)
    assert some.z is None and some.mean is None and some.count is None
    assert_same(some, an.anomaly(num, None, periods=P, window=W, outputs=('pct', 'std')), 'HOST mode, no den, a subset')
    cube = mod16_amd.anomaly_series(num.reshape(S, 8, 75), den.reshape(S, 8, 75), **kw)      # (S, R, C)
    assert cube.z.shape == (S, 8, 75) and cube.mean.shape == (P, 8, 75) and cube.count.shape == (P, 8, 75)
    dev = engine().anomaly(on_device(torch, num), on_device(torch, den), **kw)
    engine().check()
    assert_same(dev, want, 'RasterEngine.anomaly')
    assert_same(an.Anomaly(*[a.reshape(a.shape[0], -1) for a in cube]), host(dev), 'an (S, 8, 75) cube')


def test_two_calls_give_the_same_bits(env):
    torch, _ = env
    eng = engine()
    num, den = (on_device(torch, a) for a in record(64, 5, 'float32'))
    a = host(eng.anomaly(num, den, periods=5, window=4, outputs=ALL))
    b = host(eng.anomaly(num, den, periods=5, window=4, outputs=ALL))
    eng.check()
    for name, p, q in zip(ALL, a, b):
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), name


def test_composites_feed_the_anomaly_on_the_device(env):
    """Four "years" of two 8-day ET and PET totals of RasterEngine.composite over a 2 x 50 raster, written
    into the rows of two stacks and fed straight into RasterEngine.anomaly: the definition on the
    downloaded stacks."""
    torch, _ = env
    from oracle import synth
    eng = engine()
    years, P, days, n = 4, 2, 16, 2 * 50
    dev = eng._dev()
    et = torch.empty((years * P, n), dtype=torch.float64, device=dev)
    pet = torch.empty((years * P, n), dtype=torch.float64, device=dev)
    c_et = torch.empty((years * P, n), dtype=torch.uint16, device=dev)
    c_pet = torch.empty((years * P, n), dtype=torch.uint16, device=dev)
    for y in range(years):
        cls, drivers = synth.drivers((days, n), seed=300 + y, special=False)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        c = torch.from_numpy(np.ascontiguousarray(synth.drivers((1, n), seed=300, special=False)[0][0])).to(dev)
        hours = put(np.random.default_rng(y).uniform(6, 18, (days, n)))
        rows = slice(y * P, (y + 1) * P)
        eng.composite(c, [put(d) for d in drivers], hours, days, period_days=8, pet=True,
                      out=[et[rows], pet[rows], c_et[rows], c_pet[rows]])
    got = eng.anomaly(et, pet, periods=P, window=2, min_valid=3, outputs=ALL)
    eng.check()
    e, p = et.cpu().numpy(), pet.cpu().numpy()
    want = an.anomaly(e, p, periods=P, window=2, min_valid=3, outputs=ALL)
    assert np.isfinite(e).sum() > 3 * P * n and np.isfinite(want.z).sum() > P * n
    assert_same(got, want, 'composites')
