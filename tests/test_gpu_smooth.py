"""GPU tests of the Whittaker smoother (mod16_smooth_u8 / _f32 / _f64: RasterEngine.smooth,
mod16_amd.smooth_series) against its numpy definition (mod16_amd/smooth.py, itself held to a scalar
loop and to the dense solve by tests/test_smooth_host.py). Every output must be EQUAL to the
definition -- uint8 and uint16 value for value, the floats bit for bit (integer views; NaN is any
NaN): the kernel performs the definition's float64 operations in its order, so there is no tolerance.

Base shape: S = 23 slabs, n = 8192 + 37 pixels (33 blocks of 256 lanes, the last with 37), codes and QC
from the recipe of tests/test_gapfill_host.py (codes uniform in 0..100 with 5 % fill codes, QC bytes that
weight ~57 % of the slabs under the 1 / 0.5 / 0 table), a float32 weight stack that also holds 0, NaN
and negative weights, and nine planted pixels (PLANTS): never weighted; 1, 2 and 3 weighted slabs
(order - 1, order and min_valid of the two orders); weighted only in the first, only in the last slab;
weighted everywhere; a constant series; one deep single-slab dip. The kernel has ONE storage path (the
workspace of columns, for every S), so there is no switch to straddle: S = 1 ... 5, 23 and 138 are the
lengths. The definition's z of a configuration is computed once and shared by the output types."""
import functools

import numpy as np
import pytest

from mod16_amd import smooth as sm
from test_gapfill_host import recipe, same_bits

pytestmark = pytest.mark.gpu

S = 23
N = 8192 + 37
PLANTS = dict(never=5, one=6, two=7, three=8, first=9, last=10, everywhere=11, constant=12, dip=13)
PAIRS = [('uint8', 'uint8'), ('uint8', 'float32'), ('uint8', 'float64'), ('float32', 'float32'), ('float64', 'float64')]
SCALE = 0.01            # of the uint8 -> float outputs

q_ = np.arange(256)
GRADED = np.where(((q_ & 1) == 0) & ((q_ & 4) == 0) & np.isin((q_ >> 3) & 3, (0, 3)),
                  np.select([(q_ >> 5) == 0, (q_ >> 5) == 1], [1.0, 0.5], 0.0), 0.0)
GRADED.setflags(write=False)


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    return torch, mod16_amd, _lib


@functools.lru_cache(maxsize=None)
def engine(dtype='float64'):
    from mod16_amd.raster import RasterEngine
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    return RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250), dtype=dtype)


@functools.lru_cache(maxsize=None)
def inputs(s=S, n=N, seed=7):
    """-> (codes uint8, qc uint8, weights float32), read-only; the planted pixels where n holds them."""
    codes, qc, _ = recipe(s, n, seed)
    rng = np.random.default_rng(seed + 100)
    w = rng.choice(np.array([0, 0.5, 1, 0.25, np.nan, -1], np.float32), (s, n), p=[.25, .25, .25, .1, .1, .05])
    if n > max(PLANTS.values()):
        def plant(p, slabs, values=None):
            """pixel p is weighted at `slabs` only (fill codes elsewhere: in every weight mode)"""
            col = np.full(s, 255, np.uint8)
            col[slabs] = np.minimum(codes[slabs, p], 100) if values is None else values
            codes[:, p] = col
            qc[:, p] = 1
            qc[slabs, p] = 0
            w[:, p] = 0
            w[slabs, p] = 1
        every = np.arange(s)
        mid = s // 2
        plant(PLANTS['never'], [])
        plant(PLANTS['one'], [mid])
        plant(PLANTS['two'], [0, s - 1] if s > 1 else [0])
        plant(PLANTS['three'], sorted({0, mid, s - 1}))
        plant(PLANTS['first'], [0])
        plant(PLANTS['last'], [s - 1])
        plant(PLANTS['everywhere'], every)
        plant(PLANTS['constant'], every, 37)
        curve = np.round(40 + 30 * np.sin(np.pi * every / max(s - 1, 1))).astype(np.uint8)
        curve[mid] = 5
        plant(PLANTS['dip'], every, curve)
    for a in (codes, qc, w):
        a.setflags(write=False)
    return codes, qc, w


@functools.lru_cache(maxsize=None)
def values_as(in_type, s=S, n=N, seed=7):
    codes = inputs(s, n, seed)[0]
    if in_type == 'uint8':
        return codes
    v = np.where(codes >= 249, np.nan, codes * 0.37).astype(in_type)
    v.setflags(write=False)
    return v


def weight_kw(mode, s=S, n=N, seed=7):
    _, qc, w = inputs(s, n, seed)
    return {'none': {}, 'stack': dict(weights=w), 'qc': dict(qc=qc, qc_weight=GRADED)}[mode]


@functools.lru_cache(maxsize=None)
def solved(in_type, mode, lam, order, envelope, s=S, n=N, seed=7):
    """-> (z float64, count uint16) of the definition, read-only."""
    kw = weight_kw(mode, s, n, seed)
    y, w = sm.weights_of(values_as(in_type, s, n, seed), kw.get('weights'), kw.get('qc'), kw.get('qc_weight'))
    z = sm.smooth_values(y, w, lam, order, envelope)
    cnt = (w > 0).sum(axis=0).astype(np.uint16)
    z.setflags(write=False)
    cnt.setflags(write=False)
    return z, cnt


def oracle(in_type, out_type, mode, lam, order, envelope, min_valid=3, s=S, n=N, seed=7):
    z, cnt = solved(in_type, mode, lam, order, envelope, s, n, seed)
    scale = SCALE if (in_type == 'uint8' and out_type != 'uint8') else 1.0
    return sm.encode(z, cnt, min_valid, out_type, scale), cnt


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def counts(torch, t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def run_device(torch, in_type, out_type, mode, lam, order, envelope, min_valid=3, s=S, n=N, seed=7, **more):
    kw = {k: (v if k == 'qc_weight' else dev(torch, v)) for k, v in weight_kw(mode, s, n, seed).items()}
    scale = SCALE if (in_type == 'uint8' and out_type != 'uint8') else None
    eng = engine()
    kw.update(more)
    kw.setdefault('values', None)
    values = kw.pop('values')
    if values is None:
        values = dev(torch, values_as(in_type, s, n, seed))
    out, cnt = eng.smooth(values, lam=lam, order=order, envelope=envelope, min_valid=min_valid, dtype=out_type,
                          scale=scale, count=True, **kw)
    eng.check()
    return out.cpu().numpy(), counts(torch, cnt)


def assert_equal(got, want, what):
    (g, gc), (w, wc) = got, want
    assert np.array_equal(gc, wc), '%s: counts differ at %d pixels' % (what, (gc != wc).sum())
    if not same_bits(g, w):
        both = ~(np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64)))
        bad = np.argwhere((g != w) & both)
        raise AssertionError('%s: %d elements differ, first at slab %d pixel %d: %r, want %r'
                             % (what, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])]))


def test_the_recipe_reaches_every_planted_case():
    for mode in ('none', 'stack', 'qc'):
        cnt = solved('uint8', mode, 0.5, 2, 0)[1]
        assert [int(cnt[PLANTS[k]]) for k in ('never', 'one', 'two', 'three', 'first', 'last', 'everywhere', 'constant', 'dip')] == \
            [0, 1, 2, 3, 1, 1, S, S, S]
    cnt = solved('uint8', 'qc', 0.5, 2, 0)[1]
    assert 0.5 < cnt[14:].mean() / S < 0.65
    # the dip is lifted by the envelope, the constant series comes back as it is
    z0, z3 = solved('uint8', 'none', 0.5, 2, 0)[0], solved('uint8', 'none', 0.5, 2, 3)[0]
    assert z3[S // 2, PLANTS['dip']] > z0[S // 2, PLANTS['dip']] + 1
    assert np.abs(solved('uint8', 'none', 1600.0, 2, 0)[0][:, PLANTS['constant']] - 37).max() < 1e-9


@pytest.mark.parametrize('in_type,out_type', PAIRS)
@pytest.mark.parametrize('mode', ['none', 'stack', 'qc'])
@pytest.mark.parametrize('envelope', [0, 1, 3])
@pytest.mark.parametrize('lam', [0.5, 1600.0])
@pytest.mark.parametrize('order', [1, 2])
def test_equals_the_definition(env, order, lam, envelope, mode, in_type, out_type):
    torch = env[0]
    want = oracle(in_type, out_type, mode, lam, order, envelope)
    got = run_device(torch, in_type, out_type, mode, lam, order, envelope)
    assert_equal(got, want, '%s -> %s, %s, order %d, lam %g, envelope %d' % (in_type, out_type, mode, order, lam, envelope))
    smoothed = want[1] >= 3
    if out_type == 'uint8':
        assert (got[0][:, ~smoothed] == 255).all() and (got[0][:, smoothed] <= 248).all()
    else:
        assert np.isnan(got[0][:, ~smoothed]).all() and np.isfinite(got[0][:, smoothed]).all()


@pytest.mark.parametrize('order', [1, 2])
def test_min_valid_at_the_order(env, order):
    """min_valid = order: the pixel with exactly `order` weighted slabs is solved, the one with order - 1 is not."""
    torch = env[0]
    for envelope in (0, 2):
        want = oracle('uint8', 'float64', 'qc', 10.0, order, envelope, min_valid=order)
        got = run_device(torch, 'uint8', 'float64', 'qc', 10.0, order, envelope, min_valid=order)
        assert_equal(got, want, 'min_valid = order = %d' % order)
        exactly, below = (PLANTS['one'], PLANTS['never']) if order == 1 else (PLANTS['two'], PLANTS['one'])
        assert np.isfinite(got[0][:, exactly]).all() and np.isnan(got[0][:, below]).all()


@pytest.mark.parametrize('in_type,out_type', [('uint8', 'uint8'), ('uint8', 'float32'), ('float64', 'float64')])
@pytest.mark.parametrize('s,n', [(1, 257), (2, 257), (3, 257), (4, 257), (5, 257), (138, 515), (S, 1), (S, 3), (S, 255)])
def test_short_long_and_small(env, s, n, in_type, out_type):
    """S = 1 ... 5: every row of the bands is an edge row, and S <= order has no penalty at all."""
    torch = env[0]
    for order, envelope, mode in ((1, 0, 'qc'), (2, 2, 'qc'), (2, 1, 'stack')):
        want = oracle(in_type, out_type, mode, 10.0, order, envelope, order, s, n, 11)
        got = run_device(torch, in_type, out_type, mode, 10.0, order, envelope, order, s, n, 11)
        assert_equal(got, want, 'S = %d, n = %d, order %d' % (s, n, order))


def test_no_pixels(env):
    torch = env[0]
    out, cnt = engine().smooth(torch.empty((S, 0), dtype=torch.uint8, device='cuda'), lam=1.0, dtype='float32', count=True)
    assert tuple(out.shape) == (S, 0) and out.dtype == torch.float32 and tuple(cnt.shape) == (0,)


@pytest.mark.parametrize('in_type,out_type', [('uint8', 'uint8'), ('uint8', 'float64'), ('float32', 'float32')])
@pytest.mark.parametrize('offset', [1, 3])
def test_views_at_odd_offsets_and_pitches(env, in_type, out_type, offset):
    """Values, weights, QC and outputs as views that start 1 and 3 elements into a larger buffer, rows n + 5
    apart; the padding stays untouched."""
    torch = env[0]
    pitch = N + 5

    def view(dt, rows=S):
        elem = torch.empty((), dtype=dt).element_size()
        buf = torch.full(((rows * pitch + 8) * elem,), 0xA5, dtype=torch.uint8, device='cuda').view(dt)
        return buf, buf[offset:offset + rows * pitch].view(rows, pitch)[:, :N]
    tin = getattr(torch, in_type)
    _, vv = view(tin)
    vv.copy_(dev(torch, values_as(in_type)))
    codes, qc, w = inputs()
    for mode, (src, dt) in (('qc', (qc, torch.uint8)), ('stack', (w, torch.float32))):
        _, wv = view(dt)
        wv.copy_(dev(torch, src))
        obuf, ov = view(getattr(torch, out_type))
        cbuf = torch.full((2 * (N + 8),), 0xA5, dtype=torch.uint8, device='cuda').view(torch.uint16)
        cv = cbuf[offset:offset + N]
        want = oracle(in_type, out_type, mode, 1600.0, 2, 2)
        got = run_device(torch, in_type, out_type, mode, 1600.0, 2, 2, values=vv, out=(ov, cv),
                         **({'qc': wv} if mode == 'qc' else {'weights': wv}))
        assert_equal(got, want, 'views at offset %d, %s' % (offset, mode))
        raw = obuf.view(torch.uint8).cpu().numpy()
        e = obuf.element_size()
        mask = np.ones(raw.size, bool)
        for r in range(S):
            lo = (offset + r * pitch) * e
            mask[lo:lo + N * e] = False
        assert (raw[mask] == 0xA5).all()
        craw = cbuf.view(torch.uint8).cpu().numpy()
        assert (craw[:2 * offset] == 0xA5).all() and (craw[2 * (offset + N):] == 0xA5).all()


def test_out_reuse_two_launches_same_bits_and_nothing_untouched(env):
    torch = env[0]
    for in_type, out_type in (('uint8', 'uint8'), ('float64', 'float64')):
        tdtype = getattr(torch, out_type)
        esz = torch.empty((), dtype=tdtype).element_size()
        out = torch.full((S, N * esz), 0xA5, dtype=torch.uint8, device='cuda').view(tdtype)
        cnt = torch.full((2 * N,), 0xA5, dtype=torch.uint8, device='cuda').view(torch.uint16)
        want = oracle(in_type, out_type, 'qc', 1600.0, 2, 1)
        first = run_device(torch, in_type, out_type, 'qc', 1600.0, 2, 1, out=(out, cnt))
        assert_equal(first, want, 'out=')
        # the same tensors again with another configuration: every element is written again
        again = run_device(torch, in_type, out_type, 'stack', 0.5, 1, 0, out=(out, cnt))
        assert_equal(again, oracle(in_type, out_type, 'stack', 0.5, 1, 0), 'out= reused')
        back = run_device(torch, in_type, out_type, 'qc', 1600.0, 2, 1, out=(out, cnt))
        assert back[0].tobytes() == first[0].tobytes() and back[1].tobytes() == first[1].tobytes()


@pytest.mark.parametrize('in_type,out_type,mode', [('uint8', 'float32', 'qc'), ('uint8', 'uint8', 'stack'),
                                                   ('float64', 'float64', 'none')])
def test_host_mode_equals_device_mode_across_tiles(env, in_type, out_type, mode):
    """numpy in / numpy out through the staged tiles. A slot holds 4 x 33 KiB of stagger + 512 bytes and,
    per pixel, the rows of the plan: these stage sizes give tiles of 2048 and 1024 pixels (5 and 9 tiles,
    the last ragged)."""
    torch, mod16_amd = env[0], env[1]
    want = oracle(in_type, out_type, mode, 1600.0, 2, 2)
    device = run_device(torch, in_type, out_type, mode, 1600.0, 2, 2)
    assert_equal(device, want, 'DEVICE')
    kw = weight_kw(mode)
    osz, isz = np.dtype(out_type).itemsize, np.dtype(in_type).itemsize
    esz = max(osz, isz, 4 if mode == 'stack' else 1, 2)
    wide_rows = S + (1 if isz == 1 else S) + (S if mode == 'stack' else 1) + 1
    byte_rows = (S if isz == 1 else 1) + (S if mode == 'qc' else 1)
    fixed = 4 * 33 * 1024 + 512
    scale = SCALE if (in_type == 'uint8' and out_type != 'uint8') else None
    for pixels in (2048 + 100, 1024 + 100, None):
        stage = None if pixels is None else fixed + pixels * (wide_rows * esz + byte_rows)
        out, cnt = mod16_amd.smooth_series(values_as(in_type), lam=1600.0, order=2, envelope=2, dtype=out_type, scale=scale,
                                           count=True, stage_bytes=stage, **kw)
        assert_equal((out, cnt), device, 'HOST, stage for %r pixels' % pixels)


def test_smooth_series_on_a_pixel_shape(env):
    mod16_amd = env[1]
    s, shape = S, (7, 13)
    codes, qc, w = inputs(s, 7 * 13, 5)
    got = mod16_amd.smooth_series(codes.reshape((s,) + shape), qc=qc.reshape((s,) + shape), lam=10.0, envelope=1,
                                  dtype='float32', scale=0.1)
    assert got.shape == (s,) + shape and got.dtype == np.float32
    want = sm.smooth(codes, qc=qc, lam=10.0, envelope=1, dtype='float32', scale=0.1)
    assert same_bits(got.reshape(s, 91), want)
    # the default table is gapfill's table of acceptable bytes; a float stack of weights, without counts
    vals = values_as('float64', s, 91, 5).reshape((s,) + shape)
    got = mod16_amd.smooth_series(vals, weights=w.reshape((s,) + shape), lam=10.0, order=1)
    assert same_bits(got.reshape(s, 91), sm.smooth(vals.reshape(s, 91), weights=w, lam=10.0, order=1))


def test_tensor_refusals(env):
    torch = env[0]
    eng = engine()
    codes, qc, w = inputs()
    v, q, wt = dev(torch, codes), dev(torch, qc), dev(torch, w)
    keep = v.clone()
    with pytest.raises(TypeError, match='values must be a uint8 or float32 or float64 tensor'):
        eng.smooth(v.to(torch.int16), lam=1.0)
    with pytest.raises(TypeError, match='values must be'):
        eng.smooth(v.cpu(), lam=1.0)
    with pytest.raises(TypeError, match='weights must be a float32 tensor'):
        eng.smooth(v, weights=wt.double(), lam=1.0)
    with pytest.raises(TypeError, match='qc must be a uint8 tensor'):
        eng.smooth(v, qc=q.cpu(), lam=1.0)
    with pytest.raises(TypeError, match=r'out\[0\] must be a float32 tensor'):
        eng.smooth(v, lam=1.0, dtype='float32', out=torch.empty((S, N), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='unit stride in pixels'):
        eng.smooth(dev(torch, np.ascontiguousarray(codes.T)).t(), lam=1.0)
    with pytest.raises(ValueError, match='stride in time must be at least'):
        eng.smooth(v[0].expand(S, N), lam=1.0)
    with pytest.raises(ValueError, match='unit stride in pixels'):
        eng.smooth(v, qc=dev(torch, np.ascontiguousarray(qc.T)).t(), lam=1.0)
    with pytest.raises(ValueError, match=r'values must be an \(S, n\) tensor'):
        eng.smooth(v.view(S, 3, N // 3), lam=1.0)
    with pytest.raises(ValueError, match='lam'):
        eng.smooth(v, lam=-1.0)
    with pytest.raises(ValueError, match='overlaps'):
        eng.smooth(v, qc=q, lam=1.0, out=v)                                    # in place
    with pytest.raises(ValueError, match='overlaps'):
        eng.smooth(v, qc=q, lam=1.0, out=q)                                    # the QC layer as the output
    big = torch.zeros(S * N + N, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):                          # one row of overlap
        eng.smooth(big[:S * N].view(S, N), lam=1.0, out=big[N:].view(S, N))
    out = torch.empty((S, N), dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):                          # the counts on the output
        eng.smooth(v, lam=1.0, dtype='float64', count=True, out=(out, out.view(torch.uint16).view(-1)[:N]))
    eng.check()
    assert torch.equal(v, keep)                                                # refused before any device work
