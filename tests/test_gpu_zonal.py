"""GPU tests of the zonal statistics (mod16_zonal_*: RasterEngine.zonal, mod16_amd.zonal_statistics)
against the numpy definition (mod16_amd/zonal.py, itself held to Python big integers by
tests/test_zonal_host.py). Every comparison is EQUALITY of the int64 words with `zonal.accumulate`
under identical explicit bounds: the sums are integers, so there is no tolerance anywhere.

Base shape: (R, C) = (61, 67), n = 4087 -- ragged against every vector (2, 4), wave (64) and block
(256) size -- K = 3 layers; zones are coherent blocks ((row // 8) * 5 + col // 16: 40 zones) with 5 %
of the ids replaced at random and 5 % of ids >= Z; values gamma-distributed with 5 % NaN and every
17th negative; planted pixels: |x| just above xmax, +inf, -inf, exactly +-xmax with w == wmax, w = 0,
w = NaN, w < 0, -0.0 next to +0.0 in one zone. Bounds: exact powers of two in one case, not in the
other. The oracle of a configuration is computed once and shared."""
import functools

import numpy as np
import pytest

from mod16_amd import zonal as zs

pytestmark = pytest.mark.gpu

R, C, K, Z0 = 61, 67, 3, 40
N = R * C
BOUNDS = {'pow2': (262144.0, 64.0), 'odd': (2.5e5, 50.0)}
ROWS = R + 40          # per-row weights reach beyond the raster: sub-ranges start further down


@functools.lru_cache(maxsize=None)
def table():
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    t = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def engine(dtype='float64'):
    from mod16_amd.raster import RasterEngine
    return RasterEngine(table(), dtype=dtype)


def block_zones(n=N):
    row, col = np.divmod(np.arange(n), C)
    return (row // 8) * 5 + col // 16


@functools.lru_cache(maxsize=None)
def inputs(dtype, case, nzones=Z0, zmap='blocks', n=N, seed=5):
    """(values (K, n), zones (n,) int64, per-pixel weights (n,), per-row weights (ROWS,)), read-only."""
    wmax, xmax = BOUNDS[case]
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, 1.5, size=(K, n))
    x[rng.random((K, n)) < 0.05] = np.nan
    x[:, ::17] *= -1.0
    x = x.astype(dt)
    if zmap == 'blocks':
        z = block_zones(n) * nzones // Z0 if nzones != Z0 else block_zones(n)
        swap = rng.random(n) < 0.05
        z = np.where(swap, rng.integers(0, nzones, n), z)
        z = np.where(rng.random(n) < 0.05, nzones + rng.integers(0, 3, n), z)
        z[n // 2] = nzones - 1               # the top zone is reached
        x[:, n // 2] = 1.5
    elif zmap == 'noruns':
        z = (np.arange(n) * 7) % nzones      # every pixel's zone differs from its neighbour's
        z[0] = nzones - 1
        x[:, 0] = 1.5
    else:
        z = np.full(n, nzones - 1)           # one zone: every lane on one entry
    wp = (2e5 * (1.0 + 0.1 * rng.random(n))).astype(dt)
    wr = 1e5 * (1.5 + np.cos(np.arange(ROWS)))
    if n >= 1000:
        plant = iter(range(300, 1000, 31))
        for value, weight in ((np.nextafter(dt.type(xmax), dt.type(np.inf)), None), (np.inf, None), (-np.inf, None),
                              (xmax, wmax), (-xmax, wmax), (1.0, 0.0), (1.0, np.nan), (1.0, -3.0), (np.nan, np.nan),
                              (np.inf, np.nan)):
            i = next(plant)
            x[:, i] = value
            if zmap == 'blocks':
                z[i] = 3
            if weight is not None:
                wp[i] = weight
        i = next(plant)
        x[:, i], x[:, i + 1] = -0.0, 0.0
        if zmap == 'blocks':
            z[i] = z[i + 1] = 0
        x[1, z == 0] = np.where(np.arange((z == 0).sum()) % 2, 0.0, -0.0)     # a zone of nothing but zeros
        wr[3], wr[5], wr[7], wr[9] = 0.0, np.nan, -1.0, wmax
    for a in (x, z, wp, wr):
        a.setflags(write=False)
    return x, z, wp, wr


def weights_of(kind, wp, wr, lo=0, hi=None):
    """-> the keywords of `zonal.accumulate` for the pixels [lo, hi)."""
    if kind == 'none':
        return {}
    if kind == 'row':
        return dict(weights=wr, cols=C, first_pixel=lo)
    return dict(weights=wp[lo:hi])


@functools.lru_cache(maxsize=None)
def oracle(dtype, case, kind, nzones=Z0, zmap='blocks', n=N, lo=0, hi=None):
    x, z, wp, wr = inputs(dtype, case, nzones, zmap, n)
    acc = zs.accumulate(x[:, lo:hi], z[lo:hi], nzones, bounds=BOUNDS[case], **weights_of(kind, wp, wr, lo, hi))
    acc.setflags(write=False)
    return acc


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).cuda()


def device_words(dtype, x, z, nzones, kind, wp, wr, bounds, ztype=np.int32, lo=0, hi=None, acc=None, first=None):
    """RasterEngine.zonal on the pixels [lo, hi) -> the accumulator as numpy (and the tensor)."""
    import torch
    eng = engine(dtype)
    area, cols = None, None
    if kind == 'row':
        area, cols = dev(wr), C
    elif kind == 'pixel':
        area = dev(wp[lo:hi])
    out = eng.zonal(dev(x[:, lo:hi]), dev(z[lo:hi].astype(ztype)), nzones, area=area, cols=cols,
                    first_pixel=lo if first is None else first, bounds=bounds, acc=acc)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out


@pytest.mark.parametrize('case', ['pow2', 'odd'])
@pytest.mark.parametrize('kind', ['none', 'row', 'pixel'])
@pytest.mark.parametrize('ztype', [np.uint8, np.int32])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_device_call_equals_the_definition(dtype, ztype, kind, case):
    x, z, wp, wr = inputs(dtype, case)
    want = oracle(dtype, case, kind)
    assert want[..., zs.COUNT].sum() > 0.8 * K * N and want[..., zs.REJECTED].sum() >= 3 * K
    got, _ = device_words(dtype, x, z, Z0, kind, wp, wr, BOUNDS[case], ztype)
    assert np.array_equal(got, want)
    if kind == 'row':        # a sub-range that starts and ends in the middle of a row
        lo, hi = 1000, 3001
        got, _ = device_words(dtype, x, z, Z0, kind, wp, wr, BOUNDS[case], ztype, lo, hi)
        assert np.array_equal(got, oracle(dtype, case, kind, lo=lo, hi=hi))
    if ztype == np.int32:    # negative ids are outside every zone
        z2 = z.copy()
        z2[::50] = -1 - z2[::50]
        got, _ = device_words(dtype, x, z2, Z0, kind, wp, wr, BOUNDS[case], ztype)
        assert np.array_equal(got, zs.accumulate(x, z2, Z0, bounds=BOUNDS[case], **weights_of(kind, wp, wr)))


@pytest.mark.parametrize('zmap', ['blocks', 'noruns', 'one'])
@pytest.mark.parametrize('where', ['small', 'lds', 'global'])
def test_both_accumulation_paths(where, zmap):
    from mod16_amd import _lib
    lds = _lib.zonal_lds_zones()
    assert lds >= 256
    nzones = {'small': Z0, 'lds': lds, 'global': lds + 3}[where]
    x, z, wp, wr = inputs('float64', 'pow2', nzones, zmap)
    assert z.max() >= nzones - 1 and (zmap != 'noruns' or (np.diff(z) != 0).all())
    want = oracle('float64', 'pow2', 'pixel', nzones, zmap)
    assert want[:, nzones - 1, zs.COUNT].all()
    got, _ = device_words('float64', x, z, nzones, 'pixel', wp, wr, BOUNDS['pow2'])
    assert np.array_equal(got, want)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_small_shapes(dtype, n):
    x, z, wp, wr = inputs(dtype, 'odd', n=n)
    for kind in ('none', 'row', 'pixel'):
        got, _ = device_words(dtype, x, z, Z0, kind, wp, wr, BOUNDS['odd'], np.uint8)
        assert np.array_equal(got, oracle(dtype, 'odd', kind, n=n)), kind


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('cols', [1, 3])
def test_rows_narrower_than_a_vector(dtype, cols):
    """Per-row weights over rows of 1 and 3 pixels: a 16-byte vector of 2 or 4 values crosses a row end
    more than once. The range starts at raster pixel 2; 2051 pixels are several blocks, the last vector
    ragged; the weights are positive, (first_pixel + n - 1) // cols + 1 of them."""
    import torch
    n, first, layers, nzones = 2051, 2, 2, 5
    rng = np.random.default_rng(11)
    x = rng.gamma(2.0, 1.5, size=(layers, n)).astype(dtype)
    z = np.where(rng.random(n) < 0.2, rng.integers(0, nzones, n), (np.arange(n) // 29) % nzones)
    wr = 1e5 * (1.5 + np.cos(np.arange((first + n - 1) // cols + 1)))
    assert len(wr) == {1: 2053, 3: 685}[cols] and (wr > 0).all()
    want = zs.accumulate(x, z, nzones, weights=wr, cols=cols, first_pixel=first, bounds=BOUNDS['odd'])
    assert want[..., zs.COUNT].sum() == layers * n
    got = engine(dtype).zonal(dev(x), dev(z.astype(np.uint8)), nzones, area=dev(wr), cols=cols, first_pixel=first,
                              bounds=BOUNDS['odd'])
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('ztype', [np.uint8, np.int32])
def test_unaligned_views_and_value_pitch(dtype, ztype):
    import torch
    eng = engine(dtype)
    x, z, wp, wr = inputs(dtype, 'pow2')
    want = oracle(dtype, 'pow2', 'pixel')
    for off, pitch in ((0, N + 13), (3, N + 13), (1, N + 6)):      # aligned rows apart; odd element offsets
        big = torch.full((K, pitch), float('inf'), dtype=eng.dtype, device='cuda')
        values = big[:, off:off + N]
        values.copy_(dev(x))
        zbig = torch.zeros(N + 8, dtype=torch.uint8 if ztype == np.uint8 else torch.int32, device='cuda')
        zones = zbig[off:off + N]
        zones.copy_(dev(z.astype(ztype)))
        wbig = torch.zeros(N + 8, dtype=eng.dtype, device='cuda')
        area = wbig[off:off + N]
        area.copy_(dev(wp))
        assert values.stride(0) == pitch and values.data_ptr() % 16 == (off * values.element_size()) % 16
        got = eng.zonal(values, zones, Z0, area=area, bounds=BOUNDS['pow2'])
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), (off, pitch)


@pytest.mark.parametrize('kind', ['none', 'row', 'pixel'])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_order_independence(dtype, kind):
    from mod16_amd import _lib
    x, z, wp, wr = inputs(dtype, 'odd')
    bounds = BOUNDS['odd']
    want = oracle(dtype, 'odd', kind)
    one, _ = device_words(dtype, x, z, Z0, kind, wp, wr, bounds)
    again, _ = device_words(dtype, x, z, Z0, kind, wp, wr, bounds)
    assert np.array_equal(one, want) and np.array_equal(again, one)
    # the same pixels in two calls that accumulate into one acc
    cut = 2001
    _, acc = device_words(dtype, x, z, Z0, kind, wp, wr, bounds, hi=cut)
    two, _ = device_words(dtype, x, z, Z0, kind, wp, wr, bounds, lo=cut, acc=acc)
    assert np.array_equal(two, want)
    # HOST mode, 16 tiles of 256 pixels on the context's staging slots
    ctx = _lib.context(0)
    z32 = np.ascontiguousarray(z, np.int32)
    host = zs.empty(K, Z0)
    w = {'none': None, 'row': wr, 'pixel': wp}[kind]
    wk = {'none': _lib.ZONAL_WEIGHT_NONE, 'row': _lib.ZONAL_WEIGHT_ROW, 'pixel': _lib.ZONAL_WEIGHT_PIXEL}[kind]
    xc = np.ascontiguousarray(x)
    ctx.zonal(xc.dtype, N, K, Z0, zs.ZONE_I32, xc.ctypes.data, z32.ctypes.data, None if w is None else w.ctypes.data,
              host.ctypes.data, zs.check_bounds(bounds), weight_kind=wk, cols=C, where=_lib.HOST, stage_bytes=1)
    assert np.array_equal(host, want)
    if kind != 'row':        # the pixels permuted
        perm = np.random.default_rng(1).permutation(N)
        got, _ = device_words(dtype, x[:, perm], z[perm], Z0, kind, wp[perm], wr, bounds)
        assert np.array_equal(got, want)


def test_capacity_of_the_hi_lo_words():
    import torch
    n = 1 << 20
    wmax, xmax = BOUNDS['pow2']
    eng = engine('float64')
    values = torch.full((1, n), xmax, dtype=torch.float64, device='cuda')
    area = torch.full((n,), wmax, dtype=torch.float64, device='cuda')
    zones = torch.zeros(n, dtype=torch.uint8, device='cuda')
    got = eng.zonal(values, zones, 1, area=area, bounds=BOUNDS['pow2'])
    torch.cuda.synchronize()
    q = n << 62                                          # every term is 2^62
    want = [n, 0, q >> 32, q & 0xffffffff, q >> 32, q & 0xffffffff, q >> 32, q & 0xffffffff,
            int(zs.key(xmax)), int(zs.key(xmax))]
    assert got.cpu().numpy()[0, 0].tolist() == want
    res = zs.ZonalResult.from_tensor(got)
    assert res.sum_w[0, 0] == n * wmax and res.sum_wxx[0, 0] == n * wmax * xmax * xmax and res.var[0, 0] == 0.0


@pytest.mark.parametrize('kind', ['none', 'row', 'pixel'])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bounds_pre_pass(dtype, kind):
    import torch
    eng = engine(dtype)
    x, z, wp, wr = inputs(dtype, 'odd')
    lo = 1000 if kind == 'row' else 0
    area = {'none': None, 'row': dev(wr), 'pixel': dev(wp)}[kind]
    got = eng.zonal_bounds(dev(x[:, lo:]), area, C if kind == 'row' else None, lo)
    xa = np.abs(x[:, lo:].astype(np.float64))
    wa = {'none': np.ones(1), 'row': wr[lo // C:(N - 1) // C + 1], 'pixel': wp.astype(np.float64)}[kind]
    assert got == (wa[np.isfinite(wa) & (wa >= 0)].max(), xa[np.isfinite(xa)].max())
    if kind == 'none':       # bounds=None: the pre-pass's bounds reject nothing but the infinities
        out = eng.zonal(dev(x), dev(z.astype(np.int32)), Z0)
        torch.cuda.synchronize()
        res = zs.ZonalResult.from_tensor(out)
        assert (res.ew, res.ex) == (zs.exponent(got[0]), zs.exponent(got[1]))
        assert np.array_equal(res.words, zs.accumulate(x, z, Z0, bounds=got))
        inside = (z >= 0) & (z < Z0)
        assert res.rejected.sum() == np.isinf(x[:, inside]).sum() > 0


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_public_call_end_to_end(dtype):
    import mod16_amd
    x, z, wp, wr = inputs(dtype, 'pow2')
    z2, area = z.reshape(R, C), wr[:R]
    res = mod16_amd.zonal_statistics(x.reshape(K, R, C), z2, nzones=Z0, area=area)
    xa = np.abs(x.astype(np.float64))
    bounds = (area[np.isfinite(area) & (area >= 0)].max(), xa[np.isfinite(xa)].max())
    want = zs.ZonalResult(zs.accumulate(x, z, Z0, weights=area, cols=C, bounds=bounds), zs.exponent(bounds[0]),
                          zs.exponent(bounds[1]))
    assert (res.ew, res.ex) == (want.ew, want.ex) and np.array_equal(res.words, want.words)
    for name in ('count', 'rejected', 'sum_w', 'sum_wx', 'sum_wxx', 'mean', 'var', 'std', 'min', 'max'):
        a, b = getattr(res, name), getattr(want, name)
        assert a.shape == (K, Z0) and np.array_equal(a, b, equal_nan=True), name
    assert np.isnan(res.mean).any() or (res.count > 0).all()
    # one layer without a layer axis, uint16 zones, a scalar area, staged in tiles: (Z,) statistics
    one = mod16_amd.zonal_statistics(x[0].reshape(R, C), z2.astype(np.uint16), nzones=Z0, area=2.5, stage_bytes=1)
    ref = zs.accumulate(x[:1], z, Z0, weights=np.array([2.5]), cols=N, bounds=(2.5, bounds[1]))
    assert one.sum_wx.shape == (Z0,) and np.array_equal(one.words, ref)
    # accumulating two halves with explicit bounds (that cover the finite pixels; the infinities are cut out)
    fin = np.where(np.isinf(x), np.nan, x).astype(x.dtype)
    full = (BOUNDS['pow2'][0], 128.0)
    whole = mod16_amd.zonal_statistics(fin, z, nzones=Z0, area=np.abs(np.nan_to_num(wp)), bounds=full)
    h = N // 2
    first = mod16_amd.zonal_statistics(fin[:, :h], z[:h], nzones=Z0, area=np.abs(np.nan_to_num(wp))[:h], bounds=full)
    both = mod16_amd.zonal_statistics(fin[:, h:], z[h:], nzones=Z0, area=np.abs(np.nan_to_num(wp))[h:], bounds=full, acc=first)
    assert np.array_equal(both.words, whole.words) and not whole.rejected.any()


def test_refusals():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    eng = engine('float64')
    x, z, wp, wr = inputs('float64', 'pow2')
    with pytest.raises(ValueError, match='zone 3, layer 0'):
        mod16_amd.zonal_statistics(x, z, nzones=Z0, bounds=BOUNDS['pow2'])
    vals, zones, area = dev(x), dev(z.astype(np.int32)), dev(wp)
    acc = eng.zonal(vals, zones, Z0, area=area, bounds=BOUNDS['pow2'])
    with pytest.raises(ValueError, match='exponents'):
        eng.zonal(vals, zones, Z0, area=area, bounds=(BOUNDS['pow2'][0], 65.0), acc=acc)
    with pytest.raises(ValueError, match='explicit bounds'):
        eng.zonal(vals, zones, Z0, area=area, acc=acc)
    with pytest.raises(TypeError):
        eng.zonal(vals, zones.to(torch.int64), Z0)
    torch.cuda.synchronize()
    before = acc.cpu().numpy()
    good = dict(dtype=np.float64, n=N, layers=K, nzones=Z0, zone_type=zs.ZONE_I32, values=vals.data_ptr(),
                zones=zones.data_ptr(), weights=area.data_ptr(), acc=acc.data_ptr(), bounds=zs.check_bounds(BOUNDS['pow2']),
                weight_kind=_lib.ZONAL_WEIGHT_PIXEL, where=_lib.DEVICE)
    for change in (dict(n=-1), dict(n=2 ** 30 + 1, value_pitch=2 ** 30 + 1), dict(layers=0), dict(layers=65536),
                   dict(nzones=0), dict(nzones=2 ** 24 + 1), dict(zone_type=3), dict(weight_kind=3), dict(where=7),
                   dict(weight_kind=_lib.ZONAL_WEIGHT_ROW, cols=0), dict(value_pitch=N - 1), dict(values=None),
                   dict(zones=None), dict(acc=None), dict(weights=None), dict(bounds=(1.0, 1.0, 963, 0)),
                   dict(bounds=(1.0, 1.0, 0, -500)), dict(bounds=(3.0, 1.0, 1, 0)), dict(bounds=(1.0, np.nan, 0, 0)),
                   dict(acc=vals.data_ptr() + 8), dict(acc=zones.data_ptr()), dict(acc=area.data_ptr())):
        with pytest.raises(_lib.Mod16Error, match='mod16_zonal: ') as info:
            eng.ctx.zonal(**dict(good, **change))
        assert info.value.status == _lib.ERR_ARG, change
    eng.ctx.zonal(**dict(good, n=0))                     # n = 0: fine, and acc stays as it was
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), before)
