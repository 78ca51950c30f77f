"""GPU tests of the zonal histograms and exact zonal quantiles (mod16_zonal_hist_*, mod16_zonal_select:
RasterEngine.zonal_histogram / zonal_selection / zonal_quantiles, mod16_amd.zonal_histogram /
zonal_quantiles) against the numpy definition (mod16_amd/zonalq.py, itself held to a per-pixel loop in
Python integers by tests/test_zonalq_host.py). Every comparison is EQUALITY: the int64 words equal,
the values with the same bits. There is no tolerance anywhere.

Values are normal(3, 2) with 5 % NaN and planted +-0.0, +-inf, a pair that differs in the last key bit;
weights carry 0, wmax, a weight below the quantum, NaN, a negative one and one above wmax. The device
inputs are views that start one element into their buffers, the layers n + 5 elements apart (scalar
accesses), or aligned with a pitch of whole vectors (vector accesses). The oracle of a configuration is
computed once and shared."""
import functools

import numpy as np
import pytest

from mod16_amd import zonalq as Q

pytestmark = pytest.mark.gpu

COLS, FIRST = 67, 5
WMAX = 2.5e5                                   # ew = 18
QS = {1: (0.5,), 3: (0.05, 0.5, 0.95), 5: (0.0, 5e-324, 0.1, 1 - 2.0 ** -53, 1.0)}


@functools.lru_cache(maxsize=None)
def table():
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    t = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def engine(dtype):
    from mod16_amd.raster import RasterEngine
    return RasterEngine(table(), dtype=dtype)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def lds_zones(slots, nb):
    """The largest zone count whose table of `slots` slots of `nb` words a block holds in LDS."""
    from mod16_amd import _lib
    return _lib.zonal_hist_lds_bytes() // 8 // (slots * nb)


@functools.lru_cache(maxsize=None)
def inputs(dtype, n, K, nzones, zmap='blocks', raster='random', seed=7):
    """(values (K, n), zones (n,) int64, per-pixel weights (n,), per-row weights), read-only."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed + n + 31 * nzones)
    if raster == 'constant':
        x = np.full((K, n), 2.5, dt)
    elif raster == 'pair':                      # two values that differ in the last key bit only
        x = np.where(rng.random((K, n)) < 0.5, dt.type(1.0), np.nextafter(dt.type(1.0), dt.type(2.0))).astype(dt)
    else:
        x = rng.normal(3.0, 2.0, (K, n))
        x[rng.random((K, n)) < 0.05] = np.nan
        x = x.astype(dt)
    if zmap == 'blocks':                        # coherent runs with 5 % of the ids replaced and 5 % out of range
        z = (np.arange(n) // 37) % nzones
        z = np.where(rng.random(n) < 0.05, rng.integers(0, nzones, n), z)
        z = np.where(rng.random(n) < 0.05, nzones + rng.integers(0, 3, n), z)
        z[n // 2] = nzones - 1
    elif zmap == 'noruns':
        z = (np.arange(n) * 7) % nzones
    else:
        z = np.full(n, nzones - 1)
    wp = (2e5 * (1.0 + 0.1 * rng.random(n))).astype(dt)
    wr = 1e5 * (1.5 + np.cos(np.arange((FIRST + n - 1) // COLS + 1)))
    if n >= 1000 and raster == 'random':
        spot = iter(range(300, 1000, 23))
        for value in (0.0, -0.0, np.inf, -np.inf, 1.0, np.nextafter(dt.type(1.0), dt.type(2.0)), -0.0, 0.0):
            x[:, next(spot)] = value
        for weight in (0.0, WMAX, 2.0 ** (18 - 33), np.nan, -3.0, WMAX * 1.01, 2.0 ** (18 - 31)):
            wp[next(spot)] = weight
        wr[3], wr[5], wr[7], wr[9], wr[11] = 0.0, np.nan, -1.0, WMAX, 2.0 ** (18 - 33)
    for a in (x, z, wp, wr):
        a.setflags(write=False)
    return x, z, wp, wr


def weights_of(kind, wp, wr, lo=0, hi=None):
    """-> the keywords of the definition for the pixels [lo, hi)."""
    if kind == 'none':
        return {}
    if kind == 'row':
        return dict(weights=wr, cols=COLS, first_pixel=FIRST + lo, wmax=WMAX)
    return dict(weights=wp[lo:hi], wmax=WMAX)


@functools.lru_cache(maxsize=None)
def oracle_quantiles(dtype, n, K, nzones, S, kind, bits, zmap='blocks', raster='random'):
    x, z, wp, wr = inputs(dtype, n, K, nzones, zmap, raster)
    return Q.quantiles(x, z, nzones, QS[S], bits=bits, **weights_of(kind, wp, wr))


@functools.lru_cache(maxsize=None)
def oracle_histogram(dtype, n, K, nzones, bins, kind, zmap='blocks', raster='random', lo=0, hi=None):
    x, z, wp, wr = inputs(dtype, n, K, nzones, zmap, raster)
    h = Q.histogram(x[:, lo:hi], z[lo:hi], nzones, bins, *RANGE, **weights_of(kind, wp, wr, lo, hi))
    h.setflags(write=False)
    return h


RANGE = (-1.0, 7.5)                            # some values lie under, some over


def device_inputs(dtype, x, z, wp, wr, zone_dtype, kind, aligned=False, lo=0, hi=None):
    """The pixels [lo, hi) on the device: (values view (K, m), zones, engine keywords)."""
    import torch
    eng = engine(dtype)
    dev = eng._dev()
    x, z = x[:, lo:hi], z[lo:hi]
    K, m = x.shape
    tdt = torch.float32 if dtype == 'float32' else torch.float64
    V = 16 // np.dtype(dtype).itemsize
    off, pitch = (0, (m + 5 + V - 1) // V * V) if aligned else (1, m + 5)
    buf = torch.full((off + K * pitch + 16,), float('nan'), dtype=tdt, device=dev)
    vals = buf[off:].as_strided((K, m), (pitch, 1))
    vals.copy_(torch.from_numpy(np.array(x)))
    zt = torch.uint8 if zone_dtype == 'uint8' else torch.int32
    zbuf = torch.zeros(off + m + 16, dtype=zt, device=dev)
    zones = zbuf[off:off + m]
    zones.copy_(torch.from_numpy(np.array(z).astype(zone_dtype if zone_dtype == 'uint8' else np.int32)))
    if kind == 'none':
        return vals, zones, {}
    if kind == 'row':
        return vals, zones, dict(area=torch.from_numpy(np.array(wr)).to(dev), cols=COLS, first_pixel=FIRST + lo, wmax=WMAX)
    wbuf = torch.zeros(off + m + 16, dtype=tdt, device=dev)
    area = wbuf[off:off + m]
    area.copy_(torch.from_numpy(np.array(wp[lo:hi])))
    return vals, zones, dict(area=area, wmax=WMAX)


def same(got, ref):
    assert got.values.dtype == ref.values.dtype and got.values.shape == ref.values.shape
    assert np.array_equal(got.weight, ref.weight)
    assert np.array_equal(bits_of(got.values), bits_of(ref.values))


# n, K, zones ('ldsN': the largest count the LDS table of N slots holds; '+1': one more), S, zone type, weights, bits, aligned
QUANTILE_CASES = [
    (1, 1, 1, 1, 'uint8', 'none', 8, False),
    (63, 3, 13, 3, 'uint8', 'row', 8, False),
    (4097, 3, 13, 3, 'uint8', 'pixel', 8, False),
    (70001, 3, 13, 3, 'uint8', 'row', 8, False),            # the LDS table, full, at every level
    (70001, 3, 13, 3, 'uint8', 'pixel', 8, True),           # ... with vector accesses
    (70001, 1, 13, 5, 'uint8', 'none', 8, True),            # five slots: the table in global memory from level 1
    (70001, 1, 'lds1', 1, 'int32', 'pixel', 8, False),
    (70001, 1, 'lds1+1', 1, 'int32', 'row', 8, True),
    (4097, 3, 'lds3+1', 3, 'uint8', 'none', 8, False),
    (70001, 3, 3000, 3, 'int32', 'row', 8, False),
    (4097, 1, 3000, 5, 'int32', 'pixel', 8, True),
    (4097, 3, 4, 1, 'uint8', 'row', 11, False),             # 11 bits: 4 x 2048 words in LDS
    (70001, 1, 1, 3, 'uint8', 'none', 11, True),
    (4097, 1, 13, 3, 'int32', 'pixel', 11, False),          # 11 bits, 13 zones: global
]


def zone_count(spec, nb):
    if isinstance(spec, int):
        return spec
    slots, _, more = spec[3:].partition('+')
    return lds_zones(int(slots), nb) + (1 if more else 0)


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('n,K,zones,S,zone_dtype,kind,bits,aligned', QUANTILE_CASES)
def test_quantiles_equal_the_definition(dtype, n, K, zones, S, zone_dtype, kind, bits, aligned):
    nzones = zone_count(zones, 1 << bits)
    x, z, wp, wr = inputs(dtype, n, K, nzones)
    vals, zt, kw = device_inputs(dtype, x, z, wp, wr, zone_dtype, kind, aligned)
    got = engine(dtype).zonal_quantiles(vals, zt, nzones, QS[S], bits=bits, **kw)
    same(got, oracle_quantiles(dtype, n, K, nzones, S, kind, bits))
    assert got.q == QS[S] and got.ew == (31 if kind == 'none' else 18)


HIST_CASES = [
    (1, 1, 1, 1, 'uint8', 'none', False),
    (63, 3, 13, 256, 'uint8', 'row', False),
    (4097, 3, 13, 1, 'uint8', 'pixel', False),
    (70001, 3, 13, 256, 'uint8', 'row', False),
    (70001, 3, 13, 256, 'uint8', 'pixel', True),
    (70001, 1, 1, 4094, 'uint8', 'none', True),             # 4096 words: the large LDS table
    (4097, 3, 13, 4094, 'int32', 'row', False),             # 13 x 4096 words: global
    (70001, 1, 'lds', 256, 'int32', 'pixel', False),
    (70001, 1, 'lds+1', 256, 'int32', 'row', True),
    (4097, 3, 3000, 256, 'int32', 'none', False),
]


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('n,K,zones,bins,zone_dtype,kind,aligned', HIST_CASES)
def test_histogram_equals_the_definition(dtype, n, K, zones, bins, zone_dtype, kind, aligned):
    nzones = zones if isinstance(zones, int) else lds_zones(1, bins + 2) + (zones == 'lds+1')
    x, z, wp, wr = inputs(dtype, n, K, nzones)
    vals, zt, kw = device_inputs(dtype, x, z, wp, wr, zone_dtype, kind, aligned)
    got = engine(dtype).zonal_histogram(vals, zt, nzones, bins, RANGE, **kw)
    assert got.ew == (31 if kind == 'none' else 18) and got.range == RANGE
    assert np.array_equal(got.cpu().numpy(), oracle_histogram(dtype, n, K, nzones, bins, kind))


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('cols', (1, 3))
def test_rows_narrower_than_a_vector(dtype, cols):
    """Per-row weights over rows of 1 and 3 pixels: a 16-byte vector of 2 or 4 values crosses a row end
    more than once. The range starts at raster pixel 2; 2051 pixels are several blocks, the last vector
    ragged; the weights are positive, (first_pixel + n - 1) // cols + 1 of them. The uniform histogram
    with 8 bins and the digit table of level 0 with bits = 8, word for word."""
    import torch
    from mod16_amd import _lib
    n, first, K, nzones = 2051, 2, 2, 5
    eng = engine(dtype)
    rng = np.random.default_rng(13)
    x = rng.normal(3.0, 2.0, (K, n)).astype(dtype)
    z = np.where(rng.random(n) < 0.2, rng.integers(0, nzones, n), (np.arange(n) // 29) % nzones)
    wr = 1e5 * (1.5 + np.cos(np.arange((first + n - 1) // cols + 1)))
    assert len(wr) == {1: 2053, 3: 685}[cols] and (wr > 0).all()
    kw = dict(weights=wr, cols=cols, first_pixel=first, wmax=WMAX)
    vals, zones, area = (torch.from_numpy(a).to(eng._dev()) for a in (x, z.astype(np.uint8), wr))
    got = eng.zonal_histogram(vals, zones, nzones, 8, RANGE, area=area, cols=cols, first_pixel=first, wmax=WMAX)
    want = Q.histogram(x, z, nzones, 8, *RANGE, **kw)
    assert want.sum() > 0 and np.array_equal(got.cpu().numpy(), want)
    spec = eng.ctx.zonal_hist_spec(eng.np_dtype, n, K, nzones, _lib.ZONE_U8, _lib.ZONAL_WEIGHT_ROW, cols, first, n, WMAX, 18,
                                   bits=8, level=0, slots=1)
    table = torch.zeros((K, nzones, 1, 256), dtype=torch.int64, device=eng._dev())
    eng.ctx.zonal_hist(spec, eng.np_dtype, vals.data_ptr(), zones.data_ptr(), area.data_ptr(), None, table.data_ptr(),
                       where=_lib.DEVICE, stream=eng._stream())
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), Q.digits(x, z, nzones, 0, 8, slots=1, **kw))


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('zmap,raster,nzones,S,bits', [
    ('blocks', 'constant', 13, 3, 8),           # every pixel of every level on one word per zone and slot
    ('single', 'constant', 1, 3, 8),
    ('single', 'constant', 5, 1, 11),
    ('blocks', 'pair', 13, 3, 8),               # the answer is decided by the last key bit
    ('noruns', 'pair', 13, 5, 11),
    ('noruns', 'random', 13, 3, 8),             # a zone map without runs
    ('noruns', 'random', 3000, 3, 8),
    ('single', 'random', 1, 3, 8),              # a single zone
    ('single', 'random', 40, 1, 8),
])
def test_special_rasters(dtype, zmap, raster, nzones, S, bits):
    n, K = 4097, 3
    x, z, wp, wr = inputs(dtype, n, K, nzones, zmap, raster)
    for kind in ('none', 'row'):
        vals, zt, kw = device_inputs(dtype, x, z, wp, wr, 'int32', kind)
        same(engine(dtype).zonal_quantiles(vals, zt, nzones, QS[S], bits=bits, **kw),
             oracle_quantiles(dtype, n, K, nzones, S, kind, bits, zmap, raster))
        got = engine(dtype).zonal_histogram(vals, zt, nzones, 256, RANGE, **kw)
        assert np.array_equal(got.cpu().numpy(), oracle_histogram(dtype, n, K, nzones, 256, kind, zmap, raster))
    if raster == 'constant':
        assert (oracle_quantiles(dtype, n, K, nzones, S, 'none', bits, zmap, raster).values[:, -1] == 2.5).all()


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('kind', ('none', 'row', 'pixel'))
def test_selection_is_order_independent_level_by_level(dtype, kind):
    """The digit table of every level, word for word: one add = two adds into one table = four parts
    dealt over two selections and merged = the pixels permuted (per-pixel weights permuted with them)."""
    import torch
    n, K, nzones, S, bits = 4097, 3, 13, 3, 8
    x, z, wp, wr = inputs(dtype, n, K, nzones)
    eng = engine(dtype)
    cuts = (0, 1001, 2300, 2301, n)
    whole = device_inputs(dtype, x, z, wp, wr, 'uint8', kind)
    parts = [device_inputs(dtype, x, z, wp, wr, 'uint8', kind, aligned=bool(i % 2), lo=cuts[i], hi=cuts[i + 1]) for i in range(4)]
    a, b, c, d = (eng.zonal_selection(K, nzones, QS[S], bits) for _ in range(4))
    perm = np.random.default_rng(1).permutation(n)
    shuffled = None
    if kind != 'row':
        shuffled = device_inputs(dtype, x[:, perm], z[perm], wp[perm], wr, 'uint8', kind)
    kw = weights_of(kind, wp, wr)
    prefix = None
    for level in range(a.levels):
        ref = Q.digits(x, z, nzones, level, bits, prefix, slots=S, **kw)
        a.add(whole[0], whole[1], **whole[2])
        assert np.array_equal(a.hist.cpu().numpy(), ref), level
        for i in (0, 1):                                   # two calls accumulating into one table ...
            b.add(parts[i][0], parts[i][1], **parts[i][2])
        for i in (2, 3):                                   # ... the rest on another selection, merged
            c.add(parts[i][0], parts[i][1], **parts[i][2])
        b.merge(c)
        assert np.array_equal(b.hist.cpu().numpy(), ref), level
        if shuffled is not None:
            d.add(shuffled[0], shuffled[1], **shuffled[2])
            assert np.array_equal(d.hist.cpu().numpy(), ref), level
        a.select()
        b.select()
        c.adopt(b)
        d.adopt(a)
        assert not a.hist.any().item() and a.level == level + 1
        prefix = a.prefix.cpu().numpy().view(np.uint64)
        assert np.array_equal(prefix, b.prefix.cpu().numpy().view(np.uint64))
        assert np.array_equal(a.remaining.cpu().numpy(), b.remaining.cpu().numpy())
    assert a.done and b.done and c.done
    ref = oracle_quantiles(dtype, n, K, nzones, S, kind, bits)
    same(a.result(), ref)
    same(b.result(), ref)
    same(c.result(), ref)
    with pytest.raises(ValueError):
        a.select()
    with pytest.raises(ValueError):
        a.add(whole[0], whole[1], **whole[2])
    with pytest.raises(ValueError):
        eng.zonal_selection(K, nzones, QS[S], bits).result()


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('kind', ('none', 'row', 'pixel'))
def test_histogram_accumulates_and_merges(dtype, kind):
    n, K, nzones, bins = 4097, 3, 13, 256
    x, z, wp, wr = inputs(dtype, n, K, nzones)
    eng = engine(dtype)
    cut = 1501
    first = device_inputs(dtype, x, z, wp, wr, 'uint8', kind, lo=0, hi=cut)
    second = device_inputs(dtype, x, z, wp, wr, 'uint8', kind, aligned=True, lo=cut, hi=n)
    acc = eng.zonal_histogram(first[0], first[1], nzones, bins, RANGE, **first[2])
    assert np.array_equal(acc.cpu().numpy(), oracle_histogram(dtype, n, K, nzones, bins, kind, lo=0, hi=cut))
    other = eng.zonal_histogram(second[0], second[1], nzones, bins, RANGE, **second[2])
    out = eng.zonal_histogram(second[0], second[1], nzones, bins, RANGE, acc=acc, **second[2])
    ref = oracle_histogram(dtype, n, K, nzones, bins, kind)
    assert out is acc and np.array_equal(acc.cpu().numpy(), ref)
    merged = Q.ZonalHistogram(oracle_histogram(dtype, n, K, nzones, bins, kind, lo=0, hi=cut), *RANGE, ew=acc.ew).merge(
        Q.ZonalHistogram(other.cpu().numpy(), *other.range, ew=other.ew))
    assert np.array_equal(merged.words, ref)


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('zone_dtype,kind', [('uint8', 'row'), ('int32', 'pixel'), ('uint16', 'none')])
def test_host_mode_equals_the_resident_calls_whatever_the_staging(dtype, zone_dtype, kind):
    """The numpy entry points: one tile = 16 staged tiles = the resident call = the definition."""
    import mod16_amd
    R, n, K, nzones, S, bits = 60, 60 * COLS, 2, 13, 3, 8
    x, z, wp, _ = inputs(dtype, n, K, nzones)
    wr = 1e5 * (1.5 + np.cos(np.arange(R)))
    area = {'none': None, 'row': wr, 'pixel': wp.reshape(R, COLS)}[kind]
    kw = {} if kind == 'none' else dict(wmax=WMAX)
    zones = np.where(z < nzones, z, 200).astype(zone_dtype).reshape(R, COLS)
    values = x.reshape(K, R, COLS)
    esz = np.dtype(dtype).itemsize
    narrow = zone_dtype == 'uint8'
    # a slot for 256 pixels: 4020 pixels are 16 tiles
    stage = (2 + (not narrow)) * 33 * 1024 + 512 + 300 * ((K + 1 + (not narrow)) * esz + narrow)
    ref_kw = {'none': {}, 'row': dict(weights=wr, cols=COLS, wmax=WMAX), 'pixel': dict(weights=wp, wmax=WMAX)}[kind]
    ref_q = Q.quantiles(x, z, nzones, QS[S], bits=bits, **ref_kw)
    ref_h = Q.histogram(x, z, nzones, 256, *RANGE, **ref_kw)
    for stage_bytes in (None, stage):
        got = mod16_amd.zonal_quantiles(values, zones, QS[S], nzones=nzones, area=area, bits=bits, stage_bytes=stage_bytes, **kw)
        same(got, ref_q)
        hist = mod16_amd.zonal_histogram(values, zones, 256, RANGE, nzones=nzones, area=area, stage_bytes=stage_bytes, **kw)
        assert np.array_equal(hist.words, ref_h) and hist.ew == (31 if kind == 'none' else 18)
        assert hist.counts.shape == (K, nzones, 256) and np.array_equal(hist.under, ref_h[..., 0])
    # accumulating two halves with acc=, and values without a layer axis
    half = R // 2
    part = lambda a, s: None if a is None else (a if np.ndim(a) == 0 else a[s])
    top = mod16_amd.zonal_histogram(values[:, :half], zones[:half], 256, RANGE, nzones=nzones, area=part(area, slice(0, half)), **kw)
    both = mod16_amd.zonal_histogram(values[:, half:], zones[half:], 256, RANGE, nzones=nzones, area=part(area, slice(half, R)), acc=top, **kw)
    assert np.array_equal(both.words, ref_h)
    flat = mod16_amd.zonal_quantiles(values[0], zones, 0.5, nzones=nzones, area=area, **kw)
    assert flat.values.shape == (nzones, 1) and flat.weight.shape == (nzones,)
    assert np.array_equal(bits_of(flat.values[:, 0]), bits_of(ref_q.values[0, :, 1]))
    # ... and the resident calls on the same arrays
    if zone_dtype != 'uint16':
        vals, zt, dkw = device_inputs(dtype, x, np.where(z < nzones, z, 200), wp, wr, zone_dtype, kind)
        if kind == 'row':
            dkw['first_pixel'] = 0
        same(engine(dtype).zonal_quantiles(vals, zt, nzones, QS[S], bits=bits, **dkw), ref_q)


def test_the_pre_pass_and_slab_groups():
    """wmax=None runs the zonal_bounds pre-pass; a small slab_bytes cuts the layers into groups."""
    dtype, n, K, nzones = 'float32', 4097, 3, 13
    x, z, wp, wr = inputs(dtype, n, K, nzones)
    w = np.where(np.isfinite(wp) & (wp >= 0), wp, 1.0).astype(np.float32)
    w[w > 2.2e5] = 2.2e5
    wmax = float(w.max())
    import torch
    eng = engine(dtype)
    vals, zt, _ = device_inputs(dtype, x, z, wp, wr, 'uint8', 'none')
    area = torch.from_numpy(w).to(eng._dev())
    ref = Q.quantiles(x, z, nzones, QS[3], weights=w, wmax=wmax)
    same(eng.zonal_quantiles(vals, zt, nzones, QS[3], area=area), ref)
    same(eng.zonal_quantiles(vals, zt, nzones, QS[3], area=area, wmax=wmax, slab_bytes=1), ref)         # one layer per group
    hist = eng.zonal_histogram(vals, zt, nzones, 64, RANGE, area=area)
    assert np.array_equal(hist.cpu().numpy(), Q.histogram(x, z, nzones, 64, *RANGE, weights=w, wmax=wmax))
    with pytest.raises(ValueError):
        eng.zonal_histogram(vals, zt, nzones, 64, RANGE, area=area, acc=hist)           # acc= needs wmax
    with pytest.raises(ValueError):
        eng.zonal_histogram(vals, zt, nzones, 64, RANGE, area=area, wmax=wmax * 4, acc=hist)      # another exponent
    with pytest.raises(ValueError):
        eng.zonal_histogram(vals, zt, nzones, 0, RANGE)
    with pytest.raises(ValueError):
        eng.zonal_histogram(vals, zt, nzones, 64, (1.0, 1.0))
    with pytest.raises(ValueError):
        eng.zonal_quantiles(vals, zt, nzones, 1.5)
    with pytest.raises(ValueError):
        eng.zonal_quantiles(vals, zt, nzones, 0.5, bits=13)
