"""GPU tests of upscaling from rasters with row-affine columns (mod16_upscale_create_rows and a rows handle
in mod16_upscale_f32 / _f64 / _classes / _sums_*: RasterEngine.upscale_grid(col_affine=...), UpscaleGrid.sums,
mod16_amd.upscale_fields / upscale_classes / upscale_sums) against the numpy definition (mod16_amd/upscale.py:
aggregate_rows, sums_rows, majority_rows, held to a per-pixel loop by tests/test_upscale_rows_host.py). Every
output must have the BITS of the definition: NaN at the same places, everything else equal as integers; the
definition is float64 arithmetic of correctly rounded operations in a fixed order and integer counts, and
which cell a pixel belongs to is decided by the same operations on both sides, so there is no tolerance.

The values follow the recipe of test_gpu_upscale.py: gamma(4, 5); per coarse column its own share of NaN,
0 ... 100 %; in coarse row 0 cell 1 of -0.0, cell 2 with +inf, cell 3 with +inf and -inf, cell 4 all NaN."""
import functools
import itertools

import numpy as np
import pytest

from mod16_amd import downscale as ds
from mod16_amd import upscale as up
import parity

pytestmark = pytest.mark.gpu

ALL, SUMS, CLASSES = up.OUTPUT_NAMES, up.SUM_NAMES, up.CLASS_OUTPUT_NAMES


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


def on_device(torch, x):
    return torch.from_numpy(np.array(x)).to(engine()._dev())


def host(res):
    return type(res)(*[None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for a in res])


def assert_same(got, want, what):
    got = host(got)
    assert type(got) is type(want), what
    for name, g, w in zip(type(want)._fields, got, want):
        if w is None:
            assert g is None, '%s: %s was produced' % (what, name)
            continue
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, '%s: %s %r %r' % (what, name, g.dtype, g.shape)
        if w.dtype.kind == 'f':
            assert parity.same_bits(g, w), '%s: %s differs at %d of %d places' % (
                what, name, int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum()), w.size)
        else:
            assert np.array_equal(g, w), '%s: %s differs at %d of %d places' % (what, name, int((g != w).sum()), w.size)


class Geometry(object):
    """A fine raster with row-affine columns over a coarse grid, and what the definition makes of it."""

    def __init__(self, shape, coarse_shape, row_pos, origin, scale, wrap=False, col_range=None, area=None):
        self.shape, self.coarse_shape, self.wrap = tuple(shape), tuple(coarse_shape), wrap
        self.row_pos = np.asarray(row_pos, np.float64)
        self.affine = (np.asarray(origin, np.float64), np.asarray(scale, np.float64))
        self.col_range = None if col_range is None else tuple(np.asarray(t, np.int32) for t in col_range)
        self.area = area
        H, W = self.coarse_shape
        self.rows = up.cell_runs(up.cell_table(self.row_pos, H), H)
        self.row_cell = up.cell_table(self.row_pos, H).astype(np.int64)
        self.col_cell = up.cell_table_rows(self.affine[0], self.affine[1], shape[1], W, wrap, self.col_range).astype(np.int64)
        self.runs = up.cell_runs_rows(self.col_cell, W)          # (raises unless every cell is one run per fine row)

    def kw(self):
        return dict(wrap=self.wrap, area=self.area, col_affine=self.affine, col_range=self.col_range)

    def grid(self):
        return engine().upscale_grid(self.shape, self.coarse_shape, self.row_pos, **self.kw())

    def fill(self, rng, K, dtype):
        H, W = self.coarse_shape
        R, C = self.shape
        v = rng.gamma(4.0, 5.0, (K, R, C))
        share = np.linspace(-0.1, 1.1, max(W, 2))[np.maximum(self.col_cell, 0)]
        v[rng.uniform(0, 1, (K, R, C)) < share[None]] = np.nan
        in0 = (self.row_cell == 0)[:, None]
        for j in range(1, 5):
            at = in0 & (self.col_cell == j)
            if not at.any():
                continue
            if j == 1:
                v[:, at] = -0.0
            elif j == 4:
                v[:, at] = np.nan
            else:
                v[:, at] = rng.gamma(4.0, 5.0, (K, int(at.sum())))
                r, c = np.argwhere(at)[0]
                v[:, r, c] = np.inf
                if j == 3:
                    r, c = np.argwhere(at)[-1]
                    v[:, r, c] = -np.inf
        v = v.astype(dtype)
        v.setflags(write=False)
        return v

    def mean(self, v, min_fraction=0.0, outputs=ALL):
        return up.aggregate_rows(v, self.rows, self.affine, self.coarse_shape[1], self.wrap, self.col_range, self.area,
                                 min_fraction, outputs)

    def sums(self, v, outputs=SUMS):
        return up.sums_rows(v, self.rows, self.affine, self.coarse_shape[1], self.wrap, self.col_range, self.area, outputs)

    def majority(self, cls, valid=None, outputs=CLASSES):
        return up.majority_rows(cls, self.rows, self.affine, self.coarse_shape[1], self.wrap, self.col_range, valid, outputs)


def rows_over(R, H, margin=0.0):
    """R fine rows spread over H coarse rows (and `margin` cells beyond both ends)"""
    return (np.arange(R) + 0.5) * (H + 2 * margin) / R - 0.5 - margin


@functools.lru_cache(maxsize=None)
def mixed(wrap):
    """(a) 37 x 150 over 5 x 9: scales 0.06 ... 0.3 of both signs, a zero scale, a row outside (no wrap) or
    with an empty range (wrap), ranges that keep a row from lapping (wrap), a cell across the end of the
    periodic axis (the rows whose origin is 6 and above, with positive scale)."""
    R, C, H, W = 37, 150, 5, 9
    rng = np.random.default_rng(11 + wrap)
    mag = rng.uniform(0.06, 0.3, R)
    scale = np.where(rng.uniform(size=R) < 0.5, -mag, mag)
    origin = np.where(scale > 0, rng.uniform(-1.5, 8.0, R), rng.uniform(1.0, 10.5, R))
    scale[5] = 0.0
    origin[5] = 3.25
    origin[9], scale[9] = -50.0, 0.06                            # no wrap: wholly outside
    origin[12], scale[12] = 6.0, 0.11                            # wrap: crosses W -> 0
    n = np.minimum(C, np.floor((W - 2) / np.maximum(np.abs(scale), 1e-9)).astype(np.int64) + 1)
    if not wrap:                                                 # whole rows but every fourth
        n[np.arange(R) % 4 != 0] = C
    first = np.array([rng.integers(0, C - k + 1) for k in n])
    first[12] = 0
    n[20] = 0                                                    # an empty range
    n[21], first[21] = 1, C - 1                                  # one pixel, the last column
    area = rng.uniform(0.2, 1.0, R)
    return Geometry((R, C), (H, W), rows_over(R, H, 0.3), origin, scale, wrap, (first, n), area)


def sinusoidal(h, v, size=48):
    """(d) a MODIS tile over the 361 x 576 reanalysis grid (0.5 x 0.625 degrees, north to south), on-globe columns"""
    row_pos, origin, scale = ds.sinusoidal_positions(h, v, size, 90.0, -0.5, -180.0, 0.625)
    return Geometry((size, size), (361, 576), row_pos, origin, scale, True, ds.sinusoidal_columns(h, v, size))


def run_all(torch, geo, v, min_fraction=0.5, what=''):
    grid = geo.grid()
    assert grid.col_runs is None and grid.col_affine is not None
    got = grid.run(on_device(torch, v), min_fraction=min_fraction, outputs=ALL)
    engine().check()
    assert_same(got, geo.mean(v, min_fraction), what)
    grid.close()


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_mixed_rows_have_the_bits_of_the_definition(env, dtype, wrap):
    torch, _ = env
    geo = mixed(wrap)
    assert (geo.runs.count.sum(axis=1) == 0).any() and (geo.affine[1] < 0).any() and (geo.affine[1] == 0).any()
    if wrap:
        r = 12                                                   # the row that crosses the end of the periodic axis
        cells = geo.col_cell[r][geo.col_cell[r] >= 0]
        assert cells[0] > cells[-1] and (np.diff(cells) < 0).sum() == 1
    v = geo.fill(np.random.default_rng(5), 3, dtype)
    want = geo.mean(v, 0.5)
    assert np.isnan(want.mean).any() and np.isfinite(want.mean).sum() > want.mean[0].size // 4
    assert np.isinf(v).any() and (want.count > 0).sum() > want.count.size // 2
    grid = geo.grid()
    dev = on_device(torch, v)
    for K in (1, 3):
        part = dev if K == 3 else dev[0]
        got = grid.run(part, min_fraction=0.5, outputs=ALL)
        engine().check()
        assert_same(got, up.Upscaled(*[a if K == 3 else a[0] for a in want]), 'mixed, %s, wrap %r, K = %d' % (dtype, wrap, K))
    got = grid.run(dev)                                          # the defaults: the mean alone, min_fraction 0
    engine().check()
    assert_same(got, geo.mean(v, 0.0, ('mean',)), 'defaults')
    grid.close()


def test_runs_longer_than_one_lds_span_beside_short_ones(env):
    """(b) 3 x 4500 over 1 x 3: a run of 4200 columns is carried over three chunks of kUpSpan = 2048
    (csrc/mod16_upscale.hpp) with a short run in the same block; a decreasing row; a row of 10-pixel cells."""
    torch, _ = env
    origin = np.array([-0.5, 2.4, -0.45])
    scale = np.array([1.0 / 4200, -1.0 / 2100, 0.1])
    geo = Geometry((3, 4500), (1, 3), np.zeros(3), origin, scale)
    assert geo.runs.count[0].tolist() == [4200, 300, 0] and geo.runs.count[1].max() > 2048 and geo.runs.count[2].max() == 10
    for dtype in ('float32', 'float64'):
        v = geo.fill(np.random.default_rng(77), 2, dtype)
        run_all(torch, geo, v, 0.25, 'long runs, %s' % dtype)
    cls = np.random.default_rng(3).integers(0, 4, geo.shape).astype(np.uint8)
    grid = geo.grid()
    got = grid.majority(on_device(torch, cls), outputs=CLASSES)
    engine().check()
    assert_same(got, geo.majority(cls), 'long runs, classes')


def quarter(H, W, R, wrap, seed):
    """(c) W cells of about four pixels: scale near 0.25 of both signs, origins that differ from row to row"""
    rng = np.random.default_rng(seed)
    C = 4 * W + 8
    scale = rng.uniform(0.245, 0.255, R) * np.where(rng.uniform(size=R) < 0.3, -1, 1)
    origin = np.where(scale > 0, rng.uniform(-1.2, 0.5, R), W - rng.uniform(-0.5, 1.2, R))
    col_range = None
    if wrap:
        n = np.minimum(C, np.floor((W - 2) / np.abs(scale)).astype(np.int64) + 1)
        col_range = (rng.integers(0, C - n + 1), n)
        origin = origin + rng.integers(-2, 3, R) * W + W / 2.0
    return Geometry((R, C), (H, W), rows_over(R, H), origin, scale, wrap, col_range, rng.uniform(0.2, 1.0, R))


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('W', [63, 65, 129, 300])
def test_both_sides_of_a_wave_and_several_spans(env, W, wrap):
    torch, _ = env
    geo = quarter(2, W, 5, wrap, W)
    assert geo.runs.count.max() >= 4 and (geo.runs.count.sum(axis=0) > 0).sum() >= W - 8
    v = geo.fill(np.random.default_rng(W), 2, 'float32')
    run_all(torch, geo, v, 0.5, 'W = %d, wrap %r' % (W, wrap))


@pytest.mark.parametrize('H,K,wrap', [(800, 1, False), (400, 3, True)])
def test_blocks_of_two_and_four_waves(env, H, K, wrap):
    """The launch halves its 256-lane blocks while fewer than 8 blocks per compute unit would exist: 800 coarse
    rows of 300 cells are 1600 blocks of 256 lanes but 2400 of 128, three layers of 400 rows 2400 of 256 (as in
    test_gpu_upscale.py): the exchange of the run boundaries and the block-wide minima then cross waves."""
    torch, _ = env
    geo = quarter(H, 300, H, wrap, H + K)
    v = geo.fill(np.random.default_rng(H), K, 'float32')
    run_all(torch, geo, v, 0.5, 'H = %d, K = %d' % (H, K))
    if K == 1:
        cls = np.random.default_rng(K).integers(0, 3, geo.shape).astype(np.uint8)
        grid = geo.grid()
        got = grid.majority(on_device(torch, cls), outputs=CLASSES)
        engine().check()
        assert_same(got, geo.majority(cls), 'classes')


@pytest.mark.parametrize('tile', [(17, 0), (35, 9), (11, 2)])
def test_real_tiles_over_the_reanalysis_grid(env, tile):
    """(d) polar rows (a scale of about 180 cells per pixel: one pixel per touched cell), the tile at the date
    line, a mid-latitude tile; fields and classes (g)."""
    torch, _ = env
    geo = sinusoidal(*tile)
    if tile == (17, 0):
        assert np.abs(geo.affine[1]).max() > 100 and geo.runs.count.max() == 1
    if tile == (35, 9):
        assert geo.col_cell.max() >= 574 and geo.col_range[1].min() < 48
    for dtype in ('float32', 'float64'):
        v = geo.fill(np.random.default_rng(sum(tile)), 2, dtype)
        run_all(torch, geo, v, 0.5, 'tile %r, %s' % (tile, dtype))
    cls = np.random.default_rng(7).integers(0, 14, geo.shape).astype(np.uint8)
    grid = geo.grid()
    got = grid.majority(on_device(torch, cls), outputs=CLASSES)
    engine().check()
    want = geo.majority(cls)
    assert (want.cls != 255).sum() > 100 and (want.share > 0).any()
    assert_same(got, want, 'tile %r, classes' % (tile,))


def test_ties_go_to_the_far_cell_on_the_device_as_on_the_host(env):
    """(e) origin -0.5, scale 0.25: every fourth pixel lies exactly between two cells, f == 0.5."""
    torch, _ = env
    R, C, H, W = 9, 40, 3, 7
    for sign, wrap in itertools.product((1, -1), (False, True)):
        origin = np.full(R, -0.5 if sign > 0 else 7.5)
        n = 21 if wrap else C                                    # (wrap: 0.25 * 20 = 5 = W - 2)
        geo = Geometry((R, C), (H, W), rows_over(R, H), origin, np.full(R, 0.25 * sign), wrap,
                       (np.full(R, 3), np.full(R, n)) if wrap else None)
        pos = origin[0] + 0.25 * sign * np.arange(C)
        tie = np.flatnonzero(pos - np.floor(pos) == 0.5)
        assert tie.size >= 9 and all(geo.col_cell[0, c] in (-1, int(np.floor(pos[c]) + 1) % (W if wrap else 99)) for c in tie)
        v = geo.fill(np.random.default_rng(1), 2, 'float64')
        run_all(torch, geo, v, 0.0, 'ties, sign %d, wrap %r' % (sign, wrap))


def test_majority_on_the_mixed_rows(env):
    torch, _ = env
    for wrap in (False, True):
        geo = mixed(wrap)
        rng = np.random.default_rng(50 + wrap)
        cls = rng.choice(np.array([0, 1, 2, 12, 13, 31, 32, 254, 255], np.uint8), geo.shape)
        cls[:, :50] = rng.integers(0, 2, (geo.shape[0], 50))     # two codes: ties
        grid = geo.grid()
        for valid in (None, (1, 13, 31)):
            got = grid.majority(on_device(torch, cls), valid=valid, outputs=CLASSES)
            engine().check()
            assert_same(got, geo.majority(cls, valid), 'classes, wrap %r, valid %r' % (wrap, valid))
        only = grid.majority(on_device(torch, cls))
        engine().check()
        assert only.share is None
        assert_same(only, geo.majority(cls, outputs=('cls',)), 'the class alone')
        grid.close()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_strided_arrays_at_an_odd_offset_every_subset_and_the_refusals(env, dtype):
    """(f)"""
    torch, _ = env
    eng = engine()
    geo = mixed(True)
    K, (R, C), (H, W) = 3, geo.shape, geo.coarse_shape
    v = geo.fill(np.random.default_rng(8), K, dtype)
    want, wsum = geo.mean(v, 0.5), geo.sums(v)
    tdtype = getattr(torch, dtype)
    dev = eng._dev()

    def strided(rows, cols, kind, fill, pad=3, gap=11):
        plane = rows * (cols + pad) + gap
        b = torch.full((K * plane + 1,), fill, dtype=kind, device=dev)
        return b, b[1:].view(K, plane)[:, :rows * (cols + pad)].view(K, rows, cols + pad)[:, :, :cols]

    vbuf, values = strided(R, C, tdtype, float('nan'))
    values.copy_(on_device(torch, v))
    kinds = dict(mean=tdtype, fraction=tdtype, count=torch.int32, num=torch.float64, den=torch.float64, tot=torch.float64)
    bufs, outs = {}, {}
    for k, kind in kinds.items():
        bufs[k], outs[k] = strided(H, W, kind, 0, pad=5, gap=7)
    grid = geo.grid()
    got = grid.run(values, min_fraction=0.5, outputs=ALL, out={k: outs[k] for k in ALL})
    eng.check()
    assert all(got[i] is outs[k] for i, k in enumerate(ALL))
    assert_same(got, want, 'strided, %s' % dtype)
    got = grid.sums(values, out={k: outs[k] for k in SUMS})
    eng.check()
    assert_same(got, wsum, 'strided sums, %s' % dtype)
    for k in kinds:                                              # the guard elements
        plane = H * (W + 5) + 7
        assert float(bufs[k][0]) == 0
        layers = bufs[k][1:].view(K, plane)
        assert bool((layers[:, H * (W + 5):] == 0).all()), k
        assert bool((layers[:, :H * (W + 5)].view(K, H, W + 5)[:, :, W:] == 0).all()), k
    for r in range(1, 3):
        for names in itertools.combinations(ALL, r):
            got = grid.run(values, min_fraction=0.5, outputs=names)
            eng.check()
            assert_same(got, up.Upscaled(*[a if k in names else None for k, a in zip(ALL, want)]), repr(names))
    for r in range(1, 4):
        for names in itertools.combinations(SUMS, r):
            got = grid.sums(values, outputs=names)
            eng.check()
            assert_same(got, up.UpscaledSums(*[a if k in names else None for k, a in zip(SUMS, wsum)]), repr(names))
    on_input = vbuf[1:1 + K * H * W].view(K, H, W)
    with pytest.raises(ValueError, match='overlaps'):
        grid.run(values, outputs=('mean',), out=dict(mean=on_input))
    with pytest.raises(ValueError, match='overlaps'):
        grid.run(values, outputs=('mean', 'fraction'), out=dict(mean=outs['mean'], fraction=outs['mean']))
    if dtype == 'float64':
        with pytest.raises(ValueError, match='overlaps'):
            grid.sums(values, outputs=('num',), out=dict(num=on_input))
    with pytest.raises(ValueError, match='overlaps'):
        grid.sums(values, outputs=('num', 'tot'), out=dict(num=outs['num'], tot=outs['num']))
    with pytest.raises(ValueError, match='shape'):
        grid.sums(values[:, :R - 1])
    grid.close()
    with pytest.raises(ValueError, match='closed'):
        grid.sums(values)


def test_sums_of_both_geometries_and_the_merge_of_two_tiles(env):
    """(h) the rectilinear sums kernel; two tiles of dyadic geometry and small integers (every sum exact) merge
    to the bits of the mosaic's means."""
    torch, _ = env
    eng = engine()
    R, C, H, W = 12, 150, 4, 9
    rng = np.random.default_rng(31)
    row_pos = rows_over(R, H)
    origin, scale = np.full(R, -0.375) + 0.5 * (np.arange(R) % 3), np.full(R, 0.125)
    area = 2.0 ** -rng.integers(0, 3, R)
    for wrap in (False, True):
        n = 57 if wrap else C                                    # (wrap: 0.125 * 56 = 7 = W - 2)
        rng_cols = (np.zeros(R, np.int32), np.full(R, n, np.int32))
        mosaic = Geometry((R, C), (H, W), row_pos, origin, scale, wrap, rng_cols, area)
        v = rng.integers(0, 50, (2, R, C)).astype(np.float32)
        v[rng.uniform(size=v.shape) < 0.2] = np.nan
        want = mosaic.mean(v, 0.5)
        half = 24
        parts = []
        for c0, c1 in ((0, half), (half, C)):
            cols = (np.zeros(R, np.int32), np.full(R, max(0, min(n, c1) - c0), np.int32))
            tile = Geometry((R, c1 - c0), (H, W), row_pos, origin + scale * c0, scale, wrap, cols, area)
            grid = tile.grid()
            s = grid.sums(on_device(torch, v[:, :, c0:c1].copy()))
            eng.check()
            assert_same(s, tile.sums(v[:, :, c0:c1]), 'tile sums, wrap %r' % wrap)
            parts.append(host(s))
            grid.close()
        assert_same(up.merge(parts, 0.5, np.float32), want, 'merge, wrap %r' % wrap)
        assert_same(up.merge(parts[::-1], 0.5, np.float32), want, 'merge, the other order (exact sums)')
    # the rectilinear geometry: the same positions as a col_pos table
    col_pos = ds.column_positions(origin[:1], scale[:1], C)[0]
    rows, cols = up.cell_runs(up.cell_table(row_pos, H), H), up.cell_runs(up.cell_table(col_pos, W), W)
    grid = eng.upscale_grid((R, C), (H, W), row_pos, col_pos, area=area)
    assert grid.col_affine is None and grid.col_runs is not None
    for dtype in ('float32', 'float64'):
        x = (rng.gamma(4.0, 5.0, (2, R, C))).astype(dtype)
        x[rng.uniform(size=x.shape) < 0.2] = np.nan
        got = grid.sums(on_device(torch, x))
        eng.check()
        assert_same(got, up.sums(x, rows, cols, area), 'rectilinear sums, %s' % dtype)
        assert_same(up.merge([host(got)], 0.25, dtype), up.aggregate(x, rows, cols, area, 0.25), 'merge of one is aggregate')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_host_mode_any_stage_bytes_gives_the_same_bits(env, dtype):
    """(i) one coarse row of one layer per pass, two coarse rows, one band"""
    _, mod16_amd = env
    geo = mixed(False)
    K, (R, C), (H, W) = 3, geo.shape, geo.coarse_shape
    v = geo.fill(np.random.default_rng(9), K, dtype)
    want, wsum = geo.mean(v, 0.5), geo.sums(v)
    esz = v.dtype.itemsize
    tallest = int(geo.rows.count.max())
    coarse_row = tallest * C * esz + W * 28 + 4 * 256
    kw = dict(wrap=False, area=geo.area, col_affine=geo.affine, col_range=geo.col_range)
    cls = np.random.default_rng(9).integers(0, 16, (R, C)).astype(np.uint8)
    cwant = geo.majority(cls, (1, 2, 3, 14, 15))
    for stage in (1, 3 * 2 * coarse_row + 4096, None):
        got = mod16_amd.upscale_fields(v, (H, W), geo.row_pos, min_fraction=0.5, outputs=ALL, stage_bytes=stage, **kw)
        assert_same(got, want, 'HOST mode, stage_bytes = %r' % stage)
        got = mod16_amd.upscale_sums(v, (H, W), geo.row_pos, stage_bytes=stage, **kw)
        assert_same(got, wsum, 'HOST mode sums, stage_bytes = %r' % stage)
        got = mod16_amd.upscale_classes(cls, (H, W), geo.row_pos, valid=(1, 2, 3, 14, 15), outputs=CLASSES, stage_bytes=stage,
                                        wrap=False, col_affine=geo.affine, col_range=geo.col_range)
        assert_same(got, cwant, 'HOST mode classes, stage_bytes = %r' % stage)
    some = mod16_amd.upscale_sums(v[0], (H, W), geo.row_pos, outputs=('tot', 'count'), stage_bytes=1, **kw)
    assert some.num is None and some.tot.shape == (H, W)
    assert_same(some, geo.sums(v[0], ('tot', 'count')), 'one plane, a subset')


def test_refusals(env):
    """(j) and what only the library can refuse"""
    torch, _ = env
    eng = engine()
    geo = mixed(True)
    with pytest.raises(ValueError, match='col_affine'):
        eng.upscale_grid(geo.shape, geo.coarse_shape, geo.row_pos, np.zeros(geo.shape[1]), col_affine=geo.affine)
    with pytest.raises(ValueError, match='col_affine'):
        eng.upscale_grid(geo.shape, geo.coarse_shape, geo.row_pos)
    with pytest.raises(ValueError, match='fine row 3 may lap'):
        eng.upscale_grid((4, 100), (2, 9), np.zeros(4), wrap=True, col_affine=(np.zeros(4), np.array([0.01, 0.01, 0.01, 0.08])))
    from mod16_amd import _lib
    spec = _lib.UpscaleSpec(4, 100, 2, 9, 1, 0)
    handle = _lib.C.c_void_p()
    rf, rc = np.array([0, 2], np.int32), np.array([2, 2], np.int32)
    origin, scale = np.zeros(4), np.array([0.01, 0.01, 0.01, 0.08])
    rcode = eng.ctx.lib.mod16_upscale_create_rows(eng.ctx.handle, _lib.C.byref(spec), rf.ctypes.data, rc.ctypes.data, origin.ctypes.data,
                                                  scale.ctypes.data, None, None, None, _lib.C.byref(handle))
    assert rcode != 0 and not handle.value
    with pytest.raises(_lib.Mod16Error, match='mod16_upscale_create_rows: a fine row may lap'):
        eng.ctx.check(rcode)
