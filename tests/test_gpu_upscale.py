"""GPU tests of upscaling (mod16_upscale_f32 / _f64 / _classes: RasterEngine.upscale_grid,
mod16_amd.upscale_fields / upscale_classes) against the numpy definition (mod16_amd/upscale.py, itself
held to known answers, numpy's nanmean and its bit-level properties by tests/test_upscale_host.py). Every
output must have the BITS of the definition: NaN at the same places, everything else equal as integers.
The definition is float64 arithmetic of correctly rounded operations in a fixed order and integer
counts, so there is no tolerance anywhere.

Cells (rows x columns of fine pixels): 1 x 1, 2 x 2, 3 x 5, 1 x 12 and 12 x 12 (12 elements between the
LDS reads of neighbouring lanes: the distance that is 4-way without the padding), runs of 7 and 8 mixed
on both axes, 40 x 1, and column runs of 4500 and 5000 pixels -- longer than kUpSpan = 2048, the
elements of a fine row a block holds in LDS at a time (csrc/mod16_upscale.hpp), so the run is carried over
three chunks, once together with short runs in the same block. W in (1, 63, 65, 129, 300): one cell, both
sides of a wave -- these grids being small the launch stays at one wave per block, so there are several
blocks per coarse row from 65; blocks of two and four waves have a test of their own --, H in (1, 3), K
in (1, 3). The raster of a cell shape is
made once for 3 layers of 3 x 300 cells and its definition computed once; the smaller grids are its
first layers, rows and columns (cells are independent), passed as strided views, whose launches differ.

Per pixel, from a seeded generator: gamma(4, 5); its cell's own share of NaN, 0 ... 100 % across the
cells of a row, so that the valid count crosses min_fraction within one launch; cell 1 of -0.0, cell 2
with +inf, cell 3 with +inf and -inf, cell 4 all NaN."""
import functools
import itertools

import numpy as np
import pytest

from mod16_amd import upscale as up
import parity

pytestmark = pytest.mark.gpu

WIDTHS = (1, 63, 65, 129, 300)
HEIGHTS = (1, 3)
LAYERS = (1, 3)
KMAX, HMAX, WMAX = 3, 3, 300
ALL = up.OUTPUT_NAMES
SHAPES = {'1x1': (1, 1), '2x2': (2, 2), '3x5': (3, 5), '1x12': (1, 12), '12x12': (12, 12), '7/8': ((7, 8), (7, 8)),
          '40x1': (40, 1)}


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


def counts(per, cells):
    """the run lengths of `cells` cells: all `per`, or a tuple of lengths taken in turn"""
    per = per if isinstance(per, tuple) else (per,)
    return tuple(per[k % len(per)] for k in range(cells))


def axis(lengths, margin=0, reverse=False, roll=0):
    """The cell of every fine index of an axis whose cells have these run lengths, with `margin` pixels
    outside the grid at both ends, the order reversed, or (a periodic axis) rolled so that the first
    `roll` pixels of cell 0 lie at the end. -> float64 positions: the cell's centre, -3 outside."""
    cells = np.repeat(np.arange(len(lengths)), lengths)
    cells = np.concatenate([np.full(margin, -3), cells, np.full(margin, -3)])
    if reverse:
        cells = cells[::-1]
    return np.roll(cells, -roll).astype(np.float64)


def cell_ids(pos, size, wrap=False):
    return up.cell_table(pos, size, wrap).astype(np.int64)


def fill(rng, K, row_pos, col_pos, H, W, wrap, dtype):
    """(K, R, C) values by the recipe of the module docstring, read-only"""
    ri, ci = cell_ids(row_pos, H), cell_ids(col_pos, W, wrap)
    R, C = ri.size, ci.size
    v = rng.gamma(4.0, 5.0, (K, R, C))
    share = np.linspace(-0.1, 1.1, max(W, 2))[np.maximum(ci, 0)]         # per cell of a row: 0 % ... 100 %
    v[rng.uniform(0, 1, (K, R, C)) < share[None, None, :]] = np.nan
    r0 = np.flatnonzero(ri == 0)                                         # the fine rows of coarse row 0: the special cells
    for j in range(1, 5) if r0.size else ():
        c = np.flatnonzero(ci == j)
        if not c.size:
            continue
        at = (slice(None), r0[:, None], c[None, :])
        if j == 1:
            v[at] = -0.0
        elif j == 4:
            v[at] = np.nan
        else:
            v[at] = rng.gamma(4.0, 5.0, (K, r0.size, c.size))
            v[:, r0[0], c[0]] = np.inf
            if j == 3:
                v[:, r0[-1], c[-1]] = -np.inf                            # (a 1 x 1 cell: -inf alone)
    v = v.astype(dtype)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def shape_case(name, dtype):
    """(row_pos, col_pos, values (3, R, C), area, the definition for min_fraction 0.5) of a cell shape"""
    fr, fc = SHAPES[name]
    row_pos, col_pos = axis(counts(fr, HMAX)), axis(counts(fc, WMAX))
    rng = np.random.default_rng(sorted(SHAPES).index(name))
    v = fill(rng, KMAX, row_pos, col_pos, HMAX, WMAX, False, dtype)
    area = rng.uniform(0.2, 1.0, row_pos.size)
    rows, cols = (up.cell_runs(up.cell_table(p, s), s) for p, s in ((row_pos, HMAX), (col_pos, WMAX)))
    want = up.aggregate(v, rows, cols, area=area, min_fraction=0.5, outputs=ALL)
    for a in want:
        a.setflags(write=False)
    return row_pos, col_pos, v, area, want


def host(res):
    return type(res)(*[None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for a in res])


def assert_same(got, want, what):
    got = host(got)
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


def on_device(torch, x):
    return torch.from_numpy(np.array(x)).to(engine()._dev())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_every_cell_shape_and_grid_size_has_the_bits_of_the_definition(env, name, dtype):
    torch, _ = env
    eng = engine()
    row_pos, col_pos, v, area, want = shape_case(name, dtype)
    fr, fc = SHAPES[name]
    if min(counts(fc, 5)) >= 2:
        assert want.count[0, 0, 1] == fr * fc if isinstance(fr, int) else True
        assert want.mean[0, 0, 1] == 0 and not np.signbit(want.mean[0, 0, 1])        # the cell of -0.0
        assert want.mean[0, 0, 2] == np.inf and np.isnan(want.mean[0, 0, 3]) and want.count[0, 0, 3] > 0
    assert want.count[:, 0, 4].max() == 0                                # the cell that is all NaN
    assert np.isnan(want.mean).any() and np.isfinite(want.mean).sum() > want.mean.size // 4
    dev = on_device(torch, v)
    for H, W in itertools.product(HEIGHTS, WIDTHS):
        R, C = sum(counts(fr, H)), sum(counts(fc, W))
        grid = eng.upscale_grid((R, C), (H, W), row_pos[:R], col_pos[:C], area=area[:R])
        for K in LAYERS:
            part = dev[:K, :R, :C] if K > 1 else dev[0, :R, :C]            # a view: the strides stay the large raster's
            got = grid.run(part, min_fraction=0.5, outputs=ALL)
            eng.check()
            sub = up.Upscaled(*[a[:K, :H, :W] if K > 1 else a[0, :H, :W] for a in want])
            assert_same(got, sub, '%s, H = %d, W = %d, K = %d' % (name, H, W, K))
        grid.close()


def test_a_run_longer_than_one_lds_span(env):
    """4500 and 5000 columns exceed kUpSpan = 2048 (csrc/mod16_upscale.hpp): the lane carries its row sum
    over three chunks, with a 3-pixel cell between the long ones in the same block; 2 and 1 rows."""
    torch, _ = env
    eng = engine()
    row_pos, col_pos = axis((2, 1)), axis((4500, 3, 5000))
    rows, cols = up.cell_runs(up.cell_table(row_pos, 2), 2), up.cell_runs(up.cell_table(col_pos, 3), 3)
    assert max(cols.count) > 2 * 2048
    for dtype in ('float32', 'float64'):
        v = fill(np.random.default_rng(77), 2, row_pos, col_pos, 2, 3, False, dtype)
        grid = eng.upscale_grid(v.shape[1:], (2, 3), row_pos, col_pos)
        got = grid.run(on_device(torch, v), outputs=ALL)
        eng.check()
        assert_same(got, up.aggregate(v, rows, cols, outputs=ALL), 'long runs, %s' % dtype)


@pytest.mark.parametrize('H,K,roll', [(800, 1, 0), (400, 3, 0), (400, 3, 1)])
def test_blocks_of_two_and_four_waves(env, H, K, roll):
    """The launch halves its 256-lane blocks while fewer than 8 blocks per compute unit (256 of them) would
    exist: 800 coarse rows of 300 cells are 1600 blocks of 256 lanes but 2400 of 128, three layers of 400
    rows 2400 blocks of 256 -- the block-wide minimum and sum then cross waves. 2 x 3 cells; rolled by one
    pixel, the first block of every row holds the straddling cell and takes the path with gaps."""
    torch, _ = env
    eng = engine()
    W = 300
    row_pos, col_pos = axis((2,) * H), axis((3,) * W, roll=roll)
    rows, cols = up.cell_runs(up.cell_table(row_pos, H), H), up.cell_runs(up.cell_table(col_pos, W, roll > 0), W, roll > 0)
    rng = np.random.default_rng(H + K)
    v = fill(rng, K, row_pos, col_pos, H, W, roll > 0, 'float32')
    area = rng.uniform(0.2, 1.0, row_pos.size)
    grid = eng.upscale_grid(v.shape[1:], (H, W), row_pos, col_pos, wrap=roll > 0, area=area)
    got = grid.run(on_device(torch, v), min_fraction=0.5, outputs=ALL)
    eng.check()
    assert_same(got, up.aggregate(v, rows, cols, area=area, min_fraction=0.5, outputs=ALL, wrap=roll > 0), 'H = %d, K = %d' % (H, K))
    if K == 1:
        cls = rng.integers(0, 3, v.shape[1:]).astype(np.uint8)
        got = grid.majority(on_device(torch, cls), outputs=('cls', 'share'))
        eng.check()
        assert_same(got, up.majority(cls, rows, cols, wrap=roll > 0), 'classes')


GEOMETRIES = {
    # name: (row lengths, column lengths, kwargs of the rows, of the columns, wrap)
    'wrap': ((3, 2), (6,) * 70, {}, dict(roll=2), True),                     # cell 0 straddles the end of the axis
    'wrap-long': ((1,), (5000, 4200, 7), {}, dict(roll=4999), True),        # ... with a run longer than the LDS span
    'decreasing': ((7, 8, 7), (3,) * 67, dict(reverse=True), {}, False),
    'decreasing-columns': ((2, 2), (5,) * 130, {}, dict(reverse=True), False),
    'margin': ((2, 3), (4,) * 66, dict(margin=3), dict(margin=5), False),    # fine pixels outside the grid
    'empty': ((2, 0, 3), (3, 0) * 40 + (2,), {}, {}, False),                 # an empty coarse row and empty coarse columns
    'nothing': ((0, 0), (0,) * 5, dict(margin=2), dict(margin=3), False),    # every cell empty
}


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_geometries(env, name):
    torch, _ = env
    eng = engine()
    rl, cl, rkw, ckw, wrap = GEOMETRIES[name]
    row_pos, col_pos = axis(rl, **rkw), axis(cl, **ckw)
    H, W = len(rl), len(cl)
    rows = up.cell_runs(up.cell_table(row_pos, H), H)
    cols = up.cell_runs(up.cell_table(col_pos, W, wrap), W, wrap)
    assert sorted(rows.count) == sorted(rl) and sorted(cols.count) == sorted(cl)
    if wrap:
        assert cols.first[0] + cols.count[0] > col_pos.size
    rng = np.random.default_rng(len(name))
    area = rng.uniform(0.2, 1.0, row_pos.size)
    for dtype, K in (('float32', 2), ('float64', 1)):
        v = fill(rng, K, row_pos, col_pos, H, W, wrap, dtype)
        grid = eng.upscale_grid(v.shape[1:], (H, W), row_pos, col_pos, wrap=wrap, area=area)
        assert np.array_equal(grid.col_runs.first, cols.first) and np.array_equal(grid.row_runs.count, rows.count)
        got = grid.run(on_device(torch, v), min_fraction=0.25, outputs=ALL)
        eng.check()
        assert_same(got, up.aggregate(v, rows, cols, area=area, min_fraction=0.25, outputs=ALL, wrap=wrap), '%s, %s' % (name, dtype))
        cls = np.random.default_rng(3).integers(0, 4, v.shape[1:]).astype(np.uint8)      # four codes: heavy ties
        got = grid.majority(on_device(torch, cls), outputs=('cls', 'share'))
        eng.check()
        assert_same(got, up.majority(cls, rows, cols, wrap=wrap), '%s, classes' % name)


def test_area_min_fraction_and_every_subset_of_the_outputs(env):
    torch, _ = env
    eng = engine()
    row_pos, col_pos, v, area, _ = shape_case('7/8', 'float32')
    rows, cols = (up.cell_runs(up.cell_table(p, s), s) for p, s in ((row_pos, HMAX), (col_pos, WMAX)))
    dev = on_device(torch, v)
    for weights in (None, area):
        grid = eng.upscale_grid(v.shape[1:], (HMAX, WMAX), row_pos, col_pos, area=weights)
        for mf in (0.0, 0.5, 1.0):
            want = up.aggregate(v, rows, cols, area=weights, min_fraction=mf, outputs=ALL)
            got = grid.run(dev, min_fraction=mf, outputs=ALL)
            eng.check()
            assert_same(got, want, 'area %s, min_fraction %r' % (weights is not None, mf))
        assert np.isnan(want.mean[want.fraction < 1]).all() and np.isfinite(want.mean[want.fraction == 1]).any()
        for r in range(1, 4):
            for names in itertools.combinations(ALL, r):
                got = grid.run(dev, min_fraction=1.0, outputs=names)
                eng.check()
                assert_same(got, up.Upscaled(*[a if k in names else None for k, a in zip(ALL, want)]), repr(names))
    got = grid.run(dev)                                                      # the defaults: the mean alone, min_fraction 0
    eng.check()
    assert got.fraction is None and got.count is None
    assert_same(got, up.aggregate(v, rows, cols, area=area, outputs=('mean',)), 'defaults')


def test_output_subsets_leave_the_other_arrays_alone(env):
    """mean alone; fraction and count: what is not requested keeps its sentinel (the C ABI directly)."""
    torch, _ = env
    from mod16_amd import _lib
    eng = engine()
    row_pos, col_pos, v, area, want = shape_case('3x5', 'float64')
    grid = eng.upscale_grid(v.shape[1:], (HMAX, WMAX), row_pos, col_pos, area=area)
    values = on_device(torch, v)
    dev = eng._dev()
    shape = (KMAX, HMAX, WMAX)
    buf = dict(mean=torch.full(shape, -7.0, dtype=torch.float64, device=dev),
               fraction=torch.full(shape, -7.0, dtype=torch.float64, device=dev),
               count=torch.full(shape, -7, dtype=torch.int32, device=dev))
    R, C = v.shape[1:]
    done = set()
    for names in (('mean',), ('fraction', 'count')):
        grid._grid.run(np.dtype('float64'), values.data_ptr(), KMAX, R * C, C, 0.5,
                       [(buf[k].data_ptr(), HMAX * WMAX, WMAX) if k in names else None for k in ALL],
                       where=_lib.DEVICE, stream=eng._stream())
        eng.check()
        done |= set(names)
        for k in ALL:
            if k in done:
                got = buf[k].cpu().numpy()
                assert parity.same_bits(got, getattr(want, k)) if k != 'count' else np.array_equal(got, want.count), (names, k)
            else:
                assert bool((buf[k] == -7).all()), (names, k)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_strided_arrays_at_an_odd_offset_on_another_stream(env, dtype):
    torch, _ = env
    eng = engine()
    row_pos, col_pos, v, area, want = shape_case('7/8', dtype)
    K, H, W = 3, 3, 129
    R, C = sum(counts((7, 8), H)), sum(counts((7, 8), W))
    want = up.Upscaled(*[a[:K, :H, :W] for a in want])
    tdtype = getattr(torch, dtype)
    dev = eng._dev()

    def strided(rows, cols, kind, fill, pad=3, gap=11):
        """(buffer, its (K, rows, cols) view one element in: rows cols + pad apart, layers a plane + gap)"""
        plane = rows * (cols + pad) + gap
        b = torch.full((K * plane + 1,), fill, dtype=kind, device=dev)
        return b, b[1:].view(K, plane)[:, :rows * (cols + pad)].view(K, rows, cols + pad)[:, :, :cols]

    vbuf, values = strided(R, C, tdtype, float('nan'))
    values.copy_(on_device(torch, v[:K, :R, :C].copy()))
    kinds = dict(mean=tdtype, fraction=tdtype, count=torch.int32)
    bufs, outs = {}, {}
    for k, kind in kinds.items():
        bufs[k], outs[k] = strided(H, W, kind, 0, pad=5, gap=7)
    grid = eng.upscale_grid((R, C), (H, W), row_pos[:R], col_pos[:C], area=area[:R])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = grid.run(values, min_fraction=0.5, outputs=ALL, out=outs)
    side.synchronize()
    eng.check()
    assert all(got[i] is outs[k] for i, k in enumerate(ALL))
    assert_same(got, want, 'strided, %s' % dtype)
    for k in kinds:                                        # the guard elements: in front, between the rows, between the layers
        plane = H * (W + 5) + 7
        assert float(bufs[k][0]) == 0
        layers = bufs[k][1:].view(K, plane)
        assert bool((layers[:, H * (W + 5):] == 0).all()), k
        assert bool((layers[:, :H * (W + 5)].view(K, H, W + 5)[:, :, W:] == 0).all()), k
    on_input = vbuf[1:1 + K * H * W].view(K, H, W)
    with pytest.raises(ValueError, match='overlaps'):
        grid.run(values, outputs=('mean',), out=dict(mean=on_input))
    with pytest.raises(ValueError, match='overlaps'):
        grid.run(values, outputs=('mean', 'fraction'), out=dict(mean=outs['mean'], fraction=outs['mean']))
    with pytest.raises(ValueError, match='unit stride'):
        grid.run(values.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match='shape'):
        grid.run(values[:, :R - 1])
    with pytest.raises(ValueError, match='exactly the fields'):
        grid.run(values, outputs=('mean',), out=outs)
    with pytest.raises(ValueError, match='col_affine'):
        eng.upscale_grid((R, C), (H, W), row_pos[:R], col_pos[:C], col_affine=(np.zeros(R), np.ones(R)))
    grid.close()
    with pytest.raises(ValueError, match='closed'):
        grid.run(values)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_host_mode_any_stage_bytes_and_both_entry_points_agree(env, dtype):
    torch, mod16_amd = env
    row_pos, col_pos, v, area, want = shape_case('7/8', dtype)
    R, C = v.shape[1:]
    esz = v.dtype.itemsize
    coarse_row = 8 * C * esz + WMAX * (2 * esz + 4)                          # one layer of the tallest coarse row, and its outputs
    kw = dict(area=area, min_fraction=0.5, outputs=ALL)
    # one band; the three layers of two coarse rows at the most (two bands); one layer of one coarse row per pass
    for stage in (None, 3 * 2 * coarse_row + 4096, 1):
        got = mod16_amd.upscale_fields(v, (HMAX, WMAX), row_pos, col_pos, stage_bytes=stage, **kw)
        assert_same(got, want, 'HOST mode, stage_bytes = %r' % stage)
    got = mod16_amd.upscale_fields(v, (HMAX, WMAX), row_pos, col_pos, stage_bytes=2 * coarse_row, **kw)     # layers cut: one per pass
    assert_same(got, want, 'HOST mode, layers cut')
    some = mod16_amd.upscale_fields(v[0], (HMAX, WMAX), row_pos, col_pos, outputs=('count', 'mean'), stage_bytes=1)
    assert some.fraction is None and some.mean.shape == (HMAX, WMAX)
    rows, cols = (up.cell_runs(up.cell_table(p, s), s) for p, s in ((row_pos, HMAX), (col_pos, WMAX)))
    assert_same(some, up.aggregate(v[0], rows, cols, outputs=('mean', 'count')), 'HOST mode, one plane, a subset')
    grid = engine().upscale_grid((R, C), (HMAX, WMAX), row_pos, col_pos, area=area)
    dev = grid.run(on_device(torch, v), min_fraction=0.5, outputs=ALL)
    engine().check()
    assert_same(dev, want, 'RasterEngine.upscale_grid')
    cls = np.random.default_rng(9).integers(0, 16, (R, C)).astype(np.uint8)
    cwant = up.majority(cls, rows, cols, valid=(1, 2, 3, 14, 15))
    for stage in (None, 2 * (8 * C + 5 * WMAX) + 4096, 1):
        got = mod16_amd.upscale_classes(cls, (HMAX, WMAX), row_pos, col_pos, valid=(1, 2, 3, 14, 15), outputs=('cls', 'share'),
                                        stage_bytes=stage)
        assert_same(got, cwant, 'HOST mode, classes, stage_bytes = %r' % stage)
    only = mod16_amd.upscale_classes(cls.astype(np.int64), (HMAX, WMAX), row_pos, col_pos)
    assert only.share is None
    assert_same(only, up.majority(cls, rows, cols, outputs=('cls',)), 'HOST mode, the class alone')


def test_host_mode_with_decreasing_rows_a_margin_and_the_wrap_cell(env):
    _, mod16_amd = env
    row_pos, col_pos = axis((7, 8, 0, 7), margin=3, reverse=True), axis((6,) * 70, roll=2)
    rows = up.cell_runs(up.cell_table(row_pos, 4), 4)
    cols = up.cell_runs(up.cell_table(col_pos, 70, True), 70, True)
    v = fill(np.random.default_rng(21), 2, row_pos, col_pos, 4, 70, True, 'float32')
    want = up.aggregate(v, rows, cols, outputs=ALL, wrap=True)
    for stage in (None, 1):
        got = mod16_amd.upscale_fields(v, (4, 70), row_pos, col_pos, wrap=True, outputs=ALL, stage_bytes=stage)
        assert_same(got, want, 'stage_bytes = %r' % stage)


def test_two_grids_alive_at_once_and_two_calls_give_the_same_bits(env):
    torch, _ = env
    eng = engine()
    a_pos = shape_case('3x5', 'float32')
    b_pos = shape_case('12x12', 'float32')
    grids = [eng.upscale_grid(c[2].shape[1:], (HMAX, WMAX), c[0], c[1], area=c[3]) for c in (a_pos, b_pos)]
    values = [on_device(torch, c[2]) for c in (a_pos, b_pos)]
    for _ in range(2):
        for g, x, c in zip(grids, values, (a_pos, b_pos)):
            got = g.run(x, min_fraction=0.5, outputs=ALL)
            eng.check()
            assert_same(got, c[4], 'two grids')
    grids[0].close()
    got = grids[1].run(values[1], min_fraction=0.5, outputs=ALL)
    eng.check()
    assert_same(got, b_pos[4], 'after the other grid was closed')


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_classes_with_heavy_ties(env, name):
    torch, _ = env
    eng = engine()
    row_pos, col_pos = shape_case(name, 'float32')[:2]
    fr, fc = SHAPES[name]
    rng = np.random.default_rng(50 + sorted(SHAPES).index(name))
    full = rng.choice(np.array([0, 1, 2, 12, 13, 31, 32, 254, 255], np.uint8), (row_pos.size, col_pos.size))
    full[:, :col_pos.size // 3] = rng.integers(0, 2, (row_pos.size, col_pos.size // 3))          # two codes: ties wherever a cell is even
    dev = on_device(torch, full)
    for H, W in itertools.product(HEIGHTS, WIDTHS):
        R, C = sum(counts(fr, H)), sum(counts(fc, W))
        rows = up.cell_runs(up.cell_table(row_pos[:R], H), H)
        cols = up.cell_runs(up.cell_table(col_pos[:C], W), W)
        grid = eng.upscale_grid((R, C), (H, W), row_pos[:R], col_pos[:C])
        for valid in (None, (1, 13, 31)):
            got = grid.majority(dev[:R, :C], valid=valid, outputs=('cls', 'share'))
            eng.check()
            want = up.majority(full[:R, :C], rows, cols, valid=valid)
            assert_same(got, want, '%s, H = %d, W = %d, valid = %r' % (name, H, W, valid))
        if (fr, fc) == (2, 2) and W == 300:
            assert ((want.share == 0.5) | (want.share == 0.25)).sum() > 10      # ties
            assert (want.cls == 255).any() or valid is None
        only = grid.majority(dev[:R, :C])
        eng.check()
        assert only.share is None and only.cls.dtype == torch.uint8


def test_composites_feed_the_upscaling_on_the_device(env):
    """Two 8-day ET totals of RasterEngine.composite over a 14 x 45 raster, the (P, n) rows viewed as (P, R,
    C) and fed straight into UpscaleGrid.run: the definition on the downloaded totals."""
    torch, _ = env
    from oracle import synth
    eng = engine()
    P, days, R, C = 2, 16, 14, 45
    n = R * C
    dev = eng._dev()
    et = torch.empty((P, n + 6), dtype=torch.float64, device=dev)[:, :n]     # rows a pitch apart
    pet = torch.empty((P, n + 6), dtype=torch.float64, device=dev)[:, :n]
    c_et = torch.empty((P, n + 6), dtype=torch.uint16, device=dev)[:, :n]
    c_pet = torch.empty((P, n + 6), dtype=torch.uint16, device=dev)[:, :n]
    cls, drivers = synth.drivers((days, n), seed=300, special=False)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(synth.drivers((1, n), seed=300, special=False)[0][0])).to(dev)
    hours = put(np.random.default_rng(0).uniform(6, 18, (days, n)))
    eng.composite(c, [put(d) for d in drivers], hours, days, period_days=8, pet=True, out=[et, pet, c_et, c_pet])
    row_pos, col_pos = axis((7, 7)), axis((15, 15, 15))
    grid = eng.upscale_grid((R, C), (2, 3), row_pos, col_pos)
    got = grid.run(et.as_strided((P, R, C), (n + 6, C, 1)), outputs=ALL)
    eng.check()
    e = et.cpu().numpy().reshape(P, R, C)
    rows, cols = up.cell_runs(up.cell_table(row_pos, 2), 2), up.cell_runs(up.cell_table(col_pos, 3), 3)
    want = up.aggregate(e, rows, cols, outputs=ALL)
    assert np.isfinite(want.mean).all() and (want.count > 0).all()
    assert_same(got, want, 'composites')
    coarse_cls = grid.majority(c.view(R, C), outputs=('cls', 'share'))
    eng.check()
    assert_same(coarse_cls, up.majority(c.cpu().numpy().reshape(R, C), rows, cols), 'the class map')
