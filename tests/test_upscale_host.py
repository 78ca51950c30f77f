"""The numpy definition of upscaling (mod16_amd/upscale.py), on the CPU: the known runs of the global
30-arc-second grid over MERRA-2, answers worked by hand on a 2 x 2 cell, numpy's own nanmean over
reshaped blocks, the round trip with 'nearest' interpolation, the bit-level properties the definition
promises (scaling by a power of two, one rounding for float32 input), the geometry cases (mixed runs,
decreasing positions, pixels outside, an empty cell, the cell that straddles the date line), the class
rule, every argument check, and the ABI pieces that need no device. The device result is held to this
definition bit for bit by tests/test_gpu_upscale.py."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mod16_amd import downscale as ds
from mod16_amd import upscale as up

HEADER = os.path.join(ROOT, 'include', 'mod16_hip.h')
ALL = up.OUTPUT_NAMES
NAN, INF = np.nan, np.inf


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def runs_of(pos, size, wrap=False):
    return up.cell_runs(up.cell_table(pos, size, wrap), size, wrap)


def block_runs(cells, per):
    """`cells` cells of `per` fine indices each"""
    return up.Runs(np.arange(cells, dtype=np.int32) * per, np.full(cells, per, np.int32))


ONE = block_runs(1, 2)           # a 2 x 2 raster that is one cell


def cell(values, **kw):
    res = up.aggregate(np.array(values, np.float64).reshape(2, 2), ONE, ONE, outputs=ALL, **kw)
    return res.mean[0, 0], res.fraction[0, 0], res.count[0, 0]


# ---- the known answers of the global grid

def test_global_30_arc_second_grid_over_merra2():
    col_pos = ds.positions(-180 + 1 / 240, 1 / 120, 43200, -180.0, 0.625)
    row_pos = ds.positions(90 - 1 / 240, -1 / 120, 21600, 90.0, -0.5)
    cols = runs_of(col_pos, 576, wrap=True)
    rows = runs_of(row_pos, 361)
    assert tuple(cols.first[:3]) == (43162, 37, 112) and (cols.count == 75).all()
    assert tuple(rows.first[:3]) == (0, 30, 90)
    assert rows.count[0] == 30 and rows.count[-1] == 30 and (rows.count[1:-1] == 60).all()
    assert (up.cell_table(row_pos, 361) >= 0).all() and rows.count.sum() == 21600 and cols.count.sum() == 43200
    assert cols.first.dtype == np.int32 and rows.count.dtype == np.int32
    (R, C), (H, W), r2, c2 = up.check_geometry((21600, 43200), (361, 576), row_pos, col_pos, wrap=True)
    assert (R, C, H, W) == (21600, 43200, 361, 576) and np.array_equal(r2.first, rows.first) and np.array_equal(c2.count, cols.count)


# ---- by hand, on a 2 x 2 cell

def test_one_nan_in_the_cell():
    mean, fraction, count = cell([1.0, NAN, 4.0, 7.0])
    assert mean == ((1.0) + (4.0 + 7.0)) / (1.0 + 2.0) == 4.0 and fraction == 3.0 / 4.0 and count == 3


def test_all_nan():
    mean, fraction, count = cell([NAN] * 4)
    assert np.isnan(mean) and fraction == 0.0 and count == 0


def test_infinities_take_part_as_the_arithmetic_has_them():
    mean, fraction, count = cell([1.0, INF, 2.0, 3.0])
    assert mean == INF and fraction == 1.0 and count == 4
    mean, fraction, count = cell([1.0, INF, -INF, 3.0])
    assert np.isnan(mean) and fraction == 1.0 and count == 4          # inf + -inf: NaN from the arithmetic, all four valid


def test_a_cell_of_negative_zeros_has_the_mean_positive_zero():
    mean, _, count = cell([-0.0] * 4)
    assert mean == 0.0 and not np.signbit(mean) and count == 4


def test_min_fraction_exactly_met_passes_and_one_pixel_short_fails():
    three = [1.0, NAN, 4.0, 7.0]
    assert cell(three, min_fraction=0.75)[0] == 4.0
    assert np.isnan(cell([1.0, NAN, NAN, 7.0], min_fraction=0.75)[0])
    assert cell([1.0, NAN, NAN, 7.0], min_fraction=0.5)[0] == 4.0
    assert cell(three, min_fraction=1.0)[1] == 0.75 and np.isnan(cell(three, min_fraction=1.0)[0])
    assert cell([1.0, 2.0, 3.0, 6.0], min_fraction=1.0)[0] == 3.0
    assert np.isnan(cell([NAN] * 4, min_fraction=0.0)[0])              # no valid pixel: NaN whatever the threshold


def test_area_doubling_one_row():
    res = up.aggregate(np.array([[1.0, 2.0], [4.0, NAN]]), ONE, ONE, area=np.array([1.0, 2.0]), outputs=ALL)
    assert res.mean[0, 0] == (1.0 * 3.0 + 2.0 * 4.0) / (1.0 * 2.0 + 2.0 * 1.0) == 2.75
    assert res.fraction[0, 0] == 4.0 / 6.0 and res.count[0, 0] == 3


# ---- against numpy, and the round trip

@pytest.mark.parametrize('fr,fc', [(3, 5), (1, 1), (2, 2), (6, 6)])
def test_nanmean_over_reshaped_blocks(fr, fc):
    rng = np.random.default_rng(fr * 10 + fc)
    K, H, W = 2, 4, 5
    v = rng.gamma(4.0, 5.0, (K, H * fr, W * fc))
    v[rng.uniform(0, 1, v.shape) < 0.2] = NAN
    res = up.aggregate(v, block_runs(H, fr), block_runs(W, fc), outputs=ALL)
    blocks = v.reshape(K, H, fr, W, fc).transpose(0, 1, 3, 2, 4).reshape(K, H, W, fr * fc)
    some = (~np.isnan(blocks)).any(axis=-1)                             # (a cell that is all NaN has the mean NaN)
    want = np.where(some, np.nansum(blocks, axis=-1) / np.maximum((~np.isnan(blocks)).sum(axis=-1), 1), NAN)
    assert np.array_equal(np.isnan(res.mean), ~some) and some.sum() > some.size // 2
    assert np.abs(res.mean - want)[some].max() <= 1e-12
    assert np.allclose(want[some], np.nanmean(blocks[some], axis=-1), rtol=1e-15, atol=0)
    assert np.array_equal(res.count, (~np.isnan(blocks)).sum(axis=-1))
    assert np.array_equal(res.fraction, res.count / float(fr * fc))


@pytest.mark.parametrize('fr,fc,narrow', [(2, 2, False), (1, 2, False), (4, 8, True), (16, 2, True)])
def test_round_trip_with_nearest_interpolation_on_power_of_two_cells(fr, fc, narrow):
    """Every pixel of a cell holds the cell's value x, so the sums are x, 2 x, 3 x, ...: with up to two
    columns and two rows every one of them is x times a power of two, exact for any float64 x. A longer
    run passes 3 x, which needs two more bits than x has: exact where x has bits to spare (float32
    values, 24 bits, widened), and num / den = (c x) / c is then x for the power of two c."""
    H, W = 3, 5
    rng = np.random.default_rng(5)
    coarse = rng.gamma(4.0, 5.0, (H, W))
    if narrow:
        coarse = coarse.astype(np.float32).astype(np.float64)
    row_pos = ds.positions(0.5, 1.0, H * fr, fr / 2, fr)              # fine centres 0.5, 1.5, ...; cell 0 centred on fr / 2
    col_pos = ds.positions(0.5, 1.0, W * fc, fc / 2, fc)
    fine = ds.interpolate(coarse, ds.corner_tables(row_pos, H, False, 'nearest'), ds.corner_tables(col_pos, W, False, 'nearest'))
    res = up.aggregate(fine, runs_of(row_pos, H), runs_of(col_pos, W), outputs=ALL)
    assert same(res.mean[0] if res.mean.ndim == 3 else res.mean, coarse)
    assert (res.count == fr * fc).all() and (res.fraction == 1.0).all()


def test_scaling_by_a_power_of_two_changes_no_bit_it_should_not():
    rng = np.random.default_rng(6)
    v = rng.gamma(4.0, 5.0, (2, 9, 10))
    v[rng.uniform(0, 1, v.shape) < 0.3] = NAN
    rows, cols = block_runs(3, 3), block_runs(2, 5)
    area = rng.uniform(0.2, 1.0, 9)
    base = up.aggregate(v, rows, cols, area=area, min_fraction=0.5, outputs=ALL)
    scaled = up.aggregate(v * 2.0 ** -7, rows, cols, area=area, min_fraction=0.5, outputs=ALL)
    assert same(scaled.mean, base.mean * 2.0 ** -7) and same(scaled.fraction, base.fraction)
    wide = up.aggregate(v, rows, cols, area=area * 2.0 ** 5, min_fraction=0.5, outputs=ALL)
    assert same(wide.mean, base.mean) and same(wide.fraction, base.fraction) and np.array_equal(wide.count, base.count)


def test_float32_is_the_float64_result_rounded_once():
    rng = np.random.default_rng(7)
    v = rng.gamma(4.0, 5.0, (7, 12)).astype(np.float32)
    v[rng.uniform(0, 1, v.shape) < 0.2] = NAN
    rows, cols = runs_of(ds.positions(0.5, 1, 7, 1.5, 3), 3), block_runs(4, 3)
    r32 = up.aggregate(v, rows, cols, outputs=ALL)
    r64 = up.aggregate(v.astype(np.float64), rows, cols, outputs=ALL)
    assert r32.mean.dtype == np.float32 and r32.fraction.dtype == np.float32 and r32.count.dtype == np.int32
    assert r32.mean.shape == (3, 4)
    assert same(r32.mean, r64.mean.astype(np.float32)) and same(r32.fraction, r64.fraction.astype(np.float32))
    assert np.array_equal(r32.count, r64.count)


# ---- geometry

def test_37_fine_rows_over_5_cells():
    pos = ds.positions(0.5, 1.0, 37, 3.7, 7.4)                         # cell k covers [7.4 k, 7.4 (k + 1))
    runs = runs_of(pos, 5)
    assert list(runs.count) == [7, 8, 7, 8, 7] and list(runs.first) == [0, 7, 15, 22, 30]


def test_half_way_goes_to_the_far_cell_and_outside_is_minus_one():
    assert list(up.cell_table([-0.51, -0.5, 0.49, 0.5, 1.49, 1.5, 7.0], 2)) == [-1, 0, 0, 1, 1, -1, -1]
    assert list(up.cell_table([-0.5, 1.5, 1.49, 2.5, -0.51], 2, wrap=True)) == [0, 0, 1, 1, 1]
    near = ds.corner_tables([0.0, 0.49, 0.5, 1.0], 2, False, 'nearest')
    assert list(np.where(near[3] == 1.0, near[1], near[0])) == list(up.cell_table([0.0, 0.49, 0.5, 1.0], 2))


def test_decreasing_positions():
    pos = ds.positions(0.5, 1.0, 6, 4.5, -3.0)                         # cell 0 holds fine 3, 4, 5
    runs = runs_of(pos, 2)
    assert list(runs.first) == [3, 0] and list(runs.count) == [3, 3]
    v = np.arange(12.0).reshape(6, 2)
    res = up.aggregate(v, runs, block_runs(1, 2))
    assert res.mean[0, 0] == v[3:].mean() and res.mean[1, 0] == v[:3].mean()


def test_pixels_outside_the_grid_belong_to_no_cell():
    pos = ds.positions(0.5, 1.0, 10, 3.0, 2.0)                         # cells of 2; fine 0, 1 and 8, 9 lie outside 3 cells
    table = up.cell_table(pos, 3)
    assert list(table) == [-1, -1, 0, 0, 1, 1, 2, 2, -1, -1]
    runs = runs_of(pos, 3)
    assert list(runs.first) == [2, 4, 6] and list(runs.count) == [2, 2, 2]
    v = np.full((10, 2), 1e30)
    v[2:8] = 5.0
    assert (up.aggregate(v, runs, block_runs(1, 2)).mean == 5.0).all()


def test_an_empty_cell():
    runs = runs_of([0.0, 0.1, 2.0, 2.2], 3)
    assert list(runs.count) == [2, 0, 2] and runs.first[1] == 0
    res = up.aggregate(np.ones((4, 4)), runs, runs, outputs=ALL)
    assert np.isnan(res.mean[1]).all() and np.isnan(res.mean[:, 1]).all() and res.mean[0, 0] == 1.0
    assert (res.fraction[1] == 0).all() and (res.count[1] == 0).all() and res.fraction[2, 2] == 1.0


def test_the_wrap_cell_is_a_cyclic_run():
    pos = ds.positions(0.5, 1.0, 12, 0.0, 4.0)                         # cell 0 centred on 0: fine 10, 11, 0, 1
    assert list(up.cell_table(pos, 3, wrap=True)) == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0, 0]
    runs = runs_of(pos, 3, wrap=True)
    assert list(runs.first) == [10, 2, 6] and list(runs.count) == [4, 4, 4]
    with pytest.raises(ValueError, match='one run'):
        up.cell_runs(up.cell_table(pos, 3, wrap=True), 3, wrap=False)
    v = np.array([[1.0, NAN, 5, 5, 5, 5, 9, 9, 9, 9, 1e-30, 1e30]])
    res = up.aggregate(v, block_runs(1, 1), runs, wrap=True, outputs=ALL)
    assert res.mean[0, 0] == ((1e-30 + 1e30) + 1.0) / 3.0 and res.count[0, 0] == 3      # run order: 10, 11, 0, 1
    assert res.mean[0, 1] == 5.0 and res.mean[0, 2] == 9.0
    whole = up.cell_runs(np.zeros(5, np.int32), 1, wrap=True)
    assert list(whole.first) == [0] and list(whole.count) == [5]


def test_order_of_the_definition_rows_then_columns():
    big = 2.0 ** 60
    v = np.array([[big, 1.0], [-big, 1.0]])
    mean, _, _ = (a[0, 0] for a in up.aggregate(v, ONE, ONE, outputs=ALL))
    assert mean == ((big + 1.0) + (-big + 1.0)) / 4.0 == 0.0          # each row's 1.0 is lost in its own row sum


# ---- classes

def test_majority_ties_subsets_and_255():
    cls = np.array([[3, 1, 7, 7, 200, 13],
                    [1, 3, 7, 9, 200, 31]], np.uint8)
    rows, cols = block_runs(1, 2), block_runs(3, 2)
    res = up.majority(cls, rows, cols)
    assert list(res.cls[0]) == [1, 7, 255] and res.cls.dtype == np.uint8 and res.share.dtype == np.float32
    assert list(res.share[0]) == [np.float32(0.5), np.float32(0.75), np.float32(0.0)]
    res = up.majority(cls, rows, cols, valid=(3, 9, 13, 31))
    assert list(res.cls[0]) == [3, 9, 13] and list(res.share[0]) == [np.float32(0.5), np.float32(0.25), np.float32(0.25)]
    res = up.majority(cls, rows, cols, valid=(), outputs=('share',))
    assert res.cls is None and (res.share == 0).all()
    third = up.majority(np.array([[2, 2, 5]], np.uint8), block_runs(1, 1), block_runs(1, 3), outputs=('cls', 'share'))
    assert third.cls[0, 0] == 2 and third.share[0, 0] == np.float32(2.0 / 3.0)
    empty = up.majority(cls, rows, up.Runs(np.array([0, 0, 4], np.int32), np.array([4, 0, 2], np.int32)))
    assert list(empty.cls[0]) == [7, 255, 255] and list(empty.share[0]) == [np.float32(3 / 8), 0, 0]
    assert up.valid_mask() == 0x1fff and up.valid_mask((0, 31)) == 0x80000001


# ---- refusals

def test_every_refusal():
    v = np.ones((2, 4, 6))
    rows, cols = block_runs(2, 2), block_runs(3, 2)
    bad = lambda *a, **k: pytest.raises(ValueError, match=k.pop('match', None))
    with bad(match='not finite'):
        up.cell_table([0.0, NAN], 2)
    with bad(match='not finite'):
        up.cell_table([INF], 2, wrap=True)
    with bad(match='one-dimensional'):
        up.cell_table(np.zeros((2, 2)), 2)
    with bad(match='size must be'):
        up.cell_table([0.0], 0)
    with bad(match='size must be'):
        up.cell_table([0.0], ds.MAX_EXTENT + 1)
    with bad(match='one run'):
        up.cell_runs(np.array([0, 1, 0], np.int32), 2)
    with bad(match='outside'):
        up.cell_runs(np.array([0, 2], np.int32), 2)
    with bad(match='not contiguous'):
        up.aggregate(v, up.Runs(np.array([0, 1], np.int32), np.array([2, 2], np.int32)), cols)
    with bad(match='leaves'):
        up.aggregate(v, up.Runs(np.array([0, 3], np.int32), np.array([2, 2], np.int32)), cols)
    with bad(match='leaves'):
        up.aggregate(v, rows, up.Runs(np.array([0, 2, 5], np.int32), np.array([2, 2, 2], np.int32)))       # cyclic only with wrap
    assert up.aggregate(v, rows, up.Runs(np.array([1, 3, 5], np.int32), np.array([2, 2, 2], np.int32)), wrap=True).mean.shape == (2, 2, 3)
    with bad(match='2\\^31'):
        up.check_cell_size(up.Runs(np.zeros(1, np.int32), np.array([2 ** 16], np.int32)),
                           up.Runs(np.zeros(1, np.int32), np.array([2 ** 15], np.int32)))
    up.check_cell_size(up.Runs(np.zeros(1, np.int32), np.array([2 ** 16], np.int32)),
                       up.Runs(np.zeros(1, np.int32), np.array([2 ** 15 - 1], np.int32)))
    pos4, pos6 = ds.positions(0.5, 1, 4, 1.0, 2.0), ds.positions(0.5, 1, 6, 1.0, 2.0)
    with bad(match='between 1 and'):
        up.check_geometry((4, 6), (2, ds.MAX_EXTENT + 1), pos4, pos6)
    with bad(match='between 1 and'):
        up.check_geometry((0, 6), (2, 3), pos4[:0], pos6)
    with bad(match='shapes'):
        up.check_geometry((4, 6), (2, 3), pos6, pos6)
    with bad(match='col_affine'):
        up.check_geometry((4, 6), (2, 3), pos4, pos6, col_affine=(np.zeros(4), np.ones(4)))
    with bad(match='layers'):
        up.check_layers((0, 4, 6), (4, 6))
    with bad(match='layers'):
        up.check_layers((65536, 4, 6), (4, 6))
    assert up.check_layers((65535, 4, 6), (4, 6)) == (65535, False) and up.check_layers((4, 6), (4, 6)) == (1, True)
    with bad(match='shape'):
        up.check_layers((2, 4, 7), (4, 6))
    with bad(match='float32 or float64'):
        up.aggregate(np.ones((4, 6), np.int32), rows, cols)
    for area in (np.ones(5), np.ones((4, 1)), [1, 0, 1, 1], [1, -1, 1, 1], [1, NAN, 1, 1], [1, INF, 1, 1]):
        with bad(match='area'):
            up.aggregate(v, rows, cols, area=area)
    for mf in (-0.1, 1.1, NAN, 'x', None):
        with bad(match='min_fraction'):
            up.aggregate(v, rows, cols, min_fraction=mf)
    for outs in ((), ('median',), ('mean', 'mean'), 'share'):
        with bad(match='outputs'):
            up.aggregate(v, rows, cols, outputs=outs)
    with bad(match='outputs'):
        up.majority(np.zeros((4, 6), np.uint8), rows, cols, outputs=('mean',))
    for valid in ((32,), (-1,), (1.0,), (True,)):
        with bad(match='valid'):
            up.majority(np.zeros((4, 6), np.uint8), rows, cols, valid=valid)
    with bad(match='uint8'):
        up.majority(np.zeros((4, 6), np.int32), rows, cols)


# ---- the ABI pieces that need no device

def test_the_symbols_are_in_the_header_and_the_prototypes():
    from mod16_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    names = ('mod16_upscale_create', 'mod16_upscale_destroy', 'mod16_upscale_f32', 'mod16_upscale_f64', 'mod16_upscale_classes')
    for name in names:
        assert re.search(r'MOD16_API\s+int\s+%s\s*\(' % name, text), name
        assert name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES['mod16_upscale_f32'][1]) == 19 and len(_lib.PROTOTYPES['mod16_upscale_classes'][1]) == 12
    assert _lib.ABI_VERSION == 16
    fields = [f for f, _ in _lib.UpscaleSpec._fields_]
    spec = re.search(r'typedef struct mod16_upscale_spec \{(.*?)\}', text, flags=re.S).group(1)
    assert fields == re.findall(r'(\w+)\s*[,;]', spec)
    import mod16
    import mod16_amd
    assert mod16.upscale_fields is mod16_amd.upscale_fields and mod16.upscale_classes is mod16_amd.upscale_classes


def test_entry_points_check_their_arguments_before_they_need_a_device():
    import mod16_amd
    pos4, pos6 = ds.positions(0.5, 1, 4, 1.0, 2.0), ds.positions(0.5, 1, 6, 1.0, 2.0)
    with pytest.raises(ValueError, match='outputs'):
        mod16_amd.upscale_fields(np.ones((4, 6)), (2, 3), pos4, pos6, outputs=('median',))
    with pytest.raises(ValueError, match='min_fraction'):
        mod16_amd.upscale_fields(np.ones((4, 6)), (2, 3), pos4, pos6, min_fraction=2)
    with pytest.raises(ValueError, match='not finite'):
        mod16_amd.upscale_fields(np.ones((4, 6)), (2, 3), pos4 * NAN, pos6)
    with pytest.raises(ValueError, match='stage_bytes'):
        mod16_amd.upscale_fields(np.ones((4, 6)), (2, 3), pos4, pos6, stage_bytes=-1)
    with pytest.raises(ValueError, match='valid'):
        mod16_amd.upscale_classes(np.zeros((4, 6), np.uint8), (2, 3), pos4, pos6, valid=(40,))
    with pytest.raises(IndexError):
        mod16_amd.upscale_classes(np.full((4, 6), 300), (2, 3), pos4, pos6)
