"""The numpy definition of upscaling with row-affine columns (mod16_amd/upscale.py: cell_table_rows,
cell_runs_rows, aggregate_rows, sums_rows, majority_rows, merge, check_rows; downscale.sinusoidal_columns)
against a per-pixel Python loop, against the rectilinear definition where the two geometries coincide, and
the ABI pieces that need no device. No GPU."""
import math
import os
import re

import numpy as np
import pytest

from mod16_amd import downscale as ds
from mod16_amd import upscale as up

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mod16_hip.h')
R, C, H, W = 9, 40, 3, 7
ROW_POS = (np.arange(R) + 0.5) * H / R - 0.5


def bad(match):
    return pytest.raises(ValueError, match=match)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.where(np.isnan(b), a, b).tobytes() \
        and np.array_equal(np.isnan(a), np.isnan(b)) if a.dtype.kind == 'f' else (a.dtype == b.dtype and np.array_equal(a, b))


def cell_of(pos, size, wrap):
    """cell_table for one position, in Python floats"""
    if wrap:
        p = pos - math.floor(pos / float(size)) * float(size)
        if p >= size or p < 0:
            p = 0.0
        i0 = math.floor(p)
        return (int(i0) + (p - i0 >= 0.5)) % size
    i0 = math.floor(pos)
    cell = int(i0) + (pos - i0 >= 0.5)
    return cell if 0 <= cell < size else -1


def brute(values, cls, origin, scale, wrap, col_range, area, min_fraction, valid=range(13)):
    """per pixel, in raster order within a cell: (cells, num, den, tot, cnt, mean, fraction, cls, share)"""
    K = values.shape[0]
    cells = np.full((R, C), -1, np.int64)
    for r in range(R):
        f, n = (0, C) if col_range is None else (int(col_range[0][r]), int(col_range[1][r]))
        for c in range(f, f + n):
            cells[r, c] = cell_of(float(origin[r]) + float(scale[r]) * float(c), W, wrap)
    row_cell = [cell_of(float(p), H, False) for p in ROW_POS]
    num, den, tot = np.zeros((K, H, W)), np.zeros((K, H, W)), np.zeros((K, H, W))
    cnt = np.zeros((K, H, W), np.int64)
    votes = np.zeros((H, W, 256), np.int64)
    pixels = np.zeros((H, W), np.int64)
    for r in range(R):
        i = row_cell[r]
        if i < 0:
            continue
        a = 1.0 if area is None else float(area[r])
        for j in range(W):
            at = [c for c in range(C) if cells[r, c] == j]
            pixels[i, j] += len(at)
            for c in at:
                votes[i, j, cls[r, c]] += 1
            for k in range(K):
                s, m = 0.0, 0
                for c in at:
                    x = float(values[k, r, c])
                    if x == x:
                        s, m = s + x, m + 1
                num[k, i, j] = num[k, i, j] + a * s
                den[k, i, j] = den[k, i, j] + a * float(m)
                tot[k, i, j] = tot[k, i, j] + a * float(len(at))
                cnt[k, i, j] += m
    with np.errstate(all='ignore'):
        fraction = np.where(tot > 0, den / tot, 0.0)
        mean = np.where((cnt >= 1) & (den >= min_fraction * tot), num / den, np.nan)
    out_cls, share = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.float32)
    for i in range(H):
        for j in range(W):
            best = max((int(votes[i, j, code]), -code) for code in valid)
            if best[0] > 0:
                out_cls[i, j], share[i, j] = -best[1], np.float32(best[0] / float(pixels[i, j]))
    return cells, num, den, tot, cnt, mean, fraction, out_cls, share


def raster(seed, dtype=np.float64, K=2):
    rng = np.random.default_rng(seed)
    v = rng.gamma(4.0, 5.0, (K, R, C))
    v[rng.uniform(size=v.shape) < 0.25] = np.nan
    v[0, 4, 3:9] = [-0.0, np.inf, -np.inf, 1e300, -1e300, 0.0]
    with np.errstate(over='ignore'):                            # (1e300 is inf in float32)
        v = v.astype(dtype)
    return v, rng.integers(0, 5, (R, C)).astype(np.uint8)


GEOMETRIES = {
    # origin, scale, wrap, col_range
    'plain': (np.full(R, -0.375), np.full(R, 0.25), False, None),
    'mixed': (np.array([-0.4, 7.3, 0.0, 3.25, -60.0, 1.1, 6.9, -0.5, 2.0]),
              np.array([0.19, -0.21, 0.3, 0.0, 0.1, 2.6, -0.07, 0.25, -1.4]), False, None),
    'ranges': (np.array([-0.4, 7.3, 0.0, 3.25, -60.0, 1.1, 6.9, -0.5, 2.0]),
               np.array([0.19, -0.21, 0.3, 0.0, 0.1, 2.6, -0.07, 0.25, -1.4]), False,
               (np.array([0, 5, 39, 2, 0, 1, 10, 0, 3], np.int32), np.array([40, 30, 1, 0, 40, 3, 30, 17, 4], np.int32))),
    'wrap': (np.array([-0.4, 7.3, 6.0, 3.25, -60.0, 1.1, 6.9, 13.5, 2.0]),
             np.array([0.19, -0.21, 0.3, 0.0, 0.1, 2.6, -0.07, 0.25, -1.4]), True,
             (np.array([0, 5, 20, 2, 0, 1, 0, 0, 3], np.int32), np.array([27, 24, 17, 38, 40, 2, 40, 21, 4], np.int32))),
}


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_definition_is_the_per_pixel_loop(name, dtype):
    origin, scale, wrap, col_range = GEOMETRIES[name]
    v, cls = raster(len(name), dtype)
    area = np.random.default_rng(1).uniform(0.2, 1.0, R)
    cells, num, den, tot, cnt, mean, fraction, out_cls, share = brute(v, cls, origin, scale, wrap, col_range, area, 0.5)
    table = up.cell_table_rows(origin, scale, C, W, wrap, col_range)
    assert table.dtype == np.int32 and np.array_equal(table, cells)
    runs = up.cell_runs_rows(table, W)
    assert runs.first.dtype == np.int32 and runs.first.shape == (R, W)
    for r in range(R):
        for j in range(W):
            at = np.flatnonzero(cells[r] == j)
            assert runs.count[r, j] == at.size and (not at.size or (runs.first[r, j] == at[0] and at[-1] - at[0] + 1 == at.size))
    rows = up.cell_runs(up.cell_table(ROW_POS, H), H)
    got = up.aggregate_rows(v, rows, (origin, scale), W, wrap, col_range, area, 0.5)
    assert same(got.mean, mean.astype(dtype)) and same(got.fraction, fraction.astype(dtype)) and same(got.count, cnt.astype(np.int32))
    sums = up.sums_rows(v, rows, (origin, scale), W, wrap, col_range, area)
    assert type(sums) is up.UpscaledSums and up.SUM_NAMES == ('num', 'den', 'tot', 'count')
    assert same(sums.num, num) and same(sums.den, den) and same(sums.tot, tot) and same(sums.count, cnt.astype(np.int32))
    assert sums.num.dtype == np.float64
    some = up.sums_rows(v[0], rows, (origin, scale), W, wrap, col_range, area, outputs=('tot', 'count'))
    assert some.num is None and some.den is None and same(some.tot, tot[0]) and some.count.shape == (H, W)
    assert all(same(a, b) for a, b in zip(up.merge([sums], 0.5, dtype), got))
    maj = up.majority_rows(cls, rows, (origin, scale), W, wrap, col_range)
    assert same(maj.cls, out_cls) and same(maj.share, share)
    if name in ('mixed', 'ranges'):
        assert (cells == -1).all(axis=1).any()                  # a row that belongs to no cell
        assert (np.diff(np.where(cells[5] >= 0, cells[5], 0)) > 1).any()      # |scale| > 1: cells without a pixel in between


def test_dyadic_geometry_has_the_bits_of_the_rectilinear_definition():
    origin, scale = np.full(R, -0.375), np.full(R, 0.25)
    pos = ds.column_positions(origin, scale, C)
    assert np.array_equal(pos[0], -0.375 + 0.25 * np.arange(C)) and (pos == pos[0]).all()
    rows = up.cell_runs(up.cell_table(ROW_POS, H), H)
    v, cls = raster(3)
    area = np.random.default_rng(2).uniform(0.2, 1.0, R)
    for wrap in (False, True):
        col_range = (np.zeros(R, np.int32), np.full(R, 21, np.int32)) if wrap else None      # 0.25 * 20 = W - 2
        cols = up.cell_runs(up.cell_table(pos[0], W), W)
        if wrap:
            cols = up.cell_runs(np.where(np.arange(C) < 21, up.cell_table(pos[0], W, True), -1), W, False)
        a = up.aggregate(v, rows, cols, area, 0.5)
        b = up.aggregate_rows(v, rows, (origin, scale), W, wrap, col_range, area, 0.5)
        assert all(same(x, y) for x, y in zip(a, b))
        assert all(same(x, y) for x, y in zip(up.sums(v, rows, cols, area), up.sums_rows(v, rows, (origin, scale), W, wrap, col_range, area)))
        assert all(same(x, y) for x, y in zip(up.majority(cls, rows, cols), up.majority_rows(cls, rows, (origin, scale), W, wrap, col_range)))
    assert all(same(x, y) for x, y in zip(up.merge([up.sums(v, rows, cols, area)], 0.5), up.aggregate(v, rows, cols, area, 0.5)))


def test_a_tie_goes_to_the_far_cell():
    table = up.cell_table_rows([-0.5], [0.25], C, W)
    assert table[0, :9].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2]          # pos -0.5, 0.5, 1.5: f == 0.5 -> the far cell
    assert up.cell_table_rows([6.5], [-0.25], C, W)[0, :6].tolist() == [-1, 6, 6, 6, 6, 5]       # 6.5 -> 7: outside; 5.5 -> 6
    assert up.cell_table_rows([6.5], [0.25], 3, W, wrap=True)[0].tolist() == [0, 0, 0]      # 6.5 -> 7 = 0 (mod 7)


def test_the_acceptance_rule():
    origin, scale = np.zeros(4), np.array([0.1, 0.1, 0.2, 0.1])
    up.check_rows((4, 40), 7, (origin, scale), wrap=False)
    up.check_rows((4, 51), 7, (origin, np.full(4, 0.1)), wrap=True)                       # 0.1 * 50 <= 5
    with bad('fine row 2 may lap'):
        up.check_rows((4, 40), 7, (origin, scale), wrap=True)                            # 0.2 * 39 > 5
    with bad('col_range'):
        up.check_rows((4, 40), 7, (origin, scale), wrap=True)
    affine, col_range = up.check_rows((4, 40), 7, (origin, scale), True, (np.zeros(4, np.int32), np.array([40, 40, 26, 40], np.int32)))
    assert affine[0].dtype == np.float64 and col_range.count.tolist() == [40, 40, 26, 40]
    up.check_rows((4, 40), 7, (origin, np.array([0.1, 0.1, 500.0, 0.1])), True, (np.zeros(4, np.int32), np.array([40, 40, 1, 0], np.int32)))
    # a row the rule accepts is one run per cell: random rows against cell_table and cell_runs
    rng = np.random.default_rng(0)
    tried = 0
    for _ in range(600):
        w, c = int(rng.integers(1, 40)), int(rng.integers(1, 200))
        s = float(rng.choice([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, rng.normal(), rng.normal() * 0.1]))
        o = float(rng.choice([-1e-20, w - 0.5, 0.0, rng.normal() * w, 1000.0 * w, -77.0 * w + 0.5]))
        n = c if abs(s) * (c - 1) <= w - 2 else (int((w - 2) / abs(s)) + 1 if w >= 2 else 1)
        if n > 1 and not abs(s) * float(n - 1) <= float(w - 2):
            n -= 1
        first = int(rng.integers(0, c - n + 1))
        col_range = (np.array([first], np.int32), np.array([n], np.int32))
        up.check_rows((1, c), w, ([o], [s]), True, col_range)
        up.cell_runs_rows(up.cell_table_rows([o], [s], c, w, True, col_range), w)
        tried += 1
    assert tried == 600
    with bad('fine row 0: the fine indices of cell 0 do not form one run'):
        up.cell_runs_rows(np.array([[0, 1, 0]], np.int32), 2)
    with bad('fine row 1'):
        up.cell_runs_rows(up.cell_table_rows([0.0, 0.0], [0.1, 0.5], 40, 7, True), 7)       # a lapping row is not one run per cell


def test_sinusoidal_columns():
    for size in (24, 48):
        first, count = ds.sinusoidal_columns(18, 8, size)
        assert first.dtype == np.int32 and count.dtype == np.int32 and (first == 0).all() and (count == size).all()      # an interior tile
        first, count = ds.sinusoidal_columns(11, 2, size)
        assert (count[-size // 4:] == size).all() and (count > 0).all() and count[0] < size           # cut near its top only (70 N at 70 W x / cos)
        assert ((first + count)[count < size] == size).all()                                         # its west is cut
        for tile in ((17, 0), (0, 8), (35, 9)):
            first, count = ds.sinusoidal_columns(*tile, size)
            assert count.min() < size and count.max() > 0 and (first >= 0).all() and (first + count <= size).all(), tile
        first, count = ds.sinusoidal_columns(0, 8, size)
        assert count[0] < size and ((first + count) == size).all() and (np.diff(count) >= 0).all()    # wider towards the equator
        first, count = ds.sinusoidal_columns(35, 9, size)
        assert (first == 0).all() and (np.diff(count) <= 0).all()
    # the range is the pixels whose longitude lies within 180 degrees, and every such row passes the rule over 361 x 576
    for tile in ((17, 0), (35, 9), (11, 2), (0, 8), (24, 15), (17, 17)):
        row_pos, origin, scale = ds.sinusoidal_positions(*tile, 48, 90.0, -0.5, -180.0, 0.625)
        col_range = ds.sinusoidal_columns(*tile, 48)
        lon = (origin[:, None] + scale[:, None] * np.arange(48)) * 0.625 - 180.0
        on = np.abs(lon) <= 180.0 + 1e-9
        inside = (np.arange(48) >= col_range[0][:, None]) & (np.arange(48) < (col_range[0] + col_range[1])[:, None])
        assert (on == inside).mean() > 0.999 and not (inside & (np.abs(lon) > 180.0 + 1e-6)).any()
        geometry = up.check_geometry_rows((48, 48), (361, 576), row_pos, (origin, scale), True, col_range)
        up.cell_runs_rows(up.cell_table_rows(origin, scale, 48, 576, True, col_range), 576)
        assert geometry[0] == (48, 48) and geometry[1] == (361, 576) and len(geometry) == 5
    for args in ((36, 0, 4), (0, 18, 4), (-1, 0, 4), (0, 0, 0)):
        with bad('must be between'):
            ds.sinusoidal_columns(*args)


def test_merge():
    rows = up.cell_runs(up.cell_table(ROW_POS, H), H)
    origin, scale = np.full(R, -0.375), np.full(R, 0.125)                # dyadic: origin + scale * 20 is exact
    rng = np.random.default_rng(4)
    v = rng.integers(0, 40, (2, R, C)).astype(np.float64)                # small integers, dyadic weights: every sum is exact
    v[rng.uniform(size=v.shape) < 0.2] = np.nan
    area = 2.0 ** -rng.integers(0, 3, R)
    whole = up.aggregate_rows(v, rows, (origin, scale), W, area=area, min_fraction=0.5)
    parts = [up.sums_rows(v[:, :, c0:c1], rows, (origin + scale * c0, scale), W, area=area) for c0, c1 in ((0, 20), (20, C))]
    for order in (parts, parts[::-1]):
        assert all(same(a, b) for a, b in zip(up.merge(order, 0.5), whole))
    assert all(same(a, b) for a, b in zip(up.merge(parts, 0.5, np.float32), up.aggregate_rows(v.astype(np.float32), rows, (origin, scale), W,
                                                                                              area=area, min_fraction=0.5)))
    # the order of the parts matters where the sums round
    x = [up.UpscaledSums(np.array([[t]]), np.array([[1.0]]), np.array([[1.0]]), np.array([[1]], np.int32)) for t in (1e16, 1.0, 1.0)]
    assert up.merge(x).mean[0, 0] == (1e16 + 1.0 + 1.0) / 3.0 and up.merge(x[::-1]).mean[0, 0] == (2.0 + 1e16) / 3.0
    assert up.merge(x).mean[0, 0] != up.merge(x[::-1]).mean[0, 0] and up.merge(x).count.dtype == np.int32
    assert 'order' in up.merge.__doc__
    # windows of a larger accumulator, cyclic in the columns
    one = up.UpscaledSums(np.full((2, 3), 6.0), np.full((2, 3), 2.0), np.full((2, 3), 4.0), np.full((2, 3), 2, np.int32))
    m = up.merge([one, one], shape=(3, 5), offsets=((0, 0), (1, 3)), wrap=True)
    want_cnt = np.zeros((3, 5), np.int32)
    want_cnt[0:2, 0:3] += 2
    want_cnt[1:3, [3, 4, 0]] += 2
    assert np.array_equal(m.count, want_cnt) and m.mean[1, 0] == 3.0 and np.isnan(m.mean[0, 4]) and m.fraction[2, 4] == 0.5
    assert up.merge([one], shape=(2, 3), offsets=((0, 0),)).mean.shape == (2, 3)
    with bad('leaves'):
        up.merge([one, one], shape=(3, 5), offsets=((0, 0), (1, 3)))
    with bad('leaves'):
        up.merge([one], shape=(3, 5), offsets=((2, 0),), wrap=True)
    with bad('together'):
        up.merge([one], shape=(3, 5))
    with bad('equal shape'):
        up.merge([one, up.UpscaledSums(*[a[:1] for a in one])])
    with bad('at least one'):
        up.merge([])
    with bad('all of num, den, tot, count'):
        up.merge([one._replace(tot=None)])
    with bad('does not fit'):
        up.merge([one], shape=(2, 3, 5), offsets=((0, 0),))
    with bad('one \\(i0, j0\\) per part'):
        up.merge([one], shape=(3, 5), offsets=((0, 0), (0, 0)))
    with bad('int32'):
        up.merge([one._replace(count=np.full((2, 3), 2 ** 30, np.int32))] * 2)
    with bad('min_fraction'):
        up.merge([one], 2.0)
    with bad('float32 or float64'):
        up.merge([one], dtype=np.int32)


def test_every_new_refusal():
    rows = up.cell_runs(up.cell_table(ROW_POS, H), H)
    origin, scale = np.full(R, -0.375), np.full(R, 0.25)
    v, cls = raster(0)
    i32 = lambda *a: np.array(a, np.int32)
    full = np.full(R, C, np.int32)
    with bad('exactly one of col_pos and col_affine'):
        up.check_geometry((R, C), (H, W), ROW_POS, None)
    with bad('exactly one of col_pos and col_affine'):
        up.check_geometry((R, C), (H, W), ROW_POS, np.zeros(C), col_affine=(origin, scale))
    with bad('check_geometry_rows'):
        up.check_geometry((R, C), (H, W), ROW_POS, None, col_affine=(origin, scale))
    with bad('row_pos must have shape'):
        up.check_geometry_rows((R, C), (H, W), ROW_POS[:-1], (origin, scale))
    with bad('between 1 and'):
        up.check_geometry_rows((R, C), (0, W), ROW_POS, (origin, scale))
    with bad('col_affine must be'):
        up.check_rows((R, C), W, (origin,))
    with bad('expected \\(9,\\)'):
        up.check_rows((R, C), W, (origin[:-1], scale[:-1]))
    with bad('not finite'):
        up.check_rows((R, C), W, (origin, scale * np.inf))
    with bad('not finite in some row'):
        up.check_rows((R, C), W, (np.full(R, 1e308), np.full(R, 1e307)))
    for col_range, match in (((np.zeros(R, np.int32),), 'must be \\(col_first, col_count\\)'),
                             ((np.zeros(R, np.int64), full), 'int32'), ((np.zeros(R - 1, np.int32), full[:-1]), 'shape'),
                             ((np.full(R, -1, np.int32), full), 'leaves'), ((np.zeros(R, np.int32), -full), 'leaves'),
                             ((np.ones(R, np.int32), full), 'leaves')):
        with bad(match):
            up.check_col_range(col_range, R, C)
        with bad(match):
            up.aggregate_rows(v, rows, (origin, scale), W, col_range=col_range)
    assert up.check_col_range(None, 2, 5).count.tolist() == [5, 5]
    with bad('2\\^31'):
        up.check_geometry_rows((2 ** 16, 2 ** 15), (1, 1), np.zeros(2 ** 16), (np.zeros(2 ** 16), np.zeros(2 ** 16)))
    with bad('two-dimensional integer'):
        up.cell_runs_rows(np.zeros(3, np.int32), 2)
    with bad('outside'):
        up.cell_runs_rows(np.array([[0, 2]], np.int32), 2)
    with bad('size must be'):
        up.cell_table_rows(origin, scale, C, 0)
    with bad('outputs'):
        up.sums_rows(v, rows, (origin, scale), W, outputs=('mean',))
    with bad('outputs'):
        up.aggregate_rows(v, rows, (origin, scale), W, outputs=('num',))
    with bad('area'):
        up.sums_rows(v, rows, (origin, scale), W, area=np.ones(R - 1))
    with bad('min_fraction'):
        up.aggregate_rows(v, rows, (origin, scale), W, min_fraction=-1)
    with bad('float32 or float64'):
        up.sums_rows(np.zeros((R, C), np.int32), rows, (origin, scale), W)
    with bad('uint8'):
        up.majority_rows(cls.astype(np.int32), rows, (origin, scale), W)
    with bad('valid'):
        up.majority_rows(cls, rows, (origin, scale), W, valid=(32,))
    with bad('may lap'):
        up.majority_rows(cls, rows, (origin, scale), W, wrap=True)


def test_the_entry_points_refuse_before_they_touch_a_device():
    import mod16
    import mod16_amd
    assert mod16.upscale_sums is mod16_amd.upscale_sums
    origin, scale = np.zeros(4), np.full(4, 0.1)
    pos4 = np.array([0.0, 0.2, 1.0, 1.2])
    for call in (mod16_amd.upscale_fields, mod16_amd.upscale_sums):
        with bad('exactly one of col_pos and col_affine'):
            call(np.ones((4, 6)), (2, 3), pos4, np.zeros(6), col_affine=(origin, scale))
        with bad('exactly one of col_pos and col_affine'):
            call(np.ones((4, 6)), (2, 3), pos4)
        with bad('exactly one of col_pos and col_affine'):
            call(np.ones((4, 6)), (2, 3), pos4, np.zeros(6), col_range=(np.zeros(4, np.int32), np.ones(4, np.int32)))
        with bad('may lap'):
            call(np.ones((4, 60)), (2, 3), pos4, col_affine=(origin, scale), wrap=True)
        with bad('outputs'):
            call(np.ones((4, 6)), (2, 3), pos4, col_affine=(origin, scale), outputs=('median',))
    with bad('exactly one of col_pos and col_affine'):
        mod16_amd.upscale_classes(np.zeros((4, 6), np.uint8), (2, 3), pos4, np.zeros(6), col_affine=(origin, scale))
    with bad('leaves'):
        mod16_amd.upscale_classes(np.zeros((4, 6), np.uint8), (2, 3), pos4, col_affine=(origin, scale),
                                  col_range=(np.zeros(4, np.int32), np.full(4, 7, np.int32)))


def test_the_new_symbols_are_in_the_header_and_the_prototypes():
    from mod16_amd import _lib
    raw = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    assert _lib.ABI_VERSION == 16 and re.search(r'#define\s+MOD16_ABI_VERSION\s+16\b', raw)
    kinds = {'mod16_ctx*': _lib.C.c_void_p, 'int32_t': _lib.C.c_int32, 'int64_t': _lib.C.c_int64, 'int': _lib.C.c_int,
             'size_t': _lib.C.c_size_t, 'double': _lib.C.c_double}
    for name in ('mod16_upscale_create_rows', 'mod16_upscale_sums_f32', 'mod16_upscale_sums_f64'):
        m = re.search(r'MOD16_API\s+int\s+%s\s*\(([^)]*)\)' % name, text)
        assert m, name
        restype, argtypes = _lib.PROTOTYPES[name]
        params = [' '.join(p.split()) for p in m.group(1).split(',')]
        assert restype is _lib.C.c_int and len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            kind = p.rsplit(' ', 1)[0].replace('const ', '')
            if kind == 'mod16_upscale_spec*':
                assert t is _lib.C.POINTER(_lib.UpscaleSpec), (name, p)
            elif kind == 'mod16_upscale**':
                assert t is _lib.C.POINTER(_lib.C.c_void_p), (name, p)
            elif kind.endswith('*'):
                assert t is _lib.C.c_void_p, (name, p)
            else:
                assert t is kinds[kind], (name, p)
    assert len(_lib.PROTOTYPES['mod16_upscale_create_rows'][1]) == 10 and len(_lib.PROTOTYPES['mod16_upscale_sums_f32'][1]) == 21
    assert len(_lib.PROTOTYPES['mod16_upscale_create'][1]) == 8 and len(_lib.PROTOTYPES['mod16_upscale_f32'][1]) == 19
    assert len(_lib.PROTOTYPES['mod16_upscale_classes'][1]) == 12
    comment = [c for c in re.findall(r'/\*.*?\*/', raw, flags=re.S) if 'mod16_upscale_create_rows' in c]
    assert comment and all('added under ABI 16, new symbols only' in c for c in comment[:1])
    assert up.OUTPUT_NAMES == ('mean', 'fraction', 'count') and up.CLASS_OUTPUT_NAMES == ('cls', 'share')
    assert up.Upscaled._fields == up.OUTPUT_NAMES and up.UpscaledClasses._fields == up.CLASS_OUTPUT_NAMES
