"""GPU tests of the GEOMETRY of the downscaled forward run (mod16_et_downscaled_*, mod16_downscale_fields_*,
mod16_downscale_create): its index arithmetic at the widths, ranges and coarse shapes at which it takes
another path. tests/test_gpu_downscale.py checks the values at one geometry (37 x 53 over 5 x 7); this
file keeps the values simple and moves the geometry. The reference is always the numpy definition
(mod16_amd.downscale: corner_tables + interpolate; for ET, RasterEngine.run on the drivers it
materialises), the comparison bit for bit (parity.same_bits); the one exception is the 'cos4' weight
of the library's own tables (section 4).

What was not exercised before, and why it matters:

* the q = 0 / 1 regime. ds_corners splits `col0 + lane` into a row carry q and a column by a 32-bit
  division. At C = 53 a batch of 256 pixels spans five or six rows and q is never 0 for a whole
  batch; at C >= 256 q is 0 or 1, at C = 255 / 256 / 257 a batch boundary walks through the row
  boundary, and at C = 1000 whole batches lie inside one row. Fine shapes (3, 255), (3, 256), (3, 257),
  (2, 1000), (1, 300).
* C = 1 and R = 1: q = lane (every lane its own row), and a raster that is one row. (300, 1), (257, 3),
  (1, 300), (1, 1).
* aliased cells. On a coarse axis of one cell both corners are the same cell: the kernel reads one
  address twice. By the definition the far weight of a HELD axis of one cell is 0 (p is clamped to 0,
  f = 0: i0 == i1, w0 = 1, w1 = 0, asserted), so `i0 == i1 with w1 != 0` exists on a WRAPPED axis of one
  cell only (W = 1 with wrap: p = pos - floor(pos), both weights on cell 0, asserted). Coarse shapes
  (1, 1), (1, 7), (5, 1), (2, 2) next to (5, 7).
* ranges inside a row: `first` on the last column of a row (C - 1), on the first column of the next
  (C), behind it (C + 1), on both sides of a batch boundary (255, 256), and a range that begins and
  ends inside row 1 of the 1000-wide raster.
* the two ends of the mask of coarse drivers: `lw_net_day` alone (bit 0), `lai` alone (bit 13), all 14.
* the domain guard at C = 300: ds_redo_kernel finds its pixels by the marker and divides once per
  pixel; the marked pixels lie on both sides of a batch boundary and of a row boundary.
* pitched HOST planes: ds_upload_planes' copy per row (coarse_pitch != W), values checked, float64 and
  float32, from numpy arrays that end with the last row's W elements.
* the HOST `fields` tile cut: 32 MiB / (F x sizeof T) pixels, `first + t.off` and the output pitch
  re-based per tile; F = 16, float64, three tiles (the last of 37 pixels), and F = 1 in one tile.
* the library's own tables (mod16_downscale_create -> ds_axis_tables, what a C caller gets; Python
  always sends numpy's): read back exactly through the kernel. On an axis whose OTHER axis has one
  cell (weights 1 and 0) ds_interp returns `w0 * v[i0] + w1 * v[i1]`: a one-hot plane per cell returns
  the weights unchanged (w * 1.0, + 0.0), a plane that is NaN in one cell and 0 elsewhere shows exactly
  which cells carry weight, a plane of the cell indices under 'nearest' returns the index. A WRAPPED
  axis of one cell returns (1 - w1) + w1, which is 1.0 for every w1 in [0, 1]: there the weights cannot
  be observed, and the test asserts the 1.0.

Section 4's 'cos4' bound. 'nearest' and 'bilinear' weights are compared bit for bit. numpy's cosine of
an array is not the C library's, so the 'cos4' weights are held to the formula itself: b / (a + b), a =
cos(pi/2 f)^4, b = sin(pi/2 f)^4 in mpmath at 50 digits on the float64 f. The absolute error of numpy's
w1 against it is measured in the test, in units of 2^-53, over the test's own positions; the library's
may be at most twice that (one rounding each in two cosines, two powers and a division on both
sides; the factor allows for another libm). Absolute, not relative: towards f -> 0 the definition
loses all relative accuracy in b (1 - f cancels), a property of the definition. Measured on an
MI355X host, the largest over the axes and sizes (the wrapped columns of 7 cells), in units of 2^-53:
numpy 3.227, the library 3.227; wrapped columns of 2 cells: 3.001 and 3.001; the held axes: numpy
2.236 / 2.730 (2 / 7 cells), the library 2.229 / 2.730; the library's w1 differs from numpy's by at
most 2."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import synth
import parity

pytestmark = pytest.mark.gpu

FINE = ((1, 1), (1, 300), (300, 1), (3, 255), (3, 256), (3, 257), (2, 1000), (257, 3))
COARSE = ((1, 1), (1, 7), (5, 1), (2, 2), (5, 7))
METHODS = ('nearest', 'bilinear', 'cos4')
POISON = -7.0
PAD = 5                              # elements of poison behind every output row
MARK64 = 0x7ff80000000d05ca          # DsMark<double>, csrc/mod16_downscale.hpp
INSIDE_ROW = (1000 + 123, 600)       # row 1 of the 1000-wide raster, columns 123 ... 722: three batches


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    from mod16_amd import downscale as ds
    return torch, mod16_amd, _lib, ds


@functools.lru_cache(maxsize=None)
def table():
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    t = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def engine(dtype='float64', exact=False):
    from mod16_amd import _lib
    from mod16_amd.raster import RasterEngine
    return RasterEngine(table(), dtype=dtype, math=_lib.MATH_EXACT if exact else _lib.MATH_FAST)


# --- positions ------------------------------------------------------------------------------------

def axis_start_step(count, size):
    """Positions `start + k * step` of an axis of `count` fine entries over `size` cells, dyadic (so
    that `positions` is exact and cell centres are hit exactly): from 1.25 cells in front of one
    period in front of the grid to at least 1.25 cells behind two periods behind it."""
    span = 3.0 * size + 2.5
    step = 2.0 ** int(np.ceil(np.log2(span / (count - 1))))
    assert step <= 0.25
    return -(size + 1.25), step


@functools.lru_cache(maxsize=None)
def axis_positions(count, size, descending):
    """The position table of one axis. Long axes (count >= 255): a regular grid through
    mod16_amd.downscale.positions -- with a negative coarse_step (a north-to-south latitude) where
    `descending` -- that reaches outside the coarse grid on both sides, passes several seams of a
    wrapped axis and holds cell centres exactly (asserted). Short axes cannot hold all of that: 1
    entry lies between cells 0 and 1 (nearer to 1), 2 in front of the grid and there, 3 a period and
    more in front of the grid, on the centre of cell 1 and two periods behind the grid."""
    from mod16_amd import downscale as ds
    if count == 1:
        pos = np.array([0.625])
    elif count == 2:
        pos = np.array([-1.25, 0.625])
    elif count == 3:
        pos = np.array([-size - 1.25, min(1.0, size - 1.0), 2.0 * size + 0.375])
    else:
        start, step = axis_start_step(count, size)
        if descending:          # coordinates fall from 10 - 2 start in steps of 2 step; cell 0 at 10, cells 2 apart
            pos = ds.positions(10.0 - 2.0 * start, -2.0 * step, count, 10.0, -2.0)
        else:
            pos = ds.positions(start, step, count, 0.0, 1.0)
        assert np.array_equal(pos, start + step * np.arange(count))
        assert pos.min() < -1 and pos.max() > size                         # outside on both sides
        assert len(np.unique(np.floor(pos / size))) >= 3                   # several seams under wrap
        centre = (pos == np.round(pos)) & (pos >= 0) & (pos <= size - 1)
        assert centre.any() and not centre.all()                          # cell centres, exactly
    pos.setflags(write=False)
    return pos


def tables(ds, shape, coarse_shape, wrap, method):
    """(row_pos, col_pos, row tables, column tables) of a fine shape over a coarse one: the rows descend."""
    row_pos = axis_positions(shape[0], coarse_shape[0], True)
    col_pos = axis_positions(shape[1], coarse_shape[1], False)
    return (row_pos, col_pos, ds.corner_tables(row_pos, coarse_shape[0], False, method),
            ds.corner_tables(col_pos, coarse_shape[1], wrap, method))


def check_aliasing(rt, ct, coarse_shape, wrap):
    """An axis of one cell reads one cell twice. Held: the far weight is 0 by the definition. Wrapped
    (the columns only): it is not."""
    H, W = coarse_shape
    if H == 1:
        assert (rt[0] == rt[1]).all() and (rt[3] == 0).all() and (rt[2] == 1).all()
    if W == 1 and not wrap:
        assert (ct[0] == ct[1]).all() and (ct[3] == 0).all() and (ct[2] == 1).all()
    if W == 1 and wrap:
        assert (ct[0] == ct[1]).all() and (ct[3] != 0).any()
        return True
    return False


def ranges(shape):
    """(first, n) of the whole raster and of every range of the issue's list that fits it."""
    R, C = shape
    N = R * C
    cand = [(0, N), (0, 1), (C - 1, 2), (C, 1), (C + 1, 255), (255, 2), (256, 257)]
    if C == 1000:
        cand.append(INSIDE_ROW)
    out = []
    for first, n in cand:
        if first + n <= N and (first, n) not in out:
            out.append((first, n))
    for first, n in out:
        if (first, n) == (C - 1, 2):
            assert first // C + 1 == (first + n - 1) // C                  # really crosses a row boundary
        if (first, n) == INSIDE_ROW:
            assert first // C == (first + n - 1) // C == 1 and first % C and (first + n) % C and n > 2 * 256
    return out


# --- 1. fields against the definition ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def coarse_planes(coarse_shape, dtype):
    """16 coarse planes (F, H, W) in `dtype`: plane 1 holds a NaN, plane 2 an infinity, in cell (1, 1)
    (row / column 0 on an axis of one cell), which every fine shape's positions give weight."""
    H, W = coarse_shape
    _, a = synth.drivers((H, W), seed=7, special=False)
    _, b = synth.drivers((H, W), seed=8, special=False)
    planes = np.stack((a + b)[:16])
    planes[1, min(1, H - 1), min(1, W - 1)] = np.nan
    planes[2, min(1, H - 1), min(1, W - 1)] = np.inf
    planes = planes.astype(dtype)
    planes.setflags(write=False)
    return planes


@pytest.mark.parametrize('shape', FINE, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_fields_equal_the_definition_over_shapes_and_ranges(env, dtype, method, wrap, shape):
    torch, mod16_amd, _lib, ds = env
    eng = engine(dtype)
    R, C = shape
    N = R * C
    aliased, launches = 0, 0
    for coarse_shape in COARSE:
        H, W = coarse_shape
        row_pos, col_pos, rt, ct = tables(ds, shape, coarse_shape, wrap, method)
        aliased += check_aliasing(rt, ct, coarse_shape, wrap)
        planes = coarse_planes(coarse_shape, dtype)
        with np.errstate(all='ignore'):
            want = np.stack([ds.interpolate(p, rt, ct).reshape(-1) for p in planes]).astype(dtype)
        assert want.shape == (16, N)
        if N >= 255:          # the NaN and the infinity reach pixels, and do not reach all of them
            assert np.isnan(want[1]).any() and np.isinf(want[2]).any() and np.isfinite(want[0]).all()
            if coarse_shape == (5, 7):
                assert np.isfinite(want[1]).any() and np.isfinite(want[2]).any()
        dev = torch.from_numpy(np.array(planes)).to(eng._dev())
        grid = eng.downscale_grid(shape, coarse_shape, row_pos, col_pos, wrap=wrap, method=method)
        for F in (1, 3, 16):
            for first, n in ranges(shape):
                buf = torch.full((F, n + PAD), POISON, dtype=eng.dtype, device=eng._dev())
                out = grid.fields([dev[f] for f in range(F)], first_pixel=first, n=n, out=buf[:, :n])
                eng.check()
                got = buf.cpu().numpy()
                what = '%s over %s, F = %d, pixels [%d, %d)' % (shape, coarse_shape, F, first, first + n)
                assert out.data_ptr() == buf.data_ptr()
                assert parity.same_bits(got[:, :n], want[:F, first:first + n]), what
                assert (got[:, n:] == POISON).all(), what
                launches += 1
        grid.close()
    assert aliased == (2 if wrap else 0)                 # W = 1 of (1, 1) and (5, 1)
    assert launches == 3 * len(COARSE) * len(ranges(shape))


# --- 2. run at the same edges -----------------------------------------------------------------------

# fine shape -> (coarse shape, coarse drivers (None: the eleven meteorological ones, 'all': all 14), method, wrap)
RUN_CASES = {
    (1, 1): ((5, 7), ('lai',), 'bilinear', False),
    (1, 300): ((1, 7), None, 'cos4', True),
    (300, 1): ((5, 1), None, 'bilinear', True),
    (3, 255): ((1, 1), None, 'cos4', True),
    (3, 256): ((5, 7), 'all', 'nearest', False),
    (3, 257): ((5, 7), None, 'cos4', True),
    (2, 1000): ((1, 7), None, 'bilinear', True),
    (257, 3): ((5, 1), ('lw_net_day',), 'nearest', True),
}
RANGED = ((3, 257), (2, 1000))


@functools.lru_cache(maxsize=None)
def run_inputs(shape, coarse_shape):
    """(cls, the 14 fine drivers, the 14 coarse ones): oracle.synth, the fine ones with its special
    values (NaN, 0 and 1 in fPAR / LAI, classes without parameters)."""
    cls, fine = synth.drivers(shape, seed=63, special=True)         # (a seed whose raster of ONE pixel has a result)
    _, coarse = synth.drivers(coarse_shape, seed=64, special=False)
    for a in [cls] + fine + coarse:
        a.setflags(write=False)
    return cls, tuple(fine), tuple(coarse)


def pick(ds, fine, coarse, names):
    out = [c if name in names else f for name, f, c in zip(ds.DRIVER_NAMES, fine, coarse)]
    if 'sw_rad_night' not in names:
        out[3] = 0.0
    return out


def materialise(ds, drivers, names, rt, ct):
    return [ds.interpolate(d, rt, ct) if name in names else d for name, d in zip(ds.DRIVER_NAMES, drivers)]


def put(torch, eng, a):
    return torch.from_numpy(np.array(a, eng.np_dtype)).to(eng._dev()) if isinstance(a, np.ndarray) else a


def run_step(torch, eng, cls, drivers):
    out = eng.run(torch.from_numpy(np.array(cls)).to(eng._dev()).reshape(-1),
                  [put(torch, eng, d).reshape(-1) if isinstance(d, np.ndarray) else d for d in drivers])
    eng.check()
    return [o.cpu().numpy() for o in out]


def run_grid(torch, ds, eng, grid, cls, drivers, names, first, n):
    """DownscaleGrid.run on numpy inputs, pixels [first, first + n), into poisoned outputs -> numpy (day, night)"""
    dev = []
    for name, d in zip(ds.DRIVER_NAMES, drivers):
        if not isinstance(d, np.ndarray):
            dev.append(d)
        elif name in names:
            dev.append(put(torch, eng, d))
        else:
            dev.append(put(torch, eng, d.reshape(-1)[first:first + n]))
    c = torch.from_numpy(np.array(cls).reshape(-1)[first:first + n]).to(eng._dev())
    day = torch.full((n,), POISON, dtype=eng.dtype, device=eng._dev())
    night = torch.full((n,), POISON, dtype=eng.dtype, device=eng._dev())
    grid.run(c, dev, coarse=names, first_pixel=first, out_day=day, out_night=night)
    eng.check()
    return [day.cpu().numpy(), night.cpu().numpy()]


def both_kinds(day):
    """Pixels with a result and pixels without one both take part (a raster of one pixel: it has one)."""
    if day.size >= 255:
        assert 0.9 < np.isfinite(day).mean() < 1.0
    else:
        assert np.isfinite(day).all() and (day != 0).all()


def check_run(env, shape, dtype, exact):
    torch, mod16_amd, _lib, ds = env
    coarse_shape, names, method, wrap = RUN_CASES[shape]
    names = ds.MET_DRIVERS if names is None else ds.DRIVER_NAMES if names == 'all' else names
    N = shape[0] * shape[1]
    cls, fine, coarse = run_inputs(shape, coarse_shape)
    row_pos, col_pos, rt, ct = tables(ds, shape, coarse_shape, wrap, method)
    assert check_aliasing(rt, ct, coarse_shape, wrap) == (coarse_shape[1] == 1 and wrap)
    drivers = pick(ds, fine, coarse, names)
    if dtype == 'float32':
        drivers = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in drivers]
    wide = [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in drivers]
    # the reference: the step of the same arithmetic on the drivers numpy materialises, in float64
    # (a float32 engine computes in float64 and rounds once)
    want = run_step(torch, engine('float64', exact), cls, materialise(ds, wide, names, rt, ct))
    both_kinds(want[0])
    with np.errstate(all='ignore'):
        want = [w.astype(dtype) for w in want]
    eng = engine(dtype, exact)
    grid = eng.downscale_grid(shape, coarse_shape, row_pos, col_pos, wrap=wrap, method=method)
    todo = ranges(shape) if shape in RANGED else [(0, N)]
    assert len(todo) == (8 if shape == (2, 1000) else 7 if shape == (3, 257) else 1)
    for first, n in todo:
        got = run_grid(torch, ds, eng, grid, cls, drivers, names, first, n)
        for g, w, what in zip(got, want, ('day', 'night')):
            assert g.dtype == np.dtype(dtype)
            assert parity.same_bits(g, w[first:first + n]), \
                '%s %s over %s, pixels [%d, %d), %s' % (what, shape, coarse_shape, first, first + n, method)
    grid.close()


@pytest.mark.parametrize('shape', FINE, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('exact', [False, True])
def test_run_has_the_bits_of_the_step_at_every_fine_shape(env, exact, shape):
    check_run(env, shape, 'float64', exact)


@pytest.mark.parametrize('shape', FINE, ids=lambda s: '%dx%d' % s)
def test_run_float32_at_every_fine_shape(env, shape):
    check_run(env, shape, 'float32', False)


def test_run_cases_cover_what_they_claim(env):
    torch, mod16_amd, _lib, ds = env
    assert set(RUN_CASES) == set(FINE)
    assert {c[0] for c in RUN_CASES.values()} == {(1, 1), (5, 1), (1, 7), (5, 7)}
    assert {c[2] for c in RUN_CASES.values()} == set(METHODS)
    names = [c[1] for c in RUN_CASES.values()]
    assert names.count('all') == 1 and names.count(None) == 5
    assert (ds.DRIVER_NAMES[-1],) in names and (ds.DRIVER_NAMES[0],) in names      # the two ends of the mask


def test_domain_guard_across_a_batch_and_a_row_boundary(env):
    """C = 300: a coarse temp_day cell of 1400 K under 'nearest' marks fine columns 235 ... 277 of
    fine rows 0 and 1 -- pixels 255 and 256 (a batch boundary of the first kernel and of the one
    behind it) and both sides of the row boundary at pixel 300."""
    torch, mod16_amd, _lib, ds = env
    shape, coarse_shape = (5, 300), (5, 7)
    N = 1500
    cls, fine, coarse = run_inputs(shape, coarse_shape)
    row_pos = np.array([0.75, 1.25, 2.0, 3.125, 4.5])
    col_pos = np.arange(300) * (3.0 / 128) - 1.0
    rt, ct = ds.corner_tables(row_pos, 5, False, 'nearest'), ds.corner_tables(col_pos, 7, False, 'nearest')
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    base = list(drivers)
    drivers[5] = drivers[5].copy()
    drivers[5][1, 5] = 1400.0
    eng = engine()
    dense = materialise(ds, drivers, ds.MET_DRIVERS, rt, ct)
    marked = np.flatnonzero(dense[5].reshape(-1) == 1400.0)
    assert set(marked // 300) == {0, 1} and set(marked % 300) == set(range(235, 278))
    assert {255, 256} <= set(marked) and {0, 1} <= set(marked // 256)            # a batch boundary
    assert marked.min() < 300 <= marked.max() and 299 not in marked and 300 not in marked
    want = run_step(torch, eng, cls, dense)
    both_kinds(want[0])
    grid = eng.downscale_grid(shape, coarse_shape, row_pos, col_pos, wrap=False, method='nearest')
    got = run_grid(torch, ds, eng, grid, cls, drivers, ds.MET_DRIVERS, 0, N)
    plain = run_grid(torch, ds, eng, grid, cls, base, ds.MET_DRIVERS, 0, N)
    for g, w in zip(got, want):
        assert parity.same_bits(g[marked], w[marked]) and parity.same_bits(g, w)
        assert not (g.view(np.uint64) == MARK64).any()
    rest = np.setdiff1d(np.arange(N), marked)
    assert parity.same_bits(got[0][rest], plain[0][rest]) and not parity.same_bits(got[0], plain[0])
    # a range from behind the marked pixels of row 0: its first batch ends among those of row 1
    first, n = 290, 400
    assert {first + 255, first + 256} <= set(marked)
    got = run_grid(torch, ds, eng, grid, cls, drivers, ds.MET_DRIVERS, first, n)
    for g, w in zip(got, want):
        assert parity.same_bits(g, w[first:first + n]) and not (g.view(np.uint64) == MARK64).any()
    grid.close()


# --- 3. HOST mode values ----------------------------------------------------------------------------

def pitched(plane, pitch, dtype):
    """A coarse plane as a host array whose rows lie `pitch` elements apart, NaN between them, and
    which ENDS with the last row's W elements -> (the array that owns the memory, the (H, W) view)"""
    H, W = plane.shape
    mem = np.full((H - 1) * pitch + W, np.nan, dtype)
    view = np.lib.stride_tricks.as_strided(mem, (H, W), (pitch * mem.itemsize, mem.itemsize))
    view[...] = plane
    assert np.isnan(mem).sum() == (H - 1) * (pitch - W) + np.isnan(plane).sum()
    return mem, view


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_host_run_with_pitched_planes(env, dtype):
    """_lib.Downscale.run, where=HOST, numpy addresses, coarse planes W + 3 apart: the bits of the
    DEVICE call and of the step on the materialised drivers. 37 x 53 over 5 x 7, pixels [100, 1600):
    the range begins in column 47 of row 1."""
    torch, mod16_amd, _lib, ds = env
    shape, coarse_shape, names, method = (37, 53), (5, 7), ('sw_albedo', 'temp_day', 'vpd_day', 'pressure', 'lai'), 'cos4'
    H, W = coarse_shape
    first, n = 100, 1500
    assert first % shape[1] and first + n < shape[0] * shape[1]
    cls, fine, coarse = run_inputs(shape, coarse_shape)
    row_pos = ds.positions(-0.8, 0.17, shape[0], 0.0, 1.0)
    col_pos = ds.positions(-9.3, 0.41, shape[1], 0.0, 1.0)
    rt, ct = ds.corner_tables(row_pos, H, False, method), ds.corner_tables(col_pos, W, True, method)
    drivers = [a.astype(dtype) if isinstance(a, np.ndarray) else a for a in pick(ds, fine, coarse, names)]
    wide = [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in drivers]
    want = run_step(torch, engine(), cls, materialise(ds, wide, names, rt, ct))
    both_kinds(want[0])
    with np.errstate(all='ignore'):
        want = [w.astype(dtype)[first:first + n] for w in want]
    eng = engine(dtype)
    grid = eng.downscale_grid(shape, coarse_shape, row_pos, col_pos, wrap=True, method=method)
    device = run_grid(torch, ds, eng, grid, cls, drivers, names, first, n)
    grid.close()
    torch.cuda.synchronize()
    keep, ptrs, kinds = [], [], []
    for name, d in zip(ds.DRIVER_NAMES, drivers):
        if name in names:
            mem, view = pitched(d, W + 3, dtype)
            assert view.strides[0] == (W + 3) * mem.itemsize
            kinds.append(ds.KIND_COARSE)
        elif isinstance(d, np.ndarray):
            mem = np.ascontiguousarray(d.reshape(-1)[first:first + n])
            kinds.append(ds.KIND_FINE)
        else:
            mem = np.array([d], dtype)
            kinds.append(ds.KIND_SCALAR)
        keep.append(mem)
        ptrs.append(mem.ctypes.data)
    assert kinds.count(ds.KIND_COARSE) == 5 and kinds.count(ds.KIND_SCALAR) == 1
    c = np.ascontiguousarray(cls.reshape(-1)[first:first + n])
    outs = [np.full(n + PAD, POISON, dtype) for _ in range(2)]
    low = _lib.Downscale(eng.ctx, shape, coarse_shape, row_pos, col_pos, wrap=True, method=method)
    low.run(dtype, c.ctypes.data, ptrs, kinds, W + 3, first, n, outs[0].ctypes.data, outs[1].ctypes.data,
            flags=_lib.MATH_FAST, where=_lib.HOST)
    low.close()
    for o, d, w, what in zip(outs, device, want, ('day', 'night')):
        assert parity.same_bits(o[:n], d), what
        assert parity.same_bits(o[:n], w), what
        assert (o[n:] == POISON).all(), what


@pytest.mark.parametrize('F,n', [(16, 2 * 262144 + 37), (1, 1000)])
def test_host_fields_across_its_own_tiles(env, F, n):
    """_lib.Downscale.fields, where=HOST, float64. F = 16: the tile is 32 MiB / (16 x 8 B) = 262 144
    pixels, n = 2 tiles and 37 pixels of a third from a `first` that is no multiple of 256; F = 1: one
    tile. Pitched planes, a pitched output with poison behind every row; the bits of interpolate."""
    torch, mod16_amd, _lib, ds = env
    shape, coarse_shape, method = (683, 768), (5, 7), 'cos4'
    H, W = coarse_shape
    first = 131
    tile = min((32 << 20) // (F * 8) // 256 * 256, 1 << 21)          # (at most the tile of every HOST call)
    assert first % 256 and first % shape[1] and first + n <= shape[0] * shape[1]
    assert (F, tile, -(-n // tile)) in ((16, 262144, 3), (1, 1 << 21, 1)) and (F == 1 or n % tile == 37)
    row_pos = ds.positions(4.6, -5.6 / shape[0], shape[0], 0.0, 1.0)            # descending, beyond both edges
    col_pos = ds.positions(-9.3, 3.0 * W / shape[1], shape[1], 0.0, 1.0)       # three periods
    rt, ct = ds.corner_tables(row_pos, H, False, method), ds.corner_tables(col_pos, W, True, method)
    planes = coarse_planes(coarse_shape, 'float64')[:F]
    eng = engine()
    torch.cuda.synchronize()
    keep = [pitched(p, W + 3, 'float64') for p in planes]
    out = np.full((F, n + PAD), POISON)
    low = _lib.Downscale(eng.ctx, shape, coarse_shape, row_pos, col_pos, wrap=True, method=method)
    low.fields('float64', [mem.ctypes.data for mem, _ in keep], W + 3, first, n, out.ctypes.data, n + PAD, where=_lib.HOST)
    low.close()
    assert (out[:, n:] == POISON).all()
    for f in range(F):
        want = ds.interpolate(planes[f], rt, ct).reshape(-1)[first:first + n]
        assert parity.same_bits(out[f, :n], want), 'field %d' % f
        if f == 1:
            assert np.isnan(want).any() and np.isfinite(want).any()


# --- 4. the library's own tables --------------------------------------------------------------------

def table_positions(size):
    """The positions at which mod16_downscale_create's tables are compared with corner_tables'."""
    rng = np.random.default_rng(4)
    special = [0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), 0.0, -0.0, size - 1.0, -0.75, -3.5,
               size - 0.5, size + 2.25, -1e-17, float(size), np.nextafter(float(size), 0.0), 1e15, -1e15, 1e-300,
               1.0 - 2.0 ** -53]
    pos = np.concatenate([np.arange(size, dtype=np.float64), special, rng.uniform(-2.0 * size - 1, 3.0 * size + 1, 2000),
                          rng.uniform(-1.0, size, 1000)])
    assert np.signbit(pos[size + 4]) and pos[size + 4] == 0
    return pos


@functools.lru_cache(maxsize=None)
def cos4_reference(f):
    """b / (a + b), a = cos(pi/2 f)^4, b = sin(pi/2 f)^4, at 50 digits on the float64 f -> mpf"""
    import mpmath
    with mpmath.workdps(50):
        x = mpmath.pi / 2 * mpmath.mpf(f)
        a, b = mpmath.cos(x) ** 4, mpmath.sin(x) ** 4
        return b / (a + b)


def cos4_error(w1, f):
    """The largest |w1 - reference| over the entries with f != 0, in units of 2^-53"""
    import mpmath
    worst = 0.0
    with mpmath.workdps(50):
        for w, x in zip(w1.tolist(), f.tolist()):
            if x != 0.0:
                worst = max(worst, float(abs(mpmath.mpf(w) - cos4_reference(x)) * 2 ** 53))
    return worst


def library_axis(torch, _lib, ds, eng, pos, size, rows, wrap, method):
    """The library's OWN tables of one axis (mod16_downscale_create), seen through the fields kernel on
    an n x 1 (rows) or 1 x n raster whose other axis has one cell (weights 1 and 0). Planes: a one-hot
    plane per cell, a plane per cell that is NaN there and 0 elsewhere, the cells' indices.
    -> (onehot (size, n), carries weight (size, n) bool, index plane (n,), numpy's interpolation of
    the same planes (2 size + 1, n) by corner_tables)"""
    n = len(pos)
    one = np.zeros(1)
    shape, coarse_shape = ((n, 1), (size, 1)) if rows else ((1, n), (1, size))
    eye = np.eye(size)
    planes = np.concatenate([eye, np.where(eye == 1, np.nan, 0.0), np.arange(size, dtype=np.float64)[None]])
    planes = planes.reshape((2 * size + 1,) + coarse_shape)
    F = len(planes)
    assert F <= 16
    spec = _lib.DownscaleSpec(shape[0], shape[1], coarse_shape[0], coarse_shape[1], int(wrap), ds.method_code(method))
    row_pos, col_pos = (np.ascontiguousarray(pos), one) if rows else (one, np.ascontiguousarray(pos))
    handle = ctypes.c_void_p()
    ctx = eng.ctx
    ctx.check(ctx.lib.mod16_downscale_create(ctx.handle, ctypes.byref(spec), row_pos.ctypes.data, col_pos.ctypes.data,
                                             ctypes.byref(handle)))
    dev = torch.from_numpy(planes).to(eng._dev())
    out = torch.full((F, n + PAD), POISON, dtype=torch.float64, device=eng._dev())
    cell = coarse_shape[0] * coarse_shape[1] * 8
    try:
        ctx.check(ctx.lib.mod16_downscale_fields_f64(ctx.handle, handle, _lib.ptr_array([dev.data_ptr() + f * cell for f in range(F)]),
                                                     F, coarse_shape[1], 0, n, out.data_ptr(), n + PAD, _lib.DEVICE, eng._stream()))
        eng.check()
    finally:
        ctx.lib.mod16_downscale_destroy(handle)
    got = out.cpu().numpy()
    assert (got[:, n:] == POISON).all()
    got = got[:, :n]
    # the same planes through numpy's tables (the other axis: one cell, position 0)
    axis = ds.corner_tables(pos, size, wrap and not rows, method)
    other = ds.corner_tables(one, 1, False, method)
    rt, ct = (axis, other) if rows else (other, axis)
    want = np.stack([ds.interpolate(p, rt, ct).reshape(-1) for p in planes])
    return got[:size], np.isnan(got[size:2 * size]), got[2 * size], want


@pytest.mark.parametrize('size', [1, 2, 7])
@pytest.mark.parametrize('axis', ['rows', 'columns', 'columns-wrapped', 'rows-of-a-wrapped-grid'])
def test_the_librarys_own_tables_equal_corner_tables(env, axis, size):
    """mod16_downscale_create's tables (ds_axis_tables, C++) against corner_tables (numpy): indices,
    'nearest' and 'bilinear' weights bit for bit, 'cos4' weights within twice numpy's own error
    against the formula at 50 digits (module docstring). The rows never wrap, whatever wrap_cols says."""
    torch, mod16_amd, _lib, ds = env
    eng = engine()
    rows = axis.startswith('rows')
    flag = axis in ('columns-wrapped', 'rows-of-a-wrapped-grid')
    wrap = flag and not rows
    pos = table_positions(size)
    n = len(pos)
    cells = np.arange(size)[:, None]
    i0, i1, _, f = ds.corner_tables(pos, size, wrap, 'bilinear')          # f: the fraction behind every weight
    assert (f == 0).sum() >= size and (f != 0).sum() > (2900 if wrap else 300 if size > 1 else -1)
    if wrap:
        assert i0[list(pos).index(-1e-17)] == 0 and f[list(pos).index(-1e-17)] == 0      # rounds up to `size`: cell 0
    observable = i0 != i1                      # two cells: their one-hot planes return w0 and w1 unchanged
    assert observable.any() == (size > 1) and (observable.all() == (size > 1 and wrap))
    at = np.arange(n)
    for method in METHODS:
        onehot, carries, index, want = library_axis(torch, _lib, ds, eng, pos, size, rows, flag, method)
        n0, n1, w0, w1 = ds.corner_tables(pos, size, wrap, method)
        assert np.array_equal(n0, i0) and np.array_equal(n1, i1)
        # indices: exactly the cells that carry weight by numpy's tables carry weight (a NaN there reaches the pixel)
        expect = ((cells == i0) & (w0 != 0)) | ((cells == i1) & (w1 != 0))
        assert np.array_equal(carries, expect), method
        assert np.array_equal(onehot != 0, expect), method
        if method == 'nearest':
            assert np.array_equal(index, np.where(w1 != 0, i1, i0).astype(np.float64))
        if method != 'cos4':
            assert parity.same_bits(np.concatenate([onehot, index[None]]), np.concatenate([want[:size], want[2 * size:]])), method
            assert np.array_equal(carries, np.isnan(want[size:2 * size]))
        if size == 1 and wrap:
            # one wrapped cell: (1 - w1) + w1, which is 1.0 whatever w1 in [0, 1] is -- the weights are not observable
            assert (w1 != 0).any() and (onehot == 1.0).all() and parity.same_bits(onehot, want[:1])
            continue
        # where the two cells alias (held at the axis' end: p is an integer, f = 0) numpy's w1 is 0 and the plane returns w0
        assert (w1[~observable] == 0).all() and (onehot[i0[~observable], at[~observable]] == 1.0).all()
        if not observable.any():
            continue
        lib_w0, lib_w1 = onehot[i0, at][observable], onehot[i1, at][observable]
        np_w0, np_w1, fo = w0[observable], w1[observable], f[observable]
        if method != 'cos4':
            assert parity.same_bits(lib_w0, np_w0) and parity.same_bits(lib_w1, np_w1), method
            continue
        # cos4: exactly 0 at f == 0 (and the far cell's NaN did not reach the pixel: `carries` above)
        assert (fo == 0).any() and (lib_w1[fo == 0] == 0).all() and (lib_w0[fo == 0] == 1).all()
        assert not carries[i1[observable], at[observable]][fo == 0].any()
        assert np.array_equal(lib_w0, 1.0 - lib_w1)
        err_numpy, err_library = cos4_error(np_w1, fo), cos4_error(lib_w1, fo)
        differ = np.abs(lib_w1 - np_w1).max() * 2 ** 53
        print('cos4 %s size %d: |w1 - reference| in units of 2^-53: numpy %.3f, library %.3f; library against numpy %.1f'
              % (axis, size, err_numpy, err_library, differ))
        assert 0 < err_numpy < 8                  # (the reference is one: a handful of roundings)
        assert err_library <= 2 * err_numpy
