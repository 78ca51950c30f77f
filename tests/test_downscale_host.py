"""The definition of the downscaled forward run (mod16_amd/downscale.py: positions, corner_tables,
interpolate, check_call) against a scalar Python loop that follows its docstrings literally. Host
only: no library, no device.

Shapes: fine grid 37 x 53 over a coarse grid 5 x 7, positions that start outside the coarse grid on
both sides (held edges / several wraps), all three methods, with and without wrap."""
import math

import numpy as np
import pytest

from mod16_amd import downscale as ds

R, C, H, W = 37, 53, 5, 7


def scalar_entry(pos, size, wrap, method):
    """One entry of corner_tables, in Python floats."""
    if wrap:
        p = pos - math.floor(pos / size) * size
        if p >= size or p < 0:        # rounded up to `size` (or, by the division's rounding, below 0)
            p = 0.0
        i0 = math.floor(p)
        f = p - i0
        i1 = (i0 + 1) % size
    else:
        p = min(max(pos, 0.0), float(size - 1))
        i0 = math.floor(p)
        f = p - i0
        i1 = min(i0 + 1, size - 1)
    if method == 'nearest':
        w1 = 1.0 if f >= 0.5 else 0.0
    elif method == 'bilinear':
        w1 = f
    else:
        # numpy's cosine and power of ARRAYS (its scalar paths call another implementation, which
        # rounds some arguments differently): one-element arrays
        a = float((np.cos((np.pi / 2) * np.array([f])) ** 4)[0])
        b = float((np.cos((np.pi / 2) * np.array([1.0 - f])) ** 4)[0])
        w1 = 0.0 if f == 0 else b / (a + b)
    return int(i0), int(i1), 1.0 - w1, w1


def scalar_interpolate(field, rt, ct):
    out = np.empty((len(rt[0]), len(ct[0])))
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            terms = []
            for ri, wr in ((rt[0][r], rt[2][r]), (rt[1][r], rt[3][r])):
                for ci, wc in ((ct[0][c], ct[2][c]), (ct[1][c], ct[3][c])):
                    w = float(wr) * float(wc)
                    terms.append(w * float(field[ri, ci]) if w != 0 else 0.0)
            out[r, c] = ((terms[0] + terms[1]) + terms[2]) + terms[3]
    return out


def grids():
    row_pos = ds.positions(-0.8, 0.17, R, 0.0, 1.0)          # -0.8 ... 5.3: beyond both edges of 5 cells
    col_pos = ds.positions(-9.3, 0.41, C, 0.0, 1.0)          # -9.3 ... 12.0: several wraps of 7 cells
    return row_pos, col_pos


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_positions():
    p = ds.positions(10.0, 0.5, 4, 9.0, 2.0)
    assert p.dtype == np.float64 and p.tolist() == [0.5, 0.75, 1.0, 1.25]
    assert ds.positions(0, 1, 0, 0, 1).shape == (0,)
    north_south = ds.positions(89.75, -0.5, 3, 90.0, -1.0)
    assert north_south.tolist() == [0.25, 0.75, 1.25]
    for bad in (0.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='coarse_step'):
            ds.positions(0, 1, 3, 0, bad)
    with pytest.raises(ValueError, match='count'):
        ds.positions(0, 1, -1, 0, 1)


@pytest.mark.parametrize('method', ds.METHODS)
@pytest.mark.parametrize('wrap', [False, True])
def test_tables_and_interpolation_follow_the_scalar_loop(method, wrap):
    row_pos, col_pos = grids()
    rt = ds.corner_tables(row_pos, H, False, method)
    ct = ds.corner_tables(col_pos, W, wrap, method)
    for pos, size, w, t in ((row_pos, H, False, rt), (col_pos, W, wrap, ct)):
        assert t[0].dtype == t[1].dtype == np.int32 and t[2].dtype == t[3].dtype == np.float64
        want = [scalar_entry(float(x), size, w, method) for x in pos]
        assert t[0].tolist() == [e[0] for e in want] and t[1].tolist() == [e[1] for e in want]
        assert np.array_equal(bits(t[2]), bits([e[2] for e in want]))
        assert np.array_equal(bits(t[3]), bits([e[3] for e in want]))
        assert np.all(t[2] + t[3] == 1.0)
        assert t[0].min() >= 0 and max(t[0].max(), t[1].max()) < size
    field = np.random.default_rng(5).normal(280.0, 30.0, (H, W))
    got = ds.interpolate(field, rt, ct)
    assert got.shape == (R, C) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(scalar_interpolate(field, rt, ct)))
    # a float32 field is widened first
    narrow = field.astype(np.float32)
    assert np.array_equal(bits(ds.interpolate(narrow, rt, ct)), bits(ds.interpolate(narrow.astype(np.float64), rt, ct)))


@pytest.mark.parametrize('method', ds.METHODS)
def test_cell_centres_ignore_the_far_corner(method):
    """Positions exactly on cell centres: f = 0, the far corner has no weight and its NaN (or
    infinity) does not reach the pixel."""
    rt = ds.corner_tables(np.arange(H, dtype=np.float64), H, False, method)
    ct = ds.corner_tables(np.arange(W, dtype=np.float64), W, False, method)
    assert np.all(rt[3] == 0.0) and np.all(rt[2] == 1.0) and rt[0].tolist() == list(range(H))
    field = np.arange(H * W, dtype=np.float64).reshape(H, W)
    assert np.array_equal(ds.interpolate(field, rt, ct), field)
    poisoned = field.copy()
    poisoned[2, 3] = np.nan
    poisoned[4, 1] = np.inf
    got = ds.interpolate(poisoned, rt, ct)
    assert np.isnan(got[2, 3]) and np.isinf(got[4, 1])
    clean = np.ones((H, W), bool)
    clean[2, 3] = clean[4, 1] = False
    assert np.array_equal(got[clean], field[clean])
    # halfway between a NaN cell and its neighbour the NaN has weight (nearest: f >= 0.5 takes the far cell)
    half = ds.corner_tables(np.array([2.5]), W, False, method)
    assert np.isnan(ds.interpolate(poisoned, (rt[0][2:3], rt[1][2:3], rt[2][2:3], rt[3][2:3]), half)[0, 0])


def test_positions_outside_hold_the_edge():
    field = np.random.default_rng(6).normal(size=(H, W))
    for method in ds.METHODS:
        rt = ds.corner_tables(np.array([-3.0, -1e-9, H - 1 + 1e-9, H + 10.0]), H, False, method)
        ct = ds.corner_tables(np.array([-0.5, W - 1.0, W - 0.5, 1e30]), W, False, method)
        assert rt[0].tolist() == [0, 0, H - 1, H - 1] and rt[1].tolist() == [1, 1, H - 1, H - 1]
        assert np.all(rt[3] == 0.0) and np.all(ct[3] == 0.0)
        got = ds.interpolate(field, rt, ct)
        assert np.array_equal(got, field[np.ix_([0, 0, H - 1, H - 1], [0, W - 1, W - 1, W - 1])])


def test_wrap_seam_and_negative_longitudes():
    field = np.random.default_rng(7).normal(size=(1, W))
    pos = np.array([W - 1.0, W - 0.75, W - 0.25, -0.25, -1.0, -W - 0.5, 2.0 * W + 1.5, -1e-300, float(W)])
    i0, i1, w0, w1 = ds.corner_tables(pos, W, True, 'bilinear')
    assert i0.tolist() == [W - 1, W - 1, W - 1, W - 1, W - 1, W - 1, 1, 0, 0]
    assert i1.tolist() == [0, 0, 0, 0, 0, 0, 2, 1, 1]
    assert w1.tolist() == [0.0, 0.25, 0.75, 0.75, 0.0, 0.5, 0.5, 0.0, 0.0]
    got = ds.interpolate(field, ds.corner_tables(np.zeros(1), 1, False), (i0, i1, w0, w1))[0]
    assert got[1] == (0.75 * field[0, W - 1] + 0.25 * field[0, 0]) + 0.0 + 0.0
    assert got[3] == got[2] and got[4] == field[0, W - 1] and got[7] == field[0, 0]
    # the same positions without wrap hold the edges
    held = ds.corner_tables(pos, W, False, 'bilinear')
    assert held[0].tolist() == [W - 1, W - 1, W - 1, 0, 0, 0, W - 1, 0, W - 1]


def test_size_one():
    for wrap in (False, True):
        for method in ds.METHODS:
            i0, i1, w0, w1 = ds.corner_tables(np.array([-2.0, 0.0, 0.4, 0.6, 5.0]), 1, wrap, method)
            assert i0.tolist() == [0] * 5 and i1.tolist() == [0] * 5 and np.all(w0 + w1 == 1.0)
            t = (i0, i1, w0, w1)
            got = ds.interpolate(np.array([[3.5]]), t, t)
            # one cell: every pixel has its value (the weights of a wrapped axis sum to 1 within an ulp)
            assert np.allclose(got, 3.5, rtol=4e-16, atol=0)
            if not wrap:
                assert np.all(got == 3.5)


def test_bilinear_reproduces_a_linear_field():
    """Inside the grid a field a + b r + c c is reproduced to rounding: four products and three sums
    of values up to 26 -- a few ulp of 26 (3.6e-15 each); 7e-15 holds. The error is taken against the
    exact rational value at the (float64) positions, so that it is the interpolant's alone: a float64
    evaluation of a + b r + c c carries an ulp of its own."""
    from fractions import Fraction
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    field = 1.25 + 3.5 * rr + 1.75 * cc
    assert field.max() <= 26 and field.max() > 25
    row_pos = np.linspace(0.0, H - 1.0, R)
    col_pos = np.linspace(0.0, W - 1.0, C)
    got = ds.interpolate(field, ds.corner_tables(row_pos, H), ds.corner_tables(col_pos, W))
    a, b, c = Fraction(1.25), Fraction(3.5), Fraction(1.75)
    worst = max(abs(Fraction(float(got[i, j])) - (a + b * Fraction(float(row_pos[i])) + c * Fraction(float(col_pos[j]))))
                for i in range(R) for j in range(C))
    print('bilinear on a linear field: worst error %.3e' % float(worst))
    assert float(worst) <= 7e-15


def test_weights_sum_to_one_everywhere():
    pos = np.random.default_rng(8).uniform(-20.0, 20.0, 5000)
    for method in ds.METHODS:
        for wrap in (False, True):
            i0, i1, w0, w1 = ds.corner_tables(pos, W, wrap, method)
            assert np.all(w0 + w1 == 1.0) and np.all((w1 >= 0.0) & (w1 <= 1.0))
    # cos4 is symmetric about the middle and steeper than bilinear
    _, _, _, w = ds.corner_tables(np.array([0.25, 0.5, 0.75]), W, False, 'cos4')
    assert w[1] == 0.5 and abs(w[0] + w[2] - 1.0) < 1e-15 and w[0] < 0.25


def test_corner_tables_errors():
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='not finite'):
            ds.corner_tables(np.array([0.0, bad]), W)
    for size in (0, -3):
        with pytest.raises(ValueError, match='size'):
            ds.corner_tables(np.zeros(2), size)
    with pytest.raises(ValueError, match='method'):
        ds.corner_tables(np.zeros(2), W, method='cubic')
    with pytest.raises(ValueError, match='one-dimensional'):
        ds.corner_tables(np.zeros((2, 2)), W)
    rt = ds.corner_tables(np.zeros(R), H)
    ct = ds.corner_tables(np.zeros(C), W)
    with pytest.raises(ValueError, match='two-dimensional'):
        ds.interpolate(np.zeros(W), rt, ct)
    with pytest.raises(ValueError, match='outside'):
        ds.interpolate(np.zeros((H, W)), (rt[0] + H,) + rt[1:], ct)
    with pytest.raises(ValueError, match='shape'):
        ds.interpolate(np.zeros((H, W)), (rt[0][:-1],) + rt[1:], ct)
    with pytest.raises(ValueError, match='not finite'):
        ds.interpolate(np.zeros((H, W)), rt, ct[:3] + (np.full(C, np.nan),))


def shapes(coarse=ds.MET_DRIVERS, fine=(R, C)):
    return [(H, W) if name in coarse else fine for name in ds.DRIVER_NAMES]


def test_check_call():
    assert len(ds.MET_DRIVERS) == 11 and set(ds.DRIVER_NAMES) - set(ds.MET_DRIVERS) == {'sw_albedo', 'fpar', 'lai'}
    assert [n for n in ds.DRIVER_NAMES if n in ds.MET_DRIVERS] == list(ds.MET_DRIVERS)
    kinds, first, n = ds.check_call((R, C), (H, W), shapes(), cls_size=R * C)
    assert (first, n) == (0, R * C)
    assert kinds == [ds.KIND_COARSE] * 4 + [ds.KIND_FINE] + [ds.KIND_COARSE] * 7 + [ds.KIND_FINE] * 2
    kinds, first, n = ds.check_call((R, C), (H, W), shapes(('tmin',), ()) , coarse=['tmin'], first_pixel=100, n=257)
    assert (first, n) == (100, 257) and kinds.count(ds.KIND_SCALAR) == 13 and kinds[8] == ds.KIND_COARSE
    kinds, _, n = ds.check_call((R, C), (H, W), shapes(fine=(255,)), first_pixel=53, n=255, cls_size=255)
    assert kinds[4] == ds.KIND_FINE and n == 255
    assert ds.check_call((R, C), (H, W), shapes(fine=()), first_pixel=R * C)[1:] == (R * C, 0)
    assert ds.check_call((R, C), (H, W), shapes(()), coarse=())[0] == [ds.KIND_FINE] * 14


def test_check_call_errors():
    ok = shapes()
    with pytest.raises(ValueError, match='method'):
        ds.check_call((R, C), (H, W), ok, method='linear')
    with pytest.raises(ValueError, match='not one of'):
        ds.check_call((R, C), (H, W), ok, coarse=('temperature',))
    with pytest.raises(ValueError, match='twice'):
        ds.check_call((R, C), (H, W), ok, coarse=('tmin', 'tmin'))
    with pytest.raises(ValueError, match='string'):
        ds.check_call((R, C), (H, W), ok, coarse='tmin')
    with pytest.raises(ValueError, match='coarse driver'):        # a coarse driver on the fine grid
        ds.check_call((R, C), (H, W), [(R, C)] * 14)
    with pytest.raises(ValueError, match='coarse driver'):        # ... or a scalar
        ds.check_call((R, C), (H, W), [()] + ok[1:])
    with pytest.raises(ValueError, match='coarse driver'):        # ... or the transposed grid
        ds.check_call((R, C), (H, W), [(W, H)] + ok[1:])
    with pytest.raises(ValueError, match='fpar has shape'):       # a fine driver on the coarse grid
        ds.check_call((R, C), (H, W), ok[:12] + [(H, W)] + ok[13:])
    with pytest.raises(ValueError, match='sw_albedo has shape'):        # the whole raster for a part of it
        ds.check_call((R, C), (H, W), ok, first_pixel=53, n=100)
    with pytest.raises(ValueError, match='14 drivers'):
        ds.check_call((R, C), (H, W), ok[:13])
    for first, n in ((-1, None), (R * C + 1, None), (0, R * C + 1), (100, R * C - 99), (0, -1)):
        with pytest.raises(ValueError, match='first_pixel|pixel range'):
            ds.check_call((R, C), (H, W), shapes(fine=()), first_pixel=first, n=n)
    with pytest.raises(ValueError, match='class raster'):
        ds.check_call((R, C), (H, W), ok, cls_size=R * C - 1)
    for shape, coarse_shape in (((0, C), (H, W)), ((R, C), (H, 0)), ((R, 2 ** 30 + 1), (H, W))):
        with pytest.raises(ValueError, match='must be between 1 and'):
            ds.check_call(shape, coarse_shape, ok)
    with pytest.raises(ValueError, match='rows, columns'):
        ds.check_call((R, C, 1), (H, W), ok)
    with pytest.raises(ValueError, match='row_pos has shape'):
        ds.check_call((R, C), (H, W), ok, row_pos=np.zeros(R + 1), col_pos=np.zeros(C))
    with pytest.raises(ValueError, match='col_pos has shape'):
        ds.check_call((R, C), (H, W), ok, row_pos=np.zeros(R), col_pos=np.zeros((C, 1)))
