"""The definition of the temporal gap filling (mod16_amd/gapfill.py: reliable, fill_series, encode,
check_series) against a scalar Python loop that follows the five cases of the table literally, pixel
by pixel and slab by slab. No GPU, no library: numpy only.

Shapes: (S, n) = (23, 600) drawn with the recipe of tests/test_gpu_gapfill.py (codes uniform in
0..100 with 5 % fill codes, QC bytes from a list of twelve whose four acceptable ones are drawn with
probability 0.15 each and the others with 0.05 each -- 0.6 x 0.95 = 57 % of the slabs reliable -- and
the five planted pixels), so the loop covers all five sources and the half-way roundings; S = 1 and S = 2 on
their own. Equality throughout: the definition is exact."""
import numpy as np
import pytest

from mod16_amd import gapfill as gf

QC_CODES = (0, 2, 8, 16, 24, 32, 64, 96, 128, 1, 4, 157)
QC_WEIGHTS = tuple(0.15 if q in (0, 2, 24, 32) else 0.05 for q in QC_CODES)      # the four acceptable codes: 0.6


def recipe(S, n, seed=7):
    """(values, qc, fallback) of the module docstring; the planted pixels are the first five."""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 101, (S, n)).astype(np.uint8)
    fill = rng.uniform(0, 1, (S, n)) < 0.05
    values[fill] = rng.integers(249, 256, int(fill.sum())).astype(np.uint8)
    qc = rng.choice(np.array(QC_CODES, np.uint8), (S, n), p=QC_WEIGHTS)
    fallback = rng.integers(0, 101, n).astype(np.uint8)
    fallback[rng.uniform(0, 1, n) < 0.1] = 255
    if n >= 5:
        clean = np.minimum(values[:, :5], 100)
        values[:, :5] = clean
        qc[:, 0] = 1                       # never reliable
        qc[:, 1] = 1; qc[S - 1, 1] = 0     # reliable only in the last slab
        qc[:, 2] = 1; qc[0, 2] = 0         # ... only in the first
        qc[:, 3] = 0                       # ... everywhere
        qc[:, 4] = 1; qc[0, 4] = 0; qc[S - 1, 4] = 0     # one gap over slabs 1 .. S - 2, between 0 and 100
        values[0, 4] = 0; values[S - 1, 4] = 100
    return values, qc, fallback


def scalar_fill(values, rel, max_gap, fallback):
    """The table of mod16_amd/gapfill.py, literally: -> (num, den, source) as Python-int arrays."""
    S, n = values.shape
    num = np.zeros((S, n), np.int64)
    den = np.ones((S, n), np.int64)
    src = np.zeros((S, n), np.uint8)
    for p in range(n):
        for t in range(S):
            i = next((s for s in range(t, -1, -1) if rel[s, p]), None)
            j = next((s for s in range(t, S) if rel[s, p]), None)
            if rel[t, p]:
                num[t, p], src[t, p] = int(values[t, p]), 0
            elif i is not None and j is not None and (max_gap is None or j - i - 1 <= max_gap):
                num[t, p] = int(values[i, p]) * (j - t) + int(values[j, p]) * (t - i)
                den[t, p], src[t, p] = j - i, 1
            elif i is not None and j is None and (max_gap is None or t - i <= max_gap):
                num[t, p], src[t, p] = int(values[i, p]), 2
            elif j is not None and i is None and (max_gap is None or j - t <= max_gap):
                num[t, p], src[t, p] = int(values[j, p]), 2
            elif fallback is not None and fallback[p] < 249:
                num[t, p], src[t, p] = int(fallback[p]), 3
            else:
                src[t, p] = 4
    return num, den, src


def scalar_encode(num, den, src, dtype, scale):
    out = np.empty(num.shape, dtype)
    for idx in np.ndindex(num.shape):
        if src[idx] == 4:
            out[idx] = 255 if np.dtype(dtype) == np.uint8 else np.nan
        elif np.dtype(dtype) == np.uint8:
            out[idx] = (2 * int(num[idx]) + int(den[idx])) // (2 * int(den[idx]))
        else:
            out[idx] = np.dtype(dtype).type((np.float64(int(num[idx])) / np.float64(int(den[idx]))) * np.float64(scale))
    return out


def same_bits(a, b):
    if a.dtype.kind == 'f':
        nan = np.isnan(a)
        view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and \
            np.array_equal(a.view(view)[~nan], b.view(view)[~nan])
    return a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize('with_fallback', [False, True])
@pytest.mark.parametrize('max_gap', [None, 2, 0])
def test_fill_series_and_encode_equal_the_scalar_loop(max_gap, with_fallback):
    values, qc, fallback = recipe(23, 600)
    fb = fallback if with_fallback else None
    rel = gf.reliable(values, qc)
    assert 0.5 < rel.mean() < 0.65
    num, den, src = gf.fill_series(values, rel, max_gap, fb)
    wnum, wden, wsrc = scalar_fill(values, rel, max_gap, fb)
    assert np.array_equal(src, wsrc)
    filled = wsrc < 4
    assert np.array_equal(num[filled], wnum[filled]) and np.array_equal(den[filled], wden[filled])
    if max_gap == 2:
        assert set(np.unique(wsrc)) == ({0, 1, 2, 3, 4} if with_fallback else {0, 1, 2, 4})
    for dtype, scale in (('uint8', 1.0), ('float32', 0.01), ('float64', 0.1)):
        got = gf.encode(num, den, src, dtype, scale)
        assert same_bits(got, scalar_encode(wnum, wden, wsrc, dtype, scale)), dtype
    if max_gap is None:     # exact half-way roundings are part of the recipe
        twice = 2 * wnum
        assert ((wsrc == 1) & (twice % wden == 0) & ((twice // wden) % 2 == 1)).sum() > 10


def test_planted_pixels():
    S = 23
    values, qc, fallback = recipe(S, 600)
    rel = gf.reliable(values, qc)
    assert not rel[:, 0].any() and rel[:, 1].sum() == 1 and rel[:, 2].sum() == 1 and rel[:, 3].all()
    num, den, src = gf.fill_series(values, rel)
    assert (src[:, 0] == 4).all()
    assert (src[:-1, 1] == 2).all() and (num[:, 1] == values[-1, 1]).all()
    assert (src[1:, 2] == 2).all() and (num[:, 2] == values[0, 2]).all()
    assert (src[:, 3] == 0).all()
    assert (src[1:-1, 4] == 1).all() and (den[1:-1, 4] == S - 1).all()
    assert np.array_equal(num[1:-1, 4], 100 * np.arange(1, S - 1))
    # with a fallback the never-reliable pixel takes it; a limit turns the long holds into fallback / unfilled
    num, den, src = gf.fill_series(values, rel, 2, np.full(600, 7, np.uint8))
    assert (src[:, 0] == 3).all() and (num[:, 0] == 7).all()
    assert (src[-3:-1, 1] == 2).all() and (src[:-3, 1] == 3).all()
    assert (src[1:3, 2] == 2).all() and (src[3:, 2] == 3).all()
    assert (src[1:-1, 4] == 3).all()


def test_default_table_is_the_eight_codes():
    assert gf.MOD15_GOOD == (0, 2, 24, 26, 32, 34, 56, 58)
    good = gf.default_good()
    assert good.shape == (256,) and good.dtype == bool and good.sum() == 8
    assert sorted(np.flatnonzero(good)) == list(gf.MOD15_GOOD)
    # a caller's table replaces it; without a QC layer only the fill codes count
    v = np.array([[5], [250], [7]], np.uint8)
    q = np.array([[8], [0], [0]], np.uint8)
    assert gf.reliable(v, q).ravel().tolist() == [False, False, True]
    assert gf.reliable(v, q, np.ones(256, bool)).ravel().tolist() == [True, False, True]
    assert gf.reliable(v).ravel().tolist() == [True, False, True]
    assert gf.reliable(np.array([248, 249], np.uint8)).tolist() == [True, False]


def test_half_way_rounds_up():
    v = np.array([[0], [255], [1]], np.uint8)
    num, den, src = gf.fill_series(v, v < 249)
    assert (int(num[1, 0]), int(den[1, 0]), int(src[1, 0])) == (1, 2, 1)
    assert gf.encode(num, den, src, 'uint8')[1, 0] == 1
    assert gf.encode(num, den, src, 'float64')[1, 0] == 0.5
    assert gf.encode(num, den, src, 'float32', 0.1)[1, 0] == np.float32(0.5 * 0.1)
    v = np.array([[3], [255], [255], [255], [4]], np.uint8)       # 3.25, 3.5, 3.75 -> 3, 4, 4
    num, den, src = gf.fill_series(v, v < 249)
    assert gf.encode(num, den, src, 'uint8').ravel().tolist() == [3, 3, 4, 4, 4]


@pytest.mark.parametrize('S', [1, 2])
def test_short_series(S):
    values, qc, fallback = recipe(S, 64, seed=3)
    for max_gap in (None, 0):
        for fb in (None, fallback):
            rel = gf.reliable(values, qc)
            num, den, src = gf.fill_series(values, rel, max_gap, fb)
            wnum, wden, wsrc = scalar_fill(values, rel, max_gap, fb)
            assert np.array_equal(src, wsrc)
            assert np.array_equal(gf.encode(num, den, src, 'uint8'), scalar_encode(wnum, wden, wsrc, 'uint8', 1.0))
            assert not (src == 1).any()           # nothing to interpolate between in one or two slabs


def test_check_series_refuses():
    ok = (23, 600)
    S, shape, table, mg, name, scales = gf.check_series([ok, ok], ok, None, None, [(600,), None], 'float64', (0.01, 0.1))
    assert (S, shape, mg, name, scales) == (23, (600,), -1, 'float64', [0.01, 0.1]) and table.sum() == 8
    assert gf.check_series([ok], max_gap=3)[3] == 3
    assert gf.check_series([(4096, 2, 3)])[:2] == (4096, (2, 3))
    bad = [
        dict(shapes=[(0, 600)]),                                # S out of range
        dict(shapes=[(4097, 600)]),
        dict(shapes=[()]),
        dict(shapes=[]),
        dict(shapes=[ok] * 4),                                  # more than three fields
        dict(shapes=[ok, (23, 601)]),                           # shape mismatches
        dict(shapes=[ok], qc_shape=(22, 600)),
        dict(shapes=[ok], fallback_shapes=[(601,)]),
        dict(shapes=[ok, ok], fallback_shapes=[(600,)]),
        dict(shapes=[ok], good=np.ones(255, bool)),             # a table that is not 256 long
        dict(shapes=[ok], good=np.ones((2, 128), bool)),
        dict(shapes=[ok], max_gap=-1),                          # negative max_gap
        dict(shapes=[ok], max_gap=1.5),
        dict(shapes=[ok], max_gap=True),
        dict(shapes=[ok], dtype='int16'),                       # a bad dtype
        dict(shapes=[ok], dtype='float16'),
        dict(shapes=[ok], dtype='nonsense'),
        dict(shapes=[ok], dtype='uint8', scale=0.01),           # scale with uint8 output
        dict(shapes=[ok, ok], dtype='float32', scale=(0.01,)),
        dict(shapes=[ok], dtype='float32', scale=float('nan')),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            gf.check_series(**kw)
    with pytest.raises(ValueError):
        gf.fill_series(np.zeros((3, 4), np.uint8), np.zeros((3, 5), bool))
    with pytest.raises(ValueError):
        gf.encode(np.zeros(3, np.int64), np.ones(3, np.int64), np.zeros(3, np.uint8), 'int32')


def test_the_package_entry_point_checks_before_any_device_work():
    """gapfill_series validates with check_series first: the errors arrive without a GPU."""
    import mod16_amd
    v = np.zeros((3, 8), np.uint8)
    with pytest.raises(ValueError):
        mod16_amd.gapfill_series(v, max_gap=-2)
    with pytest.raises(ValueError):
        mod16_amd.gapfill_series((v, v, v, v))
    with pytest.raises(ValueError):
        mod16_amd.gapfill_series(v, qc=np.zeros((3, 9), np.uint8))
    with pytest.raises(ValueError):
        mod16_amd.gapfill_series(v, scale=0.01)
    with pytest.raises(ValueError):
        mod16_amd.gapfill_series(v.astype(np.int16))
    with pytest.raises(ValueError):
        mod16_amd.gapfill_series(np.zeros((4097, 2), np.uint8))
    import mod16
    assert mod16.gapfill_series is mod16_amd.gapfill_series
    # nothing to do is done without a device as well
    out, src = mod16_amd.gapfill_series(np.zeros((3, 0), np.uint8), source=True)
    assert out.shape == (3, 0) and out.dtype == np.uint8 and src.shape == (3, 0)
