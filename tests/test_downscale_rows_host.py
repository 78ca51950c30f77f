"""Host-only tests of the row-affine column geometry of the downscaled families (sinusoidal tiles):
the numpy definition in mod16_amd.downscale (column_positions, corner_tables_rows, interpolate_rows,
sinusoidal_positions, check_affine), the two new ctypes prototypes (mod16_downscale_create_rows,
mod16_downscale_create_rows_tables; the ABI stays 16) and the numpy entry points' argument checks
without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mod16_amd import downscale as ds

R, C, H, W = 37, 53, 5, 7
METHODS = ('nearest', 'bilinear')


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def geometry(base):
    """The two column geometries of tests/test_gpu_downscale_rows.py: scale = base / cos(lat) over
    lat = 70 ... -70 degrees, row 5 with scale 0, row 6 east to west, row 7 on exact centres and halves."""
    lat = np.radians(np.linspace(70.0, -70.0, R))
    scale = base / np.cos(lat)
    scale[5] = 0.0
    scale[6] = -scale[6]
    origin = 3.0 - scale * 26
    scale[7], origin[7] = 0.5, -2.0
    return origin, scale


def test_column_positions_is_one_multiplication_and_one_addition():
    origin, scale = geometry(0.41)
    pos = ds.column_positions(origin, scale, C)
    assert pos.shape == (R, C) and pos.dtype == np.float64
    for r in (0, 5, 6, 7, 36):
        for c in (0, 1, 26, 52):
            assert pos[r, c] == origin[r] + np.float64(scale[r] * np.float64(c))


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_corner_tables_rows_is_corner_tables_row_by_row(method, wrap):
    origin, scale = geometry(0.41 if wrap else 0.09)
    pos = ds.column_positions(origin, scale, C)
    got = ds.corner_tables_rows(origin, scale, C, W, wrap, method)
    assert [t.shape for t in got] == [(R, C)] * 4
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    for r in range(R):
        want = ds.corner_tables(pos[r], W, wrap, method)
        for g, w in zip(got, want):
            assert same_bits(g[r], w), (r, method, wrap)
    assert got[0].min() >= 0 and got[1].max() < W


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_interpolate_rows_is_interpolate_row_by_row(method, wrap):
    origin, scale = geometry(0.41 if wrap else 0.09)
    rng = np.random.default_rng(5)
    field = rng.normal(size=(H, W))
    field[2, 3] = np.nan
    field[0, 6] = np.inf
    row_pos = ds.positions(-0.8, 0.17, R, 0.0, 1.0)
    rt = ds.corner_tables(row_pos, H, False, method)
    ct = ds.corner_tables_rows(origin, scale, C, W, wrap, method)
    got = ds.interpolate_rows(field, rt, ct)
    assert got.shape == (R, C) and got.dtype == np.float64
    for r in range(R):
        one = ds.interpolate(field, tuple(t[r:r + 1] for t in rt), tuple(t[r] for t in ct))
        assert same_bits(got[r:r + 1], one), r
    assert np.isnan(got).any() and np.isfinite(got).any()
    with pytest.raises(ValueError, match='two-dimensional'):
        ds.interpolate_rows(field[0], rt, ct)
    with pytest.raises(ValueError, match='column table has shape'):
        ds.interpolate_rows(field, rt, tuple(t[0] for t in ct))
    with pytest.raises(ValueError, match='outside'):
        ds.interpolate_rows(field[:, :W - 1], rt, ct)


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_constant_dyadic_affine_equals_the_rectilinear_path(method, wrap):
    """origin -9.25 and scale 0.375 in every row: origin + scale * c is exact, so the row-affine
    tables are the rectilinear ones in every entry and interpolate_rows has the bytes of interpolate."""
    origin, scale = np.full(R, -9.25), np.full(R, 0.375)
    col_pos = -9.25 + 0.375 * np.arange(C)
    assert np.array_equal(ds.column_positions(origin, scale, C), np.broadcast_to(col_pos, (R, C)))
    want = ds.corner_tables(col_pos, W, wrap, method)
    got = ds.corner_tables_rows(origin, scale, C, W, wrap, method)
    for g, w in zip(got, want):
        assert same_bits(g, np.ascontiguousarray(np.broadcast_to(w, (R, C))))
    field = np.random.default_rng(9).normal(size=(H, W))
    field[1, 2] = np.nan
    rt = ds.corner_tables(ds.positions(-0.8, 0.17, R, 0.0, 1.0), H, False, method)
    assert same_bits(ds.interpolate_rows(field, rt, got), ds.interpolate(field, rt, want))


# ---- sinusoidal_positions against an independent forward formula

RADIUS = 6371007.181
GRID = (90.0, -0.5, -180.0, 0.625)          # a global 0.5 x 0.625 degree grid from 90 N / 180 W: 361 x 576


def forward(h, v, size, r, c):
    """(latitude, longitude) in degrees of the centre of pixel (r, c) of tile (h, v): the inverse
    sinusoidal projection from the tile's corner, written out on its own."""
    import math
    tile = 2 * math.pi * RADIUS / 36
    x = (h - 18) * tile + (c + 0.5) * tile / size
    y = (9 - v) * tile - (r + 0.5) * tile / size
    lat = y / RADIUS
    return math.degrees(lat), math.degrees(x / (RADIUS * math.cos(lat)))


def test_sinusoidal_positions_polar_tile():
    row_pos, origin, scale = ds.sinusoidal_positions(18, 0, 1200, *GRID)
    assert row_pos.shape == origin.shape == scale.shape == (1200,)
    assert row_pos[0] == pytest.approx(1.0 / 120.0, rel=1e-9)
    assert np.all(np.isfinite(origin + scale * 1199))
    ds.check_affine((1200, 1200), origin, scale, 'bilinear')
    for r, c in ((0, 0), (0, 1199), (599, 17), (1199, 1199)):
        lat, lon = forward(18, 0, 1200, r, c)
        assert row_pos[r] == pytest.approx((lat - 90.0) / -0.5, rel=1e-12, abs=1e-12)
        assert origin[r] + scale[r] * c == pytest.approx((lon + 180.0) / 0.625, rel=1e-12)


def test_sinusoidal_positions_mid_latitude_tile():
    row_pos, origin, scale = ds.sinusoidal_positions(11, 4, 1200, *GRID)
    assert row_pos[0] == pytest.approx(80.008333, abs=1e-6) and row_pos[-1] == pytest.approx(99.991667, abs=1e-6)
    assert np.all(np.diff(row_pos) > 0)
    assert scale[0] / scale[-1] == pytest.approx(1.19158, abs=1e-5)
    for r, c in ((0, 0), (700, 311), (1199, 1199)):
        lat, lon = forward(11, 4, 1200, r, c)
        assert row_pos[r] == pytest.approx((lat - 90.0) / -0.5, rel=1e-12)
        assert origin[r] + scale[r] * c == pytest.approx((lon + 180.0) / 0.625, rel=1e-12)


def test_sinusoidal_positions_meridian_and_mirror():
    # h = 18: column 0 lies half a pixel east of the prime meridian
    _, origin, scale = ds.sinusoidal_positions(18, 5, 240, 90.0, -0.5, 0.0, 0.625)
    assert np.allclose(origin, 0.5 * scale, rtol=1e-14, atol=0) and np.all(origin > 0)
    # a tile and its mirror (35 - h, v): column c of one is column size - 1 - c of the other, across the meridian
    for h, v in ((11, 4), (0, 8), (20, 16)):
        rp, o, s = ds.sinusoidal_positions(h, v, 240, 90.0, -0.5, 0.0, 0.625)
        rm, om, sm = ds.sinusoidal_positions(35 - h, v, 240, 90.0, -0.5, 0.0, 0.625)
        assert np.array_equal(rp, rm)
        pos, mirror = ds.column_positions(o, s, 240), ds.column_positions(om, sm, 240)
        assert np.allclose(pos, -mirror[:, ::-1], rtol=1e-12, atol=1e-9)
    # other pixel counts, a coarse grid that runs south to north
    rp, o, s = ds.sinusoidal_positions(11, 4, 7, -90.0, 0.5, -180.0, 0.625)
    lat, lon = forward(11, 4, 7, 3, 5)
    assert rp[3] == pytest.approx((lat + 90.0) / 0.5, rel=1e-12)
    assert o[3] + s[3] * 5 == pytest.approx((lon + 180.0) / 0.625, rel=1e-12)


def test_sinusoidal_positions_argument_errors():
    for bad in ((-1, 4, 1200) + GRID, (36, 4, 1200) + GRID, (11, -1, 1200) + GRID, (11, 18, 1200) + GRID,
                (11, 4, 0) + GRID, (11, 4, 1200, 90.0, 0.0, -180.0, 0.625), (11, 4, 1200, 90.0, -0.5, -180.0, 0.0),
                (11, 4, 1200, 90.0, np.nan, -180.0, 0.625), (11, 4, 1200, 90.0, -0.5, -180.0, np.inf)):
        with pytest.raises(ValueError):
            ds.sinusoidal_positions(*bad)


def test_affine_argument_errors():
    origin, scale = geometry(0.09)
    with pytest.raises(ValueError, match='cos4.*cosine'):
        ds.corner_tables_rows(origin, scale, C, W, False, 'cos4')
    with pytest.raises(ValueError, match='cos4.*cosine'):
        ds.check_affine((R, C), origin, scale, 'cos4')
    with pytest.raises(ValueError, match='method must be one of'):
        ds.corner_tables_rows(origin, scale, C, W, False, 'cubic')
    nan = np.where(np.arange(R) == 3, np.nan, origin)
    inf = np.where(np.arange(R) == 4, np.inf, scale)
    far = np.where(np.arange(R) == 9, 1e307, scale)           # finite, but 52 of them overflow
    assert np.all(np.isfinite(far))
    for fn in (lambda o, s: ds.column_positions(o, s, C), lambda o, s: ds.corner_tables_rows(o, s, C, W),
               lambda o, s: ds.check_affine((R, C), o, s)):
        with pytest.raises(ValueError, match='col_origin holds a value that is not finite'):
            fn(nan, scale)
        with pytest.raises(ValueError, match='col_scale holds a value that is not finite'):
            fn(origin, inf)
        with pytest.raises(ValueError, match=r'col_origin \+ col_scale \* \(cols - 1\) is not finite'):
            fn(origin, far)
        with pytest.raises(ValueError, match='equal length'):
            fn(origin, scale[:-1])
        with pytest.raises(ValueError, match='one-dimensional'):
            fn(origin.reshape(1, R), scale.reshape(1, R))
    with pytest.raises(ValueError, match=r'expected \(37,\)'):
        ds.check_affine((R, C), origin[:-1], scale[:-1])
    o, s = ds.check_affine((R, C), list(origin), list(scale), 'nearest')
    assert o.dtype == np.float64 and s.flags.c_contiguous and np.array_equal(o, origin)


def test_prototypes_header_and_abi_version():
    from mod16_amd import _lib
    assert _lib.ABI_VERSION == 16
    res, args = _lib.PROTOTYPES['mod16_downscale_create_rows']
    assert res is ctypes.c_int and len(args) == 6 and args[1] == ctypes.POINTER(_lib.DownscaleSpec)
    res, args = _lib.PROTOTYPES['mod16_downscale_create_rows_tables']
    assert res is ctypes.c_int and len(args) == 9 and args[-1] == ctypes.POINTER(ctypes.c_void_p)
    header = open(os.path.join(ROOT, 'include', 'mod16_hip.h')).read()
    assert re.search(r'#define\s+MOD16_ABI_VERSION\s+16\b', header)
    for name in ('mod16_downscale_create_rows', 'mod16_downscale_create_rows_tables'):
        assert re.search(r'MOD16_API int %s\(mod16_ctx\* ctx, const mod16_downscale_spec\* spec,' % name, header), name
    lib = _lib.load()
    assert lib.mod16_version() == 16
    for name in ('mod16_downscale_create_rows', 'mod16_downscale_create_rows_tables'):
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    # a NULL context is refused before anything is looked at
    handle = ctypes.c_void_p()
    assert lib.mod16_downscale_create_rows(None, None, None, None, None, ctypes.byref(handle)) == _lib.ERR_ARG
    assert lib.mod16_downscale_create_rows_tables(None, None, None, None, None, None, None, None,
                                                  ctypes.byref(handle)) == _lib.ERR_ARG
    assert not handle.value


def test_downscale_handle_wants_exactly_one_column_geometry():
    """_lib.Downscale checks its arguments before it touches the context."""
    from mod16_amd import _lib
    origin, scale = geometry(0.09)
    row_pos = ds.positions(-0.8, 0.17, R, 0.0, 1.0)
    with pytest.raises(ValueError, match='exactly one of col_pos and col_affine'):
        _lib.Downscale(None, (R, C), (H, W), row_pos, np.zeros(C), col_affine=(origin, scale))
    with pytest.raises(ValueError, match='exactly one of col_pos and col_affine'):
        _lib.Downscale(None, (R, C), (H, W), row_pos)
    with pytest.raises(ValueError, match='cos4'):
        _lib.Downscale(None, (R, C), (H, W), row_pos, method='cos4', col_affine=(origin, scale))
    with pytest.raises(ValueError, match='not finite'):
        _lib.Downscale(None, (R, C), (H, W), row_pos, col_affine=(origin, np.where(np.arange(R) == 1, np.inf, scale)))


def test_numpy_entry_points_check_then_need_a_device():
    """Both numpy entry points with col_affine: every bad argument is a ValueError with no device
    present; a good call then meets the library's "no CPU fallback" error (or, on a GPU box, runs)."""
    import mod16
    import mod16_amd
    from mod16_amd import _lib
    assert mod16.evapotranspiration_downscaled is mod16_amd.evapotranspiration_downscaled
    r, c, h, w, K = 6, 5, 3, 4, 3
    table, cls = np.ones((13, 11)), np.ones((r, c), np.uint8)
    row_pos, col_pos = np.arange(r) * 0.4, np.arange(c) * 0.7
    origin, scale = np.linspace(-1.0, 1.0, r), np.linspace(0.3, 0.9, r)
    step = [np.ones((h, w)) if name in ds.MET_DRIVERS else np.ones((r, c)) for name in ds.DRIVER_NAMES]
    series = [np.ones((K, h, w)) if name in ds.MET_DRIVERS else np.ones((K, r, c)) for name in ds.DRIVER_NAMES]
    calls = ((mod16_amd.evapotranspiration_downscaled, lambda: (table, cls) + tuple(step) + (row_pos,)),
             (mod16_amd.evapotranspiration_composite_downscaled,
              lambda: (table, cls) + tuple(series) + (np.ones((K, r, c)), row_pos)))
    for call, args in calls:
        def bad(match, cols=None, **kw):
            kw.setdefault('col_affine', (origin, scale))
            with pytest.raises(ValueError, match=match):
                call(*args(), cols, **kw)
        bad('exactly one of col_pos and col_affine', cols=col_pos)
        bad('exactly one of col_pos and col_affine', col_affine=None)
        bad('cos4', method='cos4')
        bad('method must be one of', method='cubic')
        bad('col_origin holds a value that is not finite', col_affine=(np.where(np.arange(r) == 2, np.nan, origin), scale))
        bad('col_scale holds a value that is not finite', col_affine=(origin, np.where(np.arange(r) == 2, -np.inf, scale)))
        bad(r'\(cols - 1\) is not finite', col_affine=(origin, np.full(r, 1e308)))
        bad('equal length', col_affine=(origin, scale[:-1]))
        bad('one-dimensional', col_affine=(origin.reshape(2, 3), scale.reshape(2, 3)))
        bad(r'expected \(6,\)', col_affine=(np.zeros(r + 1), np.ones(r + 1)))
        bad('MATH_FAST or MATH_EXACT', math=_lib.MATH_MIXED)
        if _lib.device_count() > 0:      # a GPU is present: the good call runs (tests/test_gpu_downscale_rows.py)
            call(*args(), None, col_affine=(origin, scale))
            continue
        with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
            call(*args(), None, col_affine=(origin, scale))
