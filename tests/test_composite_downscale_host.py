"""Host-side tests of the composite over coarse drivers (no GPU): the argument checks of
mod16_amd.downscale (check_coarse_arrays, coarse_mask, coarse_grid_shape, check_composite_call), the
ctypes prototypes of mod16_et_composite_downscaled_*, and the numpy entry point's behaviour without a
device."""
import ctypes

import numpy as np
import pytest

from mod16_amd import composite as cp
from mod16_amd import downscale as ds

R, C, H, W, K = 6, 5, 3, 4, 19
N = R * C
EVERY = {'sw_albedo': 8, 'fpar': 8, 'lai': 8}


def shapes(coarse=ds.MET_DRIVERS, **over):
    """The 15 shapes of a well-formed call: coarse arrays (K, H, W), temp_annual (H, W) or (N,), the
    8-day arrays (3, N), sw_rad_night a scalar unless coarse, everything else (K, N)."""
    out = []
    for name in cp.ARRAY_NAMES:
        S = -(-K // EVERY.get(name, 1))
        if name in over:
            out.append(over[name])
        elif name == 'temp_annual':
            out.append((H, W) if name in coarse else (N,))
        elif name in coarse:
            out.append((S, H, W))
        elif name == 'sw_rad_night':
            out.append(())
        else:
            out.append((S, N))
    return out


def test_check_coarse_arrays_orders_and_refuses():
    assert ds.check_coarse_arrays(ds.MET_DRIVERS) == ds.MET_DRIVERS
    assert ds.check_coarse_arrays(['day_hours', 'lai', 'temp_day']) == ('temp_day', 'lai', 'day_hours')
    assert ds.check_coarse_arrays(()) == ()
    assert ds.check_coarse_arrays(cp.ARRAY_NAMES) == cp.ARRAY_NAMES
    with pytest.raises(ValueError, match='not a string'):
        ds.check_coarse_arrays('day_hours')
    with pytest.raises(ValueError, match="names 'ndvi', which is not one of"):
        ds.check_coarse_arrays(['ndvi'])
    with pytest.raises(ValueError, match='twice'):
        ds.check_coarse_arrays(['lai', 'lai'])
    # the forward run's check does not know the hours
    with pytest.raises(ValueError, match='not one of'):
        ds.check_coarse(['day_hours'])


def test_coarse_mask_has_bit_14_for_the_hours():
    assert ds.coarse_mask(()) == 0
    assert ds.coarse_mask(('day_hours',)) == 1 << 14
    assert ds.coarse_mask(ds.MET_DRIVERS) == 0b000111111101111
    assert ds.coarse_mask(cp.ARRAY_NAMES) == (1 << 15) - 1


def test_coarse_grid_shape_wants_one_grid():
    assert ds.coarse_grid_shape(ds.MET_DRIVERS, shapes()) == (H, W)
    assert ds.coarse_grid_shape((), shapes(())) == (1, 1)
    assert ds.coarse_grid_shape(('day_hours',), shapes(('day_hours',))) == (H, W)
    with pytest.raises(ValueError, match=r'share one grid: lw_net_day is \(3, 4\), temp_day is \(3, 5\)'):
        ds.coarse_grid_shape(ds.MET_DRIVERS, shapes(temp_day=(K, H, W + 1)))
    with pytest.raises(ValueError, match=r'tmin is a coarse array: expected shape \(H, W\) or \(S, H, W\)'):
        ds.coarse_grid_shape(ds.MET_DRIVERS, shapes(tmin=(N,)))
    with pytest.raises(ValueError, match='pressure is a coarse array'):
        ds.coarse_grid_shape(ds.MET_DRIVERS, shapes(pressure=()))


def test_every_shape_kind_is_accepted():
    kinds, slabs, first, n = ds.check_composite_call((R, C), (H, W), shapes(), K, EVERY)
    assert (first, n) == (0, N)
    want = {'sw_albedo': ds.KIND_FINE_TIME, 'fpar': ds.KIND_FINE_TIME, 'lai': ds.KIND_FINE_TIME,
            'day_hours': ds.KIND_FINE_TIME, 'temp_annual': ds.KIND_COARSE}
    assert kinds == [want.get(name, ds.KIND_COARSE_TIME) for name in cp.ARRAY_NAMES]
    assert slabs == [3 if name in EVERY else 1 if name == 'temp_annual' else K for name in cp.ARRAY_NAMES]
    # nothing coarse: a scalar, a constant, slabs; the whole raster as (R, C) and (S, R, C)
    kinds, slabs, _, _ = ds.check_composite_call((R, C), (1, 1), shapes((), lai=(3, R, C), tmin=(R, C)), K, EVERY, coarse=())
    assert kinds[3] == ds.KIND_SCALAR and kinds[7] == ds.KIND_FINE and kinds[8] == ds.KIND_FINE
    assert kinds[13] == ds.KIND_FINE_TIME and kinds[0] == ds.KIND_FINE_TIME and slabs[13] == 3 and slabs[8] == 1
    # the hours coarse and 8-day, a coarse 8-day driver, a range of the raster
    ev = dict(EVERY, day_hours=8)
    sh = shapes(('fpar', 'day_hours'), day_hours=(3, H, W))
    sh = [(s[0], 11) if len(s) == 2 and name not in ('fpar', 'day_hours') else (11,) if s == (N,) else s
          for name, s in zip(cp.ARRAY_NAMES, sh)]
    kinds, slabs, first, n = ds.check_composite_call((R, C), (H, W), sh, K, ev, coarse=('day_hours', 'fpar'), first_pixel=7,
                                                     n=11, cls_size=11)
    assert (first, n) == (7, 11) and kinds[14] == ds.KIND_COARSE_TIME and kinds[12] == ds.KIND_COARSE_TIME
    assert slabs[14] == 3 and kinds[0] == ds.KIND_FINE_TIME and kinds[7] == ds.KIND_FINE
    # to the end of the raster
    assert ds.check_composite_call((R, C), (H, W), sh, K, ev, coarse=('day_hours', 'fpar'), first_pixel=N - 11)[2:] == (N - 11, 11)


def test_every_refusal_has_its_message():
    def bad(match, array_shapes=None, days=K, every=EVERY, shape=(R, C), coarse_shape=(H, W), **kw):
        with pytest.raises(ValueError, match=match):
            ds.check_composite_call(shape, coarse_shape, shapes() if array_shapes is None else array_shapes, days, every, **kw)
    bad(r'temp_day is a coarse array: expected shape \(3, 4\) or \(S, 3, 4\), got \(19, 30\)', shapes(temp_day=(K, N)))
    bad('tmin is a coarse array', shapes(tmin=()))
    bad('vpd_day is a coarse array', shapes(vpd_day=(K, W, H)))
    bad(r'fpar has shape \(3, 31\): expected a scalar, the 30 pixels of the range or the raster \(6, 5\)', shapes(fpar=(3, N + 1)))
    bad('lai has shape', shapes(lai=(3, C, R)))
    bad('day_hours has shape', shapes(day_hours=(2, K, N)))
    # slab counts against every
    bad(r'temp_day has 18 time slabs, expected ceil\(days / every\) = ceil\(19 / 1\) = 19', shapes(temp_day=(K - 1, H, W)))
    bad(r'sw_albedo has 3 time slabs, expected .* = 19', every=None)
    bad(r'lw_net_day has 19 time slabs, expected .* = 20', days=20)
    bad(r'pressure has 19 time slabs, expected .* = 10', every=dict(EVERY, pressure=2))
    bad(r'day_hours has 2 time slabs', shapes(('day_hours',), day_hours=(2, H, W)), coarse=('day_hours',), every=dict(EVERY, day_hours=8))
    bad('days must be between', days=0)
    bad('days must be between', days=4097)
    bad('not one of', every={'ndvi': 8})
    bad("names 'ndvi'", coarse=('ndvi',))
    bad('expected 15 arrays', shapes()[:14])
    bad(r'shape and coarse_shape must be \(rows, columns\)', shape=(R, C, 1))
    bad('coarse rows must be between', coarse_shape=(0, W))
    bad('columns must be between', shape=(R, 2 ** 30 + 1))
    bad('first_pixel must be between', first_pixel=-1)
    bad('leaves the raster', first_pixel=N - 3, n=4)
    bad('the class raster has 29 elements, expected 30', cls_size=N - 1)
    # a whole-raster shape is no shape of a range
    bad('lai has shape', [(s[0], 11) if len(s) == 2 and s != (H, W) else s for s in shapes(lai=(3, R, C))], first_pixel=0, n=11)


def test_prototypes_and_abi_version():
    from mod16_amd import _lib
    assert _lib.ABI_VERSION == 16
    for name in ('mod16_et_composite_downscaled_f64', 'mod16_et_composite_downscaled_f32'):
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == 15
        assert args[2] is ctypes.POINTER(_lib.CompositeDownscaledSpec) and args[10] is ctypes.c_int64 and args[14] is ctypes.c_int64
    spec = _lib.CompositeDownscaledSpec
    assert [f[0] for f in spec._fields_] == ['composite', 'coarse_mask', 'reserved_', 'coarse_pitch', 'first_pixel']
    assert spec.composite.offset == 0 and spec.coarse_mask.offset == ctypes.sizeof(_lib.CompositeSpec)
    assert ctypes.sizeof(spec) == ctypes.sizeof(_lib.CompositeSpec) + 24
    assert callable(_lib.Downscale.composite)
    lib = _lib.load()
    assert lib.mod16_version() == 16
    for name in ('mod16_et_composite_downscaled_f64', 'mod16_et_composite_downscaled_f32'):
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    # a NULL context is refused before anything is looked at
    assert lib.mod16_et_composite_downscaled_f64(None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None, 0) == _lib.ERR_ARG


def entry_arrays():
    coarse = np.ones((K, H, W))
    slow = np.ones((3, R, C))
    return [coarse] * 4 + [slow] + [coarse] * 2 + [np.ones((H, W))] + [coarse] * 4 + [slow, slow], np.ones((K, R, C))


def test_numpy_entry_point_checks_then_needs_a_device():
    """Every bad argument is a ValueError with no device present; a good call then meets the library's
    "no CPU fallback" error (or, on a GPU box, runs)."""
    import mod16
    import mod16_amd
    from mod16_amd import _lib
    assert mod16.evapotranspiration_composite_downscaled is mod16_amd.evapotranspiration_composite_downscaled
    call = mod16_amd.evapotranspiration_composite_downscaled
    table, cls = np.ones((13, 11)), np.ones((R, C), np.uint8)
    base, hours = entry_arrays()
    row_pos, col_pos = np.arange(R) * 0.4, np.arange(C) * 0.7

    def bad(match, drivers=base, hours=hours, cls=cls, rows=row_pos, cols=col_pos, **kw):
        kw.setdefault('every', EVERY)
        with pytest.raises(ValueError, match=match):
            call(table, cls, *drivers, hours, rows, cols, **kw)
    bad('time slabs', every=None)
    bad('time slabs', days=20)
    bad('days must be between', days=0)
    bad('period_days', period_days=0)
    bad('min_valid', min_valid=9)
    bad('not one of', every={'ndvi': 8})
    bad("coarse names 'ndvi'", coarse=('ndvi',))
    bad('method must be one of', method='cubic')
    bad('share one grid', drivers=base[:5] + [np.ones((K, H + 1, W))] + base[6:])
    bad('lw_net_day is a coarse array', drivers=[np.ones(N)] + base[1:])
    bad('lw_net_night is a coarse array', drivers=[base[0], np.ones((2, K, H, W))] + base[2:])
    bad('fpar has shape', drivers=base[:12] + [np.ones((3, R, C + 1))] + base[13:])
    bad('share one grid: lw_net_day is .*, day_hours is', coarse=ds.MET_DRIVERS + ('day_hours',))
    bad('day_hours is a coarse array', hours=np.ones(N), coarse=ds.MET_DRIVERS + ('day_hours',))
    bad(r'cls must be an \(R, C\) raster', cls=np.ones(N, np.uint8))
    bad(r'row_pos has shape \(5,\), expected \(6,\)', rows=row_pos[:5])
    bad('col_pos has shape', cols=np.ones((C, 1)))
    bad('MATH_FAST or MATH_EXACT', math=_lib.MATH_MIXED)
    bad('MATH_FAST or MATH_EXACT', math=_lib.DOMAIN_TRUSTED)
    bad('stage_bytes', stage_bytes=-1)
    bad('out must hold', out=[np.empty((3, R, C))])
    bad(r'out\[1\]', out=[np.empty((3, R, C)), np.empty((3, R, C))])
    bad('days is required', drivers=[1.0] * 4 + [base[4]] + [1.0] * 7 + base[12:], hours=12.0, coarse=())
    bad('not finite', rows=np.where(np.arange(R) == 2, np.nan, row_pos))
    if _lib.device_count() > 0:          # a GPU is present: the good call runs (tests/test_gpu_composite_downscale.py)
        got = call(table, cls, *base, hours, row_pos, col_pos, every=EVERY)
        assert got.et.shape == (3, R, C) and got.count.dtype == np.uint16
        return
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        call(table, cls, *base, hours, row_pos, col_pos, every=EVERY)
    # 'day_hours' among the coarse arrays passes the checks too
    with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
        call(table, cls, *base, np.ones((K, H, W)), row_pos, col_pos, every=EVERY, coarse=ds.MET_DRIVERS + ('day_hours',), pet=True)
