"""What the numpy entry points hand to the library, and what they refuse, without a GPU and without
the library: `_lib.context`, `_lib.load`, `_lib.Ensemble`, `_lib.Downscale` and `_lib.Upscale` are
replaced by stand-ins that record their calls (and read what the addresses point at while the call's
arrays are alive). The argument handling of `evapotranspiration_raster`, `_ensemble`,
`_ensemble_quantiles`, `_composite`, `_downscaled`, `_raw`, `gapfill_series`, `zonal_statistics`,
`aggregate_daynight`, `trend_series`, `anomaly_series`, `upscale_fields` and `upscale_classes` is
pinned here: strides and kinds, `n`, `inner`, flags and `where`, addresses relative to the arrays
they must point into, output dtype / shape / return type, `set_bplut` before the call, the dealing
of pixel ranges over `devices=`, and the exact refusals with the order in which they fire."""
import ctypes as C
import threading

import numpy as np
import pytest

import mod16_amd
from mod16_amd import _lib, multi

SHAPE, N = (2, 3), 6
BIG_TILE = 1 << 20


def _plain(a):
    if isinstance(a, C.Array):
        return list(a)
    if isinstance(a, C.c_void_p):
        return a.value
    return a


def _slot():
    '''None on the caller's thread, else the position in the device list of the worker thread.'''
    name = threading.current_thread().name
    return int(name.rsplit('slot', 1)[1]) if name.startswith('mod16-dev') else None


def _firsts(ptrs, dtype):
    '''The element each address points at (None stays None).'''
    ct = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    return [None if p is None else ct.from_address(p).value for p in ptrs]


def _bytes(ptr, n):
    return None if ptr is None else list((C.c_uint8 * n).from_address(ptr))


class Recorder(object):
    def __init__(self, tile):
        self.tile, self.events, self.lock = tile, {}, threading.Lock()

    def log(self, what, **seen):
        with self.lock:
            self.events.setdefault(_slot(), []).append((what, seen))

    def take(self):
        events, self.events = self.events, {}
        return events


class Lib(object):
    '''Stands in for the loaded library: every ``mod16_*`` entry point records its arguments.'''
    # name stem -> position of (class raster, address list, pixel count) among the arguments
    PEEK = {'mod16_et_pet': (1, 2, 6), 'mod16_et_hdiag': (1, 2, 6), 'mod16_et_raw': (1, 2, 8)}

    def __init__(self, rec):
        self.rec = rec

    def mod16_host_tile_pixels(self):
        return self.rec.tile

    def __getattr__(self, name):
        if not name.startswith('mod16_'):
            raise AttributeError(name)

        def fn(*args):
            args = [_plain(a) for a in args]
            seen = dict(args=args)
            stem, _, suffix = name.rpartition('_')
            if stem in self.PEEK:
                c, p, m = self.PEEK[stem]
                seen.update(first=_firsts(args[p], 'float32' if suffix == 'f32' else 'float64'),
                            cls=_bytes(args[c], args[m]))
            if stem == 'mod16_et_raw':
                seen.update(fpar=_bytes(args[4], args[8]), lai=_bytes(args[5], args[8]))
            self.rec.log(name, **seen)
            return _lib.OK
        return fn


class Ctx(object):
    '''Stands in for ``_lib.Context``: ``.lib``, ``.handle``, ``.check`` and the wrapper methods.'''

    def __init__(self, rec, device):
        self.rec, self.device, self.lib = rec, device, Lib(rec)
        self.handle = C.c_void_p(0x1000 + device)

    def check(self, rc):
        assert rc == _lib.OK

    def set_bplut(self, table):
        self.rec.log('set_bplut', table=np.array(table))

    def et(self, dtype, cls, drivers, dstride, params, pstride, n, out_day, out_night, out_sep,
           flags=_lib.MATH_FAST, where=_lib.HOST, stream=None):
        self.rec.log('et', dtype=np.dtype(dtype), cls=cls, cls_bytes=_bytes(cls, n), drivers=list(drivers),
                     dstride=list(dstride), first=_firsts(drivers, dtype),
                     params=None if params is None else list(params),
                     pstride=None if pstride is None else list(pstride),
                     pfirst=None if params is None else _firsts(params, dtype), n=n,
                     out=(out_day, out_night, None if out_sep is None else list(out_sep)),
                     flags=flags, where=where, stream=stream)

    def et2(self, dtype, cls, cls_kind, drivers, dkind, params, pkind, inner, n, out_day, out_night, out_sep,
            flags=_lib.MATH_FAST, where=_lib.HOST, stream=None):
        self.rec.log('et2', dtype=np.dtype(dtype), cls=cls, cls_kind=cls_kind, drivers=list(drivers),
                     dkind=list(dkind), first=_firsts(drivers, dtype),
                     params=None if params is None else list(params),
                     pkind=None if pkind is None else list(pkind),
                     pfirst=None if params is None else _firsts(params, dtype), inner=inner, n=n,
                     out=(out_day, out_night, None if out_sep is None else list(out_sep)),
                     flags=flags, where=where, stream=stream)

    def composite(self, dtype, n, days, period_days, cls, arrays, pixel_stride, time_stride, every,
                  out_et, out_pet, count_et, count_pet, out_pitch, min_valid=1, rescale=False,
                  flags=_lib.MATH_FAST, where=_lib.HOST, stream=None, stage_bytes=None):
        self.rec.log('composite', dtype=np.dtype(dtype), n=n, days=days, period_days=period_days, cls=cls,
                     cls_bytes=_bytes(cls, n), arrays=list(arrays), first=_firsts(arrays, dtype),
                     pixel_stride=list(pixel_stride), time_stride=list(time_stride), every=list(every),
                     out=(out_et, out_pet, count_et, count_pet), out_pitch=out_pitch, min_valid=min_valid,
                     rescale=rescale, flags=flags, where=where, stream=stream, stage_bytes=stage_bytes)

    def gapfill(self, out_type, n, slabs, fields, qc, good, fallback, out, source, in_pitch, qc_pitch,
                out_pitch, source_pitch, max_gap=-1, scale=(1.0, 1.0, 1.0), where=_lib.HOST, stream=None,
                stage_bytes=None):
        self.rec.log('gapfill', out_type=out_type, n=n, slabs=slabs, fields=list(fields), qc=qc,
                     good=_bytes(good, 256), fallback=None if fallback is None else list(fallback),
                     out=list(out), source=source, pitches=(in_pitch, qc_pitch, out_pitch, source_pitch),
                     max_gap=max_gap, scale=list(scale), where=where, stream=stream, stage_bytes=stage_bytes)

    def zonal(self, dtype, n, layers, nzones, zone_type, values, zones, weights, acc, bounds, weight_kind=0,
              cols=1, first_pixel=0, value_pitch=None, where=_lib.HOST, stream=None, stage_bytes=None):
        self.rec.log('zonal', dtype=np.dtype(dtype), n=n, layers=layers, nzones=nzones, zone_type=zone_type,
                     values=values, zones=zones, weights=weights, acc=acc, bounds=tuple(bounds),
                     weight_kind=weight_kind, cols=cols, first_pixel=first_pixel, value_pitch=value_pitch,
                     where=where, stream=stream, stage_bytes=stage_bytes)

    def zonal_bounds(self, dtype, n, layers, values, weights, weight_kind=0, cols=1, first_pixel=0,
                     value_pitch=None, where=_lib.HOST, stream=None, stage_bytes=None):
        self.rec.log('zonal_bounds', dtype=np.dtype(dtype), n=n, layers=layers, values=values, weights=weights,
                     weight_kind=weight_kind, cols=cols, where=where, stage_bytes=stage_bytes)
        return 2.0, 3.0

    def daynight(self, dtype, out_type, rows, cols, days, steps_per_day, fields, tables, out, temp_annual, in_pitch,
                 in_plane, out_pitch, out_plane, mode=0, threshold=0.0, where=_lib.HOST, stream=None, stage_bytes=None):
        self.rec.log('daynight', dtype=np.dtype(dtype), out_type=out_type, grid=(rows, cols, days, steps_per_day),
                     fields=list(fields), tables=tables, out=list(out), temp_annual=temp_annual,
                     pitches=(in_pitch, in_plane, out_pitch, out_plane), mode=mode, threshold=threshold, where=where,
                     stream=stream, stage_bytes=stage_bytes)

    def trend(self, dtype, n, steps, values, times, out, s, count, time_stride=None, min_valid=4, zq=0.0,
              where=_lib.HOST, stream=None, stage_bytes=None):
        self.rec.log('trend', dtype=np.dtype(dtype), n=n, steps=steps, values=values, times=[float(v) for v in times],
                     out=list(out), s=s, count=count, time_stride=time_stride, min_valid=min_valid, zq=zq, where=where,
                     stream=stream, stage_bytes=stage_bytes)

    def anomaly(self, dtype, n, years, periods, num, den, z, pct, mean, std, count, window=1, base_first=0,
                base_end=None, min_valid=3, in_stride=None, out_stride=None, clim_stride=None, where=_lib.HOST,
                stream=None, stage_bytes=None):
        self.rec.log('anomaly', dtype=np.dtype(dtype), n=n, years=years, periods=periods, num=num, den=den,
                     out=[z, pct, mean, std, count], window=window, baseline=(base_first, base_end),
                     min_valid=min_valid, strides=(in_stride, out_stride, clim_stride), where=where, stream=stream,
                     stage_bytes=stage_bytes)


class Upscale(object):
    def __init__(self, ctx, shape, coarse_shape, row_pos=None, col_pos=None, wrap=False, area=None, runs=None,
                 col_affine=None):
        self.ctx, self.pixels = ctx, int(shape[0]) * int(shape[1])
        ctx.rec.log('cells', device=ctx.device, shape=tuple(shape), coarse_shape=tuple(coarse_shape), row_pos=row_pos,
                    col_pos=col_pos, wrap=wrap, area=area, runs=runs, col_affine=col_affine)

    def run(self, dtype, values, layers, layer_stride, row_stride, min_fraction, outs, where=_lib.HOST, stream=None,
            stage_bytes=None):
        self.ctx.rec.log('run', dtype=np.dtype(dtype), values=values, layers=layers, strides=(layer_stride, row_stride),
                         min_fraction=min_fraction, outs=list(outs), where=where, stream=stream,
                         stage_bytes=stage_bytes)

    def classes(self, cls, row_stride, valid, out_cls, out_share, where=_lib.HOST, stream=None, stage_bytes=None):
        self.ctx.rec.log('classes', cls=cls, cls_bytes=_bytes(cls, self.pixels), row_stride=row_stride, valid=valid, out=(out_cls, out_share), where=where,
                         stream=stream, stage_bytes=stage_bytes)

    def close(self):
        self.ctx.rec.log('close')


class Ensemble(object):
    def __init__(self, ctx, tables):
        self.ctx = ctx
        ctx.rec.log('ensemble', device=ctx.device, tables=np.array(tables))

    def run(self, dtype, cls, drivers, dstride, n, outs, flags=_lib.MATH_FAST, where=_lib.HOST, stream=None):
        self.ctx.rec.log('run', dtype=np.dtype(dtype), cls=cls, cls_bytes=_bytes(cls, n), drivers=list(drivers),
                         dstride=list(dstride), first=_firsts(drivers, dtype), n=n, outs=list(outs), flags=flags,
                         where=where, stream=stream)

    def quantiles(self, dtype, cls, drivers, dstride, n, q, outs, slab_bytes=None, flags=_lib.MATH_FAST,
                  where=_lib.HOST, stream=None):
        self.ctx.rec.log('quantiles', dtype=np.dtype(dtype), cls=cls, cls_bytes=_bytes(cls, n),
                         drivers=list(drivers), dstride=list(dstride), first=_firsts(drivers, dtype), n=n,
                         q=[float(v) for v in q], outs=list(outs), slab_bytes=slab_bytes, flags=flags, where=where,
                         stream=stream)

    def close(self):
        self.ctx.rec.log('close')


class Downscale(object):
    def __init__(self, ctx, shape, coarse_shape, row_pos, col_pos, wrap=False, method='bilinear', tables=None):
        self.ctx = ctx
        ctx.rec.log('grid', device=ctx.device, shape=tuple(shape), coarse_shape=tuple(coarse_shape),
                    row_pos=row_pos, col_pos=col_pos, wrap=wrap, method=method, tables=tables)

    def run(self, dtype, cls, drivers, kinds, coarse_pitch, first_pixel, n, out_day, out_night,
            flags=_lib.MATH_FAST, where=_lib.HOST, stream=None):
        self.ctx.rec.log('run', dtype=np.dtype(dtype), cls=cls, cls_bytes=_bytes(cls, n), drivers=list(drivers),
                         first=_firsts(drivers, dtype), kinds=list(kinds), coarse_pitch=coarse_pitch,
                         first_pixel=first_pixel, n=n, out=(out_day, out_night), flags=flags, where=where,
                         stream=stream)

    def close(self):
        self.ctx.rec.log('close')


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(BIG_TILE)
    monkeypatch.setattr(_lib, 'context', lambda device=0: Ctx(r, device))
    monkeypatch.setattr(_lib, 'load', lambda: Lib(r))
    monkeypatch.setattr(_lib, 'Ensemble', Ensemble)
    monkeypatch.setattr(_lib, 'Downscale', Downscale)
    monkeypatch.setattr(_lib, 'Upscale', Upscale)
    yield r
    multi.shutdown()


@pytest.fixture
def no_library(monkeypatch):
    '''A refusal must come before anything of the library is asked for.'''
    def never(*a, **kw):
        raise AssertionError('the library was asked for')
    for name in ('context', 'load', 'Ensemble', 'Downscale', 'Upscale'):
        monkeypatch.setattr(_lib, name, never)


def make_drivers(dtype=np.float64):
    '''Fourteen drivers over SHAPE: a Python scalar, a size-1 array, twelve dense arrays; driver k
    holds 100 k + the pixel index.'''
    d = [100.0 * k + np.arange(N, dtype=dtype).reshape(SHAPE) for k in range(14)]
    d[0] = 1.5
    d[1] = np.array([2.5], dtype)
    return d


def make_table():
    '''A (13, 11) table whose beta column is missing where ``beta=`` must fill it (rows with
    parameters) and where it must not (row 0, without).'''
    t = np.arange(13 * 11, dtype=np.float64).reshape(13, 11)
    t[0] = np.nan
    t[:, 10] = np.nan
    t[5, 10] = 77.0
    return t


def filled(table, beta):
    '''What ``beta=`` makes of ``make_table()`` (plus a constant): rows 1 to 12 take it, except row
    5, which has a value of its own; row 0 has no parameters and stays without.'''
    want = table.copy()
    want[1:, 10] = beta
    want[5, 10] = table[5, 10]
    return want


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check_drivers(seen, drv, off, strides='dstride', ptrs='drivers'):
    '''The scalar and the size-1 driver are neighbours in one small array with stride 0; a dense
    driver is read where it lies, ``off`` pixels in.'''
    esz = seen['dtype'].itemsize
    assert seen[strides] == [0, 0] + [1] * 12
    assert seen['first'][:2] == [1.5, 2.5] and seen[ptrs][1] - seen[ptrs][0] == esz
    for k in range(2, 14):
        assert seen[ptrs][k] == drv[k].ctypes.data + off * esz
        assert seen['first'][k] == drv[k].flat[off]


CLS = np.array([[1, 2, 3], [4, 5, 12]])


# ------------------------------------------------------------------ evapotranspiration_raster / _forward
def test_raster_totals_on_one_device(rec):
    drv, table = make_drivers(), make_table()
    got = mod16_amd.evapotranspiration_raster(table, CLS, *drv, beta=250, math=_lib.MATH_EXACT, device=3)
    assert type(got) is tuple and len(got) == 2
    assert all(type(o) is np.ndarray and o.shape == SHAPE and o.dtype == np.float64 for o in got)
    events = rec.take()
    assert list(events) == [None]
    (bp, set_), (name, seen) = events[None]
    assert bp == 'set_bplut' and same(set_['table'], filled(table, 250)) and np.isnan(table[1, 10])
    assert name == 'et' and seen['dtype'] == np.float64 and seen['n'] == N
    assert seen['cls_bytes'] == [1, 2, 3, 4, 5, 12]          # int64 codes became bytes
    check_drivers(seen, drv, 0)
    assert seen['params'] is None and seen['pstride'] is None
    assert seen['out'] == (got[0].ctypes.data, got[1].ctypes.data, None)
    assert (seen['flags'], seen['where'], seen['stream']) == (_lib.MATH_EXACT, _lib.HOST, None)
    # a dict goes through utils.bplut_table, with the same rule for beta
    from mod16_amd.utils import bplut_table
    names = mod16_amd.MOD16.required_parameters
    as_dict = {k: table[:, j] for j, k in enumerate(names)}
    mod16_amd.evapotranspiration_raster(as_dict, CLS.astype(np.uint8), *drv, beta=250)
    (bp, set_), (name, seen) = rec.take()[None]
    assert same(set_['table'], bplut_table(as_dict, beta=250)) and same(set_['table'], filled(table, 250))
    # without beta= an array is taken as it is
    mod16_amd.evapotranspiration_raster(table, CLS.astype(np.uint8), *drv)
    assert same(rec.take()[None][0][1]['table'], table)


def test_raster_uint8_class_raster_is_read_in_place(rec):
    cls = CLS.astype(np.uint8)
    mod16_amd.evapotranspiration_raster(make_table(), cls, *make_drivers())
    assert rec.take()[None][1][1]['cls'] == cls.ctypes.data


def test_raster_components_dealt_over_two_devices_at_tile_boundaries(rec):
    rec.tile = 4                    # shards (0, 4) and (4, 2)
    drv, table = make_drivers(), make_table()
    day, night = mod16_amd.evapotranspiration_raster(table, CLS, *drv, separate=True, devices=[0, 0])
    assert type(day) is tuple and type(night) is tuple and len(day) == len(night) == 3
    outs = list(day) + list(night)
    assert all(type(o) is np.ndarray and o.shape == SHAPE and o.dtype == np.float64 for o in outs)
    events = rec.take()
    assert sorted(events) == [0, 1]
    for slot, (off, m) in enumerate([(0, 4), (4, 2)]):
        (bp, set_), (name, seen) = events[slot]
        assert bp == 'set_bplut' and same(set_['table'], table)
        assert name == 'et' and seen['n'] == m and seen['cls_bytes'] == list(CLS.flat[off:off + m])
        check_drivers(seen, drv, off)
        assert seen['out'] == (None, None, [o.ctypes.data + off * 8 for o in outs])
        assert (seen['flags'], seen['where']) == (_lib.MATH_FAST, _lib.HOST)


def test_raster_pet_float32_with_an_empty_second_shard(rec):
    drv = make_drivers(np.float32)
    got = mod16_amd.evapotranspiration_raster(make_table(), CLS, *drv, pet=True, devices=[0, 0])
    assert type(got) is tuple and len(got) == 4
    assert all(o.shape == SHAPE and o.dtype == np.float32 for o in got)
    events = rec.take()
    # the device without pixels is still given the table, and nothing else
    assert [e[0] for e in events[1]] == ['set_bplut']
    (bp, _), (name, seen) = events[0]
    assert bp == 'set_bplut' and name == 'mod16_et_pet_f32'
    a = seen['args']
    assert a[0] == 0x1000 and seen['cls'] == [1, 2, 3, 4, 5, 12]
    check_drivers(dict(dtype=np.dtype(np.float32), drivers=a[2], dstride=a[3], first=seen['first']), drv, 0)
    assert a[4] is None and a[5] is None and a[6] == N
    assert a[7:11] == [o.ctypes.data for o in got]
    assert a[11:] == [_lib.MATH_FAST, _lib.HOST, None]


def test_raster_diagnostics_folds_one_vector_per_tile(rec):
    rec.tile = 4
    drv = make_drivers()
    got = mod16_amd.evapotranspiration_raster(make_table(), CLS, *drv, diagnostics=True, devices=[0, 0])
    assert len(got) == 3 and got[2].shape == (8,) and got[2].dtype == np.float64
    events = rec.take()
    fold = [e for e in events.pop(None) if e[0] == 'mod16_fold_diag_host']
    assert len(fold) == 1 and fold[0][1]['args'][1] == 2                 # two tiles of four pixels
    tiles = fold[0][1]['args'][0]
    for slot, (off, m) in enumerate([(0, 4), (4, 2)]):
        (bp, _), (name, seen) = events[slot]
        a = seen['args']
        assert bp == 'set_bplut' and name == 'mod16_et_hdiag_f64' and a[6] == m
        assert seen['cls'] == list(CLS.flat[off:off + m])
        check_drivers(dict(dtype=np.dtype(np.float64), drivers=a[2], dstride=a[3], first=seen['first']), drv, off)
        assert a[4] is None and a[5] is None
        assert a[7:] == [got[0].ctypes.data + off * 8, got[1].ctypes.data + off * 8, _lib.MATH_FAST,
                         tiles + slot * 8 * 8]


def test_raster_writes_into_the_callers_arrays(rec):
    out = [np.empty(SHAPE), np.empty(SHAPE)]
    got = mod16_amd.evapotranspiration_raster(make_table(), CLS, *make_drivers(), out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert rec.take()[None][1][1]['out'] == (out[0].ctypes.data, out[1].ctypes.data, None)


def test_raster_rows_and_columns_take_the_two_level_path(rec):
    '''(T, N) = (2, 3): an (N,) class row, an (N,) driver row and a (T, 1) driver column stay as
    small as they are, and a device's share starts at a whole row.'''
    T, n = SHAPE
    drv = make_drivers()
    drv[2] = np.array([7.0, 8.0, 9.0])
    drv[3] = np.array([[0.25], [0.75]])
    cls = np.array([3, 4, 5], np.uint8)
    day, night = mod16_amd.evapotranspiration_raster(make_table(), cls, *drv, devices=[0, 0])
    assert day.shape == SHAPE and night.shape == SHAPE
    events = rec.take()
    kinds = [_lib.BC_SCALAR, _lib.BC_SCALAR, _lib.BC_ROW, _lib.BC_COL] + [_lib.BC_DENSE] * 10
    for slot, off in enumerate([0, 3]):
        (bp, _), (name, seen) = events[slot]
        assert bp == 'set_bplut' and name == 'et2'
        assert (seen['inner'], seen['n'], seen['cls_kind'], seen['cls']) == (n, 3, _lib.BC_ROW, cls.ctypes.data)
        assert seen['dkind'] == kinds and seen['params'] is None and seen['pkind'] is None
        assert seen['first'][:2] == [1.5, 2.5]
        assert seen['drivers'][2] == drv[2].ctypes.data                    # a row does not move
        assert seen['drivers'][3] == drv[3].ctypes.data + (off // n) * 8   # a column moves by rows
        for k in range(4, 14):
            assert seen['drivers'][k] == drv[k].ctypes.data + off * 8
        assert seen['out'] == (day.ctypes.data + off * 8, night.ctypes.data + off * 8, None)
        assert (seen['flags'], seen['where']) == (_lib.MATH_FAST, _lib.HOST)


def test_model_call_passes_parameters_and_returns_scalars_for_scalars(rec):
    names = mod16_amd.MOD16.required_parameters
    params = {k: float(j + 1) for j, k in enumerate(names)}
    model = mod16_amd.MOD16(params)
    site = [float(k) for k in range(14)]
    day, night = model.evapotranspiration(*site)
    assert type(day) is np.float64 and type(night) is np.float64
    (name, seen), = rec.take()[None]                 # no table without a class raster
    assert name == 'et' and seen['n'] == 1 and seen['cls'] is None and seen['dtype'] == np.float64
    assert seen['dstride'] == [0] * 14 and seen['pstride'] == [0] * 11
    assert seen['first'] == site and seen['pfirst'] == [float(j + 1) for j in range(11)]
    # components of an all-scalar call: the soil component is a scalar, the others 0-d arrays
    day, night = model.evapotranspiration(*site, separate=True)
    assert [type(o) for o in day] == [np.ndarray, np.float64, np.ndarray] and day[0].shape == ()
    assert [type(o) for o in night] == [np.ndarray, np.float64, np.ndarray]
    rec.take()
    # a year of one site, float32: arrays in, arrays out
    year = [np.full(365, v, np.float32) for v in site]
    day, night = model.evapotranspiration(*year)
    assert day.shape == (365,) and day.dtype == np.float32
    (name, seen), = rec.take()[None]
    assert name == 'et' and seen['dtype'] == np.float32 and seen['n'] == 365
    assert seen['drivers'] == [a.ctypes.data for a in year] and seen['dstride'] == [1] * 14
    # a per-site parameter row against (T, N) drivers
    params['beta'] = np.array([100.0, 200.0, 300.0])
    drv = [100.0 * k + np.arange(N, dtype=np.float64).reshape(SHAPE) for k in range(14)]
    mod16_amd.MOD16(params).evapotranspiration(*drv)
    (name, seen), = rec.take()[None]
    assert name == 'et2' and seen['inner'] == 3 and seen['n'] == N and seen['cls'] is None
    assert seen['dkind'] == [_lib.BC_DENSE] * 14 and seen['pkind'] == [_lib.BC_SCALAR] * 10 + [_lib.BC_ROW]
    assert seen['params'][10] == params['beta'].ctypes.data


# ------------------------------------------------------------------ the ensemble entry points
def test_ensemble_hands_over_the_stack_and_closes_it(rec):
    drv, table = make_drivers(), make_table()
    stack = np.stack([table, table + 1.0])
    got = mod16_amd.evapotranspiration_ensemble(stack, CLS, *drv, beta=250, math=_lib.MATH_EXACT, device=2)
    assert type(got) is mod16_amd.EnsembleET
    assert all(type(o) is np.ndarray and o.shape == SHAPE and o.dtype == np.float64 for o in got)
    (made, ens), (name, seen), (last, _) = rec.take()[None]
    assert made == 'ensemble' and ens['device'] == 2
    assert same(ens['tables'], np.stack([filled(table, 250), filled(table + 1.0, 250)]))
    assert name == 'run' and last == 'close' and seen['n'] == N and seen['cls_bytes'] == [1, 2, 3, 4, 5, 12]
    check_drivers(seen, drv, 0)
    assert seen['outs'] == [o.ctypes.data for o in got]
    assert (seen['flags'], seen['where'], seen['stream']) == (_lib.MATH_EXACT, _lib.HOST, None)
    # dicts, float32, the caller's arrays; scalars stay scalars
    names = mod16_amd.MOD16.required_parameters
    dicts = [{k: t[:, j] for j, k in enumerate(names)} for t in (table, table + 1.0)]
    out = [np.empty(SHAPE, np.float32) for _ in range(5)]
    got = mod16_amd.evapotranspiration_ensemble(dicts, CLS, *make_drivers(np.float32), beta=250, out=out)
    assert all(g is o for g, o in zip(got, out))
    (made, ens), (name, seen), (last, _) = rec.take()[None]
    assert same(ens['tables'], np.stack([filled(table, 250), filled(table + 1.0, 250)]))
    assert seen['dtype'] == np.float32 and seen['outs'] == [o.ctypes.data for o in out]
    got = mod16_amd.evapotranspiration_ensemble(stack, 3, *[float(k) for k in range(14)])
    assert all(type(o) is np.float64 for o in got)
    assert rec.take()[None][1][1]['n'] == 1


def test_ensemble_quantiles_lays_out_series_major_outputs(rec):
    drv, table = make_drivers(), make_table()
    stack = np.stack([table, table + 1.0, table + 2.0])
    got = mod16_amd.evapotranspiration_ensemble_quantiles(stack, CLS, *drv, q=(0.25, 0.75), beta=250,
                                                          slab_bytes=4096)
    assert type(got) is mod16_amd.EnsembleQuantiles and same(got.q, [0.25, 0.75]) and got.q.dtype == np.float64
    assert all(type(o) is np.ndarray and o.shape == (2,) + SHAPE and o.dtype == np.float64 for o in got[1:])
    (made, ens), (name, seen), (last, _) = rec.take()[None]
    assert made == 'ensemble' and ens['tables'].shape == (3, 13, 11) and ens['tables'][2, 1, 10] == 250
    assert name == 'quantiles' and last == 'close' and seen['n'] == N and seen['q'] == [0.25, 0.75]
    check_drivers(seen, drv, 0)
    assert seen['outs'] == [o.ctypes.data + k * N * 8 for o in got[1:] for k in range(2)]
    assert (seen['slab_bytes'], seen['flags'], seen['where']) == (4096, _lib.MATH_FAST, _lib.HOST)
    out = [np.empty((1,) + SHAPE, np.float32) for _ in range(3)]
    got = mod16_amd.evapotranspiration_ensemble_quantiles(stack, CLS, *make_drivers(np.float32), q=0.5, out=out)
    assert all(g is o for g, o in zip(got[1:], out))
    assert rec.take()[None][1][1]['outs'] == [o.ctypes.data for o in out]
    # all-scalar input gives (Q,) arrays
    got = mod16_amd.evapotranspiration_ensemble_quantiles(stack, 3, *[float(k) for k in range(14)])
    assert all(type(o) is np.ndarray and o.shape == (3,) for o in got[1:])


# ------------------------------------------------------------------ composite
def test_composite_sets_the_table_first_and_orders_its_outputs(rec):
    K = 3
    table = make_table()
    daily = [100.0 * k + np.arange(K * N, dtype=np.float64).reshape((K,) + SHAPE) for k in range(15)]
    arrays = list(daily)
    arrays[0] = 1.5
    arrays[7] = daily[7][0]                          # constant in time
    got = mod16_amd.evapotranspiration_composite(table, CLS, *arrays, period_days=2, pet=True, beta=250,
                                                 math=_lib.MATH_EXACT, stage_bytes=1 << 16)
    assert type(got) is mod16_amd.CompositeETPET
    assert [o.dtype for o in got] == [np.float64, np.float64, np.uint16, np.uint16]
    assert all(type(o) is np.ndarray and o.shape == (2,) + SHAPE for o in got)
    (bp, set_), (name, seen) = rec.take()[None]
    assert bp == 'set_bplut' and same(set_['table'], filled(table, 250)) and name == 'composite'
    assert (seen['n'], seen['days'], seen['period_days'], seen['out_pitch']) == (N, K, 2, N)
    assert seen['cls_bytes'] == [1, 2, 3, 4, 5, 12]
    assert seen['pixel_stride'] == [0] + [1] * 14
    assert seen['time_stride'] == [0] + [N] * 6 + [0] + [N] * 7
    assert seen['every'] == [K] + [1] * 6 + [K] + [1] * 7
    assert seen['first'][0] == 1.5
    assert seen['arrays'][1:] == [a.ctypes.data for a in arrays[1:]]
    assert seen['out'] == tuple(o.ctypes.data for o in got)               # et, pet, count_et, count_pet
    assert (seen['min_valid'], seen['rescale'], seen['flags'], seen['where'], seen['stage_bytes']) == \
        (1, False, _lib.MATH_EXACT, _lib.HOST, 1 << 16)
    # without pet: (et, count); the caller's arrays; float32
    out = [np.empty((2,) + SHAPE, np.float32), np.empty((2,) + SHAPE, np.uint16)]
    arrays32 = [np.asarray(a, np.float32) for a in daily]
    got = mod16_amd.evapotranspiration_composite(table, CLS.astype(np.uint8), *arrays32, period_days=2, out=out)
    assert type(got) is mod16_amd.CompositeET and got.et is out[0] and got.count is out[1]
    seen = rec.take()[None][1][1]
    assert seen['dtype'] == np.float32 and seen['out'] == (out[0].ctypes.data, None, out[1].ctypes.data, None)
    assert seen['stage_bytes'] is None


# ------------------------------------------------------------------ downscaled
def test_downscaled_deals_whole_rows_and_gives_every_device_the_table(rec):
    table = make_table()
    drv = make_drivers()
    coarse = ('temp_day', 'pressure')
    grid = {5: np.arange(4.0).reshape(2, 2), 11: 10 + np.arange(4.0).reshape(2, 2)}
    for k, v in grid.items():
        drv[k] = v
    row_pos, col_pos = np.array([0.25, 0.75]), np.array([0.0, 0.5, 1.0])
    got = mod16_amd.evapotranspiration_downscaled(table, CLS, *drv, row_pos, col_pos, wrap=True, coarse=coarse,
                                                  beta=250, devices=[0, 0, 0])
    assert type(got) is tuple and len(got) == 2
    assert all(type(o) is np.ndarray and o.shape == SHAPE and o.dtype == np.float64 for o in got)
    events = rec.take()
    assert sorted(events) == [0, 1, 2]
    assert [e[0] for e in events[2]] == ['set_bplut']               # two rows, three devices
    from mod16_amd import downscale as ds
    kinds = [ds.KIND_SCALAR, ds.KIND_SCALAR] + [ds.KIND_FINE] * 12
    kinds[5] = kinds[11] = ds.KIND_COARSE
    for slot, off in enumerate([0, 3]):
        (bp, set_), (made, g), (name, seen), (last, _) = events[slot]
        assert bp == 'set_bplut' and same(set_['table'], filled(table, 250))
        assert made == 'grid' and (g['shape'], g['coarse_shape'], g['wrap'], g['method']) == (SHAPE, (2, 2), True, 'bilinear')
        assert g['row_pos'] is row_pos and g['col_pos'] is col_pos and len(g['tables']) == 2
        assert name == 'run' and last == 'close' and seen['kinds'] == kinds
        assert (seen['coarse_pitch'], seen['first_pixel'], seen['n']) == (2, off, 3)
        assert seen['cls_bytes'] == list(CLS.flat[off:off + 3])
        assert seen['first'][:2] == [1.5, 2.5]
        for k in range(2, 14):
            assert seen['drivers'][k] == drv[k].ctypes.data + (0 if k in grid else off * 8)
        assert seen['out'] == (got[0].ctypes.data + off * 8, got[1].ctypes.data + off * 8)
        assert (seen['flags'], seen['where']) == (_lib.MATH_FAST, _lib.HOST)
    # one device, float32, the caller's arrays
    drv32 = [np.asarray(v, np.float32) if isinstance(v, np.ndarray) else v for v in drv]
    out = [np.empty(SHAPE, np.float32) for _ in range(2)]
    got = mod16_amd.evapotranspiration_downscaled(table, CLS, *drv32, row_pos, col_pos, coarse=coarse, out=out,
                                                  method='nearest', math=_lib.MATH_EXACT, device=1)
    assert got[0] is out[0] and got[1] is out[1]
    (bp, _), (made, g), (name, seen), (last, _) = rec.take()[None]
    assert g['device'] == 1 and g['method'] == 'nearest' and g['wrap'] is False
    assert seen['dtype'] == np.float32 and seen['n'] == N and seen['flags'] == _lib.MATH_EXACT
    assert seen['out'] == (out[0].ctypes.data, out[1].ctypes.data)


# ------------------------------------------------------------------ raw drivers
def test_raw_drivers_shift_every_raster_of_a_shard(rec):
    rec.tile = 4
    table = make_table()
    raw = make_drivers()
    fpar, lai = np.arange(10, 16).reshape(SHAPE), np.arange(20, 26).reshape(SHAPE)
    hours = 30.0 + np.arange(N, dtype=np.float64).reshape(SHAPE)
    got = mod16_amd.evapotranspiration_raw(table, CLS, *raw, fpar, lai, day_hours=hours, beta=250,
                                           math=_lib.MATH_EXACT, devices=[0, 0])
    assert type(got) is tuple and len(got) == 3
    assert all(type(o) is np.ndarray and o.shape == SHAPE and o.dtype == np.float64 for o in got)
    events = rec.take()
    for slot, (off, m) in enumerate([(0, 4), (4, 2)]):
        (bp, set_), (name, seen) = events[slot]
        a = seen['args']
        assert bp == 'set_bplut' and same(set_['table'], filled(table, 250)) and name == 'mod16_et_raw_f64'
        assert seen['cls'] == list(CLS.flat[off:off + m])
        check_drivers(dict(dtype=np.dtype(np.float64), drivers=a[2], dstride=a[3], first=seen['first']), raw, off)
        assert seen['fpar'] == list(fpar.flat[off:off + m]) and seen['lai'] == list(lai.flat[off:off + m])
        assert a[6] == hours.ctypes.data + off * 8 and a[7] == 1 and a[8] == m
        assert a[9:12] == [o.ctypes.data + off * 8 for o in got]
        assert a[12:] == [_lib.MATH_EXACT, _lib.HOST, None]
    # without the hours: two outputs, no hours array, float32; the empty shard gets its table
    rec.tile = BIG_TILE
    got = mod16_amd.evapotranspiration_raw(table, CLS.astype(np.uint8), *make_drivers(np.float32),
                                           fpar.astype(np.uint8), lai.astype(np.uint8), devices=[0, 0])
    assert len(got) == 2 and all(o.dtype == np.float32 for o in got)
    events = rec.take()
    assert [e[0] for e in events[1]] == ['set_bplut']
    a = events[0][1][1]['args']
    assert events[0][1][0] == 'mod16_et_raw_f32' and a[6] is None and a[7] == 0 and a[8] == N and a[11] is None
    # scalars stay scalars
    got = mod16_amd.evapotranspiration_raw(table, 3, *[float(k) for k in range(14)], 50, 20)
    assert all(type(o) is np.float64 for o in got)


# ------------------------------------------------------------------ gap filling, zonal statistics
def test_gapfill_series_flattens_the_pixels(rec):
    S = 3
    fpar = np.arange(S * N, dtype=np.uint8).reshape((S,) + SHAPE)
    lai = fpar + 100
    qc = np.zeros((S,) + SHAPE, np.uint8)
    clim = np.full(SHAPE, 9, np.uint8)
    (f, l), (sf, sl) = mod16_amd.gapfill_series((fpar, lai), qc=qc, max_gap=2, fallback=(clim, None),
                                                dtype='float32', scale=(0.01, 0.1), source=True, device=1,
                                                stage_bytes=1 << 16)
    assert all(type(o) is np.ndarray and o.shape == (S,) + SHAPE for o in (f, l, sf, sl))
    assert f.dtype == l.dtype == np.float32 and sf.dtype == sl.dtype == np.uint8
    (name, seen), = rec.take()[None]
    from mod16_amd import gapfill as gf
    assert name == 'gapfill' and (seen['out_type'], seen['n'], seen['slabs']) == (gf.OUT_TYPES['float32'], N, S)
    assert seen['fields'] == [fpar.ctypes.data, lai.ctypes.data] and seen['qc'] == qc.ctypes.data
    assert seen['fallback'] == [clim.ctypes.data, None]
    assert seen['good'] == [int(v) for v in gf.default_good()]
    assert seen['out'] == [f.ctypes.data, l.ctypes.data]
    assert seen['source'] == sf.ctypes.data and sl.ctypes.data == sf.ctypes.data + S * N
    assert seen['pitches'] == (N, N, N, N) and seen['max_gap'] == 2 and seen['scale'] == [0.01, 0.1, 1.0]
    assert (seen['where'], seen['stage_bytes']) == (_lib.HOST, 1 << 16)
    # one field: an array back, not a tuple; codes out
    filled_ = mod16_amd.gapfill_series(fpar)
    assert type(filled_) is np.ndarray and filled_.dtype == np.uint8 and filled_.shape == (S,) + SHAPE
    seen = rec.take()[None][0][1]
    assert seen['qc'] is None and seen['fallback'] is None and seen['source'] is None and seen['max_gap'] == -1
    assert seen['stage_bytes'] is None


def test_zonal_statistics_finds_its_bounds_then_accumulates(rec):
    from mod16_amd import zonal as zn
    values = np.arange(2 * N, dtype=np.float32).reshape((2,) + SHAPE)
    zones = np.array([[0, 1, 2], [2, 1, 0]], np.int64)
    area = np.array([0.5, 2.0])
    got = mod16_amd.zonal_statistics(values, zones, area=area, device=1, stage_bytes=1 << 16)
    assert type(got) is zn.ZonalResult and got.words.shape == (2, 3, zn.NWORDS) and got.count.shape == (2, 3)
    (first, b), (name, seen) = rec.take()[None]
    assert first == 'zonal_bounds' and name == 'zonal'
    assert (b['dtype'], b['n'], b['layers'], b['values']) == (np.float32, N, 2, values.ctypes.data)
    assert (b['weight_kind'], b['cols'], b['where'], b['stage_bytes']) == (_lib.ZONAL_WEIGHT_ROW, 3, _lib.HOST, 1 << 16)
    assert (seen['dtype'], seen['n'], seen['layers'], seen['nzones']) == (np.float32, N, 2, 3)
    assert seen['zone_type'] == zn.ZONE_TYPES['int32'] and seen['values'] == values.ctypes.data
    assert seen['weights'] == b['weights'] and seen['acc'] == got.words.ctypes.data
    assert seen['bounds'] == tuple(zn.check_bounds((2.0, 3.0))) and (got.ew, got.ex) == seen['bounds'][2:]
    assert (seen['weight_kind'], seen['cols'], seen['where'], seen['stage_bytes']) == \
        (_lib.ZONAL_WEIGHT_ROW, 3, _lib.HOST, 1 << 16)
    # explicit bounds: no pre-pass; zone ids of a type the library takes are read in place
    z8 = zones.astype(np.uint8)
    got = mod16_amd.zonal_statistics(values[0].astype(np.float64), z8, nzones=4, bounds=(1.0, 16.0))
    assert got.count.shape == (4,)
    (name, seen), = rec.take()[None]
    assert name == 'zonal' and seen['zones'] == z8.ctypes.data and seen['zone_type'] == zn.ZONE_TYPES['uint8']
    assert (seen['dtype'], seen['layers'], seen['nzones'], seen['weights']) == (np.float64, 1, 4, None)
    assert (seen['weight_kind'], seen['cols'], seen['stage_bytes']) == (_lib.ZONAL_WEIGHT_NONE, 1, None)


# ------------------------------------------------------------------ day / night, trend, anomaly, upscaling
DN_DAYS, DN_STEPS = 2, 2


def daynight_case(dtype=np.float32):
    '''(fields 't' and 'sw' of (D H,) + SHAPE, the three solar tables)'''
    from mod16_amd import daynight as dn
    steps = DN_DAYS * DN_STEPS
    fields = {'t': 280.0 + np.arange(steps * N, dtype=dtype).reshape((steps,) + SHAPE),
              'sw': 10.0 * np.arange(steps * N, dtype=dtype).reshape((steps,) + SHAPE), 'qv': None}
    return fields, dn.solar_tables(np.arange(1, DN_DAYS + 1), np.array([30.0, -30.0]), np.array([-90.0, 0.0, 90.0]))


def test_aggregate_daynight_allocates_by_name_or_writes_into_the_callers_arrays(rec):
    from mod16_amd import daynight as dn
    R, W = SHAPE
    fields, (half, noon, offset) = daynight_case()
    got, annual = mod16_amd.aggregate_daynight(fields, half, noon, offset, steps_per_day=DN_STEPS, device=1,
                                               stage_bytes=1 << 16)
    produced = ('sw_rad_day', 'temp_day', 'temp_night', 'tmin', 'day_hours', 'temp_mean')
    assert type(got) is dn.DayNight and type(annual) is np.ndarray
    for name in dn.OUTPUT_NAMES:
        o = getattr(got, name)
        assert (o is None) == (name not in produced), name
        assert o is None or (type(o) is np.ndarray and o.shape == (DN_DAYS,) + SHAPE and o.dtype == np.float32)
    assert annual.shape == SHAPE and annual.dtype == np.float32
    (name, seen), = rec.take()[None]
    assert name == 'daynight' and seen['dtype'] == np.float32 and seen['out_type'] == dn.OUT_TYPES['float32']
    assert seen['grid'] == (R, W, DN_DAYS, DN_STEPS)
    assert seen['fields'] == [fields['t'].ctypes.data, None, None, fields['sw'].ctypes.data, None]     # t, qv, ps, sw, lw
    assert all(same(t, want) and t.dtype == np.float64 for t, want in zip(seen['tables'], (half, noon, offset)))
    assert seen['out'] == [None if getattr(got, k) is None else getattr(got, k).ctypes.data for k in dn.OUTPUT_NAMES]
    assert seen['temp_annual'] == annual.ctypes.data
    assert seen['pitches'] == (W, R * W, W, R * W)
    assert (seen['mode'], seen['threshold'], seen['where'], seen['stream'], seen['stage_bytes']) == \
        (dn.MODES['solar'], 0.0, _lib.HOST, None, 1 << 16)
    # the caller's arrays by name, float64 out of float32 fields, a threshold on sw in place of the tables
    out = {'tmin': np.empty((DN_DAYS,) + SHAPE), 'temp_annual': np.empty(SHAPE)}
    got, annual = mod16_amd.aggregate_daynight(fields, sw_threshold=25.0, steps_per_day=DN_STEPS, dtype='float64',
                                               outputs=('temp_annual', 'tmin'), out=out)
    assert got.tmin is out['tmin'] and annual is out['temp_annual']
    assert [k for k in dn.OUTPUT_NAMES if getattr(got, k) is not None] == ['tmin']
    (name, seen), = rec.take()[None]
    assert seen['dtype'] == np.float32 and seen['out_type'] == dn.OUT_TYPES['float64'] and seen['tables'] is None
    assert seen['out'] == [out['tmin'].ctypes.data if k == 'tmin' else None for k in dn.OUTPUT_NAMES]
    assert seen['temp_annual'] == out['temp_annual'].ctypes.data
    assert (seen['mode'], seen['threshold'], seen['stage_bytes']) == (dn.MODES['sw'], 25.0, None)
    # no cells: the shapes, and nothing of the library
    empty = {'t': np.empty((DN_DAYS * DN_STEPS, 0, 3), np.float32)}
    got, annual = mod16_amd.aggregate_daynight(empty, sw_threshold=None, half_day=np.empty((DN_DAYS, 0)), offset=offset,
                                               steps_per_day=DN_STEPS, outputs=('tmin', 'temp_annual'))
    assert got.tmin.shape == (DN_DAYS, 0, 3) and annual.shape == (0, 3) and rec.take() == {}


def test_trend_series_flattens_the_pixels(rec):
    import statistics
    from mod16_amd import trend as tr
    Y = 4
    values = np.arange(Y * N, dtype=np.float32).reshape((Y,) + SHAPE)
    got = mod16_amd.trend_series(values, times=[0, 1, 2, 4], min_valid=3, alpha=0.1, device=1, stage_bytes=1 << 16)
    assert type(got) is tr.Trend
    assert [o.dtype for o in got] == [np.float64] * 4 + [np.int32, np.float64, np.uint8]
    assert all(type(o) is np.ndarray and o.shape == SHAPE for o in got)
    (name, seen), = rec.take()[None]
    assert name == 'trend' and (seen['dtype'], seen['n'], seen['steps']) == (np.float32, N, Y)
    assert seen['values'] == values.ctypes.data and seen['times'] == [0.0, 1.0, 2.0, 4.0]
    assert seen['out'] == [getattr(got, k).ctypes.data for k in tr.FLOAT_NAMES]
    assert (seen['s'], seen['count']) == (got.s.ctypes.data, got.count.ctypes.data)
    assert (seen['time_stride'], seen['min_valid'], seen['zq']) == (N, 3, statistics.NormalDist().inv_cdf(0.95))
    assert (seen['where'], seen['stream'], seen['stage_bytes']) == (_lib.HOST, None, 1 << 16)
    # without alpha: no interval, and no address for it; float64, the default times
    got = mod16_amd.trend_series(values.astype(np.float64))
    assert got.slope_lo is None and got.slope_hi is None and got.z.shape == SHAPE
    (name, seen), = rec.take()[None]
    assert seen['dtype'] == np.float64 and seen['times'] == [0.0, 1.0, 2.0, 3.0]
    assert seen['out'] == [got.slope.ctypes.data, got.intercept.ctypes.data, None, None, got.z.ctypes.data]
    assert (seen['min_valid'], seen['zq'], seen['stage_bytes']) == (4, 0.0, None)
    # no pixels: the shapes and dtypes, and nothing of the library
    got = mod16_amd.trend_series(np.empty((Y, 0, 3), np.float32), alpha=0.1)
    assert all(o.shape == (0, 3) for o in got) and got.s.dtype == np.int32 and got.count.dtype == np.uint8
    assert rec.take() == {}


def test_anomaly_series_lays_out_the_record_and_the_climatology(rec):
    from mod16_amd import anomaly as an
    Y, P = 3, 2
    num = np.arange(Y * P * N, dtype=np.float32).reshape((Y * P,) + SHAPE)
    den = num + 1
    got = mod16_amd.anomaly_series(num, den, periods=P, window=2, baseline=(0, 2), min_valid=2, outputs=an.OUTPUT_NAMES,
                                   device=1, stage_bytes=1 << 16)
    assert type(got) is an.Anomaly and all(type(o) is np.ndarray for o in got)
    assert [o.dtype for o in got] == [np.float32, np.float32, np.float64, np.float64, np.uint8]
    assert [o.shape for o in got] == [(Y * P,) + SHAPE] * 2 + [(P,) + SHAPE] * 3
    (name, seen), = rec.take()[None]
    assert name == 'anomaly' and (seen['dtype'], seen['n'], seen['years'], seen['periods']) == (np.float32, N, Y, P)
    assert (seen['num'], seen['den']) == (num.ctypes.data, den.ctypes.data)
    assert seen['out'] == [o.ctypes.data for o in got]
    assert (seen['window'], seen['baseline'], seen['min_valid']) == (2, (0, 2), 2)
    assert seen['strides'] == (None, None, None)                          # dense: the library's default
    assert (seen['where'], seen['stream'], seen['stage_bytes']) == (_lib.HOST, None, 1 << 16)
    # the defaults: z alone, no denominator, every year in the baseline; float64
    got = mod16_amd.anomaly_series(num.astype(np.float64), periods=P)
    assert got.z.dtype == np.float64 and got.z.shape == (Y * P,) + SHAPE and list(got[1:]) == [None] * 4
    (name, seen), = rec.take()[None]
    assert seen['dtype'] == np.float64 and seen['den'] is None and seen['out'] == [got.z.ctypes.data] + [None] * 4
    assert (seen['window'], seen['baseline'], seen['min_valid'], seen['stage_bytes']) == (1, (0, Y), 3, None)
    # no pixels: the shapes, and nothing of the library
    got = mod16_amd.anomaly_series(np.empty((Y * P, 0), np.float32), periods=P, outputs=('pct', 'count'))
    assert got.pct.shape == (Y * P, 0) and got.count.shape == (P, 0) and got.count.dtype == np.uint8 and got.z is None
    assert rec.take() == {}


UP_FINE, UP_COARSE = (4, 6), (2, 3)
UP_ROWS, UP_COLS = np.array([0.0, 0.2, 1.0, 1.2]), np.array([0.0, 0.1, 1.0, 1.1, 2.0, 2.1])


def check_cells(g, device, wrap, area):
    '''The grid an upscaling entry point makes: the runs of its own geometry check, no positions.'''
    assert (g['device'], g['shape'], g['coarse_shape'], g['wrap']) == (device, UP_FINE, UP_COARSE, wrap)
    assert g['row_pos'] is None and g['col_pos'] is None and g['col_affine'] is None
    assert (g['area'] is None) if area is None else (same(g['area'], area) and g['area'].dtype == np.float64)
    (rf, rc), (cf, cc) = g['runs']
    assert [list(t) for t in (rf, rc, cf, cc)] == [[0, 2], [2, 2], [0, 2, 4], [2, 2, 2]]


def test_upscale_fields_hands_over_layers_and_strides_and_closes_the_grid(rec):
    from mod16_amd import upscale as up
    K, (R, Cc), (H, W) = 2, UP_FINE, UP_COARSE
    values = np.arange(K * R * Cc, dtype=np.float32).reshape((K,) + UP_FINE)
    area = np.array([1, 2, 3, 4])
    got = mod16_amd.upscale_fields(values, UP_COARSE, UP_ROWS, UP_COLS, wrap=True, area=area, min_fraction=0.25,
                                   outputs=up.OUTPUT_NAMES, device=1, stage_bytes=1 << 16)
    assert type(got) is up.Upscaled and all(type(o) is np.ndarray and o.shape == (K,) + UP_COARSE for o in got)
    assert [o.dtype for o in got] == [np.float32, np.float32, np.int32]
    (made, g), (name, seen), (last, _) = rec.take()[None]
    assert made == 'cells' and name == 'run' and last == 'close'
    check_cells(g, 1, True, area)
    assert (seen['dtype'], seen['values'], seen['layers'], seen['strides']) == (np.float32, values.ctypes.data, K, (R * Cc, Cc))
    assert seen['min_fraction'] == 0.25 and seen['outs'] == [(o.ctypes.data, H * W, W) for o in got]
    assert (seen['where'], seen['stream'], seen['stage_bytes']) == (_lib.HOST, None, 1 << 16)
    # one layer without a layer axis: (H, W) back, the mean alone; float64
    got = mod16_amd.upscale_fields(values[0].astype(np.float64), UP_COARSE, UP_ROWS, UP_COLS)
    assert got.mean.shape == UP_COARSE and got.mean.dtype == np.float64 and got.fraction is None and got.count is None
    (made, g), (name, seen), (last, _) = rec.take()[None]
    check_cells(g, 0, False, None)
    assert (seen['dtype'], seen['layers'], seen['min_fraction']) == (np.float64, 1, 0.0)
    assert seen['outs'] == [(got.mean.ctypes.data, H * W, W), None, None] and seen['stage_bytes'] is None


def test_upscale_classes_makes_bytes_of_the_codes(rec):
    from mod16_amd import upscale as up
    (R, Cc), (H, W) = UP_FINE, UP_COARSE
    cls = np.arange(R * Cc).reshape(UP_FINE) % 13
    got = mod16_amd.upscale_classes(cls, UP_COARSE, UP_ROWS, UP_COLS, valid=(1, 2, 31), outputs=up.CLASS_OUTPUT_NAMES,
                                    device=1, stage_bytes=1 << 16)
    assert type(got) is up.UpscaledClasses and all(type(o) is np.ndarray and o.shape == UP_COARSE for o in got)
    assert (got.cls.dtype, got.share.dtype) == (np.uint8, np.float32)
    (made, g), (name, seen), (last, _) = rec.take()[None]
    assert made == 'cells' and name == 'classes' and last == 'close'
    check_cells(g, 1, False, None)
    assert seen['cls_bytes'] == [int(c) for c in cls.flat]                # int64 codes became bytes
    assert (seen['row_stride'], seen['valid']) == (Cc, (1 << 1) | (1 << 2) | (1 << 31))
    assert seen['out'] == ((got.cls.ctypes.data, W), (got.share.ctypes.data, W))
    assert (seen['where'], seen['stream'], seen['stage_bytes']) == (_lib.HOST, None, 1 << 16)
    # uint8 codes are read in place; the default: the class alone, the 13 classes of the table
    c8 = cls.astype(np.uint8)
    got = mod16_amd.upscale_classes(c8, UP_COARSE, UP_ROWS, UP_COLS)
    assert got.share is None
    seen = rec.take()[None][1][1]
    assert seen['cls'] == c8.ctypes.data and seen['valid'] == (1 << 13) - 1
    assert seen['out'] == ((got.cls.ctypes.data, W), None) and seen['stage_bytes'] is None


# ------------------------------------------------------------------ refusals
def _raster(**kw):
    kw.setdefault('cls', CLS)
    return mod16_amd.evapotranspiration_raster(make_table(), kw.pop('cls'), *make_drivers(), **kw)


def _ensemble(**kw):
    kw.setdefault('cls', CLS)
    stack = np.stack([make_table()] * 2)
    return mod16_amd.evapotranspiration_ensemble(stack, kw.pop('cls'), *make_drivers(), **kw)


def _quantiles(**kw):
    kw.setdefault('cls', CLS)
    stack = np.stack([make_table()] * 2)
    return mod16_amd.evapotranspiration_ensemble_quantiles(stack, kw.pop('cls'), *make_drivers(), **kw)


def _composite(**kw):
    kw.setdefault('cls', CLS)
    daily = [np.ones((1,) + SHAPE)] * 15
    return mod16_amd.evapotranspiration_composite(make_table(), kw.pop('cls'), *daily, **kw)


def _downscaled(**kw):
    kw.setdefault('cls', CLS)
    return mod16_amd.evapotranspiration_downscaled(make_table(), kw.pop('cls'), *make_drivers(), np.zeros(2),
                                                   np.zeros(3), coarse=(), **kw)


def _raw(**kw):
    u8 = dict(cls=CLS, fpar_pct=np.full(SHAPE, 50), lai_x10=np.full(SHAPE, 20))
    u8.update((k, kw.pop(k)) for k in list(kw) if k in u8)
    return mod16_amd.evapotranspiration_raw(make_table(), u8['cls'], *make_drivers(), u8['fpar_pct'], u8['lai_x10'],
                                            **kw)


def _gapfill(**kw):
    return mod16_amd.gapfill_series(np.zeros((3,) + SHAPE, np.uint8), **kw)


def _zonal(**kw):
    return mod16_amd.zonal_statistics(np.zeros(SHAPE), np.zeros(SHAPE, np.uint8), **kw)


def _daynight(**kw):
    fields, (half, noon, offset) = daynight_case(np.float64)
    kw.setdefault('outputs', ('tmin', 'temp_annual'))
    return mod16_amd.aggregate_daynight(kw.pop('fields', fields), half, noon, offset, steps_per_day=DN_STEPS, **kw)


def _trend(**kw):
    return mod16_amd.trend_series(kw.pop('values', np.zeros((4,) + SHAPE)), **kw)


def _anomaly(**kw):
    kw.setdefault('periods', 2)
    return mod16_amd.anomaly_series(kw.pop('num', np.zeros((6,) + SHAPE)), **kw)


def _upscale(**kw):
    return mod16_amd.upscale_fields(kw.pop('values', np.zeros(UP_FINE)), UP_COARSE, UP_ROWS, UP_COLS, **kw)


def _classes(**kw):
    return mod16_amd.upscale_classes(kw.pop('cls', np.zeros(UP_FINE, np.uint8)), UP_COARSE, UP_ROWS, UP_COLS, **kw)


BAD_CLS = np.array([[1, 2, 3], [4, 5, 256]])
NEG_CLS = np.array([[1, 2, 3], [4, 5, -1]])
CLASS_CODE = 'class code outside [0, 255]'
OUT_F64 = 'out arrays must be writeable C-contiguous float64 arrays of shape (2, 3)'

REFUSALS = [
    # the cases the entry points share
    (_raster, dict(cls=BAD_CLS), IndexError, CLASS_CODE),
    (_raster, dict(cls=NEG_CLS), IndexError, CLASS_CODE),
    (_ensemble, dict(cls=BAD_CLS), IndexError, CLASS_CODE),
    (_quantiles, dict(cls=BAD_CLS), IndexError, CLASS_CODE),
    (_composite, dict(cls=BAD_CLS), IndexError, CLASS_CODE),
    (_downscaled, dict(cls=BAD_CLS), IndexError, CLASS_CODE),
    (_raw, dict(cls=BAD_CLS), IndexError, 'uint8 raster value outside [0, 255]'),
    (_raw, dict(fpar_pct=np.full(SHAPE, 300)), IndexError, 'uint8 raster value outside [0, 255]'),
    (_raw, dict(lai_x10=np.full(SHAPE, -1)), IndexError, 'uint8 raster value outside [0, 255]'),
    (_raster, dict(out=[np.empty(SHAPE)]), ValueError, 'out must hold 2 arrays'),
    (_raster, dict(out=[np.empty(SHAPE)] * 2, separate=True), ValueError, 'out must hold 6 arrays'),
    (_raster, dict(out=[np.empty(SHAPE)] * 2, pet=True), ValueError, 'out must hold 4 arrays'),
    (_ensemble, dict(out=[np.empty(SHAPE)] * 2), ValueError, 'out must hold 5 arrays'),
    (_quantiles, dict(out=[np.empty(SHAPE)] * 2), ValueError, 'out must hold 3 arrays'),
    (_composite, dict(out=[np.empty((1,) + SHAPE)]), ValueError, 'out must hold 2 arrays'),
    (_composite, dict(out=[np.empty((1,) + SHAPE)], pet=True), ValueError, 'out must hold 4 arrays'),
    (_downscaled, dict(out=[np.empty(SHAPE)]), ValueError, 'out must hold 2 arrays'),
    (_raster, dict(out=[np.empty(SHAPE), np.empty((3, 2))]), ValueError, OUT_F64),
    (_raster, dict(out=[np.empty(SHAPE), np.empty(SHAPE, np.float32)]), ValueError, OUT_F64),
    (_raster, dict(out=[np.empty(SHAPE), np.empty((2, 6))[:, ::2]]), ValueError, OUT_F64),
    (_raster, dict(out=[np.empty(SHAPE), [[0.0] * 3] * 2]), ValueError, OUT_F64),
    (_ensemble, dict(out=[np.empty(SHAPE)] * 4 + [np.empty(N)]), ValueError, OUT_F64),
    (_quantiles, dict(out=[np.empty((3,) + SHAPE)] * 2 + [np.empty(SHAPE)]), ValueError,
     'out arrays must be writeable C-contiguous float64 arrays of shape (3, 2, 3)'),
    (_downscaled, dict(out=[np.empty(SHAPE), np.empty(SHAPE, np.float32)]), ValueError, OUT_F64),
    (_composite, dict(out=[np.empty((1,) + SHAPE), np.empty((1,) + SHAPE)]), ValueError,
     'out[1] must be a writeable C-contiguous uint16 array of shape (1, 2, 3)'),
    (_composite, dict(out=[np.empty(SHAPE), np.empty((1,) + SHAPE, np.uint16)]), ValueError,
     'out[0] must be a writeable C-contiguous float64 array of shape (1, 2, 3)'),
    (_composite, dict(out=[np.empty((1,) + SHAPE)] * 3 + [np.empty((1,) + SHAPE, np.uint16)], pet=True), ValueError,
     'out[2] must be a writeable C-contiguous uint16 array of shape (1, 2, 3)'),
    (_composite, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_gapfill, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_zonal, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    # two faults at once: which one wins
    (_raster, dict(cls=BAD_CLS, out=[np.empty(SHAPE)]), IndexError, CLASS_CODE),
    (_raster, dict(cls=BAD_CLS, diagnostics=True, pet=True), IndexError, CLASS_CODE),
    (_raster, dict(out=[np.empty(SHAPE)], diagnostics=True, pet=True), ValueError,
     'diagnostics come with the (day, night) totals only'),
    (_raster, dict(cls=BAD_CLS, devices=[]), ValueError, 'devices must name at least one GPU'),
    (_ensemble, dict(cls=BAD_CLS, out=[np.empty(SHAPE)]), IndexError, CLASS_CODE),
    (_quantiles, dict(cls=BAD_CLS, out=[np.empty(SHAPE)]), IndexError, CLASS_CODE),
    (_quantiles, dict(cls=BAD_CLS, q=1.5), ValueError, None),
    (_composite, dict(cls=BAD_CLS, stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_composite, dict(cls=BAD_CLS, out=[np.empty(SHAPE)]), IndexError, CLASS_CODE),
    (_composite, dict(stage_bytes=-1, math=2), ValueError, 'math must be MATH_FAST or MATH_EXACT for the composite run'),
    (_downscaled, dict(cls=BAD_CLS, out=[np.empty(SHAPE)]), IndexError, CLASS_CODE),
    (_downscaled, dict(cls=BAD_CLS, math=2), ValueError, 'math must be MATH_FAST or MATH_EXACT for the downscaled run'),
    (_downscaled, dict(cls=BAD_CLS, devices=[-1]), ValueError, 'negative device index'),
    (_raw, dict(cls=BAD_CLS, devices=[]), ValueError, 'devices must name at least one GPU'),
    (_gapfill, dict(stage_bytes=-1, qc=np.zeros((3,) + SHAPE, np.int16)), ValueError, 'qc must be uint8, got int16'),
    (_gapfill, dict(stage_bytes=-1, max_gap=-1), ValueError, 'max_gap must be None or at least 0, got -1'),
    (_zonal, dict(stage_bytes=-1, area=np.zeros(5)), ValueError,
     'area must be a scalar, (rows,) for a 2-D raster or of the shape of zones (2, 3), got (5,)'),
    (_zonal, dict(stage_bytes=-1, acc='no result'), ValueError, 'stage_bytes must not be negative'),
    # day / night: the out= dict -- its key set, then per name dtype, shape, layout, type
    (_daynight, dict(out={'tmin': np.empty((2,) + SHAPE)}), ValueError,
     'out must hold exactly the requested outputs: tmin, temp_annual'),
    (_daynight, dict(out={'tmin': np.empty((2,) + SHAPE), 'temp_annual': np.empty(SHAPE), 'temp_day': np.empty((2,) + SHAPE)}),
     ValueError, 'out must hold exactly the requested outputs: tmin, temp_annual'),
    (_daynight, dict(out={'tmin': np.empty((2,) + SHAPE, np.float32), 'temp_annual': np.empty(SHAPE)}), ValueError,
     "out['tmin'] must be a writeable C-contiguous float64 array of shape (2, 2, 3)"),
    (_daynight, dict(out={'tmin': np.empty((2,) + SHAPE), 'temp_annual': np.empty((1,) + SHAPE)}), ValueError,
     "out['temp_annual'] must be a writeable C-contiguous float64 array of shape (2, 3)"),
    (_daynight, dict(out={'tmin': np.empty((2, 2, 6))[:, :, ::2], 'temp_annual': np.empty(SHAPE)}), ValueError,
     "out['tmin'] must be a writeable C-contiguous float64 array of shape (2, 2, 3)"),
    (_daynight, dict(out={'tmin': [[0.0]], 'temp_annual': np.empty(SHAPE)}), ValueError,
     "out['tmin'] must be a writeable C-contiguous float64 array of shape (2, 2, 3)"),
    (_daynight, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_daynight, dict(stage_bytes=-1, out={'tmin': np.empty((2,) + SHAPE)}), ValueError, 'stage_bytes must not be negative'),
    (_daynight, dict(stage_bytes=-1, dtype='int16'), ValueError, "dtype must be 'float32' or 'float64', got 'int16'"),
    (_daynight, dict(outputs=('vpd_day',)), ValueError, "outputs: 'vpd_day' needs the field 'qv'"),
    # trend
    (_trend, dict(values=np.zeros((4,) + SHAPE, np.int64)), ValueError, 'values must be float32 or float64, got int64'),
    (_trend, dict(values=np.zeros((1,) + SHAPE)), ValueError,
     'values must have shape (Y,) + pixel shape with 2 <= Y <= 64, got (1, 2, 3)'),
    (_trend, dict(times=np.arange(3.0)), ValueError, 'times must have shape (4,), got (3,)'),
    (_trend, dict(min_valid=1), ValueError, 'min_valid must be an integer between 2 and Y = 4, got 1'),
    (_trend, dict(alpha=0.7), ValueError, 'alpha must be None or a level in (0, 0.5], got 0.7'),
    (_trend, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_trend, dict(stage_bytes=-1, alpha=0.7), ValueError, 'alpha must be None or a level in (0, 0.5], got 0.7'),
    (_trend, dict(values=np.zeros((4,) + SHAPE, np.int64), min_valid=1), ValueError,
     'values must be float32 or float64, got int64'),
    # anomaly
    (_anomaly, dict(den=np.zeros((6, 3))), ValueError, 'den must have the shape of num (6, 2, 3), got (6, 3)'),
    (_anomaly, dict(den=np.zeros((6,) + SHAPE, np.float32)), ValueError,
     'den must have the dtype of num (float64), got float32'),
    (_anomaly, dict(periods=None), ValueError, 'periods must be given'),
    (_anomaly, dict(num=np.zeros((6,) + SHAPE, np.int64)), ValueError, 'num must be float32 or float64, got int64'),
    (_anomaly, dict(periods=4), ValueError,
     'num must have shape (S,) + pixel shape with S = Y * periods and 2 <= Y <= 64, got (6, 2, 3) with periods = 4'),
    (_anomaly, dict(window=3), ValueError, 'window must be between 1 and min(periods, 16) = 2, got 3'),
    (_anomaly, dict(baseline=(0, 1)), ValueError, 'the baseline needs at least 2 years, got (0, 1)'),
    (_anomaly, dict(min_valid=1), ValueError, 'min_valid must be between 2 and the baseline length 3, got 1'),
    (_anomaly, dict(outputs=('q',)), ValueError,
     "outputs must name one or more of z, pct, mean, std, count, each once, got ('q',)"),
    (_anomaly, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_anomaly, dict(periods=None, den=np.zeros((6, 3))), ValueError, 'den must have the shape of num (6, 2, 3), got (6, 3)'),
    (_anomaly, dict(periods=None, num=np.zeros((6,) + SHAPE, np.int64)), ValueError,
     'num must be float32 or float64, got int64'),
    (_anomaly, dict(periods=None, outputs=('q',)), ValueError, 'periods must be given'),
    (_anomaly, dict(stage_bytes=-1, outputs=('q',)), ValueError,
     "outputs must name one or more of z, pct, mean, std, count, each once, got ('q',)"),
    # upscaling
    (_upscale, dict(values=np.zeros(6)), ValueError, 'values must have shape (K, R, C) or (R, C), got (6,)'),
    (_upscale, dict(values=np.zeros(UP_FINE, np.int64)), ValueError, 'values must be float32 or float64, got int64'),
    (_upscale, dict(values=np.zeros((2, 3, 6))), ValueError,
     'row_pos and col_pos must have shapes (3,) and (6,), got (4,) and (6,)'),
    (_upscale, dict(min_fraction=2), ValueError, 'min_fraction must lie in [0, 1], got 2'),
    (_upscale, dict(area=np.ones(3)), ValueError, 'area must have shape (4,) -- a weight per fine row --, got (3,)'),
    (_upscale, dict(outputs=('mean', 'mean')), ValueError,
     "outputs must name one or more of mean, fraction, count, each once, got ('mean', 'mean')"),
    (_upscale, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_upscale, dict(stage_bytes=-1, outputs=()), ValueError,
     'outputs must name one or more of mean, fraction, count, each once, got ()'),
    (_classes, dict(cls=np.zeros((1,) + UP_FINE, np.uint8)), ValueError,
     'cls must be a two-dimensional class raster, got shape (1, 4, 6)'),
    (_classes, dict(cls=np.full(UP_FINE, 256)), IndexError, CLASS_CODE),
    (_classes, dict(valid=[40]), ValueError, 'valid must hold class codes in [0, 32), got 40'),
    (_classes, dict(outputs=('mean',)), ValueError,
     "outputs must name one or more of cls, share, each once, got ('mean',)"),
    (_classes, dict(stage_bytes=-1), ValueError, 'stage_bytes must not be negative'),
    (_classes, dict(stage_bytes=-1, valid=[True]), ValueError, 'valid must hold class codes in [0, 32), got True'),
]


@pytest.mark.parametrize('call, kw, exc, message', REFUSALS,
                         ids=['%s-%d' % (r[0].__name__.lstrip('_'), i) for i, r in enumerate(REFUSALS)])
def test_refusals_come_before_the_library_with_their_exact_message(no_library, call, kw, exc, message):
    with pytest.raises(exc) as info:
        call(**kw)
    assert type(info.value) is exc
    if message is not None:
        assert str(info.value) == message
