"""The definition of the day / night aggregation (mod16_amd/daynight.py: day_weights, sw_weights,
split_field, aggregate, solar_tables, check_call) and its interface, without a GPU: numpy only, plus
the loaded library's prototypes and its refusal of a NULL context.

Weight properties on a 7 x 576 grid (rows with half_day exactly 0 and exactly 12 among random ones,
noon in 12 +- 0.3, longitudes -180 ... 179.375) for H in (1, 8, 24, 48), D = 5: 0 <= w <= 1;
|day_hours - 2 half_day| <= 1e-12 hours (the numpy prototype of the formula gives at most 1.1e-14: a few
hundred ulps of 24 are the bound); energy closure day hours + night (24 - hours) = delta sum X within
1e-12 relative on positive data."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mod16_amd import daynight as dn

HEADER = os.path.join(ROOT, 'include', 'mod16_hip.h')
R, W, D = 7, 576, 5


def tables(seed=3, days=D, rows=R, cols=W):
    rng = np.random.default_rng(seed)
    half = rng.uniform(0.0, 12.0, (days, rows))
    half[:, 0] = 0.0            # polar night
    half[:, -1] = 12.0          # polar day
    half[0, 1], half[1, 1] = 12.0, 0.0
    noon = 12.0 + rng.uniform(-0.3, 0.3, days)
    offset = (-180.0 + 360.0 / cols * np.arange(cols)) / 15.0
    return half, noon, offset


@pytest.mark.parametrize('H', (1, 8, 24, 48))
def test_weights_are_fractions_and_add_up_to_the_day_length(H):
    half, noon, offset = tables()
    assert offset[0] == -12.0 and abs(offset[-1] * 15.0 - 179.375) < 1e-12
    w = dn.day_weights(H, half, noon, offset)
    assert w.shape == (D, H, R, W) and w.dtype == np.float64
    assert w.min() >= 0.0 and w.max() <= 1.0
    sum_w, sum_n = dn.split_weights(w)
    hours = (24.0 / H) * sum_w
    err = np.abs(hours - 2.0 * half[:, :, None]).max()
    print('H = %d: max |day_hours - 2 half_day| = %.3g h' % (H, err))
    assert err <= 1e-12
    assert np.all(sum_w[:, 0] == 0.0)          # polar night: a == b, every window is empty, exactly
    # energy closure on positive data
    rng = np.random.default_rng(11)
    x = rng.uniform(1.0, 400.0, (D * H, R, W))
    day, night, mean = dn.split_field(x, w)
    total = (24.0 / H) * x.reshape(D, H, R, W).sum(axis=1)
    closed = day * hours + night * (24.0 - hours)
    rel = np.abs(closed - total) / total
    print('H = %d: energy closure, max relative error %.3g' % (H, rel.max()))
    assert rel.max() <= 1e-12


def test_every_window_contributes_somewhere():
    """the three windows m = -H, 0, +H of the weight formula are all needed over the full circle"""
    H = 24
    half, noon, offset = tables()
    delta = 24.0 / H
    a = ((noon[:, None, None] - half[:, :, None]) - offset[None, None, :]) / delta
    b = ((noon[:, None, None] + half[:, :, None]) - offset[None, None, :]) / delta
    k = np.arange(H, dtype=np.float64)[None, :, None, None]
    for m in (-float(H), 0.0, float(H)):
        term = np.maximum(np.minimum(k + 1.0, b[:, None] + m) - np.maximum(k, a[:, None] + m), 0.0)
        assert term.max() > 0.0, m


def small_fields(seed=5, days=3, H=8, rows=4, cols=6, dtype=np.float64):
    rng = np.random.default_rng(seed)
    shape = (days * H, rows, cols)
    return {'t': rng.uniform(250.0, 310.0, shape).astype(dtype), 'qv': rng.uniform(0.001, 0.02, shape).astype(dtype),
            'ps': rng.uniform(6e4, 1.02e5, shape).astype(dtype), 'sw': rng.uniform(0.0, 900.0, shape).astype(dtype),
            'lw': rng.uniform(-120.0, -10.0, shape).astype(dtype)}


def test_polar_night_and_polar_day_fall_back_to_the_mean():
    """half_day = 0 gives weights of exactly 0 at every longitude (a == b: every window is empty).
    half_day = 12 gives exactly 1 where sunrise falls on a step boundary -- here: noon 12 and offsets
    of whole steps -- and the fallback is then taken, bit for bit; at other longitudes the two pieces
    of the step that holds sunrise may add up to 1 - 1 ulp, sum_n is then a few 1e-16 and the night
    value a finite weighted one (it is multiplied by 24 - day_hours <= 1e-14 hours downstream)."""
    days, H, rows, cols = 3, 8, 4, 6
    f = small_fields()
    half, noon, offset = tables(days=days, rows=rows, cols=cols)
    res, annual = dn.aggregate(f, H, half, noon, offset)
    for name in dn.OUTPUT_NAMES:
        assert np.all(np.isfinite(getattr(res, name))), name
    assert np.all(np.isfinite(annual))
    assert np.all(res.day_hours[:, 0] == 0.0) and np.abs(res.day_hours[:, -1] - 24.0).max() <= 1e-12
    whole = np.array([-12.0, -9.0, -6.0, 0.0, 3.0, 9.0])      # multiples of delta = 3 h
    res, annual = dn.aggregate(f, H, half, None, whole)
    for name in dn.OUTPUT_NAMES:
        assert np.all(np.isfinite(getattr(res, name))), name
    assert np.all(res.day_hours[:, 0] == 0.0) and np.all(res.day_hours[:, -1] == 24.0)
    w = dn.day_weights(H, half, np.full(days, 12.0), whole)
    for field, day_name, night_name in (('lw', 'lw_net_day', 'lw_net_night'), ('t', 'temp_day', 'temp_night')):
        day, night, mean = dn.split_field(f[field], w)
        want = f[field].reshape(days, H, rows, cols).sum(axis=1) / H
        assert np.allclose(mean, want, rtol=1e-14, atol=0)
        assert np.array_equal(getattr(res, day_name)[:, 0], mean[:, 0])          # polar night: no day steps
        assert np.array_equal(getattr(res, night_name)[:, -1], mean[:, -1])      # polar day: no night steps
        assert np.array_equal(getattr(res, night_name)[:, 0], mean[:, 0])        # ... and the other half IS the mean
        assert np.array_equal(getattr(res, day_name)[:, -1], mean[:, -1])
    assert np.array_equal(res.temp_mean, dn.split_field(f['t'], w)[2])
    assert res.lw_net_day.dtype == np.float64
    r32, a32 = dn.aggregate({k: v.astype(np.float32) for k, v in f.items()}, H, half, noon, offset)
    assert r32.tmin.dtype == np.float32 and a32.dtype == np.float32
    r64, _ = dn.aggregate({k: v.astype(np.float32) for k, v in f.items()}, H, half, noon, offset, dtype='float64')
    assert r64.tmin.dtype == np.float64 and np.array_equal(r64.tmin.astype(np.float32), r32.tmin)


@pytest.mark.parametrize('field', dn.FIELD_NAMES)
def test_a_nan_step_poisons_only_its_field_in_solar_mode(field):
    days, H, rows, cols = 3, 8, 4, 6
    f = small_fields()
    f[field] = f[field].copy()
    f[field][1 * H + 3, 2, 4] = np.nan
    half, noon, offset = tables(days=days, rows=rows, cols=cols)
    res, annual = dn.aggregate(f, H, half, noon, offset)
    poisoned = {'t': ('temp_day', 'temp_night', 'tmin', 'temp_mean', 'vpd_day', 'vpd_night'),
                'qv': ('vpd_day', 'vpd_night'), 'ps': ('vpd_day', 'vpd_night'), 'sw': ('sw_rad_day',),
                'lw': ('lw_net_day', 'lw_net_night')}[field]
    for name in dn.OUTPUT_NAMES:
        nan = np.isnan(getattr(res, name))
        if name in poisoned:
            assert nan[1, 2, 4] and nan.sum() == 1, name
        else:
            assert not nan.any(), name
    assert np.isnan(annual).sum() == (1 if field == 't' else 0)


def test_sw_mode_against_a_hand_written_loop():
    days, H, rows, cols = 2, 4, 2, 3
    f = small_fields(days=days, H=H, rows=rows, cols=cols)
    f['sw'][:H, 0, 0] = 0.0         # a cell without a day step on day 0
    f['sw'][:H, 0, 1] = 800.0       # ... without a night step
    f['sw'][H + 1, 1, 2] = np.nan   # a missing step: the weight is NaN
    thr = 20.0
    res, annual = dn.aggregate(f, H, sw_threshold=thr)
    delta = np.float64(24.0) / np.float64(H)
    for d in range(days):
        for r in range(rows):
            for c in range(cols):
                sw_, sn, st, sd, snn, tmin = (np.float64(0.0),) * 5 + (np.float64(np.inf),)
                nan_t = False
                for k in range(H):
                    s = np.float64(f['sw'][d * H + k, r, c])
                    w = np.float64(np.nan) if np.isnan(s) else np.float64(1.0 if s > thr else 0.0)
                    t = np.float64(f['t'][d * H + k, r, c])
                    sw_, sn = sw_ + w, sn + (1.0 - w)
                    st, sd, snn = st + t, sd + w * t, snn + (1.0 - w) * t
                    tmin = min(tmin, t)
                mean = st / np.float64(H)
                day = sd / sw_ if sw_ > 0 else mean
                night = snn / sn if sn > 0 else mean
                for got, want in ((res.temp_day, day), (res.temp_night, night), (res.temp_mean, mean),
                                  (res.day_hours, delta * sw_), (res.tmin, tmin)):
                    g = got[d, r, c]
                    assert (np.isnan(g) and np.isnan(want)) or g == want, (d, r, c)
    assert res.day_hours[0, 0, 0] == 0.0 and res.day_hours[0, 0, 1] == 24.0
    assert np.isnan(res.day_hours[1, 1, 2]) and np.isfinite(res.temp_mean[1, 1, 2])
    assert res.sw_rad_day[0, 0, 0] == 0.0 and np.isfinite(res.lw_net_day[0, 0, 0])
    assert np.array_equal(annual, (res.temp_mean[0] + res.temp_mean[1]) / 2.0)


def test_vpd_follows_the_aggregated_values_and_clamps_the_night():
    days, H, rows, cols = 3, 8, 4, 6
    f = small_fields()
    f['qv'][:, 0, 0] = 0.05         # above saturation at these temperatures
    half, noon, offset = tables(days=days, rows=rows, cols=cols)
    res, _ = dn.aggregate(f, H, half, noon, offset)
    w = dn.day_weights(H, half, noon, offset)
    parts = {k: dn.split_field(f[k], w) for k in ('t', 'qv', 'ps')}
    assert np.array_equal(res.vpd_day, dn.vpd(parts['qv'][0], parts['ps'][0], parts['t'][0]))
    night = dn.vpd(parts['qv'][1], parts['ps'][1], parts['t'][1])
    assert (night[:, 0, 0] < 0).all() and np.all(res.vpd_night[:, 0, 0] == 0.0)
    assert np.array_equal(res.vpd_night, np.where(night < 0, 0.0, night))
    assert (res.vpd_day[:, 0, 0] < 0).all()        # the day value is not clamped


def test_outputs_may_be_left_out_and_fields_with_them():
    days, H, rows, cols = 3, 8, 4, 6
    f = small_fields()
    half, noon, offset = tables(days=days, rows=rows, cols=cols)
    full, annual = dn.aggregate(f, H, half, noon, offset)
    res, ann = dn.aggregate({'lw': f['lw']}, H, half, noon, offset)
    assert [n for n in dn.OUTPUT_NAMES if getattr(res, n) is not None] == ['lw_net_day', 'lw_net_night', 'day_hours']
    assert ann is None and np.array_equal(res.lw_net_day, full.lw_net_day)
    res, ann = dn.aggregate({'t': f['t']}, H, half, noon, offset, outputs=('tmin', 'temp_annual'))
    assert [n for n in dn.OUTPUT_NAMES if getattr(res, n) is not None] == ['tmin']
    assert np.array_equal(ann, annual) and np.array_equal(res.tmin, full.tmin)


def test_solar_tables():
    lat = np.array([90.0, 45.0, 0.0, -45.0, -90.0])
    lon = np.array([-180.0, 0.0, 179.375])
    doy = np.array([81, 172, 355])          # March equinox, June and December solstice (Cooper's formula)
    half, noon, offset = dn.solar_tables(doy, lat, lon)
    assert half.shape == (3, 5) and noon.shape == (3,) and offset.shape == (3,)
    assert np.all(noon == 12.0) and np.array_equal(offset, lon / 15.0)
    assert np.allclose(half[:, 2], 6.0, rtol=0, atol=1e-12)           # the equator: 12 h every day
    assert abs(half[0, 1] - 6.0) < 1e-6                               # equinox: 12 h everywhere
    assert half[1, 0] == 12.0 and half[1, 4] == 0.0                   # June: polar day in the north
    assert half[2, 0] == 0.0 and half[2, 4] == 12.0                   # December: the other way round
    assert np.allclose(half + half[:, ::-1], 12.0, rtol=0, atol=1e-12)     # symmetric in latitude
    assert half[1, 1] > 7.5 and half[2, 1] < 4.5
    dn.check_call({'t': (3 * 24, 5, 3)}, 24, half, noon, offset)
    with pytest.raises(ValueError, match='lat must lie'):
        dn.solar_tables(doy, [91.0], lon)
    with pytest.raises(ValueError, match='lon must lie'):
        dn.solar_tables(doy, lat, [181.0])


def test_every_refusal_of_check_call_has_its_message():
    H, days, rows, cols = 24, 2, 3, 4
    shape = (days * H, rows, cols)
    half, noon, offset = np.full((days, rows), 6.0), np.full(days, 12.0), np.zeros(cols)
    good = dict(shapes={'t': shape, 'sw': shape}, steps_per_day=H, half_day=half, noon=noon, offset=offset)
    got = dn.check_call(**good)
    assert got[:5] == (days, H, rows, cols, 'solar') and got[7] == ('sw_rad_day', 'temp_day', 'temp_night', 'tmin',
                                                                   'day_hours', 'temp_mean', 'temp_annual')
    assert dn.check_call({'t': shape, 'sw': shape}, H, sw_threshold=10.0)[4:7] == ('sw', None, 10.0)
    assert np.array_equal(dn.check_call({'t': shape}, H, half, None, offset)[5][1], noon)

    def bad(match, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            dn.check_call(**args)
    bad("unknown field 'rh'", shapes={'rh': shape})
    bad('at least one field', shapes={})
    bad(r'must have shape \(D \* H, R, W\)', shapes={'t': shape[1:]})
    bad('fields must share one shape', shapes={'t': shape, 'sw': (days * H, rows, cols + 1)})
    bad('steps_per_day must be between 1 and 48', steps_per_day=0)
    bad('steps_per_day must be between 1 and 48', steps_per_day=49)
    bad('steps_per_day must be an integer', steps_per_day=24.0)
    bad('multiple of steps_per_day', shapes={'t': (days * H + 1, rows, cols)})
    bad('at most 4096 days', shapes={'t': (4097, 1, 1)}, steps_per_day=1, half_day=np.zeros((4097, 1)),
        noon=None, offset=np.zeros(1))
    bad("mode must be 'solar' or 'sw'", mode='lunar')
    bad("needs half_day and offset", half_day=None)
    bad("needs half_day and offset", offset=None)
    bad(r'half_day must have shape \(2, 3\)', half_day=half[:1])
    bad(r'noon must have shape \(2,\)', noon=np.full(3, 12.0))
    bad(r'offset must have shape \(4,\)', offset=np.zeros(5))
    bad('half_day must lie between 0 and 12', half_day=half + 6.5)
    bad('half_day must lie between 0 and 12', half_day=half - 6.5)
    bad('noon must lie between 0 and 24', noon=noon + 12.5)
    bad('offset must lie between -12 and 12', offset=offset - 12.5)
    bad('half_day holds a value that is not finite', half_day=np.where(np.arange(rows) == 1, np.nan, half))
    bad('noon holds a value that is not finite', noon=np.array([12.0, np.inf]))
    bad('offset holds a value that is not finite', offset=np.array([0.0, np.nan, 0.0, 0.0]))
    bad("sw_threshold belongs to mode 'sw'", sw_threshold=5.0, mode='solar')
    bad("belong to mode 'solar'", sw_threshold=5.0)
    sw = dict(half_day=None, noon=None, offset=None)
    bad('sw_threshold must be finite', sw_threshold=np.inf, **sw)
    bad('sw_threshold must be finite', sw_threshold=np.nan, **sw)
    bad("needs sw_threshold", mode='sw', **sw)
    bad("needs the field 'sw'", shapes={'t': shape}, sw_threshold=5.0, outputs=('tmin',), **sw)
    bad("unknown name 'sw_rad_night'", outputs=('sw_rad_night',))
    bad("'vpd_day' needs the field 'qv'", outputs=('vpd_day',))
    bad('at least one output', outputs=())
    with pytest.raises(ValueError, match='all float32 or all float64'):
        dn.check_dtypes({'t': np.zeros(3, np.float32), 'sw': np.zeros(3)})
    with pytest.raises(ValueError, match='all float32 or all float64'):
        dn.check_dtypes({'t': np.zeros(3, np.int32)})
    with pytest.raises(ValueError, match="dtype must be 'float32' or 'float64'"):
        dn.check_out_dtype('uint8', np.float32)
    assert dn.check_out_dtype(None, np.float32) == np.float32 and dn.check_out_dtype(None, np.float64) == np.float64


def header_struct(name):
    """-> [(field name, ctypes type)] of a typedef struct of the header, in order"""
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, flags=re.S).group(1)
    types = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), types[ctype]) for n in names.split(',')]
    return fields


def test_prototypes_abi_version_and_spec_layout():
    from mod16_amd import _lib
    assert _lib.ABI_VERSION == 16
    text = open(HEADER).read()
    assert re.search(r'#define MOD16_ABI_VERSION 16\b', text) and 'added under ABI 16' in text
    for name in ('mod16_daynight_f32', 'mod16_daynight_f64'):
        assert re.search(r'MOD16_API int %s\(' % name, text)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == 11
        assert args[1] is ctypes.POINTER(_lib.DaynightSpec) and args[10] is ctypes.c_size_t
    fields = header_struct('mod16_daynight_spec')
    assert fields == list(_lib.DaynightSpec._fields_)

    class Twin(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(_lib.DaynightSpec) == ctypes.sizeof(Twin) == 72
    for (mode, code) in dn.MODES.items():
        assert re.search(r'MOD16_DAYNIGHT_%s = %d\b' % (mode.upper(), code), text)
    assert re.search(r'MOD16_DAYNIGHT_F32 = %d, MOD16_DAYNIGHT_F64 = %d\b' % (dn.OUT_TYPES['float32'], dn.OUT_TYPES['float64']), text)
    assert (_lib.DAYNIGHT_SOLAR, _lib.DAYNIGHT_SW, _lib.DAYNIGHT_F32, _lib.DAYNIGHT_F64) == (0, 1, 0, 1)
    assert callable(_lib.Context.daynight)
    lib = _lib.load()
    assert lib.mod16_version() == 16
    for name in ('mod16_daynight_f32', 'mod16_daynight_f64'):
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
        # a NULL context (and with it a NULL spec) is refused before anything is looked at
        assert getattr(lib, name)(None, None, None, None, None, None, None, None, 0, None, 0) == _lib.ERR_ARG


def test_numpy_entry_point_checks_then_needs_a_device():
    """Every bad argument is a ValueError with no device present; a good call then meets the library's
    "no CPU fallback" error (or, on a GPU box, runs and agrees with the definition)."""
    import mod16
    import mod16_amd
    from mod16_amd import _lib
    assert mod16.aggregate_daynight is mod16_amd.aggregate_daynight
    call = mod16_amd.aggregate_daynight
    days, H, rows, cols = 2, 4, 3, 5
    f = small_fields(days=days, H=H, rows=rows, cols=cols, dtype=np.float32)
    half, noon, offset = tables(days=days, rows=rows, cols=cols)
    with pytest.raises(ValueError, match='needs half_day and offset'):
        call(f, steps_per_day=H)
    with pytest.raises(ValueError, match='all float32 or all float64'):
        call(dict(f, t=f['t'].astype(np.float64)), half, noon, offset, steps_per_day=H)
    with pytest.raises(ValueError, match="dtype must be"):
        call(f, half, noon, offset, steps_per_day=H, dtype='int16')
    with pytest.raises(ValueError, match='stage_bytes'):
        call(f, half, noon, offset, steps_per_day=H, stage_bytes=-1)
    with pytest.raises(ValueError, match='out must hold exactly'):
        call(f, half, noon, offset, steps_per_day=H, out={'tmin': np.empty((days, rows, cols), np.float32)})
    with pytest.raises(ValueError, match=r"out\['tmin'\] must be a writeable C-contiguous float32 array"):
        call({'t': f['t']}, half, noon, offset, steps_per_day=H, outputs=('tmin',),
             out={'tmin': np.empty((days, rows, cols), np.float64)})
    if _lib.device_count() > 0:
        res, annual = call(f, half, noon, offset, steps_per_day=H)
        want, want_annual = dn.aggregate(f, H, half, noon, offset)
        assert res.tmin.dtype == np.float32 and np.array_equal(res.tmin, want.tmin)
        assert np.array_equal(annual, want_annual)
    else:
        with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
            call(f, half, noon, offset, steps_per_day=H)
