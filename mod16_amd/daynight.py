'''
Hourly reanalysis aggregated into the model's day / night drivers: the definition, in numpy, of what
``mod16_daynight_f32`` / ``mod16_daynight_f64`` compute (``RasterEngine.daynight``,
``mod16_amd.aggregate_daynight``), and the argument checks of those calls. Host only: nothing here
touches the library or a device; the kernel (``csrc/mod16_daynight.hpp``) follows ``day_weights``,
``split_field`` and ``aggregate`` operation for operation.

This day / night split is THIS PACKAGE's definition. It is not a transcription of the operational
MOD16 preprocessing: the reference package never performs this step (its loaders read ready-made
``*_daytime`` / ``*_nighttime`` datasets and take the day length from a sunrise / sunset package).

The coarse grid has ``R`` latitude rows and ``W`` longitude columns. Five fields are ``(D * H, R, W)``
series, all float32 or all float64: ``t`` (air temperature, K), ``qv`` (specific humidity), ``ps``
(surface pressure, Pa), ``sw`` (downward short-wave radiation) and ``lw`` (net long-wave radiation).
``H`` (1 ... 48) is the number of steps per day, ``D`` (1 ... 4096) the number of days; step ``s = d H +
k`` covers the UTC hours ``[k delta, (k + 1) delta)`` of day ``d``, ``delta = 24 / H``. NaN is the
missing value (mapping a product's fill value to NaN is the caller's job).

Every step of every cell gets a day weight ``w`` in [0, 1] (``day_weights``):

``'solar'``  from three float64 tables made on the host (``solar_tables``, or the caller's own, e.g.
             from a sunrise / sunset package): ``half_day[D, R]`` (half the day length in hours, 0 ...
             12; 0 is polar night, 12 polar day), ``noon[D]`` (local solar noon in hours, 0 ... 24;
             default 12) and ``offset[W]`` (longitude / 15 in hours, -12 ... 12). With ``a = ((noon -
             half_day) - offset) / delta`` and ``b = ((noon + half_day) - offset) / delta`` (sunrise and
             sunset in UTC steps), ``w = min(sum over m in (-H, 0, +H) of max(min(k + 1, b + m) - max(k,
             a + m), 0), 1)``, the three terms added in that order: the three windows cover every
             longitude's wrap of the local day across the UTC day. All transcendental work is in the
             tables; the device multiplies, adds, divides and takes min / max only.
``'sw'``     from the data: 1.0 where ``sw > threshold``, else 0.0; NaN where ``sw`` is NaN.

Per day and cell, in float64, sums sequential in ``k`` from 0.0, every product rounded before it is
added (``split_field``): ``sum_w = sum w``, ``sum_n = sum (1 - w)``, ``day_hours = delta sum_w``, and per
field ``mean = (sum X) / H``, ``day = (sum w X) / sum_w`` where ``sum_w > 0`` else ``mean``, ``night =
(sum (1 - w) X) / sum_n`` where ``sum_n > 0`` else ``mean`` (the fallback keeps polar night and polar
day finite: the value is multiplied by zero hours downstream, but a NaN there would invalidate the
day in a composite; at polar day the two pieces of the step that holds sunrise may add up to 1 - 1
ulp where sunrise is no whole step: ``sum_n`` is then a few 1e-16, not 0, and the night value that
step's, finite either way and weighted with ``24 - day_hours`` of about 1e-14 hours downstream).
``tmin`` is the minimum of ``t`` over the steps, NaN if any step is NaN.
``vpd_day`` is the VPD of ``MOD16.vpd`` on ``(qv_day, ps_day, t_day)``, ``vpd_night`` the same of the night
values with negative values set to 0 -- aggregate first, VPD after, as the reference's loader and
``evapotranspiration_raw`` do. ``temp_annual`` is ``(sum over d of temp_mean[d]) / D``, sequential in
``d``, on the float64 means: the reference's "overall mean" as one plane. Outputs are float32 or
float64, each value rounded once.

``sw_rad_night`` is deliberately not produced: callers pass 0.0, as the reference's loader does.
'''
import collections

import numpy as np

#: the hourly fields in argument order
FIELD_NAMES = ('t', 'qv', 'ps', 'sw', 'lw')
#: the day / night series, in the order of the C ABI's output array
OUTPUT_NAMES = ('lw_net_day', 'lw_net_night', 'sw_rad_day', 'temp_day', 'temp_night', 'tmin', 'vpd_day',
                'vpd_night', 'day_hours', 'temp_mean')
#: ... and the fields each of them is made from (``'sw'`` mode adds ``sw`` to every one of them)
NEEDS = {'lw_net_day': ('lw',), 'lw_net_night': ('lw',), 'sw_rad_day': ('sw',), 'temp_day': ('t',),
         'temp_night': ('t',), 'tmin': ('t',), 'vpd_day': ('t', 'qv', 'ps'), 'vpd_night': ('t', 'qv', 'ps'),
         'day_hours': (), 'temp_mean': ('t',), 'temp_annual': ('t',)}
DayNight = collections.namedtuple('DayNight', OUTPUT_NAMES)
MODES = {'solar': 0, 'sw': 1}                      # enum mod16_daynight_mode
OUT_TYPES = {'float32': 0, 'float64': 1}           # enum mod16_daynight_out
MAX_STEPS = 48
MAX_DAYS = 4096
MAX_EXTENT = 2 ** 30


def _as_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (what, value))
    return int(value)


def _table(values, shape, lo, hi, what):
    t = np.asarray(values, np.float64)
    if t.shape != shape:
        raise ValueError('%s must have shape %r, got %r' % (what, shape, t.shape))
    if not np.all(np.isfinite(t)):
        raise ValueError('%s holds a value that is not finite' % what)
    if t.size and (t.min() < lo or t.max() > hi):
        raise ValueError('%s must lie between %g and %g' % (what, lo, hi))
    return np.ascontiguousarray(t)


def check_outputs(outputs, given, mode):
    '''``outputs`` (None: every output all of whose fields are in ``given``) -> the requested names, in
    the order of ``OUTPUT_NAMES`` with ``'temp_annual'`` last; ValueError for an unknown name or one
    whose field is missing.'''
    extra = ('sw',) if mode == 'sw' else ()
    every = OUTPUT_NAMES + ('temp_annual',)
    if outputs is None:
        return tuple(n for n in every if all(f in given for f in NEEDS[n] + extra))
    if isinstance(outputs, str):
        outputs = (outputs,)
    names = tuple(outputs)
    for n in names:
        if n not in every:
            raise ValueError('outputs: unknown name %r (one of %s)' % (n, ', '.join(every)))
        for f in NEEDS[n] + extra:
            if f not in given:
                raise ValueError("outputs: %r needs the field '%s'" % (n, f))
    if not names:
        raise ValueError('outputs must name at least one output')
    return tuple(n for n in every if n in names)


def output_table(names, D, R, W, dtype):
    '''What a call produces, in the order of ``names`` (that of ``check_outputs``): name -> ``(shape, numpy
    dtype)``, ``(D, R, W)`` series and the ``(R, W)`` plane ``'temp_annual'``, all in the output ``dtype``.'''
    return {n: ((R, W) if n == 'temp_annual' else (D, R, W), np.dtype(dtype)) for n in names}


def check_call(shapes, steps_per_day=24, half_day=None, noon=None, offset=None, sw_threshold=None,
               outputs=None, mode=None):
    '''The argument checks of every day / night call. ``shapes``: field name -> shape of the fields
    given, each ``(D * H, R, W)``; ``mode``: ``'solar'``, ``'sw'`` or None (``'sw'`` if ``sw_threshold``
    is given, else ``'solar'``).

    Returns ``(D, H, R, W, mode, (half_day, noon, offset) as contiguous float64 tables or None,
    threshold, requested output names)``; ValueError otherwise, with a message naming the argument.'''
    shapes = {k: tuple(v) for k, v in dict(shapes).items()}
    for k in shapes:
        if k not in FIELD_NAMES:
            raise ValueError('fields: unknown field %r (one of %s)' % (k, ', '.join(FIELD_NAMES)))
    if not shapes:
        raise ValueError('fields must hold at least one field')
    if mode is None:
        mode = 'sw' if sw_threshold is not None else 'solar'
    if mode not in MODES:
        raise ValueError("mode must be 'solar' or 'sw', got %r" % (mode,))
    H = _as_int(steps_per_day, 'steps_per_day')
    if not 1 <= H <= MAX_STEPS:
        raise ValueError('steps_per_day must be between 1 and %d, got %d' % (MAX_STEPS, H))
    first = next(iter(shapes.values()))
    for k, s in shapes.items():
        if len(s) != 3:
            raise ValueError("fields['%s'] must have shape (D * H, R, W), got %r" % (k, s))
        if s != first:
            raise ValueError('fields must share one shape, got %r and %r' % (first, s))
    steps, R, W = first
    if steps % H != 0 or steps < H:
        raise ValueError('fields: the time axis (%d) must be a multiple of steps_per_day (%d), at least one day'
                         % (steps, H))
    D = steps // H
    if D > MAX_DAYS:
        raise ValueError('fields: at most %d days, got %d' % (MAX_DAYS, D))
    if R > MAX_EXTENT or W > MAX_EXTENT:
        raise ValueError('fields: rows and columns must not exceed 2^30')
    tables, threshold = None, 0.0
    if mode == 'solar':
        if sw_threshold is not None:
            raise ValueError("sw_threshold belongs to mode 'sw'")
        if half_day is None or offset is None:
            raise ValueError("mode 'solar' needs half_day and offset (mod16_amd.daynight.solar_tables)")
        tables = (_table(half_day, (D, R), 0.0, 12.0, 'half_day'),
                  _table(np.full(D, 12.0) if noon is None else noon, (D,), 0.0, 24.0, 'noon'),
                  _table(offset, (W,), -12.0, 12.0, 'offset'))
    else:
        if half_day is not None or noon is not None or offset is not None:
            raise ValueError("half_day, noon and offset belong to mode 'solar'")
        if sw_threshold is None or isinstance(sw_threshold, (bool, np.bool_)) or np.ndim(sw_threshold) != 0:
            raise ValueError("mode 'sw' needs sw_threshold, one number")
        threshold = float(sw_threshold)
        if not np.isfinite(threshold):
            raise ValueError('sw_threshold must be finite, got %r' % (sw_threshold,))
    names = check_outputs(outputs, tuple(shapes), mode)
    return D, H, R, W, mode, tables, threshold, names


def solar_tables(day_of_year, lat, lon):
    '''The three tables of ``'solar'`` mode on the host -> ``(half_day[D, R], noon[D], offset[W])``.

    ``day_of_year[D]``: 1 ... 366; ``lat[R]`` and ``lon[W]``: cell centres in degrees (-90 ... 90, -180
    ... 180). Declination by Cooper (1969): ``delta = 23.45 deg sin(2 pi (284 + n) / 365)``; ``half_day =
    arccos(clip(-tan(lat) tan(delta), -1, 1)) 12 / pi``; ``noon`` is 12 everywhere (no equation of
    time); ``offset = lon / 15``.'''
    n = np.atleast_1d(np.asarray(day_of_year, np.float64))
    lat = np.atleast_1d(np.asarray(lat, np.float64))
    lon = np.atleast_1d(np.asarray(lon, np.float64))
    if n.ndim != 1 or lat.ndim != 1 or lon.ndim != 1:
        raise ValueError('day_of_year, lat and lon must be vectors')
    if not (np.all(np.isfinite(lat)) and np.all(np.abs(lat) <= 90)):
        raise ValueError('lat must lie between -90 and 90')
    if not (np.all(np.isfinite(lon)) and np.all(np.abs(lon) <= 180)):
        raise ValueError('lon must lie between -180 and 180')
    if not np.all(np.isfinite(n)):
        raise ValueError('day_of_year must be finite')
    decl = np.deg2rad(23.45) * np.sin(2.0 * np.pi * (284.0 + n) / 365.0)
    with np.errstate(all='ignore'):
        x = -np.tan(np.deg2rad(lat))[None, :] * np.tan(decl)[:, None]
    half_day = np.arccos(np.clip(x, -1.0, 1.0)) * 12.0 / np.pi
    return np.clip(half_day, 0.0, 12.0), np.full(n.shape, 12.0), lon / 15.0


def day_weights(steps_per_day, half_day, noon, offset):
    '''``'solar'`` mode's weights -> ``(D, H, R, W)`` float64 (see the module text).'''
    H = int(steps_per_day)
    half_day = np.asarray(half_day, np.float64)[:, None, :, None]
    noon = np.asarray(noon, np.float64)[:, None, None, None]
    offset = np.asarray(offset, np.float64)[None, None, None, :]
    delta = np.float64(24.0) / np.float64(H)
    a = ((noon - half_day) - offset) / delta
    b = ((noon + half_day) - offset) / delta
    k = np.arange(H, dtype=np.float64)[None, :, None, None]
    total = None
    for m in (-np.float64(H), np.float64(0.0), np.float64(H)):
        term = np.maximum(np.minimum(k + 1.0, b + m) - np.maximum(k, a + m), 0.0)
        total = term if total is None else total + term
    return np.minimum(total, 1.0)


def sw_weights(sw, steps_per_day, threshold):
    '''``'sw'`` mode's weights -> ``(D, H, R, W)`` float64: 1.0 where ``sw > threshold``, else 0.0, NaN
    where ``sw`` is NaN.'''
    sw = np.asarray(sw)
    x = sw.astype(np.float64).reshape((-1, int(steps_per_day)) + sw.shape[1:])
    with np.errstate(invalid='ignore'):
        w = np.where(x > np.float64(threshold), 1.0, 0.0)
    return np.where(np.isnan(x), np.nan, w)


def split_weights(w):
    '''``(sum_w, sum_n)`` of ``(D, H, R, W)`` weights, sequential in the step.'''
    sum_w = np.zeros(w.shape[:1] + w.shape[2:], np.float64)
    sum_n = np.zeros_like(sum_w)
    for k in range(w.shape[1]):
        sum_w = sum_w + w[:, k]
        sum_n = sum_n + (1.0 - w[:, k])
    return sum_w, sum_n


def split_field(x, w):
    '''One field's ``(day, night, mean)`` as ``(D, R, W)`` float64 planes from its ``(D * H, R, W)``
    series and the ``(D, H, R, W)`` weights (broadcastable ones are fine).'''
    x = np.asarray(x)
    H = w.shape[1]
    x = x.astype(np.float64).reshape((-1, H) + x.shape[1:])
    w = np.broadcast_to(w, x.shape)
    sum_w, sum_n = split_weights(w)
    sx = np.zeros_like(sum_w)
    swx = np.zeros_like(sum_w)
    snx = np.zeros_like(sum_w)
    with np.errstate(all='ignore'):
        for k in range(H):
            sx = sx + x[:, k]
            swx = swx + w[:, k] * x[:, k]
            snx = snx + (1.0 - w[:, k]) * x[:, k]
        mean = sx / np.float64(H)
        day = np.where(sum_w > 0, swx / sum_w, mean)
        night = np.where(sum_n > 0, snx / sum_n, mean)
    return day, night, mean


def vpd(qv, ps, t):
    '''``MOD16.vpd`` in numpy (its own SVP constants), operation for operation.'''
    with np.errstate(all='ignore'):
        tc = t - 273.15
        avp = (qv * ps) / (0.622 + (0.379 * qv))
        sv = 610.7 * np.exp((17.38 * tc) / (239 + tc))
        return sv - avp


def aggregate(fields, steps_per_day=24, half_day=None, noon=None, offset=None, sw_threshold=None,
              outputs=None, dtype=None, mode=None):
    '''The definition. ``fields``: a dict of the hourly series by name (``FIELD_NAMES``), all float32
    or all float64; tables, threshold, ``outputs`` and ``mode`` as ``check_call`` takes them;
    ``dtype``: ``'float32'`` or ``'float64'`` (default: float32 only if the fields are float32).

    Returns ``(DayNight, temp_annual)``: ``(D, R, W)`` series and one ``(R, W)`` plane, None where an
    output was not requested. ``sw_rad_night`` is not produced (pass 0.0, as the reference's loader
    does).'''
    fields = {k: np.asarray(v) for k, v in dict(fields).items() if v is not None}
    D, H, R, W, mode, tables, threshold, names = check_call(
        {k: v.shape for k, v in fields.items()}, steps_per_day, half_day, noon, offset, sw_threshold, outputs, mode)
    in_dtype = check_dtypes(fields)
    out_dtype = check_out_dtype(dtype, in_dtype)
    if mode == 'solar':
        w = np.broadcast_to(day_weights(H, *tables), (D, H, R, W))
    else:
        w = sw_weights(fields['sw'], H, threshold)
    sum_w, _ = split_weights(w)
    want = set(names)
    res = dict.fromkeys(OUTPUT_NAMES)
    res['day_hours'] = (np.float64(24.0) / np.float64(H)) * sum_w
    parts = {}
    for f in FIELD_NAMES:
        if f in fields and any(f in NEEDS[n] for n in want):
            parts[f] = split_field(fields[f], w)
    if 'lw' in parts:
        res['lw_net_day'], res['lw_net_night'] = parts['lw'][0], parts['lw'][1]
    if 'sw' in parts:
        res['sw_rad_day'] = parts['sw'][0]
    annual = None
    if 't' in parts:
        res['temp_day'], res['temp_night'], res['temp_mean'] = parts['t']
        x = fields['t'].astype(np.float64).reshape(D, H, R, W)
        res['tmin'] = np.min(x, axis=1)
        annual = np.zeros((R, W), np.float64)
        for d in range(D):
            annual = annual + res['temp_mean'][d]
        annual = annual / np.float64(D)
    if 'qv' in parts and 'ps' in parts and 't' in parts:
        res['vpd_day'] = vpd(parts['qv'][0], parts['ps'][0], parts['t'][0])
        v = vpd(parts['qv'][1], parts['ps'][1], parts['t'][1])
        with np.errstate(invalid='ignore'):
            res['vpd_night'] = np.where(v < 0, 0.0, v)
    out = DayNight(*[res[n].astype(out_dtype) if n in want else None for n in OUTPUT_NAMES])
    return out, (annual.astype(out_dtype) if 'temp_annual' in want else None)


def check_dtypes(fields):
    '''The common dtype of the fields given (a dict of arrays): float32 or float64, else ValueError.'''
    kinds = set(np.dtype(v.dtype).name for v in fields.values())
    if len(kinds) != 1 or not kinds <= {'float32', 'float64'}:
        raise ValueError('fields must be all float32 or all float64, got %s' % ', '.join(sorted(kinds)))
    return np.dtype(kinds.pop())


def check_out_dtype(dtype, in_dtype):
    '''``dtype`` (None: float32 only if the inputs are float32) -> a numpy dtype; ValueError otherwise.'''
    if dtype is None:
        return np.dtype(in_dtype)
    try:
        name = np.dtype(dtype).name
    except TypeError:
        name = None
    if name not in OUT_TYPES:
        raise ValueError("dtype must be 'float32' or 'float64', got %r" % (dtype,))
    return np.dtype(name)
