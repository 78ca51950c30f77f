"""What the device-tensor entry points refuse, and that they take pitched, offset views: one table
over every tensor-taking method of mod16_amd.raster -- RasterEngine.composite, .gapfill, .daynight,
.trend, .anomaly, .zonal, .zonal_bounds, DownscaleGrid.run, .fields, .composite and UpscaleGrid.run,
.majority.

A refusal case starts from a call that is accepted, commits ONE offence against one argument and
asserts the exception type, that the message names the argument, and the phrase that names the
condition ('unit stride', 'distance between rows', 'stride in time', 'must share one', 'tensor on
cuda:', 'shape', 'overlaps'; a few conditions outside the strided layouts have a phrase of their
own: a flat array that must be 'contiguous', a wrong count of outputs that 'must hold' another, a
dict of outputs that must hold 'exactly the fields' produced or 'exactly the requested' outputs).
Every refusal comes before any device work. An accepted call per method runs on views that start one
element into a larger buffer with rows (and planes) further apart than they are long, and must equal
the call on contiguous copies bit for bit: a helper that reported a wrong pitch would show there.

Shapes, the smallest with every edge: n = 7 pixels; gap filling S = 3 slabs; day / night 3 x 5 cells,
D = 2 days of H = 2 steps; zonal K = 2 layers, 3 zones; a 5 x 6 fine raster over a 3 x 4 coarse grid,
of which the calls take the 7 pixels from pixel 11; composites of 4 days in periods of 2; a trend over
Y = 4 steps with min_valid = 2 and alpha = 0.1 (all seven fields); anomalies of 3 years of 2 periods
with window = 2, min_valid = 2 and a denominator (all five outputs); upscaling of K = 2 layers of the
5 x 6 raster onto the 3 x 4 grid (all three outputs) and its class raster (both outputs). A `(Y, n - 1)`
stack is just another trend or anomaly call, so `wrong_shape` is no offence against `values` / `num`."""
import numpy as np
import pytest

from oracle import synth

pytestmark = pytest.mark.gpu

N, S = 7, 3
R, W, D, H = 3, 5, 2, 2
K, NZ = 2, 3
FINE, COARSE, FIRST = (5, 6), (3, 4), 11
DAYS, PERIOD = 4, 2
COARSE_DRIVERS = ('temp_day', 'temp_night', 'temp_annual')       # drivers 5, 6 and 7
STEPS, YEARS, PERIODS = 4, 3, 2
TREND_FIELDS = ('slope', 'intercept', 'slope_lo', 'slope_hi', 's', 'z', 'count')
ANOMALY_FIELDS = ('z', 'pct', 'mean', 'std', 'count')
UPSCALE_FIELDS = ('mean', 'fraction', 'count')
CLASS_FIELDS = ('cls', 'share')


@pytest.fixture(scope='module')
def env():
    """(torch, engine, grid, the accepted arguments of every method as contiguous device tensors)"""
    import torch
    from mod16_amd import daynight as dn, downscale as ds
    from mod16_amd.models import COLLECTION61_BPLUT
    from mod16_amd.raster import RasterEngine
    from mod16_amd.utils import restore_bplut, bplut_table
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    grid = eng.downscale_grid(FINE, COARSE, ds.positions(0.1, 0.4, FINE[0], 0.0, 1.0),
                              ds.positions(0.2, 0.5, FINE[1], 0.0, 1.0))
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cls, daily = synth.drivers((DAYS, N), seed=3, special=False)
    _, coarse = synth.drivers((DAYS,) + COARSE, seed=4, special=False)
    base = {}
    # composite: daily (4, n) arrays, a scalar, an (n,) array; hours (4, n)
    drivers = [dev(a) for a in daily]
    drivers[3] = 0.0
    drivers[7] = dev(daily[7][0])
    base['composite'] = dict(cls=dev(cls[0]), drivers=drivers, day_hours=dev(rng.uniform(6, 18, (DAYS, N))), out=None)
    # composite over coarse arrays: two (4, 3, 4) series and one (3, 4) plane
    cdrivers = list(drivers)
    cdrivers[5], cdrivers[6], cdrivers[7] = dev(coarse[5]), dev(coarse[6]), dev(coarse[7][0])
    base['grid.composite'] = dict(cls=dev(cls[0]), drivers=cdrivers, day_hours=base['composite']['day_hours'], out=None)
    # downscaled run: three coarse planes, fine arrays, a scalar
    rdrivers = [dev(a[0]) for a in daily]
    rdrivers[3] = 0.0
    rdrivers[5], rdrivers[6], rdrivers[7] = dev(coarse[5][0]), dev(coarse[6][0]), dev(coarse[7][0])
    base['grid.run'] = dict(cls=dev(cls[0]), drivers=rdrivers, out_day=None, out_night=None)
    base['grid.fields'] = dict(fields=[dev(coarse[5][0]), dev(coarse[6][1])], out=None)
    # gap filling: two (3, n) series, QC, fallbacks
    base['gapfill'] = dict(fields=[dev(rng.integers(0, 101, (S, N), dtype=np.uint8)) for _ in range(2)],
                           qc=dev(rng.choice(np.array([0, 0, 8, 157], np.uint8), (S, N))),
                           fallback=[dev(rng.integers(0, 101, N, dtype=np.uint8)) for _ in range(2)],
                           source=False, out=None)
    # day / night: t and sw, (D H, R, W); solar tables
    lat = np.linspace(60.0, -60.0, R)
    half, noon, offset = dn.solar_tables(np.arange(1, D + 1), lat, np.linspace(-150.0, 150.0, W))
    base['daynight'] = dict(fields={'t': dev(rng.uniform(260.0, 300.0, (D * H, R, W))),
                                    'sw': dev(rng.uniform(0.0, 800.0, (D * H, R, W)))},
                            tables=(half, noon, offset), out=None)
    # zonal: (K, n) values, zone ids, per-pixel weights
    base['zonal'] = dict(values=dev(rng.uniform(-3.0, 9.0, (K, N))), zones=dev(rng.integers(0, NZ, N).astype(np.int32)),
                         area=dev(rng.uniform(0.5, 2.0, N)), cols=None, acc=None)
    base['zonal_bounds'] = dict(values=base['zonal']['values'], area=base['zonal']['area'], cols=None)
    # trend: a (Y, n) stack; anomaly: (Y P, n) numerator and denominator
    base['trend'] = dict(values=dev(rng.uniform(0.0, 9.0, (STEPS, N))), out=None)
    base['anomaly'] = dict(num=dev(rng.uniform(1.0, 9.0, (YEARS * PERIODS, N))),
                           den=dev(rng.uniform(1.0, 9.0, (YEARS * PERIODS, N))), out=None)
    # upscaling: the downscaled grid's geometry the other way round; (K, 5, 6) values, a (5, 6) class raster
    up = eng.upscale_grid(FINE, COARSE, ds.positions(0.1, 0.4, FINE[0], 0.0, 1.0),
                          ds.positions(0.2, 0.5, FINE[1], 0.0, 1.0))
    base['upscale.run'] = dict(grid=up, values=dev(rng.uniform(0.0, 9.0, (K,) + FINE)), out=None)
    base['upscale.majority'] = dict(grid=up, cls=dev(rng.integers(0, 13, FINE).astype(np.uint8)), out=None)
    yield torch, eng, grid, base
    up.close()
    grid.close()


def call(env, method, a):
    """The call of `method` with the arguments `a` (a copy of its entry of the fixture, changed by the case)."""
    torch, eng, grid, _ = env
    if method == 'composite':
        return eng.composite(a['cls'], a['drivers'], a['day_hours'], DAYS, PERIOD, pet=a.get('pet', False), out=a['out'])
    if method == 'grid.composite':
        return grid.composite(a['cls'], a['drivers'], a['day_hours'], DAYS, PERIOD, coarse=COARSE_DRIVERS,
                              first_pixel=FIRST, out=a['out'])
    if method == 'grid.run':
        return grid.run(a['cls'], a['drivers'], coarse=COARSE_DRIVERS, first_pixel=FIRST, out_day=a['out_day'],
                        out_night=a['out_night'])
    if method == 'grid.fields':
        return grid.fields(a['fields'], first_pixel=FIRST, n=N, out=a['out'])
    if method == 'gapfill':
        return eng.gapfill(tuple(a['fields']), qc=a['qc'], max_gap=1, fallback=a['fallback'], source=a['source'], out=a['out'])
    if method == 'daynight':
        return eng.daynight(a['fields'], *a['tables'], steps_per_day=H, outputs=('temp_day', 'sw_rad_day', 'temp_annual'),
                            out=a['out'])
    if method == 'trend':
        return eng.trend(a['values'], min_valid=2, alpha=0.1, out=a['out'])
    if method == 'anomaly':
        return eng.anomaly(a['num'], a['den'], periods=PERIODS, window=2, min_valid=2, outputs=ANOMALY_FIELDS,
                           out=a['out'])
    if method == 'upscale.run':
        return a['grid'].run(a['values'], outputs=UPSCALE_FIELDS, out=a['out'])
    if method == 'upscale.majority':
        return a['grid'].majority(a['cls'], outputs=CLASS_FIELDS, out=a['out'])
    if method == 'zonal':
        return eng.zonal(a['values'], a['zones'], NZ, area=a['area'], cols=a['cols'], bounds=(2.0, 9.0), acc=a['acc'])
    return eng.zonal_bounds(a['values'], a['area'], a['cols'])


# ------------------------------------------------------------ offences
def full(torch, shape, dtype, fill=0):
    """(uint16 tensors are made, copied and compared as int16: the counts of a composite)"""
    if dtype == torch.uint16:
        return torch.full(shape, fill, dtype=torch.int16, device='cuda').view(dtype)
    return torch.full(shape, fill, dtype=dtype, device='cuda')


def signed(torch, t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def not_a_tensor(torch, t):
    return signed(torch, t).cpu().numpy()


def wrong_dtype(torch, t):
    return signed(torch, t).to(torch.int64 if t.dtype == torch.uint16 else torch.int16)


def wrong_shape(torch, t):
    return full(torch, tuple(t.shape[:-1]) + (t.shape[-1] - 1,), t.dtype)


def non_unit(torch, t):
    """t's shape with stride 2 in the last dimension"""
    return full(torch, tuple(t.shape[:-1]) + (2 * t.shape[-1],), t.dtype)[..., ::2]


def rows_too_close(torch, t):
    """t's shape with rows one element less than a row apart"""
    strides = list(t.contiguous().stride())
    strides[-2] = t.shape[-1] - 1
    return full(torch, (t.numel() + 8,), t.dtype).as_strided(tuple(t.shape), strides)


def planes_too_close(torch, t):
    """t's shape with planes (or time slabs) one element less than a plane apart"""
    strides = list(t.contiguous().stride())
    strides[0] -= 1
    return full(torch, (t.numel() + 8,), t.dtype).as_strided(tuple(t.shape), strides)


def pitched(torch, t, fill=0):
    """t's values in a view one element into a larger buffer: rows 3 elements further apart than
    they are long, one row more than t has between two planes"""
    if t.dim() == 1:
        view = full(torch, (t.numel() + 2,), t.dtype, fill)[1:-1]
    else:
        view = full(torch, tuple(t.shape[:-2]) + (t.shape[-2] + 1, t.shape[-1] + 3), t.dtype, fill)[..., :-1, 1:-2]
    signed(torch, view).copy_(signed(torch, t))
    return view


def outputs_of(torch, env, method, a):
    """the tensors an accepted call returns, as a flat list"""
    res = call(env, method, a)
    env[1].check()
    flat = []
    for x in (res if isinstance(res, (tuple, list)) else [res]):
        flat.extend(x if isinstance(x, (tuple, list)) else [x])
    return [x for x in flat if x is not None]


def put(a, path, value):
    """a copy of the arguments `a` with the entry at `path` (a key, or a key and an index or name) replaced"""
    a = dict(a)
    if len(path) == 1:
        a[path[0]] = value
    else:
        box = a[path[0]]
        box = dict(box) if isinstance(box, dict) else list(box)
        box[path[1]] = value
        a[path[0]] = box
    return a


def get(a, path):
    return a[path[0]] if len(path) == 1 else a[path[0]][path[1]]


#: (method, path of the argument, offence, exception, name in the message, phrase)
ONE_ARGUMENT = [
    # ---- RasterEngine.composite: inputs
    ('composite', ('cls',), wrong_dtype, TypeError, 'cls', 'tensor on cuda:'),
    ('composite', ('drivers', 0), wrong_dtype, TypeError, 'lw_net_day', 'tensor on cuda:'),
    ('composite', ('drivers', 0), wrong_shape, ValueError, 'lw_net_day', '(S, n) tensor'),
    ('composite', ('drivers', 0), non_unit, ValueError, 'lw_net_day', 'unit stride'),
    ('composite', ('drivers', 0), planes_too_close, ValueError, 'lw_net_day', 'stride in time'),
    ('composite', ('drivers', 7), wrong_dtype, TypeError, 'temp_annual', 'tensor on cuda:'),
    ('composite', ('drivers', 7), non_unit, ValueError, 'temp_annual', 'unit stride'),
    ('composite', ('day_hours',), wrong_dtype, TypeError, 'day_hours', 'tensor on cuda:'),
    ('composite', ('day_hours',), planes_too_close, ValueError, 'day_hours', 'stride in time'),
    # ---- DownscaleGrid.composite: coarse and fine inputs
    ('grid.composite', ('drivers', 5), not_a_tensor, ValueError, 'temp_day', 'shape'),
    ('grid.composite', ('drivers', 5), wrong_dtype, TypeError, 'temp_day', 'tensor on cuda:'),
    ('grid.composite', ('drivers', 5), wrong_shape, ValueError, 'temp_day', 'shape'),
    ('grid.composite', ('drivers', 5), non_unit, ValueError, 'temp_day', 'unit stride'),
    ('grid.composite', ('drivers', 5), rows_too_close, ValueError, 'temp_day', 'distance between rows'),
    ('grid.composite', ('drivers', 5), planes_too_close, ValueError, 'temp_day', 'stride in time'),
    ('grid.composite', ('drivers', 5), pitched, ValueError, 'coarse arrays', 'must share one'),
    ('grid.composite', ('drivers', 7), wrong_dtype, TypeError, 'temp_annual', 'tensor on cuda:'),
    ('grid.composite', ('drivers', 7), non_unit, ValueError, 'temp_annual', 'unit stride'),
    ('grid.composite', ('drivers', 7), rows_too_close, ValueError, 'temp_annual', 'distance between rows'),
    ('grid.composite', ('drivers', 0), wrong_dtype, TypeError, 'lw_net_day', 'tensor on cuda:'),
    ('grid.composite', ('drivers', 0), non_unit, ValueError, 'lw_net_day', 'unit stride'),
    ('grid.composite', ('drivers', 0), planes_too_close, ValueError, 'lw_net_day', 'stride in time'),
    ('grid.composite', ('cls',), wrong_dtype, TypeError, 'cls', 'tensor on cuda:'),
    # ---- DownscaleGrid.run
    ('grid.run', ('drivers', 5), not_a_tensor, ValueError, 'temp_day', 'shape'),
    ('grid.run', ('drivers', 5), wrong_dtype, TypeError, 'temp_day', 'tensor on cuda:'),
    ('grid.run', ('drivers', 5), wrong_shape, ValueError, 'temp_day', 'shape'),
    ('grid.run', ('drivers', 5), non_unit, ValueError, 'temp_day', 'unit stride'),
    ('grid.run', ('drivers', 5), rows_too_close, ValueError, 'temp_day', 'distance between rows'),
    ('grid.run', ('drivers', 5), pitched, ValueError, 'coarse drivers', 'must share one'),
    ('grid.run', ('drivers', 0), wrong_dtype, TypeError, 'lw_net_day', 'tensor on cuda:'),
    ('grid.run', ('drivers', 0), wrong_shape, ValueError, 'lw_net_day', 'shape'),
    ('grid.run', ('drivers', 0), non_unit, TypeError, 'lw_net_day', 'contiguous'),
    ('grid.run', ('cls',), wrong_dtype, TypeError, 'cls', 'tensor on cuda:'),
    # ---- DownscaleGrid.fields
    ('grid.fields', ('fields', 1), not_a_tensor, TypeError, 'field 1', 'tensor on cuda:'),
    ('grid.fields', ('fields', 1), wrong_dtype, TypeError, 'field 1', 'tensor on cuda:'),
    ('grid.fields', ('fields', 1), wrong_shape, ValueError, 'field 1', 'shape'),
    ('grid.fields', ('fields', 1), non_unit, ValueError, 'field 1', 'unit stride'),
    ('grid.fields', ('fields', 1), rows_too_close, ValueError, 'field 1', 'distance between rows'),
    ('grid.fields', ('fields', 1), pitched, ValueError, 'coarse fields', 'must share one'),
    # ---- RasterEngine.gapfill: inputs and optional inputs
    ('gapfill', ('fields', 1), not_a_tensor, TypeError, 'fields[1]', 'tensor on cuda:'),
    ('gapfill', ('fields', 1), wrong_dtype, TypeError, 'fields[1]', 'tensor on cuda:'),
    ('gapfill', ('fields', 1), wrong_shape, ValueError, 'fields', 'shape'),
    ('gapfill', ('fields', 1), non_unit, ValueError, 'fields[1]', 'unit stride'),
    ('gapfill', ('fields', 1), rows_too_close, ValueError, 'fields[1]', 'stride in time'),
    ('gapfill', ('fields', 1), pitched, ValueError, 'fields', 'must share one'),
    ('gapfill', ('qc',), not_a_tensor, TypeError, 'qc', 'tensor on cuda:'),
    ('gapfill', ('qc',), wrong_dtype, TypeError, 'qc', 'tensor on cuda:'),
    ('gapfill', ('qc',), wrong_shape, ValueError, 'qc', 'shape'),
    ('gapfill', ('qc',), non_unit, ValueError, 'qc', 'unit stride'),
    ('gapfill', ('qc',), rows_too_close, ValueError, 'qc', 'stride in time'),
    ('gapfill', ('fallback', 0), not_a_tensor, TypeError, 'fallback[0]', 'tensor on cuda:'),
    ('gapfill', ('fallback', 0), wrong_dtype, TypeError, 'fallback[0]', 'tensor on cuda:'),
    ('gapfill', ('fallback', 0), wrong_shape, ValueError, 'fallback', 'shape'),
    ('gapfill', ('fallback', 0), non_unit, ValueError, 'fallback[0]', 'unit stride'),
    # ---- RasterEngine.daynight: inputs
    ('daynight', ('fields', 'sw'), not_a_tensor, TypeError, "fields['sw']", 'tensor on cuda:'),
    ('daynight', ('fields', 'sw'), wrong_dtype, TypeError, "fields['sw']", 'tensor on cuda:'),
    ('daynight', ('fields', 'sw'), wrong_shape, ValueError, 'fields', 'shape'),
    ('daynight', ('fields', 'sw'), non_unit, ValueError, "fields['sw']", 'unit stride'),
    ('daynight', ('fields', 'sw'), rows_too_close, ValueError, "fields['sw']", 'distance between rows'),
    ('daynight', ('fields', 'sw'), planes_too_close, ValueError, "fields['sw']", 'stride in time'),
    ('daynight', ('fields', 'sw'), pitched, ValueError, 'fields', 'must share one'),
    # ---- RasterEngine.zonal and .zonal_bounds: inputs and optional inputs
    ('zonal', ('values',), not_a_tensor, TypeError, 'values', 'tensor on cuda:'),
    ('zonal', ('values',), wrong_dtype, TypeError, 'values', 'tensor on cuda:'),
    ('zonal', ('values',), non_unit, ValueError, 'values', 'unit stride'),
    ('zonal', ('values',), rows_too_close, ValueError, 'values', 'distance between rows'),
    ('zonal', ('zones',), not_a_tensor, TypeError, 'zones', 'tensor on cuda:'),
    ('zonal', ('zones',), wrong_dtype, TypeError, 'zones', 'tensor on cuda:'),
    ('zonal', ('zones',), wrong_shape, ValueError, 'zones', 'shape'),
    ('zonal', ('zones',), non_unit, ValueError, 'zones', 'unit stride'),
    ('zonal', ('area',), not_a_tensor, TypeError, 'area', 'tensor on cuda:'),
    ('zonal', ('area',), wrong_dtype, TypeError, 'area', 'tensor'),
    ('zonal', ('area',), wrong_shape, TypeError, 'area', 'elements'),
    ('zonal', ('area',), non_unit, ValueError, 'area', 'unit stride'),
    ('zonal_bounds', ('values',), not_a_tensor, TypeError, 'values', 'tensor on cuda:'),
    ('zonal_bounds', ('values',), wrong_dtype, TypeError, 'values', 'tensor on cuda:'),
    ('zonal_bounds', ('values',), non_unit, ValueError, 'values', 'unit stride'),
    ('zonal_bounds', ('values',), rows_too_close, ValueError, 'values', 'distance between rows'),
    ('zonal_bounds', ('area',), not_a_tensor, TypeError, 'area', 'tensor on cuda:'),
    ('zonal_bounds', ('area',), non_unit, ValueError, 'area', 'unit stride'),
    # ---- RasterEngine.trend: the stack
    ('trend', ('values',), not_a_tensor, TypeError, 'values', 'tensor on cuda:'),
    ('trend', ('values',), wrong_dtype, TypeError, 'values', 'tensor on cuda:'),
    ('trend', ('values',), non_unit, ValueError, 'values', 'unit stride'),
    ('trend', ('values',), rows_too_close, ValueError, 'values', 'stride in time'),
    # ---- RasterEngine.anomaly: numerator and denominator
    ('anomaly', ('num',), not_a_tensor, TypeError, 'num', 'tensor on cuda:'),
    ('anomaly', ('num',), wrong_dtype, TypeError, 'num', 'tensor on cuda:'),
    ('anomaly', ('num',), non_unit, ValueError, 'num', 'unit stride'),
    ('anomaly', ('num',), rows_too_close, ValueError, 'num', 'stride in time'),
    ('anomaly', ('num',), pitched, ValueError, 'num and den', 'must share one'),
    ('anomaly', ('den',), not_a_tensor, TypeError, 'den', 'tensor on cuda:'),
    ('anomaly', ('den',), wrong_dtype, TypeError, 'den', 'tensor on cuda:'),
    ('anomaly', ('den',), wrong_shape, ValueError, 'den', 'shape'),
    ('anomaly', ('den',), non_unit, ValueError, 'den', 'unit stride'),
    ('anomaly', ('den',), rows_too_close, ValueError, 'den', 'stride in time'),
    ('anomaly', ('den',), pitched, ValueError, 'num and den', 'must share one'),
    # ---- UpscaleGrid.run and .majority: the layers and the class raster
    ('upscale.run', ('values',), not_a_tensor, TypeError, 'values', 'tensor on cuda:'),
    ('upscale.run', ('values',), wrong_dtype, TypeError, 'values', 'tensor on cuda:'),
    ('upscale.run', ('values',), wrong_shape, ValueError, 'values', 'shape'),
    ('upscale.run', ('values',), non_unit, ValueError, 'values', 'unit stride'),
    ('upscale.run', ('values',), rows_too_close, ValueError, 'values', 'distance between rows'),
    ('upscale.run', ('values',), planes_too_close, ValueError, 'values', 'stride in time'),
    ('upscale.majority', ('cls',), not_a_tensor, TypeError, 'cls', 'tensor on cuda:'),
    ('upscale.majority', ('cls',), wrong_dtype, TypeError, 'cls', 'tensor on cuda:'),
    ('upscale.majority', ('cls',), wrong_shape, ValueError, 'cls', 'shape'),
    ('upscale.majority', ('cls',), non_unit, ValueError, 'cls', 'unit stride'),
    ('upscale.majority', ('cls',), rows_too_close, ValueError, 'cls', 'distance between rows'),
]


@pytest.mark.parametrize('method,path,offence,exc,name,phrase', ONE_ARGUMENT,
                         ids=['%s-%s-%s' % (m, '.'.join(str(p) for p in path), f.__name__)
                              for m, path, f, _, _, _ in ONE_ARGUMENT])
def test_an_input_with_one_offence_is_refused(env, method, path, offence, exc, name, phrase):
    torch, base = env[0], env[3]
    a = put(base[method], path, offence(torch, get(base[method], path)))
    with pytest.raises(exc) as info:
        call(env, method, a)
    assert type(info.value) is exc
    assert name in str(info.value) and phrase in str(info.value), str(info.value)


def out_shapes(torch, method):
    """name -> (shape, dtype) of the caller's output tensors of a method, in the order `out` takes them"""
    f64 = torch.float64
    return {'composite': [((DAYS // PERIOD, N), f64), ((DAYS // PERIOD, N), torch.uint16)],
            'grid.composite': [((DAYS // PERIOD, N), f64), ((DAYS // PERIOD, N), torch.uint16)],
            'grid.fields': [((2, N), f64)],
            'gapfill': [((S, N), torch.uint8), ((S, N), torch.uint8), ((2, S, N), torch.uint8)],
            'daynight': [((D, R, W), f64), ((D, R, W), f64), ((R, W), f64)],
            'trend': [((N,), torch.int32 if k == 's' else torch.uint8 if k == 'count' else f64) for k in TREND_FIELDS],
            'anomaly': [((YEARS * PERIODS, N), f64)] * 2 + [((PERIODS, N), f64)] * 2 + [((PERIODS, N), torch.uint8)],
            'upscale.run': [((K,) + COARSE, f64)] * 2 + [((K,) + COARSE, torch.int32)],
            'upscale.majority': [(COARSE, torch.uint8), (COARSE, torch.float32)]}[method]


#: the names of the outputs of the methods that take `out` as a dict, in the order of `out_shapes`
OUT_NAMES = {'daynight': ('temp_day', 'sw_rad_day', 'temp_annual'), 'trend': TREND_FIELDS, 'anomaly': ANOMALY_FIELDS,
             'upscale.run': UPSCALE_FIELDS, 'upscale.majority': CLASS_FIELDS}


def with_out(torch, method, a, change=None, k=0):
    """The arguments `a` with contiguous output tensors, output k passed through `change`."""
    outs = [full(torch, shape, dt) for shape, dt in out_shapes(torch, method)]
    if change is not None:
        outs[k] = change(torch, outs[k])
    if method == 'grid.fields':
        return put(a, ('out',), outs[0])
    if method in OUT_NAMES:
        return put(a, ('out',), dict(zip(OUT_NAMES[method], outs)))
    if method == 'gapfill':
        return put(put(a, ('out',), outs), ('source',), True)
    return put(a, ('out',), outs)


#: (method, index of the output, offence, exception, name in the message, phrase)
ONE_OUTPUT = [
    ('composite', 0, not_a_tensor, TypeError, 'out[0]', 'tensor on cuda:'),
    ('composite', 1, wrong_dtype, TypeError, 'out[1]', 'tensor on cuda:'),
    ('composite', 0, wrong_dtype, TypeError, 'out[0]', 'tensor on cuda:'),
    ('composite', 1, wrong_shape, ValueError, 'out[1]', 'shape'),
    ('composite', 0, non_unit, ValueError, 'out[0]', 'unit stride'),
    ('composite', 0, rows_too_close, ValueError, 'out', 'distance between rows'),
    ('composite', 1, pitched, ValueError, 'out', 'must share one'),
    ('grid.composite', 0, not_a_tensor, TypeError, 'out[0]', 'tensor on cuda:'),
    ('grid.composite', 0, wrong_dtype, TypeError, 'out[0]', 'tensor on cuda:'),
    ('grid.composite', 0, wrong_shape, ValueError, 'out[0]', 'shape'),
    ('grid.composite', 1, non_unit, ValueError, 'out[1]', 'unit stride'),
    ('grid.composite', 1, rows_too_close, ValueError, 'out', 'distance between rows'),
    ('grid.composite', 0, pitched, ValueError, 'out', 'must share one'),
    ('grid.fields', 0, not_a_tensor, TypeError, 'out', 'tensor on cuda:'),
    ('grid.fields', 0, wrong_dtype, TypeError, 'out', 'tensor on cuda:'),
    ('grid.fields', 0, wrong_shape, ValueError, 'out', 'shape'),
    ('grid.fields', 0, non_unit, ValueError, 'out', 'unit stride'),
    ('grid.fields', 0, rows_too_close, ValueError, 'out', 'distance between rows'),
    ('gapfill', 1, not_a_tensor, TypeError, 'out[1]', 'tensor on cuda:'),
    ('gapfill', 1, wrong_dtype, TypeError, 'out[1]', 'tensor on cuda:'),
    ('gapfill', 1, wrong_shape, ValueError, 'out[1]', 'shape'),
    ('gapfill', 1, non_unit, ValueError, 'out[1]', 'unit stride'),
    ('gapfill', 1, rows_too_close, ValueError, 'out[1]', 'stride in time'),
    ('gapfill', 1, pitched, ValueError, 'out', 'must share one'),
    ('gapfill', 2, not_a_tensor, TypeError, 'source', 'tensor'),
    ('gapfill', 2, wrong_dtype, TypeError, 'source', 'tensor'),
    ('gapfill', 2, wrong_shape, TypeError, 'source', 'shape'),
    ('gapfill', 2, non_unit, ValueError, 'source', 'unit stride'),
    ('gapfill', 2, rows_too_close, ValueError, 'source', 'stride in time'),
    ('gapfill', 2, planes_too_close, ValueError, 'source', 'back to back'),
    ('daynight', 1, not_a_tensor, TypeError, "out['sw_rad_day']", 'tensor on cuda:'),
    ('daynight', 1, wrong_dtype, TypeError, "out['sw_rad_day']", 'tensor on cuda:'),
    ('daynight', 1, wrong_shape, ValueError, "out['sw_rad_day']", 'shape'),
    ('daynight', 2, wrong_shape, ValueError, "out['temp_annual']", 'shape'),
    ('daynight', 1, non_unit, ValueError, "out['sw_rad_day']", 'unit stride'),
    ('daynight', 1, rows_too_close, ValueError, "out['sw_rad_day']", 'distance between rows'),
    ('daynight', 2, rows_too_close, ValueError, "out['temp_annual']", 'distance between rows'),
    ('daynight', 1, planes_too_close, ValueError, "out['sw_rad_day']", 'stride in time'),
    ('daynight', 1, pitched, ValueError, 'out', 'must share one'),
    ('daynight', 2, pitched, ValueError, 'out', 'must share one'),
    ('trend', 4, not_a_tensor, TypeError, "out['s']", 'tensor on cuda:'),
    ('trend', 4, wrong_dtype, TypeError, "out['s']", 'tensor on cuda:'),
    ('trend', 0, wrong_dtype, TypeError, "out['slope']", 'tensor on cuda:'),
    ('trend', 6, wrong_shape, ValueError, "out['count']", 'shape'),
    ('trend', 3, non_unit, ValueError, "out['slope_hi']", 'unit stride'),
    ('anomaly', 1, not_a_tensor, TypeError, "out['pct']", 'tensor on cuda:'),
    ('anomaly', 1, wrong_dtype, TypeError, "out['pct']", 'tensor on cuda:'),
    ('anomaly', 4, wrong_dtype, TypeError, "out['count']", 'tensor on cuda:'),
    ('anomaly', 1, wrong_shape, ValueError, "out['pct']", 'shape'),
    ('anomaly', 3, wrong_shape, ValueError, "out['std']", 'shape'),
    ('anomaly', 1, non_unit, ValueError, "out['pct']", 'unit stride'),
    ('anomaly', 1, rows_too_close, ValueError, "out['pct']", 'stride in time'),
    ('anomaly', 2, rows_too_close, ValueError, "out['mean']", 'stride in time'),
    ('anomaly', 1, pitched, ValueError, "out['z'] and out['pct']", 'must share one'),
    ('anomaly', 4, pitched, ValueError, "out['mean'], out['std'] and out['count']", 'must share one'),
    ('upscale.run', 1, not_a_tensor, TypeError, "out['fraction']", 'tensor on cuda:'),
    ('upscale.run', 1, wrong_dtype, TypeError, "out['fraction']", 'tensor on cuda:'),
    ('upscale.run', 2, wrong_dtype, TypeError, "out['count']", 'tensor on cuda:'),
    ('upscale.run', 1, wrong_shape, ValueError, "out['fraction']", 'shape'),
    ('upscale.run', 1, non_unit, ValueError, "out['fraction']", 'unit stride'),
    ('upscale.run', 1, rows_too_close, ValueError, "out['fraction']", 'distance between rows'),
    ('upscale.run', 1, planes_too_close, ValueError, "out['fraction']", 'stride in time'),
    ('upscale.majority', 1, not_a_tensor, TypeError, "out['share']", 'tensor on cuda:'),
    ('upscale.majority', 1, wrong_dtype, TypeError, "out['share']", 'tensor on cuda:'),
    ('upscale.majority', 0, wrong_shape, ValueError, "out['cls']", 'shape'),
    ('upscale.majority', 1, non_unit, ValueError, "out['share']", 'unit stride'),
    ('upscale.majority', 1, rows_too_close, ValueError, "out['share']", 'distance between rows'),
]


@pytest.mark.parametrize('method,k,offence,exc,name,phrase', ONE_OUTPUT,
                         ids=['%s-out%d-%s' % (m, k, f.__name__) for m, k, f, _, _, _ in ONE_OUTPUT])
def test_an_output_with_one_offence_is_refused(env, method, k, offence, exc, name, phrase):
    torch, base = env[0], env[3]
    with pytest.raises(exc) as info:
        call(env, method, with_out(torch, method, base[method], offence, k))
    assert type(info.value) is exc
    assert name in str(info.value) and phrase in str(info.value), str(info.value)


def test_flat_outputs_and_accumulators_with_one_offence_are_refused(env):
    """DownscaleGrid.run's out_day / out_night and zonal's acc are flat, contiguous arrays."""
    torch, eng, grid, base = env
    run, zonal = base['grid.run'], base['zonal']
    day = torch.zeros(N, dtype=torch.float64, device='cuda')
    acc = torch.zeros((K, NZ, 10), dtype=torch.int64, device='cuda')
    cases = [('grid.run', put(run, ('out_day',), not_a_tensor(torch, day)), TypeError, 'out_day', 'tensor on cuda:'),
             ('grid.run', put(run, ('out_night',), wrong_dtype(torch, day)), TypeError, 'out_night', 'tensor on cuda:'),
             ('grid.run', put(run, ('out_day',), wrong_shape(torch, day)), ValueError, 'out_day', 'elements'),
             ('grid.run', put(run, ('out_night',), non_unit(torch, day)), TypeError, 'out_night', 'contiguous'),
             ('zonal', put(zonal, ('acc',), not_a_tensor(torch, acc)), TypeError, 'acc', 'tensor on cuda:'),
             ('zonal', put(zonal, ('acc',), wrong_dtype(torch, acc)), TypeError, 'acc', 'tensor on cuda:'),
             ('zonal', put(zonal, ('acc',), wrong_shape(torch, acc)), ValueError, 'acc', 'shape'),
             ('zonal', put(zonal, ('acc',), non_unit(torch, acc)), TypeError, 'acc', 'contiguous')]
    for method, a, exc, name, phrase in cases:
        with pytest.raises(exc) as info:
            call(env, method, a)
        assert type(info.value) is exc, (method, name, phrase)
        assert name in str(info.value) and phrase in str(info.value), str(info.value)


def test_a_wrong_number_of_outputs_is_refused(env):
    torch, base = env[0], env[3]
    for method in ('composite', 'grid.composite', 'gapfill'):
        a = with_out(torch, method, base[method])
        with pytest.raises(ValueError, match='out must hold'):
            call(env, method, put(a, ('out',), a['out'][:-1]))
        with pytest.raises(ValueError, match='out must hold'):
            call(env, method, put(a, ('out',), a['out'] + a['out'][:1]))
    a = with_out(torch, 'daynight', base['daynight'])
    fewer = {n: t for n, t in a['out'].items() if n != 'temp_annual'}
    with pytest.raises(ValueError, match='out must hold'):
        call(env, 'daynight', put(a, ('out',), fewer))
    with pytest.raises(ValueError, match='out must hold'):
        call(env, 'daynight', put(a, ('out',), dict(a['out'], temp_night=a['out']['temp_day'].clone())))


@pytest.mark.parametrize('method,phrase', [('daynight', 'exactly the requested'), ('trend', 'exactly the fields'),
                                           ('anomaly', 'exactly the fields'), ('upscale.run', 'exactly the fields'),
                                           ('upscale.majority', 'exactly the fields')])
def test_a_missing_and_a_surplus_output_key_are_refused(env, method, phrase):
    torch, base = env[0], env[3]
    a = with_out(torch, method, base[method])
    last = OUT_NAMES[method][-1]
    for out in ({k: t for k, t in a['out'].items() if k != last}, dict(a['out'], surplus=a['out'][last].clone())):
        with pytest.raises(ValueError) as info:
            call(env, method, put(a, ('out',), out))
        assert type(info.value) is ValueError
        assert 'out must hold' in str(info.value) and phrase in str(info.value), str(info.value)
        assert all(k in str(info.value) for k in OUT_NAMES[method])           # the message lists what is produced


def test_an_output_that_overlaps_an_input_is_refused(env):
    torch, eng, grid, base = env
    # gap filling: a field as its own output; day / night: a plane of t as temp_annual
    a = base['gapfill']
    with pytest.raises(ValueError, match='output overlaps'):
        call(env, 'gapfill', put(a, ('out',), [a['fields'][0], torch.empty_like(a['fields'][1])]))
    a = base['daynight']
    out = with_out(torch, 'daynight', a)['out']
    with pytest.raises(ValueError, match='output overlaps'):
        call(env, 'daynight', put(a, ('out',), dict(out, temp_annual=a['fields']['t'][0])))
    with pytest.raises(ValueError, match='output overlaps'):
        call(env, 'daynight', put(a, ('out',), dict(out, temp_day=out['sw_rad_day'])))
    # zonal: the last words of the accumulator are the first values
    words = K * NZ * 10
    buf = torch.zeros(words + K * N, dtype=torch.int64, device='cuda')
    values = buf.view(torch.float64)[words - 1:words - 1 + K * N].view(K, N)
    a = put(put(base['zonal'], ('values',), values), ('acc',), buf[:words].view(K, NZ, 10))
    with pytest.raises(ValueError, match='acc overlaps'):
        call(env, 'zonal', a)
    eng.check()


def padding(torch, view):
    """the elements of the buffer behind a `pitched` view that are not the view's"""
    buf = signed(torch, view._base)
    mine = torch.zeros(buf.shape, dtype=torch.bool, device='cuda')
    (mine[1:-1] if view.dim() == 1 else mine[..., :-1, 1:-2]).fill_(True)
    return buf[~mine]


@pytest.mark.parametrize('method', ['composite', 'grid.composite', 'grid.run', 'grid.fields', 'gapfill', 'daynight',
                                    'zonal', 'zonal_bounds', 'trend', 'anomaly', 'upscale.run', 'upscale.majority'])
def test_pitched_offset_views_give_the_bits_of_contiguous_copies(env, method):
    """Every tensor argument (inputs and, where the method takes them, outputs) as a view one element
    into a larger buffer with rows 3 elements and planes a row further apart than they are long."""
    torch, eng, grid, base = env
    a = put(base[method], ('source',), True) if method == 'gapfill' else base[method]
    want = outputs_of(torch, env, method, a)
    assert all(t.is_contiguous() for t in want if isinstance(t, torch.Tensor))

    def view(x):
        if isinstance(x, torch.Tensor) and x.dim() >= 1:
            return pitched(torch, x)
        if isinstance(x, dict):
            return {k: view(v) for k, v in x.items()}
        if isinstance(x, list):
            return [view(v) for v in x]
        return x
    flat = ('cls',) if method.startswith('grid') else ()     # contiguous by contract
    b = {k: (v if k in flat or k == 'tables' else view(v)) for k, v in a.items()}
    poisoned = []
    if method == 'grid.run':      # its fine drivers and outputs are flat arrays: offset, not pitched
        b['out_day'], b['out_night'] = full(torch, (N + 1,), torch.float64)[1:], full(torch, (N + 1,), torch.float64)[1:]
    elif method == 'zonal':
        b['acc'] = None
    elif method != 'zonal_bounds':
        b = with_out(torch, method, b, None)
        poison = lambda t: pitched(torch, t, fill=77)
        if isinstance(b['out'], dict):
            b['out'] = {k: poison(v) for k, v in b['out'].items()}
        elif isinstance(b['out'], list):
            b['out'] = [poison(v) for v in b['out']]
        else:
            b['out'] = poison(b['out'])
        poisoned = list(b['out'].values()) if isinstance(b['out'], dict) else list(b['out']) if isinstance(b['out'], list) \
            else [b['out']]
        if method == 'gapfill':
            # (the source tensor holds its fields back to back: pitched rows, dense planes)
            b['out'][2] = torch.full((2, S, N + 3), 77, dtype=torch.uint8, device='cuda')[:, :, 1:-2]
            poisoned.pop()
    got = outputs_of(torch, env, method, b)
    if method not in ('grid.run', 'zonal', 'zonal_bounds', 'trend'):      # (a trend's outputs are (n,): offset only)
        assert any(not t.is_contiguous() for t in got)
    for t in poisoned:                       # what lies in front of, between and behind the rows is not touched
        assert bool((padding(torch, t) == 77).all())
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(g, torch.Tensor):
            assert g.shape == w.shape and g.dtype == w.dtype
            assert signed(torch, g).contiguous().view(torch.uint8).equal(signed(torch, w).contiguous().view(torch.uint8))
        else:
            assert g == w
