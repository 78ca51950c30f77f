"""GPU tests of the day / night aggregation (mod16_daynight_f32 / _f64: RasterEngine.daynight,
mod16_amd.aggregate_daynight) against its numpy definition (mod16_amd/daynight.py, itself held to its
properties and to a scalar loop by tests/test_daynight_host.py). Every output except the two VPDs must
have the BITS of the definition (parity.same_bits; NaN is any NaN): the definition is float64
arithmetic in a fixed order with one rounding, so there is no tolerance. The VPDs must have the bits of
mod16_amd.MOD16.vpd (the library's own method kernel: the device's exp) on the definition's aggregated
planes, and agree with the numpy oracle within RTOL = 2e-13, the bound tests/test_gpu_methods.py holds
that method to (exp differs from glibc's by an ulp; everything else is IEEE-exact).

Grids (rows x columns; a lane owns two consecutive cells of a row):
  scalar  5 x 37, row pitch 40, plane stride 205, base offset of one element: nothing is aligned
  vector  4 x 64 contiguous: every lane takes vector accesses
  ragged  3 x 66 contiguous: 33 lanes a row
  tail    3 x 67, row pitch 68, plane stride 206, aligned: 33 vector lanes and a one-cell lane per row
D in (1, 3, 11) (a lane walks chunks of 4 days: 11 days are chunks of 4, 4 and 3), H in (1, 8, 24),
float32 and float64 inputs x float32 and float64 outputs. The first and last row are the poles
(half_day 0 and 12, swapped on odd days), the longitudes span the full circle. Every field holds a NaN
step in a cell of its own, one cell is above saturation. The definition of a configuration is computed
once and shared."""
import functools

import numpy as np
import pytest

from mod16_amd import daynight as dn
from oracle import mod16_oracle as oracle
import parity

pytestmark = pytest.mark.gpu

RTOL = 2e-13          # tests/test_gpu_methods.py: RTOL
RTOL_FAST = 1e-8      # tests/test_gpu_parity.py: RTOL['fast']
#: rows, columns, row pitch, plane stride, base offset (elements)
GRIDS = {'scalar': (5, 37, 40, 205, 1), 'vector': (4, 64, 64, 256, 0), 'ragged': (3, 66, 66, 198, 0),
         'tail': (3, 67, 68, 206, 0)}
TYPES = (('float32', 'float32'), ('float32', 'float64'), ('float64', 'float32'), ('float64', 'float64'))
PLAIN = tuple(n for n in dn.OUTPUT_NAMES if not n.startswith('vpd'))


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    return torch, mod16_amd


@functools.lru_cache(maxsize=None)
def table():
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    t = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def engine(dtype='float64'):
    from mod16_amd.raster import RasterEngine
    return RasterEngine(table(), dtype=dtype)


@functools.lru_cache(maxsize=None)
def tables(D, R, W):
    """(half_day, noon, offset): the poles in the first and last row, swapped on odd days; noon in 12
    +- 0.3; longitudes -180 ... 180 (exclusive)."""
    rng = np.random.default_rng(100 * D + R)
    half = rng.uniform(0.5, 11.5, (D, R))
    half[:, 0], half[:, -1] = 0.0, 12.0
    half[1::2, 0], half[1::2, -1] = 12.0, 0.0
    noon = 12.0 + rng.uniform(-0.3, 0.3, D)
    offset = (-180.0 + 360.0 / W * np.arange(W)) / 15.0
    for a in (half, noon, offset):
        a.setflags(write=False)
    return half, noon, offset


@functools.lru_cache(maxsize=None)
def fields(D, H, R, W, dtype, humid=False):
    """The five hourly series, read-only. humid: relative humidity 0.4 ... 0.6 at every step and a
    diurnal temperature range of 6 K, so that the aggregated humidity stays within 0.2 ... 0.8 and no NaN."""
    rng = np.random.default_rng(7 + D + 10 * H + 100 * R)
    S = D * H
    shape = (S, R, W)
    t = rng.uniform(255.0, 305.0, (1, R, W)) + rng.uniform(-3.0, 3.0, shape)
    ps = rng.uniform(6e4, 1.02e5, shape)
    if humid:
        avp = rng.uniform(0.4, 0.6, shape) * 610.7 * np.exp(17.38 * (t - 273.15) / (239 + (t - 273.15)))
        qv = 0.622 * avp / (ps - 0.379 * avp)
    else:
        qv = rng.uniform(0.001, 0.02, shape)
    sw = np.maximum(rng.uniform(-600.0, 900.0, shape), 0.0)
    lw = rng.uniform(-120.0, -10.0, shape)
    if not humid:
        qv[:, 0, 0] = 0.05                              # above saturation at every step ...
        t[:, 0, 0] = rng.uniform(272.0, 278.0, S)       # ... of a cold cell (saturation near 700 Pa, 4 kPa of vapour)
        t[min(S - 1, 1), 1, 5] = np.nan
        qv[0, 2, 7] = np.nan
        ps[S - 1, 1, 9] = np.nan
        sw[0, 0, 11] = np.nan
        lw[S - 1, 2, 13] = np.nan
    out = {'t': t, 'qv': qv, 'ps': ps, 'sw': sw, 'lw': lw}
    out = {k: v.astype(dtype) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def definition(D, H, R, W, in_dtype, out_dtype, mode='solar', humid=False):
    f = fields(D, H, R, W, in_dtype, humid)
    kw = dict(zip(('half_day', 'noon', 'offset'), tables(D, R, W))) if mode == 'solar' else {'sw_threshold': 25.0}
    res, annual = dn.aggregate(f, H, dtype=out_dtype, **kw)
    for a in tuple(res) + (annual,):
        a.setflags(write=False)
    return res, annual


@functools.lru_cache(maxsize=None)
def aggregated(D, H, R, W, in_dtype, mode='solar', humid=False):
    """The float64 (day, night) planes of t, qv and ps of the definition: what the VPDs are made from."""
    f = fields(D, H, R, W, in_dtype, humid)
    if mode == 'solar':
        w = np.broadcast_to(dn.day_weights(H, *tables(D, R, W)), (D, H, R, W))
    else:
        w = dn.sw_weights(f['sw'], H, 25.0)
    return {k: dn.split_field(f[k], w)[:2] for k in ('t', 'qv', 'ps')}


def place(torch, a, pitch, plane, base, fill=None):
    """a (S, R, W) -> (the flat device buffer, a view of it with the given row pitch, plane stride and
    base offset holding a's values); fill: what the rest of the buffer holds"""
    S, R, W = a.shape
    total = base + (S - 1) * plane + (R - 1) * pitch + W + 6
    tdtype = {'float32': torch.float32, 'float64': torch.float64}[a.dtype.name]
    buf = torch.full((total,), -777.0 if fill is None else fill, dtype=tdtype, device='cuda')
    view = buf.as_strided((S, R, W), (plane, pitch, 1), base)
    view.copy_(torch.from_numpy(np.array(a)).cuda())
    return buf, view


def placed_fields(torch, f, grid):
    R, W, pitch, plane, base = GRIDS[grid]
    return {k: place(torch, v, pitch, plane, base)[1] for k, v in f.items()}


SENTINEL = -12345.5


def out_buffers(torch, names, D, grid, dtype):
    """One sentinel-filled buffer per output with the grid's pitch, plane stride and base offset ->
    ({name: buffer}, {name: view})"""
    R, W, pitch, plane, base = GRIDS[grid]
    bufs, views = {}, {}
    for n in names:
        planes = 1 if n == 'temp_annual' else D
        b, v = place(torch, np.full((planes, R, W), SENTINEL, dtype), pitch, plane, base, fill=SENTINEL)
        bufs[n], views[n] = b, (v[0] if n == 'temp_annual' else v)
    return bufs, views


def check_padding(torch, bufs, views, what):
    """everything of a buffer outside its view still holds the sentinel"""
    for n, b in bufs.items():
        host = b.cpu().numpy().copy()
        v = views[n]
        idx = torch.arange(host.size).as_strided(tuple(v.shape), tuple(v.stride()), v.storage_offset()).numpy().reshape(-1)
        mask = np.ones(host.shape, bool)
        mask[idx] = False
        assert np.all(host[mask] == SENTINEL), (what, n)


def vpd_planes(m16, parts):
    """(vpd_day, vpd_night) as MOD16.vpd gives them on the aggregated float64 planes, night clamped"""
    day = np.asarray(m16.MOD16.vpd(parts['qv'][0], parts['ps'][0], parts['t'][0]))
    night = np.asarray(m16.MOD16.vpd(parts['qv'][1], parts['ps'][1], parts['t'][1]))
    with np.errstate(invalid='ignore'):
        return day, np.where(night < 0, 0.0, night)


def compare(res, annual, want, want_annual, what):
    for n in PLAIN:
        assert parity.same_bits(getattr(res, n).cpu().numpy(), getattr(want, n)), (what, n)
    assert parity.same_bits(annual.cpu().numpy(), want_annual), (what, 'temp_annual')


def test_all_three_windows_contribute():
    """the longitudes of these tests span the circle: each of the windows m = -H, 0, +H of the weight
    formula is the one that gives some cell its weight (asserted on the definition)"""
    D, H = 3, 24
    R, W = GRIDS['scalar'][:2]
    half, noon, offset = tables(D, R, W)
    delta = 24.0 / H
    a = (((noon[:, None, None] - half[:, :, None]) - offset[None, None, :]) / delta)[:, None]
    b = (((noon[:, None, None] + half[:, :, None]) - offset[None, None, :]) / delta)[:, None]
    k = np.arange(H, dtype=np.float64)[None, :, None, None]
    for m in (-float(H), 0.0, float(H)):
        assert np.maximum(np.minimum(k + 1.0, b + m) - np.maximum(k, a + m), 0.0).max() > 0.0, m
    assert np.any(half[:, 0] == 0.0) and np.any(half[:, 0] == 12.0) and np.any(half[:, -1] == 12.0)


@pytest.mark.parametrize('H', (1, 8, 24))
@pytest.mark.parametrize('D', (1, 3, 11))
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_solar_mode_has_the_bits_of_the_definition(env, grid, D, H):
    torch, m16 = env
    R, W = GRIDS[grid][:2]
    half, noon, offset = tables(D, R, W)
    for in_dtype, out_dtype in TYPES:
        f = fields(D, H, R, W, in_dtype)
        want, want_annual = definition(D, H, R, W, in_dtype, out_dtype)
        names = dn.OUTPUT_NAMES + ('temp_annual',)
        bufs, views = out_buffers(torch, names, D, grid, out_dtype)
        res, annual = engine().daynight(placed_fields(torch, f, grid), half, noon, offset, steps_per_day=H,
                                        dtype=out_dtype, out=views)
        what = (grid, D, H, in_dtype, out_dtype)
        assert annual is views['temp_annual'] and res.tmin is views['tmin']
        compare(res, annual, want, want_annual, what)
        check_padding(torch, bufs, views, what)
        # NaN steps: the cell-day of a field's NaN is NaN in that field's outputs (the definition says where)
        assert np.isnan(want.lw_net_day).sum() == 1 and np.isnan(want.tmin).sum() == 1
        # the VPDs: the library's own vpd on the definition's aggregated planes, rounded once
        day, night = vpd_planes(m16, aggregated(D, H, R, W, in_dtype))
        assert parity.same_bits(res.vpd_day.cpu().numpy(), day.astype(out_dtype)), what
        assert parity.same_bits(res.vpd_night.cpu().numpy(), night.astype(out_dtype)), what
        got_night = res.vpd_night.cpu().numpy()
        assert np.all(got_night[:, 0, 0] == 0.0) and not np.signbit(got_night[:, 0, 0]).any()    # above saturation
        assert np.isnan(got_night).sum() == 3 and np.isnan(res.vpd_day.cpu().numpy()).sum() == 3  # t, qv, ps: one cell-day each


@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_sw_mode_has_the_bits_of_the_definition(env, grid):
    torch, m16 = env
    D, H = 3, 8
    R, W = GRIDS[grid][:2]
    for in_dtype, out_dtype in TYPES:
        f = fields(D, H, R, W, in_dtype)
        want, want_annual = definition(D, H, R, W, in_dtype, out_dtype, mode='sw')
        res, annual = engine().daynight(placed_fields(torch, f, grid), sw_threshold=25.0, steps_per_day=H, dtype=out_dtype)
        what = (grid, in_dtype, out_dtype)
        compare(res, annual, want, want_annual, what)
        assert np.isnan(want.day_hours).sum() == 1          # the NaN step of sw: its weight is NaN
        day, night = vpd_planes(m16, aggregated(D, H, R, W, in_dtype, mode='sw'))
        assert parity.same_bits(res.vpd_day.cpu().numpy(), day.astype(out_dtype)), what
        assert parity.same_bits(res.vpd_night.cpu().numpy(), night.astype(out_dtype)), what
        assert res.tmin.stride() == res.vpd_day.stride() and annual.stride(0) == res.tmin.stride(1)


def test_vpd_agrees_with_the_oracle(env):
    """relative humidity 0.2 ... 0.8 in the aggregated planes (asserted): no cell has to be left out for
    cancellation; the bound is the one tests/test_gpu_methods.py holds MOD16.vpd to"""
    torch, m16 = env
    D, H, grid = 3, 8, 'vector'
    R, W = GRIDS[grid][:2]
    half, noon, offset = tables(D, R, W)
    f = fields(D, H, R, W, 'float64', humid=True)
    parts = aggregated(D, H, R, W, 'float64', humid=True)
    res, _ = engine().daynight(placed_fields(torch, f, grid), half, noon, offset, steps_per_day=H,
                               outputs=('vpd_day', 'vpd_night'))
    for k, name in enumerate(('vpd_day', 'vpd_night')):
        qv, ps, t = parts['qv'][k], parts['ps'][k], parts['t'][k]
        want = oracle.vpd_from_humidity(qv, ps, t)
        sv = 610.7 * np.exp(17.38 * (t - 273.15) / (239 + (t - 273.15)))
        rh = 1.0 - want / sv
        assert rh.min() >= 0.2 and rh.max() <= 0.8, (name, rh.min(), rh.max())
        err = parity.assert_parity(getattr(res, name).cpu().numpy(), want, RTOL, name)
        print('%s against the oracle: max relative error %.3g' % (name, err))
    assert res.tmin is None and res.day_hours is None


def test_outputs_left_out_stay_untouched_and_two_calls_agree(env):
    torch, m16 = env
    D, H, grid = 3, 8, 'scalar'
    R, W, pitch, plane, base = GRIDS[grid]
    half, noon, offset = tables(D, R, W)
    f = fields(D, H, R, W, 'float32')
    want, want_annual = definition(D, H, R, W, 'float32', 'float64')
    every = dn.OUTPUT_NAMES + ('temp_annual',)
    asked = ('sw_rad_day', 'temp_night', 'day_hours', 'temp_annual')
    bufs, views = out_buffers(torch, every, D, grid, 'float64')
    dev = placed_fields(torch, f, grid)
    res, annual = engine().daynight({k: dev[k] for k in ('t', 'sw')}, half, noon, offset, steps_per_day=H,
                                    outputs=asked, dtype='float64', out={n: views[n] for n in asked})
    for n in every:
        host = bufs[n].cpu().numpy()
        if n not in asked:
            assert np.all(host == SENTINEL), n
            assert n == 'temp_annual' or getattr(res, n) is None
    for n in asked[:3]:
        assert parity.same_bits(getattr(res, n).cpu().numpy(), getattr(want, n)), n
    assert parity.same_bits(annual.cpu().numpy(), want_annual)
    check_padding(torch, {n: bufs[n] for n in asked}, views, 'asked')
    again, annual2 = engine().daynight({k: dev[k] for k in ('t', 'sw')}, half, noon, offset, steps_per_day=H,
                                       outputs=asked, dtype='float64')
    for n in asked[:3]:
        assert parity.same_bits(getattr(again, n).cpu().numpy(), getattr(res, n).cpu().numpy()), n
        assert getattr(again, n).is_contiguous()
    assert parity.same_bits(annual2.cpu().numpy(), annual.cpu().numpy())
    with pytest.raises(ValueError, match='overlaps'):
        engine().daynight({'t': dev['t']}, half, noon, offset, steps_per_day=H, outputs=('temp_annual',), dtype='float32',
                          out={'temp_annual': dev['t'][0]})


@pytest.mark.parametrize('in_dtype', ('float32', 'float64'))
def test_host_mode_equals_device_mode_whatever_the_chunks(env, in_dtype):
    torch, m16 = env
    D, H, grid = 5, 8, 'scalar'
    R, W = GRIDS[grid][:2]
    half, noon, offset = tables(D, R, W)
    f = fields(D, H, R, W, in_dtype)
    for out_dtype in ('float32', 'float64'):
        res, annual = engine().daynight(placed_fields(torch, f, grid), half, noon, offset, steps_per_day=H, dtype=out_dtype)
        want, want_annual = definition(D, H, R, W, in_dtype, out_dtype)
        per_day = 5 * H * R * W * np.dtype(in_dtype).itemsize + 10 * R * W * np.dtype(out_dtype).itemsize
        for stage in (per_day, 2 * per_day + 100, None):        # chunks of one day, of two (2, 2, 1), one chunk
            host, host_annual = m16.aggregate_daynight(f, half, noon, offset, steps_per_day=H, dtype=out_dtype, stage_bytes=stage)
            for n in dn.OUTPUT_NAMES:
                assert parity.same_bits(getattr(host, n), getattr(res, n).cpu().numpy()), (n, stage, out_dtype)
            assert parity.same_bits(host_annual, annual.cpu().numpy()), (stage, out_dtype)
            for n in PLAIN:
                assert parity.same_bits(getattr(host, n), getattr(want, n)), (n, stage, out_dtype)
            assert parity.same_bits(host_annual, want_annual)
    # the default output type follows the inputs; out= arrays are written in place
    asked = ('tmin', 'day_hours', 'temp_annual')
    out = {'tmin': np.full((D, R, W), SENTINEL, in_dtype), 'day_hours': np.full((D, R, W), SENTINEL, in_dtype),
           'temp_annual': np.full((R, W), SENTINEL, in_dtype)}
    got, got_annual = m16.aggregate_daynight({'t': f['t']}, half, noon, offset, steps_per_day=H, outputs=asked, out=out)
    want, want_annual = definition(D, H, R, W, in_dtype, in_dtype)
    assert got.tmin is out['tmin'] and got_annual is out['temp_annual'] and got.temp_day is None
    assert got.tmin.dtype == np.dtype(in_dtype)
    assert parity.same_bits(out['tmin'], want.tmin) and parity.same_bits(out['day_hours'], want.day_hours)
    assert parity.same_bits(out['temp_annual'], want_annual)


def test_daynight_feeds_the_downscaled_composite(env):
    """Hourly fields on a 5 x 8 grid -> eng.daynight -> eng.downscale_grid(...).composite over a 6 x 10
    fine raster, D = 8 days in one period: equal, counts included, to evapotranspiration_composite_downscaled
    on the definition's numpy planes (the VPDs among them as MOD16.vpd gives them on the definition's
    aggregated planes: the bits the kernel is held to above) -- the pitch and stride conventions of the
    two families line up. With the definition's own numpy VPDs (glibc's exp) the totals agree within
    the FAST arithmetic's bound."""
    torch, m16 = env
    from mod16_amd import downscale as ds
    D, H, R, W = 8, 24, 5, 8
    FR, FC = 6, 10
    eng = engine()
    rng = np.random.default_rng(99)
    f = fields(D, H, R, W, 'float64', humid=True)
    half, noon, offset = tables(D, R, W)
    half = np.clip(half, 3.0, 9.0)          # no polar rows here: every day has a day and a night
    want, want_annual = dn.aggregate(f, H, half, noon, offset)
    parts = {k: dn.split_field(f[k], np.broadcast_to(dn.day_weights(H, half, noon, offset), (D, H, R, W)))[:2]
             for k in ('t', 'qv', 'ps')}
    vday, vnight = vpd_planes(m16, parts)
    res, annual = eng.daynight({k: torch.from_numpy(np.array(v)).cuda() for k, v in f.items()}, half, noon, offset,
                               steps_per_day=H)
    torch.cuda.synchronize()
    cls = rng.integers(0, 13, (FR, FC)).astype(np.uint8)
    pressure = rng.uniform(8.5e4, 1.01e5, (R, W))
    zeros = np.zeros((R, W))
    row_pos = ds.positions(-0.3, 0.8, FR, 0.0, 1.0)
    col_pos = ds.positions(-1.2, 0.9, FC, 0.0, 1.0)
    coarse = ds.MET_DRIVERS + ('day_hours',)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    grid = eng.downscale_grid((FR, FC), (R, W), row_pos, col_pos, wrap=True)
    drivers = [res.lw_net_day, res.lw_net_night, res.sw_rad_day, dev(zeros), 0.2, res.temp_day, res.temp_night, annual,
               res.tmin, res.vpd_day, res.vpd_night, dev(pressure), 0.5, 2.0]
    out = grid.composite(dev(cls.reshape(-1)), drivers, res.day_hours, days=D, period_days=8, coarse=coarse)
    eng.ctx.check_status(eng._stream())
    torch.cuda.synchronize()
    got_et = out[0].cpu().numpy()
    got_count = out[1].view(torch.int16).cpu().numpy().view(np.uint16)
    grid.close()

    def host(vd, vn):
        return m16.evapotranspiration_composite_downscaled(
            table(), cls, want.lw_net_day, want.lw_net_night, want.sw_rad_day, zeros, 0.2, want.temp_day,
            want.temp_night, want_annual, want.tmin, vd, vn, pressure, 0.5, 2.0, want.day_hours, row_pos, col_pos,
            days=D, period_days=8, wrap=True, coarse=coarse)
    ref = host(vday, vnight)
    assert parity.same_bits(got_et.reshape(ref.et.shape), ref.et)
    assert np.array_equal(got_count.reshape(ref.count.shape), ref.count)
    assert np.isfinite(ref.et[:, cls != 0]).any() and ref.count.max() == D
    loose = host(want.vpd_day, want.vpd_night)
    assert np.array_equal(loose.count, ref.count)
    parity.assert_parity(got_et.reshape(loose.et.shape), loose.et, RTOL_FAST, 'definition VPDs')
