"""GPU tests of the downscaled forward run (mod16_et_downscaled_*, mod16_downscale_fields_*:
RasterEngine.downscale_grid, mod16_amd.evapotranspiration_downscaled) against what it replaces --
the coarse drivers blown up to the fine grid by the numpy definition (mod16_amd.downscale.interpolate),
then RasterEngine.run -- bit for bit, and against the numpy oracle.

Shapes: fine grid 37 x 53 (n = 1961: eight batches of 256 pixels, each spanning several rows, a
ragged last one) over a coarse grid 5 x 7; the fine rows run from 0.8 cells above the coarse grid
to 0.3 below it (held edges), the fine columns from 9.3 cells left of it to 5 right of it (three
wraps of the 7 cells). Fine drivers and classes from oracle.synth with its special values (NaN,
0 and 1 in fPAR / LAI, classes without parameters), coarse drivers from oracle.synth without.

Tolerance against the oracle: 1e-8 relative, what tests/test_gpu_parity.py holds the FAST float64
step kernel to (RTOL['fast']; tighter than parity.RTOL_NORTH_STAR) -- the oracle runs on the drivers
the numpy definition materialises, so the interpolation adds nothing to it."""
import functools

import numpy as np
import pytest

from oracle import mod16_oracle as oracle
from oracle import synth
import parity

pytestmark = pytest.mark.gpu

R, C, H, W = 37, 53, 5, 7
N = R * C
RTOL_FAST = 1e-8                     # tests/test_gpu_parity.py: RTOL['fast']
MARK64 = 0x7ff80000000d05ca          # DsMark<double>, csrc/mod16_downscale.hpp
MARK32 = 0x7fcd05ca
MIX = ('sw_albedo', 'temp_day', 'vpd_day', 'pressure', 'lai')


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


@functools.lru_cache(maxsize=None)
def inputs(seed=61):
    """(cls (R, C), the 14 drivers on the fine grid, the 14 on the coarse grid, row_pos, col_pos):
    numpy, read-only."""
    from mod16_amd import downscale as ds
    cls, fine = synth.drivers((R, C), seed=seed, special=True)
    _, coarse = synth.drivers((H, W), seed=seed + 1, special=False)
    row_pos = ds.positions(-0.8, 0.17, R, 0.0, 1.0)
    col_pos = ds.positions(-9.3, 0.41, C, 0.0, 1.0)
    for a in [cls, row_pos, col_pos] + fine + coarse:
        a.setflags(write=False)
    return cls, tuple(fine), tuple(coarse), row_pos, col_pos


def pick(ds, fine, coarse, names):
    """The 14 drivers of a call whose coarse drivers are `names` (sw_rad_night a scalar unless coarse)."""
    out = [c if name in names else f for name, f, c in zip(ds.DRIVER_NAMES, fine, coarse)]
    if 'sw_rad_night' not in names:
        out[3] = 0.0
    return out


def materialise(ds, drivers, names, row_pos, col_pos, wrap, method):
    """What the user did before: every coarse driver on the fine grid, by the numpy definition."""
    rt = ds.corner_tables(row_pos, H, False, method)
    ct = ds.corner_tables(col_pos, W, wrap, method)
    return [ds.interpolate(d, rt, ct) if name in names else d for name, d in zip(ds.DRIVER_NAMES, drivers)]


def put(torch, eng, a):
    return torch.from_numpy(np.array(a, eng.np_dtype)).to(eng._dev()) if isinstance(a, np.ndarray) else a


def run_step(torch, eng, cls, drivers):
    """RasterEngine.run on (R, C) numpy drivers -> numpy (day, night), flat."""
    out = eng.run(torch.from_numpy(np.array(cls)).to(eng._dev()).reshape(-1),
                  [put(torch, eng, d).reshape(-1) if isinstance(d, np.ndarray) else d for d in drivers])
    eng.check()
    return [o.cpu().numpy() for o in out]


def run_grid(torch, ds, eng, cls, drivers, names, row_pos, col_pos, wrap=False, method='bilinear', first=0, n=None):
    """DownscaleGrid.run on numpy inputs, pixels [first, first + n) -> numpy (day, night)."""
    n = N - first if n is None else n
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=wrap, method=method)
    dev = []
    for name, d in zip(ds.DRIVER_NAMES, drivers):
        if not isinstance(d, np.ndarray):
            dev.append(d)
        elif name in names:
            dev.append(put(torch, eng, d))
        else:
            dev.append(put(torch, eng, d.reshape(-1)[first:first + n]))
    c = torch.from_numpy(np.array(cls).reshape(-1)[first:first + n]).to(eng._dev())
    out = grid.run(c, dev, coarse=names, first_pixel=first)
    eng.check()
    res = [o.cpu().numpy() for o in out]
    grid.close()
    return res


@pytest.mark.parametrize('exact', [False, True])
@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', ['nearest', 'bilinear', 'cos4'])
def test_same_bits_as_the_step_on_materialised_drivers(env, method, wrap, exact):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine('float64', exact)
    for names in (ds.MET_DRIVERS, MIX, ()):
        drivers = pick(ds, fine, coarse, names)
        got = run_grid(torch, ds, eng, cls, drivers, names, row_pos, col_pos, wrap, method)
        want = run_step(torch, eng, cls, materialise(ds, drivers, names, row_pos, col_pos, wrap, method))
        for g, w, what in zip(got, want, ('day', 'night')):
            assert g.shape == (N,) and g.dtype == np.float64
            assert parity.same_bits(g, w), '%s %s wrap=%s exact=%s coarse=%d' % (what, method, wrap, exact, len(names))
        assert 0.9 < np.isfinite(want[0]).mean() < 1.0          # both kinds of pixel take part


def test_all_fourteen_coarse_and_the_default(env):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine()
    got = run_grid(torch, ds, eng, cls, list(coarse), ds.DRIVER_NAMES, row_pos, col_pos, True, 'cos4')
    want = run_step(torch, eng, cls, materialise(ds, list(coarse), ds.DRIVER_NAMES, row_pos, col_pos, True, 'cos4'))
    assert parity.same_bits(got[0], want[0]) and parity.same_bits(got[1], want[1])
    # coarse= defaults to the eleven reanalysis drivers
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos)
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    dev = [put(torch, eng, d if name in ds.MET_DRIVERS else d.reshape(-1)) for name, d in zip(ds.DRIVER_NAMES, drivers)]
    day, night = grid.run(torch.from_numpy(np.array(cls)).to(eng._dev()).reshape(-1), dev)
    eng.check()
    want = run_step(torch, eng, cls, materialise(ds, drivers, ds.MET_DRIVERS, row_pos, col_pos, False, 'bilinear'))
    assert parity.same_bits(day.cpu().numpy(), want[0]) and parity.same_bits(night.cpu().numpy(), want[1])


@pytest.mark.parametrize('method', ['nearest', 'bilinear', 'cos4'])
def test_fields_equal_the_definition_in_a_pitched_output(env, method):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine()
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=True, method=method)
    planes = [np.array(coarse[k]) for k in (5, 9, 11)]
    planes[1][2, 3] = np.nan
    planes[2][0, 6] = np.inf
    rt, ct = ds.corner_tables(row_pos, H, False, method), ds.corner_tables(col_pos, W, True, method)
    want = np.stack([ds.interpolate(p, rt, ct).reshape(-1) for p in planes])
    first, n, pitch, poison = 100, 1500, 1500 + 37, -7.0
    buf = torch.full((3, pitch), poison, dtype=eng.dtype, device=eng._dev())
    out = grid.fields([put(torch, eng, p) for p in planes], first_pixel=first, n=n, out=buf[:, :n])
    eng.check()
    assert out.data_ptr() == buf.data_ptr()
    assert parity.same_bits(buf[:, :n].cpu().numpy(), want[:, first:first + n])
    assert (buf[:, n:] == poison).all()
    whole = grid.fields([put(torch, eng, p) for p in planes])
    eng.check()
    assert tuple(whole.shape) == (3, N) and parity.same_bits(whole.cpu().numpy(), want)
    assert np.isnan(want[1]).any() and np.isinf(want[2]).any()


def test_float32_engine_rounds_once(env):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    narrow = lambda arrays: [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    widen = lambda arrays: [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in arrays]
    for names in (ds.MET_DRIVERS, MIX):
        drivers = narrow(pick(ds, fine, coarse, names))
        got = run_grid(torch, ds, engine('float32'), cls, drivers, names, row_pos, col_pos, True, 'cos4')
        wide = run_step(torch, engine(), cls, materialise(ds, widen(drivers), names, row_pos, col_pos, True, 'cos4'))
        for g, w in zip(got, wide):
            assert g.dtype == np.float32
            with np.errstate(all='ignore'):
                assert parity.same_bits(g, w.astype(np.float32))
    # fields: the float64 interpolant, rounded once
    eng = engine('float32')
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, method='cos4')
    plane = coarse[5].astype(np.float32)
    got = grid.fields([put(torch, eng, plane)])
    eng.check()
    want = ds.interpolate(plane, ds.corner_tables(row_pos, H, False, 'cos4'), ds.corner_tables(col_pos, W, False, 'cos4'))
    assert got.dtype == torch.float32 and parity.same_bits(got.cpu().numpy()[0], want.reshape(-1).astype(np.float32))


@pytest.mark.parametrize('method', ['nearest', 'bilinear', 'cos4'])
def test_against_the_numpy_oracle(env, method):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    got = run_grid(torch, ds, engine(), cls, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, method)
    dense = materialise(ds, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, method)
    bplut = {k: table()[:, j] for j, k in enumerate(oracle.PARAM_NAMES)}
    with np.errstate(all='ignore'):
        want = oracle.evapotranspiration_raster(bplut, cls, *dense)
    for g, w, what in zip(got, want, ('day', 'night')):
        err = parity.assert_parity(g, np.asarray(w, np.float64).reshape(-1), RTOL_FAST, '%s %s' % (method, what))
        print('%s %s: max rel err %.3e' % (method, what, err))
    assert RTOL_FAST <= parity.RTOL_NORTH_STAR


def test_nan_cells(env):
    """Fine rows and columns an eighth of a cell apart, every eighth one on a cell centre: a NaN in
    cell (2, 3) of pressure (which both periods read) is NaN exactly where the definition says -- where the cell has weight --
    and not at the pixels on the centres of its neighbours, where its weight is 0."""
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, _, _ = inputs()
    row_pos, col_pos = np.arange(R) * 0.125, np.arange(C) * 0.125
    cls = np.where(np.isin(cls, (0, 11)), 1, cls).astype(np.uint8)          # every class has parameters
    fine = [np.nan_to_num(f, nan=0.5) for f in fine]                         # no NaN but the planted one
    # bilinear / cos4: weight strictly inside (1, 3) x (2, 4) cells = rows 9 ... 23, columns 17 ... 31;
    # nearest (f >= 0.5 takes the far cell): [1.5, 2.5) x [2.5, 3.5) = rows 12 ... 19, columns 20 ... 27
    for method, box in (('bilinear', (9, 23, 17, 31)), ('cos4', (9, 23, 17, 31)), ('nearest', (12, 19, 20, 27))):
        drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
        drivers[11] = drivers[11].copy()
        drivers[11][2, 3] = np.nan
        got = run_grid(torch, ds, engine(), cls, drivers, ds.MET_DRIVERS, row_pos, col_pos, False, method)
        dense = materialise(ds, drivers, ds.MET_DRIVERS, row_pos, col_pos, False, method)
        want = np.isnan(dense[11])
        assert np.array_equal(np.isnan(got[0].reshape(R, C)), want), method
        assert np.array_equal(np.isnan(got[1].reshape(R, C)), want), method
        # pixel (16, 24) is the centre of cell (2, 3); (8, 24), (24, 24), (16, 16), (16, 32) those of its neighbours
        assert want[16, 24] and not (want[8, 24] or want[24, 24] or want[16, 16] or want[16, 32])
        rows, cols = np.flatnonzero(want.any(axis=1)), np.flatnonzero(want.any(axis=0))
        assert (rows.min(), rows.max(), cols.min(), cols.max()) == box, method
        assert want.sum() == (box[1] - box[0] + 1) * (box[3] - box[2] + 1)


def test_domain_guard(env):
    """A coarse temp_day cell above 1332 K (the value of tests/test_gpu_composite.py's domain-guard
    test): every pixel it has weight in leaves the domain of the fast arithmetic, goes through the
    kernel behind, and still has the bits of the guarded step on the materialised drivers."""
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    drivers[5] = drivers[5].copy()
    drivers[5][1, 2] = 1400.0
    drivers[11] = drivers[11].copy()
    drivers[11][4, 0] = -5.0                       # and a negative pressure in a corner cell
    eng = engine()
    # 'nearest' hands the planted values on as they are; 'bilinear' mixes them with their neighbours
    # (1400 K and 280 K: above 1332 K only close to the cell's centre, where these grids have no pixel)
    got = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    dense = materialise(ds, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    want = run_step(torch, eng, cls, dense)
    affected = ((dense[5] == 1400.0) | (dense[11] == -5.0)).reshape(-1)
    assert 20 < affected.sum() < N // 2
    for g, w in zip(got, want):
        assert parity.same_bits(g[affected], w[affected]) and parity.same_bits(g, w)
        assert not (g.view(np.uint64) == MARK64).any()
    again = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, again))
    # only the affected pixels changed
    base = run_grid(torch, ds, eng, cls, pick(ds, fine, coarse, ds.MET_DRIVERS), ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    assert parity.same_bits(got[0][~affected], base[0][~affected]) and not parity.same_bits(got[0], base[0])
    mixed = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, 'bilinear')
    smooth = run_step(torch, eng, cls, materialise(ds, drivers, ds.MET_DRIVERS, row_pos, col_pos, True, 'bilinear'))
    for g, w in zip(mixed, smooth):
        assert parity.same_bits(g, w) and not (g.view(np.uint64) == MARK64).any()
    # float32 storage: the same, and no mark either
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in drivers]
    g32 = run_grid(torch, ds, engine('float32'), cls, narrow, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    w64 = run_step(torch, eng, cls, materialise(ds, [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in narrow],
                                                ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest'))
    for g, w in zip(g32, w64):
        with np.errstate(all='ignore'):
            assert parity.same_bits(g, w.astype(np.float32))
        assert not (g.view(np.uint32) == MARK32).any()


@functools.lru_cache(maxsize=None)
def full_call():
    import torch
    from mod16_amd import downscale as ds
    cls, fine, coarse, row_pos, col_pos = inputs()
    out = run_grid(torch, ds, engine(), cls, pick(ds, fine, coarse, MIX), MIX, row_pos, col_pos, True, 'cos4')
    for o in out:
        o.setflags(write=False)
    return out


@pytest.mark.parametrize('first', [0, 53, 100])
def test_ranges_equal_slices_of_the_full_call(env, first):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    want = full_call()
    drivers = pick(ds, fine, coarse, MIX)
    for n in (0, 1, 255, 257, None):
        got = run_grid(torch, ds, engine(), cls, drivers, MIX, row_pos, col_pos, True, 'cos4', first=first, n=n)
        hi = N if n is None else first + n
        for g, w in zip(got, want):
            assert g.shape == (hi - first,) and parity.same_bits(g, w[first:hi]), (first, n)


def test_coarse_pitch_and_caller_outputs(env):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine()
    want = full_call()
    drivers = pick(ds, fine, coarse, MIX)
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=True, method='cos4')
    dev = []
    for name, d in zip(ds.DRIVER_NAMES, drivers):
        if name in MIX:
            buf = torch.full((H, W + 3), float('nan'), dtype=eng.dtype, device=eng._dev())
            view = buf[:, :W]
            view.copy_(put(torch, eng, d))
            assert view.stride() == (W + 3, 1) and not view.is_contiguous()
            dev.append(view)
        else:
            dev.append(put(torch, eng, d.reshape(-1)) if isinstance(d, np.ndarray) else d)
    c = torch.from_numpy(np.array(cls)).to(eng._dev()).reshape(-1)
    day = torch.full((N,), -7.0, dtype=eng.dtype, device=eng._dev())
    night = torch.full((N,), -7.0, dtype=eng.dtype, device=eng._dev())
    out = grid.run(c, dev, coarse=MIX, out_day=day, out_night=night)
    eng.check()
    assert out[0].data_ptr() == day.data_ptr() and out[1].data_ptr() == night.data_ptr()
    assert parity.same_bits(day.cpu().numpy(), want[0]) and parity.same_bits(night.cpu().numpy(), want[1])
    # the coarse drivers share one pitch
    mixed = list(dev)
    mixed[4] = put(torch, eng, drivers[4])
    with pytest.raises(ValueError, match='one distance between rows'):
        grid.run(c, mixed, coarse=MIX)
    with pytest.raises(ValueError, match='unit stride'):
        grid.fields([torch.zeros((H, 2 * W), dtype=eng.dtype, device=eng._dev())[:, ::2]])
    grid.close()
    with pytest.raises(ValueError, match='closed'):
        grid.run(c, dev, coarse=MIX)


def test_numpy_entry_point_equals_the_device_call(env):
    """evapotranspiration_downscaled stages the fine arrays in tiles of mod16_host_tile_pixels() = 2^21
    pixels, the smallest (and only) tile its HOST path cuts: a 2049 x 2049 raster is 2 tiles and 4097
    pixels of a third. The fine arrays repeat the 37 x 53 ones."""
    torch, mod16_amd, _lib, ds = env
    from mod16_amd import multi
    cls, fine, coarse, _, _ = inputs()
    BR = BC = 2049
    assert 2 * multi.host_tile() < BR * BC < 3 * multi.host_tile()
    big = lambda a: np.resize(a, (BR, BC))
    bcls = big(cls)
    drivers = [c if name in ds.MET_DRIVERS else big(f) for name, f, c in zip(ds.DRIVER_NAMES, fine, coarse)]
    row_pos = ds.positions(-0.2, (H - 0.6) / BR, BR, 0.0, 1.0)
    col_pos = ds.positions(-3.0, (W + 5.0) / BC, BC, 0.0, 1.0)
    day, night = mod16_amd.evapotranspiration_downscaled(table(), bcls, *drivers, row_pos, col_pos, wrap=True, method='cos4')
    assert day.shape == (BR, BC) and day.dtype == np.float64
    eng = engine()
    grid = eng.downscale_grid((BR, BC), (H, W), row_pos, col_pos, wrap=True, method='cos4')
    dev = [put(torch, eng, d if name in ds.MET_DRIVERS else d.reshape(-1)) for name, d in zip(ds.DRIVER_NAMES, drivers)]
    want = grid.run(torch.from_numpy(bcls).to(eng._dev()).reshape(-1), dev)
    eng.check()
    assert parity.same_bits(day.reshape(-1), want[0].cpu().numpy())
    assert parity.same_bits(night.reshape(-1), want[1].cpu().numpy())
    grid.close()


def test_numpy_entry_point_small_shapes_and_device_lists(env):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    want = full_call()
    drivers = pick(ds, fine, coarse, MIX)
    kw = dict(wrap=True, method='cos4', coarse=MIX)
    got = mod16_amd.evapotranspiration_downscaled(table(), cls, *drivers, row_pos, col_pos, **kw)
    assert got[0].shape == (R, C)
    assert parity.same_bits(got[0].reshape(-1), want[0]) and parity.same_bits(got[1].reshape(-1), want[1])
    # ranges of whole rows over a device list: the same bits, into the caller's arrays
    outs = [np.full((R, C), -7.0), np.full((R, C), -7.0)]
    res = mod16_amd.evapotranspiration_downscaled(table(), cls, *drivers, row_pos, col_pos, devices=[0, 0, 0], out=outs, **kw)
    assert res[0] is outs[0] and parity.same_bits(outs[0].reshape(-1), want[0]) and parity.same_bits(outs[1].reshape(-1), want[1])
    # float32 in, float32 out
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in drivers]
    g32 = mod16_amd.evapotranspiration_downscaled(table(), cls, *narrow, row_pos, col_pos, **kw)
    d32 = run_grid(torch, ds, engine('float32'), cls, narrow, MIX, row_pos, col_pos, True, 'cos4')
    assert g32[0].dtype == np.float32 and parity.same_bits(g32[0].reshape(-1), d32[0]) and parity.same_bits(g32[1].reshape(-1), d32[1])


def test_errors(env):
    torch, mod16_amd, _lib, ds = env
    from mod16_amd.raster import RasterEngine
    cls, fine, coarse, row_pos, col_pos = inputs()
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    bad = cls.copy()
    bad[R - 1, C - 2] = 13
    with pytest.raises(IndexError):
        run_grid(torch, ds, engine(), bad, drivers, ds.MET_DRIVERS, row_pos, col_pos)
    with pytest.raises(IndexError):
        mod16_amd.evapotranspiration_downscaled(table(), bad, *drivers, row_pos, col_pos)
    # the engine still works
    assert parity.same_bits(run_grid(torch, ds, engine(), cls, pick(ds, fine, coarse, MIX), MIX, row_pos, col_pos, True, 'cos4')[0],
                            full_call()[0])
    # the mixed-precision and the trusted forms are refused, by the engine and by the library
    for eng in (RasterEngine(table(), dtype='float32', math=_lib.MATH_MIXED), RasterEngine(table(), trusted=True)):
        grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos)
        with pytest.raises(ValueError, match='MATH_FAST or MATH_EXACT'):
            grid.run(None, [0.0] * 14)
    with pytest.raises(ValueError, match='MATH_FAST or MATH_EXACT'):
        mod16_amd.evapotranspiration_downscaled(table(), cls, *drivers, row_pos, col_pos, math=_lib.MATH_MIXED)
    eng = engine()
    low = _lib.Downscale(eng.ctx, (R, C), (H, W), row_pos, col_pos)
    one = torch.zeros(N, dtype=eng.dtype, device=eng._dev())
    c = torch.zeros(N, dtype=torch.uint8, device=eng._dev())
    args = (eng.np_dtype, c.data_ptr(), [one.data_ptr()] * 14, [1] * 14, W, 0, N, one.data_ptr(), one.data_ptr())
    for flags, what in ((_lib.MATH_MIXED, 'MOD16_MATH_MIXED is not available'), (_lib.DOMAIN_TRUSTED, 'MOD16_DOMAIN_TRUSTED is not available')):
        with pytest.raises(_lib.Mod16Error, match=what):
            low.run(*args, flags=flags, where=_lib.DEVICE)
    with pytest.raises(_lib.Mod16Error, match='leaves the raster'):
        low.run(*(args[:5] + (1, N) + args[7:]), where=_lib.DEVICE)
    with pytest.raises(_lib.Mod16Error, match='coarse_pitch'):
        low.run(*(args[:3] + ([2] * 14, W - 1) + args[5:]), where=_lib.DEVICE)
    with pytest.raises(_lib.Mod16Error, match='kind'):
        low.run(*(args[:3] + ([3] * 14,) + args[4:]), where=_lib.DEVICE)
    low.close()
    # a wrong coarse shape is refused before any device work
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos)
    dev = [put(torch, eng, d if name in ds.MET_DRIVERS else d.reshape(-1)) if isinstance(d, np.ndarray) else d
           for name, d in zip(ds.DRIVER_NAMES, drivers)]
    dev[5] = torch.zeros((W, H), dtype=eng.dtype, device=eng._dev())
    cdev = torch.from_numpy(np.array(cls)).to(eng._dev()).reshape(-1)
    with pytest.raises(ValueError, match='coarse driver'):
        grid.run(cdev, dev)
    wrong = list(drivers)
    wrong[0] = np.zeros((H + 1, W))
    with pytest.raises(ValueError, match='coarse driver'):
        mod16_amd.evapotranspiration_downscaled(table(), cls, *wrong, row_pos, col_pos)
    with pytest.raises(ValueError, match='row_pos has shape'):
        eng.downscale_grid((R, C), (H, W), row_pos[:-1], col_pos)
    with pytest.raises(ValueError, match='not finite'):
        eng.downscale_grid((R, C), (H, W), np.where(np.arange(R) == 3, np.nan, row_pos), col_pos)
    with pytest.raises(ValueError, match='method'):
        eng.downscale_grid((R, C), (H, W), row_pos, col_pos, method='cubic')
    # the library validates tables it is handed: an index outside the coarse grid never reaches a kernel
    spec = _lib.DownscaleSpec(R, C, H, W, 0, 1)
    rt = ds.check_tables(ds.corner_tables(row_pos, H), R, H, 'row')
    ct = ds.check_tables(ds.corner_tables(col_pos, W), C, W, 'column')
    far = rt[1].copy()
    far[7] = H
    import ctypes
    handle = ctypes.c_void_p()
    rc = eng.ctx.lib.mod16_downscale_create_tables(eng.ctx.handle, ctypes.byref(spec), rt[0].ctypes.data, far.ctypes.data,
                                                   rt[2].ctypes.data, rt[3].ctypes.data, *[t.ctypes.data for t in ct],
                                                   ctypes.byref(handle))
    assert rc == _lib.ERR_ARG and not handle.value
    # the library's own tables (mod16_downscale_create) agree with numpy's where no cosine is involved
    pos_r, pos_c = np.ascontiguousarray(row_pos), np.ascontiguousarray(col_pos)
    eng.ctx.check(eng.ctx.lib.mod16_downscale_create(eng.ctx.handle, ctypes.byref(spec), pos_r.ctypes.data, pos_c.ctypes.data,
                                                     ctypes.byref(handle)))
    plane = put(torch, eng, coarse[5])
    out = torch.empty((1, N), dtype=eng.dtype, device=eng._dev())
    eng.ctx.check(eng.ctx.lib.mod16_downscale_fields_f64(eng.ctx.handle, handle, _lib.ptr_array([plane.data_ptr()]), 1, W, 0, N,
                                                         out.data_ptr(), N, _lib.DEVICE, eng._stream()))
    eng.check()
    eng.ctx.lib.mod16_downscale_destroy(handle)
    assert parity.same_bits(out.cpu().numpy()[0], ds.interpolate(coarse[5], rt, ct).reshape(-1))
