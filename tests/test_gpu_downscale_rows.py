"""GPU tests of the row-affine column geometry of the downscaled families (sinusoidal tiles:
RasterEngine.downscale_grid(..., col_affine=(col_origin, col_scale)), the numpy entry points'
col_affine): the column cell pair and its weights are formed per pixel inside the kernels, and
everything is held, bit for bit, to the numpy definition mod16_amd.downscale (corner_tables_rows,
interpolate_rows) -- for ET, to RasterEngine.run / .composite on the drivers it materialises.

Shapes and inputs are those of tests/test_gpu_downscale.py (fine 37 x 53 = 1961 pixels: eight batches
of 256 that each span several rows, the last one ragged; coarse 5 x 7; fine inputs from oracle.synth
with its special values, coarse without; row_pos = positions(-0.8, 0.17, 37, 0, 1)) and, for the
composite, of tests/test_gpu_composite_downscale.py (K = 19 days in periods of 8).

Two column geometries from lat = linspace(70, -70, 37) degrees, scale = base / cos(lat), origin =
3.0 - scale * 26 -- but row 5 with scale 0 (a whole row on one cell centre), row 6 with its scale
negated (columns running east to west) and row 7 with scale 0.5 from origin -2.0 (exact cell centres
and exact halves: the tie of 'nearest'):
  narrow  base 0.09, used without wrap: positions -3.8 ... 24, 15 % of the pixels outside [0, W - 1]
  wide    base 0.41, used with wrap: positions -28 ... 34, ten different wrap counts
test_the_geometries_are_what_they_claim asserts these as conditions on the inputs.

Tolerance against the oracle: 1e-8 relative, what tests/test_gpu_parity.py holds the FAST float64
step kernel to (RTOL['fast']) -- the oracle runs on the drivers the numpy definition materialises,
so the interpolation adds nothing to it. Everything else is equality of bits."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import mod16_oracle as oracle
import parity
import test_gpu_downscale as base
import test_gpu_composite_downscale as cbase

pytestmark = pytest.mark.gpu

R, C, H, W, N = base.R, base.C, base.H, base.W, base.N
RTOL_FAST = 1e-8                     # tests/test_gpu_parity.py: RTOL['fast']
MARK64 = base.MARK64
MIX = base.MIX
METHODS = ('nearest', 'bilinear')
engine, table, put, pick, run_step = base.engine, base.table, base.put, base.pick, base.run_step


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    from mod16_amd import downscale as ds
    return torch, mod16_amd, _lib, ds


@functools.lru_cache(maxsize=None)
def geometry(wrap):
    """(col_origin, col_scale): the wide geometry for wrap, the narrow one without; read-only."""
    lat = np.radians(np.linspace(70.0, -70.0, R))
    scale = (0.41 if wrap else 0.09) / np.cos(lat)
    scale[5] = 0.0
    scale[6] = -scale[6]
    origin = 3.0 - scale * 26
    scale[7], origin[7] = 0.5, -2.0
    origin.setflags(write=False)
    scale.setflags(write=False)
    return origin, scale


def inputs():
    cls, fine, coarse, row_pos, _ = base.inputs()
    return cls, fine, coarse, row_pos


@functools.lru_cache(maxsize=None)
def tables(wrap, method):
    from mod16_amd import downscale as ds
    row_pos = base.inputs()[3]
    origin, scale = geometry(wrap)
    return ds.corner_tables(row_pos, H, False, method), ds.corner_tables_rows(origin, scale, C, W, wrap, method)


def materialise(ds, drivers, names, wrap, method):
    """Every coarse driver on the fine grid, by the numpy definition."""
    rt, ct = tables(wrap, method)
    return [ds.interpolate_rows(d, rt, ct) if name in names else d for name, d in zip(ds.DRIVER_NAMES, drivers)]


def run_grid(torch, ds, eng, cls, drivers, names, row_pos, wrap=False, method='bilinear', first=0, n=None, **geo):
    """DownscaleGrid.run of a row-affine grid on numpy inputs, pixels [first, first + n) -> numpy (day, night);
    `geo`: col_pos=... for the rectilinear grid instead."""
    n = N - first if n is None else n
    if not geo:
        geo = dict(col_affine=geometry(wrap))
    grid = eng.downscale_grid((R, C), (H, W), row_pos, wrap=wrap, method=method, **geo)
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


def test_the_geometries_are_what_they_claim(env):
    torch, mod16_amd, _lib, ds = env
    narrow = ds.column_positions(*geometry(False), C)
    wide = ds.column_positions(*geometry(True), C)
    assert ((narrow < 0) | (narrow > W - 1)).mean() < 0.5          # most narrow pixels interpolate inside the grid
    assert ((narrow < 0) | (narrow > W - 1)).any()
    assert len(np.unique(np.floor(wide / W))) >= 5                  # several wrap counts, both signs
    assert wide.min() < -W and wide.max() > 2 * W
    for pos in (narrow, wide):
        f = pos - np.floor(pos)
        assert (f == 0).any() and (f == 0.5).any()                  # exact centres, the tie of 'nearest'
    assert np.all(narrow[5] == 3.0) and narrow[6, 0] > narrow[6, -1] and narrow[7, 10] == 3.0 and narrow[7, 11] == 3.5


@pytest.mark.parametrize('exact', [False, True])
@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_same_bits_as_the_step_on_materialised_drivers(env, method, wrap, exact):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    eng = engine('float64', exact)
    for names in (ds.MET_DRIVERS, MIX, ()):
        drivers = pick(ds, fine, coarse, names)
        got = run_grid(torch, ds, eng, cls, drivers, names, row_pos, wrap, method)
        want = run_step(torch, eng, cls, materialise(ds, drivers, names, wrap, method))
        for g, w, what in zip(got, want, ('day', 'night')):
            assert g.shape == (N,) and g.dtype == np.float64
            assert parity.same_bits(g, w), '%s %s wrap=%s exact=%s coarse=%d' % (what, method, wrap, exact, len(names))
        assert 0.9 < np.isfinite(want[0]).mean() < 1.0          # both kinds of pixel take part


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_constant_dyadic_affine_equals_the_rectilinear_grid(env, method, wrap):
    """origin -9.25 and scale 0.375 in every row (origin + scale * c is exact): run and fields have the
    bits of the rectilinear grid with col_pos = -9.25 + 0.375 * arange(53)."""
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    eng = engine()
    affine = (np.full(R, -9.25), np.full(R, 0.375))
    col_pos = -9.25 + 0.375 * np.arange(C)
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    got = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, wrap, method, col_affine=affine)
    want = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, wrap, method, col_pos=col_pos)
    assert parity.same_bits(got[0], want[0]) and parity.same_bits(got[1], want[1])
    planes = [put(torch, eng, coarse[k]) for k in (5, 9, 11)]
    ga = eng.downscale_grid((R, C), (H, W), row_pos, wrap=wrap, method=method, col_affine=affine)
    gr = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=wrap, method=method)
    assert ga.col_tables is None and ga.col_affine is not None and gr.col_affine is None
    a, b = ga.fields(planes), gr.fields(planes)
    eng.check()
    assert parity.same_bits(a.cpu().numpy(), b.cpu().numpy())
    ga.close()
    gr.close()


@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_fields_equal_the_definition_in_a_pitched_output(env, method, wrap):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    eng = engine()
    grid = eng.downscale_grid((R, C), (H, W), row_pos, wrap=wrap, method=method, col_affine=geometry(wrap))
    planes = [np.array(coarse[k]) for k in (5, 9, 11)]
    planes[1][2, 3] = np.nan
    planes[2][0, 6] = np.inf
    rt, ct = tables(wrap, method)
    want = np.stack([ds.interpolate_rows(p, rt, ct).reshape(-1) for p in planes])
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
    grid.close()


def test_float32_engine_rounds_once(env):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    narrow = lambda arrays: [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    widen = lambda arrays: [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in arrays]
    for names in (ds.MET_DRIVERS, MIX):
        drivers = narrow(pick(ds, fine, coarse, names))
        got = run_grid(torch, ds, engine('float32'), cls, drivers, names, row_pos, True, 'bilinear')
        wide = run_step(torch, engine(), cls, materialise(ds, widen(drivers), names, True, 'bilinear'))
        for g, w in zip(got, wide):
            assert g.dtype == np.float32
            with np.errstate(all='ignore'):
                assert parity.same_bits(g, w.astype(np.float32))
    # fields: the float64 interpolant, rounded once
    eng = engine('float32')
    for wrap in (False, True):
        grid = eng.downscale_grid((R, C), (H, W), row_pos, wrap=wrap, col_affine=geometry(wrap))
        plane = coarse[5].astype(np.float32)
        got = grid.fields([put(torch, eng, plane)])
        eng.check()
        want = ds.interpolate_rows(plane, *tables(wrap, 'bilinear'))
        assert got.dtype == torch.float32 and parity.same_bits(got.cpu().numpy()[0], want.reshape(-1).astype(np.float32))
        grid.close()


@pytest.mark.parametrize('method', METHODS)
def test_against_the_numpy_oracle(env, method):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    got = run_grid(torch, ds, engine(), cls, drivers, ds.MET_DRIVERS, row_pos, True, method)
    dense = materialise(ds, drivers, ds.MET_DRIVERS, True, method)
    bplut = {k: table()[:, j] for j, k in enumerate(oracle.PARAM_NAMES)}
    with np.errstate(all='ignore'):
        want = oracle.evapotranspiration_raster(bplut, cls, *dense)
    for g, w, what in zip(got, want, ('day', 'night')):
        err = parity.assert_parity(g, np.asarray(w, np.float64).reshape(-1), RTOL_FAST, '%s %s' % (method, what))
        print('%s %s: max rel err %.3e' % (method, what, err))
    assert RTOL_FAST <= parity.RTOL_NORTH_STAR


@pytest.mark.parametrize('method', METHODS)
def test_nan_cell(env, method):
    """A NaN in cell (0, 4) of pressure is NaN exactly where interpolate_rows says -- where the cell has
    weight. Row 5 sits on the centre of column 3 throughout and row 7 on a centre at every even column
    (column 4's at c = 12, its neighbours' at c = 10 and c = 14): the pixels on a neighbour's centre
    are clean."""
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    cls = np.where(np.isin(cls, (0, 11)), 1, cls).astype(np.uint8)          # every class has parameters
    fine = [np.nan_to_num(f, nan=0.5) for f in fine]                         # no NaN but the planted one
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    drivers[11] = drivers[11].copy()
    drivers[11][0, 4] = np.nan
    got = run_grid(torch, ds, engine(), cls, drivers, ds.MET_DRIVERS, row_pos, False, method)
    want = np.isnan(materialise(ds, drivers, ds.MET_DRIVERS, False, method)[11])
    assert np.array_equal(np.isnan(got[0].reshape(R, C)), want)
    assert np.array_equal(np.isnan(got[1].reshape(R, C)), want)
    assert not want[5].any()
    assert want[7, 12] and want[7, 11] and not (want[7, 10] or want[7, 14] or want[7, 8])
    assert 10 < want.sum() < N // 2


def test_domain_guard(env):
    """A coarse temp_day cell above 1332 K: every pixel it has weight in leaves the domain of the fast
    arithmetic, goes through the kernel behind, and still has the bits of the guarded step (the EXACT
    arithmetic there) on the materialised drivers; no output keeps the mark."""
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    drivers = pick(ds, fine, coarse, ds.MET_DRIVERS)
    drivers[5] = drivers[5].copy()
    drivers[5][1, 2] = 1400.0
    eng = engine()
    got = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, True, 'nearest')
    dense = materialise(ds, drivers, ds.MET_DRIVERS, True, 'nearest')
    want = run_step(torch, eng, cls, dense)
    exact = run_step(torch, engine('float64', True), cls, dense)
    affected = (dense[5] == 1400.0).reshape(-1)
    assert 0 < affected.sum() < N // 2
    for g, w, e in zip(got, want, exact):
        assert parity.same_bits(g, w) and parity.same_bits(g[affected], e[affected])
        assert not (g.view(np.uint64) == MARK64).any()
    again = run_grid(torch, ds, eng, cls, drivers, ds.MET_DRIVERS, row_pos, True, 'nearest')
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, again))


@functools.lru_cache(maxsize=None)
def full_call():
    import torch
    from mod16_amd import downscale as ds
    cls, fine, coarse, row_pos = inputs()
    eng = engine()
    out = run_grid(torch, ds, eng, cls, pick(ds, fine, coarse, MIX), MIX, row_pos, True, 'bilinear')
    grid = eng.downscale_grid((R, C), (H, W), row_pos, wrap=True, col_affine=geometry(True))
    fields = grid.fields([put(torch, eng, coarse[k]) for k in (5, 11)])
    eng.check()
    out = list(out) + [fields.cpu().numpy()]
    grid.close()
    for o in out:
        o.setflags(write=False)
    return out


@pytest.mark.parametrize('first', [0, 1, 53 * 7 + 11, N - 1])
def test_ranges_equal_slices_of_the_full_call(env, first):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    day, night, fields = full_call()
    drivers = pick(ds, fine, coarse, MIX)
    eng = engine()
    grid = eng.downscale_grid((R, C), (H, W), row_pos, wrap=True, col_affine=geometry(True))
    planes = [put(torch, eng, coarse[k]) for k in (5, 11)]
    for n in (0, 1, 255, 257, None):
        if n is not None and first + n > N:
            continue
        got = run_grid(torch, ds, eng, cls, drivers, MIX, row_pos, True, 'bilinear', first=first, n=n)
        hi = N if n is None else first + n
        for g, w in zip(got, (day, night)):
            assert g.shape == (hi - first,) and parity.same_bits(g, w[first:hi]), (first, n)
        f = grid.fields(planes, first_pixel=first, n=n)
        eng.check()
        assert parity.same_bits(f.cpu().numpy(), np.ascontiguousarray(fields[:, first:hi])), (first, n)
    grid.close()


# ---- the composite (shapes of tests/test_gpu_composite_downscale.py)

def materialise_series(cp, ds, arrays, names, wrap, method):
    rt, ct = tables(wrap, method)
    out = []
    for name, a in zip(cp.ARRAY_NAMES, arrays):
        if name not in names:
            out.append(a)
        elif a.ndim == 2:
            out.append(ds.interpolate_rows(a, rt, ct).reshape(-1))
        else:
            out.append(np.stack([ds.interpolate_rows(p, rt, ct).reshape(-1) for p in a]))
    return out


def run_composite(torch, cp, eng, cls, arrays, names, row_pos, wrap, method, first=0, n=None, **kw):
    n = N - first if n is None else n
    grid = eng.downscale_grid((R, C), (H, W), row_pos, wrap=wrap, method=method, col_affine=geometry(wrap))
    dev = cbase.device_arrays(torch, cp, eng, arrays, names, first, n)
    c = torch.from_numpy(np.array(cls)[first:first + n]).to(eng._dev())
    out = grid.composite(c, dev[:14], dev[14], cbase.K, cbase.L, coarse=names, first_pixel=first, every=cbase.EVERY, **kw)
    eng.check()
    res = cbase.to_numpy(torch, out)
    grid.close()
    return res


@pytest.mark.parametrize('pet', [False, True])
@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', METHODS)
def test_composite_same_bits_as_the_composite_on_materialised_slabs(env, method, wrap, pet):
    torch, mod16_amd, _lib, ds = env
    from mod16_amd import composite as cp
    cls, fine, coarse, row_pos, _ = cbase.inputs()
    eng = cbase.engine()
    for key in ('met', 'mix'):
        names = cbase.names_of(ds, key)
        arrays = cbase.pick(cp, fine, coarse, names)
        got = run_composite(torch, cp, eng, cls, arrays, names, row_pos, wrap, method, pet=pet)
        dense = materialise_series(cp, ds, arrays, names, wrap, method)
        want = cbase.run_reference(torch, eng, cls, dense, pet=pet)
        assert got[0].shape == (cbase.P, N) and got[0].dtype == np.float64
        cbase.same_results(got, want, '%s %s wrap=%s pet=%s' % (key, method, wrap, pet))
        assert 0.9 < np.isfinite(want[0]).mean() < 1.0
    # a range that starts inside a row and ends inside another
    first, n = 53 * 7 + 11, 700
    part = run_composite(torch, cp, eng, cls, arrays, names, row_pos, wrap, method, first=first, n=n, pet=pet)
    cbase.same_results(part, [np.ascontiguousarray(w[:, first:first + n]) for w in want], 'range')


def test_composite_exact_engine_and_float32(env):
    torch, mod16_amd, _lib, ds = env
    from mod16_amd import composite as cp
    cls, fine, coarse, row_pos, _ = cbase.inputs()
    names = cbase.names_of(ds, 'mix')
    arrays = cbase.pick(cp, fine, coarse, names)
    eng = cbase.engine('float64', True)
    got = run_composite(torch, cp, eng, cls, arrays, names, row_pos, True, 'bilinear', pet=True)
    want = cbase.run_reference(torch, eng, cls, materialise_series(cp, ds, arrays, names, True, 'bilinear'), pet=True)
    cbase.same_results(got, want, 'exact')
    e32 = cbase.engine('float32')
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    got = run_composite(torch, cp, e32, cls, narrow, names, row_pos, False, 'nearest')
    wide = [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in narrow]
    dense = [a.astype(np.float32) if isinstance(a, np.ndarray) else a
             for a in materialise_series(cp, ds, wide, names, False, 'nearest')]
    # 'nearest' hands float32 cells on unchanged, so the float32 composite on them is the reference
    want = cbase.run_reference(torch, e32, cls, dense)
    cbase.same_results(got, want, 'float32 nearest')


# ---- the numpy entry points

def test_numpy_entry_points_equal_the_device_calls(env):
    torch, mod16_amd, _lib, ds = env
    from mod16_amd import composite as cp
    cls, fine, coarse, row_pos = inputs()
    day, night, _ = full_call()
    drivers = pick(ds, fine, coarse, MIX)
    kw = dict(wrap=True, method='bilinear', coarse=MIX, col_affine=geometry(True))
    got = mod16_amd.evapotranspiration_downscaled(table(), cls, *drivers, row_pos, None, **kw)
    assert got[0].shape == (R, C)
    assert parity.same_bits(got[0].reshape(-1), day) and parity.same_bits(got[1].reshape(-1), night)
    two = mod16_amd.evapotranspiration_downscaled(table(), cls, *drivers, row_pos, None, devices=[0, 0], **kw)
    assert parity.same_bits(two[0], got[0]) and parity.same_bits(two[1], got[1])
    with pytest.raises(ValueError, match='exactly one'):
        mod16_amd.evapotranspiration_downscaled(table(), cls, *drivers, row_pos, np.zeros(C), **kw)
    # the composite
    ccls, cfine, ccoarse, crow, _ = cbase.inputs()
    names = cbase.names_of(ds, 'mix')
    arrays = cbase.pick(cp, cfine, ccoarse, names)
    want = run_composite(torch, cp, cbase.engine(), ccls, arrays, names, crow, True, 'bilinear', pet=True)
    host = [a if not isinstance(a, np.ndarray) or name in names else a.reshape(a.shape[:-1] + (R, C))
            for name, a in zip(cp.ARRAY_NAMES, arrays)]
    res = mod16_amd.evapotranspiration_composite_downscaled(
        table(), ccls.reshape(R, C), *host, crow, None, days=cbase.K, period_days=cbase.L, every=cbase.EVERY,
        wrap=True, method='bilinear', coarse=names, pet=True, col_affine=geometry(True))
    cbase.same_results([np.asarray(r).reshape(cbase.P, N) for r in res], want, 'numpy entry point')


# ---- a sinusoidal tile end to end, small

@pytest.mark.parametrize('tile', [(0, 8), (18, 0)])
def test_sinusoidal_tile_fields(env, tile):
    """48 x 48 pixels of tile (0, 8) (an edge tile whose western pixels lie beyond the globe's outline and
    wrap) and of tile (18, 0) (polar: huge finite scales, many turns around the globe per row) over a
    361 x 576 plane with wrap: fields equals interpolate_rows, 2304 pixels each."""
    torch, mod16_amd, _lib, ds = env
    size, HH, WW = 48, 361, 576
    row_pos, origin, scale = ds.sinusoidal_positions(tile[0], tile[1], size, 90.0, -0.5, -180.0, 0.625)
    pos = ds.column_positions(origin, scale, size)
    if tile == (0, 8):
        assert (pos < 0).any() and (pos >= 0).any()              # some pixels west of 180 W: they wrap
    else:
        assert np.abs(scale).max() > 100 and len(np.unique(np.floor(pos / WW))) > 10
    rng = np.random.default_rng(17)
    planes = [rng.normal(size=(HH, WW)), rng.uniform(200.0, 320.0, (HH, WW))]
    eng = engine()
    for method in METHODS:
        grid = eng.downscale_grid((size, size), (HH, WW), row_pos, wrap=True, method=method, col_affine=(origin, scale))
        got = grid.fields([put(torch, eng, p) for p in planes])
        eng.check()
        rt = ds.corner_tables(row_pos, HH, False, method)
        ct = ds.corner_tables_rows(origin, scale, size, WW, True, method)
        want = np.stack([ds.interpolate_rows(p, rt, ct).reshape(-1) for p in planes])
        assert tuple(got.shape) == (2, size * size) and parity.same_bits(got.cpu().numpy(), want), method
        grid.close()


def test_errors(env):
    torch, mod16_amd, _lib, ds = env
    cls, fine, coarse, row_pos = inputs()
    origin, scale = geometry(False)
    eng = engine()
    with pytest.raises(ValueError, match='cos4'):
        eng.downscale_grid((R, C), (H, W), row_pos, method='cos4', col_affine=(origin, scale))
    with pytest.raises(ValueError, match='exactly one'):
        eng.downscale_grid((R, C), (H, W), row_pos, np.zeros(C), col_affine=(origin, scale))
    with pytest.raises(ValueError, match='exactly one'):
        eng.downscale_grid((R, C), (H, W), row_pos)
    for o, s in ((np.where(np.arange(R) == 3, np.nan, origin), scale), (origin, np.where(np.arange(R) == 3, np.inf, scale)),
                 (origin, np.where(np.arange(R) == 3, 1e307, scale))):
        with pytest.raises(ValueError, match='not finite'):
            eng.downscale_grid((R, C), (H, W), row_pos, col_affine=(o, s))
    # the library validates what it is handed, before any launch: cos4, non-finite geometry
    rt = ds.check_tables(ds.corner_tables(row_pos, H), R, H, 'row')
    o, s = np.ascontiguousarray(origin), np.ascontiguousarray(scale)
    lib, handle = eng.ctx.lib, ctypes.c_void_p()

    def create(spec, o, s):
        return lib.mod16_downscale_create_rows_tables(eng.ctx.handle, ctypes.byref(spec), *[t.ctypes.data for t in rt],
                                                      o.ctypes.data, s.ctypes.data, ctypes.byref(handle))
    assert create(_lib.DownscaleSpec(R, C, H, W, 0, 2), o, s) == _lib.ERR_ARG and not handle.value
    bad = s.copy()
    bad[R - 1] = 1e307
    assert create(_lib.DownscaleSpec(R, C, H, W, 1, 1), o, bad) == _lib.ERR_ARG and not handle.value
    bad = o.copy()
    bad[0] = np.nan
    assert create(_lib.DownscaleSpec(R, C, H, W, 1, 1), bad, s) == _lib.ERR_ARG and not handle.value
    with pytest.raises(_lib.Mod16Error, match='mod16_downscale_create: .*not finite'):
        eng.ctx.check(create(_lib.DownscaleSpec(R, C, H, W, 1, 1), bad, s))
    # the library's own row tables (mod16_downscale_create_rows) agree with numpy's
    pos_r = np.ascontiguousarray(row_pos)
    eng.ctx.check(lib.mod16_downscale_create_rows(eng.ctx.handle, ctypes.byref(_lib.DownscaleSpec(R, C, H, W, 0, 1)),
                                                  pos_r.ctypes.data, o.ctypes.data, s.ctypes.data, ctypes.byref(handle)))
    plane = put(torch, eng, coarse[5])
    out = torch.empty((1, N), dtype=eng.dtype, device=eng._dev())
    eng.ctx.check(lib.mod16_downscale_fields_f64(eng.ctx.handle, handle, _lib.ptr_array([plane.data_ptr()]), 1, W, 0, N,
                                                 out.data_ptr(), N, _lib.DEVICE, eng._stream()))
    eng.check()
    lib.mod16_downscale_destroy(handle)
    assert parity.same_bits(out.cpu().numpy()[0], ds.interpolate_rows(coarse[5], *tables(False, 'bilinear')).reshape(-1))
    # a grid of another engine refuses this engine's tensors; a closed grid refuses everything
    other = engine('float32').downscale_grid((R, C), (H, W), row_pos, col_affine=(origin, scale))
    with pytest.raises(TypeError, match='float32'):
        other.fields([plane])
    other.close()
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_affine=(origin, scale))
    grid.close()
    with pytest.raises(ValueError, match='closed'):
        grid.fields([plane])
    c = torch.zeros(N, dtype=torch.uint8, device=eng._dev())
    with pytest.raises(ValueError, match='closed'):
        grid.run(c, [0.0] * 14, coarse=())
