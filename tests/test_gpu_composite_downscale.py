"""GPU tests of the composite over coarse drivers (mod16_et_composite_downscaled_*:
DownscaleGrid.composite, mod16_amd.evapotranspiration_composite_downscaled) against what it replaces --
every coarse array blown up to the fine grid slab by slab by the numpy definition
(mod16_amd.downscale.interpolate), then RasterEngine.composite -- bit for bit, counts included, and
against the numpy oracle per day.

Shapes: fine grid 37 x 53 (n = 1961: eight batches of 256 pixels, each spanning several rows, a
ragged last one) over a coarse grid 5 x 7, the position tables of tests/test_gpu_downscale.py (held
edges, three wraps of the columns); K = 19 days in periods of L = 8 (8, 8 and 3 days), albedo, fPAR
and LAI in 3 eight-day slabs. Fine data from oracle.synth with its special values; the coarse series
one oracle.synth draw per day, without; temp_annual a coarse (H, W) constant.

Tolerance against the oracle: 1e-8 relative, what tests/test_gpu_composite.py and
tests/test_gpu_parity.py hold the FAST float64 arithmetic to -- the oracle runs on the arrays the
numpy definition materialises, so the interpolation adds nothing to it."""
import functools

import numpy as np
import pytest

from oracle import mod16_oracle as oracle
from oracle import synth
import parity

pytestmark = pytest.mark.gpu

R, C, H, W = 37, 53, 5, 7
N = R * C
K, L, P = 19, 8, 3
EVERY = {'sw_albedo': 8, 'fpar': 8, 'lai': 8}
RTOL_FAST = 1e-8                     # tests/test_gpu_parity.py: RTOL['fast']
MARK64 = 0x7ff80000000c0351          # CompMark<double>, csrc/mod16_composite.hpp
MARK32 = 0x7fcc0351
MIX = ('sw_albedo', 'temp_day', 'vpd_day', 'pressure', 'lai', 'day_hours')
SETS = {'met': None, 'mix': MIX, 'none': ()}          # None: downscale.MET_DRIVERS


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    from mod16_amd import composite as cp
    from mod16_amd import downscale as ds
    return torch, mod16_amd, _lib, cp, ds


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


def slabs_of(name):
    return -(-K // EVERY.get(name, 1))


@functools.lru_cache(maxsize=None)
def inputs(seed=71):
    """(cls (N,), the 15 arrays on the fine grid, the 15 on the coarse grid, row_pos, col_pos): numpy,
    read-only. Fine: (S, N) per array, albedo / fPAR / LAI and the classes with synth's special values;
    coarse: (S, H, W), one draw per day; temp_annual constant on both grids; the hours uniform in 6 ... 18."""
    from mod16_amd import composite as cp
    from mod16_amd import downscale as ds
    cls3, slow = synth.drivers((P, N), seed=seed, special=True)
    _, daily = synth.drivers((K, N), seed=seed + 1, special=False)
    days = [synth.drivers((H, W), seed=seed + 10 + t, special=False)[1] for t in range(K)]
    rng = np.random.default_rng(seed + 2)
    fine, coarse = [], []
    for k, name in enumerate(cp.ARRAY_NAMES):
        S = slabs_of(name)
        if name == 'day_hours':
            fine.append(rng.uniform(6, 18, (K, N)))
            coarse.append(rng.uniform(6, 18, (K, H, W)))
            continue
        fine.append(np.ascontiguousarray(slow[k]) if S == P else np.ascontiguousarray(daily[k]))
        coarse.append(np.stack([days[s * EVERY.get(name, 1)][k] for s in range(S)]))
    k = cp.ARRAY_NAMES.index('temp_annual')
    fine[k], coarse[k] = np.ascontiguousarray(fine[k][0]), np.ascontiguousarray(coarse[k][0])
    row_pos = ds.positions(-0.8, 0.17, R, 0.0, 1.0)
    col_pos = ds.positions(-9.3, 0.41, C, 0.0, 1.0)
    cls = np.ascontiguousarray(cls3[0])
    for a in [cls, row_pos, col_pos] + fine + coarse:
        a.setflags(write=False)
    return cls, tuple(fine), tuple(coarse), row_pos, col_pos


def names_of(ds, key):
    return ds.MET_DRIVERS if SETS[key] is None else SETS[key]


def pick(cp, fine, coarse, names):
    """The 15 arrays of a call whose coarse arrays are `names` (sw_rad_night a scalar unless coarse)."""
    out = [c if name in names else f for name, f, c in zip(cp.ARRAY_NAMES, fine, coarse)]
    if 'sw_rad_night' not in names:
        out[3] = 0.0
    return out


def materialise(cp, ds, arrays, names, row_pos, col_pos, wrap, method):
    """What the user did before: every coarse array on the fine grid, slab by slab, by the numpy
    definition -> (S, N) or (N,) float64 arrays."""
    rt = ds.corner_tables(row_pos, H, False, method)
    ct = ds.corner_tables(col_pos, W, wrap, method)
    out = []
    for name, a in zip(cp.ARRAY_NAMES, arrays):
        if name not in names:
            out.append(a)
        elif a.ndim == 2:
            out.append(ds.interpolate(a, rt, ct).reshape(-1))
        else:
            out.append(np.stack([ds.interpolate(p, rt, ct).reshape(-1) for p in a]))
    return out


def put(torch, eng, a):
    return torch.from_numpy(np.array(a, eng.np_dtype)).to(eng._dev()) if isinstance(a, np.ndarray) else a


def counts(torch, t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def to_numpy(torch, out):
    half = len(out) // 2
    return [o.cpu().numpy() for o in out[:half]] + [counts(torch, o) for o in out[half:]]


def run_reference(torch, eng, cls, dense, **kw):
    """RasterEngine.composite on materialised numpy arrays -> numpy outputs (totals, then counts)."""
    kw.setdefault('every', EVERY)
    out = eng.composite(torch.from_numpy(np.array(cls)).to(eng._dev()), [put(torch, eng, a) for a in dense[:14]],
                        put(torch, eng, dense[14]), K, L, **kw)
    eng.check()
    return to_numpy(torch, out)


def device_arrays(torch, cp, eng, arrays, names, first, n):
    dev = []
    for name, a in zip(cp.ARRAY_NAMES, arrays):
        if not isinstance(a, np.ndarray) or name in names:
            dev.append(put(torch, eng, a))
        else:
            dev.append(put(torch, eng, a[..., first:first + n]))
    return dev


def run_grid(torch, cp, eng, cls, arrays, names, row_pos, col_pos, wrap=False, method='bilinear', first=0, n=None, **kw):
    """DownscaleGrid.composite on numpy inputs, pixels [first, first + n) -> numpy outputs."""
    n = N - first if n is None else n
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=wrap, method=method)
    dev = device_arrays(torch, cp, eng, arrays, names, first, n)
    c = torch.from_numpy(np.array(cls)[first:first + n]).to(eng._dev())
    kw.setdefault('every', EVERY)
    out = grid.composite(c, dev[:14], dev[14], K, L, coarse=names, first_pixel=first, **kw)
    eng.check()
    res = to_numpy(torch, out)
    grid.close()
    return res


def same_results(got, want, what):
    assert len(got) == len(want)
    half = len(got) // 2
    for j in range(half):
        assert got[half + j].dtype == np.uint16 and np.array_equal(got[half + j], want[half + j]), '%s: counts of series %d differ' % (what, j)
        assert got[j].dtype == want[j].dtype and parity.same_bits(got[j], want[j]), '%s: series %d differs' % (what, j)


@pytest.mark.parametrize('pet', [False, True])
@pytest.mark.parametrize('exact', [False, True])
@pytest.mark.parametrize('wrap', [False, True])
@pytest.mark.parametrize('method', ['nearest', 'bilinear', 'cos4'])
def test_same_bits_as_the_composite_on_materialised_drivers(env, method, wrap, exact, pet):
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine('float64', exact)
    for key in SETS:
        names = names_of(ds, key)
        arrays = pick(cp, fine, coarse, names)
        got = run_grid(torch, cp, eng, cls, arrays, names, row_pos, col_pos, wrap, method, pet=pet)
        want = run_reference(torch, eng, cls, materialise(cp, ds, arrays, names, row_pos, col_pos, wrap, method), pet=pet)
        assert got[0].shape == (P, N) and got[0].dtype == np.float64
        same_results(got, want, '%s %s wrap=%s exact=%s pet=%s' % (key, method, wrap, exact, pet))
        assert 0.9 < np.isfinite(want[0]).mean() < 1.0          # both kinds of pixel take part
    if not exact and method == 'cos4' and wrap:                 # two launches give the same bits
        again = run_grid(torch, cp, eng, cls, arrays, names, row_pos, col_pos, wrap, method, pet=pet)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))


def test_the_default_coarse_set_is_the_met_drivers(env):
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine()
    arrays = pick(cp, fine, coarse, ds.MET_DRIVERS)
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos)
    dev = device_arrays(torch, cp, eng, arrays, ds.MET_DRIVERS, 0, N)
    out = grid.composite(torch.from_numpy(np.array(cls)).to(eng._dev()), dev[:14], dev[14], K, every=EVERY)
    eng.check()
    want = run_reference(torch, eng, cls, materialise(cp, ds, arrays, ds.MET_DRIVERS, row_pos, col_pos, False, 'bilinear'))
    same_results(to_numpy(torch, out), want, 'defaults')


@pytest.mark.parametrize('rescale', [False, True])
def test_against_the_numpy_oracle(env, rescale):
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    arrays = pick(cp, fine, coarse, ds.MET_DRIVERS)
    got = run_grid(torch, cp, engine(), cls, arrays, ds.MET_DRIVERS, row_pos, col_pos, True, 'cos4', pet=True, rescale=rescale)
    dense = materialise(cp, ds, arrays, ds.MET_DRIVERS, row_pos, col_pos, True, 'cos4')
    bplut = {k: table()[:, j] for j, k in enumerate(oracle.PARAM_NAMES)}
    par = oracle.gather_params(bplut, cls)
    rates = [np.empty((K, N)) for _ in range(4)]
    with np.errstate(all='ignore'):
        for t in range(K):
            day = [a[cp.slab_index(t, EVERY.get(name, 1))] if getattr(a, 'ndim', 0) == 2 else a
                   for name, a in zip(cp.ARRAY_NAMES, dense)]
            rates[0][t], rates[1][t] = oracle.evapotranspiration(par, *day[:14])
            rates[2][t], rates[3][t] = oracle.potential_et(par, *day[:14])
    hours = dense[14]
    for j, (day, night) in enumerate((rates[0:2], rates[2:4])):
        want, cnt = cp.composite_reduce(cp.daily_total(day, night, hours), L, rescale=rescale)
        assert np.array_equal(got[2 + j], cnt), 'series %d: counts differ from the oracle\'s' % j
        err = parity.assert_parity(got[j], want, RTOL_FAST, 'series %d rescale=%s' % (j, rescale))
        print('series %d rescale=%s: max rel err %.3e over %d pixel-periods' % (j, rescale, err, np.isfinite(want).sum()))
        assert 0.9 < np.isfinite(want).mean() < 1.0
    assert RTOL_FAST <= parity.RTOL_NORTH_STAR


def test_float32_engine_rounds_once(env):
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    narrow = lambda arrays: [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    widen = lambda arrays: [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in arrays]
    for key in ('met', 'mix'):
        names = names_of(ds, key)
        arrays = narrow(pick(cp, fine, coarse, names))
        for exact in (False, True):
            got = run_grid(torch, cp, engine('float32', exact), cls, arrays, names, row_pos, col_pos, True, 'cos4', pet=True)
            wide = run_grid(torch, cp, engine('float64', exact), cls, widen(arrays), names, row_pos, col_pos, True, 'cos4', pet=True)
            for j in range(2):
                assert got[j].dtype == np.float32
                with np.errstate(all='ignore'):
                    assert parity.same_bits(got[j], wide[j].astype(np.float32)), (key, exact, j)
                assert np.array_equal(got[2 + j], wide[2 + j])


def test_a_nan_cell_on_one_day(env):
    """Fine rows and columns an eighth of a cell apart (tests/test_gpu_downscale.py::test_nan_cells): a
    NaN in cell (2, 3) of vpd_day on day 10 takes exactly one day from period 1's count exactly where
    the cell has weight, and nothing anywhere else."""
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, _, _ = inputs()
    row_pos, col_pos = np.arange(R) * 0.125, np.arange(C) * 0.125
    cls = np.where(np.isin(cls, (0, 11)), 1, cls).astype(np.uint8)          # every class has parameters
    fine = [np.nan_to_num(f, nan=0.5) for f in fine]                         # no NaN but the planted one
    day, k = 10, cp.ARRAY_NAMES.index('vpd_day')
    for method, box in (('bilinear', (9, 23, 17, 31)), ('cos4', (9, 23, 17, 31)), ('nearest', (12, 19, 20, 27))):
        arrays = pick(cp, fine, coarse, ds.MET_DRIVERS)
        base = run_grid(torch, cp, engine(), cls, arrays, ds.MET_DRIVERS, row_pos, col_pos, False, method)
        assert (base[1] == np.array([8, 8, 3], np.uint16)[:, None]).all()
        arrays[k] = arrays[k].copy()
        arrays[k][day, 2, 3] = np.nan
        got = run_grid(torch, cp, engine(), cls, arrays, ds.MET_DRIVERS, row_pos, col_pos, False, method)
        dense = materialise(cp, ds, arrays, ds.MET_DRIVERS, row_pos, col_pos, False, method)
        hit = np.isnan(dense[k][day])
        rows, cols = np.flatnonzero(hit.reshape(R, C).any(axis=1)), np.flatnonzero(hit.reshape(R, C).any(axis=0))
        assert (rows.min(), rows.max(), cols.min(), cols.max()) == box and hit.sum() == (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
        want = base[1].astype(np.int64)
        want[day // L, hit] -= 1
        assert np.array_equal(got[1], want), method
        assert parity.same_bits(got[0][:, ~hit], base[0][:, ~hit]) and parity.same_bits(got[0][[0, 2]], base[0][[0, 2]])
        # min_valid = the period's length: those periods are NaN (and the short last period everywhere)
        strict = run_grid(torch, cp, engine(), cls, arrays, ds.MET_DRIVERS, row_pos, col_pos, False, method, min_valid=L)
        assert np.array_equal(strict[1], want)
        assert np.isnan(strict[0][1, hit]).all() and np.isfinite(strict[0][1, ~hit]).all()
        assert np.isfinite(strict[0][0]).all() and np.isnan(strict[0][2]).all()


def loop_daily(torch, cp, eng, cls, dense):
    """The per-day loop: RasterEngine.run per day on the materialised arrays (a flagged pixel-day in
    the reference's operation order, every other by the fast arithmetic), daily_total on the host."""
    c = torch.from_numpy(np.array(cls)).to(eng._dev())
    et = np.empty((K, N))
    for t in range(K):
        day = [a[cp.slab_index(t, EVERY.get(name, 1))] if getattr(a, 'ndim', 0) == 2 else a
               for name, a in zip(cp.ARRAY_NAMES, dense)]
        res = eng.run(c, [put(torch, eng, np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a for a in day[:14]])
        eng.check()
        et[t] = cp.daily_total(res[0].cpu().numpy(), res[1].cpu().numpy(), day[14])
    return et


def test_domain_guard(env):
    """A coarse temp_day cell above 1332 K on day 3 and a negative pressure in a corner cell on day 17
    (the recipe of tests/test_gpu_downscale.py::test_domain_guard; 'nearest' hands the values on as
    they are): the pixels they have weight in go through the kernel behind, and every pixel has the
    bits of the per-day loop."""
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    arrays = pick(cp, fine, coarse, ds.MET_DRIVERS)
    kt, kp = cp.ARRAY_NAMES.index('temp_day'), cp.ARRAY_NAMES.index('pressure')
    arrays[kt] = arrays[kt].copy()
    arrays[kt][3, 1, 2] = 1400.0
    arrays[kp] = arrays[kp].copy()
    arrays[kp][17, 4, 0] = -5.0
    eng = engine()
    got = run_grid(torch, cp, eng, cls, arrays, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    dense = materialise(cp, ds, arrays, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    want, cnt = cp.composite_reduce(loop_daily(torch, cp, eng, cls, dense), L)
    flagged = (dense[kt][3] == 1400.0) | (dense[kp][17] == -5.0)
    assert 20 < flagged.sum() < N // 2                        # at least one pixel flagged, at least one not
    assert np.array_equal(got[1], cnt)
    assert parity.same_bits(got[0][:, flagged], want[:, flagged]) and parity.same_bits(got[0], want)
    assert not (got[0].view(np.uint64) == MARK64).any()
    # only the flagged pixels changed
    base = run_grid(torch, cp, eng, cls, pick(cp, fine, coarse, ds.MET_DRIVERS), ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest')
    assert parity.same_bits(got[0][:, ~flagged], base[0][:, ~flagged]) and not parity.same_bits(got[0], base[0])
    # with potential ET, and in float32 storage: the same, and no mark either
    pet = run_grid(torch, cp, eng, cls, arrays, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest', pet=True)
    same_results(pet, run_reference(torch, eng, cls, dense, pet=True), 'guard pet')
    assert parity.same_bits(pet[0], want) and not any((g.view(np.uint64) == MARK64).any() for g in pet[:2])
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    g32 = run_grid(torch, cp, engine('float32'), cls, narrow, ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest', pet=True)
    w64 = run_grid(torch, cp, eng, cls, [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in narrow],
                   ds.MET_DRIVERS, row_pos, col_pos, True, 'nearest', pet=True)
    for j in range(2):
        with np.errstate(all='ignore'):
            assert parity.same_bits(g32[j], w64[j].astype(np.float32))
        assert np.array_equal(g32[2 + j], w64[2 + j])
        assert not (g32[j].view(np.uint32) == MARK32).any()


@functools.lru_cache(maxsize=None)
def full_call():
    import torch
    from mod16_amd import composite as cp
    cls, fine, coarse, row_pos, col_pos = inputs()
    out = run_grid(torch, cp, engine(), cls, pick(cp, fine, coarse, MIX), MIX, row_pos, col_pos, True, 'cos4', pet=True)
    for o in out:
        o.setflags(write=False)
    return out


@pytest.mark.parametrize('first,n', [(256, 512), (0, 256), (100, 300), (53, 1), (1792, None), (1800, 161), (N, 0)])
def test_ranges_equal_slices_of_the_full_call(env, first, n):
    """A batch boundary, mid-row, one pixel, the last ragged batch, nothing."""
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    want = full_call()
    got = run_grid(torch, cp, engine(), cls, pick(cp, fine, coarse, MIX), MIX, row_pos, col_pos, True, 'cos4',
                   first=first, n=n, pet=True)
    hi = N if n is None else first + n
    assert got[0].shape == (P, hi - first)
    same_results(got, [w[:, first:hi] for w in want], 'range %d + %s' % (first, n))


def test_strides_and_caller_outputs(env):
    """Coarse planes with a row pitch of W + 3 and a time stride of (H + 1)(W + 3), as views of larger
    tensors; the coarse (H, W) constant beside them; pitched caller outputs."""
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    eng = engine()
    names = ds.MET_DRIVERS
    arrays = pick(cp, fine, coarse, names)
    want = run_grid(torch, cp, eng, cls, arrays, names, row_pos, col_pos, True, 'cos4', pet=True)
    dev = device_arrays(torch, cp, eng, arrays, names, 0, N)
    for k, name in enumerate(cp.ARRAY_NAMES):
        if name not in names:
            continue
        lead = tuple(dev[k].shape[:-2])
        buf = torch.full(lead + (H + 1, W + 3), float('nan'), dtype=eng.dtype, device=eng._dev())
        view = buf[..., :H, :W]
        view.copy_(dev[k])
        assert view.stride()[-2:] == (W + 3, 1) and not view.is_contiguous()
        assert not lead or view.stride(0) == (H + 1) * (W + 3)
        dev[k] = view
    assert dev[cp.ARRAY_NAMES.index('temp_annual')].dim() == 2 and dev[0].dim() == 3
    pitch, poison = N + 59, -7
    bufs = [torch.full((P, pitch), poison, dtype=eng.dtype, device=eng._dev()) for _ in range(2)] + \
           [torch.full((P, pitch), 7, dtype=torch.int16, device=eng._dev()).view(torch.uint16) for _ in range(2)]
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=True, method='cos4')
    c = torch.from_numpy(np.array(cls)).to(eng._dev())
    out = grid.composite(c, dev[:14], dev[14], K, L, every=EVERY, pet=True, out=[b[:, :N] for b in bufs])
    eng.check()
    assert all(o.data_ptr() == b.data_ptr() for o, b in zip(out, bufs))
    same_results(to_numpy(torch, out), want, 'strided')
    assert all((b[:, N:] == poison).all() for b in bufs[:2]) and all((counts(torch, b)[:, N:] == 7).all() for b in bufs[2:])
    # the coarse arrays share one pitch; a time stride below a plane is refused
    mixed = list(dev)
    mixed[0] = put(torch, eng, arrays[0])
    with pytest.raises(ValueError, match='one distance between rows'):
        grid.composite(c, mixed[:14], mixed[14], K, L, every=EVERY)
    mixed[0] = dev[0][:1].expand(K, H, W)
    with pytest.raises(ValueError, match='stride in time'):
        grid.composite(c, mixed[:14], mixed[14], K, L, every=EVERY)
    mixed[0] = dev[0][:K - 1]
    with pytest.raises(ValueError, match='time slabs'):
        grid.composite(c, mixed[:14], mixed[14], K, L, every=EVERY)
    grid.close()
    with pytest.raises(ValueError, match='closed'):
        grid.composite(c, dev[:14], dev[14], K, L, every=EVERY)


def test_mixed_and_trusted_engines_are_refused(env):
    torch, mod16_amd, _lib, cp, ds = env
    from mod16_amd.raster import RasterEngine
    cls, fine, coarse, row_pos, col_pos = inputs()
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in pick(cp, fine, coarse, ds.MET_DRIVERS)]
    for kw in (dict(math=_lib.MATH_MIXED), dict(trusted=True)):
        eng = RasterEngine(table(), dtype='float32', **kw)
        with pytest.raises(ValueError, match='MATH_FAST or MATH_EXACT'):
            run_grid(torch, cp, eng, cls, narrow, ds.MET_DRIVERS, row_pos, col_pos)


def shaped(arrays, names, cp):
    """The numpy entry point's arrays: fine ones as (S, R, C) / (R, C)."""
    return [a.reshape(a.shape[:-1] + (R, C)) if isinstance(a, np.ndarray) and name not in names else a
            for name, a in zip(cp.ARRAY_NAMES, arrays)]


def test_numpy_entry_point(env):
    torch, mod16_amd, _lib, cp, ds = env
    cls, fine, coarse, row_pos, col_pos = inputs()
    call = mod16_amd.evapotranspiration_composite_downscaled
    for key in ('met', 'mix'):
        names = names_of(ds, key)
        arrays = pick(cp, fine, coarse, names)
        want = run_grid(torch, cp, engine(), cls, arrays, names, row_pos, col_pos, True, 'cos4', pet=True)
        # the result does not depend on stage_bytes, down to one batch of 256 pixels per tile
        for stage_bytes in (None, 3 << 20, 1):
            got = call(table(), cls.reshape(R, C), *shaped(arrays, names, cp), row_pos, col_pos, days=K, period_days=L,
                       every=EVERY, wrap=True, method='cos4', coarse=names, pet=True, stage_bytes=stage_bytes)
            assert type(got).__name__ == 'CompositeETPET' and got.et.shape == (P, R, C)
            same_results([g.reshape(P, N) for g in got], want, '%s stage_bytes=%s' % (key, stage_bytes))
    # days from the daily arrays, the default coarse set, EXACT, out=, float32
    names = ds.MET_DRIVERS
    arrays = pick(cp, fine, coarse, names)
    outs = [np.full((P, R, C), -7.0), np.zeros((P, R, C), np.uint16)]
    got = call(table(), cls.reshape(R, C), *shaped(arrays, names, cp), row_pos, col_pos, every=EVERY, math=_lib.MATH_EXACT, out=outs)
    assert got.et is outs[0] and got.count is outs[1]
    want = run_grid(torch, cp, engine('float64', True), cls, arrays, names, row_pos, col_pos)
    same_results([g.reshape(P, N) for g in got], want, 'exact')
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    g32 = call(table(), cls.reshape(R, C), *shaped(narrow, names, cp), row_pos, col_pos, every=EVERY, min_valid=2, rescale=True)
    w32 = run_grid(torch, cp, engine('float32'), cls, narrow, names, row_pos, col_pos, min_valid=2, rescale=True)
    assert g32.et.dtype == np.float32
    same_results([g.reshape(P, N) for g in g32], w32, 'float32')
    # a class code >= 13, the mixed and the trusted forms
    bad = np.array(cls).reshape(R, C)
    bad[20, 31] = 13
    with pytest.raises(IndexError):
        call(table(), bad, *shaped(arrays, names, cp), row_pos, col_pos, every=EVERY)
    for math in (_lib.MATH_MIXED, _lib.DOMAIN_TRUSTED):
        with pytest.raises(ValueError, match='MATH_FAST or MATH_EXACT'):
            call(table(), cls.reshape(R, C), *shaped(arrays, names, cp), row_pos, col_pos, every=EVERY, math=math)


def test_host_call_with_pitched_coarse_series(env):
    """_lib.Downscale.composite, where=HOST, numpy addresses: fine 6 x 10 over coarse 5 x 7, three days in
    periods of two. Every coarse series with its rows 9 elements apart and its planes a plane's span
    ((H - 1) 9 + W) apart, NaN in between -- the upload's copy per row -- against the same call on packed
    planes, bit for bit, counts included. temp_annual is one coarse plane, sw_rad_night a scalar, albedo,
    fPAR and LAI fine daily arrays."""
    torch, mod16_amd, _lib, cp, ds = env
    shape, days, period, pitch = (6, 10), 3, 2, 9
    n, periods = shape[0] * shape[1], 2
    cls3, fine = synth.drivers((days, n), seed=91, special=True)
    planes = [synth.drivers((H, W), seed=92 + t, special=False)[1] for t in range(days)]
    names = tuple(name for name in ds.MET_DRIVERS if name != 'sw_rad_night') + ('day_hours',)
    series = {name: np.stack([planes[t][k] for t in range(days)]) for k, name in enumerate(cp.ARRAY_NAMES[:14]) if name in names}
    series['day_hours'] = np.random.default_rng(95).uniform(6, 18, (days, H, W))
    series['temp_annual'] = series['temp_annual'][:1]
    cls = np.ascontiguousarray(cls3[0])
    row_pos, col_pos = ds.positions(-0.8, 0.9, shape[0], 0.0, 1.0), ds.positions(-9.3, 2.1, shape[1], 0.0, 1.0)
    eng = engine()
    torch.cuda.synchronize()

    def call(cpitch):
        span = (H - 1) * cpitch + W
        keep, ptrs, pstride, tstride, every = [], [], [], [], []
        for k, name in enumerate(cp.ARRAY_NAMES):
            if name in names:
                a = series[name]
                mem = np.full((len(a) - 1) * span + span, np.nan)
                view = np.lib.stride_tricks.as_strided(mem, a.shape, (span * 8, cpitch * 8, 8))
                view[...] = a
                assert np.isnan(mem).sum() == len(a) * (H - 1) * (cpitch - W) + np.isnan(a).sum()
                pstride.append(0); tstride.append(span if len(a) > 1 else 0); every.append(1 if len(a) > 1 else days)
            elif name == 'sw_rad_night':
                mem = np.zeros(1)
                pstride.append(0); tstride.append(0); every.append(days)
            else:
                mem = np.ascontiguousarray(fine[k])
                pstride.append(1); tstride.append(n); every.append(1)
            keep.append(mem)
            ptrs.append(mem.ctypes.data)
        outs = [np.full((periods, n), -7.0) for _ in range(2)] + [np.full((periods, n), 7, np.uint16) for _ in range(2)]
        low = _lib.Downscale(eng.ctx, shape, (H, W), row_pos, col_pos, wrap=True, method='bilinear')
        low.composite('float64', n, days, period, cls.ctypes.data, ptrs, pstride, tstride, every, ds.coarse_mask(names),
                      cpitch, 0, outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data, n,
                      flags=_lib.MATH_FAST, where=_lib.HOST)
        low.close()
        return outs

    packed, pitched = call(W), call(pitch)
    same_results(pitched, packed, 'pitched coarse series')
    assert 0.5 < np.isfinite(packed[0]).mean() and (packed[2] <= period).all() and (packed[2] > 0).any()
