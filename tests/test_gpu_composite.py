"""GPU tests of the multi-day composites (mod16_et_composite_*: RasterEngine.composite,
mod16_amd.evapotranspiration_composite) against the loop they replace -- a per-day RasterEngine.run /
run_pet on the same tensors, then mod16_amd.composite.daily_total and composite_reduce on the host --
bit for bit, and against the numpy oracle per day.

Shapes: n = 8192 + 37 pixels (33 batches of 256, a ragged last one), K = 19 days in periods of L = 8
(8, 8 and 3 days), albedo / fPAR / LAI in 3 eight-day slabs, temp_annual and pressure constant,
sw_rad_night the scalar 0, everything else daily; NaN planted in temp_day on 2 % of the pixel-days.

Tolerance against the oracle: |got - want| <= (1e-8 + K 2^-52) * scale, scale = the sum over the
period's valid days of (|day_t| h_t + |night_t| (24 - h_t)) * 3600, times the rescale factor where
used. 1e-8 is what tests/test_gpu_raster.py holds every FAST float64 value to, a sum is 1-Lipschitz
in its terms, and K 2^-52 covers the order of K additions. Where scale is 0 the output is exactly 0."""
import functools

import numpy as np
import pytest

from oracle import mod16_oracle as oracle
from oracle import synth
import parity

pytestmark = pytest.mark.gpu

N = 8192 + 37
K = 19
L = 8
P = 3
EVERY = {'sw_albedo': 8, 'fpar': 8, 'lai': 8}


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    from mod16_amd import composite as cp
    from mod16_amd.raster import RasterEngine
    return torch, mod16_amd, _lib, cp, RasterEngine


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
def inputs(seed=41):
    """(cls, the 14 drivers, hours): numpy, read-only; the recipe of the module docstring."""
    cls3, slow = synth.drivers((P, N), seed=seed, special=True)
    _, daily = synth.drivers((K, N), seed=seed + 1, special=False)
    rng = np.random.default_rng(seed + 2)
    arrays = list(daily)
    arrays[3] = 0.0                                  # sw_rad_night
    for k in (4, 12, 13):                            # albedo, fPAR, LAI: 8-day slabs
        arrays[k] = slow[k]
    for k in (7, 11):                                # temp_annual, pressure: constant
        arrays[k] = np.ascontiguousarray(slow[k][0])
    t_day = daily[5].copy()
    t_day[rng.uniform(0, 1, (K, N)) < 0.02] = np.nan
    arrays[5] = t_day
    hours = rng.uniform(6, 18, (K, N))
    cls = np.ascontiguousarray(cls3[0])
    for a in [cls, hours] + [a for a in arrays if isinstance(a, np.ndarray)]:
        a.setflags(write=False)
    return cls, tuple(arrays), hours


def day_of(cp, arrays, hours, t):
    """Day t's 14 drivers and hours: the slab t // every of an array with a time axis."""
    out = []
    for name, a in zip(cp.ARRAY_NAMES, tuple(arrays) + (hours,)):
        out.append(a[cp.slab_index(t, EVERY.get(name, 1))] if getattr(a, 'ndim', 0) == 2 else a)
    return out[:14], out[14]


def to_device(torch, eng, cls, arrays, hours):
    dev = eng._dev()
    put = lambda a: torch.from_numpy(np.array(a, eng.np_dtype)).to(dev) if isinstance(a, np.ndarray) else a
    return torch.from_numpy(np.array(cls)).to(dev), [put(a) for a in arrays], put(hours)


def counts(torch, t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def run_composite(torch, eng, cls, arrays, hours, **kw):
    """RasterEngine.composite on numpy inputs -> numpy outputs (totals, then counts)."""
    c, a, h = to_device(torch, eng, cls, arrays, hours)
    kw.setdefault('every', EVERY)
    out = eng.composite(c, a, h, K, L, **kw)
    eng.check()
    half = len(out) // 2
    return [o.cpu().numpy() for o in out[:half]] + [counts(torch, o) for o in out[half:]]


def loop_daily(torch, cp, eng, cls, arrays, hours, pet):
    """The loop the composite replaces: run (run_pet) per day on the device, daily_total on the host.
    -> (K, n) daily ET totals, and the PET ones or None."""
    c, a, h = to_device(torch, eng, cls, arrays, hours)
    et = np.empty((K, cls.size))
    pt = np.empty((K, cls.size)) if pet else None
    for t in range(K):
        drv, hrs = day_of(cp, a, h, t)
        res = eng.run_pet(c, drv) if pet else eng.run(c, drv)
        eng.check()
        res = [r.cpu().numpy() for r in res]
        hrs = hrs.cpu().numpy()
        et[t] = cp.daily_total(res[0], res[1], hrs)
        if pet:
            pt[t] = cp.daily_total(res[2], res[3], hrs)
    return et, pt


@functools.lru_cache(maxsize=None)
def reference_loop(pet, exact=False):
    """The per-day loop on the parity inputs, once per form."""
    import torch
    from mod16_amd import composite as cp
    et, pt = loop_daily(torch, cp, engine('float64', exact), *inputs(), pet)
    et.setflags(write=False)
    if pt is not None:
        pt.setflags(write=False)
    return et, pt


def population(count, want):
    """The conditions every comparison is held to: enough of every kind of pixel-period."""
    lens = np.array([8, 8, 3])[:, None]
    assert np.isfinite(want).mean() >= 0.95, np.isfinite(want).mean()
    assert ((count > 0) & (count < lens)).mean() >= 0.05
    assert (count == 0).mean() >= 0.01


def same_as_loop(cp, got, daily_et, daily_pt, what, **kw):
    pet = daily_pt is not None
    half = len(got) // 2
    assert half == (2 if pet else 1)
    for j, daily in enumerate((daily_et, daily_pt)[:half]):
        want, cnt = cp.composite_reduce(daily, L, **kw)
        assert got[half + j].dtype == np.uint16 and np.array_equal(got[half + j], cnt), '%s: counts of series %d differ' % (what, j)
        assert parity.same_bits(got[j], want), '%s: series %d differs from the per-day loop' % (what, j)
    return cp.composite_reduce(daily_et, L, **kw)


@pytest.mark.parametrize('pet', [False, True])
def test_same_bits_as_the_per_day_loop_fast(env, pet):
    torch, mod16_amd, _lib, cp, _ = env
    got = run_composite(torch, engine(), *inputs(), pet=pet)
    et, pt = reference_loop(pet)
    want, cnt = same_as_loop(cp, got, et, pt, 'FAST pet=%s' % pet)
    population(cnt, want)
    # two launches give the same bits
    again = run_composite(torch, engine(), *inputs(), pet=pet)
    assert all(parity.same_bits(a, b) if a.dtype != np.uint16 else np.array_equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('pet', [False, True])
def test_same_bits_as_the_per_day_loop_exact(env, pet):
    torch, mod16_amd, _lib, cp, _ = env
    got = run_composite(torch, engine('float64', True), *inputs(), pet=pet)
    et, pt = reference_loop(pet, True)
    want, cnt = same_as_loop(cp, got, et, pt, 'EXACT pet=%s' % pet)
    population(cnt, want)


@functools.lru_cache(maxsize=None)
def oracle_daily():
    """Per day: the oracle's day / night rates and potential-ET rates, (K, n) each."""
    from mod16_amd import composite as cp
    cls, arrays, hours = inputs()
    bplut = {k: table()[:, j] for j, k in enumerate(oracle.PARAM_NAMES)}
    par = oracle.gather_params(bplut, cls)
    out = [np.empty((K, N)) for _ in range(4)]
    with np.errstate(all='ignore'):
        for t in range(K):
            drv, _ = day_of(cp, arrays, hours, t)
            out[0][t], out[1][t] = oracle.evapotranspiration(par, *drv)
            out[2][t], out[3][t] = oracle.potential_et(par, *drv)
    return tuple(out)


@pytest.mark.parametrize('rescale', [False, True])
def test_against_the_numpy_oracle(env, rescale):
    torch, mod16_amd, _lib, cp, _ = env
    cls, arrays, hours = inputs()
    got = run_composite(torch, engine(), cls, arrays, hours, pet=True, rescale=rescale)
    rates = oracle_daily()
    assert not np.isinf(np.array(rates)).any()
    for j, (day, night) in enumerate((rates[0:2], rates[2:4])):
        daily = cp.daily_total(day, night, hours)
        want, cnt = cp.composite_reduce(daily, L, rescale=rescale)
        population(cnt, want)
        g = got[j]
        assert np.array_equal(got[2 + j], cnt), 'series %d: counts differ from the oracle\'s' % j
        assert np.array_equal(np.isnan(g), np.isnan(want)), 'series %d: NaN masks differ from the oracle\'s' % j
        mag = (np.abs(day) * hours + np.abs(night) * (24.0 - hours)) * 3600.0
        scale, _ = cp.composite_reduce(np.where(np.isnan(daily), np.nan, mag), L, rescale=rescale)
        ok = ~np.isnan(want)
        assert ok.mean() >= 0.95
        err = np.abs(g[ok] - want[ok])
        bound = (1e-8 + K * 2.0 ** -52) * scale[ok]
        worst = float(np.max(err / np.where(scale[ok] > 0, scale[ok], 1.0)))
        print('series %d rescale=%s: worst |got - want| / scale = %.3e over %d pixel-periods' % (j, rescale, worst, ok.sum()))
        assert (err <= bound).all(), worst
        assert (g[ok][scale[ok] == 0] == 0).all()


def test_float32_is_the_float64_composite_rounded_once(env):
    torch, mod16_amd, _lib, cp, _ = env
    cls, arrays, hours = inputs()
    narrow = [a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in arrays]
    h32 = hours.astype(np.float32)
    got = run_composite(torch, engine('float32'), cls, narrow, h32, pet=True)
    wide = run_composite(torch, engine(), cls, [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in narrow],
                         h32.astype(np.float64), pet=True)
    for j in range(2):
        assert got[j].dtype == np.float32
        with np.errstate(all='ignore'):
            assert parity.same_bits(got[j], wide[j].astype(np.float32)), 'series %d' % j
        assert np.array_equal(got[2 + j], wide[2 + j])
    population(wide[2], wide[0])


def test_min_valid_and_rescale(env):
    torch, mod16_amd, _lib, cp, _ = env
    cls, arrays, hours = inputs()
    et, _ = reference_loop(False)
    got = run_composite(torch, engine(), cls, arrays, hours, min_valid=3, rescale=True)
    want, cnt = same_as_loop(cp, got, et, None, 'min_valid=3 rescale', min_valid=3, rescale=True)
    assert np.isnan(want[cnt < 3]).all() and (cnt < 3).sum() > (cnt == 0).sum()
    # a pixel with exactly min_valid - 1 = 2 valid days in period 1: NaN there, finite elsewhere
    arrays = list(arrays)
    t_day = arrays[5].copy()
    pixel = int(np.flatnonzero((cnt == np.array([8, 8, 3])[:, None]).all(axis=0))[7])
    t_day[8:16, pixel] = np.nan
    t_day[[9, 14], pixel] = arrays[5][[9, 14], pixel]
    arrays[5] = t_day
    planted = run_composite(torch, engine(), cls, arrays, hours, min_valid=3, rescale=True)
    assert planted[1][:, pixel].tolist() == [8, 2, 3]
    assert np.isnan(planted[0][1, pixel]) and np.isfinite(planted[0][[0, 2], pixel]).all()
    loose = run_composite(torch, engine(), cls, arrays, hours, min_valid=2, rescale=True)
    assert np.isfinite(loose[0][:, pixel]).all()
    others = np.arange(N) != pixel
    assert parity.same_bits(planted[0][:, others], got[0][:, others])


@pytest.mark.parametrize('pet', [False, True])
def test_domain_guard_matches_the_per_day_loop(env, pet):
    """Values outside the domain of the fast arithmetic (bounds: include/mod16_hip.h) in a few
    pixel-days: those pixels go through the kernel behind, and still have the per-day loop's bits."""
    torch, mod16_amd, _lib, cp, _ = env
    cls, arrays, hours = inputs()
    cls = cls.copy()
    arrays = [a.copy() if isinstance(a, np.ndarray) else a for a in arrays]
    first, last_day, always, empty0, cold = 3, 300, 4097, 8000, N - 1
    cls[[first, last_day, always, empty0, cold]] = 1
    arrays[5][0, first] = 1400.0              # day 0: temp_day above 1332 K
    arrays[9][K - 1, last_day] = np.inf       # day K - 1: an infinite vpd_day
    arrays[11][always] = -5.0                 # a negative (constant) pressure: every day
    arrays[5][0:8, empty0] = np.nan           # period 0 has no valid day ...
    arrays[13][1, empty0] = 1e210             # ... and the LAI of days 8-15 overflows the fast products
    arrays[6][5, cold] = 20.0                 # temp_night below the pole of the Tetens formula
    arrays[4][2, 17] = -np.inf                # an infinite albedo in the last, short period
    got = run_composite(torch, engine(), cls, arrays, hours, pet=pet)
    et, pt = loop_daily(torch, cp, engine(), cls, arrays, hours, pet)
    want, cnt = same_as_loop(cp, got, et, pt, 'domain guard pet=%s' % pet)
    assert cnt[0, empty0] == 0 and np.isnan(got[0][0, empty0])
    # the mark the fast kernel leaves for the kernel behind it (CompMark) is in no output: same_bits
    # does not look at NaN payloads
    for g in got[:len(got) // 2]:
        assert not (g.view(np.uint64) == 0x7ff80000000c0351).any()
    # only the planted pixels changed
    base = run_composite(torch, engine(), *inputs(), pet=pet)
    untouched = np.ones(N, bool)
    untouched[[first, last_day, always, empty0, cold, 17]] = False
    assert parity.same_bits(got[0][:, untouched], base[0][:, untouched])


def test_strided_inputs_and_pitched_outputs(env):
    torch, mod16_amd, _lib, cp, _ = env
    eng = engine()
    cls, arrays, hours = inputs()
    want = run_composite(torch, eng, cls, arrays, hours, pet=True)
    c, a, h = to_device(torch, eng, cls, arrays, hours)
    pitch = N + 59

    def strided(t):
        if not (isinstance(t, torch.Tensor) and t.dim() == 2):
            return t
        buf = torch.full((t.shape[0], pitch), float('nan'), dtype=t.dtype, device=t.device)
        view = buf[:, 3:3 + N]
        view.copy_(t)
        assert view.stride() == (pitch, 1) and not view.is_contiguous()
        return view
    opitch = N + 101
    poison = -7.0
    bufs = [torch.full((P, opitch), poison, dtype=eng.dtype, device=eng._dev()) for _ in range(2)] + \
           [torch.full((P, opitch), 0x7fff, dtype=torch.int16, device=eng._dev()).view(torch.uint16) for _ in range(2)]
    out = eng.composite(c, [strided(t) for t in a], strided(h), K, L, every=EVERY, pet=True, out=[b[:, :N] for b in bufs])
    eng.check()
    for j in range(2):
        assert parity.same_bits(bufs[j][:, :N].cpu().numpy(), want[j]), j
        assert (bufs[j][:, N:] == poison).all()
        assert np.array_equal(counts(torch, bufs[2 + j][:, :N]), want[2 + j]), j
        assert (counts(torch, bufs[2 + j][:, N:]) == 0x7fff).all()
    assert out[0].data_ptr() == bufs[0].data_ptr()
    # n = 1: the first pixel alone, through views of the same buffers
    one = eng.composite(c[:1], [t[..., :1] if isinstance(t, torch.Tensor) else t for t in a], h[:, :1], K, L,
                        every=EVERY, pet=True)
    eng.check()
    for j in range(2):
        assert one[j].shape == (P, 1) and parity.same_bits(one[j].cpu().numpy()[:, 0], want[j][:, 0])
        assert np.array_equal(counts(torch, one[2 + j])[:, 0], want[2 + j][:, 0])
    # n = 0: nothing to do, empty results
    none = eng.composite(c[:0], [t[..., :0] if isinstance(t, torch.Tensor) else t for t in a], h[:, :0], K, L, every=EVERY)
    assert len(none) == 2 and tuple(none[0].shape) == (P, 0) and tuple(none[1].shape) == (P, 0)
    with pytest.raises(ValueError, match='time slabs'):
        eng.composite(c, a, h, K, L)                      # the 8-day arrays without their divisor
    with pytest.raises(ValueError, match='unit stride'):
        eng.composite(c, [torch.zeros((K, 2 * N), dtype=eng.dtype, device=eng._dev())[:, ::2]] + a[1:], h, K, L, every=EVERY)


@pytest.mark.parametrize('pet', [False, True])
def test_host_path_equals_the_device_call(env, pet):
    """evapotranspiration_composite on numpy arrays stages pixel tiles, every time slab of every
    array: 20 arrays (19 of them T-sized, 33 KiB of stagger each) in 191 (195 with PET) slab rows here,
    so with stage_bytes = 5.7e6 a tile is (5.7e6 - 19 * 33792 - 512) / (rows * 8 + 1) = 3307 (3239) ->
    3072 pixels and n spans three; with 2e6 it is 768 pixels, by default the whole raster."""
    torch, mod16_amd, _lib, cp, _ = env
    cls, arrays, hours = inputs()
    want = run_composite(torch, engine(), cls, arrays, hours, pet=pet)
    for stage_bytes in (5700000, 2000000, None):
        got = mod16_amd.evapotranspiration_composite(table(), cls, *arrays, hours, days=K, period_days=L, every=EVERY,
                                                     pet=pet, stage_bytes=stage_bytes)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == (P, N) and g.dtype == w.dtype
            assert np.array_equal(g, w) if g.dtype == np.uint16 else parity.same_bits(g, w), stage_bytes
    # the pixel shape is the class raster's; days from the daily arrays
    shaped = mod16_amd.evapotranspiration_composite(
        table(), cls[:8192].reshape(64, 128), *[a[..., :8192].reshape(a.shape[:-1] + (64, 128)) if isinstance(a, np.ndarray) else a
                                                 for a in arrays], hours[:, :8192].reshape(K, 64, 128), every=EVERY, pet=pet)
    assert shaped[0].shape == (P, 64, 128) and parity.same_bits(shaped[0].reshape(P, -1), want[0][:, :8192])


def test_class_code_out_of_range_raises_index_error(env):
    torch, mod16_amd, _lib, cp, _ = env
    cls, arrays, hours = inputs()
    cls = cls.copy()
    cls[N - 2] = 13
    with pytest.raises(IndexError):
        run_composite(torch, engine(), cls, arrays, hours)
    with pytest.raises(IndexError):
        mod16_amd.evapotranspiration_composite(table(), cls, *arrays, hours, every=EVERY)
    # the mixed-precision and the trusted forms are refused, by the engine and by the library
    from mod16_amd.raster import RasterEngine
    with pytest.raises(ValueError, match='MATH_FAST or MATH_EXACT'):
        RasterEngine(table(), dtype='float32', math=_lib.MATH_MIXED).composite(None, [0.0] * 14, 12.0, K, L)
    with pytest.raises(ValueError, match='MATH_FAST or MATH_EXACT'):
        RasterEngine(table(), trusted=True).composite(None, [0.0] * 14, 12.0, K, L)
