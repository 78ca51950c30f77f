"""GPU tests of the ensemble forward run (mod16_et_ensemble_*: per-pixel mean and spread of ET over D
parameter tables) against a plain loop over the numpy oracle, one member at a time, followed by
np.mean / np.std over the member axis.

Tolerance (every test that compares with the oracle): 1e-8 * scale, scale = max_m |x_m| for the day
and night outputs and max_m (|day_m| + |night_m|) for std_total. 1e-8 is what tests/test_gpu_raster.py
holds every FAST float64 member value to; mean and std are 1-Lipschitz in the largest member error;
the single-pass accumulation adds about D 2^-52 scale; numpy's two-pass std and a sequential shifted
single pass differ by at most 7e-16 scale at D = 33 on these inputs. Where scale is 0 the outputs are
exactly 0."""
import functools
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import mod16_oracle as oracle
from oracle import synth
import parity

pytestmark = pytest.mark.gpu

N = 65536 + 37          # a ragged tail behind 256 whole batches
D_MAX = 33              # neither a multiple of nor smaller than the 16-member chunk of the kernel
NAMES = ('mean_day', 'mean_night', 'std_day', 'std_night', 'std_total')


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    from mod16_amd.raster import RasterEngine
    return torch, mod16_amd, _lib, RasterEngine


@functools.lru_cache(maxsize=None)
def base_table():
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    t = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def tables(D=D_MAX, seed=2024):
    """The Collection 6.1 table perturbed by up to 10 % per entry: the ramps stay ramps (checked), the
    member spread is 4-5 % of the mean."""
    rng = np.random.default_rng(seed)
    t = base_table() * (1 + 0.1 * rng.uniform(-1, 1, (D, 13, 11)))
    pft = list(oracle.PFT_VALID)
    assert (t[:, pft, 1] > t[:, pft, 0]).all() and (t[:, pft, 3] > t[:, pft, 2]).all() and (t[:, pft, 9] > t[:, pft, 8]).all()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def raster(n=N, seed=11):
    cls, drv = synth.drivers((n,), seed=seed)
    for a in [cls] + drv:
        a.setflags(write=False)
    return cls, tuple(drv)


def members_of(tabs, cls, drv):
    """(D, n) day and night totals of the oracle, one member at a time."""
    days, nights = [], []
    for t in tabs:
        bplut = {k: t[:, j] for j, k in enumerate(oracle.PARAM_NAMES)}
        with np.errstate(all='ignore'):
            d, g = oracle.evapotranspiration_raster(bplut, cls, *drv)
        days.append(d)
        nights.append(g)
    return np.array(days), np.array(nights)


@functools.lru_cache(maxsize=None)
def reference_members():
    """The oracle's members of the parity raster, computed once (D = 1 and 5 are its first members)."""
    cls, drv = raster()
    days, nights = members_of(tables(), cls, drv)
    days.setflags(write=False)
    nights.setflags(write=False)
    return days, nights


def check(got, days, nights, what, plain=False):
    """The non-finite rules and the tolerance of the module docstring. plain: no member is
    infinite (ordinary drivers), so the NaN masks are numpy's."""
    with np.errstate(all='ignore'):
        total = days + nights
        cases = ((got[0], days, np.mean, np.abs(days).max(axis=0)),
                 (got[1], nights, np.mean, np.abs(nights).max(axis=0)),
                 (got[2], days, np.std, np.abs(days).max(axis=0)),
                 (got[3], nights, np.std, np.abs(nights).max(axis=0)),
                 (got[4], total, np.std, (np.abs(days) + np.abs(nights)).max(axis=0)))
        for name, g, x, fn, scale in zip(NAMES, *zip(*cases)):
            assert g.dtype == np.float64 and g.shape == x.shape[1:], (what, name)
            want = fn(x, axis=0)
            any_nan = np.isnan(x).any(axis=0)
            any_inf = np.isinf(x).any(axis=0) & ~any_nan
            if plain:
                assert not any_inf.any()
                assert np.array_equal(np.isnan(g), np.isnan(want)), '%s %s: NaN masks differ from numpy\'s' % (what, name)
            assert np.isnan(g[any_nan]).all(), '%s %s: a NaN member did not make the output NaN' % (what, name)
            assert (~np.isfinite(g[any_inf])).all(), '%s %s: an infinite member left a finite output' % (what, name)
            fin = ~any_nan & ~any_inf
            ok = fin & np.isfinite(want)
            assert np.isfinite(g[ok]).all(), (what, name)
            err = np.abs(g[ok] - want[ok])
            rel = err[scale[ok] > 0] / scale[ok][scale[ok] > 0]
            print('%s %s: max |got - numpy| / scale = %.3e over %d pixels' % (what, name, rel.max() if rel.size else 0.0, int(ok.sum())))
            assert (err <= 1e-8 * scale[ok]).all(), '%s %s: %.3e x scale' % (what, name, rel.max())
            assert (g[fin & (scale == 0)] == 0).all(), (what, name)
            # finite members whose squared deviations overflow in numpy (members beyond 1e154): inf
            # there; the shifted sums square x_m - x_0 instead of x_m - mean, at most twice as large,
            # so they overflow too or hold a value of that size
            over = fin & ~np.isfinite(want)
            assert (~np.isfinite(g[over]) | (np.abs(g[over]) >= 1e150)).all(), (what, name)


def host_run(m16, tabs, cls, drv, **kw):
    return m16.evapotranspiration_ensemble(tabs, cls, *drv, **kw)


def device_run(env, tabs, cls, drv, math=None, dtype='float64'):
    torch, m16, _lib, RasterEngine = env
    eng = RasterEngine(base_table(), dtype=dtype, math=_lib.MATH_FAST if math is None else math)
    ens = eng.ensemble(tabs)
    assert ens.members == len(tabs)
    out = ens.run(torch.from_numpy(np.array(cls)).cuda(), [torch.from_numpy(np.array(d)).cuda() for d in drv])
    eng.check()
    res = [t.cpu().numpy() for t in out]
    ens.close()
    return res


@pytest.mark.parametrize('math', ['fast', 'exact'])
@pytest.mark.parametrize('D', [1, 5, D_MAX])
def test_parity_with_the_member_loop(env, D, math):
    torch, m16, _lib, RasterEngine = env
    cls, drv = raster()
    days, nights = reference_members()
    got = device_run(env, tables()[:D], cls, drv, math=_lib.MATH_EXACT if math == 'exact' else _lib.MATH_FAST)
    check(got, days[:D], nights[:D], 'D = %d, %s' % (D, math), plain=True)
    if D > 1:       # the spread is a number to lose: 4-5 % of the mean on these tables
        ok = np.isfinite(got[0]) & (got[0] > 0)
        assert 0.02 < np.median(got[2][ok] / got[0][ok]) < 0.1


def test_identical_members(env):
    """D = 7 copies of one table: a spread of exactly 0 wherever the mean is finite, and the mean of
    the one-member ensemble, bit for bit."""
    cls, drv = raster()
    one = device_run(env, tables()[:1], cls, drv)
    seven = device_run(env, np.repeat(tables()[:1], 7, axis=0), cls, drv)
    for k in (0, 1):
        assert parity.same_bits(seven[k], one[k]), NAMES[k]
        assert np.isfinite(one[k]).sum() > 0.9 * N
    assert (seven[2][np.isfinite(seven[0])] == 0).all()
    assert (seven[3][np.isfinite(seven[1])] == 0).all()
    assert (seven[4][np.isfinite(seven[0]) & np.isfinite(seven[1])] == 0).all()
    for k in (2, 3, 4):
        assert parity.same_bits(seven[k], one[k]), NAMES[k]      # (NaN where the mean is NaN)


def test_two_launches_give_the_same_bits(env):
    cls, drv = raster()
    a = device_run(env, tables(), cls, drv)
    b = device_run(env, tables(), cls, drv)
    for x, y, name in zip(a, b, NAMES):
        assert parity.same_bits(x, y), name


def test_special_values(env):
    """Each of the 18 special values in each of the 14 drivers, one pixel apiece among ordinary ones
    (252 of 4096), D = 5: the flagged-pixel path. Two more pixels carry a SIGNALLING NaN (pressure,
    vpd_night) next to an infinite sw_rad_day: it must not hide the infinity from the guard."""
    torch, m16, _lib, RasterEngine = env
    from fuzz_special_values import SPECIAL
    assert len(SPECIAL) == 18
    n = 4096
    cls, drv = synth.drivers((n,), seed=5)
    drv = [d.copy() for d in drv]
    at = 7 + 16 * np.arange(14 * len(SPECIAL))
    for j in range(14):
        for s, v in enumerate(SPECIAL):
            drv[j][at[j * len(SPECIAL) + s]] = v
    snan = np.array([0x7ff0000000000001], np.uint64).view(np.float64)[0]
    drv[11][4090], drv[2][4090] = snan, np.inf
    drv[10][4092], drv[2][4092] = snan, np.inf
    assert drv[11].view(np.uint64)[4090] == 0x7ff0000000000001      # (numpy kept the bit pattern)
    cls = cls.copy()
    cls[at] = np.array(oracle.PFT_VALID, np.uint8)[np.arange(at.size) % 11]
    cls[[4090, 4092]] = 1
    tabs = tables()[:5]
    days, nights = members_of(tabs, cls, drv)
    special = np.zeros(n, bool)
    special[at] = True
    assert np.isfinite(days[:, special]).any() and np.isnan(days[:, special]).any()
    for math, flag in (('fast', _lib.MATH_FAST), ('exact', _lib.MATH_EXACT)):
        got = device_run(env, tabs, cls, drv, math=flag)
        check(got, days, nights, 'special values, ' + math)
        host = host_run(m16, tabs, cls, drv, math=flag)
        for x, y, name in zip(host, got, NAMES):
            assert parity.same_bits(x, y), (math, name)


def test_tables_with_holes(env):
    """One member whose row for class 4 is NaN: class-4 pixels are NaN in all five outputs, the other
    classes are untouched. A class code 13 raises IndexError: from the HOST call, and from check()
    behind the DEVICE call."""
    torch, m16, _lib, RasterEngine = env
    n = 4096
    cls, drv = synth.drivers((n,), seed=9)
    tabs = tables()[:5].copy()
    whole = host_run(m16, tabs, cls, drv)
    tabs[3, 4, :] = np.nan
    holed = host_run(m16, tabs, cls, drv)
    c4 = cls == 4
    assert c4.sum() > 100
    for a, b, name in zip(holed, whole, NAMES):
        assert np.isnan(a[c4]).all(), name
        assert parity.same_bits(a[~c4], b[~c4]), name
        assert np.isfinite(b[c4]).sum() > 0.9 * c4.sum(), name
    bad = cls.copy()
    bad[1234] = 13
    with pytest.raises(IndexError):
        host_run(m16, tabs, bad, drv)
    eng = RasterEngine(base_table())
    ens = eng.ensemble(tabs)
    out = ens.run(torch.from_numpy(bad).cuda(), [torch.from_numpy(d).cuda() for d in drv])
    with pytest.raises(IndexError):
        eng.check()
    res = [t.cpu().numpy() for t in out]
    assert all(np.isnan(r[1234]) for r in res)
    keep = np.arange(n) != 1234
    assert all(parity.same_bits(r[keep], h[keep]) for r, h in zip(res, holed))
    eng.check()         # (the status word was cleared)


def test_float32_storage(env):
    """float32 drivers: float64 arithmetic and accumulation, one rounding on store -- the float64
    engine on the same values widened, rounded to float32, bit for bit. Both arithmetics."""
    torch, m16, _lib, RasterEngine = env
    cls, drv = synth.drivers((N,), seed=21, dtype=np.float32)
    wide = [d.astype(np.float64) for d in drv]
    tabs = tables()[:5]
    for math in (_lib.MATH_FAST, _lib.MATH_EXACT):
        got = device_run(env, tabs, cls, drv, math=math, dtype='float32')
        want = device_run(env, tabs, cls, wide, math=math)
        for g, w, name in zip(got, want, NAMES):
            assert g.dtype == np.float32
            assert parity.same_bits(g, w.astype(np.float32)), name
        host = host_run(m16, tabs, cls, drv, math=math)
        assert all(h.dtype == np.float32 and parity.same_bits(h, g) for h, g in zip(host, got))
    assert np.isfinite(got[2]).sum() > 0.9 * N and (got[2][np.isfinite(got[2])] > 0).mean() > 0.9


def test_one_kernel_behind_every_door(env):
    """DEVICE, HOST small path and HOST staged path: the same bits. Once across a staging tile
    (mod16_host_tile_pixels() + 5 pixels, D = 2), compared with the DEVICE result only."""
    torch, m16, _lib, RasterEngine = env
    n = 4096
    cls, drv = synth.drivers((n,), seed=13)
    tabs = tables()[:5]
    dev = device_run(env, tabs, cls, drv)
    small = host_run(m16, tabs, cls, drv)
    staged = parity.in_a_fresh_thread(lambda: host_run(m16, tabs, cls, drv), {'MOD16_SMALL_PIXELS': '0'})
    days, nights = members_of(tabs, cls, drv)
    check(dev, days, nights, 'device', plain=True)
    for a, b, c, name in zip(dev, small, staged, NAMES):
        assert parity.same_bits(a, b) and parity.same_bits(a, c), name
    # scalars broadcast, and scalars in give scalars out
    scal = [d if k % 3 else float(d[0]) for k, d in enumerate(drv)]
    dense = [d if k % 3 else np.full(n, d[0]) for k, d in enumerate(drv)]
    for a, b in zip(host_run(m16, tabs, cls, scal), host_run(m16, tabs, cls, dense)):
        assert parity.same_bits(a, b)
    one = host_run(m16, tabs, int(cls[3]), [float(d[3]) for d in drv])
    assert all(np.ndim(v) == 0 for v in one) and parity.same_bits(np.array(one), np.array([s[3] for s in small]))
    assert type(one).__name__ == 'EnsembleET' and one.std_total == one[4]
    # across a staging tile
    big = int(_lib.load().mod16_host_tile_pixels()) + 5
    cls, drv = synth.drivers((big,), seed=14)
    dev = device_run(env, tables()[:2], cls, drv)
    host = host_run(m16, tables()[:2], cls, drv)
    for a, b, name in zip(dev, host, NAMES):
        assert parity.same_bits(a, b), name
    assert np.isfinite(dev[4][-5:]).any()


def test_refusals(env):
    """No members, too many members, the mixed arithmetic and the trusted flag: a Mod16Error that
    carries the message include/mod16_hip.h states."""
    torch, m16, _lib, RasterEngine = env
    header = ' '.join(open(os.path.join(ROOT, 'include', 'mod16_hip.h')).read().replace(' * ', ' ').split())
    cls, drv = synth.drivers((256,), seed=3)
    members = 'mod16_ensemble_create: members must be between 1 and 65536'
    mixed = 'MOD16_MATH_MIXED is not available for the ensemble run'
    trusted = 'MOD16_DOMAIN_TRUSTED is not available for the ensemble run'
    for msg in (members, mixed, trusted):
        assert msg in header, msg
    with pytest.raises(_lib.Mod16Error, match=members):
        host_run(m16, np.zeros((0, 13, 11)), cls, drv)
    with pytest.raises(_lib.Mod16Error, match=members):
        host_run(m16, np.broadcast_to(base_table(), (65537, 13, 11)), cls, drv)
    with pytest.raises(_lib.Mod16Error, match=mixed):
        host_run(m16, tables()[:2], cls, drv, math=_lib.MATH_MIXED)
    with pytest.raises(_lib.Mod16Error, match=trusted):
        host_run(m16, tables()[:2], cls, drv, math=_lib.MATH_FAST | _lib.DOMAIN_TRUSTED)
    f32 = [d.astype(np.float32) for d in drv]
    for eng, msg in ((RasterEngine(base_table(), dtype='float32', math=_lib.MATH_MIXED), mixed),
                     (RasterEngine(base_table(), trusted=True), trusted)):
        ens = eng.ensemble(tables()[:2])
        d = f32 if eng.np_dtype == np.float32 else drv
        with pytest.raises(_lib.Mod16Error, match=msg):
            ens.run(torch.from_numpy(cls).cuda(), [torch.from_numpy(x).cuda() for x in d])
    # 65536 members are accepted (128 MiB of tables); one pixel of them
    out = host_run(m16, np.broadcast_to(base_table(), (65536, 13, 11)), cls[:1], [d[:1] for d in drv])
    one = host_run(m16, base_table()[None], cls[:1], [d[:1] for d in drv])
    assert parity.same_bits(out.mean_day, one.mean_day) and (np.isnan(out.std_day) | (out.std_day == 0)).all()
