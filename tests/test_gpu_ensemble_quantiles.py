"""GPU tests of the per-pixel quantiles and the per-member outputs of the ensemble run
(mod16_et_ensemble_quantiles_*, mod16_et_ensemble_members_*; EnsembleRun.quantiles / .run_members,
mod16_amd.evapotranspiration_ensemble_quantiles).

Two yardsticks. (1) The oracle's member loop followed by np.quantile(..., axis=0), to 1e-8 * scale
(scale = max_m |x_m|; for the total max_m (|day_m| + |night_m|)): the bound the project holds every
FAST member value to (tests/test_gpu_raster.py); order statistics and their linear interpolation are
1-Lipschitz in the largest member error; numpy's own interpolation adds under 4e-16 scale
(tests/test_ensemble_quantiles_host.py). Where scale is 0 the values are exactly 0. (2) The statement
mod16_amd.calibration.ensemble_quantile applied to the GPU's OWN members (run_members): equal as
numbers (-0 equals +0), NaN in the same places -- the selection is exact."""
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import mod16_oracle as oracle
from oracle import synth
import parity
from test_gpu_ensemble import base_table, members_of, tables

pytestmark = pytest.mark.gpu

N = 4096 + 37            # 16 whole batches of the member kernel and a ragged one
N_WIDE = 1024 + 37       # the rasters of the wide ensembles (D >= 64) and of the chunked runs
Q6 = (0, 0.05, 1 / 3, 0.5, 0.95, 1)
SERIES = ('day', 'night', 'total')
_cache = {}


@pytest.fixture(scope='module')
def env():
    import torch
    import mod16_amd
    from mod16_amd import _lib
    from mod16_amd.raster import RasterEngine
    return torch, mod16_amd, _lib, RasterEngine


def raster(n=N, seed=11, dtype=np.float64):
    key = ('raster', n, seed, np.dtype(dtype).name)
    if key not in _cache:
        cls, drv = synth.drivers((n,), seed=seed, dtype=dtype)
        for a in [cls] + list(drv):
            a.setflags(write=False)
        _cache[key] = (cls, tuple(drv))
    return _cache[key]


def reference_members():
    """The oracle's 33 members of the base raster, computed once and left unchanged."""
    if 'ref' not in _cache:
        cls, drv = raster()
        days, nights = members_of(tables(), cls, drv)
        days.setflags(write=False)
        nights.setflags(write=False)
        _cache['ref'] = (days, nights)
    return _cache['ref']


def series_of(days, nights):
    """-> ((name, members, scale), ...) of the three series"""
    with np.errstate(all='ignore'):
        return (('day', days, np.abs(days).max(axis=0)), ('night', nights, np.abs(nights).max(axis=0)),
                ('total', days + nights, (np.abs(days) + np.abs(nights)).max(axis=0)))


def on_device(env, tabs, cls, drv, math=None, dtype='float64'):
    torch, m16, _lib, RasterEngine = env
    eng = RasterEngine(base_table(), dtype=dtype, math=_lib.MATH_FAST if math is None else math)
    ens = eng.ensemble(tabs)
    c = torch.from_numpy(np.array(cls)).cuda()
    d = [torch.from_numpy(np.array(x)).cuda() for x in drv]
    return eng, ens, c, d


def device_quantiles(env, tabs, cls, drv, q=Q6, math=None, dtype='float64', slab_bytes=None):
    eng, ens, c, d = on_device(env, tabs, cls, drv, math, dtype)
    out = ens.quantiles(c, d, q, slab_bytes=slab_bytes)
    eng.check()
    res = [t.cpu().numpy() for t in out]
    ens.close()
    assert all(r.shape == (np.size(q), len(cls)) for r in res)
    return res


def device_members(env, tabs, cls, drv, math=None, dtype='float64'):
    eng, ens, c, d = on_device(env, tabs, cls, drv, math, dtype)
    out = ens.run_members(c, d)
    eng.check()
    res = [t.cpu().numpy() for t in out]
    ens.close()
    assert all(r.shape == (len(tabs), len(cls)) for r in res)
    return res


def device_means(env, tabs, cls, drv, math=None, dtype='float64'):
    eng, ens, c, d = on_device(env, tabs, cls, drv, math, dtype)
    out = ens.run(c, d)
    eng.check()
    res = [t.cpu().numpy() for t in out[:2]]
    ens.close()
    return res


def host_quantiles(m16, tabs, cls, drv, q=Q6, **kw):
    return m16.evapotranspiration_ensemble_quantiles(tabs, cls, *drv, q=q, **kw)


def same_numbers(a, b):
    """Equal as numbers (-0 equals +0), NaN in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and (a[~na] == b[~nb]).all())


def check_against_numpy(got, days, nights, what, where=None):
    """Yardstick (1) on the pixels `where` (default: all): np.quantile of the oracle's members."""
    worst = 0.0
    for g, (name, x, scale) in zip(got, series_of(days, nights)):
        with np.errstate(all='ignore'):
            want = np.quantile(x, Q6, axis=0)
        sel = np.ones(x.shape[1], bool) if where is None else where
        g, want, scale = g[:, sel], want[:, sel], scale[sel]
        assert g.dtype == np.float64 and g.shape == want.shape, (what, name)
        assert np.array_equal(np.isnan(g), np.isnan(want)), '%s %s: NaN masks differ from numpy\'s' % (what, name)
        ok = ~np.isnan(want[0])
        err = np.abs(g[:, ok] - want[:, ok])
        pos = scale[ok] > 0
        rel = (err[:, pos] / scale[ok][pos]).max() if pos.any() else 0.0
        worst = max(worst, rel)
        print('%s %s: max |got - np.quantile| / scale = %.3e over %d pixels' % (what, name, rel, int(ok.sum())))
        assert (err <= 1e-8 * scale[ok]).all(), '%s %s: %.3e x scale' % (what, name, rel)
        assert (g[:, ok][:, ~pos] == 0).all(), (what, name)
    return worst


def check_against_statement(got, mem_day, mem_night, what, q=Q6):
    """Yardstick (2): the statement on the GPU's own members."""
    from mod16_amd.calibration import ensemble_quantile
    mem_day, mem_night = mem_day.astype(np.float64), mem_night.astype(np.float64)
    with np.errstate(all='ignore'):
        total = mem_day + mem_night
    for g, x, name in zip(got, (mem_day, mem_night, total), SERIES):
        want = ensemble_quantile(x, q).astype(g.dtype)
        assert same_numbers(g, want), '%s %s: %d values differ from the statement' % (
            what, name, int((~((g == want) | (np.isnan(g) & np.isnan(want)))).sum()))
        assert np.isnan(g[:, np.isnan(x).any(axis=0)]).all(), (what, name)


@pytest.mark.parametrize('math', ['fast', 'exact'])
@pytest.mark.parametrize('D', [1, 2, 5, 17, 33])
def test_parity_with_the_oracle_member_loop(env, D, math):
    torch, m16, _lib, RasterEngine = env
    cls, drv = raster()
    days, nights = reference_members()
    got = device_quantiles(env, tables()[:D], cls, drv, math=_lib.MATH_EXACT if math == 'exact' else _lib.MATH_FAST)
    assert not np.isinf(days).any() and not np.isinf(nights).any()
    check_against_numpy(got, days[:D], nights[:D], 'D = %d, %s' % (D, math))
    nan = np.isnan(got[2][0])
    assert 100 < nan.sum() < 140
    if D >= 17:        # a wrong position would show: the 5-95 % band is 16-24 % of the median
        ok = ~nan & (got[2][3] > 0)
        band = np.median((got[2][4][ok] - got[2][1][ok]) / got[2][3][ok])
        assert 0.1 < band < 0.3, band


@pytest.mark.parametrize('D', [1, 2, 16, 17, 33, 64, 256])
def test_the_selection_is_exact(env, D):
    """Every capacity of the selection kernel (16, 32, 64, 128 of them idle here, 256: the 128 KiB
    LDS instance, which must launch), full and ragged columns."""
    n = N if D < 64 else N_WIDE
    cls, drv = raster(n)
    tabs = tables()[:D] if D <= 33 else tables(D)
    got = device_quantiles(env, tabs, cls, drv)
    mem = device_members(env, tabs, cls, drv)
    check_against_statement(got, mem[0], mem[1], 'D = %d' % D)
    assert np.isfinite(got[2]).all(axis=0).sum() > 0.9 * n


def test_the_selection_is_exact_with_ties_and_128_members(env):
    cls, drv = raster(N_WIDE)
    # 17 members drawn from 5 distinct tables: every finite pixel has ties
    tabs = tables()[:5][np.arange(17) % 5]
    got = device_quantiles(env, tabs, cls, drv)
    mem = device_members(env, tabs, cls, drv)
    for x in mem:
        s = np.sort(x, axis=0)
        fin = np.isfinite(x).all(axis=0)
        assert fin.sum() > 0.9 * N_WIDE and (s[1:, fin] == s[:-1, fin]).sum(axis=0).min() >= 12
    check_against_statement(got, mem[0], mem[1], 'ties')
    # the 128-member capacity, ragged (100 members)
    tabs = tables(100)
    got = device_quantiles(env, tabs, cls, drv)
    mem = device_members(env, tabs, cls, drv)
    check_against_statement(got, mem[0], mem[1], 'D = 100')


@pytest.mark.parametrize('math', ['fast', 'exact'])
def test_run_members(env, math):
    """Row m is mean_day / mean_night of the one-member ensemble of tables[m], bit for bit."""
    torch, m16, _lib, RasterEngine = env
    flag = _lib.MATH_EXACT if math == 'exact' else _lib.MATH_FAST
    cls, drv = raster()
    tabs = tables()[:17]
    day, night = device_members(env, tabs, cls, drv, math=flag)
    for m in (0, 1, 15, 16):
        one = device_means(env, tabs[m:m + 1], cls, drv, math=flag)
        assert parity.same_bits(day[m], one[0]) and parity.same_bits(night[m], one[1]), m
    assert np.isfinite(day).all(axis=0).sum() > 0.9 * N
    days, nights = reference_members()
    for got, want in ((day, days[:17]), (night, nights[:17])):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= 1e-8 * np.abs(want[ok])).all()


@pytest.mark.parametrize('math', ['fast', 'exact'])
def test_float32_storage(env, math):
    """float32 drivers: members, sum, order and interpolation in float64, one rounding on store --
    the float64 engine on the widened drivers, rounded to float32, bit for bit."""
    torch, m16, _lib, RasterEngine = env
    flag = _lib.MATH_EXACT if math == 'exact' else _lib.MATH_FAST
    cls, drv = raster(N, seed=21, dtype=np.float32)
    wide = [d.astype(np.float64) for d in drv]
    tabs = tables()[:17]
    got = device_members(env, tabs, cls, drv, math=flag, dtype='float32')
    want = device_members(env, tabs, cls, wide, math=flag)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and parity.same_bits(g, w.astype(np.float32))
    got = device_quantiles(env, tabs, cls, drv, math=flag, dtype='float32')
    wantq = device_quantiles(env, tabs, cls, wide, math=flag)
    for g, w, name in zip(got, wantq, SERIES):
        assert g.dtype == np.float32 and parity.same_bits(g, w.astype(np.float32)), name
    host = host_quantiles(m16, tabs, cls, drv, math=flag)
    for h, g, name in zip(host[1:], got, SERIES):
        assert h.dtype == np.float32 and parity.same_bits(h, g), name
    assert np.isfinite(got[2]).all(axis=0).sum() > 0.9 * N


def test_identical_members(env):
    cls, drv = raster()
    one = device_means(env, tables()[:1], cls, drv)
    got = device_quantiles(env, np.repeat(tables()[:1], 7, axis=0), cls, drv)
    with np.errstate(all='ignore'):
        for g, want in zip(got, (one[0], one[1], one[0] + one[1])):
            for k in range(len(Q6)):
                assert same_numbers(g[k], want)
    # q = 0 and q = 1 are the smallest and the largest member; the quantiles do not decrease with q
    tabs = tables()[:17]
    got = device_quantiles(env, tabs, cls, drv)
    mem = device_members(env, tabs, cls, drv)
    with np.errstate(all='ignore'):
        for g, x in zip(got, (mem[0], mem[1], mem[0] + mem[1])):
            fin = ~np.isnan(x).any(axis=0)
            assert np.array_equal(g[0][fin], x.min(axis=0)[fin]) and np.array_equal(g[-1][fin], x.max(axis=0)[fin])
            assert (np.diff(g[:, fin], axis=0) >= 0).all()
            assert (g[-1][fin] > g[0][fin]).mean() > 0.9


def test_special_values(env):
    """Each of the 18 special values in each of the 14 drivers, one pixel apiece among ordinary ones
    (252 of 4096; the layout of tests/test_gpu_ensemble.py::test_special_values, with its two
    signalling-NaN pixels), D = 5: the flagged-pixel path of the member kernel."""
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
    assert drv[11].view(np.uint64)[4090] == 0x7ff0000000000001
    cls = cls.copy()
    cls[at] = np.array(oracle.PFT_VALID, np.uint8)[np.arange(at.size) % 11]
    cls[[4090, 4092]] = 1
    tabs = tables()[:5]
    days, nights = members_of(tabs, cls, drv)
    special = np.zeros(n, bool)
    special[at] = True
    assert np.isfinite(days[:, special]).any() and np.isnan(days[:, special]).any()
    with np.errstate(all='ignore'):
        finite = np.isfinite(days).all(axis=0) & np.isfinite(nights).all(axis=0) & np.isfinite(days + nights).all(axis=0)
    assert (finite & special).sum() > 20
    for math, flag in (('fast', _lib.MATH_FAST), ('exact', _lib.MATH_EXACT)):
        got = device_quantiles(env, tabs, cls, drv, math=flag)
        mem = device_members(env, tabs, cls, drv, math=flag)
        # a NaN member makes the series NaN (the oracle's NaN members are the GPU's)
        for g, (name, x, scale) in zip(got, series_of(days, nights)):
            assert np.isnan(g[:, np.isnan(x).any(axis=0)]).all(), (math, name)
        check_against_statement(got, mem[0], mem[1], 'special values, ' + math)
        check_against_numpy(got, days, nights, 'special values, ' + math, where=finite)
        host = host_quantiles(m16, tabs, cls, drv, math=flag)
        for h, g, name in zip(host[1:], got, SERIES):
            assert parity.same_bits(h, g), (math, name)


def test_class_codes(env):
    """One member whose row for class 4 is NaN: class-4 pixels are NaN, the others keep their bits. A
    class code 13 raises IndexError: from the HOST call, and from check() behind the DEVICE call."""
    torch, m16, _lib, RasterEngine = env
    n = 4096
    cls, drv = synth.drivers((n,), seed=9)
    tabs = tables()[:5].copy()
    whole = host_quantiles(m16, tabs, cls, drv)
    tabs[3, 4, :] = np.nan
    holed = host_quantiles(m16, tabs, cls, drv)
    c4 = cls == 4
    assert c4.sum() > 100
    for a, b, name in zip(holed[1:], whole[1:], SERIES):
        assert np.isnan(a[:, c4]).all(), name
        assert parity.same_bits(a[:, ~c4], b[:, ~c4]), name
        assert np.isfinite(b[:, c4]).sum() > 0.9 * 6 * c4.sum(), name
    bad = cls.copy()
    bad[1234] = 13
    with pytest.raises(IndexError):
        host_quantiles(m16, tabs, bad, drv)
    eng, ens, c, d = on_device(env, tabs, bad, drv)
    out = ens.quantiles(c, d, Q6)
    with pytest.raises(IndexError):
        eng.check()
    res = [t.cpu().numpy() for t in out]
    assert all(np.isnan(r[:, 1234]).all() for r in res)
    keep = np.arange(n) != 1234
    assert all(parity.same_bits(r[:, keep], h[:, keep]) for r, h in zip(res, holed[1:]))
    eng.check()         # (the status word was cleared)
    mem = ens.run_members(c, d)
    with pytest.raises(IndexError):
        eng.check()
    assert all(np.isnan(t.cpu().numpy()[:, 1234]).all() for t in mem)


def test_every_door(env):
    """DEVICE, HOST small path, HOST staged path and a DEVICE run whose slab holds one batch of 256
    pixels (five chunks, the last ragged): the same bits."""
    torch, m16, _lib, RasterEngine = env
    cls, drv = raster(N_WIDE, seed=13)
    tabs = tables()[:5]
    dev = device_quantiles(env, tabs, cls, drv)
    small = host_quantiles(m16, tabs, cls, drv)
    staged = parity.in_a_fresh_thread(lambda: host_quantiles(m16, tabs, cls, drv), {'MOD16_SMALL_PIXELS': '0'})
    chunked = device_quantiles(env, tabs, cls, drv, slab_bytes=16 * 5 * 256 + 100)
    tiny = device_quantiles(env, tabs, cls, drv, slab_bytes=1)       # raised to one batch
    assert type(small).__name__ == 'EnsembleQuantiles' and small.total is small[3]
    assert small.q.dtype == np.float64 and small.q.tolist() == list(map(float, Q6))
    for k, name in enumerate(SERIES):
        assert small[1 + k].shape == (6, N_WIDE)
        for other in (small[1 + k], staged[1 + k], chunked[k], tiny[k]):
            assert parity.same_bits(dev[k], other), name
    days, nights = members_of(tabs, cls, drv)
    check_against_numpy(dev, days, nights, 'device')
    # out= is written into and handed back; a wrong shape is refused
    outs = [np.empty((6, N_WIDE)) for _ in range(3)]
    res = host_quantiles(m16, tabs, cls, drv, out=outs)
    assert all(r is o and parity.same_bits(o, d) for r, o, d in zip(res[1:], outs, dev))
    with pytest.raises(ValueError):
        host_quantiles(m16, tabs, cls, drv, out=[np.empty((N_WIDE,)) for _ in range(3)])
    # scalars broadcast; all-scalar input gives (Q,)
    scal = [d if k % 3 else float(d[0]) for k, d in enumerate(drv)]
    dense = [d if k % 3 else np.full(N_WIDE, d[0]) for k, d in enumerate(drv)]
    for a, b in zip(host_quantiles(m16, tabs, cls, scal)[1:], host_quantiles(m16, tabs, cls, dense)[1:]):
        assert parity.same_bits(a, b)
    one = host_quantiles(m16, tabs, int(cls[3]), [float(d[3]) for d in drv])
    for k in range(3):
        assert one[1 + k].shape == (6,) and parity.same_bits(one[1 + k], small[1 + k][:, 3])
    med = host_quantiles(m16, tabs, cls, drv, q=0.5)                  # a scalar q is a 1-tuple
    assert med.day.shape == (1, N_WIDE) and parity.same_bits(med.total[0], small.total[3])
    # a 2-D raster keeps its shape behind the quantile axis
    grid = host_quantiles(m16, tabs, cls[:1024].reshape(32, 32), [d[:1024].reshape(32, 32) for d in drv])
    assert grid.day.shape == (6, 32, 32) and parity.same_bits(grid.day.reshape(6, -1), small.day[:, :1024])


def test_across_a_staging_tile(env):
    torch, m16, _lib, RasterEngine = env
    big = int(_lib.load().mod16_host_tile_pixels()) + 5
    cls, drv = synth.drivers((big,), seed=14)
    q = (0.25, 1.0)
    dev = device_quantiles(env, tables()[:2], cls, drv, q=q)
    host = host_quantiles(m16, tables()[:2], cls, drv, q=q)
    for a, b, name in zip(dev, host[1:], SERIES):
        assert parity.same_bits(a, b), name
    assert np.isfinite(dev[2][:, -5:]).any()


def test_two_launches_give_the_same_bits(env):
    cls, drv = raster()
    a = device_quantiles(env, tables(), cls, drv)
    b = device_quantiles(env, tables(), cls, drv)
    for x, y, name in zip(a, b, SERIES):
        assert parity.same_bits(x, y), name


def test_refusals(env):
    """Each refusal carries the message include/mod16_hip.h states."""
    import re
    torch, m16, _lib, RasterEngine = env
    header = ' '.join(open(os.path.join(ROOT, 'include', 'mod16_hip.h')).read().replace(' * ', ' ').split())
    nq = 'mod16_et_ensemble_quantiles: nq must be between 1 and 8'
    qrange = 'mod16_et_ensemble_quantiles: every q must lie in [0, 1] and not be NaN'
    wide = 'mod16_et_ensemble_quantiles: more than 256 members'
    slab = 'mod16_et_ensemble_quantiles: slab_bytes must not be negative'
    pitch = 'mod16_et_ensemble_members: pitch must be at least n'
    mixed = 'MOD16_MATH_MIXED is not available for the ensemble run'
    trusted = 'MOD16_DOMAIN_TRUSTED is not available for the ensemble run'
    other = "the ensemble was created on another device than this context's"
    for msg in (nq, qrange, wide, slab, pitch, mixed, trusted, other):
        assert msg in header, msg
    n = 256
    cls, drv = synth.drivers((n,), seed=3)
    eng, ens, c, d = on_device(env, tables()[:2], cls, drv)
    keep, dptr, dstride = eng._marshal_drivers(d, n)
    out = torch.empty((3 * 9, n), dtype=torch.float64, device='cuda')
    optr = [out[k].data_ptr() for k in range(27)]

    def call(q, e=ens._ens, slab_bytes=None, flags=_lib.MATH_FAST, where=_lib.DEVICE):
        e.quantiles(np.float64, c.data_ptr(), dptr, dstride, n, q, optr[:3 * len(q)], slab_bytes=slab_bytes,
                    flags=flags, where=where, stream=eng._stream())

    for q in ((), (0.5,) * 9):
        with pytest.raises(_lib.Mod16Error, match=re.escape(nq)):
            call(q)
    for q in ((-0.01,), (0.5, 1.0000001), (float('nan'),)):
        with pytest.raises(_lib.Mod16Error, match=re.escape(qrange)):
            call(q)
    with pytest.raises(_lib.Mod16Error, match=re.escape(slab)):
        call((0.5,), slab_bytes=-1)
    with pytest.raises(_lib.Mod16Error, match=re.escape(mixed)):
        call((0.5,), flags=_lib.MATH_MIXED)
    with pytest.raises(_lib.Mod16Error, match=re.escape(trusted)):
        call((0.5,), flags=_lib.MATH_FAST | _lib.DOMAIN_TRUSTED)
    call((0.5,) * 8)                               # eight are accepted
    eng.check()
    # more than 256 members: the ensemble exists and serves the other calls, the quantile call refuses
    many = eng.ensemble(np.broadcast_to(base_table(), (257, 13, 11)))
    with pytest.raises(_lib.Mod16Error, match=re.escape(wide)):
        many.quantiles(c, d, (0.5,))
    with pytest.raises(_lib.Mod16Error, match=re.escape(wide)):
        host_quantiles(m16, np.broadcast_to(base_table(), (257, 13, 11)), cls, drv)
    assert len(many.run(c, d)) == 5
    eng.check()
    # the Python entry points state the q rules themselves
    for q in ((), (0.5,) * 9, -0.01, float('nan')):
        with pytest.raises(ValueError):
            ens.quantiles(c, d, q)
        with pytest.raises(ValueError):
            host_quantiles(m16, tables()[:2], cls, drv, q=q)
    # per-member outputs: the mixed and the trusted form, a pitch below n
    mem = torch.empty((2, 2, n), dtype=torch.float64, device='cuda')
    for flags, msg in ((_lib.MATH_MIXED, mixed), (_lib.MATH_FAST | _lib.DOMAIN_TRUSTED, trusted)):
        with pytest.raises(_lib.Mod16Error, match=re.escape(msg)):
            ens._ens.run_members(np.float64, c.data_ptr(), dptr, dstride, n, mem[0].data_ptr(), mem[1].data_ptr(), n,
                                 flags=flags, stream=eng._stream())
    with pytest.raises(_lib.Mod16Error, match=re.escape(pitch)):
        ens._ens.run_members(np.float64, c.data_ptr(), dptr, dstride, n, mem[0].data_ptr(), mem[1].data_ptr(), n - 1,
                             stream=eng._stream())
    f32 = [x.astype(np.float32) for x in drv]
    for e2, msg in ((RasterEngine(base_table(), dtype='float32', math=_lib.MATH_MIXED), mixed),
                    (RasterEngine(base_table(), trusted=True), trusted)):
        ens2 = e2.ensemble(tables()[:2])
        dd = [torch.from_numpy(x).cuda() for x in (f32 if e2.np_dtype == np.float32 else drv)]
        with pytest.raises(_lib.Mod16Error, match=re.escape(msg)):
            ens2.quantiles(c, dd, (0.5,))
        with pytest.raises(_lib.Mod16Error, match=re.escape(msg)):
            ens2.run_members(c, dd)
    # an ensemble of another device (where there is a second one)
    if torch.cuda.device_count() > 1:
        ctx1 = _lib.Context(1)
        fn = ctx1.lib.mod16_et_ensemble_quantiles_f64
        qs = (_lib.C.c_double * 1)(0.5)
        rc = fn(ctx1.handle, ens._ens.handle, c.data_ptr(), _lib.ptr_array(dptr), _lib.i64_array(dstride), n, qs, 1,
                _lib.ptr_array(optr[:3]), 0, _lib.MATH_FAST, _lib.DEVICE, None)
        with pytest.raises(_lib.Mod16Error, match=re.escape(other)):
            ctx1.check(rc)
        ctx1.close()
