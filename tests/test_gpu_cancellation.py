"""The cancellation class of the float32 mixed-precision form (MOD16_MATH_MIXED; mod16_mixed.hpp,
period_mixed) where its machinery has its cases (mod16_stream.hpp): the per-run list of kCancelCap =
32 entries filled exactly and overflowed by one, the ballot group that straddles the cap, overflow
reachable only through the last of the 44 piece-flag bits, the 64 x 32 table of
et_stream_cancel_kernel full, marked pixels in the ragged last piece, class pixels next to pixels
outside the domain, every form and every schedule, the tiled layout, a captured step, the HOST mode.

The pixels are constructed (tests/cancel_class.py: membership is a float64 condition checked on the
CPU, tests/test_cancellation_host.py). Yardsticks, all on the same float32 tensors:
    T   the float64 oracle on the widened inputs                       (the independent truth)
    F   the float32-storage FAST engine                                (the contract: include/mod16_hip.h
        promises for a class pixel "what the FAST kernel stores for it")
    U   the trusted mixed instance, which revisits nothing             (totals form only)
and what is asserted:
    no output holds kCancelPoison; at every class pixel every output is within 1 float32 ulp of F
    (the redo kernels and the FAST pipeline are different instantiations of et_pixel_fast: a last-bit
    float64 difference times 1 / delta can cross a float32 rounding boundary, no more), NaN / zero /
    inf masks those of F everywhere; U is off F by more than 1 ulp on more than half of the class
    pixels (the raster has teeth); every value of the guarded run is bit-equal to U's or within 1 ulp
    of F's; the rest within assert_mixed_parity of F; the in-kernel diagnostics are those of the
    outputs; against T the guarded run is no worse than F (+ 2^-23) on the class pixels."""
import os

import numpy as np
import pytest

import cancel_class as cc
from parity import assert_mixed_parity, bits_equal, ulps, untouched_or_redone

pytestmark = pytest.mark.gpu

FORMS = ('totals', 'sep6', 'sep8', 'pet', 'raw', 'raw scalar hours', 'raw hour array')
DYN = {'MOD16_STATIC_BELOW': '0'}
NOT_BIT_EQUAL = {}                 # layout / form / schedule -> (class pixels, of them not bit-equal to F)


class Kit(object):
    pass


@pytest.fixture(scope='module')
def kit():
    import torch
    from mod16_amd import _lib
    from mod16_amd.raster import RasterEngine
    k = Kit()
    k.torch, k.lib, k.RasterEngine = torch, _lib, RasterEngine
    k.table, k.bplut = cc.tables()
    k.pools = {}
    for raw in (False, True):
        clear = cc.clear_pool(30000, seed=11, raw=raw, bplut=k.bplut)
        klass = cc.class_pool(8000, seed=12, raw=raw, bplut=k.bplut)
        k.pools[raw] = combined(k, clear, klass)
    k.F = RasterEngine(k.table, dtype='float32')
    k.U = RasterEngine(k.table, dtype='float32', math=_lib.MATH_MIXED, trusted=True)
    k.engines = {}
    yield k
    print('\n[class pixels not bit-equal to F, per layout | form | schedule]')
    for key, (count, off) in NOT_BIT_EQUAL.items():
        print('  %-60s %8d of %9d' % (key, off, count))


def combined(k, clear, klass):
    """clear pool + class pool as device tensors, and T of every pool pixel (float64, on the device)"""
    torch = k.torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    both = lambda a, b: dev(np.concatenate([a, b]))
    c = Kit()
    c.raw, c.n_clear, c.n_class, c.klass = klass.raw, len(clear), len(klass), klass
    c.cls = both(clear.cls, klass.cls)
    c.drv = [both(a, b) for a, b in zip(clear.drv, klass.drv)]
    if klass.raw:
        c.fpar_pct, c.lai_x10 = both(clear.fpar_pct, klass.fpar_pct), both(clear.lai_x10, klass.lai_x10)
        c.hours = both(clear.hours, klass.hours)
    c.truth = [dev(np.concatenate([a, b])) for a, b in zip(clear.truth(k.bplut), klass.truth(k.bplut))]
    return c


def engine(k, switches, math=None):
    """A mixed engine (guarded) of the experiments library under the given launch-geometry switches."""
    key = tuple(sorted(switches.items()))
    if key not in k.engines:
        old = {s: os.environ.get(s) for s in switches}
        os.environ.update(switches)
        try:
            k.engines[key] = k.RasterEngine(k.table, dtype='float32', math=k.lib.MATH_MIXED, experiments=True)
        finally:
            for s, v in old.items():
                if v is None:
                    del os.environ[s]
                else:
                    os.environ[s] = v
    return k.engines[key]


def raster(k, layout, raw=False, seed=0, pool=None, in_order=False):
    """The layout as device tensors: every pixel a copy of a pool pixel."""
    torch = k.torch
    c = pool or k.pools[raw]
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    idx = torch.randint(0, c.n_clear, (layout.n,), generator=g, device='cuda')
    pos = torch.from_numpy(layout.positions).cuda()
    if in_order:
        src = torch.arange(pos.numel(), device='cuda')
    else:
        src = torch.randint(0, c.n_class, (pos.numel(),), generator=g, device='cuda')
    idx[pos] = c.n_clear + src
    r = Kit()
    r.layout, r.n, r.pos, r.src, r.pool = layout, layout.n, pos, src, c
    r.cls = c.cls[idx]
    r.drv = [d[idx] for d in c.drv]
    if c.raw:
        r.fpar_pct, r.lai_x10, r.hours = c.fpar_pct[idx], c.lai_x10[idx], c.hours[idx]
    r.touched = pos
    if layout.fills:
        where = torch.tensor([q for q, _, _ in layout.fills], device='cuda')
        for q, field, value in layout.fills:
            r.drv[field][q] = value
        r.touched = torch.cat([pos, where])
    r.truth = [t[c.n_clear + src] for t in c.truth]                # at the class positions
    return r


def run_form(k, eng, form, r, diag=None):
    """every output array of one form of the forward run, totals first where the form has them"""
    if form == 'totals':
        return list(eng.run(r.cls, r.drv, diag=diag))
    if form == 'sep6':
        out = eng.empty(r.n, 6)
        eng.run(r.cls, r.drv, None, None, out_sep=out)
        return out
    if form == 'sep8':
        day, night = eng.empty(r.n, 2)
        out = eng.empty(r.n, 6)
        eng.run(r.cls, r.drv, day, night, out_sep=out)
        return [day, night] + out
    if form == 'pet':
        return list(eng.run_pet(r.cls, r.drv))
    if form == 'raw scalar hours':
        # On device tensors the pipeline's scalar-hours instance is reached through the tiled layout
        # (run_form_tiled; run_raw with a one-element hours tensor takes the plain kernel, which is FAST).
        assert r.n % 4 == 0, 'a tiled raster holds whole vectors'
        t = eng.alloc_tiled(r.n, form=k.lib.FORM_RAW_TOTAL8)
        for dst, src in list(zip(t.wide, r.drv)) + list(zip(t.bytes, (r.cls, r.fpar_pct, r.lai_x10))):
            t.put(dst, src)
        eng.run_form_tiled(t, day_hours=11.5)
        return [t.flat(o) for o in t.outs]
    hours = {'raw': None, 'raw hour array': r.hours}[form]
    return list(eng.run_raw(r.cls, r.drv, r.fpar_pct, r.lai_x10, day_hours=hours))


def night_of(form):
    """index of the output that holds a class pixel's night value (six components: the night's soil
    evaporation -- over bare ground it is the night total)"""
    return 4 if form == 'sep6' else 1


def same_bits(torch, a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def no_poison(torch, outs, what):
    for j, o in enumerate(outs):
        hits = int((o.contiguous().view(torch.int32) == cc.POISON).sum())
        assert hits == 0, '%s: output %d holds kCancelPoison at %d pixels' % (what, j, hits)


def check_outputs(k, r, form, got, want, what, trusted=None):
    """The assertions every run of this file is held to (module docstring). ``got``: the guarded mixed
    run's outputs, ``want``: F's, ``trusted``: U's (totals form). Returns the number of class pixels
    that are not bit-equal to F."""
    torch = k.torch
    no_poison(torch, got, what)
    pos = r.pos
    off = 0
    for j, (g, w) in enumerate(zip(got, want)):
        # masks, everywhere
        for name, mask in (('NaN', torch.isnan), ('inf', torch.isinf), ('zero', lambda t: t == 0)):
            differ = int((mask(g) != mask(w)).sum())
            assert differ == 0, '%s: output %d: %s masks differ from FAST at %d pixels' % (what, j, name, differ)
        # the contract, at the class pixels
        d = ulps(torch, g[pos], w[pos])
        worst = int(d.max()) if d.numel() else 0
        assert worst <= 1, '%s: output %d: %d class pixels more than 1 ulp from FAST (worst %d ulps)' % (
            what, j, int((d > 1).sum()), worst)
        off = max(off, int((d != 0).sum()))
        # universal invariant: untouched mixed arithmetic, or a float64 redo
        if trusted is not None:
            neither = untouched_or_redone(torch, g, trusted[j], w)
            assert neither == 0, '%s: output %d: %d values are neither the trusted instance\'s nor FAST\'s' % (what, j, neither)
    # teeth: without the revisit more than half of the class pixels are off F by more than 1 ulp
    in_pipeline = pos < r.n // 4 * 4                       # (the scalar tail runs FAST in every instance)
    if trusted is not None and int(in_pipeline.sum()) >= 8:
        j = night_of(form)
        d = ulps(torch, trusted[j][pos], want[j][pos])[in_pipeline]
        assert float((d > 1).double().mean()) > 0.5, '%s: the trusted instance is within 1 ulp of FAST on %d of %d class pixels' % (
            what, int((d <= 1).sum()), d.numel())
    # everything else: the mixed form's tolerances
    keep = torch.ones(r.n, dtype=torch.bool, device='cuda')
    keep[r.touched] = False
    if bool(keep.any()):
        windows = [slice(0, r.n)] if r.n <= 5_000_000 else [slice(a, a + 2_000_000) for a in (0, r.n // 2, r.n - 2_000_000)]
        for j, (g, w) in enumerate(zip(got, want)):
            for win in windows:
                m = keep[win]
                assert_mixed_parity(g[win][m].cpu().numpy(), w[win][m].cpu().numpy(), '%s: output %d, other pixels' % (what, j))
    # the independent truth
    if pos.numel():
        j = night_of(form)
        t = r.truth[1]
        err = lambda x: float(((x[pos].double() - t).abs() / t.abs()).max())
        mine, theirs = err(got[j]), err(want[j])
        print('\n[%s] night value of %d class pixels against the float64 oracle: guarded mixed %.3e, FAST %.3e; '
              'not bit-equal to FAST: %d' % (what, pos.numel(), mine, theirs, off))
        assert mine <= theirs + 2.0 ** -23, (what, mine, theirs)
    seen, differ = NOT_BIT_EQUAL.get(what, (0, 0))                # (the sizes of a ragged-end case add up)
    NOT_BIT_EQUAL[what] = (seen + int(pos.numel()), differ + off)
    return off


def check_diag(k, eng, diag, day, night, what):
    want = eng.diagnostics(day, night)
    eng.check()
    d, w = diag.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(d[2:], w[2:]), (what, d, w)             # counts and maxima exactly
    np.testing.assert_allclose(d[:2], w[:2], rtol=1e-12, err_msg=what)


def cell(k, layout, form, switches, seed=0):
    torch = k.torch
    raw = form.startswith('raw')
    r = raster(k, layout, raw=raw, seed=seed)
    eng = engine(k, switches)
    what = '%s | %s | %s' % (layout.name, form, ' '.join('%s=%s' % kv for kv in sorted(switches.items())) or 'default')
    diag = torch.zeros(8, dtype=torch.float64, device='cuda') if form == 'totals' else None
    got = run_form(k, eng, form, r, diag)
    eng.check()
    want = run_form(k, k.F, form, r)
    k.F.check()
    trusted = None
    if form == 'totals':
        trusted = run_form(k, k.U, form, r)
        k.U.check()
    check_outputs(k, r, form, got, want, what, trusted)
    if diag is not None:
        check_diag(k, eng, diag, got[0], got[1], what)
        # a second launch: same bits, outputs and diagnostics
        first = [g.clone() for g in got]
        d2 = torch.zeros(8, dtype=torch.float64, device='cuda')
        eng.run(r.cls, r.drv, got[0].fill_(7.0), got[1].fill_(7.0), diag=d2)
        eng.check()
        assert same_bits(torch, got[0], first[0]) and same_bits(torch, got[1], first[1]), what
        assert bool(torch.equal(d2.view(torch.int64), diag.view(torch.int64))), (what, d2, diag)
    return r, eng, got, want


RS1 = dict(DYN, MOD16_RUN_SHIFT='1')
RS3 = dict(DYN, MOD16_RUN_SHIFT='3')
RS6 = dict(DYN, MOD16_RUN_SHIFT='6')
STATIC64 = {'MOD16_STATIC_BELOW': '64'}
ONE_BLOCK = {'MOD16_STREAM_BLOCKS': '1'}

# layout, form, schedule. Every layout at least once, every form and every schedule at least twice:
# default (small: static; 34 M pixels: dynamic, runs of 8 pieces on a 256-CU device), a small raster on
# the dynamic schedule, a larger one on the static schedule with more iterations per wave than flag
# bits, runs of 2 and of 64 pieces, one block per CU.
CELLS = [
    ('exact cap 32', lambda: cc.exact_cap(300, 3, 32, extra=1000), 'totals', RS3),
    ('exact cap 33', lambda: cc.exact_cap(300, 3, 33, extra=1000), 'totals', RS3),
    ('exact cap 33', lambda: cc.exact_cap(40, 6, 33, extra=5000), 'totals', RS6),
    ('straddle', lambda: cc.straddle(300, 3, extra=7 * 256 + 40), 'totals', RS3),
    ('straddle', lambda: cc.straddle(1000, 1, extra=256 + 12), 'totals', RS1),
    ('straddle', lambda: cc.straddle(40, 6, extra=3), 'totals', RS6),
    ('high pieces', lambda: cc.high_pieces(60, extra=300), 'totals', RS6),
    ('full table', lambda: cc.full_table(3), 'totals', RS3),
    ('full table + 1', lambda: cc.full_table(3, one_more=True), 'totals', RS3),
    ('full table + 1', lambda: cc.full_table(1, one_more=True), 'totals', RS1),
    ('dense', lambda: cc.dense(500, 3, extra=777), 'totals', RS3),
    ('dense', lambda: cc.dense(1000, 3, extra=777), 'totals', {}),
    ('straddle', lambda: cc.straddle(16602, 3, extra=5 * 256 + 4 * 17 + 2), 'totals', {}),
    ('scattered', lambda: cc.scattered(30_000_000 + 6, 0, 40000, seed=3, name='scattered'), 'totals', STATIC64),
    ('dense', lambda: cc.dense(4000, 0, extra=13), 'totals', ONE_BLOCK),
    ('scattered', lambda: cc.scattered(16_000_000 + 4 * 31, 0, 30000, seed=4, name='scattered'), 'sep8', dict(STATIC64, **ONE_BLOCK)),
    ('mixed company', lambda: cc.mixed_company(300, 3, 65535.0, extra=12), 'totals', RS3),
    ('mixed company', lambda: cc.mixed_company(2000, 0, -9999.0, extra=12), 'totals', {}),
    ('exact cap 33', lambda: cc.exact_cap(300, 3, 33, extra=1000), 'sep6', RS3),
    ('dense', lambda: cc.dense(1000, 3, extra=777), 'sep6', {}),
    ('mixed company', lambda: cc.mixed_company(300, 3, 65535.0, extra=12), 'sep6', RS3),
    ('high pieces', lambda: cc.high_pieces(60, extra=300), 'sep8', RS6),
    ('straddle', lambda: cc.straddle(1000, 1, extra=256 + 12), 'pet', RS1),
    ('dense', lambda: cc.dense(1000, 3, extra=777), 'pet', {}),
    ('straddle', lambda: cc.straddle(300, 3, extra=7 * 256 + 40), 'raw', RS3),
    ('dense', lambda: cc.dense(1000, 3, extra=777), 'raw', {}),
    ('exact cap 33', lambda: cc.exact_cap(300, 3, 33, extra=1000), 'raw scalar hours', RS3),
    ('scattered', lambda: cc.scattered(16_000_000 + 4 * 31, 0, 30000, seed=5, name='scattered'), 'raw scalar hours', STATIC64),
    ('high pieces', lambda: cc.high_pieces(60, extra=300), 'raw hour array', RS6),
    ('dense', lambda: cc.dense(4000, 0, extra=13), 'raw hour array', ONE_BLOCK),
]


def cell_id(c):
    return '%s-%s-%s' % (c[0].replace(' ', '_'), c[2].replace(' ', '_'),
                         '+'.join('%s%s' % (s[6:].lower(), v) for s, v in sorted(c[3].items())) or 'default')


def test_matrix_covers_every_layout_form_and_schedule():
    layouts = {c[0] for c in CELLS}
    assert {'dense', 'exact cap 32', 'exact cap 33', 'straddle', 'high pieces', 'full table', 'full table + 1',
            'mixed company'} <= layouts            # (ragged end and ladder: tests of their own below)
    for form in FORMS:
        assert sum(1 for c in CELLS if c[2] == form) >= 2, form
    for wanted in ({}, RS1, RS6, STATIC64, ONE_BLOCK):
        assert sum(1 for c in CELLS if wanted.items() <= c[3].items() and (wanted or not c[3])) >= 2, wanted
    assert sum(1 for c in CELLS if c[3].get('MOD16_STATIC_BELOW') == '0') >= 2


@pytest.mark.parametrize('c', CELLS, ids=[cell_id(c) for c in CELLS])
def test_class_pixels_get_the_fast_result(kit, c):
    name, make, form, switches = c
    layout = make()
    assert layout.name == name
    cell(kit, layout, form, switches, seed=len(form))


SIZES = [4, 252, 256, 257, 512, 2047, 2048, 2053, 4355]       # test_mixed_at_piece_and_run_boundaries


@pytest.mark.parametrize('form', ['totals', 'sep6', 'raw hour array'])
def test_marked_pixels_at_the_ragged_end(kit, form):
    """Class pixels in the last full piece, the ragged last piece, the last vector and the scalar tail
    (which runs FAST), at sizes around one vector, one piece and one run under the default (static)
    schedule, and at a size with a partial last run on the dynamic one."""
    for n in SIZES:
        cell(kit, cc.ragged_end(n, 0), form, {}, seed=n)
    # (a ragged piece of one or two vectors: lane 2, which stores a partial's flag field, computes nothing in it)
    for n, switches in ((5 * 2048 + 3 * 256 + 4 * 9 + 3, RS3), (5 * 2048 + 3 * 256 + 4 * 9 + 3, RS6), (70 * 512 + 256 + 4 * 63 + 1, RS1),
                        (5 * 2048 + 3 * 256 + 4 * 1 + 2, RS3), (5 * 2048 + 3 * 256 + 4 * 2, RS3), (70 * 512 + 4 * 2 + 1, RS1)):
        cell(kit, cc.ragged_end(n, int(switches['MOD16_RUN_SHIFT'])), form, switches, seed=n)


@pytest.mark.parametrize('make,switches', [(lambda: cc.straddle(300, 3, extra=7 * 256 + 40), RS3),
                                           (lambda: cc.high_pieces(60, extra=300 * 4), RS6),
                                           (lambda: cc.dense(1000, 3, extra=776), {})],
                         ids=['straddle-dynamic', 'high_pieces-dynamic', 'dense-default'])
def test_tiled_layout_and_captured_step(kit, make, switches):
    """The tiled layout gives the plain arrays' bits, outputs and diagnostics; a captured step
    replayed three times gives them each time."""
    torch = kit.torch
    r, eng, got, want = cell(kit, make(), 'totals', switches, seed=9)
    first = torch.zeros(8, dtype=torch.float64, device='cuda')
    eng.run(r.cls, r.drv, got[0], got[1], diag=first)
    t = eng.to_tiled(r.cls, r.drv)
    d_tiled = torch.zeros(8, dtype=torch.float64, device='cuda')
    eng.run_tiled(t, diag=d_tiled)
    eng.check()
    tiled = [t.flat(t.day), t.flat(t.night)]
    no_poison(torch, tiled, 'tiled')
    assert same_bits(torch, tiled[0], got[0]) and same_bits(torch, tiled[1], got[1])
    assert np.array_equal(d_tiled.cpu().numpy()[2:], first.cpu().numpy()[2:])
    assert np.allclose(d_tiled.cpu().numpy()[:2], first.cpu().numpy()[:2], rtol=1e-12, atol=0)
    check_diag(kit, eng, d_tiled, tiled[0], tiled[1], 'tiled')
    day, night = eng.empty(r.n, 2)
    diag = torch.zeros(8, dtype=torch.float64, device='cuda')
    step = eng.bind(r.cls, r.drv, day, night, diag, graph=True)
    for replay in range(3):
        day.fill_(7.0)
        night.fill_(7.0)
        diag.zero_()
        step()
        torch.cuda.synchronize()
        eng.check()
        assert same_bits(torch, day, got[0]) and same_bits(torch, night, got[1]), replay
        assert bool(torch.equal(diag.view(torch.int64), first.view(torch.int64))), (replay, diag, first)


@pytest.mark.parametrize('switches', [RS3, {}], ids=['dynamic', 'default'])
def test_nothing_of_a_launch_stays_in_the_workspace(kit, switches):
    """A dense raster, one with full lists, then a raster of the same size without a class pixel through the same engine:
    the second run's outputs and diagnostics are a fresh engine's, bit for bit -- no count, list or
    flag of the first launch is read again."""
    torch = kit.torch
    eng = engine(kit, switches)
    lay = cc.dense(500, 3, extra=777)
    full = raster(kit, lay, seed=21)
    none = raster(kit, cc.Layout('class-free', lay.n, 3, []), seed=22)
    lists = raster(kit, cc.straddle(500, 3, extra=777), seed=23)      # (the same size: full lists and flags)
    assert lists.n == full.n
    d0 = torch.zeros(8, dtype=torch.float64, device='cuda')
    eng.run(full.cls, full.drv, diag=d0)
    eng.run(lists.cls, lists.drv, diag=d0)
    d1 = torch.zeros(8, dtype=torch.float64, device='cuda')
    got = eng.run(none.cls, none.drv, diag=d1)
    eng.check()
    os.environ.update(switches)
    try:
        fresh = kit.RasterEngine(kit.table, dtype='float32', math=kit.lib.MATH_MIXED, experiments=True)
    finally:
        for s in switches:
            del os.environ[s]
    d2 = torch.zeros(8, dtype=torch.float64, device='cuda')
    want = fresh.run(none.cls, none.drv, diag=d2)
    fresh.check()
    no_poison(torch, got, 'class-free raster behind a dense one')
    assert same_bits(torch, got[0], want[0]) and same_bits(torch, got[1], want[1])
    assert bool(torch.equal(d1.view(torch.int64), d2.view(torch.int64))), (d1, d2)
    # (and the class-free raster is one: the trusted instance, which revisits nothing, gives the same bits)
    trusted = kit.U.run(none.cls, none.drv)
    kit.U.check()
    assert same_bits(torch, got[0], trusted[0]) and same_bits(torch, got[1], trusted[1])


def test_host_mode_over_staged_tiles(kit):
    """numpy in, numpy out (HOST mode: tiles of 2 Mi pixels staged through one workspace): the dense
    layout in the first tile, ordinary pixels in the second, the ragged-end layout at the end of the
    third."""
    import mod16_amd
    torch = kit.torch
    tile, tail = 1 << 21, 4355
    end = cc.ragged_end(tail, 3)
    lay = cc.Layout('host: dense tile + ragged end', 2 * tile + tail, 3,
                    np.concatenate([np.arange(tile), 2 * tile + end.positions]))
    r = raster(kit, lay, seed=31)
    host = lambda t: t.cpu().numpy()
    cls, drv = host(r.cls), [host(d) for d in r.drv]
    got = mod16_amd.evapotranspiration_raster(kit.table, cls, *drv, math=kit.lib.MATH_MIXED)
    want = mod16_amd.evapotranspiration_raster(kit.table, cls, *drv, math=kit.lib.MATH_FAST)
    assert got[0].dtype == np.float32 and want[0].dtype == np.float32
    dev = lambda a: torch.from_numpy(a).cuda()
    check_outputs(kit, r, 'totals', [dev(a) for a in got], [dev(a) for a in want], 'host mode | totals | default')


def test_ladder_across_the_threshold(kit):
    """delta on a log ladder from 1e-5 to 1e-1, 500 pixels per decade, scattered: deep inside the
    class, around the kernel's threshold (a budget of 320 totals) and outside. Up to delta = 1 / 1280
    the pixels meet the class condition and the contract holds; beyond it the guarded run is, decade by
    decade, no worse against T than the oracle run entirely in float32 (the criterion of
    test_gpu_mixed.py::test_f5_reference_float32_run). The per-decade maxima are printed (DESIGN.md 5.1
    has the table)."""
    torch = kit.torch
    deltas = cc.ladder_deltas(500, seed=6)
    klass = cc.class_pool(deltas.size, delta=deltas, seed=13, bplut=kit.bplut, hold_at=1 / 1280)
    clear = cc.clear_pool(30000, seed=11, bplut=kit.bplut)
    pool = combined(kit, clear, klass)
    lay = cc.scattered(1 << 20, 0, deltas.size, seed=7)
    r = raster(kit, lay, pool=pool, in_order=True)
    eng = kit.RasterEngine(kit.table, dtype='float32', math=kit.lib.MATH_MIXED)
    got = eng.run(r.cls, r.drv)
    eng.check()
    want = kit.F.run(r.cls, r.drv)
    trusted = kit.U.run(r.cls, r.drv)
    kit.F.check()
    kit.U.check()
    no_poison(torch, got, 'ladder')
    d = torch.from_numpy(deltas).cuda()
    inside = d <= 1 / 1280
    for j in (0, 1):
        for mask in (torch.isnan, torch.isinf, lambda t: t == 0):
            assert bool(torch.equal(mask(got[j]), mask(want[j])))
        off = ulps(torch, got[j][r.pos], want[j][r.pos])
        assert int(off[inside].max()) <= 1, ('ladder, delta <= 1/1280', j, int((off[inside] > 1).sum()))
        assert untouched_or_redone(torch, got[j], trusted[j], want[j]) == 0
    truth = klass.truth(kit.bplut)[1]
    rel = lambda x: np.abs(np.asarray(x, np.float64) - truth) / truth
    e_g, e_f = rel(got[1][r.pos].cpu().numpy()), rel(want[1][r.pos].cpu().numpy())
    e_u, e_np = rel(trusted[1][r.pos].cpu().numpy()), rel(klass.numpy_float32(kit.bplut)[1])
    redone = (~bits_equal(torch, got[1][r.pos], trusted[1][r.pos])).cpu().numpy()
    rows = []
    print('\n[ladder] maximum relative error of the night total against the float64 oracle, per decade of delta')
    print('  delta            pixels  revisited   guarded mixed   FAST (float32 storage)   trusted mixed   numpy float32')
    for e in range(-5, -1):
        m = (deltas >= 10.0 ** e) & (deltas < 10.0 ** (e + 1))
        rows.append((e, int(m.sum()), int(redone[m].sum()), e_g[m].max(), e_f[m].max(), e_u[m].max(), e_np[m].max()))
        print('  1e%d .. 1e%d   %6d   %6d       %.2e        %.2e                 %.2e        %.2e' % ((e, e + 1) + rows[-1][1:]))
        out = m & (deltas > 1 / 1280)
        if out.any():
            assert e_g[out].max() <= e_np[out].max(), ('outside the class, decade 1e%d' % e, e_g[out].max(), e_np[out].max())
