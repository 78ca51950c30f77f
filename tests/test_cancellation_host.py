"""The constructor of cancellation-class pixels and its layouts (tests/cancel_class.py), checked on
the CPU: what tests/test_gpu_cancellation.py takes for granted about its inputs."""
import numpy as np
import pytest

import cancel_class as cc

RUN_SHIFTS = (1, 3, 6)


@pytest.fixture(scope='module')
def bplut():
    return cc.tables()[1]


@pytest.fixture(scope='module', params=['drivers', 'raw drivers'])
def pool(request, bplut):
    return cc.class_pool(6000, seed=3, raw=request.param == 'raw drivers', bplut=bplut)


def test_constructed_pixels_meet_the_class_condition(pool, bplut):
    """|s A_soil r_tot| >= 4 x 320 x |numerator| in float64 on the rounded inputs, for the night's
    bare-soil quotient, and the same factor between its budget and the night total."""
    ratio, soil_night = cc.budget_ratio(bplut, pool.cls, pool.drivers64())
    assert pool.delta.max() <= 1e-4 and pool.delta.min() >= 2e-5
    assert (soil_night >= 4 * 320).all(), soil_night.min()
    assert (ratio >= 4 * 320).all(), ratio.min()
    assert all(d.dtype == np.float32 for d in pool.drv)
    drv = pool.drivers64()
    assert (drv[12] == 0).all()                                   # bare ground
    assert (oracle_rh(drv[6], drv[10]) < 0.7).all()               # a dry night


def oracle_rh(t, vpd):
    from oracle import mod16_oracle as oracle
    return oracle.rhumidity(t, vpd)


def test_their_night_total_is_a_small_positive_number(pool, bplut):
    night = pool.truth(bplut)[1]
    assert np.isfinite(night).all() and (night > 0).all()
    # ... about delta x the night total of the same pixels with the radiation balance one W m-2 from zero
    ordinary = cc.Pool(pool.cls, [d if k != 1 else np.full_like(d, -1.0) for k, d in enumerate(pool.drv)],
                       pool.raw, pool.fpar_pct, pool.lai_x10).truth(bplut)[1]
    rel = night / ordinary
    assert np.median(rel) < 3e-4 and rel.max() < 2e-3, (np.median(rel), rel.max())


def test_numpy_float32_cannot_resolve_them(pool, bplut):
    """What proves the GPU tests can fail: the oracle run entirely in float32 is off by more than 100
    float32 ulps at the median of these pixels (all have delta <= 1e-4), with the same zero mask or not."""
    truth = pool.truth(bplut)[1]
    got = pool.numpy_float32(bplut)[1]
    assert got.dtype == np.float32
    ulp = np.spacing(truth.astype(np.float32)).astype(np.float64)
    off = np.abs(got.astype(np.float64) - truth) / ulp
    print('\n[float32 numpy on %d class pixels] median %.0f ulps, maximum %.0f ulps; relative: median %.2e, maximum %.2e'
          % (len(pool), np.median(off), off.max(), np.median(np.abs(got - truth) / truth), np.max(np.abs(got - truth) / truth)))
    assert np.median(off) > 100


@pytest.mark.parametrize('raw', [False, True])
def test_background_pixels_are_clear_of_the_class(bplut, raw):
    clear = cc.clear_pool(20000, seed=5, raw=raw, bplut=bplut)
    ratio, _ = cc.budget_ratio(bplut, clear.cls, clear.drivers64())
    assert (ratio <= 320 / 4).all()
    assert np.isin(clear.cls, np.array(cc.oracle.PFT_VALID)).all()
    day, night = clear.truth(bplut)[:2]
    assert np.isfinite(day).all() and np.isfinite(night).all()


def test_ladder_pixels_are_members_up_to_the_threshold_of_the_condition(bplut):
    deltas = cc.ladder_deltas(500, seed=2)
    assert deltas.size == 2000
    for e in range(-5, -1):
        assert ((deltas >= 10.0 ** e) & (deltas < 10.0 ** (e + 1))).sum() == 500
    pool = cc.class_pool(deltas.size, delta=deltas, seed=4, bplut=bplut, hold_at=1 / 1280)
    assert np.array_equal(pool.delta, deltas)
    inside = deltas <= 1 / 1280
    assert cc.is_class(bplut, pool.cls, pool.drivers64())[inside].all()
    ratio, _ = cc.budget_ratio(bplut, pool.cls, pool.drivers64())
    assert (ratio[deltas >= 2e-2] < 320).all()                   # the far end of the ladder is outside the class
    night = pool.truth(bplut)[1]
    assert np.isfinite(night).all() and (night > 0).all()


def per_run(layout):
    run = cc.coords(layout.positions, layout.run_shift)[0]
    return np.bincount(run, minlength=-(-layout.n // layout.run_pixels))


@pytest.mark.parametrize('rs', RUN_SHIFTS)
def test_exact_cap_layouts(rs):
    for k in (32, 33):
        lay = cc.exact_cap(7, rs, k, extra=1000)
        assert lay.n == 7 * (256 << rs) + 1000
        counts = per_run(lay)
        assert (counts[:7] == k).all() and counts[7:].sum() == 0
        # spread over the run's pieces: every piece of a short run, one piece each in a long one
        run, piece, group, lane, px = cc.coords(lay.positions, rs)
        for r in range(7):
            assert np.unique(piece[run == r]).size == min(1 << rs, k)
        sim = cc.simulate(lay)
        assert len(sim) == 7
        for r in range(7):
            listed, flagged, pieces = sim[r]
            assert listed == 32 and flagged == k - 32 and len(pieces) == k - 32
    table = cc.full_table(rs)
    assert per_run(table).tolist() == [32] * 64 and table.n == 64 * (256 << rs)
    assert sum(v[0] for v in cc.simulate(table).values()) == 64 * 32          # who[]: 2048 entries exactly
    more = cc.full_table(rs, one_more=True)
    assert per_run(more).tolist() == [32] * 65


@pytest.mark.parametrize('rs', RUN_SHIFTS)
def test_straddle_layout(rs):
    lay = cc.straddle(5, rs)
    assert (per_run(lay) == 34).all()
    run, piece, group, lane, px = cc.coords(lay.positions, rs)
    for r in range(5):
        g, size = np.unique(group[run == r], return_counts=True)
        # 31 entries first (singles where the run has the groups for them), then a group of 2, then a single
        assert size[:-2].sum() == 31 and size[-2] == 2 and size[-1] == 1
        if rs == 6:
            assert (size[:-2] == 1).all()
        listed, flagged, pieces = cc.simulate(lay)[r]
        assert listed == 32 and flagged == 2 and len(pieces) == 1


def test_high_pieces_layout():
    lay = cc.high_pieces(4, extra=300)
    assert lay.run_shift == 6
    run, piece, group, lane, px = cc.coords(lay.positions, 6)
    for r in range(4):
        p = piece[run == r]
        assert (p < 2).sum() == 32 and ((p >= 2) & (p < 44)).sum() == 0 and (p >= 44).sum() == 21
        assert np.array_equal(np.unique(p[p >= 2]), np.arange(44, 64))
        listed, flagged, pieces = cc.simulate(lay)[r]
        assert listed == 32 and flagged == 21 and pieces == list(range(44, 64))   # all beyond flag bit 43


@pytest.mark.parametrize('rs', RUN_SHIFTS)
def test_dense_and_scattered_layouts(rs):
    lay = cc.dense(3, rs, extra=777)
    assert lay.positions.size == lay.n == 3 * (256 << rs) + 777
    sim = cc.simulate(lay)
    # the first ballot group of a run is 128 pixels: nothing is ever listed, every piece is flagged
    # (but for the ragged piece of the partial last run: 777 = 3 pieces + two vectors + one pixel)
    assert all(sim[r][0] == 0 for r in range(max(sim))) and sim[max(sim)][0] == 8
    assert sum(v[0] + v[1] for v in sim.values()) == lay.n // 4 * 4
    assert sim[0][2] == list(range(1 << rs))
    lad = cc.scattered(1 << 20, rs, 2000, seed=1)
    assert lad.positions.size == 2000 and np.all(np.diff(lad.positions) > 0)


@pytest.mark.parametrize('rs', RUN_SHIFTS)
@pytest.mark.parametrize('n', [4, 252, 256, 257, 512, 2047, 2048, 2053, 4355, 5 * (256 << 3) + 3 * 256 + 4 * 9 + 3])
def test_ragged_end_layout(n, rs):
    lay = cc.ragged_end(n, rs)
    pos = set(lay.positions.tolist())
    nvec = n // 4
    assert set(range(nvec * 4, n)) <= pos                          # the scalar tail, whole
    assert nvec * 4 - 1 in pos                                     # the last vector
    nfull, nrem = nvec // 64, nvec % 64
    if nfull:
        assert sum(1 for q in pos if q // 256 == nfull - 1) >= 5    # the last full piece
    if nrem:
        assert sum(1 for q in pos if q // 256 == nfull and q < nvec * 4) >= 3   # the ragged piece
    sim = cc.simulate(lay)
    assert sum(v[0] + v[1] for v in sim.values()) == sum(1 for q in pos if q < nvec * 4)


@pytest.mark.parametrize('rs', RUN_SHIFTS)
def test_mixed_company_layout(rs):
    lay = cc.mixed_company(6, rs, 65535.0, extra=12)
    assert (per_run(lay)[:6] == 4).all()
    filled = {q for q, k, v in lay.fills}
    assert not filled & set(lay.positions.tolist())
    for r in range(6):
        mine = lay.positions[cc.coords(lay.positions, rs)[0] == r]
        near = sorted(q for q in filled if q // lay.run_pixels == r)
        a, b, c, d = mine
        assert a ^ 1 in near                                        # in its pair
        assert any(q // 4 == b // 4 and q // 2 != b // 2 for q in near)      # in its lane's other pair
        assert any(q // 256 == c // 256 and q // 4 != c // 4 for q in near)  # in another lane of its piece
        assert any(q == d ^ 1 and np.isnan(v) for q, k, v in lay.fills)      # a NaN driver beside it
    assert len({q // 256 for q in lay.positions[:4].tolist()}) == 1


def test_sources_cover_the_raster():
    lay = cc.straddle(3, 3)
    bg, src = cc.sources(lay, 100, 1000, seed=1)
    assert bg.shape == (lay.n,) and bg.max() < 1000 and src.shape == lay.positions.shape and src.max() < 100
    bg2, src2 = cc.sources(lay, 100, 1000, seed=1)
    assert np.array_equal(bg, bg2) and np.array_equal(src, src2)
