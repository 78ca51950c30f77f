"""mod16_amd.calibration.ensemble_tables (no GPU): from posteriors to the parameter tables of an
ensemble forward run -- joint draws without replacement, seeded per PFT, base rows elsewhere."""
import numpy as np
import pytest

from mod16_amd import calibration as cal

FREE = ['gl_sh', 'csl', 'beta']
COLS = [cal.PARAM_NAMES.index(k) for k in FREE]
CHAINS, DRAWS = 3, 40


@pytest.fixture(scope='module')
def base():
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    return bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)


def samples(pft, chains=CHAINS, draws=DRAWS):
    """Distinct values everywhere: value = f(parameter, chain, draw), so a tuple names its pool index."""
    c, k = np.meshgrid(np.arange(chains), np.arange(draws), indexing='ij')
    return {name: 1000.0 * (j + 1) + 100.0 * pft + c * draws + k + 0.25 for j, name in enumerate(FREE)}


def as_trace(s):
    shape = next(iter(s.values())).shape
    z = np.zeros(shape)
    return cal.Trace(list(s), s, z, z, np.ones(shape, bool), np.ones(shape[0]), np.ones(shape[0]))


def pool_index(row, pft):
    """The pool index (chain * k + draw) each free parameter of a member's row came from."""
    return [int(round(row[col] - 1000.0 * (j + 1) - 100.0 * pft - 0.25)) for j, col in enumerate(COLS)]


def test_members_are_joint_draws_without_repeats(base):
    post = {1: samples(1), 7: as_trace(samples(7))}
    t = cal.ensemble_tables(base, post, 50, seed=3)
    assert t.shape == (50, 13, 11) and t.dtype == np.float64
    for pft in (1, 7):
        picks = []
        for m in range(50):
            idx = pool_index(t[m, pft], pft)
            assert idx[0] == idx[1] == idx[2], 'one pool index serves all free parameters of a member'
            assert 0 <= idx[0] < CHAINS * DRAWS
            # ... and the row IS that column tuple of the pool, chain-major
            c, k = divmod(idx[0], DRAWS)
            assert [t[m, pft, col] for col in COLS] == [samples(pft)[name][c, k] for name in FREE]
            picks.append(idx[0])
        assert len(set(picks)) == 50, 'no repeats within a PFT'
    assert pool_index(t[0, 1], 1) != pool_index(t[0, 7], 7) or pool_index(t[1, 1], 1) != pool_index(t[1, 7], 7)


def test_seed_decides_the_bits(base):
    post = {1: samples(1), 7: samples(7)}
    a = cal.ensemble_tables(base, post, 20, seed=5)
    b = cal.ensemble_tables(base, post, 20, seed=5)
    c = cal.ensemble_tables(base, post, 20, seed=6)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes()
    # the stream of a PFT is default_rng([seed, pft]): PFT 7 draws the same with or without PFT 1 there
    d = cal.ensemble_tables(base, {7: samples(7)}, 20, seed=5)
    assert np.array_equal(a[:, 7], d[:, 7])
    want = np.random.default_rng([5, 7]).choice(CHAINS * DRAWS, size=20, replace=False)
    assert [pool_index(r, 7)[0] for r in a[:, 7]] == list(want)


def test_burn_and_thin(base):
    burn, thin = 10, 3
    kept = len(range(burn, DRAWS, thin))
    for post in ({4: samples(4)}, {4: as_trace(samples(4))}):
        t = cal.ensemble_tables(base, post, CHAINS * kept, burn=burn, thin=thin)
        draws = sorted(pool_index(r, 4)[0] for r in t[:, 4])
        # the whole pool, once each: every chain's draws burn, burn + thin, ...
        assert draws == sorted(c * DRAWS + k for c in range(CHAINS) for k in range(burn, DRAWS, thin))
        with pytest.raises(ValueError, match='pool'):
            cal.ensemble_tables(base, post, CHAINS * kept + 1, burn=burn, thin=thin)
    # chain-major pooling: pool index j of the kept draws is chain j // kept, kept draw j % kept
    want = np.random.default_rng([0, 4]).choice(CHAINS * kept, size=5, replace=False)
    t = cal.ensemble_tables(base, {4: samples(4)}, 5, burn=burn, thin=thin)
    assert [pool_index(r, 4)[0] for r in t[:, 4]] == [(j // kept) * DRAWS + burn + (j % kept) * thin for j in want]


def test_everything_else_is_the_base(base):
    t = cal.ensemble_tables(base, {1: samples(1), 7: samples(7)}, 9)
    fixed = [j for j in range(11) if j not in COLS]
    for m in range(9):
        for pft in range(13):
            cols = fixed if pft in (1, 7) else range(11)
            assert np.array_equal(t[m, pft, cols], base[pft, cols], equal_nan=True), (m, pft)
    assert np.isnan(t[:, [0, 11]]).all() and np.isnan(base[[0, 11]]).all()
    assert not np.shares_memory(t, base)
    # no posterior at all: copies of the base
    assert np.array_equal(cal.ensemble_tables(base, {}, 3), np.repeat(base[None], 3, axis=0), equal_nan=True)


def test_refusals(base):
    with pytest.raises(ValueError, match='pool'):
        cal.ensemble_tables(base, {1: samples(1)}, CHAINS * DRAWS + 1)
    with pytest.raises(ValueError, match=r'\(13, 11\)'):
        cal.ensemble_tables(base[:, :10], {1: samples(1)}, 4)
    with pytest.raises(ValueError, match=r'\(13, 11\)'):
        cal.ensemble_tables(base[None], {1: samples(1)}, 4)
    with pytest.raises(ValueError, match='shape'):
        cal.ensemble_tables(base, {1: {'gl_sh': np.zeros(30)}}, 4)
    ragged = samples(1)
    ragged['csl'] = ragged['csl'][:, :-1]
    with pytest.raises(ValueError, match='shape'):
        cal.ensemble_tables(base, {1: ragged}, 4)
    with pytest.raises(ValueError, match='unknown parameter'):
        cal.ensemble_tables(base, {1: {'gl': np.zeros((2, 8))}}, 4)
    with pytest.raises(ValueError, match='PFT'):
        cal.ensemble_tables(base, {13: samples(1)}, 4)
    with pytest.raises(ValueError):
        cal.ensemble_tables(base, {1: samples(1)}, 0)
    with pytest.raises(ValueError):
        cal.ensemble_tables(base, {1: samples(1)}, 4, thin=0)
