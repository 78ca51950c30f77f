"""mod16_amd/regress.py, the numpy definition of the per-pixel least squares (no GPU): the vectorised
statement against a plain scalar loop over the pixels, bit for bit; against numpy.linalg.lstsq within
the bound the normal equations allow; the edge pixels; the series outputs; every refusal of
check_call; the new names in the ctypes table and the header."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mod16_amd import regress as R

EPS = 2.0 ** -52
# test_definition_agrees_with_lstsq: the worst max|b - b_ref| / max|b_ref| over its cases, in units of
# cond(X)^2 * 2^-52, measured on the CPU, and the bound's constant: 8 times that
WORST_RATIO = 2.81
C_BOUND = 8 * WORST_RATIO


def f64(v):
    return np.float64(v)


def scalar_pixel(y, x, w, min_valid, stderr, series):
    """One pixel, as the module text states it: ``y`` (T,), ``x`` (T, P), ``w`` (T,) float64, samples
    with their validity decided here. -> (coef, se, rss, tss, r2, count, series values or None)."""
    T, P = x.shape
    nan = f64(np.nan)
    with np.errstate(all='ignore'):
        valid = [bool(np.isfinite(y[i]) and np.isfinite(x[i]).all() and np.isfinite(w[i]) and w[i] > 0) for i in range(T)]
        G = [[f64(0.0)] * P for _ in range(P)]
        h = [f64(0.0)] * P
        Sw = Sy = f64(0.0)
        count = 0
        for i in range(T):
            if not valid[i]:
                continue
            count += 1
            for a in range(P):
                wx = w[i] * x[i][a]
                h[a] = h[a] + wx * y[i]
                for b in range(a, P):
                    G[a][b] = G[a][b] + wx * x[i][b]
            Sw = Sw + w[i]
            Sy = Sy + w[i] * y[i]
        L = [[f64(0.0)] * P for _ in range(P)]
        d = [f64(0.0)] * P
        degenerate = False
        for j in range(P):
            dj = G[j][j]
            for k in range(j):
                dj = dj - (L[j][k] * L[j][k]) * d[k]
            d[j] = dj
            if not dj > f64(2.0 ** -40) * G[j][j]:
                degenerate = True
            for i in range(j + 1, P):
                s = G[j][i]
                for k in range(j):
                    s = s - (L[i][k] * L[j][k]) * d[k]
                L[i][j] = s / dj
        z = [f64(0.0)] * P
        for i in range(P):
            s = h[i]
            for k in range(i):
                s = s - L[i][k] * z[k]
            z[i] = s
        b = [z[i] / d[i] for i in range(P)]
        for i in range(P - 1, -1, -1):
            s = b[i]
            for k in range(i + 1, P):
                s = s - L[k][i] * b[k]
            b[i] = s
        ybar = Sy / Sw
        rss = tss = f64(0.0)
        f, r = [nan] * T, [nan] * T
        for i in range(T):
            fi = x[i][0] * b[0]
            for a in range(1, P):
                fi = fi + x[i][a] * b[a]
            f[i], r[i] = fi, y[i] - fi
            if valid[i]:
                rss = rss + w[i] * (r[i] * r[i])
                tss = tss + w[i] * ((y[i] - ybar) * (y[i] - ybar))
        r2 = f64(1.0) - rss / tss
        sigma2 = rss / f64(count - P)
        se = [nan] * P
        for j in range(P):
            M = [f64(0.0)] * P
            M[j] = f64(1.0)
            for i in range(j + 1, P):
                s = L[i][j]
                for k in range(j + 1, i):
                    s = s + L[i][k] * M[k]
                M[i] = -s
            t = (M[j] * M[j]) / d[j]
            for k in range(j + 1, P):
                t = t + (M[k] * M[k]) / d[k]
            se[j] = np.sqrt(sigma2 * t)
        empty = count < min_valid or degenerate
        if empty:
            b, se, rss, tss, r2 = [nan] * P, [nan] * P, nan, nan, nan
        out = None
        if series == 'residuals':
            out = [r[i] if valid[i] and not empty else nan for i in range(T)]
        elif series == 'fitted':
            out = [f[i] if np.isfinite(x[i]).all() and not empty else nan for i in range(T)]
    return b, (se if stderr else None), rss, tss, r2, count, out


def scalar_loop(values, design, terms, weights, min_valid, stderr, series):
    """``R.regress`` pixel by pixel through ``scalar_pixel``."""
    T, n = values.shape
    design = np.zeros((T, 0)) if design is None else np.asarray(design, np.float64)
    P = design.shape[1] + len(terms)
    min_valid = P + 1 if min_valid is None else min_valid
    coef, se = np.empty((P, n)), np.empty((P, n))
    rss, tss, r2 = np.empty(n), np.empty(n), np.empty(n)
    count = np.empty(n, np.uint16)
    out = np.empty((T, n), values.dtype)
    for p in range(n):
        x = np.concatenate([design] + [np.asarray(t[:, p], np.float64)[:, None] for t in terms], axis=1)
        w = np.ones(T) if weights is None else weights[:, p].astype(np.float64)
        b, s, rss[p], tss[p], r2[p], count[p], o = scalar_pixel(values[:, p].astype(np.float64), x, w, min_valid, stderr, series)
        coef[:, p] = b
        if stderr:
            se[:, p] = s
        if series:
            with np.errstate(all='ignore'):
                out[:, p] = np.asarray(o, np.float64).astype(values.dtype)
    return R.Regression(coef, se if stderr else None, rss, tss, r2, count, out if series else None)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == np.where(np.isnan(b), a, b).tobytes() \
        and np.array_equal(np.isnan(a), np.isnan(b))


def assert_same(got, want):
    for name, g, w in zip(R.Regression._fields, got, want):
        assert same_bits(g, w), name


def make_case(seed, T, n, Ks, Kp, dtype, weighted, missing=0.2):
    rng = np.random.default_rng(seed)
    design = None
    if Ks:
        t = np.arange(T, dtype=np.float64)
        cols = [np.ones(T)] + [np.cos(0.7 * k * t + k) + 0.1 * rng.standard_normal(T) for k in range(1, Ks)]
        design = np.stack(cols, axis=1)
    terms = [rng.standard_normal((T, n)).astype(dtype) for _ in range(Kp)]
    values = rng.standard_normal((T, n)).astype(dtype) * 3 + 10
    values[rng.random((T, n)) < missing] = np.nan
    for t in terms:
        t[rng.random((T, n)) < missing / 4] = np.nan
    if n > 2:
        values[:, 1] = np.nan                    # an empty pixel
        values[1::2, 2] = np.inf                 # infinities are missing too
    weights = None
    if weighted:
        weights = rng.random((T, n)).astype(np.float32) + 0.25
        weights[rng.random((T, n)) < 0.1] = 0.0
        weights[0, 0], weights[1, 0], weights[2, 0] = np.nan, -1.0, np.inf
    return values, design, terms, weights


SPLITS = sorted({(P, ks, P - ks) for P in (1, 2, 5, 8) for ks in (P, 0, 1)})


@pytest.mark.parametrize('P,Ks,Kp', SPLITS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('weighted', [False, True])
def test_definition_equals_the_scalar_loop(P, Ks, Kp, dtype, weighted):
    """The vectorised definition and the loop written out above give the same bits, every output."""
    values, design, terms, weights = make_case(100 * P + 10 * Ks + weighted, 19, 9, Ks, Kp, dtype, weighted)
    for series, stderr, min_valid in ((None, False, None), ('residuals', True, P), ('fitted', True, P + 3)):
        got = R.regress(values, design, terms, weights, min_valid=min_valid, stderr=stderr, series=series)
        want = scalar_loop(values, design, terms, weights, min_valid, stderr, series)
        assert_same(got, want)
        assert got.coef.shape == (P, 9) and got.count.dtype == np.uint16
        assert np.isnan(got.coef[:, 1]).all() and got.count[1] == 0


def lstsq_reference(y, X, w):
    """coef, se, rss, tss, r2 and cond(X) of one pixel by numpy.linalg.lstsq on the valid rows scaled
    by sqrt(w)."""
    s = np.sqrt(w)
    A, rhs = X * s[:, None], y * s
    b = np.linalg.lstsq(A, rhs, rcond=None)[0]
    res = rhs - A @ b
    rss = float(res @ res)
    ybar = (w * y).sum() / w.sum()
    tss = float((w * (y - ybar) ** 2).sum())
    m, P = A.shape
    se = np.sqrt(rss / (m - P) * np.diag(np.linalg.inv(A.T @ A)))
    return b, se, rss, tss, 1.0 - rss / tss, np.linalg.cond(A)


def lstsq_cases():
    """(name, values (T, n), design or None, terms, weights or None)."""
    cases = []
    for T, period, missing, seed in ((24, 12.0, 0.3, 1), (46, 46.0, 0.5, 2), (138, 46.0, 0.8, 3), (1104, 46.0, 0.4, 4),
                                     (1104, 46.0, 0.8, 5)):
        rng = np.random.default_rng(seed)
        n = 6
        t = np.arange(T, dtype=np.float64)
        harmonics = 1 if T == 24 else 2
        design = R.harmonic_design(t, period, harmonics=harmonics, trend=1)
        truth = rng.standard_normal((design.shape[1], n))
        values = design @ truth + 0.3 * rng.standard_normal((T, n)) + 5.0
        values[rng.random((T, n)) < missing] = np.nan
        weights = (rng.random((T, n)) + 0.5).astype(np.float32) if seed % 2 else None
        cases.append(('harmonic T=%d missing=%.1f' % (T, missing), values, design, [], weights))
    rng = np.random.default_rng(6)
    T, n = 60, 6
    q = np.linalg.qr(rng.standard_normal((T, 3)))[0] * np.sqrt(T)          # orthogonalised random terms
    terms = [np.repeat(q[:, k:k + 1], n, axis=1) + 0.05 * rng.standard_normal((T, n)) for k in range(3)]
    values = sum((k + 1.0) * terms[k] for k in range(3)) + 0.2 * rng.standard_normal((T, n))
    values[rng.random((T, n)) < 0.3] = np.nan
    cases.append(('orthogonalised Kp=3', values, None, terms, None))
    return cases


def lstsq_ratios(case):
    """Per pixel the four errors of the definition against lstsq in units of cond^2 * 2^-52:
    (coef, se, rss, r2)."""
    name, values, design, terms, weights = case
    got = R.regress(values, design, terms, weights, stderr=True)
    T, n = values.shape
    rows = []
    for p in range(n):
        X = np.concatenate(([design] if design is not None else []) + [t[:, p:p + 1] for t in terms], axis=1)
        w = np.ones(T) if weights is None else weights[:, p].astype(np.float64)
        v = np.isfinite(values[:, p]) & np.isfinite(X).all(axis=1)
        assert got.count[p] == v.sum() and v.sum() > X.shape[1]
        b, se, rss, tss, r2, cond = lstsq_reference(values[v, p], X[v], w[v])
        unit = cond ** 2 * EPS
        rows.append((np.abs(got.coef[:, p] - b).max() / np.abs(b).max() / unit,
                     np.abs(got.stderr[:, p] - se).max() / np.abs(se).max() / unit,
                     abs(got.rss[p] - rss) / rss / unit, abs(got.r2[p] - r2) / unit))
    return np.array(rows)


@pytest.mark.parametrize('case', lstsq_cases(), ids=lambda c: c[0])
def test_definition_agrees_with_lstsq(case):
    """max|b - b_ref| / max|b_ref| <= c * cond(X)^2 * 2^-52 against numpy.linalg.lstsq on the valid rows
    scaled by sqrt(w); stderr (relative to its largest), rss (relative to itself) and r2 (absolute) within
    the same bound. Measured on the CPU over these cases the worst ratio of the coefficients is 2.81
    (the orthogonalised case, where cond(X) is 1.1 and the unit is a few ulps; the harmonic designs reach
    2.28 at T = 1104 with 80 % missing; stderr 2.16, rss 3.50, r2 0.36), so c = 8 * 2.81 = 22.5: the margin
    covers LAPACK's other summation order."""
    ratios = lstsq_ratios(case)
    print(case[0], 'worst ratios (coef, stderr, rss, r2):', ratios.max(axis=0))
    assert (ratios <= C_BOUND).all(), ratios.max(axis=0)


def edge_stack(dtype=np.float64):
    """A (T, 8) stack of edge pixels for ``design = [1, t]`` (T = 8, P = 2, min_valid = 4) and what is
    expected of each: 0 all missing, 1 count = 3, 2 count = 4, 3 a full pixel."""
    T = 8
    t = np.arange(T, dtype=np.float64)
    values = np.empty((T, 4), dtype)
    values[:] = (2.0 + 0.5 * t + np.sin(t))[:, None]
    values[:, 0] = np.nan
    values[3:, 1] = np.nan
    values[4:, 2] = np.nan
    return values, np.stack([np.ones(T), t], axis=1)


def test_edge_pixels_counts():
    values, design = edge_stack()
    got = R.regress(values, design, min_valid=4, stderr=True, series='residuals')
    assert list(got.count) == [0, 3, 4, 8]
    for p in (0, 1):
        assert np.isnan(got.coef[:, p]).all() and np.isnan(got.stderr[:, p]).all()
        assert np.isnan(got.rss[p]) and np.isnan(got.tss[p]) and np.isnan(got.r2[p]) and np.isnan(got.series[:, p]).all()
    for p in (2, 3):
        assert np.isfinite(got.coef[:, p]).all() and np.isfinite(got.stderr[:, p]).all() and 0 <= got.r2[p] <= 1


def test_count_equal_to_terms_gives_what_ieee_gives():
    """count == P with min_valid = P: an exact fit, sigma2 = rss / 0 -- inf or NaN, not an exception;
    the coefficients are there."""
    values, design = edge_stack()
    values[2:, 1] = np.nan
    got = R.regress(values, design, min_valid=2, stderr=True)
    assert got.count[1] == 2 and np.isfinite(got.coef[:, 1]).all()
    assert np.allclose(got.coef[:, 1], [values[0, 1], values[1, 1] - values[0, 1]])
    assert not np.isfinite(got.stderr[:, 1]).any()
    want = scalar_loop(values, design, [], None, 2, True, None)
    assert_same(got, want)


def test_constant_term_next_to_an_intercept_is_degenerate():
    rng = np.random.default_rng(3)
    T, n = 24, 3
    values = rng.standard_normal((T, n))
    term = rng.standard_normal((T, n))
    term[:, 1] = 3.7                                # exactly constant: collinear with the intercept
    got = R.regress(values, np.ones((T, 1)), [term], stderr=True, series='fitted')
    assert list(got.count) == [T] * n
    assert np.isnan(got.coef[:, 1]).all() and np.isnan(got.stderr[:, 1]).all() and np.isnan(got.r2[1])
    assert np.isnan(got.series[:, 1]).all()
    assert np.isfinite(got.coef[:, [0, 2]]).all() and np.isfinite(got.series[:, [0, 2]]).all()


def test_uncentred_year_column_is_not_degenerate():
    rng = np.random.default_rng(4)
    years = np.arange(2000.0, 2024.0)
    values = (0.02 * (years - 2000) + 1.0)[:, None] + 0.01 * rng.standard_normal((24, 2))
    got = R.regress(values, np.stack([np.ones(24), years], axis=1), stderr=True)
    assert np.isfinite(got.coef).all() and np.allclose(got.coef[1], 0.02, atol=5e-3)


def test_bad_weights_are_excluded():
    rng = np.random.default_rng(5)
    T = 12
    values = rng.standard_normal((T, 1))
    design = np.stack([np.ones(T), np.arange(T, dtype=np.float64)], axis=1)
    weights = np.ones((T, 1), np.float32)
    weights[[0, 3, 5, 7], 0] = [0.0, -2.0, np.nan, np.inf]
    got = R.regress(values, design, weights=weights, series='residuals')
    keep = np.ones(T, bool)
    keep[[0, 3, 5, 7]] = False
    want = R.regress(values[keep], design[keep])
    assert got.count[0] == 8
    assert same_bits(got.coef, want.coef) and same_bits(got.rss, want.rss)
    assert np.isnan(got.series[~keep, 0]).all() and np.isfinite(got.series[keep, 0]).all()


def test_one_step_one_term():
    got = R.regress(np.array([[3.0, np.nan]]), np.array([[2.0]]), min_valid=1, stderr=True, series='fitted')
    assert list(got.count) == [1, 0] and got.coef[0, 0] == 1.5 and np.isnan(got.coef[0, 1])
    assert got.rss[0] == 0.0 and np.isnan(got.stderr[0, 0])          # 0 / 0
    assert got.series[0, 0] == 3.0 and np.isnan(got.series[0, 1])
    assert_same(got, scalar_loop(np.array([[3.0, np.nan]]), np.array([[2.0]]), [], None, 1, True, 'fitted'))


def test_fitted_fills_missing_slabs_and_residuals_do_not():
    rng = np.random.default_rng(7)
    T, n = 46, 4
    design = R.harmonic_design(np.arange(T), 46.0, harmonics=1, trend=1)
    values = (design @ rng.standard_normal((4, n)) + 0.1 * rng.standard_normal((T, n))).astype(np.float32)
    gaps = rng.random((T, n)) < 0.4
    values[gaps] = np.nan
    fitted = R.regress(values, design, series='fitted')
    resid = R.regress(values, design, series='residuals')
    assert fitted.series.dtype == np.float32 and np.isfinite(fitted.series).all()
    assert np.array_equal(np.isnan(resid.series), gaps)
    ok = ~gaps
    assert np.allclose(fitted.series[ok] + resid.series[ok], values[ok], atol=1e-5)
    # with a per-pixel term the fitted value needs the term, not y
    term = rng.standard_normal((T, n)).astype(np.float32)
    term[5, :] = np.nan
    got = R.regress(values, design, [term], series='fitted')
    assert np.isnan(got.series[5]).all() and np.isfinite(np.delete(got.series, 5, axis=0)).all()


def test_harmonic_design():
    t = np.arange(1104) * 8.0
    d = R.harmonic_design(t, 368.0, harmonics=2, trend=1)
    assert d.shape == (1104, 6) and d.dtype == np.float64 and d.flags.c_contiguous
    assert (d[:, 0] == 1.0).all() and d[0, 1] == -1.0 and d[-1, 1] == 1.0
    assert np.allclose(d[:, 2], np.cos(2 * np.pi * t / 368.0)) and np.allclose(d[:, 5], np.sin(4 * np.pi * t / 368.0))
    assert R.harmonic_design(t, 368.0, harmonics=0, trend=3).shape == (1104, 4)
    rng = np.random.default_rng(0)
    for missing in (0.4, 0.8):
        assert np.linalg.cond(d[rng.random(1104) > missing]) < 3.0
    for bad in (dict(times=[0.0, np.nan], period=1.0), dict(times=t, period=0.0), dict(times=t, period=1.0, harmonics=-1)):
        with pytest.raises(ValueError):
            R.harmonic_design(**bad)


def test_refusals():
    shape = (10, 4, 5)
    ok = dict(shape=shape, dtype=np.float32, design_shape=(10, 2), term_shapes=[shape], term_dtypes=[np.float32])
    assert R.check_call(**ok) == (10, (4, 5), 2, 1, 4, False, 0)
    assert R.check_call(**dict(ok, min_valid=3, stderr=True, series='fitted'))[4:] == (3, True, 2)

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            R.check_call(**dict(ok, **change))
    refused('between 1 and 8 terms', design_shape=None, term_shapes=[], term_dtypes=[])                   # P = 0
    refused('between 1 and 8 terms', design_shape=(10, 8))                                                # P = 9
    refused('between 1 and 8 terms', design_shape=(10, 9), term_shapes=[], term_dtypes=[])
    refused('between 1 and 8 terms', design_shape=None, term_shapes=[shape] * 9, term_dtypes=[np.float32] * 9)
    refused('between 1 and 4096 steps', shape=(0, 4), design_shape=(0, 2), term_shapes=[(0, 4)])
    refused('between 1 and 4096 steps', shape=(4097, 4), design_shape=(4097, 2), term_shapes=[(4097, 4)])
    refused('leading time axis', shape=())
    refused(r'design must have shape \(10, Ks\)', design_shape=(9, 2))
    refused(r'design must have shape \(10, Ks\)', design_shape=(10,))
    refused(r'terms\[0\] must have the shape', term_shapes=[(10, 4, 4)])
    refused(r'terms\[0\] must have the dtype', term_dtypes=[np.float64])
    refused('float32 or float64', dtype=np.int16)
    refused('float32 or float64', dtype=np.uint8)
    refused('weights must have the shape', weights_shape=(10, 4))
    refused('min_valid must be at least', min_valid=2)
    refused('min_valid must be an integer', min_valid=3.5)
    refused('series must be', series='fit')
    refused('series must be', series=1)
    with pytest.raises(ValueError, match='design must be finite'):
        R.check_design(np.array([[1.0, np.inf]] * 10), 10)
    with pytest.raises(ValueError, match=r'design must have shape'):
        R.check_design(np.ones((9, 2)), 10)
    with pytest.raises(ValueError, match='design must be finite'):
        R.regress(np.zeros((3, 2)), np.array([[1.0], [np.nan], [1.0]]))
    with pytest.raises(ValueError, match='float32 or float64'):
        R.regress(np.zeros((3, 2), np.int32), np.ones((3, 1)))
    with pytest.raises(ValueError, match='weights must be float32'):
        R.regress(np.zeros((3, 2)), np.ones((3, 1)), weights=np.ones((3, 2)))
    assert R.check_design(None, 7).shape == (7, 0)


def test_output_table():
    table = R.output_table((4, 5), 10, 3, np.float32, stderr=True, series=1)
    assert list(table) == list(R.Regression._fields)
    assert table['coef'] == ((3, 4, 5), np.dtype(np.float64)) and table['stderr'] == table['coef']
    assert table['count'] == ((4, 5), np.dtype(np.uint16)) and table['series'] == ((10, 4, 5), np.dtype(np.float32))
    assert list(R.output_table((4,), 10, 3, np.float64)) == ['coef', 'rss', 'tss', 'r2', 'count']


def test_abi_has_the_new_names():
    from mod16_amd import _lib
    names = ('mod16_regress_f32', 'mod16_regress_f64', 'mod16_regress_max_steps', 'mod16_regress_max_terms')
    for name in names:
        assert name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 16
    text = open(os.path.join(ROOT, 'include', 'mod16_hip.h')).read()
    assert re.search(r'#define MOD16_ABI_VERSION 16\b', text)
    block = text[text.index('Per-pixel weighted least squares'):]
    assert 'added under ABI 16' in block[:400]
    for name in names + ('mod16_regress_spec',):
        assert name in block
    fields = re.search(r'typedef struct mod16_regress_spec \{(.*?)\} mod16_regress_spec;', text, flags=re.S).group(1)
    declared = re.findall(r'\b(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', fields, flags=re.S))
    assert declared == [f for f, _ in _lib.RegressSpec._fields_]
    assert (_lib.REGRESS_SERIES_NONE, _lib.REGRESS_SERIES_RESIDUALS, _lib.REGRESS_SERIES_FITTED) == (0, 1, 2)
    assert R.SERIES == {None: 0, 'residuals': 1, 'fitted': 2}
    import mod16
    import mod16_amd
    assert mod16.regress_series is mod16_amd.regress_series
