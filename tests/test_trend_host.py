"""Host tests of the per-pixel trend: the numpy definition (mod16_amd/trend.py) against answers worked
out by hand, its own properties and scipy.stats.theilslopes; every refusal of the argument checks
trend_series and RasterEngine.trend share; the C ABI's three new symbols. Nothing here needs a device
(tests/test_gpu_trend.py holds the kernel to this definition bit for bit)."""
import ctypes
import os
import re
import statistics

import numpy as np
import pytest

from conftest import ROOT
from mod16_amd import trend as tr

HEADER = os.path.join(ROOT, 'include', 'mod16_hip.h')
Z95 = statistics.NormalDist().inv_cdf(0.975)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def one(x, t=None, min_valid=2, alpha=None):
    """The definition of one pixel -> Trend of Python scalars."""
    r = tr.trend(np.asarray(x, np.float64).reshape(-1, 1), t, min_valid, alpha)
    return tr.Trend(*[None if a is None else a[0] for a in r])


def test_known_answers_worked_out_by_hand():
    # Y = 4, no ties: slopes -1, 1/2, 1, 4/3, 2, 3 (M = 6, even); five pairs rise, one falls
    r = one([1.0, 3.0, 2.0, 5.0])
    slope = (1.0 + 4.0 / 3.0) * 0.5
    assert (r.count, r.s) == (4, 4) and r.slope == slope and r.intercept == 2.5 - slope * 1.5
    assert r.z == 3.0 / np.sqrt(156.0 / 18.0) and r.slope_lo is None and r.slope_hi is None
    # Y = 5 with a tie: slopes -1, 0, 1/3, 1/2, 1/2, 1/2, 1, 1, 1, 2 (M = 10); V18 = 300 - 18
    r = one([1.0, 2.0, 2.0, 4.0, 3.0], alpha=0.05)
    assert (r.count, r.s) == (5, 7) and r.slope == 0.5 and r.intercept == 1.0
    assert r.z == 6.0 / np.sqrt(282.0 / 18.0)
    # C = 1.96 sqrt(282 / 18) = 7.76: ranks min(rint(8.88), 9) = 9 and rint(1.12) - 1 = 0
    assert (r.slope_lo, r.slope_hi) == (-1.0, 2.0)
    # all tied: nothing rises, V18 = 0
    r = one([7.0] * 5, alpha=0.05)
    assert (r.count, r.s, r.z, r.slope, r.intercept) == (5, 0, 0.0, 0.0, 7.0)
    assert bits(r.slope) == bits(0.0) and (r.slope_lo, r.slope_hi) == (0.0, 0.0)
    # odd M = 3 on irregular times: slopes 2, 1, 1/2
    r = one([1.0, 3.0, 4.0], [0.0, 1.0, 3.0])
    assert (r.count, r.s, r.slope, r.intercept) == (3, 3, 1.0, 2.0) and r.z == 2.0 / np.sqrt(66.0 / 18.0)


def test_sign_change_shift_and_the_parity_of_m():
    rng = np.random.default_rng(5)
    for Y in (4, 5, 6, 7, 24):                      # M = 6, 10, 15, 21, 276: even and odd
        x = np.round(rng.normal(500.0, 60.0, (Y, 40)))
        x[rng.uniform(0, 1, x.shape) < 0.1] = np.nan
        t = np.cumsum(rng.uniform(0.5, 1.5, Y))
        a, b, c = tr.trend(x, t, 3, 0.05), tr.trend(-x, t, 3, 0.05), tr.trend(x + 1024.0, t, 3, 0.05)
        ok = ~np.isnan(a.slope)
        assert ok.any() and np.array_equal(ok, a.count >= 3)
        assert np.array_equal(b.s, -a.s) and np.array_equal(bits(b.slope[ok]), bits(-a.slope[ok] + 0.0))
        assert np.array_equal(bits(b.z[ok]), bits(-a.z[ok] + 0.0))
        assert np.array_equal(bits(b.slope_lo[ok]), bits(-a.slope_hi[ok] + 0.0))
        assert np.array_equal(c.s, a.s) and np.array_equal(bits(c.slope), bits(a.slope)) and np.array_equal(bits(c.z), bits(a.z))
        assert np.array_equal(a.count, np.isfinite(x).sum(0))


def test_min_valid_cut_and_missing_values():
    x = np.array([1.0, np.nan, 3.0, np.inf, 2.0, -np.inf, 7.0])
    r = one(x, min_valid=4)
    assert r.count == 4 and r.s == 4            # 1, 3, 2, 7: the infinities are missing
    same = one([1.0, 3.0, 2.0, 7.0], [0.0, 2.0, 4.0, 6.0], min_valid=4)
    assert bits(r.slope) == bits(same.slope) and bits(r.intercept) == bits(same.intercept) and bits(r.z) == bits(same.z)
    r = one(x, min_valid=5, alpha=0.05)
    assert r.count == 4 and r.s == 0 and all(np.isnan(v) for v in (r.slope, r.intercept, r.slope_lo, r.slope_hi, r.z))
    r = one([np.nan] * 6)
    assert r.count == 0 and r.s == 0 and np.isnan(r.slope)
    # equal values are indistinguishable: -0.0 among 0.0 changes nothing, and no -0.0 comes out
    r, q = one([0.0, -0.0, 0.0, -0.0]), one([-0.0, 0.0, -0.0, 0.0])
    assert r.s == q.s == 0 and bits(r.slope) == bits(q.slope) == bits(0.0) and bits(r.intercept) == bits(q.intercept) == bits(0.0)
    # a difference that overflows is what IEEE gives: slopes inf, 7.5e307, -1.5e308; then inf, inf, 1e307
    r = one([-1.5e308, 1.5e308, 0.0], min_valid=3)
    assert r.s == 1 and r.slope == 7.5e307 and np.isinf(one([-1.5e308, 1.5e308, 1.6e308], min_valid=3).slope)
    assert r.slope.dtype == np.float64 and tr.trend(np.zeros((4, 2, 3), np.float32)).s.shape == (2, 3)
    full = tr.trend(np.zeros((4, 2, 3), np.float32))
    assert full.s.dtype == np.int32 and full.count.dtype == np.uint8 and full.count.max() == 4


def generator(ties):
    """The cases of the issue's prototype: default_rng(3), Y in (5, 8, 24, 33, 64), t = arange(Y),
    x = round(normal(500, 60, Y) + 2 t, 0 or 3 decimals alternately)."""
    rng = np.random.default_rng(3)
    k = 0
    for Y in (5, 8, 24, 33, 64):
        for _ in range(70):
            t = np.arange(Y, dtype=np.float64)
            x = np.round(rng.normal(500.0, 60.0, Y) + 2.0 * t, 0 if k % 2 == 0 else 3)
            k += 1
            if (k % 2 == 1) == ties:
                yield Y, t, x, rng


def test_slope_and_intercept_have_the_bits_of_scipy_theilslopes():
    stats = pytest.importorskip('scipy.stats')
    cases = 0
    for ties in (True, False):
        for Y, t, x, rng in generator(ties):
            x = x.copy()
            x[rng.uniform(0, 1, Y) < 0.15] = np.nan
            v = np.isfinite(x)
            if v.sum() < 2:
                continue
            got = one(x, t)
            want = stats.theilslopes(x[v], t[v], 0.95)
            assert bits(got.slope) == bits(want[0] + 0.0) and bits(got.intercept) == bits(want[1]), (Y, x)
            cases += 1
    assert cases > 300


def test_interval_picks_the_ranks_scipy_picks():
    stats = pytest.importorskip('scipy.stats')
    cases = 0
    for ties in (False, True):
        for Y, t, x, _ in generator(ties):
            got = one(x, t, alpha=0.05)
            want = stats.theilslopes(x, t, 0.95)
            assert bits(got.slope_lo) == bits(want[2] + 0.0) and bits(got.slope_hi) == bits(want[3] + 0.0), (Y, x)
            cases += 1
    assert cases == 350


def test_every_refusal_of_the_shared_checks_has_its_message():
    def bad(match, shape=(6, 10), **kw):
        with pytest.raises(ValueError, match=match):
            tr.check_call(shape, **kw)
    bad('2 <= Y <= 64', shape=())
    bad('2 <= Y <= 64', shape=(1, 10))
    bad('2 <= Y <= 64', shape=(65, 10))
    bad(r'times must have shape \(6,\)', times=np.arange(5.0))
    bad('times must be finite', times=[0, 1, 2, np.nan, 4, 5])
    bad('times must be finite', times=[0, 1, 2, 3, 4, np.inf])
    bad('strictly increasing', times=[0, 1, 2, 2, 4, 5])
    bad('strictly increasing', times=[5, 4, 3, 2, 1, 0])
    bad('span of times', times=[-1.5e308, 1, 2, 3, 4, 1.5e308])
    for mv in (1, 7, 2.5, True):
        bad('min_valid must be an integer between 2 and Y = 6', min_valid=mv)
    for alpha in (0.0, -0.1, 0.51, 1.0, float('nan')):
        bad(r'alpha must be None or a level in \(0, 0.5\]', alpha=alpha)
    Y, shape, t, mv, zq = tr.check_call((6, 2, 5), None, 6, 0.05)
    assert (Y, shape, mv) == (6, (2, 5), 6) and np.array_equal(t, np.arange(6.0)) and t.dtype == np.float64
    assert zq == Z95 and tr.check_call((2,), min_valid=2)[4] == 0.0 and tr.check_call((2,), min_valid=2)[1] == ()
    assert tr.check_call((64, 0), alpha=0.5)[4] == statistics.NormalDist().inv_cdf(0.75)
    for dtype in (np.int32, np.float16, np.uint8):
        with pytest.raises(ValueError, match='values must be float32 or float64'):
            tr.check_dtype(dtype)


def test_numpy_entry_point_checks_then_needs_a_device():
    import mod16
    import mod16_amd
    from mod16_amd import _lib
    assert mod16.trend_series is mod16_amd.trend_series
    call = mod16_amd.trend_series
    x = np.round(np.random.default_rng(2).normal(500.0, 60.0, (6, 3, 7))).astype(np.float32)
    with pytest.raises(ValueError, match='float32 or float64'):
        call(x.astype(np.int32))
    with pytest.raises(ValueError, match='2 <= Y <= 64'):
        call(x[:1])
    with pytest.raises(ValueError, match='strictly increasing'):
        call(x, times=[0, 1, 1, 2, 3, 4])
    with pytest.raises(ValueError, match='min_valid'):
        call(x, min_valid=7)
    with pytest.raises(ValueError, match='alpha'):
        call(x, alpha=0.75)
    with pytest.raises(ValueError, match='stage_bytes'):
        call(x, stage_bytes=-1)
    empty = call(x[:, :, :0], alpha=0.05)           # no pixels: no device work
    assert empty.slope.shape == empty.slope_hi.shape == empty.count.shape == (3, 0) and empty.s.dtype == np.int32
    if _lib.device_count() > 0:
        got, want = call(x, alpha=0.05), tr.trend(x, alpha=0.05)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    else:
        with pytest.raises(_lib.Mod16Error, match='no CPU fallback'):
            call(x)


def test_tensor_entry_point_refusals_that_need_no_device():
    torch = pytest.importorskip('torch')
    from mod16_amd import _tensors
    from mod16_amd.raster import RasterEngine
    eng = object.__new__(RasterEngine)         # the checks in front of the first use of a device
    eng.device = 0
    for bad in (np.zeros((4, 5)), torch.zeros((4, 5)), torch.zeros((4, 5), dtype=torch.float64)):
        with pytest.raises(TypeError, match='values must be a float32 or float64 tensor on cuda:0'):
            eng.trend(bad)
    # the layout rule the stack is held to: unit stride in pixels, a stride in time of at least n
    assert _tensors.row_pitch(torch.zeros((4, 9))[:, :5], 'values', 'stride in time') == 9
    with pytest.raises(ValueError, match='values must have unit stride in pixels'):
        _tensors.row_pitch(torch.zeros((4, 10))[:, ::2], 'values', 'stride in time')
    with pytest.raises(ValueError, match='values: the stride in time must be at least 5'):
        _tensors.row_pitch(torch.zeros(8).as_strided((4, 5), (1, 1)), 'values', 'stride in time')


def header_struct(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, flags=re.S).group(1)
    types = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), types[ctype]) for n in names.split(',')]
    return fields


def test_abi_symbols_spec_layout_and_capacity():
    from mod16_amd import _lib
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 16 and re.search(r'#define MOD16_ABI_VERSION 16\b', text)
    for name in ('mod16_trend_f32', 'mod16_trend_f64', 'mod16_trend_max_steps'):
        assert re.search(r'MOD16_API int %s\(' % name, text) and name in _lib.PROTOTYPES
    for name in ('mod16_trend_f32', 'mod16_trend_f64'):
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == 10
        assert args[1] is ctypes.POINTER(_lib.TrendSpec) and args[9] is ctypes.c_size_t
    fields = header_struct('mod16_trend_spec')
    assert fields == list(_lib.TrendSpec._fields_)

    class Twin(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(_lib.TrendSpec) == ctypes.sizeof(Twin) == 32
    assert callable(_lib.Context.trend)
    lib = _lib.load()
    assert lib.mod16_trend_max_steps() == 64 == tr.MAX_STEPS
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mod16_trend_f32', 'mod16_trend_f64', 'mod16_trend_max_steps'):
        assert hasattr(exported, name)
    for name in ('mod16_trend_f32', 'mod16_trend_f64'):
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
        # a NULL context (and with it a NULL spec) is refused before anything is looked at
        assert getattr(lib, name)(None, None, None, None, None, None, None, 0, None, 0) == _lib.ERR_ARG
