r'''
Sobol sensitivity analysis on the GPU: the reference's ``mod16/sensitivity.py`` without SALib.

The reference samples with ``SALib.sample.sobol.sample``, evaluates ``MOD16._et`` row by row and
calls ``SALib.analyze.sobol.analyze``. Here the same steps run on the device
(``mod16_sobol_*_f64``, C ABI ``include/mod16_hip.h``; the arithmetic is stated in full at the top
of ``mod16_amd/csrc/mod16_sobol.hpp``):

- ``saltelli_sample(bounds, n)``: the (n R, D) Saltelli matrix from the unscrambled Sobol sequence
  of ``scipy.stats.qmc.Sobol(2D, scramble=False, bits=32)``, in SALib's documented row layout
  (R = 2D + 2 rows per base sample, D + 2 without second order);
- ``sobol_analyze(Y, num_vars)``: S1, ST, S2 and their bootstrap confidence half-widths, keyed as
  SALib's result;
- ``sobol_drivers(params, bounds)``: the ``analysis="drivers"`` mode -- sample, ``MOD16._et`` and
  analysis with nothing of the sample's size on the host;
- ``sobol_parameters(drivers, observed, bounds)``: the ``analysis="parameters"`` mode -- the model's
  skill against a tower record (NSE, normalised NSE or RMSD) over a Saltelli sample of parameters.

Callers pass their bounds, as SALib's ``problem``; no bound table ships with the package. The
layout and the normalisation are meant to be SALib's, which is not on hand to check against.
Not provided: scrambled sequences, float32, the FAST arithmetic in the drivers' kernel, an HDF5
loader / command line like the reference's ``main``, several GPUs. There is no CPU fallback: without
an MI355X every entry point raises ``Mod16Error``.
'''
import statistics

import numpy as np

from . import _lib
from . import DRIVER_NAMES, MOD16, _is_device_tensor

MAX_VARS = 14
MAX_N = 1 << 26
METRICS = ('nse', 'nnse', 'rmsd')


def _rows_per_sample(d, second_order):
    return 2 * d + 2 if second_order else d + 2


def _check_n(n):
    n = int(n)
    if n < 1 or n > MAX_N or n & (n - 1):
        raise ValueError('n must be a power of two, at most 2^26 (got %d)' % n)
    return n


def _check_d(d):
    d = int(d)
    if d < 1 or d > MAX_VARS:
        raise ValueError('between 1 and %d variables can be analysed (got %d)' % (MAX_VARS, d))
    return d


def _bounds(bounds, names=None, n=None, skip=0):
    '''(names, lo, hi) of an ordered {name: (lo, hi)}, checked; names outside `names` are refused.'''
    if not hasattr(bounds, 'items'):
        raise ValueError('bounds must be an ordered mapping {name: (lo, hi)}')
    keys = list(bounds)
    _check_d(len(keys))
    if names is not None:
        unknown = [k for k in keys if k not in names]
        if unknown:
            raise ValueError('unknown name(s) %s; expected some of %s' % (unknown, list(names)))
    lo = np.empty(len(keys))
    hi = np.empty(len(keys))
    for i, k in enumerate(keys):
        pair = np.asarray(bounds[k], np.float64).ravel()
        if pair.size != 2:
            raise ValueError('bounds[%r] must be (lo, hi)' % k)
        lo[i], hi[i] = pair
        if not (np.isfinite(lo[i]) and np.isfinite(hi[i]) and lo[i] < hi[i]):
            raise ValueError('bounds[%r] = %r: lo < hi, both finite' % (k, tuple(pair)))
    if n is not None and (int(skip) < 0 or int(skip) + n > 1 << 32):
        raise ValueError('skip must be >= 0 with skip + n <= 2^32')
    return keys, lo, hi


def saltelli_sample(bounds, n, second_order=True, skip=0, device=0):
    '''
    The Saltelli sample of ``bounds`` (an ordered ``{name: (lo, hi)}``, D = len(bounds) <= 14) with
    ``n`` base samples (a power of two), drawn on the device: an (n R, D) float64 array whose rows
    for base sample j are A_j, AB_j^(1..D), [BA_j^(1..D) with ``second_order``], B_j. ``skip``
    starts the sequence later (SALib's ``skip_values``).
    '''
    n = _check_n(n)
    keys, lo, hi = _bounds(bounds, n=n, skip=skip)
    d = len(keys)
    out = np.empty((n * _rows_per_sample(d, second_order), d))
    ctx = _lib.context(device)
    ctx.check(ctx.lib.mod16_sobol_sample_f64(ctx.handle, d, lo.ctypes.data, hi.ctypes.data, n, int(skip),
                                             int(bool(second_order)), out.ctypes.data, _lib.HOST, None))
    return out


def _result(idx, std, d, second_order, conf_level):
    z = statistics.NormalDist().inv_cdf(0.5 + conf_level / 2.0)
    res = {'S1': idx[:d].copy(), 'S1_conf': z * std[:d], 'ST': idx[d:2 * d].copy(),
           'ST_conf': z * std[d:2 * d]}
    if second_order:
        res['S2'] = idx[2 * d:].reshape(d, d).copy()
        res['S2_conf'] = z * std[2 * d:].reshape(d, d)
    return res


def _analyze_args(size, num_vars, second_order, resamples, conf_level):
    d = _check_d(num_vars)
    R = _rows_per_sample(d, second_order)
    if size % R:
        raise ValueError('Y has %d values, not a multiple of the %d rows per base sample' % (size, R))
    n = _check_n(size // R)
    if not 0 < conf_level < 1:
        raise ValueError('conf_level must lie in (0, 1)')
    if int(resamples) < 0 or int(resamples) > 1 << 20:
        raise ValueError('resamples must be 0 .. 2^20')
    return d, n


def sobol_analyze(Y, num_vars, second_order=True, normalize=True, resamples=100, conf_level=0.95,
                  seed=0, device=0):
    '''
    Sobol indices of the model outputs ``Y`` (n R values in the row order of ``saltelli_sample``:
    a numpy array, or a float64 tensor on the GPU, which stays there): a dict keyed as SALib's
    ``sobol.analyze`` -- ``S1``, ``S1_conf``, ``ST``, ``ST_conf`` and, with ``second_order``, ``S2``
    and ``S2_conf`` (D x D, NaN on and below the diagonal) -- as numpy arrays. The confidence values
    are the standard deviation of each index over ``resamples`` bootstrap resamples of the base
    samples (keyed on ``seed``) times the normal quantile of ``conf_level``.
    '''
    d, n = _analyze_args(int(np.prod(np.shape(Y))), num_vars, second_order, resamples, conf_level)
    ctx = _lib.context(device)
    nidx = 2 * d + d * d
    args = (d, n, int(bool(second_order)), int(bool(normalize)), int(resamples), int(seed) & (2 ** 64 - 1))
    if _is_device_tensor(Y):
        import torch
        if Y.dtype != torch.float64 or not Y.is_contiguous():
            raise ValueError('a device Y must be a contiguous float64 tensor')
        idx = torch.empty(nidx, dtype=torch.float64, device=Y.device)
        std = torch.empty(nidx, dtype=torch.float64, device=Y.device)
        stream = torch.cuda.current_stream(Y.device).cuda_stream
        ctx.check(ctx.lib.mod16_sobol_analyze_f64(ctx.handle, Y.data_ptr(), *args, idx.data_ptr(),
                                                  std.data_ptr(), _lib.DEVICE, stream))
        idx, std = idx.cpu().numpy(), std.cpu().numpy()
    else:
        y = np.ascontiguousarray(Y, np.float64)
        idx, std = np.empty(nidx), np.empty(nidx)
        ctx.check(ctx.lib.mod16_sobol_analyze_f64(ctx.handle, y.ctypes.data, *args, idx.ctypes.data,
                                                  std.ctypes.data, _lib.HOST, None))
    return _result(idx, std, d, second_order, conf_level)


def _param_vector(params, what='params'):
    if hasattr(params, 'items'):
        missing = [k for k in MOD16.required_parameters if k not in params]
        if missing:
            raise ValueError('%s lacks %s' % (what, missing))
        return np.array([float(np.asarray(params[k])) for k in MOD16.required_parameters])
    vec = np.asarray(params, np.float64).ravel()
    if vec.size != 11:
        raise ValueError('%s must be a dict or 11 values in MOD16.required_parameters order' % what)
    return vec


def sobol_drivers(params, bounds, n=2048, fixed=None, second_order=True, skip=0, normalize=True,
                  resamples=100, conf_level=0.95, seed=0, device=0, return_outputs=False):
    '''
    The reference's ``analysis="drivers"``: Sobol indices of ``MOD16._et(params, *drivers)`` over
    the drivers named in ``bounds`` (an ordered ``{driver: (lo, hi)}``, any subset of
    ``mod16_amd.DRIVER_NAMES``); the others take their value from ``fixed`` (``{driver: value}``).
    ``params`` is a dict or 11 values in ``MOD16.required_parameters`` order. Each row is evaluated
    as its own scalar call in the reference's operation order; sample, evaluation and analysis run
    on the device, and the n R outputs stay there unless ``return_outputs``, which returns
    ``(result, Y)`` with Y in the row order of ``saltelli_sample(bounds, n, second_order, skip)``.
    '''
    n = _check_n(n)
    keys, lo, hi = _bounds(bounds, DRIVER_NAMES, n=n, skip=skip)
    d = len(keys)
    fixed = dict(fixed or {})
    unknown = [k for k in fixed if k not in DRIVER_NAMES]
    if unknown:
        raise ValueError('unknown driver name(s) in fixed: %s' % unknown)
    missing = [k for k in DRIVER_NAMES if k not in keys and k not in fixed]
    if missing:
        raise ValueError('drivers neither in bounds nor in fixed: %s' % missing)
    base = np.array([float(np.asarray(fixed[k])) if k in fixed and k not in keys else 0.0
                     for k in DRIVER_NAMES])
    vary = np.array([DRIVER_NAMES.index(k) for k in keys], np.int32)
    par = _param_vector(params)
    R = _rows_per_sample(d, second_order)
    _analyze_args(n * R, d, second_order, resamples, conf_level)
    ctx = _lib.context(device)                    # raises first without a device
    import torch
    dev = torch.device('cuda', device)
    y = torch.empty((n, R), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx.check(ctx.lib.mod16_sobol_rows_f64(ctx.handle, par.ctypes.data, base.ctypes.data, vary.ctypes.data,
                                           lo.ctypes.data, hi.ctypes.data, d, n, int(skip),
                                           int(bool(second_order)), y.data_ptr(), _lib.DEVICE, stream))
    res = sobol_analyze(y, d, second_order=second_order, normalize=normalize, resamples=resamples,
                        conf_level=conf_level, seed=seed, device=device)
    if return_outputs:
        return res, y.cpu().numpy().ravel()
    return res


def skill(sse, count, observed, metric):
    '''The score of each parameter vector from ``(sse, count)`` of ``BoundCalibration.objective``:
    ``nse`` = 1 - sse / sum((obs - nanmean(obs))^2) (the denominator over the finite observations;
    Nash & Sutcliffe 1970), ``nnse`` = 1 / (2 - nse) (the reference's ``norm=True``), ``rmsd`` =
    sqrt(sse / count).'''
    if metric == 'rmsd':
        return np.sqrt(sse / count)
    obs = np.asarray(observed, np.float64)
    nse = 1.0 - sse / np.nansum((obs - np.nanmean(obs)) ** 2)
    return nse if metric == 'nse' else 1.0 / (2.0 - nse)


def sobol_parameters(drivers, observed, bounds, n=512, params=None, metric='nnse', max_draws=4096,
                     math=_lib.MATH_EXACT, second_order=True, skip=0, normalize=True, resamples=100,
                     conf_level=0.95, seed=0, device=0, return_outputs=False):
    '''
    The reference's ``analysis="parameters"``: Sobol indices of the model's skill against a tower
    record over the parameters named in ``bounds`` (an ordered ``{parameter: (lo, hi)}``, names of
    ``MOD16.required_parameters``); the others come from ``params`` (a dict, or 11 values). The
    14 ``drivers`` (a sequence in ``DRIVER_NAMES`` order, or a dict) and ``observed`` are bound on
    the device once (``MOD16._et_bind``), the sample is drawn there, and the rows are scored
    ``max_draws`` at a time by ``metric`` (``'nse'``, ``'nnse'`` or ``'rmsd'``, see ``skill``).
    ``math``: ``MATH_EXACT`` (default, the reference's operation order) or ``MATH_FAST``. With
    ``return_outputs``: ``(result, Y)``, Y the score of each row of ``saltelli_sample(bounds, n,
    second_order, skip)``.
    '''
    if metric not in METRICS:
        raise ValueError('metric must be one of %s' % (METRICS,))
    n = _check_n(n)
    names = list(MOD16.required_parameters)
    keys, _, _ = _bounds(bounds, names, n=n, skip=skip)
    d = len(keys)
    if hasattr(drivers, 'items'):
        missing = [k for k in DRIVER_NAMES if k not in drivers]
        if missing:
            raise ValueError('drivers lacks %s' % missing)
        drivers = [drivers[k] for k in DRIVER_NAMES]
    if len(drivers) != 14:
        raise ValueError('drivers must be the 14 drivers in DRIVER_NAMES order')
    rest = [k for k in names if k not in keys]
    if rest:
        if params is None:
            raise ValueError('parameters neither in bounds nor in params: %s' % rest)
        if hasattr(params, 'items'):
            missing = [k for k in rest if k not in params]
            if missing:
                raise ValueError('parameters neither in bounds nor in params: %s' % missing)
            full = np.array([float(np.asarray(params[k])) if k in rest else 0.0 for k in names])
        else:
            full = _param_vector(params)
    else:
        full = np.zeros(11)
    R = _rows_per_sample(d, second_order)
    _analyze_args(n * R, d, second_order, resamples, conf_level)
    if int(max_draws) < 1:
        raise ValueError('max_draws must be >= 1')
    X = saltelli_sample(bounds, n, second_order=second_order, skip=skip, device=device)
    P = np.repeat(full[None, :], X.shape[0], axis=0)
    P[:, [names.index(k) for k in keys]] = X
    problem = MOD16._et_bind(*drivers, observed=observed, max_draws=max_draws, math=math, device=device)
    try:
        sse, count = np.empty(X.shape[0]), np.empty(X.shape[0])
        for a in range(0, X.shape[0], int(max_draws)):
            sse[a:a + max_draws], count[a:a + max_draws] = problem.objective(P[a:a + max_draws])
    finally:
        problem.close()
    obs = np.broadcast_to(np.asarray(observed, np.float64), problem.shape)
    Y = skill(sse, count, obs, metric)
    res = sobol_analyze(Y, d, second_order=second_order, normalize=normalize, resamples=resamples,
                        conf_level=conf_level, seed=seed, device=device)
    return (res, Y) if return_outputs else res
