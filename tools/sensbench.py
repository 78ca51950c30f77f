#!/usr/bin/env python3
"""Throughput of the Sobol sensitivity analysis (mod16_amd.sensitivity), in one GPU process:

  rows      the fused sample + MOD16._et kernel (mod16_sobol_rows_f64, all 14 drivers, R = 30)
            at N = 2^12 .. 2^22 base samples: evaluations/s from HIP events around DEVICE calls
  yardstick MOD16._et_batch(..., math=MATH_EXACT) on the same device, the same pixel function:
            pixel-draws/s of a whole (host-synchronous) call with `observed`, so only (sse, count)
            come back
  analyze   mod16_sobol_analyze_f64 at R = 30 with 100 resamples: ms from HIP events, and the bytes
            the Gram kernel gathers ((resamples + 1) x n x R x 8) over that time
  drivers   wall time of a whole sobol_drivers (sample, rows, analysis, indices to the host) at the
            reference's N = 2048 and at N = 2^20

  python tools/sensbench.py [--out FILE]      prints one JSON line (and writes it to FILE)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mod16_amd  # noqa: E402
from mod16_amd import _lib, sensitivity as sens  # noqa: E402

BOUNDS = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'sensitivity_bounds.json')))['drivers']
P = dict(tmin_close=-8.0, tmin_open=8.0, vpd_open=650.0, vpd_close=3000.0, gl_sh=0.01, gl_wv=0.01,
         g_cuticular=1e-5, csl=2.4e-3, rbl_min=60.0, rbl_max=90.0, beta=250.0)
PVEC = np.array([P[k] for k in mod16_amd.MOD16.required_parameters])


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ctx = _lib.context(0)
    d, R = 14, 30
    lo = np.array([v[0] for v in BOUNDS.values()], np.float64)
    hi = np.array([v[1] for v in BOUNDS.values()], np.float64)
    vary = np.arange(14, dtype=np.int32)
    base = np.zeros(14)
    stream = torch.cuda.current_stream().cuda_stream
    out = {'tool': 'sensbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(0)}
    rows = {}
    for lg in range(12, 23, 2):
        n = 1 << lg
        y = torch.empty((n, R), dtype=torch.float64, device='cuda')

        def run():
            ctx.check(ctx.lib.mod16_sobol_rows_f64(ctx.handle, PVEC.ctypes.data, base.ctypes.data,
                                                   vary.ctypes.data, lo.ctypes.data, hi.ctypes.data, d, n, 0,
                                                   1, y.data_ptr(), _lib.DEVICE, stream))
        ms = events_ms(run, 20 if lg < 20 else 5)
        rows['2^%d' % lg] = {'ms': round(ms, 4), 'evals_per_s': n * R / ms * 1e3}
    out['rows'] = rows
    # yardstick: the batched calibration path, EXACT, same pixel function
    rng = np.random.default_rng(0)
    npx, ndraw = 16384, 2048
    drv = [rng.uniform(a, b, npx) for a, b in zip(lo, hi)]
    par = np.repeat(PVEC[None], ndraw, axis=0) * rng.uniform(0.9, 1.1, (ndraw, 11))
    obs = mod16_amd.MOD16._et(PVEC, *drv)
    mod16_amd.MOD16._et_batch(par[:8], *drv, observed=obs, math=_lib.MATH_EXACT)
    best = np.inf
    for _ in range(3):
        t = time.perf_counter()
        mod16_amd.MOD16._et_batch(par, *drv, observed=obs, math=_lib.MATH_EXACT)
        best = min(best, time.perf_counter() - t)
    out['et_batch_exact'] = {'pixels': npx, 'draws': ndraw, 's': best, 'evals_per_s': npx * ndraw / best}
    top = rows['2^22']['evals_per_s']
    out['rows_over_et_batch'] = top / out['et_batch_exact']['evals_per_s']
    # analysis + bootstrap
    an = {}
    for lg in (12, 16, 20):
        n = 1 << lg
        y = torch.randn((n, R), dtype=torch.float64, device='cuda')
        idx = torch.empty(2 * d + d * d, dtype=torch.float64, device='cuda')
        std = torch.empty_like(idx)

        def run():
            ctx.check(ctx.lib.mod16_sobol_analyze_f64(ctx.handle, y.data_ptr(), d, n, 1, 1, 100, 0,
                                                      idx.data_ptr(), std.data_ptr(), _lib.DEVICE, stream))
        ms = events_ms(run, 5)
        gathered = 101 * n * R * 8
        an['2^%d' % lg] = {'ms': round(ms, 4), 'gathered_bytes': gathered, 'GB_per_s': gathered / ms / 1e6,
                           'of_8TB_per_s': gathered / ms / 1e6 / 8000}
    out['analyze_100_resamples'] = an
    # whole drivers mode
    wall = {}
    for lg in (11, 20):
        sens.sobol_drivers(P, BOUNDS, n=1 << lg)
        t = time.perf_counter()
        res = sens.sobol_drivers(P, BOUNDS, n=1 << lg)
        wall['2^%d' % lg] = {'s': time.perf_counter() - t, 'finite': bool(np.all(np.isfinite(res['ST'])))}
    out['sobol_drivers_wall'] = wall
    line = json.dumps(out)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
