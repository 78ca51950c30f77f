#!/usr/bin/env python3
"""The composite over coarse drivers (DownscaleGrid.composite, mod16_et_composite_downscaled_*) against
what it replaces, in one GPU process, float64, resident: 4 x 1200 x 1200 fine pixels (a 2400 x 2400
window of 20 x 20 degrees) over a global 361 x 576 reanalysis grid, bilinear; ten reanalysis drivers and
the hours of daylight as daily coarse series, temp_annual one coarse plane, albedo / fPAR / LAI fine
8-day slabs. Two sizes: K = 8 days in one period, and K = 368 days in 46 periods of 8.

  (a) downscaled    one call on the coarse series
  (b) materialised  what a user wrote before, period by period (a year of materialised drivers is
                    88 B per pixel-day: 187 GB at this size): DownscaleGrid.fields of the period's coarse
                    planes into (8, n) tensors, then RasterEngine.composite on them
  (c) composite     RasterEngine.composite alone, period by period, on the tensors (b) left behind: the floor

Device events on the current stream; one warm-up of each, then --repeats alternating repeats of windows
of at least --window seconds each; the medians. The outputs of (a) and (b) must have the same bits, counts
included -- checked before anything is timed. One JSON line: per size the three times, ps and counted
bytes per pixel-day, the ratios, the device memory of the drivers either way. Exits non-zero only where
the bits differ: whether (a) beats (b) is what is measured.

  python tools/compositedownscalebench.py [--out FILE] [--repeats 3] [--window 0.25] [--days 8 368]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mod16_amd import _lib  # noqa: E402
from mod16_amd import composite as cp  # noqa: E402
from mod16_amd import downscale as ds  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

R = C = 2400
H, W = 361, 576
L = 8
SLOW = ('sw_albedo', 'fpar', 'lai')
COARSE = tuple(n for n in cp.ARRAY_NAMES if n not in SLOW)             # eleven drivers and the hours
SERIES = tuple(n for n in COARSE if n != 'temp_annual')                 # ... of which these are daily
EVERY = dict.fromkeys(SLOW, L)
#: counted per pixel-day, float64. (a): the three fine slabs once per 8 days, per period one total and one
#: count out, the class byte once per call (not counted); the coarse planes stay in cache (11 x 361 x 576 x 8 B
#: = 18 MB a day, 3 B per pixel-day at this size, not counted). (c): (a) plus one 8-byte read per materialised
#: value and day. (b): (c) plus the 8-byte store of each (the interpolation's own reads not counted).
BYTES_DOWNSCALED = (3 * 8 + 8 + 2) / L
BYTES_COMPOSITE = BYTES_DOWNSCALED + len(SERIES) * 8
BYTES_MATERIALISED = BYTES_COMPOSITE + len(SERIES) * 8


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def same_bits(a, b):
    if a.dtype == torch.uint16:
        return bool((a.view(torch.int16) == b.view(torch.int16)).all())
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all())


def case(eng, grid, K, repeats, window):
    dev, n, P = eng._dev(), R * C, -(-K // L)
    cls, fine = eng.synth(n, seed=16)
    arrays = {}
    for name in SLOW:
        arrays[name] = torch.empty((P, n), dtype=eng.dtype, device=dev)
    for p in range(P):
        _, slab = eng.synth(n, seed=16, step=p)
        for name in SLOW:
            arrays[name][p].copy_(slab[cp.ARRAY_NAMES.index(name)])
    for name in SERIES:
        arrays[name] = torch.empty((K, H, W), dtype=eng.dtype, device=dev)
    for t in range(K):
        _, planes = eng.synth(H * W, seed=17, step=t)
        for name in SERIES:
            k = cp.ARRAY_NAMES.index(name)
            if name == 'day_hours':
                arrays[name][t].copy_((planes[5].view(H, W) - 250.0).clamp(6.0, 18.0))      # hours from a temperature field
            else:
                arrays[name][t].copy_(planes[k].view(H, W))
    arrays['temp_annual'] = eng.synth(H * W, seed=18)[1][7].view(H, W).clone()
    del slab, planes
    full = [arrays[name] for name in cp.ARRAY_NAMES]
    out_a = [torch.empty((P, n), dtype=eng.dtype, device=dev), torch.empty((P, n), dtype=torch.uint16, device=dev)]
    out_b = [torch.empty_like(o) for o in out_a]
    out_c = [torch.empty_like(o) for o in out_a]
    # one period's materialised drivers: (8, n) per series, (n,) for the constant
    dense = {name: torch.empty((L, n), dtype=eng.dtype, device=dev) for name in SERIES}
    dense['temp_annual'] = torch.empty((1, n), dtype=eng.dtype, device=dev)

    def call_a():
        grid.composite(cls, full[:14], full[14], K, L, every=EVERY, coarse=COARSE, out=out_a)

    def materialise(p):
        days = min(L, K - p * L)
        for name in SERIES:
            grid.fields([arrays[name][p * L + d] for d in range(days)], out=dense[name][:days])
        grid.fields([arrays['temp_annual']], out=dense['temp_annual'])
        return days

    def composite(p, days, out):
        per = []
        for name in cp.ARRAY_NAMES:
            if name in SLOW:
                per.append(arrays[name][p])
            elif name == 'temp_annual':
                per.append(dense[name][0])
            else:
                per.append(dense[name][:days])
        eng.composite(cls, per[:14], per[14], days, L, out=[o[p:p + 1] for o in out])

    def call_b():
        for p in range(P):
            composite(p, materialise(p), out_b)

    def call_c():
        for p in range(P):
            composite(p, min(L, K - p * L), out_c)
    call_a()
    call_b()
    call_c()
    eng.check()
    if not all(same_bits(x, y) for x, y in zip(out_a, out_b)):
        raise SystemExit('compositedownscalebench: K = %d: the downscaled composite and the materialised one differ in their bits' % K)
    calls = {'downscaled': call_a, 'materialised': call_b, 'composite': call_c}
    inner = {}
    for name, fn in calls.items():
        ms = timed(fn, 1)                      # (the warm-up above loaded the code objects)
        inner[name] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            times[name].append(timed(fn, inner[name]))
    eng.check()
    med = {name: float(np.median(t)) for name, t in times.items()}
    esz = 8
    return {'days': K, 'periods': P,
            'ms': {name: round(ms, 4) for name, ms in med.items()},
            'ps_per_pixel_day': {name: round(ms * 1e9 / (n * K), 2) for name, ms in med.items()},
            'bytes_per_pixel_day_counted': {'downscaled': round(BYTES_DOWNSCALED, 2), 'materialised': round(BYTES_MATERIALISED, 2),
                                            'composite': round(BYTES_COMPOSITE, 2)},
            'downscaled_over_materialised': round(med['downscaled'] / med['materialised'], 4),
            'downscaled_over_composite': round(med['downscaled'] / med['composite'], 4),
            'finite_fraction': round(float(torch.isfinite(out_a[0]).double().mean()), 4),
            'driver_bytes_on_device': {'downscaled': 3 * P * n * esz + (len(SERIES) * K + 1) * H * W * esz,
                                       'materialised_whole': (3 * P + (len(SERIES) * K + 1)) * n * esz},
            'ms_all': {name: [round(t, 4) for t in ts] for name, ts in times.items()},
            'launches_per_window': inner, 'same_bits': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    ap.add_argument('--days', type=int, nargs='+', default=[8, 368])
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    # the window: rows from 60 N southwards, columns from 0 E eastwards, pixel centres
    row_pos = ds.positions(60.0 - 10.0 / R, -20.0 / R, R, 90.0, -0.5)
    col_pos = ds.positions(10.0 / C, 20.0 / C, C, -180.0, 0.625)
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=True, method='bilinear')
    res = {'tool': 'compositedownscalebench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'dtype': 'float64', 'pixels': R * C, 'coarse_grid': [H, W], 'method': 'bilinear', 'coarse_arrays': len(COARSE),
           'period_days': L, 'cases': []}
    for K in a.days:
        res['cases'].append(case(eng, grid, K, a.repeats, a.window))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
