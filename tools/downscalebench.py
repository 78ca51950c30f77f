#!/usr/bin/env python3
"""The downscaled forward run (RasterEngine.downscale_grid(...).run, mod16_et_downscaled_*) against
what it replaces, in one GPU process, float64, resident: 4 x 1200 x 1200 fine pixels (a 2400 x 2400
window of 20 x 20 degrees) over a global 361 x 576 reanalysis grid (0.5 x 0.625 degrees: 60 x 75 fine
pixels per cell), bilinear, the eleven reanalysis drivers coarse, albedo / fPAR / LAI fine:

  (a) downscaled    one call on the coarse planes
  (b) materialised  what a user wrote before, with calls that predate the family: per coarse driver four
                    torch gathers and the weighted sum into a fine tensor (indices and weights made once,
                    outside the clock), then run() on the 14 fine tensors
  (c) run           run() alone on the 14 fine tensors (b) left behind

Device events on the current stream; one warm-up of each, then --repeats alternating repeats of windows
of at least --window seconds each; the medians. The outputs of (a), (b) and (c) must have the same bits
-- checked before anything is timed. One JSON line: the three times, their ratios, the counted bytes per
pixel, the rates as fractions of the copy kernel's (measured in this process), the device memory of the
drivers either way. Exits non-zero only where the bits differ: whether (a) beats (c) is what is measured.

  python tools/downscalebench.py [--out FILE] [--repeats 5] [--window 0.25]
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
from mod16_amd import downscale as ds  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

R = C = 2400
H, W = 361, 576
COARSE = [k for k, name in enumerate(ds.DRIVER_NAMES) if name in ds.MET_DRIVERS]
#: counted, float64: the fine drivers, the class byte, two outputs (the coarse planes and the tables
#: stay in cache: 11 x 361 x 576 x 8 B = 18 MB read once is 3.2 B per pixel on top at this size)
BYTES_DOWNSCALED = 3 * 8 + 1 + 2 * 8
BYTES_RUN = 14 * 8 + 1 + 2 * 8
#: (b) at the least: (c) plus one 8-byte store per materialised value (its temporaries not counted)
BYTES_MATERIALISED = BYTES_RUN + 11 * 8


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def same_bits(a, b):
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    dev = eng._dev()
    copy_gbps = float(eng.measure_copy())
    n = R * C
    # the window: rows from 60 N southwards, columns from 0 E eastwards, pixel centres
    row_pos = ds.positions(60.0 - 10.0 / R, -20.0 / R, R, 90.0, -0.5)
    col_pos = ds.positions(10.0 / C, 20.0 / C, C, -180.0, 0.625)
    grid = eng.downscale_grid((R, C), (H, W), row_pos, col_pos, wrap=True, method='bilinear')
    cls, fine = eng.synth(n, seed=16)
    _, planes = eng.synth(H * W, seed=16, step=1)
    drivers = [planes[k].view(H, W) if k in COARSE else fine[k] for k in range(14)]
    out_a = eng.empty(n, 2)
    out_b = eng.empty(n, 2)
    out_c = eng.empty(n, 2)
    # (b)'s geometry, once: the four index pairs and the four weights of every pixel
    ri0, ri1, rw0, rw1 = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in grid.row_tables)
    ci0, ci1, cw0, cw1 = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in grid.col_tables)
    rows = [ri0.long()[:, None], ri1.long()[:, None]]
    cols = [ci0.long()[None, :], ci1.long()[None, :]]
    w = [rw0[:, None] * cw0[None, :], rw0[:, None] * cw1[None, :], rw1[:, None] * cw0[None, :], rw1[:, None] * cw1[None, :]]
    dense = [torch.empty((R, C), dtype=eng.dtype, device=dev) if k in COARSE else fine[k] for k in range(14)]

    def call_a():
        grid.run(cls, drivers, out_day=out_a[0], out_night=out_a[1])

    def materialise():
        for k in COARSE:
            g = drivers[k]
            t = w[0] * g[rows[0], cols[0]]
            t += w[1] * g[rows[0], cols[1]]
            t += w[2] * g[rows[1], cols[0]]
            torch.add(t, w[3] * g[rows[1], cols[1]], out=dense[k])

    def call_c(out=out_c):
        eng.run(cls, [d.view(-1) for d in dense], out[0], out[1])

    def call_b():
        materialise()
        call_c(out_b)
    call_a()
    call_b()
    call_c()
    eng.check()
    for x, y, what in ((out_a, out_b, 'materialised run'), (out_a, out_c, 'run on materialised drivers')):
        if not (same_bits(x[0], y[0]) and same_bits(x[1], y[1])):
            raise SystemExit('downscalebench: the downscaled run and the %s differ in their bits' % what)
    calls = {'downscaled': call_a, 'materialised': call_b, 'run': call_c}
    inner = {}
    for name, fn in calls.items():
        ms = timed(fn, 1)                      # (the warm-up above loaded the code objects)
        inner[name] = max(1, int(np.ceil(a.window * 1e3 / ms)))
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, fn in calls.items():
            times[name].append(timed(fn, inner[name]))
    eng.check()
    med = {name: float(np.median(t)) for name, t in times.items()}
    gbps = lambda nbytes, ms: nbytes * n / (ms * 1e-3) / 1e9
    res = {'tool': 'downscalebench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'dtype': 'float64', 'pixels': n, 'coarse_grid': [H, W], 'method': 'bilinear', 'coarse_drivers': len(COARSE),
           'copy_kernel_gbps': round(copy_gbps, 1),
           'downscaled_ms': round(med['downscaled'], 4), 'materialised_ms': round(med['materialised'], 4),
           'run_ms': round(med['run'], 4),
           'downscaled_over_materialised': round(med['downscaled'] / med['materialised'], 4),
           'downscaled_over_run': round(med['downscaled'] / med['run'], 4),
           'ps_per_pixel': {name: round(ms * 1e9 / n, 2) for name, ms in med.items()},
           'bytes_per_pixel_counted': {'downscaled': BYTES_DOWNSCALED, 'materialised': BYTES_MATERIALISED, 'run': BYTES_RUN},
           'fraction_of_copy_rate': {'downscaled': round(gbps(BYTES_DOWNSCALED, med['downscaled']) / copy_gbps, 4),
                                     'run': round(gbps(BYTES_RUN, med['run']) / copy_gbps, 4)},
           'driver_bytes_on_device': {'downscaled': 3 * 8 * n + 11 * 8 * H * W, 'materialised': 14 * 8 * n},
           'ms_all': {name: [round(t, 4) for t in ts] for name, ts in times.items()},
           'launches_per_window': inner, 'same_bits': True}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
