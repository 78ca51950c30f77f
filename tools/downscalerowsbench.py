#!/usr/bin/env python3
"""The downscaled run on MODIS sinusoidal tiles (RasterEngine.downscale_grid(..., col_affine=...): the
column cell pair formed per pixel inside the kernel) against what it replaces, in one GPU process,
float64, resident: four real tiles (h11v04, h12v04, h11v05, h12v05) of 1200 x 1200 pixels, geometry
from mod16_amd.downscale.sinusoidal_positions, over a global 361 x 576 reanalysis grid (0.5 x 0.625
degrees), bilinear, the eleven reanalysis drivers coarse, albedo / fPAR / LAI fine:

  run        (a) affine        grid.run on the four row-affine grids, one call per tile
             (b) rectilinear   grid.run on four rectilinear grids of the same shape (every row with the
                               columns of the tile's middle row): what deriving the columns on the
                               device costs
             (c) row by row    what the documentation recommended before: one rectilinear grid per tile
                               row (1 x 1200, made outside the clock) and one run per row: 4800 calls
  composite  the same three for grid.composite at K = 8 days in one period, the coarse drivers daily

Device events on the current stream; one warm-up of each, then --repeats alternating repeats of windows
of at least --window seconds each; the medians. (a) and (c) must have the same bits -- checked before
anything is timed. One JSON line: the times, their ratios, the launches per window. Exits non-zero only
where the bits differ: the ratios are what is measured.

  python tools/downscalerowsbench.py [--out FILE] [--repeats 5] [--window 0.25] [--size 1200]
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

TILES = ((11, 4), (12, 4), (11, 5), (12, 5))
H, W = 361, 576
GRID = (90.0, -0.5, -180.0, 0.625)          # latitude of row 0 and its step, longitude of column 0 and its step
K = 8
COARSE = [k for k, name in enumerate(ds.DRIVER_NAMES) if name in ds.MET_DRIVERS]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    ap.add_argument('--size', type=int, default=1200, help='pixels per tile side')
    a = ap.parse_args()
    S = a.size
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    n1, n = S * S, len(TILES) * S * S
    cls, fine = eng.synth(n, seed=16)
    _, planes = eng.synth(H * W, seed=16, step=1)
    series = [eng.synth(H * W, seed=20 + t, step=1)[1] for t in range(K)]
    drivers = [planes[k].view(H, W) if k in COARSE else fine[k] for k in range(14)]
    daily = [torch.stack([series[t][k].view(H, W) for t in range(K)]) if k in COARSE else fine[k] for k in range(14)]
    hours = torch.full((n,), 12.0, dtype=eng.dtype, device=eng._dev())     # (a fine array: no per-call upload of a scalar)
    affine, rect, rows = [], [], []
    for h, v in TILES:
        row_pos, origin, scale = ds.sinusoidal_positions(h, v, S, *GRID)
        pos = ds.column_positions(origin, scale, S)
        affine.append(eng.downscale_grid((S, S), (H, W), row_pos, wrap=True, col_affine=(origin, scale)))
        rect.append(eng.downscale_grid((S, S), (H, W), row_pos, pos[S // 2], wrap=True))
        rows.append([eng.downscale_grid((1, S), (H, W), row_pos[r:r + 1], pos[r], wrap=True) for r in range(S)])
    out = {name: eng.empty(n, 2) for name in ('affine', 'rect', 'rows')}
    comp = {name: (torch.empty((1, n), dtype=eng.dtype, device=eng._dev()),
                   torch.empty((1, n), dtype=torch.uint16, device=eng._dev())) for name in ('affine', 'rect', 'rows')}

    def part(arrays, lo, hi):
        return [d if k in COARSE else d[lo:hi] for k, d in enumerate(arrays)]

    def run_tiles(grids, o):
        for t, g in enumerate(grids):
            lo, hi = t * n1, (t + 1) * n1
            g.run(cls[lo:hi], part(drivers, lo, hi), out_day=o[0][lo:hi], out_night=o[1][lo:hi])

    def run_rows(o):
        for t, grids in enumerate(rows):
            for r, g in enumerate(grids):
                lo = t * n1 + r * S
                g.run(cls[lo:lo + S], part(drivers, lo, lo + S), out_day=o[0][lo:lo + S], out_night=o[1][lo:lo + S])

    def comp_tiles(grids, o):
        for t, g in enumerate(grids):
            lo, hi = t * n1, (t + 1) * n1
            g.composite(cls[lo:hi], part(daily, lo, hi), hours[lo:hi], K, K, out=[o[0][:, lo:hi], o[1][:, lo:hi]])

    def comp_rows(o):
        for t, grids in enumerate(rows):
            for r, g in enumerate(grids):
                lo = t * n1 + r * S
                g.composite(cls[lo:lo + S], part(daily, lo, lo + S), hours[lo:lo + S], K, K, out=[o[0][:, lo:lo + S], o[1][:, lo:lo + S]])

    calls = {'run_affine': lambda: run_tiles(affine, out['affine']), 'run_rectilinear': lambda: run_tiles(rect, out['rect']),
             'run_row_by_row': lambda: run_rows(out['rows']),
             'composite_affine': lambda: comp_tiles(affine, comp['affine']),
             'composite_rectilinear': lambda: comp_tiles(rect, comp['rect']),
             'composite_row_by_row': lambda: comp_rows(comp['rows'])}
    for fn in calls.values():
        fn()
    eng.check()
    if not (same_bits(out['affine'][0], out['rows'][0]) and same_bits(out['affine'][1], out['rows'][1])):
        raise SystemExit('downscalerowsbench: the row-affine run and the run row by row differ in their bits')
    if not (same_bits(comp['affine'][0], comp['rows'][0]) and same_bits(comp['affine'][1], comp['rows'][1])):
        raise SystemExit('downscalerowsbench: the row-affine composite and the composite row by row differ in their bits')
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
    ratio = lambda x, y: round(med[x] / med[y], 4)
    res = {'tool': 'downscalerowsbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'dtype': 'float64', 'tiles': ['h%02dv%02d' % t for t in TILES], 'tile_size': S, 'pixels': n,
           'coarse_grid': [H, W], 'method': 'bilinear', 'coarse_drivers': len(COARSE), 'composite_days': K,
           'ms': {name: round(ms, 4) for name, ms in med.items()},
           'ps_per_pixel': {name: round(ms * 1e9 / n, 2) for name, ms in med.items()},
           'run_affine_over_rectilinear': ratio('run_affine', 'run_rectilinear'),
           'run_row_by_row_over_affine': ratio('run_row_by_row', 'run_affine'),
           'composite_affine_over_rectilinear': ratio('composite_affine', 'composite_rectilinear'),
           'composite_row_by_row_over_affine': ratio('composite_row_by_row', 'composite_affine'),
           'calls_per_pass': {'affine': len(TILES), 'rectilinear': len(TILES), 'row_by_row': len(TILES) * S},
           'ms_all': {name: [round(t, 4) for t in ts] for name, ts in times.items()},
           'passes_per_window': inner, 'same_bits': True}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
