#!/usr/bin/env python3
"""Upscaling from sinusoidal tiles (RasterEngine.upscale_grid(col_affine=...): the row-affine walk of
mod16_upscale_f32 and mod16_upscale_classes) against what it costs over the rectilinear walk and against
what it replaces, in one GPU process, resident, float32:

  (a) four 1200 x 1200 tiles -- (17, 0) at the pole, (35, 9) at the date line, (17, 3) and (20, 8) --, 46
      layers each, onto MERRA-2's 361 x 576 grid with wrap, on-globe columns (downscale.sinusoidal_columns)
  (b) the same tiles onto a 0.05-degree window of their own (coarse_*_first shifted to the tile), no wrap
  (c) the class raster of a 2400 x 2400 tile, (17, 3), onto 361 x 576

Yardsticks, per tile and in the same process:
  rectilinear   grid.run on a rectilinear grid of the same shape whose columns are those of the tile's
                middle row (the same mean cell size): the price of the per-row geometry as a ratio
  zonal         engine.zonal over an int32 cell-id raster (4 B per pixel more, global 64-bit atomics) into
                an accumulator that is reset on the device before every call (a device copy of K x cells x 80
                B, counted in its time: a fresh accumulator per call would be built on the host and uploaded)
  index_add     torch index_add_ of the values and of the valid pixels over the same raster (float64 sums,
                float atomics; what upscalebench's case (b) uses); ONE timed pass per tile, not repeated
  copy          the engine's copy kernel for the bytes counted: 4 B per pixel-layer read (1 B for the
                classes) plus the outputs written

The kernel must agree with the index_add pass before anything is timed (NaN at the same places, the mean to
1e-5 relative: float32 outputs, another order of summation) and with the cell counts of the definition's
tables. Device events on the current stream, one warm-up of each, then --repeats alternating repeats of
windows of at least --window seconds of the three kernels; the medians. One JSON line. No threshold.

  python tools/upscalerowsbench.py [--out FILE] [--cases abc] [--size 1200] [--layers 46] [--repeats 5] [--window 0.25]
(progress goes to stderr, one line per case)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mod16_amd import _lib, downscale as ds, upscale as up, zonal as zs  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402
from upscalebench import agree, make_values, timed  # noqa: E402

TILES = ((17, 0), (35, 9), (17, 3), (20, 8))


def tile_geometry(h, v, size, window):
    """-> (coarse shape, row_pos, origin, scale, col_range, wrap): MERRA-2 with wrap, or a 0.05-degree window"""
    col_range = ds.sinusoidal_columns(h, v, size)
    if not window:
        row_pos, origin, scale = ds.sinusoidal_positions(h, v, size, 90.0, -0.5, -180.0, 0.625)
        return (361, 576), row_pos, origin, scale, col_range, True
    row_pos, origin, scale = ds.sinusoidal_positions(h, v, size, 0.0, -0.05, 0.0, 0.05)      # cells from (0 N, 0 E)
    first, count = (t.astype(np.int64) for t in col_range)
    on = count > 0
    ends = np.concatenate([(origin + scale * first)[on], (origin + scale * (first + count - 1))[on]])
    j0, i0 = int(np.floor(ends.min())), int(np.floor(row_pos.min()))
    W, H = int(np.ceil(ends.max())) - j0 + 1, int(np.ceil(row_pos.max())) - i0 + 1
    return (H, W), row_pos - i0, origin - j0, scale, col_range, False


def cell_ids(shape, coarse, row_pos, origin, scale, col_range, wrap):
    H, W = coarse
    rows = up.cell_table(row_pos, H).astype(np.int64)
    cols = up.cell_table_rows(origin, scale, shape[1], W, wrap, col_range).astype(np.int64)
    ids = np.where((rows[:, None] >= 0) & (cols >= 0), rows[:, None] * W + cols, -1)
    return ids.astype(np.int32)


def scatter(v, ids, ok_ids, H, W, out):
    """torch: index_add_ over the cell-id raster (ids < 0: no cell) -> out (K, H, W) float32"""
    K = v.shape[0]
    idx = ids.reshape(-1)[ok_ids]
    for k in range(K):
        x = v[k].reshape(-1)[ok_ids].double()
        ok = ~torch.isnan(x)
        num = torch.zeros(H * W, dtype=torch.float64, device=v.device).index_add_(0, idx, torch.where(ok, x, 0.0))
        den = torch.zeros(H * W, dtype=torch.float64, device=v.device).index_add_(0, idx, ok.double())
        out[k] = (num / den).view(H, W).float()


def medians(calls, repeats, window):
    """{name: call} -> {name: (median ms, all)}; the first call sets the launches per window"""
    names = list(calls)
    for n in names:
        calls[n]()
    torch.cuda.synchronize()
    inner = {n: max(1, int(np.ceil(window * 1e3 / max(timed(calls[n], 1), 1e-3)))) for n in names}
    times = {n: [] for n in names}
    for _ in range(repeats):
        for n in names:
            times[n].append(timed(calls[n], inner[n]))
    return {n: (float(np.median(t)), [round(x, 4) for x in t]) for n, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--cases', default='abc')
    ap.add_argument('--size', type=int, default=1200)
    ap.add_argument('--layers', type=int, default=46)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25)
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250), dtype='float32')      # (zonal takes the engine's dtype)
    dev = eng._dev()
    copy_gbps = float(eng.measure_copy())
    K, T = a.layers, a.size
    v = make_values(dev, K, T, T, 11)
    runs = []
    for window in [w for w, c in ((False, 'a'), (True, 'b')) if c in a.cases]:
        for h, t in TILES:
            coarse, row_pos, origin, scale, col_range, wrap = tile_geometry(h, t, T, window)
            H, W = coarse
            grid = eng.upscale_grid((T, T), coarse, row_pos, wrap=wrap, col_affine=(origin, scale), col_range=col_range)
            mid = T // 2
            col_pos = origin[mid] + scale[mid] * np.arange(T)
            if wrap and abs(scale[mid]) * (T - 1) > W - 2:
                rect = None                                          # (the middle row of a polar tile laps: no rectilinear twin)
            else:
                rect = eng.upscale_grid((T, T), coarse, row_pos, col_pos, wrap=wrap)
            ids_np = cell_ids((T, T), coarse, row_pos, origin, scale, col_range, wrap)
            ids = torch.from_numpy(ids_np).to(dev)
            ok_ids = torch.nonzero(ids.reshape(-1) >= 0).reshape(-1)
            out = dict(mean=torch.empty((K, H, W), dtype=torch.float32, device=dev), count=torch.empty((K, H, W), dtype=torch.int32, device=dev))
            rout = dict(mean=torch.empty((K, H, W), dtype=torch.float32, device=dev))
            ref = torch.empty((K, H, W), dtype=torch.float32, device=dev)
            flat = v.view(K, T * T)
            bounds = eng.zonal_bounds(flat)
            fresh = torch.from_numpy(zs.empty(K, H * W)).to(dev)        # (built on the host once per tile)
            acc = torch.empty_like(fresh)

            def zonal():
                acc.copy_(fresh)
                eng.zonal(flat, ids.view(-1), H * W, bounds=bounds, acc=acc)
            calls = {'rows': lambda: grid.run(v, outputs=('mean',), out=dict(mean=out['mean']))}
            if rect is not None:
                calls['rectilinear'] = lambda: rect.run(v, outputs=('mean',), out=rout)
            calls['zonal'] = zonal
            grid.run(v, outputs=('mean', 'count'), out=out)
            scatter(v[:1], ids, ok_ids, H, W, ref[:1])                 # (warm-up: one layer)
            # one timed pass, the one the agreement is checked on: where a tile meets a few hundred cells the
            # float atomics land on as many words and a pass takes 10 to 25 s (measured), so it is not repeated
            index_add_ms = timed(lambda: scatter(v, ids, ok_ids, H, W, ref), 1)
            eng.check()
            err = agree(out['mean'], ref, 'the mean of tile (%d, %d)' % (h, t))
            pixels = np.bincount(ids_np[ids_np >= 0], minlength=H * W).reshape(H, W)
            if not bool((out['count'].amax(0).cpu().numpy() <= pixels).all()):
                raise SystemExit('upscalerowsbench: the counts of tile (%d, %d) exceed the cells of the tables' % (h, t))
            med = medians(calls, a.repeats, a.window)
            ms = med['rows'][0]
            counted = 4 * K * int((ids_np >= 0).sum()) + 4 * K * H * W
            res = {'case': '%s: tile (%d, %d) %d x %d x %d onto %d x %d' % ('b' if window else 'a', h, t, K, T, T, H, W),
                   'rows_ms': round(ms, 4), 'ps_per_pixel_layer': round(ms * 1e9 / (K * T * T), 3),
                   'touched_cells': int((pixels > 0).sum()), 'pixels_in_cells': int(pixels.sum()),
                   'bytes_counted': counted, 'rows_gbps_counted': round(counted / (ms * 1e-3) / 1e9, 1),
                   'fraction_of_copy_rate': round(counted / (ms * 1e-3) / 1e9 / copy_gbps, 4), 'max_rel_diff_to_index_add': float('%.3g' % err)}
            for n in ('rectilinear', 'zonal'):
                if n in med:
                    res[n + '_ms'] = round(med[n][0], 4)
                    res['rows_over_' + n] = round(ms / med[n][0], 4)
            res['index_add_ms'], res['rows_over_index_add'] = round(index_add_ms, 1), float('%.3g' % (ms / index_add_ms))
            res['rows_ms_all'] = med['rows'][1]
            runs.append(res)
            print('upscalerowsbench: %s' % json.dumps(res), file=sys.stderr, flush=True)
            grid.close()
            if rect is not None:
                rect.close()
            del ids, ok_ids, out, rout, ref, fresh, acc
    del v
    if 'c' in a.cases:
        runs.append(classes_case(eng, dev, T, copy_gbps, a))
        print('upscalerowsbench: %s' % json.dumps(runs[-1]), file=sys.stderr, flush=True)
    res = {'tool': 'upscalerowsbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device), 'in': 'float32',
           'size': T, 'layers': K, 'copy_kernel_gbps': round(copy_gbps, 1), 'runs': runs}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


def classes_case(eng, dev, T, copy_gbps, a):
    """(c) the class raster of a 2400 x 2400 tile"""
    T2 = 2 * T
    coarse, row_pos, origin, scale, col_range, wrap = tile_geometry(17, 3, T2, False)
    H, W = coarse
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    cls = torch.randint(0, 13, (T2, T2), device=dev, generator=gen, dtype=torch.uint8)
    grid = eng.upscale_grid((T2, T2), coarse, row_pos, wrap=True, col_affine=(origin, scale), col_range=col_range)
    mid = T2 // 2
    rect = eng.upscale_grid((T2, T2), coarse, row_pos, origin[mid] + scale[mid] * np.arange(T2), wrap=True)
    cout, rcout = dict(cls=torch.empty((H, W), dtype=torch.uint8, device=dev)), dict(cls=torch.empty((H, W), dtype=torch.uint8, device=dev))
    ids_np = cell_ids((T2, T2), coarse, row_pos, origin, scale, col_range, wrap)
    ids = torch.from_numpy(ids_np).to(dev).view(-1).long()
    inside = ids >= 0
    grid.majority(cls, outputs=('cls',), out=cout)
    votes = torch.zeros(13 * H * W, dtype=torch.int32, device=dev)
    votes.index_add_(0, (cls.view(-1).long() * (H * W) + ids)[inside], torch.ones(int(inside.sum()), dtype=torch.int32, device=dev))
    votes = votes.view(13, H * W)
    best = votes.max(0).values
    first_max = (votes == best[None]).int().argmax(0)                  # the lowest code on a tie
    want = torch.where(best > 0, first_max, torch.full_like(first_max, up.NO_CLASS)).to(torch.uint8)
    eng.check()
    if not bool((cout['cls'].view(-1) == want).all()):
        raise SystemExit('upscalerowsbench: the classes of (c) differ from the torch pass')
    med = medians({'rows': lambda: grid.majority(cls, outputs=('cls',), out=cout),
                   'rectilinear': lambda: rect.majority(cls, outputs=('cls',), out=rcout)}, a.repeats, a.window)
    ms = med['rows'][0]
    counted = int(inside.sum()) + H * W
    return {'case': 'c: classes, tile (17, 3) %d x %d onto %d x %d' % (T2, T2, H, W), 'rows_ms': round(ms, 4),
                 'ps_per_pixel': round(ms * 1e9 / (T2 * T2), 3), 'rectilinear_ms': round(med['rectilinear'][0], 4),
                 'rows_over_rectilinear': round(ms / med['rectilinear'][0], 4), 'bytes_counted': counted,
                 'fraction_of_copy_rate': round(counted / (ms * 1e-3) / 1e9 / copy_gbps, 4), 'rows_ms_all': med['rows'][1]}


if __name__ == '__main__':
    main()
