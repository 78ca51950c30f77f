#!/usr/bin/env python3
"""Upscaling (RasterEngine.upscale_grid: mod16_upscale_f32, mod16_upscale_classes) against the torch
passes it replaces, in one GPU process, resident, float32:

  (a) one layer of the global 30-arc-second grid, 43200 x 21600, onto 0.05 degrees, 7200 x 3600 (6 x 6
      cells), area = cos(latitude); torch: the (3600, 6, 7200, 6) view, the weighted nansum and the
      weighted valid count over the two block axes, in float64, --chunk coarse rows at a time
  (b) the same raster onto MERRA-2's 361 x 576 grid (60 x 75 cells, 30 rows at the poles, the first
      column straddling the date line; wrap); torch: index_add_ of the weighted values and of the
      weights of the valid pixels over a resident int32 cell-id raster (float64 sums, float atomics)
  (c) 46 layers of 2400 x 2400 onto 200 x 200 (12 x 12 cells), no area; torch: as (a)
  (d) the class raster of (a) (uint8, 13 codes) onto 0.05 degrees; torch: one (3600, 6, 7200, 6) count
      per code and the largest count, the lowest code on a tie

The kernel and the torch passes must agree before anything is timed: NaN at the same places and the
mean to 1e-5 relative (float32 outputs; the torch reductions sum in another order), the classes
equal. Device events on the current stream; one warm-up of each, then --repeats alternating repeats:
windows of at least --window seconds of the kernel, one pass of torch; the medians. The engine's copy
kernel (measure_copy) runs in the same process. One JSON line: per case the two times, their ratio,
picoseconds per pixel-layer, and the bytes counted (the input read once -- 4 B per pixel-layer, 1 B for
the classes -- plus the outputs written) as a rate and as a share of the copy kernel's. No threshold:
the torch passes and the copy kernel are the yardsticks.

  python tools/upscalebench.py [--out FILE] [--scale 1] [--chunk 360] [--repeats 5] [--window 0.25]
(--scale N divides the global raster's extents by N: a smoke run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mod16_amd import _lib, downscale as ds, upscale as up  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402


def make_values(dev, K, R, C, seed):
    """gamma-like positive values, 10 % missing; made row block by row block (no temporary of the raster's size)"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    v = torch.empty((K, R, C), device=dev, dtype=torch.float32)
    step = max(1, (1 << 26) // C)
    for k in range(K):
        for r in range(0, R, step):
            a = torch.rand((min(step, R - r), C), device=dev, generator=gen) * 30.0 + 1.0
            a[torch.rand(a.shape, device=dev, generator=gen) < 0.1] = float('nan')
            v[k, r:r + step] = a
    return v


def block_means(v, fr, fc, area, chunk, out):
    """torch, integer ratios: (K, R, C) -> out (K, H, W) float32"""
    K, R, C = v.shape
    H, W = R // fr, C // fc
    for k in range(K):
        for h in range(0, H, chunk):
            n = min(chunk, H - h)
            x = v[k, h * fr:(h + n) * fr].view(n, fr, W, fc).double()
            ok = ~torch.isnan(x)
            if area is None:
                num, den = torch.nansum(x, (1, 3)), ok.sum((1, 3)).double()
            else:
                w = area[h * fr:(h + n) * fr].view(n, fr, 1, 1)
                num = torch.nansum(w * x, (1, 3))
                den = (w * ok).sum((1, 3))
            out[k, h:h + n] = (num / den).float()


def scatter_means(v, ids, area, H, W, chunk_rows, out):
    """torch, any geometry: index_add_ over the cell-id raster `ids` (R, C) int32 -> out (K, H, W) float32"""
    K, R, C = v.shape
    for k in range(K):
        num = torch.zeros(H * W, dtype=torch.float64, device=v.device)
        den = torch.zeros(H * W, dtype=torch.float64, device=v.device)
        for r in range(0, R, chunk_rows):
            x = v[k, r:r + chunk_rows].double()
            ok = ~torch.isnan(x)
            w = area[r:r + chunk_rows, None].expand_as(x)
            idx = ids[r:r + chunk_rows].reshape(-1)
            num.index_add_(0, idx, torch.where(ok, w * x, 0.0).reshape(-1))
            den.index_add_(0, idx, torch.where(ok, w, 0.0).reshape(-1))
        out[k] = (num / den).view(H, W).float()


def block_classes(cls, fr, fc, chunk, out):
    """torch: per code a block count; the largest, the lowest code on a tie -> out (H, W) uint8"""
    R, C = cls.shape
    H, W = R // fr, C // fc
    for h in range(0, H, chunk):
        n = min(chunk, H - h)
        x = cls[h * fr:(h + n) * fr].view(n, fr, W, fc)
        best = torch.zeros((n, W), dtype=torch.int32, device=cls.device)
        win = torch.full((n, W), up.NO_CLASS, dtype=torch.uint8, device=cls.device)
        for c in range(13):
            cnt = (x == c).sum((1, 3), dtype=torch.int32)
            more = cnt > best
            best = torch.where(more, cnt, best)
            win = torch.where(more, torch.full_like(win, c), win)
        out[h:h + n] = win


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def agree(a, b, what):
    if not bool((torch.isnan(a) == torch.isnan(b)).all()):
        raise SystemExit('upscalebench: %s is NaN at other places than the torch passes' % what)
    fin = ~torch.isnan(a)
    err = float(((a[fin] - b[fin]).abs() / b[fin].abs().clamp(min=1.0)).max()) if bool(fin.any()) else 0.0
    if not err <= 1e-5:
        raise SystemExit('upscalebench: %s differs from the torch passes by %g' % (what, err))
    return err


def measure(eng, name, call_a, call_b, check, pixel_layers, counted_bytes, repeats, window, copy_gbps, extra):
    call_a()
    call_b()
    eng.check()
    err = check()
    torch.cuda.empty_cache()
    inner = max(1, int(np.ceil(window * 1e3 / timed(call_a, 1))))
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(call_a, inner))
        tb.append(timed(call_b, 1))
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    gbps = counted_bytes / (a_ms * 1e-3) / 1e9
    res = {'case': name, 'upscale_ms': round(a_ms, 4), 'torch_ms': round(b_ms, 3), 'upscale_over_torch': round(a_ms / b_ms, 5),
           'ps_per_pixel_layer': round(a_ms * 1e9 / pixel_layers, 3), 'bytes_counted': int(counted_bytes),
           'upscale_gbps_counted': round(gbps, 1), 'fraction_of_copy_rate': round(gbps / copy_gbps, 4),
           'max_rel_diff_to_torch': float('%.3g' % err), 'upscale_ms_all': [round(v, 4) for v in ta],
           'torch_ms_all': [round(v, 3) for v in tb], 'launches_per_window': inner, 'agrees_with_torch': True}
    res.update(extra)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--scale', type=int, default=1, help='divide the global raster by this (a smoke run)')
    ap.add_argument('--chunk', type=int, default=360, help='coarse rows per chunk of the torch passes')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window of the kernel, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    dev = eng._dev()
    copy_gbps = float(eng.measure_copy())
    runs = []
    args = (a.repeats, a.window, copy_gbps)

    # the global grid
    R, C = 21600 // a.scale, 43200 // a.scale
    step = 180.0 / R
    lat = 90.0 - step / 2 - step * np.arange(R)
    area_np = np.cos(np.deg2rad(lat))
    area = torch.from_numpy(area_np).to(dev)
    v = make_values(dev, 1, R, C, 7)

    # (a) onto 6 x 6 cells
    H, W = R // 6, C // 6
    grid = eng.upscale_grid((R, C), (H, W), ds.positions(0.5, 1.0, R, 3.0, 6.0), ds.positions(0.5, 1.0, C, 3.0, 6.0), area=area_np)
    assert (grid.row_runs.count == 6).all() and (grid.col_runs.count == 6).all()
    out = dict(mean=torch.empty((1, H, W), dtype=torch.float32, device=dev))
    ref = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    runs.append(measure(eng, 'a: %d x %d onto %d x %d (6 x 6), area' % (C, R, W, H),
                        lambda: grid.run(v, outputs=('mean',), out=out), lambda: block_means(v, 6, 6, area, a.chunk, ref),
                        lambda: agree(out['mean'], ref, 'the mean of (a)'), R * C, 4 * R * C + 4 * H * W, *args,
                        extra={'pixels': R * C, 'cells': H * W}))
    grid.close()

    # (b) onto MERRA-2: 0.5 x 0.625 degrees, cell (0, 0) centred on 90 N, 180 W
    Hm, Wm = 361, 576
    row_pos = ds.positions(90.0 - step / 2, -step, R, 90.0, -0.5)
    col_pos = ds.positions(-180.0 + step / 2, step, C, -180.0, 0.625)
    grid = eng.upscale_grid((R, C), (Hm, Wm), row_pos, col_pos, wrap=True, area=area_np)
    ids_np = up.cell_table(row_pos, Hm).astype(np.int32)[:, None] * Wm + up.cell_table(col_pos, Wm, True).astype(np.int32)[None, :]
    ids = torch.from_numpy(ids_np).to(dev)
    del ids_np
    out = dict(mean=torch.empty((1, Hm, Wm), dtype=torch.float32, device=dev))
    ref = torch.empty((1, Hm, Wm), dtype=torch.float32, device=dev)
    runs.append(measure(eng, 'b: %d x %d onto MERRA-2 %d x %d, wrap, area' % (C, R, Wm, Hm),
                        lambda: grid.run(v, outputs=('mean',), out=out),
                        lambda: scatter_means(v, ids, area, Hm, Wm, a.chunk * 6, ref),
                        lambda: agree(out['mean'], ref, 'the mean of (b)'), R * C, 4 * R * C + 4 * Hm * Wm, *args,
                        extra={'pixels': R * C, 'cells': Hm * Wm, 'cell_id_raster_bytes': 4 * R * C,
                               'col_first': [int(x) for x in grid.col_runs.first[:3]]}))
    grid.close()
    del ids, v

    # (c) 46 layers of a 2400 x 2400 tile onto 12 x 12 cells
    K, T = 46, 2400
    v = make_values(dev, K, T, T, 11)
    grid = eng.upscale_grid((T, T), (T // 12, T // 12), ds.positions(0.5, 1.0, T, 6.0, 12.0), ds.positions(0.5, 1.0, T, 6.0, 12.0))
    out = dict(mean=torch.empty((K, T // 12, T // 12), dtype=torch.float32, device=dev))
    ref = torch.empty((K, T // 12, T // 12), dtype=torch.float32, device=dev)
    runs.append(measure(eng, 'c: %d layers of %d x %d onto %d x %d (12 x 12)' % (K, T, T, T // 12, T // 12),
                        lambda: grid.run(v, outputs=('mean',), out=out), lambda: block_means(v, 12, 12, None, a.chunk, ref),
                        lambda: agree(out['mean'], ref, 'the mean of (c)'), K * T * T, 4 * K * T * T + 4 * K * (T // 12) ** 2, *args,
                        extra={'pixels': T * T, 'layers': K, 'cells': (T // 12) ** 2}))
    grid.close()
    del v

    # (d) the class raster of the global grid onto 6 x 6 cells
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    cls = torch.empty((R, C), dtype=torch.uint8, device=dev)
    rows = max(1, (1 << 26) // C)
    for r in range(0, R, rows):
        cls[r:r + rows] = torch.randint(0, 13, (min(rows, R - r), C), device=dev, generator=gen, dtype=torch.uint8)
    grid = eng.upscale_grid((R, C), (H, W), ds.positions(0.5, 1.0, R, 3.0, 6.0), ds.positions(0.5, 1.0, C, 3.0, 6.0))
    cout = dict(cls=torch.empty((H, W), dtype=torch.uint8, device=dev))
    cref = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def classes_agree():
        if not bool((cout['cls'] == cref).all()):
            raise SystemExit('upscalebench: the classes of (d) differ from the torch passes')
        return 0.0
    runs.append(measure(eng, 'd: classes, %d x %d onto %d x %d (6 x 6)' % (C, R, W, H),
                        lambda: grid.majority(cls, outputs=('cls',), out=cout), lambda: block_classes(cls, 6, 6, a.chunk, cref),
                        classes_agree, R * C, R * C + H * W, *args, extra={'pixels': R * C, 'cells': H * W}))
    grid.close()

    res = {'tool': 'upscalebench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'in': 'float32', 'scale': a.scale, 'torch_chunk_rows': a.chunk, 'copy_kernel_gbps': round(copy_gbps, 1), 'runs': runs}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
