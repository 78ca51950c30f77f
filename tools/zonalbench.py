#!/usr/bin/env python3
"""The zonal reduction (RasterEngine.zonal, mod16_zonal_*) against the torch passes it replaces, in
one GPU process, resident: K = 46 layers (a year of 8-day composites) of 4 x 1200 x 1200 float64
pixels laid out as a 2400 x 2400 raster, per-row weights (the area of a latitude row), 5 % NaN, and
two zone maps:

  class   the uint8 class raster as zones (Z = 13, blocks of 50 x 70 pixels): the LDS path
  basins  a synthetic int32 map of 45 x 45 = 2025 square basins of 54 x 54 pixels: more zones than the
          LDS table holds, so every run of a lane goes to the accumulator with global 64-bit integer
          atomics -- the rate the design rests on and no guide gives

  (a) zonal   one call for all layers (explicit bounds: no pre-pass)
  (b) torch   what a user wrote before, per layer: the product w * x with the NaNs zeroed, torch.bincount
              of it, torch.bincount of the weights of the valid pixels, and the count

(a) is checked against (b) before anything is timed: counts equal, sums to 1e-9 relative (the float
atomics of bincount are what moves). Device events on the current stream; one warm-up of each, then
--repeats alternating repeats of windows of at least --window seconds each; the medians. The engine's
copy kernel (measure_copy) runs in the same process. One JSON line: per zone map the bytes counted per
pixel-layer (the value and the zone id read), both times, the counted rate of (a), that rate as a
share of the copy kernel's, and the ratio to (b). No threshold: the torch passes and the copy kernel
are the yardsticks.

  python tools/zonalbench.py [--out FILE] [--layers 46] [--side 2400] [--repeats 5] [--window 0.25]
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
from mod16_amd import zonal as zs  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

BOUNDS = (1.0, 8.0)      # row areas in (0, 1], values in [0, 5)


def make_inputs(dev, K, side):
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    n = side * side
    x = torch.rand((K, n), dtype=torch.float64, device=dev, generator=gen) * 5.0
    x[torch.rand((K, n), device=dev, generator=gen) < 0.05] = float('nan')
    row = torch.arange(side, device=dev).repeat_interleave(side)
    col = torch.arange(side, device=dev).repeat(side)
    cls = ((row // 50 + col // 70) % 13).to(torch.uint8)
    per = (side + 44) // 45
    basins = ((row // per) * 45 + col // per).to(torch.int32)
    area = torch.cos(torch.linspace(-1.2, 1.2, side, dtype=torch.float64, device=dev))
    return x, cls, basins, area


def torch_passes(x, zones64, w, Z):
    """(b): per layer the product, two bincounts with weights, and the count."""
    out = []
    for k in range(x.shape[0]):
        valid = ~torch.isnan(x[k])
        wx = torch.where(valid, w * x[k], 0.0)
        out.append((torch.bincount(zones64, weights=wx, minlength=Z),
                    torch.bincount(zones64, weights=torch.where(valid, w, 0.0), minlength=Z),
                    torch.bincount(zones64, weights=valid.double(), minlength=Z)))
    return out


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench(eng, name, x, zones, Z, area, side, repeats, window, copy_gbps):
    K, n = x.shape
    zones64 = zones.long()
    w = area.repeat_interleave(side)
    fresh = torch.from_numpy(zs.empty(K, Z)).to(x.device)
    acc = fresh.clone()

    def call_a():
        acc.copy_(fresh)
        eng.zonal(x, zones, Z, area=area, cols=side, bounds=BOUNDS, acc=acc)

    def call_b():
        return torch_passes(x, zones64, w, Z)
    call_a()
    want = call_b()
    torch.cuda.synchronize()
    res = zs.ZonalResult.from_tensor(acc)
    if res.rejected.any():
        raise SystemExit('zonalbench: %s: pixels outside the bounds' % name)
    for k, (swx, sw, cnt) in enumerate(want):
        if not np.array_equal(res.count[k], cnt.cpu().numpy().astype(np.int64)) or \
                not np.allclose(res.sum_wx[k], swx.cpu().numpy(), rtol=1e-9, atol=0) or \
                not np.allclose(res.sum_w[k], sw.cpu().numpy(), rtol=1e-9, atol=0):
            raise SystemExit('zonalbench: %s: layer %d differs from the torch passes' % (name, k))
    del want
    inner = {}
    for key, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)
        inner[key] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    a, b = float(np.median(times['a'])), float(np.median(times['b']))
    counted = x.element_size() + zones.element_size()
    gbps = counted * n * K / (a * 1e-3) / 1e9
    return {'zones': name, 'nzones': Z, 'zone_bytes': zones.element_size(),
            'path': 'lds' if Z <= _lib.zonal_lds_zones() else 'global', 'zonal_ms': round(a, 4), 'torch_ms': round(b, 4),
            'zonal_over_torch': round(a / b, 4), 'bytes_per_pixel_layer_counted': counted,
            'zonal_gbps_counted': round(gbps, 1), 'fraction_of_copy_rate': round(gbps / copy_gbps, 4),
            'ps_per_pixel_layer': round(a * 1e9 / (n * K), 3), 'zonal_ms_all': [round(v, 4) for v in times['a']],
            'torch_ms_all': [round(v, 4) for v in times['b']], 'launches_per_window': inner, 'agrees_with_torch': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--layers', type=int, default=46)
    ap.add_argument('--side', type=int, default=2400)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    x, cls, basins, area = make_inputs(eng._dev(), a.layers, a.side)
    res = {'tool': 'zonalbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'layers': a.layers, 'pixels': a.side * a.side, 'dtype': 'float64', 'weights': 'per row',
           'lds_zones': _lib.zonal_lds_zones(), 'copy_kernel_gbps': round(copy_gbps, 1), 'runs': []}
    for name, zones, Z in (('class', cls, 13), ('basins', basins, 45 * 45)):
        res['runs'].append(bench(eng, name, x, zones, Z, area, a.side, a.repeats, a.window, copy_gbps))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
