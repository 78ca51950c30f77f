#!/usr/bin/env python3
"""Exact zonal quantiles and zonal histograms (RasterEngine.zonal_quantiles / zonal_histogram,
mod16_zonal_hist_*, mod16_zonal_select) against the torch passes they replace, in one GPU process,
resident: K = 46 layers (a year of 8-day composites) of 4 x 1200 x 1200 pixels laid out as a 2400 x
2400 raster, float32 and float64, per-row weights (the area of a latitude row), 5 % NaN, q = (0.05,
0.5, 0.95), and the zone maps of tools/zonalbench.py:

  class   the uint8 class raster as zones (Z = 13, blocks of 50 x 70 pixels)
  basins  a synthetic int32 map of 45 x 45 = 2025 square basins

  (a) class, quantiles with bits = 8 (the LDS table at every level) and bits = 11 (fewer levels, the
      table in global memory)
  (b) basins, quantiles with the default bits
  (c) the uniform histogram with 256 bins, both maps
  (d) class, quantiles of a raster of one constant value: every pixel of every level lands on one
      word per zone and slot. Time only.
  torch   what a user wrote before. Quantiles, per layer: a stable torch.sort by value, then by zone, a
          cumulative sum of the float weights and a searchsorted per zone and q. Histogram, per layer:
          torch.bincount of zone * (bins + 2) + bin with the weights.
  zonal   engine.zonal on the same inputs (one pass; the moments)

Every result is checked against its torch counterpart before anything is timed: quantiles to 1e-3
absolute (the float cumulative sum may pick a neighbour of the exact order statistic; the values are
uniform on [0, 5)), the constant raster exactly, histogram words to 1e-6 relative. Device events on the
current stream; one warm-up of each, then --repeats alternating repeats of windows of at least
--window seconds each; the medians. The engine's copy kernel (measure_copy) runs in the same process.
Every GPU step runs under its own time limit (--limit seconds: a watchdog thread ends the process),
and the tool stops at the first failure. One JSON line: per run the time, the ps per pixel-layer and
level, the bytes counted per pixel-layer and level (the value and the zone id read), the counted rate
as a share of the copy kernel's, and the ratio to the torch passes.

  python tools/zonalqbench.py [--out FILE] [--layers 46] [--side 2400] [--repeats 5] [--window 0.25] [--limit 240]
"""
import argparse
import faulthandler
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mod16_amd import _lib  # noqa: E402
from mod16_amd import zonal as zs  # noqa: E402
from mod16_amd import zonalq as zq  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

Q = (0.05, 0.5, 0.95)
WMAX = 1.0               # row areas in (0, 1]
RANGE = (0.0, 5.0)       # values in [0, 5)
BINS = 256
LIMIT = [240]


class step(object):
    """A GPU step under its own time limit: past it a watchdog thread dumps the stacks and ends the process."""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        print('zonalqbench: %s' % self.what, file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(LIMIT[0], exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def make_inputs(dev, K, side, dtype):
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    n = side * side
    x = (torch.rand((K, n), dtype=torch.float64, device=dev, generator=gen) * 5.0).to(dtype)
    x[torch.rand((K, n), device=dev, generator=gen) < 0.05] = float('nan')
    row = torch.arange(side, device=dev).repeat_interleave(side)
    col = torch.arange(side, device=dev).repeat(side)
    cls = ((row // 50 + col // 70) % 13).to(torch.uint8)
    per = (side + 44) // 45
    basins = ((row // per) * 45 + col // per).to(torch.int32)
    area = torch.cos(torch.linspace(-1.2, 1.2, side, dtype=torch.float64, device=dev))
    return x, cls, basins, area


def torch_quantiles(x, zones64, w, Z, q):
    """Per layer: stable sort by value, then by zone (NaN to a zone of its own), cumulative float weights, searchsorted."""
    out = []
    ids = torch.arange(Z + 1, device=x.device)
    for k in range(x.shape[0]):
        vs, i1 = torch.sort(x[k], stable=True)
        z1 = torch.where(torch.isnan(vs), Z, zones64[i1])
        z2, i2 = torch.sort(z1, stable=True)
        vs, ws = vs[i2], w[i1][i2]
        cw = torch.cumsum(ws, 0)
        start = torch.searchsorted(z2, ids)                      # first index of each zone; [Z]: the NaNs
        base = torch.where(start[:-1] > 0, cw[(start[:-1] - 1).clamp(min=0)], 0.0)
        top = torch.where(start[1:] > 0, cw[(start[1:] - 1).clamp(min=0)], 0.0)
        want = base[:, None] + q[None, :] * (top - base)[:, None]
        idx = torch.searchsorted(cw, want.reshape(-1)).reshape(Z, -1)
        idx = torch.minimum(torch.maximum(idx, start[:-1, None]), (start[1:, None] - 1).clamp(min=0))
        out.append(torch.where((start[1:] > start[:-1])[:, None], vs[idx], float('nan')))
    return torch.stack(out)


def torch_histogram(x, zones64, w, Z):
    lo, hi = RANGE
    scale = BINS / (hi - lo)
    out = []
    for k in range(x.shape[0]):
        v = x[k].double()
        b = torch.where(v < lo, 0, torch.where(v < hi, ((v - lo) * scale).floor().clamp(max=BINS - 1).long() + 1, BINS + 1))
        valid = ~torch.isnan(v)
        out.append(torch.bincount(zones64 * (BINS + 2) + torch.where(valid, b, 0), weights=torch.where(valid, w, 0.0),
                                  minlength=Z * (BINS + 2)).reshape(Z, BINS + 2))
    return torch.stack(out)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(name, call_a, call_b, repeats, window):
    """Medians of `repeats` alternating windows of at least `window` seconds; call_b may be None."""
    calls = {'a': call_a, 'b': call_b} if call_b else {'a': call_a}
    inner, times = {}, {}
    for key, fn in calls.items():
        with step('%s: sizing the window of (%s)' % (name, key)):
            inner[key] = max(1, int(np.ceil(window * 1e3 / timed(fn, 1))))
        times[key] = []
    for r in range(repeats):
        for key, fn in calls.items():
            with step('%s: repeat %d of (%s)' % (name, r, key)):
                times[key].append(timed(fn, inner[key]))
    return {k: float(np.median(v)) for k, v in times.items()}, times, inner


def report(name, what, x, zones, Z, levels, med, times, inner, copy_gbps, extra):
    K, n = x.shape
    counted = x.element_size() + zones.element_size()
    a = med['a']
    gbps = counted * n * K * levels / (a * 1e-3) / 1e9
    out = {'run': name, 'what': what, 'nzones': Z, 'zone_bytes': zones.element_size(), 'levels': levels, 'ms': round(a, 4),
           'ps_per_pixel_layer_level': round(a * 1e9 / (n * K * levels), 3), 'bytes_per_pixel_layer_level_counted': counted,
           'gbps_counted': round(gbps, 1), 'fraction_of_copy_rate': round(gbps / copy_gbps, 4),
           'ms_all': [round(v, 4) for v in times['a']], 'launches_per_window': inner}
    if 'b' in med:
        out.update(torch_ms=round(med['b'], 4), over_torch=round(a / med['b'], 4), not_slower_than_torch=bool(a <= med['b']),
                   torch_ms_all=[round(v, 4) for v in times['b']], agrees_with_torch=True)
    out.update(extra)
    return out


def bench_dtype(eng, K, side, repeats, window, copy_gbps):
    x, cls, basins, area = make_inputs(eng._dev(), K, side, eng.dtype)
    n = side * side
    w = area.repeat_interleave(side)
    q = torch.tensor(Q, dtype=torch.float64, device=x.device)
    wd = 8 * x.element_size()
    runs = []
    lds = _lib.zonal_hist_lds_bytes()
    for name, zones, Z, bits_list in (('class', cls, 13, (8, 11)), ('basins', basins, 45 * 45, (zq.DEFAULT_BITS,))):
        zones64 = zones.long()
        with step('%s: the torch quantile passes' % name):
            want = torch_quantiles(x, zones64, w, Z, q).cpu().numpy()
        with step('%s: engine.zonal' % name):
            fresh = torch.from_numpy(zs.empty(K, Z)).to(x.device)
            acc = fresh.clone()

            def call_z():
                acc.copy_(fresh)
                eng.zonal(x, zones, Z, area=area, cols=side, bounds=(WMAX, 8.0), acc=acc)
            call_z()
            torch.cuda.synchronize()
        zonal_ms = alternate('%s: engine.zonal' % name, call_z, None, repeats, window)[0]['a']
        for bits in bits_list:
            def call_a():
                return eng.zonal_quantiles(x, zones, Z, Q, area=area, cols=side, wmax=WMAX, bits=bits)

            def call_b():
                return torch_quantiles(x, zones64, w, Z, q)
            with step('%s: quantiles, bits %d, checked against the torch passes' % (name, bits)):
                got = call_a().values
                if not np.allclose(got, want, rtol=0, atol=1e-3, equal_nan=True):
                    raise SystemExit('zonalqbench: %s, bits %d: quantiles differ from the torch passes by %g'
                                     % (name, bits, np.nanmax(np.abs(got - want))))
            med, times, inner = alternate('%s quantiles bits %d' % (name, bits), call_a, call_b, repeats, window)
            levels = zq.levels(wd, bits)
            table = Z * len(Q) * (8 << bits)
            runs.append(report(name, 'quantiles', x, zones, Z, levels, med, times, inner, copy_gbps,
                               {'bits': bits, 'table': 'lds' if table <= lds else 'global', 'zonal_ms': round(zonal_ms, 4),
                                'level_over_zonal': round(med['a'] / levels / zonal_ms, 4)}))

        def hist_a():
            return eng.zonal_histogram(x, zones, Z, BINS, RANGE, area=area, cols=side, wmax=WMAX)

        def hist_b():
            return torch_histogram(x, zones64, w, Z)
        with step('%s: histogram, checked against torch.bincount' % name):
            got = hist_a().cpu().numpy() * 2.0 ** -31
            ref = hist_b().cpu().numpy()
            if not np.allclose(got, ref, rtol=1e-6, atol=1e-6):
                raise SystemExit('zonalqbench: %s: the histogram differs from torch.bincount' % name)
        med, times, inner = alternate('%s histogram' % name, hist_a, hist_b, repeats, window)
        runs.append(report(name, 'histogram', x, zones, Z, 1, med, times, inner, copy_gbps,
                           {'bins': BINS, 'table': 'lds' if Z * (BINS + 2) * 8 <= lds else 'global', 'zonal_ms': round(zonal_ms, 4),
                            'level_over_zonal': round(med['a'] / zonal_ms, 4)}))
        del want
        torch.cuda.empty_cache()
    # (d) the constant raster: correct, and its time
    x.fill_(2.5)
    with step('constant raster: quantiles'):
        got = eng.zonal_quantiles(x, cls, 13, Q, area=area, cols=side, wmax=WMAX).values
        if not (got == 2.5).all():
            raise SystemExit('zonalqbench: the constant raster gave other values')
    med, times, inner = alternate('constant raster', lambda: eng.zonal_quantiles(x, cls, 13, Q, area=area, cols=side, wmax=WMAX),
                                  None, 3, 0.0)
    runs.append(report('constant', 'quantiles', x, cls, 13, zq.levels(wd, zq.DEFAULT_BITS), med, times, inner, copy_gbps,
                       {'bits': zq.DEFAULT_BITS, 'table': 'lds'}))
    del x
    torch.cuda.empty_cache()
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--layers', type=int, default=46)
    ap.add_argument('--side', type=int, default=2400)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    ap.add_argument('--limit', type=int, default=240, help='seconds a single GPU step may take')
    ap.add_argument('--dtypes', default='float32,float64')
    a = ap.parse_args()
    LIMIT[0] = a.limit
    res = {'tool': 'zonalqbench', 'build_id': _lib.build_id(), 'layers': a.layers, 'pixels': a.side * a.side, 'q': list(Q),
           'weights': 'per row', 'lds_bytes': _lib.zonal_hist_lds_bytes(), 'default_bits': zq.DEFAULT_BITS, 'dtypes': {}}
    for dtype in a.dtypes.split(','):
        eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250), dtype=dtype)
        with step('%s: the copy kernel' % dtype):
            copy_gbps = float(eng.measure_copy())
        res['device'] = torch.cuda.get_device_name(eng.device)
        res['dtypes'][dtype] = {'copy_kernel_gbps': round(copy_gbps, 1),
                                'runs': bench_dtype(eng, a.layers, a.side, a.repeats, a.window, copy_gbps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
