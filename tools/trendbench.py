#!/usr/bin/env python3
"""The per-pixel trend (RasterEngine.trend, mod16_trend_f32) against the torch passes it replaces, in one
GPU process, resident: four MODIS tiles -- 4 x 1200 x 1200 = 5.76 M pixels -- of Y = 24 and Y = 46 float32
annual totals, about 10 % of them NaN, default times, min_valid 4, alpha = 0.05.

  (a) trend  one call: slope, intercept, the slope's interval, S, z and the valid count
  (b) torch  what a user wrote before, for S and the slope alone: the (Y (Y - 1) / 2, n) tensor of pairwise
             differences, its sign sum, the slopes, torch.sort along the pair axis (NaN sorts last) and a
             gather of the one or two middle ranks of every pixel's own number of valid pairs -- in
             chunks of --chunk pixels, since the whole tensor (12.7 GB at Y = 24, 47.7 GB at Y = 46, and
             the sort's indices twice that) is the reason the step left the package

(a) and (b) must agree before anything is timed: S exactly, the slope bit for bit (NaN at the same
pixels). Device events on the current stream; one warm-up of each, then --repeats alternating repeats:
windows of at least --window seconds of (a), one pass of (b); the medians. The engine's copy kernel
(measure_copy) runs in the same process. One JSON line: per Y the two times, their ratio, picoseconds
per pixel-pair, and the bytes counted per pixel (Y float32 read; five float64, an int32 and a byte
written) as a rate and as a share of the copy kernel's. No threshold: the torch passes and the copy
kernel are the yardsticks.

  python tools/trendbench.py [--out FILE] [--pixels 5760000] [--steps 24,46] [--chunk 262144] [--repeats 3] [--window 0.25]
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
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

MIN_VALID = 4


def make_stack(dev, Y, n):
    gen = torch.Generator(device=dev)
    gen.manual_seed(24 + Y)
    x = torch.randn((Y, n), device=dev, generator=gen, dtype=torch.float32) * 60.0 + 500.0
    x += 2.0 * torch.arange(Y, device=dev, dtype=torch.float32)[:, None]
    x[torch.rand((Y, n), device=dev, generator=gen) < 0.1] = float('nan')
    return x


def torch_passes(x, chunk):
    """(b): S and the Theil-Sen slope of mod16_amd/trend.py in torch passes, `chunk` pixels at a time."""
    Y, n = x.shape
    a, b = torch.triu_indices(Y, Y, 1, device=x.device)
    dt = (b - a).double()[:, None]
    s = torch.empty(n, dtype=torch.int32, device=x.device)
    slope = torch.empty(n, dtype=torch.float64, device=x.device)
    for lo in range(0, n, chunk):
        xc = x[:, lo:lo + chunk].double()
        d = xc[b] - xc[a]                                            # (M, chunk); NaN where a value is missing
        m = torch.isfinite(xc).sum(0)
        s[lo:lo + chunk] = torch.where(m >= MIN_VALID, torch.nan_to_num(torch.sign(d)).sum(0), 0.0).to(torch.int32)
        q = torch.sort(d / dt + 0.0, dim=0).values                   # NaN last
        M = m * (m - 1) // 2
        mid = torch.stack(((M - 1).clamp_(min=0) // 2, M // 2))
        two = torch.gather(q, 0, mid.clamp_(max=q.shape[0] - 1))
        med = torch.where(M % 2 == 1, two[0], (two[0] + two[1]) * 0.5)
        slope[lo:lo + chunk] = torch.where(m >= MIN_VALID, med, float('nan'))
    return s, slope


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(eng, Y, n, chunk, repeats, window, copy_gbps):
    dev = eng._dev()
    x = make_stack(dev, Y, n)
    names = ('slope', 'intercept', 'slope_lo', 'slope_hi', 's', 'z', 'count')
    kinds = {'s': torch.int32, 'count': torch.uint8}
    out = {k: torch.empty((n,), dtype=kinds.get(k, torch.float64), device=dev) for k in names}

    def call_a():
        eng.trend(x, min_valid=MIN_VALID, alpha=0.05, out=out)

    def call_b():
        return torch_passes(x, chunk)
    call_a()
    s, slope = call_b()
    eng.check()
    if not torch.equal(s, out['s']):
        raise SystemExit('trendbench: S differs from the torch passes at Y = %d' % Y)
    both_nan = torch.isnan(slope) & torch.isnan(out['slope'])
    if not bool((both_nan | (slope.view(torch.int64) == out['slope'].view(torch.int64))).all()):
        raise SystemExit('trendbench: the slope differs from the torch passes at Y = %d' % Y)
    valid_share = float(torch.isfinite(x).double().mean())
    del s, slope, both_nan
    torch.cuda.empty_cache()
    inner = max(1, int(np.ceil(window * 1e3 / timed(call_a, 1))))
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(call_a, inner))
        tb.append(timed(call_b, 1))
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    pairs = Y * (Y - 1) // 2
    counted = Y * 4 + 5 * 8 + 4 + 1
    gbps = counted * n / (a_ms * 1e-3) / 1e9
    return {'steps': Y, 'pairs': pairs, 'valid_share': round(valid_share, 4), 'trend_ms': round(a_ms, 4),
            'torch_ms': round(b_ms, 3), 'trend_over_torch': round(a_ms / b_ms, 5),
            'ps_per_pixel_pair': round(a_ms * 1e9 / (n * pairs), 3), 'bytes_per_pixel_counted': counted,
            'trend_gbps_counted': round(gbps, 2), 'fraction_of_copy_rate': round(gbps / copy_gbps, 5),
            'pair_tensor_gb': round(pairs * n * 8 / 1e9, 2), 'trend_ms_all': [round(v, 4) for v in ta],
            'torch_ms_all': [round(v, 3) for v in tb], 'launches_per_window': inner, 'agrees_with_torch': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--pixels', type=int, default=4 * 1200 * 1200)
    ap.add_argument('--steps', default='24,46')
    ap.add_argument('--chunk', type=int, default=1 << 18, help='pixels per chunk of the torch passes')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window of the call, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    res = {'tool': 'trendbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'pixels': a.pixels, 'in': 'float32', 'alpha': 0.05, 'min_valid': MIN_VALID, 'torch_chunk': a.chunk,
           'copy_kernel_gbps': round(copy_gbps, 1),
           'runs': [measure(eng, int(Y), a.pixels, a.chunk, a.repeats, a.window, copy_gbps) for Y in a.steps.split(',')]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
