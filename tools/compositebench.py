#!/usr/bin/env python3
"""The multi-day composite (RasterEngine.composite, mod16_et_composite_*) against the per-day loop it
replaces, in one GPU process, on 4 x 1200 x 1200 float64 pixels of the engine's generator, resident,
for K = 8, L = 8 (one MOD16A2 period) and K = 46 x 8 = 368, L = 8 (a year of them), with albedo / fPAR /
LAI every 8 days, temp_annual and pressure constant and the other nine drivers and the hours daily:

  (a) composite  one call: (P, n) totals and counts
  (b) loop       what a user wrote before, with calls that predate the composite: run() per day into
                 two buffers, the daily total (day * h * 3600) + (night * (24 - h) * 3600) and a masked
                 accumulation in torch, the period's result at its end

A year of daily drivers for all pixels is 170 GB: where the device has less to spare the year runs on
fewer pixels (the JSON says how many). Device events on the current stream; one warm-up of each, then
--repeats alternating repeats of windows of at least --window seconds each; the medians. (a) and (b)
must agree -- the same NaN masks and counts, values within 1e-12 of the sum of |terms| (they are the
same operations: the line says whether the bits are equal) -- checked before anything is timed. One
JSON line: both times, their ratio, ns and counted bytes per pixel-day of (a), its rate as a fraction
of the copy kernel's. Exits non-zero unless the composite is faster.

  python tools/compositebench.py [--out FILE] [--days 8 368] [--pixels N] [--repeats 5] [--window 0.25]
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
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

L = 8
EVERY = {'sw_albedo': 8, 'fpar': 8, 'lai': 8}
CONSTANT = ('temp_annual', 'pressure')


def slabs_of(name, K):
    return 1 if name in CONSTANT else cp.slab_count(K, EVERY.get(name, 1))


def bytes_per_pixel_day(K):
    """Counted, float64: every slab of every array read once, one total and one count per period, the class byte."""
    P = cp.slab_count(K, L)
    return (8 * sum(slabs_of(name, K) for name in cp.ARRAY_NAMES) + (8 + 2) * P + 1) / K


def make_inputs(eng, n, K):
    """cls, the 14 drivers -- (S, n) tensors, (n,) for the constants -- and the hours, from the generator."""
    dev = eng._dev()
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    drv = []
    for name in cp.ARRAY_NAMES[:14]:
        S = slabs_of(name, K)
        drv.append(torch.empty(n if name in CONSTANT else (S, n), dtype=eng.dtype, device=dev))
    for t in reversed(range(K)):       # (day 0 last: the constants and the 8-day slabs hold their first day's field)
        rows = [d if d.dim() == 1 else d[cp.slab_index(t, EVERY.get(name, 1))] for name, d in zip(cp.ARRAY_NAMES, drv)]
        eng.synth(n, seed=16, step=t, out=(cls, rows))
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    hours = torch.rand((K, n), dtype=eng.dtype, device=dev, generator=gen).mul_(12.0).add_(6.0)
    return cls, drv, hours


def day_loop(eng, cls, drv, hours, K, buf, scales=False):
    """(b): (P, n) totals and counts as the composite returns them; scales (the untimed check pass only):
    also the sums of |terms|."""
    day, night, total, count, scale, out, out_count, out_scale = buf
    zero = torch.zeros((), dtype=total.dtype, device=total.device)
    nan = torch.full((), float('nan'), dtype=total.dtype, device=total.device)
    for t in range(K):
        rows = [d if d.dim() == 1 else d[cp.slab_index(t, EVERY.get(name, 1))] for name, d in zip(cp.ARRAY_NAMES, drv)]
        if t % L == 0:
            total.zero_()
            count.zero_()
            if scales:
                scale.zero_()
        eng.run(cls, rows, day, night)
        h = hours[t]
        v = (day * h * 3600.0) + (night * (24.0 - h) * 3600.0)
        ok = ~torch.isnan(v)
        total += torch.where(ok, v, zero)          # (total is never -0.0: adding +0.0 leaves its bits)
        count += ok
        if scales:
            scale += torch.where(ok, v.abs(), zero)
        if (t + 1) % L == 0 or t + 1 == K:
            p = t // L
            out[p].copy_(torch.where(count < 1, nan, total))
            out_count[p].copy_(count)
            if scales:
                out_scale[p].copy_(scale)
    return out, out_count, out_scale


def agree(a, a_count, b, b_count, scale):
    if not torch.equal(a_count.view(torch.int16).to(torch.int32), b_count):
        raise SystemExit('compositebench: the counts of the composite call and of the per-day loop differ')
    if not torch.equal(torch.isnan(a), torch.isnan(b)):
        raise SystemExit('compositebench: the NaN masks of the composite call and of the per-day loop differ')
    ok = ~torch.isnan(a)
    err = (a[ok] - b[ok]).abs()
    if not bool((err <= 1e-12 * scale[ok]).all()):
        raise SystemExit('compositebench: the composite call and the per-day loop differ by more than 1e-12 x scale')
    return bool(torch.equal(a[ok], b[ok]))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench(eng, pixels, K, repeats, window, copy_gbps):
    P = cp.slab_count(K, L)
    per_pixel = 8 * sum(slabs_of(name, K) for name in cp.ARRAY_NAMES) + 8 * K + 1 + 14 * 8 * P
    free, _ = torch.cuda.mem_get_info(eng.device)
    n = int(min(pixels, (0.6 * free) // per_pixel // 256 * 256))
    cls, drv, hours = make_inputs(eng, n, K)
    dev = eng._dev()
    out = (torch.empty((P, n), dtype=eng.dtype, device=dev), torch.empty((P, n), dtype=torch.uint16, device=dev))
    f64 = lambda *shape: torch.empty(shape, dtype=eng.dtype, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    buf = (f64(n), f64(n), f64(n), i32(n), f64(n), f64(P, n), i32(P, n), f64(P, n))

    def call_a():
        eng.composite(cls, drv, hours, K, L, every=EVERY, out=out)

    def call_b():
        return day_loop(eng, cls, drv, hours, K, buf)
    call_a()
    got_b, count_b, scale = day_loop(eng, cls, drv, hours, K, buf, scales=True)
    eng.check()
    same_bits = agree(out[0], out[1], got_b, count_b, scale)
    inner = {}
    for name, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)                      # (the warm-up above loaded the code objects)
        inner[name] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    eng.check()
    a, b = float(np.median(times['a'])), float(np.median(times['b']))
    bpd = bytes_per_pixel_day(K)
    gbps = bpd * n * K / (a * 1e-3) / 1e9
    return {'days': K, 'period_days': L, 'pixels': n, 'composite_ms': round(a, 4), 'loop_ms': round(b, 4),
            'composite_over_loop': round(a / b, 4), 'ns_per_pixel_day': round(a * 1e6 / (n * K), 5),
            'loop_ns_per_pixel_day': round(b * 1e6 / (n * K), 5), 'bytes_per_pixel_day_counted': round(bpd, 2),
            'composite_gbps_counted': round(gbps, 1), 'fraction_of_copy_rate': round(gbps / copy_gbps, 4),
            'composite_ms_all': [round(t, 4) for t in times['a']], 'loop_ms_all': [round(t, 4) for t in times['b']],
            'launches_per_window': inner, 'same_bits_as_loop': same_bits}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--days', type=int, nargs='+', default=[8, 368])
    ap.add_argument('--pixels', type=int, default=4 * 1200 * 1200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    base = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    eng = RasterEngine(base)
    copy_gbps = float(eng.measure_copy())
    res = {'tool': 'compositebench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'dtype': 'float64', 'copy_kernel_gbps': round(copy_gbps, 1), 'runs': []}
    for K in a.days:
        res['runs'].append(bench(eng, a.pixels, K, a.repeats, a.window, copy_gbps))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if any(r['composite_over_loop'] >= 1 for r in res['runs']):
        raise SystemExit('compositebench: the composite call is not faster than the per-day loop it replaces')


if __name__ == '__main__':
    main()
