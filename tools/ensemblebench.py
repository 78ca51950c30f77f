#!/usr/bin/env python3
"""The ensemble forward run (RasterEngine.ensemble, mod16_et_ensemble_*) against the member loop it
replaces, in one GPU process, on 4 x 1200 x 1200 float64 pixels of the engine's generator with D = 8
and D = 64 tables (the Collection 6.1 table perturbed by up to 10 % per entry, tests/test_gpu_ensemble.py's):

  (a) ensemble   one call: five rasters (mean and spread of day / night, spread of the total)
  (b) loop       what a user wrote before, on the same engine: per member ctx.set_bplut(table),
                 run(), then torch accumulation of x - x_0 and its square for the three quantities;
                 the final formulas at the end

Device events on the current stream; one warm-up of each, then five alternating repeats of windows of
at least --window seconds each; the medians. (a) and (b) must agree to 1e-8 * scale (the bound of
tests/test_gpu_ensemble.py; scale = max_m |x_m|, for the total max_m (|day_m| + |night_m|)), NaN masks
identical -- checked before anything is timed. One JSON line: both times, their ratio, ns per
pixel-member of (a).

  python tools/ensemblebench.py [--out FILE] [--members 8 64] [--pixels N] [--repeats 5] [--window 0.25]
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


def member_loop(eng, tables, cls, drv, buf):
    """(b): five tensors as the ensemble call returns them, and the scales of the comparison."""
    D = len(tables)
    day, night = buf
    for m, t in enumerate(tables):
        eng.ctx.set_bplut(t)
        eng.run(cls, drv, day, night)
        if m == 0:
            d0, n0 = day.clone(), night.clone()
            t0 = d0 + n0
            sums = [torch.zeros_like(day) for _ in range(6)]
            scale_d, scale_n, scale_t = day.abs(), night.abs(), day.abs() + night.abs()
            continue
        for k, x in enumerate((day - d0, night - n0, (day + night) - t0)):
            sums[2 * k] += x
            sums[2 * k + 1] += x * x
        scale_d = torch.maximum(scale_d, day.abs())
        scale_n = torch.maximum(scale_n, night.abs())
        scale_t = torch.maximum(scale_t, day.abs() + night.abs())

    def std(s, s2):
        return torch.sqrt(torch.clamp((s2 - s * s / D) / D, min=0.0))
    out = (d0 + sums[0] / D, n0 + sums[2] / D, std(sums[0], sums[1]), std(sums[2], sums[3]), std(sums[4], sums[5]))
    return out, (scale_d, scale_n, scale_d, scale_n, scale_t)


def agree(a, b, scales):
    """max |a - b| / scale per output; raises unless NaN masks are equal and every value within 1e-8 scale."""
    worst = []
    for x, y, s in zip(a, b, scales):
        if not torch.equal(torch.isnan(x), torch.isnan(y)):
            raise SystemExit('ensemblebench: NaN masks of the ensemble call and the member loop differ')
        ok = torch.isfinite(x) & torch.isfinite(y)
        err = (x[ok] - y[ok]).abs()
        if not bool((err <= 1e-8 * s[ok]).all()):
            raise SystemExit('ensemblebench: the ensemble call and the member loop differ by more than 1e-8 x scale')
        pos = s[ok] > 0
        worst.append(float((err[pos] / s[ok][pos]).max()) if bool(pos.any()) else 0.0)
    return worst


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench(eng, base, cls, drv, D, repeats, window):
    n = cls.numel()
    rng = np.random.default_rng(2024)
    tables = base * (1 + 0.1 * rng.uniform(-1, 1, (D, 13, 11)))
    ens = eng.ensemble(tables)
    out = eng.empty(n, 5)
    buf = eng.empty(n, 2)

    def call_a():
        ens.run(cls, drv, out=out)

    def call_b():
        return member_loop(eng, tables, cls, drv, buf)
    call_a()
    got_b, scales = call_b()
    eng.check()
    worst = agree(out, got_b, scales)
    del got_b, scales
    inner = {}
    for name, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)                      # (the warm-up above loaded the code objects)
        inner[name] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    eng.check()
    eng.ctx.set_bplut(base)
    ens.close()
    a, b = float(np.median(times['a'])), float(np.median(times['b']))
    return {'members': D, 'pixels': n, 'ensemble_ms': round(a, 4), 'loop_ms': round(b, 4),
            'ensemble_over_loop': round(a / b, 4), 'ns_per_pixel_member': round(a * 1e6 / (n * D), 5),
            'loop_ns_per_pixel_member': round(b * 1e6 / (n * D), 5),
            'ensemble_ms_all': [round(t, 4) for t in times['a']], 'loop_ms_all': [round(t, 4) for t in times['b']],
            'launches_per_window': inner, 'max_difference_over_scale': worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--members', type=int, nargs='+', default=[8, 64])
    ap.add_argument('--pixels', type=int, default=4 * 1200 * 1200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    base = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    eng = RasterEngine(base)
    cls, drv = eng.synth(a.pixels, seed=16)
    res = {'tool': 'ensemblebench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'dtype': 'float64', 'runs': [bench(eng, base, cls, drv, D, a.repeats, a.window) for D in a.members]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if any(r['ensemble_over_loop'] >= 1 for r in res['runs']):
        raise SystemExit('ensemblebench: the ensemble call is not faster than the member loop it replaces')


if __name__ == '__main__':
    main()
