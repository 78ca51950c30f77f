#!/usr/bin/env python3
"""The day / night aggregation (RasterEngine.daynight, mod16_daynight_f32) against the torch passes it
replaces, in one GPU process, resident: a month of hourly MERRA-2 -- D = 32 days of H = 24 steps of the
five fields t, qv, ps, sw, lw on the 361 x 576 grid, float32 in (3.2 GB), float64 out, 'solar' mode with
the tables of mod16_amd.daynight.solar_tables.

  (a) daynight  one call: the ten series and temp_annual
  (b) torch     what a user wrote before: the broadcast (D, H, R, W) weight tensor from the same tables,
                per field the weighted sums over the step axis and their quotients with the fallback,
                amin for tmin, the VPD expression on the aggregated planes, the mean over the days

(a) and (b) must agree before anything is timed: torch's sum over the step axis is a tree and its exp
is its own, so the check is 1e-9 relative (plus 1e-9 of the output's largest value), NaN masks equal;
the night values of cells in polar day (24 - day_hours below 1e-6 h) are left out of it.
Device events on the current stream; one warm-up of each, then --repeats alternating repeats of windows
of at least --window seconds each; the medians. The engine's copy kernel (measure_copy) runs in the
same process. One JSON line: the bytes counted per cell-step (five float32 read, ten float64 planes
written per day: 20 + 80 / H) and moved (temp_annual's workspace of float64 daily means is written and
read once: + 16 / H), both times, the counted
rate of (a), that rate as a share of the copy kernel's, and the ratio to (b). No threshold: the torch
passes and the copy kernel are the yardsticks.

  python tools/daynightbench.py [--out FILE] [--days 32] [--steps 24] [--rows 361] [--cols 576] [--repeats 5] [--window 0.25]
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
from mod16_amd import daynight as dn  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402


def make_inputs(dev, D, H, R, W):
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    shape = (D * H, R, W)

    def uniform(lo, hi):
        return torch.rand(shape, device=dev, generator=gen, dtype=torch.float32) * (hi - lo) + lo
    t = uniform(-3.0, 3.0) + (torch.rand((1, R, W), device=dev, generator=gen, dtype=torch.float32) * 50.0 + 255.0)
    return {'t': t, 'qv': uniform(0.001, 0.012), 'ps': uniform(6e4, 1.02e5), 'sw': uniform(-600.0, 900.0).clamp_(min=0.0),
            'lw': uniform(-120.0, -10.0)}


def torch_passes(f, half, noon, offset, H):
    """(b): mod16_amd/daynight.py in torch passes -> the ten series in OUTPUT_NAMES order, temp_annual."""
    D, R = half.shape
    W = offset.shape[0]
    delta = 24.0 / H
    a = (((noon[:, None, None] - half[:, :, None]) - offset[None, None, :]) / delta)[:, None]
    b = (((noon[:, None, None] + half[:, :, None]) - offset[None, None, :]) / delta)[:, None]
    k = torch.arange(H, dtype=torch.float64, device=half.device)[None, :, None, None]
    w = None
    for m in (-float(H), 0.0, float(H)):
        term = (torch.minimum(k + 1.0, b + m) - torch.maximum(k, a + m)).clamp_(min=0.0)
        w = term if w is None else w + term
    w = w.clamp_(max=1.0)                            # (D, H, R, W) float64
    u = 1.0 - w
    sum_w, sum_n = w.sum(1), u.sum(1)
    parts = {}
    for name, x in f.items():
        x = x.double().view(D, H, R, W)
        mean = x.sum(1) / H
        day = torch.where(sum_w > 0, (w * x).sum(1) / sum_w, mean)
        night = torch.where(sum_n > 0, (u * x).sum(1) / sum_n, mean)
        parts[name] = (day, night, mean)
    tmin = f['t'].double().view(D, H, R, W).amin(1)

    def vpd(qv, ps, t):
        tc = t - 273.15
        return 610.7 * torch.exp((17.38 * tc) / (239 + tc)) - (qv * ps) / (0.622 + (0.379 * qv))
    vd = vpd(parts['qv'][0], parts['ps'][0], parts['t'][0])
    vn = vpd(parts['qv'][1], parts['ps'][1], parts['t'][1])
    vn = torch.where(vn < 0, 0.0, vn)
    series = (parts['lw'][0], parts['lw'][1], parts['sw'][0], parts['t'][0], parts['t'][1], tmin, vd, vn,
              delta * sum_w, parts['t'][2])
    return series, parts['t'][2].mean(0)


def agree(got, want):
    scale = float(want[~torch.isnan(want)].abs().max())
    return bool(torch.allclose(got, want, rtol=1e-9, atol=1e-9 * scale, equal_nan=True))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--days', type=int, default=32)
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--rows', type=int, default=361)
    ap.add_argument('--cols', type=int, default=576)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    D, H, R, W = a.days, a.steps, a.rows, a.cols
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    dev = eng._dev()
    f = make_inputs(dev, D, H, R, W)
    lat = np.linspace(-90.0, 90.0, R)
    lon = -180.0 + 360.0 / W * np.arange(W)
    half, noon, offset = dn.solar_tables(np.arange(1, D + 1), lat, lon)
    dtab = tuple(torch.from_numpy(x).to(dev) for x in (half, noon, offset))
    names = dn.OUTPUT_NAMES + ('temp_annual',)
    out = {n: torch.empty((R, W) if n == 'temp_annual' else (D, R, W), dtype=torch.float64, device=dev) for n in names}

    def call_a():
        eng.daynight(f, half, noon, offset, steps_per_day=H, dtype='float64', out=out)

    def call_b():
        return torch_passes(f, dtab[0], dtab[1], dtab[2], H)
    call_a()
    series, annual = call_b()
    eng.check()
    # (polar day: where 24 - day_hours is rounding noise the night value is the quotient of two such
    # sums in both forms -- finite, weighted with ~1e-14 hours downstream, and not comparable)
    some_night = out['day_hours'] < 24.0 - 1e-6
    for n, want in list(zip(dn.OUTPUT_NAMES, series)) + [('temp_annual', annual)]:
        got = out[n]
        if n.endswith('_night'):
            got, want = torch.where(some_night, got, 0.0), torch.where(some_night, want, 0.0)
        if not agree(got, want):
            raise SystemExit('daynightbench: %s differs from the torch passes' % n)
    del series, annual, want, got
    torch.cuda.empty_cache()
    inner = {}
    for name, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)
        inner[name] = max(1, int(np.ceil(a.window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(a.repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    ta, tb = float(np.median(times['a'])), float(np.median(times['b']))
    cell_steps = D * H * R * W
    counted = 5 * 4 + 10 * 8 / H
    moved = counted + 2 * 8 / H
    gbps = counted * cell_steps / (ta * 1e-3) / 1e9
    res = {'tool': 'daynightbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'days': D, 'steps_per_day': H, 'rows': R, 'cols': W, 'in': 'float32', 'out': 'float64', 'mode': 'solar',
           'input_gb': round(5 * 4 * cell_steps / 1e9, 3), 'copy_kernel_gbps': round(copy_gbps, 1),
           'daynight_ms': round(ta, 4), 'torch_ms': round(tb, 4), 'daynight_over_torch': round(ta / tb, 4),
           'bytes_per_cell_step_counted': round(counted, 3), 'bytes_per_cell_step_moved': round(moved, 3),
           'daynight_gbps_counted': round(gbps, 1), 'daynight_gbps_moved': round(moved * cell_steps / (ta * 1e-3) / 1e9, 1),
           'fraction_of_copy_rate': round(gbps / copy_gbps, 4), 'ps_per_cell_step': round(ta * 1e9 / cell_steps, 3),
           'daynight_ms_all': [round(x, 4) for x in times['a']], 'torch_ms_all': [round(x, 4) for x in times['b']],
           'launches_per_window': inner, 'agrees_with_torch': True}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
