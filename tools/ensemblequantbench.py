#!/usr/bin/env python3
"""The per-pixel quantiles of the ensemble run (EnsembleRun.quantiles, mod16_et_ensemble_quantiles_*)
against the member loop they replace, in one GPU process, on 4 x 1200 x 1200 float64 pixels of the
engine's generator with D = 8 and D = 64 tables (the Collection 6.1 table perturbed by up to 10 % per
entry, tests/test_gpu_ensemble.py's) and q = (0.05, 0.5, 0.95):

  (a) quantiles  one call: 3 x 3 rasters (day, night, total at each q), the member values through a slab
  (b) loop       what a user wrote before, on the same engine: per member ctx.set_bplut(table) and
                 run() into (D, n) tensors, torch.sort(dim=0) of the three series, the interpolation
                 of mod16_amd.calibration.ensemble_quantile in torch
  (c) moments    ens.run(...) for the same D: what the selection costs over the mean and the spread

Device events on the current stream; one warm-up of each, then five alternating repeats of windows of
at least --window seconds each; the medians. (a) and (b) must have identical NaN masks and agree to
4 x 2^-52 x max_m |x_m| (for the total max_m (|day_m| + |night_m|)) -- checked before anything is
timed. One JSON line: the three times, (a)/(b), (a)/(c), ns per pixel-member of (a). Exits non-zero
if (a) is not faster than (b).

  python tools/ensemblequantbench.py [--out FILE] [--members 8 64] [--pixels N] [--repeats 5] [--window 0.25]
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
from mod16_amd.calibration import quantile_positions  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

Q = (0.05, 0.5, 0.95)


def member_loop(eng, tables, cls, drv, buf, scales=False):
    """(b): three (Q, n) tensors as the quantile call returns them (and the scales of the comparison)."""
    D = len(tables)
    day, night = buf
    for m, t in enumerate(tables):
        eng.ctx.set_bplut(t)
        eng.run(cls, drv, day[m], night[m])
    lo, frac = quantile_positions(Q, D)
    out = []
    for x in (day, night, day + night):
        nan = torch.isnan(x).any(dim=0)
        s = torch.sort(x, dim=0).values
        res = torch.empty((len(Q), x.shape[1]), dtype=x.dtype, device=x.device)
        for k in range(len(Q)):
            a, b = s[int(lo[k])], s[min(int(lo[k]) + 1, D - 1)]
            v = a if frac[k] == 0 else torch.where(a == b, a, a + float(frac[k]) * (b - a))
            res[k] = torch.where(nan, torch.full_like(v, float('nan')), v)
        out.append(res)
    if not scales:
        return out
    sd, sn = day.abs().amax(dim=0), night.abs().amax(dim=0)
    return out, (sd, sn, (day.abs() + night.abs()).amax(dim=0))


def agree(a, b, scales):
    """max |a - b| / scale per series; raises unless NaN masks are equal and every value within 4 ulp of the scale."""
    worst = []
    for x, y, s in zip(a, b, scales):
        if not torch.equal(torch.isnan(x), torch.isnan(y)):
            raise SystemExit('ensemblequantbench: NaN masks of the quantile call and the member loop differ')
        ok = ~torch.isnan(x)
        err = torch.where(ok, (x - y).abs(), torch.zeros_like(x))
        if not bool((err <= 4 * 2.0 ** -52 * s).all()):
            raise SystemExit('ensemblequantbench: the quantile call and the member loop differ by more than 4 x 2^-52 x scale')
        rel = torch.where(s > 0, err / s, torch.zeros_like(err))
        worst.append(float(rel.max()))
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
    out = tuple(torch.empty((len(Q), n), dtype=eng.dtype, device=cls.device) for _ in range(3))
    mom = eng.empty(n, 5)
    buf = tuple(torch.empty((D, n), dtype=eng.dtype, device=cls.device) for _ in range(2))

    def call_a():
        ens.quantiles(cls, drv, Q, out=out)

    def call_b():
        return member_loop(eng, tables, cls, drv, buf)

    def call_c():
        ens.run(cls, drv, out=mom)
    call_a()
    call_c()
    got_b, scales = member_loop(eng, tables, cls, drv, buf, scales=True)
    eng.check()
    worst = agree(out, got_b, scales)
    del got_b, scales
    calls = (('a', call_a), ('b', call_b), ('c', call_c))
    inner = {}
    for name, fn in calls:
        ms = timed(fn, 1)                      # (the warm-up above loaded the code objects)
        inner[name] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {name: [] for name, _ in calls}
    for _ in range(repeats):
        for name, fn in calls:
            times[name].append(timed(fn, inner[name]))
    eng.check()
    eng.ctx.set_bplut(base)
    ens.close()
    a, b, c = (float(np.median(times[k])) for k in 'abc')
    return {'members': D, 'pixels': n, 'q': list(Q), 'quantiles_ms': round(a, 4), 'loop_ms': round(b, 4),
            'moments_ms': round(c, 4), 'quantiles_over_loop': round(a / b, 4),
            'quantiles_over_moments': round(a / c, 4), 'ns_per_pixel_member': round(a * 1e6 / (n * D), 5),
            'quantiles_ms_all': [round(t, 4) for t in times['a']], 'loop_ms_all': [round(t, 4) for t in times['b']],
            'moments_ms_all': [round(t, 4) for t in times['c']],
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
    res = {'tool': 'ensemblequantbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'dtype': 'float64', 'runs': [bench(eng, base, cls, drv, D, a.repeats, a.window) for D in a.members]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if any(r['quantiles_over_loop'] >= 1 for r in res['runs']):
        raise SystemExit('ensemblequantbench: the quantile call is not faster than the member loop it replaces')


if __name__ == '__main__':
    main()
