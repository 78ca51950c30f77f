#!/usr/bin/env python3
"""The per-pixel anomaly (RasterEngine.anomaly, mod16_anomaly_f32) against the torch passes it replaces,
in one GPU process, resident: one MODIS tile -- 1200 x 1200 = 1.44 M pixels -- of Y = 24 years x P = 46
8-day ET and PET totals (two float32 stacks of 1104 slabs, 6.4 GB each), about 10 % of the ET values NaN,
all years the baseline, min_valid 3.

  shape 1  window = 1, outputs z
  shape 2  window = 4, outputs z and pct

  (a) anomaly  one call
  (b) torch    what a user wrote before, in chunks of --chunk pixels and float64: the window sums by
               unfold, the ratio with PET <= 0 and non-finite values masked, the (Y, P, c) view, the masked
               mean and standard deviation over the year axis (two passes), the z-score; for shape 2
               also the (Y, Y, P, c) comparison tensors, summed over the baseline years, for the mid-rank
               percentile (in chunks of --chunk / 4 pixels)

(a) and (b) must agree before anything is timed: NaN at the same places, z to 1e-4 relative (float32
outputs; the torch reductions sum in another order), pct to 1e-6. Device events on the current stream;
one warm-up of each, then --repeats alternating repeats: windows of at least --window seconds of (a),
one pass of (b); the medians. The engine's copy kernel (measure_copy) runs in the same process. One
JSON line: per shape the two times, their ratio, picoseconds per pixel-slab, and the bytes counted per
pixel-slab (two float32 read, one float32 written per output; the window's re-reads of the W - 1
earlier slabs and the climatology, which is not requested, are not counted) as a rate and as a share of
the copy kernel's. No threshold: the torch passes and the copy kernel are the yardsticks.

  python tools/anomalybench.py [--out FILE] [--pixels 1440000] [--years 24] [--periods 46] [--chunk 131072] [--repeats 5] [--window 0.25]
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

MIN_VALID = 3
SHAPES = ((1, ('z',)), (4, ('z', 'pct')))


def make_stacks(dev, S, n):
    """ET and PET totals of S slabs: gamma-like positive values, PET above ET, 10 % of ET missing; made
    slab by slab so that no temporary of the stacks' size exists."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(2446)
    et = torch.empty((S, n), device=dev, dtype=torch.float32)
    pet = torch.empty((S, n), device=dev, dtype=torch.float32)
    for s in range(S):
        a = torch.rand((n,), device=dev, generator=gen) * 30.0 + 5.0
        pet[s] = a + torch.rand((n,), device=dev, generator=gen) * 40.0 + 1.0
        a[torch.rand((n,), device=dev, generator=gen) < 0.1] = float('nan')
        et[s] = a
    return et, pet


def torch_passes(et, pet, Y, P, W, want_pct, chunk, z, pct):
    """(b): the definition of mod16_amd/anomaly.py in torch passes, `chunk` pixels at a time, into z (and pct)."""
    S, n = et.shape
    nan = float('nan')
    for lo in range(0, n, chunk):
        a, b = et[:, lo:lo + chunk].double(), pet[:, lo:lo + chunk].double()
        if W > 1:
            head = torch.full((W - 1, a.shape[1]), nan, dtype=torch.float64, device=a.device)
            a = torch.cat((head, a.unfold(0, W, 1).sum(-1)))
            b = torch.cat((head, b.unfold(0, W, 1).sum(-1)))
        r = a / b
        ok = torch.isfinite(r) & (b > 0) & torch.isfinite(b)
        r = torch.where(ok, r, nan).view(Y, P, -1)
        ok = ok.view(Y, P, -1)
        m = ok.sum(0)
        mean = torch.nansum(r, 0) / m
        e = torch.where(ok, r - mean, 0.0)
        std = torch.sqrt((e * e).sum(0) / (m - 1))
        good = ok & (m >= MIN_VALID)
        zz = torch.where(good & torch.isfinite(std) & (std > 0), (r - mean) / std, nan)
        z[:, lo:lo + chunk] = zz.view(S, -1).float()
        if want_pct:
            small = max(1, chunk // 4)
            for l2 in range(0, r.shape[2], small):
                rc = r[:, :, l2:l2 + small]
                lt = (rc[None] < rc[:, None]).sum(1)               # (target year, baseline year, P, c)
                eq = (rc[None] == rc[:, None]).sum(1)
                pp = (lt.double() + 0.5 * eq.double()) / m[:, l2:l2 + small]
                pp = torch.where(good[:, :, l2:l2 + small], pp, nan)
                pct[:, lo + l2:lo + l2 + rc.shape[2]] = pp.view(S, -1).float()


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def agree(a, b, rtol, what):
    if not bool((torch.isnan(a) == torch.isnan(b)).all()):
        raise SystemExit('anomalybench: %s is NaN at other places than the torch passes' % what)
    fin = ~torch.isnan(a)
    err = ((a[fin] - b[fin]).abs() / b[fin].abs().clamp(min=1.0)).max()
    if not float(err) <= rtol:
        raise SystemExit('anomalybench: %s differs from the torch passes by %g' % (what, float(err)))
    return float(err)


def measure(eng, et, pet, Y, P, W, names, chunk, repeats, window, copy_gbps):
    S, n = et.shape
    out = {k: torch.empty((S, n), dtype=torch.float32, device=et.device) for k in names}
    ref = {k: torch.empty((S, n), dtype=torch.float32, device=et.device) for k in names}
    want_pct = 'pct' in names

    def call_a():
        eng.anomaly(et, pet, periods=P, window=W, min_valid=MIN_VALID, outputs=names, out=out)

    def call_b():
        torch_passes(et, pet, Y, P, W, want_pct, chunk, ref['z'], ref.get('pct'))
    call_a()
    call_b()
    eng.check()
    errs = {'z': agree(out['z'], ref['z'], 1e-4, 'z')}
    if want_pct:
        errs['pct'] = agree(out['pct'], ref['pct'], 1e-6, 'pct')
    finite_share = float(torch.isfinite(out['z']).float().mean())
    torch.cuda.empty_cache()
    inner = max(1, int(np.ceil(window * 1e3 / timed(call_a, 1))))
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(call_a, inner))
        tb.append(timed(call_b, 1))
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    counted = 2 * 4 + 4 * len(names)
    gbps = counted * S * n / (a_ms * 1e-3) / 1e9
    return {'window': W, 'outputs': list(names), 'z_finite_share': round(finite_share, 4), 'anomaly_ms': round(a_ms, 4),
            'torch_ms': round(b_ms, 3), 'anomaly_over_torch': round(a_ms / b_ms, 5),
            'ps_per_pixel_slab': round(a_ms * 1e9 / (S * n), 3), 'bytes_per_pixel_slab_counted': counted,
            'anomaly_gbps_counted': round(gbps, 1), 'fraction_of_copy_rate': round(gbps / copy_gbps, 4),
            'max_rel_diff_to_torch': {k: float('%.3g' % v) for k, v in errs.items()},
            'anomaly_ms_all': [round(v, 4) for v in ta], 'torch_ms_all': [round(v, 3) for v in tb],
            'launches_per_window': inner, 'agrees_with_torch': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--pixels', type=int, default=1200 * 1200)
    ap.add_argument('--years', type=int, default=24)
    ap.add_argument('--periods', type=int, default=46)
    ap.add_argument('--chunk', type=int, default=1 << 17, help='pixels per chunk of the torch passes')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window of the call, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    Y, P = a.years, a.periods
    et, pet = make_stacks(eng._dev(), Y * P, a.pixels)
    res = {'tool': 'anomalybench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'pixels': a.pixels, 'years': Y, 'periods': P, 'in': 'float32', 'min_valid': MIN_VALID, 'torch_chunk': a.chunk,
           'nan_share_of_et': round(float(torch.isnan(et[:64]).float().mean()), 4), 'copy_kernel_gbps': round(copy_gbps, 1),
           'runs': [measure(eng, et, pet, Y, P, W, names, a.chunk, a.repeats, a.window, copy_gbps) for W, names in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
