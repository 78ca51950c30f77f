#!/usr/bin/env python3
"""The temporal gap filling (RasterEngine.gapfill, mod16_gapfill_u8) against the torch passes it
replaces, in one GPU process, resident: S = 46 slabs (a year of 8-day periods) of two fields (fPAR and
LAI codes) and their shared QC layer on 4 x 1200 x 1200 pixels, no limit on the gap, no fallback.
Codes are uniform in 0..100 with 5 % fill codes; of the twelve QC bytes drawn the four acceptable ones
come up with probability 0.15 each, so 57 % of the slabs are reliable.

  (a) gapfill  one call, with uint8 output and with float64 output (scale 0.01 / 0.1)
  (b) torch    what a user wrote before, with calls that predate the kernel: the table looked up per
               QC byte, cummax / flipped cummin of the slab indices, two gathers, the masks, the
               integer interpolation and its rounding (or the float64 division), per field

(a) and (b) must be equal -- uint8 value for value, float64 bit for bit with the same NaN mask --
checked before anything is timed. Device events on the current stream; one warm-up of each, then
--repeats alternating repeats of windows of at least --window seconds each; the medians. The
engine's copy kernel (measure_copy) runs in the same process. One JSON line: per output type the
bytes counted per pixel-slab (2 fields + QC read, 2 outputs written), both times, the counted rate of
(a), that rate as a share of the copy kernel's, and the ratio to (b). No threshold: the torch passes
and the copy kernel are the yardsticks.

  python tools/gapfillbench.py [--out FILE] [--slabs 46] [--pixels N] [--repeats 5] [--window 0.25]
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
from mod16_amd import gapfill as gf  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

SCALES = (0.01, 0.1)
# twelve QC bytes; the four acceptable ones three times each: 12 of 20 draws
QC_DRAW = (0, 2, 24, 32) * 3 + (8, 16, 64, 96, 128, 1, 4, 157)


def make_inputs(dev, S, n):
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    fields = []
    for _ in range(2):
        v = torch.randint(0, 101, (S, n), dtype=torch.uint8, device=dev, generator=gen)
        fill = torch.rand((S, n), device=dev, generator=gen) < 0.05
        v[fill] = 255
        fields.append(v)
    draw = torch.tensor(QC_DRAW, dtype=torch.uint8, device=dev)
    qc = draw[torch.randint(0, len(QC_DRAW), (S, n), device=dev, generator=gen)]
    return fields, qc


def torch_fill(fields, qc, good, dtype):
    """(b): the definition of mod16_amd/gapfill.py (no limit, no fallback) in torch passes."""
    S = qc.shape[0]
    ok = good[qc.long()]
    t = torch.arange(S, dtype=torch.int32, device=qc.device).unsqueeze(1)
    outs = []
    for v, scale in zip(fields, SCALES):
        rel = (v < gf.FILL) & ok
        i = torch.where(rel, t, -1).cummax(0).values
        j = torch.where(rel, t, S).flip(0).cummin(0).values.flip(0)
        left, right = i >= 0, j < S
        vi = v.to(torch.int32)
        a = torch.gather(vi, 0, i.clamp(min=0).long())
        b = torch.gather(vi, 0, j.clamp(max=S - 1).long())
        both = left & right & ~rel
        num = torch.where(rel, vi, torch.where(both, a * (j - t) + b * (t - i), torch.where(left, a, b)))
        den = torch.where(both, j - i, 1)
        missing = ~left & ~right
        if dtype == 'uint8':
            outs.append(torch.where(missing, 255, (2 * num + den) // (2 * den)).to(torch.uint8))
        else:
            outs.append(torch.where(missing, float('nan'), (num.double() / den.double()) * scale))
    return outs


def equal(a, b):
    if a.dtype == torch.uint8:
        return bool(torch.equal(a, b))
    nan = torch.isnan(a)
    return bool(torch.equal(nan, torch.isnan(b))) and bool(torch.equal(a.view(torch.int64)[~nan], b.view(torch.int64)[~nan]))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench(eng, fields, qc, good, dtype, repeats, window, copy_gbps):
    S, n = qc.shape
    tdtype = torch.uint8 if dtype == 'uint8' else torch.float64
    out = tuple(torch.empty((S, n), dtype=tdtype, device=qc.device) for _ in fields)
    scale = None if dtype == 'uint8' else SCALES

    def call_a():
        eng.gapfill(tuple(fields), qc=qc, dtype=dtype, scale=scale, out=out)

    def call_b():
        return torch_fill(fields, qc, good, dtype)
    call_a()
    want = call_b()
    eng.check()
    for f, (g, w) in enumerate(zip(out, want)):
        if not equal(g, w):
            raise SystemExit('gapfillbench: field %d of the %s fill differs from the torch passes' % (f, dtype))
    del want
    inner = {}
    for name, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)
        inner[name] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    a, b = float(np.median(times['a'])), float(np.median(times['b']))
    counted = len(fields) + 1 + len(fields) * out[0].element_size()
    gbps = counted * n * S / (a * 1e-3) / 1e9
    reliable = float(((fields[0] < gf.FILL) & good[qc.long()]).float().mean())
    return {'out': dtype, 'gapfill_ms': round(a, 4), 'torch_ms': round(b, 4), 'gapfill_over_torch': round(a / b, 4),
            'bytes_per_pixel_slab_counted': counted, 'gapfill_gbps_counted': round(gbps, 1),
            'fraction_of_copy_rate': round(gbps / copy_gbps, 4), 'ps_per_pixel_slab': round(a * 1e9 / (n * S), 3),
            'reliable_fraction': round(reliable, 4), 'gapfill_ms_all': [round(x, 4) for x in times['a']],
            'torch_ms_all': [round(x, 4) for x in times['b']], 'launches_per_window': inner, 'equal_to_torch': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--slabs', type=int, default=46)
    ap.add_argument('--pixels', type=int, default=4 * 1200 * 1200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    dev = eng._dev()
    fields, qc = make_inputs(dev, a.slabs, a.pixels)
    good = torch.from_numpy(gf.default_good()).to(dev)
    res = {'tool': 'gapfillbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'slabs': a.slabs, 'pixels': a.pixels, 'fields': 2, 'copy_kernel_gbps': round(copy_gbps, 1), 'runs': []}
    for dtype in ('uint8', 'float64'):
        res['runs'].append(bench(eng, fields, qc, good, dtype, a.repeats, a.window, copy_gbps))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
