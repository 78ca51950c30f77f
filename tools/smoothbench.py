#!/usr/bin/env python3
"""The Whittaker smoother (RasterEngine.smooth, mod16_smooth_u8) against the torch passes it replaces,
in one GPU process, resident: S = 46 and S = 138 slabs (one and three years of 8-day periods) of uint8
codes and their QC layer on 4 x 1200 x 1200 pixels, order 2, lam 1600, the default QC table. Codes are
uniform in 0..100 with 5 % fill codes; of the twelve QC bytes drawn the four acceptable ones come up
with probability 0.15 each, so 57 % of the slabs are weighted.

  (a) smooth   one call, with envelope 0 and 2, float32 output (scale 0.01) and uint8 output
  (b) torch    the definition of mod16_amd/smooth.py transcribed to torch on the device: an S-loop of
               elementwise float64 passes over (n,) tensors -- the factorisation, the forward and the
               backward substitution, the lift of y and the substitutions again per envelope round

(a) and (b) must be equal -- uint8 value for value, float32 bit for bit with the same NaN mask --
checked before anything is timed. Device events on the current stream; one warm-up of each, then
--repeats alternating repeats of windows of at least --window seconds each; the medians. The
engine's copy kernel (measure_copy) runs in the same process. One JSON line: per run the bytes counted
per pixel-slab (code and QC byte read, the output written; the workspace traffic of the columns is
stated apart, as the doubles a pixel-slab moves), both times, the counted rate of (a), that rate as a
share of the copy kernel's, ps per pixel-slab and the ratio to (b). No threshold: the torch passes and
the copy kernel are the yardsticks.

  python tools/smoothbench.py [--out FILE] [--slabs 46,138] [--pixels N] [--repeats 5] [--window 0.25]
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
from mod16_amd import smooth as sm  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

LAM, ORDER, MIN_VALID, SCALE = 1600.0, 2, 3, 0.01
# twelve QC bytes; the four acceptable ones three times each: 12 of 20 draws
QC_DRAW = (0, 2, 24, 32) * 3 + (8, 16, 64, 96, 128, 1, 4, 157)


def make_inputs(dev, S, n):
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    v = torch.randint(0, 101, (S, n), dtype=torch.uint8, device=dev, generator=gen)
    v[torch.rand((S, n), device=dev, generator=gen) < 0.05] = 255
    draw = torch.tensor(QC_DRAW, dtype=torch.uint8, device=dev)
    qc = draw[torch.randint(0, len(QC_DRAW), (S, n), device=dev, generator=gen)]
    return v, qc


def torch_smooth(values, qc, table, envelope, dtype):
    """(b): weights_of, factor, solve, the envelope and encode of mod16_amd/smooth.py, slab by slab."""
    S, n = values.shape
    dev = values.device
    # lam * a, float64 products as the definition forms them; 0-dim tensors (a Python float over a tensor
    # would be a reciprocal and a multiplication: another rounding)
    a0, a1, a2 = (torch.from_numpy(LAM * b).to(dev) for b in sm.penalty_bands(S, ORDER))
    w = table[qc.long()]
    have = (values < 249) & (w > 0)
    w = torch.where(have, w, 0.0)
    y = torch.where(have, values.double(), 0.0)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    d, c, e = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    d1 = d2 = c1 = e1 = e2 = zero
    for i in range(S):
        di = ((w[i] + a0[i]) - (c1 * c1) * d1) - (e2 * e2) * d2
        ci = (a1[i] - (d1 * c1) * e1) / di
        ei = a2[i] / di
        d[i], c[i], e[i] = di, ci, ei
        d2, d1, c1, e2, e1 = d1, di, ci, e1, ei
    g, z = torch.empty_like(w), torch.empty_like(w)
    for rnd in range(envelope + 1):
        f1 = f2 = c1 = e1 = e2 = zero
        for i in range(S):
            fi = (w[i] * y[i] - c1 * f1) - e2 * f2
            g[i] = fi / d[i]
            f2, f1, c1, e2, e1 = f1, fi, c[i], e1, e[i]
        z1 = z2 = zero
        for i in range(S - 1, -1, -1):
            zi = (g[i] - c[i] * z1) - e[i] * z2
            z[i] = zi
            z2, z1 = z1, zi
        if rnd < envelope:
            y = torch.where((w > 0) & (z > y), z, y)
    unsmoothed = ((w > 0).sum(0) < MIN_VALID).unsqueeze(0)
    if dtype == 'uint8':
        return torch.where(unsmoothed, 255.0, torch.floor(z + 0.5).clamp(0.0, 248.0)).to(torch.uint8)
    return torch.where(unsmoothed, float('nan'), z * SCALE).float()


def equal(a, b):
    if a.dtype == torch.uint8:
        return bool(torch.equal(a, b))
    nan = torch.isnan(a)
    return bool(torch.equal(nan, torch.isnan(b))) and bool(torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan]))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def workspace_doubles(envelope):
    """float64 values a pixel-slab moves to and from the workspace of columns: the first pass stores c, e, g
    (and y, d); a backward pass loads c, e, g and stores z unless it is the last; an envelope pass loads z,
    y, d, c, e and stores g (and y where it is lifted: counted)."""
    return (5 if envelope else 3) + (envelope + 1) * 3 + envelope + envelope * 7


def bench(eng, values, qc, table, envelope, dtype, repeats, window, copy_gbps):
    S, n = values.shape
    out = torch.empty((S, n), dtype=torch.uint8 if dtype == 'uint8' else torch.float32, device=values.device)
    scale = None if dtype == 'uint8' else SCALE

    def call_a():
        eng.smooth(values, qc=qc, lam=LAM, order=ORDER, envelope=envelope, min_valid=MIN_VALID, dtype=dtype, scale=scale, out=out)

    def call_b():
        return torch_smooth(values, qc, table, envelope, dtype)
    call_a()
    want = call_b()
    eng.check()
    if not equal(out, want):
        raise SystemExit('smoothbench: the %s output with envelope %d differs from the torch passes' % (dtype, envelope))
    del want
    torch.cuda.empty_cache()
    inner = {}
    for name, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)
        inner[name] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    a, b = float(np.median(times['a'])), float(np.median(times['b']))
    counted = 2 + out.element_size()
    gbps = counted * n * S / (a * 1e-3) / 1e9
    weighted = float(((values < 249) & (table[qc.long()] > 0)).float().mean())
    return {'slabs': S, 'envelope': envelope, 'out': dtype, 'smooth_ms': round(a, 4), 'torch_ms': round(b, 4),
            'smooth_over_torch': round(a / b, 5), 'bytes_per_pixel_slab_counted': counted,
            'workspace_bytes_per_pixel_slab': 8 * workspace_doubles(envelope), 'smooth_gbps_counted': round(gbps, 1),
            'fraction_of_copy_rate': round(gbps / copy_gbps, 4), 'ps_per_pixel_slab': round(a * 1e9 / (n * S), 3),
            'weighted_fraction': round(weighted, 4), 'smooth_ms_all': [round(x, 4) for x in times['a']],
            'torch_ms_all': [round(x, 4) for x in times['b']], 'launches_per_window': inner, 'equal_to_torch': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--slabs', default='46,138')
    ap.add_argument('--pixels', type=int, default=4 * 1200 * 1200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    dev = eng._dev()
    table = torch.from_numpy(sm.default_qc_weight()).to(dev)
    res = {'tool': 'smoothbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'pixels': a.pixels, 'lam': LAM, 'order': ORDER, 'copy_kernel_gbps': round(copy_gbps, 1), 'runs': []}
    for S in (int(s) for s in a.slabs.split(',')):
        values, qc = make_inputs(dev, S, a.pixels)
        for envelope in (0, 2):
            for dtype in ('float32', 'uint8'):
                res['runs'].append(bench(eng, values, qc, table, envelope, dtype, a.repeats, a.window, copy_gbps))
                torch.cuda.empty_cache()
        del values, qc
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
