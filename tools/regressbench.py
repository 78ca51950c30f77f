#!/usr/bin/env python3
"""The per-pixel least squares (RasterEngine.regress, mod16_regress_f32) against the torch passes it
replaces, in one GPU process, resident, float32 stacks with missing values:

  case 1   one 1200 x 1200 tile, T = 1104 (24 years of 8-day periods), Ks = 6 shared columns
           (regress.harmonic_design: intercept, linear trend, two harmonics), 40 % missing, without
           and with series='residuals'
  case 2   four tiles, T = 24, Ks = 1 (intercept), Kp = 3 per-pixel terms, 10 % missing

  (a) regress  one call
  (b) torch    the masked normal equations in float64: the Gram matrices by einsum over the masked
               rows (with a shared design that is a matrix product of the mask with the rows' outer
               products; with per-pixel terms 'tna,tnb->nab' over the masked (T, n, P) predictors),
               torch.linalg.cholesky and cholesky_solve, then the residual pass (fitted values,
               residuals, rss and tss; the residual stack where (a) writes it)

(b) sums in another order than (a), so the two are compared, not equated: the counts must be equal and
the coefficients of the fitted pixels agree to 1e-6 of the largest, checked before anything is timed.
Device events on the current stream; one warm-up of each, then --repeats alternating repeats of windows
of at least --window seconds each; the medians. The engine's copy kernel (measure_copy) runs in the same
process. One JSON line: per run both times, their ratio, ps per pixel-step, the bytes (a) moves as
counted from its loads and stores (two passes over the stacks, the series once, the per-pixel results),
the counted rate and its share of the copy kernel's. No threshold: the torch passes and the copy kernel
are the yardsticks.

  python tools/regressbench.py [--out FILE] [--cases 1,2] [--steps T] [--repeats 5] [--window 0.25]
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
from mod16_amd import regress as rg  # noqa: E402
from mod16_amd.models import COLLECTION61_BPLUT  # noqa: E402
from mod16_amd.raster import RasterEngine  # noqa: E402
from mod16_amd.utils import bplut_table, restore_bplut  # noqa: E402

TILE = 1200 * 1200


def make_inputs(dev, T, n, design, Kp, missing):
    """A (T, n) float32 stack that follows the design (and the terms) plus noise, `missing` of it NaN."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(23)
    values = torch.randn((T, n), dtype=torch.float32, device=dev, generator=gen) * 0.3
    if design is not None:
        truth = torch.randn((design.shape[1], n), dtype=torch.float32, device=dev, generator=gen)
        values += design.float() @ truth
    terms = []
    for k in range(Kp):
        t = torch.randn((T, n), dtype=torch.float32, device=dev, generator=gen)
        values += (0.5 + k) * t
        terms.append(t)
    values[torch.rand((T, n), device=dev, generator=gen) < missing] = float('nan')
    return values, terms


def torch_regress(values, design, terms, series):
    """(b) -> (coef (P, n), rss, tss, count, residuals or None), float64."""
    T, n = values.shape
    mask = torch.isfinite(values)
    for t in terms:
        mask &= torch.isfinite(t)
    m = mask.double()
    y = torch.where(mask, values.double(), 0.0)
    if not terms:                         # shared columns only: the mask times the rows' outer products
        P = design.shape[1]
        outer = (design.unsqueeze(2) * design.unsqueeze(1)).reshape(T, P * P)
        G = (m.t() @ outer).reshape(n, P, P)
        h = y.t() @ design
        X = None
    else:
        cols = ([design[:, a].unsqueeze(1).expand(T, n) for a in range(design.shape[1])] if design is not None else [])
        X = torch.stack(cols + [torch.where(mask, t.double(), 0.0) for t in terms], dim=2)       # (T, n, P)
        Xm = X * m.unsqueeze(2)
        G = torch.einsum('tna,tnb->nab', Xm, X)
        h = torch.einsum('tna,tn->na', Xm, y)
    count = mask.sum(0)
    P = G.shape[1]
    ok = count > P
    eye = torch.eye(P, dtype=torch.float64, device=values.device)
    G = torch.where(ok.view(n, 1, 1), G, eye)                     # (an empty pixel would stop the factorisation)
    L = torch.linalg.cholesky(G)
    b = torch.cholesky_solve(h.unsqueeze(2), L).squeeze(2)        # (n, P)
    f = design @ b.t() if X is None else torch.einsum('tna,na->tn', X, b)
    r = torch.where(mask, values.double() - f, 0.0)
    rss = (r * r).sum(0)
    ybar = y.sum(0) / m.sum(0)
    tss = (m * (y - ybar) ** 2).sum(0)
    nan = float('nan')
    res = torch.where(mask & ok, r, nan).float() if series else None
    return torch.where(ok, b.t(), nan), torch.where(ok, rss, nan), torch.where(ok, tss, nan), count, res


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench(eng, name, values, design, terms, series, repeats, window, copy_gbps):
    T, n = values.shape
    Ks, Kp = (0 if design is None else design.shape[1]), len(terms)
    P = Ks + Kp
    table = rg.output_table((n,), T, P, np.float32, False, rg.SERIES[series])
    out = {k: torch.empty(s, dtype=getattr(torch, dt.name), device=values.device) for k, (s, dt) in table.items()}

    def call_a():
        eng.regress(values, design, terms, series=series, out=out)

    def call_b():
        return torch_regress(values, design, terms, series)
    call_a()
    coef, rss, tss, count, res = call_b()
    eng.check()
    fitted = torch.isfinite(coef).all(0)
    if not torch.equal(out['count'].view(torch.int16).long(), count):
        raise SystemExit('regressbench: %s: the counts differ from the torch passes' % name)
    if not torch.equal(torch.isfinite(out['coef']).all(0), fitted):
        raise SystemExit('regressbench: %s: other pixels are fitted than by the torch passes' % name)
    worst = float((out['coef'][:, fitted] - coef[:, fitted]).abs().max() / coef[:, fitted].abs().max())
    worst_rss = float(((out['rss'][fitted] - rss[fitted]).abs() / tss[fitted]).max())
    if not (worst <= 1e-6 and worst_rss <= 1e-6):
        raise SystemExit('regressbench: %s: coefficients differ from the torch passes by %.3g, rss by %.3g' % (name, worst, worst_rss))
    if series:
        both = torch.isfinite(res)
        if not torch.equal(both, torch.isfinite(out['series'])) or float((out['series'][both] - res[both]).abs().max()) > 1e-3:
            raise SystemExit('regressbench: %s: the residuals differ from the torch passes' % name)
    missing = float(torch.isnan(values).float().mean())
    del coef, rss, tss, count, res
    call_b()                              # (the allocator keeps the passes' temporaries: (b) is timed without allocations)
    inner = {}
    for key, fn in (('a', call_a), ('b', call_b)):
        ms = timed(fn, 1)
        inner[key] = max(1, int(np.ceil(window * 1e3 / ms)))
    times = {'a': [], 'b': []}
    for _ in range(repeats):
        times['a'].append(timed(call_a, inner['a']))
        times['b'].append(timed(call_b, inner['b']))
    a, b = float(np.median(times['a'])), float(np.median(times['b']))
    esz = values.element_size()
    per_step = 2 * esz * (1 + Kp) + (esz if series else 0)          # two passes over the stacks, the series once
    total = per_step * n * T + n * (8 * P + 3 * 8 + 2)
    gbps = total / (a * 1e-3) / 1e9
    return {'case': name, 'pixels': n, 'steps': T, 'ks': Ks, 'kp': Kp, 'series': series, 'missing_fraction': round(missing, 4),
            'regress_ms': round(a, 4), 'torch_ms': round(b, 4), 'regress_over_torch': round(a / b, 5),
            'ps_per_pixel_step': round(a * 1e9 / (n * T), 3), 'bytes_per_pixel_step_counted': per_step,
            'bytes_counted': total, 'regress_gbps_counted': round(gbps, 1), 'fraction_of_copy_rate': round(gbps / copy_gbps, 4),
            'fitted_fraction': round(float(fitted.float().mean()), 4), 'coef_vs_torch': worst, 'rss_vs_torch': worst_rss,
            'regress_ms_all': [round(x, 4) for x in times['a']], 'torch_ms_all': [round(x, 4) for x in times['b']],
            'launches_per_window': inner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--cases', default='1,2')
    ap.add_argument('--steps', type=int, default=1104, help='T of case 1')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window, at least')
    a = ap.parse_args()
    eng = RasterEngine(bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250))
    copy_gbps = float(eng.measure_copy())
    dev = eng._dev()
    res = {'tool': 'regressbench', 'build_id': _lib.build_id(), 'device': torch.cuda.get_device_name(eng.device),
           'copy_kernel_gbps': round(copy_gbps, 1), 'runs': []}
    cases = [int(c) for c in a.cases.split(',')]
    if 1 in cases:
        T = a.steps
        design = torch.from_numpy(rg.harmonic_design(np.arange(T) * 8.0, 368.0, harmonics=2, trend=1)).to(dev)
        values, _ = make_inputs(dev, T, TILE, design, 0, 0.4)
        for series in (None, 'residuals'):
            res['runs'].append(bench(eng, 'harmonic, one tile', values, design, [], series, a.repeats, a.window, copy_gbps))
            torch.cuda.empty_cache()
        del values
        torch.cuda.empty_cache()
    if 2 in cases:
        T = 24
        design = torch.ones((T, 1), dtype=torch.float64, device=dev)
        values, terms = make_inputs(dev, T, 4 * TILE, design, 3, 0.1)
        res['runs'].append(bench(eng, 'attribution, four tiles', values, design, terms, None, a.repeats, a.window, copy_gbps))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
