#!/usr/bin/env python3
"""Throughput of the GPU DE-MCMC-Z sampler (mod16_amd.calibration), in one GPU process, on
synthetic towers (tools/_drivers.py) of n site-days with `chains` chains (default: n in {2^14, 2^17} x chains in
{3, 64, 1024}, 1000 tuning steps + 5000 draws, 8 free parameters with priors of the shipped families):

  sampler    us per step (GPU time of the captured graphs, HIP events; and wall time of the whole
             sample() call) and chain-draws/s
  objective  problem.gpu_milliseconds() at the same number of draws: the objective-only graph
  ratio      sampler step / objective graph: what propose + accept (and the graph boundaries) add
  host loop  the same sampler restated in numpy (vectorised over chains, numpy's generator for the
             random numbers), driving problem.objective() from the host: us per step over
             `--host-steps` steps

  python tools/mcmcbench.py [--out FILE] [--config N,CHAINS ...] [--tune T] [--draws D]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mod16_amd  # noqa: E402
from mod16_amd import _lib, calibration as cal  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import _drivers  # noqa: E402

P = dict(tmin_close=-8.0, tmin_open=8.0, vpd_open=650.0, vpd_close=4000.0, gl_sh=0.04, gl_wv=0.04,
         g_cuticular=1e-5, csl=0.005, rbl_min=20.0, rbl_max=500.0, beta=250.0)
PRIOR = {'vpd_close': {'lower': 1000.0, 'upper': 8000.0}, 'gl_sh': {'mu': -3.45, 'sigma': 0.71},
         'gl_wv': {'mu': -3.45, 'sigma': 0.71}, 'g_cuticular': {'mu': -10.19, 'sigma': 1.44},
         'csl': {'mu': -5.5, 'sigma': 0.8}, 'rbl_min': {'lower': 10.0, 'upper': 1000.0, 'c': 10.0},
         'rbl_max': {'lower': 100.0, 'upper': 1000.0, 'c': 1000.0},
         'beta': {'lower': 0.0, 'upper': 1000.0}}


def tower(n, seed=3):
    _, drv = _drivers.drivers((n,), seed=seed)
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    rng = np.random.default_rng(seed)
    obs = mod16_amd.MOD16._et(pvec, *drv) + rng.normal(0, 5.0, n)
    return drv, obs


def host_loop_us(problem, chains, steps, seed=0):
    '''us per step of the numpy sampler around problem.objective() (tuning off: the cost per step
    does not depend on it).'''
    names = [k for k in cal.PARAM_NAMES if k in PRIOR]
    idx = [cal.PARAM_NAMES.index(k) for k in names]
    fp = [cal.prior_family(PRIOR[k]) for k in names]
    d = len(names)
    row = np.array([P[k] for k in cal.PARAM_NAMES])
    rng = np.random.default_rng(seed)

    def logp(Y):
        rows = np.repeat(row[None], chains, axis=0)
        lpr = np.zeros(chains)
        for i in range(d):
            rows[:, idx[i]] = cal.x_of_y(fp[i][0], fp[i][1], Y[:, i])
            lpr = lpr + cal.log_prior(fp[i][0], fp[i][1], Y[:, i])
        sse, cnt = problem.objective(rows)
        return lpr - np.sqrt(sse / cnt)

    Y = np.array([[cal.y_of_x(f, p, cal.support_point(f, p)) for f, p in fp]] * chains)
    lp = logp(Y)
    hist = [Y.copy(), Y.copy()]
    lamb, sc = 2.38 / math.sqrt(2 * d), 1e-3
    ar = np.arange(chains)
    t0 = time.perf_counter()
    for t in range(steps):
        m = len(hist)
        i1 = rng.integers(0, m, chains)
        i2 = (i1 + rng.integers(1, m, chains)) % m
        H = np.stack(hist)
        Yp = (Y + lamb * (H[i1, ar] - H[i2, ar])) + (2.0 * rng.random((chains, d)) - 1.0) * sc
        lpn = logp(Yp)
        mr = lpn - lp
        acc = np.isfinite(mr) & (np.log(rng.random(chains)) < mr)
        Y[acc], lp[acc] = Yp[acc], lpn[acc]
        hist.append(Y.copy())
    return (time.perf_counter() - t0) / steps * 1e6


def bench(n, chains, tune, draws, host_steps):
    drv, obs = tower(n)
    problem = mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=np.full(n, 0.2), max_draws=chains)
    rows = np.repeat(np.array([P[k] for k in cal.PARAM_NAMES])[None], chains, axis=0)
    problem.objective(rows)
    obj_ms = problem.gpu_milliseconds(20)
    s = cal.DEMetropolisZ(problem, P, PRIOR, chains=chains, tune=tune, seed=1)
    s.run(64)                       # capture + first replays outside the timed call
    t0 = time.perf_counter()
    s.run(tune + draws)
    wall = time.perf_counter() - t0
    steps = tune + draws
    gpu_us = s.last_gpu_ms * 1e3 / steps
    _, _, _, _, acc, sc, _ = s.read(s.steps - draws, draws)
    out = {'n': n, 'chains': chains, 'steps': steps, 'step_us_gpu': round(gpu_us, 2),
           'step_us_wall': round(wall / steps * 1e6, 2),
           'chain_draws_per_s': round(chains * steps / wall, 1),
           'objective_graph_us': round(obj_ms * 1e3, 2),
           'sampler_over_objective': round(gpu_us / (obj_ms * 1e3), 4),
           'acceptance_rate_mean': round(float(acc.mean()), 4)}
    if host_steps:
        hs = host_steps if chains <= 64 else max(20, host_steps // 10)
        out['host_loop_step_us'] = round(host_loop_us(problem, chains, hs), 2)
        out['host_loop_steps_timed'] = hs
        out['sampler_over_host_loop'] = round(out['step_us_wall'] / out['host_loop_step_us'], 4)
    s.close()
    problem.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--config', action='append', help='N,CHAINS (repeatable)')
    ap.add_argument('--tune', type=int, default=1000)
    ap.add_argument('--draws', type=int, default=5000)
    ap.add_argument('--host-steps', type=int, default=500)
    a = ap.parse_args()
    configs = [tuple(int(v) for v in c.split(',')) for c in a.config] if a.config else \
        [(n, c) for n in (1 << 14, 1 << 17) for c in (3, 64, 1024)]
    res = {'tool': 'mcmcbench', 'build_id': _lib.build_id(), 'tune': a.tune, 'draws': a.draws,
           'free_parameters': len(PRIOR), 'runs': []}
    try:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    for n, c in configs:
        r = bench(n, c, a.tune, a.draws, a.host_steps)
        print(json.dumps(r), file=sys.stderr, flush=True)
        res['runs'].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
