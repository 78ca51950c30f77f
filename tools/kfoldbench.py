#!/usr/bin/env python3
"""k-fold cross-validation in one sampler (mod16_amd.calibration, DEMetropolisZ(..., folds=...)) on
synthetic towers of n site-days -- tools/mcmcbench.py's tower(), drawn by tools/_drivers.py -- with
the 8 free parameters of tools/mcmcbench.py, in one GPU process. For n in {2^14, 2^17} (default) and
chains in {3, 64}:

  plain      us per step of a plain sampler of `chains` chains (GPU time of the captured graphs)
  folds      us per step of K = 5 folds x `chains` chains in one graph, and that over K x plain
  objective  the fold objective (TRAIN codes, K x chains draws) against the plain objective at the
             same number of draws: GPU time of the cached graph (problem.gpu_milliseconds)
  heldout    wall time of sampler.heldout() on 5 folds x 3 chains x 5000 kept draws (n only)

  python tools/kfoldbench.py [--out FILE] [--n N ...] [--chains C ...] [--steps S]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mod16_amd  # noqa: E402
from mod16_amd import _lib, calibration as cal  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from mcmcbench import P, PRIOR, tower  # noqa: E402

K = 5


def step_us(problem, chains, steps, folds=None):
    s = cal.DEMetropolisZ(problem, P, PRIOR, chains=chains, tune=steps, seed=1, folds=folds)
    s.run(64)                       # capture + first replays outside the timed call
    s.run(steps)
    us = s.last_gpu_ms * 1e3 / steps
    s.close()
    return us


def bench(n, chains, steps):
    drv, obs = tower(n)
    problem = mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=np.full(n, 0.2),
                                       max_draws=max(K * chains, 1024), folds=K)
    plain = step_us(problem, chains, steps)
    folds = step_us(problem, chains, steps, folds=True)
    D = K * chains
    rows = np.repeat(np.array([P[k] for k in cal.PARAM_NAMES])[None], D, axis=0)
    problem.objective(rows)
    obj_plain = problem.gpu_milliseconds(50)
    problem.objective(rows, folds=np.arange(D) % K)
    obj_fold = problem.gpu_milliseconds(50)
    problem.objective(rows)
    obj_plain2 = problem.gpu_milliseconds(50)
    out = {'n': n, 'chains': chains, 'folds': K, 'steps': steps,
           'plain_step_us': round(plain, 2), 'folds_step_us': round(folds, 2),
           'folds_over_k_plain': round(folds / (K * plain), 4),
           'objective_draws': D, 'objective_plain_us': round(obj_plain * 1e3, 2),
           'objective_fold_us': round(obj_fold * 1e3, 2), 'objective_plain_again_us': round(obj_plain2 * 1e3, 2),
           'fold_over_plain_objective': round(obj_fold / obj_plain, 4)}
    problem.close()
    return out


def heldout(n, draws):
    drv, obs = tower(n)
    problem = mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=np.full(n, 0.2), max_draws=1024, folds=K)
    s = cal.DEMetropolisZ(problem, P, PRIOR, chains=3, tune=200, seed=1, folds=True)
    tr = s.sample(draws)
    t0 = time.perf_counter()
    res = s.heldout(tr)
    wall = time.perf_counter() - t0
    rows = K * 3 * draws + K
    out = {'n': n, 'heldout_rows': rows, 'heldout_wall_s': round(wall, 4),
           'heldout_rows_per_s': round(rows / wall, 1),
           'posterior_mean_heldout_rmsd': {str(f): round(r['mean_rmsd'], 4) for f, r in res.items()}}
    s.close()
    problem.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--n', type=int, action='append')
    ap.add_argument('--chains', type=int, action='append')
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--heldout-draws', type=int, default=5000)
    a = ap.parse_args()
    res = {'tool': 'kfoldbench', 'build_id': _lib.build_id(), 'free_parameters': len(PRIOR), 'runs': [],
           'heldout': []}
    try:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    for n in a.n or [1 << 14, 1 << 17]:
        for c in a.chains or [3, 64]:
            r = bench(n, c, a.steps)
            print(json.dumps(r), file=sys.stderr, flush=True)
            res['runs'].append(r)
        r = heldout(n, a.heldout_draws)
        print(json.dumps(r), file=sys.stderr, flush=True)
        res['heldout'].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
