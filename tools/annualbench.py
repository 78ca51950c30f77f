#!/usr/bin/env python3
"""The annual-precipitation constraint in the sampler (mod16_amd.calibration, DEMetropolisZ(...,
constraints=True)) on synthetic towers -- tools/mcmcbench.py's tower(), drawn by tools/_drivers.py
-- with the 8 free parameters of tools/mcmcbench.py, in one GPU process. The two sizes the README
quotes for the sampler, as (T days, N sites) problems of whole years of 365 days at one site:

  3 chains  x (45 x 365, 1)  = 16425 site-days (2^14 = 16384)
  64 chains x (360 x 365, 1) = 131400 site-days (2^17 = 131072)

Every site-year is padded to 6 waves of 64 pixels (365 -> 384), so the constrained problem holds
5.2 % more pixels than the caller's. Per size, us per sampler step (GPU time of the captured graphs):

  plain            a plain sampler on a problem bound WITHOUT the constraint (the caller's layout)
  plain_on_annual  a plain sampler on the problem bound with the constraint (the padded layout,
                   the plain kernels): what the layout alone costs
  annual           the constrained sampler on that problem (the ANNUAL kernels and the penalty's)

and the GPU time of the cached objective graphs at `chains` draws, plain and constrained.

  python tools/annualbench.py [--out FILE] [--config YEARS,SITES,CHAINS ...] [--steps S]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mod16_amd  # noqa: E402
from mod16_amd import _lib, calibration as cal  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from mcmcbench import P, PRIOR, tower  # noqa: E402


def step_us(problem, chains, steps, constraints=None):
    s = cal.DEMetropolisZ(problem, P, PRIOR, chains=chains, tune=steps, seed=1, constraints=constraints)
    s.run(64)                       # capture + first replays outside the timed call
    s.run(steps)
    us = s.last_gpu_ms * 1e3 / steps
    s.close()
    return us


def bench(years, sites, chains, steps):
    T = years * 365
    n = T * sites
    drv, obs = tower(n)
    drv = [np.asarray(v, np.float64).reshape(T, sites) for v in drv]
    obs = obs.reshape(T, sites)
    w = np.full((T, sites), 0.2)
    year = np.repeat(2000 + np.arange(years), 365)
    lhv = mod16_amd.latent_heat_vaporization((drv[5] + drv[6]) / 2)
    pvec = [P[k] for k in mod16_amd.MOD16.required_parameters]
    mass = np.maximum(mod16_amd.MOD16._et(pvec, *drv) * 86400.0 / lhv, 0.0)
    limit = 0.8 * mass.reshape(years, 365, sites).sum(axis=1)       # binding at the planted parameters
    plain_problem = mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=w, max_draws=max(chains, 64))
    plain = step_us(plain_problem, chains, steps)
    rows = np.repeat(np.array([P[k] for k in cal.PARAM_NAMES])[None], chains, axis=0)
    plain_problem.objective(rows)
    obj_plain = plain_problem.gpu_milliseconds(50)
    plain_problem.close()
    problem = mod16_amd.MOD16._et_bind(*drv, observed=obs, weights=w, max_draws=max(chains, 64),
                                       annual_precip=(year, limit))
    on_annual = step_us(problem, chains, steps)
    annual = step_us(problem, chains, steps, constraints=True)
    problem.objective(rows)
    obj_on_annual = problem.gpu_milliseconds(50)
    pen = problem.objective(rows, penalty=True)[2]
    obj_annual = problem.gpu_milliseconds(50)
    problem.close()
    return {'T': T, 'N': sites, 'n': n, 'site_years': years * sites, 'chains': chains, 'steps': steps,
            'plain_step_us': round(plain, 2), 'plain_on_annual_step_us': round(on_annual, 2),
            'annual_step_us': round(annual, 2), 'annual_over_plain': round(annual / plain, 4),
            'annual_over_plain_on_annual': round(annual / on_annual, 4),
            'objective_plain_us': round(obj_plain * 1e3, 2), 'objective_plain_on_annual_us': round(obj_on_annual * 1e3, 2),
            'objective_annual_us': round(obj_annual * 1e3, 2), 'penalty_at_planted': float(pen[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--config', action='append', help='YEARS,SITES,CHAINS (repeatable)')
    ap.add_argument('--steps', type=int, default=2000)
    a = ap.parse_args()
    configs = [tuple(int(v) for v in c.split(',')) for c in a.config] if a.config else [(45, 1, 3), (360, 1, 64)]
    res = {'tool': 'annualbench', 'build_id': _lib.build_id(), 'free_parameters': len(PRIOR), 'runs': []}
    try:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    for years, sites, chains in configs:
        r = bench(years, sites, chains, a.steps)
        print(json.dumps(r), file=sys.stderr, flush=True)
        res['runs'].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
