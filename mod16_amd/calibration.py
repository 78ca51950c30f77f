r'''
MCMC calibration of MOD16 parameters on the GPU: the reference's ``mod16/calibration.py`` sampler
without PyMC.

The reference's ``MOD16StochasticSampler`` (calibration.py:152-267) builds a PyMC model whose
priors come from a prior YAML (``CalibrationAPI.tune``, calibration.py:923-931), wraps
``MOD16._et`` as a black-box likelihood (mod17's ``BlackBoxLikelihood``) and samples it with PyMC's
``DEMetropolisZ``, one chain per process, evaluating the model one draw at a time on the CPU.

Here the whole chain lives on the device (``mod16_mcmc_*``, C ABI ``include/mod16_hip.h``; the
arithmetic is stated in full at the top of ``mod16_amd/csrc/mod16_mcmc.hpp``):

- ``load_prior(path, pft)``: the prior dict ``tune()`` builds from a YAML laid out as the
  reference's (per parameter, lists indexed by PFT, ``~`` for none);
- ``DEMetropolisZ(problem, params, prior, ...)``: independent DE-MCMC-Z chains (ter Braak & Vrugt
  2008) over the free parameters of a ``MOD16._et_bind`` problem. Proposals, prior densities, the
  likelihood, the Metropolis decision, tuning and the Z-history are in device memory; K steps run
  as one captured graph; any number of chains (up to the problem's ``max_draws``) run in one batch;
- ``Trace``: the samples (x-values) of the free parameters, log-likelihood, log-posterior and
  acceptance per step, ``posterior(burn, thin)``, ``rhat()`` (classic split R-hat, BDA3) and
  ``to_npz``;
- k-fold cross-validation, the reference's ``CalibrationAPI.tune(pft, k_folds=K)``
  (calibration.py:851-958): ``kfold_labels(n, K)`` (its random partition of the tower-days),
  ``MOD16._et_bind(..., folds=K or labels)``, and ``DEMetropolisZ(problem, ..., folds=True)``: the
  chains of every fold in ONE sampler -- each fold's chains train on the site-days outside it -- with
  a ``KFoldTrace`` (``trace.fold(f)`` a plain ``Trace``; R-hat per fold) and ``sampler.heldout(trace)``
  (the held-out RMSD of every kept draw and of the posterior mean);
- the annual-precipitation constraint, the reference's ``constrain_by_map`` (calibration.py:776-796,
  wired in at :827-849; the only constraint it supports, what its ``classes_are_dynamic``
  calibrations use): ``MOD16._et_bind(..., annual_precip=(years, precip))`` on a (T days x N sites)
  problem, ``problem.penalty(params)``, ``DEMetropolisZ(problem, ..., constraints=True)`` and
  ``sampler.penalty(trace)``; ``annual_precip_penalty`` states the formula in numpy. The sums per
  site-year are made on the device inside the objective's launches; nothing of size draws x n exists;
- ``ensemble_tables(table, posterior, members)``: from posteriors to the parameter tables of an
  ensemble forward run (``mod16_amd.evapotranspiration_ensemble``, ``RasterEngine.ensemble``): joint
  draws without replacement per PFT, host only -- what the reference's ``export_posterior``
  (calibration.py:633-709) hands on, put onto a raster;
- ``quantile_positions(q, members)`` and ``ensemble_quantile(x, q)``: the numpy statement of the
  per-pixel quantiles over the members of an ensemble run
  (``mod16_amd.evapotranspiration_ensemble_quantiles``, ``EnsembleRun.quantiles``): the definition
  the selection kernel follows operation for operation. Host only.

  The reference's own k-fold loop does not do what its docstring says, and this port does what the
  docstring says. (1) The restore-and-mask block (``tower_obs[idx] = np.nan`` and the driver filter,
  :889-901) is indented inside ``if k_folds > 1 and fold == 1:``, so folds 2..K never mask their own
  test set: they refit fold 1's training subset under new backend names. Here fold f trains on
  everything except its own test slice. (2) ``fold_idx[-1][-1] = indices.max()`` ends the last slice
  at ``n - 1``, exclusive, so the last shuffled row is never held out; here the last slice runs to
  the end. Do not "fix" either back toward the reference.

The sampler is the project's own restatement of PyMC's ``DEMetropolisZ`` (its ``astep``, ``tune``
table and ``stop_tuning`` history drop), and the likelihoods -- ``'rmsd'``: ``-sqrt(sse / count)``,
mod17's ``BlackBoxLikelihood`` as the reference's shipped config uses it; ``'gaussian'``:
``-sse / 2`` -- are the project's restatements of mod17's. Neither PyMC nor mod17 is available to
check against, and the random stream is the project's own (counter-based), so chains are not
PyMC's draw for draw. With ``constraints`` the penalty is ADDED to the log-likelihood of either
objective: how mod17's ``BlackBoxLikelihood`` combines its ``constraints`` with the objective cannot
be read here (mod17 is absent), so adding is likewise this project's restatement. The reference
config's hint to "use nRMSD if there are constraints" names an objective that is defined nowhere in
the reference; it is left out. A NaN penalty (a NaN prediction anywhere in a site-year) makes the log
posterior NaN: such a step is rejected, such an initial point refused -- what the reference's
arithmetic gives too. The defaults (``tune=1000``, ``scaling=1e-3``, ``tune_interval=100``,
``tune_drop_fraction=0.9``, ``lamb = 2.38 / sqrt(2 d)``) are PyMC's and the reference config's;
``tune=1000`` is pm.sample's default, which mod17's ``run()`` is believed, not verified, to keep.
Every chain starts at the priors' support points (Uniform: the midpoint; LogNormal:
exp(mu + sigma^2 / 2); Triangular: (lower + upper + c) / 3) -- believed, not verified, to be PyMC's
initial point -- unless ``initial`` is given. The caller states the fixed parameters explicitly
(the reference fixes ``tmin_close``, ``tmin_open`` and ``vpd_open`` from the BPLUT row plus
``config['optimization']['fixed']``).

Not provided: HDF5 loading (h5py is absent; ``tools/h5_to_store.py`` covers the field map), the
constraint together with k-fold cross-validation (the reference's own combination cannot run: its
closure indexes a (T,)-long mask into ravelled, compacted rows), the constraint on float32, EXACT or
device-bound problems, plots, netCDF / arviz backends, population DE-MCMC (proposals drawn from
other chains), several GPUs, float32 problems.
There is no CPU fallback: without an MI355X the sampler raises ``Mod16Error``.
'''
import ctypes as C
import math

import numpy as np

from . import _lib
from . import MOD16

PARAM_NAMES = list(MOD16.required_parameters)
FAMILIES = ('uniform', 'lognormal', 'triangular')
_FAMILY_CODE = {'uniform': _lib.PRIOR_UNIFORM, 'lognormal': _lib.PRIOR_LOGNORMAL,
                'triangular': _lib.PRIOR_TRIANGULAR}
OBJECTIVES = ('rmsd', 'gaussian')
CONSTRAINTS = ('annual_precipitation',)
HALF_LOG_2PI = float.fromhex('0x1.d67f1c864beb4p-1')
_M64 = (1 << 64) - 1


def load_prior(path, pft):
    '''The prior of PFT ``pft`` from a YAML laid out as the reference's prior files: what
    ``CalibrationAPI.tune`` builds (calibration.py:923-931), ``{name: {key: value}}`` for the
    parameters of ``MOD16.required_parameters`` the file names, in that order.'''
    import yaml
    with open(path, 'r') as f:
        prior = yaml.safe_load(f)
    return {p: {k: v[pft] for k, v in prior[p].items()} for p in PARAM_NAMES if p in prior}


def prior_family(spec):
    '''(family, (p0, p1, p2)) of one parameter's prior, inferred from its keys as in the reference's
    prior YAML: ``lower``/``upper`` Uniform, ``mu``/``sigma`` LogNormal, ``lower``/``upper``/``c``
    Triangular. Refuses (``ValueError``) other key sets and bad values.'''
    keys = set(spec)
    val = lambda k: float(spec[k]) if spec[k] is not None else float('nan')
    if keys == {'lower', 'upper'}:
        fam, p = 'uniform', (val('lower'), val('upper'), 0.0)
    elif keys == {'mu', 'sigma'}:
        fam, p = 'lognormal', (val('mu'), val('sigma'), 0.0)
    elif keys == {'lower', 'upper', 'c'}:
        fam, p = 'triangular', (val('lower'), val('upper'), val('c'))
    else:
        raise ValueError('prior keys %s: expected lower/upper, mu/sigma or lower/upper/c' % sorted(keys))
    if not all(np.isfinite(p)):
        raise ValueError('%s prior %r: every value must be a finite number' % (fam, dict(spec)))
    if fam == 'lognormal' and not p[1] > 0:
        raise ValueError('lognormal prior: sigma must be > 0 (got %r)' % p[1])
    if fam != 'lognormal' and not p[0] < p[1]:
        raise ValueError('%s prior: lower < upper needed (got %r, %r)' % (fam, p[0], p[1]))
    if fam == 'triangular' and not p[0] <= p[2] <= p[1]:
        raise ValueError('triangular prior: c must lie in [lower, upper] (got %r)' % p[2])
    return fam, p


# ---- the arithmetic of mod16_mcmc.hpp in numpy (host reference of the device code)
def _softplus(z):
    z = np.asarray(z, np.float64)
    with np.errstate(over='ignore'):
        return np.where(z > 36.0, z, np.log1p(np.exp(np.minimum(z, 36.0))))


def x_of_y(family, p, y):
    '''The model's x of the sampler's y (float64, numpy).'''
    y = np.asarray(y, np.float64)
    if family == 'lognormal':
        return np.exp(y)
    with np.errstate(over='ignore'):
        s = 1.0 / (1.0 + np.exp(-y))
    return p[0] + (p[1] - p[0]) * s


def y_of_x(family, p, x):
    '''The sampler's y of an x inside the support.'''
    x = np.asarray(x, np.float64)
    if family == 'lognormal':
        return np.log(x)
    q = (x - p[0]) / (p[1] - p[0])
    return np.log(q / (1.0 - q))


def log_prior(family, p, y):
    '''log p(y) of the prior in y-space, the Jacobian of x(y) included (-inf where the density is
    0 or undefined).'''
    y = np.asarray(y, np.float64)
    if family == 'lognormal':
        u = y - p[0]
        return (-np.log(p[1]) - HALF_LOG_2PI) - (u * u) / (2.0 * p[1] * p[1])
    logistic = -y - 2.0 * _softplus(-y)
    if family == 'uniform':
        return logistic
    a, b, c = p
    x = x_of_y(family, p, y)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(x < c, 2.0 * (x - a) / ((b - a) * (c - a)), 2.0 * (b - x) / ((b - a) * (b - c)))
        lf = np.where(f > 0.0, np.log(np.where(f > 0.0, f, 1.0)), -np.inf)
    return ((lf + np.log(b - a)) - y) - 2.0 * _softplus(-y)


def support_point(family, p):
    '''The initial x of a chain: Uniform the midpoint, LogNormal exp(mu + sigma^2 / 2),
    Triangular (lower + upper + c) / 3.'''
    if family == 'uniform':
        return p[0] + (p[1] - p[0]) / 2.0
    if family == 'lognormal':
        return math.exp(p[0] + p[1] * p[1] / 2.0)
    return (p[0] + p[1] + p[2]) / 3.0


def tune_factor(rate):
    '''PyMC's tune(): the factor scaling (or lamb) is multiplied by, from the acceptance rate.'''
    if rate < 0.001:
        return 0.1
    if rate < 0.05:
        return 0.5
    if rate < 0.2:
        return 0.9
    if rate > 0.95:
        return 10.0
    if rate > 0.75:
        return 2.0
    if rate > 0.5:
        return 1.1
    return 1.0


def mix(z):
    '''splitmix64's finaliser on a Python int (uint64).'''
    z &= _M64
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & _M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def stream(seed, c, t, k):
    '''r(c, t, k) = mix(mix(mix(seed) ^ c) ^ ((t << 6) | k)): the sampler's random word of chain c,
    step t, slot k.'''
    return mix(mix(mix(int(seed)) ^ int(c)) ^ ((int(t) << 6) | int(k)))


def unit(z):
    return float(z >> 11) * 2.0 ** -53


def index(z, m):
    return (z * int(m)) >> 64


def group_stream(seed, fold, j, t, k):
    '''The random word of chain j of the group of fold ``fold`` (``DEMetropolisZ(..., folds=...)``):
    the plain stream with seed (seed + fold) mod 2^64 and chain index j.'''
    return stream((int(seed) + int(fold)) & _M64, j, t, k)


def annual_precip_penalty(le, years, lhv, annual_precip):
    '''The reference's ``constrain_by_map`` (calibration.py:776-796) in numpy, float64: ``le``
    (..., T, N) predicted latent heat flux [W m-2], ``years`` (T,) the year of each day, ``lhv``
    (T, N) latent heat of vaporization [J kg-1], ``annual_precip`` (Y, N) [mm per year], rows in the
    order of ``np.unique(years)``:

        mass = max(le * 86400 / lhv, 0); tot[y, n] = sum of mass over the days of year y
        over = max(tot - annual_precip, 0); penalty = -100 * mean(over ** 2) / annual_precip.sum()

    with NaN kept by both max (``x[x < 0] = 0``), over every day, observed or not. Returns (...):
    <= 0, or NaN. (Host statement of what ``problem.penalty`` computes on the device.)'''
    le = np.asarray(le, np.float64)
    lhv = np.asarray(lhv, np.float64)
    annual_precip = np.asarray(annual_precip, np.float64)
    uniq, inv = np.unique(np.asarray(years), return_inverse=True)
    inv = inv.reshape(-1)
    if le.ndim < 2 or le.shape[-2:] != lhv.shape or inv.size != le.shape[-2] or \
            annual_precip.shape != (uniq.size, le.shape[-1]):
        raise ValueError('le (..., T, N), years (T,), lhv (T, N) and annual_precip (Y, N) do not fit: %s, %s, %s, %s'
                         % (le.shape, np.shape(years), lhv.shape, annual_precip.shape))
    with np.errstate(invalid='ignore', over='ignore'):
        mass = (le * 60 * 60 * 24) / lhv
        mass = np.where(mass < 0, 0.0, mass)
        tot = np.stack([mass[..., inv == k, :].sum(axis=-2) for k in range(uniq.size)], axis=-2)
        diff = tot - annual_precip
        diff = np.where(diff < 0, 0.0, diff)
        return -(100 * ((diff ** 2).mean(axis=(-2, -1)) / annual_precip.sum()))


def kfold_labels(n, k, seed=0):
    '''The fold label (0 .. k-1, uint8, (n,)) of each of ``n`` site-days: the reference's partition
    (calibration.py:859-869) -- a permutation of range(n) (here
    ``np.random.default_rng(seed).permutation(n)``; the reference's is unseeded) cut into k
    consecutive slices of n // k, the last slice taking the remainder through the final index (the
    reference's ends one short, see the module docstring); a row's label is its slice.'''
    n, k = int(n), int(k)
    if not 2 <= k <= 255:
        raise ValueError('k must lie in 2 .. 255 (got %d)' % k)
    if n < k:
        raise ValueError('k = %d folds need at least k site-days (got n = %d)' % (k, n))
    perm = np.random.default_rng(seed).permutation(n)
    size = n // k
    labels = np.empty(n, np.uint8)
    for f in range(k):
        labels[perm[f * size:(f + 1) * size if f < k - 1 else n]] = f
    return labels


class Trace(object):
    '''The draws of a ``DEMetropolisZ.sample`` call: ``samples[name]`` (chains, draws) x-values of
    the free parameters; ``log_likelihood``, ``log_posterior`` (chains, draws) float64; ``accepted``
    (chains, draws) bool; ``scaling``, ``lamb`` (chains,) at the end of the call; ``acceptance_rate``
    (chains,) over these draws.'''

    def __init__(self, names, samples, log_likelihood, log_posterior, accepted, scaling, lamb):
        self.names = list(names)
        self.samples = samples
        self.log_likelihood = log_likelihood
        self.log_posterior = log_posterior
        self.accepted = accepted
        self.scaling = scaling
        self.lamb = lamb
        self.acceptance_rate = accepted.mean(axis=1) if accepted.shape[1] else np.full(accepted.shape[0], np.nan)

    @property
    def chains(self):
        return self.accepted.shape[0]

    @property
    def draws(self):
        return self.accepted.shape[1]

    def posterior(self, burn=0, thin=1):
        '''{name: (chains, k)}: the draws after the first ``burn``, every ``thin``-th.'''
        burn, thin = int(burn), int(thin)
        if burn < 0 or thin < 1:
            raise ValueError('burn >= 0 and thin >= 1 needed')
        return {k: v[:, burn::thin] for k, v in self.samples.items()}

    def rhat(self, burn=0, thin=1):
        '''Split R-hat (BDA3, Gelman et al. 2013, 11.4) per free parameter: each chain's draws cut
        in two halves (the middle draw dropped when odd), then sqrt(var+ / W) over the halves.'''
        out = {}
        for name, v in self.posterior(burn, thin).items():
            n = v.shape[1] // 2
            if n < 2:
                raise ValueError('split R-hat needs at least 4 draws per chain')
            halves = np.concatenate([v[:, :n], v[:, v.shape[1] - n:]], axis=0)
            m = halves.shape[0]
            means = halves.mean(axis=1)
            B = n / (m - 1.0) * np.sum((means - means.mean()) ** 2)
            W = halves.var(axis=1, ddof=1).mean()
            var_plus = (n - 1.0) / n * W + B / n
            out[name] = float(np.sqrt(var_plus / W)) if W > 0 else float('nan')
        return out

    def to_npz(self, path, **extra):
        '''All of the trace in one ``.npz`` (samples under their parameter names).'''
        np.savez(path, names=np.array(self.names), log_likelihood=self.log_likelihood,
                 log_posterior=self.log_posterior, accepted=self.accepted, scaling=self.scaling,
                 lamb=self.lamb, acceptance_rate=self.acceptance_rate,
                 **dict({'sample_' + k: v for k, v in self.samples.items()}, **extra))

    def _take(self, chains):
        return Trace(self.names, {k: v[chains] for k, v in self.samples.items()},
                     self.log_likelihood[chains], self.log_posterior[chains], self.accepted[chains],
                     self.scaling[chains], self.lamb[chains])


def test_indices(labels, k):
    '''The reference-shaped ``test_indices`` (k, max fold size) int64 of fold labels: row f the
    site-days of fold f, ascending, padded with -1 (the reference pads with NaN in a uint32 array).'''
    rows = [np.flatnonzero(labels == f) for f in range(k)]
    out = np.full((k, max(r.size for r in rows)), -1, np.int64)
    for f, r in enumerate(rows):
        out[f, :r.size] = r
    return out


class KFoldTrace(Trace):
    '''The trace of a cross-validating sampler (``DEMetropolisZ(..., folds=...)``): a ``Trace`` over
    every chain of every fold, and ``chain_fold`` (chains,), the fold each chain trains for.
    ``fold(f)`` is the plain ``Trace`` of fold f's chains; ``rhat()`` is ``{f: {name: R-hat}}``,
    per fold (chains of different folds sample different posteriors).'''

    def __init__(self, names, samples, log_likelihood, log_posterior, accepted, scaling, lamb,
                 chain_fold, labels, nfolds):
        super().__init__(names, samples, log_likelihood, log_posterior, accepted, scaling, lamb)
        self.chain_fold = np.asarray(chain_fold)
        self.folds = sorted(set(int(f) for f in self.chain_fold))
        self.labels = labels
        self.nfolds = nfolds

    def fold(self, f):
        if int(f) not in self.folds:
            raise ValueError('fold %r is not sampled here (folds %s)' % (f, self.folds))
        return self._take(np.flatnonzero(self.chain_fold == int(f)))

    def rhat(self, burn=0, thin=1):
        return {f: self.fold(f).rhat(burn, thin) for f in self.folds}

    def to_npz(self, path):
        '''As ``Trace.to_npz``, plus ``chain_fold``, the fold ``labels`` of the site-days and the
        reference-shaped ``test_indices`` (``test_indices()``).'''
        super().to_npz(path, chain_fold=self.chain_fold, labels=self.labels,
                       test_indices=test_indices(self.labels, self.nfolds))


def ensemble_tables(table, posterior, members, seed=0, burn=0, thin=1):
    '''
    From posteriors to the parameter tables of an ensemble forward run
    (``mod16_amd.evapotranspiration_ensemble``, ``RasterEngine.ensemble``): what the reference's
    ``export_posterior`` (calibration.py:633-709) hands on as one (PFT, samples) array per parameter,
    drawn down to ``members`` tables. Host only.

    Parameters
    ----------
    table : numpy.ndarray
        (13, 11) base table (``mod16_amd.utils.bplut_table``): the value of every parameter that
        was not calibrated and every row of a PFT that was not
    posterior : dict
        ``{pft: Trace}`` or ``{pft: {name: (chains, k) array}}`` (``Trace.posterior()``)
    members : int
        tables to draw
    seed : int
        PFT ``pft`` draws with ``numpy.random.default_rng([seed, pft])``
    burn, thin : int
        every chain's draws after the first ``burn``, every ``thin``-th, are the pool

    For each PFT the kept draws of all chains are pooled chain-major (pool index = chain * k + draw)
    and ``members`` pool indices are picked WITHOUT replacement; one index serves all of that PFT's
    free parameters -- a member's row is a joint draw, so the posterior's correlations survive.
    ``ValueError`` if a pool holds fewer than ``members`` draws. Returns (members, 13, 11) float64.
    '''
    base = np.array(table, np.float64)
    if base.shape != (_lib.N_CLASSES, _lib.N_PARAMS):
        raise ValueError('table must have shape (13, 11), got %r' % (base.shape,))
    members, burn, thin = int(members), int(burn), int(thin)
    if members < 1:
        raise ValueError('members >= 1 needed')
    if burn < 0 or thin < 1:
        raise ValueError('burn >= 0 and thin >= 1 needed')
    out = np.repeat(base[None], members, axis=0)
    for pft, post in posterior.items():
        if int(pft) != pft or not 0 <= int(pft) < _lib.N_CLASSES:
            raise ValueError('PFT code %r is not one of 0..12' % (pft,))
        samples = post.samples if isinstance(post, Trace) else post
        unknown = [k for k in samples if k not in PARAM_NAMES]
        if unknown:
            raise ValueError('unknown parameter name(s) %s; expected some of %s' % (unknown, PARAM_NAMES))
        kept, shape = {}, None
        for name, v in samples.items():
            v = np.asarray(v, np.float64)
            if v.ndim != 2:
                raise ValueError('samples of %r must have shape (chains, draws), got %r' % (name, v.shape))
            if shape is not None and v.shape != shape:
                raise ValueError('samples of PFT %d differ in shape: %r and %r' % (pft, shape, v.shape))
            shape = v.shape
            kept[name] = np.ascontiguousarray(v[:, burn::thin]).reshape(-1)      # chain-major
        if not kept:
            continue
        pool = next(iter(kept.values())).size
        if pool < members:
            raise ValueError('PFT %d: %d draws in the pool (chains x kept draws), %d members wanted'
                             % (pft, pool, members))
        pick = np.random.default_rng([int(seed), int(pft)]).choice(pool, size=members, replace=False)
        for name, v in kept.items():
            out[:, int(pft), PARAM_NAMES.index(name)] = v[pick]
    return out


MAX_QUANTILES = 8


def quantile_positions(q, members):
    '''
    Where the quantiles ``q`` fall among ``members`` ordered values: ``h = q * (members - 1)`` (one
    float64 multiply), ``lo = floor(h)``, ``frac = h - lo`` -- numpy's default ``'linear'`` method.

    ``q`` is a scalar (a 1-tuple) or a sequence of 1 to 8 values, each in [0, 1] and not NaN; anything
    else raises ``ValueError``. Returns ``(lo int64 (Q,), frac float64 (Q,))``.
    '''
    members = int(members)
    if members < 1:
        raise ValueError('members >= 1 needed')
    q = np.atleast_1d(np.asarray(q, np.float64))
    if q.ndim != 1 or not 1 <= q.size <= MAX_QUANTILES:
        raise ValueError('q must be a scalar or a sequence of 1 to %d values' % MAX_QUANTILES)
    if not ((q >= 0.0) & (q <= 1.0)).all():       # (a NaN compares false)
        raise ValueError('every q must lie in [0, 1] and not be NaN')
    h = q * np.float64(members - 1)
    lo = np.floor(h)
    return lo.astype(np.int64), h - lo


def ensemble_quantile(x, q):
    '''
    The quantiles ``q`` over axis 0 of ``x`` (members first, float64): THE definition of what
    ``mod16_et_ensemble_quantiles_*`` returns; its selection kernel follows this statement operation
    for operation. With ``lo, frac = quantile_positions(q, D)`` and ``s`` the members in ascending
    order, ``a = s[lo]``, ``b = s[min(lo + 1, D - 1)]``; the value is ``a`` where ``frac == 0`` or
    ``a == b``, else ``a + frac * (b - a)`` (a multiply, then an add: two roundings). On finite members
    this is ``np.quantile(x, q, axis=0)`` to 3.3e-16 max|x_m| (measured, D = 1 ... 256, zeros and ties
    included). A NaN anywhere along axis 0 makes all Q values of that column NaN. The ``frac == 0`` /
    ``a == b`` rule defines infinite members: equal infinities stay, a position that falls exactly on
    a finite member is that member (``np.quantile`` gives NaN in both cases).

    Returns float64 ``(Q,) + x.shape[1:]``.
    '''
    x = np.asarray(x, np.float64)
    if x.ndim < 1 or x.shape[0] < 1:
        raise ValueError('x must have at least one member along axis 0')
    D = x.shape[0]
    lo, frac = quantile_positions(q, D)
    nan = np.isnan(x).any(axis=0)
    s = np.sort(np.where(nan, 0.0, x), axis=0)
    out = np.empty((lo.size,) + x.shape[1:], np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(lo.size):
            a, b = s[lo[k]], s[min(lo[k] + 1, D - 1)]
            t = frac[k] * (b - a)
            v = np.where((frac[k] == 0.0) | (a == b), a, a + t)
            out[k] = np.where(nan, np.nan, v)
    return out


def _row(params):
    if hasattr(params, 'items'):
        unknown = [k for k in params if k not in PARAM_NAMES]
        if unknown:
            raise ValueError('unknown parameter name(s) %s; expected some of %s' % (unknown, PARAM_NAMES))
        return [params.get(k) for k in PARAM_NAMES]
    row = list(params)
    if len(row) != len(PARAM_NAMES):
        raise ValueError('params must be a dict or a sequence of %d values (MOD16.required_parameters order)'
                         % len(PARAM_NAMES))
    return row


def _number(v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        return float('nan')
    return v


class DEMetropolisZ(object):
    '''
    Independent DE-MCMC-Z chains on the GPU over the free parameters of a resident calibration
    problem (``MOD16._et_bind(..., observed=..., weights=..., max_draws >= chains)``, float64,
    ``math=MATH_FAST``).

    ``params``: a BPLUT row (dict or 11 values, ``MOD16.required_parameters`` order) that supplies
    the fixed values. ``prior``: ``{name: {lower, upper} | {mu, sigma} | {lower, upper, c}}`` (what
    ``load_prior`` returns); a parameter with a prior is free unless ``fixed`` names it. ``fixed``:
    ``{name: value}`` overriding ``params`` (a ``None`` value fixes nothing, as in the reference).
    Every parameter must end up free or with a finite value -- a NaN ``beta`` with neither is an
    error (the reference silently puts in 250). ``tune_target``: ``'scaling'``, ``'lambda'``
    (``'lamb'``) or ``None``. ``objective``: ``'rmsd'`` or ``'gaussian'`` (any case). ``initial``:
    optional (chains, d) x-values of the free parameters. ``segment``: steps per captured graph.
    ``folds`` (k-fold cross-validation, a problem bound with ``folds``): ``True`` (every fold) or a
    list of distinct folds; then ``chains`` chains run for each listed fold in the same graphs
    (``chains x folds <= max_draws``), each training on the site-days outside its fold. Chain j of
    the group of fold f (global chain g chains + j) is, draw for draw, the plain sampler with seed
    ``seed + f`` on the problem with fold f's observations set to NaN, whenever some training row
    has g_surf > 0 (``mod16_mcmc.hpp``); ``initial`` is then (chains, d), the same for every fold,
    or (folds, chains, d). ``sample`` returns a ``KFoldTrace``; ``heldout(trace)`` scores it.
    ``constraints`` (a problem bound with ``annual_precip``, no ``folds``): ``None``, ``True`` or
    ``('annual_precipitation',)``; the penalty of the row is then added to the log-likelihood of
    either objective -- ``Trace.log_likelihood`` includes it -- and ``penalty(trace)`` gives it alone.
    Everything is checked on the host before any device call (``ValueError``).
    '''

    def __init__(self, problem, params, prior, fixed=None, chains=3, tune=1000, tune_target='scaling',
                 tune_interval=100, tune_drop_fraction=0.9, scaling=1e-3, lamb=None, objective='rmsd',
                 seed=0, initial=None, segment=64, folds=None, constraints=None):
        self.problem = problem
        self._handle = C.c_void_p()
        row = _row(params)
        prior = dict(prior or {})
        fixed = dict(fixed or {})
        for what, names in (('prior', prior), ('fixed', fixed)):
            unknown = [k for k in names if k not in PARAM_NAMES]
            if unknown:
                raise ValueError('unknown parameter name(s) in %s: %s; expected some of %s'
                                 % (what, unknown, PARAM_NAMES))
        free, values = [], []
        for j, name in enumerate(PARAM_NAMES):
            is_fixed = name in fixed and fixed[name] is not None
            has_prior = prior.get(name) is not None and any(v is not None for v in prior[name].values())
            if is_fixed:
                v = _number(fixed[name])
                if not np.isfinite(v):
                    raise ValueError('fixed[%r] = %r: a fixed value must be a finite number' % (name, fixed[name]))
                values.append(v)
            elif has_prior:
                free.append((j, name) + prior_family(prior[name]))
                values.append(0.0)
            else:
                v = _number(row[j])
                if not np.isfinite(v):
                    raise ValueError('%r is neither free (no prior) nor fixed (no fixed value, params gives %r)'
                                     % (name, row[j]))
                values.append(v)
        if not free:
            raise ValueError('no free parameter: give at least one a prior')
        self.names = [f[1] for f in free]
        self.families = {f[1]: f[2] for f in free}
        self.prior_params = {f[1]: f[3] for f in free}
        self.fixed_row = np.array(values)
        d = len(free)
        self.chains = int(chains)
        self.tune = int(tune)
        self.tune_interval = int(tune_interval)
        self.tune_drop_fraction = float(tune_drop_fraction)
        self.scaling = float(scaling)
        self.lamb = 2.38 / math.sqrt(2 * d) if lamb is None else float(lamb)
        self.seed = int(seed) & _M64
        target = {None: 0, 'scaling': 1, 'lambda': 2, 'lamb': 2}
        key = tune_target.lower() if isinstance(tune_target, str) else tune_target
        if key not in target:
            raise ValueError("tune_target must be 'scaling', 'lambda' or None (got %r)" % (tune_target,))
        self.tune_target = key if key != 'lamb' else 'lambda'
        obj = str(objective).lower()
        if obj not in OBJECTIVES:
            raise ValueError('objective must be one of %s (got %r)' % (OBJECTIVES, objective))
        self.objective = obj
        if self.chains < 1:
            raise ValueError('chains must be >= 1')
        if self.tune < 0 or self.tune_interval < 1 or not 0.0 <= self.tune_drop_fraction < 1.0:
            raise ValueError('tune >= 0, tune_interval >= 1 and 0 <= tune_drop_fraction < 1 needed')
        if not (np.isfinite(self.scaling) and np.isfinite(self.lamb)):
            raise ValueError('scaling and lamb must be finite')
        if not 0 <= int(segment) <= 1024:
            raise ValueError('segment must be 0 .. 1024')
        # the problem: float64, FAST, with observations, room for the chains
        if getattr(problem, 'dtype', None) != np.float64:
            raise ValueError('the sampler needs a float64 problem (this one is %s)' % getattr(problem, 'dtype', None))
        if (int(problem.math) & 3) != _lib.MATH_FAST:
            raise ValueError('the sampler needs a problem bound with math=MATH_FAST (EXACT cannot be captured)')
        if not problem.has_observed:
            raise ValueError('the problem was bound without observed')
        #: the folds of the chain groups (None: a plain sampler)
        self.folds = None
        if isinstance(folds, (bool, np.bool_)):
            folds = True if folds else None         # (False: a plain sampler)
        elif folds is not None:
            arr = np.asarray(folds)
            if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
                raise ValueError('folds must be True or a list of folds (got %r)' % (folds,))
        if folds is not None:
            nf = getattr(problem, 'nfolds', 0)
            if not nf:
                raise ValueError('folds need a problem bound with folds (MOD16._et_bind(..., folds=...))')
            fl = list(range(nf)) if folds is True else [int(f) for f in folds]
            if not fl or len(set(fl)) != len(fl) or min(fl) < 0 or max(fl) >= nf:
                raise ValueError('folds must be True or distinct folds in 0 .. %d (got %r)' % (nf - 1, folds))
            self.folds = fl
        #: the constraints in force, names of ``CONSTRAINTS``
        self.constraints = ()
        if isinstance(constraints, (bool, np.bool_)):
            constraints = CONSTRAINTS if constraints else None
        if constraints is not None:
            names = (constraints,) if isinstance(constraints, str) else tuple(constraints)
            unknown = [k for k in names if k not in CONSTRAINTS]
            if unknown:
                raise ValueError('unknown constraint(s) %s; expected some of %s' % (unknown, CONSTRAINTS))
            self.constraints = tuple(k for k in CONSTRAINTS if k in names)
        if self.constraints:
            if self.folds:
                raise ValueError('constraints cannot be combined with folds')
            if not getattr(problem, 'has_annual', False):
                raise ValueError('constraints need a problem bound with annual_precip '
                                 '(MOD16._et_bind(..., annual_precip=(years, precip)))')
        groups = len(self.folds) if self.folds else 1
        if self.chains * groups > problem.max_draws:
            raise ValueError('%d chains x %d fold(s), the problem was bound for max_draws = %d'
                             % (self.chains, groups, problem.max_draws))
        x0 = None
        if initial is not None:
            x0 = np.asarray(initial, np.float64)
            if self.folds and x0.shape == (self.chains, d):
                x0 = np.concatenate([x0] * groups)
            elif self.folds and x0.shape == (groups, self.chains, d):
                x0 = x0.reshape(groups * self.chains, d)
            elif self.folds or x0.shape != (self.chains, d):
                raise ValueError('initial must be (chains, %d) = (%d, %d)%s' % (
                    d, self.chains, d, ' or (folds, chains, d)' if self.folds else ''))
            x0 = np.ascontiguousarray(x0)
            for i, name in enumerate(self.names):
                fam, p = self.families[name], self.prior_params[name]
                ok = (x0[:, i] > 0) & np.isfinite(x0[:, i]) if fam == 'lognormal' else (x0[:, i] > p[0]) & (x0[:, i] < p[1])
                if not ok.all():
                    raise ValueError('initial values of %r outside the support of its prior' % name)
        spec = _lib.McmcSpec()
        spec.chains, spec.nfree = self.chains, d
        for i, (j, name, fam, p) in enumerate(free):
            spec.index[i] = j
            spec.family[i] = _FAMILY_CODE[fam]
            spec.p0[i], spec.p1[i], spec.p2[i] = p
        for j in range(11):
            spec.fixed[j] = values[j]
        spec.lamb, spec.scaling = self.lamb, self.scaling
        spec.tune_target = target[key]
        spec.tune_interval = self.tune_interval
        spec.tune_steps = self.tune
        spec.tune_drop_fraction = self.tune_drop_fraction
        spec.objective = OBJECTIVES.index(obj)
        spec.segment = int(segment)
        spec.seed = self.seed
        spec.constraints = _lib.CONSTRAINT_ANNUAL_PRECIP if self.constraints else 0
        self._ctx = problem._ctx
        x0p = x0.ctypes.data if x0 is not None else None
        if self.folds:
            fold_arr = np.array(self.folds, np.int32)
            self._keep = (spec, x0, fold_arr)
            status = self._ctx.lib.mod16_mcmc_create_groups(problem._handle, C.byref(spec), groups,
                                                            fold_arr.ctypes.data, x0p, C.byref(self._handle))
        else:
            self._keep = (spec, x0)
            status = self._ctx.lib.mod16_mcmc_create(problem._handle, C.byref(spec), x0p, C.byref(self._handle))
        if status == _lib.ERR_ARG:
            raise ValueError(self._ctx.lib.mod16_last_error(self._ctx.handle).decode())
        self._ctx.check(status)
        self.steps = 0          # steps taken by every chain, tuning included
        #: GPU milliseconds of the graphs of the last sample() call
        self.last_gpu_ms = 0.0

    @property
    def d(self):
        return len(self.names)

    @property
    def total_chains(self):
        '''Chains in the sampler: ``chains`` x the number of folds.'''
        return self.chains * (len(self.folds) if self.folds else 1)

    def run(self, steps):
        '''``steps`` more steps of every chain (no trace returned); the GPU milliseconds they took.'''
        ms = C.c_float(0)
        self._ctx.check(self._ctx.lib.mod16_mcmc_run(self._handle, int(steps), C.byref(ms)))
        self.steps += int(steps)
        self.last_gpu_ms = ms.value
        return ms.value

    def read(self, t0, count):
        '''Steps [t0, t0 + count) of every chain: (x (count, chains, d), y, loglik (count, chains),
        logpost, accepted, scaling (chains,), lamb).'''
        C_, d = self.total_chains, self.d
        x = np.empty((count, C_, d))
        y = np.empty((count, C_, d))
        ll = np.empty((count, C_))
        lp = np.empty((count, C_))
        acc = np.empty((count, C_), np.uint8)
        sc = np.empty(C_)
        lb = np.empty(C_)
        taken = C.c_int64(0)
        self._ctx.check(self._ctx.lib.mod16_mcmc_read(
            self._handle, int(t0), int(count), x.ctypes.data, y.ctypes.data, ll.ctypes.data, lp.ctypes.data,
            acc.ctypes.data, sc.ctypes.data, lb.ctypes.data, C.byref(taken)))
        return x, y, ll, lp, acc.astype(bool), sc, lb

    def sample(self, draws):
        '''``draws`` more draws of every chain -- tuning first on the first call -- as a ``Trace`` of
        these draws. A later call continues the same chains.'''
        draws = int(draws)
        if draws < 0:
            raise ValueError('draws must be >= 0')
        first = self.tune if self.steps == 0 else 0
        start = self.steps + first
        self.run(first + draws)
        x, _, ll, lp, acc, sc, lb = self.read(start, draws)
        samples = {name: np.ascontiguousarray(x[:, :, i].T) for i, name in enumerate(self.names)}
        args = (self.names, samples, np.ascontiguousarray(ll.T), np.ascontiguousarray(lp.T),
                np.ascontiguousarray(acc.T), sc, lb)
        if not self.folds:
            return Trace(*args)
        return KFoldTrace(*args, chain_fold=np.repeat(self.folds, self.chains),
                          labels=self.problem.labels, nfolds=self.problem.nfolds)

    def rows(self, samples):
        '''Parameter rows (m, 11): the fixed row with the free columns from ``samples`` (m, d).'''
        samples = np.asarray(samples, np.float64).reshape(-1, self.d)
        rows = np.repeat(self.fixed_row[None], samples.shape[0], axis=0)
        for i, name in enumerate(self.names):
            rows[:, PARAM_NAMES.index(name)] = samples[:, i]
        return rows

    def penalty(self, trace, burn=0, thin=1):
        '''The annual-precipitation penalty (chains, k) of every kept draw of ``trace`` (after
        ``burn``, every ``thin``-th), up to ``max_draws`` rows per launch; a problem bound with
        ``annual_precip``, whether or not the sampler ran with ``constraints``.'''
        if not getattr(self.problem, 'has_annual', False):
            raise ValueError('penalty() needs a problem bound with annual_precip')
        post = trace.posterior(burn, thin)
        x = np.stack([post[name] for name in self.names], axis=-1)          # (chains, k, d)
        rows = self.rows(x.reshape(-1, self.d))
        out = np.empty(rows.shape[0])
        step = self.problem.max_draws
        for a in range(0, rows.shape[0], step):
            out[a:a + step] = self.problem.penalty(rows[a:a + step])
        return out.reshape(x.shape[:2])

    def heldout(self, trace, burn=0, thin=1):
        '''Scores a ``KFoldTrace`` of this sampler on the site-days each fold held out:
        ``{f: {'sse', 'count', 'rmsd': (chains, k) of every kept draw (after ``burn``, every
        ``thin``-th), 'mean': the posterior-mean x-values (d,), 'mean_rmsd': the held-out RMSD of
        that row}}``. Every fold's rows are evaluated in HELDOUT mode, up to ``max_draws`` rows (of
        any folds) per launch.'''
        if not self.folds or not isinstance(trace, KFoldTrace):
            raise ValueError('heldout() scores the KFoldTrace of a sampler made with folds')
        post = {f: trace.fold(f).posterior(burn, thin) for f in trace.folds}
        rows, codes, shapes = [], [], {}
        for f in trace.folds:
            x = np.stack([post[f][name] for name in self.names], axis=-1)     # (chains, k, d)
            shapes[f] = x.shape[:2]
            mean = x.reshape(-1, self.d).mean(axis=0) if x.size else np.full(self.d, np.nan)
            rows.append(self.rows(np.concatenate([x.reshape(-1, self.d), mean[None]])))
            codes.append(np.full(rows[-1].shape[0], f))
        rows, codes = np.concatenate(rows), np.concatenate(codes)
        sse, cnt = np.empty(rows.shape[0]), np.empty(rows.shape[0])
        step = self.problem.max_draws
        for a in range(0, rows.shape[0], step):
            sse[a:a + step], cnt[a:a + step] = self.problem.objective(
                rows[a:a + step], folds=codes[a:a + step], heldout=True)
        out, a = {}, 0
        with np.errstate(invalid='ignore', divide='ignore'):
            for f in trace.folds:
                m = shapes[f][0] * shapes[f][1]
                s, c = sse[a:a + m].reshape(shapes[f]), cnt[a:a + m].reshape(shapes[f])
                out[f] = {'sse': s, 'count': c, 'rmsd': np.sqrt(s / c),
                          'mean': rows[a + m, [PARAM_NAMES.index(k) for k in self.names]],
                          'mean_rmsd': float(np.sqrt(sse[a + m] / cnt[a + m]))}
                a += m + 1
        return out

    def close(self):
        '''Frees the sampler. Once its context is destroyed (interpreter teardown can finalise the
        context before the sampler) there is nothing to free through it -- the context's lock went
        with it -- and close() does nothing.'''
        if getattr(self, '_handle', None) is not None and self._handle.value and self._ctx.handle.value:
            self._ctx.lib.mod16_mcmc_destroy(self._handle)
            self._handle.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
