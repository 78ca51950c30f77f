"""Pixels of the mixed-precision form's CANCELLATION CLASS (mod16_amd/csrc/mod16_mixed.hpp,
period_mixed), constructed so that their membership is known on the CPU, and the layouts that put
them where the machinery behind the class has its cases (mod16_stream.hpp: the per-run list of
kCancelCap entries, the ballot group that does not fit, the last flag bit, the table of
et_stream_cancel_kernel, the ragged end). Plain test infrastructure: numpy and ``oracle`` only.

A period's value belongs to the class when the radiative term of the wet canopy's or the bare
soil's numerator, carried through the component's quotient (its *budget*), is negative and exceeds
kMixedCancel = 320 times the period's total: the kernel's test is ``budget + 320 * bracket < 0``
with ``bracket`` = total + (the component as masked - the component before its mask).
``budget_ratio`` evaluates -budget / bracket in float64 from the oracle's building blocks. The
kernel evaluates it in float32, so

    CLASS   a pixel with a ratio of at least 4 x 320  (every float32 evaluation flags it)
    CLEAR   a pixel whose four ratios are all at most 320 / 4  (none does)

and nothing in between is used where a count matters.

The constructed class pixel is the unbounded case, a dry night over bare ground: fPAR = 0 (no
canopy, no transpiration), night relative humidity below 0.7 (no saturated fraction), and a net
longwave radiation a relative ``delta`` above the root at which the night's soil numerator
s A_soil + rho Cp vpd / r_as changes sign: the night total is then about delta times its terms,
and its budget ratio about 1 / delta.
"""
import numpy as np

from oracle import mod16_oracle as oracle
from oracle import synth

LANES, VEC = 64, 4
PIECE = LANES * VEC              # pixels of one piece of a float32 raster
CANCEL_CAP = 32                  # kCancelCap: entries of a run's list
CANCEL_SHIFT = 44                # kCancelShift: piece-flag bits of the dynamic schedule
MIXED_CANCEL = 320.0             # kMixedCancel
MARGIN = 4.0                     # what the float32 evaluation of a budget may be off by, generously
POISON = 0x7fc16a5d              # kCancelPoison
MAX_BISECT = 65536               # pixels bisected per pool at most
CP = oracle.SPECIFIC_HEAT_CAPACITY_AIR


def tables():
    """(13 x 11 table for the engine, the oracle's dict of it)"""
    from mod16_amd.utils import restore_bplut, bplut_table
    from mod16_amd.models import COLLECTION61_BPLUT
    table = bplut_table(restore_bplut(COLLECTION61_BPLUT), beta=250)
    return table, {k: table[:, j] for j, k in enumerate(oracle.PARAM_NAMES)}


def raw_to_drivers(raw, fpar_pct, lai_x10):
    """The 14 pixel-function drivers of raw drivers, as oracle.evapotranspiration_raw forms them."""
    (lw_d, lw_n, sw_d, sw_n, alb, t_d, t_n, t_a, tmin, qv_d, qv_n, ps_d, ps_n, elev) = raw
    with np.errstate(all='ignore'):
        vpd_d = oracle.vpd_from_humidity(qv_d, ps_d, t_d)
        vpd_n = oracle.vpd_from_humidity(qv_n, ps_n, t_n)
        vpd_n = np.where(vpd_n < 0, 0, vpd_n)
        pa = oracle.air_pressure(elev)
        fpar = np.where(fpar_pct >= 249, np.nan, np.asarray(fpar_pct, t_d.dtype)) / 100
        lai = np.where(lai_x10 >= 249, np.nan, np.asarray(lai_x10, t_d.dtype)) / 10
    return [lw_d, lw_n, sw_d, sw_n, alb, t_d, t_n, t_a, tmin, vpd_d, vpd_n, pa, fpar, lai]


def budget_ratio(bplut, cls, drv):
    """float64. Returns (ratio, soil_night): ``ratio`` = the largest -budget / bracket of the four
    budgets of a pixel (day and night, wet canopy and bare soil; 0 where no budget is negative, inf
    where a negative budget meets a bracket <= 0); ``soil_night`` = |s A_soil| / |numerator| of the
    night's bare-soil quotient alone (|s A_soil r_tot| against |numerator|: numerator and radiative term share
    the factor r_tot in the kernel's form of the quotient)."""
    drv = [np.asarray(d, np.float64) for d in drv]
    p = oracle.gather_params(bplut, cls)
    (lw_d, lw_n, sw_d, sw_n, alb, t_d, t_n, t_ann, tmin, vpd_d, vpd_n, pa, fpar, lai) = drv
    worst = np.zeros(drv[0].shape)
    soil_night = None
    with np.errstate(all='ignore'):
        rad_soil = oracle.radiation_soil(p, lw_d, lw_n, sw_d, sw_n, alb, t_d, t_n, t_ann, fpar)
        for i, (t, vpd, sw, lw) in enumerate(((t_d, vpd_d, sw_d, lw_d), (t_n, vpd_n, sw_n, lw_n))):
            rad_canopy = fpar * (sw * (1 - alb) + lw)
            rh = oracle.rhumidity(t, vpd)
            fw = oracle.wet_fraction(rh)
            lhv = oracle.latent_heat_vaporization(t)
            r_corr = oracle.r_correction(pa, t)
            s = oracle.svp_slope(t)
            rho = oracle.air_density(t, pa, rh)
            gamma = oracle.psychrometric_constant(pa, t)
            r_r = oracle.radiative_resistance(rho, t)
            canopy = oracle.evaporation_wet_canopy(p, pa, t, vpd, lai, fpar, rad_canopy, lhv, rh, fw)
            soil = oracle.evaporation_soil(p, pa, t, vpd, fpar, rad_soil[i], r_corr, lhv, rh, fw)
            trans = oracle.transpiration(p, pa, t, vpd, lai, fpar, rad_canopy, tmin, r_corr, lhv, rh, fw,
                                         daytime=(i == 0))
            total = canopy + soil + trans
            # wet canopy (oracle.evaporation_wet_canopy): the value before its masks and its budget;
            # a dry period or a vanishing LAI carries none
            none_c = (fw == 0) | (lai <= oracle.TINY)
            fw_, lai_ = np.where(fw == 0, oracle.TINY, fw), np.where(lai == 0, oracle.TINY, lai)
            r_h, r_e = 1 / (p['gl_sh'] * lai_ * fw_), 1 / (p['gl_wv'] * lai_ * fw_)
            r_a_wet = (r_h * r_r) / (r_h + r_r)
            den_c = (s + (pa * CP * r_e) / (lhv * oracle.MOL_WEIGHT_WET_DRY_RATIO_AIR * r_a_wet)) * lhv
            ev = np.where(none_c, 0, fw_ * (s * rad_canopy + rho * CP * fpar * vpd / r_a_wet) / den_c)
            bud_c = np.where(none_c, 0, fw_ * s * rad_canopy / den_c)
            # bare soil (oracle.potential_soil_evaporation, evaporation_soil)
            r_tot = np.where(vpd <= p['vpd_open'], p['rbl_min'], np.where(
                vpd >= p['vpd_close'], p['rbl_max'],
                p['rbl_max'] - ((p['rbl_max'] - p['rbl_min']) * (p['vpd_close'] - vpd)) / (p['vpd_close'] - p['vpd_open'])))
            r_tot = r_tot / r_corr
            r_as = (r_tot * r_r) / (r_tot + r_r)
            num_s = s * rad_soil[i] + rho * CP * (1 - fpar) * (vpd / r_as)
            den_s = (s + gamma * (r_tot / r_as)) * lhv
            wet = fw + (1 - fw) * np.power(rh, vpd / p['beta'])
            es = num_s * wet / den_s
            bud_s = s * rad_soil[i] * wet / den_s
            for bud, bracket in ((bud_c, total + canopy - ev), (bud_s, total + soil - es)):
                r = np.where(bud < 0, np.where(bracket > 0, -bud / bracket, np.inf), 0.0)
                worst = np.maximum(worst, np.where(np.isnan(r), 0.0, r))
            if i == 1:
                soil_night = np.abs(s * rad_soil[i]) / np.abs(num_s)
    return worst, soil_night


def is_class(bplut, cls, drv):
    ratio, soil_night = budget_ratio(bplut, cls, drv)
    return (soil_night >= MARGIN * MIXED_CANCEL) & (ratio >= MARGIN * MIXED_CANCEL)


def is_clear(bplut, cls, drv):
    ratio, _ = budget_ratio(bplut, cls, drv)
    return ratio <= MIXED_CANCEL / MARGIN


class Pool(object):
    """Unique pixels, float32: ``cls``, ``drv`` (14 drivers, or the 14 raw fields), for raw drivers
    also ``fpar_pct`` / ``lai_x10`` / ``hours``; class pools carry ``delta`` per pixel."""

    def __init__(self, cls, drv, raw=False, fpar_pct=None, lai_x10=None, hours=None, delta=None):
        self.cls, self.drv, self.raw = cls, drv, raw
        self.fpar_pct, self.lai_x10, self.hours, self.delta = fpar_pct, lai_x10, hours, delta

    def __len__(self):
        return self.cls.size

    def take(self, idx):
        opt = lambda a: None if a is None else a[idx]
        return Pool(self.cls[idx], [d[idx] for d in self.drv], self.raw, opt(self.fpar_pct),
                    opt(self.lai_x10), opt(self.hours), opt(self.delta))

    def drivers64(self):
        """the 14 pixel-function drivers in float64 of the (float32) pixels"""
        wide = [d.astype(np.float64) for d in self.drv]
        return raw_to_drivers(wide, self.fpar_pct, self.lai_x10) if self.raw else wide

    def truth(self, bplut):
        """T: the float64 oracle on the widened float32 inputs -> (day, night[, total8])"""
        wide = [d.astype(np.float64) for d in self.drv]
        with np.errstate(all='ignore'):
            if self.raw:
                return oracle.evapotranspiration_raw(bplut, self.cls, wide, self.fpar_pct, self.lai_x10,
                                                     None if self.hours is None else self.hours.astype(np.float64))
            return oracle.evapotranspiration_raster(bplut, self.cls, *wide)

    def numpy_float32(self, bplut):
        """the oracle run entirely in float32 (numpy's dtype rule, as fixture F5) -> (day, night)"""
        b32 = {k: np.asarray(v, np.float32) for k, v in bplut.items()}
        with np.errstate(all='ignore'):
            if self.raw:
                return oracle.evapotranspiration_raw(b32, self.cls, self.drv, self.fpar_pct, self.lai_x10)[:2]
            return oracle.evapotranspiration_raster(b32, self.cls, *self.drv)


def _candidates(m, seed, raw):
    """m ordinary synthetic pixels (float64) -> (cls, fields, fpar_pct, lai_x10, hours)"""
    cls, drv = synth.drivers((m,), seed=seed, special=False)
    rng = np.random.default_rng(seed + 1000)
    if not raw:
        return cls, drv, None, None, None
    # raw drivers: the first nine fields pass through; specific humidity from a relative one
    ps_d, ps_n = rng.uniform(70000, 101340, m), rng.uniform(70000, 101340, m)
    rh_d, rh_n = rng.uniform(0.05, 1.0, m), rng.uniform(0.05, 1.0, m)
    qv = lambda rh, t, ps: 0.622 * rh * oracle.svp(t) / (ps - 0.379 * rh * oracle.svp(t))
    fields = drv[:9] + [qv(rh_d, drv[5], ps_d), qv(rh_n, drv[6], ps_n), ps_d, ps_n, rng.uniform(-50, 4500, m)]
    return (cls, fields, rng.integers(1, 90, m).astype(np.uint8), rng.integers(1, 60, m).astype(np.uint8),
            rng.uniform(6, 18, m))


def clear_pool(count, seed=0, raw=False, bplut=None):
    """``count`` ordinary synthetic pixels none of whose budgets comes within a factor 4 of the
    class (about 98 % of the synthetic field are such)."""
    bplut = bplut or tables()[1]
    cls, f, fp, lx, hours = _candidates(int(count * 1.2) + 64, seed, raw)
    pool = Pool(cls, [a.astype(np.float32) for a in f], raw, fp, lx, None if hours is None else hours.astype(np.float32))
    keep = np.flatnonzero(is_clear(bplut, pool.cls, pool.drivers64()))
    assert keep.size >= count, (keep.size, count)
    return pool.take(keep[:count])


def class_pool(count, delta=(2e-5, 1e-4), seed=0, raw=False, bplut=None, steps=60, hold_at=None):
    """``count`` class pixels: dry nights over bare ground whose ``lw_net_night`` lies a relative
    ``delta`` above the root of the night total (``delta``: a (lo, hi) range drawn log-uniformly, or
    an array of ``count`` values). Every pixel returned meets the class condition in float64 on its
    float32 inputs and has a positive, finite night total there (asserted). With ``hold_at`` (the
    ladder) this is asked of the pixels whose delta is at most ``hold_at``; the deltas beyond it
    leave the class by design."""
    bplut = bplut or tables()[1]
    m = MAX_BISECT
    cls, f, fp, lx, hours = _candidates(m, seed + 77, raw)
    rng = np.random.default_rng(seed + 2000)
    f = [a.copy() for a in f]
    rh_n = rng.uniform(0.05, 0.65, m)                  # a dry night: no saturated fraction
    if raw:
        fp = np.zeros(m, np.uint8)                     # bare ground
        e = rh_n * oracle.svp(f[6])
        f[10] = 0.622 * e / (f[12] - 0.379 * e)
    else:
        f[12] = np.zeros(m)
        f[10] = oracle.svp(f[6]) * (1 - rh_n)

    def night(lw, fields=None, sel=slice(None)):
        g = [a[sel] for a in (fields or f)]
        g[1] = lw
        with np.errstate(all='ignore'):
            if raw:
                return oracle.evapotranspiration_raw(bplut, cls[sel], g, fp[sel], lx[sel])[1]
            return oracle.evapotranspiration_raster(bplut, cls[sel], *g)[1]
    lo, hi = np.full(m, -400.0), np.zeros(m)           # the night total is 0 below the root, positive above
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        pos = night(mid) > 0
        hi, lo = np.where(pos, mid, hi), np.where(pos, lo, mid)
    root = hi
    ok = np.flatnonzero((root < -1) & (root > -399))

    def build(sel, dl):
        g = [a[sel].astype(np.float32) for a in f]
        g[1] = (root[sel] * (1 - dl)).astype(np.float32)
        return Pool(cls[sel], g, raw, None if fp is None else fp[sel], None if lx is None else lx[sel],
                    None if hours is None else hours[sel].astype(np.float32), np.asarray(dl, np.float64))

    def member(pool):
        t = pool.truth(bplut)[1]
        return is_class(bplut, pool.cls, pool.drivers64()) & np.isfinite(t) & (t > 0)
    if isinstance(delta, tuple):
        delta = np.exp(rng.uniform(np.log(delta[0]), np.log(delta[1]), count))
    delta = np.asarray(delta, np.float64)
    assert delta.shape == (count,)
    hold = float(delta.max() if hold_at is None else hold_at)
    assert hold <= 1.0 / (MARGIN * MIXED_CANCEL)
    # the pixels that are members at the largest delta asked of them are members at every smaller one
    keep = ok[np.flatnonzero(member(build(ok, np.full(ok.size, hold))))]
    assert keep.size >= count, (keep.size, count)
    out = build(keep[:count], delta)
    assert member(out)[delta <= hold].all()
    return out


# ---------------------------------------------------------------------------------------------
# Layouts: where the class pixels of a raster sit. The geometry is explicit: a piece is 64 lanes x
# 4 pixels, a run 2^run_shift pieces; lane l of a piece holds its pixels 4 l .. 4 l + 3, and the
# pipeline's loop ballots the pixel PAIRS (4 l, 4 l + 1) and (4 l + 2, 4 l + 3) of a piece's 64
# lanes one after the other -- a ballot GROUP is (piece, pair), 128 pixels.

class Layout(object):
    """``positions``: sorted pixel indices of the class pixels of a raster of ``n`` pixels;
    ``fills``: (pixel, driver, value) triples written over the background afterwards."""

    def __init__(self, name, n, run_shift, positions, fills=()):
        self.name, self.n, self.run_shift = name, int(n), int(run_shift)
        self.positions = np.unique(np.asarray(positions, np.int64))
        assert self.positions.size == np.asarray(positions).size, 'duplicate positions'
        assert self.positions.size == 0 or (0 <= self.positions[0] and self.positions[-1] < n)
        self.fills = list(fills)

    @property
    def run_pixels(self):
        return PIECE << self.run_shift


def coords(positions, run_shift):
    """(run, piece of the run, ballot group of the raster, lane, pixel of the lane)"""
    pos = np.asarray(positions, np.int64)
    piece = pos // PIECE
    return (piece >> run_shift, piece & ((1 << run_shift) - 1), piece * 2 + (pos % VEC) // 2,
            (pos % PIECE) // VEC, pos % VEC)


def simulate(layout, run_shift=None):
    """What the pipeline's loop does with the layout's class pixels under the DYNAMIC schedule, per
    run that holds any: {run: (listed, flagged pixels, sorted flagged pieces of the run)}. Pixels
    behind the last whole vector (the scalar tail) never reach the pipeline."""
    rs = layout.run_shift if run_shift is None else run_shift
    pos = layout.positions[layout.positions < layout.n // VEC * VEC]
    run, piece, group, _, _ = coords(pos, rs)
    out = {}
    groups, first, size = np.unique(group, return_index=True, return_counts=True)
    for g, i, k in zip(groups, first, size):
        listed, flagged, pieces = out.get(int(run[i]), (0, 0, []))
        if listed + k > CANCEL_CAP:
            flagged += int(k)
            if not pieces or pieces[-1] != int(piece[i]):
                pieces = pieces + [int(piece[i])]
        else:
            listed += int(k)
        out[int(run[i])] = (listed, flagged, pieces)
    return out


def _group_members(run_shift, group_of_run, size):
    """``size`` distinct pixels of one ballot group of run 0"""
    piece, pair = divmod(group_of_run, 2)
    m = np.arange(size)
    assert size <= 2 * LANES
    lane = (group_of_run * 11 + m // 2) % LANES
    return piece * PIECE + lane * VEC + pair * 2 + m % 2


def _every_run(name, nruns, run_shift, extra, in_run, fills=()):
    """the same pixels ``in_run`` (offsets from the run's first pixel) in each of ``nruns`` runs"""
    rp = PIECE << run_shift
    in_run = np.asarray(in_run, np.int64)
    pos = (np.arange(nruns, dtype=np.int64)[:, None] * rp + in_run[None, :]).ravel()
    return Layout(name, nruns * rp + extra, run_shift, pos, fills)


def dense(nruns, run_shift, extra=0):
    """every pixel of nruns runs (+ ``extra`` pixels of a partial last run)"""
    n = nruns * (PIECE << run_shift) + extra
    return Layout('dense', n, run_shift, np.arange(n))


def exact_cap(nruns, run_shift, per_run, extra=0, name=None):
    """Exactly ``per_run`` class pixels in every run, spread evenly over its pieces: singles where the
    run has ballot groups enough, else shared among all its groups with a single in the last one -- so
    that 32 fill the list exactly and the 33rd alone does not fit."""
    groups = 2 << run_shift
    m = min(per_run, groups)
    chosen = (np.arange(m) * groups) // m
    sizes = np.full(m - 1, (per_run - 1) // (m - 1))
    sizes[:(per_run - 1) % (m - 1)] += 1
    sizes = list(sizes) + [1]
    in_run = np.concatenate([_group_members(run_shift, int(g), int(k)) for g, k in zip(chosen, sizes)])
    return _every_run(name or 'exact cap %d' % per_run, nruns, run_shift, extra, in_run)


def straddle(nruns, run_shift, extra=0):
    """Per run: 31 entries, as singles where the run has ballot groups enough (run_shift >= 5; a
    shorter run spreads them over all but its last two chosen groups), then a group of 2 (31 + 2 > 32:
    flagged, not listed), then a single that still fits as entry 32."""
    groups = 2 << run_shift
    pre = min(CANCEL_CAP - 1, groups - 2)
    chosen = (np.arange(pre + 2) * groups) // (pre + 2)
    sizes = np.full(pre, (CANCEL_CAP - 1) // pre)
    sizes[:(CANCEL_CAP - 1) % pre] += 1
    sizes = list(sizes) + [2, 1]
    in_run = np.concatenate([_group_members(run_shift, int(g), int(k)) for g, k in zip(chosen, sizes)])
    return _every_run('straddle', nruns, run_shift, extra, in_run)


def high_pieces(nruns, extra=0):
    """Runs of 64 pieces: the list fills in pieces 0-1 (8 entries in each of their four ballot
    groups), the overflow sits only in pieces 44 .. 63 -- beyond the 44 piece-flag bits of the mixed
    forms, reached only through the last one."""
    rs = 6
    in_run = [_group_members(rs, g, 8) for g in range(4)]
    in_run += [_group_members(rs, 2 * p + p % 2, 1 + (p == 63)) for p in range(CANCEL_SHIFT, 64)]
    return _every_run('high pieces', nruns, rs, extra, np.concatenate(in_run))


def full_table(run_shift, one_more=False):
    """64 consecutive runs with 32 entries each: 2048 entries, the table of et_stream_cancel_kernel
    exactly, worked off in 32 batches; ``one_more``: a 65th run, the wave's next batch of runs"""
    return exact_cap(65 if one_more else 64, run_shift, CANCEL_CAP, name='full table' + (' + 1' if one_more else ''))


def ragged_end(n, run_shift):
    """Class pixels in the last full piece, the ragged last piece (first and last vector), the last
    4-pixel vector and the scalar tail behind it (n % 4 pixels, which run FAST)."""
    nvec = n // VEC
    nfull, nrem = nvec // LANES, nvec % LANES
    pos = set(range(nvec * VEC, n))                                        # the scalar tail
    if nvec:
        pos |= {nvec * VEC - 1, nvec * VEC - 3}                            # the last vector
    if nfull:
        base = (nfull - 1) * PIECE
        pos |= {base, base + 5, base + 126, base + 127, base + PIECE - 2}  # the last full piece
    if nrem:
        pos |= {nfull * PIECE + 1, nfull * PIECE + 2}                      # first vector of the ragged piece
    return Layout('ragged end', n, run_shift, sorted(pos))


def mixed_company(nruns, run_shift, fill, extra=0):
    """Per run three class pixels, each with an out-of-domain neighbour -- ``fill`` in its day
    temperature -- in its pair, in its lane's other pair, in another lane of its piece; and a fourth
    with a NaN driver (LAI) in the pixel beside it."""
    rp = PIECE << run_shift
    pos, fills = [], []
    for r in range(nruns):
        b = r * rp + ((r * 3) % (1 << run_shift)) * PIECE + ((r * 7) % 56) * VEC
        pos += [b, b + 4 + 1, b + 8 + 2, b + 12 + 3]
        fills += [(b + 1, 5, fill), (b + 4 + 3, 5, fill), (b + 8 + 2 + 4 * 3, 5, fill), (b + 12 + 2, 13, np.nan)]
    return Layout('mixed company', nruns * rp + extra, run_shift, pos, fills)


def scattered(n, run_shift, count, seed=0, name='ladder'):
    """``count`` class pixels at random places of n pixels"""
    rng = np.random.default_rng(seed)
    pos = np.unique(rng.integers(0, n, count + count // 8 + 16))
    assert pos.size >= count
    return Layout(name, n, run_shift, np.sort(rng.permutation(pos)[:count]))


def ladder_deltas(per_decade, lo=-5, hi=-1, seed=0):
    """log-uniform deltas, ``per_decade`` in each decade of [10^lo, 10^hi), shuffled"""
    rng = np.random.default_rng(seed)
    d = np.concatenate([10.0 ** rng.uniform(e, e + 1, per_decade) for e in range(lo, hi)])
    return rng.permutation(d)


def sources(layout, n_class, n_clear, seed=0, in_order=False):
    """Which pool pixel every pixel of the raster is a copy of: (index into the clear pool per
    pixel, index into the class pool per class position). ``in_order``: class position k takes class
    pixel k (the ladder: every delta once)."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, n_clear, layout.n).astype(np.int64)
    if in_order:
        assert layout.positions.size <= n_class
        src = np.arange(layout.positions.size, dtype=np.int64)
    else:
        src = rng.integers(0, n_class, layout.positions.size).astype(np.int64)
    return bg, src
