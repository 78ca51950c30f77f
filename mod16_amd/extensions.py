'''
The extension entry points of the numpy surface -- what the reference package does not have: the
ensemble forward run and its quantiles, multi-day composites, the downscaled forward run, gap
filling and smoothing of the 8-day series, zonal statistics and the forward run on raw drivers. numpy
in, numpy out, as ``evapotranspiration_raster``; ``mod16_amd`` re-exports every name here. The
definitions they are checked against live in ``mod16_amd.composite``, ``.downscale``, ``.gapfill``,
``.smooth``, ``.zonal`` and ``.calibration``; the argument rules they share with the package root in ``mod16_amd._args``.
'''
import collections as _collections

import numpy as np

from . import _lib
from ._args import (_U16, _as_uint8, _broadcast, _check_stage_bytes, _marshal, _named_outputs, _outputs, _result_dtype,
                    _shape, _shift, _zonal_inputs)
from .downscale import MET_DRIVERS as _MET_DRIVERS


EnsembleET = _collections.namedtuple('EnsembleET', 'mean_day mean_night std_day std_night std_total')


def _ensemble_stack(tables, beta=None):
    '''``tables`` of the ensemble entry points -> float64 (D, 13, 11): a (D, 13, 11) array, or a
    sequence of D ``restore_bplut`` dicts; ``beta`` fills the ``beta`` column where a table has none.'''
    from .utils import bplut_table
    if isinstance(tables, np.ndarray) or not len(tables) or not isinstance(tables[0], dict):
        stack = np.array(tables, np.float64)
        if stack.ndim != 3 or stack.shape[1:] != (_lib.N_CLASSES, _lib.N_PARAMS):
            raise ValueError('tables must have shape (members, 13, 11), got %r' % (stack.shape,))
        if beta is not None:
            fill = np.isnan(stack[:, :, 10]) & ~np.isnan(stack[:, :, 0])
            stack[:, :, 10][fill] = beta
        return stack
    return np.stack([bplut_table(t, beta=beta) for t in tables])


def evapotranspiration_ensemble(
        tables, cls, lw_net_day, lw_net_night, sw_rad_day, sw_rad_night,
        sw_albedo, temp_day, temp_night, temp_annual, tmin, vpd_day,
        vpd_night, pressure, fpar, lai, beta=None, math=_lib.MATH_FAST, device=0, out=None):
    r'''
    (Extension.) Forward run of an ENSEMBLE of parameter tables over a multi-class raster: what a
    loop over ``evapotranspiration_raster(tables[m], cls, *drivers)`` followed by ``np.mean`` /
    ``np.std`` over the members returns, from one kernel that reads each pixel's drivers once,
    evaluates every member and keeps only the running sums (``mod16_et_ensemble_*``): the posterior
    of a calibration (``mod16_amd.calibration.ensemble_tables``) as an ET map with its parameter
    uncertainty.

    Parameters
    ----------
    tables : numpy.ndarray or sequence of dict
        (D, 13, 11) parameter tables (``MOD16.required_parameters`` column order), or D dicts as
        ``restore_bplut`` returns them; 1 <= D <= 65536
    cls : numpy.ndarray
        Class raster as for ``evapotranspiration_raster``: a pixel's class picks its row in EVERY
        table; codes without parameters give NaN, a code >= 13 raises IndexError
    beta : float
        (Optional) value for the ``beta`` column where a table has none
    math : int
        ``MATH_FAST`` (default) or ``MATH_EXACT``; the mixed and the trusted forms are refused
    out : sequence of numpy.ndarray
        (Optional) the five output arrays to write into

    Returns
    -------
    EnsembleET
        ``(mean_day, mean_night, std_day, std_night, std_total)`` [kg m-2 s-1]: mean and standard
        deviation (``ddof = 0``) over the members of the day and night totals, and the standard
        deviation of their sum (whose mean is ``mean_day + mean_night``). float32 only if every
        driver array is float32 (computed in float64, rounded once). A NaN in any member makes that
        period's mean and spread NaN. Pixels broadcast as in numpy; scalars stay scalars.
    '''
    stack = _ensemble_stack(tables, beta)
    drivers = (
        lw_net_day, lw_net_night, sw_rad_day, sw_rad_night, sw_albedo,
        temp_day, temp_night, temp_annual, tmin, vpd_day, vpd_night,
        pressure, fpar, lai)
    dtype = _result_dtype(drivers)
    cls = _as_uint8(cls)
    shape, n = _broadcast([_shape(v) for v in drivers] + [cls.shape])
    keep, dptr, dstride = _marshal(drivers, shape, dtype)
    cls = np.ascontiguousarray(np.broadcast_to(cls, shape))
    outs = _outputs(out, shape, [dtype] * 5)
    ens = _lib.Ensemble(_lib.context(device), stack)
    try:
        if n:
            ens.run(dtype, cls.ctypes.data, dptr, dstride, n, [o.ctypes.data for o in outs],
                    flags=math, where=_lib.HOST)
    finally:
        ens.close()
    if not shape:
        outs = [o[()] for o in outs]
    return EnsembleET(*outs)


CompositeET = _collections.namedtuple('CompositeET', 'et count')
CompositeETPET = _collections.namedtuple('CompositeETPET', 'et pet count_et count_pet')


def evapotranspiration_composite(
        bplut, cls, lw_net_day, lw_net_night, sw_rad_day, sw_rad_night,
        sw_albedo, temp_day, temp_night, temp_annual, tmin, vpd_day,
        vpd_night, pressure, fpar, lai, day_hours, days=None, period_days=8, every=None,
        pet=False, min_valid=1, rescale=False, beta=None, math=_lib.MATH_FAST, device=0, out=None,
        stage_bytes=None):
    r'''
    (Extension.) Multi-day ET composites over a multi-class raster: per-pixel totals of ET over
    periods of ``period_days`` days [kg m-2 per period], what a loop over
    ``evapotranspiration_raster`` per day, ``(day * hours + night * (24 - hours)) * 3600`` and a masked
    sum return -- MOD16A2 is ``period_days=8``, MOD16A3 the days of the year -- from one kernel that
    walks the days of a period per pixel and keeps the sums in registers
    (``mod16_et_composite_*``). The definition is ``mod16_amd.composite`` (``daily_total``,
    ``composite_reduce``).

    Parameters
    ----------
    bplut, beta
        as for ``evapotranspiration_raster``
    cls : numpy.ndarray
        Class raster; its shape is the pixel shape
    the 14 drivers, day_hours
        each a scalar, an array of the pixel shape (constant in time) or an array with one more
        leading axis: its time axis, ``S = ceil(days / every[name])`` slabs of the pixel shape
        (day ``t`` reads slab ``t // every[name]``). ``day_hours`` are the hours of daylight.
    days : int
        1 to 4096 (Default: the slabs of an array with a time axis whose divisor is 1)
    period_days : int
        days per period; the last period may be short
    every : dict
        divisor per array name (``mod16_amd.composite.ARRAY_NAMES``); default 1, daily
    pet : bool
        True to return the potential-ET composite as well
    min_valid : int
        a period with fewer valid days (daily total not NaN) is NaN; 1 to ``period_days``
    rescale : bool
        True to multiply a period's sum by ``len / count``
    math : int
        ``MATH_FAST`` (default) or ``MATH_EXACT``
    out : sequence of numpy.ndarray
        (Optional) the 2 (``pet``: 4) arrays ``(P,) + shape`` to write into
    stage_bytes : int
        (Optional) device memory a staging slot may take (default 128 MiB); the result does not
        depend on it

    Returns
    -------
    CompositeET or CompositeETPET
        ``(et, count)`` or ``(et, pet, count_et, count_pet)``, each ``(P,) + shape`` with ``P =
        ceil(days / period_days)``; counts are uint16. float32 only if every array input is float32
        (computed in float64, rounded once).
    '''
    from . import composite as _c
    from .utils import as_bplut_table
    arrays = [lw_net_day, lw_net_night, sw_rad_day, sw_rad_night, sw_albedo,
              temp_day, temp_night, temp_annual, tmin, vpd_day, vpd_night,
              pressure, fpar, lai, day_hours]
    ev = _c.check_every(every)
    cls = np.asarray(cls)
    shape = cls.shape
    n = int(cls.size)
    dtype = _result_dtype(arrays)
    timed = []
    for name, v in zip(_c.ARRAY_NAMES, arrays):
        sh = _shape(v)
        if sh == () or sh == shape:
            timed.append(False)
        elif len(sh) == len(shape) + 1 and tuple(sh[1:]) == tuple(shape):
            timed.append(True)
        else:
            raise ValueError('%s has shape %r: expected a scalar, the pixel shape %r or one more leading (time) axis'
                             % (name, sh, shape))
    if days is None:
        daily = [_shape(v)[0] for name, v, t in zip(_c.ARRAY_NAMES, arrays, timed) if t and ev[name] == 1]
        if not daily:
            raise ValueError('days is required when no array has a daily time axis')
        days = int(daily[0])
    K, L, mv, P = _c.check_periods(days, period_days, min_valid)
    for name, v, t in zip(_c.ARRAY_NAMES, arrays, timed):
        if t:
            _c.check_slabs(name, _shape(v)[0], K, ev[name])
    if int(math) & ~_lib.MATH_EXACT:
        raise ValueError('math must be MATH_FAST or MATH_EXACT for the composite run')
    _check_stage_bytes(stage_bytes)
    cls = np.ascontiguousarray(_as_uint8(cls))
    full = (P,) + tuple(shape)
    half = 2 if pet else 1
    outs = _outputs(out, full, [dtype] * half + [_U16] * half, pinned=False, indexed=True)
    table = as_bplut_table(bplut, beta)
    keep, ptrs, pstride, tstride, divisor = [], [], [], [], []
    for name, v, t in zip(_c.ARRAY_NAMES, arrays, timed):
        scalar = _shape(v) == ()
        a = np.array(v, dtype).reshape(1) if scalar else np.ascontiguousarray(v, dtype)
        keep.append(a)
        pstride.append(0 if scalar else 1)
        ptrs.append(a.ctypes.data)
        tstride.append(n if t and a.shape[0] > 1 else 0)
        divisor.append(ev[name] if t else K)
    if n:
        ctx = _lib.context(device)
        ctx.set_bplut(table)
        optr = [o.ctypes.data for o in outs]
        et, pt = (optr[0], optr[1]) if pet else (optr[0], None)
        c_et, c_pt = (optr[2], optr[3]) if pet else (optr[1], None)
        ctx.composite(dtype, n, K, L, cls.ctypes.data, ptrs, pstride, tstride, divisor, et, pt, c_et, c_pt, n,
                      min_valid=mv, rescale=rescale, flags=math, where=_lib.HOST, stage_bytes=stage_bytes)
    return (CompositeETPET if pet else CompositeET)(*outs)


def evapotranspiration_downscaled(
        bplut, cls, lw_net_day, lw_net_night, sw_rad_day, sw_rad_night,
        sw_albedo, temp_day, temp_night, temp_annual, tmin, vpd_day,
        vpd_night, pressure, fpar, lai, row_pos, col_pos, wrap=False, method='bilinear',
        coarse=_MET_DRIVERS, beta=None, math=_lib.MATH_FAST, device=0, out=None, devices=None, col_affine=None):
    r'''
    (Extension.) Forward run over a multi-class raster whose reanalysis drivers stay on their own
    coarse grid: what ``evapotranspiration_raster`` returns on drivers blown up to the fine grid
    with ``mod16_amd.downscale.interpolate``, bit for bit, without those fine arrays ever existing --
    the kernel interpolates the four surrounding cells per pixel (``mod16_et_downscaled_*``). The
    definition is ``mod16_amd.downscale`` (``corner_tables``, ``interpolate``).

    Parameters
    ----------
    bplut, beta
        as for ``evapotranspiration_raster``
    cls : numpy.ndarray
        ``(R, C)`` class raster: the fine grid
    the 14 drivers
        a driver named in ``coarse`` is an ``(H, W)`` array on the coarse grid, one grid for all of
        them; any other is an ``(R, C)`` array or a scalar
    row_pos, col_pos : numpy.ndarray
        ``(R,)`` and ``(C,)``: the position of every fine row and column in units of coarse cells,
        cell centres at the integers (``mod16_amd.downscale.positions`` for regular grids)
    col_affine : tuple of numpy.ndarray
        (Optional) ``(col_origin, col_scale)``, each ``(R,)``, in place of ``col_pos`` (pass
        ``col_pos=None``): row-affine columns, the column position of pixel ``(r, c)`` being
        ``col_origin[r] + col_scale[r] * c`` (a MODIS sinusoidal tile:
        ``mod16_amd.downscale.sinusoidal_positions``; ``'nearest'`` or ``'bilinear'``). The result is
        then that on drivers materialised with ``mod16_amd.downscale.interpolate_rows``
    wrap : bool
        True where the coarse column axis is periodic (the longitude axis of a global grid);
        otherwise, and always for the rows, the edge value is held outside the grid
    method : str
        ``'nearest'``, ``'bilinear'`` (default) or ``'cos4'`` (a separable cosine-to-the-fourth
        weighting; see ``mod16_amd.downscale.corner_tables`` for what it is not)
    coarse : sequence of str
        the names of the coarse drivers (Default: ``mod16_amd.downscale.MET_DRIVERS``, the eleven
        reanalysis fields; albedo, fPAR and LAI are fine-grid data)
    math : int
        ``MATH_FAST`` (default) or ``MATH_EXACT``
    out : sequence of numpy.ndarray
        (Optional) the two ``(R, C)`` arrays to write into
    devices : sequence of int
        (Optional) several GPUs behind this call: ranges of whole rows dealt over the listed devices
        (``mod16_amd.multi``), every device with its own copy of the coarse arrays; the same bits
        whatever the list

    Returns
    -------
    tuple
        ``(day, night)`` [kg m-2 s-1], each ``(R, C)``; float32 only if every array input is float32
        (interpolated and computed in float64, rounded once). A NaN coarse cell gives NaN at the
        pixels where it has weight; a class code >= 13 raises IndexError.
    '''
    from . import downscale as _d, multi
    from .utils import as_bplut_table
    arrays = [lw_net_day, lw_net_night, sw_rad_day, sw_rad_night, sw_albedo,
              temp_day, temp_night, temp_annual, tmin, vpd_day, vpd_night,
              pressure, fpar, lai]
    devs = multi.device_list(devices)
    names = _d.check_coarse(coarse)
    cls = np.asarray(cls)
    if cls.ndim != 2:
        raise ValueError('cls must be an (R, C) raster, got shape %r' % (cls.shape,))
    shape = cls.shape
    coarse_shape = (1, 1)
    for name, v in zip(_d.DRIVER_NAMES, arrays):
        if name in names:
            coarse_shape = _shape(v)
            break
    if len(coarse_shape) != 2:
        raise ValueError('a coarse driver must be an (H, W) array, got shape %r' % (coarse_shape,))
    if int(math) & ~_lib.MATH_EXACT:
        raise ValueError('math must be MATH_FAST or MATH_EXACT for the downscaled run')
    shapes = [_shape(v) if name in names or np.size(v) != 1 else () for name, v in zip(_d.DRIVER_NAMES, arrays)]
    if (col_pos is None) == (col_affine is None):
        raise ValueError('exactly one of col_pos and col_affine must be given')
    kinds, _, n = _d.check_call(shape, coarse_shape, shapes, coarse=names, method=method, cls_size=cls.size,
                                row_pos=row_pos, col_pos=col_pos)
    if col_affine is not None:
        col_affine = _d.check_affine(shape, col_affine[0], col_affine[1], method)
    row_tables = _d.corner_tables(row_pos, coarse_shape[0], False, method)
    col_tables = None if col_affine is not None else _d.corner_tables(col_pos, coarse_shape[1], bool(wrap), method)
    geometry = {} if col_affine is None else {'col_affine': col_affine}       # (rectilinear calls are made as before)
    dtype = _result_dtype(arrays)
    cls = np.ascontiguousarray(_as_uint8(cls))
    outs = _outputs(out, shape, [dtype] * 2)
    table = as_bplut_table(bplut, beta)
    keep, ptrs = [], []
    for v, kind in zip(arrays, kinds):
        a = np.array(v, dtype).reshape(1) if kind == _d.KIND_SCALAR else np.ascontiguousarray(v, dtype)
        keep.append(a)
        ptrs.append(a.ctypes.data)
    esz = dtype.itemsize
    optr = [o.ctypes.data for o in outs]

    def part(ctx, off, m):
        '''pixels [off, off + m) on the calling thread's context'''
        ctx.set_bplut(table)
        if m <= 0:
            return
        grid = _lib.Downscale(ctx, shape, coarse_shape, row_pos, col_pos, wrap=wrap, method=method,
                              tables=(row_tables, col_tables), **geometry)
        try:
            d = [p + off * esz if kind == _d.KIND_FINE else p for p, kind in zip(ptrs, kinds)]
            grid.run(dtype, cls.ctypes.data + off, d, kinds, coarse_shape[1], off, m, optr[0] + off * esz,
                     optr[1] + off * esz, flags=math, where=_lib.HOST)
        finally:
            grid.close()

    multi.deal(devs, device, n, part, unit=shape[1])        # whole rows per device
    return (outs[0], outs[1])


def evapotranspiration_composite_downscaled(
        bplut, cls, lw_net_day, lw_net_night, sw_rad_day, sw_rad_night,
        sw_albedo, temp_day, temp_night, temp_annual, tmin, vpd_day,
        vpd_night, pressure, fpar, lai, day_hours, row_pos, col_pos, days=None, period_days=8, every=None,
        wrap=False, method='bilinear', coarse=_MET_DRIVERS, pet=False, min_valid=1, rescale=False, beta=None,
        math=_lib.MATH_FAST, device=0, out=None, stage_bytes=None, col_affine=None):
    r'''
    (Extension.) Multi-day ET composites over a multi-class raster whose reanalysis drivers stay on
    their own coarse grid: what ``evapotranspiration_composite`` returns on arrays blown up to the
    fine grid slab by slab with ``mod16_amd.downscale.interpolate``, bit for bit, counts included,
    without those arrays ever existing -- a year of daily reanalysis is 11 x 365 coarse planes, not
    88 bytes per pixel and day (``mod16_et_composite_downscaled_*``). The definitions are
    ``mod16_amd.composite`` and ``mod16_amd.downscale``.

    Parameters
    ----------
    bplut, beta
        as for ``evapotranspiration_raster``
    cls : numpy.ndarray
        ``(R, C)`` class raster: the fine grid
    the 14 drivers, day_hours
        an array named in ``coarse`` is an ``(H, W)`` array on the coarse grid (constant in time) or
        an ``(S, H, W)`` array, one grid for all of them; any other is a scalar, an ``(R, C)`` array
        or an ``(S, R, C)`` array. ``S = ceil(days / every[name])``: day ``t`` reads slab
        ``t // every[name]``
    row_pos, col_pos, wrap, method, col_affine
        the geometry, as for ``evapotranspiration_downscaled`` (``col_pos=None`` with ``col_affine``)
    days, period_days, every, pet, min_valid, rescale
        as for ``evapotranspiration_composite``
    coarse : sequence of str
        the names of the coarse arrays (Default: ``mod16_amd.downscale.MET_DRIVERS``);
        ``'day_hours'`` may be among them
    math : int
        ``MATH_FAST`` (default) or ``MATH_EXACT``
    out : sequence of numpy.ndarray
        (Optional) the 2 (``pet``: 4) arrays ``(P, R, C)`` to write into
    stage_bytes : int
        (Optional) device memory a staging slot of the fine arrays may take (default 128 MiB); the
        result does not depend on it. The coarse arrays are uploaded whole, once

    Returns
    -------
    CompositeET or CompositeETPET
        ``(et, count)`` or ``(et, pet, count_et, count_pet)``, each ``(P, R, C)`` with ``P =
        ceil(days / period_days)``; counts are uint16. float32 only if every array input is float32
        (interpolated, computed and summed in float64, rounded once). A NaN coarse cell makes that
        day invalid at the pixels where the cell has weight; a class code >= 13 raises IndexError.
    '''
    from . import composite as _c, downscale as _d
    from .utils import as_bplut_table
    arrays = [lw_net_day, lw_net_night, sw_rad_day, sw_rad_night, sw_albedo,
              temp_day, temp_night, temp_annual, tmin, vpd_day, vpd_night,
              pressure, fpar, lai, day_hours]
    ev = _c.check_every(every)
    names = _d.check_coarse_arrays(coarse)
    _d.method_code(method)
    cls = np.asarray(cls)
    if cls.ndim != 2:
        raise ValueError('cls must be an (R, C) raster, got shape %r' % (cls.shape,))
    shape = cls.shape
    shapes = [_shape(v) if name in names or np.size(v) != 1 else () for name, v in zip(_c.ARRAY_NAMES, arrays)]
    coarse_shape = _d.coarse_grid_shape(names, shapes)
    if (col_pos is None) == (col_affine is None):
        raise ValueError('exactly one of col_pos and col_affine must be given')
    for pos, count, what in ((row_pos, shape[0], 'row_pos'), (col_pos, shape[1], 'col_pos')):
        if pos is not None and np.shape(pos) != (count,):
            raise ValueError('%s has shape %r, expected (%d,)' % (what, np.shape(pos), count))
    if col_affine is not None:
        col_affine = _d.check_affine(shape, col_affine[0], col_affine[1], method)
    if days is None:
        daily = [sh[0] for name, sh in zip(_c.ARRAY_NAMES, shapes)
                 if ev[name] == 1 and len(sh) == 3 and (name in names or tuple(sh[1:]) == tuple(shape))]
        if not daily:
            raise ValueError('days is required when no array has a daily time axis')
        days = int(daily[0])
    K, L, mv, P = _c.check_periods(days, period_days, min_valid)
    kinds, slabs, _, n = _d.check_composite_call(shape, coarse_shape, shapes, K, ev, coarse=names, cls_size=cls.size)
    if int(math) & ~_lib.MATH_EXACT:
        raise ValueError('math must be MATH_FAST or MATH_EXACT for the composite run')
    _check_stage_bytes(stage_bytes)
    row_tables = _d.corner_tables(row_pos, coarse_shape[0], False, method)
    col_tables = None if col_affine is not None else _d.corner_tables(col_pos, coarse_shape[1], bool(wrap), method)
    geometry = {} if col_affine is None else {'col_affine': col_affine}       # (rectilinear calls are made as before)
    dtype = _result_dtype(arrays)
    cls = np.ascontiguousarray(_as_uint8(cls))
    full = (P,) + tuple(shape)
    half = 2 if pet else 1
    outs = _outputs(out, full, [dtype] * half + [_U16] * half, pinned=False, indexed=True)
    table = as_bplut_table(bplut, beta)
    plane = coarse_shape[0] * coarse_shape[1]
    keep, ptrs, pstride, tstride, divisor = [], [], [], [], []
    for name, v, kind, S in zip(_c.ARRAY_NAMES, arrays, kinds, slabs):
        a = np.array(v, dtype).reshape(1) if kind == _d.KIND_SCALAR else np.ascontiguousarray(v, dtype)
        keep.append(a)
        ptrs.append(a.ctypes.data)
        pstride.append(1 if kind in (_d.KIND_FINE, _d.KIND_FINE_TIME) else 0)
        timed = kind in (_d.KIND_FINE_TIME, _d.KIND_COARSE_TIME)
        tstride.append(0 if S <= 1 else plane if kind == _d.KIND_COARSE_TIME else n)
        divisor.append(ev[name] if timed else K)
    ctx = _lib.context(device)
    ctx.set_bplut(table)
    grid = _lib.Downscale(ctx, shape, coarse_shape, row_pos, col_pos, wrap=wrap, method=method,
                          tables=(row_tables, col_tables), **geometry)
    try:
        optr = [o.ctypes.data for o in outs]
        et, pt = (optr[0], optr[1]) if pet else (optr[0], None)
        c_et, c_pt = (optr[2], optr[3]) if pet else (optr[1], None)
        grid.composite(dtype, n, K, L, cls.ctypes.data, ptrs, pstride, tstride, divisor, _d.coarse_mask(names),
                       coarse_shape[1], 0, et, pt, c_et, c_pt, n, min_valid=mv, rescale=rescale, flags=math,
                       where=_lib.HOST, stage_bytes=stage_bytes)
    finally:
        grid.close()
    return (CompositeETPET if pet else CompositeET)(*outs)


def gapfill_series(fields, qc=None, good=None, max_gap=None, fallback=None, dtype='uint8', scale=None,
                   source=False, device=0, stage_bytes=None):
    r'''
    (Extension.) QC-driven temporal gap filling of one to three 8-day byte series (MOD15A2H fPAR /
    LAI codes) in one kernel launch per staged tile (``mod16_gapfill_u8``): unreliable slabs are
    linearly interpolated between the nearest reliable slabs before and after, a gap at either end
    takes the nearest reliable value, and what ``max_gap`` leaves open takes ``fallback`` or stays
    unfilled. The definition is ``mod16_amd.gapfill`` (``reliable``, ``fill_series``, ``encode``).

    Parameters
    ----------
    fields : numpy.ndarray or tuple of up to three
        uint8 codes, each ``(S,) + pixel shape`` with ``1 <= S <= 4096``; codes >= 249 are fill values
    qc : numpy.ndarray
        (Optional) uint8 QC layer of the same shape, shared by the fields
    good : sequence of 256 booleans
        (Optional) which QC bytes are acceptable (Default: ``mod16_amd.gapfill.default_good()``)
    max_gap : int
        (Optional) longest run of unreliable slabs that is interpolated, and the furthest a value is
        held at either end (Default: None, no limit)
    fallback : numpy.ndarray or tuple
        (Optional) one uint8 array of the pixel shape (or None) per field, e.g. a climatology
    dtype : str
        ``'uint8'`` (codes, rounded half up; 255 where unfilled), ``'float32'`` or ``'float64'``
        (``code * scale``; NaN where unfilled)
    scale : float or tuple
        (Optional) per field, float output only: 0.01 and 0.1 turn fPAR and LAI codes into what the
        14-driver entry points take (Default: 1)
    source : bool
        True to return, per field, the bytes that say where each value came from (0 observed,
        1 interpolated, 2 held, 3 fallback, 4 unfilled)
    stage_bytes : int
        (Optional) device memory a staging slot may take; the result does not depend on it

    Returns
    -------
    numpy.ndarray or tuple
        the filled array (a tuple if ``fields`` was one), and with ``source`` a pair ``(filled,
        source)`` of the same structure
    '''
    from . import gapfill as _g
    single = isinstance(fields, np.ndarray) or not isinstance(fields, (tuple, list))
    flds = [np.asarray(f) for f in ([fields] if single else fields)]
    if fallback is not None and (isinstance(fallback, np.ndarray) or not isinstance(fallback, (tuple, list))):
        fallback = [fallback]
    fbs = None if fallback is None else [None if f is None else np.asarray(f) for f in fallback]
    qc = None if qc is None else np.asarray(qc)
    S, shape, table, mg, name, scales = _g.check_series(
        [f.shape for f in flds], None if qc is None else qc.shape, good, max_gap,
        None if fbs is None else [None if f is None else f.shape for f in fbs], dtype, scale)
    for what, arrs in (('fields', flds), ('qc', [qc]), ('fallback', fbs or [])):
        for a in arrs:
            if a is not None and a.dtype != np.uint8:
                raise ValueError('%s must be uint8, got %s' % (what, a.dtype))
    _check_stage_bytes(stage_bytes)
    n = int(np.prod(shape, dtype=np.int64))
    flds = [np.ascontiguousarray(f).reshape(S, n) for f in flds]
    qc = None if qc is None else np.ascontiguousarray(qc).reshape(S, n)
    fbs = None if fbs is None else [None if f is None else np.ascontiguousarray(f).reshape(n) for f in fbs]
    outs = [np.empty((S, n), name) for _ in flds]
    src = np.empty((len(flds), S, n), np.uint8) if source else None
    if n:
        good8 = np.ascontiguousarray(table, np.uint8)
        _lib.context(device).gapfill(
            _g.OUT_TYPES[name], n, S, [f.ctypes.data for f in flds], None if qc is None else qc.ctypes.data,
            good8.ctypes.data, None if fbs is None else [None if f is None else f.ctypes.data for f in fbs],
            [o.ctypes.data for o in outs], None if src is None else src.ctypes.data, n, n, n, n,
            max_gap=mg, scale=scales + [1.0] * (3 - len(scales)), where=_lib.HOST, stage_bytes=stage_bytes)
    full = (S,) + tuple(shape)
    filled = [o.reshape(full) for o in outs]
    filled = filled[0] if single else tuple(filled)
    if not source:
        return filled
    srcs = [src[f].reshape(full) for f in range(len(flds))]
    return filled, (srcs[0] if single else tuple(srcs))


def smooth_series(values, weights=None, qc=None, qc_weight=None, lam=None, order=2, envelope=0, min_valid=3,
                  dtype=None, scale=None, count=False, out=None, device=0, stage_bytes=None):
    r'''
    (Extension.) Whittaker smoothing of an 8-day series (MOD15A2H fPAR / LAI codes, or float values),
    weighted by QC, in one kernel launch per staged tile (``mod16_smooth_*``): per pixel the solution
    ``z`` of ``(W + lam D'D) z = W y`` by a banded factorisation, then ``envelope`` passes that lift the
    fit towards the upper envelope of the weighted values. A slab with zero weight is interpolated by
    the smoother itself, so this step can follow ``gapfill_series`` or take its place. The definition
    is ``mod16_amd.smooth`` (``weights_of``, ``factor``, ``solve``, ``encode``); the result has its bits.

    Parameters
    ----------
    values : numpy.ndarray
        ``(S,) + pixel shape`` with ``1 <= S <= 4096``: uint8 codes (>= 249 are fill values), float32
        or float64 (not finite: missing)
    weights : numpy.ndarray
        (Optional) float32 weights of the same shape; a slab counts where its weight is finite and > 0
    qc : numpy.ndarray
        (Optional, instead of ``weights``) uint8 QC layer of the same shape
    qc_weight : sequence of 256 numbers
        (Optional) the weight of every QC byte, finite and >= 0 (Default: 1 where
        ``mod16_amd.gapfill.default_good()`` holds, else 0; ``mod16_amd.smooth`` shows a graded table)
    lam : float
        the smoothing parameter, finite and > 0
    order : int
        1 or 2, the order of the differences that are penalised (Default: 2)
    envelope : int
        0 ... 8 upper-envelope passes (Default: 0)
    min_valid : int
        a pixel with fewer weighted slabs is left unsmoothed: NaN, or 255, in every slab (Default: 3;
        at least ``order``)
    dtype : str
        (uint8 values only) ``'uint8'`` (Default: codes, rounded half up and clipped to 0 ... 248),
        ``'float32'`` or ``'float64'`` (``z * scale``); float values return their own type
    scale : float
        (Optional) uint8 values with float output only, e.g. 0.01 for fPAR
    count : bool
        True to return a pair ``(smoothed, count)``, ``count`` being the uint16 number of weighted
        slabs of every pixel
    out : numpy.ndarray or sequence
        (Optional) the result arrays, C-contiguous: the smoothed array, and with ``count`` the counts
    stage_bytes : int
        (Optional) device memory a staging slot may take; the result does not depend on it

    Returns
    -------
    numpy.ndarray or tuple
    '''
    from . import smooth as _s
    values = np.asarray(values)
    weights = None if weights is None else np.asarray(weights)
    qc = None if qc is None else np.asarray(qc)
    S, shape, mode, table, lam, order, envelope, min_valid, name, scale = _s.check_call(
        values.shape, values.dtype, None if weights is None else weights.shape, None if qc is None else qc.shape,
        qc_weight, lam, order, envelope, min_valid, dtype, scale)
    if weights is not None and weights.dtype != np.float32:
        raise ValueError('weights must be float32, got %s' % weights.dtype)
    if qc is not None and qc.dtype != np.uint8:
        raise ValueError('qc must be uint8, got %s' % qc.dtype)
    _check_stage_bytes(stage_bytes)
    full = (S,) + tuple(shape)
    if out is not None:
        out = [out] if isinstance(out, np.ndarray) else list(out)
        if len(out) != (2 if count else 1):
            raise ValueError('out must hold %d arrays' % (2 if count else 1))
    smoothed, = _outputs(None if out is None else out[:1], full, [np.dtype(name)], pinned=False, indexed=True)
    cnt = None
    if count:
        cnt = np.empty(tuple(shape), _U16) if out is None else out[1]
        if not (isinstance(cnt, np.ndarray) and cnt.shape == tuple(shape) and cnt.dtype == _U16
                and cnt.flags.c_contiguous and cnt.flags.writeable):
            raise ValueError('out[1] must be a writeable C-contiguous uint16 array of shape %s' % (tuple(shape),))
    n = int(np.prod(shape, dtype=np.int64))
    if n:
        values = np.ascontiguousarray(values).reshape(S, n)
        stack = weights if mode == _s.WEIGHT_STACK else qc if mode == _s.WEIGHT_QC else None
        stack = None if stack is None else np.ascontiguousarray(stack).reshape(S, n)
        table = None if (table is None or qc_weight is None) else np.ascontiguousarray(table, np.float64)
        _lib.context(device).smooth(
            values.dtype, _s.OUT_TYPES[name], n, S, values.ctypes.data, None if stack is None else stack.ctypes.data,
            None if table is None else table.ctypes.data, smoothed.ctypes.data, None if cnt is None else cnt.ctypes.data,
            n, n, n, lam, order=order, envelope=envelope, min_valid=min_valid, weight_mode=mode, scale=scale,
            where=_lib.HOST, stage_bytes=stage_bytes)
    return (smoothed, cnt) if count else smoothed


def regress_series(values, design=None, terms=(), weights=None, min_valid=None, stderr=False, series=None, out=None,
                   device=0, stage_bytes=None):
    r'''
    (Extension.) Per-pixel weighted least squares ``y = X b`` over a stack, in one kernel launch per
    staged tile (``mod16_regress_*``): a harmonic (seasonal) model plus trend over a long 8-day record,
    an OLS trend on more steps than ``trend_series`` takes, or ET regressed per pixel on precipitation,
    net radiation and VPD stacks. Missing values are left out sample by sample. The definition is
    ``mod16_amd.regress`` (``regress``); the result has its bits.

    Parameters
    ----------
    values : numpy.ndarray
        ``(T,) + pixel shape`` with ``1 <= T <= 4096``, float32 or float64; a value that is not finite
        is missing
    design : numpy.ndarray
        (Optional) ``(T, Ks)`` float64, finite: the columns every pixel shares (intercept, time,
        harmonics; ``mod16_amd.regress.harmonic_design`` builds one)
    terms : sequence of numpy.ndarray
        (Optional) ``Kp`` per-pixel predictors of ``values``' shape and dtype; ``1 <= Ks + Kp <= 8``, the
        coefficients come in the order design columns, then terms
    weights : numpy.ndarray
        (Optional) float32 weights of ``values``' shape; a sample counts where its weight is finite
        and > 0
    min_valid : int
        (Optional) a pixel with fewer valid samples is left empty: NaN in every float output (Default:
        ``Ks + Kp + 1``; at least ``Ks + Kp``)
    stderr : bool
        True for the standard errors of the coefficients
    series : str
        (Optional) ``'residuals'`` (NaN where the sample is not valid) or ``'fitted'`` (wherever every
        per-pixel term is finite: with a shared-only design the model-based fill of every slab)
    out : dict
        (Optional) the result arrays by name, C-contiguous: exactly the fields produced
    stage_bytes : int
        (Optional) device memory a staging slot may take; the result does not depend on it

    Returns
    -------
    mod16_amd.regress.Regression
        ``(coef, stderr, rss, tss, r2, count, series)``: ``coef`` and ``stderr`` ``(Ks + Kp,) + pixel
        shape``, ``rss``, ``tss``, ``r2`` of the pixel shape, float64; ``count`` uint16 (the valid
        samples); ``series`` ``(T,) + pixel shape`` in the dtype of ``values``; ``stderr`` and
        ``series`` are None where they are not asked for
    '''
    from . import regress as _r
    values = np.asarray(values)
    terms = [np.asarray(t) for t in terms]
    weights = None if weights is None else np.asarray(weights)
    T, shape, Ks, Kp, min_valid, stderr, code = _r.check_call(
        values.shape, values.dtype, None if design is None else np.shape(design), [t.shape for t in terms],
        [t.dtype for t in terms], None if weights is None else weights.shape, min_valid, stderr, series)
    design = _r.check_design(design, T)
    if weights is not None and weights.dtype != np.float32:
        raise ValueError('weights must be float32, got %s' % weights.dtype)
    _check_stage_bytes(stage_bytes)
    P = Ks + Kp
    outs = _named_outputs(out, _r.output_table(shape, T, P, values.dtype, stderr, code))
    n = int(np.prod(shape, dtype=np.int64))
    if n:
        x = np.ascontiguousarray(values).reshape(T, n)
        cols = [np.ascontiguousarray(t).reshape(T, n) for t in terms]
        w = None if weights is None else np.ascontiguousarray(weights).reshape(T, n)

        def address(k):
            return outs[k].ctypes.data if k in outs else None
        try:
            _lib.context(device).regress(
                values.dtype, n, T, x.ctypes.data, design.ctypes.data if Ks else None, Ks, [c.ctypes.data for c in cols],
                None if w is None else w.ctypes.data, address('coef'), address('stderr'), address('rss'), address('tss'),
                address('r2'), address('count'), address('series'), min_valid=min_valid, series_mode=code, where=_lib.HOST,
                stage_bytes=stage_bytes)
        except _lib.Mod16Error as e:
            raise _lib.overlap_as_value_error(e)
    return _r.Regression(*[outs.get(k) for k in _r.Regression._fields])


def aggregate_daynight(fields, half_day=None, noon=None, offset=None, sw_threshold=None, steps_per_day=24,
                       outputs=None, dtype=None, out=None, device=0, stage_bytes=None):
    r'''
    (Extension.) Hourly reanalysis aggregated into the model's day / night drivers in one kernel
    launch per staged chunk of days (``mod16_daynight_*``): the planes of ``lw_net_day/night``,
    ``sw_rad_day``, ``temp_day/night``, ``tmin``, ``vpd_day/night``, the hours of daylight, the daily mean
    temperature and ``temp_annual`` on the reanalysis grid -- what
    ``evapotranspiration_composite_downscaled`` takes as its coarse arrays. The definition is
    ``mod16_amd.daynight`` (this package's day / night split, not a transcription of the operational
    MOD16 preprocessing).

    Parameters
    ----------
    fields : dict
        the hourly series by name -- ``'t'`` (K), ``'qv'``, ``'ps'`` (Pa), ``'sw'``, ``'lw'``, those the
        requested outputs need -- each ``(D * H, R, W)``, all float32 or all float64; NaN is missing
    half_day, noon, offset : numpy.ndarray
        the float64 tables of ``'solar'`` mode: ``(D, R)`` half day lengths in hours, ``(D,)`` local
        solar noon (Default: 12) and ``(W,)`` longitude / 15 (``mod16_amd.daynight.solar_tables``)
    sw_threshold : float
        (Optional) instead of the tables: a step counts as day where ``sw > sw_threshold``
    steps_per_day : int
        ``H``, 1 ... 48 (Default: 24)
    outputs : sequence of str
        (Optional) names of ``mod16_amd.daynight.OUTPUT_NAMES`` and ``'temp_annual'`` (Default: every one
        the fields given allow)
    dtype : str
        ``'float32'`` or ``'float64'`` (Default: float32 only if the fields are float32)
    out : dict
        (Optional) the result arrays by name, C-contiguous, written in place
    stage_bytes : int
        (Optional) device memory a chunk of days may take; the result does not depend on it

    Returns
    -------
    (DayNight, numpy.ndarray)
        the ``(D, R, W)`` series as a namedtuple and the ``(R, W)`` ``temp_annual``; None where an output
        was not requested. ``sw_rad_night`` is not produced: pass 0.0, as the reference's loader does.
    '''
    from . import daynight as _dn
    flds = {k: np.asarray(v) for k, v in dict(fields).items() if v is not None}
    D, H, R, W, mode, tables, threshold, names = _dn.check_call(
        {k: v.shape for k, v in flds.items()}, steps_per_day, half_day, noon, offset, sw_threshold, outputs)
    in_dtype = _dn.check_dtypes(flds)
    out_dtype = _dn.check_out_dtype(dtype, in_dtype)
    _check_stage_bytes(stage_bytes)
    flds = {k: np.ascontiguousarray(v) for k, v in flds.items()}
    outs = _named_outputs(out, _dn.output_table(names, D, R, W, out_dtype))
    if D and R and W:
        try:
            _lib.context(device).daynight(
                in_dtype, _dn.OUT_TYPES[out_dtype.name], R, W, D, H,
                [flds[f].ctypes.data if f in flds else None for f in _dn.FIELD_NAMES], tables,
                [outs[n].ctypes.data if n in outs else None for n in _dn.OUTPUT_NAMES],
                outs['temp_annual'].ctypes.data if 'temp_annual' in outs else None, W, R * W, W, R * W,
                mode=_dn.MODES[mode], threshold=threshold, where=_lib.HOST, stage_bytes=stage_bytes)
        except _lib.Mod16Error as e:
            raise _lib.overlap_as_value_error(e)
    return _dn.DayNight(*[outs.get(n) for n in _dn.OUTPUT_NAMES]), outs.get('temp_annual')


def trend_series(values, times=None, min_valid=4, alpha=None, device=0, stage_bytes=None):
    r'''
    (Extension.) Per-pixel Mann-Kendall test and Theil-Sen slope over a stack of composites -- twenty
    annual totals of ``evapotranspiration_composite`` per pixel, say -- in one kernel launch per staged
    range of pixels (``mod16_trend_*``): is the pixel's ET rising, by how much per unit of time, and is
    the rise significant. The definition is ``mod16_amd.trend`` (``pixel_trend``), which the result
    equals bit for bit.

    Parameters
    ----------
    values : numpy.ndarray
        ``(Y,) + pixel shape`` with ``2 <= Y <= 64``, float32 or float64; NaN and the infinities are
        missing. A stack ``(Y, P, n)`` -- one trend per 8-day period -- is the same call: the pixel
        shape is ``(P, n)``
    times : sequence of float
        (Optional) ``(Y,)``, finite and strictly increasing (Default: ``arange(Y)``)
    min_valid : int
        (Optional) fewest valid values a trend is computed from, ``2 ... Y`` (Default: 4)
    alpha : float
        (Optional) a level in (0, 0.5] for the slope's confidence interval: 0.05 gives the 95 %
        interval, and ``abs(z) > NormalDist().inv_cdf(1 - alpha / 2)`` is the test at that level
    stage_bytes : int
        (Optional) device memory a staging slot may take; the result does not depend on it

    Returns
    -------
    mod16_amd.trend.Trend
        ``(slope, intercept, slope_lo, slope_hi, s, z, count)`` of the pixel shape: float64, ``s``
        int32, ``count`` uint8 (the valid values); NaN (``s``: 0) where ``count < min_valid``;
        ``slope_lo`` and ``slope_hi`` are None without ``alpha``
    '''
    from . import trend as _tr
    values = np.asarray(values)
    dtype = _tr.check_dtype(values.dtype)
    Y, shape, t, min_valid, zq = _tr.check_call(values.shape, times, min_valid, alpha)
    _check_stage_bytes(stage_bytes)
    n = int(np.prod(shape, dtype=np.int64))
    x = np.ascontiguousarray(values).reshape(Y, n)
    outs = _named_outputs(None, _tr.output_table(shape, zq))          # (of the pixel shape: each is n values in a row)
    if n:
        _lib.context(device).trend(
            dtype, n, Y, x.ctypes.data, t, [outs[k].ctypes.data if k in outs else None for k in _tr.FLOAT_NAMES],
            outs['s'].ctypes.data, outs['count'].ctypes.data, time_stride=n, min_valid=min_valid, zq=zq, where=_lib.HOST,
            stage_bytes=stage_bytes)
    return _tr.Trend(*[outs.get(k) for k in _tr.Trend._fields])


def anomaly_series(num, den=None, periods=None, window=1, baseline=None, min_valid=3, outputs=('z',), device=0,
                   stage_bytes=None):
    r'''
    (Extension.) Per-pixel climatology, standardized anomalies and percentile ranks over a record of
    composites -- 24 years of 46 8-day ET and PET totals of ``evapotranspiration_composite`` per pixel,
    say -- in one kernel launch per staged range of pixels (``mod16_anomaly_*``): how unusual is this
    period of this year against the same period of the baseline years. The definition is
    ``mod16_amd.anomaly`` (``anomaly``), which the result equals bit for bit.

    Parameters
    ----------
    num : numpy.ndarray
        ``(S,) + pixel shape`` with ``S = Y * periods`` slabs in time order, years outermost,
        ``2 <= Y <= 64`` and ``S <= 4096``, float32 or float64; NaN and the infinities are missing
    den : numpy.ndarray
        (Optional) the same shape and dtype: the quantity is the ratio ``num / den`` of the window
        sums (ET / PET); a window whose ``den`` sum is not positive is missing
    periods : int
        periods of a year, ``1 ... 366``
    window : int
        (Optional) periods summed into a value, ``1 ... min(periods, 16)``; windows run across year
        boundaries and the first ``window - 1`` slabs of the record are missing (Default: 1)
    baseline : tuple of int
        (Optional) ``(y0, y1)``: the climatology comes from years ``y0 ... y1 - 1``, at least two
        (Default: all years)
    min_valid : int
        (Optional) fewest valid baseline values a climatology is computed from, ``2 ... y1 - y0``
        (Default: 3)
    outputs : sequence of str
        (Optional) any of ``'z'``, ``'pct'``, ``'mean'``, ``'std'``, ``'count'`` (Default: ``('z',)``)
    stage_bytes : int
        (Optional) device memory a staging slot may take; the result does not depend on it

    Returns
    -------
    mod16_amd.anomaly.Anomaly
        ``(z, pct, mean, std, count)``, None for what ``outputs`` does not name: ``z`` and ``pct``
        ``(S,) + pixel shape`` in the dtype of ``num``, ``mean`` and ``std`` ``(periods,) + pixel
        shape`` float64, ``count`` likewise uint8 (the valid baseline values)
    '''
    from . import anomaly as _an
    num = np.asarray(num)
    if den is not None:
        den = np.asarray(den)
        _an.check_den_shape(num.shape, den.shape)
    dtype = _an.check_dtype(num.dtype, None if den is None else den.dtype)
    Y, P, shape, W, (y0, y1), min_valid = _an.check_call(num.shape, periods, window, baseline, min_valid)
    names = _an.check_outputs(outputs)
    _check_stage_bytes(stage_bytes)
    S = Y * P
    n = int(np.prod(shape, dtype=np.int64))
    x = np.ascontiguousarray(num).reshape(S, n)
    d = None if den is None else np.ascontiguousarray(den).reshape(S, n)
    outs = _named_outputs(None, _an.output_table(names, S, P, shape, dtype))
    if n:
        _lib.context(device).anomaly(
            dtype, n, Y, P, x.ctypes.data, None if d is None else d.ctypes.data,
            *[outs[k].ctypes.data if k in outs else None for k in _an.OUTPUT_NAMES], window=W, base_first=y0, base_end=y1,
            min_valid=min_valid, where=_lib.HOST, stage_bytes=stage_bytes)
    return _an.Anomaly(*[outs.get(k) for k in _an.OUTPUT_NAMES])


def _upscale_handle(shape, coarse_shape, row_pos, col_pos, wrap, area, col_affine, col_range, device):
    '''The checked geometry of a numpy upscaling call -> ``(Upscale handle, (H, W))``.'''
    from . import upscale as _u
    if col_affine is None and col_range is None:
        fine, (H, W), row_runs, col_runs = _u.check_geometry(shape, coarse_shape, row_pos, col_pos, wrap)
        area = _u.check_area(area, shape[0])
        return _lib.Upscale(_lib.context(device), fine, (H, W), wrap=wrap, area=area, runs=(row_runs, col_runs)), (H, W)
    if col_pos is not None or col_affine is None:
        raise ValueError('exactly one of col_pos and col_affine must be given (col_range goes with col_affine)')
    fine, (H, W), row_runs, affine, col_range = _u.check_geometry_rows(shape, coarse_shape, row_pos, col_affine, wrap, col_range)
    area = _u.check_area(area, shape[0])
    return _lib.Upscale(_lib.context(device), fine, (H, W), wrap=wrap, area=area, runs=row_runs, col_affine=affine,
                        col_range=col_range), (H, W)


def upscale_fields(values, coarse_shape, row_pos, col_pos=None, wrap=False, area=None, min_fraction=0.0, outputs=('mean',),
                   device=0, stage_bytes=None, col_affine=None, col_range=None):
    r'''
    (Extension.) Upscaling: the area-weighted mean of the valid fine pixels of every cell of a coarse
    grid -- an ET map onto the 0.5-degree grid of the reanalysis that drove it, say -- with the valid
    fraction and count of every cell (``mod16_upscale_*``). The opposite direction of
    ``evapotranspiration_downscaled``, with the same position tables. The definition is
    ``mod16_amd.upscale`` (``aggregate``), which the result equals bit for bit.

    Parameters
    ----------
    values : numpy.ndarray
        ``(K, R, C)`` or ``(R, C)``, float32 or float64; NaN is missing
    coarse_shape : tuple of int
        ``(H, W)``
    row_pos, col_pos : numpy.ndarray
        ``(R,)`` and ``(C,)``: the positions of the fine rows and columns in units of coarse cells,
        cell centres at the integers (``mod16_amd.downscale.positions``); a pixel belongs to the cell
        its centre lies in, a pixel outside the grid to none
    wrap : bool
        (Optional) the coarse column axis is periodic (a global longitude axis)
    area : numpy.ndarray
        (Optional) ``(R,)``: the weight of a pixel of that fine row, ``cos(latitude)`` say (Default: 1)
    min_fraction : float
        (Optional) the mean is NaN where the valid weight of a cell is below this share of the cell's
    outputs : sequence of str
        (Optional) any of ``'mean'``, ``'fraction'``, ``'count'`` (Default: ``('mean',)``)
    stage_bytes : int
        (Optional) device memory a staged band may take; the result does not depend on it
    col_affine : tuple of numpy.ndarray
        (Optional, instead of ``col_pos``) ``(col_origin, col_scale)``, ``(R,)`` each: row-affine columns,
        a sinusoidal tile (``mod16_amd.downscale.sinusoidal_positions``); the definition is then
        ``mod16_amd.upscale.aggregate_rows``
    col_range : tuple of numpy.ndarray
        (Optional, with ``col_affine``) ``(col_first, col_count)``, ``(R,)`` int32: the columns of every
        fine row that can belong to a cell (``mod16_amd.downscale.sinusoidal_columns``)

    Returns
    -------
    mod16_amd.upscale.Upscaled
        ``(mean, fraction, count)``, None for what ``outputs`` does not name: ``(K, H, W)`` or ``(H,
        W)``, ``mean`` and ``fraction`` in the dtype of ``values``, ``count`` int32
    '''
    from . import upscale as _u
    values = np.asarray(values)
    dtype = _u.check_dtype(values.dtype)
    if values.ndim not in (2, 3):
        raise ValueError('values must have shape (K, R, C) or (R, C), got %r' % (values.shape,))
    shape = tuple(values.shape[-2:])
    K, squeeze = _u.check_layers(values.shape, shape)
    min_fraction = _u.check_min_fraction(min_fraction)
    names = _u.check_outputs(outputs)
    _check_stage_bytes(stage_bytes)
    grid, (H, W) = _upscale_handle(shape, coarse_shape, row_pos, col_pos, wrap, area, col_affine, col_range, device)
    x = np.ascontiguousarray(values).reshape(K, shape[0], shape[1])
    outs = _named_outputs(None, _u.output_table(names, (H, W) if squeeze else (K, H, W), dtype))
    try:
        grid.run(dtype, x.ctypes.data, K, shape[0] * shape[1], shape[1], min_fraction,
                 [(outs[k].ctypes.data, H * W, W) if k in outs else None for k in _u.OUTPUT_NAMES], where=_lib.HOST,
                 stage_bytes=stage_bytes)
    finally:
        grid.close()
    return _u.Upscaled(*[outs.get(k) for k in _u.OUTPUT_NAMES])


def upscale_sums(values, coarse_shape, row_pos, col_pos=None, wrap=False, area=None, outputs=None, device=0,
                 stage_bytes=None, col_affine=None, col_range=None):
    r'''
    (Extension.) ``upscale_fields`` stopped before its divisions (``mod16_upscale_sums_*``; the
    definition is ``mod16_amd.upscale.sums`` / ``sums_rows``): what one raster -- a tile -- contributes
    to the cells of a coarse grid it covers only in part. ``mod16_amd.upscale.merge`` adds the sums of
    several rasters in a fixed order and divides once.

    Parameters
    ----------
    values, coarse_shape, row_pos, col_pos, wrap, area, stage_bytes, col_affine, col_range
        as ``upscale_fields`` takes them
    outputs : sequence of str
        (Optional) any of ``'num'``, ``'den'``, ``'tot'``, ``'count'`` (Default: all four)

    Returns
    -------
    mod16_amd.upscale.UpscaledSums
        ``(num, den, tot, count)``, None for what ``outputs`` does not name: ``(K, H, W)`` or ``(H, W)``,
        float64 whatever the type of ``values``, ``count`` int32
    '''
    from . import upscale as _u
    values = np.asarray(values)
    dtype = _u.check_dtype(values.dtype)
    if values.ndim not in (2, 3):
        raise ValueError('values must have shape (K, R, C) or (R, C), got %r' % (values.shape,))
    shape = tuple(values.shape[-2:])
    K, squeeze = _u.check_layers(values.shape, shape)
    names = _u.check_sum_outputs(_u.SUM_NAMES if outputs is None else outputs)
    _check_stage_bytes(stage_bytes)
    grid, (H, W) = _upscale_handle(shape, coarse_shape, row_pos, col_pos, wrap, area, col_affine, col_range, device)
    x = np.ascontiguousarray(values).reshape(K, shape[0], shape[1])
    outs = _named_outputs(None, _u.sum_table(names, (H, W) if squeeze else (K, H, W)))
    try:
        grid.sums(dtype, x.ctypes.data, K, shape[0] * shape[1], shape[1],
                  [(outs[k].ctypes.data, H * W, W) if k in outs else None for k in _u.SUM_NAMES], where=_lib.HOST,
                  stage_bytes=stage_bytes)
    finally:
        grid.close()
    return _u.UpscaledSums(*[outs.get(k) for k in _u.SUM_NAMES])


def upscale_classes(cls, coarse_shape, row_pos, col_pos=None, wrap=False, valid=None, outputs=('cls',), device=0,
                    stage_bytes=None, col_affine=None, col_range=None):
    r'''
    (Extension.) The dominant class of a class raster per cell of a coarse grid
    (``mod16_upscale_classes``; the definition is ``mod16_amd.upscale.majority``): the class map a coarse
    forward run needs. Per cell the valid code with the most pixels -- the lowest code on a tie --, 255
    where no pixel is valid, and the winner's share of the cell's pixels.

    Parameters
    ----------
    cls : numpy.ndarray
        ``(R, C)`` class codes (uint8, or integers in [0, 255])
    coarse_shape, row_pos, col_pos, wrap, col_affine, col_range
        the geometry, as ``upscale_fields`` takes it (row-affine columns: ``mod16_amd.upscale.majority_rows``)
    valid : iterable of int
        (Optional) the codes that count, each in [0, 32) (Default: 0 ... 12)
    outputs : sequence of str
        (Optional) any of ``'cls'``, ``'share'`` (Default: ``('cls',)``)

    Returns
    -------
    mod16_amd.upscale.UpscaledClasses
        ``(cls, share)``: ``(H, W)`` uint8 and float32, None for what ``outputs`` does not name
    '''
    from . import upscale as _u
    c = _as_uint8(cls)
    if c.ndim != 2:
        raise ValueError('cls must be a two-dimensional class raster, got shape %r' % (c.shape,))
    mask = _u.valid_mask(valid)
    names = _u.check_class_outputs(outputs)
    _check_stage_bytes(stage_bytes)
    grid, (H, W) = _upscale_handle(c.shape, coarse_shape, row_pos, col_pos, wrap, None, col_affine, col_range, device)
    c = np.ascontiguousarray(c)
    outs = _named_outputs(None, _u.output_table(names, (H, W)))
    try:
        grid.classes(c.ctypes.data, c.shape[1], mask, *[(outs[k].ctypes.data, W) if k in outs else None for k in _u.CLASS_OUTPUT_NAMES],
                     where=_lib.HOST, stage_bytes=stage_bytes)
    finally:
        grid.close()
    return _u.UpscaledClasses(*[outs.get(k) for k in _u.CLASS_OUTPUT_NAMES])


def zonal_statistics(values, zones, nzones=None, area=None, bounds=None, acc=None, device=0, stage_bytes=None):
    r'''
    (Extension.) Zonal statistics of a raster: per zone (river basin, country, biome, climate-grid
    cell) and layer (composite period) the exact weighted totals ``sum w``, ``sum w x`` and ``sum w x
    x``, the count, minimum and maximum of the valid pixels, in one pass over the values
    (``mod16_zonal_*``). The sums are order-independent by construction -- every term is quantised
    once to a 62-bit fixed point and added as an integer -- so the result does not depend on
    ``stage_bytes``, on how a raster is cut into calls that accumulate (``acc=``), or on the device
    that ran a part (``ZonalResult.merge``). The definition is ``mod16_amd.zonal`` (``accumulate``).

    Parameters
    ----------
    values : numpy.ndarray
        float32 or float64, ``shape`` or ``(K,) + shape``; NaN masks a pixel
    zones : numpy.ndarray
        integer zone ids of ``shape``; ids outside ``[0, nzones)`` are ignored (uint8, uint16 and
        int32 are taken as they are, other integer types are range-checked and cast to int32)
    nzones : int
        (Optional) the number of zones (Default: ``zones.max() + 1``)
    area : None, float or numpy.ndarray
        (Optional) the weight of a pixel: None (1), a scalar, ``(R,)`` for a 2-D ``shape`` with R
        rows (the area of a latitude row, float64) or an array of ``shape`` (a land fraction; taken
        in the values' dtype); NaN masks a pixel
    bounds : (float, float)
        (Optional) ``(wmax, xmax)``: the largest weight and the largest ``|value|`` the call accepts;
        a pixel beyond them raises ValueError. They fix the fixed-point scale, so calls that are to
        be accumulated or merged must share their exponents (``zonal.exponent``). Default: a
        pre-pass over the inputs finds them (infinities are then counted in ``rejected``)
    acc : ZonalResult
        (Optional) a result to add into (it is not modified); needs ``bounds`` with its exponents
    stage_bytes : int
        (Optional) device memory a staging slot may take; the result does not depend on it

    Returns
    -------
    mod16_amd.zonal.ZonalResult
        ``count``, ``rejected``, ``sum_w``, ``sum_wx``, ``sum_wxx``, ``mean``, ``var``, ``std``,
        ``min``, ``max``, each ``(K, Z)`` (``(Z,)`` for values without a layer axis); ``words``, the
        ``(K, Z, 10)`` int64 accumulator; ``merge(other)``
    '''
    from . import zonal as _z
    values, zones, nzones, layered, kind, cols, weights = _zonal_inputs(values, zones, nzones, area)
    K, n = values.shape
    _check_stage_bytes(stage_bytes)
    explicit = bounds is not None
    if acc is not None:
        if not isinstance(acc, _z.ZonalResult):
            raise ValueError('acc must be a ZonalResult')
        _z.check_acc_bounds(bounds)
        if acc.words.shape != (K, nzones, _z.NWORDS):
            raise ValueError('acc holds %r words, this call needs %r' % (acc.words.shape, (K, nzones, _z.NWORDS)))
    if explicit:
        bounds = _z.check_bounds(bounds)
        if acc is not None and (acc.ew, acc.ex) != bounds[2:]:
            raise ValueError('the exponents of bounds %r differ from the accumulator\'s %r' % (bounds[2:], (acc.ew, acc.ex)))
    wptr = None if weights is None else weights.ctypes.data
    ztype = _z.ZONE_TYPES[zones.dtype.name]
    ctx = _lib.context(device)
    if not explicit:
        wmax, xmax = ctx.zonal_bounds(values.dtype, n, K, values.ctypes.data, wptr, weight_kind=kind, cols=cols,
                                      where=_lib.HOST, stage_bytes=stage_bytes) if n else (1.0, 1.0)
        bounds = _z.check_bounds((wmax if wmax > 0 else 1.0, xmax if xmax > 0 else 1.0))
    words = _z.empty(K, nzones) if acc is None else acc.words.copy()
    before = words[..., _z.REJECTED].copy()
    if n:
        ctx.zonal(values.dtype, n, K, nzones, ztype, values.ctypes.data, zones.ctypes.data, wptr, words.ctypes.data,
                  bounds, weight_kind=kind, cols=cols, where=_lib.HOST, stage_bytes=stage_bytes)
    if explicit:
        bad = np.argwhere(words[..., _z.REJECTED] != before)
        if len(bad):
            k, z = (int(v) for v in bad[0])
            raise ValueError('%d pixels of zone %d, layer %d lie outside the bounds (wmax %r, xmax %r)'
                             % (words[k, z, _z.REJECTED] - before[k, z], z, k, bounds[0], bounds[1]))
    return _z.ZonalResult(words, bounds[2], bounds[3], squeeze=not layered)


def _zonalq_wmax(ctx, values, weights, kind, cols, wmax, stage_bytes):
    '''``(wmax, ew)`` of a histogram call on host arrays: ``(1.0, 31)`` without weights, the given bound,
    or what the ``mod16_zonal_bounds_*`` pre-pass finds.'''
    from . import zonalq as _q
    if kind == _lib.ZONAL_WEIGHT_NONE:
        return 1.0, 31
    K, n = values.shape
    if wmax is None:
        wmax = ctx.zonal_bounds(values.dtype, n, K, values.ctypes.data, weights.ctypes.data, weight_kind=kind, cols=cols,
                                where=_lib.HOST, stage_bytes=stage_bytes)[0] if n else 1.0
        wmax = wmax if wmax > 0 else 1.0
    return _q.check_wmax(wmax)


def zonal_histogram(values, zones, bins, range, nzones=None, area=None, wmax=None, acc=None, device=0, stage_bytes=None):
    r'''
    (Extension.) Zonal histograms of a raster: per zone and layer the weight of the valid pixels in
    ``bins`` equal bins over ``range = (lo, hi)``, with an under bin (``x < lo``) and an over bin (``not x
    < hi``), in one pass over the values (``mod16_zonal_hist_*``). The words are integers that integer
    adds fill, so the result does not depend on ``stage_bytes``, on how a raster is cut into calls
    that accumulate (``acc=``) or on the device that ran a part (``ZonalHistogram.merge``). The
    definition is ``mod16_amd.zonalq`` (``histogram``).

    Parameters
    ----------
    values, zones, nzones, area, device, stage_bytes
        as in ``zonal_statistics``; infinite values take part (they land in the under or over bin)
    bins : int
        between 1 and 4094
    range : (float, float)
        ``(lo, hi)``, finite, ``lo < hi``; bin ``i`` holds ``lo + i (hi - lo) / bins <= x <`` the next edge
    wmax : float
        (Optional) the largest weight the call accepts (a pixel whose weight lies outside ``[0, wmax]``
        is skipped); its exponent fixes the scale of the words, so calls that are to be accumulated
        or merged must share it. Default: a pre-pass over the weights finds it
    acc : ZonalHistogram
        (Optional) a histogram to add into (it is not modified); with an ``area`` it needs ``wmax``

    Returns
    -------
    mod16_amd.zonalq.ZonalHistogram
        ``counts`` ``(K, Z, bins)``, ``under``, ``over`` ``(K, Z)`` (without the ``K`` for values without a
        layer axis), ``edges``, ``words``, ``lo``, ``hi``, ``bins``, ``ew``, ``merge(other)``. A word times
        ``2**(ew - 31)`` is a sum of weights; without weights ``ew`` is 31 and a word is a count.
    '''
    from . import zonal as _z, zonalq as _q
    values, zones, nzones, layered, kind, cols, weights = _zonal_inputs(values, zones, nzones, area)
    K, n = values.shape
    bins = _q.check_bins(bins)
    try:
        lo, hi = range
    except (TypeError, ValueError):
        raise ValueError('range must be a pair (lo, hi), got %r' % (range,))
    lo, hi, scale = _q.check_range(bins, lo, hi)
    _check_stage_bytes(stage_bytes)
    if acc is not None:
        if not isinstance(acc, _q.ZonalHistogram):
            raise ValueError('acc must be a ZonalHistogram')
        if kind != _lib.ZONAL_WEIGHT_NONE:
            _q.check_acc_wmax(wmax)
        if acc.words.shape != (K, nzones, bins + 2) or (acc.lo, acc.hi) != (lo, hi):
            raise ValueError('acc holds %r words over %r, this call needs %r over %r'
                             % (acc.words.shape, (acc.lo, acc.hi), (K, nzones, bins + 2), (lo, hi)))
    ctx = _lib.context(device)
    wmax, ew = _zonalq_wmax(ctx, values, weights, kind, cols, wmax, stage_bytes)
    if acc is not None and acc.ew != ew:
        raise ValueError('the exponent of wmax, %d, differs from the histogram\'s %d' % (ew, acc.ew))
    words = np.zeros((K, nzones, bins + 2), np.int64) if acc is None else acc.words.copy()
    if n:
        spec = ctx.zonal_hist_spec(values.dtype, n, K, nzones, _z.ZONE_TYPES[zones.dtype.name], kind, cols, 0, n, wmax, ew,
                                   bins=bins, lo=lo, hi=hi, scale=scale)
        ctx.zonal_hist(spec, values.dtype, values.ctypes.data, zones.ctypes.data, None if weights is None else weights.ctypes.data,
                       None, words.ctypes.data, where=_lib.HOST, stage_bytes=stage_bytes)
    return _q.ZonalHistogram(words, lo, hi, ew, squeeze=not layered)


def zonal_quantiles(values, zones, q=(0.05, 0.5, 0.95), nzones=None, area=None, wmax=None, bits=None, device=0,
                    stage_bytes=None):
    r'''
    (Extension.) Exact zonal quantiles of a raster: per zone, layer and ``q`` the smallest value of the
    zone whose cumulative weight reaches ``q`` of the zone's total weight -- the weighted inverted-CDF
    quantile, a value of the raster, found by radix selection over integer histograms of the values'
    order-preserving keys (``mod16_zonal_hist_*``, ``mod16_zonal_select``). It does not depend on the
    order of the pixels, on ``stage_bytes`` or on ``bits``. ``q`` is taken as the exact rational of its
    double. The definition is ``mod16_amd.zonalq`` (``quantiles``).

    The values are staged to the device once per level and the level is closed on the host: the call
    crosses PCIe ``levels = ceil(width / bits)`` times (4 for float32 and 8 for float64 at 8 bits).
    ``RasterEngine.zonal_quantiles`` keeps a resident stack on the device.

    Parameters
    ----------
    values, zones, nzones, area, device, stage_bytes
        as in ``zonal_statistics``; infinite values take part
    q : float or sequence of float
        between 1 and 16 quantiles in ``[0, 1]``
    wmax : float
        (Optional) the largest weight the call accepts (Default: a pre-pass finds it); a weight below
        ``2**-32`` of the power of two above it counts for nothing
    bits : int
        (Optional) bits of the key a level resolves, 4 to 12 (Default: 8)

    Returns
    -------
    mod16_amd.zonalq.ZonalQuantiles
        ``values`` ``(K, Z, S)`` in the values' dtype (``(Z, S)`` for values without a layer axis; NaN where
        a zone holds no weight), ``weight`` ``(K, Z)`` int64, ``q``, ``ew``
    '''
    from . import zonal as _z, zonalq as _q
    values, zones, nzones, layered, kind, cols, weights = _zonal_inputs(values, zones, nzones, area)
    K, n = values.shape
    qs = _q.check_q(q)
    bits = _q.DEFAULT_BITS if bits is None else _q.check_bits(bits)
    _check_stage_bytes(stage_bytes)
    ctx = _lib.context(device)
    wmax, ew = _zonalq_wmax(ctx, values, weights, kind, cols, wmax, stage_bytes)
    wd = _q.width(values.dtype)
    nlevels, S = _q.levels(wd, bits), len(qs)
    hist = np.zeros((K, nzones, S, 1 << bits), np.int64)
    remaining = np.zeros((K, nzones, S), np.int64)
    prefix = np.zeros((K, nzones, S), np.uint64)
    weight = np.zeros((K, nzones), np.int64)
    out = np.full((K, nzones, S), np.nan, values.dtype)
    wptr = None if weights is None else weights.ctypes.data
    for level in range(nlevels):
        spec = ctx.zonal_hist_spec(values.dtype, n, K, nzones, _z.ZONE_TYPES[zones.dtype.name], kind, cols, 0, n, wmax, ew,
                                   bits=bits, level=level, slots=S)
        if n:
            ctx.zonal_hist(spec, values.dtype, values.ctypes.data, zones.ctypes.data, wptr,
                           prefix.ctypes.data if level else None, hist.ctypes.data, where=_lib.HOST, stage_bytes=stage_bytes)
        ctx.zonal_select(spec, hist.ctypes.data, remaining.ctypes.data, prefix.ctypes.data,
                         out.ctypes.data if level == nlevels - 1 else None, weight.ctypes.data if level == 0 else None,
                         q=[_q.rational(v) for v in qs] if level == 0 else None, where=_lib.HOST)
        hist[...] = 0
    return _q.ZonalQuantiles(out, weight, qs, ew, squeeze=not layered)


EnsembleQuantiles = _collections.namedtuple('EnsembleQuantiles', 'q day night total')


def evapotranspiration_ensemble_quantiles(
        tables, cls, lw_net_day, lw_net_night, sw_rad_day, sw_rad_night,
        sw_albedo, temp_day, temp_night, temp_annual, tmin, vpd_day,
        vpd_night, pressure, fpar, lai, q=(0.05, 0.5, 0.95), beta=None, math=_lib.MATH_FAST, device=0,
        out=None, slab_bytes=None):
    r'''
    (Extension.) Per-pixel quantiles of ET over an ENSEMBLE of parameter tables: what a loop over
    ``evapotranspiration_raster(tables[m], cls, *drivers)`` followed by ``np.quantile(..., q, axis=0)``
    returns -- the median and a credible interval of a calibration posterior per pixel -- without the
    (D, n) arrays: the member values of a batch of pixels pass through a slab on the device and are
    ordered there (``mod16_et_ensemble_quantiles_*``). The definition is
    ``mod16_amd.calibration.ensemble_quantile`` (numpy's default ``'linear'`` method).

    Parameters
    ----------
    tables, cls, the 14 drivers, beta, math, device
        as for ``evapotranspiration_ensemble``; 1 <= D <= 256 here
    q : float or sequence of float
        1 to 8 quantiles, each in [0, 1]
    out : sequence of numpy.ndarray
        (Optional) three arrays ``(Q,) + shape`` to write day, night and total into
    slab_bytes : int
        (Optional) device memory the member values may take at a time (default 128 MiB; at least
        one batch of 256 pixels is taken); the result does not depend on it

    Returns
    -------
    EnsembleQuantiles
        ``(q, day, night, total)``: ``q`` as a float64 array (Q,); the quantiles of the day total, the
        night total and of day + night (summed per member), each ``(Q,) + shape`` [kg m-2 s-1].
        float32 only if every driver array is float32 (members, sum, order and interpolation in
        float64, rounded once). A NaN in any member makes all Q values of that pixel and series NaN.
        Pixels broadcast as in numpy; all-scalar input gives ``(Q,)`` arrays.
    '''
    from .calibration import quantile_positions
    stack = _ensemble_stack(tables, beta)
    qs = np.atleast_1d(np.asarray(q, np.float64))
    if len(stack):
        quantile_positions(qs, len(stack))       # ValueError for a bad q
    nq = qs.size
    drivers = (
        lw_net_day, lw_net_night, sw_rad_day, sw_rad_night, sw_albedo,
        temp_day, temp_night, temp_annual, tmin, vpd_day, vpd_night,
        pressure, fpar, lai)
    dtype = _result_dtype(drivers)
    cls = _as_uint8(cls)
    shape, n = _broadcast([_shape(v) for v in drivers] + [cls.shape])
    keep, dptr, dstride = _marshal(drivers, shape, dtype)
    cls = np.ascontiguousarray(np.broadcast_to(cls, shape))
    full = (nq,) + tuple(shape)
    outs = _outputs(out, full, [dtype] * 3)
    ens = _lib.Ensemble(_lib.context(device), stack)
    try:
        if n:
            esz = np.dtype(dtype).itemsize
            optr = [o.ctypes.data + k * n * esz for o in outs for k in range(nq)]
            ens.quantiles(dtype, cls.ctypes.data, dptr, dstride, n, qs, optr, slab_bytes=slab_bytes,
                          flags=math, where=_lib.HOST)
    finally:
        ens.close()
    return EnsembleQuantiles(qs, *outs)


def evapotranspiration_raw(
        bplut, cls, lw_net_day, lw_net_night, sw_rad_day, sw_rad_night,
        sw_albedo, temp_day, temp_night, temp_annual, tmin, qv10m_day,
        qv10m_night, ps_day, ps_night, elevation, fpar_pct, lai_x10,
        day_hours=None, beta=None, math=_lib.MATH_FAST, device=0, devices=None):
    r'''
    (Extension) Forward run on raw drivers: the
    pre-processing the reference does in front of ``evapotranspiration()``
    (mod16/calibration.py:380-423) is folded into the kernel --

    - ``vpd_day = MOD16.vpd(qv10m_day, ps_day, temp_day)``,
      ``vpd_night = max(MOD16.vpd(qv10m_night, ps_night, temp_night), 0)``;
    - ``pressure = MOD16.air_pressure(elevation)``;
    - ``fpar = fpar_pct / 100``, ``lai = lai_x10 / 10`` with ``fpar_pct`` and
      ``lai_x10`` as uint8 rasters in the MODIS encodings (codes >= 249 are
      fill values and give NaN).

    Returns ``(day, night)`` [kg m-2 s-1] or, with ``day_hours`` (hours of
    daylight), ``(day, night, total8)`` where ``total8 = (day h + night (24 -
    h)) * 8 * 3600`` [kg m-2 (8 d)-1], the MOD16A2 unit
    (tests/verification/verify2.py:113-115). ``devices``: several GPUs behind the
    one call, as for ``evapotranspiration_raster``.
    '''
    from . import multi
    from .utils import as_bplut_table
    table = as_bplut_table(bplut, beta)
    devs = multi.device_list(devices)
    raw = [lw_net_day, lw_net_night, sw_rad_day, sw_rad_night, sw_albedo,
           temp_day, temp_night, temp_annual, tmin, qv10m_day, qv10m_night,
           ps_day, ps_night, elevation]
    hours = [day_hours] if day_hours is not None else []
    dtype = _result_dtype(raw + hours)
    u8 = [np.asarray(v) for v in (cls, fpar_pct, lai_x10)]
    shape = np.broadcast_shapes(*[np.shape(v) for v in raw + hours + u8])
    n = int(np.prod(shape, dtype=np.int64))
    keep, rptr, rstr = _marshal(raw, shape, dtype)
    hkeep, hptr, hstr = _marshal(hours, shape, dtype) if hours else (None, [None], [0])
    bytes_ = [np.ascontiguousarray(np.broadcast_to(_as_uint8(a, 'uint8 raster value outside [0, 255]'), shape))
              for a in u8]
    outs = [_lib.pinned.empty(shape, dtype) for _ in range(3 if hours else 2)]
    esz = dtype.itemsize

    def part(ctx, off, m):
        ctx.set_bplut(table)
        if m <= 0:
            return
        ctx.check(_lib.typed(ctx.lib, 'mod16_et_raw', dtype)(
            ctx.handle, bytes_[0].ctypes.data + off, _lib.ptr_array(_shift(rptr, rstr, off, 1, esz)),
            _lib.i64_array(rstr), bytes_[1].ctypes.data + off, bytes_[2].ctypes.data + off,
            _shift(hptr, hstr, off, 1, esz)[0], int(hstr[0]), m,
            outs[0].ctypes.data + off * esz, outs[1].ctypes.data + off * esz,
            outs[2].ctypes.data + off * esz if hours else None, int(math), _lib.HOST, None))

    multi.deal(devs, device, n, part)
    if not shape:
        outs = [o[()] for o in outs]
    return tuple(outs)
