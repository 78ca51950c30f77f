'''
Device-resident forward run for large rasters.

``RasterEngine`` is the zero-copy, asynchronous form of
``mod16_amd.evapotranspiration_raster``: drivers, class raster and outputs are
``torch`` tensors already in HBM, the kernel is enqueued on the current HIP
stream through the C ABI (``mod16_et_*`` with ``where = MOD16_DEVICE``) and
nothing is copied. PyTorch is used for device memory and streams only.
'''
import ctypes as C

import numpy as np

from . import _lib, _tensors as _t
from .downscale import MET_DRIVERS

#: algorithmic HBM bytes per pixel: 14 driver loads +
#: 1 class byte + 2 stores
BYTES_PER_PIXEL = {'float64': 14 * 8 + 1 + 2 * 8, 'float32': 14 * 4 + 1 + 2 * 4}
DIAG_FIELDS = ('sum_day', 'sum_night', 'n_valid_day', 'n_valid_night',
               'n_nan_day', 'n_nan_night', 'max_day', 'max_night')


def _torch():
    import torch
    return torch


class _GraphHandle(object):
    '''Owns a ``mod16_graph`` (destroyed with the bound launch that uses it).'''

    def __init__(self, lib, handle, ctx=None):
        self.lib, self.handle = lib, handle
        self.ctx = ctx          # keeps the context alive as long as its graph

    def __del__(self):
        try:
            if self.handle and self.handle.value:
                self.lib.mod16_graph_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class TiledRaster(object):
    '''
    A raster resident on the device in the engine's own layout (``mod16_layout``
    in include/mod16_hip.h): the pixels are cut into tiles of ``tile`` pixels and
    the 14 driver arrays interleaved tile by tile -- ``[tile][driver][tile
    pixels]`` -- the two outputs likewise in a block of their own, the class
    raster as plain bytes. ``form`` (``_lib.FORM_*``, ``enum mod16_form``) selects
    another form of the forward run -- potential ET, components, raw drivers -- with
    its own counts of arrays: ``wide`` (the drivers), ``bytes`` (class raster first,
    then the uint8 fPAR / LAI of the raw forms) and ``outs``, in the order of
    include/mod16_hip.h. Every array is still an array: ``drivers[k]``, ``day``,
    ``night`` and ``cls`` are 2-D strided ``torch`` views of shape ``(ntiles,
    tile)`` into one allocation, so ``drivers[5].copy_(temp.view(-1, tile))``,
    slicing and reductions work as on any tensor. Why: streamed side by side, 16
    separate 7 GB arrays lie GiB apart in HBM and the kernel's 14-read + 2-write
    mix reaches 5.7 TB/s; with the fields of a tile inside one ~1 MiB block the
    same bytes move at 6.5 TB/s (``tools/probe_layout.hip``).
    The storage is padded to whole tiles; ``n`` is the number of real pixels.
    '''

    def __init__(self, engine, n, tile=None, form=_lib.FORM_TOTALS):
        torch = _torch()
        esz = engine.np_dtype.itemsize
        self.n = int(n)
        self.form = int(form)
        nw, nb, no = _lib.FORM_SHAPE[self.form]
        self.tile = int(tile) if tile else engine.TILE_BYTES // esz
        if self.tile & (self.tile - 1) or self.tile * esz < 8192:
            raise ValueError('tile must be a power of two of at least 8 KiB per field')
        vec = 16 // esz
        if self.n % vec:
            raise ValueError('a tiled raster holds a multiple of %d pixels' % vec)
        self.ntiles = max(1, -(-self.n // self.tile))
        P, nt = self.tile, self.ntiles
        in_bytes, out_bytes, byte_bytes = nt * nw * P * esz, nt * no * P * esz, nt * nb * P
        self.slab = torch.empty(in_bytes + out_bytes + byte_bytes + 4096, dtype=torch.uint8,
                                device=engine._dev())
        wide = self.slab[:in_bytes].view(engine.dtype).view(nt, nw, P)
        self.wide = [wide[:, k, :] for k in range(nw)]
        outs = self.slab[in_bytes:in_bytes + out_bytes].view(engine.dtype).view(nt, no, P)
        self.outs = [outs[:, k, :] for k in range(no)]
        rasters = self.slab[in_bytes + out_bytes:in_bytes + out_bytes + byte_bytes].view(nt, nb, P)
        self.bytes = [rasters[:, k, :] for k in range(nb)]
        # the names of the totals form (the production step)
        self.drivers = self.wide[:14]
        self.cls = self.bytes[0]
        totals = self.form != _lib.FORM_COMPONENTS
        self.day, self.night = (self.outs[0], self.outs[1]) if totals else (None, None)
        self.layout = _lib.Layout(P, nw * P, no * P, nb * P)
        self.dtype = engine.dtype

    def flat(self, field, lo=0, hi=None):
        '''Pixels [lo, hi) of one array of the raster as a contiguous 1-D
        tensor -- always a COPY (only the tiles it touches are read): inside one
        tile the strided view is contiguous and reshape would hand back an alias
        of live raster memory, which the next launch overwrites.'''
        hi = self.n if hi is None else hi
        P = self.tile
        t0, t1 = lo // P, -(-hi // P)
        out = field[t0:t1].reshape(-1)[lo - t0 * P:hi - t0 * P]
        if out.data_ptr() == field[t0:t1].data_ptr() + (lo - t0 * P) * field.element_size():
            out = out.clone()
        return out

    def put(self, field, src, lo=0):
        '''Write the 1-D tensor ``src`` into pixels [lo, lo + len(src)) of one
        array of the raster.'''
        P = self.tile
        pos, end = lo, lo + src.numel()
        while pos < end:                       # head, whole tiles at once, tail
            t, w = divmod(pos, P)
            if w == 0 and end - pos >= P:
                k = (end - pos) // P
                field[t:t + k].copy_(src[pos - lo:pos - lo + k * P].view(k, P))
                pos += k * P
            else:
                m = min(P - w, end - pos)
                field[t, w:w + m].copy_(src[pos - lo:pos - lo + m])
                pos += m


class BoundStep(object):
    '''A pre-marshalled step (see ``RasterEngine.bind`` / ``bind_tiled``):
    calling it enqueues the step on the current stream.'''

    def __init__(self, launch, outputs, graph=None, device=0):
        self._launch, self.outputs, self._graph, self._device = launch, outputs, graph, device

    def __call__(self):
        self._launch()
        return self.outputs

    def time(self, launches=10):
        '''Mean milliseconds per replay of the captured step, HIP events on
        the current stream (``mod16_time_graph``).'''
        if self._graph is None:
            raise RuntimeError('only a step bound as a HIP graph can be timed this way')
        torch = _torch()
        ms = C.c_float(0)
        rc = self._graph.lib.mod16_time_graph(
            self._graph.handle, int(launches),
            C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream), C.byref(ms))
        self._graph.ctx.check(rc)
        return ms.value


class EnsembleRun(object):
    '''The members of an ensemble forward run resident on an engine's device
    (``RasterEngine.ensemble``): ``members`` parameter tables uploaded once, ``run`` (mean and spread),
    ``quantiles`` and ``run_members`` as often as there are rasters.'''

    def __init__(self, engine, tables):
        from . import _ensemble_stack
        self.engine = engine
        self._ens = _lib.Ensemble(engine.ctx, _ensemble_stack(tables))
        self.members = self._ens.members

    def run(self, cls, drivers, out=None):
        '''Enqueue the ensemble kernel on the current stream: per-pixel mean and spread of ET over
        the members for device-resident drivers (tensors, or scalars to broadcast). Returns the five
        tensors ``(mean_day, mean_night, std_day, std_night, std_total)`` (``out`` may give them).
        Asynchronous: call the engine's ``check()`` (or synchronise the stream) before trusting the
        data; a class code >= 13 raises IndexError there.'''
        eng, torch = self.engine, _torch()
        n = cls.numel()
        cptr = eng._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = eng._marshal_drivers(drivers, n)
        out = tuple(out) if out is not None else tuple(eng.empty(n, 5))
        if len(out) != 5:
            raise ValueError('out must hold 5 tensors')
        optr = [eng._check_tensor(t, eng.dtype, n, 'out') for t in out]
        self._ens.run(eng.np_dtype, cptr, dptr, dstride, n, optr, flags=eng.math, where=_lib.DEVICE,
                      stream=eng._stream())
        return out

    def quantiles(self, cls, drivers, q=(0.05, 0.5, 0.95), out=None, slab_bytes=None):
        '''Enqueue the quantile run on the current stream: the quantiles ``q`` (1 to 8 values in
        [0, 1]) over the members of the day total, the night total and day + night per pixel
        (``mod16_et_ensemble_quantiles_*``, defined by ``mod16_amd.calibration.ensemble_quantile``).
        Returns three ``(Q, n)`` tensors ``(day, night, total)`` (``out`` may give them). The member
        values pass through a stream-ordered temporary of at most ``slab_bytes`` (default 128 MiB, at
        least one batch of 256 pixels). At most 256 members. Asynchronous, ``check()`` as for ``run``.'''
        from .calibration import quantile_positions
        eng, torch = self.engine, _torch()
        n = cls.numel()
        qs = np.atleast_1d(np.asarray(q, np.float64))
        quantile_positions(qs, self.members)
        nq = qs.size
        cptr = eng._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = eng._marshal_drivers(drivers, n)
        if out is None:
            out = tuple(torch.empty((nq, n), dtype=eng.dtype, device=eng._dev()) for _ in range(3))
        out = tuple(out)
        if len(out) != 3:
            raise ValueError('out must hold 3 tensors')
        esz = eng.np_dtype.itemsize
        optr = [eng._check_tensor(t, eng.dtype, nq * n, 'out') + k * n * esz for t in out for k in range(nq)]
        self._ens.quantiles(eng.np_dtype, cptr, dptr, dstride, n, qs, optr, slab_bytes=slab_bytes,
                            flags=eng.math, where=_lib.DEVICE, stream=eng._stream())
        return out

    def run_members(self, cls, drivers, out=None):
        '''Enqueue the member kernel on the current stream: every member's day and night total,
        two ``(members, n)`` tensors ``(day, night)`` (``out`` may give them)
        (``mod16_et_ensemble_members_*``). Asynchronous, ``check()`` as for ``run``.'''
        eng, torch = self.engine, _torch()
        n = cls.numel()
        D = self.members
        cptr = eng._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = eng._marshal_drivers(drivers, n)
        if out is None:
            out = tuple(torch.empty((D, n), dtype=eng.dtype, device=eng._dev()) for _ in range(2))
        out = tuple(out)
        if len(out) != 2:
            raise ValueError('out must hold 2 tensors')
        optr = [eng._check_tensor(t, eng.dtype, D * n, 'out') for t in out]
        self._ens.run_members(eng.np_dtype, cptr, dptr, dstride, n, optr[0], optr[1], n, flags=eng.math,
                              stream=eng._stream())
        return out

    def close(self):
        self._ens.close()


class UpscaleGrid(object):
    '''The cells of an ``H x W`` coarse grid in an ``R x C`` fine raster, resident on an engine's device
    (``RasterEngine.upscale_grid``): the run tables uploaded once, ``run`` (the area-weighted mean of
    the valid fine pixels of every cell, the valid fraction and the count) and ``majority`` (the
    dominant class per cell) as often as there are rasters, ``sums`` for what several rasters (tiles) add
    up before ``mod16_amd.upscale.merge`` divides. The definition is ``mod16_amd.upscale``. With row-affine
    columns (``col_affine``: a sinusoidal tile) ``col_runs`` is None -- the device finds the column runs per
    fine row -- and ``col_affine`` and ``col_range`` hold the checked geometry.'''

    def __init__(self, engine, shape, coarse_shape, row_pos, col_pos=None, wrap=False, area=None, col_affine=None,
                 col_range=None):
        self.engine = engine                 # keeps the engine alive as long as its grid
        self._grid = _lib.Upscale(engine.ctx, shape, coarse_shape, row_pos, col_pos, wrap=wrap, area=area,
                                  col_affine=col_affine, col_range=col_range)
        self.shape, self.coarse_shape = self._grid.shape, self._grid.coarse_shape
        self.row_runs, self.col_runs, self.wrap = self._grid.row_runs, self._grid.col_runs, self._grid.wrap
        self.col_affine, self.col_range = self._grid.col_affine, self._grid.col_range

    def run(self, values, min_fraction=0.0, outputs=('mean',), out=None):
        '''Enqueue the upscaling kernel on the current stream (``mod16_upscale_*``; the definition is
        ``mod16_amd.upscale.aggregate``, which the result equals bit for bit). ``values`` is a ``(K, R,
        C)`` or ``(R, C)`` float32 or float64 tensor with unit stride in columns, rows at least ``C``
        apart and layers at least a plane apart, at any element offset -- the ``(P, n)`` rows a composite
        wrote, viewed as ``(P, R, C)``, pass as they are. NaN is missing. Returns ``Upscaled(mean,
        fraction, count)`` on the coarse grid with the fields ``outputs`` names (None for the others,
        which are neither computed nor written): ``mean`` is NaN where a cell has no valid pixel or its
        valid weight is below ``min_fraction`` of the cell's. ``out`` may give the tensors as a dict by
        name; no output may overlap the input. Asynchronous, like ``composite``.'''
        from . import upscale as _u
        eng, torch = self.engine, _torch()
        _t.check_device(values, 'values', eng.device, torch.float32, torch.float64)
        K, squeeze = _u.check_layers(tuple(values.shape), self.shape)
        min_fraction = _u.check_min_fraction(min_fraction)
        names = _u.check_outputs(outputs)
        pitch, plane = _t.plane_layout(values, 'values')
        dtype = _t.numpy_dtype(values.dtype)
        outs, lay = _t.named_outputs(out, _u.output_table(names, (() if squeeze else (K,)) + self.coarse_shape, dtype),
                                     eng.device)
        try:                       # (per output: address, plane stride, row pitch)
            self._grid.run(dtype, values.data_ptr(), K, plane, pitch, min_fraction,
                           [(outs[k].data_ptr(), lay[k][1], lay[k][0]) if k in outs else None for k in _u.OUTPUT_NAMES],
                           where=_lib.DEVICE, stream=eng._stream())
        except _lib.Mod16Error as e:
            raise _lib.overlap_as_value_error(e)
        return _u.Upscaled(*[outs.get(k) for k in _u.OUTPUT_NAMES])

    def sums(self, values, outputs=None, out=None):
        '''Enqueue the sums kernel on the current stream (``mod16_upscale_sums_*``; the definition is
        ``mod16_amd.upscale.sums`` / ``sums_rows``): ``values`` as ``run`` takes them -> ``UpscaledSums(num,
        den, tot, count)``, float64 whatever the type of ``values`` and int32, with the fields ``outputs``
        names (default: all four). What a raster contributes to cells it covers only in part: add the
        tensors of several tiles in a fixed order, or download them and ``mod16_amd.upscale.merge``.'''
        from . import upscale as _u
        eng, torch = self.engine, _torch()
        _t.check_device(values, 'values', eng.device, torch.float32, torch.float64)
        K, squeeze = _u.check_layers(tuple(values.shape), self.shape)
        names = _u.check_sum_outputs(_u.SUM_NAMES if outputs is None else outputs)
        pitch, plane = _t.plane_layout(values, 'values')
        outs, lay = _t.named_outputs(out, _u.sum_table(names, (() if squeeze else (K,)) + self.coarse_shape), eng.device)
        try:
            self._grid.sums(_t.numpy_dtype(values.dtype), values.data_ptr(), K, plane, pitch,
                            [(outs[k].data_ptr(), lay[k][1], lay[k][0]) if k in outs else None for k in _u.SUM_NAMES],
                            where=_lib.DEVICE, stream=eng._stream())
        except _lib.Mod16Error as e:
            raise _lib.overlap_as_value_error(e)
        return _u.UpscaledSums(*[outs.get(k) for k in _u.SUM_NAMES])

    def majority(self, cls, valid=None, outputs=('cls',), out=None):
        '''Enqueue the class kernel on the current stream (``mod16_upscale_classes``; the definition is
        ``mod16_amd.upscale.majority``): ``cls`` an ``(R, C)`` uint8 tensor -> ``UpscaledClasses(cls,
        share)``, per cell the valid code with the most pixels (the lowest on a tie, 255 where none is
        valid; ``valid``: the codes that count, default 0 ... 12) and its share of the cell's pixels
        (float32).'''
        from . import upscale as _u
        eng, torch = self.engine, _torch()
        _t.check_device(cls, 'cls', eng.device, torch.uint8)
        if tuple(cls.shape) != self.shape:
            raise ValueError('cls must have shape %r, got %r' % (self.shape, tuple(cls.shape)))
        mask = _u.valid_mask(valid)
        names = _u.check_class_outputs(outputs)
        pitch, _ = _t.plane_layout(cls, 'cls')
        outs, lay = _t.named_outputs(out, _u.output_table(names, self.coarse_shape), eng.device)
        pair = {k: (outs[k].data_ptr(), lay[k][0]) for k in outs}
        try:
            self._grid.classes(cls.data_ptr(), pitch, mask, pair.get('cls'), pair.get('share'), where=_lib.DEVICE,
                               stream=eng._stream())
        except _lib.Mod16Error as e:
            raise _lib.overlap_as_value_error(e)
        return _u.UpscaledClasses(*[outs.get(k) for k in _u.CLASS_OUTPUT_NAMES])

    def close(self):
        self._grid.close()


class DownscaleGrid(object):
    '''The geometry of an ``R x C`` fine raster over an ``H x W`` coarse grid resident on an engine's
    device (``RasterEngine.downscale_grid``): the corner tables uploaded once, ``run`` (ET with coarse
    drivers interpolated per pixel inside the kernel) and ``fields`` (the interpolated fields alone)
    as often as there are days. The definition is ``mod16_amd.downscale``. Exactly one of ``col_pos``
    (column tables) and ``col_affine = (col_origin, col_scale)`` (row-affine columns, e.g. a sinusoidal
    tile: the kernels form the column pair per pixel, ``col_tables`` is None) gives the columns;
    ``run``, ``fields`` and ``composite`` are the same for both.'''

    def __init__(self, engine, shape, coarse_shape, row_pos, col_pos=None, wrap=False, method='bilinear',
                 col_affine=None):
        self.engine = engine
        self._grid = _lib.Downscale(engine.ctx, shape, coarse_shape, row_pos, col_pos, wrap=wrap, method=method,
                                    col_affine=col_affine)
        self.shape, self.coarse_shape = self._grid.shape, self._grid.coarse_shape
        self.row_tables, self.col_tables = self._grid.row_tables, self._grid.col_tables
        self.col_affine = self._grid.col_affine      # (col_origin, col_scale) of row-affine columns, else None

    def _coarse(self, t, what, series=False):
        '''-> (address, row pitch, plane stride in elements) of an (H, W) tensor or, with ``series``, an
        (S, H, W) one'''
        eng = self.engine
        H, W = self.coarse_shape
        _t.check_device(t, what, eng.device, eng.dtype)
        if tuple(t.shape[-2:]) != (H, W) or t.dim() != 2 and not (series and t.dim() == 3):
            raise ValueError('%s is a coarse array: expected shape %r%s, got %r'
                             % (what, (H, W), ' or (S, %d, %d)' % (H, W) if series else '', tuple(t.shape)))
        return (t.data_ptr(),) + _t.plane_layout(t, what)

    def run(self, cls, drivers, coarse=MET_DRIVERS, first_pixel=0, out_day=None, out_night=None):
        '''Enqueue the downscaled forward run on the current stream: ET day and night for the
        ``n = cls.numel()`` pixels ``[first_pixel, first_pixel + n)`` of the raster (row-major).
        Each of the 14 ``drivers`` named in ``coarse`` (default ``mod16_amd.downscale.MET_DRIVERS``,
        the eleven reanalysis fields) is an ``(H, W)`` tensor with unit stride in columns and any
        row pitch >= W, the same for all of them; every other driver is a scalar or a tensor of
        the ``n`` pixels of the range. Returns ``(day, night)`` (``out_day`` / ``out_night`` may give
        them): what ``run`` returns on the drivers ``mod16_amd.downscale.interpolate`` materialises,
        bit for bit. The engine's ``math`` must be ``MATH_FAST`` or ``MATH_EXACT``. Asynchronous:
        call the engine's ``check()`` (or synchronise the stream) before trusting the data; a class
        code >= 13 raises IndexError there.'''
        from . import downscale as _d
        eng, torch = self.engine, _torch()
        if eng.math & ~_lib.MATH_EXACT:
            raise ValueError('the downscaled run needs an engine with MATH_FAST or MATH_EXACT (no MATH_MIXED, not trusted)')
        names = _d.check_coarse(coarse)
        if len(drivers) != _lib.N_DRIVERS:
            raise ValueError('expected 14 drivers')
        n = cls.numel()
        shapes = [tuple(d.shape) if isinstance(d, torch.Tensor) and (name in names or d.numel() != 1) else ()
                  for name, d in zip(_d.DRIVER_NAMES, drivers)]
        kinds, first, n = _d.check_call(self.shape, self.coarse_shape, shapes, coarse=names, first_pixel=first_pixel,
                                        n=n, method=self._grid.method, cls_size=n)
        cptr = eng._check_tensor(cls, torch.uint8, n, 'cls')
        keep, ptrs, rows = [], [], []
        for name, d, kind in zip(_d.DRIVER_NAMES, drivers, kinds):
            if kind == _d.KIND_COARSE:
                ptr, row, _ = self._coarse(d, name)
                rows.append(row)
                keep.append(d)
            elif kind == _d.KIND_FINE:
                ptr = eng._check_tensor(d, eng.dtype, n, name)
                keep.append(d)
            else:
                sc = torch.as_tensor(d, dtype=eng.dtype).reshape(1).to(eng._dev())
                keep.append(sc)
                ptr = sc.data_ptr()
            ptrs.append(ptr)
        pitch = _t.share_one(rows, 'the coarse drivers', 'distance between rows')
        if out_day is None:
            out_day = eng.empty(n)[0]
        if out_night is None:
            out_night = eng.empty(n)[0]
        pd = eng._check_tensor(out_day, eng.dtype, n, 'out_day')
        pn = eng._check_tensor(out_night, eng.dtype, n, 'out_night')
        if n:
            self._grid.run(eng.np_dtype, cptr, ptrs, kinds, pitch or self.coarse_shape[1], first, n, pd, pn,
                           flags=eng.math, where=_lib.DEVICE, stream=eng._stream())
        return out_day, out_night

    def fields(self, coarse_fields, first_pixel=0, n=None, out=None):
        '''Enqueue the interpolation alone on the current stream: the ``F`` coarse ``(H, W)`` tensors
        ``coarse_fields`` (one row pitch for all) at the pixels ``[first_pixel, first_pixel + n)``
        (``n`` None: to the end) as an ``(F, n)`` tensor in the engine's dtype -- the float64
        interpolant of ``mod16_amd.downscale.interpolate``, rounded once. ``out`` may give it: rows of
        unit stride, any distance >= n between them; what lies between the rows is not touched.'''
        from . import downscale as _d
        eng, torch = self.engine, _torch()
        fields = list(coarse_fields)
        if not fields:
            raise ValueError('fields needs at least one coarse field')
        first, n = _d.check_range(self.shape, first_pixel, n)
        ptrs, rows, _ = zip(*[self._coarse(t, 'field %d' % k) for k, t in enumerate(fields)])
        pitch = _t.share_one(rows, 'the coarse fields', 'distance between rows')
        F = len(fields)
        if out is None:
            out = torch.empty((F, n), dtype=eng.dtype, device=eng._dev())
        _t.check_device(out, 'out', eng.device, eng.dtype)
        if tuple(out.shape) != (F, n):
            raise ValueError('out must have shape (%d, %d)' % (F, n))
        opitch = _t.row_pitch(out, 'out')
        esz = eng.np_dtype.itemsize
        for f0 in range(0, F if n else 0, 16):       # the library takes 16 fields a call
            self._grid.fields(eng.np_dtype, ptrs[f0:f0 + 16], pitch, first, n, out.data_ptr() + f0 * opitch * esz,
                              opitch, where=_lib.DEVICE, stream=eng._stream())
        return out

    def composite(self, cls, drivers, day_hours, days, period_days=8, every=None, coarse=MET_DRIVERS, first_pixel=0,
                  pet=False, min_valid=1, rescale=False, out=None):
        '''Enqueue the composite over coarse drivers on the current stream: what
        ``RasterEngine.composite`` returns for the ``n = cls.numel()`` pixels ``[first_pixel,
        first_pixel + n)`` of the raster (row-major) when each array named in ``coarse`` is
        materialised slab by slab with ``mod16_amd.downscale.interpolate`` -- bit for bit, counts
        included, without those ``(S, n)`` arrays ever existing (``mod16_et_composite_downscaled_*``).

        ``coarse`` names arrays of ``mod16_amd.composite.ARRAY_NAMES`` (default: the eleven reanalysis
        drivers; ``'day_hours'`` may be among them). A coarse array is an ``(H, W)`` tensor (constant in
        time) or an ``(S, H, W)`` tensor with ``S = ceil(days / every[name])``, unit stride in columns,
        one row pitch >= W for all of them and any stride in time of at least a plane (views of
        larger tensors are fine). Every other array is what ``RasterEngine.composite`` takes: a
        scalar, an ``(n,)`` or an ``(S, n)`` tensor of the range's pixels. ``days``, ``period_days``,
        ``every``, ``pet``, ``min_valid``, ``rescale`` and ``out`` as there; returns what it returns.
        Asynchronous: call the engine's ``check()`` before trusting the data; a class code >= 13
        raises IndexError there.'''
        from . import composite as _c, downscale as _d
        eng, torch = self.engine, _torch()
        K, L, mv, P = _c.check_periods(days, period_days, min_valid)
        ev = _c.check_every(every)
        if eng.math & ~_lib.MATH_EXACT:
            raise ValueError('composite needs an engine with MATH_FAST or MATH_EXACT (no MATH_MIXED, not trusted)')
        names = _d.check_coarse_arrays(coarse)
        if len(drivers) != _lib.N_DRIVERS:
            raise ValueError('expected 14 drivers')
        arrays = list(drivers) + [day_hours]
        n = cls.numel()
        shapes = [tuple(d.shape) if isinstance(d, torch.Tensor) and (name in names or d.dim() > 0) else ()
                  for name, d in zip(_c.ARRAY_NAMES, arrays)]
        kinds, slabs, first, n = _d.check_composite_call(self.shape, self.coarse_shape, shapes, K, ev, coarse=names,
                                                         first_pixel=first_pixel, n=n, cls_size=n)
        cptr = eng._check_tensor(cls, torch.uint8, n, 'cls')
        keep, ptrs, pstride, tstride, divisor, rows = [], [], [], [], [], []
        for name, d, kind, S in zip(_c.ARRAY_NAMES, arrays, kinds, slabs):
            if kind in (_d.KIND_COARSE, _d.KIND_COARSE_TIME):
                ptr, row, plane = self._coarse(d, name, series=True)
                rows.append(row)
                ps, ts, div = 0, (plane if S > 1 else 0), (ev[name] if kind == _d.KIND_COARSE_TIME else K)
            elif kind == _d.KIND_FINE:          # (contiguous: it may have the raster's shape)
                ptr, ps, ts, div = eng._check_tensor(d, eng.dtype, n, name), 1, 0, K
            else:
                d, ptr, ps, ts, div = eng._composite_array(name, d, n, K, ev)
            keep.append(d)
            ptrs.append(ptr)
            pstride.append(ps)
            tstride.append(ts)
            divisor.append(div)
        cpitch = _t.share_one(rows, 'the coarse arrays', 'distance between rows')
        out, pitch = eng._composite_outputs(out, P, n, pet)
        if n:
            optr = [o.data_ptr() for o in out]
            et, pt = (optr[0], optr[1]) if pet else (optr[0], None)
            c_et, c_pt = (optr[2], optr[3]) if pet else (optr[1], None)
            self._grid.composite(eng.np_dtype, n, K, L, cptr, ptrs, pstride, tstride, divisor, _d.coarse_mask(names),
                                 cpitch or self.coarse_shape[1], first, et, pt, c_et, c_pt, pitch, min_valid=mv,
                                 rescale=rescale, flags=eng.math, where=_lib.DEVICE, stream=eng._stream())
        return out

    def close(self):
        self._grid.close()


class ZonalSelection(object):
    '''The state of a radix selection of zonal quantiles on one device (``RasterEngine.zonal_selection``):
    ``hist`` ``(K, Z, S, 2**bits)`` int64, the digit histogram of the current ``level``; ``remaining`` and
    ``prefix`` ``(K, Z, S)`` int64 (the prefix holds the bits of an unsigned key); ``weight`` ``(K, Z)``;
    ``level``; ``done``. A level is ``add`` for every part of the raster, ``merge`` for every other device's
    selection, then ``select()``. The first ``add`` fixes the weight bound ``wmax`` of the selection.'''

    def __init__(self, engine, layers, nzones, q, bits=None):
        from . import zonal as _z, zonalq as _q
        torch = _torch()
        self.engine = engine
        self.q = _q.check_q(q)
        self.bits = _q.DEFAULT_BITS if bits is None else _q.check_bits(bits)
        self.layers, self.nzones = int(layers), _z.check_nzones(nzones)
        if not 1 <= self.layers <= _z.MAX_LAYERS:
            raise ValueError('between 1 and %d layers, got %d' % (_z.MAX_LAYERS, self.layers))
        self.width = 8 * engine.np_dtype.itemsize
        self.levels = _q.levels(self.width, self.bits)
        dev, shape = engine._dev(), (self.layers, self.nzones, len(self.q))
        self.hist = torch.zeros(shape + (1 << self.bits,), dtype=torch.int64, device=dev)
        self.remaining = torch.zeros(shape, dtype=torch.int64, device=dev)
        self.prefix = torch.zeros(shape, dtype=torch.int64, device=dev)
        self.weight = torch.zeros(shape[:2], dtype=torch.int64, device=dev)
        self.values = torch.full(shape, float('nan'), dtype=engine.dtype, device=dev)
        self.level, self.done = 0, False
        self.wmax = self.ew = None

    def _spec(self, n=0, zone_type=0, kind=0, cols=1, first_pixel=0, pitch=None, wmax=1.0, ew=31):
        return self.engine.ctx.zonal_hist_spec(self.engine.np_dtype, n, self.layers, self.nzones, zone_type, kind, cols,
                                               first_pixel, pitch, wmax, ew, bits=self.bits, level=self.level,
                                               slots=len(self.q))

    def add(self, values, zones, area=None, cols=None, first_pixel=0, wmax=None):
        '''Adds a part of the raster to the histogram of the current level (asynchronous). ``values``
        ``(K, n)``, ``zones``, ``area``, ``cols``, ``first_pixel``: as in ``RasterEngine.zonal``. ``wmax``: with an
        ``area``, the largest weight of the WHOLE raster -- every part and every level must use one
        bound; None takes the selection's (the first ``add`` finds it with the ``zonal_bounds`` pre-pass
        over its own part if none is given).'''
        from . import zonal as _z
        torch = _torch()
        if self.done:
            raise ValueError('the selection is finished')
        eng = self.engine
        K, n, pitch, kind, wptr, cols, first_pixel = eng._zonal_args(values, zones, area, cols, first_pixel)
        if K != self.layers:
            raise ValueError('values must have %d layers, got %d' % (self.layers, K))
        if wmax is None and self.wmax is not None:
            wmax = self.wmax
        wmax, ew = eng._zonalq_wmax(values, area, cols, first_pixel, kind, wmax)
        if self.wmax is not None and (wmax, ew) != (self.wmax, self.ew):
            raise ValueError('every part and level of a selection must use one wmax: %r, then %r' % (self.wmax, wmax))
        self.wmax, self.ew = wmax, ew
        if n:
            spec = self._spec(n, _z.ZONE_U8 if zones.dtype == torch.uint8 else _z.ZONE_I32, kind, cols, first_pixel, pitch, wmax, ew)
            try:
                eng.ctx.zonal_hist(spec, eng.np_dtype, values.data_ptr(), zones.data_ptr(), wptr,
                                   self.prefix.data_ptr() if self.level else None, self.hist.data_ptr(),
                                   where=_lib.DEVICE, stream=eng._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return self

    def merge(self, other):
        '''Adds another selection's histogram of the same level (another device's share of the pixels).'''
        if (other.level, other.bits, other.q, tuple(other.hist.shape)) != (self.level, self.bits, self.q, tuple(self.hist.shape)):
            raise ValueError('selections of another level, shape or q cannot be merged')
        if None not in (self.ew, other.ew) and (self.wmax, self.ew) != (other.wmax, other.ew):
            raise ValueError('selections with the bounds %r and %r cannot be merged' % (self.wmax, other.wmax))
        if self.ew is None:
            self.wmax, self.ew = other.wmax, other.ew
        self.hist += other.hist.to(self.hist.device)
        return self

    def adopt(self, other):
        '''Takes ``remaining`` and ``prefix`` of a selection that closed the level for all devices.'''
        self.remaining.copy_(other.remaining)
        self.prefix.copy_(other.prefix)
        self.weight.copy_(other.weight)
        self.values.copy_(other.values)
        self.hist.zero_()
        self.level, self.done = other.level, other.done
        return self

    def select(self):
        '''Closes the level on the device (``mod16_zonal_select``; asynchronous) and clears the histogram.'''
        from . import zonalq as _q
        if self.done:
            raise ValueError('the selection is finished')
        eng = self.engine
        last = self.level == self.levels - 1
        eng.ctx.zonal_select(self._spec(), self.hist.data_ptr(), self.remaining.data_ptr(), self.prefix.data_ptr(),
                             self.values.data_ptr() if last else None, self.weight.data_ptr() if self.level == 0 else None,
                             q=[_q.rational(v) for v in self.q] if self.level == 0 else None, where=_lib.DEVICE,
                             stream=eng._stream())
        self.hist.zero_()
        self.level += 1
        self.done = last
        return self

    def result(self):
        '''The ``ZonalQuantiles`` of a finished selection (downloads: waits).'''
        from . import zonalq as _q
        if not self.done:
            raise ValueError('the selection has %d of %d levels' % (self.level, self.levels))
        return _q.ZonalQuantiles(self.values.cpu().numpy(), self.weight.cpu().numpy(), self.q, 31 if self.ew is None else self.ew)


class RasterEngine(object):
    '''
    Parameters
    ----------
    table : numpy.ndarray
        (13, 11) BPLUT table (``mod16_amd.utils.bplut_table``)
    device : int
        GPU index (Default: the current torch device)
    dtype : str
        'float64' (default) or 'float32'
    math : int
        ``_lib.MATH_FAST`` (default), ``_lib.MATH_EXACT`` or, for float32
        rasters, ``_lib.MATH_MIXED`` (see ``include/mod16_hip.h``)
    trusted : bool
        ``MOD16_DOMAIN_TRUSTED``: the caller vouches that every driver lies inside
        the domain of the production arithmetic (quality-controlled or NaN-masked
        rasters; the bounds are in ``include/mod16_hip.h``) -- the totals form then
        runs without the domain test and without the dispatch that revisits flagged
        pixels (-1.6 % kernel time on the float64 global grid, -2.3 % MIXED: tools/guardcost.py, round 5).
        Default: False, the
        arithmetic that returns the reference's result on every input.
    '''

    def __init__(self, table, device=None, dtype='float64', math=_lib.MATH_FAST, trusted=False,
                 experiments=False):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.Mod16Error(
                _lib.ERR_NO_DEVICE, 'RasterEngine needs an MI355X; there is no CPU fallback')
        self.device = torch.cuda.current_device() if device is None else int(device)
        # a context of its own: the BPLUT set here is what this engine's launches
        # (and the graphs bound from it) read at run time, whatever table other
        # engines or the numpy entry points of the process use meanwhile
        # (experiments: a context of libmod16hip_exp.so, which reads the launch-geometry overrides
        # from the environment -- tests and tools only)
        self.ctx = _lib.Context(self.device, experiments=experiments)
        self.ctx.set_bplut(table)
        self.np_dtype = np.dtype(dtype)
        self.bytes_per_pixel = BYTES_PER_PIXEL[self.np_dtype.name]       # (float32 or float64: KeyError otherwise)
        self.dtype = _t.torch_dtype(self.np_dtype)
        self.math = int(math) | (_lib.DOMAIN_TRUSTED if trusted else 0)

    def _gate(self):
        '''A zero-work dispatch on the compute stream in front of a step of the series runners.
        Measured (round 4, 46-step series, generator on the second stream): with the persistent
        pipeline kernel enqueued directly behind its cross-stream event wait the step took 45 ms --
        the two kernels got in each other's way -- with one tiny dispatch between the wait and the
        kernel 38.5 ms, the sum of the two kernels alone (19.4 + 19.9 ms: both are bound by the same
        HBM). Round 3's launch sequence had such a dispatch by accident (the memset of the ticket
        counter, gone since the kernel resets it itself). Round 5, wall clock and kernel trace of both
        (``tools/gate_probe.py``, ``profiles/r05_gate_probe.json``): 39.4 ms per step with the gate = the sum
        of the kernels alone (39.2), 46.3 without; ``bench.py`` reports the ratio of every run
        (``configs.c4_series_float64.step_over_sum_of_kernels``, 1.004).'''
        torch = _torch()
        if getattr(self, '_gate_word', None) is None:
            self._gate_word = torch.zeros(64, dtype=torch.float32, device=self._dev())
        self._gate_word.zero_()

    #: bytes of one field per tile of a ``TiledRaster`` (16-64 KiB measured: 32 KiB best)
    TILE_BYTES = 32 * 1024

    # ---------------------------------------------------------- helpers
    def _dev(self):
        return _torch().device('cuda', self.device)

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _check_tensor(self, t, dtype, n, what):
        _t.check_device(t, what, self.device, dtype)
        if not t.is_contiguous():
            raise TypeError('%s must be contiguous %s' % (what, dtype))
        if t.numel() != n:
            raise ValueError('%s has %d elements, expected %d' % (what, t.numel(), n))
        return t.data_ptr()

    #: extra bytes between successive arrays of ``alloc_raster``: with arrays
    #: spaced by (a multiple of 4 KiB) + 0 or + 4 KiB the 16 concurrent streams
    #: collide in HBM (+6-9 % kernel time, measured); any offset >= 8 KiB
    #: is fine, 33 KiB measured best
    STAGGER_BYTES = 33 * 1024

    def _carve(self, slab, n, per):
        esz = self.np_dtype.itemsize
        views = [slab[k * per:k * per + n * esz].view(self.dtype) for k in range(16)]
        cls = slab[16 * per:16 * per + n]
        return cls, views[:14], views[14], views[15]

    def _pitch(self, n, extra):
        return (n * self.np_dtype.itemsize + 4095) // 4096 * 4096 + self.STAGGER_BYTES + int(extra)

    def alloc_raster(self, n, extra=0):
        '''Device arrays for one raster of n pixels in the layout the fused
        kernel streams best: class raster, 14 drivers and the two outputs are
        carved out of ONE allocation, successive arrays ``STAGGER_BYTES`` +
        ``extra`` bytes apart on top of their size (see ``alloc_raster_tuned``
        for ``extra``), so their relative placement in HBM does not depend on
        the allocator. Returns ``(cls, drivers, day, night)``.'''
        torch = _torch()
        per = self._pitch(n, extra)
        slab = torch.empty(16 * per + n + 4096, dtype=torch.uint8, device=self._dev())
        return self._carve(slab, n, per)

    #: candidate extra spacings between the arrays of a raster [bytes] that
    #: ``alloc_raster_tuned`` looks at
    TUNE_EXTRA = tuple(int(g * 2 ** 30) for g in (0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75))

    def alloc_raster_tuned(self, n, extras=None, launches=3, seed=16):
        '''``alloc_raster`` with the distance between the arrays chosen by
        measurement. The 16 streams of the fused kernel walk their arrays in
        lock step, and how far apart the arrays lie -- at the scale of
        hundreds of MiB -- changes the DRAM-side read latency and with it the
        kernel time by 5-9 % (43200 x 21600 float64: 21.9-22.5 ms with the
        arrays back to back, 21.0-21.2 ms with 0.5 GiB between them;
        DESIGN.md section 6, ``tools/layout_sweep.py``). Which spacing is best
        depends on the raster size and somewhat on where the allocation
        landed, so for a raster that stays resident this allocates one slab
        large enough for every candidate in ``extras`` (bytes, default
        ``TUNE_EXTRA``), times the production kernel on synthetic drivers
        for each and keeps the fastest -- a few launches per candidate,
        once, at set-up.

        Returns ``((cls, drivers, day, night), report)``; ``report`` maps each
        extra spacing to its milliseconds per launch and names the choice.
        The arrays hold the synthetic fields of ``seed``, to be overwritten.'''
        torch = _torch()
        extras = [int(e) for e in (self.TUNE_EXTRA if extras is None else extras)]
        per_max = self._pitch(n, max(extras))
        slab = torch.empty(16 * per_max + n + 4096, dtype=torch.uint8, device=self._dev())
        times = {}
        for e in extras:
            cand = self._carve(slab, n, self._pitch(n, e))
            self.synth(n, seed=seed, out=(cand[0], cand[1]))
            self.time_kernel(cand[0], cand[1], cand[2], cand[3], launches=1)
            times[e] = self.time_kernel(cand[0], cand[1], cand[2], cand[3], launches=launches)
        best = min(times, key=times.get)
        report = {'extra_bytes_ms': {str(e): round(ms, 4) for e, ms in times.items()},
                  'chosen_extra_bytes': best}
        return self._carve(slab, n, self._pitch(n, best)), report

    def empty(self, n, count=1):
        torch = _torch()
        return [torch.empty(n, dtype=self.dtype, device=self._dev()) for _ in range(count)]

    def _marshal_drivers(self, drivers, n):
        torch = _torch()
        if len(drivers) != _lib.N_DRIVERS:
            raise ValueError('expected 14 drivers')
        keep, ptrs, strides = [], [], []
        for k, d in enumerate(drivers):
            if isinstance(d, torch.Tensor) and d.numel() != 1:
                ptrs.append(self._check_tensor(d, self.dtype, n, 'driver %d' % k))
                strides.append(1)
                keep.append(d)
            else:       # broadcast scalar
                s = torch.as_tensor(d, dtype=self.dtype).reshape(1).to(self._dev())
                keep.append(s)
                ptrs.append(s.data_ptr())
                strides.append(0)
        return keep, ptrs, strides

    # -------------------------------------------------------------- API
    def synth(self, n, seed=16, step=0, pixel_offset=0, out=None):
        '''Fill (or allocate) the class raster and the 14 driver tensors for
        global pixels [pixel_offset, pixel_offset + n) on the device
        (``mod16_synth_*``). Returns ``(cls, drivers)``.'''
        torch = _torch()
        if out is None:
            cls = torch.empty(n, dtype=torch.uint8, device=self._dev())
            drivers = self.empty(n, _lib.N_DRIVERS)
        else:
            cls, drivers = out
        fn = _lib.typed(self.ctx.lib, 'mod16_synth', self.np_dtype)
        ptrs = [self._check_tensor(d, self.dtype, n, 'driver') for d in drivers]
        self.ctx.check(fn(
            self.ctx.handle, int(seed), int(step), int(pixel_offset), int(n),
            self._check_tensor(cls, torch.uint8, n, 'cls'),
            _lib.ptr_array(ptrs), self._stream()))
        return cls, drivers

    def run(self, cls, drivers, out_day=None, out_night=None, out_sep=None, diag=None):
        '''Enqueue the fused ET kernel on the current stream; returns
        ``(day, night)`` tensors (allocated unless given). With ``diag`` (a
        float64 tensor of 8 on the device) the diagnostics vector
        (``DIAG_FIELDS``) is produced in the same pass (``mod16_et_diag_*``).
        Asynchronous: call ``check()`` (or synchronise the stream) before
        trusting the data.'''
        torch = _torch()
        n = cls.numel()
        cptr = self._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = self._marshal_drivers(drivers, n)
        if out_day is None and out_sep is None:
            out_day, out_night = self.empty(n, 2)
        pd = self._check_tensor(out_day, self.dtype, n, 'out_day') if out_day is not None else None
        pn = self._check_tensor(out_night, self.dtype, n, 'out_night') if out_night is not None else None
        if diag is not None:
            if out_sep is not None:
                raise ValueError('diag and out_sep cannot be combined')
            fn = _lib.typed(self.ctx.lib, 'mod16_et_diag', self.np_dtype)
            self.ctx.check(fn(
                self.ctx.handle, cptr, _lib.ptr_array(dptr), _lib.i64_array(dstride), n,
                pd, pn, int(self.math),
                self._check_tensor(diag, torch.float64, 8, 'diag'), self._stream()))
            return out_day, out_night
        sep = None
        if out_sep is not None:
            sep = [self._check_tensor(t, self.dtype, n, 'out_sep') if t is not None else None
                   for t in out_sep]
        self.ctx.et(self.np_dtype, cptr, dptr, dstride, None, None, n, pd, pn, sep,
                    flags=self.math, where=_lib.DEVICE, stream=self._stream())
        return out_day, out_night

    def composite(self, cls, drivers, day_hours, days, period_days=8, every=None, pet=False,
                  min_valid=1, rescale=False, out=None):
        '''Enqueue the composite kernel on the current stream: per-pixel totals of ET over periods
        of ``period_days`` days [kg m-2 per period] from ``days`` days of device-resident drivers in
        one launch (``mod16_et_composite_*``; the definition is ``mod16_amd.composite``) -- ``days=8,
        period_days=8`` is one MOD16A2 value per pixel, ``days=365, period_days=365`` MOD16A3.

        ``cls`` is the ``(n,)`` class raster. Each of the 14 ``drivers`` and ``day_hours`` (hours of
        daylight) is a scalar, an ``(n,)`` tensor (constant in time) or an ``(S, n)`` tensor with unit
        stride in pixels and any stride in time (views of a larger buffer are fine), where ``S =
        ceil(days / every[name])``: day ``t`` reads row ``t // every[name]``. ``every`` maps names of
        ``mod16_amd.composite.ARRAY_NAMES`` to divisors (default 1: daily; 8 for 8-day fPAR / LAI /
        albedo). A day counts where its total is not NaN; a period with fewer than ``min_valid`` such
        days is NaN; ``rescale`` brings a period with missing days to its full length.

        Returns ``(et, count)``, or with ``pet`` ``(et, pet, count_et, count_pet)``: totals in the
        engine's dtype and uint16 counts of valid days, each ``(P, n)`` with ``P = ceil(days /
        period_days)``. ``out`` may give them: rows of unit stride, all with the same distance
        between rows. The engine's ``math`` must be ``MATH_FAST`` or ``MATH_EXACT``. Asynchronous:
        call ``check()`` (or synchronise the stream) before trusting the data; a class code >= 13
        raises IndexError there.'''
        from . import composite as _c
        torch = _torch()
        K, L, mv, P = _c.check_periods(days, period_days, min_valid)
        ev = _c.check_every(every)
        if self.math & ~_lib.MATH_EXACT:
            raise ValueError('composite needs an engine with MATH_FAST or MATH_EXACT (no MATH_MIXED, not trusted)')
        if len(drivers) != _lib.N_DRIVERS:
            raise ValueError('expected 14 drivers')
        n = cls.numel()
        cptr = self._check_tensor(cls, torch.uint8, n, 'cls')
        keep, ptrs, pstride, tstride, divisor = zip(*[
            self._composite_array(name, d, n, K, ev) for name, d in zip(_c.ARRAY_NAMES, list(drivers) + [day_hours])])
        out, pitch = self._composite_outputs(out, P, n, pet)
        if n:
            optr = [o.data_ptr() for o in out]
            et, pt = (optr[0], optr[1]) if pet else (optr[0], None)
            c_et, c_pt = (optr[2], optr[3]) if pet else (optr[1], None)
            self.ctx.composite(self.np_dtype, n, K, L, cptr, ptrs, pstride, tstride, divisor, et, pt, c_et, c_pt,
                               pitch, min_valid=mv, rescale=rescale, flags=self.math, where=_lib.DEVICE,
                               stream=self._stream())
        return out

    def _composite_array(self, name, d, n, K, every):
        '''One array of a composite call given per pixel -- a scalar, an ``(n,)`` or an ``(S, n)`` tensor
        -- -> (the tensor to keep alive, address, pixel stride, stride in time, divisor of the day).'''
        from . import composite as _c
        torch = _torch()
        if not isinstance(d, torch.Tensor) or d.dim() == 0:       # broadcast scalar, constant in time
            sc = torch.as_tensor(d, dtype=self.dtype).reshape(1).to(self._dev())
            return sc, sc.data_ptr(), 0, 0, K
        ptr, ts = _t.series(d, name, n, self.device, self.dtype)
        if d.dim() == 2:
            _c.check_slabs(name, d.shape[0], K, every[name])
        return d, ptr, 1, ts, every[name] if d.dim() == 2 else K

    def _composite_outputs(self, out, P, n, pet):
        '''The 2 (``pet``: 4) ``(P, n)`` result tensors of a composite call -- new ones, or the caller's
        ``out`` after a check -- and their common distance between rows.'''
        totals = 2 if pet else 1
        table = {k: ((P, n), self.np_dtype if k < totals else np.dtype(np.uint16)) for k in range(2 * totals)}
        outs, rows = _t.named_outputs(out, table, self.device, 'distance between rows')
        return tuple(outs.values()), _t.share_one(rows.values(), 'the out tensors', 'distance between rows')

    def downscale_grid(self, shape, coarse_shape, row_pos, col_pos=None, wrap=False, method='bilinear',
                       col_affine=None):
        '''The geometry of an ``R x C`` fine raster (``shape``) over an ``H x W`` coarse grid
        (``coarse_shape``) on this engine's device -> ``DownscaleGrid``. ``row_pos[R]`` and
        ``col_pos[C]`` are the positions of the fine rows and columns in units of coarse cells, cell
        centres at the integers (``mod16_amd.downscale.positions`` builds them for regular grids);
        ``wrap``: the coarse column axis is periodic (a global longitude axis); ``method``:
        ``'nearest'``, ``'bilinear'`` or ``'cos4'`` (``mod16_amd.downscale.corner_tables``).

        For a fine grid whose column mapping depends on the row (a MODIS sinusoidal tile:
        ``mod16_amd.downscale.sinusoidal_positions``) give ``col_affine = (col_origin[R],
        col_scale[R])`` instead of ``col_pos``: the column position of pixel ``(r, c)`` is
        ``col_origin[r] + col_scale[r] * c`` and the kernels form its cell pair and weights per
        pixel (``mod16_amd.downscale.corner_tables_rows``; ``'nearest'`` or ``'bilinear'``). Exactly
        one of the two must be given.'''
        return DownscaleGrid(self, shape, coarse_shape, row_pos, col_pos, wrap=wrap, method=method,
                             col_affine=col_affine)

    def upscale_grid(self, shape, coarse_shape, row_pos, col_pos=None, wrap=False, area=None, col_affine=None, col_range=None):
        '''The cells of an ``H x W`` coarse grid (``coarse_shape``) in an ``R x C`` fine raster (``shape``)
        on this engine's device -> ``UpscaleGrid``, the opposite direction of ``downscale_grid`` with the
        same position tables: ``row_pos[R]`` and ``col_pos[C]`` in units of coarse cells, cell centres at
        the integers (``mod16_amd.downscale.positions``). A pixel belongs to the cell its centre lies in,
        a pixel outside the grid to none; ``wrap``: the coarse column axis is periodic; ``area[R]``: the
        weight of a pixel of that fine row (``cos(latitude)``; default 1). Exactly one of ``col_pos`` and
        ``col_affine`` is given: ``col_affine = (col_origin[R], col_scale[R])`` are row-affine columns (a
        sinusoidal tile, ``mod16_amd.downscale.sinusoidal_positions``), the column position of pixel ``(r,
        c)`` being ``col_origin[r] + col_scale[r] * c``; ``col_range = (col_first[R], col_count[R])``
        (int32; ``downscale.sinusoidal_columns``) then names the columns of every fine row that can
        belong to a cell, the others being neither counted nor read. With ``wrap`` a fine row must not
        span the whole periodic axis (``mod16_amd.upscale.check_rows``).'''
        return UpscaleGrid(self, shape, coarse_shape, row_pos, col_pos, wrap=wrap, area=area, col_affine=col_affine,
                           col_range=col_range)

    def gapfill(self, fields, qc=None, good=None, max_gap=None, fallback=None, dtype=None, scale=None,
                source=False, out=None):
        '''Enqueue the gap-filling kernel on the current stream: the annual profile of every pixel
        of one to three device-resident byte series (MOD15A2H fPAR / LAI codes) filled in one launch
        (``mod16_gapfill_u8``; the definition is ``mod16_amd.gapfill``) -- unreliable slabs are
        interpolated between the nearest reliable ones, held at the ends of the series, and beyond
        ``max_gap`` take ``fallback`` or stay unfilled.

        ``fields`` is one ``(S, n)`` uint8 tensor or a tuple of up to three, ``qc`` an optional one
        shared by them, each with unit stride in pixels and any stride >= n in time (views of a
        larger buffer are fine, at any byte offset); ``good`` a 256-entry table of acceptable QC bytes
        (default ``mod16_amd.gapfill.default_good()``); ``fallback`` one ``(n,)`` uint8 tensor (or
        None) per field. ``dtype``: ``'uint8'`` (default: codes, 255 where unfilled -- a row goes into
        ``run_raw``), ``'float32'`` / ``'float64'``, or ``'engine'``: the engine's type, where
        ``scale`` defaults to 0.01 and 0.1 for two fields (fPAR, LAI: fractions and m2 m-2, NaN where
        unfilled -- what ``composite(..., every={'fpar': 8, 'lai': 8})`` takes).

        Returns the filled tensor (a tuple for a tuple of fields), and with ``source`` a pair
        ``(filled, source)``: per field the ``(S, n)`` bytes 0 observed, 1 interpolated, 2 held, 3
        fallback, 4 unfilled. ``out`` may give the filled tensors (and, with ``source``, one ``(fields,
        S, n)`` uint8 tensor behind them); no output may overlap an input. Asynchronous, like
        ``composite``.'''
        from . import gapfill as _g
        torch = _torch()
        single = isinstance(fields, torch.Tensor)
        flds = [fields] if single else list(fields)
        if fallback is not None and isinstance(fallback, torch.Tensor):
            fallback = [fallback]
        engine = dtype == 'engine'
        if dtype is None:
            dtype = 'uint8'
        elif engine:
            dtype = self.np_dtype.name
            if scale is None and len(flds) == 2:
                scale = (0.01, 0.1)
        for what, t in [('fields[%d]' % k, f) for k, f in enumerate(flds)] + [('qc', qc)] + \
                [('fallback[%d]' % k, f) for k, f in enumerate(fallback or [])]:
            if t is not None or what.startswith('fields'):
                _t.check_device(t, what, self.device, torch.uint8)
        S, shape, table, mg, name, scales = _g.check_series(
            [tuple(f.shape) for f in flds], None if qc is None else tuple(qc.shape), good, max_gap,
            None if fallback is None else [None if f is None else tuple(f.shape) for f in fallback], dtype, scale)
        if len(shape) != 1:
            raise ValueError('fields must be (S, n) tensors, got %r' % (tuple(flds[0].shape),))
        n = shape[0]
        in_pitch = _t.share_one([_t.row_pitch(f, 'fields[%d]' % k, 'stride in time') for k, f in enumerate(flds)],
                                'the fields', 'stride in time')
        qc_pitch = _t.row_pitch(qc, 'qc', 'stride in time') if qc is not None else n
        for k, f in enumerate(fallback or []):
            if f is not None:
                _t.row_pitch(f, 'fallback[%d]' % k)
        if out is None:
            src = torch.empty((len(flds), S, n), dtype=torch.uint8, device=self._dev()) if source else None
        else:                      # (the source tensor comes behind the filled ones)
            out = [out] if isinstance(out, torch.Tensor) else list(out)
            if len(out) != len(flds) + (1 if source else 0):
                raise ValueError('out must hold %d tensors' % (len(flds) + (1 if source else 0)))
            src = out.pop() if source else None
        outs, rows = _t.named_outputs(out, {k: ((S, n), np.dtype(name)) for k in range(len(flds))}, self.device,
                                      'stride in time')
        outs = list(outs.values())
        out_pitch = _t.share_one(rows.values(), 'the out tensors', 'distance between rows')
        src_pitch = n
        if src is not None:
            _t.check_device(src, 'source', self.device, torch.uint8)
            if tuple(src.shape) != (len(flds), S, n):
                raise TypeError('source must have shape (%d, %d, %d)' % (len(flds), S, n))
            src_pitch = _t.row_pitch(src, 'source', 'stride in time')
            if len(flds) > 1 and src.stride(0) != S * src_pitch:
                raise ValueError('the source tensor must hold its fields back to back')
        if n:
            good8 = None
            if good is not None:       # (the default table is the library's own)
                good8 = torch.from_numpy(np.ascontiguousarray(table, np.uint8)).to(self._dev())
            try:
                self.ctx.gapfill(
                    _g.OUT_TYPES[name], n, S, [f.data_ptr() for f in flds], None if qc is None else qc.data_ptr(),
                    None if good8 is None else good8.data_ptr(),
                    None if fallback is None else [None if f is None else f.data_ptr() for f in fallback],
                    [o.data_ptr() for o in outs], None if src is None else src.data_ptr(), in_pitch, qc_pitch,
                    out_pitch, src_pitch, max_gap=mg, scale=scales + [1.0] * (3 - len(scales)),
                    where=_lib.DEVICE, stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        filled = outs[0] if single else tuple(outs)
        if not source:
            return filled
        return filled, (src[0] if single else tuple(src[f] for f in range(len(flds))))

    def smooth(self, values, weights=None, qc=None, qc_weight=None, lam=None, order=2, envelope=0, min_valid=3,
               dtype=None, scale=None, count=False, out=None):
        '''Enqueue the Whittaker smoother on the current stream: the profile of every pixel of one
        device-resident series smoothed in one launch (``mod16_smooth_*``; the definition is
        ``mod16_amd.smooth``, whose bits the result has) -- per pixel the banded solve of ``(W + lam
        D'D) z = W y`` and ``envelope`` passes towards the upper envelope of the weighted values.

        ``values`` is an ``(S, n)`` uint8, float32 or float64 tensor; ``weights`` an optional float32
        one or ``qc`` an optional uint8 one, each with unit stride in pixels and any stride >= n in
        time (views of a larger buffer are fine, at any element offset); ``qc_weight`` a 256-entry
        table of weights per QC byte (default: 1 for the codes ``gapfill`` accepts, else 0). ``dtype``:
        for uint8 values ``'uint8'`` (default: codes, 255 where unsmoothed -- a row goes into
        ``run_raw``), ``'float32'`` / ``'float64'`` or ``'engine'`` (the engine's type; ``scale``
        applies); float values return their own type. The other arguments are those of
        ``mod16_amd.smooth_series``.

        Returns the smoothed tensor, and with ``count`` a pair ``(smoothed, count)``, ``count`` being
        the ``(n,)`` uint16 number of weighted slabs. ``out`` may give the tensors; no output may
        overlap an input. Asynchronous, like ``gapfill``.'''
        from . import smooth as _s
        torch = _torch()
        _t.check_device(values, 'values', self.device, torch.uint8, torch.float32, torch.float64)
        if weights is not None:
            _t.check_device(weights, 'weights', self.device, torch.float32)
        if qc is not None:
            _t.check_device(qc, 'qc', self.device, torch.uint8)
        if dtype == 'engine':
            dtype = self.np_dtype.name
        S, shape, mode, table, lam, order, envelope, min_valid, name, scale = _s.check_call(
            tuple(values.shape), _t.numpy_dtype(values.dtype), None if weights is None else tuple(weights.shape),
            None if qc is None else tuple(qc.shape), qc_weight, lam, order, envelope, min_valid, dtype, scale)
        if len(shape) != 1:
            raise ValueError('values must be an (S, n) tensor, got %r' % (tuple(values.shape),))
        n = shape[0]
        in_pitch = _t.row_pitch(values, 'values', 'stride in time')
        stack = weights if weights is not None else qc
        w_pitch = n if stack is None else _t.row_pitch(stack, 'weights' if weights is not None else 'qc', 'stride in time')
        if out is not None:
            out = [out] if isinstance(out, torch.Tensor) else list(out)
            if len(out) != (2 if count else 1):
                raise ValueError('out must hold %d tensors' % (2 if count else 1))
        outs, rows = _t.named_outputs(None if out is None else out[:1], {0: ((S, n), np.dtype(name))}, self.device,
                                      'stride in time')
        smoothed, out_pitch = outs[0], rows[0]
        cnt = None
        if count:
            if out is None:
                cnt = torch.empty((n,), dtype=torch.uint16, device=self._dev())
            else:
                cnt = out[1]
                _t.check_device(cnt, 'out[1]', self.device, torch.uint16)
                if tuple(cnt.shape) != (n,):
                    raise ValueError('out[1] must have shape %r, got %r' % ((n,), tuple(cnt.shape)))
                _t.row_pitch(cnt, 'out[1]')
        if n:
            table64 = None
            if qc_weight is not None:       # (the default table is the library's own)
                table64 = torch.from_numpy(np.ascontiguousarray(table, np.float64)).to(self._dev())
            try:
                self.ctx.smooth(
                    _t.numpy_dtype(values.dtype), _s.OUT_TYPES[name], n, S, values.data_ptr(),
                    None if stack is None else stack.data_ptr(), None if table64 is None else table64.data_ptr(),
                    smoothed.data_ptr(), None if cnt is None else cnt.data_ptr(), in_pitch, w_pitch, out_pitch, lam,
                    order=order, envelope=envelope, min_valid=min_valid, weight_mode=mode, scale=scale,
                    where=_lib.DEVICE, stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return (smoothed, cnt) if count else smoothed

    def regress(self, values, design=None, terms=(), weights=None, min_valid=None, stderr=False, series=None,
                out=None):
        '''Enqueue the regression kernel on the current stream: per pixel the weighted least-squares fit
        ``y = X b`` over a device-resident stack, every output in one launch (``mod16_regress_*``; the
        definition is ``mod16_amd.regress``, whose bits the result has).

        ``values`` is one ``(T, n)`` float32 or float64 tensor, ``1 <= T <= 4096``, with unit stride in
        pixels and any stride >= n in time (a view of a larger buffer is fine, at any element offset);
        a value that is not finite is missing. ``design``: the ``(T, Ks)`` float64 columns every pixel
        shares, as a numpy array (checked finite, uploaded) or as a contiguous float64 tensor on the
        engine's device (its values are the caller's: they must be finite); ``terms``: ``Kp`` per-pixel
        predictors, tensors of ``values``' shape and dtype that share one stride in time; ``1 <= Ks +
        Kp <= 8``. ``weights``: an optional float32 tensor of that shape. The other arguments are those
        of ``mod16_amd.regress_series``.

        Returns ``Regression(coef, stderr, rss, tss, r2, count, series)``: ``coef`` / ``stderr`` ``(Ks +
        Kp, n)``, ``rss`` / ``tss`` / ``r2`` ``(n,)`` float64, ``count`` ``(n,)`` uint16, ``series``
        ``(T, n)`` in the dtype of ``values``; ``stderr`` and ``series`` are None where they are not
        asked for. ``out`` may give the tensors as a dict by name (exactly the fields produced); no
        output may overlap an input. Asynchronous, like ``smooth``.'''
        from . import regress as _r
        torch = _torch()
        _t.check_device(values, 'values', self.device, torch.float32, torch.float64)
        if values.dim() != 2:
            raise ValueError('values must be a (T, n) tensor, got %r' % (tuple(values.shape),))
        terms = list(terms)
        for k, t in enumerate(terms):
            _t.check_device(t, 'terms[%d]' % k, self.device, values.dtype)
        if weights is not None:
            _t.check_device(weights, 'weights', self.device, torch.float32)
        on_device = isinstance(design, torch.Tensor)
        if on_device:
            _t.check_device(design, 'design', self.device, torch.float64)
        dtype = _t.numpy_dtype(values.dtype)
        T, shape, Ks, Kp, min_valid, stderr, code = _r.check_call(
            tuple(values.shape), dtype, None if design is None else tuple(design.shape), [tuple(t.shape) for t in terms],
            [dtype] * len(terms), None if weights is None else tuple(weights.shape), min_valid, stderr, series)
        if on_device:
            if not design.is_contiguous():
                raise ValueError('design must be contiguous')
            design64 = design
        else:
            design64 = _r.check_design(design, T)
        n = shape[0]
        value_pitch = _t.row_pitch(values, 'values', 'stride in time')
        term_pitch = _t.share_one([_t.row_pitch(t, 'terms[%d]' % k, 'stride in time') for k, t in enumerate(terms)],
                                  'the terms', 'stride in time')
        weight_pitch = None if weights is None else _t.row_pitch(weights, 'weights', 'stride in time')
        outs, pitch = _t.named_outputs(out, _r.output_table(shape, T, Ks + Kp, dtype, stderr, code), self.device,
                                       'stride in time')
        if n:
            if Ks and not on_device:
                design64 = torch.from_numpy(design64).to(self._dev())

            def address(k):
                return outs[k].data_ptr() if k in outs else None
            try:
                self.ctx.regress(
                    dtype, n, T, values.data_ptr(), design64.data_ptr() if Ks else None, Ks, [t.data_ptr() for t in terms],
                    None if weights is None else weights.data_ptr(), address('coef'), address('stderr'), address('rss'),
                    address('tss'), address('r2'), address('count'), address('series'), value_pitch=value_pitch,
                    term_pitch=term_pitch, weight_pitch=weight_pitch, coef_pitch=pitch['coef'], se_pitch=pitch.get('stderr'),
                    series_pitch=pitch.get('series'), min_valid=min_valid, series_mode=code, where=_lib.DEVICE,
                    stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return _r.Regression(*[outs.get(k) for k in _r.Regression._fields])

    def daynight(self, fields, half_day=None, noon=None, offset=None, sw_threshold=None, steps_per_day=24,
                 outputs=None, dtype=None, out=None):
        '''Enqueue the day / night aggregation on the current stream: hourly reanalysis fields in, the
        coarse planes ``DownscaleGrid.composite`` and ``DownscaleGrid.run`` take out
        (``mod16_daynight_*``; the definition is ``mod16_amd.daynight``).

        ``fields`` is a dict of device tensors by name -- ``'t'``, ``'qv'``, ``'ps'``, ``'sw'``, ``'lw'``,
        those the requested outputs need -- each ``(D * H, R, W)`` with ``H = steps_per_day``, all
        float32 or all float64, unit stride in columns and one row pitch >= W and one stride in time
        of at least a plane for all of them (views of larger tensors are fine). The day weights come
        from the float64 host tables ``half_day[D, R]``, ``noon[D]`` (default 12) and ``offset[W]``
        (``mod16_amd.daynight.solar_tables``), or, with ``sw_threshold``, from ``sw > sw_threshold``.
        ``outputs``: names of ``mod16_amd.daynight.OUTPUT_NAMES`` and ``'temp_annual'`` (default:
        every one the fields given allow); ``dtype``: ``'float32'`` or ``'float64'`` (default: the
        engine's, what its ``downscale_grid`` takes).

        Returns ``(DayNight, temp_annual)``: ``(D, R, W)`` tensors and one ``(R, W)`` tensor with one
        common row pitch, None where an output was not requested. ``sw_rad_night`` is not produced:
        pass 0.0. ``out`` may give the tensors as a dict by name (one row pitch and one stride in
        time for all; what lies between the rows is not touched); no output may overlap an input.
        Asynchronous, like ``composite``.'''
        from . import daynight as _dn
        torch = _torch()
        flds = {k: v for k, v in dict(fields).items() if v is not None}
        for k, t in flds.items():
            _t.check_device(t, "fields['%s']" % k, self.device, torch.float32, torch.float64)
        D, H, R, W, mode, tables, threshold, names = _dn.check_call(
            {k: tuple(t.shape) for k, t in flds.items()}, steps_per_day, half_day, noon, offset, sw_threshold, outputs)
        in_types = set(t.dtype for t in flds.values())
        if len(in_types) != 1:
            raise ValueError('fields must be all float32 or all float64')
        in_dtype = _t.numpy_dtype(in_types.pop())
        out_dtype = _dn.check_out_dtype(self.np_dtype if dtype is None else dtype, in_dtype)
        both = 'distance between rows and one stride in time'
        in_pitch, in_plane = _t.share_one([_t.plane_layout(t, "fields['%s']" % k) for k, t in flds.items()],
                                          'the fields', both)
        outs, lay = _t.named_outputs(out, _dn.output_table(names, D, R, W, out_dtype), self.device,
                                     called='requested outputs')
        out_pitch = _t.share_one([p for p, _ in lay.values()], 'the out tensors', both)
        out_plane = _t.share_one([q for n, (_, q) in lay.items() if n != 'temp_annual' and D > 1],
                                 'the out tensors', both)
        if out_pitch is None:
            out_pitch = W
        if out_plane is None:
            out_plane = (R - 1) * out_pitch + W
        if D and R and W:
            try:
                self.ctx.daynight(
                    in_dtype, _dn.OUT_TYPES[out_dtype.name], R, W, D, H,
                    [flds[f].data_ptr() if f in flds else None for f in _dn.FIELD_NAMES], tables,
                    [outs[n].data_ptr() if n in outs else None for n in _dn.OUTPUT_NAMES],
                    outs['temp_annual'].data_ptr() if 'temp_annual' in outs else None, in_pitch, in_plane,
                    out_pitch, out_plane, mode=_dn.MODES[mode], threshold=threshold, where=_lib.DEVICE,
                    stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return _dn.DayNight(*[outs.get(n) for n in _dn.OUTPUT_NAMES]), outs.get('temp_annual')

    def trend(self, values, times=None, min_valid=4, alpha=None, out=None):
        '''Enqueue the trend kernel on the current stream: per pixel the Mann-Kendall test and the
        Theil-Sen slope over a device-resident stack of composites, all outputs in one launch
        (``mod16_trend_*``; the definition is ``mod16_amd.trend``, which the result equals bit for bit).

        ``values`` is one ``(Y, n)`` float32 or float64 tensor, ``2 <= Y <= 64``, with unit stride in
        pixels and any stride >= n in time (a view of a larger buffer is fine, at any element
        offset); NaN and the infinities are missing. A stack ``(Y, P, n)`` -- one trend per 8-day
        period -- is the same call on its ``(Y, P * n)`` view. ``times``: ``(Y,)`` host values, finite
        and strictly increasing (default ``arange(Y)``); ``min_valid``: fewest valid values a trend is
        computed from; ``alpha``: a level in (0, 0.5] for the slope's interval (default: none).

        Returns ``Trend(slope, intercept, slope_lo, slope_hi, s, z, count)`` of ``(n,)`` tensors:
        float64, ``s`` int32, ``count`` uint8; ``slope_lo`` / ``slope_hi`` are None without ``alpha``.
        ``out`` may give the tensors as a dict by name (exactly the fields produced, contiguous); no
        output may overlap the input. Asynchronous, like ``composite``.'''
        from . import trend as _tr
        torch = _torch()
        _t.check_device(values, 'values', self.device, torch.float32, torch.float64)
        if values.dim() != 2:
            raise ValueError('values must be a (Y, n) tensor, got %r' % (tuple(values.shape),))
        Y, shape, t, min_valid, zq = _tr.check_call(tuple(values.shape), times, min_valid, alpha)
        n = shape[0]
        stride = _t.row_pitch(values, 'values', 'stride in time')
        outs, _ = _t.named_outputs(out, _tr.output_table(shape, zq), self.device, 'distance between rows')
        if n:
            try:
                self.ctx.trend(
                    _t.numpy_dtype(values.dtype), n, Y, values.data_ptr(), t,
                    [outs[k].data_ptr() if k in outs else None for k in _tr.FLOAT_NAMES], outs['s'].data_ptr(),
                    outs['count'].data_ptr(), time_stride=stride, min_valid=min_valid, zq=zq, where=_lib.DEVICE,
                    stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return _tr.Trend(*[outs.get(k) for k in _tr.Trend._fields])

    def anomaly(self, num, den=None, periods=None, window=1, baseline=None, min_valid=3, outputs=('z',), out=None):
        '''Enqueue the anomaly kernel on the current stream: per pixel and 8-day period the climatology
        of a device-resident record of composites over the baseline years, and per slab its
        standardized anomaly and percentile rank, in one launch (``mod16_anomaly_*``; the definition is
        ``mod16_amd.anomaly``, which the result equals bit for bit).

        ``num`` is one ``(S, n)`` float32 or float64 tensor, ``S = Y * periods`` slabs in time order
        (years outermost, ``2 <= Y <= 64``), with unit stride in pixels and any stride >= n in time (a
        view of a larger buffer is fine, at any element offset); ``den`` is None or a tensor of the same
        shape, dtype and stride in time -- the quantity is then the ratio, ET / PET say. ``window``
        sums that many periods into a value first (1 ... min(periods, 16)); ``baseline = (y0, y1)``
        takes the climatology from years ``y0 ... y1 - 1`` (default: all); ``min_valid``: fewest valid
        baseline values a climatology is computed from. NaN, the infinities and ``den <= 0`` are missing.

        Returns ``Anomaly(z, pct, mean, std, count)`` with the fields ``outputs`` names and None for the
        others: ``z`` / ``pct`` ``(S, n)`` in the input dtype, ``mean`` / ``std`` ``(periods, n)``
        float64, ``count`` ``(periods, n)`` uint8. ``out`` may give the tensors as a dict by name
        (exactly the fields produced; ``z`` and ``pct`` share one stride in time, the climatology
        another); no output may overlap an input. Asynchronous, like ``composite``.'''
        from . import anomaly as _an
        torch = _torch()
        _t.check_device(num, 'num', self.device, torch.float32, torch.float64)
        if num.dim() != 2:
            raise ValueError('num must be an (S, n) tensor, got %r' % (tuple(num.shape),))
        Y, P, shape, W, (y0, y1), min_valid = _an.check_call(tuple(num.shape), periods, window, baseline, min_valid)
        names = _an.check_outputs(outputs)
        S, n = Y * P, shape[0]
        in_stride = _t.row_pitch(num, 'num', 'stride in time')
        if den is not None:
            _t.check_device(den, 'den', self.device, num.dtype)
            _an.check_den_shape((S, n), den.shape)
            in_stride = _t.share_one([in_stride, _t.row_pitch(den, 'den', 'stride in time')], 'num and den', 'stride in time')
        dtype = _t.numpy_dtype(num.dtype)
        outs, pitch = _t.named_outputs(out, _an.output_table(names, S, P, shape, dtype), self.device, 'stride in time')
        out_stride = _t.share_one([pitch[k] for k in names if k in ('z', 'pct')], "out['z'] and out['pct']", 'stride in time')
        clim_stride = _t.share_one([pitch[k] for k in names if k not in ('z', 'pct')],
                                   "out['mean'], out['std'] and out['count']", 'stride between periods')
        if n:
            try:
                self.ctx.anomaly(
                    dtype, n, Y, P, num.data_ptr(), None if den is None else den.data_ptr(),
                    *[outs[k].data_ptr() if k in outs else None for k in _an.OUTPUT_NAMES], window=W, base_first=y0,
                    base_end=y1, min_valid=min_valid, in_stride=in_stride, out_stride=out_stride, clim_stride=clim_stride,
                    where=_lib.DEVICE, stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return _an.Anomaly(*[outs.get(k) for k in _an.OUTPUT_NAMES])

    def _zonal_args(self, values, zones, area, cols, first_pixel):
        '''The checks ``zonal`` and ``zonal_bounds`` share: -> (K, n, value pitch, weight kind, address
        of the weights or None, cols, first_pixel).'''
        torch = _torch()
        _t.check_device(values, 'values', self.device, self.dtype)
        if values.dim() != 2:
            raise ValueError('values must be a (K, n) tensor, got %r' % (tuple(values.shape),))
        K, n = values.shape
        pitch = _t.row_pitch(values, 'values')
        if zones is not None:
            _t.check_device(zones, 'zones', self.device, torch.uint8, torch.int32)
            if tuple(zones.shape) != (n,) or not zones.is_contiguous():
                raise ValueError('zones must have shape (%d,) and unit stride' % n)
        if area is None:
            return K, n, pitch, _lib.ZONAL_WEIGHT_NONE, None, 1, 0
        _t.check_device(area, 'area', self.device)
        if area.dim() != 1 or not area.is_contiguous():
            raise ValueError('area must be a vector with unit stride')
        if cols is None:
            if area.dtype != self.dtype or area.numel() != n:
                raise TypeError('per-pixel area must be a %s tensor of %d elements' % (self.dtype, n))
            return K, n, pitch, _lib.ZONAL_WEIGHT_PIXEL, area.data_ptr(), 1, 0
        cols, first_pixel = int(cols), int(first_pixel)
        if cols < 1 or first_pixel < 0:
            raise ValueError('cols must be at least 1 and first_pixel at least 0')
        if area.dtype != torch.float64:
            raise TypeError('per-row area must be a float64 tensor')
        if n and area.numel() < (first_pixel + n - 1) // cols + 1:
            raise ValueError('area holds %d rows, the pixel range reaches row %d'
                             % (area.numel(), (first_pixel + n - 1) // cols))
        return K, n, pitch, _lib.ZONAL_WEIGHT_ROW, area.data_ptr(), cols, first_pixel

    def zonal_bounds(self, values, area=None, cols=None, first_pixel=0):
        '''``(wmax, xmax)`` of a ``zonal`` call's inputs (``mod16_zonal_bounds_*``): the largest finite
        weight >= 0 and the largest finite ``|value|``; waits for the result.'''
        K, n, pitch, kind, wptr, cols, first_pixel = self._zonal_args(values, None, area, cols, first_pixel)
        if not n:
            return 1.0, 1.0
        return self.ctx.zonal_bounds(self.np_dtype, n, K, values.data_ptr(), wptr, weight_kind=kind, cols=cols,
                                     first_pixel=first_pixel, value_pitch=pitch, where=_lib.DEVICE, stream=self._stream())

    def zonal(self, values, zones, nzones, area=None, cols=None, first_pixel=0, bounds=None, acc=None):
        '''Enqueue the zonal reduction on the current stream: per zone and layer the exact weighted
        totals, count, minimum and maximum of device-resident values in one launch (``mod16_zonal_*``;
        the definition is ``mod16_amd.zonal``). The sums are integers: they do not depend on the order
        in which the pixels arrive, so calls that add parts of a raster into one ``acc`` give the
        words of one call over the whole.

        ``values`` is ``(K, n)`` in the engine's dtype with unit stride in pixels and any distance >= n
        between layers; ``zones`` ``(n,)`` uint8 or int32 (ids outside ``[0, nzones)`` are ignored);
        ``area`` None, a float64 vector with one weight per raster row (with ``cols``; pixel ``p``
        takes ``area[(first_pixel + p) // cols]``) or ``(n,)`` in the engine's dtype (``cols`` None).
        ``bounds``: ``(wmax, xmax)``; None runs the pre-pass (``zonal_bounds``, which waits for its
        result). ``acc``: a ``(K, nzones, 10)`` int64 tensor to add into (then ``bounds`` is
        mandatory, with the exponents the accumulator was started with); default a fresh one.

        Returns the accumulator tensor, with the exponents of the bounds recorded on it as
        ``.exponents``; ``mod16_amd.zonal.ZonalResult.from_tensor(acc)`` downloads it. Pixels beyond
        the bounds are counted in the ``rejected`` word. Asynchronous, like ``composite``.'''
        from . import zonal as _z
        torch = _torch()
        K, n, pitch, kind, wptr, cols, first_pixel = self._zonal_args(values, zones, area, cols, first_pixel)
        nzones = _z.check_nzones(nzones)
        if acc is not None:
            _z.check_acc_bounds(bounds)
            _t.check_device(acc, 'acc', self.device, torch.int64)
            if tuple(acc.shape) != (K, nzones, _z.NWORDS):
                raise ValueError('acc must have shape %r, got %r' % ((K, nzones, _z.NWORDS), tuple(acc.shape)))
            if not acc.is_contiguous():
                raise TypeError('acc must be contiguous %s' % torch.int64)
        if bounds is None:
            wmax, xmax = self.zonal_bounds(values, area, cols if kind == _lib.ZONAL_WEIGHT_ROW else None, first_pixel)
            bounds = (wmax if wmax > 0 else 1.0, xmax if xmax > 0 else 1.0)
        bounds = _z.check_bounds(bounds)
        if acc is not None and getattr(acc, 'exponents', bounds[2:]) != bounds[2:]:
            raise ValueError('the exponents of bounds %r differ from the accumulator\'s %r' % (bounds[2:], acc.exponents))
        if acc is None:
            acc = torch.from_numpy(_z.empty(K, nzones)).to(self._dev())
        acc.exponents = bounds[2:]
        if n:
            try:
                self.ctx.zonal(self.np_dtype, n, K, nzones, _z.ZONE_U8 if zones.dtype == torch.uint8 else _z.ZONE_I32,
                               values.data_ptr(), zones.data_ptr(), wptr, acc.data_ptr(), bounds, weight_kind=kind,
                               cols=cols, first_pixel=first_pixel, value_pitch=pitch, where=_lib.DEVICE,
                               stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return acc

    def _zonalq_wmax(self, values, area, cols, first_pixel, kind, wmax):
        '''``(wmax, ew)`` of a histogram call: ``(1.0, 31)`` without weights (a word is a count), else the
        given bound or, for None, what the ``zonal_bounds`` pre-pass finds (it waits for its result).'''
        from . import zonalq as _q
        if kind == _lib.ZONAL_WEIGHT_NONE:
            return 1.0, 31
        if wmax is None:
            wmax = self.zonal_bounds(values, area, cols if kind == _lib.ZONAL_WEIGHT_ROW else None, first_pixel)[0]
            wmax = wmax if wmax > 0 else 1.0
        return _q.check_wmax(wmax)

    def zonal_histogram(self, values, zones, nzones, bins, range, area=None, cols=None, first_pixel=0, wmax=None, acc=None):
        '''Enqueue the uniform zonal histogram on the current stream: per zone and layer the weight
        words of the valid pixels in ``bins`` equal bins over ``range = (lo, hi)``, with an under bin
        in front and an over bin behind (``mod16_zonal_hist_*``; the definition is
        ``mod16_amd.zonalq.histogram``). The words are integers: calls that add parts of a raster
        into one ``acc`` give the words of one call over the whole.

        ``values``, ``zones``, ``area``, ``cols``, ``first_pixel``: as in ``zonal``. ``wmax``: the largest
        weight the call accepts; None runs the ``zonal_bounds`` pre-pass (which waits for its result).
        ``acc``: a ``(K, nzones, bins + 2)`` int64 tensor to add into (then an ``area`` needs an explicit
        ``wmax``); default a fresh one.

        Returns the table tensor with ``ew`` (a word times ``2**(ew - 31)`` is a sum of weights; 31
        without weights: a count) and ``range`` recorded on it;
        ``mod16_amd.zonalq.ZonalHistogram(t.cpu().numpy(), *t.range, ew=t.ew)`` reads it. Asynchronous.'''
        from . import zonal as _z, zonalq as _q
        torch = _torch()
        K, n, pitch, kind, wptr, cols, first_pixel = self._zonal_args(values, zones, area, cols, first_pixel)
        nzones = _z.check_nzones(nzones)
        bins = _q.check_bins(bins)
        try:
            lo, hi = range
        except (TypeError, ValueError):
            raise ValueError('range must be a pair (lo, hi), got %r' % (range,))
        lo, hi, scale = _q.check_range(bins, lo, hi)
        if acc is not None:
            if kind != _lib.ZONAL_WEIGHT_NONE:
                _q.check_acc_wmax(wmax)
            _t.check_device(acc, 'acc', self.device, torch.int64)
            if tuple(acc.shape) != (K, nzones, bins + 2):
                raise ValueError('acc must have shape %r, got %r' % ((K, nzones, bins + 2), tuple(acc.shape)))
            if not acc.is_contiguous():
                raise TypeError('acc must be contiguous %s' % torch.int64)
        wmax, ew = self._zonalq_wmax(values, area, cols, first_pixel, kind, wmax)
        if acc is not None and getattr(acc, 'ew', ew) != ew:
            raise ValueError('the exponent of wmax, %d, differs from the table\'s %d' % (ew, acc.ew))
        if acc is None:
            acc = torch.zeros((K, nzones, bins + 2), dtype=torch.int64, device=self._dev())
        acc.ew, acc.range = ew, (lo, hi)
        if n:
            spec = self.ctx.zonal_hist_spec(self.np_dtype, n, K, nzones, _z.ZONE_U8 if zones.dtype == torch.uint8 else _z.ZONE_I32,
                                            kind, cols, first_pixel, pitch, wmax, ew, bins=bins, lo=lo, hi=hi, scale=scale)
            try:
                self.ctx.zonal_hist(spec, self.np_dtype, values.data_ptr(), zones.data_ptr(), wptr, None, acc.data_ptr(),
                                    where=_lib.DEVICE, stream=self._stream())
            except _lib.Mod16Error as e:
                raise _lib.overlap_as_value_error(e)
        return acc

    def zonal_selection(self, layers, nzones, q, bits=None):
        '''A ``ZonalSelection``: the radix selection of exact zonal quantiles for rasters that arrive
        in tiles or are dealt over devices. Every level sees every part once: ``.add`` each part,
        ``.merge`` the other devices' selections of the same level, ``.select()``; after ``levels``
        levels ``.result()`` gives the ``ZonalQuantiles``.'''
        return ZonalSelection(self, layers, nzones, q, bits)

    def zonal_quantiles(self, values, zones, nzones, q=(0.05, 0.5, 0.95), area=None, cols=None, first_pixel=0, wmax=None,
                        bits=None, slab_bytes=None):
        '''Exact weighted quantiles per zone and layer of a device-resident stack (the loop over the
        levels of a ``ZonalSelection``; the definition is ``mod16_amd.zonalq.quantiles``): the smallest
        value of the zone whose cumulative weight reaches ``q`` of the zone's total, an order statistic
        that does not depend on the order of the pixels. Layers are processed in groups so that the
        ``(K', Z, S, 2**bits)`` int64 table stays within ``slab_bytes`` (default 128 MiB; at least one
        layer). Every level reads the values once and nothing waits for the host between levels.
        Returns a ``mod16_amd.zonalq.ZonalQuantiles`` (downloads the results: waits).'''
        from . import zonal as _z, zonalq as _q
        K, n, pitch, kind, wptr, cols_, first_ = self._zonal_args(values, zones, area, cols, first_pixel)
        nzones = _z.check_nzones(nzones)
        qs = _q.check_q(q)
        bits = _q.DEFAULT_BITS if bits is None else _q.check_bits(bits)
        slab_bytes = (128 << 20) if slab_bytes is None else int(slab_bytes)
        if slab_bytes < 0:
            raise ValueError('slab_bytes must not be negative')
        wmax, _ = self._zonalq_wmax(values, area, cols_, first_, kind, wmax)
        group = max(1, min(K, slab_bytes // (nzones * len(qs) * (8 << bits))))
        out, weight, ew = [], [], 31
        for k0 in range(0, K, group):
            part = values[k0:k0 + group]
            sel = ZonalSelection(self, part.shape[0], nzones, qs, bits)
            while not sel.done:
                sel.add(part, zones, area=area, cols=cols, first_pixel=first_pixel, wmax=wmax)
                sel.select()
            res = sel.result()
            out.append(res.values)
            weight.append(res.weight)
            ew = res.ew
        return _q.ZonalQuantiles(np.concatenate(out), np.concatenate(weight), qs, ew)

    def ensemble(self, tables):
        '''The members of an ensemble forward run on this engine's device: ``tables`` is a (D, 13,
        11) array or a sequence of D ``restore_bplut`` dicts (``mod16_amd.calibration.ensemble_tables``
        draws them from a posterior). Returns an ``EnsembleRun``: ``.members``, ``.run(cls, drivers,
        out=None)`` -> five device tensors (mean and standard deviation over the members of the day
        and night totals, standard deviation of their sum), ``.close()``. The engine's own table
        plays no part; its ``math`` must be ``MATH_FAST`` or ``MATH_EXACT`` (``mod16_et_ensemble_*``).'''
        return EnsembleRun(self, tables)

    def run_pet(self, cls, drivers, out=None):
        '''ET and potential ET from one pass over device-resident drivers
        (``mod16_et_pet_*``, see ``mod16_amd.evapotranspiration_raster(...,
        pet=True)``). Returns ``(day, night, pet_day, pet_night)``; ``out`` may
        give the four output tensors.'''
        torch = _torch()
        n = cls.numel()
        cptr = self._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = self._marshal_drivers(drivers, n)
        out = tuple(out) if out is not None else tuple(self.empty(n, 4))
        optr = [self._check_tensor(t, self.dtype, n, 'out') for t in out]
        fn = _lib.typed(self.ctx.lib, 'mod16_et_pet', self.np_dtype)
        self.ctx.check(fn(
            self.ctx.handle, cptr, _lib.ptr_array(dptr), _lib.i64_array(dstride), None, None,
            n, optr[0], optr[1], optr[2], optr[3], int(self.math), _lib.DEVICE, self._stream()))
        return out

    def alloc_series(self, n, extra=0):
        '''Device buffers of ``run_series``: class raster, the two-slot driver
        ring and two output pairs (``extra``: see ``alloc_raster``).'''
        torch = _torch()
        a, b = self.alloc_raster(n, extra), self.alloc_raster(n, extra)
        return {'cls': a[0], 'ring': [a[1], b[1]], 'outs': [[a[2], a[3]], [b[2], b[3]]]}

    def run_series(self, n, steps, seed=16, pixel_offset=0, on_step=None, buffers=None):
        '''A time series streamed through HBM (BASELINE.json configs[3]): the
        drivers of step s + 1 are produced on a second HIP stream into the
        other half of a two-slot ring while the fused kernel works on step s.
        Here the producer is the on-device generator (``mod16_synth_*``), the
        stand-in for an ingest stage; the ring, the two streams and the event
        hand-off are what a real ingest would use. Returns ``(diag, day,
        night)``: the [steps, 8] diagnostics series and the outputs of the
        last step. ``on_step(s, day, night)`` is called (compute stream
        current) after step s has been enqueued, e.g. to accumulate; what it
        enqueues on the compute stream may read the outputs and the ring slot
        of step s (``buffers['ring'][s % 2]``), which is handed back to the
        ingest stream only behind it.'''
        torch = _torch()
        dev = self._dev()
        compute = torch.cuda.current_stream(self.device)
        ingest = torch.cuda.Stream(device=dev)
        buffers = buffers or self.alloc_series(n)
        cls, ring, outs = buffers['cls'], buffers['ring'], buffers['outs']
        diag = torch.zeros(steps, 8, dtype=torch.float64, device=dev)
        filled = [torch.cuda.Event() for _ in range(steps)]
        consumed = [torch.cuda.Event() for _ in range(steps)]
        ingest.wait_stream(compute)

        def produce(s):
            with torch.cuda.stream(ingest):
                if s >= 2:
                    ingest.wait_event(consumed[s - 2])      # slot is free again
                self.synth(n, seed=seed, step=s, pixel_offset=pixel_offset,
                           out=(cls, ring[s % 2]))
                filled[s].record(ingest)

        for s in range(min(2, steps)):
            produce(s)
        day = night = None
        for s in range(steps):
            compute.wait_event(filled[s])
            self._gate()
            day, night = outs[s % 2]
            self.run(cls, ring[s % 2], day, night, diag=diag[s])
            if on_step is not None:
                on_step(s, day, night)
            consumed[s].record(compute)     # behind on_step: it may still read the slot
            if s + 2 < steps:
                produce(s + 2)
        compute.wait_stream(ingest)
        return diag, day, night

    def run_raw(self, cls, raw, fpar_pct, lai_x10, day_hours=None, out_day=None,
                out_night=None, out_total8=None):
        '''Forward run on raw drivers held on the device (``mod16_et_raw_*``,
        see ``mod16_amd.evapotranspiration_raw``): ``raw`` = 14 tensors in
        ``mod16_raw_driver`` order, ``fpar_pct`` / ``lai_x10`` uint8 tensors.
        Returns ``(day, night)`` or, with ``day_hours``, ``(day, night,
        total8)``; outputs are allocated unless given.'''
        torch = _torch()
        n = cls.numel()
        keep, rptr, rstr = self._marshal_drivers(raw, n)
        hptr, hstr = None, 0
        if day_hours is not None:
            if isinstance(day_hours, torch.Tensor) and day_hours.numel() != 1:
                hptr, hstr = self._check_tensor(day_hours, self.dtype, n, 'day_hours'), 1
            else:
                hkeep = torch.as_tensor(day_hours, dtype=self.dtype).reshape(1).to(self._dev())
                keep.append(hkeep)
                hptr = hkeep.data_ptr()
        if out_day is None and out_night is None and out_total8 is None:
            out_day, out_night = self.empty(n, 2)
            if day_hours is not None:
                out_total8 = self.empty(n, 1)[0]
        ptr = lambda t, what: self._check_tensor(t, self.dtype, n, what) if t is not None else None
        fn = _lib.typed(self.ctx.lib, 'mod16_et_raw', self.np_dtype)
        self.ctx.check(fn(
            self.ctx.handle, self._check_tensor(cls, torch.uint8, n, 'cls'),
            _lib.ptr_array(rptr), _lib.i64_array(rstr),
            self._check_tensor(fpar_pct, torch.uint8, n, 'fpar_pct'),
            self._check_tensor(lai_x10, torch.uint8, n, 'lai_x10'), hptr, hstr, n,
            ptr(out_day, 'out_day'), ptr(out_night, 'out_night'), ptr(out_total8, 'out_total8'),
            int(self.math), _lib.DEVICE, self._stream()))
        if day_hours is not None:
            return out_day, out_night, out_total8
        return out_day, out_night

    def bind(self, cls, drivers, out_day, out_night, diag, graph=True):
        '''Pre-marshal one ``run(..., diag=diag)`` call and return a function
        that enqueues it on the then-current stream with a single library call
        (the per-step host cost of a time loop: no tensor checks, no ctypes
        array construction). With ``graph`` the launch sequence (counter
        reset, pipeline kernel, staged sum of the diagnostics) is captured
        into a HIP graph once (``mod16_graph_et_diag_*``) and a step is one
        ``hipGraphLaunch``. The tensors must stay alive and in place; their
        contents may change between steps.'''
        torch = _torch()
        n = cls.numel()
        cptr = self._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = self._marshal_drivers(drivers, n)
        args = (self.ctx.handle, cptr, _lib.ptr_array(dptr), _lib.i64_array(dstride), n,
                self._check_tensor(out_day, self.dtype, n, 'out_day'),
                self._check_tensor(out_night, self.dtype, n, 'out_night'), int(self.math),
                self._check_tensor(diag, torch.float64, 8, 'diag'))
        check, device, lib = self.ctx.check, self.device, self.ctx.lib
        keepalive = (keep, cls, out_day, out_night, diag)
        if graph:
            handle = C.c_void_p()
            make = _lib.typed(lib, 'mod16_graph_et_diag', self.np_dtype)
            rc = make(*args, C.byref(handle))
            if rc == _lib.OK:
                owner = _GraphHandle(lib, handle, self.ctx)

                def launch():
                    check(lib.mod16_graph_launch(owner.handle, torch.cuda.current_stream(device).cuda_stream))
                step = BoundStep(launch, (keepalive[2], keepalive[3]), owner, device)
                step._keep = keepalive
                return step
            if rc != _lib.ERR_HIP:      # argument errors are the caller's; a refused capture is not
                check(rc)
            import warnings
            warnings.warn('HIP graph capture failed (%s); the bound launch enqueues its kernels one by one'
                          % self.ctx.lib.mod16_last_error(self.ctx.handle).decode())
        fn = _lib.typed(lib, 'mod16_et_diag', self.np_dtype)

        def launch():
            check(fn(*args, torch.cuda.current_stream(device).cuda_stream))
        step = BoundStep(launch, (keepalive[2], keepalive[3]), None, device)
        step._keep = keepalive
        return step

    # ------------------------------------------------------ tiled rasters
    def alloc_tiled(self, n, tile=None, form=_lib.FORM_TOTALS):
        '''A ``TiledRaster`` for n pixels (``tile`` pixels per tile, default
        ``TILE_BYTES`` per field) of one form of the forward run.'''
        return TiledRaster(self, n, tile, form)

    def run_form_tiled(self, r, day_hours=None):
        '''The forward run of the raster's form over a tiled raster
        (``mod16_et_form_tiled_*``): what ``run_pet``, ``run(out_sep=...)`` and
        ``run_raw`` compute on plain arrays. ``day_hours``: the hours of daylight of
        ``FORM_RAW_TOTAL8`` (one value; ``FORM_RAW_TOTAL8_HOURS`` reads them per pixel
        from ``r.wide[14]``). Asynchronous on the current stream; returns ``r.outs``.'''
        if r.form == _lib.FORM_RAW_TOTAL8 and day_hours is None:
            raise ValueError('FORM_RAW_TOTAL8 needs day_hours')
        fn = _lib.typed(self.ctx.lib, 'mod16_et_form_tiled', self.np_dtype)
        self.ctx.check(fn(
            self.ctx.handle, C.byref(r.layout), r.form,
            _lib.ptr_array([b.data_ptr() for b in r.bytes]),
            _lib.ptr_array([w.data_ptr() for w in r.wide]),
            _lib.ptr_array([o.data_ptr() for o in r.outs]),
            float(day_hours) if day_hours is not None else 0.0, r.n, int(self.math),
            self._stream()))
        return r.outs

    def _tiled_args(self, r):
        return (C.byref(r.layout), r.cls.data_ptr(),
                _lib.ptr_array([d.data_ptr() for d in r.drivers]), r.n,
                r.day.data_ptr(), r.night.data_ptr(), int(self.math))

    def synth_tiled(self, r, seed=16, step=0, pixel_offset=0):
        '''The synthetic drivers of ``synth`` written straight into the tiled
        raster ``r`` (``mod16_synth_tiled_*``): same field, pixel for pixel.'''
        fn = _lib.typed(self.ctx.lib, 'mod16_synth_tiled', self.np_dtype)
        self.ctx.check(fn(
            self.ctx.handle, C.byref(r.layout), int(seed), int(step), int(pixel_offset), r.n,
            r.cls.data_ptr(), _lib.ptr_array([d.data_ptr() for d in r.drivers]), self._stream()))
        return r

    def to_tiled(self, cls, drivers, r=None):
        '''Copy plain device arrays (class raster + 14 drivers, 1-D tensors)
        into a tiled raster (one strided copy per array).'''
        n = cls.numel()
        r = r or self.alloc_tiled(n)
        r.put(r.cls, cls)
        for k in range(14):
            r.put(r.drivers[k], drivers[k])
        return r

    def run_tiled(self, r, diag=None):
        '''The fused ET kernel over a tiled raster (``mod16_et_tiled_*``),
        asynchronous on the current stream; outputs in ``r.day`` / ``r.night``,
        with ``diag`` (float64 tensor of 8 on the device) the diagnostics too.'''
        torch = _torch()
        fn = _lib.typed(self.ctx.lib, 'mod16_et_tiled', self.np_dtype)
        dptr = self._check_tensor(diag, torch.float64, 8, 'diag') if diag is not None else None
        self.ctx.check(fn(self.ctx.handle, *self._tiled_args(r), dptr, self._stream()))
        return r.day, r.night

    def time_tiled(self, r, launches=10, diag=None):
        '''Mean milliseconds per direct launch of ``run_tiled`` (HIP events on the
        current stream, ``mod16_time_et_tiled``).'''
        torch = _torch()
        ms = C.c_float(0)
        lay, cls, drv, n, day, night, math = self._tiled_args(r)
        self.ctx.check(self.ctx.lib.mod16_time_et_tiled(
            self.ctx.handle, int(self.np_dtype == np.float32), lay, cls, drv, n, day, night, math,
            self._check_tensor(diag, torch.float64, 8, 'diag') if diag is not None else None,
            int(launches), self._stream(), C.byref(ms)))
        return ms.value

    def bind_tiled(self, r, diag):
        '''``run_tiled(r, diag)`` captured once into a HIP graph
        (``mod16_graph_et_tiled_*``); the returned ``BoundStep`` replays it with
        one library call and can time itself.'''
        torch = _torch()
        handle = C.c_void_p()
        lib, check, device = self.ctx.lib, self.ctx.check, self.device
        make = _lib.typed(lib, 'mod16_graph_et_tiled', self.np_dtype)
        check(make(self.ctx.handle, *self._tiled_args(r),
                   self._check_tensor(diag, torch.float64, 8, 'diag'), C.byref(handle)))
        owner = _GraphHandle(lib, handle, self.ctx)
        keep = (r, diag)

        def launch():
            check(lib.mod16_graph_launch(owner.handle, torch.cuda.current_stream(device).cuda_stream))
        step = BoundStep(launch, (r.day, r.night), owner, device)
        step._keep = keep
        return step

    def run_series_tiled(self, n, steps, seed=16, pixel_offset=0, on_step=None, ring=None):
        '''``run_series`` on tiled rasters: a ring of two ``TiledRaster`` slots,
        the drivers of step s + 1 produced on a second stream while the kernel
        works on step s. Returns ``(diag, raster of the last step)``.'''
        torch = _torch()
        dev = self._dev()
        compute = torch.cuda.current_stream(self.device)
        ingest = torch.cuda.Stream(device=dev)
        ring = ring or [self.alloc_tiled(n), self.alloc_tiled(n)]
        diag = torch.zeros(steps, 8, dtype=torch.float64, device=dev)
        filled = [torch.cuda.Event() for _ in range(steps)]
        consumed = [torch.cuda.Event() for _ in range(steps)]
        ingest.wait_stream(compute)

        def produce(s):
            with torch.cuda.stream(ingest):
                if s >= 2:
                    ingest.wait_event(consumed[s - 2])
                self.synth_tiled(ring[s % 2], seed=seed, step=s, pixel_offset=pixel_offset)
                filled[s].record(ingest)

        for s in range(min(2, steps)):
            produce(s)
        last = None
        for s in range(steps):
            compute.wait_event(filled[s])
            self._gate()
            last = ring[s % 2]
            self.run_tiled(last, diag=diag[s])
            if on_step is not None:
                on_step(s, last)
            consumed[s].record(compute)
            if s + 2 < steps:
                produce(s + 2)
        compute.wait_stream(ingest)
        return diag, last

    def run_series_host(self, ring, host_steps, steps, day_hours=None, on_step=None):
        '''A time series whose drivers arrive from HOST memory (a real ingest: SURVEY.md 8f
        N1 / N4, reference calibration.py:380-423): ``ring`` is two ``TiledRaster`` slots of one
        form -- typically ``FORM_RAW`` on a float32 engine, the light input form: 14 float32 raw
        fields + uint8 fPAR / LAI = 58 bytes per pixel and step over PCIe instead of the 113 of
        float64 plain drivers. ``host_steps`` is a list of K step records ``{'wide': [...],
        'bytes': [...]}`` of page-locked CPU tensors with ``ntiles * tile`` elements each (``None``
        = the field stays as it is in the slots: the class raster, static fields); step ``s``
        takes record ``s % K``. The copies of step s + 1 run on a second stream -- tile-wide rows
        straight into the slot's pitch, no repacking pass -- under the kernel of step s; the
        kernel is ``run_form_tiled`` (the reference's pre-processing is inside it).
        ``on_step(s, slot)`` is called with the compute stream current behind step s's kernel.
        Returns the slot of the last step.'''
        torch = _torch()
        compute = torch.cuda.current_stream(self.device)
        ingest = torch.cuda.Stream(device=self._dev())
        filled = [torch.cuda.Event() for _ in range(steps)]
        consumed = [torch.cuda.Event() for _ in range(steps)]
        ingest.wait_stream(compute)

        def produce(s):
            rec, slot = host_steps[s % len(host_steps)], ring[s % 2]
            with torch.cuda.stream(ingest):
                if s >= 2:
                    ingest.wait_event(consumed[s - 2])      # the slot is free again
                for dst, src in list(zip(slot.wide, rec.get('wide', []))) + list(zip(slot.bytes, rec.get('bytes', []))):
                    if src is not None:
                        dst.copy_(src.view(slot.ntiles, slot.tile), non_blocking=True)
                filled[s].record(ingest)

        for s in range(min(2, steps)):
            produce(s)
        last = None
        for s in range(steps):
            compute.wait_event(filled[s])
            self._gate()
            last = ring[s % 2]
            self.run_form_tiled(last, day_hours)
            if on_step is not None:
                on_step(s, last)
            consumed[s].record(compute)
            if s + 2 < steps:
                produce(s + 2)
        compute.wait_stream(ingest)
        return last

    def measure_copy(self, nbytes=4 << 30, reps=3):
        '''GB/s of a plain device-to-device copy kernel on this GPU
        (``mod16_measure_copy``): the measured reference point next to the
        nominal HBM peak.'''
        gbps = C.c_float(0)
        self.ctx.check(self.ctx.lib.mod16_measure_copy(self.ctx.handle, int(nbytes), int(reps),
                                                       C.byref(gbps)))
        return gbps.value

    def fold_ranks(self, gathered, world, diag):
        '''The rank-order fold behind the all-gather of the diagnostics vectors
        (``mod16_fold_diag``; ``mod16_amd.dist.allreduce_diag`` calls it): ``gathered`` is the
        ``(world, 8)`` float64 block, ``diag`` (8) receives sums in rank order and maxima. One
        kernel on the current stream.'''
        torch = _torch()
        self.ctx.check(self.ctx.lib.mod16_fold_diag(
            self.ctx.handle, self._check_tensor(gathered, torch.float64, world * 8, 'gathered'),
            int(world), self._check_tensor(diag, torch.float64, 8, 'diag'), self._stream()))
        return diag

    def check(self):
        '''Synchronise and raise deferred errors (IndexError for a class code
        >= 13, as the reference's numpy gather would).'''
        self.ctx.check_status(self._stream())

    def diagnostics(self, day, night, out=None):
        '''Deterministic reduction of a (day, night) pair on the device ->
        float64 tensor of 8 (``DIAG_FIELDS``), asynchronous.'''
        torch = _torch()
        n = day.numel()
        if out is None:
            out = torch.empty(8, dtype=torch.float64, device=self._dev())
        fn = _lib.typed(self.ctx.lib, 'mod16_reduce_diag', self.np_dtype)
        self.ctx.check(fn(
            self.ctx.handle, self._check_tensor(day, self.dtype, n, 'day'),
            self._check_tensor(night, self.dtype, n, 'night'), n, None,
            self._check_tensor(out, torch.float64, 8, 'out'), self._stream()))
        return out

    def time_kernel(self, cls, drivers, out_day, out_night, launches=10, diag=None):
        '''Mean milliseconds per launch of the fused kernel (with ``diag``: of
        the kernel that also reduces the diagnostics), measured with HIP
        events on the stream the kernel runs on (``mod16_time_et``).'''
        torch = _torch()
        n = cls.numel()
        cptr = self._check_tensor(cls, torch.uint8, n, 'cls')
        keep, dptr, dstride = self._marshal_drivers(drivers, n)
        ms = C.c_float(0)
        self.ctx.check(self.ctx.lib.mod16_time_et(
            self.ctx.handle, int(self.np_dtype == np.float32), cptr,
            _lib.ptr_array(dptr), _lib.i64_array(dstride), None, None, n,
            self._check_tensor(out_day, self.dtype, n, 'out_day'),
            self._check_tensor(out_night, self.dtype, n, 'out_night'), None,
            int(self.math),
            self._check_tensor(diag, torch.float64, 8, 'diag') if diag is not None else None,
            int(launches), self._stream(), C.byref(ms)))
        return ms.value


class ShardedSeries(object):
    '''
    ``RasterEngine.run_series_host`` over several GPUs of one node, in one process
    (``mod16_amd.multi``; SURVEY.md 8e for the PCIe-bound ingest: N links instead of one,
    no collective). The tiles of the raster are dealt over ``devices`` in order --
    device ``i`` holds tiles ``[t0_i, t1_i)`` in a two-slot ring of ``TiledRaster`` of
    its own, fed by its own host thread, ingest stream and engine -- and every step's
    kernel runs on each device over its tiles only. A pixel's result does not depend on
    the device list (``devices=[0]`` and ``[0, 0]`` give the same bits).

    Parameters
    ----------
    table : numpy.ndarray
        (13, 11) BPLUT table
    n : int
        Pixels of the raster (a multiple of the 16-byte vector width)
    devices : sequence of int
        GPU indices; one may be listed more than once
    form, dtype, math, trusted, tile
        As for ``RasterEngine`` / ``RasterEngine.alloc_tiled``; the defaults are the light
        input form (``FORM_RAW`` on float32: 58 bytes per pixel and step over PCIe)
    '''

    def __init__(self, table, n, devices, form=_lib.FORM_RAW, dtype='float32',
                 math=_lib.MATH_FAST, trusted=False, tile=None):
        from . import multi
        torch = _torch()
        devs = multi.device_list(devices)
        if devs is None:
            raise ValueError('devices is required')
        self.n, self.form = int(n), int(form)
        self.parts = []             # per device that holds tiles: dict(device, engine, ring, t0, t1, offset, n)
        probe = RasterEngine(table, device=devs[0], dtype=dtype, math=math, trusted=trusted)
        self.tile = int(tile) if tile else probe.TILE_BYTES // probe.np_dtype.itemsize
        self.ntiles = max(1, -(-self.n // self.tile))
        for i, (t0, count) in enumerate(multi.shards(self.ntiles, len(devs), 1)):
            if not count:
                continue
            lo, hi = t0 * self.tile, min(self.n, (t0 + count) * self.tile)
            with torch.cuda.device(devs[i]):
                eng = probe if (i == 0) else RasterEngine(table, device=devs[i], dtype=dtype, math=math,
                                                           trusted=trusted)
                ring = [eng.alloc_tiled(hi - lo, self.tile, self.form) for _ in range(2)]
                stream = torch.cuda.Stream(device=eng._dev())
            self.parts.append(dict(device=devs[i], engine=eng, ring=ring, stream=stream,
                                   t0=t0, t1=t0 + count, offset=lo, n=hi - lo))

    def run_host(self, host_steps, steps, day_hours=None, on_step=None):
        '''``run_series_host`` on every device at once. ``host_steps``: as there, records of
        page-locked CPU tensors covering the WHOLE raster (``ntiles * tile`` elements; ``None`` = the
        field stays as it is); each device copies its tiles' part. ``on_step(part, s, slot)``
        is called on the device's own host thread (compute stream current) behind step ``s``'s
        kernel, ``part`` being the entry of ``self.parts`` (``part['offset']`` = first pixel of
        the slot in the raster). Returns the slots of the last step, one per part. Errors of any
        device are raised here (first in device order) after all of them have finished.'''
        import threading
        torch = _torch()
        P = self.tile
        results, errors = [None] * len(self.parts), [None] * len(self.parts)

        def cut(rec, part):
            a, b = part['t0'] * P, part['t1'] * P
            return {key: [None if t is None else t[a:b] for t in rec.get(key, [])] for key in ('wide', 'bytes')}

        def work(k, part):
            try:
                torch.cuda.set_device(part['device'])
                mine = [cut(rec, part) for rec in host_steps]
                with torch.cuda.stream(part['stream']):
                    hook = (lambda s, slot: on_step(part, s, slot)) if on_step is not None else None
                    results[k] = part['engine'].run_series_host(part['ring'], mine, steps, day_hours, hook)
                    part['engine'].check()
            except BaseException as exc:
                errors[k] = exc

        threads = [threading.Thread(target=work, args=(k, p)) for k, p in enumerate(self.parts)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for e in errors:
            if e is not None:
                raise e
        return results

    def read(self, slots, out_index, into):
        '''Copies output ``out_index`` of the per-device ``slots`` (what ``run_host`` returned)
        into the 1-D CPU tensor ``into`` (n elements, ideally page-locked), every part at its
        pixel offset; synchronous.'''
        torch = _torch()
        for part, slot in zip(self.parts, slots):
            with torch.cuda.device(part['device']):
                flat = slot.flat(slot.outs[out_index], 0, part['n'])
                into[part['offset']:part['offset'] + part['n']].copy_(flat)
        return into
