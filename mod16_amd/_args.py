'''
Argument handling shared by the numpy entry points (``mod16_amd`` and ``mod16_amd.extensions``):
the dtype rule, broadcasting, marshalling of inputs into addresses and strides for the C ABI, and
the rules every entry point applies to its class raster, its ``out=`` arrays and ``stage_bytes``.
Nothing here loads the library.
'''
import ctypes as _ctypes

import numpy as np

from . import _lib


def _result_dtype(values):
    '''float32 only if every array-like input is float32 (numpy's own rule
    for the reference code); Python scalars are weak.'''
    seen32, others = False, None
    for v in values:
        t = type(v)
        if t is float or t is int:
            continue
        if isinstance(v, (np.ndarray, np.generic)):
            if v.dtype == _F32:
                seen32 = True
            elif others is None:
                others = [v.dtype]
            else:
                others.append(v.dtype)
    if others is None:
        return _F32 if seen32 else _F64
    if seen32:
        others.append(_F32)
    return _F32 if np.result_type(*others) == _F32 else _F64


_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_U16 = np.dtype(np.uint16)


def _address(a):
    '''Address of a C-contiguous array's first element (the buffer protocol is a third of
    the cost of ``a.ctypes.data``, but wants a writeable, non-empty array).'''
    if a.flags.writeable and a.size:
        return _ctypes.addressof(_ctypes.c_char.from_buffer(a))
    return a.__array_interface__['data'][0]


def _broadcast(shapes):
    '''-> (broadcast shape, number of elements); equal shapes -- the usual call -- without numpy.'''
    shape = shapes[0]
    for sh in shapes:
        if sh != shape:
            shape = np.broadcast_shapes(*shapes)
            break
    n = 1
    for extent in shape:
        n *= int(extent)
    return shape, n


def _shape(v):
    '''``np.shape`` without its detour through ``asarray`` for the two common cases.'''
    t = type(v)
    if t is float or t is int:
        return ()
    if t is np.ndarray:
        return v.shape
    return np.shape(v)


def _broadcast_kind(a_shape, size, shape):
    '''How an input of shape ``a_shape`` broadcasts against the full ``shape``,
    as one of the kinds the C ABI takes without making it dense (``mod16_et2_*``):
    scalar, dense, an (N,) row against (..., N), or a (..., 1) column. ``None``:
    another pattern (made dense by the caller).'''
    if size == 1:
        return _lib.BC_SCALAR
    padded = (1,) * (len(shape) - len(a_shape)) + tuple(a_shape)
    if padded == tuple(shape):
        return _lib.BC_DENSE
    if len(shape) >= 2:
        if padded[-1] == shape[-1] and all(x == 1 for x in padded[:-1]):
            return _lib.BC_ROW
        if padded[-1] == 1 and padded[:-1] == tuple(shape[:-1]):
            return _lib.BC_COL
    return None


def _marshal(values, shape, dtype, kinds=False):
    '''-> (keepalive arrays, addresses, element strides) for the C ABI: a
    size-1 input is passed as a broadcast scalar (stride 0), anything else is
    made dense over ``shape`` (stride 1). With ``kinds`` the third list holds
    broadcast kinds (``_lib.BC_*``) and (N,) rows / (..., 1) columns stay as
    small as they are. (The size-1 inputs share ONE small array: a call on the
    scalars of a flux-tower site costs a handful of numpy operations, not 25
    times three.)'''
    keep, ptrs, strides = [], [], []
    scal = base = None
    dtype = np.dtype(dtype)
    esz = dtype.itemsize
    for i, v in enumerate(values):
        t = type(v)
        if t is float or t is int:
            a = None
        else:
            a = v if (t is np.ndarray and v.dtype == dtype) else np.asarray(v, dtype=dtype)
            if a.size == 1:
                v = a.reshape(-1)[0]
                a = None
        if a is None:
            if scal is None:
                scal = np.empty(len(values), dtype)
                base = _address(scal)
                keep.append(scal)
            scal[i] = v
            ptrs.append(base + i * esz)
            strides.append(0)
            continue
        kind = _broadcast_kind(a.shape, a.size, shape) if kinds else None
        if kind in (_lib.BC_ROW, _lib.BC_COL):
            a = np.ascontiguousarray(a.reshape(-1))
            strides.append(kind)
        else:
            if a.shape != shape:
                a = np.broadcast_to(a, shape)
            if not a.flags.c_contiguous:
                a = np.ascontiguousarray(a)
            strides.append(1)
        keep.append(a)
        ptrs.append(_address(a))
    return keep, ptrs, strides


def _shift(ptrs, kinds, off, inner, itemsize):
    '''The addresses of pixel ``off`` onwards: dense arrays move by ``off``
    elements, (T, 1) columns by ``off // inner`` (``off`` is then a multiple of
    ``inner``), scalars and (N,) rows stay.'''
    if ptrs is None or off == 0:
        return ptrs
    step = {_lib.BC_SCALAR: 0, _lib.BC_DENSE: off, _lib.BC_ROW: 0, _lib.BC_COL: off // max(inner, 1)}
    return [p + step[k] * itemsize if p is not None else None for p, k in zip(ptrs, kinds)]


def _as_uint8(raster, message='class code outside [0, 255]'):
    '''A class raster (or another byte raster) as a uint8 array: other integer types are
    range-checked first, IndexError(``message``) as the numpy gather would raise. Broadcasting it
    and making it contiguous is the caller's.'''
    a = np.asarray(raster)
    if a.dtype != np.uint8:
        if a.size and (a.min() < 0 or a.max() > 255):
            raise IndexError(message)
        a = a.astype(np.uint8)
    return a


def _outputs(out, shape, dtypes, pinned=True, indexed=False):
    '''The result arrays of an entry point, one per entry of ``dtypes`` (numpy dtype objects), each
    of ``shape``: new ones -- from the page-locked pool (``_lib.pinned``) or, ``pinned=False``, plain
    ``np.empty`` -- or the caller's ``out`` arrays after a check: their count, then that every one
    is a writeable C-contiguous ndarray of that shape and dtype. ``indexed``: the refusal names the
    array (``out[k] must be ...``) instead of speaking of all of them.'''
    if out is None:
        empty = _lib.pinned.empty if pinned else np.empty
        return [empty(shape, dt) for dt in dtypes]
    outs = list(out)
    if len(outs) != len(dtypes):
        raise ValueError('out must hold %d arrays' % len(dtypes))
    for k, (o, dt) in enumerate(zip(outs, dtypes)):
        if not (isinstance(o, np.ndarray) and o.shape == shape and o.dtype == dt
                and o.flags.c_contiguous and o.flags.writeable):
            if indexed:
                raise ValueError('out[%d] must be a writeable C-contiguous %s array of shape %s' % (k, dt, shape))
            raise ValueError('out arrays must be writeable C-contiguous %s arrays of shape %s' % (dt, shape))
    return outs


def _named_outputs(out, table):
    '''The result arrays of an entry point whose results go by name, ``table`` stating them as name ->
    ``(shape, numpy dtype)`` (the ``output_table`` of a definition module): new ones from ``np.empty``,
    or the caller's ``out`` dict after a check -- exactly the table's names, then in its order that
    every one is a writeable C-contiguous ndarray of that shape and dtype. The counterpart of
    ``_tensors.named_outputs``.'''
    if out is None:
        return {k: np.empty(shape, dt) for k, (shape, dt) in table.items()}
    outs = dict(out)
    if sorted(outs) != sorted(table):
        raise ValueError('out must hold exactly the requested outputs: %s' % ', '.join(table))
    for k, (shape, dt) in table.items():
        o = outs[k]
        if not (isinstance(o, np.ndarray) and o.shape == shape and o.dtype == dt
                and o.flags.c_contiguous and o.flags.writeable):
            raise ValueError("out['%s'] must be a writeable C-contiguous %s array of shape %s" % (k, dt, shape))
    return outs


def _check_stage_bytes(stage_bytes):
    if stage_bytes is not None and int(stage_bytes) < 0:
        raise ValueError('stage_bytes must not be negative')


def _zonal_inputs(values, zones, nzones, area):
    '''What the zonal entry points (``zonal_statistics``, ``zonal_histogram``, ``zonal_quantiles``) make of
    their arrays: -> ``(values (K, n), zones (n,), nzones, layered, weight kind, cols, weights or None)``.
    ``values``: float32 or float64 of the zones' shape or ``(K,) +`` that shape; ``zones``: integers
    (uint8, uint16 and int32 as they are, others range-checked and cast to int32); ``nzones`` None:
    ``zones.max() + 1``; ``area``: None, a scalar (one "row" that holds every pixel), ``(R,)`` float64 for a
    2-D raster of R rows, or an array of the zones' shape taken in the values' dtype.'''
    from . import zonal as _z
    values, zones = np.asarray(values), np.asarray(zones)
    if values.dtype not in (np.float32, np.float64):
        raise ValueError('values must be float32 or float64, got %s' % values.dtype)
    if zones.dtype.kind not in 'iu':
        raise ValueError('zones must be integers, got %s' % zones.dtype)
    shape = zones.shape
    if values.shape == shape:
        layered, K = False, 1
    elif values.ndim == zones.ndim + 1 and values.shape[1:] == shape:
        layered, K = True, values.shape[0]
    else:
        raise ValueError('values must have the shape of zones %r or (K,) + that shape, got %r' % (shape, values.shape))
    n = int(np.prod(shape, dtype=np.int64))
    if n > _z.MAX_PIXELS:
        raise ValueError('a call takes at most 2**30 pixels (accumulate parts with acc=), got %d' % n)
    if not 1 <= K <= _z.MAX_LAYERS:
        raise ValueError('between 1 and %d layers, got %d' % (_z.MAX_LAYERS, K))
    if nzones is None:
        nzones = max(int(zones.max()) + 1, 1) if n else 1
    nzones = _z.check_nzones(nzones)
    if zones.dtype.name not in _z.ZONE_TYPES:
        if n and (int(zones.min()) < -2 ** 31 or int(zones.max()) >= 2 ** 31):
            raise ValueError('zone ids must fit an int32')
        zones = zones.astype(np.int32)
    zones = np.ascontiguousarray(zones).reshape(n)
    values = np.ascontiguousarray(values).reshape(K, n)
    kind, cols, weights = _lib.ZONAL_WEIGHT_NONE, 1, None
    if area is not None:
        area = np.asarray(area)
        if area.dtype.kind not in 'fiu':
            raise ValueError('area must be numeric, got %s' % area.dtype)
        if area.ndim == 0:               # one weight for every pixel: one "row" that holds them all
            kind, cols, weights = _lib.ZONAL_WEIGHT_ROW, max(n, 1), np.array([area], np.float64)
        elif len(shape) == 2 and area.shape == (shape[0],):
            kind, cols, weights = _lib.ZONAL_WEIGHT_ROW, max(shape[1], 1), np.ascontiguousarray(area, np.float64)
        elif area.shape == shape:
            kind, weights = _lib.ZONAL_WEIGHT_PIXEL, np.ascontiguousarray(area, values.dtype).reshape(n)
        else:
            raise ValueError('area must be a scalar, (rows,) for a 2-D raster or of the shape of zones %r, got %r'
                             % (shape, area.shape))
    return values, zones, nzones, layered, kind, cols, weights
