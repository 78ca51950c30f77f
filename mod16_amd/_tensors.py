'''
Argument handling shared by the device-tensor entry points (``mod16_amd.raster``), the counterpart
of ``_args.py``: is this a tensor on the engine's device, and what strided layout does it have in
the terms of the C ABI (a row pitch, a plane stride, a stride in time, all in elements), and the
``out=`` protocol over a family's table of results (``named_outputs``). The layout rules look at
``shape`` and ``stride()`` only, so they hold for CPU tensors as well (tests/
test_tensor_args_host.py). Nothing here loads the library, or ``torch`` before a call needs it.
'''
import numpy as np


_Tensor = None       # torch.Tensor, once a check has needed it (this sits on every enqueue path)


def check_device(t, what, device, *dtypes):
    '''TypeError unless ``t`` is a tensor on ``cuda:<device>`` with one of ``dtypes`` (none given: any).'''
    global _Tensor
    if _Tensor is None:
        import torch
        _Tensor = torch.Tensor
    if not isinstance(t, _Tensor) or t.get_device() != device or not t.is_cuda or \
            (dtypes and t.dtype not in dtypes):
        kinds = ' or '.join(str(d).replace('torch.', '') for d in dtypes)
        raise TypeError('%s must be a %stensor on cuda:%d' % (what, kinds + ' ' if kinds else '', device))


def row_pitch(t, what, between='distance between rows'):
    '''The distance between the rows of a ``(..., rows, n)`` or ``(n,)`` tensor in elements: unit
    stride in the last dimension (not looked at with at most one element), rows at least ``n``
    apart; one row: ``n`` (at least 1) whatever its stride says. ``between``: what the rows' distance
    is called where they are time slabs.'''
    shape, stride = t.shape, t.stride()       # (both whole: one call each)
    n = shape[-1]
    if n > 1 and stride[-1] != 1:
        raise ValueError('%s must have unit stride in pixels' % what)
    pitch = stride[-2] if len(shape) > 1 and shape[-2] > 1 else max(n, 1)
    if pitch < n:
        raise ValueError('%s: the %s must be at least %d' % (what, between, n))
    return pitch


def plane_layout(t, what):
    '''-> (row pitch, plane stride) in elements of a ``(planes, R, W)`` or ``(R, W)`` tensor: unit
    stride in columns (not looked at with at most one), rows at least ``W`` apart (one row: ``W``),
    planes at least a plane -- ``(R - 1) * pitch + W`` elements -- apart (one plane: exactly that).'''
    shape, stride = t.shape, t.stride()
    R, W = shape[-2:]
    if W > 1 and stride[-1] != 1:
        raise ValueError('%s must have unit stride in columns' % what)
    pitch = stride[-2] if R > 1 else W
    if pitch < W:
        raise ValueError('%s: the distance between rows must be at least %d' % (what, W))
    least = (R - 1) * pitch + W
    plane = stride[0] if len(shape) == 3 and shape[0] > 1 else least
    if plane < least:
        raise ValueError('%s: the stride in time must be at least a plane (%d elements)' % (what, least))
    return pitch, plane


def torch_dtype(dtype):
    '''The torch dtype of a numpy dtype (or its name); ``numpy_dtype`` is the way back. The two
    libraries share the names, which is the whole table.'''
    import torch
    return getattr(torch, np.dtype(dtype).name)


def numpy_dtype(dtype):
    return np.dtype(str(dtype).replace('torch.', ''))


def named_outputs(out, table, device, between=None, called='fields produced'):
    '''The ``out=`` protocol of the tensor entry points -> ``(tensors by key, layouts by key)`` in the
    order of ``table``, which states the results as key -> ``(shape, numpy dtype)`` (a definition
    module's ``output_table``; keys ``0, 1, ...``: positional results). ``out``: None (new tensors), or
    the caller's dict (sequence, for positional results). ``between``: None for ``(planes, R, W)`` /
    ``(R, W)`` results (``plane_layout``), else they are rows (``row_pitch``) that far apart.

    First the key set or the count; then per result, in the table's order, ``check_device``, the shape,
    the layout rule, under the label ``out[<key>]``: of two offences in different results the earlier
    result's is reported, whatever its kind. What results must share is the caller's (``share_one``).'''
    if out is None:
        import torch
        where = torch.device('cuda', device)
        outs = {k: torch.empty(shape, dtype=torch_dtype(dt), device=where) for k, (shape, dt) in table.items()}
    elif 0 in table:
        outs = dict(enumerate(out))
        if len(outs) != len(table):
            raise ValueError('out must hold %d tensors' % len(table))
    else:
        outs = dict(out)
        if sorted(outs) != sorted(table):
            raise ValueError('out must hold exactly the %s: %s' % (called, ', '.join(table)))
    layouts = {}
    for k, (shape, dt) in table.items():
        t, what = outs[k], 'out[%r]' % (k,)
        check_device(t, what, device, torch_dtype(dt))
        if tuple(t.shape) != tuple(shape):
            raise ValueError('%s must have shape %r, got %r' % (what, tuple(shape), tuple(t.shape)))
        layouts[k] = plane_layout(t, what) if between is None else row_pitch(t, what, between)
    return {k: outs[k] for k in table}, layouts


def share_one(values, who, what):
    '''The one value in ``values`` (None: there is none); ValueError ``<who> must share one <what>``
    where they differ.'''
    seen = set(values)
    if len(seen) > 1:
        raise ValueError('%s must share one %s' % (who, what))
    return seen.pop() if seen else None


def series(t, what, n, device, dtype):
    '''-> (address, stride in time) of an ``(n,)`` or ``(S, n)`` tensor of a composite call: the
    pixels of one array, constant in time or slab by slab; the stride is 0 with one slab.'''
    check_device(t, what, device, dtype)
    if t.dim() > 2 or t.shape[-1] != n:
        raise ValueError('%s must be a scalar, an (n,) or an (S, n) tensor with n = %d, got %r'
                         % (what, n, tuple(t.shape)))
    pitch = row_pitch(t, what, 'stride in time')
    return t.data_ptr(), pitch if t.dim() == 2 and t.shape[0] > 1 else 0
