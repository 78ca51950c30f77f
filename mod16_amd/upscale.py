'''
Upscaling: area-weighted means of the valid fine pixels of every cell of a coarse grid, and the
dominant class of a class raster per cell -- the numpy statement of what ``mod16_upscale_f32`` /
``mod16_upscale_f64`` / ``mod16_upscale_classes`` compute (``RasterEngine.upscale_grid``,
``mod16_amd.upscale_fields``, ``mod16_amd.upscale_classes``), and the argument checks of those calls.
Host only: nothing here touches the library or a device; the kernels (``csrc/mod16_upscale.hpp``)
follow ``aggregate`` and ``majority`` step for step and give their bits.

Geometry. A fine ``R x C`` raster lies over an ``H x W`` coarse grid; ``row_pos[R]`` and ``col_pos[C]``
are the positions of the fine rows and columns in units of coarse cells, cell centres at the integers
(``mod16_amd.downscale.positions``), as a ``DownscaleGrid`` takes them. A pixel belongs to the cell its
centre lies in (``cell_table``: inside the grid the cell ``'nearest'`` interpolation picks); a pixel
outside the grid belongs to none. The fine indices of a cell form one run of consecutive indices on
either axis (``cell_runs``), so a cell's pixels are a rectangle of the raster: all geometry is host work
and the device sees four int32 tables, ``(row_first, row_count)`` and ``(col_first, col_count)``.

``aggregate``, per layer ``k`` and cell ``(i, j)``, in float64 (float32 values are widened first:
exact), every operation rounded on its own:

- ``num = den = tot = +0.0``, ``cnt = 0``; for the cell's rows in run order ``r = row_first[i] + 0, 1,
  ...``: ``s = +0.0``, ``m = 0``; for the cell's columns in run order (cyclic with ``wrap``): ``x =
  values[k, r, col]``, and where ``x`` is not NaN ``s = s + x``, ``m += 1`` (infinities take part as the
  arithmetic has them); then ``num = num + area[r] * s``, ``den = den + area[r] * float(m)``, ``tot =
  tot + area[r] * float(col_count[j])``, ``cnt += m``;
- ``fraction = den / tot``, 0.0 for a cell without pixels; ``mean = num / den`` where ``cnt >= 1`` and
  ``den >= min_fraction * tot`` (one rounded multiplication, then the comparison), else NaN; ``count =
  cnt``.

``majority``: per cell the pixels of every valid class code are counted; the winner is the code with
the highest count, the LOWEST code on a tie (the site-level ancestor, ``Counter.most_common``, takes the
first met, which depends on the traversal order); 255 where no pixel is valid; ``share =
float32(float64(winner's count) / float64(pixels of the cell))``, 0 for an empty or all-invalid cell.

Row-affine columns (a sinusoidal tile; ``col_affine = (col_origin[R], col_scale[R])`` as
``mod16_amd.downscale`` has them). The column position of pixel ``(r, c)`` is ``col_origin[r] +
col_scale[r] * c`` and its coarse column ``cell_table`` of that position, so the column run of a cell
differs from fine row to fine row: ``cell_table_rows`` and ``cell_runs_rows`` state the geometry as ``(R,
C)`` and ``(R, W)`` tables -- the tests' oracle; the device never sees them, it finds the runs from the
two float64 of a row -- and ``aggregate_rows`` / ``majority_rows`` are ``aggregate`` / ``majority`` with
the column run of cell ``j`` taken per fine row (``tot = tot + area[r] * float64(count[r, j])``; the
pixels of a cell are ``sum_r count[r, j]``). ``col_range = (col_first[R], col_count[R])`` names the
columns of every fine row that can belong to a cell (the on-globe pixels of an edge tile:
``downscale.sinusoidal_columns``); the others belong to none and are not read. The pixels of one cell
in one fine row must be ONE run of consecutive columns, never cyclic in ``c``; ``check_rows`` accepts a
row without ``wrap``, or with ``n = col_count[r] <= 1``, or where ``abs(col_scale[r]) * float64(n - 1)
<= float64(W - 2)``, which is sufficient for that: a row that spans the whole periodic axis (a mosaic
row of 36 tiles) is refused -- upscale per tile or per half and ``merge``.

``sums_rows`` / ``aggregate_rows(..., sums=True)`` stop before the divisions: ``UpscaledSums(num, den,
tot, count)`` (float64 whatever the input type, int32), what a tile contributes to cells it covers
only in part; ``merge`` adds the parts of several tiles IN THE GIVEN ORDER and divides once.
'''
import collections

import numpy as np

from . import downscale as _d

MAX_LAYERS = 65535
MAX_CODES = 32                                     # class codes a ``valid`` set may name: [0, 32)
NO_CLASS = 255
OUTPUT_NAMES = ('mean', 'fraction', 'count')
CLASS_OUTPUT_NAMES = ('cls', 'share')
Upscaled = collections.namedtuple('Upscaled', OUTPUT_NAMES)
UpscaledClasses = collections.namedtuple('UpscaledClasses', CLASS_OUTPUT_NAMES)
Runs = collections.namedtuple('Runs', ('first', 'count'))
SUM_NAMES = ('num', 'den', 'tot', 'count')
UpscaledSums = collections.namedtuple('UpscaledSums', SUM_NAMES)


def _positions(pos, size):
    size = int(size)
    if not 1 <= size <= _d.MAX_EXTENT:
        raise ValueError('size must be between 1 and %d, got %d' % (_d.MAX_EXTENT, size))
    pos = np.asarray(pos, np.float64)
    if pos.ndim != 1:
        raise ValueError('a position table must be one-dimensional, got shape %r' % (pos.shape,))
    if pos.size > _d.MAX_EXTENT:
        raise ValueError('a position table must have at most %d entries, got %d' % (_d.MAX_EXTENT, pos.size))
    if not np.all(np.isfinite(pos)):
        raise ValueError('a position table holds a value that is not finite')
    return pos, size


def cell_table(pos, size, wrap=False):
    '''One axis: positions in units of coarse cells -> the cell (int32) of every fine index, for a
    coarse axis of ``size`` cells. Without ``wrap``: ``i0 = floor(pos)``, ``f = pos - i0``, ``cell = i0
    + (f >= 0.5)``, and -1 where that lies outside ``[0, size)``: the pixel belongs to no cell (it is
    NOT held to the edge, as the interpolation holds it). With ``wrap`` (a global longitude axis) ``p``
    is reduced as ``downscale.corner_tables`` reduces it -- ``p = pos - floor(pos / size) * size``, 0
    where that rounds up to ``size`` -- and ``cell = (floor(p) + (f >= 0.5)) % size``. ``f == 0.5``
    goes to the far cell. ValueError for a non-finite position.'''
    pos, size = _positions(pos, size)
    with np.errstate(all='ignore'):
        if wrap:
            p = pos - np.floor(pos / np.float64(size)) * np.float64(size)
            p = np.where((p >= size) | (p < 0), 0.0, p)
            i0 = np.floor(p)
            f = p - i0
            cell = (i0.astype(np.int64) + (f >= 0.5)) % size
        else:
            i0 = np.floor(pos)
            f = pos - i0
            cell = np.clip(i0, -2.0, np.float64(size) + 1.0).astype(np.int64) + (f >= 0.5)
            cell = np.where((cell < 0) | (cell >= size), -1, cell)
    return cell.astype(np.int32)


def cell_runs(cells, size, wrap=False):
    '''``(first[size], count[size])`` (int32) of a cell table: the fine indices of a cell must form
    ONE run of consecutive indices, ``first + k`` for ``k = 0 ... count - 1``; with ``wrap`` the run is
    cyclic, ``(first + k) % n``, starting at the index whose cyclic predecessor is not in the cell.
    ValueError otherwise. An empty cell has ``count = 0`` (and ``first = 0``). Increasing and decreasing
    positions both give such runs.'''
    cells = np.asarray(cells)
    size = int(size)
    if cells.ndim != 1 or cells.dtype.kind not in 'iu':
        raise ValueError('a cell table must be a one-dimensional integer array')
    cells = cells.astype(np.int64)
    n = cells.size
    if n and (cells.min() < -1 or cells.max() >= size):
        raise ValueError('a cell table holds a cell outside [-1, %d)' % size)
    first = np.zeros(size, np.int64)
    count = np.zeros(size, np.int64)
    if n:
        inside = cells >= 0
        count = np.bincount(cells[inside], minlength=size).astype(np.int64)
        start = np.ones(n, bool)
        start[1:] = cells[1:] != cells[:-1]
        if wrap:
            start[0] = cells[0] != cells[-1]
            if not start.any():                    # one cell holds the whole axis
                start[0] = True
        at = np.flatnonzero(start & inside)
        owner = cells[at]
        twice = np.flatnonzero(np.bincount(owner, minlength=1) > 1)
        if twice.size:
            raise ValueError('the fine indices of cell %d do not form one run of consecutive indices' % int(twice[0]))
        first[owner] = at
    return Runs(first.astype(np.int32), count.astype(np.int32))


def check_runs(runs, n, size, what, wrap=False):
    '''``(first, count)`` of one axis as contiguous int32 arrays of ``size`` entries that name disjoint
    runs inside ``n`` fine indices (cyclic with ``wrap``); ValueError otherwise.'''
    if len(runs) != 2:
        raise ValueError('%s runs must be (first, count)' % what)
    first, count = (np.ascontiguousarray(t, np.int32) for t in runs)
    n, size = int(n), int(size)
    if first.shape != (size,) or count.shape != (size,):
        raise ValueError('%s runs must have shape (%d,), got %r and %r' % (what, size, first.shape, count.shape))
    f, c = first.astype(np.int64), count.astype(np.int64)
    some = c > 0
    if np.any(c < 0) or np.any(c > n) or np.any(some & ((f < 0) | (f >= n))) or (not wrap and np.any(some & (f + c > n))):
        raise ValueError('a %s run leaves the %d fine indices' % (what, n))
    order = np.argsort(f[some], kind='stable')
    lo, hi = f[some][order], (f + c)[some][order]
    if lo.size and (np.any(lo[1:] < hi[:-1]) or hi[-1] - n > lo[0]):
        raise ValueError('the %s runs are not contiguous: two cells share a fine index' % what)
    return Runs(first, count)


def _shapes(shape, coarse_shape):
    try:
        (R, C), (H, W) = (int(e) for e in shape), (int(e) for e in coarse_shape)
    except (TypeError, ValueError):
        raise ValueError('shape and coarse_shape must be (rows, cols) pairs, got %r and %r' % (shape, coarse_shape))
    for e in (R, C, H, W):
        if not 1 <= e <= _d.MAX_EXTENT:
            raise ValueError('rows, cols, coarse rows and coarse cols must be between 1 and %d, got %r over %r'
                             % (_d.MAX_EXTENT, (R, C), (H, W)))
    return (R, C), (H, W)


def check_geometry(shape, coarse_shape, row_pos, col_pos, wrap=False, col_affine=None):
    '''The checks of a rectilinear grid: -> ``((R, C), (H, W), row_runs, col_runs)``. Row-affine columns
    (``col_affine`` with ``col_pos=None``) have ``check_geometry_rows``.'''
    if (col_pos is None) == (col_affine is None):
        raise ValueError('exactly one of col_pos and col_affine must be given')
    if col_affine is not None:
        raise ValueError('col_affine (row-affine columns) has no column runs: its checks are check_geometry_rows')
    (R, C), (H, W) = _shapes(shape, coarse_shape)
    row_pos, col_pos = np.asarray(row_pos, np.float64), np.asarray(col_pos, np.float64)
    if row_pos.shape != (R,) or col_pos.shape != (C,):
        raise ValueError('row_pos and col_pos must have shapes (%d,) and (%d,), got %r and %r'
                         % (R, C, row_pos.shape, col_pos.shape))
    rows = cell_runs(cell_table(row_pos, H), H)
    cols = cell_runs(cell_table(col_pos, W, wrap), W, wrap)
    check_cell_size(rows, cols)
    return (R, C), (H, W), rows, cols


def check_col_range(col_range, R, C):
    '''``(col_first[R], col_count[R])`` or None (the whole row) -> two contiguous int32 arrays with ``0 <=
    first``, ``count >= 0`` and ``first + count <= C``; ValueError otherwise.'''
    R, C = int(R), int(C)
    if col_range is None:
        return Runs(np.zeros(R, np.int32), np.full(R, C, np.int32))
    if len(col_range) != 2:
        raise ValueError('col_range must be (col_first, col_count)')
    first, count = (np.asarray(t) for t in col_range)
    if first.dtype != np.int32 or count.dtype != np.int32:
        raise ValueError('col_range must hold two int32 arrays, got %s and %s' % (first.dtype, count.dtype))
    if first.shape != (R,) or count.shape != (R,):
        raise ValueError('col_range must hold two arrays of shape (%d,), got %r and %r' % (R, first.shape, count.shape))
    f, n = first.astype(np.int64), count.astype(np.int64)
    if np.any(f < 0) or np.any(n < 0) or np.any(f + n > C):
        raise ValueError('col_range leaves the %d columns of a row (0 <= first, 0 <= count, first + count <= cols)' % C)
    return Runs(np.ascontiguousarray(first), np.ascontiguousarray(count))


def check_rows(shape, coarse_cols, col_affine, wrap=False, col_range=None):
    '''The checks of row-affine columns -> ``((col_origin, col_scale), (col_first, col_count))``:
    ``downscale.check_affine``, ``check_col_range`` and the acceptance rule of the module docstring, O(R).'''
    R, C = int(shape[0]), int(shape[1])
    W = int(coarse_cols)
    if col_affine is None or len(col_affine) != 2:
        raise ValueError('col_affine must be (col_origin, col_scale)')
    origin, scale = _d.check_affine((R, C), col_affine[0], col_affine[1])
    first, count = check_col_range(col_range, R, C)
    if wrap:
        n = count.astype(np.int64)
        with np.errstate(all='ignore'):
            laps = (n > 1) & ~(np.abs(scale) * (n - 1).astype(np.float64) <= np.float64(W - 2))
        if laps.any():
            r = int(np.flatnonzero(laps)[0])
            raise ValueError('fine row %d may lap the periodic axis (abs(col_scale) * (columns - 1) = %r exceeds the %d '
                             'coarse columns - 2): give a narrower col_range or cut the raster' %
                             (r, float(abs(scale[r]) * float(n[r] - 1)), W))
    return (origin, scale), Runs(first, count)


def check_geometry_rows(shape, coarse_shape, row_pos, col_affine, wrap=False, col_range=None):
    '''The checks of a grid with row-affine columns: -> ``((R, C), (H, W), row_runs, (col_origin, col_scale),
    (col_first, col_count))``; ``col_range`` None comes back as the whole rows.'''
    (R, C), (H, W) = _shapes(shape, coarse_shape)
    row_pos = np.asarray(row_pos, np.float64)
    if row_pos.shape != (R,):
        raise ValueError('row_pos must have shape (%d,), got %r' % (R, row_pos.shape))
    rows = cell_runs(cell_table(row_pos, H), H)
    affine, col_range = check_rows((R, C), W, col_affine, wrap, col_range)
    check_cell_size(rows, col_range)
    return (R, C), (H, W), rows, affine, col_range


def cell_table_rows(col_origin, col_scale, cols, size, wrap=False, col_range=None):
    '''Row-affine columns: -> ``(R, C)`` int32, the coarse column of every pixel, -1 for "no cell":
    ``cell_table`` (both of its branches as they are) applied to ``downscale.column_positions(col_origin,
    col_scale, cols)``, and -1 outside the row's ``col_range``.'''
    pos = _d.column_positions(col_origin, col_scale, cols)
    R, C = pos.shape
    if R > _d.MAX_EXTENT:
        raise ValueError('col_origin must have at most %d entries, got %d' % (_d.MAX_EXTENT, R))
    _positions(np.zeros(0), size)
    cells = np.stack([cell_table(pos[r], size, wrap) for r in range(R)]) if R else np.zeros((0, C), np.int32)
    first, count = check_col_range(col_range, R, C)
    c = np.arange(C, dtype=np.int64)[None, :]
    inside = (c >= first.astype(np.int64)[:, None]) & (c < (first.astype(np.int64) + count)[:, None])
    return np.where(inside, cells, -1).astype(np.int32)


def cell_runs_rows(cells, size):
    '''``(first[R, W], count[R, W])`` (int32) of an ``(R, C)`` cell table: per fine row ``cell_runs(cells[r],
    size, wrap=False)`` -- the pixels of one cell in one fine row must be ONE run of consecutive columns,
    never cyclic in ``c``; ValueError naming the row and the cell otherwise.'''
    cells = np.asarray(cells)
    size = int(size)
    if cells.ndim != 2 or cells.dtype.kind not in 'iu':
        raise ValueError('a cell table of rows must be a two-dimensional integer array')
    R = cells.shape[0]
    first, count = np.zeros((R, size), np.int32), np.zeros((R, size), np.int32)
    for r in range(R):
        try:
            first[r], count[r] = cell_runs(cells[r], size, wrap=False)
        except ValueError as e:
            raise ValueError('fine row %d: %s' % (r, e))
    return Runs(first, count)


def check_cell_size(row_runs, col_runs):
    if int(np.max(row_runs[1], initial=0)) * int(np.max(col_runs[1], initial=0)) >= 2 ** 31:
        raise ValueError('a cell must hold fewer than 2^31 pixels (row_count * col_count)')


def check_area(area, R):
    '''-> None or ``area`` as a contiguous float64 ``(R,)`` array of positive finite weights.'''
    if area is None:
        return None
    area = np.ascontiguousarray(area, np.float64)
    if area.shape != (int(R),):
        raise ValueError('area must have shape (%d,) -- a weight per fine row --, got %r' % (R, area.shape))
    if not (np.all(np.isfinite(area)) and np.all(area > 0)):
        raise ValueError('area must be positive and finite')
    return area


def check_min_fraction(min_fraction):
    try:
        v = float(min_fraction)
    except (TypeError, ValueError):
        raise ValueError('min_fraction must be a number in [0, 1], got %r' % (min_fraction,))
    if not 0.0 <= v <= 1.0:                        # (NaN fails both comparisons)
        raise ValueError('min_fraction must lie in [0, 1], got %r' % (min_fraction,))
    return v


def check_layers(shape, fine_shape, what='values'):
    '''``(K, R, C)`` or ``(R, C)`` against the grid's fine shape -> ``(K, squeeze)``.'''
    shape = tuple(int(e) for e in shape)
    if len(shape) not in (2, 3) or shape[-2:] != tuple(fine_shape):
        raise ValueError('%s must have shape (K, %d, %d) or (%d, %d), got %r' % ((what,) + tuple(fine_shape) * 2 + (shape,)))
    K = shape[0] if len(shape) == 3 else 1
    if not 1 <= K <= MAX_LAYERS:
        raise ValueError('%s must have between 1 and %d layers, got %d' % (what, MAX_LAYERS, K))
    return K, len(shape) == 2


def check_dtype(dtype):
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('values must be float32 or float64, got %s' % dtype)
    return dtype


def _names(outputs, known):
    if isinstance(outputs, str):
        outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or len(set(outputs)) != len(outputs) or any(k not in known for k in outputs):
        raise ValueError('outputs must name one or more of %s, each once, got %r' % (', '.join(known), outputs))
    return tuple(k for k in known if k in outputs)


def check_outputs(outputs):
    '''-> the requested names in the order of ``OUTPUT_NAMES``; at least one, no unknown one, none twice.'''
    return _names(outputs, OUTPUT_NAMES)


def check_class_outputs(outputs):
    return _names(outputs, CLASS_OUTPUT_NAMES)


def output_table(names, shape, dtype=None):
    '''What ``aggregate`` or ``majority`` produces, in the order of ``OUTPUT_NAMES`` / ``CLASS_OUTPUT_NAMES``:
    name -> ``(shape, numpy dtype)`` for the requested ``names``; ``dtype`` is that of ``values``.'''
    kinds = dict(mean=dtype, fraction=dtype, count=np.int32, cls=np.uint8, share=np.float32)
    return {k: (tuple(shape), np.dtype(kinds[k])) for k in OUTPUT_NAMES + CLASS_OUTPUT_NAMES if k in names}


def valid_mask(valid=None):
    '''A set of class codes in ``[0, 32)`` (None: the 13 classes of the parameter table) -> the 32-bit
    mask ``mod16_upscale_classes`` takes.'''
    codes = range(13) if valid is None else valid
    mask = 0
    for c in codes:
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < MAX_CODES:
            raise ValueError('valid must hold class codes in [0, %d), got %r' % (MAX_CODES, c))
        mask |= 1 << int(c)
    return mask


def aggregate(values, row_runs, col_runs, area=None, min_fraction=0.0, outputs=OUTPUT_NAMES, wrap=False):
    '''The definition: ``values`` ``(K, R, C)`` or ``(R, C)``, float32 or float64 -> ``Upscaled(mean,
    fraction, count)``: ``mean`` and ``fraction`` ``(K, H, W)`` (or ``(H, W)``) in the dtype of
    ``values`` (float32: the float64 result rounded once), ``count`` int32; None for what ``outputs``
    does not name. ``wrap``: the column runs are cyclic. Vectorised over layers and cells, Python loops
    over the pixels of a cell: the statement the device result is compared with, not a fast path.'''
    values = np.asarray(values)
    dtype = check_dtype(values.dtype)
    if values.ndim not in (2, 3):
        raise ValueError('values must have shape (K, R, C) or (R, C), got %r' % (values.shape,))
    R, C = values.shape[-2:]
    K, squeeze = check_layers(values.shape, (R, C))
    rf, rc = check_runs(row_runs, R, len(row_runs[0]), 'row')
    cf, cc = check_runs(col_runs, C, len(col_runs[0]), 'column', wrap)
    check_cell_size((rf, rc), (cf, cc))
    area = check_area(area, R)
    min_fraction = check_min_fraction(min_fraction)
    names = check_outputs(outputs)
    H, W = rf.size, cf.size
    x3 = values.reshape(K, R, C).astype(np.float64)
    first2, count2 = np.broadcast_to(cf.astype(np.int64), (R, W)), np.broadcast_to(cc.astype(np.int64), (R, W))
    num, den, tot, cnt = _sums(x3, rf, rc, first2, count2, area)
    return _finish(num, den, tot, cnt, min_fraction, names, (H, W) if squeeze else (K, H, W), dtype)


def _sums(x3, rf, rc, first2, count2, area):
    '''The sums of the definition: ``x3`` ``(K, R, C)`` float64, the row runs, the column run of cell ``j`` in
    fine row ``r`` as ``first2[r, j]``, ``count2[r, j]`` (int64; rectilinear: the same in every row; cyclic
    mod ``C``) -> ``(num, den, tot, cnt)``, ``(K, H, W)`` float64 and int64. Vectorised over layers and
    cells, Python loops over the pixels of a cell.'''
    K, R, C = x3.shape
    H, W = rf.size, first2.shape[1]
    w = np.ones(R) if area is None else area
    num, den, tot = np.zeros((K, H, W)), np.zeros((K, H, W)), np.zeros((K, H, W))
    cnt = np.zeros((K, H, W), np.int64)
    with np.errstate(all='ignore'):
        for t in range(int(rc.max(initial=0))):
            rows_on = t < rc                               # (H,)
            r = np.where(rows_on, rf.astype(np.int64) + t, 0)
            cf, cc = first2[r], np.where(rows_on[:, None], count2[r], 0)       # (H, W)
            s = np.zeros((K, H, W))
            m = np.zeros((K, H, W), np.int64)
            for k in range(int(cc.max(initial=0))):
                cols_on = k < cc                           # (H, W)
                col = np.where(cols_on, (cf + k) % C, 0)
                x = x3[:, r[:, None], col]
                ok = cols_on[None] & ~np.isnan(x)
                s = np.where(ok, s + x, s)
                m += ok
            a = w[r][None, :, None]
            on = rows_on[None, :, None]
            num = np.where(on, num + a * s, num)
            den = np.where(on, den + a * m.astype(np.float64), den)
            tot = np.where(on, tot + a * cc.astype(np.float64)[None], tot)
            cnt += np.where(on, m, 0)
    return num, den, tot, cnt


def _finish(num, den, tot, cnt, min_fraction, names, shape, dtype):
    '''``fraction``, ``mean`` and ``count`` from the sums, by the rules of the module docstring.'''
    with np.errstate(all='ignore'):
        fraction = np.where(tot > 0, den / tot, 0.0)
        mean = np.where((cnt >= 1) & (den >= min_fraction * tot), num / den, np.nan)
    res = dict(mean=mean, fraction=fraction, count=cnt)
    table = output_table(names, shape, dtype)
    return Upscaled(*[res[k].astype(table[k][1]).reshape(table[k][0]) if k in table else None for k in OUTPUT_NAMES])


def check_sum_outputs(outputs):
    return _names(outputs, SUM_NAMES)


def sum_table(names, shape):
    '''What ``sums`` / ``sums_rows`` produce: name -> ``(shape, numpy dtype)`` for the requested ``names``.'''
    return {k: (tuple(shape), np.dtype(np.int32 if k == 'count' else np.float64)) for k in SUM_NAMES if k in names}


def _as_sums(num, den, tot, cnt, names, shape):
    res = dict(num=num, den=den, tot=tot, count=cnt)
    table = sum_table(names, shape)
    return UpscaledSums(*[res[k].astype(table[k][1]).reshape(table[k][0]) if k in table else None for k in SUM_NAMES])


def _values(values):
    values = np.asarray(values)
    dtype = check_dtype(values.dtype)
    if values.ndim not in (2, 3):
        raise ValueError('values must have shape (K, R, C) or (R, C), got %r' % (values.shape,))
    R, C = values.shape[-2:]
    K, squeeze = check_layers(values.shape, (R, C))
    return values.reshape(K, R, C).astype(np.float64), dtype, (K, R, C), squeeze


def sums(values, row_runs, col_runs, area=None, outputs=SUM_NAMES, wrap=False):
    '''``aggregate`` stopped before its divisions (rectilinear): -> ``UpscaledSums(num, den, tot, count)``,
    ``num``, ``den`` and ``tot`` float64 whatever the type of ``values``, ``count`` int32.'''
    x3, _, (K, R, C), squeeze = _values(values)
    rf, rc = check_runs(row_runs, R, len(row_runs[0]), 'row')
    cf, cc = check_runs(col_runs, C, len(col_runs[0]), 'column', wrap)
    check_cell_size((rf, rc), (cf, cc))
    area = check_area(area, R)
    names = check_sum_outputs(outputs)
    H, W = rf.size, cf.size
    first2, count2 = np.broadcast_to(cf.astype(np.int64), (R, W)), np.broadcast_to(cc.astype(np.int64), (R, W))
    return _as_sums(*_sums(x3, rf, rc, first2, count2, area), names, (H, W) if squeeze else (K, H, W))


def _rows_tables(shape, row_runs, col_affine, W, wrap, col_range):
    R, C = shape
    W = int(W)
    rf, rc = check_runs(row_runs, R, len(row_runs[0]), 'row')
    (origin, scale), col_range = check_rows((R, C), W, col_affine, wrap, col_range)
    check_cell_size((rf, rc), col_range)
    first2, count2 = cell_runs_rows(cell_table_rows(origin, scale, C, W, wrap, col_range), W)
    return rf, rc, first2.astype(np.int64), count2.astype(np.int64)


def sums_rows(values, row_runs, col_affine, W, wrap=False, col_range=None, area=None, outputs=SUM_NAMES):
    '''``aggregate_rows`` stopped before its divisions: -> ``UpscaledSums``, as ``sums`` gives them.'''
    x3, _, (K, R, C), squeeze = _values(values)
    rf, rc, first2, count2 = _rows_tables((R, C), row_runs, col_affine, W, wrap, col_range)
    area = check_area(area, R)
    names = check_sum_outputs(outputs)
    shape = (rf.size, int(W)) if squeeze else (K, rf.size, int(W))
    return _as_sums(*_sums(x3, rf, rc, first2, count2, area), names, shape)


def aggregate_rows(values, row_runs, col_affine, W, wrap=False, col_range=None, area=None, min_fraction=0.0,
                   outputs=OUTPUT_NAMES):
    '''``aggregate`` with row-affine columns: the column run of cell ``j`` is taken per fine row
    (``cell_runs_rows`` of ``cell_table_rows``), in the same order -- per fine row of the cell in run
    order, the columns in increasing ``c``, then the fold with ``area[r]`` and ``tot = tot + area[r] *
    float64(count[r, j])`` -- with the same ``fraction``, ``mean`` and ``count`` rules and rounding.'''
    x3, dtype, (K, R, C), squeeze = _values(values)
    rf, rc, first2, count2 = _rows_tables((R, C), row_runs, col_affine, W, wrap, col_range)
    area = check_area(area, R)
    min_fraction = check_min_fraction(min_fraction)
    names = check_outputs(outputs)
    shape = (rf.size, int(W)) if squeeze else (K, rf.size, int(W))
    return _finish(*_sums(x3, rf, rc, first2, count2, area), min_fraction, names, shape, dtype)


def merge(parts, min_fraction=0.0, dtype=np.float64, shape=None, offsets=None, wrap=False):
    '''The sums of several rasters (tiles) over one coarse grid -> ``Upscaled(mean, fraction, count)`` by the
    rules of ``aggregate``, in ``dtype`` (float32: the float64 result rounded once). ``parts`` is a sequence
    of ``UpscaledSums`` with all four fields, of equal shape -- or, with ``shape = (..., H, W)`` and ``offsets
    = ((i0, j0), ...)``, each part a window of the accumulator that starts at coarse row ``i0`` and column
    ``j0`` (columns modulo ``W`` with ``wrap``). The parts are added IN THE GIVEN ORDER, ``num = (num0 +
    num1) + num2 ...`` from +0.0, likewise ``den`` and ``tot``, ``count`` as int64: float64 addition is not
    associative, so the last bits of the result depend on the order of ``parts`` -- merge in a fixed order
    (by tile number, say) for reproducible products. ValueError if a count leaves int32.'''
    parts = [UpscaledSums(*p) for p in parts]
    if not parts:
        raise ValueError('merge needs at least one part')
    for p in parts:
        if any(a is None for a in p):
            raise ValueError('every part must have all of %s' % ', '.join(SUM_NAMES))
        if len({np.shape(a) for a in p}) != 1:
            raise ValueError('the fields of a part must have one shape')
    dtype = check_dtype(dtype)
    min_fraction = check_min_fraction(min_fraction)
    if (shape is None) != (offsets is None):
        raise ValueError('shape and offsets must be given together')
    if shape is None:
        shape = np.shape(parts[0].num)
        if any(np.shape(p.num) != shape for p in parts):
            raise ValueError('the parts must have equal shape (or give shape and offsets)')
        offsets = [(0, 0)] * len(parts)
    shape = tuple(int(e) for e in shape)
    offsets = [tuple(int(e) for e in o) for o in offsets]
    if len(shape) < 2 or len(offsets) != len(parts) or any(len(o) != 2 for o in offsets):
        raise ValueError('shape must be (..., H, W) and offsets one (i0, j0) per part')
    H, W = shape[-2:]
    num, den, tot = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    cnt = np.zeros(shape, np.int64)
    with np.errstate(all='ignore'):
        for p, (i0, j0) in zip(parts, offsets):
            ps = np.shape(p.num)
            if len(ps) != len(shape) or ps[:-2] != shape[:-2]:
                raise ValueError('a part of shape %r does not fit an accumulator of shape %r' % (ps, shape))
            h, w = ps[-2:]
            if i0 < 0 or i0 + h > H or w > W or (not wrap and (j0 < 0 or j0 + w > W)):
                raise ValueError('a part of %d x %d cells at offset %r leaves the %d x %d accumulator' % (h, w, (i0, j0), H, W))
            rows = slice(i0, i0 + h)
            cols = (j0 + np.arange(w)) % W
            for acc, add, kind in ((num, p.num, np.float64), (den, p.den, np.float64), (tot, p.tot, np.float64),
                                   (cnt, p.count, np.int64)):
                acc[..., rows, cols] = acc[..., rows, cols] + np.asarray(add).astype(kind)
    if cnt.size and cnt.max() > np.iinfo(np.int32).max:
        raise ValueError('a merged count leaves int32')
    return _finish(num, den, tot, cnt, min_fraction, OUTPUT_NAMES, shape, dtype)


def majority(cls, row_runs, col_runs, valid=None, outputs=CLASS_OUTPUT_NAMES, wrap=False):
    '''The definition for a class raster: ``cls`` ``(R, C)`` uint8 -> ``UpscaledClasses(cls uint8 (H, W),
    share float32 (H, W))``; ``valid``: the codes that count (None: 0 ... 12).'''
    cls = np.asarray(cls)
    if cls.ndim != 2 or cls.dtype != np.uint8:
        raise ValueError('cls must be a two-dimensional uint8 array, got %s %r' % (cls.dtype, cls.shape))
    R, C = cls.shape
    rf, rc = check_runs(row_runs, R, len(row_runs[0]), 'row')
    cf, cc = check_runs(col_runs, C, len(col_runs[0]), 'column', wrap)
    check_cell_size((rf, rc), (cf, cc))
    mask = valid_mask(valid)
    names = check_class_outputs(outputs)
    H, W = rf.size, cf.size
    row_cell = np.full(R, -1, np.int64)
    col_cell = np.full(C, -1, np.int64)
    for i in range(H):
        row_cell[int(rf[i]):int(rf[i]) + int(rc[i])] = i
    for j in range(W):
        col_cell[(int(cf[j]) + np.arange(int(cc[j]))) % C] = j
    code_ok = np.array([(mask >> c) & 1 if c < MAX_CODES else 0 for c in range(256)], bool)
    take = (row_cell[:, None] >= 0) & (col_cell[None, :] >= 0) & code_ok[cls]
    cell = (row_cell[:, None] * W + col_cell[None, :])[take]
    counts = np.bincount(cls[take].astype(np.int64) * (H * W) + cell, minlength=MAX_CODES * H * W).reshape(MAX_CODES, H, W)
    winner = counts.argmax(axis=0)                         # the first maximum: the lowest code
    best = counts.max(axis=0)
    pixels = rc.astype(np.float64)[:, None] * cc.astype(np.float64)[None, :]
    with np.errstate(all='ignore'):
        share = np.where(best > 0, best.astype(np.float64) / pixels, 0.0).astype(np.float32)
    res = dict(cls=np.where(best > 0, winner, NO_CLASS).astype(np.uint8), share=share)
    return UpscaledClasses(*[res[k] if k in names else None for k in CLASS_OUTPUT_NAMES])


def majority_rows(cls, row_runs, col_affine, W, wrap=False, col_range=None, valid=None, outputs=CLASS_OUTPUT_NAMES):
    '''``majority`` with row-affine columns: the pixels of cell ``(i, j)`` are those of its fine rows whose
    coarse column (``cell_table_rows``) is ``j``, their number ``sum_r count[r, j]`` is taken as an integer
    and then widened to float64; the same tie rule, ``valid`` mask and 255.'''
    cls = np.asarray(cls)
    if cls.ndim != 2 or cls.dtype != np.uint8:
        raise ValueError('cls must be a two-dimensional uint8 array, got %s %r' % (cls.dtype, cls.shape))
    R, C = cls.shape
    W = int(W)
    rf, rc, _, count2 = _rows_tables((R, C), row_runs, col_affine, W, wrap, col_range)
    mask = valid_mask(valid)
    names = check_class_outputs(outputs)
    H = rf.size
    (origin, scale), col_range = check_rows((R, C), W, col_affine, wrap, col_range)
    col_cell = cell_table_rows(origin, scale, C, W, wrap, col_range).astype(np.int64)
    row_cell = np.full(R, -1, np.int64)
    for i in range(H):
        row_cell[int(rf[i]):int(rf[i]) + int(rc[i])] = i
    code_ok = np.array([(mask >> c) & 1 if c < MAX_CODES else 0 for c in range(256)], bool)
    take = (row_cell[:, None] >= 0) & (col_cell >= 0) & code_ok[cls]
    cell = (row_cell[:, None] * W + col_cell)[take]
    counts = np.bincount(cls[take].astype(np.int64) * (H * W) + cell, minlength=MAX_CODES * H * W).reshape(MAX_CODES, H, W)
    winner = counts.argmax(axis=0)                         # the first maximum: the lowest code
    best = counts.max(axis=0)
    pixels = np.zeros((H, W), np.int64)
    np.add.at(pixels, row_cell[row_cell >= 0], count2[row_cell >= 0])
    with np.errstate(all='ignore'):
        share = np.where(best > 0, best.astype(np.float64) / pixels.astype(np.float64), 0.0).astype(np.float32)
    res = dict(cls=np.where(best > 0, winner, NO_CLASS).astype(np.uint8), share=share)
    return UpscaledClasses(*[res[k] if k in names else None for k in CLASS_OUTPUT_NAMES])
