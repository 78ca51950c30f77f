'''
Coarse-grid meteorology interpolated inside the forward run: the definition, in numpy, of what
``mod16_et_downscaled_*`` and ``mod16_downscale_fields_*`` compute (``RasterEngine.downscale_grid``,
``mod16_amd.evapotranspiration_downscaled``), and the argument checks of those calls. Host only:
nothing here touches the library or a device; the kernels (``csrc/mod16_downscale.hpp``) follow
``interpolate`` operation for operation.

A fine raster of ``R x C`` pixels lies over a coarse grid of ``H x W`` cells. The geometry is two
float64 tables, ``row_pos[R]`` and ``col_pos[C]``: the position of every fine row and column in
units of coarse cells, cell centres at the integers (``positions`` builds them for regular grids).
Any rectilinear pair of grids is covered. Per axis ``corner_tables`` turns the positions into two
cell indices and two weights; ``interpolate`` forms a pixel's value from the four surrounding cells.
All transcendental work happens in ``corner_tables``, on the host: the device multiplies and adds
only, and its result has the bits of ``interpolate``.

A second geometry, "row-affine columns", covers fine grids whose column mapping depends on the row
-- MODIS sinusoidal tiles, where ``lon = x / (R_earth cos(lat_row))``: the column position of pixel
``(r, c)`` is ``col_origin[r] + col_scale[r] * c``, two float64 per row (``sinusoidal_positions``
builds them for a tile). The rows keep their table; ``corner_tables_rows`` is ``corner_tables`` on
those ``(R, C)`` positions and ``interpolate_rows`` is ``interpolate`` with its tables. The device
forms the column pair per pixel with multiply, add, divide, floor and compare and reproduces these
bits. Out of scope in this geometry: ``'cos4'`` (its weights need a cosine), arbitrary per-pixel
positions, projections whose columns are not affine in ``c`` within a row, and the masking of
off-globe pixels of edge tiles (the class raster's job).
'''
import numpy as np

#: the 14 drivers in argument order
DRIVER_NAMES = (
    'lw_net_day', 'lw_net_night', 'sw_rad_day', 'sw_rad_night', 'sw_albedo',
    'temp_day', 'temp_night', 'temp_annual', 'tmin', 'vpd_day', 'vpd_night',
    'pressure', 'fpar', 'lai')
#: the eleven reanalysis drivers, in driver order: what is coarse unless the caller says otherwise
#: (albedo, fPAR and LAI are fine-grid data)
MET_DRIVERS = (
    'lw_net_day', 'lw_net_night', 'sw_rad_day', 'sw_rad_night',
    'temp_day', 'temp_night', 'temp_annual', 'tmin', 'vpd_day', 'vpd_night', 'pressure')
METHODS = ('nearest', 'bilinear', 'cos4')
#: a scalar, an array on the fine grid, an array on the coarse grid (the ``kinds`` of the C ABI)
KIND_SCALAR, KIND_FINE, KIND_COARSE = 0, 1, 2
MAX_EXTENT = 2 ** 30        # rows, columns, coarse rows, coarse columns: the library's limit


def positions(fine_first, fine_step, count, coarse_first, coarse_step):
    '''The position table of one axis of two regular grids: fine coordinate ``fine_first + k *
    fine_step`` (``k = 0 ... count - 1``) in units of coarse cells, ``(fine_first + k * fine_step -
    coarse_first) / coarse_step``, where ``coarse_first`` is the coordinate of the centre of coarse
    cell 0 and ``coarse_step`` the distance between two centres (negative for a north-to-south
    latitude axis).'''
    count = int(count)
    if count < 0:
        raise ValueError('count must not be negative, got %d' % count)
    if not np.isfinite(coarse_step) or coarse_step == 0:
        raise ValueError('coarse_step must be finite and not zero, got %r' % (coarse_step,))
    k = np.arange(count, dtype=np.float64)
    return (np.float64(fine_first) + k * np.float64(fine_step) - np.float64(coarse_first)) / np.float64(coarse_step)


def method_code(method):
    '''``'nearest'``, ``'bilinear'``, ``'cos4'`` -> 0, 1, 2 (``enum mod16_downscale_method``).'''
    if method not in METHODS:
        raise ValueError('method must be one of %s, got %r' % (', '.join(repr(m) for m in METHODS), method))
    return METHODS.index(method)


def corner_tables(pos, size, wrap=False, method='bilinear'):
    '''One axis: positions in units of coarse cells -> ``(i0, i1, w0, w1)``, the near and the far
    cell (int32) and their weights (float64, ``w0 = 1.0 - w1``), for a coarse axis of ``size`` cells.

    Without ``wrap`` the edge value is held outside the grid: ``p = min(max(pos, 0), size - 1)``,
    ``i0 = floor(p)``, ``f = p - i0``, ``i1 = min(i0 + 1, size - 1)``. With ``wrap`` (the longitude
    axis of a global grid) ``p = pos - floor(pos / size) * size``, 0 where that rounds up to
    ``size``; ``i0 = floor(p)``, ``f = p - i0``, ``i1 = (i0 + 1) % size``.

    The far cell's weight ``w1``: ``'nearest'`` 1.0 where ``f >= 0.5``, else 0.0; ``'bilinear'``
    ``f``; ``'cos4'`` ``b / (a + b)`` with ``a = cos(pi/2 * f)**4`` and ``b = cos(pi/2 * (1 - f))**4``, and
    exactly 0.0 where ``f == 0``: the float64 cosine of pi/2 is 6e-17, whose fourth power would give the
    far cell a weight of 1e-65 -- enough for its NaN to reach a pixel that sits on a cell centre.

    ``'cos4'`` is a SEPARABLE form of the cosine-to-the-fourth distance weighting that the
    operational MOD16 algorithm applies to the four reanalysis cells around a pixel: a weight per
    axis, multiplied. The operational weighting uses the great-circle distance to each of the four
    cells, which does not factor into a row and a column term; this is not that, and no equality
    with the operational product's interpolation is claimed.

    ValueError for a non-finite position, ``size < 1`` or a ``pos`` that is not one-dimensional.'''
    code = method_code(method)
    size = int(size)
    if size < 1:
        raise ValueError('size must be at least 1, got %d' % size)
    if size > MAX_EXTENT:
        raise ValueError('size must be at most %d, got %d' % (MAX_EXTENT, size))
    pos = np.asarray(pos, np.float64)
    if pos.ndim != 1:
        raise ValueError('a position table must be one-dimensional, got shape %r' % (pos.shape,))
    if not np.all(np.isfinite(pos)):
        raise ValueError('a position table holds a value that is not finite')
    with np.errstate(all='ignore'):
        if wrap:
            p = pos - np.floor(pos / np.float64(size)) * np.float64(size)
            p = np.where((p >= size) | (p < 0), 0.0, p)
            i0 = np.floor(p)
            f = p - i0
            i0 = i0.astype(np.int32)
            i1 = ((i0.astype(np.int64) + 1) % size).astype(np.int32)
        else:
            p = np.minimum(np.maximum(pos, 0.0), np.float64(size - 1))
            i0 = np.floor(p)
            f = p - i0
            i0 = i0.astype(np.int32)
            i1 = np.minimum(i0.astype(np.int64) + 1, size - 1).astype(np.int32)
        if code == 0:
            w1 = np.where(f >= 0.5, 1.0, 0.0)
        elif code == 1:
            w1 = f
        else:
            a = np.cos((np.pi / 2) * f) ** 4
            b = np.cos((np.pi / 2) * (1.0 - f)) ** 4
            w1 = np.where(f == 0.0, 0.0, b / (a + b))        # (cos(pi/2) is 6e-17 in float64, not 0)
        w1 = np.asarray(w1, np.float64)
        w0 = 1.0 - w1
    return i0, i1, w0, w1


def check_tables(tables, count, size, what):
    '''``(i0, i1, w0, w1)`` of one axis as contiguous int32 / float64 arrays of ``count`` entries
    whose indices lie in ``[0, size)`` and whose weights are finite; ValueError otherwise.'''
    if len(tables) != 4:
        raise ValueError('%s tables must be (i0, i1, w0, w1)' % what)
    i0, i1 = (np.ascontiguousarray(t, np.int32) for t in tables[:2])
    w0, w1 = (np.ascontiguousarray(t, np.float64) for t in tables[2:])
    for t in (i0, i1, w0, w1):
        if t.shape != (int(count),):
            raise ValueError('a %s table has shape %r, expected (%d,)' % (what, t.shape, count))
    for t in (i0, i1):
        if t.size and (t.min() < 0 or t.max() >= size):
            raise ValueError('a %s table holds an index outside [0, %d)' % (what, size))
    if not (np.all(np.isfinite(w0)) and np.all(np.isfinite(w1))):
        raise ValueError('a %s table holds a weight that is not finite' % what)
    return i0, i1, w0, w1


def interpolate(field, row_tables, col_tables):
    '''A coarse ``(H, W)`` field at every pixel of the fine raster -> ``(R, C)`` float64. The field
    is widened to float64 first. With the corners in the order (row i0, col i0), (i0, i1), (i1, i0),
    (i1, i1), a corner's weight is ``wr * wc`` (one multiplication), its term ``w * v`` where ``w !=
    0`` and ``+0.0`` where ``w == 0`` -- a corner without weight cannot poison a pixel with its NaN
    or infinity -- and the value ``((t00 + t01) + t10) + t11``, left to right, no contraction. A NaN
    in a corner with weight gives NaN; nothing is renormalised over the valid corners.'''
    field = np.asarray(field)
    if field.ndim != 2:
        raise ValueError('a coarse field must be two-dimensional, got shape %r' % (field.shape,))
    field = field.astype(np.float64)
    H, W = field.shape
    ri0, ri1, rw0, rw1 = check_tables(row_tables, len(row_tables[0]), H, 'row')
    ci0, ci1, cw0, cw1 = check_tables(col_tables, len(col_tables[0]), W, 'column')
    with np.errstate(all='ignore'):
        def term(ri, ci, wr, wc):
            w = wr[:, None] * wc[None, :]
            v = field[ri[:, None], ci[None, :]]
            return np.where(w != 0, w * v, 0.0)
        t00 = term(ri0, ci0, rw0, cw0)
        t01 = term(ri0, ci1, rw0, cw1)
        t10 = term(ri1, ci0, rw1, cw0)
        t11 = term(ri1, ci1, rw1, cw1)
        return ((t00 + t01) + t10) + t11


# ---- row-affine columns: fine grids whose column mapping depends on the row (MODIS sinusoidal tiles).
# The column position of pixel (r, c) is ``col_origin[r] + col_scale[r] * c``; the rows keep their table.

#: the methods of the row-affine geometry (no ``'cos4'``)
AFFINE_METHODS = ('nearest', 'bilinear')
#: the MODIS sinusoidal grid: radius of its sphere [m], tiles across and down, the edge of a tile [m]
SINUSOIDAL_RADIUS = 6371007.181
SINUSOIDAL_TILES = (36, 18)
SINUSOIDAL_TILE_EDGE = 2 * np.pi * SINUSOIDAL_RADIUS / 36


def check_affine(shape, col_origin, col_scale, method=None):
    '''The row-affine column geometry of an ``R x C`` raster -> ``(col_origin, col_scale)`` as
    contiguous float64 arrays of ``R`` entries. ValueError unless both are one-dimensional with
    ``R`` entries and, for every row, ``col_origin[r]``, ``col_scale[r]`` and ``col_origin[r] +
    col_scale[r] * (C - 1)`` are finite (finite end points make every position of the row finite),
    or where ``method`` is given and is ``'cos4'``: its weights need a cosine, and the contract of
    this geometry is that the device reproduces the definition's bits with multiply, add, divide,
    floor and compare only.'''
    if method is not None:
        method_code(method)
        if method not in AFFINE_METHODS:
            raise ValueError("method 'cos4' is not available with row-affine columns (col_affine): its weights need a "
                             "cosine, which the device would not reproduce bit for bit; use 'nearest' or 'bilinear'")
    R, C = int(shape[0]), int(shape[1])
    column_positions(col_origin, col_scale, C, _check_only=True)
    origin = np.ascontiguousarray(col_origin, np.float64)
    scale = np.ascontiguousarray(col_scale, np.float64)
    if origin.shape != (R,):
        raise ValueError('col_origin and col_scale have shape %r, expected (%d,)' % (origin.shape, R))
    return origin, scale


def column_positions(col_origin, col_scale, cols, _check_only=False):
    '''The column position of every pixel of a raster with row-affine columns -> ``(R, C)`` float64:
    ``col_origin[:, None] + col_scale[:, None] * arange(C)``, one multiplication and one addition,
    each rounded. ValueError unless both inputs are one-dimensional with equal length and, for every
    row, ``col_origin[r]``, ``col_scale[r]`` and ``col_origin[r] + col_scale[r] * (C - 1)`` are finite.'''
    origin = np.asarray(col_origin, np.float64)
    scale = np.asarray(col_scale, np.float64)
    cols = int(cols)
    if cols < 1 or cols > MAX_EXTENT:
        raise ValueError('cols must be between 1 and %d, got %d' % (MAX_EXTENT, cols))
    if origin.ndim != 1 or scale.ndim != 1:
        raise ValueError('col_origin and col_scale must be one-dimensional, got shapes %r and %r'
                         % (origin.shape, scale.shape))
    if origin.shape != scale.shape:
        raise ValueError('col_origin and col_scale must have equal length, got %d and %d' % (origin.size, scale.size))
    if not np.all(np.isfinite(origin)):
        raise ValueError('col_origin holds a value that is not finite')
    if not np.all(np.isfinite(scale)):
        raise ValueError('col_scale holds a value that is not finite')
    with np.errstate(all='ignore'):
        far = origin + scale * np.float64(cols - 1)
        if not np.all(np.isfinite(far)):
            raise ValueError('col_origin + col_scale * (cols - 1) is not finite in some row')
        if _check_only:
            return None
        return origin[:, None] + scale[:, None] * np.arange(cols, dtype=np.float64)[None, :]


def corner_tables_rows(col_origin, col_scale, cols, size, wrap=False, method='bilinear'):
    '''The column tables of a raster with row-affine columns -> ``(i0, i1, w0, w1)``, each ``(R, C)``:
    ``corner_tables`` applied to ``column_positions(col_origin, col_scale, cols)``, with the same
    formulas (clamp or wrap, ``floor``, ``f``, ``i1``, ``w1``, ``w0 = 1.0 - w1``). This is what the
    kernels form per pixel from the two float64 of the pixel's row.

    ``method`` is ``'nearest'`` or ``'bilinear'``. ``'cos4'`` raises ValueError for this geometry: its
    weights need a cosine, and the contract here is that the device reproduces the definition's bits
    with multiply, add, divide, floor and compare only.'''
    method_code(method)
    if method not in AFFINE_METHODS:
        raise ValueError("method 'cos4' is not available with row-affine columns: its weights need a cosine, which "
                         "the device would not reproduce bit for bit; use 'nearest' or 'bilinear'")
    pos = column_positions(col_origin, col_scale, cols)
    i0, i1, w0, w1 = corner_tables(pos.reshape(-1), size, wrap, method)
    return tuple(t.reshape(pos.shape) for t in (i0, i1, w0, w1))


def interpolate_rows(field, row_tables, col_tables_2d):
    '''``interpolate`` with ``(R, C)`` column tables (``corner_tables_rows``): the same corner order,
    the same ``w != 0`` rule and the same left-to-right sum without contraction -> ``(R, C)`` float64.'''
    field = np.asarray(field)
    if field.ndim != 2:
        raise ValueError('a coarse field must be two-dimensional, got shape %r' % (field.shape,))
    field = field.astype(np.float64)
    H, W = field.shape
    ri0, ri1, rw0, rw1 = check_tables(row_tables, len(row_tables[0]), H, 'row')
    if len(col_tables_2d) != 4:
        raise ValueError('column tables must be (i0, i1, w0, w1)')
    R = len(ri0)
    ci0, ci1 = (np.asarray(t, np.int32) for t in col_tables_2d[:2])
    cw0, cw1 = (np.asarray(t, np.float64) for t in col_tables_2d[2:])
    for t in (ci0, ci1, cw0, cw1):
        if t.ndim != 2 or t.shape[0] != R or t.shape != ci0.shape:
            raise ValueError('a column table has shape %r, expected (%d, C)' % (t.shape, R))
    for t in (ci0, ci1):
        if t.size and (t.min() < 0 or t.max() >= W):
            raise ValueError('a column table holds an index outside [0, %d)' % W)
    if not (np.all(np.isfinite(cw0)) and np.all(np.isfinite(cw1))):
        raise ValueError('a column table holds a weight that is not finite')
    with np.errstate(all='ignore'):
        def term(ri, ci, wr, wc):
            w = wr[:, None] * wc
            v = field[ri[:, None], ci]
            return np.where(w != 0, w * v, 0.0)
        t00 = term(ri0, ci0, rw0, cw0)
        t01 = term(ri0, ci1, rw0, cw1)
        t10 = term(ri1, ci0, rw1, cw0)
        t11 = term(ri1, ci1, rw1, cw1)
        return ((t00 + t01) + t10) + t11


def sinusoidal_positions(h, v, size, coarse_lat_first, coarse_lat_step, coarse_lon_first, coarse_lon_step):
    '''The geometry of MODIS sinusoidal tile ``(h, v)`` with ``size`` pixels per side (1200, 2400, 4800,
    or any positive int) over a regular latitude / longitude grid -> ``(row_pos[size],
    col_origin[size], col_scale[size])``: ``row_pos`` for ``corner_tables``, the other two for
    ``col_affine`` / ``corner_tables_rows``.

    The grid's public constants: a sphere of radius 6371007.181 m, 36 x 18 tiles of edge ``T = 2 pi R
    / 36``. The tile's upper-left corner is ``((h - 18) T, (9 - v) T)``; pixel centres lie at +0.5
    pixel; ``lat = y / R`` and ``lon = x / (R cos(lat))``. The coarse coordinates are in degrees, cell
    centres at the integers as in ``positions``: ``coarse_lat_first`` / ``coarse_lon_first`` are the
    centre of cell 0, the steps the distance between two centres (negative for north to south).

    On edge tiles the pixels beyond the globe's outline (``|lon| > 180`` degrees) get finite positions
    that wrap around the coarse grid like any other; masking them is the class raster's job. The
    sinusoidal grid is equal-area, so ``zonal`` needs no per-row ``area`` on it.

    ValueError for ``h`` outside 0..35, ``v`` outside 0..17, ``size < 1``, or a zero or non-finite step.'''
    h, v, size = int(h), int(v), int(size)
    if h < 0 or h >= SINUSOIDAL_TILES[0]:
        raise ValueError('h must be between 0 and 35, got %d' % h)
    if v < 0 or v >= SINUSOIDAL_TILES[1]:
        raise ValueError('v must be between 0 and 17, got %d' % v)
    if size < 1 or size > MAX_EXTENT:
        raise ValueError('size must be between 1 and %d, got %d' % (MAX_EXTENT, size))
    for step, what in ((coarse_lat_step, 'coarse_lat_step'), (coarse_lon_step, 'coarse_lon_step')):
        if not np.isfinite(step) or step == 0:
            raise ValueError('%s must be finite and not zero, got %r' % (what, step))
    for first, what in ((coarse_lat_first, 'coarse_lat_first'), (coarse_lon_first, 'coarse_lon_first')):
        if not np.isfinite(first):
            raise ValueError('%s must be finite, got %r' % (what, first))
    radius, edge = np.float64(SINUSOIDAL_RADIUS), np.float64(SINUSOIDAL_TILE_EDGE)
    pixel = edge / np.float64(size)
    k = np.arange(size, dtype=np.float64)
    y = np.float64(9 - v) * edge - (k + 0.5) * pixel
    lat = y / radius                                   # radians
    x0 = np.float64(h - 18) * edge + 0.5 * pixel       # the centre of column 0
    across = radius * np.cos(lat)                      # metres per radian of longitude in every row: > 0
    row_pos = (np.degrees(lat) - np.float64(coarse_lat_first)) / np.float64(coarse_lat_step)
    col_origin = (np.degrees(x0 / across) - np.float64(coarse_lon_first)) / np.float64(coarse_lon_step)
    col_scale = np.degrees(pixel / across) / np.float64(coarse_lon_step)
    return row_pos, col_origin, col_scale


def sinusoidal_columns(h, v, size):
    '''The columns of MODIS sinusoidal tile ``(h, v)`` with ``size`` pixels per side whose centre lies on
    the globe -> ``(col_first[size], col_count[size])`` int32, per tile row the one range of such
    columns (a count of 0: the row lies beyond the outline): ``abs(x_c) <= pi * across[r]`` with the
    centre ``x_c = x0 + c * pixel`` of column ``c`` and ``x0``, ``pixel`` and ``across`` formed as
    ``sinusoidal_positions`` forms them. What ``col_range`` of the upscaling takes, so that the
    off-globe pixels of an edge tile do not alias onto cells on the far side of a periodic axis.'''
    h, v, size = int(h), int(v), int(size)
    if h < 0 or h >= SINUSOIDAL_TILES[0]:
        raise ValueError('h must be between 0 and 35, got %d' % h)
    if v < 0 or v >= SINUSOIDAL_TILES[1]:
        raise ValueError('v must be between 0 and 17, got %d' % v)
    if size < 1 or size > MAX_EXTENT:
        raise ValueError('size must be between 1 and %d, got %d' % (MAX_EXTENT, size))
    radius, edge = np.float64(SINUSOIDAL_RADIUS), np.float64(SINUSOIDAL_TILE_EDGE)
    pixel = edge / np.float64(size)
    k = np.arange(size, dtype=np.float64)
    y = np.float64(9 - v) * edge - (k + 0.5) * pixel
    across = radius * np.cos(y / radius)
    x0 = np.float64(h - 18) * edge + 0.5 * pixel
    first, count = np.zeros(size, np.int32), np.zeros(size, np.int32)
    step = max(1, (1 << 22) // size)
    for r0 in range(0, size, step):                    # (blocks of rows: size x size booleans at 4800 are 23 MB)
        on = np.abs(x0 + k[None, :] * pixel) <= np.pi * across[r0:r0 + step, None]
        n = on.sum(axis=1)
        f = np.where(n > 0, on.argmax(axis=1), 0)
        last = size - 1 - on[:, ::-1].argmax(axis=1)
        assert np.all((n == 0) | (last - f + 1 == n)), 'the on-globe columns of a row are one range'
        first[r0:r0 + step], count[r0:r0 + step] = f, n
    return first, count


def check_coarse(coarse):
    '''``coarse`` of a downscaled call -> the tuple of driver names it holds, in driver order;
    ValueError for a name that is no driver or one named twice.'''
    if isinstance(coarse, str):
        raise ValueError('coarse must be a sequence of driver names, not a string')
    names = list(coarse)
    for name in names:
        if name not in DRIVER_NAMES:
            raise ValueError('coarse names %r, which is not one of %s' % (name, ', '.join(DRIVER_NAMES)))
    if len(set(names)) != len(names):
        raise ValueError('coarse names a driver twice')
    return tuple(n for n in DRIVER_NAMES if n in names)


def check_range(shape, first_pixel=0, n=None):
    '''The pixel range ``[first_pixel, first_pixel + n)`` of an ``R x C`` raster -> ``(first, n)``
    as ints (``n`` None: to the end); ValueError where it leaves the raster.'''
    total = int(shape[0]) * int(shape[1])
    first = int(first_pixel)
    if first < 0 or first > total:
        raise ValueError('first_pixel must be between 0 and %d, got %d' % (total, first))
    count = total - first if n is None else int(n)
    if count < 0 or first + count > total:
        raise ValueError('the pixel range [%d, %d) leaves the raster of %d pixels' % (first, first + count, total))
    return first, count


def check_call(shape, coarse_shape, driver_shapes, coarse=MET_DRIVERS, first_pixel=0, n=None,
               method='bilinear', cls_size=None, row_pos=None, col_pos=None):
    '''The argument checks of every downscaled call, before any device work.

    ``shape`` = ``(R, C)``, ``coarse_shape`` = ``(H, W)``; ``driver_shapes``: the shape of each of
    the 14 drivers (``()`` for a scalar). A driver named in ``coarse`` must be ``(H, W)``; any other
    is a scalar, the ``n`` pixels of the range as ``(n,)``, or -- for the whole raster -- ``(R, C)``.
    ``cls_size``: the elements of the class raster, which must be ``n``. ``row_pos`` / ``col_pos``:
    the position tables, which must hold ``R`` and ``C`` entries.

    Returns ``(kinds, first, n)``: the 14 kinds (``KIND_SCALAR``, ``KIND_FINE``, ``KIND_COARSE``) and
    the range as ints. ValueError otherwise.'''
    method_code(method)
    if len(shape) != 2 or len(coarse_shape) != 2:
        raise ValueError('shape and coarse_shape must be (rows, columns)')
    R, C = int(shape[0]), int(shape[1])
    H, W = int(coarse_shape[0]), int(coarse_shape[1])
    for v, what in ((R, 'rows'), (C, 'columns'), (H, 'coarse rows'), (W, 'coarse columns')):
        if v < 1 or v > MAX_EXTENT:
            raise ValueError('%s must be between 1 and %d, got %d' % (what, MAX_EXTENT, v))
    for pos, count, what in ((row_pos, R, 'row_pos'), (col_pos, C, 'col_pos')):
        if pos is not None and np.shape(pos) != (count,):
            raise ValueError('%s has shape %r, expected (%d,)' % (what, np.shape(pos), count))
    names = check_coarse(coarse)
    first, count = check_range((R, C), first_pixel, n)
    if len(driver_shapes) != len(DRIVER_NAMES):
        raise ValueError('expected 14 drivers, got %d' % len(driver_shapes))
    kinds = []
    for name, sh in zip(DRIVER_NAMES, driver_shapes):
        sh = tuple(int(x) for x in sh)
        if name in names:
            if sh != (H, W):
                raise ValueError('%s is a coarse driver: expected shape %r, got %r' % (name, (H, W), sh))
            kinds.append(KIND_COARSE)
        elif sh == ():
            kinds.append(KIND_SCALAR)
        elif sh == (count,) or (sh == (R, C) and first == 0 and count == R * C):
            kinds.append(KIND_FINE)
        else:
            raise ValueError('%s has shape %r: expected a scalar, the %d pixels of the range or the raster %r'
                             % (name, sh, count, (R, C)))
    if cls_size is not None and int(cls_size) != count:
        raise ValueError('the class raster has %d elements, expected %d' % (cls_size, count))
    return kinds, first, count


# ---- composites over coarse drivers (``mod16_et_composite_downscaled_*``, ``DownscaleGrid.composite``,
# ``mod16_amd.evapotranspiration_composite_downscaled``): any of the 15 arrays of
# ``mod16_amd.composite.ARRAY_NAMES`` -- the 14 drivers and the hours of daylight -- a scalar, a fine
# array or a coarse array, the last two with or without a time axis

#: a fine array with a leading time axis, a coarse array with one (after KIND_SCALAR, KIND_FINE, KIND_COARSE)
KIND_FINE_TIME, KIND_COARSE_TIME = 3, 4


def check_coarse_arrays(coarse):
    '''``coarse`` of a composite call over coarse drivers -> the tuple of array names it holds, in the
    order of ``mod16_amd.composite.ARRAY_NAMES`` (``'day_hours'`` may be among them: the hours of
    daylight are a function of latitude and day); ValueError for a name that is no array of the
    call or one named twice.'''
    from .composite import ARRAY_NAMES
    if isinstance(coarse, str):
        raise ValueError('coarse must be a sequence of array names, not a string')
    names = list(coarse)
    for name in names:
        if name not in ARRAY_NAMES:
            raise ValueError('coarse names %r, which is not one of %s' % (name, ', '.join(ARRAY_NAMES)))
    if len(set(names)) != len(names):
        raise ValueError('coarse names an array twice')
    return tuple(n for n in ARRAY_NAMES if n in names)


def coarse_mask(names):
    '''The C ABI's ``coarse_mask`` of the names ``check_coarse_arrays`` returned: bit k for array k
    of ``ARRAY_NAMES`` (bit 14: the hours of daylight).'''
    from .composite import ARRAY_NAMES
    return sum(1 << ARRAY_NAMES.index(n) for n in names)


def coarse_grid_shape(names, array_shapes):
    '''``(H, W)`` of the coarse grid of a composite call: the last two extents of the arrays named
    coarse (``array_shapes``: the 15 shapes in ``ARRAY_NAMES`` order), which must be ``(H, W)`` or
    ``(S, H, W)`` and agree; ``(1, 1)`` where nothing is coarse. ValueError otherwise.'''
    from .composite import ARRAY_NAMES
    grid, owner = None, None
    for name, sh in zip(ARRAY_NAMES, array_shapes):
        if name not in names:
            continue
        sh = tuple(int(x) for x in sh)
        if len(sh) not in (2, 3):
            raise ValueError('%s is a coarse array: expected shape (H, W) or (S, H, W), got %r' % (name, sh))
        if grid is not None and sh[-2:] != grid:
            raise ValueError('the coarse arrays must share one grid: %s is %r, %s is %r' % (owner, grid, name, sh[-2:]))
        if grid is None:
            grid, owner = sh[-2:], name
    return grid if grid is not None else (1, 1)


def check_composite_call(shape, coarse_shape, array_shapes, days, every=None, coarse=MET_DRIVERS, first_pixel=0,
                         n=None, cls_size=None):
    '''The shape checks of every composite call over coarse drivers, before any device work.

    ``shape`` = ``(R, C)``, ``coarse_shape`` = ``(H, W)``; ``array_shapes``: the shape of each of the
    15 arrays of ``ARRAY_NAMES`` (``()`` for a scalar); ``days`` and ``every`` as for the composite
    (``mod16_amd.composite.check_every``). With ``S = ceil(days / every[name])``, an array named in
    ``coarse`` must be ``(H, W)`` (constant in time) or ``(S, H, W)``; any other is a scalar, the
    ``n`` pixels of the range as ``(n,)`` or ``(S, n)``, or -- for the whole raster -- ``(R, C)`` or
    ``(S, R, C)``. ``cls_size``: the elements of the class raster, which must be ``n``.

    Returns ``(kinds, slabs, first, n)``: per array its kind (``KIND_SCALAR``, ``KIND_FINE``,
    ``KIND_FINE_TIME``, ``KIND_COARSE``, ``KIND_COARSE_TIME``) and its time slabs (1 without a
    time axis), and the range as ints. ValueError otherwise.'''
    from . import composite as _c
    if len(shape) != 2 or len(coarse_shape) != 2:
        raise ValueError('shape and coarse_shape must be (rows, columns)')
    R, C = int(shape[0]), int(shape[1])
    H, W = int(coarse_shape[0]), int(coarse_shape[1])
    for v, what in ((R, 'rows'), (C, 'columns'), (H, 'coarse rows'), (W, 'coarse columns')):
        if v < 1 or v > MAX_EXTENT:
            raise ValueError('%s must be between 1 and %d, got %d' % (what, MAX_EXTENT, v))
    names = check_coarse_arrays(coarse)
    ev = _c.check_every(every)
    K = _c.check_periods(days, 1)[0]
    first, count = check_range((R, C), first_pixel, n)
    whole = first == 0 and count == R * C
    if len(array_shapes) != len(_c.ARRAY_NAMES):
        raise ValueError('expected 15 arrays (14 drivers and day_hours), got %d' % len(array_shapes))
    kinds, slabs = [], []
    for name, sh in zip(_c.ARRAY_NAMES, array_shapes):
        sh = tuple(int(x) for x in sh)
        timed = None
        if name in names:
            if sh == (H, W):
                kinds.append(KIND_COARSE)
            elif len(sh) == 3 and sh[1:] == (H, W):
                kinds.append(KIND_COARSE_TIME)
                timed = sh[0]
            else:
                raise ValueError('%s is a coarse array: expected shape %r or (S, %d, %d), got %r' % (name, (H, W), H, W, sh))
        elif sh == ():
            kinds.append(KIND_SCALAR)
        elif sh == (count,) or (sh == (R, C) and whole):
            kinds.append(KIND_FINE)
        elif (len(sh) == 2 and sh[1] == count) or (len(sh) == 3 and sh[1:] == (R, C) and whole):
            kinds.append(KIND_FINE_TIME)
            timed = sh[0]
        else:
            raise ValueError('%s has shape %r: expected a scalar, the %d pixels of the range or the raster %r, '
                             'each with or without a leading time axis' % (name, sh, count, (R, C)))
        if timed is not None:
            _c.check_slabs(name, timed, K, ev[name])
        slabs.append(1 if timed is None else timed)
    if cls_size is not None and int(cls_size) != count:
        raise ValueError('the class raster has %d elements, expected %d' % (cls_size, count))
    return kinds, slabs, first, count
