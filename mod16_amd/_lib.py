'''
ctypes binding of ``libmod16hip.so`` (C ABI: ``include/mod16_hip.h``).

There is no CPU fallback: if the library is missing, or no MI355X is visible
when a computation is requested, the call fails loudly.
'''
import ctypes as C
import os
import threading
import weakref

import numpy as np

N_DRIVERS = 14
N_PARAMS = 11
N_CLASSES = 13
N_COMPONENTS = 6
HOST, DEVICE = 0, 1
BC_SCALAR, BC_DENSE, BC_ROW, BC_COL = 0, 1, 2, 3      # enum mod16_broadcast
MATH_FAST, MATH_EXACT, MATH_MIXED = 0, 1, 2
DOMAIN_TRUSTED = 4        # flag bit MOD16_DOMAIN_TRUSTED: or it into a math value (include/mod16_hip.h)
# enum mod16_form: (wide arrays, byte rasters, outputs) of each form of the forward run
(FORM_TOTALS, FORM_PET, FORM_COMPONENTS, FORM_TOTALS_COMPONENTS, FORM_RAW, FORM_RAW_TOTAL8,
 FORM_RAW_TOTAL8_HOURS) = range(7)
FORM_SHAPE = {FORM_TOTALS: (14, 1, 2), FORM_PET: (14, 1, 4), FORM_COMPONENTS: (14, 1, 6),
              FORM_TOTALS_COMPONENTS: (14, 1, 8), FORM_RAW: (14, 3, 2), FORM_RAW_TOTAL8: (14, 3, 3),
              FORM_RAW_TOTAL8_HOURS: (15, 3, 3)}

METHOD_MAX_IN = 13
(M_SVP, M_SVP_SLOPE, M_LHV, M_PSYCHROMETRIC, M_RADIATION_NET, M_AIR_DENSITY,
 M_AIR_PRESSURE, M_VPD, M_RHUMIDITY, M_POT_SOIL_EVAP, M_POT_TRANSPIRATION,
 M_EVAP_SOIL, M_EVAP_WET_CANOPY, M_RADIATION_SOIL, M_SOIL_HEAT_FLUX,
 M_SURFACE_CONDUCTANCE, M_TRANSPIRATION_DAY, M_TRANSPIRATION_NIGHT) = range(18)

OK = 0
ERR_ARG, ERR_HIP, ERR_CLASS_RANGE, ERR_NOMEM, ERR_NO_DEVICE, ERR_NO_BPLUT = \
    -1, -2, -3, -4, -5, -6

ABI_VERSION = 16
LIB_NAME = 'libmod16hip.so'
# MOD16_LIB: alternative build of the same library (kernel experiments only)
LIB_PATH = os.environ.get('MOD16_LIB') or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
# the same sources built with -DMOD16_EXPERIMENTS (launch-geometry overrides read from the
# environment at context creation): tests and tools only, see load_experiments()
EXP_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libmod16hip_exp.so')


class Mod16Error(RuntimeError):
    '''A failed call into libmod16hip (anything but a class-range error).'''

    def __init__(self, status, message):
        super().__init__('libmod16hip: %s (status %d)' % (message, status))
        self.status = status


def overlap_as_value_error(e):
    '''``except Mod16Error as e: raise overlap_as_value_error(e)``: the library's refusal of an output
    that overlaps an input (or another output) is the caller's mistake in the arguments -- ValueError, as
    the other argument checks raise; any other error is raised again as it is.'''
    if e.status == ERR_ARG and 'overlaps' in str(e):
        return ValueError(str(e))
    return e


_PP = C.POINTER(C.c_void_p)
_I64P = C.POINTER(C.c_int64)


class Layout(C.Structure):
    '''``mod16_layout`` (include/mod16_hip.h): pixel i of an array of a tiled
    raster lives at ``base[(i // tile) * row + (i % tile)]``.'''
    _fields_ = [('tile', C.c_int64), ('driver_row', C.c_int64),
                ('out_row', C.c_int64), ('cls_row', C.c_int64)]


_LAYP = C.POINTER(Layout)


PRIOR_UNIFORM, PRIOR_LOGNORMAL, PRIOR_TRIANGULAR = 0, 1, 2     # enum mod16_prior
CONSTRAINT_ANNUAL_PRECIP = 1      # MOD16_CONSTRAINT_ANNUAL_PRECIP: a bit of mod16_mcmc_spec.constraints
FOLD_HELDOUT = 0x100      # MOD16_FOLD_HELDOUT: or it into a fold code (include/mod16_hip.h)


class McmcSpec(C.Structure):
    '''``mod16_mcmc_spec`` (include/mod16_hip.h): the sampler's chains, free parameters, priors and tuning.'''
    _fields_ = [('chains', C.c_int32), ('nfree', C.c_int32), ('index', C.c_int32 * 11),
                ('family', C.c_int32 * 11), ('p0', C.c_double * 11), ('p1', C.c_double * 11),
                ('p2', C.c_double * 11), ('fixed', C.c_double * 11), ('lamb', C.c_double),
                ('scaling', C.c_double), ('tune_target', C.c_int32), ('tune_interval', C.c_int32),
                ('tune_steps', C.c_int64), ('tune_drop_fraction', C.c_double), ('objective', C.c_int32),
                ('segment', C.c_int32), ('seed', C.c_uint64), ('constraints', C.c_int32),
                ('reserved_', C.c_int32)]

class CompositeSpec(C.Structure):
    '''``mod16_composite_spec`` (include/mod16_hip.h): the pixels, days and periods of a composite call
    and, per driver and for the hours of daylight, a pixel stride, a time stride and a divisor.'''
    _fields_ = [('n', C.c_int64), ('days', C.c_int32), ('period_days', C.c_int32), ('min_valid', C.c_int32),
                ('rescale', C.c_int32), ('pixel_stride', C.c_int64 * 14), ('time_stride', C.c_int64 * 14),
                ('every', C.c_int32 * 14), ('hours_pixel_stride', C.c_int64), ('hours_time_stride', C.c_int64),
                ('hours_every', C.c_int32), ('reserved_', C.c_int32)]


_COMPOSITE_ARGS = [C.c_void_p, C.POINTER(CompositeSpec), C.c_void_p, _PP, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_int64, C.c_uint, C.c_int, C.c_void_p, C.c_int64]

class GapfillSpec(C.Structure):
    '''``mod16_gapfill_spec`` (include/mod16_hip.h): the pixels, slabs, fields, output type, scales,
    gap limit and pitches of a gap-filling call.'''
    _fields_ = [('n', C.c_int64), ('slabs', C.c_int32), ('nfields', C.c_int32), ('out_type', C.c_int32),
                ('max_gap', C.c_int32), ('scale', C.c_double * 3), ('in_pitch', C.c_int64),
                ('qc_pitch', C.c_int64), ('out_pitch', C.c_int64), ('source_pitch', C.c_int64)]


GAPFILL_U8, GAPFILL_F32, GAPFILL_F64 = 0, 1, 2     # enum mod16_gapfill_out


class SmoothSpec(C.Structure):
    '''``mod16_smooth_spec`` (include/mod16_hip.h): the pixels and slabs of a smoothing call, the order
    of the penalty, the envelope rounds, the fewest weighted slabs a pixel is smoothed from, the weight
    mode and output type, ``lam``, the scale and the pitches.'''
    _fields_ = [('n', C.c_int64), ('slabs', C.c_int32), ('order', C.c_int32), ('envelope', C.c_int32),
                ('min_valid', C.c_int32), ('weight_mode', C.c_int32), ('out_type', C.c_int32),
                ('lam', C.c_double), ('scale', C.c_double), ('in_pitch', C.c_int64),
                ('weight_pitch', C.c_int64), ('out_pitch', C.c_int64)]


SMOOTH_U8, SMOOTH_F32, SMOOTH_F64 = 0, 1, 2                         # enum mod16_smooth_out
SMOOTH_WEIGHT_NONE, SMOOTH_WEIGHT_STACK, SMOOTH_WEIGHT_QC = 0, 1, 2    # enum mod16_smooth_weight
_SMOOTH_ARGS = [C.c_void_p, C.POINTER(SmoothSpec)] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_size_t]


class RegressSpec(C.Structure):
    '''``mod16_regress_spec`` (include/mod16_hip.h): the pixels and steps of a regression call, the shared
    and the per-pixel terms, the fewest valid samples a pixel is fitted from, the series mode and the
    pitches.'''
    _fields_ = [('n', C.c_int64), ('steps', C.c_int32), ('ks', C.c_int32), ('kp', C.c_int32),
                ('min_valid', C.c_int32), ('series', C.c_int32), ('flags', C.c_int32),
                ('value_pitch', C.c_int64), ('term_pitch', C.c_int64), ('weight_pitch', C.c_int64),
                ('coef_pitch', C.c_int64), ('se_pitch', C.c_int64), ('series_pitch', C.c_int64)]


REGRESS_SERIES_NONE, REGRESS_SERIES_RESIDUALS, REGRESS_SERIES_FITTED = 0, 1, 2     # enum mod16_regress_series
_REGRESS_ARGS = [C.c_void_p, C.POINTER(RegressSpec)] + [C.c_void_p] * 11 + [C.c_int, C.c_void_p, C.c_size_t]


class DaynightSpec(C.Structure):
    '''``mod16_daynight_spec`` (include/mod16_hip.h): the grid, days and steps per day, the mode and its
    threshold, the output type, and the row pitch and plane stride of the fields and of the outputs.'''
    _fields_ = [('rows', C.c_int64), ('cols', C.c_int64), ('days', C.c_int32), ('steps_per_day', C.c_int32),
                ('mode', C.c_int32), ('out_type', C.c_int32), ('threshold', C.c_double), ('in_pitch', C.c_int64),
                ('in_plane', C.c_int64), ('out_pitch', C.c_int64), ('out_plane', C.c_int64)]


DAYNIGHT_SOLAR, DAYNIGHT_SW = 0, 1        # enum mod16_daynight_mode
DAYNIGHT_F32, DAYNIGHT_F64 = 0, 1         # enum mod16_daynight_out
_DAYNIGHT_ARGS = [C.c_void_p, C.POINTER(DaynightSpec), _PP, C.c_void_p, C.c_void_p, C.c_void_p, _PP, C.c_void_p,
                  C.c_int, C.c_void_p, C.c_size_t]


class TrendSpec(C.Structure):
    '''``mod16_trend_spec`` (include/mod16_hip.h): the pixels and steps of a trend call, the fewest valid
    values a trend is computed from, the stride in time and the normal quantile of the interval.'''
    _fields_ = [('n', C.c_int64), ('steps', C.c_int32), ('min_valid', C.c_int32), ('time_stride', C.c_int64),
                ('zq', C.c_double)]


_TREND_ARGS = [C.c_void_p, C.POINTER(TrendSpec), C.c_void_p, C.c_void_p, _PP, C.c_void_p, C.c_void_p, C.c_int,
               C.c_void_p, C.c_size_t]


class AnomalySpec(C.Structure):
    '''``mod16_anomaly_spec`` (include/mod16_hip.h): the pixels, years and periods of an anomaly call,
    the window, the baseline years, the fewest valid baseline values a climatology is computed from and
    the strides of the inputs, of ``z`` / ``pct`` and of the climatology.'''
    _fields_ = [('n', C.c_int64), ('years', C.c_int32), ('periods', C.c_int32), ('window', C.c_int32),
                ('base_first', C.c_int32), ('base_end', C.c_int32), ('min_valid', C.c_int32),
                ('in_stride', C.c_int64), ('out_stride', C.c_int64), ('clim_stride', C.c_int64)]


_ANOMALY_ARGS = [C.c_void_p, C.POINTER(AnomalySpec)] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_size_t]


class UpscaleSpec(C.Structure):
    '''``mod16_upscale_spec`` (include/mod16_hip.h): the fine raster, the coarse grid, whether its column
    runs are cyclic.'''
    _fields_ = [('rows', C.c_int64), ('cols', C.c_int64), ('coarse_rows', C.c_int64), ('coarse_cols', C.c_int64),
                ('wrap_cols', C.c_int32), ('reserved_', C.c_int32)]


_UPSCALE_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_double] + \
    [C.c_void_p, C.c_int64, C.c_int64] * 3 + [C.c_int, C.c_void_p, C.c_size_t]
_UPSCALE_SUMS_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64] + \
    [C.c_void_p, C.c_int64, C.c_int64] * 4 + [C.c_int, C.c_void_p, C.c_size_t]


class DownscaleSpec(C.Structure):
    '''``mod16_downscale_spec`` (include/mod16_hip.h): the fine raster, the coarse grid, whether its
    column axis is periodic, the weighting method.'''
    _fields_ = [('rows', C.c_int64), ('cols', C.c_int64), ('coarse_rows', C.c_int64), ('coarse_cols', C.c_int64),
                ('wrap_cols', C.c_int32), ('method', C.c_int32)]


class ZonalSpec(C.Structure):
    '''``mod16_zonal_spec`` (include/mod16_hip.h): the pixels, layers and zones of a zonal call, the
    types of its zone ids and weights, the raster geometry of per-row weights, the value pitch, and
    the bounds with their exponents.'''
    _fields_ = [('n', C.c_int64), ('layers', C.c_int32), ('nzones', C.c_int32), ('zone_type', C.c_int32),
                ('weight_kind', C.c_int32), ('cols', C.c_int64), ('first_pixel', C.c_int64),
                ('value_pitch', C.c_int64), ('ew', C.c_int32), ('ex', C.c_int32), ('wmax', C.c_double),
                ('xmax', C.c_double)]


ZONE_U8, ZONE_U16, ZONE_I32 = 0, 1, 2                           # enum mod16_zone_type
ZONAL_WEIGHT_NONE, ZONAL_WEIGHT_ROW, ZONAL_WEIGHT_PIXEL = 0, 1, 2     # enum mod16_zonal_weight
_ZONAL_ARGS = [C.c_void_p, C.POINTER(ZonalSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
               C.c_void_p, C.c_size_t]
_ZONAL_BOUNDS_ARGS = [C.c_void_p, C.POINTER(ZonalSpec), C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                      C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_size_t]


class ZonalHistSpec(C.Structure):
    '''``mod16_zonal_hist_spec`` (include/mod16_hip.h): the geometry fields of ``mod16_zonal_spec``, the
    weight bound with its exponent, the mode, the uniform histogram's bins, range and scale, the
    width of a value and the digit histogram's bits, level and slots.'''
    _fields_ = [('n', C.c_int64), ('layers', C.c_int32), ('nzones', C.c_int32), ('zone_type', C.c_int32),
                ('weight_kind', C.c_int32), ('cols', C.c_int64), ('first_pixel', C.c_int64),
                ('value_pitch', C.c_int64), ('ew', C.c_int32), ('mode', C.c_int32), ('wmax', C.c_double),
                ('bins', C.c_int32), ('width', C.c_int32), ('lo', C.c_double), ('hi', C.c_double),
                ('scale', C.c_double), ('bits', C.c_int32), ('level', C.c_int32), ('slots', C.c_int32),
                ('reserved', C.c_int32)]


ZONAL_HIST_UNIFORM, ZONAL_HIST_DIGIT = 0, 1                     # enum mod16_zonal_hist_mode
_ZONAL_HIST_ARGS = [C.c_void_p, C.POINTER(ZonalHistSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                    C.c_int, C.c_void_p, C.c_size_t]
_ZONAL_SELECT_ARGS = [C.c_void_p, C.POINTER(ZonalHistSpec), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

_I32P = C.POINTER(C.c_int32)
_DOWNSCALED_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I32P, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                    C.c_void_p, C.c_uint, C.c_int, C.c_void_p]
_DOWNSCALE_FIELDS_ARGS = [C.c_void_p, C.c_void_p, _PP, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                          C.c_int64, C.c_int, C.c_void_p]


class CompositeDownscaledSpec(C.Structure):
    '''``mod16_composite_downscaled_spec`` (include/mod16_hip.h): a composite call's spec, which of its
    15 arrays are series of coarse planes (bit 14: the hours of daylight), their row pitch, and the
    first pixel of the range.'''
    _fields_ = [('composite', CompositeSpec), ('coarse_mask', C.c_uint32), ('reserved_', C.c_uint32),
                ('coarse_pitch', C.c_int64), ('first_pixel', C.c_int64)]


_COMPOSITE_DOWNSCALED_ARGS = [C.c_void_p, C.c_void_p, C.POINTER(CompositeDownscaledSpec), C.c_void_p, _PP, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint, C.c_int, C.c_void_p,
                              C.c_int64]

# name -> (restype, argtypes); one entry per function declared in the header
PROTOTYPES = {
    'mod16_version': (C.c_int, []),
    'mod16_strerror': (C.c_char_p, [C.c_int]),
    'mod16_last_error': (C.c_char_p, [C.c_void_p]),
    'mod16_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'mod16_create': (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    'mod16_destroy': (C.c_int, [C.c_void_p]),
    'mod16_set_bplut_f64': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mod16_et_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, _PP, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, _PP, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et2_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_int, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_int64,
        C.c_void_p, C.c_void_p, _PP, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et2_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_int, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_int64,
        C.c_void_p, C.c_void_p, _PP, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_host_tile_pixels': (C.c_int64, []),
    'mod16_et_hdiag_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_uint, C.c_void_p]),
    'mod16_et_hdiag_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_uint, C.c_void_p]),
    'mod16_fold_diag_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    'mod16_et_pet_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_pet_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_raw_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
        C.c_int, C.c_void_p]),
    'mod16_et_raw_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
        C.c_int, C.c_void_p]),
    'mod16_et_diag_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.c_void_p]),
    'mod16_et_diag_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.c_void_p]),
    'mod16_graph_et_diag_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.POINTER(C.c_void_p)]),
    'mod16_graph_et_diag_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.POINTER(C.c_void_p)]),
    'mod16_graph_launch': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mod16_graph_destroy': (C.c_int, [C.c_void_p]),
    'mod16_method_f64': (C.c_int, [
        C.c_void_p, C.c_int, _PP, _I64P, _PP, _I64P, C.c_int64, _PP, C.c_double,
        C.c_double, C.c_int, C.c_void_p]),
    'mod16_method_f32': (C.c_int, [
        C.c_void_p, C.c_int, _PP, _I64P, _PP, _I64P, C.c_int64, _PP, C.c_float,
        C.c_float, C.c_int, C.c_void_p]),
    'mod16_et_static_f64': (C.c_int, [
        C.c_void_p, _PP, _I64P, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_double, C.c_int, C.c_void_p]),
    'mod16_et_static_f32': (C.c_int, [
        C.c_void_p, _PP, _I64P, _PP, _I64P, _PP, _I64P, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    'mod16_et_static_batch_f64': (C.c_int, [
        C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_static_batch_f32': (C.c_int, [
        C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_int, C.c_void_p]),
    'mod16_static_batch_bind_f64': (C.c_int, [
        C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint, C.c_int,
        C.POINTER(C.c_void_p)]),
    'mod16_static_batch_bind_f32': (C.c_int, [
        C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint, C.c_int,
        C.POINTER(C.c_void_p)]),
    'mod16_static_batch_objective': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'mod16_static_batch_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mod16_static_batch_info': (C.c_int, [C.c_void_p, _I64P, _I64P, _I64P]),
    'mod16_static_batch_time': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    'mod16_static_batch_destroy': (C.c_int, [C.c_void_p]),
    'mod16_static_batch_set_folds': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    'mod16_static_batch_objective_folds': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    'mod16_static_batch_set_annual': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p]),
    'mod16_static_batch_objective_annual': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]),
    'mod16_check_status': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mod16_reduce_diag_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_void_p]),
    'mod16_reduce_diag_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_void_p]),
    'mod16_synth_f64': (C.c_int, [
        C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
        _PP, C.c_void_p]),
    'mod16_synth_f32': (C.c_int, [
        C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
        _PP, C.c_void_p]),
    'mod16_et_tiled_f64': (C.c_int, [
        C.c_void_p, _LAYP, C.c_void_p, _PP, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.c_void_p]),
    'mod16_et_tiled_f32': (C.c_int, [
        C.c_void_p, _LAYP, C.c_void_p, _PP, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.c_void_p]),
    'mod16_graph_et_tiled_f64': (C.c_int, [
        C.c_void_p, _LAYP, C.c_void_p, _PP, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.POINTER(C.c_void_p)]),
    'mod16_graph_et_tiled_f32': (C.c_int, [
        C.c_void_p, _LAYP, C.c_void_p, _PP, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.POINTER(C.c_void_p)]),
    'mod16_synth_tiled_f64': (C.c_int, [
        C.c_void_p, _LAYP, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
        _PP, C.c_void_p]),
    'mod16_synth_tiled_f32': (C.c_int, [
        C.c_void_p, _LAYP, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
        _PP, C.c_void_p]),
    'mod16_form_shape': (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'mod16_et_form_tiled_f64': (C.c_int, [
        C.c_void_p, _LAYP, C.c_int, _PP, _PP, _PP, C.c_double, C.c_int64, C.c_uint, C.c_void_p]),
    'mod16_et_form_tiled_f32': (C.c_int, [
        C.c_void_p, _LAYP, C.c_int, _PP, _PP, _PP, C.c_double, C.c_int64, C.c_uint, C.c_void_p]),
    'mod16_time_et_tiled': (C.c_int, [
        C.c_void_p, C.c_int, _LAYP, C.c_void_p, _PP, C.c_int64, C.c_void_p, C.c_void_p,
        C.c_uint, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    'mod16_time_graph': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    'mod16_host_alloc': (C.c_int, [C.c_int64, C.POINTER(C.c_void_p)]),
    'mod16_host_free': (C.c_int, [C.c_void_p]),
    'mod16_measure_copy': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float)]),
    'mod16_build_id': (C.c_char_p, []),
    'mod16_fold_diag': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'mod16_classify_f64': (C.c_int, [C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                     C.POINTER(C.c_int64), C.c_void_p]),
    'mod16_classify_f32': (C.c_int, [C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                     C.POINTER(C.c_int64), C.c_void_p]),
    'mod16_time_et': (C.c_int, [
        C.c_void_p, C.c_int, C.c_void_p, _PP, _I64P, _PP, _I64P, C.c_int64,
        C.c_void_p, C.c_void_p, _PP, C.c_uint, C.c_void_p, C.c_int, C.c_void_p,
        C.POINTER(C.c_float)]),
    'mod16_sobol_sample_f64': (C.c_int, [
        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
        C.c_int, C.c_void_p]),
    'mod16_sobol_rows_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
        C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'mod16_sobol_analyze_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'mod16_mcmc_create': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    'mod16_mcmc_create_groups': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_void_p)]),
    'mod16_mcmc_run': (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_float)]),
    'mod16_mcmc_read': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _I64P]),
    'mod16_mcmc_destroy': (C.c_int, [C.c_void_p]),
    'mod16_ensemble_create': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    'mod16_ensemble_destroy': (C.c_int, [C.c_void_p]),
    'mod16_et_ensemble_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, _PP, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_ensemble_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, _PP, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_ensemble_members_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
        C.c_uint, C.c_void_p]),
    'mod16_et_ensemble_members_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
        C.c_uint, C.c_void_p]),
    'mod16_et_ensemble_quantiles_f64': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.POINTER(C.c_double), C.c_int, _PP,
        C.c_int64, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_ensemble_quantiles_f32': (C.c_int, [
        C.c_void_p, C.c_void_p, C.c_void_p, _PP, _I64P, C.c_int64, C.POINTER(C.c_double), C.c_int, _PP,
        C.c_int64, C.c_uint, C.c_int, C.c_void_p]),
    'mod16_et_composite_f64': (C.c_int, _COMPOSITE_ARGS),
    'mod16_et_composite_f32': (C.c_int, _COMPOSITE_ARGS),
    'mod16_gapfill_u8': (C.c_int, [C.c_void_p, C.POINTER(GapfillSpec), _PP, C.c_void_p, C.c_void_p, _PP, _PP,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    'mod16_downscale_create': (C.c_int, [C.c_void_p, C.POINTER(DownscaleSpec), C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_void_p)]),
    'mod16_downscale_create_tables': (C.c_int, [C.c_void_p, C.POINTER(DownscaleSpec)] + [C.c_void_p] * 8 +
                                      [C.POINTER(C.c_void_p)]),
    'mod16_downscale_create_rows': (C.c_int, [C.c_void_p, C.POINTER(DownscaleSpec)] + [C.c_void_p] * 3 +
                                    [C.POINTER(C.c_void_p)]),
    'mod16_downscale_create_rows_tables': (C.c_int, [C.c_void_p, C.POINTER(DownscaleSpec)] + [C.c_void_p] * 6 +
                                           [C.POINTER(C.c_void_p)]),
    'mod16_downscale_destroy': (C.c_int, [C.c_void_p]),
    'mod16_et_downscaled_f64': (C.c_int, _DOWNSCALED_ARGS),
    'mod16_et_downscaled_f32': (C.c_int, _DOWNSCALED_ARGS),
    'mod16_downscale_fields_f64': (C.c_int, _DOWNSCALE_FIELDS_ARGS),
    'mod16_downscale_fields_f32': (C.c_int, _DOWNSCALE_FIELDS_ARGS),
    'mod16_zonal_f64': (C.c_int, _ZONAL_ARGS),
    'mod16_zonal_f32': (C.c_int, _ZONAL_ARGS),
    'mod16_zonal_bounds_f64': (C.c_int, _ZONAL_BOUNDS_ARGS),
    'mod16_zonal_bounds_f32': (C.c_int, _ZONAL_BOUNDS_ARGS),
    'mod16_zonal_lds_zones': (C.c_int, []),
    'mod16_zonal_hist_f64': (C.c_int, _ZONAL_HIST_ARGS),
    'mod16_zonal_hist_f32': (C.c_int, _ZONAL_HIST_ARGS),
    'mod16_zonal_select': (C.c_int, _ZONAL_SELECT_ARGS),
    'mod16_zonal_hist_lds_bytes': (C.c_int, []),
    'mod16_et_composite_downscaled_f64': (C.c_int, _COMPOSITE_DOWNSCALED_ARGS),
    'mod16_et_composite_downscaled_f32': (C.c_int, _COMPOSITE_DOWNSCALED_ARGS),
    'mod16_daynight_f64': (C.c_int, _DAYNIGHT_ARGS),
    'mod16_daynight_f32': (C.c_int, _DAYNIGHT_ARGS),
    'mod16_trend_f64': (C.c_int, _TREND_ARGS),
    'mod16_trend_f32': (C.c_int, _TREND_ARGS),
    'mod16_trend_max_steps': (C.c_int, []),
    'mod16_anomaly_f64': (C.c_int, _ANOMALY_ARGS),
    'mod16_anomaly_f32': (C.c_int, _ANOMALY_ARGS),
    'mod16_anomaly_max_window': (C.c_int, []),
    'mod16_upscale_create': (C.c_int, [C.c_void_p, C.POINTER(UpscaleSpec)] + [C.c_void_p] * 5 + [C.POINTER(C.c_void_p)]),
    'mod16_upscale_destroy': (C.c_int, [C.c_void_p]),
    'mod16_upscale_f64': (C.c_int, _UPSCALE_ARGS),
    'mod16_upscale_f32': (C.c_int, _UPSCALE_ARGS),
    'mod16_upscale_classes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_size_t]),
    'mod16_upscale_create_rows': (C.c_int, [C.c_void_p, C.POINTER(UpscaleSpec)] + [C.c_void_p] * 7 + [C.POINTER(C.c_void_p)]),
    'mod16_upscale_sums_f64': (C.c_int, _UPSCALE_SUMS_ARGS),
    'mod16_upscale_sums_f32': (C.c_int, _UPSCALE_SUMS_ARGS),
    'mod16_smooth_u8': (C.c_int, _SMOOTH_ARGS),
    'mod16_smooth_f32': (C.c_int, _SMOOTH_ARGS),
    'mod16_smooth_f64': (C.c_int, _SMOOTH_ARGS),
    'mod16_smooth_max_slabs': (C.c_int, []),
    'mod16_regress_f32': (C.c_int, _REGRESS_ARGS),
    'mod16_regress_f64': (C.c_int, _REGRESS_ARGS),
    'mod16_regress_max_steps': (C.c_int, []),
    'mod16_regress_max_terms': (C.c_int, []),
}

_lib = None


def _preload_torch_hip_runtime():
    '''PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/
    libamdhip64.so, SONAME libamdhip64.so.7). If libmod16hip.so pulled in the
    system copy first and torch were imported later, the process would hold two
    HIP/HSA runtimes and the second one could not open the GPU. Loading torch's
    copy first makes both resolve to the same runtime, in either import order.
    torch itself is not imported here.'''
    import importlib.util
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


def _declare(lib, tolerate_missing):
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # an older experimental build given through MOD16_LIB (tools/kbench.py
            # A/B runs) may predate an entry point; the in-tree library may not
            if tolerate_missing:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    if lib.mod16_version() != ABI_VERSION:
        raise ImportError('libmod16hip ABI version %d, expected %d'
                          % (lib.mod16_version(), ABI_VERSION))
    return lib


def load():
    '''Load libmod16hip.so (once) and declare its prototypes.'''
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            '%s is not built: run `python -c "import __graft_entry__ as g; '
            'g.build()"` (or mod16_amd/csrc/build.py) at the repo root. '
            'mod16_amd has no CPU fallback.' % LIB_PATH)
    _preload_torch_hip_runtime()
    _lib = _declare(C.CDLL(LIB_PATH), 'MOD16_LIB' in os.environ)
    return _lib


_exp_lib = None


def load_experiments():
    '''The experiments build of the library (``libmod16hip_exp.so``: the same sources with
    ``-DMOD16_EXPERIMENTS``), whose contexts read the launch-geometry overrides ``MOD16_NO_DMA``,
    ``MOD16_RUN_SHIFT``, ``MOD16_STATIC_BELOW``, ``MOD16_STREAM_BLOCKS``, ``MOD16_PITCH``,
    ``MOD16_GRID_MULT`` (and the fault injection ``MOD16_POISON_TICKET``) from the environment when they are created. For tests and tools: the
    product never calls this (``Context(device, experiments=True)`` is how a test asks for it).'''
    global _exp_lib
    if _exp_lib is None:
        if not os.path.exists(EXP_LIB_PATH):
            raise ImportError('%s is not built (mod16_amd/csrc/build.py builds it)' % EXP_LIB_PATH)
        load()          # the HIP runtime both resolve to
        _exp_lib = _declare(C.CDLL(EXP_LIB_PATH), False)
    return _exp_lib


def build_id():
    '''Digest of the sources and flags the loaded library was built from (``mod16_build_id``).'''
    return load().mod16_build_id().decode()


def device_count():
    n = C.c_int(0)
    load().mod16_device_count(C.byref(n))
    return n.value


_ARRAY_TYPES = {}


def _array_type(base, n):
    t = _ARRAY_TYPES.get((base, n))
    if t is None:
        t = _ARRAY_TYPES[(base, n)] = base * n
    return t


_F32 = np.dtype(np.float32)


def typed(lib, stem, dtype):
    '''The float32 or the float64 form of an entry point: ``lib.<stem>_f32`` for float32 (a dtype,
    a scalar type or a name), ``lib.<stem>_f64`` for anything else.'''
    return getattr(lib, stem + ('_f32' if dtype == _F32 else '_f64'))


def ptr_array(ptrs):
    '''Python ints / None -> void*[len]'''
    return _array_type(C.c_void_p, len(ptrs))(*ptrs)


def i64_array(vals):
    try:
        return _array_type(C.c_int64, len(vals))(*vals)
    except TypeError:       # numpy integers
        return _array_type(C.c_int64, len(vals))(*[int(v) for v in vals])


class Context:
    '''One device context (``mod16_ctx``): BPLUT, staging tiles, workspace.'''

    def __init__(self, device=0, experiments=False):
        self.lib = load_experiments() if experiments else load()
        self.handle = C.c_void_p()
        self.device = device
        rc = self.lib.mod16_create(int(device), C.byref(self.handle))
        if rc != OK:
            self.handle = C.c_void_p()
            raise Mod16Error(rc, (
                'cannot create a context on device %d: %s -- mod16_amd needs '
                'an MI355X (gfx950); there is no CPU fallback'
                % (device, self.lib.mod16_strerror(rc).decode())))
        self._bplut_key = None

    def close(self):
        if getattr(self, 'handle', None) and self.handle.value:
            self.lib.mod16_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc == OK:
            return
        msg = self.lib.mod16_last_error(self.handle).decode() or \
            self.lib.mod16_strerror(rc).decode()
        if rc == ERR_CLASS_RANGE:
            # what numpy raises for params_dict[key][pft_map] with a code >= 13
            raise IndexError(msg)
        raise Mod16Error(rc, msg)

    def set_bplut(self, table):
        '''table: float64 [13][11], rows = PFT code, columns in
        MOD16.required_parameters order.'''
        table = np.ascontiguousarray(table, np.float64)
        if table.shape != (N_CLASSES, N_PARAMS):
            raise ValueError('BPLUT table must have shape (13, 11), got %r'
                             % (table.shape,))
        key = table.tobytes()
        if key != self._bplut_key:
            self.check(self.lib.mod16_set_bplut_f64(
                self.handle, table.ctypes.data))
            self._bplut_key = key

    def et(self, dtype, cls, drivers, dstride, params, pstride, n, out_day,
           out_night, out_sep, flags=MATH_FAST, where=HOST, stream=None):
        '''Thin wrapper of mod16_et_f64 / mod16_et_f32; every array argument
        is a raw address (int) or None.'''
        fn = typed(self.lib, 'mod16_et', dtype)
        self.check(fn(
            self.handle, cls, ptr_array(drivers), i64_array(dstride),
            ptr_array(params) if params is not None else None,
            i64_array(pstride) if pstride is not None else None,
            int(n), out_day, out_night,
            ptr_array(out_sep) if out_sep is not None else None,
            int(flags), int(where), stream))

    def et2(self, dtype, cls, cls_kind, drivers, dkind, params, pkind, inner, n,
            out_day, out_night, out_sep, flags=MATH_FAST, where=HOST, stream=None):
        '''mod16_et2_f64 / mod16_et2_f32: as ``et`` with a broadcast kind
        (``BC_*``) per input instead of a 0 / 1 stride.'''
        fn = typed(self.lib, 'mod16_et2', dtype)
        self.check(fn(
            self.handle, cls, int(cls_kind), ptr_array(drivers), i64_array(dkind),
            ptr_array(params) if params is not None else None,
            i64_array(pkind) if pkind is not None else None,
            int(inner), int(n), out_day, out_night,
            ptr_array(out_sep) if out_sep is not None else None,
            int(flags), int(where), stream))

    def method(self, dtype, method, inputs, istride, params, pstride, n, outs,
               alpha=1.26, tiny=1e-7, where=HOST, stream=None):
        '''Thin wrapper of mod16_method_f64 / _f32 (raw addresses or None).'''
        fn = typed(self.lib, 'mod16_method', dtype)
        self.check(fn(
            self.handle, int(method), ptr_array(inputs), i64_array(istride),
            ptr_array(params) if params is not None else None,
            i64_array(pstride) if pstride is not None else None,
            int(n), ptr_array(outs), float(alpha), float(tiny), int(where), stream))

    def check_status(self, stream=None):
        self.check(self.lib.mod16_check_status(self.handle, stream))

    def composite(self, dtype, n, days, period_days, cls, arrays, pixel_stride, time_stride, every,
                  out_et, out_pet, count_et, count_pet, out_pitch, min_valid=1, rescale=False,
                  flags=MATH_FAST, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_et_composite_f64 / _f32. ``arrays``, ``pixel_stride``, ``time_stride``
        and ``every`` have 15 entries: the 14 drivers, then the hours of daylight. Every array argument
        is a raw address (int) or None; ``stage_bytes`` None: the library's default.'''
        spec = CompositeSpec()
        fill_composite_spec(spec, n, days, period_days, pixel_stride, time_stride, every, min_valid, rescale)
        fn = typed(self.lib, 'mod16_et_composite', dtype)
        self.check(fn(self.handle, C.byref(spec), cls, ptr_array(list(arrays[:N_DRIVERS])), arrays[N_DRIVERS],
                      out_et, out_pet, count_et, count_pet, int(out_pitch), int(flags), int(where), stream,
                      0 if stage_bytes is None else int(stage_bytes)))

    def gapfill(self, out_type, n, slabs, fields, qc, good, fallback, out, source, in_pitch, qc_pitch,
                out_pitch, source_pitch, max_gap=-1, scale=(1.0, 1.0, 1.0), where=HOST, stream=None,
                stage_bytes=None):
        '''Thin wrapper of mod16_gapfill_u8. ``fields`` and ``out`` hold one raw address per field,
        ``fallback`` one address or None per field (or is None); ``qc``, ``good`` (256 bytes) and
        ``source`` are raw addresses or None; pitches in elements; ``max_gap`` -1: none;
        ``stage_bytes`` None: the library's default.'''
        spec = GapfillSpec()
        spec.n, spec.slabs, spec.nfields = int(n), int(slabs), len(fields)
        spec.out_type, spec.max_gap = int(out_type), int(max_gap)
        for f in range(min(len(fields), 3)):
            spec.scale[f] = float(scale[f])
        spec.in_pitch, spec.qc_pitch = int(in_pitch), int(qc_pitch)
        spec.out_pitch, spec.source_pitch = int(out_pitch), int(source_pitch)
        self.check(self.lib.mod16_gapfill_u8(
            self.handle, C.byref(spec), ptr_array(list(fields)), qc, good,
            ptr_array(list(fallback)) if fallback is not None else None, ptr_array(list(out)), source,
            int(where), stream, 0 if stage_bytes is None else int(stage_bytes)))

    def smooth(self, in_dtype, out_type, n, slabs, values, weights, qc_weight, out, count, in_pitch, weight_pitch,
               out_pitch, lam, order=2, envelope=0, min_valid=3, weight_mode=SMOOTH_WEIGHT_NONE, scale=1.0,
               where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_smooth_u8 / _f32 / _f64 (``in_dtype``: the type of ``values``).
        ``values`` and ``out`` are raw addresses; ``weights`` (a float32 stack or a uint8 QC layer, as
        ``weight_mode`` says), ``qc_weight`` (256 float64) and ``count`` (uint16) are raw addresses or
        None; pitches in elements; ``stage_bytes`` None: the library's default.'''
        spec = SmoothSpec()
        spec.n, spec.slabs, spec.order, spec.envelope = int(n), int(slabs), int(order), int(envelope)
        spec.min_valid, spec.weight_mode, spec.out_type = int(min_valid), int(weight_mode), int(out_type)
        spec.lam, spec.scale = float(lam), float(scale)
        spec.in_pitch, spec.weight_pitch, spec.out_pitch = int(in_pitch), int(weight_pitch), int(out_pitch)
        fn = getattr(self.lib, 'mod16_smooth_' + {'uint8': 'u8', 'float32': 'f32', 'float64': 'f64'}[np.dtype(in_dtype).name])
        self.check(fn(self.handle, C.byref(spec), values, weights, qc_weight, out, count, int(where), stream,
                      0 if stage_bytes is None else int(stage_bytes)))

    def regress(self, dtype, n, steps, values, design, ks, terms, weights, coef, se, rss, tss, r2, count, series,
                value_pitch=None, term_pitch=None, weight_pitch=None, coef_pitch=None, se_pitch=None,
                series_pitch=None, min_valid=None, series_mode=REGRESS_SERIES_NONE, where=HOST, stream=None,
                stage_bytes=None):
        '''Thin wrapper of mod16_regress_f32 / _f64 (``dtype``: the type of ``values``, of the terms and
        of ``series``). ``values`` and ``coef`` are raw addresses; ``design`` (``steps x ks`` float64),
        ``weights`` (float32), ``se``, ``rss``, ``tss``, ``r2``, ``count`` (uint16) and ``series`` raw
        addresses or None; ``terms`` a sequence of raw addresses; pitches in elements (None: ``n``);
        ``min_valid`` None: ``ks + len(terms) + 1``; ``stage_bytes`` None: the library's default.'''
        terms = list(terms)
        spec = RegressSpec()
        spec.n, spec.steps, spec.ks, spec.kp = int(n), int(steps), int(ks), len(terms)
        spec.min_valid = int(ks) + len(terms) + 1 if min_valid is None else int(min_valid)
        spec.series, spec.flags = int(series_mode), 0
        for name, pitch in (('value_pitch', value_pitch), ('term_pitch', term_pitch), ('weight_pitch', weight_pitch),
                            ('coef_pitch', coef_pitch), ('se_pitch', se_pitch), ('series_pitch', series_pitch)):
            setattr(spec, name, int(n if pitch is None else pitch))
        fn = typed(self.lib, 'mod16_regress', dtype)
        self.check(fn(self.handle, C.byref(spec), values, design, ptr_array(terms) if terms else None, weights, coef, se,
                      rss, tss, r2, count, series, int(where), stream, 0 if stage_bytes is None else int(stage_bytes)))

    def daynight(self, dtype, out_type, rows, cols, days, steps_per_day, fields, tables, out, temp_annual, in_pitch,
                 in_plane, out_pitch, out_plane, mode=DAYNIGHT_SOLAR, threshold=0.0, where=HOST, stream=None,
                 stage_bytes=None):
        '''Thin wrapper of mod16_daynight_f64 / _f32 (``dtype``: the fields' type). ``fields`` holds five
        raw addresses or None (t, qv, ps, sw, lw), ``out`` ten (``daynight.OUTPUT_NAMES``), ``temp_annual``
        one; ``tables`` is None or three contiguous float64 numpy arrays (half_day, noon, offset: host
        memory in both modes); pitches and plane strides in elements; ``stage_bytes`` None: the
        library's default.'''
        spec = DaynightSpec()
        spec.rows, spec.cols, spec.days, spec.steps_per_day = int(rows), int(cols), int(days), int(steps_per_day)
        spec.mode, spec.out_type, spec.threshold = int(mode), int(out_type), float(threshold)
        spec.in_pitch, spec.in_plane = int(in_pitch), int(in_plane)
        spec.out_pitch, spec.out_plane = int(out_pitch), int(out_plane)
        half, noon, offset = tables if tables is not None else (None, None, None)
        fn = typed(self.lib, 'mod16_daynight', dtype)
        self.check(fn(self.handle, C.byref(spec), ptr_array(list(fields)),
                      None if half is None else half.ctypes.data, None if noon is None else noon.ctypes.data,
                      None if offset is None else offset.ctypes.data, ptr_array(list(out)), temp_annual,
                      int(where), stream, 0 if stage_bytes is None else int(stage_bytes)))

    def trend(self, dtype, n, steps, values, times, out, s, count, time_stride=None, min_valid=4, zq=0.0,
              where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_trend_f64 / _f32 (``dtype``: the values' type). ``values``, ``s`` and
        ``count`` are raw addresses (the last two or None), ``out`` holds five or None (slope, intercept,
        slope_lo, slope_hi, z); ``times`` is a contiguous float64 numpy array (host memory in both
        modes); ``time_stride`` in elements (None: ``n``); ``zq`` 0: no interval; ``stage_bytes`` None:
        the library's default.'''
        spec = TrendSpec()
        spec.n, spec.steps, spec.min_valid = int(n), int(steps), int(min_valid)
        spec.time_stride, spec.zq = int(n if time_stride is None else time_stride), float(zq)
        fn = typed(self.lib, 'mod16_trend', dtype)
        self.check(fn(self.handle, C.byref(spec), values, times.ctypes.data, ptr_array(list(out)), s, count,
                      int(where), stream, 0 if stage_bytes is None else int(stage_bytes)))

    def anomaly(self, dtype, n, years, periods, num, den, z, pct, mean, std, count, window=1, base_first=0,
                base_end=None, min_valid=3, in_stride=None, out_stride=None, clim_stride=None, where=HOST,
                stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_anomaly_f64 / _f32 (``dtype``: the type of ``num``, ``den``, ``z`` and
        ``pct``). The seven arrays are raw addresses, every one but ``num`` or None (``den`` None: no
        ratio; an output None: not produced); the strides in elements (None: ``n``); ``base_end``
        None: ``years``; ``stage_bytes`` None: the library's default.'''
        spec = AnomalySpec()
        spec.n, spec.years, spec.periods, spec.window = int(n), int(years), int(periods), int(window)
        spec.base_first, spec.base_end = int(base_first), int(years if base_end is None else base_end)
        spec.min_valid = int(min_valid)
        spec.in_stride = int(n if in_stride is None else in_stride)
        spec.out_stride = int(n if out_stride is None else out_stride)
        spec.clim_stride = int(n if clim_stride is None else clim_stride)
        fn = typed(self.lib, 'mod16_anomaly', dtype)
        self.check(fn(self.handle, C.byref(spec), num, den, z, pct, mean, std, count, int(where), stream,
                      0 if stage_bytes is None else int(stage_bytes)))

    @staticmethod
    def _zonal_geometry(spec, n, layers, nzones, zone_type, weight_kind, cols, first_pixel, value_pitch, **int32):
        '''Fills the eight fields a ``ZonalSpec`` and a ``ZonalHistSpec`` share; ValueError where one of
        their int32 fields, or of the further ones given by name, does not fit.'''
        for what, v in dict(layers=layers, nzones=nzones, zone_type=zone_type, weight_kind=weight_kind, **int32).items():
            if not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError('%s must fit an int32, got %r' % (what, v))
        spec.n, spec.layers, spec.nzones = int(n), int(layers), int(nzones)
        spec.zone_type, spec.weight_kind = int(zone_type), int(weight_kind)
        spec.cols, spec.first_pixel = int(cols), int(first_pixel)
        spec.value_pitch = int(n if value_pitch is None else value_pitch)
        return spec

    @staticmethod
    def _zonal_spec(n, layers, nzones, zone_type, weight_kind, cols, first_pixel, value_pitch, bounds=None):
        spec = Context._zonal_geometry(ZonalSpec(), n, layers, nzones, zone_type, weight_kind, cols, first_pixel, value_pitch)
        if bounds is not None:
            spec.wmax, spec.xmax, spec.ew, spec.ex = float(bounds[0]), float(bounds[1]), int(bounds[2]), int(bounds[3])
        return spec

    def zonal(self, dtype, n, layers, nzones, zone_type, values, zones, weights, acc, bounds, weight_kind=0,
              cols=1, first_pixel=0, value_pitch=None, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_zonal_f64 / _f32. ``values``, ``zones``, ``weights`` (or None) and
        ``acc`` are raw addresses; ``bounds`` is ``(wmax, xmax, ew, ex)`` (``zonal.check_bounds``);
        ``value_pitch`` None: ``n``; ``stage_bytes`` None: the library's default.'''
        spec = self._zonal_spec(n, layers, nzones, zone_type, weight_kind, cols, first_pixel, value_pitch, bounds)
        fn = typed(self.lib, 'mod16_zonal', dtype)
        self.check(fn(self.handle, C.byref(spec), values, zones, weights, acc, int(where), stream,
                      0 if stage_bytes is None else int(stage_bytes)))

    @staticmethod
    def zonal_hist_spec(dtype, n, layers, nzones, zone_type=0, weight_kind=0, cols=1, first_pixel=0, value_pitch=None,
                        wmax=1.0, ew=31, bins=None, lo=0.0, hi=0.0, scale=0.0, bits=0, level=0, slots=1):
        '''A ``mod16_zonal_hist_spec``: uniform mode where ``bins`` is given, else digit mode.'''
        spec = Context._zonal_geometry(ZonalHistSpec(), n, layers, nzones, zone_type, weight_kind, cols, first_pixel, value_pitch,
                                       ew=ew, bins=bins or 0, bits=bits, level=level, slots=slots)
        spec.ew, spec.wmax = int(ew), float(wmax)
        spec.width = 8 * np.dtype(dtype).itemsize
        if bins is not None:
            spec.mode, spec.bins, spec.lo, spec.hi, spec.scale = ZONAL_HIST_UNIFORM, int(bins), float(lo), float(hi), float(scale)
        else:
            spec.mode, spec.bits, spec.level, spec.slots = ZONAL_HIST_DIGIT, int(bits), int(level), int(slots)
        return spec

    def zonal_hist(self, spec, dtype, values, zones, weights, prefix, hist, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_zonal_hist_f64 / _f32 (raw addresses; ``spec`` from ``zonal_hist_spec``):
        ADDS the uniform histogram, or one level's digit histogram, into ``hist``.'''
        fn = typed(self.lib, 'mod16_zonal_hist', dtype)
        self.check(fn(self.handle, C.byref(spec), values, zones, weights, prefix, hist, int(where), stream,
                      0 if stage_bytes is None else int(stage_bytes)))

    def zonal_select(self, spec, hist, remaining, prefix, out_values=None, weight=None, q=None, where=HOST, stream=None):
        '''Thin wrapper of mod16_zonal_select (raw addresses): closes level ``spec.level``; ``q`` (level 0):
        the quantiles as ``(M, E)`` pairs (``zonalq.rational``).'''
        mant = exp = None
        if q is not None:
            mant = (C.c_int64 * len(q))(*[m for m, _ in q])
            exp = (C.c_int32 * len(q))(*[e for _, e in q])
        self.check(self.lib.mod16_zonal_select(self.handle, C.byref(spec), hist, mant, exp, remaining, prefix, out_values,
                                               weight, int(where), stream))

    def zonal_bounds(self, dtype, n, layers, values, weights, weight_kind=0, cols=1, first_pixel=0,
                     value_pitch=None, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_zonal_bounds_f64 / _f32 (raw addresses): ``(wmax, xmax)``, the
        largest finite weight >= 0 (1.0 without weights) and the largest finite ``|x|`` of a call's
        inputs; synchronous.'''
        spec = self._zonal_spec(n, layers, 1, 0, weight_kind, cols, first_pixel, value_pitch)
        fn = typed(self.lib, 'mod16_zonal_bounds', dtype)
        wmax, xmax = C.c_double(0.0), C.c_double(0.0)
        self.check(fn(self.handle, C.byref(spec), values, weights, C.byref(wmax), C.byref(xmax), int(where), stream,
                      0 if stage_bytes is None else int(stage_bytes)))
        return wmax.value, xmax.value


def fill_composite_spec(spec, n, days, period_days, pixel_stride, time_stride, every, min_valid, rescale):
    '''Fills a ``CompositeSpec``; ``pixel_stride``, ``time_stride`` and ``every`` have 15 entries: the 14
    drivers, then the hours of daylight.'''
    for v in list(every) + [days, period_days, min_valid]:
        if not 0 <= int(v) < 2 ** 31:
            raise ValueError('days, period_days, min_valid and every must fit an int32, got %r' % (v,))
    spec.n, spec.days, spec.period_days = int(n), int(days), int(period_days)
    spec.min_valid, spec.rescale = int(min_valid), 1 if rescale else 0
    for k in range(N_DRIVERS):
        spec.pixel_stride[k] = int(pixel_stride[k])
        spec.time_stride[k] = int(time_stride[k])
        spec.every[k] = int(every[k])
    spec.hours_pixel_stride = int(pixel_stride[N_DRIVERS])
    spec.hours_time_stride = int(time_stride[N_DRIVERS])
    spec.hours_every = int(every[N_DRIVERS])


def zonal_lds_zones():
    '''``mod16_zonal_lds_zones()``: the zone count up to which a block accumulates in LDS.'''
    return int(load().mod16_zonal_lds_zones())


def zonal_hist_lds_bytes():
    '''``mod16_zonal_hist_lds_bytes()``: the bytes of a layer's table up to which a block fills it in LDS.'''
    return int(load().mod16_zonal_hist_lds_bytes())


class Ensemble:
    '''D parameter tables on a context's device (``mod16_ensemble``): the members of an ensemble
    forward run (``mod16_et_ensemble_*``). ``tables``: float64 (D, 13, 11), each as ``set_bplut`` takes.'''

    def __init__(self, ctx, tables):
        tables = np.ascontiguousarray(tables, np.float64)
        if tables.ndim != 3 or tables.shape[1:] != (N_CLASSES, N_PARAMS):
            raise ValueError('ensemble tables must have shape (members, 13, 11), got %r' % (tables.shape,))
        self.ctx = ctx                  # keeps the context alive as long as its ensemble
        self.handle = C.c_void_p()
        self.members = int(tables.shape[0])
        ctx.check(ctx.lib.mod16_ensemble_create(ctx.handle, tables.ctypes.data, self.members,
                                                C.byref(self.handle)))

    def run(self, dtype, cls, drivers, dstride, n, outs, flags=MATH_FAST, where=HOST, stream=None):
        '''Thin wrapper of mod16_et_ensemble_f64 / _f32; every array argument is a raw address.'''
        if not self.handle.value:
            raise ValueError('the ensemble has been closed')
        fn = typed(self.ctx.lib, 'mod16_et_ensemble', dtype)
        self.ctx.check(fn(self.ctx.handle, self.handle, cls, ptr_array(drivers), i64_array(dstride),
                          int(n), ptr_array(outs), int(flags), int(where), stream))

    def run_members(self, dtype, cls, drivers, dstride, n, day, night, pitch, flags=MATH_FAST, stream=None):
        '''Thin wrapper of mod16_et_ensemble_members_f64 / _f32 (device addresses).'''
        if not self.handle.value:
            raise ValueError('the ensemble has been closed')
        fn = typed(self.ctx.lib, 'mod16_et_ensemble_members', dtype)
        self.ctx.check(fn(self.ctx.handle, self.handle, cls, ptr_array(drivers), i64_array(dstride),
                          int(n), day, night, int(pitch), int(flags), stream))

    def quantiles(self, dtype, cls, drivers, dstride, n, q, outs, slab_bytes=None, flags=MATH_FAST,
                  where=HOST, stream=None):
        '''Thin wrapper of mod16_et_ensemble_quantiles_f64 / _f32: ``q`` a sequence of floats,
        ``outs`` the 3 * len(q) addresses, series-major (day, night, total); ``slab_bytes`` None: the
        library's default.'''
        if not self.handle.value:
            raise ValueError('the ensemble has been closed')
        fn = typed(self.ctx.lib, 'mod16_et_ensemble_quantiles', dtype)
        qs = _array_type(C.c_double, len(q))(*[float(v) for v in q])
        self.ctx.check(fn(self.ctx.handle, self.handle, cls, ptr_array(drivers), i64_array(dstride),
                          int(n), qs, len(q), ptr_array(outs), 0 if slab_bytes is None else int(slab_bytes),
                          int(flags), int(where), stream))

    def close(self):
        if getattr(self, 'handle', None) and self.handle.value:
            self.ctx.lib.mod16_ensemble_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Downscale:
    '''The geometry of a fine raster over a coarse grid on a context's device (``mod16_downscale``):
    the corner tables of ``mod16_amd.downscale.corner_tables`` for both axes, computed here in numpy
    and handed to ``mod16_downscale_create_tables``, so that the device's interpolation carries the
    bits of the numpy definition. With ``col_affine = (col_origin, col_scale)`` in place of ``col_pos``
    (row-affine columns: ``mod16_amd.downscale.corner_tables_rows``) the rows keep their numpy tables,
    ``col_tables`` is None and the handle comes from ``mod16_downscale_create_rows_tables``.'''

    def __init__(self, ctx, shape, coarse_shape, row_pos, col_pos=None, wrap=False, method='bilinear', tables=None,
                 col_affine=None):
        from . import downscale as _d
        if (col_pos is None) == (col_affine is None):
            raise ValueError('exactly one of col_pos and col_affine must be given')
        _d.check_call(shape, coarse_shape, [()] * N_DRIVERS, coarse=(), method=method, row_pos=row_pos,
                      col_pos=col_pos)
        self.shape = (int(shape[0]), int(shape[1]))
        self.coarse_shape = (int(coarse_shape[0]), int(coarse_shape[1]))
        self.wrap, self.method = bool(wrap), method
        self.col_affine = None
        if col_affine is not None:      # row-affine columns: the device forms the column pair per pixel
            self.col_affine = _d.check_affine(self.shape, col_affine[0], col_affine[1], method)
        if tables is not None:          # (another context's grid of the same call: computed once)
            self.row_tables, self.col_tables = tables
        else:
            self.row_tables = _d.corner_tables(row_pos, self.coarse_shape[0], False, method)
            self.col_tables = None if col_affine is not None else \
                _d.corner_tables(col_pos, self.coarse_shape[1], self.wrap, method)
        rt = _d.check_tables(self.row_tables, self.shape[0], self.coarse_shape[0], 'row')
        spec = DownscaleSpec(self.shape[0], self.shape[1], self.coarse_shape[0], self.coarse_shape[1],
                             1 if self.wrap else 0, _d.method_code(method))
        self.ctx = ctx                  # keeps the context alive as long as its grid
        self.handle = C.c_void_p()
        if self.col_affine is not None:
            ctx.check(ctx.lib.mod16_downscale_create_rows_tables(
                ctx.handle, C.byref(spec), *([t.ctypes.data for t in rt] + [t.ctypes.data for t in self.col_affine]),
                C.byref(self.handle)))
            return
        ct = _d.check_tables(self.col_tables, self.shape[1], self.coarse_shape[1], 'column')
        ctx.check(ctx.lib.mod16_downscale_create_tables(
            ctx.handle, C.byref(spec), *([t.ctypes.data for t in rt] + [t.ctypes.data for t in ct]),
            C.byref(self.handle)))

    def _open(self):
        if not self.handle.value:
            raise ValueError('the downscale grid has been closed')

    def run(self, dtype, cls, drivers, kinds, coarse_pitch, first_pixel, n, out_day, out_night,
            flags=MATH_FAST, where=HOST, stream=None):
        '''Thin wrapper of mod16_et_downscaled_f64 / _f32; every array argument is a raw address.'''
        self._open()
        fn = typed(self.ctx.lib, 'mod16_et_downscaled', dtype)
        self.ctx.check(fn(self.ctx.handle, self.handle, cls, ptr_array(drivers),
                          _array_type(C.c_int32, len(kinds))(*[int(k) for k in kinds]), int(coarse_pitch),
                          int(first_pixel), int(n), out_day, out_night, int(flags), int(where), stream))

    def fields(self, dtype, fields, coarse_pitch, first_pixel, n, out, out_pitch, where=HOST, stream=None):
        '''Thin wrapper of mod16_downscale_fields_f64 / _f32 (raw addresses; 1 to 16 fields).'''
        self._open()
        fn = typed(self.ctx.lib, 'mod16_downscale_fields', dtype)
        self.ctx.check(fn(self.ctx.handle, self.handle, ptr_array(list(fields)), len(fields), int(coarse_pitch),
                          int(first_pixel), int(n), out, int(out_pitch), int(where), stream))

    def composite(self, dtype, n, days, period_days, cls, arrays, pixel_stride, time_stride, every, coarse_mask,
                  coarse_pitch, first_pixel, out_et, out_pet, count_et, count_pet, out_pitch, min_valid=1,
                  rescale=False, flags=MATH_FAST, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_et_composite_downscaled_f64 / _f32: the arguments of ``Context.composite``
        (15 entries per list; raw addresses) and the coarse mask (bit k: array k is a series of coarse
        planes), their row pitch and the range's first pixel.'''
        self._open()
        spec = CompositeDownscaledSpec()
        fill_composite_spec(spec.composite, n, days, period_days, pixel_stride, time_stride, every, min_valid, rescale)
        spec.coarse_mask, spec.coarse_pitch, spec.first_pixel = int(coarse_mask), int(coarse_pitch), int(first_pixel)
        fn = typed(self.ctx.lib, 'mod16_et_composite_downscaled', dtype)
        self.ctx.check(fn(self.ctx.handle, self.handle, C.byref(spec), cls, ptr_array(list(arrays[:N_DRIVERS])),
                          arrays[N_DRIVERS], out_et, out_pet, count_et, count_pet, int(out_pitch), int(flags),
                          int(where), stream, 0 if stage_bytes is None else int(stage_bytes)))

    def close(self):
        if getattr(self, 'handle', None) and self.handle.value:
            self.ctx.lib.mod16_downscale_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Upscale:
    '''The runs of a coarse grid's cells in a fine raster on a context's device (``mod16_upscale``): the
    four tables of ``mod16_amd.upscale.cell_runs`` for both axes, computed here in numpy from the
    positions (or given as ``runs = (row_runs, col_runs)``), and the area weights of the fine rows. With
    ``col_affine = (col_origin, col_scale)`` and ``col_pos=None`` (row-affine columns, a sinusoidal tile:
    ``mod16_upscale_create_rows``) the rows keep their runs, ``col_runs`` is None and the device finds the
    column runs per fine row; ``col_range = (col_first, col_count)`` names the columns that can belong to a
    cell (``runs`` is then the row runs alone).'''

    def __init__(self, ctx, shape, coarse_shape, row_pos=None, col_pos=None, wrap=False, area=None, runs=None,
                 col_affine=None, col_range=None):
        from . import upscale as _u
        self.wrap = bool(wrap)
        self.col_affine = self.col_range = None
        if col_affine is not None and col_pos is None:
            if runs is None:
                self.shape, self.coarse_shape, self.row_runs, self.col_affine, self.col_range = _u.check_geometry_rows(
                    shape, coarse_shape, row_pos, col_affine, self.wrap, col_range)
            else:
                self.shape, self.coarse_shape = (int(shape[0]), int(shape[1])), (int(coarse_shape[0]), int(coarse_shape[1]))
                self.row_runs = _u.check_runs(runs, self.shape[0], self.coarse_shape[0], 'row')
                self.col_affine, self.col_range = _u.check_rows(self.shape, self.coarse_shape[1], col_affine, self.wrap, col_range)
                _u.check_cell_size(self.row_runs, self.col_range)
            self.col_runs = None
        elif col_range is not None:
            raise ValueError('col_range goes with col_affine (row-affine columns)')
        elif runs is None:
            self.shape, self.coarse_shape, self.row_runs, self.col_runs = _u.check_geometry(
                shape, coarse_shape, row_pos, col_pos, self.wrap, col_affine)
        else:
            self.shape, self.coarse_shape = (int(shape[0]), int(shape[1])), (int(coarse_shape[0]), int(coarse_shape[1]))
            self.row_runs = _u.check_runs(runs[0], self.shape[0], self.coarse_shape[0], 'row')
            self.col_runs = _u.check_runs(runs[1], self.shape[1], self.coarse_shape[1], 'column', self.wrap)
            _u.check_cell_size(self.row_runs, self.col_runs)
        self.area = _u.check_area(area, self.shape[0])
        spec = UpscaleSpec(self.shape[0], self.shape[1], self.coarse_shape[0], self.coarse_shape[1], 1 if self.wrap else 0, 0)
        self.ctx = ctx                  # keeps the context alive as long as its grid
        self.handle = C.c_void_p()
        area_ptr = None if self.area is None else self.area.ctypes.data
        if self.col_affine is not None:
            whole = col_range is None    # (the library takes NULL for "every column")
            ctx.check(ctx.lib.mod16_upscale_create_rows(
                ctx.handle, C.byref(spec), self.row_runs[0].ctypes.data, self.row_runs[1].ctypes.data,
                self.col_affine[0].ctypes.data, self.col_affine[1].ctypes.data,
                None if whole else self.col_range[0].ctypes.data, None if whole else self.col_range[1].ctypes.data,
                area_ptr, C.byref(self.handle)))
        else:
            ctx.check(ctx.lib.mod16_upscale_create(
                ctx.handle, C.byref(spec), *([t.ctypes.data for t in tuple(self.row_runs) + tuple(self.col_runs)] + [area_ptr]),
                C.byref(self.handle)))

    def _open(self):
        if not self.handle.value:
            raise ValueError('the upscale grid has been closed')

    def run(self, dtype, values, layers, layer_stride, row_stride, min_fraction, outs, where=HOST, stream=None,
            stage_bytes=None):
        '''Thin wrapper of mod16_upscale_f64 / _f32. ``values`` is a raw address, ``outs`` three entries
        (mean, fraction, count), each None or ``(address, layer stride, row stride)`` in elements.'''
        self._open()
        fn = typed(self.ctx.lib, 'mod16_upscale', dtype)
        flat = []
        for o in outs:
            flat += [None, 0, 0] if o is None else [o[0], int(o[1]), int(o[2])]
        self.ctx.check(fn(self.ctx.handle, self.handle, values, int(layers), int(layer_stride), int(row_stride),
                          float(min_fraction), *(flat + [int(where), stream, 0 if stage_bytes is None else int(stage_bytes)])))

    def sums(self, dtype, values, layers, layer_stride, row_stride, outs, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_upscale_sums_f64 / _f32. ``values`` is a raw address, ``outs`` four entries
        (num, den, tot, count), each None or ``(address, layer stride, row stride)`` in elements.'''
        self._open()
        fn = typed(self.ctx.lib, 'mod16_upscale_sums', dtype)
        flat = []
        for o in outs:
            flat += [None, 0, 0] if o is None else [o[0], int(o[1]), int(o[2])]
        self.ctx.check(fn(self.ctx.handle, self.handle, values, int(layers), int(layer_stride), int(row_stride),
                          *(flat + [int(where), stream, 0 if stage_bytes is None else int(stage_bytes)])))

    def classes(self, cls, row_stride, valid, out_cls, out_share, where=HOST, stream=None, stage_bytes=None):
        '''Thin wrapper of mod16_upscale_classes: ``cls`` a raw address, ``valid`` the 32-bit mask, the
        outputs None or ``(address, row stride)``.'''
        self._open()
        oc, os_ = out_cls or (None, 0), out_share or (None, 0)
        self.ctx.check(self.ctx.lib.mod16_upscale_classes(
            self.ctx.handle, self.handle, cls, int(row_stride), int(valid), oc[0], int(oc[1]), os_[0], int(os_[1]),
            int(where), stream, 0 if stage_bytes is None else int(stage_bytes)))

    def close(self):
        if getattr(self, 'handle', None) and self.handle.value:
            self.ctx.lib.mod16_upscale_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_ram_bytes():
    try:
        return os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES')
    except (ValueError, OSError, AttributeError):
        return 0


def _default_pinned_live():
    '''Default bound on page-locked result memory of THIS process: a quarter of the host's RAM,
    between 8 and 64 GiB -- divided by the number of processes the launcher put on the node
    (LOCAL_WORLD_SIZE, else WORLD_SIZE: one rank per GPU), so that eight ranks together stay within
    that quarter instead of pinning twice the RAM (never below 1 GiB per rank).'''
    try:
        ranks = max(1, int(os.environ.get('LOCAL_WORLD_SIZE') or os.environ.get('WORLD_SIZE') or 1))
    except ValueError:
        ranks = 1
    whole = min(64 << 30, max(8 << 30, _host_ram_bytes() // 4))
    return max(1 << 30, whole // ranks)


class _PinnedPool(object):
    '''Page-locked host blocks behind the result arrays of the numpy entry points.

    The reference returns fresh arrays; writing 1.5 GB of results into fresh
    pageable memory costs a page fault per 4 KiB (13 GB/s measured) where PCIe
    moves 57 GB/s, so result arrays of ``MIN_BYTES`` or more are numpy views of
    ``hipHostMalloc`` blocks. A block goes back to the pool when its array is
    garbage-collected and is handed out again for the next result of that size
    (a time loop allocates once). Two bounds: at most ``MAX_LIVE`` bytes are
    page-locked in total (default: a quarter of the host's RAM, between 8 and 64 GiB;
    ``MOD16_PINNED_LIVE``) -- beyond that ``empty`` returns plain numpy arrays and says
    so once (``warnings``; ``fallbacks`` counts them) -- and idle blocks are kept up to the
    larger of ``MAX_CACHED`` (1 GiB; ``MOD16_PINNED_CACHE``) and the sizes of the last eight
    results handed out, so the results of one step of a time loop always find their
    blocks again. ``trim()`` frees the idle blocks. Everything else about the arrays is
    ordinary (writeable, C-contiguous, own their memory through ``.base``).

    Locking: ``give`` runs from ``weakref.finalize``, i.e. possibly inside a garbage
    collection triggered while ``take`` / ``trim`` holds the lock on the same thread -- the lock
    is re-entrant, and ``hipHostFree`` (which synchronises the device) is only ever called
    after the lock has been released: a ``give`` that finds its own thread inside the lock leaves
    the blocks it wants freed on ``deferred``, and whoever holds the lock frees them on the way out.'''
    MIN_BYTES = 1 << 20
    MAX_CACHED = int(os.environ.get('MOD16_PINNED_CACHE', 1 << 30))
    MAX_LIVE = int(os.environ.get('MOD16_PINNED_LIVE', _default_pinned_live()))

    def __init__(self):
        import collections
        self.lock = threading.RLock()
        self.free = {}          # nbytes -> [address, ...]
        self.cached = 0         # idle bytes in `free`
        self.live = 0           # bytes allocated (handed out + idle)
        self.recent = collections.deque(maxlen=8)     # sizes of the last results handed out
        self.fallbacks = 0      # results that had to be plain numpy arrays
        self._warned = False
        self.deferred = []      # blocks a re-entrant give() wants freed (by the lock's holder, after release)
        self._inside = threading.local()    # depth of this thread inside `with self.lock`

    def _enter(self):
        self.lock.acquire()
        self._inside.n = getattr(self._inside, 'n', 0) + 1

    def _leave(self, doomed):
        '''Releases the lock; the outermost holder takes the deferred blocks along.'''
        self._inside.n -= 1
        if self._inside.n == 0 and self.deferred:
            doomed.extend(self.deferred)
            del self.deferred[:]
        self.lock.release()

    def _cache_bound(self):
        return min(self.MAX_LIVE, max(self.MAX_CACHED, sum(self.recent)))

    def _free_blocks(self, doomed):
        '''hipHostFree of blocks already taken off the books; called WITHOUT the lock.'''
        for addr in doomed:
            try:
                load().mod16_host_free(addr)
            except Exception:       # interpreter shutdown
                pass

    def _trim_locked(self, want, doomed):
        '''Takes idle blocks worth `want` bytes off the books (largest first) into `doomed`.'''
        for size in sorted(self.free, reverse=True):
            blocks = self.free[size]
            while blocks and want > 0:
                doomed.append(blocks.pop())
                self.cached -= size
                self.live -= size
                want -= size
        return want

    def take(self, nbytes):
        doomed = []
        self._enter()
        try:
            self.recent.append(nbytes)
            blocks = self.free.get(nbytes)
            hit = blocks.pop() if blocks else None
            room = True
            if hit is not None:
                self.cached -= nbytes
            else:
                if self.live + nbytes > self.MAX_LIVE:
                    self._trim_locked(self.live + nbytes - self.MAX_LIVE, doomed)
                    room = self.live + nbytes <= self.MAX_LIVE
                if room:
                    self.live += nbytes
        finally:
            self._leave(doomed)
        self._free_blocks(doomed)
        if hit is not None:
            return hit
        if not room:
            self._over_bound(nbytes)
            return None
        p = C.c_void_p()
        if load().mod16_host_alloc(nbytes, C.byref(p)) != OK or not p.value:
            with self.lock:         # no page-locked memory to be had (no GPU / the host's limit)
                self.live -= nbytes
            return None
        return p.value

    def _over_bound(self, nbytes):
        self.fallbacks += 1
        if not self._warned:
            self._warned = True
            import warnings
            warnings.warn(
                'mod16_amd: a result array of %.3f GB did not fit the page-locked pool (%.3f of %.3f GB '
                'in use; MOD16_PINNED_LIVE raises the bound): it is an ordinary numpy array and its '
                'device-to-host copy runs at the page-fault rate, not the PCIe rate'
                % (nbytes / 1e9, self.live / 1e9, self.MAX_LIVE / 1e9), RuntimeWarning, stacklevel=4)

    def trim(self, keep=0):
        '''Free idle blocks until at most ``keep`` bytes of them remain.'''
        doomed = []
        self._enter()
        try:
            self._trim_locked(self.cached - keep, doomed)
        finally:
            self._leave(doomed)
        self._free_blocks(doomed)

    def give(self, addr, nbytes):
        doomed = []
        reentrant = getattr(self._inside, 'n', 0) > 0      # a finalizer running inside take() / trim() of this thread
        self._enter()
        try:
            if self.cached + nbytes <= self._cache_bound():
                self.free.setdefault(nbytes, []).append(addr)
                self.cached += nbytes
            else:
                self.live -= nbytes
                (self.deferred if reentrant else doomed).append(addr)
        finally:
            self._leave(doomed)
        if doomed:
            self._free_blocks(doomed)

    def empty(self, shape, dtype):
        '''``numpy.empty(shape, dtype)``, page-locked when large enough.'''
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.MIN_BYTES or os.environ.get('MOD16_PINNED_RESULTS') == '0':
            return np.empty(shape, dtype)
        addr = self.take(nbytes)
        if addr is None:
            return np.empty(shape, dtype)
        buf = (C.c_char * nbytes).from_address(addr)
        weakref.finalize(buf, self.give, addr, nbytes)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)


pinned = _PinnedPool()
_local = threading.local()


def context(device=0):
    '''The calling thread's context on ``device`` (created on first use).

    One context per host thread and GPU: the reference's functions are pure and
    may be called from several threads at once; a context
    owns staging slabs (HOST mode: up to ``MOD16_HOST_THREADS`` = 8 of them, ~0.6 GB
    each for float64, allocated on the first numpy call of the thread and freed
    with it -- N threads on the numpy path hold N x 4.7 GB of HBM), streams, a
    BPLUT copy and a workspace, so threads that shared one would take turns (the library serialises calls on a ctx) and
    would see each other's ``set_bplut``. Contexts of finished threads are
    destroyed with the thread's locals.'''
    table = getattr(_local, 'contexts', None)
    if table is None:
        table = _local.contexts = {}
    ctx = table.get(device)
    if ctx is None:
        ctx = table[device] = Context(device)
    return ctx
