// libmod16hip.so -- host side of the C ABI declared in include/mod16_hip.h, as ONE translation
// unit: the entry-point families of capi/ included one after the other (single-command builds:
// kernel variants, tests/host_asan, hipcc -S listings). mod16_amd/csrc/build.py compiles the
// families side by side and links them into the same library.
#include "capi/context.hip"
#include "capi/forward.hip"
#include "capi/methods.hip"
#include "capi/raw.hip"
#include "capi/calibration.hip"
#include "capi/diagnostics.hip"
#include "capi/tiled.hip"
#include "capi/sensitivity.hip"
#include "capi/mcmc.hip"
#include "capi/ensemble.hip"
#include "capi/composite.hip"
#include "capi/gapfill.hip"
#include "capi/downscale.hip"
#include "capi/composite_downscale.hip"
#include "capi/zonal.hip"
#include "capi/zonalq.hip"
#include "capi/daynight.hip"
#include "capi/trend.hip"
#include "capi/anomaly.hip"
#include "capi/upscale.hip"
