// Listing aid (tools/kernel_regs.py): every instance of zonal_kernel and zonal_hist_kernel the
// library launches -- float32 and float64, the three zone types, the three weight kinds, both LDS
// table sizes and the global table, both histogram modes -- and nothing else:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o x.s tools/zonal_instances.hip
#include <hip/hip_runtime.h>
#include "../mod16_amd/csrc/mod16_kernels.hpp"
#include "../mod16_amd/csrc/mod16_zonalq.hpp"
namespace mod16 {
#define ZONAL_TABLES(T, ZT, WK)                                                                                 \
    template __global__ void zonal_kernel<T, ZT, WK, kZonalLdsSmall>(ZonalArgs);                                \
    template __global__ void zonal_kernel<T, ZT, WK, kZonalLdsZones>(ZonalArgs);                                \
    template __global__ void zonal_kernel<T, ZT, WK, 0>(ZonalArgs);                                             \
    ZONAL_HIST_TABLES(T, ZT, WK, kZonalqUniform)                                                                \
    ZONAL_HIST_TABLES(T, ZT, WK, kZonalqDigit)
#define ZONAL_HIST_TABLES(T, ZT, WK, MODE)                                                                      \
    template __global__ void zonal_hist_kernel<T, ZT, WK, MODE, kZonalqLdsSmall>(ZonalHistArgs);                \
    template __global__ void zonal_hist_kernel<T, ZT, WK, MODE, kZonalqLdsWords>(ZonalHistArgs);                \
    template __global__ void zonal_hist_kernel<T, ZT, WK, MODE, 0>(ZonalHistArgs);
#define ZONAL_WEIGHTS(T, ZT) \
    ZONAL_TABLES(T, ZT, kZonalWeightNone) ZONAL_TABLES(T, ZT, kZonalWeightRow) ZONAL_TABLES(T, ZT, kZonalWeightPixel)
#define ZONAL_ZONES(T) ZONAL_WEIGHTS(T, uint8_t) ZONAL_WEIGHTS(T, uint16_t) ZONAL_WEIGHTS(T, int32_t)
ZONAL_ZONES(float)
ZONAL_ZONES(double)
}  // namespace mod16
