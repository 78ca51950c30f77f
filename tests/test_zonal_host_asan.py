"""The HOST mode of mod16_zonal_* and mod16_zonal_bounds_* under AddressSanitizer +
UndefinedBehaviorSanitizer: the library's host half (`hipcc --cuda-host-only
-fsanitize=address,undefined`, its own source) linked, unchanged, against the HIP stand-in of
tests/host_asan, and driven by a stand-alone program (tests/host_asan/zonal.cpp) that calls
the HOST-mode zonal reduction and its bounds pre-pass with guard bytes around every host array: 1237
pixels in tiles of 256, of 512 and in one tile, K = 3 layers with a value pitch above n, all three
zone types, all three weight kinds with cols = 67 and first_pixel = 5, float64 and float32. Clean =
no sanitizer report, no guard byte touched, the accumulator back as it went up, nothing left
allocated; and every argument error of the entry points is refused before acc is touched.

The zonal kernels have no shadow in the stand-in: their launches are checked for their shapes only,
and what is under the sanitizers here is the plan of the staged copies (the layers' rows, zone ids of
1, 2 and 4 bytes, the optional weights), the tile cut from stage_bytes, the accumulator's and the
per-row weights' upload and the entry points' checks -- not the kernels' own address arithmetic, which
tests/test_gpu_zonal.py covers on the device with pitched buffers at odd offsets. Sanitizers run on
the CPU build only; nothing here is loaded into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_zonal_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('zonal', tmp_path)
    for name in ('float64', 'float32'):
        assert 'host_asan_zonal: %s done' % name in out
    assert 'host_asan_zonal: refusals done' in out
    assert launched(lines, '12zonal_kernel')
    assert launched(lines, '19zonal_bounds_kernel')
