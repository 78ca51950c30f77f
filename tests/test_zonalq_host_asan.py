"""The HOST mode of mod16_zonal_hist_* and of mod16_zonal_select under AddressSanitizer +
UndefinedBehaviorSanitizer: the library's host half (`hipcc --cuda-host-only
-fsanitize=address,undefined`, its own source) linked, unchanged, against the HIP stand-in of
tests/host_asan, and driven by a stand-alone program (tests/host_asan/zonalq.cpp) with guard bytes
around every host array: 1237 pixels in tiles of 256, of 512 and in one tile, K = 3 layers with a
value pitch above n, all three zone types, all three weight kinds with cols = 67 and first_pixel = 5,
the uniform table and the digit table on level 0 and on a level with prefixes, float64 and float32.
The CPU selection loop really runs there: a hand-made table is closed level by level (float32 with 11
bits, float64 with 12: last levels of 10 and 4 bits) and the values are checked. Clean = no sanitizer
report, no guard byte touched, the table back as it went up, nothing left allocated; and every
argument error of the entry points is refused before an output is touched.

The histogram kernels have no shadow in the stand-in: their launches are checked for their shapes
only; tests/test_gpu_zonalq.py covers their address arithmetic on the device. Sanitizers run on the
CPU build only; nothing here is loaded into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_zonal_histograms_and_selection_are_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('zonalq', tmp_path)
    for name in ('float64', 'float32', 'select float32', 'select float64', 'refusals'):
        assert 'host_asan_zonalq: %s done' % name in out
    assert launched(lines, '17zonal_hist_kernel')
    assert not launched(lines, '19zonal_select_kernel')       # HOST mode selects on the CPU
