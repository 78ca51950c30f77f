"""mod16_upscale_create_rows and the HOST mode of mod16_upscale_f32 / _f64 / _classes / _sums_f32 / _sums_f64 on a
rows handle (row-affine columns: sinusoidal tiles) under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked, unchanged,
against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/upscale_rows.cpp) that calls the family with guard bytes around every host array: 37 fine
rows over 5 coarse rows increasing and decreasing, with a margin of rows outside the grid and an empty coarse
row, 70 columns over 9 cells at scales of both signs with and without wrap_cols, column ranges (an empty one
among them) and area, 1 and 3 layers, three stage_bytes (one coarse row of one layer per pass, a band of two
coarse rows, one band), dense arrays and arrays whose row and layer strides exceed the row and the plane,
every output and a subset, both types, the class raster, and the sums of a rectilinear handle. Clean = no
sanitizer report, every requested output element overwritten, no guard byte and no element between the rows
or the layers touched, nothing left allocated; and every argument error of mod16_upscale_create_rows and
the sums is refused with MOD16_ERR_ARG and its message before an output is touched.

The upscale kernels have no shadow in the stand-in: their launches are checked for their shapes only, and
what is under the sanitizers here is the checks and upload of the per-row tables, the band loop with up to
four outputs and the entry points' checks -- not the kernels' own address arithmetic, which
tests/test_gpu_upscale_rows.py covers on the device with strided arrays at odd offsets and guard elements.
Sanitizers run on the CPU build only; nothing here is loaded into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_upscale_rows_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('upscale_rows', tmp_path)
    for name in ('float32', 'float64'):
        assert 'host_asan_upscale_rows: %s done' % name in out
    assert 'host_asan_upscale_rows: refusals done' in out
    for kernel in ('18upscale_ext_kernel', '27upscale_classes_rows_kernel'):
        assert launched(lines, kernel), kernel
