"""The HOST mode of mod16_et_composite_downscaled_* under AddressSanitizer +
UndefinedBehaviorSanitizer: the library's host half (`hipcc --cuda-host-only
-fsanitize=address,undefined`, its own source) linked, unchanged, against the HIP stand-in of
tests/host_asan, and driven by a stand-alone program
(tests/host_asan/composite_downscale.cpp) for both data types:

  1237 pixels from pixel 777 of a 60 x 47 raster, 11 days in periods of 4: ten reanalysis drivers and
  the hours as coarse series with a row pitch of W + 3 and a time stride of a plane + 5, in heap
  blocks of exactly their size; albedo, fPAR and LAI fine in pitched slabs; a scalar; guard bytes
  around every array; stage_bytes for 5 tiles, 3 tiles and one, with and without the optional
  outputs. Every refusal of the entry point with its text, n = 0, a context without a parameter
  table, and the upload of the coarse series without memory (MOD16_ERR_NOMEM, then a good call).

Clean = no sanitizer report, every output element overwritten, no guard byte and no padding touched,
nothing left allocated, no output touched by a refused call.

The kernels have no shadow in the stand-in: their launches are checked for their shapes only. Their
own address arithmetic is covered on the device by tests/test_gpu_composite_downscale.py (ranges,
pitches, poisoned padding). Sanitizers run on the CPU build only, and nothing sanitised is loaded
into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_composite_downscaled_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('composite_downscale', tmp_path)
    for name in ('no room', 'float64', 'float32'):
        assert 'host_asan_composite_downscale: %s done' % name in out, name
    # both instances and the kernel behind the fast one were launched
    for kernel in ('9cd_kernel', '14cd_redo_kernel'):
        assert launched(lines, kernel), kernel
