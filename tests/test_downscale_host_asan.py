"""The HOST mode of mod16_et_downscaled_* and mod16_downscale_fields_*, and the host-side corner
tables of mod16_downscale_create, under AddressSanitizer + UndefinedBehaviorSanitizer: the library's
host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked, unchanged,
against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/downscale.cpp) for both data types:

  small    1237 pixels from pixel 777 of a 60 x 47 raster (not row-aligned): coarse planes with a row
           pitch of W + 3 in heap blocks of exactly their size (the last row ends with its W elements),
           a scalar, fine arrays, guard bytes around the outputs; one tile, real memory
  ragged   2 x 2^21 + 1237 pixels: three staging tiles, the last ragged. A slot's slab is above the
           stand-in's 64 MiB of real memory, so the tile copies are range-checked against the slab
           and skipped; the plan's offsets and the per-tile first pixel are what is checked
  fields   3 fields over 3 000 001 pixels into a pitched output: the tile is cut so that a slab stays
           within 32 MiB -- real copies, ragged tiles, untouched padding

Clean = no sanitizer report, every output element of the real-memory calls overwritten, no guard
byte and no padding touched, nothing left allocated; every argument error refused before an output
is touched; positions of 1e300 and NaN through the table code.

The downscale kernels have no shadow in the stand-in: their launches are checked for their shapes
only. Their own address arithmetic is covered on the device by tests/test_gpu_downscale.py (ranges,
pitches, poisoned padding). Sanitizers run on the CPU build only, and nothing sanitised is loaded
into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_downscale_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('downscale', tmp_path)
    for name in ('create', 'float64 small', 'float64 ragged', 'float64 fields', 'float32 small', 'float32 ragged',
                 'float32 fields'):
        assert 'host_asan_downscale: %s done' % name in out, name
    # both instances, the kernel behind the fast one and the fields kernel were launched
    for kernel in ('9ds_kernel', '14ds_redo_kernel', '16ds_fields_kernel'):
        assert launched(lines, kernel), kernel
