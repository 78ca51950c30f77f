"""The HOST mode of mod16_et_composite_* under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/composite.cpp) that calls the HOST-mode composite with guard bytes around
every host array, on sizes that make the tiles ragged (1237 pixels in tiles of 256 and of 512, and
in one tile) and the last period short (11 days in periods of 4), for both data types, with and
without the optional outputs, pitched inputs and outputs. Clean = no sanitizer report, every output
element overwritten, no guard byte and no padding of a pitched output touched, nothing left
allocated; and every argument error is refused before an output is touched.

The composite kernels have no shadow in the stand-in: their launches are checked for their shapes
only, and what is under the sanitizers here is the plan of the staged copies (several rows per
array), the tile cut from stage_bytes and the entry point's checks -- not the kernels' own address
arithmetic, which tests/test_gpu_composite.py covers on the device with pitched and poisoned buffers.
Sanitizers run on the CPU build only."""
from host_asan_harness import launched, run_harness


def test_host_mode_composite_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('composite', tmp_path)
    assert 'host_asan_composite: float64 done' in out and 'host_asan_composite: float32 done' in out
    # both instances and the kernel behind the fast one were launched, for every tile
    for kernel in ('11comp_kernel', '16comp_redo_kernel'):
        assert launched(lines, kernel), kernel
