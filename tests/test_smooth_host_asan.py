"""The HOST mode of mod16_smooth_u8 / _f32 / _f64 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/smooth.cpp) that calls the HOST-mode smoother with guard bytes around every host
array: 1237 pixels in tiles of 256, of 512 and in one tile, S = 5 and S = 1 slabs, the three input
types with every output type they allow, no weights, a float32 stack, a QC layer with the default
table and with one of the caller's, with and without the counts, every array with a pitch of its own.
Clean = no sanitizer report, every output element overwritten, no guard byte and no padding of a pitched
output touched, nothing left allocated (the context's workspace of columns goes with the context); and
every argument error -- an output that overlaps an input or another output among them -- is refused with
its "mod16_smooth: ..." message before an output is touched.

The smoothing kernels have no shadow in the stand-in: their launches are checked for their shapes
only, and what is under the sanitizers here is the plan of the staged copies (arrays of four element
sizes in places of the widest), the tile cut from stage_bytes, the workspace and the upload of the
table to its head, and the entry points' checks -- not the kernel's own address arithmetic, which
tests/test_gpu_smooth.py covers on the device with pitched buffers at odd offsets. Sanitizers run on the
CPU build only; nothing here is loaded into Python."""
from host_asan_harness import launched, run_harness, shape_only


def test_host_mode_smooth_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('smooth', tmp_path)
    for name in ('uint8 -> uint8', 'uint8 -> float32', 'uint8 -> float64', 'float32', 'float64'):
        for slabs in (5, 1):
            assert 'host_asan_smooth: %s, %d slabs done' % (name, slabs) in out
    assert 'host_asan_smooth: refusals done' in out
    assert launched(lines, '13smooth_kernel') and shape_only(lines, '13smooth_kernel')
