"""The HOST mode of mod16_anomaly_f32 / _f64 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/anomaly.cpp) that calls the HOST-mode anomaly with guard bytes around every host
array: n = 37 and 300 pixels, (Y, P, W) = (3, 5, 2) and (33, 2, 1), with and without den, three
stage_bytes (the smallest range of pixels -- 256 and 44 of 300 --, a slab cut from the bytes of a range's
rows, one chunk), dense arrays and arrays whose three strides exceed n, every output and a subset, both
types. Clean = no sanitizer report, every requested output element overwritten, no guard byte and no
element between the rows touched, nothing left allocated; and every argument error of the entry points
is refused with MOD16_ERR_ARG and its "mod16_anomaly: ..." message before an output is touched.

The anomaly kernels have no shadow in the stand-in: their launches are checked for their shapes only,
and what is under the sanitizers here is the plan of the staged copies (all S rows of a range of pixels
for the inputs and for z / pct, P rows of the climatology in three element sizes, absent arrays keeping
their place), the range cut from stage_bytes and the entry point's checks -- not the kernel's own
address arithmetic, which tests/test_gpu_anomaly.py covers on the device with strided arrays at odd
offsets. Sanitizers run on the CPU build only; nothing here is loaded into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_anomaly_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('anomaly', tmp_path)
    for name in ('float32', 'float64'):
        assert 'host_asan_anomaly: %s done' % name in out
    assert 'host_asan_anomaly: refusals done' in out
    assert launched(lines, '14anomaly_kernel')
