"""The HOST mode of mod16_trend_f32 / _f64 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/trend.cpp) that calls the HOST-mode trend with guard bytes around every host
array: n = 37 and 300 pixels, Y = 5 and 33 steps, three stage_bytes (the smallest range of pixels -- 256
and 44 of 300 --, a slab cut from the bytes of a range's rows, one chunk), a dense stack and one with
time_stride > n, every output and a subset, both input types. Clean = no sanitizer report, every
requested output element overwritten, no guard byte touched, nothing left allocated; and every
argument error of the entry points is refused with MOD16_ERR_ARG and its "mod16_trend: ..." message
before an output is touched.

The trend kernels have no shadow in the stand-in: their launches are checked for their shapes only,
and what is under the sanitizers here is the plan of the staged copies (all Y rows of a range of
pixels, the outputs of three element sizes), the range cut from stage_bytes, the upload of the times
and the entry point's checks -- not the kernel's own address arithmetic, which tests/test_gpu_trend.py
covers on the device with strided stacks at odd offsets. Sanitizers run on the CPU build only;
nothing here is loaded into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_trend_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('trend', tmp_path)
    for name in ('float32', 'float64'):
        assert 'host_asan_trend: %s done' % name in out
    assert 'host_asan_trend: refusals done' in out
    assert launched(lines, '12trend_kernel')
