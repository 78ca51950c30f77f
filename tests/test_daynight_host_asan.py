"""The HOST mode of mod16_daynight_f32 / _f64 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/daynight.cpp) that calls the HOST-mode aggregation with guard bytes around
every host array: a 7 x 37 grid, D = 5 days of H = 3 steps in chunks of 2 days (ragged), of 1 day and
in one chunk, dense and pitched fields and outputs (row pitch and plane stride of their own), every
output and three of them, both modes, both input and both output types. Clean = no sanitizer report,
every requested output element overwritten, no guard byte and no padding byte touched, nothing left
allocated; and every argument error of the entry points is refused with MOD16_ERR_ARG and its
"mod16_daynight: ..." message before an output is touched.

The day / night kernels have no shadow in the stand-in: their launches are checked for their shapes
only, and what is under the sanitizers here is the plan of the staged copies (whole chunks, planes or
rows, by what is dense), the chunk cut from stage_bytes, the table uploads and the entry point's
checks -- not the kernel's own address arithmetic, which tests/test_gpu_daynight.py covers on the
device with pitched buffers at odd offsets. Sanitizers run on the CPU build only; nothing here is
loaded into Python."""
from host_asan_harness import launched, run_harness


def test_host_mode_daynight_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('daynight', tmp_path)
    for name in ('float32 -> float32', 'float32 -> float64', 'float64 -> float32', 'float64 -> float64'):
        assert 'host_asan_daynight: %s done' % name in out
    assert 'host_asan_daynight: refusals done' in out
    assert launched(lines, '15daynight_kernel')
    assert launched(lines, '22daynight_annual_kernel')
