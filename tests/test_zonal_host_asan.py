"""The HOST mode of mod16_zonal_* and mod16_zonal_bounds_* under AddressSanitizer +
UndefinedBehaviorSanitizer: the library's host half (`hipcc --cuda-host-only
-fsanitize=address,undefined`, its own source) linked, unchanged, against the HIP stand-in of
tests/host_asan, and driven by a stand-alone program (tests/host_asan_zonal/driver.cpp) that calls
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
import os
import subprocess

from conftest import ROOT


def test_host_mode_zonal_is_clean_under_asan_and_ubsan(tmp_path):
    script = os.path.join(ROOT, 'tests', 'host_asan_zonal', 'build_and_run.sh')
    proc = subprocess.run(['bash', script, str(tmp_path)], capture_output=True, text=True, timeout=900)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out[-4000:]
    assert 'host_asan_zonal: ok' in out, out[-2000:]
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error:' not in out and 'LeakSanitizer' not in out, out[-4000:]
    for name in ('float64', 'float32'):
        assert 'host_asan_zonal: %s done' % name in out
    assert 'host_asan_zonal: refusals done' in out
    lines = out.splitlines()
    assert any('12zonal_kernel' in l for l in lines if l.strip().startswith('launches'))
    assert any('19zonal_bounds_kernel' in l for l in lines if l.strip().startswith('launches'))
    report = [l for l in lines if l.startswith('hip_stub:') and 'live allocations' in l]
    assert report and report[-1].rstrip().endswith('live allocations 0'), report
