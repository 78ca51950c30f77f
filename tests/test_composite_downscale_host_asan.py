"""The HOST mode of mod16_et_composite_downscaled_* under AddressSanitizer +
UndefinedBehaviorSanitizer: the library's host half (`hipcc --cuda-host-only
-fsanitize=address,undefined`, its own source) linked, unchanged, against the HIP stand-in of
tests/host_asan, and driven by a stand-alone program
(tests/host_asan_composite_downscale/driver.cpp) for both data types:

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
import os
import subprocess

from conftest import ROOT


def test_host_mode_composite_downscaled_is_clean_under_asan_and_ubsan(tmp_path):
    script = os.path.join(ROOT, 'tests', 'host_asan_composite_downscale', 'build_and_run.sh')
    proc = subprocess.run(['bash', script, str(tmp_path)], capture_output=True, text=True, timeout=900)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out[-4000:]
    assert 'host_asan_composite_downscale: ok' in out, out[-2000:]
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error:' not in out and 'LeakSanitizer' not in out, out[-4000:]
    for name in ('no room', 'float64', 'float32'):
        assert 'host_asan_composite_downscale: %s done' % name in out, name
    lines = out.splitlines()
    # both instances and the kernel behind the fast one were launched
    for kernel in ('9cd_kernel', '14cd_redo_kernel'):
        assert any(kernel in l for l in lines if l.strip().startswith('launches')), kernel
    report = [l for l in lines if l.startswith('hip_stub:') and 'live allocations' in l]
    assert report and report[-1].rstrip().endswith('live allocations 0'), report
