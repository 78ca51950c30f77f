"""The HOST mode of mod16_et_composite_* under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan_composite/driver.cpp) that calls the HOST-mode composite with guard bytes around
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
import os
import subprocess

from conftest import ROOT


def test_host_mode_composite_is_clean_under_asan_and_ubsan(tmp_path):
    script = os.path.join(ROOT, 'tests', 'host_asan_composite', 'build_and_run.sh')
    proc = subprocess.run(['bash', script, str(tmp_path)], capture_output=True, text=True, timeout=900)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out[-4000:]
    assert 'host_asan_composite: ok' in out, out[-2000:]
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error:' not in out and 'LeakSanitizer' not in out, out[-4000:]
    assert 'host_asan_composite: float64 done' in out and 'host_asan_composite: float32 done' in out
    lines = out.splitlines()
    # both instances and the kernel behind the fast one were launched, for every tile
    for kernel in ('11comp_kernel', '16comp_redo_kernel'):
        assert any(kernel in l for l in lines if l.strip().startswith('launches')), kernel
    report = [l for l in lines if l.startswith('hip_stub:') and 'live allocations' in l]
    assert report and report[-1].rstrip().endswith('live allocations 0'), report
