"""The HOST mode of mod16_gapfill_u8 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan_gapfill/driver.cpp) that calls the HOST-mode gap filling with guard bytes around
every host array, on sizes that make the tiles ragged (1237 pixels in tiles of 256 and of 512, and
in one tile), for S = 5 and S = 1 slabs, one to three fields, all three output types, with and
without the QC layer, the table, the fallbacks and the source bytes, every array with a pitch of its
own. Clean = no sanitizer report, every output element overwritten, no guard byte and no padding of a
pitched output touched, nothing left allocated; and every argument error -- an output that overlaps an
input or another output among them -- is refused before an output is touched.

The gap-filling kernel has no shadow in the stand-in: its launches are checked for their shapes only,
and what is under the sanitizers here is the plan of the staged copies (several rows per byte array
and per output), the tile cut from stage_bytes and the entry point's checks -- not the kernel's own
address arithmetic, which tests/test_gpu_gapfill.py covers on the device with pitched buffers at odd
offsets. Sanitizers run on the CPU build only; nothing here is loaded into Python."""
import os
import subprocess

from conftest import ROOT


def test_host_mode_gapfill_is_clean_under_asan_and_ubsan(tmp_path):
    script = os.path.join(ROOT, 'tests', 'host_asan_gapfill', 'build_and_run.sh')
    proc = subprocess.run(['bash', script, str(tmp_path)], capture_output=True, text=True, timeout=900)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out[-4000:]
    assert 'host_asan_gapfill: ok' in out, out[-2000:]
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error:' not in out and 'LeakSanitizer' not in out, out[-4000:]
    for name in ('uint8', 'float32', 'float64'):
        for slabs in (5, 1):
            assert 'host_asan_gapfill: %s, %d slabs done' % (name, slabs) in out
    assert 'host_asan_gapfill: refusals done' in out
    lines = out.splitlines()
    assert any('14gapfill_kernel' in l for l in lines if l.strip().startswith('launches'))
    report = [l for l in lines if l.startswith('hip_stub:') and 'live allocations' in l]
    assert report and report[-1].rstrip().endswith('live allocations 0'), report
