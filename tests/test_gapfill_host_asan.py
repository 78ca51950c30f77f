"""The HOST mode of mod16_gapfill_u8 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/gapfill.cpp) that calls the HOST-mode gap filling with guard bytes around
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
from host_asan_harness import launched, run_harness


def test_host_mode_gapfill_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('gapfill', tmp_path)
    for name in ('uint8', 'float32', 'float64'):
        for slabs in (5, 1):
            assert 'host_asan_gapfill: %s, %d slabs done' % (name, slabs) in out
    assert 'host_asan_gapfill: refusals done' in out
    assert launched(lines, '14gapfill_kernel')
