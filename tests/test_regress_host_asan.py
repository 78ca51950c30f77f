"""The HOST mode of mod16_regress_f32 / _f64 under AddressSanitizer + UndefinedBehaviorSanitizer: the
library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its own source) linked,
unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone program
(tests/host_asan/regress.cpp) that calls the HOST-mode regression with guard bytes around every host
array: 1237 pixels in tiles of 256, of 512 and in one tile, T = 5 and T = 1 steps, both value types,
(Ks, Kp) = (2, 0), (0, 2) and (1, 3), with and without weights, standard errors and either series
output, every array with a pitch of its own. Clean = no sanitizer report, every output element
overwritten, no guard byte and no padding of a pitched output touched, nothing left allocated (the
context's copy of the design goes with the context); and every argument error -- an output that overlaps
an input or another output among them -- is refused with its "mod16_regress: ..." message before an
output is touched. The stand-in's count of the kernel's launches must be the number of tiles the program
meant to cut: five, three and one per configuration.

The regression kernels have no shadow in the stand-in: their launches are checked for their shapes
only, and what is under the sanitizers here is the plan of the staged copies (up to Kp + 2 input stacks
of T slabs, coefficients and standard errors as P-slab outputs, arrays of three element sizes in
float64-sized places), the tile cut from stage_bytes, the upload of the design, and the entry points'
checks -- not the kernel's own address arithmetic, which tests/test_gpu_regress.py covers on the device
with pitched buffers at odd offsets. Sanitizers run on the CPU build only; nothing here is loaded into
Python."""
from host_asan_harness import launched, run_harness, shape_only


def test_host_mode_regress_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('regress', tmp_path)
    for name in ('float32', 'float64'):
        for steps in (5, 1):
            for ks, kp in ((2, 0), (0, 2), (1, 3)):
                assert 'host_asan_regress: %s, %d steps, %d + %d terms done' % (name, steps, ks, kp) in out
    assert 'host_asan_regress: refusals done' in out
    assert launched(lines, '14regress_kernel') and shape_only(lines, '14regress_kernel')
    # the tiles were cut as meant: 5 + 3 + 1 launches a configuration, none from the refusals
    expected = [int(l.split()[-1]) for l in lines if l.startswith('host_asan_regress: expected launches')]
    counted = [int(l.split()[-1]) for l in lines if l.strip().startswith('launches') and '14regress_kernel' in l]
    assert expected == [12 * 12 * 9] and counted == expected
