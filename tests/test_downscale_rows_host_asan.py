"""The row-affine column geometry of the downscaled families on the host, under AddressSanitizer +
UndefinedBehaviorSanitizer: mod16_downscale_create_rows and mod16_downscale_create_rows_tables, and the
HOST mode of mod16_et_downscaled_*, mod16_downscale_fields_* and mod16_et_composite_downscaled_* on a
row-affine handle -- the library's host half (`hipcc --cuda-host-only -fsanitize=address,undefined`, its
own source) linked, unchanged, against the HIP stand-in of tests/host_asan, and driven by a stand-alone
program (tests/host_asan/downscale_rows.cpp) for both data types:

  create     both functions; every refusal (cos4, a non-finite origin, scale or far end -- in the
             LAST row, NULLs, the spec, the row tables) with its text, and the handle left NULL
  run        1237 pixels from pixel 777 of a 60 x 47 raster (starts inside a row, ends ragged), FAST and
             EXACT, col_origin / col_scale in heap blocks of exactly 60 x 8 bytes, guard bytes around
             the outputs
  fields     3 fields over the same range into a pitched output whose padding stays untouched
  composite  11 days in periods of 4 over the same range, with and without the potential-ET outputs,
             in tiles of 512 pixels and in one

Clean = no sanitizer report, every output element overwritten, no guard byte and no padding touched,
nothing left allocated, and the row-affine instances of all five kernels among the stand-in's recorded
launches. The kernels have no shadow in the stand-in: their own arithmetic is covered on the device by
tests/test_gpu_downscale_rows.py. Sanitizers run on the CPU build only, and nothing sanitised is loaded
into Python."""
from host_asan_harness import run_harness


def test_host_mode_row_affine_downscale_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('downscale_rows', tmp_path)
    assert 'host_asan_downscale_rows: create done' in out
    for dtype in ('float64', 'float32'):
        for case in ('run', 'fields', 'composite'):
            assert 'host_asan_downscale_rows: %s %s done' % (dtype, case) in out, (dtype, case)
    # the row-affine instances of the five kernels were launched, for both data types
    shapes = [l for l in lines if l.strip().startswith('launch shape only')]
    for kernel in ('9ds_kernelI%sLb0E', '9ds_kernelI%sLb1E', '14ds_redo_kernelI%s', '16ds_fields_kernelI%s',
                   '9cd_kernelI%sLb0ELb0E', '9cd_kernelI%sLb0ELb1E', '9cd_kernelI%sLb1ELb0E', '9cd_kernelI%sLb1ELb1E',
                   '14cd_redo_kernelI%sLb0E', '14cd_redo_kernelI%sLb1E'):
        for t in 'df':
            assert any((kernel % t) + 'NS_10DsRowsGridE' in l for l in shapes), kernel % t
    assert not any('6DsGridE' in l for l in shapes)          # and no rectilinear one: the handle's geometry picks
