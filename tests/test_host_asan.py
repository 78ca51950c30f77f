"""SURVEY.md section 5 (sanitizers): the HOST half of libmod16hip -- its own source, compiled with
`hipcc --cuda-host-only -fsanitize=address,undefined` -- linked against a stand-in for the HIP
runtime (tests/host_asan/hip_stub.hip: device memory = host heap under AddressSanitizer, kernel
launches = shadows that replay the launch's address arithmetic against the allocation table) and
driven through the C ABI over ragged sizes, every form and layout, bad layouts, the global grid,
2^31 + 12344 pixels, graphs, the HOST-mode tiler, and the calibration family: resident problems
(float64 / float32, FAST / EXACT, HOST / DEVICE) whose workspaces grow under cached graphs, folds,
DE-MCMC-Z samplers with their own workspace and a growing trace, the annual-precipitation constraint
(the site-year-major layout, its objective, rows gathered back, its sampler), the ensemble run, the
Sobol entry points; and every call that builds a handle or grows a workspace once per allocation it
makes, with that allocation failing: the call reports it, frees what it had made and leaves its
object usable. Clean = no sanitizer report, no address outside an allocation, nothing leaked; and a
planted fault (a raster one tile short) is reported. Sanitizers run on the CPU build only (the GPU pool refuses them)."""
from host_asan_harness import launched, run_harness, shape_only


def test_host_half_of_the_library_is_clean_under_asan_and_ubsan(tmp_path):
    out, lines = run_harness('driver', tmp_path)
    assert 'planted fault detected' in out, out[-2000:]
    # the shadows that carry the launch geometry ran, on both data types and on the big rasters
    assert 'et_stream_kernel' in out and 'et_stream_redo_kernel' in out and 'et_kernel' in out
    assert 'graph lifetime: done' in out
    # the kernels of the other HOST-mode families ran under their shadows, not on launch shapes alone
    for kernel in ('13method_kernel', '13et_raw_kernel', '18static_flag_kernel', '13static_kernel'):
        assert launched(lines, kernel), kernel
        assert not shape_only(lines, kernel), kernel
    # the calibration family: every array of the objective's, the rows' and the sampler's launches is
    # checked with the extent its kernel indexes
    for kernel in ('24static_obj_params_kernel', '17static_obj_kernel', '22static_obj_redo_kernel',
                   '21static_obj_any_kernel', '23static_obj_final_kernel', '20static_domain_kernel',
                   '24static_batch_flag_kernel', '19static_batch_kernel', '29static_batch_flag_fast_kernel',
                   '24static_batch_fast_kernel', '32static_batch_flag_skipped_kernel',
                   '29static_batch_redo_rows_kernel', '23static_batch_sse_kernel', '15zero_u32_kernel',
                   '16mcmc_init_kernel', '19mcmc_propose_kernel', '18mcmc_accept_kernel', '23mcmc_init_accept_kernel'):
        assert launched(lines, kernel), kernel
        assert not shape_only(lines, kernel), kernel
    assert 'calibration family: done' in out and 'Sobol entry points: done' in out
    # the constraint's kernels, the gather of its rows and the ensemble's kernels likewise
    for kernel in ('25static_annual_redo_kernel', '26static_annual_final_kernel', '25static_rows_gather_kernel',
                   '10ens_kernel', '15ens_redo_kernel'):
        assert launched(lines, kernel), kernel
        assert not shape_only(lines, kernel), kernel
    assert 'annual: done' in out and 'ensemble: done' in out and 'allocation failures: done' in out
    for what in ('tiled rasters, float64', 'tiled rasters, float32', 'plain device arrays, float64',
                 'HOST mode, float64', 'HOST mode, float32'):
        assert what in out, what
