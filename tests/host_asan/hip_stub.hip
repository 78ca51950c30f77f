// A stand-in for the HIP runtime under the HOST half of libmod16hip (tests/host_asan): SURVEY.md
// section 5 asks for a sanitizer build of the host shim, and GPU AddressSanitizer is not available on
// the pool, so the library's host code -- mod16_amd/csrc/mod16_capi.hip compiled with
// `hipcc --cuda-host-only -fsanitize=address,undefined` -- is linked against THIS instead of
// libamdhip64: "device" memory is host heap (so every staged copy, memset and workspace is under
// AddressSanitizer), streams / events / graphs are inert handles, and a kernel launch runs the
// kernel's SHADOW: the launch's address arithmetic -- tile / row / pitch offsets of every piece,
// workspace sizes, ticket-ring slots, grid and block shapes -- replayed on the host against the table
// of live allocations, touching nothing. An address range outside every allocation, a misaligned
// vector access, an impossible launch shape or a use of freed memory ends the run with a message.
//
// Allocations above 64 MiB are address-space reservations without memory (PROT_NONE): the shadows
// only compute addresses, so rasters of 43200 x 21600 or 2^31 + 12345 pixels run through the real
// launch geometry in a container without a GPU. Copies and memsets that touch such a range are range-checked
// and skipped.
//
// Compiled as HIP (host only) so that it sees the kernels' own argument structures
// (StreamArgs, EtArgs, SynthArgs, MethodArgs, RawArgs, StaticArgs, StaticBatchArgs, StaticObjArgs,
// StaticAnnualRedoArgs, McmcArgs, EnsArgs: mod16_amd/csrc/*.hpp) instead of copies of them.
//
// Fresh "device" memory is filled with 0xA5. No kernel runs, so that is what the library reads
// back: as a double 0xA5A5A5A5A5A5A5A5 is finite (about -2e-127), which mod16_mcmc_create's check
// of the initial log posterior needs; as a domain mask every byte is set, so a resident problem
// lists every pixel as outside the FAST domain and the redo kernels always launch.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mod16_hip.h"
// (this translation unit's copy of the kernels' declarations lives in a namespace of its own: the
// non-template kernels of the headers would otherwise be defined twice in the linked program)
#define mod16 mod16_shadow
#include "../../mod16_amd/csrc/mod16_kernels.hpp"
#include "../../mod16_amd/csrc/mod16_stream.hpp"
#include "../../mod16_amd/csrc/mod16_methods.hpp"
#include "../../mod16_amd/csrc/mod16_mcmc.hpp"
#include "../../mod16_amd/csrc/mod16_ensemble.hpp"

using namespace mod16;

namespace stub {

constexpr size_t kRealBelow = size_t(64) << 20;

struct Block { size_t size; bool fake; };
// (constructed on first use: the library's module constructor registers its kernels before this
// translation unit's globals would be initialised)
static std::map<uintptr_t, Block>& blocks() { static auto* m = new std::map<uintptr_t, Block>; return *m; }   // base -> block
static std::mutex& mu() { static auto* m = new std::mutex; return *m; }
static std::map<const void*, std::string>& kernels() { static auto* m = new std::map<const void*, std::string>; return *m; }   // host stub -> mangled device name
static std::map<std::string, long>& launches() { static auto* m = new std::map<std::string, long>; return *m; }
static std::map<std::string, long>& unchecked() { static auto* m = new std::map<std::string, long>; return *m; }
#define g_blocks blocks()
#define g_mu mu()
#define g_kernels kernels()
#define g_launches launches()
#define g_unchecked unchecked()
static long g_checked_ranges = 0;
static int g_cus = 256;

[[noreturn]] static void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "hip_stub: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    abort();
}

// [p, p + bytes) must lie inside ONE live allocation
static bool inside(const void* p, size_t bytes, bool* fake = nullptr) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_blocks.upper_bound(a);
    if (it == g_blocks.begin()) return false;
    --it;
    if (a + bytes > it->first + it->second.size) return false;
    if (fake) *fake = it->second.fake;
    return true;
}
static void need(const void* p, size_t bytes, size_t align, const char* what, const char* kernel) {
    ++g_checked_ranges;
    if (bytes == 0) return;
    if (!p) die("%s: %s is NULL", kernel, what);
    if (reinterpret_cast<uintptr_t>(p) % align) die("%s: %s at %p is not %zu-byte aligned", kernel, what, p, align);
    if (!inside(p, bytes)) die("%s: %s [%p, +%zu) lies outside every live device allocation", kernel, what, p, bytes);
}

static void* alloc(size_t bytes) {
    if (bytes == 0) bytes = 1;
    void* p;
    bool fake = bytes >= kRealBelow;
    if (fake) {
        p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) return nullptr;
    } else {
        p = aligned_alloc(256, (bytes + 255) / 256 * 256);      // hipMalloc hands out 256-byte aligned blocks
        if (!p) return nullptr;
        memset(p, 0xA5, bytes);
    }
    std::lock_guard<std::mutex> lock(g_mu);
    g_blocks[reinterpret_cast<uintptr_t>(p)] = Block{bytes, fake};
    return p;
}
static hipError_t release(void* p) {
    if (!p) return hipSuccess;
    Block b;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
        if (it == g_blocks.end()) die("free of %p, which is not the base of a live allocation", p);
        b = it->second;
        g_blocks.erase(it);
    }
    if (b.fake) munmap(p, b.size);
    else free(p);
    return hipSuccess;
}

// ------------------------------------------------------------------ shadows
static int stream_counts(int mode, int* nw, int* nb, int* nout) {
    switch (mode) {
#define C(M) case M: *nw = StreamSpec<M>::NW; *nb = StreamSpec<M>::NB; *nout = StreamSpec<M>::NOUT; return 1;
        C(kStreamPet) C(kStreamSep8) C(kStreamSep6) C(kStreamRaw) C(kStreamRawTotal) C(kStreamRawTotalHours)
        C(kStreamTotals) C(kStreamTotalsMixed) C(kStreamPetMixed) C(kStreamSep8Mixed) C(kStreamSep6Mixed)
        C(kStreamRawMixed) C(kStreamRawTotalMixed) C(kStreamRawTotalHoursMixed)
#undef C
    }
    return 0;
}

// et_stream_kernel<T, MODE, PITCHED, GUARD>: every piece's reads and writes, the workspace, the ticket
template <typename T>
static void shadow_stream(const StreamArgs<T>& a, int mode, bool pitched, dim3 grid, dim3 block, const char* name) {
    constexpr int V = 16 / (int)sizeof(T);
    int NW, NB, NOUT;
    if (!stream_counts(mode, &NW, &NB, &NOUT)) die("%s: unknown mode %d", name, mode);
    if (block.x != (unsigned)kBlock || block.y != 1 || block.z != 1) die("%s: block %u x %u x %u", name, block.x, block.y, block.z);
    if (grid.x < 1 || grid.x > (unsigned)(g_cus * 2) || grid.y != 1) die("%s: grid %u (persistent waves: 1 .. 2 blocks per CU)", name, grid.x);
    if (a.n <= 0 || a.n % V) die("%s: n = %lld is not a positive multiple of the vector width", name, (long long)a.n);
    if (a.run_shift < 0 || a.run_shift > 6) die("%s: run_shift %d", name, a.run_shift);
    if (a.run_shift > a.tile_shift) die("%s: a run of 2^%d pieces straddles tiles of 2^%d", name, a.run_shift, a.tile_shift);
    const int64_t nvec = a.n / V, npiece = (nvec + 63) / 64;
    const int64_t nruns_geom = (npiece + (int64_t(1) << a.run_shift) - 1) >> a.run_shift;
    if (a.static_sched) {
        if (a.nruns != (int64_t)grid.x) die("%s: static schedule with %lld partials for %u blocks", name, (long long)a.nruns, grid.x);
    } else {
        if (a.nruns != nruns_geom) die("%s: %lld partials for %lld runs", name, (long long)a.nruns, (long long)nruns_geom);
        need(a.dyn_counter, 16, 8, "ticket counter", name);
    }
    need(a.lut64, sizeof(double) * MOD16_LUT_ROWS * kLutCols, 8, "BPLUT", name);
    need(a.tab, sizeof(double) * FastMath<double>::kTabDoubles, 16, "exp / log tables", name);
    need(a.status, 4, 4, "status word", name);
    need(a.diag_partial, sizeof(double) * kDiag * (size_t)a.nruns, 8, "diagnostics partials", name);
    // the runs' cancellation lists (mixed-precision forms under the dynamic schedule write them)
    if (!a.static_sched && stream_is_mixed(mode))
        need(a.cancel_list, sizeof(uint16_t) * kCancelCap * (size_t)a.nruns, 2, "cancellation lists", name);
    if (a.diag_out) {
        need(a.diag_out, sizeof(double) * kDiag, 8, "diagnostics vector", name);
        need(a.done_counter, 4, 4, "blocks-done counter", name);
    }
    if (pitched) {
        for (int k = 1; k < NW; ++k)
            if (a.wide[k] != a.wide[0] + k * a.wide_pitch) die("%s: wide[%d] is not wide[0] + %d * pitch", name, k, k);
        // the two steps between successive DMA bases (four LDS slots per value of M0, et_stream_kernel's issue())
        const int64_t pitch_b = a.wide_pitch * (int64_t)sizeof(T);
        if (a.dma_step[0] != pitch_b - 1024 || a.dma_step[1] != pitch_b + 3072)
            die("%s: DMA steps %lld / %lld for a pitch of %lld bytes", name, (long long)a.dma_step[0], (long long)a.dma_step[1], (long long)pitch_b);
    }
    // 32-bit piece numbers and tile rows in the kernel
    if (npiece > kMaxPieces || (uint64_t)a.wide_row >> 32 || (uint64_t)a.out_row >> 32 || (uint64_t)a.byte_row >> 32)
        die("%s: %lld pieces / rows %lld %lld %lld do not fit the kernel's 32-bit scalars", name, (long long)npiece,
            (long long)a.wide_row, (long long)a.out_row, (long long)a.byte_row);
    const bool tiled = a.tile_shift != kNoTile;
    // plain arrays: one check per array; tiled: per tile (pieces of a tile are contiguous)
    const int64_t per_tile = tiled ? (int64_t(1) << a.tile_shift) : npiece;
    for (int64_t p0 = 0; p0 < npiece; p0 += per_tile) {
        const int64_t p1 = std::min(npiece, p0 + per_tile);
        const int64_t tile = tiled ? (p0 >> a.tile_shift) : 0;
        const int64_t first = (p0 - (tiled ? (tile << a.tile_shift) : 0)) * (int64_t)(64 * V);
        const int64_t elems = std::min<int64_t>(a.n - p0 * 64 * V, (p1 - p0) * 64 * V);
        const int64_t ow = tile * a.wide_row + first, oo = tile * a.out_row + first, ob = tile * a.byte_row + first;
        for (int k = 0; k < NW; ++k) need(a.wide[k] + ow, sizeof(T) * elems, 16, "driver array", name);
        for (int k = 0; k < NB; ++k) need(a.bytes[k] + ob, (size_t)elems, V, "byte raster", name);
        for (int k = 0; k < NOUT; ++k) need(a.out[k] + oo, sizeof(T) * elems, 16, "output array", name);
    }
}

template <typename T>
static void shadow_et(const EtArgs<T>& a, dim3 grid, dim3 block, const char* name) {
    if (block.x != (unsigned)kBlock) die("%s: block %u", name, block.x);
    if (grid.x < 1) die("%s: empty grid", name);
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    const int64_t inner = a.inner > 0 ? a.inner : 1;
    auto len = [&](bool dense, bool row, bool col) -> int64_t {
        if (dense) return a.n;
        if (row) return inner;
        if (col) return (a.base + a.n + inner - 1) / inner;
        return 1;
    };
    for (int k = 0; k < 14; ++k)
        need(a.drv[k], sizeof(T) * len((a.dense_drv >> k) & 1u, (a.row_drv >> k) & 1u, (a.col_drv >> k) & 1u), sizeof(T), "driver", name);
    if (a.cls) {
        need(a.cls, (size_t)len(a.cls_mode == MOD16_BC_DENSE, a.cls_mode == MOD16_BC_ROW, a.cls_mode == MOD16_BC_COL), 1, "class raster", name);
        need(a.lut64, sizeof(double) * MOD16_LUT_ROWS * kLutCols, 8, "BPLUT", name);
    } else {
        for (int k = 0; k < 11; ++k)
            need(a.par[k], sizeof(T) * len((a.dense_par >> k) & 1u, (a.row_par >> k) & 1u, (a.col_par >> k) & 1u), sizeof(T), "parameter", name);
    }
    for (int k = 0; k < 10; ++k)
        if (a.out[k]) need(a.out[k], sizeof(T) * a.n, sizeof(T), "output", name);
    need(a.status, 4, 4, "status word", name);
}

template <typename T>
static void shadow_synth(const SynthArgs<T>& a, const char* name) {
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    const int64_t tile = a.tile_shift >= 62 ? a.n : (int64_t(1) << a.tile_shift);
    for (int64_t i = 0; i < a.n; i += tile) {
        const int64_t m = std::min(tile, a.n - i);
        const int64_t e = a.tile_shift >= 62 ? 0 : (i >> a.tile_shift) * a.drv_row;
        const int64_t c = a.tile_shift >= 62 ? 0 : (i >> a.tile_shift) * a.cls_row;
        for (int k = 0; k < 14; ++k) need(a.drv[k] + e, sizeof(T) * m, sizeof(T), "driver array", name);
        need(a.cls + c, (size_t)m, 1, "class raster", name);
    }
}

// a dense array is read or written at [p, p + n), a broadcast scalar at p[0]
template <typename T>
static void need_arr(const T* p, bool dense, int64_t n, const char* what, const char* name) {
    need(p, sizeof(T) * (dense ? (size_t)n : 1), sizeof(T), what, name);
}

// method_kernel<T>: the present inputs, all 11 parameters, the outputs given
template <typename T>
static void shadow_method(const MethodArgs<T>& a, const char* name) {
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    for (int k = 0; k < kMethodMaxIn; ++k)
        if ((a.present_in >> k) & 1u) need_arr(a.in[k], (a.dense_in >> k) & 1u, a.n, "input", name);
    for (int k = 0; k < 11; ++k) need_arr(a.par[k], (a.dense_par >> k) & 1u, a.n, "parameter", name);
    for (int k = 0; k < 2; ++k)
        if (a.out[k]) need_arr(a.out[k], true, a.n, "output", name);
}

// et_raw_kernel<T, FAST>: drivers, the three byte rasters, day_hours (with the 8-day total), outputs, tables
template <typename T>
static void shadow_raw(const RawArgs<T>& a, bool fast, const char* name) {
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, a.n, "driver", name);
    need(a.fpar_pct, (size_t)a.n, 1, "fPAR raster", name);
    need(a.lai_x10, (size_t)a.n, 1, "LAI raster", name);
    need(a.cls, (size_t)a.n, 1, "class raster", name);
    if (a.out[2]) need_arr(a.day_hours, a.dense_hours & 1u, a.n, "day_hours", name);
    for (int k = 0; k < 3; ++k)
        if (a.out[k]) need_arr(a.out[k], true, a.n, "output", name);
    if (fast) {
        need(a.lut64, sizeof(double) * MOD16_LUT_ROWS * kLutCols, 8, "BPLUT", name);
        need(a.tab, sizeof(double) * FastMath<double>::kTabDoubles, 16, "exp / log tables", name);
    } else {
        need(a.lut, sizeof(T) * MOD16_LUT_ROWS * kLutCols, sizeof(T), "BPLUT", name);
    }
    need(a.status, 4, 4, "status word", name);
}

// static_flag_kernel<T> (pixels = false) / static_kernel<T>: drivers, parameters, r_corr if given, the flag word
template <typename T>
static void shadow_static(const StaticArgs<T>& a, bool pixels, const char* name) {
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, a.n, "driver", name);
    for (int k = 0; k < 11; ++k) need_arr(a.par[k], (a.dense_par >> k) & 1u, a.n, "parameter", name);
    if (a.rc[0])
        for (int k = 0; k < (pixels ? 2 : 1); ++k) need_arr(a.rc[k], (a.dense_rc >> k) & 1u, a.n, "r_corr", name);
    need(a.flag, 4, 4, "flag word", name);
    if (pixels)
        for (int k = 0; k < 2; ++k) need_arr(a.out[k], true, a.n, "output", name);
}

// ---- the calibration family (capi/calibration.hip, capi/batch.hpp, capi/mcmc.hip): every extent below
// is what the kernel indexes, in the kernels' own constants
static void need_block(dim3 block, const char* name) {
    if (block.x != (unsigned)kBlock || block.y != 1 || block.z != 1) die("%s: block %u x %u x %u", name, block.x, block.y, block.z);
}
// gridDim chunks of `per` items: they cover `count`, and none of them is empty
static void need_cover(unsigned chunks, int64_t per, int64_t count, const char* what, const char* name) {
    if (count <= 0 || (int64_t)chunks * per < count || ((int64_t)chunks - 1) * per >= count)
        die("%s: %u chunks of %lld for %lld %s", name, chunks, (long long)per, (long long)count, what);
}

// static_obj_params_kernel<T>: params [ndraw][11] -> par16 [ndraw][kPar16]
template <typename T>
static void shadow_obj_params(void** args, dim3 grid, dim3 block, const char* name) {
    const T* params = *static_cast<const T* const*>(args[0]);
    const int64_t ndraw = *static_cast<const int64_t*>(args[1]);
    double* par16 = *static_cast<double* const*>(args[2]);
    need_block(block, name);
    need_cover(grid.x, kBlock, ndraw, "draws", name);
    need(params, sizeof(T) * 11 * (size_t)ndraw, sizeof(T), "params", name);
    need(par16, sizeof(double) * kPar16 * (size_t)ndraw, 8, "par16", name);
}

// static_obj_kernel<T, TR, FOLD>: a thread per pixel, kObjDraws draws per block row
template <typename T>
static void shadow_obj(const StaticObjArgs<T>& a, bool fold, dim3 grid, dim3 block, const char* name) {
    need_block(block, name);
    if ((int64_t)grid.x * kBlock < a.n || a.n <= 0) die("%s: %u blocks for %lld pixels", name, grid.x, (long long)a.n);
    need_cover(grid.y, kObjDraws, a.ndraw, "draws", name);
    const size_t nd = (size_t)a.ndraw;
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, a.n, "driver", name);
    need_arr(a.observed, true, a.n, "observed", name);
    if (a.weights) need_arr(a.weights, true, a.n, "weights", name);
    if (a.skip) need(a.skip, (size_t)a.n, 1, "domain mask", name);
    need(a.par16, sizeof(double) * kPar16 * nd, 8, "par16", name);
    need(a.tab, sizeof(double) * FastMath<double>::kTabDoubles, 16, "exp / log tables", name);
    need(a.any_draw, sizeof(unsigned) * nd, 4, "any_draw", name);
    need(a.partial, sizeof(double) * 2 * nd * grid.x, 16, "partial", name);
    need(a.any_gs, sizeof(unsigned) * nd * grid.x, 4, "any_gs", name);
    if (fold) {
        need(a.code, sizeof(int32_t) * nd, 4, "fold codes", name);
        need(a.label, (size_t)a.n, 1, "fold labels", name);
    }
    // the ANNUAL instances: the scale of every pixel, one mass per wave of 64 pixels and draw
    if (a.scale) need(a.scale, sizeof(double) * (size_t)a.n, 8, "scale", name);
    if (a.mass) need(a.mass, sizeof(double) * nd * grid.x * (kBlock / 64), 8, "mass", name);
}

// where the memory of [p, p + count) is real: its largest entry, every entry checked to be >= 0 (-1: not readable)
static int64_t top_index(const int64_t* p, int64_t count, const char* what, const char* name) {
    bool fake = true;
    if (!inside(p, sizeof(int64_t) * (size_t)count, &fake) || fake) return -1;
    int64_t top = 0;
    for (int64_t u = 0; u < count; ++u) {
        if (p[u] < 0) die("%s: %s[%lld] = %lld", name, what, (long long)u, (long long)p[u]);
        top = std::max(top, p[u]);
    }
    return top;
}

// static_annual_redo_kernel<T>: a block per draw, a thread per site-year over its part of the list
template <typename T>
static void shadow_annual_redo(const StaticAnnualRedoArgs<T>& a, dim3 grid, dim3 block, const char* name) {
    need_block(block, name);
    if (a.G < 1) die("%s: G = %d", name, a.G);
    const size_t nd = grid.x;
    need(a.params, sizeof(T) * 11 * nd, sizeof(T), "params", name);
    need(a.lstart, sizeof(int64_t) * ((size_t)a.G + 1), 8, "lstart", name);
    need(a.rmass, sizeof(double) * 2 * nd * (size_t)a.G, 8, "rmass", name);
    // (the tables are small and real: the site-years' parts of the list are ascending and end where the list ends)
    for (int g = 0; g < a.G; ++g)
        if (a.lstart[g] < 0 || a.lstart[g] > a.lstart[g + 1]) die("%s: lstart[%d] = %lld, [%d] = %lld", name, g, (long long)a.lstart[g], g + 1, (long long)a.lstart[g + 1]);
    const int64_t nlist = a.lstart[a.G];
    if (nlist <= 0) die("%s: %lld listed pixels", name, (long long)nlist);
    need(a.list, sizeof(int64_t) * (size_t)nlist, 8, "pixel list", name);
    const int64_t n = std::max<int64_t>(0, top_index(a.list, nlist, "list", name)) + 1;
    need(a.scale, sizeof(double) * (size_t)n, 8, "scale", name);
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, n, "driver", name);
}

// static_annual_final_kernel(mass, rmass, any_draw, wstart, limit, G, S, ndraw, penalty)
static void shadow_annual_final(void** args, dim3 grid, dim3 block, const char* name) {
    const double* mass = *static_cast<const double* const*>(args[0]);
    const double* rmass = *static_cast<const double* const*>(args[1]);
    const unsigned* any_draw = *static_cast<const unsigned* const*>(args[2]);
    const int32_t* wstart = *static_cast<const int32_t* const*>(args[3]);
    const double* limit = *static_cast<const double* const*>(args[4]);
    const int G = *static_cast<const int*>(args[5]);
    const int64_t ndraw = *static_cast<const int64_t*>(args[7]);
    double* penalty = *static_cast<double* const*>(args[8]);
    need_block(block, name);
    need_cover(grid.x, kObjPerBlock, ndraw, "draws", name);
    if (G < 1) die("%s: G = %d", name, G);
    const size_t nd = (size_t)ndraw;
    need(wstart, sizeof(int32_t) * ((size_t)G + 1), 4, "wstart", name);
    for (int g = 0; g < G; ++g)
        if (wstart[g] < 0 || wstart[g] >= wstart[g + 1]) die("%s: wstart[%d] = %d, [%d] = %d", name, g, wstart[g], g + 1, wstart[g + 1]);
    need(mass, sizeof(double) * nd * (size_t)wstart[G], 8, "mass", name);
    if (rmass) need(rmass, sizeof(double) * 2 * nd * (size_t)G, 8, "rmass", name);
    need(any_draw, sizeof(unsigned) * nd, 4, "any_draw", name);
    need(limit, sizeof(double) * (size_t)G, 8, "limit", name);
    need(penalty, sizeof(double) * nd, 8, "penalty", name);
}

// static_rows_gather_kernel<T>(in [ndraw][n_in], pos [n], n_in, n, ndraw, out [ndraw][n])
static void shadow_rows_gather(void** args, size_t el, dim3 block, const char* name) {
    const void* in = *static_cast<const void* const*>(args[0]);
    const int64_t* pos = *static_cast<const int64_t* const*>(args[1]);
    const int64_t n_in = *static_cast<const int64_t*>(args[2]), n = *static_cast<const int64_t*>(args[3]);
    const int64_t ndraw = *static_cast<const int64_t*>(args[4]);
    need_block(block, name);
    if (n_in <= 0 || n <= 0 || ndraw <= 0) die("%s: n_in %lld, n %lld, ndraw %lld", name, (long long)n_in, (long long)n, (long long)ndraw);
    need(pos, sizeof(int64_t) * (size_t)n, 8, "pos", name);
    if (top_index(pos, n, "pos", name) >= n_in) die("%s: pos points past the %lld resident pixels", name, (long long)n_in);
    need(in, el * (size_t)ndraw * (size_t)n_in, el, "resident rows", name);
    need(*static_cast<void* const*>(args[5]), el * (size_t)ndraw * (size_t)n, el, "gathered rows", name);
}

// ens_kernel<T, FAST> / ens_redo_kernel<T>: drivers, the class raster, the members' tables, the five outputs
template <typename T>
static void shadow_ens(const EnsArgs<T>& a, bool fast, dim3 block, const char* name) {
    need_block(block, name);
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    if (a.members < 1 || a.members > kEnsMaxMembers) die("%s: %d members", name, a.members);
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, a.n, "driver", name);
    need(a.cls, (size_t)a.n, 1, "class raster", name);
    need(a.tables, sizeof(double) * kEnsTable * (size_t)a.members, 8, "members' tables", name);
    if (fast) need(a.tab, sizeof(double) * FastMath<double>::kTabDoubles, 16, "exp / log tables", name);
    for (int k = 0; k < kEnsOut; ++k) need_arr(a.out[k], true, a.n, "output", name);
    need(a.status, 4, 4, "status word", name);
}

// static_obj_redo_kernel<T, FOLD>: a block per draw over the listed pixels
template <typename T>
static void shadow_obj_redo(const StaticObjRedoArgs<T>& a, bool fold, dim3 grid, dim3 block, const char* name) {
    need_block(block, name);
    if (a.nlist <= 0) die("%s: %lld listed pixels", name, (long long)a.nlist);
    const size_t nd = grid.x;
    need(a.params, sizeof(T) * 11 * nd, sizeof(T), "params", name);
    need(a.list, sizeof(int64_t) * (size_t)a.nlist, 8, "pixel list", name);
    need(a.redo, sizeof(double) * 5 * nd, 8, "redo", name);
    // the pixels are known by the list alone: where its memory is real, every entry is an index
    // into observed (and the dense drivers, the weights, the labels)
    bool fake = true;
    int64_t top = 0;
    if (inside(a.list, sizeof(int64_t) * (size_t)a.nlist, &fake) && !fake)
        for (int64_t u = 0; u < a.nlist; ++u) {
            if (a.list[u] < 0) die("%s: list[%lld] = %lld", name, (long long)u, (long long)a.list[u]);
            top = std::max(top, a.list[u]);
        }
    const int64_t n = top + 1;
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, n, "driver", name);
    need_arr(a.observed, true, n, "observed", name);
    if (a.weights) need_arr(a.weights, true, n, "weights", name);
    if (fold) {
        need(a.code, sizeof(int32_t) * nd, 4, "fold codes", name);
        need(a.label, (size_t)n, 1, "fold labels", name);
    }
}

// static_domain_kernel<T> (skip_out set) and the static_batch_* kernels that take a StaticBatchArgs
static std::map<std::string, int64_t>& batch_next() { static auto* m = new std::map<std::string, int64_t>; return *m; }   // kernel -> first draw its next launch must bring
template <typename T>
static void shadow_batch(const StaticBatchArgs<T>& a, const uint8_t* skip_out, bool fast, bool skipped, dim3 grid, dim3 block,
                         const char* name) {
    need_block(block, name);
    if (a.n <= 0) die("%s: n = %lld", name, (long long)a.n);
    for (int k = 0; k < 14; ++k) need_arr(a.drv[k], (a.dense_drv >> k) & 1u, a.n, "driver", name);
    if (skip_out) {     // a thread per pixel, no draws
        if ((int64_t)grid.x * kBlock < a.n || grid.y != 1) die("%s: %u x %u blocks for %lld pixels", name, grid.x, grid.y, (long long)a.n);
        need(skip_out, (size_t)a.n, 1, "domain mask", name);
        return;
    }
    // the launches of one call bring the draws in order, kBatchDraws per block row, all of them
    if (a.draw0 < 0 || a.draw0 >= a.ndraw) die("%s: draw0 %lld of %lld", name, (long long)a.draw0, (long long)a.ndraw);
    if (((int64_t)grid.y - 1) * kBatchDraws >= a.ndraw - a.draw0) die("%s: %u block rows for %lld draws left", name, grid.y, (long long)(a.ndraw - a.draw0));
    {
        std::lock_guard<std::mutex> lock(g_mu);
        int64_t& next = batch_next()[name];
        if (a.draw0 != next) die("%s: draw0 %lld where %lld was due", name, (long long)a.draw0, (long long)next);
        next = a.draw0 + (int64_t)grid.y * kBatchDraws;
        if (next >= a.ndraw) batch_next().erase(name);
    }
    const size_t nd = (size_t)a.ndraw;
    need(a.params, sizeof(T) * 11 * nd, sizeof(T), "params", name);
    for (int k = 0; k < 3; ++k)
        if (a.out[k]) need(a.out[k], sizeof(T) * nd * (size_t)a.n, sizeof(T), "output rows", name);
    need(a.flags, sizeof(unsigned) * nd, 4, "flags", name);
    if (fast) need(a.tab, sizeof(double) * FastMath<double>::kTabDoubles, 16, "exp / log tables", name);
    if (skipped || (fast && a.skip)) need(a.skip, (size_t)a.n, 1, "domain mask", name);
}

// mcmc_init_kernel (x0 set) / mcmc_propose_kernel / mcmc_accept_kernel / mcmc_init_accept_kernel. The
// step counter a.t lives in memory no shadow advances: the history and trace are checked for one step.
static void shadow_mcmc(const McmcArgs& a, const double* x0, bool history, bool trace, dim3 grid, dim3 block, const char* name) {
    need_block(block, name);
    if (a.d < 1 || a.d > kMcmcMaxD) die("%s: d = %d", name, a.d);
    need_cover(grid.x, kBlock, a.chains, "chains", name);
    const size_t c = (size_t)a.chains, cd = c * a.d;
    need(a.y, 8 * cd, 8, "y", name);
    need(a.yp, 8 * cd, 8, "yp", name);
    need(a.xc, 8 * cd, 8, "xc", name);
    need(a.logp, 8 * c, 8, "logp", name);
    need(a.loglik, 8 * c, 8, "loglik", name);
    need(a.lprior_p, 8 * c, 8, "lprior_p", name);
    need(a.scaling, 8 * c, 8, "scaling", name);
    need(a.lamb, 8 * c, 8, "lamb", name);
    need(a.acc, sizeof(int) * c, 4, "acc", name);
    need(a.t, 8 * c, 8, "t", name);
    need(a.key, 8 * c, 8, "key", name);
    need(a.params, 8 * 11 * c, 8, "params", name);
    need(a.sse, 8 * c, 8, "sse", name);
    need(a.cnt, 8 * c, 8, "cnt", name);
    if (x0) need(x0, 8 * cd, 8, "x0", name);
    if (history || trace) need(a.hist, 8 * cd, 8, "history", name);
    if (trace) {
        need(a.xtr, 8 * cd, 8, "x trace", name);
        need(a.tr_ll, 8 * c, 8, "log-likelihood trace", name);
        need(a.tr_lp, 8 * c, 8, "log-posterior trace", name);
        need(a.tr_acc, c, 1, "accepted trace", name);
    }
}

static bool has(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }
// the position behind `key` in a mangled name (its first template argument follows an ...I)
static size_t after(const std::string& s, const char* key) { return s.find(key) + strlen(key); }

static void run_shadow(const std::string& name, dim3 grid, dim3 block, void** args) {
    {
        std::lock_guard<std::mutex> lock(g_mu);
        ++g_launches[name.substr(0, name.find('I') == std::string::npos ? name.size() : name.find('I'))];
    }
    if (grid.x == 0 || grid.y == 0 || grid.z == 0 || block.x == 0 || block.x * block.y * block.z > 1024)
        die("%s: launch shape %u x %u x %u blocks of %u x %u x %u", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z);
    const char* n = name.c_str();
    if (has(name, "16et_stream_kernelI")) {
        // ...et_stream_kernelI{d|f}Li<MODE>ELb<PITCHED>ELb<GUARD>EE...
        const size_t at = name.find("16et_stream_kernelI") + 19;
        const bool f64 = name[at] == 'd';
        const int mode = atoi(name.c_str() + at + 3);
        const size_t lb = name.find("ELb", at);
        const bool pitched = name[lb + 3] == '1';
        if (f64) shadow_stream(*static_cast<const StreamArgs<double>*>(args[0]), mode, pitched, grid, block, n);
        else shadow_stream(*static_cast<const StreamArgs<float>*>(args[0]), mode, pitched, grid, block, n);
    } else if (has(name, "21et_stream_redo_kernelI")) {
        const size_t at = name.find("21et_stream_redo_kernelI") + 24;
        if (name[at] == 'd') {
            const auto& a = *static_cast<const StreamArgs<double>*>(args[0]);
            need(a.diag_partial, sizeof(double) * kDiag * (size_t)a.nruns, 8, "diagnostics partials", n);
        } else {
            const auto& a = *static_cast<const StreamArgs<float>*>(args[0]);
            need(a.diag_partial, sizeof(double) * kDiag * (size_t)a.nruns, 8, "diagnostics partials", n);
            need(a.cancel_list, sizeof(uint16_t) * kCancelCap * (size_t)a.nruns, 2, "cancellation lists", n);
        }
    } else if (has(name, "23et_stream_cancel_kernelI")) {
        const auto& a = *static_cast<const StreamArgs<float>*>(args[0]);      // (float32 rasters only)
        need(a.diag_partial, sizeof(double) * kDiag * (size_t)a.nruns, 8, "diagnostics partials", n);
        need(a.cancel_list, sizeof(uint16_t) * kCancelCap * (size_t)a.nruns, 2, "cancellation lists", n);
    } else if (has(name, "9et_kernelI")) {
        const size_t at = name.find("9et_kernelI") + 11;
        if (name[at] == 'd') shadow_et(*static_cast<const EtArgs<double>*>(args[0]), grid, block, n);
        else shadow_et(*static_cast<const EtArgs<float>*>(args[0]), grid, block, n);
    } else if (has(name, "13method_kernelI")) {
        if (name[name.find("13method_kernelI") + 16] == 'd') shadow_method(*static_cast<const MethodArgs<double>*>(args[0]), n);
        else shadow_method(*static_cast<const MethodArgs<float>*>(args[0]), n);
    } else if (has(name, "13et_raw_kernelI")) {
        // ...et_raw_kernelI{d|f}Lb<FAST>EE...
        const size_t at = name.find("13et_raw_kernelI") + 16;
        const bool fast = name[at + 3] == '1';
        if (name[at] == 'd') shadow_raw(*static_cast<const RawArgs<double>*>(args[0]), fast, n);
        else shadow_raw(*static_cast<const RawArgs<float>*>(args[0]), fast, n);
    } else if (has(name, "18static_flag_kernelI") || has(name, "13static_kernelI")) {
        const bool pixels = has(name, "13static_kernelI");
        const size_t at = name.find(pixels ? "13static_kernelI" : "18static_flag_kernelI") + (pixels ? 16 : 21);
        if (name[at] == 'd') shadow_static(*static_cast<const StaticArgs<double>*>(args[0]), pixels, n);
        else shadow_static(*static_cast<const StaticArgs<float>*>(args[0]), pixels, n);
    } else if (has(name, "24static_obj_params_kernelI")) {
        if (name[after(name, "24static_obj_params_kernelI")] == 'd') shadow_obj_params<double>(args, grid, block, n);
        else shadow_obj_params<float>(args, grid, block, n);
    } else if (has(name, "17static_obj_kernelI")) {
        // ...static_obj_kernelI{d|f}Lb<TR>ELb<FOLD>EE...
        const size_t at = after(name, "17static_obj_kernelI");
        const bool fold = name[at + 7] == '1';
        if (name[at] == 'd') shadow_obj(*static_cast<const StaticObjArgs<double>*>(args[0]), fold, grid, block, n);
        else shadow_obj(*static_cast<const StaticObjArgs<float>*>(args[0]), fold, grid, block, n);
    } else if (has(name, "22static_obj_redo_kernelI")) {
        // ...static_obj_redo_kernelI{d|f}Lb<FOLD>EE...
        const size_t at = after(name, "22static_obj_redo_kernelI");
        const bool fold = name[at + 3] == '1';
        if (name[at] == 'd') shadow_obj_redo(*static_cast<const StaticObjRedoArgs<double>*>(args[0]), fold, grid, block, n);
        else shadow_obj_redo(*static_cast<const StaticObjRedoArgs<float>*>(args[0]), fold, grid, block, n);
    } else if (has(name, "21static_obj_any_kernel") || has(name, "23static_obj_final_kernel")) {
        // (any_gs, redo, ndraw, gx, any_draw) / (partial, redo, any_draw, ndraw, gx, sse, count)
        const bool fin = has(name, "23static_obj_final_kernel");
        const double* redo = *static_cast<const double* const*>(args[1]);
        const int64_t ndraw = *static_cast<const int64_t*>(args[fin ? 3 : 2]);
        const int gx = *static_cast<const int*>(args[fin ? 4 : 3]);
        need_block(block, n);
        need_cover(grid.x, kObjPerBlock, ndraw, "draws", n);
        if (gx < 1) die("%s: gx = %d", n, gx);
        const size_t nd = (size_t)ndraw;
        if (fin) need(*static_cast<const double* const*>(args[0]), sizeof(double) * 2 * nd * gx, 16, "partial", n);
        else need(*static_cast<const unsigned* const*>(args[0]), sizeof(unsigned) * nd * gx, 4, "any_gs", n);
        if (redo) need(redo, sizeof(double) * 5 * nd, 8, "redo", n);
        need(*static_cast<const unsigned* const*>(args[fin ? 2 : 4]), sizeof(unsigned) * nd, 4, "any_draw", n);
        if (fin) {
            need(*static_cast<double* const*>(args[5]), sizeof(double) * nd, 8, "sse", n);
            need(*static_cast<double* const*>(args[6]), sizeof(double) * nd, 8, "count", n);
        }
    } else if (has(name, "25static_annual_redo_kernelI")) {
        shadow_annual_redo(*static_cast<const StaticAnnualRedoArgs<double>*>(args[0]), grid, block, n);     // (float64 only)
    } else if (has(name, "26static_annual_final_kernel")) {
        shadow_annual_final(args, grid, block, n);
    } else if (has(name, "25static_rows_gather_kernelI")) {
        shadow_rows_gather(args, name[after(name, "25static_rows_gather_kernelI")] == 'd' ? 8 : 4, block, n);
    } else if (has(name, "10ens_kernelI") || has(name, "15ens_redo_kernelI")) {
        // ...ens_kernelI{d|f}Lb<FAST>EE... / ...ens_redo_kernelI{d|f}E...
        const bool redo = has(name, "15ens_redo_kernelI");
        const size_t at = after(name, redo ? "15ens_redo_kernelI" : "10ens_kernelI");
        const bool fast = !redo && name[at + 3] == '1';
        if (name[at] == 'd') shadow_ens(*static_cast<const EnsArgs<double>*>(args[0]), fast, block, n);
        else shadow_ens(*static_cast<const EnsArgs<float>*>(args[0]), fast, block, n);
    } else if (has(name, "20static_domain_kernelI")) {
        uint8_t* skip = *static_cast<uint8_t* const*>(args[1]);
        if (!skip) die("%s: no domain mask", n);
        if (name[after(name, "20static_domain_kernelI")] == 'd') shadow_batch(*static_cast<const StaticBatchArgs<double>*>(args[0]), skip, false, false, grid, block, n);
        else shadow_batch(*static_cast<const StaticBatchArgs<float>*>(args[0]), skip, false, false, grid, block, n);
    } else if (has(name, "24static_batch_flag_kernelI") || has(name, "19static_batch_kernelI") ||
               has(name, "29static_batch_flag_fast_kernelI") || has(name, "24static_batch_fast_kernelI") ||
               has(name, "32static_batch_flag_skipped_kernelI") || has(name, "29static_batch_redo_rows_kernelI")) {
        const bool fast = has(name, "_fast_kernelI");
        const bool skipped = has(name, "flag_skipped_kernelI") || has(name, "redo_rows_kernelI");
        if (name[name.find("kernelI") + 7] == 'd') shadow_batch(*static_cast<const StaticBatchArgs<double>*>(args[0]), nullptr, fast, skipped, grid, block, n);
        else shadow_batch(*static_cast<const StaticBatchArgs<float>*>(args[0]), nullptr, fast, skipped, grid, block, n);
    } else if (has(name, "23static_batch_sse_kernelI")) {
        // (total [gridDim.x][n], obs [n], weights [n] or NULL, n, sse, cnt [gridDim.x])
        const size_t el = name[after(name, "23static_batch_sse_kernelI")] == 'd' ? 8 : 4;
        const int64_t cnt = *static_cast<const int64_t*>(args[3]);
        need_block(block, n);
        if (cnt <= 0) die("%s: n = %lld", n, (long long)cnt);
        need(*static_cast<const void* const*>(args[0]), el * (size_t)cnt * grid.x, el, "total rows", n);
        need(*static_cast<const void* const*>(args[1]), el * (size_t)cnt, el, "observed", n);
        if (*static_cast<const void* const*>(args[2])) need(*static_cast<const void* const*>(args[2]), el * (size_t)cnt, el, "weights", n);
        need(*static_cast<double* const*>(args[4]), sizeof(double) * grid.x, 8, "sse", n);
        need(*static_cast<double* const*>(args[5]), sizeof(double) * grid.x, 8, "count", n);
    } else if (has(name, "15zero_u32_kernel")) {
        const int64_t cnt = *static_cast<const int64_t*>(args[1]);
        need_block(block, n);
        need_cover(grid.x, kBlock, cnt, "words", n);
        need(*static_cast<unsigned* const*>(args[0]), sizeof(unsigned) * (size_t)cnt, 4, "words", n);
    } else if (has(name, "16mcmc_init_kernel")) {
        shadow_mcmc(*static_cast<const McmcArgs*>(args[0]), *static_cast<const double* const*>(args[1]), false, false, grid, block, n);
    } else if (has(name, "23mcmc_init_accept_kernel")) {
        shadow_mcmc(*static_cast<const McmcArgs*>(args[0]), nullptr, false, false, grid, block, n);
    } else if (has(name, "19mcmc_propose_kernel")) {
        shadow_mcmc(*static_cast<const McmcArgs*>(args[0]), nullptr, true, false, grid, block, n);
    } else if (has(name, "18mcmc_accept_kernel")) {
        shadow_mcmc(*static_cast<const McmcArgs*>(args[0]), nullptr, false, true, grid, block, n);
    } else if (has(name, "12synth_kernelI")) {
        const size_t at = name.find("12synth_kernelI") + 15;
        if (name[at] == 'd') shadow_synth(*static_cast<const SynthArgs<double>*>(args[0]), n);
        else shadow_synth(*static_cast<const SynthArgs<float>*>(args[0]), n);
    } else if (has(name, "17diag_stage_kernel")) {
        const double* partial = *static_cast<const double* const*>(args[0]);
        const int64_t count = *static_cast<const int64_t*>(args[1]), per = *static_cast<const int64_t*>(args[2]);
        double* out = *static_cast<double* const*>(args[3]);
        if (per < 1 || (int64_t)grid.x * per < count) die("%s: %u slices of %lld do not cover %lld partials", n, grid.x, (long long)per, (long long)count);
        need(partial, sizeof(double) * kDiag * (size_t)count, 8, "partials", n);
        need(out, sizeof(double) * kDiag * grid.x, 8, "stage output", n);
    } else if (has(name, "23diag_final_fused_kernel") || has(name, "17diag_final_kernel")) {
        const double* partial = *static_cast<const double* const*>(args[0]);
        const int nb = *static_cast<const int*>(args[1]);
        double* out = *static_cast<double* const*>(args[has(name, "fused") ? 3 : 2]);
        if (nb < 1) die("%s: %d partials", n, nb);
        need(partial, sizeof(double) * kDiag * (size_t)nb, 8, "partials", n);
        need(out, sizeof(double) * kDiag, 8, "diagnostics vector", n);
    } else if (has(name, "19diag_partial_kernelI")) {
        const int64_t cnt = *static_cast<const int64_t*>(args[2]);
        const bool f64 = name[name.find("19diag_partial_kernelI") + 22] == 'd';
        need(*static_cast<const void* const*>(args[0]), (f64 ? 8 : 4) * (size_t)cnt, f64 ? 8 : 4, "day", n);
        need(*static_cast<const void* const*>(args[1]), (f64 ? 8 : 4) * (size_t)cnt, f64 ? 8 : 4, "night", n);
        need(*static_cast<double* const*>(args[3]), sizeof(double) * kDiag * grid.x, 8, "partials", n);
    } else if (has(name, "16fold_diag_kernel")) {
        const int world = *static_cast<const int*>(args[1]);
        need(*static_cast<const double* const*>(args[0]), sizeof(double) * kDiag * (size_t)world, 8, "gathered vectors", n);
        need(*static_cast<double* const*>(args[2]), sizeof(double) * kDiag, 8, "diagnostics vector", n);
    } else if (has(name, "11copy_kernel")) {
        const int64_t nvec = *static_cast<const int64_t*>(args[2]);
        need(*static_cast<const void* const*>(args[0]), 16 * (size_t)nvec, 16, "source", n);
        need(*static_cast<void* const*>(args[1]), 16 * (size_t)nvec, 16, "destination", n);
    } else {
        std::lock_guard<std::mutex> lock(g_mu);
        ++g_unchecked[name.substr(0, 48)];
    }
}

}  // namespace stub

extern "C" void mod16_stub_report(FILE* f) {
    for (auto& kv : stub::batch_next()) stub::die("%s: its launches stopped before draw %lld", kv.first.c_str(), (long long)kv.second);
    fprintf(f, "hip_stub: %ld address ranges checked; live allocations %zu\n", stub::g_checked_ranges, stub::g_blocks.size());
    for (auto& kv : stub::g_launches) fprintf(f, "  launches  %-44s %ld\n", kv.first.c_str(), kv.second);
    for (auto& kv : stub::g_unchecked) fprintf(f, "  launch shape only (no shadow)  %-48s %ld\n", kv.first.c_str(), kv.second);
}
extern "C" size_t mod16_stub_live_allocations(void) { return stub::g_blocks.size(); }

// ------------------------------------------------------------------ the runtime's entry points
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle[1]; return handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    stub::g_kernels[host] = device_name;
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}

static thread_local struct { dim3 grid, block; size_t shmem; hipStream_t stream; } t_cfg;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    t_cfg = {grid, block, shmem, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    *grid = t_cfg.grid; *block = t_cfg.block; *shmem = t_cfg.shmem; *stream = t_cfg.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* func, dim3 grid, dim3 block, void** args, size_t, hipStream_t) {
    auto it = stub::g_kernels.find(func);
    if (it == stub::g_kernels.end()) stub::die("launch of an unregistered kernel %p", func);
    stub::run_shadow(it->second, grid, block, args);
    return hipSuccess;
}

hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int) {
    memset(p, 0, sizeof *p);
    strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
    p->multiProcessorCount = stub::g_cus;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }

static int g_fail_malloc = 0;           // mod16_stub_fail_malloc(k): the k-th next hipMalloc / hipMallocAsync fails, once (0: none)
extern "C" void mod16_stub_fail_malloc(int k) { g_fail_malloc = k; }
hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_malloc > 0 && --g_fail_malloc == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = stub::alloc(bytes);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) { return stub::release(p); }
hipError_t hipMallocAsync(void** p, size_t bytes, hipStream_t) { return hipMalloc(p, bytes); }
hipError_t hipFreeAsync(void* p, hipStream_t) { return stub::release(p); }
// page-locked host memory is in the device's address space too (the HOST mode's small calls hand it
// to their kernels): a tracked block like any other, always real memory
static int g_fail_host_malloc = 0;      // mod16_stub_fail_host_malloc(k): the next k hipHostMalloc calls fail; (-k): the k-th next one, once
extern "C" void mod16_stub_fail_host_malloc(int k) { g_fail_host_malloc = k; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    if (g_fail_host_malloc > 0) { --g_fail_host_malloc; *p = nullptr; return hipErrorOutOfMemory; }
    if (g_fail_host_malloc < 0 && ++g_fail_host_malloc == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    if (bytes >= stub::kRealBelow) stub::die("hipHostMalloc of %zu bytes: the library pins small buffers only", bytes);
    *p = stub::alloc(bytes);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { return stub::release(p); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) { *dev = host; return hipSuccess; }

static hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    // the device side of a copy must be a device allocation; host sides are plain memory under ASan
    bool fake = false;
    if (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice)
        if (!stub::inside(dst, bytes, &fake)) stub::die("copy of %zu bytes to device %p: outside every allocation", bytes, dst);
    if (kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice)
        if (!stub::inside(src, bytes, &fake)) stub::die("copy of %zu bytes from device %p: outside every allocation", bytes, src);
    if (!fake) memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { return copy(dst, src, bytes, kind); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) { return copy(dst, src, bytes, kind); }
static hipError_t fill(void* dst, int v, size_t bytes) {
    bool fake = false;
    if (!stub::inside(dst, bytes, &fake)) stub::die("memset of %zu bytes at device %p: outside every allocation", bytes, dst);
    if (!fake) memset(dst, v, bytes);
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t bytes) { return fill(dst, v, bytes); }
hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t) { return fill(dst, v, bytes); }

// streams, events and graphs: inert handles (heap objects, so leaks and double destroys show)
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = reinterpret_cast<hipStream_t>(new int(1)); return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t* s) { return hipStreamCreateWithFlags(s, 0); }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<int*>(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static thread_local bool t_capturing = false;
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) {
    *st = t_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { t_capturing = true; return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* g) { t_capturing = false; *g = reinterpret_cast<hipGraph_t>(new int(2)); return hipSuccess; }
hipError_t hipGraphInstantiate(hipGraphExec_t* e, hipGraph_t, hipGraphNode_t*, char*, size_t) { *e = reinterpret_cast<hipGraphExec_t>(new int(3)); return hipSuccess; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t e) { delete reinterpret_cast<int*>(e); return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t g) { delete reinterpret_cast<int*>(g); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new int(4)); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<int*>(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 1.0f; return hipSuccess; }
}
