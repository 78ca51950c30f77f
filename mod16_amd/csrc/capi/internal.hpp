// libmod16hip.so, host side: what the entry-point families (capi/*.hip) share -- the device
// context, the launch machinery of the pipeline and of the plain kernels (the HOST mode: host.hpp).
// Internal linkage throughout (every translation unit holds its own copy of what it uses);
// mod16_capi.hip includes all families into ONE unit for single-command builds (variants,
// tests/host_asan, listings), mod16_amd/csrc/build.py compiles them side by side.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mod16_hip.h"
#include "own.hpp"
#include "../mod16_kernels.hpp"
#include "../mod16_stream.hpp"

using namespace mod16;

namespace {
constexpr int kDiagBlocks = 1024;
constexpr int kSlots = 12;                          // staging slots = host threads of the HOST mode
constexpr int kSmallPixels = 65536;                 // HOST mode: calls up to this size take the copy-free path
constexpr int kSmallPixelsMax = 1 << 18;            // ... and what MOD16_SMALL_PIXELS may raise it to
}  // namespace

// Workspace of the per-run diagnostics partials of et_stream_kernel (and of the
// stand-alone reduction). The context owns one, sized on demand; a captured
// graph owns its own, so growing the context's never pulls memory from under
// a graph that is replayed later.
struct DiagWs {
    DevMem mem;                  // device [capacity][kDiag], then 128 bytes: the "blocks done" counter
    int64_t capacity = 0;        // in partials
    double* partial() const { return mem.as<double>(); }
    unsigned* done() const { return reinterpret_cast<unsigned*>(partial() + capacity * 8); }
};

// A captured graph's kernel nodes point into its context (parameter table, exp / log tables, status
// word): the context keeps a list of its live graphs, and mod16_destroy marks them dead -- a replay
// of one returns MOD16_ERR_ARG instead of reading freed memory; mod16_graph_destroy still frees it.
// One process-wide lock (an inline function: the same object in every translation unit of the library).
inline std::mutex& graph_registry_mu() {
    static std::mutex mu;
    return mu;
}

struct mod16_ctx {
    std::recursive_mutex api_mu;     // every entry point holds it: a ctx may be shared by threads
    int device = 0;
    int cus = 256;
    int grid_mult = 64;              // blocks per CU in the grid-stride launches of the plain kernels
    int host_threads = 8;            // MOD16_HOST_THREADS: staging threads of the HOST mode (1..kSlots)
    // launch geometry; fixed in the shipped library, overridable in -DMOD16_EXPERIMENTS builds only
    bool use_dma = true;             // production pipeline (mod16_stream.hpp); off: plain kernels only
    int run_shift = -1;              // force 2^k pieces per run
    int stream_blocks = 2;           // blocks of the pipeline kernel per CU (1 = one wave per SIMD)
    int static_below = 8;            // runs per wave below which runs are dealt out statically (0: never)
    int use_pitch = 1;               // scalar base + pitch addressing for slab layouts
    int poison_byte = -1;            // ... MOD16_POISON_BYTE=b: the byte every byte of that ticket is set to (default: the ticket becomes 2^40)
    int poison_ticket = 0;           // experiments build, MOD16_POISON_TICKET=k: the k-th dynamically scheduled launch finds
                                     // its ticket counter in use (what an abandoned launch leaves behind): the test of kStatusIncomplete
    // Ownership: DevMem / PinnedMem / Event / Stream members own what they name and free it with the
    // context, in reverse order of declaration (the streams, declared last, go first); raw pointers
    // are views of memory owned elsewhere.
    DevMem dyn_counters;             // ring of ticket counters (unsigned long long), 128 B apart
    int dyn_next = 0;
    bool have_lut = false;
    DevMem lut64;                    // device double [MOD16_LUT_ROWS][kLutCols]
    DevMem lut32;                    // ... float
    DevMem tab64;                    // exp/log tables of FastMath<double>
    DevMem status;                   // device status word (unsigned)
    PinnedMem status_host;           // pinned mirror
    DevMem static_flag;              // device word of mod16_et_static_*
    DiagWs ws;                       // diagnostics partials of launches outside a graph
    std::vector<DevMem> retired;     // outgrown workspaces (freed with the context)
    std::vector<mod16_graph*> graphs; // graphs captured with this context and still alive (graph_registry_mu); views
    DiagWs* force_ws = nullptr;      // workspace to use instead (graph capture); a view
    Event ws_event;                  // recorded behind the last launch that produced diagnostics in `ws`
    hipStream_t ws_stream = nullptr; // ... and the stream it ran on (the caller's)
    bool ws_pending = false;
    bool ws_recorded = false;        // ... and whether ws_event was recorded behind it
    bool ws_multi = false;           // the context has launched on more than one stream (or runs HOST tiles on
                                     // its slots): every launch records ws_event from now on
    DevMem diag_dev;                 // device double [kDiag]
    PinnedMem diag_host;             // pinned double [kDiag]
    DevMem hdiag_dev;                // device double [kSlots][kDiag]: per-tile diagnostics of the HOST mode (mod16_et_hdiag_*)
    // HOST-mode staging: per slot one device slab (+ one stream, below)
    DevMem slab[kSlots];
    size_t slab_bytes = 0;           // what every slab holds (the largest call seen)
    std::mutex launch_mu;            // HOST mode: kernel launches of the staging threads
    DevMem scalars;                  // device copies of broadcast scalars
    // HOST mode, small calls (a flux-tower site, a year of one pixel): one page-locked buffer the
    // kernel reads its inputs from and writes its outputs to over the link -- no copy commands at all
    int small_pixels = kSmallPixels; // MOD16_SMALL_PIXELS: calls of at most this many pixels go that way (0: none)
    PinnedMem small_host;
    void* small_dev = nullptr;       // ... as the device addresses it; a view
    unsigned long long* force_counter = nullptr;   // ticket counter to use instead of the ring (graph capture); a view
    DevMem bc_buf;                   // HOST mode: device copies of (N,) / (T, 1) inputs (mod16_et2_*); only grows
    DevMem batch_buf;                // HOST-mode workspace of mod16_et_static_batch_*; only grows
    DevMem smooth_ws;                // mod16_smooth_*: 2 KiB for a HOST-mode weight table, then the columns of the pixels
                                     // in flight; only grows (the outgrown block is retired), launches ordered by ws_event
    DevMem regress_design;           // mod16_regress_*: a HOST-mode call's design on the device; only grows (the outgrown block is retired)
    std::string err;
    Stream streams[kSlots];          // one per staging slot, made on first use; [0] also serves the other HOST-mode calls
};

#define HIPCHK(ctx, call)                                                          \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                    \
            char b_[512];                                                          \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call,                \
                     hipGetErrorString(e_), __FILE__, __LINE__);                   \
            (ctx)->err = b_;                                                       \
            return MOD16_ERR_HIP;                                                  \
        }                                                                          \
    } while (0)

// every entry point that takes a ctx holds its mutex for the duration of the call
#define MOD16_LOCK(ctx) std::unique_lock<std::recursive_mutex> api_lock_; \
    if (ctx) api_lock_ = std::unique_lock<std::recursive_mutex>((ctx)->api_mu)

static int fail(mod16_ctx* ctx, int code, const char* msg) {
    if (ctx) ctx->err = msg;
    return code;
}
// ... with the message in two parts: prefix ("<entry point>: "), then what is wrong
static int fail(mod16_ctx* ctx, int code, const char* prefix, const char* what) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s%s", prefix, what);
    return fail(ctx, code, msg);
}

// A workspace for `blocks` partials + the (zeroed) counter behind them
static int ws_alloc(mod16_ctx* ctx, DiagWs& ws, int64_t blocks) {
    ws.capacity = 0;
    int rc = ws.mem.alloc(ctx, sizeof(double) * (blocks * 8 + 16), "device memory for the diagnostics workspace");
    if (rc != MOD16_OK) return rc;
    ws.capacity = blocks;
    HIPCHK(ctx, hipMemset(ws.done(), 0, 128));
    return MOD16_OK;
}

// One allocation carved into arrays: pieces of whole 256-byte lines taken in order from `base`.
// With base NULL the pointers are NULL and `used` is the size to allocate.
static size_t align256(size_t x) { return (x + 255) / 256 * 256; }
struct Carver {
    char* base;
    size_t used = 0;
    explicit Carver(void* b = nullptr) : base(static_cast<char*>(b)) {}
    template <typename T> T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += align256(bytes);
        return p;
    }
};

// A (13, 11) parameter table -> the table the kernels index by class code: [MOD16_LUT_ROWS][kLutCols]
// float64, row-major by parameter -- the 11 parameters, the derived reciprocals, NaN in the columns
// behind class 12 (mod16_set_bplut_f64, and every member of mod16_ensemble_create).
static void derive_lut(const double* lut, double* h64) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int c = 0; c < kLutCols; ++c) {
        double row[MOD16_LUT_ROWS];
        for (int k = 0; k < MOD16_LUT_ROWS; ++k) row[k] = nan;
        if (c < MOD16_N_CLASSES) {
            const double* p = lut + (size_t)c * MOD16_N_PARAMS;
            for (int k = 0; k < MOD16_N_PARAMS; ++k) row[k] = p[k];
            row[11] = 1.0 / (p[MOD16_TMIN_OPEN] - p[MOD16_TMIN_CLOSE]);
            row[12] = 1.0 / (p[MOD16_VPD_CLOSE] - p[MOD16_VPD_OPEN]);
            row[13] = (p[MOD16_RBL_MAX] - p[MOD16_RBL_MIN]) / (p[MOD16_VPD_CLOSE] - p[MOD16_VPD_OPEN]);
            row[14] = 1.0 / p[MOD16_BETA];
            // smallest float32 >= 273.15 + tmin_close: for a float32 x,
            // x >= 273.15 + tmin_close (in float64) <=> x >= this (mixed-precision form)
            const double thr = 273.15 + p[MOD16_TMIN_CLOSE];
            float tf = (float)thr;
            if ((double)tf < thr) tf = std::nextafterf(tf, std::numeric_limits<float>::infinity());
            row[15] = (double)tf;
        }
        for (int k = 0; k < MOD16_LUT_ROWS; ++k) h64[k * kLutCols + c] = row[k];
    }
}

// ------------------------------------------------------------------ launch
template <typename T> static const T* ctx_lut(const mod16_ctx* ctx);
template <> const double* ctx_lut<double>(const mod16_ctx* ctx) { return ctx->lut64.as<double>(); }
template <> const float* ctx_lut<float>(const mod16_ctx* ctx) { return ctx->lut32.as<float>(); }


template <typename T> struct VecOf;
template <> struct VecOf<double> { static constexpr int v = 2; };
template <> struct VecOf<float> { static constexpr int v = 4; };

// Instantiated variants: the production (FAST, vectorised) kernel gets the
// SEP / DENSE specialisations; the scalar-tail and EXACT kernels are generic.
template <typename T, int V>
static void launch_variant(const EtArgs<T>& a, bool lut, bool fast, bool sep, bool dense,
                           int grid, hipStream_t st) {
    // FAST on float32 with 4 pixels per thread is never built (see launch_et): EXACT only
#ifdef MOD16_REPRO_V4   // reproduction builds of DESIGN.md 5.2 only (tools/repro_v4.py)
    constexpr bool kFastOk = true;
#else
    constexpr bool kFastOk = !(std::is_same<T, float>::value && V == 4);
#endif
    if (a.out[8] || a.out[9]) {   // potential ET wanted: the generic all-outputs form
#define MOD16_LAUNCH_PET(LUT, FAST) \
    hipLaunchKernelGGL((et_kernel<T, V, LUT, FAST, true, false, true>), dim3(grid), dim3(kBlock), 0, st, a)
        if constexpr (kFastOk) {
            if (fast) {
                if (lut) {
                    MOD16_LAUNCH_PET(true, true);
                } else {
                    // per-pixel parameter arrays + potential ET: one pixel per thread (with two,
                    // the 25 inputs, 10 outputs and the guard's slow branch do not fit the
                    // register budget of two waves per SIMD without spilling)
                    const int g1 = (int)std::min<int64_t>((a.n + kBlock - 1) / kBlock, (int64_t)grid * V);
                    hipLaunchKernelGGL((et_kernel<T, 1, false, true, true, false, true>), dim3(std::max(1, g1)),
                                       dim3(kBlock), 0, st, a);
                }
                return;
            }
        }
        if (lut) MOD16_LAUNCH_PET(true, false); else MOD16_LAUNCH_PET(false, false);
#undef MOD16_LAUNCH_PET
        return;
    }
#define MOD16_LAUNCH(LUT, FAST, SEP, DENSE) \
    hipLaunchKernelGGL((et_kernel<T, V, LUT, FAST, SEP, DENSE>), dim3(grid), dim3(kBlock), 0, st, a)
    if constexpr (kFastOk && V > 1) {
        if (fast) {
            if (lut) {
                if (sep) { if (dense) MOD16_LAUNCH(true, true, true, true); else MOD16_LAUNCH(true, true, true, false); }
                else     { if (dense) MOD16_LAUNCH(true, true, false, true); else MOD16_LAUNCH(true, true, false, false); }
            } else if (sep) {
                // per-pixel parameter arrays + the six components: one pixel per thread (with two,
                // 25 inputs, 8 outputs and the guard's slow branch spill two registers)
                const int g1 = (int)std::min<int64_t>((a.n + kBlock - 1) / kBlock, (int64_t)grid * V);
                hipLaunchKernelGGL((et_kernel<T, 1, false, true, true, false>), dim3(std::max(1, g1)),
                                   dim3(kBlock), 0, st, a);
            } else {
                if (dense) MOD16_LAUNCH(false, true, false, true); else MOD16_LAUNCH(false, true, false, false);
            }
            return;
        }
    } else if constexpr (kFastOk) {
        if (fast) {
            if (lut) MOD16_LAUNCH(true, true, true, false); else MOD16_LAUNCH(false, true, true, false);
            return;
        }
    }
    if (lut) MOD16_LAUNCH(true, false, true, false); else MOD16_LAUNCH(false, false, true, false);
#undef MOD16_LAUNCH
}

static int grid_for(const mod16_ctx* ctx, int64_t nvec) {
    int64_t need = (nvec + kBlock - 1) / kBlock;
    int64_t cap = (int64_t)ctx->cus * ctx->grid_mult;
    return (int)std::max<int64_t>(1, std::min(need, cap));
}
// ... of the kernels that walk batches of kBlock items block by block: a block per batch, at most 8 per CU
static int batch_blocks(const mod16_ctx* ctx, int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, (int64_t)ctx->cus * 8));
}

// All pointers are device pointers here.
// -> the workspace for `blocks` partials: the forced one (graph capture; it was
// sized by its owner) or the context's, grown if need be. Captured graphs never
// point into the context's workspace, so it can be replaced once the device is idle.
static int reserve_diag(mod16_ctx* ctx, int64_t blocks, DiagWs** out = nullptr) {
    if (ctx->force_ws) {
        if (blocks > ctx->force_ws->capacity)
            return fail(ctx, MOD16_ERR_ARG, "internal: graph workspace smaller than its launch");
        if (out) *out = ctx->force_ws;
        return MOD16_OK;
    }
    if (out) *out = &ctx->ws;
    if (blocks <= ctx->ws.capacity) return MOD16_OK;
    // Growing: earlier launches may still use the old block. No device-wide wait (other
    // contexts of the process -- the workers of mod16_amd.io -- would stall with this one) and
    // no hipFree (which synchronises the device): the old block is retired and freed with the
    // context; sizes at least double, so the retired blocks add up to less than the live one.
    // Launches that follow use the new block and are ordered behind the old one's by the
    // workspace event as before.
    const int64_t want = std::max<int64_t>(blocks, 2 * ctx->ws.capacity);
    ctx->retired.push_back(std::move(ctx->ws.mem));
    return ws_alloc(ctx, ctx->ws, want);
}

// The context's workspace is shared by its launches (every pipeline launch
// writes per-run partials, wanted or not). Launches on ONE stream are ordered
// anyway; a launch on another stream than the previous one waits for it, so the
// previous launch's final sum has read its partials before they are overwritten.
// Inside a graph capture the graph's own workspace is used instead.
static int ws_acquire(mod16_ctx* ctx, hipStream_t st) {
    if (ctx->force_ws) return MOD16_OK;
    // A caller capturing its own stream into a graph would bake the context's workspace (which
    // may be replaced later) and this event bookkeeping into it: refused -- mod16_graph_* builds
    // graphs that own their workspace.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(ctx, MOD16_ERR_ARG, "the stream is being captured into a graph: use mod16_graph_et_diag_* / "
                                        "mod16_graph_et_tiled_* (they capture the step with a workspace of its own)");
    // Ordering across streams costs a marker packet behind EVERY launch (the event) -- part of the
    // 5.5 us that lie between two 1200 x 1200 launches on one stream -- so a context pays for it
    // only once it has seen a second stream (round 5): until then nothing is recorded; the first
    // launch that arrives on another stream waits for the DEVICE (once per context: the earlier
    // stream may be gone by now -- its owner may destroy it, and an event cannot be recorded on a
    // destroyed stream), and from then on every launch leaves its event behind (ws_release).
    if (ctx->ws_pending && st != ctx->ws_stream) {
        if (ctx->ws_recorded) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ws_event, 0));
        else HIPCHK(ctx, hipDeviceSynchronize());
        ctx->ws_multi = true;
        ctx->ws_pending = false;
    }
    return MOD16_OK;
}
static int ws_release(mod16_ctx* ctx, hipStream_t st) {
    if (ctx->force_ws) return MOD16_OK;
    ctx->ws_recorded = false;
    if (ctx->ws_multi) {
        HIPCHK(ctx, hipEventRecord(ctx->ws_event, st));
        ctx->ws_recorded = true;
    }
    ctx->ws_stream = st;
    ctx->ws_pending = true;
    return MOD16_OK;
}

template <typename T>
static int reduce_entry(mod16_ctx* ctx, const T* day, const T* night, int64_t n, double* diag,
                        double* ddiag, void* stream);

// Launch geometry of the production pipeline for n pixels, V per 16-byte vector.
struct StreamGeom { int run_shift; int64_t npiece, nruns; int grid; int static_sched; };
static StreamGeom stream_geom(const mod16_ctx* ctx, int64_t n, int V, int tile_shift = kNoTile) {
    StreamGeom g;
    g.npiece = (n / V + 63) / 64;
    // run length: kDynRun pieces, halved for small rasters until every wave the
    // chip holds (2 blocks of 4 per CU) gets at least one run
    const int64_t chip_waves = (int64_t)ctx->cus * 2 * (kBlock / 64);
    int run_shift = 0;
    while ((1 << run_shift) < kDynRun) ++run_shift;
    // tiled rasters: runs of 2 kDynRun pieces (16 KiB per field, half a default tile):
    // -0.8 % on the global grid in two same-box A/Bs, where on plain arrays runs of 16
    // measured +0.4-1.4 % (round 1); fewer claims and partials, the tail stays < 0.5 %
    if (tile_shift != kNoTile) ++run_shift;
    while (run_shift > 1 && (g.npiece >> run_shift) < chip_waves) --run_shift;   // >= 2 pieces: the claim of a run is consumed in its second iteration
    // A small raster (fewer than kStaticBelow runs per wave) is latency-bound and ends
    // with its slowest SIMD: single pieces dealt out round-robin -- all waves start together,
    // no claim's round trip sits on a path that is only a few iterations long, and the load is
    // balanced to within one PIECE per wave. (Rounds 2-3 dealt runs of 2 pieces: a 1200 x 1200
    // raster, 11250 pieces over 2048 waves, then gave the waves 6 or 4 pieces, and since a CU holds
    // blocks c and c + 256, the first 127 CUs got 12 pieces per SIMD against an average of 11;
    // piece by piece it is 6 or 5 per wave and at most 11 per SIMD.)
    g.static_sched = 0;
    if (ctx->static_below > 0 && (g.npiece >> run_shift) < (int64_t)ctx->static_below * chip_waves) {
        g.static_sched = 1;
        run_shift = 0;
    }
    if (ctx->run_shift > 0) run_shift = ctx->run_shift;
    run_shift = std::min(run_shift, tile_shift);     // a run never straddles two tiles
    g.run_shift = run_shift;
    g.nruns = (g.npiece + (int64_t(1) << run_shift) - 1) >> run_shift;
    // persistent waves: 2 blocks per CU is what the LDS slots allow
    g.grid = (int)std::max<int64_t>(1, std::min<int64_t>(
        (g.nruns + (kBlock / 64) - 1) / (kBlock / 64), (int64_t)ctx->cus * ctx->stream_blocks));
    return g;
}
constexpr int kStage = 1024;     // slices of the two-level sum of the per-run partials
// workspace of a pipeline launch, in partials (64 bytes): one per run, the stage of the two-level sum,
// and one more per run -- the run's cancellation list (mixed-precision forms, mod16_stream.hpp)
static_assert(kCancelCap * sizeof(uint16_t) == kDiag * sizeof(double), "a cancellation list is the size of a partial");
static int64_t stream_ws_blocks(int64_t nruns) { return 2 * nruns + kStage; }
constexpr int64_t kFuseFinalBelow = 16384;   // partials up to which the pipeline kernel sums them itself

// The production pipeline for dense class rasters (mod16_stream.hpp). s.n must
// be a multiple of the vector width. ddiag != NULL: also the fixed-order sum
// of the per-run diagnostics partials -> ddiag (8 doubles on the device), over
// n_valid_total pixels.
// GUARD = false: MOD16_DOMAIN_TRUSTED (the instance without the domain test; totals forms).
template <typename T, int MODE, bool GUARD = true>
static int launch_stream(mod16_ctx* ctx, StreamArgs<T> s, hipStream_t st, double* ddiag = nullptr) {
    constexpr int V = VecOf<T>::v;
    s.lut64 = ctx->lut64.as<double>();
    s.tab = ctx->tab64.as<double>();
    s.status = ctx->status.as<unsigned>();
    if (s.tile_shift <= 0) {       // plain arrays: one "tile"
        s.tile_shift = kNoTile;
        s.wide_row = s.out_row = s.byte_row = 0;
    }
    const StreamGeom g = stream_geom(ctx, s.n, V, s.tile_shift);
    // (the pipeline kernel's piece numbers and tile rows are 32-bit scalars: 2^30 pieces are 137 G
    // float64 pixels -- a raster of 1.7 TB -- and a row is 15 tiles' worth of elements)
    if (g.npiece > kMaxPieces || (uint64_t)s.wide_row >> 32 || (uint64_t)s.out_row >> 32 || (uint64_t)s.byte_row >> 32)
        return fail(ctx, MOD16_ERR_ARG, "pipeline launch: more than 2^30 pieces, or a tile row of 2^32 elements or more");
    unsigned long long* ctr = ctx->force_counter ? ctx->force_counter
                                                 : ctx->dyn_counters.as<unsigned long long>() + 16 * (ctx->dyn_next++ % 64);
    // the ticket counter of the dynamic schedule (a statically scheduled raster never reads it):
    // zero when it was allocated, and every launch leaves it at zero again (the kernel's last
    // block resets it) -- no memset in front of the kernel, see et_stream_kernel
    s.dyn_counter = ctr;
#ifdef MOD16_EXPERIMENTS
    if (ctx->poison_ticket > 0 && !g.static_sched && --ctx->poison_ticket == 0) {
        // (MOD16_POISON_TICKET=k: the k-th dynamically scheduled launch of the context) the ticket
        // -- zero between launches -- becomes 2^40: "every run has been claimed", as a counter left
        // behind by an abandoned launch says: the waves process their first, statically assigned
        // runs and find nothing to claim
        // MOD16_POISON_BYTE=b (round 6): all eight bytes of the ticket become b instead -- 0x3f is the
        // pattern whose (nwaves + ticket) << run_shift overflowed into a negative base in round 5 (a
        // wild read and a wild store); 0xff is -1. The kernel clamps the ticket before it forms a base.
        if (ctx->poison_byte >= 0) HIPCHK(ctx, hipMemsetAsync(ctr, ctx->poison_byte, 8, st));
        else HIPCHK(ctx, hipMemsetAsync(reinterpret_cast<char*>(ctr) + 5, 1, 1, st));
    }
#endif
    s.run_shift = g.run_shift;
    s.static_sched = g.static_sched;
    const int grid = g.grid;
    // partials: one per run, or (static schedule) one per block
    const int64_t nruns = g.static_sched ? grid : g.nruns;
    DiagWs* ws = nullptr;
    int rc = reserve_diag(ctx, stream_ws_blocks(nruns), &ws);
    if (rc != MOD16_OK) return rc;
    rc = ws_acquire(ctx, st);
    if (rc != MOD16_OK) return rc;
    s.diag_partial = ws->partial();
    s.cancel_list = reinterpret_cast<uint16_t*>(ws->partial() + (nruns + kStage) * kDiag);
    // few partials: the kernel's last block adds them up itself (two dispatches less)
    // (only under the static schedule: a dynamically scheduled raster's flagged pieces are
    // revisited by the kernel BEHIND this one, which corrects the partials before they are summed)
    const bool fused_final = ddiag && g.static_sched && nruns <= kFuseFinalBelow;
    s.diag_out = fused_final ? ddiag : nullptr;
    s.done_counter = ws->done();
    s.nruns = nruns;
    // equally spaced wide arrays (one slab): scalar base + k * pitch
    constexpr int NW = StreamSpec<MODE>::NW;
    const ptrdiff_t pitch_b = reinterpret_cast<const char*>(s.wide[1]) - reinterpret_cast<const char*>(s.wide[0]);
    bool pitched = ctx->use_pitch && pitch_b % (ptrdiff_t)sizeof(T) == 0;
    for (int k = 2; k < NW && pitched; ++k)
        pitched = reinterpret_cast<const char*>(s.wide[k]) - reinterpret_cast<const char*>(s.wide[0]) == k * pitch_b;
    s.wide_pitch = pitched ? pitch_b / (ptrdiff_t)sizeof(T) : 0;
    s.dma_step[0] = (int64_t)pitch_b - 1024;
    s.dma_step[1] = (int64_t)pitch_b + 3072;
    if (pitched) hipLaunchKernelGGL((et_stream_kernel<T, MODE, true, GUARD>), dim3(grid), dim3(kBlock), 0, st, s);
    else hipLaunchKernelGGL((et_stream_kernel<T, MODE, false, GUARD>), dim3(grid), dim3(kBlock), 0, st, s);
    // pixels outside the domain of the production arithmetic (mod16_physics.hpp, "domain
    // guard"): a statically scheduled (small) raster has revisited them inside the kernel; a
    // large one left one flag per piece in its runs' partials for this kernel
#ifndef MOD16_NO_REDO_LAUNCH
    if constexpr (GUARD) if (!g.static_sched) {
        const int64_t groups = (nruns + 63) / 64;
        // a group of 64 runs per wave: both kernels get a block per kBlock runs, the first at most
        // 8 blocks per CU, the second at most 4
        const int cgrid = batch_blocks(ctx, groups * 64);
        const int rgrid = std::min(cgrid, ctx->cus * 4);
        // mixed-precision forms: first the runs' cancellation lists (mod16_mixed.hpp, period_mixed)
        if constexpr (stream_is_mixed(MODE))
            hipLaunchKernelGGL((et_stream_cancel_kernel<T, MODE>), dim3(cgrid), dim3(kBlock), 0, st, s);
        hipLaunchKernelGGL((et_stream_redo_kernel<T, MODE>), dim3(rgrid), dim3(kBlock), 0, st, s);
    }
#endif
    if (ddiag && !fused_final) {
        const double* fin = ws->partial();
        int64_t count = nruns;
        // (a trusted launch has no kernel behind it that looks at every run: the kernel that reads
        // the runs' own partials compares every run's marker)
        bool check = !GUARD && !g.static_sched;
        const unsigned* serial_word = reinterpret_cast<const unsigned*>(ctr) + 3;
        if (count > 4 * kStage) {   // two-level: 1024 fixed slices, then one block
            double* stage = ws->partial() + nruns * kDiag;
            const int64_t per = (count + kStage - 1) / kStage;
            hipLaunchKernelGGL(diag_stage_kernel, dim3(kStage), dim3(kBlock), 0, st, fin, count, per, stage,
                               check ? serial_word : (const unsigned*)nullptr,
                               check ? ctx->status.as<unsigned>() : (unsigned*)nullptr);
            fin = stage;
            count = (count + per - 1) / per;
            check = false;
        }
        hipLaunchKernelGGL(diag_final_fused_kernel, dim3(1), dim3(kFinalBlock), 0, st,
                           fin, (int)count, s.n, ddiag,
                           check ? serial_word : (const unsigned*)nullptr,
                           check ? ctx->status.as<unsigned>() : (unsigned*)nullptr);
    }
    return ws_release(ctx, st);
}

// The totals form (the production step): FAST or, float32, MIXED arithmetic; with
// MOD16_DOMAIN_TRUSTED the instance without the domain test.
template <typename T>
static int launch_totals(mod16_ctx* ctx, const StreamArgs<T>& s, hipStream_t st, double* ddiag, unsigned flags) {
    const bool trusted = (flags & MOD16_DOMAIN_TRUSTED) != 0;
    if constexpr (std::is_same<T, float>::value) {
        if (flags & MOD16_MATH_MIXED)
            return trusted ? launch_stream<T, kStreamTotalsMixed, false>(ctx, s, st, ddiag)
                           : launch_stream<T, kStreamTotalsMixed>(ctx, s, st, ddiag);
    }
    return trusted ? launch_stream<T, kStreamTotals, false>(ctx, s, st, ddiag)
                   : launch_stream<T, kStreamTotals>(ctx, s, st, ddiag);
}

template <typename T> static bool has_rows_or_cols(const EtArgs<T>& a) {
    return (a.row_drv | a.col_drv | a.row_par | a.col_par) != 0u || (a.cls && a.cls_mode != MOD16_BC_DENSE);
}

// ddiag != NULL: also produce the diagnostics vector (device, 8 doubles).
template <typename T>
static int launch_et(mod16_ctx* ctx, EtArgs<T> a, unsigned flags, hipStream_t st,
                     double* ddiag = nullptr) {
    constexpr int V = VecOf<T>::v;
    const bool lut = a.cls != nullptr;
    const bool fast = (flags & MOD16_MATH_EXACT) == 0;
    if (a.n <= 0) return MOD16_OK;
    a.lut = ctx_lut<T>(ctx);
    a.lut64 = ctx->lut64.as<double>();
    a.tab = ctx->tab64.as<double>();
    a.status = ctx->status.as<unsigned>();
    // 16-byte vector path needs every dense pointer 16-byte aligned
    bool aligned = true;
    auto chk = [&](const void* p, size_t al) {
        if (p && (reinterpret_cast<uintptr_t>(p) % al)) aligned = false;
    };
    for (int k = 0; k < 14; ++k) if ((a.dense_drv >> k) & 1u) chk(a.drv[k], 16);
    if (lut) chk(a.cls, V);
    else for (int k = 0; k < 11; ++k) if ((a.dense_par >> k) & 1u) chk(a.par[k], 16);
    bool sep = false;
    for (int k = 0; k < 10; ++k) {
        chk(a.out[k], 16);
        if (k >= 2 && a.out[k]) sep = true;
    }
    const bool dense = a.dense_drv == 0x3fffu;
    // (N,) rows or (T, 1) columns among the inputs: the one-pixel-per-thread kernel
    // indexes them; the vector kernels see plain dense arrays and scalars only
    const int64_t nbody = (aligned && !has_rows_or_cols(a)) ? (a.n / V) * V : 0;
    bool fused_diag = false;
    // dense class rasters with one of the supported output sets take the
    // production pipeline (mod16_stream.hpp), everything else the plain kernel
    int smode = -1;
    if (ctx->use_dma && lut && fast && dense) {
        bool all6 = true, none6 = true;
        for (int k = 2; k < 8; ++k) { all6 = all6 && a.out[k]; none6 = none6 && !a.out[k]; }
        const bool tot = a.out[0] && a.out[1], notot = !a.out[0] && !a.out[1];
        const bool pet = a.out[8] && a.out[9], nopet = !a.out[8] && !a.out[9];
        if (tot && none6 && nopet) smode = kStreamTotals;
        else if (ddiag) smode = -1;      // the fused diagnostics belong to the totals form
        else if (tot && none6 && pet) smode = kStreamPet;
        else if (tot && all6 && nopet) smode = kStreamSep8;
        else if (notot && all6 && nopet) smode = kStreamSep6;
    }
    if (nbody && smode >= 0) {
        StreamArgs<T> s;
        memset(&s, 0, sizeof s);
        for (int k = 0; k < 14; ++k) s.wide[k] = a.drv[k];
        s.bytes[0] = a.cls;
        s.n = nbody;
        int rc;
        if (smode == kStreamTotals) {
            s.out[0] = a.out[0]; s.out[1] = a.out[1];
            fused_diag = ddiag && nbody == a.n;
            rc = launch_totals<T>(ctx, s, st, fused_diag ? ddiag : nullptr, flags);
        } else {
            // float32 rasters: MOD16_MATH_MIXED selects the mixed-precision pixel function
            bool mixed = false;
            if constexpr (std::is_same<T, float>::value) mixed = (flags & MOD16_MATH_MIXED) != 0;
            if (smode == kStreamPet) {
                s.out[0] = a.out[0]; s.out[1] = a.out[1]; s.out[2] = a.out[8]; s.out[3] = a.out[9];
            } else if (smode == kStreamSep8) {
                for (int k = 0; k < 8; ++k) s.out[k] = a.out[k];
            } else {
                for (int k = 0; k < 6; ++k) s.out[k] = a.out[k + 2];
            }
            rc = MOD16_OK;
            if constexpr (std::is_same<T, float>::value) {
                if (mixed) {
                    rc = smode == kStreamPet ? launch_stream<T, kStreamPetMixed>(ctx, s, st)
                         : smode == kStreamSep8 ? launch_stream<T, kStreamSep8Mixed>(ctx, s, st)
                                                : launch_stream<T, kStreamSep6Mixed>(ctx, s, st);
                }
            }
            if (!mixed)
                rc = smode == kStreamPet ? launch_stream<T, kStreamPet>(ctx, s, st)
                     : smode == kStreamSep8 ? launch_stream<T, kStreamSep8>(ctx, s, st)
                                            : launch_stream<T, kStreamSep6>(ctx, s, st);
        }
        if (rc != MOD16_OK) return rc;
    } else if (nbody) {
        EtArgs<T> b = a;
        b.n = nbody;
        // float32 rasters with the FAST (float64) arithmetic: 2 pixels per thread. The
        // 4-pixel instances need ~400 registers; built from the round-1 sources at -O2 / -O3
        // they computed wrong values (which instance goes wrong moves with the
        // scheduler's settings, -O1 is right, today's sources are right) -- they stay unbuilt.
#ifndef MOD16_REPRO_V4
        if (fast && std::is_same<T, float>::value)
            launch_variant<T, 2>(b, lut, fast, sep, dense, grid_for(ctx, nbody / 2), st);
        else
#endif
            launch_variant<T, V>(b, lut, fast, sep, dense, grid_for(ctx, nbody / V), st);
    }
    if (nbody < a.n) {   // ragged tail (or unaligned input): scalar variant
        EtArgs<T> t = a;
        const int64_t off = nbody;
        for (int k = 0; k < 14; ++k) if ((t.dense_drv >> k) & 1u) t.drv[k] += off;
        if (lut) { if (t.cls_mode == MOD16_BC_DENSE) t.cls += off; }
        else for (int k = 0; k < 11; ++k) if ((t.dense_par >> k) & 1u) t.par[k] += off;
        for (int k = 0; k < 10; ++k) if (t.out[k]) t.out[k] += off;
        t.n = a.n - off;
        t.base = a.base + off;
        launch_variant<T, 1>(t, lut, fast, sep, dense, grid_for(ctx, t.n), st);
    }
    HIPCHK(ctx, hipGetLastError());
    if (ddiag && !fused_diag) {
        if (!a.out[0] || !a.out[1]) return fail(ctx, MOD16_ERR_ARG, "diagnostics need both out_day and out_night");
        return reduce_entry<T>(ctx, a.out[0], a.out[1], a.n, nullptr, ddiag, st);
    }
    return MOD16_OK;
}

// dstride / pstride hold a broadcast kind per array: MOD16_BC_SCALAR (0), MOD16_BC_DENSE (1)
// and, with inner > 0 (mod16_et2_*), MOD16_BC_ROW (2) / MOD16_BC_COL (3).
template <typename T>
static int fill_args(mod16_ctx* ctx, EtArgs<T>& a, const uint8_t* cls, const T* const* drivers,
                     const int64_t* dstride, const T* const* params, const int64_t* pstride,
                     int64_t n, T* out_day, T* out_night, T* const* out_sep,
                     T* pet_day = nullptr, T* pet_night = nullptr, int64_t inner = 0,
                     int cls_mode = MOD16_BC_DENSE) {
    if (!ctx) return MOD16_ERR_ARG;
    if (!drivers || !dstride || n < 0) return fail(ctx, MOD16_ERR_ARG, "mod16_et: NULL drivers/strides or n < 0");
    memset(&a, 0, sizeof a);
    const int64_t max_kind = inner > 0 ? MOD16_BC_COL : MOD16_BC_DENSE;
    if (inner > 0 && n % inner != 0) return fail(ctx, MOD16_ERR_ARG, "mod16_et2: n must be a multiple of inner");
    a.inner = inner > 0 ? inner : 1;
    a.base = 0;
    for (int k = 0; k < 14; ++k) {
        if (!drivers[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et: NULL driver array");
        if (dstride[k] < 0 || dstride[k] > max_kind) return fail(ctx, MOD16_ERR_ARG, "mod16_et: driver stride must be 0 or 1 (mod16_et2: a MOD16_BC_* kind)");
        a.drv[k] = drivers[k];
        if (dstride[k] == MOD16_BC_DENSE) a.dense_drv |= 1u << k;
        if (dstride[k] == MOD16_BC_ROW) a.row_drv |= 1u << k;
        if (dstride[k] == MOD16_BC_COL) a.col_drv |= 1u << k;
    }
    a.cls = cls;
    a.cls_mode = (uint32_t)cls_mode;
    if (cls) {
        if (!ctx->have_lut) return fail(ctx, MOD16_ERR_NO_BPLUT, "mod16_et: class raster given but mod16_set_bplut_f64 was not called");
        if (cls_mode < 0 || cls_mode > max_kind) return fail(ctx, MOD16_ERR_ARG, "mod16_et2: bad broadcast kind of the class raster");
    } else {
        if (!params || !pstride) return fail(ctx, MOD16_ERR_ARG, "mod16_et: neither a class raster nor parameter arrays given");
        for (int k = 0; k < 11; ++k) {
            if (!params[k]) return fail(ctx, MOD16_ERR_ARG, "mod16_et: NULL parameter array");
            if (pstride[k] < 0 || pstride[k] > max_kind) return fail(ctx, MOD16_ERR_ARG, "mod16_et: parameter stride must be 0 or 1 (mod16_et2: a MOD16_BC_* kind)");
            a.par[k] = params[k];
            if (pstride[k] == MOD16_BC_DENSE) a.dense_par |= 1u << k;
            if (pstride[k] == MOD16_BC_ROW) a.row_par |= 1u << k;
            if (pstride[k] == MOD16_BC_COL) a.col_par |= 1u << k;
        }
    }
    a.out[0] = out_day;
    a.out[1] = out_night;
    bool any = out_day || out_night;
    if (out_sep)
        for (int k = 0; k < 6; ++k) {
            a.out[2 + k] = out_sep[k];
            any = any || out_sep[k];
        }
    a.out[8] = pet_day;
    a.out[9] = pet_night;
    any = any || pet_day || pet_night;
    if (!any) return fail(ctx, MOD16_ERR_ARG, "mod16_et: no output array given");
    a.n = n;
    return MOD16_OK;
}

static int read_status(mod16_ctx* ctx, hipStream_t st) {
    const unsigned* host = ctx->status_host.as<unsigned>();
    HIPCHK(ctx, hipMemcpyAsync(ctx->status_host.get(), ctx->status.get(), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->status.get(), 0, sizeof(unsigned), st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (*host & kStatusIncomplete)
        return fail(ctx, MOD16_ERR_HIP, "a launch processed only part of its raster: it found its ticket counter in use "
                                        "(an earlier launch on this context ended abnormally, or more launches were in "
                                        "flight than the context has counters) -- the outputs of that step are not valid");
    if (*host & kStatusClassRange)
        return fail(ctx, MOD16_ERR_CLASS_RANGE, "class raster holds a code >= 13 (numpy would raise IndexError)");
    return MOD16_OK;
}

// A chain of kernel launches on one stream, captured and instantiated once and kept under a key (what
// the kernels' arguments hold: the draws of an objective graph, the steps of a sampler graph; a
// captured forward step has none). Owns the graph and its executable.
struct CachedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int64_t key = -1;
    CachedGraph() = default;
    CachedGraph(const CachedGraph&) = delete;
    CachedGraph& operator=(const CachedGraph&) = delete;
    ~CachedGraph() { drop(); }
    void drop() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
        key = -1;
    }
    // what `enqueue()` launches on `st` becomes the graph; the capture is always ended before a failed
    // launch is reported
    template <typename F>
    int capture(mod16_ctx* ctx, hipStream_t st, int64_t k, F enqueue) {
        drop();
        HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        enqueue();
        const hipError_t launched = hipGetLastError();
        const hipError_t ended = hipStreamEndCapture(st, &graph);
        HIPCHK(ctx, launched);
        HIPCHK(ctx, ended);
        HIPCHK(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        key = k;
        return MOD16_OK;
    }
};

// ---- the forward run + diagnostics of one raster as a HIP graph: the launch
// sequence of mod16_et_diag_* (counter reset, pipeline kernel, staged fixed-order
// sum) captured once and replayed with one call per time step.
// (Members go in reverse order of declaration: the captured graph before the memory its nodes point into.)
struct mod16_graph {
    mod16_ctx* ctx = nullptr;                // NULL once the context has been destroyed (graph_registry_mu); a view
    int device = 0;
    DevMem counter;                          // its own ticket counter: replays never meet the ring
    DiagWs ws;                               // its own diagnostics workspace (freed with the graph)
    CachedGraph cg;                          // the captured step
};
static void graph_register(mod16_ctx* ctx, mod16_graph* g) {
    std::lock_guard<std::mutex> lock(graph_registry_mu());
    ctx->graphs.push_back(g);
}
// false: the context the graph was captured with is gone (its tables with it)
static bool graph_alive(const mod16_graph* g) {
    std::lock_guard<std::mutex> lock(graph_registry_mu());
    return g->ctx != nullptr;
}


// ------------------------------------------------------------- diagnostics
template <typename T>
static int reduce_entry(mod16_ctx* ctx, const T* day, const T* night, int64_t n, double* diag,
                        double* ddiag, void* stream) {
    if (!ctx || !day || !night || n < 0) return fail(ctx, MOD16_ERR_ARG, "mod16_reduce_diag: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kDiagBlocks, (n + kBlock - 1) / kBlock));
    DiagWs* ws = nullptr;
    int rc = reserve_diag(ctx, blocks, &ws);
    if (rc != MOD16_OK) return rc;
    rc = ws_acquire(ctx, st);
    if (rc != MOD16_OK) return rc;
    hipLaunchKernelGGL((diag_partial_kernel<T>), dim3(blocks), dim3(kBlock), 0, st, day, night, n, ws->partial());
    double* dst = ddiag ? ddiag : ctx->diag_dev.as<double>();
    hipLaunchKernelGGL(diag_final_kernel, dim3(1), dim3(kBlock), 0, st, ws->partial(), blocks, dst);
    HIPCHK(ctx, hipGetLastError());
    rc = ws_release(ctx, st);
    if (rc != MOD16_OK) return rc;
    if (diag) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->diag_host.get(), dst, sizeof(double) * kDiag, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        memcpy(diag, ctx->diag_host.get(), sizeof(double) * kDiag);
    }
    return MOD16_OK;
}


// ---------------------------------------------------------------- generator
// tile (pixels) -> log2, or -1 if it is not a power of two >= lo
static int tile_log2(int64_t tile, int64_t lo) {
    if (tile < lo || (tile & (tile - 1)) != 0) return -1;
    int sh = 0;
    while ((int64_t(1) << sh) < tile) ++sh;
    return sh;
}


