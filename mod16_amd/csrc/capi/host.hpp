// libmod16hip.so, host side: the HOST mode (host arrays in, host arrays out) of the pixel-wise
// families -- mod16_et_* / mod16_et2_* / mod16_et_pet_* / mod16_et_hdiag_* (forward.hip),
// mod16_et_raw_* (raw.hip), mod16_method_* (methods.hip), mod16_et_static_* (calibration.hip). A family
// describes the arrays of one call (HostPlan) and enqueues one tile's kernels (a callback); the two
// paths here do everything else: host_small (small calls, no copy commands) and host_tiled (tiles
// staged through the context's slabs).
#pragma once
#include "internal.hpp"

namespace {
constexpr int64_t kTilePixels = int64_t(1) << 21;   // HOST mode: pixels per staged tile
constexpr size_t kStagger = 33 * 1024;              // see RasterEngine.STAGGER_BYTES
constexpr int kSmallUnavailable = 1;                // host_small: no page-locked buffer -- the caller stages the call
constexpr int kHostMaxArrays = 40;
enum HostKind {
    kIn,         // per pixel, staged tile by tile
    kOut,        // per pixel, copied back tile by tile
    kScalar,     // one value, in the scalar block: index x size, within its 256 bytes
    kResident,   // a device copy the family uploaded itself, whole (mod16_et2_*'s (N,) and (T, 1) inputs)
};
}  // namespace

// The arrays of one HOST-mode call in slab order: the T-sized arrays first (per_arr apart, so the 14
// drivers -- and raw's per-pixel day_hours -- stay equally spaced and the pipeline takes its pitched
// instance), the byte rasters behind them. An absent optional array keeps its place (host = NULL)
// and reaches the kernel as NULL.
// An array may consist of several ROWS of n pixels each (the time slabs of a composite's drivers, the
// periods of its outputs: composite.hip): `pitch` host elements apart, and in the slab back to back
// (`row` bytes apart = HostTile::row_bytes, no stagger between them: the stagger separates ARRAYS;
// the rows of a byte array HostTile::byte_row_bytes apart: gapfill.hip).
// Every array of the other families has one row: their offsets are what they were.
struct HostPlan {
    struct Array { void* host; void* dev; int elem; int kind; int rows; int64_t pitch; int first; };
    Array a[kHostMaxArrays];
    int count = 0, nwide = 0;
    int wide_rows = 0, byte_rows = 0;  // places of the slab's two regions
    int elem;                          // sizeof(T)
    const uint8_t* cls = nullptr;      // the class raster: the small path checks its codes on the host
    explicit HostPlan(int elem_) : elem(elem_) {}
    // elem_size: an array of another element type than T in a T-sized place (0: T, or a byte)
    void add(int kind, const void* host, bool bytes = false, int rows = 1, int64_t pitch = 0, int elem_size = 0) {
        int& region = bytes ? byte_rows : wide_rows;
        a[count++] = Array{const_cast<void*>(host), nullptr, elem_size ? elem_size : (bytes ? 1 : elem), kind, rows, pitch, region};
        region += rows;
        if (!bytes) ++nwide;
    }
    // per_arr: from one T-sized array to the next when both have one row; row: what every further row adds
    size_t offset(int i, size_t per_arr, size_t per_b, size_t row = 0) const {
        const size_t wide = per_arr * nwide + row * (wide_rows - nwide);
        if (i >= count) return wide + per_b * byte_rows;
        return i < nwide ? per_arr * i + row * (a[i].first - i) : wide + per_b * a[i].first;
    }
    void put_scalars(char* block) const {
        for (int i = 0; i < count; ++i)
            if (a[i].host && a[i].kind == kScalar) memcpy(block + a[i].elem * i, a[i].host, a[i].elem);
    }
    // device address of array i: its slot of the slab (or buffer), the scalar block, its resident copy
    void* where(int i, char* slot, char* scalars) const {
        if (!a[i].host) return nullptr;
        return a[i].kind == kScalar ? scalars + a[i].elem * i : a[i].kind == kResident ? a[i].dev : slot;
    }
};

// The tile of a HOST-mode call whose arrays have many rows: a slot's slab -- `wide_rows` rows of esz
// bytes and `byte_rows` byte rows per pixel, the stagger once per T-sized array -- fits stage_bytes
// (whole blocks of pixels, at least one, at most kTilePixels).
static int64_t stage_tile(const HostPlan& p, size_t esz, int64_t stage_bytes) {
    const int64_t fixed = (int64_t)p.nwide * (int64_t)kStagger + 512;
    const int64_t per_pixel = (int64_t)p.wide_rows * (int64_t)esz + p.byte_rows;
    const int64_t tile = (stage_bytes - fixed) / per_pixel / kBlock * kBlock;
    return std::max<int64_t>(kBlock, std::min<int64_t>(tile, kTilePixels));
}

// ---- the argument checks the array families share (gapfill.hip, zonal.hip, daynight.hip) ----
// -> NULL, or what is wrong with `where`
static const char* check_where(int where) {
    return where != MOD16_DEVICE && where != MOD16_HOST ? "`where` must be MOD16_HOST or MOD16_DEVICE" : nullptr;
}
// ... or with stage_bytes, the device memory a HOST-mode call may stage through (0: stage_budget's default)
static const char* check_where_stage(int where, size_t stage_bytes) {
    if (const char* what = check_where(where)) return what;
    return stage_bytes > (size_t)std::numeric_limits<int64_t>::max() ? "stage_bytes is out of range" : nullptr;
}
static int64_t stage_budget(size_t stage_bytes) { return stage_bytes ? (int64_t)stage_bytes : (int64_t)128 << 20; }

// The bytes an argument spans: `planes` planes of `rows` rows of n elements of `elem` bytes, rows
// `pitch` and planes `plane` elements apart.
struct Extent { uintptr_t lo, hi; };
static Extent extent(const void* p, int64_t planes, int64_t plane, int64_t rows, int64_t pitch, int64_t n, size_t elem) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Extent{lo, lo + (uintptr_t)(((planes - 1) * plane + (rows - 1) * pitch + n) * (int64_t)elem)};
}
// ... one dense row of n elements
static Extent extent(const void* p, int64_t n, size_t elem) { return extent(p, 1, 0, 1, 0, n, elem); }
// In place is refused: does an output share a byte with an input or with an earlier output?
static bool overlaps(const Extent* outs, int no, const Extent* ins, int ni) {
    auto meet = [](const Extent& a, const Extent& b) { return a.lo < b.hi && b.lo < a.hi; };
    for (int o = 0; o < no; ++o) {
        for (int i = 0; i < ni; ++i)
            if (meet(outs[o], ins[i])) return true;
        for (int o2 = 0; o2 < o; ++o2)
            if (meet(outs[o], outs[o2])) return true;
    }
    return false;
}

// What a family's callback gets: the device address of every array of the plan for this tile (plan
// order), its pixels, the stream; it enqueues the tile's kernels and returns a status.
struct HostTile {
    void* dev[kHostMaxArrays];
    int64_t m, off;      // pixels of the tile, its first pixel in the call
    size_t row_bytes;    // between two rows of a T-sized array with several (host_tiled)
    size_t byte_row_bytes;   // ... of a byte array
    hipStream_t st;
    double* diag;        // host_tiled with tile_diag: where this tile's diagnostics vector goes (device)
};

// The page-locked buffer of the small calls: 256 bytes of scalars, `arrays` arrays of `elem`-byte
// values and up to three of bytes behind them, for n pixels. It grows with the largest call seen
// (powers of two from 1024 pixels: a caller of scalars pins 0.3 MB, one of 256 x 256 windows 18 MB).
// Also makes sure of streams[0]. -> false: no page-locked memory to be had (the context stops
// asking: its calls are staged from now on).
static bool small_reserve(mod16_ctx* ctx, int64_t n, size_t elem, int arrays, size_t* per_arr) {
    int64_t cap = 1024;
    while (cap < n) cap *= 2;
    *per_arr = (size_t)cap * elem;
    const size_t need = 256 + *per_arr * arrays + 3 * (size_t)cap + 256;
    bool ok = true;
    if (ctx->small_host.bytes() < need)
        ok = ctx->small_host.alloc(ctx, need, "page-locked memory for the small calls' buffer") == MOD16_OK &&
             hipHostGetDevicePointer(&ctx->small_dev, ctx->small_host.get(), 0) == hipSuccess;
    ok = ok && ctx->streams[0].ensure() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ctx->small_host.release();
        ctx->small_dev = nullptr;
        ctx->small_pixels = 0;
    }
    return ok;
}

// HOST mode, small calls. The staged path costs a dozen copy commands whatever the size (each
// dense input its own, pageable memory: the runtime stages and waits), a status read-back and
// three synchronisations -- 64 us for ONE pixel, where the reference's numpy takes 86 us for its
// whole forward run (BASELINE.json configs[0]: a flux-tower site), ~290 us up to 16 k pixels.
// Measured against it (tools/smallcall.py, profiles/r05_small_calls.jsonl): 18 us against 64 for one
// pixel, 102 against 273 at 100 x 100, 371 against 420 at 256 x 256, even at ~90 k pixels, slower
// beyond (the CPU's copies into the buffer grow faster than the runtime's DMA): kSmallPixels.
// Here the CPU copies the inputs into one page-locked buffer, the kernel reads them from there and
// writes its outputs there (host memory is in the device's address space: a few KB over the link),
// and the CPU copies the outputs on: one launch sequence, one synchronisation, the same kernels on
// the same values -- the same bits as the staged path gives. Class codes are checked here instead of
// by the kernel (the staged path reads the kernel's status word back).
// pad: whole 16-byte vectors -- a ragged end would cost a second launch (the one-pixel-per-thread
// kernel behind the vector kernel); the buffer has the room, the pad pixels repeat the last pixel
// (so they are no new case for the domain guard), and their outputs stay in the buffer.
template <typename Launch>
static int host_small(mod16_ctx* ctx, const HostPlan& p, int64_t n, bool pad, Launch&& launch) {
    size_t per_arr = 0;
    if (!small_reserve(ctx, n, p.elem, p.nwide, &per_arr)) return kSmallUnavailable;
    if (p.cls)
        for (int64_t i = 0; i < n; ++i)
            if (p.cls[i] >= MOD16_N_CLASSES)
                return fail(ctx, MOD16_ERR_CLASS_RANGE, "class raster holds a code >= 13 (numpy would raise IndexError)");
    char* hb = ctx->small_host.as<char>();
    char* db = static_cast<char*>(ctx->small_dev);
    const size_t cap = per_arr / p.elem;           // the buffer's capacity in pixels
    auto at = [&](int i) { return 256 + p.offset(i, per_arr, cap); };
    const int64_t V = 16 / p.elem;
    const int64_t npad = pad ? (n + V - 1) / V * V : n;
    p.put_scalars(hb);                             // the scalars in the first 256 bytes
    HostTile t;
    t.m = npad;
    t.off = 0;
    t.row_bytes = per_arr;
    t.byte_row_bytes = cap;
    t.st = ctx->streams[0];
    t.diag = nullptr;
    for (int i = 0; i < p.count; ++i) {
        const HostPlan::Array& x = p.a[i];
        t.dev[i] = p.where(i, db + at(i), db);
        if (!x.host || x.kind != kIn) continue;
        memcpy(hb + at(i), x.host, x.elem * n);
        for (int64_t j = n; j < npad; ++j) memcpy(hb + at(i) + x.elem * j, static_cast<const char*>(x.host) + x.elem * (n - 1), x.elem);
    }
    int rc = launch(t);
    if (rc != MOD16_OK) return rc;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(t.st));
    for (int i = 0; i < p.count; ++i)
        if (p.a[i].host && p.a[i].kind == kOut) memcpy(p.a[i].host, hb + at(i), p.a[i].elem * n);
    return MOD16_OK;
}

// The context's staging slabs hold at least `need` bytes each (they grow together: all are released,
// the slots in use get new ones) and slots [0, nslots) have their slab and their stream.
static int reserve_slabs(mod16_ctx* ctx, size_t need, int nslots) {
    if (ctx->slab_bytes < need) {
        for (int s = 0; s < kSlots; ++s) ctx->slab[s].release();
        ctx->slab_bytes = need;
    }
    for (int s = 0; s < nslots; ++s) {
        if (!ctx->slab[s]) {
            int rc = ctx->slab[s].alloc(ctx, ctx->slab_bytes, "HOST mode: device memory for a staging slab");
            if (rc != MOD16_OK) return rc;
        }
        HIPCHK(ctx, ctx->streams[s].ensure());
    }
    return MOD16_OK;
}

// HOST mode: tiles of kTilePixels staged through the context's slabs, one host thread and one stream
// per slot, tile t on slot t % nslots (nslots <= max_slots). The copies from and to pageable memory
// are what bounds this mode (the HIP runtime stages them through its own pinned buffers on the
// calling thread), so the slots run them concurrently; kernel launches are serialised (they share the
// context's workspace). pipeline: the callback may launch the production pipeline -- its workspace is
// reserved at its final size before any thread launches, and the status word is read back at the end.
// tile_diag: one diagnostics vector per tile (host, 8 doubles each), reduced by the callback into
// HostTile::diag while the tile's outputs are on the device.
// tile_pixels: a family whose arrays have many rows cuts the tile so that a slot's slab keeps its size.
// A row of an array is one copy command per tile.
template <typename Launch>
static int host_tiled(mod16_ctx* ctx, const HostPlan& p, int64_t n, int max_slots, bool pipeline,
                      Launch&& launch, double* tile_diag = nullptr, int64_t tile_pixels = kTilePixels) {
    const int64_t tile = std::min<int64_t>(n, tile_pixels);
    const int64_t ntiles = (n + tile - 1) / tile;
    const int nslots = (int)std::min<int64_t>(ntiles, max_slots);
    if (nslots > 1) ctx->ws_multi = true;       // one stream per slot: the launches leave their events (ws_release)
    // successive staged arrays are kStagger bytes apart on top of their size
    const size_t row = ((size_t)tile * p.elem + 255) / 256 * 256;
    const size_t per_arr = row + kStagger;
    const size_t per_b = ((size_t)tile + 255) / 256 * 256;
    int rc = reserve_slabs(ctx, p.offset(p.count, per_arr, per_b, row) + 256, nslots);
    if (rc != MOD16_OK) return rc;
    // broadcast scalars live in one small device array
    char hs[256] = {};
    p.put_scalars(hs);
    HIPCHK(ctx, hipMemcpy(ctx->scalars.get(), hs, sizeof hs, hipMemcpyHostToDevice));
    char* dscal = ctx->scalars.as<char>();
    if (pipeline) {   // the kernels' shared workspace at its final size before any thread launches
        const int64_t npiece = (tile / (16 / p.elem) + 63) / 64;
        rc = reserve_diag(ctx, npiece / 2 + 2048);
        if (rc != MOD16_OK) return rc;
    }
    auto stage = [&](int slot, int64_t off) -> int {
        char* base = ctx->slab[slot].as<char>();
        HostTile t;
        t.m = std::min(tile, n - off);
        t.off = off;
        t.row_bytes = row;
        t.byte_row_bytes = per_b;
        t.st = ctx->streams[slot];
        t.diag = tile_diag ? ctx->hdiag_dev.as<double>() + (size_t)slot * kDiag : nullptr;
        for (int i = 0; i < p.count; ++i) {
            const HostPlan::Array& x = p.a[i];
            t.dev[i] = p.where(i, base + p.offset(i, per_arr, per_b, row), dscal);
            const size_t step = i < p.nwide ? row : per_b;      // between the rows of this array in the slab
            if (x.host && x.kind == kIn)
                for (int r = 0; r < x.rows; ++r)
                    HIPCHK(ctx, hipMemcpyAsync(static_cast<char*>(t.dev[i]) + step * r,
                                               static_cast<const char*>(x.host) + x.elem * (x.pitch * r + off), x.elem * t.m,
                                               hipMemcpyHostToDevice, t.st));
        }
        {
            std::lock_guard<std::mutex> lock(ctx->launch_mu);
            int rc = launch(t);
            if (rc != MOD16_OK) return rc;
            HIPCHK(ctx, hipGetLastError());
        }
        for (int i = 0; i < p.count; ++i) {
            const HostPlan::Array& x = p.a[i];
            const size_t step = i < p.nwide ? row : per_b;
            if (x.host && x.kind == kOut)
                for (int r = 0; r < x.rows; ++r)
                    HIPCHK(ctx, hipMemcpyAsync(static_cast<char*>(x.host) + x.elem * (x.pitch * r + off),
                                               static_cast<const char*>(t.dev[i]) + step * r, x.elem * t.m,
                                               hipMemcpyDeviceToHost, t.st));
        }
        if (t.diag) HIPCHK(ctx, hipMemcpyAsync(tile_diag + off / tile * kDiag, t.diag, sizeof(double) * kDiag, hipMemcpyDeviceToHost, t.st));
        HIPCHK(ctx, hipStreamSynchronize(t.st));      // the slab of this slot is free again
        return MOD16_OK;
    };
    if (nslots == 1) {
        for (int64_t off = 0; off < n; off += tile) {
            int rc = stage(0, off);
            if (rc != MOD16_OK) return rc;
        }
    } else {
        int rcs[kSlots] = {};
        std::vector<std::thread> workers;
        for (int s = 0; s < nslots; ++s)
            workers.emplace_back([&, s]() {
                if (hipSetDevice(ctx->device) != hipSuccess) { rcs[s] = MOD16_ERR_HIP; return; }
                for (int64_t t = s; t < ntiles && rcs[s] == MOD16_OK; t += nslots) rcs[s] = stage(s, t * tile);
            });
        for (auto& w : workers) w.join();
        for (int s = 0; s < nslots; ++s)
            if (rcs[s] != MOD16_OK) return rcs[s];
    }
    return pipeline ? read_status(ctx, ctx->streams[0]) : MOD16_OK;
}
