// libmod16hip.so, host side: the grid handle of the downscaled families (downscale.hip creates and
// destroys it; downscale.hip and composite_downscale.hip launch with it and, in HOST mode, upload
// their coarse arrays beside it).
#pragma once
#include "host.hpp"
#include "../mod16_downscale.hpp"

// The corner tables of both axes on the device (mod16_amd/downscale.py: corner_tables) -- or, in the
// row-affine geometry (mod16_downscale_create_rows*: corner_tables_rows), the row tables and the
// per-row (origin, scale) of the columns. The geometry picks the kernel instance at launch.
struct mod16_downscale {
    int device = 0;
    mod16_downscale_spec spec = {};
    DevMem tables;               // ri0, ri1 (int32 [R]), rw0, rw1 (double [R]), the same four for the columns;
                                 // row-affine: ri0, ri1, rw0, rw1, origin, scale (double [R])
    bool affine = false;         // true: `gr` holds the views, false: `g`
    DsGrid g = {};               // views into `tables`
    DsRowsGrid gr = {};
};

// -> f(the handle's geometry): a DsRowsGrid or a DsGrid, which picks the kernel instances in f
template <typename F> static auto ds_dispatch(const mod16_downscale* grid, F&& f) {
    if (grid->affine) return f(grid->gr);
    return f(grid->g);
}

// HOST mode: the coarse arrays of a call (ptrs[k] != NULL: slabs[k] planes, tstride[k] host elements
// apart, rows cpitch apart; slabs NULL: one plane each) uploaded whole, once, planes and rows back
// to back (pitch = coarse_cols, time stride = a plane), into the context's buffer for resident
// inputs; dev[k] receives the address of its first plane. label: what the allocation holds
template <typename T>
static int upload_coarse(mod16_ctx* ctx, const mod16_downscale* grid, const T* const* ptrs, const int* slabs,
                         const int64_t* tstride, int64_t cpitch, int count, const char* label, const T** dev) {
    const size_t H = (size_t)grid->spec.coarse_rows, W = (size_t)grid->spec.coarse_cols;
    const size_t plane = H * W * sizeof(T);
    auto bytes = [&](int k) { return align256(plane * (size_t)(slabs ? slabs[k] : 1)); };
    size_t total = 256;
    for (int k = 0; k < count; ++k)
        if (ptrs[k]) total += bytes(k);
    char what[96];
    snprintf(what, sizeof what, "HOST mode: device memory for the %s", label);
    int rc = ctx->bc_buf.reserve(ctx, total, what);
    if (rc != MOD16_OK) return rc;
    char* cur = ctx->bc_buf.as<char>();
    // (one copy per plane where its rows lie back to back, else one per row: a plane has a few hundred)
    const bool packed = (size_t)cpitch == W;
    const size_t rows = packed ? 1 : H, row_bytes = (packed ? H : 1) * W * sizeof(T);
    for (int k = 0; k < count; ++k) {
        dev[k] = nullptr;
        if (!ptrs[k]) continue;
        for (int s = 0; s < (slabs ? slabs[k] : 1); ++s) {
            const T* from = ptrs[k] + (s ? (int64_t)s * tstride[k] : 0);
            char* to = cur + (size_t)s * plane;
            for (size_t r = 0; r < rows; ++r)
                if (hipMemcpy(to + r * W * sizeof(T), from + r * (size_t)cpitch, row_bytes, hipMemcpyHostToDevice) != hipSuccess)
                    return fail(ctx, MOD16_ERR_HIP, "HOST mode: upload of a coarse plane failed");
        }
        dev[k] = reinterpret_cast<const T*>(cur);
        cur += bytes(k);
    }
    return MOD16_OK;
}
