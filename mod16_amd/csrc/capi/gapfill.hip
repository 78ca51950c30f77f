// libmod16hip.so -- QC-driven temporal gap filling of byte series: mod16_gapfill_u8 (the annual fPAR / LAI profile of every pixel filled in one launch: interpolated, held, fallback)
#include "host.hpp"
#include "../mod16_gapfill.hpp"

namespace {
// the package's default table for MOD15A2H's FparLai_QC (mod16_amd/gapfill.py: default_good)
bool gap_default_good(int q) {
    const int cloud = (q >> 3) & 3;
    return !(q & 1) && !(q & 4) && (cloud == 0 || cloud == 3) && (q >> 5) <= 1;
}
size_t gap_out_size(int out_type) { return out_type == MOD16_GAPFILL_U8 ? 1 : out_type == MOD16_GAPFILL_F32 ? 4 : 8; }
}  // namespace

// All pointers are device pointers here (a.good may be NULL: the table travels in a.good_bits).
template <typename OUT>
static int launch_gapfill_as(mod16_ctx* ctx, GapArgs a, int nf, hipStream_t st) {
    constexpr int PX = GapPx<OUT>::v;
    // vector access: every row of an argument starts on a multiple of the vector size
    auto aligned = [](const void* p, int64_t pitch_bytes, size_t to) {
        return !p || (reinterpret_cast<uintptr_t>(p) % to == 0 && (size_t)pitch_bytes % to == 0);
    };
    a.wide = 0;
    bool in = aligned(a.qc, a.qc_pitch, PX);
    bool out = true;
    for (int f = 0; f < nf; ++f) {
        in = in && aligned(a.field[f], a.in_pitch, PX);
        out = out && aligned(a.out[f], a.out_pitch * (int64_t)sizeof(OUT), 16);
    }
    if (in) a.wide |= kGapWideIn;
    if (out) a.wide |= kGapWideOut;
    if (aligned(a.source, a.src_pitch, PX)) a.wide |= kGapWideSrc;
    const int64_t lanes = (a.n + PX - 1) / PX;
    const int64_t grid = (lanes + kBlock - 1) / kBlock;
    if (grid > 0x7fffffff) return fail(ctx, MOD16_ERR_ARG, "mod16_gapfill: n is too large for one launch");
    if (nf == 1) hipLaunchKernelGGL((gapfill_kernel<OUT, 1>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    else if (nf == 2) hipLaunchKernelGGL((gapfill_kernel<OUT, 2>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((gapfill_kernel<OUT, 3>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

static int launch_gapfill(mod16_ctx* ctx, const GapArgs& a, int nf, int out_type, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    if (out_type == MOD16_GAPFILL_U8) return launch_gapfill_as<uint8_t>(ctx, a, nf, st);
    if (out_type == MOD16_GAPFILL_F32) return launch_gapfill_as<float>(ctx, a, nf, st);
    return launch_gapfill_as<double>(ctx, a, nf, st);
}

// HOST mode: the slabs of the outputs (the plan's wide arrays: elements of the output type), of the
// fields, the QC layer and the source bytes, and the fallback rows, through the shared staging path;
// the tile cut so that a slot's slab fits stage_bytes
static int gapfill_host(mod16_ctx* ctx, const GapArgs& a, int nf, int out_type, int64_t stage_bytes) {
    const int S = a.slabs;
    const size_t esz = gap_out_size(out_type);
    HostPlan p((int)esz);
    for (int f = 0; f < kGapMaxFields; ++f) p.add(kOut, f < nf ? a.out[f] : nullptr, false, f < nf ? S : 1, a.out_pitch);
    for (int f = 0; f < kGapMaxFields; ++f) p.add(kIn, f < nf ? a.field[f] : nullptr, true, f < nf ? S : 1, a.in_pitch);
    p.add(kIn, a.qc, true, a.qc ? S : 1, a.qc_pitch);
    for (int f = 0; f < kGapMaxFields; ++f) p.add(kIn, a.fallback[f], true);
    p.add(kOut, a.source, true, a.source ? nf * S : 1, a.src_pitch);
    auto launch = [&](const HostTile& t) {
        GapArgs d = a;
        d.n = t.m;
        d.good = nullptr;               // (the host's table: in d.good_bits)
        for (int f = 0; f < kGapMaxFields; ++f) {
            d.out[f] = t.dev[f];
            d.field[f] = static_cast<const uint8_t*>(t.dev[kGapMaxFields + f]);
            d.fallback[f] = static_cast<const uint8_t*>(t.dev[2 * kGapMaxFields + 1 + f]);
        }
        d.qc = static_cast<const uint8_t*>(t.dev[2 * kGapMaxFields]);
        d.source = static_cast<uint8_t*>(t.dev[3 * kGapMaxFields + 1]);
        d.out_pitch = (int64_t)(t.row_bytes / esz);
        d.in_pitch = d.qc_pitch = d.src_pitch = (int64_t)t.byte_row_bytes;
        return launch_gapfill(ctx, d, nf, out_type, t.st);
    };
    return host_tiled(ctx, p, a.n, ctx->host_threads, false, launch, nullptr, stage_tile(p, esz, stage_bytes));
}

extern "C" int mod16_gapfill_u8(mod16_ctx* ctx, const mod16_gapfill_spec* spec, const uint8_t* const* fields,
                                const uint8_t* qc, const uint8_t* good256, const uint8_t* const* fallback,
                                void* const* out, uint8_t* source, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_gapfill: ", what); };
    if (!spec || !fields || !out) return bad("NULL spec, fields or out");
    if (spec->n < 0) return bad("n < 0");
    if (spec->slabs < 1 || spec->slabs > kGapMaxSlabs) return bad("slabs must be between 1 and 4096");
    if (spec->nfields < 1 || spec->nfields > kGapMaxFields) return bad("nfields must be between 1 and 3");
    if (spec->out_type != MOD16_GAPFILL_U8 && spec->out_type != MOD16_GAPFILL_F32 && spec->out_type != MOD16_GAPFILL_F64)
        return bad("out_type must be MOD16_GAPFILL_U8, MOD16_GAPFILL_F32 or MOD16_GAPFILL_F64");
    if (spec->max_gap < -1) return bad("max_gap must be -1 (none) or at least 0");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int nf = spec->nfields, S = spec->slabs;
    const int64_t n = spec->n;
    const size_t esz = gap_out_size(spec->out_type);
    for (int f = 0; f < nf; ++f) {
        if (!fields[f] || !out[f]) return bad("NULL field or output array");
        if (spec->out_type != MOD16_GAPFILL_U8 && !std::isfinite(spec->scale[f])) return bad("scale must be finite");
    }
    if (spec->in_pitch < n || spec->out_pitch < n) return bad("in_pitch and out_pitch must be at least n");
    if (qc && spec->qc_pitch < n) return bad("qc_pitch must be at least n");
    if (source && spec->source_pitch < n) return bad("source_pitch must be at least n");
    if (n == 0) return MOD16_OK;
    // in place is refused: no output may share a byte with an input or with another output
    {
        Extent ins[2 * kGapMaxFields + 2], outs[kGapMaxFields + 1];
        int ni = 0, no = 0;
        for (int f = 0; f < nf; ++f) {
            ins[ni++] = extent(fields[f], 1, 0, S, spec->in_pitch, n, 1);
            if (fallback && fallback[f]) ins[ni++] = extent(fallback[f], n, 1);
            outs[no++] = extent(out[f], 1, 0, S, spec->out_pitch, n, esz);
        }
        if (qc) ins[ni++] = extent(qc, 1, 0, S, spec->qc_pitch, n, 1);
        if (good256) ins[ni++] = extent(good256, 256, 1);
        if (source) outs[no++] = extent(source, 1, 0, (int64_t)nf * S, spec->source_pitch, n, 1);
        if (overlaps(outs, no, ins, ni)) return bad("an output overlaps an input or another output");
    }
    GapArgs a;
    memset(&a, 0, sizeof a);
    for (int f = 0; f < nf; ++f) {
        a.field[f] = fields[f];
        a.fallback[f] = fallback ? fallback[f] : nullptr;
        a.out[f] = out[f];
        a.scale[f] = spec->out_type == MOD16_GAPFILL_U8 ? 1.0 : spec->scale[f];
    }
    a.qc = qc;
    a.source = source;
    a.n = n;
    a.in_pitch = spec->in_pitch;
    a.qc_pitch = qc ? spec->qc_pitch : 0;
    a.out_pitch = spec->out_pitch;
    a.src_pitch = source ? spec->source_pitch : 0;
    a.slabs = S;
    a.max_gap = spec->max_gap < 0 ? kGapMaxSlabs + 1 : std::min(spec->max_gap, kGapMaxSlabs + 1);
    // the table as bits: the default, or (HOST mode) the caller's; a device table is read by the kernel
    for (int q = 0; q < 256; ++q) {
        const bool g = (good256 && where == MOD16_HOST) ? good256[q] != 0 : gap_default_good(q);
        if (g) a.good_bits[q >> 5] |= 1u << (q & 31);
    }
    a.good = where == MOD16_DEVICE ? good256 : nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_gapfill(ctx, a, nf, spec->out_type, static_cast<hipStream_t>(stream));
    return gapfill_host(ctx, a, nf, spec->out_type, stage_budget(stage_bytes));
}
