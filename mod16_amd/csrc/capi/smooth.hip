// libmod16hip.so -- Whittaker smoothing of 8-day series, weighted by QC: mod16_smooth_u8 / _f32 / _f64 (the banded solve of every pixel's profile in one launch, with upper-envelope passes)
#include "host.hpp"
#include "../mod16_smooth.hpp"

namespace {
constexpr size_t kSmoothTableBytes = 256 * sizeof(double);      // head of the workspace: a HOST-mode call's weight table
constexpr int64_t kSmoothBudget = (int64_t)256 << 20;           // what the columns of the pixels in flight may take
// the package's default table for MOD15A2H's FparLai_QC (mod16_amd/gapfill.py: default_good)
bool smooth_default_good(int q) {
    const int cloud = (q >> 3) & 3;
    return !(q & 1) && !(q & 4) && (cloud == 0 || cloud == 3) && (q >> 5) <= 1;
}
size_t smooth_out_size(int out_type) { return out_type == MOD16_SMOOTH_U8 ? 1 : out_type == MOD16_SMOOTH_F32 ? 4 : 8; }

// The lanes of a launch over n pixels: whole blocks, no more than the pixels need, than the chip holds
// (8 blocks per CU) or than the workspace budget holds columns for; at least one block.
int64_t smooth_lanes(const mod16_ctx* ctx, int64_t n, int slabs, int envelope) {
    const int64_t per_lane = (int64_t)smooth_columns(envelope) * slabs * (int64_t)sizeof(double);
    const int64_t need = (n + kBlock - 1) / kBlock * kBlock;
    const int64_t fit = kSmoothBudget / per_lane / kBlock * kBlock;
    return std::max<int64_t>(kBlock, std::min({need, fit, (int64_t)ctx->cus * 8 * kBlock}));
}
size_t smooth_ws_bytes(int64_t lanes, int slabs, int envelope) {
    return kSmoothTableBytes + (size_t)smooth_columns(envelope) * slabs * (size_t)lanes * sizeof(double);
}
}  // namespace

// The context's workspace holds `bytes`. It only grows, at least twofold while that stays within the
// budget; the outgrown block is retired (earlier launches may still use it) and freed with the context.
static int smooth_reserve(mod16_ctx* ctx, size_t bytes) {
    if (ctx->smooth_ws.bytes() >= bytes) return MOD16_OK;
    const size_t cap = std::max(bytes, kSmoothTableBytes + (size_t)kSmoothBudget);
    const size_t want = std::min(cap, std::max(bytes, 2 * ctx->smooth_ws.bytes()));
    if (ctx->smooth_ws) ctx->retired.push_back(std::move(ctx->smooth_ws));
    return ctx->smooth_ws.alloc(ctx, want, "mod16_smooth: device memory for the workspace of the columns");
}

// All pointers are device pointers here (a.qc_weight may be NULL: the default table, in a.good_bits).
template <typename IN>
static int launch_smooth(mod16_ctx* ctx, SmoothArgs a, int out_type, hipStream_t st) {
    if (a.n <= 0) return MOD16_OK;
    a.lanes = smooth_lanes(ctx, a.n, a.slabs, a.envelope);
    int rc = smooth_reserve(ctx, smooth_ws_bytes(a.lanes, a.slabs, a.envelope));
    if (rc != MOD16_OK) return rc;
    a.ws = reinterpret_cast<double*>(ctx->smooth_ws.as<char>() + kSmoothTableBytes);
    rc = ws_acquire(ctx, st);          // the workspace is shared by the context's launches: one behind the other
    if (rc != MOD16_OK) return rc;
    const dim3 grid((unsigned)(a.lanes / kBlock)), block(kBlock);
    if constexpr (std::is_same<IN, uint8_t>::value) {
        if (out_type == MOD16_SMOOTH_U8) hipLaunchKernelGGL((smooth_kernel<uint8_t, uint8_t>), grid, block, 0, st, a);
        else if (out_type == MOD16_SMOOTH_F32) hipLaunchKernelGGL((smooth_kernel<uint8_t, float>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((smooth_kernel<uint8_t, double>), grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL((smooth_kernel<IN, IN>), grid, block, 0, st, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return ws_release(ctx, st);
}

// HOST mode: the slabs of the output, of the values, of the weights or the QC layer, and the counts,
// through the shared staging path; the tile cut so that a slot's slab fits stage_bytes. The plan's
// element is the widest of the arrays that are not bytes; the others sit in places of that size.
template <typename IN>
static int smooth_host(mod16_ctx* ctx, const SmoothArgs& a, int mode, int out_type, const double* table, int64_t stage_bytes) {
    const int S = a.slabs;
    const size_t osz = smooth_out_size(out_type);
    constexpr bool kBytesIn = sizeof(IN) == 1;
    const bool stack = mode == MOD16_SMOOTH_WEIGHT_STACK, qc = mode == MOD16_SMOOTH_WEIGHT_QC;
    const size_t esz = std::max({osz, sizeof(IN), stack ? sizeof(float) : (size_t)1, a.count ? sizeof(uint16_t) : (size_t)1});
    HostPlan p((int)esz);
    p.add(kOut, a.out, false, S, a.out_pitch, (int)osz);
    p.add(kIn, kBytesIn ? nullptr : a.in, false, kBytesIn ? 1 : S, a.in_pitch, (int)sizeof(IN));
    p.add(kIn, stack ? a.weights : nullptr, false, stack ? S : 1, a.w_pitch, (int)sizeof(float));
    p.add(kOut, a.count, false, 1, 0, (int)sizeof(uint16_t));
    p.add(kIn, kBytesIn ? a.in : nullptr, true, kBytesIn ? S : 1, a.in_pitch);
    p.add(kIn, qc ? a.qc : nullptr, true, qc ? S : 1, a.w_pitch);
    const int64_t tile = stage_tile(p, esz, stage_bytes);
    // the workspace at the size of a whole tile before the table goes to its head
    int rc = smooth_reserve(ctx, smooth_ws_bytes(smooth_lanes(ctx, std::min(a.n, tile), S, a.envelope), S, a.envelope));
    if (rc != MOD16_OK) return rc;
    if (table) HIPCHK(ctx, hipMemcpy(ctx->smooth_ws.get(), table, kSmoothTableBytes, hipMemcpyHostToDevice));
    auto launch = [&](const HostTile& t) {
        SmoothArgs d = a;
        d.n = t.m;
        d.out = t.dev[0];
        d.in = kBytesIn ? t.dev[4] : t.dev[1];
        d.weights = static_cast<const float*>(t.dev[2]);
        d.count = static_cast<uint16_t*>(t.dev[3]);
        d.qc = static_cast<const uint8_t*>(t.dev[5]);
        d.qc_weight = table ? ctx->smooth_ws.as<double>() : nullptr;
        d.out_pitch = (int64_t)(t.row_bytes / osz);
        d.in_pitch = kBytesIn ? (int64_t)t.byte_row_bytes : (int64_t)(t.row_bytes / sizeof(IN));
        d.w_pitch = stack ? (int64_t)(t.row_bytes / sizeof(float)) : (int64_t)t.byte_row_bytes;
        return launch_smooth<IN>(ctx, d, out_type, t.st);
    };
    return host_tiled(ctx, p, a.n, ctx->host_threads, false, launch, nullptr, tile);
}

template <typename IN>
static int smooth_entry(mod16_ctx* ctx, const mod16_smooth_spec* spec, const IN* values, const void* weights,
                        const double* qc_weight256, void* out, uint16_t* count, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_smooth: ", what); };
    if (!spec || !values || !out) return bad("NULL spec, values or out");
    if (spec->n < 0) return bad("n < 0");
    if (spec->slabs < 1 || spec->slabs > kSmoothMaxSlabs) return bad("slabs must be between 1 and 4096");
    if (spec->order != 1 && spec->order != 2) return bad("order must be 1 or 2");
    if (spec->envelope < 0 || spec->envelope > kSmoothMaxEnvelope) return bad("envelope must be between 0 and 8");
    if (spec->min_valid < spec->order) return bad("min_valid must be at least the order");
    if (!(std::isfinite(spec->lam) && spec->lam > 0.0)) return bad("lam must be finite and > 0");
    const int out_type = spec->out_type, mode = spec->weight_mode;
    if (out_type != MOD16_SMOOTH_U8 && out_type != MOD16_SMOOTH_F32 && out_type != MOD16_SMOOTH_F64)
        return bad("out_type must be MOD16_SMOOTH_U8, MOD16_SMOOTH_F32 or MOD16_SMOOTH_F64");
    constexpr bool kBytesIn = sizeof(IN) == 1;
    if (!kBytesIn && out_type != (sizeof(IN) == 4 ? MOD16_SMOOTH_F32 : MOD16_SMOOTH_F64))
        return bad("float values return their own type: out_type must be that of the values");
    if (mode != MOD16_SMOOTH_WEIGHT_NONE && mode != MOD16_SMOOTH_WEIGHT_STACK && mode != MOD16_SMOOTH_WEIGHT_QC)
        return bad("weight_mode must be MOD16_SMOOTH_WEIGHT_NONE, MOD16_SMOOTH_WEIGHT_STACK or MOD16_SMOOTH_WEIGHT_QC");
    if ((mode == MOD16_SMOOTH_WEIGHT_NONE) != (weights == nullptr)) return bad("weights must be given exactly where weight_mode asks for them");
    if (qc_weight256 && mode != MOD16_SMOOTH_WEIGHT_QC) return bad("qc_weight256 needs MOD16_SMOOTH_WEIGHT_QC");
    const bool scaled = kBytesIn && out_type != MOD16_SMOOTH_U8;
    if (scaled && !std::isfinite(spec->scale)) return bad("scale must be finite");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int S = spec->slabs;
    const int64_t n = spec->n;
    if (spec->in_pitch < n || spec->out_pitch < n) return bad("in_pitch and out_pitch must be at least n");
    if (weights && spec->weight_pitch < n) return bad("weight_pitch must be at least n");
    if (qc_weight256 && where == MOD16_HOST)
        for (int q = 0; q < 256; ++q)
            if (!(std::isfinite(qc_weight256[q]) && qc_weight256[q] >= 0.0)) return bad("qc_weight256 must be finite and not negative");
    if (n == 0) return MOD16_OK;
    const size_t osz = smooth_out_size(out_type);
    // in place is refused: no output may share a byte with an input or with another output
    {
        Extent ins[3], outs[2];
        int ni = 0, no = 0;
        ins[ni++] = extent(values, 1, 0, S, spec->in_pitch, n, sizeof(IN));
        if (weights) ins[ni++] = extent(weights, 1, 0, S, spec->weight_pitch, n, mode == MOD16_SMOOTH_WEIGHT_STACK ? sizeof(float) : 1);
        if (qc_weight256) ins[ni++] = extent(qc_weight256, 256, sizeof(double));
        outs[no++] = extent(out, 1, 0, S, spec->out_pitch, n, osz);
        if (count) outs[no++] = extent(count, n, sizeof(uint16_t));
        if (overlaps(outs, no, ins, ni)) return bad("an output overlaps an input or another output");
    }
    SmoothArgs a;
    memset(&a, 0, sizeof a);
    a.in = values;
    a.weights = mode == MOD16_SMOOTH_WEIGHT_STACK ? static_cast<const float*>(weights) : nullptr;
    a.qc = mode == MOD16_SMOOTH_WEIGHT_QC ? static_cast<const uint8_t*>(weights) : nullptr;
    a.qc_weight = where == MOD16_DEVICE ? qc_weight256 : nullptr;
    a.out = out;
    a.count = count;
    a.n = n;
    a.in_pitch = spec->in_pitch;
    a.w_pitch = weights ? spec->weight_pitch : 0;
    a.out_pitch = spec->out_pitch;
    a.lam = spec->lam;
    a.scale = scaled ? spec->scale : 1.0;
    for (int q = 0; q < 256; ++q)
        if (smooth_default_good(q)) a.good_bits[q >> 5] |= 1u << (q & 31);
    a.slabs = S;
    a.order = spec->order;
    a.envelope = spec->envelope;
    a.min_valid = spec->min_valid;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_DEVICE) return launch_smooth<IN>(ctx, a, out_type, static_cast<hipStream_t>(stream));
    return smooth_host<IN>(ctx, a, mode, out_type, qc_weight256, stage_budget(stage_bytes));
}

extern "C" int mod16_smooth_u8(mod16_ctx* ctx, const mod16_smooth_spec* spec, const uint8_t* values, const void* weights,
                               const double* qc_weight256, void* out, uint16_t* count, int where, void* stream,
                               size_t stage_bytes) {
    return smooth_entry<uint8_t>(ctx, spec, values, weights, qc_weight256, out, count, where, stream, stage_bytes);
}
extern "C" int mod16_smooth_f32(mod16_ctx* ctx, const mod16_smooth_spec* spec, const float* values, const void* weights,
                                const double* qc_weight256, void* out, uint16_t* count, int where, void* stream,
                                size_t stage_bytes) {
    return smooth_entry<float>(ctx, spec, values, weights, qc_weight256, out, count, where, stream, stage_bytes);
}
extern "C" int mod16_smooth_f64(mod16_ctx* ctx, const mod16_smooth_spec* spec, const double* values, const void* weights,
                                const double* qc_weight256, void* out, uint16_t* count, int where, void* stream,
                                size_t stage_bytes) {
    return smooth_entry<double>(ctx, spec, values, weights, qc_weight256, out, count, where, stream, stage_bytes);
}
extern "C" int mod16_smooth_max_slabs(void) { return kSmoothMaxSlabs; }
