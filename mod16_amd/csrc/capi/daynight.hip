// libmod16hip.so -- hourly reanalysis aggregated into day / night drivers: mod16_daynight_f32 / _f64 (the coarse planes of lw_net, sw_rad, temp, tmin, vpd, the hours of daylight and the daily mean per day in one launch, temp_annual behind it)
#include "host.hpp"
#include "../mod16_daynight.hpp"

namespace {
constexpr int64_t kDnMaxExtent = int64_t(1) << 30;
// the fields an output is made from, as bits of kDnT ... kDnLw
constexpr unsigned kDnNeeds[kDnOutputs] = {1u << kDnLw, 1u << kDnLw, 1u << kDnSw, 1u << kDnT, 1u << kDnT, 1u << kDnT,
                                           (1u << kDnT) | (1u << kDnQv) | (1u << kDnPs),
                                           (1u << kDnT) | (1u << kDnQv) | (1u << kDnPs), 0u, 1u << kDnT};

// The arguments of a call as the entry point checked them; pointers of the caller's side (`where`).
struct DnCall {
    const void* field[kDnFields];
    void* out[kDnOutputs];
    void* annual;
    const double* half_day;
    const double* noon;
    const double* offset;
    int64_t rows, cols, in_pitch, in_plane, out_pitch, out_plane;
    int days, steps, mode;
    double threshold;
};

// rows of n elements between two layouts (pitch, plane in elements): whole runs where both sides are dense
int dn_copy(mod16_ctx* ctx, char* dst, int64_t dpitch, int64_t dplane, const char* src, int64_t spitch, int64_t splane,
            int64_t planes, int64_t rows, int64_t n, size_t elem, hipMemcpyKind kind, hipStream_t st) {
    const bool dense_rows = (dpitch == n && spitch == n) || rows == 1;
    if (dense_rows && ((dplane == rows * n && splane == rows * n) || planes == 1)) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)(planes * rows * n) * elem, kind, st));
        return MOD16_OK;
    }
    for (int64_t p = 0; p < planes; ++p) {
        if (dense_rows) {
            HIPCHK(ctx, hipMemcpyAsync(dst + p * dplane * elem, src + p * splane * elem, (size_t)(rows * n) * elem, kind, st));
            continue;
        }
        for (int64_t r = 0; r < rows; ++r)
            HIPCHK(ctx, hipMemcpyAsync(dst + (p * dplane + r * dpitch) * elem, src + (p * splane + r * spitch) * elem,
                                       (size_t)n * elem, kind, st));
    }
    return MOD16_OK;
}
}  // namespace

// All pointers are device pointers here (the tables too). days: of this launch; total_days, first,
// last, acc: temp_annual across the chunks of HOST mode (annual NULL: not wanted); mean64: the
// workspace of the launch's daily means of t, [days][rows * cols].
template <typename IN, typename OUT>
static int launch_daynight_as(mod16_ctx* ctx, const DnCall& c, void* annual, int64_t annual_pitch, double* mean64, double* acc,
                              bool first, bool last, int total_days, hipStream_t st) {
    DnArgs a;
    memset(&a, 0, sizeof a);
    // vector access: base, row pitch and plane stride are multiples of the vector size (kDnPx elements)
    auto aligned = [](const void* p, int64_t pitch, int64_t plane, size_t elem) {
        return !p || (reinterpret_cast<uintptr_t>(p) % (kDnPx * elem) == 0 && pitch % kDnPx == 0 && plane % kDnPx == 0);
    };
    bool in = true, out = true, any = false;
    for (int f = 0; f < kDnFields; ++f) {
        a.field[f] = c.field[f];
        in = in && aligned(c.field[f], c.in_pitch, c.in_plane, sizeof(IN));
    }
    for (int o = 0; o < kDnOutputs; ++o) {
        a.out[o] = c.out[o];
        any = any || c.out[o];
        out = out && aligned(c.out[o], c.out_pitch, c.out_plane, sizeof(OUT));
    }
    a.wide = (in ? kDnWideIn : 0) | (out ? kDnWideOut : 0);
    a.half_day = c.half_day;
    a.noon = c.noon;
    a.offset = c.offset;
    a.mean64 = annual ? mean64 : nullptr;
    a.in_pitch = c.in_pitch; a.in_plane = c.in_plane; a.out_pitch = c.out_pitch; a.out_plane = c.out_plane;
    a.lanes_per_row = (c.cols + kDnPx - 1) / kDnPx;
    a.hd = (double)c.steps;
    a.delta = 24.0 / a.hd;
    a.threshold = c.threshold;
    a.rows = (int)c.rows; a.cols = (int)c.cols; a.days = c.days; a.steps = c.steps; a.mode = c.mode;
    const int64_t blocks = (a.lanes_per_row * c.rows + kBlock - 1) / kBlock;
    const int64_t cells = (c.rows * c.cols + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffff || cells > 0x7fffffff) return fail(ctx, MOD16_ERR_ARG, "mod16_daynight: rows x cols is too large for one launch");
    if (any || annual) {
        // day chunks: enough blocks for four per CU, at least kDnMinChunk days per lane
        const int64_t want = std::max<int64_t>(1, ((int64_t)ctx->cus * 4 + blocks - 1) / blocks);
        int chunk = (int)((c.days + want - 1) / want);
        chunk = std::min(c.days, std::max(chunk, kDnMinChunk));
        a.chunk = chunk;
        const int ny = (c.days + chunk - 1) / chunk;
        hipLaunchKernelGGL((daynight_kernel<IN, OUT>), dim3((unsigned)blocks, (unsigned)ny), dim3(kBlock), 0, st, a);
    }
    if (annual) {
        DnAnnualArgs n;
        memset(&n, 0, sizeof n);
        n.mean64 = mean64;
        n.acc = acc;
        n.out = annual;
        n.out_pitch = annual_pitch;
        n.total_days = (double)total_days;
        n.rows = (int)c.rows; n.cols = (int)c.cols; n.days = c.days;
        n.first = first; n.last = last;
        hipLaunchKernelGGL((daynight_annual_kernel<OUT>), dim3((unsigned)cells), dim3(kBlock), 0, st, n);
    }
    HIPCHK(ctx, hipGetLastError());
    return MOD16_OK;
}

template <typename IN>
static int launch_daynight(mod16_ctx* ctx, int out_type, const DnCall& c, void* annual, int64_t annual_pitch, double* mean64,
                           double* acc, bool first, bool last, int total_days, hipStream_t st) {
    if (out_type == MOD16_DAYNIGHT_F32)
        return launch_daynight_as<IN, float>(ctx, c, annual, annual_pitch, mean64, acc, first, last, total_days, st);
    return launch_daynight_as<IN, double>(ctx, c, annual, annual_pitch, mean64, acc, first, last, total_days, st);
}

// the three tables ('solar' mode) as device copies in one stream-ordered block -> c.half_day, c.noon, c.offset
static int dn_upload_tables(mod16_ctx* ctx, DnCall& c, AsyncMem& block, hipStream_t st) {
    if (c.mode != kDnModeSolar) return MOD16_OK;
    const size_t nh = (size_t)c.days * (size_t)c.rows, nn = (size_t)c.days, no = (size_t)c.cols;
    Carver size;
    size.take<double>(nh * 8); size.take<double>(nn * 8); size.take<double>(no * 8);
    int rc = block.alloc(ctx, size.used, "mod16_daynight: device memory for the tables");
    if (rc != MOD16_OK) return rc;
    Carver at(block.p);
    double* dh = at.take<double>(nh * 8);
    double* dn = at.take<double>(nn * 8);
    double* dof = at.take<double>(no * 8);
    HIPCHK(ctx, hipMemcpyAsync(dh, c.half_day, nh * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dn, c.noon, nn * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dof, c.offset, no * 8, hipMemcpyHostToDevice, st));
    c.half_day = dh; c.noon = dn; c.offset = dof;
    return MOD16_OK;
}

// HOST mode: chunks of whole days through slab 0 on stream 0 -- the steps of the chunk's days of every
// field given, the chunk's planes of every output requested, dense ([rows][cols]) on the device; the
// running sum of temp_annual, its plane and the chunk's daily means live beside the tables for the
// whole call
template <typename IN>
static int daynight_host(mod16_ctx* ctx, int out_type, const DnCall& h, int64_t stage_bytes) {
    const size_t isz = sizeof(IN), osz = out_type == MOD16_DAYNIGHT_F32 ? 4 : 8;
    const int64_t R = h.rows, W = h.cols, cells = R * W;
    int nf = 0, no = 0;
    for (int f = 0; f < kDnFields; ++f) nf += h.field[f] != nullptr;
    for (int o = 0; o < kDnOutputs; ++o) no += h.out[o] != nullptr;
    const int64_t per_day = (int64_t)nf * h.steps * cells * (int64_t)isz + (int64_t)no * cells * (int64_t)osz;
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(h.days, stage_bytes / std::max<int64_t>(per_day, 1)));
    const size_t in_bytes = align256((size_t)chunk * h.steps * cells * isz), out_bytes = align256((size_t)chunk * cells * osz);
    int rc = reserve_slabs(ctx, in_bytes * nf + out_bytes * no + 256, 1);
    if (rc != MOD16_OK) return rc;
    hipStream_t st = ctx->streams[0];
    DnCall dev = h;
    AsyncMem tables(st), annual(st);
    rc = dn_upload_tables(ctx, dev, tables, st);
    if (rc != MOD16_OK) return rc;
    const double* const all_half = dev.half_day;
    const double* const all_noon = dev.noon;
    double* acc = nullptr;
    double* mean64 = nullptr;
    char* aplane = nullptr;
    if (h.annual) {
        Carver size;
        size.take<double>((size_t)cells * 8); size.take<char>((size_t)cells * osz); size.take<double>((size_t)chunk * cells * 8);
        rc = annual.alloc(ctx, size.used, "mod16_daynight: device memory for temp_annual");
        if (rc != MOD16_OK) return rc;
        Carver at(annual.p);
        acc = at.take<double>((size_t)cells * 8);
        aplane = at.take<char>((size_t)cells * osz);
        mean64 = at.take<double>((size_t)chunk * cells * 8);
    }
    char* base = ctx->slab[0].as<char>();
    dev.in_pitch = dev.out_pitch = W;
    dev.in_plane = dev.out_plane = cells;
    for (int d0 = 0; d0 < h.days; d0 += chunk) {
        const int m = std::min(chunk, h.days - d0);
        char* at = base;
        for (int f = 0; f < kDnFields; ++f) {
            dev.field[f] = nullptr;
            if (!h.field[f]) continue;
            rc = dn_copy(ctx, at, W, cells, static_cast<const char*>(h.field[f]) + (size_t)d0 * h.steps * h.in_plane * isz,
                         h.in_pitch, h.in_plane, (int64_t)m * h.steps, R, W, isz, hipMemcpyHostToDevice, st);
            if (rc != MOD16_OK) return rc;
            dev.field[f] = at;
            at += in_bytes;
        }
        char* outs = at;
        for (int o = 0; o < kDnOutputs; ++o) {
            dev.out[o] = h.out[o] ? at : nullptr;
            if (h.out[o]) at += out_bytes;
        }
        dev.days = m;
        if (h.mode == kDnModeSolar) {
            dev.half_day = all_half + (size_t)d0 * R;
            dev.noon = all_noon + d0;
        }
        rc = launch_daynight<IN>(ctx, out_type, dev, aplane, W, mean64, acc, d0 == 0, d0 + m == h.days, h.days, st);
        if (rc != MOD16_OK) return rc;
        at = outs;
        for (int o = 0; o < kDnOutputs; ++o) {
            if (!h.out[o]) continue;
            rc = dn_copy(ctx, static_cast<char*>(h.out[o]) + (size_t)d0 * h.out_plane * osz, h.out_pitch, h.out_plane, at, W,
                         cells, m, R, W, osz, hipMemcpyDeviceToHost, st);
            if (rc != MOD16_OK) return rc;
            at += out_bytes;
        }
        HIPCHK(ctx, hipStreamSynchronize(st));      // the slab is free again
    }
    if (h.annual) {
        rc = dn_copy(ctx, static_cast<char*>(h.annual), h.out_pitch, 0, aplane, W, 0, 1, R, W, osz, hipMemcpyDeviceToHost, st);
        if (rc != MOD16_OK) return rc;
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    return MOD16_OK;
}

template <typename IN>
static int daynight_entry(mod16_ctx* ctx, const mod16_daynight_spec* spec, const IN* const* fields, const double* half_day,
                          const double* noon, const double* offset, void* const* out, void* temp_annual, int where,
                          void* stream, size_t stage_bytes) {
    if (!ctx) return MOD16_ERR_ARG;
    auto bad = [&](const char* what) { return fail(ctx, MOD16_ERR_ARG, "mod16_daynight: ", what); };
    if (!spec) return bad("NULL spec");
    if (!fields || !out) return bad("NULL fields or out");
    if (spec->rows < 0 || spec->rows > kDnMaxExtent || spec->cols < 0 || spec->cols > kDnMaxExtent)
        return bad("rows and cols must be between 0 and 2^30");
    if (spec->days < 0 || spec->days > kDnMaxDays) return bad("days must be between 0 and 4096");
    if (spec->steps_per_day < 1 || spec->steps_per_day > kDnMaxSteps) return bad("steps_per_day must be between 1 and 48");
    if (spec->mode != MOD16_DAYNIGHT_SOLAR && spec->mode != MOD16_DAYNIGHT_SW) return bad("mode must be MOD16_DAYNIGHT_SOLAR or MOD16_DAYNIGHT_SW");
    if (spec->out_type != MOD16_DAYNIGHT_F32 && spec->out_type != MOD16_DAYNIGHT_F64) return bad("out_type must be MOD16_DAYNIGHT_F32 or MOD16_DAYNIGHT_F64");
    if (const char* what = check_where_stage(where, stage_bytes)) return bad(what);
    const int64_t R = spec->rows, W = spec->cols;
    const int D = spec->days, H = spec->steps_per_day;
    const bool solar = spec->mode == MOD16_DAYNIGHT_SOLAR;
    DnCall c;
    memset(&c, 0, sizeof c);
    unsigned given = 0;
    bool any = temp_annual != nullptr;
    for (int f = 0; f < kDnFields; ++f) {
        c.field[f] = fields[f];
        if (fields[f]) given |= 1u << f;
    }
    const unsigned extra = solar ? 0u : 1u << kDnSw;
    for (int o = 0; o < kDnOutputs; ++o) {
        c.out[o] = out[o];
        any = any || out[o];
        if (out[o] && ((kDnNeeds[o] | extra) & ~given)) return bad("an output is requested whose field is NULL");
    }
    if (temp_annual && (((1u << kDnT) | extra) & ~given)) return bad("temp_annual is requested and the field t is NULL");
    if (!any) return bad("no output is requested");
    if (spec->in_pitch < W || spec->out_pitch < W) return bad("in_pitch and out_pitch must be at least cols");
    const int64_t plane = R > 0 ? (R - 1) * spec->in_pitch + W : 0, oplane = R > 0 ? (R - 1) * spec->out_pitch + W : 0;
    if (spec->in_plane < plane || spec->out_plane < oplane) return bad("in_plane and out_plane must be at least a plane ((rows - 1) pitch + cols)");
    if (solar) {
        if (!half_day || !noon || !offset) return bad("MOD16_DAYNIGHT_SOLAR needs half_day, noon and offset");
        for (int64_t i = 0; i < (int64_t)D * R; ++i)
            if (!(half_day[i] >= 0.0 && half_day[i] <= 12.0)) return bad("half_day holds a value outside 0 ... 12 (or not finite)");
        for (int i = 0; i < D; ++i)
            if (!(noon[i] >= 0.0 && noon[i] <= 24.0)) return bad("noon holds a value outside 0 ... 24 (or not finite)");
        for (int64_t i = 0; i < W; ++i)
            if (!(offset[i] >= -12.0 && offset[i] <= 12.0)) return bad("offset holds a value outside -12 ... 12 (or not finite)");
    } else if (!std::isfinite(spec->threshold)) {
        return bad("threshold must be finite");
    }
    if (D == 0 || R == 0 || W == 0) return MOD16_OK;
    const size_t osz = spec->out_type == MOD16_DAYNIGHT_F32 ? 4 : 8;
    // no output may share a byte with an input or with another output
    {
        Extent ins[kDnFields + 3], outs[kDnOutputs + 1];
        int ni = 0, no = 0;
        for (int f = 0; f < kDnFields; ++f)
            if (fields[f]) ins[ni++] = extent(fields[f], (int64_t)D * H, spec->in_plane, R, spec->in_pitch, W, sizeof(IN));
        if (solar && where == MOD16_HOST) {
            ins[ni++] = extent(half_day, (int64_t)D * R, 8);
            ins[ni++] = extent(noon, D, 8);
            ins[ni++] = extent(offset, W, 8);
        }
        for (int o = 0; o < kDnOutputs; ++o)
            if (out[o]) outs[no++] = extent(out[o], D, spec->out_plane, R, spec->out_pitch, W, osz);
        if (temp_annual) outs[no++] = extent(temp_annual, 1, 0, R, spec->out_pitch, W, osz);
        if (overlaps(outs, no, ins, ni)) return bad("an output overlaps an input or another output");
    }
    c.annual = temp_annual;
    c.half_day = half_day; c.noon = noon; c.offset = offset;
    c.rows = R; c.cols = W;
    c.in_pitch = spec->in_pitch; c.in_plane = spec->in_plane; c.out_pitch = spec->out_pitch; c.out_plane = spec->out_plane;
    c.days = D; c.steps = H; c.mode = solar ? kDnModeSolar : kDnModeSw;
    c.threshold = spec->threshold;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MOD16_HOST) return daynight_host<IN>(ctx, spec->out_type, c, stage_budget(stage_bytes));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AsyncMem tables(st), means(st);
    int rc = dn_upload_tables(ctx, c, tables, st);
    if (rc == MOD16_OK && temp_annual) rc = means.alloc(ctx, (size_t)D * (size_t)(R * W) * 8, "mod16_daynight: device memory for the daily means of temp_annual");
    if (rc != MOD16_OK) return rc;
    return launch_daynight<IN>(ctx, spec->out_type, c, temp_annual, spec->out_pitch, static_cast<double*>(means.p), nullptr, true, true, D, st);
}

extern "C" int mod16_daynight_f32(mod16_ctx* ctx, const mod16_daynight_spec* spec, const float* const* fields,
                                  const double* half_day, const double* noon, const double* offset, void* const* out,
                                  void* temp_annual, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    return daynight_entry<float>(ctx, spec, fields, half_day, noon, offset, out, temp_annual, where, stream, stage_bytes);
}
extern "C" int mod16_daynight_f64(mod16_ctx* ctx, const mod16_daynight_spec* spec, const double* const* fields,
                                  const double* half_day, const double* noon, const double* offset, void* const* out,
                                  void* temp_annual, int where, void* stream, size_t stage_bytes) {
    MOD16_LOCK(ctx);
    return daynight_entry<double>(ctx, spec, fields, half_day, noon, offset, out, temp_annual, where, stream, stage_bytes);
}
