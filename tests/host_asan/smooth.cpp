// Stand-alone driver of tests/test_smooth_host_asan.py: the HOST mode of mod16_smooth_u8 / _f32 / _f64 --
// the library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP
// stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check;
// the smoothing kernels have no shadow there). Every host array sits between guard bytes; 1237 pixels in
// tiles of 256, of 512 and in one tile; S = 5 and S = 1; the three input types with every output type
// they allow; no weights, a float32 stack, a QC layer with the default and with a table of the caller's;
// with and without the counts; every array with a pitch of its own. Pass: no sanitizer report, every
// output element overwritten, no guard byte and no padding byte of a pitched output touched, nothing
// left allocated.
#include <algorithm>
#include <cmath>
#include <limits>

#define HARNESS_NAME "host_asan_smooth"
#include "harness.hpp"

template <typename IN>
static int call(mod16_ctx* ctx, const mod16_smooth_spec* spec, const void* values, const void* weights, const double* table,
                void* out, uint16_t* count, int where, size_t stage) {
    if (sizeof(IN) == 1)
        return mod16_smooth_u8(ctx, spec, static_cast<const uint8_t*>(values), weights, table, out, count, where, nullptr, stage);
    if (sizeof(IN) == 4)
        return mod16_smooth_f32(ctx, spec, static_cast<const float*>(values), weights, table, out, count, where, nullptr, stage);
    return mod16_smooth_f64(ctx, spec, static_cast<const double*>(values), weights, table, out, count, where, nullptr, stage);
}

static size_t out_size(int out_type) { return out_type == MOD16_SMOOTH_U8 ? 1 : out_type == MOD16_SMOOTH_F32 ? 4 : 8; }

template <typename IN>
static void run(mod16_ctx* ctx, int out_type, int S, const char* what) {
    const int64_t n = 1237, pitch = n + 19, wpitch = n + 3, opitch = n + 7;
    const size_t osz = out_size(out_type);
    std::vector<double> table(256, 0.5);
    for (int mode = 0; mode < 4; ++mode)              // none, stack, QC with the default table, QC with the caller's
        for (int counted = 0; counted < 2; ++counted) {
            const bool stack = mode == 1, qc = mode >= 2;
            mod16_smooth_spec spec;
            memset(&spec, 0, sizeof spec);
            spec.n = n; spec.slabs = S; spec.order = 1 + mode % 2; spec.envelope = counted ? 2 : 0; spec.min_valid = 2;
            spec.weight_mode = stack ? MOD16_SMOOTH_WEIGHT_STACK : qc ? MOD16_SMOOTH_WEIGHT_QC : MOD16_SMOOTH_WEIGHT_NONE;
            spec.out_type = out_type;
            spec.lam = 10.0; spec.scale = 0.01;
            spec.in_pitch = pitch; spec.weight_pitch = wpitch; spec.out_pitch = opitch;
            Guarded in(span(S, pitch, n, sizeof(IN)), 0), w(span(S, wpitch, n, stack ? 4 : 1), 0);
            // the slab of a slot: 4 arrays apart by the stagger; per pixel the rows of the widest element and the byte rows
            const size_t esz = std::max({osz, sizeof(IN), stack ? (size_t)4 : (size_t)1, counted ? (size_t)2 : (size_t)1});
            const int wide_rows = S + (sizeof(IN) == 1 ? 1 : S) + (stack ? S : 1) + 1;
            const int byte_rows = (sizeof(IN) == 1 ? S : 1) + (qc ? S : 1);
            const size_t fixed = (size_t)4 * 33 * 1024 + 512, per_pixel = (size_t)wide_rows * esz + byte_rows;
            // tiles of 256 and of 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
            const size_t stages[] = {fixed + 300 * per_pixel, fixed + 600 * per_pixel, 0};
            for (size_t stage : stages) {
                Guarded out(span(S, opitch, n, osz), kFresh), count((size_t)n * 2, kFresh);
                const int rc = call<IN>(ctx, &spec, in.data(), mode ? w.data() : nullptr, mode == 3 ? table.data() : nullptr,
                                        out.data(), counted ? count.as<uint16_t>() : nullptr, MOD16_HOST, stage);
                if (rc != MOD16_OK) {
                    fprintf(stderr, "host_asan_smooth: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                    exit(1);
                }
                check_written(out, S, opitch, n, osz, true, "out");
                check_written(count, 2, counted != 0, "count");
            }
            EXPECT(in.guards_intact() && w.guards_intact());
        }
    printf("host_asan_smooth: %s, %d slabs done\n", what, S);
}

// refused before any device work and before an output is touched; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const int64_t n = 300;
    const int S = 4;
    const char* pre = "mod16_smooth: ";
    Guarded a(span(S, n, n, 1), 50), qc(span(S, n, n, 1), 0), wf(span(S, n, n, 4), 0), xf(span(S, n, n, 8), 0);
    Guarded out(span(S, n, n, 8), kFresh), cnt((size_t)n * 2, kFresh);
    std::vector<double> table(256, 1.0);
    mod16_smooth_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.n = n; spec.slabs = S; spec.order = 2; spec.envelope = 1; spec.min_valid = 3;
    spec.weight_mode = MOD16_SMOOTH_WEIGHT_QC; spec.out_type = MOD16_SMOOTH_F64;
    spec.lam = 10.0; spec.scale = 1.0;
    spec.in_pitch = spec.weight_pitch = spec.out_pitch = n;
    uint16_t* count = cnt.as<uint16_t>();
    auto u8 = [&](const mod16_smooth_spec& s, const void* v, const void* w, const double* t, void* o, uint16_t* c, int where) {
        return mod16_smooth_u8(ctx, &s, static_cast<const uint8_t*>(v), w, t, o, c, where, nullptr, 0);
    };
    mod16_smooth_spec s = spec;
    EXPECT(mod16_smooth_u8(nullptr, &spec, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    EXPECT(refused(ctx, mod16_smooth_u8(ctx, nullptr, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST, nullptr, 0), pre, "NULL"));
    EXPECT(refused(ctx, u8(spec, nullptr, qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "NULL"));
    EXPECT(refused(ctx, u8(spec, a.data(), qc.data(), nullptr, nullptr, count, MOD16_HOST), pre, "NULL"));
    s.n = -1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "n < 0"));
    s = spec; s.slabs = 0; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "slabs"));
    s = spec; s.slabs = mod16_smooth_max_slabs() + 1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "slabs"));
    s = spec; s.order = 0; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "order"));
    s = spec; s.order = 3; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "order"));
    s = spec; s.envelope = -1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "envelope"));
    s = spec; s.envelope = 9; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "envelope"));
    s = spec; s.min_valid = 1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "min_valid"));
    s = spec; s.lam = 0.0; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "lam"));
    s = spec; s.lam = std::nan(""); EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "lam"));
    s = spec; s.lam = std::numeric_limits<double>::infinity();
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "lam"));
    s = spec; s.out_type = 3; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "out_type"));
    s = spec; s.weight_mode = 3; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "weight_mode"));
    s = spec; s.weight_mode = MOD16_SMOOTH_WEIGHT_NONE;
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "weights"));
    EXPECT(refused(ctx, u8(spec, a.data(), nullptr, nullptr, out.data(), count, MOD16_HOST), pre, "weights"));
    s = spec; s.weight_mode = MOD16_SMOOTH_WEIGHT_STACK;
    EXPECT(refused(ctx, u8(s, a.data(), wf.data(), table.data(), out.data(), count, MOD16_HOST), pre, "qc_weight256"));
    s = spec; s.scale = std::nan(""); EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "scale"));
    s = spec; s.in_pitch = n - 1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "pitch"));
    s = spec; s.out_pitch = n - 1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "pitch"));
    s = spec; s.weight_pitch = n - 1; EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST), pre, "weight_pitch"));
    EXPECT(refused(ctx, u8(spec, a.data(), qc.data(), nullptr, out.data(), count, 7), pre, "where"));
    table[17] = -0.5;
    EXPECT(refused(ctx, u8(spec, a.data(), qc.data(), table.data(), out.data(), count, MOD16_HOST), pre, "qc_weight256"));
    table[17] = std::nan("");
    EXPECT(refused(ctx, u8(spec, a.data(), qc.data(), table.data(), out.data(), count, MOD16_HOST), pre, "qc_weight256"));
    table[17] = 1.0;
    // float values return their own type
    s = spec; s.out_type = MOD16_SMOOTH_F32;
    EXPECT(refused(ctx, mod16_smooth_f64(ctx, &s, xf.as<double>(), qc.data(), nullptr, out.data(), count, MOD16_HOST, nullptr, 0), pre, "own type"));
    s.out_type = MOD16_SMOOTH_U8;
    EXPECT(refused(ctx, mod16_smooth_f32(ctx, &s, xf.as<float>(), qc.data(), nullptr, out.data(), count, MOD16_HOST, nullptr, 0), pre, "own type"));
    // in place, the output on the QC layer, on the table, the counts on the output, on the values
    s = spec; s.out_type = MOD16_SMOOTH_U8;
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, a.data(), count, MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, qc.data() + 5, count, MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), table.data(), table.data(), count, MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), out.as<uint16_t>() + 3, MOD16_HOST), pre, "overlaps"));
    EXPECT(refused(ctx, u8(s, a.data(), qc.data(), nullptr, out.data(), a.as<uint16_t>(), MOD16_DEVICE), pre, "overlaps"));
    EXPECT(refused(ctx, mod16_smooth_f64(ctx, &spec, xf.as<double>(), qc.data(), nullptr, xf.data(), count, MOD16_HOST, nullptr, 0), pre, "overlaps"));
    s = spec; s.n = 0; EXPECT(u8(s, a.data(), qc.data(), nullptr, out.data(), count, MOD16_HOST) == MOD16_OK);
    check_written(out, S, n, n, 8, false, "out of the refused calls");
    check_written(cnt, 2, false, "count of the refused calls");
    EXPECT(a.guards_intact() && qc.guards_intact() && wf.guards_intact() && xf.guards_intact());
    printf("host_asan_smooth: refusals done\n");
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    EXPECT(mod16_smooth_max_slabs() >= 138);
    const int slabs[] = {5, 1};
    for (int S : slabs) {
        run<uint8_t>(ctx, MOD16_SMOOTH_U8, S, "uint8 -> uint8");
        run<uint8_t>(ctx, MOD16_SMOOTH_F32, S, "uint8 -> float32");
        run<uint8_t>(ctx, MOD16_SMOOTH_F64, S, "uint8 -> float64");
        run<float>(ctx, MOD16_SMOOTH_F32, S, "float32");
        run<double>(ctx, MOD16_SMOOTH_F64, S, "float64");
    }
    refusals(ctx);
    harness_finish(ctx);
    return 0;
}
