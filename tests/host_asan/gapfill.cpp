// Stand-alone driver of tests/test_gapfill_host_asan.py: the HOST mode of mod16_gapfill_u8 -- the
// library's own host code under AddressSanitizer + UndefinedBehaviorSanitizer, linked against the HIP
// stand-in of tests/host_asan (device memory = host heap filled with 0xA5, a launch = its shape check;
// the gap-filling kernel has no shadow there). Every host array sits between guard bytes; the sizes
// make the tiles ragged; S = 1 and S = 5; all three output types; with and without the optional
// arrays. Pass: no sanitizer report, every output element overwritten, no guard byte and no padding
// byte of a pitched output touched, nothing left allocated.
#include <algorithm>
#include <cmath>

#define HARNESS_NAME "host_asan_gapfill"
#include "harness.hpp"

static void run(mod16_ctx* ctx, int out_type, int S, const char* what) {
    const int64_t n = 1237, pitch = n + 19, qpitch = n + 3, opitch = n + 7, spitch = n + 1;
    const size_t elem = out_type == MOD16_GAPFILL_U8 ? 1 : out_type == MOD16_GAPFILL_F32 ? 4 : 8;
    for (int nf = 1; nf <= 3; ++nf)
        for (int all = 0; all < 2; ++all) {          // with / without qc, good256, fallback and source
            mod16_gapfill_spec spec;
            memset(&spec, 0, sizeof spec);
            spec.n = n;
            spec.slabs = S;
            spec.nfields = nf;
            spec.out_type = out_type;
            spec.max_gap = all ? 2 : -1;
            spec.scale[0] = 0.01; spec.scale[1] = 0.1; spec.scale[2] = 1.0;
            spec.in_pitch = pitch; spec.qc_pitch = qpitch; spec.out_pitch = opitch; spec.source_pitch = spitch;
            std::vector<Guarded> in, fb;
            in.reserve(3); fb.reserve(3);
            const uint8_t* fields[3] = {nullptr, nullptr, nullptr};
            const uint8_t* fallback[3] = {nullptr, nullptr, nullptr};
            for (int f = 0; f < nf; ++f) {
                in.emplace_back(span(S, pitch, n, 1), (unsigned char)(40 + f));
                fields[f] = in.back().data();
                if (all && f != 1) {                 // (field 1 goes without)
                    fb.emplace_back((size_t)n, (unsigned char)7);
                    fallback[f] = fb.back().data();
                }
            }
            Guarded qc(span(S, qpitch, n, 1), 0), good(256, 1);
            // the slab of a slot: 3 output arrays apart by the stagger, rows of outputs and bytes per pixel
            const int wide_rows = nf * S + (3 - nf);
            const int byte_rows = nf * S + (3 - nf) + (all ? S : 1) + 3 + (all ? nf * S : 1);
            const size_t fixed = (size_t)3 * 33 * 1024 + 512, per_pixel = (size_t)wide_rows * elem + byte_rows;
            // tiles of 256 and of 512 pixels -- 5 and 3 tiles, the last ragged -- and, by default, one tile
            const size_t stages[] = {fixed + 300 * per_pixel, fixed + 600 * per_pixel, 0};
            for (size_t stage : stages) {
                std::vector<Guarded> out;
                out.reserve(3);
                void* outs[3] = {nullptr, nullptr, nullptr};
                for (int f = 0; f < nf; ++f) {
                    out.emplace_back(span(S, opitch, n, elem), kFresh);
                    outs[f] = out.back().data();
                }
                Guarded source(span(nf * S, spitch, n, 1), kFresh);
                const int rc = mod16_gapfill_u8(ctx, &spec, fields, all ? qc.data() : nullptr, all ? good.data() : nullptr,
                                                all ? fallback : nullptr, outs, all ? source.data() : nullptr, MOD16_HOST,
                                                nullptr, stage);
                if (rc != MOD16_OK) {
                    fprintf(stderr, "host_asan_gapfill: %s: status %d: %s\n", what, rc, mod16_last_error(ctx));
                    exit(1);
                }
                for (int f = 0; f < nf; ++f) check_written(out[f], S, opitch, n, elem, true, "out");
                check_written(source, nf * S, spitch, n, 1, all != 0, "source");
            }
            for (Guarded& g : in) EXPECT(g.guards_intact());
            for (Guarded& g : fb) EXPECT(g.guards_intact());
            EXPECT(qc.guards_intact() && good.guards_intact());
        }
    printf("host_asan_gapfill: %s, %d slabs done\n", what, S);
}

// refused before any device work; n = 0 is fine
static void refusals(mod16_ctx* ctx) {
    const int64_t n = 300;
    const int S = 4;
    Guarded a(span(S, n, n, 1), 50), b(span(S, n, n, 1), 60), qc(span(S, n, n, 1), 0);
    Guarded out0(span(S, n, n, 8), kFresh), out1(span(S, n, n, 8), kFresh), src(span(2 * S, n, n, 1), kFresh);
    const uint8_t* fields[3] = {a.data(), b.data(), nullptr};
    void* outs[3] = {out0.data(), out1.data(), nullptr};
    mod16_gapfill_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.n = n; spec.slabs = S; spec.nfields = 2; spec.out_type = MOD16_GAPFILL_F64; spec.max_gap = -1;
    spec.scale[0] = spec.scale[1] = 1.0;
    spec.in_pitch = spec.qc_pitch = spec.out_pitch = spec.source_pitch = n;
    auto call = [&](const mod16_gapfill_spec& s, const uint8_t* const* f, void* const* o, uint8_t* so, int where) {
        return mod16_gapfill_u8(ctx, &s, f, qc.data(), nullptr, nullptr, o, so, where, nullptr, 0);
    };
    mod16_gapfill_spec s = spec;
    EXPECT(call(spec, nullptr, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, fields, nullptr, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(mod16_gapfill_u8(ctx, nullptr, fields, nullptr, nullptr, nullptr, outs, nullptr, MOD16_HOST, nullptr, 0) == MOD16_ERR_ARG);
    s.n = -1; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.slabs = 0; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.slabs = 4097; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "slabs") != nullptr);
    s = spec; s.nfields = 0; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.nfields = 4; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.nfields = 3; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);   // a NULL third field
    s = spec; s.out_type = 3; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.max_gap = -2; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.in_pitch = n - 1; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.qc_pitch = n - 1; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.out_pitch = n - 1; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.source_pitch = n - 1; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    s = spec; s.scale[1] = std::nan(""); EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(spec, fields, outs, src.data(), 7) == MOD16_ERR_ARG);
    // in place, an output on the QC layer, two outputs on each other, the source bytes on an output
    s = spec; s.out_type = MOD16_GAPFILL_U8;
    void* inplace[3] = {a.data(), out1.data(), nullptr};
    EXPECT(call(s, fields, inplace, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(strstr(mod16_last_error(ctx), "overlaps") != nullptr);
    void* onqc[3] = {out0.data(), qc.data() + 5, nullptr};
    EXPECT(call(s, fields, onqc, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    void* twice[3] = {out0.data(), out0.data() + n, nullptr};
    EXPECT(call(s, fields, twice, src.data(), MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(s, fields, outs, out1.data() + 3, MOD16_HOST) == MOD16_ERR_ARG);
    EXPECT(call(s, fields, outs, a.data(), MOD16_DEVICE) == MOD16_ERR_ARG);
    s = spec; s.n = 0; EXPECT(call(s, fields, outs, src.data(), MOD16_HOST) == MOD16_OK);
    check_written(out0, S, n, n, 8, false, "out[0] of the refused calls");
    check_written(out1, S, n, n, 8, false, "out[1] of the refused calls");
    check_written(src, 2 * S, n, n, 1, false, "source of the refused calls");
    EXPECT(a.guards_intact() && b.guards_intact() && qc.guards_intact());
    printf("host_asan_gapfill: refusals done\n");
}

int main() {
    setenv("MOD16_HOST_THREADS", "3", 1);
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    const int types[] = {MOD16_GAPFILL_U8, MOD16_GAPFILL_F32, MOD16_GAPFILL_F64};
    const char* names[] = {"uint8", "float32", "float64"};
    for (int k = 0; k < 3; ++k) {
        run(ctx, types[k], 5, names[k]);
        run(ctx, types[k], 1, names[k]);
    }
    refusals(ctx);
    harness_finish(ctx);
    return 0;
}
