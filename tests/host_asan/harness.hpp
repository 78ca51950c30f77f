// What the stand-alone sanitizer programs of this directory share. A driver names itself first,
//   #define HARNESS_NAME "host_asan_trend"
//   #include "harness.hpp"
// and gets: EXPECT, host blocks between guard bytes (Guarded), the one check that an output was
// overwritten where it should be and nowhere else (check_written), the check of a refusal (refused), the
// declarations of the HIP stand-in's own entry points (hip_stub.hip) and the common end of main
// (harness_finish).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mod16_hip.h"

extern "C" void mod16_stub_report(FILE* f);
extern "C" size_t mod16_stub_live_allocations(void);
extern "C" void mod16_stub_fail_malloc(int k);           // the k-th next hipMalloc / hipMallocAsync fails, once
extern "C" void mod16_stub_fail_host_malloc(int k);      // k > 0: the next k calls fail; -k: the k-th next call fails, once

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, HARNESS_NAME ": %s failed (line %d)\n", #cond, __LINE__); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

constexpr size_t kGuard = 64;
constexpr unsigned char kGuardByte = 0xC3, kFresh = 0x11;

// `bytes` of payload between two runs of guard bytes, in one heap block of its own
struct Guarded {
    std::vector<unsigned char> mem;
    size_t bytes;
    explicit Guarded(size_t b, unsigned char fill = kFresh) : mem(b + 2 * kGuard, kGuardByte), bytes(b) { memset(data(), fill, b); }
    unsigned char* data() { return mem.data() + kGuard; }
    template <typename T> T* as() { return reinterpret_cast<T*>(data()); }
    bool guards_intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (mem[i] != kGuardByte || mem[kGuard + bytes + i] != kGuardByte) return false;
        return true;
    }
};

// the bytes from the first to the last element of `planes` planes of `rows` rows of n elements, rows
// `pitch` and planes `plane` elements apart: the last row ends with its n elements
inline size_t span(int64_t planes, int64_t plane, int64_t rows, int64_t pitch, int64_t n, size_t elem) {
    return (size_t)((planes - 1) * plane + (rows - 1) * pitch + n) * elem;
}
inline size_t span(int64_t rows, int64_t pitch, int64_t n, size_t elem) { return span(1, 0, rows, pitch, n, elem); }

// A block filled with kFresh before the call: every element of [p][r][0, n) overwritten (none still holds
// kFresh in every byte) iff `written`, every other element of the block -- between the rows, between
// the planes, behind the last plane -- untouched, the guards intact.
inline void check_written(Guarded& g, int64_t planes, int64_t plane, int64_t rows, int64_t pitch, int64_t n, size_t elem,
                          bool written, const char* what) {
    EXPECT(g.guards_intact());
    std::vector<unsigned char> fresh(elem, kFresh);
    const int64_t total = (int64_t)(g.bytes / elem);
    for (int64_t i = 0; i < total; ++i) {
        const int64_t p = i / plane, in_plane = i - p * plane, r = in_plane / pitch, c = in_plane - r * pitch;
        const bool inside = written && p < planes && r < rows && c < n;
        const bool same = memcmp(g.data() + (size_t)i * elem, fresh.data(), elem) == 0;
        if (same == inside) {
            fprintf(stderr, HARNESS_NAME ": %s, element %lld (plane %lld row %lld column %lld): %s\n", what, (long long)i,
                    (long long)p, (long long)r, (long long)c, same ? "not overwritten" : "padding overwritten");
            exit(1);
        }
    }
}
// rows x pitch elements
inline void check_written(Guarded& g, int64_t rows, int64_t pitch, int64_t n, size_t elem, bool written, const char* what) {
    check_written(g, 1, rows * pitch, rows, pitch, n, elem, written, what);
}
// the whole block, one row
inline void check_written(Guarded& g, size_t elem, bool written, const char* what) {
    const int64_t n = (int64_t)(g.bytes / elem);
    check_written(g, 1, n, 1, n, n, elem, written, what);
}

// a block that knows its shape
struct Shaped : Guarded {
    int64_t planes, plane, rows, pitch, n;
    size_t elem;
    Shaped(int64_t planes_, int64_t plane_, int64_t rows_, int64_t pitch_, int64_t n_, size_t elem_, unsigned char fill)
        : Guarded(span(planes_, plane_, rows_, pitch_, n_, elem_), fill), planes(planes_), plane(plane_), rows(rows_),
          pitch(pitch_), n(n_), elem(elem_) {}
    Shaped(int64_t rows_, int64_t pitch_, int64_t n_, size_t elem_, unsigned char fill)
        : Shaped(1, rows_ * pitch_, rows_, pitch_, n_, elem_, fill) {}
    void check(bool written, const char* what) { check_written(*this, planes, plane, rows, pitch, n, elem, written, what); }
};

// the call was refused as an argument error whose message starts with `prefix` and contains `part`
inline bool refused(mod16_ctx* ctx, int rc, const char* prefix, const char* part) {
    const char* msg = mod16_last_error(ctx);
    return rc == MOD16_ERR_ARG && strncmp(msg, prefix, strlen(prefix)) == 0 && strstr(msg, part) != nullptr;
}

// the end of every main: the context goes (NULL: it went already), nothing the library allocated is left
inline void harness_finish(mod16_ctx* ctx) {
    EXPECT(mod16_destroy(ctx) == MOD16_OK);
    mod16_stub_report(stdout);
    EXPECT(mod16_stub_live_allocations() == 0);
    printf(HARNESS_NAME ": ok\n");
}
