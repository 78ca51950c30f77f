// Drives the HOST half of libmod16hip -- built with AddressSanitizer + UndefinedBehaviorSanitizer
// against tests/host_asan/hip_stub.hip -- through the C ABI (include/mod16_hip.h): ragged sizes,
// every form, every raster layout, bad layouts, more than 2^31 pixels, graphs, the HOST-mode tiler
// with its staging threads, the resident calibration problem. "Device" memory is host heap or (large
// rasters) an address-space reservation; kernel launches run their shadows (address arithmetic only).
// Exit code 0 and "host_asan: ok" = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#define HARNESS_NAME "host_asan"
#include "harness.hpp"      // the stand-in's declarations; this program's EXPECT and OK count their checks

static int g_checks = 0;
#undef EXPECT
#define EXPECT(cond)                                                                      \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) { fprintf(stderr, "host_asan: %s:%d: %s failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)
#define OK(call)                                                                           \
    do {                                                                                   \
        ++g_checks;                                                                        \
        int rc_ = (call);                                                                  \
        if (rc_ != MOD16_OK) { fprintf(stderr, "host_asan: %s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, mod16_last_error(ctx)); exit(1); } \
    } while (0)

static void* dmalloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess || !p) { fprintf(stderr, "host_asan: no memory for %zu bytes\n", bytes); exit(1); }
    return p;
}

template <typename T> struct TypeOps;
template <> struct TypeOps<double> {
    static constexpr int V = 2;
    static int et(mod16_ctx* c, const uint8_t* cls, const double* const* d, const int64_t* ds, const double* const* p, const int64_t* ps,
                  int64_t n, double* a, double* b, double* const* sep, unsigned f, int w) { return mod16_et_f64(c, cls, d, ds, p, ps, n, a, b, sep, f, w, nullptr); }
    static int tiled(mod16_ctx* c, const mod16_layout* l, const uint8_t* cls, const double* const* d, int64_t n, double* a, double* b, unsigned f, double* dd) { return mod16_et_tiled_f64(c, l, cls, d, n, a, b, f, dd, nullptr); }
    static int form(mod16_ctx* c, const mod16_layout* l, int form, const uint8_t* const* by, const double* const* w, double* const* o, int64_t n, unsigned f) { return mod16_et_form_tiled_f64(c, l, form, by, w, o, 12.0, n, f, nullptr); }
    static int graph(mod16_ctx* c, const mod16_layout* l, const uint8_t* cls, const double* const* d, int64_t n, double* a, double* b, unsigned f, double* dd, mod16_graph** g) { return mod16_graph_et_tiled_f64(c, l, cls, d, n, a, b, f, dd, g); }
    static int synth(mod16_ctx* c, const mod16_layout* l, int64_t n, uint8_t* cls, double* const* d) { return mod16_synth_tiled_f64(c, l, 16, 0, 0, n, cls, d, nullptr); }
    static int diag(mod16_ctx* c, const uint8_t* cls, const double* const* d, const int64_t* ds, int64_t n, double* a, double* b, unsigned f, double* dd) { return mod16_et_diag_f64(c, cls, d, ds, n, a, b, f, dd, nullptr); }
    static int method(mod16_ctx* c, int m, const double* const* in, const int64_t* is, const double* const* p, const int64_t* ps, int64_t n, double* const* o) { return mod16_method_f64(c, m, in, is, p, ps, n, o, 1.26, 1e-7, MOD16_HOST, nullptr); }
    static int stat(mod16_ctx* c, const double* const* d, const int64_t* ds, const double* const* p, const int64_t* ps, const double* const* rc, const int64_t* rs,
                    int64_t n, double* a, double* b) { return mod16_et_static_f64(c, d, ds, p, ps, rc, rs, n, a, b, 1e-7, MOD16_HOST, nullptr); }
};
template <> struct TypeOps<float> {
    static constexpr int V = 4;
    static int et(mod16_ctx* c, const uint8_t* cls, const float* const* d, const int64_t* ds, const float* const* p, const int64_t* ps,
                  int64_t n, float* a, float* b, float* const* sep, unsigned f, int w) { return mod16_et_f32(c, cls, d, ds, p, ps, n, a, b, sep, f, w, nullptr); }
    static int tiled(mod16_ctx* c, const mod16_layout* l, const uint8_t* cls, const float* const* d, int64_t n, float* a, float* b, unsigned f, double* dd) { return mod16_et_tiled_f32(c, l, cls, d, n, a, b, f, dd, nullptr); }
    static int form(mod16_ctx* c, const mod16_layout* l, int form, const uint8_t* const* by, const float* const* w, float* const* o, int64_t n, unsigned f) { return mod16_et_form_tiled_f32(c, l, form, by, w, o, 12.0, n, f, nullptr); }
    static int graph(mod16_ctx* c, const mod16_layout* l, const uint8_t* cls, const float* const* d, int64_t n, float* a, float* b, unsigned f, double* dd, mod16_graph** g) { return mod16_graph_et_tiled_f32(c, l, cls, d, n, a, b, f, dd, g); }
    static int synth(mod16_ctx* c, const mod16_layout* l, int64_t n, uint8_t* cls, float* const* d) { return mod16_synth_tiled_f32(c, l, 16, 0, 0, n, cls, d, nullptr); }
    static int diag(mod16_ctx* c, const uint8_t* cls, const float* const* d, const int64_t* ds, int64_t n, float* a, float* b, unsigned f, double* dd) { return mod16_et_diag_f32(c, cls, d, ds, n, a, b, f, dd, nullptr); }
    static int method(mod16_ctx* c, int m, const float* const* in, const int64_t* is, const float* const* p, const int64_t* ps, int64_t n, float* const* o) { return mod16_method_f32(c, m, in, is, p, ps, n, o, 1.26f, 1e-7f, MOD16_HOST, nullptr); }
    static int stat(mod16_ctx* c, const float* const* d, const int64_t* ds, const float* const* p, const int64_t* ps, const float* const* rc, const int64_t* rs,
                    int64_t n, float* a, float* b) { return mod16_et_static_f32(c, d, ds, p, ps, rc, rs, n, a, b, 1e-7f, MOD16_HOST, nullptr); }
};

// A tiled raster of one form: [tile][field][tile pixels] as mod16_amd/raster.py lays it out
template <typename T> struct Raster {
    mod16_layout lay;
    int64_t n, ntiles;
    char* slab;
    std::vector<const T*> wide;
    std::vector<T*> outs;
    std::vector<const uint8_t*> bytes;
    Raster(int64_t n_, int64_t tile, int nw, int nb, int no, int64_t extra_row = 0) : n(n_) {
        ntiles = (n + tile - 1) / tile;
        if (ntiles < 1) ntiles = 1;
        const int64_t wrow = nw * tile + extra_row, orow = no * tile + extra_row, brow = nb * tile + extra_row;
        const size_t wb = (size_t)ntiles * wrow * sizeof(T), ob = (size_t)ntiles * orow * sizeof(T), bb = (size_t)ntiles * brow;
        slab = static_cast<char*>(dmalloc(wb + ob + bb + 4096));
        lay = mod16_layout{tile, wrow, orow, brow};
        for (int k = 0; k < nw; ++k) wide.push_back(reinterpret_cast<const T*>(slab) + k * tile);
        for (int k = 0; k < no; ++k) outs.push_back(reinterpret_cast<T*>(slab + wb) + k * tile);
        for (int k = 0; k < nb; ++k) bytes.push_back(reinterpret_cast<const uint8_t*>(slab + wb + ob) + k * tile);
    }
    ~Raster() { (void)hipFree(slab); }
};

template <typename T>
static void tiled_cases(mod16_ctx* ctx, const char* what) {
    constexpr int V = TypeOps<T>::V;
    double* ddiag = static_cast<double*>(dmalloc(64));
    const int64_t tile = 32768 / (int64_t)sizeof(T);
    // sizes: one piece, ragged ends, a 1200 x 1200 tile (static schedule), the global grid and more than 2^31 pixels
    const int64_t sizes[] = {V, 64 * V, 64 * V + V, tile - V, tile, tile + V, 1200 * 1200, 7 * tile + 5 * V,
                             (int64_t)43200 * 21600, ((int64_t)1 << 31) + 12344};
    for (int64_t n : sizes) {
        Raster<T> r(n, tile, 14, 1, 2);
        OK(TypeOps<T>::synth(ctx, &r.lay, n, const_cast<uint8_t*>(r.bytes[0]), reinterpret_cast<T* const*>(const_cast<T**>(const_cast<const T**>(r.wide.data())))));
        OK(TypeOps<T>::tiled(ctx, &r.lay, r.bytes[0], r.wide.data(), n, r.outs[0], r.outs[1], MOD16_MATH_FAST, ddiag));
        OK(TypeOps<T>::tiled(ctx, &r.lay, r.bytes[0], r.wide.data(), n, r.outs[0], r.outs[1], MOD16_MATH_FAST | MOD16_DOMAIN_TRUSTED, nullptr));
        if (sizeof(T) == 4) OK(TypeOps<T>::tiled(ctx, &r.lay, r.bytes[0], r.wide.data(), n, r.outs[0], r.outs[1], MOD16_MATH_MIXED, ddiag));
        mod16_graph* g = nullptr;
        OK(TypeOps<T>::graph(ctx, &r.lay, r.bytes[0], r.wide.data(), n, r.outs[0], r.outs[1], MOD16_MATH_FAST, ddiag, &g));
        EXPECT(mod16_graph_launch(g, nullptr) == MOD16_OK);
        float ms = 0;
        EXPECT(mod16_time_graph(g, 2, nullptr, &ms) == MOD16_OK);
        EXPECT(mod16_graph_destroy(g) == MOD16_OK);
        OK(mod16_check_status(ctx, nullptr));
    }
    // rows wider than the tile (a padded pitch), other tile sizes
    for (int64_t tl : {tile / 4, tile * 2, tile * 16}) {
        Raster<T> r(5 * tl + 3 * V, tl, 14, 1, 2, 64);
        OK(TypeOps<T>::tiled(ctx, &r.lay, r.bytes[0], r.wide.data(), r.n, r.outs[0], r.outs[1], MOD16_MATH_FAST, ddiag));
    }
    // every form on the tiled layout
    for (int form = MOD16_FORM_TOTALS; form <= MOD16_FORM_RAW_TOTAL8_HOURS; ++form) {
        int nw, nb, no;
        EXPECT(mod16_form_shape(form, &nw, &nb, &no) == MOD16_OK);
        for (int64_t n : {(int64_t)(3 * tile + 7 * V), (int64_t)10800 * 43200}) {
            Raster<T> r(n, tile, nw, nb, no);
            OK(TypeOps<T>::form(ctx, &r.lay, form, r.bytes.data(), r.wide.data(), r.outs.data(), n, MOD16_MATH_FAST));
            if (sizeof(T) == 4) OK(TypeOps<T>::form(ctx, &r.lay, form, r.bytes.data(), r.wide.data(), r.outs.data(), n, MOD16_MATH_MIXED));
        }
    }
    int dummy;
    EXPECT(mod16_form_shape(99, &dummy, &dummy, &dummy) == MOD16_ERR_ARG);
    // layouts that must be refused: tile not a power of two / too small, rows narrower than the tile or
    // not a multiple of the vector width, misaligned bases, n not a multiple of the vector width
    {
        Raster<T> r(4 * tile, tile, 14, 1, 2);
        auto bad = [&](mod16_layout lay, const uint8_t* cls, const T* const* w, int64_t n, T* day) {
            return TypeOps<T>::tiled(ctx, &lay, cls, w, n, day, r.outs[1], MOD16_MATH_FAST, ddiag);
        };
        mod16_layout l = r.lay;
        l.tile = tile - 64; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        l = r.lay; l.tile = 64; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        l = r.lay; l.driver_row = tile - V; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        l = r.lay; l.out_row += 1; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        l = r.lay; l.cls_row = 0; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        // what the pipeline kernel's 32-bit scalars cannot hold (round 6): more than 2^30 pieces of 64 vectors,
        // a row between tiles of 2^32 elements -- refused before anything is launched
        EXPECT(bad(r.lay, r.bytes[0], r.wide.data(), (((int64_t)1 << 30) + 1) * 64 * V, r.outs[0]) == MOD16_ERR_ARG);
        l = r.lay; l.driver_row = (int64_t)1 << 32; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        l = r.lay; l.out_row = (int64_t)1 << 32; EXPECT(bad(l, r.bytes[0], r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        EXPECT(bad(r.lay, r.bytes[0] + 1, r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        EXPECT(bad(r.lay, r.bytes[0], r.wide.data(), r.n - 1, r.outs[0]) == MOD16_ERR_ARG);
        EXPECT(bad(r.lay, r.bytes[0], r.wide.data(), r.n, r.outs[0] + 1) == MOD16_ERR_ARG);
        std::vector<const T*> w = r.wide;
        w[3] += 1; EXPECT(bad(r.lay, r.bytes[0], w.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        w[3] = nullptr; EXPECT(bad(r.lay, r.bytes[0], w.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        EXPECT(bad(r.lay, nullptr, r.wide.data(), r.n, r.outs[0]) == MOD16_ERR_ARG);
        EXPECT(TypeOps<T>::tiled(ctx, &r.lay, r.bytes[0], r.wide.data(), r.n, r.outs[0], r.outs[1], MOD16_MATH_EXACT, ddiag) == MOD16_ERR_ARG);
        EXPECT(TypeOps<T>::tiled(ctx, &r.lay, r.bytes[0], r.wide.data(), 0, r.outs[0], r.outs[1], MOD16_MATH_FAST, ddiag) == MOD16_OK);
    }
    (void)hipFree(ddiag);
    printf("host_asan: tiled rasters, %s: done\n", what);
}

// plain device arrays: aligned slab (pitched), scattered, misaligned (scalar kernels), scalars, ragged n
template <typename T>
static void plain_device_cases(mod16_ctx* ctx, const char* what) {
    constexpr int V = TypeOps<T>::V;
    double* ddiag = static_cast<double*>(dmalloc(64));
    for (int64_t n : {(int64_t)1, (int64_t)V - 1, (int64_t)64 * V + 1, (int64_t)1200 * 1200, (int64_t)1200 * 1200 + 3, (int64_t)2700 * 43200}) {
        const size_t per = ((size_t)n * sizeof(T) + 4095) / 4096 * 4096 + 33 * 1024;
        char* slab = static_cast<char*>(dmalloc(16 * per + n + 4096));
        const T* drv[14];
        int64_t ds[14];
        for (int k = 0; k < 14; ++k) { drv[k] = reinterpret_cast<const T*>(slab + k * per); ds[k] = 1; }
        T* day = reinterpret_cast<T*>(slab + 14 * per);
        T* night = reinterpret_cast<T*>(slab + 15 * per);
        const uint8_t* cls = reinterpret_cast<const uint8_t*>(slab + 16 * per);
        OK(TypeOps<T>::diag(ctx, cls, drv, ds, n, day, night, MOD16_MATH_FAST, ddiag));
        OK(TypeOps<T>::et(ctx, cls, drv, ds, nullptr, nullptr, n, day, night, nullptr, MOD16_MATH_EXACT, MOD16_DEVICE));
        // a broadcast scalar among the drivers, and a misaligned one: the plain kernels
        T* scalar = static_cast<T*>(dmalloc(sizeof(T)));
        const T* d2[14];
        int64_t s2[14];
        for (int k = 0; k < 14; ++k) { d2[k] = drv[k]; s2[k] = 1; }
        d2[7] = scalar; s2[7] = 0;
        OK(TypeOps<T>::diag(ctx, cls, d2, s2, n, day, night, MOD16_MATH_FAST, ddiag));
        if (n > 8) {
            d2[7] = drv[7] + 1; s2[7] = 1;
            OK(TypeOps<T>::et(ctx, cls, d2, s2, nullptr, nullptr, n - 1, day, night, nullptr, MOD16_MATH_FAST, MOD16_DEVICE));
        }
        (void)hipFree(scalar);
        // components and per-pixel parameter arrays
        std::vector<T*> sep(6);
        std::vector<const T*> par(11);
        std::vector<int64_t> ps(11, 1);
        char* extra = static_cast<char*>(dmalloc(17 * per));
        for (int k = 0; k < 6; ++k) sep[k] = reinterpret_cast<T*>(extra + k * per);
        for (int k = 0; k < 11; ++k) par[k] = reinterpret_cast<const T*>(extra + (6 + k) * per);
        OK(TypeOps<T>::et(ctx, cls, drv, ds, nullptr, nullptr, n, day, night, sep.data(), MOD16_MATH_FAST, MOD16_DEVICE));
        OK(TypeOps<T>::et(ctx, cls, drv, ds, nullptr, nullptr, n, nullptr, nullptr, sep.data(), MOD16_MATH_FAST, MOD16_DEVICE));
        OK(TypeOps<T>::et(ctx, nullptr, drv, ds, par.data(), ps.data(), n, day, night, sep.data(), MOD16_MATH_FAST, MOD16_DEVICE));
        OK(mod16_check_status(ctx, nullptr));
        (void)hipFree(extra);
        (void)hipFree(slab);
    }
    EXPECT(TypeOps<T>::et(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, 4, nullptr, nullptr, nullptr, 0, MOD16_DEVICE) == MOD16_ERR_ARG);
    (void)hipFree(ddiag);
    printf("host_asan: plain device arrays, %s: done\n", what);
}

// HOST mode: host arrays staged through the slabs by the library's own threads
template <typename T>
static void host_cases(mod16_ctx* ctx, const char* what) {
    const int64_t tile = mod16_host_tile_pixels();
    for (int64_t n : {(int64_t)5, (int64_t)tile + 12345, (int64_t)3 * tile}) {
        std::vector<std::vector<T>> drv(14, std::vector<T>(n, T(1)));
        std::vector<uint8_t> cls(n, 1);
        std::vector<T> day(n), night(n);
        const T* dp[14];
        int64_t ds[14];
        for (int k = 0; k < 14; ++k) { dp[k] = drv[k].data(); ds[k] = 1; }
        OK(TypeOps<T>::et(ctx, cls.data(), dp, ds, nullptr, nullptr, n, day.data(), night.data(), nullptr, MOD16_MATH_FAST, MOD16_HOST));
        T one = T(300);
        dp[5] = &one; ds[5] = 0;                 // a broadcast scalar
        std::vector<double> tile_diag(8 * ((n + tile - 1) / tile), -1.0);
        if (sizeof(T) == 8)
            OK(mod16_et_hdiag_f64(ctx, cls.data(), reinterpret_cast<const double* const*>(dp), ds, nullptr, nullptr, n,
                                  reinterpret_cast<double*>(day.data()), reinterpret_cast<double*>(night.data()), MOD16_MATH_FAST, tile_diag.data()));
        else
            OK(mod16_et_hdiag_f32(ctx, cls.data(), reinterpret_cast<const float* const*>(dp), ds, nullptr, nullptr, n,
                                  reinterpret_cast<float*>(day.data()), reinterpret_cast<float*>(night.data()), MOD16_MATH_FAST, tile_diag.data()));
        double folded[8];
        EXPECT(mod16_fold_diag_host(tile_diag.data(), (int64_t)tile_diag.size() / 8, folded) == MOD16_OK);
    }
    // small calls: the copy-free path (page-locked buffer read and written by the kernel) up to its
    // limit, the staged path one pixel above it; parameters as arrays / scalars, every output set,
    // a class code the reference would refuse
    for (int64_t n : {(int64_t)1, (int64_t)365, (int64_t)1025, (int64_t)65535, (int64_t)65536, (int64_t)65537}) {
        std::vector<std::vector<T>> drv(14, std::vector<T>(n, T(1))), par(11, std::vector<T>(n, T(2)));
        std::vector<std::vector<T>> outs(6, std::vector<T>(n));
        std::vector<uint8_t> cls(n, 1);
        std::vector<T> day(n), night(n);
        const T *dp[14], *pp[11];
        int64_t ds[14], ps[11];
        T one = T(300);
        for (int k = 0; k < 14; ++k) { dp[k] = k % 3 ? drv[k].data() : &one; ds[k] = k % 3 ? 1 : 0; }
        for (int k = 0; k < 11; ++k) { pp[k] = k % 2 ? par[k].data() : &one; ps[k] = k % 2 ? 1 : 0; }
        T* sep[6];
        for (int k = 0; k < 6; ++k) sep[k] = outs[k].data();
        OK(TypeOps<T>::et(ctx, nullptr, dp, ds, pp, ps, n, day.data(), night.data(), nullptr, MOD16_MATH_FAST, MOD16_HOST));
        OK(TypeOps<T>::et(ctx, nullptr, dp, ds, pp, ps, n, nullptr, nullptr, sep, MOD16_MATH_EXACT, MOD16_HOST));
        OK(TypeOps<T>::et(ctx, cls.data(), dp, ds, nullptr, nullptr, n, day.data(), night.data(), sep, MOD16_MATH_FAST, MOD16_HOST));
        if (n <= 65536) {    // (above it the kernel reports the code; the stand-in's kernels report nothing)
            cls[n - 1] = 13;
            EXPECT(TypeOps<T>::et(ctx, cls.data(), dp, ds, nullptr, nullptr, n, day.data(), night.data(), nullptr, MOD16_MATH_FAST, MOD16_HOST) == MOD16_ERR_CLASS_RANGE);
        }
    }
    // raw drivers through the same staging (threads and slots since round 5), hours dense / scalar / absent
    for (int64_t n : {(int64_t)7, (int64_t)2 * tile + 4321}) {
        std::vector<std::vector<T>> raw(14, std::vector<T>(n, T(280)));
        std::vector<uint8_t> cls(n, 1), fpar(n, 50), lai(n, 20);
        std::vector<T> day(n), night(n), total(n), hours(n, T(12));
        const T* rp[14];
        int64_t rs[14];
        for (int k = 0; k < 14; ++k) { rp[k] = raw[k].data(); rs[k] = 1; }
        T elev = T(350);
        rp[13] = &elev; rs[13] = 0;
        if (sizeof(T) == 8) {
            auto R = reinterpret_cast<const double* const*>(rp);
            OK(mod16_et_raw_f64(ctx, cls.data(), R, rs, fpar.data(), lai.data(), reinterpret_cast<const double*>(hours.data()), 1, n,
                                reinterpret_cast<double*>(day.data()), reinterpret_cast<double*>(night.data()), reinterpret_cast<double*>(total.data()), MOD16_MATH_FAST, MOD16_HOST, nullptr));
            OK(mod16_et_raw_f64(ctx, cls.data(), R, rs, fpar.data(), lai.data(), reinterpret_cast<const double*>(hours.data()), 0, n,
                                reinterpret_cast<double*>(day.data()), reinterpret_cast<double*>(night.data()), reinterpret_cast<double*>(total.data()), MOD16_MATH_FAST, MOD16_HOST, nullptr));
            OK(mod16_et_raw_f64(ctx, cls.data(), R, rs, fpar.data(), lai.data(), nullptr, 0, n,
                                reinterpret_cast<double*>(day.data()), reinterpret_cast<double*>(night.data()), nullptr, MOD16_MATH_EXACT, MOD16_HOST, nullptr));
        } else {
            auto R = reinterpret_cast<const float* const*>(rp);
            OK(mod16_et_raw_f32(ctx, cls.data(), R, rs, fpar.data(), lai.data(), reinterpret_cast<const float*>(hours.data()), 1, n,
                                reinterpret_cast<float*>(day.data()), reinterpret_cast<float*>(night.data()), reinterpret_cast<float*>(total.data()), MOD16_MATH_MIXED, MOD16_HOST, nullptr));
            OK(mod16_et_raw_f32(ctx, cls.data(), R, rs, fpar.data(), lai.data(), nullptr, 0, n,
                                reinterpret_cast<float*>(day.data()), reinterpret_cast<float*>(night.data()), nullptr, MOD16_MATH_FAST, MOD16_HOST, nullptr));
        }
    }
    // the class-surface methods: the small path, and tile by tile on one slot; inputs dense and scalar,
    // optional inputs and parameters absent
    for (int64_t n : {(int64_t)5, (int64_t)tile + 12345}) {
        std::vector<std::vector<T>> in(6, std::vector<T>(n, T(280)));
        std::vector<T> par(n, T(2)), sat(n), unsat(n);
        T pa = T(90000);
        const T* ip[13] = {&pa, in[1].data(), in[2].data(), in[3].data(), in[4].data(), nullptr, nullptr, in[5].data()};
        int64_t is[13] = {0, 1, 1, 1, 1, 0, 0, 1};
        const T* pp[11] = {};
        int64_t ps[11] = {};
        pp[3] = par.data(); ps[3] = 1;
        pp[4] = &pa;
        T* outs[2] = {sat.data(), unsat.data()};
        OK(TypeOps<T>::method(ctx, MOD16_M_POT_SOIL_EVAP, ip, is, pp, ps, n, outs));
        const T* rh[13] = {in[1].data(), &pa};
        int64_t rhs[13] = {1, 0};
        outs[1] = nullptr;
        OK(TypeOps<T>::method(ctx, MOD16_M_RHUMIDITY, rh, rhs, nullptr, nullptr, n, outs));
    }
    {   // the calibration path's small calls: with and without r_corr_list, scalars among every kind
        const int64_t n = 365;
        std::vector<std::vector<T>> drv(14, std::vector<T>(n, T(280))), par(11, std::vector<T>(n, T(2)));
        std::vector<T> rc(n, T(1)), day(n), night(n);
        const T *dp[14], *pp[11];
        int64_t ds[14], ps[11];
        T one = T(300);
        for (int k = 0; k < 14; ++k) { dp[k] = k % 4 ? drv[k].data() : &one; ds[k] = k % 4 ? 1 : 0; }
        for (int k = 0; k < 11; ++k) { pp[k] = k % 3 ? par[k].data() : &one; ps[k] = k % 3 ? 1 : 0; }
        const T* rp[2] = {rc.data(), &one};
        int64_t rs[2] = {1, 0};
        OK(TypeOps<T>::stat(ctx, dp, ds, pp, ps, rp, rs, n, day.data(), night.data()));
        OK(TypeOps<T>::stat(ctx, dp, ds, pp, ps, nullptr, nullptr, n, day.data(), night.data()));
    }
    double x[8];
    EXPECT(mod16_fold_diag_host(nullptr, 1, x) == MOD16_ERR_ARG);
    EXPECT(mod16_fold_diag_host(x, 0, x) == MOD16_ERR_ARG);
    printf("host_asan: HOST mode, %s: done\n", what);
}

// ---- the calibration family under its shadows: a resident problem's workspaces as they grow, the
// sampler that owns its own, folds, float32 and EXACT problems, DEVICE-mode arrays, many draws
template <typename T> struct Problem {
    int64_t n;
    std::vector<std::vector<T>> drv;
    std::vector<T> obs, wts;
    const T* dp[14];
    int64_t ds[14];
    explicit Problem(int64_t n_) : n(n_), drv(14, std::vector<T>(n_, T(280))), obs(n_, T(10)), wts(n_, T(1)) {
        for (int k = 0; k < 14; ++k) { dp[k] = drv[k].data(); ds[k] = 1; }
        ds[7] = 0;      // a broadcast scalar among the drivers
    }
};

static mod16_mcmc_spec sampler_spec(int chains, int segment) {
    mod16_mcmc_spec s;
    memset(&s, 0, sizeof s);
    s.chains = chains;
    s.nfree = 2;
    s.index[0] = 4; s.family[0] = MOD16_PRIOR_UNIFORM; s.p0[0] = 0.0; s.p1[0] = 1.0;
    s.index[1] = 10; s.family[1] = MOD16_PRIOR_LOGNORMAL; s.p0[1] = 0.0; s.p1[1] = 1.0;
    for (int k = 0; k < 11; ++k) s.fixed[k] = 1.0;
    s.lamb = 0.8;
    s.scaling = 0.001;
    s.tune_target = 1;
    s.tune_interval = 10;
    s.tune_steps = 20;
    s.tune_drop_fraction = 0.5;
    s.segment = segment;
    s.seed = 42;
    return s;
}

static void calibration_cases(mod16_ctx* ctx) {
    const int64_t n = 1000, maxd = 300;
    Problem<double> p(n);
    std::vector<double> par(maxd * 11, 1.0), sse(maxd), cnt(maxd);
    float ms = 0;
    {   // float64, FAST, bound for many more draws than the first calls bring
        mod16_batch* b = nullptr;
        OK(mod16_static_batch_bind_f64(ctx, p.dp, p.ds, n, p.obs.data(), p.wts.data(), maxd, MOD16_MATH_FAST, MOD16_HOST, &b));
        int64_t outside = -1;
        OK(mod16_static_batch_info(b, nullptr, nullptr, &outside));
        EXPECT(outside == n);       // (the stand-in's mask lists every pixel: the redo kernels launch)
        EXPECT(mod16_static_batch_time(b, 1, &ms) == MOD16_ERR_ARG);      // no objective call yet
        OK(mod16_static_batch_objective(b, par.data(), 7, sse.data(), cnt.data()));
        // a sampler created BEFORE the problem's per-block workspace grows and run AFTER it: its graphs
        // must hold its own workspace, not the problem's
        mod16_mcmc_spec spec = sampler_spec(5, 4);
        mod16_mcmc *m1 = nullptr, *m2 = nullptr;
        OK(mod16_mcmc_create(b, &spec, nullptr, &m1));
        OK(mod16_static_batch_objective(b, par.data(), 100, sse.data(), cnt.data()));    // 64 -> 128 draws: graphs dropped
        OK(mod16_static_batch_objective(b, par.data(), 7, sse.data(), cnt.data()));      // ... and captured again
        OK(mod16_static_batch_time(b, 2, &ms));
        OK(mod16_mcmc_run(m1, 10, &ms));                // two segments and a remainder of 2
        OK(mod16_static_batch_objective(b, par.data(), maxd, sse.data(), cnt.data()));   // grows to max_draws, not to 512
        OK(mod16_mcmc_run(m1, 7, nullptr));             // the trace is outgrown (copied over, graphs dropped); remainder 3
        OK(mod16_mcmc_run(m1, 9, nullptr));             // remainder 1
        OK(mod16_mcmc_run(m1, 0, nullptr));
        {
            const int64_t t0 = 5, count = 12;
            std::vector<double> x(count * 5 * 2), y(count * 5 * 2), ll(count * 5), lp(count * 5), sc(5), lamb(5);
            std::vector<uint8_t> acc(count * 5);
            int64_t steps = -1;
            OK(mod16_mcmc_read(m1, t0, count, x.data(), y.data(), ll.data(), lp.data(), acc.data(), sc.data(), lamb.data(), &steps));
            EXPECT(steps == 26);
            EXPECT(mod16_mcmc_read(m1, 20, 7, x.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MOD16_ERR_ARG);
        }
        // a second sampler (given initial values, the default segment) on the same problem
        mod16_mcmc_spec spec2 = sampler_spec(3, 0);
        std::vector<double> x0(3 * 2, 0.5);
        OK(mod16_mcmc_create(b, &spec2, x0.data(), &m2));
        OK(mod16_mcmc_run(m2, 70, nullptr));            // one segment of 64 and 6
        OK(mod16_mcmc_run(m1, 4, nullptr));             // the first one's graphs are its own
        std::vector<uint8_t> labels(n);
        for (int64_t i = 0; i < n; ++i) labels[i] = (uint8_t)(i % 3);
        EXPECT(mod16_static_batch_set_folds(b, labels.data(), 3) == MOD16_ERR_ARG);     // a sampler lives
        mod16_mcmc* bad = nullptr;
        x0[3] = -1.0;
        EXPECT(mod16_mcmc_create(b, &spec2, x0.data(), &bad) == MOD16_ERR_ARG && !bad);  // outside the prior's support
        spec2.chains = (int)maxd + 1;
        EXPECT(mod16_mcmc_create(b, &spec2, nullptr, &bad) == MOD16_ERR_ARG && !bad);
        // two samplers on one problem, destroyed in either order (always before the problem)
        EXPECT(mod16_mcmc_destroy(m1) == MOD16_OK);
        EXPECT(mod16_mcmc_destroy(m2) == MOD16_OK);
        OK(mod16_mcmc_create(b, &spec, nullptr, &m1));
        spec2 = sampler_spec(3, 7);
        OK(mod16_mcmc_create(b, &spec2, nullptr, &m2));
        OK(mod16_mcmc_run(m2, 7, nullptr));             // exactly one segment: no remainder graph
        EXPECT(mod16_mcmc_destroy(m2) == MOD16_OK);
        EXPECT(mod16_mcmc_destroy(m1) == MOD16_OK);
        // folds, now that no sampler lives: plain and fold calls keep a graph each
        OK(mod16_static_batch_set_folds(b, labels.data(), 3));
        EXPECT(mod16_static_batch_set_folds(b, labels.data(), 3) == MOD16_ERR_ARG);     // once per problem
        std::vector<int32_t> code(maxd);
        for (int64_t d = 0; d < maxd; ++d) code[d] = (int32_t)(d % 3) | ((d & 1) ? MOD16_FOLD_HELDOUT : 0);
        OK(mod16_static_batch_objective_folds(b, par.data(), 40, code.data(), sse.data(), cnt.data()));
        OK(mod16_static_batch_objective(b, par.data(), 40, sse.data(), cnt.data()));
        OK(mod16_static_batch_objective_folds(b, par.data(), 40, code.data(), sse.data(), cnt.data()));
        OK(mod16_static_batch_objective_folds(b, par.data(), 9, code.data(), sse.data(), cnt.data()));
        OK(mod16_static_batch_objective(b, par.data(), 40, sse.data(), cnt.data()));
        OK(mod16_static_batch_time(b, 1, &ms));
        code[3] = 3;
        EXPECT(mod16_static_batch_objective_folds(b, par.data(), 9, code.data(), sse.data(), cnt.data()) == MOD16_ERR_ARG);
        code[3] = 1 | 0x200;
        EXPECT(mod16_static_batch_objective_folds(b, par.data(), 9, code.data(), sse.data(), cnt.data()) == MOD16_ERR_ARG);
        code[3] = MOD16_FOLD_HELDOUT;
        // every fold in one sampler: two groups of four chains
        int32_t folds[2] = {2, 0};
        mod16_mcmc_spec spec3 = sampler_spec(4, 3);
        OK(mod16_mcmc_create_groups(b, &spec3, 2, folds, nullptr, &m1));
        OK(mod16_mcmc_run(m1, 8, &ms));
        OK(mod16_static_batch_objective_folds(b, par.data(), maxd, code.data(), sse.data(), cnt.data()));
        OK(mod16_mcmc_run(m1, 3, nullptr));
        folds[1] = 2;
        EXPECT(mod16_mcmc_create_groups(b, &spec3, 2, folds, nullptr, &bad) == MOD16_ERR_ARG && !bad);    // a fold twice
        folds[1] = 3;
        EXPECT(mod16_mcmc_create_groups(b, &spec3, 2, folds, nullptr, &bad) == MOD16_ERR_ARG && !bad);
        EXPECT(mod16_mcmc_destroy(m1) == MOD16_OK);
        std::vector<double> day(7 * n), total(7 * n);
        OK(mod16_static_batch_rows(b, par.data(), 7, day.data(), nullptr, total.data()));
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
    }
    {   // float32 (no folds, no sampler), without weights
        Problem<float> q(n);
        std::vector<float> par32(16 * 11, 1.0f), rows(5 * n);
        mod16_batch* b = nullptr;
        OK(mod16_static_batch_bind_f32(ctx, q.dp, q.ds, n, q.obs.data(), nullptr, 16, MOD16_MATH_FAST, MOD16_HOST, &b));
        OK(mod16_static_batch_objective(b, par32.data(), 5, sse.data(), cnt.data()));
        OK(mod16_static_batch_rows(b, par32.data(), 5, nullptr, rows.data(), nullptr));
        std::vector<uint8_t> labels(n, 0);
        labels[0] = 1;
        EXPECT(mod16_static_batch_set_folds(b, labels.data(), 2) == MOD16_ERR_ARG);
        mod16_mcmc_spec spec = sampler_spec(2, 0);
        mod16_mcmc* bad = nullptr;
        EXPECT(mod16_mcmc_create(b, &spec, nullptr, &bad) == MOD16_ERR_ARG && !bad);
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
    }
    {   // EXACT: the rows workspace through objective and through rows, growing
        std::vector<double> rows(3 * 9 * n);
        mod16_batch* b = nullptr;
        OK(mod16_static_batch_bind_f64(ctx, p.dp, p.ds, n, p.obs.data(), p.wts.data(), 16, MOD16_MATH_EXACT, MOD16_HOST, &b));
        OK(mod16_static_batch_objective(b, par.data(), 3, sse.data(), cnt.data()));
        OK(mod16_static_batch_objective(b, par.data(), 9, sse.data(), cnt.data()));
        OK(mod16_static_batch_rows(b, par.data(), 9, rows.data(), rows.data() + 9 * n, rows.data() + 18 * n));
        OK(mod16_static_batch_rows(b, par.data(), 2, nullptr, rows.data(), nullptr));
        OK(mod16_static_batch_objective(b, par.data(), 9, sse.data(), cnt.data()));
        EXPECT(mod16_static_batch_time(b, 1, &ms) == MOD16_ERR_ARG);      // an EXACT problem has no graph
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
    }
    {   // DEVICE mode: the caller's device arrays, bound and unbound
        const size_t per = ((size_t)n * 8 + 255) / 256 * 256;
        char* slab = static_cast<char*>(dmalloc(17 * per + 9 * 11 * 8 + 9 * n * 8 + 2 * 9 * 8));
        const double* dp[14];
        for (int k = 0; k < 14; ++k) dp[k] = reinterpret_cast<const double*>(slab + k * per);
        const double* dobs = reinterpret_cast<const double*>(slab + 14 * per);
        const double* dw = reinterpret_cast<const double*>(slab + 15 * per);
        mod16_batch* b = nullptr;
        OK(mod16_static_batch_bind_f64(ctx, dp, p.ds, n, dobs, dw, 9, MOD16_MATH_FAST, MOD16_DEVICE, &b));
        OK(mod16_static_batch_objective(b, par.data(), 9, sse.data(), cnt.data()));
        std::vector<double> total(9 * n);
        OK(mod16_static_batch_rows(b, par.data(), 9, nullptr, nullptr, total.data()));
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
        double* dpar = reinterpret_cast<double*>(slab + 17 * per);
        double* dtotal = dpar + 9 * 11;
        double* dsse = dtotal + 9 * n;
        for (unsigned flags : {(unsigned)MOD16_MATH_FAST, (unsigned)MOD16_MATH_EXACT})
            OK(mod16_et_static_batch_f64(ctx, dp, p.ds, n, dpar, 9, nullptr, nullptr, dtotal, dobs, dw, dsse, dsse + 9, flags, MOD16_DEVICE, nullptr));
        (void)hipFree(slab);
    }
    {   // more draws than one launch takes (32768 block rows): the launches of a call cover them all
        const int64_t m = 2, ndraw = (int64_t)32768 * 32 + 5;
        Problem<double> q(m);
        std::vector<double> many((size_t)ndraw * 11, 1.0), s2(ndraw), c2(ndraw);
        OK(mod16_et_static_batch_f64(ctx, q.dp, q.ds, m, many.data(), ndraw, nullptr, nullptr, nullptr, q.obs.data(), nullptr, s2.data(),
                                     c2.data(), MOD16_MATH_FAST, MOD16_HOST, nullptr));
    }
    printf("host_asan: calibration family: done\n");
}

// ---- the annual-precipitation constraint: T x N = 6 x 3 pixels in years of 4 and 2 days (so every
// site-year is padded to 64 by a different amount), a pixel outside the FAST domain, one scalar driver
struct AnnualProblem {
    static constexpr int64_t T = 6, N = 3, n = T * N, maxd = 40;
    static constexpr int Y = 2;
    Problem<double> p;
    int32_t year[T] = {0, 0, 0, 0, 1, 1};
    std::vector<double> precip, lhv;
    AnnualProblem() : p(n), precip(Y * N, 500.0), lhv(n, 2.45e6) { p.drv[MOD16_PRESSURE][7] = 0.5; }
    int bind(mod16_ctx* ctx, bool weights, mod16_batch** b) {
        return mod16_static_batch_bind_f64(ctx, p.dp, p.ds, n, p.obs.data(), weights ? p.wts.data() : nullptr, maxd, MOD16_MATH_FAST, MOD16_HOST, b);
    }
    int set(mod16_batch* b) { return mod16_static_batch_set_annual(b, T, N, year, Y, precip.data(), lhv.data()); }
};

static void annual_cases(mod16_ctx* ctx) {
    AnnualProblem a;
    const int64_t n = a.n, maxd = a.maxd;
    std::vector<double> par(maxd * 11, 1.0), sse(maxd), cnt(maxd), pen(maxd);
    for (bool weights : {true, false}) {
        mod16_batch* b = nullptr;
        OK(a.bind(ctx, weights, &b));
        EXPECT(mod16_static_batch_objective_annual(b, par.data(), 9, sse.data(), cnt.data(), pen.data()) == MOD16_ERR_ARG);   // no constraint yet
        OK(a.set(b));
        int64_t n_user = -1, outside = -1;
        OK(mod16_static_batch_info(b, &n_user, nullptr, &outside));
        EXPECT(n_user == n && outside > 0);
        size_t live = mod16_stub_live_allocations();
        EXPECT(a.set(b) == MOD16_ERR_ARG);                          // once per problem
        EXPECT(mod16_stub_live_allocations() == live);
        OK(mod16_static_batch_objective_annual(b, par.data(), 40, sse.data(), cnt.data(), pen.data()));
        OK(mod16_static_batch_objective_annual(b, par.data(), 9, sse.data(), cnt.data(), pen.data()));     // captured again
        OK(mod16_static_batch_objective_annual(b, par.data(), 40, sse.data(), cnt.data(), pen.data()));
        OK(mod16_static_batch_objective(b, par.data(), 40, sse.data(), cnt.data()));                       // the plain graph of the same problem
        std::vector<double> day(9 * n), night(9 * n), total(9 * n);
        OK(mod16_static_batch_rows(b, par.data(), 9, day.data(), night.data(), total.data()));              // gathered through pos
        mod16_mcmc_spec spec = sampler_spec(5, 4);
        spec.constraints = MOD16_CONSTRAINT_ANNUAL_PRECIP;
        mod16_mcmc* m = nullptr;
        OK(mod16_mcmc_create(b, &spec, nullptr, &m));
        OK(mod16_mcmc_run(m, 9, nullptr));              // the trace grows once; two segments and a remainder of 1
        EXPECT(mod16_mcmc_destroy(m) == MOD16_OK);
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
    }
    {   // refused: after folds, and while a sampler lives -- nothing allocated, nothing freed
        std::vector<uint8_t> labels(n);
        for (int64_t i = 0; i < n; ++i) labels[i] = (uint8_t)(i % 3);
        mod16_batch* b = nullptr;
        OK(a.bind(ctx, true, &b));
        OK(mod16_static_batch_set_folds(b, labels.data(), 3));
        size_t live = mod16_stub_live_allocations();
        EXPECT(a.set(b) == MOD16_ERR_ARG);
        EXPECT(mod16_stub_live_allocations() == live);
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
        OK(a.bind(ctx, true, &b));
        mod16_mcmc_spec spec = sampler_spec(5, 4);
        mod16_mcmc* m = nullptr;
        OK(mod16_mcmc_create(b, &spec, nullptr, &m));
        live = mod16_stub_live_allocations();
        EXPECT(a.set(b) == MOD16_ERR_ARG);
        EXPECT(mod16_stub_live_allocations() == live);
        spec.constraints = MOD16_CONSTRAINT_ANNUAL_PRECIP;
        mod16_mcmc* bad = nullptr;
        EXPECT(mod16_mcmc_create(b, &spec, nullptr, &bad) == MOD16_ERR_ARG && !bad);     // a problem without the constraint
        EXPECT(mod16_mcmc_destroy(m) == MOD16_OK);
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
    }
    printf("host_asan: annual: done\n");
}

// ---- the ensemble forward run: the small path, one pixel above it (staged), DEVICE arrays
template <typename T>
static int ensemble_call(mod16_ctx* ctx, const mod16_ensemble* e, const uint8_t* cls, const T* const* d, const int64_t* ds, int64_t n,
                         T* const* out, unsigned flags, int where) {
    if constexpr (sizeof(T) == 8) return mod16_et_ensemble_f64(ctx, e, cls, d, ds, n, out, flags, where, nullptr);
    else return mod16_et_ensemble_f32(ctx, e, cls, d, ds, n, out, flags, where, nullptr);
}
template <typename T>
static void ensemble_cases_of(mod16_ctx* ctx, const mod16_ensemble* e) {
    for (int64_t n : {(int64_t)1, (int64_t)257, (int64_t)65537}) {
        std::vector<std::vector<T>> drv(14, std::vector<T>(n, T(280))), outs(5, std::vector<T>(n));
        std::vector<uint8_t> cls(n, 1);
        const T* dp[14];
        int64_t ds[14];
        T one = T(300);
        for (int k = 0; k < 14; ++k) { dp[k] = k == 5 ? &one : drv[k].data(); ds[k] = k == 5 ? 0 : 1; }
        T* op[5];
        for (int k = 0; k < 5; ++k) op[k] = outs[k].data();
        OK(ensemble_call<T>(ctx, e, cls.data(), dp, ds, n, op, MOD16_MATH_FAST, MOD16_HOST));
        OK(ensemble_call<T>(ctx, e, cls.data(), dp, ds, n, op, MOD16_MATH_EXACT, MOD16_HOST));
        op[4] = nullptr;
        EXPECT(ensemble_call<T>(ctx, e, cls.data(), dp, ds, n, op, MOD16_MATH_FAST, MOD16_HOST) == MOD16_ERR_ARG);
    }
    const int64_t n = 257;
    const size_t per = ((size_t)n * sizeof(T) + 255) / 256 * 256;
    char* slab = static_cast<char*>(dmalloc(20 * per));
    const T* dp[14];
    int64_t ds[14];
    for (int k = 0; k < 14; ++k) { dp[k] = reinterpret_cast<const T*>(slab + k * per); ds[k] = k == 5 ? 0 : 1; }
    T* op[5];
    for (int k = 0; k < 5; ++k) op[k] = reinterpret_cast<T*>(slab + (14 + k) * per);
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(slab + 19 * per);
    OK(ensemble_call<T>(ctx, e, cls, dp, ds, n, op, MOD16_MATH_FAST, MOD16_DEVICE));
    OK(ensemble_call<T>(ctx, e, cls, dp, ds, n, op, MOD16_MATH_EXACT, MOD16_DEVICE));
    (void)hipFree(slab);
}
static void ensemble_cases(mod16_ctx* ctx) {
    std::vector<double> tables(3 * 13 * 11);
    for (size_t i = 0; i < tables.size(); ++i) tables[i] = 1.0 + (double)i;
    mod16_ensemble* bad = nullptr;
    EXPECT(mod16_ensemble_create(ctx, tables.data(), 0, &bad) == MOD16_ERR_ARG && !bad);
    for (int64_t members : {(int64_t)1, (int64_t)3}) {
        mod16_ensemble* e = nullptr;
        OK(mod16_ensemble_create(ctx, tables.data(), members, &e));
        ensemble_cases_of<double>(ctx, e);
        ensemble_cases_of<float>(ctx, e);
        EXPECT(mod16_ensemble_destroy(e) == MOD16_OK);
    }
    printf("host_asan: ensemble: done\n");
}

// ---- allocation failures. One call of the library under them: allocation k = 1, 2, ... of the call
// fails (device memory, or with `pinned` page-locked memory) until the call succeeds. Every failing
// round returns MOD16_ERR_NOMEM or MOD16_ERR_HIP, leaves as many allocations alive as there were, and
// leaves its object usable: the same call without a failure succeeds, and finish() -- an evaluation
// under the shadows, then the object's destruction -- runs clean. prepare() makes what the call needs,
// fresh for every round. HOST_ASAN_SWEEP_REPORT=1 prints a changed count and goes on (a survey of
// another build of the library) where the test stops.
template <typename Prepare, typename Call, typename Finish>
static void sweep(const char* what, bool pinned, Prepare prepare, Call call, Finish finish) {
    static const bool report = getenv("HOST_ASAN_SWEEP_REPORT") != nullptr;
    for (int k = 1; k <= 64; ++k) {
        prepare();
        const size_t live = mod16_stub_live_allocations();
        if (pinned) mod16_stub_fail_host_malloc(-k); else mod16_stub_fail_malloc(k);
        const int rc = call();
        mod16_stub_fail_host_malloc(0);
        mod16_stub_fail_malloc(0);
        ++g_checks;
        if (rc != MOD16_OK) {
            if (rc != MOD16_ERR_NOMEM && rc != MOD16_ERR_HIP) { fprintf(stderr, "host_asan: %s, %s allocation %d fails: status %d\n", what, pinned ? "pinned" : "device", k, rc); exit(1); }
            if (mod16_stub_live_allocations() != live) {
                fprintf(stderr, "host_asan: %s, %s allocation %d fails: %zu live allocations became %zu\n", what, pinned ? "pinned" : "device", k, live, mod16_stub_live_allocations());
                if (!report) exit(1);
            }
            const int again = call();
            if (again != MOD16_OK) { fprintf(stderr, "host_asan: %s: the call after a failed %s allocation %d -> %d\n", what, pinned ? "pinned" : "device", k, again); exit(1); }
        }
        finish();
        if (rc == MOD16_OK) {
            printf("host_asan: %s: %d failing %s allocations\n", what, k - 1, pinned ? "pinned" : "device");
            return;
        }
    }
    fprintf(stderr, "host_asan: %s: still failing after 64 rounds\n", what);
    exit(1);
}

static void failure_cases(mod16_ctx* ctx, const double* lut) {
    const int64_t n = 300, maxd = 16;
    Problem<double> p(n);
    std::vector<double> par(maxd * 11, 1.0), sse(maxd), cnt(maxd), pen(maxd), rows(3 * 7 * n);
    std::vector<uint8_t> labels(n);
    std::vector<int32_t> code(maxd);
    for (int64_t i = 0; i < n; ++i) labels[i] = (uint8_t)(i % 3);
    for (int64_t d = 0; d < maxd; ++d) code[d] = (int32_t)(d % 3);
    mod16_batch* b = nullptr;
    mod16_mcmc* m = nullptr;
    auto none = [] {};
    auto bind = [&] { b = nullptr; OK(mod16_static_batch_bind_f64(ctx, p.dp, p.ds, n, p.obs.data(), p.wts.data(), maxd, MOD16_MATH_FAST, MOD16_HOST, &b)); };
    auto evaluate = [&] { OK(mod16_static_batch_objective(b, par.data(), 7, sse.data(), cnt.data())); };
    auto unbind = [&] { EXPECT(mod16_static_batch_destroy(b) == MOD16_OK); };
    for (bool pinned : {false, true}) {
        mod16_ctx* c2 = nullptr;
        sweep("mod16_create", pinned, none, [&] { c2 = nullptr; return mod16_create(0, &c2); },
              [&] { mod16_ctx* ctx = c2; OK(mod16_set_bplut_f64(ctx, lut)); EXPECT(mod16_destroy(c2) == MOD16_OK); });
        sweep("mod16_static_batch_bind_f64", pinned, none,
              [&] { b = nullptr; return mod16_static_batch_bind_f64(ctx, p.dp, p.ds, n, p.obs.data(), p.wts.data(), maxd, MOD16_MATH_FAST, MOD16_HOST, &b); },
              [&] { evaluate(); unbind(); });
        sweep("mod16_static_batch_set_folds", pinned, bind, [&] { return mod16_static_batch_set_folds(b, labels.data(), 3); },
              [&] { OK(mod16_static_batch_objective_folds(b, par.data(), 7, code.data(), sse.data(), cnt.data())); evaluate(); unbind(); });
        AnnualProblem a;
        sweep("mod16_static_batch_set_annual", pinned, [&] { b = nullptr; OK(a.bind(ctx, true, &b)); }, [&] { return a.set(b); },
              [&] { OK(mod16_static_batch_objective_annual(b, par.data(), 7, sse.data(), cnt.data(), pen.data())); evaluate(); unbind(); });
    }
    mod16_mcmc_spec spec = sampler_spec(5, 4);
    sweep("mod16_mcmc_create", false, bind, [&] { m = nullptr; return mod16_mcmc_create(b, &spec, nullptr, &m); },
          [&] { OK(mod16_mcmc_run(m, 3, nullptr)); EXPECT(mod16_mcmc_destroy(m) == MOD16_OK); evaluate(); unbind(); });
    sweep("mod16_mcmc_run (the trace grows)", false,
          [&] { bind(); m = nullptr; OK(mod16_mcmc_create(b, &spec, nullptr, &m)); OK(mod16_mcmc_run(m, 5, nullptr)); },
          [&] { return mod16_mcmc_run(m, 4, nullptr); },
          [&] { int64_t steps = -1; std::vector<double> x(2 * 5 * 2);
                OK(mod16_mcmc_read(m, 6, 2, x.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &steps));
                EXPECT(steps == 9);                      // (a failing round took no step)
                EXPECT(mod16_mcmc_destroy(m) == MOD16_OK); evaluate(); unbind(); });
    sweep("mod16_static_batch_objective (first call)", false, bind, [&] { return mod16_static_batch_objective(b, par.data(), 7, sse.data(), cnt.data()); },
          [&] { evaluate(); unbind(); });
    sweep("mod16_static_batch_rows (first call)", false, bind,
          [&] { return mod16_static_batch_rows(b, par.data(), 7, rows.data(), rows.data() + 7 * n, rows.data() + 14 * n); }, [&] { evaluate(); unbind(); });
    {   // on the caller's device arrays: the captured step, and the unbound call's stream-ordered temporaries
        const size_t per = ((size_t)n * 8 + 255) / 256 * 256;
        char* slab = static_cast<char*>(dmalloc(19 * per + 7 * 11 * 8 + 2 * 7 * 8 + 64));
        const double* dp[14];
        int64_t ds[14];
        for (int k = 0; k < 14; ++k) { dp[k] = reinterpret_cast<const double*>(slab + k * per); ds[k] = 1; }
        double* day = reinterpret_cast<double*>(slab + 14 * per);
        double* night = reinterpret_cast<double*>(slab + 15 * per);
        const double* dobs = reinterpret_cast<const double*>(slab + 16 * per);
        const uint8_t* cls = reinterpret_cast<const uint8_t*>(slab + 17 * per);
        double* dtotal = reinterpret_cast<double*>(slab + 18 * per);       // (one draw's row)
        double* dpar = reinterpret_cast<double*>(slab + 19 * per);
        double* dsse = dpar + 7 * 11;
        double* ddiag = dsse + 2 * 7;
        mod16_graph* g = nullptr;
        sweep("mod16_graph_et_diag_f64", false, none,
              [&] { g = nullptr; return mod16_graph_et_diag_f64(ctx, cls, dp, ds, n, day, night, MOD16_MATH_FAST, ddiag, &g); },
              [&] { EXPECT(mod16_graph_launch(g, nullptr) == MOD16_OK); EXPECT(mod16_graph_destroy(g) == MOD16_OK); });
        sweep("mod16_et_static_batch_f64 (DEVICE)", false, none,
              [&] { return mod16_et_static_batch_f64(ctx, dp, ds, n, dpar, 1, nullptr, nullptr, dtotal, dobs, nullptr, dsse, dsse + 7, MOD16_MATH_FAST, MOD16_DEVICE, nullptr); },
              none);
        (void)hipFree(slab);
    }
    {
        std::vector<double> tables(3 * 13 * 11, 1.0), out(5 * 5);
        std::vector<uint8_t> cls(5, 1);
        double* op[5];
        for (int k = 0; k < 5; ++k) op[k] = out.data() + 5 * k;
        mod16_ensemble* e = nullptr;
        sweep("mod16_ensemble_create", false, none, [&] { e = nullptr; return mod16_ensemble_create(ctx, tables.data(), 3, &e); },
              [&] { OK(mod16_et_ensemble_f64(ctx, e, cls.data(), p.dp, p.ds, 5, op, MOD16_MATH_FAST, MOD16_HOST, nullptr)); EXPECT(mod16_ensemble_destroy(e) == MOD16_OK); });
    }
    printf("host_asan: allocation failures: done\n");
}

// the Sobol entry points in HOST mode: their workspaces and their release (launch shapes only)
static void sobol_cases(mod16_ctx* ctx) {
    const int d = 3;
    const int64_t n = 64;
    const double lo[3] = {0.0, 1.0, 2.0}, hi[3] = {1.0, 2.0, 3.0};
    for (int second = 0; second < 2; ++second) {
        const int R = second ? 2 * d + 2 : d + 2;
        std::vector<double> sample(n * R * d), y(n * R), idx(2 * d + d * d), sd(2 * d + d * d);
        OK(mod16_sobol_sample_f64(ctx, d, lo, hi, n, 0, second, sample.data(), MOD16_HOST, nullptr));
        double params[11], base[14];
        for (double& v : params) v = 1.0;
        for (double& v : base) v = 280.0;
        const int vary[3] = {0, 3, 5};
        OK(mod16_sobol_rows_f64(ctx, params, base, vary, lo, hi, d, n, 0, second, y.data(), MOD16_HOST, nullptr));
        OK(mod16_sobol_analyze_f64(ctx, y.data(), d, n, second, second, second ? 10 : 0, 7, idx.data(), sd.data(), MOD16_HOST, nullptr));
    }
    EXPECT(mod16_sobol_sample_f64(ctx, d, lo, hi, n + 1, 0, 0, nullptr, MOD16_HOST, nullptr) == MOD16_ERR_ARG);
    printf("host_asan: Sobol entry points: done\n");
}

int main(int argc, char** argv) {
    mod16_ctx* ctx = nullptr;
    EXPECT(mod16_create(3, &ctx) == MOD16_ERR_NO_DEVICE);
    EXPECT(mod16_create(0, &ctx) == MOD16_OK && ctx);
    if (argc > 1 && !strcmp(argv[1], "--fault")) {
        // the harness must SEE a fault: a raster whose storage is one tile short of what the call says
        // (the library cannot know; on a GPU this launch would read and write past the allocation)
        double lut[13 * 11] = {};
        OK(mod16_set_bplut_f64(ctx, lut));
        const int64_t tile = 4096;
        Raster<double> r(3 * tile, tile, 14, 1, 2);
        fprintf(stderr, "host_asan: launching 4 tiles on a raster of 3\n");
        (void)mod16_et_tiled_f64(ctx, &r.lay, r.bytes[0], r.wide.data(), 4 * tile, r.outs[0], r.outs[1], MOD16_MATH_FAST, nullptr, nullptr);
        fprintf(stderr, "host_asan: the fault went unnoticed\n");
        return 0;
    }
    {   // a class raster before a BPLUT: refused
        mod16_layout lay{4096, 14 * 4096, 2 * 4096, 4096};
        const double* w[14] = {};
        double o[2];
        uint8_t c[2] = {};
        EXPECT(mod16_et_tiled_f64(ctx, &lay, c, w, 4096, o, o, 0, nullptr, nullptr) == MOD16_ERR_NO_BPLUT);
    }
    double lut[13 * 11];
    for (int i = 0; i < 13 * 11; ++i) lut[i] = 1.0 + i;
    OK(mod16_set_bplut_f64(ctx, lut));
    tiled_cases<double>(ctx, "float64");
    tiled_cases<float>(ctx, "float32");
    plain_device_cases<double>(ctx, "float64");
    plain_device_cases<float>(ctx, "float32");
    host_cases<double>(ctx, "float64");
    host_cases<float>(ctx, "float32");
    {   // a graph and its context, destroyed in either order: once the context is gone a replay is
        // refused (its kernels would read the freed tables), the graph itself can still be freed
        mod16_ctx* c2 = nullptr;
        EXPECT(mod16_create(0, &c2) == MOD16_OK && c2);
        OK(mod16_set_bplut_f64(c2, lut));
        const int64_t tile = 4096;
        Raster<double> r(3 * tile, tile, 14, 1, 2);
        double* dd = static_cast<double*>(dmalloc(64));
        mod16_graph *g1 = nullptr, *g2 = nullptr;
        EXPECT(mod16_graph_et_tiled_f64(c2, &r.lay, r.bytes[0], r.wide.data(), r.n, r.outs[0], r.outs[1], MOD16_MATH_FAST, dd, &g1) == MOD16_OK);
        EXPECT(mod16_graph_et_tiled_f64(c2, &r.lay, r.bytes[0], r.wide.data(), r.n, r.outs[0], r.outs[1], MOD16_MATH_FAST, dd, &g2) == MOD16_OK);
        EXPECT(mod16_graph_launch(g1, nullptr) == MOD16_OK);
        EXPECT(mod16_graph_destroy(g1) == MOD16_OK);          // graph first: leaves the context's list
        EXPECT(mod16_destroy(c2) == MOD16_OK);                // context first: g2 is dead ...
        float ms = 0;
        EXPECT(mod16_graph_launch(g2, nullptr) == MOD16_ERR_ARG);
        EXPECT(mod16_time_graph(g2, 1, nullptr, &ms) == MOD16_ERR_ARG);
        EXPECT(mod16_graph_destroy(g2) == MOD16_OK);          // ... and still freed
        (void)hipFree(dd);
        printf("host_asan: graph lifetime: done\n");
    }
    {   // the stand-alone reduction, the rank-order fold, the copy probe
        const int64_t n = 1200 * 1200 + 1;
        double* day = static_cast<double*>(dmalloc(8 * n));
        double* gathered = static_cast<double*>(dmalloc(8 * 64));
        double host[8];
        OK(mod16_reduce_diag_f64(ctx, day, day, n, host, nullptr, nullptr));
        OK(mod16_fold_diag(ctx, gathered, 8, gathered, nullptr));
        EXPECT(mod16_fold_diag(ctx, gathered, 0, gathered, nullptr) == MOD16_ERR_ARG);
        float gbps = 0;
        OK(mod16_measure_copy(ctx, 1 << 20, 1, &gbps));
        (void)hipFree(day);
        (void)hipFree(gathered);
    }
    {   // the resident calibration problem: bind, objective, rows, destroy
        const int64_t n = 1000, ndraw = 7;
        std::vector<std::vector<double>> drv(14, std::vector<double>(n, 280.0));
        std::vector<double> obs(n, 10.0), par(ndraw * 11, 1.0), sse(ndraw), cnt(ndraw), rows(ndraw * n);
        const double* dp[14];
        int64_t ds[14];
        for (int k = 0; k < 14; ++k) { dp[k] = drv[k].data(); ds[k] = 1; }
        ds[7] = 0;
        mod16_batch* b = nullptr;
        OK(mod16_static_batch_bind_f64(ctx, dp, ds, n, obs.data(), nullptr, 16, MOD16_MATH_FAST, MOD16_HOST, &b));
        EXPECT(mod16_static_batch_objective(b, par.data(), ndraw, sse.data(), cnt.data()) == MOD16_OK);
        EXPECT(mod16_static_batch_rows(b, par.data(), ndraw, nullptr, nullptr, rows.data()) == MOD16_OK);
        EXPECT(mod16_static_batch_objective(b, par.data(), 17, sse.data(), cnt.data()) != MOD16_OK);   // more than max_draws
        EXPECT(mod16_static_batch_destroy(b) == MOD16_OK);
        OK(mod16_et_static_batch_f64(ctx, dp, ds, n, par.data(), ndraw, nullptr, nullptr, nullptr, obs.data(), nullptr, sse.data(),
                                     cnt.data(), MOD16_MATH_EXACT, MOD16_HOST, nullptr));
    }
    calibration_cases(ctx);
    annual_cases(ctx);
    ensemble_cases(ctx);
    sobol_cases(ctx);
    failure_cases(ctx, lut);
    EXPECT(mod16_destroy(ctx) == MOD16_OK);
    {   // no page-locked memory for the small calls' buffer: the call is staged instead (and the
        // context stops asking), every entry point that has the small path
        mod16_ctx* c2 = nullptr;
        EXPECT(mod16_create(0, &c2) == MOD16_OK && c2);
        ctx = c2;
        OK(mod16_set_bplut_f64(ctx, lut));
        const int64_t n = 9;
        std::vector<std::vector<double>> drv(14, std::vector<double>(n, 280.0)), par(11, std::vector<double>(n, 2.0));
        std::vector<uint8_t> cls(n, 1), fpar(n, 50), lai(n, 20);
        std::vector<double> day(n), night(n);
        const double *dp[14], *pp[11];
        int64_t ds[14], ps[11];
        for (int k = 0; k < 14; ++k) { dp[k] = drv[k].data(); ds[k] = 1; }
        for (int k = 0; k < 11; ++k) { pp[k] = par[k].data(); ps[k] = 1; }
        mod16_stub_fail_host_malloc(1000);
        OK(mod16_et_f64(ctx, cls.data(), dp, ds, nullptr, nullptr, n, day.data(), night.data(), nullptr, MOD16_MATH_FAST, MOD16_HOST, nullptr));
        OK(mod16_et_static_f64(ctx, dp, ds, pp, ps, nullptr, nullptr, n, day.data(), night.data(), 1e-7, MOD16_HOST, nullptr));
        OK(mod16_et_raw_f64(ctx, cls.data(), dp, ds, fpar.data(), lai.data(), nullptr, 0, n, day.data(), night.data(), nullptr, MOD16_MATH_FAST, MOD16_HOST, nullptr));
        const double* in[13] = {dp[5], dp[9]};
        int64_t is[13] = {1, 1};
        double* outs[2] = {day.data(), nullptr};
        OK(mod16_method_f64(ctx, MOD16_M_RHUMIDITY, in, is, nullptr, nullptr, n, outs, 1.26, 1e-7, MOD16_HOST, nullptr));
        mod16_stub_fail_host_malloc(0);
        EXPECT(mod16_destroy(ctx) == MOD16_OK);
    }
    mod16_stub_report(stdout);
    // everything the library allocated is gone with its context
    EXPECT(mod16_stub_live_allocations() == 0);
    printf("host_asan: ok (%d checks)\n", g_checks);
    return 0;
}
