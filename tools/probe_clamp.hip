// Probe of the VOP3 `clamp` output modifier on float64 (gfx950): what v_mul_f64 ... clamp and
// v_fma_f64 ... clamp return for NaN, -0.0, values below 0 and above 1, with MODE.DX10_CLAMP at its
// start-up value and cleared (profiles/r07_probe_clamp.txt).
// hipcc --offload-arch=gfx950 -O3 tools/probe_clamp.hip -o tools/bin/probe_clamp && tools/bin/probe_clamp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

constexpr int kN = 12;

template <bool CLEAR> __global__ void clamp_kernel(const double* x, double* mul, double* fma) {
    if (CLEAR) asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 8, 1), 0\n\ts_nop 3" ::: "memory");
    const double v = x[threadIdx.x], one = 1.0, zero = 0.0;
    double m, f;
    asm volatile("v_mul_f64 %0, %1, %2 clamp" : "=v"(m) : "v"(v), "v"(one));
    asm volatile("v_fma_f64 %0, %1, %2, %3 clamp" : "=v"(f) : "v"(v), "v"(one), "v"(zero));
    mul[threadIdx.x] = m;
    fma[threadIdx.x] = f;
}

int main() {
    const double sig = [] { unsigned long long b = 0x7ff0000000000001ull; double d; memcpy(&d, &b, 8); return d; }();
    const double hx[kN] = {NAN, -NAN, sig, -0.0, 0.0, -1e-300, -2.5, 0.25, 1.0, 1.0 + 0x1p-52, 7.0, INFINITY};
    double *x, *m, *f, hm[kN], hf[kN];
    if (hipMalloc(&x, sizeof hx) != hipSuccess || hipMalloc(&m, sizeof hx) != hipSuccess ||
        hipMalloc(&f, sizeof hx) != hipSuccess || hipMemcpy(x, hx, sizeof hx, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    for (int clear = 0; clear < 2; ++clear) {
        if (clear) clamp_kernel<true><<<1, kN>>>(x, m, f); else clamp_kernel<false><<<1, kN>>>(x, m, f);
        if (hipMemcpy(hm, m, sizeof hx, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        if (hipMemcpy(hf, f, sizeof hx, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        printf("MODE.DX10_CLAMP = %d\n", 1 - clear);
        for (int i = 0; i < kN; ++i) {
            unsigned long long bx, bm, bf;
            memcpy(&bx, &hx[i], 8); memcpy(&bm, &hm[i], 8); memcpy(&bf, &hf[i], 8);
            printf("  x %-24.17g %016llx   x*1 clamp %-8g %016llx   fma(x,1,0) clamp %-8g %016llx\n",
                   hx[i], bx, hm[i], bm, hf[i], bf);
        }
    }
    return 0;
}
