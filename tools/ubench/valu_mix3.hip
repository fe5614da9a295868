// Microbenchmark, third batch: issue cost of the forms the wide ring's staging classification uses (csrc/wide_classify.hpp:
// v_fract_f32, v_or3_b32, v_max3_f32 with |.| source modifiers) beside the ones it replaced (v_cvt_f32_i32, v_and_b32,
// v_max_u32, v_max3_u32) and the v_add_u32 / v_cvt_i32_f32 that stay, at 8 / 12 / 16 waves per CU like
// tools/ubench/valu_mix.hip and valu_mix2.hip (whose figures tools/valu_bound.py prices with).
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/valu_mix3.hip -o tools/ubench/valu_mix3.bin && tools/ubench/valu_mix3.bin
#include <hip/hip_runtime.h>
#include <cstdio>

#define REP8(x) x x x x x x x x

template <int MODE>
__global__ __launch_bounds__(1024) void k(unsigned* out, int iters) {
    unsigned a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    unsigned b = out[threadIdx.x], c = b + 7;
    for (int it = 0; it < iters; ++it) {
#define OPS(INS)                                                                                \
    asm volatile(REP8(INS(0) INS(1) INS(2) INS(3) INS(4) INS(5) INS(6) INS(7))                    \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)   \
                 : "v"(b), "v"(c));
#define I_ADD(n) "v_add_u32 %" #n ", %" #n ", %8\n"
#define I_FRACT(n) "v_fract_f32 %" #n ", %8\n"
#define I_OR3(n) "v_or3_b32 %" #n ", %" #n ", %8, %9\n"
#define I_MAX3F(n) "v_max3_f32 %" #n ", %" #n ", |%8|, |%9|\n"
#define I_CVTI(n) "v_cvt_i32_f32 %" #n ", %8\n"
#define I_CVTF(n) "v_cvt_f32_i32 %" #n ", %8\n"
#define I_AND(n) "v_and_b32 %" #n ", %" #n ", %8\n"
#define I_MAXU(n) "v_max_u32 %" #n ", %" #n ", %8\n"
#define I_MAX3U(n) "v_max3_u32 %" #n ", %" #n ", %8, %9\n"
#define I_OR(n) "v_or_b32 %" #n ", %" #n ", %8\n"
        if (MODE == 0) { OPS(I_ADD) }
        if (MODE == 1) { OPS(I_FRACT) }
        if (MODE == 2) { OPS(I_OR3) }
        if (MODE == 3) { OPS(I_MAX3F) }
        if (MODE == 4) { OPS(I_CVTI) }
        if (MODE == 5) { OPS(I_CVTF) }
        if (MODE == 6) { OPS(I_AND) }
        if (MODE == 7) { OPS(I_MAXU) }
        if (MODE == 8) { OPS(I_MAX3U) }
        if (MODE == 9) { OPS(I_OR) }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}

template <int MODE>
void run(const char* name, unsigned* d, int waves) {
    const int blocks = 256, iters = 2000;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(waves * 64), 0, 0, d, iters);
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(waves * 64), 0, 0, d, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    const double instr_per_simd = (double)waves / 4.0 * iters * 64.0;
    printf("%-34s %2d waves/CU: %8.3f ms  %6.2f ns/instr/SIMD (wall)  = %5.2f cycles at 2.4 GHz\n", name, waves, ms,
           ms * 1e6 / instr_per_simd, ms * 1e6 / instr_per_simd * 2.4);
}

int main() {
    unsigned* d;
    if (hipMalloc(&d, 256 * 1024 * sizeof(unsigned)) != hipSuccess) return 1;
    if (hipMemset(d, 0, 256 * 1024 * sizeof(unsigned)) != hipSuccess) return 1;
    for (int waves : {8, 12, 16}) {
        run<0>("v_add_u32", d, waves);
        run<1>("v_fract_f32", d, waves);
        run<2>("v_or3_b32", d, waves);
        run<3>("v_max3_f32 |a| |b|", d, waves);
        run<4>("v_cvt_i32_f32", d, waves);
        run<5>("v_cvt_f32_i32", d, waves);
        run<6>("v_and_b32", d, waves);
        run<7>("v_max_u32", d, waves);
        run<8>("v_max3_u32", d, waves);
        run<9>("v_or_b32", d, waves);
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
