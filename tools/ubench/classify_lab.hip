// Lab proof for csrc/wide_classify.hpp: the staging waves' classification of the wide ring gives the same two flags of a
// batch as the expressions it replaced (round 11: convert, convert back, compare; |x| as bits, unsigned maximum), for
// EVERY float32 bit pattern - denormals, both zeros, both infinities, quiet and signalling NaNs of either sign and the
// magnitudes around 2^18, 2^23 and 2^31 among them.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/ubench/classify_lab.hip -o tools/ubench/classify_lab.bin
//   tools/ubench/classify_lab.bin          ->  "0 mismatches of 4294967296" and exit status 0
//
// (the library's own compile flags: the denormal mode of v_fract_f32 and of the compare is the build's)
//
// A lane walks its share of the patterns.  For each it forms the flags of a lane's batch - 16 rows of two samples - that
// holds the pattern in one slot of the first row (slot 0, then slot 1) and 1900.0f everywhere else, with both codes.  The
// flags of a wave's batch are these lane answers ORed over the lanes and then combined the same way in both codes
// (wild wins over fractional), and a lane's (bad, frac_only) pair names its (wild, fractional-unless-wild) answers one
// to one: equal pairs for every pattern are equal flags for every batch.  One pass, no timing loop.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../topo_descriptors_amd/csrc/wide_classify.hpp"

namespace {

constexpr float kAbsLim = 262144.0f;  // disc_wave_impl.hpp
constexpr int kBad = 1, kFracOnly = 1 << 15;
constexpr int kRows = 16;
constexpr float kFill = 1900.0f;
constexpr int kKeep = 16;  // mismatching patterns kept for the report

struct Report {
    unsigned long long mismatches;
    unsigned kept;
    uint32_t pattern[kKeep];
    int slot[kKeep], want[kKeep], got[kKeep];
};

// The parent's classification, per sample as stage_batch of round 11 had it (a lane's share: the ballots there ORed these
// per-lane answers over the wave).
struct ParentAcc {
    uint32_t amax = 0;  // largest |x| seen, as float bits (NaN / inf sort above all)
    bool frac = false;  // saw x != (float)(int)x
};
__device__ __forceinline__ void parent_row(ParentAcc& a, float x0, float x1) {
    const int i0 = (int)x0, i1 = (int)x1;
    const uint32_t a0 = __float_as_uint(x0) & 0x7fffffffu, a1 = __float_as_uint(x1) & 0x7fffffffu;
    a.frac |= (x0 != (float)i0) | (x1 != (float)i1);
    a.amax = max(a.amax, max(a0, a1));
}
__device__ __forceinline__ int parent_flags(const ParentAcc& a) {
    const uint32_t kLimBits = __float_as_uint(kAbsLim + 1.0f);  // |trunc(x)| <= kAbsLim  <=>  |x| < kAbsLim + 1
    const bool wild = a.amax >= kLimBits;
    const bool any_frac = a.frac;
    const bool bad = wild || any_frac;
    const bool fr = !wild && any_frac;
    return (bad ? kBad : 0) | (fr ? kFracOnly : 0);
}

__global__ __launch_bounds__(256) void walk(Report* rep, uint32_t per_thread) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nthreads = gridDim.x * blockDim.x;
    // (the fill value through a register the compiler cannot see into: all sixteen rows are classified, not folded)
    float fill = kFill;
    asm volatile("" : "+v"(fill));
    for (uint32_t k = 0; k < per_thread; ++k) {
        const uint32_t bits = k * nthreads + tid;  // a wave's lanes hold 64 adjacent patterns
        const float x = __uint_as_float(bits);
        for (int slot = 0; slot < 2; ++slot) {
            ParentAcc pa;
            topo::WideClassAcc na;
            for (int r = 0; r < kRows; ++r) {
                const float x0 = r == 0 && slot == 0 ? x : fill, x1 = r == 0 && slot == 1 ? x : fill;
                parent_row(pa, x0, x1);
                topo::wide_classify_row(na, x0, x1);
            }
            const int want = parent_flags(pa);
            const int got = topo::wide_class_flags(topo::wide_lane_wild(na, kAbsLim + 1.0f), topo::wide_lane_frac(na), kBad, kFracOnly);
            if (want != got) {
                atomicAdd(&rep->mismatches, 1ull);
                const unsigned at = atomicAdd(&rep->kept, 1u);
                if (at < kKeep) {
                    rep->pattern[at] = bits;
                    rep->slot[at] = slot;
                    rep->want[at] = want;
                    rep->got[at] = got;
                }
            }
        }
    }
}

}  // namespace

#define HIP_OK(x)                                                            \
    do {                                                                     \
        hipError_t e_ = (x);                                                 \
        if (e_ != hipSuccess) {                                              \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));          \
            return 2;                                                        \
        }                                                                    \
    } while (0)

int main() {
    constexpr uint32_t kBlocks = 4096, kThreads = 256, kPerThread = 4096;
    static_assert((unsigned long long)kBlocks * kThreads * kPerThread == 1ull << 32, "every pattern once");
    Report* d = nullptr;
    Report h = {};
    HIP_OK(hipMalloc((void**)&d, sizeof(Report)));
    HIP_OK(hipMemset(d, 0, sizeof(Report)));
    hipLaunchKernelGGL(walk, dim3(kBlocks), dim3(kThreads), 0, 0, d, kPerThread);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(&h, d, sizeof(Report), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d));
    // (both slots of a pattern count as one pattern's check: the count is of (pattern, slot) pairs that differ)
    printf("%llu mismatches of %llu\n", h.mismatches, 1ull << 32);
    for (unsigned i = 0; i < (h.kept < (unsigned)kKeep ? h.kept : (unsigned)kKeep); ++i)
        printf("  pattern 0x%08x (%g) in slot %d: parent flags 0x%04x, helper flags 0x%04x\n", h.pattern[i],
               (double)__builtin_bit_cast(float, h.pattern[i]), h.slot[i], h.want[i], h.got[i]);
    return h.mismatches == 0 ? 0 : 1;
}
