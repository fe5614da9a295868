// Lab bench for the 67-px TPI / STD kernels: builds variants of the disc kernels from the product's headers in
// one translation unit (30-60 s instead of the whole library), times them on the bench DEM and compares the
// output plane with the product library's, bit for bit.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off [-DMARCH_STAMPS] tools/ubench/tpi_lab.hip \
//         -Ltopo_descriptors_amd -ltopo_amd -Wl,-rpath,'$ORIGIN/../../topo_descriptors_amd' -o tools/ubench/tpi_lab.bin
//   tools/ubench/tpi_lab.bin <variant> [n=32768] [reps=5] [integer=1]
//     variant march : tpi_march_kernel<67, 60, 12> as the product launches it (+ the two empty follow-up launches)
//     variant ring  : tpi_ring_kernel<67, 8> (round 2, 8 columns per lane)
//     variants any_tpi / any_std / any_tpi_std : the product's dispatch for 67 px, compiled with this build's flags
//   (-DMARCH_DYN_ROWS=0/1, -DCHAIN_PRIO=0/1, -DMARCH_STAMPS)
//   -DWIDE_STAMPS=1/2 (variant any_tpi): clock stamps of tpi_ring_wide_kernel<67> at the end of a phase, printed per wave for
//   two blocks - 1 with the chain waves' output stores drained in front of the barrier, 2 without (the kernel as built) - and
//   per SIMD how much earlier its older chain wave is at the barrier than its younger one; -DWIDE_PRIO=0: no wave touches its
//   issue priority (the A/B of the priority ladder, profiles/r13_tpi67_prio_stamps.txt); -DWIDE_BOUNDARY=1: the chain waves'
//   lead fetches in front of the phase barrier, their phase state by increments (round 14: measured, not kept) - the stamps
//   also give a chain wave's ticks from the barrier to the arrival of its lead rows (profiles/r14_tpi67_boundary_stamps.txt)
//   -DWIDE_STAGE_CEILING=1 (variant any_tpi): tpi_ring_wide_kernel<67> whose staging only converts, prefixes and writes, flags
//   constant 0 (whole-metre rasters only: the ceiling of a leaner staging stream); -DWIDE_LEAN=0: every batch on the general path
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/topo_amd.h"
#include "../../topo_descriptors_amd/csrc/disc_wave_impl.hpp"
#include "../../topo_descriptors_amd/csrc/disc_ring_impl.hpp"
#ifdef LAB_EXTRA
#include LAB_EXTRA
#endif

#ifndef LAB_TH
#define LAB_TH 60  // rows a marching tile adds (12 waves: a multiple of 12)
#endif

#define CK(x)                                                                         \
    do {                                                                              \
        int rc_ = (x);                                                                \
        if (rc_ != TOPO_AMD_OK) {                                                     \
            fprintf(stderr, "%s -> %d: %s\n", #x, rc_, topo_amd_last_error());        \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

__global__ void diff_kernel(const uint32_t* a, const uint32_t* b, size_t n, unsigned long long* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = 0;
    for (; i < n; i += (size_t)gridDim.x * blockDim.x) bad += a[i] != b[i];
    if (bad) atomicAdd(out, bad);
}

int main(int argc, char** argv) {
    const char* variant = argc > 1 ? argv[1] : "march";
    const int n = argc > 2 ? atoi(argv[2]) : 32768;
    const int reps = argc > 3 ? atoi(argv[3]) : 5;
    const int integer = argc > 4 ? atoi(argv[4]) : 1;
#ifndef LAB_SIZE
#define LAB_SIZE 67
#endif
    constexpr int SIZE = LAB_SIZE;
    CK(topo_amd_init(0));
    void *dem = nullptr, *out = nullptr, *ref = nullptr, *out2 = nullptr, *ref2 = nullptr;
    const size_t bytes = (size_t)n * n * 4;
    CK(topo_amd_malloc(&dem, bytes));
    CK(topo_amd_malloc(&out, bytes));
    CK(topo_amd_malloc(&ref, bytes));
    CK(topo_amd_synth_dem_dev((float*)dem, n, 0, n, 0, integer));
    topo::Block b{(const float*)dem, n, 0, n, n, 0, n};
    const bool want_std = strstr(variant, "std") != nullptr;
    if (want_std) {
        CK(topo_amd_malloc(&out2, bytes));
        CK(topo_amd_malloc(&ref2, bytes));
    }
    // the product's answer
    CK(topo_amd_tpi_std_dev((const float*)dem, n, 0, n, n, SIZE, 0, n, (float*)ref, (float*)ref2));
    if (!strcmp(variant, "any_std")) CK(topo_amd_memcpy_d2d(out, ref, bytes));  // no TPI plane in this variant
    CK(topo_amd_memset(out, 0xFF, bytes));
    if (out2) CK(topo_amd_memset(out2, 0xFF, bytes));
    auto run = [&]() -> int {
        if (!strcmp(variant, "march")) {
            int rc = topo::launch_march<SIZE, LAB_TH, 12, true, true, true>(b, (float*)out);
            if (rc != TOPO_AMD_OK) return rc;
            rc = topo::launch_fraction_march<SIZE, LAB_TH, 12>(b, (float*)out);
            if (rc != TOPO_AMD_OK) return rc;
            // (the general kernel's tile of LAB_TH > 60 rows does not fit LDS; on the bench DEM nothing is deferred to it)
            if constexpr (LAB_TH <= 60) return topo::launch_wave<SIZE, LAB_TH, 12, true, false>(b, (float*)out, nullptr, true);
            return TOPO_AMD_OK;
        }
        if (!strcmp(variant, "ring")) return topo::launch_ring<SIZE, 8, topo::kRingMain>(b, (float*)out);
        // the product's dispatch (launch_wave_any) with this build's -D flags
        if (!strcmp(variant, "any_tpi")) return topo::launch_wave_any<SIZE>(b, (float*)out, nullptr);
        if (!strcmp(variant, "any_std")) return topo::launch_wave_any<SIZE>(b, nullptr, (float*)out2);
        if (!strcmp(variant, "any_tpi_std")) return topo::launch_wave_any<SIZE>(b, (float*)out, (float*)out2);
#ifdef LAB_EXTRA
        return lab_run(variant, b, (float*)out, (float*)out2);
#else
        topo::set_error("unknown variant %s", variant);
        return TOPO_AMD_EINVAL;
#endif
    };
    CK(run());
    CK(topo_amd_sync());
    float best = 1e30f, sum = 0.f;
    for (int r = 0; r < reps; ++r) {
        CK(topo_amd_mark(2 * r));
        CK(run());
        CK(topo_amd_mark(2 * r + 1));
    }
    for (int r = 0; r < reps; ++r) {
        float ms = 0.f;
        CK(topo_amd_mark_elapsed(2 * r, 2 * r + 1, &ms));
        best = ms < best ? ms : best;
        sum += ms;
    }
#if WIDE_STAMPS
    {
        // what the last launch of tpi_ring_wide_kernel left (variant any_tpi at 67 px): per stamped block and wave the ticks
        // of its phases, of the chain waves' store drain in front of the phase barrier, of the barrier, of a stamp pair
        unsigned long long st[topo::kWideStampBlocks][topo::kWideStampWaves][topo::kWideStampFields];
        if (hipMemcpyFromSymbol(st, HIP_SYMBOL(topo::wide_stamps), sizeof(st)) != hipSuccess) return 1;
        printf("WIDE_BOUNDARY %d, %d valid columns a strip\n", WIDE_BOUNDARY, topo::WGeo<SIZE>::TILE_W);
        for (int k = 0; k < topo::kWideStampBlocks; ++k)
            for (int w = 0; w < topo::kWideStampWaves; ++w) {
                const unsigned long long* s = st[k][w];
                const double n = s[0] ? (double)s[0] : 1.0;
                printf("blk %s wave %2d (%s): phases %llu  ticks a phase %.1f | drain %.1f | barrier %.1f | stamp pair %.1f"
                       "   drain less the pair: %.2f %% of a phase\n",
                       k ? "mid" : "  0", w, w < 3 ? "stager" : "chain ", s[0], s[1] / n, s[2] / n, s[3] / n, s[4] / n,
                       s[1] ? 100.0 * ((double)s[2] - (double)s[4]) / (double)s[1] : 0.0);
                // a chain wave's way from the barrier to its sweep: the stamp behind the barrier to the stamp where the lead
                // rows have arrived (both stamps wait for the wave's LDS reads; a stamp pair's own ticks are beside it)
                if (w >= 3 && s[5])
                    printf("                      sweeps behind a barrier %llu  barrier to lead rows %.1f ticks, less the pair %.1f:"
                           " %.2f %% of a phase\n",
                           s[5], (double)s[6] / (double)s[5], (double)s[6] / (double)s[5] - s[4] / n,
                           s[1] ? 100.0 * ((double)s[6] / (double)s[5] - s[4] / n) / (s[1] / n) : 0.0);
            }
        // wave w runs on SIMD w mod 4: per SIMD how much longer its older chain wave waits at the barrier than its younger one
        for (int k = 0; k < topo::kWideStampBlocks; ++k) {
            printf("blk %s older chain wave at the barrier before the younger, SIMD 0 .. 3:", k ? "mid" : "  0");
            for (int simd = 0; simd < 4; ++simd) {
                const unsigned long long *a = st[k][simd == 3 ? 3 : 4 + simd], *b = st[k][simd == 3 ? 7 : 8 + simd];
                printf(" %.0f", (double)a[3] / (a[0] ? (double)a[0] : 1.0) - (double)b[3] / (b[0] ? (double)b[0] : 1.0));
            }
            printf(" ticks\n");
        }
    }
#endif
    unsigned long long* d_bad = nullptr;
    unsigned long long bad[2] = {0, 0};
    CK(topo_amd_malloc((void**)&d_bad, 16));
    CK(topo_amd_memset(d_bad, 0, 16));
    CK(topo_amd_sync());
    hipLaunchKernelGGL(diff_kernel, dim3(4096), dim3(256), 0, 0, (const uint32_t*)out, (const uint32_t*)ref, (size_t)n * n, d_bad);
    if (out2) hipLaunchKernelGGL(diff_kernel, dim3(4096), dim3(256), 0, 0, (const uint32_t*)out2, (const uint32_t*)ref2, (size_t)n * n, d_bad + 1);
    (void)hipDeviceSynchronize();
    CK(topo_amd_memcpy_d2h(bad, d_bad, 16));
    printf("{\"variant\": \"%s\", \"integer_dem\": %d, \"n\": %d, \"ms_mean\": %.4f, \"ms_min\": %.4f, \"reps\": %d, "
           "\"pixels_differing_from_product\": %llu, \"std_pixels_differing\": %llu}\n",
           variant, integer, n, sum / reps, best, reps, bad[0], bad[1]);
    return 0;
}
