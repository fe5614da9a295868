// Mean and standard deviation of a float32 plane with the bits numpy's own float32 mean() / std() give (kernel K7).
//
// The valley / ridge index standardises the DEM with them (reference topo.py:427), and two directions that nearly tie flip
// on the last digit of either: the float64 moments of valley.hip are closer to the truth and still the wrong answer there.
// So the sums are formed in numpy's ORDER, which for n contiguous float32 samples is:
//   - consecutive chunks of `chunk` samples (numpy's buffer size, 8192 by default), each reduced by numpy's pairwise sum,
//     the chunk sums added one after the other in float32 from 0.0f, a last partial chunk the same way;
//   - the pairwise sum of m samples: fewer than 8, a sequential loop from 0; up to 128, eight accumulators
//     r[k] += a[8 j + k] combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the m % 8 samples left added one by one;
//     otherwise the sums of the first h = m / 2 - (m / 2) % 8 samples and of the rest, added.  A chunk that is a power of
//     two >= 128 is therefore a perfect tree over leaves of 128 samples, neighbours combined level by level;
//   - mean = sum / (float)n;  std = sqrtf(sum of ((a - mean) * (a - mean)) / (float)n), the difference and the product each
//     rounded to float32 (no fused multiply-add), summed in the same order.
// The kernel forms the sums of the FULL chunks (one float per chunk, or per 8192 samples of a longer chunk); the host
// downloads them (131072 floats for 32768^2), finishes longer chunks' trees, runs the sequential chain and reduces the tail
// of fewer than `chunk` samples itself.  Every float32 operation below is a single IEEE operation: this file is built with
// -ffp-contract=off and without fast-math, and the device code spells the roundings out (__fadd_rn ...).
#include <cmath>
#include <vector>

#include "common.hpp"

#pragma clang fp contract(off)

namespace topo {
namespace {

constexpr int kLeaf = 128;                  // samples of a leaf of the pairwise tree
constexpr int kTileLeaves = 64;             // leaves a block stages: 8192 samples, 32 KiB
constexpr int kTile = kLeaf * kTileLeaves;
constexpr int kPitch = kLeaf + 8;           // floats between leaves in LDS: 4 leaves x 8 accumulators on 32 different banks
constexpr int kNpThreads = 256;

// One block per tile of 8192 samples of in[0, covered) (covered: a multiple of 128 `group` leaves).  The tile goes through
// LDS with 16-byte loads (VEC; sample by sample for a plane that is not 16-byte aligned), squared deviations from `mean`
// formed on the way in (SQ).  Thread (leaf, k) then walks accumulator k of its leaf, 8 lanes combine a leaf's accumulators
// and the first wave combines neighbouring leaves, `group` (1 ... 64, a power of two) to a sum: partial[tile * 64 / group + i].
template <bool VEC, bool SQ>
__global__ __launch_bounds__(kNpThreads) void np_partials_kernel(const float* __restrict__ in, size_t covered, float mean, int group,
                                                                 size_t n_partials, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float tile[kTileLeaves * kPitch];
    __shared__ float leaf_sum[kTileLeaves];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kTile;
    float4 x[kTile / 4 / kNpThreads];
#pragma unroll
    for (int q = 0; q < kTile / 4 / kNpThreads; ++q) {
        const size_t g = base + (size_t)(q * kNpThreads + t) * 4;
        x[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (leaves past the last full chunk: their sums are never stored)
        if (g < covered) {
            if (VEC) {
                x[q] = *reinterpret_cast<const float4*>(in + g);
            } else {
                x[q] = make_float4(in[g], in[g + 1], in[g + 2], in[g + 3]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kTile / 4 / kNpThreads; ++q) {
        float4 v = x[q];
        if (SQ) {
            v.x = __fsub_rn(v.x, mean), v.y = __fsub_rn(v.y, mean), v.z = __fsub_rn(v.z, mean), v.w = __fsub_rn(v.w, mean);
            v.x = __fmul_rn(v.x, v.x), v.y = __fmul_rn(v.y, v.y), v.z = __fmul_rn(v.z, v.z), v.w = __fmul_rn(v.w, v.w);
        }
        const int f = q * kNpThreads + t;  // float4 index in the tile: 32 to a leaf
        *reinterpret_cast<float4*>(&tile[(f >> 5) * kPitch + (f & 31) * 4]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kTileLeaves * 8 / kNpThreads; ++r) {
        const int p = r * kNpThreads + t, leaf = p >> 3, k = p & 7;
        const float* a = &tile[leaf * kPitch + k];
        float acc = a[0];
#pragma unroll
        for (int j = 1; j < kLeaf / 8; ++j) acc = __fadd_rn(acc, a[8 * j]);
        acc = __fadd_rn(acc, __shfl_xor(acc, 1));  // r0+r1 | r2+r3 | r4+r5 | r6+r7 (an IEEE sum does not depend on the operands' order)
        acc = __fadd_rn(acc, __shfl_xor(acc, 2));  // (r0+r1)+(r2+r3) | (r4+r5)+(r6+r7)
        acc = __fadd_rn(acc, __shfl_xor(acc, 4));
        if (k == 0) leaf_sum[leaf] = acc;
    }
    __syncthreads();
    if (t < kTileLeaves) {
        float v = leaf_sum[t];
        for (int w = 1; w < group; w <<= 1) v = __fadd_rn(v, __shfl_xor(v, w));  // lane i, a multiple of 2w: leaves [i, i+w) + [i+w, i+2w)
        const size_t at = (size_t)blockIdx.x * (kTileLeaves / group) + t / group;
        if (t % group == 0 && at < n_partials) partial[at] = v;
    }
}

// numpy's pairwise sum on the host (the tail of fewer than `chunk` samples)
float pairwise_host(const float* a, size_t n) {
    if (n < 8) {
        float res = 0.0f;
        for (size_t i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    if (n <= (size_t)kLeaf) {
        float r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        size_t i = 8;
        for (; i + 8 <= n; i += 8)
            for (int k = 0; k < 8; ++k) r[k] = r[k] + a[i + k];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + a[i];
        return res;
    }
    size_t h = n / 2;
    h -= h % 8;
    const float lo = pairwise_host(a, h), hi = pairwise_host(a + h, n - h);
    return lo + hi;
}

// One pass: the sum of in[0, count) (sq: of the squared deviations from `mean`) in numpy's order.  `tail`: the last
// count % chunk samples on the host (downloaded by the caller once for both passes).
int np_sum(const float* in, size_t count, size_t chunk, bool sq, float mean, const std::vector<float>& tail, float* sum) {
    Context& c = ctx();
    const size_t n_chunks = count / chunk, covered = n_chunks * chunk;
    const size_t per = chunk < (size_t)kTile ? chunk : (size_t)kTile;  // samples of a partial
    const size_t n_partials = covered / per;
    std::vector<float> part(n_partials);
    if (n_partials) {
        const size_t tiles = (covered + kTile - 1) / kTile;
        TOPO_REQUIRE(tiles <= 0x7fffffffu, "mean_std_f32: %zu samples are more than one launch covers", count);
        void* d_part = nullptr;
        TOPO_TRY(workspace(0, n_partials * sizeof(float), &d_part));
        const bool vec = ((uintptr_t)in & 15) == 0;
        const dim3 grid((unsigned)tiles), block(kNpThreads);
        const int group = (int)(per / kLeaf);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, c.compute, in, covered, mean, group, n_partials, (float*)d_part);
        };
        if (vec) {
            sq ? launch(np_partials_kernel<true, true>) : launch(np_partials_kernel<true, false>);
        } else {
            sq ? launch(np_partials_kernel<false, true>) : launch(np_partials_kernel<false, false>);
        }
        TOPO_HIP(hipGetLastError());
        TOPO_HIP(hipMemcpyAsync(part.data(), d_part, n_partials * sizeof(float), hipMemcpyDeviceToHost, c.compute));
        TOPO_HIP(hipStreamSynchronize(c.compute));
    }
    // a chunk longer than a tile: the upper levels of its tree, neighbours combined
    for (size_t m = chunk / per; m > 1; m /= 2) {
        for (size_t i = 0; i < n_chunks * (m / 2); ++i) part[i] = part[2 * i] + part[2 * i + 1];
    }
    float s = 0.0f;
    for (size_t i = 0; i < n_chunks; ++i) s = s + part[i];
    if (!tail.empty()) {
        if (sq) {
            std::vector<float> dev2(tail.size());
            for (size_t i = 0; i < tail.size(); ++i) {
                const float d = tail[i] - mean;
                dev2[i] = d * d;
            }
            s = s + pairwise_host(dev2.data(), dev2.size());
        } else {
            s = s + pairwise_host(tail.data(), tail.size());
        }
    }
    *sum = s;
    return TOPO_AMD_OK;
}

}  // namespace

int launch_mean_std_np(const float* in, size_t count, size_t chunk, float* mean, float* stdev) {
    TOPO_REQUIRE(chunk >= (size_t)kLeaf && (chunk & (chunk - 1)) == 0, "mean_std_f32: chunk %zu (a power of two, 128 at least)", chunk);
    Context& c = ctx();
    std::vector<float> tail(count % chunk);
    if (!tail.empty())
        TOPO_HIP(hipMemcpyAsync(tail.data(), in + (count - tail.size()), tail.size() * sizeof(float), hipMemcpyDeviceToHost, c.compute));
    TOPO_HIP(hipStreamSynchronize(c.compute));
    const float n = (float)count;
    float sum = 0.0f, sum2 = 0.0f;
    TOPO_TRY(np_sum(in, count, chunk, false, 0.0f, tail, &sum));
    const float m = sum / n;
    TOPO_TRY(np_sum(in, count, chunk, true, m, tail, &sum2));
    *mean = m;
    *stdev = std::sqrt(sum2 / n);
    return TOPO_AMD_OK;
}

}  // namespace topo
