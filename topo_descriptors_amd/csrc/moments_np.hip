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
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
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

// ---- the same order on row shards (topo_amd_shard_mean_std_f32) ----------------------------------------------------------------
// A rank owns samples [first, first + n) of the raster's `count`; numpy's chunks sit at GLOBAL offsets k * chunk.  What the
// ranks exchange in a pass is an array of 32-bit WORDS whose size follows from (count, chunk, slots) alone:
//   words [0, np_shard_partials): the partial sums of the full chunks, indexed by global chunk (chunk / 8192 partials for a
//     chunk longer than a tile) - a rank fills the chunks that lie wholly inside its samples with np_partials_kernel started
//     at its first global chunk boundary;
//   pass 1 only, per slot (rank): 4 header words {first, n} as two 64-bit numbers, then the head and the tail fragment (the
//     samples before the first / after the last chunk boundary; all of them as head when there is no boundary), each in an
//     area of min(chunk, count) words.
// Every word is written by one rank and zero on all others, so a sum-reduction of the array as unsigned integers hands every
// rank every word bit for bit (NaN payloads and -0.0f included); np_shard_sum then runs numpy's chain over the same words
// on every rank: the chunk trees' upper levels, the straddling chunks put together from the fragments and summed with
// pairwise_host, the sums added one after the other from 0.0f.
namespace {
constexpr size_t kNpSlotHeader = 4;

struct NpWindow {
    size_t c0, c1;            // global chunks [c0, c1) lie wholly inside (c0 > c1: no chunk boundary among the samples)
    size_t head, tail, tail_at;  // fragment lengths, the tail's global offset
};
NpWindow np_window(size_t first, size_t n, size_t chunk) {
    NpWindow w;
    const size_t end = first + n;
    w.c0 = (first + chunk - 1) / chunk;
    w.c1 = end / chunk;
    if (w.c0 > w.c1) {
        w.head = n, w.tail = 0, w.tail_at = end;
    } else {
        w.head = w.c0 * chunk - first, w.tail = end - w.c1 * chunk, w.tail_at = w.c1 * chunk;
    }
    return w;
}
size_t np_frag_cap(size_t count, size_t chunk) { return chunk < count ? chunk : count; }
size_t np_per(size_t chunk) { return chunk < (size_t)kTile ? chunk : (size_t)kTile; }

// header and fragments of one slot: words[0 .. 4) the header, [4, 4 + cap) the head, [4 + cap, 4 + 2 cap) the tail
__global__ __launch_bounds__(kNpThreads) void np_fragments_kernel(const uint32_t* __restrict__ owned, unsigned long long first,
                                                                  unsigned long long n, unsigned long long head,
                                                                  unsigned long long tail, unsigned long long cap,
                                                                  uint32_t* __restrict__ words) {
    const size_t i = (size_t)blockIdx.x * kNpThreads + threadIdx.x;
    if (i == 0) {
        words[0] = (uint32_t)first, words[1] = (uint32_t)(first >> 32);
        words[2] = (uint32_t)n, words[3] = (uint32_t)(n >> 32);
    }
    if (i < head && i < cap) words[kNpSlotHeader + i] = owned[i];
    if (i < tail && i < cap) words[kNpSlotHeader + cap + i] = owned[n - tail + i];
}
float word_float(uint32_t w) {
    float f;
    std::memcpy(&f, &w, sizeof(f));
    return f;
}
}  // namespace

bool np_chunk_ok(size_t chunk) { return chunk >= (size_t)kLeaf && (chunk & (chunk - 1)) == 0; }

size_t np_shard_partials(size_t count, size_t chunk) { return (count / chunk) * (chunk / np_per(chunk)); }

size_t np_shard_words(size_t count, size_t chunk, int slots, bool fragments) {
    return np_shard_partials(count, chunk) + (fragments ? (size_t)slots * (kNpSlotHeader + 2 * np_frag_cap(count, chunk)) : 0);
}

// The window form of np_sum's device half: queues, on the compute stream, the partial sums of the full global chunks inside
// owned[0, n) = samples [first, first + n) of `count` into d_words (zeroed by the caller) and, !sq, the slot's header and
// fragments.  sq: of the squared deviations from `mean`.
int launch_np_shard_parts(const float* owned, size_t first, size_t n, size_t count, size_t chunk, int slot, bool sq, float mean,
                          uint32_t* d_words) {
    Context& c = ctx();
    TOPO_REQUIRE(n >= 1 && first + n <= count, "shard_mean_std_f32: samples [%zu, %zu) of a raster of %zu", first, first + n, count);
    const NpWindow w = np_window(first, n, chunk);
    if (w.c1 > w.c0) {
        const size_t per = np_per(chunk), covered = (w.c1 - w.c0) * chunk, n_partials = covered / per;
        const size_t tiles = (covered + kTile - 1) / kTile;
        TOPO_REQUIRE(tiles <= 0x7fffffffu, "shard_mean_std_f32: %zu samples are more than one launch covers", n);
        const float* in = owned + (w.c0 * chunk - first);  // the first global chunk boundary: 16-byte aligned whenever nx % 4 == 0
        float* partial = reinterpret_cast<float*>(d_words) + w.c0 * (chunk / per);
        const bool vec = ((uintptr_t)in & 15) == 0;
        const dim3 grid((unsigned)tiles), block(kNpThreads);
        const int group = (int)(per / kLeaf);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, c.compute, in, covered, mean, group, n_partials, partial);
        };
        if (vec) {
            sq ? launch(np_partials_kernel<true, true>) : launch(np_partials_kernel<true, false>);
        } else {
            sq ? launch(np_partials_kernel<false, true>) : launch(np_partials_kernel<false, false>);
        }
        TOPO_HIP(hipGetLastError());
    }
    if (!sq) {
        const size_t cap = np_frag_cap(count, chunk);
        TOPO_REQUIRE(w.head <= cap && w.tail <= cap, "shard_mean_std_f32: fragments of %zu / %zu samples", w.head, w.tail);
        uint32_t* area = d_words + np_shard_partials(count, chunk) + (size_t)slot * (kNpSlotHeader + 2 * cap);
        const size_t most = std::max<size_t>(1, std::max(w.head, w.tail));
        hipLaunchKernelGGL(np_fragments_kernel, dim3((unsigned)((most + kNpThreads - 1) / kNpThreads)), dim3(kNpThreads), 0, c.compute,
                           reinterpret_cast<const uint32_t*>(owned), (unsigned long long)first, (unsigned long long)n,
                           (unsigned long long)w.head, (unsigned long long)w.tail, (unsigned long long)cap, area);
        TOPO_HIP(hipGetLastError());
    }
    return TOPO_AMD_OK;
}

// The host chain of a pass.  `words`: the pass's reduced array (its partial sums); `fragments`: pass 1's reduced array (headers
// and raw fragments; == words in pass 1).  Refuses slots that do not tile the raster's samples.
int np_shard_sum(const uint32_t* words, const uint32_t* fragments, size_t count, size_t chunk, int slots, bool sq, float mean,
                 float* sum) {
    const size_t n_chunks = count / chunk, ppc = chunk / np_per(chunk), cap = np_frag_cap(count, chunk);
    struct Slot {
        size_t first, n;
        const uint32_t* head;
        NpWindow w;
    };
    std::vector<Slot> s;
    for (int k = 0; k < slots; ++k) {
        const uint32_t* a = fragments + np_shard_partials(count, chunk) + (size_t)k * (kNpSlotHeader + 2 * cap);
        Slot t{(size_t)a[0] | (size_t)a[1] << 32, (size_t)a[2] | (size_t)a[3] << 32, a + kNpSlotHeader, {}};
        if (t.n == 0) continue;
        TOPO_REQUIRE(t.first <= count && t.n <= count - t.first, "shard_mean_std_f32: a rank reports samples [%zu, +%zu) of %zu",
                     t.first, t.n, count);
        t.w = np_window(t.first, t.n, chunk);
        s.push_back(t);
    }
    std::sort(s.begin(), s.end(), [](const Slot& a, const Slot& b) { return a.first < b.first; });
    size_t at = 0;
    for (const Slot& t : s) {
        TOPO_REQUIRE(t.first == at, "shard_mean_std_f32: the ranks' rows do not tile the raster (sample %zu is owned %s)", at,
                     t.first > at ? "by nobody" : "twice");
        at = t.first + t.n;
    }
    TOPO_REQUIRE(at == count, "shard_mean_std_f32: the ranks' rows do not tile the raster (%zu of %zu samples)", at, count);
    std::vector<char> full(n_chunks, 0);  // summed on some rank's GPU
    for (const Slot& t : s)
        for (size_t k = t.w.c0; k < t.w.c1; ++k) full[k] = 1;
    std::vector<float> tree(ppc), piece;
    float acc = 0.0f;
    const size_t total = n_chunks + (count % chunk ? 1 : 0);
    for (size_t k = 0; k < total; ++k) {
        if (k < n_chunks && full[k]) {
            for (size_t i = 0; i < ppc; ++i) tree[i] = word_float(words[k * ppc + i]);
            for (size_t m = ppc; m > 1; m /= 2)
                for (size_t i = 0; i < m / 2; ++i) tree[i] = tree[2 * i] + tree[2 * i + 1];
            acc = acc + tree[0];
            continue;
        }
        const size_t lo = k * chunk, hi = std::min(lo + chunk, count);
        piece.clear();
        for (const Slot& t : s) {
            if (t.first + t.n <= lo || t.first >= hi) continue;
            auto take = [&](const uint32_t* from, size_t start, size_t len) {
                if (len == 0 || start < lo || start >= hi) return;
                for (size_t i = 0; i < len; ++i) piece.push_back(word_float(from[i]));
            };
            take(t.head, t.first, t.w.head);
            take(t.head + cap, t.w.tail_at, t.w.tail);
        }
        TOPO_REQUIRE(piece.size() == hi - lo, "shard_mean_std_f32: %zu of the %zu samples of chunk %zu arrived", piece.size(), hi - lo, k);
        if (sq) {
            for (float& v : piece) {
                const float d = v - mean;
                v = d * d;
            }
        }
        acc = acc + pairwise_host(piece.data(), piece.size());
    }
    *sum = acc;
    return TOPO_AMD_OK;
}

}  // namespace topo
