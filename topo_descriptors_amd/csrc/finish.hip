// K-finish: the last step of a wrapper call on the device - a window of a float32 result plane, with NaN put back where a
// uint8 mask plane says so, stored as the compact array a file holds: float32 as it is, or the packed samples of encode.hpp
// (encode_dev per sample, the formula is not restated here).  Only the window then crosses the link; no float32 copy of it
// is made for the packed types.
//
// A streaming pass, 4 B + 1 B of mask in and 1 - 4 B out per window sample, bound by HBM.  The compact output is ONE flat
// array of rows * cols samples: a lane takes whole 16-byte store groups of it (V = 4 floats, 8 two-byte samples, 16 uint8)
// and the grid strides over the groups, kFinishUnroll groups per lane and trip with their loads issued before the first
// conversion.  Nothing is assumed about nx, col0 or cols: the source row start (row0 + r) * nx + col0 changes its 16-byte
// phase from row to row, and a group may straddle the end of a window row (cols < V: several).  So each group decides for
// itself: where its V samples lie inside one source row and their first float stands on a 16-byte boundary it takes 16-byte
// loads (and 4-byte loads of the mask, where those are aligned); otherwise it walks its samples one by one, stepping to the
// next source row where the window row ends.  The samples in front of the output's first 16-byte boundary and behind its
// last whole group are converted one by one by the first lanes of the grid.  Every read is of a window sample (r < rows,
// c < cols) and every store of one of the rows * cols output samples.
// The counters are those of encode.hip: per lane, per wave with shuffles, per block through LDS, one atomicAdd pair a block.
#include <algorithm>

#include "encode.hpp"

namespace topo {
namespace {

constexpr int kFinishThreads = 256;
constexpr int kFinishWaves = kFinishThreads / 64;
constexpr int kFinishUnroll = 2;       // groups per lane in flight
constexpr int kFinishBlocksPerCu = 8;  // resident blocks the grid is sized for
constexpr uint32_t kQuietNaN = 0x7fc00000u;  // what `array[ind_nans] = np.nan` stores in a float32 array

struct FinishWindow {
    size_t nx;          // samples per source row
    size_t first;       // row0 * nx + col0: the source index of window sample (0, 0)
    unsigned cols;
    bool narrow;        // rows * cols < 2^32: 32-bit divisions
};

__device__ __forceinline__ unsigned finish_wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // (lane 0 holds the sum)
}

// flat output index -> (window row, window column)
__device__ __forceinline__ void finish_split(size_t f, const FinishWindow& w, size_t& r, unsigned& c) {
    if (w.narrow) {
        const unsigned q = (unsigned)f / w.cols;
        r = q;
        c = (unsigned)f - q * w.cols;
    } else {
        r = f / w.cols;
        c = (unsigned)(f - r * w.cols);
    }
}

// the bits of one sample with the mask applied -> the stored sample
template <class T>
__device__ __forceinline__ T finish_sample(uint32_t bits, const EncodeParams& p, unsigned& missing, unsigned& saturated) {
    return encode_dev<T>(__uint_as_float(bits), p, missing, saturated);
}
template <>
__device__ __forceinline__ uint32_t finish_sample<uint32_t>(uint32_t bits, const EncodeParams&, unsigned& missing, unsigned&) {
    missing += (bits & 0x7fffffffu) > 0x7f800000u;  // a NaN, whatever its payload: copied bit for bit
    return bits;
}

// T: the stored sample (uint32_t: float32, moved as its bits)
template <class T>
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(const uint32_t* __restrict__ in, const uint8_t* __restrict__ mask,
                                                                T* __restrict__ out, size_t n, size_t head, size_t groups, FinishWindow w,
                                                                EncodeParams p, unsigned long long* __restrict__ counts) {
    constexpr int V = 16 / (int)sizeof(T), L = V / 4, U = kFinishUnroll;
    const size_t tid = (size_t)blockIdx.x * kFinishThreads + threadIdx.x, stride = (size_t)gridDim.x * kFinishThreads;
    const size_t body_end = head + groups * V;
    const size_t edge = head + (n - body_end);
    unsigned missing = 0, saturated = 0;
    for (size_t e = tid; e < edge; e += stride) {
        const size_t f = e < head ? e : body_end + (e - head);
        size_t r;
        unsigned c;
        finish_split(f, w, r, c);
        const size_t i = w.first + r * w.nx + c;
        const uint32_t bits = (mask && mask[i]) ? kQuietNaN : in[i];
        out[f] = finish_sample<T>(bits, p, missing, saturated);
    }
    uint4* dst = reinterpret_cast<uint4*>(out + head);
    union Raw {
        uint4 w[L];
        uint32_t s[V];
    };
    union Flags {
        uint32_t w[L];
        uint8_t s[V];
    };
    union Codes {
        uint4 w;
        T s[V];
    };
    for (size_t g0 = tid; g0 < groups; g0 += U * stride) {
        Raw raw[U];
        Flags flag[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = g0 + u * stride;
            if (g < groups) {
                size_t r;
                unsigned c;
                finish_split(head + g * V, w, r, c);
                size_t i = w.first + r * w.nx + c;
#pragma unroll
                for (int l = 0; l < L; ++l) flag[u].w[l] = 0;
                if (c + V <= w.cols && (uintptr_t)(in + i) % 16 == 0) {  // inside one source row, on a 16-byte boundary
#pragma unroll
                    for (int l = 0; l < L; ++l) raw[u].w[l] = *reinterpret_cast<const uint4*>(in + i + 4 * l);
                    if (mask) {
                        if ((uintptr_t)(mask + i) % 4 == 0) {
#pragma unroll
                            for (int l = 0; l < L; ++l) flag[u].w[l] = *reinterpret_cast<const uint32_t*>(mask + i + 4 * l);
                        } else {
#pragma unroll
                            for (int q = 0; q < V; ++q) flag[u].s[q] = mask[i + q];
                        }
                    }
                } else {  // sample by sample, on to the next source row where the window row ends
#pragma unroll
                    for (int q = 0; q < V; ++q) {
                        raw[u].s[q] = in[i];
                        if (mask) flag[u].s[q] = mask[i];
                        ++i;
                        if (++c == w.cols) {
                            c = 0;
                            i += w.nx - w.cols;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = g0 + u * stride;
            if (g < groups) {
                Codes codes;
#pragma unroll
                for (int q = 0; q < V; ++q)
                    codes.s[q] = finish_sample<T>(flag[u].s[q] ? kQuietNaN : raw[u].s[q], p, missing, saturated);
                dst[g] = codes.w;
            }
        }
    }
    __shared__ unsigned part[2][kFinishWaves];
    missing = finish_wave_sum(missing);
    saturated = finish_wave_sum(saturated);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = missing;
        part[1][threadIdx.x >> 6] = saturated;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0, s = 0;
#pragma unroll
        for (int k = 0; k < kFinishWaves; ++k) {
            m += part[0][k];
            s += part[1][k];
        }
        if (m) atomicAdd(counts, m);
        if (s) atomicAdd(counts + 1, s);
    }
}

template <class T>
int launch_typed(hipStream_t stream, const float* in, const uint8_t* mask, const FinishWindow& w, size_t n, const EncodeParams& p, T* out,
                 unsigned long long* counts) {
    constexpr size_t V = 16 / sizeof(T);
    // the samples in front of the output's first 16-byte boundary (the output is aligned to its sample type)
    const size_t head = std::min(n, (size_t)((16 - (uintptr_t)out % 16) % 16) / sizeof(T));
    const size_t groups = (n - head) / V;
    const size_t per_block = (size_t)kFinishThreads * kFinishUnroll;
    const size_t want = std::max<size_t>(1, (std::max(groups, n - groups * V) + per_block - 1) / per_block);
    const unsigned blocks = (unsigned)std::min<size_t>(want, (size_t)ctx().num_cu * kFinishBlocksPerCu);
    hipLaunchKernelGGL(finish_kernel<T>, dim3(blocks), dim3(kFinishThreads), 0, stream, reinterpret_cast<const uint32_t*>(in), mask, out, n,
                       head, groups, w, p, counts);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}

}  // namespace

int launch_finish(hipStream_t stream, const float* in, int nx, const uint8_t* mask, int row0, int rows, int col0, int cols,
                  const EncodeParams& p, void* out, unsigned long long* counts) {
    const size_t n = (size_t)rows * (size_t)cols;
    if (n == 0) return TOPO_AMD_OK;
    FinishWindow w;
    w.nx = (size_t)nx;
    w.first = (size_t)row0 * (size_t)nx + (size_t)col0;
    w.cols = (unsigned)cols;
    w.narrow = n < ((size_t)1 << 32);
    TOPO_REQUIRE((uintptr_t)in % sizeof(float) == 0 && (uintptr_t)out % plane_sample_bytes(p.dtype) == 0,
                 "finish: a pointer is not aligned to its sample type");
    if (p.plain()) return launch_typed(stream, in, mask, w, n, p, (uint32_t*)out, counts);
    int rc = TOPO_AMD_OK;
    const bool known = with_code_type(p.dtype, [&](auto t) { rc = launch_typed(stream, in, mask, w, n, p, (decltype(t)*)out, counts); });
    TOPO_REQUIRE(known, "finish: sample type %d has no encode", (int)p.dtype);
    return rc;
}

}  // namespace topo
