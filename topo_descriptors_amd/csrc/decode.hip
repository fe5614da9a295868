// K-decode: a raster as it is stored (int16 / uint16 / int32 / uint8 / float64, or float32 with a scale, an offset or a
// nodata value) turned into the float32 plane every other kernel reads - decode_dev of decode.hpp per sample.  The host
// pipeline (host_api.hip, HostCall::run) uploads the caller's bytes as they are and runs this on the upload stream behind each
// row chunk's copy, so the single-threaded host cast in front of a call is gone and int16 rasters cross the link at half
// the bytes.
//
// A streaming conversion, 2 / 4 / 8 B in and 4 B out per sample, bound by HBM: a lane takes a group of V consecutive
// samples - whole 16-byte loads and whole 16-byte stores (V = 16 B of input for the 1- and 2-byte types, one 16-byte store
// for the others) - and the grid strides over the groups, kDecodeUnroll groups per lane and trip with all their loads issued
// before the first conversion.  A flat run need not start on a 16-byte boundary (a row chunk of an int16 raster with an
// odd number of columns) nor hold a whole number of groups: the samples before the first group boundary common to the
// input and the output, and those behind the last whole group, are converted one by one by the first lanes of the grid.
// Input and output that share no group boundary (pointers of unrelated phase handed to topo_amd_decode_dev; never the
// pipeline, whose raw and float32 planes are indexed alike) are converted sample by sample throughout.
// No LDS, no atomics, plain vector stores.
#include <algorithm>

#include "decode.hpp"

namespace topo {
namespace {

constexpr int kDecodeThreads = 256;
constexpr int kDecodeUnroll = 4;       // groups per lane in flight
constexpr int kDecodeBlocksPerCu = 8;  // resident blocks the grid is sized for

template <class T>
struct DecodeGroup {
    static constexpr int kSamples = sizeof(T) >= 4 ? 4 : 16 / (int)sizeof(T);  // V
    static constexpr int kLoads = kSamples * (int)sizeof(T) / 16;              // 16-byte loads per group
    static constexpr int kStores = kSamples / 4;                               // 16-byte stores per group
};

// samples [0, head) and [head + groups * V, n): one by one; [head, head + groups * V): in groups (in + head and out + head are
// 16-byte aligned, or groups == 0)
template <class T>
__global__ __launch_bounds__(kDecodeThreads) void decode_kernel(const T* __restrict__ in, float* __restrict__ out, size_t n, size_t head,
                                                                size_t groups, DecodeParams p) {
    using G = DecodeGroup<T>;
    constexpr int V = G::kSamples;
    const size_t tid = (size_t)blockIdx.x * kDecodeThreads + threadIdx.x, stride = (size_t)gridDim.x * kDecodeThreads;
    const size_t body_end = head + groups * V;
    const size_t edge = head + (n - body_end);
    for (size_t e = tid; e < edge; e += stride) {
        const size_t i = e < head ? e : body_end + (e - head);
        out[i] = decode_dev(in[i], p);
    }
    const uint4* src = reinterpret_cast<const uint4*>(in + head);
    uint4* dst = reinterpret_cast<uint4*>(out + head);
    union Raw {
        uint4 w[G::kLoads];
        T s[V];
    };
    for (size_t g0 = tid; g0 < groups; g0 += kDecodeUnroll * stride) {
        Raw r[kDecodeUnroll];
#pragma unroll
        for (int u = 0; u < kDecodeUnroll; ++u) {
            const size_t g = g0 + u * stride;
            if (g < groups) {
#pragma unroll
                for (int l = 0; l < G::kLoads; ++l) r[u].w[l] = src[g * G::kLoads + l];
            }
        }
#pragma unroll
        for (int u = 0; u < kDecodeUnroll; ++u) {
            const size_t g = g0 + u * stride;
            if (g < groups) {
#pragma unroll
                for (int q = 0; q < G::kStores; ++q) {
                    uint4 o;
                    o.x = __float_as_uint(decode_dev(r[u].s[4 * q + 0], p));
                    o.y = __float_as_uint(decode_dev(r[u].s[4 * q + 1], p));
                    o.z = __float_as_uint(decode_dev(r[u].s[4 * q + 2], p));
                    o.w = __float_as_uint(decode_dev(r[u].s[4 * q + 3], p));
                    dst[g * G::kStores + q] = o;
                }
            }
        }
    }
}

template <class T>
int launch_typed(hipStream_t stream, const T* in, size_t n, const DecodeParams& p, float* out) {
    constexpr size_t V = DecodeGroup<T>::kSamples;
    TOPO_REQUIRE((uintptr_t)in % sizeof(T) == 0 && (uintptr_t)out % sizeof(float) == 0, "decode: a pointer is not aligned to its sample type");
    // the first sample at which the input and the output both stand on a 16-byte boundary (n: there is none)
    size_t head = n;
    for (size_t h = 0; h < 16; ++h)  // (16: the longest period, uint8's)
        if ((uintptr_t)(in + h) % 16 == 0 && (uintptr_t)(out + h) % 16 == 0) {
            head = std::min(h, n);
            break;
        }
    const size_t groups = (n - head) / V;
    const size_t per_block = (size_t)kDecodeThreads * kDecodeUnroll;
    const size_t want = std::max<size_t>(1, (std::max(groups, n - groups * V) + per_block - 1) / per_block);
    const unsigned blocks = (unsigned)std::min<size_t>(want, (size_t)ctx().num_cu * kDecodeBlocksPerCu);
    hipLaunchKernelGGL(decode_kernel<T>, dim3(blocks), dim3(kDecodeThreads), 0, stream, in, out, n, head, groups, p);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}

}  // namespace

int launch_decode(hipStream_t stream, const void* raw, int dtype, size_t count, const DecodeParams& p, float* out) {
    if (count == 0) return TOPO_AMD_OK;
    int rc = TOPO_AMD_OK;
    const bool known = with_sample_type(dtype, [&](auto t) { rc = launch_typed(stream, (const decltype(t)*)raw, count, p, out); });
    TOPO_REQUIRE(known, "decode: unknown sample type %d", dtype);
    return rc;
}

int decode_host_array(const void* raw, int dtype, size_t count, const DecodeParams& p, float* out) {
    const bool known = with_sample_type(dtype, [&](auto t) {
        const decltype(t)* in = (const decltype(t)*)raw;
        for (size_t i = 0; i < count; ++i) out[i] = decode_host(in[i], p);
    });
    TOPO_REQUIRE(known, "decode: unknown sample type %d", dtype);
    return TOPO_AMD_OK;
}

}  // namespace topo
