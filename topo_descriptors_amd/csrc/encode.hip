// K-encode: a float32 result plane turned into the samples a file stores - int16 / uint16 / uint8 codes with a scale, an
// offset and a nodata code, or binary16 - encode_dev of encode.hpp per sample.  The host pipeline (host_api.hip, HostCall::run)
// runs this on the compute stream behind each row chunk's kernels and downloads the packed rows, so a result crosses the
// link at a half or a quarter of the float32 bytes; decode.hip is its mirror on the upload side.
//
// A streaming conversion, 4 B in and 1 - 2 B out per sample, bound by HBM: a lane takes a group of V consecutive samples -
// one 16-byte store and the 16-byte loads that fill it (V = 8 floats in two loads for the 2-byte types, 16 in four for
// uint8) - and the grid strides over the groups, kEncodeUnroll groups per lane and trip with all their loads issued before
// the first conversion.  A flat run need not start on a 16-byte boundary (a row chunk of a raster with an odd number of
// columns) nor hold a whole number of groups: the samples before the first group boundary common to the input and the
// output, and those behind the last whole group, are converted one by one by the first lanes of the grid.  Input and output
// that share no group boundary (pointers of unrelated phase handed to topo_amd_encode_dev; never the pipeline, whose float32
// and packed planes are indexed alike) are converted sample by sample throughout.
// The two counters (samples stored as nodata / NaN, samples clamped) are summed per lane, per wave with shuffles, per block
// through 32 bytes of LDS; one lane of a block then adds them with an ordinary atomicAdd each to a pair of unsigned long
// long in device memory.  Plain vector stores otherwise.
#include <algorithm>

#include "encode.hpp"

namespace topo {
namespace {

constexpr int kEncodeThreads = 256;
constexpr int kEncodeWaves = kEncodeThreads / 64;
constexpr int kEncodeUnroll = 4;       // groups per lane in flight (2-byte types; uint8's groups are twice as long: 2)
constexpr int kEncodeBlocksPerCu = 8;  // resident blocks the grid is sized for

template <class T>
struct EncodeGroup {
    static constexpr int kSamples = 16 / (int)sizeof(T);  // V: one 16-byte store
    static constexpr int kLoads = kSamples / 4;           // 16-byte loads per group
    static constexpr int kUnroll = kEncodeUnroll * 2 / kLoads;
};

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // (lane 0 holds the sum)
}

// samples [0, head) and [head + groups * V, n): one by one; [head, head + groups * V): in groups (in + head and out + head are
// 16-byte aligned, or groups == 0)
template <class T>
__global__ __launch_bounds__(kEncodeThreads) void encode_kernel(const float* __restrict__ in, T* __restrict__ out, size_t n, size_t head,
                                                                size_t groups, EncodeParams p, unsigned long long* __restrict__ counts) {
    using G = EncodeGroup<T>;
    constexpr int V = G::kSamples, U = G::kUnroll;
    const size_t tid = (size_t)blockIdx.x * kEncodeThreads + threadIdx.x, stride = (size_t)gridDim.x * kEncodeThreads;
    const size_t body_end = head + groups * V;
    const size_t edge = head + (n - body_end);
    unsigned missing = 0, saturated = 0;
    for (size_t e = tid; e < edge; e += stride) {
        const size_t i = e < head ? e : body_end + (e - head);
        out[i] = encode_dev<T>(in[i], p, missing, saturated);
    }
    const uint4* src = reinterpret_cast<const uint4*>(in + head);
    uint4* dst = reinterpret_cast<uint4*>(out + head);
    union Raw {
        uint4 w[G::kLoads];
        float s[V];
    };
    union Codes {
        uint4 w;
        T s[V];
    };
    for (size_t g0 = tid; g0 < groups; g0 += U * stride) {
        Raw r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = g0 + u * stride;
            if (g < groups) {
#pragma unroll
                for (int l = 0; l < G::kLoads; ++l) r[u].w[l] = src[g * G::kLoads + l];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = g0 + u * stride;
            if (g < groups) {
                Codes c;
#pragma unroll
                for (int q = 0; q < V; ++q) c.s[q] = encode_dev<T>(r[u].s[q], p, missing, saturated);
                dst[g] = c.w;
            }
        }
    }
    __shared__ unsigned part[2][kEncodeWaves];
    missing = wave_sum(missing);
    saturated = wave_sum(saturated);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = missing;
        part[1][threadIdx.x >> 6] = saturated;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0, s = 0;
#pragma unroll
        for (int w = 0; w < kEncodeWaves; ++w) {
            m += part[0][w];
            s += part[1][w];
        }
        if (m) atomicAdd(counts, m);
        if (s) atomicAdd(counts + 1, s);
    }
}

template <class T>
int launch_typed(hipStream_t stream, const float* in, size_t n, const EncodeParams& p, T* out, unsigned long long* counts) {
    constexpr size_t V = EncodeGroup<T>::kSamples;
    TOPO_REQUIRE((uintptr_t)in % sizeof(float) == 0 && (uintptr_t)out % sizeof(T) == 0, "encode: a pointer is not aligned to its sample type");
    // the first sample at which the input and the output both stand on a 16-byte boundary (n: there is none)
    size_t head = n;
    for (size_t h = 0; h < 16; ++h)  // (16: the longest period, uint8's)
        if ((uintptr_t)(in + h) % 16 == 0 && (uintptr_t)(out + h) % 16 == 0) {
            head = std::min(h, n);
            break;
        }
    const size_t groups = (n - head) / V;
    const size_t per_block = (size_t)kEncodeThreads * EncodeGroup<T>::kUnroll;
    const size_t want = std::max<size_t>(1, (std::max(groups, n - groups * V) + per_block - 1) / per_block);
    const unsigned blocks = (unsigned)std::min<size_t>(want, (size_t)ctx().num_cu * kEncodeBlocksPerCu);
    hipLaunchKernelGGL(encode_kernel<T>, dim3(blocks), dim3(kEncodeThreads), 0, stream, in, out, n, head, groups, p, counts);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}

}  // namespace

int make_encode(const topo_amd_plane* plane, const char* who, EncodeParams* p) {
    TOPO_REQUIRE(plane != nullptr, "%s: NULL plane", who);
    const int dtype = plane->dtype;
    TOPO_REQUIRE(plane_sample_bytes(dtype) != 0, "%s: sample type %d of a result plane (TOPO_AMD_F32, _I16, _U16, _U8 or _F16)", who, dtype);
    TOPO_REQUIRE(std::isfinite(plane->scale) && plane->scale != 0.0, "%s: scale %g of a result plane (it must be finite and not 0)", who,
                 plane->scale);
    TOPO_REQUIRE(std::isfinite(plane->offset), "%s: offset %g of a result plane is not finite", who, plane->offset);
    *p = EncodeParams();
    p->dtype = dtype;
    if (dtype == TOPO_AMD_F32 || dtype == TOPO_AMD_F16) {
        TOPO_REQUIRE(plane->scale == 1.0 && plane->offset == 0.0 && !plane->has_nodata,
                     "%s: a %s result plane takes scale 1, offset 0 and no nodata", who, dtype == TOPO_AMD_F32 ? "float32" : "float16");
        return TOPO_AMD_OK;
    }
    const double lowest = dtype == TOPO_AMD_I16 ? -32768.0 : 0.0;
    const double highest = dtype == TOPO_AMD_I16 ? 32767.0 : (dtype == TOPO_AMD_U16 ? 65535.0 : 255.0);
    TOPO_REQUIRE(plane->has_nodata, "%s: an integer result plane needs a nodata code (NaN has no other place)", who);
    TOPO_REQUIRE(plane->nodata == lowest || plane->nodata == highest,
                 "%s: nodata %g of a result plane: it must be the type's lowest or highest code (%g or %g)", who, plane->nodata, lowest, highest);
    p->scale = plane->scale;
    p->offset = plane->offset;
    p->nodata = (int32_t)plane->nodata;
    p->lo = plane->nodata == lowest ? lowest + 1.0 : lowest;
    p->hi = plane->nodata == highest ? highest - 1.0 : highest;
    return TOPO_AMD_OK;
}

int launch_encode(hipStream_t stream, const float* in, size_t count, const EncodeParams& p, void* out, unsigned long long* counts) {
    if (count == 0) return TOPO_AMD_OK;
    int rc = TOPO_AMD_OK;
    const bool known = with_code_type(p.dtype, [&](auto t) { rc = launch_typed(stream, in, count, p, (decltype(t)*)out, counts); });
    TOPO_REQUIRE(known, "encode: sample type %d has no encode", (int)p.dtype);
    return rc;
}

int encode_host_array(const float* in, size_t count, const EncodeParams& p, void* out, uint64_t* missing, uint64_t* saturated) {
    uint64_t m = 0, s = 0;
    const bool known = with_code_type(p.dtype, [&](auto t) {
        decltype(t)* codes = (decltype(t)*)out;
        for (size_t i = 0; i < count; ++i) codes[i] = encode_host<decltype(t)>(in[i], p, m, s);
    });
    TOPO_REQUIRE(known, "encode: sample type %d has no encode", (int)p.dtype);
    *missing = m;
    *saturated = s;
    return TOPO_AMD_OK;
}

}  // namespace topo
