// The decode of a stored raster sample (include/topo_amd.h, "raw sources"), stated once for the host and once for the
// device.  Everything that turns a stored sample into the float32 the kernels read - the decode kernel (decode.hip),
// topo_amd_decode_host and the raster-class scan of a caller's array (raster_class.hip) - goes through these two templates.
//
//     value = NaN                                       if has_nodata and (double)raw == nodata
//     value = (float) ( (double)raw * scale + offset )  otherwise
//
// The product and the sum are each rounded in float64 (no FMA: __dmul_rn / __dadd_rn on the device, contraction off on the
// host), the result is rounded to nearest-even to float32.  NaN is 0x7FC00000 on both sides.
#pragma once

#include <cstddef>
#include <cstdint>
#include <limits>

#include "common.hpp"

namespace topo {

struct DecodeParams {
    double scale = 1.0, offset = 0.0, nodata = 0.0;
    int has_nodata = 0;
};

template <class T>
inline float decode_host(T raw, const DecodeParams& p) {
#pragma clang fp contract(off)
    const double x = (double)raw;
    if (p.has_nodata && x == p.nodata) return std::numeric_limits<float>::quiet_NaN();
    const double scaled = x * p.scale;
    return (float)(scaled + p.offset);
}

template <class T>
__device__ __forceinline__ float decode_dev(T raw, const DecodeParams& p) {
    const double x = (double)raw;
    const float v = (float)__dadd_rn(__dmul_rn(x, p.scale), p.offset);
    return p.has_nodata && x == p.nodata ? __uint_as_float(0x7fc00000u) : v;
}

// f(T()) with the sample type of a TOPO_AMD_* dtype code; false: no such code
template <class F>
inline bool with_sample_type(int dtype, F&& f) {
    switch (dtype) {
        case TOPO_AMD_F32: f(float()); return true;
        case TOPO_AMD_I16: f(int16_t()); return true;
        case TOPO_AMD_U16: f(uint16_t()); return true;
        case TOPO_AMD_I32: f(int32_t()); return true;
        case TOPO_AMD_U8: f(uint8_t()); return true;
        case TOPO_AMD_F64: f(double()); return true;
        default: return false;
    }
}
inline size_t sample_bytes(int dtype) {
    size_t n = 0;
    with_sample_type(dtype, [&](auto t) { n = sizeof(t); });
    return n;
}

// decode.hip
// count samples of raw (device) -> out (device) on `stream`; both pointers aligned to their sample type
int launch_decode(hipStream_t stream, const void* raw, int dtype, size_t count, const DecodeParams& p, float* out);
// the same on host arrays (one thread: the CPU statement of the formula, not a fast path)
int decode_host_array(const void* raw, int dtype, size_t count, const DecodeParams& p, float* out);

}  // namespace topo
