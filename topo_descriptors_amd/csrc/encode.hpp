// The encode of a float32 result sample into the type a file stores it in (include/topo_amd.h, "packed result planes"),
// stated once for the host and once for the device.  Everything that packs a result plane - the encode kernel (encode.hip),
// topo_amd_encode_host, topo_amd_encode_dev and the row chunks of the *_packed entry points (host_api.hip) - goes through these
// two templates.  For an integer type T, [lo, hi] being T's range without the nodata code:
//
//     code = nodata                                  if v is NaN                      (counted in `missing`)
//     q    = rint( ((double)v - offset) / scale )    otherwise
//     code = lo if q < lo, hi if q > hi              (+-inf included; counted in `saturated`)
//     code = (T) q                                   otherwise
//
// The difference and the quotient are each rounded in float64 (a true division, no reciprocal: __dsub_rn / __ddiv_rn on the
// device, contraction off on the host), rint rounds to nearest-even.  The nodata code is T's lowest or highest code and
// lies outside [lo, hi], so no value is ever stored as nodata: decode(encode(v)) is NaN exactly where v is NaN.
// Half (TOPO_AMD_F16): float32 -> binary16, round to nearest-even; NaN is 0x7E00 (counted in `missing`), a finite sample
// that becomes +-inf is counted in `saturated`.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "common.hpp"

namespace topo {

struct EncodeParams {
    double scale = 1.0, offset = 0.0;
    double lo = 0.0, hi = 0.0;  // the type's range without the nodata code
    int32_t nodata = 0;         // the code of a NaN
    int32_t dtype = TOPO_AMD_F32;
    bool plain() const { return dtype == TOPO_AMD_F32; }  // float32 passed through: nothing to encode
};

struct Half {  // the sample type of TOPO_AMD_F16
    uint16_t bits;
};
constexpr uint16_t kHalfNaN = 0x7e00, kHalfInf = 0x7c00;

// float32 bits (not a NaN) -> binary16 bits, round to nearest-even
inline uint16_t half_bits_host(uint32_t x) {
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    const uint32_t mag = x & 0x7fffffffu;
    if (mag >= 0x47800000u) return sign | kHalfInf;  // 65536 and beyond, inf
    if (mag >= 0x38800000u) {                        // 2^-14 and beyond: a normal binary16, unless the rounding carries into inf
        const uint32_t m = mag - 0x38000000u;
        return sign | (uint16_t)((m + 0xfffu + ((m >> 13) & 1u)) >> 13);
    }
    const uint32_t e = mag >> 23;
    if (e < 102) return sign;  // below 2^-25: zero
    const uint32_t m = (mag & 0x7fffffu) | 0x800000u, shift = 126 - e;  // 14 ... 24: units of 2^-24
    uint32_t h = m >> shift;
    const uint32_t rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rest > half || (rest == half && (h & 1u))) ++h;
    return sign | (uint16_t)h;
}

template <class T>
inline T encode_host(float v, const EncodeParams& p, uint64_t& missing, uint64_t& saturated) {
#pragma clang fp contract(off)
    if (v != v) {
        ++missing;
        return (T)p.nodata;
    }
    const double d = (double)v - p.offset;
    const double q = std::rint(d / p.scale);
    if (q < p.lo || q > p.hi) {
        ++saturated;
        return (T)(int32_t)(q < p.lo ? p.lo : p.hi);
    }
    return (T)(int32_t)q;
}
template <>
inline Half encode_host<Half>(float v, const EncodeParams&, uint64_t& missing, uint64_t& saturated) {
    if (v != v) {
        ++missing;
        return Half{kHalfNaN};
    }
    uint32_t x;
    std::memcpy(&x, &v, sizeof x);
    const uint16_t h = half_bits_host(x);
    if ((h & 0x7fffu) == kHalfInf && (x & 0x7fffffffu) != 0x7f800000u) ++saturated;
    return Half{h};
}

template <class T>
__device__ __forceinline__ T encode_dev(float v, const EncodeParams& p, unsigned& missing, unsigned& saturated) {
    const double q = rint(__ddiv_rn(__dsub_rn((double)v, p.offset), p.scale));
    const bool nan = v != v, below = q < p.lo, above = q > p.hi;
    missing += nan;
    saturated += !nan && (below || above);  // (a NaN compares false)
    const int32_t code = nan ? p.nodata : (int32_t)(below ? p.lo : (above ? p.hi : q));
    return (T)code;
}
template <>
__device__ __forceinline__ Half encode_dev<Half>(float v, const EncodeParams&, unsigned& missing, unsigned& saturated) {
    const _Float16 h = (_Float16)v;  // v_cvt_f16_f32: nearest-even, binary16 denormals kept
    uint16_t bits = __builtin_bit_cast(uint16_t, h);
    const bool nan = v != v;
    missing += nan;
    saturated += (bits & 0x7fffu) == kHalfInf && (__float_as_uint(v) & 0x7fffffffu) != 0x7f800000u;
    return Half{nan ? kHalfNaN : bits};
}

// f(T()) with the sample type of an encoded plane's dtype code; false: float32 (nothing to encode) or no such code
template <class F>
inline bool with_code_type(int dtype, F&& f) {
    switch (dtype) {
        case TOPO_AMD_I16: f(int16_t()); return true;
        case TOPO_AMD_U16: f(uint16_t()); return true;
        case TOPO_AMD_U8: f(uint8_t()); return true;
        case TOPO_AMD_F16: f(Half()); return true;
        default: return false;
    }
}
inline size_t plane_sample_bytes(int dtype) {
    size_t n = dtype == TOPO_AMD_F32 ? sizeof(float) : 0;
    with_code_type(dtype, [&](auto t) { n = sizeof(t); });
    return n;
}

// encode.hip
// A caller's topo_amd_plane checked against the rules above -> the parameters of its encode (TOPO_AMD_EINVAL otherwise)
int make_encode(const topo_amd_plane* plane, const char* who, EncodeParams* p);
// count floats of in (device) -> out (device, aligned to its sample type) on `stream`; the kernel ADDS its samples stored as
// nodata / NaN to counts[0] and its clamped ones to counts[1] (device; zeroed on the same stream in front of the first launch)
int launch_encode(hipStream_t stream, const float* in, size_t count, const EncodeParams& p, void* out, unsigned long long* counts);
// the same on host arrays (one thread: the CPU statement of the formula, not a fast path); the counters are SET
int encode_host_array(const float* in, size_t count, const EncodeParams& p, void* out, uint64_t* missing, uint64_t* saturated);

// finish.hip
// Window [row0, row0 + rows) x [col0, col0 + cols) of the float32 plane `in` (device, nx samples a row; the caller has
// checked that the window lies inside it) -> out (device, rows * cols compact samples of p.dtype, float32 included, aligned
// to the sample type) on `stream`: NaN where `mask` (device, uint8, indexed like `in`; or NULL) is not 0, then encode_dev.
// The counters as launch_encode's; for float32 counts[0] receives the NaNs stored.
int launch_finish(hipStream_t stream, const float* in, int nx, const uint8_t* mask, int row0, int rows, int col0, int cols,
                  const EncodeParams& p, void* out, unsigned long long* counts);

}  // namespace topo
