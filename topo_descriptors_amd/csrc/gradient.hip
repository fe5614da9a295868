// K4 / K5: the gradient -> slope / aspect epilogue, Sobel, and axis 1 of the Gaussian fused with the epilogue (LDS-tiled
// and by wavefront shifts).  The smooths themselves are gauss.hip and gauss_f16.hip; which radius gets which kernel:
// gauss_route.hpp.
//
// Replaces numpy.gradient plus the normalisation / slope / aspect arithmetic (topo.py:631-642, :707-712) and
// scipy.ndimage.convolve with the Sobel pair (topo.py:679-683).
#include "gauss.hpp"
#include "atan.hpp"

namespace topo {

// What topo_amd_gradient_route reports (include/topo_amd.h): the launchers of the three units note what they decide as
// they go, launch_gradient clears the note first and packs it once its launches succeeded.  (The Gaussian writes it too;
// nobody reads that.)
thread_local GradNote t_grad;

namespace {

// ---- slope / aspect arithmetic -----------------------------------------------------------------
// The libm routines (atanf, atan2f, IEEE division with scaling) cost ~300 instructions per pixel
// together and made the epilogue VALU-bound at 3 TB/s.  These replacements keep float32-level
// accuracy (atan: Abramowitz & Stegun 4.4.49, |err| <= 2e-8 on [0,1]; division: reciprocal plus
// one FMA correction, correctly rounded except in rare half-way cases) and the IEEE special cases
// the descriptors rely on: signed zeros (flat terrain: dy = -0 -> atan2(+0,-0) = pi -> aspect 0),
// NaN propagation, and numpy's values for infinite gradients: dx, dy +-inf, slope 90 (np.hypot: an infinite component wins
// over a NaN one), aspect atan2's (90 / 270 for an infinite dx, 0 / 180 for an infinite dy, 45 ... 315 for both).
__device__ __forceinline__ float div_f32(float a, float b) {
    const float r = __builtin_amdgcn_rcpf(b);
    const float q = a * r;
    const float c = fmaf(fmaf(-q, b, a), r, q);
    return fabsf(q) == INFINITY ? q : c;  // (the correction of an infinite quotient is inf - inf)
}

__device__ __forceinline__ float atan2_f32(float y, float x) {
    const float a = fabsf(y), b = fabsf(x);
    const float mx = fmaxf(a, b), mn = fminf(a, b);
    // (both infinite: inf * rcp(inf) would be NaN; atan2 says pi / 4)
    const float t = mx == 0.0f ? 0.0f : (mn == INFINITY ? 1.0f : mn * __builtin_amdgcn_rcpf(mx));
    float r = atan_unit(t);
    if (a > b) r = 1.5707963267948966f - r;
    if (__float_as_uint(x) >> 31) r = 3.14159265358979323846f - r;  // sign BIT: x = -0 counts
    r = copysignf(r, y);
    return (x != x || y != y) ? NAN : r;
}

__device__ __forceinline__ void resolution_at(const GradArgs& p, int oy, int ox, float& rx, float& ry) {
    if (p.res_mode == TOPO_AMD_RES_SCALAR) {
        rx = p.res_x[0];
        ry = p.res_y[0];
    } else if (p.res_mode == TOPO_AMD_RES_1D) {
        rx = p.res_x[ox];
        ry = p.res_y[oy];
    } else {
        const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
        rx = p.res_x[o];
        ry = p.res_y[o];
    }
}

// dx, dy in -> normalised dx, dy, slope and aspect in degrees (topo.py:637-642)
__device__ __forceinline__ void gradient_values(float& dx, float& dy, float rx, float ry, float& slope,
                                                float& aspect) {
    dx = div_f32(dx, rx);  // signed resolutions: -0.0 must survive (aspect of flat terrain)
    dy = div_f32(dy, ry);
    const float rad2deg = 57.29577951308232f;
    const float d2 = dx * dx;
    const float e2 = dy * dy;
    const float h = fmaxf(fabsf(dx), fabsf(dy)) == INFINITY ? INFINITY : __builtin_amdgcn_sqrtf(d2 + e2);  // (fmaxf drops a NaN)
    slope = atan_pos(h) * rad2deg;
    float a = 180.0f + atan2_f32(dx, dy) * rad2deg;
    if (a >= 360.0f) a -= 360.0f;  // float32 "% 360" of a value in [0, 360]
    aspect = a;
}

__device__ __forceinline__ void finish_gradient(const GradArgs& p, int oy, int ox, float dx,
                                                float dy) {
    const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
    float rx, ry, slope, aspect;
    resolution_at(p, oy, ox, rx, ry);
    gradient_values(dx, dy, rx, ry, slope, aspect);
    if (p.dx) p.dx[o] = dx;
    if (p.dy) p.dy[o] = dy;
    if (p.slope) p.slope[o] = slope;
    if (p.aspect) p.aspect[o] = aspect;
}

__device__ __forceinline__ void epilogue_pixel(const GradArgs& p, int oy, int ox);
__global__ __launch_bounds__(kThreads) void gradient_epilogue_kernel(GradArgs p) {
    const int ox = blockIdx.x * kThreads + threadIdx.x;
    const int oy = p.out_row0 + blockIdx.y;
    if (ox >= p.nx) return;
    epilogue_pixel(p, oy, ox);
}
// the epilogue behind a deferred two-pass smooth: nothing unless *p.run_if != 0; a grid of a few hundred rows that
// strides over the output rows (a million blocks that only read the flag would take a few hundred microseconds)
__global__ __launch_bounds__(kThreads) void gradient_epilogue_if_kernel(GradArgs p) {
    if (*p.run_if == 0) return;
    const int ox = blockIdx.x * kThreads + threadIdx.x;
    if (ox >= p.nx) return;
    for (int oy = p.out_row0 + blockIdx.y; oy < p.out_row0 + p.out_rows; oy += gridDim.y) epilogue_pixel(p, oy, ox);
}
__device__ __forceinline__ void epilogue_pixel(const GradArgs& p, int oy, int ox) {
    // numpy.gradient: central difference / 2 inside, first-order one-sided at the edges
    const float* rowx = p.gx_src + (size_t)(oy - p.s_row0) * p.nx;
    float dx;
    if (ox == 0) dx = rowx[1] - rowx[0];
    else if (ox == p.nx - 1) dx = rowx[ox] - rowx[ox - 1];
    else dx = (rowx[ox + 1] - rowx[ox - 1]) * 0.5f;
    const float* coly = p.gy_src + (size_t)(oy - p.s_row0) * p.nx + ox;
    float dy;
    if (oy == 0) dy = coly[p.nx] - coly[0];
    else if (oy == p.gny - 1) dy = coly[0] - coly[-p.nx];
    else dy = (coly[p.nx] - coly[-p.nx]) * 0.5f;
    finish_gradient(p, oy, ox, dx, dy);
}

// The same, four adjacent pixels per thread: 16-byte loads of the three smoothed rows and 16-byte stores of
// the four outputs (the one-pixel kernel moves the 20 B/pixel as dwords and ran at 3.2 TB/s).  Identical arithmetic
// per pixel, hence identical bits.  Any width from 8 columns (round 3: the 16-byte accesses only need dword alignment;
// the last 1 ... 3 pixels of a row whose length is not a multiple of 4 go one by one).
__device__ __forceinline__ void epilogue_row4(const GradArgs& p, int oy, int ox);
__global__ __launch_bounds__(kThreads) void gradient_epilogue4_kernel(GradArgs p) {
    const int ox = (blockIdx.x * kThreads + threadIdx.x) * 4;
    const int oy = p.out_row0 + blockIdx.y;
    if (ox >= p.nx) return;
    epilogue_row4(p, oy, ox);
}
__global__ __launch_bounds__(kThreads) void gradient_epilogue4_if_kernel(GradArgs p) {  // (see gradient_epilogue_if_kernel)
    if (*p.run_if == 0) return;
    const int ox = (blockIdx.x * kThreads + threadIdx.x) * 4;
    if (ox >= p.nx) return;
    for (int oy = p.out_row0 + blockIdx.y; oy < p.out_row0 + p.out_rows; oy += gridDim.y) epilogue_row4(p, oy, ox);
}
__device__ __forceinline__ void epilogue_row4(const GradArgs& p, int oy, int ox) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    if (ox + 4 > p.nx) {
        for (int x = ox; x < p.nx; ++x) epilogue_pixel(p, oy, x);
        return;
    }
    const float* rowx = p.gx_src + (size_t)(oy - p.s_row0) * p.nx;
    const f4 mid = *reinterpret_cast<const f4*>(rowx + ox);
    const float left = ox > 0 ? rowx[ox - 1] : 0.0f, right = ox + 4 < p.nx ? rowx[ox + 4] : 0.0f;
    const float* coly = p.gy_src + (size_t)(oy - p.s_row0) * p.nx + ox;
    const f4 cen = *reinterpret_cast<const f4*>(coly);
    const f4 up = oy > 0 ? *reinterpret_cast<const f4*>(coly - p.nx) : cen;
    const f4 dn = oy < p.gny - 1 ? *reinterpret_cast<const f4*>(coly + p.nx) : cen;
    f4 odx, ody, osl, oas;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int x = ox + t;
        const float xm = t == 0 ? left : mid[t == 0 ? 0 : t - 1], xp = t == 3 ? right : mid[t == 3 ? 3 : t + 1];
        // numpy.gradient: central difference / 2 inside, first-order one-sided at the edges
        float dx;
        if (x == 0) dx = mid[1] - mid[0];
        else if (x == p.nx - 1) dx = mid[3] - mid[2];
        else dx = (xp - xm) * 0.5f;
        float dy;
        if (oy == 0) dy = dn[t] - cen[t];
        else if (oy == p.gny - 1) dy = cen[t] - up[t];
        else dy = (dn[t] - up[t]) * 0.5f;
        float rx, ry, slope, aspect;
        resolution_at(p, oy, x, rx, ry);
        gradient_values(dx, dy, rx, ry, slope, aspect);
        odx[t] = dx;
        ody[t] = dy;
        osl[t] = slope;
        oas[t] = aspect;
    }
    const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
    // streaming stores (nobody reads the four planes back from the caches; the smoothed rows above and below are what
    // L2 should keep): gradient sigma 3.25 / 30.25 on 32768^2 5.95-6.38 / 9.12-9.30 -> 5.87-5.90 / 8.96-9.00 ms
    if (p.dx) __builtin_nontemporal_store(odx, reinterpret_cast<f4*>(p.dx + o));
    if (p.dy) __builtin_nontemporal_store(ody, reinterpret_cast<f4*>(p.dy + o));
    if (p.slope) __builtin_nontemporal_store(osl, reinterpret_cast<f4*>(p.slope + o));
    if (p.aspect) __builtin_nontemporal_store(oas, reinterpret_cast<f4*>(p.aspect + o));
}

__device__ __forceinline__ double raw_reflect(const GradArgs& p, int gy, int gx) {
    gy = reflect_index(gy, p.gny);
    gx = reflect_index(gx, p.nx);
    return (double)p.raw[(size_t)(gy - p.raw_row0) * p.nx + gx];
}

// Sobel pair / 8, true convolution (kernel flipped), evaluated in float64 like ndimage.
template <bool FINISH>
__global__ __launch_bounds__(kThreads) void sobel_kernel(GradArgs p) {
    const int ox = blockIdx.x * kThreads + threadIdx.x;
    const int oy = p.out_row0 + blockIdx.y;
    if (ox >= p.nx) return;
    const double nw = raw_reflect(p, oy - 1, ox - 1), n = raw_reflect(p, oy - 1, ox),
                 ne = raw_reflect(p, oy - 1, ox + 1);
    const double w = raw_reflect(p, oy, ox - 1), e = raw_reflect(p, oy, ox + 1);
    const double sw = raw_reflect(p, oy + 1, ox - 1), s = raw_reflect(p, oy + 1, ox),
                 se = raw_reflect(p, oy + 1, ox + 1);
    // float32 taps 1/8, 2/8 are exact; accumulate in double, round once
    const float dx = (float)(0.125 * (ne - nw) + 0.25 * (e - w) + 0.125 * (se - sw));
    const float dy = (float)(0.125 * (sw - nw) + 0.25 * (s - n) + 0.125 * (se - ne));
    if (FINISH) {
        finish_gradient(p, oy, ox, dx, dy);
    } else {
        const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
        if (p.dx) p.dx[o] = dx;
        if (p.dy) p.dy[o] = dy;
    }
}

// ---- axis 1 fused with the gradient epilogue -------------------------------------------------
// Same tiling as gauss_axis1_kernel, but the 64 x (NW*TB) smoothed tile stays in LDS and the
// block emits dx, dy, slope, aspect for the 62 x (NW*TB - 2) pixels inside it: the smoothed
// plane never goes to HBM (28 instead of 36 B/pixel for the whole gradient).  Tiles sit on
// global multiples of 62 rows / (NW*TB - 2) columns, so results do not depend on the row block.
//
// Blocks are persistent and walk the tile list in row-major order.  A stamped build of the
// one-tile-per-block version showed a wave spending 42 % of its time fetching its tile and 14 % in
// the convolution, so the next tile's samples are loaded into registers as soon as the current
// tile is in LDS and stay in flight through the convolution and the epilogue.  The barriers are raw
// s_barrier + lgkmcnt(0): __syncthreads() would also wait for those loads.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int TB, int KB, int NW, int PF>
__global__ __launch_bounds__(NW * 64) void gauss_axis1_grad_kernel(GaussArgs p, GradArgs g, int tiles_x, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    constexpr int TR = 64;
    constexpr int TC = NW * TB;
    constexpr int OUT_R = TR - 2, OUT_C = TC - 2;
    constexpr int RPW = TR / NW;  // tile rows fetched per wave
    // PF: samples per lane and row held in registers for the next tile, cols_l <= 64 PF (the launcher picks it)
    const int R = p.radius;
    const int cols_l = TC + p.nchunks * KB - 1;
    const int stride = cols_l | 1;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    float pf[RPW][PF];
    auto issue = [&](int tile) {
        const int sx0 = (tile % tiles_x) * OUT_C - 1;                                   // smoothed tile origin
        const int sy0 = (g.out_row0 / OUT_R + tile / tiles_x) * OUT_R - 1;
        const bool inner = sx0 - R >= 0 && sx0 - R + cols_l <= p.nx;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = wave + rr * NW;
            const int gy = min(max(sy0 + r, p.in_row0), p.in_row0 + p.in_rows - 1);  // unused rows clamp
            const float* src = p.in + (size_t)(gy - p.in_row0) * p.nx;
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                const int k = min(lane + 64 * q, cols_l - 1);
                pf[rr][q] = inner ? src[sx0 - R + k] : src[reflect_index(sx0 - R + k, p.nx)];
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            float* dst = L + (wave + rr * NW) * stride;
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                const int k = lane + 64 * q;
                if (k < cols_l) dst[k] = pf[rr][q];
            }
        }
    };

    int tile = blockIdx.x;
    if (tile < ntiles) issue(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        const int ox0 = (tile % tiles_x) * OUT_C;                                   // first output column
        const int oy0 = (g.out_row0 / OUT_R + tile / tiles_x) * OUT_R;               // first output row (global)
        lds_barrier();  // the previous tile's epilogue is done with the LDS image
        commit();
        lds_barrier();
        if (tile + (int)gridDim.x < ntiles) issue(tile + (int)gridDim.x);

        const float* rowp = L + lane * stride + wave * TB;
        auto fetch = [&](int i) -> float { return rowp[i]; };
        const float c = finite_or_zero(rowp[R]);
        float acc[TB];
        tap_chunks<TB, KB>(p.taps, p.nchunks, c, fetch, acc);
        lds_barrier();
        constexpr int ostride = TC + 1;
        float* O = L;  // smoothed tile, rounded to float32 like the reference's intermediate
#pragma unroll
        for (int t = 0; t < TB; ++t) O[lane * ostride + wave * TB + t] = c + acc[t];
        lds_barrier();

        for (int idx = threadIdx.x; idx < OUT_R * OUT_C; idx += NW * 64) {
            const int r = idx / OUT_C, k = idx % OUT_C;
            const int oy = oy0 + r, ox = ox0 + k;
            if (oy < g.out_row0 || oy >= g.out_row0 + g.out_rows || ox >= g.nx) continue;
            const float* q = O + (r + 1) * ostride + (k + 1);  // smoothed value of this pixel
            // numpy.gradient: central difference / 2 inside, first-order one-sided at the edges
            float dx, dy;
            if (ox == 0) dx = q[1] - q[0];
            else if (ox == g.nx - 1) dx = q[0] - q[-1];
            else dx = (q[1] - q[-1]) * 0.5f;
            if (oy == 0) dy = q[ostride] - q[0];
            else if (oy == g.gny - 1) dy = q[0] - q[-ostride];
            else dy = (q[ostride] - q[-ostride]) * 0.5f;
            finish_gradient(g, oy, ox, dx, dy);
        }
    }
}

// ---- axis 1 by wavefront shifts, fused with the gradient epilogue: no LDS at all -----------------
// Lanes own GC = 16 adjacent columns of one row (a wave-row is 1024 columns, 4 KiB, loaded with
// four coalesced dwordx4 per lane).  out[16L+t] = sum_k w[k] in[16L+t+k-R] is evaluated like the disc
// chain of disc_wave_impl.hpp: for each lane offset D the lane adds the contribution of its own 16
// samples to 16 partial sums (256 FMAs against 31 wave-uniform taps), and the partial sums hop
// one lane per step with a DPP wave shift.  The three most recent smoothed rows stay in
// registers, so the central differences, slope and aspect of a row are formed without the smoothed
// plane ever leaving the register file, and the four outputs leave as 64-byte pieces per lane.
//
// float32 accumulation keeps its digits through offsets: samples enter relative to the lane's own
// first sample, and that sample's offset from a wave-uniform base rides along as a 17th input with
// the summed taps (wsum), so every product is a small number.

struct WaveGradArgs {
    const float* in;   // plane already smoothed along axis 0: rows [in_row0, in_row0 + in_rows)
    int in_row0, in_rows;
    const float* wtab;  // nsteps x 32: taps w[GC*D + (j - 15) + R] for j = 0..30, zero outside the filter
    const float* wsum;  // nsteps x 16: for output sub-column t, sum over s of the taps applied to sample s
    int radius, d_lo, nsteps, nvl;
    int out_c;          // output columns per strip = GC * (nvl - 2)
    int rows_per_wave;
    float* smooth_out;  // non-NULL: store the smoothed rows themselves instead of the gradient
    GradArgs g;
};

#define GDPP_SHL1 0x130  // lane i takes lane i + 1
#define GDPP_SHR1 0x138  // lane i takes lane i - 1
__device__ __forceinline__ float hop_down(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), GDPP_SHL1, 0xf, 0xf, true));
}
__device__ __forceinline__ float hop_up(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), GDPP_SHR1, 0xf, 0xf, true));
}

__device__ __forceinline__ void wave_row_load(const WaveGradArgs& p, int gy, int xs, bool inner, float (&v)[GC]) {
    const int by = min(max(gy - p.in_row0, 0), p.in_rows - 1);  // rows outside only feed unused outputs
    const float* row = p.in + (size_t)by * p.g.nx;
    if (inner) {
#pragma unroll
        for (int q = 0; q < GC / 4; ++q) {
            const float4 f = *reinterpret_cast<const float4*>(row + xs + 4 * q);
            v[4 * q] = f.x;
            v[4 * q + 1] = f.y;
            v[4 * q + 2] = f.z;
            v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < GC; ++s) v[s] = row[reflect_index(xs + s, p.g.nx)];
    }
}

// smoothed values of one row: lane l ends up with the 16 columns of lane l - d_lo (valid l < nvl).
// Inputs enter the chain as small numbers only: x[s] = v[s] - v[0] (relief inside the lane's 16
// columns) and eps = v[0] - v[0] of the lane to the left, weighted with the cumulated taps wcum, which
// is an exact rewrite of sum_D wsum[D] (v0[L+D] - v0[L]); v0[L] itself is added once at the end.
__device__ __forceinline__ void wave_row_smooth(const WaveGradArgs& p, int lane, const float (&v)[GC],
                                                float (&out)[GC]) {
    const float eps = v[0] - hop_up(v[0]);
    float x[GC];
#pragma unroll
    for (int s = 0; s < GC; ++s) x[s] = v[s] - v[0];
    float acc[GC];
#pragma unroll
    for (int t = 0; t < GC; ++t) acc[t] = 0.0f;
    for (int step = 0; step < p.nsteps; ++step) {
        // Wave-uniform tap tables, read through the constant address space: the kernel stores to
        // global memory between uses, so as plain global pointers the compiler does not treat these
        // loads as invariant and fetched all 47 taps of a step through the vector path into VGPRs
        // (3.9e8 vector loads per 32768^2 launch, in a kernel at 246 VGPRs).  Nothing writes the
        // tables while the kernel runs.
        typedef const __attribute__((address_space(4))) float* cptr;
        cptr w = (cptr)p.wtab + step * 32;
        cptr wc = (cptr)p.wsum + step * GC;
#pragma unroll
        for (int t = 0; t < GC; ++t) {
            float a = step == 0 ? 0.0f : hop_down(acc[t]);
            a = fmaf(wc[t], eps, a);
#pragma unroll
            for (int sidx = 0; sidx < GC; ++sidx) a = fmaf(w[sidx - t + 15], x[sidx], a);
            acc[t] = a;
        }
    }
    // first sample of the lane whose columns these sums belong to
    const int src = min(lane - p.d_lo, 63);
    const float base = __int_as_float(__builtin_amdgcn_ds_bpermute(src * 4, __float_as_int(v[0])));
#pragma unroll
    for (int t = 0; t < GC; ++t) out[t] = acc[t] + base;
}

__global__ __launch_bounds__(kThreads) void gauss_axis1_wave_grad_kernel(WaveGradArgs p) {
    const GradArgs& g = p.g;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int ox0 = blockIdx.x * p.out_c;                      // first output column of the strip
    const int xs = ox0 - GC * (1 - p.d_lo) + GC * lane;        // first staged column of this lane
    const int col0 = ox0 + GC * (lane - 1);                    // first column this lane's results cover
    const bool inner = ox0 - GC * (1 - p.d_lo) >= 0 && ox0 - GC * (1 - p.d_lo) + 64 * GC <= g.nx &&
                       (g.nx & 3) == 0;
    const int tile = (g.out_row0 / p.rows_per_wave) + blockIdx.y * (kThreads / 64) + wave;
    const int y_begin = max(tile * p.rows_per_wave, g.out_row0);
    const int y_end = min((tile + 1) * p.rows_per_wave, g.out_row0 + g.out_rows);
    if (y_begin >= y_end) return;
    const bool lane_out = lane >= 1 && lane <= p.nvl - 2 && col0 < g.nx;
    const bool vec_ok = (g.nx & 3) == 0 && col0 + GC <= g.nx;
    float* planes[4] = {g.dx, g.dy, g.slope, g.aspect};

    float raw[GC], up[GC], mid[GC], dn[GC];
#pragma unroll
    for (int t = 0; t < GC; ++t) up[t] = mid[t] = 0.0f;
    wave_row_load(p, y_begin - 1, xs, inner, raw);
    // rows y_begin-1 .. y_end are smoothed one after the other; once three of them are there the
    // middle one is differenced and written
#pragma unroll 1
    for (int yy = y_begin - 1; yy <= y_end; ++yy) {
        wave_row_smooth(p, lane, raw, dn);
        if (yy < y_end) wave_row_load(p, yy + 1, xs, inner, raw);  // in flight during the epilogue
        const int y = yy - 1;  // row held in `mid`
        if (y >= y_begin) {
            // neighbours across the lane boundary
            const float left = hop_up(mid[GC - 1]);
            const float right = hop_down(mid[0]);
            if (lane_out && p.smooth_out) {
                const size_t o = (size_t)(y - g.out_row0) * g.nx + col0;
#pragma unroll
                for (int t = 0; t < GC; ++t)
                    if (col0 + t < g.nx) p.smooth_out[o + t] = mid[t];
            } else if (lane_out) {
                const size_t o = (size_t)(y - g.out_row0) * g.nx + col0;
#pragma unroll
                for (int q = 0; q < GC / 4; ++q) {
                    float val[4][4];
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = 4 * q + tt;
                        const int ox = col0 + t;
                        const float qm = t == 0 ? left : mid[t == 0 ? 0 : t - 1];
                        const float qp = t == GC - 1 ? right : mid[t == GC - 1 ? GC - 1 : t + 1];
                        // numpy.gradient: central difference / 2 inside, one-sided at the edges
                        float dx, dy;
                        if (ox == 0) dx = qp - mid[t];
                        else if (ox == g.nx - 1) dx = mid[t] - qm;
                        else dx = (qp - qm) * 0.5f;
                        if (y == 0) dy = dn[t] - mid[t];
                        else if (y == g.gny - 1) dy = mid[t] - up[t];
                        else dy = (dn[t] - up[t]) * 0.5f;
                        float rx, ry;
                        resolution_at(g, y, min(ox, g.nx - 1), rx, ry);
                        gradient_values(dx, dy, rx, ry, val[2][tt], val[3][tt]);
                        val[0][tt] = dx;
                        val[1][tt] = dy;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (!planes[k]) continue;
                        if (vec_ok) {
                            *reinterpret_cast<float4*>(planes[k] + o + 4 * q) =
                                make_float4(val[k][0], val[k][1], val[k][2], val[k][3]);
                        } else {
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt)
                                if (col0 + 4 * q + tt < g.nx) planes[k][o + 4 * q + tt] = val[k][tt];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < GC; ++t) {
            up[t] = mid[t];
            mid[t] = dn[t];
        }
    }
}

// ---- host side -----------------------------------------------------------------------------
template <int KB, int PF>
int launch_axis1_grad_pf(const GaussArgs& a, const GradArgs& g, size_t lds) {
    constexpr int TB = 16, NW = 8;
    Context& c = ctx();
    constexpr int tc = NW * TB;
    const void* kernel = (const void*)gauss_axis1_grad_kernel<TB, KB, NW, PF>;
    TOPO_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = 0;
    TOPO_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, NW * 64, lds));
    if (per_cu < 1) per_cu = 1;
    constexpr int out_r = 62, out_c = tc - 2;
    const int tiles_y = (g.out_row0 + g.out_rows - 1) / out_r - g.out_row0 / out_r + 1;
    const int tiles_x = (g.nx + out_c - 1) / out_c;
    const long ntiles = (long)tiles_x * tiles_y;
    long grid = (long)(c.num_cu - c.reserve_cus) * per_cu;  // persistent: every block walks the tile list
    if (grid > ntiles) grid = ntiles;
    if (grid < 1) grid = 1;
    TOPO_TRY(launch(gauss_axis1_grad_kernel<TB, KB, NW, PF>, dim3((unsigned)grid), dim3(NW * 64), lds, c.compute, a, g, tiles_x, (int)ntiles));
    t_grad.finish = kGradFinishTiled;
    t_grad.kb = KB;
    t_grad.pf = PF;
    return TOPO_AMD_OK;
}

template <int KB>
int launch_axis1_grad(const GaussArgs& a, const GradArgs& g, double sigma) {
    const int cols_l = axis1_tile_cols(16, KB, 8, a.nchunks);
    const size_t lds = axis1_tile_lds(16, 8, cols_l);
    const auto outside = [&]() -> int {
        set_error("gradient: sigma %.3f (radius %d) needs %zu B of LDS and %d columns per tile; "
                  "outside what the LDS-tiled axis-1 kernel is built for", sigma, a.radius, lds, cols_l);
        return TOPO_AMD_EUNSUP;
    };
    if (lds > kLdsMax || cols_l > kGradTileMaxCols) return outside();
    const auto with_pf = [&](auto PF) -> int {
        if constexpr (axis1_grad_built(KB, PF())) return launch_axis1_grad_pf<KB, PF()>(a, g, lds);
        else return outside();
    };
    const int pf = grad_tile_pf(cols_l);
    return pf == 5 ? with_pf(Int<5>{}) : pf == 4 ? with_pf(Int<4>{}) : with_pf(Int<3>{});
}

// axis-1 smoothing of the plane `in` (rows [s_row0, s_row0 + s_rows) of the DEM, already
// smoothed along axis 0) fused with the gradient epilogue described by g.
int run_axis1_grad(const float* in, int s_row0, int s_rows, int gny, int nx, double sigma, const GradArgs& g, int table_slot) {
    const int kb = grad_tile_kb(gaussian_radius(sigma));
    GaussArgs a;
    TOPO_TRY(gauss_args(Block{in, s_rows, s_row0, gny, nx, 0, 0}, nullptr, sigma, kb, table_slot, &a));
    return kb == 16 ? launch_axis1_grad<16>(a, g, sigma) : launch_axis1_grad<8>(a, g, sigma);
}

}  // namespace

int run_axis1_wave_grad(const float* in, int s_row0, int s_rows, double sigma, const GradArgs& g, float* smooth_out) {
    Context& c = ctx();
    const int R = gaussian_radius(sigma);
    const int d_hi = wave_lane_reach(R), d_lo = -d_hi;
    const int nsteps = d_hi - d_lo + 1;
    const int nvl = wave_out_lanes(R);  // lanes of a wavefront that produce output
    if (nvl < kWaveMinLanes) return TOPO_AMD_EUNSUP;
    std::vector<double> w;
    const double sum = gauss_taps(sigma, &w);
    // chain step `step` handles lane offset D = d_hi - step: output sub-column t of lane L takes
    // sample s of lane L + D with tap index GC*D + s - t + R
    std::vector<float> wtab((size_t)nsteps * 32, 0.0f), wsum((size_t)nsteps * GC, 0.0f);
    for (int step = 0; step < nsteps; ++step) {
        const int D = d_hi - step;
        for (int j = 0; j <= 30; ++j) {
            const int k = GC * D + (j - 15) + R;
            if (k >= 0 && k <= 2 * R) wtab[(size_t)step * 32 + j] = (float)(w[k] / sum);
        }
    }
    // wsum[D][t] = taps lane L+D contributes to sub-column t in total; the chain consumes them
    // cumulated: sum_D wsum[D] (v0[L+D] - v0[L]) = sum_{j>=1} eps[L+j] T+[j] - sum_{j<=0} eps[L+j] T-[j],
    // eps[m] = v0[m] - v0[m-1], T+[j] = sum_{D>=j} wsum[D], T-[j] = sum_{D<=j-1} wsum[D]
    for (int t = 0; t < GC; ++t) {
        std::vector<double> ws(nsteps);
        for (int step = 0; step < nsteps; ++step) {
            double acc = 0.0;
            for (int sidx = 0; sidx < GC; ++sidx) acc += (double)wtab[(size_t)step * 32 + sidx - t + 15];
            ws[step] = acc;
        }
        for (int step = 0; step < nsteps; ++step) {
            const int j = d_hi - step;
            double acc = 0.0;
            if (j >= 1) {
                for (int D = j; D <= d_hi; ++D) acc += ws[d_hi - D];
            } else {
                for (int D = d_lo; D <= j - 1; ++D) acc -= ws[d_hi - D];
            }
            wsum[(size_t)step * GC + t] = (float)acc;
        }
    }
    void *d_w = nullptr, *d_s = nullptr;
    TOPO_TRY(upload_table(2, wtab.data(), wtab.size() * sizeof(float), &d_w));
    TOPO_TRY(upload_table(3, wsum.data(), wsum.size() * sizeof(float), &d_s));
    WaveGradArgs a;
    a.in = in;
    a.in_row0 = s_row0;
    a.in_rows = s_rows;
    a.wtab = (const float*)d_w;
    a.wsum = (const float*)d_s;
    a.radius = R;
    a.d_lo = d_lo;
    a.nsteps = nsteps;
    a.nvl = nvl;
    a.out_c = GC * (nvl - 2);
    a.rows_per_wave = 32;
    a.smooth_out = smooth_out;
    a.g = g;
    const int tiles = (g.out_row0 + g.out_rows - 1) / a.rows_per_wave - g.out_row0 / a.rows_per_wave + 1;
    dim3 grid((g.nx + a.out_c - 1) / a.out_c, (tiles + kThreads / 64 - 1) / (kThreads / 64));
    TOPO_TRY(launch(gauss_axis1_wave_grad_kernel, grid, dim3(kThreads), 0, c.compute, a));
    if (!smooth_out) t_grad.finish = kGradFinishWave;  // (with a plane to write it is the smooth of run_axis1, no finish)
    return TOPO_AMD_OK;
}

int gradient_ghost_rows(double sigma, double sig_ratio, bool least) {
    if (sigma <= 1.0) return 1;
    if (sig_ratio != 0.0 && sig_ratio != 1.0) return gaussian_radius(std::max(sigma, sigma * sig_ratio)) + 1;
    return (least ? gaussian_radius(sigma) : gauss_ghost_rows(sigma)) + 1;
}

int launch_sobel(const Block& b, float* dx_out, float* dy_out) {
    return for_row_slabs(b.out_rows, [&](int r, int n) -> int {
        GradArgs g{};
        g.raw = b.in;
        g.raw_rows = b.in_rows;
        g.raw_row0 = b.in_row0;
        g.gny = b.gny;
        g.nx = b.nx;
        g.out_row0 = b.out_row0 + r;
        g.out_rows = n;
        g.dx = dx_out ? dx_out + (size_t)r * b.nx : nullptr;
        g.dy = dy_out ? dy_out + (size_t)r * b.nx : nullptr;
        TOPO_TRY(check_grid_rows(n, "sobel / gradient epilogue"));
        return launch(sobel_kernel<false>, dim3((b.nx + kThreads - 1) / kThreads, n), dim3(kThreads), 0, ctx().compute, g);
    });
}

namespace {
int upload_resolution(int res_mode, const void* res_x, const void* res_y, int nx, int gny, const float** dx, const float** dy) {
    if (res_mode == TOPO_AMD_RES_2D) {
        *dx = (const float*)res_x;
        *dy = (const float*)res_y;
        return TOPO_AMD_OK;
    }
    const int n_x = res_mode == TOPO_AMD_RES_SCALAR ? 1 : nx;
    const int n_y = res_mode == TOPO_AMD_RES_SCALAR ? 1 : gny;
    std::vector<float> fx(n_x), fy(n_y);
    const double* hx = (const double*)res_x;
    const double* hy = (const double*)res_y;
    for (int i = 0; i < n_x; ++i) fx[i] = (float)hx[i];
    for (int i = 0; i < n_y; ++i) fy[i] = (float)hy[i];
    void *d0 = nullptr, *d1 = nullptr;
    TOPO_TRY(upload_table(4, fx.data(), fx.size() * sizeof(float), &d0));
    TOPO_TRY(upload_table(5, fy.data(), fy.size() * sizeof(float), &d1));
    *dx = (const float*)d0;
    *dy = (const float*)d1;
    return TOPO_AMD_OK;
}

// the rows the gradient smooths: the output rows plus one neighbour row inside the DEM
Block smoothed_rows_block(const Block& b) {
    Block r = b;
    r.out_row0 = b.out_row0 > 0 ? b.out_row0 - 1 : 0;
    const int s1 = (b.out_row0 + b.out_rows + 1 < b.gny) ? b.out_row0 + b.out_rows + 1 : b.gny;
    r.out_rows = s1 - r.out_row0;
    return r;
}

// the stand-alone epilogue, `rows` grid rows from g.out_row0 on `stream`: four pixels a thread on rows of 8 columns or more,
// one below; run_if != nullptr: the kernels that return at once unless *run_if != 0 (and stride over g's rows)
int launch_epilogue(GradArgs g, int rows, hipStream_t stream, const int* run_if = nullptr) {
    g.run_if = run_if;
    const bool wide = g.nx >= 8;
    const dim3 grid(((wide ? (g.nx + 3) / 4 : g.nx) + kThreads - 1) / kThreads, rows);
    const auto kernel = wide ? (run_if ? gradient_epilogue4_if_kernel : gradient_epilogue4_kernel)
                             : (run_if ? gradient_epilogue_if_kernel : gradient_epilogue_kernel);
    TOPO_TRY(launch(kernel, grid, dim3(kThreads), 0, stream, g));
    t_grad.epilogue = wide ? 2 : 1;
    t_grad.rerun = t_grad.rerun || run_if != nullptr;
    return TOPO_AMD_OK;
}

// Sobel: sigma <= 1 (topo.py:628-629).  One sigma (topo.py:630-631) on the matrix cores: chunked from
// TOPO_AMD_GRAD_CHUNK_MIN_ROWS output rows, else in one shot; elsewhere the vector-ALU kernels with axis 1 and the
// epilogue fused.  Two sigmas (topo.py:633-635): two smooths.
enum class GradRoute { Sobel, Chunked, Mfma, Valu, Aniso };
// the code of include/topo_amd.h (topo_amd_gradient_route) for what t_grad holds
int gradient_route_code(GradRoute route) {
    const GradNote& n = t_grad;
    const bool mfma = n.tile_steps || n.s1_steps;
    const int smooth = n.fused_steps ? 1 : n.s1_steps ? 3 : n.tile_steps ? 2 : n.valu_smooth ? 4 : 0;
    const int steps = n.fused_steps ? n.fused_steps : n.s1_steps ? n.s1_steps : n.tile_steps;
    return (int)route | smooth << 3 | (n.valu_smooth && mfma ? 1 << 6 : 0) | steps << 7 | n.finish << 12 | (n.kb == 16 ? 1 << 14 : 0) |
           n.pf << 15 | n.epilogue << 18 | (n.rerun ? 1 << 20 : 0) | (n.taper ? 1 << 21 : 0) | n.chunks << 22;
}
GradRoute gradient_route(const Block& b, double sigma, double sig_ratio, int mfma_from) {
    // (2048: the interior of a 4096-row shard of the 8-GPU split goes in two chunks)
    static const int chunk_min = env_int("TOPO_AMD_GRAD_CHUNK_MIN_ROWS", 2048);
    if (sigma <= 1.0) return GradRoute::Sobel;
    if (sig_ratio != 1.0) return GradRoute::Aniso;
    const int R = gaussian_radius(sigma);
    if (!mfma_radius(R, b.nx, mfma_from) || !mfma_rows_ok(smoothed_rows_block(b), R)) return GradRoute::Valu;
    return b.out_rows >= chunk_min ? GradRoute::Chunked : GradRoute::Mfma;
}

// The chunked matrix-core route: the smooth is MFMA-bound and leaves HBM idle, the epilogue is HBM-bound and needs no
// LDS, so the rows go in chunks and the epilogue of chunk k runs on a second stream next to the smooth of chunk k + 1
// (15.7 -> 14.5 ms at sigma 30.25 on 32768^2 with 4 -> 8 chunks; one chunk: 18.5).  Row chunks are row blocks: same bits.
int gradient_chunked(const Block& b, double sigma, const GradArgs& g) {
    Context& c = ctx();
    static const int NCH = std::max(1, std::min(64, env_int("TOPO_AMD_GRAD_CHUNKS", 8)));
    // smallest chunk (rows); a chunk's planes should fit the 256 MB Infinity Cache
    // 32768^2, chunks x rows (profiles/r03_gradient_chunks.txt): 8 x 4096 8.04 / 13.70 ms at sigma 3.25 / 30.25,
    // 16 x 2048 7.77 / 13.50, 32 x 1024 8.27 / 14.55, 64 x 512 8.54 / 16.16
    // with the f16 kernels (profiles/r03_gauss_f16.txt, section 7): 4 x 8192 6.15 / 9.01, 8 x 4096 6.08 / 9.12,
    // 12 x 2752 6.31 / 9.40, 16 x 2048 6.31 / 9.59, 32 x 1024 6.64 / 11.20; one stream: 6.71 / 10.43
    static const int chunk_rows = std::max(256, env_int("TOPO_AMD_GRAD_CHUNK_ROWS", 4096));
    const int R = gaussian_radius(sigma);
    const bool gated = c.ghost.armed;
    // A short block (a row shard: 4096 rows) in few chunks leaves the smooth of its first chunk and the epilogue of its
    // last one uncovered: the fused route (one kernel per chunk, nothing restaged across a cut but Rp rows) goes in at
    // least 6 chunks of 512 rows or more, the two-pass route (every chunk restages 2 R rows on axis 0: 24 % at
    // radius 121 and 1024 rows) in at least 3.  One 4096-row shard in loop-back, sigma 3.25 / 30.25, ms per step
    // (profiles/r04_shard_fused.txt): 2 chunks 0.98 / 1.56, 3: 0.95 / 1.55, 4: 0.83 / 1.60, 6: 0.81 / 1.73, 8: 0.85 / 1.91.
    const int min_chunks = std::max(2, std::min(fused_radius(R, true, fused_on()) ? 6 : 3, b.out_rows / 512));
    if (!c.aux) {
        TOPO_HIP(hipStreamCreateWithFlags(&c.aux, hipStreamNonBlocking));
        for (auto& e : c.aux_ready) TOPO_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        TOPO_HIP(hipEventCreateWithFlags(&c.aux_done, hipEventDisableTiming));
    }
    // smoothed rows [s0, s1), cut at global multiples of 32 rows (the row tiles of the axis-0 kernel; a chunk of 32 k
    // rows is also a whole number of axis-1 bands).  Behind the smooth of a chunk, the epilogue emits the output rows
    // whose two neighbour rows are smoothed by then: the chunk's own rows, short of the first / last one where the chunk
    // next to it is still to come, plus the row that chunk left behind where it is done.
    const Block sb = smoothed_rows_block(b);
    const int s0 = sb.out_row0, s1 = sb.out_row0 + sb.out_rows;
    const int out_end = b.out_row0 + b.out_rows;
    const size_t bytes = (size_t)(s1 - s0) * b.nx * sizeof(float);
    void *pa = nullptr, *pb = nullptr;
    TOPO_TRY(workspace(1, bytes, &pa));
    TOPO_TRY(workspace(2, bytes, &pb));
    // chunks of >= 2048 rows (every chunk restages the 2 R halo rows of the axis-0 ring: 12 % at radius 121); a
    // short block (a row shard) goes in at least min_chunks, because the epilogue of its LAST chunk runs alone
    const int nch = std::max(min_chunks, std::min(NCH, (s1 - s0) / chunk_rows));
    const int per = std::max(32, ((s1 - s0 + nch - 1) / nch + 31) / 32 * 32);
    struct Chunk {
        int c0, c1;
        bool ghost, done;
    };
    std::vector<Chunk> chunks;
    // Taper (from 4 chunks): the smooth of the chunk processed FIRST and the epilogue of the one processed LAST run
    // uncovered, so those two chunks are a quarter of the others (>= 256 rows).  Processing order = row order, except in
    // a row shard, where the first chunk processed is the second in row order (the top one waits for the exchange).
    // (32768^2, sigma 3.25: 5.76 -> 5.52 ms; a 4096-row shard in 6 chunks LOSES 7 % with a 256-row first chunk, so only
    // blocks whose chunks are 2048 rows and more are tapered; sigma 30.25: no difference either way)
    const bool taper = nch >= 4 && (s1 - s0) / nch >= 2048;
    const int small = std::max(256, ((s1 - s0) / nch / 4 + 31) / 32 * 32);
    const int big = taper ? std::max(32, ((s1 - s0 - 2 * small + nch - 3) / (nch - 2) + 31) / 32 * 32) : per;
    const int first_small = gated ? 1 : 0;  // row-order index of the chunk processed first
    for (int c0 = s0, k = 0; c0 < s1; ++k) {
        const int want = taper && k == first_small ? small : big;
        int c1 = (c0 + want) / 32 * 32;
        if (taper && s1 - c1 < small + 32 && s1 - c1 > 0 && c1 < s1) c1 = std::max(c0 + 32, (s1 - small) / 32 * 32);  // leave the small last chunk
        if (c1 + 32 > s1 || c1 <= c0) c1 = s1;  // no sliver at the end
        // row shard with its exchange in flight: does the filter of these rows reach into the ghost rows?
        chunks.push_back({c0, c1, gated && (c0 - R < c.ghost.ghost_lo || c1 + R > c.ghost.ghost_hi), false});
        c0 = c1;
    }
    TOPO_REQUIRE(chunks.size() <= 64, "gradient: %zu row chunks (at most 64)", chunks.size());
    t_grad.chunks = (int)chunks.size();
    t_grad.taper = taper;
    // Row shard: the chunks that stay clear of the ghost rows go first, on the rows the shard owns (the ghost rows are
    // being written meanwhile; staging clamps to the view), then the compute stream waits for the exchange and the
    // chunks at the two seams follow on the whole block - ordinary chunks of the ordinary pipeline, no seam strips
    // of their own, and the exchange hides behind the first chunks.  Row chunks are row blocks: same bits.
    std::vector<int> order;
    for (int pass = 0; pass < 2; ++pass)
        for (int k = 0; k < (int)chunks.size(); ++k)
            if (chunks[k].ghost == (pass == 1)) order.push_back(k);
    Block owned = b;
    if (gated) {
        const int lo = std::max(b.in_row0, c.ghost.ghost_lo), hi = std::min(b.in_row0 + b.in_rows, c.ghost.ghost_hi);
        owned.in = b.in + (size_t)(lo - b.in_row0) * b.nx;
        owned.in_row0 = lo;
        owned.in_rows = hi - lo;
        c.ghost.armed = false;  // taken
    }
    // one "met a sample that is not a plain finite one" flag for the call: the fused kernels of all chunks raise it, and
    // the two-pass route (five launches that return at once on an ordinary DEM) is queued ONCE, behind the last
    // chunk, over all rows - not behind every chunk, where its launches sat in front of the next chunk's smooth
    void* wild = nullptr;
    TOPO_TRY(workspace(11, 64, &wild));
    TOPO_HIP(hipMemsetAsync(wild, 0, sizeof(int), c.compute));
    GradArgs sg = g;  // the epilogue over the smoothed plane
    sg.gx_src = sg.gy_src = (const float*)pb;
    sg.s_row0 = s0;
    sg.s_rows = s1 - s0;
    bool owed = false;
    bool waited = !gated;
    for (int k : order) {
        Chunk& ck = chunks[k];
        if (ck.ghost && !waited) {
            TOPO_TRY(topo_amd_halo_wait());
            waited = true;
        }
        Block rows = ck.ghost || !gated ? b : owned;
        rows.out_row0 = ck.c0;
        rows.out_rows = ck.c1 - ck.c0;
        float* a_k = (float*)pa + (size_t)(ck.c0 - s0) * b.nx;
        float* b_k = (float*)pb + (size_t)(ck.c0 - s0) * b.nx;
        bool owes = false;
        TOPO_TRY(smooth_both_mfma(rows, sigma, a_k, b_k, 1, true, (const int*)wild, &owes));
        owed = owed || owes;
        ck.done = true;
        TOPO_HIP(hipEventRecord(c.aux_ready[k], c.compute));
        TOPO_HIP(hipStreamWaitEvent(c.aux, c.aux_ready[k], 0));
        const bool first = k == 0, last = k + 1 == (int)chunks.size();
        const int o0 = std::max(b.out_row0, first ? b.out_row0 : (chunks[k - 1].done ? ck.c0 - 1 : ck.c0 + 1));
        const int o1 = std::min(out_end, last ? out_end : (chunks[k + 1].done ? ck.c1 + 1 : ck.c1 - 1));
        if (o1 > o0) {
            GradArgs gk = sg;
            const size_t shift = (size_t)(o0 - b.out_row0) * b.nx;
            gk.out_row0 = o0;
            gk.out_rows = o1 - o0;
            gk.dx = g.dx ? g.dx + shift : nullptr;
            gk.dy = g.dy ? g.dy + shift : nullptr;
            gk.slope = g.slope ? g.slope + shift : nullptr;
            gk.aspect = g.aspect ? g.aspect + shift : nullptr;
            if (g.res_mode == TOPO_AMD_RES_2D) {
                gk.res_x = g.res_x + shift;
                gk.res_y = g.res_y + shift;
            }
            TOPO_TRY(launch_epilogue(gk, o1 - o0, c.aux));
        }
    }
    if (!waited) TOPO_TRY(topo_amd_halo_wait());
    TOPO_HIP(hipEventRecord(c.aux_done, c.aux));
    TOPO_HIP(hipStreamWaitEvent(c.compute, c.aux_done, 0));
    if (!owed) return TOPO_AMD_OK;
    // behind every chunk and its epilogue: smooth [s0, s1) again by the two passes and redo the epilogue, if the flag is up
    TOPO_TRY(smooth_two_pass(sb, sigma, (float*)pa, (float*)pb, 1, {(const int*)wild, true}));
    return launch_epilogue(sg, std::min(b.out_rows, 512), c.compute, (const int*)wild);
}

// the gradient of a block no taller than a launch covers
int gradient_slab(const Block& b, double sigma, double sig_ratio, int res_mode, const void* res_x, const void* res_y, float* dx,
                  float* dy, float* slope, float* aspect) {
    Context& c = ctx();
    TOPO_REQUIRE(res_mode >= 0 && res_mode <= 2, "gradient: bad res_mode %d", res_mode);
    TOPO_REQUIRE(res_x && res_y, "gradient: resolution arrays are NULL");
    const bool large = large_sample_call();
    const GradRoute route = gradient_route(b, sigma, sig_ratio, mfma_from(large, true));
    t_grad = GradNote{};  // (the Gaussian's launchers write it too: it means something only from here to noter.done)
    // noted only when every launch of the call succeeded
    struct Noter {
        GradRoute route;
        int done(int r) {
            if (r == TOPO_AMD_OK) note_gradient_route(gradient_route_code(route));
            return r;
        }
    } noter{route};
    // a row shard whose exchange is in flight (common.hpp, GhostGate): only the chunked route knows what to do with it;
    // every other route says so before it launches anything
    if (c.ghost.armed && route != GradRoute::Chunked) return TOPO_AMD_EUNSUP;
    GradArgs g{};
    TOPO_TRY(upload_resolution(res_mode, res_x, res_y, b.nx, b.gny, &g.res_x, &g.res_y));
    g.res_mode = res_mode;
    g.gny = b.gny;
    g.nx = b.nx;
    g.out_row0 = b.out_row0;
    g.out_rows = b.out_rows;
    g.dx = dx;
    g.dy = dy;
    g.slope = slope;
    g.aspect = aspect;
    TOPO_TRY(check_grid_rows(b.out_rows, "sobel / gradient epilogue"));
    if (route == GradRoute::Sobel) {
        g.raw = b.in;
        g.raw_rows = b.in_rows;
        g.raw_row0 = b.in_row0;
        return noter.done(launch(sobel_kernel<true>, dim3((b.nx + kThreads - 1) / kThreads, b.out_rows), dim3(kThreads), 0, c.compute, g));
    }
    TOPO_REQUIRE(b.gny >= 2 && b.nx >= 2, "gradient: numpy.gradient needs at least 2 samples per axis (got %d x %d)", b.gny, b.nx);
    if (route == GradRoute::Chunked) return noter.done(gradient_chunked(b, sigma, g));
    const Block s = smoothed_rows_block(b);
    const size_t bytes = (size_t)s.out_rows * b.nx * sizeof(float);
    void *plane_a = nullptr, *plane_b = nullptr;
    TOPO_TRY(workspace(1, bytes, &plane_a));
    if (route == GradRoute::Valu) {
        TOPO_TRY(run_axis0(s, sigma, (float*)plane_a, 1, kNoMfma));
        // short and medium filters: LDS-tiled axis 1 (9.8 vs 13.6 ms at sigma 3.25 on 32768^2); long
        // filters: wave-shift axis 1 (26.7 vs 27.8 ms at sigma 30.25) while enough lanes produce output
        if (gaussian_radius(sigma) <= kGradTiledMaxRadius) {
            const int r = run_axis1_grad((const float*)plane_a, s.out_row0, s.out_rows, b.gny, b.nx, sigma, g, 2);
            if (r != TOPO_AMD_EUNSUP) return noter.done(r);
        }
        const int r = run_axis1_wave_grad((const float*)plane_a, s.out_row0, s.out_rows, sigma, g, nullptr);
        if (r != TOPO_AMD_EUNSUP) return noter.done(r);
        // a filter wider than a wavefront can chain: finish the smooth unfused (beyond radius 121 axis 1 goes through
        // the wave-shift or the transpose path)
        TOPO_TRY(workspace(2, bytes, &plane_b));
        TOPO_TRY(run_axis1((const float*)plane_a, s.out_rows, b.nx, sigma, (float*)plane_b, 2, mfma_from(large, true)));
        t_grad.finish = kGradFinishUnfused;
        plane_a = plane_b;
    } else if (route == GradRoute::Mfma) {  // the smooth of the chunked route (same kernels, same bits)
        TOPO_TRY(workspace(2, bytes, &plane_b));
        TOPO_TRY(smooth_both_mfma(s, sigma, (float*)plane_a, (float*)plane_b, 1, true));
        plane_a = plane_b;
    } else {
        const double perp = sigma * sig_ratio;
        TOPO_TRY(workspace(2, bytes, &plane_b));
        // (two radii, one ghost depth: the matrix-core kernels only from radius 16, where they need no more
        // ghost rows than the filter itself)
        TOPO_TRY(smooth_rows(b, perp, sigma, s.out_row0, s.out_rows, (float*)plane_a, mfma_from(large, false)));
        TOPO_TRY(smooth_rows(b, sigma, perp, s.out_row0, s.out_rows, (float*)plane_b, mfma_from(large, false)));
    }
    g.gx_src = (const float*)plane_a;
    g.gy_src = (const float*)plane_b;
    g.s_row0 = s.out_row0;
    g.s_rows = s.out_rows;
    return noter.done(launch_epilogue(g, b.out_rows, c.compute));
}
// ---- K4v: the valid-sample gradient (topo.gradient(skipna=True), include/topo_amd.h: topo_amd_gradient_valid_dev) --------
// sigma > 1: an epilogue over one or two planes q of the valid-sample Gaussian taken with fill (gauss_valid.hip), in which NaN
// says "q is not defined here".  Along an axis the derivative at a pixel whose q is defined is the central difference / 2 where
// both neighbours exist and are defined, the one-sided first-order difference where one of them does, NaN where neither does;
// a raster edge is a neighbour that does not exist, so on a gap-free raster this is numpy.gradient.  sigma <= 1: the Sobel pair
// where all six samples under the non-zero taps of a derivative are valid.  Both: NaN in every plane at a pixel whose own
// sample is missing unless `fill`; then gradient_values, the arithmetic of every other route.
struct ValidGradArgs {
    GradArgs g;  // raw: the block itself (the epilogue reads it only when fill == 0); gx_src / gy_src: the q planes
    int fill;
};

// selects only: the three cases are picked by v_cndmask on q == q, no lane takes a path of its own
__device__ __forceinline__ float valid_difference(float qm, float q0, float qp) {
    // (& and |, not && and ||: a short-circuit becomes an exec-masked region)
    const bool hm = qm == qm, hp = qp == qp, h0 = q0 == q0;
    const float d = ((hp ? qp : q0) - (hm ? qm : q0)) * ((hm & hp) ? 0.5f : 1.0f);
    return (h0 & (hm | hp)) ? d : NAN;
}

// gradient_values behind the rule for a pixel's own sample; slope and aspect are NaN where dx or dy is
__device__ __forceinline__ void valid_gradient_values(float& dx, float& dy, bool keep, float rx, float ry, float& slope, float& aspect) {
    const bool has_dx = keep & (dx == dx), has_dy = keep & (dy == dy);
    gradient_values(dx, dy, rx, ry, slope, aspect);
    dx = has_dx ? dx : NAN;  // (one NaN, whatever the arithmetic made of its operand)
    dy = has_dy ? dy : NAN;
    slope = (has_dx & has_dy) ? slope : NAN;
    aspect = (has_dx & has_dy) ? aspect : NAN;
}

__device__ __forceinline__ void valid_epilogue_pixel(const ValidGradArgs& a, int oy, int ox) {
    const GradArgs& p = a.g;
    const float* rowx = p.gx_src + (size_t)(oy - p.s_row0) * p.nx;
    const float xm = rowx[max(ox - 1, 0)], xp = rowx[min(ox + 1, p.nx - 1)];  // (clamped loads, the edge is a select)
    float dx = valid_difference(ox > 0 ? xm : NAN, rowx[ox], ox < p.nx - 1 ? xp : NAN);
    const float* coly = p.gy_src + (size_t)(oy - p.s_row0) * p.nx + ox;
    const float ym = coly[oy > 0 ? -p.nx : 0], yp = coly[oy < p.gny - 1 ? p.nx : 0];
    float dy = valid_difference(oy > 0 ? ym : NAN, coly[0], oy < p.gny - 1 ? yp : NAN);
    const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
    const float own = a.fill ? 0.0f : p.raw[(size_t)(oy - p.raw_row0) * p.nx + ox];
    float rx, ry, slope, aspect;
    resolution_at(p, oy, ox, rx, ry);
    valid_gradient_values(dx, dy, sample_valid(own), rx, ry, slope, aspect);
    if (p.dx) p.dx[o] = dx;
    if (p.dy) p.dy[o] = dy;
    if (p.slope) p.slope[o] = slope;
    if (p.aspect) p.aspect[o] = aspect;
}

// Built like gradient_epilogue4_kernel: four adjacent pixels a thread, 16-byte loads of the three q rows (and of the raw row
// when fill == 0: 24 instead of 20 B / pixel) and 16-byte streaming stores, which need dword alignment only - any width; the
// last 1 ... 3 pixels of a row (every pixel of a row under 4 columns) go one by one.
__global__ __launch_bounds__(kThreads) void gradient_valid_epilogue4_kernel(ValidGradArgs a) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const GradArgs& p = a.g;
    const int ox = (blockIdx.x * kThreads + threadIdx.x) * 4;
    const int oy = p.out_row0 + blockIdx.y;
    if (ox >= p.nx) return;
    if (ox + 4 > p.nx) {
        for (int x = ox; x < p.nx; ++x) valid_epilogue_pixel(a, oy, x);
        return;
    }
    const float* rowx = p.gx_src + (size_t)(oy - p.s_row0) * p.nx;
    const f4 mid = *reinterpret_cast<const f4*>(rowx + ox);
    const float left = rowx[max(ox - 1, 0)], right = rowx[min(ox + 4, p.nx - 1)];
    const float* coly = p.gy_src + (size_t)(oy - p.s_row0) * p.nx + ox;
    const bool has_up = oy > 0, has_dn = oy < p.gny - 1;  // (block-uniform)
    const f4 cen = *reinterpret_cast<const f4*>(coly);
    const f4 up = *reinterpret_cast<const f4*>(coly - (has_up ? p.nx : 0));
    const f4 dn = *reinterpret_cast<const f4*>(coly + (has_dn ? p.nx : 0));
    // the pixels' own samples; with fill nobody asks, and the load goes to the row just fetched instead of the raw plane (an
    // address chosen per block: a conditional load would put a wait for it in front of the arithmetic)
    const bool fill = a.fill != 0;
    const f4 own = *reinterpret_cast<const f4*>(fill ? coly : p.raw + (size_t)(oy - p.raw_row0) * p.nx + ox);
    f4 odx, ody, osl, oas;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int x = ox + t;
        const float xm = t == 0 ? (x > 0 ? left : NAN) : mid[t == 0 ? 0 : t - 1];
        const float xp = t == 3 ? (x < p.nx - 1 ? right : NAN) : mid[t == 3 ? 3 : t + 1];
        float dx = valid_difference(xm, mid[t], xp);
        float dy = valid_difference(has_up ? up[t] : NAN, cen[t], has_dn ? dn[t] : NAN);
        float rx, ry, slope, aspect;
        resolution_at(p, oy, x, rx, ry);
        valid_gradient_values(dx, dy, fill | sample_valid(own[t]), rx, ry, slope, aspect);
        odx[t] = dx;
        ody[t] = dy;
        osl[t] = slope;
        oas[t] = aspect;
    }
    const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
    if (p.dx) __builtin_nontemporal_store(odx, reinterpret_cast<f4*>(p.dx + o));
    if (p.dy) __builtin_nontemporal_store(ody, reinterpret_cast<f4*>(p.dy + o));
    if (p.slope) __builtin_nontemporal_store(osl, reinterpret_cast<f4*>(p.slope + o));
    if (p.aspect) __builtin_nontemporal_store(oas, reinterpret_cast<f4*>(p.aspect + o));
}

// sobel_kernel with a mask: a missing sample enters the sums as 0 and takes away the derivatives it has a tap in (the centre
// has a tap in neither).  On a raster without gaps: the bits of sobel_kernel<true>.
__global__ __launch_bounds__(kThreads) void sobel_valid_kernel(ValidGradArgs a) {
    const GradArgs& p = a.g;
    const int ox = blockIdx.x * kThreads + threadIdx.x;
    const int oy = p.out_row0 + blockIdx.y;
    if (ox >= p.nx) return;
    bool has_dx = true, has_dy = true;
    auto tap = [&](int gy, int gx, bool in_dx, bool in_dy) -> double {
        const double v = raw_reflect(p, gy, gx);
        const bool ok = fabs(v) < (double)kMissingLim;  // (the float32 sample, widened exactly)
        has_dx = has_dx && (ok || !in_dx);
        has_dy = has_dy && (ok || !in_dy);
        return ok ? v : 0.0;
    };
    const double nw = tap(oy - 1, ox - 1, true, true), n = tap(oy - 1, ox, false, true), ne = tap(oy - 1, ox + 1, true, true);
    const double w = tap(oy, ox - 1, true, false), e = tap(oy, ox + 1, true, false);
    const double sw = tap(oy + 1, ox - 1, true, true), s = tap(oy + 1, ox, false, true), se = tap(oy + 1, ox + 1, true, true);
    float dx = has_dx ? (float)(0.125 * (ne - nw) + 0.25 * (e - w) + 0.125 * (se - sw)) : NAN;
    float dy = has_dy ? (float)(0.125 * (sw - nw) + 0.25 * (s - n) + 0.125 * (se - ne)) : NAN;
    const size_t o = (size_t)(oy - p.out_row0) * p.nx + ox;
    const bool keep = a.fill || sample_valid(p.raw[(size_t)(oy - p.raw_row0) * p.nx + ox]);
    float rx, ry, slope, aspect;
    resolution_at(p, oy, ox, rx, ry);
    valid_gradient_values(dx, dy, keep, rx, ry, slope, aspect);
    if (p.dx) p.dx[o] = dx;
    if (p.dy) p.dy[o] = dy;
    if (p.slope) p.slope[o] = slope;
    if (p.aspect) p.aspect[o] = aspect;
}

// the valid-sample gradient of a block no taller than a launch covers
int gradient_valid_slab(const Block& b, double sigma, double sig_ratio, double min_weight, bool fill, int res_mode, const void* res_x,
                        const void* res_y, float* dx, float* dy, float* slope, float* aspect) {
    Context& c = ctx();
    ValidGradArgs a{};
    GradArgs& g = a.g;
    TOPO_TRY(upload_resolution(res_mode, res_x, res_y, b.nx, b.gny, &g.res_x, &g.res_y));
    g.res_mode = res_mode;
    g.raw = b.in;
    g.raw_rows = b.in_rows;
    g.raw_row0 = b.in_row0;
    g.gny = b.gny;
    g.nx = b.nx;
    g.out_row0 = b.out_row0;
    g.out_rows = b.out_rows;
    g.dx = dx;
    g.dy = dy;
    g.slope = slope;
    g.aspect = aspect;
    a.fill = fill ? 1 : 0;
    TOPO_TRY(check_grid_rows(b.out_rows, "valid-sample sobel / gradient epilogue"));
    if (sigma <= 1.0) return launch(sobel_valid_kernel, dim3((b.nx + kThreads - 1) / kThreads, b.out_rows), dim3(kThreads), 0, c.compute, a);
    // q over the output rows and one neighbour row inside the raster, where launch_gradient keeps its smoothed planes
    const Block s = smoothed_rows_block(b);
    const size_t bytes = (size_t)s.out_rows * b.nx * sizeof(float);
    void *plane_a = nullptr, *plane_b = nullptr;
    TOPO_TRY(workspace(1, bytes, &plane_a));
    if (sig_ratio == 1.0) {
        TOPO_TRY(launch_gaussian_valid(s, sigma, sigma, min_weight, true, (float*)plane_a, nullptr));
        plane_b = plane_a;
    } else {  // dx of the field smoothed with sigma * sig_ratio down the columns, dy of the one smoothed with it along the rows
        const double perp = sigma * sig_ratio;
        TOPO_TRY(workspace(2, bytes, &plane_b));
        TOPO_TRY(launch_gaussian_valid(s, perp, sigma, min_weight, true, (float*)plane_a, nullptr));
        TOPO_TRY(launch_gaussian_valid(s, sigma, perp, min_weight, true, (float*)plane_b, nullptr));
    }
    g.gx_src = (const float*)plane_a;
    g.gy_src = (const float*)plane_b;
    g.s_row0 = s.out_row0;
    g.s_rows = s.out_rows;
    const dim3 grid(((b.nx + 3) / 4 + kThreads - 1) / kThreads, b.out_rows);
    return launch(gradient_valid_epilogue4_kernel, grid, dim3(kThreads), 0, c.compute, a);
}
}  // namespace

int launch_gradient_valid(const Block& b, double sigma, double sig_ratio, double min_weight, bool fill, int res_mode, const void* res_x,
                          const void* res_y, float* dx, float* dy, float* slope, float* aspect) {
    TOPO_REQUIRE(res_mode >= 0 && res_mode <= 2, "gradient_valid: bad res_mode %d", res_mode);
    TOPO_REQUIRE(res_x && res_y, "gradient_valid: resolution arrays are NULL");
    if (sigma > 1.0) TOPO_REQUIRE(b.gny >= 2 && b.nx >= 2, "gradient_valid: a finite difference needs at least 2 samples per axis (got %d x %d)", b.gny, b.nx);
    if (ctx().ghost.armed) return TOPO_AMD_EUNSUP;  // (a row shard whose exchange is in flight: this call is not sharded)
    TOPO_TRY(for_row_slabs(b.out_rows, [&](int r, int n) -> int {
        Block s = b;
        s.out_row0 = b.out_row0 + r;
        s.out_rows = n;
        const size_t shift = (size_t)r * b.nx;
        const void *rx = res_x, *ry = res_y;
        if (res_mode == TOPO_AMD_RES_2D) {
            rx = (const float*)res_x + shift;
            ry = (const float*)res_y + shift;
        }
        return gradient_valid_slab(s, sigma, sig_ratio, min_weight, fill, res_mode, rx, ry, dx ? dx + shift : nullptr, dy ? dy + shift : nullptr,
                                   slope ? slope + shift : nullptr, aspect ? aspect + shift : nullptr);
    }));
    note_gradient_route(sigma > 1.0 && sig_ratio != 1.0 ? kGradRouteValidAniso : kGradRouteValid);
    return TOPO_AMD_OK;
}

int launch_gradient(const Block& b, double sigma, double sig_ratio, int res_mode, const void* res_x, const void* res_y, float* dx,
                    float* dy, float* slope, float* aspect) {
    if (b.out_rows > kMaxLaunchRows && ctx().ghost.armed) return TOPO_AMD_EUNSUP;
    return for_row_slabs(b.out_rows, [&](int r, int n) -> int {
        Block s = b;
        s.out_row0 = b.out_row0 + r;
        s.out_rows = n;
        const size_t shift = (size_t)r * b.nx;
        const void *rx = res_x, *ry = res_y;
        if (res_mode == TOPO_AMD_RES_2D && res_x && res_y) {
            rx = (const float*)res_x + shift;
            ry = (const float*)res_y + shift;
        }
        return gradient_slab(s, sigma, sig_ratio, res_mode, rx, ry, dx ? dx + shift : nullptr, dy ? dy + shift : nullptr,
                             slope ? slope + shift : nullptr, aspect ? aspect + shift : nullptr);
    });
}

}  // namespace topo
