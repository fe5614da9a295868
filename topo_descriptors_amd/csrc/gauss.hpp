// What the Gaussian / gradient units share (gauss.hip: vector-ALU kernels and the smooth of a row block; gauss_f16.hip:
// the f16 matrix-core kernels; gradient.hip: epilogue, Sobel, axis 1 fused with the epilogue): kernel argument blocks,
// the device helpers more than one unit uses, the route note, and the few host functions that cross units.
// The arithmetic that picks a kernel for a radius is gauss_route.hpp.
#pragma once

#include "common.hpp"
#include "gauss_route.hpp"

#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace topo {

constexpr int kThreads = 256;

__device__ __forceinline__ int reflect_index(int i, int n) {
    // scipy mode="reflect": (d c b a | a b c d | d c b a), period 2n
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

// The accumulation offset of a group of outputs is one of its own samples; a non-finite sample cannot serve
// (x - NaN is NaN for every x of the group).
__device__ __forceinline__ float finite_or_zero(float c) { return fabsf(c) <= 3.0e38f ? c : 0.0f; }

// the valid-sample units (gauss_valid.hip, the valid-sample gradient of gradient.hip): at or beyond 2^24 (or not finite) a
// sample is missing (disc_valid.hip)
constexpr float kMissingLim = 16777216.0f;
__device__ __forceinline__ bool sample_valid(float v) { return fabsf(v) < kMissingLim; }  // false for NaN / inf

struct GaussArgs {
    const float* in;
    float* out;
    const float* taps;  // 2R+1 taps followed by zeros up to a multiple of the tap chunk
    int in_rows, in_row0, gny, nx;
    int out_row0, out_rows;
    int radius, nchunks;
    int group0;  // axis 0: first row group (global numbering) that intersects the output rows
    unsigned char* flags;  // matrix-core kernels: one byte per 32 x 32 output tile, 1 = an output is not finite
    float tap_scale, out_scale;  // f16 matrix-core kernels: taps are multiplied by tap_scale (a power of two), sums by out_scale
    int* wild_flag;     // fused kernel: set to 1 when it stages a sample that is not a plain finite one
    uint32_t* wild_host;  // ... and this pinned host word of the DEM's memo entry (dem_memo_wild), or nullptr
    const int* run_if;  // two-pass f16 kernels behind a fused launch: return at once unless *run_if != 0 (nullptr: run)
    const float* wtab;  // split-once kernels: W[5][64], the taps an output lays over each slab of 64 (behind the plain taps)
    int fine_rows, fine_cols;  // split-once axis-1 kernel: flags is [fine_rows bands of 16 rows][fine_cols tiles of 32 columns] (0: one byte per 32 x 32 unit)
};

// Register tiling shared by both axes: a thread produces TB consecutive outputs along the
// filter axis, out[t] = sum_k w[k] in[t + k].  The taps are walked in chunks of KB; a chunk needs
// the TB + KB - 1 samples in[c KB ... c KB + TB + KB - 2], of which only KB are new, so per chunk
// the thread fetches KB samples (all in flight together, one chunk ahead of the FMAs) and issues
// TB x KB FMAs against KB wave-uniform taps (one scalar load per chunk).
// The padded zero taps of the last chunk are multiplied in like the others: skipping them (a second copy of
// the unrolled chunk body, bounded by the true tap count) was measured and costs 28 % of the gradient at
// sigma 3.25 (10.9 ms against 8.5 ms at 32768^2).  What it would buy: 0 x NaN = NaN, so a non-finite sample
// reaches up to KB - 1 outputs further along each axis (towards lower indices) than in ndimage.gaussian_filter;
// finite data is unaffected.  tests/test_gpu_parity.py::test_gaussian_nan_footprint pins that bound.
template <int TB, int KB, class Fetch>
__device__ __forceinline__ void tap_chunks(const float* taps, int nchunks, float c, Fetch fetch,
                                           float (&acc)[TB]) {
    float win[TB + KB - 1];
    float nxt[KB];
#pragma unroll
    for (int t = 0; t < TB; ++t) acc[t] = 0.0f;
#pragma unroll
    for (int i = 0; i < TB - 1; ++i) win[i] = fetch(i) - c;
#pragma unroll
    for (int i = 0; i < KB; ++i) nxt[i] = fetch(TB - 1 + i);
    for (int ch = 0; ch < nchunks; ++ch) {
#pragma unroll
        for (int i = 0; i < KB; ++i) win[TB - 1 + i] = nxt[i] - c;
        if (ch + 1 < nchunks) {
#pragma unroll
            for (int i = 0; i < KB; ++i) nxt[i] = fetch((ch + 1) * KB + TB - 1 + i);
        }
        const float* w = taps + ch * KB;  // wave-uniform
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            const float wk = w[kk];
#pragma unroll
            for (int t = 0; t < TB; ++t) acc[t] = fmaf(wk, win[t + kk], acc[t]);
        }
#pragma unroll
        for (int i = 0; i < TB - 1; ++i) win[i] = win[i + KB];
    }
}

// ---- gradient epilogue ---------------------------------------------------------------------
struct GradArgs {
    const float* gx_src;  // smoothed field differenced along x (rows start at s_row0)
    const float* gy_src;  // smoothed field differenced along y
    const float* raw;     // Sobel branch: the DEM block itself
    int raw_rows, raw_row0;
    int s_row0, s_rows;
    int gny, nx, out_row0, out_rows;
    int res_mode;
    const float* res_x;   // device: 1 value, nx values, or out_rows*nx values
    const float* res_y;   // device: 1 value, gny values, or out_rows*nx values
    float *dx, *dy, *slope, *aspect;
    const int* run_if;  // nullptr, or: return at once unless *run_if != 0 (the epilogue behind a deferred two-pass smooth)
};

// ---- host side ----
struct GradNote {  // what the launchers decided, for topo_amd_gradient_route (gradient.hip)
    int fused_steps = 0, tile_steps = 0, s1_steps = 0;  // step counts of the f16 kernels that were queued (0: none)
    bool valu_smooth = false;                            // a pass on the vector-ALU kernels
    int finish = 0, kb = 0, pf = 0;                      // axis-1 finish of the Valu route (kGradFinish*), its tap chunk and PF
    int epilogue = 0;                                    // stand-alone epilogue: 1 one pixel a thread, 2 four
    bool rerun = false;                                  // an _if epilogue behind a deferred two-pass smooth
    int chunks = 0;
    bool taper = false;
};
extern thread_local GradNote t_grad;  // (defined in gradient.hip)
constexpr int kGradFinishTiled = 1, kGradFinishWave = 2, kGradFinishUnfused = 3;
// the route codes of the valid-sample gradient (launch_gradient_valid: no other field), behind GradRoute's 0 ... 4
constexpr int kGradRouteValid = 5, kGradRouteValidAniso = 6;

// the environment's switches, read by their callers once: on unless the variable starts with '0'; a number, or `unset`
inline bool env_switch_on(const char* name) { const char* e = std::getenv(name); return !(e && *e == '0'); }
inline int env_int(const char* name, int unset) { const char* e = std::getenv(name); return e && *e ? std::atoi(e) : unset; }

// a plane of `rows` rows taken as a raster of its own
inline Block plane_block(const float* in, int rows, int nx) { return Block{in, rows, 0, rows, nx, 0, rows}; }
inline bool mfma_rows_ok(const Block& b, int R) { return mfma_rows_ok(b.in_row0, b.in_rows, b.gny, b.out_row0, b.out_rows, R); }

// f(first row of the slab, counted from the block's first output row; rows of the slab) over the output rows of a block:
// one slab unless the block is taller than a launch covers (kMaxLaunchRows, common.hpp)
template <class F>
int for_row_slabs(int out_rows, F f) {
    for (int r = 0; r < out_rows; r += kMaxLaunchRows) TOPO_TRY(f(r, std::min(kMaxLaunchRows, out_rows - r)));
    return TOPO_AMD_OK;
}

template <int N> using Int = std::integral_constant<int, N>;  // a template argument chosen at run time, handed to a generic lambda

// a kernel launch and its check
template <class K, class... Args>
int launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}
// the launch of a kernel that asks for more dynamic LDS than a block gets by default, on the compute stream: the
// attribute is set once per kernel (the template is keyed on the kernel, so is the static)
template <auto Kernel, class... Args>
int launch_big_lds(dim3 grid, dim3 block, size_t lds, Args... args) {
    static bool ready = false;
    if (!ready) {
        TOPO_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
        ready = true;
    }
    return launch(Kernel, grid, block, lds, ctx().compute, args...);
}

// ---- gauss.hip ----
// the float64 taps exp(-k^2 / 2 sigma^2), k = -R ... R (R = gaussian_radius(sigma)), into *w if given; returns their sum
double gauss_taps(double sigma, std::vector<double>* w = nullptr);
// the arguments of a pass over block b into `out`, with the taps of sigma in table slot `slot` (chunks of kb taps; kb == 1:
// the plain taps and the slab table)
int gauss_args(const Block& b, float* out, double sigma, int kb, int slot, GaussArgs* a);
int mfma_min_radius();     // TOPO_AMD_GAUSS_MFMA_MIN_RADIUS
bool large_sample_call();  // the raster of the call is a large-sample one (TOPO_AMD_GAUSS_LARGE_SAMPLE=0: never)
inline int mfma_from(bool large, bool small_ok) { return mfma_from(large, small_ok, mfma_min_radius()); }
int run_axis0(const Block& b, double sigma, float* out, int table_slot, int mfma_from);
// `in` holds exactly the rows [out_row0, out_row0 + out_rows) starting at in_row0 == out_row0
int run_axis1(const float* in, int rows, int nx, double sigma, float* out, int table_slot, int mfma_from);
// Full 2-D smooth of rows [row0, row0+rows) into `out`: scratch plane in workspace 0, taps in table slots 1 and 2
int smooth_rows(const Block& src, double sigma_y, double sigma_x, int row0, int rows, float* out, int mfma_from);

// ---- gauss_f16.hip ----
// The two passes queued behind (or instead of) a fused launch: they run only if *run_if != 0 (nullptr: always), and with
// one_tile axis 0 keeps the fused kernel's 32-row tiles, so that they give its bits.
struct TwoPass { const int* run_if = nullptr; bool one_tile = false; };
bool fused_on();  // TOPO_AMD_GAUSS_FUSED
// axis 0 on the f16 route: tiles of 32 MT rows on the global grid, one flag byte per 32 x 32 unit
int run_axis0_mfma(const Block& b, double sigma, float* out, int table_slot, const TwoPass& tp = {});
// axis 1 on the f16 route: `in` is a plane of `rows` rows; the pass runs only if *run_if != 0 (nullptr: always)
int run_axis1_mfma(const float* in, int rows, int nx, double sigma, float* out, int table_slot, const int* run_if = nullptr);
// the two passes on the matrix cores: rows `b.out_row0 ...` -> out; tmp: a plane of the same size
int smooth_two_pass(const Block& b, double sigma, float* tmp, float* out, int table_slot, const TwoPass& tp);
// both passes with one sigma on the matrix cores: rows `b.out_row0 ...` -> out; tmp: a plane of the same size
// deferred != nullptr (chunked gradient): on the fused route only the fused kernel is launched, raising *deferred (a flag
// the caller cleared) when it meets a sample that is not a plain finite one; the caller queues the two passes behind
// its last chunk.  Returns whether the two passes are still owed in *owed.
int smooth_both_mfma(const Block& b, double sigma, float* tmp, float* out, int table_slot, bool for_gradient,
                     const int* deferred = nullptr, bool* owed = nullptr);

// ---- gradient.hip ----
// Wave-shift axis 1 + epilogue (smooth_out: the smoothed rows themselves instead, for the long filters of run_axis1).
// TOPO_AMD_EUNSUP when the filter spans too many lanes.
int run_axis1_wave_grad(const float* in, int s_row0, int s_rows, double sigma, const GradArgs& g, float* smooth_out);

}  // namespace topo
