// K3v: valid-sample Gaussian - the normalised convolution of a DEM with gaps (topo.dem(skipna=True), Block.gaussian_valid).
//
// With m(q) = 1 where sample q is valid (finite and within +-2^24: the MISSING of disc_valid.hip) and 0 elsewhere, and the
// taps w_y, w_x of the plain Gaussian (gauss.hip: radius int(4 sigma + 0.5), float64-normalised taps rounded to float32,
// scipy's reflect at the GLOBAL edges; a reflected tap is valid exactly when the sample it lands on is):
//     D(p) = sum w_y[i] w_x[j] m(q)          N(p) = sum w_y[i] w_x[j] m(q) x(q)          q = reflect(p + (i, j))
//     out(p) = N / D  where D > 0, D >= min_weight and (fill or m(p) = 1);  NaN elsewhere;  weight(p) = D, always.
// Both sums are separable, so TWO channels go through both 1-D passes and the division happens once, behind the second
// (dividing between the passes is another function).  The mask replaces the plain Gaussian's repair machinery: a missing
// sample is a zero in both channels, nothing non-finite ever reaches an accumulator.
//
// Arithmetic.  A pass accumulates A = sum w m (x - c) and D = sum w m around an offset c and closes with c + A / D, which
// equals N / D for any finite c; c is a sample (axis 0: the middle row of the output group, axis 1: N0 / D0 at the group's
// first column) so that the terms are relief, not elevation.  Both accumulators are float64: next to a gap or a -9999 block
// the terms of a long filter are thousands of metres and hundreds of float32 roundings of such partial sums would cost more
// than the 1e-3 m the mode is held to; x - c is formed in float64 as well, hence exact.  Between the passes D0 and then
// N0 = A0 + c D0 are rounded to float32 ONCE each (the reference's own float32 intermediate); behind axis 1 the quotient is rounded
// once.  No rounding is amplified by a small D: every term of A is bounded by D max|x - c| before the division.
// Offsets and output groups sit on the GLOBAL grid (axis 0: row groups at multiples of TB, like gauss_axis0_kernel; axis 1
// works within a row), so a pixel gets the same instruction sequence in any row block.
#include "gauss.hpp"

namespace topo {

namespace {

// a raw sample as the two channels (m x, m)
__device__ __forceinline__ float2 classify(float v) { return sample_valid(v) ? make_float2(v, 1.0f) : make_float2(0.0f, 0.0f); }

struct ValidGaussArgs {
    const float* in;      // the raw block: axis 0 and the raw axis 1 filter it, the closing rule reads a pixel's own sample
    const float2* nd_in;  // axis 1 behind axis 0: (N0, D0) of exactly the output rows
    float2* nd_out;       // axis 0 in front of axis 1
    float* out;
    float* weight;        // or nullptr
    const float* taps;    // 2R+1 taps followed by zeros up to a multiple of the tap chunk
    int in_rows, in_row0, gny, nx;
    int out_row0, out_rows;
    int radius, nchunks;
    int group0;           // axis 0: first row group (global numbering) that intersects the output rows
    float min_weight;
    int fill;
};

// out and weight of one pixel from the closed sums: value = c + A / D (meaningless where D == 0), own = the raw sample
__device__ __forceinline__ void close_pixel(const ValidGaussArgs& p, size_t at, float value, float d, float own) {
    const bool ok = d > 0.0f && d >= p.min_weight && (p.fill || sample_valid(own));
    p.out[at] = ok ? value : __builtin_nanf("");
    if (p.weight) p.weight[at] = d;
}

// tap_chunks (gauss.hpp) for the two channels: fetch(i) gives (N, D) of sample i - (m x, m) of a raw sample - and
// an[t] = sum_k w[k] (N - c D)[t + k], ad[t] = sum_k w[k] D[t + k] in float64.  A padded zero tap meets finite channels only.
template <int TB, int KB, class Fetch>
__device__ __forceinline__ void tap_chunks2(const float* taps, int nchunks, float c, Fetch fetch, double (&an)[TB],
                                            double (&ad)[TB]) {
    double wn[TB + KB - 1], wd[TB + KB - 1];
    float2 nxt[KB];
    const double nc = -(double)c;
#pragma unroll
    for (int t = 0; t < TB; ++t) an[t] = ad[t] = 0.0;
#pragma unroll
    for (int i = 0; i < TB - 1; ++i) {
        const float2 s = fetch(i);
        wd[i] = (double)s.y;
        wn[i] = fma(nc, wd[i], (double)s.x);
    }
#pragma unroll
    for (int i = 0; i < KB; ++i) nxt[i] = fetch(TB - 1 + i);
    for (int ch = 0; ch < nchunks; ++ch) {
#pragma unroll
        for (int i = 0; i < KB; ++i) {
            wd[TB - 1 + i] = (double)nxt[i].y;
            wn[TB - 1 + i] = fma(nc, wd[TB - 1 + i], (double)nxt[i].x);
        }
        if (ch + 1 < nchunks) {
#pragma unroll
            for (int i = 0; i < KB; ++i) nxt[i] = fetch((ch + 1) * KB + TB - 1 + i);
        }
        const float* w = taps + ch * KB;  // wave-uniform
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            const double wk = (double)w[kk];
#pragma unroll
            for (int t = 0; t < TB; ++t) {
                an[t] = fma(wk, wn[t + kk], an[t]);
                ad[t] = fma(wk, wd[t + kk], ad[t]);
            }
        }
#pragma unroll
        for (int i = 0; i < TB - 1; ++i) {
            wn[i] = wn[i + KB];
            wd[i] = wd[i + KB];
        }
    }
}

// ---- axis 0 (down the columns): lanes run along x, the raw block is classified as it is loaded -------------------------
// Row groups at GLOBAL multiples of TB; c is the group's middle row where that sample is valid, else 0.  The host picks
// TB <= 2 radius, so that row lies within `radius` rows of every row of the group, hence inside any block that computes
// part of it.  LAST: there is no axis 1 behind this pass - close the pixels here.
template <int TB, int KB, bool LAST>
__global__ __launch_bounds__(kThreads) void gauss_valid_axis0_kernel(ValidGaussArgs p) {
    const int x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= p.nx) return;
    const int y0 = (p.group0 + (int)blockIdx.y) * TB;
    const int first = y0 - p.radius;                       // global row of sample 0
    const int last = first + TB - 1 + p.nchunks * KB - 1;  // last sample fetched (the ones past 2 radius + TB - 1 meet no tap)
    const bool plain = first >= 0 && last < p.gny && first >= p.in_row0 && last < p.in_row0 + p.in_rows;
    const float* col = p.in + x;
    auto raw = [&](int i) -> float {
        int gy = first + i;
        if (!plain) {  // wave-uniform: reflect at the global edges, clamp into the block (only rows no tap of an output row meets)
            gy = reflect_index(gy, p.gny);
            gy = min(max(gy, p.in_row0), p.in_row0 + p.in_rows - 1);
        }
        return col[(size_t)(gy - p.in_row0) * p.nx];
    };
    auto fetch = [&](int i) -> float2 { return classify(raw(i)); };
    const float c = fetch(p.radius + TB / 2).x;
    double an[TB], ad[TB];
    tap_chunks2<TB, KB>(p.taps, p.nchunks, c, fetch, an, ad);
#pragma unroll
    for (int t = 0; t < TB; ++t) {
        const int oy = y0 + t;
        if (oy < p.out_row0 || oy >= p.out_row0 + p.out_rows) continue;
        const size_t at = (size_t)(oy - p.out_row0) * p.nx + x;
        const float d = (float)ad[t];
        if (LAST) {
            close_pixel(p, at, (float)((double)c + an[t] / ad[t]), d, col[(size_t)(oy - p.in_row0) * p.nx]);
        } else {
            // N0 around the ROUNDED D0: N0 / D0 = c + A0 / D0 then carries the rounding of D0 on the relief term A0 / D0 only,
            // not on the elevation c (at -9999 m a relative 2^-24 on the whole quotient is 6e-4 m: more than half the budget)
            p.nd_out[at] = make_float2((float)fma((double)c, (double)d, an[t]), d);
        }
    }
}

// ---- axis 1 (along the rows): both channels of a tile staged in LDS as float2, lanes run along y ---------------------------
// block = 32 rows x (NW * 2 * TB) output columns: a half-wave per column group of TB, so that the tile of the longest filter
// (radius 121: 32 x 375 x 8 B = 94 KB) fits LDS, which 64 rows of two channels would not.  One shape for every radius.
// RAW: there was no axis 0 - stage (m x, m) of the raw rows.
template <int TB, int KB, int NW, bool RAW>
__global__ __launch_bounds__(NW * 64) void gauss_valid_axis1_kernel(ValidGaussArgs p) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int TR = 32;
    constexpr int TC = NW * 2 * TB;
    const int R = p.radius;
    const int cols_l = TC + p.nchunks * KB - 1;  // samples a row of the tile can be asked for
    const int stride = cols_l | 1;               // odd, in 8-byte words: a half-wave's 32 rows meet 32 different bank pairs
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int ox0 = blockIdx.x * TC;
    const int oy0 = blockIdx.y * TR;  // relative to out_row0; rows here need no halo

    const bool inner = ox0 - R >= 0 && ox0 - R + cols_l <= p.nx;
    for (int r = wave; r < TR; r += NW) {
        const int row = min(oy0 + r, p.out_rows - 1);
        float2* dst = tile + r * stride;
        for (int k = lane; k < cols_l; k += 64) {
            const int gx = inner ? ox0 - R + k : reflect_index(ox0 - R + k, p.nx);
            if (RAW) {
                dst[k] = classify(p.in[(size_t)(row + p.out_row0 - p.in_row0) * p.nx + gx]);
            } else {
                dst[k] = p.nd_in[(size_t)row * p.nx + gx];
            }
        }
    }
    __syncthreads();

    const int r = lane & (TR - 1);
    const int group = wave * 2 + (lane >> 5);
    const float2* rowp = tile + r * stride + group * TB;
    auto fetch = [&](int i) -> float2 { return rowp[i]; };
    const float2 s0 = rowp[R];  // the group's first column (a column of the global grid: ox0 is a multiple of TC)
    const float c = s0.y > 0.0f ? finite_or_zero(s0.x / s0.y) : 0.0f;
    double an[TB], ad[TB];
    tap_chunks2<TB, KB>(p.taps, p.nchunks, c, fetch, an, ad);
    __syncthreads();
    // transpose back through LDS so the stores are row-coalesced: (c + A / D, D)
    constexpr int ostride = TC + 1;  // (<= stride: cols_l >= TC + KB - 1)
#pragma unroll
    for (int t = 0; t < TB; ++t)
        tile[r * ostride + group * TB + t] = make_float2((float)((double)c + an[t] / ad[t]), (float)ad[t]);
    __syncthreads();
    for (int idx = threadIdx.x; idx < TR * TC; idx += NW * 64) {
        const int orow = idx / TC, k = idx % TC;
        const int oy = oy0 + orow, ox = ox0 + k;
        if (oy >= p.out_rows || ox >= p.nx) continue;
        const float2 v = tile[orow * ostride + k];
        const float own = p.fill ? 0.0f : p.in[(size_t)(oy + p.out_row0 - p.in_row0) * p.nx + ox];
        close_pixel(p, (size_t)oy * p.nx + ox, v.x, v.y, own);
    }
}

// ---- neither axis filters (sigma 0, radius 0): the sample's own bits where it is valid, the weight its 0 / 1 mask ---------
__global__ __launch_bounds__(kThreads) void gauss_valid_mask_kernel(ValidGaussArgs p) {
    const size_t n = (size_t)p.out_rows * p.nx;
    const float* src = p.in + (size_t)(p.out_row0 - p.in_row0) * p.nx;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const float v = src[i];
        close_pixel(p, i, v, sample_valid(v) ? 1.0f : 0.0f, v);
    }
}

constexpr int kA1TB = 8, kA1KB = 8, kA1NW = 8;  // the axis-1 tile: 32 rows x 128 columns, 512 threads
constexpr size_t axis1_lds(int R) {
    return (size_t)32 * ((kA1NW * 2 * kA1TB + tap_chunk_count(R, kA1KB) * kA1KB - 1) | 1) * sizeof(float2);
}
static_assert(axis1_lds(kGaussValidMaxRadius) <= kLdsMax, "the two-channel tile of the longest filter must fit LDS");

// taps of sigma in chunks of kb, through the table slot of the plain Gaussian's pass on that axis
int valid_taps(double sigma, int kb, int slot, ValidGaussArgs* a) {
    GaussArgs g;
    TOPO_TRY(gauss_args(Block{}, nullptr, sigma, kb, slot, &g));
    a->taps = g.taps;
    a->radius = g.radius;
    a->nchunks = g.nchunks;
    return TOPO_AMD_OK;
}

template <int TB, int KB>
int launch_axis0(ValidGaussArgs a, double sigma, bool last) {
    TOPO_TRY(valid_taps(sigma, KB, 1, &a));
    a.group0 = a.out_row0 / TB;
    const int groups = (a.out_row0 + a.out_rows - 1) / TB - a.group0 + 1;
    dim3 grid((a.nx + kThreads - 1) / kThreads, groups);
    return last ? launch(gauss_valid_axis0_kernel<TB, KB, true>, grid, dim3(kThreads), 0, ctx().compute, a)
                : launch(gauss_valid_axis0_kernel<TB, KB, false>, grid, dim3(kThreads), 0, ctx().compute, a);
}

// the tallest row group whose middle row every block holds: TB <= 2 radius; long filters take 16 rows a thread
int run_axis0(const ValidGaussArgs& a, double sigma, bool last) {
    const int R = gaussian_radius(sigma);
    if (R >= 16) return launch_axis0<16, 8>(a, sigma, last);
    if (R >= 4) return launch_axis0<8, 8>(a, sigma, last);
    if (R >= 2) return launch_axis0<4, 4>(a, sigma, last);
    return launch_axis0<2, 2>(a, sigma, last);
}

int run_axis1(ValidGaussArgs a, double sigma, bool raw) {
    TOPO_TRY(valid_taps(sigma, kA1KB, 2, &a));
    const size_t lds = axis1_lds(a.radius);
    dim3 grid((a.nx + kA1NW * 2 * kA1TB - 1) / (kA1NW * 2 * kA1TB), (a.out_rows + 31) / 32);
    return raw ? launch_big_lds<gauss_valid_axis1_kernel<kA1TB, kA1KB, kA1NW, true>>(grid, dim3(kA1NW * 64), lds, a)
               : launch_big_lds<gauss_valid_axis1_kernel<kA1TB, kA1KB, kA1NW, false>>(grid, dim3(kA1NW * 64), lds, a);
}

// rows [row0, row0 + rows) of the block into out / weight (both start at row0)
int smooth_valid_rows(const Block& b, double sigma_y, double sigma_x, float min_weight, bool fill, int row0, int rows, float* out,
                      float* weight) {
    const bool do_y = sigma_y > 1e-15 && gaussian_radius(sigma_y) >= 1, do_x = sigma_x > 1e-15 && gaussian_radius(sigma_x) >= 1;
    ValidGaussArgs a{};
    a.in = b.in;
    a.out = out;
    a.weight = weight;
    a.in_rows = b.in_rows;
    a.in_row0 = b.in_row0;
    a.gny = b.gny;
    a.nx = b.nx;
    a.out_row0 = row0;
    a.out_rows = rows;
    a.min_weight = min_weight;
    a.fill = fill ? 1 : 0;
    if (do_y && do_x) {
        void* nd = nullptr;
        TOPO_TRY(workspace(kGaussValidSlot, (size_t)rows * b.nx * sizeof(float2), &nd));
        a.nd_out = (float2*)nd;
        a.nd_in = (const float2*)nd;
        TOPO_TRY(run_axis0(a, sigma_y, false));
        return run_axis1(a, sigma_x, false);
    }
    if (do_y) return run_axis0(a, sigma_y, true);
    if (do_x) return run_axis1(a, sigma_x, true);
    const size_t n = (size_t)rows * b.nx;
    const unsigned blocks = (unsigned)std::min<size_t>((n + kThreads - 1) / kThreads, 65535);
    return launch(gauss_valid_mask_kernel, dim3(blocks), dim3(kThreads), 0, ctx().compute, a);
}

}  // namespace

int launch_gaussian_valid(const Block& b, double sigma_y, double sigma_x, double min_weight, bool fill, float* out, float* weight) {
    for (double sigma : {sigma_y, sigma_x})
        if (4.0 * sigma + 0.5 >= kGaussValidMaxRadius + 1.0) {  // (compared as doubles: no cast of an absurd sigma)
            set_error("gaussian_valid: sigma %.3f (radius %.0f); the valid-sample Gaussian covers radii 0 ... %d", sigma,
                      std::floor(4.0 * sigma + 0.5), kGaussValidMaxRadius);
            return TOPO_AMD_EUNSUP;
        }
    return for_row_slabs(b.out_rows, [&](int r, int n) {
        return smooth_valid_rows(b, sigma_y, sigma_x, (float)min_weight, fill, b.out_row0 + r, n, out + (size_t)r * b.nx,
                                 weight ? weight + (size_t)r * b.nx : nullptr);
    });
}

}  // namespace topo
