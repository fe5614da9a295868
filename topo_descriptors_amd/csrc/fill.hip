// K8: DEM gaps filled with the nearest valid sample along x (replaces helpers.fill_na, reference helpers.py:137-154:
// interpolate_na(dim="x", method="nearest", fill_value="extrapolate"), and the masking at or below
// CFG.min_elevation of get_dem_netcdf, helpers.py:30-31).
//
// The result is a selection of input samples, so the contract is bit for bit that of scipy's interp1d(kind="nearest")
// on the valid samples of each row (what xarray calls): between the valid neighbours L and R of a missing sample j the
// one with the smaller coordinate is taken when x[j] <= x_lo / 2 + x_hi / 2 in float64 (scipy's midpoints; a tie goes to
// the smaller coordinate), beyond the first / last valid sample the edge sample.  A row with fewer than two valid samples
// is left alone (xarray's fast path): without a threshold its NaNs keep their bits; with one, every missing sample of it
// becomes 0x7FC00000 (numpy's NaN: what the masking, np.where(x > m, x, nan), wrote).
//
// One workgroup owns a row.  Phase 1 reads the row once from HBM: a wave's __ballot over 64 consecutive columns is one
// validity word, kept on chip; valid samples are copied (out of place) and the missing mask written.  A block scan over the
// words gives, per word, the last valid column before it and the first valid column after it.  Phase 2 visits only the
// words that hold a missing sample: the masked bits of the word (clz / ctz) or the scanned neighbours give L and R, and the
// chosen sample is read back (from L2: the block read the row a moment ago) and stored.  Rows of up to kFillWordsOnChip
// words keep the words in LDS (16 KiB); wider rows keep them in a global workspace, one slice per resident block, and the
// blocks stride over the rows.
#include <algorithm>
#include <climits>

#include "common.hpp"

namespace topo {
namespace {

constexpr int kFillThreads = 256;        // four waves
constexpr int kFillStep = 8;             // words (of 64 columns) a wave loads per step: eight loads in flight per lane
constexpr int kFillWordsOnChip = 1024;   // 65536 columns: 8 KiB of words + 8 KiB of scanned neighbours
constexpr int kFillBlocksOffChip = 256;  // resident blocks of the wide-row form (its workspace: 16 B per word and block)
constexpr uint32_t kNumpyNaN = 0x7fc00000u;

// in / out: the first output row of the block (row pitch nx).  out == in: in place (only missing samples are written, only
// valid ones read).  xs: device double[nx] coordinates (nullptr: the column index), ascending: their direction.
template <bool kOnChip>
__global__ __launch_bounds__(kFillThreads) void fill_na_kernel(const uint32_t* in, uint32_t* out, uint8_t* missing, int rows, int nx,
                                                               const double* __restrict__ xs, int ascending, int use_thresh,
                                                               float thresh, unsigned long long* g_mask, int* g_prev, int* g_next) {
    __shared__ unsigned long long s_mask[kOnChip ? kFillWordsOnChip : 1];
    __shared__ int s_prev[kOnChip ? kFillWordsOnChip : 1], s_next[kOnChip ? kFillWordsOnChip : 1];
    __shared__ int s_wave_last[kFillThreads / 64], s_wave_first[kFillThreads / 64];
    const int nw = (nx + 63) >> 6;
    unsigned long long* mask = kOnChip ? s_mask : g_mask + (size_t)blockIdx.x * nw;
    int* prev = kOnChip ? s_prev : g_prev + (size_t)blockIdx.x * nw;   // last valid column before the word (-1: none)
    int* next = kOnChip ? s_next : g_next + (size_t)blockIdx.x * nw;   // first valid column after the word (INT_MAX: none)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int kWaves = kFillThreads / 64;
    const int per = (nw + kFillThreads - 1) / kFillThreads;  // words each thread scans
    const int t0 = min(nw, (int)threadIdx.x * per), t1 = min(nw, t0 + per);

    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const size_t base = (size_t)r * nx;
        const uint32_t* src = in + base;
        uint32_t* dst = out + base;
        uint8_t* mrow = missing ? missing + base : nullptr;
        const bool copy = src != dst;
        __syncthreads();  // the previous row's phase 2 is done with the words

        // ---- phase 1: validity words, copy of the valid samples, the missing mask
        for (int w0 = kFillStep * wave; w0 < nw; w0 += kFillStep * kWaves) {
            const int j0 = w0 * 64 + lane;
            const uint32_t* p = src + j0;  // (one address, constant offsets)
            uint32_t v[kFillStep];
            if (w0 * 64 + kFillStep * 64 <= nx) {
#pragma unroll
                for (int e = 0; e < kFillStep; ++e) v[e] = p[e * 64];
            } else {
#pragma unroll
                for (int e = 0; e < kFillStep; ++e) v[e] = j0 + e * 64 < nx ? p[e * 64] : 0u;
            }
#pragma unroll
            for (int e = 0; e < kFillStep; ++e) {
                const float x = __uint_as_float(v[e]);
                const bool inside = j0 + e * 64 < nx;
                const bool valid = inside && (use_thresh ? x > thresh : x == x);  // (x > thresh is false for NaN)
                const unsigned long long word = __builtin_amdgcn_ballot_w64(valid);
                if (lane == 0 && w0 + e < nw) mask[w0 + e] = word;
                if (copy && valid) dst[j0 + e * 64] = v[e];
                if (mrow && inside) mrow[j0 + e * 64] = valid ? 0 : 1;
            }
        }
        __syncthreads();

        // ---- block scan over the words: each thread a contiguous run of words, waves by shuffles, the block through LDS
        int last = -1, first = INT_MAX;
        for (int w = t0; w < t1; ++w) {
            const unsigned long long m = mask[w];
            if (m) {
                if (first == INT_MAX) first = w * 64 + __builtin_ctzll(m);
                last = w * 64 + 63 - __builtin_clzll(m);
            }
        }
        int incl_last = last, incl_first = first;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int a = __shfl_up(incl_last, d), b = __shfl_down(incl_first, d);
            if (lane >= d) incl_last = max(incl_last, a);
            if (lane + d < 64) incl_first = min(incl_first, b);
        }
        if (lane == 63) s_wave_last[wave] = incl_last;
        if (lane == 0) s_wave_first[wave] = incl_first;
        __syncthreads();
        int before = __shfl_up(incl_last, 1), after = __shfl_down(incl_first, 1);
        if (lane == 0) before = -1;
        if (lane == 63) after = INT_MAX;
        int row_last = -1, row_first = INT_MAX;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            if (k < wave) before = max(before, s_wave_last[k]);
            if (k > wave) after = min(after, s_wave_first[k]);
            row_last = max(row_last, s_wave_last[k]);
            row_first = min(row_first, s_wave_first[k]);
        }
        const bool fill = row_first < row_last;  // two valid samples at least
        int run = before;
        for (int w = t0; w < t1; ++w) {
            prev[w] = run;
            const unsigned long long m = mask[w];
            if (m) run = w * 64 + 63 - __builtin_clzll(m);
        }
        run = after;
        for (int w = t1 - 1; w >= t0; --w) {
            next[w] = run;
            const unsigned long long m = mask[w];
            if (m) run = w * 64 + __builtin_ctzll(m);
        }
        __syncthreads();

        // ---- phase 2: the missing samples, a step of words at a time: first every lane's source column (LDS only), then all
        // the reads of the step at once (their latencies overlap), then the stores
        for (int w0 = kFillStep * wave; w0 < nw; w0 += kFillStep * kWaves) {
            int s[kFillStep];  // column to copy from; -1: nothing to write; -2: numpy's NaN
            bool any = false;
#pragma unroll
            for (int e = 0; e < kFillStep; ++e) {
                const int w = w0 + e;
                s[e] = -1;
                if (w >= nw) continue;
                const unsigned long long m = mask[w];
                const int live = min(64, nx - w * 64);
                const unsigned long long cols = live == 64 ? ~0ull : ((1ull << live) - 1);
                if ((~m & cols) == 0) continue;  // (wave-uniform) nothing missing in this word
                any = true;
                const int j = w * 64 + lane;
                if (lane >= live || ((m >> lane) & 1)) continue;
                if (!fill) {
                    s[e] = use_thresh ? -2 : j;  // (without a threshold the missing samples are the input's NaNs)
                    continue;
                }
                const unsigned long long below = m & ((1ull << lane) - 1);
                const unsigned long long above = m & ~((2ull << lane) - 1);  // (lane 63: 2 << 63 wraps to 0, nothing above)
                const int L = below ? w * 64 + 63 - __builtin_clzll(below) : prev[w];
                const int R = above ? w * 64 + __builtin_ctzll(above) : next[w];
                if (L < 0) {
                    s[e] = R;
                } else if (R == INT_MAX) {
                    s[e] = L;
                } else if (!xs) {
                    s[e] = j - L <= R - j ? L : R;
                } else {
                    // scipy: x_bds = x / 2.0; x_bds[1:] + x_bds[:-1] over the sorted valid coordinates, searchsorted(side="left")
                    const double xl = xs[L], xr = xs[R];
                    const double lo = ascending ? xl : xr, hi = ascending ? xr : xl;
                    const bool take_lo = xs[j] <= hi / 2.0 + lo / 2.0;
                    s[e] = take_lo == (ascending != 0) ? L : R;
                }
            }
            if (!any) continue;  // (wave-uniform)
            uint32_t val[kFillStep];
#pragma unroll
            for (int e = 0; e < kFillStep; ++e) val[e] = s[e] >= 0 ? src[s[e]] : kNumpyNaN;
#pragma unroll
            for (int e = 0; e < kFillStep; ++e)
                if (s[e] != -1) dst[(w0 + e) * 64 + lane] = val[e];
        }
    }
}

}  // namespace

int launch_fill_na(const Block& b, const double* xs, bool ascending, bool use_thresh, float thresh, float* out, uint8_t* missing) {
    Context& c = ctx();
    const int nw = (b.nx + 63) / 64;
    const uint32_t* in = (const uint32_t*)(b.in + (size_t)(b.out_row0 - b.in_row0) * b.nx);
    if (nw <= kFillWordsOnChip) {
        hipLaunchKernelGGL(fill_na_kernel<true>, dim3((unsigned)b.out_rows), dim3(kFillThreads), 0, c.compute, in, (uint32_t*)out, missing,
                           b.out_rows, b.nx, xs, (int)ascending, (int)use_thresh, thresh, nullptr, nullptr, nullptr);
    } else {
        const int blocks = std::min(b.out_rows, kFillBlocksOffChip);
        void* ws = nullptr;
        TOPO_TRY(workspace(12, (size_t)blocks * nw * 16, &ws));
        unsigned long long* g_mask = (unsigned long long*)ws;
        int* g_prev = (int*)(g_mask + (size_t)blocks * nw);
        int* g_next = g_prev + (size_t)blocks * nw;
        hipLaunchKernelGGL(fill_na_kernel<false>, dim3((unsigned)blocks), dim3(kFillThreads), 0, c.compute, in, (uint32_t*)out, missing,
                           b.out_rows, b.nx, xs, (int)ascending, (int)use_thresh, thresh, g_mask, g_prev, g_next);
    }
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}

}  // namespace topo
