// K1v: disc statistics over the samples that exist - TPI and STD that skip missing samples.
//
//   n, s1, s2 : number of valid taps of the disc, sum of x and sum of trunc(x)^2 over them (n', s1': without the tap TPI excludes)
//   TPI = x - s1' / n'                           NaN where the centre is missing or n' < max(1, min_count)
//   STD = sqrt(max(0, (s2 - s1^2 / n) / (n - 1)))  NaN where the centre is missing or n  < max(2, min_count)
//
// A tap is valid when it lies inside the raster and its sample is not MISSING (not finite, or beyond +-2^24); nothing is
// padded with zeros and nothing is poisoned: every output has its own divisor.  On the plan of disc_prefix_kernel (disc.hip):
// a tile plus its halo is staged in LDS, transformed per sample, turned into per-row prefix sums in place, and every output
// takes one prefix difference per disc row.  The images, staged one after the other into the same LDS tile (at 101 px one
// halo tile is 118 KB of the 160 KB):
//   MF   (m << 24) + f   m = 1 for a valid sample, f its fractional part in units of 2^-16 m (|f| <= 2^16)
//   U    m (trunc(x) - c)        c: an integer offset close to the tile's elevation
//   U2   m (trunc(x) - c)^2      (STD only)
// Missing and out-of-domain samples are 0 in every image.  Field widths of MF: a row window holds at most 101 taps, so its
// count is below 2^7 and |sum f| <= 101 * 2^16 < 2^23: count = (d + 2^23) >> 24 and sum f = d - (count << 24) are exact on
// the int32 window sum d, which stays below 2^31.  All sums are exact integers, c drops out, and the closing formulas run in
// float64, rounded to float32 once: the bits depend on no tile, row block or output window.
//
// A tile whose 32-bit window sums cannot hold its samples - a valid |trunc(x)| beyond 2^18, or |trunc(x) - c| beyond
// kReliefLim (101 squares of it fill a uint32: -9999 left finite next to terrain) - is flagged while MF is staged and takes the
// EXACT SLOW FORM in the same launch: every output gathers its taps one by one from the DEM into int64 sums (|x| < 2^24 and
// 10201 taps: below 2^62).  The same integers, hence the same bits, wherever both forms apply.
#include "common.hpp"

#include <algorithm>

namespace topo {

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128;  // output columns per block; lanes run along columns (coalesced)
constexpr int kTileH = 32;   // output rows per block: 256 threads = 128 columns x 2 row phases x 16 outputs
constexpr int kNout = kTileH / 2;
constexpr int kCountShift = 24;
constexpr float kOrdinaryLim = 262144.0f;   // 2^18
constexpr float kMissingLim = 16777216.0f;  // 2^24: at or beyond it (or not finite) a sample is missing
constexpr float kReliefLim = 6521.0f;       // floor(sqrt((2^32 - 1) / 101)): one bound for every size
constexpr size_t kLdsCap = 160 * 1024;

constexpr int lds_stride(int size) { return (kTileW + size - 1 + 1) | 1; }  // +1 for the leading zero; odd: no bank clash
constexpr size_t lds_bytes(int size) { return (size_t)(kTileH + size - 1) * lds_stride(size) * sizeof(uint32_t); }
static_assert(lds_bytes(kDiscValidMaxSize) <= kLdsCap, "the halo tile of the largest disc must fit LDS");
static_assert(kDiscValidMaxSize < (1 << (31 - kCountShift)), "the count field of MF holds a row window");
static_assert((double)kReliefLim * kReliefLim * kDiscValidMaxSize < 4294967296.0, "a row window of u^2 fits uint32");

struct ValidArgs {
    const float* in;
    float* tpi;
    float* sd;
    const int* runs;  // per disc row: lo | (hi << 16), both biased by -di_min (>= 0)
    int* slow;        // set to 1 by a tile that took the exact slow form
    int in_rows, in_row0, gny, nx;
    int out_row0, out_rows;
    int n_disc_rows;  // dj_max - dj_min + 1
    int dj_min, di_min;
    int halo_cols;    // di_max - di_min
    int centre_dj, centre_di;
    int min_tpi, min_std;  // max(1, min_count), max(2, min_count)
};

enum Image { kImgMF = 0, kImgU = 1, kImgU2 = 2 };

// a tap: *v is read only where the tap lies inside the raster (rows outside the block feed unused outputs only)
__device__ __forceinline__ bool load_valid(const ValidArgs& p, int gy, int gx, float* v) {
    const int by = gy - p.in_row0;
    if (gy < 0 || gy >= p.gny || gx < 0 || gx >= p.nx || by < 0 || by >= p.in_rows) return false;
    *v = p.in[(size_t)by * p.nx + gx];
    return fabsf(truncf(*v)) < kMissingLim;  // false for NaN / inf
}

__device__ __forceinline__ int frac16(float v, float t) { return (int)rintf((v - t) * 65536.0f); }

// Stage one image of the tile and turn every LDS row into a prefix sum in place (uint32, modulo 2^32: differences are exact
// while a row-window sum fits 32 bits).  L[r][0] = 0, L[r][k] = sum of the first k staged values of row r.  kImgMF returns
// whether the block met a valid sample the 32-bit images cannot take.
template <int IMG>
__device__ bool stage_and_scan(const ValidArgs& p, uint32_t* L, int stride, int rows_l, int cols_v, int gy0, int gx0, float c,
                               int ci) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int bad = 0;
    for (int r = wave; r < rows_l; r += kThreads / 64) {
        const int gy = gy0 + r;
        uint32_t* row = L + r * stride + 1;
        for (int k = lane; k < cols_v; k += 64) {
            float v = 0.0f;
            uint32_t w = 0;
            if (load_valid(p, gy, gx0 + k, &v)) {
                const float t = truncf(v);
                if (IMG == kImgMF) {
                    if (!(fabsf(t) <= kOrdinaryLim) || !(fabsf(t - c) <= kReliefLim)) bad = 1;
                    w = (1u << kCountShift) + (uint32_t)frac16(v, t);
                } else {
                    const int u = (int)t - ci;
                    w = IMG == kImgU ? (uint32_t)u : (uint32_t)u * (uint32_t)u;
                }
            }
            row[k] = w;
        }
    }
    bool any = false;
    if (IMG == kImgMF) {
        any = __syncthreads_or(bad) != 0;
    } else {
        __syncthreads();
    }
    for (int r = threadIdx.x; r < rows_l; r += kThreads) {
        uint32_t* row = L + r * stride;
        uint32_t run = 0;
        row[0] = 0;
        for (int k = 1; k <= cols_v; ++k) {
            run += row[k];
            row[k] = run;
        }
    }
    __syncthreads();
    return any;
}

// the prefix differences of the disc rows of this thread's kNout outputs (rows row_first, row_first + 2, ...)
template <class Take>
__device__ __forceinline__ void gather(const ValidArgs& p, const uint32_t* L, int stride, int col, int row_first, Take take) {
    for (int d = 0; d < p.n_disc_rows; ++d) {
        const int packed = p.runs[d];  // wave-uniform: scalar load
        const int lo = packed & 0xffff;
        const int hi = packed >> 16;
        const uint32_t* base = L + (row_first + d) * stride + col;
#pragma unroll
        for (int k = 0; k < kNout; ++k) {
            const uint32_t* rowp = base + (2 * k) * stride;
            take(k, rowp[hi + 1] - rowp[lo]);
        }
    }
}

__device__ __forceinline__ double int128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 mag = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    const double d = (double)(uint64_t)(mag >> 64) * 18446744073709551616.0 + (double)(uint64_t)mag;
    return neg ? -d : d;
}

// The exact sums of one output's valid taps: n of them, T = sum trunc(x), F = sum of the fractional parts (2^-16 m),
// S2 = sum trunc(x)^2; ordinary: no tap beyond 2^18 (S2 then stays below 2^53).
struct TapSums {
    int n;
    int64_t T, F, S2;
    bool ordinary;
};

template <bool WANT_TPI, bool WANT_STD>
__device__ __forceinline__ void finish(const ValidArgs& p, int oy, int gx, const TapSums& s) {
    const size_t o = (size_t)(oy - p.out_row0) * p.nx + gx;
    const float nan = __uint_as_float(0x7fc00000u);
    float x = 0.0f;
    const bool have = load_valid(p, oy, gx, &x);
    if (WANT_TPI) {
        // n', s1': without the tap TPI excludes (kernel[size // 2, size // 2]: the pixel itself for odd sizes)
        float xc = 0.0f;
        int n1 = s.n;
        int64_t T1 = s.T, F1 = s.F;
        if (load_valid(p, oy + p.centre_dj, gx + p.centre_di, &xc)) {
            const float tc = truncf(xc);
            n1 -= 1;
            T1 -= (int64_t)(int)tc;
            F1 -= frac16(xc, tc);
        }
        const double s1 = (double)T1 + (double)F1 * (1.0 / 65536.0);
        p.tpi[o] = (have && n1 >= p.min_tpi) ? (float)((double)x - s1 / (double)n1) : nan;
    }
    if (WANT_STD) {
        float v = nan;
        if (have && s.n >= p.min_std) {
            const double n = (double)s.n;
            double var;
            if (s.ordinary) {
                const double s1 = (double)s.T + (double)s.F * (1.0 / 65536.0);
                var = ((double)s.S2 - s1 * s1 / n) / (n - 1.0);
            } else {
                // taps beyond 2^18: 2^32 (n s2 - s1^2) exactly in 128 bits, as disc_prefix_kernel does
                const __int128 A = (__int128)s.n * s.S2 - (__int128)s.T * s.T;
                const __int128 num = (A << 32) - (((__int128)s.T * s.F) << 17) - (__int128)s.F * s.F;
                var = int128_to_double(num) * (1.0 / 4294967296.0) / (n * (n - 1.0));
            }
            if (var < 0.0) var = 0.0;
            v = (float)sqrt(var);
        }
        p.sd[o] = v;
    }
}

// the exact slow form: one output's taps, one by one
template <bool WANT_STD>
__device__ TapSums gather_taps(const ValidArgs& p, int oy, int gx) {
    TapSums s{0, 0, 0, 0, true};
    for (int d = 0; d < p.n_disc_rows; ++d) {
        const int packed = p.runs[d];
        const int x0 = gx + p.di_min + (packed & 0xffff), x1 = gx + p.di_min + (packed >> 16);
        const int gy = oy + p.dj_min + d;
        for (int tx = x0; tx <= x1; ++tx) {
            float v = 0.0f;
            if (!load_valid(p, gy, tx, &v)) continue;
            const float t = truncf(v);
            const int64_t ti = (int)t;
            s.n += 1;
            s.T += ti;
            s.F += frac16(v, t);
            if (WANT_STD) s.S2 += ti * ti;
            if (!(fabsf(t) <= kOrdinaryLim)) s.ordinary = false;
        }
    }
    return s;
}

template <bool WANT_TPI, bool WANT_STD>
__global__ __launch_bounds__(kThreads) void disc_valid_kernel(ValidArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t L[];

    const int cols_v = kTileW + p.halo_cols;  // staged values per LDS row
    const int stride = (cols_v + 1) | 1;
    const int rows_l = kTileH + p.n_disc_rows - 1;

    const int ox0 = blockIdx.x * kTileW;
    // row tiles sit on GLOBAL multiples of kTileH, whatever row block the call is on
    const int oy0 = (p.out_row0 / kTileH + (int)blockIdx.y) * kTileH;
    const int gy0 = oy0 + p.dj_min;
    const int gx0 = ox0 + p.di_min;

    // integer offset near the local elevation: the first ordinary sample among the tile's centre and its quarter points
    // (clamped into the raster and the block's view), 0 without one.  It picks the form a tile takes, never a bit.
    float c = 0.0f;
    {
        const int ylo = max(0, p.in_row0), yhi = min(p.gny, p.in_row0 + p.in_rows) - 1;
        const int qy[5] = {kTileH / 2, kTileH / 4, kTileH / 4, 3 * kTileH / 4, 3 * kTileH / 4};
        const int qx[5] = {kTileW / 2, kTileW / 4, 3 * kTileW / 4, kTileW / 4, 3 * kTileW / 4};
        for (int q = 4; q >= 0; --q) {
            const int y = min(max(oy0 + qy[q], ylo), yhi), x = min(ox0 + qx[q], p.nx - 1);
            const float t = truncf(p.in[(size_t)(y - p.in_row0) * p.nx + x]);
            if (fabsf(t) <= kOrdinaryLim) c = t;  // (false for NaN / inf); the centre, probed last, wins
        }
    }
    const int ci = (int)c;

    const int col = threadIdx.x & (kTileW - 1);
    const int phase = threadIdx.x >> 7;
    const int gx = ox0 + col;

    if (stage_and_scan<kImgMF>(p, L, stride, rows_l, cols_v, gy0, gx0, c, ci)) {
        if (threadIdx.x == 0) atomicOr(p.slow, 1);
        if (gx >= p.nx) return;
        for (int k = 0; k < kNout; ++k) {
            const int oy = oy0 + phase + 2 * k;
            if (oy < p.out_row0 || oy >= p.out_row0 + p.out_rows) continue;
            finish<WANT_TPI, WANT_STD>(p, oy, gx, gather_taps<WANT_STD>(p, oy, gx));
        }
        return;
    }

    int cnt[kNout], sf[kNout];
    int64_t su[kNout], su2[kNout];
#pragma unroll
    for (int k = 0; k < kNout; ++k) {
        cnt[k] = sf[k] = 0;
        su[k] = su2[k] = 0;
    }
    gather(p, L, stride, col, phase, [&](int k, uint32_t d) {
        const int n = ((int)d + (1 << (kCountShift - 1))) >> kCountShift;
        cnt[k] += n;
        sf[k] += (int)d - (n << kCountShift);  // at most 10201 * 2^16 in all: an int32
    });
    __syncthreads();
    stage_and_scan<kImgU>(p, L, stride, rows_l, cols_v, gy0, gx0, c, ci);
    gather(p, L, stride, col, phase, [&](int k, uint32_t d) { su[k] += (int64_t)(int32_t)d; });
    if (WANT_STD) {
        __syncthreads();
        stage_and_scan<kImgU2>(p, L, stride, rows_l, cols_v, gy0, gx0, c, ci);
        gather(p, L, stride, col, phase, [&](int k, uint32_t d) { su2[k] += (int64_t)(uint64_t)d; });
    }

    if (gx >= p.nx) return;
#pragma unroll
    for (int k = 0; k < kNout; ++k) {
        const int oy = oy0 + phase + 2 * k;
        if (oy < p.out_row0 || oy >= p.out_row0 + p.out_rows) continue;
        // sum trunc(x) = Su + c n and sum trunc(x)^2 = Su2 + 2 c Su + c^2 n over the n valid taps: c drops out
        const int64_t n = cnt[k], cl = ci;
        const TapSums s{cnt[k], su[k] + cl * n, (int64_t)sf[k], su2[k] + 2 * cl * su[k] + cl * cl * n, true};
        finish<WANT_TPI, WANT_STD>(p, oy, gx, s);
    }
}

template <bool WANT_TPI, bool WANT_STD>
int launch_kernel(const ValidArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    TOPO_HIP(hipFuncSetAttribute((const void*)disc_valid_kernel<WANT_TPI, WANT_STD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
    hipLaunchKernelGGL((disc_valid_kernel<WANT_TPI, WANT_STD>), grid, dim3(kThreads), lds, s, a);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}

// The flag words of the slow form: a ring in a workspace, one word per call (a call of many launches - row chunks of the
// host pipeline - shares one word).  Zeroed on the compute stream in front of the call's launches, read behind them.
constexpr int kFlagWords = 256;
unsigned g_flag_serial = 0;
thread_local int t_flag_word = -1;

int flag_word(int index, int** out) {
    void* ring = nullptr;
    TOPO_TRY(workspace(kDiscValidFlagSlot, kFlagWords * sizeof(int), &ring));
    *out = (int*)ring + index;
    return TOPO_AMD_OK;
}

}  // namespace

int disc_valid_begin() {
    t_flag_word = (int)(g_flag_serial++ % kFlagWords);
    int* word = nullptr;
    TOPO_TRY(flag_word(t_flag_word, &word));
    TOPO_HIP(hipMemsetAsync(word, 0, sizeof(int), ctx().compute));
    return TOPO_AMD_OK;
}

int disc_valid_slow(int* slow) {
    *slow = 0;
    if (t_flag_word < 0 || !ctx().ready) return TOPO_AMD_OK;
    int* word = nullptr;
    TOPO_TRY(flag_word(t_flag_word, &word));
    TOPO_HIP(hipMemcpyAsync(slow, word, sizeof(int), hipMemcpyDeviceToHost, ctx().compute));
    TOPO_HIP(hipStreamSynchronize(ctx().compute));
    return TOPO_AMD_OK;
}

int launch_tpi_std_valid(const Block& b, const DiscRuns& disc, int min_count, float* tpi_out, float* std_out) {
    TOPO_REQUIRE(tpi_out || std_out, "tpi_std_valid: both outputs are NULL");
    TOPO_REQUIRE(min_count >= 1, "tpi_std_valid: min_count %d (at least 1)", min_count);
    if (disc.size > kDiscValidMaxSize) {
        set_error("tpi_std_valid: disc size %d; the valid-sample kernel covers 1 ... %d", disc.size, kDiscValidMaxSize);
        return TOPO_AMD_EUNSUP;
    }
    if (b.out_rows > kMaxLaunchRows) {
        for (int r = 0; r < b.out_rows; r += kMaxLaunchRows) {
            Block s = b;
            s.out_row0 = b.out_row0 + r;
            s.out_rows = std::min(kMaxLaunchRows, b.out_rows - r);
            TOPO_TRY(launch_tpi_std_valid(s, disc, min_count, tpi_out ? tpi_out + (size_t)r * b.nx : nullptr,
                                          std_out ? std_out + (size_t)r * b.nx : nullptr));
        }
        note_disc_route(noted_disc_route() | kDiscSplit);  // (the word of the last part)
        return TOPO_AMD_OK;
    }
    Context& c = ctx();
    const int n_rows = disc.dj_max - disc.dj_min + 1;
    std::vector<int> packed(n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const int lo = disc.lo[r] - disc.di_min;
        const int hi = disc.hi[r] - disc.di_min;  // empty run encodes hi + 1 == lo
        packed[r] = (lo & 0xffff) | (hi << 16);
    }
    void* d_runs = nullptr;
    TOPO_TRY(upload_table(0, packed.data(), packed.size() * sizeof(int), &d_runs));
    if (t_flag_word < 0) TOPO_TRY(disc_valid_begin());

    ValidArgs a;
    a.in = b.in;
    a.tpi = tpi_out;
    a.sd = std_out;
    a.runs = (const int*)d_runs;
    TOPO_TRY(flag_word(t_flag_word, &a.slow));
    a.in_rows = b.in_rows;
    a.in_row0 = b.in_row0;
    a.gny = b.gny;
    a.nx = b.nx;
    a.out_row0 = b.out_row0;
    a.out_rows = b.out_rows;
    a.n_disc_rows = n_rows;
    a.dj_min = disc.dj_min;
    a.di_min = disc.di_min;
    a.halo_cols = disc.di_max - disc.di_min;
    a.centre_dj = disc.centre_dj;
    a.centre_di = disc.centre_di;
    a.min_tpi = std::max(1, min_count);
    a.min_std = std::max(2, min_count);

    const int stride = (kTileW + a.halo_cols + 1) | 1;
    const size_t lds = (size_t)(kTileH + n_rows - 1) * stride * sizeof(uint32_t);
    TOPO_REQUIRE(lds <= kLdsCap, "tpi_std_valid: the tile of disc size %d does not fit LDS", disc.size);
    dim3 grid((b.nx + kTileW - 1) / kTileW, (b.out_row0 + b.out_rows - 1) / kTileH - b.out_row0 / kTileH + 1);
    const bool tpi = tpi_out != nullptr, sd = std_out != nullptr;
    const int word = kDiscValid | (tpi ? kDiscTpi : 0) | (sd ? kDiscStd : 0) | (kTileH << kDiscTileShift);
    if (tpi && sd) return note_disc_if_ok(launch_kernel<true, true>(a, grid, lds, c.compute), word);
    if (tpi) return note_disc_if_ok(launch_kernel<true, false>(a, grid, lds, c.compute), word);
    return note_disc_if_ok(launch_kernel<false, true>(a, grid, lds, c.compute), word);
}

}  // namespace topo
