// K3 on the matrix cores: the Gaussian's banded Toeplitz products as f16 MFMAs - tile kernels for both axes, the
// split-once axis-1 kernel, both passes fused in one kernel, the float32 repair pass - and their launchers.
// Which radius gets which of them, and what is built: gauss_route.hpp.
#include "gauss.hpp"

namespace topo {

namespace {

// ---- long filters on the matrix cores: banded Toeplitz x data with v_mfma_f32_32x32x2_f32 --------------
// out = T in, T[i][k] = w[k - i] for 0 <= k - i <= 2 R.  For a tile of 32 outputs along the filter axis the
// band touches K = 32 + 2 R inputs, so the product spends (32 + 2 R) / (2 R + 1) of the minimum number of
// multiply-adds (1.13 at radius 121) - but at the f32 MFMA rate, which one wave per SIMD reaches with
// nothing but an LDS read per operand, where the vector-ALU kernels issue 2.3 instructions per useful FMA.
// The result of a 32x32x2 f32 MFMA chain is the k-ordered fmaf chain, one rounding per product; the taps
// outside the band are exact zeros, so an output is the fmaf chain over its own 2 R + 1 taps in ascending
// order whatever tile it falls in (partition invariance needs no tile alignment; only the accumulation
// offsets do: they are taken per column / per row from samples that any block covering the output holds).
// A non-finite sample reaches every output of the tiles whose (padded) band contains it (0 x NaN), i.e. up to 37
// rows / columns further than in ndimage.gaussian_filter.  Two accumulators (even / odd groups) were tried to
// take the dependent-MFMA wait out: 7.9 ms against 6.9 ms for the one chain, so it stays one chain.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// (the float32 matrix-core kernels of round 2 - v_mfma_f32_32x32x2_f32, 11.3 ms at sigma 30.25 - were retired in round 5:
// docs/DESIGN_HISTORY.md, profiles/r02_gauss_mfma.txt, r03_gauss_f16.txt keep their numbers)

// ---- the banded products on the f16 matrix pipe (round 3) ------------------------------------------------
// v_mfma_f32_32x32x16_f16 does 16 x the multiply-adds of the f32 instruction per cycle.  A float32 difference
// d = (x - c) / 4 (c: the tile's offset as above; the quarter keeps |d| inside f16 for any |x| <= 1e5) is split
// on the fly into d = h + l + e, h = d cut to 11 significant bits (exact in f16), l = f16(d - h) rounded to
// nearest, |e| <= 2^-22 |d|; a tap t 2^k (k: the scale that puts the largest tap in [512, 1024)) into th + tm the
// same way, once per kernel, in registers.  Three products stand for t d: th h + tm h + th l (the fourth, tm l, is
// <= 2^-22 t d like e).  The sums are float32 inside the matrix pipe, 3 roundings per 16 taps instead of 16, on
// values of the size of x - c: the error against the exact filter is that of the f32 chain or smaller
// (tools/gauss_f16_error.py).  x = c over a lake gives h = l = 0 and the output c, as before.
// What changes is the order of the additions: 16 taps at a time, on a grid of steps that starts Rp = R rounded up
// to 16 above (left of) the 32-output tile.  Tiles sit on global multiples of 32 on both axes, so an output still
// sees the same operands in the same places whatever row block it is computed in.
// Non-finite and absurd samples (|x| > 1e5) never reach the matrix pipe: the loader stages them as 0, remembers
// that the window holds one, and the tile is marked; the repair pass then recomputes, tap by tap in float32, the
// outputs whose OWN window holds such a sample and leaves the others alone (they are what they would be without
// it: a zero tap times 0 or times a finite sample adds the same nothing).  The mark may be conservative (a block's
// clamped ghost rows, neighbouring columns): it costs time, never bits.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr float kWild = 1.0e5f;
__device__ __forceinline__ bool wild(float x) { return !(fabsf(x) <= kWild); }

// lane (j = lane & 31, g = lane >> 5) of step s holds the taps T[j][16 s + 8 g + q], q = 0 ... 7: the operand the
// Toeplitz factor has on either side of the product (A for axis 0, B for axis 1: the band is symmetric)
template <int S>
__device__ __forceinline__ void build_tap_blocks(const float* taps, int R, float scale, int lane, f16x8 (&hi)[S], f16x8 (&lo)[S]) {
    const int j = lane & 31, g = lane >> 5, Rp = 8 * (S - 2);
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = 16 * s + 8 * g + q - j - (Rp - R);
            const float t = (n >= 0 && n <= 2 * R) ? taps[n] * scale : 0.0f;
            const _Float16 th = (_Float16)t;
            hi[s][q] = th;
            lo[s][q] = (_Float16)(t - (float)th);
        }
    }
}

// 8 samples -> (x - c) / 4 -> f16 pair of operands
__device__ __forceinline__ void split8(const float (&x)[8], f32x2 quarter, f32x2 mcq, f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        // (plain fma / sub: a wave alone on its SIMD takes 53 ns for the 8 samples this way, 64 ns with v_pk_fma_f32 /
        // v_pk_add_f32: tools/ubench/split_rate.hip)
        const f32x2 d = {__builtin_fmaf(x[2 * u], quarter[0], mcq[0]), __builtin_fmaf(x[2 * u + 1], quarter[1], mcq[1])};
        // (as one vector operation: __builtin_bit_cast on the ELEMENT d[1] reads d[0] with this compiler)
        const f32x2 hf = __builtin_bit_cast(f32x2, __builtin_bit_cast(u32x2, d) & u32x2{0xFFFFE000u, 0xFFFFE000u});
        const f32x2 r = {d[0] - hf[0], d[1] - hf[1]};
        const f16x2 hh = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(hf[0], hf[1]));  // exact: hf has 11 bits
        const f16x2 ll = __builtin_convertvector(r, f16x2);                                     // v_cvt_pk_f16_f32, to nearest
        hi[2 * u] = hh[0];
        hi[2 * u + 1] = hh[1];
        lo[2 * u] = ll[0];
        lo[2 * u + 1] = ll[1];
    }
}

template <bool DATA_IS_A, int NP>
__device__ __forceinline__ void f16_products(const f16x8& th, const f16x8& tm, const f16x8& dh, const f16x8& dl, f32x16& acc) {
    if (DATA_IS_A) {
        if (NP >= 4) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl, tm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, tm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl, th, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, th, acc, 0, 0, 0);
    } else {
        if (NP >= 4) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(tm, dl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(tm, dh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, dl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, dh, acc, 0, 0, 0);
    }
}

constexpr int kNoWild = -(1 << 28);

// Axis 0.  A wave owns 32 columns and a run of row tiles, top to bottom, and talks to nobody: its window of input
// rows is a ring in LDS (its 32 columns of the block's [row][128] array), the rows the next tile adds are loaded
// into registers while this tile is computed and written over the oldest rows afterwards (the wave's own reads come
// first in program order: no spare rows, no barrier).
// MT = 2: the wave's tile is 64 rows (two MFMA tiles on top of each other, global multiples of 64) with ONE offset
// per column, so one split of the samples feeds both: the vector-ALU work per output halves.  The offset row is 32
// rows into the tile; a row block holds it for every tile it computes when it carries 32 ghost rows, so the
// launcher takes MT = 2 from radius 32 (except behind a fused launch, whose bands are 32-row tiles).
template <int S, int NP, int MT>
__global__ __launch_bounds__(256) void gauss_axis0_f16_kernel(GaussArgs p, int tile_first, int ntiles, int tiles_per_block) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    constexpr int Rp = 8 * (S - 2), NS = S + 2 * (MT - 1), RR = 16 * NS, TILE = 32 * MT;
    constexpr int kStay = (RR + TILE - 1) / TILE;  // tiles whose window holds a slab of TILE rows, rounded up
    static_assert(S % 2 == 0, "whole 16-row steps on both sides of the tile");
    const int R = p.radius;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, g = lane >> 5;
    const int x0 = blockIdx.x * kMfmaCols;
    const int tb = blockIdx.y * tiles_per_block, te = min(tb + tiles_per_block, ntiles);
    if (tb >= te) return;
    if (p.run_if && *p.run_if == 0) return;
    f16x8 twh[S], twl[S];
    build_tap_blocks<S>(p.taps, R, p.tap_scale, lane, twh, twl);
    float* ring = L + 32 * wave;  // [row][128], this wave's 32 columns
    // loader: lane -> row (lane >> 3) of a pass of 8 rows, 4 columns (lane & 7) * 4
    const int lq = lane >> 3, lcol = (lane & 7) * 4;
    typedef float f4 __attribute__((ext_vector_type(4)));
    // the lane's 4 columns of a row: one 16-byte load (dword alignment is all it needs, so any row length will do); the
    // group that straddles the DEM's right edge (widths that are not multiples of 4) and the groups beyond it go
    // column by column, clamped (what lies past the edge is never stored)
    const int lx = x0 + 32 * wave + lcol;
    const bool lane_full = lx + 4 <= p.nx;
    auto load4 = [&](const float* rowbase) {
        if (lane_full) return *reinterpret_cast<const f4*>(rowbase + lx);
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rowbase[min(lx + e, p.nx - 1)];
        return v;
    };
    auto row_base = [&](int gy) {
        gy = reflect_index(gy, p.gny);
        gy = min(max(gy, p.in_row0), p.in_row0 + p.in_rows - 1);
        return p.in + (size_t)(gy - p.in_row0) * p.nx;
    };
    float* const ring_lane = ring + lq * kMfmaCols + lcol;
    const int row_lo = max(0, p.in_row0), row_hi = min(p.gny, p.in_row0 + p.in_rows);
    int last_wild = kNoWild;  // last tile whose window holds a staged sample that is not a plain finite one
    {
        const int y0 = (tile_first + tb) * TILE;
        bool bad = false;
        for (int k = 0; k < RR; k += 8) {
            f4 v = load4(row_base(y0 - Rp + k + lq));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool w = wild(v[e]);
                bad |= w;
                v[e] = w ? 0.0f : v[e];
            }
            *reinterpret_cast<f4*>(ring_lane + k * kMfmaCols) = v;
        }
        if (__builtin_amdgcn_ballot_w64(bad)) last_wild = tb + kStay - 1;
    }
    int base = 0;  // ring row of input row y0 - Rp
    const int xw = 32 * wave + j;
    const unsigned out_lane_off = (unsigned)(4 * g * p.nx + xw) * 4u;
    const f32x2 quarter = {0.25f, 0.25f};
    const float* const bl = L + (8 * g) * kMfmaCols + xw;
    for (int t = tb; t < te; ++t) {
        const int y0 = (tile_first + t) * TILE;
        f4 pre[4 * MT];
        const bool more = t + 1 < te;
        if (more) {
            const int n0 = y0 - Rp + RR;  // the rows the next tile adds
            if (n0 >= row_lo && n0 + TILE <= row_hi) {
                const float* rb = p.in + (size_t)(n0 + lq - p.in_row0) * p.nx;
#pragma unroll
                for (int q = 0; q < 4 * MT; ++q) pre[q] = load4(rb + (size_t)(8 * q) * p.nx);
            } else {
#pragma unroll
                for (int q = 0; q < 4 * MT; ++q) pre[q] = load4(row_base(n0 + 8 * q + lq));
            }
        }
        int sc = base + Rp + TILE / 2;
        sc = sc >= RR ? sc - RR : sc;
        const float c = L[sc * kMfmaCols + xw];  // the column's sample at the tile's middle row (0 if it was not a plain finite one)
        const f32x2 mcq = {-0.25f * c, -0.25f * c};
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[m][v] = 0.0f;
        int slot = base;
        auto fetch = [&](float (&x)[8]) {
            const float* bp = bl + slot * kMfmaCols;
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = bp[q * kMfmaCols];
            slot += 16;
            slot = slot >= RR ? slot - RR : slot;
        };
        float xa[8], xb[8];
        fetch(xa);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            f16x8 dh, dl;
            // the next step's samples are requested before this step's are split (the compiler otherwise sinks the
            // reads to their use and the wave, alone on its SIMD, waits out the LDS latency every step)
            if (s & 1) {
                if (s + 1 < NS) fetch(xa);
                __builtin_amdgcn_sched_barrier(0);
                split8(xb, quarter, mcq, dh, dl);
            } else {
                if (s + 1 < NS) fetch(xb);
                __builtin_amdgcn_sched_barrier(0);
                split8(xa, quarter, mcq, dh, dl);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (s - 2 * m >= 0 && s - 2 * m < S) f16_products<false, NP>(twh[s - 2 * m], twl[s - 2 * m], dh, dl, acc[m]);
        }
        if (more) {
            bool bad = false;
#pragma unroll
            for (int q = 0; q < 4 * MT; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) bad |= wild(pre[q][e]);
            if (__builtin_amdgcn_ballot_w64(bad)) {
#pragma unroll
                for (int q = 0; q < 4 * MT; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) pre[q][e] = wild(pre[q][e]) ? 0.0f : pre[q][e];
                last_wild = t + kStay;  // the rows enter with tile t + 1
            }
            int s8 = base;  // over the oldest rows
#pragma unroll
            for (int q = 0; q < 4 * MT; ++q) {
                *reinterpret_cast<f4*>(ring_lane + s8 * kMfmaCols) = pre[q];
                s8 += 8;
                s8 = s8 >= RR ? s8 - RR : s8;
            }
        }
        const int ox = x0 + xw;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int ym = y0 + 32 * m;
            if (lane == 0) p.flags[((size_t)(t * MT + m) * gridDim.x + blockIdx.x) * 4 + wave] = last_wild >= t ? 1 : 0;
            if (ox < p.nx) {
                if (ym >= p.out_row0 && ym + 32 <= p.out_row0 + p.out_rows) {
                    char* ub = reinterpret_cast<char*>(p.out + (size_t)(ym - p.out_row0) * p.nx + x0);
#pragma unroll
                    for (int v = 0; v < 16; ++v)
                        *reinterpret_cast<float*>(ub + (size_t)((v & 3) + 8 * (v >> 2)) * p.nx * 4 + out_lane_off) = fmaf(acc[m][v], p.out_scale, c);
                } else {
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int oy = ym + (v & 3) + 8 * (v >> 2) + 4 * g;
                        if (oy >= p.out_row0 && oy < p.out_row0 + p.out_rows) p.out[(size_t)(oy - p.out_row0) * p.nx + ox] = fmaf(acc[m][v], p.out_scale, c);
                    }
                }
            }
        }
        base += TILE;
        base = base >= RR ? base - RR : base;
    }
}

// Axis 1.  A wave owns a band of 32 rows and marches along x; its window of input columns is a ring of LDS columns
// (row pitch = window + 4 floats: the two 16-byte reads of an A operand are aligned and 16 rows fall into 16
// different bank groups).  `in` holds plane rows [0, rows); a row's result depends on that row alone.  MT = 2: tiles
// of 64 columns with one offset per row (the sample 32 columns into the tile: always there), one split for two MFMA
// tiles.  NW waves per block: the widest window (radius 113 ... 121, MT = 2) fits LDS three times, not four.
template <int S, int NP, int MT, int NW>
__global__ __launch_bounds__(64 * NW) void gauss_axis1_f16_kernel(GaussArgs p, int rows, int nseg) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    constexpr int Rp = 8 * (S - 2), NS = S + 2 * (MT - 1), RC = 16 * NS, pitch = RC + 4, TILE = 32 * MT;
    constexpr int kStay = (RC + TILE - 1) / TILE;
    static_assert(S % 2 == 0, "whole 16-column steps on both sides of the tile");
    const int R = p.radius;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* ring = L + wave * (32 * pitch + 32);
    float* crow = ring + 32 * pitch;
    const int gw = blockIdx.x * NW + wave;
    const int band = gw / nseg, seg = gw - band * nseg;
    const int r0 = band * 32;
    if (r0 >= rows) return;
    if (p.run_if && *p.run_if == 0) return;
    const int i = lane & 31, g = lane >> 5;
    f16x8 twh[S], twl[S];
    build_tap_blocks<S>(p.taps, R, p.tap_scale, lane, twh, twl);
    auto load_cols = [&](int xfirst, int q) {  // rows 2 q + g, columns xfirst + i
        const int r = min(r0 + 2 * q + g, rows - 1);
        const int cx = reflect_index(xfirst + i, p.nx);
        return p.in[(size_t)r * p.nx + cx];
    };
    const unsigned in_lane_off = (unsigned)(g * p.nx + i) * 4u;
    const unsigned out_lane_off = (unsigned)(4 * g * p.nx + i) * 4u;
    const bool full_band = r0 + 32 <= rows;
    const int ntile = (p.nx + TILE - 1) / TILE, nunit = (p.nx + 31) / 32;
    const int tper = (ntile + nseg - 1) / nseg;
    const int seg_first = seg * tper, seg_last = min(seg_first + tper, ntile);
    if (seg_first >= seg_last) return;
    // (the bands do not walk the row in step: gauss_axis1_s1_kernel has the reasons)
    const int turn = p.group0 != 0 && ntile >= 32 ? (int)(((unsigned)band * 40503u) % (unsigned)ntile) : 0;
    const int run_first = (seg_first + turn) % ntile, run_len = seg_last - seg_first;
    for (int part = 0; part < 2; ++part) {
    const int t_first = part == 0 ? run_first : 0;
    const int t_last = part == 0 ? min(run_first + run_len, ntile) : run_first + run_len - ntile;
    if (t_first >= t_last) continue;
    int last_wild = kNoWild;
    {
        bool bad = false;
        for (int k0 = 0; k0 < RC; k0 += 32) {
            if (k0 + i < RC) {
#pragma unroll 4
                for (int q = 0; q < 16; ++q) {
                    const float v = load_cols(t_first * TILE - Rp + k0, q);
                    const bool w = wild(v);
                    bad |= w;
                    ring[(2 * q + g) * pitch + k0 + i] = w ? 0.0f : v;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(bad)) last_wild = t_first + kStay - 1;
    }
    int base = 0;  // ring column of input column x0 - Rp
    const f32x2 quarter = {0.25f, 0.25f};
    typedef float f4 __attribute__((ext_vector_type(4)));
    const float* const al = ring + i * pitch + 8 * g;
    for (int t = t_first; t < t_last; ++t) {
        const int x0 = t * TILE;
        float pre[16 * MT];
        const bool more = t + 1 < t_last;
        if (more) {
            const int n0 = x0 - Rp + RC;  // the columns the next tile adds
            if (full_band && n0 >= 0 && n0 + TILE <= p.nx) {
                const char* rb = reinterpret_cast<const char*>(p.in + (size_t)r0 * p.nx + n0);
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int q = 0; q < 16; ++q) pre[16 * m + q] = *reinterpret_cast<const float*>(rb + (size_t)(2 * q) * p.nx * 4 + 128 * m + in_lane_off);
            } else {
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int q = 0; q < 16; ++q) pre[16 * m + q] = load_cols(n0 + 32 * m, q);
            }
        }
        int sc = base + Rp + TILE / 2;
        sc = sc >= RC ? sc - RC : sc;
        const float c = ring[i * pitch + sc];  // the row's sample at the tile's middle column
        if (g == 0) crow[i] = c;
        const f32x2 mcq = {-0.25f * c, -0.25f * c};
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[m][v] = 0.0f;
        int slot = base;
        auto fetch = [&](float (&x)[8]) {
            const f4 lo4 = *reinterpret_cast<const f4*>(al + slot), hi4 = *reinterpret_cast<const f4*>(al + slot + 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = lo4[q];
                x[4 + q] = hi4[q];
            }
            slot += 16;
            slot = slot >= RC ? slot - RC : slot;
        };
        float xa[8], xb[8];
        fetch(xa);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            f16x8 dh, dl;
            if (s & 1) {
                if (s + 1 < NS) fetch(xa);
                __builtin_amdgcn_sched_barrier(0);
                split8(xb, quarter, mcq, dh, dl);
            } else {
                if (s + 1 < NS) fetch(xb);
                __builtin_amdgcn_sched_barrier(0);
                split8(xa, quarter, mcq, dh, dl);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (s - 2 * m >= 0 && s - 2 * m < S) f16_products<true, NP>(twh[s - 2 * m], twl[s - 2 * m], dh, dl, acc[m]);
        }
        if (more) {
            bool bad = false;
#pragma unroll
            for (int q = 0; q < 16 * MT; ++q) bad |= wild(pre[q]);
            if (__builtin_amdgcn_ballot_w64(bad)) {
#pragma unroll
                for (int q = 0; q < 16 * MT; ++q) pre[q] = wild(pre[q]) ? 0.0f : pre[q];
                last_wild = t + kStay;
            }
            int sl = base;  // over the oldest columns
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int q = 0; q < 16; ++q) ring[(2 * q + g) * pitch + sl + i] = pre[16 * m + q];
                sl += 32;
                sl = sl >= RC ? sl - RC : sl;
            }
        }
        float cr[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) cr[v] = crow[(v & 3) + 8 * (v >> 2) + 4 * g];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int xm = x0 + 32 * m, ox = xm + i;  // D: column = lane & 31
            if (xm >= p.nx) break;
            if (lane == 0) p.flags[(size_t)band * nunit + (t * MT + m)] = last_wild >= t ? 1 : 0;
            if (ox < p.nx) {
                if (full_band) {
                    char* ub = reinterpret_cast<char*>(p.out + (size_t)r0 * p.nx + xm);
#pragma unroll
                    for (int v = 0; v < 16; ++v)
                        *reinterpret_cast<float*>(ub + (size_t)((v & 3) + 8 * (v >> 2)) * p.nx * 4 + out_lane_off) = fmaf(acc[m][v], p.out_scale, cr[v]);
                } else {
                    float* o = p.out + (size_t)(r0 + 4 * g) * p.nx + ox;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int ri = (v & 3) + 8 * (v >> 2);
                        if (r0 + 4 * g + ri < rows) o[(size_t)ri * p.nx] = fmaf(acc[m][v], p.out_scale, cr[v]);
                    }
                }
            }
        }
        base += TILE;
        base = base >= RC ? base - RC : base;
    }
    }
}

// ---- split once: axis 1, radius 49 ... 121 -------------------------------------------------------------------------
// The kernels above split every sample of a tile's window into its f16 pair again for every tile: 24 vector
// instructions per 8 samples and step (profiles/r03_gauss_f16.txt, section 5).  Here a sample is split ONCE, when it
// is staged: the ring in LDS holds the two f16 planes and a step is two 16-byte LDS reads and its MFMAs.  For that the
// offset a sample is taken against cannot belong to the tile: the row is cut into slabs of 64 columns (global
// multiples of 64) and every sample of a slab is taken against the slab's reference c_s, the sample of its row in
// the slab's first column.  A tile's window holds up to five slabs; with W_s[o] the sum of the taps that the output at
// position o of its own slab lays over slab s (a table of the host: float64 sums, rounded once) and b the tile's slab
//     out = c_b + [ scale * sum_k t_k (x_k - c_s(k)) / 4  +  sum_{s != b} (c_s - c_b) W_s ]
// - the taps sum to 1 as far as the tile kernels' "+ c" assumes it.  |x - c_s| is the relief inside 64 samples (the
// tile kernels: inside the 288 ... 320 of a window); the correction costs 2.5 vector instructions per output and slab.
// Results depend on the global slab grid only, not on how the march is cut.  Samples that are not plain finite ones go
// in as 0 and mark the tiles whose windows hold them (or hold samples taken against a reference that was one), as
// above: the repair pass recomputes those.  (Axis 0 was built the same way - a wave owns 16 columns, slab references
// on row 32 of each 64-row slab, R + 32 ghost rows for whole-DEM bits - and gives the tile kernel's time, 2.51 against
// 2.56 ms at sigma 30.25: 16 columns are 64-byte halves of lines shared with the neighbour wave, 1.56 x the plane
// fetched unless a block barrier per tile keeps the waves together, which takes the overlap away again; it is not in the
// library: profiles/r04_gauss_split_once.txt.  Round 6 built it again with staging waves loading whole 512-byte row
// segments for the block, and once more with every wave for itself at one wave per SIMD: correct, 5 - 8 % on axis 0 alone at
// radius 97 ... 121, nothing on the gradient, R + 32 ghost rows for every caller - left out again: profiles/r06_gauss_axis0_s1.txt,
// commit d700ebd.)
__device__ __forceinline__ int floor_div64(int a) { return a >> 6; }  // arithmetic shift: floor for negative a
// The ring's row pitch is the window + kS1Pad halves.  An A operand is one ds_read_b128 per plane: lane (n = lane & 15, kg =
// lane >> 4) reads 16 bytes of row n from position 8 kg.  The instruction is served in four groups of 16 lanes that are NOT
// the four kg - {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X_MICROARCH.md, LDS) - i.e. rows
// {0-3, 12-15} at kg and rows {4-11} at kg + 1.  With the pitch of round 4 (window + 8 halves = 4 x 37 dwords at radius
// 121) row n starts 5 n sixteen-byte slots into the 256-byte bank row, and three of the eight rows of the second set land
// on slots of the first: every group two LDS cycles instead of one (SQ_LDS_BANK_CONFLICT 40 % of SQ_LDS_IDX_ACTIVE, rounds
// 4 and 5).  A pitch of 4 p dwords with p = 2 (mod 4) puts rows {0-3, 12-15} on the even slots and rows {4-11}, one slot
// further, on the odd ones: window + 16 halves for every window of 32 NK columns, NK odd.  (The time did not move - the
// conflicts were not what the kernel waits for: profiles/r06_gauss_axis0_s1.txt, section 4.)
// (kS1Pad = 16: gauss_route.hpp, with the LDS sizes)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// 4 samples -> (x - c) / 4 -> f16 pairs (split8's arithmetic)
__device__ __forceinline__ void split4(const float (&x)[4], float mcq, f16x4& hi, f16x4& lo) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const f32x2 d = {__builtin_fmaf(x[2 * u], 0.25f, mcq), __builtin_fmaf(x[2 * u + 1], 0.25f, mcq)};
        const f32x2 hf = __builtin_bit_cast(f32x2, __builtin_bit_cast(u32x2, d) & u32x2{0xFFFFE000u, 0xFFFFE000u});
        const f32x2 r = {d[0] - hf[0], d[1] - hf[1]};
        const f16x2 hh = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(hf[0], hf[1]));  // exact: hf has 11 bits
        const f16x2 ll = __builtin_convertvector(r, f16x2);                                     // to nearest
        hi[2 * u] = hh[0];
        hi[2 * u + 1] = hh[1];
        lo[2 * u] = ll[0];
        lo[2 * u + 1] = ll[1];
    }
}

// the Toeplitz factor of 16 outputs for v_mfma_f32_16x16x32_f16: lane (n = lane & 15, kg = lane >> 4) of step s holds
// the taps that window position j = 32 s + 8 kg + q, q = 0 ... 7, has for output n of sub-tile m (outputs 16 m + n of a
// 32-output tile whose window starts Rp before it): tap index j - n - 16 m - (Rp - R)
template <int NK>
__device__ __forceinline__ void build_tap_blocks16(const float* taps, int R, float scale, int lane, int m, f16x8 (&hi)[NK], f16x8 (&lo)[NK]) {
    const int n = lane & 15, kg = lane >> 4, Rp = 16 * (NK - 1);
#pragma unroll
    for (int s = 0; s < NK; ++s) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = 32 * s + 8 * kg + q - n - 16 * m - (Rp - R);
            const float t = (k >= 0 && k <= 2 * R) ? taps[k] * scale : 0.0f;
            const _Float16 th = (_Float16)t;
            hi[s][q] = th;
            lo[s][q] = (_Float16)(t - (float)th);
        }
    }
}

// data pair (dh, dl) x the tap pairs of two sub-tiles that share it (axis 1: the data is the A operand), the cross
// product with the taps' low part first (f16_products' order), the two chains alternating
template <int NP>
__device__ __forceinline__ void f16_products16_pair(const f16x8& t0h, const f16x8& t0l, const f16x8& t1h, const f16x8& t1l, const f16x8& dh,
                                                    const f16x8& dl, f32x4& acc0, f32x4& acc1) {
    if (NP >= 4) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dl, t0l, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dl, t1l, acc1, 0, 0, 0);
    }
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dh, t0l, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dh, t1l, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dl, t0h, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dl, t1h, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dh, t0h, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(dh, t1h, acc1, 0, 0, 0);
}

// a value of lane 8 r (the first of the 8 lanes that load row r) to all 8 of them
__device__ __forceinline__ float octet_first(float v, int lane) {
    const int q = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x00 /* quad_perm [0,0,0,0] */, 0xf, 0xf, false);
    const int up = __builtin_amdgcn_mov_dpp(q, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    return __builtin_bit_cast(float, (lane & 4) ? up : q);
}

// Axis 1.  A wave owns a band of 16 rows and marches along x in tiles of 32 columns - two sub-tiles of 16, each with
// its own tap blocks, both fed by one read of the window (v_mfma_f32_16x16x32_f16: the rate of the 32 x 32 x 16 form per
// multiply-add).  The ring - hi[16][PITCH], lo[16][PITCH] in f16, PITCH = window + 8 - is half the size of a 32-row
// band's, so EIGHT waves fit a CU, two per SIMD: one wave alone leaves half of the matrix pipe idle (a 32 x 32 x 16
// MFMA every 32 cycles from one wave, every 16 from two: tools/ubench/mfma_valu_overlap.hip) and hides at most 4
// vector instructions under each.  Window of the tile at x0: [x0 - Rp, x0 + 32 + Rp) = 32 NK columns, Rp = 16 (NK - 1)
// >= R.  The loader takes the 32 columns a tile adds two tiles ahead: lane -> rows (lane >> 3) and + 8, columns
// 4 (lane & 7) ...: 16-byte loads, 8 rows x 128 B per instruction.  The 32 columns lie in one slab; a slab starts
// with them when they start on a multiple of 64.  LDS: 8 x (ring + references of 8 slabs x 16 rows) + the table W.
// Flags: one byte per 16 x 32 tile, [band][tile]; the repair pass takes the two of a 32 x 32 unit together.
template <int NK, int NP>
__global__ __launch_bounds__(512) void gauss_axis1_s1_kernel(GaussArgs p, int rows, int nseg) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    constexpr int Rp = 16 * (NK - 1), RC = 32 * NK, PITCH = RC + kS1Pad, NSIDE = (Rp + 63) / 64;
    constexpr int kStay = NK;                         // tiles whose window holds a group of 32 columns
    constexpr int kWaveFloats = 16 * PITCH + 8 * 16;  // two f16 planes = 16 x PITCH floats, then the references
    static_assert(NSIDE <= 2 && Rp % 32 == 0, "at most 5 slabs per window; groups of 32 columns inside one slab");
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int R = p.radius;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* const wlds = L + 8 * kWaveFloats;  // W[5][64]
    for (int k = threadIdx.x; k < 5 * 64; k += 512) wlds[k] = p.wtab[k];
    __syncthreads();
    _Float16* const hi = reinterpret_cast<_Float16*>(L + wave * kWaveFloats);
    _Float16* const lo = hi + 16 * PITCH;
    float* const ctab = L + wave * kWaveFloats + 16 * PITCH;  // [8 slabs][16 rows]
    const int gw = blockIdx.x * 8 + wave;
    const int band = gw / nseg, seg = gw - band * nseg;
    const int r0 = band * 16;
    if (r0 >= rows) return;
    if (p.run_if && *p.run_if == 0) return;
    const int ntile = (p.nx + 31) / 32;
    const int tper = (ntile + nseg - 1) / nseg;
    const int t_first = seg * tper, t_last = min(t_first + tper, ntile);
    if (t_first >= t_last) return;
    f16x8 t0h[NK], t0l[NK], t1h[NK], t1l[NK];
    build_tap_blocks16<NK>(p.taps, R, p.tap_scale, lane, 0, t0h, t0l);
    build_tap_blocks16<NK>(p.taps, R, p.tap_scale, lane, 1, t1h, t1l);
    const bool full_band = r0 + 16 <= rows;
    const int lr = lane >> 3, lc = 4 * (lane & 7);  // loader: rows lr and lr + 8 of the band, 4 columns from lc of the group
    const float* const lrow0 = p.in + (size_t)min(r0 + lr, rows - 1) * p.nx;
    const float* const lrow1 = p.in + (size_t)min(r0 + lr + 8, rows - 1) * p.nx;
    struct Pre {
        f4 a, b;  // rows lr, lr + 8
    };
    auto load = [&](int col0) {
        Pre v;
        const int col = col0 + lc;
        if (col0 >= 0 && col0 + 32 <= p.nx) {
            v.a = *reinterpret_cast<const f4*>(lrow0 + col);
            v.b = *reinterpret_cast<const f4*>(lrow1 + col);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cx = reflect_index(col + e, p.nx);
                v.a[e] = lrow0[cx];
                v.b[e] = lrow1[cx];
            }
        }
        return v;
    };
    // the 32 columns from `col0` (a multiple of 32) into the ring at `slot`; c_old: the references of their slab for
    // the lane's two rows as the table has them (read ahead of time; not used when the slab starts here)
    auto stage = [&](const Pre& v, int col0, int slot, float c_old0, float c_old1, bool& bad, bool& ref_bad) {
        float x0[4], x1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool w0 = wild(v.a[e]), w1 = wild(v.b[e]);
            bad |= w0 | w1;
            x0[e] = w0 ? 0.0f : v.a[e];
            x1[e] = w1 ? 0.0f : v.b[e];
        }
        float c0 = c_old0, c1 = c_old1;
        if ((col0 & 63) == 0) {  // (wave-uniform) the slab's first column: lane & 7 == 0 of every row holds its reference
            ref_bad |= (lane & 7) == 0 && (wild(v.a[0]) || wild(v.b[0]));
            c0 = octet_first(x0[0], lane);
            c1 = octet_first(x1[0], lane);
            if ((lane & 7) == 0) {
                ctab[(floor_div64(col0) & 7) * 16 + lr] = c0;
                ctab[(floor_div64(col0) & 7) * 16 + lr + 8] = c1;
            }
        }
        f16x4 dh, dl;
        split4(x0, -0.25f * c0, dh, dl);
        *reinterpret_cast<f16x4*>(hi + lr * PITCH + slot + lc) = dh;
        *reinterpret_cast<f16x4*>(lo + lr * PITCH + slot + lc) = dl;
        split4(x1, -0.25f * c1, dh, dl);
        *reinterpret_cast<f16x4*>(hi + (lr + 8) * PITCH + slot + lc) = dh;
        *reinterpret_cast<f16x4*>(lo + (lr + 8) * PITCH + slot + lc) = dl;
    };
    // The bands do not walk the row in step: band b's tile order is turned by turn_b tiles (tile = (position + turn_b) mod
    // ntile), so its runs start somewhere else than its neighbours' and the one run that meets the end of the row goes
    // on at its start (a second run-in for that run).  In step, all bands of the DEM sit on the same columns at the
    // same time, 2^17 bytes apart on a 32768-wide DEM, and whether HBM's channels then collide depends on the physical
    // pages: the + 30 ... 45 % slow mode most processes show on some boxes (profiles/r04_pitch_spread.txt; axis 1 alone at
    // sigma 13 / 20: 1.66 / 1.86 ms or 2.40 / 2.43 ms in step, 1.79 / 1.88 ms turned).
    const int run_len = t_last - t_first;
    const int turn = p.group0 != 0 && ntile >= 64 ? (int)(((unsigned)band * 40503u) % (unsigned)ntile) : 0;
    const int run_first = (t_first + turn) % ntile;
    for (int part = 0; part < 2; ++part) {
    const int t_first = part == 0 ? run_first : 0;
    const int t_last = part == 0 ? min(run_first + run_len, ntile) : run_first + run_len - ntile;
    if (t_first >= t_last) continue;
    unsigned ref_wild = 0;  // slabs (slot bits) whose reference column holds a sample that is not a plain finite one
    int last_wild = kNoWild;
    const int x_start = t_first * 32 - Rp;
    {
        ctab[lane] = 0.0f;
        ctab[64 + lane] = 0.0f;
        __builtin_amdgcn_wave_barrier();
        // the references of the slabs the first window holds: the first one may start left of the window (the others are
        // written again, with the same value, when their first column is staged)
        unsigned used = 0;
        for (int s = floor_div64(x_start); s <= floor_div64(x_start + RC - 1); ++s) {
            const int cx = reflect_index(64 * s, p.nx);
            const float v0 = lrow0[cx], v1 = lrow1[cx];
            const bool w0 = wild(v0), w1 = wild(v1);
            if ((lane & 7) == 0) {
                ctab[(s & 7) * 16 + lr] = w0 ? 0.0f : v0;
                ctab[(s & 7) * 16 + lr + 8] = w1 ? 0.0f : v1;
            }
            if (__builtin_amdgcn_ballot_w64(w0 | w1)) ref_wild |= 1u << (s & 7);
            used |= 1u << (s & 7);
        }
        __builtin_amdgcn_wave_barrier();
        bool bad = false, ref_bad = false;  // (ref_bad: covered by the loop above)
        for (int k0 = 0; k0 < RC; k0 += 96) {  // three groups in flight
            Pre v[3];
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (k0 + 32 * u < RC) v[u] = load(x_start + k0 + 32 * u);
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (k0 + 32 * u < RC) {
                    const int col0 = x_start + k0 + 32 * u, sl = (floor_div64(col0) & 7) * 16;
                    stage(v[u], col0, k0 + 32 * u, ctab[sl + lr], ctab[sl + lr + 8], bad, ref_bad);
                }
        }
        if (__builtin_amdgcn_ballot_w64(bad) || (ref_wild & used)) last_wild = t_first + kStay - 1;
    }
    int base = 0;  // ring column of input column x0 - Rp
    const int n = lane & 15, kg = lane >> 4;
    const unsigned out_lane_off = (unsigned)(4 * kg * p.nx + n) * 4u;  // D: column n, rows 4 kg + v
    const _Float16* const ah = hi + n * PITCH + 8 * kg;  // A: row n of the band, 8 window positions from 8 kg
    const _Float16* const al = lo + n * PITCH + 8 * kg;
    // The columns tile t + 1 adds are loaded while tile t - 1 is computed and staged behind tile t: two register sets
    // that swap roles from tile to tile (the loop below takes two tiles per turn, so nothing is copied and nothing
    // waits for a load before its data is due).
    Pre pre_a, pre_b;
    if (t_first + 1 < t_last) pre_a = load(x_start + RC);
    auto tile = [&](const int t, const Pre& pre, Pre& pre_next) {
        const int x0 = t * 32;
        const bool more = t + 1 < t_last;
        const int n0 = x0 - Rp + RC;  // the 32 columns the next tile adds
        if (t + 2 < t_last) pre_next = load(n0 + 32);
        float c_n0 = 0.0f, c_n1 = 0.0f;
        if (more) {
            const int sl = (floor_div64(n0) & 7) * 16;
            c_n0 = ctab[sl + lr];
            c_n1 = ctab[sl + lr + 8];
        }
        // the correction (ahead of the products: nothing waits on LDS behind them): the other slabs' references against
        // the tile's own.  D: column n, rows 4 kg + v
        const int b = x0 >> 6, o = (x0 & 63) + n;
        const f4 cb = *reinterpret_cast<const f4*>(ctab + (b & 7) * 16 + 4 * kg);
        f4 corr0 = {0.0f, 0.0f, 0.0f, 0.0f}, corr1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int d = -NSIDE; d <= NSIDE; ++d) {
            if (d == 0) continue;
            const float w0 = wlds[(d + 2) * 64 + o], w1 = wlds[(d + 2) * 64 + o + 16];
            const f4 cs = *reinterpret_cast<const f4*>(ctab + ((b + d) & 7) * 16 + 4 * kg);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dlt = cs[e] - cb[e];
                corr0[e] = fmaf(dlt, w0, corr0[e]);
                corr1[e] = fmaf(dlt, w1, corr1[e]);
            }
        }
        f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
        int slot = base;
        f16x8 bh[3], bl[3];
        auto fetch = [&](int k) {
            bh[k] = *reinterpret_cast<const f16x8*>(ah + slot);
            bl[k] = *reinterpret_cast<const f16x8*>(al + slot);
            slot += 32;
            slot = slot >= RC ? slot - RC : slot;
        };
        fetch(0);
        fetch(1);
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            if (s + 2 < NK) fetch((s + 2) % 3);
            __builtin_amdgcn_sched_barrier(0);
            f16_products16_pair<NP>(t0h[s], t0l[s], t1h[s], t1l[s], bh[s % 3], bl[s % 3], acc0, acc1);
        }
        {
            const int ox = x0 + n;
            if (full_band && x0 + 32 <= p.nx) {  // (wave-uniform) every row and both sub-tiles: one base, immediate offsets
                char* ub = reinterpret_cast<char*>(p.out + (size_t)r0 * p.nx + x0) + out_lane_off;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float* o0 = reinterpret_cast<float*>(ub + (size_t)v * p.nx * 4);
                    o0[0] = fmaf(acc0[v], p.out_scale, corr0[v]) + cb[v];
                    o0[16] = fmaf(acc1[v], p.out_scale, corr1[v]) + cb[v];
                }
            } else {
                float* o0 = p.out + (size_t)(r0 + 4 * kg) * p.nx + ox;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (full_band || r0 + 4 * kg + v < rows) {
                        if (ox < p.nx) o0[(size_t)v * p.nx] = fmaf(acc0[v], p.out_scale, corr0[v]) + cb[v];
                        if (ox + 16 < p.nx) o0[(size_t)v * p.nx + 16] = fmaf(acc1[v], p.out_scale, corr1[v]) + cb[v];
                    }
            }
        }
        if (lane == 0) p.flags[(size_t)band * ntile + t] = last_wild >= t ? 1 : 0;
        if (more) {
            bool bad = false, ref_bad = false;
            stage(pre, n0, base, c_n0, c_n1, bad, ref_bad);  // over the oldest 32 columns
            if ((n0 & 63) == 0) {  // the slab that starts here takes over the slot of the slab 8 before it
                if (__builtin_amdgcn_ballot_w64(ref_bad)) ref_wild |= 1u << (floor_div64(n0) & 7);
                else ref_wild &= ~(1u << (floor_div64(n0) & 7));
            }
            if (__builtin_amdgcn_ballot_w64(bad) || (ref_wild & (1u << (floor_div64(n0) & 7)))) last_wild = t + kStay;
        }
        base += 32;
        base = base >= RC ? base - RC : base;
    };
    for (int t = t_first; t < t_last; t += 2) {
        tile(t, pre_a, pre_b);
        if (t + 1 < t_last) tile(t + 1, pre_b, pre_a);
    }
    }
}

// Both passes of a short isotropic filter (radius 4 ... 16: 4 steps of 16 taps per 32-output tile) in ONE kernel:
// the intermediate plane (4 B written + 4 B read per pixel out of 16) stays in LDS.  A block owns 4 bands of 32
// rows (global multiples of 32) and marches along x in blocks of 64 columns.  Per step: the block's 160 raw rows
// (its 128 + 16 above and below) x 64 columns come in through a double buffer; every wave forms the axis-0 product
// for its band - the arithmetic of gauss_axis0_f16_kernel<4, ., 1>, tile for tile: same rows, same offset (the
// column's sample 16 rows into the band), same steps - rounds it to float32 like the stored intermediate, and puts
// the 32 x 64 block into its own ring of 96 columns; then it takes the 64-column output tile whose window the block
// completes with the arithmetic of gauss_axis1_f16_kernel<4, ., 2, .>.  An output therefore has the bits of the two
// kernels (tests/test_gpu_parity.py::test_gaussian_fused_is_the_two_passes).  The raw blocks sit 16 columns to the
// right of the tile grid, so block u completes the window of tile u; columns beyond the DEM are the reflected
// columns (the axis-0 result of a reflected column is that column's).  Rows are read 160 / 128 times, not twice.
// A sample that is not a plain finite one is staged as 0 and raises *wild_flag: the launcher has queued the two-pass
// kernels behind this one with run_if = wild_flag, and they (with their repair passes) redo the whole plane then.
// (S = 6, radius 17 ... 32: raw blocks of 32 columns - 192 rows of them, twice, plus four rings of 128 columns are
// 117 KB - two per output tile, two run-in blocks.)
template <int NP, int S, int CW>
__global__ __launch_bounds__(256) void gauss_fused_f16_kernel(GaussArgs p, int tile_first, int ntile_rows, int nseg) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    constexpr int Rp = 8 * (S - 2), RAWR = 128 + 2 * Rp, NS = S + 2, RC = 16 * NS, pitch = RC + 4;
    constexpr int BPT = 64 / CW;                  // raw blocks per 64-column output tile
    constexpr int TPR = CW / 4, RPP = 256 / TPR;  // loader: threads per raw row, rows per pass
    constexpr int NPASS = RAWR / RPP;
    static_assert(RAWR % RPP == 0 && (CW == 32 || CW == 64), "loader geometry");
    const int R = p.radius;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, g = lane >> 5;
    float* const rawbuf = L;  // 2 x [RAWR][CW]
    float* const ring = L + 2 * RAWR * CW + wave * (32 * pitch + 32);
    float* const crow = ring + 32 * pitch;
    f16x8 twh[S], twl[S];
    build_tap_blocks<S>(p.taps, R, p.tap_scale, lane, twh, twl);
    const int y_blk = (tile_first + 4 * (int)blockIdx.y) * 32;  // global row of the block's first band
    const int y_band = y_blk + 32 * wave;
    const bool band_on = 4 * (int)blockIdx.y + wave < ntile_rows;
    const int ntile = (p.nx + 63) / 64;
    const int tper = (ntile + nseg - 1) / nseg;
    const int seg_first = blockIdx.x * tper, seg_last = min(seg_first + tper, ntile);
    if (seg_first >= seg_last) return;
    const int row_lo = max(0, p.in_row0), row_hi = min(p.gny, p.in_row0 + p.in_rows);
    const bool rows_inside = y_blk - Rp >= row_lo && y_blk + 128 + Rp <= row_hi;
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int lr = threadIdx.x / TPR, lcq = (threadIdx.x % TPR) * 4;
    // raw block u: columns CW u + Rp ... (the blocks sit Rp columns to the right of the tile grid, so the last block
    // of a tile completes its window)
    auto load_raw = [&](int u, f4 (&pre)[NPASS]) {
        const int xb = CW * u + Rp;
        if (rows_inside && xb >= 0 && xb + CW <= p.nx) {
            const float* rbp = p.in + (size_t)(y_blk - Rp + lr - p.in_row0) * p.nx + xb + lcq;
#pragma unroll
            for (int q = 0; q < NPASS; ++q) pre[q] = *reinterpret_cast<const f4*>(rbp + (size_t)(RPP * q) * p.nx);
        } else {
#pragma unroll
            for (int q = 0; q < NPASS; ++q) {
                int gy = reflect_index(y_blk - Rp + RPP * q + lr, p.gny);
                gy = min(max(gy, p.in_row0), p.in_row0 + p.in_rows - 1);
                const float* rowp = p.in + (size_t)(gy - p.in_row0) * p.nx;
#pragma unroll
                for (int e = 0; e < 4; ++e) pre[q][e] = rowp[reflect_index(xb + lcq + e, p.nx)];
            }
        }
    };
    auto store_raw = [&](f4 (&pre)[NPASS], float* dst) {
        bool bad = false;
#pragma unroll
        for (int q = 0; q < NPASS; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= wild(pre[q][e]);
        if (__builtin_amdgcn_ballot_w64(bad)) {
#pragma unroll
            for (int q = 0; q < NPASS; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) pre[q][e] = wild(pre[q][e]) ? 0.0f : pre[q][e];
            if (lane == 0) {
                *p.wild_flag = 1;
                if (p.wild_host) __hip_atomic_store(p.wild_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
#pragma unroll
        for (int q = 0; q < NPASS; ++q) *reinterpret_cast<f4*>(dst + (RPP * q + lr) * CW + lcq) = pre[q];
    };
    const f32x2 quarter = {0.25f, 0.25f};
    const unsigned out_lane_off = (unsigned)(4 * g * p.nx + i) * 4u;
    const bool full_band = y_band >= p.out_row0 && y_band + 32 <= p.out_row0 + p.out_rows;
    // The row blocks do not walk the DEM in step (gauss_axis1_s1_kernel has the reasons): row block y's tile order is turned
    // by a number of tiles of its own, and the run that meets the end of the row goes on at its start (a second run-in).
    const int turn = p.group0 != 0 && ntile >= 32 ? (int)(((unsigned)blockIdx.y * 40503u) % (unsigned)ntile) : 0;
    const int run_first = (seg_first + turn) % ntile, run_len = seg_last - seg_first;
    for (int part = 0; part < 2; ++part) {
    const int t_first = part == 0 ? run_first : 0;
    const int t_last = part == 0 ? min(run_first + run_len, ntile) : run_first + run_len - ntile;
    if (t_first >= t_last) continue;
    const int u0 = BPT * t_first;                       // first block of the first tile
    const int u_start = u0 - (2 * Rp + CW - 1) / CW;    // run-in: the 2 Rp columns left of it
    const int u_last = BPT * t_last - 1;
    {
        f4 pre[NPASS];
        load_raw(u_start, pre);
        store_raw(pre, rawbuf);
    }
    __syncthreads();
    int cur = 0;
    int rb = 0;                                   // ring column of the window of the next output tile (global column 64 t - Rp)
    int rel = CW * (u_start - u0) + 2 * Rp;       // column of block u relative to the first tile's window (may start below 0)
    for (int u = u_start; u <= u_last; ++u) {
        f4 pre[NPASS];
        const bool more = u < u_last;
        if (more) load_raw(u + 1, pre);
        const bool tile_done = u >= u0 && (u + 1) % BPT == 0;
        if (band_on) {
            // ---- axis 0: the band's 32 rows of raw block u -> ring ----
            const float* raw = rawbuf + cur * (RAWR * CW);
#pragma unroll
            for (int nt = 0; nt < CW / 32; ++nt) {
                if (rel + 32 * nt < 0) continue;  // (run-in of S = 4: only the second half of the block is in the window)
                const int col = 32 * nt + i;
                const float c0 = raw[(32 * wave + Rp + 16) * CW + col];
                const f32x2 mcq = {-0.25f * c0, -0.25f * c0};
                f32x16 acc;
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
                const float* bl = raw + (32 * wave + 8 * g) * CW + col;
                float xa[8], xb[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) xa[q] = bl[q * CW];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    f16x8 dh, dl;
                    // the next step's samples are on their way while this step's are split (as in the two-pass kernels)
                    if (s & 1) {
                        if (s + 1 < S) {
#pragma unroll
                            for (int q = 0; q < 8; ++q) xa[q] = bl[(16 * (s + 1) + q) * CW];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        split8(xb, quarter, mcq, dh, dl);
                    } else {
                        if (s + 1 < S) {
#pragma unroll
                            for (int q = 0; q < 8; ++q) xb[q] = bl[(16 * (s + 1) + q) * CW];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        split8(xa, quarter, mcq, dh, dl);
                    }
                    f16_products<false, NP>(twh[s], twl[s], dh, dl, acc);
                }
                int wc = (rel + 32 * nt) % RC;
#pragma unroll
                for (int v = 0; v < 16; ++v) ring[((v & 3) + 8 * (v >> 2) + 4 * g) * pitch + wc + i] = fmaf(acc[v], p.out_scale, c0);
            }
            // ---- axis 1: the output tile this block completes, columns 64 t ... 64 t + 63 ----
            if (tile_done) {
                const int x0 = 64 * ((u + 1) / BPT - 1);
                int sc = rb + Rp + 32;
                sc = sc >= RC ? sc - RC : sc;
                const float c = ring[i * pitch + sc];
                if (g == 0) crow[i] = c;
                const f32x2 mcq = {-0.25f * c, -0.25f * c};
                f32x16 acc[2];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[m][v] = 0.0f;
                const float* const al = ring + i * pitch + 8 * g;
                int slot = rb;
                auto fetch = [&](float (&x)[8]) {
                    const f4 lo4 = *reinterpret_cast<const f4*>(al + slot), hi4 = *reinterpret_cast<const f4*>(al + slot + 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        x[q] = lo4[q];
                        x[4 + q] = hi4[q];
                    }
                    slot += 16;
                    slot = slot >= RC ? slot - RC : slot;
                };
                float xa[8], xb[8];
                fetch(xa);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    f16x8 dh, dl;
                    if (s & 1) {
                        if (s + 1 < NS) fetch(xa);
                        __builtin_amdgcn_sched_barrier(0);
                        split8(xb, quarter, mcq, dh, dl);
                    } else {
                        if (s + 1 < NS) fetch(xb);
                        __builtin_amdgcn_sched_barrier(0);
                        split8(xa, quarter, mcq, dh, dl);
                    }
#pragma unroll
                    for (int m = 0; m < 2; ++m)
                        if (s - 2 * m >= 0 && s - 2 * m < S) f16_products<true, NP>(twh[s - 2 * m], twl[s - 2 * m], dh, dl, acc[m]);
                }
                float cr[16];
#pragma unroll
                for (int v = 0; v < 16; ++v) cr[v] = crow[(v & 3) + 8 * (v >> 2) + 4 * g];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int xm = x0 + 32 * m, ox = xm + i;
                    if (ox < p.nx) {
                        if (full_band) {
                            char* ub = reinterpret_cast<char*>(p.out + (size_t)(y_band - p.out_row0) * p.nx + xm);
#pragma unroll
                            for (int v = 0; v < 16; ++v)
                                *reinterpret_cast<float*>(ub + (size_t)((v & 3) + 8 * (v >> 2)) * p.nx * 4 + out_lane_off) = fmaf(acc[m][v], p.out_scale, cr[v]);
                        } else {
#pragma unroll
                            for (int v = 0; v < 16; ++v) {
                                const int oy = y_band + (v & 3) + 8 * (v >> 2) + 4 * g;
                                if (oy >= p.out_row0 && oy < p.out_row0 + p.out_rows) p.out[(size_t)(oy - p.out_row0) * p.nx + ox] = fmaf(acc[m][v], p.out_scale, cr[v]);
                            }
                        }
                    }
                }
            }
        }
        if (tile_done) {
            rb += 64;
            rb = rb >= RC ? rb - RC : rb;
        }
        rel += CW;
        if (rel >= 64 * RC) rel -= 63 * RC;  // (kept small; only rel % RC and its sign before the first tile matter)
        if (more) store_raw(pre, rawbuf + (cur ^ 1) * (RAWR * CW));
        __syncthreads();
        cur ^= 1;
    }
    }
}

// Repair pass of the f16 route: the outputs of a marked tile whose own window holds a sample that is not a plain
// finite one (non-finite, or |x| > 1e5) are taken tap by tap in float32 - an ascending chain of fused multiply-adds
// on x - c, c the tile's offset - so they are NaN / inf exactly where the reference's are; every other output
// keeps what the matrix cores gave it.
template <bool AXIS1>
__global__ __launch_bounds__(64) void gauss_f16_repair_kernel(GaussArgs p, int units_a, int units_b, int first_a, int rows_plane) {
    if (p.run_if && *p.run_if == 0) return;
    const int lane = threadIdx.x;
    const long units = (long)units_a * units_b;
    const int R = p.radius;
    // A lane takes 16 consecutive outputs along the filter axis.  `at(m)`: the sample m places after the first
    // output's window start (so output k owns at(k) ... at(k + 2 R), its own sample is at(k + R)).  The marks are
    // conservative and a marked tile is mostly clean windows, or mostly NaN (a sea): the lane first COUNTS the samples
    // of the first window that are not plain finite ones (loads 8 at a time, nothing depends on them), then slides
    // the count from output to output (one sample in, one out) and runs the float32 chain - left at the first NaN -
    // only where the count is not 0.  (The first version ran 16 full chains of dependent loads per lane: 8192^2 with
    // a NaN third at sigma 30.25 took 135 ms instead of 0.45; now ~1 ms.)
    auto sixteen = [&](auto at, float c, auto dst, auto wanted) {
        // (deep in a NaN sea every output is NaN by its own sample: 16 loads in flight settle the lane)
        float own[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) own[k] = at(k + R);
        bool all_nan = true;
#pragma unroll
        for (int k = 0; k < 16; ++k) all_nan = all_nan && __builtin_isnan(own[k]);
        if (all_nan) {
            for (int k = 0; k < 16; ++k)
                if (wanted(k)) *dst(k) = __builtin_nanf("");
            return;
        }
        int cnt = 0;
        for (int m0 = 0; m0 <= 2 * R; m0 += 8) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = m0 + e <= 2 * R ? at(m0 + e) : 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) cnt += wild(v[e]) ? 1 : 0;
        }
        for (int k = 0; k < 16; ++k) {
            if (cnt != 0 && wanted(k)) {
                float acc = 0.0f;
                bool nan = false;
                for (int q = 0; q <= 2 * R; ++q) {
                    const float v = at(k + q);
                    if (__builtin_isnan(v)) {
                        nan = true;
                        break;
                    }
                    acc = fmaf(p.taps[q], v - c, acc);
                }
                *dst(k) = nan ? __builtin_nanf("") : c + acc;
            }
            if (k < 15) cnt += (wild(at(k + 2 * R + 1)) ? 1 : 0) - (wild(at(k)) ? 1 : 0);
        }
    };
    for (long base = (long)blockIdx.x * 64; base < units; base += (long)gridDim.x * 64) {
        const long mine = base + lane;
        bool mark = false;
        if (mine < units) {
            if (p.fine_cols == 0) {
                mark = p.flags[mine] != 0;
            } else {  // the two 16-row bands of the unit
                const int fa = (int)(mine / units_b) * 2, fb = (int)(mine % units_b);
                mark = p.flags[(size_t)fa * p.fine_cols + fb] != 0 || (fa + 1 < p.fine_rows && p.flags[(size_t)(fa + 1) * p.fine_cols + fb] != 0);
            }
        }
        unsigned long long marked = __builtin_amdgcn_ballot_w64(mark);
        while (marked) {
            const int bit = __builtin_ctzll(marked);
            marked &= marked - 1;
            const long u = base + bit;
            const int a = (int)(u / units_b), b = (int)(u % units_b);
            const int j = lane & 31, h = lane >> 5;
            if (!AXIS1) {
                const int y0 = (first_a + a) * 32, x = 32 * b + j;
                if (x >= p.nx) continue;
                auto in_at = [&](int gy) {
                    gy = reflect_index(gy, p.gny);
                    gy = min(max(gy, p.in_row0), p.in_row0 + p.in_rows - 1);
                    return p.in[(size_t)(gy - p.in_row0) * p.nx + x];
                };
                float c = in_at(y0 + 16);
                c = wild(c) ? 0.0f : c;
                const int oy0 = y0 + 16 * h;  // first output row of this lane
                const int row_lo = max(0, p.in_row0), row_hi = min(p.gny, p.in_row0 + p.in_rows);
                auto dst = [&](int k) { return p.out + (size_t)(oy0 + k - p.out_row0) * p.nx + x; };
                auto wanted = [&](int k) { return oy0 + k >= p.out_row0 && oy0 + k < p.out_row0 + p.out_rows; };
                if (oy0 - R >= row_lo && oy0 + 16 + R < row_hi) {  // every window inside the block: a pointer and a stride
                    const float* w0 = p.in + (size_t)(oy0 - R - p.in_row0) * p.nx + x;
                    const size_t nx = (size_t)p.nx;
                    sixteen([&](int m) { return w0[(size_t)m * nx]; }, c, dst, wanted);
                } else {
                    sixteen([&](int m) { return in_at(oy0 - R + m); }, c, dst, wanted);
                }
            } else {
                const int r = 32 * a + j, x0 = 32 * b + 16 * h;  // first output column of this lane
                if (r >= rows_plane) continue;
                const float* row = p.in + (size_t)r * p.nx;
                float c = row[reflect_index(32 * b + 16, p.nx)];
                c = wild(c) ? 0.0f : c;
                auto dst = [&](int k) { return p.out + (size_t)r * p.nx + x0 + k; };
                auto wanted = [&](int k) { return x0 + k < p.nx; };
                if (x0 - R >= 0 && x0 + 16 + R < p.nx) {
                    const float* w0 = row + x0 - R;
                    sixteen([&](int m) { return w0[m]; }, c, dst, wanted);
                } else {
                    sixteen([&](int m) { return row[reflect_index(x0 - R + m, p.nx)]; }, c, dst, wanted);
                }
            }
        }
    }
}

// ---- host side -----------------------------------------------------------------------------
// repair passes: one wave per block; enough blocks to fill the chip when many tiles are marked (a DEM with a NaN sea),
// a short scan of the marks when none is
constexpr long kRepairBlocks = 8192;
template <bool AXIS1>
int launch_repair(const GaussArgs& a, int units_a, int units_b, int first_a, int rows_plane) {
    const long units = (long)units_a * units_b;
    return launch(gauss_f16_repair_kernel<AXIS1>, dim3((unsigned)std::min<long>(kRepairBlocks, (units + 63) / 64)), dim3(64), 0,
                  ctx().compute, a, units_a, units_b, first_a, rows_plane);
}

// ---- f16 route: scales, dispatch over the step count ----
#ifndef TOPO_F16_NP
#define TOPO_F16_NP 3  // products per tap block: th h + tm h + th l (4 adds tm l: 7 % slower, same error; lab builds)
#endif
void set_f16_scales(double sigma, GaussArgs* a) {
    const float peak = (float)(1.0 / gauss_taps(sigma));  // the largest tap, as upload_weights rounds it
    const int e = 9 - std::ilogb(peak);                    // peak 2^e in [512, 1024)
    a->tap_scale = std::ldexp(1.0f, e);
    a->out_scale = std::ldexp(1.0f, 2 - e);  // the data goes in divided by 4
}
int no_f16_kernel() {
    set_error("gaussian (f16 matrix-core route): no kernel for this radius");
    return TOPO_AMD_EUNSUP;
}
// f(S, MT) with the step count and the tiles per offset of a tile kernel as compile-time constants (either axis)
template <class F>
int with_f16_tile(int steps, int mt, F f) {
    switch (steps) {
#define TOPO_F16_CASE(S_) case S_: return mt == 2 ? f(Int<S_>{}, Int<2>{}) : f(Int<S_>{}, Int<1>{});
        TOPO_F16_CASE(4) TOPO_F16_CASE(6) TOPO_F16_CASE(8) TOPO_F16_CASE(10) TOPO_F16_CASE(12) TOPO_F16_CASE(14) TOPO_F16_CASE(16) TOPO_F16_CASE(18)
#undef TOPO_F16_CASE
    }
    return no_f16_kernel();
}
int launch_f16_axis0_any(int steps, int mt, dim3 grid, const GaussArgs& a, int tile_first, int ntiles, int per) {
    return with_f16_tile(steps, mt, [&](auto S, auto MT) {
        if constexpr (f16_axis0_built(S(), MT()))
            return launch_big_lds<gauss_axis0_f16_kernel<S(), TOPO_F16_NP, MT()>>(grid, dim3(256), f16_axis0_lds(S(), MT()), a, tile_first, ntiles, per);
        else
            return no_f16_kernel();
    });
}
int launch_f16_axis1_any(int steps, int mt, long waves, const GaussArgs& a, int rows, int nseg) {
    constexpr int NW = kF16Axis1Waves;
    return with_f16_tile(steps, mt, [&](auto S, auto MT) {
        if constexpr (f16_axis1_built(S(), MT()))
            return launch_big_lds<gauss_axis1_f16_kernel<S(), TOPO_F16_NP, MT(), NW>>(dim3((unsigned)((waves + NW - 1) / NW)), dim3(64 * NW),
                                                                                      f16_axis1_lds(S(), MT()), a, rows, nseg);
        else
            return no_f16_kernel();
    });
}
static_assert(s1_axis1_lds(9) <= kLdsMax, "the widest ring fits LDS");
int launch_s1_axis1_any(int nk, long waves, const GaussArgs& a, int rows, int nseg) {
    const dim3 grid((unsigned)((waves + 7) / 8));
    switch (nk) {
        case 5: return launch_big_lds<gauss_axis1_s1_kernel<5, TOPO_F16_NP>>(grid, dim3(512), s1_axis1_lds(5), a, rows, nseg);
        case 7: return launch_big_lds<gauss_axis1_s1_kernel<7, TOPO_F16_NP>>(grid, dim3(512), s1_axis1_lds(7), a, rows, nseg);
        case 9: return launch_big_lds<gauss_axis1_s1_kernel<9, TOPO_F16_NP>>(grid, dim3(512), s1_axis1_lds(9), a, rows, nseg);
    }
    set_error("gaussian (split-once matrix-core route): no kernel for this radius");
    return TOPO_AMD_EUNSUP;
}

// axis 1 on the split-once route: bands of 16 rows, tiles of 32 columns, one flag byte per tile
int run_axis1_s1(GaussArgs a, int rows, int nx) {
    Context& c = ctx();
    const int nk = s1_steps(a.radius);
    t_grad.s1_steps = nk;
    const int bands = (rows + 15) / 16, ntile = (nx + 31) / 32;
    // one block of 8 waves per CU; runs no shorter than 512 columns
    const int nseg = run_cut(bands, ntile, ntile / 16, 8L * c.num_cu, nk);
    const long waves = (long)bands * nseg;
    void* flags = nullptr;
    TOPO_TRY(workspace(10, (size_t)bands * ntile, &flags));
    a.flags = (unsigned char*)flags;
    a.fine_rows = bands;
    a.fine_cols = ntile;
    TOPO_TRY(launch_s1_axis1_any(nk, waves, a, rows, nseg));
    return launch_repair<true>(a, (rows + 31) / 32, (nx + 31) / 32, 0, rows);
}

// ---- one kernel for both passes (radius 4 ... 31, the gradient to 47; one sigma) ----
template <int S>
int launch_fused_f16(dim3 grid, const GaussArgs& a, int tile_first, int ntile_rows, int nseg) {
    constexpr int CW = fused_block_cols(S);
    return launch_big_lds<gauss_fused_f16_kernel<TOPO_F16_NP, S, CW>>(grid, dim3(256), fused_lds(S, CW), a, tile_first, ntile_rows, nseg);
}
// *flag_out == nullptr on entry: the launch gets a flag of its own, cleared here.  Otherwise it raises the caller's flag
// (the chunked gradient clears one flag per call and queues the two-pass route behind all of its chunks).
int run_fused_f16(const Block& b, double sigma, float* out, int table_slot, const int** flag_out) {
    Context& c = ctx();
    GaussArgs a;
    TOPO_TRY(gauss_args(b, out, sigma, 1, table_slot, &a));
    a.group0 = 1;  // (as on axis 1)
    set_f16_scales(sigma, &a);
    if (*flag_out == nullptr) {
        void* flag = nullptr;
        TOPO_TRY(workspace(11, 64, &flag));
        TOPO_HIP(hipMemsetAsync(flag, 0, sizeof(int), c.compute));
        *flag_out = (const int*)flag;
    }
    a.wild_flag = const_cast<int*>(*flag_out);
    a.wild_host = dem_memo_wild_word(b);
    t_grad.fused_steps = f16_steps(a.radius);
    const int tile_first = b.out_row0 / 32;
    const int ntile_rows = (b.out_row0 + b.out_rows - 1) / 32 - tile_first + 1;
    const int row_blocks = (ntile_rows + 3) / 4;
    const int ntile = (b.nx + 63) / 64;
    const int nseg = run_cut(row_blocks, ntile, ntile / 4, c.num_cu, 1);  // one block per CU (the LDS)
    TOPO_TRY(check_grid_rows(row_blocks, "gaussian (fused matrix-core kernel)"));
    const dim3 grid(nseg, row_blocks);
    if (f16_steps(a.radius) == 4) return launch_fused_f16<4>(grid, a, tile_first, ntile_rows, nseg);
    if (f16_steps(a.radius) == 6) return launch_fused_f16<6>(grid, a, tile_first, ntile_rows, nseg);
    return launch_fused_f16<8>(grid, a, tile_first, ntile_rows, nseg);
}

}  // namespace

bool fused_on() {
    static const bool on = env_switch_on("TOPO_AMD_GAUSS_FUSED");
    return on;
}

int run_axis0_mfma(const Block& b, double sigma, float* out, int table_slot, const TwoPass& tp) {
    Context& c = ctx();
    GaussArgs a;
    TOPO_TRY(gauss_args(b, out, sigma, 1, table_slot, &a));
    set_f16_scales(sigma, &a);
    a.run_if = tp.run_if;
    const int steps = f16_steps(a.radius);
    t_grad.tile_steps = steps;
    const int mt = f16_mt(false, a.radius, tp.one_tile), tile = 32 * mt;
    const int tile_first = b.out_row0 / tile;
    const int ntiles = (b.out_row0 + b.out_rows - 1) / tile - tile_first + 1;
    const int strips = (b.nx + kMfmaCols - 1) / kMfmaCols;
    // blocks the chip holds at once: the ring of the long filters takes a CU's LDS (one block per CU), two fit up to 80 KB
    const int per_cu = f16_axis0_lds(steps, mt) <= 80 * 1024 ? 2 : 1;
    int splits = (per_cu * c.num_cu + strips - 1) / strips;
    const int min_run = 8 / mt;  // a cut restages 2 Rp rows: runs of 256 rows or more
    splits = std::max(1, std::min(splits, ntiles / min_run > 0 ? ntiles / min_run : 1));
    if (strips >= c.num_cu) splits = 1;
    const int per = (ntiles + splits - 1) / splits;
    TOPO_TRY(check_grid_rows((ntiles + per - 1) / per, "gaussian (matrix-core axis 0)"));
    dim3 grid(strips, (ntiles + per - 1) / per);
    void* flags = nullptr;
    TOPO_TRY(workspace(10, (size_t)ntiles * mt * strips * 4, &flags));
    a.flags = (unsigned char*)flags;
    TOPO_TRY(launch_f16_axis0_any(steps, mt, grid, a, tile_first, ntiles, per));
    return launch_repair<false>(a, ntiles * mt, strips * 4, tile_first * mt, 0);
}

int run_axis1_mfma(const float* in, int rows, int nx, double sigma, float* out, int table_slot, const int* run_if) {
    Context& c = ctx();
    GaussArgs a;
    TOPO_TRY(gauss_args(plane_block(in, rows, nx), out, sigma, 1, table_slot, &a));
    set_f16_scales(sigma, &a);
    a.run_if = run_if;
    a.group0 = 1;  // every band turns its tile order by a number of tiles of its own (profiles/r04_pitch_spread.txt)
    const int steps = f16_steps(a.radius);
    static const bool s1_on = env_switch_on("TOPO_AMD_GAUSS_SPLIT_ONCE");  // =0: the tile kernels everywhere (A/B)
    if (split_once(steps, s1_on)) return run_axis1_s1(a, rows, nx);
    t_grad.tile_steps = steps;
    const int mt = f16_mt(true, a.radius);
    const int bands = (rows + 31) / 32;
    const int ntile = (nx + 32 * mt - 1) / (32 * mt), nunit = (nx + 31) / 32;
    // one block of kF16Axis1Waves waves per CU (the rings take the LDS); runs no shorter than 512 columns
    const int nseg = run_cut(bands, ntile, ntile / (16 / mt), (long)kF16Axis1Waves * c.num_cu, (2 * a.radius + 32 * mt - 1) / (32 * mt));
    const long waves = (long)bands * nseg;
    void* flags = nullptr;
    TOPO_TRY(workspace(10, (size_t)bands * nunit, &flags));
    a.flags = (unsigned char*)flags;
    TOPO_TRY(launch_f16_axis1_any(steps, mt, waves, a, rows, nseg));
    return launch_repair<true>(a, bands, nunit, 0, rows);
}

int smooth_two_pass(const Block& b, double sigma, float* tmp, float* out, int table_slot, const TwoPass& tp) {
    TOPO_TRY(run_axis0_mfma(b, sigma, tmp, table_slot, tp));
    return run_axis1_mfma(tmp, b.out_rows, b.nx, sigma, out, table_slot + 1, tp.run_if);
}

int smooth_both_mfma(const Block& b, double sigma, float* tmp, float* out, int table_slot, bool for_gradient, const int* deferred,
                     bool* owed) {
    // (a DEM the fused kernel has met a non-finite or huge sample on - dem_memo, common.hpp - goes straight to the two
    // passes: the fused attempt would only be thrown away again)
    const bool fused_class = fused_radius(gaussian_radius(sigma), for_gradient, fused_on());
    const bool fused = fused_class && !dem_memo_wild(b);
    const int* flag = fused ? deferred : nullptr;
    if (fused) TOPO_TRY(run_fused_f16(b, sigma, out, table_slot, &flag));
    if (owed) *owed = fused && deferred != nullptr;
    if (fused && deferred != nullptr) return TOPO_AMD_OK;
    // (the two passes behind - or instead of - a fused launch keep its tiling of axis 0, hence its bits)
    return smooth_two_pass(b, sigma, tmp, out, table_slot, {flag, fused_class});
}

}  // namespace topo
