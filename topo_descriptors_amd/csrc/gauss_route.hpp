// Which kernel a Gaussian / gradient radius gets, and how much LDS it asks for: the arithmetic of the launchers of
// gauss.hip, gauss_f16.hip and gradient.hip, and the statement of which template instances are built at all.
// Nothing of HIP in here: plain C++17 compiles it, and tools/gauss_route_check.cpp (tests/test_gauss_route_design.py)
// walks every radius and switch setting through it on the CPU.  Environment switches are read in the .hip files and
// come in as values.
#pragma once

#include <algorithm>
#include <cstddef>

namespace topo {

constexpr size_t kLdsMax = 160 * 1024;  // dynamic LDS a block may ask for (gfx950)

// the cut of each of `lines` lines of `ntile` tiles into at most max(1, max_runs) runs with the least rounds x (tiles per
// run + the `halo` tiles a run restages), `slots` lines running at once
inline int run_cut(long lines, int ntile, int max_runs, long slots, int halo) {
    int nseg = 1;
    long best = -1;
    for (int n = 1; n <= std::max(1, max_runs); ++n) {
        const long rounds = (lines * n + slots - 1) / slots;
        const long cost = rounds * ((ntile + n - 1) / n + halo);
        if (best < 0 || cost < best) {
            best = cost;
            nseg = n;
        }
    }
    return nseg;
}

// ---- vector-ALU kernels ----
// wide tiling for long filters, narrow for short ones (fewer padded taps)
constexpr bool wide_tiling(int radius) { return radius >= 24; }
constexpr int tap_chunk_count(int R, int kb) { return (2 * R + 1 + kb - 1) / kb; }  // chunks of kb taps, the last one padded with zeros
// a tile of 64 rows x (NW * TB) output columns of the LDS-tiled axis-1 kernels: the samples a row can be asked for, and
// the bytes of the staged tile / of the tile transposed back (whichever is larger)
constexpr int axis1_tile_cols(int tb, int kb, int nw, int nchunks) { return nw * tb + nchunks * kb - 1; }
constexpr size_t axis1_tile_lds(int tb, int nw, int cols_l) {
    return std::max((size_t)64 * (cols_l | 1), (size_t)64 * (nw * tb + 1)) * sizeof(float);
}
// axis 1 of a long filter (wide tiling) has no LDS tile from here: wave-shift kernel, then the transpose path
constexpr bool axis1_tile_fits(int R) { return axis1_tile_lds(16, 8, axis1_tile_cols(16, 16, 8, tap_chunk_count(R, 16))) <= kLdsMax; }

// ---- which radii go to the matrix cores ----
// The MFMA kernels take the filters whose ring fits LDS (radius <= 121, sigma <= 30.3).  Same-box sweeps on the
// 32768^2 bench DEM (tools/grad_time.py, profiles/r02_gauss_mfma.txt).  Gaussian alone: they win at every radius
// tried, down to 4 (sigma 1.1 ... 1.75: 3.5-3.6 ms against 5.6 ms for the vector-ALU pair; sigma 2 ... 3.75: 3.9-4.2
// against 6.0-6.5; sigma 30.25: 11.3 against 23.0).  Gradient: the vector-ALU axis-1 kernel has the epilogue fused
// in while the MFMA route pays a separate epilogue (36 instead of 28 B/pixel of HBM traffic, ~8.3 ms whatever the
// radius); with the final kernels and the epilogue overlapped by row chunks the MFMA route wins from radius 8
// (sigma 2 ... 3.75: 8.3-8.4 against 8.7-10.5 ms, the fused kernel being bimodal from box to box; sigma 4: 7.85
// against 9.26; sigma 7: 8.2 against 9.8) and loses below (sigma 1.1 ... 1.75: 8.3 against 7.65); with both passes in
// one kernel it wins from radius 4 (sigma 1.25: 6.1 ms against 7.4 for the vector-ALU kernel with the epilogue fused in).
// Below radius 16 the kernels need more of the caller: the per-column accumulation offset of an axis-0 tile is the
// sample 16 rows into the (global) 32-row tile, and a row block holds that row for every tile it computes only
// when it carries 16 ghost rows (17 for the gradient) instead of R (R + 1).  gauss_ghost_rows asks for them;
// a block that comes with less takes the vector-ALU kernels (mfma_rows_ok), whose results differ from the
// matrix-core ones in the last bits: row-block bit-identity holds for ghost depths of topo_amd_halo_rows or more
// (the pre-smoothing of topo.tpi / topo.std included).  The two smooths of an anisotropic gradient keep the
// radius-16 floor: they have two radii and one ghost depth.
constexpr int kMfmaSmallFloor = 4;
constexpr int kMfmaMaxRadius = 121;
constexpr int kNoMfma = 1 << 30;
// TOPO_AMD_GAUSS_MFMA_MIN_RADIUS as the library takes it (unset: 4)
constexpr int mfma_min_radius_from(int env_value) { return std::max(kMfmaSmallFloor, env_value); }
// the smallest radius a call puts on the matrix cores: none on a large-sample raster (the vector-ALU kernels), from 16
// where the block has one ghost depth for two radii (!small_ok)
constexpr int mfma_from(bool large, bool small_ok, int min_radius) {
    return large ? kNoMfma : std::max(small_ok ? kMfmaSmallFloor : 16, min_radius);
}
// (any width from 4 columns: the loaders' 16-byte loads only need dword alignment, which a row of any length has)
constexpr bool mfma_radius(int R, int nx, int from) { return R >= from && R <= kMfmaMaxRadius && nx >= 4; }
// the accumulation-offset row of every axis-0 tile that holds one of the block's output rows is inside the block
// (or the block reaches the DEM edge there)
constexpr bool mfma_rows_ok(int in_row0, int in_rows, int gny, int out_row0, int out_rows, int R) {
    if (R >= 16) return true;
    const int y_first = out_row0 / 32 * 32 + 16, y_last = (out_row0 + out_rows - 1) / 32 * 32 + 16;
    const bool top = in_row0 <= 0 || y_first >= in_row0;
    const bool bottom = in_row0 + in_rows >= gny || y_last <= in_row0 + in_rows - 1;
    return top && bottom;
}
// ghost rows a block carries for the Gaussian of radius R: 16 for the matrix-core radii below 16 (mfma_rows_ok)
constexpr int gauss_ghost_rows_of(int R, int min_radius) { return R >= min_radius && R < 16 ? 16 : R; }

// ---- f16 matrix-core route: step counts, tiles, LDS ----
constexpr int kMfmaCols = 128;  // axis 0: columns per block (4 waves x 32)
constexpr int f16_steps(int R) { return 2 + (R + 15) / 16 * 2; }  // 16-sample steps of a 32-output tile's window: 32 + 2 Rp, Rp = R rounded up to 16
// one kernel for both passes (one sigma).  The raw blocks and rings of 10 steps no longer fit LDS.  Radius 32 ... 47 only
// where the caller says so - the gradient, whose smooth shares HBM with the epilogue (sigma 10: 7.9 -> 6.7 ms); alone the
// two passes with 64-row tiles on axis 0 are faster there (Gaussian sigma 10: 3.3 ms against 4.4).  on: TOPO_AMD_GAUSS_FUSED
constexpr int kFusedMaxRadius = 47;
constexpr bool fused_radius(int R, bool wide_too, bool on) { return on && R >= kMfmaSmallFloor && R <= (wide_too ? kFusedMaxRadius : 31); }
constexpr int fused_block_cols(int S) { return S == 4 ? 64 : 32;  }  // CW: columns of a raw block of the fused kernel
// two MFMA tiles per offset (MT = 2): axis 1 always, except the widest window (it fits LDS 3 times with MT = 2: 2.95 ms
// against 2.66 with MT = 1 four times); axis 0 from radius 32 (the offset row is 32 rows into a 64-row tile) unless
// it keeps the fused kernel's tiles (TwoPass::one_tile)
constexpr int f16_mt(bool axis1, int R, bool one_tile = false) {
    if (axis1) return f16_steps(R) < 18 ? 2 : 1;
    return R >= 32 && !one_tile ? 2 : 1;
}
constexpr int kF16Axis1Waves = 4;  // waves (32-row bands) of a block of the axis-1 tile kernel
// split once (gauss_axis1_s1_kernel): radius 49 ... 121.  on: TOPO_AMD_GAUSS_SPLIT_ONCE
constexpr bool split_once(int steps, bool on) { return on && steps >= 10; }
// NK steps of 32 window positions per 16-output tile: Rp = 16 (NK - 1) >= R
// (Rp a multiple of 32: the groups of 32 columns the march stages then never straddle a slab)
constexpr int s1_steps(int R) { return (R + 31) / 32 * 2 + 1; }
constexpr int kS1Pad = 16;  // halves behind a ring row of the split-once kernel (gauss_f16.hip has the reasons)

constexpr size_t f16_axis0_lds(int S, int MT) { return (size_t)(16 * (S + 2 * (MT - 1))) * kMfmaCols * sizeof(float); }
constexpr size_t f16_axis1_lds(int S, int MT) { return kF16Axis1Waves * (size_t)(32 * (16 * (S + 2 * (MT - 1)) + 4) + 32) * sizeof(float); }
constexpr size_t s1_axis1_lds(int NK) { return (8 * (size_t)(16 * (32 * NK + kS1Pad) + 8 * 16) + 5 * 64) * sizeof(float); }
constexpr size_t fused_lds(int S, int CW) {
    return (size_t)(2 * (128 + 2 * 8 * (S - 2)) * CW + 4 * (32 * (16 * (S + 2) + 4) + 32)) * sizeof(float);
}

// ---- gradient: the axis-1 finish of the vector-ALU route ----
// 16-wide tap chunks pay from radius ~60: 4.13 (narrow) / 3.92 ms (wide) at radius 64, 3.33 / 3.65
// at radius 56 on 16384^2 (tools/gauss_fused_sweep.sh)
constexpr int grad_tile_kb(int R) { return R >= 60 ? 16 : 8; }
// the LDS-tiled fused kernel while its tile fits (320 columns: radius 92), the wave-shift one
// beyond: 2.67 vs 3.63 ms at radius 32, 3.33 vs 4.07 at 56, 4.60 vs 5.17 at 92 on 16384^2
constexpr int kGradTiledMaxRadius = 92, kGradTileMaxCols = 320;
// PF: samples per lane and row the LDS-tiled kernel holds in registers for the next tile, cols_l <= 64 PF
constexpr int grad_tile_pf(int cols_l) { return cols_l > 256 ? 5 : cols_l > 192 ? 4 : 3; }
// the wave-shift kernel: lanes own GC adjacent columns; lanes of a wavefront that produce output at radius R.  Below
// ~42 of 64 (radius > 176, sigma > ~44) the transpose path is faster: 11.2 vs 9.0 ms at sigma 50, 68 vs 17 ms at
// sigma 107 on 16384^2 (tools/gauss_long_crossover.py)
constexpr int GC = 16;
constexpr int kWaveMinLanes = 42;
constexpr int wave_lane_reach(int R) { return (R + GC - 1) / GC; }  // lanes to either side a filter reaches into
constexpr int wave_out_lanes(int R) { return 64 - 2 * wave_lane_reach(R); }

// ---- what is built ----
// The launch switches instantiate a kernel only where its predicate holds; tools/gauss_route_check.cpp asserts that the
// rules above never pick another one and that each of these is picked by some call.
// gauss_axis0_f16_kernel<S, ., MT>.  MT = 1 below radius 32 and, behind a fused launch (one_tile), up to the fused
// kernel's last radius; MT = 2 from radius 32.
constexpr bool f16_axis0_built(int S, int MT) {
    if (S < 4 || S > f16_steps(kMfmaMaxRadius) || S % 2) return false;
    return MT == 1 ? S <= f16_steps(kFusedMaxRadius) : MT == 2 && S >= f16_steps(32);
}
// gauss_axis1_f16_kernel<S, ., MT, 4>.  f16_mt(true, .) gives MT = 2 below 18 steps and MT = 1 at 18, nothing else.
// (From 10 steps they run only with TOPO_AMD_GAUSS_SPLIT_ONCE=0.)
constexpr bool f16_axis1_built(int S, int MT) {
    if (S < 4 || S > f16_steps(kMfmaMaxRadius) || S % 2) return false;
    return MT == (S < 18 ? 2 : 1);
}
// gauss_axis1_grad_kernel<16, KB, 8, PF>.  KB = 16 runs from radius 60, where a tile row is 255 samples or more: never
// PF = 3 (<= 192).  KB = 8 runs below radius 60, 247 samples at the most: never PF = 5 (> 256).
constexpr bool axis1_grad_built(int KB, int PF) { return KB == 16 ? PF == 4 || PF == 5 : KB == 8 && (PF == 3 || PF == 4); }

}  // namespace topo
