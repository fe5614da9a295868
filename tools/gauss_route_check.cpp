// Stand-alone check of csrc/gauss_route.hpp on the CPU: every radius 0 ... 260 under every setting of the Gaussian's
// switches is walked through the decisions of the launchers (gauss.hip smooth_rows / run_axis0 / run_axis1, gauss_f16.hip
// smooth_both_mfma / run_axis*_mfma, gradient.hip gradient_slab), which are sequences of calls into that header.  Asserted:
// (a) every kernel the rules pick satisfies its *_built predicate, (b) every kernel whose predicate holds is picked by
// some input - nothing unreachable is built -, (c) no LDS size the formulas give exceeds 160 KB.  No HIP, no GPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itopo_descriptors_amd/csrc tools/gauss_route_check.cpp -o check && ./check
#include "gauss_route.hpp"

#include <cstdio>
#include <set>
#include <utility>

using namespace topo;

namespace {
struct Switches {
    int min_radius;                  // TOPO_AMD_GAUSS_MFMA_MIN_RADIUS as taken
    bool split_on, fused_on, large;  // _SPLIT_ONCE, _FUSED; a large-sample raster with _LARGE_SAMPLE on
    bool memo_wild;                  // the fused kernel met a wild sample on this DEM before
};
struct Rows {  // a row block (common.hpp Block)
    int in_row0, in_rows, gny, out_row0, out_rows;
};
constexpr int kNx = 321;

std::set<std::pair<int, int>> axis0_picked, axis1_picked, grad_picked;  // (S, MT), (S, MT), (KB, PF)
std::set<int> s1_picked, fused_picked;
int bad = 0;

void fail(const char* what, int R, int a, int b) {
    std::printf("radius %d: %s (%d, %d)\n", R, what, a, b);
    ++bad;
}
void lds_fits(size_t bytes, const char* what, int R) {
    if (bytes > kLdsMax) fail(what, R, (int)bytes, (int)kLdsMax);
}

void axis0_mfma(int R, bool one_tile) {
    const int S = f16_steps(R), mt = f16_mt(false, R, one_tile);
    axis0_picked.insert({S, mt});
    if (!f16_axis0_built(S, mt)) fail("axis-0 tile kernel picked but not built", R, S, mt);
    lds_fits(f16_axis0_lds(S, mt), "axis-0 ring", R);
}
void axis1_mfma(int R, const Switches& sw) {
    const int S = f16_steps(R);
    if (split_once(S, sw.split_on)) {
        const int nk = s1_steps(R);
        s1_picked.insert(nk);
        if (nk != 5 && nk != 7 && nk != 9) fail("split-once kernel picked but not built", R, nk, 0);
        lds_fits(s1_axis1_lds(nk), "split-once rings", R);
        return;
    }
    const int mt = f16_mt(true, R);
    axis1_picked.insert({S, mt});
    if (!f16_axis1_built(S, mt)) fail("axis-1 tile kernel picked but not built", R, S, mt);
    lds_fits(f16_axis1_lds(S, mt), "axis-1 rings", R);
}
void smooth_both_mfma(int R, bool for_gradient, const Switches& sw) {
    const bool fused_class = fused_radius(R, for_gradient, sw.fused_on);
    if (fused_class && !sw.memo_wild) {
        const int S = f16_steps(R);
        fused_picked.insert(S);
        if (S != 4 && S != 6 && S != 8) fail("fused kernel picked but not built", R, S, 0);
        lds_fits(fused_lds(S, fused_block_cols(S)), "fused kernel", R);
    }
    axis0_mfma(R, fused_class);  // the two passes, behind or instead of the fused launch
    axis1_mfma(R, sw);
}
void run_axis0(const Rows& b, int R, int from) {
    if (mfma_radius(R, kNx, from) && mfma_rows_ok(b.in_row0, b.in_rows, b.gny, b.out_row0, b.out_rows, R)) axis0_mfma(R, false);
}
void run_axis1(int rows, int R, int from, const Switches& sw) {
    if (mfma_radius(R, kNx, from)) return axis1_mfma(R, sw);
    if (!wide_tiling(R)) return lds_fits(axis1_tile_lds(8, 8, axis1_tile_cols(8, 8, 8, tap_chunk_count(R, 8))), "narrow axis-1 tile", R);
    if (axis1_tile_fits(R)) return lds_fits(axis1_tile_lds(16, 8, axis1_tile_cols(16, 16, 8, tap_chunk_count(R, 16))), "wide axis-1 tile", R);
    if (wave_out_lanes(R) >= kWaveMinLanes) return;                     // wave-shift kernel: no LDS
    run_axis0(Rows{0, kNx, kNx, 0, kNx}, R, from);                      // the transposed plane: kNx rows, `rows` columns
    (void)rows;
}
void smooth_rows(const Rows& b, int Ry, int Rx, int from, const Switches& sw) {
    if (Ry > 0 && Rx > 0) {
        if (Ry == Rx && mfma_radius(Ry, kNx, from) && mfma_rows_ok(b.in_row0, b.in_rows, b.gny, b.out_row0, b.out_rows, Ry))
            return smooth_both_mfma(Ry, false, sw);
        run_axis0(b, Ry, from);
        run_axis1(b.out_rows, Rx, from, sw);
    } else if (Ry > 0) {
        run_axis0(b, Ry, from);
    } else if (Rx > 0) {
        run_axis1(b.out_rows, Rx, from, sw);
    }
}
Rows smoothed_rows(const Rows& b) {  // the output rows plus one neighbour row inside the DEM
    Rows r = b;
    r.out_row0 = b.out_row0 > 0 ? b.out_row0 - 1 : 0;
    r.out_rows = std::min(b.out_row0 + b.out_rows + 1, b.gny) - r.out_row0;
    return r;
}
void gradient(const Rows& b, int R, bool iso, const Switches& sw) {
    if (R <= 4) return;  // sigma = R / 4 <= 1: Sobel
    const Rows s = smoothed_rows(b);
    if (!iso) {  // sig_ratio 2: two smooths, radii R and 2 R, matrix cores from radius 16
        const int from = mfma_from(sw.large, false, sw.min_radius);
        smooth_rows(s, 2 * R, R, from, sw);
        smooth_rows(s, R, 2 * R, from, sw);
        return;
    }
    const int from = mfma_from(sw.large, true, sw.min_radius);
    if (mfma_radius(R, kNx, from) && mfma_rows_ok(s.in_row0, s.in_rows, s.gny, s.out_row0, s.out_rows, R))
        return smooth_both_mfma(R, true, sw);  // chunked or in one piece: the same kernels
    run_axis0(s, R, kNoMfma);
    if (R <= kGradTiledMaxRadius) {
        const int kb = grad_tile_kb(R), cols_l = axis1_tile_cols(16, kb, 8, tap_chunk_count(R, kb));
        if (axis1_tile_lds(16, 8, cols_l) <= kLdsMax && cols_l <= kGradTileMaxCols) {
            const int pf = grad_tile_pf(cols_l);
            grad_picked.insert({kb, pf});
            if (!axis1_grad_built(kb, pf)) fail("LDS-tiled axis-1 + epilogue kernel picked but not built", R, kb, pf);
            if (cols_l > 64 * pf) fail("a tile row does not fit the prefetch registers", R, cols_l, pf);
            return;
        }
    }
    if (wave_out_lanes(R) >= kWaveMinLanes) return;
    run_axis1(s.out_rows, R, from, sw);
}
}  // namespace

int main() {
    long inputs = 0;
    for (int R = 0; R <= 260; ++R)
        for (int min_radius : {4, 16, 1000})
            for (int bits = 0; bits < 16; ++bits) {
                const Switches sw{mfma_min_radius_from(min_radius), (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0};
                // the whole raster; a block in its middle whose first / last tile's offset row is the farthest from it,
                // with what the filter needs and no more, and with the 16 (17) ghost rows of gauss_ghost_rows
                for (int ghost = -1; ghost <= 1; ++ghost)
                    for (bool grad : {false, true}) {
                        const int need = R + (grad ? 1 : 0), deep = std::max(R, 16) + (grad ? 1 : 0);
                        const int g = ghost == 1 ? deep : need;
                        const Rows b = ghost < 0 ? Rows{0, 1000, 1000, 0, 1000} : Rows{223 - g, 98 + 2 * g, 1000, 223, 98};
                        if (!grad) {
                            const int from = mfma_from(sw.large, true, sw.min_radius);
                            smooth_rows(b, R, R, from, sw);
                            smooth_rows(b, R, 0, from, sw);
                            smooth_rows(b, 0, R, from, sw);
                        } else {
                            gradient(b, R, true, sw);
                            gradient(b, R, false, sw);
                        }
                        ++inputs;
                    }
            }
    int built = 0;
    for (int S = 0; S <= 24; ++S)
        for (int MT = 1; MT <= 2; ++MT) {
            built += f16_axis0_built(S, MT) + f16_axis1_built(S, MT);
            if (f16_axis0_built(S, MT) && !axis0_picked.count({S, MT})) fail("axis-0 tile kernel built but never picked", -1, S, MT);
            if (f16_axis1_built(S, MT) && !axis1_picked.count({S, MT})) fail("axis-1 tile kernel built but never picked", -1, S, MT);
        }
    for (int KB : {8, 16})
        for (int PF = 1; PF <= 6; ++PF) {
            built += axis1_grad_built(KB, PF);
            if (axis1_grad_built(KB, PF) && !grad_picked.count({KB, PF})) fail("axis-1 + epilogue kernel built but never picked", -1, KB, PF);
        }
    for (int nk : {5, 7, 9})
        if (!s1_picked.count(nk)) fail("split-once kernel built but never picked", -1, nk, 0);
    for (int S : {4, 6, 8})
        if (!fused_picked.count(S)) fail("fused kernel built but never picked", -1, S, 0);
    std::printf("%ld inputs; %d tile / axis-1 + epilogue kernels built, %zu + %zu + %zu picked; %s\n", inputs, built, axis0_picked.size(),
                axis1_picked.size(), grad_picked.size(), bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
