// K1 wide ring: TPI of the large discs with 6 columns per lane, staging waves apart from chain waves.
//
// tpi_march_kernel<67> (disc_wave_impl.hpp) is bound by vector-ALU issue: 315 instructions per wave-row, of which the
// 18 run-in lanes of a 4-column layout waste 28 % (46 of 64 lanes write a sum) and the lane hops - 17 DPP forms per
// output column, every one at half rate - a further fifth (profiles/r06_tpi67_valu_bound.json).  Here:
//
//   * a lane owns NCW = 6 adjacent columns: 6 lane hops per side for 67 px, 52 of 64 lanes valid in all their columns and
//     the lane either side of them in one pair (316 of 384 staged columns: the disc reaches 33 columns, not 36; WGeo::XV),
//     the chain two-sided and rim first as in ring_disc_sum (disc_ring_impl.hpp);
//   * a ring row is 384 dwords (1.5 KiB), staged column c at dword c: lane l reads its 6 columns as three ds_read_b64 at
//     +0, +8 and +16 from byte 24 l (dwords 6 l, 6 l + 1 of the 32 lanes of a group are distinct mod 64: conflict-free);
//   * the ring holds R = SIZE + 32 rows plus GR = 6 guard rows behind them, copies of slots 0 .. GR - 1 (WideCfg), so
//     that one VGPR address at slot (s0 + k) mod R reaches the rows k .. k + GR of the window by immediate offsets: nine
//     addresses a row pair (WPair) instead of one per read;
//   * a chain wave sums its two rows of a phase in ONE sweep (wide_pair_sum): the pair needs 55 distinct prefix rows at
//     67 px where two single rows read 84, and each is read once;
//   * the staging runs on waves of its own (std_ring_spec_kernel's structure):
//     waves 0-2 convert, classify and write batch ph + 1 (16 rows, two columns per lane, 8-byte loads) and issue the
//     loads of batch ph + 2 while waves 3-10 run two output rows each of phase ph; ONE barrier per phase, in front of which
//     a chain wave has already issued the first fetches of its next sweep (WIDE_BOUNDARY); a batch whose rows,
//     columns and slots need no test, clamp or wrap (wave-uniform: nearly all of them) takes a lean path of its own; the
//     classification is wide_classify.hpp's: per row two fractional parts ORed into one register and one float maximum of
//     magnitudes into another, three compares a batch;
//   * prefix sums are uint32 modulo 2^32 with no offset and the finalisation is tpi_march_kernel's expression, so the
//     bits are those of the marching kernel.
//
// Which phases it computes: a phase (16 output rows of a strip) whose window holds a fractional, non-finite or absurd
// sample is not computed; the block marks the tiles of the MARCHING geometry (Geo<SIZE>::TILE_W x 60 rows) that the
// phase overlaps kNeedsFraction in p.defer (the launcher clears that map first), and the scaled pass and the general
// kernel that follow take those tiles exactly as they take the marching kernel's.  A pixel whose disc holds whole metres
// only gets the same bits from every one of them (tpi_scaled_march_kernel), so the granularity of the marking cannot
// change a bit.  Single-block calls only (no seam parts).
#pragma once

#include "wide_classify.hpp"

namespace topo {

namespace {

constexpr int NCW = 6;  // columns per lane of the wide ring

template <int SIZE>
struct WGeo {
    static constexpr DiscTable<SIZE> T = make_disc_table<SIZE>();
    static_assert(T.centre == 0 && T.off_min == -T.off_max, "odd disc sizes only");
    static constexpr int M = T.off_max;
    static constexpr int DL = (M + NCW - 1) / NCW;  // lane hops per side
    static constexpr int NVL = 64 - 2 * DL;         // lanes that end up with full sums in all their columns
    static constexpr int W = 64 * NCW;              // staged columns = dwords per ring row
    // The disc needs M staged columns a side, not NCW DL: the lanes next to the whole ones (DL - 1 and 64 - DL) hold valid
    // sums in the columns whose step DL takes nothing (WSweep::edges_valid), and the hops shift zeros in at the wave's ends.
    // Stores go by pairs of columns, so the first valid staged column is M rounded up to even.
    static constexpr int XV = (M + 1) / 2 * 2;      // first staged column that is stored
    static constexpr int TILE_W = W - 2 * XV;       // valid output columns per strip
    static constexpr int X0 = XV;                   // staged column of the first valid output
    static constexpr int NR = T.num_runs;
    static_assert(NVL >= 16, "disc too wide for one wavefront");
    // RGeo::Sched for 6 columns per lane: per run the largest step that uses it, the runs in the order first needed
    struct Sched {
        int first_step[SIZE];
        int order[SIZE];
        int centre_run;
    };
    static constexpr Sched make() {
        Sched t{};
        for (int r = 0; r < SIZE; ++r) t.first_step[r] = -1;
        for (int r = 0; r < SIZE; ++r) t.order[r] = 0;
        t.centre_run = -1;
        for (int D = 0; D <= DL; ++D)
            for (int s = 0; s < NCW; ++s)
                for (int q = 0; q < NCW; ++q) {
                    const int dr = NCW * D + s - q, dl = -NCW * D + s - q;
                    if (dr >= 0 && dr <= M) {
                        const int r = T.run_of[dr - T.off_min];
                        if (D > t.first_step[r]) t.first_step[r] = D;
                    }
                    if (dl < 0 && dl >= -M) {
                        const int r = T.run_of[dl - T.off_min];
                        if (D > t.first_step[r]) t.first_step[r] = D;
                    }
                }
        int n = 0;
        for (int D = DL; D >= 0; --D)
            for (int d = M; d >= 0; --d) {
                const int r = T.run_of[d - T.off_min];
                bool seen = false;
                for (int i = 0; i < n; ++i) seen = seen || t.order[i] == r;
                if (!seen && t.first_step[r] == D) t.order[n++] = r;
            }
        for (int r = 0; r < NR; ++r)
            if (T.run_lo[r] == 0 && T.run_hi[r] == 0) t.centre_run = r;
        return t;
    }
    static constexpr Sched S = make();
    static_assert(S.centre_run >= 0, "the disc's outermost column is the pixel's own row");
};

template <int SIZE>
struct WideCfg {
    using G = WGeo<SIZE>;
    static constexpr int SW = 3;        // staging waves: two columns per lane, 128 columns per wave
    static constexpr int CW = 8;        // chain waves
    static constexpr int NW = SW + CW;
    static constexpr int RPW = 2;       // output rows per chain wave and phase
    static constexpr int B = CW * RPW;  // rows per phase and per batch
    static constexpr int TH = 64;       // rows of a work tile (the blocks' runs are made of these)
    static constexpr int PPT = TH / B;
    static constexpr int R = SIZE + 2 * B;  // the window of a phase and the batch staged beside it
    static constexpr int GR = 6;            // guard rows: slot R + s holds what slot s holds (s < GR)
    static constexpr int HALO = SIZE - 1;
    static constexpr int PAD = 1 + (B - (1 + HALO + B) % B) % B;
    static constexpr int PRO = PAD + HALO + B;
    static constexpr int NB_PRO = PRO / B;  // batches a phase's window touches
    static constexpr size_t LDS = (size_t)(R + GR) * G::W * sizeof(uint32_t) + 2 * SW * sizeof(int) + 16;
    static_assert(SW * 128 == G::W, "two staged columns per staging lane");
    static_assert(TH % B == 0 && PRO % B == 0, "whole batches");
    static_assert(LDS <= 160 * 1024, "ring does not fit LDS");
    static_assert(NB_PRO <= 15, "batch history: two fields of a flag word");
};

constexpr bool tpi_wide_ring_fits(int size) {
    return size >= 5 && size % 2 == 1 && (size_t)(size + 32 + 6) * 384 * 4 + 64 <= 160 * 1024 && 64 - 2 * ((size / 2 + 5) / 6) >= 16;
}

// The prefix-row reads of a chain wave's row pair, rows A and B = A + 1 of a phase, in Q indices of row A's window
// (0 .. 2 M + 2; row B's index k is row A's k + 1).  Run r of row A reads top = run_hi + 1 + M and bot = run_lo + M, of row
// B the rows one below: the top row of B at height h is the top row of A at height h + 1 and the bottom row of B at
// height h the bottom row of A at height h - 1, so wherever the disc's run heights are consecutive the pair needs each
// of those rows once.  A distinct row is loaded by the first fetch (index into WGeo::S.order) that needs it and stays in
// registers until the last that does; use[i][w][e] names the row that serves fetch i, row w of the pair, top (e = 0) or
// bottom (e = 1) - the Q index itself.
// The VGPR addresses: a base at Q index kb is the one VGPR 24 lane + ((s0 + kb) mod R) PB; a read at k with
// kb <= k <= kb + GR is that base plus the immediate (k - kb) PB (+0, +8, +16): it lands in slot
// (s0 + kb) mod R + k - kb <= R - 1 + GR, a guard row where the ring wraps.  The bases cover the distinct rows greedily from
// the smallest, and each is formed at the first fetch that loads through it (so it lives only over its stretch of the sweep).
template <int SIZE, int GR>
struct WPair {
    using G = WGeo<SIZE>;
    static constexpr int NR = G::NR;
    static constexpr int NK = 2 * G::M + 3;  // Q indices of the pair
    struct Tab {
        int rows;              // distinct prefix rows of the pair
        int nb;                // bases
        int kb[NK];            // Q index of base b
        int first[NK];         // fetch that forms base b
        int base[NK];          // per Q index: the base its read goes through
        int use[SIZE][2][2];   // per fetch, row of the pair, top / bottom: the Q index that serves it
        int nload[SIZE];       // per fetch: rows it loads
        int load[SIZE][4];     // ... and their Q indices
    };
    static constexpr Tab make() {
        Tab t{};
        bool need[NK] = {};
        for (int i = 0; i < NR; ++i) {
            const int r = G::S.order[i];
            for (int w = 0; w < 2; ++w) {
                t.use[i][w][0] = G::T.run_hi[r] + 1 + G::M + w;
                t.use[i][w][1] = G::T.run_lo[r] + G::M + w;
            }
            for (int w = 0; w < 2; ++w)
                for (int e = 0; e < 2; ++e) {
                    const int k = t.use[i][w][e];
                    if (!need[k]) t.load[i][t.nload[i]++] = k;
                    need[k] = true;
                }
        }
        for (int k = 0; k < NK; ++k) {
            if (!need[k]) continue;
            ++t.rows;
            if (t.nb == 0 || k > t.kb[t.nb - 1] + GR) t.kb[t.nb++] = k;
            t.base[k] = t.nb - 1;
        }
        for (int b = 0; b < t.nb; ++b) t.first[b] = NR;
        for (int i = NR - 1; i >= 0; --i)
            for (int n = 0; n < t.nload[i]; ++n) t.first[t.base[t.load[i][n]]] = i;
        return t;
    }
    static constexpr Tab T = make();
    static constexpr bool check() {
        bool loaded[NK] = {};
        for (int i = 0; i < NR; ++i) {
            for (int n = 0; n < T.nload[i]; ++n) {
                const int k = T.load[i][n], b = T.base[k];
                if (k < T.kb[b] || k - T.kb[b] > GR || T.first[b] > i || loaded[k]) return false;
                loaded[k] = true;
            }
            for (int w = 0; w < 2; ++w)
                for (int e = 0; e < 2; ++e)
                    if (!loaded[T.use[i][w][e]]) return false;
        }
        return true;
    }
    // the rows the first `lead` fetches load, and the largest Q index among them
    static constexpr int lead_rows(int lead) {
        int n = 0;
        for (int i = 0; i < lead && i < NR; ++i) n += T.nload[i];
        return n;
    }
    static constexpr int lead_bases(int lead) {
        int n = 0;
        for (int b = 0; b < T.nb; ++b) n += T.first[b] < lead ? 1 : 0;
        return n;
    }
    static constexpr int lead_reach(int lead) {
        int m = 0;
        for (int i = 0; i < lead && i < NR; ++i)
            for (int n = 0; n < T.nload[i]; ++n) m = T.load[i][n] > m ? T.load[i][n] : m;
        return m;
    }
    // The lead fetches of a pair's NEXT phase may be issued in front of the barrier that ends this one: in indices
    // u = j + k of the next phase's window (j: the pair's first row in the phase, at most B - 2; k: the Q index) the batch
    // that barrier publishes is u = 2 M + 1 .. 2 M + B, everything below it was published a barrier earlier, and the staging
    // waves meanwhile write only slots of rows older than the window.  So: the lead fetches' largest k plus B - 2 is at most 2 M.
    template <int LEAD, int B>
    static constexpr bool lead_is_published() { return lead_reach(LEAD) + B - 2 <= 2 * G::M; }
    // the rows a pair would read without sharing (four a run), and what the run heights of the disc leave of them
    static constexpr int kUnshared = 4 * NR;
    static_assert(check(), "every row loaded once, before its uses, within GR rows of a base formed by then");
    static_assert(T.rows < kUnshared, "the pair shares no prefix row");
    static_assert(SIZE != 67 || T.rows == 55, "67 px: 55 distinct prefix rows a pair (84 unshared)");
};

// (a loop whose index is a constant expression in its body: if constexpr on the disc's tables)
template <int N, int I = 0, class F>
__device__ __forceinline__ void wide_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        wide_static_for<N, I + 1>(f);
    }
}

// The joint sweep's order of sums: the runs in the order WGeo::S.order, the lane's columns s = 0 .. NCW - 1 of each.
// firstR[D][t] (firstL) is j NCW + s of the first difference that goes into step D of the right (left) chain for output
// t - the one that starts the sum - or -1 where the lane's own columns give that step nothing.
// lo_s[j][side][D][t] .. hi_s[j][side][D][t] (side 0 right, 1 left) are the first and last column s of the lane whose tap
// for that sum belongs to fetch j's run (lo_s > hi_s: none).  A run's columns on one side of the centre are adjacent, so
// the taps of a sum within a run are ONE interval of s, and the sweep adds the interval's sum, not its members.
template <int SIZE>
struct WSweep {
    using G = WGeo<SIZE>;
    struct Tab {
        int firstR[G::DL + 1][NCW], firstL[G::DL + 1][NCW];
        int lo_s[G::NR][2][G::DL + 1][NCW], hi_s[G::NR][2][G::DL + 1][NCW];
    };
    // the disc offset of column s of the lane in step D of the chain of `side` for output t, and whether that side takes it
    static constexpr int tap(int side, int D, int s, int t) { return (side == 0 ? NCW * D : -NCW * D) + s - t; }
    static constexpr bool takes(int side, int di) { return side == 0 ? di >= 0 && di <= G::M : di < 0 && di >= -G::M; }
    static constexpr Tab make() {
        Tab t{};
        for (int D = 0; D <= G::DL; ++D)
            for (int o = 0; o < NCW; ++o) t.firstR[D][o] = t.firstL[D][o] = -1;
        for (int j = G::NR - 1; j >= 0; --j)
            for (int s = NCW - 1; s >= 0; --s)
                for (int D = 0; D <= G::DL; ++D)
                    for (int o = 0; o < NCW; ++o) {
                        const int dr = NCW * D + s - o, dl = -NCW * D + s - o;
                        if (dr >= 0 && dr <= G::M && G::T.run_of[dr - G::T.off_min] == G::S.order[j]) t.firstR[D][o] = j * NCW + s;
                        if (dl < 0 && dl >= -G::M && G::T.run_of[dl - G::T.off_min] == G::S.order[j]) t.firstL[D][o] = j * NCW + s;
                    }
        for (int j = 0; j < G::NR; ++j)
            for (int side = 0; side < 2; ++side)
                for (int D = 0; D <= G::DL; ++D)
                    for (int o = 0; o < NCW; ++o) {
                        int lo = NCW, hi = -1;
                        for (int s = 0; s < NCW; ++s) {
                            const int di = tap(side, D, s, o);
                            if (takes(side, di) && G::T.run_of[di - G::T.off_min] == G::S.order[j]) {
                                lo = s < lo ? s : lo;
                                hi = s;
                            }
                        }
                        t.lo_s[j][side][D][o] = lo;
                        t.hi_s[j][side][D][o] = hi;
                    }
        return t;
    }
    static constexpr Tab T = make();
    // over all runs the intervals take every (offset, output) pair with |offset| <= M exactly once
    static constexpr bool covers() {
        int hits[NCW][2 * G::M + 1] = {};
        int total = 0;
        for (int j = 0; j < G::NR; ++j)
            for (int side = 0; side < 2; ++side)
                for (int D = 0; D <= G::DL; ++D)
                    for (int o = 0; o < NCW; ++o)
                        for (int s = T.lo_s[j][side][D][o]; s <= T.hi_s[j][side][D][o]; ++s) {
                            const int di = tap(side, D, s, o);
                            if (di < -G::M || di > G::M) return false;
                            ++hits[o][di + G::M];
                            ++total;
                        }
        for (int o = 0; o < NCW; ++o)
            for (int d = 0; d <= 2 * G::M; ++d)
                if (hits[o][d] != 1) return false;
        return total == NCW * (2 * G::M + 1);
    }
    // the difference that starts a sum is the first column of an interval, and no interval lies before it
    static constexpr bool firsts_start_intervals() {
        for (int side = 0; side < 2; ++side)
            for (int D = 0; D <= G::DL; ++D)
                for (int o = 0; o < NCW; ++o) {
                    const int f = side == 0 ? T.firstR[D][o] : T.firstL[D][o];
                    for (int j = 0; j < G::NR; ++j) {
                        const bool empty = T.lo_s[j][side][D][o] > T.hi_s[j][side][D][o];
                        if (f < 0 || j < f / NCW) {
                            if (!empty) return false;
                        } else if (j == f / NCW) {
                            if (empty || T.lo_s[j][side][D][o] != f % NCW) return false;
                        }
                    }
                }
        return true;
    }
    // every stored column (staged XV .. W - XV - 1) has its taps among the staged columns, and where a step's source lane
    // lies beyond the wave's ends (-1, 64: the hop shifts a zero in) that step takes nothing for the column
    static constexpr bool edges_valid() {
        for (int c = G::XV; c < G::W - G::XV; ++c) {
            const int lane = c / NCW, o = c % NCW;
            if (c - G::M < 0 || c + G::M > G::W - 1) return false;
            for (int D = 0; D <= G::DL; ++D) {
                if (lane + D > 63 && T.firstR[D][o] >= 0) return false;
                if (lane - D < 0 && T.firstL[D][o] >= 0) return false;
            }
        }
        return true;
    }
    static_assert(covers(), "the intervals take every tap of every output once: SIZE taps an output");
    static_assert(G::XV % 2 == 0 && G::XV >= G::M && G::TILE_W % 2 == 0,
                  "whole store pairs, a disc's reach inside the staged columns");
    static_assert(edges_valid(), "a stored column takes nothing from beyond the wave's ends");
    static_assert(SIZE != 67 || NCW * (2 * G::M + 1) == 402, "67 px: 402 taps per side pair");
    static_assert(firsts_start_intervals(), "firstR / firstL name an interval's first column");
    // issue priority over the steps DL ... 0: 3 at the first, 0 at the last
    static constexpr int prio_of(int D) { return 3 - (G::DL - D) * 4 / (G::DL + 1); }
};

#ifndef WIDE_LEAD
#define WIDE_LEAD 2
#endif
// (1: the issue-priority ladder of wide_pair_sum for the chain waves, and the staging waves at priority 3 while they stage
// a batch; 0: no wave touches its priority, the kernel of rounds 9 - 12, kept as the A/B switch.  See wide_pair_sum.)
#ifndef WIDE_PRIO
#define WIDE_PRIO 1
#endif

// (lab switch, off in the product: 1 lets a chain wave issue the lead fetches of its NEXT phase in front of the phase barrier,
// which it then crosses bare, and keep its phase state - ring slot, output rows - by increments.  Measured in round 14 and
// not kept: the way from the barrier to the sweep falls from 93 to 46 instructions and the counters follow, the bench step
// does not (-0.3 % and +0.2 % in two sessions, inside the runs' spread).  DESIGN.md K1 round 14, tools/valu_bound.py wide,
// tools/ubench/tpi_lab.hip -DWIDE_BOUNDARY=1, profiles/r14_tpi67_boundary_stamps.txt.)
#ifndef WIDE_BOUNDARY
#define WIDE_BOUNDARY 0
#endif

// (lab switch: 1 stamps the clock around what a wave waits for at the end of a phase - a drain of the chain waves' output
// stores (s_waitcnt vmcnt(0), which the compiler put there itself until round 10), then the barrier - summed per wave in
// scalar registers and written by two blocks with ordinary stores when the kernel ends; 2 stamps the same points and
// drains nothing, the kernel as it is built.  tools/ubench/tpi_lab.hip -DWIDE_STAMPS=1, profiles/r10_tpi67_store_drain.txt.
// Round 14 adds the chain waves' way from the barrier to the sweep: a stamp where the lead rows have arrived, summed per wave
// over the phases that sweep as its distance from the stamp behind the barrier.  profiles/r14_tpi67_boundary_stamps.txt)
#ifndef WIDE_STAMPS
#define WIDE_STAMPS 0
#endif
// (lab switch: 0 stages every batch on the general path, the kernel of rounds 7 - 10, for an A/B against the lean path)
#ifndef WIDE_LEAN
#define WIDE_LEAN 1
#endif
// (lab switch: 1 leaves the classification out of stage_batch - convert, prefix, write, flags constant 0 - on both of its
// paths: what the staging waves' stream could shrink to at the most.  Right on rasters of whole metres only, where every
// window is computed anyway.  tools/ubench/tpi_lab.hip -DWIDE_STAGE_CEILING=1, profiles/r11_tpi67_staging_ceiling.txt)
#ifndef WIDE_STAGE_CEILING
#define WIDE_STAGE_CEILING 0
#endif
#if WIDE_STAMPS
constexpr int kWideStampBlocks = 2, kWideStampWaves = 11, kWideStampFields = 7;
// per stamped block and wave: phases, ticks in all of them, in the drain, at the barrier, in a back-to-back stamp pair; sweeps
// that follow a barrier of the run, ticks from that barrier to the sweep's start
__device__ unsigned long long wide_stamps[kWideStampBlocks][kWideStampWaves][kWideStampFields];
__device__ __forceinline__ uint32_t wide_now() {  // (the low word: a phase is a few thousand ticks, a launch's sums fit)
    const uint32_t t = (uint32_t)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stamp is taken here, not where its first use falls
    return t;
}
#endif

typedef uint32_t u32x2w __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const char lds_char;
typedef __attribute__((address_space(1))) const u32x2w glb_u32x2w;
typedef __attribute__((address_space(3))) const volatile u32x2w lds_u32x2w;

// Fetch I of a pair's sweep: the bases it is the first to load through, then its rows.  b0 is the byte offset of the ring
// slot of Q index 0 of row A's window, lb the lane's byte offset in a ring row.
template <int SIZE, int R, int GR, int I>
__device__ __forceinline__ void wide_pair_fetch(const uint32_t* ring, uint32_t b0, uint32_t lb,
                                                u32x2w (&row)[WPair<SIZE, GR>::NK][3], uint32_t (&vb)[WPair<SIZE, GR>::T.nb]) {
    using PT = WPair<SIZE, GR>;
    constexpr uint32_t PB = (uint32_t)WGeo<SIZE>::W * 4;  // bytes per ring row
    constexpr uint32_t RB = (uint32_t)R * PB;
    lds_char* q = (lds_char*)ring;
#pragma unroll
    for (int b = 0; b < PT::T.nb; ++b)
        if (PT::T.first[b] == I) {
            const uint32_t d = b0 + (uint32_t)PT::T.kb[b] * PB;
            vb[b] = lb + min(d, d - RB);  // the scalar wrap, then one vector add
            asm("" : "+v"(vb[b]));        // (opaque: every read of the base keeps it and takes an immediate offset)
        }
#pragma unroll
    for (int n = 0; n < PT::T.nload[I]; ++n) {
        const int k = PT::T.load[I][n];
        lds_char* pk = q + vb[PT::T.base[k]] + (uint32_t)(k - PT::T.kb[PT::T.base[k]]) * PB;
        // (volatile: three ds_read_b64, not merged into ds_read2_b64, which banks 32 wide and moves half as many bytes a cycle)
#pragma unroll
        for (int h = 0; h < 3; ++h) row[k][h] = *(lds_u32x2w*)(pk + 8 * h);
    }
}

// The lead fetches of a pair: the first LEAD fetches of its sweep, issued before the sweep starts - with WIDE_BOUNDARY in
// front of the phase barrier (WPair::lead_is_published), so that the sweep behind it starts on registers already loading.
// Their rows and bases, and nothing else of the sweep's, live from one phase to the next: lrow and lvb hold them in the order
// loaded / formed (wide_lead_rows copies them to and from the sweep's own arrays; the copies are names, not instructions).
template <int SIZE, int GR, int LEAD, bool OUT, class ROWS, class BASES>
__device__ __forceinline__ void wide_lead_rows(ROWS& lrow, BASES& lvb, u32x2w (&row)[WPair<SIZE, GR>::NK][3],
                                               uint32_t (&vb)[WPair<SIZE, GR>::T.nb]) {
    using PT = WPair<SIZE, GR>;
    int n = 0;
#pragma unroll
    for (int i = 0; i < LEAD && i < PT::NR; ++i)
#pragma unroll
        for (int m = 0; m < PT::T.nload[i]; ++m, ++n)
#pragma unroll
            for (int h = 0; h < 3; ++h) {
                if (OUT) lrow[n][h] = row[PT::T.load[i][m]][h];
                else row[PT::T.load[i][m]][h] = lrow[n][h];
            }
    int nb = 0;
#pragma unroll
    for (int b = 0; b < PT::T.nb; ++b)
        if (PT::T.first[b] < LEAD) {
            if (OUT) lvb[nb] = vb[b];
            else vb[b] = lvb[nb];
            ++nb;
        }
}

template <int SIZE, int R, int GR, int LEAD>
__device__ __forceinline__ void wide_pair_lead(const uint32_t* ring, uint32_t b0, int lane,
                                               u32x2w (&lrow)[WPair<SIZE, GR>::lead_rows(LEAD)][3],
                                               uint32_t (&lvb)[WPair<SIZE, GR>::lead_bases(LEAD)]) {
    using PT = WPair<SIZE, GR>;
    constexpr int NR = WGeo<SIZE>::NR;
    const uint32_t lb = (uint32_t)lane * (NCW * 4);
    u32x2w row[PT::NK][3];
    uint32_t vb[PT::T.nb];
    wide_static_for<(LEAD < NR ? LEAD : NR)>(
        [&](auto I) { wide_pair_fetch<SIZE, R, GR, decltype(I)::value>(ring, b0, lb, row, vb); });
    wide_lead_rows<SIZE, GR, LEAD, true>(lrow, lvb, row, vb);
}

// Disc sums of the two output rows of a chain wave in ONE sweep (ring_disc_sum with 6 columns per lane, two rows): b0 is
// the byte offset of the ring slot of Q index 0 of row A's window, acc[w][t] the sum of row w for the lane's column
// NCW lane + t (valid for DL <= lane < 64 - DL, and for the columns WGeo::XV admits of the lanes beside them), ctr[w][t]
// that pixel's own value.  The runs go in the order WGeo::S.order; fetch i loads the prefix rows of the pair that no
// earlier fetch has loaded (WPair), and both rows' differences of a run are formed from the loaded rows, the shared ones
// among them.
// PRIO (WIDE_PRIO, on): the wave's issue priority goes 3 -> 2 -> 1 -> 0 over the sweep's steps (CHAIN_PRIO,
// disc_wave_impl.hpp), the counterpart of the 3 -> 2, 1 -> 0 pair that made the two chain waves of a SIMD advance together
// when each summed its two rows one after the other.  A SIMD serves the higher priority first and among equals the older
// wave, so without a ladder the older chain wave of a SIMD runs nearly unimpeded, reaches the barrier some 2300 ticks of a
// phase's 8800 before the younger, and the younger runs that quarter of a phase alone, at half the rate a SIMD can issue.  With the
// ladder the wave behind always outranks or ties the wave ahead and the two leapfrog a level at a time: the gap is about 440
// ticks and a phase about 8160.  The ladder holds only with the staging waves on top of it: they raise themselves to 3
// while they stage a batch (run_phases) and drop to 0 for the next batch's loads and the barrier, and being the oldest waves
// they win the tie with a chain wave at 3.  The ladder alone (round 9) lost, 4.12 against 3.68 ms a bench step: chain waves
// at 3, 2 and 1 hold a staging wave at 0 back by thousands of ticks (rounds 9 and 13).  The
// wave leaves the sweep at 0 - the finalisation and the stores run there - and a wave that sweeps nothing in a phase never
// raised itself.  A compile-time choice, and no branch in the sweep either way: a DPP move and the add it feeds fold into
// one DPP add only within a basic block.
// (LEAD_DONE: the caller has issued the lead fetches - wide_pair_lead with this b0 - into row and vb)
template <int SIZE, int R, int GR, int LEAD, bool PRIO, bool LEAD_DONE>
__device__ __forceinline__ void wide_pair_sum(const uint32_t* ring, uint32_t b0, int lane,
                                              u32x2w (&lrow)[WPair<SIZE, GR>::lead_rows(LEAD)][3],
                                              uint32_t (&lvb)[WPair<SIZE, GR>::lead_bases(LEAD)], uint32_t (&acc)[2][NCW],
                                              uint32_t (&ctr)[2][NCW]
#if WIDE_STAMPS
                                              , uint32_t& t_sweep
#endif
) {
    using G = WGeo<SIZE>;
    using PT = WPair<SIZE, GR>;
    using SW_ = WSweep<SIZE>;
    constexpr int NR = G::NR;
    constexpr int DL = G::DL;
    // pR[w][D][t], pL[w][D][t]: what the lane's own columns give step D of row w's right / left chain for output t, summed
    // run by run as the differences are formed (a difference goes into every step that takes it at once and is not
    // kept: one sweep holds the open steps' sums of two rows, not two rows' differences of the runs in flight)
    uint32_t pR[2][DL + 1][NCW], pL[2][DL + 1][NCW];
    uint32_t aR[2][NCW], aL[2][NCW];
    u32x2w row[PT::NK][3];
    uint32_t vb[PT::T.nb];
    const uint32_t lb = (uint32_t)lane * (NCW * 4);
    auto fetch = [&](auto I) { wide_pair_fetch<SIZE, R, GR, decltype(I)::value>(ring, b0, lb, row, vb); };
    // step D of the chains of both rows: the lane's own part, then the hop
    auto close = [&](auto DD) {
        constexpr int D = decltype(DD)::value;
        wide_static_for<NCW * 2>([&](auto TW) {
            constexpr int t = decltype(TW)::value / 2, w = decltype(TW)::value % 2;
            constexpr bool anyr = SW_::T.firstR[D][t] >= 0, anyl = SW_::T.firstL[D][t] >= 0;
            uint32_t pr = 0, pl = 0;
            if constexpr (anyr) pr = pR[w][D][t];
            if constexpr (anyl) pl = pL[w][D][t];
            if constexpr (D == DL) {
                aR[w][t] = pr;
                aL[w][t] = pl;
            } else if constexpr (D == 0) {
                // the last step and the final aR + aL as one plain add and two DPP adds: hop(aR) + (hop_up(aL) + (pr + pl))
                uint32_t own = anyr && anyl ? pr + pl : anyr ? pr : pl;
                asm("" : "+v"(own));
                own = hop_up(aL[w][t]) + own;
                asm("" : "+v"(own));
                aR[w][t] = hop(aR[w][t]) + own;  // the disc sum
                asm("" : "+v"(aR[w][t]));        // (here, beside its DPP move, not sunk behind the caller's lane test)
            } else {
                // (the lane's own part opaque: the DPP move folds into a two-operand add, see ring_disc_sum)
                if constexpr (anyr) {
                    asm("" : "+v"(pr));
                    aR[w][t] = hop(aR[w][t]) + pr;
                } else {
                    aR[w][t] = hop(aR[w][t]);
                }
                if constexpr (anyl) {
                    asm("" : "+v"(pl));
                    aL[w][t] = hop_up(aL[w][t]) + pl;
                } else {
                    aL[w][t] = hop_up(aL[w][t]);
                }
            }
        });
        RING_SB();
    };
    if constexpr (LEAD_DONE) wide_lead_rows<SIZE, GR, LEAD, false>(lrow, lvb, row, vb);
    else wide_static_for<(LEAD < NR ? LEAD : NR)>([&](auto I) { fetch(I); });
#if WIDE_STAMPS
    t_sweep = wide_now();  // (waits for the lead rows: the sweep's first subtract would)
#endif
    if constexpr (PRIO) CHAIN_SETPRIO(3);
    static_assert(DL >= 1 && G::S.first_step[G::S.order[0]] == DL, "the first run opens the chains, the last step (D = 0) closes both");
    wide_static_for<NR>([&](auto J) {
        constexpr int j = decltype(J)::value;
        constexpr int r = G::S.order[j];
        constexpr int D = G::S.first_step[r];  // the step that takes run r first (the steps go DL ... 0)
        constexpr int Dprev = j == 0 ? DL : G::S.first_step[G::S.order[j > 0 ? j - 1 : 0]];
        constexpr int Dnext = j + 1 < NR ? G::S.first_step[G::S.order[j + 1 < NR ? j + 1 : j]] : -1;
        if constexpr (PRIO && SW_::prio_of(D) != SW_::prio_of(Dprev)) CHAIN_SETPRIO(SW_::prio_of(D));
        if constexpr (j + LEAD < NR) fetch(std::integral_constant<int, j + LEAD>{});
        RING_SB();
        // the differences of the run for the lane's six columns of both rows, their prefix and suffix sums over s (the
        // compiler drops the ones no interval asks for), then every (side, step, output) sum takes its interval in one add
        uint32_t cv[2][NCW], pre[2][NCW], suf[2][NCW];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
            for (int s = 0; s < NCW; ++s) {
                cv[w][s] = row[PT::T.use[j][w][0]][s / 2][s % 2] - row[PT::T.use[j][w][1]][s / 2][s % 2];
                if (r == G::S.centre_run) ctr[w][s] = cv[w][s];
            }
            pre[w][0] = cv[w][0];
            suf[w][NCW - 1] = cv[w][NCW - 1];
#pragma unroll
            for (int s = 1; s < NCW; ++s) {
                pre[w][s] = pre[w][s - 1] + cv[w][s];
                suf[w][NCW - 1 - s] = suf[w][NCW - s] + cv[w][NCW - 1 - s];
            }
        }
        wide_static_for<2 * (DL + 1) * NCW>([&](auto ET) {
            constexpr int side = decltype(ET)::value / ((DL + 1) * NCW);
            constexpr int E = decltype(ET)::value / NCW % (DL + 1), t = decltype(ET)::value % NCW;
            constexpr int a = SW_::T.lo_s[j][side][E][t], b = SW_::T.hi_s[j][side][E][t];
            if constexpr (a <= b) {
                static_assert(E <= D, "a run arrives at the first step that takes it");
                constexpr bool starts = (side == 0 ? SW_::T.firstR[E][t] : SW_::T.firstL[E][t]) / NCW == j;
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const uint32_t iv = a == b ? cv[w][a] : a == 0 ? pre[w][b] : b == NCW - 1 ? suf[w][a] :
                                        b == a + 1 ? cv[w][a] + cv[w][b] : pre[w][b] - pre[w][a - 1];
                    uint32_t& acc_p = side == 0 ? pR[w][E][t] : pL[w][E][t];
                    acc_p = starts ? iv : acc_p + iv;
                }
            }
        });
        RING_SB();
        // the steps no later run opens: closed here
        wide_static_for<D - Dnext>([&](auto C) { close(std::integral_constant<int, D - decltype(C)::value>{}); });
    });
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
        for (int t = 0; t < NCW; ++t) acc[w][t] = aR[w][t];
}


template <int SIZE>
__global__ __launch_bounds__(WideCfg<SIZE>::NW * 64) void tpi_ring_wide_kernel(WaveArgs p, int tiles_x, int tiles_y, PartRun deal) {
    using G = WGeo<SIZE>;
    using C = WideCfg<SIZE>;
    constexpr int B = C::B, R = C::R, PPT = C::PPT, SW = C::SW, NB_PRO = C::NB_PRO;
    constexpr unsigned kWindow = (1u << NB_PRO) - 1u;
    constexpr int kBad = 1, kFracOnly = 1 << 15;  // flag word: one field per batch history (the prologue shifts both)
    constexpr unsigned kHistMask = kWindow | kWindow * kFracOnly;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_u[];
    uint32_t* Q = lds_u;
    int* wflags = reinterpret_cast<int*>(Q + (R + C::GR) * G::W);  // [2 parities][SW]: what each staging wave saw

    const int nb = (int)gridDim.x;
    const int vb = (nb & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (nb >> 3) + (int)(blockIdx.x >> 3);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ntiles = tiles_x * tiles_y;
    const int first = deal.first(vb);
    const int last = min(first + deal.count(vb), ntiles);
    const double inv_nm1 = 1.0 / ((double)G::T.taps - 1.0);
    const int rmin = max(0, p.in_row0), rmax = min(p.gny, p.in_row0 + p.in_rows);
    const bool stager = wave < SW;
    const int scol = 128 * wave + 2 * lane;  // a staging lane's first staged column (and the next one)
    int seen_tiles = 0, seen_frac = 0;
#if WIDE_STAMPS
    uint32_t ts_n = 0, ts_all = 0, ts_drain = 0, ts_bar = 0, ts_pair = 0, ts_prev = 0, ts_nsw = 0, ts_lead = 0;
#endif

#pragma unroll 1
    for (int pos = first; pos < last;) {
        const int tile0 = pos;
        const int ty0 = tile0 % tiles_y;
        const int run_tiles = min(last - tile0, tiles_y - ty0);
        const int strip = tile0 / tiles_y;
        const int nphase = run_tiles * PPT;
        const int ox0 = strip * G::TILE_W;
        const int oyS = (p.out_row0 / C::TH + ty0) * C::TH;
        const int gx0 = ox0 - G::X0;
        // stream row n is DEM row gy0 + n, in ring slot n % R
        const int gy0 = oyS - G::M - C::PAD;
        const int gcol = gx0 + scol;  // even, and nx % 4 == 0: the lane's two columns are both inside or both outside
        const bool col_ok = stager && gcol >= 0 && gcol < p.nx;
        const float* src = p.in + (col_ok ? gcol : 0);
        // A batch is INTERIOR when its B rows all lie in the raster; the staging takes it on a lean path when, besides, every
        // lane of the wave has its columns in the raster and the batch's slots do not wrap the ring: wave-uniform conditions,
        // one branch a batch, and then no row needs a clamp, a test, a multiplication or a slot wrap of its own.  On the
        // bench DEM that is every batch but a run's first and last ones and the last strip's.
        // (The lean path leans on two empty asm statements in load_batch that only hold the optimiser back: the opaque row
        // base and the statement behind the loads.  What they buy is a property of the compiled code, not of the source:
        // after a compiler update run tools/valu_bound.py wide and tools/spill_survey.py tpi_ring_wide_kernel again - the
        // tool asserts the loads' form, the rows without branch, select, compare, convert back or multiplication, and the
        // size of the chain waves' loop, reloads of spilled registers included.)
        constexpr bool kLean = WIDE_LEAN || WIDE_STAGE_CEILING;
        const bool cols_in = kLean && __builtin_amdgcn_ballot_w64(col_ok) == ~0ull;
        const uint32_t voff = (uint32_t)(col_ok ? gcol : 0) * 4u;
        auto load_batch = [&](int n0, float2 (&v)[B]) {
            const int g0 = gy0 + n0;
            if (kLean && g0 >= rmin && g0 + B <= rmax && p.nx < (1 << 29)) {  // (a lane's byte offset in a row: 32 bits)
                // interior rows: one scalar row base a batch that runs on by the pitch, the lane's offset beside it.  (The base
                // is opaque in every row: the address stays scalar base + 32-bit lane offset, which is the load's own form,
                // where the compiler would hoist base + lane offset as a 64-bit vector and add the rows to that.)
                uint64_t rowa = reinterpret_cast<uint64_t>(p.in) + (uint64_t)(g0 - p.in_row0) * (uint64_t)p.nx * sizeof(float);
                uint32_t vo = voff;
                asm("" : "+v"(vo));
#pragma unroll
                for (int r = 0; r < B; ++r) {
                    asm("" : "+s"(rowa));
                    const u32x2w t = *reinterpret_cast<glb_u32x2w*>(rowa + vo);
                    v[r] = make_float2(__uint_as_float(t.x), __uint_as_float(t.y));
                    rowa += (uint64_t)p.nx * sizeof(float);
                }
                // (the compiler would sink these loads into one block with the general path's below, behind a 64-bit vector
                // address for each: with this in their way they stay here, scalar base and 32-bit lane offset)
                asm volatile("");
                return;
            }
#pragma unroll
            for (int r = 0; r < B; ++r) {
                int gy = g0 + r;
                gy = min(max(gy, rmin), rmax - 1);  // a clamped row is read and thrown away
                v[r] = *reinterpret_cast<const float2*>(src + (size_t)(gy - p.in_row0) * p.nx);
            }
        };
        uint32_t run0 = 0, run1 = 0;  // running prefixes of the lane's two columns (wrap, harmlessly)
        int wslot = 0;                // ring slot of the next row to stage
        // (stagers) one batch: convert, classify, prefix, write.  Returns kBad when the batch holds a sample the chain cannot
        // take (fractional, non-finite or absurd) and kFracOnly when it holds fractional samples and no non-finite or absurd
        // one (what the dem_memo report counts, like the marching kernel, which counts no tile it leaves for such samples)
        auto stage_batch = [&](int n0, const float2 (&v)[B]) {
            WideClassAcc cls;  // the lane's samples of the batch: fractional parts ORed, largest magnitude (wide_classify.hpp)
            // one row's two samples: classified, added to the running prefixes; the row's ring entry
            auto take = [&](float x0, float x1) {
                const int i0 = (int)x0, i1 = (int)x1;
#if !WIDE_STAGE_CEILING
                wide_classify_row(cls, x0, x1);
#endif
                run0 += (uint32_t)i0;
                run1 += (uint32_t)i1;
                const u32x2w v2 = {run0, run1};
                return v2;
            };
            const int g0 = gy0 + n0;
            if (cols_in && g0 >= rmin && g0 + B <= rmax && wslot + B <= R) {
                uint32_t* q = Q + wslot * G::W + scol;  // the batch's slots are wslot + r: one address, immediate offsets
#pragma unroll
                for (int r = 0; r < B; ++r) *reinterpret_cast<u32x2w*>(q + r * G::W) = take(v[r].x, v[r].y);
            } else {
#pragma unroll
                for (int r = 0; r < B; ++r) {
                    const int gy = g0 + r;
                    const bool ok = col_ok && gy >= rmin && gy < rmax;
                    int sl = wslot + r;
                    sl = sl >= R ? sl - R : sl;
                    // padding is staged as zero (mode="same")
                    *reinterpret_cast<u32x2w*>(Q + sl * G::W + scol) = take(ok ? v[r].x : 0.0f, ok ? v[r].y : 0.0f);
                }
            }
            // The guard copies, in the same batch and so behind the same barrier as their source slots: a chain wave reads
            // slot R + s only in a window that holds slot s, which the staging then does not write.  The batch's slots
            // below GR are glo .. ghi - 1 - its first ones when it starts there, the ones behind the wrap when it wraps -
            // and few batches have any: one wave-uniform test a batch, and the lane copies its own entries of those slots
            // (written above: a wave's LDS operations keep their order) with the slot clamped on the scalar side, so that no
            // row has a branch of its own.
            const int glo = wslot < C::GR ? wslot : 0;
            const int ghi = wslot < C::GR ? C::GR : min(wslot + B - R, C::GR);
            if (glo < ghi) {
#pragma unroll
                for (int g = 0; g < C::GR; ++g) {
                    const int sl = min(max(g, glo), ghi - 1);
                    *reinterpret_cast<u32x2w*>(Q + (sl + R) * G::W + scol) = *reinterpret_cast<const u32x2w*>(Q + sl * G::W + scol);
                }
            }
#if WIDE_STAGE_CEILING
            return 0;
#else
            // |trunc(x)| <= kAbsLim  <=>  |x| < kAbsLim + 1
            return wide_classify_batch(cls, kAbsLim + 1.0f, kBad, kFracOnly);
#endif
        };
        auto advance_wslot = [&]() {
            wslot += B;
            wslot = wslot >= R ? wslot - R : wslot;
        };
        // bit k: batch (newest - k) holds a sample the chain cannot take; bit 15 + k: it holds a fractional sample (the
        // report only) - the flag word's two fields, shifted together
        unsigned hist = 0;
        auto fold = [&](int parity, auto AT_ONCE) {
            int f[SW];
#pragma unroll
            for (int w = 0; w < SW; ++w) f[w] = wflags[parity * SW + w];
            // (the chain waves with WIDE_BOUNDARY: all the words read before any is combined - one round trip to LDS behind the
            // barrier, not one a read, and one OR of three)
            static_assert(SW == 3, "the flag words of the staging waves, held at once");
            if constexpr (decltype(AT_ONCE)::value) asm("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]));
            int all = 0;
#pragma unroll
            for (int w = 0; w < SW; ++w) all |= f[w];
            all = __builtin_amdgcn_readfirstlane(all);
            hist = ((hist << 1) | (unsigned)all) & kHistMask;
        };

        const int ocol = gx0 + lane * NCW;
        // pair P of the lane's columns is stored when it lies among the strip's valid columns (WGeo::XV: the whole lanes, the
        // last pair of the lane in front of them and the first pair of the lane behind) and in the raster (nx % 4 == 0, ocol
        // even: a pair is inside or outside).  Invariant over the run: masks in scalar registers, no test in the phase loop.
        bool pair_ok[NCW / 2];
        bool lane_ok = false;
#pragma unroll
        for (int P = 0; P < NCW / 2; ++P) {
            pair_ok[P] = lane * NCW + 2 * P >= G::XV && lane * NCW + 2 * P < G::W - G::XV && ocol + 2 * P < p.nx;
            lane_ok = lane_ok || pair_ok[P];
        }
        __syncthreads();  // (the previous run's chain waves are done with the ring and the flag words)
        // The run's prologue and phases, once for the staging waves and once for the chain waves: the same barriers on both
        // sides, and the batch a staging wave holds in registers from one phase to the next (va) is no live value in the
        // chain waves' loop, whose sweep needs those registers.
        auto run_phases = [&](auto STG) {
        constexpr bool stg = decltype(STG)::value;
        float2 va[stg ? B : 1];
        if constexpr (stg) {
            int bits = 0;
#pragma unroll 1
            for (int k = 0; k < NB_PRO; ++k) {
                load_batch(k * B, va);
                bits |= stage_batch(k * B, va) << (NB_PRO - 1 - k);
                advance_wslot();
            }
            if (lane == 0) wflags[wave] = bits;
            load_batch(C::PRO, va);
        } else {
            for (int k = 0; k < NB_PRO; ++k) advance_wslot();
        }
        __syncthreads();
        {
            int all = 0;
#pragma unroll
            for (int w = 0; w < SW; ++w) all |= wflags[w];
            hist = (unsigned)__builtin_amdgcn_readfirstlane(all) & kHistMask;
        }

        // A chain wave's pair of the phase (WIDE_BOUNDARY): its first row, that row's offset in the output plane and the byte
        // offset of the ring slot of Q index 0 of its window go on from phase to phase by scalar increments, and the rows and
        // bases of the lead fetches live across the barrier.
        using PT = WPair<SIZE, C::GR>;
        constexpr uint32_t PB = (uint32_t)G::W * 4, RB = (uint32_t)R * PB;
        constexpr bool kAhead = !stg && WIDE_BOUNDARY != 0;
        static_assert(C::RPW == 2, "a chain wave sums its two rows of a phase in one sweep");
        static_assert(!kAhead || PT::template lead_is_published<WIDE_LEAD, B>(),
                      "the lead fetches read rows published a barrier earlier");
        static_assert(C::PAD - 1 + B - C::RPW < R, "a run's first slots need no wrap");
        const int pj = stg ? 0 : (wave - SW) * C::RPW;  // first row of the pair in the phase
        [[maybe_unused]] int py = oyS + pj;
        [[maybe_unused]] long long prow = (long long)(py - p.out_row0) * p.nx;
        [[maybe_unused]] uint32_t pb0 = (uint32_t)(C::PAD - 1 + pj) * PB;
        [[maybe_unused]] u32x2w row[PT::lead_rows(WIDE_LEAD)][3];
        [[maybe_unused]] uint32_t vbase[PT::lead_bases(WIDE_LEAD)];
        if constexpr (kAhead) {
            if (nphase > 0) wide_pair_lead<SIZE, R, C::GR, WIDE_LEAD>(Q, pb0, lane, row, vbase);
        }
#if WIDE_STAMPS
        [[maybe_unused]] uint32_t t_sweep = 0;
#endif
        // one row of the pair: finalised as tpi_march_kernel does, stored by pairs of columns
        [[maybe_unused]] auto store_row = [&](bool row_ok, long long off, const uint32_t (&acc_k)[NCW],
                                              const uint32_t (&ctr_k)[NCW]) {
            if (lane_ok && row_ok) {
                float out_t[NCW];
#pragma unroll
                for (int t = 0; t < NCW; ++t) {
                    const int xi = (int)ctr_k[t];  // integers: see tpi_march_kernel
                    out_t[t] = (float)((double)xi - (double)((int)acc_k[t] - xi) * inv_nm1);
                }
                // (the row's six values are formed HERE, under the one test of lane and row: left to itself the compiler sinks
                // each pair's float64 arithmetic behind that pair's mask, a branch a pair)
#pragma unroll
                for (int t = 0; t < NCW; ++t) asm volatile("" : "+v"(out_t[t]));
#pragma unroll
                for (int P = 0; P < NCW / 2; ++P)
                    if (__builtin_expect(pair_ok[P], true))  // (the address per pair: ocol < 0 in the lane in front of strip 0)
                        *reinterpret_cast<float2*>(p.tpi + (off + ocol + 2 * P)) = make_float2(out_t[2 * P], out_t[2 * P + 1]);
            }
        };

        bool tile_frac = false;
#pragma unroll 1
        for (int ph = 0; ph < nphase; ++ph) {
            const bool compute = (hist & kWindow) == 0;
            const int oyA = oyS + ph * B;
            tile_frac = tile_frac || (hist & (kWindow * kFracOnly)) != 0;
            if (!compute) {
                // the tiles of the marching geometry that this phase's output rows overlap go to the scaled pass
                const int r0 = max(oyA, p.out_row0), r1 = min(oyA + B, p.out_row0 + p.out_rows) - 1;
                if (r0 <= r1 && threadIdx.x == 0) {
                    const int base = p.out_row0 / p.map_th;
                    const int mx0 = ox0 / p.map_tw, mx1 = (min(ox0 + G::TILE_W, p.nx) - 1) / p.map_tw;
                    for (int mx = mx0; mx <= mx1; ++mx)
                        for (int my = r0 / p.map_th; my <= r1 / p.map_th; ++my) p.defer[mx * p.map_tiles_y + (my - base)] = kNeedsFraction;
                }
            }
            if (ph % PPT == PPT - 1) {
                ++seen_tiles;
                seen_frac += tile_frac ? 1 : 0;
                tile_frac = false;
            }
            if constexpr (stg) {
                // the batch phase ph + 1 needs, into the slots behind this phase's window; then the loads of the one after
                // (WIDE_PRIO: on top of the chain waves' ladder from the barrier until the flags are written, then back to 0
                // for the loads and the wait at the barrier.  s_setprio ignores EXEC: both stand on this wave-uniform path,
                // outside lane 0's store)
                if constexpr (WIDE_PRIO != 0) CHAIN_SETPRIO(3);
                const int seen = stage_batch(C::PRO + ph * B, va);
                if (lane == 0) wflags[((ph + 1) & 1) * SW + wave] = seen;
                if constexpr (WIDE_PRIO != 0) CHAIN_SETPRIO(0);
                load_batch(C::PRO + (ph + 1) * B, va);
            } else if (compute) {
                if constexpr (kAhead) {
                    // A pair with a row in the output range is summed whole and the other row's store masked: no branch inside
                    // the sweep.  The masked row reads ring rows of this phase's window like its partner, and the staging has
                    // written the whole window of a phase that is computed (rows outside the raster as zeros).
                    if (py + C::RPW > p.out_row0 && py < p.out_row0 + p.out_rows) {
                        uint32_t acc[C::RPW][NCW], ctr[C::RPW][NCW];
                        wide_pair_sum<SIZE, R, C::GR, WIDE_LEAD, WIDE_PRIO != 0, true>(Q, pb0, lane, row, vbase, acc, ctr
#if WIDE_STAMPS
                                                                                       , t_sweep
#endif
                        );
#pragma unroll
                        for (int k = 0; k < C::RPW; ++k)
                            store_row(py + k >= p.out_row0 && py + k < p.out_row0 + p.out_rows, prow + (long long)k * p.nx,
                                      acc[k], ctr[k]);
#if WIDE_STAMPS
                        if (ph > 0) ts_nsw += 1, ts_lead += t_sweep - ts_prev;
#endif
                    }
                } else {
                    // (round 13's phase: slot, rows and lead fetches formed here, behind the barrier)
                    const int oy = oyA + pj;
                    if (oy + C::RPW > p.out_row0 && oy < p.out_row0 + p.out_rows) {
                        const int s0 = (C::PAD - 1 + ph * B + pj) % R;  // slot of Q index 0 of the first row's window
                        uint32_t acc[C::RPW][NCW], ctr[C::RPW][NCW];
                        wide_pair_sum<SIZE, R, C::GR, WIDE_LEAD, WIDE_PRIO != 0, false>(Q, (uint32_t)s0 * PB, lane, row, vbase, acc, ctr
#if WIDE_STAMPS
                                                                                        , t_sweep
#endif
                        );
#pragma unroll
                        for (int k = 0; k < C::RPW; ++k)
                            store_row(oy + k >= p.out_row0 && oy + k < p.out_row0 + p.out_rows, (long long)(oy + k - p.out_row0) * p.nx,
                                      acc[k], ctr[k]);
#if WIDE_STAMPS
                        if (ph > 0) ts_nsw += 1, ts_lead += t_sweep - ts_prev;
#endif
                    }
                }
            }
            advance_wslot();
#if WIDE_STAMPS
            const uint32_t t0 = wide_now();
            if constexpr (!stg && WIDE_STAMPS == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t t1 = wide_now();
#endif
            if constexpr (kAhead) {
                // the next phase's pair: its state by increments (one conditional subtract for the ring's wrap), then its lead
                // fetches - rows that earlier barriers published (lead_is_published) - so that the sweep behind the barrier
                // starts on registers already loading.  The run's last phase fetches nothing.
                py += B;
                prow += (long long)B * p.nx;
                pb0 += (uint32_t)B * PB;
                pb0 = pb0 >= RB ? pb0 - RB : pb0;
                if (ph + 1 < nphase) {
                    wide_pair_lead<SIZE, R, C::GR, WIDE_LEAD>(Q, pb0, lane, row, vbase);
                } else {
                    // (no instruction: the registers get new, undefined values, so that the ones the sweep has consumed are
                    // dead behind it - else they would count as live round the loop on this path and be spilled over the sweep)
#pragma unroll
                    for (int n = 0; n < PT::lead_rows(WIDE_LEAD); ++n)
#pragma unroll
                        for (int h = 0; h < 3; ++h) asm volatile("" : "=v"(row[n][h]));  // (volatile: one value each)
#pragma unroll
                    for (int b = 0; b < PT::lead_bases(WIDE_LEAD); ++b) asm volatile("" : "=v"(vbase[b]));
                }
                // A chain wave writes nothing to LDS, so it has nothing to release: it crosses the barrier bare, with no wait
                // for the reads just issued (__syncthreads would put s_waitcnt lgkmcnt(0) here and hand their latency to
                // the last wave to arrive).  The ring and flag reads behind it stay behind it: the statement clobbers memory,
                // and a wave's LDS operations are carried out in the order issued.  The sweep's own reads have all been
                // waited for by the finalisation, so the staging waves may write their slots behind this barrier as before.
                asm volatile("s_barrier" ::: "memory");
            } else {
                __syncthreads();
            }
#if WIDE_STAMPS
            const uint32_t t2 = wide_now(), t3 = wide_now();
            if (ph > 0) {  // (a run's first phase has no phase before it to measure from)
                ts_n += 1;
                ts_all += t2 - ts_prev;
                ts_drain += t1 - t0;
                ts_bar += t2 - t1;
                ts_pair += t3 - t2;
            }
            ts_prev = t2;
#endif
            fold((ph + 1) & 1, std::bool_constant<kAhead>{});
        }
        if constexpr (stg) {
            // The last phase's loads (the batch behind the run, clamped rows, never staged) are taken up HERE, so that no
            // load is in flight where this path meets the chain waves' at the top of the run loop.  The compiler's wait
            // counts are per program point, not per wave: with these sixteen loads open at that point it guards every
            // write of one of their registers (v10 .. v41, which the sweep reuses) in the CHAIN waves' phase loop as well -
            // s_waitcnt vmcnt(0) in front of the phase barrier and vmcnt(12), (7), (0) at the sweep's start.  A chain wave
            // has no load in flight, only its six output stores of the phase, and so waited out their round trip in
            // every phase with nothing to overlap it.  One wait per run of the staging waves instead.
#pragma unroll
            for (int r = 0; r < B; ++r) asm volatile("" ::"v"(va[r].x), "v"(va[r].y));
        }
        };
        if (stager) run_phases(std::true_type{});
        else run_phases(std::false_type{});
        pos += run_tiles;
    }
#if WIDE_STAMPS
    static_assert(WideCfg<SIZE>::NW == kWideStampWaves, "one record per wave");
    if (lane == 0 && (vb == 0 || vb == nb / 2)) {
        unsigned long long* o = wide_stamps[vb == 0 ? 0 : 1][wave];
        o[0] = (unsigned long long)ts_n, o[1] = (unsigned long long)ts_all, o[2] = (unsigned long long)ts_drain;
        o[3] = (unsigned long long)ts_bar, o[4] = (unsigned long long)ts_pair;
        o[5] = (unsigned long long)ts_nsw, o[6] = (unsigned long long)ts_lead;
    }
#endif
    if (p.report != nullptr && vb == nb / 2 && threadIdx.x == 0) {
        __hip_atomic_store(p.report + 1, (uint32_t)seen_frac, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p.report, (uint32_t)seen_tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The wide ring's pass over a single block: clears the marching geometry's tile map (map_th x map_tw), then marks in it
// the tiles the scaled pass and the general kernel are to take.
template <int SIZE>
int launch_ring_wide(const Block& b, float* tpi_out, int map_th, int map_tw) {
    using G = WGeo<SIZE>;
    using C = WideCfg<SIZE>;
    Context& c = ctx();
    TOPO_REQUIRE(c.seams.n == 0, "the wide ring takes single-block calls only");
    WaveArgs a = wave_args(b, tpi_out, nullptr);
    a.report = dem_memo_report(b);
    static int blocks_per_cu = 0;
    const auto clear_map = [&](WaveParts& ps, long) -> int {
        TOPO_REQUIRE(ps.n == 1 && ps.a[0].map_th == map_th && ps.a[0].map_tw == map_tw, "wide ring: tile map of another geometry");
        const size_t map_bytes = (size_t)((b.nx + map_tw - 1) / map_tw) * ps.a[0].map_tiles_y;
        TOPO_HIP(hipMemsetAsync(ps.a[0].defer, kTileDone, map_bytes, c.compute));
        return TOPO_AMD_OK;
    };
    return launch_tiles(tpi_ring_wide_kernel<SIZE>, nullptr, &blocks_per_cu, C::NW * 64, C::LDS, 0, b, a, C::TH, G::TILE_W, true, false,
                        map_th, map_tw, clear_map);
}

}  // namespace

}  // namespace topo
