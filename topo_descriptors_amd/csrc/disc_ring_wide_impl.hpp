// K1 wide ring: TPI of the large discs with 6 columns per lane, staging waves apart from chain waves.
//
// tpi_march_kernel<67> (disc_wave_impl.hpp) is bound by vector-ALU issue: 315 instructions per wave-row, of which the
// 18 run-in lanes of a 4-column layout waste 28 % (46 of 64 lanes write a sum) and the lane hops - 17 DPP forms per
// output column, every one at half rate - a further fifth (profiles/r06_tpi67_valu_bound.json).  Here:
//
//   * a lane owns NCW = 6 adjacent columns: 6 lane hops per side for 67 px, 52 of 64 lanes valid (312 of 384 staged
//     columns), the chain two-sided and rim first as in ring_disc_sum (disc_ring_impl.hpp);
//   * a ring row is 384 dwords (1.5 KiB), staged column c at dword c: lane l reads its 6 columns as three ds_read_b64 at
//     +0, +8 and +16 from byte 24 l (dwords 6 l, 6 l + 1 of the 32 lanes of a group are distinct mod 64: conflict-free);
//   * the ring holds R = SIZE + 32 rows plus GR = 6 guard rows behind them, copies of slots 0 .. GR - 1 (WideCfg), so
//     that one VGPR address at slot (s0 + k) mod R reaches the rows k .. k + GR of the window by immediate offsets: nine
//     addresses a row (WBase) instead of one per read;
//   * the staging runs on waves of its own (std_ring_spec_kernel's structure):
//     waves 0-2 convert, classify and write batch ph + 1 (16 rows, two columns per lane, 8-byte loads) and issue the
//     loads of batch ph + 2 while waves 3-10 run two output rows each of phase ph; ONE barrier per phase;
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

namespace topo {

namespace {

constexpr int NCW = 6;  // columns per lane of the wide ring

template <int SIZE>
struct WGeo {
    static constexpr DiscTable<SIZE> T = make_disc_table<SIZE>();
    static_assert(T.centre == 0 && T.off_min == -T.off_max, "odd disc sizes only");
    static constexpr int M = T.off_max;
    static constexpr int DL = (M + NCW - 1) / NCW;  // lane hops per side
    static constexpr int NVL = 64 - 2 * DL;         // lanes that end up with full sums
    static constexpr int TILE_W = NCW * NVL;        // valid output columns per strip
    static constexpr int X0 = NCW * DL;             // staged column of the first valid output
    static constexpr int W = 64 * NCW;              // staged columns = dwords per ring row
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

// The VGPR addresses of a row's prefix-row reads.  The chain reads run r at Q indices top = run_hi + 1 + M and
// bot = run_lo + M, in the order WGeo::S.order.  A base at Q index kb is the one VGPR 24 lane + ((s0 + kb) mod R) PB; a read
// at k with kb <= k <= kb + GR is that base plus the immediate (k - kb) PB (+0, +8, +16): it lands in slot
// (s0 + kb) mod R + k - kb <= R - 1 + GR, a guard row where the ring wraps.  The bases cover the read indices greedily from
// the smallest, and each is formed at the first fetch that needs it (so it lives only over its stretch of the sweep).
template <int SIZE, int GR>
struct WBase {
    using G = WGeo<SIZE>;
    static constexpr int NR = G::NR;
    struct Tab {
        int nb;           // bases
        int kb[2 * SIZE]; // Q index of base b
        int first[2 * SIZE];  // fetch (index into S.order) that forms base b
        int top_b[SIZE], bot_b[SIZE];  // per fetch i: base of the top / bottom read
        int top_k[SIZE], bot_k[SIZE];  // per fetch i: Q index of the top / bottom read
    };
    static constexpr Tab make() {
        Tab t{};
        bool need[2 * SIZE + 2] = {};
        for (int i = 0; i < NR; ++i) {
            const int r = G::S.order[i];
            t.top_k[i] = G::T.run_hi[r] + 1 + G::M;
            t.bot_k[i] = G::T.run_lo[r] + G::M;
            need[t.top_k[i]] = need[t.bot_k[i]] = true;
        }
        t.nb = 0;
        for (int k = 0; k <= 2 * G::M + 1; ++k)
            if (need[k] && (t.nb == 0 || k > t.kb[t.nb - 1] + GR)) t.kb[t.nb++] = k;
        for (int b = 0; b < t.nb; ++b) t.first[b] = NR;
        auto base_of = [&](int k) {
            int b = 0;
            while (b + 1 < t.nb && t.kb[b + 1] <= k) ++b;
            return b;
        };
        for (int i = 0; i < NR; ++i) {
            t.top_b[i] = base_of(t.top_k[i]);
            t.bot_b[i] = base_of(t.bot_k[i]);
            if (i < t.first[t.top_b[i]]) t.first[t.top_b[i]] = i;
            if (i < t.first[t.bot_b[i]]) t.first[t.bot_b[i]] = i;
        }
        return t;
    }
    static constexpr Tab T = make();
    static constexpr bool check() {
        for (int i = 0; i < NR; ++i)
            if (T.top_k[i] - T.kb[T.top_b[i]] > GR || T.top_k[i] < T.kb[T.top_b[i]] || T.bot_k[i] - T.kb[T.bot_b[i]] > GR ||
                T.bot_k[i] < T.kb[T.bot_b[i]])
                return false;
        return true;
    }
    static_assert(check(), "every read within GR rows of its base");
};

#ifndef WIDE_LEAD
#define WIDE_LEAD 2
#endif
#ifndef WIDE_PRIO
#define WIDE_PRIO 1
#endif

typedef uint32_t u32x2w __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const char lds_char;
typedef __attribute__((address_space(3))) const volatile u32x2w lds_u32x2w;

// Disc sums of one output row (ring_disc_sum with 6 columns per lane): s0 is the ring slot of the row's Q index 0,
// acc[t] the sum for the lane's column NCW lane + t (valid for DL <= lane < 64 - DL), ctr[t] that pixel's own value.
// FIRST (WIDE_PRIO): the wave's first row of the phase - its issue priority goes 3 -> 2 over that row and 1 -> 0 over the
// second (CHAIN_PRIO, disc_wave_impl.hpp), so that the two chain waves of a SIMD advance together.  A template argument,
// so that no branch splits the chain: a DPP move and the add it feeds fold into one DPP add only within a basic block.
template <int SIZE, int R, int GR, int LEAD, bool FIRST>
__device__ __forceinline__ void wide_disc_sum(const uint32_t* ring, int s0, int lane, uint32_t (&acc)[NCW], uint32_t (&ctr)[NCW]) {
    using G = WGeo<SIZE>;
    using BT = WBase<SIZE, GR>;
    constexpr int NR = G::NR;
    constexpr int DL = G::DL;
    constexpr int M = G::M;
    constexpr uint32_t PB = (uint32_t)G::W * 4;  // bytes per ring row
    constexpr uint32_t RB = (uint32_t)R * PB;
    u32x2w top[NR][3], bot[NR][3];
    uint32_t cv[NR][NCW];
    uint32_t aR[NCW], aL[NCW];
    uint32_t vb[BT::T.nb];
    lds_char* q = (lds_char*)ring;
    const uint32_t b0 = (uint32_t)s0 * PB, lb = (uint32_t)lane * (NCW * 4);
    auto fetch = [&](int i) {
        const int r = G::S.order[i];
#pragma unroll
        for (int b = 0; b < BT::T.nb; ++b)
            if (BT::T.first[b] == i) {
                const uint32_t d = b0 + (uint32_t)BT::T.kb[b] * PB;
                vb[b] = lb + min(d, d - RB);  // the scalar wrap, then one vector add
                asm("" : "+v"(vb[b]));        // (opaque: every read of the base keeps it and takes an immediate offset)
            }
        lds_char* pt = q + vb[BT::T.top_b[i]] + (uint32_t)(BT::T.top_k[i] - BT::T.kb[BT::T.top_b[i]]) * PB;
        lds_char* pb = q + vb[BT::T.bot_b[i]] + (uint32_t)(BT::T.bot_k[i] - BT::T.kb[BT::T.bot_b[i]]) * PB;
        // (volatile: three ds_read_b64, not merged into ds_read2_b64, which banks 32 wide and moves half as many bytes a cycle)
#pragma unroll
        for (int h = 0; h < 3; ++h) top[r][h] = *(lds_u32x2w*)(pt + 8 * h);
#pragma unroll
        for (int h = 0; h < 3; ++h) bot[r][h] = *(lds_u32x2w*)(pb + 8 * h);
    };
#pragma unroll
    for (int i = 0; i < LEAD && i < NR; ++i) fetch(i);
#if WIDE_PRIO
    if (FIRST) CHAIN_SETPRIO(3);
    else CHAIN_SETPRIO(1);
#endif
    static_assert(DL >= 1, "the last step (D = 0) closes both chains");
#pragma unroll
    for (int D = DL; D >= 0; --D) {
#if WIDE_PRIO
        if (D == DL / 2) {
            if (FIRST) CHAIN_SETPRIO(2);
            else CHAIN_SETPRIO(0);
        }
#endif
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (G::S.first_step[G::S.order[j]] == D) {
                const int r = G::S.order[j];
                if (j + LEAD < NR) fetch(j + LEAD);
                RING_SB();
#pragma unroll
                for (int s = 0; s < NCW; ++s) cv[r][s] = top[r][s / 2][s % 2] - bot[r][s / 2][s % 2];
                RING_SB();
            }
        }
#pragma unroll
        for (int t = 0; t < NCW; ++t) {
            uint32_t pr = 0, pl = 0;
            bool anyr = false, anyl = false;
#pragma unroll
            for (int s = 0; s < NCW; ++s) {
                const int dr = NCW * D + s - t;
                const int dl = -NCW * D + s - t;
                if (dr >= 0 && dr <= M) {
                    const uint32_t c = cv[G::T.run_of[dr - G::T.off_min]][s];
                    pr = anyr ? pr + c : c;
                    anyr = true;
                }
                if (dl < 0 && dl >= -M) {
                    const uint32_t c = cv[G::T.run_of[dl - G::T.off_min]][s];
                    pl = anyl ? pl + c : c;
                    anyl = true;
                }
            }
            if (D == DL) {
                aR[t] = pr;
                aL[t] = pl;
            } else if (D == 0) {
                // the last step and the final aR + aL as one plain add and two DPP adds: hop(aR) + (hop_up(aL) + (pr + pl))
                uint32_t own = anyr && anyl ? pr + pl : anyr ? pr : pl;
                asm("" : "+v"(own));
                own = hop_up(aL[t]) + own;
                asm("" : "+v"(own));
                aR[t] = hop(aR[t]) + own;  // the disc sum
                asm("" : "+v"(aR[t]));     // (here, beside its DPP move, not sunk behind the caller's lane test)
            } else {
                // (the lane's own part opaque: the DPP move folds into a two-operand add, see ring_disc_sum)
                if (anyr) {
                    asm("" : "+v"(pr));
                    aR[t] = hop(aR[t]) + pr;
                } else {
                    aR[t] = hop(aR[t]);
                }
                if (anyl) {
                    asm("" : "+v"(pl));
                    aL[t] = hop_up(aL[t]) + pl;
                } else {
                    aL[t] = hop_up(aL[t]);
                }
            }
        }
        RING_SB();
    }
#pragma unroll
    for (int t = 0; t < NCW; ++t) {
        acc[t] = aR[t];
        ctr[t] = cv[G::S.centre_run][t];
    }
}


template <int SIZE>
__global__ __launch_bounds__(WideCfg<SIZE>::NW * 64) void tpi_ring_wide_kernel(WaveArgs p, int tiles_x, int tiles_y, PartRun deal) {
    using G = WGeo<SIZE>;
    using C = WideCfg<SIZE>;
    constexpr int B = C::B, R = C::R, PPT = C::PPT, SW = C::SW, NB_PRO = C::NB_PRO, DL = G::DL;
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
        auto load_batch = [&](int n0, float2 (&v)[B]) {
#pragma unroll
            for (int r = 0; r < B; ++r) {
                int gy = gy0 + n0 + r;
                gy = min(max(gy, rmin), rmax - 1);  // a clamped row is read and thrown away
                v[r] = *reinterpret_cast<const float2*>(src + (size_t)(gy - p.in_row0) * p.nx);
            }
        };
        uint32_t run0 = 0, run1 = 0;  // running prefixes of the lane's two columns (wrap, harmlessly)
        int wslot = 0;                // ring slot of the next row to stage
        // (stagers) one batch: convert, classify, prefix, write.  Returns kBad when the batch holds a sample the chain cannot
        // take (fractional, non-finite or absurd) and kFracOnly when it holds fractional samples and no non-finite or absurd
        // one (what the dem_memo report counts, like the marching kernel, which counts no tile it leaves for such samples)
        const uint32_t kLimBits = __float_as_uint(kAbsLim + 1.0f);  // |trunc(x)| <= kAbsLim  <=>  |x| < kAbsLim + 1
        auto stage_batch = [&](int n0, const float2 (&v)[B]) {
            uint32_t amax = 0;  // largest |x| seen, as float bits (NaN / inf sort above all)
            bool frac = false;
#pragma unroll
            for (int r = 0; r < B; ++r) {
                const int gy = gy0 + n0 + r;
                const bool ok = col_ok && gy >= rmin && gy < rmax;
                const float x0 = ok ? v[r].x : 0.0f, x1 = ok ? v[r].y : 0.0f;  // padding is staged as zero (mode="same")
                const int i0 = (int)x0, i1 = (int)x1;
                const uint32_t a0 = __float_as_uint(x0) & 0x7fffffffu, a1 = __float_as_uint(x1) & 0x7fffffffu;
                frac |= x0 != (float)i0 || x1 != (float)i1;
                amax = max(amax, max(a0, a1));
                run0 += (uint32_t)i0;
                run1 += (uint32_t)i1;
                int sl = wslot + r;
                sl = sl >= R ? sl - R : sl;
                const u32x2w v2 = {run0, run1};
                *reinterpret_cast<u32x2w*>(Q + sl * G::W + scol) = v2;
                // the guard copy, in the same batch and so behind the same barrier as its source slot: a chain wave reads
                // slot R + s only in a window that holds slot s, which the staging then does not write
                if (sl < C::GR) *reinterpret_cast<u32x2w*>(Q + (sl + R) * G::W + scol) = v2;
            }
            // (in a batch without non-finite or absurd samples, x != (float)(int)x is a fractional part)
            const bool wild = __builtin_amdgcn_ballot_w64(amax >= kLimBits) != 0;
            const bool any_frac = __builtin_amdgcn_ballot_w64(frac) != 0;
            const bool bad = wild || any_frac;
            const bool fr = !wild && any_frac;
            return (bad ? kBad : 0) | (fr ? kFracOnly : 0);
        };
        auto advance_wslot = [&]() {
            wslot += B;
            wslot = wslot >= R ? wslot - R : wslot;
        };
        // bit k: batch (newest - k) holds a sample the chain cannot take; bit 15 + k: it holds a fractional sample (the
        // report only) - the flag word's two fields, shifted together
        unsigned hist = 0;
        auto fold = [&](int parity) {
            int all = 0;
#pragma unroll
            for (int w = 0; w < SW; ++w) all |= wflags[parity * SW + w];
            all = __builtin_amdgcn_readfirstlane(all);
            hist = ((hist << 1) | (unsigned)all) & kHistMask;
        };

        float2 va[B];
        __syncthreads();  // (the previous run's chain waves are done with the ring and the flag words)
        if (stager) {
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

        const int ocol = gx0 + lane * NCW;
        const bool lane_ok = lane >= DL && lane < DL + G::NVL && ocol < p.nx;
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
            if (stager) {
                // the batch phase ph + 1 needs, into the slots behind this phase's window; then the loads of the one after
                const int seen = stage_batch(C::PRO + ph * B, va);
                if (lane == 0) wflags[((ph + 1) & 1) * SW + wave] = seen;
                load_batch(C::PRO + (ph + 1) * B, va);
            } else if (compute) {
                static_assert(C::RPW == 2, "two rows per chain wave: the first and the second priority pair");
#pragma unroll
                for (int k = 0; k < C::RPW; ++k) {
                    const int j = (wave - SW) * C::RPW + k;  // row of the phase
                    const int oy = oyA + j;
                    if (oy < p.out_row0 || oy >= p.out_row0 + p.out_rows) continue;
                    const int s0 = (C::PAD - 1 + ph * B + j) % R;  // slot of Q index 0 of the row's window
                    uint32_t acc[NCW], ctr[NCW];
                    if (k == 0) wide_disc_sum<SIZE, R, C::GR, WIDE_LEAD, true>(Q, s0, lane, acc, ctr);
                    else wide_disc_sum<SIZE, R, C::GR, WIDE_LEAD, false>(Q, s0, lane, acc, ctr);
                    if (lane_ok) {
                        float* o = p.tpi + (size_t)(oy - p.out_row0) * p.nx + ocol;
                        float out_t[NCW];
#pragma unroll
                        for (int t = 0; t < NCW; ++t) {
                            const int xi = (int)ctr[t];  // integers: see tpi_march_kernel
                            out_t[t] = (float)((double)xi - (double)((int)acc[t] - xi) * inv_nm1);
                        }
#pragma unroll
                        for (int P = 0; P < NCW / 2; ++P)  // (nx % 4 == 0, ocol even: a pair is inside or outside)
                            if (ocol + 2 * P < p.nx) *reinterpret_cast<float2*>(o + 2 * P) = make_float2(out_t[2 * P], out_t[2 * P + 1]);
                    }
                }
            }
            advance_wslot();
            __syncthreads();
            fold((ph + 1) & 1);
        }
        pos += run_tiles;
    }
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
    WaveArgs a{b.in, tpi_out, nullptr, b.in_rows, b.in_row0, b.gny, b.nx, b.out_row0, b.out_rows,
               nullptr, nullptr, nullptr, 0, 0, 0};
    static int blocks_per_cu = 0;
    if (blocks_per_cu == 0) {
        TOPO_HIP(hipFuncSetAttribute((const void*)tpi_ring_wide_kernel<SIZE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS));
        int nblk = 0;
        TOPO_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, (const void*)tpi_ring_wide_kernel<SIZE>, C::NW * 64, C::LDS));
        blocks_per_cu = nblk < 1 ? 1 : nblk;
    }
    a.report = dem_memo_report(b);
    WaveParts ps;
    int tiles_x = 0;
    long ntiles = 0;
    TOPO_TRY(make_parts(b, a, C::TH, G::TILE_W, true, false, &ps, &tiles_x, &ntiles, map_th, map_tw));
    TOPO_REQUIRE(ps.n == 1 && ps.a[0].map_th == map_th && ps.a[0].map_tw == map_tw, "wide ring: tile map of another geometry");
    const size_t map_bytes = (size_t)((b.nx + map_tw - 1) / map_tw) * ps.a[0].map_tiles_y;
    TOPO_HIP(hipMemsetAsync(ps.a[0].defer, kTileDone, map_bytes, c.compute));
    const long grid = march_grid(c, blocks_per_cu, ntiles);
    deal_parts(&ps, tiles_x, grid, blocks_per_cu);
    hipLaunchKernelGGL(tpi_ring_wide_kernel<SIZE>, dim3((unsigned)grid), dim3(C::NW * 64), C::LDS, c.compute, ps.a[0], tiles_x, ps.tiles_y[0], ps.run[0]);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}

}  // namespace

}  // namespace topo
