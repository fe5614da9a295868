// C ABI of libtopo_amd.so (declared in include/topo_amd.h), row shards: the RCCL communicator, the ghost-row exchange and
// its gate, and the topo_amd_shard_* entry points.
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi.hpp"

namespace topo {

// ---- RCCL state -----------------------------------------------------------------------------
namespace {
struct Comm {
    ncclComm_t comm = nullptr;
    int rank = 0, size = 1;
    bool halo_pending = false;
} g_comm;
// declared ghost depth of the shard buffers (topo_amd_shard_layout): per calling thread, so that two threads (or an
// application and a ShardedDEM inside it) that drive shards with different buffer layouts do not see each other's
// shards.  A thread that has never declared a layout sees the process-wide one - the last one any thread declared (an
// application that declares it once at set-up and drives the shards from worker threads: ADVICE r03).
thread_local int t_layout_above = -1, t_layout_below = -1;
thread_local bool t_layout_set = false;
std::atomic<int> g_layout_above{-1}, g_layout_below{-1};
int layout_above() { return t_layout_set ? t_layout_above : g_layout_above.load(); }
int layout_below() { return t_layout_set ? t_layout_below : g_layout_below.load(); }

// TOPO_AMD_HALO_LOOPBACK=1 with a communicator of one rank: the exchange talks to itself
bool halo_loopback() {
    const char* e = std::getenv("TOPO_AMD_HALO_LOOPBACK");
    return e && e[0] == '1' && g_comm.size == 1 && g_comm.comm != nullptr;
}

#define TOPO_NCCL(call)                                                                    \
    do {                                                                                   \
        ncclResult_t r_ = (call);                                                          \
        if (r_ != ncclSuccess) {                                                           \
            ::topo::set_error("%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_),      \
                              __FILE__, __LINE__);                                         \
            return TOPO_AMD_ERCCL;                                                         \
        }                                                                                  \
    } while (0)

uint32_t g_giveups_reported = 0;  // value of the give-up counter at the last topo_amd_gate_giveups
uint32_t g_giveups_probed = 0;    //                              ... at the last look of the mode logic
int g_probe_calls = 0;            // careful calls whose completion nobody has looked at yet (the probe event stands behind the last of them)
void gate_probe_poll();
}  // namespace

// lean mode: a block's wait at the gate ran out (gate.hpp) - the seam rows of that call were computed from ghost rows
// that had not arrived.  Reported once, by the next call that synchronises; the library is careful from then on.
int check_gate_errors() {
    Context& c = ctx();
    gate_probe_poll();  // (a synchronising call: whatever careful calls were in flight are over)
    volatile uint32_t* err = c.gate_timeouts ? c.gate_timeouts + 4 : nullptr;
    if (err && *err != 0) {
        const unsigned n = *err;
        *err = 0;
        c.gate_mode = 2;
        set_error("ghost-row gate: %u blocks waited longer than TOPO_AMD_GATE_TIMEOUT_MS for the halo exchange; the seam "
                  "rows of the sharded calls since the last synchronisation are invalid (is a neighbour rank missing?).  "
                  "Later calls run with the clean-up launch again", n);
        return TOPO_AMD_ERCCL;
    }
    return TOPO_AMD_OK;
}

void reset_shard() {
    g_giveups_reported = g_giveups_probed = 0;
    g_probe_calls = 0;
}

void release_shard() {
    if (g_comm.comm) {
        (void)ncclCommDestroy(g_comm.comm);
        g_comm = Comm();
    }
}

}  // namespace topo

using namespace topo;

extern "C" {

// Blocks of sharded launches that gave up waiting at the ghost-row gate since the last call (gate.hpp): their seam
// tiles were done by the clean-up launch behind the exchange, i.e. the exchange was NOT hidden behind the interior
// rows for them.  0 in a healthy run (after the first calls, in which RCCL sets its connections up); a statistic
// for bench.py and the tests, never an error.
int topo_amd_gate_giveups(unsigned* count) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(count != nullptr, "gate_giveups: NULL output");
    const uint32_t now = *(volatile uint32_t*)ctx().gate_timeouts;
    *count = now - g_giveups_reported;  // (both reset by topo_amd_init)
    g_giveups_reported = now;
    return TOPO_AMD_OK;
}

// ---- RCCL row sharding ------------------------------------------------------------------------
namespace {
// CUs the persistent kernels of a sharded call leave to RCCL's send / receive kernel (TOPO_AMD_RESERVE_CUS, 0 ... 64;
// effective in steps of 8: one CU on every XCD, see march_grid)
int reserve_cus_setting() {
    static const int v = [] {
        const char* e = std::getenv("TOPO_AMD_RESERVE_CUS");
        return e && *e ? std::max(0, std::min(64, std::atoi(e))) : 8;
    }();
    return v;
}
// The ghost-row exchange is two point-to-point messages of a few MB over one xGMI link each (50 GB/s): it needs a
// few channels, not the 64 workgroups RCCL launches by default - which do not fit next to a persistent kernel
// that fills the chip, so that the "overlapped" exchange of rounds 1-3 really ran when the interior launch ended
// (kernel trace: profiles/r04_shard_fused.txt).  8 channels = 8 workgroups (256 threads, 37 KB of LDS, 124 VGPRs),
// one per XCD, each on the CU the shorter grid leaves free there; in loop-back they move the 2 x 4.3 MB of the TPI
// halo in 46 us (4 channels: 79 us, 2: 163 us).  Whatever the user has set stays.
void cap_rccl_channels() {
    setenv("NCCL_MAX_NCHANNELS", "8", 0);
    setenv("NCCL_MAX_P2P_NCHANNELS", "8", 0);
    setenv("NCCL_MIN_P2P_NCHANNELS", "1", 0);
}
}  // namespace

int topo_amd_comm_unique_id(char id[TOPO_AMD_UNIQUE_ID_BYTES]) {
    TOPO_ENTER();
    static_assert(sizeof(ncclUniqueId) <= TOPO_AMD_UNIQUE_ID_BYTES, "unique id size");
    cap_rccl_channels();
    ncclUniqueId uid;
    TOPO_NCCL(ncclGetUniqueId(&uid));
    std::memset(id, 0, TOPO_AMD_UNIQUE_ID_BYTES);
    std::memcpy(id, &uid, sizeof(uid));
    return TOPO_AMD_OK;
}

int topo_amd_comm_init(int rank, int nranks, const char id[TOPO_AMD_UNIQUE_ID_BYTES]) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "comm_init: rank %d of %d", rank, nranks);
    TOPO_REQUIRE(g_comm.comm == nullptr, "comm_init: communicator already exists");
    cap_rccl_channels();
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    TOPO_NCCL(ncclCommInitRank(&g_comm.comm, nranks, uid, rank));
    g_comm.rank = rank;
    g_comm.size = nranks;
    return TOPO_AMD_OK;
}

int topo_amd_comm_rank(void) { return g_comm.rank; }
int topo_amd_comm_size(void) { return g_comm.size; }

int topo_amd_comm_destroy(void) {
    TOPO_ENTER();
    if (g_comm.comm) {
        (void)hipDeviceSynchronize();
        TOPO_NCCL(ncclCommDestroy(g_comm.comm));
    }
    g_comm = Comm();
    return TOPO_AMD_OK;
}

namespace {
__global__ void stamp_kernel(uint32_t* word, uint32_t value) {
    __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// writes the current epoch into the gate word, in stream order on the communication stream: a stream memory
// operation where the runtime has one (no kernel, no CU), a one-thread kernel otherwise
int stamp_gate(Context& c) {
    static int mode = 0;
    if (mode == 0) {
        if (hipStreamWriteValue32(c.comm, c.gate_word, c.gate_epoch, 0) == hipSuccess) return TOPO_AMD_OK;
        (void)hipGetLastError();
        mode = 1;
    }
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, c.comm, c.gate_word, c.gate_epoch);
    TOPO_HIP(hipGetLastError());
    return TOPO_AMD_OK;
}
}  // namespace

int topo_amd_halo_exchange_start(float* block, int rows_local, int nx, int halo_above,
                                 int halo_below) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Context& c = ctx();
    TOPO_REQUIRE(block && rows_local >= 1 && nx >= 1 && halo_above >= 0 && halo_below >= 0,
                 "halo_exchange: bad arguments");
    TOPO_REQUIRE(rows_local >= halo_above && rows_local >= halo_below,
                 "halo_exchange: %d local rows cannot feed ghost depths %d/%d (shard too thin)",
                 rows_local, halo_above, halo_below);
    // the local rows must be final before neighbours read them
    TOPO_HIP(hipEventRecord(c.input_ready, c.compute));
    TOPO_HIP(hipStreamWaitEvent(c.comm, c.input_ready, 0));
    float* ghost_top = block;
    float* local = block + (size_t)halo_above * nx;
    float* ghost_bot = local + (size_t)rows_local * nx;
    if (halo_loopback()) {
        // the rank is its own upper and lower neighbour: same calls, same counts, periodic wrap.  Sends and
        // receives to one peer inside a group match in order.
        TOPO_NCCL(ncclGroupStart());
        if (halo_above > 0) {
            TOPO_NCCL(ncclSend(local + (size_t)(rows_local - halo_above) * nx, (size_t)halo_above * nx, ncclFloat, 0,
                               g_comm.comm, c.comm));
            TOPO_NCCL(ncclRecv(ghost_top, (size_t)halo_above * nx, ncclFloat, 0, g_comm.comm, c.comm));
        }
        if (halo_below > 0) {
            TOPO_NCCL(ncclSend(local, (size_t)halo_below * nx, ncclFloat, 0, g_comm.comm, c.comm));
            TOPO_NCCL(ncclRecv(ghost_bot, (size_t)halo_below * nx, ncclFloat, 0, g_comm.comm, c.comm));
        }
        TOPO_NCCL(ncclGroupEnd());
    } else if (g_comm.size > 1) {
        TOPO_REQUIRE(g_comm.comm != nullptr, "halo_exchange: call topo_amd_comm_init first");
        const int up = g_comm.rank - 1, down = g_comm.rank + 1;
        TOPO_NCCL(ncclGroupStart());
        if (up >= 0) {
            // my first halo_below rows become the upper neighbour's bottom ghost rows
            if (halo_below > 0)
                TOPO_NCCL(ncclSend(local, (size_t)halo_below * nx, ncclFloat, up, g_comm.comm, c.comm));
            if (halo_above > 0)
                TOPO_NCCL(ncclRecv(ghost_top, (size_t)halo_above * nx, ncclFloat, up, g_comm.comm, c.comm));
        }
        if (down < g_comm.size) {
            if (halo_above > 0)
                TOPO_NCCL(ncclSend(local + (size_t)(rows_local - halo_above) * nx,
                                   (size_t)halo_above * nx, ncclFloat, down, g_comm.comm, c.comm));
            if (halo_below > 0)
                TOPO_NCCL(ncclRecv(ghost_bot, (size_t)halo_below * nx, ncclFloat, down, g_comm.comm, c.comm));
        }
        TOPO_NCCL(ncclGroupEnd());
    }
    // the gate of the fused seam parts: the epoch of this exchange, written behind the receives
    ++c.gate_epoch;
    TOPO_TRY(stamp_gate(c));
    TOPO_HIP(hipEventRecord(c.halo_done, c.comm));
    g_comm.halo_pending = true;
    return TOPO_AMD_OK;
}

int topo_amd_shard_layout(int halo_above, int halo_below) {
    TOPO_REQUIRE((halo_above >= 0 && halo_below >= 0) || (halo_above == -1 && halo_below == -1),
                 "shard_layout: ghost depths %d / %d (both >= 0, or -1 / -1 for 'as the descriptor needs')", halo_above,
                 halo_below);
    t_layout_above = halo_above;
    t_layout_below = halo_below;
    t_layout_set = true;
    g_layout_above.store(halo_above);
    g_layout_below.store(halo_below);
    return TOPO_AMD_OK;
}

int topo_amd_shard_layout_get(int* halo_above, int* halo_below) {
    TOPO_REQUIRE(halo_above && halo_below, "shard_layout_get: NULL output");
    *halo_above = layout_above();
    *halo_below = layout_below();
    return TOPO_AMD_OK;
}

// Collective: every rank scans the lattice points of the rows it owns, the scans are added up (three all-reduces of a few
// bytes, once per DEM), and the class of the WHOLE raster is declared for the calling thread's later topo_amd_shard_* calls -
// so every shard takes the kernels the single-GPU run of the raster takes.  `owned`: the first row the rank owns.
int topo_amd_shard_classify(const float* owned, int rows_local, int row0, int gny, int nx) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(owned && rows_local >= 1 && row0 >= 0 && row0 + rows_local <= gny && nx >= 1, "shard_classify: bad arguments");
    // (a shard that is not the whole raster needs its neighbours' samples: without a communicator - a ShardedDEM built
    // before topo_amd_comm_init - the class of the rows at hand would pass for the raster's.  Loop-back: the rank is its
    // own neighbour, its rows are all there is.)
    TOPO_REQUIRE(rows_local == gny || g_comm.size > 1 || halo_loopback(),
                 "shard_classify: rows [%d, %d) of a raster of %d rows, but no communicator exists (topo_amd_comm_init) - the other "
                 "shards' samples cannot be added", row0, row0 + rows_local, gny);
    Scan s;
    if (halo_loopback() && rows_local < gny) {
        // the rank is every rank: the raster is its rows stacked periodically, so they are scanned at every placement
        for (long place = (long)row0 - ((long)row0 + rows_local - 1) / rows_local * rows_local; place < gny; place += rows_local) {
            const int o0 = (int)std::max(0L, place), o1 = (int)std::min((long)gny, place + rows_local);
            if (o1 <= o0) continue;
            Block b{owned, rows_local, (int)place, gny, nx, o0, o1 - o0};
            TOPO_TRY(scan_block(b, o0, o1 - o0, &s));
        }
    } else {
        Block b{owned, rows_local, row0, gny, nx, row0, rows_local};
        TOPO_TRY(scan_block(b, row0, rows_local, &s));
    }
    if (g_comm.size > 1) {
        TOPO_REQUIRE(g_comm.comm != nullptr, "shard_classify: call topo_amd_comm_init first");
        Context& c = ctx();
        void* d = nullptr;
        TOPO_TRY(workspace(0, 64, &d));
        struct Wire {
            unsigned long long counts[3];
            float lo, hi;
        } w{{s.taken, s.large, s.frac}, s.lo, s.hi};
        TOPO_HIP(hipMemcpyAsync(d, &w, sizeof(w), hipMemcpyHostToDevice, c.compute));
        char* base = (char*)d;
        TOPO_NCCL(ncclAllReduce(base, base, 3, ncclUint64, ncclSum, g_comm.comm, c.compute));
        TOPO_NCCL(ncclAllReduce(base + 24, base + 24, 1, ncclFloat, ncclMin, g_comm.comm, c.compute));
        TOPO_NCCL(ncclAllReduce(base + 28, base + 28, 1, ncclFloat, ncclMax, g_comm.comm, c.compute));
        TOPO_HIP(hipMemcpyAsync(&w, d, sizeof(w), hipMemcpyDeviceToHost, c.compute));
        TOPO_HIP(hipStreamSynchronize(c.compute));
        s.taken = w.counts[0];
        s.large = w.counts[1];
        s.frac = w.counts[2];
        s.lo = w.lo;
        s.hi = w.hi;
    }
    declare_class(owned, rows_local, gny, nx, class_of(s));
    return TOPO_AMD_OK;
}

int topo_amd_halo_wait(void) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    if (g_comm.halo_pending) {
        TOPO_HIP(hipStreamWaitEvent(ctx().compute, ctx().halo_done, 0));
        g_comm.halo_pending = false;
    }
    return TOPO_AMD_OK;
}

}  // extern "C"

namespace topo {
namespace {

// Geometry of one rank's haloed block inside the global DEM.
struct Shard {
    Block whole;           // block including the ghost rows that exist
    Block owned;           // the owned rows alone: what a launch may read while the exchange is in flight
    int row0, rows_local;  // owned rows
    int interior0, interior1;  // owned rows whose stencil stays inside the owned rows
};

// The buffer is laid out with the declared ghost depth (topo_amd_shard_layout); a descriptor that needs
// `above` rows uses the last `above` of the declared ones.  Moves *block to where its [above | local | below] view
// starts and fills the shard of that view.
int open_shard(float** block_io, int rows_local, int row0, int gny, int nx, int above, int below, const char* who, Shard* out) {
    TOPO_REQUIRE(*block_io != nullptr, "%s: NULL block", who);
    if (layout_above() >= 0) {
        TOPO_REQUIRE(above <= layout_above() && below <= layout_below(),
                     "%s needs %d / %d ghost rows but the shard buffers were declared with %d / %d (topo_amd_shard_layout)",
                     who, above, below, layout_above(), layout_below());
        *block_io += (size_t)(layout_above() - above) * nx;
    }
    float* block = *block_io;
    Shard& s = *out;
    const bool has_up = row0 > 0, has_down = row0 + rows_local < gny;
    // the buffer always reserves `above` ghost rows on top; at the global edge they are unused
    s.whole.in = block + (size_t)(has_up ? 0 : above) * nx;
    s.whole.in_row0 = has_up ? row0 - above : row0;
    s.whole.in_rows = rows_local + (has_up ? above : 0) + (has_down ? below : 0);
    s.whole.gny = gny;
    s.whole.nx = nx;
    s.owned = s.whole;
    s.owned.in = block + (size_t)above * nx;
    s.owned.in_row0 = row0;
    s.owned.in_rows = rows_local;
    s.row0 = row0;
    s.rows_local = rows_local;
    s.interior0 = has_up ? std::min(row0 + above, row0 + rows_local) : row0;
    s.interior1 = has_down ? std::max(row0 + rows_local - below, s.interior0) : row0 + rows_local;
    return TOPO_AMD_OK;
}

// output rows [o0, o0 + on) of a view a run form hands out: the launcher's block, checked for its ghost rows
int out_block(const Block& view, int o0, int on, int above, int below, const char* who, Block* b) {
    *b = view;
    b->out_row0 = o0;
    b->out_rows = on;
    return check_block(*b, above, below, who);
}

// The three-launch route of rounds 1-3: runs `fn(block, out_row0, out_rows)` for the interior rows first, then, behind the
// exchange's event (the ghost rows have landed), for the two seam strips: the exchange overlaps the interior compute.  The
// interior launch gets the OWNED rows as its block: the ghost rows are being written by the exchange meanwhile, and a
// tile-based kernel stages (and classifies) every row of its block that a tile touches, not only the rows its outputs
// need.  `started`: the exchange is already in flight.
template <class Fn>
int run_three(float* block, const Shard& s, int above, int below, Fn fn, bool started) {
    if (!started) TOPO_TRY(topo_amd_halo_exchange_start(block, s.rows_local, s.whole.nx, above, below));
    // persistent launches leave a round of CUs to RCCL's kernel (march_grid)
    ctx().reserve_cus = (g_comm.size > 1 || halo_loopback()) ? reserve_cus_setting() : 0;
    int rc = TOPO_AMD_OK;
    if (s.interior1 > s.interior0) rc = fn(s.owned, s.interior0, s.interior1 - s.interior0);
    ctx().reserve_cus = 0;
    if (rc != TOPO_AMD_OK) return rc;
    TOPO_TRY(topo_amd_halo_wait());
    if (s.interior0 > s.row0) TOPO_TRY(fn(s.whole, s.row0, s.interior0 - s.row0));
    const int end = s.row0 + s.rows_local;
    if (end > s.interior1) TOPO_TRY(fn(s.whole, s.interior1, end - s.interior1));
    return TOPO_AMD_OK;
}

// ---- round 4: ONE launch per kernel of the descriptor for the whole shard -------------------------------------------
// Two forms, both behind the ghost-row gate (gate.hpp) that the communication stream opens when the ghost rows have
// landed, both with the block views, output rows and kernels of run_three, hence its bits:
//  * run_fused (marching kernels: TPI / STD): the seam strips travel with the interior launch as "parts"
//    (Context::seams; disc_wave_impl.hpp, make_parts): every persistent block does its share of the interior, finds the
//    gate open - the exchange ran next to the interior - and does its share of the seams;
//  * run_gated (kernels of independent tiles: Sx): one launch over all owned rows on the block with its ghost rows; the
//    tile rows that read ghost rows are dispatched last and wait at the gate (Context::ghost).
// No relaunch tail, no under-filled seam launches, a third of the launches.  A launcher that cannot do it says so
// (leaves the gate armed / answers TOPO_AMD_EUNSUP before launching) and the call takes run_three.
// TOPO_AMD_SHARD_FUSED=0: always run_three (A/B).
bool shard_fused_on() {
    static const bool on = [] {
        const char* e = std::getenv("TOPO_AMD_SHARD_FUSED");
        return !(e && *e == '0');
    }();
    return on;
}
// how long a block waits at a closed gate before it leaves its seam tiles to the clean-up launch (TOPO_AMD_GATE_WAIT_US)
uint32_t gate_limit_ticks() {
    static const uint32_t v = [] {
        const char* e = std::getenv("TOPO_AMD_GATE_WAIT_US");
        const double us = e && *e ? std::atof(e) : 100.0;
        return (uint32_t)std::min(4.0e9, std::max(0.0, us) * 100.0);  // s_memtime: 100 MHz
    }();
    return v;
}
// lean mode: how long a block waits before it reports an error (TOPO_AMD_GATE_TIMEOUT_MS)
uint32_t gate_timeout_ticks() {
    static const uint32_t v = [] {
        const char* e = std::getenv("TOPO_AMD_GATE_TIMEOUT_MS");
        const double ms = e && *e ? std::atof(e) : 5000.0;  // (ranks drift apart by milliseconds, a first allocation by tens)
        return (uint32_t)std::min(4.0e9, std::max(1.0, ms) * 1.0e5);
    }();
    return v;
}
void gate_probe_poll() {
    Context& c = ctx();
    if (c.gate_mode != 0 || !c.gate_probe_pending || hipEventQuery(c.gate_probe) != hipSuccess) return;
    // every careful call up to the probe is over: did all of their blocks find the gate open?
    c.gate_probe_pending = false;
    const uint32_t now = *(volatile uint32_t*)c.gate_timeouts;
    c.gate_clean_calls = now == g_giveups_probed ? c.gate_clean_calls + g_probe_calls : 0;
    g_giveups_probed = now;
    g_probe_calls = 0;
    if (c.gate_clean_calls >= 3) c.gate_mode = 1;
}
// The gate of the exchange just started, careful or lean (Context::gate_mode; TOPO_AMD_GATE_MODE=careful / lean pins it).
Gate make_gate(bool* lean) {
    Context& c = ctx();
    // TOPO_AMD_GATE_MODE: careful (the default: a block that finds the gate closed for long leaves its seam tiles to the
    // clean-up launch behind the exchange's event - right whatever the neighbour ranks do, whoever reads the outputs),
    // lean (no clean-up launch, no event wait: a neighbour later than TOPO_AMD_GATE_TIMEOUT_MS is an ERROR that only
    // the next synchronising library call reports - for applications that do call one), auto (careful until a
    // few calls found the gate open, then lean).
    static const int pinned = [] {
        const char* e = std::getenv("TOPO_AMD_GATE_MODE");
        return e && e[0] == 'l' ? 1 : e && e[0] == 'a' ? 0 : 2;
    }();
    if (pinned) c.gate_mode = c.gate_mode == 2 ? 2 : pinned;  // (an error always ends lean mode)
    gate_probe_poll();
    *lean = c.gate_mode == 1;
    return Gate{c.gate_word, c.gate_epoch, c.gate_timeouts, *lean ? gate_timeout_ticks() : gate_limit_ticks(),
                (uint8_t*)c.gate_word + 256, *lean ? c.gate_timeouts + 4 : nullptr};
}
// behind a call whose launcher took the gate
int finish_gated(bool lean, bool probe) {
    Context& c = ctx();
    // every later launch on the compute stream is ordered behind a kernel all of whose blocks passed the gate
    if (lean) {
        g_comm.halo_pending = false;  // (no event wait on the compute stream: nothing is left to wait for)
        return TOPO_AMD_OK;
    }
    if (c.gate_mode == 0 && probe) {
        TOPO_HIP(hipEventRecord(c.gate_probe, c.compute));
        c.gate_probe_pending = true;
        ++g_probe_calls;
    }
    return topo_amd_halo_wait();  // (the clean-up launch waited already: keeps topo_amd_halo_wait's contract)
}

// tile_rows: the tile height of the descriptor's first kernel (a hint, 0 = unknown).  The kernels' tile rows sit on global
// multiples of it, so an interior that starts or ends inside a tile makes that tile be staged twice - once by the
// interior part for its lower rows, once by the seam part for its upper ones: the interior is shrunk to whole tiles and
// the two edge tiles belong to the seam parts entirely (any interior inside [interior0, interior1) is valid: the seam
// parts see the ghost rows).  68 + 2 tile slots per strip become 66 + 2 at 67 px on a 4096-row shard.
template <class Fn>
int run_fused(float* block, const Shard& s0, int above, int below, int tile_rows, Fn fn) {
    Shard s = s0;
    const int end = s.row0 + s.rows_local;
    if (tile_rows > 0) {
        const int a = s.interior0 > s.row0 ? (s.interior0 + tile_rows - 1) / tile_rows * tile_rows : s.interior0;
        const int b = end > s.interior1 ? s.interior1 / tile_rows * tile_rows : s.interior1;
        if (b > a) {
            s.interior0 = a;
            s.interior1 = b;
        }
    }
    const bool top = s.interior0 > s.row0, bottom = end > s.interior1;
    if (!shard_fused_on() || s.interior1 <= s.interior0 || (!top && !bottom)) return run_three(block, s0, above, below, fn, false);
    Context& c = ctx();
    TOPO_TRY(topo_amd_halo_exchange_start(block, s.rows_local, s.whole.nx, above, below));
    const bool live = g_comm.size > 1 || halo_loopback();
    c.reserve_cus = live ? reserve_cus_setting() : 0;
    c.seams = Seams();
    auto add = [&](int r0, int rows) {
        Block b = s.whole;
        b.out_row0 = r0;
        b.out_rows = rows;
        c.seams.b[c.seams.n++] = b;
    };
    if (top) add(s.row0, s.interior0 - s.row0);
    if (bottom) add(s.interior1, end - s.interior1);
    bool lean = false;
    c.seams.gate = make_gate(&lean);
    c.seams.gate_armed = true;
    const int rc = fn(s.owned, s.interior0, s.interior1 - s.interior0);
    const bool taken = !c.seams.gate_armed;
    c.seams = Seams();
    c.reserve_cus = 0;
    if (rc != TOPO_AMD_OK) return rc;
    if (taken) return finish_gated(lean, true);
    TOPO_TRY(topo_amd_halo_wait());
    if (top) TOPO_TRY(fn(s.whole, s.row0, s.interior0 - s.row0));
    if (bottom) TOPO_TRY(fn(s.whole, s.interior1, end - s.interior1));
    return TOPO_AMD_OK;
}

// device_gate: the launcher's kernel waits at the gate itself (Sx) - in lean mode only: a grid kernel keeps every CU
// slot filled with its own pending workgroups, so RCCL's kernel gets to run when the grid drains, i.e. when the
// blocks of the ghost tile rows are already waiting; with the careful mode's short wait they would all give up.
// Otherwise (gradient) the launcher orders its row chunks around the exchange's event and needs no mode.
template <class Fn>
int run_gated(float* block, const Shard& s, int above, int below, bool device_gate, Fn fn) {
    const int end = s.row0 + s.rows_local;
    const bool top = s.interior0 > s.row0, bottom = end > s.interior1;
    if (!shard_fused_on() || (!top && !bottom)) return run_three(block, s, above, below, fn, false);
    Context& c = ctx();
    bool lean = false;
    const Gate gate = make_gate(&lean);  // (the epoch is patched in below, once the exchange has its number)
    if (device_gate && !lean) return run_three(block, s, above, below, fn, false);
    TOPO_TRY(topo_amd_halo_exchange_start(block, s.rows_local, s.whole.nx, above, below));
    c.ghost = GhostGate();
    c.ghost.gate = gate;
    c.ghost.gate.epoch = c.gate_epoch;
    c.ghost.ghost_lo = s.whole.in_row0 < s.row0 ? s.row0 : -(1 << 30);  // rows above the owned ones that exist: ghost rows
    c.ghost.ghost_hi = s.whole.in_row0 + s.whole.in_rows > end ? end : (1 << 30);
    c.ghost.slots = kGateSlots;
    c.ghost.armed = true;
    const int rc = fn(s.whole, s.row0, s.rows_local);
    const bool taken = !c.ghost.armed;
    c.ghost = GhostGate();
    if (taken) return rc == TOPO_AMD_OK ? finish_gated(lean && device_gate, false) : rc;
    if (rc != TOPO_AMD_EUNSUP) return rc;  // (an error before anything was launched)
    return run_three(block, s, above, below, fn, true);
}

// The class of the raster a shard belongs to, before the first launcher asks: a shard that is the whole raster is scanned
// like any whole block; a partial one uses what was declared for its owned rows, and declares it itself - collectively,
// every rank being in the same call on a buffer nobody has declared anything for since it was last written - when
// nothing was (a C caller that never heard of topo_amd_shard_classify gets the single GPU's bits too).
int ensure_shard_class(const Shard& s) {
    if (s.rows_local == s.owned.gny || declared_class(s.owned, nullptr)) return TOPO_AMD_OK;
    return topo_amd_shard_classify(s.owned.in, s.rows_local, s.row0, s.owned.gny, s.owned.nx);
}

// The mean and standard deviation of the WHOLE DEM (topo.py:427) from the rows this rank owns: float64 moments about 0,
// then the one all-reduce of the path.  On a DEM of whole metres the three numbers are exact integers (< 2^53), so every
// sharding gets the same mean and std.
int shard_moments(const float* owned, int rows_local, int nx, double* mean, double* stdev, double* moments_out) {
    double mom[3] = {(double)rows_local * (double)nx, 0.0, 0.0};
    TOPO_TRY(launch_moments(owned, (size_t)rows_local * nx, 0.0, false, &mom[1], &mom[2]));
    if (g_comm.size > 1) {
        void* d_mom = nullptr;
        TOPO_TRY(workspace(0, 3 * sizeof(double), &d_mom));
        TOPO_HIP(hipMemcpyAsync(d_mom, mom, sizeof(mom), hipMemcpyHostToDevice, ctx().compute));
        TOPO_NCCL(ncclAllReduce(d_mom, d_mom, 3, ncclDouble, ncclSum, g_comm.comm, ctx().compute));
        TOPO_HIP(hipMemcpyAsync(mom, d_mom, sizeof(mom), hipMemcpyDeviceToHost, ctx().compute));
        TOPO_HIP(hipStreamSynchronize(ctx().compute));
    }
    *mean = mom[1] / mom[0];
    double var = mom[2] / mom[0] - *mean * *mean;
    if (var < 0.0) var = 0.0;
    *stdev = std::sqrt(var);
    if (moments_out) {
        moments_out[0] = *mean;
        moments_out[1] = *stdev;
    }
    return TOPO_AMD_OK;
}

// One pass of the numpy-order moments across the shards (moments_np.hip): the array of `words` the ranks' parts were queued
// into on the compute stream is sum-reduced as unsigned integers on the communication stream - every word is one rank's, zero
// on the others, so every rank receives every word bit for bit - and downloaded behind it.  A communicator of one rank (loop-
// back: the rank filled every slot itself) has nothing to reduce.
int np_exchange(uint32_t* d_words, size_t words, std::vector<uint32_t>* host) {
    Context& c = ctx();
    host->resize(words);
    hipStream_t from = c.compute;
    if (g_comm.size > 1) {
        TOPO_REQUIRE(g_comm.comm != nullptr, "shard_mean_std_f32: call topo_amd_comm_init first");
        TOPO_HIP(hipEventRecord(c.input_ready, c.compute));
        TOPO_HIP(hipStreamWaitEvent(c.comm, c.input_ready, 0));
        TOPO_NCCL(ncclAllReduce(d_words, d_words, words, ncclUint32, ncclSum, g_comm.comm, c.comm));
        from = c.comm;
    }
    TOPO_HIP(hipMemcpyAsync(host->data(), d_words, words * sizeof(uint32_t), hipMemcpyDeviceToHost, from));
    TOPO_HIP(hipStreamSynchronize(from));
    return TOPO_AMD_OK;
}

// numpy's own float32 mean() / std() of the WHOLE raster from the rows this rank owns (route 3): per pass the rank's part of
// numpy's summation tree on its GPU, one collective, one download, and the same host chain over the same floats on every
// rank - the bits topo_amd_mean_std_f32_dev gives on the whole raster, however the rows are cut.  Loop-back: the rank stands
// for every placement of the periodic stack of its rows and fills every placement's slot.
int shard_mean_std_np(const float* owned, int rows_local, int row0, int gny, int nx, size_t chunk, float* mean, float* stdev) {
    TOPO_REQUIRE(owned && rows_local >= 1 && row0 >= 0 && row0 + rows_local <= gny && nx >= 1, "shard_mean_std_f32: bad arguments");
    TOPO_REQUIRE(np_chunk_ok(chunk), "shard_mean_std_f32: chunk %zu (a power of two, 128 at least)", chunk);
    TOPO_REQUIRE(rows_local == gny || g_comm.size > 1 || halo_loopback(),
                 "shard_mean_std_f32: rows [%d, %d) of a raster of %d rows, but no communicator exists (topo_amd_comm_init) - the other "
                 "shards' samples cannot be added", row0, row0 + rows_local, gny);
    const bool stacked = halo_loopback() && rows_local < gny;
    TOPO_REQUIRE(!stacked || (gny % rows_local == 0 && row0 % rows_local == 0),
                 "shard_mean_std_f32: loop-back stacks whole copies of the rank's rows, %d rows at row %d do not tile %d", rows_local, row0, gny);
    const int slots = stacked ? gny / rows_local : g_comm.size;
    const size_t count = (size_t)gny * nx, n = (size_t)rows_local * nx;
    const size_t words1 = np_shard_words(count, chunk, slots, true), words2 = np_shard_words(count, chunk, slots, false);
    void* d = nullptr;
    TOPO_TRY(workspace(0, words1 * sizeof(uint32_t), &d));
    uint32_t* d_words = (uint32_t*)d;
    Context& c = ctx();
    std::vector<uint32_t> first_pass, second_pass;
    auto pass = [&](bool sq, float m, size_t words, std::vector<uint32_t>* host) {
        TOPO_HIP(hipMemsetAsync(d_words, 0, words * sizeof(uint32_t), c.compute));
        for (int k = 0; k < (stacked ? slots : 1); ++k) {
            const int slot = stacked ? k : g_comm.rank;
            const size_t first = (size_t)(stacked ? k * rows_local : row0) * nx;
            TOPO_TRY(launch_np_shard_parts(owned, first, n, count, chunk, slot, sq, m, d_words));
        }
        return np_exchange(d_words, words, host);
    };
    float sum = 0.0f, sum2 = 0.0f;
    TOPO_TRY(pass(false, 0.0f, words1, &first_pass));
    TOPO_TRY(np_shard_sum(first_pass.data(), first_pass.data(), count, chunk, slots, false, 0.0f, &sum));
    const float m = sum / (float)count;
    if (words2) TOPO_TRY(pass(true, m, words2, &second_pass));  // (no whole chunk in the raster: the fragments are all there is)
    TOPO_TRY(np_shard_sum(second_pass.data(), first_pass.data(), count, chunk, slots, true, m, &sum2));
    *mean = m;
    *stdev = std::sqrt(sum2 / (float)count);
    return TOPO_AMD_OK;
}

int shard_valley_ridge(float* block, int rows_local, int row0, int gny, int nx, const float* taps, const int32_t* ksize,
                       const float* angles, int n_angles, int n_planes, float* norm_out, float* dir_out, double* moments_out,
                       size_t np_chunk = 0, float* np_moments_out = nullptr) {
    TOPO_REQUIRE(block && taps && ksize && angles && norm_out && dir_out && n_angles >= 1,
                 "shard_valley_ridge: NULL argument");
    int above = 0, below = 0;
    (void)valley_ridge_reach(ksize, n_angles, &above, &below);
    Shard s;
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, above, below, "shard_valley_ridge", &s));
    double mean = 0.0, stdev = 0.0;
    if (np_chunk) {  // numpy's float32 moments of the whole raster (route 3)
        float m = 0.0f, sd = 0.0f;
        TOPO_TRY(shard_mean_std_np(s.owned.in, rows_local, row0, gny, nx, np_chunk, &m, &sd));
        mean = (double)m, stdev = (double)sd;
        if (np_moments_out) np_moments_out[0] = m, np_moments_out[1] = sd;
        note_valley_moments(3);
    } else {
        note_valley_moments(2);  // (the shards' float64 all-reduce)
        TOPO_TRY(shard_moments(s.owned.in, rows_local, nx, &mean, &stdev, moments_out));
    }
    return run_three(block, s, above, below, [&](const Block& view, int o0, int on) {
        Block b;
        TOPO_TRY(out_block(view, o0, on, above, below, "shard_valley_ridge", &b));
        return launch_valley_ridge(b, taps, ksize, angles, n_angles, n_planes, mean, stdev,
                                   shift(norm_out, o0 - row0, nx), shift(dir_out, o0 - row0, nx));
    }, false);
}

// Gaussian of rows [s0, s1) of a shard into `plane` (row s0 first), around ONE ghost-row exchange of depth above / below
// that this starts: the rows whose filter (g ghost rows: gauss_ghost_rows) stays inside the owned rows first, on the owned
// rows, while the exchange is in flight; then the compute stream waits for the exchange's event and the two seam bands
// follow on the block with its ghost rows.  Row blocks of the Gaussian carrying g ghost rows give the single block's bits.
// The owned-row part keeps kGaussSeamSlack rows more away from the seams: the vector-ALU axis-0 kernel (radii below 4, and
// every radius on a raster of the large-sample class) fetches whole row groups of up to 16 rows with taps in chunks of
// up to 16, so a launch reads up to R + 30 rows beyond its output rows, with zero taps; a non-finite sample there still
// makes the output NaN (0 x NaN).  In the single call those rows are the DEM's; on the owned rows alone they would be
// clamped to the last owned row - another NaN footprint.  The seam bands read them on the block with its ghost rows, as
// any row block with g ghost rows does.
// (This is run_three's order.  run_gated would hand the launcher the whole shard with the gate armed, and only the
// gradient's chunked pipeline knows what to do with that: launch_gaussian has no row chunks of its own to put the seam
// ones last, so it would answer EUNSUP and the call would take run_three anyway.)
int smooth_shard_rows(float* block, const Shard& s, int above, int below, double sigma_y, double sigma_x, int g, int s0,
                      int s1, float* plane) {
    const int nx = s.whole.nx, end = s.row0 + s.rows_local;
    Shard band = s;  // the exchange, the views and the clean-up of run_three, over the rows [s0, s1)
    band.row0 = s0;
    band.rows_local = s1 - s0;
    constexpr int kGaussSeamSlack = 32;
    band.interior0 = std::min(s1, std::max(s0, s.row0 > 0 ? s.row0 + g + kGaussSeamSlack : s.row0));
    band.interior1 = std::max(band.interior0, std::min(s1, end < s.whole.gny ? end - g - kGaussSeamSlack : end));
    TOPO_TRY(topo_amd_halo_exchange_start(block, s.rows_local, nx, above, below));
    return run_three(block, band, above, below, [&](const Block& view, int o0, int on) {
        Block b;
        TOPO_TRY(out_block(view, o0, on, g, g, "shard smoothing", &b));
        return launch_gaussian(b, sigma_y, sigma_x, plane + (size_t)(o0 - s0) * nx);
    }, true);
}

// The class of the smoothed raster for the kernels that run on it (TPI / STD): what the single GPU's Block(smooth) scans
// on the whole smoothed plane.  A shard that is the whole raster is scanned like any whole block (the ClassScope of the
// plane's block does it); a partial one adds up the lattice samples of the OWNED smoothed rows of every rank
// (topo_amd_shard_classify, collective), so that every sharding takes the same kernels.
int smoothed_class(const float* owned_plane, const Shard& s, RasterClass* out, bool* whole) {
    *whole = s.rows_local == s.whole.gny;
    if (*whole) return TOPO_AMD_OK;
    TOPO_TRY(topo_amd_shard_classify(owned_plane, s.rows_local, s.row0, s.whole.gny, s.whole.nx));
    Block b{owned_plane, s.rows_local, s.row0, s.whole.gny, s.whole.nx, s.row0, s.rows_local};
    TOPO_REQUIRE(declared_class(b, out), "shard smoothing: the class of the smoothed rows was not declared");
    return TOPO_AMD_OK;
}

// The smoothed plane of a sharded call: rows [s0, s1) of the shard's smoothed raster, s0 first (workspace 13).  Whatever
// was remembered or declared for that memory is dropped before it is written and after the call (it is scratch).
struct SmoothedPlane {
    float* p = nullptr;
    int s0 = 0, s1 = 0, nx = 0;
    int take(int r0, int r1, int n) {
        s0 = r0;
        s1 = r1;
        nx = n;
        void* w = nullptr;
        TOPO_TRY(workspace(13, (size_t)(s1 - s0) * nx * sizeof(float), &w));
        p = (float*)w;
        forget_plane(p, s1 - s0, nx);
        return TOPO_AMD_OK;
    }
    ~SmoothedPlane() { forget_plane(p, s1 - s0, nx); }
    const float* row(int r) const { return p + (size_t)(r - s0) * nx; }
    Block block(int out_row0, int out_rows, int gny) const { return Block{p, s1 - s0, s0, gny, nx, out_row0, out_rows}; }
};

// The shared start of the *_smoothed calls, for a descriptor that reads up / down rows of the smoothed raster: the view of
// up + g / down + g ghost rows (g: the Gaussian's), its shard, and every row the descriptor reads, smoothed into `sp` around
// ONE exchange - the descriptor's step needs no second one.
int smoothed_shard(float** block, int rows_local, int row0, int gny, int nx, int up, int down, double sigma, const char* who,
                   Shard* s, SmoothedPlane* sp) {
    TOPO_REQUIRE(rows_local >= 1 && row0 >= 0 && row0 + rows_local <= gny && nx >= 1, "%s: rows [%d, %d) of a raster of %d rows", who,
                 row0, row0 + rows_local, gny);
    const int g = gauss_ghost_rows(sigma);
    const int above = up + g, below = down + g;  // == topo_amd_halo_rows(TPI / VALLEY_RIDGE, size / kmax, sigma)
    TOPO_TRY(open_shard(block, rows_local, row0, gny, nx, above, below, who, s));
    TOPO_TRY(sp->take(std::max(0, row0 - up), std::min(gny, row0 + rows_local + down), nx));
    TOPO_TRY(ensure_shard_class(*s));
    ClassScope cls(s->owned);
    return smooth_shard_rows(*block, *s, above, below, sigma, sigma, g, sp->s0, sp->s1, sp->p);
}
}  // namespace
}  // namespace topo

extern "C" {

int topo_amd_shard_tpi_std(float* block, int rows_local, int row0, int gny, int nx, int size,
                           float* tpi_out, float* std_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    DiscRuns disc;
    TOPO_TRY(build_disc(size, &disc));
    const int above = -disc.dj_min, below = disc.dj_max;
    Shard s;
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, above, below, "shard_tpi_std", &s));
    TOPO_TRY(ensure_shard_class(s));
    ClassScope cls(s.owned);  // (the shard is the raster, or what ensure_shard_class found declared for its owned rows)
    forget_plane(tpi_out, rows_local, nx);
    forget_plane(std_out, rows_local, nx);
    // (tile rows of the first kernel: 48 / 60 for the ring kernels of STD, 60 for the marching TPI kernels, 64 for the TPI rings)
    const int tile_rows = std_out ? std_tile_rows(size) : (size <= 17 ? 64 : 60);
    return run_fused(block, s, above, below, tile_rows, [&](const Block& view, int o0, int on) {
        Block b;
        TOPO_TRY(out_block(view, o0, on, above, below, "shard_tpi_std", &b));
        return launch_tpi_std(b, disc, shift(tpi_out, o0 - row0, nx), shift(std_out, o0 - row0, nx));
    });
}

int topo_amd_shard_gradient(float* block, int rows_local, int row0, int gny, int nx, double sigma,
                            double sig_ratio, int res_mode, const void* res_x, const void* res_y,
                            float* dx_out, float* dy_out, float* slope_out, float* aspect_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    const int h = gradient_ghost_rows(sigma, sig_ratio, false);  // == topo_amd_halo_rows(GRADIENT, sigma, sig_ratio)
    Shard s;
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, h, h, "shard_gradient", &s));
    TOPO_TRY(ensure_shard_class(s));
    ClassScope cls(s.owned);
    for (float* o : {dx_out, dy_out, slope_out, aspect_out}) forget_plane(o, rows_local, nx);
    return run_gated(block, s, h, h, false, [&](const Block& view, int o0, int on) {
        Block b;
        TOPO_TRY(out_block(view, o0, on, h, h, "shard_gradient", &b));
        const void *rx = res_x, *ry = res_y;
        if (res_mode == TOPO_AMD_RES_2D) {
            rx = (const float*)res_x + (size_t)(o0 - row0) * nx;
            ry = (const float*)res_y + (size_t)(o0 - row0) * nx;
        }
        return launch_gradient(b, sigma, sig_ratio, res_mode, rx, ry, shift(dx_out, o0 - row0, nx),
                               shift(dy_out, o0 - row0, nx), shift(slope_out, o0 - row0, nx),
                               shift(aspect_out, o0 - row0, nx));
    });
}

int topo_amd_shard_sx(float* block, int rows_local, int row0, int gny, int nx, const int32_t* dj,
                      const int32_t* di, const double* dist, int n_off, int window, double height,
                      float* out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    int up = 0, down = 0;
    sx_reach(dj, dist, 0, n_off, &up, &down);
    Shard s;
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, up, down, "shard_sx", &s));
    return run_gated(block, s, up, down, true, [&](const Block& view, int o0, int on) {
        Block b;
        TOPO_TRY(out_block(view, o0, on, up, down, "shard_sx", &b));
        return launch_sx(b, dj, di, dist, n_off, window, height, shift(out, o0 - row0, nx));
    });
}

int topo_amd_shard_sx_multi(float* block, int rows_local, int row0, int gny, int nx, int n_az,
                            const int32_t* first, const int32_t* dj, const int32_t* di, const double* dist,
                            const int32_t* window, double height, float* const* outs) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(n_az >= 1 && first && dj && di && dist && window && outs, "shard_sx_multi: NULL argument");
    int up = 0, down = 0;
    sx_reach(dj, dist, first[0], first[n_az], &up, &down);
    Shard s;
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, up, down, "shard_sx_multi", &s));
    std::vector<float*> moved(n_az);
    return run_three(block, s, up, down, [&](const Block& view, int o0, int on) {
        Block b;
        TOPO_TRY(out_block(view, o0, on, up, down, "shard_sx_multi", &b));
        for (int k = 0; k < n_az; ++k) moved[k] = shift(outs[k], o0 - row0, nx);
        return launch_sx_multi(b, n_az, first, dj, di, dist, window, height, moved.data());
    }, false);
}

int topo_amd_shard_valley_ridge(float* block, int rows_local, int row0, int gny, int nx, const float* taps,
                                const int32_t* ksize, const float* angles, int n_angles, int n_planes,
                                float* norm_out, float* dir_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    return shard_valley_ridge(block, rows_local, row0, gny, nx, taps, ksize, angles, n_angles, n_planes, norm_out, dir_out,
                              nullptr);
}

int topo_amd_shard_gaussian(float* block, int rows_local, int row0, int gny, int nx, double sigma_y, double sigma_x,
                            float* out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(block && out, "shard_gaussian: NULL argument");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "shard_gaussian: negative sigma");
    TOPO_REQUIRE(rows_local >= 1 && row0 >= 0 && row0 + rows_local <= gny && nx >= 1,
                 "shard_gaussian: rows [%d, %d) of a raster of %d rows", row0, row0 + rows_local, gny);
    const int g = gauss_ghost_rows(sigma_y);  // == topo_amd_halo_rows(GAUSS, sigma_y)
    Shard s;
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, g, g, "shard_gaussian", &s));
    // the vector-ALU or the matrix-core kernels: a property of the WHOLE raster, never of one shard's rows
    TOPO_TRY(ensure_shard_class(s));
    ClassScope cls(s.owned);
    forget_plane(out, rows_local, nx);
    return smooth_shard_rows(block, s, g, g, sigma_y, sigma_x, g, row0, row0 + rows_local, out);
}

int topo_amd_shard_tpi_std_smoothed(float* block, int rows_local, int row0, int gny, int nx, int size, double sigma,
                                    float* tpi_out, float* std_out) {
    if (!(sigma > 0.0)) return topo_amd_shard_tpi_std(block, rows_local, row0, gny, nx, size, tpi_out, std_out);
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    DiscRuns disc;
    TOPO_TRY(build_disc(size, &disc));
    const int up = -disc.dj_min, down = disc.dj_max;
    Shard s;
    SmoothedPlane sp;
    TOPO_TRY(smoothed_shard(&block, rows_local, row0, gny, nx, up, down, sigma, "shard_tpi_std_smoothed", &s, &sp));
    RasterClass c;
    bool whole = false;
    TOPO_TRY(smoothed_class(sp.row(row0), s, &c, &whole));
    const Block d = sp.block(row0, rows_local, gny);
    ClassScope cls = whole ? ClassScope(d) : ClassScope(c);
    forget_plane(tpi_out, rows_local, nx);
    forget_plane(std_out, rows_local, nx);
    TOPO_TRY(check_block(d, up, down, "shard_tpi_std_smoothed"));
    return launch_tpi_std(d, disc, tpi_out, std_out);
}

int topo_amd_shard_valley_ridge_smoothed(float* block, int rows_local, int row0, int gny, int nx, const float* taps,
                                         const int32_t* ksize, const float* angles, int n_angles, int n_planes,
                                         double sigma, float* norm_out, float* dir_out, double* moments_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    if (!(sigma > 0.0))
        return shard_valley_ridge(block, rows_local, row0, gny, nx, taps, ksize, angles, n_angles, n_planes, norm_out,
                                  dir_out, moments_out);
    TOPO_REQUIRE(block && taps && ksize && angles && norm_out && dir_out && n_angles >= 1,
                 "shard_valley_ridge_smoothed: NULL argument");
    int up = 0, down = 0;
    (void)valley_ridge_reach(ksize, n_angles, &up, &down);
    Shard s;
    SmoothedPlane sp;
    TOPO_TRY(smoothed_shard(&block, rows_local, row0, gny, nx, up, down, sigma, "shard_valley_ridge_smoothed", &s, &sp));
    note_valley_moments(2);  // (the shards' float64 all-reduce)
    // the standardisation of the smoothed field (topo.py:424-427): moments of the owned smoothed rows, all-reduced.
    // (The valley kernels are chosen by the kernel tables alone, never by the raster class: nothing to classify.)
    double mean = 0.0, stdev = 0.0;
    TOPO_TRY(shard_moments(sp.row(row0), rows_local, nx, &mean, &stdev, moments_out));
    const Block d = sp.block(row0, rows_local, gny);
    TOPO_TRY(check_block(d, up, down, "shard_valley_ridge_smoothed"));
    forget_plane(norm_out, rows_local, nx);
    forget_plane(dir_out, rows_local, nx);
    return launch_valley_ridge(d, taps, ksize, angles, n_angles, n_planes, mean, stdev, norm_out, dir_out);
}

// numpy's own float32 mean() / std() of the whole sharded raster: see include/topo_amd.h
int topo_amd_shard_mean_std_f32(const float* owned, int rows_local, int row0, int gny, int nx, size_t chunk, float* mean,
                                float* stdev) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(mean && stdev, "shard_mean_std_f32: NULL output");
    return shard_mean_std_np(owned, rows_local, row0, gny, nx, chunk, mean, stdev);
}

int topo_amd_shard_valley_ridge_std(float* block, int rows_local, int row0, int gny, int nx, const float* taps,
                                    const int32_t* ksize, const float* angles, int n_angles, int n_planes, double sigma,
                                    size_t chunk, float* norm_out, float* dir_out, float moments_out[2]) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(np_chunk_ok(chunk), "shard_valley_ridge_std: chunk %zu (a power of two, 128 at least)", chunk);
    if (!(sigma > 0.0))
        return shard_valley_ridge(block, rows_local, row0, gny, nx, taps, ksize, angles, n_angles, n_planes, norm_out, dir_out,
                                  nullptr, chunk, moments_out);
    TOPO_REQUIRE(block && taps && ksize && angles && norm_out && dir_out && n_angles >= 1, "shard_valley_ridge_std: NULL argument");
    int up = 0, down = 0;
    (void)valley_ridge_reach(ksize, n_angles, &up, &down);
    Shard s;
    SmoothedPlane sp;
    TOPO_TRY(smoothed_shard(&block, rows_local, row0, gny, nx, up, down, sigma, "shard_valley_ridge_std", &s, &sp));
    // the standardisation of the smoothed field (topo.py:424-427) with numpy's float32 moments of the whole smoothed raster:
    // the parts of the OWNED smoothed rows of every rank, where _smoothed takes its float64 moments
    float mean = 0.0f, stdev = 0.0f;
    TOPO_TRY(shard_mean_std_np(sp.row(row0), rows_local, row0, gny, nx, chunk, &mean, &stdev));
    note_valley_moments(3);
    if (moments_out) moments_out[0] = mean, moments_out[1] = stdev;
    const Block d = sp.block(row0, rows_local, gny);
    TOPO_TRY(check_block(d, up, down, "shard_valley_ridge_std"));
    forget_plane(norm_out, rows_local, nx);
    forget_plane(dir_out, rows_local, nx);
    return launch_valley_ridge(d, taps, ksize, angles, n_angles, n_planes, (double)mean, (double)stdev, norm_out, dir_out);
}

int topo_amd_shard_fill_na(float* block, int rows_local, int row0, int gny, int nx, const double* x_coords,
                           double min_elevation, float* out, uint8_t* missing) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Shard s;  // (its view of no ghost rows starts at the owned rows: rows are independent, no exchange)
    TOPO_TRY(open_shard(&block, rows_local, row0, gny, nx, 0, 0, "shard_fill_na", &s));
    // (out == the owned rows: in place; topo_amd_fill_na_dev drops the class declared for them, and the next sharded
    // call re-classifies collectively - so every rank makes this call, or none)
    return topo_amd_fill_na_dev(block, rows_local, row0, gny, nx, x_coords, min_elevation, row0, rows_local, out, missing);
}

}  // extern "C"
