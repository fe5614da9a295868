// C ABI of libtopo_amd.so (declared in include/topo_amd.h), the context: error plumbing, the call guard, workspaces and
// parameter tables, init / shutdown, memory, copies, timers and marks.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "capi.hpp"

namespace topo {

static thread_local std::string g_error;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}

Context& ctx() {
    static Context c;
    return c;
}

std::recursive_mutex& call_mutex() {
    static std::recursive_mutex mu;
    return mu;
}
namespace {
thread_local int t_bound_device = -1;  // the device this thread's HIP calls go to, as far as the library has set it
}
CallGuard::CallGuard() : lock(call_mutex()) {
    const Context& c = ctx();
    if (c.ready && t_bound_device != c.device) {
        if (hipSetDevice(c.device) == hipSuccess) t_bound_device = c.device;
    }
}

int require_ready() {
    if (!ctx().ready) {
        set_error("libtopo_amd: call topo_amd_init(device) first");
        return TOPO_AMD_ENODEV;
    }
    return TOPO_AMD_OK;
}

int workspace(int slot, size_t bytes, void** out) {
    Context& c = ctx();
    if (c.ws_bytes[slot] < bytes) {
        if (c.ws[slot]) {
            TOPO_HIP(hipStreamSynchronize(c.compute));
            TOPO_HIP(hipFree(c.ws[slot]));
            c.ws[slot] = nullptr;
            c.ws_bytes[slot] = 0;
        }
        TOPO_HIP(hipMalloc(&c.ws[slot], bytes));
        c.ws_bytes[slot] = bytes;
        dem_memo_forget(c.ws[slot], bytes);  // (a recycled address)
    }
    *out = c.ws[slot];
    return TOPO_AMD_OK;
}

// Small parameter tables: pinned staging + async copy on the compute stream.  The previous
// content is remembered so a loop over the same parameters uploads nothing.
namespace {
struct TableSlot {
    void* pinned = nullptr;
    size_t cap = 0;
    std::vector<char> last;
    hipEvent_t copied = nullptr;
};
TableSlot g_slots[kTables];
}  // namespace

int upload_table(int slot, const void* host, size_t bytes, void** out) {
    Context& c = ctx();
    TableSlot& s = g_slots[slot];
    if (bytes == 0) bytes = 4;
    if (c.tab_bytes[slot] < bytes || s.cap < bytes) {
        const size_t cap = bytes * 2 + 256;
        TOPO_HIP(hipStreamSynchronize(c.compute));
        if (c.tab[slot]) TOPO_HIP(hipFree(c.tab[slot]));
        if (s.pinned) TOPO_HIP(hipHostFree(s.pinned));
        TOPO_HIP(hipMalloc(&c.tab[slot], cap));
        TOPO_HIP(hipHostMalloc(&s.pinned, cap, hipHostMallocDefault));
        c.tab_bytes[slot] = cap;
        s.cap = cap;
        s.last.clear();
        if (!s.copied) TOPO_HIP(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    }
    if (s.last.size() != bytes || std::memcmp(s.last.data(), host, bytes) != 0) {
        if (!s.last.empty()) TOPO_HIP(hipEventSynchronize(s.copied));  // staging still in use?
        std::memcpy(s.pinned, host, bytes);
        TOPO_HIP(hipMemcpyAsync(c.tab[slot], s.pinned, bytes, hipMemcpyHostToDevice, c.compute));
        TOPO_HIP(hipEventRecord(s.copied, c.compute));
        s.last.assign((const char*)host, (const char*)host + bytes);
    }
    *out = c.tab[slot];
    return TOPO_AMD_OK;
}

int check_block(const Block& b, int need_above, int need_below, const char* who) {
    TOPO_REQUIRE(b.in != nullptr, "%s: input pointer is NULL", who);
    TOPO_REQUIRE(b.gny >= 1 && b.nx >= 1, "%s: empty DEM %d x %d", who, b.gny, b.nx);
    TOPO_REQUIRE(b.in_rows >= 1 && b.in_row0 >= 0 && b.in_row0 + b.in_rows <= b.gny,
                 "%s: block rows [%d, %d) outside the DEM of %d rows", who, b.in_row0,
                 b.in_row0 + b.in_rows, b.gny);
    TOPO_REQUIRE(b.out_rows >= 1 && b.out_row0 >= 0 && b.out_row0 + b.out_rows <= b.gny,
                 "%s: output rows [%d, %d) outside the DEM of %d rows", who, b.out_row0,
                 b.out_row0 + b.out_rows, b.gny);
    const int first = std::max(0, b.out_row0 - need_above);
    const int last = std::min(b.gny, b.out_row0 + b.out_rows + need_below);
    TOPO_REQUIRE(b.in_row0 <= first && b.in_row0 + b.in_rows >= last,
                 "%s: block rows [%d, %d) do not cover the %d/%d ghost rows needed by output rows "
                 "[%d, %d)", who, b.in_row0, b.in_row0 + b.in_rows, need_above, need_below,
                 b.out_row0, b.out_row0 + b.out_rows);
    return TOPO_AMD_OK;
}

}  // namespace topo

using namespace topo;

extern "C" {

const char* topo_amd_version(void) { return "topo_amd 0.1.0 (gfx950)"; }
const char* topo_amd_last_error(void) { return g_error.c_str(); }

int topo_amd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int topo_amd_init(int device) {
    TOPO_ENTER();
    Context& c = ctx();
    if (c.ready && c.device == device) return TOPO_AMD_OK;
    if (c.ready) {
        set_error("topo_amd_init: already bound to device %d (one process drives one GPU)", c.device);
        return TOPO_AMD_EINVAL;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        set_error("topo_amd_init: no HIP device visible");
        return TOPO_AMD_ENODEV;
    }
    TOPO_REQUIRE(device >= 0 && device < n, "topo_amd_init: device %d not in [0, %d)", device, n);
    TOPO_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    TOPO_HIP(hipGetDeviceProperties(&prop, device));
    c.num_cu = prop.multiProcessorCount;
    // TOPO_AMD_CU_LIMIT=<n>: persistent kernels size their grids for at most n compute units (to
    // leave room for other work on the GPU; the results do not depend on it)
    if (const char* lim = std::getenv("TOPO_AMD_CU_LIMIT")) {
        const int n = std::atoi(lim);
        if (n >= 8 && n < c.num_cu) c.num_cu = n;
    }
    TOPO_HIP(hipStreamCreateWithFlags(&c.compute, hipStreamNonBlocking));
    {
        // the ghost-row exchange goes on a high-priority stream: RCCL's few workgroups are dispatched ahead of the
        // pending workgroups of a grid kernel on the compute stream (which otherwise refill every slot that frees up
        // and leave the exchange for the end of the launch: Sx, kernel trace in profiles/r04_shard_fused.txt)
        int least = 0, greatest = 0;
        TOPO_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        TOPO_HIP(hipStreamCreateWithPriority(&c.comm, hipStreamNonBlocking, greatest));
    }
    TOPO_HIP(hipEventCreateWithFlags(&c.halo_done, hipEventDisableTiming));
    TOPO_HIP(hipEventCreateWithFlags(&c.input_ready, hipEventDisableTiming));
    TOPO_HIP(hipEventCreate(&c.t0));
    TOPO_HIP(hipEventCreate(&c.t1));
    // the ghost-row gate (common.hpp): a device word the communication stream stamps with the exchange epoch, and a
    // pinned host word in which blocks that gave up waiting count themselves
    TOPO_HIP(hipMalloc((void**)&c.gate_word, kGateBytes));
    TOPO_HIP(hipMemset(c.gate_word, 0, kGateBytes));
    TOPO_HIP(hipHostMalloc((void**)&c.gate_timeouts, 64, hipHostMallocMapped));
    reset_shard();
    c.gate_timeouts[0] = 0;  // blocks that gave up at a closed gate (careful mode)
    c.gate_timeouts[4] = 0;  // blocks whose wait ran out (lean mode): an error
    c.gate_epoch = 0;
    c.gate_mode = 0;
    c.gate_clean_calls = 0;
    c.gate_probe_pending = false;
    TOPO_HIP(hipEventCreateWithFlags(&c.gate_probe, hipEventDisableTiming));
    c.device = device;
    c.ready = true;
    return TOPO_AMD_OK;
}

// Per-launch timing without a host synchronise per launch: numbered HIP events on the compute stream.
namespace {
constexpr int kMarks = 512;
hipEvent_t g_marks[kMarks] = {};
}  // namespace

int topo_amd_shutdown(void) {
    TOPO_ENTER();
    Context& c = ctx();
    if (!c.ready) return TOPO_AMD_OK;
    (void)hipDeviceSynchronize();
    release_shard();
    release_raster_class();
    valley_fft_release();  // FFT plans hold the stream that goes away below
    for (int i = 0; i < kWorkspaces; ++i)
        if (c.ws[i]) (void)hipFree(c.ws[i]);
    for (int i = 0; i < kTables; ++i) {
        if (c.tab[i]) (void)hipFree(c.tab[i]);
        if (g_slots[i].pinned) (void)hipHostFree(g_slots[i].pinned);
        if (g_slots[i].copied) (void)hipEventDestroy(g_slots[i].copied);
        g_slots[i] = TableSlot();
    }
    for (auto& e : g_marks) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (c.gate_word) (void)hipFree(c.gate_word);
    if (c.gate_timeouts) (void)hipHostFree(c.gate_timeouts);
    if (c.gate_probe) (void)hipEventDestroy(c.gate_probe);
    (void)hipEventDestroy(c.halo_done);
    (void)hipEventDestroy(c.input_ready);
    (void)hipEventDestroy(c.t0);
    (void)hipEventDestroy(c.t1);
    (void)hipStreamDestroy(c.compute);
    (void)hipStreamDestroy(c.comm);
    for (void* q : c.host_planes)
        if (q) (void)hipFree(q);
    if (c.up) {
        (void)hipStreamDestroy(c.up);
        (void)hipStreamDestroy(c.down);
    }
    for (hipEvent_t e : c.pipe_events) (void)hipEventDestroy(e);
    if (c.aux) {
        (void)hipStreamDestroy(c.aux);
        for (auto& e : c.aux_ready) (void)hipEventDestroy(e);
        (void)hipEventDestroy(c.aux_done);
    }
    c = Context();
    return TOPO_AMD_OK;
}

int topo_amd_device_name(char* buf, int buflen) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    hipDeviceProp_t prop;
    TOPO_HIP(hipGetDeviceProperties(&prop, ctx().device));
    // (the runtime of this image reports an empty marketing name for the MI355X)
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name[0] ? prop.name : "AMD Instinct", prop.gcnArchName, prop.multiProcessorCount);
    return TOPO_AMD_OK;
}

int topo_amd_cu_count(void) {
    TOPO_ENTER();
    if (require_ready() != TOPO_AMD_OK) return TOPO_AMD_ENODEV;
    return ctx().num_cu;
}

int topo_amd_malloc(void** dptr, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(dptr != nullptr, "topo_amd_malloc: NULL result pointer");
    TOPO_HIP(hipMalloc(dptr, bytes ? bytes : 4));
    dem_memo_forget(*dptr, bytes ? bytes : 4);
    return TOPO_AMD_OK;
}

int topo_amd_free(void* dptr) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    if (dptr) {
        TOPO_HIP(hipStreamSynchronize(ctx().compute));
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dptr) == hipSuccess) dem_memo_forget(base, size);
        else (void)hipGetLastError();
        dem_memo_forget(dptr, 0);
        TOPO_HIP(hipFree(dptr));
    }
    return TOPO_AMD_OK;
}

// Page-locked host memory for the arrays handed to the host-buffer entry points (topo_amd_*_f32): the copies then run
// at the link's rate without the driver staging them (bench.py, end_to_end: pinned against pageable).
int topo_amd_host_alloc(void** hptr, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(hptr != nullptr && bytes > 0, "host_alloc: bad arguments");
    TOPO_HIP(hipHostMalloc(hptr, bytes, hipHostMallocDefault));
    return TOPO_AMD_OK;
}
int topo_amd_host_free(void* hptr) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    if (hptr) TOPO_HIP(hipHostFree(hptr));
    return TOPO_AMD_OK;
}

int topo_amd_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    dem_memo_forget(dst, bytes);
    TOPO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx().compute));
    TOPO_HIP(hipStreamSynchronize(ctx().compute));
    return TOPO_AMD_OK;
}

int topo_amd_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    // a destination fresh from the allocator has no pages yet: fault them in from several
    // threads (the kernels launched before this call are usually still running meanwhile)
    prefault_pages(dst, bytes);
    TOPO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx().compute));
    TOPO_HIP(hipStreamSynchronize(ctx().compute));
    return check_gate_errors();
}

int topo_amd_memcpy_d2d(void* dst, const void* src, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    dem_memo_forget(dst, bytes);
    TOPO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx().compute));
    return TOPO_AMD_OK;
}

int topo_amd_memset(void* dst, int value, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    dem_memo_forget(dst, bytes);
    TOPO_HIP(hipMemsetAsync(dst, value, bytes, ctx().compute));
    return TOPO_AMD_OK;
}

int topo_amd_sync(void) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_HIP(hipStreamSynchronize(ctx().compute));
    TOPO_HIP(hipStreamSynchronize(ctx().comm));
    return check_gate_errors();
}

int topo_amd_timer_start(void) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_HIP(hipEventRecord(ctx().t0, ctx().compute));
    return TOPO_AMD_OK;
}

int topo_amd_timer_stop(float* elapsed_ms) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_HIP(hipEventRecord(ctx().t1, ctx().compute));
    TOPO_HIP(hipEventSynchronize(ctx().t1));
    TOPO_HIP(hipEventElapsedTime(elapsed_ms, ctx().t0, ctx().t1));
    return check_gate_errors();
}

int topo_amd_mark(int index) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(index >= 0 && index < kMarks, "mark: index %d outside [0, %d)", index, kMarks);
    if (!g_marks[index]) TOPO_HIP(hipEventCreate(&g_marks[index]));
    TOPO_HIP(hipEventRecord(g_marks[index], ctx().compute));
    return TOPO_AMD_OK;
}

int topo_amd_mark_elapsed(int from, int to, float* elapsed_ms) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(from >= 0 && from < kMarks && to >= 0 && to < kMarks && g_marks[from] && g_marks[to] && elapsed_ms,
                 "mark_elapsed: marks %d and %d must have been recorded", from, to);
    TOPO_HIP(hipEventSynchronize(g_marks[to]));
    TOPO_HIP(hipEventElapsedTime(elapsed_ms, g_marks[from], g_marks[to]));
    return check_gate_errors();
}

}  // extern "C"
