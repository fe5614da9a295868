// C ABI of libtopo_amd.so (declared in include/topo_amd.h), the host-buffer entry points: a caller's array goes up, the
// device entry points (capi.hip) run on it, the result planes come down - in row chunks that overlap the three.
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <thread>

#include <sys/mman.h>

#include "capi.hpp"
#include "decode.hpp"
#include "encode.hpp"

namespace topo {
namespace {

thread_local int t_host_chunks = 0;  // row chunks of the calling thread's last host-buffer call (topo_amd_host_chunks)
// The device planes of one call: the k-th plane it asks for is the k-th plane of the context's pool (Context::host_planes),
// grown when it must be.
struct PlanePool {
    std::vector<void*> bufs;
    std::vector<size_t> sizes;
    ~PlanePool() {
        for (size_t k = 0; k < bufs.size(); ++k) dem_memo_forget(bufs[k], sizes[k]);  // (the planes stay; what was known about their content goes)
    }
    int alloc(void** p, size_t bytes) {
        Context& c = ctx();
        const size_t k = bufs.size();
        if (c.host_planes.size() <= k) {
            c.host_planes.resize(k + 1, nullptr);
            c.host_plane_bytes.resize(k + 1, 0);
        }
        if (c.host_plane_bytes[k] < bytes) {
            if (c.host_planes[k]) {
                TOPO_HIP(hipStreamSynchronize(c.compute));
                TOPO_HIP(hipFree(c.host_planes[k]));
                c.host_planes[k] = nullptr;
                c.host_plane_bytes[k] = 0;
            }
            TOPO_HIP(hipMalloc(&c.host_planes[k], bytes));
            c.host_plane_bytes[k] = bytes;
        }
        *p = c.host_planes[k];
        bufs.push_back(*p);
        sizes.push_back(bytes);
        dem_memo_forget(*p, c.host_plane_bytes[k]);  // (another call's data: nothing is known about this plane)
        return TOPO_AMD_OK;
    }
};
// The preparation of a call's result arrays.  A result array fresh from the allocator has no pages yet; faulting them in one
// by one under the download is what a host-buffer call spends most of its time on (tools/ubench/page_touch.cpp: 92 ms per GiB
// against 19 ms for the copy itself).  prefault() asks for huge pages and touches the array from a few threads while the
// upload and the kernels run; ready() joins them before the first download.
struct PageToucher {
    std::vector<std::thread> touchers;
    ~PageToucher() { ready(); }
    void prefault(void* host, size_t bytes) {
        constexpr uintptr_t kPage = 4096, kHuge = (uintptr_t)2 << 20;
        static const bool enabled = [] {
            const char* e = std::getenv("TOPO_AMD_HOST_PREFAULT");  // 0 switches it off (for measurements)
            return !(e && e[0] == '0');
        }();
        if (!enabled || !host || bytes < 4 * kHuge) return;
        const uintptr_t lo = ((uintptr_t)host + kPage - 1) & ~(kPage - 1);
        const uintptr_t hi = ((uintptr_t)host + bytes) & ~(kPage - 1);
        if (hi <= lo) return;
        (void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);  // a hint; refused where THP is off
        const unsigned hw = std::thread::hardware_concurrency();
        const uintptr_t n = std::min<uintptr_t>(hw >= 16 ? 8 : (hw >= 4 ? 2 : 1), (hi - lo) / kHuge);
        const uintptr_t per = (((hi - lo) / n) + kHuge - 1) & ~(kHuge - 1);
        for (uintptr_t a = lo; a < hi; a += per) {
            const uintptr_t b = std::min(a + per, hi);
            try {
                touchers.emplace_back([a, b] {
                    // read and write back one byte per page: the array keeps whatever it held
                    for (uintptr_t q = a; q < b; q += kPage) {
                        volatile char* c = (volatile char*)q;
                        *c = *c;
                    }
                });
            } catch (...) {
                return;  // no thread to be had: the download faults the remaining pages in itself
            }
        }
    }
    void ready() {
        for (auto& t : touchers) t.join();
        touchers.clear();
    }
};

// One result plane of a host-buffer call: the caller's array - checked once, by make_plane() for a topo_amd_plane, or any
// array of `elem` bytes a sample that is downloaded as the kernels write it (HostCall::stored) - and, once HostCall::add()
// has bound it, its device planes.  host == nullptr: absent (a NULL struct or NULL data, where the call allows it).
struct HostPlane {
    void* host = nullptr;
    void* dev = nullptr;          // what is downloaded
    size_t elem = sizeof(float);  // bytes per sample (the missing mask of topo_amd_fill_na_f32: 1; a packed plane: 1 or 2)
    // A packed result plane (include/topo_amd.h): the kernels write the float32 device plane `f32`, its rows are encoded
    // behind them into the packed device plane `dev` - taken from the pool by HostCall::run, behind every plane a float32
    // call takes - and `dev` is what gets downloaded.  f32 == nullptr: a plane downloaded as the kernels write it.
    const float* f32 = nullptr;
    EncodeParams enc;
    topo_amd_plane* report = nullptr;  // the caller's struct: its counters are written after the last chunk
    void** pool = nullptr;             // a multi-scale call: where the packed device plane (2 bytes a sample) is kept between its scales
    explicit operator bool() const { return host != nullptr; }
    bool packed() const { return host != nullptr && f32 != nullptr; }
    size_t bytes(int ny, int nx) const { return (size_t)ny * nx * elem; }
    void* host_row(int r, int nx) const { return (char*)host + (size_t)r * nx * elem; }
    const void* dev_row(int r, int nx) const { return (const char*)dev + (size_t)r * nx * elem; }
};
int make_plane(topo_amd_plane* plane, const char* who, HostPlane* h) {
    *h = HostPlane();
    if (!plane || !plane->data) return TOPO_AMD_OK;
    TOPO_TRY(make_encode(plane, who, &h->enc));
    plane->missing = plane->saturated = 0;
    h->host = plane->data;
    h->elem = plane_sample_bytes(h->enc.dtype);
    h->report = plane;
    return TOPO_AMD_OK;
}
topo_amd_plane f32_plane(float* p) { return topo_amd_plane{p, TOPO_AMD_F32, 0, 1.0, 0.0, 0.0, 0, 0}; }
int pipeline_chunk_rows(int ny, int nx) {
    const char* e = std::getenv("TOPO_AMD_HOST_PIPELINE");
    if (e && *e == '0') return ny;
    e = std::getenv("TOPO_AMD_HOST_CHUNK_MB");
    const double chunk_mb = e && *e ? std::max(1.0, std::atof(e)) : 64.0;
    // whole tile rows of every kernel (60 and 64: 960), at least 960 rows
    long rows = (long)(chunk_mb * 1048576.0 / ((double)nx * sizeof(float)));
    rows = std::max(960L, rows / 960 * 960);
    return rows * 3 > ny ? ny : (int)rows;  // fewer than three chunks: nothing to overlap
}
// The row cuts of a call, chunk k being rows [cut[k], cut[k + 1]): {0, ny} for a call that is not cut (one_chunk, or what
// pipeline_chunk_rows says), else chunks of that many rows, the last one half a chunk to a chunk and a half (no sliver at the
// end) - three chunks at least.
// (Round 6 tried a taper - a quarter and a half chunk at both ends, so that less stands in front of the first kernels and
// behind the last ones: 16384^2 TPI 67 px 26.05 -> 25.93 ms page-locked, 24.97 -> 24.80 pageable, profiles/r06_host_pipeline.txt:
// the fill and the drain are not what separates the call from the 22.4 ms of 1 GiB each way at 48 GB/s.  Not kept.)
std::vector<int> row_cuts(int ny, int nx, bool one_chunk) {
    const int chunk = one_chunk ? ny : pipeline_chunk_rows(ny, nx);
    std::vector<int> cut{0};
    for (int at = 0; chunk < ny && ny - at > chunk + chunk / 2;) cut.push_back(at += chunk);
    cut.push_back(ny);
    return cut;
}
// The caller's raster as a host-buffer call sees it: a checked topo_amd_raster.  as_stored: float32 that needs no decode (the
// *_f32 path: copied straight into the float32 plane, no raw plane, no decode launch).
struct Source {
    const char* data = nullptr;
    int dtype = TOPO_AMD_F32;
    size_t elem = sizeof(float);
    DecodeParams p;
    bool as_stored = true;
    const char* row(int r, int nx) const { return data + (size_t)r * nx * elem; }
};
int make_source(const topo_amd_raster* r, const char* who, Source* s) {
    TOPO_REQUIRE(r != nullptr && r->data != nullptr, "%s: bad DEM", who);
    s->elem = sample_bytes(r->dtype);
    TOPO_REQUIRE(s->elem != 0, "%s: unknown sample type %d (TOPO_AMD_F32 ... TOPO_AMD_F64)", who, (int)r->dtype);
    TOPO_REQUIRE(std::isfinite(r->scale) && r->scale != 0.0, "%s: scale %g (it must be finite and not 0)", who, r->scale);
    TOPO_REQUIRE(std::isfinite(r->offset), "%s: offset %g is not finite", who, r->offset);
    s->data = (const char*)r->data;
    s->dtype = r->dtype;
    s->p.scale = r->scale;
    s->p.offset = r->offset;
    s->p.has_nodata = r->has_nodata != 0 && !std::isnan(r->nodata);  // (NaN equals nothing: "none")
    s->p.nodata = s->p.has_nodata ? r->nodata : 0.0;
    s->as_stored = r->dtype == TOPO_AMD_F32 && r->scale == 1.0 && r->offset == 0.0 && !s->p.has_nodata;
    return TOPO_AMD_OK;
}
topo_amd_raster f32_raster(const float* dem) { return topo_amd_raster{dem, TOPO_AMD_F32, 0, 1.0, 0.0, 0.0}; }
RasterClass scan_source(const Source& s, int ny, int nx) { return scan_host_raster(s.data, s.dtype, s.p, s.as_stored, ny, nx); }
// rows [r0, r1) of the source -> the same rows of the float32 plane d_in, enqueued on `stream`: a copy, or a copy into the
// raw plane d_raw and the decode behind it
hipError_t enqueue_rows(const Source& s, char* d_raw, float* d_in, int r0, int r1, int nx, hipStream_t stream) {
    const size_t count = (size_t)(r1 - r0) * nx;
    if (s.as_stored) return hipMemcpyAsync(d_in + (size_t)r0 * nx, s.row(r0, nx), count * sizeof(float), hipMemcpyHostToDevice, stream);
    char* raw = d_raw + (size_t)r0 * nx * s.elem;
    hipError_t e = hipMemcpyAsync(raw, s.row(r0, nx), count * s.elem, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    if (launch_decode(stream, raw, s.dtype, count, s.p, d_in + (size_t)r0 * nx) != TOPO_AMD_OK) return hipErrorLaunchFailure;
    return hipSuccess;
}
// the raw plane of a call (nullptr for a source that needs none): the LAST plane a call takes from the pool, so the planes
// of a float32 call are the ones they always were
int raw_plane(PlanePool& pool, const Source& s, int ny, int nx, char** d_raw) {
    *d_raw = nullptr;
    if (s.as_stored) return TOPO_AMD_OK;
    void* p = nullptr;
    TOPO_TRY(pool.alloc(&p, (size_t)ny * nx * s.elem));
    *d_raw = (char*)p;
    return TOPO_AMD_OK;
}

// The missing / saturated counters of the encode kernels: one pair per plane, in a workspace of their own.  reserve() zeroes
// them on the compute stream, in front of the launches that get pair(q); fetch() enqueues their copy back; behind the caller's
// synchronise, store() puts pair q into a caller's struct.
struct EncodeCounts {
    unsigned long long* dev = nullptr;
    std::vector<unsigned long long> host;
    int reserve(size_t planes) {
        void* w = nullptr;
        TOPO_TRY(workspace(kEncodeCountsSlot, planes * 2 * sizeof(unsigned long long), &w));
        dev = (unsigned long long*)w;
        host.assign(planes * 2, 0);
        TOPO_HIP(hipMemsetAsync(dev, 0, host.size() * sizeof(unsigned long long), ctx().compute));
        return TOPO_AMD_OK;
    }
    unsigned long long* pair(size_t q) const { return dev + 2 * q; }
    int fetch() {
        if (dev) TOPO_HIP(hipMemcpyAsync(host.data(), dev, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx().compute));
        return TOPO_AMD_OK;
    }
    void store(size_t q, topo_amd_plane* plane) const {
        plane->missing = host[2 * q];
        plane->saturated = host[2 * q + 1];
    }
};

// the two copy streams of the pipelined calls and n of their events (Context::up / down / pipe_events: created on first use)
int copy_streams(int n) {
    Context& c = ctx();
    if (!c.up) {
        TOPO_HIP(hipStreamCreateWithFlags(&c.up, hipStreamNonBlocking));
        TOPO_HIP(hipStreamCreateWithFlags(&c.down, hipStreamNonBlocking));
    }
    while ((int)c.pipe_events.size() < n) {
        hipEvent_t e = nullptr;
        TOPO_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c.pipe_events.push_back(e);
    }
    return TOPO_AMD_OK;
}

// One host-buffer call, for as long as its entry point runs: the checked source, the shape, the device planes it takes from
// the context's pool and its result planes.
// POOL ORDER - pool slots only grow, so a changed order makes alternating calls reallocate, and copies out of fresh device
// memory run at half rate.  A call takes: d_in (open), the wanted result planes in the order they are
// registered (plane / stored / shared), the call's extras (extra), and in run() the raw plane of a source that is decoded on
// the device, then the packed device planes.
constexpr bool kRowChunks = false, kOneChunk = true;
struct HostCall {
    Source src;
    int ny = 0, nx = 0;
    const char* who = "";
    float* d_in = nullptr;
    PlanePool pool;     // (released behind the page threads: declared in front of them)
    PageToucher pages;
    std::vector<HostPlane> outs;
    bool uploaded = false;  // the DEM is on the device: every run() but the first (the later scales of a multi-scale call)

    // the source and the shape checked, the chunk counter reset, d_in taken
    int open(const topo_amd_raster* raster, int rows, int cols, const char* name, const char* bad_shape = "bad DEM") {
        who = name;
        TOPO_TRY(make_source(raster, who, &src));
        TOPO_REQUIRE(rows >= 1 && cols >= 1, "%s: %s", who, bad_shape);
        ny = rows;
        nx = cols;
        t_host_chunks = 0;
        return extra(&d_in);
    }
    size_t samples() const { return (size_t)ny * nx; }
    template <class T>
    int extra(T** p) {  // a device plane of ny x nx samples of T
        void* q = nullptr;
        TOPO_TRY(pool.alloc(&q, samples() * sizeof(T)));
        *p = (T*)q;
        return TOPO_AMD_OK;
    }
    // a checked plane on the device plane the kernels write for it (nullptr: not wanted); pool: see HostPlane
    void add(HostPlane h, void* dev, void** packed_pool = nullptr) {
        if (!dev) h.host = nullptr;
        if (h.host && !h.enc.plain()) {
            h.f32 = (const float*)dev;
            h.pool = packed_pool;
        } else {
            h.dev = dev;
        }
        outs.push_back(h);
    }
    // registers a plane of the caller's: checked, its device plane taken (*dev; nullptr when the plane is absent), its pages
    // being touched, in the list of what run() downloads
    int plane(topo_amd_plane* p, float** dev) {
        HostPlane h;
        TOPO_TRY(make_plane(p, who, &h));
        *dev = nullptr;
        if (h) TOPO_TRY(extra(dev));
        pages.prefault(h.host, h.bytes(ny, nx));
        add(h, *dev);
        return TOPO_AMD_OK;
    }
    // ... an array that takes the samples as the kernels write them: float32 only (sobel), the uint8 mask of fill_na
    template <class T>
    int stored(T* host, T** dev) {
        *dev = nullptr;
        if (host) TOPO_TRY(extra(dev));
        in_place(host, *dev);
        return TOPO_AMD_OK;
    }
    // ... on a device plane the call has already (fill_na fills d_in itself)
    template <class T>
    void in_place(T* host, T* dev) {
        HostPlane h;
        h.host = host;
        h.elem = sizeof(T);
        pages.prefault(host, h.bytes(ny, nx));
        add(h, dev);
    }
    // ... planes that take turns on one device plane (the scales of a multi-scale call): that plane if any of them is wanted,
    // the pages of all; each scale add()s its own in front of its run()
    int shared(const std::vector<HostPlane>& planes, float** dev) {
        *dev = nullptr;
        if (std::any_of(planes.begin(), planes.end(), [](const HostPlane& h) { return (bool)h; })) TOPO_TRY(extra(dev));
        for (const HostPlane& h : planes) pages.prefault(h.host, h.bytes(ny, nx));
        return TOPO_AMD_OK;
    }
    float* at(float* p, int r0) const { return shift(p, r0, nx); }
    template <class Compute>
    int run(int below, bool one_chunk, Compute&& compute);
};

// ---- upload || kernels || download in row chunks -------------------------------------------------------
// A host-buffer call used to be three serial steps - 18.7 ms up, 1.3 ms of kernels, 19.9 ms down for TPI 67 px on 16384^2 -
// over a link that carries both directions at once (48.6 GB/s each way against 57 one way, profiles/r01_host_path.txt).  Row
// blocks give the single block's bits, so the call is cut into row chunks: the calling thread uploads chunk k on one
// stream and, as soon as the rows a chunk's outputs depend on are on the device, enqueues its kernels (on the block view
// "the rows uploaded so far") on the compute stream; a second host thread downloads the output rows of every finished
// chunk on a third stream (its own thread because copies to and from pageable memory block the caller).
// TOPO_AMD_HOST_PIPELINE=0: one chunk (the old order).  TOPO_AMD_HOST_CHUNK_MB: size of a chunk of the DEM (default 64).
// TOPO_AMD_HOST_DOWNLOADS=thread / inline: who issues the downloads (default: by the arrays, below).  All three are read at
// every call (a getenv each), so a test can walk through them in one process.
// compute(view, r0): enqueue the kernels that write the output rows of the block `view` - rows [r0, r0 + view.out_rows) of
// every plane - reading the rows of d_in that are uploaded so far (the whole of view).  below: rows of the DEM beneath an
// output row that it depends on.  A source that is not float32-as-stored goes chunk by chunk into a raw device plane and is
// decoded into d_in on the stream of the copy, in front of the event the kernels wait for.
// one_chunk: the call is not cut, whatever TOPO_AMD_HOST_* say.
template <class Compute>
int HostCall::run(int below, bool one_chunk, Compute&& compute_view) {
    Context& c = ctx();
    const bool upload = !uploaded;
    uploaded = true;
    auto compute = [&](int view_rows, int r0, int rows) { return compute_view(Block{d_in, view_rows, 0, ny, nx, r0, rows}, r0); };
    char* d_raw = nullptr;
    if (upload) TOPO_TRY(raw_plane(pool, src, ny, nx, &d_raw));
    // packed result planes: their device planes (behind every plane a float32 call takes), one pair of counters each
    EncodeCounts counts;
    for (HostPlane& o : outs) {
        if (!o.packed()) continue;
        if (o.pool && *o.pool) {
            o.dev = *o.pool;
        } else {
            TOPO_TRY(pool.alloc(&o.dev, samples() * (o.pool ? 2 : o.elem)));
            if (o.pool) *o.pool = o.dev;
        }
    }
    const bool any_packed = std::any_of(outs.begin(), outs.end(), [](const HostPlane& o) { return o.packed(); });
    if (any_packed) TOPO_TRY(counts.reserve(outs.size()));
    // rows [r0, r1) of every packed plane: float32 -> codes, on the compute stream behind the kernels that wrote them
    auto encode_rows = [&](int r0, int r1) -> int {
        for (size_t q = 0; q < outs.size(); ++q) {
            const HostPlane& o = outs[q];
            if (!o.packed()) continue;
            TOPO_TRY(launch_encode(c.compute, o.f32 + (size_t)r0 * nx, (size_t)(r1 - r0) * nx, o.enc, (char*)o.dev + (size_t)r0 * nx * o.elem,
                                   counts.pair(q)));
        }
        return TOPO_AMD_OK;
    };
    // behind the last download: the compute stream drains, the counters go into the callers' structs
    auto finish = [&]() -> int {
        TOPO_TRY(counts.fetch());
        TOPO_HIP(hipStreamSynchronize(c.compute));
        for (size_t q = 0; q < outs.size(); ++q)
            if (outs[q].packed() && outs[q].report) counts.store(q, outs[q].report);
        return TOPO_AMD_OK;
    };
    const std::vector<int> cut = row_cuts(ny, nx, one_chunk);
    const int nchunks = (int)cut.size() - 1;
    t_host_chunks = std::max(t_host_chunks, nchunks);  // (a multi-scale call: the most any of its scales ran in)
    if (nchunks == 1) {
        if (upload) TOPO_HIP(enqueue_rows(src, d_raw, d_in, 0, ny, nx, c.compute));
        const int rc = compute(ny, 0, ny);
        if (rc != TOPO_AMD_OK && rc != TOPO_AMD_EEMPTY) return rc;
        TOPO_TRY(encode_rows(0, ny));
        pages.ready();
        for (const HostPlane& o : outs)
            if (o.host) TOPO_HIP(hipMemcpyAsync(o.host, o.dev, o.bytes(ny, nx), hipMemcpyDeviceToHost, c.compute));
        TOPO_TRY(finish());  // (one synchronisation, behind the counters' copy)
        return rc;
    }
    TOPO_TRY(copy_streams(2 * nchunks));
    hipEvent_t* up_done = c.pipe_events.data();
    hipEvent_t* computed = c.pipe_events.data() + nchunks;
    // Page-locked arrays (topo_amd_host_alloc, hipHostRegister): every copy is asynchronous, and the calling thread issues the
    // downloads itself, behind each chunk's kernels.  Pageable arrays: copies block their caller, so the downloads go to a
    // second thread (tools/ubench/pipe_paths.hip: 23.4 / 23.9 ms for 2 x 1 GiB against 38 - 39 ms one after the other).
    // TOPO_AMD_HOST_DOWNLOADS=thread / inline forces one or the other.
    const int forced_mode = [] {
        const char* e = std::getenv("TOPO_AMD_HOST_DOWNLOADS");
        return e && *e == 't' ? 1 : (e && *e == 'i' ? 2 : 0);
    }();
    auto page_locked = [](const void* p) {
        if (!p) return true;
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return attr.type == hipMemoryTypeHost;
    };
    bool all_locked = !upload || page_locked(src.data);
    for (const HostPlane& o : outs) all_locked = all_locked && page_locked(o.host);
    const bool inline_downloads = forced_mode == 2 || (forced_mode == 0 && all_locked);
    // rows [r0, r1) of every plane the caller wants, on the download stream behind the kernels of chunk j
    auto download_rows = [&](int j, int r0, int r1) {
        hipError_t e = hipStreamWaitEvent(c.down, computed[j], 0);
        for (size_t q = 0; q < outs.size() && e == hipSuccess; ++q)
            if (outs[q].host)
                e = hipMemcpyAsync(outs[q].host_row(r0, nx), outs[q].dev_row(r0, nx), (size_t)(r1 - r0) * nx * outs[q].elem,
                                   hipMemcpyDeviceToHost, c.down);
        return e;
    };
    std::mutex mu;
    std::condition_variable cv;
    int ready_chunks = 0;  // chunks whose kernels are enqueued and whose event is recorded
    bool failed = false;
    int down_rc = TOPO_AMD_OK;
    std::string down_error;
    const int device = c.device;
    if (inline_downloads) pages.ready();
    std::thread downloader([&] {
        if (inline_downloads) return;
        (void)hipSetDevice(device);
        pages.ready();  // the result arrays have their pages
        for (int j = 0; j < nchunks; ++j) {
            {
                std::unique_lock<std::mutex> lock(mu);
                cv.wait(lock, [&] { return ready_chunks > j || failed; });
                if (failed) return;
            }
            const hipError_t e = download_rows(j, cut[j], cut[j + 1]);
            if (e != hipSuccess) {
                down_rc = TOPO_AMD_EHIP;
                down_error = std::string("download of a row chunk failed: ") + hipGetErrorString(e);
                return;
            }
        }
        if (hipStreamSynchronize(c.down) != hipSuccess) {
            down_rc = TOPO_AMD_EHIP;
            down_error = "hipStreamSynchronize(download stream) failed";
        }
    });
    int rc = TOPO_AMD_OK, next = 0;
    bool empty = false;
    auto fail = [&](int code) {
        rc = code;
        std::lock_guard<std::mutex> lock(mu);
        failed = true;
    };
    for (int k = 0; k < nchunks && rc == TOPO_AMD_OK; ++k) {
        const int u0 = cut[k], u1 = cut[k + 1];
        if (upload) {
            hipError_t e = enqueue_rows(src, d_raw, d_in, u0, u1, nx, c.up);
            if (e == hipSuccess) e = hipEventRecord(up_done[k], c.up);
            if (e != hipSuccess) {
                set_error("upload of a row chunk failed: %s", hipGetErrorString(e));
                fail(TOPO_AMD_EHIP);
                break;
            }
        }
        const int uploaded = upload ? u1 : ny;
        while (next < nchunks && std::min(ny, cut[next + 1] + below) <= uploaded) {
            const int r0 = cut[next], r1 = cut[next + 1];
            if (upload && hipStreamWaitEvent(c.compute, up_done[k], 0) != hipSuccess) {
                set_error("hipStreamWaitEvent(compute, upload) failed");
                fail(TOPO_AMD_EHIP);
                break;
            }
            const int r = compute(uploaded, r0, r1 - r0);
            if (r != TOPO_AMD_OK && r != TOPO_AMD_EEMPTY) {
                fail(r);
                break;
            }
            if (r == TOPO_AMD_EEMPTY) empty = true;  // (Sx: every plane was written; reported at the end)
            if (const int e = encode_rows(r0, r1); e != TOPO_AMD_OK) {
                fail(e);
                break;
            }
            if (hipEventRecord(computed[next], c.compute) != hipSuccess) {
                set_error("hipEventRecord(computed chunk) failed");
                fail(TOPO_AMD_EHIP);
                break;
            }
            if (const hipError_t e = inline_downloads ? download_rows(next, r0, r1) : hipSuccess; e != hipSuccess) {
                set_error("download of a row chunk failed: %s", hipGetErrorString(e));
                fail(TOPO_AMD_EHIP);
                break;
            }
            {
                std::lock_guard<std::mutex> lock(mu);
                ready_chunks = ++next;
            }
            cv.notify_all();
        }
    }
    cv.notify_all();
    downloader.join();
    if (inline_downloads && hipStreamSynchronize(c.down) != hipSuccess && rc == TOPO_AMD_OK) {
        set_error("hipStreamSynchronize(download stream) failed");
        rc = TOPO_AMD_EHIP;
    }
    (void)hipStreamSynchronize(c.compute);
    if (upload) (void)hipStreamSynchronize(c.up);
    if (rc != TOPO_AMD_OK) return rc;
    if (down_rc != TOPO_AMD_OK) {
        set_error("%s", down_error.c_str());
        return down_rc;
    }
    if (any_packed) TOPO_TRY(finish());
    return empty ? TOPO_AMD_EEMPTY : TOPO_AMD_OK;
}

}  // namespace

void prefault_pages(void* host, size_t bytes) {
    PageToucher pages;
    pages.prefault(host, bytes);
}

}  // namespace topo

using namespace topo;

extern "C" {

int topo_amd_release_host_planes(void) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Context& c = ctx();
    TOPO_HIP(hipStreamSynchronize(c.compute));
    for (size_t k = 0; k < c.host_planes.size(); ++k) {
        if (c.host_planes[k]) {
            dem_memo_forget(c.host_planes[k], c.host_plane_bytes[k]);
            TOPO_HIP(hipFree(c.host_planes[k]));
        }
    }
    c.host_planes.clear();
    c.host_plane_bytes.clear();
    return TOPO_AMD_OK;
}

int topo_amd_host_chunks(int* chunks) {
    TOPO_REQUIRE(chunks != nullptr, "host_chunks: NULL output");
    *chunks = t_host_chunks;
    return TOPO_AMD_OK;
}

// ---- host-buffer entry points ----------------------------------------------------------------
int topo_amd_tpi_std_packed(const topo_amd_raster* raster, int ny, int nx, int size, double sigma, topo_amd_plane* tpi_plane,
                            topo_amd_plane* std_plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "tpi_std"));
    float *d_tpi, *d_std;
    TOPO_TRY(call.plane(tpi_plane, &d_tpi));
    TOPO_TRY(call.plane(std_plane, &d_std));
    TOPO_REQUIRE(d_tpi || d_std, "tpi_std: both outputs are NULL");
    ClassScope cls(scan_source(call.src, ny, nx));  // the raster class from the caller's array: no launch, no synchronisation
    int above = 0, below = 0;
    TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_TPI, (double)size, sigma, &above, &below));
    return call.run(below, kRowChunks, [&](const Block& view, int r0) {
        return tpi_std_block(view, size, sigma, call.at(d_tpi, r0), call.at(d_std, r0));
    });
}

// the same pipeline over the valid-sample kernel (disc_valid.hip): a declared nodata is NaN behind the decode, hence missing
int topo_amd_tpi_std_valid_packed(const topo_amd_raster* raster, int ny, int nx, int size, int min_count, topo_amd_plane* tpi_plane,
                                  topo_amd_plane* std_plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "tpi_std_valid"));
    TOPO_REQUIRE(size >= 1 && min_count >= 1, "tpi_std_valid: size %d, min_count %d (both at least 1)", size, min_count);
    float *d_tpi, *d_std;
    TOPO_TRY(call.plane(tpi_plane, &d_tpi));
    TOPO_TRY(call.plane(std_plane, &d_std));
    TOPO_REQUIRE(d_tpi || d_std, "tpi_std_valid: both outputs are NULL");
    if (size > kDiscValidMaxSize) {
        set_error("tpi_std_valid: disc size %d; the valid-sample kernel covers 1 ... %d", size, kDiscValidMaxSize);
        return TOPO_AMD_EUNSUP;
    }
    int above = 0, below = 0;
    TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_TPI, (double)size, 0.0, &above, &below));
    TOPO_TRY(disc_valid_begin());  // one flag word for the launches of every row chunk
    return call.run(below, kRowChunks, [&](const Block& view, int r0) {
        return tpi_std_valid_block(view, size, min_count, call.at(d_tpi, r0), call.at(d_std, r0));
    });
}

int topo_amd_tpi_std_valid_raw(const topo_amd_raster* raster, int ny, int nx, int size, int min_count, float* tpi_out,
                               float* std_out) {
    topo_amd_plane t = f32_plane(tpi_out), s = f32_plane(std_out);
    return topo_amd_tpi_std_valid_packed(raster, ny, nx, size, min_count, &t, &s);
}

int topo_amd_tpi_std_multi_packed(const topo_amd_raster* raster, int ny, int nx, int n_scales, const int32_t* sizes,
                                  const double* sigmas, topo_amd_plane* tpi_planes, topo_amd_plane* std_planes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "tpi_std_multi"));
    TOPO_REQUIRE(n_scales >= 1 && sizes, "tpi_std_multi: no scales");
    TOPO_REQUIRE(tpi_planes || std_planes, "tpi_std_multi: both output lists are NULL");
    std::vector<HostPlane> tpi_outs(n_scales), std_outs(n_scales);
    for (int k = 0; k < n_scales; ++k) {
        TOPO_TRY(make_plane(tpi_planes ? tpi_planes + k : nullptr, "tpi_std_multi", &tpi_outs[k]));
        TOPO_TRY(make_plane(std_planes ? std_planes + k : nullptr, "tpi_std_multi", &std_outs[k]));
    }
    for (int k = 0; k < n_scales; ++k) TOPO_REQUIRE(tpi_outs[k] || std_outs[k], "tpi_std_multi: scale %d has no output plane", k);
    ClassScope cls(scan_source(call.src, ny, nx));
    float *d_tpi, *d_std;  // one device plane of each kind, and (p_*) one packed device plane, for all the scales
    TOPO_TRY(call.shared(tpi_outs, &d_tpi));
    TOPO_TRY(call.shared(std_outs, &d_std));
    void *p_tpi = nullptr, *p_std = nullptr;
    // scale 0 rides on the upload; every scale overlaps its kernels with its own downloads (the two device planes are
    // reused, so a scale starts when the one before it is down)
    for (int k = 0; k < n_scales; ++k) {
        float* t = tpi_outs[k] ? d_tpi : nullptr;
        float* sd = std_outs[k] ? d_std : nullptr;
        const double sigma = sigmas ? sigmas[k] : 0.0;
        int above = 0, below = 0;
        TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_TPI, (double)sizes[k], sigma, &above, &below));
        call.outs.clear();
        call.add(tpi_outs[k], t, &p_tpi);
        call.add(std_outs[k], sd, &p_std);
        TOPO_TRY(call.run(below, kRowChunks, [&](const Block& view, int r0) {
            return tpi_std_block(view, sizes[k], sigma, call.at(t, r0), call.at(sd, r0));
        }));
    }
    return TOPO_AMD_OK;
}

int topo_amd_tpi_std_raw(const topo_amd_raster* raster, int ny, int nx, int size, double sigma, float* tpi_out, float* std_out) {
    topo_amd_plane t = f32_plane(tpi_out), s = f32_plane(std_out);
    return topo_amd_tpi_std_packed(raster, ny, nx, size, sigma, &t, &s);
}

int topo_amd_tpi_std_multi_raw(const topo_amd_raster* raster, int ny, int nx, int n_scales, const int32_t* sizes,
                               const double* sigmas, float* const* tpi_outs, float* const* std_outs) {
    std::vector<topo_amd_plane> t, s;  // (no scales: refused by the callee, behind its other checks)
    for (int k = 0; k < n_scales; ++k) {
        if (tpi_outs) t.push_back(f32_plane(tpi_outs[k]));
        if (std_outs) s.push_back(f32_plane(std_outs[k]));
    }
    return topo_amd_tpi_std_multi_packed(raster, ny, nx, n_scales, sizes, sigmas, tpi_outs ? t.data() : nullptr,
                                         std_outs ? s.data() : nullptr);
}

int topo_amd_tpi_raw(const topo_amd_raster* raster, int ny, int nx, int size, double sigma, float* out) {
    TOPO_ENTER();
    TOPO_REQUIRE(out != nullptr, "tpi: NULL output");
    return topo_amd_tpi_std_raw(raster, ny, nx, size, sigma, out, nullptr);
}

int topo_amd_std_raw(const topo_amd_raster* raster, int ny, int nx, int size, double sigma, float* out) {
    TOPO_ENTER();
    TOPO_REQUIRE(out != nullptr, "std: NULL output");
    return topo_amd_tpi_std_raw(raster, ny, nx, size, sigma, nullptr, out);
}

int topo_amd_gauss_raw(const topo_amd_raster* raster, int ny, int nx, double sigma_y, double sigma_x, float* out) {
    topo_amd_plane o = f32_plane(out);
    return topo_amd_gauss_packed(raster, ny, nx, sigma_y, sigma_x, &o);
}

int topo_amd_gauss_packed(const topo_amd_raster* raster, int ny, int nx, double sigma_y, double sigma_x, topo_amd_plane* plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "gauss", "bad arguments"));
    float* d_out;
    TOPO_TRY(call.plane(plane, &d_out));
    TOPO_REQUIRE(d_out, "gauss: bad arguments");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "gaussian: negative sigma");
    ClassScope cls(scan_source(call.src, ny, nx));
    int above = 0, below = 0;
    TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_GAUSS, sigma_y, 0.0, &above, &below));
    return call.run(below, kRowChunks, [&](const Block& v, int r0) {
        return topo_amd_gaussian_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, sigma_y, sigma_x, r0, v.out_rows, call.at(d_out, r0));
    });
}

// the valid-sample Gaussian (gauss_valid.hip) through the same pipeline: a declared nodata is NaN behind the decode, hence a
// gap; the weight plane is float32 whatever the packing of `plane`
int topo_amd_gauss_valid_packed(const topo_amd_raster* raster, int ny, int nx, double sigma_y, double sigma_x, double min_weight,
                                int fill, topo_amd_plane* plane, float* weight_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "gauss_valid", "bad arguments"));
    float *d_out, *d_weight;
    TOPO_TRY(call.plane(plane, &d_out));
    TOPO_TRY(call.stored(weight_out, &d_weight));
    TOPO_REQUIRE(d_out, "gauss_valid: bad arguments");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "gauss_valid: negative sigma");
    TOPO_REQUIRE(min_weight >= 0.0 && min_weight <= 1.0, "gauss_valid: min_weight %g outside [0, 1]", min_weight);
    const int below = (int)std::min(4.0 * sigma_y + 0.5, kGaussValidMaxRadius + 1.0);  // the radius: all the ghost rows it wants
    return call.run(below, kRowChunks, [&](const Block& v, int r0) {
        return topo_amd_gaussian_valid_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, sigma_y, sigma_x, min_weight, fill, r0, v.out_rows,
                                           call.at(d_out, r0), call.at(d_weight, r0));
    });
}

int topo_amd_gauss_valid_raw(const topo_amd_raster* raster, int ny, int nx, double sigma_y, double sigma_x, double min_weight,
                             int fill, float* out, float* weight_out) {
    topo_amd_plane o = f32_plane(out);
    return topo_amd_gauss_valid_packed(raster, ny, nx, sigma_y, sigma_x, min_weight, fill, &o, weight_out);
}

int topo_amd_sobel_raw(const topo_amd_raster* raster, int ny, int nx, float* dx_out, float* dy_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "sobel", "bad arguments"));
    TOPO_REQUIRE(dx_out && dy_out, "sobel: bad arguments");
    float *d_dx, *d_dy;
    TOPO_TRY(call.stored(dx_out, &d_dx));
    TOPO_TRY(call.stored(dy_out, &d_dy));
    return call.run(1, kRowChunks, [&](const Block& v, int r0) {
        return topo_amd_sobel_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, r0, v.out_rows, call.at(d_dx, r0), call.at(d_dy, r0));
    });
}

int topo_amd_fill_na_raw(const topo_amd_raster* raster, int ny, int nx, const double* x_coords, double min_elevation, float* out,
                         uint8_t* missing_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "fill_na", "bad arguments"));
    TOPO_REQUIRE(out, "fill_na: bad arguments");
    bool ascending = true;
    TOPO_TRY(check_fill_coords(x_coords, nx, &ascending));  // (before anything moves)
    uint8_t* d_miss;
    call.in_place(out, call.d_in);  // filled in place on the device
    TOPO_TRY(call.stored(missing_out, &d_miss));
    return call.run(0, kRowChunks, [&](const Block& v, int r0) {
        return topo_amd_fill_na_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, x_coords, min_elevation, r0, v.out_rows,
                                    call.at(call.d_in, r0), d_miss ? d_miss + (size_t)r0 * nx : nullptr);
    });
}

int topo_amd_gradient_raw(const topo_amd_raster* raster, int ny, int nx, double sigma, double sig_ratio,
                          int res_mode, const void* res_x, const void* res_y, float* dx_out,
                          float* dy_out, float* slope_out, float* aspect_out) {
    topo_amd_plane dx = f32_plane(dx_out), dy = f32_plane(dy_out), slope = f32_plane(slope_out), aspect = f32_plane(aspect_out);
    return topo_amd_gradient_packed(raster, ny, nx, sigma, sig_ratio, res_mode, res_x, res_y, &dx, &dy, &slope, &aspect);
}

int topo_amd_gradient_packed(const topo_amd_raster* raster, int ny, int nx, double sigma, double sig_ratio, int res_mode,
                             const void* res_x, const void* res_y, topo_amd_plane* dx_out, topo_amd_plane* dy_out,
                             topo_amd_plane* slope_out, topo_amd_plane* aspect_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "gradient"));
    topo_amd_plane* planes[4] = {dx_out, dy_out, slope_out, aspect_out};
    float* d_o[4];
    for (int k = 0; k < 4; ++k) TOPO_TRY(call.plane(planes[k], &d_o[k]));
    ClassScope cls(scan_source(call.src, ny, nx));
    const void *rx = res_x, *ry = res_y;
    if (res_mode == TOPO_AMD_RES_2D) {  // the call's extras: the two resolution planes on the device
        TOPO_REQUIRE(res_x && res_y, "gradient: resolution arrays are NULL");
        float *d_rx, *d_ry;
        TOPO_TRY(call.extra(&d_rx));
        TOPO_TRY(call.extra(&d_ry));
        TOPO_HIP(hipMemcpyAsync(d_rx, res_x, call.samples() * sizeof(float), hipMemcpyHostToDevice, ctx().compute));
        TOPO_HIP(hipMemcpyAsync(d_ry, res_y, call.samples() * sizeof(float), hipMemcpyHostToDevice, ctx().compute));
        rx = d_rx;
        ry = d_ry;
    }
    const int h = gradient_ghost_rows(sigma, sig_ratio, true);
    return call.run(h, kRowChunks, [&](const Block& v, int r0) {
        const void *cx = rx, *cy = ry;
        if (res_mode == TOPO_AMD_RES_2D) {  // [out_rows x nx], aligned with the output rows
            cx = (const float*)rx + (size_t)r0 * nx;
            cy = (const float*)ry + (size_t)r0 * nx;
        }
        return topo_amd_gradient_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, sigma, sig_ratio, res_mode, cx, cy, r0, v.out_rows,
                                     call.at(d_o[0], r0), call.at(d_o[1], r0), call.at(d_o[2], r0), call.at(d_o[3], r0));
    });
}

// the valid-sample gradient (gradient.hip, K4v) through the same pipeline: a declared nodata is NaN behind the decode, hence a gap
int topo_amd_gradient_valid_raw(const topo_amd_raster* raster, int ny, int nx, double sigma, double sig_ratio, double min_weight,
                                int fill, int res_mode, const void* res_x, const void* res_y, float* dx_out, float* dy_out,
                                float* slope_out, float* aspect_out) {
    topo_amd_plane dx = f32_plane(dx_out), dy = f32_plane(dy_out), slope = f32_plane(slope_out), aspect = f32_plane(aspect_out);
    return topo_amd_gradient_valid_packed(raster, ny, nx, sigma, sig_ratio, min_weight, fill, res_mode, res_x, res_y, &dx, &dy, &slope,
                                          &aspect);
}

int topo_amd_gradient_valid_packed(const topo_amd_raster* raster, int ny, int nx, double sigma, double sig_ratio, double min_weight,
                                   int fill, int res_mode, const void* res_x, const void* res_y, topo_amd_plane* dx_out,
                                   topo_amd_plane* dy_out, topo_amd_plane* slope_out, topo_amd_plane* aspect_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "gradient_valid"));
    TOPO_REQUIRE(sigma >= 0.0, "gradient_valid: negative sigma");
    TOPO_REQUIRE(sig_ratio > 0.0 && sig_ratio <= 1e6, "gradient_valid: sig_ratio %g (a positive factor)", sig_ratio);
    TOPO_REQUIRE(min_weight >= 0.0 && min_weight <= 1.0, "gradient_valid: min_weight %g outside [0, 1]", min_weight);
    topo_amd_plane* planes[4] = {dx_out, dy_out, slope_out, aspect_out};
    float* d_o[4];
    for (int k = 0; k < 4; ++k) TOPO_TRY(call.plane(planes[k], &d_o[k]));
    const void *rx = res_x, *ry = res_y;
    if (res_mode == TOPO_AMD_RES_2D) {  // the call's extras: the two resolution planes on the device
        TOPO_REQUIRE(res_x && res_y, "gradient_valid: resolution arrays are NULL");
        float *d_rx, *d_ry;
        TOPO_TRY(call.extra(&d_rx));
        TOPO_TRY(call.extra(&d_ry));
        TOPO_HIP(hipMemcpyAsync(d_rx, res_x, call.samples() * sizeof(float), hipMemcpyHostToDevice, ctx().compute));
        TOPO_HIP(hipMemcpyAsync(d_ry, res_y, call.samples() * sizeof(float), hipMemcpyHostToDevice, ctx().compute));
        rx = d_rx;
        ry = d_ry;
    }
    // the radius of the wider filter and the row of the difference: all the ghost rows the device call wants
    const double wide = sigma > 1.0 ? std::max(sigma, sigma * sig_ratio) : 0.0;
    const int below = (int)std::min(4.0 * wide + 0.5, kGaussValidMaxRadius + 1.0) + 1;
    return call.run(below, kRowChunks, [&](const Block& v, int r0) {
        const void *cx = rx, *cy = ry;
        if (res_mode == TOPO_AMD_RES_2D) {  // [out_rows x nx], aligned with the output rows
            cx = (const float*)rx + (size_t)r0 * nx;
            cy = (const float*)ry + (size_t)r0 * nx;
        }
        return topo_amd_gradient_valid_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, sigma, sig_ratio, min_weight, fill, res_mode, cx, cy,
                                           r0, v.out_rows, call.at(d_o[0], r0), call.at(d_o[1], r0), call.at(d_o[2], r0),
                                           call.at(d_o[3], r0));
    });
}

int topo_amd_sx_raw(const topo_amd_raster* raster, int ny, int nx, const int32_t* dj, const int32_t* di,
                    const double* dist, int n_off, int window, double height, float* out) {
    topo_amd_plane o = f32_plane(out);
    return topo_amd_sx_packed(raster, ny, nx, dj, di, dist, n_off, window, height, &o);
}

int topo_amd_sx_packed(const topo_amd_raster* raster, int ny, int nx, const int32_t* dj, const int32_t* di, const double* dist,
                       int n_off, int window, double height, topo_amd_plane* plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "sx", "bad arguments"));
    float* d_out;
    TOPO_TRY(call.plane(plane, &d_out));
    TOPO_REQUIRE(d_out, "sx: bad arguments");
    // (no ray pixel at all: the tables may be NULL; the plane is zero-filled and the call answers TOPO_AMD_EEMPTY, like
    // a sector whose pixels are all NaN)
    TOPO_REQUIRE(n_off >= 0 && (n_off == 0 || (dj && di && dist)), "sx: NULL argument");
    int up = 0, down = 0;
    sx_reach(dj, dist, 0, n_off, &up, &down);
    return call.run(down, kRowChunks, [&](const Block& v, int r0) {
        return topo_amd_sx_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, dj, di, dist, n_off, window, height, r0, v.out_rows,
                               call.at(d_out, r0));
    });
}

int topo_amd_sx_multi_raw(const topo_amd_raster* raster, int ny, int nx, int n_az, const int32_t* first,
                          const int32_t* dj, const int32_t* di, const double* dist, const int32_t* window,
                          double height, float* const* outs) {
    std::vector<topo_amd_plane> planes;  // (no planes: refused by the callee, behind its other checks)
    for (int k = 0; outs && k < n_az; ++k) planes.push_back(f32_plane(outs[k]));
    return topo_amd_sx_multi_packed(raster, ny, nx, n_az, first, dj, di, dist, window, height, outs && n_az >= 1 ? planes.data() : nullptr);
}

int topo_amd_sx_multi_packed(const topo_amd_raster* raster, int ny, int nx, int n_az, const int32_t* first, const int32_t* dj,
                             const int32_t* di, const double* dist, const int32_t* window, double height,
                             topo_amd_plane* out_planes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "sx_multi", "bad arguments"));
    TOPO_REQUIRE(out_planes && n_az >= 1, "sx_multi: bad arguments");
    TOPO_REQUIRE(first && dj && di && dist && window, "sx_multi: NULL argument");
    std::vector<float*> d_out(n_az, nullptr), moved(n_az);
    for (int k = 0; k < n_az; ++k) {
        TOPO_TRY(call.plane(out_planes + k, &d_out[k]));
        TOPO_REQUIRE(d_out[k], "sx_multi: NULL output plane %d", k);
    }
    int up = 0, down = 0;
    sx_reach(dj, dist, first[0], first[n_az], &up, &down);
    return call.run(down, kRowChunks, [&](const Block& v, int r0) {
        for (int k = 0; k < n_az; ++k) moved[k] = call.at(d_out[k], r0);
        return topo_amd_sx_multi_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, n_az, first, dj, di, dist, window, height, r0, v.out_rows,
                                     moved.data());  // (EEMPTY: every plane was written)
    });
}

int topo_amd_valley_ridge_raw(const topo_amd_raster* raster, int ny, int nx, const float* taps, const int32_t* ksize,
                              const float* angles, int n_angles, int n_planes, double mean, double stdev,
                              float* norm_out, float* dir_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "valley_ridge", "bad arguments"));
    TOPO_REQUIRE(norm_out && dir_out, "valley_ridge: bad arguments");
    float *d_norm, *d_dir;
    TOPO_TRY(call.stored(norm_out, &d_norm));
    TOPO_TRY(call.stored(dir_out, &d_dir));
    // (not pipelined: half a second of kernels per 20 ms of copies at full size, and the FFT route of the large kernels is
    // not cut-invariant)
    return call.run(0, kOneChunk, [&](const Block& v, int r0) {
        return topo_amd_valley_ridge_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, taps, ksize, angles, n_angles, n_planes, mean, stdev, r0,
                                         v.out_rows, call.at(d_norm, r0), call.at(d_dir, r0));
    });
}

// The standardised, optionally smoothed and optionally packed index of a host raster in one call: upload and decode, the
// Gaussian of topo_amd_gaussian_dev when sigma > 0, numpy's float32 moments of that field (moments_np.hip), the index, the
// planes encoded behind it.  One chunk, like topo_amd_valley_ridge_raw.
int topo_amd_valley_ridge_packed(const topo_amd_raster* raster, int ny, int nx, const float* taps, const int32_t* ksize,
                                 const float* angles, int n_angles, int n_planes, double sigma, size_t chunk,
                                 topo_amd_plane* norm_plane, topo_amd_plane* dir_plane, float moments_out[2]) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    HostCall call;
    TOPO_TRY(call.open(raster, ny, nx, "valley_ridge", "bad arguments"));
    float *d_norm, *d_dir, *d_smooth = nullptr;
    TOPO_TRY(call.plane(norm_plane, &d_norm));
    TOPO_TRY(call.plane(dir_plane, &d_dir));
    TOPO_REQUIRE(d_norm && d_dir, "valley_ridge: bad arguments");
    TOPO_REQUIRE(sigma >= 0.0, "valley_ridge: sigma %g", sigma);
    if (sigma > 0.0) TOPO_TRY(call.extra(&d_smooth));  // the call's extra: the smoothed plane
    return call.run(0, kOneChunk, [&](const Block& v, int) {  // (one chunk: the whole raster)
        const float* field = v.in;
        if (sigma > 0.0) {
            ClassScope cls(scan_source(call.src, ny, nx));  // the smoothing kernels topo_amd_gauss_raw takes for this raster
            TOPO_TRY(topo_amd_gaussian_dev(v.in, v.in_rows, v.in_row0, v.gny, v.nx, sigma, sigma, v.out_row0, v.out_rows, d_smooth));
            field = d_smooth;
        }
        return topo_amd_valley_ridge_std_dev(field, ny, nx, taps, ksize, angles, n_angles, n_planes, chunk, d_norm, d_dir, moments_out);
    });
}

int topo_amd_valley_ridge_std_raw(const topo_amd_raster* raster, int ny, int nx, const float* taps, const int32_t* ksize,
                                  const float* angles, int n_angles, int n_planes, double sigma, size_t chunk, float* norm_out,
                                  float* dir_out, float moments_out[2]) {
    topo_amd_plane n = f32_plane(norm_out), d = f32_plane(dir_out);
    return topo_amd_valley_ridge_packed(raster, ny, nx, taps, ksize, angles, n_angles, n_planes, sigma, chunk, &n, &d, moments_out);
}

// ---- the *_f32 entry points: the *_raw ones on float32 as stored -------------------------------------------------------------
int topo_amd_tpi_f32(const float* dem, int ny, int nx, int size, double sigma, float* out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_tpi_raw(&r, ny, nx, size, sigma, out);
}
int topo_amd_std_f32(const float* dem, int ny, int nx, int size, double sigma, float* out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_std_raw(&r, ny, nx, size, sigma, out);
}
int topo_amd_tpi_std_f32(const float* dem, int ny, int nx, int size, double sigma, float* tpi_out, float* std_out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_tpi_std_raw(&r, ny, nx, size, sigma, tpi_out, std_out);
}
int topo_amd_tpi_std_multi_f32(const float* dem, int ny, int nx, int n_scales, const int32_t* sizes, const double* sigmas,
                               float* const* tpi_outs, float* const* std_outs) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_tpi_std_multi_raw(&r, ny, nx, n_scales, sizes, sigmas, tpi_outs, std_outs);
}
int topo_amd_gauss_f32(const float* dem, int ny, int nx, double sigma_y, double sigma_x, float* out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_gauss_raw(&r, ny, nx, sigma_y, sigma_x, out);
}
int topo_amd_sobel_f32(const float* dem, int ny, int nx, float* dx_out, float* dy_out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_sobel_raw(&r, ny, nx, dx_out, dy_out);
}
int topo_amd_fill_na_f32(const float* dem, int ny, int nx, const double* x_coords, double min_elevation, float* out,
                         uint8_t* missing_out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_fill_na_raw(&r, ny, nx, x_coords, min_elevation, out, missing_out);
}
int topo_amd_gradient_f32(const float* dem, int ny, int nx, double sigma, double sig_ratio, int res_mode, const void* res_x,
                          const void* res_y, float* dx_out, float* dy_out, float* slope_out, float* aspect_out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_gradient_raw(&r, ny, nx, sigma, sig_ratio, res_mode, res_x, res_y, dx_out, dy_out, slope_out, aspect_out);
}
int topo_amd_sx_f32(const float* dem, int ny, int nx, const int32_t* dj, const int32_t* di, const double* dist, int n_off,
                    int window, double height, float* out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_sx_raw(&r, ny, nx, dj, di, dist, n_off, window, height, out);
}
int topo_amd_sx_multi_f32(const float* dem, int ny, int nx, int n_az, const int32_t* first, const int32_t* dj, const int32_t* di,
                          const double* dist, const int32_t* window, double height, float* const* outs) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_sx_multi_raw(&r, ny, nx, n_az, first, dj, di, dist, window, height, outs);
}
int topo_amd_valley_ridge_f32(const float* dem, int ny, int nx, const float* taps, const int32_t* ksize, const float* angles,
                              int n_angles, int n_planes, double mean, double stdev, float* norm_out, float* dir_out) {
    const topo_amd_raster r = f32_raster(dem);
    return topo_amd_valley_ridge_raw(&r, ny, nx, taps, ksize, angles, n_angles, n_planes, mean, stdev, norm_out, dir_out);
}

// ---- the decode on its own ---------------------------------------------------------------------------------------------------
int topo_amd_decode_host(const topo_amd_raster* raster, size_t count, float* out) {
    Source src;  // (no GPU, no context: nothing to lock)
    TOPO_TRY(make_source(raster, "decode_host", &src));
    TOPO_REQUIRE(out != nullptr || count == 0, "decode_host: NULL output");
    if (src.as_stored) {
        if (count) std::memcpy(out, src.data, count * sizeof(float));
        return TOPO_AMD_OK;
    }
    return decode_host_array(src.data, src.dtype, count, src.p, out);
}

int topo_amd_decode_dev(const void* raw_dev, int dtype, size_t count, double scale, double offset, int has_nodata, double nodata,
                        float* out_dev) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    const topo_amd_raster r{raw_dev, dtype, has_nodata, scale, offset, nodata};
    Source src;
    TOPO_TRY(make_source(&r, "decode_dev", &src));
    TOPO_REQUIRE(out_dev != nullptr, "decode_dev: NULL output");
    dem_memo_forget(out_dev, count * sizeof(float));
    if (count == 0) return TOPO_AMD_OK;
    if (src.as_stored) {
        if ((const void*)out_dev != raw_dev)
            TOPO_HIP(hipMemcpyAsync(out_dev, raw_dev, count * sizeof(float), hipMemcpyDeviceToDevice, ctx().compute));
        return TOPO_AMD_OK;
    }
    return launch_decode(ctx().compute, raw_dev, dtype, count, src.p, out_dev);
}

// ---- the encode on its own ---------------------------------------------------------------------------------------------------
int topo_amd_encode_host(const float* in, size_t count, topo_amd_plane* plane) {
    EncodeParams p;  // (no GPU, no context: nothing to lock)
    TOPO_TRY(make_encode(plane, "encode_host", &p));
    TOPO_REQUIRE((in != nullptr && plane->data != nullptr) || count == 0, "encode_host: NULL array");
    plane->missing = plane->saturated = 0;
    if (p.plain()) {
        if (count) std::memmove(plane->data, in, count * sizeof(float));
        return TOPO_AMD_OK;
    }
    return encode_host_array(in, count, p, plane->data, &plane->missing, &plane->saturated);
}

int topo_amd_encode_dev(const float* in_dev, size_t count, topo_amd_plane* plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    EncodeParams p;
    TOPO_TRY(make_encode(plane, "encode_dev", &p));
    TOPO_REQUIRE((in_dev != nullptr && plane->data != nullptr) || count == 0, "encode_dev: NULL array");
    plane->missing = plane->saturated = 0;
    if (count == 0) return TOPO_AMD_OK;
    Context& c = ctx();
    dem_memo_forget(plane->data, count * plane_sample_bytes(p.dtype));
    if (p.plain()) {
        if ((const void*)in_dev != plane->data)
            TOPO_HIP(hipMemcpyAsync(plane->data, in_dev, count * sizeof(float), hipMemcpyDeviceToDevice, c.compute));
        TOPO_HIP(hipStreamSynchronize(c.compute));
        return TOPO_AMD_OK;
    }
    EncodeCounts counts;
    TOPO_TRY(counts.reserve(1));
    TOPO_TRY(launch_encode(c.compute, in_dev, count, p, plane->data, counts.pair(0)));
    TOPO_TRY(counts.fetch());
    TOPO_HIP(hipStreamSynchronize(c.compute));
    counts.store(0, plane);
    return TOPO_AMD_OK;
}

int topo_amd_finish_dev(const float* in_dev, int ny, int nx, const uint8_t* mask_dev, int row0, int rows, int col0, int cols,
                        topo_amd_plane* plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    EncodeParams p;
    TOPO_TRY(make_encode(plane, "finish_dev", &p));
    TOPO_REQUIRE(ny >= 0 && nx >= 0 && row0 >= 0 && rows >= 0 && col0 >= 0 && cols >= 0 && (long long)row0 + rows <= ny &&
                     (long long)col0 + cols <= nx,
                 "finish_dev: window rows [%d, %d + %d) x columns [%d, %d + %d) of a %d x %d plane", row0, row0, rows, col0, col0, cols, ny, nx);
    TOPO_REQUIRE((uintptr_t)plane->data % plane_sample_bytes(p.dtype) == 0, "finish_dev: plane->data is not aligned to its sample type");
    plane->missing = plane->saturated = 0;
    if (rows == 0 || cols == 0) return TOPO_AMD_OK;
    TOPO_REQUIRE(in_dev != nullptr && plane->data != nullptr, "finish_dev: NULL array");
    Context& c = ctx();
    dem_memo_forget(plane->data, (size_t)rows * cols * plane_sample_bytes(p.dtype));
    EncodeCounts counts;
    TOPO_TRY(counts.reserve(1));
    TOPO_TRY(launch_finish(c.compute, in_dev, nx, mask_dev, row0, rows, col0, cols, p, plane->data, counts.pair(0)));
    TOPO_TRY(counts.fetch());
    TOPO_HIP(hipStreamSynchronize(c.compute));
    counts.store(0, plane);
    return TOPO_AMD_OK;
}

int topo_amd_upload_raw(const topo_amd_raster* raster, int ny, int nx, float* out_dev) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Source src;
    TOPO_TRY(make_source(raster, "upload_raw", &src));
    TOPO_REQUIRE(out_dev && ny >= 1 && nx >= 1, "upload_raw: bad arguments");
    Context& c = ctx();
    dem_memo_forget(out_dev, (size_t)ny * nx * sizeof(float));
    PlanePool pool;
    char* d_raw = nullptr;
    TOPO_TRY(raw_plane(pool, src, ny, nx, &d_raw));
    // the copies on the upload stream, each chunk's decode on the compute stream behind its copy: chunk k is decoded while
    // chunk k + 1 crosses the link (float32 as stored: nothing to decode, one copy)
    const std::vector<int> cut = row_cuts(ny, nx, src.as_stored);
    const int nchunks = (int)cut.size() - 1;
    if (nchunks == 1) {
        TOPO_HIP(enqueue_rows(src, d_raw, out_dev, 0, ny, nx, c.compute));
        TOPO_HIP(hipStreamSynchronize(c.compute));
        return TOPO_AMD_OK;
    }
    TOPO_TRY(copy_streams(nchunks));
    TOPO_HIP(hipStreamSynchronize(c.compute));  // (whatever still reads or writes the plane is over before the copies start)
    int rc = TOPO_AMD_OK;
    for (int k = 0; k < nchunks && rc == TOPO_AMD_OK; ++k) {
        const size_t at = (size_t)cut[k] * nx, count = (size_t)(cut[k + 1] - cut[k]) * nx;
        hipError_t e = hipMemcpyAsync(d_raw + at * src.elem, src.row(cut[k], nx), count * src.elem, hipMemcpyHostToDevice, c.up);
        if (e == hipSuccess) e = hipEventRecord(c.pipe_events[k], c.up);
        if (e == hipSuccess) e = hipStreamWaitEvent(c.compute, c.pipe_events[k], 0);
        if (e != hipSuccess) {
            set_error("upload of a row chunk failed: %s", hipGetErrorString(e));
            rc = TOPO_AMD_EHIP;
            break;
        }
        rc = launch_decode(c.compute, d_raw + at * src.elem, src.dtype, count, src.p, out_dev + at);
    }
    (void)hipStreamSynchronize(c.up);
    (void)hipStreamSynchronize(c.compute);
    return rc;
}

}  // extern "C"
