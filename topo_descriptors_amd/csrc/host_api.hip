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
// Device buffers of one host-buffer call, and the preparation of its result arrays.  A result array
// fresh from the allocator has no pages yet; faulting them in one by one under the download is what a
// host-buffer call spends most of its time on (tools/ubench/page_touch.cpp: 92 ms per GiB against 19 ms
// for the copy itself).  prefault() asks for huge pages and touches the array from a few threads
// while the upload and the kernels run; ready() joins them before the first download.
struct HostRun {
    std::vector<void*> bufs;
    std::vector<std::thread> touchers;
    explicit HostRun(bool entry_point = true) {
        if (entry_point) t_host_chunks = 0;
    }
    ~HostRun() {
        ready();
        for (size_t k = 0; k < bufs.size(); ++k) dem_memo_forget(bufs[k], sizes[k]);  // (the planes stay; what was known about their content goes)
    }
    std::vector<size_t> sizes;
    // the k-th plane this call asks for is the k-th plane of the context's pool (Context::host_planes), grown when it must be
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
struct HostPlane {
    void* host;
    void* dev;
    size_t elem = sizeof(float);  // bytes per sample (the missing mask of topo_amd_fill_na_f32: 1; a packed plane: 1 or 2)
    // A packed result plane (include/topo_amd.h): the kernels write the float32 device plane `f32`, its rows are encoded
    // behind them into the packed device plane `dev` - taken from the pool by run_pipelined, behind every plane a float32
    // call takes - and `dev` is what gets downloaded.  f32 == nullptr: a plane downloaded as the kernels write it.
    const float* f32 = nullptr;
    EncodeParams enc;
    topo_amd_plane* report = nullptr;  // the caller's struct: its counters are written after the last chunk
    void** pool = nullptr;             // a multi-scale call: where the packed device plane (2 bytes a sample) is kept between its scales
    bool packed() const { return host != nullptr && f32 != nullptr; }
    void* host_row(int r, int nx) const { return (char*)host + (size_t)r * nx * elem; }
    const void* dev_row(int r, int nx) const { return (const char*)dev + (size_t)r * nx * elem; }
};
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
// The cuts of a pipelined call: chunks of `chunk` rows, the last one half a chunk to a chunk and a half (no sliver at the end).
// (Round 6 tried a taper - a quarter and a half chunk at both ends, so that less stands in front of the first kernels and
// behind the last ones: 16384^2 TPI 67 px 26.05 -> 25.93 ms page-locked, 24.97 -> 24.80 pageable, profiles/r06_host_pipeline.txt:
// the fill and the drain are not what separates the call from the 22.4 ms of 1 GiB each way at 48 GB/s.  Not kept.)
std::vector<int> pipeline_cuts(int ny, int chunk) {
    std::vector<int> cut{0};
    int at = 0;
    while (ny - at > chunk + chunk / 2) cut.push_back(at += chunk);
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
int raw_plane(HostRun& run, const Source& s, int ny, int nx, char** d_raw) {
    *d_raw = nullptr;
    if (s.as_stored) return TOPO_AMD_OK;
    void* p = nullptr;
    TOPO_TRY(run.alloc(&p, (size_t)ny * nx * s.elem));
    *d_raw = (char*)p;
    return TOPO_AMD_OK;
}

// A caller's result plane as a host-buffer call sees it: a checked topo_amd_plane (absent: a NULL struct or NULL data, where
// the call allows it).  Float32 planes are downloaded as the kernels write them, the others encoded first (HostPlane).
struct OutPlane {
    void* host = nullptr;
    EncodeParams enc;
    topo_amd_plane* report = nullptr;
    explicit operator bool() const { return host != nullptr; }
    size_t bytes(int ny, int nx) const { return (size_t)ny * nx * plane_sample_bytes(enc.dtype); }
    // ... on the float32 device plane the kernels write; pool: see HostPlane
    HostPlane on(float* dev, void** pool = nullptr) const {
        HostPlane h{dev ? host : nullptr, dev};
        if (h.host && !enc.plain()) {
            h.dev = nullptr;
            h.elem = plane_sample_bytes(enc.dtype);
            h.f32 = dev;
            h.enc = enc;
            h.report = report;
            h.pool = pool;
        }
        return h;
    }
};
int make_out(topo_amd_plane* plane, const char* who, OutPlane* o) {
    *o = OutPlane();
    if (!plane || !plane->data) return TOPO_AMD_OK;
    TOPO_TRY(make_encode(plane, who, &o->enc));
    plane->missing = plane->saturated = 0;
    o->host = plane->data;
    o->report = plane;
    return TOPO_AMD_OK;
}
topo_amd_plane f32_plane(float* p) { return topo_amd_plane{p, TOPO_AMD_F32, 0, 1.0, 0.0, 0.0, 0, 0}; }

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

// compute(view_rows, out_row0, out_rows): enqueue the kernels that write output rows [out_row0, out_row0 + out_rows) of
// every plane, reading rows [0, view_rows) of d_in.  below: rows of the DEM beneath an output row that it depends on.
// upload == false: the DEM is on the device already (later scales of a multi-scale call).
// src: the caller's raster (ignored when upload == false).  A source that is not float32-as-stored goes chunk by chunk into
// a raw device plane and is decoded into d_in on the stream of the copy, in front of the event the kernels wait for.
// one_chunk: the call is not cut, whatever TOPO_AMD_HOST_* say.
constexpr bool kRowChunks = false, kOneChunk = true;
template <class Compute>
int run_pipelined(HostRun& run, const Source& src, float* d_in, int ny, int nx, int below, bool upload, bool one_chunk,
                  std::vector<HostPlane> outs, Compute&& compute) {
    Context& c = ctx();
    char* d_raw = nullptr;
    if (upload) TOPO_TRY(raw_plane(run, src, ny, nx, &d_raw));
    // packed result planes: their device planes (behind every plane a float32 call takes), one pair of counters each
    EncodeCounts counts;
    for (HostPlane& o : outs) {
        if (!o.packed()) continue;
        if (o.pool && *o.pool) {
            o.dev = *o.pool;
        } else {
            TOPO_TRY(run.alloc(&o.dev, (size_t)ny * nx * (o.pool ? 2 : o.elem)));
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
    const int chunk = one_chunk ? ny : pipeline_chunk_rows(ny, nx);
    const std::vector<int> cut = chunk >= ny ? std::vector<int>{0, ny} : pipeline_cuts(ny, chunk);
    const int nchunks = (int)cut.size() - 1;
    t_host_chunks = std::max(t_host_chunks, nchunks < 3 ? 1 : nchunks);  // (a multi-scale call: the most any of its scales ran in)
    if (nchunks < 3) {
        if (upload) TOPO_HIP(enqueue_rows(src, d_raw, d_in, 0, ny, nx, c.compute));
        const int rc = compute(ny, 0, ny);
        if (rc != TOPO_AMD_OK && rc != TOPO_AMD_EEMPTY) return rc;
        TOPO_TRY(encode_rows(0, ny));
        run.ready();
        for (const HostPlane& o : outs)
            if (o.host) TOPO_HIP(hipMemcpyAsync(o.host, o.dev, (size_t)ny * nx * o.elem, hipMemcpyDeviceToHost, c.compute));
        if (!one_chunk) TOPO_HIP(hipStreamSynchronize(c.compute));  // (the valley calls synchronise once, behind the counters' copy)
        TOPO_TRY(finish());
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
    if (inline_downloads) run.ready();
    std::thread downloader([&] {
        if (inline_downloads) return;
        (void)hipSetDevice(device);
        run.ready();  // the result arrays have their pages
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
    HostRun pages(false);
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
    Source src;
    TOPO_TRY(make_source(raster, "tpi_std", &src));
    TOPO_REQUIRE(ny >= 1 && nx >= 1, "tpi_std: bad DEM");
    OutPlane tpi_out, std_out;
    TOPO_TRY(make_out(tpi_plane, "tpi_std", &tpi_out));
    TOPO_TRY(make_out(std_plane, "tpi_std", &std_out));
    TOPO_REQUIRE(tpi_out || std_out, "tpi_std: both outputs are NULL");
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    ClassScope cls(scan_source(src, ny, nx));  // the raster class from the caller's array: no launch, no synchronisation
    int above = 0, below = 0;
    TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_TPI, (double)size, sigma, &above, &below));
    HostRun run;
    void *d_in = nullptr, *d_tpi = nullptr, *d_std = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    if (tpi_out) TOPO_TRY(run.alloc(&d_tpi, bytes));
    if (std_out) TOPO_TRY(run.alloc(&d_std, bytes));
    run.prefault(tpi_out.host, tpi_out.bytes(ny, nx));
    run.prefault(std_out.host, std_out.bytes(ny, nx));
    return run_pipelined(run, src, (float*)d_in, ny, nx, below, true, kRowChunks, {tpi_out.on((float*)d_tpi), std_out.on((float*)d_std)},
                         [&](int view_rows, int r0, int rows) {
                             Block b{(const float*)d_in, view_rows, 0, ny, nx, r0, rows};
                             return tpi_std_block(b, size, sigma, shift((float*)d_tpi, r0, nx), shift((float*)d_std, r0, nx));
                         });
}

// the same pipeline over the valid-sample kernel (disc_valid.hip): a declared nodata is NaN behind the decode, hence missing
int topo_amd_tpi_std_valid_packed(const topo_amd_raster* raster, int ny, int nx, int size, int min_count, topo_amd_plane* tpi_plane,
                                  topo_amd_plane* std_plane) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Source src;
    TOPO_TRY(make_source(raster, "tpi_std_valid", &src));
    TOPO_REQUIRE(ny >= 1 && nx >= 1, "tpi_std_valid: bad DEM");
    TOPO_REQUIRE(size >= 1 && min_count >= 1, "tpi_std_valid: size %d, min_count %d (both at least 1)", size, min_count);
    OutPlane tpi_out, std_out;
    TOPO_TRY(make_out(tpi_plane, "tpi_std_valid", &tpi_out));
    TOPO_TRY(make_out(std_plane, "tpi_std_valid", &std_out));
    TOPO_REQUIRE(tpi_out || std_out, "tpi_std_valid: both outputs are NULL");
    if (size > kDiscValidMaxSize) {
        set_error("tpi_std_valid: disc size %d; the valid-sample kernel covers 1 ... %d", size, kDiscValidMaxSize);
        return TOPO_AMD_EUNSUP;
    }
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    int above = 0, below = 0;
    TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_TPI, (double)size, 0.0, &above, &below));
    HostRun run;
    void *d_in = nullptr, *d_tpi = nullptr, *d_std = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    if (tpi_out) TOPO_TRY(run.alloc(&d_tpi, bytes));
    if (std_out) TOPO_TRY(run.alloc(&d_std, bytes));
    run.prefault(tpi_out.host, tpi_out.bytes(ny, nx));
    run.prefault(std_out.host, std_out.bytes(ny, nx));
    TOPO_TRY(disc_valid_begin());  // one flag word for the launches of every row chunk
    return run_pipelined(run, src, (float*)d_in, ny, nx, below, true, kRowChunks, {tpi_out.on((float*)d_tpi), std_out.on((float*)d_std)},
                         [&](int view_rows, int r0, int rows) {
                             Block b{(const float*)d_in, view_rows, 0, ny, nx, r0, rows};
                             return tpi_std_valid_block(b, size, min_count, shift((float*)d_tpi, r0, nx), shift((float*)d_std, r0, nx));
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
    Source src;
    TOPO_TRY(make_source(raster, "tpi_std_multi", &src));
    TOPO_REQUIRE(ny >= 1 && nx >= 1, "tpi_std_multi: bad DEM");
    TOPO_REQUIRE(n_scales >= 1 && sizes, "tpi_std_multi: no scales");
    TOPO_REQUIRE(tpi_planes || std_planes, "tpi_std_multi: both output lists are NULL");
    std::vector<OutPlane> tpi_outs(n_scales), std_outs(n_scales);
    for (int k = 0; k < n_scales; ++k) {
        TOPO_TRY(make_out(tpi_planes ? tpi_planes + k : nullptr, "tpi_std_multi", &tpi_outs[k]));
        TOPO_TRY(make_out(std_planes ? std_planes + k : nullptr, "tpi_std_multi", &std_outs[k]));
    }
    bool any_tpi = false, any_std = false;
    for (int k = 0; k < n_scales; ++k) {
        const bool t = (bool)tpi_outs[k], s = (bool)std_outs[k];
        TOPO_REQUIRE(t || s, "tpi_std_multi: scale %d has no output plane", k);
        any_tpi |= t;
        any_std |= s;
    }
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    ClassScope cls(scan_source(src, ny, nx));
    HostRun run;
    void *d_in = nullptr, *d_tpi = nullptr, *d_std = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    if (any_tpi) TOPO_TRY(run.alloc(&d_tpi, bytes));
    if (any_std) TOPO_TRY(run.alloc(&d_std, bytes));
    for (int k = 0; k < n_scales; ++k) {
        run.prefault(tpi_outs[k].host, tpi_outs[k].bytes(ny, nx));
        run.prefault(std_outs[k].host, std_outs[k].bytes(ny, nx));
    }
    void *p_tpi = nullptr, *p_std = nullptr;  // the packed device planes, one of each kind for all the scales
    // scale 0 rides on the upload; every scale overlaps its kernels with its own downloads (the two device planes are
    // reused, so a scale starts when the one before it is down)
    for (int k = 0; k < n_scales; ++k) {
        float* t = tpi_outs[k] ? (float*)d_tpi : nullptr;
        float* sd = std_outs[k] ? (float*)d_std : nullptr;
        int above = 0, below = 0;
        TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_TPI, (double)sizes[k], sigmas ? sigmas[k] : 0.0, &above, &below));
        TOPO_TRY(run_pipelined(run, src, (float*)d_in, ny, nx, below, k == 0, kRowChunks,
                               {tpi_outs[k].on(t, &p_tpi), std_outs[k].on(sd, &p_std)}, [&](int view_rows, int r0, int rows) {
                                   Block b{(const float*)d_in, view_rows, 0, ny, nx, r0, rows};
                                   return tpi_std_block(b, sizes[k], sigmas ? sigmas[k] : 0.0, shift(t, r0, nx), shift(sd, r0, nx));
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
    Source src;
    TOPO_TRY(make_source(raster, "gauss", &src));
    OutPlane out;
    TOPO_TRY(make_out(plane, "gauss", &out));
    TOPO_REQUIRE(out && ny >= 1 && nx >= 1, "gauss: bad arguments");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "gaussian: negative sigma");
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    ClassScope cls(scan_source(src, ny, nx));
    int above = 0, below = 0;
    TOPO_TRY(topo_amd_halo_rows(TOPO_AMD_DESC_GAUSS, sigma_y, 0.0, &above, &below));
    HostRun run;
    void *d_in = nullptr, *d_out = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    TOPO_TRY(run.alloc(&d_out, bytes));
    run.prefault(out.host, out.bytes(ny, nx));
    return run_pipelined(run, src, (float*)d_in, ny, nx, below, true, kRowChunks, {out.on((float*)d_out)},
                         [&](int view_rows, int r0, int rows) {
                             return topo_amd_gaussian_dev((const float*)d_in, view_rows, 0, ny, nx, sigma_y, sigma_x, r0, rows,
                                                          shift((float*)d_out, r0, nx));
                         });
}

// the valid-sample Gaussian (gauss_valid.hip) through the same pipeline: a declared nodata is NaN behind the decode, hence a
// gap; the weight plane is float32 whatever the packing of `plane`
int topo_amd_gauss_valid_packed(const topo_amd_raster* raster, int ny, int nx, double sigma_y, double sigma_x, double min_weight,
                                int fill, topo_amd_plane* plane, float* weight_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Source src;
    TOPO_TRY(make_source(raster, "gauss_valid", &src));
    OutPlane out, weight;
    TOPO_TRY(make_out(plane, "gauss_valid", &out));
    topo_amd_plane w = f32_plane(weight_out);
    TOPO_TRY(make_out(&w, "gauss_valid", &weight));
    TOPO_REQUIRE(out && ny >= 1 && nx >= 1, "gauss_valid: bad arguments");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "gauss_valid: negative sigma");
    TOPO_REQUIRE(min_weight >= 0.0 && min_weight <= 1.0, "gauss_valid: min_weight %g outside [0, 1]", min_weight);
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    const int below = (int)std::min(4.0 * sigma_y + 0.5, kGaussValidMaxRadius + 1.0);  // the radius: all the ghost rows it wants
    HostRun run;
    void *d_in = nullptr, *d_out = nullptr, *d_weight = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    TOPO_TRY(run.alloc(&d_out, bytes));
    if (weight) TOPO_TRY(run.alloc(&d_weight, bytes));
    run.prefault(out.host, out.bytes(ny, nx));
    run.prefault(weight.host, weight.bytes(ny, nx));
    return run_pipelined(run, src, (float*)d_in, ny, nx, below, true, kRowChunks, {out.on((float*)d_out), weight.on((float*)d_weight)},
                         [&](int view_rows, int r0, int rows) {
                             return topo_amd_gaussian_valid_dev((const float*)d_in, view_rows, 0, ny, nx, sigma_y, sigma_x, min_weight,
                                                                fill, r0, rows, shift((float*)d_out, r0, nx),
                                                                shift((float*)d_weight, r0, nx));
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
    Source src;
    TOPO_TRY(make_source(raster, "sobel", &src));
    TOPO_REQUIRE(dx_out && dy_out && ny >= 1 && nx >= 1, "sobel: bad arguments");
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    HostRun run;
    void *d_in = nullptr, *d_dx = nullptr, *d_dy = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    TOPO_TRY(run.alloc(&d_dx, bytes));
    TOPO_TRY(run.alloc(&d_dy, bytes));
    run.prefault(dx_out, bytes);
    run.prefault(dy_out, bytes);
    return run_pipelined(run, src, (float*)d_in, ny, nx, 1, true, kRowChunks, {{dx_out, (float*)d_dx}, {dy_out, (float*)d_dy}},
                         [&](int view_rows, int r0, int rows) {
                             return topo_amd_sobel_dev((const float*)d_in, view_rows, 0, ny, nx, r0, rows, shift((float*)d_dx, r0, nx),
                                                       shift((float*)d_dy, r0, nx));
                         });
}

int topo_amd_fill_na_raw(const topo_amd_raster* raster, int ny, int nx, const double* x_coords, double min_elevation, float* out,
                         uint8_t* missing_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Source src;
    TOPO_TRY(make_source(raster, "fill_na", &src));
    TOPO_REQUIRE(out && ny >= 1 && nx >= 1, "fill_na: bad arguments");
    bool ascending = true;
    TOPO_TRY(check_fill_coords(x_coords, nx, &ascending));  // (before anything moves)
    const size_t bytes = (size_t)ny * nx * sizeof(float), mask_bytes = (size_t)ny * nx;
    HostRun run;
    void *d_plane = nullptr, *d_miss = nullptr;
    TOPO_TRY(run.alloc(&d_plane, bytes));  // filled in place on the device
    if (missing_out) TOPO_TRY(run.alloc(&d_miss, mask_bytes));
    run.prefault(out, bytes);
    run.prefault(missing_out, mask_bytes);
    return run_pipelined(run, src, (float*)d_plane, ny, nx, 0, true, kRowChunks, {{out, d_plane}, {missing_out, d_miss, 1}},
                         [&](int view_rows, int r0, int rows) {
                             return topo_amd_fill_na_dev((const float*)d_plane, view_rows, 0, ny, nx, x_coords, min_elevation, r0, rows,
                                                         shift((float*)d_plane, r0, nx),
                                                         d_miss ? (uint8_t*)d_miss + (size_t)r0 * nx : nullptr);
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
    Source src;
    TOPO_TRY(make_source(raster, "gradient", &src));
    TOPO_REQUIRE(ny >= 1 && nx >= 1, "gradient: bad DEM");
    topo_amd_plane* planes[4] = {dx_out, dy_out, slope_out, aspect_out};
    OutPlane host_out[4];
    for (int k = 0; k < 4; ++k) TOPO_TRY(make_out(planes[k], "gradient", &host_out[k]));
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    ClassScope cls(scan_source(src, ny, nx));
    HostRun run;
    void *d_in = nullptr, *d_o[4] = {nullptr, nullptr, nullptr, nullptr};
    TOPO_TRY(run.alloc(&d_in, bytes));
    for (int k = 0; k < 4; ++k)
        if (host_out[k]) TOPO_TRY(run.alloc(&d_o[k], bytes));
    for (int k = 0; k < 4; ++k) run.prefault(host_out[k].host, host_out[k].bytes(ny, nx));
    const void *rx = res_x, *ry = res_y;
    if (res_mode == TOPO_AMD_RES_2D) {
        TOPO_REQUIRE(res_x && res_y, "gradient: resolution arrays are NULL");
        void *d_rx = nullptr, *d_ry = nullptr;
        TOPO_TRY(run.alloc(&d_rx, bytes));
        TOPO_TRY(run.alloc(&d_ry, bytes));
        TOPO_HIP(hipMemcpyAsync(d_rx, res_x, bytes, hipMemcpyHostToDevice, ctx().compute));
        TOPO_HIP(hipMemcpyAsync(d_ry, res_y, bytes, hipMemcpyHostToDevice, ctx().compute));
        rx = d_rx;
        ry = d_ry;
    }
    const int h = gradient_ghost_rows(sigma, sig_ratio, true);
    std::vector<HostPlane> outs;
    for (int k = 0; k < 4; ++k) outs.push_back(host_out[k].on((float*)d_o[k]));
    return run_pipelined(run, src, (float*)d_in, ny, nx, h, true, kRowChunks, outs, [&](int view_rows, int r0, int rows) {
        const void *cx = rx, *cy = ry;
        if (res_mode == TOPO_AMD_RES_2D) {  // [out_rows x nx], aligned with the output rows
            cx = (const float*)rx + (size_t)r0 * nx;
            cy = (const float*)ry + (size_t)r0 * nx;
        }
        return topo_amd_gradient_dev((const float*)d_in, view_rows, 0, ny, nx, sigma, sig_ratio, res_mode, cx, cy, r0, rows,
                                     shift((float*)d_o[0], r0, nx), shift((float*)d_o[1], r0, nx), shift((float*)d_o[2], r0, nx),
                                     shift((float*)d_o[3], r0, nx));
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
    Source src;
    TOPO_TRY(make_source(raster, "sx", &src));
    OutPlane out;
    TOPO_TRY(make_out(plane, "sx", &out));
    TOPO_REQUIRE(out && ny >= 1 && nx >= 1, "sx: bad arguments");
    // (no ray pixel at all: the tables may be NULL; the plane is zero-filled and the call answers TOPO_AMD_EEMPTY, like
    // a sector whose pixels are all NaN)
    TOPO_REQUIRE(n_off >= 0 && (n_off == 0 || (dj && di && dist)), "sx: NULL argument");
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    int up = 0, down = 0;
    sx_reach(dj, dist, 0, n_off, &up, &down);
    HostRun run;
    void *d_in = nullptr, *d_out = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    TOPO_TRY(run.alloc(&d_out, bytes));
    run.prefault(out.host, out.bytes(ny, nx));
    return run_pipelined(run, src, (float*)d_in, ny, nx, down, true, kRowChunks, {out.on((float*)d_out)},
                         [&](int view_rows, int r0, int rows) {
                             return topo_amd_sx_dev((const float*)d_in, view_rows, 0, ny, nx, dj, di, dist, n_off, window, height, r0, rows,
                                                    shift((float*)d_out, r0, nx));
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
    Source src;
    TOPO_TRY(make_source(raster, "sx_multi", &src));
    TOPO_REQUIRE(out_planes && n_az >= 1 && ny >= 1 && nx >= 1, "sx_multi: bad arguments");
    TOPO_REQUIRE(first && dj && di && dist && window, "sx_multi: NULL argument");
    std::vector<OutPlane> outs(n_az);
    for (int k = 0; k < n_az; ++k) {
        TOPO_TRY(make_out(out_planes + k, "sx_multi", &outs[k]));
        TOPO_REQUIRE(outs[k], "sx_multi: NULL output plane %d", k);
    }
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    HostRun run;
    void* d_in = nullptr;
    std::vector<float*> d_out(n_az, nullptr);
    TOPO_TRY(run.alloc(&d_in, bytes));
    for (int k = 0; k < n_az; ++k) TOPO_TRY(run.alloc((void**)&d_out[k], bytes));
    for (int k = 0; k < n_az; ++k) run.prefault(outs[k].host, outs[k].bytes(ny, nx));
    int up = 0, down = 0;
    sx_reach(dj, dist, first[0], first[n_az], &up, &down);
    std::vector<HostPlane> planes;
    for (int k = 0; k < n_az; ++k) planes.push_back(outs[k].on(d_out[k]));
    std::vector<float*> moved(n_az);
    return run_pipelined(run, src, (float*)d_in, ny, nx, down, true, kRowChunks, planes, [&](int view_rows, int r0, int rows) {
        for (int k = 0; k < n_az; ++k) moved[k] = shift(d_out[k], r0, nx);
        return topo_amd_sx_multi_dev((const float*)d_in, view_rows, 0, ny, nx, n_az, first, dj, di, dist, window, height, r0, rows,
                                     moved.data());  // (EEMPTY: every plane was written)
    });
}

int topo_amd_valley_ridge_raw(const topo_amd_raster* raster, int ny, int nx, const float* taps, const int32_t* ksize,
                              const float* angles, int n_angles, int n_planes, double mean, double stdev,
                              float* norm_out, float* dir_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Source src;
    TOPO_TRY(make_source(raster, "valley_ridge", &src));
    TOPO_REQUIRE(ny >= 1 && nx >= 1 && norm_out && dir_out, "valley_ridge: bad arguments");
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    HostRun run;
    void *d_in = nullptr, *d_norm = nullptr, *d_dir = nullptr;
    TOPO_TRY(run.alloc(&d_in, bytes));
    TOPO_TRY(run.alloc(&d_norm, bytes));
    TOPO_TRY(run.alloc(&d_dir, bytes));
    run.prefault(norm_out, bytes);
    run.prefault(dir_out, bytes);
    // (not pipelined: half a second of kernels per 20 ms of copies at full size, and the FFT route of the large kernels is
    // not cut-invariant)
    return run_pipelined(run, src, (float*)d_in, ny, nx, 0, true, kOneChunk, {{norm_out, d_norm}, {dir_out, d_dir}},
                         [&](int view_rows, int r0, int rows) {
                             return topo_amd_valley_ridge_dev((const float*)d_in, view_rows, 0, ny, nx, taps, ksize, angles, n_angles,
                                                              n_planes, mean, stdev, r0, rows, shift((float*)d_norm, r0, nx),
                                                              shift((float*)d_dir, r0, nx));
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
    Source src;
    TOPO_TRY(make_source(raster, "valley_ridge", &src));
    OutPlane outs[2];
    TOPO_TRY(make_out(norm_plane, "valley_ridge", &outs[0]));
    TOPO_TRY(make_out(dir_plane, "valley_ridge", &outs[1]));
    TOPO_REQUIRE(ny >= 1 && nx >= 1 && outs[0] && outs[1], "valley_ridge: bad arguments");
    TOPO_REQUIRE(sigma >= 0.0, "valley_ridge: sigma %g", sigma);
    const size_t bytes = (size_t)ny * nx * sizeof(float);
    HostRun run;
    void *d_in = nullptr, *d_smooth = nullptr, *d_res[2] = {nullptr, nullptr};
    TOPO_TRY(run.alloc(&d_in, bytes));
    TOPO_TRY(run.alloc(&d_res[0], bytes));
    TOPO_TRY(run.alloc(&d_res[1], bytes));
    if (sigma > 0.0) TOPO_TRY(run.alloc(&d_smooth, bytes));
    for (int q = 0; q < 2; ++q) run.prefault(outs[q].host, outs[q].bytes(ny, nx));
    return run_pipelined(run, src, (float*)d_in, ny, nx, 0, true, kOneChunk, {outs[0].on((float*)d_res[0]), outs[1].on((float*)d_res[1])},
                         [&](int, int, int) {  // (one chunk: the whole raster)
                             const float* field = (const float*)d_in;
                             if (sigma > 0.0) {
                                 ClassScope cls(scan_source(src, ny, nx));  // the smoothing kernels topo_amd_gauss_raw takes for this raster
                                 TOPO_TRY(topo_amd_gaussian_dev(field, ny, 0, ny, nx, sigma, sigma, 0, ny, (float*)d_smooth));
                                 field = (const float*)d_smooth;
                             }
                             return topo_amd_valley_ridge_std_dev(field, ny, nx, taps, ksize, angles, n_angles, n_planes, chunk,
                                                                  (float*)d_res[0], (float*)d_res[1], moments_out);
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
    HostRun run(false);
    char* d_raw = nullptr;
    TOPO_TRY(raw_plane(run, src, ny, nx, &d_raw));
    // the copies on the upload stream, each chunk's decode on the compute stream behind its copy: chunk k is decoded while
    // chunk k + 1 crosses the link (float32 as stored: nothing to decode, one copy)
    const int chunk = src.as_stored ? ny : pipeline_chunk_rows(ny, nx);
    const std::vector<int> cut = chunk >= ny ? std::vector<int>{0, ny} : pipeline_cuts(ny, chunk);
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
