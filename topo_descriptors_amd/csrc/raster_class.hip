// C ABI of libtopo_amd.so (declared in include/topo_amd.h), the raster class: the DEM memo, what was declared for row
// blocks, the lattice scan of a raster, and the class of the call in flight (common.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi.hpp"
#include "decode.hpp"

namespace topo {

// ---- dem_memo and the raster class (common.hpp) -------------------------------------------------------------------------
namespace {
struct DemMemo {
    const void* in = nullptr;
    int rows = 0, nx = 0;
    unsigned long used = 0;
    unsigned asked = 0;     // calls that asked "wild?" (every 32nd one is told no: the fused kernel looks again; time only)
    bool cls_valid = false;  // the block is a whole raster and has been scanned
    RasterClass cls;
};
constexpr int kMemos = 8;
constexpr int kMemoWords = 4;
DemMemo g_memo[kMemos];
uint32_t* g_memo_words = nullptr;  // pinned: kMemoWords words per entry: tiles, fractional tiles, wild sample seen
unsigned long g_memo_clock = 0;
std::mutex g_memo_mu;              // (several driver threads: topo_amd_shard_layout is per thread for them)

// g_memo_mu held
int memo_slot(const Block& b, bool create) {
    if (!g_memo_words) {
        if (hipHostMalloc((void**)&g_memo_words, kMemos * kMemoWords * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess) return -1;
        std::memset(g_memo_words, 0, kMemos * kMemoWords * sizeof(uint32_t));
    }
    int oldest = 0;
    for (int k = 0; k < kMemos; ++k) {
        if (g_memo[k].in == b.in && g_memo[k].rows == b.in_rows && g_memo[k].nx == b.nx) {
            g_memo[k].used = ++g_memo_clock;
            return k;
        }
        if (g_memo[k].used < g_memo[oldest].used) oldest = k;
    }
    if (!create) return -1;
    g_memo[oldest] = DemMemo{b.in, b.in_rows, b.nx, ++g_memo_clock, 0, false, RasterClass()};
    // (a launch in flight may still write the evicted entry's words: they are cleared here, and a late report for
    // another DEM can at worst pick the slower first kernel once - the results do not depend on that choice)
    for (int w = 0; w < kMemoWords; ++w) g_memo_words[kMemoWords * oldest + w] = 0;
    return oldest;
}
// What was declared for partial row blocks (topo_amd_raster_class_set / _from_scan / topo_amd_shard_classify): keyed by the
// device rows the declaration was made for and the shape of the raster they belong to.  A call's block finds its class
// when its first row lies inside a declared range of a raster of the same shape.  Declarations of one raster shape and
// class may overlap (row blocks of one buffer, each with its ghost rows: one entry per block); a declaration replaces
// the entries it overlaps that have another shape or class, and the entry of exactly its rows.  Dropped like the memo:
// whenever the library writes or frees memory that overlaps the range, by topo_amd_dem_changed, and by a withdrawal.
// Nothing here belongs to a thread or outlives its memory: two rasters in one process cannot inherit each other's class.
struct Declared {
    uintptr_t lo = 0, hi = 0;  // [lo, hi): the device rows
    int gny = 0, nx = 0;
    unsigned long used = 0;
    RasterClass cls;
};
constexpr size_t kMaxDeclared = 256;
std::vector<Declared> g_declared;  // g_memo_mu held
// g_memo_mu held
const Declared* find_declared(const Block& b) {
    const uintptr_t p = (uintptr_t)b.in;
    for (Declared& e : g_declared)
        if (p >= e.lo && p < e.hi && e.gny == b.gny && e.nx == b.nx) {
            e.used = ++g_memo_clock;
            return &e;
        }
    return nullptr;
}
// g_memo_mu held
void forget_declared(uintptr_t lo, uintptr_t hi) {
    g_declared.erase(std::remove_if(g_declared.begin(), g_declared.end(), [&](const Declared& e) { return e.lo < hi && lo < e.hi; }),
                     g_declared.end());
}
}  // namespace
bool declared_class(const Block& b, RasterClass* out) {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const Declared* e = find_declared(b);
    if (e && out) *out = e->cls;
    return e != nullptr;
}
void declare_class(const float* block, int in_rows, int gny, int nx, const RasterClass& cls) {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const uintptr_t lo = (uintptr_t)block, hi = lo + (size_t)in_rows * nx * sizeof(float);
    // a declaration replaces what was declared for overlapping memory of a raster of another shape or with another class,
    // and a declaration of exactly these rows; overlapping blocks of the same raster and class (row blocks of one buffer,
    // each with its ghost rows) keep their own entries, so a later write drops only those overlapping the written rows
    const auto replaced = [&](const Declared& e) {
        if (!(e.lo < hi && lo < e.hi)) return false;
        const bool same = e.gny == gny && e.nx == nx && e.cls.large == cls.large && e.cls.lo == cls.lo && e.cls.hi == cls.hi &&
                          e.cls.frac_share == cls.frac_share;
        return !same || (e.lo == lo && e.hi == hi);
    };
    g_declared.erase(std::remove_if(g_declared.begin(), g_declared.end(), replaced), g_declared.end());
    if (g_declared.size() >= kMaxDeclared) {
        auto oldest = std::min_element(g_declared.begin(), g_declared.end(), [](const Declared& x, const Declared& y) { return x.used < y.used; });
        g_declared.erase(oldest);
    }
    Declared e;
    e.lo = lo;
    e.hi = hi;
    e.gny = gny;
    e.nx = nx;
    e.used = ++g_memo_clock;
    e.cls = cls;
    g_declared.push_back(e);
}

uint32_t* dem_memo_report(const Block& b) {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const int k = memo_slot(b, true);
    return k < 0 ? nullptr : g_memo_words + kMemoWords * k;
}
bool dem_memo_mostly_fractional(const Block& b) {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const int k = memo_slot(b, false);
    if (k < 0) return false;
    // (both routes report afresh on every call, so a wrong guess costs one slower call and corrects itself)
    const uint32_t tiles = *(volatile uint32_t*)(g_memo_words + kMemoWords * k), frac = *(volatile uint32_t*)(g_memo_words + kMemoWords * k + 1);
    return tiles > 0 && 2 * frac > tiles;
}

uint32_t* dem_memo_wild_word(const Block& b) {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const int k = memo_slot(b, true);
    return k < 0 ? nullptr : g_memo_words + kMemoWords * k + 2;
}
bool dem_memo_wild(const Block& b) {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const int k = memo_slot(b, false);
    if (k < 0) return false;
    if (++g_memo[k].asked % 32 == 0) {  // (a caller may have rewritten the buffer with kernels of its own and not said so)
        *(volatile uint32_t*)(g_memo_words + kMemoWords * k + 2) = 0;
        return false;
    }
    return *(volatile uint32_t*)(g_memo_words + kMemoWords * k + 2) != 0;
}
// every entry whose block overlaps [p, p + bytes) (bytes == 0: that starts at p) is dropped
void dem_memo_forget(const void* p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(g_memo_mu);
    const uintptr_t lo = (uintptr_t)p, hi = lo + (bytes ? bytes : 1);
    forget_declared(lo, hi);
    for (int k = 0; k < kMemos; ++k) {
        DemMemo& m = g_memo[k];
        if (!m.in) continue;
        const uintptr_t a = (uintptr_t)m.in, b = a + (size_t)m.rows * m.nx * sizeof(float);
        if (a < hi && lo < b) {
            m = DemMemo();
            if (g_memo_words)
                for (int w = 0; w < kMemoWords; ++w) g_memo_words[kMemoWords * k + w] = 0;
        }
    }
}

// ---- lattice scan of a raster (the raster class) ---------------------------------------------------------------------------
// The lattice belongs to the GLOBAL grid: rows step_r / 2 + i step_r, columns step_c / 2 + j step_c with step = extent / 128
// (about 16 K points), so the scans of the row blocks of a raster add up to the scan of the whole raster, point for point.
namespace {
constexpr float kClassLarge = 1.0e5f;     // kWild of gauss_f16.hip: what the f16 matrix-core kernels stage as 0 and repair
constexpr float kClassOrdinary = 262144.0f;  // kAbsLim of the disc kernels
inline int lattice_step(int extent) { return std::max(1, extent / 128); }
__device__ __forceinline__ uint32_t ordered_bits(float f) {  // unsigned order = float order (finite values)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float from_ordered_bits(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}
// words: [0] taken, [1] large, [2] min key, [3] max key, [4] fractional (pinned host memory)
__global__ __launch_bounds__(256) void raster_scan_kernel(const float* in, int in_rows, int in_row0, int nx, int own_row0, int own_rows,
                                                          int step_r, int step_c, int ni, int nj, uint32_t* words) {
    const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
    const int i = idx / nj, j = idx - i * nj;
    const int r = step_r / 2 + i * step_r, c = step_c / 2 + j * step_c;
    const bool take = i < ni && r >= own_row0 && r < own_row0 + own_rows && r >= in_row0 && r < in_row0 + in_rows && c < nx;
    const float x = take ? in[(size_t)(r - in_row0) * nx + c] : 0.0f;
    const float a = fabsf(x);
    const bool large = take && a > kClassLarge && a <= 3.0e38f;
    const bool ordinary = take && a <= kClassOrdinary;
    const bool fractional = take && a <= 3.0e38f && x != truncf(x);
    uint32_t kmin = ordinary ? ordered_bits(x) : 0xffffffffu, kmax = ordinary ? ordered_bits(x) : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, m));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, m));
    }
    const unsigned long long mt = __builtin_amdgcn_ballot_w64(take), ml = __builtin_amdgcn_ballot_w64(large);
    const unsigned long long mf = __builtin_amdgcn_ballot_w64(fractional);
    if ((threadIdx.x & 63) == 0 && mt) {
        __hip_atomic_fetch_add(words, (uint32_t)__builtin_popcountll(mt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (ml) __hip_atomic_fetch_add(words + 1, (uint32_t)__builtin_popcountll(ml), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (mf) __hip_atomic_fetch_add(words + 4, (uint32_t)__builtin_popcountll(mf), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_fetch_min(words + 2, kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_fetch_max(words + 3, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
uint32_t* g_scan_words = nullptr;  // pinned
std::mutex g_scan_mu;
// the same lattice on a host array (the host-buffer entry points: no launch, no synchronisation), each sample decoded
// as the device will decode it (decode.hpp): the class is that of the float32 plane the kernels read
// (kAsStored: a float32 source that goes to the device untouched is classified on its own bits)
template <bool kAsStored, class T>
RasterClass scan_host(const T* dem, const DecodeParams& p, int ny, int nx) {
    Scan s;
    const int step_r = lattice_step(ny), step_c = lattice_step(nx);
    for (int r = step_r / 2; r < ny; r += step_r)
        for (int c = step_c / 2; c < nx; c += step_c) {
            const T x = dem[(size_t)r * nx + c];
            if constexpr (kAsStored) s.add((float)x);
            else s.add(decode_host(x, p));
        }
    return class_of(s);
}
// The class of the call in flight on this thread: set by the outermost entry point, resolved when a launcher first asks.
thread_local const Block* t_call_block = nullptr;  // the block the outermost entry point was given
thread_local bool t_class_known = false;
thread_local RasterClass t_class;
}  // namespace
void Scan::add(float x) {
    ++taken;
    const float a = std::fabs(x);
    if (a > kClassLarge && a <= 3.0e38f) ++large;
    if (a <= 3.0e38f && x != std::trunc(x)) ++frac;
    if (a <= kClassOrdinary) {  // (false for NaN)
        lo = std::min(lo, x);
        hi = std::max(hi, x);
    }
}
RasterClass class_of(const Scan& s) {
    RasterClass c;
    c.large = 4 * s.large > s.taken;
    c.frac_share = s.taken ? (float)((double)s.frac / (double)s.taken) : 0.0f;
    c.lo = s.lo;
    c.hi = s.hi;
    return c;
}
int scan_block(const Block& b, int own_row0, int own_rows, Scan* out) {
    std::lock_guard<std::mutex> lock(g_scan_mu);
    Context& c = ctx();
    if (!g_scan_words) TOPO_HIP(hipHostMalloc((void**)&g_scan_words, 8 * sizeof(uint32_t), hipHostMallocMapped));
    TOPO_HIP(hipStreamSynchronize(c.compute));  // (no scan of an earlier call in flight on the words; the block's data are final)
    g_scan_words[0] = g_scan_words[1] = g_scan_words[4] = 0;
    g_scan_words[2] = 0xffffffffu;
    g_scan_words[3] = 0u;
    const int step_r = lattice_step(b.gny), step_c = lattice_step(b.nx);
    const int ni = (b.gny - step_r / 2 + step_r - 1) / step_r, nj = (b.nx - step_c / 2 + step_c - 1) / step_c;
    const long n = (long)ni * nj;
    hipLaunchKernelGGL(raster_scan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.compute, b.in, b.in_rows, b.in_row0, b.nx,
                       own_row0, own_rows, step_r, step_c, ni, nj, g_scan_words);
    TOPO_HIP(hipGetLastError());
    TOPO_HIP(hipStreamSynchronize(c.compute));
    out->taken += g_scan_words[0];
    out->large += g_scan_words[1];
    out->frac += g_scan_words[4];
    if (g_scan_words[2] <= g_scan_words[3]) {
        out->lo = std::min(out->lo, from_ordered_bits(g_scan_words[2]));
        out->hi = std::max(out->hi, from_ordered_bits(g_scan_words[3]));
    }
    return TOPO_AMD_OK;
}
RasterClass scan_host_raster(const void* data, int dtype, const DecodeParams& p, bool as_stored, int ny, int nx) {
    RasterClass cls;
    if (as_stored) return scan_host<true>((const float*)data, p, ny, nx);
    with_sample_type(dtype, [&](auto t) { cls = scan_host<false>((const decltype(t)*)data, p, ny, nx); });
    return cls;
}

RasterClass current_class() {
    if (t_class_known) return t_class;
    RasterClass c;  // nothing declared: an ordinary DEM in whole metres
    const Block* b = t_call_block;
    if (b != nullptr && !(b->in_row0 == 0 && b->in_rows == b->gny)) (void)declared_class(*b, &c);
    if (b != nullptr && b->in_row0 == 0 && b->in_rows == b->gny) {
        // the block IS the raster: its own scan, remembered with the block
        bool have = false;
        {
            std::lock_guard<std::mutex> lock(g_memo_mu);
            const int k = memo_slot(*b, true);
            if (k >= 0 && g_memo[k].cls_valid) {
                c = g_memo[k].cls;
                have = true;
            }
        }
        if (!have) {
            Scan s;
            if (scan_block(*b, 0, b->gny, &s) == TOPO_AMD_OK) {
                c = class_of(s);
                std::lock_guard<std::mutex> lock(g_memo_mu);
                const int k = memo_slot(*b, true);
                if (k >= 0) {
                    g_memo[k].cls = c;
                    g_memo[k].cls_valid = true;
                }
            }
        }
    }
    t_class = c;
    t_class_known = true;
    return c;
}

ClassScope::ClassScope(const Block& b) : outer(t_call_block == nullptr && !t_class_known) {
    if (outer) t_call_block = &b;
}
ClassScope::ClassScope(const RasterClass& c) : outer(t_call_block == nullptr && !t_class_known) {
    if (outer) {
        t_class = c;
        t_class_known = true;
    }
}
ClassScope::~ClassScope() {
    if (outer) {
        t_call_block = nullptr;
        t_class_known = false;
    }
}

void release_raster_class() {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    g_declared.clear();
    if (g_memo_words) {
        (void)hipHostFree(g_memo_words);
        g_memo_words = nullptr;
        for (auto& m : g_memo) m = DemMemo();
    }
}

}  // namespace topo

using namespace topo;

extern "C" {

// ---- the raster class (common.hpp) ----------------------------------------------------------------------------------
int topo_amd_dem_changed(const void* dptr, size_t bytes) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(dptr != nullptr, "dem_changed: NULL pointer");
    if (bytes == 0) {  // the whole allocation
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dptr) == hipSuccess) dem_memo_forget(base, size);
        else (void)hipGetLastError();
    }
    dem_memo_forget(dptr, bytes);
    return TOPO_AMD_OK;
}

int topo_amd_raster_scan_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int own_row0, int own_rows,
                             uint64_t counts[3], float range[2]) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(in && counts && range && gny >= 1 && nx >= 1 && in_rows >= 1 && in_row0 >= 0 && in_row0 + in_rows <= gny,
                 "raster_scan: bad block");
    TOPO_REQUIRE(own_rows >= 0 && own_row0 >= in_row0 && own_row0 + own_rows <= in_row0 + in_rows,
                 "raster_scan: rows [%d, %d) are not inside the block's rows [%d, %d)", own_row0, own_row0 + own_rows, in_row0,
                 in_row0 + in_rows);
    Block b{in, in_rows, in_row0, gny, nx, own_row0, own_rows};
    Scan s;
    s.lo = range[0];
    s.hi = range[1];
    TOPO_TRY(scan_block(b, own_row0, own_rows, &s));
    counts[0] += s.taken;
    counts[1] += s.large;
    counts[2] += s.frac;
    range[0] = s.lo;
    range[1] = s.hi;
    return TOPO_AMD_OK;
}

namespace {
int check_declared_rows(const float* block, int in_rows, int gny, int nx, const char* who) {
    TOPO_REQUIRE(block != nullptr && in_rows >= 1 && gny >= in_rows && nx >= 1,
                 "%s: the declaration is for device rows: block != NULL, 1 <= in_rows <= gny, nx >= 1 (got %p, %d, %d, %d)", who,
                 (const void*)block, in_rows, gny, nx);
    return TOPO_AMD_OK;
}
}  // namespace

int topo_amd_raster_class_set(const float* block, int in_rows, int gny, int nx, int large, float lo, float hi, float frac_share) {
    if (large < 0) {  // withdraw: what was declared for memory overlapping these rows (block == NULL: every declaration)
        std::lock_guard<std::mutex> lock(g_memo_mu);
        if (block == nullptr) g_declared.clear();
        else forget_declared((uintptr_t)block, (uintptr_t)block + (size_t)std::max(1, in_rows) * std::max(1, nx) * sizeof(float));
        return TOPO_AMD_OK;
    }
    TOPO_TRY(check_declared_rows(block, in_rows, gny, nx, "raster_class_set"));
    TOPO_REQUIRE(!(lo != lo) && !(hi != hi) && frac_share >= 0.0f && frac_share <= 1.0f, "raster_class_set: bad range or share");
    RasterClass c;
    c.large = large != 0;
    c.lo = lo;
    c.hi = hi;
    c.frac_share = frac_share;
    declare_class(block, in_rows, gny, nx, c);
    return TOPO_AMD_OK;
}

int topo_amd_raster_class_from_scan(const float* block, int in_rows, int gny, int nx, const uint64_t counts[3], const float range[2]) {
    TOPO_REQUIRE(counts && range, "raster_class_from_scan: NULL argument");
    TOPO_TRY(check_declared_rows(block, in_rows, gny, nx, "raster_class_from_scan"));
    Scan s;
    s.taken = counts[0];
    s.large = counts[1];
    s.frac = counts[2];
    s.lo = range[0];
    s.hi = range[1];
    declare_class(block, in_rows, gny, nx, class_of(s));
    return TOPO_AMD_OK;
}

int topo_amd_raster_class_get(const float* block, int gny, int nx, int* declared, int* large, float* lo, float* hi, float* frac_share) {
    TOPO_REQUIRE(block && declared && large && lo && hi && frac_share, "raster_class_get: NULL argument");
    RasterClass c;  // (nothing declared: what a partial block is then taken for)
    Block b{block, 1, 0, gny, nx, 0, 1};
    *declared = declared_class(b, &c) ? 1 : 0;
    *large = c.large ? 1 : 0;
    *lo = c.lo;
    *hi = c.hi;
    *frac_share = c.frac_share;
    return TOPO_AMD_OK;
}

}  // extern "C"
