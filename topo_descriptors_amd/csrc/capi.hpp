// What the units of the C API (context.hip, raster_class.hip, capi.hip, host_api.hip, shard.hip) share with each other.
// Each unit keeps its state to itself; another unit reaches it through the functions below.  The kernels' header is common.hpp.
#pragma once

#include <cmath>

#include "common.hpp"

namespace topo {

struct DecodeParams;  // decode.hpp

// ---- raster_class.hip -----------------------------------------------------------------------------------------------------
// Around the launchers of one entry point.  The outermost scope on a thread names the block (or, for the host-buffer
// entry points, the class found on the caller's array); scopes inside it - the device entry points the host-buffer ones
// call, the Gaussian in front of a disc - change nothing, so a smoothed plane inherits the class of the DEM it came from.
struct ClassScope {
    bool outer;
    explicit ClassScope(const Block& b);
    explicit ClassScope(const RasterClass& c);
    ~ClassScope();
    ClassScope(const ClassScope&) = delete;
    ClassScope& operator=(const ClassScope&) = delete;
};
inline void forget_plane(const void* p, int rows, int nx) {
    if (p) dem_memo_forget(p, (size_t)rows * nx * sizeof(float));
}
bool declared_class(const Block& b, RasterClass* out);
void declare_class(const float* block, int in_rows, int gny, int nx, const RasterClass& cls);
// the lattice samples of a raster, added up
struct Scan {
    unsigned long long taken = 0, large = 0, frac = 0;
    float lo = INFINITY, hi = -INFINITY;
    void add(float x);
};
RasterClass class_of(const Scan& s);
// scans the lattice points in rows [own_row0, own_row0 + own_rows) of the block; synchronises the compute stream
int scan_block(const Block& b, int own_row0, int own_rows, Scan* out);
// the class of a caller's host array of ny x nx samples, each decoded as the device will decode it
RasterClass scan_host_raster(const void* data, int dtype, const DecodeParams& p, bool as_stored, int ny, int nx);
void release_raster_class();  // topo_amd_shutdown: every declaration, the DEM memo and its pinned words

// ---- capi.hip -------------------------------------------------------------------------------------------------------------
inline float* shift(float* p, int rows, int nx) { return p ? p + (size_t)rows * nx : nullptr; }
int tpi_std_block(const Block& b, int size, double sigma, float* tpi_out, float* std_out);
int tpi_std_valid_block(const Block& b, int size, int min_count, float* tpi_out, float* std_out);
// rows above / below an output row that the ray pixels n0 ... n1 - 1 of the Sx tables reach
void sx_reach(const int32_t* dj, const double* dist, int n0, int n1, int* up, int* down);
// x_coords (host, nx entries; NULL: the column index) must be finite and strictly monotonic; *ascending: their direction
int check_fill_coords(const double* x, int nx, bool* ascending);
void note_valley_moments(int route);  // what topo_amd_valley_moments_route reports for the calling thread

// ---- host_api.hip ---------------------------------------------------------------------------------------------------------
void prefault_pages(void* host, size_t bytes);  // PageToucher::prefault on its own: returns when the pages are there

// ---- shard.hip ------------------------------------------------------------------------------------------------------------
int check_gate_errors();  // behind every call that synchronises: a lean-mode wait at the ghost-row gate that ran out
void reset_shard();       // topo_amd_init: the give-up counters of the gate's mode logic
void release_shard();     // topo_amd_shutdown: the communicator

}  // namespace topo
