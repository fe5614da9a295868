// C ABI of libtopo_amd.so (declared in include/topo_amd.h), the device row-block entry points: the descriptors on a row
// block, the geometry helpers, and the kernel-route reports.  Its other parts: context.hip, raster_class.hip, host_api.hip
// (the host-buffer entry points) and shard.hip (RCCL ghost-row exchange for row shards).
#include <algorithm>
#include <cmath>

#include "capi.hpp"

namespace topo {

// compose pre-smoothing + disc: TPI/STD with sigma (topo.py:172-173, :297-298)
int tpi_std_block(const Block& b, int size, double sigma, float* tpi_out, float* std_out) {
    DiscRuns disc;
    TOPO_TRY(build_disc(size, &disc));
    const int above = -disc.dj_min, below = disc.dj_max;
    if (!(sigma > 0.0)) {
        TOPO_TRY(check_block(b, above, below, "tpi_std"));
        return launch_tpi_std(b, disc, tpi_out, std_out);
    }
    const int R = gaussian_radius(sigma);
    TOPO_TRY(check_block(b, above + R, below + R, "tpi_std(sigma)"));
    // smooth exactly the rows the disc will read, then run the disc on that plane
    const int s0 = std::max(0, b.out_row0 - above);
    const int s1 = std::min(b.gny, b.out_row0 + b.out_rows + below);
    void* plane = nullptr;
    TOPO_TRY(workspace(3, (size_t)(s1 - s0) * b.nx * sizeof(float), &plane));
    Block g = b;
    g.out_row0 = s0;
    g.out_rows = s1 - s0;
    TOPO_TRY(launch_gaussian(g, sigma, sigma, (float*)plane));
    dem_memo_forget(plane, (size_t)(s1 - s0) * b.nx * sizeof(float));  // (the workspace holds another plane now)
    Block d = b;
    d.in = (const float*)plane;
    d.in_row0 = s0;
    d.in_rows = s1 - s0;
    return launch_tpi_std(d, disc, tpi_out, std_out);
}

// TPI / STD over the valid samples of the disc (disc_valid.hip); the caller has taken the call's flag word (disc_valid_begin)
int tpi_std_valid_block(const Block& b, int size, int min_count, float* tpi_out, float* std_out) {
    TOPO_REQUIRE(size >= 1, "tpi_std_valid: disc size %d (at least 1)", size);
    TOPO_REQUIRE(min_count >= 1, "tpi_std_valid: min_count %d (at least 1)", min_count);
    TOPO_REQUIRE(tpi_out || std_out, "tpi_std_valid: both outputs are NULL");
    DiscRuns disc;
    TOPO_TRY(build_disc(size, &disc));
    TOPO_TRY(check_block(b, -disc.dj_min, disc.dj_max, "tpi_std_valid"));
    return launch_tpi_std_valid(b, disc, min_count, tpi_out, std_out);
}

namespace {
thread_local int t_tpi_route = 0;    // 1: the calling thread's last TPI / STD disc call took the wide ring (topo_amd_tpi_route)
thread_local int t_valley_route = 0;  // the evaluation the calling thread's last valley / ridge call took (topo_amd_valley_route)
thread_local int t_valley_moments = 0;  // 1: that call formed the DEM's mean / std on the device (topo_amd_valley_moments_route)
thread_local int t_sx_route = 0;      // the kernel route the calling thread's last Sx call took (topo_amd_sx_route)
thread_local int t_gradient_route = 0;  // the same of its last gradient call (topo_amd_gradient_route)
thread_local int t_disc_route = 0;      // the same of its last TPI / STD disc call (topo_amd_disc_route)
int report_route(int* route, int value, const char* who) {
    TOPO_REQUIRE(route != nullptr, "%s: NULL output", who);
    *route = value;
    return TOPO_AMD_OK;
}
}  // namespace
void note_tpi_route(int route) { t_tpi_route = route; }
void note_valley_route(int route) { t_valley_route = route; }
void note_sx_route(int route) { t_sx_route = route; }
void note_gradient_route(int route) { t_gradient_route = route; }
void note_disc_route(int route) { t_disc_route = route; }
int noted_disc_route() { return t_disc_route; }
void note_valley_moments(int route) { t_valley_moments = route; }

void sx_reach(const int32_t* dj, const double* dist, int n0, int n1, int* up, int* down) {
    *up = *down = 0;
    for (int n = n0; n < n1; ++n) {
        if (std::isnan(dist[n])) continue;
        *up = std::max(*up, -dj[n]);
        *down = std::max(*down, dj[n]);
    }
}

int check_fill_coords(const double* x, int nx, bool* ascending) {
    *ascending = true;
    if (!x) return TOPO_AMD_OK;
    for (int i = 0; i < nx; ++i) TOPO_REQUIRE(std::isfinite(x[i]), "fill_na: x_coords[%d] is not finite", i);
    if (nx >= 2) *ascending = x[1] > x[0];
    for (int i = 1; i < nx; ++i)
        TOPO_REQUIRE(*ascending ? x[i] > x[i - 1] : x[i] < x[i - 1], "fill_na: x_coords are not strictly monotonic at index %d", i);
    return TOPO_AMD_OK;
}

}  // namespace topo

using namespace topo;

extern "C" {

int topo_amd_tpi_route(int* route) { return report_route(route, t_tpi_route, "tpi_route"); }
int topo_amd_valley_route(int* route) { return report_route(route, t_valley_route, "valley_route"); }
int topo_amd_valley_moments_route(int* route) { return report_route(route, t_valley_moments, "valley_moments_route"); }
int topo_amd_sx_route(int* route) { return report_route(route, t_sx_route, "sx_route"); }
int topo_amd_gradient_route(int* route) { return report_route(route, t_gradient_route, "gradient_route"); }
int topo_amd_disc_route(int* route) {  // (the wide-ring bit IS topo_amd_tpi_route)
    if ((t_disc_route & kDiscLauncherMask) == kDiscValid) {
        // the slow-form bit is the kernels' word: read from the device behind the call's launches
        TOPO_ENTER();
        int slow = 0;
        TOPO_TRY(disc_valid_slow(&slow));
        return report_route(route, (t_disc_route & ~kDiscValidSlow) | (slow ? kDiscValidSlow : 0), "disc_route");
    }
    return report_route(route, (t_disc_route & ~kDiscWideRing) | (t_tpi_route ? kDiscWideRing : 0), "disc_route");
}

int topo_amd_synth_dem_dev(float* out, int rows, int row0, int nx, uint32_t seed, int integer_valued) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(out && rows >= 1 && nx >= 1, "synth_dem: bad arguments");
    forget_plane(out, rows, nx);
    return launch_synth(out, rows, row0, nx, seed, integer_valued != 0);
}

// ---- geometry helpers ---------------------------------------------------------------------
int topo_amd_disc_tap_count(int size) {
    DiscRuns d;
    if (build_disc(size, &d) != TOPO_AMD_OK) return TOPO_AMD_EINVAL;
    return d.taps;
}

int topo_amd_disc_mask(int size, float* mask) {
    TOPO_REQUIRE(mask != nullptr, "disc_mask: NULL output");
    DiscRuns d;
    TOPO_TRY(build_disc(size, &d));
    const int c = (size - 1) / 2;
    for (int a = 0; a < size; ++a) {
        const int row = (c - a) - d.dj_min;
        for (int b = 0; b < size; ++b) {
            const int di = c - b;
            mask[a * size + b] = (di >= d.lo[row] && di <= d.hi[row]) ? 1.0f : 0.0f;
        }
    }
    return TOPO_AMD_OK;
}

int topo_amd_halo_rows(int descriptor, double p0, double p1, int* above, int* below) {
    TOPO_REQUIRE(above && below, "halo_rows: NULL output");
    switch (descriptor) {
        case TOPO_AMD_DESC_TPI:
        case TOPO_AMD_DESC_STD: {
            DiscRuns d;
            TOPO_TRY(build_disc((int)p0, &d));
            const int R = p1 > 0.0 ? gauss_ghost_rows(p1) : 0;  // the pre-smoothing
            *above = -d.dj_min + R;
            *below = d.dj_max + R;
            return TOPO_AMD_OK;
        }
        case TOPO_AMD_DESC_GAUSS:
            *above = *below = gauss_ghost_rows(p0);
            return TOPO_AMD_OK;
        case TOPO_AMD_DESC_GRADIENT:
            *above = *below = gradient_ghost_rows(p0, p1, false);
            return TOPO_AMD_OK;
        case TOPO_AMD_DESC_SOBEL:
            *above = *below = 1;
            return TOPO_AMD_OK;
        case TOPO_AMD_DESC_SX:
            *above = p0 > 0 ? (int)p0 : 0;
            *below = p1 > 0 ? (int)p1 : 0;
            return TOPO_AMD_OK;
        case TOPO_AMD_DESC_VALLEY_RIDGE: {
            const int32_t kmax = (int32_t)p0;
            TOPO_REQUIRE(kmax >= 1, "halo_rows: kernel side %d", kmax);
            (void)valley_ridge_reach(&kmax, 1, above, below);
            const int R = p1 > 0.0 ? gauss_ghost_rows(p1) : 0;  // the pre-smoothing (topo_amd_shard_valley_ridge_smoothed)
            *above += R;
            *below += R;
            return TOPO_AMD_OK;
        }
        default:
            set_error("halo_rows: unknown descriptor %d", descriptor);
            return TOPO_AMD_EINVAL;
    }
}

// ---- device row-block entry points ------------------------------------------------------------
int topo_amd_tpi_std_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int size,
                         int out_row0, int out_rows, float* tpi_out, float* std_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    ClassScope cls(b);
    forget_plane(tpi_out, out_rows, nx);
    forget_plane(std_out, out_rows, nx);
    return tpi_std_block(b, size, 0.0, tpi_out, std_out);
}

int topo_amd_tpi_std_valid_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int size, int min_count, int out_row0,
                               int out_rows, float* tpi_out, float* std_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    forget_plane(tpi_out, out_rows, nx);
    forget_plane(std_out, out_rows, nx);
    TOPO_TRY(disc_valid_begin());  // (one flag word per call; the arguments are checked with the block)
    return tpi_std_valid_block(b, size, min_count, tpi_out, std_out);
}

int topo_amd_tpi_multi_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int n_sizes, const int32_t* sizes,
                           int out_row0, int out_rows, float* const* tpi_outs) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(n_sizes >= 1 && sizes && tpi_outs, "tpi_multi: no sizes");
    for (int k = 0; k < n_sizes; ++k) TOPO_REQUIRE(tpi_outs[k], "tpi_multi: NULL output plane %d", k);
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    ClassScope cls(b);
    for (int k = 0; k < n_sizes; ++k) forget_plane(tpi_outs[k], out_rows, nx);
    // sizes that have a two-disc kernel (disc_pair.hip) go through it in pairs - the smallest with the next one up,
    // so that the shared ring is no larger than it has to be - the rest one by one
    std::vector<int> order(n_sizes), left;
    for (int k = 0; k < n_sizes; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return sizes[x] < sizes[y]; });
    std::vector<char> done(n_sizes, 0);
    for (int i = 0; i + 1 < n_sizes; ++i) {
        const int a = order[i], c = order[i + 1];
        if (done[a] || done[c] || !tpi_pair_covers(sizes[a], sizes[c])) continue;
        DiscRuns da, dc;
        TOPO_TRY(build_disc(sizes[a], &da));
        TOPO_TRY(build_disc(sizes[c], &dc));
        TOPO_TRY(check_block(b, -dc.dj_min, dc.dj_max, "tpi_multi"));
        const int rc = launch_tpi_pair(b, sizes[a], tpi_outs[a], sizes[c], tpi_outs[c]);
        if (rc == TOPO_AMD_EUNSUP) break;  // planes the 16-byte row accesses cannot take: single launches handle them
        if (rc != TOPO_AMD_OK) return rc;
        done[a] = done[c] = 1;
        ++i;
    }
    for (int k = 0; k < n_sizes; ++k)
        if (!done[k]) TOPO_TRY(tpi_std_block(b, sizes[k], 0.0, tpi_outs[k], nullptr));
    return TOPO_AMD_OK;
}

int topo_amd_gaussian_dev(const float* in, int in_rows, int in_row0, int gny, int nx,
                          double sigma_y, double sigma_x, int out_row0, int out_rows, float* out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(out != nullptr, "gaussian: NULL output");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "gaussian: negative sigma");
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    const int R = gaussian_radius(sigma_y);
    TOPO_TRY(check_block(b, R, R, "gaussian"));
    ClassScope cls(b);
    forget_plane(out, out_rows, nx);
    return launch_gaussian(b, sigma_y, sigma_x, out);
}

int topo_amd_gaussian_valid_dev(const float* in, int in_rows, int in_row0, int gny, int nx, double sigma_y, double sigma_x,
                                double min_weight, int fill, int out_row0, int out_rows, float* out, float* weight_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(out != nullptr, "gaussian_valid: NULL output");
    TOPO_REQUIRE(sigma_y >= 0.0 && sigma_x >= 0.0, "gaussian_valid: negative sigma");  // (false for NaN)
    TOPO_REQUIRE(min_weight >= 0.0 && min_weight <= 1.0, "gaussian_valid: min_weight %g outside [0, 1]", min_weight);
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    const int R = (int)std::min(4.0 * sigma_y + 0.5, kGaussValidMaxRadius + 1.0);  // (beyond it the launcher refuses the call)
    TOPO_TRY(check_block(b, R, R, "gaussian_valid"));
    forget_plane(out, out_rows, nx);
    forget_plane(weight_out, out_rows, nx);
    return launch_gaussian_valid(b, sigma_y, sigma_x, min_weight, fill != 0, out, weight_out);
}

int topo_amd_sobel_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int out_row0,
                       int out_rows, float* dx_out, float* dy_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    TOPO_TRY(check_block(b, 1, 1, "sobel"));
    forget_plane(dx_out, out_rows, nx);
    forget_plane(dy_out, out_rows, nx);
    return launch_sobel(b, dx_out, dy_out);
}

int topo_amd_gradient_dev(const float* in, int in_rows, int in_row0, int gny, int nx, double sigma,
                          double sig_ratio, int res_mode, const void* res_x, const void* res_y,
                          int out_row0, int out_rows, float* dx_out, float* dy_out,
                          float* slope_out, float* aspect_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    const int h = gradient_ghost_rows(sigma, sig_ratio, true);
    TOPO_TRY(check_block(b, h, h, "gradient"));
    ClassScope cls(b);
    for (float* o : {dx_out, dy_out, slope_out, aspect_out}) forget_plane(o, out_rows, nx);
    return launch_gradient(b, sigma, sig_ratio, res_mode, res_x, res_y, dx_out, dy_out, slope_out,
                           aspect_out);
}

int topo_amd_gradient_valid_dev(const float* in, int in_rows, int in_row0, int gny, int nx, double sigma, double sig_ratio,
                                double min_weight, int fill, int res_mode, const void* res_x, const void* res_y, int out_row0,
                                int out_rows, float* dx_out, float* dy_out, float* slope_out, float* aspect_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(sigma >= 0.0, "gradient_valid: negative sigma");  // (false for NaN)
    TOPO_REQUIRE(sig_ratio > 0.0 && sig_ratio <= 1e6, "gradient_valid: sig_ratio %g (a positive factor)", sig_ratio);
    TOPO_REQUIRE(min_weight >= 0.0 && min_weight <= 1.0, "gradient_valid: min_weight %g outside [0, 1]", min_weight);
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    // ghost rows: the wider filter's radius and the row of the difference; 1 for the Sobel pair (beyond the radii of the
    // valid-sample Gaussian the launcher refuses the call)
    const double wide = sigma > 1.0 ? std::max(sigma, sigma * sig_ratio) : 0.0;
    const int h = (int)std::min(4.0 * wide + 0.5, kGaussValidMaxRadius + 1.0) + 1;
    TOPO_TRY(check_block(b, h, h, "gradient_valid"));
    for (float* o : {dx_out, dy_out, slope_out, aspect_out}) forget_plane(o, out_rows, nx);
    return launch_gradient_valid(b, sigma, sig_ratio, min_weight, fill != 0, res_mode, res_x, res_y, dx_out, dy_out, slope_out,
                                 aspect_out);
}

int topo_amd_sx_dev(const float* in, int in_rows, int in_row0, int gny, int nx, const int32_t* dj,
                    const int32_t* di, const double* dist, int n_off, int window, double height,
                    int out_row0, int out_rows, float* out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(out && n_off >= 0 && (n_off == 0 || (dj && di && dist)), "sx: NULL argument");
    int up = 0, down = 0;
    sx_reach(dj, dist, 0, n_off, &up, &down);
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    // rows of the zero frame need no neighbours, interior rows never reach outside the DEM
    TOPO_TRY(check_block(b, up, down, "sx"));
    forget_plane(out, out_rows, nx);
    return launch_sx(b, dj, di, dist, n_off, window, height, out);
}

int topo_amd_sx_multi_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int n_az,
                          const int32_t* first, const int32_t* dj, const int32_t* di, const double* dist,
                          const int32_t* window, double height, int out_row0, int out_rows,
                          float* const* outs) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(n_az >= 1 && first && dj && di && dist && window && outs, "sx_multi: NULL argument");
    for (int k = 0; k < n_az; ++k) TOPO_REQUIRE(outs[k], "sx_multi: NULL output plane %d", k);
    int up = 0, down = 0;
    sx_reach(dj, dist, first[0], first[n_az], &up, &down);
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    TOPO_TRY(check_block(b, up, down, "sx_multi"));
    for (int k = 0; k < n_az; ++k) forget_plane(outs[k], out_rows, nx);
    return launch_sx_multi(b, n_az, first, dj, di, dist, window, height, outs);
}

int topo_amd_valley_ridge_dev(const float* in, int in_rows, int in_row0, int gny, int nx, const float* taps,
                              const int32_t* ksize, const float* angles, int n_angles, int n_planes, double mean,
                              double stdev, int out_row0, int out_rows, float* norm_out, float* dir_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(taps && ksize && angles && norm_out && dir_out && n_angles >= 1, "valley_ridge: NULL argument");
    int up = 0, down = 0;
    (void)valley_ridge_reach(ksize, n_angles, &up, &down);
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    TOPO_TRY(check_block(b, up, down, "valley_ridge"));
    t_valley_moments = 0;  // (the caller's)
    forget_plane(norm_out, out_rows, nx);
    forget_plane(dir_out, out_rows, nx);
    return launch_valley_ridge(b, taps, ksize, angles, n_angles, n_planes, mean, stdev, norm_out, dir_out);
}

int topo_amd_mean_std_dev(const float* in, size_t count, double* mean, double* stdev) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(in && mean && stdev && count >= 1, "mean_std: bad arguments");
    return launch_mean_std(in, count, mean, stdev);
}

int topo_amd_mean_std_f32_dev(const float* in, size_t count, size_t chunk, float* mean, float* stdev) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(in && mean && stdev && count >= 1, "mean_std_f32: bad arguments");
    return launch_mean_std_np(in, count, chunk, mean, stdev);
}

int topo_amd_valley_ridge_std_dev(const float* in, int ny, int nx, const float* taps, const int32_t* ksize, const float* angles,
                                  int n_angles, int n_planes, size_t chunk, float* norm_out, float* dir_out, float moments_out[2]) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(in && ny >= 1 && nx >= 1, "valley_ridge_std: bad DEM");
    float mean = 0.0f, stdev = 0.0f;
    TOPO_TRY(launch_mean_std_np(in, (size_t)ny * nx, chunk, &mean, &stdev));
    if (moments_out) {
        moments_out[0] = mean;
        moments_out[1] = stdev;
    }
    TOPO_TRY(topo_amd_valley_ridge_dev(in, ny, 0, ny, nx, taps, ksize, angles, n_angles, n_planes, (double)mean, (double)stdev, 0, ny,
                                       norm_out, dir_out));
    t_valley_moments = 1;
    return TOPO_AMD_OK;
}

// ---- gap filling: nearest valid sample along x (fill.hip; reference helpers.py:137-154 and :30-31) ---------------------
int topo_amd_fill_na_dev(const float* in, int in_rows, int in_row0, int gny, int nx, const double* x_coords, double min_elevation,
                         int out_row0, int out_rows, float* out, uint8_t* missing_out) {
    TOPO_ENTER();
    TOPO_TRY(require_ready());
    TOPO_REQUIRE(out != nullptr, "fill_na: NULL output");
    Block b{in, in_rows, in_row0, gny, nx, out_row0, out_rows};
    TOPO_TRY(check_block(b, 0, 0, "fill_na"));
    bool ascending = true;
    TOPO_TRY(check_fill_coords(x_coords, nx, &ascending));
    // in place means the block's own output rows; any other output must lie apart from them
    const size_t bytes = (size_t)out_rows * nx * sizeof(float);
    const uintptr_t own = (uintptr_t)(in + (size_t)(out_row0 - in_row0) * nx), o = (uintptr_t)out;
    TOPO_REQUIRE(o == own || o + bytes <= own || own + bytes <= o, "fill_na: the output overlaps the input rows without being them");
    const double* d_x = nullptr;
    if (x_coords) {
        void* t = nullptr;
        TOPO_TRY(upload_table(6, x_coords, (size_t)nx * sizeof(double), &t));
        d_x = (const double*)t;
    }
    forget_plane(out, out_rows, nx);  // (in place: what was remembered or declared for the DEM's rows goes with them)
    if (missing_out) dem_memo_forget(missing_out, (size_t)out_rows * nx);
    const bool thresh = !std::isnan(min_elevation);
    return launch_fill_na(b, d_x, ascending, thresh, thresh ? (float)min_elevation : 0.0f, out, missing_out);
}

}  // extern "C"
