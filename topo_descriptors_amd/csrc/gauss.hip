// K3: separable Gaussian - the vector-ALU kernels, the tap tables, and the smooth of a row block on whatever kernels its
// radius gets (the f16 matrix-core kernels are gauss_f16.hip; the gradient and Sobel, K4 / K5, gradient.hip).
//
// Replaces scipy.ndimage.gaussian_filter (topo.py:80, :173, :298, :631-635).
//
// Gaussian = two 1-D passes like scipy (axis 0, then axis 1), radius int(4 sigma + 0.5),
// float64-normalised taps rounded to float32, reflect ("symmetric") boundary at the GLOBAL
// DEM edges, and the intermediate rounded to float32 between the passes exactly as the
// reference does.  Each thread register-blocks TB consecutive outputs along the filter
// axis so that one loaded sample feeds TB FMAs; samples are taken relative to a per-thread
// offset so float32 accumulation keeps its digits on 2000 m terrain.
#include "gauss.hpp"

namespace topo {

namespace {

// ---- axis 0 (down the columns): lanes run along x, plain coalesced global loads ------------
// Row groups are aligned to GLOBAL multiples of TB and the accumulation offset c is a sample of
// the group itself, so an output pixel is computed by exactly the same instruction sequence
// whatever row block it is part of (shards stay bit-identical to the single-block run).
template <int TB, int KB>
__global__ __launch_bounds__(kThreads) void gauss_axis0_kernel(GaussArgs p) {
    const int x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= p.nx) return;
    const int y0 = (p.group0 + (int)blockIdx.y) * TB;
    const int first = y0 - p.radius;                       // global row of sample 0
    const int last = first + TB - 1 + p.nchunks * KB - 1;  // last sample fetched (the ones past 2 radius + TB - 1 meet no tap)
    const bool plain = first >= 0 && last < p.gny && first >= p.in_row0 && last < p.in_row0 + p.in_rows;
    const float* col = p.in + x;
    auto fetch = [&](int i) -> float {
        int gy = first + i;
        if (!plain) {  // wave-uniform: reflect at the global edges, clamp into the block
            gy = reflect_index(gy, p.gny);
            gy = min(max(gy, p.in_row0), p.in_row0 + p.in_rows - 1);
        }
        return col[(size_t)(gy - p.in_row0) * p.nx];
    };
    // the middle row of the group lies within `radius` rows of every row of the group, hence
    // inside any block that computes part of it - provided radius >= TB/2 - 1; tiny filters
    // accumulate without an offset (they have nothing to lose)
    // (a NaN or inf there would make every output of the group non-finite instead of the ones its taps reach)
    const float c = finite_or_zero(p.radius >= TB / 2 - 1 ? fetch(p.radius + TB / 2) : 0.0f);
    float acc[TB];
    tap_chunks<TB, KB>(p.taps, p.nchunks, c, fetch, acc);
#pragma unroll
    for (int t = 0; t < TB; ++t) {
        const int oy = y0 + t;
        if (oy >= p.out_row0 && oy < p.out_row0 + p.out_rows)
            p.out[(size_t)(oy - p.out_row0) * p.nx + x] = c + acc[t];
    }
}

// ---- axis 1 (along the rows): tile staged in LDS, lanes run along y ------------------------
// block = 64 rows x (NW * TB) output columns; wave w owns TB consecutive columns of every row.
template <int TB, int KB, int NW>
__global__ __launch_bounds__(NW * 64) void gauss_axis1_kernel(GaussArgs p) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    constexpr int TR = 64;
    constexpr int TC = NW * TB;
    const int R = p.radius;
    const int cols_l = TC + p.nchunks * KB - 1;  // samples a row of the tile can be asked for
    const int stride = cols_l | 1;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int ox0 = blockIdx.x * TC;
    const int oy0 = blockIdx.y * TR;  // relative to out_row0; rows here need no halo

    // stage: wave per row, lanes along x (coalesced); tiles that reach past the left/right DEM
    // edge reflect there, all others copy straight
    const bool inner = ox0 - R >= 0 && ox0 - R + cols_l <= p.nx;
    for (int r = wave; r < TR; r += NW) {
        const int row = min(oy0 + r, p.out_rows - 1);
        const float* src = p.in + (size_t)(row + p.out_row0 - p.in_row0) * p.nx;
        float* dst = L + r * stride;
        if (inner) {
            const float* s0 = src + (ox0 - R);
            for (int k = lane; k < cols_l; k += 64) dst[k] = s0[k];
        } else {
            for (int k = lane; k < cols_l; k += 64) dst[k] = src[reflect_index(ox0 - R + k, p.nx)];
        }
    }
    __syncthreads();

    const float* rowp = L + lane * stride + wave * TB;
    auto fetch = [&](int i) -> float { return rowp[i]; };
    const float c = finite_or_zero(rowp[R]);
    float acc[TB];
    tap_chunks<TB, KB>(p.taps, p.nchunks, c, fetch, acc);
    __syncthreads();
    // transpose back through LDS so the stores are row-coalesced
    constexpr int ostride = TC + 1;
    float* O = L;
#pragma unroll
    for (int t = 0; t < TB; ++t) O[lane * ostride + wave * TB + t] = c + acc[t];
    __syncthreads();
    for (int idx = threadIdx.x; idx < TR * TC; idx += NW * 64) {
        const int r = idx / TC, k = idx % TC;
        const int oy = oy0 + r, ox = ox0 + k;
        if (oy < p.out_rows && ox < p.nx) p.out[(size_t)oy * p.nx + ox] = O[r * ostride + k];
    }
}

// ---- plane transpose (used to run very long axis-1 filters as axis-0 filters) -----------------
__global__ __launch_bounds__(kThreads) void transpose_kernel(const float* in, float* out, int rows, int cols) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8 threads
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int y = y0 + ty + k, x = x0 + tx;
        if (y < rows && x < cols) tile[ty + k][tx] = in[(size_t)y * cols + x];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int y = x0 + ty + k, x = y0 + tx;  // coordinates in the transposed plane
        if (y < cols && x < rows) out[(size_t)y * rows + x] = tile[tx][ty + k];
    }
}

// ---- host side -----------------------------------------------------------------------------
int upload_weights(int slot, double sigma, int kb, GaussArgs* a) {
    const int R = gaussian_radius(sigma);
    std::vector<double> w;
    const double sum = gauss_taps(sigma, &w);
    const int nchunks = (2 * R + 1 + kb - 1) / kb;
    std::vector<float> padded((size_t)nchunks * kb, 0.0f);
    for (int k = 0; k <= 2 * R; ++k) padded[k] = (float)(w[k] / sum);
    // behind the plain taps (kb == 1): the slab table of the split-once kernels, W[d + 2][o] = the sum of the (float32)
    // taps that the output at position o = 0 ... 63 of its slab lays over the slab d slabs further on
    const size_t ntaps = padded.size();
    if (kb == 1) {
        padded.resize(ntaps + 5 * 64, 0.0f);
        for (int d = -2; d <= 2; ++d)
            for (int o = 0; o < 64; ++o) {
                double acc = 0.0;
                for (int k = 64 * d; k < 64 * d + 64; ++k) {
                    const int q = k - o + R;
                    if (q >= 0 && q <= 2 * R) acc += (double)padded[q];
                }
                padded[ntaps + (size_t)(d + 2) * 64 + o] = (float)acc;
            }
    }
    void* d = nullptr;
    TOPO_TRY(upload_table(slot, padded.data(), padded.size() * sizeof(float), &d));
    a->taps = (const float*)d;
    a->wtab = kb == 1 ? (const float*)d + ntaps : nullptr;
    a->radius = R;
    a->nchunks = nchunks;
    return TOPO_AMD_OK;
}

template <int TB, int KB, int NW>
int launch_axis1(const GaussArgs& a, int rows, int nx, double sigma) {
    Context& c = ctx();
    constexpr int tc = NW * TB;
    const size_t lds = axis1_tile_lds(TB, NW, axis1_tile_cols(TB, KB, NW, a.nchunks));
    if (lds > kLdsMax) {
        set_error("gaussian: sigma %.3f (radius %d) needs %zu B of LDS per tile; the "
                  "large-sigma path is not built yet", sigma, a.radius, lds);
        return TOPO_AMD_EUNSUP;
    }
    TOPO_HIP(hipFuncSetAttribute((const void*)gauss_axis1_kernel<TB, KB, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dim3 grid((nx + tc - 1) / tc, (rows + 63) / 64);
    return launch(gauss_axis1_kernel<TB, KB, NW>, grid, dim3(NW * 64), lds, c.compute, a);
}

}  // namespace

double gauss_taps(double sigma, std::vector<double>* w) {
    const int R = gaussian_radius(sigma);
    if (w) w->resize(2 * R + 1);
    double sum = 0.0;
    for (int k = -R; k <= R; ++k) {
        const double t = std::exp(-0.5 / (sigma * sigma) * (double)k * (double)k);
        if (w) (*w)[k + R] = t;
        sum += t;
    }
    return sum;
}

int gauss_args(const Block& b, float* out, double sigma, int kb, int slot, GaussArgs* a) {
    *a = GaussArgs{};
    a->in = b.in;
    a->out = out;
    a->in_rows = b.in_rows;
    a->in_row0 = b.in_row0;
    a->gny = b.gny;
    a->nx = b.nx;
    a->out_row0 = b.out_row0;
    a->out_rows = b.out_rows;
    return upload_weights(slot, sigma, kb, a);
}

int mfma_min_radius() {
    static const int r = mfma_min_radius_from(env_int("TOPO_AMD_GAUSS_MFMA_MIN_RADIUS", 4));
    return r;
}

// A property of the WHOLE raster (common.hpp RasterClass: its samples are mostly beyond the f16 kernels' range), so that
// every row block of it takes the same kernels.  A/B: tools/large_raster_time.py
bool large_sample_call() {
    static const bool on = env_switch_on("TOPO_AMD_GAUSS_LARGE_SAMPLE");
    return on && current_class().large;
}

int run_axis0(const Block& b, double sigma, float* out, int table_slot, int mfma_from) {
    Context& c = ctx();
    const int R = gaussian_radius(sigma);
    if (mfma_radius(R, b.nx, mfma_from) && mfma_rows_ok(b, R)) return run_axis0_mfma(b, sigma, out, table_slot);
    const int tb = wide_tiling(R) ? 16 : 8;
    t_grad.valu_smooth = true;
    GaussArgs a;
    TOPO_TRY(gauss_args(b, out, sigma, tb, table_slot, &a));
    a.group0 = b.out_row0 / tb;
    const int groups = (b.out_row0 + b.out_rows - 1) / tb - a.group0 + 1;
    dim3 grid((b.nx + kThreads - 1) / kThreads, groups);
    return launch(tb == 16 ? gauss_axis0_kernel<16, 16> : gauss_axis0_kernel<8, 8>, grid, dim3(kThreads), 0, c.compute, a);
}

int run_axis1(const float* in, int rows, int nx, double sigma, float* out, int table_slot, int mfma_from) {
    const int R = gaussian_radius(sigma);
    if (mfma_radius(R, nx, mfma_from)) return run_axis1_mfma(in, rows, nx, sigma, out, table_slot);
    const bool wide = wide_tiling(R);
    t_grad.valu_smooth = true;
    GaussArgs a;
    TOPO_TRY(gauss_args(plane_block(in, rows, nx), out, sigma, wide ? 16 : 8, table_slot, &a));
    if (wide) {
        if (!axis1_tile_fits(a.radius)) {
            // long filter: the wave-shift kernel has no LDS tile
            GradArgs g{};
            g.gny = rows;
            g.nx = nx;
            g.out_rows = rows;
            const int r = run_axis1_wave_grad(in, 0, rows, sigma, g, out);
            if (r != TOPO_AMD_EUNSUP) return r;
            // filter wider than a wavefront can chain: transpose, filter down the columns, transpose back
            Context& c = ctx();
            const size_t bytes = (size_t)rows * nx * sizeof(float);
            void *t1 = nullptr, *t2 = nullptr;
            TOPO_TRY(workspace(6, bytes, &t1));
            TOPO_TRY(workspace(7, bytes, &t2));
            dim3 g1((nx + 31) / 32, (rows + 31) / 32), g2((rows + 31) / 32, (nx + 31) / 32);
            TOPO_TRY(launch(transpose_kernel, g1, dim3(kThreads), 0, c.compute, in, (float*)t1, rows, nx));
            TOPO_TRY(run_axis0(plane_block((const float*)t1, nx, rows), sigma, (float*)t2, table_slot, mfma_from));
            return launch(transpose_kernel, g2, dim3(kThreads), 0, c.compute, (const float*)t2, out, nx, rows);
        }
        return launch_axis1<16, 16, 8>(a, rows, nx, sigma);
    }
    return launch_axis1<8, 8, 8>(a, rows, nx, sigma);
}

int smooth_rows(const Block& src, double sigma_y, double sigma_x, int row0, int rows, float* out, int mfma_from) {
    Context& c = ctx();
    const bool do_y = sigma_y > 1e-15, do_x = sigma_x > 1e-15;
    Block b = src;
    b.out_row0 = row0;
    b.out_rows = rows;
    const size_t bytes = (size_t)rows * src.nx * sizeof(float);
    const float* first = src.in + (size_t)(row0 - src.in_row0) * src.nx;
    if (do_y && do_x) {
        void* tmp = nullptr;
        TOPO_TRY(workspace(0, bytes, &tmp));
        const int R = gaussian_radius(sigma_y);
        if (sigma_y == sigma_x && mfma_radius(R, b.nx, mfma_from) && mfma_rows_ok(b, R)) {
            TOPO_TRY(smooth_both_mfma(b, sigma_y, (float*)tmp, out, 1, false));
        } else {
            TOPO_TRY(run_axis0(b, sigma_y, (float*)tmp, 1, mfma_from));
            TOPO_TRY(run_axis1((const float*)tmp, rows, src.nx, sigma_x, out, 2, mfma_from));
        }
    } else if (do_y) {
        TOPO_TRY(run_axis0(b, sigma_y, out, 1, mfma_from));
    } else if (do_x) {
        TOPO_TRY(run_axis1(first, rows, src.nx, sigma_x, out, 2, mfma_from));
    } else {
        TOPO_HIP(hipMemcpyAsync(out, first, bytes, hipMemcpyDeviceToDevice, c.compute));
    }
    return TOPO_AMD_OK;
}

int gaussian_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

int gauss_ghost_rows(double sigma) { return gauss_ghost_rows_of(gaussian_radius(sigma), mfma_min_radius()); }

int launch_gaussian(const Block& b, double sigma_y, double sigma_x, float* out) {
    const int from = mfma_from(large_sample_call(), true);
    return for_row_slabs(b.out_rows, [&](int r, int n) {
        return smooth_rows(b, sigma_y, sigma_x, b.out_row0 + r, n, out + (size_t)r * b.nx, from);
    });
}

}  // namespace topo
