/*
 * topo_amd.h - C ABI of libtopo_amd.so, the MI355X (gfx950) implementation of the
 * per-pixel descriptor hot path of MeteoSwiss/topo-descriptors.
 *
 * The reference has no FFI of its own (it is pure Python on scipy/numba wheels); the
 * boundary this library replaces is the set of Python call sites listed next to each
 * entry point (file:line into the reference).  INTEGRATION.md shows the ctypes stub a
 * maintainer adds to `topo_descriptors/topo.py` to route those calls here.
 *
 * Conventions
 *   - every function returns 0 on success, a negative TOPO_AMD_E* code otherwise; the
 *     message is available from topo_amd_last_error() (thread-local).
 *   - arrays are C-contiguous float32, ny rows x nx columns, row pitch == nx.
 *   - *_f32 entry points take HOST pointers, do upload -> kernels -> download and return
 *     when the result is in the caller's buffer.  No pointer is retained after return (the
 *     device planes are: topo_amd_release_host_planes).
 *   - *_dev entry points take DEVICE pointers obtained from topo_amd_malloc, enqueue on the
 *     library's compute stream and return immediately; call topo_amd_sync() before reading.
 *   - row-block form: a device block holds `in_rows` consecutive rows of a global
 *     `gny x nx` DEM starting at global row `in_row0`.  Output rows are
 *     [out_row0, out_row0+out_rows) in global numbering and `out` points at the first of
 *     them.  The boundary rule of each descriptor (zero padding, reflection, one-sided
 *     difference, zero frame) is applied at the GLOBAL edges only, so that a row shard
 *     plus its ghost rows gives results bit-identical to the single-block run.  The block
 *     must contain every row the requested output rows depend on (see topo_amd_halo_rows).
 *   - one process drives one GPU (topo_amd_init(device)); entry points are serialised on
 *     that device's compute stream.
 *
 * Threading
 *   Every entry point may be called from any thread at any time.  The context (workspaces, the device planes of the
 *   host-buffer entry points, the streams and events of their pipeline, the gate of a sharded call) is guarded by ONE
 *   mutex that every entry point touching it holds from its first to its last line, so concurrent calls run one after
 *   the other, each exactly as if it were alone - same bits as a serial run.  A host-buffer call (*_f32) holds it until its
 *   result is in the caller's array; a device call (*_dev, topo_amd_shard_*) only while it enqueues, so the GPU work of
 *   several threads queues up back to back on the compute stream (in the order the threads took the mutex).
 *   topo_amd_sync() waits for everything enqueued so far, by whichever thread.  The calling thread is bound to the
 *   context's device on entry (hipSetDevice).  topo_amd_last_error() and topo_amd_shard_layout are per thread; the
 *   stopwatch (topo_amd_timer_*, topo_amd_mark*) is one per process and means what it says only when one thread launches
 *   between its two ends.  Collective calls (topo_amd_shard_*, topo_amd_comm_*) must be issued in the same order on
 *   every rank: drive them from one thread per process.
 */
#ifndef TOPO_AMD_H
#define TOPO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOPO_AMD_OK 0
#define TOPO_AMD_EINVAL (-1)   /* bad argument                                   */
#define TOPO_AMD_EHIP (-2)     /* a HIP runtime call failed                      */
#define TOPO_AMD_ENODEV (-3)   /* no usable GPU / library not initialised        */
#define TOPO_AMD_ERCCL (-4)    /* an RCCL call failed                            */
#define TOPO_AMD_EUNSUP (-5)   /* valid request the kernels do not cover (yet)   */
#define TOPO_AMD_EEMPTY (-6)   /* Sx: a sector has no usable ray pixel; its plane was zero-filled and the
                                  other sectors were computed (nanmax over nothing, topo.py:947-951) */

/* descriptor ids for topo_amd_halo_rows */
#define TOPO_AMD_DESC_TPI 0
#define TOPO_AMD_DESC_STD 1
#define TOPO_AMD_DESC_GAUSS 2
#define TOPO_AMD_DESC_GRADIENT 3
#define TOPO_AMD_DESC_SOBEL 4
#define TOPO_AMD_DESC_SX 5
#define TOPO_AMD_DESC_VALLEY_RIDGE 6 /* p0 = side of the largest rotated kernel */

/* resolution layout for the gradient normalisation (reference topo.py:688-712) */
#define TOPO_AMD_RES_SCALAR 0 /* res_x[0], res_y[0]                                   */
#define TOPO_AMD_RES_1D 1     /* res_x[nx] per column, res_y[gny] per GLOBAL row      */
#define TOPO_AMD_RES_2D 2     /* res_x, res_y: [out_rows x nx] aligned with `out`     */

/* ---- runtime ------------------------------------------------------------------------ */
const char* topo_amd_version(void);
const char* topo_amd_last_error(void);
int topo_amd_device_count(void);
int topo_amd_init(int device);            /* idempotent for the same device           */
int topo_amd_shutdown(void);
int topo_amd_device_name(char* buf, int buflen);
/* Compute units the persistent kernels size their grids for: the device's CU count, or the
 * smaller TOPO_AMD_CU_LIMIT from the environment at init.  Results never depend on it.   */
int topo_amd_cu_count(void);

int topo_amd_malloc(void** dptr, size_t bytes);
int topo_amd_free(void* dptr);
/* Page-locked host memory for arrays handed to the host-buffer entry points (copies at the link's rate). */
int topo_amd_host_alloc(void** hptr, size_t bytes);
int topo_amd_host_free(void* hptr);
int topo_amd_memcpy_h2d(void* dst, const void* src, size_t bytes);
int topo_amd_memcpy_d2h(void* dst, const void* src, size_t bytes);
int topo_amd_memcpy_d2d(void* dst, const void* src, size_t bytes);
int topo_amd_memset(void* dst, int value, size_t bytes);
int topo_amd_sync(void);

/* ---- what kernel routing may know about a raster ------------------------------------------------------------------------
 * Results never depend on how a raster is cut into row blocks or shards, nor on what the library has seen before.  Nearly
 * all kernel choices cannot change a bit (integer sums are exact whoever forms them).  Two can, in the last bits: the
 * Gaussian / gradient of a raster whose ORDINARY values lie beyond 1e5 (a DEM in millimetres) runs on the vector-ALU kernels
 * instead of the f16 matrix-core ones, and TPI alone on fractional elevations (discs from 19 px) sums x in units of 2^-k m
 * with k = 8 ... 16 chosen from the raster's value range.  Both are properties of the WHOLE raster - its "class", read off a
 * lattice of about 16 K samples of the GLOBAL grid (rows / columns step / 2 + i step, step = extent / 128):
 *   - a block that is the whole raster (in_row0 == 0, in_rows == gny) is scanned by the library at the first call that
 *     needs the class and remembered with the buffer until the library writes or frees the buffer - or the caller, having
 *     written it with kernels of its own, says so with topo_amd_dem_changed;
 *   - the host-buffer entry points scan the caller's array;
 *   - a PARTIAL row block uses the class that was declared FOR ITS MEMORY: topo_amd_raster_scan_dev adds up the lattice
 *     points of the rows each block owns (counts += {samples, samples finite and beyond 1e5, samples with a fractional
 *     part}; range = {min, max} of the samples within +-2^18; start from 0, 0, 0 and +inf, -inf), then
 *     topo_amd_raster_class_from_scan(block, in_rows, gny, nx, counts, range) declares the sum for the device rows
 *     [block, block + in_rows * nx) of a gny x nx raster - once per block the application holds (the share of fractional
 *     samples only picks which exact disc kernels run first: time, never bits).  A later call whose `in` pointer lies
 *     inside declared rows of a raster of the same shape takes that class.  Blocks may overlap (views of one buffer, each
 *     with its ghost rows): declarations of the same shape and class keep one entry per block, in any order; one of
 *     another shape or class replaces every declaration it overlaps, one of the same rows replaces their declaration.
 *     A declaration lives exactly as long as the data it describes: it is dropped when the library writes or frees
 *     memory overlapping the rows (uploads, copies, memset, an output plane, topo_amd_free), by topo_amd_dem_changed, or
 *     by topo_amd_raster_class_set(..., large = -1, ...) (block == NULL: every declaration).  It is not a property of a
 *     thread or of the process: two rasters held in one process never see each other's class.
 *   - the topo_amd_shard_* calls declare the class of their shard THEMSELVES at the first call on a buffer nothing is
 *     declared for (topo_amd_shard_classify: the scans of all ranks, added up by an all-reduce - collective like the
 *     calls themselves), so every shard takes the single GPU's kernels without the application doing anything.
 *   - a partial row block of the *_dev entry points that nothing was declared for is taken for an ordinary DEM in whole
 *     metres (large = 0, range 0 ... 4096, no fractional samples): a fixed rule, not a memory of earlier calls.  On such
 *     a raster the blocks give the whole raster's bits; on a raster of another class (fractional elevations within a
 *     few hundred metres, millimetres) they stay inside the tolerances below but may differ from the whole raster in
 *     the last bits of TPI / the Gaussian - declare the class to get its bits.                                           */
int topo_amd_dem_changed(const void* dptr, size_t bytes); /* bytes == 0: the whole allocation dptr lies in */
int topo_amd_raster_scan_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int own_row0, int own_rows,
                             uint64_t counts[3], float range[2]);
int topo_amd_raster_class_from_scan(const float* block, int in_rows, int gny, int nx, const uint64_t counts[3],
                                    const float range[2]);
int topo_amd_raster_class_set(const float* block, int in_rows, int gny, int nx, int large, float lo, float hi,
                              float frac_share);
/* The class a call on a block starting at `block` (any row of declared rows) of a gny x nx raster would take; *declared = 0:
 * nothing is declared there (the values are then the ordinary DEM's).                                                     */
int topo_amd_raster_class_get(const float* block, int gny, int nx, int* declared, int* large, float* lo, float* hi,
                              float* frac_share);

/* HIP-event stopwatch on the compute stream (what bench.py times kernels with). */
int topo_amd_timer_start(void);
int topo_amd_timer_stop(float* elapsed_ms); /* records, synchronises, returns ms        */
/* Numbered HIP events on the compute stream (index 0 .. 511): one per launch boundary gives the
 * duration of every launch of a timed loop without a host synchronise inside the loop (bench.py
 * reports the median next to the mean).  topo_amd_mark_elapsed waits for mark `to`.         */
int topo_amd_mark(int index);
int topo_amd_mark_elapsed(int from, int to, float* elapsed_ms);

/* Deterministic synthetic terrain (float32 metres) written on the device: the value depends
 * only on (global row, column, seed), so shards agree on overlaps.  integer_valued != 0 rounds
 * to whole metres (SRTM/DHM25-like; TPI then takes the one-pass path), 0 keeps the fractional
 * part (swissALTI3D-like; every tile takes the two-pass path).                          */
int topo_amd_synth_dem_dev(float* out, int rows, int row0, int nx, uint32_t seed, int integer_valued);

/* ---- geometry helpers (host) -------------------------------------------------------- */
/* Tap count of the reference's circular_kernel(size) (topo.py:191-213).               */
int topo_amd_disc_tap_count(int size);
/* Writes the size x size 0/1 mask (row-major float32).                                 */
int topo_amd_disc_mask(int size, float* mask);
/* Ghost rows a row block needs above / below its output rows for one descriptor.
 * p0: size (TPI/STD) | sigma (GAUSS: of axis 0; GRADIENT: the `sigma` argument of the gradient)
 * p1: pre-smoothing sigma (TPI/STD/VALLEY_RIDGE, 0 = none) | sig_ratio (GRADIENT; 0 or 1 = isotropic) | unused
 * GRADIENT answers exactly the depth topo_amd_shard_gradient(sigma, sig_ratio) lays its block out with.
 * For SX pass the extremes of the offset table instead: p0 = -min(dj), p1 = max(dj).
 * For Gaussian radii int(4 sigma + 0.5) of 4 ... 15 (the gradient's too; also the pre-smoothing of TPI / STD) the
 * answer is 16 rows (gradient: 17) rather than the radius: the matrix-core kernels used there take a per-tile
 * offset sample 16 rows into their 32-row tiles.  A block with fewer ghost rows (but at least the radius) is still
 * computed correctly, by the vector-ALU kernels; only bit-identity with other partitions is lost.              */
int topo_amd_halo_rows(int descriptor, double p0, double p1, int* above, int* below);

/* ---- descriptors, device row-block form --------------------------------------------- */
/* TPI and/or STD over the reference's disc (replaces topo.tpi topo.py:144-181 and topo.std
 * topo.py:272-307, called from topo.py:138 and :266).  Either output may be NULL.  STD is
 * float32 on the device (the Python wrapper widens to float64 like the reference).       */
/* Arithmetic.  Sums of trunc(x), trunc(x)^2 and of the fractional parts (units of 2^-16 m) are exact integers in every
 * kernel, so the values do not depend on tiles, kernels or row blocks.  A sample that is not finite or beyond +-2^24 is
 * MISSING: exactly the pixels whose disc holds one are NaN.  Samples beyond +-2^18 (a raster in millimetres) and windows
 * with more relief than the 32-bit chains hold (nodata like -9999 next to terrain) take exact multi-limb passes (slower).
 * TPI alone (std_out == NULL), discs of 19 ... 101 px, windows with fractional elevations: the neighbourhood sum is taken
 * on x in units of 2^-k m (one integer chain; csrc/disc_wave_impl.hpp, tpi_scaled_march_kernel), k = 8 for an ordinary DEM
 * (at most 2^-9 m = 1.95 mm off per sample and therefore on TPI), up to 16 for rasters of small values (the raster class,
 * above); an output row whose own window holds more relief than that chain unwraps exactly is computed by the exact
 * general kernel - decided per row on the rows every row block that computes it holds.  Whole-metre DEMs, smaller discs
 * and the fused TPI + STD call are exact to float32 rounding.  TOPO_AMD_TPI_FRACTION_EXACT=1: the exact two-pass route.  */
int topo_amd_tpi_std_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int size,
                         int out_row0, int out_rows, float* tpi_out, float* std_out);

/* Valid-sample TPI / STD: the statistics of the samples that EXIST in the disc (numpy's nanmean / nanstd reading; no
 * reference counterpart - its FFT turns one NaN into a NaN array, and fill_na invents terrain).  Either output may be NULL.
 * Semantics.  The disc D(p) holds exactly the tap offsets topo_amd_tpi_std_dev uses for `size` (topo_amd_disc_mask as
 * scipy.signal.convolve(..., "same") sees it, even sizes and the square below 5 included).  A tap is VALID when it lies
 * inside the gny x nx raster and its sample is not MISSING (not finite, or beyond +-2^24: the definition above); nothing is
 * padded with zeros.  Over the valid taps of a pixel: n their number, s1 = sum x, s2 = sum trunc(x)^2 (the int32-truncation
 * quirk stays: where every tap is valid STD equals topo_amd_tpi_std_dev's); n' and s1' are n and s1 without the tap TPI
 * excludes (kernel[size / 2][size / 2]).
 *     TPI = x(p) - s1' / n'                              NaN where x(p) is missing or n' < max(1, min_count)
 *     STD = sqrt(max(0, (s2 - s1^2 / n) / (n - 1)))      NaN where x(p) is missing or n  < max(2, min_count)
 * Arithmetic.  The sums are exact integers - trunc(x) around an integer tile offset, fractional parts in units of 2^-16 m,
 * the count an integer - and the closing formula is evaluated in float64 on the device and rounded to float32 once, so the
 * bits do not depend on tiles, row blocks or out_row0 / out_rows.  A tile holding a valid sample beyond +-2^18, or more
 * relief around its offset than 32-bit window sums of squares take (6521 m: -9999 left finite next to terrain), is summed
 * tap by tap in 64 bits instead (slower, the same bits; reported by topo_amd_disc_route).
 * Row blocks: ghost rows as topo_amd_halo_rows(TOPO_AMD_DESC_TPI, size, 0) gives them; rows beyond gny are outside the
 * raster.  There is no pre-smoothing in this call: smooth over the gaps with topo_amd_gaussian_valid_dev (the normalised
 * convolution, below) and hand its plane to this one - topo.tpi(topo.dem(d, sigma, skipna=True), size, skipna=True).
 * size 1 ... 101; larger sizes: TOPO_AMD_EUNSUP.  size < 1, min_count < 1 or both outputs NULL: TOPO_AMD_EINVAL.            */
int topo_amd_tpi_std_valid_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int size, int min_count,
                               int out_row0, int out_rows, float* tpi_out, float* std_out);

/* TPI for several disc sizes of one resident block (the scale loop of compute_tpi, reference
 * topo.py:132-141, and of scripts/compute_topo_descriptors.py:25-38): sizes that have a two-disc
 * kernel (pairs out of 5, 7, 9, 11 px) are evaluated two at a time from ONE pass over the DEM,
 * the rest one by one; every plane has the bits of topo_amd_tpi_std_dev for its size.
 * tpi_outs[k] receives the plane of sizes[k] (out_rows x nx each).                         */
int topo_amd_tpi_multi_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int n_sizes,
                           const int32_t* sizes, int out_row0, int out_rows, float* const* tpi_outs);
/* ndimage.gaussian_filter(dem, (sigma_y, sigma_x)), reflect boundary, truncate 4 sigma
 * (replaces topo.dem topo.py:62-80 and the pre-smoothing at topo.py:173, :298).  A sigma of
 * 0 skips that axis.  The intermediate plane lives in the library's own workspace.       */
/* Gaussian / gradient, matrix-core routes (filter radius 4 ... 121): a sample that is not finite, or larger than 1e5 in
 * magnitude (a sentinel like 1e20), is "wild": its outputs are recomputed by slower repair passes with exactly
 * ndimage.gaussian_filter's footprint (a block on which the fused short-filter kernel met one is remembered and takes the
 * two-pass kernels on later calls: the same bits).  A raster whose ORDINARY values lie beyond 1e5 (a DEM in millimetres)
 * runs on the vector-ALU kernels, which have no such limit (8192^2, sigma 3.25 / 13: 0.45 / 0.71 ms against 21.9 / 68.3 ms
 * through the repair passes): a property of the whole raster (the raster class, above), so every row block of it takes
 * the same kernels.  TOPO_AMD_GAUSS_LARGE_SAMPLE=0: always the matrix-core kernels.                                    */
int topo_amd_gaussian_dev(const float* in, int in_rows, int in_row0, int gny, int nx,
                          double sigma_y, double sigma_x, int out_row0, int out_rows,
                          float* out);

/* Valid-sample Gaussian: the normalised convolution of a DEM with gaps (csrc/gauss_valid.hip; no reference counterpart -
 * ndimage.gaussian_filter lets one NaN spoil its whole window, and fill_na invents terrain).
 * Semantics.  m(q) = 1 where sample q is valid, 0 where it is MISSING (not finite, or beyond +-2^24: the definition above, so
 * a 1e20 sentinel is a gap).  w_y, w_x: exactly the taps of topo_amd_gaussian_dev - radius R = int(4 sigma + 0.5), normalised
 * in float64 and rounded to float32; a sigma of 0 or a radius of 0 skips that axis; scipy's "reflect" at the edges of the
 * GLOBAL raster, periodic, and a reflected tap is valid exactly when the sample it lands on is.
 *     D(p) = sum_i sum_j w_y[i] w_x[j] m(q)              q = reflect(p + (i, j))
 *     N(p) = sum_i sum_j w_y[i] w_x[j] m(q) x(q)
 *     out(p) = N(p) / D(p)   where D(p) > 0, D(p) >= min_weight and (fill != 0 or m(p) = 1);   NaN elsewhere
 * With min_weight = 0 and fill = 0 the output is NaN exactly at the missing pixels; with fill != 0 exactly where the reflected
 * (2 R_y + 1) x (2 R_x + 1) window holds no valid sample - a two-dimensional gap interpolator.  weight_out (may be NULL)
 * receives D(p) as float32 at every pixel, 0 where no tap is valid, whatever the NaN rule does to out.  On a gap-free raster D is
 * 1 to rounding and out is topo_amd_gaussian_dev's value to 1e-3 m.
 * Arithmetic.  N and D go through both 1-D passes and the division happens once, behind the second.  Each pass sums
 * w m (x - c) and w m in float64 around an offset c taken on the global grid (N / D = c + sum w m (x - c) / sum w m for any
 * finite c); between the passes N and D are rounded to float32 once each (N around the rounded D), the quotient once at the end.  Every term is
 * bounded by D max|x - c| before the division, so a small D amplifies no rounding.  The bits do not depend on row blocks or
 * out_row0 / out_rows.
 * Row blocks: ghost rows as topo_amd_halo_rows(TOPO_AMD_DESC_GAUSS, sigma_y, 0) gives them (at least R); rows beyond gny do
 * not exist - the filter reflects there.  The result is a plane topo_amd_tpi_std_valid_dev takes as it is: smooth over the
 * gaps, then valid-sample TPI / STD.
 * Radius 0 ... 121 per axis (sigma <= 30.25); beyond: TOPO_AMD_EUNSUP.  min_weight outside [0, 1] or NaN, a negative or NaN
 * sigma, out NULL: TOPO_AMD_EINVAL.                                                                                        */
int topo_amd_gaussian_valid_dev(const float* in, int in_rows, int in_row0, int gny, int nx, double sigma_y, double sigma_x,
                                double min_weight, int fill, int out_row0, int out_rows, float* out,
                                float* weight_out /* may be NULL */);

/* 3x3 Sobel pair / 8, true convolution, reflect (replaces topo.sobel topo.py:658-685).  */
int topo_amd_sobel_dev(const float* in, int in_rows, int in_row0, int gny, int nx,
                       int out_row0, int out_rows, float* dx_out, float* dy_out);

/* [dx, dy, slope, aspect] (replaces topo.gradient topo.py:597-644, called from :583).
 * sigma <= 1 -> Sobel; sig_ratio == 1 -> one isotropic smooth; otherwise the two
 * anisotropic smooths.  res_x / res_y are HOST double arrays for RES_SCALAR / RES_1D and
 * DEVICE float arrays for RES_2D.  Any output may be NULL.                                */
int topo_amd_gradient_dev(const float* in, int in_rows, int in_row0, int gny, int nx,
                          double sigma, double sig_ratio, int res_mode, const void* res_x,
                          const void* res_y, int out_row0, int out_rows, float* dx_out,
                          float* dy_out, float* slope_out, float* aspect_out);

/* Valid-sample gradient: dx, dy, slope and aspect of a DEM with its gaps left open (csrc/gradient.hip, K4v; no reference
 * counterpart - fill_na invents terrain along x, and in the plain call one NaN erases a disc of radius 4 sigma + 1).
 * MISSING as above: not finite, or beyond +-2^24.
 * sigma > 1.  q is topo_amd_gaussian_valid_dev(..., sigma, sigma, min_weight, fill = 1): N / D where D > 0 and D >= min_weight,
 * undefined elsewhere - defined inside gaps wherever the window reaches a valid sample, so a valid pixel on a gap's rim still has
 * both neighbours.  Along an axis, at a pixel where q is defined, the derivative is
 *     (q[+1] - q[-1]) / 2       where both neighbours exist and are defined,
 *     q[+1] - q[0] or q[0] - q[-1]   where only one of them does,
 * and undefined where neither does or q[0] itself is not.  A raster edge is a neighbour that does not exist, so on a gap-free
 * raster this is numpy.gradient of the Gaussian.  sig_ratio != 1: two such planes, dx from q(sigma sig_ratio, sigma) (axis 0,
 * axis 1) and dy from q(sigma, sigma sig_ratio), each with its own D and the same min_weight.
 * sigma <= 1.  The Sobel pair of topo_amd_sobel_dev (kernel / 8, true convolution, reflect at the global edges); dx is defined
 * where all six samples under its non-zero taps are valid (a reflected tap is valid when the sample it lands on is), dy by the
 * same rule with its own six taps; the centre is a tap of neither.  min_weight is accepted and ignored.
 * Both.  All four outputs are NaN at a pixel whose own sample is missing unless fill != 0.  dx, dy, slope and aspect then follow
 * from the arithmetic of topo_amd_gradient_dev (signed resolutions, the three resolution modes, aspect in [0, 360)); slope and
 * aspect are NaN where dx or dy is, and no output is infinite.  Any output may be NULL; leaving one out does not change the others.
 * Row blocks: the wider filter's radius + 1 ghost rows (1 for sigma <= 1), fewer are refused; the Gaussian's offsets sit on the
 * global grid, so the bits do not depend on row blocks or out_row0 / out_rows.  topo_amd_gradient_route reports 5 (6 with
 * sig_ratio != 1 at sigma > 1).
 * A filter radius above 121 (sigma or sigma sig_ratio beyond 30.25): TOPO_AMD_EUNSUP.  A negative or NaN sigma, sig_ratio not
 * positive, min_weight outside [0, 1] or NaN, fewer than 2 samples along an axis at sigma > 1: TOPO_AMD_EINVAL.             */
int topo_amd_gradient_valid_dev(const float* in, int in_rows, int in_row0, int gny, int nx, double sigma, double sig_ratio,
                                double min_weight, int fill, int res_mode, const void* res_x, const void* res_y, int out_row0,
                                int out_rows, float* dx_out, float* dy_out, float* slope_out, float* aspect_out);

/* Sx max-elevation-angle scan (replaces topo._sx_rolling topo.py:928-953, called from :856).
 * dj/di: offsets of the ray pixels relative to the target (host int32, n_off entries,
 * duplicates allowed); dist: metric distance of each (host double, NaN = skip, as left by
 * radius_min at topo.py:845); window: zero-frame width int(W/2); height: topo.py:947.
 * Non-finite samples as in numpy's nanmax over the angles: a NaN ray sample is skipped, whether
 * quiet or signalling; a pixel whose own sample is NaN, or whose ray samples are all NaN, is
 * NaN; +inf on a ray gives 90, and a pixel whose own sample is +inf (or whose ray samples are
 * all -inf) gives -90.                                                                     */
int topo_amd_sx_dev(const float* in, int in_rows, int in_row0, int gny, int nx,
                    const int32_t* dj, const int32_t* di, const double* dist, int n_off,
                    int window, double height, int out_row0, int out_rows, float* out);

/* Sx for n_az azimuth sectors in one pass over the DEM (the reference scans one
 * azimuth per call, topo.py:715-772 / :856, and its users loop).  Sector a owns entries
 * first[a] .. first[a+1]-1 of dj / di / dist (first: host int32, n_az + 1 entries), has the zero
 * frame window[a] and writes the device plane outs[a] (outs: host array of device pointers).
 * Neighbouring sectors overlap: ray pixels shared by several sectors are scanned once.  Every
 * plane has exactly the bits topo_amd_sx_dev gives for that sector alone.  A sector without a
 * usable ray pixel is treated as by topo_amd_sx_dev (plane zero-filled, TOPO_AMD_EEMPTY), but
 * only after the other sectors are done.                                                     */
int topo_amd_sx_multi_dev(const float* in, int in_rows, int in_row0, int gny, int nx, int n_az,
                          const int32_t* first, const int32_t* dj, const int32_t* di,
                          const double* dist, const int32_t* window, double height,
                          int out_row0, int out_rows, float* const* outs);

/* Valley / ridge index (replaces the angle loop of topo.valley_ridge, topo.py:431-447).
 * The host builds the kernels exactly as the reference does (V / U profiles topo.py:456-492,
 * quadratic-spline rotation and re-normalisation :515-525) and hands over, for each of
 * n_angles angles, n_planes (1..TOPO_AMD_VALLEY_MAX_PLANES, one per flat fraction) 2-D kernels
 * of side ksize[a]: the sums of neighbouring kernel planes that the reference's 3-D "same"
 * convolution of the broadcast DEM applies, flipped in both axes so that the device
 * evaluates a correlation.  taps: HOST float32, angle after angle, ksize[a]^2 taps in row-major
 * order, 4 ceil(n_planes / 4) floats per tap: group g holds planes 4g .. 4g+3, unused slots 0
 * (4 floats for up to 4 planes).  The host tables grow with ceil(n_planes / 4): at 1001 px the
 * tables of 3 planes already take ~5.8 GB, those of 5 to 8 planes twice that.  More planes than
 * TOPO_AMD_VALLEY_MAX_PLANES: TOPO_AMD_EINVAL.  angles: HOST float32, the value stored in dir_out for each angle.
 * mean / stdev: the DEM is normalised as (x - mean) / stdev in float32 while it is read
 * (topo.py:427); topo_amd_mean_std_dev computes them for a device-resident DEM.
 * norm_out = max over angles and planes, clipped at 0; dir_out = first angle reaching it.
 * Three evaluations, chosen by the kernel tables alone (never by the data or the block):
 * rotated kernels of up to 25 cells a side run as a dense product on the matrix pipe
 * (split-f16 operands, float32 accumulation: closer to float64 than the float32 chain;
 * TOPO_AMD_VALLEY_MFMA_MAX_KERNEL, 0 = never) - over PAIRS of opposite cells when every
 * table is point-symmetric bit by bit, as the reference's are (rotated kernels of up to 120
 * cells a side: kernels of up to ~85 px; TOPO_AMD_VALLEY_FOLD=0: never), over the cells
 * otherwise (at most 240 cells with taps: up to 13 px); what neither takes tap by tap in
 * float32; of that, rotated kernels of 64 cells a side and more
 * (TOPO_AMD_VALLEY_FFT_MIN_KERNEL), and any too large for that kernel, by FFT like the
 * reference's signal.convolve.  The first two: a pixel whose kernel footprint holds a
 * non-finite sample is evaluated tap by tap in both, row blocks give the single block's bits.
 * FFT: same contract (1e-4 of the range), but a NaN in the block reaches every output and
 * row blocks agree to rounding instead of bit for bit.  More than 4 planes: the first two run
 * the planes in groups of four and merge the groups' unclipped maxima (the larger value, then
 * the earlier angle index), the FFT evaluates all planes in one pass; same contract.         */
#define TOPO_AMD_VALLEY_MAX_PLANES 16
int topo_amd_valley_ridge_dev(const float* in, int in_rows, int in_row0, int gny, int nx,
                              const float* taps, const int32_t* ksize, const float* angles,
                              int n_angles, int n_planes, double mean, double stdev,
                              int out_row0, int out_rows, float* norm_out, float* dir_out);
/* Which evaluation the calling thread's last valley / ridge call took (for tests and diagnostics): 0 tap by tap,
 * 1 matrix pipe, 2 FFT; + 4: the matrix-pipe pass was followed by the tap-by-tap kernel over the tiles in which it met
 * non-finite samples (launched whenever the matrix pipe is used; it returns at once in tiles that are not flagged);
 * + 8: the matrix pipe ran over pairs of opposite cells (point-symmetric tables); + 16: with the pixel operands streamed
 * in chunks (more than 240 pairs: kernels of 19 px and more); + 32: more than 4 planes, run in groups of four through
 * those kernels (the codes of the groups OR-ed; the FFT takes all planes in one pass and reports 2).                    */
int topo_amd_valley_route(int* route);
/* Which kernel the calling thread's last TPI / STD disc call (topo_amd_tpi_std_dev and the calls built on it) finished
 * its whole-metre tiles with (for tests and diagnostics): 1 the wide ring (TPI alone, 67 px, a single block of a
 * whole-metre raster class: csrc/disc_ring_wide_impl.hpp), 0 any other kernel.                                        */
int topo_amd_tpi_route(int* route);
/* Which kernel route the calling thread's last Sx call took (topo_amd_sx_dev, topo_amd_sx_multi_dev and the calls built on
 * them; for tests and diagnostics).  Bits 0 - 2, the scan: 0 chains down the columns, 1 along the rows, 2 along the diagonal
 * (dj + 1, di + 1), 3 along the diagonal (dj + 1, di - 1), 4 the kernel without an LDS tile (sx_global_kernel: a search window
 * too large for LDS; every other bit is 0 then).  + 8: tiles of 64 x 128 pixels with 8 waves (else 64 x 64 with 4).  The chain
 * tables that held at least one chain: + 16 eights, + 32 fours, + 64 twos, + 128 pairs of eights, + 256 pairs of fours, + 512
 * pairs of twos.  Bits 10 - 13: the index of the LDS row stride among the 16 the kernels are built for (67, 71, 75, 81, 89,
 * 97, 105, 113, 129, 145, 161, 177, 193, 209, 225, 257).  + 16384: topo_amd_sx_multi_dev ran at least one group of more than
 * one sector in a single launch of the multi-sector kernel; the other bits are those of the call's last launch (a grouped
 * launch scans down the columns or along the rows, with 4 waves and without pairs).  -1: no usable ray pixel, nothing
 * scanned.                                                                                                               */
int topo_amd_sx_route(int* route);
/* Which kernels the calling thread's last gradient call queued (topo_amd_gradient_dev and the calls built on it; for tests
 * and diagnostics): what the host decided, noted once every launch of the call succeeded.  A call taller than one launch
 * covers reports its last part.
 *   bits 0 - 2   the route: 0 Sobel (sigma <= 1; every other field is 0), 1 Chunked (matrix cores, row chunks with the
 *                epilogue of one next to the smooth of the next), 2 Mfma (matrix cores, one shot), 3 Valu (vector-ALU
 *                kernels), 4 Aniso (sig_ratio != 1: two smooths).
 *   bits 3 - 5   the smooth: 0 none, 1 the fused f16 kernel with the two passes queued behind its flag, 2 the two-pass tile
 *                kernels, 3 two passes with the split-once axis 1, 4 vector-ALU axis 0 (Aniso: vector-ALU passes only;
 *                otherwise the highest of 2 / 3 among its four passes).
 *   bit 6        Aniso: some of its passes ran on the vector ALUs, some on the matrix cores.
 *   bits 7 - 11  the step count of that f16 kernel: 4 / 6 / 8 of the fused kernel, 4 ... 18 of the tile kernels, NK 5 / 7 / 9 of
 *                the split-once axis 1 (0 without matrix-core pass).
 *   bits 12 - 13 the axis-1 finish of the Valu route: 0 none, 1 LDS-tiled axis 1 + epilogue, 2 wave-shift axis 1 +
 *                epilogue, 3 unfused (axis 1 alone, then a stand-alone epilogue).
 *   bit 14       LDS-tiled finish: tap chunks of 16 (KB 16; else 8).    bits 15 - 17: its PF (3, 4 or 5 samples per lane
 *                held for the next tile; 0 without that kernel).
 *   bits 18 - 19 the stand-alone epilogue: 0 none, 1 one pixel a thread (rows under 8 columns), 2 four pixels a thread.
 *   bit 20       an _if epilogue was queued behind a deferred two-pass smooth (it runs only if the fused kernels of the
 *                chunks met a sample that is not a plain finite one).
 *   bit 21       the row chunks were tapered (first and last a quarter of the others).
 *   bits 22 - 28 the number of row chunks (0 unless Chunked).
 * topo_amd_gradient_valid_dev and the calls built on it report route 5, or 6 for sig_ratio != 1 at sigma > 1 (two planes of the
 * valid-sample Gaussian), with every other field 0.                                                                      */
int topo_amd_gradient_route(int* route);
/* Which kernels the calling thread's last TPI / STD disc call queued (topo_amd_tpi_std_dev, topo_amd_tpi_multi_dev and the
 * calls built on them; for tests and diagnostics): what the host decided, noted by the code that decided it once every
 * launch of the call succeeded.  A call taller than one launch covers reports its last part (and bit 23); a multi-size call
 * reports its last launch.  0: no disc call yet.
 *   bits 0 - 2   the launcher: 1 the wave-shift kernels on the block as it is (odd sizes 3 ... 101), 2 the same on a copy
 *                re-pitched to a multiple of 4 columns, 3 the LDS-gather kernel (even sizes, 1, odd sizes on fewer than 4
 *                columns; below 70 px), 4 the prefix planes (from 70 px), 5 the two-disc kernel of topo_amd_tpi_multi_dev.
 *   bit 3        TPI was wanted.        bit 4: STD was wanted.
 *   bits 5 - 8   the first kernel over the whole-metre tiles (launchers 1, 2, 5): 0 none (the general kernel alone over every
 *                tile), 1 tpi_march, 2 the TPI ring (marking), 3 the wide ring, 4 the scaled march taking every tile, 5 the
 *                STD ring, 6 the STD ring with staging waves apart, 4 columns a lane, 7 the same with 8 columns a lane,
 *                8 the marching sums of the three-pass route, 9 the TPI ring of two discs.
 *   bit 9        std_march followed.
 *   bits 10 - 12 the second pass over the tiles with fractional samples: 0 none, 1 fraction_march, 2 the TPI ring with two
 *                images, 3 the STD ring with three images, 4 the same with staging waves apart.
 *   bit 13       scaled_march followed.        bit 14: the general kernel followed over the tiles left marked.
 *   bits 16 - 22 the tile height of the first kernel (launcher 3: of the gather kernel; launcher 4: 0).
 *   bit 23       the call was split by rows (more rows than one launch covers).
 *   bit 24       the value of topo_amd_tpi_route.
 *   bit 25       launcher 4: the float64 planes (a sample that is not finite or beyond +-65536).
 *   bit 26       launcher 4: the narrow planes' kernel with the plane of fractional parts.
 * The valid-sample calls (topo_amd_tpi_std_valid_dev / _raw / _packed) report launcher 6 in bits 0 - 2 (csrc/disc_valid.hip),
 * bits 3 / 4, the tile height in bits 16 - 22, bit 23, and
 *   bit 27       at least one tile of the call took the exact slow form (tap by tap, 64-bit sums).  This bit is the
 *                kernels' word: topo_amd_disc_route waits for the compute stream to read it.                              */
int topo_amd_disc_route(int* route);
/* Mean and population standard deviation (numpy's default ddof = 0) of count device floats,
 * accumulated in float64.                                                                */
int topo_amd_mean_std_dev(const float* in, size_t count, double* mean, double* stdev);
/* The same two numbers with the BITS numpy's own float32 a.mean() / a.std() give for a C-contiguous float32 array of count
 * samples (csrc/moments_np.hip) - what the reference standardises the DEM with (topo.py:427); near-tied directions of the
 * valley / ridge index flip on their last digit, so the float64 moments above are not a substitute.  numpy's order: chunks
 * of `chunk` samples (np.getbufsize(); 8192 by default) each reduced by its pairwise sum (leaves of 128 samples on eight
 * accumulators, neighbours combined level by level), the chunk sums added one after the other from 0.0f, a partial last
 * chunk the same way; mean = sum / (float)count; std = sqrtf(sum((a - mean) * (a - mean)) / (float)count), the difference
 * and the product each rounded to float32, summed in that order.  The sums of the full chunks are formed on the GPU, the
 * chain over them and the tail on the host; the call returns when both numbers are there.  chunk: a power of two >= 128,
 * anything else is TOPO_AMD_EINVAL; count >= 1.  Non-finite samples give what IEEE arithmetic gives in that order (a NaN
 * result is a NaN; its payload is not specified).                                                                       */
int topo_amd_mean_std_f32_dev(const float* in, size_t count, size_t chunk, float* mean, float* stdev);
/* topo_amd_valley_ridge_dev on a device block that is the WHOLE raster [ny x nx], standardised with the moments
 * topo_amd_mean_std_f32_dev forms of it; moments_out (may be NULL): {mean, std}.                                        */
int topo_amd_valley_ridge_std_dev(const float* in, int ny, int nx, const float* taps, const int32_t* ksize,
                                  const float* angles, int n_angles, int n_planes, size_t chunk, float* norm_out,
                                  float* dir_out, float moments_out[2]);
/* What the calling thread's last valley / ridge call did about the moments (for tests and diagnostics): 0 taken from the
 * caller (topo_amd_valley_ridge_dev / _f32 / _raw), 1 formed on the device in numpy's order (topo_amd_valley_ridge_std_dev
 * / _std_raw / _packed), 2 the float64 all-reduce of a sharded call, 3 numpy's order across the shards
 * (topo_amd_shard_valley_ridge_std).  topo_amd_valley_route is not touched by this.                                      */
int topo_amd_valley_moments_route(int* route);

/* Gaps of a DEM filled with the nearest valid sample along x: replaces hlp.fill_na(dem_ds) (reference helpers.py:137-154,
 * interpolate_na(dim="x", method="nearest", fill_value="extrapolate")) together with the masking at or below
 * CFG.min_elevation of get_dem_netcdf (helpers.py:30-31).  A sample is MISSING when it is NaN or, with a threshold
 * (min_elevation not NaN), when !(x > (float)min_elevation) in float32; +-inf and -0.0 are otherwise valid and copied bit for
 * bit.  Per row, a missing sample takes the valid sample L or R on either side with the smaller coordinate when
 * x[j] <= x_lo / 2 + x_hi / 2 (float64; scipy's interp1d "nearest", a tie goes to the smaller coordinate), the edge sample
 * beyond the first / last valid one.  A row with fewer than two valid samples is left alone: without a threshold its NaNs
 * keep their bits, with one every missing sample of it becomes 0x7FC00000 (numpy's NaN, as np.where(x > m, x, nan) writes).
 * x_coords: HOST double[nx], finite and strictly monotonic (either direction), or NULL for the column index; anything else
 * is TOPO_AMD_EINVAL.  out may be the block's own output rows (in place: only missing samples are written, only valid
 * ones read); missing_out (uint8 [out_rows x nx], 1 = missing before the fill) may be NULL.  Rows are independent: no
 * ghost rows, a row shard fills its own rows with this call.  Writing the rows drops the raster class remembered or
 * declared for them (above).                                                                                           */
int topo_amd_fill_na_dev(const float* in, int in_rows, int in_row0, int gny, int nx, const double* x_coords,
                         double min_elevation, int out_row0, int out_rows, float* out, uint8_t* missing_out);

/* ---- descriptors, host-buffer form (single block, whole DEM) -------------------------- */
/* Upload, kernels and download run in row chunks on three streams (upload || kernels || download: row blocks give the
 * single block's bits), page-locked arrays (topo_amd_host_alloc) and pageable ones alike.  The device planes a call needs
 * are kept for the next call (grow-only); topo_amd_release_host_planes() gives them back to the device.                  */
int topo_amd_release_host_planes(void);
/* Row chunks the calling thread's last host-buffer call ran in (1: upload, kernels, download one after the other - arrays
 * of fewer than three chunks, or TOPO_AMD_HOST_PIPELINE=0; a multi-scale call: the most any scale ran in).  For tests and
 * diagnostics: which branch of the pipeline a call took.  Environment, read at every call: TOPO_AMD_HOST_CHUNK_MB (64; a
 * chunk is whole multiples of 960 rows, at least 960; the last one takes the rest: half a chunk to a chunk and a half),
 * TOPO_AMD_HOST_PIPELINE=0 (off), TOPO_AMD_HOST_DOWNLOADS=thread|inline
 * (who issues the downloads; default: the calling thread when every array is page-locked, a second thread otherwise).
 * topo_amd_valley_ridge_f32 is not pipelined (always one chunk).                                                         */
int topo_amd_host_chunks(int* chunks);
int topo_amd_tpi_f32(const float* dem, int ny, int nx, int size, double sigma, float* out);
int topo_amd_std_f32(const float* dem, int ny, int nx, int size, double sigma, float* out);
int topo_amd_tpi_std_f32(const float* dem, int ny, int nx, int size, double sigma,
                         float* tpi_out, float* std_out);
/* Several scales of TPI and / or STD from ONE upload of the DEM (the loop over scales of the reference's
 * compute_tpi / compute_std, topo.py:88-141 and :216-269, which calls tpi / std once per scale): sizes[k],
 * sigmas[k] (0 = no pre-smoothing) -> tpi_outs[k], std_outs[k], each a host plane [ny x nx] or NULL (either
 * array of planes may itself be NULL).  Plane k has the bits of topo_amd_tpi_std_f32(sizes[k], sigmas[k]);
 * the call moves (1 + planes) x ny x nx x 4 bytes over PCIe instead of (scales + planes) x that.          */
int topo_amd_tpi_std_multi_f32(const float* dem, int ny, int nx, int n_scales, const int32_t* sizes,
                               const double* sigmas, float* const* tpi_outs, float* const* std_outs);
int topo_amd_gauss_f32(const float* dem, int ny, int nx, double sigma_y, double sigma_x,
                       float* out);
int topo_amd_sobel_f32(const float* dem, int ny, int nx, float* dx_out, float* dy_out);
/* topo_amd_fill_na_dev on a host array (pipelined like the others; out may be dem; missing_out: uint8 [ny x nx] or NULL). */
int topo_amd_fill_na_f32(const float* dem, int ny, int nx, const double* x_coords, double min_elevation, float* out,
                         uint8_t* missing_out);
/* res_mode RES_2D here takes HOST float arrays [ny x nx].                                 */
int topo_amd_gradient_f32(const float* dem, int ny, int nx, double sigma, double sig_ratio,
                          int res_mode, const void* res_x, const void* res_y, float* dx_out,
                          float* dy_out, float* slope_out, float* aspect_out);
int topo_amd_sx_f32(const float* dem, int ny, int nx, const int32_t* dj, const int32_t* di,
                    const double* dist, int n_off, int window, double height, float* out);
/* outs: host array of n_az HOST planes [ny x nx].                                          */
int topo_amd_sx_multi_f32(const float* dem, int ny, int nx, int n_az, const int32_t* first,
                          const int32_t* dj, const int32_t* di, const double* dist,
                          const int32_t* window, double height, float* const* outs);
int topo_amd_valley_ridge_f32(const float* dem, int ny, int nx, const float* taps,
                              const int32_t* ksize, const float* angles, int n_angles,
                              int n_planes, double mean, double stdev, float* norm_out,
                              float* dir_out);

/* ---- raw sources: a DEM uploaded as it is stored, decoded on the GPU ------------------------------------------------------
 * SRTM and most GeoTIFF tiles are int16 with a nodata value, CF-packed netCDF is int16 / int32 with scale_factor,
 * add_offset and _FillValue, xarray hands out float64.  A topo_amd_raster describes such an array; the *_raw entry points
 * upload its bytes as they are and decode them to the float32 plane the kernels read, on the GPU, behind each row chunk's
 * copy (csrc/decode.hip).  The decode, for a sample `raw` of the source type:
 *
 *     value = NaN                                       if has_nodata and (double)raw == nodata
 *     value = (float) ( (double)raw * scale + offset )  otherwise
 *
 * The product and the sum are each rounded in float64 (never contracted into an FMA), the result is rounded to
 * nearest-even to float32; NaN is 0x7FC00000.  With scale 1, offset 0 and no nodata this is numpy's astype(float32).  For
 * float64 sources a NaN nodata means "none".  A nodata the source type cannot hold never matches.  A float32 source with
 * scale 1, offset 0 and no nodata is passed through untouched (a copy: no decode runs, every bit is kept): the *_f32
 * entry points are the *_raw ones called with such a source.  scale must be finite and not 0, offset finite, dtype one of
 * the six below: anything else is TOPO_AMD_EINVAL.
 * Every result is, bit for bit, that of the *_f32 call on the array topo_amd_decode_host gives: the raster class (above)
 * is read off the decoded samples of the caller's array, chunks are cut by the float32 rows.                             */
#define TOPO_AMD_F32 0
#define TOPO_AMD_I16 1
#define TOPO_AMD_U16 2
#define TOPO_AMD_I32 3
#define TOPO_AMD_U8 4
#define TOPO_AMD_F64 5
typedef struct topo_amd_raster {
    const void* data; /* ny x nx samples of `dtype`, C-contiguous, native byte order */
    int32_t dtype;    /* TOPO_AMD_F32 ... TOPO_AMD_F64 */
    int32_t has_nodata;
    double scale, offset, nodata;
} topo_amd_raster;
/* The formula above on the host, one thread: count samples of src->data -> out.  Needs no GPU and no topo_amd_init.      */
int topo_amd_decode_host(const topo_amd_raster* src, size_t count, float* out);
/* The same on the device, enqueued on the compute stream: count samples at raw_dev (aligned to the sample type) -> out_dev
 * (any float-aligned address; 16-byte accesses where the two share a 16-byte phase, sample by sample otherwise).  Row
 * shards hold device-resident blocks: they decode with this call.                                                        */
int topo_amd_decode_dev(const void* raw_dev, int dtype, size_t count, double scale, double offset, int has_nodata,
                        double nodata, float* out_dev);
/* A host raster -> a float32 device plane [ny x nx]: uploaded in row chunks, each decoded while the next one is copied.
 * Returns when the plane is complete (the source array is not retained).                                                 */
int topo_amd_upload_raw(const topo_amd_raster* src, int ny, int nx, float* out_dev);
/* The host-buffer entry points on a raw source: as their *_f32 namesakes with `src` in place of `dem`.                   */
int topo_amd_tpi_raw(const topo_amd_raster* src, int ny, int nx, int size, double sigma, float* out);
int topo_amd_std_raw(const topo_amd_raster* src, int ny, int nx, int size, double sigma, float* out);
int topo_amd_tpi_std_raw(const topo_amd_raster* src, int ny, int nx, int size, double sigma, float* tpi_out, float* std_out);
int topo_amd_tpi_std_multi_raw(const topo_amd_raster* src, int ny, int nx, int n_scales, const int32_t* sizes,
                               const double* sigmas, float* const* tpi_outs, float* const* std_outs);
/* topo_amd_tpi_std_valid_dev on a host raster, through the upload / decode / row-chunk pipeline of topo_amd_tpi_std_raw: a
 * declared nodata is NaN behind the decode, hence missing.  Either output may be NULL.                                     */
int topo_amd_tpi_std_valid_raw(const topo_amd_raster* src, int ny, int nx, int size, int min_count, float* tpi_out,
                               float* std_out);
int topo_amd_gauss_raw(const topo_amd_raster* src, int ny, int nx, double sigma_y, double sigma_x, float* out);
/* topo_amd_gaussian_valid_dev (its semantics: D, N, out = N / D under min_weight and fill, weight_out = D or NULL) on a host
 * raster, through the upload / decode / row-chunk pipeline of topo_amd_gauss_raw: a declared nodata is NaN behind the decode,
 * hence a gap.  Errors as for the device call.                                                                            */
int topo_amd_gauss_valid_raw(const topo_amd_raster* src, int ny, int nx, double sigma_y, double sigma_x, double min_weight,
                             int fill, float* out, float* weight_out);
int topo_amd_sobel_raw(const topo_amd_raster* src, int ny, int nx, float* dx_out, float* dy_out);
int topo_amd_fill_na_raw(const topo_amd_raster* src, int ny, int nx, const double* x_coords, double min_elevation, float* out,
                         uint8_t* missing_out);
int topo_amd_gradient_raw(const topo_amd_raster* src, int ny, int nx, double sigma, double sig_ratio, int res_mode,
                          const void* res_x, const void* res_y, float* dx_out, float* dy_out, float* slope_out,
                          float* aspect_out);
/* topo_amd_gradient_valid_dev on a host raster, through the upload / decode / row-chunk pipeline of topo_amd_gradient_raw: a
 * declared nodata is NaN behind the decode, hence a gap.  Errors as for the device call.                                   */
int topo_amd_gradient_valid_raw(const topo_amd_raster* src, int ny, int nx, double sigma, double sig_ratio, double min_weight,
                                int fill, int res_mode, const void* res_x, const void* res_y, float* dx_out, float* dy_out,
                                float* slope_out, float* aspect_out);
int topo_amd_sx_raw(const topo_amd_raster* src, int ny, int nx, const int32_t* dj, const int32_t* di, const double* dist,
                    int n_off, int window, double height, float* out);
int topo_amd_sx_multi_raw(const topo_amd_raster* src, int ny, int nx, int n_az, const int32_t* first, const int32_t* dj,
                          const int32_t* di, const double* dist, const int32_t* window, double height, float* const* outs);
int topo_amd_valley_ridge_raw(const topo_amd_raster* src, int ny, int nx, const float* taps, const int32_t* ksize,
                              const float* angles, int n_angles, int n_planes, double mean, double stdev, float* norm_out,
                              float* dir_out);
/* The standardised index of a host raster in one call: `src` is uploaded and decoded once, smoothed on the device when
 * sigma > 0 (the kernels topo_amd_gauss_raw runs on it: the bits of that call), the moments of that field are taken by
 * topo_amd_mean_std_f32_dev (chunk: see there) and written to moments_out (may be NULL), and the index of
 * topo_amd_valley_ridge_dev is downloaded.  Bit for bit topo_amd_valley_ridge_raw of the (smoothed) float32 array with
 * numpy's float32 mean() / std() of it.  One chunk, like topo_amd_valley_ridge_raw.                                      */
int topo_amd_valley_ridge_std_raw(const topo_amd_raster* src, int ny, int nx, const float* taps, const int32_t* ksize,
                                  const float* angles, int n_angles, int n_planes, double sigma, size_t chunk,
                                  float* norm_out, float* dir_out, float moments_out[2]);

/* ---- packed result planes: a result encoded on the GPU, downloaded as the file will store it -----------------------------
 * The users' files hold these quantities packed - CF scale_factor / add_offset / _FillValue in netCDF, int16 in GeoTIFF -
 * and a host-buffer call is bound by the link: a topo_amd_plane describes a result array of 1 or 2 bytes a sample, and the
 * *_packed entry points encode each row chunk of the float32 device plane behind its kernels (csrc/encode.hip) and download
 * the packed rows.  The encode of a float32 sample v into an integer type T, [lo, hi] being T's range without `nodata`:
 *
 *     code = nodata                                  if v is NaN                      (counted in `missing`)
 *     q    = rint( ((double)v - offset) / scale )    otherwise
 *     code = lo if q < lo, hi if q > hi              (+-inf included; counted in `saturated`)
 *     code = (T) q                                   otherwise
 *
 * The difference and the quotient are each rounded in float64 (a true division, no reciprocal), rint rounds to
 * nearest-even.  has_nodata is required and nodata must be T's lowest or highest code (-32768 or 32767, 0 or 65535, 0 or
 * 255), so no value is ever stored as the nodata code: decode(encode(v)) is NaN exactly where v is NaN.  scale finite and
 * not 0, offset finite.
 * TOPO_AMD_F16: IEEE binary16, round to nearest-even; scale 1, offset 0, no nodata; NaN is stored as 0x7E00 (counted in
 * `missing`), a finite sample that becomes +-inf is counted in `saturated`.  A code for result planes only: as a source
 * dtype it is TOPO_AMD_EINVAL.
 * TOPO_AMD_F32: scale 1, offset 0, no nodata; the plane is passed through - no encode runs, no extra device plane is
 * taken, both counters are 0.  The *_raw entry points are the *_packed ones called with such planes.
 * Anything else (I32, F64, an unknown dtype, a nodata inside the range) is TOPO_AMD_EINVAL.
 * Sobel and fill_na stay float32-only.  The valley / ridge index is packed by topo_amd_valley_ridge_packed (one chunk by
 * design: both planes are encoded behind the index and then downloaded); its direction plane holds whole degrees
 * 0 ... 179, which uint8 with scale 1 stores exactly.  Row shards encode their device planes with topo_amd_encode_dev.   */
#define TOPO_AMD_F16 6
typedef struct topo_amd_plane {
    void* data;         /* host, ny x nx samples of dtype, C-contiguous; NULL where the _raw namesake allows NULL */
    int32_t dtype;      /* TOPO_AMD_F32, _I16, _U16, _U8, _F16 */
    int32_t has_nodata;
    double scale, offset, nodata;
    uint64_t missing;   /* out: samples stored as nodata / NaN */
    uint64_t saturated; /* out: samples clamped (integer types) or overflowed to inf (F16) */
} topo_amd_plane;
/* The formula above on the host, one thread: count floats at `in` -> plane->data.  Needs no GPU and no topo_amd_init.    */
int topo_amd_encode_host(const float* in, size_t count, topo_amd_plane* plane);
/* The same on the device: plane->data is a DEVICE address aligned to the sample type (16-byte accesses where it shares a
 * 16-byte phase with in_dev, sample by sample otherwise).  Enqueued on the compute stream; the call returns when the
 * counters are valid (it waits for the stream).                                                                          */
int topo_amd_encode_dev(const float* in_dev, size_t count, topo_amd_plane* plane);
/* The finishing step of a wrapper call on the device (csrc/finish.hip): the window [row0, row0 + rows) x [col0, col0 + cols)
 * of the float32 device plane in_dev (ny x nx), with NaN put back where the uint8 device plane mask_dev (ny x nx; or NULL)
 * is not 0, stored compactly.  plane->data is a DEVICE address of rows x cols C-contiguous samples of plane->dtype, aligned
 * to the sample type.  For window sample (r, c) and the source index i = (row0 + r) * nx + col0 + c: the sample is NaN if
 * mask_dev is given and mask_dev[i] != 0 (float32 bits 0x7FC00000), in_dev[i] otherwise, and is then encoded exactly as
 * topo_amd_encode_dev encodes it.  TOPO_AMD_F32 is a real case here - the masked window copy, every unmasked sample bit
 * for bit, a NaN's payload included; for the other types no float32 copy of the window is made.  `missing` counts the
 * window samples stored as nodata / NaN (for TOPO_AMD_F32 too; masked samples and samples that were NaN already),
 * `saturated` is topo_amd_encode_dev's.  Enqueued on the compute stream; the call returns when the counters are valid.
 * rows == 0 or cols == 0: TOPO_AMD_OK, nothing is launched, both counters 0.  A window that is not inside the plane, a
 * negative extent or a misaligned plane->data: TOPO_AMD_EINVAL.  Nothing outside the ny x nx samples of in_dev and
 * mask_dev is read and nothing outside the rows x cols samples of plane->data is written.                               */
int topo_amd_finish_dev(const float* in_dev, int ny, int nx, const uint8_t* mask_dev, int row0, int rows, int col0, int cols,
                        topo_amd_plane* plane);
/* The host-buffer entry points with packed result planes: as their *_raw namesakes with a topo_amd_plane in place of every
 * float* (NULL, or a plane whose data is NULL, where the namesake allows NULL) and an array of n planes in place of every
 * float* const*.  Every plane is, bit for bit, topo_amd_encode_host of the float32 plane the *_raw call gives; the counters
 * of each plane are written when the call returns.                                                                       */
int topo_amd_tpi_std_packed(const topo_amd_raster* src, int ny, int nx, int size, double sigma, topo_amd_plane* tpi_out,
                            topo_amd_plane* std_out);
int topo_amd_tpi_std_multi_packed(const topo_amd_raster* src, int ny, int nx, int n_scales, const int32_t* sizes,
                                  const double* sigmas, topo_amd_plane* tpi_outs, topo_amd_plane* std_outs);
/* topo_amd_tpi_std_valid_raw with packed result planes: a NaN output (missing centre, too few valid taps) takes the plane's
 * nodata code and is counted in `missing`.                                                                                */
int topo_amd_tpi_std_valid_packed(const topo_amd_raster* src, int ny, int nx, int size, int min_count,
                                  topo_amd_plane* tpi_plane, topo_amd_plane* std_plane);
int topo_amd_gauss_packed(const topo_amd_raster* src, int ny, int nx, double sigma_y, double sigma_x, topo_amd_plane* out);
/* topo_amd_gauss_valid_raw with a packed result plane: a NaN output (a gap left open: D = 0, D < min_weight, or a missing
 * pixel without fill) takes the plane's nodata code and is counted in `missing`.  weight_out stays float32 (or NULL).       */
int topo_amd_gauss_valid_packed(const topo_amd_raster* src, int ny, int nx, double sigma_y, double sigma_x, double min_weight,
                                int fill, topo_amd_plane* out, float* weight_out);
int topo_amd_gradient_packed(const topo_amd_raster* src, int ny, int nx, double sigma, double sig_ratio, int res_mode,
                             const void* res_x, const void* res_y, topo_amd_plane* dx_out, topo_amd_plane* dy_out,
                             topo_amd_plane* slope_out, topo_amd_plane* aspect_out);
/* topo_amd_gradient_valid_raw with packed result planes: a NaN output (an undefined derivative, a missing pixel without fill)
 * takes the plane's nodata code and is counted in `missing`.                                                                */
int topo_amd_gradient_valid_packed(const topo_amd_raster* src, int ny, int nx, double sigma, double sig_ratio, double min_weight,
                                   int fill, int res_mode, const void* res_x, const void* res_y, topo_amd_plane* dx_out,
                                   topo_amd_plane* dy_out, topo_amd_plane* slope_out, topo_amd_plane* aspect_out);
int topo_amd_sx_packed(const topo_amd_raster* src, int ny, int nx, const int32_t* dj, const int32_t* di, const double* dist,
                       int n_off, int window, double height, topo_amd_plane* out);
int topo_amd_sx_multi_packed(const topo_amd_raster* src, int ny, int nx, int n_az, const int32_t* first, const int32_t* dj,
                             const int32_t* di, const double* dist, const int32_t* window, double height,
                             topo_amd_plane* outs);
/* topo_amd_valley_ridge_std_raw (above) with packed result planes; both planes are required.                            */
int topo_amd_valley_ridge_packed(const topo_amd_raster* src, int ny, int nx, const float* taps, const int32_t* ksize,
                                 const float* angles, int n_angles, int n_planes, double sigma, size_t chunk,
                                 topo_amd_plane* norm_out, topo_amd_plane* dir_out, float moments_out[2]);

/* ---- row sharding over the GPUs of one node (RCCL over xGMI) -------------------------- */
/* The reference's only precedent is dask map_overlap(depth, boundary="none") for TPI
 * (topo.py:177-178): independent blocks plus ghost rows.  Rank r owns a contiguous row
 * block; ghost rows travel with one ncclSend/ncclRecv pair per neighbour.                */
#define TOPO_AMD_UNIQUE_ID_BYTES 128
int topo_amd_comm_unique_id(char id[TOPO_AMD_UNIQUE_ID_BYTES]); /* rank 0, then broadcast */
int topo_amd_comm_init(int rank, int nranks, const char id[TOPO_AMD_UNIQUE_ID_BYTES]);
int topo_amd_comm_rank(void);
int topo_amd_comm_size(void);
int topo_amd_comm_destroy(void);

/* `block` holds [halo_above | rows_local | halo_below] rows of nx floats.  Fills the ghost
 * rows from the neighbours on the communication stream (ranks at the global edge skip the
 * missing side) and records an event; topo_amd_halo_wait() makes the compute stream wait
 * for it.  Every rank must call with the same halo depths.  Requires rows_local >= both.  */
/* Loop-back mode (environment TOPO_AMD_HALO_LOOPBACK=1, communicator of ONE rank): the same
 * ncclSend / ncclRecv pairs are issued to rank 0 itself, with periodic wrap - the block's last
 * halo_above rows land in its top ghost rows, its first halo_below rows in its bottom ghost
 * rows - so that pointer offsets, counts, stream ordering and the CU reservation of the
 * exchange run on a single GPU (tests/test_gpu_halo_loopback.py).                          */
int topo_amd_halo_exchange_start(float* block, int rows_local, int nx, int halo_above,
                                 int halo_below);
int topo_amd_halo_wait(void);
/* Collective: the class of the WHOLE sharded raster (above), declared for this rank's owned rows.  owned: the first row this
 * rank owns (device pointer), rows_local of them starting at global row row0.  The topo_amd_shard_* calls run it themselves
 * when nothing is declared for the shard (first call, or after the shard's rows were rewritten through the library); calling
 * it is only needed after the application rewrote the rows with kernels of its own (or use topo_amd_dem_changed).  Refused
 * when the shard is part of a raster and no communicator exists.  In loop-back mode the rank's rows are scanned at every
 * placement of the periodic stack they stand for.                                                                        */
int topo_amd_shard_classify(const float* owned, int rows_local, int row0, int gny, int nx);
/* Round 4: a sharded call is ONE launch per kernel - the interior rows, then, behind a device-side gate the
 * communication stream opens when the ghost rows have landed, the seam rows - with a clean-up launch behind the
 * exchange's event for blocks that found the gate closed for longer than TOPO_AMD_GATE_WAIT_US (100).  Reads and
 * resets the number of such blocks since the last call: 0 when the exchange hid behind the interior rows.      */
int topo_amd_gate_giveups(unsigned* count);
/* Declares the ghost depth the shard buffers handed to topo_amd_shard_* are laid out with:
 * [halo_above | rows_local | halo_below] rows.  A descriptor that needs fewer ghost rows uses
 * the ones next to the owned rows; one that needs more is refused (TOPO_AMD_EINVAL) instead of
 * reading the owned rows from the wrong offset and receiving past the end of the buffer.
 * -1 / -1 (the default): the buffer has exactly the depth topo_amd_halo_rows gives for the
 * descriptor of each call.  The declaration belongs to the CALLING THREAD (thread-local), so
 * concurrent drivers of differently laid-out shards do not disturb each other; a thread that
 * has never declared one uses the last layout any thread declared (set up once, drive from
 * worker threads).  topo_amd_shard_layout_get reads back what applies to the calling thread
 * (to save and restore around a call).                                                      */
int topo_amd_shard_layout(int halo_above, int halo_below);
int topo_amd_shard_layout_get(int* halo_above, int* halo_below);

/* Sharded TPI/STD step: ghost exchange overlapped with the interior rows, then the two
 * seam strips.  `block` as above with halo_above == halo_below == topo_amd_halo_rows(TPI).
 * row0 = global index of the first local row.  Outputs are rows_local x nx.               */
int topo_amd_shard_tpi_std(float* block, int rows_local, int row0, int gny, int nx, int size,
                           float* tpi_out, float* std_out);
int topo_amd_shard_gradient(float* block, int rows_local, int row0, int gny, int nx,
                            double sigma, double sig_ratio, int res_mode, const void* res_x,
                            const void* res_y, float* dx_out, float* dy_out, float* slope_out,
                            float* aspect_out);
int topo_amd_shard_sx(float* block, int rows_local, int row0, int gny, int nx,
                      const int32_t* dj, const int32_t* di, const double* dist, int n_off,
                      int window, double height, float* out);
/* halo_above / halo_below: the largest -dj / dj over the usable ray pixels of all sectors;
 * one ghost-row exchange serves every sector.                                               */
int topo_amd_shard_sx_multi(float* block, int rows_local, int row0, int gny, int nx, int n_az,
                            const int32_t* first, const int32_t* dj, const int32_t* di,
                            const double* dist, const int32_t* window, double height,
                            float* const* outs);
/* Sharded valley / ridge index: `block` as above with halo_above / halo_below =
 * topo_amd_halo_rows(VALLEY_RIDGE, largest kernel side).  The mean and standard deviation of
 * the whole DEM come from float64 moments of the owned rows and one ncclAllReduce (the only
 * true collective on the path; exact, hence the same for every sharding, on a DEM of whole
 * metres).  That is route 2 of topo_amd_valley_moments_route, and so is _smoothed below.
 * Route 3, topo_amd_shard_valley_ridge_std: the moments are numpy's own float32 mean() /
 * std() of the WHOLE raster (topo_amd_shard_mean_std_f32), bit for bit and for every sharding
 * and every DEM - so a sharded index is the single GPU's topo_amd_valley_ridge_std_dev on the
 * owned rows, near-tied directions included.                                                */
int topo_amd_shard_valley_ridge(float* block, int rows_local, int row0, int gny, int nx,
                                const float* taps, const int32_t* ksize, const float* angles,
                                int n_angles, int n_planes, float* norm_out, float* dir_out);

/* ---- the smoothed descriptors and the gap fill on a row shard ------------------------------------------------------------
 * The Gaussian (topo.dem), the pre-smoothed TPI / STD and valley / ridge index (topo.py:172-173, :297-298, :424-427) and
 * fill_na (helpers.py:137-154), each with the single GPU's bits on the shard's rows (the valley: given the same moments).
 * Every call is collective like the ones above: all ranks make it, in the same order, with the same parameters.
 *
 * Smoothed descriptors: ONE exchange of raw ghost rows, of depth disc / valley reach + gauss_ghost rows (topo_amd_halo_rows
 * of TPI / STD with p1 = sigma, of VALLEY_RIDGE with p1 = sigma).  The shard smooths every row its disc / kernels will read
 * into a plane of the library's workspace - the rows that need only owned raw rows while the exchange is in flight, the two
 * seam bands behind its event - and runs ONE descriptor launch over its owned rows from that plane (its "ghost rows" were
 * smoothed locally: no second exchange, no gate).
 * Raster class: the Gaussian takes the class of the WHOLE raw raster (declared collectively, as every shard call does), so
 * no shard picks the vector-ALU or the matrix-core kernels from its own rows.  The smoothed field is a raster of its own:
 * as the single GPU's Block(smooth) scans the whole smoothed plane, TPI / STD classify the OWNED smoothed rows of all ranks
 * together (topo_amd_shard_classify: an all-reduce at every call) before the disc launch, so two shardings of a DEM take the
 * same disc kernels.  The valley kernels are chosen by the kernel tables alone, never by the class: no scan there.      */
/* topo.dem on a shard: reflect at global rows 0 and gny - 1 only, 4 sigma truncation, the single call's NaN footprint
 * (as far as any row block with this ghost depth has it: the vector-ALU kernels also carry a non-finite sample through zero
 * taps up to 30 rows past the filter, which a block reads only where it holds the rows).
 * Ghost depth topo_amd_halo_rows(GAUSS, sigma_y); out: rows_local x nx.                                                 */
int topo_amd_shard_gaussian(float* block, int rows_local, int row0, int gny, int nx, double sigma_y, double sigma_x,
                            float* out);
/* ndimage.gaussian_filter(dem, sigma) then TPI / STD of size (either output may be NULL).  Ghost depth
 * topo_amd_halo_rows(TPI, size, sigma).  sigma <= 0: exactly topo_amd_shard_tpi_std.                                    */
int topo_amd_shard_tpi_std_smoothed(float* block, int rows_local, int row0, int gny, int nx, int size, double sigma,
                                    float* tpi_out, float* std_out);
/* topo_amd_shard_valley_ridge on the field smoothed with sigma.  Ghost depth topo_amd_halo_rows(VALLEY_RIDGE, largest
 * kernel side, sigma).  The mean and standard deviation are float64 moments of the OWNED SMOOTHED rows, all-reduced;
 * moments_out (host double[2], or NULL) receives the (mean, std) the call standardised with.  sigma <= 0: the result of
 * topo_amd_shard_valley_ridge (and its moments).                                                                         */
int topo_amd_shard_valley_ridge_smoothed(float* block, int rows_local, int row0, int gny, int nx, const float* taps,
                                         const int32_t* ksize, const float* angles, int n_angles, int n_planes,
                                         double sigma, float* norm_out, float* dir_out, double* moments_out);
/* Collective: topo_amd_mean_std_f32_dev of the WHOLE raster [gny x nx] from row shards, bit for bit, on every rank.  owned: the
 * first row this rank owns (device pointer), rows_local of them from global row row0; the ranks' rows must tile the raster
 * (refused otherwise, after the collective, on every rank alike).  numpy's chunks sit at global sample offsets k * chunk: a
 * rank sums the chunks that lie wholly inside its samples on its GPU (the kernel of topo_amd_mean_std_f32_dev, started at its
 * first global chunk boundary) and contributes the samples before / after its first / last boundary as they are.  Per pass
 * (sum; squared deviations) the parts travel in ONE ncclAllReduce over an array whose size follows from (gny, nx, chunk,
 * communicator size) alone - chunk sums indexed by global chunk, then per rank a header and two fragment areas of chunk
 * samples (first pass only) - each word written by one rank and zero elsewhere, summed as unsigned integers: every rank gets
 * every word bit for bit, and runs the same chain over them on its host.  chunk: as topo_amd_mean_std_f32_dev
 * (TOPO_AMD_EINVAL otherwise).  Refused when the shard is part of a raster and no communicator exists.  Loop-back mode: the
 * rank's rows stand at every placement of the periodic stack (gny / rows_local copies; gny % rows_local != 0 is
 * TOPO_AMD_EINVAL), so the call yields the moments of the stacked raster.                                                 */
int topo_amd_shard_mean_std_f32(const float* owned, int rows_local, int row0, int gny, int nx, size_t chunk, float* mean,
                                float* stdev);
/* topo_amd_shard_valley_ridge_smoothed standardised with those moments (route 3): with sigma <= 0 of the owned raw rows,
 * otherwise of the owned SMOOTHED rows in the workspace plane; exchange, ghost depths, layout declaration and kernels are
 * those of the two calls above.  moments_out (host float[2], or NULL): the (mean, std) the call standardised with.  Given the
 * same moments the kernels give the single block's bits on every row block, so this is topo_amd_valley_ridge_std_dev of the
 * whole (smoothed) raster on the owned rows, bit for bit, for every sharding.                                              */
int topo_amd_shard_valley_ridge_std(float* block, int rows_local, int row0, int gny, int nx, const float* taps,
                                    const int32_t* ksize, const float* angles, int n_angles, int n_planes, double sigma,
                                    size_t chunk, float* norm_out, float* dir_out, float moments_out[2]);
/* topo_amd_fill_na_dev on the owned rows: row-local, no exchange, no RCCL call.  out may be the owned rows themselves (in
 * place); missing (uint8 rows_local x nx) may be NULL; x_coords: the WHOLE DEM's, one per column.  An in-place fill drops
 * the raster class declared for the rows it writes, and the next shard call re-classifies - collectively.  So this call is
 * collective by contract: all ranks or none, or the ranks' declared state drifts apart and the next call hangs in the
 * all-reduce one rank skips.                                                                                             */
int topo_amd_shard_fill_na(float* block, int rows_local, int row0, int gny, int nx, const double* x_coords,
                           double min_elevation, float* out, uint8_t* missing);

#ifdef __cplusplus
}
#endif
#endif /* TOPO_AMD_H */
