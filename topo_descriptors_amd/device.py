"""Device-resident DEM blocks: upload once, run many descriptors, download what you need.

Thin Python over the ``*_dev`` entry points of the C ABI (include/topo_amd.h).  This is what
``bench.py`` times (inputs already in HBM) and what the batch wrappers of the reference
(``compute_tpi`` ... topo.py:88-141) would use to keep the DEM on the GPU across scales.
"""
import ctypes as C

import numpy as np

from . import _lib


class DeviceArray:
    """rows x nx plane in HBM owned by libtopo_amd: float32, uint8 for the missing mask of :meth:`Block.fill_na`, or the
    sample types of a packed result plane (int16, uint16, uint8, float16: :meth:`to_packed`)."""

    DTYPES = tuple(np.dtype(t) for t in (np.float32, np.uint8, np.int16, np.uint16, np.float16))

    def __init__(self, rows, nx, dtype=np.float32):
        self.rows, self.nx = int(rows), int(nx)
        self.dtype = np.dtype(dtype)
        if self.dtype not in self.DTYPES:
            raise ValueError(f"DeviceArray: float32, uint8, int16, uint16 or float16 planes, not {self.dtype}")
        self.nbytes = self.rows * self.nx * self.dtype.itemsize
        p = C.c_void_p()
        _lib.check(_lib.lib().topo_amd_malloc(C.byref(p), self.nbytes), "topo_amd_malloc")
        self.ptr = p.value

    @classmethod
    def from_host(cls, array):
        """A float32 plane from an ndarray or ``PackedDem``: supported dtypes are uploaded as stored, in row chunks, and decoded
        on the GPU while the next chunk is copied (``topo_amd_upload_raw``)."""
        a, raster = _lib.source_of(array)
        d = cls(a.shape[0], a.shape[1])
        _lib.check(_lib.lib().topo_amd_upload_raw(C.byref(raster), a.shape[0], a.shape[1], d.ptr), "upload_raw")
        return d

    def row_ptr(self, row):
        return self.ptr + int(row) * self.nx * self.dtype.itemsize

    def to_host(self, row0=0, rows=None):
        rows = self.rows - row0 if rows is None else rows
        out = np.empty((rows, self.nx), dtype=self.dtype)
        _lib.check(_lib.lib().topo_amd_memcpy_d2h(_lib.ptr(out), self.row_ptr(row0), out.nbytes),
                   "memcpy_d2h")
        return out

    def to_packed(self, packing, row0=0, rows=None):
        """Rows of this float32 plane as a ``PackedPlane``: encoded on the GPU into a packed device plane
        (``topo_amd_encode_dev``), which is what crosses the link.  The twin of :meth:`to_host`."""
        if self.dtype != np.float32:
            raise ValueError(f"DeviceArray.to_packed: a float32 plane is encoded, not {self.dtype}")
        rows = self.rows - row0 if rows is None else rows
        dev = DeviceArray(rows, self.nx, dtype=packing.dtype)
        try:
            plane = packing.struct(dev.ptr)
            _lib.check(_lib.lib().topo_amd_encode_dev(self.row_ptr(row0), rows * self.nx, C.byref(plane)), "encode_dev")
            return _lib.PackedPlane(dev.to_host(), packing, plane.missing, plane.saturated)
        finally:
            dev.free()

    def finish(self, packing=None, mask=None, window=None):
        """The last step of a wrapper call, on the GPU (``topo_amd_finish_dev``): the ``window`` ``(row0, rows, col0, cols)`` of
        this float32 plane (``None``: all of it) with NaN where ``mask`` - a uint8 ``DeviceArray`` of this plane's shape, or
        ``None`` - is not 0, as a float32 ndarray or, with a ``packing``, as a ``PackedPlane`` whose counters are those of the
        window.  Only the window crosses the link.  With neither a mask nor a window it is :meth:`to_host` /
        :meth:`to_packed`; an empty window gives a zero-size result without a GPU call."""
        if self.dtype != np.float32:
            raise ValueError(f"DeviceArray.finish: a float32 plane is finished, not {self.dtype}")
        if packing is not None and not isinstance(packing, _lib.Packing):
            raise ValueError(f"DeviceArray.finish: {packing!r} is not a Packing")
        if mask is not None:
            if not isinstance(mask, DeviceArray) or mask.dtype != np.uint8:
                raise ValueError("DeviceArray.finish: the mask is a uint8 DeviceArray")
            if (mask.rows, mask.nx) != (self.rows, self.nx):
                raise ValueError(f"DeviceArray.finish: a {mask.rows} x {mask.nx} mask for a {self.rows} x {self.nx} plane")
        if window is None:
            if mask is None:
                return self.to_host() if packing is None else self.to_packed(packing)
            window = (0, self.rows, 0, self.nx)
        try:
            row0, rows, col0, cols = (int(v) for v in window)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"DeviceArray.finish: window {window!r} is not (row0, rows, col0, cols)") from exc
        if min(row0, rows, col0, cols) < 0 or row0 + rows > self.rows or col0 + cols > self.nx:
            raise ValueError(f"DeviceArray.finish: window rows [{row0}, {row0} + {rows}) x columns [{col0}, {col0} + {cols}) of a "
                             f"{self.rows} x {self.nx} plane")
        stored = _lib.Packing(np.float32) if packing is None else packing
        if rows == 0 or cols == 0:
            values = np.empty((rows, cols), dtype=stored.dtype)
            return values if packing is None else _lib.PackedPlane(values, packing, 0, 0)
        dev = DeviceArray(rows, cols, dtype=stored.dtype)
        try:
            plane = stored.struct(dev.ptr)
            _lib.check(_lib.lib().topo_amd_finish_dev(self.ptr, self.rows, self.nx, None if mask is None else mask.ptr,
                                                      row0, rows, col0, cols, C.byref(plane)), "finish_dev")
            values = dev.to_host()
            return values if packing is None else _lib.PackedPlane(values, packing, plane.missing, plane.saturated)
        finally:
            dev.free()

    def upload_rows(self, array, row0=0):
        a = np.ascontiguousarray(array, dtype=self.dtype)
        _lib.check(_lib.lib().topo_amd_memcpy_h2d(self.row_ptr(row0), _lib.ptr(a), a.nbytes),
                   "memcpy_h2d")

    def free(self):
        if self.ptr:
            _lib.check(_lib.lib().topo_amd_free(self.ptr), "topo_amd_free")
            self.ptr = None

    def __del__(self):  # best effort
        try:
            self.free()
        except Exception:  # noqa: BLE001
            pass


def sync():
    _lib.check(_lib.lib().topo_amd_sync(), "topo_amd_sync")


class RasterScan:
    """The class of a raster that is held as several row blocks (include/topo_amd.h, "what kernel routing may know about
    a raster"): ``add`` the rows each block owns, then ``declare`` it for every block the descriptors will be called on -
    those blocks then take the kernels the whole raster takes.  A declaration belongs to the block's MEMORY (it goes when
    the library writes or frees it), not to a thread.  (A block that is the whole raster needs none of this, and
    ``ShardedDEM`` does it by itself.)"""

    def __init__(self):
        self.counts = (C.c_uint64 * 3)(0, 0, 0)
        self.range = (C.c_float * 2)(np.inf, -np.inf)

    def add(self, block, own_row0=None, own_rows=None):
        """``block``: a :class:`Block`; the rows it OWNS default to all of its rows (give them when blocks overlap)."""
        o0 = block.row0 if own_row0 is None else own_row0
        on = block.rows if own_rows is None else own_rows
        _lib.check(_lib.lib().topo_amd_raster_scan_dev(*block._head(), int(o0), int(on), self.counts, self.range),
                   "raster_scan_dev")
        return self

    def declare(self, *blocks):
        """Declare the class added up so far for the device rows of each :class:`Block` in ``blocks``.  The blocks may
        overlap (views of one buffer with their ghost rows): each keeps its declaration, whatever the order; a later
        declaration of another class or raster shape replaces the declarations it overlaps."""
        if not blocks:
            raise ValueError("RasterScan.declare: name the blocks the class is declared for (it is keyed by their memory)")
        for blk in blocks:
            _lib.check(_lib.lib().topo_amd_raster_class_from_scan(blk.data.row_ptr(blk.first), blk.rows, blk.gny, blk.nx,
                                                                  self.counts, self.range), "raster_class_from_scan")
        return self


def forget_raster_class(block=None):
    """Withdraw what was declared for ``block``'s rows (``None``: every declaration): undeclared partial row blocks are
    ordinary DEMs in whole metres."""
    if block is None:
        _lib.check(_lib.load().topo_amd_raster_class_set(None, 0, 0, 0, -1, 0.0, 0.0, 0.0), "raster_class_set")
    else:
        _lib.check(_lib.load().topo_amd_raster_class_set(block.data.row_ptr(block.first), block.rows, block.gny, block.nx,
                                                         -1, 0.0, 0.0, 0.0), "raster_class_set")


def raster_class(block):
    """``(declared, large, lo, hi, frac_share)`` a call on ``block`` would take (``declared`` False: the ordinary DEM's)."""
    dec, large = C.c_int32(), C.c_int32()
    lo, hi, share = C.c_float(), C.c_float(), C.c_float()
    _lib.check(_lib.lib().topo_amd_raster_class_get(block.data.row_ptr(block.first), block.gny, block.nx, C.byref(dec),
                                                    C.byref(large), C.byref(lo), C.byref(hi), C.byref(share)),
               "raster_class_get")
    return bool(dec.value), bool(large.value), lo.value, hi.value, share.value


def release_host_planes():
    """Give the device planes the host-buffer calls (``topo.tpi(ndarray)`` ...) keep between calls back to the GPU: a
    32768 x 32768 gradient leaves about 20 GiB behind (they are kept because copies out of freshly mapped device memory run
    at half the link's rate)."""
    _lib.check(_lib.lib().topo_amd_release_host_planes(), "release_host_planes")


def host_chunks():
    """Row chunks the calling thread's last host-buffer call ran in (1: the serial order)."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_host_chunks(C.byref(n)), "host_chunks")
    return n.value


def tpi_route():
    """The kernel the calling thread's last TPI / STD disc call took for its whole-metre tiles: 1 the wide ring
    (``csrc/disc_ring_wide_impl.hpp``: TPI alone at 67 px on a single block of a whole-metre raster class), 0 any other."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_tpi_route(C.byref(n)), "tpi_route")
    return n.value


def valley_route():
    """The evaluation the calling thread's last valley / ridge call took: 0 tap by tap (``csrc/valley.hip``), 1 matrix pipe
    (``csrc/valley_mfma.hip``), 2 FFT; + 4 when the tap-by-tap kernel followed the matrix pipe over its flagged tiles; + 8 when the
    matrix pipe ran its folded form (point-symmetric tables: pairs of opposite window cells); + 16 when that form streamed its pixel
    operands (kernels of 19 px and more); + 32 when more than 4 planes ran in groups of four through those kernels (the FFT takes
    all planes in one pass: 2)."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_valley_route(C.byref(n)), "valley_route")
    return n.value


def valley_moments_route():
    """What the calling thread's last valley / ridge call did about the DEM's mean and std: 0 taken from the caller, 1 formed
    on the device in numpy's order (``mean_std_numpy``), 2 the float64 all-reduce of a sharded call, 3 numpy's order across the
    shards (``ShardedDEM.valley_ridge(numpy_moments=True)``)."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_valley_moments_route(C.byref(n)), "valley_moments_route")
    return n.value


def sx_route():
    """The kernel route the calling thread's last Sx call took (``topo_amd_sx_route``): bits 0 - 2 the scan (0 chains down the
    columns, 1 along the rows, 2 / 3 along the diagonals (dj + 1, di + 1) / (dj + 1, di - 1), 4 the kernel without an LDS tile);
    + 8 with 8 waves; + 16 / 32 / 64 chains of 8 / 4 / 2, + 128 / 256 / 512 pairs of them; bits 10 - 13 the index of the LDS
    stride among the 16 the kernels are built for (``include/topo_amd.h``); + 16384 when ``sx_multi`` ran a group of several sectors in one launch (the other bits: the
    call's last launch); -1 without a usable ray pixel."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_sx_route(C.byref(n)), "sx_route")
    return n.value


def gradient_route():
    """The kernels the calling thread's last gradient call queued (``topo_amd_gradient_route``, packed as ``include/topo_amd.h``
    says): bits 0 - 2 the route (0 Sobel, 1 Chunked, 2 Mfma, 3 Valu, 4 Aniso); bits 3 - 5 the smooth (0 none, 1 fused f16 kernel
    with the two passes queued behind its flag, 2 two-pass tile kernels, 3 two passes with split-once axis 1, 4 vector-ALU
    axis 0), bit 6 Aniso with passes on both kinds of kernel, bits 7 - 11 the f16 step count; bits 12 - 13 the axis-1 finish of
    the Valu route (1 LDS-tiled, 2 wave-shift, 3 unfused), bit 14 its tap chunks of 16, bits 15 - 17 its PF; bits 18 - 19 the
    stand-alone epilogue (1 one pixel a thread, 2 four), bit 20 an ``_if`` rerun queued; bit 21 tapered chunks, bits 22 - 28
    the number of row chunks.  A valid-sample call (``skipna=True``, ``Block.gradient_valid``) reports route 5, or 6 with
    ``sig_ratio != 1`` at ``sigma > 1``, and nothing else."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_gradient_route(C.byref(n)), "gradient_route")
    return n.value


def disc_route():
    """The kernels the calling thread's last TPI / STD disc call queued (``topo_amd_disc_route``, packed as ``include/topo_amd.h``
    says): bits 0 - 2 the launcher (1 wave-shift kernels, 2 the same on a re-pitched copy, 3 LDS gather, 4 prefix planes, 5 the
    two-disc kernel), bit 3 / 4 TPI / STD wanted, bits 5 - 8 the first kernel over the whole-metre tiles, bit 9 ``std_march``,
    bits 10 - 12 the second pass over fractional tiles, bit 13 ``scaled_march``, bit 14 the deferred general kernel, bits
    16 - 22 the first kernel's tile height, bit 23 split by rows, bit 24 ``tpi_route()``, bits 25 / 26 the float64 / the
    fractional prefix planes.  A valid-sample call (``skipna=True``, ``Block.tpi_std_valid``) reports launcher 6 with bits
    3 / 4, 16 - 23 and bit 27: a tile took the exact slow form (read from the device: this call then waits for the stream)."""
    n = C.c_int32()
    _lib.check(_lib.lib().topo_amd_disc_route(C.byref(n)), "disc_route")
    return n.value


def dem_changed(array):
    """Tell the library that ``array`` (a :class:`DeviceArray`) was written by something other than the library."""
    _lib.check(_lib.lib().topo_amd_dem_changed(array.ptr, array.nbytes), "dem_changed")


def timer_start():
    _lib.check(_lib.lib().topo_amd_timer_start(), "timer_start")


def timer_stop():
    ms = C.c_float()
    _lib.check(_lib.lib().topo_amd_timer_stop(C.byref(ms)), "timer_stop")
    return ms.value


def mark(index):
    """Record numbered event ``index`` (0 .. 511) on the compute stream."""
    _lib.check(_lib.lib().topo_amd_mark(int(index)), "mark")


def mark_elapsed(a, b):
    """Milliseconds between marks ``a`` and ``b`` (waits for ``b``)."""
    ms = C.c_float()
    _lib.check(_lib.lib().topo_amd_mark_elapsed(int(a), int(b), C.byref(ms)), "mark_elapsed")
    return ms.value


def time_launches(fn, reps, warm=1):
    """Per-launch HIP-event durations (ms) of ``reps`` back-to-back calls of ``fn`` (<= 511), after
    ``warm`` untimed ones: one event between consecutive launches, no host synchronise inside."""
    if not 1 <= reps <= 511:
        raise ValueError(f"time_launches: reps = {reps} outside 1 .. 511 (the library keeps 512 numbered events)")
    for _ in range(warm):
        fn()
    sync()
    mark(0)
    for k in range(reps):
        fn()
        mark(k + 1)
    return [mark_elapsed(k, k + 1) for k in range(reps)]


def synth_dem(rows, nx, row0=0, seed=0, out=None, out_row=0, integer=True):
    """Fill (part of) a DeviceArray with the deterministic synthetic terrain.

    integer=True rounds to whole metres, integer=False keeps fractional elevations."""
    d = out if out is not None else DeviceArray(rows, nx)
    _lib.check(_lib.lib().topo_amd_synth_dem_dev(d.row_ptr(out_row), rows, row0, nx, seed, int(bool(integer))),
               "synth_dem")
    return d


class Block:
    """A device plane seen as rows [row0, row0+rows) of a global gny x nx DEM."""

    def __init__(self, data, row0=0, gny=None, first_buffer_row=0, rows=None):
        self.data = data
        self.first = first_buffer_row
        self.rows = data.rows - first_buffer_row if rows is None else rows
        self.row0 = row0
        self.gny = self.rows if gny is None else gny
        self.nx = data.nx

    def _head(self):
        return (self.data.row_ptr(self.first), self.rows, self.row0, self.gny, self.nx)

    def _range(self, out_row0, out_rows):
        o0 = self.row0 if out_row0 is None else out_row0
        on = (self.row0 + self.rows - o0) if out_rows is None else out_rows
        return o0, on

    def tpi_std(self, size, tpi=None, std=None, out_row0=None, out_rows=None):
        o0, on = self._range(out_row0, out_rows)
        _lib.check(_lib.lib().topo_amd_tpi_std_dev(*self._head(), int(size), o0, on,
                                                   tpi.ptr if tpi else None,
                                                   std.ptr if std else None), "tpi_std_dev")

    def tpi_std_valid(self, size, tpi=None, std=None, min_count=1, out_row0=None, out_rows=None):
        """TPI and / or STD over the samples that exist in the disc (``topo_amd_tpi_std_valid_dev``; ``topo.tpi(skipna=True)``
        for the rules): a missing sample or a tap outside the raster is left out of the sums and of their divisor.  Sizes
        1 ... 101; ghost rows as for :meth:`tpi_std`."""
        o0, on = self._range(out_row0, out_rows)
        _lib.check(_lib.lib().topo_amd_tpi_std_valid_dev(*self._head(), int(size), int(min_count), o0, on,
                                                         tpi.ptr if tpi else None,
                                                         std.ptr if std else None), "tpi_std_valid_dev")

    def tpi_multi(self, sizes, outs, out_row0=None, out_rows=None):
        """TPI for several disc sizes; pairs of small sizes (5 ... 11 px) share one pass over the DEM
        (``topo_amd_tpi_multi_dev``).  outs: one DeviceArray per size.  Same bits as ``tpi_std`` per size."""
        o0, on = self._range(out_row0, out_rows)
        sz = np.ascontiguousarray(np.atleast_1d(sizes), dtype=np.int32)
        if sz.size != len(outs):
            raise ValueError(f"{sz.size} sizes but {len(outs)} output planes")
        planes = (C.c_void_p * len(outs))(*[o.ptr for o in outs])
        _lib.check(_lib.lib().topo_amd_tpi_multi_dev(*self._head(), int(sz.size), sz.ctypes.data_as(_lib._i32p), o0, on,
                                                     planes), "tpi_multi_dev")

    def gaussian(self, sigma_y, sigma_x, out, out_row0=None, out_rows=None):
        o0, on = self._range(out_row0, out_rows)
        _lib.check(_lib.lib().topo_amd_gaussian_dev(*self._head(), float(sigma_y), float(sigma_x),
                                                    o0, on, out.ptr), "gaussian_dev")

    def gaussian_valid(self, sigma_y, sigma_x, out, weight=None, min_weight=0.0, fill=False, out_row0=None, out_rows=None):
        """The Gaussian over the samples that exist (``topo_amd_gaussian_valid_dev``; ``topo.dem(skipna=True)`` for the
        rules): ``out = N / D`` of the normalised convolution, NaN where ``D`` is 0 or below ``min_weight`` and - unless
        ``fill`` - at the missing pixels; ``weight`` receives ``D``.  Radii 0 ... 121; ghost rows as for :meth:`gaussian`.
        ``out`` is a plane :meth:`tpi_std_valid` takes as it is."""
        o0, on = self._range(out_row0, out_rows)
        _lib.check(_lib.lib().topo_amd_gaussian_valid_dev(*self._head(), float(sigma_y), float(sigma_x), float(min_weight),
                                                          int(bool(fill)), o0, on, out.ptr,
                                                          weight.ptr if weight else None), "gaussian_valid_dev")

    def gradient(self, sigma, res_x, res_y, sig_ratio=1.0, dx=None, dy=None, slope=None,
                 aspect=None, out_row0=None, out_rows=None):
        o0, on = self._range(out_row0, out_rows)
        rx = np.ascontiguousarray(res_x, dtype=np.float64)
        ry = np.ascontiguousarray(res_y, dtype=np.float64)
        mode = _lib.RES_SCALAR if rx.size == 1 and ry.size == 1 else _lib.RES_1D
        if mode == _lib.RES_1D:
            assert rx.size == self.nx and ry.size == self.gny
        p = [a.ptr if a else None for a in (dx, dy, slope, aspect)]
        _lib.check(_lib.lib().topo_amd_gradient_dev(*self._head(), float(sigma), float(sig_ratio),
                                                    mode, _lib.ptr(rx), _lib.ptr(ry), o0, on, *p),
                   "gradient_dev")

    def gradient_valid(self, sigma, res_x, res_y, sig_ratio=1.0, min_weight=0.0, fill=False, dx=None, dy=None, slope=None,
                       aspect=None, out_row0=None, out_rows=None):
        """The gradient over the samples that exist (``topo_amd_gradient_valid_dev``; ``topo.gradient(skipna=True)`` for the
        rules): differences of the valid-sample Gaussian taken with ``fill`` that know which of their neighbours are defined,
        the mask-aware Sobel pair for ``sigma <= 1``; all four planes NaN at a missing pixel unless ``fill``.  Radii up to
        121; ghost rows: the wider filter's radius + 1 (1 for ``sigma <= 1``).  Any plane may be left out."""
        o0, on = self._range(out_row0, out_rows)
        rx = np.ascontiguousarray(res_x, dtype=np.float64)
        ry = np.ascontiguousarray(res_y, dtype=np.float64)
        mode = _lib.RES_SCALAR if rx.size == 1 and ry.size == 1 else _lib.RES_1D
        if mode == _lib.RES_1D:
            assert rx.size == self.nx and ry.size == self.gny
        p = [a.ptr if a else None for a in (dx, dy, slope, aspect)]
        _lib.check(_lib.lib().topo_amd_gradient_valid_dev(*self._head(), float(sigma), float(sig_ratio), float(min_weight),
                                                          int(bool(fill)), mode, _lib.ptr(rx), _lib.ptr(ry), o0, on, *p),
                   "gradient_valid_dev")

    def sx(self, dj, di, dist, window, height, out, out_row0=None, out_rows=None):
        o0, on = self._range(out_row0, out_rows)
        dj = np.ascontiguousarray(dj, dtype=np.int32)
        di = np.ascontiguousarray(di, dtype=np.int32)
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        _lib.check(_lib.lib().topo_amd_sx_dev(*self._head(), dj.ctypes.data_as(_lib._i32p),
                                              di.ctypes.data_as(_lib._i32p),
                                              dist.ctypes.data_as(_lib._f64p), dist.size, int(window),
                                              float(height), o0, on, out.ptr), "sx_dev")

    def sx_multi(self, sectors, height, outs, out_row0=None, out_rows=None):
        """Sx of several azimuth sectors in one pass.  sectors: [(window, dj, di, dist), ...] as
        returned by ``sx_offsets``; outs: one DeviceArray per sector.  Same bits as ``sx`` per sector."""
        o0, on = self._range(out_row0, out_rows)
        first, dj, di, dist, window = pack_sectors(sectors)
        planes = (C.c_void_p * len(outs))(*[o.ptr for o in outs])
        _lib.check(_lib.lib().topo_amd_sx_multi_dev(
            *self._head(), len(sectors), first.ctypes.data_as(_lib._i32p), dj.ctypes.data_as(_lib._i32p),
            di.ctypes.data_as(_lib._i32p), dist.ctypes.data_as(_lib._f64p), window.ctypes.data_as(_lib._i32p),
            float(height), o0, on, planes), "sx_multi_dev")

    def moments(self):
        """numpy's float32 ``(mean(), std())`` of this block's rows, as the valley / ridge index standardises with them: formed
        on the device in numpy's order (``mean_std_numpy``), or on the host where ``helpers.moments_chunk`` says so."""
        from .helpers import moments_chunk  # noqa: PLC0415

        chunk = moments_chunk()
        if chunk is not None:
            return mean_std_numpy(self.data, chunk, self.first, self.rows)
        field = self.data.to_host(self.first, self.rows)
        return field.mean(), field.std()

    def valley_ridge(self, taps, ksize, angles, n_planes, mean=None, stdev=None, norm=None, direction=None, out_row0=None,
                     out_rows=None):
        """taps / ksize / angles as returned by ``topo._valley_ridge_tables``; mean / stdev of the WHOLE DEM, as numpy's
        float32 ``mean()`` / ``std()`` give them.  ``None`` (both): the block must be the whole raster (``ValueError``
        otherwise - a row block cannot know them) and they are formed on the device (``mean_std_numpy``; on the host where
        ``helpers.moments_chunk`` says so)."""
        from .helpers import moments_chunk  # noqa: PLC0415

        if norm is None or direction is None:
            raise ValueError("Block.valley_ridge: norm and direction planes are required")
        o0, on = self._range(out_row0, out_rows)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        ksize = np.ascontiguousarray(ksize, dtype=np.int32)
        angles = np.ascontiguousarray(angles, dtype=np.float32)
        if mean is None or stdev is None:
            if mean is not None or stdev is not None:
                raise ValueError("Block.valley_ridge: give both mean and stdev, or neither")
            if self.row0 != 0 or self.rows != self.gny:
                raise ValueError(f"Block.valley_ridge: rows [{self.row0}, {self.row0 + self.rows}) of a raster of {self.gny} "
                                 "rows cannot form the whole raster's mean and stdev: pass them")
            chunk = moments_chunk()
            if chunk is not None and (o0, on) == (0, self.gny):
                _lib.check(_lib.lib().topo_amd_valley_ridge_std_dev(
                    self.data.row_ptr(self.first), self.rows, self.nx, taps.ctypes.data_as(_lib._vp),
                    ksize.ctypes.data_as(_lib._i32p), angles.ctypes.data_as(_lib._vp), ksize.size, int(n_planes), chunk,
                    norm.ptr, direction.ptr, None), "valley_ridge_std_dev")
                return
            mean, stdev = self.moments()
        _lib.check(_lib.lib().topo_amd_valley_ridge_dev(
            *self._head(), taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(_lib._i32p),
            angles.ctypes.data_as(_lib._vp), ksize.size, int(n_planes), float(mean), float(stdev), o0, on,
            norm.ptr, direction.ptr), "valley_ridge_dev")


    def fill_na(self, out, missing=None, x_coords=None, min_elevation=None, out_row0=None, out_rows=None):
        """Missing samples (NaN, or at or below ``min_elevation``) of the output rows replaced by the nearest valid sample
        along x (``topo_amd_fill_na_dev``; ``helpers.fill_na_gpu`` for the rules).  ``out``: a float32 DeviceArray holding
        the output rows from its first row, or this block's own plane (in place); ``missing``: a uint8 DeviceArray of the
        output rows (1 = missing before the fill) or None; ``x_coords``: one coordinate per column or None (the index)."""
        from .helpers import _fill_coords  # noqa: PLC0415

        o0, on = self._range(out_row0, out_rows)
        x = _fill_coords(x_coords, self.nx)
        if missing is not None and missing.dtype != np.uint8:
            raise ValueError("Block.fill_na: the missing mask is a uint8 DeviceArray")
        dst = self.data.row_ptr(self.first + o0 - self.row0) if out is self.data else out.ptr
        m = np.nan if min_elevation is None else float(min_elevation)
        _lib.check(_lib.lib().topo_amd_fill_na_dev(*self._head(), None if x is None else x.ctypes.data_as(_lib._f64p), m,
                                                   o0, on, dst, missing.ptr if missing is not None else None),
                   "fill_na_dev")


def mean_std(array):
    """(mean, population std) of a DeviceArray, accumulated in float64 on the GPU."""
    m, s = C.c_double(), C.c_double()
    _lib.check(_lib.lib().topo_amd_mean_std_dev(array.ptr, array.rows * array.nx, C.byref(m), C.byref(s)),
               "mean_std_dev")
    return m.value, s.value


def mean_std_numpy(array, chunk=None, row0=0, rows=None):
    """``(mean, std)`` of (rows of) a float32 DeviceArray as ``np.float32``, with the bits numpy's own ``a.mean()`` / ``a.std()``
    give for the same samples on the host: the sums are formed on the GPU in numpy's order (``topo_amd_mean_std_f32_dev``).
    ``chunk``: numpy's buffer size in samples (``np.getbufsize()``)."""
    if array.dtype != np.float32:
        raise ValueError(f"mean_std_numpy: a float32 plane, not {array.dtype}")
    rows = array.rows - row0 if rows is None else rows
    m, s = C.c_float(), C.c_float()
    _lib.check(_lib.lib().topo_amd_mean_std_f32_dev(array.row_ptr(row0), rows * array.nx,
                                                    int(np.getbufsize()) if chunk is None else int(chunk), C.byref(m), C.byref(s)),
               "mean_std_f32_dev")
    return np.float32(m.value), np.float32(s.value)


def pack_sectors(sectors):
    """Concatenated tables of the multi-azimuth entry points: (first, dj, di, dist, window)."""
    if len(sectors) == 0:
        raise ValueError("sx_multi needs at least one sector")
    counts = [len(np.atleast_1d(sec[1])) for sec in sectors]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dj = np.ascontiguousarray(np.concatenate([np.atleast_1d(sec[1]) for sec in sectors]), dtype=np.int32)
    di = np.ascontiguousarray(np.concatenate([np.atleast_1d(sec[2]) for sec in sectors]), dtype=np.int32)
    dist = np.ascontiguousarray(np.concatenate([np.atleast_1d(sec[3]) for sec in sectors]), dtype=np.float64)
    window = np.array([int(sec[0]) for sec in sectors], dtype=np.int32)
    return first, dj, di, dist, window


def sx_offsets(azimuth, radius, dx, dy, azimuth_arc=10.0, azimuth_steps=15, radius_min=0.0):
    """(window, dj, di, dist) for the C ABI from Sx parameters and mean grid spacing."""
    from . import topo  # noqa: PLC0415
    return topo._sx_sector(azimuth, radius, dx, dy, azimuth_arc, azimuth_steps, radius_min)
