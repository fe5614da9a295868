"""ctypes binding of libtopo_amd.so (C ABI: include/topo_amd.h).  No fallback of any kind."""
import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# TOPO_AMD_LIBRARY: another build of the same library (A/B runs of two builds inside one GPU session)
LIB_PATH = os.environ.get("TOPO_AMD_LIBRARY") or os.path.join(HERE, "libtopo_amd.so")

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p


class Raster(C.Structure):
    """``topo_amd_raster`` (include/topo_amd.h): a raster as it is stored, and how its samples decode to float32."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("has_nodata", C.c_int32),
                ("scale", C.c_double), ("offset", C.c_double), ("nodata", C.c_double)]


_rp = C.POINTER(Raster)
# numpy dtype -> TOPO_AMD_F32 ... TOPO_AMD_F64
F32, I16, U16, I32, U8, F64 = range(6)
SOURCE_DTYPES = {np.dtype(np.float32): F32, np.dtype(np.int16): I16, np.dtype(np.uint16): U16,
                 np.dtype(np.int32): I32, np.dtype(np.uint8): U8, np.dtype(np.float64): F64}

# name -> (restype, argtypes); every symbol include/topo_amd.h declares
SIGNATURES = {
    "topo_amd_version": (C.c_char_p, []),
    "topo_amd_last_error": (C.c_char_p, []),
    "topo_amd_device_count": (C.c_int, []),
    "topo_amd_init": (C.c_int, [C.c_int]),
    "topo_amd_shutdown": (C.c_int, []),
    "topo_amd_device_name": (C.c_int, [C.c_char_p, C.c_int]),
    "topo_amd_malloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "topo_amd_free": (C.c_int, [_vp]),
    "topo_amd_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "topo_amd_host_free": (C.c_int, [C.c_void_p]),
    "topo_amd_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_size_t]),
    "topo_amd_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_size_t]),
    "topo_amd_memcpy_d2d": (C.c_int, [_vp, _vp, C.c_size_t]),
    "topo_amd_memset": (C.c_int, [_vp, C.c_int, C.c_size_t]),
    "topo_amd_sync": (C.c_int, []),
    "topo_amd_release_host_planes": (C.c_int, []),
    "topo_amd_host_chunks": (C.c_int, [_i32p]),
    "topo_amd_valley_route": (C.c_int, [_i32p]),
    "topo_amd_tpi_route": (C.c_int, [_i32p]),
    "topo_amd_sx_route": (C.c_int, [_i32p]),
    "topo_amd_gradient_route": (C.c_int, [_i32p]),
    "topo_amd_disc_route": (C.c_int, [_i32p]),
    "topo_amd_dem_changed": (C.c_int, [_vp, C.c_size_t]),
    "topo_amd_raster_scan_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_uint64), _f32p]),
    "topo_amd_raster_class_from_scan": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), _f32p]),
    "topo_amd_raster_class_set": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]),
    "topo_amd_raster_class_get": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _f32p, _f32p, _f32p]),
    "topo_amd_shard_classify": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "topo_amd_timer_start": (C.c_int, []),
    "topo_amd_timer_stop": (C.c_int, [_f32p]),
    "topo_amd_mark": (C.c_int, [C.c_int]),
    "topo_amd_mark_elapsed": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "topo_amd_cu_count": (C.c_int, []),
    "topo_amd_synth_dem_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]),
    "topo_amd_disc_tap_count": (C.c_int, [C.c_int]),
    "topo_amd_disc_mask": (C.c_int, [C.c_int, _f32p]),
    "topo_amd_halo_rows": (C.c_int, [C.c_int, C.c_double, C.c_double, _i32p, _i32p]),
    "topo_amd_tpi_std_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, _vp, _vp]),
    "topo_amd_gaussian_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_int, C.c_int, _vp]),
    "topo_amd_sobel_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     _vp, _vp]),
    "topo_amd_gradient_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp,
                                        _vp, _vp]),
    "topo_amd_sx_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p,
                                  C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _vp]),
    "topo_amd_tpi_multi_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int,
                                         C.POINTER(_vp)]),
    "topo_amd_sx_multi_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p,
                                        _f64p, _i32p, C.c_double, C.c_int, C.c_int, C.POINTER(_vp)]),
    "topo_amd_valley_ridge_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int,
                                            C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_mean_std_dev": (C.c_int, [_vp, C.c_size_t, _f64p, _f64p]),
    "topo_amd_fill_na_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, C.c_double, C.c_int, C.c_int,
                                       _vp, _vp]),
    "topo_amd_valley_ridge_f32": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int, C.c_int,
                                            C.c_double, C.c_double, _vp, _vp]),
    "topo_amd_tpi_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp]),
    "topo_amd_std_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp]),
    "topo_amd_tpi_std_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp]),
    "topo_amd_tpi_std_multi_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _f64p, _vp, _vp]),
    "topo_amd_gauss_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double, _vp]),
    "topo_amd_sobel_f32": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_fill_na_f32": (C.c_int, [_vp, C.c_int, C.c_int, _f64p, C.c_double, _vp, _vp]),
    "topo_amd_gradient_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "topo_amd_sx_f32": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _f64p, C.c_int, C.c_int,
                                  C.c_double, _vp]),
    "topo_amd_sx_multi_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _i32p,
                                        C.c_double, C.POINTER(_vp)]),
    "topo_amd_decode_host": (C.c_int, [_rp, C.c_size_t, _vp]),
    "topo_amd_decode_dev": (C.c_int, [_vp, C.c_int, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_double, _vp]),
    "topo_amd_upload_raw": (C.c_int, [_rp, C.c_int, C.c_int, _vp]),
    "topo_amd_valley_ridge_raw": (C.c_int, [_rp, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int, C.c_int,
                                            C.c_double, C.c_double, _vp, _vp]),
    "topo_amd_tpi_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, C.c_double, _vp]),
    "topo_amd_std_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, C.c_double, _vp]),
    "topo_amd_tpi_std_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp]),
    "topo_amd_tpi_std_multi_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, _i32p, _f64p, _vp, _vp]),
    "topo_amd_gauss_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, _vp]),
    "topo_amd_sobel_raw": (C.c_int, [_rp, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_fill_na_raw": (C.c_int, [_rp, C.c_int, C.c_int, _f64p, C.c_double, _vp, _vp]),
    "topo_amd_gradient_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "topo_amd_sx_raw": (C.c_int, [_rp, C.c_int, C.c_int, _i32p, _i32p, _f64p, C.c_int, C.c_int,
                                  C.c_double, _vp]),
    "topo_amd_sx_multi_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _i32p,
                                        C.c_double, C.POINTER(_vp)]),
    "topo_amd_shard_sx_multi": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p,
                                          _i32p, _f64p, _i32p, C.c_double, C.POINTER(_vp)]),
    "topo_amd_shard_valley_ridge": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int,
                                              C.c_int, _vp, _vp]),
    "topo_amd_comm_unique_id": (C.c_int, [C.c_char_p]),
    "topo_amd_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_char_p]),
    "topo_amd_comm_rank": (C.c_int, []),
    "topo_amd_comm_size": (C.c_int, []),
    "topo_amd_comm_destroy": (C.c_int, []),
    "topo_amd_halo_exchange_start": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "topo_amd_halo_wait": (C.c_int, []),
    "topo_amd_gate_giveups": (C.c_int, [C.POINTER(C.c_uint)]),
    "topo_amd_shard_layout": (C.c_int, [C.c_int, C.c_int]),
    "topo_amd_shard_layout_get": (C.c_int, [_i32p, _i32p]),
    "topo_amd_shard_tpi_std": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_shard_gradient": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                          C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "topo_amd_shard_sx": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p,
                                    C.c_int, C.c_int, C.c_double, _vp]),
    "topo_amd_shard_gaussian": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _vp]),
    "topo_amd_shard_tpi_std_smoothed": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp,
                                                  _vp]),
    "topo_amd_shard_valley_ridge_smoothed": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _i32p, _vp,
                                                       C.c_int, C.c_int, C.c_double, _vp, _vp, _f64p]),
    "topo_amd_shard_fill_na": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, C.c_double, _vp, _vp]),
}

UNIQUE_ID_BYTES = 128
RES_SCALAR, RES_1D, RES_2D = 0, 1, 2
DESC_TPI, DESC_STD, DESC_GAUSS, DESC_GRADIENT, DESC_SOBEL, DESC_SX, DESC_VALLEY_RIDGE = range(7)


class TopoAmdError(RuntimeError):
    """An entry point of libtopo_amd.so returned a non-zero status."""


_lock = threading.Lock()
_lib = None
_ready = False


def load():
    """dlopen the library and attach signatures (no GPU needed for this step)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise TopoAmdError(
                    f"{LIB_PATH} is missing: build it with `python -m topo_descriptors_amd.build` "
                    "(needs hipcc). There is no CPU fallback.")
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
        return _lib


def check(status, what):
    if status != 0:
        msg = load().topo_amd_last_error().decode(errors="replace")
        raise TopoAmdError(f"{what} failed with status {status}: {msg}")


def lib():
    """The loaded library bound to a GPU; raises when there is none."""
    global _ready
    handle = load()
    if not _ready:
        device = int(os.environ.get("TOPO_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        if handle.topo_amd_device_count() < 1:
            raise TopoAmdError("no HIP device visible: topo_descriptors_amd needs an AMD GPU "
                               "(gfx950); there is no CPU fallback")
        check(handle.topo_amd_init(device), "topo_amd_init")
        _ready = True
    return handle


def ptr(array):
    """void* of a C-contiguous numpy array (or None)."""
    if array is None:
        return None
    return array.ctypes.data_as(_vp)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def as_source(values, scale=1.0, offset=0.0, nodata=None):
    """``(array, Raster)`` for the ``*_raw`` entry points: the array to keep alive for the call and the struct that points
    into it.  Native-endian arrays of float32, int16, uint16, int32, uint8 and float64 go as they are stored (copied only
    to make them C-contiguous; the dtype never changes) and are decoded on the GPU; anything else (int64, float16, bool,
    byte-swapped, object) is cast to float32 on the host first, as :func:`as_f32` does."""
    a = np.asarray(values)
    if a.dtype in SOURCE_DTYPES and a.dtype.isnative:
        a = np.ascontiguousarray(a)
    else:
        a = as_f32(a)
    raster = Raster(a.ctypes.data, SOURCE_DTYPES[a.dtype], int(nodata is not None), float(scale), float(offset),
                    0.0 if nodata is None else float(nodata))
    return a, raster


class PackedDem:
    """A DEM as a file stores it - ``values`` of any dtype with CF's ``scale_factor``, ``add_offset`` and ``_FillValue`` -
    for every ``topo.*`` function that takes an ndarray: the samples are uploaded as stored and decoded on the GPU
    (include/topo_amd.h, "raw sources": ``fill_value`` becomes NaN, every other sample ``float32(float64(raw) *
    scale_factor + add_offset)``).  What it decodes to is float32: ``dtype`` says so, whatever ``values.dtype`` is."""

    def __init__(self, values, scale_factor=1.0, add_offset=0.0, fill_value=None):
        self.values = np.asarray(values)
        self.scale_factor = float(scale_factor)
        self.add_offset = float(add_offset)
        self.fill_value = None if fill_value is None else float(fill_value)
        self.shape = self.values.shape
        self.ndim = self.values.ndim
        self.dtype = np.dtype(np.float32)

    def source(self):
        return as_source(self.values, self.scale_factor, self.add_offset, self.fill_value)

    def decode(self):
        """The float32 array the GPU decodes to, computed on the host (``topo_amd_decode_host``; one thread)."""
        a, raster = self.source()
        out = np.empty(a.shape, dtype=np.float32)
        check(load().topo_amd_decode_host(C.byref(raster), a.size, ptr(out)), "topo_amd_decode_host")
        return out


def source_of(values):
    """:func:`as_source` of an ndarray or a :class:`PackedDem`."""
    if isinstance(values, PackedDem):
        return values.source()
    return as_source(values)
