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


class Plane(C.Structure):
    """``topo_amd_plane`` (include/topo_amd.h): a result array as a file stores it, how float32 samples encode into it, and
    the two counters the encode reports."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("has_nodata", C.c_int32),
                ("scale", C.c_double), ("offset", C.c_double), ("nodata", C.c_double),
                ("missing", C.c_uint64), ("saturated", C.c_uint64)]


_rp = C.POINTER(Raster)
_pp = C.POINTER(Plane)
# numpy dtype -> TOPO_AMD_F32 ... TOPO_AMD_F64
F32, I16, U16, I32, U8, F64 = range(6)
SOURCE_DTYPES = {np.dtype(np.float32): F32, np.dtype(np.int16): I16, np.dtype(np.uint16): U16,
                 np.dtype(np.int32): I32, np.dtype(np.uint8): U8, np.dtype(np.float64): F64}
F16 = 6  # TOPO_AMD_F16: result planes only
PLANE_DTYPES = {np.dtype(np.float32): F32, np.dtype(np.int16): I16, np.dtype(np.uint16): U16, np.dtype(np.uint8): U8,
                np.dtype(np.float16): F16}

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
    "topo_amd_valley_moments_route": (C.c_int, [_i32p]),
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
    "topo_amd_tpi_std_valid_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, _vp, _vp]),
    "topo_amd_tpi_std_valid_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_tpi_std_valid_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, C.c_int, _pp, _pp]),
    "topo_amd_gaussian_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_int, C.c_int, _vp]),
    "topo_amd_gaussian_valid_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                              C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_gauss_valid_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp]),
    "topo_amd_gauss_valid_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _pp, _vp]),
    "topo_amd_sobel_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     _vp, _vp]),
    "topo_amd_gradient_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp,
                                        _vp, _vp]),
    "topo_amd_gradient_valid_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                              C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "topo_amd_gradient_valid_raw": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                              _vp, _vp, _vp, _vp, _vp, _vp]),
    "topo_amd_gradient_valid_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                                 _vp, _vp, _pp, _pp, _pp, _pp]),
    "topo_amd_sx_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p,
                                  C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _vp]),
    "topo_amd_tpi_multi_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int,
                                         C.POINTER(_vp)]),
    "topo_amd_sx_multi_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p,
                                        _f64p, _i32p, C.c_double, C.c_int, C.c_int, C.POINTER(_vp)]),
    "topo_amd_valley_ridge_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int,
                                            C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp]),
    "topo_amd_mean_std_dev": (C.c_int, [_vp, C.c_size_t, _f64p, _f64p]),
    "topo_amd_mean_std_f32_dev": (C.c_int, [_vp, C.c_size_t, C.c_size_t, _f32p, _f32p]),
    "topo_amd_valley_ridge_std_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int, C.c_int, C.c_size_t, _vp, _vp,
                                                _f32p]),
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
    "topo_amd_valley_ridge_std_raw": (C.c_int, [_rp, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int, C.c_int, C.c_double,
                                                C.c_size_t, _vp, _vp, _f32p]),
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
    "topo_amd_encode_host": (C.c_int, [_vp, C.c_size_t, _pp]),
    "topo_amd_encode_dev": (C.c_int, [_vp, C.c_size_t, _pp]),
    "topo_amd_finish_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _pp]),
    "topo_amd_tpi_std_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, C.c_double, _pp, _pp]),
    "topo_amd_tpi_std_multi_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, _i32p, _f64p, _pp, _pp]),
    "topo_amd_gauss_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, _pp]),
    "topo_amd_gradient_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                           _vp, _vp, _pp, _pp, _pp, _pp]),
    "topo_amd_sx_packed": (C.c_int, [_rp, C.c_int, C.c_int, _i32p, _i32p, _f64p, C.c_int, C.c_int,
                                     C.c_double, _pp]),
    "topo_amd_sx_multi_packed": (C.c_int, [_rp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _i32p,
                                           C.c_double, _pp]),
    "topo_amd_valley_ridge_packed": (C.c_int, [_rp, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int, C.c_int, C.c_double,
                                               C.c_size_t, _pp, _pp, _f32p]),
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
    "topo_amd_shard_mean_std_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, _f32p, _f32p]),
    "topo_amd_shard_valley_ridge_std": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _i32p, _vp, C.c_int, C.c_int,
                                                  C.c_double, C.c_size_t, _vp, _vp, _f32p]),
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


# ---- packed result planes (include/topo_amd.h, "packed result planes") --------------------------------------------------------
class Packing:
    """How a float32 result plane is to be stored: ``dtype`` int16, uint16 or uint8 with CF's ``scale_factor``,
    ``add_offset`` and a ``fill_value`` for NaN - which must be the type's lowest or highest code, so that no value is ever
    stored as it - or float16 (no scale, no offset, no fill value: NaN stays NaN), or float32 (the plane as it is).  A sample
    ``v`` becomes ``rint((float64(v) - add_offset) / scale_factor)``, clamped to the codes that are left.  The request is
    checked here, on the host, with the library's rules: ``ValueError`` before any library call."""

    def __init__(self, dtype, scale_factor=1.0, add_offset=0.0, fill_value=None):
        try:
            self.dtype = np.dtype(dtype)
        except TypeError as exc:
            raise ValueError(f"Packing: {dtype!r} is not a dtype") from exc
        if self.dtype not in PLANE_DTYPES or not self.dtype.isnative:
            raise ValueError(f"Packing: result planes are int16, uint16, uint8, float16 or float32, not {self.dtype}")
        self.scale_factor, self.add_offset = float(scale_factor), float(add_offset)
        self.fill_value = None if fill_value is None else float(fill_value)
        if not np.isfinite(self.scale_factor) or self.scale_factor == 0.0:
            raise ValueError(f"Packing: scale_factor {self.scale_factor} (it must be finite and not 0)")
        if not np.isfinite(self.add_offset):
            raise ValueError(f"Packing: add_offset {self.add_offset} is not finite")
        if self.dtype.kind == "f":
            if self.scale_factor != 1.0 or self.add_offset != 0.0 or self.fill_value is not None:
                raise ValueError(f"Packing: a {self.dtype} plane takes scale_factor 1, add_offset 0 and no fill_value")
        else:
            info = np.iinfo(self.dtype)
            if self.fill_value is None:
                raise ValueError(f"Packing: an {self.dtype} plane needs a fill_value (NaN has no other place)")
            if self.fill_value not in (float(info.min), float(info.max)):
                raise ValueError(f"Packing: fill_value {self.fill_value} must be the lowest or highest code of {self.dtype} "
                                 f"({info.min} or {info.max})")

    def __repr__(self):
        return f"Packing({self.dtype}, {self.scale_factor}, {self.add_offset}, {self.fill_value})"

    def struct(self, address):
        """The ``Plane`` of an array of this packing at ``address`` (host or device)."""
        return Plane(address, PLANE_DTYPES[self.dtype], int(self.fill_value is not None), self.scale_factor, self.add_offset,
                     0.0 if self.fill_value is None else self.fill_value, 0, 0)


class PackedPlane(PackedDem):
    """A result plane as it came off the GPU: ``values`` (int16 / uint16 / uint8 codes, float16 or float32) with the CF triple
    of its :class:`Packing`, ``missing`` (samples stored as the fill value, or NaN for float16) and ``saturated`` (samples
    clamped to the end of the code range, or finite ones that became inf in float16).  It is a :class:`PackedDem`:
    ``decode()`` gives the float32 array - NaN exactly where the result was NaN - and it can go straight back in as a source
    (a packed smoothed DEM into ``topo.tpi``)."""

    def __init__(self, values, packing, missing=0, saturated=0):
        super().__init__(values, packing.scale_factor, packing.add_offset, packing.fill_value)
        self.packing = packing
        self.missing, self.saturated = int(missing), int(saturated)


def result_plane(packing, shape):
    """``(array, Plane)`` of one result of a ``*_packed`` call: an uninitialised array of the packing's dtype (``None``:
    float32) and the struct that points into it."""
    packing = Packing(np.float32) if packing is None else packing
    array = np.empty(shape, dtype=packing.dtype)
    return array, packing.struct(array.ctypes.data)


def wrap_plane(array, plane, packing):
    """What a ``pack=`` call returns for one plane: the float32 array for ``None``, a :class:`PackedPlane` otherwise."""
    return array if packing is None else PackedPlane(array, packing, plane.missing, plane.saturated)


def plane_array(structs):
    """A C array of ``Plane`` from a list of structs (the ``topo_amd_plane*`` of the multi-plane calls)."""
    return (Plane * len(structs))(*structs)


def encode_host(array, packing):
    """``array`` (float32) packed on the host (``topo_amd_encode_host``; one thread): the CPU statement of what the GPU does."""
    a = as_f32(array)
    out, plane = result_plane(packing, a.shape)
    check(load().topo_amd_encode_host(ptr(a), a.size, C.byref(plane)), "topo_amd_encode_host")
    return PackedPlane(out, packing, plane.missing, plane.saturated)


def pack_list(pack, names):
    """One packing (or ``None``: float32) per plane of a call from its ``pack`` argument: a single :class:`Packing` for all
    planes, a sequence with one entry per plane, or a dict keyed by ``names``."""
    if pack is None or isinstance(pack, Packing):
        out = [pack] * len(names)
    elif isinstance(pack, dict):
        unknown = set(pack) - set(names)
        if unknown:
            raise ValueError(f"pack: unknown planes {sorted(map(str, unknown))}; the planes are {list(names)}")
        out = [pack.get(n) for n in names]
    else:
        out = list(pack)
        if len(out) != len(names):
            raise ValueError(f"pack: {len(out)} entries for {len(names)} planes")
    for q in out:
        if q is not None and not isinstance(q, Packing):
            raise ValueError(f"pack: {q!r} is not a Packing")
    return out
