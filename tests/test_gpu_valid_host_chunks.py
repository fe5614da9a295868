"""The two valid-sample host calls - ``topo_amd_tpi_std_valid_packed`` (``topo.tpi(skipna=True)``) and
``topo_amd_gauss_valid_packed`` (``topo.dem(skipna=True)``) - in THREE row chunks, like tests/test_gpu_host_pipeline.py for the
other host calls: each of them hands the pipeline its own count of ghost rows beneath a chunk, and a wrong count shows only at a
chunk seam.

``TOPO_AMD_HOST_CHUNK_MB=1`` makes chunks of 960 rows (the minimum) and a call is cut only when it holds three of them, so the
raster has 3100 rows (960 + 960 + 1180); 203 columns keep a chunk under two minimum chunks.  Its gaps lie on the seams: a whole NaN
row at 958, a 23-row block across row 960, a patch across row 1920.  A second source stores the same raster as int16 decimetres
with a declared nodata.  Every plane and both counters of a packed one must equal, byte for byte, those of the serial order
(``TOPO_AMD_HOST_PIPELINE=0``) and of the ``*_dev`` call on the resident whole raster - with pageable and page-locked arrays,
downloads issued by the default rule, a second thread and the calling thread."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, device as d  # noqa: E402

NY, NX = 3100, 203
SEAM = 960  # first row of the second chunk; the third starts at 2 * SEAM
ENV = ("TOPO_AMD_HOST_CHUNK_MB", "TOPO_AMD_HOST_PIPELINE", "TOPO_AMD_HOST_DOWNLOADS")
# (pipeline switch, downloads) - the first entry is the serial order: one chunk
MODES = [("0", None), (None, None), (None, "thread"), (None, "inline")]
TPI_PACK = tda.Packing(np.int16, 0.01, 0.0, -32768)
STD_PACK = tda.Packing(np.uint16, 0.01, 0.0, 65535)
DEM_PACK = tda.Packing(np.uint16, 0.05, 0.0, 65535)


def gappy():
    dem = orc.synthetic_dem(NY, NX, seed=31, integer=False)
    dem[SEAM - 2, :] = np.nan                          # a whole row just above the first seam
    dem[SEAM - 11: SEAM + 12, 60:150] = np.nan         # 23 rows across it
    dem[2 * SEAM - 4: 2 * SEAM + 5, 20:45] = np.nan    # a patch across the second seam
    dem.setflags(write=False)
    return dem


def as_int16(dem):
    with np.errstate(invalid="ignore"):
        codes = np.where(np.isnan(dem), -32768, np.rint(dem.astype(np.float64) * 10.0)).astype(np.int16)
    return tda.PackedDem(codes, scale_factor=0.1, fill_value=-32768)


SOURCES = {"float32": gappy(), "int16": as_int16(gappy())}


@functools.lru_cache(maxsize=None)
def resident(source):
    return d.DeviceArray.from_host(SOURCES[source])


class Pinned:
    """A page-locked array from topo_amd_host_alloc."""

    def __init__(self, shape, dtype):
        self.p = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _lib.check(_lib.lib().topo_amd_host_alloc(C.byref(self.p), n), "host_alloc")
        self.a = np.frombuffer((C.c_char * n).from_address(self.p.value), dtype=dtype).reshape(shape)

    def free(self):
        self.a = None
        _lib.check(_lib.lib().topo_amd_host_free(self.p), "host_free")


class Arrays:
    """The source as it is stored and one result array per dtype of ``dtypes``, pageable or page-locked."""

    def __init__(self, source, dtypes, pinned):
        stored, _ = _lib.source_of(SOURCES[source])
        self.pins = []
        if pinned:
            self.pins = [Pinned(stored.shape, stored.dtype)] + [Pinned((NY, NX), t) for t in dtypes]
            self.src = self.pins[0].a
            self.src[:] = stored
            self.outs = [p.a for p in self.pins[1:]]
        else:
            self.src = stored
            self.outs = [np.empty((NY, NX), dtype=t) for t in dtypes]
        self.raster = _lib.source_of(SOURCES[source])[1]
        self.raster.data = self.src.ctypes.data

    def spoil(self):
        for o in self.outs:
            o.view(np.uint8)[:] = 0xA5  # a row no download reaches would show

    def free(self):
        for p in self.pins:
            p.free()


def set_mode(pipeline, downloads):
    os.environ["TOPO_AMD_HOST_CHUNK_MB"] = "1"
    for key, val in (("TOPO_AMD_HOST_PIPELINE", pipeline), ("TOPO_AMD_HOST_DOWNLOADS", downloads)):
        if val is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = val


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.get(k) for k in ENV}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def struct_of(packing, array):
    return (_lib.Packing(np.float32) if packing is None else packing).struct(array.ctypes.data)


def dtype_of(packing):
    return np.dtype(np.float32) if packing is None else packing.dtype


def device_planes(source, n, dev_call):
    """The float32 planes of the ``*_dev`` call on the resident whole raster, as device arrays."""
    outs = [d.DeviceArray(NY, NX) for _ in range(n)]
    dev_call(d.Block(resident(source)), outs)
    d.sync()
    return outs


def wanted(plane, packing):
    """``(bytes, missing, saturated)`` of a device plane as the caller of a host call gets it."""
    if packing is None:
        return plane.to_host(), 0, 0
    packed = plane.to_packed(packing)
    return packed.values, packed.missing, packed.saturated


def walk(source, packs, host_call, want):
    """``host_call(lib, raster, plane structs, arrays)`` in every mode on pageable and page-locked arrays: three chunks unless
    the pipeline is off, and the planes and counters of ``want`` every time."""
    lib = _lib.lib()
    for pinned in (False, True):
        arrays = Arrays(source, [dtype_of(q) for q in packs], pinned)
        try:
            for pipeline, downloads in MODES:
                arrays.spoil()
                structs = [struct_of(q, a) for q, a in zip(packs, arrays.outs)]
                set_mode(pipeline, downloads)
                rc = host_call(lib, C.byref(arrays.raster), structs, arrays.outs)
                where = (source, "pinned" if pinned else "pageable", pipeline, downloads)
                assert rc == 0, (where, rc, lib.topo_amd_last_error())
                chunks = d.host_chunks()
                assert chunks == 1 if pipeline == "0" else chunks >= 3, (where, chunks)
                for k, (got, plane, q, (w, missing, saturated)) in enumerate(zip(arrays.outs, structs, packs, want)):
                    assert same_bits(got, w), (where, k, int((got != w).sum()))
                    if q is not None:
                        assert (plane.missing, plane.saturated) == (missing, saturated), (where, k)
        finally:
            arrays.free()


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("min_count", [1, 40])
@pytest.mark.parametrize("size", [9, 101])
def test_valid_sample_tpi_std_in_three_chunks(size, min_count, source):
    planes = device_planes(source, 2, lambda blk, o: blk.tpi_std_valid(size, tpi=o[0], std=o[1], min_count=min_count))
    try:
        assert np.isnan(planes[0].to_host()).sum() > NX  # (the gaps are there)
        for packs in ((None, None), (TPI_PACK, STD_PACK)):
            want = [wanted(p, q) for p, q in zip(planes, packs)]
            walk(source, packs, lambda lib, src, s, _: lib.topo_amd_tpi_std_valid_packed(src, NY, NX, size, min_count, C.byref(s[0]), C.byref(s[1])),
                 want)
    finally:
        for p in planes:
            p.free()


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("sigma", [2.0, 30.25])
def test_valid_sample_gaussian_in_three_chunks(sigma, fill, source):
    planes = device_planes(source, 2, lambda blk, o: blk.gaussian_valid(sigma, sigma, o[0], weight=o[1], fill=fill))
    try:
        for pack in (None, DEM_PACK):
            want = [wanted(planes[0], pack), wanted(planes[1], None)]  # (the weight plane is float32 whatever the packing)
            walk(source, (pack, None),
                 lambda lib, src, s, a: lib.topo_amd_gauss_valid_packed(src, NY, NX, sigma, sigma, 0.0, int(fill), C.byref(s[0]), _lib.ptr(a[1])),
                 want)
    finally:
        for p in planes:
            p.free()
