"""Raw sources on the GPU (include/topo_amd.h, "raw sources"): a DEM uploaded as it is stored - int16 with a nodata value,
packed int16 / int32, uint16, uint8, float64, scaled float32 - and decoded on the device (csrc/decode.hip) must give, in every
output plane and bit for bit, what the same call gives on the float32 array ``topo_amd_decode_host`` makes of it.

Every ``*_raw`` entry point x seven sources x two shapes (3100 x 1999: a row chunk of a 2-byte source does not start on a
16-byte boundary; 3100 x 1024) x {one chunk, three chunks (``TOPO_AMD_HOST_CHUNK_MB=1``: 960 + 960 + 1180 rows)} x {pageable,
page-locked arrays}; then the Python layer (``PackedDem`` through ``topo.*``, ``helpers.fill_na_gpu``, ``batch.compute_tpi``,
``DeviceArray.from_host``), the decode on its own (``topo_amd_decode_dev`` / ``topo_amd_upload_raw`` against
``topo_amd_decode_host``, at counts and offsets that are not multiples of a 16-byte group) and two threads with different
source types.  No tolerance anywhere.  (``topo_amd_valley_ridge_raw`` is one chunk by design, like its ``_f32`` namesake.)"""
import ctypes as C
import os
import threading
import zlib

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, batch, device as d, helpers as hlp, topo  # noqa: E402

NY = 3100
SHAPES = {"odd_nx": (NY, 1999), "nx_mult_of_4": (NY, 1024)}
SEAM = 960  # first row of the second chunk
ENV = ("TOPO_AMD_HOST_CHUNK_MB", "TOPO_AMD_HOST_PIPELINE", "TOPO_AMD_HOST_DOWNLOADS")
NODATA = -32768


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.get(k) for k in ENV}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def set_chunks(many):
    os.environ["TOPO_AMD_HOST_CHUNK_MB"] = "1"
    os.environ.pop("TOPO_AMD_HOST_DOWNLOADS", None)
    if many:
        os.environ.pop("TOPO_AMD_HOST_PIPELINE", None)
    else:
        os.environ["TOPO_AMD_HOST_PIPELINE"] = "0"


def make_sources(ny, nx):
    """name -> (stored array, scale, offset, nodata)"""
    whole = orc.synthetic_dem(ny, nx, seed=51, integer=True)
    frac = orc.synthetic_dem(ny, nx, seed=52, integer=False)
    out = {}
    a = whole.astype(np.int16)
    a[100, 200] = NODATA                                # a void of one pixel,
    a[500:540, 300:340] = NODATA                        # a block of 40,
    a[SEAM - 3: SEAM + 4, nx // 3: nx // 3 + 200] = NODATA  # and a run lying across the first chunk seam
    out["metres_i16_nodata"] = (a, 1.0, 0.0, NODATA)
    out["decimetres_i16"] = (np.rint(np.clip(frac, -3000.0, 3000.0) * 10.0).astype(np.int16), 0.1, 0.0, None)
    out["plain_u16"] = (np.clip(whole, 0, 65535).astype(np.uint16), 1.0, 0.0, None)
    out["millimetres_i32"] = (np.rint(frac.astype(np.float64) * 1000.0).astype(np.int32), 0.001, 0.0, None)
    out["plain_u8"] = (np.clip(whole / 16.0, 0, 255).astype(np.uint8), 1.0, 0.0, None)
    f = frac.astype(np.float64) + 0.123456789  # (not float32 values: the rounding to float32 is the device's)
    f[1234, 567] = np.nan
    out["fractional_f64_nan"] = (f, 1.0, 0.0, None)
    out["scaled_f32"] = (frac.copy(), 0.3048, -12.5, None)
    return out


_CACHE = {}


def source(shape_name, name):
    """(stored array, Raster arguments, host-decoded float32 array)"""
    if shape_name not in _CACHE:
        _CACHE.clear()  # (one shape's rasters at a time)
        _CACHE[shape_name] = {}
        for k, (a, scale, offset, nodata) in make_sources(*SHAPES[shape_name]).items():
            _CACHE[shape_name][k] = (a, (scale, offset, nodata), host_decode(a, scale, offset, nodata))
    return _CACHE[shape_name][name]


SOURCE_NAMES = ["metres_i16_nodata", "decimetres_i16", "plain_u16", "millimetres_i32", "plain_u8", "fractional_f64_nan", "scaled_f32"]


def host_decode(a, scale, offset, nodata):
    keep, raster = _lib.as_source(a, scale, offset, nodata)
    assert keep.dtype == a.dtype
    out = np.empty(a.shape, dtype=np.float32)
    _lib.check(_lib.load().topo_amd_decode_host(C.byref(raster), a.size, _lib.ptr(out)), "decode_host")
    return out


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


class Buffer:
    """nbytes of pageable or page-locked (topo_amd_host_alloc) host memory."""

    def __init__(self, nbytes, pinned):
        self.p = None
        if pinned:
            self.p = C.c_void_p()
            _lib.check(_lib.lib().topo_amd_host_alloc(C.byref(self.p), nbytes), "host_alloc")
            self.bytes = np.frombuffer((C.c_char * nbytes).from_address(self.p.value), dtype=np.uint8)
        else:
            self.bytes = np.empty(nbytes, dtype=np.uint8)

    def free(self):
        self.bytes = None
        if self.p is not None:
            _lib.check(_lib.lib().topo_amd_host_free(self.p), "host_free")


def vp(buf):
    return buf.bytes.ctypes.data_as(_lib._vp)


# ---- the calls: name -> (output planes, bytes per sample of each, call(lib, kind, src, ny, nx, outs)); kind: "raw" | "f32"
def fn(lib, base, kind):
    return getattr(lib, f"topo_amd_{base}_{kind}")


def tables(shape):
    ny, nx = shape
    sectors = [d.sx_offsets(a, 500.0, 30.0, -30.0) for a in (350.0, 0.0, 45.0)]
    w, dj, di, dist = sectors[1]
    dj, di = np.ascontiguousarray(dj, dtype=np.int32), np.ascontiguousarray(di, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    first, mdj, mdi, mdist, mwin = d.pack_sectors(sectors)
    kernels = topo._valley_kernels(7, [0, 0.15, 0.3])
    taps, ksize, angles = topo._valley_ridge_tables(kernels, np.arange(0, 180, 45, dtype=np.float32))
    sizes = np.array([5, 9, 67], dtype=np.int32)
    sigmas = np.zeros(3)
    rx, ry = np.array([30.0]), np.array([-30.0])
    xs = 2600000.0 + 30.0 * np.arange(nx)
    i32, f64 = _lib._i32p, _lib._f64p

    def multi(lib, kind, s, o):
        t = (C.c_void_p * 3)(*[b.bytes.ctypes.data for b in o[:3]])
        sd = (C.c_void_p * 3)(*[b.bytes.ctypes.data for b in o[3:]])
        return fn(lib, "tpi_std_multi", kind)(s, ny, nx, 3, sizes.ctypes.data_as(i32), sigmas.ctypes.data_as(f64), t, sd)

    def sx_multi(lib, kind, s, o):
        planes = (C.c_void_p * 3)(*[b.bytes.ctypes.data for b in o])
        return fn(lib, "sx_multi", kind)(s, ny, nx, 3, first.ctypes.data_as(i32), mdj.ctypes.data_as(i32), mdi.ctypes.data_as(i32),
                                        mdist.ctypes.data_as(f64), mwin.ctypes.data_as(i32), 10.0, planes)

    return {
        "tpi7": ([4], lambda lib, k, s, o: fn(lib, "tpi", k)(s, ny, nx, 7, 0.0, vp(o[0]))),
        "tpi31": ([4], lambda lib, k, s, o: fn(lib, "tpi", k)(s, ny, nx, 31, 0.0, vp(o[0]))),
        "tpi67": ([4], lambda lib, k, s, o: fn(lib, "tpi", k)(s, ny, nx, 67, 0.0, vp(o[0]))),
        "std7": ([4], lambda lib, k, s, o: fn(lib, "std", k)(s, ny, nx, 7, 0.0, vp(o[0]))),
        "std67": ([4], lambda lib, k, s, o: fn(lib, "std", k)(s, ny, nx, 67, 0.0, vp(o[0]))),
        "tpi_std67": ([4, 4], lambda lib, k, s, o: fn(lib, "tpi_std", k)(s, ny, nx, 67, 0.0, vp(o[0]), vp(o[1]))),
        "tpi_std_multi": ([4] * 6, multi),
        "gauss3.25": ([4], lambda lib, k, s, o: fn(lib, "gauss", k)(s, ny, nx, 3.25, 3.25, vp(o[0]))),
        "gradient3.25": ([4] * 4, lambda lib, k, s, o: fn(lib, "gradient", k)(s, ny, nx, 3.25, 1.0, _lib.RES_SCALAR, _lib.ptr(rx),
                                                                                _lib.ptr(ry), *[vp(b) for b in o])),
        "sobel": ([4, 4], lambda lib, k, s, o: fn(lib, "sobel", k)(s, ny, nx, vp(o[0]), vp(o[1]))),
        "sx": ([4], lambda lib, k, s, o: fn(lib, "sx", k)(s, ny, nx, dj.ctypes.data_as(i32), di.ctypes.data_as(i32),
                                                          dist.ctypes.data_as(f64), dist.size, int(w), 10.0, vp(o[0]))),
        "sx_multi": ([4] * 3, sx_multi),
        "valley_ridge7": ([4, 4], lambda lib, k, s, o: fn(lib, "valley_ridge", k)(
            s, ny, nx, taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(i32), angles.ctypes.data_as(_lib._vp), ksize.size,
            int(kernels.shape[0]), 1234.5, 321.25, vp(o[0]), vp(o[1]))),
        "fill_na": ([4, 1], lambda lib, k, s, o: fn(lib, "fill_na", k)(s, ny, nx, xs.ctypes.data_as(f64), 250.0, vp(o[0]), vp(o[1]))),
    }


CASE_NAMES = ["tpi7", "tpi31", "tpi67", "std7", "std67", "tpi_std67", "tpi_std_multi", "gauss3.25", "gradient3.25", "sobel", "sx",
              "sx_multi", "valley_ridge7", "fill_na"]
_TABLES = {}


@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("src_name", SOURCE_NAMES)
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_raw_call_has_the_bits_of_the_f32_call_on_the_decoded_array(shape_name, src_name, case):
    shape = SHAPES[shape_name]
    ny, nx = shape
    stored, (scale, offset, nodata), decoded = source(shape_name, src_name)
    if shape_name not in _TABLES:
        _TABLES[shape_name] = tables(shape)
    elems, call = _TABLES[shape_name][case]
    lib = _lib.lib()
    for many in (False, True):
        set_chunks(many)
        want = [Buffer(ny * nx * e, False) for e in elems]
        for b in want:
            b.bytes[:] = 0xA5
        rc_want = call(lib, "f32", decoded.ctypes.data_as(_lib._vp), want)
        assert rc_want in (0, -6), (case, rc_want, lib.topo_amd_last_error())
        chunks_want = d.host_chunks()
        for pinned in (False, True):
            raw = Buffer(stored.nbytes, pinned)
            raw.bytes[:] = stored.reshape(-1).view(np.uint8)
            outs = [Buffer(ny * nx * e, pinned) for e in elems]
            try:
                for b in outs:
                    b.bytes[:] = 0xA5
                raster = _lib.Raster(raw.bytes.ctypes.data, _lib.SOURCE_DTYPES[stored.dtype], int(nodata is not None), scale, offset,
                                     0.0 if nodata is None else float(nodata))
                rc = call(lib, "raw", C.byref(raster), outs)
                assert rc == rc_want, (case, src_name, rc, lib.topo_amd_last_error())
                chunks = d.host_chunks()
                assert chunks == chunks_want  # (cuts are sized by the float32 rows)
                if case == "valley_ridge7" or not many:
                    assert chunks == 1, (case, chunks)
                else:
                    assert chunks >= 3, (case, chunks)
                for k, (g, w) in enumerate(zip(outs, want)):
                    if not np.array_equal(g.bytes, w.bytes):
                        bad = int((g.bytes != w.bytes).sum())
                        raise AssertionError((shape_name, src_name, case, "chunks" if many else "one chunk",
                                              "pinned" if pinned else "pageable", "plane", k, "bytes that differ", bad))
            finally:
                raw.free()
                for b in outs:
                    b.free()


# ---- the decode on its own ----------------------------------------------------------------------------------------------
PARAMS = [(1.0, 0.0, None), (0.1, 0.0, -32768.0), (0.001, -500.25, 65535.0), (1.0 / 3.0, 7e-3, None)]
DTYPES = [np.float32, np.int16, np.uint16, np.int32, np.uint8, np.float64]


def raw_samples(dtype, count, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=count, endpoint=True).astype(dt)
        special = [v for v in (info.min, info.max, 0, -32768, 65535) if info.min <= v <= info.max]
    else:
        info = np.finfo(dt)
        a = (rng.standard_normal(count) * 3000.0).astype(dt)
        special = [info.min, info.max, info.tiny, 0.0, -0.0, 65535.0, -32768.0, np.nan, np.inf, -np.inf]
        if dt == np.float64:
            special += [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e39, -1e39, 1e-40, -1e-40, 2.0 ** -150, 3 * 2.0 ** -150, 5e-324]
    special = np.array(special, dtype=dt)
    k = min(count, special.size)
    a[:k] = special[:k]
    return a


def assert_decoded(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
def test_decode_dev_is_decode_host(dtype):
    lib = _lib.lib()
    item = np.dtype(dtype).itemsize
    room = 100003 + 64
    d_raw = d.DeviceArray(1, room * item, dtype=np.uint8)
    d_out = d.DeviceArray(1, room, dtype=np.float32)
    try:
        for scale, offset, nodata in PARAMS:
            # (sample offset of the input, of the output): the same phase, and phases that share no 16-byte boundary
            for off_in, off_out in ((0, 0), (1, 1), (3, 3), (5, 5), (8, 8), (13, 13), (1, 2), (0, 1), (3, 0)):
                for count in (0, 1, 7, 8, 9, 33, 1000, 100003):
                    raw = raw_samples(dtype, count, seed=count + off_in)
                    want = host_decode(raw, scale, offset, nodata)
                    _lib.check(lib.topo_amd_memset(d_out.ptr, 0x5A, d_out.nbytes), "memset")
                    if count:
                        _lib.check(lib.topo_amd_memcpy_h2d(d_raw.ptr + off_in * item, _lib.ptr(raw), raw.nbytes), "h2d")
                    _lib.check(lib.topo_amd_decode_dev(d_raw.ptr + off_in * item, _lib.SOURCE_DTYPES[np.dtype(dtype)], count, scale, offset,
                                                       int(nodata is not None), 0.0 if nodata is None else nodata, d_out.ptr + 4 * off_out),
                               "decode_dev")
                    d.sync()
                    got = d_out.to_host().reshape(-1)
                    what = (np.dtype(dtype).name, scale, offset, nodata, off_in, off_out, count)
                    assert_decoded(got[off_out: off_out + count], want, what)
                    rest = np.concatenate([got[:off_out], got[off_out + count:]]).view(np.uint32)
                    assert (rest == 0x5A5A5A5A).all(), ("written outside the run", what)
    finally:
        d_raw.free()
        d_out.free()


def test_decode_dev_refuses_bad_arguments():
    lib = _lib.lib()
    buf = d.DeviceArray(1, 64)
    try:
        assert lib.topo_amd_decode_dev(buf.ptr, 9, 8, 1.0, 0.0, 0, 0.0, buf.ptr) == -1
        assert lib.topo_amd_decode_dev(buf.ptr, _lib.I16, 8, 0.0, 0.0, 0, 0.0, buf.ptr) == -1
        assert lib.topo_amd_decode_dev(buf.ptr, _lib.I16, 8, 1.0, np.inf, 0, 0.0, buf.ptr) == -1
        assert lib.topo_amd_decode_dev(buf.ptr + 1, _lib.I16, 8, 1.0, 0.0, 0, 0.0, buf.ptr + 128) == -1  # misaligned int16
    finally:
        buf.free()


@pytest.mark.parametrize("src_name", SOURCE_NAMES)
def test_upload_raw_is_decode_host(src_name):
    stored, (scale, offset, nodata), decoded = source("odd_nx", src_name)
    for many in (False, True):
        set_chunks(many)
        dev = d.DeviceArray.from_host(tda.PackedDem(stored, scale, offset, nodata))
        try:
            got = dev.to_host()
        finally:
            dev.free()
        assert_decoded(got, decoded, (src_name, many))
    odd = stored[7:1008, 3:1000]  # a view that is not contiguous: 1001 x 997
    dev = d.DeviceArray.from_host(tda.PackedDem(odd, scale, offset, nodata))
    try:
        assert_decoded(dev.to_host(), host_decode(np.ascontiguousarray(odd), scale, offset, nodata), (src_name, "view"))
    finally:
        dev.free()


# ---- the Python layer -------------------------------------------------------------------------------------------------------
class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class FakeDataset:
    def __init__(self, dem, x, y):
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(x, ("x",)), "y": FakeVar(y, ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def flat(result):
    if isinstance(result, np.ndarray):
        return [result]
    out = []
    for r in result:
        out += flat(r) if r is not None else []
    return out


@pytest.mark.parametrize("src_name", SOURCE_NAMES)
def test_packed_dem_through_the_python_functions(src_name):
    ny, nx = SHAPES["odd_nx"]
    stored, (scale, offset, nodata), decoded = source("odd_nx", src_name)
    packed = tda.PackedDem(stored, scale, offset, nodata)
    x = 2600000.0 + 30.0 * np.arange(nx)
    y = 1200000.0 - 30.0 * np.arange(ny)
    res = {"x": np.float64(30.0), "y": np.float64(-30.0)}
    calls = {
        "tpi67": lambda a: topo.tpi(a, 67),
        "tpi31_sigma": lambda a: topo.tpi(a, 31, sigma=2.0),
        "std7": lambda a: topo.std(a, 7),
        "tpi_std67": lambda a: topo.tpi_std(a, 67),
        "tpi_std_multi": lambda a: topo.tpi_std_multi(a, [5, 9, 67]),
        "dem": lambda a: topo.dem(a, 3.25),
        "gradient": lambda a: topo.gradient(a, 3.25, res),
        "sobel": lambda a: topo.sobel(a),
        "sx": lambda a: topo.sx(FakeDataset(a, x, y), 0.0, 500.0),
        "sx_multi": lambda a: topo.sx_multi(FakeDataset(a, x, y), [350.0, 0.0, 45.0], 500.0),
        "valley_ridge": lambda a: topo.valley_ridge(a, 7, "valley"),
        "fill_na_gpu": lambda a: hlp.fill_na_gpu(a, x_coords=x, min_elevation=250.0),
    }
    set_chunks(True)
    for name, call in calls.items():
        if name == "valley_ridge" and np.isnan(decoded).any():
            # numpy's mean of a raster with a NaN is NaN, which the library refuses - for the packed raster as for the array
            for a in (packed, decoded):
                with pytest.raises(_lib.TopoAmdError, match="mean nan"):
                    call(a)
            continue
        got, want = flat(call(packed)), flat(call(decoded))
        assert len(got) == len(want) and len(got) >= 1
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype, (src_name, name, k, g.dtype, w.dtype)
            assert same_bits(g, w), (src_name, name, k)
    # an ndarray of a supported dtype takes the same road without the wrapper
    if scale == 1.0 and offset == 0.0 and nodata is None:
        assert same_bits(topo.tpi(stored, 67), topo.tpi(decoded, 67))
        assert d.host_chunks() >= 3


def test_fill_na_gpu_of_a_packed_int16_is_fill_na_array_of_the_decoded_array():
    whole = orc.synthetic_dem(600, 701, seed=61, integer=True)
    a = whole.astype(np.int16)
    rng = np.random.default_rng(7)
    a[rng.random(a.shape) < 0.02] = NODATA
    a[100:140, 200:260] = NODATA
    a[300, :] = NODATA          # a row without a valid sample
    a[301, 1:] = NODATA         # and one with a single valid sample
    decoded = host_decode(a, 1.0, 0.0, NODATA)
    missing, filled = hlp.fill_na_gpu(tda.PackedDem(a, fill_value=NODATA))
    assert np.array_equal(missing, np.isnan(decoded))
    want = hlp.fill_na_array(decoded)
    assert_decoded(filled, want, "fill_na_gpu(PackedDem)")
    assert same_bits(filled, hlp.fill_na_gpu(decoded)[1])


def test_compute_tpi_on_a_float64_dataset_is_the_float32_one():
    ny, nx = 400, 517
    f = orc.synthetic_dem(ny, nx, seed=71, integer=False).astype(np.float64) + 0.123456789
    x = 2600000.0 + 30.0 * np.arange(nx)
    y = 1200000.0 - 30.0 * np.arange(ny)
    scales = [150, 200, 500, 2000]
    got = batch.compute_tpi(FakeDataset(f, x, y), scales, smth_factors=[None, None, 0.5, None], outdir=None)
    want = batch.compute_tpi(FakeDataset(f.astype(np.float32), x, y), scales, smth_factors=[None, None, 0.5, None], outdir=None)
    assert set(got) == set(want) and len(got) == 4
    for name in want:
        assert same_bits(got[name], want[name]), name
    res = batch._ResidentDem(f)
    try:
        assert res._host is None  # (nothing cast or decoded on the host until somebody asks)
        assert same_bits(res.host, f.astype(np.float32))
    finally:
        res.close()


def crc(planes):
    return tuple(zlib.crc32(np.ascontiguousarray(p).view(np.uint8)) for p in planes)


def test_two_threads_with_different_source_types():
    """In the style of tests/test_gpu_threads.py: the raw plane, the pipeline's streams and events are one set per context."""
    os.environ["TOPO_AMD_HOST_CHUNK_MB"] = "1"
    whole = orc.synthetic_dem(3100, 1001, seed=81, integer=True)
    a = whole.astype(np.int16)
    a[SEAM - 2: SEAM + 2, 100:400] = NODATA
    packed = tda.PackedDem(a, fill_value=NODATA)
    f64 = orc.synthetic_dem(700, 517, seed=82, integer=False).astype(np.float64) / 3.0
    res = {"x": np.float64(30.0), "y": np.float64(-30.0)}
    jobs = [lambda: crc(topo.tpi_std(packed, 31)), lambda: crc(topo.gradient(f64, 3.25, res))]
    serial = [crc(topo.tpi_std(host_decode(a, 1.0, 0.0, NODATA), 31)), crc(topo.gradient(f64.astype(np.float32), 3.25, res))]
    assert [job() for job in jobs] == serial
    results, errors = [[] for _ in jobs], []
    gate = threading.Barrier(len(jobs))

    def work(k, job):
        try:
            gate.wait()
            for _ in range(10):
                results[k].append(job())
        except Exception as exc:  # noqa: BLE001
            errors.append((k, repr(exc)))

    threads = [threading.Thread(target=work, args=(k, job)) for k, job in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, runs in enumerate(results):
        assert len(runs) == 10 and all(r == serial[k] for r in runs), (k, sum(r != serial[k] for r in runs))
