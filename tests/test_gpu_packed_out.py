"""Packed result planes on the GPU (include/topo_amd.h, "packed result planes"): every plane of a ``*_packed`` call must be, code
for code and counter for counter, the numpy twin (written here, independent of the library) of the float32 plane the ``*_raw``
call gives.

Every ``*_packed`` entry point x two sources x two shapes (3100 x 1999: a row chunk's packed rows start off the 16-byte phase;
3100 x 1024) x {one chunk, three chunks (``TOPO_AMD_HOST_CHUNK_MB=1``: 960 + 960 + 1180 rows)} x {pageable, page-locked
arrays}; an all-float32 ``*_packed`` call against the ``*_raw`` call; ``topo_amd_encode_dev`` against ``topo_amd_encode_host`` at
counts and offsets that are not multiples of a 16-byte group, with guard bytes; the Python layer; two threads.  No tolerance
anywhere."""
import ctypes as C
import os
import threading
import zlib

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, batch, device as d, topo  # noqa: E402

NY = 3100
SHAPES = {"odd_nx": (NY, 1999), "nx_mult_of_4": (NY, 1024)}
SEAM = 960  # first row of the second chunk
ENV = ("TOPO_AMD_HOST_CHUNK_MB", "TOPO_AMD_HOST_PIPELINE", "TOPO_AMD_HOST_DOWNLOADS")
NODATA = -32768
HALF_NAN = 0x7E00


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
    a = whole.astype(np.int16)
    a[100, 200] = NODATA                                # a void of one pixel,
    a[500:540, 300:340] = NODATA                        # a block of 40,
    a[SEAM - 3: SEAM + 4, nx // 3: nx // 3 + 200] = NODATA  # and a run lying across the first chunk seam
    return {"metres_i16_nodata": (a, 1.0, 0.0, NODATA), "scaled_f32": (frac.copy(), 0.3048, -12.5, None)}


SOURCE_NAMES = ["metres_i16_nodata", "scaled_f32"]
_CACHE = {}


def source(shape_name, name):
    if shape_name not in _CACHE:
        _CACHE.clear()  # (one shape's rasters at a time)
        _CACHE[shape_name] = make_sources(*SHAPES[shape_name])
    return _CACHE[shape_name][name]


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


# ---- the twin: numpy, independent of the library ------------------------------------------------------------------------------
def twin(v, packing):
    """(codes, missing, saturated) of a float32 array under a ``Packing`` (``None``: float32 as it is)"""
    if packing is None:
        return v, 0, 0
    nan = np.isnan(v)
    with np.errstate(all="ignore"):
        if packing.dtype == np.float16:
            code = v.astype(np.float16)
            code.view(np.uint16)[nan] = HALF_NAN
            return code, int(nan.sum()), int((np.isfinite(v) & np.isinf(code)).sum())
        info = np.iinfo(packing.dtype)
        nodata = int(packing.fill_value)
        lo, hi = (info.min + 1, info.max) if nodata == info.min else (info.min, info.max - 1)
        q = np.rint((v.astype(np.float64) - packing.add_offset) / packing.scale_factor)
        code = np.where(nan, nodata, np.clip(q, lo, hi)).astype(packing.dtype)
        return code, int(nan.sum()), int((~nan & ((q < lo) | (q > hi))).sum())


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


TPI_DM = tda.Packing(np.int16, 0.1, 0.0, -32768)       # TPI in decimetres: +-3276.7 m
TPI_CM = tda.Packing(np.int16, 0.01, 0.0, -32768)      # in centimetres: +-327.67 m, the zero-padded border saturates
STD_5CM = tda.Packing(np.uint16, 0.05, 0.0, 65535)     # STD and elevations in units of 5 cm: 0 ... 3276.7 m
HALF = tda.Packing(np.float16)
SLOPE = tda.Packing(np.uint8, 0.5, 0.0, 255)           # degrees / 2
ASPECT = tda.Packing(np.uint16, 0.01, 0.0, 65535)      # centidegrees
SX_CDEG = tda.Packing(np.int16, 0.01, 0.0, -32768)     # centidegrees


# ---- the calls: name -> (packing per plane, raw(lib, src, buffers), packed(lib, src, plane array)) ---------------------------
def tables(shape):
    ny, nx = shape
    sectors = [d.sx_offsets(a, 500.0, 30.0, -30.0) for a in (350.0, 0.0, 45.0)]
    w, dj, di, dist = sectors[1]
    dj, di = np.ascontiguousarray(dj, dtype=np.int32), np.ascontiguousarray(di, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    first, mdj, mdi, mdist, mwin = d.pack_sectors(sectors)
    sizes = np.array([5, 9, 67], dtype=np.int32)
    sigmas = np.zeros(3)
    rx, ry = np.array([30.0]), np.array([-30.0])
    i32, f64 = _lib._i32p, _lib._f64p
    ref = C.byref

    def at(planes, k):  # topo_amd_plane* of the planes from k on
        return C.cast(C.byref(planes, k * C.sizeof(_lib.Plane)), _lib._pp)

    def tpi(size):
        return ([TPI_DM], lambda lib, s, o: lib.topo_amd_tpi_raw(s, ny, nx, size, 0.0, vp(o[0])),
                lambda lib, s, p: lib.topo_amd_tpi_std_packed(s, ny, nx, size, 0.0, ref(p[0]), None))

    def multi_raw(lib, s, o):
        t = (C.c_void_p * 3)(*[b.bytes.ctypes.data for b in o[:3]])
        sd = (C.c_void_p * 3)(*[b.bytes.ctypes.data for b in o[3:]])
        return lib.topo_amd_tpi_std_multi_raw(s, ny, nx, 3, sizes.ctypes.data_as(i32), sigmas.ctypes.data_as(f64), t, sd)

    def sx_multi_raw(lib, s, o):
        planes = (C.c_void_p * 3)(*[b.bytes.ctypes.data for b in o])
        return lib.topo_amd_sx_multi_raw(s, ny, nx, 3, first.ctypes.data_as(i32), mdj.ctypes.data_as(i32), mdi.ctypes.data_as(i32),
                                         mdist.ctypes.data_as(f64), mwin.ctypes.data_as(i32), 10.0, planes)

    sx_args = (dj.ctypes.data_as(i32), di.ctypes.data_as(i32), dist.ctypes.data_as(f64), dist.size, int(w), 10.0)
    return {
        "tpi7": tpi(7),
        "tpi67": tpi(67),
        "tpi67_cm": ([TPI_CM],) + tpi(67)[1:],
        "tpi_std67": ([TPI_DM, STD_5CM], lambda lib, s, o: lib.topo_amd_tpi_std_raw(s, ny, nx, 67, 0.0, vp(o[0]), vp(o[1])),
                      lambda lib, s, p: lib.topo_amd_tpi_std_packed(s, ny, nx, 67, 0.0, ref(p[0]), ref(p[1]))),
        "tpi_std_multi": ([TPI_DM, None, TPI_DM, STD_5CM, HALF, STD_5CM], multi_raw,
                          lambda lib, s, p: lib.topo_amd_tpi_std_multi_packed(s, ny, nx, 3, sizes.ctypes.data_as(i32),
                                                                              sigmas.ctypes.data_as(f64), at(p, 0), at(p, 3))),
        "gauss3.25": ([STD_5CM], lambda lib, s, o: lib.topo_amd_gauss_raw(s, ny, nx, 3.25, 3.25, vp(o[0])),
                      lambda lib, s, p: lib.topo_amd_gauss_packed(s, ny, nx, 3.25, 3.25, ref(p[0]))),
        "gradient3.25": ([HALF, HALF, SLOPE, ASPECT],
                         lambda lib, s, o: lib.topo_amd_gradient_raw(s, ny, nx, 3.25, 1.0, _lib.RES_SCALAR, _lib.ptr(rx), _lib.ptr(ry),
                                                                     *[vp(b) for b in o]),
                         lambda lib, s, p: lib.topo_amd_gradient_packed(s, ny, nx, 3.25, 1.0, _lib.RES_SCALAR, _lib.ptr(rx),
                                                                        _lib.ptr(ry), *[ref(p[k]) for k in range(4)])),
        "sx": ([SX_CDEG], lambda lib, s, o: lib.topo_amd_sx_raw(s, ny, nx, *sx_args, vp(o[0])),
               lambda lib, s, p: lib.topo_amd_sx_packed(s, ny, nx, *sx_args, ref(p[0]))),
        "sx_multi": ([SX_CDEG] * 3, sx_multi_raw,
                     lambda lib, s, p: lib.topo_amd_sx_multi_packed(s, ny, nx, 3, first.ctypes.data_as(i32), mdj.ctypes.data_as(i32),
                                                                    mdi.ctypes.data_as(i32), mdist.ctypes.data_as(f64),
                                                                    mwin.ctypes.data_as(i32), 10.0, at(p, 0))),
    }


CASE_NAMES = ["tpi7", "tpi67", "tpi67_cm", "tpi_std67", "tpi_std_multi", "gauss3.25", "gradient3.25", "sx", "sx_multi"]
_TABLES = {}


def raster_of(buf, stored, scale, offset, nodata):
    return _lib.Raster(buf.bytes.ctypes.data, _lib.SOURCE_DTYPES[stored.dtype], int(nodata is not None), scale, offset,
                       0.0 if nodata is None else float(nodata))


def plane_structs(packings, buffers):
    structs = [(q or tda.Packing(np.float32)).struct(b.bytes.ctypes.data) for q, b in zip(packings, buffers)]
    for s in structs:
        s.missing = s.saturated = 12345  # (the call sets them, also to 0)
    return _lib.plane_array(structs)


def elem(packing):
    return 4 if packing is None else packing.dtype.itemsize


@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("src_name", SOURCE_NAMES)
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_packed_call_is_the_twin_of_the_raw_call(shape_name, src_name, case):
    shape = SHAPES[shape_name]
    ny, nx = shape
    stored, scale, offset, nodata = source(shape_name, src_name)
    if shape_name not in _TABLES:
        _TABLES[shape_name] = tables(shape)
    packings, raw_call, packed_call = _TABLES[shape_name][case]
    lib = _lib.lib()
    # the float32 planes, once, and their twins
    set_chunks(True)
    src_buf = Buffer(stored.nbytes, False)
    src_buf.bytes[:] = stored.reshape(-1).view(np.uint8)
    floats = [Buffer(ny * nx * 4, False) for _ in packings]
    rc_want = raw_call(lib, C.byref(raster_of(src_buf, stored, scale, offset, nodata)), floats)
    assert rc_want in (0, -6), (case, rc_want, lib.topo_amd_last_error())
    want = [twin(b.bytes.view(np.float32), q) for b, q in zip(floats, packings)]
    for k, ((codes, missing, saturated), q) in enumerate(zip(want, packings)):
        print(case, src_name, shape_name, "plane", k, q, "missing", missing, "saturated", saturated)
    if case in ("tpi7", "tpi67", "tpi_std67"):
        assert want[0][2] == 0  # |TPI| <= 1928 m on both DEMs (the zero-padded border): inside +-3276.7 m
        if src_name == "metres_i16_nodata":
            assert want[0][1] > 0  # (the voids, one of them across the first chunk seam)
    if case == "tpi67_cm":
        assert want[0][2] > 0  # the border pixels saturate at +-327.67 m
    for many in (False, True):
        set_chunks(many)
        for pinned in (False, True):
            raw = Buffer(stored.nbytes, pinned)
            raw.bytes[:] = src_buf.bytes
            outs = [Buffer(ny * nx * elem(q), pinned) for q in packings]
            try:
                for b in outs:
                    b.bytes[:] = 0xA5
                planes = plane_structs(packings, outs)
                rc = packed_call(lib, C.byref(raster_of(raw, stored, scale, offset, nodata)), planes)
                where = (shape_name, src_name, case, "chunks" if many else "one chunk", "pinned" if pinned else "pageable")
                assert rc == rc_want, (where, rc, lib.topo_amd_last_error())
                chunks = d.host_chunks()
                assert chunks == 1 if not many else chunks >= 3, (where, chunks)
                for k, (b, (codes, missing, saturated)) in enumerate(zip(outs, want)):
                    got = b.bytes.view(codes.dtype)
                    if not np.array_equal(got.view(np.uint8), codes.reshape(-1).view(np.uint8)):
                        bad = np.flatnonzero(got.view(codes.dtype.str.replace("f", "u")) != codes.reshape(-1).view(codes.dtype.str.replace("f", "u")))
                        raise AssertionError((where, "plane", k, "samples that differ", bad.size, "first", bad[:5]))
                    assert (planes[k].missing, planes[k].saturated) == (missing, saturated), (where, "plane", k)
            finally:
                raw.free()
                for b in outs:
                    b.free()


@pytest.mark.parametrize("case", ["tpi67", "tpi_std_multi", "gradient3.25", "sx_multi"])
def test_packed_call_with_float32_planes_is_the_raw_call(case):
    shape_name = "odd_nx"
    ny, nx = SHAPES[shape_name]
    stored, scale, offset, nodata = source(shape_name, "metres_i16_nodata")
    if shape_name not in _TABLES:
        _TABLES[shape_name] = tables(SHAPES[shape_name])
    packings, raw_call, packed_call = _TABLES[shape_name][case]
    plain = [None] * len(packings)
    lib = _lib.lib()
    src_buf = Buffer(stored.nbytes, False)
    src_buf.bytes[:] = stored.reshape(-1).view(np.uint8)
    raster = raster_of(src_buf, stored, scale, offset, nodata)
    for many in (False, True):
        set_chunks(many)
        want = [Buffer(ny * nx * 4, False) for _ in plain]
        got = [Buffer(ny * nx * 4, False) for _ in plain]
        for b in want + got:
            b.bytes[:] = 0xA5
        rc_want = raw_call(lib, C.byref(raster), want)
        chunks_want = d.host_chunks()
        planes = plane_structs(plain, got)
        assert packed_call(lib, C.byref(raster), planes) == rc_want
        assert d.host_chunks() == chunks_want and (chunks_want >= 3) == many
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g.bytes, w.bytes), (case, many, k)
            assert (planes[k].missing, planes[k].saturated) == (0, 0)


# ---- the encode on its own ----------------------------------------------------------------------------------------------------
ENCODINGS = {"int16": TPI_DM, "uint16": tda.Packing(np.uint16, 0.01, -500.25, 65535), "uint8": tda.Packing(np.uint8, 1.0 / 3.0, 7e-3, 0),
             "float16": HALF}


def float_samples(count, packing, seed):
    rng = np.random.default_rng(seed)
    if packing.dtype == np.float16:
        a = (rng.standard_normal(count) * 10.0 ** rng.uniform(-9, 5.5, count)).astype(np.float32)
    else:
        info = np.iinfo(packing.dtype)
        span = info.max - info.min
        codes = rng.uniform(info.min - 0.1 * span, info.max + 0.1 * span, count)
        codes[::3] = np.floor(codes[::3]) + 0.5  # ties, as far as float32 keeps them
        a = (codes * packing.scale_factor + packing.add_offset).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 65520.0, 3e38, -3e38, 1e-40, 2.0 ** -25], dtype=np.float32)
    if count >= 7:
        at = rng.choice(count, size=min(count, 3 * special.size) // 3, replace=False)
        a[at] = special[: at.size]
    return a


@pytest.mark.parametrize("name", sorted(ENCODINGS))
def test_encode_dev_is_encode_host(name):
    packing = ENCODINGS[name]
    lib = _lib.lib()
    item = packing.dtype.itemsize
    room = 100003 + 64
    d_in = d.DeviceArray(1, room, dtype=np.float32)
    d_out = d.DeviceArray(1, room * item, dtype=np.uint8)
    try:
        for count in (1, 7, 8, 9, 1023, 4097, 100003):
            v = float_samples(count, packing, seed=count)
            want = _lib.encode_host(v, packing)
            for off_in in range(4):
                _lib.check(lib.topo_amd_memcpy_h2d(d_in.ptr + 4 * off_in, _lib.ptr(v), v.nbytes), "h2d")
                for off_out in range(8):
                    _lib.check(lib.topo_amd_memset(d_out.ptr, 0x5A, d_out.nbytes), "memset")
                    plane = packing.struct(d_out.ptr + off_out * item)
                    plane.missing = plane.saturated = 999
                    _lib.check(lib.topo_amd_encode_dev(d_in.ptr + 4 * off_in, count, C.byref(plane)), "encode_dev")
                    got = d_out.to_host().reshape(-1)  # (the counters are valid, so the plane is written: no sync needed)
                    what = (name, count, off_in, off_out)
                    lo, hi = off_out * item, (off_out + count) * item
                    assert np.array_equal(got[lo:hi], want.values.view(np.uint8)), what
                    assert (got[:lo] == 0x5A).all() and (got[hi:] == 0x5A).all(), ("written outside the run", what)
                    assert (plane.missing, plane.saturated) == (want.missing, want.saturated), what
        assert want.missing > 0 and want.saturated > 0
    finally:
        d_in.free()
        d_out.free()


def test_encode_dev_refuses_bad_arguments():
    lib = _lib.lib()
    buf = d.DeviceArray(1, 64)
    out = d.DeviceArray(1, 64)
    try:
        def call(dtype, scale, offset, has_nodata, nodata, at=0):
            plane = _lib.Plane(out.ptr + at, dtype, has_nodata, scale, offset, nodata, 0, 0)
            return lib.topo_amd_encode_dev(buf.ptr, 8, C.byref(plane))
        assert call(_lib.I16, 0.1, 0.0, 1, -32768.0) == 0
        assert call(_lib.I16, 0.1, 0.0, 1, -9999.0) == -1   # nodata inside the range
        assert call(_lib.I16, 0.1, 0.0, 0, 0.0) == -1       # no nodata
        assert call(_lib.F16, 0.5, 0.0, 0, 0.0) == -1
        assert call(_lib.F32, 0.5, 0.0, 0, 0.0) == -1
        assert call(_lib.U8, 0.0, 0.0, 1, 255.0) == -1
        assert call(_lib.I32, 1.0, 0.0, 1, 0.0) == -1
        assert call(7, 1.0, 0.0, 0, 0.0) == -1
        assert call(_lib.I16, 0.1, 0.0, 1, -32768.0, at=1) == -1  # misaligned int16
    finally:
        buf.free()
        out.free()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
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


def assert_twin(plane, array, packing, what):
    codes, missing, saturated = twin(np.asarray(array, dtype=np.float32), packing)
    if packing is None:
        assert isinstance(plane, np.ndarray) and same_bits(plane, array), what
        return
    assert isinstance(plane, tda.PackedPlane), what
    assert same_bits(plane.values, codes), what
    assert (plane.missing, plane.saturated) == (missing, saturated), what
    assert (plane.scale_factor, plane.add_offset, plane.fill_value) == (packing.scale_factor, packing.add_offset, packing.fill_value)


def small_dem(ny=1100, nx=701, seed=91):
    a = orc.synthetic_dem(ny, nx, seed=seed, integer=True).astype(np.int16)
    a[300:310, 100:160] = NODATA
    return tda.PackedDem(a, fill_value=NODATA)


def test_pack_through_the_python_functions():
    dem = small_dem()
    ny, nx = dem.shape
    x = 2600000.0 + 30.0 * np.arange(nx)
    y = 1200000.0 - 30.0 * np.arange(ny)
    res = {"x": np.float64(30.0), "y": np.float64(-30.0)}
    assert_twin(topo.tpi(dem, 67, pack=TPI_DM), topo.tpi(dem, 67), TPI_DM, "tpi")
    assert_twin(topo.tpi(dem, 31, sigma=2.0, pack=HALF), topo.tpi(dem, 31, sigma=2.0), HALF, "tpi sigma")
    got = topo.std(dem, 7, pack=STD_5CM)
    assert got.values.dtype == np.uint16  # (not widened)
    assert_twin(got, topo.std(dem, 7).astype(np.float32), STD_5CM, "std")
    t, s = topo.tpi_std(dem, 31, pack=(TPI_DM, None))
    wt, ws = topo.tpi_std(dem, 31)
    assert_twin(t, wt, TPI_DM, "tpi_std tpi")
    assert s.dtype == np.float64 and same_bits(s, ws)
    tpis, stds = topo.tpi_std_multi(dem, [5, 9, 67], pack={"tpi": [TPI_DM, None, HALF], "std": STD_5CM})
    wtpis, wstds = topo.tpi_std_multi(dem, [5, 9, 67])
    for k, q in enumerate([TPI_DM, None, HALF]):
        assert_twin(tpis[k], wtpis[k], q, ("multi tpi", k))
        assert_twin(stds[k], wstds[k].astype(np.float32), STD_5CM, ("multi std", k))
    assert_twin(topo.dem(dem, 3.25, pack=STD_5CM), topo.dem(dem, 3.25), STD_5CM, "dem")
    pack = {"dx": HALF, "dy": HALF, "slope": SLOPE, "aspect": ASPECT}
    for name, g, w in zip(topo.GRADIENT_PLANES, topo.gradient(dem, 3.25, res, pack=pack), topo.gradient(dem, 3.25, res)):
        assert_twin(g, w, pack[name], ("gradient", name))
    g = topo.gradient(dem, 3.25, res, pack={"slope": SLOPE})
    assert [type(p) for p in g] == [np.ndarray, np.ndarray, tda.PackedPlane, np.ndarray]
    ds = FakeDataset(dem, x, y)
    assert_twin(topo.sx(ds, 0.0, 500.0, pack=SX_CDEG), topo.sx(ds, 0.0, 500.0), SX_CDEG, "sx")
    az = [350.0, 0.0, 45.0]
    for k, (g, w) in enumerate(zip(topo.sx_multi(ds, az, 500.0, pack=SX_CDEG), topo.sx_multi(ds, az, 500.0))):
        assert_twin(g, w, SX_CDEG, ("sx_multi", k))
    for k, (g, w) in enumerate(zip(topo.sx_multi(ds, az, 500.0, pack=[SX_CDEG, None, HALF]), topo.sx_multi(ds, az, 500.0))):
        assert_twin(g, w, [SX_CDEG, None, HALF][k], ("sx_multi mixed", k))
    # a raster that is nothing but frame: the plane is made and packed on the host
    tiny = FakeDataset(np.zeros((20, 20), np.float32), x[:20], y[:20])
    assert_twin(topo.sx(tiny, 0.0, 500.0, pack=SX_CDEG), topo.sx(tiny, 0.0, 500.0), SX_CDEG, "sx frame")


def test_a_packed_smoothed_dem_goes_back_in_as_a_source():
    dem = small_dem(seed=92)
    smooth = topo.dem(dem, 3.25, pack=STD_5CM)
    assert smooth.values.dtype == np.uint16 and smooth.missing > 0
    assert same_bits(topo.tpi(smooth, 67), topo.tpi(smooth.decode(), 67))
    half = topo.dem(dem, 3.25, pack=HALF)
    assert same_bits(topo.tpi(half, 7), topo.tpi(half.decode(), 7))


def test_device_array_to_packed_is_the_twin_of_to_host():
    a = orc.synthetic_dem(500, 333, seed=93, integer=False)
    a[17, 5:40] = np.nan
    dev = d.DeviceArray.from_host(a)
    try:
        for q in (STD_5CM, TPI_CM, HALF, tda.Packing(np.uint8, 16.0, 0.0, 0)):
            assert_twin(dev.to_packed(q), dev.to_host(), q, q)
            assert_twin(dev.to_packed(q, 3, 101), dev.to_host(3, 101), q, (q, "rows"))
        with pytest.raises(ValueError):
            d.DeviceArray(2, 2, dtype=np.float64)
        for t in (np.int16, np.uint16, np.float16):
            d.DeviceArray(2, 3, dtype=t).free()
    finally:
        dev.free()


def test_compute_tpi_packed_writes_npz_and_sets_the_fill_code(tmp_path):
    ny, nx = 400, 517
    f = orc.synthetic_dem(ny, nx, seed=71, integer=False)
    x = 2600000.0 + 30.0 * np.arange(nx)
    y = 1200000.0 - 30.0 * np.arange(ny)
    ds = FakeDataset(f, x, y)
    mask = np.zeros((ny, nx), dtype=bool)
    mask[10:20, 30:50] = True
    ind_nans = np.where(mask)
    scales = [150, 200, 2000]
    plain_dir, packed_dir = tmp_path / "plain", tmp_path / "packed"
    want = batch.compute_tpi(ds, scales, ind_nans=ind_nans, outdir=str(plain_dir))
    got = batch.compute_tpi(ds, scales, ind_nans=ind_nans, outdir=str(packed_dir), pack=TPI_DM)
    assert set(got) == set(want) and len(got) == 3
    for name in want:
        assert np.isnan(want[name][mask]).all()
        assert same_bits(np.load(plain_dir / f"topo_{name}.npy"), want[name])  # (the unpacked call: as before)
        assert not (plain_dir / f"topo_{name}.npz").exists() and not (packed_dir / f"topo_{name}.npy").exists()
        codes, missing, saturated = twin(want[name], TPI_DM)
        plane = got[name]
        assert isinstance(plane, tda.PackedPlane) and same_bits(plane.values, codes)
        assert (plane.values[mask] == -32768).all() and plane.missing == missing == mask.sum() and plane.saturated == saturated
        with np.load(packed_dir / f"topo_{name}.npz") as z:
            assert same_bits(z["values"], codes)
            assert (float(z["scale_factor"]), float(z["add_offset"]), float(z["fill_value"])) == (0.1, 0.0, -32768.0)
    halves = batch.compute_std(ds, [200], ind_nans=ind_nans, outdir=None, pack=HALF)
    (name, plane), = halves.items()
    assert plane.values.dtype == np.float16 and np.isnan(plane.values[mask]).all() and plane.missing == mask.sum()
    grads = batch.compute_gradient(ds, [200], ind_nans=ind_nans, outdir=None, pack={"slope": SLOPE, "aspect": ASPECT})
    kinds = [type(v) for v in grads.values()]
    assert kinds == [np.ndarray, np.ndarray, tda.PackedPlane, tda.PackedPlane]


def crc(planes):
    return tuple(zlib.crc32(np.ascontiguousarray(getattr(p, "values", p)).view(np.uint8)) for p in planes) + \
        tuple((p.missing, p.saturated) for p in planes if hasattr(p, "missing"))


def test_two_threads_with_different_packings():
    """In the style of tests/test_gpu_threads.py: the packed planes and the counters are one set per context."""
    os.environ["TOPO_AMD_HOST_CHUNK_MB"] = "1"
    whole = orc.synthetic_dem(3100, 1001, seed=81, integer=True)
    a = whole.astype(np.int16)
    a[SEAM - 2: SEAM + 2, 100:400] = NODATA
    packed = tda.PackedDem(a, fill_value=NODATA)
    f32 = orc.synthetic_dem(700, 517, seed=82, integer=False) / 3.0
    res = {"x": np.float64(30.0), "y": np.float64(-30.0)}
    jobs = [lambda: crc(topo.tpi_std(packed, 31, pack=(TPI_DM, STD_5CM))), lambda: crc(topo.gradient(f32, 3.25, res, pack=HALF))]
    serial = [job() for job in jobs]
    t, s = topo.tpi_std(packed, 31)
    assert serial[0][:2] == crc([twin(t, TPI_DM)[0], twin(s.astype(np.float32), STD_5CM)[0]])
    assert d.host_chunks() >= 3
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
