"""Raw sources without a GPU: the decode of a stored sample (include/topo_amd.h, "raw sources") as ``topo_amd_decode_host``
states it, against numpy bit for bit; what ``_lib.as_source`` hands to the library; ``PackedDem``; refused arguments.

The numpy side of the decode is ``np.where(raw == nodata, nan, raw.astype(f8) * scale + offset).astype(f4)`` (the
comparison taken on ``raw.astype(f8)``, as the formula says: ``(double)raw == nodata``): numpy rounds the product and the sum
in float64 one after the other and casts to nearest-even, which is the contract."""
import ctypes as C

import numpy as np
import pytest

import topo_descriptors_amd as tda
from topo_descriptors_amd import _lib, topo

DTYPES = [np.float32, np.int16, np.uint16, np.int32, np.uint8, np.float64]
# (scale, offset, nodata)
PARAMS = [(1.0, 0.0, None), (0.1, 0.0, -32768.0), (0.001, -500.25, 65535.0), (1.0 / 3.0, 7e-3, None)]
COUNTS = [0, 1, 7, 8, 9, 100003]


def samples(dtype, count, seed):
    """Seeded random samples with the type's extremes in front (and, where they fit, the nodata values of PARAMS)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=count, endpoint=True).astype(dt)
        special = [info.min, info.max, 0, 1]
        special += [v for v in (-32768, 65535, -1) if info.min <= v <= info.max]
    else:
        info = np.finfo(dt)
        a = (rng.standard_normal(count) * 3000.0).astype(dt)
        special = [info.min, info.max, info.tiny, -info.tiny, 0.0, 65535.0, -32768.0]
        if dt == np.float64:
            one = np.float64(1.0)
            ulp = np.float64(2.0 ** -23)
            special += [one + ulp / 2,                # the tie between 1 and 1 + ulp: down, to the even one
                        one + ulp + ulp / 2,          # the tie between 1 + ulp and 1 + 2 ulp: up, to the even one
                        np.nextafter(one + ulp / 2, 2.0), np.nextafter(one + ulp / 2, 0.0),  # just off the tie
                        1e39, -1e39,                  # beyond float32: +-inf
                        1e-40, -1e-40, 1.4e-45, 7e-46, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150,  # float32 denormals and their ties
                        5e-324, np.nan]
    special = np.array(special, dtype=dt)
    k = min(count, special.size)
    a[:k] = special[:k]
    return a


def numpy_decode(raw, scale, offset, nodata):
    wide = raw.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        value = (wide * scale + offset).astype(np.float32)
    if nodata is not None:
        value = np.where(wide == nodata, np.float32(np.nan), value).astype(np.float32)
    return value


def host_decode(raw, scale, offset, nodata):
    keep, raster = _lib.as_source(raw, scale, offset, nodata)
    assert keep.dtype == raw.dtype
    out = np.full(raw.shape, -12345.0, dtype=np.float32)
    rc = _lib.load().topo_amd_decode_host(C.byref(raster), raw.size, _lib.ptr(out))
    assert rc == 0, _lib.load().topo_amd_last_error()
    return out


def assert_same_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: f"{p[0]:.4g}_{p[1]:.4g}_{p[2]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_decode_host_is_numpy_bit_for_bit(dtype, params):
    scale, offset, nodata = params
    for count in COUNTS:
        raw = samples(dtype, count, seed=count + 17)
        got = host_decode(raw, scale, offset, nodata)
        want = numpy_decode(raw, scale, offset, nodata)
        assert got.shape == want.shape
        assert_same_bits(got, want, (np.dtype(dtype).name, params, count))
    if nodata is not None and np.dtype(dtype).kind in "iu":
        info = np.iinfo(dtype)
        raw = samples(dtype, 64, seed=3)
        hits = int((raw.astype(np.float64) == nodata).sum())
        assert np.isnan(host_decode(raw, scale, offset, nodata)).sum() == hits
        assert (hits > 0) == (info.min <= nodata <= info.max)  # a nodata the type cannot hold never matches


def test_plain_cast_is_astype_float32():
    for dtype in DTYPES:
        raw = samples(dtype, 5000, seed=5)
        if np.dtype(dtype) == np.float64:
            raw = raw[~np.isnan(raw)]
        with np.errstate(over="ignore"):
            want = raw.astype(np.float32)
        assert_same_bits(host_decode(raw, 1.0, 0.0, None), want, np.dtype(dtype).name)


def test_float64_nan_nodata_means_none():
    raw = np.array([1.5, np.nan, -3.25, 0.0])
    got = host_decode(raw, 2.0, 1.0, np.nan)
    assert_same_bits(got, np.array([4.0, np.nan, -5.5, 1.0], dtype=np.float32), "nan nodata")


def test_nodata_becomes_numpys_nan():
    got = host_decode(np.array([-32768, 5], dtype=np.int16), 0.1, 0.0, -32768)
    assert got.view(np.uint32)[0] == 0x7FC00000 and got[1] == np.float32(0.5)


def test_float32_as_stored_keeps_every_bit():
    raw = np.array([0x80000000, 0x7FC00001, 0xFF800000, 0x00000001, 0x7FA00000], dtype=np.uint32).view(np.float32)
    assert np.array_equal(host_decode(raw, 1.0, 0.0, None).view(np.uint32), raw.view(np.uint32))


def test_as_source_keeps_supported_dtypes():
    for code, dtype in enumerate(DTYPES):
        a = np.arange(12, dtype=dtype).reshape(3, 4)
        keep, raster = _lib.as_source(a)
        assert keep is a or np.shares_memory(keep, a)
        assert keep.dtype == np.dtype(dtype) and raster.dtype == code == _lib.SOURCE_DTYPES[np.dtype(dtype)]
        assert raster.data == a.ctypes.data and raster.has_nodata == 0
        assert (raster.scale, raster.offset) == (1.0, 0.0)
        view = np.arange(24, dtype=dtype).reshape(4, 6)[:, ::2]  # not contiguous: copied, same dtype
        keep, raster = _lib.as_source(view, 0.5, 2.0, -1)
        assert keep.dtype == np.dtype(dtype) and keep.flags.c_contiguous and not np.shares_memory(keep, view)
        assert np.array_equal(keep, view) and raster.data == keep.ctypes.data
        assert (raster.scale, raster.offset, raster.nodata, raster.has_nodata) == (0.5, 2.0, -1.0, 1)


def test_as_source_falls_back_to_float32():
    for a in (np.arange(6, dtype=np.int64).reshape(2, 3), np.arange(6, dtype=np.float16).reshape(2, 3),
              np.arange(6, dtype=np.int16).reshape(2, 3).astype(np.dtype(np.int16).newbyteorder()),
              np.arange(6, dtype=">f8").reshape(2, 3) if np.little_endian else np.arange(6, dtype="<f8").reshape(2, 3),
              np.array([[True, False, True]])):
        keep, raster = _lib.as_source(a)
        assert keep.dtype == np.float32 and raster.dtype == _lib.F32
        assert np.array_equal(keep, a.astype(np.float32))


def test_packed_dem_plumbing():
    raw = np.array([[10, -32768, 30], [40, 50, 60]], dtype=np.int16)
    p = tda.PackedDem(raw, scale_factor=0.1, add_offset=100.0, fill_value=-32768)
    assert p.shape == (2, 3) and p.ndim == 2 and p.dtype == np.float32 and p.values.dtype == np.int16
    keep, raster = p.source()
    assert keep.dtype == np.int16 and raster.dtype == _lib.I16
    assert (raster.scale, raster.offset, raster.nodata, raster.has_nodata) == (0.1, 100.0, -32768.0, 1)
    assert_same_bits(p.decode(), numpy_decode(raw, 0.1, 100.0, -32768.0), "PackedDem.decode")
    plain = tda.PackedDem(raw)
    assert plain.source()[1].has_nodata == 0 and plain.fill_value is None
    values, rewrap = topo._unwrap(p)
    assert values is p and rewrap("x") == "x"
    with pytest.raises(ValueError):
        topo._check_2d(tda.PackedDem(np.zeros(4, dtype=np.int16)), "tpi")

    class Var:  # a DataArray-like whose values are packed
        values = p

        def copy(self, data):
            return ("wrapped", data)
    values, rewrap = topo._unwrap(Var())
    assert values is p and rewrap(1) == ("wrapped", 1)


def raster_of(a, dtype=None, scale=1.0, offset=0.0):
    return _lib.Raster(a.ctypes.data, _lib.SOURCE_DTYPES[a.dtype] if dtype is None else dtype, 0, scale, offset, 0.0)


@pytest.mark.parametrize("what,kw", [("dtype 6", dict(dtype=6)), ("dtype -1", dict(dtype=-1)), ("scale 0", dict(scale=0.0)),
                                     ("scale inf", dict(scale=np.inf)), ("scale nan", dict(scale=np.nan)),
                                     ("offset inf", dict(offset=-np.inf)), ("offset nan", dict(offset=np.nan))])
def test_bad_sources_are_refused(what, kw):
    lib = _lib.load()
    a = np.arange(8, dtype=np.int16)
    out = np.zeros(8, dtype=np.float32)
    r = raster_of(a, **kw)
    assert lib.topo_amd_decode_host(C.byref(r), a.size, _lib.ptr(out)) == -1, what  # TOPO_AMD_EINVAL
    assert lib.topo_amd_last_error() != b""
    assert not out.any()


def test_null_source_is_refused():
    lib = _lib.load()
    out = np.zeros(8, dtype=np.float32)
    assert lib.topo_amd_decode_host(None, 8, _lib.ptr(out)) == -1
    r = _lib.Raster(None, _lib.I16, 0, 1.0, 0.0, 0.0)
    assert lib.topo_amd_decode_host(C.byref(r), 8, _lib.ptr(out)) == -1


def test_raw_entry_points_need_an_initialised_library():
    lib = _lib.load()
    if lib.topo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    a = np.zeros((8, 8), dtype=np.int16)
    out = np.zeros((8, 8), dtype=np.float32)
    r = raster_of(a)
    assert lib.topo_amd_tpi_raw(C.byref(r), 8, 8, 3, 0.0, _lib.ptr(out)) != 0
    assert b"topo_amd_init" in lib.topo_amd_last_error()
    with pytest.raises(_lib.TopoAmdError):
        topo.tpi(tda.PackedDem(a, fill_value=-32768), 3)
