"""Packed result planes on the host (include/topo_amd.h, "packed result planes"): ``topo_amd_encode_host`` - the CPU statement
of the encode the GPU runs behind every row chunk - against a numpy twin written here, bit for bit and counter for counter;
the round trip through ``PackedPlane.decode()``; every refusal; the ctypes plumbing.  No GPU needed: nothing here launches a
kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import topo_descriptors_amd as tda
from topo_descriptors_amd import _lib, topo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_NAN = 0x7E00
INT_TYPES = [np.int16, np.uint16, np.uint8]
PACKINGS = [(1.0, 0.0), (0.1, 0.0), (0.01, -500.25), (1.0 / 3.0, 7e-3), (-0.25, 12.5)]


# ---- the twin: numpy, independent of the library ------------------------------------------------------------------------------
def code_range(dtype, nodata):
    info = np.iinfo(dtype)
    return (info.min + 1, info.max) if nodata == info.min else (info.min, info.max - 1)


def twin(v, dtype, scale=1.0, offset=0.0, nodata=None):
    """(codes, missing, saturated) of float32 samples ``v``"""
    dtype = np.dtype(dtype)
    nan = np.isnan(v)
    with np.errstate(all="ignore"):
        if dtype == np.float16:
            code = v.astype(np.float16)
            code.view(np.uint16)[nan] = HALF_NAN
            return code, int(nan.sum()), int((np.isfinite(v) & np.isinf(code)).sum())
        lo, hi = code_range(dtype, nodata)
        q = np.rint((v.astype(np.float64) - offset) / scale)
        code = np.where(nan, nodata, np.clip(q, lo, hi)).astype(dtype)
        return code, int(nan.sum()), int((~nan & ((q < lo) | (q > hi))).sum())


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


NANS = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FC12345, 0xFFFFFFFF, 0x7FBFFFFF])
EDGES = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf], np.float32), f32([1, 0x80000001, 0x007FFFFF, 0x807FFFFF]),
                        np.array([np.finfo(np.float32).max, np.finfo(np.float32).min, np.finfo(np.float32).tiny,
                                  -np.finfo(np.float32).tiny], np.float32)])


def integer_samples(dtype, scale, offset, nodata, seed):
    info = np.iinfo(dtype)
    lo, hi = code_range(dtype, nodata)
    k = np.arange(-6, 7, dtype=np.float64)
    # k + 0.5 for k of both parities, around 0, around both ends of the range and around the middle (exact ties for the packing
    # (1, 0), whatever float32 leaves of them for the others); q exactly lo, hi, lo - 1, hi + 1; the value that rounds onto nodata
    codes = np.concatenate([k + 0.5, lo + k + 0.5, hi + k + 0.5, (lo + hi) // 2 + k + 0.5, lo + k, hi + k,
                            [lo, hi, lo - 1, hi + 1, nodata, info.min, info.max, info.min - 1, info.max + 1]])
    rng = np.random.default_rng(seed)
    span = hi - lo
    codes = np.concatenate([codes, rng.uniform(lo - 0.05 * span, hi + 0.05 * span, 100000)])
    v = (codes * scale + offset).astype(np.float32)
    return np.concatenate([v, EDGES, NANS])


def half_samples(seed):
    ulp = np.float32(2.0 ** -25) * np.float32(2.0 ** -23)
    edge = np.array([65504.0, 65519.99, 65520.0, 65536.0, 2.0 ** -24, 2.0 ** -25, np.float32(2.0 ** -25) + ulp, 2.0 ** -14,
                     2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                     1.0 + 2.0 ** -11 + 2.0 ** -23, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2047.5, 2048.5, 1e-8, 1e6], dtype=np.float32)
    rng = np.random.default_rng(seed)
    rnd = (rng.standard_normal(100000) * 10.0 ** rng.uniform(-9, 6, 100000)).astype(np.float32)
    return np.concatenate([edge, -edge, EDGES, NANS, rnd])


def encode_host(v, dtype, scale=1.0, offset=0.0, nodata=None):
    """(status, codes, missing, saturated) of the library's host encode"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.empty(v.shape, dtype=dtype)
    out.view(np.uint8)[...] = 0x5A
    plane = _lib.Plane(out.ctypes.data, _lib.PLANE_DTYPES[np.dtype(dtype)], int(nodata is not None), scale, offset,
                       0.0 if nodata is None else float(nodata), 77, 77)
    rc = _lib.load().topo_amd_encode_host(_lib.ptr(v), v.size, C.byref(plane))
    return rc, out, plane.missing, plane.saturated


# ---- topo_amd_encode_host against the twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing", PACKINGS, ids=lambda p: f"{p[0]:.3g}_{p[1]:.3g}")
@pytest.mark.parametrize("top", [False, True], ids=["nodata_lowest", "nodata_highest"])
@pytest.mark.parametrize("dtype", INT_TYPES, ids=lambda t: np.dtype(t).name)
def test_encode_host_integer_types_against_the_twin(dtype, top, packing):
    scale, offset = packing
    info = np.iinfo(dtype)
    nodata = info.max if top else info.min
    v = integer_samples(dtype, scale, offset, nodata, seed=info.max + top)
    want, missing, saturated = twin(v, dtype, scale, offset, nodata)
    rc, got, got_missing, got_saturated = encode_host(v, dtype, scale, offset, nodata)
    assert rc == 0, _lib.load().topo_amd_last_error()
    assert got.dtype == want.dtype and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (got_missing, got_saturated) == (missing, saturated)
    assert missing == NANS.size and saturated > 0
    assert not (got[~np.isnan(v)] == nodata).any()  # no value is ever stored as the nodata code


def test_encode_host_float16_against_the_twin():
    v = half_samples(seed=16)
    want, missing, saturated = twin(v, np.float16)
    rc, got, got_missing, got_saturated = encode_host(v, np.float16)
    assert rc == 0, _lib.load().topo_amd_last_error()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), np.flatnonzero(got.view(np.uint16) != want.view(np.uint16))[:10]
    assert (got_missing, got_saturated) == (missing, saturated)
    assert missing == NANS.size and saturated >= 6  # (+-65520, +-65536, +-1e6, +-float32 max ...)
    assert (got.view(np.uint16)[np.isnan(v)] == HALF_NAN).all()


def test_encode_host_float32_is_a_copy_without_counters():
    v = np.concatenate([EDGES, NANS, np.arange(100, dtype=np.float32) / 7])
    rc, got, missing, saturated = encode_host(v, np.float32)
    assert rc == 0 and (missing, saturated) == (0, 0)
    assert np.array_equal(got.view(np.uint32), v.view(np.uint32))
    rc, _, missing, saturated = encode_host(np.zeros(0, np.float32), np.int16, 0.1, 0.0, -32768)
    assert rc == 0 and (missing, saturated) == (0, 0)  # (an empty run)


# ---- the round trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing", PACKINGS, ids=lambda p: f"{p[0]:.3g}_{p[1]:.3g}")
@pytest.mark.parametrize("dtype", INT_TYPES, ids=lambda t: np.dtype(t).name)
def test_round_trip_of_integer_planes(dtype, packing):
    scale, offset = packing
    info = np.iinfo(dtype)
    for nodata in (info.min, info.max):
        lo, hi = code_range(dtype, nodata)
        v = integer_samples(dtype, scale, offset, nodata, seed=3)
        packed = _lib.encode_host(v, tda.Packing(dtype, scale, offset, nodata))
        assert isinstance(packed, tda.PackedPlane) and isinstance(packed, tda.PackedDem)
        assert packed.values.dtype == np.dtype(dtype) and packed.missing == NANS.size
        back = packed.decode()
        assert back.dtype == np.float32
        assert np.array_equal(np.isnan(back), np.isnan(v))  # NaN exactly where the input was NaN
        with np.errstate(all="ignore"):
            q = np.rint((v.astype(np.float64) - offset) / scale)
        kept = ~np.isnan(v) & (q >= lo) & (q <= hi)
        assert packed.saturated == int((~np.isnan(v) & ~kept).sum())
        ulp = np.spacing(np.maximum(np.abs(v[kept]), np.abs(back[kept]))).astype(np.float64)
        err = np.abs(back[kept].astype(np.float64) - v[kept].astype(np.float64))
        assert (err <= abs(scale) / 2 + ulp).all(), float((err - abs(scale) / 2 - ulp).max())


def test_round_trip_of_a_float16_plane():
    v = half_samples(seed=5)
    packed = _lib.encode_host(v, tda.Packing(np.float16))
    back = packed.decode()
    assert np.array_equal(np.isnan(back), np.isnan(v))
    with np.errstate(all="ignore"):
        assert np.array_equal(back[~np.isnan(v)], packed.values.astype(np.float32)[~np.isnan(v)])
    fine = np.isfinite(v) & np.isfinite(back)
    assert packed.saturated == int((np.isfinite(v) & ~np.isfinite(back)).sum())
    err = np.abs(back[fine].astype(np.float64) - v[fine].astype(np.float64))
    assert (err <= np.maximum(np.abs(v[fine]).astype(np.float64) * 2.0 ** -11, 2.0 ** -25)).all()  # half an ulp of binary16


# ---- refusals -----------------------------------------------------------------------------------------------------------------
BAD_PLANES = [
    ("nodata inside the range", np.int16, 1.0, 0.0, -9999),
    ("nodata inside the range", np.uint16, 1.0, 0.0, 1),
    ("nodata inside the range", np.uint8, 1.0, 0.0, 254),
    ("nodata outside the type", np.uint8, 1.0, 0.0, 65535),
    ("no nodata on an integer type", np.int16, 0.1, 0.0, None),
    ("no nodata on an integer type", np.uint8, 0.5, 0.0, None),
    ("float16 with a scale", np.float16, 0.5, 0.0, None),
    ("float16 with an offset", np.float16, 1.0, 1.0, None),
    ("float16 with a nodata", np.float16, 1.0, 0.0, 0),
    ("float32 with a scale", np.float32, 0.5, 0.0, None),
    ("float32 with a nodata", np.float32, 1.0, 0.0, -9999),
    ("scale 0", np.int16, 0.0, 0.0, -32768),
    ("scale inf", np.int16, np.inf, 0.0, -32768),
    ("scale nan", np.uint16, np.nan, 0.0, 65535),
    ("offset inf", np.uint16, 1.0, -np.inf, 65535),
]


@pytest.mark.parametrize("what,dtype,scale,offset,nodata", BAD_PLANES, ids=[f"{b[0]} {np.dtype(b[1]).name}" for b in BAD_PLANES])
def test_a_bad_plane_is_refused_by_the_library_and_by_packing(what, dtype, scale, offset, nodata):
    v = np.arange(8, dtype=np.float32)
    rc, out, _, _ = encode_host(v, dtype, scale, offset, nodata)
    assert rc == -1, what  # TOPO_AMD_EINVAL
    assert _lib.load().topo_amd_last_error()
    assert (out.view(np.uint8) == 0x5A).all()  # nothing was written
    with pytest.raises(ValueError):
        tda.Packing(dtype, scale, offset, nodata)


@pytest.mark.parametrize("code", [3, 5, 7, -1])
def test_a_dtype_that_is_no_result_type_is_refused(code):
    v = np.arange(8, dtype=np.float32)
    out = np.zeros(8, dtype=np.float64)
    plane = _lib.Plane(out.ctypes.data, code, 1, 1.0, 0.0, 0.0, 0, 0)
    assert _lib.load().topo_amd_encode_host(_lib.ptr(v), v.size, C.byref(plane)) == -1
    assert not out.any()
    assert _lib.load().topo_amd_encode_host(_lib.ptr(v), v.size, None) == -1  # (no plane at all)


@pytest.mark.parametrize("dtype", [np.int32, np.float64, np.int8, np.int64, bool, ">i2", "no such type"])
def test_packing_refuses_other_dtypes(dtype):
    with pytest.raises(ValueError):
        tda.Packing(dtype, 1.0, 0.0, 0)


def test_float16_stays_refused_as_a_source_dtype():
    a = np.zeros(8, dtype=np.float16)
    raster = _lib.Raster(a.ctypes.data, _lib.F16, 0, 1.0, 0.0, 0.0)
    out = np.zeros(8, dtype=np.float32)
    assert _lib.load().topo_amd_decode_host(C.byref(raster), 8, _lib.ptr(out)) == -1


def test_pack_arguments_are_checked_before_any_library_call():
    dem = np.zeros((8, 8), dtype=np.float32)
    p = tda.Packing(np.int16, 0.1, 0.0, -32768)
    with pytest.raises(ValueError):
        topo.tpi(dem, 3, pack="int16")
    with pytest.raises(ValueError):
        topo.gradient(dem, 2.0, {"x": 30.0, "y": -30.0}, pack={"dz": p})
    with pytest.raises(ValueError):
        topo.gradient(dem, 2.0, {"x": 30.0, "y": -30.0}, pack=(p, p))
    with pytest.raises(ValueError):
        topo.tpi_std(dem, 3, pack=(p, p, p))
    assert _lib.pack_list(p, ["a", "b"]) == [p, p]
    assert _lib.pack_list({"b": p}, ["a", "b"]) == [None, p]
    assert _lib.pack_list((None, p), ["a", "b"]) == [None, p]
    assert _lib.pack_list(None, ["a"]) == [None]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------
C_TYPES = {"void*": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}


def test_the_ctypes_plane_has_the_layout_of_the_header():
    header = open(os.path.join(REPO, "include", "topo_amd.h")).read()
    body = re.search(r"typedef struct topo_amd_plane \{(.*?)\} topo_amd_plane;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(",")]
    assert fields == list(_lib.Plane._fields_)
    # natural alignment, no padding: 8 + 4 + 4 + 3 * 8 + 2 * 8
    assert C.sizeof(_lib.Plane) == 56 == sum(C.sizeof(t) for _, t in fields)
    offsets = [getattr(_lib.Plane, n).offset for n, _ in fields]
    assert offsets == [0, 8, 12, 16, 24, 32, 40, 48]
    assert int(re.search(r"#define TOPO_AMD_F16 (\d+)", header).group(1)) == _lib.F16 == 6
    for name in ("encode_host", "encode_dev", "tpi_std_packed", "tpi_std_multi_packed", "gauss_packed", "gradient_packed",
                 "sx_packed", "sx_multi_packed"):
        assert "topo_amd_" + name in _lib.SIGNATURES and hasattr(_lib.load(), "topo_amd_" + name)


def test_a_packed_plane_is_a_source():
    v = (np.arange(6 * 7, dtype=np.float32).reshape(6, 7) - 20.0) / 3.0
    v[2, 3] = np.nan
    packed = _lib.encode_host(v, tda.Packing(np.uint16, 0.05, -10.0, 65535))
    assert packed.shape == (6, 7) and packed.dtype == np.float32 and packed.missing == 1 and packed.saturated == 0
    keep, raster = _lib.source_of(packed)
    assert keep.dtype == np.uint16 and keep.ctypes.data == raster.data
    assert (raster.dtype, raster.has_nodata, raster.scale, raster.offset, raster.nodata) == (_lib.U16, 1, 0.05, -10.0, 65535.0)
    half = _lib.encode_host(v, tda.Packing(np.float16))
    keep, raster = _lib.source_of(half)  # (float16 decodes through the host cast of as_source)
    assert keep.dtype == np.float32 and raster.dtype == _lib.F32 and raster.has_nodata == 0
    assert np.array_equal(np.isnan(half.decode()), np.isnan(v))
    plain = _lib.encode_host(v, tda.Packing(np.float32))
    assert np.array_equal(plain.values.view(np.uint32), v.view(np.uint32)) and (plain.missing, plain.saturated) == (0, 0)
    assert repr(tda.Packing(np.int16, 0.1, 0.0, -32768)) == "Packing(int16, 0.1, 0.0, -32768.0)"
