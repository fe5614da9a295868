"""The valley / ridge index with its moments, smoothing and packing on the GPU (include/topo_amd.h, topo_amd_mean_std_f32_dev and
topo_amd_valley_ridge_packed): the two moments must be numpy's own float32 ``mean()`` / ``std()`` bit for bit, so every plane of
the single call and of ``compute_valley_ridge`` keeps the bits of the path that took them on the host
(``TOPO_AMD_VALLEY_HOST_MOMENTS=1``); packed planes are ``topo_amd_encode_host`` of the float32 ones.  Equalities throughout."""
import ctypes as C

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, batch, device as d, helpers as hlp, topo  # noqa: E402

HOST = "TOPO_AMD_VALLEY_HOST_MOMENTS"
# 1, 5, 8, 127, 128, 129, 8191, 8192, 8193, 16383, 16385, 3 * 8192 + 77 samples, and planes of several chunks with a tail
SHAPES = [(1, 1), (1, 5), (2, 4), (1, 127), (2, 64), (3, 43), (1, 8191), (64, 128), (1, 8193), (129, 127), (5, 3277),
          (1, 3 * 8192 + 77), (300, 1003), (2049, 2051)]


def plane(shape, kind, seed=0):
    z = np.random.default_rng(seed).normal(1800.0, 600.0, size=shape)
    return {"metres": np.rint(z), "fractional": z, "millimetres": np.rint(z * 1000.0)}[kind].astype(np.float32)


def device_moments(a, **kw):
    dev = d.DeviceArray.from_host(a)
    try:
        return d.mean_std_numpy(dev, **kw)
    finally:
        dev.free()


def assert_numpy_moments(a, got):
    with np.errstate(all="ignore"):
        want = (a.mean(), a.std())
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    np.testing.assert_array_equal(np.array(got), np.array(want))  # (NaN equals NaN)


@pytest.mark.parametrize("kind", ["metres", "fractional"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mean_std_numpy_is_numpy(shape, kind):
    a = plane(shape, kind, seed=shape[1])
    assert_numpy_moments(a, device_moments(a))


def test_mean_std_numpy_special_planes():
    shape = (300, 1003)  # 36 chunks of 8192 and a tail of 5988
    flat = np.full(shape, 1024.0, np.float32)  # every partial sum is exact: the mean is the constant, std exactly 0
    assert_numpy_moments(flat, device_moments(flat))
    assert device_moments(flat) == (1024.0, 0.0)
    flat = np.full(shape, 1234.5678, np.float32)  # the mean is rounded: numpy's std is 2.4e-4, and so is this one
    assert_numpy_moments(flat, device_moments(flat))
    assert_numpy_moments(plane(shape, "millimetres"), device_moments(plane(shape, "millimetres")))
    for index, value in ((100, np.nan), (300000, np.nan), (100, np.inf), (300000, np.inf)):
        a = plane(shape, "fractional", seed=index)
        a.reshape(-1)[index] = value
        got = device_moments(a)
        assert_numpy_moments(a, got)
        assert np.isnan(got[1]) and (np.isnan(got[0]) if np.isnan(value) else got[0] == np.inf)
    # rows of a plane: a start that is not 16-byte aligned
    a = plane(shape, "fractional", seed=5)
    assert_numpy_moments(a[1:], device_moments(a, row0=1))
    assert_numpy_moments(a[3:40], device_moments(a, row0=3, rows=37))


@pytest.mark.parametrize("chunk", [128, 1024, 16384, 65536])
def test_mean_std_numpy_other_buffer_sizes(chunk):
    """``chunk`` is numpy's buffer size; the model (``helpers.numpy_order_moments``, equal to numpy under ``np.setbufsize`` in
    tests/test_numpy_order_moments.py) is the reference for sizes this process's numpy is not set to."""
    for shape in ((300, 1003), (3, 43), (129, 127)):
        a = plane(shape, "fractional", seed=chunk)
        np.testing.assert_array_equal(np.array(device_moments(a, chunk=chunk)), np.array(hlp.numpy_order_moments(a, chunk)))


@pytest.mark.parametrize("chunk", [100, 64, 0, 8192 + 128])
def test_mean_std_numpy_refuses_other_chunks(chunk):
    with pytest.raises(_lib.TopoAmdError, match="status -1"):
        device_moments(plane((3, 43), "metres"), chunk=chunk)
    with pytest.raises(ValueError):
        d.mean_std_numpy(d.DeviceArray(2, 2, dtype=np.uint8))


# ---- the single call against the path that takes the moments on the host ---------------------------------------------------
def both_paths(monkeypatch, call):
    """``call()`` on the new path and on the forced old one: (planes, moments route, valley route) of each."""
    out = []
    for forced in (False, True):
        if forced:
            monkeypatch.setenv(HOST, "1")
        else:
            monkeypatch.delenv(HOST, raising=False)
        planes = call()
        out.append((planes, d.valley_moments_route(), d.valley_route()))
    monkeypatch.delenv(HOST, raising=False)
    return out


def same_planes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("sigma", [None, 1.5])
@pytest.mark.parametrize("integer", [True, False], ids=["metres", "fractional"])
@pytest.mark.parametrize("shape,mode", [((150, 200), "valley"), ((97, 131), "ridge")], ids=["150x200", "97x131"])
def test_single_call_keeps_the_bits_of_the_host_moments(shape, mode, integer, sigma, monkeypatch):
    dem = orc.synthetic_dem(*shape, seed=17, integer=integer)
    (new, new_moments, new_route), (old, old_moments, old_route) = both_paths(monkeypatch, lambda: topo.valley_ridge(dem, 7, mode, sigma=sigma))
    assert same_planes(new, old)
    assert (new_moments, old_moments) == (1, 0) and new_route == old_route


def test_sources_whose_moments_numpy_takes_in_float64_stay_on_the_host(monkeypatch):
    monkeypatch.delenv(HOST, raising=False)
    dem = orc.synthetic_dem(97, 131, seed=2)
    as_int = dem.astype(np.int16)
    got = topo.valley_ridge(as_int, 7, "valley")
    assert d.valley_moments_route() == 0
    # ... and with sigma the field is the smoothed float32 array: the device
    smoothed = topo.valley_ridge(as_int, 7, "valley", sigma=1.5)
    assert d.valley_moments_route() == 1
    assert same_planes(smoothed, topo.valley_ridge(topo.dem(as_int, 1.5), 7, "valley"))
    # a packed int16 source decodes to float32: the device, with the bits of the decoded array
    packed = tda.PackedDem(as_int, 1.0, 0.0, None)
    assert same_planes(topo.valley_ridge(packed, 7, "valley"), topo.valley_ridge(dem, 7, "valley"))
    assert d.valley_moments_route() == 1
    assert got[0].shape == dem.shape
    # a float32 view that is not C-contiguous: numpy sums it in another order
    topo.valley_ridge(np.asfortranarray(dem), 7, "valley")
    assert d.valley_moments_route() == 0


@pytest.mark.parametrize("sigma", [0.0, 1.5])
def test_moments_out_are_numpys(sigma):
    dem = orc.synthetic_dem(150, 200, seed=23, integer=False)
    field = topo.dem(dem, sigma) if sigma else dem
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(7, [0, 0.15, 0.3]), np.arange(0, 180, 15, dtype=np.float32))
    keep, raster = _lib.source_of(dem)
    norm, direction = np.empty_like(dem), np.empty_like(dem)
    moments = (C.c_float * 2)()
    _lib.check(_lib.lib().topo_amd_valley_ridge_std_raw(
        C.byref(raster), 150, 200, taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(_lib._i32p), angles.ctypes.data_as(_lib._vp),
        ksize.size, 3, sigma, np.getbufsize(), _lib.ptr(norm), _lib.ptr(direction), moments), "valley_ridge_std_raw")
    assert d.valley_moments_route() == 1
    np.testing.assert_array_equal(np.array(moments[:], np.float32), np.array([field.mean(), field.std()]))
    want_n, want_d = np.empty_like(dem), np.empty_like(dem)
    keep2, raster2 = _lib.source_of(field)
    _lib.check(_lib.lib().topo_amd_valley_ridge_raw(
        C.byref(raster2), 150, 200, taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(_lib._i32p), angles.ctypes.data_as(_lib._vp),
        ksize.size, 3, float(field.mean()), float(field.std()), _lib.ptr(want_n), _lib.ptr(want_d)), "valley_ridge_raw")
    assert d.valley_moments_route() == 0
    assert same_planes([norm, direction], [want_n, want_d])


# ---- packed planes -----------------------------------------------------------------------------------------------------------
NORM_MILLI = tda.Packing(np.int16, 0.001, 0.0, -32768)  # the norm in thousandths: saturates beyond 32.767
DEGREES = tda.Packing(np.uint8, 1.0, 0.0, 255)          # whole degrees 0 ... 179: exact
HALF = tda.Packing(np.float16)


def assert_encoded(got, plane32, packing):
    want = _lib.encode_host(plane32, packing)
    assert isinstance(got, tda.PackedPlane) and got.packing is packing
    assert got.values.dtype == want.values.dtype and got.values.tobytes() == want.values.tobytes()
    assert (got.missing, got.saturated) == (want.missing, want.saturated)


@pytest.mark.parametrize("sigma", [None, 1.5])
def test_packed_planes_are_the_encoded_float32_planes(sigma, monkeypatch):
    monkeypatch.delenv(HOST, raising=False)
    dem = orc.synthetic_dem(97, 131, seed=31, integer=False)
    norm, direction = topo.valley_ridge(dem, 7, "valley", sigma=sigma)
    for pack in ({"norm": NORM_MILLI, "direction": DEGREES}, HALF, {"direction": DEGREES}):
        got = topo.valley_ridge(dem, 7, "valley", sigma=sigma, pack=pack)
        assert d.valley_moments_route() == 1
        for g, p32, q in zip(got, (norm, direction), _lib.pack_list(pack, ["norm", "direction"])):
            if q is None:
                assert isinstance(g, np.ndarray) and g.tobytes() == p32.tobytes()
            else:
                assert_encoded(g, p32, q)
        if isinstance(pack, dict):  # whole degrees in uint8: nothing lost
            assert got[1].decode().tobytes() == direction.tobytes() and (got[1].missing, got[1].saturated) == (0, 0)
    assert norm.max() > 0.0 and len(np.unique(direction)) > 20


def test_pack_on_the_host_moments_path_is_the_same_plane(monkeypatch):
    dem = orc.synthetic_dem(97, 131, seed=33)
    pack = {"norm": NORM_MILLI, "direction": DEGREES}
    (new, *_), (old, old_moments, _) = both_paths(monkeypatch, lambda: topo.valley_ridge(dem, 7, "ridge", pack=pack))
    assert old_moments == 0
    for a, b in zip(new, old):
        assert a.values.tobytes() == b.values.tobytes() and (a.missing, a.saturated) == (b.missing, b.saturated)


# ---- compute_valley_ridge ----------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def dataset():
    ny, nx = 120, 160
    dem = orc.synthetic_dem(ny, nx, seed=41, integer=False)
    ds = FakeDataset(dem, 2600000.0 + 30.0 * np.arange(nx), 1200000.0 - 30.0 * np.arange(ny))
    assert list(hlp.scale_to_pixel([200, 260], ds)[0]) == [7, 9]
    return ds


@pytest.fixture(scope="module")
def host_moment_planes(dataset):
    """The wrapper's float32 planes with the moments taken on the host, as before: computed once, never changed."""
    mp = pytest.MonkeyPatch()
    mp.setenv(HOST, "1")
    try:
        out = batch.compute_valley_ridge(dataset, [200, 260], "valley", smth_factors=[None, 1], outdir=None)
        assert d.valley_moments_route() == 0
    finally:
        mp.undo()
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["float32", "packed"])
def test_compute_valley_ridge_downloads_only_its_results(dataset, host_moment_planes, packed, monkeypatch):
    monkeypatch.delenv(HOST, raising=False)
    pack = {"norm": NORM_MILLI, "direction": DEGREES} if packed else None
    downloads = []
    real = d.DeviceArray.to_host

    def counting(self, row0=0, rows=None):
        downloads.append(self.dtype)
        return real(self, row0, rows)

    monkeypatch.setattr(d.DeviceArray, "to_host", counting)
    out = batch.compute_valley_ridge(dataset, [200, 260], "valley", smth_factors=[None, 1], outdir=None, pack=pack)
    assert d.valley_moments_route() == 1
    # two scales x (norm, direction), each leaving once in the type it is stored in: no plane left for the moments
    assert sorted(map(str, downloads)) == sorted(["int16", "uint8"] * 2 if packed else ["float32"] * 4)
    assert list(out) == list(host_moment_planes)
    for name, want in host_moment_planes.items():
        if packed:
            assert_encoded(out[name], want, NORM_MILLI if "NORM" in name else DEGREES)
        else:
            assert out[name].dtype == np.float32 and out[name].tobytes() == want.tobytes(), name
    # the wrapper and the single call agree, smoothed scale included
    if not packed:
        dem = dataset["dem"].values
        assert same_planes([out[n] for n in list(out)[2:]], topo.valley_ridge(dem, 9, "valley", sigma=9 / 4))


def test_a_partial_block_cannot_form_the_moments():
    dem = orc.synthetic_dem(60, 80, seed=3)
    dev = d.DeviceArray.from_host(dem)
    norm, direction = d.DeviceArray(60, 80), d.DeviceArray(60, 80)
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(5, [0]), np.arange(0, 180, 45, dtype=np.float32))
    try:
        for blk in (d.Block(dev, row0=0, gny=100), d.Block(dev, row0=40, gny=100), d.Block(dev, rows=30, gny=60)):
            with pytest.raises(ValueError, match="whole raster"):
                blk.valley_ridge(taps, ksize, angles, 1, norm=norm, direction=direction)
        with pytest.raises(ValueError):
            d.Block(dev).valley_ridge(taps, ksize, angles, 1, mean=1900.0, norm=norm, direction=direction)
        # the whole raster forms them itself, and the result is the call with numpy's moments
        d.Block(dev).valley_ridge(taps, ksize, angles, 1, norm=norm, direction=direction)
        assert d.valley_moments_route() == 1
        got = [norm.to_host(), direction.to_host()]
        d.Block(dev).valley_ridge(taps, ksize, angles, 1, float(dem.mean()), float(dem.std()), norm, direction)
        assert d.valley_moments_route() == 0
        assert same_planes(got, [norm.to_host(), direction.to_host()])
    finally:
        for a in (dev, norm, direction):
            a.free()
