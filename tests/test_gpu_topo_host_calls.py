"""``topo.*`` with ``pack=None`` goes through the ``*_packed`` entry points on float32 plane structs (tests/test_topo_host_calls.py
pins that on the CPU); here each function gives the bytes of a direct ctypes call of the ``*_raw`` symbol of the same
descriptor on the same source.  97 x 131 samples (one chunk): fractional float32 elevations, and an int16 ``PackedDem`` in
decimetres with a fill value."""
import ctypes as C

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, device as d, topo  # noqa: E402

NY, NX = 97, 131
X = 2600000.0 + 30.0 * np.arange(NX)
Y = 1200000.0 - 30.0 * np.arange(NY)
RES = orc.grid_resolution(X, Y)
AZIMUTHS = [350.0, 0.0, 45.0]


def sources():
    dem = orc.synthetic_dem(NY, NX, seed=41, integer=False)
    codes = np.rint(dem.astype(np.float64) * 10.0).astype(np.int16)
    codes[40:47, 60:90] = -32768
    codes[0, :5] = -32768
    return {"float32": dem, "int16": tda.PackedDem(codes, scale_factor=0.1, fill_value=-32768)}


SOURCES = sources()


class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class FakeDataset:
    def __init__(self, dem):
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(X, ("x",)), "y": FakeVar(Y, ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def raw(symbol, source, n_out, *args, tail=()):
    """``n_out`` float32 planes of ``symbol(raster, NY, NX, *args, planes..., *tail)``."""
    keep, raster = _lib.source_of(SOURCES[source])
    outs = [np.full((NY, NX), -12345.0, dtype=np.float32) for _ in range(n_out)]
    _lib.check(getattr(_lib.lib(), symbol)(C.byref(raster), NY, NX, *args, *[_lib.ptr(o) for o in outs], *tail), symbol)
    return outs


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_lib._i32p)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib._f64p)


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_tpi_std_and_the_pair(source):
    dem = SOURCES[source]
    for size, sigma in ((9, None), (21, 2.5)):
        t, s = raw("topo_amd_tpi_std_raw", source, 2, size, float(sigma or 0.0))
        assert same_bits(topo.tpi(dem, size, sigma), raw("topo_amd_tpi_raw", source, 1, size, float(sigma or 0.0))[0])
        assert same_bits(topo.tpi(dem, size, sigma), t)
        got = topo.std(dem, size, sigma)
        assert same_bits(got, raw("topo_amd_std_raw", source, 1, size, float(sigma or 0.0))[0].astype(np.float64)) and same_bits(got, s.astype(np.float64))
        pair = topo.tpi_std(dem, size, sigma)
        assert same_bits(pair[0], t) and same_bits(pair[1], s.astype(np.float64))
    t, s = raw("topo_amd_tpi_std_valid_raw", source, 2, 9, 3)
    assert same_bits(topo.tpi(dem, 9, skipna=True, min_count=3), t)
    assert same_bits(topo.std(dem, 9, skipna=True, min_count=3), s.astype(np.float64))
    pair = topo.tpi_std(dem, 9, skipna=True, min_count=3)
    assert same_bits(pair[0], t) and same_bits(pair[1], s.astype(np.float64))


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_tpi_std_multi(source):
    sizes, sigmas = [5, 9, 21], [0.0, 0.0, 2.5]
    keep, raster = _lib.source_of(SOURCES[source])
    want = [np.empty((NY, NX), dtype=np.float32) for _ in range(6)]
    lists = [(C.c_void_p * 3)(*[a.ctypes.data for a in want[k:k + 3]]) for k in (0, 3)]
    _lib.check(_lib.lib().topo_amd_tpi_std_multi_raw(C.byref(raster), NY, NX, 3, i32(sizes), f64(sigmas), *lists), "tpi_std_multi_raw")
    tpis, stds = topo.tpi_std_multi(SOURCES[source], sizes, [None, None, 2.5])
    for k in range(3):
        assert same_bits(tpis[k], want[k]) and same_bits(stds[k], want[3 + k].astype(np.float64)), k
    tpis, stds = topo.tpi_std_multi(SOURCES[source], sizes, [None, None, 2.5], want_std=False)
    assert stds is None and all(same_bits(t, w) for t, w in zip(tpis, want))


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_dem(source):
    dem = SOURCES[source]
    assert same_bits(topo.dem(dem, 3.25), raw("topo_amd_gauss_raw", source, 1, 3.25, 3.25)[0])
    assert same_bits(topo.dem(dem, (2.0, 0.75)), raw("topo_amd_gauss_raw", source, 1, 2.0, 0.75)[0])
    out, weight = raw("topo_amd_gauss_valid_raw", source, 2, 3.25, 3.25, 0.25, 1)
    got = topo.dem(dem, 3.25, skipna=True, min_weight=0.25, fill=True, return_weight=True)
    assert same_bits(got[0], out) and same_bits(got[1], weight)
    assert same_bits(topo.dem(dem, 3.25, skipna=True), raw("topo_amd_gauss_valid_raw", source, 1, 3.25, 3.25, 0.0, 0, tail=(None,))[0])


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_gradient(source):
    mode, rx, ry = topo._resolution_args(RES, (NY, NX))
    for sigma in (0.75, 3.25):
        want = raw("topo_amd_gradient_raw", source, 4, sigma, 1.0, mode, _lib.ptr(rx), _lib.ptr(ry))
        got = topo.gradient(SOURCES[source], sigma, RES)
        assert len(got) == 4 and all(same_bits(g, w) for g, w in zip(got, want)), sigma


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_sx_and_sx_multi(source):
    dem = SOURCES[source]
    sectors = [d.sx_offsets(a, 500.0, 30.0, -30.0) for a in AZIMUTHS]
    ds = FakeDataset(dem)
    for azimuth, (reach, dj, di, dist) in zip(AZIMUTHS, sectors):
        want, = raw("topo_amd_sx_raw", source, 1, i32(dj), i32(di), f64(dist), int(np.size(dist)), int(reach), 10.0)
        assert same_bits(topo._sx_scan(dem, reach, dj, di, dist, 10.0), want)
        assert same_bits(topo.sx(ds, azimuth, 500.0), want)
    first, dj, di, dist, window = d.pack_sectors(sectors)
    keep, raster = _lib.source_of(dem)
    want = [np.full((NY, NX), -12345.0, dtype=np.float32) for _ in sectors]
    planes = (C.c_void_p * 3)(*[a.ctypes.data for a in want])
    _lib.check(_lib.lib().topo_amd_sx_multi_raw(C.byref(raster), NY, NX, 3, i32(first), i32(dj), i32(di), f64(dist), i32(window), 10.0, planes),
               "sx_multi_raw")
    got = topo.sx_multi(ds, AZIMUTHS, 500.0)
    assert len(got) == 3 and all(g.dtype == np.float32 and same_bits(g, w) for g, w in zip(got, want))
