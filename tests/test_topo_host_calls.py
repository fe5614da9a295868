"""``topo.*`` on a host array makes ONE library call per function - the ``*_packed`` entry point, whatever ``pack`` is (a
float32 plane struct is what the ``*_raw`` entry points build themselves) - checked without a GPU: a recording stand-in
takes the place of ``_lib.lib()``, notes the symbol and its arguments, writes ``k + 1`` into every sample of the k-th result
plane through the struct's pointer and returns 0.  So the result must hold those values, in the type and dtype the function
promises: float32 TPI, float64 STD unless packed, Sx in the DEM's dtype, ``PackedPlane`` for a ``Packing``."""
import ctypes as C

import numpy as np
import pytest

import topo_descriptors_amd as tda
from topo_descriptors_amd import _lib, topo

NY, NX = 8, 9
ITEMSIZE = {code: dtype.itemsize for dtype, code in _lib.PLANE_DTYPES.items()}
NUMPY = {code: dtype for dtype, code in _lib.PLANE_DTYPES.items()}
P16 = tda.Packing(np.int16, 0.1, 0.0, -32768)
SOURCES = {
    "float32": np.arange(NY * NX, dtype=np.float32).reshape(NY, NX),
    "int16": tda.PackedDem(np.arange(NY * NX, dtype=np.int16).reshape(NY, NX), fill_value=-32768),
}
RES = {"x": 30.0, "y": -30.0}


class Recorder:
    """Stands in for the loaded library: every symbol is a function that records its call and fills the planes it is given."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            planes = []
            for a in args:
                obj = getattr(a, "_obj", a)  # (byref(x) keeps x in _obj)
                if isinstance(obj, _lib.Plane):
                    planes.append(obj)
                elif isinstance(obj, C.Array) and obj._type_ is _lib.Plane:
                    planes.extend(obj)
            for k, p in enumerate(planes):
                assert p.data, (name, k)
                np.frombuffer((C.c_char * (NY * NX * ITEMSIZE[p.dtype])).from_address(p.data), dtype=NUMPY[p.dtype])[:] = k + 1
            self.calls.append((name, args, planes))
            return 0
        return call


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class FakeDataset:
    def __init__(self, dem):
        x, y = 2600000.0 + 30.0 * np.arange(NX), 1200000.0 - 30.0 * np.arange(NY)
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(x, ("x",)), "y": FakeVar(y, ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def one_call(rec, symbol, packs):
    """The single call ``rec`` saw: ``symbol``, with one plane struct per entry of ``packs`` in the dtype of that packing."""
    assert [c[0] for c in rec.calls] == [symbol]
    planes = rec.calls[0][2]
    assert [p.dtype for p in planes] == [_lib.PLANE_DTYPES[np.dtype(np.float32) if q is None else q.dtype] for q in packs]
    return planes


def holds(result, k, packing, dtype):
    """``result`` is plane ``k`` of the call: ``k + 1`` everywhere, an ndarray of ``dtype`` or a ``PackedPlane`` of the packing."""
    if packing is None:
        assert isinstance(result, np.ndarray) and result.dtype == dtype and result.shape == (NY, NX)
        assert (result == k + 1).all()
    else:
        assert isinstance(result, _lib.PackedPlane) and result.packing is packing
        assert result.values.dtype == packing.dtype and result.values.shape == (NY, NX) and (result.values == k + 1).all()


SKIPNA = [False, True]
PACKS = [None, P16]


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("skipna", SKIPNA)
@pytest.mark.parametrize("pack", PACKS, ids=["float32", "packed"])
def test_tpi_std_and_the_pair(rec, pack, skipna, source):
    symbol = "topo_amd_tpi_std_valid_packed" if skipna else "topo_amd_tpi_std_packed"
    dem = SOURCES[source]
    holds(topo.tpi(dem, 5, pack=pack, skipna=skipna), 0, pack, np.float32)
    one_call(rec, symbol, [pack])
    rec.calls.clear()
    holds(topo.std(dem, 5, pack=pack, skipna=skipna), 0, pack, np.float64)
    one_call(rec, symbol, [pack])
    rec.calls.clear()
    pair = topo.tpi_std(dem, 5, pack=None if pack is None else (pack, None), skipna=skipna)
    assert isinstance(pair, tuple) and len(pair) == 2
    holds(pair[0], 0, pack, np.float32)
    holds(pair[1], 1, None, np.float64)
    one_call(rec, symbol, [pack, None])


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("pack", PACKS, ids=["float32", "packed"])
def test_tpi_std_multi(rec, pack, source):
    tpis, stds = topo.tpi_std_multi(SOURCES[source], [3, 5], pack=pack)
    one_call(rec, "topo_amd_tpi_std_multi_packed", [pack] * 4)
    assert isinstance(tpis, list) and isinstance(stds, list)
    for k in range(2):
        holds(tpis[k], k, pack, np.float32)
        holds(stds[k], 2 + k, pack, np.float64)
    rec.calls.clear()
    tpis, stds = topo.tpi_std_multi(SOURCES[source], [3, 5], want_std=False, pack=pack)
    one_call(rec, "topo_amd_tpi_std_multi_packed", [pack] * 2)
    assert stds is None and len(tpis) == 2


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("skipna", SKIPNA)
@pytest.mark.parametrize("pack", PACKS, ids=["float32", "packed"])
def test_dem(rec, pack, skipna, source):
    holds(topo.dem(SOURCES[source], 2.0, pack=pack, skipna=skipna), 0, pack, np.float32)
    one_call(rec, "topo_amd_gauss_valid_packed" if skipna else "topo_amd_gauss_packed", [pack])
    if skipna:
        rec.calls.clear()
        out, weight = topo.dem(SOURCES[source], 2.0, pack=pack, skipna=True, return_weight=True)
        one_call(rec, "topo_amd_gauss_valid_packed", [pack])
        holds(out, 0, pack, np.float32)
        assert weight.dtype == np.float32 and weight.shape == (NY, NX)
        assert rec.calls[0][1][-1].value == weight.ctypes.data  # (the weight plane: a float32 pointer, whatever the packing)


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("pack", PACKS, ids=["float32", "packed"])
def test_gradient(rec, pack, source):
    packs = [None] * 4 if pack is None else [pack, None, pack, None]
    out = topo.gradient(SOURCES[source], 3.25, RES, pack=None if pack is None else packs)
    one_call(rec, "topo_amd_gradient_packed", packs)
    assert isinstance(out, list) and len(out) == 4
    for k, q in enumerate(packs):
        holds(out[k], k, q, np.float32)


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("pack", PACKS, ids=["float32", "packed"])
def test_sx_scan_and_sx_multi(rec, pack, source):
    dem = SOURCES[source]
    out = topo._sx_scan(dem, 1, np.array([-1]), np.array([0]), np.array([30.0]), 10.0, pack=pack)
    one_call(rec, "topo_amd_sx_packed", [pack])
    holds(out, 0, pack, np.float32)  # (the DEM's dtype: a PackedDem decodes to float32)
    rec.calls.clear()
    outs = topo.sx_multi(FakeDataset(dem), [0.0, 90.0, 180.0], 60.0, pack=pack)
    one_call(rec, "topo_amd_sx_multi_packed", [pack] * 3)
    assert isinstance(outs, list) and len(outs) == 3
    for k, o in enumerate(outs):
        holds(o, k, pack, np.float32)


def test_sx_in_the_dtype_of_the_dem_and_planes_made_on_the_host(rec):
    dem = SOURCES["float32"].astype(np.float64)
    assert topo._sx_scan(dem, 1, np.array([-1]), np.array([0]), np.array([30.0]), 10.0).dtype == np.float64
    rec.calls.clear()
    # nothing but frame, and no usable ray pixel: no library call, zeros / NaN inside the frame, packed on the host
    frame = topo._sx_scan(dem, 4, np.array([-1]), np.array([0]), np.array([30.0]), 10.0)
    assert frame.dtype == np.float64 and not frame.any()
    empty = topo._sx_scan(dem, 1, np.array([-1]), np.array([0]), np.array([np.nan]), 10.0)
    assert np.isnan(empty[1:-1, 1:-1]).all() and not empty[0].any() and not empty[:, -1].any()
    packed = topo._sx_scan(dem, 1, np.array([-1]), np.array([0]), np.array([np.nan]), 10.0, pack=P16)
    assert isinstance(packed, _lib.PackedPlane) and packed.missing == (NY - 2) * (NX - 2)
    assert rec.calls == []
