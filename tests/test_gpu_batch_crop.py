"""``crop=`` and ``ind_nans=`` of the batch wrappers on the GPU, without xarray: every wrapper called with a crop must give the
result of the same call without it, cut on the host by ``helpers.crop_window`` - float planes bit for bit, packed planes code
for code, with the counters ``topo_amd_encode_host`` recounts on the float window.

A 96 x 131 DEM, x increasing, y decreasing (north to south); the domain is off every border, rows 9 ... 80 and columns
13 ... 115: col0 = 13 and cols = 103 are no multiples of 4.  ``ind_nans`` is given as the boolean mask of ``fill_na_gpu`` and as
the index tuple of ``np.where``, with samples inside the domain, on its edges and outside it."""
import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, batch, device as d, helpers as hlp  # noqa: E402

NY, NX = 96, 131
ROW0, ROWS, COL0, COLS = 9, 72, 13, 103


class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class FakeDataset:
    def __init__(self, dem, x, y, crs="epsg:2056"):
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(x, ("x",)), "y": FakeVar(y, ("y",))}
        self.attrs = {"crs": crs}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


X = 2600000.0 + 30.0 * np.arange(NX)
Y = 1200000.0 - 30.0 * np.arange(NY)
DEM = orc.synthetic_dem(NY, NX, seed=23, integer=False)
DS = FakeDataset(DEM, X, Y)
CROP = {"x": slice(X[COL0] - 5.0, X[COL0 + COLS - 1] + 5.0), "y": slice(Y[ROW0] + 1.0, Y[ROW0 + ROWS - 1] - 1.0)}


def _mask():
    rng = np.random.default_rng(5)
    m = rng.random((NY, NX)) < 0.03
    m[ROW0, COL0] = m[ROW0 + ROWS - 1, COL0 + COLS - 1] = True  # the domain's corners,
    m[ROW0 - 1, COL0 + 4] = m[ROW0 + 5, COL0 - 1] = True         # just outside it,
    m[0, 0] = m[NY - 1, NX - 1] = True                           # and the raster's corners
    m[40, 20:60] = True                                          # a run along a row
    return m


MASK = _mask()
INDEX = np.where(MASK)
TPI_DM = tda.Packing(np.int16, 0.1, 0.0, -32768)
STD_5CM = tda.Packing(np.uint16, 0.05, 0.0, 65535)
HALF = tda.Packing(np.float16)
SLOPE = tda.Packing(np.uint8, 0.5, 0.0, 255)
ASPECT = tda.Packing(np.uint16, 0.01, 0.0, 65535)
SX_CDEG = tda.Packing(np.int16, 0.01, 0.0, -32768)
NORM = tda.Packing(np.int16, 0.001, 0.0, 32767)
DIRECTION = tda.Packing(np.uint8, 1.0, 0.0, 255)


def test_the_window_of_the_crop():
    assert hlp.crop_window(DS, CROP) == (ROW0, ROWS, COL0, COLS)
    assert COL0 % 4 and COLS % 4 and ROW0 > 0 and ROW0 + ROWS < NY and COL0 + COLS < NX


def cut(a):
    return np.ascontiguousarray(a[ROW0:ROW0 + ROWS, COL0:COL0 + COLS])


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def compare(call, pack, masked=True):
    """``call(ind_nans, crop, pack, outdir=None)`` -> the wrapper's dict.  Float and packed, with and without the crop, the mask
    given both ways."""
    full = call(MASK, None, None)
    assert len(full) >= 1
    for ind_nans in (MASK, INDEX):
        cropped = call(ind_nans, CROP, None)
        assert list(cropped) == list(full)
        for name, want in full.items():
            assert isinstance(cropped[name], np.ndarray) and cropped[name].shape == (ROWS, COLS), name
            assert same_bits(cropped[name], cut(want)), name
            if masked:
                assert np.isnan(cropped[name][cut(MASK)]).all(), name
    packed_full = call(INDEX, None, pack)
    packed_cropped = call(MASK, CROP, pack)
    assert list(packed_cropped) == list(full)
    n_packed = 0
    for name, want in full.items():
        got, whole = packed_cropped[name], packed_full[name]
        if not isinstance(whole, _lib.PackedPlane):  # a plane of the call that stays float32
            assert same_bits(got, cut(want)), name
            continue
        n_packed += 1
        assert isinstance(got, _lib.PackedPlane) and got.values.shape == (ROWS, COLS), name
        assert same_bits(got.values, cut(whole.values)), name
        recount = _lib.encode_host(cut(want).astype(np.float32), got.packing)
        assert same_bits(got.values, recount.values), name
        assert (got.missing, got.saturated) == (recount.missing, recount.saturated), name
        if masked:
            assert got.missing >= int(cut(MASK).sum())
    assert n_packed >= 1
    return full


def test_compute_dem():
    compare(lambda i, c, p: batch.compute_dem(DS, [200, 500], ind_nans=i, crop=c, outdir=None, pack=p), STD_5CM)


def test_compute_tpi_paired_smoothed_and_67_px():
    # 5 and 7 px share a pass (Block.tpi_multi), 17 px is smoothed first, 67 px takes the wide kernels
    full = compare(lambda i, c, p: batch.compute_tpi(DS, [150, 200, 500, 2010], smth_factors=[None, None, 0.5, None], ind_nans=i,
                                                     crop=c, outdir=None, pack=p), TPI_DM)
    assert list(full) == ["TPI_150M", "TPI_200M", "TPI_500M_SMTHFACT0.5", "TPI_2010M"]
    assert int(hlp.scale_to_pixel([2010], DS)[0][0]) == 67


def test_compute_std():
    full = compare(lambda i, c, p: batch.compute_std(DS, [200, 500], smth_factors=[None, 0.5], ind_nans=i, crop=c, outdir=None,
                                                     pack=p), HALF)
    assert all(a.dtype == np.float64 for a in full.values())  # (widened after the finish)


def test_compute_gradient_1d_resolutions():
    full = compare(lambda i, c, p: batch.compute_gradient(DS, [100, 400], sig_ratios=[1, 2], ind_nans=i, crop=c, outdir=None,
                                                          pack=p), {"slope": SLOPE, "aspect": ASPECT})
    assert len(full) == 8


def test_gradient_scalar_resolutions_on_the_row_range():
    """``Block.gradient`` with scalar resolutions (the wrappers always pass one resolution per node) over the window's rows,
    then ``finish``: the whole-plane call, cut."""
    dem = d.DeviceArray.from_host(DEM)
    whole = [d.DeviceArray(NY, NX) for _ in range(4)]
    part = [d.DeviceArray(ROWS, NX) for _ in range(4)]
    mask = d.DeviceArray(ROWS, NX, dtype=np.uint8)
    try:
        mask.upload_rows(MASK[ROW0:ROW0 + ROWS].view(np.uint8))
        block = d.Block(dem)
        for sigma in (0.8, 3.25):
            block.gradient(sigma, 30.0, -30.0, dx=whole[0], dy=whole[1], slope=whole[2], aspect=whole[3])
            block.gradient(sigma, 30.0, -30.0, dx=part[0], dy=part[1], slope=part[2], aspect=part[3], out_row0=ROW0, out_rows=ROWS)
            for w, p in zip(whole, part):
                want = w.to_host()
                want[MASK] = np.nan
                assert same_bits(p.finish(None, mask, (0, ROWS, COL0, COLS)), cut(want)), sigma
    finally:
        for a in [dem, mask, *whole, *part]:
            a.free()


def test_compute_gradient_2d_resolutions():
    lon = 7.0 + 0.0004 * np.arange(NX)
    lat = 47.0 - 0.0003 * np.arange(NY)
    ds = FakeDataset(DEM, lon, lat, crs="EPSG:4326")
    crop = {"x": slice(lon[COL0] - 1e-5, lon[COL0 + COLS - 1] + 1e-5), "y": slice(lat[ROW0] + 1e-5, lat[ROW0 + ROWS - 1] - 1e-5)}
    assert hlp.crop_window(ds, crop) == (ROW0, ROWS, COL0, COLS)
    assert np.ndim(hlp.scale_to_pixel([300], ds)[1]["x"]) == 2
    full = batch.compute_gradient(ds, [300], ind_nans=MASK, outdir=None)
    cropped = batch.compute_gradient(ds, [300], ind_nans=INDEX, crop=crop, outdir=None)
    packed = batch.compute_gradient(ds, [300], ind_nans=MASK, crop=crop, outdir=None, pack={"slope": SLOPE})
    assert list(cropped) == list(full) == list(packed) and len(full) == 4
    for name, want in full.items():
        assert same_bits(cropped[name], cut(want)), name
        assert np.isnan(cropped[name][cut(MASK)]).all()
        if name.startswith("SLOPE"):
            recount = _lib.encode_host(cut(want), SLOPE)
            assert same_bits(packed[name].values, recount.values)
            assert (packed[name].missing, packed[name].saturated) == (recount.missing, recount.saturated)
        else:
            assert same_bits(packed[name], cut(want)), name


def test_compute_valley_ridge_with_and_without_smoothing():
    full = compare(lambda i, c, p: batch.compute_valley_ridge(DS, [200, 200], "valley", smth_factors=[None, 0.5], ind_nans=i, crop=c,
                                                              outdir=None, pack=p), {"norm": NORM, "direction": DIRECTION})
    assert len(full) == 4


def test_compute_sx_one_azimuth_and_a_sequence():
    compare(lambda i, c, p: batch.compute_sx(DS, 270.0, 300.0, crop=c, outdir=None, pack=p), SX_CDEG, masked=False)
    full = compare(lambda i, c, p: batch.compute_sx(DS, [0.0, 90.0, 225.0], 300.0, crop=c, outdir=None, pack=p), SX_CDEG, masked=False)
    assert len(full) == 3


def test_files_of_the_window_are_written_without_xarray(tmp_path):
    assert hlp._xr is None or not isinstance(DS, hlp._xr.Dataset)
    out = batch.compute_tpi(DS, [500], ind_nans=MASK, crop=CROP, outdir=str(tmp_path / "f32"))
    saved = np.load(tmp_path / "f32" / "topo_TPI_500M.npy")
    assert saved.shape == (ROWS, COLS) and same_bits(saved, out["TPI_500M"])
    out = batch.compute_tpi(DS, [500], ind_nans=MASK, crop=CROP, outdir=str(tmp_path / "i16"), pack=TPI_DM)
    with np.load(tmp_path / "i16" / "topo_TPI_500M.npz") as z:
        assert z["values"].shape == (ROWS, COLS) and z["values"].dtype == np.int16
        assert same_bits(z["values"], out["TPI_500M"].values)
        assert (float(z["scale_factor"]), float(z["add_offset"]), float(z["fill_value"])) == (0.1, 0.0, -32768.0)


def test_a_crop_in_the_wrong_direction_selects_nothing(tmp_path):
    crop = {"x": CROP["x"], "y": slice(Y[ROW0 + ROWS - 1], Y[ROW0])}  # south to north on a north-to-south y
    assert hlp.crop_window(DS, crop)[1] == 0
    calls = {
        "dem": lambda p: batch.compute_dem(DS, [200], ind_nans=MASK, crop=crop, outdir=None, pack=p),
        "tpi": lambda p: batch.compute_tpi(DS, [150, 200, 500], ind_nans=INDEX, crop=crop, outdir=str(tmp_path), pack=p),
        "std": lambda p: batch.compute_std(DS, [200], ind_nans=MASK, crop=crop, outdir=None, pack=p),
        "grad": lambda p: batch.compute_gradient(DS, [100], ind_nans=MASK, crop=crop, outdir=None, pack=p),
        "vr": lambda p: batch.compute_valley_ridge(DS, [200], "ridge", ind_nans=MASK, crop=crop, outdir=None, pack=p),
        "sx": lambda p: batch.compute_sx(DS, [0.0, 90.0], 300.0, crop=crop, outdir=None, pack=p),
    }
    counts = {"dem": 1, "tpi": 3, "std": 1, "grad": 4, "vr": 2, "sx": 2}
    for tag, call in calls.items():
        out = call(None)
        assert len(out) == counts[tag], tag
        for name, a in out.items():
            assert isinstance(a, np.ndarray) and a.shape == (0, COLS), (tag, name)
            assert a.dtype == (np.float64 if tag == "std" else np.float32), (tag, name)
        out = call(HALF)
        for name, a in out.items():
            assert isinstance(a, _lib.PackedPlane) and a.values.shape == (0, COLS) and a.values.dtype == np.float16, (tag, name)
            assert (a.missing, a.saturated) == (0, 0)
    assert np.load(tmp_path / "topo_TPI_500M.npy").shape == (0, COLS)


def test_an_index_outside_the_dem_is_numpys_index_error():
    with pytest.raises(IndexError):
        batch.compute_dem(DS, [200], ind_nans=(np.array([3, NY]), np.array([4, 5])), crop=CROP, outdir=None)
    with pytest.raises(IndexError):
        batch.compute_dem(DS, [200], ind_nans=(np.array([3, 4]), np.array([4, NX])), outdir=None)
