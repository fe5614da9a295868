"""Valid-sample Gaussian (``topo.dem(skipna=True)``; csrc/gauss_valid.hip) on the GPU, every pixel against the float64
reference of tests/gauss_valid_ref.py (tests/test_gauss_valid_design.py shows what its comparison notices).

Rasters: those of tests/disc_valid_ref.py - 150 x 299, 150 x 300 and 40 x 50 (radii 48 and 121 exceed it: the reflection wraps
more than once), relief of 900 ... 2900 m with a NaN block that has one valid pixel in its middle, NaN at a corner and next to two
borders, +inf, 1e20, a plateau and - ``hard`` - a block of -9999.0 left finite.  Sigmas: radii 2, 3, 9, 13, 24, 48, 121 and three
anisotropic pairs, one axis skipped in two of them.

Bounds (none fitted to a run; gauss_valid_ref.py derives them): value 1e-3 m wherever the reference is finite, weight 1e-4, the
NaN mask exactly the reference's at ``min_weight = 0`` and outside ``|D - min_weight| <= 1e-4`` otherwise.  Every comparison
prints ``FIG ...`` with its largest errors (``pytest -s``)."""
import functools

import numpy as np
import pytest

from oracle import topo_oracle as orc
import disc_valid_ref as dv
import gauss_valid_ref as gv
import topo_descriptors_amd as tda
from topo_descriptors_amd import CFG, _lib, batch, device as d, shard, topo

pytestmark = pytest.mark.gpu

ALL_SIGMAS = gv.SIGMAS + gv.PAIRS + (0.3,)  # (0.3: radius 1, the shortest row groups of axis 0)
CASES = [(k, *s) for k in gv.KINDS for s in gv.SHAPES]
CASE_IDS = [f"{k}{ny}x{nx}" for k, ny, nx in CASES]


@functools.lru_cache(maxsize=None)
def resident(kind, ny=dv.GNY, nx=dv.NX):
    return d.DeviceArray.from_host(dv.raster(kind, ny, nx))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run(block, sigma, min_weight=0.0, fill=False, rows=None, **kw):
    """``(out, weight)`` float32 host planes of ``Block.gaussian_valid``."""
    rows = block.rows if rows is None else rows
    out, weight = d.DeviceArray(rows, block.nx), d.DeviceArray(rows, block.nx)
    try:
        sy, sx = gv.pair(sigma)
        block.gaussian_valid(sy, sx, out, weight=weight, min_weight=min_weight, fill=fill, **kw)
        return out.to_host(), weight.to_host()
    finally:
        out.free()
        weight.free()


@functools.lru_cache(maxsize=None)
def whole(kind, sigma, fill=False):
    """The planes of the call on the whole 150 x 299 raster, shared by the tests that compare bits with it."""
    out, weight = run(d.Block(resident(kind)), sigma, 0.0, fill)
    out.setflags(write=False)
    weight.setflags(write=False)
    return out, weight


# ---- accuracy and NaN masks: every pixel against the reference ------------------------------------------------------------
@pytest.mark.parametrize("sigma", ALL_SIGMAS, ids=str)
@pytest.mark.parametrize("kind,ny,nx", CASES, ids=CASE_IDS)
def test_every_pixel_against_the_reference(kind, ny, nx, sigma):
    ref = gv.reference(kind, sigma, ny, nx)
    block = d.Block(resident(kind, ny, nx))
    for fill in (False, True):
        out, weight = run(block, sigma, 0.0, fill)
        gv.check(out, weight, ref, 0.0, fill, f"gauss_valid {kind} {ny}x{nx} sigma {sigma} fill {fill}")
    assert np.array_equal(np.isnan(out), ~gv.window_has_a_valid_sample(ref.miss, sigma))  # (fill: NaN where the window is empty)


@pytest.mark.parametrize("sigma", ALL_SIGMAS, ids=str)
@pytest.mark.parametrize("kind,ny,nx", CASES, ids=CASE_IDS)
def test_min_weight_against_the_reference(kind, ny, nx, sigma):
    ref = gv.reference(kind, sigma, ny, nx)
    block = d.Block(resident(kind, ny, nx))
    for min_weight in gv.MIN_WEIGHTS:
        for fill in (False, True):
            out, weight = run(block, sigma, min_weight, fill)
            gv.check(out, weight, ref, min_weight, fill, f"gauss_valid {kind} {ny}x{nx} sigma {sigma} min_weight {min_weight} fill {fill}")


def test_the_weight_plane_is_optional_and_changes_nothing():
    out = d.DeviceArray(dv.GNY, dv.NX)
    try:
        d.Block(resident("frac")).gaussian_valid(3.25, 3.25, out)
        assert same_bits(out.to_host(), whole("frac", 3.25)[0])
    finally:
        out.free()


# ---- gap-free raster --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", ALL_SIGMAS, ids=str)
def test_a_gap_free_raster_is_the_plain_gaussian(sigma):
    dem = dv.raster("clean")
    out, weight = run(d.Block(resident("clean")), sigma)
    want = orc.gaussian_exact(dem, sigma)
    err, werr = np.abs(out.astype(np.float64) - want).max(), np.abs(weight.astype(np.float64) - 1.0).max()
    print(f"FIG gauss_valid clean sigma {sigma}: value error {err:.3g} of {gv.VALUE_BOUND}, weight error {werr:.3g} of {gv.WEIGHT_BOUND}")
    assert np.isfinite(out).all() and err <= gv.VALUE_BOUND and werr <= gv.WEIGHT_BOUND
    filled, _ = run(d.Block(resident("clean")), sigma, 0.9, True)
    assert same_bits(filled, out)  # (neither argument has anything to do here)


# ---- sigma 0, radius 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 0.1, (0.0, 0.1)], ids=str)
@pytest.mark.parametrize("fill", [False, True])
def test_no_filter_gives_the_input_bits_and_the_mask(sigma, fill):
    dem = dv.raster("hard")
    miss = dv.missing_mask(dem)
    out, weight = run(d.Block(resident("hard")), sigma, 0.5, fill)
    assert np.array_equal(np.isnan(out), miss) and same_bits(out[~miss], dem[~miss])
    assert same_bits(weight, (~miss).astype(np.float32))


# ---- row blocks -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_raster():
    gny, nx = 420, 512
    dem = orc.synthetic_dem(gny, nx, seed=77)
    dem[139, 200] = np.nan      # next to a block seam for 3 blocks (rows 140, 280)
    dem[300, 31:34] = np.nan
    dem[270:290, 100:180] = np.nan  # across the seam at row 280
    dem[205:215, 400:420] = 1.0e20  # across the seam at row 210 (2 blocks)
    dem[0:3, 500:] = np.nan
    dem.setflags(write=False)
    return dem


@pytest.mark.parametrize("sigma", [3.25, 12.0])
def test_row_blocks_and_windows_give_the_single_block_bits(sigma):
    dem = seam_raster()
    gny, nx = dem.shape
    dev = d.DeviceArray.from_host(dem)
    try:
        up, down = shard.halo_rows(_lib.DESC_GAUSS, sigma)
        assert min(up, down) >= gv.radius(sigma)
        for fill in (False, True):
            w_out, w_weight = run(d.Block(dev), sigma, 0.0, fill)
            gv.check(w_out, w_weight, gv.GaussValidReference(dem, sigma), 0.0, fill, f"gauss_valid seams sigma {sigma} fill {fill}")
            for nb in (2, 3):
                for row0, rows in shard.split_rows(gny, nb):
                    lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
                    part = d.DeviceArray.from_host(np.ascontiguousarray(dem[lo:hi]))
                    try:
                        out, weight = run(d.Block(part, row0=lo, gny=gny), sigma, 0.0, fill, rows=rows, out_row0=row0, out_rows=rows)
                    finally:
                        part.free()
                    assert same_bits(out, w_out[row0:row0 + rows]) and same_bits(weight, w_weight[row0:row0 + rows]), (nb, row0, fill)
            # windows of the whole block, off every row group and tile boundary
            for row0, rows in ((37, 101), (0, 1), (gny - 3, 3)):
                out, weight = run(d.Block(dev), sigma, 0.0, fill, rows=rows, out_row0=row0, out_rows=rows)
                assert same_bits(out, w_out[row0:row0 + rows]) and same_bits(weight, w_weight[row0:row0 + rows]), (row0, rows, fill)
    finally:
        dev.free()


# ---- host paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.75, 3.25, (2.0, 5.0)], ids=str)
def test_topo_dem_gives_the_bits_of_the_resident_call(sigma):
    dem = dv.raster("frac")
    for fill in (False, True):
        want_out, want_weight = whole("frac", sigma, fill)
        out, weight = topo.dem(dem, sigma, skipna=True, fill=fill, return_weight=True)
        assert out.dtype == weight.dtype == np.float32 and same_bits(out, want_out) and same_bits(weight, want_weight)
        assert same_bits(topo.dem(dem, sigma, skipna=True, fill=fill), want_out)
    thresholded = topo.dem(dem, sigma, skipna=True, min_weight=0.5)
    assert same_bits(thresholded, run(d.Block(resident("frac")), sigma, 0.5)[0])


def test_without_skipna_the_bits_are_the_plain_call():
    dem = dv.raster("clean")
    out = d.DeviceArray(dv.GNY, dv.NX)
    try:
        d.Block(resident("clean")).gaussian(3.25, 3.25, out)
        assert same_bits(topo.dem(dem, 3.25), out.to_host())
    finally:
        out.free()


def test_an_int16_source_with_nodata_and_a_packed_dem():
    dem = np.rint(dv.raster("whole"))
    with np.errstate(invalid="ignore"):
        raw = np.where(np.isfinite(dem) & (np.abs(dem) < 30000), dem, -32768).astype(np.int16)
    packed = tda.PackedDem(raw, fill_value=-32768)
    decoded = packed.decode()
    assert np.isnan(decoded).sum() == (raw == -32768).sum() > 1000
    part = d.DeviceArray.from_host(decoded)
    try:
        want_out, want_weight = run(d.Block(part), 2.25, 0.0, True)
    finally:
        part.free()
    gv.check(want_out, want_weight, gv.GaussValidReference(decoded, 2.25), 0.0, True, "gauss_valid int16 source")
    out, weight = topo.dem(packed, 2.25, skipna=True, fill=True, return_weight=True)
    assert same_bits(out, want_out) and same_bits(weight, want_weight)
    # a PackedDem with a scale: centimetres in uint16, 65535 the gap
    cm = tda.PackedDem(np.where(raw == -32768, 65535, raw.astype(np.int64) * 20).astype(np.uint16), scale_factor=0.05, fill_value=65535)
    decoded = cm.decode()
    part = d.DeviceArray.from_host(decoded)
    try:
        want_out, want_weight = run(d.Block(part), 2.25)
    finally:
        part.free()
    out, weight = topo.dem(cm, 2.25, skipna=True, return_weight=True)
    assert np.isnan(out).sum() == (raw == -32768).sum() and same_bits(out, want_out) and same_bits(weight, want_weight)


def test_a_packed_plane_carries_the_fill_code_where_the_result_is_nan():
    dem = dv.raster("frac")
    ref = gv.reference("frac", 3.25)
    dm = tda.Packing(np.int16, 0.1, 0.0, -32768)
    for fill in (False, True):
        plane, _ = whole("frac", 3.25, fill)
        got, weight = topo.dem(dem, 3.25, pack=dm, skipna=True, fill=fill, return_weight=True)
        want = _lib.encode_host(plane, dm)
        want_nan = np.isnan(ref.out(0.0, fill))
        assert isinstance(got, _lib.PackedPlane) and same_bits(got.values, want.values)
        assert (got.missing, got.saturated) == (want.missing, want.saturated)
        assert got.missing == want_nan.sum() > 0 and np.array_equal(got.values == dm.fill_value, want_nan)
        assert same_bits(weight, whole("frac", 3.25, fill)[1])
        assert same_bits(topo.dem(dem, 3.25, pack=dm, skipna=True, fill=fill).values, got.values)


def test_a_dataarray_comes_back_as_one():
    xr = pytest.importorskip("xarray")
    dem = dv.raster("frac")
    da = xr.DataArray(dem.copy(), dims=("y", "x"), coords={"y": np.arange(dv.GNY), "x": np.arange(dv.NX)})
    out, weight = topo.dem(da, 3.25, skipna=True, return_weight=True)
    assert isinstance(out, xr.DataArray) and out.dims == da.dims and same_bits(out.values, whole("frac", 3.25)[0])
    assert isinstance(weight, np.ndarray)
    packed = topo.dem(da, 3.25, skipna=True, pack=tda.Packing(np.int16, 0.1, 0.0, -32768))
    assert isinstance(packed, _lib.PackedPlane)  # (not re-wrapped)


def test_a_dataarray_like_comes_back_as_one():
    class Array:
        def __init__(self, values):
            self.values = values

        def copy(self, data=None):
            return Array(data)

    out = topo.dem(Array(dv.raster("frac")), 3.25, skipna=True)
    assert isinstance(out, Array) and same_bits(out.values, whole("frac", 3.25)[0])


# ---- the chain: smooth over the gaps, then valid-sample TPI / STD ---------------------------------------------------------
@pytest.mark.parametrize("size", [7, 21])
def test_the_chain_into_valid_sample_tpi(size):
    sigma = 2.25
    dem = dv.raster("frac")
    smooth_ref = gv.reference("frac", sigma).out()
    ref = dv.ValidReference(smooth_ref, size)
    smooth, tpi, std = (d.DeviceArray(dv.GNY, dv.NX) for _ in range(3))
    try:
        d.Block(resident("frac")).gaussian_valid(sigma, sigma, smooth)
        d.Block(smooth).tpi_std_valid(size, tpi=tpi, std=std)
        got, got_std = tpi.to_host(), std.to_host()
    finally:
        for p in (smooth, tpi, std):
            p.free()
    dv.check_nans(got, ref.tpi, f"chain size {size} TPI")
    dv.check_nans(got_std, ref.std, f"chain size {size} STD")
    ok = ~np.isnan(ref.tpi)
    err = np.abs(got.astype(np.float64)[ok] - ref.tpi[ok])
    print(f"FIG chain sigma {sigma} size {size}: TPI error {err.max():.3g} of 2e-3")
    assert err.max() <= 2e-3  # one Gaussian tolerance on the centre and one on the mean
    if size == 7:
        host = topo.tpi(topo.dem(dem, sigma, skipna=True), size, skipna=True)
        assert same_bits(host, got)


# ---- compute_dem ------------------------------------------------------------------------------------------------------------
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


def test_compute_dem_with_skipna_fill_a_crop_and_ind_nans():
    dem = dv.raster("frac")
    x = 2600000.0 + 30.0 * np.arange(dv.NX)
    y = 1200000.0 - 30.0 * np.arange(dv.GNY)
    ds = FakeDataset(dem, x, y)
    row0, rows, col0, cols = 9, 120, 13, 203
    crop = {"x": slice(x[col0] - 5.0, x[col0 + cols - 1] + 5.0), "y": slice(y[row0] + 1.0, y[row0 + rows - 1] - 1.0)}
    mask = np.zeros(dem.shape, dtype=bool)
    mask[40, 20:60] = True
    scales = [7 * 30, 21 * 30]
    got = batch.compute_dem(ds, scales, ind_nans=mask, crop=crop, outdir=None, skipna=True, fill=True, min_weight=0.25)
    assert list(got) == list(batch.compute_dem(ds, scales, crop=crop, outdir=None))
    for name, px in zip(got, (7, 21)):
        sigma = px / CFG.scale_std
        full, _ = run(d.Block(resident("frac")), sigma, 0.25, True)
        want = np.where(mask, np.nan, full)[row0:row0 + rows, col0:col0 + cols]
        assert np.isnan(got[name][mask[row0:row0 + rows, col0:col0 + cols]]).all()
        assert same_bits(got[name], want.astype(np.float32)), name


# ---- error codes ------------------------------------------------------------------------------------------------------------
def test_error_codes():
    lib = _lib.lib()
    dem = resident("frac")
    out = d.DeviceArray(dv.GNY, dv.NX)
    try:
        def call(sigma_y, sigma_x, min_weight=0.0, ptr=out.ptr):
            return lib.topo_amd_gaussian_valid_dev(dem.ptr, dv.GNY, 0, dv.GNY, dv.NX, sigma_y, sigma_x, min_weight, 0, 0, dv.GNY, ptr, None)

        assert call(31.0, 31.0) == -5 and call(2.0, 31.0) == -5 and call(1e9, 2.0) == -5  # TOPO_AMD_EUNSUP: radius 124
        for bad in (-0.1, 1.5, float("nan")):
            assert call(2.0, 2.0, bad) == -1  # TOPO_AMD_EINVAL
        assert call(-1.0, 2.0) == -1 and call(2.0, float("nan")) == -1 and call(2.0, 2.0, 0.0, None) == -1
        assert call(30.25, 30.25, 1.0) == 0 and call(0.25, 0.25) == 0  # radii 121 and 1
        d.sync()
    finally:
        out.free()
    with pytest.raises(_lib.TopoAmdError, match="status -5"):
        topo.dem(dv.raster("frac"), 31.0, skipna=True)
    raster = _lib.source_of(dv.raster("frac"))
    host = np.empty((dv.GNY, dv.NX), dtype=np.float32)
    for bad in (-0.1, 1.5, float("nan")):
        assert lib.topo_amd_gauss_valid_raw(_lib.C.byref(raster[1]), dv.GNY, dv.NX, 2.0, 2.0, bad, 0, _lib.ptr(host), None) == -1
