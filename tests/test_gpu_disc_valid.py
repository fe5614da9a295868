"""Valid-sample TPI / STD (``skipna=True``; csrc/disc_valid.hip) on the GPU, every pixel against the exact reference of
tests/disc_valid_ref.py (tests/test_disc_valid_design.py shows what its comparisons notice).

Rasters: 150 x 299 (several tiles of 32 x 128 both ways at a 67 px halo, odd width), a second width of 300, and 40 x 50 with a
67 px disc (``nx < size``); relief of 900 ... 2900 m in multiples of 1/64 m and in whole metres, with a NaN block that has one
valid pixel in its middle, NaN at [0, 0] and one pixel from a border, +inf, 1e20, a plateau, and - ``hard`` - a 30 x 200 block
of -9999.0 left finite, which must take the exact slow form (bit 27 of ``device.disc_route()``) while no other raster does.

Bounds (none fitted to a run).  NaN pattern: the reference's exactly.  TPI: 1 float32 ulp of the reference's value.  STD:
``ulp32(ref) + delta / max(ref, sqrt(delta))``, ``delta = 2**-50 max(s2, s1**2 / n) / (n - 1)`` per pixel.  Against the existing
``topo.tpi`` / ``topo.std`` (``min_count`` = the full tap count, NaN-free interior): TPI bit for bit on whole metres and within
the 2**-9 m the header states for the scaled route on fractional ones; STD within ``3e-7 ref + ulp32(ref)`` - the 3e-7 relative
that csrc/disc_wave_impl.hpp (``std_from_int_sums``) derives for the float32 tail of the existing kernels, plus the one rounding
of this mode.  Every comparison prints ``FIG ...`` with the largest error as a share of its bound (``pytest -s``)."""
import ctypes as C
import functools

import numpy as np
import pytest

import disc_valid_ref as dv
import topo_descriptors_amd as tda
from topo_descriptors_amd import _lib, batch, device as d, topo

pytestmark = pytest.mark.gpu

OPS = ("tpi", "std", "tpi_std")
VALID, SLOW, TILE_ROWS = 6, 1 << 27, 32
WANT = {"tpi": 1 << 3, "std": 1 << 4, "tpi_std": 3 << 3}
CASES = [("frac", dv.GNY, dv.NX), ("whole", dv.GNY, dv.NX), ("hard", dv.GNY, dv.NX), ("frac", dv.GNY, 300)]


@functools.lru_cache(maxsize=None)
def resident(kind, ny=dv.GNY, nx=dv.NX):
    return d.DeviceArray.from_host(dv.raster(kind, ny, nx))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run(block, size, op, min_count=1, rows=None, **kw):
    """``(tpi, std)`` float32 host planes (``None`` for the one not asked for) of ``Block.tpi_std_valid``, and the route word."""
    rows = block.rows if rows is None else rows
    t = d.DeviceArray(rows, block.nx) if "tpi" in op else None
    s = d.DeviceArray(rows, block.nx) if "std" in op else None
    try:
        block.tpi_std_valid(size, tpi=t, std=s, min_count=min_count, **kw)
        route = d.disc_route()
        return (t.to_host() if t else None), (s.to_host() if s else None), route
    finally:
        for p in (t, s):
            if p is not None:
                p.free()


@functools.lru_cache(maxsize=None)
def fused(kind, size, ny=dv.GNY, nx=dv.NX, min_count=1):
    """The planes of the TPI + STD call on a whole raster: what the other calls must reproduce bit for bit."""
    t, s, _ = run(d.Block(resident(kind, ny, nx)), size, "tpi_std", min_count)
    t.setflags(write=False)
    s.setflags(write=False)
    return t, s


# ---- bounds: every pixel against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("size", dv.SIZES)
@pytest.mark.parametrize("kind,ny,nx", CASES, ids=[f"{k}{nx}" for k, _, nx in CASES])
def test_every_pixel_against_the_reference(kind, ny, nx, size, op):
    ref = dv.reference(kind, size, 1, ny, nx)
    t, s, route = run(d.Block(resident(kind, ny, nx)), size, op)
    label = f"valid {kind} {ny}x{nx} size {size} {op}"
    assert route & ~SLOW == VALID | WANT[op] | (TILE_ROWS << 16), hex(route)
    assert bool(route & SLOW) == (kind == "hard"), f"{label}: slow-form bit {hex(route)}"
    if t is not None:
        dv.check_tpi(t, ref, label + " TPI")
    if s is not None:
        dv.check_std(s, ref, label + " STD")
    if op != "tpi_std":  # TPI alone and STD alone: the planes of TPI + STD, bit for bit
        ft, fs = fused(kind, size, ny, nx)
        assert same_bits(t, ft) if op == "tpi" else same_bits(s, fs), label


@pytest.mark.parametrize("op", OPS)
def test_a_raster_narrower_than_the_disc(op):
    ny, nx = dv.SMALL
    ref = dv.reference("frac", 67, 1, ny, nx)
    assert (ref.n < ref.n.max()).any() and nx < 67
    t, s, route = run(d.Block(resident("frac", ny, nx)), 67, op)
    assert route == VALID | WANT[op] | (TILE_ROWS << 16), hex(route)
    if t is not None:
        dv.check_tpi(t, ref, f"valid 40x50 size 67 {op} TPI")
    if s is not None:
        dv.check_std(s, ref, f"valid 40x50 size 67 {op} STD")


def test_a_valid_centre_without_a_valid_neighbour_is_nan():
    """The single valid pixel inside the NaN block: n' = 0, so TPI is NaN; n = 1, so STD is NaN."""
    ref = dv.reference("frac", 7)
    assert ref.n[75, 130] == 1 and ref.n1[75, 130] == 0 and not dv.missing_mask(dv.raster("frac"))[75, 130]
    t, s = fused("frac", 7)
    assert np.isnan(t[75, 130]) and np.isnan(s[75, 130])
    assert not np.isnan(t[59, 130]) and not np.isnan(s[59, 130])  # next to the block: its own valid taps


# ---- cut invariance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [3, 4, 7, 21, 67, 101])
@pytest.mark.parametrize("kind", ["frac", "hard"])
def test_row_blocks_and_windows_give_the_single_call_bits(kind, size):
    dem = dv.raster(kind)
    ft, fs = fused(kind, size)
    above, below = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().topo_amd_halo_rows(_lib.DESC_TPI, float(size), 0.0, C.byref(above), C.byref(below)), "halo_rows")
    # three row blocks with their ghost rows; the seam at row 75 runs through the NaN block (rows 60 ... 89)
    for r0, r1 in ((0, 75), (75, 110), (110, dv.GNY)):
        lo, hi = max(0, r0 - above.value), min(dv.GNY, r1 + below.value)
        part = d.DeviceArray.from_host(np.ascontiguousarray(dem[lo:hi]))
        try:
            t, s, _ = run(d.Block(part, row0=lo, gny=dv.GNY), size, "tpi_std", rows=r1 - r0, out_row0=r0, out_rows=r1 - r0)
        finally:
            part.free()
        assert same_bits(t, ft[r0:r1]) and same_bits(s, fs[r0:r1]), (kind, size, r0, r1)
    # windows of the whole block, off every tile boundary
    for r0, n in ((37, 50), (0, 1), (dv.GNY - 3, 3)):
        t, s, _ = run(d.Block(resident(kind)), size, "tpi_std", rows=n, out_row0=r0, out_rows=n)
        assert same_bits(t, ft[r0:r0 + n]) and same_bits(s, fs[r0:r0 + n]), (kind, size, r0, n)


# ---- min_count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [4, 7, 21])
def test_min_count_against_the_reference(size):
    taps = topo.circular_kernel(size).sum()
    block = d.Block(resident("frac"))
    for min_count in (1, 2, int(taps)):
        ref = dv.reference("frac", size, min_count)
        t, s, _ = run(block, size, "tpi_std", min_count)
        dv.check_tpi(t, ref, f"valid frac size {size} min_count {min_count} TPI")
        dv.check_std(s, ref, f"valid frac size {size} min_count {min_count} STD")
    assert np.isnan(t).all()  # n' is at most taps - 1


@pytest.mark.parametrize("kind", ["clean", "whole_clean"])
@pytest.mark.parametrize("size", [7, 21, 67])
def test_the_full_count_leaves_the_existing_result_on_the_interior(kind, size):
    """NaN-free raster, ``min_count`` = every tap (TPI: every tap but the one it excludes): the outputs that survive are the
    pixels whose disc lies inside the raster, and there the mode is the existing ``topo.tpi`` / ``topo.std``."""
    dem = dv.raster("clean") if kind == "clean" else np.rint(dv.raster("clean"))
    taps = int(topo.circular_kernel(size).sum())
    reach = size // 2
    inside = np.zeros(dem.shape, dtype=bool)
    inside[reach:dem.shape[0] - reach, reach:dem.shape[1] - reach] = True
    tpi = topo.tpi(dem, size, skipna=True, min_count=taps - 1)
    std = topo.std(dem, size, skipna=True, min_count=taps)
    assert tpi.dtype == np.float32 and std.dtype == np.float64
    assert np.array_equal(np.isnan(tpi), ~inside) and np.array_equal(np.isnan(std), ~inside)
    old_tpi, old_std = topo.tpi(dem, size), topo.std(dem, size)
    label = f"valid {kind} size {size} full count against the existing"
    if kind == "whole_clean":
        assert same_bits(tpi[inside], old_tpi[inside]), label
    else:
        scaled = size >= 19  # TPI alone on fractional elevations, discs from 19 px: x in units of 2**-8 m
        bound = np.full(int(inside.sum()), 2.0 ** -9 if scaled else 0.0) + dv.ulp32(old_tpi[inside].astype(np.float64))
        dv.report(np.abs(tpi[inside].astype(np.float64) - old_tpi[inside]), bound, inside, label + " TPI")
    want = old_std[inside]
    dv.report(np.abs(std[inside] - want), 3e-7 * want + dv.ulp32(want), inside, label + " STD")


# ---- entry points ---------------------------------------------------------------------------------------------------------
def test_an_int16_source_with_nodata_through_the_raw_entry_point():
    dem = np.rint(dv.raster("whole"))
    with np.errstate(invalid="ignore"):
        raw = np.where(np.isfinite(dem) & (np.abs(dem) < 30000), dem, -32768).astype(np.int16)
    packed = tda.PackedDem(raw, fill_value=-32768)
    decoded = packed.decode()
    assert np.isnan(decoded).sum() == (raw == -32768).sum() > 1000
    part = d.DeviceArray.from_host(decoded)
    try:
        t, s, _ = run(d.Block(part), 21, "tpi_std", 3)
    finally:
        part.free()
    dv.check_tpi(t, dv.ValidReference(decoded, 21, 3), "valid int16 source size 21 TPI")
    got_t, got_s = topo.tpi_std(packed, 21, skipna=True, min_count=3)
    assert same_bits(got_t, t) and got_s.dtype == np.float64 and same_bits(got_s.astype(np.float32), s)
    assert same_bits(topo.tpi(packed, 21, skipna=True, min_count=3), t)
    assert same_bits(topo.std(packed, 21, skipna=True, min_count=3), got_s)


def test_packed_planes_carry_the_fill_code_where_the_result_is_nan():
    dem = dv.raster("frac")
    t, s = fused("frac", 7)
    tpi_dm = tda.Packing(np.int16, 0.1, 0.0, -32768)
    std_cm = tda.Packing(np.uint16, 0.01, 0.0, 65535)
    got_t, got_s = topo.tpi_std(dem, 7, pack=(tpi_dm, std_cm), skipna=True)
    for got, plane, packing in ((got_t, t, tpi_dm), (got_s, s, std_cm)):
        want = _lib.encode_host(plane, packing)
        assert isinstance(got, _lib.PackedPlane) and same_bits(got.values, want.values)
        assert (got.missing, got.saturated) == (want.missing, want.saturated)
        assert got.missing == np.isnan(plane).sum() > 0
        assert (got.values[np.isnan(plane)] == packing.fill_value).all()
        assert (got.values[~np.isnan(plane)] != packing.fill_value).all()
    assert same_bits(topo.tpi(dem, 7, pack=tpi_dm, skipna=True).values, got_t.values)
    assert same_bits(topo.std(dem, 7, pack=std_cm, skipna=True).values, got_s.values)


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


def test_compute_tpi_and_std_with_skipna_and_a_crop():
    dem = dv.raster("frac")
    x = 2600000.0 + 30.0 * np.arange(dv.NX)
    y = 1200000.0 - 30.0 * np.arange(dv.GNY)
    ds = FakeDataset(dem, x, y)
    row0, rows, col0, cols = 9, 120, 13, 203
    crop = {"x": slice(x[col0] - 5.0, x[col0 + cols - 1] + 5.0), "y": slice(y[row0] + 1.0, y[row0 + rows - 1] - 1.0)}
    scales = [7 * 30, 21 * 30]  # 7 and 21 px: without skipna they would share no pass either way; the names stay
    got = batch.compute_tpi(ds, scales, crop=crop, outdir=None, skipna=True, min_count=2)
    assert list(got) == list(batch.compute_tpi(ds, scales, crop=crop, outdir=None))
    for name, size in zip(got, (7, 21)):
        t, _, _ = run(d.Block(resident("frac")), size, "tpi", 2)
        assert same_bits(got[name], t[row0:row0 + rows, col0:col0 + cols]), name
    mask = np.zeros(dem.shape, dtype=bool)
    mask[40, 20:60] = True
    got = batch.compute_std(ds, scales[:1], ind_nans=mask, crop=crop, outdir=None, skipna=True)
    (name, plane), = got.items()
    _, s, _ = run(d.Block(resident("frac")), 7, "std")
    want = np.where(mask, np.nan, s)[row0:row0 + rows, col0:col0 + cols].astype(np.float64)
    assert plane.dtype == np.float64 and same_bits(plane, want), name


def test_a_dataarray_like_comes_back_as_one():
    class Array:
        def __init__(self, values):
            self.values = values

        def copy(self, data=None):
            return Array(data)

    dem = dv.raster("frac")
    out = topo.tpi(Array(dem), 7, skipna=True)
    assert isinstance(out, Array) and same_bits(out.values, fused("frac", 7)[0])


# ---- error codes ----------------------------------------------------------------------------------------------------------
def test_error_codes():
    lib = _lib.lib()
    dem = resident("frac")
    out = d.DeviceArray(dv.GNY, dv.NX)
    try:
        def call(size, min_count, tpi=out.ptr, std=None):
            return lib.topo_amd_tpi_std_valid_dev(dem.ptr, dv.GNY, 0, dv.GNY, dv.NX, size, min_count, 0, dv.GNY, tpi, std)

        assert call(103, 1) == -5  # TOPO_AMD_EUNSUP: the prefix-plane route is a follow-up
        assert call(0, 1) == -1 and call(7, 0) == -1 and call(7, 1, None, None) == -1  # TOPO_AMD_EINVAL
        assert call(101, 1) == 0 and call(1, 1) == 0
        d.sync()
    finally:
        out.free()
    with pytest.raises(_lib.TopoAmdError, match="status -5"):
        topo.tpi(dv.raster("frac"), 103, skipna=True)
