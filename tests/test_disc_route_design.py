"""The comparisons of tests/test_gpu_disc_routes.py, judged on the float64 oracle alone (no GPU): a result computed with a
subtly wrong disc - one rim tap lost, one disc row's run shifted by a column, with the full tap count kept as a kernel with
a wrong run table would - or with a tile seam in it (a row at a tile-row boundary or the column at a strip boundary repeated)
must fail the value bounds for TPI and for STD, and a NaN footprint one pixel too wide or too narrow the NaN comparison."""
import numpy as np
import pytest

from oracle import topo_oracle as orc
import test_gpu_disc_routes as routes
from test_gpu_disc_routes import Reference, check_nans, check_std, check_tpi, raster, reference, shape_of


# ---- the route word of every odd size, from the thresholds ``ROUTES`` documents ---------------------------------------------
TPI_RING_MAX = 17        # TPI alone: the ring build, 5 ... 17 px (below 17 px without it: one marching kernel, no second pass)
STD_SPEC_WIDE_MAX = 13   # TPI + STD on whole metres: the 512-column build (STD alone from 2^27 pixels and up to 7 px only)
STD_SPEC_BOTH_MAX = 21   # the second pass over fractional tiles in the form with staging waves apart
STD_RING_BOTH_MAX = 41   # ... in the ring kernel's form; up to here the first pass has staging waves apart (tiles of 48 rows)
STD_RING_MAX = 67        # STD / TPI + STD: the ring kernel
FULL_TILE_MAX = 77       # LDS holds the 60-row tile of the marching kernels


def tile_rows(size, nwaves, cap):
    """Rows of a tile of the marching (12 waves, at most 60) and general (8 waves, at most 64) kernels: what 160 KiB hold."""
    th = cap
    while th > nwaves and (th + size + nwaves) * 256 * 4 + (th * (size + 1) + 8) * 2 + 16 > 160 * 1024:
        th -= nwaves
    return th


def route_rule(size, op, cls, one_block=True, big=False):
    """The kernels (``ROUTES``' part of the word) of an odd ``size`` from 3 to 101, ``op`` of ``OPS`` and raster class ``cls``
    (0 whole metres, 1 at most half fractional, 2 mostly fractional); ``big``: a call of 2^27 pixels or more."""
    assert size % 2 == 1 and 3 <= size <= 101
    r = routes
    th12, th8 = tile_rows(size, 12, 60), tile_rows(size, 8, 64)
    assert (th12 == 60) == (size <= FULL_TILE_MAX)
    if op == "tpi":
        if 5 <= size <= TPI_RING_MAX:
            return r.kernels(r.F_RING, 64, r.FR_RING_BOTH | r.DEFERRED)
        if size < TPI_RING_MAX:
            return r.kernels(r.F_MARCH, th12, r.DEFERRED)
        if size == 67 and cls == 0 and one_block:
            return r.kernels(r.F_WIDE, 64, r.SCALED | r.DEFERRED) | r.WIDE_BIT
        if cls == 2:
            return r.kernels(r.F_SCALED_ALL, th12, r.DEFERRED)
        return r.kernels(r.F_MARCH, th12, r.SCALED | r.DEFERRED)
    if 5 <= size <= STD_RING_MAX:
        if cls == 2 and size > STD_RING_BOTH_MAX:
            return r.kernels(r.F_SUMS, th12, r.STD_MARCH | r.FR_MARCH | r.DEFERRED)
        spec = size <= STD_RING_BOTH_MAX
        if cls == 0 and size <= STD_SPEC_WIDE_MAX and (op == "tpi_std" or (size <= 7 and big)):
            return r.kernels(r.F_SPEC8, 48, r.DEFERRED)
        second = r.FR_SPEC_BOTH if size <= STD_SPEC_BOTH_MAX else r.FR_STD_RING_BOTH if size <= STD_RING_BOTH_MAX else 0
        return r.kernels(r.F_SPEC4 if spec else r.F_STD_RING, 48 if spec else 60, second | r.DEFERRED)
    if size >= 31 and th12 == 60:
        return r.kernels(r.F_MARCH, th12, r.STD_MARCH | r.DEFERRED)
    return r.kernels(r.F_GENERAL, th8, 0)


def test_route_rule_reproduces_the_pinned_routes():
    assert sorted(routes.ROUTES) == list(routes.SIZES)
    for size, by_op in routes.ROUTES.items():
        for op, by_class in zip(routes.OPS, by_op):
            for cls, word in enumerate(by_class):
                assert route_rule(size, op, cls) == word, (size, op, cls, hex(route_rule(size, op, cls)), hex(word))
    assert route_rule(67, "tpi", 0, one_block=False) == routes.MARCH_SCALED
    assert route_rule(7, "std", 0, big=True) == routes.SPEC8 and route_rule(9, "std", 0, big=True) == routes.SPEC4_SPEC


def shifted(field, dj, di):
    """field[j + dj, i + di] with the convolution's zero padding."""
    ny, nx = field.shape
    pad = max(abs(dj), abs(di))
    big = np.zeros((ny + 2 * pad, nx + 2 * pad))
    big[pad:pad + ny, pad:pad + nx] = field
    return big[pad + dj:pad + dj + ny, pad + di:pad + di + nx]


def with_taps_changed(ref, size, removed, added):
    """(TPI, STD) of the reference's formulas over the disc without the taps ``removed`` and with the taps ``added`` (the tap
    count stays the disc's: a kernel's run table went wrong, not its constants)."""
    x = ref.clean.astype(np.float64)
    t2 = np.trunc(x) ** 2
    n = len(orc.disc_taps(size)[0])
    s1 = orc._disc_sum_f64(x, size, drop_centre=False)[0]
    s2 = orc._disc_sum_f64(t2, size, drop_centre=False)[0]
    for sign, taps in ((-1.0, removed), (1.0, added)):
        for dj, di in taps:
            s1 = s1 + sign * shifted(x, dj, di)
            s2 = s2 + sign * shifted(t2, dj, di)
    tpi = x - (s1 - x) / (n - 1)  # (odd sizes: the tap TPI leaves out is the pixel itself)
    std = np.sqrt(np.clip((s2 - s1 * s1 / n) / (n - 1), 0, None))
    return tpi, std


def fails(check, *args, **kwargs):
    try:
        check(*args, **kwargs)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("kind", ["whole", "hard_frac"])
@pytest.mark.parametrize("size", [7, 43, 77, 101])
def test_a_subtly_wrong_disc_fails_the_value_bounds(size, kind):
    ny, nx = shape_of(size)
    ref = reference(kind, size, ny, nx)
    dj, di, _ = orc.disc_taps(size)
    # the reference itself passes (and so does its float32 rounding, TPI alone with the scaled route's allowance too)
    check_tpi(ref.tpi_as_stored(), ref)
    check_tpi(ref.tpi_as_stored(), ref, scaled_allowance=True)
    check_std(ref.std_as_stored(), ref)
    unchanged = with_taps_changed(ref, size, [], [])
    ok = ~ref.nan
    assert np.max(np.abs(unchanged[0][ok] - ref.tpi[ok])) < 1e-9 and np.max(np.abs(unchanged[1][ok] - ref.std[ok])) < 1e-6
    # one rim tap removed: the first tap of the topmost disc row
    top = int(dj.max())
    rim = (top, int(di[dj == top].min()))
    # one disc row's run shifted by a column: the row a quarter of the way down
    row = int(dj.max()) - size // 4
    lo, hi = int(di[dj == row].min()), int(di[dj == row].max())
    for removed, added in (([rim], []), ([(row, lo)], [(row, hi + 1)])):
        tpi, std = with_taps_changed(ref, size, removed, added)
        tpi[ref.nan], std[ref.nan] = np.nan, np.nan
        assert fails(check_tpi, tpi.astype(np.float32), ref, scaled_allowance=True), (removed, added)
        assert fails(check_std, std.astype(np.float32), ref), (removed, added)
    # a tile seam: the row at a tile-row boundary of 48 / 60 rows, the column at a strip boundary, repeated
    for axis, index in ((0, 48), (0, 60), (1, 512)):
        for check, plane, kwargs in ((check_tpi, ref.tpi_as_stored(), {"scaled_allowance": True}), (check_std, ref.std_as_stored(), {})):
            seam = plane.copy()
            if axis == 0:
                seam[index] = np.where(np.isnan(seam[index]), np.nan, seam[index - 1])
            else:
                seam[:, index] = np.where(np.isnan(seam[:, index]), np.nan, seam[:, index - 1])
            seam[ref.nan] = np.nan
            assert fails(check, seam, ref, **kwargs), (axis, index, check.__name__)


@pytest.mark.parametrize("size", [7, 77])
def test_a_footprint_a_pixel_off_fails_the_nan_comparison(size):
    ref = reference("hard_frac", size)
    plane = ref.tpi_as_stored()
    check_nans(plane, ref.nan)
    grown = ref.nan | np.roll(ref.nan, 1, axis=0) | np.roll(ref.nan, -1, axis=0) | np.roll(ref.nan, 1, axis=1) | np.roll(ref.nan, -1, axis=1)
    shrunk = ref.nan & np.roll(ref.nan, 1, axis=0) & np.roll(ref.nan, -1, axis=0) & np.roll(ref.nan, 1, axis=1) & np.roll(ref.nan, -1, axis=1)
    one_more = ref.nan.copy()
    one_more[tuple(np.argwhere(grown & ~ref.nan)[0])] = True
    one_less = ref.nan.copy()
    one_less[tuple(np.argwhere(ref.nan & ~shrunk)[0])] = False
    for wrong in (grown, shrunk, one_more, one_less):
        assert not np.array_equal(wrong, ref.nan)
        assert fails(check_nans, np.where(wrong, np.nan, np.where(ref.nan, 0.0, plane)).astype(np.float32), ref.nan)


def test_reference_masks():
    """The three masks share one tap-by-tap sum: each against a sum of its own."""
    dem = raster("hard_frac")
    ref = Reference(dem, 13)
    finite = np.isfinite(dem) & (np.abs(dem) < 2.0 ** 24)
    for mask, field in ((ref.nan, ~finite), (ref.near, finite & (np.abs(dem) >= 9999.0)), (ref.fractional, finite & (dem != np.trunc(dem)))):
        assert np.array_equal(mask, orc._disc_sum_f64(field.astype(np.float64), 13, drop_centre=False)[0] > 0)
    assert ref.nan.any() and not ref.nan.all() and (ref.near & ~ref.nan).any() and not ref.near.all()
