"""The comparisons of tests/test_gpu_disc_routes.py, judged on the float64 oracle alone (no GPU): a result computed with a
subtly wrong disc - one rim tap lost, one disc row's run shifted by a column, with the full tap count kept as a kernel with
a wrong run table would - or with a tile seam in it (a row at a tile-row boundary or the column at a strip boundary repeated)
must fail the value bounds for TPI and for STD, and a NaN footprint one pixel too wide or too narrow the NaN comparison."""
import numpy as np
import pytest

from oracle import topo_oracle as orc
from test_gpu_disc_routes import Reference, check_nans, check_std, check_tpi, raster, reference, shape_of


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
