"""The valid-sample gradient (``topo.gradient(skipna=True)``) judged without a GPU: the comparison of
tests/test_gpu_gradient_valid.py against results that are subtly wrong, the definition on a raster without gaps, and the
condition on the reference that lets the GPU tests leave the pixels next to a threshold out."""
import numpy as np
import pytest

from oracle import topo_oracle as orc
import disc_valid_ref as dv
import gauss_valid_ref as gv
import gradient_valid_ref as gr

GAUSS_VARIANTS = ("nan_one_sided", "wrong_side", "no_halving", "unfilled_plane", "centre_only_weight", "finite_only")
SOBEL_VARIANTS = ("correlation", "finite_only")


def as_stored(ref):
    """What a kernel that is exactly right would return: dx, dy rounded to float32, slope and aspect of those."""
    dx, dy = (p.astype(np.float32) for p in ref.planes[:2])
    slope, aspect = (p.astype(np.float32) for p in gr.slope_aspect(dx.astype(np.float64), dy.astype(np.float64)))
    aspect[aspect >= 360.0] = 0.0  # (359.99999 rounds to 360 in float32: the same direction)
    return [dx, dy, slope, aspect]


def fails(got, ref):
    try:
        gr.check(got, ref)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mode", gr.RES_MODES)
@pytest.mark.parametrize("sigma,ratio", gr.CASES, ids=str)
def test_the_reference_itself_passes(sigma, ratio, mode):
    for fill in (False, True):
        ref = gr.reference("frac", dv.GNY, dv.NX, sigma, ratio, mode, 0.0, fill)
        gr.check(as_stored(ref), ref)
        assert not np.isinf(np.concatenate([p.ravel() for p in ref.planes])).any()
        nan = np.isnan(ref.planes[0]) | np.isnan(ref.planes[1])
        assert np.array_equal(np.isnan(ref.planes[2]), nan) and np.array_equal(np.isnan(ref.planes[3]), nan)
        if not fill:
            assert np.isnan(ref.planes[0][ref.miss]).all() and np.isnan(ref.planes[1][ref.miss]).all()


@pytest.mark.parametrize("variant", GAUSS_VARIANTS)
@pytest.mark.parametrize("sigma,ratio", [(3.25, 1), (3.25, 2), (12.0, 1)], ids=str)
def test_the_comparison_notices_a_wrong_difference(sigma, ratio, variant):
    dem = dv.raster("frac")
    res = gr.resolutions("s", dem.shape)
    # (a threshold only where the variant is about one: at min_weight 0 "at the centre only" is the definition itself)
    min_weight = 0.5 if variant == "centre_only_weight" else 0.0
    for fill in (False, True):
        ref = gr.reference("frac", dv.GNY, dv.NX, sigma, ratio, "s", min_weight, fill)
        bad = gr.GradientValidReference(dem, sigma, res, ratio, min_weight, fill, **{variant: True})
        assert not fails(as_stored(ref), ref) and fails(as_stored(bad), ref), (variant, fill)


@pytest.mark.parametrize("variant", SOBEL_VARIANTS)
def test_the_comparison_notices_a_wrong_sobel(variant):
    dem = dv.raster("frac")
    res = gr.resolutions("1d", dem.shape)
    for fill in (False, True):
        ref = gr.reference("frac", dv.GNY, dv.NX, 0.75, 1, "1d", 0.0, fill)
        bad = gr.GradientValidReference(dem, 0.75, res, 1, 0.0, fill, **{variant: True})
        assert not fails(as_stored(ref), ref) and fails(as_stored(bad), ref), (variant, fill)


def test_the_comparison_notices_a_lost_tap_a_nan_off_and_a_wrong_angle():
    ref = gr.reference("frac", dv.GNY, dv.NX, 0.75, 1, "s")
    good = as_stored(ref)
    lost = [p.copy() for p in good]
    lost[0][100, 20] += np.float32(900.0 / 8.0 / 25.0)  # one tap of the smallest weight on the lowest relief
    assert fails(lost, ref)
    ref = gr.reference("frac", dv.GNY, dv.NX, 3.25, 1, "s")
    good = as_stored(ref)
    for k in range(4):
        more, less = [p.copy() for p in good], [p.copy() for p in good]
        more[k][tuple(np.argwhere(~np.isnan(good[k]))[0])] = np.nan
        less[k][tuple(np.argwhere(np.isnan(good[k]))[0])] = 1.0
        assert fails(more, ref) and fails(less, ref), k
    off = [p.copy() for p in good]
    off[1][40, 40] += np.float32(2.5e-3 / 25.0)
    assert fails(off, ref)
    for k, step in ((2, 1e-3), (3, 1e-3)):
        off = [p.copy() for p in good]
        off[k][40, 40] += np.float32(step)
        assert fails(off, ref), k
    inf = [p.copy() for p in good]
    inf[2][40, 40] = np.inf
    assert fails(inf, ref)
    # planes that were left out are not judged
    gr.check([good[0], None, None, None], ref)
    gr.check([None, None, good[2], good[3]], ref)


@pytest.mark.parametrize("sigma,ratio", [c for c in gr.CASES if c[0] > 1], ids=str)
def test_a_gap_free_raster_gives_numpy_gradient_of_the_gaussian(sigma, ratio):
    dem = dv.raster("clean")
    one = {"x": 1.0, "y": 1.0}
    ref = gr.GradientValidReference(dem, sigma, one, ratio)
    want = orc.gradient_exact(dem, sigma, one, ratio)
    for fill, mw in ((False, 0.0), (True, 0.9)):
        ref = gr.GradientValidReference(dem, sigma, one, ratio, mw, fill)
        err = max(float(np.abs(ref.planes[k] - want[k]).max()) for k in (0, 1))
        print(f"FIG clean sigma {sigma} ratio {ratio}: |d - np.gradient(gaussian_exact)| {err:.3g} of 1e-11")
        assert err <= 1e-11
        # one-sided differences at the raster's edges, and only there
        assert not ref.one_sided[0][:, 1:-1].any() and ref.one_sided[0][:, [0, -1]].all()
        assert not ref.one_sided[1][1:-1].any() and ref.one_sided[1][[0, -1]].all()


def test_a_gap_free_raster_gives_the_sobel_pair():
    dem = dv.raster("clean")
    ref = gr.GradientValidReference(dem, 0.75, {"x": 1.0, "y": 1.0})
    want = orc.sobel_exact(dem)
    assert max(float(np.abs(ref.planes[k] - want[k]).max()) for k in (0, 1)) <= 1e-11


def test_a_rim_pixel_keeps_both_neighbours_and_an_isolated_one_has_none():
    dem = dv.raster("frac")
    ref = gr.reference("frac", dv.GNY, dv.NX, 3.25)
    # [60, 120] lies on the upper rim of the NaN block [60:90, 100:160]... inside it; [59, 120] is the valid pixel above it
    assert np.isfinite(ref.planes[1][59, 120]) and not ref.one_sided[1][59, 120]
    # the one valid pixel in the middle of the block: valid, with neighbours the Gaussian fills
    assert np.isfinite(ref.planes[0][75, 130]) and np.isnan(ref.planes[0][75, 131])
    filled = gr.reference("frac", dv.GNY, dv.NX, 3.25, 1, "s", 0.0, True)
    assert np.isfinite(filled.planes[0][75, 131])
    # Sobel: the same pixel has no valid tap at all
    sob = gr.reference("frac", dv.GNY, dv.NX, 0.75)
    assert np.isnan(sob.planes[0][75, 130]) and np.isnan(sob.planes[1][75, 130])
    assert dem[75, 130] == dem[75, 130]


@pytest.mark.parametrize("sigma,ratio", [c for c in gr.CASES if c[0] > 1], ids=str)
@pytest.mark.parametrize("kind,ny,nx", gr.RASTERS, ids=lambda v: str(v))
def test_the_share_left_out_next_to_a_threshold_stays_below_its_cap(kind, ny, nx, sigma, ratio):
    worst = 0.0
    for mw in gr.MIN_WEIGHTS:
        ref = gr.reference(kind, ny, nx, sigma, ratio, "s", mw)
        worst = max(worst, gr.left_out_share(ref))
        assert gr.judged_mask(gr.reference(kind, ny, nx, sigma, ratio)).all()  # (no threshold: every pixel)
    print(f"FIG left out {kind} {ny}x{nx} sigma {sigma} ratio {ratio}: {worst:.4%} of {gr.BAND_SHARE:.2%}")
    assert worst <= gr.BAND_SHARE
