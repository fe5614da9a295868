"""The line rasters of tests/test_gpu_gradient_routes.py, judged on the float64 oracle alone (no GPU): zeros with lines of
height H on whole columns (rows).  The smoothed field is H w[i - line] there, so dx (dy) is H (w[i+1] - w[i-1]) / (2 res): a
filter that lost ANY single tap, or sits one pixel off, must fail the comparison the GPU tests make at the case's ``c``."""
import numpy as np
import pytest

from oracle import topo_oracle as orc
from test_gpu_gradient_routes import CASES, case, line_cap, line_units, pieces_of, radius


def lines_gradient(dem, sigma, res, axis):
    """``gradient(lost=None, shift=0)``: dx, dy of the float64 gradient whose filter along ``axis`` lost tap ``lost`` (no
    renormalisation: a tap the kernel never added) or sits ``shift`` pixels off; the other axis keeps the exact filter."""
    w, R = orc.gaussian_weights(sigma)
    other = np.array(orc.gaussian_exact(dem, (0.0, sigma) if axis == 0 else (sigma, 0.0)))
    padded = np.pad(other, [(R, R) if a == axis else (0, 0) for a in (0, 1)], mode="symmetric")
    n = other.shape[axis]

    def window(t):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(t, t + n)
        return padded[tuple(sl)]

    full = sum(w[t] * window(t) for t in range(2 * R + 1))

    def gradient(lost=None, shift=0):
        f = full if lost is None else full - w[lost] * window(lost)
        dy, dx = np.gradient(np.roll(f, shift, axis=axis))
        dx, dy = np.array(dx), np.array(dy)
        orc._divide_by_resolution(dx, dy, res)
        return dx, dy

    return gradient


@pytest.mark.parametrize("name", ["fused4_r5", "split7_r65", "wave_r122", "block_r13"])
def test_a_lost_or_shifted_tap_fails_the_line_comparison(name):
    _, _, sigma, ratio, _, _, c = CASES[name]
    assert ratio == 1 and 2 <= c <= line_cap(sigma)
    for raster, axis in (("cols", 1), ("rows", 0)):
        dem, res, want = case(name, raster)
        _, o0, o1 = pieces_of(name, raster)  # (a row block: only its output rows are compared)

        def units(planes):
            return line_units([p[o0:o1] for p in planes], want, res, (o0, o1))

        gradient = lines_gradient(dem, sigma, res, axis)
        assert units(gradient()) <= 1e-3  # (the helper is the oracle)
        for t in range(2 * radius(sigma) + 1):
            assert units(gradient(lost=t)) > c, (name, raster, t)
        for shift in (1, -1):
            assert units(gradient(shift=shift)) > c, (name, raster, shift)
