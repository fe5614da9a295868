"""The reference of the valid-sample Gaussian (``topo.dem(skipna=True)``; include/topo_amd.h, topo_amd_gaussian_valid_dev) and
the comparisons the GPU tests hold the kernels to.  ``oracle/`` has no such mode, so the tests carry it themselves.

With ``m`` 1 where a sample is valid and 0 where it is missing (``disc_valid_ref.missing_mask``: not finite, or beyond
+-2**24), ``N`` and ``D`` are ``scipy.ndimage.gaussian_filter(..., mode="reflect", truncate=4.0)`` of the float64 fields
``m * x`` and ``m``, and

    out = N / D   where D > 0, D >= min_weight and (fill or m = 1);   NaN elsewhere;   weight = D.

The keyword arguments of :class:`GaussValidReference` build deliberately WRONG variants (zero padding instead of reflect, a
division between the passes, no normalisation, only non-finite samples treated as missing) for
tests/test_gauss_valid_design.py, which shows that :func:`check` notices each.

Bounds (none fitted to a run).  Value: ``|out - ref| <= 1e-3`` m wherever the reference is finite - what
tests/test_gpu_parity.py holds ``topo.dem`` to against the float64 filter on the same kind of relief; no rounding of the
kernels is amplified by a small ``D`` (every term is bounded by ``D max|x - c|`` before the division).  Weight:
``|weight - D| <= 1e-4`` - at most 2 x 243 roundings of terms that sum to at most 1, about 3e-5 in float32.  NaN mask: the
reference's exactly at ``min_weight = 0``; for ``min_weight > 0`` at every pixel with ``|D - min_weight| > 1e-4`` (the weight
bound), and those left out may be at most 0.5 % of the raster - a condition on the reference, asserted."""
import functools

import numpy as np
from scipy import ndimage

import disc_valid_ref as dv

SIGMAS = (0.6, 0.75, 2.25, 3.25, 6.0, 12.0, 30.25)  # radii 2, 3, 9, 13, 24, 48, 121
PAIRS = ((3.25, 0.0), (0.0, 2.25), (2.0, 5.0))
KINDS = ("frac", "hard", "whole")
SHAPES = ((dv.GNY, dv.NX), (dv.GNY, 300), dv.SMALL)
MIN_WEIGHTS = (0.25, 0.5, 0.9)
VALUE_BOUND, WEIGHT_BOUND, BAND_SHARE = 1e-3, 1e-4, 0.005


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def pair(sigma):
    return tuple(float(s) for s in np.broadcast_to(np.asarray(sigma, dtype=np.float64), (2,)))


class GaussValidReference:
    """``N``, ``D`` (float64) of ``dem`` for one ``sigma`` (a scalar or an (axis 0, axis 1) pair), ``miss`` the mask of missing
    samples, and :meth:`out` the result under ``min_weight`` and ``fill``."""

    def __init__(self, dem, sigma, zero_padding=False, divide_between=False, no_normalisation=False, finite_only=False):
        dem = np.asarray(dem, dtype=np.float32)
        self.sigma = pair(sigma)
        self.miss = ~np.isfinite(dem) if finite_only else dv.missing_mask(dem)
        m = (~self.miss).astype(np.float64)
        x = np.where(self.miss, 0.0, dem).astype(np.float64)
        mode = "constant" if zero_padding else "reflect"  # (the WRONG border: taps beyond it count for nothing)

        def smooth(field, sig):
            return ndimage.gaussian_filter(field, sig, mode=mode, cval=0.0, truncate=4.0)

        self.D = smooth(m, self.sigma)
        self.N = smooth(m * x, self.sigma)
        self.no_normalisation = no_normalisation
        if divide_between:  # the WRONG order: a quotient behind axis 0, normalised again behind axis 1
            d0, n0 = smooth(m, (self.sigma[0], 0.0)), smooth(m * x, (self.sigma[0], 0.0))
            have = d0 > 0
            q0 = np.divide(n0, d0, out=np.zeros_like(n0), where=have)
            d1 = smooth(have.astype(np.float64), (0.0, self.sigma[1]))
            n1 = smooth(q0, (0.0, self.sigma[1]))
            self.N = np.divide(n1, d1, out=np.zeros_like(n1), where=d1 > 0) * self.D

    def out(self, min_weight=0.0, fill=False):
        ok = (self.D > 0) & (self.D >= min_weight)
        if not fill:
            ok &= ~self.miss
        q = self.N if self.no_normalisation else np.divide(self.N, self.D, out=np.zeros_like(self.N), where=self.D > 0)
        return np.where(ok, q, np.nan)


@functools.lru_cache(maxsize=None)
def reference(kind, sigma, ny=dv.GNY, nx=dv.NX):
    """The :class:`GaussValidReference` of a raster of ``disc_valid_ref.raster``, computed once for all the tests."""
    return GaussValidReference(dv.raster(kind, ny, nx), sigma)


def window_has_a_valid_sample(miss, sigma):
    """Whether the reflected (2 R_y + 1) x (2 R_x + 1) window of each pixel holds a valid sample (no Gaussian involved)."""
    ry, rx = (radius(s) if s > 1e-15 else 0 for s in pair(sigma))
    return ndimage.maximum_filter((~miss).astype(np.uint8), size=(2 * ry + 1, 2 * rx + 1), mode="reflect") > 0


def check(got, weight, ref, min_weight=0.0, fill=False, label="gauss_valid"):
    """``got`` / ``weight`` (float32 planes; ``weight`` may be ``None``) against the reference under the module's bounds.
    Prints ``FIG ...`` with the largest errors before it asserts."""
    want = ref.out(min_weight, fill)
    nan, want_nan = np.isnan(got), np.isnan(want)
    judged = np.ones(want.shape, dtype=bool) if min_weight == 0.0 else np.abs(ref.D - min_weight) > WEIGHT_BOUND
    left_out = 1.0 - judged.mean()
    assert left_out <= BAND_SHARE, f"{label}: {left_out:.4%} of the pixels lie within {WEIGHT_BOUND} of min_weight"
    ok = judged & ~want_nan
    verr = np.abs(got.astype(np.float64) - want)[ok & ~nan]
    werr = None if weight is None else np.abs(weight.astype(np.float64) - ref.D)
    print(f"FIG {label}: value error {verr.max() if verr.size else 0.0:.3g} of {VALUE_BOUND}, weight error "
          f"{'-' if werr is None else format(werr.max(), '.3g')} of {WEIGHT_BOUND}, {int(ok.sum())} pixels, "
          f"{left_out:.4%} left out")
    wrong = judged & (nan != want_nan)
    assert not wrong.any(), (f"{label}: {int((wrong & nan).sum())} NaN too many, {int((wrong & ~nan).sum())} too few, "
                             f"first at {np.argwhere(wrong)[0].tolist()}")
    assert not np.isinf(got).any(), f"{label}: an infinite output"
    if verr.size:
        assert verr.max() <= VALUE_BOUND, f"{label}: value error {verr.max():.6g} m"
    if weight is not None:
        assert np.isfinite(weight).all() and werr.max() <= WEIGHT_BOUND, f"{label}: weight error {werr.max():.6g}"
