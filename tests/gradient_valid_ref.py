"""The reference of the valid-sample gradient (``topo.gradient(skipna=True)``; include/topo_amd.h,
topo_amd_gradient_valid_dev) and the comparison the GPU tests hold the kernels to.  ``oracle/`` has no such mode, so the
tests carry it themselves, in float64, on top of ``gauss_valid_ref.GaussValidReference`` and ``disc_valid_ref``.

The definition.  ``m`` is ``disc_valid_ref.missing_mask``: not finite, or beyond +-2**24.

``sigma > 1``: ``q = N / D`` of the valid-sample Gaussian where ``D > 0`` and ``D >= min_weight`` (its ``fill=True`` plane),
undefined elsewhere.  At a pixel where ``q`` is defined the derivative along an axis is ``(q[+1] - q[-1]) / 2`` where both
neighbours exist and are defined, ``q[+1] - q[0]`` or ``q[0] - q[-1]`` where one of them does, undefined where neither does; a
raster edge is a neighbour that does not exist.  ``sig_ratio != 1``: ``dx`` from ``q(sigma * ratio, sigma)``, ``dy`` from
``q(sigma, sigma * ratio)``.  ``sigma <= 1``: the Sobel pair / 8, true convolution, reflect; a derivative is defined where the
six samples under its non-zero taps are valid.  Both: NaN everywhere at a pixel whose own sample is missing unless ``fill``;
``dx / res_x``, ``dy / res_y``, ``slope = degrees(arctan(hypot(dx, dy)))``, ``aspect = (180 + degrees(arctan2(dx, dy))) % 360``.

The keyword arguments of :class:`GradientValidReference` build deliberately WRONG variants for
tests/test_gradient_valid_design.py, which shows that :func:`check` notices each.

Bounds (none fitted to a run).  ``dx``, ``dy`` at ``sigma > 1``: ``k * 1e-3 / |res| + 4 * 2**-23 * |ref|`` with ``k = 1`` where
the reference took a central difference (two values each within the project's 1e-3 m of the valid Gaussian, halved) and
``k = 2`` where it took a one-sided one; the second term is the rounding of the float32 difference and of the division.  Sobel:
``8 * 2**-23 * M / |res|`` with ``M`` the raster's largest valid ``|sample|`` - six terms and their roundings; a lost tap moves a
pixel by at least 900 / 8 m.  Slope and aspect: against float64 on the float32 ``dx``, ``dy`` THE CALL RETURNED, at the
tolerances tests/test_gpu_gradient_routes.py derives (8 ulp of [64, 128), 4 ulp of [256, 512), wrapped).  NaN masks: the
reference's exactly at ``min_weight = 0``; for ``min_weight > 0`` a pixel is judged unless ``|D - min_weight| <= 1e-4`` (the
weight bound of gauss_valid_ref) at the pixel or at one of its four neighbours - five weights decide a pixel, gauss_valid_ref
allows 0.5 % for one, so the share left out may be at most 2.5 %: a condition on the reference, asserted."""
import functools

import numpy as np
from scipy import ndimage

import disc_valid_ref as dv
import gauss_valid_ref as gv

# (sigma, sig_ratio): Sobel; radii 5, 13, 48, 121; the two anisotropic forms at sigma 3.25 (radii 26 and 7 across)
CASES = ((0.75, 1), (1.25, 1), (3.25, 1), (12.0, 1), (30.25, 1), (3.25, 2), (3.25, 0.5))
RASTERS = [(k, *s) for k in gv.KINDS for s in gv.SHAPES] + [("clean", dv.GNY, dv.NX)]
MIN_WEIGHTS = (0.25, 0.5, 0.9)
RES_MODES = ("s", "1d", "2d")
VALUE_BOUND = gv.VALUE_BOUND       # 1e-3 m on the valid Gaussian
BAND, BAND_SHARE = gv.WEIGHT_BOUND, 5 * gv.BAND_SHARE
EPS32 = 2.0 ** -23
SLOPE_TOL = 8 * 2.0 ** -17         # degrees: 8 ulp of a float32 in [64, 128)
ASPECT_TOL = 4 * 2.0 ** -15        # degrees: 4 ulp of a float32 in [256, 512), as a wrapped difference
SOBEL_X = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=np.float64) / 8.0  # the reference's kernel (topo.py:679)


def resolutions(mode, shape):
    """Signed grid spacings, every value a float32: a scalar pair, 1-D with a negative y, or one value per pixel."""
    ny, nx = shape
    i, j = np.arange(nx), np.arange(ny)
    if mode == "s":
        return {"x": 25.0, "y": -25.0}
    if mode == "1d":
        return {"x": 20.0 + 0.25 * ((7 * i) % 41), "y": -(18.0 + 0.5 * ((5 * j) % 29))}
    x = 20.0 + 0.25 * ((7 * i[None, :] + 3 * j[:, None]) % 41)
    y = -(18.0 + 0.5 * ((5 * j[:, None] + 11 * i[None, :]) % 29))
    return {"x": x.astype(np.float32), "y": y.astype(np.float32)}


def res_planes(res, shape):
    """``(res_x, res_y)`` as float64 planes of ``shape``."""
    rx, ry = np.asarray(res["x"], dtype=np.float64), np.asarray(res["y"], dtype=np.float64)
    if ry.ndim == 1:
        ry = ry[:, None]
    return np.broadcast_to(rx, shape), np.broadcast_to(ry, shape)


def _neighbours(q, axis):
    """``(q[-1], q[+1])`` along ``axis``, NaN beyond the raster."""
    lo, hi = np.full_like(q, np.nan), np.full_like(q, np.nan)
    src, dst = [slice(None)] * 2, [slice(None)] * 2
    src[axis], dst[axis] = slice(None, -1), slice(1, None)
    lo[tuple(dst)] = q[tuple(src)]
    hi[tuple(src)] = q[tuple(dst)]
    return lo, hi


def valid_difference(centre, plane, axis, nan_one_sided=False, wrong_side=False, no_halving=False):
    """The derivative of ``plane`` (NaN: undefined) along ``axis`` at the pixels where ``centre`` is defined, and the mask of
    the pixels that took a one-sided difference."""
    qm, qp = _neighbours(plane, axis)
    hm, hp, h0 = ~np.isnan(qm), ~np.isnan(qp), ~np.isnan(centre)
    q0 = np.where(np.isnan(plane), 0.0, plane)
    with np.errstate(invalid="ignore"):
        central = (qp - qm) * (1.0 if no_halving else 0.5)
        forward, backward = qp - q0, q0 - qm
    if wrong_side:  # the WRONG side: the difference mirrored about the pixel
        forward, backward = -forward, -backward
    one = h0 & (hm ^ hp)
    d = np.where(hm & hp, central, np.where(hp, forward, backward))
    d = np.where(h0 & (hm | hp), d, np.nan)
    if nan_one_sided:
        d = np.where(one, np.nan, d)
    return d, one


class GradientValidReference:
    """``planes`` = [dx, dy, slope, aspect] (float64, NaN by the rules above) of ``dem`` for one call, ``one_sided`` = the masks
    of the pixels whose dx / dy is a one-sided difference, ``D`` = the weight planes that decide definedness (none for Sobel)."""

    def __init__(self, dem, sigma, res, sig_ratio=1, min_weight=0.0, fill=False, gauss=None, nan_one_sided=False, wrong_side=False,
                 no_halving=False, unfilled_plane=False, centre_only_weight=False, correlation=False, finite_only=False):
        dem = np.asarray(dem, dtype=np.float32)
        shape = dem.shape
        self.sigma, self.sig_ratio, self.min_weight, self.fill = sigma, sig_ratio, min_weight, fill
        self.miss = ~np.isfinite(dem) if finite_only else dv.missing_mask(dem)
        self.res = res_planes(res, shape)
        x = np.where(self.miss, 0.0, dem).astype(np.float64)
        self.largest = float(np.abs(x).max())
        if sigma <= 1:
            self.D = ()
            conv = ndimage.correlate if correlation else ndimage.convolve  # (the WRONG one: the kernel not flipped)
            d, self.one_sided = [], [np.zeros(shape, dtype=bool)] * 2
            for k in (SOBEL_X, SOBEL_X.T):
                lost = conv(self.miss.astype(np.float64), (k != 0).astype(np.float64), mode="reflect") > 0.5
                d.append(np.where(lost, np.nan, conv(x, k, mode="reflect")))
        else:
            perp = sigma * sig_ratio
            sig = [(sigma, sigma)] if sig_ratio == 1 else [(perp, sigma), (sigma, perp)]
            if gauss is None:
                gauss = [gv.GaussValidReference(dem, s, finite_only=finite_only) for s in sig]
            self.D = tuple(g.D for g in gauss)
            d, self.one_sided = [], []
            for axis, g in zip((1, 0), gauss if len(gauss) == 2 else gauss * 2):
                centre = g.out(min_weight, True)
                plane = g.out(0.0, True) if centre_only_weight else g.out(min_weight, not unfilled_plane)
                if unfilled_plane:
                    centre = plane
                dq, one = valid_difference(centre, plane, axis, nan_one_sided, wrong_side, no_halving)
                d.append(dq)
                self.one_sided.append(one)
        if not fill:
            d = [np.where(self.miss, np.nan, v) for v in d]
        dx, dy = d[0] / self.res[0], d[1] / self.res[1]
        self.planes = [dx, dy] + slope_aspect(dx, dy)


def slope_aspect(dx, dy):
    """float64 [slope, aspect] in degrees; NaN where either derivative is."""
    with np.errstate(all="ignore"):
        slope = np.degrees(np.arctan(np.hypot(dx, dy)))
        aspect = (180.0 + np.degrees(np.arctan2(dx, dy))) % 360.0
    bad = np.isnan(dx) | np.isnan(dy)
    return [np.where(bad, np.nan, slope), np.where(bad, np.nan, aspect)]


def gauss_sigmas(sigma, sig_ratio):
    """The (axis 0, axis 1) sigma pairs of the call's Gaussians: the plane of dx, then (``sig_ratio != 1``) the plane of dy."""
    if sigma <= 1:
        return []
    return [(sigma, sigma)] if sig_ratio == 1 else [(sigma * sig_ratio, sigma), (sigma, sigma * sig_ratio)]


@functools.lru_cache(maxsize=None)
def reference(kind, ny, nx, sigma, sig_ratio=1, mode="s", min_weight=0.0, fill=False):
    """The :class:`GradientValidReference` of a raster of ``disc_valid_ref.raster``; the Gaussians are shared through
    ``gauss_valid_ref.reference``."""
    dem = dv.raster(kind, ny, nx)
    gauss = [gv.reference(kind, s, ny, nx) for s in gauss_sigmas(sigma, sig_ratio)] or None
    return GradientValidReference(dem, sigma, resolutions(mode, (ny, nx)), sig_ratio, min_weight, fill, gauss=gauss)


def judged_mask(ref):
    """The pixels whose NaN pattern and values are compared: all at ``min_weight = 0``; else those with no weight within
    ``BAND`` of ``min_weight`` at the pixel or one of its four neighbours, in any of the call's weight planes."""
    shape = ref.planes[0].shape
    near = np.zeros(shape, dtype=bool)
    if ref.min_weight > 0.0:
        cross = ndimage.generate_binary_structure(2, 1)
        for D in ref.D:
            near |= ndimage.binary_dilation(np.abs(D - ref.min_weight) <= BAND, structure=cross)
    return ~near


def left_out_share(ref):
    return 1.0 - float(judged_mask(ref).mean())


def check(got, ref, label="gradient_valid"):
    """``got`` = [dx, dy, slope, aspect] float32 planes (``None``: a plane that was left out) against the reference under the
    module's bounds.  Prints ``FIG ...`` before it asserts."""
    judged = judged_mask(ref)
    left_out = 1.0 - float(judged.mean())
    assert left_out <= BAND_SHARE, f"{label}: {left_out:.4%} of the pixels lie next to a weight within {BAND} of min_weight"
    figs, problems = [], []
    for k, name in enumerate(("dx", "dy")):
        if got[k] is None:
            continue
        assert got[k].dtype == np.float32 and not np.isinf(got[k]).any(), f"{label}: {name} is not float32 or holds an infinity"
        want, res = ref.planes[k], np.abs(ref.res[k])
        nan, want_nan = np.isnan(got[k]), np.isnan(want)
        wrong = judged & (nan != want_nan)
        if wrong.any():
            problems.append(f"{name}: {int((wrong & nan).sum())} NaN too many, {int((wrong & ~nan).sum())} too few, first at "
                            f"{np.argwhere(wrong)[0].tolist()}")
        ok = judged & ~want_nan & ~nan
        if ref.sigma <= 1:
            bound = 8 * EPS32 * ref.largest / res
        else:
            bound = np.where(ref.one_sided[k], 2.0, 1.0) * VALUE_BOUND / res + 4 * EPS32 * np.abs(np.where(want_nan, 0.0, want))
        share = (np.abs(got[k].astype(np.float64) - np.where(want_nan, 0.0, want)) / bound)[ok]
        top = float(share.max()) if share.size else 0.0
        figs.append(f"{name} {top:.3f} of its bound ({int(ok.sum())} pixels, {int((ok & ref.one_sided[k]).sum())} one-sided)")
        if top > 1.0:
            at = np.argwhere(ok)[int(np.argmax(share))].tolist()
            problems.append(f"{name}: error {top:.3f} of the bound at {at}")
    if got[0] is not None and got[1] is not None:
        want = slope_aspect(got[0].astype(np.float64), got[1].astype(np.float64))
        for k, name, tol in ((2, "slope", SLOPE_TOL), (3, "aspect", ASPECT_TOL)):
            if got[k] is None:
                continue
            assert got[k].dtype == np.float32 and not np.isinf(got[k]).any(), f"{label}: {name} is not float32 or holds an infinity"
            if not np.array_equal(np.isnan(got[k]), np.isnan(want[k - 2])):
                problems.append(f"{name}: NaN at {int((np.isnan(got[k]) != np.isnan(want[k - 2])).sum())} pixels where float64 on the "
                                "returned dx, dy has none, or the other way round")
                continue
            ok = ~np.isnan(want[k - 2])
            err = np.abs(got[k].astype(np.float64) - want[k - 2])[ok]
            if k == 3:
                err = np.minimum(err % 360.0, 360.0 - err % 360.0)
                if not np.all((got[3][ok] >= 0) & (got[3][ok] < 360)):
                    problems.append("aspect outside [0, 360)")
            top = float(err.max()) if err.size else 0.0
            figs.append(f"{name} error {top:.3e} of {tol:.3e}")
            if top > tol:
                problems.append(f"{name}: error {top:.6g} degrees")
    print(f"FIG {label}: " + ", ".join(figs) + f", {left_out:.4%} left out")
    assert not problems, f"{label}: " + "; ".join(problems)
