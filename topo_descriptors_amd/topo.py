"""``topo.*`` descriptor functions with the reference's signatures, on MI355X.

Same names, argument meaning, return types and errors as the reference's
``topo_descriptors/topo.py`` (tpi :145, std :273, dem :62, circular_kernel :191, gradient :598,
sobel :658, sx :776 and its geometry helpers :861-925).  The per-pixel arithmetic runs in
hand-written HIP kernels behind the C ABI of ``libtopo_amd.so``; this module only prepares
parameters, hands over C-contiguous float32 buffers and wraps the results.
"""
import ctypes as C
import logging
import os

import numpy as np

from . import _lib, helpers as hlp

logger = logging.getLogger(__name__)


def __getattr__(name):
    """The reference keeps its batch wrappers in this module (``tp.compute_tpi(...)``, topo.py:24-141 and
    on); here they live in ``batch`` (which imports this module) and are resolved on first use."""
    if name.startswith("compute_"):
        from . import batch  # noqa: PLC0415
        if hasattr(batch, name):
            return getattr(batch, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ---- small utilities ------------------------------------------------------------------------
def _unwrap(dem):
    """ndarray view of an ndarray or DataArray-like input (a ``PackedDem`` stays what it is), plus a re-wrapper."""
    if isinstance(dem, (np.ndarray, _lib.PackedDem)):
        return dem, lambda out: out
    if hasattr(dem, "values") and hasattr(dem, "copy"):
        def rewrap(out, src=dem):
            try:
                return src.copy(data=out)
            except TypeError:
                return out
        return _values(dem.values), rewrap
    return np.asarray(dem), lambda out: out


def _values(v):
    return v if isinstance(v, _lib.PackedDem) else np.asarray(v)


def _source(values):
    """``(keep, by-reference Raster, shape)`` of an ndarray or ``PackedDem`` for the host-buffer entry points: supported
    dtypes go to the GPU as stored (``_lib.as_source``); ``keep`` holds the memory the struct points into."""
    keep, raster = _lib.source_of(values)
    return keep, C.byref(raster), keep.shape


def _plane(shape):
    return np.empty(shape, dtype=np.float32)


def _tpi_std(values, size, sigma, packs, want, skipna=False, min_count=1):
    """The planes of ``want`` (tpi, std) with the packings ``packs`` (``None``: float32) from ``topo_amd_tpi_std_packed`` or,
    with ``skipna``, from ``topo_amd_tpi_std_valid_packed`` (over the valid samples of the disc); an unpacked STD plane is
    widened to float64 as :func:`std` does."""
    keep, src, shape = _source(values)
    made = [_lib.result_plane(q, shape) if w else None for q, w in zip(packs, want)]
    refs = [C.byref(m[1]) if m else None for m in made]
    if skipna:
        _lib.check(_lib.lib().topo_amd_tpi_std_valid_packed(src, shape[0], shape[1], int(size), int(min_count), *refs),
                   "topo_amd_tpi_std_valid_packed")
    else:
        _lib.check(_lib.lib().topo_amd_tpi_std_packed(src, shape[0], shape[1], int(size), _sigma_arg(sigma), *refs),
                   "topo_amd_tpi_std_packed")
    out = [_lib.wrap_plane(*m, q) if m else None for m, q in zip(made, packs)]
    if want[1] and packs[1] is None:
        out[1] = out[1].astype(np.float64)
    return out


def _skipna_args(skipna, min_count, sigma, who):
    """The arguments of the valid-sample mode, checked before the library is loaded; returns ``min_count`` as an int."""
    if not skipna:
        if min_count != 1:
            raise ValueError(f"{who}: min_count belongs to skipna=True (without it every tap counts)")
        return 1
    if sigma:
        raise ValueError(f"{who}: skipna=True takes no pre-smoothing (sigma={sigma!r}): smooth over the gaps first, "
                         f"{who}(dem(d, sigma, skipna=True), size, skipna=True)")
    if int(min_count) != min_count or int(min_count) < 1:
        raise ValueError(f"{who}: min_count {min_count!r} (a whole number of valid samples, at least 1)")
    return int(min_count)


def _check_2d(a, who):
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{who}: expected a non-empty 2-D array, got shape {a.shape}")


def _sigma_arg(sigma):
    return float(sigma) if sigma else 0.0


# ---- disc kernel, TPI, STD ---------------------------------------------------------------------
def circular_kernel(size):
    """0/1 float32 disc of diameter ``size``; a full square below 5 (reference topo.py:191)."""
    size = int(size)
    mask = np.empty((size, size), dtype=np.float32)
    if size == 0:
        return mask
    lib = _lib.load()  # pure host geometry: no GPU needed
    _lib.check(lib.topo_amd_disc_mask(size, mask.ctypes.data_as(_lib._f32p)), "topo_amd_disc_mask")
    return mask


def tpi(dem, size, sigma=None, pack=None, skipna=False, min_count=1):
    """Topographic position index: elevation minus the mean of the disc neighbourhood of
    diameter ``size`` pixels, centre excluded; optional Gaussian pre-smoothing ``sigma``
    (reference topo.py:145-181).  float32 in, float32 out; DataArray in, DataArray out.

    With ``sigma`` the pre-smoothing is :func:`dem`'s: see there for how far a non-finite sample reaches.  Without it a
    sample that is not finite (or beyond +-2**24) is MISSING, and exactly the pixels whose disc holds one are NaN - the
    footprint of the disc, whatever the tiles or row blocks; the reference's FFT convolution makes the whole array NaN.

    Accuracy.  On a DEM of whole metres the result is the float64 evaluation of the reference's formula, rounded to
    float32.  Where a disc of 19 pixels or more holds fractional elevations, the neighbourhood sum is taken on ``x``
    in units of 2**-k m (one integer chain instead of two; k = 8 for an ordinary DEM, up to 16 for a raster whose whole
    value range is small): each sample is off by at most 2**-9 m = 1.95 mm, hence so are
    the mean and TPI (about 0.02 mm rms at 67 pixels when the fractional parts are spread evenly) - the order of the
    1.4 - 1.7 mm the reference's own float32 FFT is off by, and far inside 1e-4 of the range.  Smaller discs, and
    :func:`tpi_std`, are exact to 2**-16 m; ``TOPO_AMD_TPI_FRACTION_EXACT=1`` makes this function so as well, at about
    twice the time on such a DEM.

    ``pack``: a :class:`Packing` - the plane is encoded on the GPU and comes back as a :class:`PackedPlane` (never re-wrapped
    into a DataArray), over the link at 1 or 2 bytes a sample; ``None``: float32 as ever.

    ``skipna=True``: the statistics of the samples that exist (numpy's ``nanmean`` reading; sizes 1 ... 101, no ``sigma``).
    A tap counts when it lies inside the raster and its sample is not missing - nothing is padded with zeros, so the outer
    ``size / 2`` pixels are unbiased, and a gap costs its own samples only.  With ``n'`` valid taps (the tap TPI excludes
    left out) and ``s1'`` their sum, ``TPI = x - s1' / n'``; NaN where the pixel itself is missing or
    ``n' < max(1, min_count)``.  The sums are exact integers (fractional parts in units of 2**-16 m), the closing formula is
    float64 rounded to float32 once.  ``min_count`` without ``skipna`` is a ``ValueError``.  Pre-smoothing in this mode is a
    call of its own: ``tpi(dem(d, sigma, skipna=True), size, skipna=True)`` - the Gaussian over the gaps (:func:`dem`), then
    this function on its plane; ``sigma=`` together with ``skipna=True`` stays a ``ValueError``."""
    min_count = _skipna_args(skipna, min_count, sigma, "tpi")
    values, rewrap = _unwrap(dem)
    _check_2d(values, "tpi")
    out = _tpi_std(values, size, sigma, _lib.pack_list(pack, ["tpi"]) + [None], (True, False), skipna, min_count)[0]
    return rewrap(out) if pack is None else out


def std(dem, size, sigma=None, pack=None, skipna=False, min_count=1):
    """Sample standard deviation inside the disc window, with the reference's int32
    truncation of the squared term (reference topo.py:273-307).  Returns float64.  Non-finite samples: as for
    :func:`tpi` (and :func:`dem` when ``sigma`` is given).  ``pack``: as for :func:`tpi`; a packed plane is not widened.

    ``skipna=True`` (see :func:`tpi`): over the ``n`` valid taps of the disc, with ``s1`` their sum and ``s2`` the sum of
    ``trunc(x)**2``, ``STD = sqrt(max(0, (s2 - s1**2 / n) / (n - 1)))`` - the value above wherever every tap is valid; NaN
    where the pixel itself is missing or ``n < max(2, min_count)``.  Pre-smoothed: ``std(dem(d, sigma, skipna=True), size,
    skipna=True)``, as for :func:`tpi`."""
    min_count = _skipna_args(skipna, min_count, sigma, "std")
    values, _ = _unwrap(dem)
    _check_2d(values, "std")
    return _tpi_std(values, size, sigma, [None] + _lib.pack_list(pack, ["std"]), (False, True), skipna, min_count)[1]


def tpi_std(dem, size, sigma=None, pack=None, skipna=False, min_count=1):
    """TPI and STD of the same window in one pass over the DEM (no reference counterpart:
    the reference convolves three times for the pair).  ``pack``: one :class:`Packing` for both planes, or a pair / a dict
    with the keys ``tpi`` and ``std`` (``None``: that plane stays float32, STD widened to float64).  ``skipna``,
    ``min_count``: as for :func:`tpi` and :func:`std`; both planes have the bits of the single calls."""
    min_count = _skipna_args(skipna, min_count, sigma, "tpi_std")
    values, _ = _unwrap(dem)
    _check_2d(values, "tpi_std")
    return tuple(_tpi_std(values, size, sigma, _lib.pack_list(pack, ["tpi", "std"]), (True, True), skipna, min_count))


def tpi_std_multi(dem, sizes, sigmas=None, want_tpi=True, want_std=True, pack=None):
    """TPI and / or STD for several disc sizes from one upload of the DEM (the multi-scale half):
    what the reference's ``compute_tpi`` / ``compute_std`` loops do scale by scale (topo.py:88-141, :216-269).
    Returns ``(tpis, stds)``, lists of planes in the order of ``sizes`` (``None`` for the kind not asked
    for); every plane has the bits of the single call.  ``pack``: one :class:`Packing` for every plane, or a pair / a dict
    with the keys ``tpi`` and ``std`` whose entries are ``None`` (float32), a :class:`Packing` or a sequence with one entry per
    size."""
    values, _ = _unwrap(dem)
    _check_2d(values, "tpi_std_multi")
    keep, src, shape = _source(values)
    sizes = np.ascontiguousarray(np.atleast_1d(sizes), dtype=np.int32)
    n = int(sizes.size)
    if sigmas is None:
        sig = np.zeros(n, dtype=np.float64)
    else:
        sig = np.array([_sigma_arg(v) for v in np.broadcast_to(np.asarray(sigmas, dtype=object), (n,))],
                       dtype=np.float64)
    if pack is None or isinstance(pack, _lib.Packing):
        kinds = [pack, pack]
    else:
        kinds = [pack.get("tpi"), pack.get("std")] if isinstance(pack, dict) else list(pack)
    if len(kinds) != 2:
        raise ValueError("tpi_std_multi: pack is one Packing, or a pair / dict (tpi, std)")
    names = [str(k) for k in range(n)]
    lists, arrays = [], []
    for kind, want in zip(kinds, (want_tpi, want_std)):
        packs = _lib.pack_list(kind, names)
        made = [_lib.result_plane(q, shape) for q in packs] if want else None
        lists.append((packs, made))
        arrays.append(_lib.plane_array([m[1] for m in made]) if want else None)
    _lib.check(_lib.lib().topo_amd_tpi_std_multi_packed(src, shape[0], shape[1], n, sizes.ctypes.data_as(_lib._i32p),
                                                        sig.ctypes.data_as(_lib._f64p), *arrays),
               "topo_amd_tpi_std_multi_packed")
    out = []
    for (packs, made), structs, widen in zip(lists, arrays, (False, True)):
        if made is None:
            out.append(None)
            continue
        planes = [_lib.wrap_plane(m[0], structs[k], q) for k, (m, q) in enumerate(zip(made, packs))]
        out.append([p.astype(np.float64) if widen and q is None else p for p, q in zip(planes, packs)])
    return tuple(out)


# ---- Gaussian, Sobel, gradient ------------------------------------------------------------------
def _valid_gauss_args(skipna, min_weight, fill, return_weight, who):
    """The arguments of the valid-sample Gaussian, checked before the DEM is touched or the library loaded; returns
    ``min_weight`` as a float."""
    if not skipna:
        if min_weight != 0.0 or fill or return_weight:
            raise ValueError(f"{who}: min_weight, fill and return_weight belong to skipna=True (without it the filter is "
                             "ndimage.gaussian_filter's and has no weight)")
        return 0.0
    try:
        mw = float(min_weight)
    except (TypeError, ValueError):
        mw = float("nan")
    if not 0.0 <= mw <= 1.0:  # (false for NaN)
        raise ValueError(f"{who}: min_weight {min_weight!r} (a share of the filter's weight, 0 ... 1)")
    return mw


def dem(dem, sigma, pack=None, skipna=False, min_weight=0.0, fill=False, return_weight=False):
    """Gaussian-smoothed DEM, reflect boundary, 4-sigma truncation (reference topo.py:62-80).
    ``sigma`` may be a scalar or an (axis0, axis1) pair.

    ``skipna=True``: the Gaussian over the samples that exist - a normalised convolution.  With ``m`` 1 where a sample is
    valid (finite and within +-2**24; a ``PackedDem``'s ``fill_value`` arrives as NaN) and the taps ``w`` of the plain filter,
    ``D = sum w m`` and ``N = sum w m x`` over the reflected window, and the result is ``N / D`` where ``D > 0``,
    ``D >= min_weight`` (0 ... 1: the share of the filter's weight that must rest on valid samples) and the pixel itself is
    valid - or, with ``fill=True``, at the missing pixels too: a two-dimensional gap interpolator that leaves NaN only where
    the whole window is empty.  NaN elsewhere.  ``return_weight=True`` returns ``(plane, weight)`` with ``weight = D`` as
    float32.  Radii up to 121 (``sigma <= 30.25``).  The plane goes into :func:`tpi` / :func:`std` as it is:
    ``tpi(dem(d, sigma, skipna=True), size, skipna=True)`` is the pre-smoothed TPI of a DEM with gaps.  Without ``skipna``
    the kernels and bits are the ones described below, and ``min_weight``, ``fill``, ``return_weight`` are a ``ValueError``.

    Non-finite samples: a NaN / inf in the DEM makes non-finite every output whose window contains it, as in
    ``scipy.ndimage.gaussian_filter`` - and exactly those when the smoothing runs on the matrix cores (Gaussian radius
    ``int(4 sigma + 0.5)`` of 4 ... 121, any DEM width from 4 columns): those kernels keep such samples
    (and absurd ones, ``|x| > 1e5``) out of the matrix pipe, mark the tiles whose windows hold one, and a repair pass
    recomputes in float32, over each output's own window, exactly the outputs that see one.  (A raster whose ordinary
    values lie beyond 1e5 - a DEM in millimetres - is recognised by sampling at the first call and smoothed by the
    vector-ALU kernels instead.)  The vector-ALU kernels
    (shorter or much longer filters) pad their taps to chunks of 8 or 16 and spoil up to one chunk more
    towards lower indices.  ``tests/test_gpu_parity.py::test_gaussian_nan_footprint`` pins both.

    ``pack``: as for :func:`tpi`.  The :class:`PackedPlane` it gives is a source like any ``PackedDem``: a smoothed DEM packed
    to uint16 goes back into :func:`tpi` at 2 bytes a sample each way.
    """
    min_weight = _valid_gauss_args(skipna, min_weight, fill, return_weight, "dem")
    values, rewrap = _unwrap(dem)
    _check_2d(values, "dem")
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (2,))
    packing, = _lib.pack_list(pack, ["dem"])
    keep, src, shape = _source(values)
    out, plane = _lib.result_plane(packing, shape)
    weight = _plane(shape) if return_weight else None
    if skipna:
        _lib.check(_lib.lib().topo_amd_gauss_valid_packed(src, shape[0], shape[1], float(sig[0]), float(sig[1]), min_weight,
                                                          int(bool(fill)), C.byref(plane), _lib.ptr(weight)),
                   "topo_amd_gauss_valid_packed")
    else:
        _lib.check(_lib.lib().topo_amd_gauss_packed(src, shape[0], shape[1], float(sig[0]), float(sig[1]), C.byref(plane)),
                   "topo_amd_gauss_packed")
    out = rewrap(out) if packing is None else _lib.wrap_plane(out, plane, packing)  # (a packed plane is not re-wrapped)
    return (out, weight) if return_weight else out


def sobel(dem, skipna=False, fill=False):
    """Sobel derivative pair (dx, dy), kernel / 8, reflect boundary (reference topo.py:658-685).

    ``skipna=True``: over the samples that exist.  ``dx`` is defined where all six samples under its non-zero taps are valid
    (finite and within +-2**24; a reflected tap is valid when the sample it lands on is), ``dy`` by the same rule with its own
    six taps, NaN elsewhere; the centre is a tap of neither, and both are NaN at a pixel whose own sample is missing unless
    ``fill=True``.  On a raster without gaps: the bits of the plain call.  ``fill`` without ``skipna`` is a ``ValueError``."""
    _valid_gauss_args(skipna, 0.0, fill, False, "sobel")
    values, _ = _unwrap(dem)
    _check_2d(values, "sobel")
    keep, src, shape = _source(values)
    dx = _plane(shape)
    dy = _plane(shape)
    lib = _lib.lib()
    if skipna:  # the Sobel route of the valid-sample gradient at a resolution of 1: dx / 1 and dy / 1 are dx and dy
        one = np.ones(1, dtype=np.float64)
        _lib.check(lib.topo_amd_gradient_valid_raw(src, shape[0], shape[1], 0.0, 1.0, 0.0, int(bool(fill)), _lib.RES_SCALAR,
                                                   _lib.ptr(one), _lib.ptr(one), _lib.ptr(dx), _lib.ptr(dy), None, None),
                   "topo_amd_gradient_valid_raw")
        return dx, dy
    _lib.check(lib.topo_amd_sobel_raw(src, shape[0], shape[1], _lib.ptr(dx),
                                      _lib.ptr(dy)), "topo_amd_sobel_raw")
    return dx, dy


def _resolution_args(res_meters, shape):
    """(mode, x array, y array) for the C ABI from the reference's res_meters dict."""
    rx = np.asarray(res_meters["x"], dtype=np.float64)
    ry = np.asarray(res_meters["y"], dtype=np.float64)
    ny, nx = shape
    if rx.ndim == 0 and ry.ndim == 0:
        return _lib.RES_SCALAR, np.ascontiguousarray(rx.reshape(1)), np.ascontiguousarray(ry.reshape(1))
    if rx.ndim <= 1 and ry.ndim <= 1:
        rx = np.ascontiguousarray(np.broadcast_to(rx, (nx,)))
        ry = np.ascontiguousarray(np.broadcast_to(ry, (ny,)))
        return _lib.RES_1D, rx, ry
    # per-pixel resolutions (WGS84 grids): y may still be a column vector
    if ry.ndim == 1:
        ry = ry[:, None]
    rx = np.ascontiguousarray(np.broadcast_to(rx, shape), dtype=np.float32)
    ry = np.ascontiguousarray(np.broadcast_to(ry, shape), dtype=np.float32)
    return _lib.RES_2D, rx, ry


GRADIENT_PLANES = ("dx", "dy", "slope", "aspect")


def gradient(dem, sigma, res_meters, sig_ratio=1, pack=None, skipna=False, min_weight=0.0, fill=False):
    """[dx, dy, slope, aspect] of the Gaussian-smoothed DEM (reference topo.py:598-644).

    ``skipna=True``: over the samples that exist - pass the DEM UNFILLED, its gaps as NaN or as the declared fill value of a
    ``PackedDem``.  ``sigma > 1``: with ``q`` the Gaussian of :func:`dem` ``(skipna=True, fill=True)`` under this call's
    ``min_weight``, the derivative along an axis at a pixel where ``q`` is defined is ``(q[+1] - q[-1]) / 2`` where both
    neighbours exist and are defined, ``q[+1] - q[0]`` or ``q[0] - q[-1]`` where one of them does, NaN where neither does; a
    raster edge is a neighbour that does not exist, so without gaps this is ``np.gradient`` of the Gaussian.  ``q`` is defined
    inside a gap wherever the window reaches a valid sample: a valid pixel on a gap's rim keeps both neighbours.
    ``sig_ratio != 1``: ``dx`` and ``dy`` from two such planes, as below.  ``sigma <= 1``: :func:`sobel` ``(skipna=True)``,
    ``min_weight`` ignored.  All four planes are NaN at a pixel whose own sample is missing unless ``fill=True``; slope and
    aspect are NaN where ``dx`` or ``dy`` is; nothing is infinite.  Radii up to 121.  Without ``skipna`` the kernels and bits
    are the ones described below, and ``min_weight`` and ``fill`` are a ``ValueError``.

    ``sigma <= 1`` uses the Sobel pair; ``sig_ratio != 1`` smooths with ``sigma*sig_ratio``
    perpendicular to each derivative.  Derivatives are divided by the signed grid
    resolution ``res_meters`` (second return of :func:`helpers.scale_to_pixel`); slope in
    degrees; aspect in [0, 360) with north-facing = 0 and east-facing = 90.  Non-finite samples reach as far as in
    :func:`dem` (plus the one pixel of the finite difference).

    ``pack``: one :class:`Packing` for the four planes, a sequence of four, or a dict with the keys ``dx``, ``dy``, ``slope``,
    ``aspect`` (``None`` or a missing key: that plane stays float32); packed planes come back as :class:`PackedPlane`."""
    min_weight = _valid_gauss_args(skipna, min_weight, fill, False, "gradient")
    values, _ = _unwrap(dem)
    _check_2d(values, "gradient")
    packs = _lib.pack_list(pack, GRADIENT_PLANES)
    keep, src, shape = _source(values)
    mode, rx, ry = _resolution_args(res_meters, shape)
    made = [_lib.result_plane(q, shape) for q in packs]
    refs = [C.byref(m[1]) for m in made]
    if skipna:
        _lib.check(_lib.lib().topo_amd_gradient_valid_packed(src, shape[0], shape[1], float(sigma), float(sig_ratio), min_weight,
                                                             int(bool(fill)), mode, _lib.ptr(rx), _lib.ptr(ry), *refs),
                   "topo_amd_gradient_valid_packed")
    else:
        _lib.check(_lib.lib().topo_amd_gradient_packed(src, shape[0], shape[1], float(sigma), float(sig_ratio), mode, _lib.ptr(rx),
                                                       _lib.ptr(ry), *refs), "topo_amd_gradient_packed")
    return [_lib.wrap_plane(*m, q) for m, q in zip(made, packs)]


# ---- Sx ---------------------------------------------------------------------------------------------
def _sx_distance(radius, dx, dy):
    """Distance in metres from the centre of the Sx search window to each of its cells
    (reference topo.py:861-878).  The window has ceil(2*radius_px + 1) cells per side."""
    radius_px = max(radius / np.abs(dy), radius / np.abs(dx))
    side = 2 * radius_px + 1
    mid = np.floor(side / 2)
    steps = np.arange(side) - mid
    return np.hypot((steps * dy)[:, None], (steps * dx)[None, :])


def _sx_source_idx_delta(azimuths, radius, dx, dy):
    """(row, col) index offsets of the ray origins at distance ``radius`` in the directions
    ``azimuths`` (degrees); resolutions are signed (reference topo.py:881-892)."""
    rad = np.deg2rad(np.asarray(azimuths, dtype=np.float64))
    out = np.empty((rad.size, 2), dtype=np.int64)
    out[:, 0] = np.rint(radius / dy * np.cos(rad))
    out[:, 1] = np.rint(radius / dx * np.sin(rad))
    return out


def _sx_bresenhamlines(start, end):
    """Pixels on the straight lines from each ``start`` towards ``end``, both excluded
    (reference topo.py:895-925): unit steps along each ray's dominant axis, half-to-even
    rounding, cut where the L1 distance to ``end`` stops shrinking."""
    start = np.asarray(start)
    end = np.asarray(end)
    span = end - start                                   # (n_rays, 2)
    major = np.abs(span).max(axis=1)                     # steps needed per ray
    n_steps = int(major.max()) if major.size else 0
    safe = np.where(major == 0, 1, major).astype(np.float64)
    direction = np.where((major == 0)[:, None], 0.0, span / safe[:, None])
    t = np.arange(1, n_steps + 1, dtype=np.float64)
    pts = np.rint(start[:, None, :] + direction[:, None, :] * t[None, :, None]).astype(start.dtype)
    l1 = np.abs(pts - end).sum(axis=2)                   # (n_rays, n_steps)
    shrinking = np.ones_like(l1, dtype=bool)
    shrinking[:, 1:] = l1[:, 1:] <= l1[:, :-1]
    keep = shrinking & (l1 != 0)
    return pts[keep]


def _sx_scan(dem, reach, rows, cols, metres, height, pack=None):
    """Kernel K6 on a host array: for every pixel the largest elevation angle (degrees) towards the ray pixels
    ``(rows[k], cols[k])`` (offsets from the pixel) at ``metres[k]`` horizontal distance, seen from ``height``
    above the pixel.  NaN distances are skipped; a frame of ``reach`` pixels stays 0.  ``pack``: a :class:`Packing`; the
    planes made on the host (nothing but frame, no usable ray pixel) are packed there."""
    dem = _values(dem)
    _check_2d(dem, "_sx_rolling")
    packing, = _lib.pack_list(pack, ["sx"])
    host = _sx_host_plane(dem.shape, reach, metres)
    if host is not None:
        return _sx_result(host, None, packing, dem.dtype)
    metres = np.ascontiguousarray(metres, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    keep, src, (ny, nx) = _source(dem)
    out, plane = _lib.result_plane(packing, (ny, nx))
    _lib.check(_lib.lib().topo_amd_sx_packed(src, ny, nx, rows.ctypes.data_as(_lib._i32p), cols.ctypes.data_as(_lib._i32p),
                                             metres.ctypes.data_as(_lib._f64p), int(metres.size), int(reach), float(height),
                                             C.byref(plane)), "topo_amd_sx_packed")
    return _sx_result(out, plane, packing, dem.dtype)


def _sx_host_plane(shape, reach, metres):
    """The Sx plane of a sector the device has no work for, made on the host (``None``: it has): zeros where the DEM is nothing
    but the frame of ``reach`` pixels; NaN inside the frame where there is no usable ray pixel (nanmax over an empty / all-NaN
    set, like numpy)."""
    ny, nx = shape
    framed = ny <= 2 * reach or nx <= 2 * reach
    if not framed and np.size(metres) and not np.all(np.isnan(metres)):
        return None
    out = np.zeros(shape, dtype=np.float32)
    if not framed:
        out[reach : ny - reach, reach : nx - reach] = np.nan
    return out


def _sx_result(array, plane, packing, dtype):
    """What an Sx call returns for one plane: unpacked in the DEM's ``dtype``, else a ``PackedPlane`` - of the library's
    ``plane`` struct, or (``None``: a plane made on the host) packed there."""
    if packing is None:
        return array.astype(dtype, copy=False)
    return _lib.encode_host(array, packing) if plane is None else _lib.wrap_plane(array, plane, packing)


def _sx_rolling(dem, distance, blines, height):
    """The reference's private entry (topo.py:928-953): ``distance`` is the square table of distances around
    the pixel, ``blines`` the (row, column) cells of that table the rays cross."""
    reach = int(distance.shape[0] / 2)
    cells = np.asarray(blines, dtype=np.int64).reshape(-1, 2)
    return _sx_scan(dem, reach, cells[:, 0] - reach, cells[:, 1] - reach, distance[cells[:, 0], cells[:, 1]], height)


def _sx_sector(azimuth, radius, spacing_x, spacing_y, azimuth_arc=10.0, azimuth_steps=15, radius_min=0.0):
    """The ray pixels of one sector as ``(reach, rows, cols, metres)``: offsets from the target pixel and their
    distances (NaN where closer than ``radius_min``), built from the reference's three geometry helpers so that
    the set is the reference's (topo.py:825-853)."""
    n_rays = 1 if azimuth_arc == 0 else azimuth_steps
    ray_azimuths = np.linspace(azimuth - azimuth_arc / 2, azimuth + azimuth_arc / 2, n_rays)
    table = _sx_distance(radius, spacing_x, spacing_y)
    table[table < radius_min] = np.nan
    middle = np.floor(np.array(table.shape) / 2)
    far_ends = (middle + _sx_source_idx_delta(ray_azimuths, radius, spacing_x, spacing_y)).astype(int)
    cells = np.asarray(_sx_bresenhamlines(far_ends, middle), dtype=np.int64).reshape(-1, 2)
    reach = int(table.shape[0] / 2)
    return reach, cells[:, 0] - reach, cells[:, 1] - reach, table[cells[:, 0], cells[:, 1]]


def sx(dem_ds, azimuth, radius, height=10.0, azimuth_arc=10.0, azimuth_steps=15, radius_min=0.0, pack=None):
    """Sx (Winstral et al.): maximum slope towards the terrain within ``radius`` metres in a
    sector of ``azimuth_arc`` degrees around ``azimuth`` (reference topo.py:776-858).

    ``dem_ds`` must be a Dataset (TypeError otherwise, like the reference); the mean signed
    grid spacing is used; pixels closer than ``radius_min`` are ignored; ``height`` is the
    instrument height added to the target pixel.  ``pack``: as for :func:`tpi`."""
    if not hlp._looks_like_dataset(dem_ds):
        raise TypeError("Argument 'dem_ds' must be a xr.Dataset.")
    spacing = hlp.scale_to_pixel(radius, dem_ds)[1]
    sector = _sx_sector(azimuth, radius, spacing["x"].mean(), spacing["y"].mean(), azimuth_arc, azimuth_steps,
                        radius_min)
    return _sx_scan(hlp.get_da(dem_ds).values, *sector, height, pack=pack)


def sx_multi(dem_ds, azimuths, radius, height=10.0, azimuth_arc=10.0, azimuth_steps=15, radius_min=0.0, pack=None):
    """``sx`` for a sequence of azimuths in one pass over the DEM: ``[sx(dem_ds, a, radius, ...) for a
    in azimuths]`` with the same bits.  The reference scans one azimuth per call (topo.py:776-858) and
    its users loop; here the DEM is uploaded once and ray pixels shared by neighbouring sectors are
    scanned once.  Give the azimuths in angular order for the sharing to apply.  ``pack``: one
    :class:`Packing` for every plane or a sequence with one entry per azimuth (``None``: float32)."""
    if not hlp._looks_like_dataset(dem_ds):
        raise TypeError("Argument 'dem_ds' must be a xr.Dataset.")
    azimuths = [float(a) for a in np.atleast_1d(azimuths)]
    if len(azimuths) == 0:
        return []
    from . import device  # noqa: PLC0415
    _, res_meters = hlp.scale_to_pixel(radius, dem_ds)
    dx = res_meters["x"].mean()
    dy = res_meters["y"].mean()
    sectors = [device.sx_offsets(a, radius, dx, dy, azimuth_arc, azimuth_steps, radius_min) for a in azimuths]
    dem = _values(hlp.get_da(dem_ds).values)
    _check_2d(dem, "sx_multi")
    keep, src, (ny, nx) = _source(dem)
    packs = _lib.pack_list(pack, [str(a) for a in azimuths])
    # the sectors the device has work for (the others are made on the host, as in _sx_scan) go into one library call
    outs = [_sx_host_plane((ny, nx), window, dist) for window, _, _, dist in sectors]
    structs = [None] * len(sectors)
    todo = [k for k, o in enumerate(outs) if o is None]
    for k in todo:
        outs[k], structs[k] = _lib.result_plane(packs[k], (ny, nx))
    if todo:
        first, dj, di, dist, window = device.pack_sectors([sectors[k] for k in todo])
        planes = _lib.plane_array([structs[k] for k in todo])
        _lib.check(_lib.lib().topo_amd_sx_multi_packed(
            src, ny, nx, len(todo), first.ctypes.data_as(_lib._i32p), dj.ctypes.data_as(_lib._i32p),
            di.ctypes.data_as(_lib._i32p), dist.ctypes.data_as(_lib._f64p), window.ctypes.data_as(_lib._i32p),
            float(height), planes), "topo_amd_sx_multi_packed")
        for n, k in enumerate(todo):
            structs[k] = planes[n]  # (with the library's counters)
    return [_sx_result(o, s, q, dem.dtype) for o, s, q in zip(outs, structs, packs)]


# ---- valley / ridge index ---------------------------------------------------------------------
VALLEY_MAX_PLANES = 16  # flat fractions per call (TOPO_AMD_VALLEY_MAX_PLANES, include/topo_amd.h)


def _valley_kernels(size, flat_list):
    """One normalised V / U profile per flat fraction (reference topo.py:456-492): distance to the
    centre row, repeated along the columns; a fraction ``f`` flattens the band of half-width
    ``int(floor(floor(size * f / 2) + 0.5))`` to the value on its edge.  Like the reference, every
    plane is brought to mean 0 / std 1 again after each fraction is applied, so later planes are
    flattened on normalised values (this order decides the float32 result).  Odd sizes only."""
    size = int(size)
    middle = size // 2
    if 2 * middle + 1 != size:
        # the reference fails here too: its profile has 2 * (size // 2) + 1 rows and cannot be
        # broadcast to (size, size) (topo.py:477-482); scale_to_pixel only ever yields odd sizes
        raise ValueError(f"valley / ridge kernels need an odd size, got {size}: operands could not be broadcast "
                         f"together with remapped shapes ({2 * middle + 1},{size}) -> ({size},{size})")
    rows = np.abs(np.arange(-middle, middle + 1)).astype(np.float32)
    kernels = np.tile(rows[None, :, None], (len(flat_list), 1, size))
    for ind, flat in enumerate(flat_list):
        half = int(np.floor(np.floor(size * flat / 2) + 0.5))
        kernels[ind, middle - half:middle + half + 1, :] = kernels[ind, middle - half, 0]
        kernels = (kernels - kernels.mean(axis=(1, 2), keepdims=True)) / kernels.std(axis=(1, 2), keepdims=True)
    return kernels


def _ridge_kernels(size, flat_list):
    """reference topo.py:495-512"""
    return _valley_kernels(size, flat_list) * -1


def _rotate_kernels(kernel, angle):
    """The kernel stack turned by ``angle`` degrees in its (row, column) plane with scipy's
    quadratic-spline ``ndimage.rotate`` on an enlarged canvas; canvas cells outside the turned
    square (left at the fill value -9999) are excluded from the re-normalisation and end up 0
    (reference topo.py:515-525).  Host-side parameter preparation, like the Sx ray geometry."""
    from numpy import ma
    from scipy import ndimage

    turned = ndimage.rotate(kernel, angle, axes=(1, 2), reshape=True, order=2, mode="constant", cval=-9999)
    turned = ma.masked_array(turned, mask=turned == -9999)
    turned = (turned - turned.mean(axis=(1, 2), keepdims=True)) / turned.std(axis=(1, 2), keepdims=True)
    return ma.MaskedArray.filled(turned, 0).astype(np.float32)


def _valley_ridge_tables(kernels, angles):
    """Per angle, what the reference's 3-D ``signal.convolve(dem3, kernels_rot, mode="same")``
    (topo.py:436) applies to the DEM in each output plane, laid out for the C ABI.

    The DEM is broadcast to one identical plane per kernel plane, so along that axis the "same"
    convolution just adds the kernel planes that overlap: output plane ``i`` of ``L`` sees the sum of
    ``K[b]`` with ``0 <= i - b + (L - 1) // 2 < L`` (three planes: K0+K1, K0+K1+K2, K1+K2).  The
    sums are flipped in both axes (a convolution becomes a correlation) and interleaved as
    ``4 * ceil(n / 4)`` floats per tap: group ``g`` holds planes ``4g .. 4g+3``, unused slots are 0
    (four floats for up to four planes).  Returns (taps float32, ksize int32, angles float32)."""
    n = kernels.shape[0]
    if not 1 <= n <= VALLEY_MAX_PLANES:
        raise ValueError(f"valley_ridge: {n} flat fractions; 1 to {VALLEY_MAX_PLANES} are supported")
    centre = (n - 1) // 2
    width = 4 * ((n + 3) // 4)

    def one_angle(angle):
        turned = _rotate_kernels(kernels, angle).astype(np.float64)
        side = turned.shape[1]
        block = np.zeros((side, side, width), dtype=np.float32)
        for i in range(n):
            total = sum(turned[b] for b in range(n) if 0 <= i - b + centre < n)
            block[:, :, i] = total[::-1, ::-1]
        return block.reshape(-1)

    # the angles are independent and scipy / numpy release the GIL in the rotation and the
    # re-normalisation: for large kernels (seconds per call) they are spread over host threads
    workers = min(32, os.cpu_count() or 1, len(angles))
    if kernels.shape[1] >= 65 and workers > 1:
        from concurrent.futures import ThreadPoolExecutor  # noqa: PLC0415
        with ThreadPoolExecutor(workers) as pool:
            taps = list(pool.map(one_angle, angles))
    else:
        taps = [one_angle(angle) for angle in angles]
    ksize = [int(round((t.size // width) ** 0.5)) for t in taps]
    return (np.ascontiguousarray(np.concatenate(taps), dtype=np.float32), np.asarray(ksize, dtype=np.int32),
            np.ascontiguousarray(angles, dtype=np.float32))


def valley_ridge(dem, size, mode, flat_list=[0, 0.15, 0.3], sigma=None, pack=None):  # noqa: B006 (the reference's default)
    """Valley or ridge index: for 180 directions, the response of the standardised DEM to V- and
    U-shaped kernels of side ``size`` turned to that direction; returns ``[norm, direction]``, the
    largest response clipped at 0 and the direction (degrees, 0 = W-E, 90 = S-N) it came from
    (reference topo.py:389-447).  The 180 x ``len(flat_list)`` convolutions run in one pass over
    the DEM on the GPU.

    The reference standardises with numpy's own float32 mean / std of the whole (smoothed) array (topo.py:427).  Where that
    array is float32 - a C-contiguous float32 ndarray, a ``PackedDem``, anything with ``sigma`` - the whole call is one library
    call: the DEM goes up once, is smoothed there, and the two moments are formed on the GPU in numpy's summation order, bit
    for bit (``topo_amd_valley_ridge_packed``).  An ndarray of another dtype without ``sigma`` is reduced by numpy in float64:
    its moments stay numpy's, on the host (as do all under ``helpers.moments_chunk``'s conditions).

    ``pack``: one :class:`Packing` for both planes, a pair, or a dict with the keys ``norm`` and ``direction`` (``None`` or a
    missing key: float32); packed planes come back as :class:`PackedPlane`.  The direction plane holds whole degrees
    0 ... 179: ``Packing(np.uint8, fill_value=255)`` stores it exactly."""
    if mode not in ("valley", "ridge"):
        raise ValueError(f"Unknown mode {mode!r}")
    values, _ = _unwrap(dem)
    _check_2d(values, "valley_ridge")
    packs = _lib.pack_list(pack, ["norm", "direction"])
    kernels = _ridge_kernels(size, flat_list) if mode == "ridge" else _valley_kernels(size, flat_list)
    taps, ksize, angles = _valley_ridge_tables(kernels, np.arange(0, 180, dtype=np.float32))
    tables = (taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(_lib._i32p), angles.ctypes.data_as(_lib._vp), ksize.size,
              kernels.shape[0])
    float32_field = bool(sigma) or isinstance(values, _lib.PackedDem) or (values.dtype == np.float32 and values.flags.c_contiguous)
    chunk = hlp.moments_chunk() if float32_field else None
    if chunk is not None:
        keep, src, shape = _source(values)
        made = [_lib.result_plane(q, shape) for q in packs]
        _lib.check(_lib.lib().topo_amd_valley_ridge_packed(src, shape[0], shape[1], *tables, _sigma_arg(sigma), chunk,
                                                           *[C.byref(m[1]) for m in made], None), "topo_amd_valley_ridge_packed")
        return [_lib.wrap_plane(*m, q) for m, q in zip(made, packs)]
    field = globals()["dem"](values, sigma) if sigma else values
    keep, src, shape = _source(field)
    # numpy's own mean / std on the host; a PackedDem is the float32 array it decodes to
    host = field.decode() if isinstance(field, _lib.PackedDem) else field
    mean, stdev = float(host.mean()), float(host.std())
    norm = _plane(shape)
    direction = _plane(shape)
    _lib.check(_lib.lib().topo_amd_valley_ridge_raw(src, shape[0], shape[1], *tables, mean, stdev, norm.ctypes.data_as(_lib._vp),
                                                    direction.ctypes.data_as(_lib._vp)), "topo_amd_valley_ridge_raw")
    return [p if q is None else _lib.encode_host(p, q) for p, q in zip((norm, direction), packs)]
