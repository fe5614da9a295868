"""Host-side parameter preparation: metres -> pixels, sigmas, DEM validation.

Mirrors the call signatures of the reference's ``topo_descriptors/helpers.py`` for the part of
it the descriptor hot path uses (scale_to_pixel :68, round_up_to_odd :108, get_sigmas :114,
check_dem :171, get_da :191).  No per-pixel arithmetic happens here.  xarray is optional:
anything that quacks like a Dataset (``ds["x"].values``, ``ds.attrs["crs"]``, iterable
variable names, ``ds[name].dims``) is accepted, because the GPU box may not have xarray.
"""
import datetime
import functools
import logging
import os
import time

import numpy as np

from . import CFG

logger = logging.getLogger(__name__)

try:  # pragma: no cover - xarray is absent from the build image
    import xarray as _xr
except Exception:  # noqa: BLE001
    _xr = None


def _looks_like_dataset(obj):
    if _xr is not None and isinstance(obj, _xr.Dataset):
        return True
    if isinstance(obj, np.ndarray):
        return False
    # a DataArray has attrs, __getitem__ and __iter__ too; the reference raises for it (topo.py:825-826,
    # helpers.py:179-180: isinstance(dem, xr.Dataset)).  It carries ``dims`` itself and has no data variables.
    if hasattr(obj, "dims") and not hasattr(obj, "data_vars"):
        return False
    return all(hasattr(obj, a) for a in ("attrs", "__getitem__", "__iter__"))


def check_dem(dem):
    """Validate the DEM data model (reference helpers.py:171-188): Dataset, dims ('y','x'),
    a ``crs`` attribute naming an EPSG code."""
    if not _looks_like_dataset(dem):
        raise ValueError("dem must be a xr.Dataset")
    first = list(dem)[0]
    if tuple(dem[first].dims) != ("y", "x"):
        raise ValueError("dem dimensions must be ('y', 'x')")
    if "crs" not in dem.attrs:
        raise KeyError("missing 'crs' (case sensitive) attribute in dem")
    if "epsg:" not in dem.attrs["crs"].lower():
        raise ValueError("missing 'epsg:' (case insensitive) key in the 'crs' attribute")


def get_da(dem_ds):
    """First data variable of the Dataset, whatever its name (reference helpers.py:191-196)."""
    return dem_ds[list(dem_ds)[0]]


def dem_shape(dem_ds):
    """``(ny, nx)`` of the Dataset's first data variable (an ndarray, or a ``PackedDem``)."""
    values = get_da(dem_ds).values
    ny, nx = values.shape if hasattr(values, "shape") else np.shape(values)
    return int(ny), int(nx)


def round_up_to_odd(f):
    """Nearest odd integer as int64 (reference helpers.py:108-111)."""
    f = np.asarray(f, dtype=np.float64)
    return (np.round((f - 1.0) / 2.0) * 2.0 + 1.0).astype(np.int64)


# ---- WGS84 -> UTM without the `utm` wheel ---------------------------------------------------------------------------------------
# The reference reprojects a WGS84 grid with `utm.from_latlon(lat, lon)` (helpers.py:91-97; PyPI package `utm`, version not
# pinned by the reference, absent from this image).  What follows restates that function's published algorithm (Turbo87/utm,
# conversion.py: the Transverse Mercator series of USGS Professional Paper 1395 / Snyder on the WGS84 ellipsoid, scale 0.9996) for
# array input, including its choice of ONE zone for the whole array from the array's FIRST element (with the Norway / Svalbard
# exceptions) - that choice is what makes np.gradient of the eastings meaningful across a grid that straddles a zone boundary.
# Pinned by known answers of the package's own README and test-suite (tests/test_host_api.py); when the package is installed
# it is used instead.
_UTM_K0 = 0.9996
_UTM_E = 0.00669438
_UTM_E2 = _UTM_E * _UTM_E
_UTM_E3 = _UTM_E2 * _UTM_E
_UTM_E_P2 = _UTM_E / (1.0 - _UTM_E)
_UTM_M1 = 1 - _UTM_E / 4 - 3 * _UTM_E2 / 64 - 5 * _UTM_E3 / 256
_UTM_M2 = 3 * _UTM_E / 8 + 3 * _UTM_E2 / 32 + 45 * _UTM_E3 / 1024
_UTM_M3 = 15 * _UTM_E2 / 256 + 45 * _UTM_E3 / 1024
_UTM_M4 = 35 * _UTM_E3 / 3072
_UTM_R = 6378137.0


def _utm_zone_number(latitude, longitude):
    """Zone of the array's first element (the package's rule for numpy input), Norway and Svalbard as the package has them."""
    lat = float(np.asarray(latitude).flat[0])
    lon = float(np.asarray(longitude).flat[0])
    if 56 <= lat < 64 and 3 <= lon < 12:
        return 32
    if 72 <= lat <= 84 and lon >= 0:
        if lon < 9:
            return 31
        if lon < 21:
            return 33
        if lon < 33:
            return 35
        if lon < 42:
            return 37
    return int((lon + 180) / 6) + 1


def _utm_from_latlon(latitude, longitude):
    """``(easting, northing, zone_number)`` of WGS84 latitudes / longitudes in degrees (arrays of one shape), all in the zone of
    the first element.  Raises like the package outside 80 S ... 84 N / 180 W ... 180 E and for latitudes of mixed sign."""
    lat = np.asarray(latitude, dtype=np.float64)
    lon = np.asarray(longitude, dtype=np.float64)
    if lat.size == 0:
        raise ValueError("from_latlon: empty input")
    if not (np.min(lat) >= -80.0 and np.max(lat) <= 84.0):
        raise ValueError("latitude out of range (must be between 80 deg S and 84 deg N)")
    if not (np.min(lon) >= -180.0 and np.max(lon) <= 180.0):
        raise ValueError("longitude out of range (must be between 180 deg W and 180 deg E)")
    if np.min(lat) < 0 and np.max(lat) >= 0:
        raise ValueError("latitudes must all have the same sign")
    lat_rad = np.radians(lat)
    lat_sin, lat_cos = np.sin(lat_rad), np.cos(lat_rad)
    lat_tan = lat_sin / lat_cos
    lat_tan2 = lat_tan * lat_tan
    lat_tan4 = lat_tan2 * lat_tan2
    zone = _utm_zone_number(lat, lon)
    central_lon_rad = np.radians((zone - 1) * 6 - 180 + 3)
    n = _UTM_R / np.sqrt(1 - _UTM_E * lat_sin ** 2)
    c = _UTM_E_P2 * lat_cos ** 2
    d_lon = (np.radians(lon) - central_lon_rad + np.pi) % (2 * np.pi) - np.pi  # the package's mod_angle
    a = lat_cos * d_lon
    a2 = a * a
    a3 = a2 * a
    a4 = a3 * a
    a5 = a4 * a
    a6 = a5 * a
    m = _UTM_R * (_UTM_M1 * lat_rad - _UTM_M2 * np.sin(2 * lat_rad) + _UTM_M3 * np.sin(4 * lat_rad) - _UTM_M4 * np.sin(6 * lat_rad))
    easting = _UTM_K0 * n * (a + a3 / 6 * (1 - lat_tan2 + c) +
                             a5 / 120 * (5 - 18 * lat_tan2 + lat_tan4 + 72 * c - 58 * _UTM_E_P2)) + 500000
    northing = _UTM_K0 * (m + n * lat_tan * (a2 / 2 + a4 / 24 * (5 - lat_tan2 + 9 * c + 4 * c ** 2) +
                                             a6 / 720 * (61 - 58 * lat_tan2 + lat_tan4 + 600 * c - 330 * _UTM_E_P2)))
    if np.max(lat) < 0:
        northing = northing + 10000000
    return easting, northing, zone


def _wgs84_to_utm(x_coords, y_coords):
    lon, lat = np.meshgrid(x_coords, y_coords)
    try:
        import utm  # noqa: PLC0415
        east, north, _, _ = utm.from_latlon(lat, lon)
    except ImportError:
        east, north, _ = _utm_from_latlon(lat, lon)
    return east.astype(np.float32), north.astype(np.float32)


def scale_to_pixel(scales, dem_ds):
    """Scales in metres -> odd pixel diameters, plus the signed per-node grid resolution
    ``{"x": ..., "y": ...}`` in metres (reference helpers.py:68-105)."""
    check_dem(dem_ds)
    x_coords = np.asarray(dem_ds["x"].values)
    y_coords = np.asarray(dem_ds["y"].values)
    if "epsg:4326" in dem_ds.attrs["crs"].lower():
        logger.debug("Reprojecting coordinates from WGS84 to UTM to obtain units of meters")
        x_coords, y_coords = _wgs84_to_utm(x_coords, y_coords)
    x_res = np.gradient(x_coords, axis=x_coords.ndim - 1)
    y_res = np.gradient(y_coords, axis=0)
    mean_res = np.mean(np.abs([x_res.mean(), y_res.mean()]))
    logger.debug("Estimated resolution: %.0f meters.", mean_res)
    return round_up_to_odd(np.array(scales) / mean_res), {"x": x_res, "y": y_res}


def get_sigmas(smth_factors, scales_pxl):
    """Gaussian sigmas in pixels for smoothing factors; falsy factor -> None
    (reference helpers.py:114-134)."""
    factors = np.array([f if f else np.nan for f in smth_factors], dtype=np.float64)
    sigmas = factors * np.asarray(scales_pxl) / CFG.scale_std
    return [None if np.isnan(s) else s for s in sigmas]


# ---- the crop of the reference's writer (helpers.py:34-65: ``.sel(crop)``), restated on plain coordinates ------------------------
def _axis_window(coords, bounds, key):
    """``(first, count)`` of the labels ``Dataset.sel({key: bounds})`` keeps: ``pandas.Index.slice_indexer`` on a strictly
    monotonic index - label-based, both ends inclusive, a bound need not be a label."""
    n = coords.size
    if bounds is None:
        return 0, n
    if not isinstance(bounds, slice):
        raise NotImplementedError(f"crop[{key!r}] = {bounds!r}: only slice(start, stop) selections are supported")
    if bounds.step is not None:
        raise NotImplementedError(f"crop[{key!r}] = {bounds!r}: a slice with a step is not supported")
    if n and coords[0] > coords[-1]:  # decreasing: labels <= start and >= stop
        asc = coords[::-1]
        first = 0 if bounds.start is None else n - int(np.searchsorted(asc, bounds.start, side="right"))
        last = n if bounds.stop is None else n - int(np.searchsorted(asc, bounds.stop, side="left"))
    else:  # increasing: labels >= start and <= stop
        first = 0 if bounds.start is None else int(np.searchsorted(coords, bounds.start, side="left"))
        last = n if bounds.stop is None else int(np.searchsorted(coords, bounds.stop, side="right"))
    return first, max(last - first, 0)


def crop_window(dem_ds, crop):
    """``(row0, rows, col0, cols)``: the part of the DEM that ``dem_ds.sel(crop)`` selects (the reference's writer,
    helpers.py:34-65), from the 1-D ``y`` and ``x`` coordinates alone - no xarray needed.  ``crop``: ``None`` or a dict with
    the keys ``"x"`` / ``"y"`` (a missing key: the whole axis) and ``slice(start, stop)`` values, label-based with both ends
    inclusive and ``None`` for an open end, as ``pandas.Index.slice_indexer`` selects: on an increasing coordinate the labels
    ``>= start`` and ``<= stop``, on a decreasing one the labels ``<= start`` and ``>= stop``.  A slice in the wrong direction
    for its coordinate (``slice(-160000, 480000)`` on a north-to-south ``y``) selects nothing, as in the reference: ``rows`` or
    ``cols`` is 0.  ``KeyError`` for another key, ``NotImplementedError`` for a value that is no slice or has a step,
    ``ValueError`` for a coordinate that is not strictly monotonic or does not have the array's length."""
    check_dem(dem_ds)
    ny, nx = dem_shape(dem_ds)
    crop = {} if crop is None else dict(crop)
    for key in crop:
        if key not in ("x", "y"):
            raise KeyError(f"crop: {key!r} is not a dimension of the DEM ('x' or 'y')")
    window = []
    for key, n in (("y", ny), ("x", nx)):
        coords = np.asarray(dem_ds[key].values)
        if coords.ndim != 1 or coords.size != n:
            raise ValueError(f"crop: {key} has {coords.shape} coordinates for {n} samples")
        step = np.diff(coords)
        if not ((step > 0).all() or (step < 0).all()):
            raise ValueError(f"crop: the {key} coordinate must be strictly monotonic (increasing or decreasing)")
        window.append(_axis_window(coords, crop.get(key), key))
    return window[0] + window[1]


# ---- the steps either side of the path: thin, and xarray's where the reference uses it
def _need_xarray(what):
    if _xr is None:
        raise ImportError(f"{what} reads / writes netCDF through xarray, which is not installed here; "
                          "the descriptor functions themselves accept any Dataset-like object")
    return _xr


def get_dem_netcdf(path_dem):
    """The DEM of a netCDF file as a float32 Dataset, elevations at or below ``CFG.min_elevation``
    masked as NaN (reference helpers.py:17-31).  Needs xarray."""
    xr = _need_xarray("get_dem_netcdf")
    dem_ds = xr.open_dataset(path_dem).astype(np.float32).squeeze(drop=True)
    return dem_ds.where(dem_ds > CFG.min_elevation)


def to_netcdf(array, dem_ds, name, crop=None, outdir=".", units=None):
    """``array`` saved as ``topo_<NAME>.nc`` with the coordinates and attributes of ``dem_ds``
    (reference helpers.py:34-65).  Needs xarray; ``batch.write_output`` is the same writer and falls
    back to ``.npy`` without it."""
    _need_xarray("to_netcdf")
    from . import batch  # noqa: PLC0415  (batch imports this module)
    return batch.write_output(array, dem_ds, name, crop=crop, outdir=outdir, units=units)


def fill_na_array(values, x_coords=None):
    """NaNs of a 2-D array replaced row by row with the nearest valid sample along x, the edge value
    beyond the first / last valid sample: what ``interpolate_na(dim="x", method="nearest",
    fill_value="extrapolate")`` does in the reference's ``fill_na`` (helpers.py:137-154), through the
    same ``scipy.interpolate.interp1d`` xarray uses (a sample half way between two valid ones takes the
    left one).  Rows with fewer than two valid samples are left alone.  xarray is absent from the image, so
    this is pinned by hand-derived known answers (tests/test_host_api.py::test_fill_na_array_known_answers),
    not by a run of the reference."""
    from scipy.interpolate import interp1d  # noqa: PLC0415

    out = np.array(values, copy=True)
    x = np.arange(out.shape[1], dtype=np.float64) if x_coords is None else np.asarray(x_coords, dtype=np.float64)
    for row in out:
        bad = np.isnan(row)
        if bad.any() and (~bad).sum() >= 2:
            fill = interp1d(x[~bad], row[~bad], kind="nearest", fill_value="extrapolate", assume_sorted=False)
            row[bad] = fill(x[bad])
    return out


def _fill_coords(x_coords, nx):
    """``x_coords`` as the C ABI takes them (float64, contiguous; None stays None), refused unless finite, strictly
    monotonic and one per column - before any library call."""
    if x_coords is None:
        return None
    x = np.ascontiguousarray(np.asarray(x_coords, dtype=np.float64).ravel())
    if x.size != nx:
        raise ValueError(f"fill_na: {x.size} x_coords for {nx} columns")
    if not np.isfinite(x).all():
        raise ValueError("fill_na: x_coords must be finite")
    step = np.diff(x)
    if not ((step > 0).all() or (step < 0).all()):
        raise ValueError("fill_na: x_coords must be strictly monotonic (increasing or decreasing)")
    return x


def fill_na_gpu(values, x_coords=None, min_elevation=None):
    """``(missing, filled)``: what the reference's ``fill_na`` returns as ``(ind_nans, filled)`` (helpers.py:137-154),
    computed on the GPU (``topo_amd_fill_na_raw``) with the bits of :func:`fill_na_array`.  A sample is missing when it is
    NaN or, with ``min_elevation``, at or below it (float32 comparison: the masking of ``get_dem_netcdf``, helpers.py:30-31);
    each is replaced by the nearest valid sample along x (``x_coords``, or the column index), rows with fewer than two
    valid samples are left alone.  ``missing`` is a boolean array: ``np.nonzero(missing)`` is the reference's ``ind_nans``,
    and the mask itself works as ``ind_nans`` in ``batch.compute_*``.  A DataArray-like input is re-wrapped."""
    from . import _lib, topo  # noqa: PLC0415  (topo imports this module)

    a, rewrap = topo._unwrap(values)
    topo._check_2d(a, "fill_na_gpu")
    x = _fill_coords(x_coords, a.shape[1])
    keep, src, shape = topo._source(a)
    out = np.empty(shape, dtype=np.float32)
    missing = np.empty(shape, dtype=np.uint8)
    m = np.nan if min_elevation is None else float(min_elevation)
    _lib.check(_lib.lib().topo_amd_fill_na_raw(src, shape[0], shape[1],
                                               None if x is None else x.ctypes.data_as(_lib._f64p), m, _lib.ptr(out),
                                               _lib.ptr(missing)), "topo_amd_fill_na_raw")
    return missing.view(np.bool_), rewrap(out)


def fill_na(dem_ds):
    """``(ind_nans, filled Dataset)``: where the DEM has NaNs, and the DEM with them interpolated
    along x by the nearest valid value (reference helpers.py:137-154).  Needs xarray."""
    _need_xarray("fill_na")
    ind_nans = np.where(np.isnan(get_da(dem_ds)))
    return ind_nans, dem_ds.interpolate_na(dim="x", method="nearest", fill_value="extrapolate")


def timer(func):
    """Decorator that logs how long ``func`` took (reference helpers.py:157-168)."""
    @functools.wraps(func)
    def timed(*args, **kwargs):
        start = time.monotonic()
        result = func(*args, **kwargs)
        logger.info("Computed in %s (HH:mm:ss)", datetime.timedelta(seconds=time.monotonic() - start))
        return result
    return timed


# ---- numpy's own float32 mean() / std(), restated --------------------------------------------------------------------------
# The valley / ridge index standardises the DEM with them (reference topo.py:427) and the GPU forms them in numpy's
# summation order (csrc/moments_np.hip, ``device.mean_std_numpy``).  This is that order in plain numpy - elementwise
# float32 operations only, vectorised over the chunks - as the statement the kernel is held to, and as the check that the
# numpy in this process still sums that way.
def _pairwise_rows(blocks):
    """numpy's pairwise sum of every row of ``blocks`` (k x m, float32)."""
    m = blocks.shape[1]
    if m < 8:
        res = np.zeros(blocks.shape[0], dtype=np.float32)
        for i in range(m):
            res = res + blocks[:, i]
        return res
    if m <= 128:
        r = blocks[:, :8].copy()
        for j in range(1, m // 8):
            r += blocks[:, 8 * j:8 * j + 8]
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
        for i in range(m - m % 8, m):
            res = res + blocks[:, i]
        return res
    half = m // 2
    half -= half % 8
    return _pairwise_rows(blocks[:, :half]) + _pairwise_rows(blocks[:, half:])


def numpy_order_sum(samples, chunk):
    """``samples.sum()`` of a 1-D float32 array as numpy forms it: chunks of ``chunk`` samples summed pairwise, the chunk
    sums (a partial last chunk included) added one after the other from 0."""
    full = samples.size // chunk
    parts = [np.zeros(1, dtype=np.float32)]
    if full:
        parts.append(_pairwise_rows(samples[:full * chunk].reshape(full, chunk)))
    if samples.size % chunk:
        parts.append(_pairwise_rows(samples[None, full * chunk:]))
    return np.add.accumulate(np.concatenate(parts), dtype=np.float32)[-1]


def numpy_order_moments(array, chunk=None):
    """``(array.mean(), array.std())`` of a C-contiguous float32 array, bit for bit, from the model above (``chunk``:
    ``np.getbufsize()``)."""
    samples = np.ascontiguousarray(array, dtype=np.float32).reshape(-1)
    chunk = int(np.getbufsize()) if chunk is None else int(chunk)
    n = np.float32(samples.size)
    with np.errstate(all="ignore"):
        mean = numpy_order_sum(samples, chunk) / n
        dev = samples - mean
        return mean, np.sqrt(numpy_order_sum(dev * dev, chunk) / n)


# ---- the same order on row shards --------------------------------------------------------------------------------------------
# A rank owns samples [first_sample, first_sample + n) of the raster's `count`.  numpy's chunks sit at GLOBAL offsets k * chunk,
# so the rank's part of the summation tree is: one sum per global chunk that lies wholly inside its samples, and the samples
# before its first / after its last chunk boundary as they are (head / tail, each fewer than `chunk`).  A chunk that straddles
# ranks - and the raster's partial last chunk - is put together from those fragments and summed pairwise by whoever combines
# the parts; the chain over the chunk sums then runs over the same floats on every rank (``ShardedDEM.mean_std_numpy``,
# ``topo_amd_shard_mean_std_f32``).
def numpy_order_shard_parts(owned, first_sample, count, chunk, mean=None):
    """One rank's part of ``numpy_order_sum`` over a raster of ``count`` samples: ``owned`` are its samples, the first of them
    global sample ``first_sample``.  A dict: ``chunk_index`` / ``chunk_sums`` the global chunks wholly inside and their
    pairwise sums, ``head`` / ``tail`` the fragments before the first and after the last chunk boundary with ``head_at`` /
    ``tail_at`` their global offsets (samples with no boundary among them are all ``head``).  ``mean``: the same of the squared
    deviations from it, the difference and the product each rounded to float32."""
    values = np.ascontiguousarray(owned, dtype=np.float32).reshape(-1)
    first, count, chunk = int(first_sample), int(count), int(chunk)
    end = first + values.size
    if first < 0 or end > count or chunk < 1:
        raise ValueError(f"samples [{first}, {end}) of a raster of {count}, chunk {chunk}")
    if mean is not None:
        with np.errstate(all="ignore"):
            dev = values - np.float32(mean)
            values = dev * dev
    c0, c1 = -(-first // chunk), end // chunk  # the first / one past the last global chunk boundary inside [first, end]
    empty = np.zeros(0, dtype=np.float32)
    if c0 > c1:  # no boundary inside: one fragment of one chunk
        return {"chunk_index": np.zeros(0, dtype=np.int64), "chunk_sums": empty, "head": values, "head_at": first,
                "tail": empty, "tail_at": end}
    a, b = c0 * chunk - first, c1 * chunk - first
    with np.errstate(all="ignore"):
        sums = _pairwise_rows(values[a:b].reshape(c1 - c0, chunk)) if c1 > c0 else empty
    return {"chunk_index": np.arange(c0, c1, dtype=np.int64), "chunk_sums": sums, "head": values[:a], "head_at": first,
            "tail": values[b:], "tail_at": c1 * chunk}


def numpy_order_combine(parts, count, chunk):
    """``numpy_order_sum`` of the whole raster from every rank's ``numpy_order_shard_parts`` (in any order): full chunks
    taken as summed, every other chunk put together from the fragments in sample order and summed pairwise, then the chain
    from 0.  The parts must tile the raster's ``count`` samples."""
    count, chunk = int(count), int(chunk)
    total = -(-count // chunk)
    sums = np.zeros(total, dtype=np.float32)
    have = np.zeros(total, dtype=bool)
    pieces = []
    for p in parts:
        index = np.asarray(p["chunk_index"], dtype=np.int64)
        if have[index].any():
            raise ValueError("numpy_order_combine: a chunk summed by two ranks")
        sums[index] = p["chunk_sums"]
        have[index] = True
        pieces += [(int(p[k + "_at"]), np.asarray(p[k], dtype=np.float32)) for k in ("head", "tail") if len(p[k])]
    pieces.sort(key=lambda piece: piece[0])
    with np.errstate(all="ignore"):
        for k in np.flatnonzero(~have):
            lo, hi = k * chunk, min((k + 1) * chunk, count)
            mine = [(at, v) for at, v in pieces if lo <= at < hi]
            at = lo
            for start, v in mine:
                if start != at:
                    break
                at += v.size
            if at != hi:
                raise ValueError(f"numpy_order_combine: the parts do not tile samples [{lo}, {hi})")
            sums[k] = _pairwise_rows(np.concatenate([v for _, v in mine])[None, :])[0]
        return np.add.accumulate(np.concatenate([np.zeros(1, dtype=np.float32), sums]), dtype=np.float32)[-1]


def numpy_order_moments_sharded(blocks, chunk=None):
    """``numpy_order_moments`` of the raster whose consecutive row blocks are ``blocks``, from the blocks' parts alone: what a
    row-sharded run gathers, with the bits of the whole raster's ``mean()`` / ``std()`` however the rows are cut."""
    blocks = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in blocks]
    chunk = int(np.getbufsize()) if chunk is None else int(chunk)
    firsts = np.concatenate([[0], np.cumsum([b.size for b in blocks])])
    count = int(firsts[-1])
    n = np.float32(count)
    with np.errstate(all="ignore"):
        parts = [numpy_order_shard_parts(b, f, count, chunk) for b, f in zip(blocks, firsts)]
        mean = numpy_order_combine(parts, count, chunk) / n
        parts = [numpy_order_shard_parts(b, f, count, chunk, mean=mean) for b, f in zip(blocks, firsts)]
        return mean, np.sqrt(numpy_order_combine(parts, count, chunk) / n)


_moments_checked = {}  # chunk -> whether this process's numpy sums as the model says


def moments_chunk():
    """The chunk length (``np.getbufsize()``) with which the GPU forms numpy's float32 moments, or ``None`` when the host has
    to take them as before: ``TOPO_AMD_VALLEY_HOST_MOMENTS=1`` (read at every call), a buffer size that is no power of two
    of 128 or more, or a numpy that does not sum as the model says (checked once per process and buffer size, on a small
    array with a partial chunk; logged)."""
    if os.environ.get("TOPO_AMD_VALLEY_HOST_MOMENTS") == "1":
        return None
    chunk = int(np.getbufsize())
    if chunk not in _moments_checked:
        ok = chunk >= 128 and chunk & (chunk - 1) == 0
        if ok:
            rng = np.random.default_rng(427)
            probe = rng.normal(1800.0, 600.0, size=2 * chunk + 77).astype(np.float32)
            got, want = numpy_order_moments(probe, chunk), (probe.mean(), probe.std())
            ok = got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        _moments_checked[chunk] = ok
        logger.info("numpy %s float32 mean / std in chunks of %d samples: %s", np.__version__, chunk,
                    "as modelled, formed on the GPU" if ok else "not as modelled, taken on the host")
    return chunk if _moments_checked[chunk] else None
