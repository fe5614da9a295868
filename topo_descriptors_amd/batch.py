"""Batch wrappers: all scales of one descriptor with the DEM uploaded to the GPU once.

Counterparts of the reference's ``compute_dem / compute_tpi / compute_std / compute_gradient /
compute_sx`` (reference topo.py:16-59, 88-141, 216-269, 534-594, 715-772): same arguments, same
output names (``_tpi_name`` topo.py:184, ``_std_name`` :310, ``_gradient_names`` :647, ``_sx_name``
:956, ``_dem_name`` :83), NaN re-insertion through ``ind_nans`` (topo.py:139), one output per
scale.  The reference writes netCDF through xarray; here the writer is pluggable: with xarray
installed the same ``topo_<NAME>.nc`` files are produced, otherwise ``topo_<NAME>.npy``.  Every
wrapper also returns ``{name: array}``.
"""
import functools
import logging
import os

import numpy as np

from . import CFG, _lib, device as d, helpers as hlp, topo

logger = logging.getLogger(__name__)


# ---- output names (identical strings to the reference) ---------------------------------------
def _dem_name(scale):
    return f"DEM_{scale}M"


def _tpi_name(scale, smth_factor):
    add = f"_SMTHFACT{smth_factor:.3g}" if smth_factor else ""
    return f"TPI_{scale}M{add}"


def _std_name(scale, smth_factor):
    add = f"_SMTHFACT{smth_factor:.3g}" if smth_factor else ""
    return f"STD_{scale}M{add}"


def _gradient_names(scale, sig_ratio):
    tail = f"_{scale}M_SIGRATIO{sig_ratio:.3g}"
    return ["WE_DERIVATIVE" + tail, "SN_DERIVATIVE" + tail, "SLOPE" + tail, "ASPECT" + tail]


def _valley_ridge_names(scale, mode, smth_factor):
    """reference topo.py:450-458"""
    add = f"_SMTHFACT{smth_factor:.3g}" if smth_factor else ""
    return [f"{mode}_NORM_{scale}M{add}", f"{mode}_DIR_{scale}M{add}"]


def _sx_name(radius, azimuth):
    return f"SX_RADIUS{int(radius)}_AZIMUTH{int(azimuth)}"


# ---- writer ------------------------------------------------------------------------------------
def write_output(array, dem_ds, name, crop=None, outdir=".", units=None):
    """``hlp.to_netcdf`` of the reference (helpers.py:34-65) when xarray is there, .npy otherwise.  A ``PackedPlane`` goes
    into the netCDF file with its packing as the variable's encoding, or into ``topo_<NAME>.npz`` (``values``,
    ``scale_factor``, ``add_offset``, ``fill_value``: NaN for none).  ``array`` is the part of the DEM that ``crop`` selects
    (``helpers.crop_window``), already cut on the GPU: the writer cuts nothing, it takes the coordinates of
    ``dem_ds.sel(crop)`` where there are coordinates to take."""
    name = str.upper(name)
    if outdir is None:
        return None
    os.makedirs(outdir, exist_ok=True)
    packed = array if isinstance(array, _lib.PackedPlane) else None
    if hlp._xr is not None and isinstance(dem_ds, hlp._xr.Dataset):  # pragma: no cover
        domain = dem_ds if crop is None else dem_ds.sel(crop)
        ds = hlp._xr.Dataset({name: (hlp.get_da(dem_ds).dims, packed.decode() if packed else array)}, coords=domain.coords,
                             attrs=dem_ds.attrs)
        if units is not None:
            ds[name].attrs.update(units=units)
        if packed:
            enc = {"dtype": packed.values.dtype}
            if packed.values.dtype.kind != "f":
                enc.update(scale_factor=packed.scale_factor, add_offset=packed.add_offset, _FillValue=packed.fill_value)
            ds[name].encoding.update(enc)
        path = os.path.join(outdir, f"topo_{name}.nc")
        ds.to_netcdf(path)
    else:
        if packed:
            path = os.path.join(outdir, f"topo_{name}.npz")
            np.savez(path, values=packed.values, scale_factor=packed.scale_factor, add_offset=packed.add_offset,
                     fill_value=np.nan if packed.fill_value is None else packed.fill_value)
        else:
            path = os.path.join(outdir, f"topo_{name}.npy")
            np.save(path, array)
    logger.info("saved: %s", path)
    return path


def _as_list(x, n=None):
    if not hasattr(x, "__iter__"):
        x = [x] if n is None else [x] * n
    return list(x)


class _ResidentDem:
    """The DEM on the GPU for the duration of one wrapper call."""

    def __init__(self, dem_val):
        self.source = dem_val if isinstance(dem_val, _lib.PackedDem) else np.asarray(dem_val)
        self.dev = d.DeviceArray.from_host(self.source)  # as stored: decoded on the GPU
        self.block = d.Block(self.dev)
        self.shape = (self.dev.rows, self.dev.nx)
        self._host = None

    @property
    def host(self):
        """The float32 array on the host, made when somebody asks: the plane the GPU decoded."""
        if self._host is None:
            self._host = self.dev.to_host()
        return self._host

    def plane(self):
        return d.DeviceArray(*self.shape)

    def close(self):
        self.dev.free()


class _Finish:
    """What one wrapper call does to every result plane on its way out (``DeviceArray.finish``, csrc/finish.hip): the window
    ``crop`` selects (``helpers.crop_window``) and the mask of ``ind_nans``, both made once per call.  The planes it hands
    out hold the window's ROWS only - every ``*_dev`` call of the wrapper takes ``rows_kw`` and computes nothing else - and the
    finish cuts the columns, puts NaN back and packs, so that only the domain crosses the link.  With neither argument set
    it is ``to_host`` / ``to_packed`` of whole planes."""

    def __init__(self, dem_ds, ind_nans, crop):
        ny, nx = hlp.dem_shape(dem_ds)
        self.nx = nx
        self.window = None if crop is None else hlp.crop_window(dem_ds, crop)
        self.row0, self.rows, self.col0, self.cols = self.window or (0, ny, 0, nx)
        self.empty = self.rows == 0 or self.cols == 0  # nothing selected: zero-size results, no GPU call
        self.rows_kw = {} if self.window is None else {"out_row0": self.row0, "out_rows": self.rows}
        self.mask = None
        if ind_nans is not None and len(ind_nans):
            if isinstance(ind_nans, np.ndarray) and ind_nans.dtype == np.bool_ and ind_nans.shape == (ny, nx):
                flags = ind_nans.view(np.uint8)  # (what ``fill_na_gpu`` returns) as stored
            else:
                flags = np.zeros((ny, nx), dtype=np.uint8)
                flags[ind_nans] = 1  # (numpy's IndexError for an index outside the DEM)
            flags = flags[self.row0:self.row0 + self.rows]
            if not self.empty and flags.any():
                self.mask = d.DeviceArray(self.rows, nx, dtype=np.uint8)
                try:
                    self.mask.upload_rows(flags)
                except BaseException:  # (the wrappers reach close() only once this object exists)
                    self.mask.free()
                    raise

    def plane(self):
        """A result plane: the window's rows at the DEM's width."""
        return d.DeviceArray(self.rows, self.nx)

    def leave(self, plane, packing):
        """A result plane of :meth:`plane` on the host: float32, or packed on the GPU."""
        return plane.finish(packing, self.mask, None if self.window is None else (0, self.rows, self.col0, self.cols))

    def leave_host(self, array, packing):
        """The same for a whole float32 plane that was made on the host: its rows are uploaded and finished by the same device
        call (one definition of the bits is worth an upload on a rare path)."""
        dev = self.plane()
        try:
            dev.upload_rows(array[self.row0:self.row0 + self.rows])
            return self.leave(dev, packing)
        finally:
            dev.free()

    def nothing(self, packing, dtype=np.float32):
        """The result of an empty window."""
        values = np.empty((self.rows, self.cols), dtype=dtype if packing is None else packing.dtype)
        return values if packing is None else _lib.PackedPlane(values, packing, 0, 0)

    def close(self):
        if self.mask is not None:
            self.mask.free()


def _emit(array, dem_ds, name, crop, outdir, units, results):
    write_output(array, dem_ds, name, crop, outdir, units)
    results[name] = array


def compute_dem(dem_ds, scales, ind_nans=(), crop=None, outdir=".", pack=None, skipna=False, min_weight=0.0, fill=False):
    """Gaussian-smoothed DEM per scale, sigma = scale_px / CFG.scale_std (reference topo.py:16-59).  ``pack`` (here and in the
    other wrappers): a ``Packing`` - every plane is encoded on the GPU, leaves it at 1 or 2 bytes a sample, and is returned
    and saved as a ``PackedPlane`` (``write_output``); ``ind_nans`` then receive the fill code.  ``crop`` and ``ind_nans``
    (here and in the other wrappers) are applied on the GPU: only the rows of the domain are computed, only the domain is
    downloaded, returned and saved (``helpers.crop_window``: what ``Dataset.sel(crop)`` selects; no xarray needed), and
    ``ind_nans`` - an index tuple as ``np.where`` gives it, or the boolean mask of ``fill_na_gpu`` - goes up once per call.
    ``skipna=True``: the Gaussian over the samples that exist (``topo.dem(skipna=True)``: pass the DEM UNFILLED) with its
    ``min_weight`` and ``fill``; ``crop`` and ``ind_nans`` are applied afterwards as ever, output names are unchanged."""
    min_weight = topo._valid_gauss_args(skipna, min_weight, fill, False, "compute_dem")
    packing, = _lib.pack_list(pack, ["dem"])
    hlp.check_dem(dem_ds)
    scales = _as_list(scales)
    scales_pxl, _ = hlp.scale_to_pixel(scales, dem_ds)
    fin, results = _Finish(dem_ds, ind_nans, crop), {}
    if fin.empty:
        for scale in scales:
            _emit(fin.nothing(packing), dem_ds, _dem_name(scale), crop, outdir, "m", results)
        return results
    res = out = None
    try:
        res = _ResidentDem(hlp.get_da(dem_ds).values)
        out = fin.plane()
        for scale, px in zip(scales, scales_pxl):
            sigma = px / CFG.scale_std
            if skipna:
                res.block.gaussian_valid(sigma, sigma, out, min_weight=min_weight, fill=fill, **fin.rows_kw)
            else:
                res.block.gaussian(sigma, sigma, out, **fin.rows_kw)
            _emit(fin.leave(out, packing), dem_ds, _dem_name(scale), crop, outdir, "m", results)
    finally:
        if out is not None:
            out.free()
        if res is not None:
            res.close()
        fin.close()
    return results


def _tpi_std(dem_ds, scales, smth_factors, ind_nans, crop, outdir, want, pack=None, skipna=False, min_count=1):
    hlp.check_dem(dem_ds)
    packing, = _lib.pack_list(pack, [want])
    scales = _as_list(scales)
    smth_factors = _as_list(smth_factors, len(scales))
    if skipna and any(f is not None for f in smth_factors):
        raise ValueError(f"compute_{want}: skipna=True takes no smoothing factor: smooth over the gaps first, "
                         f"topo.{want}(topo.dem(d, sigma, skipna=True), size, skipna=True) - or compute_dem(skipna=True) and "
                         f"compute_{want}(skipna=True) on its planes")
    min_count = topo._skipna_args(skipna, min_count, None, f"compute_{want}")
    scales_pxl, _ = hlp.scale_to_pixel(scales, dem_ds)
    sigmas = hlp.get_sigmas(smth_factors, scales_pxl)
    name_of = _tpi_name if want == "tpi" else _std_name
    fin, results = _Finish(dem_ds, ind_nans, crop), {}
    if fin.empty:
        for scale, fact in zip(scales, smth_factors):
            array = fin.nothing(packing, np.float32 if want == "tpi" else np.float64)
            _emit(array, dem_ds, name_of(scale, fact), crop, outdir, "m", results)
        return results
    res = out = smooth = second = None
    try:
        res = _ResidentDem(hlp.get_da(dem_ds).values)
        out = fin.plane()
        # un-smoothed TPI at two small scales shares one pass over the DEM (Block.tpi_multi).  A pair is
        # computed when the loop reaches its first member: that plane is finished (NaN re-insertion, output) at once,
        # the partner's waits on the host for its turn - one extra host plane at most, and nothing computed is lost if a
        # later scale fails.
        partner, ahead = {}, {}
        if want == "tpi" and not skipna:  # (the valid-sample kernel takes its discs one by one)
            small = {}
            for k, (px, sigma) in enumerate(zip(scales_pxl, sigmas)):
                if not sigma and int(px) in (5, 7, 9, 11):
                    small.setdefault(int(px), k)
            sizes = sorted(small)
            for a, b in zip(sizes[0::2], sizes[1::2]):
                ka, kb = sorted((small[a], small[b]))
                partner[ka] = kb
            if len(sizes) % 2:
                logger.info("TPI at %s px has no partner for a shared pass: computed alone", sizes[-1])
        for k, (scale, px, fact, sigma) in enumerate(zip(scales, scales_pxl, smth_factors, sigmas)):
            logger.info("Computing scale %s meters with smoothing factor %s ...", scale, fact)
            if k in ahead:
                _emit(ahead.pop(k), dem_ds, _tpi_name(scale, fact), crop, outdir, "m", results)
                continue
            if k in partner:
                kb = partner[k]
                second = second or fin.plane()
                res.block.tpi_multi([int(px), int(scales_pxl[kb])], [out, second], **fin.rows_kw)
                ahead[kb] = fin.leave(second, packing)
                _emit(fin.leave(out, packing), dem_ds, _tpi_name(scale, fact), crop, outdir, "m", results)
                continue
            block = res.block
            if sigma:  # pre-smoothing (reference topo.py:172-173, :297-298): the whole plane, its consumer reads beyond the window
                smooth = smooth or res.plane()
                res.block.gaussian(sigma, sigma, smooth)
                block = d.Block(smooth)
            run = block.tpi_std_valid if skipna else block.tpi_std
            valid_kw = {"min_count": min_count} if skipna else {}
            run(int(px), **{want: out}, **valid_kw, **fin.rows_kw)
            array = fin.leave(out, packing)
            if want == "std" and packing is None:
                array = array.astype(np.float64)  # (packed: not widened)
            _emit(array, dem_ds, name_of(scale, fact), crop, outdir, "m", results)
    finally:
        for plane in (out, smooth, second):
            if plane is not None:
                plane.free()
        if res is not None:
            res.close()
        fin.close()
    return results


def compute_tpi(dem_ds, scales, smth_factors=None, ind_nans=(), crop=None, outdir=".", pack=None, skipna=False, min_count=1):
    """TPI for every scale (reference topo.py:88-141).  ``pack``, ``crop``, ``ind_nans``: see :func:`compute_dem`.
    ``skipna=True``: the mean of the samples that exist (``topo.tpi(skipna=True)``) - pass the DEM UNFILLED, its gaps as NaN
    or as the declared fill value of a ``PackedDem``; ``min_count``: the valid taps a pixel needs.  No smoothing factor in
    this mode (``ValueError``): pre-smoothing over gaps is the chain ``topo.tpi(topo.dem(d, sigma, skipna=True), size,
    skipna=True)``, or ``compute_dem(skipna=True)`` first; output names are unchanged."""
    logger.info("***Starting TPI computation for scales %s meters***", scales)
    return _tpi_std(dem_ds, scales, smth_factors, ind_nans, crop, outdir, "tpi", pack, skipna, min_count)


def compute_std(dem_ds, scales, smth_factors=None, ind_nans=(), crop=None, outdir=".", pack=None, skipna=False, min_count=1):
    """Windowed standard deviation for every scale (reference topo.py:216-269).  ``pack``, ``crop``, ``ind_nans``: see
    :func:`compute_dem`; a packed plane is not widened to float64.  ``skipna``, ``min_count``: see :func:`compute_tpi`
    (``topo.std(skipna=True)``)."""
    logger.info("***Starting STD computation for scales %s meters***", scales)
    return _tpi_std(dem_ds, scales, smth_factors, ind_nans, crop, outdir, "std", pack, skipna, min_count)


def compute_gradient(dem_ds, scales, sig_ratios=1, ind_nans=(), crop=None, outdir=".", pack=None, skipna=False, min_weight=0.0,
                     fill=False):
    """dx, dy, slope, aspect for every scale (reference topo.py:534-594).  ``pack``: a dict with the keys ``dx``, ``dy``,
    ``slope``, ``aspect`` (a missing key: float32), or one ``Packing`` for the four.  ``crop``, ``ind_nans``: see
    :func:`compute_dem`.  With 2-D per-pixel resolutions (a WGS84 grid) the gradient keeps its host-buffer call, which
    computes whole planes; when a mask or a crop is present that call is made at float32 and each plane's domain rows are
    uploaded again and finished by the same device call as everywhere else, so that the bits of a masked, cropped or packed
    sample have one definition - an upload on a rare path.
    ``skipna=True``: the gradient over the samples that exist (``topo.gradient(skipna=True)``: pass the DEM UNFILLED) with its
    ``min_weight`` and ``fill``, on the resident DEM (``Block.gradient_valid``); ``crop``, ``ind_nans`` and ``pack`` are applied
    afterwards as ever, output names are unchanged."""
    min_weight = topo._valid_gauss_args(skipna, min_weight, fill, False, "compute_gradient")
    valid_kw = {"skipna": True, "min_weight": min_weight, "fill": fill} if skipna else {}
    hlp.check_dem(dem_ds)
    packs = _lib.pack_list(pack, topo.GRADIENT_PLANES)
    logger.info("***Starting gradients computation for scales %s meters***", scales)
    scales = _as_list(scales)
    sig_ratios = _as_list(sig_ratios, len(scales))
    scales_pxl, res_meters = hlp.scale_to_pixel(scales, dem_ds)
    sigmas = scales_pxl / CFG.scale_std
    dem_val = hlp.get_da(dem_ds).values
    units = ["1", "1", "degree", "degree"]
    fin, results = _Finish(dem_ds, ind_nans, crop), {}
    if fin.empty:
        for scale, ratio in zip(scales, sig_ratios):
            for q, name, unit in zip(packs, _gradient_names(scale, ratio), units):
                _emit(fin.nothing(q), dem_ds, name, crop, outdir, unit, results)
        return results
    two_d = np.ndim(res_meters["x"]) > 1 or np.ndim(res_meters["y"]) > 1
    plain = fin.window is None and fin.mask is None
    res, outs = None, []
    try:
        if not two_d:
            res = _ResidentDem(dem_val)
            outs = [fin.plane() for _ in range(4)]
        for scale, sigma, ratio in zip(scales, sigmas, sig_ratios):
            names = _gradient_names(scale, ratio)
            if two_d and plain:  # per-pixel resolutions (WGS84 grids): host-buffer entry point
                arrays = topo.gradient(dem_val, sigma, res_meters, sig_ratio=ratio, pack=None if pack is None else packs, **valid_kw)
            elif two_d:
                whole = topo.gradient(dem_val, sigma, res_meters, sig_ratio=ratio, **valid_kw)
                arrays = [fin.leave_host(a, q) for a, q in zip(whole, packs)]
                arrays = [a.astype(w.dtype, copy=False) if q is None else a for a, w, q in zip(arrays, whole, packs)]
            else:
                run = res.block.gradient
                if skipna:
                    run = functools.partial(res.block.gradient_valid, min_weight=min_weight, fill=fill)
                run(sigma, res_meters["x"], res_meters["y"], sig_ratio=ratio,
                    dx=outs[0], dy=outs[1], slope=outs[2], aspect=outs[3], **fin.rows_kw)
                arrays = [fin.leave(o, q) for o, q in zip(outs, packs)]
            for array, name, unit in zip(arrays, names, units):
                _emit(array, dem_ds, name, crop, outdir, unit, results)
    finally:
        for o in outs:
            o.free()
        if res is not None:
            res.close()
        fin.close()
    return results


def compute_sx(dem_ds, azimuth, radius, height=10.0, azimuth_arc=10.0, azimuth_steps=15,
               radius_min=0.0, crop=None, outdir=".", pack=None):
    """Sx for one azimuth (reference topo.py:715-772).  ``azimuth`` may also be a sequence: the
    planes of all azimuths then come from one pass over the DEM (``topo.sx_multi``), each saved
    under the name the reference gives it.  ``pack``: see :func:`compute_dem`.  With a ``crop`` the scan runs on the
    device-resident DEM over the rows of the domain only (``Block.sx`` / ``Block.sx_multi``) and is finished like the other
    wrappers' planes: the bits of the call without a crop, inside the domain."""
    hlp.check_dem(dem_ds)
    logger.info("***Starting Sx computation for azimuth %s meters and radius %s***", azimuth, radius)
    results = {}
    if crop is not None:
        return _sx_cropped(dem_ds, azimuth, radius, height, azimuth_arc, azimuth_steps, radius_min, crop, outdir, pack)
    if np.ndim(azimuth) == 0:
        array = topo.sx(dem_ds, azimuth, radius, height=height, azimuth_arc=azimuth_arc,
                        azimuth_steps=azimuth_steps, radius_min=radius_min, pack=pack)
        _emit(array, dem_ds, _sx_name(radius, azimuth), crop, outdir, "degree", results)
        return results
    arrays = topo.sx_multi(dem_ds, azimuth, radius, height=height, azimuth_arc=azimuth_arc,
                           azimuth_steps=azimuth_steps, radius_min=radius_min, pack=pack)
    for az, array in zip(azimuth, arrays):
        _emit(array, dem_ds, _sx_name(radius, az), crop, outdir, "degree", results)
    return results


def _sx_cropped(dem_ds, azimuth, radius, height, azimuth_arc, azimuth_steps, radius_min, crop, outdir, pack):
    """``compute_sx`` with a crop: the sectors of ``topo.sx`` / ``topo.sx_multi`` scanned on a resident DEM."""
    single = np.ndim(azimuth) == 0
    azimuths = [azimuth] if single else list(azimuth)
    names = [_sx_name(radius, az) for az in azimuths]
    packs = _lib.pack_list(pack, ["sx"] if single else [str(float(a)) for a in azimuths])
    values = topo._values(hlp.get_da(dem_ds).values)
    topo._check_2d(values, "compute_sx")
    fin, results = _Finish(dem_ds, None, crop), {}
    if fin.empty:
        for q, name in zip(packs, names):
            _emit(fin.nothing(q, values.dtype), dem_ds, name, crop, outdir, "degree", results)
        return results
    spacing = hlp.scale_to_pixel(radius, dem_ds)[1]
    dx, dy = spacing["x"].mean(), spacing["y"].mean()
    sectors = [d.sx_offsets(az if single else float(az), radius, dx, dy, azimuth_arc, azimuth_steps, radius_min) for az in azimuths]
    ny, nx = values.shape
    arrays, todo = [None] * len(sectors), []
    res, outs = None, []
    try:
        for k, (reach, _, _, dist) in enumerate(sectors):
            if ny <= 2 * reach or nx <= 2 * reach or np.size(dist) == 0 or np.all(np.isnan(dist)):
                # nothing but frame, or no usable ray pixel (NaN inside the frame): made on the host, like topo.sx
                whole = np.zeros((ny, nx), dtype=np.float32)
                if ny > 2 * reach and nx > 2 * reach:
                    whole[reach:ny - reach, reach:nx - reach] = np.nan
                arrays[k] = fin.leave_host(whole, packs[k])
            else:
                todo.append(k)
        if todo:
            res = _ResidentDem(values)
            outs = [fin.plane() for _ in todo]
            if single:
                reach, dj, di, dist = sectors[0]
                res.block.sx(dj, di, dist, reach, height, outs[0], **fin.rows_kw)
            else:
                res.block.sx_multi([sectors[k] for k in todo], height, outs, **fin.rows_kw)
            for k, o in zip(todo, outs):
                arrays[k] = fin.leave(o, packs[k])
        for array, q, name in zip(arrays, packs, names):
            if q is None:
                array = array.astype(values.dtype, copy=False)  # (the DEM's type, like topo.sx)
            _emit(array, dem_ds, name, crop, outdir, "degree", results)
    finally:
        for o in outs:
            o.free()
        if res is not None:
            res.close()
        fin.close()
    return results


def compute_valley_ridge(dem_ds, scales, mode, flat_list=[0, 0.15, 0.3], smth_factors=None, ind_nans=(),  # noqa: B006
                         crop=None, outdir=".", pack=None):
    """Valley or ridge index (norm and direction) for every scale (reference topo.py:317-386).

    The DEM goes to the GPU once; per scale the optional pre-smoothing, numpy's float32 mean and standard deviation of the
    (smoothed) plane and the 180-angle pass run on the device-resident plane, and only the two result planes leave it.
    ``pack``: one ``Packing`` for both planes, or a dict with the keys ``norm`` and ``direction``.  ``crop``, ``ind_nans``: see
    :func:`compute_dem`; the mean and standard deviation stay those of the WHOLE (smoothed) raster."""
    hlp.check_dem(dem_ds)
    packs = _lib.pack_list(pack, ["norm", "direction"])
    if mode not in ("valley", "ridge"):
        raise ValueError(f"Unknown mode {mode!r}")
    logger.info("***Starting %s index computation for scales %s meters***", mode, scales)
    scales = _as_list(scales)
    smth_factors = _as_list(smth_factors, len(scales))
    scales_pxl, _ = hlp.scale_to_pixel(scales, dem_ds)
    sigmas = hlp.get_sigmas(smth_factors, scales_pxl)
    fin, results = _Finish(dem_ds, ind_nans, crop), {}
    if fin.empty:
        for scale, fact in zip(scales, smth_factors):
            for q, name in zip(packs, _valley_ridge_names(scale, mode, fact)):
                _emit(fin.nothing(q), dem_ds, name, crop, outdir, "1", results)
        return results
    angles = np.arange(0, 180, dtype=np.float32)

    def tables(px):
        kernels = topo._ridge_kernels(int(px), flat_list) if mode == "ridge" else topo._valley_kernels(int(px), flat_list)
        return (kernels.shape[0],) + topo._valley_ridge_tables(kernels, angles)

    # the rotated kernels of the next scale are built on the host while the GPU works on this one
    from concurrent.futures import ThreadPoolExecutor  # noqa: PLC0415
    pool = ThreadPoolExecutor(1)
    res = norm = direction = smooth = None
    try:
        res = _ResidentDem(hlp.get_da(dem_ds).values)
        norm, direction = fin.plane(), fin.plane()
        ahead = pool.submit(tables, scales_pxl[0]) if len(scales) else None
        for k, (scale, px, fact, sigma) in enumerate(zip(scales, scales_pxl, smth_factors, sigmas)):
            logger.info("Computing scale %s meters with smoothing factor %s ...", scale, fact)
            block = res.block
            if sigma:  # pre-smoothing (reference topo.py:424-425): the whole plane
                smooth = smooth or res.plane()
                res.block.gaussian(sigma, sigma, smooth)
                block = d.Block(smooth)
            n_planes, taps, ksize, ang = ahead.result()
            ahead = pool.submit(tables, scales_pxl[k + 1]) if k + 1 < len(scales) else None
            # numpy's own float32 mean / std of the whole (smoothed) array, like the reference (topo.py:427) and like
            # topo.valley_ridge - the wrapper and the single call agree bit for bit, also where two directions nearly tie -
            # formed on the resident plane (device.mean_std_numpy): the block is the whole raster
            moments = {}
            if fin.window is not None:  # the output rows are a subset: the whole raster's moments go in by value
                moments = dict(zip(("mean", "stdev"), block.moments()))
            block.valley_ridge(taps, ksize, ang, n_planes, norm=norm, direction=direction, **moments, **fin.rows_kw)
            for plane, packing, name in zip((norm, direction), packs, _valley_ridge_names(scale, mode, fact)):
                _emit(fin.leave(plane, packing), dem_ds, name, crop, outdir, "1", results)
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
        for a in (norm, direction, smooth):
            if a is not None:
                a.free()
        if res is not None:
            res.close()
        fin.close()
    return results
