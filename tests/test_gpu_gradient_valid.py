"""Valid-sample gradient (``topo.gradient(skipna=True)``; csrc/gradient.hip K4v) on the GPU, every pixel against the float64
reference of tests/gradient_valid_ref.py (tests/test_gradient_valid_design.py shows what its comparison notices).

Rasters: those of tests/disc_valid_ref.py - ``frac``, ``hard``, ``whole`` at 150 x 299, 150 x 300 and 40 x 50 (narrower than the
long radii), ``clean`` at 150 x 299: several tiles both ways, an odd width, a NaN block with one valid pixel in it, NaN at a corner
and beside two borders, +inf, 1e20 and a -9999 block.  sigma 0.75 (Sobel), 1.25, 3.25, 12, 30.25 (radii 5, 13, 48, 121) and
``sig_ratio`` 2 and 0.5 at 3.25.  Resolutions: scalar and 1-D with a negative y on the resident block, per pixel through
``topo.gradient``.  The bounds are gradient_valid_ref's; none is fitted to a run.  Every comparison prints ``FIG ...``."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

from oracle import topo_oracle as orc
import disc_valid_ref as dv
import gradient_valid_ref as gr
import topo_descriptors_amd as tda
from topo_descriptors_amd import CFG, _lib, batch, device as d, topo

pytestmark = pytest.mark.gpu

RASTER_IDS = [f"{k}{ny}x{nx}" for k, ny, nx in gr.RASTERS]
NAMES = ("dx", "dy", "slope", "aspect")


@functools.lru_cache(maxsize=None)
def resident(kind, ny=dv.GNY, nx=dv.NX):
    return d.DeviceArray.from_host(dv.raster(kind, ny, nx))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run(block, sigma, ratio, res, min_weight=0.0, fill=False, rows=None, want=NAMES, valid=True, **kw):
    """The four float32 host planes (``None``: not asked for) of ``Block.gradient_valid`` (``valid=False``: ``Block.gradient``)."""
    rows = block.rows if rows is None else rows
    outs = {name: d.DeviceArray(rows, block.nx) for name in want}
    try:
        if valid:
            block.gradient_valid(sigma, res["x"], res["y"], sig_ratio=ratio, min_weight=min_weight, fill=fill, **outs, **kw)
        else:
            block.gradient(sigma, res["x"], res["y"], sig_ratio=ratio, **outs, **kw)
        return [outs[name].to_host() if name in outs else None for name in NAMES]
    finally:
        for o in outs.values():
            o.free()


def compute(kind, ny, nx, sigma, ratio, mode, min_weight=0.0, fill=False):
    """The call on a whole raster: on the resident block, or (per-pixel resolutions) through ``topo.gradient``."""
    res = gr.resolutions(mode, (ny, nx))
    if mode == "2d":
        return topo.gradient(dv.raster(kind, ny, nx), sigma, res, sig_ratio=ratio, skipna=True, min_weight=min_weight, fill=fill)
    return run(d.Block(resident(kind, ny, nx)), sigma, ratio, res, min_weight, fill)


@functools.lru_cache(maxsize=None)
def whole(kind, sigma, ratio, mode, fill=False):
    """The planes of the call on the whole 150 x 299 raster, shared by the tests that compare bits with it."""
    planes = compute(kind, dv.GNY, dv.NX, sigma, ratio, mode, 0.0, fill)
    for p in planes:
        p.setflags(write=False)
    return planes


# ---- accuracy and NaN masks: every pixel against the reference ------------------------------------------------------------
@pytest.mark.parametrize("sigma,ratio", gr.CASES, ids=str)
@pytest.mark.parametrize("kind,ny,nx", gr.RASTERS, ids=RASTER_IDS)
def test_every_pixel_against_the_reference(kind, ny, nx, sigma, ratio):
    for mode in gr.RES_MODES:
        for fill in (False, True):
            got = compute(kind, ny, nx, sigma, ratio, mode, 0.0, fill)
            gr.check(got, gr.reference(kind, ny, nx, sigma, ratio, mode, 0.0, fill),
                     f"gradient_valid {kind} {ny}x{nx} sigma {sigma} ratio {ratio} res {mode} fill {fill}")


@pytest.mark.parametrize("sigma,ratio", [c for c in gr.CASES if c[0] > 1], ids=str)
@pytest.mark.parametrize("kind,ny,nx", gr.RASTERS, ids=RASTER_IDS)
def test_min_weight_against_the_reference(kind, ny, nx, sigma, ratio):
    for min_weight in gr.MIN_WEIGHTS:
        for fill in (False, True):
            got = compute(kind, ny, nx, sigma, ratio, "s", min_weight, fill)
            gr.check(got, gr.reference(kind, ny, nx, sigma, ratio, "s", min_weight, fill),
                     f"gradient_valid {kind} {ny}x{nx} sigma {sigma} ratio {ratio} min_weight {min_weight} fill {fill}")


def test_min_weight_means_nothing_to_the_sobel_route():
    res = gr.resolutions("s", (dv.GNY, dv.NX))
    assert all(same_bits(a, b) for a, b in zip(run(d.Block(resident("frac")), 0.75, 1, res, 0.9), whole("frac", 0.75, 1, "s")))


# ---- a raster without gaps: the plain gradient ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", gr.RES_MODES)
@pytest.mark.parametrize("sigma,ratio", gr.CASES, ids=str)
def test_a_gap_free_raster_agrees_with_the_plain_gradient(sigma, ratio, mode):
    """Within the sum of both modes' bounds.  dx, dy: each mode is held to ``k 1e-3 / |res| + 4 eps32 |ref|`` against float64 (the
    plain one by tests/test_gpu_parity.py's 1e-3 m on the smoothed field), Sobel to ``8 eps32 M / |res|``.  Slope and aspect: each
    mode is held to SLOPE_TOL / ASPECT_TOL against float64 on its own dx, dy; between the modes the gradient vector moves by at
    most ``|delta| = hypot`` of the two dx, dy bounds, which turns slope by at most ``degrees(|delta|)`` (atan's derivative is at
    most 1) and the direction by at most ``asin(|delta| / |g|)`` (any angle once ``|delta| >= |g|``)."""
    dem = dv.raster("clean")
    res = gr.resolutions(mode, dem.shape)
    ref = gr.reference("clean", dv.GNY, dv.NX, sigma, ratio, mode)
    got = whole("clean", sigma, ratio, mode)
    if mode == "2d":
        plain = topo.gradient(dem, sigma, res, sig_ratio=ratio)
    else:
        plain = run(d.Block(resident("clean")), sigma, ratio, res, valid=False)
    assert all(np.isfinite(p).all() for p in got)
    bounds = []
    for k in (0, 1):
        r = np.abs(ref.res[k])
        one = 8 * gr.EPS32 * ref.largest / r if sigma <= 1 else \
            np.where(ref.one_sided[k], 2.0, 1.0) * gr.VALUE_BOUND / r + 4 * gr.EPS32 * np.abs(ref.planes[k])
        bounds.append(2 * one)
        share = float((np.abs(got[k].astype(np.float64) - plain[k]) / bounds[k]).max())
        print(f"FIG clean sigma {sigma} ratio {ratio} res {mode}: {NAMES[k]} differs from the plain call by {share:.3f} of the bound")
        assert share <= 1.0
    delta = np.hypot(*bounds)
    g = np.hypot(got[0].astype(np.float64), got[1].astype(np.float64))
    slope_share = float((np.abs(got[2].astype(np.float64) - plain[2]) / (2 * gr.SLOPE_TOL + np.degrees(delta))).max())
    turn = np.where(delta < g, np.degrees(np.arcsin(np.minimum(1.0, delta / np.maximum(g, 1e-300)))), 180.0)
    aspect_share = float((orc.wrapped_angle_diff(got[3], plain[3]) / (2 * gr.ASPECT_TOL + turn)).max())
    print(f"FIG clean sigma {sigma} ratio {ratio} res {mode}: slope {slope_share:.3f}, aspect {aspect_share:.3f} of the bound")
    assert slope_share <= 1.0 and aspect_share <= 1.0
    if mode == "s":
        filled = run(d.Block(resident("clean")), sigma, ratio, res, 0.9, True)
        assert all(same_bits(a, b) for a, b in zip(filled, got))  # (neither argument has anything to do here)
        if sigma <= 1:
            assert all(same_bits(a, b) for a, b in zip(plain, got))  # the Sobel pair without a gap: the plain kernel's bits


# ---- row blocks -------------------------------------------------------------------------------------------------------------
CUTS = ((0, 47), (47, 75), (75, 150))  # the cut at row 75 goes through the NaN block [60, 90) and its one valid pixel


def ghost_rows(sigma, ratio):
    return 1 if sigma <= 1 else gr.gv.radius(max(sigma, sigma * ratio)) + 1


@pytest.mark.parametrize("sigma,ratio", [(0.75, 1), (3.25, 1), (3.25, 2), (12.0, 1)], ids=str)
def test_row_blocks_with_the_fewest_ghost_rows_give_the_whole_rasters_bits(sigma, ratio):
    dem = dv.raster("frac")
    gny = dem.shape[0]
    res = gr.resolutions("1d", dem.shape)
    h = ghost_rows(sigma, ratio)
    for fill in (False, True):
        want = whole("frac", sigma, ratio, "1d", fill)
        for o0, o1 in CUTS:
            lo, hi = max(0, o0 - h), min(gny, o1 + h)
            part = d.DeviceArray.from_host(np.ascontiguousarray(dem[lo:hi]))
            try:
                got = run(d.Block(part, row0=lo, gny=gny), sigma, ratio, res, 0.0, fill, rows=o1 - o0, out_row0=o0, out_rows=o1 - o0)
            finally:
                part.free()
            assert all(same_bits(a, b[o0:o1]) for a, b in zip(got, want)), (o0, o1, fill)
        # windows of the whole block, off every row group and tile boundary
        for o0, rows in ((37, 64), (0, 1), (gny - 3, 3)):
            got = run(d.Block(resident("frac")), sigma, ratio, res, 0.0, fill, rows=rows, out_row0=o0, out_rows=rows)
            assert all(same_bits(a, b[o0:o0 + rows]) for a, b in zip(got, want)), (o0, rows, fill)


@pytest.mark.parametrize("sigma,ratio", [(0.75, 1), (3.25, 1), (3.25, 2)], ids=str)
def test_a_block_with_one_ghost_row_fewer_is_refused(sigma, ratio):
    dem = dv.raster("frac")
    gny = dem.shape[0]
    res = gr.resolutions("s", dem.shape)
    h = ghost_rows(sigma, ratio)
    o0, o1 = 47, 75
    for lo, hi in ((o0 - h + 1, o1 + h), (o0 - h, o1 + h - 1)):
        part = d.DeviceArray.from_host(np.ascontiguousarray(dem[lo:hi]))
        try:
            with pytest.raises(_lib.TopoAmdError, match="ghost rows"):
                run(d.Block(part, row0=lo, gny=gny), sigma, ratio, res, rows=o1 - o0, out_row0=o0, out_rows=o1 - o0)
        finally:
            part.free()


# ---- output planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,ratio", [(0.75, 1), (3.25, 1)], ids=str)
def test_any_subset_of_the_planes_may_be_left_out(sigma, ratio):
    res = gr.resolutions("s", (dv.GNY, dv.NX))
    full = whole("frac", sigma, ratio, "s")
    for n in (1, 2, 3):
        for want in itertools.combinations(NAMES, n):
            got = run(d.Block(resident("frac")), sigma, ratio, res, want=want)
            for name, a, b in zip(NAMES, got, full):
                assert (a is None) == (name not in want) and (a is None or same_bits(a, b)), (want, name)
    run(d.Block(resident("frac")), sigma, ratio, res, want=())  # no plane at all: nothing to do, no error


def test_the_route_report():
    res = gr.resolutions("s", (dv.GNY, dv.NX))
    block = d.Block(resident("frac"))
    # (the plain calls on the raster without gaps: on one with a NaN the library remembers it and the next plain call goes
    # straight to the two passes - tests/test_gpu_gradient_routes.py)
    clean = d.Block(resident("clean"))
    run(clean, 3.25, 1, res, valid=False)
    plain = d.gradient_route()
    assert plain & 7 in range(5) and plain >> 3
    for sigma, ratio, code in ((3.25, 1, 5), (3.25, 2, 6), (3.25, 0.5, 6), (0.75, 1, 5), (0.75, 2, 5), (30.25, 1, 5)):
        for blk in (block, clean):
            run(blk, sigma, ratio, res)
            assert d.gradient_route() == code, (sigma, ratio)
    run(clean, 3.25, 1, res, valid=False)
    assert d.gradient_route() == plain
    run(clean, 0.75, 1, res, valid=False)
    assert d.gradient_route() == 0


# ---- error codes ------------------------------------------------------------------------------------------------------------
def test_error_codes():
    lib = _lib.lib()
    dem = resident("frac")
    out = d.DeviceArray(dv.GNY, dv.NX)
    one = np.ones(1)
    try:
        def call(sigma, ratio=1.0, min_weight=0.0, mode=_lib.RES_SCALAR, rx=one, ry=one):
            return lib.topo_amd_gradient_valid_dev(dem.ptr, dv.GNY, 0, dv.GNY, dv.NX, sigma, ratio, min_weight, 0, mode, _lib.ptr(rx),
                                                   _lib.ptr(ry), 0, dv.GNY, out.ptr, None, None, None)

        assert call(31.0) == -5 and call(16.0, 2.0) == -5 and call(1e9) == -5  # TOPO_AMD_EUNSUP: radii 124, 128
        for bad in (-0.1, 1.5, float("nan")):
            assert call(3.25, 1.0, bad) == -1  # TOPO_AMD_EINVAL
        assert call(-1.0) == -1 and call(float("nan")) == -1 and call(3.25, 0.0) == -1 and call(3.25, float("nan")) == -1
        assert call(3.25, mode=3) == -1 and call(3.25, rx=None) == -1
        assert call(30.25, 1.0, 1.0) == 0 and call(0.75, 1.0, 1.0) == 0 and call(15.0, 2.0) == 0  # radii 121, Sobel, 120
        d.sync()
    finally:
        out.free()
    with pytest.raises(_lib.TopoAmdError, match="status -5"):
        topo.gradient(dv.raster("frac"), 31.0, {"x": 25.0, "y": -25.0}, skipna=True)


# ---- host paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,ratio,mode", [(0.75, 1, "s"), (3.25, 1, "1d"), (3.25, 2, "s")], ids=str)
def test_topo_gradient_and_sobel_give_the_bits_of_the_resident_call(sigma, ratio, mode):
    dem = dv.raster("frac")
    res = gr.resolutions(mode, dem.shape)
    for fill in (False, True):
        got = topo.gradient(dem, sigma, res, sig_ratio=ratio, skipna=True, fill=fill)
        assert all(p.dtype == np.float32 and same_bits(p, w) for p, w in zip(got, whole("frac", sigma, ratio, mode, fill)))
    if sigma <= 1:
        unit = {"x": 1.0, "y": 1.0}
        for fill in (False, True):
            want = run(d.Block(resident("frac")), sigma, 1, unit, 0.0, fill)
            dx, dy = topo.sobel(dem, skipna=True, fill=fill)
            assert same_bits(dx, want[0]) and same_bits(dy, want[1])
        clean = dv.raster("clean")
        assert all(same_bits(a, b) for a, b in zip(topo.sobel(clean, skipna=True), topo.sobel(clean)))


def test_without_skipna_the_bits_are_the_plain_call():
    dem = dv.raster("clean")
    res = gr.resolutions("s", dem.shape)
    want = run(d.Block(resident("clean")), 3.25, 1, res, valid=False)
    assert all(same_bits(a, b) for a, b in zip(topo.gradient(dem, 3.25, res), want))


NY, NX, SEAM = 3100, 203, 960  # three row chunks of at least 960 rows at TOPO_AMD_HOST_CHUNK_MB=1 (tests/test_gpu_valid_host_chunks.py)
ENV = ("TOPO_AMD_HOST_CHUNK_MB", "TOPO_AMD_HOST_PIPELINE", "TOPO_AMD_HOST_DOWNLOADS")


@pytest.fixture
def chunk_env():
    saved = {k: os.environ.get(k) for k in ENV}
    os.environ["TOPO_AMD_HOST_CHUNK_MB"] = "1"
    os.environ.pop("TOPO_AMD_HOST_PIPELINE", None)
    os.environ.pop("TOPO_AMD_HOST_DOWNLOADS", None)
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


class Pinned:
    """A page-locked array from topo_amd_host_alloc."""

    def __init__(self, shape, dtype=np.float32):
        self.p = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _lib.check(_lib.lib().topo_amd_host_alloc(C.byref(self.p), n), "host_alloc")
        self.a = np.frombuffer((C.c_char * n).from_address(self.p.value), dtype=dtype).reshape(shape)

    def free(self):
        self.a = None
        _lib.check(_lib.lib().topo_amd_host_free(self.p), "host_free")


@pytest.mark.parametrize("sigma,ratio", [(0.75, 1), (12.0, 1), (3.25, 2)], ids=str)
def test_the_host_call_in_three_row_chunks(sigma, ratio, chunk_env):
    dem = orc.synthetic_dem(NY, NX, seed=31, integer=False)
    dem[SEAM - 2, :] = np.nan                          # a whole row just above the first seam
    dem[SEAM - 11: SEAM + 12, 60:150] = np.nan         # 23 rows across it
    dem[2 * SEAM - 4: 2 * SEAM + 5, 20:45] = np.nan    # a patch across the second seam
    res = gr.resolutions("1d", dem.shape)
    rx, ry = (np.ascontiguousarray(res[k], dtype=np.float64) for k in ("x", "y"))
    dev = d.DeviceArray.from_host(dem)
    try:
        want = run(d.Block(dev), sigma, ratio, res, 0.25, False)
    finally:
        dev.free()
    assert np.isnan(want[0]).sum() > NX
    lib = _lib.lib()
    for pinned in (False, True):
        pins = [Pinned(dem.shape) for _ in range(5)] if pinned else []
        try:
            src = pins[0].a if pinned else dem
            src[:] = dem
            outs = [p.a for p in pins[1:]] if pinned else [np.empty(dem.shape, dtype=np.float32) for _ in range(4)]
            for o in outs:
                o.view(np.uint8)[:] = 0xA5  # a row no download reaches would show
            raster = _lib.source_of(src)[1]
            raster.data = src.ctypes.data
            rc =lib.topo_amd_gradient_valid_raw(C.byref(raster), NY, NX, sigma, float(ratio), 0.25, 0, _lib.RES_1D, _lib.ptr(rx),
                                                 _lib.ptr(ry), *[_lib.ptr(o) for o in outs])
            assert rc == 0, (pinned, rc, lib.topo_amd_last_error())
            assert d.host_chunks() >= 3
            assert all(same_bits(a, b) for a, b in zip(outs, want)), pinned
        finally:
            for p in pins:
                p.free()


def test_an_int16_packed_dem_and_a_packed_slope_plane():
    dem = np.rint(dv.raster("whole"))
    with np.errstate(invalid="ignore"):
        raw = np.where(np.isfinite(dem) & (np.abs(dem) < 30000), dem, -32768).astype(np.int16)
    packed = tda.PackedDem(raw, fill_value=-32768)
    decoded = packed.decode()
    assert np.isnan(decoded).sum() == (raw == -32768).sum() > 1000
    res = gr.resolutions("s", dem.shape)
    part = d.DeviceArray.from_host(decoded)
    try:
        want = run(d.Block(part), 3.25, 1, res)
    finally:
        part.free()
    gr.check(want, gr.GradientValidReference(decoded, 3.25, res), "gradient_valid int16 source")
    assert all(same_bits(a, b) for a, b in zip(topo.gradient(packed, 3.25, res, skipna=True), want))
    slope_pack = tda.Packing(np.uint16, 0.01, 0.0, 65535)
    got = topo.gradient(packed, 3.25, res, skipna=True, pack={"slope": slope_pack})
    assert all(same_bits(got[k], want[k]) for k in (0, 1, 3))
    slope = got[2]
    code = _lib.encode_host(want[2], slope_pack)
    nan = np.isnan(want[2])
    assert isinstance(slope, _lib.PackedPlane) and same_bits(slope.values, code.values)
    assert np.array_equal(slope.values == slope_pack.fill_value, nan) and slope.missing == nan.sum() > 1000
    assert (slope.missing, slope.saturated) == (code.missing, code.saturated)


# ---- compute_gradient -------------------------------------------------------------------------------------------------------
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


def test_compute_gradient_with_skipna_a_crop_and_ind_nans():
    dem = dv.raster("frac")
    x = 2600000.0 + 30.0 * np.arange(dv.NX)
    y = 1200000.0 - 30.0 * np.arange(dv.GNY)
    ds = FakeDataset(dem, x, y)
    row0, rows, col0, cols = 9, 120, 13, 203
    crop = {"x": slice(x[col0] - 5.0, x[col0 + cols - 1] + 5.0), "y": slice(y[row0] + 1.0, y[row0 + rows - 1] - 1.0)}
    mask = np.zeros(dem.shape, dtype=bool)
    mask[40, 20:60] = True
    scales = [3 * 30, 21 * 30]  # sigma 0.75 (Sobel) and 5.25
    got = batch.compute_gradient(ds, scales, sig_ratios=[1, 2], ind_nans=mask, crop=crop, outdir=None, skipna=True, min_weight=0.25)
    assert list(got) == list(batch.compute_gradient(ds, scales, sig_ratios=[1, 2], crop=crop, outdir=None))
    res = {"x": 30.0, "y": -30.0}
    window = (slice(row0, row0 + rows), slice(col0, col0 + cols))
    names = iter(got)
    for px, ratio in zip((3, 21), (1, 2)):
        sigma = px / CFG.scale_std
        ref = gr.GradientValidReference(dem, sigma, res, ratio, 0.25)
        ref.planes = [np.where(mask, np.nan, p)[window] for p in ref.planes]
        ref.res = [r[window] for r in ref.res]
        ref.one_sided = [o[window] for o in ref.one_sided]
        ref.D = tuple(D[window] for D in ref.D)  # (the band next to a threshold, inside the window: its rim sees fewer neighbours, which only judges more)
        planes = [got[next(names)] for _ in range(4)]
        assert all(p.shape == (rows, cols) and np.isnan(p[mask[window]]).all() for p in planes)
        gr.check(planes, ref, f"compute_gradient skipna sigma {sigma} ratio {ratio}")
        full = run(d.Block(resident("frac")), sigma, ratio, res, 0.25)
        assert all(same_bits(p, np.where(mask, np.float32(np.nan), f)[window]) for p, f in zip(planes, full))
