"""The gradient (csrc/gradient.hip, ``launch_gradient``) on every kernel route, all four planes held to float64.

``launch_gradient`` picks Sobel / Chunked / Mfma / Valu / Aniso, under that a fused f16 kernel (4, 6 or 8 steps), the two-pass
tile kernels or the split-once axis 1 (NK 5 / 7 / 9), on the vector-ALU route the LDS-tiled axis-1 + epilogue kernel (tap
chunks of 8 or 16, PF 3 / 4 / 5), the wave-shift one or an unfused finish, and one of four stand-alone epilogues.  ``CASES``
names, for every case, the route ``device.gradient_route()`` must report (as recorded on an MI355X), so a retune that moves a
case to another kernel fails here instead of passing on that kernel.  Every case runs on

* a noisy raster: dx and dy against ``orc.gradient_exact`` at every pixel, with a per-pixel bound (``check_dx_dy``);
* two rasters of zeros with lines of height ``H`` on whole columns / whole rows: dx (dy) is then H (w[i+1] - w[i-1]) / (2 res),
  every tap of that axis on a pixel of its own, held to ``c * eps32 * H / |res|`` with the case's ``c`` (measured, doubled,
  capped so that one lost tap moves a pixel by twice the tolerance: ``tests/test_gradient_line_design.py``);
* (a route of each kind) a raster with a NaN, a +inf and a -inf sample;

and on every raster slope and aspect are compared with float64 evaluated on the float32 dx and dy THE CALL RETURNED, at
every pixel: that separates the epilogue's arithmetic from the smooth, so aspect needs no mask at small slopes.

The narrow-chunk PF 5 instance of the LDS-tiled kernel is not in the table: tap chunks of 8 end at radius 59, where the tile
has 247 columns (PF 4); PF 5 starts at 257."""
import functools

import numpy as np
import pytest

from oracle import topo_oracle as orc
from topo_descriptors_amd import _lib, device as d, topo

EPS32 = 2.0 ** -23
H = 1024.0                     # height of the lines
E_S = {"m": 1e-3, "mm": 2.0}   # the project's bound on the smoothed field (tests/test_gpu_parity.py): metres, millimetres
SLOPE_TOL = 8 * 2.0 ** -17     # degrees: 8 ulp of a float32 in [64, 128)
ASPECT_TOL = 4 * 2.0 ** -15    # degrees: 4 ulp of a float32 in [256, 512), as a wrapped difference
POISON = 0xA5A5A5A5

# ---- route codes (include/topo_amd.h, topo_amd_gradient_route) ----------------------------------------------------------
SOBEL, CHUNKED, MFMA, VALU, ANISO = range(5)
FUSED, TILE, SPLIT, VALU0 = 1, 2, 3, 4   # the smooth
MIXED = 1 << 6
TILED, WAVE, UNFUSED = 1, 2, 3           # the axis-1 finish of the Valu route
EPI1, EPI4, RERUN, TAPER = 1 << 18, 2 << 18, 1 << 20, 1 << 21


def smooth(kind, steps=0):
    return kind << 3 | steps << 7


def tiled(kb, pf):
    return TILED << 12 | (1 << 14 if kb == 16 else 0) | pf << 15


def chunks(n):
    return n << 22


def fields(route):
    """(route, smooth, steps, finish, kb16, pf, epilogue, rerun, taper, chunks)"""
    return (route & 7, route >> 3 & 7, route >> 7 & 31, route >> 12 & 3, route >> 14 & 1, route >> 15 & 7, route >> 18 & 3,
            route >> 20 & 1, route >> 21 & 1, route >> 22 & 127)


# name -> (raster kind, (ny, nx), sigma, sig_ratio, resolution mode, route, c of the line rasters)
# raster kind: "m" synthetic_dem in metres, "mm" the same x 1000 with resolutions x 1000 (a large-sample raster: the
# vector-ALU kernels), "block" the metre raster as a row block that carries only radius + 1 ghost rows.
# resolution mode: "s" scalar, "1d" uneven spacing with a negative y, "2d" varying per pixel (through topo.gradient).
# Radius int(4 sigma + 0.5): the smallest that reaches the route and, where the tile count changes with it, the largest.
CASES = {
    "sobel_s": ("m", (150, 170), 0.75, 1, "s", SOBEL, 2),
    "sobel_2d": ("m", (150, 170), 0.75, 1, "2d", SOBEL, 2),
    "fused4_r5": ("m", (230, 310), 1.25, 1, "s", MFMA | smooth(FUSED, 4) | EPI4, 2),
    "fused6_r20": ("m", (230, 310), 5.0, 1, "1d", MFMA | smooth(FUSED, 6) | EPI4, 2),
    "fused8_r33": ("m", (230, 310), 8.25, 1, "2d", MFMA | smooth(FUSED, 8) | EPI4, 2),
    "fused8_r47": ("m", (230, 310), 11.75, 1, "s", MFMA | smooth(FUSED, 8) | EPI4, 2),
    "tile_r48": ("m", (230, 310), 12.0, 1, "1d", MFMA | smooth(TILE, 8) | EPI4, 2),
    "split5_r49": ("m", (230, 310), 12.25, 1, "s", MFMA | smooth(SPLIT, 5) | EPI4, 2),
    "split7_r65": ("m", (230, 310), 16.25, 1, "1d", MFMA | smooth(SPLIT, 7) | EPI4, 2),
    "split9_r97": ("m", (330, 310), 24.25, 1, "s", MFMA | smooth(SPLIT, 9) | EPI4, 2),
    "chunk_fused": ("m", (2112, 96), 3.25, 1, "2d", CHUNKED | smooth(FUSED, 4) | EPI4 | RERUN | chunks(4), 2),
    "chunk_tile": ("m", (2112, 96), 12.0, 1, "1d", CHUNKED | smooth(TILE, 8) | EPI4 | chunks(3), 2),
    "taper_fused": ("m", (12288, 64), 3.25, 1, "s", CHUNKED | smooth(FUSED, 4) | EPI4 | RERUN | TAPER | chunks(6), 2),
    "taper_tile": ("m", (16384, 64), 12.0, 1, "s", CHUNKED | smooth(TILE, 8) | EPI4 | TAPER | chunks(4), 2),
    "valu_n3_r13": ("mm", (230, 310), 3.25, 1, "2d", VALU | smooth(VALU0) | tiled(8, 3), 2),
    "valu_n4_r32": ("mm", (230, 310), 8.0, 1, "s", VALU | smooth(VALU0) | tiled(8, 4), 2),
    "valu_w4_r60": ("mm", (230, 310), 15.0, 1, "1d", VALU | smooth(VALU0) | tiled(16, 4), 2),
    "valu_w5_r64": ("mm", (230, 310), 16.0, 1, "s", VALU | smooth(VALU0) | tiled(16, 5), 2),
    "valu_w5_r92": ("mm", (330, 310), 23.0, 1, "s", VALU | smooth(VALU0) | tiled(16, 5), 2),
    "wave_r93": ("mm", (330, 310), 23.25, 1, "2d", VALU | smooth(VALU0) | WAVE << 12, 2),
    "wave_r122": ("m", (330, 310), 30.5, 1, "1d", VALU | smooth(VALU0) | WAVE << 12, 2),
    "unfused_r177": ("m", (400, 330), 44.25, 1, "s", VALU | smooth(VALU0) | UNFUSED << 12 | EPI4, 2),
    "block_r13": ("block", (300, 310), 3.25, 1, "1d", VALU | smooth(VALU0) | tiled(8, 3), 2),
    "width_3": ("m", (150, 3), 3.25, 1, "s", VALU | smooth(VALU0) | tiled(8, 3), 2),
    "width_5": ("m", (150, 5), 3.25, 1, "2d", MFMA | smooth(FUSED, 4) | EPI1, 2),
    "width_8": ("m", (150, 8), 3.25, 1, "s", MFMA | smooth(FUSED, 4) | EPI4, 2),
    "width_9": ("m", (150, 9), 3.25, 1, "1d", MFMA | smooth(FUSED, 4) | EPI4, 2),
    "width_11": ("m", (150, 11), 3.25, 1, "s", MFMA | smooth(FUSED, 4) | EPI4, 2),
    "aniso_3_r2": ("m", (230, 310), 3.25, 2, "s", ANISO | smooth(TILE, 6) | MIXED | EPI4, 2),
    "aniso_3_r05": ("m", (230, 310), 3.25, 0.5, "1d", ANISO | smooth(VALU0) | EPI4, 2),
    "aniso_10_r2": ("m", (230, 310), 10.0, 2, "2d", ANISO | smooth(SPLIT, 7) | EPI4, 2),
    "aniso_10_r05": ("m", (230, 310), 10.0, 0.5, "s", ANISO | smooth(TILE, 6) | EPI4, 2),
}
# the cases that also run on the raster with a NaN, a +inf and a -inf sample
NON_FINITE = ("sobel_s", "fused4_r5", "fused8_r33", "tile_r48", "split5_r49", "chunk_fused", "chunk_tile", "valu_n3_r13")
BLOCK_OUT = (128, 228)  # "block": output rows [128, 228) of 300 with the fewest ghost rows the library takes, radius + 1
#                         (test_the_block_case_carries_the_fewest_ghost_rows): device rows [114, 242) at radius 13, so the
#                         accumulation-offset row 112 of the first 32-row tile is not in the block
# the first and the last cut between the row chunks of the chunked cases (csrc/gradient.hip, gradient_chunked; the route pins
# the number of chunks and the taper): chunks of 544 / 704 rows, tapered 512 + 4 x 2816 + 512 and 1024 + 2 x 7168 + 1024
CHUNK_CUTS = {"chunk_fused": (544, 1632), "chunk_tile": (704, 1408), "taper_fused": (512, 11776), "taper_tile": (1024, 15360)}


def radius(sigma, ratio=1):
    """The larger radius of the call's filters."""
    return int(4.0 * max(sigma, sigma * ratio) + 0.5)


def block_rows(name):
    """(first device row, end, first output row, end) of a "block" case."""
    _, _, sigma, ratio = CASES[name][:4]
    h = radius(sigma, ratio) + 1
    return BLOCK_OUT[0] - h, BLOCK_OUT[1] + h, BLOCK_OUT[0], BLOCK_OUT[1]


def line_cap(sigma, ratio=1):
    """The largest c that still notices one lost tap: the tap moves a pixel of dx by H w / (2 |res|) or more, the tolerance
    is c eps32 H / |res|, and twice the tolerance must fit below that.  The smallest tap of the call's filters (Aniso: of
    the wider one; Sobel: its smallest weight, 1/8)."""
    w_min = 0.125 if sigma <= 1 else float(orc.gaussian_weights(max(sigma, sigma * ratio))[0].min())
    return int(np.floor(w_min / (4 * EPS32)))


# ---- rasters and resolutions --------------------------------------------------------------------------------------------
def resolutions(mode, shape, scale):
    """Signed grid spacings, every value a float32 (the library takes scalars and vectors as float64 and rounds them)."""
    ny, nx = shape
    i, j = np.arange(nx), np.arange(ny)
    if mode == "s":
        return {"x": 25.0 * scale, "y": -25.0 * scale}
    if mode == "1d":
        return {"x": (20.0 + 0.25 * ((7 * i) % 41)) * scale, "y": -(18.0 + 0.5 * ((5 * j) % 29)) * scale}
    x = (20.0 + 0.25 * ((7 * i[None, :] + 3 * j[:, None]) % 41)) * scale
    y = -(18.0 + 0.5 * ((5 * j[:, None] + 11 * i[None, :]) % 29)) * scale
    return {"x": x.astype(np.float32), "y": y.astype(np.float32)}


def line_positions(n, R, wanted=()):
    """Up to three lines more than 2 R + 2 apart, at different phases of the 32- and 64-wide tiles: the first at ``wanted[0]``
    (37 by default), each further one at the next wanted position or, without one, right behind the last footprint, moved
    on until it is far enough and at a phase of its own."""
    pos = [wanted[0] if wanted else min(37, n // 2)]
    while len(pos) < 3:
        p = max(pos[-1] + 2 * R + 3, wanted[len(pos)] if len(pos) < len(wanted) else 0)
        while any(p % 32 == q % 32 or p % 64 == q % 64 for q in pos):
            p += 1
        if p >= n - 1:
            break
        pos.append(p)
    return pos


def row_lines(name):
    """The rows of the row-line raster.  A "block" case: one line in the ghost rows above the output rows, one in the middle
    of them (every tap on an output row), one in the ghost rows below.  A chunked case: one line in the first chunk, one
    three rows above its first cut and one two rows below its last cut, so that dy crosses a seam between two chunks'
    smooths and is taken inside the last chunk.  Any other: from row 37 on."""
    kind, (ny, _), sigma, ratio = CASES[name][:4]
    R = radius(sigma, ratio)
    if kind == "block":
        lo, hi, o0, o1 = block_rows(name)
        pos = line_positions(ny, R, (lo + 6, (o0 + o1) // 2, hi - 7))
        assert len(pos) == 3 and pos[2] < hi and o0 + R < pos[1] < o1 - R - 1
        return pos
    if name in CHUNK_CUTS:
        first, last = CHUNK_CUTS[name]
        pos = line_positions(ny, R, (37, first - 3, last + 2))
        assert len(pos) == 3 and first - R < pos[1] < first and last <= pos[2] < last + R
        return pos
    return line_positions(ny, R)


RASTERS = ("noise", "cols", "rows")


@functools.lru_cache(maxsize=None)
def case(name, raster):
    """(dem, resolutions, [dx, dy, slope, aspect] of orc.gradient_exact); computed once, read-only."""
    kind, shape, sigma, ratio, mode, _, _ = CASES[name]
    ny, nx = shape
    scale = 1000.0 if kind == "mm" else 1.0
    if raster in ("noise", "nonfinite"):
        dem = orc.synthetic_dem(ny, nx, seed=57, integer=False) * np.float32(scale)
        if raster == "nonfinite":
            dem[3, min(2, nx - 1)] = np.nan                       # near a corner
            dem[ny // 2, 64 if nx > 64 else nx // 2] = np.inf     # first column of a 32- and 64-column tile
            dem[3 * ny // 4, max(0, nx - 37)] = -np.inf
    else:
        dem = np.zeros(shape, np.float32)
        if raster == "cols":
            dem[:, line_positions(nx, radius(sigma, ratio))] = H
        else:
            dem[row_lines(name), :] = H
    res = resolutions(mode, shape, scale)
    with np.errstate(all="ignore"):
        want = orc.gradient_exact(dem, sigma, res, sig_ratio=ratio)
    dem.setflags(write=False)
    for w in want:
        w.setflags(write=False)
    return dem, res, want


# ---- device harness -----------------------------------------------------------------------------------------------------
def upload(a):
    dev = d.DeviceArray(*a.shape)
    dev.upload_rows(a)  # bit for bit
    return dev


def poisoned(rows, nx):
    out = d.DeviceArray(rows, nx)
    _lib.check(_lib.lib().topo_amd_memset(out.ptr, 0xA5, out.nbytes), "memset")
    return out


def block_gradient(blk, sigma, ratio, res, o0, rows, planes):
    """One ``launch_gradient`` on the resident block; per-pixel resolutions go in as device planes aligned with the output rows."""
    rx, ry = np.asarray(res["x"]), np.asarray(res["y"])
    if rx.ndim < 2:
        blk.gradient(sigma, rx, ry, sig_ratio=ratio, dx=planes[0], dy=planes[1], slope=planes[2], aspect=planes[3],
                     out_row0=o0, out_rows=rows)
        return
    dev_x, dev_y = upload(rx[o0:o0 + rows]), upload(ry[o0:o0 + rows])
    _lib.check(_lib.lib().topo_amd_gradient_dev(*blk._head(), float(sigma), float(ratio), _lib.RES_2D, dev_x.ptr, dev_y.ptr,
                                                o0, rows, *[p.ptr for p in planes]), "gradient_dev")
    d.sync()
    dev_x.free()
    dev_y.free()


def run_pieces(dem, pieces, sigma, ratio, res, large=False, repeat=1):
    """The gradient of ``dem`` from row blocks ``(first device row, end, first output row, end)``: ([4 planes] per repeat,
    routes).  ``large``: declare partial blocks as rows of a large-sample raster (what they are rows of in the millimetre cases)."""
    gny, nx = dem.shape
    runs, routes = [[[] for _ in range(4)] for _ in range(repeat)], []
    for lo, hi, o0, o1 in pieces:
        dev = upload(dem[lo:hi])
        blk = d.Block(dev, row0=lo, gny=gny)
        declared = large and (lo, hi) != (0, gny)
        if declared:
            _lib.check(_lib.lib().topo_amd_raster_class_set(dev.ptr, hi - lo, gny, nx, 1, 1.5e6, 3.0e6, 0.0), "raster_class_set")
        for rep in range(repeat):
            planes = [poisoned(o1 - o0, nx) for _ in range(4)]
            block_gradient(blk, sigma, ratio, res, o0, o1 - o0, planes)
            d.sync()
            routes.append(d.gradient_route())
            for k, p in enumerate(planes):
                runs[rep][k].append(p.to_host())
                p.free()
        if declared:
            d.forget_raster_class(blk)
        dev.free()
    return [[np.concatenate(p, axis=0) for p in run] for run in runs], routes


def pieces_of(name, raster):
    """(row blocks, first and last output row) of the case on that raster."""
    kind, (ny, nx), sigma, ratio, _, _, _ = CASES[name]
    if kind == "block":
        return [block_rows(name)], BLOCK_OUT[0], BLOCK_OUT[1]
    if kind == "mm" and raster in ("cols", "rows"):
        # zeros with lines are no large-sample raster by themselves: two row blocks with radius + 1 ghost rows, declared
        h, mid = radius(sigma, ratio) + 1, ny // 2
        return [(0, min(ny, mid + h), 0, mid), (max(0, mid - h), ny, mid, ny)], 0, ny
    return [(0, ny, 0, ny)], 0, ny


@functools.lru_cache(maxsize=None)
def gpu_call(name, raster):
    """([dx, dy, slope, aspect], routes) of the case: per-pixel resolutions through ``topo.gradient`` where the raster's
    class is its own, every other call through ``device.Block``."""
    kind, _, sigma, ratio, mode, _, _ = CASES[name]
    dem, res, _ = case(name, raster)
    pieces, o0, o1 = pieces_of(name, raster)
    if mode == "2d" and len(pieces) == 1 and kind != "block":
        got = topo.gradient(np.array(dem), sigma, res, sig_ratio=ratio)
        routes = [d.gradient_route()]
    else:
        (got,), routes = run_pieces(dem, pieces, sigma, ratio, res, large=kind == "mm")
    for g in got:
        g.setflags(write=False)
    return got, routes


# ---- the comparisons ----------------------------------------------------------------------------------------------------
def res_planes(res, shape):
    rx, ry = np.asarray(res["x"], np.float64), np.asarray(res["y"], np.float64)
    if ry.ndim == 1:
        ry = ry[:, None]
    return np.broadcast_to(rx, shape), np.broadcast_to(ry, shape)


def check_dx_dy(got, want, res, e_s, rows=None, padded=False):
    """dx and dy at every pixel where the oracle is finite: the result is finite there and |got - exact| <= k E_s / |res| +
    4 eps32 |exact|, k = 1 for a central difference and 2 on the first / last column (dx) or row (dy).  Returns the largest
    error / bound.  ``padded``: the vector-ALU kernels on a raster with non-finite samples, whose tap-chunk padding may
    spread the oracle's non-finite pixels by up to 8 (tests/test_gpu_parity.py, test_gaussian_nan_footprint): those pixels,
    and no others, may be non-finite and are then not compared.  Where the oracle is not finite: the caller's masks."""
    from scipy import ndimage
    shape = want[0].shape
    rx, ry = res_planes(res, shape)
    worst = 0.0
    for k, r in ((0, rx), (1, ry)):
        kk = np.ones(shape)
        if k == 0:
            kk[:, [0, -1]] = 2.0
        else:
            kk[[0, -1], :] = 2.0
        sl = slice(None) if rows is None else slice(*rows)
        g, w = got[k].astype(np.float64), want[k][sl]
        ok = np.isfinite(w)
        if padded:
            ok &= np.isfinite(g) | ~ndimage.binary_dilation(~np.isfinite(w), structure=np.ones((17, 17), bool))
        lost = ok & ~np.isfinite(g)
        assert not lost.any(), f"plane {k}: not finite at {int(lost.sum())} pixels where the oracle is, first {np.argwhere(lost)[0]}"
        bound = (kk * e_s / np.abs(r))[sl] + 4 * EPS32 * np.abs(w)
        with np.errstate(invalid="ignore"):  # (inf - inf where both are infinite: not among the pixels compared)
            ratio = np.abs(g - w)[ok] / bound[ok]
        worst = max(worst, float(ratio.max()))
    return worst


def check_slope_aspect(got):
    """Slope and aspect against float64 on the float32 dx and dy of the same call, at every pixel, signed zeros, infinite and
    NaN gradients included.  Returns (largest slope error, largest wrapped aspect error) in degrees."""
    dx, dy = got[0].astype(np.float64), got[1].astype(np.float64)
    with np.errstate(all="ignore"):
        slope = np.degrees(np.arctan(np.hypot(dx, dy)))
        aspect = (180.0 + np.degrees(np.arctan2(dx, dy))) % 360.0
    for k, ref in ((2, slope), (3, aspect)):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref)), \
            f"plane {k}: NaN at {int((np.isnan(got[k]) != np.isnan(ref)).sum())} pixels where the other has none"
    ok = ~np.isnan(aspect)
    assert np.all((got[3][ok] >= 0) & (got[3][ok] < 360))
    es = np.abs(got[2].astype(np.float64) - slope)
    ea = orc.wrapped_angle_diff(got[3][ok], aspect[ok])
    return float(np.nanmax(es)) if es.size else 0.0, float(ea.max()) if ea.size else 0.0


def line_units(got, want, res, rows=None):
    """Largest |got - exact| of dx and dy in units of eps32 H / |res|."""
    shape = want[0].shape
    sl = slice(None) if rows is None else slice(*rows)
    worst = 0.0
    for k, r in zip((0, 1), res_planes(res, shape)):
        e = np.abs(np.asarray(got[k], np.float64) - want[k][sl]) * np.abs(r)[sl] / (EPS32 * H)
        worst = max(worst, float(e.max()) if np.all(np.isfinite(e)) else np.inf)
    return worst


def e_s_of(name, raster):
    """The bound on the smoothed field: the project's for the raster kind; Sobel has no smooth: one float32 ulp of the raster's
    largest finite sample."""
    kind, _, sigma = CASES[name][:3]
    dem = case(name, raster)[0]
    return float(np.spacing(np.float32(np.abs(dem[np.isfinite(dem)]).max()))) if sigma <= 1 else E_S["mm" if kind == "mm" else "m"]


def no_poison(got):
    return not any((np.ascontiguousarray(g).view(np.uint32) == POISON).any() for g in got)


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("raster", RASTERS)
@pytest.mark.parametrize("name", list(CASES))
def test_route_and_oracle(name, raster):
    kind, shape, sigma, ratio, mode, route, c = CASES[name]
    _, res, want = case(name, raster)
    got, routes = gpu_call(name, raster)
    _, o0, o1 = pieces_of(name, raster)
    rows = None if (o0, o1) == (0, shape[0]) else (o0, o1)
    worst = check_dx_dy(got, want, res, e_s_of(name, raster), rows)
    units = line_units(got, want, res, rows) if raster != "noise" else 0.0
    print(f"{name} {raster}: routes {routes} {[fields(r) for r in routes]}, dx dy err / bound {worst:.3f}, "
          f"line units {units:.3f} (c {c}, cap {line_cap(sigma, ratio)})")
    if raster != "noise":  # the lines show in the rows that are compared: dx of the column lines, dy of the row lines
        shown = want[0 if raster == "cols" else 1][slice(o0, o1)]
        n_shown = np.count_nonzero(np.any(shown != 0, axis=1 if raster == "rows" else 0))
        assert n_shown >= min(radius(sigma), shown.shape[0 if raster == "rows" else 1] - 1), (name, raster, n_shown)
    assert all(r == route for r in routes), (name, routes, [fields(r) for r in routes], fields(route))
    assert no_poison(got)
    assert worst <= 1.0
    if raster != "noise":
        assert units <= c, (name, raster, units)
    es, ea = check_slope_aspect(got)
    print(f"{name} {raster}: slope err {es:.3e} (tol {SLOPE_TOL:.3e}), aspect err {ea:.3e} (tol {ASPECT_TOL:.3e})")
    assert es <= SLOPE_TOL and ea <= ASPECT_TOL


def test_the_cases_cover_every_route():
    f = [fields(CASES[n][5]) for n in CASES]
    assert {x[0] for x in f} == {SOBEL, CHUNKED, MFMA, VALU, ANISO}
    assert {x[1] for x in f} == {0, FUSED, TILE, SPLIT, VALU0}
    assert {x[2] for x in f if x[1] == FUSED} == {4, 6, 8} and {x[2] for x in f if x[1] == SPLIT} == {5, 7, 9}
    assert {x[3] for x in f} == {0, TILED, WAVE, UNFUSED}
    assert {(x[4], x[5]) for x in f if x[3] == TILED} == {(0, 3), (0, 4), (1, 4), (1, 5)}
    assert {x[6] for x in f} == {0, 1, 2} and {x[7] for x in f} == {0, 1} and {x[8] for x in f} == {0, 1}
    assert {x[8] for x in f if x[0] == CHUNKED and x[1] == FUSED} == {0, 1} == {x[8] for x in f if x[0] == CHUNKED and x[1] == TILE}
    assert any(CASES[n][5] & MIXED for n in CASES)
    # per-pixel resolutions on every kind of epilogue: Sobel, 1-wide, 4-wide, _if, LDS-tiled, wave-shift, several chunks
    two_d = [fields(CASES[n][5]) for n in CASES if CASES[n][4] == "2d"]
    assert any(x[0] == SOBEL for x in two_d) and {x[6] for x in two_d} >= {1, 2} and any(x[7] for x in two_d)
    assert {x[3] for x in two_d} >= {TILED, WAVE} and any(x[9] > 1 for x in two_d) and any(x[0] == ANISO for x in two_d)
    assert {CASES[n][4] for n in CASES} == {"s", "1d", "2d"}
    for n in NON_FINITE:
        assert n in CASES
    assert {fields(CASES[n][5])[:2] for n in NON_FINITE} >= {(SOBEL, 0), (MFMA, FUSED), (MFMA, TILE), (MFMA, SPLIT), (CHUNKED, FUSED),
                                                             (CHUNKED, TILE), (VALU, VALU0)}


def test_every_c_is_within_its_cap():
    for n, (_, _, sigma, ratio, _, _, c) in CASES.items():
        assert 2 <= c <= line_cap(sigma, ratio), (n, c, line_cap(sigma, ratio))


@gpu
@pytest.mark.parametrize("name", NON_FINITE)
def test_non_finite_samples(name):
    """A NaN, a +inf and a -inf sample.  Matrix-core routes and Sobel: the NaN / +inf / -inf masks of dx and dy are the
    oracle's.  Vector-ALU route: no pixel finite where the oracle is not, the extra footprint within the tap-chunk padding
    (test_gaussian_nan_footprint).  Infinite gradients: dx, dy +-inf, slope 90, aspect numpy's, through check_slope_aspect."""
    from scipy import ndimage
    kind, shape, sigma, ratio, mode, route, _ = CASES[name]
    _, res, want = case(name, "nonfinite")
    got, routes = gpu_call(name, "nonfinite")
    print(f"{name} nonfinite: routes {routes} {[fields(r) for r in routes]}")
    assert all(r == route for r in routes), (name, routes)
    if fields(route)[:2] == (CHUNKED, FUSED):
        assert route & RERUN  # the two passes and an _if epilogue are queued behind the chunks
    assert no_poison(got)
    assert np.isinf(want[0]).any() and np.isinf(want[1]).any() and np.isnan(want[0]).any()
    for k in (0, 1):
        if kind == "mm":
            bad_ref, bad = ~np.isfinite(want[k]), ~np.isfinite(got[k])
            assert not np.any(bad_ref & ~bad)
            assert not np.any(bad & ~ndimage.binary_dilation(bad_ref, structure=np.ones((17, 17), bool)))
        else:
            for what, mask in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
                diff = mask(got[k]) != mask(want[k])
                assert not diff.any(), f"plane {k}: {what} at {int(diff.sum())} pixels where the other has none"
    worst = check_dx_dy(got, want, res, e_s_of(name, "nonfinite"), padded=kind == "mm")
    es, ea = check_slope_aspect(got)
    print(f"{name} nonfinite: dx dy err / bound {worst:.3f}, slope err {es:.3e}, aspect err {ea:.3e}")
    assert worst <= 1.0 and es <= SLOPE_TOL and ea <= ASPECT_TOL
    assert np.isinf(got[0]).any() and np.isinf(got[1]).any()  # infinite gradients did come back (slope 90: check_slope_aspect)


@gpu
def test_second_call_on_a_wild_raster_goes_straight_to_the_two_passes():
    """The fused kernel notes on the resident raster that it met a sample that is not a plain finite one (dem_memo_wild): the
    next call skips it.  Another route, the same bits."""
    name = "fused4_r5"
    _, _, sigma, ratio, _, route, _ = CASES[name]
    dem, res, _ = case(name, "nonfinite")
    (first, second), routes = run_pieces(dem, [(0, dem.shape[0], 0, dem.shape[0])], sigma, ratio, res, repeat=2)
    print(f"routes {routes} {[fields(r) for r in routes]}")
    assert routes[0] == route and routes[1] == MFMA | smooth(TILE, 4) | EPI4
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
def test_the_block_case_carries_the_fewest_ghost_rows():
    """radius + 1 ghost rows are the fewest a gradient block may come with (gradient_ghost_rows, least): with one fewer,
    above or below, the library refuses the call before it launches anything."""
    name = "block_r13"
    _, _, sigma, ratio = CASES[name][:4]
    dem, res, _ = case(name, "noise")
    lo, hi, o0, o1 = block_rows(name)
    assert (o0 - lo, hi - o1) == (radius(sigma, ratio) + 1,) * 2
    for pieces in ([(lo + 1, hi, o0, o1)], [(lo, hi - 1, o0, o1)]):
        with pytest.raises(_lib.TopoAmdError):
            run_pieces(dem, pieces, sigma, ratio, res)
