"""Sx (csrc/sx.hip) on every kernel route, each against the float64 oracle.

``launch_sx`` picks a scan (chains down the columns, along the rows, along either diagonal, or the kernel without an LDS
tile), 4 or 8 waves, one of 16 LDS strides and up to six chain tables from the sector's offset table.  ``SECTORS`` names,
for every sector, the route ``device.sx_route()`` must report, so a retune that moves a sector to another kernel fails
here instead of passing on that kernel.  Every sector runs on a noisy raster, on an impulse raster on which every ray
pixel decides exactly one output pixel, and on two rasters with non-finite samples; the reference is
``orc.sx_rolling`` fed with the very offset table the kernel gets.  ``tests/test_sx_impulse_design.py`` shows on the oracle
alone that the impulse comparison notices any single lost ray pixel."""
import functools

import numpy as np
import pytest

from oracle import topo_oracle as orc
from topo_descriptors_amd import _lib, device as d, shard

REL = 1e-4      # the project's contract for Sx (tests/test_gpu_parity.py)
HEIGHT = 10.0
SPIKE = 1000.0  # metres, far above HEIGHT: one spike in a window of zeros is the only positive tangent
POISON = 0xA5A5A5A5
SNAN_BITS = 0x7FA00000

# route codes (include/topo_amd.h, topo_amd_sx_route)
COLUMNS, ROWS, DIAG_PLUS, DIAG_MINUS, GLOBAL = range(5)
WAVES8, T8, T4, T2, P8, P4, P2, GROUPED = 8, 16, 32, 64, 128, 256, 512, 16384


def stride(index):
    return index << 10


# (azimuth, radius, dx, dy, azimuth_arc, azimuth_steps, radius_min), raster (ny, nx), the route of Block.sx, the route of
# Block.sx_multi over [the same sector 5 degrees further, the sector] (None: not run).  Routes as reported on an MI355X.
SECTORS = {
    "north_500": ((0.0, 500.0, 30.0, -30.0, 10.0, 15, 0.0), (200, 230),
                  COLUMNS + T8 + P8 + stride(0), GROUPED + COLUMNS + T8 + T4 + T2 + stride(1)),
    "east_500": ((90.0, 500.0, 30.0, -30.0, 10.0, 15, 0.0), (200, 230),
                 ROWS + T8 + P8 + stride(3), GROUPED + ROWS + T8 + T4 + T2 + stride(0)),
    "north_east_1500": ((45.0, 1500.0, 30.0, -30.0, 10.0, 15, 0.0), (300, 310),
                        DIAG_MINUS + T8 + T2 + P8 + P4 + P2 + stride(8), GROUPED + ROWS + T8 + T4 + T2 + stride(2)),
    "south_east_2000": ((135.0, 2000.0, 30.0, -30.0, 10.0, 15, 0.0), (400, 390),
                        DIAG_PLUS + T8 + T4 + T2 + P8 + P4 + P2 + stride(8), GROUPED + COLUMNS + T8 + T4 + T2 + stride(8)),
    "north_2000": ((0.0, 2000.0, 30.0, -30.0, 10.0, 15, 0.0), (400, 390),
                   COLUMNS + WAVES8 + T8 + T2 + P8 + P4 + P2 + stride(3), None),
    "one_ray_300": ((20.0, 300.0, 30.0, -30.0, 0.0, 15, 0.0), (150, 170),
                    COLUMNS + T4 + T2 + stride(0), None),
    "radius_min_1000": ((200.0, 1000.0, 30.0, -30.0, 10.0, 15, 400.0), (250, 270),
                        COLUMNS + T8 + T4 + T2 + stride(3), None),
    "grid_25x40_600": ((70.0, 600.0, 25.0, -40.0, 10.0, 15, 0.0), (200, 230),
                       ROWS + T8 + T4 + T2 + stride(4), None),
    "window_beyond_lds": ((45.0, 5500.0, 30.0, -30.0, 4.0, 2, 0.0), (400, 398),  # (two rays: the impulse raster
                          # can decide one offset per interior pixel, and the interior is 32 x 30)
                          GLOBAL, GLOBAL),
}
# one sector per scan, and the kernel without a tile: sx_multi and row blocks against the single call
PER_SCAN = ("north_500", "east_500", "north_east_1500", "south_east_2000", "window_beyond_lds")


@functools.lru_cache(maxsize=None)
def sector(name):
    """(window, dj, di, dist) as ``device.sx_offsets`` returns it."""
    az, radius, dx, dy, arc, steps, rmin = SECTORS[name][0]
    return d.sx_offsets(az, radius, dx, dy, azimuth_arc=arc, azimuth_steps=steps, radius_min=rmin)


def neighbour(name):
    """The same sector 5 degrees further: what sx_multi groups with it (when their common tile is small enough)."""
    az, radius, dx, dy, arc, steps, rmin = SECTORS[name][0]
    return d.sx_offsets(az + 5.0, radius, dx, dy, azimuth_arc=arc, azimuth_steps=steps, radius_min=rmin)


def unique_offsets(sec):
    """The unique (dj, di) with a finite distance, as an (n, 2) array."""
    _, dj, di, dist = sec
    ok = ~np.isnan(dist)
    return np.unique(np.stack([np.asarray(dj)[ok], np.asarray(di)[ok]], axis=1), axis=0)


# ---- rasters ----------------------------------------------------------------------------------------------------------
def noisy_raster(ny, nx):
    return orc.synthetic_dem(ny, nx, seed=41, integer=False)


def impulse_spikes(ny, nx, window, offs):
    """Spike positions on the ny x nx raster such that no output pixel inside the frame sees two spikes, and every unique
    offset puts at least one ``spike - offset`` inside the frame.  A raster whose interior holds the offsets' bounding box
    gets spikes in the interior, on both sides of a 64-pixel tile border in x and in y, and on the last interior column
    and row (next to the zero frame on the right and at the bottom); a smaller interior (the window beyond the LDS tile)
    gets, offset by offset, a spike that puts ``spike - offset`` on a free interior pixel."""
    y0, y1, x0, x1 = window, ny - window, window, nx - window
    claimed = np.zeros((ny, nx), bool)
    covered = np.zeros(len(offs), bool)
    spikes = []

    def take(s):
        t = np.asarray(s) - offs
        inside = (t[:, 0] >= y0) & (t[:, 0] < y1) & (t[:, 1] >= x0) & (t[:, 1] < x1)
        if not (0 <= s[0] < ny and 0 <= s[1] < nx) or claimed[t[inside, 0], t[inside, 1]].any():
            return False
        claimed[t[inside, 0], t[inside, 1]] = True
        covered[inside] = True
        spikes.append((int(s[0]), int(s[1])))
        return True

    def first_of(candidates, what):
        assert any(take(s) for s in candidates), f"no room for the spike {what}"

    ext_j = offs[:, 0].max() - offs[:, 0].min() + 1
    ext_i = offs[:, 1].max() - offs[:, 1].min() + 1
    if y1 - y0 > 2 * ext_j and x1 - x0 > 2 * ext_i:
        # a spike all of whose targets lie inside the frame
        cj, ci = (y0 + y1) // 2 + offs[:, 0].max(), (x0 + x1) // 2 + offs[:, 1].max()
        first_of([(cj, ci)], "in the interior")
        assert covered.all()
        by = [b for b in range(64, ny, 64) if y0 + 2 <= b < y1 - 2]
        bx = [b for b in range(64, nx, 64) if x0 + 2 <= b < x1 - 2]
        cols = range(x0 + 1, x1 - 1, 3)
        rows = range(y0 + 1, y1 - 1, 3)
        first_of([(b - 1, c) for b in by for c in cols], "above a tile border")
        first_of([(b, c) for b in by for c in cols], "below a tile border")
        first_of([(r, b - 1) for b in bx for r in rows], "left of a tile border")
        first_of([(r, b) for b in bx for r in rows], "right of a tile border")
        first_of([(r, x1 - 1) for r in rows], "next to the frame on the right")
        first_of([(y1 - 1, c) for c in cols], "next to the frame at the bottom")
    else:
        # (at most one offset per target can be decided: the sector must have fewer unique offsets than the interior pixels)
        targets = sorted(((j, i) for j in range(y0, y1) for i in range(x0, x1)),
                         key=lambda t: (2 * t[0] - y0 - y1 + 1) ** 2 + (2 * t[1] - x0 - x1 + 1) ** 2)  # (centre first)
        for k in range(len(offs)):
            if not covered[k]:
                first_of(((t[0] + offs[k, 0], t[1] + offs[k, 1]) for t in targets if not claimed[t]), f"for offset {offs[k]}")
    assert covered.all(), "an offset decides no pixel inside the frame"
    return spikes


def impulse_raster(ny, nx, spikes):
    dem = np.zeros((ny, nx), np.float32)
    for j, i in spikes:
        dem[j, i] = SPIKE
    return dem


def tile_corner(ny, nx):
    """The corner of four 64 x 64 tiles nearest the raster's centre."""
    return 64 * max(1, round(ny / 128)), 64 * max(1, round(nx / 128))


def nan_raster(ny, nx, window, offs):
    """Noisy terrain with a single NaN (a target pixel too), NaNs on the four sides of a tile corner, a NaN run across
    several tiles, and a NaN block that holds every ray pixel of one target (and so of a few more)."""
    dem = noisy_raster(ny, nx)
    cy, cx = tile_corner(ny, nx)
    dem[window + 5, window + 7] = np.nan
    dem[cy - 1:cy + 1, cx - 1:cx + 1] = np.nan
    dem[cy + 20, max(0, cx - 70):cx + 75] = np.nan
    tj, ti = ny - window - 4, nx - window - 5
    dem[tj + offs[:, 0].min():tj + offs[:, 0].max() + 1, ti + offs[:, 1].min():ti + offs[:, 1].max() + 1] = np.nan
    return dem


def snan_position(dem, window, offs, dist_of):
    """Where a signalling NaN tests the most: ``sx_kernel`` scans two chains of equal weights as one, on the larger of the two
    SAMPLES, and a maximum that turned a signalling NaN into a quiet one instead of dropping it would lose the other sample.
    So the NaN goes where that other sample matters: the first target near the tile corner whose horizon is a ray pixel
    with a twin (another offset at the same distance: the other side of the sector) and stands at least 0.05 degrees above
    the rest of the window is looked up, and the NaN takes the twin's place in that target's window.  Returns (position,
    number of targets for which the NaN's twin is such a horizon); a sector without twins gets a fixed position and 0."""
    ny, nx = dem.shape
    cy, cx = tile_corner(ny, nx)
    inv = np.array([np.float32(1.0 / dist_of[tuple(o)]) for o in offs])
    z = dem.astype(np.float64)

    def horizon(tj, ti, skip=None):
        """(index of the horizon's offset, degrees it stands above the rest without it and its twins) at target (tj, ti)"""
        tan = (z[tj + offs[:, 0], ti + offs[:, 1]] - z[tj, ti] - HEIGHT) * inv
        if skip is not None:
            tan[skip] = -np.inf
        top = int(np.argmax(tan))
        rest = tan[inv != inv[top]]
        return top, (np.rad2deg(np.arctan(tan[top]) - np.arctan(rest.max())) if rest.size else 90.0)

    def inside(tj, ti):
        return window <= tj < ny - window and window <= ti < nx - window

    spot = (cy - 5, cx - 30)
    for tj in range(max(window, cy - 20), min(ny - window, cy + 40)):
        for ti in range(max(window, cx - 40), min(nx - window, cx - 10)):
            top, above = horizon(tj, ti)
            twins = np.flatnonzero((inv == inv[top]) & (np.arange(len(offs)) != top))
            if twins.size and above > 0.05:
                spot = (tj + int(offs[twins[0], 0]), ti + int(offs[twins[0], 1]))
                break
        else:
            continue
        break
    n = 0
    for k, o in enumerate(offs):
        tj, ti = spot[0] - o[0], spot[1] - o[1]
        if inside(tj, ti):
            top, above = horizon(tj, ti, skip=k)
            n += int(top != k and inv[top] == inv[k] and above > 0.05)
    return spot, n


@functools.lru_cache(maxsize=None)
def snan_spot(name):
    """``snan_position`` on the sector's noisy raster."""
    window, dj, di, dist = sector(name)
    dist_of = {(int(a), int(b)): float(c) for a, b, c in zip(dj, di, dist) if not np.isnan(c)}
    return snan_position(noisy_raster(*SECTORS[name][1]), window, unique_offsets(sector(name)), dist_of)


def inf_raster(name):
    """Noisy terrain with +inf, -inf (one pixel: every window that holds it holds finite samples too, unless the sector has
    a single ray pixel) and one signalling NaN."""
    ny, nx = SECTORS[name][1]
    dem = noisy_raster(ny, nx)
    cy, cx = tile_corner(ny, nx)
    (sj, si), _ = snan_spot(name)
    dem[cy - 9, cx + 11] = np.inf
    dem[cy + 17, cx + 3] = -np.inf
    dem.view(np.uint32)[sj, si] = SNAN_BITS
    return dem


RASTERS = ("noisy", "impulse", "nan", "inf")


@functools.lru_cache(maxsize=None)
def case(name, raster):
    """(dem, reference, spikes) of one sector on one raster; computed once, read-only."""
    ny, nx = SECTORS[name][1]
    window, dj, di, dist = sector(name)
    assert ny > 2 * window + 8 and nx > 2 * window + 8 and nx % 64 != 0
    offs = unique_offsets(sector(name))
    spikes = ()
    if raster == "noisy":
        dem = noisy_raster(ny, nx)
    elif raster == "impulse":
        spikes = tuple(impulse_spikes(ny, nx, window, offs))
        dem = impulse_raster(ny, nx, spikes)
    elif raster == "nan":
        dem = nan_raster(ny, nx, window, offs)
    else:
        dem = inf_raster(name)
    with np.errstate(all="ignore"):
        want = orc.sx_rolling(dem, window, np.stack([dj, di], axis=1), dist, HEIGHT)
    dem.setflags(write=False)
    want.setflags(write=False)
    return dem, want, spikes


# ---- the comparison ---------------------------------------------------------------------------------------------------
def mismatches(got, want, window, spikes=(), offs=None):
    """What is wrong with ``got`` (empty: nothing): poison left, a frame that is not 0, NaNs elsewhere than the
    reference's, more than REL of the reference's largest value anywhere or, on an impulse raster, at any
    ``spike - offset``."""
    ny, nx = want.shape
    bad = []
    if (np.ascontiguousarray(got).view(np.uint32) == POISON).any():
        bad.append("pixels not written")
    frame = np.ones((ny, nx), bool)
    frame[window:ny - window, window:nx - window] = False
    if not np.array_equal(got[frame] == 0, want[frame] == 0):
        bad.append("zero frame")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        bad.append(f"NaN at {int((np.isnan(got) != np.isnan(want)).sum())} pixels where the other has none")
    ok = ~np.isnan(want) & ~np.isnan(got)
    bound = REL * float(np.max(np.abs(want[~np.isnan(want)])))
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    if err.size and err.max() > bound:
        bad.append(f"max|got - want| {err.max():.3e} > {bound:.3e} at {int((err > bound).sum())} pixels")
    for s in spikes:
        t = np.asarray(s) - offs
        t = t[(t[:, 0] >= window) & (t[:, 0] < ny - window) & (t[:, 1] >= window) & (t[:, 1] < nx - window)]
        e = np.abs(got[t[:, 0], t[:, 1]].astype(np.float64) - want[t[:, 0], t[:, 1]].astype(np.float64))
        if not (e <= bound).all():  # (a NaN fails too)
            bad.append(f"spike {s}: {int((~(e <= bound)).sum())} of its {len(t)} pixels")
    return bad


# ---- device harness ---------------------------------------------------------------------------------------------------
def upload(dem):
    """Bit for bit (a signalling NaN stays one)."""
    dev = d.DeviceArray(*dem.shape)
    dev.upload_rows(dem)
    return dev


def poisoned(rows, nx):
    out = d.DeviceArray(rows, nx)
    _lib.check(_lib.lib().topo_amd_memset(out.ptr, 0xA5, out.nbytes), "memset")
    return out


def run_single(blk, sec, rows, nx, **kw):
    window, dj, di, dist = sec
    out = poisoned(rows, nx)
    blk.sx(dj, di, dist, window, HEIGHT, out, **kw)
    d.sync()
    route = d.sx_route()
    got = out.to_host()
    out.free()
    return got, route


def run_multi(blk, sectors, rows, nx, **kw):
    outs = [poisoned(rows, nx) for _ in sectors]
    blk.sx_multi(sectors, HEIGHT, outs, **kw)
    d.sync()
    route = d.sx_route()
    planes = [o.to_host() for o in outs]
    for o in outs:
        o.free()
    return planes, route


@functools.lru_cache(maxsize=None)
def single_call(name, raster):
    """(plane, route) of Block.sx on the whole raster."""
    dem, _, _ = case(name, raster)
    dev = upload(dem)
    got, route = run_single(d.Block(dev), sector(name), *dem.shape)
    dev.free()
    got.setflags(write=False)
    return got, route


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("raster", RASTERS)
@pytest.mark.parametrize("name", list(SECTORS))
def test_route_and_oracle(name, raster):
    dem, want, spikes = case(name, raster)
    window = sector(name)[0]
    offs = unique_offsets(sector(name))
    if raster == "nan":  # the raster holds what it is meant to hold: targets with a sample of their own and no usable ray pixel
        assert (np.isnan(want) & ~np.isnan(dem)).any() and np.isnan(want[window + 5, window + 7])
        assert (~np.isnan(want)).sum() > want.size // 4
    if raster == "inf" and SECTORS[name][2] & (P8 + P4 + P2):  # the signalling NaN sits where losing a pair's other sample shows
        assert snan_spot(name)[1] > 0
    got, route = single_call(name, raster)
    print(f"{name} {raster}: route {route}, max|got - want| "
          f"{np.nanmax(np.abs(got.astype(np.float64) - want)):.3e}, bound {REL * np.nanmax(np.abs(want)):.3e}")
    assert route == SECTORS[name][2], (name, route)
    assert mismatches(got, want, window, spikes, offs) == []


def test_the_sectors_cover_every_route():
    routes = [SECTORS[n][2] for n in SECTORS]
    assert {r & 7 for r in routes} == {COLUMNS, ROWS, DIAG_PLUS, DIAG_MINUS, GLOBAL}
    assert any(r & WAVES8 for r in routes)
    for table in (T8, T4, T2, P8, P4, P2):
        assert any(r & table for r in routes if r & 7 != GLOBAL), table
    assert len({r >> 10 & 15 for r in routes if r & 7 != GLOBAL}) >= 3
    assert any((SECTORS[n][3] or 0) & GROUPED for n in PER_SCAN)


@gpu
@pytest.mark.parametrize("raster", ("impulse", "nan", "inf"))
@pytest.mark.parametrize("name", PER_SCAN)
def test_sx_multi_has_the_bits_of_the_single_call(name, raster):
    dem, _, _ = case(name, raster)
    want, _ = single_call(name, raster)
    dev = upload(dem)
    planes, route = run_multi(d.Block(dev), [neighbour(name), sector(name)], *dem.shape)
    dev.free()
    print(f"{name} {raster}: sx_multi route {route}")
    assert route == SECTORS[name][3], (name, route)
    assert np.array_equal(planes[1].view(np.uint32), want.view(np.uint32))
    assert not (planes[0].view(np.uint32) == POISON).any()


@gpu
@pytest.mark.parametrize("raster", ("impulse", "nan", "inf"))
@pytest.mark.parametrize("name", PER_SCAN)
def test_row_blocks_have_the_bits_of_the_whole_block(name, raster):
    dem, _, _ = case(name, raster)
    gny, nx = dem.shape
    sectors = [neighbour(name), sector(name)]
    up, down = shard.sx_multi_halo(sectors)
    dev = upload(dem)
    whole, _ = run_multi(d.Block(dev), sectors, gny, nx)
    dev.free()
    assert np.array_equal(whole[1].view(np.uint32), single_call(name, raster)[0].view(np.uint32))
    for nb in (2, 3):
        pieces = [[] for _ in sectors]
        for row0, rows in shard.split_rows(gny, nb):
            lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
            part = upload(dem[lo:hi])
            got, _ = run_multi(d.Block(part, row0=lo, gny=gny), sectors, rows, nx, out_row0=row0, out_rows=rows)
            for p, g in zip(pieces, got):
                p.append(g)
            part.free()
        for w, p in zip(whole, pieces):
            assert np.array_equal(w.view(np.uint32), np.concatenate(p, axis=0).view(np.uint32)), nb


@gpu
@pytest.mark.parametrize("raster", ("impulse", "nan", "inf"))
@pytest.mark.parametrize("name", PER_SCAN)
def test_single_call_on_row_blocks_has_the_bits_of_the_whole_block(name, raster):
    """``Block.sx`` itself on 2 and 3 row blocks with ghost rows: the sector's own scan (diagonals and pairs included) with
    ``in_row0`` != 0 and tiles that reach beyond the block's rows."""
    dem, _, _ = case(name, raster)
    gny, nx = dem.shape
    whole, route = single_call(name, raster)
    up, down = shard.sx_multi_halo([sector(name)])
    for nb in (2, 3):
        pieces = []
        for row0, rows in shard.split_rows(gny, nb):
            lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
            part = upload(dem[lo:hi])
            got, r = run_single(d.Block(part, row0=lo, gny=gny), sector(name), rows, nx, out_row0=row0, out_rows=rows)
            part.free()
            assert r & 7 == route & 7, (nb, row0, r)  # (a short block may take 4 waves where the whole one takes 8)
            pieces.append(got)
        assert np.array_equal(whole.view(np.uint32), np.concatenate(pieces, axis=0).view(np.uint32)), nb
