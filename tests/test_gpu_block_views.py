"""Row blocks as overlapping views of ONE device buffer (include/topo_amd.h, "what kernel routing may know about a
raster"): an application that holds a raster in one resident DeviceArray cuts it into Block views, each with exactly
the ghost rows shard.halo_rows asks for, adds the rows each view owns to one RasterScan and declares the class for every
view.  The views overlap, so each declaration overlaps its neighbours' - every view must still find the class.

Each case checks three things of the views, called in declaration order and in reverse and stitched:
  (a) the bits (NaN included) of the call on the whole buffer as one Block;
  (b) the float64 oracle, within the tolerance the single-block test of that raster uses (tests/test_gpu_routing.py,
      tests/test_gpu_parity.py);
  (c) raster_class(view) is declared for every view, with the (large, lo, hi, share) a RasterScan of the whole buffer
      declares (raster_class of the whole block is no reference: it reads the table, a whole-block call scans itself).
The Gaussian / gradient of rasters in millimetres and TPI alone on fractional elevations from 19 px are where a view that
lost its class takes other kernels; discs below 19 px and whole-metre rasters are the controls."""
import numpy as np
import pytest

from oracle import topo_oracle as orc
from topo_descriptors_amd import _lib, device as d, shard, topo

from test_gpu_routing import GNY, NX, hard_rasters, missing_footprint, same_bits, small_value_raster

pytestmark = pytest.mark.gpu

RASTERS = hard_rasters()
SMALL = ("unit_range", "kilometres", "constant_fraction", "flat")
RES = {"x": 30.0, "y": -30.0}
_ORACLE = {}  # (what, raster, parameter) -> float64 evaluation


def raster(name):
    if name in SMALL:
        return small_value_raster(name)
    if name == "frac":  # the ordinary fractional DEM the "frac+..." rasters of hard_rasters start from
        return orc.synthetic_dem(GNY, NX, seed=6, integer=False)
    if name == "int":
        return orc.synthetic_dem(GNY, NX, seed=5, integer=True)
    return RASTERS[name]


def oracle(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def scanned_class(scan):
    """(large, lo, hi, share) topo_amd_raster_class_from_scan makes of a scan."""
    taken, large, frac = scan.counts
    share = float(np.float32(frac / taken)) if taken else 0.0
    return bool(4 * large > taken), scan.range[0], scan.range[1], share


def make_views(buf, gny, nblocks, halo):
    up, down = halo
    out = []
    for row0, rows in shard.split_rows(gny, nblocks):
        lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
        out.append((d.Block(buf, row0=lo, gny=gny, first_buffer_row=lo, rows=hi - lo), row0, rows))
    return out


def declare_views(views):
    scan = d.RasterScan()
    for blk, row0, rows in views:
        scan.add(blk, own_row0=row0, own_rows=rows)
    scan.declare(*[v[0] for v in views])


def call_views(views, call, order):
    pieces = [None] * len(views)
    for k in order:
        blk, row0, rows = views[k]
        outs = call(blk, row0, rows)
        d.sync()
        pieces[k] = [o.to_host() for o in outs]
        for o in outs:
            o.free()
    return [np.concatenate([p[i] for p in pieces], axis=0) for i in range(len(pieces[0]))]


def call_whole(buf, gny, call):
    outs = call(d.Block(buf, gny=gny), 0, gny)
    d.sync()
    host = [o.to_host() for o in outs]
    for o in outs:
        o.free()
    return host


def run_case(dem, halo, call, blocks=(2, 3, 5)):
    """The whole buffer as one Block, then 2 / 3 / 5 declared views of it called forwards and backwards.
    Returns (whole outputs, {(nblocks, order): stitched outputs}, [problems of (a) and (c)])."""
    gny = dem.shape[0]
    buf = d.DeviceArray.from_host(dem)
    problems, runs = [], {}
    try:
        want_cls = scanned_class(d.RasterScan().add(d.Block(buf, gny=gny)))
        whole = call_whole(buf, gny, call)
        for nb in blocks:
            views = make_views(buf, gny, nb, halo)
            declare_views(views)
            for order, ks in (("forward", range(nb)), ("reverse", range(nb - 1, -1, -1))):
                runs[nb, order] = got = call_views(views, call, ks)
                for i, (g, w) in enumerate(zip(got, whole)):
                    if not same_bits(g, w):
                        bad = int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum())
                        problems.append(f"(a) {nb} views {order}, output {i}: {bad} pixels differ from the whole block")
            for k, (blk, _, _) in enumerate(views):
                cls = d.raster_class(blk)
                if cls != (True,) + want_cls:
                    problems.append(f"(c) {nb} views, view {k}: {cls} instead of {(True,) + want_cls}")
            d.forget_raster_class()
    finally:
        buf.free()
    return whole, runs, problems


def check_oracle(runs, problems, measure):
    """(b) on every stitched result: ``measure(outputs)`` -> (error, bound) pairs."""
    for (nb, order), got in runs.items():
        for i, (err, bound) in enumerate(measure(got)):
            if not err <= bound:
                problems.append(f"(b) {nb} views {order}, check {i}: error {err:.3g} beyond {bound:.3g}")


def tpi_call(size, tpi=True, std=False):
    def call(blk, row0, rows):
        t = d.DeviceArray(rows, blk.nx) if tpi else None
        s = d.DeviceArray(rows, blk.nx) if std else None
        blk.tpi_std(size, tpi=t, std=s, out_row0=row0, out_rows=rows)
        return [o for o in (t, s) if o is not None]
    return call


@pytest.mark.parametrize("name", list(SMALL) + ["frac+nan", "half_int_half_frac"])
@pytest.mark.parametrize("size", [19, 31, 67, 101])
def test_tpi_alone_on_views(name, size):
    dem = raster(name)
    _, runs, problems = run_case(dem, shard.halo_rows(_lib.DESC_TPI, size), tpi_call(size))
    if name in SMALL:  # tolerance of test_scaled_tpi_on_rasters_of_small_values
        want = oracle(("tpi", name, size), lambda: orc.tpi_exact(dem, size))
        tol = max(1e-4 * float(np.max(np.abs(want))), 2.5e-4 * max(1.0, float(np.max(np.abs(dem))) / 4096.0))
        if name == "constant_fraction":
            tol = 2.0 ** -9 + 2.5e-4
        check_oracle(runs, problems, lambda got: [(float(np.max(np.abs(got[0] - want))), tol)])
    else:  # tolerance of test_missing_samples_have_the_footprint_of_the_disc (fractional rasters)
        clean = np.where(np.isfinite(dem) & (np.abs(dem) < 2.0 ** 24), dem, 0.0).astype(np.float32)
        want = oracle(("tpi", name, size), lambda: orc.tpi_exact(clean, size))
        nan = oracle(("footprint", name, size), lambda: missing_footprint(dem, size))
        tol = 2.5e-4 + 2.0 ** -9

        def measure(got):
            t = got[0]
            return [(0.0 if np.array_equal(np.isnan(t), nan) else np.inf, 0.0),
                    (float(np.max(np.abs(t[~nan] - want[~nan]))), tol)]
        check_oracle(runs, problems, measure)
    assert not problems, f"{name} {size} px:\n" + "\n".join(problems)


@pytest.mark.parametrize("name", ["mm", "half_m_half_mm", "frac+nodata_rows_at_seam", "int+nodata_cols"])
@pytest.mark.parametrize("size", [7, 31, 67])
def test_tpi_std_and_std_alone_on_views(name, size):
    """Tolerances of test_wide_relief_and_large_values_are_exact."""
    dem = raster(name)
    et = oracle(("tpi", name, size), lambda: orc.tpi_exact(dem, size))
    es = oracle(("std", name, size), lambda: orc.std_exact(dem, size))
    scale = max(1.0, float(np.max(np.abs(dem))) / 4096.0)
    halo = shard.halo_rows(_lib.DESC_TPI, size)
    problems = []
    for what, flags in (("tpi+std", (True, True)), ("std", (False, True))):
        _, runs, found = run_case(dem, halo, tpi_call(size, *flags))
        if what == "tpi+std":
            check_oracle(runs, found, lambda got: [(float(np.max(np.abs(got[0] - et))), 2.5e-4 * scale),
                                                   (float(np.max(np.abs(got[1] - es))), 1e-4 * float(np.max(es)))])
        else:
            check_oracle(runs, found, lambda got: [(float(np.max(np.abs(got[0] - es))), 1e-4 * float(np.max(es)))])
        problems += [f"{what}: {p}" for p in found]
    assert not problems, f"{name} {size} px:\n" + "\n".join(problems)


def test_tpi_multi_on_views():
    """Several sizes in one call give the bits of one tpi_std call per size, on the same views."""
    sizes = (7, 31, 67)
    dem = raster("half_int_half_frac")
    halo = shard.halo_rows(_lib.DESC_TPI, max(sizes))

    def call(blk, row0, rows):
        outs = [d.DeviceArray(rows, blk.nx) for _ in sizes]
        blk.tpi_multi(sizes, outs, out_row0=row0, out_rows=rows)
        return outs

    _, runs, problems = run_case(dem, halo, call)
    for k, size in enumerate(sizes):
        whole_one, runs_one, found = run_case(dem, halo, tpi_call(size))
        problems += [f"tpi_std {size} px: {p}" for p in found]
        for key, got in runs.items():
            if not same_bits(got[k], runs_one[key][0]):
                problems.append(f"tpi_multi {size} px, {key}: not the bits of tpi_std on the same views")
    assert not problems, "\n".join(problems)


GAUSS_RASTERS = ["mm", "half_m_half_mm", "frac"]


def gauss_bound(name):
    return 1e-3 if name == "frac" else 2.0  # mm: the bound of test_gaussian_of_a_raster_beyond_the_f16_range


@pytest.mark.parametrize("name", GAUSS_RASTERS)
@pytest.mark.parametrize("sigma", [3.25, 13.0, 30.25])
def test_gaussian_on_views(name, sigma):
    dem = raster(name)

    def call(blk, row0, rows):
        out = d.DeviceArray(rows, blk.nx)
        blk.gaussian(sigma, sigma, out, out_row0=row0, out_rows=rows)
        return [out]

    _, runs, problems = run_case(dem, shard.halo_rows(_lib.DESC_GAUSS, sigma), call)
    want = oracle(("gauss", name, sigma), lambda: orc.gaussian_exact(dem, sigma))
    check_oracle(runs, problems, lambda got: [(float(np.max(np.abs(got[0] - want))), gauss_bound(name))])
    assert not problems, f"{name} sigma {sigma}:\n" + "\n".join(problems)


def rel_range(a, b):  # as in tests/test_gpu_parity.py
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.nanmax(np.abs(a - b)) / max(np.nanmax(np.abs(b)), 1e-30))


def slope_allowed(want, rel):
    """The slope error (degrees) at each pixel that dx and dy within ``rel`` of their range allow, plus float32 rounding.
    On a raster in millimetres nearly every slope lies within a degree of 90, and the float32 results differ from the
    float64 slope by a few 1e-4 of its range where the gradient is small: the same on one block as on views, and no more
    than those dx / dy errors give through arctan."""
    dx, dy = want[0], want[1]
    e = rel * float(np.hypot(np.max(np.abs(dx)), np.max(np.abs(dy))))
    g = np.hypot(dx, dy)
    return np.degrees(np.arctan(g + e) - np.arctan(np.maximum(g - e, 0.0))) + 1e-5


@pytest.mark.parametrize("name", GAUSS_RASTERS)
@pytest.mark.parametrize("sigma", [3.25, 13.0])
def test_gradient_on_views(name, sigma):
    """Bits of the whole block; dx, dy and slope within 1e-4 of their range of the float64 evaluation (on rasters in
    millimetres the slope within what that dx / dy tolerance allows, see slope_allowed)."""
    dem = raster(name)

    def call(blk, row0, rows):
        outs = [d.DeviceArray(rows, blk.nx) for _ in range(4)]
        blk.gradient(sigma, [RES["x"]], [RES["y"]], dx=outs[0], dy=outs[1], slope=outs[2], aspect=outs[3],
                     out_row0=row0, out_rows=rows)
        return outs

    _, runs, problems = run_case(dem, shard.halo_rows(_lib.DESC_GRADIENT, sigma), call)
    want = oracle(("gradient", name, sigma), lambda: orc.gradient_exact(dem, sigma, RES))
    if name == "frac":
        check_oracle(runs, problems, lambda got: [(rel_range(got[k], want[k]), 1e-4) for k in range(3)])
    else:
        allowed = slope_allowed(want, 1e-4)
        check_oracle(runs, problems, lambda got: [(rel_range(got[0], want[0]), 1e-4), (rel_range(got[1], want[1]), 1e-4),
                                                  (float(np.max(np.abs(got[2] - want[2]) - allowed)), 0.0)])
    assert not problems, f"{name} sigma {sigma}:\n" + "\n".join(problems)


def test_sx_on_views():
    dem = raster("frac+nan")
    window, dj, di, dist = d.sx_offsets(135.0, 500.0, RES["x"], RES["y"])

    def call(blk, row0, rows):
        out = d.DeviceArray(rows, blk.nx)
        blk.sx(dj, di, dist, window, 10.0, out, out_row0=row0, out_rows=rows)
        return [out]

    _, _, problems = run_case(dem, shard.halo_rows(_lib.DESC_SX, max(0, -dj.min()), max(0, dj.max())), call)
    assert not problems, "\n".join(problems)


def test_valley_ridge_on_views():
    dem = raster("frac+nan")
    flats = [0, 0.15, 0.3]
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(9, flats), np.arange(0, 180, 7, dtype=np.float32))
    mean, stdev = float(np.nanmean(dem)), float(np.nanstd(dem))

    def call(blk, row0, rows):
        n, a = d.DeviceArray(rows, blk.nx), d.DeviceArray(rows, blk.nx)
        blk.valley_ridge(taps, ksize, angles, len(flats), mean, stdev, n, a, out_row0=row0, out_rows=rows)
        return [n, a]

    _, _, problems = run_case(dem, shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max())), call)
    assert not problems, "\n".join(problems)


def test_fill_na_out_of_place_on_views():
    dem = raster("frac+nan")

    def call(blk, row0, rows):
        out = d.DeviceArray(rows, blk.nx)
        blk.fill_na(out, out_row0=row0, out_rows=rows)
        return [out]

    whole, _, problems = run_case(dem, (3, 3), call)
    assert not np.isnan(whole[0]).any()
    assert not problems, "\n".join(problems)


def test_wide_ring_whole_buffer_and_marching_kernel_on_views():
    """TPI alone at 67 px on a whole-metre raster: the whole buffer takes the wide ring, every view the marching kernel
    (the wide ring runs on single blocks only), with the same bits."""
    size = 67
    dem = raster("int")
    routes = []

    def call(blk, row0, rows):
        t = d.DeviceArray(rows, blk.nx)
        blk.tpi_std(size, tpi=t, out_row0=row0, out_rows=rows)
        routes.append((blk.rows == blk.gny, d.tpi_route()))
        return [t]

    _, runs, problems = run_case(dem, shard.halo_rows(_lib.DESC_TPI, size), call)
    assert routes[0] == (True, 1), routes[0]
    assert all(r == (False, 0) for r in routes[1:]), routes
    want = oracle(("tpi", "int", size), lambda: orc.tpi_exact(dem, size))
    check_oracle(runs, problems, lambda got: [(float(np.max(np.abs(got[0] - want))), 2.5e-4)])
    assert not problems, "\n".join(problems)


def overlaps(view, r0, rows):
    blk = view[0]
    return blk.first < r0 + rows and r0 < blk.first + blk.rows


def test_in_place_fill_drops_the_declarations_of_the_rows_it_writes():
    """An in-place fill_na on one view writes that view's owned rows: every view overlapping them loses its declaration,
    the others keep theirs.  Scanned and declared afresh, the views give the whole block's bits on the filled buffer."""
    size = 19
    dem = raster("frac+nan")
    gny = dem.shape[0]
    buf = d.DeviceArray.from_host(dem)
    try:
        views = make_views(buf, gny, 5, shard.halo_rows(_lib.DESC_TPI, size))
        declare_views(views)
        assert all(d.raster_class(v[0])[0] for v in views)
        nan_row = int(np.argwhere(np.isnan(dem))[0][0])
        k = next(i for i, (_, r0, n) in enumerate(views) if r0 <= nan_row < r0 + n)
        blk, row0, rows = views[k]
        blk.fill_na(buf, out_row0=row0, out_rows=rows)
        d.sync()
        hit = [overlaps(v, row0, rows) for v in views]
        assert 1 < sum(hit) < len(views), hit
        # a view finds a declaration when its first row lies inside a declared view that the fill did not touch (the
        # view just above a written one starts inside the ghost rows of the untouched view above it, and takes its class)
        kept = [v for v, h in zip(views, hit) if not h]
        want = [any(overlaps(u, v[0].first, 1) for u in kept) for v in views]
        assert not want[k] and not all(want[i] for i, h in enumerate(hit) if h), want
        assert [d.raster_class(v[0])[0] for v in views] == want, (hit, want)
        filled = buf.to_host()
        assert not np.isnan(filled).any()
        assert np.array_equal(filled[:row0], dem[:row0]) and np.array_equal(filled[row0 + rows:], dem[row0 + rows:])

        declare_views(views)
        want_cls = scanned_class(d.RasterScan().add(d.Block(buf, gny=gny)))
        assert all(d.raster_class(v[0]) == (True,) + want_cls for v in views)
        whole = call_whole(buf, gny, tpi_call(size))
        got = call_views(views, tpi_call(size), range(len(views)))
        assert same_bits(got[0], whole[0])
        d.forget_raster_class()
    finally:
        buf.free()
