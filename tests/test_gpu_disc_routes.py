"""TPI / STD discs (csrc/disc.hip, csrc/disc_wave_impl.hpp) on every kernel route, each against the float64 oracle.

``launch_tpi_std`` and ``launch_wave_any<SIZE>`` choose among about twenty kernel sequences from the disc size, the outputs
wanted, the raster class, the width and whether the call is a single block.  ``ROUTES`` names, for every size, output and
raster class, the word ``device.disc_route()`` must report (derived from the dispatch code, not from a run), so a retune that
moves a size to another kernel fails here instead of passing on that kernel.  Every case is held to the tap-by-tap float64
evaluation (``orc.tpi_exact`` / ``orc.std_exact``) within the bounds ``include/topo_amd.h`` states, to the exact NaN footprint
of the disc, and to the bits of the other kernels that compute the same thing (STD alone against TPI + STD, TPI alone against
TPI + STD on whole metres, row blocks against the single call).  ``tests/test_disc_route_design.py`` shows on the oracle alone
that these comparisons notice a lost rim tap, a shifted run, a repeated row or column and a footprint that is a pixel off.

Every comparison prints ``FIG <route> ...`` with the largest error as a share of its bound (``pytest -s`` shows them)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import topo_oracle as orc
from topo_descriptors_amd import _lib, device as d, shard, topo

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GNY, NX = 200, 1040          # several tile rows of 48 and of 60, several strips at every strip width, nx % 4 == 0
SMALL = (160, 520)           # the rasters of 101 and 103 px
KINDS = ("whole", "frac", "patch", "hard_whole", "hard_frac")
SIZES = (3, 5, 7, 13, 15, 17, 19, 21, 23, 41, 43, 65, 67, 69, 77, 79, 101)
OPS = ("tpi", "std", "tpi_std")

# ---- the route word (include/topo_amd.h, topo_amd_disc_route) -----------------------------------------------------------
WAVE, REPITCHED, GATHER, PLANES, PAIR = 1, 2, 3, 4, 5
WANT = {"tpi": 1 << 3, "std": 1 << 4, "tpi_std": 3 << 3}
F_GENERAL, F_MARCH, F_RING, F_WIDE, F_SCALED_ALL, F_STD_RING, F_SPEC4, F_SPEC8, F_SUMS, F_PAIR_RING = (k << 5 for k in range(10))
STD_MARCH = 1 << 9
FR_MARCH, FR_RING_BOTH, FR_STD_RING_BOTH, FR_SPEC_BOTH = (k << 10 for k in range(1, 5))
SCALED, DEFERRED = 1 << 13, 1 << 14
SPLIT, WIDE_BIT, PLANES_F64, PLANES_FRAC = 1 << 23, 1 << 24, 1 << 25, 1 << 26


def kernels(first, tile_rows, followers):
    return first | (tile_rows << 16) | followers


# the kernel sequences of launch_wave_any
GENERAL64, GENERAL56, GENERAL40 = (kernels(F_GENERAL, th, 0) for th in (64, 56, 40))  # STD at 3 px; TH8 of 79 and 101 px
MARCH_ONLY = kernels(F_MARCH, 60, DEFERRED)                                    # TPI at 3 px
RING = kernels(F_RING, 64, FR_RING_BOTH | DEFERRED)                            # TPI 5 ... 17 px
MARCH_SCALED, MARCH_SCALED48, MARCH_SCALED36 = (kernels(F_MARCH, th, SCALED | DEFERRED) for th in (60, 48, 36))
SCALED_ALL, SCALED_ALL48, SCALED_ALL36 = (kernels(F_SCALED_ALL, th, DEFERRED) for th in (60, 48, 36))
WIDE = kernels(F_WIDE, 64, SCALED | DEFERRED) | WIDE_BIT                       # TPI 67 px, whole metres, one block
MARCH_EXACT = kernels(F_MARCH, 60, FR_MARCH | DEFERRED)                        # TOPO_AMD_TPI_FRACTION_EXACT=1
SPEC8 = kernels(F_SPEC8, 48, DEFERRED)                                         # TPI + STD 5 ... 13 px, whole metres
SPEC4_SPEC = kernels(F_SPEC4, 48, FR_SPEC_BOTH | DEFERRED)                     # STD 5 ... 21 px
SPEC4_RING = kernels(F_SPEC4, 48, FR_STD_RING_BOTH | DEFERRED)                 # STD 23 ... 41 px
STD_RING = kernels(F_STD_RING, 60, DEFERRED)                                   # STD 43 ... 67 px
SUMS = kernels(F_SUMS, 60, STD_MARCH | FR_MARCH | DEFERRED)                    # ... on a mostly fractional raster
MARCH_STD = kernels(F_MARCH, 60, STD_MARCH | DEFERRED)                         # STD 69 ... 77 px

# Raster classes: W frac_share == 0 (whole, hard_whole), P 0 < frac_share <= 0.5 (patch: 0.10, 0.25 on the small raster),
# F frac_share > 0.5 (frac, hard_frac).  size: (TPI on W, P, F), (STD on W, P, F), (TPI + STD on W, P, F), as derived from
# launch_wave_any: tile_rows(SIZE, 12, 60) is 60 up to 77 px, 48 at 79 and 36 at 101; tile_rows(SIZE, 8, 64) is 56 at 79 and
# 40 at 101; std_ring_fits holds up to 67 px, std_ring_both_fits up to 41, std_spec_both_fits up to 21, std_spec_wide_fits
# up to 13 (and STD alone takes it from 2^27 pixels only); the TPI ring is taken up to 17 px.
TPI_BIG = (MARCH_SCALED, MARCH_SCALED, SCALED_ALL)
ROUTES = {
    3: ((MARCH_ONLY,) * 3, (GENERAL64,) * 3, (GENERAL64,) * 3),
    5: ((RING,) * 3, (SPEC4_SPEC,) * 3, (SPEC8, SPEC4_SPEC, SPEC4_SPEC)),
    7: ((RING,) * 3, (SPEC4_SPEC,) * 3, (SPEC8, SPEC4_SPEC, SPEC4_SPEC)),
    13: ((RING,) * 3, (SPEC4_SPEC,) * 3, (SPEC8, SPEC4_SPEC, SPEC4_SPEC)),
    15: ((RING,) * 3, (SPEC4_SPEC,) * 3, (SPEC4_SPEC,) * 3),
    17: ((RING,) * 3, (SPEC4_SPEC,) * 3, (SPEC4_SPEC,) * 3),
    19: (TPI_BIG, (SPEC4_SPEC,) * 3, (SPEC4_SPEC,) * 3),
    21: (TPI_BIG, (SPEC4_SPEC,) * 3, (SPEC4_SPEC,) * 3),
    23: (TPI_BIG, (SPEC4_RING,) * 3, (SPEC4_RING,) * 3),
    41: (TPI_BIG, (SPEC4_RING,) * 3, (SPEC4_RING,) * 3),
    43: (TPI_BIG, (STD_RING, STD_RING, SUMS), (STD_RING, STD_RING, SUMS)),
    65: (TPI_BIG, (STD_RING, STD_RING, SUMS), (STD_RING, STD_RING, SUMS)),
    67: ((WIDE, MARCH_SCALED, SCALED_ALL), (STD_RING, STD_RING, SUMS), (STD_RING, STD_RING, SUMS)),
    69: (TPI_BIG, (MARCH_STD,) * 3, (MARCH_STD,) * 3),
    77: (TPI_BIG, (MARCH_STD,) * 3, (MARCH_STD,) * 3),
    79: ((MARCH_SCALED48, MARCH_SCALED48, SCALED_ALL48), (GENERAL56,) * 3, (GENERAL56,) * 3),
    101: ((MARCH_SCALED36, MARCH_SCALED36, SCALED_ALL36), (GENERAL40,) * 3, (GENERAL40,) * 3),
}
CLASS = {"whole": 0, "hard_whole": 0, "patch": 1, "frac": 2, "hard_frac": 2}


def expected_route(size, op, kind, launcher=WAVE, one_block=True):
    word = ROUTES[size][OPS.index(op)][CLASS[kind]]
    if word == WIDE and not one_block:
        word = MARCH_SCALED  # the wide ring takes single-block calls only
    return launcher | WANT[op] | word


# ---- rasters ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(ny, nx, integer):
    # (one field 1041 columns wide: the 1038- and 1041-column rasters share their columns with the 1040-column ones)
    wide = 1041 if nx > SMALL[1] else nx
    return orc.synthetic_dem(ny, wide, seed=61 if integer else 62, integer=integer)[:, :nx]


@functools.lru_cache(maxsize=None)
def raster(kind, ny=GNY, nx=NX):
    """whole / frac: integer metres / fractional elevations.  patch: whole with + 0.25 on 70 x 300 pixels across the tile-row
    boundaries at 48, 60 and 96 and across column 512.  hard_*: a NaN one pixel from the top border, + inf, 1e20 and a 30 x 200
    block of -9999, each in tiles of its own."""
    a = _base(ny, nx, kind in ("whole", "patch", "hard_whole")).copy()
    if kind == "patch":
        c0 = 380 if nx > SMALL[1] else 215
        a[40:110, c0:c0 + 300] += 0.25
    if kind.startswith("hard"):
        f = 1.0 if nx > SMALL[1] else nx / 1040.0
        a[1, int(700 * f)] = np.nan
        a[min(150, ny - 1), int(100 * f)] = np.inf
        a[min(100, ny - 1), int(900 * f)] = 1.0e20
        a[20:50, int(200 * f):int(400 * f)] = -9999.0
    a.setflags(write=False)
    return a


class Reference:
    """The float64 evaluation for one raster and size, and the masks the comparisons need (one tap-by-tap sum for the three
    of them: counts of at most 101^2 taps in fields of 16 bits each)."""

    def __init__(self, dem, size):
        dem = np.asarray(dem)
        self.size = size
        with np.errstate(invalid="ignore"):
            missing = (~np.isfinite(dem)) | (np.abs(np.trunc(np.nan_to_num(dem, nan=0.0, posinf=0.0, neginf=0.0))) >= 2.0 ** 24)
        self.clean = np.where(missing, 0.0, dem).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.tpi = orc.tpi_exact(self.clean, size)
            self.std = orc.std_exact(self.clean, size)
        marks = missing + 65536.0 * (np.abs(self.clean) >= 9999.0) + 4294967296.0 * (self.clean != np.trunc(self.clean))
        hits = orc._disc_sum_f64(marks.astype(np.float64), size, drop_centre=False)[0].astype(np.int64)
        self.nan = (hits & 0xffff) > 0                # missing_footprint of tests/test_gpu_routing.py
        self.near = ((hits >> 16) & 0xffff) > 0       # the disc holds a sample of magnitude >= 9999
        self.fractional = (hits >> 32) > 0            # the disc holds a fractional sample
        if size == 1:
            # a disc of one tap: n - 1 = 0, TPI is 0 / 0 everywhere and STD 0 / 0 on whole metres, as in the reference
            self.std_nan = np.isnan(self.std) | self.nan
            self.nan = self.nan | np.isnan(self.tpi)
        else:
            self.std_nan = self.nan

    def tpi_as_stored(self):
        """The reference as a kernel would store it: float32, NaN on the footprint."""
        return np.where(self.nan, np.nan, self.tpi).astype(np.float32)

    def std_as_stored(self):
        return np.where(self.std_nan, np.nan, self.std).astype(np.float32)


@functools.lru_cache(maxsize=6)
def reference(kind, size, ny=GNY, nx=NX):
    return Reference(raster(kind, ny, nx), size)


def shape_of(size):
    return SMALL if size > 100 else (GNY, NX)


# ---- the comparisons ----------------------------------------------------------------------------------------------------
def check_nans(got, want_nan, what=""):
    assert np.array_equal(np.isnan(got), want_nan), (what, "NaN on", int(np.isnan(got).sum()), "pixels, the footprint has", int(want_nan.sum()))


def _share(err, bound, mask, what):
    """The largest err / bound on the pixels of ``mask`` (asserted to be at most 1)."""
    if not mask.any():
        return 0.0
    e, b = err[mask], np.broadcast_to(bound, err.shape)[mask]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(e == 0.0, 0.0, e / b)
    over = ~(ratio <= 1.0)
    assert not over.any(), (what, "pixels over the bound", int(over.sum()), "worst share", float(np.max(ratio[over])),
                            "first at", tuple(np.argwhere(mask)[np.flatnonzero(over)[0]]))
    return float(ratio.max())


def check_tpi(got, ref, scaled_allowance=False, what="tpi"):
    """2.5e-4 max(1, max|dem| / 4096), + 2^-9 where the scaled route may have summed fractional samples.  Twice: on the pixels
    whose disc holds no sample of magnitude >= 9999 with the scale of those pixels, then on the others with the raster's."""
    check_nans(got, ref.nan, what)
    err = np.abs(got.astype(np.float64) - ref.tpi)
    extra = (2.0 ** -9) * ref.fractional if scaled_allowance else 0.0
    calm, wild = ~ref.nan & ~ref.near, ~ref.nan & ref.near
    share = 0.0
    for mask, values in ((calm, np.abs(ref.clean[calm])), (wild, np.abs(ref.clean))):
        scale = max(1.0, float(values.max()) / 4096.0) if values.size else 1.0
        share = max(share, _share(err, 2.5e-4 * scale + extra, mask, what))
    return share


def check_std(got, ref, what="std"):
    """1e-4 max(es), twice as in check_tpi."""
    check_nans(got, ref.std_nan, what)
    err = np.abs(got.astype(np.float64) - ref.std)
    calm, wild = ~ref.std_nan & ~ref.near, ~ref.std_nan & ref.near
    share = 0.0
    for mask, top in ((calm, ref.std[calm]), (wild, ref.std[~ref.std_nan])):
        bound = 1e-4 * float(top.max()) if top.size else 0.0
        share = max(share, _share(err, bound, mask, what))
    return share


def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def noted_route():
    word = d.disc_route()
    assert (word >> 24) & 1 == d.tpi_route(), hex(word)
    return word


def host_call(op, dem, size):
    """(tpi or None, std or None, route)"""
    if op == "tpi":
        t, s = topo.tpi(dem, size), None
    elif op == "std":
        t, s = None, topo.std(dem, size)
    else:
        t, s = topo.tpi_std(dem, size)
    return t, s, noted_route()


def scaled_may_run(size, op, launcher=WAVE):
    """TPI alone from 19 px on the wave-shift kernels sums fractional windows in units of 2^-8 m."""
    return op == "tpi" and launcher in (WAVE, REPITCHED) and size % 2 == 1 and 19 <= size <= 101


def check_planes(t, s, ref, size, op, route, label):
    st = check_tpi(t, ref, scaled_may_run(size, op, route & 7), (label, op, "tpi")) if t is not None else None
    ss = check_std(s, ref, (label, op, "std")) if s is not None else None
    print(f"FIG {route:#010x} {label} {op} size {size}: share of the bound, TPI {st if st is None else round(st, 4)}, "
          f"STD {ss if ss is None else round(ss, 4)}")


def block_calls(dem, cuts, size, op):
    """The raster in row blocks [cuts[k], cuts[k + 1]) with the halo of shard.halo_rows and the whole raster's class declared
    for each block's memory, as run_blocks of tests/test_gpu_routing.py does it.  (tpi, std, the blocks' routes)"""
    gny, nx = dem.shape
    above, below = shard.halo_rows(_lib.DESC_TPI, size)
    scan = d.RasterScan()
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        dev = d.DeviceArray.from_host(dem[r0:r1])
        scan.add(d.Block(dev, row0=r0, gny=gny))
        dev.free()
    planes, routes = {"tpi": [], "std": []}, []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        lo, hi = max(0, r0 - above), min(gny, r1 + below)
        dev = d.DeviceArray.from_host(dem[lo:hi])
        blk = d.Block(dev, row0=lo, gny=gny)
        scan.declare(blk)
        t = d.DeviceArray(r1 - r0, nx) if op != "std" else None
        s = d.DeviceArray(r1 - r0, nx) if op != "tpi" else None
        blk.tpi_std(size, tpi=t, std=s, out_row0=r0, out_rows=r1 - r0)
        d.sync()
        routes.append(noted_route())
        for name, plane in (("tpi", t), ("std", s)):
            if plane is not None:
                planes[name].append(plane.to_host())
                plane.free()
        dev.free()
    return (np.concatenate(planes["tpi"]) if planes["tpi"] else None,
            np.concatenate(planes["std"]) if planes["std"] else None, routes)


# ---- every size on every raster -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES)
def test_route_values_and_footprint(size, kind):
    ny, nx = shape_of(size)
    dem = raster(kind, ny, nx)
    ref = reference(kind, size, ny, nx)
    got = {}
    for op in OPS:
        t, s, route = host_call(op, dem, size)
        assert route == expected_route(size, op, kind), (op, hex(route), hex(expected_route(size, op, kind)))
        check_planes(t, s, ref, size, op, route, kind)
        got[op] = (t, s)
    # the same sums, whatever kernel took them
    assert same_bits(got["std"][1], got["tpi_std"][1])
    if kind in ("whole", "hard_whole"):
        assert same_bits(got["tpi"][0], got["tpi_std"][0])
    for cuts in ((0, 77, ny), (0, 51, 133, ny)):
        for op in OPS:
            t, s, routes = block_calls(dem, cuts, size, op)
            want = expected_route(size, op, kind, one_block=False)
            assert routes == [want] * (len(cuts) - 1), (op, cuts, [hex(r) for r in routes], hex(want))
            assert t is None or same_bits(t, got[op][0]), (op, cuts, "tpi")
            assert s is None or same_bits(s.astype(np.float64), got[op][1]), (op, cuts, "std")


# ---- every odd size from 3 to 101 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hard_whole", "hard_frac"])
@pytest.mark.parametrize("size", range(3, 103, 2))
def test_every_odd_size_takes_its_route(size, kind):
    """The sizes between the pinned ones: the word is the one ``route_rule`` (tests/test_disc_route_design.py) derives from the
    thresholds, on the wave-shift launcher - a size its translation unit does not build would fall through to the gather
    kernel or the prefix planes with correct values - and the requests agree in their bits.  160 x 520: several tile rows at
    every tile height from 36 to 64, two strips at the 256-, 384- and 512-column widths.  No oracle here."""
    from test_disc_route_design import route_rule  # (that module imports this one)

    dem = raster(kind, *SMALL)
    got = {}
    for op in OPS:
        t, s, route = host_call(op, dem, size)
        want = WAVE | WANT[op] | route_rule(size, op, CLASS[kind])
        assert route == want, (op, hex(route), hex(want))
        got[op] = (t, s)
    assert same_bits(got["std"][1], got["tpi_std"][1])
    if kind == "hard_whole":
        assert same_bits(got["tpi"][0], got["tpi_std"][0])


# ---- widths that are no multiple of 4: the re-pitched copy ------------------------------------------------------------------
@pytest.mark.parametrize("width", [1038, 1041])
@pytest.mark.parametrize("kind", ["patch", "hard_frac"])
@pytest.mark.parametrize("size", [7, 43, 77])
def test_repitched_widths(size, kind, width):
    dem = raster(kind, GNY, width)
    ref = reference(kind, size, GNY, width)
    common = min(width, NX)
    same = common - size // 2  # columns whose disc stays left of the narrower raster's last column
    for op in OPS:
        t, s, route = host_call(op, dem, size)
        assert route == expected_route(size, op, kind, launcher=REPITCHED), (op, hex(route))
        check_planes(t, s, ref, size, op, route, f"{kind} width {width}")
        t0, s0, _ = host_call(op, raster(kind), size)
        assert t is None or same_bits(t[:, :same], t0[:, :same]), (op, "tpi")
        assert s is None or same_bits(s[:, :same], s0[:, :same]), (op, "std")


# ---- rasters narrower than 4 columns, and lower than the disc ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_raster(width):
    a = orc.synthetic_dem(GNY, width, seed=63, integer=False)
    a[100:150] = np.rint(a[100:150])
    a[1, width - 1] = np.nan
    a[20:50, 0] = -9999.0
    return a


@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("size", [7, 19])
def test_odd_sizes_on_fewer_than_four_columns_take_the_gather_kernel(size, width):
    dem = narrow_raster(width)
    ref = Reference(dem, size)
    got = {}
    for op in OPS:
        t, s, route = host_call(op, dem, size)
        assert route == GATHER | WANT[op] | (32 << 16), (op, hex(route))
        check_planes(t, s, ref, size, op, route, f"width {width}")
        got[op] = (t, s)
    assert same_bits(got["std"][1], got["tpi_std"][1])


@pytest.mark.parametrize("kind", ["whole", "hard_frac"])
@pytest.mark.parametrize("size,height", [(7, 1), (7, 6), (67, 1), (67, 66)])
def test_rasters_lower_than_the_disc(size, height, kind):
    dem = np.ascontiguousarray(raster(kind)[:height])
    ref = Reference(dem, size)
    got = {}
    for op in OPS:
        t, s, route = host_call(op, dem, size)
        assert route == expected_route(size, op, kind), (op, hex(route))
        check_planes(t, s, ref, size, op, route, f"{kind} height {height}")
        got[op] = (t, s)
    assert same_bits(got["std"][1], got["tpi_std"][1])
    if kind == "whole":
        assert same_bits(got["tpi"][0], got["tpi_std"][0])


# ---- the LDS-gather kernel and the prefix planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["patch", "hard_frac"])
@pytest.mark.parametrize("size", [1, 2, 6, 40, 68, 70, 103])
def test_gather_kernel_and_prefix_planes(size, kind):
    """Sizes without a wave-shift kernel: the LDS-gather kernel below 70 px (its tile is 32 rows at every such size: the 16- and
    8-row builds and the fallback to the prefix planes are not reached), the prefix planes from 70 px - the narrow ones with
    the plane of fractional parts on ``patch``, the float64 ones on ``hard_frac`` (non-finite samples)."""
    ny, nx = shape_of(size)
    dem = raster(kind, ny, nx)
    ref = reference(kind, size, ny, nx)
    got = {}
    for op in OPS:
        t, s, route = host_call(op, dem, size)
        if size < 70:
            want = GATHER | WANT[op] | (32 << 16)
        else:
            want = PLANES | WANT[op] | (PLANES_FRAC if kind == "patch" else PLANES_F64)
        assert route == want, (op, hex(route), hex(want))
        check_planes(t, s, ref, size, op, route, kind)
        got[op] = (t, s)
    assert same_bits(got["std"][1], got["tpi_std"][1])
    for cuts in ((0, 77, ny),):
        t, s, routes = block_calls(dem, cuts, size, "tpi_std")
        assert all(r & 7 == (GATHER if size < 70 else PLANES) for r in routes)
        assert same_bits(t, got["tpi_std"][0]) and same_bits(s.astype(np.float64), got["tpi_std"][1])


# ---- a call taller than one launch covers ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tall_raster():
    a = orc.synthetic_dem(65300, 64, seed=64, integer=True)
    a[65270:65290, 10:40] += 0.25   # (between the lattice rows of the class scan: the raster's class stays whole metres)
    a[65275, 50] = np.nan
    return a


@pytest.mark.parametrize("size", [7, 70])
def test_tall_call_is_split_without_a_seam(size):
    """65300 rows: launch_tpi_std runs rows 0 ... 65279 and 65280 ... 65299 as two parts.  The rows around the cut against the
    oracle on a crop (its top edge is false: only rows at least ``size`` below it are compared; the bottom is the raster's)."""
    dem = tall_raster()
    gny, nx = dem.shape
    dev = d.DeviceArray.from_host(dem)
    t, s = d.DeviceArray(gny, nx), d.DeviceArray(gny, nx)
    d.Block(dev).tpi_std(size, tpi=t, std=s)
    d.sync()
    route = noted_route()
    if size == 7:
        assert route == WAVE | WANT["tpi_std"] | SPEC8 | SPLIT, hex(route)
    else:
        assert route == PLANES | WANT["tpi_std"] | PLANES_F64 | SPLIT, hex(route)
    top = 65280 - 3 * size
    first = 65280 - 2 * size
    got_t, got_s = t.to_host(first, gny - first), s.to_host(first, gny - first)
    for a in (dev, t, s):
        a.free()
    ref = Reference(dem[top:], size)
    for name in ("clean", "tpi", "std", "nan", "std_nan", "near", "fractional"):
        setattr(ref, name, getattr(ref, name)[first - top:])
    assert ref.nan.any() and not ref.nan.all()
    check_planes(got_t, got_s, ref, size, "tpi_std", route, "tall")


# ---- TOPO_AMD_TPI_FRACTION_EXACT=1 (read once per process: a child) ------------------------------------------------------------
_EXACT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, %(tests)r)
import test_gpu_disc_routes as cases
from topo_descriptors_amd import topo
out = {}
for size in (19, 77):
    for kind in ("frac", "patch"):
        out[f"{kind}_{size}"] = topo.tpi(cases.raster(kind), size)
        out[f"route_{kind}_{size}"] = np.int64(cases.noted_route())
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def exact_child(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("exact") / "tpi.npz")
    env = dict(os.environ, TOPO_AMD_TPI_FRACTION_EXACT="1")
    code = _EXACT_CHILD % {"repo": REPO, "tests": os.path.join(REPO, "tests")}
    run = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("kind", ["frac", "patch"])
@pytest.mark.parametrize("size", [19, 77])
def test_exact_fraction_route(exact_child, size, kind):
    route = int(exact_child[f"route_{kind}_{size}"])
    assert route == WAVE | WANT["tpi"] | MARCH_EXACT, hex(route)
    exact = exact_child[f"{kind}_{size}"]
    ref = reference(kind, size)
    share = check_tpi(exact, ref, scaled_allowance=False, what=("exact", kind, size))
    print(f"FIG {route:#010x} {kind} tpi size {size} (exact fractions): share of the bound, TPI {share:.4f}")
    default = topo.tpi(raster(kind), size)
    assert noted_route() == expected_route(size, "tpi", kind)
    assert np.max(np.abs(default.astype(np.float64) - exact)) <= 2.0 ** -9


# ---- several sizes in one call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["whole", "patch"])
def test_multi_size_calls_give_the_single_calls_bits(kind):
    """topo.tpi_std_multi runs its sizes one after the other (its word is the last size's); the device call
    Block.tpi_multi takes 5 and 7 px through the two-disc kernel and the others one by one."""
    sizes = (5, 7, 13, 69)
    dem = raster(kind)
    single = {size: topo.tpi_std(dem, size) for size in sizes}
    alone = {size: topo.tpi(dem, size) for size in sizes}
    tpis, stds = topo.tpi_std_multi(dem, sizes)
    assert noted_route() == expected_route(69, "tpi_std", kind)
    for k, size in enumerate(sizes):
        assert same_bits(tpis[k], single[size][0]) and same_bits(stds[k], single[size][1]), size
    dev = d.DeviceArray.from_host(dem)
    outs = [d.DeviceArray(GNY, NX) for _ in sizes]
    pair_word = PAIR | WANT["tpi"] | kernels(F_PAIR_RING, 64, DEFERRED)
    d.Block(dev).tpi_multi(sizes[:2], outs[:2])
    d.sync()
    assert noted_route() == pair_word, hex(noted_route())
    pair = [o.to_host() for o in outs[:2]]
    d.Block(dev).tpi_multi(sizes, outs)
    d.sync()
    assert noted_route() == expected_route(69, "tpi", kind), hex(noted_route())
    for k, size in enumerate(sizes):
        got = outs[k].to_host()
        assert same_bits(got, alone[size]), size
        if k < 2:
            assert same_bits(pair[k], got), size
    for a in [dev] + outs:
        a.free()
