"""TPI alone at the wide ring's disc sizes (csrc/disc_ring_wide_impl.hpp: 6 columns per lane, staging waves apart).

A single-block call on a raster of whole metres takes the wide ring; a call on a row block of the same DEM takes the
marching kernel.  Both are exact, so the stitched row blocks must give the single block's bits - across strips of 312
columns that the width does not fill, DEM borders, tiles with NaN, nodata values and fractional samples (which the wide
ring hands to the scaled pass and the general kernel through the marching geometry's tile map).  Every single-block call
here asserts that the wide ring ran (topo_amd_tpi_route), and every row-block call that it did not, so each comparison is
the wide ring against the marching kernel."""
import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import _lib, device as d, shard  # noqa: E402

WIDE_SIZES = [67]  # the route's sizes (csrc/disc_wave_impl.hpp: tpi_takes_wide_ring)


def lattice_samples(dem):
    """The samples the raster class is taken from (csrc/raster_class.hip, scan_block: rows step_r / 2 + i step_r, columns
    step_c / 2 + j step_c, step = max(1, extent / 128))."""
    gny, nx = dem.shape
    sr, sc = max(1, gny // 128), max(1, nx // 128)
    return dem[sr // 2::sr, sc // 2::sc]


def tpi_blocks(dem, size, nblocks, wide=True):
    """TPI of `dem` evaluated on `nblocks` row blocks, each uploaded with exactly its ghost rows, stitched.  The single
    block must take the wide ring (when `wide`), a row block the marching kernel."""
    gny, nx = dem.shape
    up, down = shard.halo_rows(_lib.DESC_TPI, size)
    pieces = []
    for row0, rows in shard.split_rows(gny, nblocks):
        lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
        dev = d.DeviceArray.from_host(dem[lo:hi])
        blk = d.Block(dev, row0=lo, gny=gny)
        t = d.DeviceArray(rows, nx)
        blk.tpi_std(size, tpi=t, out_row0=row0, out_rows=rows)
        d.sync()
        assert d.tpi_route() == (1 if nblocks == 1 and wide else 0), (size, nblocks)
        pieces.append(t.to_host())
        t.free()
        dev.free()
    return np.concatenate(pieces, axis=0)


def check_against_blocks(dem, size, blocks=(2, 3)):
    whole = tpi_blocks(dem, size, 1)
    for nb in blocks:
        parts = tpi_blocks(dem, size, nb)
        bad = ~((parts == whole) | (np.isnan(parts) & np.isnan(whole)))
        assert not bad.any(), (size, nb, np.argwhere(bad)[:5])
    return whole


@pytest.mark.parametrize("size", WIDE_SIZES)
@pytest.mark.parametrize("shape", [(200, 312), (160, 316), (230, 700), (96, 1252)])
def test_wide_ring_matches_marching_and_oracle(size, shape):
    """Widths of one strip, one strip and a piece, and several strips with a short last one; every tile a border tile."""
    dem = orc.synthetic_dem(*shape, seed=size + shape[1])
    whole = check_against_blocks(dem, size)
    assert np.max(np.abs(whole - orc.tpi_exact(dem, size))) <= 2.5e-4


@pytest.mark.parametrize("size", WIDE_SIZES)
def test_wide_ring_runs_of_several_tiles(size):
    """More tiles than blocks: a block's run carries the ring down a strip over several 64-row tiles."""
    dem = orc.synthetic_dem(5000, 1000, seed=5)
    check_against_blocks(dem, size, blocks=(2,))


@pytest.mark.parametrize("size", WIDE_SIZES)
def test_wide_ring_nan_and_nodata(size):
    gny, nx = 420, 760
    dem = orc.synthetic_dem(gny, nx, seed=23)
    dem[140:150, 400:420] = np.nan  # non-finite: the scaled pass and the general kernel
    dem[300:330, 20:90] = -9999.0   # nodata as a whole-metre value: the wide ring's own
    dem[5, 700] = 3.0e6             # absurd: beyond the integer chain
    whole = check_against_blocks(dem, size)
    assert np.isnan(whole[145, 410]) and np.isfinite(whole[20, 20]) and np.isfinite(whole[400, 300])


@pytest.mark.parametrize("size", WIDE_SIZES)
def test_wide_ring_fractional_patch(size):
    """A fractional patch in a whole-metre raster: the phases whose windows reach it go to the scaled pass."""
    gny, nx = 480, 980
    dem = orc.synthetic_dem(gny, nx, seed=31)
    rows = np.arange(200, 260)
    rows = rows[rows % max(1, gny // 128) != max(1, gny // 128) // 2]  # off the class lattice: the raster stays "whole metres"
    dem[rows, 500:560] += 0.375
    lat = lattice_samples(dem)
    assert np.array_equal(lat, np.trunc(lat)), "the patch must not reach the lattice (else the marching route runs)"
    whole = check_against_blocks(dem, size)
    exact = orc.tpi_exact(dem, size)
    # whole-metre discs exact; discs that reach the patch within the scaled route's 2^-9 m (tpi_scaled_march_kernel)
    near = np.zeros(dem.shape, bool)
    near[200 - 34:260 + 34, 500 - 34:560 + 34] = True
    assert np.max(np.abs(whole - exact)[~near]) <= 2.5e-4
    assert np.max(np.abs(whole - exact)[near]) <= 2.0 ** -9 + 2.5e-4
    # the wide ring must have left those discs: a chain over trunc(x) would be off by about 0.375 m x the patch's share
    trunc_only = orc.tpi_exact(np.trunc(dem), size)
    assert np.max(np.abs(whole[230, 530] - trunc_only[230, 530])) > 0.1
