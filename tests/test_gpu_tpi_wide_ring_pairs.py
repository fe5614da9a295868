"""The wide ring's joint sweep over a chain wave's row pair (csrc/disc_ring_wide_impl.hpp: wide_pair_sum, WPair).

A chain wave sums rows 2 w and 2 w + 1 of a phase in one sweep: every prefix row that both rows need is read once and
serves both, and a row of the pair outside the output range is summed and not stored.  As in test_gpu_tpi_wide_ring.py
the single-block call must take the wide ring (topo_amd_tpi_route == 1), the row-block calls the marching kernel (route 0),
and the two must agree bit for bit.  The rasters are whole metres with tens of kilometres of relief, so a prefix row
that serves the wrong run, or a row read from the wrong slot, cannot give the same sum.

The wide ring takes whole rasters only (its route asks for out_row0 == 0 and out_rows == gny), so what an output range
can do to a pair is to end in its middle: odd raster heights, where the last pair's first row is stored and its second
row masked.  Heights that end at a pair's end, a phase's end and a tile's end stand beside them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_twin, topo_oracle as orc

pytestmark = pytest.mark.gpu

from test_gpu_tpi_wide_ring import check_against_blocks, lattice_samples, tpi_blocks  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 67
RING = 99  # ring rows at 67 px (WideCfg::R): the tall rasters here are at least three times that


def relief_dem(gny, nx, seed):
    """Whole metres, tens of kilometres of relief (within the integer chain's range)."""
    rng = np.random.default_rng(seed)
    dem = orc.synthetic_dem(gny, nx, seed=seed).astype(np.float64)
    dem += rng.integers(-30000, 30000, size=(gny, nx))
    return np.ascontiguousarray(dem, dtype=np.float32)


def c_twin_tol(want):
    """The kernel rounds a float64 expression of exact integers to float32: half a float32 step of the result, the float64
    expression's own error (three roundings at 2^-53 of at most 2^16 m) and the twin's 1e-9 m (test_oracle_c_twin.py)."""
    return 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2e-9


@pytest.mark.parametrize("shape", [(297, 312), (299, 316), (301, 700), (313, 628), (335, 316), (384, 312), (385, 940)])
def test_pairs_heights_that_end_mid_pair(shape):
    """Heights 2 k + 1 (the last pair half inside), one past a phase (16 k + 1), one past a tile (64 k + 1), and even ones."""
    gny, nx = shape
    assert gny >= 3 * RING
    dem = relief_dem(gny, nx, seed=gny + nx)
    whole = check_against_blocks(dem, SIZE)
    want, _ = c_twin.tpi_std(dem, SIZE, want_std=False)
    assert np.all(np.abs(whole - want) <= c_twin_tol(want))


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, %(tests)r)
from test_gpu_tpi_wide_ring import tpi_blocks
from test_gpu_tpi_wide_ring_pairs import SIZE, relief_dem
gny, nx, seed = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
dem = relief_dem(gny, nx, seed)
whole = tpi_blocks(dem, SIZE, 1)
for nb in (2, 3):
    parts = tpi_blocks(dem, SIZE, nb)
    bad = ~((parts == whole) | (np.isnan(parts) & np.isnan(whole)))
    assert not bad.any(), (gny, nx, nb, int(bad.sum()), np.argwhere(bad)[:5].tolist())
print("ok", float(np.abs(whole).max()))
"""


@pytest.mark.parametrize("shape", [(1001, 640), (1523, 1000)])
def test_pairs_wrap_the_ring(shape):
    """Runs of many tiles per block (a grid sized for 8 compute units, in a fresh process): the pair's window takes every
    ring slot as its first, so its shared rows pass through every slot and every guard row.  Odd heights."""
    gny, nx = shape
    env = dict(os.environ, TOPO_AMD_CU_LIMIT="8")
    out = subprocess.run([sys.executable, "-c", _CHILD % {"repo": REPO, "tests": os.path.join(REPO, "tests")},
                          str(gny), str(nx), str(gny + nx)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout[-2000:]


def test_pairs_tall_raster_full_grid():
    """The same on the full grid: short runs that start at every tile row of a tall raster of odd height."""
    dem = relief_dem(1331, 1252, 11)
    check_against_blocks(dem, SIZE)


def test_pairs_beside_handed_over_phases():
    """Phases whose windows hold a NaN or a fractional sample are handed to the scaled pass and the general kernel; the
    phases next to them are computed, pairs and all.  The whole output equals the marching route's."""
    gny, nx = 451, 980
    dem = relief_dem(gny, nx, 41)
    dem[120, 333] = np.nan
    step = max(1, gny // 128)
    rows = np.arange(300, 331)
    rows = rows[rows % step != step // 2]  # off the class lattice: the raster stays "whole metres"
    dem[rows, 600:640] += 0.25
    lat = lattice_samples(dem)
    assert np.array_equal(lat[np.isfinite(lat)], np.trunc(lat[np.isfinite(lat)])), "the patch must not reach the lattice"
    whole = check_against_blocks(dem, SIZE)
    assert np.isnan(whole[120, 333]) and np.isnan(whole[120 + 33, 333]) and np.isfinite(whole[120 + 34, 333])
    # a computed phase well away from both, against the float64 twin on a crop that holds its discs
    crop = dem[180 - 33:260 + 34, 0:400]
    want, _ = c_twin.tpi_std(crop, SIZE, want_std=False)
    got = whole[180:260, 33:400 - 33]
    want = want[33:33 + 80, 33:400 - 33]
    assert np.all(np.abs(got - want) <= c_twin_tol(want))


@pytest.mark.parametrize("row", [150, 151, 152, 167, 176, 199, 230])
def test_pairs_one_loaded_row_at_a_time(row):
    """A raster that is zero but for ONE row of large values: an output row's disc sum then holds that row's prefix
    difference of exactly the runs that reach it, so a table entry that names the wrong loaded row for a run shows as a
    difference on a specific output row.  The row moves through both rows of a pair, a phase's edge and a tile's edge."""
    gny, nx = 331, 316
    rng = np.random.default_rng(row)
    dem = np.zeros((gny, nx), np.float32)
    dem[row] = rng.integers(10000, 30000, size=nx).astype(np.float32)
    whole = tpi_blocks(dem, SIZE, 1)
    want, _ = c_twin.tpi_std(dem, SIZE, want_std=False)
    bad = np.abs(whole - want) > c_twin_tol(want)
    assert not bad.any(), (row, sorted(set(np.argwhere(bad)[:, 0].tolist()))[:10])
    parts = tpi_blocks(dem, SIZE, 2)
    assert np.array_equal(parts, whole)
