"""The wide ring under its issue-priority ladder (csrc/disc_ring_wide_impl.hpp: WIDE_PRIO).

A chain wave lowers its priority 3 -> 2 -> 1 -> 0 over its sweep and a staging wave stands at 3 while it stages a batch.
Priorities reorder instruction issue and nothing else, so no bit can depend on them; what these cases guard is the rebuilt
kernel on the paths where the ladder's state is entered and left: sweep after sweep down long runs with a half-masked last
pair, computed phases directly before and after phases that run no sweep (the wave stays at 0 there), and chain waves
whose pair is in the output range in some phases and wholly outside it in the last.

In every test the single-block call must take the wide ring (topo_amd_tpi_route == 1: tpi_blocks asserts it) and equal
the two-block result of the marching kernel bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_tpi_wide_ring import lattice_samples, tpi_blocks  # noqa: E402
from test_gpu_tpi_wide_ring_pairs import relief_dem  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 67
GNY, NX, SEED = 401, 628, 1029  # two strips (312 + 312 of 628 columns, the second with 4 valid ones beside it), 401 = 16 k + 1


def same_bits(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, %(tests)r)
from oracle import c_twin
from topo_descriptors_amd import _lib
from test_gpu_tpi_wide_ring import tpi_blocks
from test_gpu_tpi_wide_ring_pairs import SIZE, c_twin_tol, relief_dem
assert _lib.lib().topo_amd_cu_count() == 8, "TOPO_AMD_CU_LIMIT did not take effect: the runs would be one tile long"
gny, nx, seed = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
dem = relief_dem(gny, nx, seed)
whole = tpi_blocks(dem, SIZE, 1)
parts = tpi_blocks(dem, SIZE, 2)
assert np.array_equal(parts, whole), np.argwhere(parts != whole)[:5].tolist()
want, _ = c_twin.tpi_std(dem, SIZE, want_std=False)
bad = np.abs(whole - want) > c_twin_tol(want)
assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
print("ok", float(np.abs(whole).max()))
"""


def test_long_runs_many_phases_last_pair_half_masked():
    """401 x 628 whole metres of relief on a grid sized for 8 compute units (a fresh process): a block runs down many tiles,
    a chain wave climbs and leaves the ladder phase after phase, and the odd height masks the second row of the last pair.
    Route 1, the two-block marching result's bits, and the float64 twin within c_twin_tol."""
    env = dict(os.environ, TOPO_AMD_CU_LIMIT="8")
    out = subprocess.run([sys.executable, "-c", _CHILD % {"repo": REPO, "tests": os.path.join(REPO, "tests")},
                          str(GNY), str(NX), str(SEED)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout[-2000:]


def test_computed_phases_around_handed_over_ones():
    """The same raster with one NaN and a 0.25 m patch off the class lattice: the phases whose windows hold them run no
    sweep (their chain waves never raise themselves), and computed phases lie directly before and after them."""
    dem = relief_dem(GNY, NX, SEED)
    dem[90, 200] = np.nan
    step = max(1, GNY // 128)
    rows = np.arange(270, 290)
    rows = rows[rows % step != step // 2]  # off the class lattice: the raster stays "whole metres"
    dem[rows, 400:440] += 0.25
    lat = lattice_samples(dem)
    assert np.array_equal(lat[np.isfinite(lat)], np.trunc(lat[np.isfinite(lat)])), "the patch must not reach the lattice"
    whole = tpi_blocks(dem, SIZE, 1)
    parts = tpi_blocks(dem, SIZE, 2)
    assert same_bits(parts, whole).all(), np.argwhere(~same_bits(parts, whole))[:5].tolist()
    assert np.isnan(whole[90, 200]) and np.isfinite(whole[90 + SIZE // 2 + 1, 200])


def test_pairs_in_range_then_wholly_outside():
    """297 x 312, one strip: 297 = 18 x 16 + 9, so in the last phase the pairs of rows 0 .. 7 are summed, the pair of rows
    8 / 9 is half masked and the chain waves of rows 10 .. 15 sweep nothing, after eighteen phases in which every chain
    wave swept."""
    dem = relief_dem(297, 312, 609)
    whole = tpi_blocks(dem, SIZE, 1)
    parts = tpi_blocks(dem, SIZE, 2)
    assert np.array_equal(parts, whole), np.argwhere(parts != whole)[:5].tolist()
