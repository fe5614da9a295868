"""The wide ring's output rows when nothing waits for their stores (csrc/disc_ring_wide_impl.hpp).

A chain wave no longer drains its six output stores in front of the phase barrier: they are in flight while the next
sweep overwrites the registers they were issued from, and while the staging waves overwrite the ring rows the finished
phase read.  What a stored value is made of - the disc sum and the pixel's own sample, the difference of prefix rows M
and M + 1 (row A of a pair) or M + 1 and M + 2 (row B) of the pair's window - must be what the marching kernel and the
float64 twin give, on every row of a pair, in every ring slot, next to phases that run no sweep and in a pair whose second
row is masked.

In every test the single-block call must take the wide ring (topo_amd_tpi_route == 1: tpi_blocks asserts it), equal the
two-block result of the marching kernel bit for bit, and the C twin within c_twin_tol."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_twin

pytestmark = pytest.mark.gpu

from test_gpu_tpi_wide_ring import lattice_samples, tpi_blocks  # noqa: E402
from test_gpu_tpi_wide_ring_pairs import c_twin_tol, relief_dem  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 67
M = SIZE // 2


def same_bits(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("row", [150, 151, 166, 167])
def test_own_sample_on_both_rows_of_a_pair_and_across_a_phase_edge(row):
    """Zero but for one row of large values: on that output row the pixel's own sample is the whole of x, and on the rows
    beside it none of it.  Rows 150 / 151 are the two rows of one pair, 166 / 167 those of the pair that ends a phase and
    the one that begins the next (the strip's phases start at multiples of 16)."""
    gny, nx = 331, 316
    rng = np.random.default_rng(row)
    dem = np.zeros((gny, nx), np.float32)
    dem[row] = rng.integers(10000, 30000, size=nx).astype(np.float32)
    whole = tpi_blocks(dem, SIZE, 1)
    parts = tpi_blocks(dem, SIZE, 2)
    assert np.array_equal(parts, whole)
    want, _ = c_twin.tpi_std(dem, SIZE, want_std=False)
    bad = np.abs(whole - want) > c_twin_tol(want)
    assert not bad.any(), (row, sorted(set(np.argwhere(bad)[:, 0].tolist()))[:10])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, %(tests)r)
from oracle import c_twin
from test_gpu_tpi_wide_ring import tpi_blocks
from test_gpu_tpi_wide_ring_pairs import SIZE, c_twin_tol, relief_dem
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


def test_own_rows_through_every_ring_slot():
    """Runs of many tiles per block (a grid sized for 8 compute units, in a fresh process): the pair's window takes every
    ring slot as its first, so the three rows the own samples are made of pass through every slot and every guard row,
    and the staging waves overwrite each of them while the stores of the phase that read it are still in flight."""
    gny, nx = 1001, 640
    env = dict(os.environ, TOPO_AMD_CU_LIMIT="8")
    out = subprocess.run([sys.executable, "-c", _CHILD % {"repo": REPO, "tests": os.path.join(REPO, "tests")},
                          str(gny), str(nx), str(gny + nx)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout[-2000:]


def test_computed_phases_behind_handed_over_ones():
    """One NaN and one fractional patch, as in test_pairs_beside_handed_over_phases: the phases whose windows hold them run
    no sweep and store nothing, and the computed phases behind them follow a phase boundary that no store crossed."""
    gny, nx = 451, 980
    clean = relief_dem(gny, nx, 41)
    dem = clean.copy()
    dem[120, 333] = np.nan
    step = max(1, gny // 128)
    rows = np.arange(300, 331)
    rows = rows[rows % step != step // 2]  # off the class lattice: the raster stays "whole metres"
    dem[rows, 600:640] += 0.25
    lat = lattice_samples(dem)
    assert np.array_equal(lat[np.isfinite(lat)], np.trunc(lat[np.isfinite(lat)])), "the patch must not reach the lattice"
    whole = tpi_blocks(dem, SIZE, 1)
    parts = tpi_blocks(dem, SIZE, 2)
    assert same_bits(parts, whole).all(), np.argwhere(~same_bits(parts, whole))[:5].tolist()
    assert np.isnan(whole[120, 333]) and np.isnan(whole[120 + M, 333]) and np.isfinite(whole[120 + M + 1, 333])
    # every pixel whose disc holds neither: its disc is the clean raster's, whichever kernel took it
    far = np.ones(dem.shape, bool)
    far[120 - M:120 + M + 1, 333 - M:333 + M + 1] = False
    far[300 - M:331 + M, 600 - M:640 + M] = False
    want, _ = c_twin.tpi_std(clean, SIZE, want_std=False)
    bad = far & ~(np.abs(whole - want) <= c_twin_tol(want))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    # rows of computed phases right behind the handed-over ones are among them
    assert far[120 + 2 * M + 16:300 - 2 * M - 16].all()


@pytest.mark.parametrize("shape", [(297, 316), (385, 316)])
def test_last_pair_half_masked(shape):
    """Odd heights: the last pair's first row is stored and its second row masked (297 = 16 k + 9, 385 = 64 k + 1)."""
    gny, nx = shape
    dem = relief_dem(gny, nx, seed=gny + nx)
    whole = tpi_blocks(dem, SIZE, 1)
    parts = tpi_blocks(dem, SIZE, 2)
    assert np.array_equal(parts, whole)
    want, _ = c_twin.tpi_std(dem, SIZE, want_std=False)
    assert np.all(np.abs(whole - want) <= c_twin_tol(want))
