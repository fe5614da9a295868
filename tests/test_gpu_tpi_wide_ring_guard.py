"""The wide ring's wrap and guard rows (csrc/disc_ring_wide_impl.hpp: a ring of R = SIZE + 32 prefix rows plus GR guard
rows, read through a few VGPR bases with immediate row offsets).

A row of the chain reads Q indices 0 .. SIZE of its window at slot (s0 + k) mod R.  A base that sits in the last GR slots
of the ring reaches past slot R - 1 into the guard rows, which must hold copies of slots 0 .. GR - 1 at that moment.  The
rasters here are tall (well over 1,000 rows, heights no multiple of 16 or 64) and carry a relief of tens of kilometres in
whole metres, so a row read from a wrong slot cannot give the same sum.  In a fresh process whose persistent grid is
sized for 8 compute units (TOPO_AMD_CU_LIMIT), each block takes a run of many tiles that starts mid-strip and carries
the ring round it several times, so s0 takes every slot value.  The single-block call (the wide ring, asserted through
topo_amd_tpi_route) must give the bits of the stitched row-block calls (the marching kernel), and a few pixels must
match the float64 oracle on a crop that holds their disc."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 67


def relief_dem(gny, nx, seed):
    """Whole metres, tens of kilometres of relief (within the integer chain's range)."""
    rng = np.random.default_rng(seed)
    dem = orc.synthetic_dem(gny, nx, seed=seed).astype(np.float64)
    dem += rng.integers(-30000, 30000, size=(gny, nx))
    return np.ascontiguousarray(dem, dtype=np.float32)


def spot_points(gny, nx, seed, n=6):
    rng = np.random.default_rng(seed + 1)
    m = SIZE // 2
    return [(int(rng.integers(m, gny - m)), int(rng.integers(m, nx - m))) for _ in range(n)] + [(gny - m - 1, nx - m - 1)]


def oracle_at(dem, r, c):
    """float64 TPI of pixel (r, c), at least SIZE // 2 from every border, from a crop that holds its disc."""
    m = SIZE // 2
    return float(orc.tpi_exact(dem[r - m:r + m + 1, c - m:c + m + 1], SIZE)[m, m])


def tol_at(want):
    return 4.0 * float(np.spacing(np.float32(abs(want)))) + 2.5e-4


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, %(tests)r)
from test_gpu_tpi_wide_ring import tpi_blocks
from test_gpu_tpi_wide_ring_guard import SIZE, oracle_at, relief_dem, spot_points, tol_at
gny, nx, seed = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
dem = relief_dem(gny, nx, seed)
whole = tpi_blocks(dem, SIZE, 1)
for nb in (2, 3):
    parts = tpi_blocks(dem, SIZE, nb)
    bad = ~((parts == whole) | (np.isnan(parts) & np.isnan(whole)))
    assert not bad.any(), (gny, nx, nb, int(bad.sum()), np.argwhere(bad)[:5].tolist())
for r, c in spot_points(gny, nx, seed):
    want = oracle_at(dem, r, c)
    assert abs(float(whole[r, c]) - want) <= tol_at(want), (r, c, float(whole[r, c]), want)
print("ok", float(np.abs(whole).max()))
"""


@pytest.mark.parametrize("shape", [(1237, 1000), (1509, 640), (2003, 1252)])
def test_wide_ring_long_runs_wrap_the_ring(shape):
    """Runs of many tiles per block (8-CU grid): every ring slot as s0, the guard rows read at every wrap position."""
    gny, nx = shape
    env = dict(os.environ, TOPO_AMD_CU_LIMIT="8")
    out = subprocess.run([sys.executable, "-c", _CHILD % {"repo": REPO, "tests": os.path.join(REPO, "tests")},
                          str(gny), str(nx), str(gny + nx)], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout[-2000:]


def test_wide_ring_tall_raster_full_grid():
    """The same on the full grid: short runs that start at every tile row of a tall raster."""
    from test_gpu_tpi_wide_ring import check_against_blocks

    gny, nx = 1330, 1572
    dem = relief_dem(gny, nx, 7)
    whole = check_against_blocks(dem, SIZE)
    for r, c in spot_points(gny, nx, 7):
        want = oracle_at(dem, r, c)
        assert abs(float(whole[r, c]) - want) <= tol_at(want), (r, c, float(whole[r, c]), want)
