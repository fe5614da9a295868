"""The staging of the wide ring (csrc/disc_ring_wide_impl.hpp, stage_batch / load_batch) at the shapes where it can go wrong.

A staging wave takes a batch of 16 rows either on the lean path (all rows in the raster, all of the wave's lanes in it, the
batch's ring slots not wrapping) or on the general one, and copies the slots below GR = 6 into the guard rows behind the
ring.

Small rasters (test_whole_metres, test_one_bad_sample): one strip (312 columns), a second strip of 4 valid columns whose
staging lanes are mostly outside the raster (316), and 632 columns - two full strips and a third of 8 columns; heights of
less than a batch, one batch, one window, one ring (R = 99), and 230 rows.  The grid has a block for every tile of these
rasters, so every 64-row tile is a run of its own: 6 prologue batches and 4 phase batches, ring slots 0, 16, ... 96, 13,
29, 45 for the batches' first rows.  They meet the raster's rim on every side, lanes outside the raster, the batch that
wraps the ring (slots 96 .. 98, 0 .. 12) and the guard copies of a whole range (slots 0 .. 5) - and no other residue of a
batch against the ring.

Long runs (test_long_runs_*): a child process whose grid is limited to 8 blocks (TOPO_AMD_CU_LIMIT, read when the library
starts; the ring fills a compute unit's LDS, so a block per unit) computes a 6144 x 316 raster: 192 tiles, 24 to a block,
runs of 6 + 96 batches.  The first row of batch b sits in slot 16 b mod 99, which takes every value over a run: the guard
copies of a partial range (slots w .. 5 for a batch that starts at w = 1 .. 5, slots 0 .. w - 84 for one that starts at
84 .. 88), and the lean path's wrap test at every slot.

Every case is a single-block call that must report the wide ring, and is held to
  * the float64 oracle within the bounds of include/topo_amd.h: float32 rounding where the disc holds whole metres, 2^-9 m
    more where it holds a fractional sample, NaN exactly where it holds a non-finite one (the long raster: on windows);
  * bit for bit, the same raster computed as two row blocks, which take the marching kernel (a raster of one row cannot be
    split: it is held to the oracle alone).
A bad sample (0.5, NaN, 300000 - beyond kAbsLim) sits where the staging treats rows and columns differently; stream row n of
the run that starts at the raster's top is DEM row n - 47 (gy0 = -M - PAD = -33 - 14), a batch is n = 16 k .. 16 k + 15, and
the rows with n mod 99 < 6 are the guard-copied ones.  The raster class is taken on a lattice (csrc/raster_class.hip: every
row of the small rasters, every second or fourth column), so the bad samples sit beside the lattice's columns and the class
stays "whole metres".  The dem_memo tile report is not exposed by the library's interface, so it is not compared here."""
import functools

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import _lib, device as d, shard  # noqa: E402

SIZE, M = 67, 33
GY0 = -(M + 14)  # DEM row of stream row 0 for the run at the raster's top (PAD = 14 at 67 px)
WIDTHS = [312, 316, 632]
HEIGHTS = [1, 16, 66, 99, 115, 230]


@functools.lru_cache(maxsize=None)
def base_dem(gny, nx):
    """Whole metres, about -1100 .. 900 m."""
    dem = orc.synthetic_dem(gny, nx, seed=gny + nx) - np.float32(2000.0)
    dem.setflags(write=False)
    return dem


@functools.lru_cache(maxsize=None)
def base_exact(gny, nx):
    out = orc.tpi_exact(base_dem(gny, nx), SIZE)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def base_wide(gny, nx):
    """The wide ring's TPI of the whole-metre raster."""
    out = tpi_blocks(base_dem(gny, nx), 1)
    out.setflags(write=False)
    return out


def on_lattice(gny, nx, row, col):
    sr, sc = max(1, gny // 128), max(1, nx // 128)
    return row % sr == sr // 2 and col % sc == sc // 2


def tpi_blocks(dem, nblocks):
    """tests/test_gpu_tpi_wide_ring.py, tpi_blocks: one block takes the wide ring, a row block the marching kernel."""
    gny, nx = dem.shape
    up, down = shard.halo_rows(_lib.DESC_TPI, SIZE)
    pieces = []
    for row0, rows in shard.split_rows(gny, nblocks):
        lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
        dev = d.DeviceArray.from_host(dem[lo:hi])
        blk = d.Block(dev, row0=lo, gny=gny)
        t = d.DeviceArray(rows, nx)
        blk.tpi_std(SIZE, tpi=t, out_row0=row0, out_rows=rows)
        d.sync()
        assert d.tpi_route() == (1 if nblocks == 1 else 0), (dem.shape, nblocks)
        pieces.append(t.to_host())
        t.free()
        dev.free()
    return np.concatenate(pieces, axis=0)


def disc_mask(shape, row, col):
    """The outputs whose disc holds the sample (row, col)."""
    jj = np.arange(shape[0])[:, None] - row
    ii = np.arange(shape[1])[None, :] - col
    return jj * jj + ii * ii <= M * M  # (the oracle's circular_kernel: d2 <= m^2)


def check(dem, exact, frac_at=None):
    whole = tpi_blocks(dem, 1)
    nan_want = np.isnan(exact)
    assert np.array_equal(np.isnan(whole), nan_want), np.argwhere(np.isnan(whole) != nan_want)[:5]
    # float32 rounding of the exact value: half a unit in the last place, and as much again for the float64 evaluation that
    # is rounded; a fractional sample in the disc: 2^-9 m on top (include/topo_amd.h)
    tol = np.abs(np.where(nan_want, 0.0, exact)) * 2.0 ** -23 + 1e-6
    if frac_at is not None:
        tol = tol + np.where(disc_mask(dem.shape, *frac_at), 2.0 ** -9, 0.0)
    err = np.abs(np.where(nan_want, 0.0, whole.astype(np.float64) - exact))
    print(f"max err {err.max():.3e} m, max err / tol {np.max(err / tol):.3f}")
    assert (err <= tol).all(), (np.argwhere(err > tol)[:5], err.max())
    if dem.shape[0] >= 2:
        parts = tpi_blocks(dem, 2)
        bad = ~((parts == whole) | (np.isnan(parts) & np.isnan(whole)))
        assert not bad.any(), np.argwhere(bad)[:5]
    return whole


@pytest.mark.parametrize("nx", WIDTHS)
@pytest.mark.parametrize("gny", HEIGHTS)
def test_whole_metres(gny, nx):
    check(base_dem(gny, nx), base_exact(gny, nx))


def stream_row(n):
    return GY0 + n


# (raster, row, column): the rows and columns where the staging changes its treatment, paired so that each occurs.  Stream
# rows are those of the run of the tile at the raster's top (n = 0 .. 159); the run of the tile below it starts 64 rows on.
GNY = 230
BAD_AT = [
    (632, 0, 0),                      # the raster's first row and column
    (632, GNY - 1, 631),              # ... and its last ones
    (632, stream_row(64), 91),        # first row of a batch; last column of staging wave 0's share (strip 0: columns -36 ..)
    (632, stream_row(63), 92),        # last row of a batch; first column of wave 1's share
    (632, stream_row(99), 219),       # slot 0 of the ring's second turn (guard-copied); last column of wave 1's share
    (632, stream_row(104), 220),      # slot 5, the last guard-copied one; first column of wave 2's share
    (632, stream_row(105), 403),      # the first slot without a guard copy; last column of wave 0's share in strip 1
    (632, 151, 404),                  # n = 6 of the bottom tile's run: its first slot without a guard copy; wave 1 of strip 1
    (632, 156, 311),                  # n = 11 of that run (n = 75 and 139 of the two above it); the last column of strip 0's outputs
    (632, stream_row(112), 312),      # first row behind the batch that wraps the ring (n = 96 .. 111); strip 1's first column
    (316, stream_row(99), 312),       # the second strip's four columns: one staging lane inside the raster
    (316, GNY - 1, 314),
    (316, stream_row(64), 0),
    (312, stream_row(63), 0),         # one strip
    (312, stream_row(104), 310),
]
BAD_VALUES = {"half": 0.5, "nan": np.nan, "absurd": 300000.0}


@pytest.mark.parametrize("nx,row,col", BAD_AT)
@pytest.mark.parametrize("kind", list(BAD_VALUES))
def test_one_bad_sample(kind, nx, row, col):
    assert 0 <= row < GNY and 0 <= col < nx and not on_lattice(GNY, nx, row, col), "a position beside the class lattice"
    dem = base_dem(GNY, nx).copy()
    dem[row, col] = BAD_VALUES[kind]
    # the oracle of this raster from the shared one: only the discs that hold the sample change, by the sample's difference
    # over the disc's 3408 neighbours (and the pixel's own value at the sample)
    exact = base_exact(GNY, nx).copy()
    taps = int(np.count_nonzero(orc.circular_kernel(SIZE))) - 1
    delta = float(dem[row, col]) - float(base_dem(GNY, nx)[row, col])
    hit = disc_mask(dem.shape, row, col)
    hit_n = hit.copy()
    hit_n[row, col] = False
    exact[hit_n] -= delta / taps
    exact[row, col] += delta
    whole = check(dem, exact, frac_at=(row, col) if kind == "half" else None)
    if kind == "nan":
        assert np.isnan(whole[hit]).all() and np.isfinite(whole[~hit]).all()
    # a window without the sample keeps the whole-metre raster's bits
    assert np.array_equal(whole[~hit], base_wide(GNY, nx)[~hit])


# ---- long runs: every residue of a batch against the ring ------------------------------------------------------------------
LONG_NY, LONG_NX = 6144, 316  # 2 strips x 96 tiles: 24 tiles to each of 8 blocks


def long_row(b, r):
    """DEM row of row r of batch b in the run at the raster's top."""
    return GY0 + 16 * b + r


# (batch of the top run, row in it, column): the batch starts at slot w = 16 b mod 99
LONG_AT = [
    (31, 0, 0),     # w = 1: slots 1 .. 5 guard-copied; the first of them
    (31, 4, 92),    # ... slot 5, the last
    (31, 5, 310),   # ... slot 6, the first without a copy
    (25, 1, 312),   # w = 4: slot 5; the second strip
    (56, 0, 312),   # w = 5: slot 5, the only guard-copied one
    (30, 15, 314),  # w = 84: the batch's last row wraps into slot 0, the only guard-copied one
    (24, 12, 92),   # w = 87: slot 0, the first behind the wrap
    (55, 11, 310),  # w = 88: slot 0
    (55, 15, 0),    # ... slot 4, the last
]

_LONG_CHILD = r"""
import json, sys
import numpy as np
from oracle import topo_oracle as orc
from topo_descriptors_amd import _lib, device as d, shard
assert _lib.lib().topo_amd_cu_count() == 8, "TOPO_AMD_CU_LIMIT did not take effect: the runs would be one tile long"
spec = json.loads(sys.argv[1])
ny, nx, SIZE, M = spec["ny"], spec["nx"], 67, 33
VALUES = {"half": 0.5, "nan": float("nan"), "absurd": 300000.0}

def blocks(dem, nblocks):
    up, down = shard.halo_rows(_lib.DESC_TPI, SIZE)
    pieces = []
    for row0, rows in shard.split_rows(ny, nblocks):
        lo, hi = max(0, row0 - up), min(ny, row0 + rows + down)
        dev = d.DeviceArray.from_host(dem[lo:hi])
        t = d.DeviceArray(rows, nx)
        d.Block(dev, row0=lo, gny=ny).tpi_std(SIZE, tpi=t, out_row0=row0, out_rows=rows)
        d.sync()
        assert d.tpi_route() == (1 if nblocks == 1 else 0), nblocks
        pieces.append(t.to_host())
        t.free()
        dev.free()
    return np.concatenate(pieces, axis=0)

def same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())

def ratio(got, exact, frac_hit=None):
    # the bound of check() above: float32 rounding of the exact value, 2^-9 m more where the disc holds a fractional sample
    nan = np.isnan(exact)
    tol = np.abs(np.where(nan, 0.0, exact)) * 2.0 ** -23 + 1e-6
    if frac_hit is not None:
        tol = tol + np.where(frac_hit, 2.0 ** -9, 0.0)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    return float(np.max(np.abs(np.where(nan, 0.0, got.astype(np.float64) - exact)) / tol))

base = orc.synthetic_dem(ny, nx, seed=11) - np.float32(2000.0)
wide0 = blocks(base, 1)
out = {"base_bits": same(wide0, blocks(base, 2)), "cases": {}}
taps = int(np.count_nonzero(orc.circular_kernel(SIZE))) - 1
worst = 0.0
for row, col in spec["at"]:
    # the oracle on a window of rows whose discs lie inside it (or reach the raster's top)
    j0, j1 = max(0, row - 80), min(ny, row + 81)
    a, b = (0 if j0 == 0 else j0 + M), (ny if j1 == ny else j1 - M)
    exact0 = orc.tpi_exact(base[j0:j1], SIZE)[a - j0:b - j0]
    worst = max(worst, ratio(wide0[a:b], exact0))
    jj = np.arange(a, b)[:, None] - row
    ii = np.arange(nx)[None, :] - col
    hit_w = jj * jj + ii * ii <= M * M
    hit = np.zeros((ny, nx), bool)
    hit[a:b] = hit_w
    for kind, v in VALUES.items():
        dem = base.copy()
        dem[row, col] = v
        delta = float(dem[row, col]) - float(base[row, col])
        exact = exact0.copy()
        exact[hit_w] -= delta / taps
        exact[row - a, col] += delta + delta / taps
        whole = blocks(dem, 1)
        out["cases"][f"{kind}-{row}-{col}"] = {
            "bits": same(whole, blocks(dem, 2)),
            "ratio": ratio(whole[a:b], exact, hit_w if kind == "half" else None),
            "clean_elsewhere": bool(np.array_equal(whole[~hit], wide0[~hit])),
            "nan_footprint": bool(np.array_equal(np.isnan(whole), hit)) if kind == "nan" else bool(not np.isnan(whole).any())}
out["base_ratio"] = worst
print("RESULT", json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def long_runs():
    """One child process for all the long-run cases (the grid limit is read when the library starts)."""
    import json
    import os
    import subprocess
    import sys
    spec = {"ny": LONG_NY, "nx": LONG_NX, "at": [(long_row(b, r), col) for b, r, col in LONG_AT]}
    env = dict(os.environ, TOPO_AMD_CU_LIMIT="8")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", _LONG_CHILD, json.dumps(spec)], cwd=root, env=env, capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout.strip().splitlines()[-1].split(" ", 1)[1])


def test_long_runs_whole_metres():
    res = long_runs()
    print(f"max err / tol {res['base_ratio']:.3f}")
    assert res["base_bits"], "the wide ring's bits differ from the marching kernel's"
    assert res["base_ratio"] <= 1.0, res["base_ratio"]


@pytest.mark.parametrize("b,r,col", LONG_AT)
@pytest.mark.parametrize("kind", list(BAD_VALUES))
def test_long_runs_one_bad_sample(kind, b, r, col):
    row = long_row(b, r)
    assert 1 <= (16 * b) % 99 <= 5 or 84 <= (16 * b) % 99 <= 88, "a batch with a partial guard range"
    assert 0 <= row < LONG_NY and not on_lattice(LONG_NY, LONG_NX, row, col), "a position beside the class lattice"
    res = long_runs()["cases"][f"{kind}-{row}-{col}"]
    print(f"max err / tol {res['ratio']:.3f}")
    assert res["bits"], "the wide ring's bits differ from the marching kernel's"
    assert res["nan_footprint"], "NaN exactly where the disc holds the non-finite sample"
    assert res["ratio"] <= 1.0, res["ratio"]
    assert res["clean_elsewhere"], "a window without the sample keeps the whole-metre raster's bits"
