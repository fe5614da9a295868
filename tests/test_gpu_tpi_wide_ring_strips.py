"""The wide ring's strips of 316 valid columns (csrc/disc_ring_wide_impl.hpp, WGeo::XV).

A strip stages 384 columns and stores the outputs at staged columns 34 .. 349: the 52 whole lanes 6 .. 57, the last
pair of lane 5 and the first pair of lane 58.  Those two lanes take nothing from beyond the wave's ends in the columns
they store (WSweep::edges_valid), so the bits must be what they were with strips of 312.

The reference is the marching route on the same raster: a child process started with TOPO_AMD_TPI_WIDE_RING=0 (the
switch is read once, when the library first dispatches a disc) computes every case of a group in one go, and each of its
calls asserts route 0.  Every call on this side asserts route 1.  Planes agree bit for bit, NaN for NaN.

  * widths 316 (one strip, exactly full), 320 (a second strip of four columns), 632, 636 and 312 (a partly filled strip),
    heights 96 and 200, whole metres: the marching route's bits and the float64 oracle;
  * one bad sample (NaN, +inf, 0.5, 300000) at global column 314, 315, 316 or 317 - the half-valid lanes 58 of strip 0
    and 5 of strip 1 - in row 0, 15, 16, 33 or the last row of a 96 x 896 raster.  896 columns put the class lattice
    (csrc/raster_class.hip: every seventh column from column 3) beside all four columns, so the raster stays "whole
    metres" and the single-block call takes the wide ring;
  * long runs: 1700 x 320 on a grid sized for 8 compute units (TOPO_AMD_CU_LIMIT, a fresh process), 27 tiles a strip and
    about 7 a block: a run's phases take the pairs' first slots (13 + 16 ph + j, j even, modulo the ring's 99) through
    every residue, so the chain waves' fetches cross the wrap and the guard rows at every offset.  Whole metres; a bad
    sample in row 215, which the run from row 0 stages in its phase 10 (rows 209 .. 224) so that phase 11 sees it first
    as its newest batch; and one in row 199, a batch earlier.  Both lie beside the class lattice (rows 6 + 13 k, odd columns)."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import c_twin, topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import device as d  # noqa: E402
from test_gpu_tpi_wide_ring import lattice_samples  # noqa: E402
from test_gpu_tpi_wide_ring_pairs import c_twin_tol  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 67
M = SIZE // 2
WIDTHS = [316, 320, 632, 636, 312]
HEIGHTS = [96, 200]
BAD = {"nan": np.float32(np.nan), "inf": np.float32(np.inf), "half": np.float32(0.5), "300000": np.float32(300000.0)}
BAD_COLS = [314, 315, 316, 317]
BAD_NY, BAD_NX = 96, 896
BAD_ROWS = [0, 15, 16, 33, BAD_NY - 1]
LONG_NY, LONG_NX = 1700, 320
LONG_CASES = {"whole": None, "newest_batch": (215, 316), "batch_earlier": (199, 316)}


def dem_of(ny, nx):
    dem = orc.synthetic_dem(ny, nx, seed=ny + nx)
    assert dem.dtype == np.float32 and np.array_equal(dem, np.trunc(dem))
    return dem


def with_sample(dem, row, col, value):
    out = dem.copy()
    out[row, col] = value
    lat = lattice_samples(out)
    assert np.array_equal(lat, np.trunc(lat)), "the sample must lie beside the class lattice (else the marching route runs)"
    return out


_CHILD = r"""
import json, sys
import numpy as np
from topo_descriptors_amd import _lib, device as d
spec = json.loads(sys.argv[1])
if spec["cus"]:
    assert _lib.lib().topo_amd_cu_count() == spec["cus"], "TOPO_AMD_CU_LIMIT did not take effect"
out = {}
with np.load(spec["dems"]) as z:
    for name in z.files:
        dem = z[name]
        dev = d.DeviceArray.from_host(dem)
        t = d.DeviceArray(*dem.shape)
        d.Block(dev, row0=0, gny=dem.shape[0]).tpi_std(67, tpi=t, out_row0=0, out_rows=dem.shape[0])
        d.sync()
        assert d.tpi_route() == spec["route"], (name, d.tpi_route(), spec["route"])
        out[name] = t.to_host()
        t.free()
        dev.free()
np.savez(spec["out"], **out)
print("DONE", len(out))
"""


def planes_in_child(dems, route, cus=0):
    """TPI of every raster of `dems` (name -> array) in ONE fresh process: route 0 with the wide ring switched off, route 1
    (and a grid for `cus` compute units) otherwise."""
    with tempfile.TemporaryDirectory() as tmp:
        dem_path, out_path = os.path.join(tmp, "dems.npz"), os.path.join(tmp, "planes.npz")
        np.savez(dem_path, **dems)
        env = dict(os.environ)
        if route == 0:
            env["TOPO_AMD_TPI_WIDE_RING"] = "0"
        if cus:
            env["TOPO_AMD_CU_LIMIT"] = str(cus)
        spec = {"dems": dem_path, "out": out_path, "route": route, "cus": cus}
        run = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(spec)], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        with np.load(out_path) as z:
            return {k: z[k] for k in z.files}


def tpi_wide(dem):
    dev = d.DeviceArray.from_host(dem)
    t = d.DeviceArray(*dem.shape)
    d.Block(dev, row0=0, gny=dem.shape[0]).tpi_std(SIZE, tpi=t, out_row0=0, out_rows=dem.shape[0])
    d.sync()
    assert d.tpi_route() == 1, "the single-block call did not take the wide ring"
    out = t.to_host()
    t.free()
    dev.free()
    return out


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def footprint(shape, row, col):
    """The pixels whose disc holds (row, col)."""
    k = orc.circular_kernel(SIZE) > 0
    out = np.zeros(shape, bool)
    for a, b in np.argwhere(k) - M:
        if 0 <= row + a < shape[0] and 0 <= col + b < shape[1]:
            out[row + a, col + b] = True
    return out


@functools.lru_cache(maxsize=None)
def marching_whole():
    return planes_in_child({f"{ny}x{nx}": dem_of(ny, nx) for ny in HEIGHTS for nx in WIDTHS}, 0)


@pytest.mark.parametrize("nx", WIDTHS)
@pytest.mark.parametrize("ny", HEIGHTS)
def test_strip_widths_whole_metres(ny, nx):
    dem = dem_of(ny, nx)
    wide = tpi_wide(dem)
    march = marching_whole()[f"{ny}x{nx}"]
    assert np.array_equal(wide.view(np.uint32), march.view(np.uint32)), np.argwhere(wide != march)[:5]
    err = np.max(np.abs(wide - orc.tpi_exact(dem, SIZE)))
    print(f"{ny} x {nx}: max err against float64 {err:.3e} m")
    assert err <= 2.5e-4


def bad_dems(name, col):
    base = dem_of(BAD_NY, BAD_NX)
    return {f"{name}-{col}-{row}": with_sample(base, row, col, BAD[name]) for row in BAD_ROWS}


@functools.lru_cache(maxsize=None)
def marching_bad():
    dems = {}
    for name in BAD:
        for col in BAD_COLS:
            dems.update(bad_dems(name, col))
    return planes_in_child(dems, 0)


@pytest.mark.parametrize("col", BAD_COLS)
@pytest.mark.parametrize("name", list(BAD))
def test_bad_sample_in_a_half_valid_lane(name, col):
    for key, dem in bad_dems(name, col).items():
        row = int(key.rsplit("-", 1)[1])
        wide = tpi_wide(dem)
        ok = same_bits(wide, marching_bad()[key])
        assert ok.all(), (key, np.argwhere(~ok)[:5])
        if name == "nan":
            assert np.array_equal(np.isnan(wide), footprint(dem.shape, row, col)), key


def long_dems():
    base = dem_of(LONG_NY, LONG_NX)
    out = {}
    for name, pos in LONG_CASES.items():
        if pos is None:
            out[name] = base
        else:
            for kind in ("nan", "half"):
                out[f"{name}-{kind}"] = with_sample(base, pos[0], pos[1], BAD[kind])
    return out


def test_long_runs_cross_every_ring_residue():
    dems = long_dems()
    wide = planes_in_child(dems, 1, cus=8)
    march = planes_in_child(dems, 0)
    for key, dem in dems.items():
        ok = same_bits(wide[key], march[key])
        assert ok.all(), (key, np.argwhere(~ok)[:5])
        if key.endswith("-nan"):
            pos = LONG_CASES[key.rsplit("-", 1)[0]]
            assert np.array_equal(np.isnan(wide[key]), footprint(dem.shape, *pos)), key
    want, _ = c_twin.tpi_std(dems["whole"], SIZE, want_std=False)
    assert np.all(np.abs(wide["whole"] - want) <= c_twin_tol(want))
