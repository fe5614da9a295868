"""The wide ring's classification of staged samples (csrc/wide_classify.hpp, called from stage_batch of
csrc/disc_ring_wide_impl.hpp): fractional parts ORed and a float maximum of magnitudes instead of a convert back and a compare
per sample.  Which windows the ring computes and which it leaves to the scaled pass and the general kernel must be what it
was, for every kind of float32 a DEM can hold.

The raster is 256 rows x 704 columns of whole metres: three strips of 312 output columns, staged columns -36 .. 347,
276 .. 659 and 588 .. 971.  The middle strip lies inside the raster, so its batches of 16 interior rows take the lean
staging path; the first strip and the partial last one stage on the general path, as does every batch that meets the
raster's first or last rows.  A special value sits
  * at row 100, column 10: the first strip, general path;
  * at row 100, column 400: the middle strip, in the interior batch of rows 97 .. 112 (the runs of the tiles at rows 0 and 64
    stage it at ring slots 45 and 80: no wrap), lean path;
  * in the raster's last row, at column 10 and at column 400: a batch that runs beyond the raster, general path in every strip.
These positions lie beside the lattice the raster class is taken on (csrc/raster_class.hip: every second row, every fifth
column here), so the class stays "whole metres" and the single-block call takes the wide ring: every call asserts
topo_amd_tpi_route.

The reference is the marching route on the same raster: a child process started with TOPO_AMD_TPI_WIDE_RING=0 (the switch
is read once, when the library first dispatches a disc) computes every case in one go, and each of its calls asserts
route 0.  The planes must agree bit for bit, NaN for NaN.  The DEM memo's count of fractional tiles is not exposed by the
library's interface (include/topo_amd.h), so it is not compared; nor is the map of deferred tiles, so the clean raster is
held to what can be seen of it: the marching route's bits and the float64 oracle within float32 rounding, with no allowance
for the scaled pass.

test_lab_program builds tools/ubench/classify_lab.hip and runs it once: the helper against a copy of the expressions it
replaced over all 2^32 float32 patterns."""
import functools
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import device as d  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 67
NY, NX = 256, 704


# name -> float32 bit pattern
SPECIAL = {
    "denormal": np.float32(1e-40).view(np.uint32),
    "minus_zero": np.uint32(0x80000000),
    "1900_and_2^-12": np.float32(1900.0 + 2.0 ** -12).view(np.uint32),
    "minus_half": np.float32(-0.5).view(np.uint32),
    "262144": np.float32(262144.0).view(np.uint32),
    "262145": np.float32(262145.0).view(np.uint32),
    "minus_262145": np.float32(-262145.0).view(np.uint32),
    "2^23_and_1": np.float32(8388609.0).view(np.uint32),
    "3e38": np.float32(3e38).view(np.uint32),
    "inf": np.float32(np.inf).view(np.uint32),
    "minus_inf": np.float32(-np.inf).view(np.uint32),
    "quiet_nan": np.uint32(0x7FC00000),
    "signalling_nan": np.uint32(0x7FA00000),
    "negative_nan": np.uint32(0xFFC00000),
}
POSITIONS = {"general": (100, 10), "lean": (100, 400), "last_row_10": (NY - 1, 10), "last_row_400": (NY - 1, 400)}
CASES = [(v, p) for v in SPECIAL for p in POSITIONS]


@functools.lru_cache(maxsize=None)
def base_dem():
    """Whole metres, about -1100 .. 900 m."""
    dem = orc.synthetic_dem(NY, NX, seed=NY + NX) - np.float32(2000.0)
    assert dem.dtype == np.float32 and np.array_equal(dem, np.trunc(dem))
    dem.setflags(write=False)
    return dem


def case_dem(value, pos):
    dem = base_dem().copy()
    row, col = POSITIONS[pos]
    sr, sc = max(1, NY // 128), max(1, NX // 128)
    assert not (row % sr == sr // 2 and col % sc == sc // 2), "a position beside the class lattice"
    dem.view(np.uint32)[row, col] = SPECIAL[value]  # (by bit pattern: a signalling NaN stays one)
    return dem


def tpi_single_block(dem, want_route):
    dev = d.DeviceArray.from_host(dem)
    blk = d.Block(dev, row0=0, gny=dem.shape[0])
    t = d.DeviceArray(*dem.shape)
    blk.tpi_std(SIZE, tpi=t, out_row0=0, out_rows=dem.shape[0])
    d.sync()
    assert d.tpi_route() == want_route, (d.tpi_route(), want_route)
    out = t.to_host()
    t.free()
    dev.free()
    return out


_MARCHING_CHILD = r"""
import json, sys
import numpy as np
from topo_descriptors_amd import device as d
spec = json.loads(sys.argv[1])
base = np.load(spec["base"])
out = {}
for name, row, col, bits in [("clean", -1, -1, 0)] + spec["cases"]:
    dem = base.copy()
    if row >= 0:
        dem.view(np.uint32)[row, col] = np.uint32(bits)
    dev = d.DeviceArray.from_host(dem)
    t = d.DeviceArray(*dem.shape)
    d.Block(dev, row0=0, gny=dem.shape[0]).tpi_std(67, tpi=t, out_row0=0, out_rows=dem.shape[0])
    d.sync()
    assert d.tpi_route() == 0, "TOPO_AMD_TPI_WIDE_RING=0 did not take effect"
    out[name] = t.to_host()
    t.free()
    dev.free()
np.savez(spec["out"], **out)
print("DONE", len(out))
"""


@functools.lru_cache(maxsize=None)
def marching_planes():
    """The marching route's plane of the clean raster and of every case: one child process for all of them."""
    with tempfile.TemporaryDirectory() as tmp:
        base_path, out_path = os.path.join(tmp, "base.npy"), os.path.join(tmp, "marching.npz")
        np.save(base_path, base_dem())
        spec = {"base": base_path, "out": out_path,
                "cases": [[f"{v}-{p}", POSITIONS[p][0], POSITIONS[p][1], int(SPECIAL[v])] for v, p in CASES]}
        env = dict(os.environ, TOPO_AMD_TPI_WIDE_RING="0")
        run = subprocess.run([sys.executable, "-c", _MARCHING_CHILD, json.dumps(spec)], cwd=ROOT, env=env, capture_output=True,
                             text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        with np.load(out_path) as z:
            return {k: z[k] for k in z.files}


def same_bits(a, b):
    """Bit for bit, NaN for NaN (the payload of a NaN an output holds is not part of the interface)."""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("value,pos", CASES)
def test_special_value_against_marching_route(value, pos):
    dem = case_dem(value, pos)
    wide = tpi_single_block(dem, 1)
    march = marching_planes()[f"{value}-{pos}"]
    ok = same_bits(wide, march)
    print(f"{value} at {POSITIONS[pos]}: {int((~ok).sum())} pixels differ, {int(np.isnan(wide).sum())} NaN")
    assert ok.all(), np.argwhere(~ok)[:5]


def test_clean_raster():
    dem = base_dem()
    wide = tpi_single_block(dem, 1)
    march = marching_planes()["clean"]
    assert np.array_equal(wide.view(np.uint32), march.view(np.uint32)), np.argwhere(wide != march)[:5]
    # float32 rounding of the exact value: half a unit in the last place, and as much again for the float64 evaluation that
    # is rounded (tests/test_gpu_tpi_wide_ring_staging.py, check); nothing for the scaled pass: no window holds a fraction
    exact = orc.tpi_exact(dem, SIZE)
    assert np.isfinite(wide).all() and np.isfinite(exact).all()
    tol = np.abs(exact) * 2.0 ** -23 + 1e-6
    err = np.abs(wide.astype(np.float64) - exact)
    print(f"max err {err.max():.3e} m, max err / tol {np.max(err / tol):.3f}")
    assert (err <= tol).all(), (np.argwhere(err > tol)[:5], err.max())


def test_lab_program(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is absent: the lab program cannot be built")
    exe = str(tmp_path / "classify_lab.bin")
    # (the library's own flags, topo_descriptors_amd/build.py: the denormal mode is the build's)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    os.path.join(ROOT, "tools", "ubench", "classify_lab.hip"), "-o", exe], check=True, cwd=ROOT, timeout=600)
    run = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("0 mismatches of 4294967296\n"), run.stdout[:2000]
