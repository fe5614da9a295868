"""The sharded Gaussian, smoothed TPI / STD and valley / ridge, and gap fill without a GPU: the entry points are declared,
bound and exported with their arities, the valley's ghost-row rule adds the Gaussian's rows, and bad arguments are refused
in Python before the library is reached (tests/test_gpu_shard_smoothing.py holds the GPU tests)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from topo_descriptors_amd import _lib, shard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {
    "topo_amd_shard_gaussian": 8,
    "topo_amd_shard_tpi_std_smoothed": 9,
    "topo_amd_shard_valley_ridge_smoothed": 14,
    "topo_amd_shard_fill_na": 9,
}


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "topo_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (topo_amd_\w+)", nm))
    for name, n in ARITY.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == n, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
        assert name in exported and hasattr(lib, name), name


@pytest.mark.parametrize("kmax", [3, 7, 21, 45])
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5, 3.25, 8.0, 30.25])
def test_valley_halo_adds_the_gaussian_rows(kmax, sigma):
    plain = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, kmax)
    gauss = shard.halo_rows(_lib.DESC_GAUSS, sigma)
    got = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, kmax, sigma)
    assert got == (plain[0] + gauss[0], plain[1] + gauss[1])
    assert shard.halo_rows(_lib.DESC_VALLEY_RIDGE, kmax, 0.0) == plain == (kmax // 2, kmax - 1 - kmax // 2)


def test_tpi_halo_with_sigma_is_disc_plus_gaussian():
    for size, sigma in ((7, 1.0), (33, 8.0), (67, 8.0)):
        disc = shard.halo_rows(_lib.DESC_TPI, size)
        gauss = shard.halo_rows(_lib.DESC_GAUSS, sigma)
        assert shard.halo_rows(_lib.DESC_TPI, size, sigma) == (disc[0] + gauss[0], disc[1] + gauss[1])


@pytest.fixture
def offline_shard(monkeypatch):
    """A ShardedDEM whose library calls fail the test: every refusal must come first."""
    def refuse(*_a, **_k):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)
    sd = object.__new__(shard.ShardedDEM)
    sd.plan = shard.RowShardPlan(300, 5, 3, 1, 20, 20)
    sd.block = types.SimpleNamespace(ptr=1, rows=140, nx=5, row_ptr=lambda r: 1 + 20 * r)
    return sd


def _plane(rows=100, nx=5, dtype=np.float32):
    return types.SimpleNamespace(ptr=2, rows=rows, nx=nx, dtype=np.dtype(dtype))


TABLES = (np.zeros((1, 9, 4), np.float32), np.array([3], np.int32), np.zeros(1, np.float32), 3)


@pytest.mark.parametrize("sigma", [-1.0, -1e-9, np.nan, np.inf, "wide"])
def test_bad_sigma_is_refused_before_the_library(offline_shard, sigma):
    with pytest.raises(ValueError, match="sigma"):
        offline_shard.tpi_std(7, tpi=_plane(), sigma=sigma)
    with pytest.raises(ValueError, match="sigma"):
        offline_shard.valley_ridge(*TABLES, _plane(), _plane(), sigma=sigma)
    with pytest.raises(ValueError, match="sigma"):
        offline_shard.gaussian(sigma, _plane())
    with pytest.raises(ValueError, match="sigma"):
        offline_shard.gaussian((1.0, sigma), _plane())


@pytest.mark.parametrize("sigma", [(1.0, 2.0, 3.0), [[1.0, 2.0]], (), np.ones((2, 2))])
def test_bad_sigma_pair_is_refused_before_the_library(offline_shard, sigma):
    with pytest.raises(ValueError, match="sigma"):
        offline_shard.gaussian(sigma, _plane())


@pytest.mark.parametrize("x", [np.arange(4.0), np.arange(6.0), np.array([0.0, 1.0, 1.0, 2.0, 3.0]),
                               np.array([0.0, 2.0, 1.0, 3.0, 4.0]), np.array([0.0, 1.0, np.nan, 3.0, 4.0])])
def test_bad_x_coords_are_refused_before_the_library(offline_shard, x):
    with pytest.raises(ValueError, match="x_coords"):
        offline_shard.fill_na(x_coords=x)


def test_bad_fill_planes_are_refused_before_the_library(offline_shard):
    with pytest.raises(ValueError, match="uint8"):
        offline_shard.fill_na(missing=_plane())
    with pytest.raises(ValueError, match="owns"):
        offline_shard.fill_na(out=_plane(rows=99))
    with pytest.raises(ValueError, match="owns"):
        offline_shard.fill_na(missing=_plane(nx=4, dtype=np.uint8))
