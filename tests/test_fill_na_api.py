"""The gap fill's interface without a GPU: both entry points are declared, bound and exported, and bad ``x_coords`` are
refused in Python before the library is reached (tests/test_gpu_fill_na.py holds the GPU tests)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from topo_descriptors_amd import _lib, device, helpers as hlp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("topo_amd_fill_na_dev", "topo_amd_fill_na_f32")


def test_fill_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "topo_amd.h")).read()
    declared = set(re.findall(r"\b(topo_amd_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["topo_amd_fill_na_dev"][1]) == 11
    assert len(_lib.SIGNATURES["topo_amd_fill_na_f32"][1]) == 7


BAD_COORDS = [
    np.array([0.0, 1.0, 1.0, 2.0, 3.0]),          # a repeated coordinate
    np.array([0.0, 1.0, 3.0, 2.0, 4.0]),          # not monotonic
    np.array([0.0, 1.0, np.nan, 3.0, 4.0]),       # not finite
    np.array([0.0, 1.0, 2.0, 3.0, np.inf]),
    np.arange(4.0),                               # one short
    np.arange(6.0),                               # one too many
]


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("x", BAD_COORDS)
def test_bad_x_coords_raise_before_the_library(no_library, x):
    a = np.ones((3, 5), np.float32)
    with pytest.raises(ValueError, match="x_coords"):
        hlp.fill_na_gpu(a, x_coords=x)
    block = device.Block(types.SimpleNamespace(rows=3, nx=5, row_ptr=lambda r: 0))
    with pytest.raises(ValueError, match="x_coords"):
        block.fill_na(block.data, x_coords=x)


def test_good_coords_and_shapes(no_library):
    assert hlp._fill_coords(None, 5) is None
    for x in (np.arange(5.0), -0.5 * np.arange(5.0), [3.0], np.array([1.0, 10.0, 10.5, 200.0, 201.0])):
        got = hlp._fill_coords(x, len(x))
        assert got.dtype == np.float64 and got.flags.c_contiguous
    for bad in (np.ones(4, np.float32), np.ones((2, 3, 4), np.float32), np.ones((0, 4), np.float32)):
        with pytest.raises(ValueError):
            hlp.fill_na_gpu(bad)


def test_device_array_dtypes():
    with pytest.raises(ValueError):
        device.DeviceArray(2, 2, dtype=np.float64)
