"""The valid-sample gradient's public surface, judged without a GPU: the argument errors of ``topo.gradient``, ``topo.sobel`` and
``batch.compute_gradient`` are raised before the DEM is touched or the library loaded, and the three new symbols of the C ABI
are declared, bound and exported."""
import inspect
import os
import re

import numpy as np
import pytest

from topo_descriptors_amd import _lib, batch, device, topo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"topo_amd_gradient_valid_dev": 18, "topo_amd_gradient_valid_raw": 14, "topo_amd_gradient_valid_packed": 14}
RES = {"x": 25.0, "y": -25.0}


class _Never:
    """A DEM nobody may look at: the argument errors come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the DEM was touched ({name}) before the arguments were checked")


def test_gradient_argument_errors_come_before_the_library():
    for kw in ({"min_weight": 0.5}, {"fill": True}):
        with pytest.raises(ValueError, match="skipna"):
            topo.gradient(_Never(), 3.25, RES, **kw)
    for mw in (-0.1, 1.5, float("nan"), "half"):
        with pytest.raises(ValueError, match="min_weight"):
            topo.gradient(_Never(), 3.25, RES, skipna=True, min_weight=mw)


def test_sobel_argument_errors_come_before_the_library():
    with pytest.raises(ValueError, match="skipna"):
        topo.sobel(_Never(), fill=True)


class _Var:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class _Dataset:
    attrs = {"crs": "epsg:2056"}

    def __init__(self, dem):
        self._v = {"dem": _Var(dem, ("y", "x")), "x": _Var(30.0 * np.arange(16), ("x",)), "y": _Var(-30.0 * np.arange(16), ("y",))}

    def __getitem__(self, k):
        if k == "dem" and isinstance(self._v["dem"].values, _Never):
            raise AssertionError("the DEM was touched before the arguments were checked")
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def test_compute_gradient_argument_errors():
    ds = _Dataset(_Never())
    with pytest.raises(ValueError, match="skipna"):
        batch.compute_gradient(ds, [90], min_weight=0.5, outdir=None)
    with pytest.raises(ValueError, match="skipna"):
        batch.compute_gradient(ds, [90], fill=True, outdir=None)
    for mw in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_weight"):
            batch.compute_gradient(ds, [90], skipna=True, min_weight=mw, outdir=None)


def test_the_keywords_and_their_defaults():
    for fn, names in ((topo.gradient, ("skipna", "min_weight", "fill")), (topo.sobel, ("skipna", "fill")),
                      (batch.compute_gradient, ("skipna", "min_weight", "fill")),
                      (device.Block.gradient_valid, ("min_weight", "fill"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params and params[name].default in (False, 0.0), (fn.__name__, name)
    from topo_descriptors_amd import shard
    assert "skipna" not in inspect.signature(shard.ShardedDEM.gradient).parameters  # (valid smoothing is not sharded either)


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "topo_amd.h")).read()
    lib = _lib.load()
    for name, arity in SYMBOLS.items():
        found = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert found, f"{name} is not declared in include/topo_amd.h"
        assert len(found.group(1).split(",")) == arity, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == arity and res is _lib.C.c_int, name
        assert hasattr(lib, name), f"{name} is not exported"
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "open: `topo.gradient(skipna=True)`" not in design
