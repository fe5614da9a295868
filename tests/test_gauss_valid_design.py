"""The valid-sample Gaussian (``topo.dem(skipna=True)``) judged without a GPU: the comparison of tests/test_gpu_gauss_valid.py
against results that are subtly wrong, the footprint claims of include/topo_amd.h on the reference itself, the argument errors
raised before the library is loaded, and the three new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import disc_valid_ref as dv
import gauss_valid_ref as gv
from topo_descriptors_amd import _lib, batch, topo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"topo_amd_gaussian_valid_dev": 13, "topo_amd_gauss_valid_raw": 9, "topo_amd_gauss_valid_packed": 9}
ALL_SIGMAS = gv.SIGMAS + gv.PAIRS


def fails(*args, **kw):
    try:
        gv.check(*args, **kw)
    except AssertionError:
        return True
    return False


def as_stored(ref, min_weight=0.0, fill=False):
    return ref.out(min_weight, fill).astype(np.float32), ref.D.astype(np.float32)


@pytest.mark.parametrize("variant", ["zero_padding", "divide_between", "no_normalisation", "finite_only"])
@pytest.mark.parametrize("sigma", [0.75, 3.25, (2.0, 5.0)], ids=str)
def test_the_comparison_notices_a_wrong_variant(sigma, variant):
    dem = dv.raster("frac")
    ref = gv.reference("frac", sigma)
    for fill in (False, True):
        gv.check(*as_stored(ref, 0.0, fill), ref, 0.0, fill)  # the reference itself passes, rounded to float32
        bad = gv.GaussValidReference(dem, sigma, **{variant: True})
        assert fails(*as_stored(bad, 0.0, fill), ref, 0.0, fill), (variant, fill)
        if variant in ("divide_between", "no_normalisation"):  # (their weight plane is the right one: the VALUES give them away)
            assert fails(as_stored(bad, 0.0, fill)[0], None, ref, 0.0, fill), (variant, fill)


def test_the_comparison_notices_a_nan_a_pixel_off_and_a_weight_off():
    ref = gv.reference("frac", 3.25)
    out, weight = as_stored(ref)
    one_more, one_less = out.copy(), out.copy()
    one_more[tuple(np.argwhere(~np.isnan(out))[0])] = np.nan
    one_less[tuple(np.argwhere(np.isnan(out))[0])] = 1500.0
    assert fails(one_more, weight, ref) and fails(one_less, weight, ref) and not fails(out, weight, ref)
    assert fails(out, weight + np.float32(2e-4), ref)
    assert fails(out + np.float32(2.5e-3), weight, ref)
    # a threshold: a mask that ignores min_weight fails, the reference's own passes
    assert not fails(*as_stored(ref, 0.5), ref, 0.5) and fails(out, weight, ref, 0.5)


@pytest.mark.parametrize("sigma", ALL_SIGMAS, ids=str)
@pytest.mark.parametrize("kind,ny,nx", [(k, *s) for k in gv.KINDS for s in gv.SHAPES], ids=lambda v: str(v))
def test_the_footprint_claims_hold_on_the_reference(kind, ny, nx, sigma):
    ref = gv.reference(kind, sigma, ny, nx)
    assert ref.miss.any() and (ref.D >= 0).all() and ref.D.max() <= 1.0 + 1e-12
    # D > 0 is "a valid sample in the reflected window", also once D is stored as float32
    window = gv.window_has_a_valid_sample(ref.miss, sigma)
    assert np.array_equal(ref.D > 0, window) and np.array_equal(ref.D.astype(np.float32) > 0, window)
    # defaults: NaN at the missing pixels only (a valid pixel has its own tap); fill: NaN where the window is empty
    assert np.array_equal(np.isnan(ref.out()), ref.miss)
    assert np.array_equal(np.isnan(ref.out(fill=True)), ~window)
    # the band around a threshold that the GPU tests leave out stays below its cap
    for mw in gv.MIN_WEIGHTS:
        assert (np.abs(ref.D - mw) <= gv.WEIGHT_BOUND).mean() <= gv.BAND_SHARE, mw


def test_a_gap_free_raster_is_the_plain_filter():
    from oracle import topo_oracle as orc
    dem = dv.raster("clean")
    for sigma in (0.75, 3.25, (2.0, 5.0)):
        ref = gv.GaussValidReference(dem, sigma)
        assert np.abs(ref.D - 1.0).max() <= 1e-12
        assert np.abs(ref.out() - orc.gaussian_exact(dem, sigma)).max() <= 1e-9


class _Never:
    """A DEM nobody may look at: the argument errors come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the DEM was touched ({name}) before the arguments were checked")


def test_argument_errors_come_before_the_library():
    for kw in ({"min_weight": 0.5}, {"fill": True}, {"return_weight": True}):
        with pytest.raises(ValueError, match="skipna"):
            topo.dem(_Never(), 2.0, **kw)
    for mw in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_weight"):
            topo.dem(_Never(), 2.0, skipna=True, min_weight=mw)


class _Var:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class _Dataset:
    attrs = {"crs": "epsg:2056"}

    def __init__(self, dem):
        self._v = {"dem": _Var(dem, ("y", "x")), "x": _Var(30.0 * np.arange(16), ("x",)), "y": _Var(-30.0 * np.arange(16), ("y",))}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def test_batch_argument_errors():
    ds = _Dataset(np.zeros((16, 16), dtype=np.float32))
    with pytest.raises(ValueError, match="skipna"):
        batch.compute_dem(ds, [90], min_weight=0.5, outdir=None)
    with pytest.raises(ValueError, match="skipna"):
        batch.compute_dem(ds, [90], fill=True, outdir=None)
    with pytest.raises(ValueError, match="min_weight"):
        batch.compute_dem(ds, [90], skipna=True, min_weight=1.5, outdir=None)


@pytest.mark.parametrize("fn", [topo.tpi, topo.std, topo.tpi_std])
def test_a_sigma_with_skipna_is_still_an_error_and_names_the_chain(fn):
    with pytest.raises(ValueError, match="skipna") as err:
        fn(_Never(), 7, sigma=2.0, skipna=True)
    assert "dem(d, sigma, skipna=True)" in str(err.value)


@pytest.mark.parametrize("fn", [batch.compute_tpi, batch.compute_std])
def test_a_smoothing_factor_with_skipna_is_still_an_error_and_names_the_chain(fn):
    with pytest.raises(ValueError, match="skipna") as err:
        fn(_Dataset(np.zeros((16, 16), dtype=np.float32)), [90], smth_factors=[1.0], skipna=True, outdir=None)
    assert "topo.dem(d, sigma, skipna=True)" in str(err.value)


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
    assert "needs a normalised convolution of its own" not in header
    for path in ("topo_descriptors_amd/topo.py", "topo_descriptors_amd/batch.py"):
        assert "needs a normalised convolution of its own" not in open(os.path.join(REPO, path)).read().replace("\n", " ")
