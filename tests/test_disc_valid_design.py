"""The valid-sample TPI / STD (``skipna=True``) judged without a GPU: the reference the GPU tests carry
(tests/disc_valid_ref.py) against the oracle where the two must agree, the comparisons of tests/test_gpu_disc_valid.py against
results that are subtly wrong, the argument errors raised before the library is loaded, and the three new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

from oracle import topo_oracle as orc
import disc_valid_ref as dv
from topo_descriptors_amd import _lib, batch, topo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"topo_amd_tpi_std_valid_dev": 11, "topo_amd_tpi_std_valid_raw": 7, "topo_amd_tpi_std_valid_packed": 7}


@pytest.mark.parametrize("size", dv.SIZES)
def test_the_reference_is_the_oracle_where_every_tap_is_valid(size):
    """A NaN-free raster, away from the border: n is the tap count and the formulas are the reference's own."""
    dem = dv.raster("clean")
    ref = dv.ValidReference(dem, size)
    reach = size // 2 + 1
    inner = (slice(reach, dv.GNY - reach), slice(reach, dv.NX - reach))
    taps = int(orc.circular_kernel(size).sum())
    assert (ref.n[inner] == taps).all() and (ref.n1[inner] == taps - 1).all()
    assert (ref.n < taps).any()  # (the border is not padded)
    tpi, std = orc.tpi_exact(dem, size), orc.std_exact(dem, size)
    assert np.max(np.abs(ref.tpi[inner] - tpi[inner])) <= 1e-9
    assert np.max(np.abs(ref.std[inner] - std[inner])) <= 1e-9 * np.max(std)
    assert not np.isnan(ref.tpi).any() and not np.isnan(ref.std).any()


def test_the_reference_against_a_tap_by_tap_loop():
    """Gaps and borders: the convolutions against the definition, pixel by pixel, on a corner of the small raster."""
    dem = dv.raster("frac", *dv.SMALL)
    for size in (4, 7):
        ref = dv.ValidReference(dem, size)
        dj, di, _ = orc.disc_taps(size)
        off = (size - 1) // 2 - size // 2  # the tap TPI excludes
        miss = dv.missing_mask(dem)
        for j in range(0, 24):
            for i in range(8, 36):
                taps = [(j + a, i + b) for a, b in zip(dj, di) if 0 <= j + a < dem.shape[0] and 0 <= i + b < dem.shape[1]
                        and not miss[j + a, i + b]]
                vals = np.array([float(dem[t]) for t in taps])
                rest = np.array([float(dem[t]) for t in taps if t != (j + off, i + off)])
                assert ref.n[j, i] == len(vals) and ref.n1[j, i] == len(rest)
                if miss[j, i] or len(rest) < 1:
                    assert np.isnan(ref.tpi[j, i])
                else:
                    assert abs(ref.tpi[j, i] - (float(dem[j, i]) - rest.sum() / len(rest))) < 1e-9
                if miss[j, i] or len(vals) < 2:
                    assert np.isnan(ref.std[j, i])
                else:
                    var = (np.sum(np.trunc(vals) ** 2) - vals.sum() ** 2 / len(vals)) / (len(vals) - 1)
                    assert abs(ref.std[j, i] - np.sqrt(max(var, 0.0))) < 1e-6
    assert np.isnan(dv.ValidReference(dem, 7).tpi[14, 22]) and not dv.missing_mask(dem)[14, 22]  # n' = 0 at a valid centre


def fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def as_stored(ref):
    return ref.tpi.astype(np.float32), ref.std.astype(np.float32)


@pytest.mark.parametrize("kind", ["frac", "whole"])
@pytest.mark.parametrize("size", [4, 6, 7, 67])
def test_the_comparisons_notice_a_subtly_wrong_result(size, kind):
    dem = dv.raster(kind)
    ref = dv.reference(kind, size)
    tpi, std = as_stored(ref)
    dv.check_tpi(tpi, ref)  # the reference itself passes, rounded to float32
    dv.check_std(std, ref)
    k = orc.circular_kernel(size).astype(np.float64)
    # a lost rim tap: the first tap of the mask's first row
    rim = k.copy()
    rim[0, np.flatnonzero(k[0])[0]] = 0.0
    wrong = [dv.ValidReference(dem, size, kernel=rim)]
    # a count that forgot the centre exclusion; a border padded with zeros instead of left out
    wrong.append(dv.ValidReference(dem, size, count_centre=True))
    wrong.append(dv.ValidReference(dem, size, zeros_beyond_border=True))
    for n, bad in enumerate(wrong):
        t, s = as_stored(bad)
        assert fails(dv.check_tpi, t, ref), n
        if n != 1:  # (the centre exclusion is TPI's alone)
            assert fails(dv.check_std, s, ref), n
    if size % 2 == 0:
        # the disc of an even size shifted by one pixel: the result of the neighbouring pixel
        for shift in ((1, 0), (0, 1)):
            t, s = (np.roll(p, shift, axis=(0, 1)) for p in as_stored(ref))
            assert fails(dv.check_tpi, t, ref) and fails(dv.check_std, s, ref), shift
        # ... and the off-centre disc mirrored (below 5 px the mask is a square: nothing to mirror)
        if size >= 5:
            flipped = dv.ValidReference(dem, size, kernel=k[::-1, ::-1])
            t, s = as_stored(flipped)
            assert fails(dv.check_tpi, t, ref) and fails(dv.check_std, s, ref)


def test_a_nan_pattern_a_pixel_off_fails():
    ref = dv.reference("frac", 7)
    tpi, _ = as_stored(ref)
    nan = np.isnan(tpi)
    one_more, one_less = tpi.copy(), tpi.copy()
    one_more[tuple(np.argwhere(~nan)[0])] = np.nan
    one_less[tuple(np.argwhere(nan)[0])] = 0.0
    assert fails(dv.check_tpi, one_more, ref) and fails(dv.check_tpi, one_less, ref)
    assert not fails(dv.check_tpi, tpi, ref)


def test_min_count_raises_the_threshold_only():
    a, b = dv.reference("frac", 7, 1), dv.reference("frac", 7, 30)
    assert np.isnan(b.tpi).sum() > np.isnan(a.tpi).sum()
    keep = ~np.isnan(b.tpi)
    assert np.array_equal(a.tpi[keep], b.tpi[keep]) and (b.n1[keep] >= 30).all()


class _Never:
    """A DEM nobody may look at: the argument errors come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the DEM was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("fn", [topo.tpi, topo.std, topo.tpi_std])
def test_argument_errors_come_before_the_library(fn):
    dem = np.zeros((8, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="skipna"):
        fn(dem, 7, sigma=2.0, skipna=True)
    with pytest.raises(ValueError, match="min_count"):
        fn(dem, 7, min_count=3)
    with pytest.raises(ValueError, match="min_count"):
        fn(dem, 7, skipna=True, min_count=0)
    with pytest.raises(ValueError):
        fn(_Never(), 7, sigma=2.0, skipna=True)
    with pytest.raises(ValueError):
        fn(_Never(), 7, min_count=2)


@pytest.mark.parametrize("fn", [batch.compute_tpi, batch.compute_std])
def test_batch_argument_errors(fn):
    class Var:
        def __init__(self, values, dims):
            self.values, self.dims = values, dims

    class Dataset:
        attrs = {"crs": "epsg:2056"}
        _v = {"dem": Var(np.zeros((16, 16), dtype=np.float32), ("y", "x")), "x": Var(30.0 * np.arange(16), ("x",)),
              "y": Var(-30.0 * np.arange(16), ("y",))}

        def __getitem__(self, k):
            return self._v[k]

        def __iter__(self):
            return iter(["dem"])

    with pytest.raises(ValueError, match="skipna"):
        fn(Dataset(), [90], smth_factors=[1.0], skipna=True, outdir=None)
    with pytest.raises(ValueError, match="min_count"):
        fn(Dataset(), [90], min_count=2, outdir=None)


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
    assert "launcher 6" in header and "bit 27" in header
