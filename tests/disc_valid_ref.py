"""The reference of the valid-sample TPI / STD (``skipna=True``; include/topo_amd.h, topo_amd_tpi_std_valid_dev) and the
comparisons the GPU tests hold the kernels to.  ``oracle/`` has no such mode, so the tests carry it themselves.

The tap sums are exact integers: ``scipy.signal.convolve(..., "same")`` of ``m`` (1 where a sample is valid),
``m * rint(x * 2**16)`` and ``m * trunc(x)**2`` with the 0 / 1 disc.  Every sum stays below 2**53 on the rasters used here (at
most 10201 taps of 2**16 * 10**4 and of 10**8), so the float64 convolution - direct or by FFT, whose error is far below one
half - is exact after ``rint``.  The formulas are then evaluated in float64:

    TPI = x - s1' / n'                               NaN where x is missing or n' < max(1, min_count)
    STD = sqrt(max(0, (s2 - s1**2 / n) / (n - 1)))   NaN where x is missing or n  < max(2, min_count)

``n'`` and ``s1'`` leave out the tap TPI excludes (``kernel[size // 2, size // 2]``).  The keyword arguments of
:class:`ValidReference` build deliberately WRONG variants (another mask, zeros beyond the border, the centre counted) for
tests/test_disc_valid_design.py, which shows that the comparisons below notice them."""
import functools

import numpy as np
from scipy import signal

from oracle import topo_oracle as orc

MISSING_LIM = 2.0 ** 24


GNY, NX = 150, 299  # several tiles of 32 x 128 both ways, odd width; 300: the second width
SMALL = (40, 50)    # the raster narrower than a 67 px disc
SIZES = (3, 4, 6, 7, 21, 67, 101)


@functools.lru_cache(maxsize=None)
def raster(kind="frac", ny=GNY, nx=NX):
    """Relief of 900 ... 2900 m in multiples of 1/64 m (``frac``, ``hard``, ``clean``) or in whole metres (``whole``).  Planted
    (all but ``clean``): a NaN block of 30 x 60 with ONE valid pixel in its middle (n' = 0 at a valid centre for discs that
    stay inside the block), NaN at [0, 0] and one pixel from the top and the right border, +inf, 1e20, a plateau of 40 x 50;
    ``hard``: a 30 x 200 block of -9999.0 left finite as well.  The 40 x 50 raster has the same features at its own scale."""
    base = orc.synthetic_dem(max(ny, GNY), 300, seed=71, integer=kind == "whole")[:ny, :nx].astype(np.float64)
    a = (np.rint(base * 64.0) / 64.0).astype(np.float32)
    if kind != "clean":
        if (ny, nx) == SMALL:
            a[8:20, 12:32] = np.nan
            a[14, 22] = np.float32(np.rint(base[14, 22]))
            a[0, 0] = a[1, 40] = a[25, nx - 2] = np.nan
            a[33, 9] = np.inf
            a[36, 44] = 1.0e20
            a[24:36, 20:30] = 1500.0
        else:
            a[60:90, 100:160] = np.nan
            a[75, 130] = np.float32(np.rint(base[75, 130]))
            a[0, 0] = a[1, 250] = a[80, nx - 2] = np.nan
            a[120, 50] = np.inf
            a[30, 270] = 1.0e20
            a[100:140, 180:230] = 1500.0
            if kind == "hard":
                a[10:40, 40:240] = -9999.0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(kind, size, min_count=1, ny=GNY, nx=NX):
    """The :class:`ValidReference` of a raster, computed once for all the tests that need it."""
    return ValidReference(raster(kind, ny, nx), size, min_count)


def missing_mask(dem):
    """MISSING as the library defines it: not finite, or beyond +-2**24."""
    dem = np.asarray(dem)
    with np.errstate(invalid="ignore"):
        return (~np.isfinite(dem)) | (np.abs(np.trunc(np.nan_to_num(dem, nan=0.0, posinf=0.0, neginf=0.0))) >= MISSING_LIM)


def _tap_sum(field, kernel):
    return np.rint(signal.convolve(field, kernel.astype(np.float64), mode="same"))


class ValidReference:
    """``tpi`` / ``std`` (float64, NaN by the rules above) of ``dem`` for one disc ``size`` and ``min_count``, with the sums
    they came from (``n``, ``n1``, ``s1``, ``s2``)."""

    def __init__(self, dem, size, min_count=1, kernel=None, zeros_beyond_border=False, count_centre=False):
        dem = np.asarray(dem, dtype=np.float32)
        ny, nx = dem.shape
        self.size, self.min_count = size, min_count
        k = orc.circular_kernel(size).astype(np.float64) if kernel is None else np.asarray(kernel, dtype=np.float64)
        k1 = k.copy()
        if not count_centre:
            k1[size // 2, size // 2] = 0.0
        miss = missing_mask(dem)
        x = np.where(miss, 0.0, dem).astype(np.float64)
        m = (~miss).astype(np.float64)
        if zeros_beyond_border:  # the WRONG border: taps beyond it count as valid samples of elevation 0
            pad = size
            m = np.pad(m, pad, constant_values=1.0)
            x = np.pad(x, pad)
            inner = (slice(pad, pad + ny), slice(pad, pad + nx))
        else:
            inner = (slice(None), slice(None))
        scaled = m * np.rint(x * 65536.0)
        squares = m * np.trunc(x) ** 2
        self.n = _tap_sum(m, k)[inner].astype(np.int64)
        self.n1 = _tap_sum(m, k1)[inner].astype(np.int64)
        self.s1 = _tap_sum(scaled, k)[inner] / 65536.0
        self.s1p = _tap_sum(scaled, k1)[inner] / 65536.0
        self.s2 = _tap_sum(squares, k)[inner]
        assert max(np.abs(self.s1).max() * 65536.0, self.s2.max()) < 2.0 ** 53
        x, here = x[inner], ~miss
        with np.errstate(divide="ignore", invalid="ignore"):
            tpi = x - self.s1p / self.n1
            var = (self.s2 - self.s1 * self.s1 / self.n) / (self.n - 1)
            std = np.sqrt(np.clip(var, 0.0, None))
        self.tpi = np.where(here & (self.n1 >= max(1, min_count)), tpi, np.nan)
        self.std = np.where(here & (self.n >= max(2, min_count)), std, np.nan)


def ulp32(v):
    """The spacing of float32 at ``|v|`` (float64 array)."""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def check_nans(got, ref_plane, what=""):
    """The NaN pattern: exactly the reference's."""
    nan, want = np.isnan(got), np.isnan(ref_plane)
    if not np.array_equal(nan, want):
        extra, lost = np.argwhere(nan & ~want), np.argwhere(want & ~nan)
        raise AssertionError(f"{what}: {len(extra)} NaN too many (first at {extra[:1].tolist()}), {len(lost)} too few "
                             f"(first at {lost[:1].tolist()})")


def report(err, bound, ok, label):
    """``err`` and ``bound`` of the pixels ``ok``: prints the largest error as a share of its bound, and asserts it."""
    if not err.size:
        print(f"FIG {label}: no pixel to compare")
        return 0.0
    share = err / bound
    k = int(np.argmax(share))
    top, where = float(share[k]), tuple(int(v) for v in np.argwhere(ok)[k])
    print(f"FIG {label}: largest error {top:.3f} of its bound at {where}, {err.size} pixels")
    assert top <= 1.0, f"{label}: error {float(err[k]):.6g} at {where} is {top:.3f} of the bound {float(bound[k]):.6g}"
    return top


def check_tpi(got, ref, label="tpi"):
    """Every pixel: the NaN pattern exactly, the value within 1 float32 ulp of the reference's."""
    check_nans(got, ref.tpi, label)
    ok = ~np.isnan(ref.tpi)
    return report(np.abs(got.astype(np.float64)[ok] - ref.tpi[ok]), ulp32(ref.tpi[ok]), ok, label)


def check_std(got, ref, label="std"):
    """Every pixel: the NaN pattern exactly, the value within ``ulp32(ref) + delta / max(ref, sqrt(delta))`` with
    ``delta = 2**-50 max(s2, s1**2 / n) / (n - 1)``: the two float64 roundings of the cancelling numerator."""
    check_nans(got, ref.std, label)
    ok = ~np.isnan(ref.std)
    n = ref.n[ok].astype(np.float64)
    delta = 2.0 ** -50 * np.maximum(ref.s2[ok], ref.s1[ok] ** 2 / n) / (n - 1.0)
    want = ref.std[ok]
    floor = np.maximum(want, np.sqrt(delta))
    bound = ulp32(want) + np.divide(delta, floor, out=np.zeros_like(delta), where=floor > 0)  # (all taps 0: no rounding)
    return report(np.abs(got.astype(np.float64)[ok] - want), bound, ok, label)
