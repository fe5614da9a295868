"""The valley / ridge tables for any number of flat fractions, without a GPU: 4 ceil(n / 4) floats per tap, group g holding
planes 4g .. 4g+3 (include/topo_amd.h, topo_amd_valley_ridge_dev), the layout of 1 to 4 planes unchanged, the limits."""
import os
import re

import numpy as np
import pytest

from oracle import topo_oracle as orc
from topo_descriptors_amd import topo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = np.array([0, 1, 33, 90, 137], dtype=np.float32)


def _layout_of_four(kernels, angles):
    """The layout of 1 to 4 planes as it stood before more were accepted: 4 floats per tap, plane i in slot i."""
    n = kernels.shape[0]
    centre = (n - 1) // 2
    taps = []
    for angle in angles:
        turned = topo._rotate_kernels(kernels, angle).astype(np.float64)
        side = turned.shape[1]
        block = np.zeros((side, side, 4), dtype=np.float32)
        for i in range(n):
            total = sum(turned[b] for b in range(n) if 0 <= i - b + centre < n)
            block[:, :, i] = total[::-1, ::-1]
        taps.append(block.reshape(-1))
    ksize = [int(round((t.size // 4) ** 0.5)) for t in taps]
    return np.concatenate(taps).astype(np.float32), np.asarray(ksize, dtype=np.int32)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_layout_of_up_to_four_planes_is_unchanged(n):
    kernels = topo._valley_kernels(9, [0, 0.15, 0.3, 0.4][:n])
    taps, ksize, angles = topo._valley_ridge_tables(kernels, ANGLES)
    want_taps, want_ksize = _layout_of_four(kernels, ANGLES)
    assert taps.dtype == np.float32 and taps.tobytes() == want_taps.tobytes()
    assert np.array_equal(ksize, want_ksize) and np.array_equal(angles, ANGLES)


@pytest.mark.parametrize("n", [5, 6, 9, 16])
def test_more_planes_take_groups_of_four_floats(n):
    flats = [round(0.4 * i / (n - 1), 4) for i in range(n)]
    kernels = topo._ridge_kernels(7, flats)
    taps, ksize, _ = topo._valley_ridge_tables(kernels, ANGLES)
    width = 4 * ((n + 3) // 4)
    assert width == (8 if n <= 8 else 12 if n <= 12 else 16)
    assert taps.size == int((ksize.astype(np.int64) ** 2).sum()) * width
    pos = 0
    for a, ks in enumerate(ksize):
        block = taps[pos:pos + ks * ks * width].reshape(ks, ks, width)
        pos += ks * ks * width
        sums = orc.valley_ridge_plane_sums(orc.rotate_kernels(orc.ridge_kernels(7, flats), ANGLES[a]))
        assert len(sums) == n
        for i in range(n):  # plane i in group i // 4, slot i % 4: the flipped plane sum in float32
            assert np.array_equal(block[:, :, i], sums[i][::-1, ::-1].astype(np.float32)), (a, i)
        assert not np.any(block[:, :, n:])


def test_plane_counts_outside_the_limit_are_refused():
    assert topo.VALLEY_MAX_PLANES == 16
    header = open(os.path.join(REPO, "include", "topo_amd.h")).read()
    assert int(re.search(r"#define\s+TOPO_AMD_VALLEY_MAX_PLANES\s+(\d+)", header).group(1)) == topo.VALLEY_MAX_PLANES
    with pytest.raises(ValueError, match="0 flat fractions; 1 to 16"):
        topo._valley_ridge_tables(topo._valley_kernels(5, []), ANGLES)
    with pytest.raises(ValueError, match="17 flat fractions; 1 to 16"):
        topo._valley_ridge_tables(topo._valley_kernels(5, [0.01 * i for i in range(17)]), ANGLES)
    dem = orc.synthetic_dem(16, 16, seed=1)
    for flats in ([], [0.01 * i for i in range(17)]):  # before any library call: no GPU needed to refuse
        with pytest.raises(ValueError, match="flat fractions"):
            topo.valley_ridge(dem, 5, "valley", flats)
