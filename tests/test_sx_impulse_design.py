"""The impulse raster of tests/test_gpu_sx_routes.py, judged on the float64 oracle alone (no GPU): a constant raster with
single spikes taller than ``height``, placed so that no output pixel sees two of them.  For the pixel at ``spike - offset``
that one ray pixel gives the only positive tangent, so every unique offset decides a pixel of its own - and a result
computed WITHOUT that offset (a lost, shifted or mis-weighted table entry looks the same there) must fail the comparison the
GPU tests make."""
import numpy as np
import pytest

from oracle import topo_oracle as orc
from test_gpu_sx_routes import HEIGHT, SECTORS, case, mismatches, sector, unique_offsets


@pytest.mark.parametrize("name", ["north_500", "one_ray_300", "grid_25x40_600"])
def test_every_offset_decides_a_pixel_of_the_impulse_raster(name):
    dem, want, spikes = case(name, "impulse")
    window, dj, di, dist = sector(name)
    offs = unique_offsets(sector(name))
    ny, nx = dem.shape
    assert mismatches(np.array(want), want, window, spikes, offs) == []
    # the reference is positive exactly at the spike - offset pixels inside the frame
    decided = np.zeros(dem.shape, bool)
    for s in spikes:
        t = np.asarray(s) - offs
        t = t[(t[:, 0] >= window) & (t[:, 0] < ny - window) & (t[:, 1] >= window) & (t[:, 1] < nx - window)]
        assert not decided[t[:, 0], t[:, 1]].any()
        decided[t[:, 0], t[:, 1]] = True
    assert np.array_equal(want > 0, decided)
    table = np.stack([dj, di], axis=1)
    for o in offs:
        keep = ~((table[:, 0] == o[0]) & (table[:, 1] == o[1]))
        assert keep.sum() < len(table)
        without = orc.sx_rolling(dem, window, table[keep], dist[keep], HEIGHT)
        assert mismatches(without, want, window, spikes, offs) != [], (name, tuple(o))
    # and a table entry moved by one pixel along the chain axis is noticed as well
    moved = table.copy()
    k = int(np.flatnonzero(~np.isnan(dist))[len(table) // 2])
    moved[(table[:, 0] == table[k, 0]) & (table[:, 1] == table[k, 1])] += (1, 0) if SECTORS[name][2] & 7 != 1 else (0, 1)
    assert mismatches(orc.sx_rolling(dem, window, moved, dist, HEIGHT), want, window, spikes, offs) != []
