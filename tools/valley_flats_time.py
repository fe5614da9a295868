"""The valley index with 3 and with 6 flat fractions (6: two groups of four planes through the same kernels) on an n x n DEM,
7 px (folded, operands in registers) and 21 px (folded, streamed): route and ms per call (second call on, median).
python tools/valley_flats_time.py [n=8192] [reps=5]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topo_descriptors_amd import device as d, topo  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dem = d.synth_dem(n, n, seed=0)
    blk = d.Block(dem)
    mean, stdev = d.mean_std(dem)
    norm, direction = d.DeviceArray(n, n), d.DeviceArray(n, n)
    angles = np.arange(0, 180, dtype=np.float32)
    rows = []
    for size in (7, 21):
        for flats in ([0, 0.15, 0.3], [0, 0.1, 0.2, 0.3, 0.4, 0.5]):
            taps, ksize, ang = topo._valley_ridge_tables(topo._valley_kernels(size, flats), angles)
            times = []
            for _ in range(reps + 1):
                d.sync()
                t0 = time.perf_counter()
                blk.valley_ridge(taps, ksize, ang, len(flats), mean, stdev, norm, direction)
                d.sync()
                times.append(time.perf_counter() - t0)
            rows.append({"n": n, "size": size, "flats": len(flats), "route": d.valley_route(),
                         "ms_median": round(1e3 * float(np.median(times[1:])), 2), "ms_min": round(1e3 * min(times[1:]), 2)})
            print(json.dumps(rows[-1]), flush=True)
    for x in (norm, direction, dem):
        x.free()


if __name__ == "__main__":
    main()
