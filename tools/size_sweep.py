"""TPI / STD / both for every odd disc size 3 ... 101 on one DEM - whole metres, fractional elevations, and whole metres
with a fractional patch (raster classes W, F and P) - as one call and as two row blocks with the whole raster's class
declared: per size the three times (look for steps between neighbouring sizes), the three route words of
``device.disc_route()`` and the CRC-32 of the four result planes (TPI, STD, and the two planes of TPI + STD).

Two builds of the library in one GPU session: run it once per build with ``TOPO_AMD_LIBRARY`` set and compare the outputs
with ``--diff``, which ignores the times and fails on any other difference.

usage: size_sweep.py [n=16384] [--sizes LO:HI] [--rasters whole,frac,patch] [--modes call,blocks] [--no-crc]
       size_sweep.py --diff A.txt B.txt"""
import argparse
import os
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def diff(path_a, path_b):
    """Lines as ``times | words | crcs``: everything but the times must agree."""
    def without_times(line):
        head, bar, rest = line.rstrip("\n").partition("|")
        return line.rstrip("\n") if line.startswith("#") or not bar else head.split()[0] + " |" + rest

    def lines(path):
        with open(path) as fh:
            return [without_times(line) for line in fh if line.strip()]
    a, b = lines(path_a), lines(path_b)
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in bad[:20]:
        print(f"- {x}\n+ {y}")
    print(f"{len(a)} and {len(b)} lines, {len(bad)} differ (times ignored)")
    return 1 if bad or len(a) != len(b) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=16384)
    ap.add_argument("--sizes", default="3:101")
    ap.add_argument("--rasters", default="whole,frac,patch")
    ap.add_argument("--modes", default="call,blocks")
    ap.add_argument("--no-crc", action="store_true", help="times and words only: no plane crosses the link")
    ap.add_argument("--diff", nargs=2)
    args = ap.parse_args()
    if args.diff:
        return diff(*args.diff)

    import numpy as np
    from topo_descriptors_amd import _lib, device as d, shard

    n = args.n
    lo, hi = (int(v) for v in args.sizes.split(":"))
    o = [d.DeviceArray(n, n) for _ in range(4)]  # TPI, STD, and the two planes of TPI + STD
    host = [np.empty((n, n), dtype=np.float32) for _ in o]
    pool = ThreadPoolExecutor(max_workers=len(o))

    class Rows:
        """The rows of a result plane from ``row0`` on, as an output argument."""
        def __init__(self, plane, row0):
            self.ptr = plane.row_ptr(row0)

    def timed(fn):
        fn()
        d.sync()
        d.timer_start()
        fn()
        fn()
        return d.timer_stop() / 2, d.disc_route()

    def crc(k):
        _lib.check(_lib.lib().topo_amd_memcpy_d2h(_lib.ptr(host[k]), o[k].ptr, host[k].nbytes), "memcpy_d2h")
        return pool.submit(zlib.crc32, host[k])

    for raster in args.rasters.split(","):
        dem = d.synth_dem(n, n, seed=0, integer=raster != "frac")
        if raster == "patch":  # a quarter of the rows + 0.25 m: class P (0 < frac_share <= 0.5)
            rows = dem.to_host(n // 4, n // 4)
            dem.upload_rows(rows + np.float32(0.25), n // 4)
            d.dem_changed(dem)
        for mode in args.modes.split(","):
            if mode == "call":
                blocks = [(d.Block(dem), 0, n)]
            else:  # two row blocks, views of the one plane with their halo rows, the whole raster's class declared for each
                cut = n // 2 + 13
                scan = d.RasterScan().add(d.Block(dem))
            print(f"# {n}x{n} {raster} {mode}; size, ms tpi std both | route words | crc32 tpi std both.tpi both.std", flush=True)
            for size in range(lo | 1, hi + 1, 2):
                if mode != "call":
                    above, below = shard.halo_rows(_lib.DESC_TPI, size)
                    blocks = []
                    for r0, r1 in ((0, cut), (cut, n)):
                        first, last = max(0, r0 - above), min(n, r1 + below)
                        blocks.append((d.Block(dem, row0=first, gny=n, first_buffer_row=first, rows=last - first), r0, r1))
                    scan.declare(*(blk for blk, _, _ in blocks))

                def run(tpi, std):
                    for blk, r0, r1 in blocks:
                        blk.tpi_std(size, tpi=Rows(tpi, r0) if tpi else None, std=Rows(std, r0) if std else None,
                                    out_row0=r0, out_rows=r1 - r0)
                ta, wa = timed(lambda: run(o[0], None))
                tb, wb = timed(lambda: run(None, o[1]))
                tc, wc = timed(lambda: run(o[2], o[3]))
                d.sync()
                sums = [] if args.no_crc else [f.result() for f in [crc(k) for k in range(4)]]
                print(f"{size:4d} {ta:7.3f} {tb:7.3f} {tc:7.3f} | {wa:#010x} {wb:#010x} {wc:#010x} | " + " ".join(f"{s:08x}" for s in sums),
                      flush=True)
            d.forget_raster_class()
        dem.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
