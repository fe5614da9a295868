#!/usr/bin/env python3
"""Times the valid-sample TPI / STD (csrc/disc_valid.hip, ``Block.tpi_std_valid``) on a resident raster of whole metres, next to
what a user has without it: on the NaN-free raster ``Block.tpi_std`` of the same build (the tuned routes), on the same raster
with 10 % of it missing in blobs the chain gap fill + ``tpi_std`` + finish (``fill_na`` into a work plane with its mask, the
descriptor on the filled plane, ``topo_amd_finish_dev`` putting NaN back).  Sizes 7, 21, 67; TPI, STD, TPI + STD; medians of
per-launch HIP-event times.  The slow form (bit 27 of ``disc_route``) must stay off on both rasters: the tool fails otherwise.
usage: tools/disc_valid_time.py [--n 8192] [--reps 7] [--out profiles/disc_valid_time.txt]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from topo_descriptors_amd import _lib, device as d  # noqa: E402

SIZES = (7, 21, 67)
OPS = ("tpi", "std", "tpi_std")
SLOW = 1 << 27


def blobs(n, share=0.10):
    """A boolean n x n mask of smooth blobs covering about ``share`` of the raster."""
    j = np.arange(n, dtype=np.float32)[:, None]
    i = np.arange(n, dtype=np.float32)[None, :]
    f = np.sin(j / 97.0) * np.cos(i / 131.0) + 0.5 * np.sin((j + 2.0 * i) / 53.0) + 0.3 * np.cos((3.0 * j - i) / 211.0)
    return f > np.quantile(f[::16, ::16], 1.0 - share)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    clean = d.synth_dem(n, n, seed=3)
    holes = blobs(n)
    host = clean.to_host()
    host[holes] = np.nan
    gapped = d.DeviceArray.from_host(host)
    missing_share = float(holes.mean())
    del host, holes
    work, mask = d.DeviceArray(n, n), d.DeviceArray(n, n, dtype=np.uint8)
    t, s, fin = d.DeviceArray(n, n), d.DeviceArray(n, n), d.DeviceArray(n, n)
    lib = _lib.lib()
    f32 = _lib.Packing(np.float32)

    def finish(plane):
        out = f32.struct(fin.ptr)
        _lib.check(lib.topo_amd_finish_dev(plane.ptr, n, n, mask.ptr, 0, n, 0, n, C.byref(out)), "finish_dev")

    def planes(op):
        return {"tpi": t if "tpi" in op else None, "std": s if "std" in op else None}

    def fill_chain(size, op):
        d.Block(gapped).fill_na(work, mask)
        d.Block(work).tpi_std(size, **planes(op))
        for plane in planes(op).values():
            if plane is not None:
                finish(plane)

    lines = [f"valid-sample TPI / STD, {n} x {n} whole metres resident, median of {args.reps} launches (ms); "
             f"gapped: {100 * missing_share:.1f} % missing in blobs",
             f"{'size':>4} {'call':>8} | {'valid':>8} {'tpi_std':>8} {'ratio':>6} | {'valid, gapped':>13} {'fill+tpi_std+finish':>19} {'ratio':>6}"]
    for size in SIZES:
        for op in OPS:
            row = []
            for dem, other in ((clean, lambda: d.Block(clean).tpi_std(size, **planes(op))), (gapped, lambda: fill_chain(size, op))):
                new = median(d.time_launches(lambda: d.Block(dem).tpi_std_valid(size, **planes(op)), args.reps))
                if d.disc_route() & SLOW:
                    raise SystemExit(f"size {size} {op}: a tile took the slow form on a raster of whole metres - a bug")
                old = median(d.time_launches(other, args.reps))
                row += [new, old, new / old]
            lines.append(f"{size:>4} {op:>8} | {row[0]:8.3f} {row[1]:8.3f} {row[2]:6.2f} | {row[3]:13.3f} {row[4]:19.3f} {row[5]:6.2f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
