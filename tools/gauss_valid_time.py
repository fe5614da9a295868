#!/usr/bin/env python3
"""Times the valid-sample Gaussian (csrc/gauss_valid.hip, ``Block.gaussian_valid``) on a resident raster, with and without a
weight plane, on a DEM with about 5 % of it missing in blobs and on the gap-free one - each next to ``Block.gaussian``
(``topo_amd_gaussian_dev``, the existing route: matrix-core kernels from radius 4) for the same sigma on the gap-free DEM.
Sigmas 0.75, 3.25, 12, 30.25 (radii 3, 13, 48, 121); medians of per-launch HIP-event times.
usage: tools/gauss_valid_time.py [--n 8192] [--reps 7] [--out profiles/gauss_valid_time.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from topo_descriptors_amd import device as d  # noqa: E402

SIGMAS = (0.75, 3.25, 12.0, 30.25)


def blobs(n, share=0.05):
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
    out, weight = d.DeviceArray(n, n), d.DeviceArray(n, n)

    def timed(fn):
        return median(d.time_launches(fn, args.reps))

    lines = [f"valid-sample Gaussian, {n} x {n} resident, median of {args.reps} launches (ms); gapped: "
             f"{100 * missing_share:.1f} % missing in blobs; gaussian: topo_amd_gaussian_dev on the gap-free DEM",
             f"{'sigma':>6} {'radius':>6} | {'gaussian':>8} | {'valid, gapped':>13} {'ratio':>6} {'+ weight':>9} {'ratio':>6} | "
             f"{'valid, clean':>12} {'ratio':>6} | {'fill, gapped':>12} {'ratio':>6}"]
    for sigma in SIGMAS:
        old = timed(lambda: d.Block(clean).gaussian(sigma, sigma, out))
        row = [timed(lambda: d.Block(gapped).gaussian_valid(sigma, sigma, out)),
               timed(lambda: d.Block(gapped).gaussian_valid(sigma, sigma, out, weight=weight)),
               timed(lambda: d.Block(clean).gaussian_valid(sigma, sigma, out)),
               timed(lambda: d.Block(gapped).gaussian_valid(sigma, sigma, out, fill=True))]
        lines.append(f"{sigma:>6} {int(4 * sigma + 0.5):>6} | {old:8.3f} | {row[0]:13.3f} {row[0] / old:6.2f} {row[1]:9.3f} {row[1] / old:6.2f} | "
                     f"{row[2]:12.3f} {row[2] / old:6.2f} | {row[3]:12.3f} {row[3] / old:6.2f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
