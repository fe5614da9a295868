#!/usr/bin/env python3
"""Times the valid-sample gradient (csrc/gradient.hip K4v, ``Block.gradient_valid``) on a resident raster - the gap-free DEM and
one with about 5 % of it missing in blobs - next to its parts: ``Block.gradient`` (the plain call, on the gap-free DEM), the
valid-sample Gaussian with ``fill`` alone (``Block.gaussian_valid``: the smooth the valid gradient queues, one neighbour row less
at each end), and their difference, the share of the valid-difference epilogue, with the bytes per second that share means at
20 B / pixel (``fill=True``) or 24 (the raw plane read too).  Next to it the plain ``gradient_epilogue4`` alone: the plain
gradient at a sigma whose smooth is ``Block.gaussian``'s (the matrix-core route) minus that smooth - an estimate, the two run
partly side by side in row chunks.  sigma 0.75 is the Sobel route of both calls: no smooth, the whole call is the kernel.
Sigmas 0.75, 3.25, 12, 30.25; medians of per-launch HIP-event times.
usage: tools/gradient_valid_time.py [--n 8192] [--reps 7] [--out profiles/gradient_valid_time.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from topo_descriptors_amd import device as d  # noqa: E402

SIGMAS = (0.75, 3.25, 12.0, 30.25)
RES = (25.0, -25.0)


def blobs(n, share=0.05):
    """A boolean n x n mask of smooth blobs covering about ``share`` of the raster (tools/gauss_valid_time.py)."""
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
    outs = [d.DeviceArray(n, n) for _ in range(4)]
    planes = dict(zip(("dx", "dy", "slope", "aspect"), outs))
    pixels = float(n) * n

    def timed(fn):
        return median(d.time_launches(fn, args.reps))

    lines = [f"valid-sample gradient, {n} x {n} resident, median of {args.reps} launches (ms); gapped: {100 * missing_share:.1f} % missing "
             "in blobs; plain: topo_amd_gradient_dev on the gap-free DEM; smooth: topo_amd_gaussian_valid_dev(fill = 1) alone; "
             "epilogue = valid - smooth, with TB/s at 24 B / pixel (fill = 0) and 20 (fill = 1); plain epi.: plain - topo_amd_gaussian_dev",
             f"{'sigma':>6} {'radius':>6} {'raster':>7} | {'plain':>7} {'plain epi.':>10} | {'smooth':>7} | {'valid':>7} {'epilogue':>8} {'TB/s':>5} | "
             f"{'valid, fill':>11} {'epilogue':>8} {'TB/s':>5}"]
    for sigma in SIGMAS:
        plain = timed(lambda: d.Block(clean).gradient(sigma, *RES, **planes))
        plain_smooth = timed(lambda: d.Block(clean).gaussian(sigma, sigma, outs[0])) if sigma > 1 else 0.0
        for name, dem in (("clean", clean), ("gapped", gapped)):
            smooth = timed(lambda: d.Block(dem).gaussian_valid(sigma, sigma, outs[0], fill=True)) if sigma > 1 else 0.0
            row = []
            for fill, nbytes in ((False, 24.0), (True, 20.0)):
                t = timed(lambda: d.Block(dem).gradient_valid(sigma, *RES, fill=fill, **planes))
                epi = t - smooth
                row += [t, epi, nbytes * pixels / (epi * 1e-3) / 1e12 if epi > 0 else float("nan")]
            lines.append(f"{sigma:>6} {int(4 * sigma + 0.5):>6} {name:>7} | {plain:7.3f} {plain - plain_smooth:10.3f} | {smooth:7.3f} | "
                         f"{row[0]:7.3f} {row[1]:8.3f} {row[2]:5.2f} | {row[3]:11.3f} {row[4]:8.3f} {row[5]:5.2f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
