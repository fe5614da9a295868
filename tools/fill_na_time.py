#!/usr/bin/env python3
"""Times the gap fill (csrc/fill.hip): the device-resident call at 16384^2 and 32768^2 with 0 %, 1 % scattered and 30 % block
+ 1 % scattered missing samples, in place and out of place (with the missing mask); the host-buffer call at 16384^2 next to
topo.tpi(ndarray, 67) at that size; and helpers.fill_na_array, the host oracle, on the same 16384^2 array.  One JSON line per
case; the algorithmic traffic is 4 B read + 4 B written + 1 B of mask per pixel out of place, 4 B read + 4 B per missing
pixel + 1 B of mask in place.
usage: tools/fill_na_time.py [--sizes 16384,32768] [--reps 7] [--no-host]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from topo_descriptors_amd import _lib, device as d, helpers as hlp, topo  # noqa: E402

HBM_COPY_TBS = 4.93  # device-to-device copy rate of this project (hbm_copy_live)


def with_holes(n, case, seed=0):
    """An n x n DEM on the device with the case's missing samples, built in slabs of rows (no n^2 host array)."""
    dem = d.synth_dem(n, n, seed=seed)
    if case == "0%":
        return dem
    rng = np.random.default_rng(seed)
    slab = 1024
    for r0 in range(0, n, slab):
        rows = min(slab, n - r0)
        h = dem.to_host(r0, rows)
        h[rng.random(h.shape) < 0.01] = np.nan
        if case == "30%+1%":
            h[:, int(0.35 * n):int(0.65 * n)] = np.nan
        dem.upload_rows(h, r0)
    return dem


def median(xs):
    return round(sorted(xs)[len(xs) // 2], 3)


def time_device(n, case, reps):
    src = with_holes(n, case)
    work = d.DeviceArray(n, n)
    out = d.DeviceArray(n, n)
    miss = d.DeviceArray(n, n, dtype=np.uint8)
    missing_share = None
    rows = []
    for mode in ("out_of_place", "in_place"):
        ts = []
        for k in range(reps + 1):
            if mode == "in_place":
                d.sync()
                _lib.check(_lib.lib().topo_amd_memcpy_d2d(work.ptr, src.ptr, src.nbytes), "memcpy_d2d")  # (not timed)
            d.mark(2 * k)
            if mode == "in_place":
                d.Block(work).fill_na(work, miss)
            else:
                d.Block(src).fill_na(out, miss)
            d.mark(2 * k + 1)
            if k:  # the first call is a warm-up
                ts.append(d.mark_elapsed(2 * k, 2 * k + 1))
        if missing_share is None:
            missing_share = float(miss.to_host().mean(dtype=np.float64))
        bpp = 9.0 if mode == "out_of_place" else 5.0 + 4.0 * missing_share
        ms = median(ts)
        rows.append({"tool": "fill_na_time", "form": "device", "n": n, "case": case, "mode": mode, "missing_share": round(missing_share, 4),
                     "ms_median": ms, "ms_min": round(min(ts), 3), "reps": reps, "bytes_per_px": round(bpp, 3),
                     "effective_TBs": round(bpp * n * n / (ms * 1e-3) / 1e12, 3),
                     "estimate_ms": round(bpp * n * n / (HBM_COPY_TBS * 1e12) * 1e3, 3)})
    for buf in (src, work, out, miss):
        buf.free()
    return rows


def time_host(n, reps):
    dem = with_holes(n, "30%+1%")
    host = dem.to_host()
    dem.free()
    ts_fill, ts_tpi = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        missing, filled = hlp.fill_na_gpu(host)
        t1 = time.perf_counter()
        topo.tpi(host, 67)
        t2 = time.perf_counter()
        if k:
            ts_fill.append((t1 - t0) * 1e3)
            ts_tpi.append((t2 - t1) * 1e3)
    rows = [{"tool": "fill_na_time", "form": "host_buffer", "n": n, "case": "30%+1%", "ms_median": median(ts_fill),
             "tpi67_host_buffer_ms_median": median(ts_tpi), "ratio_to_tpi67": round(median(ts_fill) / median(ts_tpi), 3),
             "reps": reps}]
    t0 = time.perf_counter()
    want = hlp.fill_na_array(host)
    t1 = time.perf_counter()
    same = bool(np.array_equal(want.view(np.uint32), filled.view(np.uint32)) and np.array_equal(missing, np.isnan(host)))
    rows.append({"tool": "fill_na_time", "form": "host_oracle_cpu", "n": n, "case": "30%+1%", "ms": round((t1 - t0) * 1e3, 1),
                 "gpu_bits_equal_oracle": same, "cpus": len(os.sched_getaffinity(0))})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,32768")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="0%,1%,30%+1%")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    for n in [int(s) for s in args.sizes.split(",")]:
        for case in args.cases.split(","):
            for row in time_device(n, case, args.reps):
                print(json.dumps(row), flush=True)
    if not args.no_host:
        for row in time_host(16384, args.reps):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
