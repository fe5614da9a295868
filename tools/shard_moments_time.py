#!/usr/bin/env python3
"""What numpy's float32 moments cost a row shard (route 3: ``ShardedDEM.mean_std_numpy``, ``valley_ridge(numpy_moments=True)``)
next to the float64 moments the sharded valley / ridge index has taken so far (route 2), on ONE GPU in loop-back
(TOPO_AMD_HALO_LOOPBACK=1, a communicator of one rank), with the library's event timers (``device.time_launches``), the two
routes alternating in one process.

A shard of rows x nx whole metres, as rank 1 of ``copies`` placements (1: the shard is the raster - what one rank does on its
GPU per call; 3: loop-back forms the parts of every placement, three times the kernel work of a real rank):

  - ``mean_std_numpy`` of the shard: two passes of the window kernel, the parts downloaded, the host chain;
  - ``device.mean_std_numpy`` of the same samples as one plane (the single GPU's call);
  - ``device.mean_std``: the float64 single pass that route 2 runs before its all-reduce of three doubles;
  - the sharded valley / ridge index at 7 px with either route.

With one rank no collective runs on either route; what would travel per rank and pass is printed from the sizes.

    python tools/shard_moments_time.py [rows=4096] [nx=32768]
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REPS = 7


def row(name, times):
    return f"    {name:58s} best {min(times):8.3f}  median {sorted(times)[len(times) // 2]:8.3f}  worst {max(times):8.3f} ms"


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    nx = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
    os.environ["TOPO_AMD_HALO_LOOPBACK"] = "1"
    from topo_descriptors_amd import _lib, device as d, shard, topo
    lib = _lib.lib()
    uid = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    _lib.check(lib.topo_amd_comm_unique_id(uid), "comm_unique_id")
    _lib.check(lib.topo_amd_comm_init(0, 1, uid.raw), "comm_init")
    chunk = int(np.getbufsize())
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(7, [0, 0.15, 0.3]), np.arange(0, 180, 9, dtype=np.float32))
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()))
    print(f"shard {rows} x {nx} whole metres ({rows * nx * 4 / 2**20:.0f} MiB, {rows * nx // chunk} chunks of {chunk}), loop-back, "
          f"{REPS} timed calls each, routes alternating")
    for copies in (1, 3):
        plan = shard.RowShardPlan(copies * rows, nx, copies, copies // 2, up, down)
        sd = shard.ShardedDEM(plan)
        d.synth_dem(rows, nx, seed=7, out=sd.block, out_row=plan.halo_above)
        plane = d.synth_dem(rows, nx, seed=7)
        n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
        d.sync()
        words = (copies * rows * nx // chunk, copies * (4 + 2 * chunk))
        print(f"  rank {plan.rank} of {copies} ({copies * rows} rows): pass 1 would all-reduce {words[0]} chunk sums + {words[1]} "
              f"header / fragment words ({(words[0] + words[1]) * 4 / 1024:.0f} KiB), pass 2 {words[0]} ({words[0] * 4 / 1024:.0f} KiB); "
              f"route 2 three doubles")
        got = sd.mean_std_numpy()
        one = d.mean_std_numpy(plane)
        print(f"    moments {got[0]!r} {got[1]!r}; of the shard's samples alone {one[0]!r} {one[1]!r}")
        t3, t1, t2 = [], [], []
        for _ in range(REPS):  # alternating
            t3 += d.time_launches(sd.mean_std_numpy, 1, 0)
            t1 += d.time_launches(lambda: d.mean_std_numpy(plane), 1, 0)
            t2 += d.time_launches(lambda: d.mean_std(plane), 1, 0)
        print(row("route 3 moments, ShardedDEM.mean_std_numpy", t3))
        print(row("single GPU, device.mean_std_numpy of the same samples", t1))
        print(row("route 2 moments, device.mean_std (float64, one pass)", t2))
        v2, v3 = [], []
        call2 = lambda: sd.valley_ridge(taps, ksize, angles, 3, n, a, moments=True)  # noqa: E731
        call3 = lambda: sd.valley_ridge(taps, ksize, angles, 3, n, a, moments=True, numpy_moments=True)  # noqa: E731
        call2(), call3()
        for _ in range(REPS):
            v2 += d.time_launches(call2, 1, 0)
            assert d.valley_moments_route() == 2
            v3 += d.time_launches(call3, 1, 0)
            assert d.valley_moments_route() == 3
        print(row("valley / ridge 7 px, route 2 (float64 all-reduce)", v2))
        print(row("valley / ridge 7 px, route 3 (numpy order across shards)", v3))
        for x in (n, a, plane, sd.block):
            x.free()
    _lib.check(lib.topo_amd_comm_destroy(), "comm_destroy")


if __name__ == "__main__":
    main()
