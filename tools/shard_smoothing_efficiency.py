"""Row-shard efficiency of the smoothed descriptors on ONE GPU: the step of one 4096-row shard of the 8-way split of the
32768^2 DEM through the live RCCL exchange in loop-back (TOPO_AMD_HALO_LOOPBACK=1: the shard is its own upper and lower
neighbour), against one eighth of the single-GPU time of the whole DEM - the Gaussian (topo.dem), TPI with pre-smoothing
and the valley index with pre-smoothing (Block.gaussian into a plane, then the descriptor on it, as batch.compute_* runs).

    python tools/shard_smoothing_efficiency.py [keys ...] [--out FILE]

Prints one JSON object (and writes it to FILE): per key the whole-DEM ms, the shard ms and
shard_efficiency = full_ms / (8 x shard_ms).  Device events, warm-up calls first, medians.  Loop-back only: both ends of
the link are one device, so this is the per-shard step of an 8-GPU run minus the wire."""
import json
import os
import sys

os.environ.setdefault("TOPO_AMD_HALO_LOOPBACK", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from topo_descriptors_amd import _lib, device as d, shard as shard_mod, topo  # noqa: E402

NY = NX = int(os.environ.get("SHARD_EFF_N", "32768"))
PARTS = 8
REPS = int(os.environ.get("SHARD_EFF_REPS", "8"))
KEYS = ("gauss_s3.25", "gauss_s30.25", "tpi_s67_sigma8", "valley_s21_sigma2.5")
VALLEY = topo._valley_ridge_tables(topo._valley_kernels(21, [0, 0.15, 0.3]), np.arange(0, 180, dtype=np.float32))


def median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def shard_steps(sd, outs):
    taps, ksize, angles = VALLEY
    return {
        "gauss_s3.25": lambda: sd.gaussian(3.25, outs[0]),
        "gauss_s30.25": lambda: sd.gaussian(30.25, outs[0]),
        "tpi_s67_sigma8": lambda: sd.tpi_std(67, tpi=outs[0], sigma=8.0),
        "valley_s21_sigma2.5": lambda: sd.valley_ridge(taps, ksize, angles, 3, outs[0], outs[1], sigma=2.5),
    }


def full_steps(blk, outs, smooth):
    taps, ksize, angles = VALLEY

    def smoothed(sigma, then):
        def run():
            blk.gaussian(sigma, sigma, smooth)
            then(d.Block(smooth))
        return run

    def valley(b):
        mean, stdev = d.mean_std(smooth)
        b.valley_ridge(taps, ksize, angles, 3, mean, stdev, outs[0], outs[1])

    return {
        "gauss_s3.25": lambda: blk.gaussian(3.25, 3.25, outs[0]),
        "gauss_s30.25": lambda: blk.gaussian(30.25, 30.25, outs[0]),
        "tpi_s67_sigma8": smoothed(8.0, lambda b: b.tpi_std(67, tpi=outs[0])),
        "valley_s21_sigma2.5": smoothed(2.5, valley),
    }


def main():
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i : i + 2]
    keys = [k for k in args if k in KEYS] or list(KEYS)
    _lib.lib()
    shard_mod.ShardedDEM.init_comm(0, 1, lambda payload: payload)
    rows = NY // PARTS
    deep = max(max(shard_mod.halo_rows(_lib.DESC_GAUSS, 30.25)), max(shard_mod.halo_rows(_lib.DESC_TPI, 67, 8.0)),
               max(shard_mod.halo_rows(_lib.DESC_VALLEY_RIDGE, int(VALLEY[1].max()), 2.5)))
    plan = shard_mod.RowShardPlan(3 * rows, NX, 3, 1, deep, deep)  # the middle shard of three; its neighbours are itself
    sd = shard_mod.ShardedDEM(plan)
    d.synth_dem(rows, NX, row0=plan.row0, seed=0, out=sd.block, out_row=plan.halo_above)
    outs = [d.DeviceArray(rows, NX) for _ in range(2)]
    d.sync()
    shard_ms = {}
    fns = shard_steps(sd, outs)
    for _ in range(2):  # two rounds: the second one with the clocks up
        for k in keys:
            shard_ms[k] = median(d.time_launches(fns[k], REPS, 2))
    d.sync()
    for o in outs:
        o.free()
    sd.block.free()
    full = d.synth_dem(NY, NX, seed=0)
    outs = [d.DeviceArray(NY, NX) for _ in range(2)]
    smooth = d.DeviceArray(NY, NX)
    fns = full_steps(d.Block(full), outs, smooth)
    full_ms = {}
    for _ in range(2):
        for k in keys:
            full_ms[k] = median(d.time_launches(fns[k], max(3, REPS // 2), 1))
    d.sync()
    res = {}
    for k in keys:
        res[k] = {"full_ms": round(full_ms[k], 4), "shard_ms": round(shard_ms[k], 4),
                  "shard_efficiency": round(full_ms[k] / (PARTS * shard_ms[k]), 4)}
    doc = {"dem": [NY, NX], "shard_rows": rows, "ghost_rows": deep, "loopback_only": True, "keys": res}
    print(json.dumps(doc))
    if out_file:
        with open(out_file, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
