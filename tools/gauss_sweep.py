"""The bits of the Gaussian and the gradient at every radius, for comparing two builds of the library (TOPO_AMD_LIBRARY).

Radii 0 ... 130 and 176, 177, 200 (sigma = radius / 4; the last three: wave-shift and transpose paths).  Per radius: the
Gaussian with one sigma, on axis 0 alone, on axis 1 alone and with two sigmas (sigma, sigma / 2), the gradient with sig_ratio
1 and 2.  Rasters: a (203, 1530) and a (129, 321) DEM and the first one x 1000 (the large-sample class), each clean and with a
NaN, an inf and a 3e9 sample; each as one call and as three row blocks with shard.halo_rows ghost rows.  One line per
result plane with its CRC-32, for the gradient also device.gradient_route().

  gauss_sweep.py OUT.txt              one sweep in this process, under the environment's switches
  gauss_sweep.py --all PREFIX         the sweep under no switch and under each of the five switch settings, each in a fresh
                                      process under its own time limit: PREFIX.<setting>.txt; stops at the first that fails
  gauss_sweep.py --diff A.txt B.txt   the lines that differ; exit status 1 if any
"""
import os
import subprocess
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = [("default", {}), ("split_once_0", {"TOPO_AMD_GAUSS_SPLIT_ONCE": "0"}), ("fused_0", {"TOPO_AMD_GAUSS_FUSED": "0"}),
            ("min_radius_16", {"TOPO_AMD_GAUSS_MFMA_MIN_RADIUS": "16"}), ("min_radius_1000", {"TOPO_AMD_GAUSS_MFMA_MIN_RADIUS": "1000"}),
            ("large_sample_0", {"TOPO_AMD_GAUSS_LARGE_SAMPLE": "0"})]
RADII = list(range(131)) + [176, 177, 200]
LIMIT_S = 420  # per setting


def sweep(path):
    import numpy as np
    from oracle import topo_oracle as orc
    from topo_descriptors_amd import _lib, device as d, shard

    base = [orc.synthetic_dem(203, 1530, seed=11), orc.synthetic_dem(129, 321, seed=12)]
    rasters = [("dem203", base[0]), ("dem129", base[1]), ("large203", base[0] * np.float32(1000.0))]
    lines = []
    for name, clean in rasters:
        gny, nx = clean.shape
        bad = clean.copy()
        bad[gny // 2, nx // 3] = np.nan
        bad[5, 64] = np.inf
        bad[gny - 40, 128] = 3.0e9
        cuts = shard.split_rows(gny, 3)
        whole_out = [d.DeviceArray(gny, nx) for _ in range(4)]
        part_out = [[d.DeviceArray(rows, nx) for _ in range(4)] for _, rows in cuts]
        for variant, host in (("clean", clean), ("wild", bad)):
            dev = d.DeviceArray.from_host(host)
            whole = d.Block(dev)
            scan = d.RasterScan().add(whole)  # the row blocks below take the whole raster's class

            def blocks(up, down):
                for (row0, rows), outs in zip(cuts, part_out):
                    lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
                    blk = d.Block(dev, row0=lo, gny=gny, first_buffer_row=lo, rows=hi - lo)
                    scan.declare(blk)
                    yield blk, row0, rows, outs

            def emit(what, mode, planes, route=""):
                for k, plane in enumerate(planes):
                    lines.append(f"{name} {variant} {what} {mode} plane{k} {zlib.crc32(plane.tobytes()):08x}{route}")

            for R in RADII:
                s = R / 4.0
                for tag, sy, sx in (("both", s, s), ("axis0", s, 0.0), ("axis1", 0.0, s), ("two", s, s / 2)):
                    whole.gaussian(sy, sx, whole_out[0])
                    d.sync()
                    emit(f"R{R} gaussian_{tag}", "one", [whole_out[0].to_host()])
                    parts = []
                    for blk, row0, rows, outs in blocks(*shard.halo_rows(_lib.DESC_GAUSS, sy)):
                        blk.gaussian(sy, sx, outs[0], out_row0=row0, out_rows=rows)
                        d.sync()
                        parts.append(outs[0].to_host())
                    emit(f"R{R} gaussian_{tag}", "blocks", [np.concatenate(parts)])
                for ratio in (1.0, 2.0):
                    whole.gradient(s, [30.0], [-30.0], sig_ratio=ratio, dx=whole_out[0], dy=whole_out[1], slope=whole_out[2],
                                   aspect=whole_out[3])
                    d.sync()
                    emit(f"R{R} gradient_{ratio:g}", "one", [o.to_host() for o in whole_out], f" route {d.gradient_route():#x}")
                    parts, routes = [], []
                    for blk, row0, rows, outs in blocks(*shard.halo_rows(_lib.DESC_GRADIENT, s, ratio)):
                        blk.gradient(s, [30.0], [-30.0], sig_ratio=ratio, dx=outs[0], dy=outs[1], slope=outs[2], aspect=outs[3],
                                     out_row0=row0, out_rows=rows)
                        d.sync()
                        routes.append(f"{d.gradient_route():#x}")
                        parts.append([o.to_host() for o in outs])
                    emit(f"R{R} gradient_{ratio:g}", "blocks", [np.concatenate(p) for p in zip(*parts)], " route " + ",".join(routes))
            d.forget_raster_class()
            dev.free()
        for o in whole_out + [o for outs in part_out for o in outs]:
            o.free()
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"{path}: {len(lines)} planes")


def main():
    if sys.argv[1] == "--diff":
        a, b = (open(p).read().splitlines() for p in sys.argv[2:4])
        differ = [f"< {x}\n> {y}" for x, y in zip(a, b) if x != y]
        print("\n".join(differ[:200]))
        print(f"{len(a)} / {len(b)} lines, {len(differ)} differ")
        return 1 if differ or len(a) != len(b) else 0
    if sys.argv[1] == "--all":
        for name, env in SETTINGS:
            out = f"{sys.argv[2]}.{name}.txt"
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, **env), timeout=LIMIT_S).returncode
            if rc != 0:
                print(f"{name}: exit status {rc}; stopping")
                return rc
        return 0
    sweep(sys.argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
