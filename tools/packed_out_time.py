#!/usr/bin/env python3
"""Packed result planes (csrc/encode.hip, the *_packed entry points) against float32 ones, end to end on an n x n DEM stored
as int16: topo_amd_tpi_raw against topo_amd_tpi_std_packed with an int16 plane (67 px), and topo_amd_gradient_raw against
topo_amd_gradient_packed with two float16 and two uint16 planes (sigma 3.25), page-locked and pageable arrays.  The float32-out
and the packed-out call alternate within one run; every configuration gets a warm-up call, then three timed ones (best and
worst are printed: the spread between repeats of one configuration is the yardstick for the difference between two).  Each
part runs in a child process.  Then one packed TPI call under `rocprofv3 --kernel-trace --memory-copy-trace --stats`, a run of
its own: the encode kernel's time per row chunk against that chunk's download.

    python tools/packed_out_time.py [n=16384] [out=profiles/packed_out_time.txt]
"""
import csv
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REPS = 3


def setup(n, pinned_only=False):
    from topo_descriptors_amd import _lib
    lib = _lib.lib()
    dem = np.rint(1900.0 + 300.0 * np.random.default_rng(0).standard_normal((n, n))).astype(np.int16)

    class Host:
        """count bytes of page-locked or pageable host memory, touched"""

        def __init__(self, count, pinned):
            if pinned:
                self.h = C.c_void_p()
                _lib.check(lib.topo_amd_host_alloc(C.byref(self.h), count), "host_alloc")
                self.bytes = np.frombuffer((C.c_char * count).from_address(self.h.value), dtype=np.uint8)
            else:
                self.bytes = np.empty(count, dtype=np.uint8)
            self.bytes[:] = 0
            self.address = self.bytes.ctypes.data

    def arrays(pinned):
        src = Host(dem.nbytes, pinned)
        src.bytes[:] = dem.reshape(-1).view(np.uint8)
        return src, [Host(n * n * 4, pinned) for _ in range(4)], [Host(n * n * 2, pinned) for _ in range(4)]

    return _lib, lib, {kind: arrays(kind == "pinned") for kind in (("pinned",) if pinned_only else ("pinned", "pageable"))}


def calls(_lib, lib, n, src, floats, packed):
    import topo_descriptors_amd as tda
    raster = _lib.Raster(src.address, _lib.I16, 0, 1.0, 0.0, 0.0)
    rx, ry = np.array([30.0]), np.array([-30.0])
    tpi_dm = tda.Packing(np.int16, 0.1, 0.0, -32768)
    grad = [tda.Packing(np.float16), tda.Packing(np.float16), tda.Packing(np.uint16, 0.002, 0.0, 65535),
            tda.Packing(np.uint16, 0.01, 0.0, 65535)]
    tpi_plane = tpi_dm.struct(packed[0].address)
    grad_planes = [q.struct(b.address) for q, b in zip(grad, packed)]
    return {
        "tpi67 float32 out": lambda: _lib.check(lib.topo_amd_tpi_raw(C.byref(raster), n, n, 67, 0.0, floats[0].address), "tpi_raw"),
        "tpi67 int16 out": lambda: _lib.check(lib.topo_amd_tpi_std_packed(C.byref(raster), n, n, 67, 0.0, C.byref(tpi_plane), None),
                                              "tpi_std_packed"),
        "gradient 3.25 float32 out (4 planes)": lambda: _lib.check(lib.topo_amd_gradient_raw(
            C.byref(raster), n, n, 3.25, 1.0, 0, _lib.ptr(rx), _lib.ptr(ry), *[f.address for f in floats]), "gradient_raw"),
        "gradient 3.25 2 float16 + 2 uint16 out": lambda: _lib.check(lib.topo_amd_gradient_packed(
            C.byref(raster), n, n, 3.25, 1.0, 0, _lib.ptr(rx), _lib.ptr(ry), *[C.byref(p) for p in grad_planes]), "gradient_packed"),
    }


def child_time(n):
    _lib, lib, arrays = setup(n)
    for kind, (src, floats, packed) in arrays.items():
        fns = calls(_lib, lib, n, src, floats, packed)
        times = {k: [] for k in fns}
        for fn in fns.values():  # warm-up: the device planes, the pages
            fn()
        for _ in range(REPS):  # the configurations alternate
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        print(f"  {kind} arrays, int16 source, {n} x {n}: best / worst of {REPS} (ms), all")
        for k, t in times.items():
            print(f"    {k:42s} {min(t):8.2f} {max(t):8.2f}    {' '.join(f'{v:.2f}' for v in t)}")
        names = list(times)
        for a, b in ((names[0], names[1]), (names[2], names[3])):
            spread = max(max(times[k]) - min(times[k]) for k in (a, b))
            print(f"    {b} / {a}: {min(times[b]) / min(times[a]):.3f}  (best {min(times[b]) - min(times[a]):+.2f} ms; "
                  f"largest spread of the two {spread:.2f} ms)")


def child_trace(n):
    _lib, lib, arrays = setup(n, pinned_only=True)
    src, floats, packed = arrays["pinned"]
    fn = calls(_lib, lib, n, src, floats, packed)["tpi67 int16 out"]
    fn()
    fn()


def read_trace(folder):
    def rows(pattern):
        found = glob.glob(os.path.join(folder, "**", pattern), recursive=True)
        return list(csv.DictReader(open(found[0]))) if found else []

    def span(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    kernels = sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    copies = sorted(rows("*memory_copy_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    enc = [r for r in kernels if "encode_kernel" in r["Kernel_Name"]]
    enc = enc[len(enc) // 2:]  # the second call
    if not enc:
        return ["    no encode kernel in the trace"]
    t0 = int(enc[0]["Start_Timestamp"])
    down = [r for r in copies if "DEVICE_TO_HOST" in r.get("Direction", "").upper() and int(r["Start_Timestamp"]) >= t0 and span(r) > 50.0]
    out = [f"    second call: {len(enc)} encode launches, {len(down)} downloads of more than 50 us behind the first of them",
           "    chunk   encode us   download us   encode / download"]
    for k, e in enumerate(enc):
        dn = span(down[k]) if k < len(down) else float("nan")
        out.append(f"    {k:5d} {span(e):11.1f} {dn:13.1f} {span(e) / dn:19.3f}")
    others = {}
    for r in kernels:
        if int(r["Start_Timestamp"]) >= t0 - 1 and "encode_kernel" not in r["Kernel_Name"]:
            name = r["Kernel_Name"].replace("void topo::(anonymous namespace)::", "")[:60]
            others[name] = others.get(name, 0.0) + span(r)
    out.append(f"    encode total {sum(span(e) for e in enc):.1f} us, downloads total {sum(span(r) for r in down):.1f} us; the other kernels of the call:")
    out += [f"      {v:10.1f} us  {k}" for k, v in sorted(others.items(), key=lambda kv: -kv[1])]
    stats = glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)
    if stats:
        out.append("    rocprofv3 --stats, kernels (both calls):")
        out += ["      " + line.rstrip() for line in open(stats[0]).read().splitlines()[:8]]
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    if len(sys.argv) > 2 and sys.argv[2] in ("time", "trace"):
        (child_time if sys.argv[2] == "time" else child_trace)(n)
        return
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "packed_out_time.txt")
    me = os.path.abspath(__file__)
    lines = [f"packed result planes against float32 ones, {n} x {n}, int16 source (tools/packed_out_time.py)"]
    run = subprocess.run([sys.executable, me, str(n), "time"], capture_output=True, text=True, timeout=900, check=False)
    lines += run.stdout.splitlines()
    if run.returncode != 0:  # (nothing more is started on the GPU after a failure)
        lines += [f"the timing child ended with status {run.returncode}", run.stderr[-2000:]]
    elif shutil.which("rocprofv3"):
        folder = tempfile.mkdtemp(prefix="packed_trace_")
        lines.append("  one packed TPI call (page-locked arrays) under rocprofv3 --kernel-trace --memory-copy-trace --stats:")
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", folder,
                              "-o", "packed", "--", sys.executable, me, str(n), "trace"], capture_output=True, text=True, timeout=900,
                             check=False)
        lines += read_trace(folder) if run.returncode == 0 else [f"    the traced child ended with status {run.returncode}", run.stderr[-2000:]]
        shutil.rmtree(folder, ignore_errors=True)
    else:
        lines.append("  rocprofv3 not found: no trace")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)
    sys.exit(run.returncode)


if __name__ == "__main__":
    main()
