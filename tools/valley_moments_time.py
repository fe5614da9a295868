#!/usr/bin/env python3
"""numpy's float32 mean / std of a device-resident DEM, formed on the GPU (csrc/moments_np.hip, ``device.mean_std_numpy``),
against what it replaces and what it is measured by, on n x n synthetic DEMs in one process with the library's event timers:

  - ``mean_std_numpy``: two passes over the plane, the chunk sums downloaded, chained on the host;
  - ``mean_std``: the float64 single pass (the yardstick for one read of the plane: the new call should stay within about 2.5 x);
  - the old way: ``to_host()`` of the whole plane, then numpy's ``mean()`` + ``std()`` (the new call should beat ``to_host()`` alone).

Then, in a child under ``rocprofv3 --kernel-trace --stats`` (a run of its own), the kernel's share of the new call, and
``compute_valley_ridge`` (one 7 px scale, unsmoothed and smoothed) with the moments formed on the device and - the wrapper as it
was, call for call - taken on the host (``TOPO_AMD_VALLEY_HOST_MOMENTS=1``).

    python tools/valley_moments_time.py [sizes=8192,32768] [wrapper n=8192] [out=profiles/valley_moments_time.txt]
"""
import csv
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
REPS = 5


def timed(d, fn, reps=REPS):
    """(result, [ms]) of ``reps`` calls between two events each, after one untimed call."""
    out = fn()
    times = []
    for _ in range(reps):
        d.timer_start()
        out = fn()
        times.append(d.timer_stop())
    return out, times


def row(name, times):
    return f"    {name:44s} best {min(times):9.3f}  median {sorted(times)[len(times) // 2]:9.3f}  worst {max(times):9.3f} ms"


def child_moments(n):
    from topo_descriptors_amd import device as d
    dem = d.synth_dem(n, n, seed=7)
    d.sync()
    print(f"  {n} x {n} whole metres, {n * n * 4 / 2**30:.2f} GiB ({n * n // 8192} chunks of 8192 samples, tail {n * n % 8192})")
    got, t_new = timed(d, lambda: d.mean_std_numpy(dem))
    f64, t_f64 = timed(d, lambda: d.mean_std(dem))
    host, t_down = timed(d, dem.to_host, reps=3)
    t0 = time.perf_counter()
    want = (host.mean(), host.std())
    t_numpy = (time.perf_counter() - t0) * 1e3
    print(row("mean_std_numpy (two passes + host chain)", t_new))
    print(row("mean_std (float64, one pass)", t_f64))
    print(row("to_host() of the plane", t_down))
    print(f"    {'numpy mean() + std() of that array':44s} once {t_numpy:9.3f} ms")
    same = got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    print(f"    mean {got[0]!r} std {got[1]!r}: {'the bits of numpy' if same else f'NOT numpy ({want[0]!r}, {want[1]!r})'}; float64 {f64[0]:.6f} {f64[1]:.6f}")
    print(f"    mean_std_numpy / mean_std {min(t_new) / min(t_f64):.2f} (expected: about 2.5 at most); "
          f"mean_std_numpy / to_host() {min(t_new) / min(t_down):.3f} (expected: below 1)")
    dem.free()
    return 0 if same else 1


def child_trace(n):
    from topo_descriptors_amd import device as d
    dem = d.synth_dem(n, n, seed=7)
    for _ in range(3):
        d.mean_std_numpy(dem)
    dem.free()


def read_trace(folder, calls=3):
    found = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if not found:
        return ["    no kernel trace"]
    spans = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in csv.DictReader(open(found[0]))
             if "np_partials_kernel" in r["Kernel_Name"]]
    if len(spans) != 2 * calls:
        return [f"    {len(spans)} launches of the moments kernel in the trace, expected {2 * calls}"]
    last = spans[-2:]
    return [f"    the last call's two launches of np_partials_kernel: {last[0]:.3f} + {last[1]:.3f} ms (sums, squared deviations); what is left "
            "of the call is the download of the chunk sums, the chain over them and the tail, twice"]


class Var:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class Dataset:
    def __init__(self, dem):
        ny, nx = dem.shape
        self._v = {"dem": Var(dem, ("y", "x")), "x": Var(2600000.0 + 30.0 * np.arange(nx), ("x",)),
                   "y": Var(1200000.0 - 30.0 * np.arange(ny), ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def child_wrapper(n):
    from topo_descriptors_amd import batch, device as d
    plane = d.synth_dem(n, n, seed=7)
    ds = Dataset(plane.to_host())
    plane.free()
    print(f"  compute_valley_ridge, {n} x {n}, one scale of 200 m = 7 px, outdir=None: wall clock of 3 calls after one (s)")
    results = {}
    for fact in (None, 1):
        for forced in ("0", "1"):
            os.environ["TOPO_AMD_VALLEY_HOST_MOMENTS"] = forced

            def call():
                t0 = time.perf_counter()
                out = batch.compute_valley_ridge(ds, [200], "valley", smth_factors=[fact], outdir=None)
                return time.perf_counter() - t0, out

            _, out = call()
            times = [call()[0] for _ in range(3)]
            results[(fact, forced)] = out
            where = "host (to_host + numpy, as before)" if forced == "1" else "device (mean_std_numpy)"
            print(f"    {'smoothed  ' if fact else 'unsmoothed'} moments on the {where:36s} {' '.join(f'{t:7.3f}' for t in times)}   moments route {d.valley_moments_route()}")
    same = all(np.array_equal(a, b, equal_nan=True) for fact in (None, 1)
               for a, b in zip(results[(fact, "0")].values(), results[(fact, "1")].values()))
    print(f"    planes of the two paths: {'bit-identical' if same else 'DIFFERENT'}")
    return 0 if same else 1


def main():
    children = {"moments": child_moments, "trace": child_trace, "wrapper": child_wrapper}
    if len(sys.argv) > 2 and sys.argv[1] in children:
        sys.exit(children[sys.argv[1]](int(sys.argv[2])) or 0)
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "8192,32768").split(",")]
    wrapper_n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "valley_moments_time.txt")
    me = os.path.abspath(__file__)
    lines = ["numpy's float32 mean / std formed on the GPU (tools/valley_moments_time.py); times between two events around each call"]
    status = 0

    def child(args, prefix=()):
        nonlocal status
        run = subprocess.run([*prefix, sys.executable, me, *args], capture_output=True, text=True, timeout=900, check=False)
        if not prefix:
            lines.extend(run.stdout.splitlines())
        if run.returncode != 0:  # (nothing more is started on the GPU after a failure)
            status = run.returncode
            lines.extend([f"  the child {' '.join(args)} ended with status {run.returncode}", run.stderr[-2000:]])
        return run

    for n in sizes:
        if not status:
            child(["moments", str(n)])
        if not status and shutil.which("rocprofv3"):
            folder = tempfile.mkdtemp(prefix="moments_trace_")
            run = child(["trace", str(n)], prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", folder, "-o",
                                                   "moments", "--"))
            if run.returncode == 0:
                lines.extend(read_trace(folder))
            shutil.rmtree(folder, ignore_errors=True)
    if not status:
        child(["wrapper", str(wrapper_n)])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
