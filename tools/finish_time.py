#!/usr/bin/env python3
"""The finishing step on the GPU (csrc/finish.hip, topo_amd_finish_dev, the crop= / ind_nans= of batch.compute_*).

Part 1, the kernel: an n x n resident float32 plane, a uint8 mask plane with every third sample set, and the window inset by
`inset` px on every side, stored as float32, int16, uint8 and float16.  topo_amd_finish_dev is timed against
topo_amd_encode_dev of the same number of (contiguous) samples and against a plain device-to-device copy of the window's float32
bytes; every call ends in a synchronise and is timed by the host clock, the three alternate, best and worst of REPS.

Part 2, end to end: batch.compute_tpi at 67 px with int16 packing and a mask with a NaN third, with and without the crop,
against the path before the finishing step existed - the whole plane encoded and downloaded, the fill code put back on the
host through the mask, a numpy slice - restated here.  That path is also run on the library of the parent commit where one is
given (TOPO_AMD_LIBRARY in a child process).  Each part runs in a child process.

    python tools/finish_time.py [n=16384] [out=profiles/finish_time.txt] [parent library]
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REPS = 5
INSET = 1000


def best_worst(times):
    return f"{min(times):8.2f} {max(times):8.2f}"


def child_kernel(n, inset):
    import topo_descriptors_amd as tda
    from topo_descriptors_amd import _lib, device as d
    lib = _lib.lib()
    rows = cols = n - 2 * inset
    count = rows * cols
    plane = d.synth_dem(n, n, seed=3, integer=False)
    flags = np.zeros(n * n, dtype=np.uint8)
    flags[::3] = 1
    mask = d.DeviceArray(n, n, dtype=np.uint8)
    mask.upload_rows(flags.reshape(n, n))
    out = d.DeviceArray(rows, cols)  # (float32: room for every type)
    packings = {"float32": tda.Packing(np.float32), "int16": tda.Packing(np.int16, 0.1, 0.0, -32768),
                "uint8": tda.Packing(np.uint8, 20.0, 0.0, 255), "float16": tda.Packing(np.float16)}
    print(f"  window {rows} x {cols} at ({inset}, {inset}) of a resident {n} x {n} plane, {count / 1e6:.1f} M samples; "
          f"best / worst of {REPS} (ms), GB/s of the best (bytes the step has to move)")
    for name, q in packings.items():
        item = q.dtype.itemsize
        s = q.struct(out.ptr)

        def finish(mask_ptr):
            _lib.check(lib.topo_amd_finish_dev(plane.ptr, n, n, mask_ptr, inset, rows, inset, cols, C.byref(s)), "finish_dev")

        def encode():
            _lib.check(lib.topo_amd_encode_dev(plane.ptr, count, C.byref(s)), "encode_dev")

        def copy():
            _lib.check(lib.topo_amd_memcpy_d2d(out.ptr, plane.ptr, count * 4), "memcpy_d2d")
            d.sync()

        fns = {"finish, mask": (lambda: finish(mask.ptr), count * (5 + item)), "finish, no mask": (lambda: finish(None), count * (4 + item)),
               "encode_dev, contiguous": (encode, count * (4 + item)), "d2d copy of the float32 bytes": (copy, count * 8)}
        times = {k: [] for k in fns}
        for fn, _ in fns.values():
            fn()
        for _ in range(REPS):
            for k, (fn, _) in fns.items():
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        print(f"    {name}")
        for k, t in times.items():
            print(f"      {k:32s} {best_worst(t)} {fns[k][1] / min(t) / 1e6:9.1f} GB/s")
    for a in (plane, mask, out):
        a.free()


class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class FakeDataset:
    def __init__(self, dem, x, y):
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(x, ("x",)), "y": FakeVar(y, ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def child_e2e(n, inset, parent):
    from topo_descriptors_amd import _lib
    if parent:  # the parent commit's library has no finishing step: only the path before it runs on it
        _lib.SIGNATURES.pop("topo_amd_finish_dev")
    import topo_descriptors_amd as tda
    from topo_descriptors_amd import batch, device as d
    dem = np.rint(1900.0 + 300.0 * np.random.default_rng(0).standard_normal((n, n))).astype(np.float32)
    x = 2600000.0 + 100.0 * np.arange(n)
    y = 1200000.0 - 100.0 * np.arange(n)
    ds = FakeDataset(dem, x, y)
    crop = {"x": slice(x[inset], x[n - inset - 1]), "y": slice(y[inset], y[n - inset - 1])}
    missing = np.zeros(n * n, dtype=np.bool_)
    missing[::3] = True
    missing = missing.reshape(n, n)
    packing = tda.Packing(np.int16, 0.1, 0.0, -32768)

    def before():
        """compute_tpi as it was: the whole plane packed and downloaded, the fill code put back on the host, a numpy slice"""
        res = batch._ResidentDem(dem)
        out = res.plane()
        try:
            res.block.tpi_std(67, tpi=out)
            array = out.to_packed(packing)
            codes = array.values
            was = codes[missing]
            codes[missing] = codes.dtype.type(array.fill_value)
            array.missing += int(was.size - np.count_nonzero(was == array.fill_value))
            return np.ascontiguousarray(codes[inset:n - inset, inset:n - inset]), array.missing
        finally:
            out.free()
            res.close()

    fns = {"before: whole plane, host re-insertion, numpy slice": before}
    if not parent:
        fns["compute_tpi, ind_nans, no crop"] = lambda: batch.compute_tpi(ds, [6700], ind_nans=missing, outdir=None, pack=packing)
        fns["compute_tpi, ind_nans, crop"] = lambda: batch.compute_tpi(ds, [6700], ind_nans=missing, crop=crop, outdir=None, pack=packing)
    results = {k: fn() for k, fn in fns.items()}  # warm-up
    if not parent:
        cropped = results["compute_tpi, ind_nans, crop"]["TPI_6700M"]
        same = np.array_equal(cropped.values, results["before: whole plane, host re-insertion, numpy slice"][0])
        print(f"  the cropped call's codes are those of the path before, sliced: {same}; route {d.tpi_route()}")
    times = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    print(f"  {'parent library' if parent else 'this library'}, TPI 67 px of a {n} x {n} float32 DEM (pageable), int16 out, a third of the "
          f"samples in ind_nans (boolean mask), domain inset by {inset} px: best / worst of 3 (ms), all")
    for k, t in times.items():
        print(f"    {k:52s} {best_worst(t)}    {' '.join(f'{v:.1f}' for v in t)}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    if len(sys.argv) > 2 and sys.argv[2] in ("kernel", "e2e", "e2e_parent"):
        inset = min(INSET, n // 8)
        if sys.argv[2] == "kernel":
            child_kernel(n, inset)
        else:
            child_e2e(n, inset, sys.argv[2] == "e2e_parent")
        return
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "finish_time.txt")
    parent = sys.argv[3] if len(sys.argv) > 3 else None
    me = os.path.abspath(__file__)
    lines = [f"the finishing step on the GPU: window, mask, packing (tools/finish_time.py), {n} x {n}"]
    status = 0
    for part in ("kernel", "e2e", "e2e_parent"):
        env = dict(os.environ)
        if part == "e2e_parent":
            if not parent:
                lines.append("  no parent library given: the path before was timed on this library only")
                continue
            env["TOPO_AMD_LIBRARY"] = os.path.abspath(parent)
        run = subprocess.run([sys.executable, me, str(n), part], capture_output=True, text=True, timeout=900, check=False, env=env)
        lines += run.stdout.splitlines()
        if run.returncode != 0:  # (nothing more is started on the GPU after a failure)
            lines += [f"the {part} child ended with status {run.returncode}", run.stderr[-2000:]]
            status = run.returncode
            break
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
