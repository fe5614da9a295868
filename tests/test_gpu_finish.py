"""``topo_amd_finish_dev`` (csrc/finish.hip): a window of a float32 device plane, NaN put back from a uint8 mask plane, stored
compactly as float32 or as packed samples.

The expected result comes from code the kernel does not share: the mask is set to NaN in numpy, numpy takes the slice, and
``topo_amd_encode_host`` (one host thread) encodes it.  Codes and both counters must be equal; for float32 the stored bits must
be the slice's bits (a NaN's payload included) and ``missing`` its NaN count, as include/topo_amd.h defines it
(``topo_amd_encode_host`` reports 0 for a float32 plane).  No tolerance anywhere.

Shapes: a 67 x 131 plane (nx % 4 = 3: the source row start changes its 16-byte phase with every row) and one with nx = 1;
every window of the cross col0 {0, 1, 2, 3, 5} x cols {1, 2, 3, 15, 16, 17, 64, 65, to the row end} x rows {1, 2, 7} x row0
{0, the last rows}, for every sample type and mask kind.  The output starts 0 ... 3 samples behind a 16-byte boundary (cycled
through the cases), with at least 64 sentinel bytes on either side, which must stay untouched.  One 1500 x 2051 window of a
1601 x 2300 plane per type, and a 2100 x 2051 float32 window, beyond 2048 blocks x 256 lanes x 2 groups: the grid-stride loop
takes a second trip."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import topo_descriptors_amd as tda  # noqa: E402
from topo_descriptors_amd import _lib, device as d  # noqa: E402

NY, NX = 67, 131
SENTINEL = 0xA5
GUARD = 64
PACKINGS = {
    "F32": tda.Packing(np.float32),
    "I16": tda.Packing(np.int16, 1.0, 0.0, -32768),   # scale 1: samples beyond +-32767 saturate
    "U16": tda.Packing(np.uint16, 0.5, -100.0, 65535),
    "U8": tda.Packing(np.uint8, 300.0, -30000.0, 0),
    "F16": tda.Packing(np.float16),                    # samples beyond 65504 become inf: saturated
}
MASKS = ("none", "sparse", "all", "where_nan")
COL0 = (0, 1, 2, 3, 5)
COLS = (1, 2, 3, 15, 16, 17, 64, 65, None)  # None: up to the row end
ROWS = (1, 2, 7)


def make_plane(ny, nx, seed):
    rng = np.random.default_rng(seed)
    a = (rng.normal(0.0, 25000.0, size=(ny, nx))).astype(np.float32)  # about one in five beyond int16
    a[rng.random((ny, nx)) < 0.02] *= 10.0                            # some beyond float16's range
    a[rng.random((ny, nx)) < 0.05] = np.nan
    a[rng.random((ny, nx)) < 0.01] = np.inf
    a[rng.random((ny, nx)) < 0.01] = -np.inf
    bits = a.view(np.uint32)
    bits[0, 0] = 0x7FC12345                 # NaNs with payloads, a negative one and a signalling one: float32 copies them
    bits[ny - 1, nx - 1] = 0xFFC00001
    bits[ny // 2, nx // 2] = 0x7F800123
    if nx > 8:
        bits[1, 5] = 0x7FC54321
        a[ny - 2, nx - 3] = np.inf
    return a


def make_mask(kind, plane, seed):
    if kind == "none":
        return None
    if kind == "all":
        return np.full(plane.shape, 255, dtype=np.uint8)
    if kind == "where_nan":
        return np.isnan(plane).astype(np.uint8)
    rng = np.random.default_rng(seed)
    m = np.zeros(plane.shape, dtype=np.uint8)
    hit = rng.random(plane.shape) < 0.1
    m[hit] = rng.integers(1, 256, size=int(hit.sum()), dtype=np.uint8)  # (any non-zero byte is a flag)
    return m


class Resident:
    """A plane and its masks on the GPU, and one output buffer with guard bytes, shared by the cases of a module run."""

    def __init__(self, ny, nx, seed):
        self.host = make_plane(ny, nx, seed)
        self.dev = d.DeviceArray(ny, nx)
        self.dev.upload_rows(self.host)
        self.masks_host = {k: make_mask(k, self.host, seed + 1) for k in MASKS}
        self.masks = {}
        for k, m in self.masks_host.items():
            if m is not None:
                self.masks[k] = d.DeviceArray(ny, nx, dtype=np.uint8)
                self.masks[k].upload_rows(m)
        self.out = d.DeviceArray(1, 2 * GUARD + 16 + ny * nx * 4, dtype=np.uint8)

    def free(self):
        for a in [self.dev, self.out, *self.masks.values()]:
            a.free()


@pytest.fixture(scope="module")
def small():
    r = Resident(NY, NX, 7)
    yield r
    r.free()


@pytest.fixture(scope="module")
def column():
    r = Resident(NY, 1, 9)
    yield r
    r.free()


@pytest.fixture(scope="module")
def large():
    r = Resident(2200, 2300, 11)
    yield r
    r.free()


def expected(res, kind, packing, ny, window):
    """(values, missing, saturated) from numpy and topo_amd_encode_host"""
    row0, rows, col0, cols = window
    w = res.host[:ny].copy()
    if res.masks_host[kind] is not None:
        w[res.masks_host[kind][:ny] != 0] = np.nan
    win = np.ascontiguousarray(w[row0:row0 + rows, col0:col0 + cols])
    want = _lib.encode_host(win, packing)
    if packing.dtype == np.float32:
        assert np.array_equal(want.values.view(np.uint32), win.view(np.uint32)) and (want.missing, want.saturated) == (0, 0)
        return want.values, int(np.isnan(win).sum()), 0
    return want.values, want.missing, want.saturated


def run(res, kind, packing, ny, window, phase):
    """The call on the device -> (status, values, missing, saturated, guard bytes intact)"""
    lib = _lib.lib()
    row0, rows, col0, cols = window
    item = packing.dtype.itemsize
    start = GUARD + phase * item
    nbytes = rows * cols * item
    assert start + nbytes + GUARD <= res.out.nbytes
    _lib.check(lib.topo_amd_memset(res.out.ptr, SENTINEL, res.out.nbytes), "memset")
    plane = packing.struct(res.out.ptr + start)
    plane.missing = plane.saturated = 987654321  # (the call sets them, also to 0)
    mask = res.masks.get(kind)
    status = lib.topo_amd_finish_dev(res.dev.ptr, ny, res.dev.nx, None if mask is None else mask.ptr, row0, rows, col0, cols,
                                     C.byref(plane))
    raw = res.out.to_host().reshape(-1)
    values = raw[start:start + nbytes].view(packing.dtype).reshape(rows, cols)
    intact = bool((raw[:start] == SENTINEL).all() and (raw[start + nbytes:] == SENTINEL).all())
    return status, values, plane.missing, plane.saturated, intact


def check(res, kind, name, ny, window, phase):
    packing = PACKINGS[name]
    want, missing, saturated = expected(res, kind, packing, ny, window)
    status, got, got_missing, got_saturated, intact = run(res, kind, packing, ny, window, phase)
    what = (name, kind, window, phase)
    assert status == 0, (what, _lib.load().topo_amd_last_error())
    assert intact, what
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
    assert (got_missing, got_saturated) == (missing, saturated), what
    return missing, saturated


def windows(ny, nx):
    for col0 in COL0:
        for cols in COLS:
            n = nx - col0 if cols is None else cols
            if col0 + n > nx:
                continue
            for rows in ROWS:
                for row0 in (0, ny - rows):
                    yield row0, rows, col0, n


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", list(PACKINGS))
def test_every_window_of_the_cross(small, name, kind):
    cases = list(windows(NY, NX))
    assert len(cases) == len(COL0) * len(COLS) * len(ROWS) * 2
    seen_missing = seen_saturated = 0
    for k, window in enumerate(cases):
        missing, saturated = check(small, kind, name, NY, window, phase=k % 4)
        seen_missing += missing
        seen_saturated += saturated
    print(name, kind, len(cases), "windows; missing", seen_missing, "saturated", seen_saturated)
    assert seen_missing > 0
    if name != "F32" and kind != "all":
        assert seen_saturated > 0  # (the plane does saturate every packed type)


@pytest.mark.parametrize("name", list(PACKINGS))
def test_a_plane_of_one_column(column, name):
    k = 0
    for kind in MASKS:
        for rows in (1, 2, 7, 33, NY):
            for row0 in (0, NY - rows):
                check(column, kind, name, NY, (row0, rows, 0, 1), phase=k % 4)
                k += 1


def test_the_float32_window_keeps_nan_payloads(small):
    _, got, missing, _, _ = run(small, "none", PACKINGS["F32"], NY, (0, NY, 0, NX), 1)
    bits = got.view(np.uint32)
    assert bits[0, 0] == 0x7FC12345 and bits[NY - 1, NX - 1] == 0xFFC00001 and bits[NY // 2, NX // 2] == 0x7F800123
    assert missing == int(np.isnan(small.host).sum())
    _, got, missing, _, _ = run(small, "all", PACKINGS["F32"], NY, (0, NY, 0, NX), 2)
    assert (got.view(np.uint32) == 0x7FC00000).all() and missing == NY * NX  # what ``array[ind_nans] = np.nan`` stores


@pytest.mark.parametrize("name", list(PACKINGS))
def test_a_window_of_three_million_samples(large, name):
    check(large, "sparse", name, 1601, (37, 1500, 113, 2051), phase=3)


def test_the_grid_stride_loop_takes_a_second_trip(large):
    rows, cols = 2100, 2051
    assert rows * cols // 4 > _lib.lib().topo_amd_cu_count() * 8 * 256 * 2  # groups > lanes of the largest grid x groups a trip
    check(large, "sparse", "F32", 2200, (100, rows, 249, cols), phase=1)
    check(large, "none", "F32", 2200, (100, rows, 248, cols), phase=0)


def test_an_empty_window_launches_nothing(small):
    for name in PACKINGS:
        for window in ((0, 0, 0, NX), (5, 3, 7, 0), (NY, 0, NX, 0), (0, 0, 0, 0)):
            status, _, missing, saturated, intact = run(small, "sparse", PACKINGS[name], NY, window, 0)
            assert (status, missing, saturated, intact) == (0, 0, 0, True), (name, window)


def test_invalid_windows_and_a_misaligned_plane(small):
    lib = _lib.lib()
    einval = -1  # TOPO_AMD_EINVAL
    for window in ((0, NY + 1, 0, NX), (1, NY, 0, NX), (0, NY, 0, NX + 1), (0, NY, 1, NX), (-1, 2, 0, 4), (0, -2, 0, 4),
                   (0, 2, -1, 4), (0, 2, 0, -4), (NY + 1, 0, 0, 4), (0, 2, NX + 1, 0), (2**31 - 1, 2**31 - 1, 0, 4)):
        status, _, _, _, intact = run_unchecked(small, PACKINGS["I16"], window, 0)
        assert (status, intact) == (einval, True), window
    for name, off in (("I16", 1), ("U16", 3), ("F16", 1), ("F32", 2), ("F32", 1)):
        status, _, _, _, intact = run_unchecked(small, PACKINGS[name], (0, 2, 0, 4), off)
        assert (status, intact) == (einval, True), (name, off)
    assert b"finish_dev" in lib.topo_amd_last_error()
    # an unknown sample type and a nodata inside the range: make_encode's refusals
    plane = PACKINGS["I16"].struct(small.out.ptr)
    plane.dtype = _lib.F64
    assert lib.topo_amd_finish_dev(small.dev.ptr, NY, NX, None, 0, 2, 0, 4, C.byref(plane)) == einval
    plane = PACKINGS["I16"].struct(small.out.ptr)
    plane.nodata = 5.0
    assert lib.topo_amd_finish_dev(small.dev.ptr, NY, NX, None, 0, 2, 0, 4, C.byref(plane)) == einval


def run_unchecked(res, packing, window, byte_offset):
    lib = _lib.lib()
    _lib.check(lib.topo_amd_memset(res.out.ptr, SENTINEL, res.out.nbytes), "memset")
    plane = packing.struct(res.out.ptr + GUARD + byte_offset)
    status = lib.topo_amd_finish_dev(res.dev.ptr, NY, NX, res.masks["sparse"].ptr, *window, C.byref(plane))
    raw = res.out.to_host().reshape(-1)
    return status, None, plane.missing, plane.saturated, bool((raw == SENTINEL).all())


def test_device_array_finish(small):
    """The Python layer: windows, masks, packings, the plain path and the refusals (raised before any library call)."""
    plane, mask = small.dev, small.masks["sparse"]
    assert np.array_equal(plane.finish().view(np.uint32), small.host.view(np.uint32))  # to_host()
    whole = plane.finish(PACKINGS["I16"])                                               # to_packed()
    want = _lib.encode_host(small.host, PACKINGS["I16"])
    assert np.array_equal(whole.values, want.values) and (whole.missing, whole.saturated) == (want.missing, want.saturated)
    window = (3, 40, 5, 101)
    for name, packing in PACKINGS.items():
        values, missing, saturated = expected(small, "sparse", packing, NY, window)
        got = plane.finish(None if name == "F32" else packing, mask, window)
        if name == "F32":
            assert isinstance(got, np.ndarray) and got.dtype == np.float32
            assert np.array_equal(got.view(np.uint32), values.view(np.uint32))
        else:
            assert isinstance(got, _lib.PackedPlane) and got.packing is packing
            assert np.array_equal(got.values.view(np.uint8), values.view(np.uint8))
            assert (got.missing, got.saturated) == (missing, saturated)
    masked = plane.finish(mask=mask)  # no window: the whole plane
    assert masked.shape == (NY, NX) and np.isnan(masked[small.masks_host["sparse"] != 0]).all()
    empty = plane.finish(PACKINGS["U8"], mask, (4, 0, 2, 9))
    assert empty.values.shape == (0, 9) and empty.values.dtype == np.uint8 and (empty.missing, empty.saturated) == (0, 0)
    assert plane.finish(window=(0, 5, NX, 0)).shape == (5, 0)
    for bad in ((0, NY + 1, 0, NX), (0, 1, 1, NX), (-1, 1, 0, 1), (0, 1, 0), "rows"):
        with pytest.raises(ValueError):
            plane.finish(window=bad)
    with pytest.raises(ValueError):
        plane.finish(mask=small.masks_host["sparse"])  # a host array
    with pytest.raises(ValueError):
        plane.finish(mask=plane)                        # not uint8
    with pytest.raises(ValueError):
        mask.finish()                                   # not float32
    with pytest.raises(ValueError):
        plane.finish(packing="int16")
    short = d.DeviceArray(NY - 1, NX, dtype=np.uint8)
    try:
        with pytest.raises(ValueError):
            plane.finish(mask=short)
    finally:
        short.free()
