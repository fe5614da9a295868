"""The gap fill on the GPU (csrc/fill.hip, topo_amd_fill_na_dev / _f32) against the host oracle ``helpers.fill_na_array``:
bit for bit (uint32 views), and the missing mask against ``np.isnan`` of the masked input.  With a threshold m the oracle
is ``fill_na_array(np.where(a > np.float32(m), a, nan))``: the masking of the reference's get_dem_netcdf
(helpers.py:30-31) followed by its fill_na (helpers.py:137-154)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import _lib, batch, device as d, helpers as hlp  # noqa: E402

NAN = np.float32(np.nan)


def masked(a, m):
    return a if m is None else np.where(a > np.float32(m), a, NAN).astype(np.float32)


def oracle(a, x=None, m=None):
    b = masked(a, m)
    return np.isnan(b), hlp.fill_na_array(b, x)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    gb, wb = bits(got), bits(want)
    if not np.array_equal(gb, wb):
        r, c = np.argwhere(gb != wb)[0]
        raise AssertionError(f"{what}: {int((gb != wb).sum())} samples differ, first at ({r}, {c}): "
                             f"{got[r, c]!r} (0x{gb[r, c]:08x}) != {want[r, c]!r} (0x{wb[r, c]:08x})")


def check(a, x=None, m=None, what=""):
    want_m, want = oracle(a, x, m)
    miss, got = hlp.fill_na_gpu(a, x_coords=x, min_elevation=m)
    assert got.dtype == np.float32 and got.shape == a.shape and miss.dtype == np.bool_
    assert_same(got, want, what)
    assert np.array_equal(miss, want_m), what
    return got


def terrain(rng, ny, nx):
    return (rng.random((ny, nx)) * 3000.0 - 50.0).astype(np.float32)


def holes(rng, ny, nx, share, kind):
    bad = np.zeros((ny, nx), bool)
    if kind == "isolated":
        bad = rng.random((ny, nx)) < share
    elif kind == "sea":  # one block over a band of rows
        w = int(round(share * nx))
        if w:
            c0 = int(rng.integers(0, nx - w + 1))
            r0 = int(rng.integers(0, ny))
            bad[r0:r0 + max(1, ny // 2), c0:c0 + w] = True
    else:  # runs of 1 ... 300 columns, crossing the 64-column words
        for r in range(ny):
            while bad[r].mean() < share:
                n = int(rng.integers(1, 301))
                c0 = int(rng.integers(-n + 1, nx))
                bad[r, max(0, c0):c0 + n] = True
    return bad


WIDTHS = [1, 2, 3, 63, 64, 65, 127, 129, 1000, 3601, 4097]


@pytest.mark.parametrize("nx", WIDTHS)
def test_seeded_sweep(nx):
    rng = np.random.default_rng(1000 + nx)
    cases = 0
    for share in (0.0, 0.01, 0.1, 0.3, 0.6, 0.9, 0.99, 1.0):
        for kind in ("isolated", "sea", "runs"):
            ny = int(rng.integers(1, 12)) * 2 + 1  # odd row counts
            a = terrain(rng, ny, nx)
            a[holes(rng, ny, nx, share, kind)] = NAN
            check(a, what=f"{nx} {share} {kind}")
            cases += 1
            if kind != "sea":
                continue
            # the same with nodata under a threshold, and with coordinates
            b = a.copy()
            b[holes(rng, ny, nx, share / 2, "isolated")] = -9999.0
            check(b, m=-100.0, what=f"{nx} {share} threshold")
            x = 2600000.0 + 25.0 * np.arange(nx)
            check(b, x=x, m=-100, what=f"{nx} {share} coords")
            cases += 2
    assert cases == 40


def tie_rows(rng, ny, nx):
    """Rows of single valid samples with gaps of odd length: the middle sample of each gap is a tie by index."""
    a = np.full((ny, nx), NAN, np.float32)
    for r in range(ny):
        c = int(rng.integers(0, 3))
        while c < nx:
            a[r, c] = np.float32(rng.random() * 1000.0)
            c += 2 * int(rng.integers(1, 40))
    return a


def test_ties_index_and_coordinates():
    rng = np.random.default_rng(7)
    ny, nx = 31, 3601
    a = tie_rows(rng, ny, nx)
    by_index = check(a, what="index ties")
    # even gaps of the column index: a tie goes to the left sample
    r = 0
    cols = np.flatnonzero(~np.isnan(a[r]))
    L, R = cols[0], cols[1]
    if (R - L) % 2 == 0 and R - L >= 2:
        assert bits(by_index)[r, (L + R) // 2] == bits(a)[r, L]
    # 0.1 * i: the midpoints are rounded, so some ties fall the other way - the coordinate rule must be followed
    x = 0.1 * np.arange(nx)
    by_coords = check(a, x=x, what="0.1 * i")
    assert (bits(by_coords) != bits(by_index)).any()
    # descending (a tie goes to the smaller coordinate: the right-hand sample) and uneven coordinates
    down = 5000.0 - 0.7 * np.arange(nx)
    by_down = check(a, x=down, what="descending")
    assert (bits(by_down) != bits(by_index)).any()
    uneven = np.cumsum(rng.random(nx) * 3.0 + 0.01)
    check(a, x=uneven, what="uneven")
    check(a, x=-uneven, what="uneven descending")
    check(a, x=np.cumsum(np.where(np.arange(nx) % 2, 1.0, 3.0)), what="alternating steps")


def test_edge_rows():
    nan_payloads = np.array([0x7FC01234, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    inf = np.float32(np.inf)
    a = np.full((9, 70), NAN, np.float32)
    a[0, :4] = nan_payloads                      # no valid sample: the NaNs keep their bits
    a[1, 30] = 5.0                               # one valid sample: left alone
    a[1, 60:64] = nan_payloads
    a[2, [3, 40]] = [inf, -inf]                  # +-inf are valid samples, copied as they are
    a[3, [0, 69]] = [np.float32(-0.0), 7.0]      # -0.0 is valid and keeps its sign
    a[4, :] = np.arange(70, dtype=np.float32)    # nothing missing
    a[5, 10:12] = [1.0, 2.0]
    a[6, 64] = 3.0
    a[6, 0] = 4.0
    a[7, 63:65] = [8.0, 9.0]                     # two valid samples either side of a word edge
    a[8, ::2] = -np.arange(35, dtype=np.float32)
    got = check(a, what="edge rows")
    assert np.array_equal(bits(got[0]), bits(a[0])) and np.array_equal(bits(got[1]), bits(a[1]))
    assert bits(got[3])[1] == 0x80000000
    # -9999 nodata under min_elevation = -100; -inf is masked by the threshold, +inf is not
    b = a.copy()
    b[4, 5:20] = -9999.0
    b[5, 30] = -9999.0
    b[2, 10] = -100.0                            # at the threshold: masked
    b[3, 20] = np.float32(-99.99)
    got = check(b, m=-100.0, what="threshold")
    assert np.array_equal(bits(got[0]), np.full(70, 0x7FC00000, np.uint32))  # masked rows hold numpy's NaN
    check(b, m=-100.0, x=np.linspace(-3.0, 11.0, 70), what="threshold, coordinates")


def test_wide_rows():
    """Rows wider than the on-chip words (65536 columns): the second form, a gap of more than 100 000 columns."""
    rng = np.random.default_rng(3)
    nx = 1 << 20
    a = terrain(rng, 2, nx)
    a[0, 200000:350001] = NAN
    a[1, :70000] = NAN
    a[1, 500000:500003] = NAN
    a[1, -65:] = NAN
    a[rng.random((2, nx)) < 0.01] = NAN
    check(a, what="2 x 2^20")
    check(a, x=1000.0 - 0.5 * np.arange(nx), what="2 x 2^20 descending")


def device_fill(a, x=None, m=None, in_place=False):
    ny, nx = a.shape
    src = d.DeviceArray.from_host(a)
    miss = d.DeviceArray(ny, nx, dtype=np.uint8)
    blk = d.Block(src)
    out = src if in_place else d.DeviceArray(ny, nx)
    blk.fill_na(out, miss, x_coords=x, min_elevation=m)
    d.sync()
    return out.to_host(), miss.to_host(), src.to_host()


def test_in_place_equals_out_of_place():
    rng = np.random.default_rng(5)
    for nx, m in ((1000, None), (3601, -100.0), (70000, None)):
        a = terrain(rng, 9, nx)
        a[holes(rng, 9, nx, 0.3, "runs")] = NAN
        a[holes(rng, 9, nx, 0.05, "isolated")] = -9999.0
        a[4] = NAN
        f_out, m_out, src = device_fill(a, m=m)
        assert np.array_equal(bits(src), bits(a))  # out of place: the input is left alone
        f_in, m_in, _ = device_fill(a, m=m, in_place=True)
        want_m, want = oracle(a, m=m)
        assert_same(f_out, want, f"out of place {nx}")
        assert_same(f_in, want, f"in place {nx}")
        assert np.array_equal(m_out, want_m.astype(np.uint8)) and np.array_equal(m_in, m_out)


def test_row_blocks_give_the_whole_raster():
    rng = np.random.default_rng(9)
    ny, nx = 157, 1000
    a = terrain(rng, ny, nx)
    a[holes(rng, ny, nx, 0.3, "sea")] = NAN
    a[holes(rng, ny, nx, 0.02, "isolated")] = -9999.0
    x = np.cumsum(rng.random(nx) + 0.5)
    want_m, want = oracle(a, x, -100.0)
    for cut in (1, 37, 64, 156):
        got = np.empty_like(a)
        miss = np.empty(a.shape, np.uint8)
        for r0, r1 in ((0, cut), (cut, ny)):
            part = d.DeviceArray.from_host(a[r0:r1])
            out = d.DeviceArray(r1 - r0, nx)
            mo = d.DeviceArray(r1 - r0, nx, dtype=np.uint8)
            d.Block(part, row0=r0, gny=ny).fill_na(out, mo, x_coords=x, min_elevation=-100.0)
            d.sync()
            got[r0:r1], miss[r0:r1] = out.to_host(), mo.to_host()
        assert_same(got, want, f"cut {cut}")
        assert np.array_equal(miss, want_m.astype(np.uint8))
    # output rows of a larger block (rows around them in the buffer), in place
    whole = d.DeviceArray.from_host(a)
    d.Block(whole, row0=0, gny=ny).fill_na(whole, x_coords=x, min_elevation=-100.0, out_row0=40, out_rows=50)
    d.sync()
    h = whole.to_host()
    assert_same(h[40:90], want[40:90], "rows 40 ... 89 in place")
    assert np.array_equal(bits(h[:40]), bits(a[:40])) and np.array_equal(bits(h[90:]), bits(a[90:]))


class Pinned:
    def __init__(self, shape, dtype):
        self.p = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _lib.check(_lib.lib().topo_amd_host_alloc(C.byref(self.p), n), "host_alloc")
        self.a = np.frombuffer((C.c_char * n).from_address(self.p.value), dtype=dtype).reshape(shape)

    def free(self):
        self.a = None
        _lib.check(_lib.lib().topo_amd_host_free(self.p), "host_free")


def test_host_buffer_form_in_chunks(monkeypatch):
    """TOPO_AMD_HOST_CHUNK_MB=1 cuts a 1024-column call into chunks of 960 rows: 3100 rows run in three."""
    monkeypatch.setenv("TOPO_AMD_HOST_CHUNK_MB", "1")
    rng = np.random.default_rng(11)
    ny, nx = 3100, 1024
    a = terrain(rng, ny, nx)
    a[900:1000, 100:700] = -9999.0  # nodata across the first seam
    a[holes(rng, ny, nx, 0.02, "isolated")] = NAN
    a[1919:1921] = NAN
    x = 100.0 - 0.25 * np.arange(nx)
    for m in (None, -100.0):
        want_m, want = oracle(a, x, m)
        dev_f, dev_m, _ = device_fill(a, x, m)
        assert_same(dev_f, want, "device form")
        miss, got = hlp.fill_na_gpu(a, x_coords=x, min_elevation=m)
        assert d.host_chunks() == 3
        assert_same(got, dev_f, "pageable")
        assert np.array_equal(miss, dev_m.astype(bool)) and np.array_equal(miss, want_m)
        src, out, mo = Pinned((ny, nx), np.float32), Pinned((ny, nx), np.float32), Pinned((ny, nx), np.uint8)
        try:
            src.a[:] = a
            mm = np.nan if m is None else m
            _lib.check(_lib.lib().topo_amd_fill_na_f32(_lib.ptr(src.a), ny, nx, x.ctypes.data_as(_lib._f64p), mm,
                                                       _lib.ptr(out.a), _lib.ptr(mo.a)), "fill_na_f32")
            assert d.host_chunks() == 3
            assert_same(out.a, dev_f, "page-locked")
            assert np.array_equal(mo.a, dev_m)
            # the caller's array filled in place, without the mask
            _lib.check(_lib.lib().topo_amd_fill_na_f32(_lib.ptr(src.a), ny, nx, x.ctypes.data_as(_lib._f64p), mm,
                                                       _lib.ptr(src.a), None), "fill_na_f32 in place")
            assert_same(src.a, dev_f, "page-locked, in place")
        finally:
            for p in (src, out, mo):
                p.free()


def test_bad_coordinates_are_refused_by_the_library():
    a = np.ones((4, 5), np.float32)
    out = np.empty_like(a)
    for x in (np.array([0.0, 1.0, 1.0, 2.0, 3.0]), np.array([0.0, 1.0, np.inf, 3.0, 4.0])):
        rc = _lib.lib().topo_amd_fill_na_f32(_lib.ptr(a), 4, 5, x.ctypes.data_as(_lib._f64p), np.nan, _lib.ptr(out), None)
        assert rc == -1 and b"x_coords" in _lib.lib().topo_amd_last_error()


def test_in_place_fill_drops_the_raster_class():
    """Fractional elevations of 0 ... 50 m and -9999 nodata: TPI at 21 px takes the scaled route, whose unit comes from the
    raster's value range.  Once the nodata are filled in place, the buffer's remembered class is stale: the second TPI must
    equal TPI of the host-filled raster uploaded fresh."""
    rng = np.random.default_rng(13)
    ny, nx = 300, 400
    a = (rng.random((ny, nx)) * 50.0).astype(np.float32)
    a[holes(rng, ny, nx, 0.2, "sea")] = -9999.0
    a[holes(rng, ny, nx, 0.01, "isolated")] = -9999.0
    dem = d.DeviceArray.from_host(a)
    blk = d.Block(dem)
    tpi = d.DeviceArray(ny, nx)
    blk.tpi_std(21, tpi=tpi)
    d.sync()
    before = tpi.to_host()
    blk.fill_na(dem, min_elevation=-100)
    blk.tpi_std(21, tpi=tpi)
    d.sync()
    after = tpi.to_host()
    _, filled = oracle(a, m=-100)
    assert_same(dem.to_host(), filled, "filled in place")
    fresh = d.DeviceArray.from_host(filled)
    t2 = d.DeviceArray(ny, nx)
    d.Block(fresh).tpi_std(21, tpi=t2)
    d.sync()
    assert_same(after, t2.to_host(), "TPI after the in-place fill")
    assert not np.array_equal(bits(before), bits(after))


class FakeDataset:
    """The few Dataset features the batch wrappers use (xarray is not needed)."""

    def __init__(self, dem, x, y):
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(x, ("x",)), "y": FakeVar(y, ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


def test_compute_tpi_takes_the_mask_as_ind_nans():
    rng = np.random.default_rng(17)
    ny, nx = 180, 256
    a = (rng.random((ny, nx)) * 800.0 + 400.0).astype(np.float32)
    a[holes(rng, ny, nx, 0.1, "sea")] = NAN
    a[holes(rng, ny, nx, 0.01, "isolated")] = -9999.0
    missing, filled = hlp.fill_na_gpu(a, min_elevation=-100)
    assert missing.any()
    x = 2600000.0 + 30.0 * np.arange(nx)
    y = 1200000.0 - 30.0 * np.arange(ny)
    ds = FakeDataset(filled, x, y)
    by_mask = batch.compute_tpi(ds, [150, 500], ind_nans=missing, outdir=None)
    by_index = batch.compute_tpi(ds, [150, 500], ind_nans=np.nonzero(missing), outdir=None)
    assert set(by_mask) == set(by_index)
    for k in by_mask:
        assert np.array_equal(bits(by_mask[k]), bits(by_index[k]))
        assert np.isnan(by_mask[k][missing]).all()


def test_dataarray_like_is_rewrapped():
    class Wrapped:
        def __init__(self, values):
            self.values = values

        def copy(self, data):
            return Wrapped(data)

    a = np.array([[1.0, np.nan, 3.0, np.nan]], np.float32)
    missing, out = hlp.fill_na_gpu(Wrapped(a))
    assert isinstance(out, Wrapped)
    assert np.array_equal(out.values, [[1.0, 1.0, 3.0, 3.0]]) and missing.tolist() == [[False, True, False, True]]
