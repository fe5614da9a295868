"""Valley / ridge index with more than four flat fractions (reference topo.py:390-447 takes a flat_list of any length).

The kernels evaluate at most four planes at a time; a call with more runs them in groups of four, carries each group's best
UNCLIPPED with the index of its angle, merges on (larger value, then smaller index) and clips at the end
(``topo_amd_valley_route`` + 32); the FFT evaluates all planes in one pass.  Against the reference itself
(``golden/valley_ridge_flats.npz``, ``golden/make_golden_flats.py``), the float64 oracle, hand-built ties, non-finite windows,
row blocks and the shard / batch paths."""
import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import _lib, batch, device as d, shard, topo  # noqa: E402

GROUPED = 32
ROUTE_CODE = {"direct": 0 + GROUPED, "matrix": 1 + 4 + GROUPED, "folded": 1 + 4 + 8 + GROUPED, "fft": 2}
STREAMED = 1 + 4 + 8 + 16 + GROUPED


def _set_route(monkeypatch, route):
    """The same switches as tests/test_gpu_valley_ridge.py (read at every launch)."""
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "1" if route == "fft" else "100000")
    if route == "direct":
        monkeypatch.setenv("TOPO_AMD_VALLEY_MFMA_MAX_KERNEL", "0")
    else:
        monkeypatch.delenv("TOPO_AMD_VALLEY_MFMA_MAX_KERNEL", raising=False)
    if route == "matrix":
        monkeypatch.setenv("TOPO_AMD_VALLEY_FOLD", "0")
    else:
        monkeypatch.delenv("TOPO_AMD_VALLEY_FOLD", raising=False)


def _block_run(dem, taps, ksize, angles, n_planes, nblocks=1, stats=None):
    gny, nx = dem.shape
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()))
    mean, stdev = stats if stats else (float(dem.mean()), float(dem.std()))
    norms, dirs = [], []
    for row0, rows in shard.split_rows(gny, nblocks):
        lo, hi = max(0, row0 - up), min(gny, row0 + rows + down)
        dev = d.DeviceArray.from_host(dem[lo:hi])
        n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
        d.Block(dev, row0=lo, gny=gny).valley_ridge(taps, ksize, angles, n_planes, mean, stdev, n, a,
                                                    out_row0=row0, out_rows=rows)
        d.sync()
        norms.append(n.to_host())
        dirs.append(a.to_host())
        for x in (dev, n, a):
            x.free()
    return np.concatenate(norms), np.concatenate(dirs)


FLAT_TAGS = ["int_valley_s7_f5", "int_ridge_s9_f6", "int_valley_s21_f5", "frac_valley_s9_f8_sig"]


@pytest.mark.parametrize("route", ["direct", "matrix", "folded", "fft"])
@pytest.mark.parametrize("tag", FLAT_TAGS)
def test_many_flats_against_the_reference(golden, tag, route, monkeypatch):
    """test_valley_ridge_against_the_reference's tolerances, 5, 6 and 8 flat fractions."""
    _set_route(monkeypatch, route)
    g = golden("valley_ridge_flats")
    p = g[f"{tag}_params"]
    size, mode, sigma, flats = int(p[0]), ("valley", "ridge")[int(p[1])], (None if p[2] < 0 else float(p[2])), list(p[3:])
    dem = g["dem_int"] if tag.startswith("int") else g["dem_frac"]
    norm_ref, dir_ref = g[f"{tag}_norm"], g[f"{tag}_dir"]
    norm, direction = topo.valley_ridge(dem, size, mode, flats, sigma)
    want = ROUTE_CODE[route]
    if size == 21 and route == "folded":
        want = STREAMED
    if size == 21 and route == "matrix":
        want = ROUTE_CODE["direct"]  # a 30-cell canvas is beyond the unfolded form: tap by tap
    assert d.valley_route() == want
    assert norm.dtype == np.float32 and direction.dtype == np.float32 and norm.shape == dem.shape
    scale = float(np.max(np.abs(norm_ref)))
    floor = float(g[f"{tag}_norm_floor"])
    assert np.max(np.abs(norm - norm_ref)) <= floor + 1e-4 * scale, tag
    (norm_ex, _), maps = orc.valley_ridge_exact(dem, size, mode, flats, sigma, return_maps=True)
    assert np.max(np.abs(norm - norm_ex)) <= 1e-4 * scale, tag
    assert np.all((direction >= 0) & (direction <= 179) & (direction == np.round(direction)))
    at_gpu_dir = np.take_along_axis(maps, direction.astype(int)[None], axis=0)[0]
    assert np.max(np.max(maps, axis=0) - at_gpu_dir) <= 1e-4 * scale, tag
    assert np.mean(direction == dir_ref) >= 0.99, (tag, float(np.mean(direction == dir_ref)))


@pytest.mark.parametrize("form", ["matrix", "folded"])
@pytest.mark.parametrize("size,planes", [(7, 5), (7, 6), (9, 8), (5, 16), (13, 5), (21, 5), (21, 6)])
def test_many_flats_against_float64_and_the_tap_by_tap_kernel(size, planes, form, monkeypatch):
    """test_matrix_pipe_against_the_tap_by_tap_kernel_and_float64's bounds for 5 to 16 planes, over the cells, folded and
    streamed (21 px); the matrix-pipe error against the tap-by-tap route's on the same tables."""
    flats = [round(0.4 * i / (planes - 1), 4) for i in range(planes)]
    dem = (orc.synthetic_dem(96, 130, seed=size + planes) + np.random.default_rng(size).uniform(0, 1, (96, 130))).astype(np.float32)
    angles = np.arange(0, 177, 7 if size > 11 else 3, dtype=np.float32)
    taps, ksize, ang = topo._valley_ridge_tables(topo._valley_kernels(size, flats), angles)
    assert taps.size == int((ksize.astype(np.int64) ** 2).sum()) * 4 * ((planes + 3) // 4)
    _set_route(monkeypatch, "direct")
    norm_d, dir_d = _block_run(dem, taps, ksize, ang, planes)
    assert d.valley_route() == ROUTE_CODE["direct"]
    _set_route(monkeypatch, form)
    norm_m, dir_m = _block_run(dem, taps, ksize, ang, planes)
    if form == "matrix" and size > 13:
        assert d.valley_route() == ROUTE_CODE["direct"]  # beyond the unfolded form: the whole call tap by tap
        return
    assert d.valley_route() == (STREAMED if size > 17 else ROUTE_CODE[form])
    (norm_ex, _), maps = orc.valley_ridge_exact(dem, size, "valley", flats, angles=angles, return_maps=True)
    scale = float(np.max(norm_ex))
    err_m, err_d = float(np.max(np.abs(norm_m - norm_ex))), float(np.max(np.abs(norm_d - norm_ex)))
    assert err_d <= 1e-5 * scale, (err_d, scale)
    bound = 3e-6 if size > 17 else 2e-6
    assert err_m <= bound * scale and err_m <= 1.5 * err_d + 1e-7 * scale, (err_m, err_d, scale)
    index = np.searchsorted(angles, dir_m)
    assert np.all(angles[index] == dir_m)
    assert np.max(np.max(maps, axis=0) - np.take_along_axis(maps, index[None], axis=0)[0]) <= 1e-5 * scale
    assert np.mean(dir_m == dir_d) >= 0.99


# hand-built 1 x 1 kernels, 4 angles x 5 planes (two groups: planes 0-3, plane 4).  z > 0: the maximum 2 z is reached at angle
# index 0 and index 2, in DIFFERENT groups; z < 0: the best is 0.1 z at index 3, and the other group's best at index 1 is smaller
# (0.25 z) but clips to the same 0 - so merging clipped groups would give index 1.
TIE_WEIGHTS = np.array([[0.5, 0.5, 0.5, 0.5, 2.0],
                        [0.25, 0.25, 0.25, 0.25, 0.25],
                        [2.0, 0.5, 0.5, 0.5, 0.5],
                        [1.0, 1.0, 1.0, 1.0, 0.1]], dtype=np.float32)


@pytest.mark.parametrize("route", ["direct", "matrix", "folded", "fft"])
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("angles", [[10, 20, 30, 40], [40, 30, 20, 10]])
def test_ties_across_plane_groups_take_the_earlier_angle_index(route, swap, angles, monkeypatch):
    w = TIE_WEIGHTS.copy()
    if swap:  # the other group holds the earlier of the two tied angles
        w[:, [0, 4]] = w[:, [4, 0]]
    taps = np.zeros((4, 8), dtype=np.float32)
    taps[:, :5] = w
    taps = taps.reshape(-1)
    ksize = np.ones(4, dtype=np.int32)
    ang = np.asarray(angles, dtype=np.float32)
    dem = orc.synthetic_dem(70, 90, seed=31, integer=False)
    mean, stdev = float(dem.mean()), float(dem.std())
    z = (dem - np.float32(mean)) / np.float32(stdev)
    assert np.all(z != 0) and np.any(z > 0) and np.any(z < 0)
    _set_route(monkeypatch, route)
    norm, direction = _block_run(dem, taps, ksize, ang, 5, stats=(mean, stdev))
    assert d.valley_route() == ROUTE_CODE[route]
    clear = np.abs(z) > 1e-3  # (the FFT's rounding must not flip a sign)
    pos, neg = clear & (z > 0), clear & (z < 0)
    assert np.all(direction[pos] == ang[0]) and np.all(direction[neg] == ang[3])
    assert np.all(norm[neg] == 0)
    assert np.max(np.abs(norm[pos] - 2 * z[pos])) <= 1e-5 * float(np.max(z))


@pytest.mark.parametrize("form", ["direct", "matrix", "folded"])
def test_many_flats_non_finite_windows_take_the_tap_by_tap_bits(form, monkeypatch):
    """6 planes, NaN / inf samples: exactly the pixels whose window (the cells with a tap in any plane) holds one have the
    direct route's bits, every other pixel those of the clean DEM; nothing left marked; row blocks keep the bits."""
    size, flats = 7, [0, 0.1, 0.2, 0.3, 0.4, 0.5]
    clean = (orc.synthetic_dem(150, 210, seed=5) + np.random.default_rng(1).uniform(0, 1, (150, 210))).astype(np.float32)
    dem = clean.copy()
    dem[40, 50] = np.nan
    dem[100:103, 150] = np.inf
    dem[0, 0] = np.nan
    dem[31, 64] = np.nan            # on a tile seam of the matrix-pipe kernels (32 rows x 64 columns)
    special = ~np.isfinite(dem)
    angles = np.arange(0, 180, 2, dtype=np.float32)
    taps, ksize, ang = topo._valley_ridge_tables(topo._valley_kernels(size, flats), angles)
    stats = (float(clean.mean()), float(clean.std()))
    _set_route(monkeypatch, "direct")
    norm_d, dir_d = _block_run(dem, taps, ksize, ang, 6, stats=stats)
    _set_route(monkeypatch, form)
    norm_m, dir_m = _block_run(dem, taps, ksize, ang, 6, stats=stats)
    assert d.valley_route() == ROUTE_CODE[form]
    norm_c, dir_c = _block_run(clean, taps, ksize, ang, 6, stats=stats)
    assert np.all(norm_m >= 0)
    kmax = int(ksize.max())
    live = np.zeros((kmax, kmax), bool)
    pos = 0
    for ks in ksize:
        t = taps[pos:pos + ks * ks * 8].reshape(ks, ks, 8)[:, :, :6]
        sh = kmax // 2 - ks // 2
        live[sh:sh + ks, sh:sh + ks] |= np.any(t != 0, axis=2)
        pos += ks * ks * 8
    touched = np.zeros(dem.shape, bool)
    for y, x in zip(*np.nonzero(special)):
        for ky, kx in zip(*np.nonzero(live)):
            oy, ox = y - (ky - kmax // 2), x - (kx - kmax // 2)
            if 0 <= oy < dem.shape[0] and 0 <= ox < dem.shape[1]:
                touched[oy, ox] = True
    assert touched.sum() > 150
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)  # noqa: E731
    assert same(norm_m[touched], norm_d[touched]) and same(dir_m[touched], dir_d[touched])
    assert same(norm_m[~touched], norm_c[~touched]) and same(dir_m[~touched], dir_c[~touched])
    for nb in (2, 5):
        norm_b, dir_b = _block_run(dem, taps, ksize, ang, 6, nb, stats=stats)
        assert same(norm_b, norm_m) and same(dir_b, dir_m), nb


@pytest.mark.parametrize("route", ["direct", "matrix", "folded"])
def test_many_flats_row_blocks_are_bit_identical(route, monkeypatch):
    _set_route(monkeypatch, route)
    dem = orc.synthetic_dem(150, 200, seed=9)
    flats = [0, 0.1, 0.2, 0.3, 0.4]
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(9, flats), np.arange(0, 180, 7, dtype=np.float32))
    whole = _block_run(dem, taps, ksize, angles, 5, 1)
    assert d.valley_route() == ROUTE_CODE[route]
    for nb in (2, 3, 7):
        parts = _block_run(dem, taps, ksize, angles, 5, nb)
        assert np.array_equal(parts[0], whole[0]) and np.array_equal(parts[1], whole[1]), nb


def test_single_rank_shard_with_many_flats_equals_the_block_call():
    """ShardedDEM.valley_ridge (one rank, loop-back: device moments, interior / seam split) with 5 planes against
    Block.valley_ridge with the same mean / std."""
    dem = orc.synthetic_dem(140, 192, seed=21)
    gny, nx = dem.shape
    flats = [0, 0.1, 0.2, 0.3, 0.4]
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(7, flats), np.arange(0, 180, 5, dtype=np.float32))
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()))
    sd = shard.ShardedDEM(shard.RowShardPlan(gny, nx, 1, 0, up, down), dem)
    n, a = d.DeviceArray(gny, nx), d.DeviceArray(gny, nx)
    sd.valley_ridge(taps, ksize, angles, len(flats), n, a)
    d.sync()
    assert d.valley_route() == ROUTE_CODE["folded"]
    dev = d.DeviceArray.from_host(dem)
    mean, stdev = d.mean_std(dev)
    n2, a2 = d.DeviceArray(gny, nx), d.DeviceArray(gny, nx)
    d.Block(dev).valley_ridge(taps, ksize, angles, len(flats), mean, stdev, n2, a2)
    d.sync()
    assert np.array_equal(n2.to_host(), n.to_host()) and np.array_equal(a2.to_host(), a.to_host())
    for x in (n, a, n2, a2, dev):
        x.free()


class _Var:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class _Dataset:
    def __init__(self, dem, x, y):
        self._v = {"dem": _Var(dem, ("y", "x")), "x": _Var(x, ("x",)), "y": _Var(y, ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


def test_compute_valley_ridge_with_many_flats_equals_the_single_call():
    ny, nx = 120, 160
    dem = orc.synthetic_dem(ny, nx, seed=8)
    ds = _Dataset(dem, 2600000.0 + 30.0 * np.arange(nx), 1200000.0 - 30.0 * np.arange(ny))
    flats = [0, 0.1, 0.2, 0.3, 0.4]
    out = batch.compute_valley_ridge(ds, 200, "ridge", flat_list=flats, smth_factors=None, outdir=None)
    assert set(out) == {"ridge_NORM_200M", "ridge_DIR_200M"}
    norm, direction = topo.valley_ridge(dem, 7, "ridge", flats)
    assert np.array_equal(out["ridge_NORM_200M"], norm) and np.array_equal(out["ridge_DIR_200M"], direction)


def test_more_planes_than_the_limit_are_refused_by_the_library():
    dem = orc.synthetic_dem(40, 50, seed=2)
    dev = d.DeviceArray.from_host(dem)
    n, a = d.DeviceArray(40, 50), d.DeviceArray(40, 50)
    taps = np.zeros(4 * 20, dtype=np.float32)
    with pytest.raises(_lib.TopoAmdError, match="17 kernel planes"):
        d.Block(dev).valley_ridge(taps, np.ones(1, np.int32), np.zeros(1, np.float32), 17, 0.0, 1.0, n, a)
    for x in (dev, n, a):
        x.free()
