"""The sharded Gaussian, pre-smoothed TPI / STD and valley / ridge, and gap fill (topo_amd_shard_gaussian,
_tpi_std_smoothed, _valley_ridge_smoothed, _fill_na) under the live ghost-row exchange, on ONE GPU.

With TOPO_AMD_HALO_LOOPBACK=1 and a communicator of one rank the exchange sends to rank 0 itself with periodic wrap, so a
middle shard whose neighbours are itself is the middle third of its rows stacked three times: its results are compared
bit for bit with the single block on the stacked DEM (what batch.compute_* run: Block.gaussian into a plane, then the
descriptor on Block(plane)).  A first shard (row0 = 0) is served as well - its bottom ghost rows are its own first rows,
the second copy of the stack - and covers the Gaussian's reflect boundary at the global edge.  The ghost rows are poisoned
with 0xFF (a NaN bit pattern) before each of two calls, so a row the exchange fails to deliver shows up in the outputs."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import _lib, device as d, shard  # noqa: E402


@pytest.fixture()
def loopback():
    lib = _lib.lib()
    os.environ["TOPO_AMD_HALO_LOOPBACK"] = "1"
    uid = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    _lib.check(lib.topo_amd_comm_unique_id(uid), "comm_unique_id")
    _lib.check(lib.topo_amd_comm_init(0, 1, uid.raw), "comm_init")
    try:
        yield lib
    finally:
        _lib.check(lib.topo_amd_comm_destroy(), "comm_destroy")
        _lib.check(lib.topo_amd_shard_layout(-1, -1), "shard_layout")
        os.environ.pop("TOPO_AMD_HALO_LOOPBACK", None)


def _shard(local, up, down, rank=1, extra=(0, 0)):
    """ShardedDEM of rank `rank` of `local` stacked three times, the whole buffer poisoned before the rows go in."""
    rows, nx = local.shape
    plan = shard.RowShardPlan(3 * rows, nx, 3, rank, up + extra[0], down + extra[1])
    sd = shard.ShardedDEM(plan)
    _lib.check(_lib.lib().topo_amd_memset(sd.block.ptr, 0xFF, sd.block.nbytes), "memset")
    sd.block.upload_rows(local, plan.halo_above)
    return sd


def _poison(sd):
    p, lib = sd.plan, _lib.lib()
    if p.halo_above:
        _lib.check(lib.topo_amd_memset(sd.block.ptr, 0xFF, p.halo_above * p.nx * 4), "memset")
    if p.halo_below:
        _lib.check(lib.topo_amd_memset(sd.block.row_ptr(p.halo_above + p.rows_local), 0xFF, p.halo_below * p.nx * 4),
                   "memset")


def _dem(kind, rows, nx, seed):
    local = orc.synthetic_dem(rows, nx, seed=seed, integer=kind != "fractional")
    if kind == "nan":  # patches at both seams: their Gaussian footprints reach into the neighbouring copies
        local[:4, 100:130] = np.nan
        local[-3:, 300:305] = np.nan
    return local


def _same(got, want, what):
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(g, w), (what, int(np.count_nonzero(g != w)))


def _free(*arrays):
    for a in arrays:
        a.free()


# ---- Gaussian -----------------------------------------------------------------------------------------------------
# 0.75: vector ALU (radius 3).  3.25: fused matrix-core (radius 13, 16 ghost rows).  30.25: the split-once long filter
# (radius 121).  (2.0, 5.0): anisotropic pair.
SIGMAS = [0.75, 3.25, 30.25, (2.0, 5.0)]


@pytest.mark.parametrize("kind", ["integer", "fractional", "nan"])
@pytest.mark.parametrize("sigma", SIGMAS, ids=str)
def test_shard_gaussian_is_the_single_block(loopback, sigma, kind):
    rows, nx = 256, 520
    local = _dem(kind, rows, nx, seed=51)
    sy, sx = (sigma, sigma) if np.isscalar(sigma) else sigma
    up, down = shard.halo_rows(_lib.DESC_GAUSS, sy)
    sd = _shard(local, up, down, extra=(2, 7))  # a plan deeper than the Gaussian needs
    out = d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        sd.gaussian(sigma, out)
    d.sync()
    whole = d.DeviceArray.from_host(np.concatenate([local] * 3, axis=0))
    want = d.DeviceArray(rows, nx)
    d.Block(whole).gaussian(sy, sx, want, out_row0=rows, out_rows=rows)
    d.sync()
    got = out.to_host()
    _same(got, want.to_host(), (sigma, kind))
    assert np.isfinite(got).all() == (kind != "nan")
    _free(out, want, whole, sd.block)


@pytest.mark.parametrize("rank", [0, 2])
@pytest.mark.parametrize("sigma", [3.25, 30.25])
def test_shard_gaussian_reflects_at_the_global_edge(loopback, sigma, rank):
    """First / last shard: reflect at global row 0 / gny - 1, ghost rows from the neighbour on the other side only."""
    rows, nx = 256, 512
    local = _dem("fractional", rows, nx, seed=53)
    up, down = shard.halo_rows(_lib.DESC_GAUSS, sigma)
    sd = _shard(local, up, down, rank=rank)
    out = d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        sd.gaussian(sigma, out)
    d.sync()
    whole = d.DeviceArray.from_host(np.concatenate([local] * 3, axis=0))
    want = d.DeviceArray(rows, nx)
    d.Block(whole).gaussian(sigma, sigma, want, out_row0=rank * rows, out_rows=rows)
    d.sync()
    _same(out.to_host(), want.to_host(), (sigma, rank))
    _free(out, want, whole, sd.block)


# ---- pre-smoothed TPI / STD -----------------------------------------------------------------------------------------
def _smoothed_single(stacked, sigma):
    whole = d.DeviceArray.from_host(stacked)
    smooth = d.DeviceArray(whole.rows, whole.nx)
    d.Block(whole).gaussian(sigma, sigma, smooth)
    return whole, smooth


@pytest.mark.parametrize("kind", ["integer", "fractional"])
@pytest.mark.parametrize("sigma", [1.0, 8.0])
@pytest.mark.parametrize("size", [7, 33, 67])
def test_shard_tpi_std_smoothed_is_the_single_block(loopback, size, sigma, kind):
    rows, nx = 224, 512
    local = _dem(kind, rows, nx, seed=61)
    up, down = shard.halo_rows(_lib.DESC_TPI, size, sigma)
    sd = _shard(local, up, down)
    whole, smooth = _smoothed_single(np.concatenate([local] * 3, axis=0), sigma)
    for want_tpi, want_std in ((True, True), (True, False), (False, True)):
        t = d.DeviceArray(rows, nx) if want_tpi else None
        s = d.DeviceArray(rows, nx) if want_std else None
        for _ in range(2):
            _poison(sd)
            sd.tpi_std(size, tpi=t, std=s, sigma=sigma)
        d.sync()
        wt = d.DeviceArray(rows, nx) if want_tpi else None
        ws = d.DeviceArray(rows, nx) if want_std else None
        d.Block(smooth).tpi_std(size, tpi=wt, std=ws, out_row0=rows, out_rows=rows)
        d.sync()
        for got, want, name in ((t, wt, "tpi"), (s, ws, "std")):
            if got is not None:
                _same(got.to_host(), want.to_host(), (size, sigma, kind, want_tpi, want_std, name))
                _free(got, want)
    _free(whole, smooth, sd.block)


def test_shard_tpi_std_sigma_zero_is_the_plain_call(loopback):
    rows, nx, size = 192, 384, 33
    local = _dem("fractional", rows, nx, seed=67)
    up, down = shard.halo_rows(_lib.DESC_TPI, size)
    sd = _shard(local, up, down)
    planes = [d.DeviceArray(rows, nx) for _ in range(6)]
    _poison(sd)
    sd.tpi_std(size, tpi=planes[0], std=planes[1])
    _poison(sd)
    sd.tpi_std(size, tpi=planes[2], std=planes[3], sigma=0.0)
    _poison(sd)
    p = sd.plan
    _lib.check(_lib.lib().topo_amd_shard_layout(p.halo_above, p.halo_below), "shard_layout")
    _lib.check(_lib.lib().topo_amd_shard_tpi_std_smoothed(sd.block.ptr, p.rows_local, p.row0, p.gny, p.nx, size, -1.0,
                                                          planes[4].ptr, planes[5].ptr), "shard_tpi_std_smoothed")
    d.sync()
    for k in (2, 4):
        _same(planes[k].to_host(), planes[0].to_host(), ("tpi", k))
        _same(planes[k + 1].to_host(), planes[1].to_host(), ("std", k))
    _free(*planes, sd.block)


# ---- pre-smoothed valley / ridge ------------------------------------------------------------------------------------
def _valley_tables(size):
    from topo_descriptors_amd import topo
    flats = [0, 0.15, 0.3]
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(size, flats),
                                                    np.arange(0, 180, 9, dtype=np.float32))
    return taps, ksize, angles, len(flats)


@pytest.mark.parametrize("size,route_bit", [(7, 8), (21, 16)])  # the fold kernel, the streamed form
def test_shard_valley_ridge_smoothed_is_the_single_block(loopback, size, route_bit, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "100000")
    rows, nx, sigma = 192, 384, 2.5
    local = _dem("integer", rows, nx, seed=71)
    taps, ksize, angles, planes = _valley_tables(size)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()), sigma)
    sd = _shard(local, up, down)
    n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        mom = sd.valley_ridge(taps, ksize, angles, planes, n, a, sigma=sigma, moments=True)
    assert sd.valley_ridge(taps, ksize, angles, planes, n, a, sigma=sigma) is None
    route = d.valley_route()
    assert route & 1 and route & route_bit, route
    d.sync()
    whole, smooth = _smoothed_single(np.concatenate([local] * 3, axis=0), sigma)
    middle = d.DeviceArray.from_host(smooth.to_host(rows, rows))
    ref = d.mean_std(middle)
    assert abs(mom[0] - ref[0]) <= 1e-12 * abs(ref[0]) and abs(mom[1] - ref[1]) <= 1e-12 * abs(ref[1]), (mom, ref)
    n2, a2 = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    d.Block(smooth).valley_ridge(taps, ksize, angles, planes, mom[0], mom[1], n2, a2, out_row0=rows, out_rows=rows)
    d.sync()
    got = n.to_host()
    assert np.isfinite(got).all()
    _same(got, n2.to_host(), (size, "norm"))
    _same(a.to_host(), a2.to_host(), (size, "direction"))
    _free(n, a, n2, a2, whole, smooth, middle, sd.block)


def test_shard_valley_ridge_smoothed_fft(loopback, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "1")
    rows, nx, sigma = 160, 256, 1.5
    local = _dem("integer", rows, nx, seed=73)
    taps, ksize, angles, planes = _valley_tables(7)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()), sigma)
    sd = _shard(local, up, down)
    n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        mom = sd.valley_ridge(taps, ksize, angles, planes, n, a, sigma=sigma, moments=True)
    assert d.valley_route() == 2
    d.sync()
    whole, smooth = _smoothed_single(np.concatenate([local] * 3, axis=0), sigma)
    n2, a2 = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    d.Block(smooth).valley_ridge(taps, ksize, angles, planes, mom[0], mom[1], n2, a2, out_row0=rows, out_rows=rows)
    d.sync()
    norm, want = n.to_host(), n2.to_host()
    assert np.isfinite(norm).all()
    assert np.max(np.abs(norm - want)) <= 1e-5 * float(np.max(np.abs(want)))
    assert np.mean(a.to_host() == a2.to_host()) >= 0.995
    _free(n, a, n2, a2, whole, smooth, sd.block)


def test_shard_valley_ridge_sigma_zero_is_the_plain_call(loopback, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "100000")
    rows, nx = 160, 256
    local = _dem("integer", rows, nx, seed=79)
    taps, ksize, angles, planes = _valley_tables(7)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()))
    sd = _shard(local, up, down)
    outs = [d.DeviceArray(rows, nx) for _ in range(6)]
    _poison(sd)
    sd.valley_ridge(taps, ksize, angles, planes, outs[0], outs[1])
    _poison(sd)
    mom = sd.valley_ridge(taps, ksize, angles, planes, outs[2], outs[3], sigma=0.0, moments=True)
    _poison(sd)
    p, m2 = sd.plan, np.zeros(2)
    _lib.check(_lib.lib().topo_amd_shard_layout(p.halo_above, p.halo_below), "shard_layout")
    _lib.check(_lib.lib().topo_amd_shard_valley_ridge_smoothed(
        sd.block.ptr, p.rows_local, p.row0, p.gny, p.nx, taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(_lib._i32p),
        angles.ctypes.data_as(_lib._vp), ksize.size, planes, -2.0, outs[4].ptr, outs[5].ptr, m2.ctypes.data_as(_lib._f64p)),
        "shard_valley_ridge_smoothed")
    d.sync()
    for k in (2, 4):
        _same(outs[k].to_host(), outs[0].to_host(), ("norm", k))
        _same(outs[k + 1].to_host(), outs[1].to_host(), ("direction", k))
    assert tuple(m2) == mom
    ref = d.mean_std(d.DeviceArray.from_host(local))
    assert abs(mom[0] - ref[0]) <= 1e-12 * ref[0] and abs(mom[1] - ref[1]) <= 1e-12 * ref[1]
    _free(*outs, sd.block)


# ---- plans: deeper is the same, too shallow is refused before anything runs -------------------------------------------
def test_deeper_plan_gives_the_same_bits_and_a_shallow_one_is_refused(loopback):
    rows, nx, size, sigma = 192, 384, 33, 8.0
    local = _dem("fractional", rows, nx, seed=83)
    taps, ksize, angles, planes = _valley_tables(7)
    tpi_depth = shard.halo_rows(_lib.DESC_TPI, size, sigma)
    valley_depth = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()), sigma)
    gauss_depth = shard.halo_rows(_lib.DESC_GAUSS, sigma)
    results = []
    for extra in ((0, 0), (9, 4)):
        sd = _shard(local, *tpi_depth, extra=extra)
        outs = [d.DeviceArray(rows, nx) for _ in range(5)]
        _poison(sd)
        sd.tpi_std(size, tpi=outs[0], std=outs[1], sigma=sigma)
        _poison(sd)
        sd.gaussian(sigma, outs[2])
        _poison(sd)
        sd.valley_ridge(taps, ksize, angles, planes, outs[3], outs[4], sigma=sigma)
        d.sync()
        results.append([o.to_host() for o in outs])
        _free(*outs, sd.block)
    for k in range(5):
        _same(results[1][k], results[0][k], k)
    # one ghost row short of each descriptor: refused (the poisoned outputs stay as they were)
    for depth, call in ((tpi_depth, lambda sd, o: sd.tpi_std(size, tpi=o, sigma=sigma)),
                        (valley_depth, lambda sd, o: sd.valley_ridge(taps, ksize, angles, planes, o, o, sigma=sigma)),
                        (gauss_depth, lambda sd, o: sd.gaussian(sigma, o))):
        sd = _shard(local, depth[0] - 1, depth[1])
        o = d.DeviceArray(rows, nx)
        _lib.check(_lib.lib().topo_amd_memset(o.ptr, 0x7F, o.nbytes), "memset")
        with pytest.raises(_lib.TopoAmdError, match="ghost rows"):
            call(sd, o)
        d.sync()
        assert (o.to_host().view(np.uint32) == 0x7F7F7F7F).all()
        _free(o, sd.block)


# ---- gap fill ----------------------------------------------------------------------------------------------------
def test_shard_fill_na_out_of_place_and_in_place(loopback):
    """Decreasing x_coords and a min_elevation; then TPI on the in-place filled shard gives the single block's bits on
    the filled stack: the class declared for the raw rows (a -9999 nodata widens its range, hence the unit of the
    scaled fractional TPI) was dropped by the fill and derived again."""
    rows, nx, size = 192, 512, 33
    local = _dem("fractional", rows, nx, seed=89)
    rng = np.random.default_rng(5)
    local[rng.random(local.shape) < 0.05] = np.nan
    local[20:24, :] = np.nan                      # whole rows: left alone
    local[100:110, 200:260] = -9999.0             # nodata under min_elevation
    x = 2700000.0 - 25.0 * np.arange(nx)
    m = 0.0
    up, down = shard.halo_rows(_lib.DESC_TPI, size)
    sd = _shard(local, up, down)
    stacked = np.concatenate([local] * 3, axis=0)
    whole = d.DeviceArray.from_host(stacked)
    want, want_miss = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx, dtype=np.uint8)
    d.Block(whole).fill_na(want, want_miss, x_coords=x, min_elevation=m, out_row0=rows, out_rows=rows)
    # out of place
    out, miss = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx, dtype=np.uint8)
    sd.fill_na(out, miss, x_coords=x, min_elevation=m)
    d.sync()
    _same(out.to_host(), want.to_host(), "out of place")
    assert np.array_equal(miss.to_host(), want_miss.to_host())
    assert np.array_equal(sd.block.to_host(sd.plan.halo_above, rows).view(np.uint32), local.view(np.uint32))
    # TPI on the raw rows first: the shard's class is declared with the -9999 in it
    t = d.DeviceArray(rows, nx)
    sd.tpi_std(size, tpi=t)
    # in place
    miss2 = d.DeviceArray(rows, nx, dtype=np.uint8)
    sd.fill_na(missing=miss2, x_coords=x, min_elevation=m)
    d.sync()
    filled = sd.block.to_host(sd.plan.halo_above, rows)
    _same(filled, want.to_host(), "in place")
    assert np.array_equal(miss2.to_host(), want_miss.to_host())
    for _ in range(2):
        _poison(sd)
        sd.tpi_std(size, tpi=t)
    d.sync()
    filled_whole = d.DeviceArray.from_host(np.concatenate([filled] * 3, axis=0))
    wt = d.DeviceArray(rows, nx)
    d.Block(filled_whole).tpi_std(size, tpi=wt, out_row0=rows, out_rows=rows)
    d.sync()
    _same(t.to_host(), wt.to_host(), "tpi after the in-place fill")
    _free(whole, want, want_miss, out, miss, t, miss2, filled_whole, wt, sd.block)
