"""numpy's float32 moments across row shards (topo_amd_shard_mean_std_f32, topo_amd_shard_valley_ridge_std; route 3 of
topo_amd_valley_moments_route) under the live ghost-row exchange, on ONE GPU.

The loop-back fixture of tests/test_gpu_shard_smoothing.py: rank 1 of a local block stacked three times, ghost rows poisoned
with 0xFF before each call.  In loop-back the rank forms its parts at every placement of the periodic stack, so
``ShardedDEM.mean_std_numpy`` yields the moments of the whole stacked raster: they are compared bit for bit with
``device.mean_std_numpy`` of the stacked plane (one GPU, one launch per pass) and with ``helpers.numpy_order_moments`` of it,
and the sharded valley / ridge index with the single GPU's ``topo_amd_valley_ridge_std_dev`` on the stacked raster - which the
float64 route does not give.

With a pre-smoothing sigma the moments are of the OWNED smoothed rows at every placement, i.e. of the middle third of the
single GPU's smoothed stack, stacked three times (the Gaussian reflects at the stack's first and last row, which a periodic
stack does not have: the first and last third of the smoothed stack are not what rank 1 stands for)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import topo_oracle as orc

pytestmark = pytest.mark.gpu

from topo_descriptors_amd import _lib, device as d, helpers as hlp, shard  # noqa: E402

EINVAL = -1  # TOPO_AMD_EINVAL


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


def _shard(local, up, down, gny=None):
    """ShardedDEM of rank 1 of `local` stacked three times, the whole buffer poisoned before the rows go in."""
    rows, nx = local.shape
    plan = shard.RowShardPlan(3 * rows if gny is None else gny, nx, 3, 1, up, down)
    assert plan.rows_local == rows
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


def _same(got, want, what):
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(g, w), (what, int(np.count_nonzero(g != w)))


def _same_pair(got, want, what):
    for g, w in zip(got, want):
        assert np.asarray(g).dtype == np.float32 and np.float32(g).tobytes() == np.float32(w).tobytes(), (what, got, want)


def _free(*arrays):
    for a in arrays:
        a.free()


def _valley_tables(size):
    from topo_descriptors_amd import topo
    flats = [0, 0.15, 0.3]
    taps, ksize, angles = topo._valley_ridge_tables(topo._valley_kernels(size, flats),
                                                    np.arange(0, 180, 9, dtype=np.float32))
    return taps, ksize, angles, len(flats)


def _single_valley(whole, taps, ksize, angles, planes, chunk):
    """topo_amd_valley_ridge_std_dev on the whole device raster: (norm, direction, (mean, std))."""
    n, a = d.DeviceArray(whole.rows, whole.nx), d.DeviceArray(whole.rows, whole.nx)
    mom = np.zeros(2, dtype=np.float32)
    _lib.check(_lib.lib().topo_amd_valley_ridge_std_dev(
        whole.ptr, whole.rows, whole.nx, taps.ctypes.data_as(_lib._vp), ksize.ctypes.data_as(_lib._i32p),
        angles.ctypes.data_as(_lib._vp), ksize.size, planes, chunk, n.ptr, a.ptr, mom.ctypes.data_as(_lib._f32p)),
        "valley_ridge_std_dev")
    return n, a, (mom[0], mom[1])


# ---- the moments alone ------------------------------------------------------------------------------------------------------
# 40 x 203 = 8120 samples at offset 8120: nx % 4 != 0 (the kernel's scalar-load form), cuts mid-chunk; with chunk 8192 the
# shard holds no whole chunk and everything travels as fragments; 192 x 384 = 9 default chunks a shard, cuts on chunk
# boundaries; 64 x 520 = 32.5 chunks of 1024: the middle placement starts mid-chunk.
@pytest.mark.parametrize("integer", [True, False], ids=["metres", "fractional"])
@pytest.mark.parametrize("rows,nx,chunk", [(40, 203, 128), (40, 203, 8192), (192, 384, None), (64, 520, 1024)])
def test_shard_mean_std_numpy_is_the_single_gpu_and_numpy(loopback, rows, nx, chunk, integer):
    local = orc.synthetic_dem(rows, nx, seed=101, integer=integer)
    sd = _shard(local, 2, 3)
    for _ in range(2):
        _poison(sd)
        got = sd.mean_std_numpy(chunk)
    stacked = np.concatenate([local] * 3, axis=0)
    whole = d.DeviceArray.from_host(stacked)
    _same_pair(got, d.mean_std_numpy(whole, chunk), "single GPU")
    _same_pair(got, hlp.numpy_order_moments(stacked, chunk), "model")
    _same_pair(got, hlp.numpy_order_moments_sharded([local] * 3, chunk), "sharded model")
    _free(whole, sd.block)


# ---- the valley / ridge index with them ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,route_bit", [(7, 8), (21, 16)])  # the fold kernel, the streamed form
def test_shard_valley_ridge_numpy_moments_is_the_single_gpu(loopback, size, route_bit, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "100000")
    rows, nx = 192, 384
    local = orc.synthetic_dem(rows, nx, seed=71, integer=True)
    taps, ksize, angles, planes = _valley_tables(size)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()))
    sd = _shard(local, up, down)
    n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        mom = sd.valley_ridge(taps, ksize, angles, planes, n, a, numpy_moments=True, moments=True)
    assert d.valley_moments_route() == 3
    route = d.valley_route()
    assert route & 1 and route & route_bit, route
    assert sd.valley_ridge(taps, ksize, angles, planes, n, a, numpy_moments=True) is None
    d.sync()
    whole = d.DeviceArray.from_host(np.concatenate([local] * 3, axis=0))
    _same_pair(mom, d.mean_std_numpy(whole), "moments")
    n2, a2, mom2 = _single_valley(whole, taps, ksize, angles, planes, hlp.moments_chunk())
    _same_pair(mom, mom2, "moments of the single call")
    got = n.to_host()
    assert np.isfinite(got).all()
    _same(got, n2.to_host(rows, rows), (size, "norm"))
    _same(a.to_host(), a2.to_host(rows, rows), (size, "direction"))
    _free(n, a, n2, a2, whole, sd.block)


def _smoothed_single(stacked, sigma):
    whole = d.DeviceArray.from_host(stacked)
    smooth = d.DeviceArray(whole.rows, whole.nx)
    d.Block(whole).gaussian(sigma, sigma, smooth)
    return whole, smooth


def _periodic_smoothed(smooth, rows):
    """What rank 1 stands for in loop-back: the middle third of the single GPU's smoothed stack at every placement."""
    return d.DeviceArray.from_host(np.concatenate([smooth.to_host(rows, rows)] * 3, axis=0))


@pytest.mark.parametrize("size,route_bit", [(7, 8), (21, 16)])
def test_shard_valley_ridge_numpy_moments_smoothed(loopback, size, route_bit, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "100000")
    rows, nx, sigma = 192, 384, 2.5
    local = orc.synthetic_dem(rows, nx, seed=71, integer=True)
    taps, ksize, angles, planes = _valley_tables(size)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()), sigma)
    sd = _shard(local, up, down)
    n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        mom = sd.valley_ridge(taps, ksize, angles, planes, n, a, sigma=sigma, numpy_moments=True, moments=True)
    assert d.valley_moments_route() == 3
    route = d.valley_route()
    assert route & 1 and route & route_bit, route
    d.sync()
    whole, smooth = _smoothed_single(np.concatenate([local] * 3, axis=0), sigma)
    stack = _periodic_smoothed(smooth, rows)
    _same_pair(mom, d.mean_std_numpy(stack), "moments of the smoothed plane")
    n2, a2 = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    d.Block(smooth).valley_ridge(taps, ksize, angles, planes, mom[0], mom[1], n2, a2, out_row0=rows, out_rows=rows)
    d.sync()
    got = n.to_host()
    assert np.isfinite(got).all()
    _same(got, n2.to_host(), (size, "norm"))
    _same(a.to_host(), a2.to_host(), (size, "direction"))
    _free(n, a, n2, a2, whole, smooth, stack, sd.block)


@pytest.mark.parametrize("sigma", [None, 1.5])
def test_shard_valley_ridge_numpy_moments_fft(loopback, sigma, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "1")
    rows, nx = 160, 256
    local = orc.synthetic_dem(rows, nx, seed=73, integer=True)
    taps, ksize, angles, planes = _valley_tables(7)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()), sigma or 0.0)
    sd = _shard(local, up, down)
    n, a = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    for _ in range(2):
        _poison(sd)
        mom = sd.valley_ridge(taps, ksize, angles, planes, n, a, sigma=sigma, numpy_moments=True, moments=True)
    assert d.valley_route() == 2 and d.valley_moments_route() == 3
    d.sync()
    stacked = np.concatenate([local] * 3, axis=0)
    n2, a2 = d.DeviceArray(rows, nx), d.DeviceArray(rows, nx)
    if sigma is None:
        whole = d.DeviceArray.from_host(stacked)
        source = whole
        _same_pair(mom, d.mean_std_numpy(whole), "moments")
    else:
        whole, source = _smoothed_single(stacked, sigma)
        stack = _periodic_smoothed(source, rows)
        _same_pair(mom, d.mean_std_numpy(stack), "moments of the smoothed plane")
        stack.free()
    d.Block(source).valley_ridge(taps, ksize, angles, planes, mom[0], mom[1], n2, a2, out_row0=rows, out_rows=rows)
    d.sync()
    norm, want = n.to_host(), n2.to_host()
    assert np.isfinite(norm).all()
    assert np.max(np.abs(norm - want)) <= 1e-5 * float(np.max(np.abs(want)))
    assert np.mean(a.to_host() == a2.to_host()) >= 0.995
    _free(n, a, n2, a2, whole, sd.block)
    if source is not whole:
        source.free()


# ---- the default is today's call; refusals ------------------------------------------------------------------------------------
def test_default_is_the_float64_route_and_bad_requests_are_refused(loopback, monkeypatch):
    monkeypatch.setenv("TOPO_AMD_VALLEY_FFT_MIN_KERNEL", "100000")
    rows, nx = 160, 256
    local = orc.synthetic_dem(rows, nx, seed=79, integer=False)
    taps, ksize, angles, planes = _valley_tables(7)
    up, down = shard.halo_rows(_lib.DESC_VALLEY_RIDGE, int(ksize.max()))
    sd = _shard(local, up, down)
    outs = [d.DeviceArray(rows, nx) for _ in range(4)]
    _poison(sd)
    assert sd.valley_ridge(taps, ksize, angles, planes, outs[0], outs[1]) is None
    assert d.valley_moments_route() == 2
    _poison(sd)
    mom = sd.valley_ridge(taps, ksize, angles, planes, outs[2], outs[3], numpy_moments=False, moments=True)
    assert d.valley_moments_route() == 2 and isinstance(mom[0], float)
    d.sync()
    _same(outs[2].to_host(), outs[0].to_host(), "norm")
    _same(outs[3].to_host(), outs[1].to_host(), "direction")
    # a chunk that is no power of two of 128 or more
    lib, p = _lib.lib(), sd.plan
    m, s = C.c_float(), C.c_float()
    for chunk in (100, 64):
        assert lib.topo_amd_shard_mean_std_f32(sd.block.row_ptr(p.halo_above), p.rows_local, p.row0, p.gny, p.nx, chunk,
                                               C.byref(m), C.byref(s)) == EINVAL
        with pytest.raises(_lib.TopoAmdError, match="chunk"):
            sd.mean_std_numpy(chunk)
        _lib.check(lib.topo_amd_memset(outs[0].ptr, 0x7F, outs[0].nbytes), "memset")
        with pytest.raises(_lib.TopoAmdError, match="chunk"):
            sd.valley_ridge(taps, ksize, angles, planes, outs[0], outs[1], numpy_moments=chunk)
        d.sync()
        assert (outs[0].to_host().view(np.uint32) == 0x7F7F7F7F).all()  # refused before anything ran
    # the switch that sends the moments to the host: no silent fall-back to the float64 route
    monkeypatch.setenv("TOPO_AMD_VALLEY_HOST_MOMENTS", "1")
    with pytest.raises(RuntimeError, match="numpy_moments"):
        sd.valley_ridge(taps, ksize, angles, planes, outs[0], outs[1], numpy_moments=True)
    monkeypatch.delenv("TOPO_AMD_VALLEY_HOST_MOMENTS")
    # loop-back stacks whole copies of the rank's rows: 3 * rows + 1 rows are not that
    odd = _shard(local, up, down, gny=3 * rows + 1)
    q = odd.plan
    assert q.gny % q.rows_local == 1
    assert lib.topo_amd_shard_mean_std_f32(odd.block.row_ptr(q.halo_above), q.rows_local, q.row0, q.gny, q.nx, 8192,
                                           C.byref(m), C.byref(s)) == EINVAL
    with pytest.raises(_lib.TopoAmdError, match="loop-back"):
        odd.mean_std_numpy()
    _free(*outs, sd.block, odd.block)


def test_part_of_a_raster_without_a_communicator_is_refused():
    rows, nx = 40, 203
    local = orc.synthetic_dem(rows, nx, seed=5, integer=True)
    sd = _shard(local, 0, 0)
    with pytest.raises(_lib.TopoAmdError, match="no communicator"):
        sd.mean_std_numpy()
    # a shard that is the whole raster needs nobody: topo_amd_mean_std_f32_dev's bits
    whole = shard.ShardedDEM(shard.RowShardPlan(rows, nx, 1, 0, 0, 0), local)
    _same_pair(whole.mean_std_numpy(128), hlp.numpy_order_moments(local, 128), "one shard")
    _free(sd.block, whole.block)
