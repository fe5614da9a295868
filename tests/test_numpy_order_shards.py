"""numpy's float32 ``mean()`` / ``std()`` of a raster from its row shards (``helpers.numpy_order_shard_parts`` /
``numpy_order_combine`` / ``numpy_order_moments_sharded``): the statement ``topo_amd_shard_mean_std_f32`` is held to.  Every
rank forms its part of numpy's summation tree - the sums of the global chunks wholly inside its samples, and the samples
before / after its first / last chunk boundary as they are - and whoever holds all parts gets the bits of the whole raster's
``mean()`` / ``std()``, however the rows are cut.  No GPU, no library load."""
import os
import socket

import numpy as np
import pytest

from oracle import topo_oracle as orc
from topo_descriptors_amd import helpers as hlp

# (chunk, nx, rows of the blocks)
CUTS = [
    # cuts mid-chunk, nx % 4 != 0, a partial last chunk of 104 samples.  (Blocks 2 and 3, 203 samples at offsets 1015 and
    # 1218, do hold one whole chunk each - [1024, 1152) and [1280, 1408): a window of 203 holds an aligned 128 whenever its
    # offset is at most 75 past a boundary.  The next case is the one with ranks that hold none.)
    (128, 203, (5, 1, 1, 9, 40)),
    # 51-sample rows: blocks 2 and 3 ([255, 306), [306, 357)) hold no whole chunk, block 3 not even a boundary; chunk 2 =
    # [256, 384) is put together from blocks 2, 3 and 4; 2856 samples end in a partial chunk of 40
    (128, 51, (5, 1, 1, 9, 40)),
    (1024, 256, (4, 4, 8)),        # every cut on a chunk boundary: no fragments, no tail
    (8192, 520, (64, 64, 64)),     # the default chunk on the GPU tests' width
    (8192, 203, (40, 40, 40)),     # shards of 8120 samples: none holds a whole chunk
    (8192, 520, (70,)),            # one block: the single-raster result
    (128, 203, (56,)),
]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


def raster(rows, nx, integer, seed=11):
    return orc.synthetic_dem(rows, nx, seed=seed, integer=integer).astype(np.float32)


def cut(dem, rows):
    edges = np.concatenate([[0], np.cumsum(rows)])
    return [dem[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("integer", [False, True], ids=["fractional", "metres"])
@pytest.mark.parametrize("chunk,nx,rows", CUTS, ids=str)
def test_sharded_model_is_the_single_raster_bit_for_bit(chunk, nx, rows, integer):
    dem = raster(sum(rows), nx, integer)
    mean, std = hlp.numpy_order_moments_sharded(cut(dem, rows), chunk)
    want = hlp.numpy_order_moments(dem, chunk)
    assert same_bits(mean, want[0]) and same_bits(std, want[1]), (mean, want[0], std, want[1])
    old = np.getbufsize()
    try:
        np.setbufsize(chunk)
        if hlp.moments_chunk() is not None:
            assert hlp.moments_chunk() == chunk
            assert same_bits(mean, dem.mean()) and same_bits(std, dem.std()), (mean, dem.mean(), std, dem.std())
            default = hlp.numpy_order_moments_sharded(cut(dem, rows))  # chunk=None: np.getbufsize()
            assert same_bits(default[0], mean) and same_bits(default[1], std)
    finally:
        np.setbufsize(old)


def test_the_cuts_hit_every_branch_of_the_combine():
    """What the comments on CUTS claim, from the parts themselves."""
    chunk, nx, rows = CUTS[1]
    dem = raster(sum(rows), nx, False)
    firsts = np.concatenate([[0], np.cumsum(rows)]) * nx
    parts = [hlp.numpy_order_shard_parts(b, f, dem.size, chunk) for b, f in zip(cut(dem, rows), firsts)]
    assert [len(p["chunk_index"]) for p in parts][1:3] == [0, 0]            # two ranks without a whole chunk
    assert parts[2]["tail"].size == 0 and parts[2]["head"].size == nx        # ... one without a chunk boundary
    assert all(p["head"].size + p["tail"].size < 2 * chunk for p in parts)
    straddle = [i for i, p in enumerate(parts) for k in ("head", "tail") if p[k].size and p[k + "_at"] // chunk == 2]
    assert sorted(set(straddle)) == [1, 2, 3]                                # one chunk from three ranks
    assert dem.size % chunk == 40 and parts[-1]["tail"].size == 40           # the partial last chunk is the last rank's tail
    owned = np.concatenate([p["chunk_index"] for p in parts])
    assert owned.size == np.unique(owned).size
    chunk, nx, rows = CUTS[2]
    dem = raster(sum(rows), nx, False)
    firsts = np.concatenate([[0], np.cumsum(rows)]) * nx
    parts = [hlp.numpy_order_shard_parts(b, f, dem.size, chunk) for b, f in zip(cut(dem, rows), firsts)]
    assert all(p["head"].size == 0 and p["tail"].size == 0 for p in parts)
    assert sum(len(p["chunk_index"]) for p in parts) == dem.size // chunk
    # parts in any order; parts that do not tile the raster are refused
    assert same_bits(hlp.numpy_order_combine(parts[::-1], dem.size, chunk), hlp.numpy_order_sum(dem.reshape(-1), chunk))
    chunk, nx, rows = CUTS[1]
    dem = raster(sum(rows), nx, False)
    firsts = np.concatenate([[0], np.cumsum(rows)]) * nx
    parts = [hlp.numpy_order_shard_parts(b, f, dem.size, chunk) for b, f in zip(cut(dem, rows), firsts)]
    with pytest.raises(ValueError, match="tile"):
        hlp.numpy_order_combine(parts[:2] + parts[3:], dem.size, chunk)


@pytest.mark.parametrize("where", ["fragment", "full chunk"])
@pytest.mark.parametrize("case", [0, 1])
def test_non_finite_samples(case, where):
    chunk, nx, rows = CUTS[case]
    dem = raster(sum(rows), nx, False)
    # row 6 is block 2, whose samples next to its cuts are fragments; row 30 lies deep inside block 4 (rows 16 ... 55)
    at = (6, 2) if where == "fragment" else (30, 10)
    firsts = np.concatenate([[0], np.cumsum(rows)]) * nx
    parts = [hlp.numpy_order_shard_parts(b, f, dem.size, chunk) for b, f in zip(cut(dem, rows), firsts)]
    flat = at[0] * nx + at[1]
    if where == "fragment":
        assert parts[2]["head_at"] <= flat < parts[2]["head_at"] + parts[2]["head"].size
    else:
        assert flat // chunk in parts[4]["chunk_index"]
    with np.errstate(all="ignore"):
        dem[at] = np.nan
        mean, std = hlp.numpy_order_moments_sharded(cut(dem, rows), chunk)
        assert np.isnan(mean) and np.isnan(std)
        dem[at] = np.inf
        mean, std = hlp.numpy_order_moments_sharded(cut(dem, rows), chunk)
        assert np.isinf(mean) and mean > 0 and np.isnan(std)
        want = hlp.numpy_order_moments(dem, chunk)
        assert np.isinf(want[0]) and np.isnan(want[1])


# ---- world of 3 over gloo: every rank computes its parts, all parts are gathered, every rank runs the same chain -------------
GLOO = (128, 203, (7, 1, 48))  # rank 1: 203 samples at offset 1421, the next boundary 115 in - no whole chunk


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out, fail):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        chunk, nx, rows = GLOO
        dem = raster(sum(rows), nx, False)
        mine = cut(dem, rows)[rank]
        first = int(sum(rows[:rank])) * nx
        n = np.float32(dem.size)

        def gathered(mean):
            parts = [None] * world
            dist.all_gather_object(parts, hlp.numpy_order_shard_parts(mine, first, dem.size, chunk, mean=mean))
            return hlp.numpy_order_combine(parts, dem.size, chunk)

        mean = gathered(None) / n
        std = np.sqrt(gathered(mean) / n)
        out.put((rank, mean.tobytes(), std.tobytes()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:  # noqa: BLE001
        fail.put(f"rank {rank}: {type(exc).__name__}: {exc}")
        raise


def test_three_ranks_over_gloo_end_with_the_single_raster_bits():
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    world = 3
    ctx = mp.get_context("spawn")
    out, fail = ctx.Queue(), ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out, fail)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    results = []
    while len(results) < world and not any(p.exitcode for p in procs):  # (a rank that died ends the wait: its peers hang)
        try:
            results.append(out.get(timeout=0.2))
        except queue.Empty:
            pass
    for p in procs:
        if len(results) < world:
            p.terminate()
        p.join(120)
    errors = []
    while not fail.empty():
        errors.append(fail.get())
    assert not errors, errors
    assert all(p.exitcode == 0 for p in procs)
    chunk, nx, rows = GLOO
    dem = raster(sum(rows), nx, False)
    want = hlp.numpy_order_moments(dem, chunk)
    assert sorted(r[0] for r in results) == list(range(world))
    for rank, mean, std in results:
        assert mean == want[0].tobytes() and std == want[1].tobytes(), rank
    sharded = hlp.numpy_order_moments_sharded(cut(dem, rows), chunk)
    assert same_bits(sharded[0], want[0]) and same_bits(sharded[1], want[1])
