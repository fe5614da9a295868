"""numpy's own float32 ``mean()`` / ``std()`` restated (``helpers.numpy_order_moments``): the statement the GPU's moments kernel
(csrc/moments_np.hip) is held to must itself equal numpy bit for bit - chunks of ``np.getbufsize()`` samples summed pairwise,
the chunk sums chained - and the Python layer must fall back to the host's moments when that cannot be relied on.  No GPU."""
import numpy as np
import pytest

from topo_descriptors_amd import _lib, helpers as hlp

COUNTS = [1, 5, 8, 127, 128, 129, 8191, 8192, 8193, 16385, 3 * 8192 + 77, (300, 1003), (2049, 2051)]


def same_bits(a, b):
    return np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def terrain(shape, kind, seed):
    z = np.random.default_rng(seed).normal(1800.0, 600.0, size=shape)
    return {"metres": np.rint(z), "fractional": z, "millimetres": np.rint(z * 1000.0)}[kind].astype(np.float32)


@pytest.mark.parametrize("kind", ["metres", "fractional", "millimetres"])
@pytest.mark.parametrize("shape", COUNTS, ids=str)
def test_the_model_is_numpy_bit_for_bit(shape, kind):
    a = np.atleast_1d(terrain(shape, kind, seed=np.prod(shape) % 1000))
    mean, std = hlp.numpy_order_moments(a)
    assert mean.dtype == np.float32 and std.dtype == np.float32
    assert same_bits(mean, a.mean()) and same_bits(std, a.std()), (mean, a.mean(), std, a.std())


def test_a_flat_pairwise_sum_is_not_numpy_beyond_two_chunks():
    """Why the chunks matter: one pairwise tree over the whole array (a chunk as long as the array) is another number."""
    differ = 0
    for seed in range(8):
        a = terrain(16385 + 8192 * seed, "fractional", seed)
        differ += not same_bits(hlp.numpy_order_sum(a, 1 << 20), a.sum())
        assert same_bits(hlp.numpy_order_sum(a, 8192), a.sum())
    assert differ > 0


def test_non_finite_samples_and_constants():
    with np.errstate(all="ignore"):
        a = terrain((129, 127), "fractional", 3)
        a[7, 11] = np.nan
        mean, std = hlp.numpy_order_moments(a)
        assert np.isnan(mean) and np.isnan(std)
        a[7, 11] = np.inf
        mean, std = hlp.numpy_order_moments(a)
        assert same_bits(mean, a.mean()) and mean == np.inf and np.isnan(std)
    c = np.full((300, 1003), 1234.5678, dtype=np.float32)
    mean, std = hlp.numpy_order_moments(c)
    assert same_bits(mean, c.mean()) and same_bits(std, c.std())


def test_other_buffer_sizes_follow_the_same_model():
    old = np.getbufsize()
    try:
        for size in (128, 1024, 16384):
            np.setbufsize(size)
            a = terrain((300, 1003), "fractional", size)
            mean, std = hlp.numpy_order_moments(a)
            assert same_bits(mean, a.mean()) and same_bits(std, a.std()), size
            assert hlp.moments_chunk() == size
        np.setbufsize(8000)  # no power of two: the pairwise tree of a chunk is not the kernel's
        assert hlp.moments_chunk() is None
    finally:
        np.setbufsize(old)


def test_moments_chunk_reads_the_environment_at_every_call(monkeypatch):
    monkeypatch.delenv("TOPO_AMD_VALLEY_HOST_MOMENTS", raising=False)
    assert hlp.moments_chunk() == np.getbufsize() == 8192
    monkeypatch.setenv("TOPO_AMD_VALLEY_HOST_MOMENTS", "1")
    assert hlp.moments_chunk() is None
    monkeypatch.setenv("TOPO_AMD_VALLEY_HOST_MOMENTS", "0")
    assert hlp.moments_chunk() == 8192


def test_a_numpy_that_sums_otherwise_sends_the_moments_to_the_host(monkeypatch):
    monkeypatch.delenv("TOPO_AMD_VALLEY_HOST_MOMENTS", raising=False)
    monkeypatch.setattr(hlp, "_moments_checked", {})
    monkeypatch.setattr(hlp, "_pairwise_rows", lambda blocks: np.add.accumulate(blocks, axis=1, dtype=np.float32)[:, -1])
    assert hlp.moments_chunk() is None


def test_the_new_entry_points_are_bound():
    for name, n_args in (("topo_amd_mean_std_f32_dev", 5), ("topo_amd_valley_ridge_std_dev", 12), ("topo_amd_valley_ridge_std_raw", 13),
                         ("topo_amd_valley_ridge_packed", 13), ("topo_amd_valley_moments_route", 1)):
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
