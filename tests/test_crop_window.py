"""``helpers.crop_window``: what ``Dataset.sel(crop)`` selects, restated on plain coordinates (no xarray, no GPU)."""
import numpy as np
import pytest

from topo_descriptors_amd import helpers as hlp


class FakeVar:
    def __init__(self, values, dims):
        self.values, self.dims = values, dims


class FakeDataset:
    def __init__(self, x, y, shape=None):
        dem = np.zeros((len(y), len(x)) if shape is None else shape, dtype=np.float32)
        self._v = {"dem": FakeVar(dem, ("y", "x")), "x": FakeVar(np.asarray(x), ("x",)), "y": FakeVar(np.asarray(y), ("y",))}
        self.attrs = {"crs": "epsg:2056"}

    def __getitem__(self, k):
        return self._v[k]

    def __iter__(self):
        return iter(["dem"])


X = [10.0, 20.0, 30.0, 40.0, 50.0, 60.0]  # increasing
Y = [500.0, 400.0, 300.0, 200.0, 100.0]   # decreasing (north to south)
DS = FakeDataset(X, Y)


@pytest.mark.parametrize("bounds, want", [
    (slice(20.0, 40.0), (1, 3)),     # on labels: both ends inclusive
    (slice(15.0, 45.0), (1, 3)),     # between labels
    (slice(20.0, 20.0), (1, 1)),     # one label
    (slice(21.0, 29.0), (2, 0)),     # between two neighbours: nothing
    (slice(-5.0, 35.0), (0, 3)),     # start outside the index
    (slice(35.0, 1000.0), (3, 3)),   # stop outside
    (slice(-5.0, 1000.0), (0, 6)),   # both outside
    (slice(70.0, 90.0), (6, 0)),     # beyond the end
    (slice(-9.0, -1.0), (0, 0)),     # before the start
    (slice(None, 30.0), (0, 3)),
    (slice(30.0, None), (2, 4)),
    (slice(None, None), (0, 6)),
    (slice(40.0, 20.0), (3, 0)),     # the wrong direction: empty
    (slice(60.0, 10.0), (5, 0)),
])
def test_increasing_coordinate(bounds, want):
    row0, rows, col0, cols = hlp.crop_window(DS, {"x": bounds})
    assert (row0, rows) == (0, 5)  # a missing key: the whole axis
    assert cols == want[1]
    if cols:  # (where an empty selection starts is not specified: the table's start is not compared for those)
        assert col0 == want[0]
        assert X[col0:col0 + cols] == [v for v in X if (bounds.start is None or v >= bounds.start)
                                       and (bounds.stop is None or v <= bounds.stop)]


@pytest.mark.parametrize("bounds, want", [
    (slice(400.0, 200.0), (1, 3)),   # on labels
    (slice(450.0, 150.0), (1, 3)),   # between labels
    (slice(300.0, 300.0), (2, 1)),
    (slice(390.0, 310.0), (2, 0)),
    (slice(9000.0, 250.0), (0, 3)),  # start outside
    (slice(250.0, -9000.0), (3, 2)), # stop outside
    (slice(9000.0, -9000.0), (0, 5)),
    (slice(50.0, 10.0), (5, 0)),
    (slice(None, 300.0), (0, 3)),
    (slice(300.0, None), (2, 3)),
    (slice(200.0, 400.0), (3, 0)),   # the classic: a south-to-north slice on a north-to-south y selects nothing
    (slice(-160000, 480000), (5, 0)),
])
def test_decreasing_coordinate(bounds, want):
    row0, rows, col0, cols = hlp.crop_window(DS, {"y": bounds})
    assert (col0, cols) == (0, 6)
    assert rows == want[1]
    if rows:  # (as above)
        assert row0 == want[0]
        assert Y[row0:row0 + rows] == [v for v in Y if (bounds.start is None or v <= bounds.start)
                                       and (bounds.stop is None or v >= bounds.stop)]


def test_both_axes_none_and_a_one_element_axis():
    assert hlp.crop_window(DS, None) == (0, 5, 0, 6)
    assert hlp.crop_window(DS, {}) == (0, 5, 0, 6)
    assert hlp.crop_window(DS, {"x": slice(25, 55), "y": slice(450, 150)}) == (1, 3, 2, 3)
    one = FakeDataset([7.0], [3.0, 2.0])
    assert hlp.crop_window(one, {"x": slice(0.0, 10.0)}) == (0, 2, 0, 1)
    assert hlp.crop_window(one, {"x": slice(7.0, 7.0)}) == (0, 2, 0, 1)
    assert hlp.crop_window(one, {"x": slice(8.0, 9.0)})[3] == 0
    assert hlp.crop_window(one, {"x": slice(10.0, 0.0)})[3] == 0
    assert hlp.crop_window(one, {"x": slice(None, None), "y": slice(2.5, None)}) == (1, 1, 0, 1)  # (labels <= 2.5)
    assert hlp.crop_window(one, {"y": slice(None, 2.5)}) == (0, 1, 0, 1)
    assert all(type(v) is int for v in hlp.crop_window(DS, {"x": slice(25, 55)}))


def test_refusals():
    with pytest.raises(KeyError):
        hlp.crop_window(DS, {"z": slice(0, 1)})
    with pytest.raises(KeyError):
        hlp.crop_window(DS, {"x": slice(0, 100), "time": slice(0, 1)})
    with pytest.raises(NotImplementedError, match="slice"):
        hlp.crop_window(DS, {"x": 30.0})
    with pytest.raises(NotImplementedError, match="slice"):
        hlp.crop_window(DS, {"y": [400.0, 300.0]})
    with pytest.raises(NotImplementedError, match="step"):
        hlp.crop_window(DS, {"x": slice(10.0, 50.0, 2)})
    with pytest.raises(ValueError, match="monotonic"):
        hlp.crop_window(FakeDataset([1.0, 2.0, 2.0, 3.0], Y), {"x": slice(0, 9)})
    with pytest.raises(ValueError, match="monotonic"):
        hlp.crop_window(FakeDataset(X, [5.0, 4.0, 6.0, 3.0, 2.0]), None)
    with pytest.raises(ValueError, match="monotonic"):
        hlp.crop_window(FakeDataset([1.0, np.nan, 3.0], Y), None)
    with pytest.raises(ValueError, match="coordinates"):
        hlp.crop_window(FakeDataset(X, Y, shape=(5, 7)), {"x": slice(0, 9)})
    with pytest.raises(ValueError, match="coordinates"):
        hlp.crop_window(FakeDataset(X, Y, shape=(4, 6)), None)


def test_random_cases_equal_pandas_slice_indexer():
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(20251)
    checked = empty = 0
    for case in range(4000):
        n = int(rng.integers(1, 40))
        if case % 2:
            coords = np.cumsum(rng.integers(1, 6, size=n)).astype(np.float64) * 25.0 - 300.0
        else:
            coords = np.sort(rng.uniform(-1000.0, 1000.0, size=n))
            if np.unique(coords).size != n:
                continue
        if case % 4 >= 2:
            coords = coords[::-1].copy()

        def bound():
            kind = rng.integers(0, 5)
            if kind == 0:
                return None
            if kind == 1:
                return float(coords[rng.integers(0, n)])                    # a label
            if kind == 2:
                return float(rng.uniform(coords.min() - 50.0, coords.max() + 50.0))  # anywhere, mostly between labels
            if kind == 3:
                return float(coords.max() + rng.uniform(1.0, 500.0))        # outside, above
            return float(coords.min() - rng.uniform(1.0, 500.0))            # outside, below

        start, stop = bound(), bound()
        want = pd.Index(coords).slice_indexer(start, stop)
        first, count, _ = want.indices(n)[0], len(range(*want.indices(n))), None
        ds = FakeDataset(coords, [1.0, 0.0])
        _, _, col0, cols = hlp.crop_window(ds, {"x": slice(start, stop)})
        assert cols == count, (coords, start, stop, want)
        if count:
            assert col0 == first, (coords, start, stop, want)
        else:
            empty += 1
        ds = FakeDataset([0.0, 1.0], coords)
        row0, rows, _, _ = hlp.crop_window(ds, {"y": slice(start, stop)})
        assert (rows, row0 if count else None) == (count, first if count else None), (coords, start, stop, want)
        checked += 1
    assert checked > 3000 and 100 < empty < checked - 1000
