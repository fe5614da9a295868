"""The table of declared raster classes (include/topo_amd.h, "what kernel routing may know about a raster") without a GPU.

An application that holds one raster as overlapping row blocks of one buffer (each block with its ghost rows) declares
the class once per block.  Every block must then find it, in whatever order the blocks were declared; a declaration of
another class or for a raster of another shape replaces what it overlaps; a withdrawal drops exactly the declarations
that overlap the withdrawn rows; declaring the same blocks again and again does not fill the table.  raster_class_set /
_from_scan / _get only touch the host table, so the addresses here are plain integers that are never dereferenced
(tests/test_gpu_block_views.py runs the descriptors on such blocks)."""
import ctypes as C
import random

import pytest

from topo_descriptors_amd import _lib, shard

GNY, NX = 400, 1000
ROW = NX * 4                      # bytes per row of a float32 raster
BASE = 0x7F3A_0000_0000           # the raster's first row
ELSEWHERE = 0x7F5C_0000_0000      # another allocation, far away
CLS = (0, 0.0, 3.5, 0.5)          # (large, lo, hi, frac_share)
OTHER = (0, -2.0, 900.0, 0.25)
ORDINARY = (0, 0.0, 4096.0, 0.0)  # what a block nothing is declared for is taken for


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("topo_amd_raster_class_set", "topo_amd_raster_class_from_scan", "topo_amd_raster_class_get"):
        restype, argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = restype
        getattr(lib, name).argtypes = argtypes
    return lib


@pytest.fixture(autouse=True)
def empty_table(lib):
    assert lib.topo_amd_raster_class_set(None, 0, 0, 0, -1, 0.0, 0.0, 0.0) == 0
    yield
    assert lib.topo_amd_raster_class_set(None, 0, 0, 0, -1, 0.0, 0.0, 0.0) == 0


def views(nblocks, halo=(33, 33), gny=GNY):
    """(first row, rows) in the buffer of each block: the rows it owns plus its ghost rows, clipped to the raster."""
    out = []
    for row0, rows in shard.split_rows(gny, nblocks):
        lo, hi = max(0, row0 - halo[0]), min(gny, row0 + rows + halo[1])
        out.append((lo, hi - lo))
    return out


def declare(lib, view, cls=CLS, gny=GNY, nx=NX, base=BASE):
    first, rows = view
    large, lo, hi, share = cls
    assert lib.topo_amd_raster_class_set(base + first * nx * 4, rows, gny, nx, large, lo, hi, share) == 0


def withdraw(lib, first, rows, base=BASE):
    assert lib.topo_amd_raster_class_set(base + first * ROW, rows, GNY, NX, -1, 0.0, 0.0, 0.0) == 0


def get(lib, row, gny=GNY, nx=NX, base=BASE):
    dec, large = C.c_int32(), C.c_int32()
    lo, hi, share = C.c_float(), C.c_float(), C.c_float()
    assert lib.topo_amd_raster_class_get(base + row * nx * 4, gny, nx, C.byref(dec), C.byref(large), C.byref(lo),
                                         C.byref(hi), C.byref(share)) == 0
    return dec.value, (large.value, lo.value, hi.value, share.value)


def probe_rows(view):
    first, rows = view
    return (first, first + rows // 2, first + rows - 1)


def assert_declared(lib, vs, cls=CLS):
    for k, v in enumerate(vs):
        for r in probe_rows(v):
            assert get(lib, r) == (1, cls), (k, v, r, get(lib, r))


ORDERS = {
    "forward": lambda n: list(range(n)),
    "reverse": lambda n: list(range(n))[::-1],
    "shuffled": lambda n: random.Random(n).sample(range(n), n),
}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("nblocks", [2, 3, 5])
def test_every_overlapping_view_keeps_the_class(lib, nblocks, order):
    vs = views(nblocks)
    assert all(a[0] + a[1] > b[0] for a, b in zip(vs, vs[1:]))  # (the views do overlap)
    for k in ORDERS[order](nblocks):
        declare(lib, vs[k])
    assert_declared(lib, vs)


def test_two_views_of_a_400_by_1000_raster(lib):
    """Rows [0, 250) and [150, 400) of a 400 x 1000 raster, either order."""
    for order in ((0, 1), (1, 0)):
        lib.topo_amd_raster_class_set(None, 0, 0, 0, -1, 0.0, 0.0, 0.0)
        vs = [(0, 250), (150, 250)]
        for k in order:
            declare(lib, vs[k])
        assert_declared(lib, vs)


def test_from_scan_declares_the_same_class_for_every_view(lib):
    counts = (C.c_uint64 * 3)(1000, 0, 500)
    rng = (C.c_float * 2)(0.0, 3.5)
    vs = views(5)
    for first, rows in vs:
        assert lib.topo_amd_raster_class_from_scan(BASE + first * ROW, rows, GNY, NX, counts, rng) == 0
    assert_declared(lib, vs, (0, 0.0, 3.5, 0.5))


@pytest.mark.parametrize("exact_range", [False, True])
def test_another_class_replaces_what_it_overlaps(lib, exact_range):
    vs = views(3)
    for v in vs:
        declare(lib, v)
    new = vs[1] if exact_range else (vs[1][0] + 10, vs[1][1] - 20)
    declare(lib, new, OTHER)
    # the middle view's neighbours overlap it: they are gone, and so are their rows outside the new declaration
    for r in (vs[0][0], vs[2][0] + vs[2][1] - 1):
        assert get(lib, r) == (0, ORDINARY), r
    for r in probe_rows(new):
        assert get(lib, r) == (1, OTHER), r


def test_a_raster_of_another_shape_replaces_what_it_overlaps(lib):
    vs = views(3)
    for v in vs:
        declare(lib, v)
    # the same class, declared over the middle view's memory for a 500 x 800 raster
    first, rows = vs[1]
    lo = BASE + first * ROW
    assert lib.topo_amd_raster_class_set(lo, rows * NX // 800, 500, 800, *CLS) == 0
    for v in vs:
        for r in probe_rows(v):
            assert get(lib, r)[0] == 0, (v, r)
    dec, cls = get(lib, 0, gny=500, nx=800, base=lo)
    assert (dec, cls) == (1, CLS)


def test_redeclaring_a_view_replaces_it(lib):
    vs = views(2)
    for v in vs:
        declare(lib, v)
    declare(lib, vs[0], OTHER)
    for r in probe_rows(vs[0]):
        assert get(lib, r) == (1, OTHER), r
    assert get(lib, GNY - 1) == (0, ORDINARY)  # (the other view overlapped it: gone)
    declare(lib, vs[0], CLS)
    declare(lib, vs[1], CLS)
    assert_declared(lib, vs)


def model_declared(declared, row):
    return any(f <= row < f + n for f, n in declared)


@pytest.mark.parametrize("rows", [(120, 4), (150, 60), (0, GNY)])
def test_a_withdrawal_drops_what_overlaps_it_and_nothing_else(lib, rows):
    vs = views(5)
    for v in vs:
        declare(lib, v)
    declare(lib, (0, 50), OTHER, gny=50, base=ELSEWHERE)
    w0, wn = rows
    withdraw(lib, w0, wn)
    kept = [v for v in vs if not (v[0] < w0 + wn and w0 < v[0] + v[1])]
    assert len(kept) < len(vs)
    for v in vs:
        for r in probe_rows(v) + tuple(range(w0, w0 + wn, 7)):
            want = (1, CLS) if model_declared(kept, r) else (0, ORDINARY)
            assert get(lib, r) == want, (v, r, rows)
    assert get(lib, 10, gny=50, base=ELSEWHERE) == (1, OTHER)


def test_redeclaring_views_does_not_fill_the_table(lib):
    declare(lib, (0, 50), OTHER, gny=50, base=ELSEWHERE)
    vs = views(5)
    for i in range(1000):
        for k in ORDERS["shuffled"](5) if i % 2 else range(5):
            declare(lib, vs[k])
    assert_declared(lib, vs)
    assert get(lib, 10, gny=50, base=ELSEWHERE) == (1, OTHER)
