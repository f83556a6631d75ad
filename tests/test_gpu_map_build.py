"""The two build paths of the 3^3 kernel maps give the same tables, element for element.

MAP_WINDOW_SORT (k_window_sort, one workgroup per mask window, against the radix sort of (window, code) keys) and MAP_BLOCK_DIR
(the 4 x 4 x 4 block directory against the per-voxel hash): every case builds the same maps with the knob at 1 and at 0 in this
process and compares nbr, out_row and mask64 of both views exactly (lgs_debug_kmap_tables) -- the row order inside a window
decides the summation order of the BatchNorm and weight-gradient partials, so equality as sets is not enough.  The directory cases
are also held to oracle.kernel_map as sets of coordinate triples."""
import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
from languagegroundedsemseg_amd import engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slab(seed, n, extent, thick=4, batches=2):
    """exactly n distinct voxels of a noisy slab [-extent, extent)^2 x [-thick/2, thick/2) per batch index, rows in random order"""
    rng = np.random.default_rng(seed)
    cells = batches * (2 * extent) ** 2 * thick
    assert n <= cells
    idx = rng.choice(cells, n, replace=False)
    b, r = idx // ((2 * extent) ** 2 * thick), idx % ((2 * extent) ** 2 * thick)
    x, y, z = r % (2 * extent) - extent, r // (2 * extent) % (2 * extent) - extent, r // (2 * extent) ** 2 - thick // 2
    return np.stack([b, x, y, z], 1).astype(np.int32)


def _build(coords, level=0, ks=3, strided=False, dilation=1, **knobs):
    """-> (tables of the forward view, tables of the dgrad view, coords in, coords out, exported triples) of one map built under `knobs`"""
    with engine.tuning(**knobs):
        c = torch.from_numpy(np.ascontiguousarray(coords)).to(DEV)
        x = ME.SparseTensor(torch.zeros(c.shape[0], 1, device=DEV), c)
        mgr, key = x.coordinate_manager, x.coordinate_map_key
        for _ in range(level):
            key = mgr.stride(key, 2)
        out_key = mgr.stride(key, 2) if strided else key
        km = mgr.kernel_map_handle(key, out_key, ks, dilation)
        views = [tuple(None if t is None else t.cpu().numpy() for t in km.tables(bwd)) for bwd in (False, True)]
        ci, co = mgr.get_coordinates(key).cpu().numpy(), mgr.get_coordinates(out_key).cpu().numpy()
        trip = tuple(t.cpu().numpy() for t in km.export())
        assert mgr._m.check() == 0
    return views[0], views[1], ci, co, trip


def _same(a, b):
    for va, vb in zip(a[:2], b[:2]):                 # forward view, dgrad view
        for name, ta, tb in zip(("nbr", "out_row", "mask64"), va, vb):
            assert (ta is None) == (tb is None), name
            if ta is not None:
                assert ta.shape == tb.shape, (name, ta.shape, tb.shape)
                assert np.array_equal(ta, tb), "%s differs at %d of %d entries" % (name, int((ta != tb).sum()), ta.size)


# ---- MAP_WINDOW_SORT
@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 700, 1025, 3000])    # one row; below one window; one row past a window; rows + padding in the last of three
def test_window_sort_equals_the_radix_sort(n, order):
    coords = _slab(10 + n, n, 14)
    a = _build(coords, MASK_WINDOW=1024, MASK_ORDER=order, MAP_WINDOW_SORT=1)
    b = _build(coords, MASK_WINDOW=1024, MASK_ORDER=order, MAP_WINDOW_SORT=0)
    assert a[0][0].shape[1] == (n + 255) // 256 * 256
    _same(a, b)


def test_window_sort_default_window_two_windows():
    coords = _slab(3, 16390, 40)                       # 16 384 + 6 rows: a full window and a nearly empty one
    assert engine.tuning_get("MASK_WINDOW") == 16384
    _same(_build(coords, MAP_WINDOW_SORT=1), _build(coords, MAP_WINDOW_SORT=0))


def test_window_sort_empty_map():
    coords = np.zeros((0, 4), np.int32)
    a, b = _build(coords, MAP_WINDOW_SORT=1), _build(coords, MAP_WINDOW_SORT=0)
    _same(a, b)
    assert a[4][0].shape[0] == 0


@pytest.mark.parametrize("window,lds", [(16384, True), (1024, True), (65536, False), (32768, False), (3000, False)])
def test_window_sort_refuses_what_the_lds_cannot_hold(window, lds):
    """a window above the LDS budget, or one that is no power of two, takes the radix sort with the knob at 1: dispatch counters"""
    coords = _slab(5, 2000, 14)
    engine.dispatch_counts(reset=True)
    a = _build(coords, MASK_WINDOW=window, MAP_WINDOW_SORT=1)
    d = engine.dispatch_counts(reset=True)
    assert (d.get("k_window_sort", 0) == 1) == lds and (d.get("k_mask_sort_keys", 0) == 1) == (not lds), d
    b = _build(coords, MASK_WINDOW=window, MAP_WINDOW_SORT=0)
    d = engine.dispatch_counts(reset=True)
    assert "k_window_sort" not in d and d.get("k_mask_sort_keys", 0) == 1, d
    _same(a, b)


# ---- MAP_BLOCK_DIR
def _full_and_single():
    """two blocks with all 64 cells (one on the negative side), one block with a single voxel, a block split by every block face"""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([g, g - 4 + np.array([0, 0, -8]), np.array([[9, 9, 9]]), g + np.array([18, 2, -2])])
    c = np.concatenate([np.zeros((pts.shape[0], 1), np.int64), pts], 1).astype(np.int32)
    return c[np.random.default_rng(0).permutation(c.shape[0])]


def _shared_batches():
    """cells straddling zero on every axis; batch 1 repeats batch 0's coordinates and adds some of its own"""
    a = _slab(21, 500, 6, thick=12, batches=1)
    b = np.concatenate([a[:300], _slab(22, 200, 6, thick=12, batches=1)])
    b = np.unique(b, axis=0)
    b[:, 0] = 1
    return np.concatenate([a, b])


def _isolated(n=3000):
    """voxels five cells apart: every voxel a block of its own, so the directory holds n entries at a load near 0.4 and collides"""
    rng = np.random.default_rng(7)
    idx = rng.choice(30 ** 3, n, replace=False)
    p = np.stack([idx % 30, idx // 30 % 30, idx // 900], 1) * 5 - 70
    return np.concatenate([np.zeros((n, 1), np.int64), p], 1).astype(np.int32)


DIR_SCENES = {"full+single": _full_and_single, "shared batches": _shared_batches, "isolated": _isolated, "slab": lambda: _slab(31, 3000, 30),
              "one row": lambda: np.array([[0, -1, 0, 5]], np.int32)}
# case -> (scene, level, kernel size, strided, dilation)
DIR_CASES = {
    "stride 1, full and single blocks": ("full+single", 0, 3, False, 1),
    "stride 1, two batches sharing coordinates": ("shared batches", 0, 3, False, 1),
    "stride 1, collisions": ("isolated", 0, 3, False, 1),
    "stride 1, n = 1": ("one row", 0, 3, False, 1),
    "tensor stride 1": ("slab", 0, 3, False, 1),
    "tensor stride 2": ("slab", 1, 3, False, 1),
    "tensor stride 4": ("slab", 2, 3, False, 1),
    "tensor stride 8": ("slab", 3, 3, False, 1),
    "dilation 2": ("shared batches", 0, 3, False, 2),
    "dilation 2 at tensor stride 2": ("slab", 1, 3, False, 2),
    "3^3 stride 2": ("slab", 0, 3, True, 1),
    "3^3 stride 2 at tensor stride 2": ("slab", 1, 3, True, 1),
    "3^3 stride 2, full and single blocks": ("full+single", 0, 3, True, 1),
}


def _triples(k, ci, co):
    return set(map(tuple, np.concatenate([np.asarray(k, np.int64)[:, None], ci, co], 1).tolist()))


@pytest.mark.parametrize("case", list(DIR_CASES))
def test_block_directory_equals_the_hash(case):
    scene, level, ks, strided, dil = DIR_CASES[case]
    coords = DIR_SCENES[scene]()
    a = _build(coords, level, ks, strided, dil, MAP_BLOCK_DIR=1)
    b = _build(coords, level, ks, strided, dil, MAP_BLOCK_DIR=0)
    _same(a, b)
    # and the map itself against the oracle, as a set of coordinate triples
    from oracle import oracle as orc
    _, _, ci, co, (hk, hi, ho) = a
    k, i, o = orc.kernel_map(ci, co, ks, (1 << level) * dil)
    assert hk.shape[0] == k.shape[0] and _triples(hk, ci[hi], co[ho]) == _triples(k, ci[i], co[o])
    if scene != "isolated":
        assert k.shape[0] > ci.shape[0] or ci.shape[0] == 1      # neighbours were found, not only the centres


def test_block_directory_builds_only_the_table_it_uses():
    coords = _slab(31, 3000, 30)
    for knob, mine, other in ((1, "k_dir_build", "k_hash_insert"), (0, "k_hash_insert", "k_dir_build")):
        engine.dispatch_counts(reset=True)
        _build(coords, 0, 3, True, 1, MAP_BLOCK_DIR=knob)
        d = engine.dispatch_counts(reset=True)
        assert d.get(mine, 0) == 2 and other not in d, d           # the fine and the coarse map's table, once each


def test_block_directory_empty_map():
    coords = np.zeros((0, 4), np.int32)
    _same(_build(coords, MAP_BLOCK_DIR=1), _build(coords, MAP_BLOCK_DIR=0))
    _same(_build(coords, 0, 3, True, 1, MAP_BLOCK_DIR=1), _build(coords, 0, 3, True, 1, MAP_BLOCK_DIR=0))
