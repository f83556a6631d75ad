"""The map stream's own kernels give the tables of the paths they replace, element for element.

MAP_PERMUTE_LDS (k_permute_map3_lds: the row permutation of a 3^3 view with its gathers taken from LDS, against k_permute_map3) and
MAP_OWN_SORTS (k_child_hist / k_child_prefix / k_child_scatter: the grouped fine view of a 2^3 stride-2 map as a stable 8-way
partition, against rocPRIM's radix sort on the child index): every case builds the same maps with the knobs at 1 and at 0 in this
process and compares nbr, out_row and mask64 of both views exactly (lgs_debug_kmap_tables), as tests/test_gpu_map_build.py does
for the two knobs before them.  tile_k of the grouped view is not among those tables: it is held through a dgrad on the view, bit
for bit.  The maps of the two-scene batch are also held to oracle.kernel_map as sets of coordinate triples, and a bf16 training
step is bitwise the same run twice with the knobs on and once with them off."""
import gc

import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
from languagegroundedsemseg_amd import engine
from test_gpu_map_build import _build, _same, _slab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ON = dict(MAP_PERMUTE_LDS=1, MAP_OWN_SORTS=1)
OFF = dict(MAP_PERMUTE_LDS=0, MAP_OWN_SORTS=0)
LDS16, LDS32, PLAIN = "k_permute_map3_lds<16>", "k_permute_map3_lds<32>", "k_permute_map3"
OWN = ("k_child_hist", "k_child_prefix", "k_child_scatter")
RADIX = ("k_child_keys", "k_group_offsets", "k_build_map2_fine")


def _two_scenes():
    """about 40 k distinct voxels of two scenes around the origin (negative coordinates on every axis), 600 rows repeated"""
    c = _slab(41, 40000, 64, thick=4, batches=2)
    return np.concatenate([c, c[:600]])


@pytest.fixture(scope="module")
def scenes():
    return _two_scenes()


def _sorted_triples(k, ci, co):
    t = np.concatenate([np.asarray(k, np.int64)[:, None], ci.astype(np.int64), co.astype(np.int64)], 1)
    return t[np.lexsort(t.T[::-1])]


def _oracle_same(built, ks, ts):
    from oracle import oracle as orc
    _, _, ci, co, (hk, hi, ho) = built
    k, i, o = orc.kernel_map(ci, co, ks, ts)
    assert hk.shape[0] == k.shape[0] and k.shape[0] > co.shape[0]
    assert np.array_equal(_sorted_triples(hk, ci[hi], co[ho]), _sorted_triples(k, ci[i], co[o]))


# ---- MAP_PERMUTE_LDS
@pytest.mark.parametrize("n", [700, 16385])     # one partial window, no multiple of 256; a second window of one row
def test_lds_permute_equals_the_global_gathers(n):
    coords = _slab(50 + n, n, 40)
    engine.dispatch_counts(reset=True)
    a = _build(coords, **ON)
    d = engine.dispatch_counts(reset=True)
    assert d.get(LDS16, 0) == 1 and PLAIN not in d, d
    b = _build(coords, **OFF)
    d = engine.dispatch_counts(reset=True)
    assert d.get(PLAIN, 0) == 1 and LDS16 not in d, d
    assert a[0][0].shape == (27, (n + 255) // 256 * 256)
    _same(a, b)


@pytest.mark.parametrize("group", [1, 2, 5, 27, 28])   # offsets per workgroup: 27 groups; 14 with a short last one; 6; one; 27 x 3 windows / 28 = 2
def test_lds_permute_offset_groups(group):
    coords = _slab(57, 3000, 30)
    _same(_build(coords, MAP_PERMUTE_GROUP=group, MASK_WINDOW=1024, **ON), _build(coords, MASK_WINDOW=1024, **OFF))


def test_lds_permute_two_scenes_and_the_oracle(scenes):
    a, b = _build(scenes, **ON), _build(scenes, **OFF)           # level 0: rows in the caller's order (`order` is staged too)
    assert a[0][0].shape[1] > 2 * 16384                          # three windows
    _same(a, b)
    _oracle_same(a, 3, 1)
    # the strided 3^3 map: a coarse-stationary view without `order` and a fine-stationary one, both through the permutation
    a, b = _build(scenes, 0, 3, True, **ON), _build(scenes, 0, 3, True, **OFF)
    _same(a, b)
    _oracle_same(a, 3, 1)


@pytest.mark.parametrize("window,site", [(1024, LDS16), (32768, LDS32), (65536, PLAIN), (3000, PLAIN)])
def test_lds_permute_windows(scenes, window, site):
    """a window whose row segment does not fit the LDS, or that is no multiple of 256, takes k_permute_map3 with the knob at 1"""
    coords = scenes if window >= 32768 else _slab(5, 2000, 14)
    engine.dispatch_counts(reset=True)
    a = _build(coords, MASK_WINDOW=window, **ON)
    d = engine.dispatch_counts(reset=True)
    assert [s for s in (LDS16, LDS32, PLAIN) if s in d] == [site] and d[site] == 1, d
    b = _build(coords, MASK_WINDOW=window, **OFF)
    d = engine.dispatch_counts(reset=True)
    assert [s for s in (LDS16, LDS32, PLAIN) if s in d] == [PLAIN], d
    _same(a, b)


# ---- MAP_OWN_SORTS
def _dgrad_2x2x2(coords, level, **knobs):
    """the gradient a 2^3 stride-2 convolution hands to its input rows: reads the grouped fine view, tile_k included"""
    with engine.tuning(**knobs):
        c = torch.from_numpy(np.ascontiguousarray(coords)).to(DEV)
        x = ME.SparseTensor(torch.zeros(c.shape[0], 1, device=DEV), c)
        mgr, key = x.coordinate_manager, x.coordinate_map_key
        for _ in range(level):
            key = mgr.stride(key, 2)
        out_key = mgr.stride(key, 2)
        km = mgr.kernel_map_handle(key, out_key, 2)
        gen = torch.Generator(device="cpu").manual_seed(7)
        g = torch.randn(mgr.get_coordinates(out_key).shape[0], 32, generator=gen).to(DEV).bfloat16()
        w = (torch.randn(8, 32, 32, generator=gen) * 0.1).to(DEV)
        return km.conv_dgrad(g, w, False).float().cpu().numpy()


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_child_partition_equals_the_radix_sort(scenes, level):
    engine.dispatch_counts(reset=True)
    a = _build(scenes, level, 2, True, **ON)
    d = engine.dispatch_counts(reset=True)
    assert all(d.get(s, 0) == 1 for s in OWN) and not any(s in d for s in RADIX), d
    b = _build(scenes, level, 2, True, **OFF)
    d = engine.dispatch_counts(reset=True)
    assert all(d.get(s, 0) == 1 for s in RADIX) and not any(s in d for s in OWN), d
    _same(a, b)
    _oracle_same(a, 2, 1 << level)
    assert np.array_equal(_dgrad_2x2x2(scenes, level, **ON), _dgrad_2x2x2(scenes, level, **OFF))


@pytest.mark.parametrize("n,rounds", [(1, 0), (700, 0), (700, 16), (4097, 16), (4097, 3), (4097, 1)])
def test_child_partition_small_maps(n, rounds):
    """one row; one partial round; a chunk that ends early; one row past a chunk of 16 rounds; six chunks of 3 rounds, the last
    short; 17 chunks of one round"""
    coords = _slab(60 + n, n, 40)
    _same(_build(coords, 0, 2, True, MAP_CHILD_ROUNDS=rounds, **ON), _build(coords, 0, 2, True, **OFF))
    assert np.array_equal(_dgrad_2x2x2(coords, 0, MAP_CHILD_ROUNDS=rounds, **ON), _dgrad_2x2x2(coords, 0, **OFF))


@pytest.mark.parametrize("rounds", [2, 16])     # 157 blocks of 256 positions at level 0: 79 chunks, 10 chunks
def test_child_partition_rounds_two_scenes(scenes, rounds):
    _same(_build(scenes, 0, 2, True, MAP_CHILD_ROUNDS=rounds, **ON), _build(scenes, 0, 2, True, **OFF))
    assert np.array_equal(_dgrad_2x2x2(scenes, 0, MAP_CHILD_ROUNDS=rounds, **ON), _dgrad_2x2x2(scenes, 0, **OFF))


# ---- both
def test_empty_batch():
    coords = np.zeros((0, 4), np.int32)
    for strided, ks in ((False, 3), (True, 3), (True, 2)):
        a, b = _build(coords, 0, ks, strided, **ON), _build(coords, 0, ks, strided, **OFF)
        _same(a, b)
        assert a[4][0].shape[0] == 0


def test_the_knobs_are_in_the_tuning_table():
    rows = {name: default for name, default, _, _ in engine.tuning_table()}
    assert rows["MAP_PERMUTE_LDS"] == 1 and rows["MAP_OWN_SORTS"] == 1
    assert rows["MAP_PERMUTE_GROUP"] == 0 and rows["MAP_CHILD_ROUNDS"] == 0      # both automatic


def test_bf16_training_step_is_bitwise_the_same_with_the_knobs_on_and_off():
    from languagegroundedsemseg_amd.synthetic import make_batch
    from test_gpu_model import run_model
    coords, feats, _ = make_batch([1, 2], voxel=0.02, n_target=60000)
    labels = np.random.default_rng(0).integers(-1, 20, coords.shape[0]).astype(np.int64)
    runs = []
    for knobs in (ON, ON, OFF):
        with engine.tuning(**knobs):
            logits, loss, grads, _ = run_model("Res16UNet14A", coords, feats, labels, DEV, dtype=torch.bfloat16)
        runs.append((logits, loss, grads))
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and runs[0][1] == other[1]
        for k in runs[0][2]:
            assert np.array_equal(runs[0][2][k], other[2][k]), k
    del runs
    gc.collect()          # three dropped models with their managers and packed weight images: not left for a later test's collector
