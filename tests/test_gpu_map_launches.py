"""The coordinate manager issues the same launches as before its host layer was restructured.

One manager walks every construction the manager has (insert, four stride-2 steps, every kernel-map relation, the origin map and two
segment maps) over a three-window scene, and the launch counters must equal a literal table: one for the default knobs and one for the
older build paths (MAP_WINDOW_SORT = MAP_BLOCK_DIR = MAP_PERMUTE_LDS = MAP_OWN_SORTS = 0).  Both tables were recorded by this same
body on the commit BEFORE the restructuring (profiles/manager_host_layer.txt), not taken from the code under test."""
import pytest
import torch

import MinkowskiEngine as ME
from languagegroundedsemseg_amd import engine
from test_gpu_map_build import _slab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OLD_PATHS = dict(MAP_WINDOW_SORT=0, MAP_BLOCK_DIR=0, MAP_PERMUTE_LDS=0, MAP_OWN_SORTS=0)

_COMMON = {
    "k_pack_keys": 1, "k_heads": 7, "k_mark_first": 1, "k_count_levels": 1, "k_emit_unique": 1, "k_emit_sorted": 1, "k_emit_inverse": 1,
    "k_emit_coarse": 4, "k_fill_segs": 5, "k_fill_i32": 1,
    "k_build_map2_coarse": 4, "k_build_map1_coarse": 1, "k_build_map1_fine": 1,
    "k_origin_coords": 1, "k_origin_segments": 1, "k_row_seg": 1, "k_compose_coarse_of": 1, "k_compose_seg_start": 1,
    "k_item_counts": 1, "k_item_fill": 1,
}
LAUNCHES_DEFAULT = dict(_COMMON, **{
    "k_dir_fill": 5, "k_dir_build": 5, "k_build_map3<DirRef>": 7, "k_build_map3_fine<DirRef>": 1,
    "k_window_sort": 8, "k_permute_map3_lds<16>": 8,
    "k_child_hist": 4, "k_child_prefix": 4, "k_child_scatter": 4,
})
LAUNCHES_OLD_PATHS = dict(_COMMON, **{
    "k_hash_fill": 5, "k_hash_insert": 5, "k_build_map3<HashRef>": 7, "k_build_map3_fine<HashRef>": 1,
    "k_mask_sort_keys": 8, "k_permute_map3": 8,
    "k_child_keys": 4, "k_group_offsets": 4, "k_build_map2_fine": 4,
})
assert sum(LAUNCHES_DEFAULT.values()) == 82 and sum(LAUNCHES_OLD_PATHS.values()) == 82


def run_manager(**knobs):
    """-> (launch counters, d_err flags) of one manager that builds everything once under `knobs` (+ MASK_WINDOW = 1024: three windows)"""
    coords = torch.from_numpy(_slab(31, 3000, 30)).to(DEV)
    feats = torch.zeros(coords.shape[0], 1, device=DEV)
    with engine.tuning(MASK_WINDOW=1024, **knobs):
        torch.cuda.synchronize()
        engine.dispatch_counts(reset=True)
        x = ME.SparseTensor(feats, coords)                                   # 1. the insert
        mgr = x.coordinate_manager
        keys = [x.coordinate_map_key]
        for _ in range(4):                                                   # 2. four stride-2 steps
            keys.append(mgr.stride(keys[-1], 2))
        for k in keys:                                                       # 3. the 3^3 map at every level
            mgr.kernel_map_handle(k, k, 3)
        for fine, coarse in zip(keys[:-1], keys[1:]):                        # 4. the 2^3 stride-2 map between consecutive levels
            mgr.kernel_map_handle(fine, coarse, 2)
        mgr.kernel_map_handle(keys[0], keys[1], 3)                           # 5. one 3^3 and one 1x1 stride-2 map
        mgr.kernel_map_handle(keys[0], keys[1], 1)
        mgr.kernel_map_handle(keys[0], keys[0], 3, 2)                        # 6. one dilated 3^3 map
        origin = mgr.origin_key()                                            # 7. the origin map
        mgr.segment_map_handle(keys[0], origin)                              # 8. level 0 -> origin, level 0 -> stride 4
        mgr.segment_map_handle(keys[0], keys[2])
        flags = mgr._m.check()
        counts = engine.dispatch_counts()     # not reset: conftest's dispatch recorder reads them after the test
    return counts, flags


@pytest.mark.parametrize("knobs,expected", [({}, LAUNCHES_DEFAULT), (OLD_PATHS, LAUNCHES_OLD_PATHS)], ids=["default", "old paths"])
def test_manager_launch_table(knobs, expected):
    counts, flags = run_manager(**knobs)
    assert flags == 0
    assert counts == expected, {k: (counts.get(k), expected.get(k)) for k in set(counts) | set(expected) if counts.get(k) != expected.get(k)}
