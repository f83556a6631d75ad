"""Pooling, global pooling and broadcast without a GPU: the float64 reference on hand-computed cases, the ME constructor surface
(the 13 operator classes are real modules with ME's signatures; unsupported windows fail at construction), the C-ABI
declarations and bindings, and the explicit error under the CPU oracle backend."""
import os
import re

import pytest
import torch

import MinkowskiEngine as ME
from languagegroundedsemseg_amd.me import modules as mods
from pool_reference import batches, cells, max_argrow, max_backward, seg_reduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLASSES = ["MinkowskiSumPooling", "MinkowskiAvgPooling", "MinkowskiMaxPooling", "MinkowskiPoolingTranspose", "MinkowskiAvgUnpooling",
           "MinkowskiGlobalPooling", "MinkowskiGlobalSumPooling", "MinkowskiGlobalAvgPooling", "MinkowskiGlobalMaxPooling",
           "MinkowskiBroadcast", "MinkowskiBroadcastAddition", "MinkowskiBroadcastMultiplication", "MinkowskiBroadcastConcatenation"]
LOCAL = ["MinkowskiSumPooling", "MinkowskiAvgPooling", "MinkowskiMaxPooling", "MinkowskiPoolingTranspose", "MinkowskiAvgUnpooling"]


# ---------------------------------------------------------------------------------------------- the reference itself
def test_reference_one_two_and_eight_voxels_in_a_cell():
    # cell (0,0,0) of stride 2 holds 8 voxels, cell (2,0,0) holds 2, cell (4,4,4) holds 1
    cube = [[0, x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    coords = torch.tensor(cube + [[0, 2, 0, 0], [0, 3, 1, 1], [0, 5, 5, 4]], dtype=torch.int32)
    x = torch.arange(coords.shape[0], dtype=torch.float64).view(-1, 1) * torch.tensor([[1.0, -2.0]])
    uniq, idx = cells(coords, 2)
    assert uniq.tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [0, 4, 4, 4]]
    s = seg_reduce(x, idx, 3, "sum")
    assert s[:, 0].tolist() == [sum(range(8)), 8 + 9, 10]
    assert s[:, 1].tolist() == [-2.0 * sum(range(8)), -2.0 * 17, -20.0]
    a = seg_reduce(x, idx, 3, "avg")
    assert a[:, 0].tolist() == [28 / 8, 17 / 2, 10.0]          # divided by the rows present, not by the kernel volume 8
    m = seg_reduce(x, idx, 3, "max")
    assert m.tolist() == [[7.0, 0.0], [9.0, -16.0], [10.0, -20.0]]
    assert max_argrow(x, idx, 3).tolist() == [[7, 0], [9, 8], [10, 10]]


def test_reference_negative_coordinates_floor():
    coords = torch.tensor([[0, -1, 0, 0], [0, -2, 0, 0], [0, -3, 0, 0], [0, 0, -1, 1], [0, 1, -4, 3]], dtype=torch.int32)
    uniq, idx = cells(coords, 2)
    assert uniq.tolist() == [[0, -4, 0, 0], [0, -2, 0, 0], [0, 0, -4, 2], [0, 0, -2, 0]]
    assert idx.tolist() == [1, 1, 0, 3, 2]
    uniq4, idx4 = cells(coords, 4)
    assert uniq4.tolist() == [[0, -4, 0, 0], [0, 0, -4, 0]]
    assert idx4.tolist() == [0, 0, 0, 1, 1]


def test_reference_global_pooling_with_sparse_batch_indices():
    coords = torch.tensor([[5, 0, 0, 0], [0, 1, 1, 1], [2, 3, 3, 3], [0, 9, 9, 9], [5, 7, 7, 7], [5, -1, 2, 3]], dtype=torch.int32)
    x = torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0], [6.0]], dtype=torch.float64)
    b, idx = batches(coords)
    assert b.tolist() == [0, 2, 5]
    assert seg_reduce(x, idx, 3, "sum").view(-1).tolist() == [6.0, 3.0, 12.0]
    assert seg_reduce(x, idx, 3, "avg").view(-1).tolist() == [3.0, 3.0, 4.0]
    assert seg_reduce(x, idx, 3, "max").view(-1).tolist() == [4.0, 3.0, 6.0]


def test_reference_max_tie_goes_to_the_smallest_row():
    coords = torch.tensor([[0, 1, 1, 1], [0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 1, 0]], dtype=torch.int32)
    x = torch.tensor([[3.0, 1.0], [3.0, 2.0], [1.0, 2.0], [3.0, 2.0]], dtype=torch.float64)
    _, idx = cells(coords, 2)
    arg = max_argrow(x, idx, 1)
    assert arg.tolist() == [[0, 1]]
    dx = max_backward(torch.tensor([[10.0, 20.0]]), arg, 4)
    assert dx.tolist() == [[10.0, 0.0], [0.0, 20.0], [0.0, 0.0], [0.0, 0.0]]


# ---------------------------------------------------------------------------------------------- the ME surface
def _build(name):
    cls = getattr(ME, name)
    if name in LOCAL:
        return cls(kernel_size=2, stride=2, dimension=3)
    return cls()


@pytest.mark.parametrize("name", CLASSES)
def test_operator_classes_are_real_modules(name):
    m = _build(name)
    assert isinstance(m, torch.nn.Module)
    assert not any(c.__name__ == "_OutOfScope" for c in type(m).__mro__)
    assert not hasattr(mods, "_OutOfScope")


@pytest.mark.parametrize("name", ["MinkowskiSumPooling", "MinkowskiAvgPooling", "MinkowskiMaxPooling", "MinkowskiPoolingTranspose",
                                  "MinkowskiAvgUnpooling"])
def test_local_pooling_accepts_power_of_two_windows(name):
    cls = getattr(ME, name)
    for s in (2, 4, 8, 16):
        m = cls(kernel_size=s, stride=s, dimension=3)
        assert m.kernel_size == [s] * 3 and m.stride == [s] * 3
    kg = ME.KernelGenerator(kernel_size=4, stride=4, dimension=3)
    assert cls(kernel_generator=kg).stride == [4] * 3
    assert cls(kernel_size=[2, 2, 2], stride=[2, 2, 2], dilation=1, dimension=3).kernel_size == [2, 2, 2]


@pytest.mark.parametrize("name", LOCAL)
@pytest.mark.parametrize("ks,st,dil", [(3, 2, 1), (2, 1, 1), (3, 3, 1), (2, 2, 2), ([2, 2, 4], [2, 2, 4], 1), (1, 1, 1), (6, 6, 1)])
def test_unsupported_windows_fail_at_construction(name, ks, st, dil):
    with pytest.raises(NotImplementedError, match="kernel_size == stride == 2\\^k"):
        getattr(ME, name)(kernel_size=ks, stride=st, dilation=dil, dimension=3)


def test_unsupported_window_through_a_kernel_generator_and_dimension_four():
    with pytest.raises(NotImplementedError, match="kernel_size == stride"):
        ME.MinkowskiMaxPooling(kernel_generator=ME.KernelGenerator(kernel_size=3, stride=2, dimension=3))
    with pytest.raises(NotImplementedError, match="D = 3"):
        ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=4)


def test_pooling_mode_enum():
    PM = ME.PoolingMode
    for n in ("LOCAL_SUM_POOLING", "LOCAL_AVG_POOLING", "LOCAL_MAX_POOLING", "GLOBAL_SUM_POOLING_DEFAULT",
              "GLOBAL_AVG_POOLING_DEFAULT", "GLOBAL_MAX_POOLING_DEFAULT", "GLOBAL_AVG_POOLING_KERNEL",
              "GLOBAL_MAX_POOLING_PYTORCH_INDEX"):
        assert hasattr(PM, n)
    assert ME.MinkowskiGlobalPooling().pooling_mode == PM.GLOBAL_AVG_POOLING_DEFAULT
    assert ME.MinkowskiGlobalPooling(mode=PM.GLOBAL_MAX_POOLING_KERNEL).pooling_mode == PM.GLOBAL_MAX_POOLING_KERNEL
    assert ME.MinkowskiGlobalSumPooling().pooling_mode == PM.GLOBAL_SUM_POOLING_DEFAULT
    assert ME.MinkowskiGlobalMaxPooling(mode=PM.GLOBAL_MAX_POOLING_PYTORCH_INDEX).pooling_mode.name.startswith("GLOBAL_MAX")
    with pytest.raises(ValueError):
        ME.MinkowskiGlobalPooling(mode=PM.LOCAL_SUM_POOLING)
    with pytest.raises(ValueError):
        ME.MinkowskiGlobalSumPooling(mode=PM.GLOBAL_MAX_POOLING_DEFAULT)


# ---------------------------------------------------------------------------------------------- the C-ABI
POOL_EXPORTS = ["lgs_manager_origin", "lgs_manager_segment_map", "lgs_segmap_size", "lgs_seg_workspace_bytes", "lgs_seg_reduce",
                "lgs_seg_broadcast", "lgs_seg_max_backward"]


def test_header_declares_and_engine_binds_the_pooling_exports():
    from languagegroundedsemseg_amd import engine
    txt = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    abi = int(re.search(r"#define\s+LGS_ABI_VERSION\s+(\d+)", txt).group(1))
    assert abi == engine.ABI_VERSION and abi >= 14      # the pooling exports arrived with ABI 14
    L = engine.lib()
    for name in POOL_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in engine.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    src = open(os.path.join(ROOT, "languagegroundedsemseg_amd", "build.py")).read()
    assert '"lgs_pool.hip"' in src


def test_segment_map_entry_points_reject_bad_arguments_without_a_gpu():
    from languagegroundedsemseg_amd import engine
    import ctypes
    L = engine.lib()
    assert L.lgs_manager_segment_map(None, 0, 1, None, None) != 0
    assert b"lgs_manager_segment_map" in L.lgs_last_error()
    assert L.lgs_seg_reduce(None, 0, None, None, 4, 4, None, None, 0, None, None) != 0
    assert L.lgs_seg_broadcast(None, 0, None, 4, None, 4, None, 4, 0, None) != 0
    assert L.lgs_seg_max_backward(None, None, None, 4, None, 0, None) != 0
    assert L.lgs_seg_workspace_bytes(None, 8) == 0
    k, n = ctypes.c_int(0), ctypes.c_int64(0)
    assert L.lgs_manager_origin(None, None, ctypes.byref(k), ctypes.byref(n)) != 0


# ---------------------------------------------------------------------------------------------- no silent fallback
@pytest.mark.parametrize("name", CLASSES)
def test_forward_under_the_oracle_backend_raises(name):
    from oracle.backend import OracleBackend
    prev = ME.set_backend(OracleBackend("torch"))
    try:
        coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [1, 2, 2, 2]], dtype=torch.int32)
        x = ME.SparseTensor(torch.randn(3, 4), coords)
        m = _build(name)
        with pytest.raises(RuntimeError, match="needs the HIP engine"):
            if name.startswith("MinkowskiBroadcast"):
                m(x, x)
            else:
                m(x)
    finally:
        ME.set_backend(prev)
