"""What of the nearest-voxel query can be checked without a GPU: the new symbol and its bindings, the refusals that come before any
HIP call, the knob, and the host-side checks of languagegroundedsemseg_amd/pointcloud.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_exported_and_the_abi_stays():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    assert "lgs_manager_nearest" in engine.EXPORTS and hasattr(L, "lgs_manager_nearest")
    assert L.lgs_abi_version() == engine.ABI_VERSION == 18              # a new symbol only
    args = L.lgs_manager_nearest.argtypes
    assert len(args) == 12 and args[8] is ctypes.c_double and args[7] == ctypes.POINTER(ctypes.c_double)


def test_null_arguments_are_refused_without_a_gpu():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    rows = (ctypes.c_int64 * 4)()
    pts = (ctypes.c_float * 12)()
    off = (ctypes.c_int64 * 2)(0, 4)
    rc = L.lgs_manager_nearest(None, 0, pts, 4, off, 1, 0, None, 0.5, rows, None, None)        # no manager
    assert rc != 0 and b"lgs_manager_nearest" in L.lgs_last_error() and b"null" in L.lgs_last_error()
    rc = L.lgs_manager_nearest(None, 0, None, 0, None, 1, 0, None, 0.5, None, None, None)       # no points, but no manager either
    assert rc != 0 and b"lgs_manager_nearest" in L.lgs_last_error()
    with pytest.raises(RuntimeError, match="lgs_manager_nearest"):
        engine.check(rc)


def test_the_integration_stub_declares_the_entry_point_like_the_header():
    """tests/test_abi.py reads the stub's `L.<name>.argtypes = [...]` lines, whose vocabulary has no double; this entry point's line is
    held to the header here"""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"nearest\.argtypes\s*=\s*\[([^\]]*)\]", txt)
    assert m and "nearest = L.lgs_manager_nearest" in txt
    names = {"vp": "ptr", "i64": "i64", "ci": "int", "ctypes.c_double": "f64", "ctypes.POINTER(ctypes.c_double)": "ptr"}
    got = [names[a.strip()] for a in re.split(r",\s*(?![^()]*\))", m.group(1)) if a.strip()]
    assert got == ["ptr", "int", "ptr", "i64", "ptr", "int", "int", "ptr", "f64", "ptr", "ptr", "ptr"]
    hdr = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    proto = re.search(r"int lgs_manager_nearest\(([^)]*)\);", hdr).group(1)
    kinds = ["ptr" if "*" in p else {"int": "int", "int64_t": "i64", "double": "f64"}[p.split()[0]] for p in proto.split(",")]
    assert kinds == got


def test_the_knob_is_listed():
    from languagegroundedsemseg_amd import engine
    rows = {n: (d, doc) for n, d, _, doc in engine.tuning_table()}
    assert rows["NEAREST_MAX_RING"][0] >= 1 and "k_nearest_scan" in rows["NEAREST_MAX_RING"][1]
    out = subprocess.run([sys.executable, "-m", "languagegroundedsemseg_amd.tuning"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         check=True).stdout.decode()
    assert "LGS_NEAREST_MAX_RING" in out


def _rotation(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])


def test_similarity_check_and_the_shapes_of_a_transformation():
    from languagegroundedsemseg_amd.pointcloud import affines_from_transformation
    t = np.eye(4)
    t[:3, :3] = 50.0 * _rotation(0.7, -0.2)
    t[:3, 3] = [1.0, 2.0, 3.0]
    want = t[:3].reshape(-1).tolist()
    assert affines_from_transformation(t, 1) == want
    assert affines_from_transformation(t[:3], 1) == want
    assert affines_from_transformation(torch.from_numpy(t.reshape(16)), 1) == want
    assert affines_from_transformation(t, 3) == want * 3                                                       # one matrix for every scene
    row = np.concatenate([t.reshape(1, 16), np.zeros((1, 4))], 1)[:, :16]
    assert affines_from_transformation(np.repeat(row, 2, 0), 2) == want * 2                                    # [b, 16], as collated
    mirror = t.copy()
    mirror[:3, 0] *= -1.0                                                                                       # a reflection is a similarity
    assert len(affines_from_transformation(mirror, 1)) == 12
    for bad in (np.diag([20.0, 20.0, 10.0, 1.0]),                                                               # anisotropic, rotation-free
                t @ np.diag([1.0, 1.0, 1.0 + 1e-4, 1.0]),                                                       # anisotropic by 1e-4
                np.array([[1.0, 0.2, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]),   # a shear
                np.zeros((4, 4))):
        with pytest.raises(NotImplementedError, match="similarity"):
            affines_from_transformation(bad, 1)
    with pytest.raises(ValueError):
        affines_from_transformation(np.eye(3), 1)
    with pytest.raises(ValueError):
        affines_from_transformation(np.repeat(row, 2, 0), 3)
    nan = t.copy()
    nan[0, 3] = np.nan
    with pytest.raises(ValueError):
        affines_from_transformation(nan, 1)


def test_shape_checks_come_before_anything_touches_a_device():
    from languagegroundedsemseg_amd.pointcloud import PointCloudEvaluator, _scene_offsets, nearest_voxel
    with pytest.raises(ValueError, match=r"\[M, 3\]"):
        nearest_voxel(None, torch.zeros(5, 4))
    with pytest.raises(ValueError, match="float32"):
        nearest_voxel(None, torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_voxel(None, torch.zeros(5, 3))
    for bad in ([0, 3], [1, 5], [0, 4, 2, 5], [5]):
        with pytest.raises(ValueError):
            _scene_offsets(bad, 5, "cpu")
    off, b = _scene_offsets([0, 2, 2, 5], 5, "cpu")
    assert b == 3 and off.dtype == torch.int64 and off.tolist() == [0, 2, 2, 5]
    ev = PointCloudEvaluator(4, ignore_label=255)
    assert ev.confmat.dtype == torch.int64 and ev.confmat.shape == (4, 4) and "confmat" in dict(ev.named_buffers())
    with pytest.raises(ValueError):
        ev.update(torch.zeros(3, 4, 2), None, torch.zeros(5, 3), torch.zeros(5))
    with pytest.raises(ValueError):
        ev.update(torch.zeros(3, 4), None, torch.zeros(5, 3), torch.zeros(4))
