"""Instance targets without a GPU: the numpy restatement (tests/insttarget_reference.py) against what the reference's own
get_instance_info wrote (tests/golden/insttarget.npz, tests/golden/make_insttarget_fixtures.py) and against the offset losses of the
insseg fixture; the C-ABI's size answers and refusals; the torch path of the loss; the refusals of the Python surface."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import insttarget_reference as ir
from languagegroundedsemseg_amd import augment, engine, instances, tuning
from languagegroundedsemseg_amd.losses import fused_instance_offset_losses, instance_offset_losses

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    return np.load(os.path.join(G, "insttarget.npz"))


def test_restatement_equals_the_recorded_reference_outputs():
    fx = fixture()
    coords, masked = fx["coords"], [int(v) for v in fx["masked_labels"]]
    ids = ir.mask_ids(fx["instance_ids"], fx["labels"], masked)
    assert len(coords) == 613 and (coords[:, 1:] < 0).any()
    for b in range(3):
        rows = coords[:, 0] == b
        info = ir.get_instance_info(coords[rows, 1:], ids[rows])
        assert np.array_equal(info["ids"], fx["s%d_ids" % b])
        assert info["center"].dtype == np.float32 and np.array_equal(info["center"].view(np.int32), fx["s%d_center" % b].view(np.int32))
        assert sorted(info["occupancy"]) == list(fx["s%d_occ_id" % b])
        assert [info["occupancy"][k] for k in sorted(info["occupancy"])] == list(fx["s%d_occ_count" % b])
        assert np.array_equal(np.array([info["bbox"][k] for k in sorted(info["bbox"])]), fx["s%d_bbox" % b])
    # the batch form: the same centres, an instance per (scene, id)
    keys, count, bbox, center, row, centers = ir.batch_instance_info(coords, ids)
    assert np.array_equal(centers.view(np.int32), np.concatenate([fx["s%d_center" % b] for b in range(3)]).view(np.int32))
    assert len(keys) == sum(len(fx["s%d_occ_id" % b]) for b in range(3))
    assert list(count) == [int(c) for b in range(3) for c in fx["s%d_occ_count" % b]]
    three = keys == ((1 << 32) | 9)                                      # the instance of 3 points: thirds, not representable
    assert count[three][0] == 3 and np.array_equal(center[three][0], np.array([5 / 3, 1 / 3, -5 / 3], np.float64).astype(np.float32))


def test_restatement_reproduces_the_insseg_fixture_losses():
    fx = np.load(os.path.join(G, "insseg_res16unet14a_forward.npz"))
    xyz, inst = fx["coords"][:, 1:], fx["inst"]
    info = ir.get_instance_info(xyz, inst)          # (that fixture took its centres over all rows: one scene as far as the ids go)
    valid = inst != -1
    assert valid.any() and np.abs(info["center"][valid] - fx["centers"][valid]).max() <= 1e-5
    nl, dl = ir.offset_losses(fx["offsets"], xyz, info["center"], inst, float(fx["voxel"]))
    assert abs(nl - float(fx["norm_loss"])) < 1e-5 and abs(dl - float(fx["dir_loss"])) < 1e-5


def _a256(b):
    return (b + 255) // 256 * 256


def test_workspace_sizes_and_refusals_through_the_c_abi():
    L = engine.lib()
    for cap in (1, 32, 33, 4096, 4097, 65536):
        t = 64
        while t < 2 * cap:
            t *= 2
        want = sum(_a256(w * t) for w in (8, 4, 24, 12, 12, 4))         # key, count, three sums, min, max, row of every entry
        assert L.lgs_instance_info_workspace_bytes(0, cap) == want == L.lgs_instance_info_workspace_bytes(1 << 20, cap), cap
    assert L.lgs_instance_info_workspace_bytes(0, 0) == -1 and L.lgs_instance_info_workspace_bytes(0, 65537) == -1
    assert L.lgs_instance_info_workspace_bytes(-1, 16) == -1 and L.lgs_instance_info_workspace_bytes(1 << 31, 16) == -1
    one = ctypes.c_int64(0)
    for cap in (0, 65537):
        assert L.lgs_instance_info(1, 1, None, 0, None, 0, cap, 1, 1, 1, 1, 1, 1, None, 1, 1, None) != 0
        assert b"lgs_instance_info: inst_cap must be in 1 .. 65536" in L.lgs_last_error()
    assert L.lgs_instance_info(None, None, None, 0, None, 0, 16, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"lgs_instance_info: null output or workspace" in L.lgs_last_error()
    assert L.lgs_instance_info(None, None, None, 5, None, 0, 16, None, None, 1, 1, 1, 1, None, 1, 1, None) != 0
    assert b"lgs_instance_info: null point argument" in L.lgs_last_error()
    assert L.lgs_instance_info(None, None, None, 0, ctypes.byref(one), 33, 16, None, None, 1, 1, 1, 1, None, 1, 1, None) != 0
    assert b"lgs_instance_info: at most 32 masked labels" in L.lgs_last_error()
    assert L.lgs_instance_info(None, None, None, 0, ctypes.byref(one), 1, 16, None, None, 1, 1, 1, 1, None, 1, 1, None) != 0
    assert b"masked labels announced" in L.lgs_last_error()
    assert L.lgs_offset_loss_forward(None, None, None, None, 0, 0.02, engine.LGS_F32, None, 1, None, None, None, None) != 0
    assert b"lgs_offset_loss_forward: partial_rows must be in 1 .. 1024" in L.lgs_last_error()
    assert L.lgs_offset_loss_forward(None, None, None, None, 0, 0.02, engine.LGS_F32, 1, 1025, 1, 1, 1, None) != 0
    assert b"lgs_offset_loss_forward: partial_rows must be in 1 .. 1024" in L.lgs_last_error()
    assert L.lgs_offset_loss_forward(None, None, None, None, 4, 0.02, engine.LGS_F32, 1, 1, 1, 1, 1, None) != 0
    assert b"lgs_offset_loss_forward: null input" in L.lgs_last_error()
    assert L.lgs_offset_loss_forward(None, None, None, None, 0, 0.02, 7, 1, 1, 1, 1, 1, None) != 0
    assert b"lgs_offset_loss_forward: unknown dtype" in L.lgs_last_error()
    assert L.lgs_offset_loss_backward(None, None, None, None, 0, 0.02, engine.LGS_F32, None, None, None, None, None) != 0
    assert b"lgs_offset_loss_backward: null gradient or valid count" in L.lgs_last_error()
    assert L.lgs_offset_loss_backward(None, None, None, None, 4, 0.02, engine.LGS_F32, 1, 1, 1, None, None) != 0
    assert b"lgs_offset_loss_backward: null input or output" in L.lgs_last_error()
    for name in ("lgs_instance_info_workspace_bytes", "lgs_instance_info", "lgs_offset_loss_forward", "lgs_offset_loss_backward"):
        assert name in engine.EXPORTS


def test_torch_path_on_cpu_tensors_equals_the_parent_loss_on_reference_centres():
    fx = fixture()
    coords = torch.from_numpy(fx["coords"])
    ids_np = ir.mask_ids(fx["instance_ids"], fx["labels"], [int(v) for v in fx["masked_labels"]])
    ref_centers = torch.from_numpy(np.concatenate([fx["s%d_center" % b] for b in range(3)]))
    assert torch.equal(instances.centers_torch(coords, torch.from_numpy(ids_np)), ref_centers)
    g = torch.Generator().manual_seed(3)
    po = (torch.randn(coords.shape[0], 3, generator=g) * 0.3).requires_grad_(True)
    po2 = po.detach().clone().requires_grad_(True)
    nl, dl = fused_instance_offset_losses(po, coords, torch.from_numpy(ids_np), 0.02)
    nl2, dl2 = instance_offset_losses(po2, coords[:, 1:], ref_centers, torch.from_numpy(ids_np), 0.02)
    assert torch.equal(nl, nl2) and torch.equal(dl, dl2)
    (2.0 * nl + 3.0 * dl).backward()
    (2.0 * nl2 + 3.0 * dl2).backward()
    assert torch.equal(po.grad, po2.grad)
    want = ir.offset_losses(po.detach().numpy(), fx["coords"][:, 1:], ref_centers.numpy(), ids_np, 0.02)
    assert abs(float(nl.detach()) - want[0]) < 1e-5 and abs(float(dl.detach()) - want[1]) < 1e-5
    with pytest.raises(ValueError, match=r"pt_offsets must be \[N, 3\]"):
        fused_instance_offset_losses(po[:, :2], coords, torch.from_numpy(ids_np), 0.02)
    with pytest.raises(ValueError, match="instance targets of 612 rows for 613 offsets"):
        fused_instance_offset_losses(po, coords, torch.from_numpy(ids_np[:-1]), 0.02)


def test_host_tensors_and_bad_arguments_are_refused_by_name():
    fx = fixture()
    coords, ids = torch.from_numpy(fx["coords"]), torch.from_numpy(fx["instance_ids"])
    with pytest.raises(RuntimeError, match="coords must be a HIP tensor.*no CPU fallback"):
        instances.instance_info(coords, ids)
    assert "INST_TARGETS_FUSED" in tuning.HOST_KNOBS and tuning.HOST_KNOBS["INST_TARGETS_FUSED"][0] in (0, 1)
    assert sorted(instances.STATUS_BITS) == [1, 2, 4]


def test_instances_with_tail_instances_is_refused_by_name():
    tail = types.SimpleNamespace(rigid=lambda r, n: None)               # stands for a TailInstancePaste: the refusal comes first
    aug = augment.DeviceAugmentation(0.02, tail_instances=tail)
    z = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="instances= together with tail_instances"):
        aug(z, z, torch.zeros(4, dtype=torch.int64), [0, 4], instances=torch.zeros(4, dtype=torch.int64))
