"""The call layer (languagegroundedsemseg_amd/hipcall.py) on the device: the operators that take the stream's shared grow-only scratch
give the same bits whatever the last call left in it and after it was replaced by a larger one, and the raw stream handle follows
torch's current stream.  Everything compared here is integer or index work: exact."""
import os

import numpy as np
import pytest
import torch

from languagegroundedsemseg_amd import augment, engine, hipcall
from languagegroundedsemseg_amd.me.utils import sparse_quantize, voxelize
from languagegroundedsemseg_amd.pointgroup import cluster_points
from test_gpu_cluster import _check as check_clusters, _scene as cluster_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "paste.npz")))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fill_scratch(needed, byte):
    """what the previous call on this stream left in the scratch: `byte` everywhere"""
    hipcall.scratch(max(1 << 20, needed), DEV).fill_(byte)


def paste_scratch_bytes(fx, max_map_cells):
    rows = np.diff(fx["bank_offsets"])
    picked = np.concatenate([fx["s0_picked"], fx["s1_picked"]])
    return int(engine.lib().lgs_paste_workspace_bytes(2, len(picked), int(rows[picked].sum()), max_map_cells))


def paste_equals_the_fixture(fx, max_map_cells=1 << 18):
    """the two-scene case of tests/golden/paste.npz in one call, compared as tests/test_gpu_paste.py compares it"""
    bank = augment.InstanceBank(dev(fx["bank_points"]), dev(fx["bank_colors"]), dev(fx["bank_labels"]), fx["bank_offsets"], fx["bank_categories"])
    pts = np.concatenate([fx["s0_points"], fx["s1_points"]])
    off = [0, len(fx["s0_points"]), len(pts)]
    scale = [float(fx["s0_scale"]), float(fx["s1_scale"])]
    vox = augment.voxelize_batched(dev(pts), off, np.stack([np.diag([s, s, s, 1.0]) for s in scale]))
    plan = augment.PastePlan(bank, np.stack([fx["s0_picked"], fx["s1_picked"]]), np.stack([fx["s0_samples"], fx["s1_samples"]]),
                             np.stack([fx["s0_matrices"], fx["s1_matrices"]]), np.zeros(2, np.uint32), 0, 50, max_map_cells)
    co, fo, lo, off_out, status, state = augment.paste_instances(
        vox, dev(np.concatenate([fx["s0_colors"], fx["s1_colors"]])), dev(np.concatenate([fx["s0_labels"], fx["s1_labels"]])), off,
        [fx["s0_boxes"], fx["s1_boxes"]], plan, scale, np.stack([fx["s0_m_r"], fx["s1_m_r"]]),
        trial_draws=np.stack([fx["s0_draws"], fx["s1_draws"]]), return_state=True)
    assert augment.aug_status(status) == []
    placement = state["placement"].cpu().numpy()
    assert state["slots"] == [(s, k) for s in (0, 1) for k in range(5)]
    assert np.array_equal(placement[:, 0], np.concatenate([fx["s0_trial"], fx["s1_trial"]]))
    assert np.array_equal(placement[:, 1:], np.concatenate([fx["s0_centroid"], fx["s1_centroid"]]))
    keep = sparse_quantize(co, return_maps_only=True)
    c, f, lab = co.index_select(0, keep).cpu().numpy(), fo.index_select(0, keep).cpu().numpy(), lo.index_select(0, keep).cpu().numpy()
    n0 = len(fx["s0_out_coords"])
    assert (c[:n0, 0] == 0).all() and (c[n0:, 0] == 1).all() and len(c) == n0 + len(fx["s1_out_coords"])
    assert np.array_equal(c[:, 1:], np.concatenate([fx["s0_out_coords"], fx["s1_out_coords"]]).astype(np.int64))
    assert np.array_equal(f, np.concatenate([fx["s0_out_feats"], fx["s1_out_feats"]]))
    assert np.array_equal(lab, np.concatenate([fx["s0_out_labels"], fx["s1_out_labels"]]))
    return co.cpu().numpy(), fo.cpu().numpy(), lo.cpu().numpy(), placement


def test_paste_does_not_read_what_the_scratch_held(fx):
    needed = paste_scratch_bytes(fx, 1 << 18)
    assert needed > 0
    runs = []
    for byte in (0xFF, 0x00):
        fill_scratch(needed, byte)
        runs.append(paste_equals_the_fixture(fx))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))               # the rows the dedup drops too


def test_cluster_does_not_read_what_the_scratch_held():
    xyz, sem = cluster_scene(5, 6000)                                       # the smallest scene tests/test_gpu_cluster.py clusters
    needed = int(engine.lib().lgs_cluster_workspace_bytes(xyz.shape[0]))
    runs = []
    for byte in (0xFF, 0x00):
        fill_scratch(needed, byte)
        assert check_clusters(xyz, sem, 0.03, 30) > 3                       # equal to the oracle's BFS, cluster by cluster
        fill_scratch(needed, byte)
        runs.append(cluster_points(torch.from_numpy(xyz).to(DEV), torch.from_numpy(sem).to(DEV), 0.03, 30))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_a_small_call_after_the_scratch_grew_still_equals_the_fixture(fx):
    """on a stream of its own, so that the buffer starts out missing whatever ran before in this process"""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    small, big = paste_scratch_bytes(fx, 1 << 18), paste_scratch_bytes(fx, 1 << 22)
    with torch.cuda.stream(side):
        first = paste_equals_the_fixture(fx)
        held = hipcall.scratch(0, DEV)
        assert small <= held.numel() < big
        grown = paste_equals_the_fixture(fx, max_map_cells=1 << 22)        # (the cap alone differs: the same rows)
        now = hipcall.scratch(0, DEV)
        assert now.numel() >= big and now.data_ptr() != held.data_ptr()
        again = paste_equals_the_fixture(fx)
        assert hipcall.scratch(0, DEV) is now
    side.synchronize()
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(first, grown, again))


def test_voxelize_and_the_label_vote_follow_the_current_stream():
    rng = np.random.default_rng(4)
    pts = (rng.permutation(4096)[:64, None] // [256, 16, 1] % 16 - 8).astype(np.float32)      # 64 different cells of 0.5, exact in fp32
    pts[[17, 40, 63]] = pts[[3, 3, 21]] + np.float32(0.125)                 # 3 duplicates: two in the voxel of point 3 (one label disagrees), one of 21
    pts *= np.float32(0.5)
    labels = rng.integers(0, 5, 64)
    labels[[17, 40, 63]] = [labels[3], labels[3] + 1, labels[21]]
    kw = dict(return_index=True, return_inverse=True, quantization_size=0.5)
    want = sparse_quantize(pts, labels=labels, ignore_label=-100, **kw)
    p, lab = dev(pts), dev(labels)
    on_default = (voxelize(p, quantization_size=0.5),) + sparse_quantize(p, labels=lab, **kw)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        assert hipcall.raw_stream() == hipcall.raw_stream(DEV) == side.cuda_stream
        p2, lab2 = p + 0.0, lab + 0                                         # produced on the side stream, just before they are read
        on_side = (voxelize(p2, quantization_size=0.5),) + sparse_quantize(p2, labels=lab2, **kw)
    side.synchronize()
    assert hipcall.raw_stream() == torch.cuda.current_stream(DEV).cuda_stream != side.cuda_stream
    assert all(torch.equal(a, b) for a, b in zip(on_default, on_side))
    assert on_side[1].shape[0] == 61 and int((on_side[2] == -100).sum()) == 1
    for got, ref in zip(on_side[1:], want):
        assert np.array_equal(got.cpu().numpy(), np.asarray(ref))
