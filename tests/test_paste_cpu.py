"""The tail-instance paste without a GPU: the numpy restatement (tests/paste_reference.py) pinned to what the reference's own
add_instances_to_cloud wrote (tests/golden/paste.npz), the clamped window against scipy's maximum_filter, the argument that one dedup
after the rotation keeps the rows the reference's three dedups keep, the host draws, and the refusals."""
import os
import types

import numpy as np
import pytest
import torch
from scipy import ndimage

import paste_reference as pr
from languagegroundedsemseg_amd import augment

HERE = os.path.dirname(os.path.abspath(__file__))
K, T = 5, 50


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "paste.npz")))


def instances_of(fx, s):
    off = fx["bank_offsets"]
    return [(fx["bank_points"][off[i]:off[i + 1]], fx["bank_colors"][off[i]:off[i + 1]], fx["bank_labels"][off[i]:off[i + 1]],
             fx["s%d_matrices" % s][k]) for k, i in enumerate(fx["s%d_picked" % s])]


def test_fixture_holds_the_cases_it_was_built_for(fx):
    t0, t1 = fx["s0_trial"], fx["s1_trial"]
    assert (t0 == 0).any() and ((t0 > 0) & (t0 < T)).any() and (t1 == T).all()
    assert (fx["s0_vox"] < 0).any() and (fx["s1_vox"] < 0).any()
    assert any(fx["s%d_picked" % s][k] == 0 and fx["s%d_mean_differs_%d" % (s, k)] for s in (0, 1) for k in range(K))
    assert min(fx["s0_floor_margin"], fx["s1_floor_margin"]) > 1e-6
    for s in (0, 1):          # the categories and instances the reference drew are consistent with the bank
        assert np.array_equal(fx["bank_categories"][fx["s%d_picked" % s]], fx["s%d_samples" % s])


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_equals_the_reference_output_exactly(fx, s):
    pre = "s%d_" % s
    got = pr.paste_scene(fx[pre + "vox"], fx[pre + "vox_feats"], fx[pre + "vox_labels"], fx[pre + "boxes"], fx[pre + "scale"], fx[pre + "m_r"],
                         instances_of(fx, s), fx[pre + "draws"], T)
    assert np.array_equal(got["trial"], fx[pre + "trial"]) and np.array_equal(got["centroid"], fx[pre + "centroid"])
    assert np.array_equal(got["coords"], fx[pre + "out_coords"])          # rows in the same order
    assert np.array_equal(got["feats"], fx[pre + "out_feats"]) and np.array_equal(got["labels"], fx[pre + "out_labels"])
    # the scene's own voxelisation with M_v alone, first dedup included
    m_v = np.diag([fx[pre + "scale"]] * 3 + [1.0])
    v = pr.affine_floor(fx[pre + "points"], m_v)
    assert np.array_equal(v[pr.first_rows(v)], fx[pre + "vox"])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (2, 3), (17, 5)])
def test_clamped_window_equals_scipy_maximum_filter_with_reflect(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    hm = rng.integers(-40, 40, shape)
    assert np.array_equal(pr.clamped_max_filter(hm), ndimage.maximum_filter(hm, size=5))
    assert np.array_equal(pr.clamped_max_filter(hm.astype(np.float64)), ndimage.maximum_filter(hm.astype(np.float64), size=5))


@pytest.mark.parametrize("s", [0, 1])
def test_one_dedup_after_the_rotation_keeps_what_three_dedups_keep(fx, s):
    """the scene with its duplicate voxel rows left in, the instances with theirs: the same final rows in the same order"""
    pre = "s%d_" % s
    m_v = np.diag([fx[pre + "scale"]] * 3 + [1.0])
    v = pr.affine_floor(fx[pre + "points"], m_v)
    assert len(v) > len(fx[pre + "vox"])                                   # there are duplicates to drop
    args = (v, fx[pre + "colors"], fx[pre + "labels"], fx[pre + "boxes"], fx[pre + "scale"], fx[pre + "m_r"], instances_of(fx, s), fx[pre + "draws"], T)
    three, one = pr.paste_scene(*args, three_dedups=True), pr.paste_scene(*args, three_dedups=False)
    assert len(one["pre_coords"]) > len(three["pre_coords"])
    for key in ("coords", "feats", "labels", "trial", "centroid"):
        assert np.array_equal(three[key], one[key]), key
    assert np.array_equal(three["coords"], fx[pre + "out_coords"])


def host_bank(fx):
    return types.SimpleNamespace(offsets=fx["bank_offsets"], categories=fx["bank_categories"])


def test_draw_frequencies_follow_the_weights_and_instances_are_uniform(fx):
    tail = augment.TailInstancePaste(host_bank(fx), fx["class_ids"], fx["weights"] * 3.0, num_instances=25, seed=4)
    plans = [tail.draw(32) for _ in range(10)]
    cats = np.concatenate([p.categories.reshape(-1) for p in plans])
    inst = np.concatenate([p.instances.reshape(-1) for p in plans])
    n = len(cats)
    assert n == 8000 and np.array_equal(fx["bank_categories"][inst], cats)
    for c, p in zip(fx["class_ids"], fx["weights"]):
        assert abs((cats == c).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n), c
        pool = np.flatnonzero(fx["bank_categories"] == c)
        m = (cats == c).sum()
        for i in pool:
            q = 1.0 / len(pool)
            assert abs((inst == i).sum() / m - q) <= 5 * np.sqrt(q * (1 - q) / m), i
    p = plans[0]
    assert p.matrices.shape == (32, 25, 4, 4) and p.scene_seeds.shape == (32,) and p.max_iterations == 50 and p.max_map_cells == 1 << 18
    # the chain binds its own voxeliser's matrix construction: scale within the bounds, a rotation in the upper block
    aug = augment.DeviceAugmentation(voxel_size=0.05, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
                                     tail_instances=augment.TailInstancePaste(host_bank(fx), fx["class_ids"], fx["weights"], seed=1), seed=2)
    plan = aug.draw(3)
    m = plan.paste.matrices[:, :, :3, :3]
    sc = np.cbrt(np.linalg.det(m))
    assert plan.paste.instances.shape == (3, 5) and ((sc >= 18.0 - 1e-9) & (sc <= 22.0 + 1e-9)).all() and len(np.unique(sc.round(9))) == 15
    assert np.abs(m @ m.transpose(0, 1, 3, 2) / sc[..., None, None] ** 2 - np.eye(3)).max() < 1e-12
    assert plan.rotations.shape == (3, 4, 4)
    # the chain's own decisions do not move when the paste is switched on
    plain = augment.DeviceAugmentation(voxel_size=0.05, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
                                       seed=2).draw(3)
    assert np.array_equal(plain.matrices, plan.matrices) and plain.seed == plan.seed and plain.paste is None
    for s in range(3):
        assert np.array_equal(plan.rotations[s] @ np.diag([plan.scale[s]] * 3 + [1.0]), plan.matrices[s])


def test_refusals_by_name(fx):
    class Dataset:
        CLIP_BOUND = None
        ELASTIC_DISTORT_PARAMS = ((0.2, 0.4), (0.8, 1.6))
        VOXEL_SIZE = 0.02
        ROTATION_AUGMENTATION_BOUND = ((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi))
        SCALE_AUGMENTATION_BOUND = (0.9, 1.1)
        ROTATION_AXIS = "z"
        VALID_CLASS_IDS = tuple(int(c) for c in fx["class_ids"])
    config = types.SimpleNamespace(data_aug_color_trans_ratio=0.1, data_aug_color_jitter_std=0.05, data_aug_color_scaling_factor=1.0,
                                   normalize_color=True, sample_tail_instances=True, num_instances_to_add=3,
                                   max_instance_placing_iterations=20)
    with pytest.raises(NotImplementedError, match="sample_tail_instances"):
        augment.DeviceAugmentation.from_dataset(Dataset, config)
    aug = augment.DeviceAugmentation.from_dataset(Dataset, config, instance_bank=host_bank(fx), instance_sampling_weights=fx["weights"])
    assert aug.tail.num_instances == 3 and aug.tail.max_iterations == 20 and np.allclose(aug.tail.weights, fx["weights"])
    config.sample_tail_instances = False
    assert augment.DeviceAugmentation.from_dataset(Dataset, config, instance_bank=host_bank(fx)).tail is None
    with pytest.raises(NotImplementedError, match="instance_augmentation"):          # stays refused as before
        augment.DeviceAugmentation(voxel_size=0.02, instance_augmentation="raw")
    # more than 1024 (scene, instance) slots
    with pytest.raises(ValueError, match="LGS_PASTE_MAX_SLOTS"):
        augment.TailInstancePaste(host_bank(fx), fx["class_ids"], fx["weights"], num_instances=33).draw(32)
    # a category with a weight and no instance
    with pytest.raises(ValueError, match="no instance"):
        augment.TailInstancePaste(host_bank(fx), [2, 4, 7, 9, 11], [1, 1, 1, 1, 1])
    # host tensors
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.InstanceBank(torch.from_numpy(fx["bank_points"]), torch.from_numpy(fx["bank_colors"]), torch.from_numpy(fx["bank_labels"]),
                             fx["bank_offsets"], fx["bank_categories"])
    plan = augment.TailInstancePaste(host_bank(fx), fx["class_ids"], fx["weights"]).draw(1)
    c = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.paste_instances(c, torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), [0, 4], [None], plan, [20.0], np.eye(4)[None])


def test_entry_points_reject_null_arguments_and_bad_shapes_before_any_hip_call():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    assert L.lgs_paste_workspace_bytes(0, 0, 0, 1 << 18) == 0 and L.lgs_paste_workspace_bytes(8, 1025, 5000, 1 << 18) == 0
    assert L.lgs_paste_workspace_bytes(8, 3, 0, 1 << 18) == 0 and L.lgs_paste_workspace_bytes(8, 0, 0, 0) == 0
    a, b = L.lgs_paste_workspace_bytes(8, 40, 80000, 1 << 18), L.lgs_paste_workspace_bytes(8, 40, 80000, 1 << 17)
    assert a - b == 8 * (1 << 17) * 4 and b > 80000 * (16 + 4 + 2 * 12)
    null = [None] * 3 + [0, 1] + [None] * 3 + [0, None, None, 0, 0, None, None, None, 0, None, 50, 0, 1 << 18] + [None] * 7
    assert L.lgs_paste_instances(*null) != 0 and b"lgs_paste_instances" in L.lgs_last_error()
    null[11] = 1025
    assert L.lgs_paste_instances(*null) != 0 and b"LGS_PASTE_MAX_SLOTS" in L.lgs_last_error()
