"""The tail-instance paste on the device (languagegroundedsemseg_amd/augment.py, csrc/lgs_paste.hip): exactly equal to what the
reference's own add_instances_to_cloud wrote (tests/golden/paste.npz) and to the numpy restatement (tests/paste_reference.py) on the
smallest shapes at which the kernels can go wrong.  Everything here is integer or index work, so every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import augment_reference as ar
import paste_reference as pr
from languagegroundedsemseg_amd import augment
from languagegroundedsemseg_amd.me.utils import sparse_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "paste.npz")))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_bank(instances):
    """instances: list of (points [p, 3], category) -> (InstanceBank, host arrays)"""
    rng = np.random.default_rng(11)
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p, _ in instances])
    cols = np.floor(rng.random((len(pts), 3)) * 256).astype(np.float32)
    labs = np.concatenate([np.full(len(np.asarray(p).reshape(-1, 3)), c, np.int64) for p, c in instances])
    off = np.concatenate([[0], np.cumsum([len(np.asarray(p).reshape(-1, 3)) for p, _ in instances])]).astype(np.int64)
    cats = np.asarray([c for _, c in instances], np.int64)
    return augment.InstanceBank(dev(pts), dev(cols), dev(labs), off, cats), (pts, cols, labs, off, cats)


def run_device(scenes, bank, host, T, max_map_cells=1 << 18, teacher=True, seed=0, scene_seeds=None):
    """scenes: list of dict(coords int [n, 3], feats, labels, boxes, scale, m_r, inst [K], matrices [K, 4, 4], draws [K, T, 2])
    -> the device's rows per scene, the placement per scene, the flagged scenes"""
    B, K = len(scenes), len(scenes[0]["inst"])
    off = np.concatenate([[0], np.cumsum([len(s["coords"]) for s in scenes])]).astype(np.int64)
    c = np.concatenate([np.concatenate([np.full((len(s["coords"]), 1), i), np.asarray(s["coords"]).reshape(-1, 3)], 1) for i, s in enumerate(scenes)])
    f = np.concatenate([np.asarray(s["feats"], np.float32).reshape(-1, 3) for s in scenes])
    lab = np.concatenate([np.asarray(s["labels"], np.int64).reshape(-1) for s in scenes])
    plan = augment.PastePlan(bank, np.stack([s["inst"] for s in scenes]), np.zeros((B, K), np.int64), np.stack([s["matrices"] for s in scenes]),
                             np.asarray(scene_seeds if scene_seeds is not None else np.zeros(B), np.uint32), seed, T, max_map_cells)
    draws = np.stack([s["draws"] for s in scenes]) if teacher else None
    co, fo, lo, off_out, status, state = augment.paste_instances(
        dev(c.astype(np.int32)), dev(f), dev(lab), off.tolist(), [s["boxes"] for s in scenes], plan, [s["scale"] for s in scenes],
        np.stack([s["m_r"] for s in scenes]), trial_draws=draws, return_state=True)
    co, fo, lo, placement = co.cpu().numpy(), fo.cpu().numpy(), lo.cpu().numpy(), state["placement"].cpu().numpy()
    assert off_out[0] == 0 and off_out[-1] == len(co) and len(off_out) == B + 1
    rows = []
    for i in range(B):
        r = slice(off_out[i], off_out[i + 1])
        assert (co[r, 0] == i).all()
        rows.append((co[r, 1:].astype(np.int64), fo[r], lo[r]))
    place = [[] for _ in range(B)]
    for (s, k), p in zip(state["slots"], placement):
        place[s].append(p)
    return rows, [np.asarray(p, np.int64).reshape(-1, 4) for p in place], augment.aug_status(status)


def restate(scene, host, T, three_dedups, seeds=None):
    pts, cols, labs, off, _ = host
    inst = [(pts[off[i]:off[i + 1]], cols[off[i]:off[i + 1]], labs[off[i]:off[i + 1]], scene["matrices"][k])
            for k, i in enumerate(scene["inst"]) if i >= 0]
    draws = None if seeds is not None else [scene["draws"][k] for k, i in enumerate(scene["inst"]) if i >= 0]
    if len(scene["coords"]) == 0:
        inst = []
    return pr.paste_scene(np.asarray(scene["coords"]).reshape(-1, 3), np.asarray(scene["feats"], np.float32).reshape(-1, 3),
                          np.asarray(scene["labels"], np.int64).reshape(-1), scene["boxes"] if scene["boxes"] is not None else np.zeros((0, 2, 3)),
                          scene["scale"], scene["m_r"], inst, draws, T, three_dedups=three_dedups, seeds=seeds)


def check_scene(rows, place, scene, host, T, seeds=None):
    """the device's rows equal the restatement's before any dedup, row by row, and after the final dedup what three dedups keep"""
    want = restate(scene, host, T, False, seeds)
    assert np.array_equal(rows[0], want["pre_coords"]) and np.array_equal(rows[1], want["pre_feats"]) and np.array_equal(rows[2], want["pre_labels"])
    assert np.array_equal(place[:, 0], want["trial"]) and np.array_equal(place[:, 1:], want["centroid"])
    keep = pr.first_rows(rows[0])
    three = restate(scene, host, T, True, seeds)
    assert np.array_equal(rows[0][keep], three["coords"]) and np.array_equal(rows[1][keep], three["feats"]) and np.array_equal(rows[2][keep], three["labels"])
    return want


# ---- 1. teacher-forced against what the reference wrote
def test_teacher_forced_both_scenes_in_one_call_equal_the_reference_exactly(fx):
    bank = augment.InstanceBank(dev(fx["bank_points"]), dev(fx["bank_colors"]), dev(fx["bank_labels"]), fx["bank_offsets"], fx["bank_categories"])
    pts = np.concatenate([fx["s0_points"], fx["s1_points"]])
    off = [0, len(fx["s0_points"]), len(pts)]
    scale = [float(fx["s0_scale"]), float(fx["s1_scale"])]
    m_v = np.stack([np.diag([s, s, s, 1.0]) for s in scale])
    vox = augment.voxelize_batched(dev(pts), off, m_v)                      # the scene's rows with their duplicates left in
    plan = augment.PastePlan(bank, np.stack([fx["s0_picked"], fx["s1_picked"]]), np.stack([fx["s0_samples"], fx["s1_samples"]]),
                             np.stack([fx["s0_matrices"], fx["s1_matrices"]]), np.zeros(2, np.uint32), 0, 50, 1 << 18)
    co, fo, lo, off_out, status, state = augment.paste_instances(
        vox, dev(np.concatenate([fx["s0_colors"], fx["s1_colors"]])), dev(np.concatenate([fx["s0_labels"], fx["s1_labels"]])), off,
        [fx["s0_boxes"], fx["s1_boxes"]], plan, scale, np.stack([fx["s0_m_r"], fx["s1_m_r"]]),
        trial_draws=np.stack([fx["s0_draws"], fx["s1_draws"]]), return_state=True)
    assert augment.aug_status(status) == []
    placement = state["placement"].cpu().numpy()
    assert state["slots"] == [(s, k) for s in (0, 1) for k in range(5)]
    assert np.array_equal(placement[:, 0], np.concatenate([fx["s0_trial"], fx["s1_trial"]]))
    assert np.array_equal(placement[:, 1:], np.concatenate([fx["s0_centroid"], fx["s1_centroid"]]))
    keep = sparse_quantize(co, return_maps_only=True)                       # the chain's dedup
    c, f, lab = co.index_select(0, keep).cpu().numpy(), fo.index_select(0, keep).cpu().numpy(), lo.index_select(0, keep).cpu().numpy()
    n0 = len(fx["s0_out_coords"])
    assert (c[:n0, 0] == 0).all() and (c[n0:, 0] == 1).all() and len(c) == n0 + len(fx["s1_out_coords"])
    assert np.array_equal(c[:, 1:], np.concatenate([fx["s0_out_coords"], fx["s1_out_coords"]]).astype(np.int64))
    assert np.array_equal(f, np.concatenate([fx["s0_out_feats"], fx["s1_out_feats"]]))
    assert np.array_equal(lab, np.concatenate([fx["s0_out_labels"], fx["s1_out_labels"]]))


# ---- 2. the smallest shapes that can go wrong
def rot_z(theta):
    m = np.eye(4)
    m[:3, :3] = augment.axis_rotation(2, theta)
    return m


def small_bank():
    rng = np.random.default_rng(3)
    return make_bank([(np.array([[0.31, -0.22, 0.13]]), 1),                            # 0: one point
                      (rng.random((257, 3)) * [0.6, 0.5, 0.7] - [0.3, 1.0, 0.1], 2),       # 1: 257 rows: crosses a workgroup
                      (np.array([0.5, 0.5, 0.5]) + rng.random((40, 3)) * 0.01, 3),         # 2: every row in one voxel (scale 16)
                      (np.array([[0.0, 0.0, 0.01], [0.0, 0.0, 0.07], [0.0, 0.0, 0.135]]) + 0.01, 4),      # 3: one column, 3 voxels tall
                      (rng.random((70, 3)) * 0.4 - 0.9, 5)])                               # 4: negative coordinates, two waves


def small_scenes(T):
    rng = np.random.default_rng(T)
    s16 = np.diag([16.0, 16.0, 16.0, 1.0])

    def scene(coords, boxes, inst, draws, m_r=np.eye(4), mats=None):
        coords = np.asarray(coords, np.int64).reshape(-1, 3)
        mats = np.stack([s16] * len(inst)) if mats is None else mats
        return dict(coords=coords, feats=np.floor(rng.random((len(coords), 3)) * 256).astype(np.float32), labels=rng.integers(0, 20, len(coords)),
                    boxes=boxes, scale=16.0, m_r=m_r, inst=np.asarray(inst, np.int64), matrices=mats, draws=np.asarray(draws, np.int64))
    K = 3
    fill = lambda x, y: np.tile([x, y], (K, T, 1))
    # 0: one row: a 1 x 1 map, no boxes
    s0 = scene([[7, -3, 2]], None, [0, 1, 2], fill(7, -3), m_r=rot_z(0.7), mats=np.stack([rot_z(0.3) @ s16, rot_z(-1.1) @ s16, s16]))
    # 1: negative z_min and an instance three voxels tall: int(-3 + 1.5) is -1, not -2.  A box that touches random_bb on a face
    #    (x_max * 16 == 4.5 == 5 - 0.5) makes trial 0 at x = 5 fail; trial 1 at x = 6 is clear of it
    flat = np.array([[x, y, -3] for x in range(0, 9) for y in range(-2, 3)])
    d1 = fill(6, 0)
    d1[:, 0] = [5, 1]
    s1 = scene(flat, np.array([[[-1.0, -1.0, -1.0], [4.5 / 16, 1.0, 1.0]]]), [3, 3, 0], d1)
    # 2: an empty scene in the middle of the batch: its instances are not pasted
    s2 = scene(np.zeros((0, 3)), None, [1, 0, 2], fill(0, 0))
    # 3: K = 0
    s3 = scene(rng.integers(-6, 6, (300, 3)), np.array([[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]]), [-1, -1, -1], fill(0, 0))
    # 4: a box over x <= 3 at every height: trials 0 .. 63 are drawn inside it, trial 64 (if there is one) outside
    room = np.concatenate([rng.integers([-5, -4, -2], [12, 9, 3], (500, 3)), [[-5, -4, -2], [11, 8, 2]]])
    d4 = np.stack([np.stack([rng.integers(-5, 3, T), rng.integers(-4, 9, T)], 1) for _ in range(K)])
    if T > 64:
        d4[:, 64] = [9, 5]
    d4[2] = [11, 7]                                                        # the third instance lands at trial 0
    s4 = scene(room, np.array([[[-2.0, -2.0, -2.0], [3.4 / 16, 2.0, 2.0]]]), [2, 4, 1], d4, m_r=rot_z(-2.0),
               mats=np.stack([s16, rot_z(0.5) @ s16, rot_z(2.2) @ (s16 * [[1.07], [1.07], [1.07], [1.0]])]))
    return [s0, s1, s2, s3, s4]


@pytest.mark.parametrize("T", [1, 64, 65])
def test_smallest_shapes_equal_the_restatement_exactly(T):
    bank, host = small_bank()
    scenes = small_scenes(T)
    rows, place, flagged = run_device(scenes, bank, host, T)
    assert flagged == []
    wants = [check_scene(rows[i], place[i], s, host, T) for i, s in enumerate(scenes)]
    assert len(rows[2][0]) == 0 and len(place[2]) == 0 and len(place[3]) == 0 and len(rows[3][0]) == 300
    assert len(rows[0][0]) == 1 + 1 + 257 + 40
    # the cases by name: truncation toward zero, the inclusive face test, the chunk boundary, one voxel for a whole instance
    if T > 1:
        assert list(place[1][:, 0]) == [1, 1, 1] and (place[1][:2, 3] == -1).all() and list(place[1][0, 1:3]) == [6, 0]
    else:
        assert list(place[1][:, 0]) == [1, 1, 1] and list(place[1][0, 1:3]) == [5, 1]          # exhausted at its only trial
    assert list(place[4][:, 0]) == [64 if T == 65 else T, 64 if T == 65 else T, 0]
    assert len(np.unique(wants[4]["pre_coords"][502:542], axis=0)) == 1


# ---- 3. a map larger than max_map_cells
def test_map_too_large_sets_the_bit_and_leaves_the_scene_unpasted():
    bank, host = small_bank()
    scenes = [small_scenes(5)[4], small_scenes(5)[1]]                       # maps of 17 x 13 and 9 x 5 cells
    rows, place, flagged = run_device(scenes, bank, host, 5, max_map_cells=100)
    assert flagged == [0] and (place[0][:, 0] == -1).all()
    unpasted = pr.affine_floor(scenes[0]["coords"], scenes[0]["m_r"])
    n = len(unpasted)
    assert np.array_equal(rows[0][0][:n], unpasted) and (rows[0][0][n:] == unpasted[0]).all() and len(rows[0][0]) == n + 40 + 70 + 257
    keep = pr.first_rows(rows[0][0])
    assert keep.max() < n and np.array_equal(rows[0][0][keep], unpasted[pr.first_rows(unpasted)])
    assert np.array_equal(rows[0][1][keep], scenes[0]["feats"][keep]) and np.array_equal(rows[0][2][keep], scenes[0]["labels"][keep])
    check_scene(rows[1], place[1], scenes[1], host, 5)                     # the other scene is pasted as usual


# ---- 4. device draws
def test_device_draws_depend_on_seeds_scene_instance_and_trial_alone():
    rng = np.random.default_rng(9)
    bank, host = make_bank([(np.array([[0.01, 0.02, 0.03]]), 1)])
    K, T, seed = 32, 7, (5 << 32) | 77

    def scene(coords, boxes):
        coords = np.asarray(coords, np.int64)
        return dict(coords=coords, feats=np.zeros((len(coords), 3), np.float32), labels=np.zeros(len(coords), np.int64), boxes=boxes, scale=16.0,
                    m_r=np.eye(4), inst=np.zeros(K, np.int64), matrices=np.stack([np.diag([16.0, 16.0, 16.0, 1.0])] * K), draws=None)
    a = scene([[3, -8, 0], [4, -7, 1]], None)                               # a 2 x 2 map
    b = scene(rng.integers(-9, 14, (200, 3)), np.array([[[-1.0, -1.0, -9.0], [2.5 / 16, 1.0, 9.0]]]))      # about half of the trials fail
    c = scene(rng.integers(0, 40, (90, 3)), None)
    seeds = [101, 202, 303]
    rows, place, flagged = run_device([a, b, c], bank, host, T, teacher=False, seed=seed, scene_seeds=seeds)
    rows2, place2, _ = run_device([a, b, c], bank, host, T, teacher=False, seed=seed, scene_seeds=seeds)
    assert flagged == [] and all(np.array_equal(x, y) for r, r2 in zip(rows, rows2) for x, y in zip(r, r2))       # two calls, identical bits
    assert all(np.array_equal(p, q) for p, q in zip(place, place2))
    for i, s in enumerate((a, b, c)):                                       # the restatement's Philox words and multiply-shift
        check_scene(rows[i], place[i], s, host, T, seeds=(seed, seeds[i]))
        lo, hi = s["coords"].min(0), s["coords"].max(0)
        assert (place[i][:, 1:3] >= lo[:2]).all() and (place[i][:, 1:3] <= hi[:2]).all()
    assert set(place[0][:, 1]) == {3, 4} and set(place[0][:, 2]) == {-8, -7}
    assert (place[1][:, 0] > 0).any() and (place[1][:, 0] == 0).any()
    # permuting the scenes of the batch permutes the results
    _, place3, _ = run_device([c, a, b], bank, host, T, teacher=False, seed=seed, scene_seeds=[303, 101, 202])
    assert np.array_equal(place3[0], place[2]) and np.array_equal(place3[1], place[0]) and np.array_equal(place3[2], place[1])
    _, place4, _ = run_device([a, b, c], bank, host, T, teacher=False, seed=seed + 1, scene_seeds=seeds)
    assert not np.array_equal(place4[2], place[2])


# ---- 5 + 6. no synchronisation; the chain
def fixture_chain(fx, **kw):
    bank = augment.InstanceBank(dev(fx["bank_points"]), dev(fx["bank_colors"]), dev(fx["bank_labels"]), fx["bank_offsets"], fx["bank_categories"])
    tail = augment.TailInstancePaste(bank, fx["class_ids"], fx["weights"], num_instances=4, max_iterations=9, seed=6)
    aug = augment.DeviceAugmentation(voxel_size=0.05, elastic_params=None, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)),
                                     scale_bound=(0.9, 1.1), coordinate_shift=True, seed=2, tail_instances=tail, **kw)
    pts = np.concatenate([fx["s0_points"], fx["s1_points"]])
    cols = np.concatenate([fx["s0_colors"], fx["s1_colors"]])
    labels = np.concatenate([fx["s0_labels"], fx["s1_labels"]])
    return aug, pts, cols, labels, [0, len(fx["s0_points"]), len(pts)], (fx["bank_points"], fx["bank_colors"], fx["bank_labels"], fx["bank_offsets"], fx["bank_categories"])


def test_paste_runs_without_a_synchronising_call(fx):
    aug, pts, cols, labels, off, _ = fixture_chain(fx)
    plan = aug.draw(2)
    vox = augment.voxelize_batched(dev(pts), off, np.stack([np.diag([s, s, s, 1.0]) for s in plan.scale]))
    c, l = dev(cols), dev(labels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = augment.paste_instances(vox, c, l, off, [fx["s0_boxes"], fx["s1_boxes"]], plan.paste, plan.scale, plan.rotations)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out[0].shape[0] == out[3][-1] > len(pts) and out[3][1] > off[1]
    # the chain runs everything before its dedup under the same mode, set by itself, and restores it
    got = aug(dev(pts), c, l, off, plan=plan, scene_boxes=[fx["s0_boxes"], fx["s1_boxes"]])
    assert torch.cuda.get_sync_debug_mode() == 0 and got[0].shape[0] == got[1].shape[0] == got[2].shape[0] > 0


def test_chain_without_tail_instances_is_the_composition_it_always_was():
    """tail_instances=None: bit-identical to the functional pieces in the chain's order, which is all the chain has ever been"""
    a = dict(np.load(os.path.join(HERE, "golden", "augment.npz")))
    pts, cols, labels = (np.concatenate([a["s0_" + k], a["s1_" + k]]) for k in ("points", "colors", "labels"))
    off = [0, len(a["s0_points"]), len(pts)]
    aug = augment.DeviceAugmentation(voxel_size=0.05, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
                                     normalize_color=True, coordinate_shift=True, seed=2, tail_instances=None)
    plan = aug.draw(2)
    plan.elastic[:] = True
    assert plan.paste is None
    got = aug(dev(pts), dev(cols), dev(labels), off, plan=plan)
    p = dev(pts)
    for stage, (g, m) in enumerate(aug.elastic_params):
        p = augment.elastic_distortion(p, off, g, m, plan.seed, scene_seeds=plan.scene_seeds, apply=plan.elastic, stage=stage)
    coords = augment.voxelize_batched(p, off, plan.matrices)
    keep = sparse_quantize(coords, return_maps_only=True)
    want_c, off_vox = augment.horizontal_flip(coords.index_select(0, keep), plan.flip_axes, shift=plan.shift, batch_size=2, return_offsets=True)
    want_f = augment.chromatic_augment(dev(cols).index_select(0, keep), off_vox, aug.color_params(plan), normalize=True, seed=plan.seed)
    assert torch.equal(got[0], want_c) and torch.equal(got[1], want_f) and torch.equal(got[2], dev(labels).index_select(0, keep))


def test_chain_with_a_bank_equals_the_restatement_stage_by_stage(fx):
    aug, pts, cols, labels, off, host = fixture_chain(fx)
    boxes = [fx["s0_boxes"], fx["s1_boxes"]]
    plan = aug.draw(2)
    plan.flip_axes[:] = [1, 2]
    plan.autocontrast[:], plan.translate[:], plan.jitter[:] = False, False, False          # the colours pass through: exact
    coords, feats, lab, state = aug(dev(pts), dev(cols), dev(labels.astype(np.int32)), off, plan=plan, scene_boxes=boxes, return_state=True)
    assert augment.aug_status(state["paste_status"]) == [] and lab.dtype == torch.int32
    vox = state["voxels"].cpu().numpy()
    pc, pf, pl = (t.cpu().numpy() for t in state["pasted"])
    po = state["paste_offsets"]
    keep = state["keep"].cpu().numpy()
    placement = state["paste"]["placement"].cpu().numpy()
    want_c, want_f, want_l, at = [], [], [], 0
    for s in (0, 1):
        rows = slice(off[s], off[s + 1])
        v = pr.affine_floor(pts[rows], np.diag([plan.scale[s]] * 3 + [1.0]))          # M_v only
        assert np.array_equal(vox[rows, 1:], v) and (vox[rows, 0] == s).all()
        scene = dict(coords=v, feats=cols[rows], labels=labels[rows], boxes=boxes[s], scale=plan.scale[s], m_r=plan.rotations[s],
                     inst=plan.paste.instances[s], matrices=plan.paste.matrices[s], draws=None)
        out = slice(po[s], po[s + 1])
        want = check_scene((pc[out, 1:].astype(np.int64), pf[out], pl[out]), placement[4 * s:4 * s + 4].astype(np.int64), scene, host, 9,
                           seeds=(plan.paste.seed, plan.paste.scene_seeds[s]))
        k = pr.first_rows(want["pre_coords"])
        assert np.array_equal(keep[at:at + len(k)], k + po[s])                        # the chain's one dedup
        at += len(k)
        axes = (0,) if s == 0 else (1,)
        want_c.append(ar.flip(want["pre_coords"][k].astype(np.int32), axes) + plan.shift.astype(np.int32))
        want_f.append(want["pre_feats"][k])
        want_l.append(want["pre_labels"][k])
    assert at == len(keep) and len(keep) > len(np.unique(vox, axis=0))                # instance voxels survived
    got = coords.cpu().numpy()
    assert np.array_equal(got[:, 1:], np.concatenate(want_c)) and np.array_equal(got[:, 0], np.repeat([0, 1], [len(want_c[0]), len(want_c[1])]))
    assert np.array_equal(feats.cpu().numpy(), np.concatenate(want_f)) and np.array_equal(lab.cpu().numpy(), np.concatenate(want_l))
