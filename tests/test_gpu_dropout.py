"""The device RandomDropout (languagegroundedsemseg_amd/augment.py, csrc/lgs_dropout.hip) against the numpy restatement of its contract
(tests/dropout_reference.py), bit for bit: the selection is integer work throughout.  Shapes are the smallest that reach each branch:
a tile is 2048 rows of one scene, a workgroup 256 threads, a wave 64 lanes."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import augment_reference as ar
import dropout_reference as dr
from languagegroundedsemseg_amd import augment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 2048
# wave, workgroup and tile boundaries, empty scenes at the front, in the middle and at the end, two scenes of several tiles plus a row
SIZES = [0, 1, 2, 5, 15, 63, 64, 65, 255, 256, 257, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 0, 3, 127, 128, 129, 511, 513, 1023, 1025,
         31, 33, 7, 300, 3 * TILE + 1, 1, 0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def run(off, apply, **kw):
    rows, o = augment.random_dropout_rows(dev(off), int(off[-1]), apply, **kw)
    assert o.device.cpu().tolist() == o.host and rows.shape[0] == o.host[-1] and rows.dtype == torch.int64
    return rows.cpu().numpy(), o.host


# ---- 1. the generator path against the restatement
def test_rows_and_offsets_equal_the_restatement_exactly():
    assert len(SIZES) == 32
    off = offsets_of(SIZES)
    apply = [s not in (4, 9, 13, 16, 20, 24, 27) for s in range(32)]        # mixed; the one-row scene (k = 0) and the large ones apply
    seeds = [(s * 2654435761 + 99) % (1 << 32) for s in range(32)]
    seed = (0x5eed << 32) | 0x89abcdef                                # both halves of the seed are in the key
    want_rows, want_off = dr.select(off, apply, 0.2, seed=seed, scene_seeds=seeds)
    got_rows, got_off = run(off, apply, ratio=0.2, seed=seed, scene_seeds=seeds)
    assert got_off == want_off and np.array_equal(got_rows, want_rows)
    again, _ = run(off, apply, ratio=0.2, seed=seed, scene_seeds=seeds)        # (the call has no launch-grid setting: a tile's workgroup
    assert np.array_equal(again, got_rows)                                       # is a function of the offsets alone)
    # a scene's subset is a function of (seed, scene seed, its rows) alone: scene 15 on its own, elsewhere in a batch
    alone, o = run(offsets_of([7, SIZES[15]]), [False, True], ratio=0.2, seed=seed, scene_seeds=[0, seeds[15]])
    assert np.array_equal(alone[7:] - 7, want_rows[want_off[15]:want_off[16]] - off[15]) and o == [0, 7, 7 + dr.keep_count(SIZES[15], 0.2)]
    # another seed half, another scene seed: another subset of the same size
    for change in (dict(seed=seed + 1), dict(seed=seed + (1 << 32)), dict(scene_seeds=[0, seeds[15] + 1])):
        other, o2 = run(offsets_of([7, SIZES[15]]), [False, True], **dict(dict(ratio=0.2, seed=seed, scene_seeds=[0, seeds[15]]), **change))
        assert o2 == o and not np.array_equal(other, alone)
    # nothing applies / ratio 0: the identity; an empty batch
    ident, o = run(off, [False] * 32, ratio=0.2, seed=seed)
    assert np.array_equal(ident, np.arange(off[-1])) and o == off.tolist()
    ident, o = run(off, [True] * 32, ratio=0.0, seed=seed)
    assert np.array_equal(ident, np.arange(off[-1])) and o == off.tolist()
    none, o = run(np.zeros(4, np.int64), [True] * 3, ratio=0.2)
    assert none.shape == (0,) and o == [0, 0, 0, 0]


# ---- 2. the count rule
@pytest.mark.parametrize("ratio", [0.1, 0.2, 0.3, 0.5])
def test_counts_equal_the_reference_rule_for_every_small_scene(ratio):
    sizes = list(range(301)) + [0] * 19                               # ten calls of 32 scenes
    for at in range(0, 320, 32):
        chunk = sizes[at:at + 32]
        off = offsets_of(chunk)
        rows, o = run(off, [True] * 32, ratio=ratio, seed=at + 1, scene_seeds=list(range(32)))
        assert list(np.diff(o)) == [int(n * (1 - ratio)) for n in chunk], (ratio, at)
        want_rows, want_off = dr.select(off, [True] * 32, ratio, seed=at + 1, scene_seeds=list(range(32)))
        assert o == want_off and np.array_equal(rows, want_rows)


# ---- 3. ties (teacher-forced keys)
def test_equal_keys_resolve_towards_the_lower_row():
    # all keys equal: the first k rows, in a scene of several tiles that does not begin at a tile boundary of the batch
    off = offsets_of([100, 2 * TILE + 500, 9])
    keys = np.full(off[-1], 7, np.int32)
    rows, o = run(off, [True, True, False], ratio=0.2, keys=dev(keys))
    k = [dr.keep_count(100, 0.2), dr.keep_count(2 * TILE + 500, 0.2)]
    assert o == [0, k[0], k[0] + k[1], k[0] + k[1] + 9]
    assert np.array_equal(rows, np.concatenate([np.arange(k[0]), 100 + np.arange(k[1]), off[2] + np.arange(9)]))
    # keys from {0, 1, 2}, threshold 1.  1900 zeros in rows [100, 2000); ones in rows [40, 90) (across the wave boundary at 64) and
    # [2030, 2070) (across the tile boundary at 2048); ratio 0.5: scene A (3860 rows) keeps 1930 = the zeros and 30 ones, the cut
    # falls at row 70; scene B (3950 rows) keeps 1975 = the zeros and 75 ones, the cut falls at row 2055
    scenes = []
    for n in (3860, 3950):
        kk = np.full(n, 2, np.int32)
        kk[100:2000] = 0
        kk[40:90] = 1
        kk[2030:2070] = 1
        scenes.append(kk)
    rng = np.random.default_rng(3)
    scenes.append(rng.integers(0, 3, 5000).astype(np.int32))         # and at random: the threshold's ties lie in every wave
    scenes.insert(1, np.zeros(37, np.int32))                          # (scene B then begins at an odd row of the batch)
    off = offsets_of([len(s) for s in scenes])
    keys = np.concatenate(scenes)
    rows, o = run(off, [True] * 4, ratio=0.5, keys=dev(keys))
    want_rows, want_off = dr.select(off, [True] * 4, 0.5, keys=keys)
    assert o == want_off and np.array_equal(rows, want_rows)
    a = rows[:o[1]]
    assert a[29] == 69 and a[30] == 100 and len(a) == 1930            # scene A by hand: ones 40 .. 69, then the zeros
    b = rows[o[2]:o[3]] - off[2]
    assert np.array_equal(b, np.concatenate([np.arange(40, 90), np.arange(100, 2000), np.arange(2030, 2055)]))
    # int32 keys are read as uint32: 0xffffffff is the LARGEST key, not -1
    keys = np.tile(np.array([-1, 0], np.int32), 300)
    rows, o = run(offsets_of([600]), [True], ratio=0.5, keys=dev(keys))
    assert o == [0, 300] and np.array_equal(rows, np.arange(1, 600, 2))
    keys = np.array([-1, 0x7fffffff, -2 ** 31, 0, 5, -7, 1, -1, 3, 2], np.int32)
    rows, o = run(offsets_of([10]), [True], ratio=0.5, keys=dev(keys))
    assert rows.tolist() == [3, 4, 6, 8, 9] and np.array_equal(rows, dr.select([0, 10], [True], 0.5, keys=keys)[0])


# ---- 4. composition with another index
def test_through_composes_the_selection_with_an_index():
    off = offsets_of([300, 0, TILE + 77])
    n = int(off[-1])
    perm = np.random.default_rng(8).permutation(n).astype(np.int64)
    plain, o = run(off, [True, True, True], ratio=0.3, seed=12, scene_seeds=[4, 5, 6])
    rows, o2 = augment.random_dropout_rows(dev(off), n, [True, True, True], ratio=0.3, seed=12, scene_seeds=[4, 5, 6], through=dev(perm))
    assert o2.host == o and np.array_equal(rows.cpu().numpy(), perm[plain])
    assert np.array_equal(plain, dr.select(off, [True] * 3, 0.3, seed=12, scene_seeds=[4, 5, 6])[0])
    # the functional form: the same rows, and the gathers
    c = dev(np.arange(n * 4, dtype=np.int32).reshape(n, 4))
    f, lab, inst = dev(np.arange(n * 3, dtype=np.float32).reshape(n, 3)), dev(np.arange(n)), dev(np.arange(n) % 9)
    gc, gf, gl, gi, grows, goff = augment.random_dropout(c, f, lab, inst, scene_offsets=dev(off), apply=[True] * 3, ratio=0.3, seed=12,
                                                         scene_seeds=[4, 5, 6])
    assert goff.host == o and np.array_equal(grows.cpu().numpy(), plain)
    assert torch.equal(gc, c[grows]) and torch.equal(gf, f[grows]) and torch.equal(gl, lab[grows]) and torch.equal(gi, inst[grows])


# ---- 5 .. 7. the chain
N_PTS = 400


@pytest.fixture(scope="module")
def scene_pair():
    fx = dict(np.load(os.path.join(HERE, "golden", "augment.npz")))
    pts, cols, labels = (np.concatenate([fx["s0_" + k][:N_PTS], fx["s1_" + k][:N_PTS]]) for k in ("points", "colors", "labels"))
    inst = (np.arange(2 * N_PTS) // 37).astype(np.int64)
    return pts, cols, labels, inst, [0, N_PTS, 2 * N_PTS]


def chain(**kw):
    return augment.DeviceAugmentation(voxel_size=0.05, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
                                      normalize_color=True, seed=2, **kw)


def forced_plan(aug, dropout):
    plan = aug.draw(2)
    plan.elastic[:] = True
    plan.flip_axes[:] = [1, 2]
    plan.autocontrast[:], plan.translate[:], plan.jitter[:] = True, True, True
    plan.dropout = None if dropout is None else np.asarray(dropout, bool)
    return plan


def voxel_offsets(keep, off):
    return np.searchsorted(keep, off).astype(np.int64)


def test_chain_with_dropout_first_sees_the_surviving_rows_only(scene_pair):
    pts, cols, labels, inst, off = scene_pair
    budget = json.load(open(os.path.join(HERE, "golden", "augment_budget.json")))["colour"]["budget"]
    aug = chain(dropout=0.2, dropout_position="first")
    plan = forced_plan(aug, [True, False])
    args = (dev(pts), dev(cols), dev(labels), off)
    # the chain without dropout and without flip: the dedup's rows and the voxel coordinates as the voxeliser left them
    unflipped = dataclasses.replace(plan, flip_axes=np.zeros(2, np.int64), dropout=None)
    c0, _, _, _, s0 = chain()(*args, plan=unflipped, instances=dev(inst), return_state=True)
    keep0, c0 = s0["keep"].cpu().numpy(), c0.cpu().numpy()
    off_vox = voxel_offsets(keep0, off)
    sel, sel_off = dr.select(off_vox, [True, False], 0.2, seed=plan.seed, scene_seeds=plan.scene_seeds)
    assert sel_off[1] == dr.keep_count(off_vox[1], 0.2) >= 10 and sel_off[2] - sel_off[1] == off_vox[2] - off_vox[1]
    rng, jit = np.random.default_rng(0), {}

    def jitter_noise(n):
        jit["z"] = rng.standard_normal((n, 3)).astype(np.float32)
        return dev(jit["z"])
    coords, feats, lab, ins, state = aug(*args, plan=plan, instances=dev(inst), jitter_noise=jitter_noise, return_state=True)
    keep = keep0[sel]
    assert np.array_equal(state["keep"].cpu().numpy(), keep) and np.array_equal(state["dropout_rows"].cpu().numpy(), keep)
    assert np.array_equal(state["dedup_keep"].cpu().numpy(), keep0)
    assert np.array_equal(lab.cpu().numpy(), labels[keep]) and np.array_equal(ins.cpu().numpy(), inst[keep])
    got_c, got_f = coords.cpu().numpy(), feats.cpu().numpy()
    assert got_c.shape[0] == len(keep) == jit["z"].shape[0]
    for s, axes in ((0, (0,)), (1, (1,))):
        at = slice(sel_off[s], sel_off[s + 1])
        want = c0[sel[at]].copy()
        want[:, 1:] = ar.flip(want[:, 1:], axes)                      # the maximum is that of the surviving rows
        assert np.array_equal(got_c[at], want)
        k = keep[at]
        want_f = ar.color_chain(cols[k], blend=plan.blend[s], translation=plan.translation[s], jitter_std=0.05, jitter_noise=jit["z"][at],
                                normalize=True)["final"]              # lo / hi are those of the surviving rows
        assert np.abs(got_f[at] - want_f).max() <= budget / 255


def test_chain_with_dropout_last_selects_from_the_finished_rows(scene_pair):
    pts, cols, labels, inst, off = scene_pair
    aug = chain(dropout=0.2, dropout_position="last")
    plan = forced_plan(aug, [False, True])
    args = (dev(pts), dev(cols), dev(labels), off)
    base = chain()(*args, plan=plan, instances=dev(inst), return_state=True)
    got = aug(*args, plan=plan, instances=dev(inst), return_state=True)
    keep0 = base[4]["keep"].cpu().numpy()
    sel, sel_off = dr.select(voxel_offsets(keep0, off), [False, True], 0.2, seed=plan.seed, scene_seeds=plan.scene_seeds)
    assert len(sel) < len(keep0) and np.array_equal(got[4]["dropout_rows"].cpu().numpy(), sel)
    assert np.array_equal(got[4]["keep"].cpu().numpy(), keep0)
    for g, w in zip(got[:4], base[:4]):                               # coordinates, colours, labels, instances: untouched by the subset
        assert torch.equal(g, w[dev(sel)])


def test_chain_with_dropout_last_after_the_tail_instance_paste():
    fx = dict(np.load(os.path.join(HERE, "golden", "paste.npz")))
    pts, cols, labels = (np.concatenate([fx["s0_" + k], fx["s1_" + k]]) for k in ("points", "colors", "labels"))
    off, boxes = [0, len(fx["s0_points"]), len(pts)], [fx["s0_boxes"], fx["s1_boxes"]]
    out = {}
    for name, kw in (("base", {}), ("last", dict(dropout=0.2)), ("first", dict(dropout=0.2, dropout_position="first"))):
        bank = augment.InstanceBank(dev(fx["bank_points"]), dev(fx["bank_colors"]), dev(fx["bank_labels"]), fx["bank_offsets"], fx["bank_categories"])
        tail = augment.TailInstancePaste(bank, fx["class_ids"], fx["weights"], num_instances=4, max_iterations=9, seed=6)
        aug = augment.DeviceAugmentation(voxel_size=0.05, elastic_params=None, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)),
                                         scale_bound=(0.9, 1.1), coordinate_shift=True, seed=2, tail_instances=tail, **kw)
        plan = aug.draw(2)                                            # the same seeds: the same plan, paste included
        plan.dropout = None if name == "base" else np.array([True, True])
        plan.autocontrast[:], plan.jitter[:] = False, False           # without autocontrast, jitter (keyed by the row) and flip the
        plan.flip_axes[:] = 0                                         # position of the dropout does not show in the output
        out[name] = aug(dev(pts), dev(cols), dev(labels), off, plan=plan, scene_boxes=boxes, return_state=True)
    base, last, first = out["base"], out["last"], out["first"]
    keep0 = base[3]["keep"].cpu().numpy()
    po = base[3]["paste_offsets"]
    assert po[-1] > len(pts)                                          # instances were pasted
    sel, _ = dr.select(voxel_offsets(keep0, po), [True, True], 0.2, seed=plan.seed, scene_seeds=plan.scene_seeds)
    assert np.array_equal(last[3]["dropout_rows"].cpu().numpy(), sel)
    for g, w in zip(last[:3], base[:3]):
        assert torch.equal(g, w[dev(sel)])
    # without flip and autocontrast the position does not matter: "first" composes the same subset with the dedup's rows
    assert np.array_equal(first[3]["keep"].cpu().numpy(), keep0[sel])
    for g, w in zip(first[:3], last[:3]):
        assert torch.equal(g, w)


def test_a_plan_in_which_no_scene_drops_costs_no_second_synchronisation(scene_pair, monkeypatch):
    pts, cols, labels, inst, off = scene_pair
    args = (dev(pts), dev(cols), dev(labels), off)
    want = chain()(*args, plan=forced_plan(chain(), None), instances=dev(inst))
    import languagegroundedsemseg_amd.me.utils as me_utils
    dedup = me_utils.sparse_quantize

    def dedup_then_no_more_syncs(*a, **kw):
        keep = dedup(*a, **kw)
        torch.cuda.set_sync_debug_mode("error")                       # everything after the dedup runs under "error"
        return keep
    for position in ("first", "last"):
        aug = chain(dropout=0.2, dropout_position=position)
        plan = forced_plan(aug, [False, False])
        monkeypatch.setattr(me_utils, "sparse_quantize", dedup_then_no_more_syncs)
        try:
            got = aug(*args, plan=plan, instances=dev(inst))
        finally:
            torch.cuda.set_sync_debug_mode("default")
            monkeypatch.setattr(me_utils, "sparse_quantize", dedup)
        assert len(got) == 4 and all(torch.equal(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="no dropout decisions"):          # a plan from a chain without dropout is not taken for "no scene drops"
        chain(dropout=0.2)(*args, plan=forced_plan(chain(), None))
    # and a plan in which one does drop is what synchronises a second time
    aug = chain(dropout=0.2, dropout_position="last")
    monkeypatch.setattr(me_utils, "sparse_quantize", dedup_then_no_more_syncs)
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            aug(*args, plan=forced_plan(aug, [True, False]), instances=dev(inst))
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.setattr(me_utils, "sparse_quantize", dedup)
