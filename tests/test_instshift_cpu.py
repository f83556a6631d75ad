"""CPU-side checks of the device instance shifts (no GPU): the numpy restatement of the contract (tests/instshift_reference.py) against
what the reference's own augment_instances / shift_hue returned (tests/golden/instshift.npz, written by
tests/golden/make_instshift_fixtures.py), the statistics of the generator path on the restatement, and the argument handling of the
Python layer and the C-ABI."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

import instshift_reference as ir

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "instshift.npz")))


def batch_of(fx):
    cat = lambda k: np.concatenate([fx["s0_" + k], fx["s1_" + k]])
    return cat("points"), cat("colors"), cat("labels"), cat("ids"), [0, len(fx["s0_points"]), len(fx["s0_points"]) + len(fx["s1_points"])]


def test_the_fixture_holds_what_it_promises(fx):
    assert os.path.getsize(os.path.join(HERE, "golden", "instshift.npz")) < 512 * 1024
    assert set(fx["forced_attr"].tolist()) == set(range(9))          # every attribute, a segment that drew nothing included
    pts, cols, labels, ids, off = batch_of(fx)
    tail = fx["tail"]
    assert 20 in labels and 20 not in tail                           # the ignored label
    for s in (0, 1):
        lab, iid = labels[off[s]:off[s + 1]], ids[off[s]:off[s + 1]]
        t_ids = {(int(l), int(i)) for l, i in zip(lab, iid) if l in tail}
        assert any((3, i) in {(int(l), int(j)) for l, j in zip(lab, iid)} for _, i in t_ids)      # a non-tail label shares an id
        assert any(sum(1 for l, j in t_ids if j == i) >= 2 for _, i in t_ids)                      # one id under two tail labels
        sizes = [len(rows) for _, _, rows in ir.segments(lab, iid, tail)]
        assert 1 in sizes and len(sizes) == (fx["forced_keys"][:, 0] == s).sum()                   # a one-point segment
    hue = {(int(k[0]), int(k[1]), int(k[2])) for k, a in zip(fx["forced_keys"], fx["forced_attr"]) if 1 <= a <= 4}
    for s, l, i in hue:               # grey rows and rows with a 255 channel inside every hue-shifted segment that has a few rows
        c = cols[off[s]:off[s + 1]][(labels[off[s]:off[s + 1]] == l) & (ids[off[s]:off[s + 1]] == i)]
        if len(c) >= 40:
            assert ((c[:, 0] == c[:, 1]) & (c[:, 1] == c[:, 2])).any() and (c.max(1) == 255).any()
    assert any(len(cols[off[s]:off[s + 1]][(labels[off[s]:off[s + 1]] == l) & (ids[off[s]:off[s + 1]] == i)]) >= 40 for s, l, i in hue)


def test_restatement_played_back_equals_the_reference_outputs_exactly(fx):
    pts, cols, labels, ids, off = batch_of(fx)
    forced = (fx["forced_keys"], fx["forced_attr"], fx["forced_factor"])
    p, c, l2, i2, order, status = ir.instance_shifts(pts, cols, labels, ids, off, fx["tail"], forced=forced)
    assert status == [0, 0] and sorted(order.tolist()) == list(range(off[-1])) and np.array_equal(i2, ids[order])
    for s in (0, 1):
        at = slice(off[s], off[s + 1])
        assert np.array_equal(p[at], fx["s%d_out_points" % s])       # rows, points, colours, both label columns: bit for bit
        assert np.array_equal(c[at], fx["s%d_out_colors" % s])
        assert np.array_equal(l2[at], fx["s%d_out_labels" % s])
        assert ((order[at] >= off[s]) & (order[at] < off[s + 1])).all()      # a permutation inside the scene
    assert not np.array_equal(order, np.arange(off[-1])) and (l2[:, 1] > 0).any()
    # a segment the table does not list gets attribute 0 and still moves
    few = tuple(a[:3] for a in forced)
    _, _, l3, _, order3, _ = ir.instance_shifts(pts, cols, labels, ids, off, fx["tail"], forced=few)
    assert np.array_equal(order3, order) and set(l3[:, 1].tolist()) <= set(few[1].tolist()) | {0}


def test_closed_form_of_the_hue_shift_equals_shift_hue(fx):
    for k, attr in enumerate((1, 2, 3, 4)):                           # Red, Green, Blue, Yellow
        assert np.array_equal(ir.shift_colors(fx["hue_in"], attr), fx["hue_out"][k]), attr
        assert set(np.unique(fx["hue_out"][k]).tolist()) == {0.0, 255.0}
    c = np.array([[10, 200, 30], [7, 7, 7], [255, 0, 255]], np.float32)     # the intent: the set's channels get the max, the others the min
    assert ir.shift_colors(c, 4, hue_as_written=False).tolist() == [[200, 200, 10], [7, 7, 7], [255, 255, 0]]
    assert ir.shift_colors(c, 3, hue_as_written=False).tolist() == [[10, 10, 200], [7, 7, 7], [0, 0, 255]]


def test_draw_statistics_of_the_generator_path():
    """m = 100 000 synthetic segments, p_color = 0.5, p_scale = 0.2: every observed count within FOUR binomial standard deviations,
    sd = sqrt(m p (1 - p)), of m p for p = p_color, (1 - p_color) p_scale, and of an even split over the six colour directions and
    the two scale directions (conditional on the number of colour / scale draws)."""
    m, p_color, p_scale = 100000, 0.5, 0.2
    rng = np.random.default_rng(11)
    labels, ids = rng.choice([5, 8, 14, 1 << 33], m), rng.integers(0, 1 << 31, m)
    attr = ir.draw_many((0x1234 << 32) | 0x9abcdef0, 77, labels, ids, p_color, p_scale)

    def within(count, total, p):
        sd = np.sqrt(total * p * (1 - p))
        print("count %d of %d, expected %.1f: %.2f sd" % (count, total, total * p, abs(count - total * p) / sd))
        return abs(count - total * p) <= 4.0 * sd
    n_color, n_scale = int(((attr >= 1) & (attr <= 6)).sum()), int((attr >= 7).sum())
    assert within(n_color, m, p_color) and within(n_scale, m, (1 - p_color) * p_scale)
    for a in range(1, 7):
        assert within(int((attr == a).sum()), n_color, 1 / 6)
    assert within(int((attr == 7).sum()), n_scale, 0.5)
    # the vector form is the scalar form; a decision is a function of (seed, scene seed, label, id)
    for j in range(50):
        assert ir.draw((0x1234 << 32) | 0x9abcdef0, 77, int(labels[j]), int(ids[j]), p_color, p_scale)[0] == attr[j]
    assert not np.array_equal(ir.draw_many((0x1234 << 32) | 0x9abcdef0, 78, labels, ids, p_color, p_scale), attr)
    assert not np.array_equal(ir.draw_many((0x1235 << 32) | 0x9abcdef0, 77, labels, ids, p_color, p_scale), attr)


def _chain(seed=0, **kw):
    from languagegroundedsemseg_amd.augment import DeviceAugmentation
    return DeviceAugmentation(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)),
                              scale_bound=(0.9, 1.1), rotation_axis="z", seed=seed, **kw)


class _Dataset:
    VOXEL_SIZE, CLIP_BOUND, ROTATION_AXIS, IS_TEMPORAL = 0.02, None, "z", False
    ELASTIC_DISTORT_PARAMS = ((0.2, 0.4), (0.8, 1.6))
    ROTATION_AUGMENTATION_BOUND = ((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi))
    SCALE_AUGMENTATION_BOUND = (0.9, 1.1)


class _Config:
    data_aug_color_trans_ratio, data_aug_color_jitter_std, data_aug_color_scaling_factor = 0.1, 0.05, 1.0
    normalize_color, data_aug_patch_dropout_ratio, elastic_distortion = True, 0.35, True
    instance_augmentation, instance_augmentation_color_aug_prob, instance_augmentation_scale_aug_prob = "raw", 0.4, 0.3


def test_refusals_by_name():
    from languagegroundedsemseg_amd import augment
    shifts = augment.InstanceShifts([5, 8, 14])
    assert (shifts.color_prob, shifts.scale_prob, shifts.hue_as_written, shifts.tail_labels) == (0.5, 0.2, True, [5, 8, 14])
    with pytest.raises(NotImplementedError, match="instance_augmentation.*instance_shifts="):      # the keyword stays refused, with a hint
        _chain(instance_augmentation="raw")
    bank = augment.InstanceBank.__new__(augment.InstanceBank)
    bank.categories = np.array([2])
    paste = augment.TailInstancePaste(bank, [2], [1.0])
    with pytest.raises(NotImplementedError, match="instance_shifts together with tail_instances"):
        _chain(instance_shifts=shifts, tail_instances=paste)
    host = (torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), [0, 4])
    with pytest.raises(ValueError, match="instances="):              # a missing instances=
        _chain(instance_shifts=shifts)(*host)
    with pytest.raises(RuntimeError, match="HIP tensor"):            # and no CPU path
        _chain(instance_shifts=shifts)(*host, instances=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.instance_shifts(host[0], host[1], host[2], host[2], [0, 4], [5], 0.5, 0.2)
    with pytest.raises(ValueError, match="tail_labels"):             # more than 256 tail labels
        augment.InstanceShifts(range(257))
    assert len(augment.InstanceShifts(list(range(256)) * 2).tail_labels) == 256      # (distinct ones count)
    for kw in (dict(color_prob=1.5), dict(scale_prob=-0.1), dict(seg_cap=0), dict(seg_cap=65537)):
        with pytest.raises(ValueError, match="color_prob|seg_cap"):
            augment.InstanceShifts([5], **kw)
    with pytest.raises(ValueError, match="InstanceShifts"):
        _chain(instance_shifts=[5, 8])
    # from_dataset: 'raw' without tail_labels is refused by name, with them it builds the stage from the config's probabilities
    with pytest.raises(NotImplementedError, match="tail_labels"):
        augment.DeviceAugmentation.from_dataset(_Dataset, _Config)
    aug = augment.DeviceAugmentation.from_dataset(_Dataset, _Config, tail_labels=[14, 5])
    assert (aug.shifts.tail_labels, aug.shifts.color_prob, aug.shifts.scale_prob) == ([5, 14], 0.4, 0.3)

    class Latent(_Config):
        instance_augmentation = "latent"

    class Off(_Config):
        instance_augmentation = None
    for cfg in (Latent, Off):                                         # as before: no stage
        assert augment.DeviceAugmentation.from_dataset(_Dataset, cfg).shifts is None
        assert augment.DeviceAugmentation.from_dataset(_Dataset, cfg, tail_labels=[5]).shifts is None


def test_draw_is_unchanged_by_instance_shifts():
    from languagegroundedsemseg_amd import augment
    plain, shifted = _chain(seed=5, coordinate_shift=True, dropout=0.2), _chain(seed=5, coordinate_shift=True, dropout=0.2,
                                                                                  instance_shifts=augment.InstanceShifts([5, 8]))
    for batch in (4, 7):                                              # the first and the second draw of each chain
        p, q = plain.draw(batch), shifted.draw(batch)
        assert [f.name for f in dataclasses.fields(p)] == [f.name for f in dataclasses.fields(q)]
        for f in dataclasses.fields(p):
            a, b = getattr(p, f.name), getattr(q, f.name)
            assert (a is None and b is None) or np.array_equal(a, b), f.name


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    W = L.lgs_instance_shift_workspace_bytes
    assert W(1000, 0, 64) == 0 and W(1000, 33, 64) == 0 and W(-1, 4, 64) == 0 and W((1 << 31) - 1, 4, 64) == 0
    assert W(1000, 4, 0) == 0 and W(1000, 4, 65537) == 0
    # (a good shape is sized with rocPRIM's temporary for the row sort, which asks the device: tests/test_gpu_instshift.py)
    tail, seeds, fake = (ctypes.c_int64 * 257)(), (ctypes.c_int32 * 33)(), 256      # fake: a non-null address that is never dereferenced

    def call(n=10, b=2, n_tail=3, p_color=0.5, p_scale=0.2, forced=(None, None, None, 0), seg_cap=64, off=fake, bounds=fake, ws=fake,
             rows=fake, out=fake, status=fake, tail_p=tail):
        return L.lgs_instance_shift(rows, rows, rows, rows, n, off, b, bounds, tail_p, n_tail, p_color, p_scale, 0, seeds, forced[0], forced[1],
                                    forced[2], forced[3], 1, seg_cap, ws, out, out, out, out, out, status, None)
    cases = {"b = 0": dict(b=0), "b = 33": dict(b=33), "n < 0": dict(n=-1), "n = 2^31 - 1": dict(n=(1 << 31) - 1),
             "seg_cap = 0": dict(seg_cap=0), "seg_cap = 65537": dict(seg_cap=65537), "257 tail labels": dict(n_tail=257),
             "null tail labels": dict(tail_p=None), "p_color > 1": dict(p_color=1.5), "p_scale NaN": dict(p_scale=float("nan")),
             "forced without keys": dict(forced=(None, fake, fake, 2)), "forced without factors": dict(forced=(fake, fake, None, 2)),
             "null offsets": dict(off=None), "null bounds": dict(bounds=None), "null workspace": dict(ws=None),
             "null rows": dict(rows=None), "null outputs": dict(out=None), "null status": dict(status=None)}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc != 0 and b"lgs_instance_shift" in L.lgs_last_error(), what
        with pytest.raises(RuntimeError, match="lgs_instance_shift"):
            engine.check(rc)
    assert engine.LGS_INSTSHIFT_MAX_TAIL == 256 and engine.LGS_INSTSHIFT_MAX_CAP == 65536
