"""CPU-side checks of the device RandomDropout (no GPU): the restatement's count rule (tests/dropout_reference.py) against the counts
the reference's two RandomDropout classes returned (tests/golden/dropout_counts.npz, written by tests/golden/make_dropout_fixtures.py),
the uniformity of the selection rule on the restatement, DeviceAugmentation.draw with and without dropout, and the argument handling
of the Python layer and the C-ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dropout_reference as dr

HERE = os.path.dirname(os.path.abspath(__file__))


def test_count_rule_equals_every_recorded_reference_count():
    fx = dict(np.load(os.path.join(HERE, "golden", "dropout_counts.npz")))
    assert len(fx["n"]) == 2 * 3 * 301 * 2 and set(fx["which"].tolist()) == {0, 1}
    assert sorted(set(fx["ratio"].tolist())) == [0.2, 0.3, 0.5] and fx["n"].min() == 0 and fx["n"].max() == 300
    for ratio, n, applied, returned in zip(fx["ratio"].tolist(), fx["n"].tolist(), fx["applied"].tolist(), fx["returned"].tolist()):
        assert returned == (dr.keep_count(n, ratio) if applied else n), (ratio, n, applied, returned)
    assert fx["applied"].sum() * 2 == len(fx["n"])                    # every n has a case that applied and one that did not
    # the restatement's select returns that many rows too, with and without the apply bit
    for n in (0, 1, 2, 5, 299):
        rows, off = dr.select([0, n, 2 * n], [True, False], 0.2, seed=3, scene_seeds=[1, 2])
        assert off == [0, dr.keep_count(n, 0.2), dr.keep_count(n, 0.2) + n] and len(rows) == off[-1]
    assert dr.keep_count(1, 0.2) == 0 and dr.keep_count(5, 0.2) == 4 and dr.keep_count(10, 0.3) == 7


def test_selection_rule_is_uniform_on_the_restatement():
    """n = 40, ratio 0.2 (k = 32), 2048 scenes: every row's inclusion frequency within 4 sd of 0.8, sd = sqrt(0.8 * 0.2 / 2048)"""
    n, trials, seed = 40, 2048, 0x0123456789abcdef
    hits = np.zeros(n, np.int64)
    for t in range(trials):
        rows, off = dr.select([0, n], [True], 0.2, seed=seed, scene_seeds=[(t * 2654435761 + 12345) % (1 << 32)])
        assert off == [0, 32] and len(rows) == 32 and len(set(rows.tolist())) == 32 and np.all(np.diff(rows) > 0)
        hits[rows] += 1
    sd = np.sqrt(0.8 * 0.2 / trials)
    dev = np.abs(hits / trials - 0.8) / sd
    print("largest deviation of a row's inclusion frequency from 0.8: %.2f sd" % dev.max())
    assert dev.max() <= 4.0


def _chain(seed=0, **kw):
    from languagegroundedsemseg_amd.augment import DeviceAugmentation
    return DeviceAugmentation(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)),
                              scale_bound=(0.9, 1.1), rotation_axis="z", seed=seed, **kw)


FIELDS = ("elastic", "flip_axes", "autocontrast", "blend", "translate", "translation", "jitter", "angles", "order", "scale", "matrices",
          "scene_seeds", "shift", "rotations")


def test_draw_streams_with_and_without_dropout():
    plain, drop, again = _chain(seed=5, coordinate_shift=True), _chain(seed=5, coordinate_shift=True, dropout=0.2), None
    for batch in (4, 7):                                              # the first draw of each chain, then a second one
        p, q = plain.draw(batch), drop.draw(batch)
        assert p.dropout is None and q.dropout.shape == (batch,) and q.dropout.dtype == bool
        if batch == 4:                 # the first plan: every pre-existing field is what the chain without dropout draws
            for f in FIELDS:
                assert np.array_equal(getattr(p, f), getattr(q, f)), f
            assert p.seed == q.seed
            again = _chain(seed=5, coordinate_shift=True, dropout=0.2).draw(batch)
            assert np.array_equal(again.dropout, q.dropout) and again.seed == q.seed      # reproducible
    n = 20000
    d = _chain(seed=9, dropout=0.3, dropout_position="first").draw(n).dropout
    assert abs(d.sum() - 0.3 * n) <= 5 * np.sqrt(n * 0.3 * 0.7)        # the application probability IS the ratio
    from languagegroundedsemseg_amd.augment import AugmentPlan
    import dataclasses
    assert {f.name: f.default for f in dataclasses.fields(AugmentPlan)}["dropout"] is None


def test_python_layer_refuses_bad_arguments_by_name():
    from languagegroundedsemseg_amd import augment
    off = torch.tensor([0, 4], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.random_dropout_rows(off, 4, [True])
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.random_dropout(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64),
                               scene_offsets=off, apply=[True])
    for ratio in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            augment.random_dropout_rows(off, 4, [True], ratio=ratio)
        with pytest.raises(ValueError, match="dropout"):
            _chain(dropout=ratio)
    with pytest.raises(ValueError, match="dropout_position"):
        _chain(dropout=0.2, dropout_position="middle")
    with pytest.raises(NotImplementedError, match="random_dropout"):          # the old keyword stays refused
        _chain(random_dropout=0.2)
    with pytest.raises(RuntimeError, match="HIP tensor"):                     # the chain itself still has no CPU path
        _chain(dropout=0.2)(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), [0, 4])


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    assert L.lgs_dropout_workspace_bytes(1000, 0) == 0 and L.lgs_dropout_workspace_bytes(1000, 33) == 0
    assert L.lgs_dropout_workspace_bytes(-1, 4) == 0 and L.lgs_dropout_workspace_bytes((1 << 40) + 1, 4) == 0
    small, big = L.lgs_dropout_workspace_bytes(0, 1), L.lgs_dropout_workspace_bytes(1 << 20, 32)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    seeds = (ctypes.c_int32 * 33)()
    fake = 256            # a non-null address that is never dereferenced: every case below is refused on the host
    cases = {"b = 33": (fake, 10, 33, 1, 0.8, fake, fake, fake), "b = 0": (fake, 10, 0, 1, 0.8, fake, fake, fake),
             "keep = 0": (fake, 10, 2, 1, 0.0, fake, fake, fake), "keep > 1": (fake, 10, 2, 1, 1.5, fake, fake, fake),
             "keep NaN": (fake, 10, 2, 1, float("nan"), fake, fake, fake), "n < 0": (fake, -1, 2, 1, 0.8, fake, fake, fake),
             "null offsets": (None, 10, 2, 1, 0.8, fake, fake, fake), "null workspace": (fake, 10, 2, 1, 0.8, None, fake, fake),
             "null rows": (fake, 10, 2, 1, 0.8, fake, None, fake), "null offsets_out": (fake, 10, 2, 1, 0.8, fake, fake, None)}
    for what, (off, n, b, mask, keep, ws, rows, out) in cases.items():
        rc = L.lgs_dropout_select(off, n, b, mask, keep, 0, seeds, None, None, ws, rows, out, None)
        assert rc != 0 and b"lgs_dropout_select" in L.lgs_last_error(), what
        with pytest.raises(RuntimeError, match="lgs_dropout_select"):
            engine.check(rc)


class _InssegDataset:
    VOXEL_SIZE, CLIP_BOUND, ROTATION_AXIS, IS_TEMPORAL = 0.05, None, "z", False
    ELASTIC_DISTORT_PARAMS = ((0.2, 0.4), (0.8, 1.6))
    ROTATION_AUGMENTATION_BOUND = ((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi))
    SCALE_AUGMENTATION_BOUND = (0.9, 1.1)


class _InssegConfig:
    class augmentation:
        data_aug_color_trans_ratio, data_aug_color_jitter_std, normalize_color = 0.1, 0.05, True


def test_constructors_for_the_two_recipes():
    from languagegroundedsemseg_amd.augment import DeviceAugmentation
    aug = DeviceAugmentation.from_insseg_dataset(_InssegDataset, _InssegConfig, seed=1)
    assert aug.dropout == 0.2 and aug.dropout_position == "first" and aug.voxel_size == 0.05 and aug.upright == 2
    assert aug.elastic_params == ((0.2, 0.4), (0.8, 1.6)) and aug.color_scale == 1.0 and aug.normalize_color and aug.coordinate_shift
    assert aug.color_trans_ratio == 0.1 and aug.color_jitter_std == 0.05 and aug.scale_bound == (0.9, 1.1)
    assert aug.draw(3).dropout.shape == (3,)

    class NoElastic(_InssegDataset):
        ELASTIC_DISTORT_PARAMS = None
    assert DeviceAugmentation.from_insseg_dataset(NoElastic, _InssegConfig).elastic_params == ()

    class Clipped(_InssegDataset):
        CLIP_BOUND = 4.0
    with pytest.raises(NotImplementedError, match="clip_bound"):
        DeviceAugmentation.from_insseg_dataset(Clipped, _InssegConfig)

    class Config:                     # the main recipe's configuration in which the reference adds RandomDropout (lib/dataset.py:385)
        data_aug_color_trans_ratio, data_aug_color_jitter_std, data_aug_color_scaling_factor = 0.1, 0.05, 1.0
        normalize_color, data_aug_patch_dropout_ratio, elastic_distortion = True, 0.0, True
    with pytest.raises(NotImplementedError, match="random_dropout"):          # unchanged without the new keyword ...
        DeviceAugmentation.from_dataset(_InssegDataset, Config)
    aug = DeviceAugmentation.from_dataset(_InssegDataset, Config, dropout=0.2)      # ... and reachable with it
    assert aug.dropout == 0.2 and aug.dropout_position == "last"
