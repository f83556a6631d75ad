"""CPU-side checks of the device augmentation chain's yardsticks (no GPU): the float64 restatement (tests/augment_reference.py)
against the reference's recorded outputs (tests/golden/augment.npz), the error budget the GPU tests use, the edge-corrected T^2
weights against scipy, DeviceAugmentation.draw, and the numpy Philox-4x32-10 against the published known-answer vectors.

    python tests/test_augment_cpu.py --write      regenerates tests/golden/augment_budget.json from the fixture"""
import json
import os
import sys

import numpy as np
import pytest
import scipy.ndimage

import augment_reference as ar

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "augment.npz")
BUDGET = os.path.join(HERE, "golden", "augment_budget.json")
STAGES = ((0.2, 0.4), (0.8, 1.6))
MARGIN = 4          # a different summation order over 125 taps and 8 corners
FLOOR_ULPS = 2      # never below 2 float32 ulp at the largest magnitude involved


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def reference_deviation(fx):
    """max |reference's float32 output - float64 restatement| per family, and the largest magnitude involved"""
    dev = {"elastic": 0.0, "colour": 0.0}
    mag = {"elastic": 0.0, "colour": 255.0}
    for s in (0, 1):
        pre = "s%d_" % s
        cur = fx[pre + "points"]
        for stage, (g, m) in enumerate(STAGES, 1):
            want = fx[pre + "e%d_out" % stage]
            got = ar.elastic_stage(cur, fx[pre + "e%d_noise" % stage], g, m)
            dev["elastic"] = max(dev["elastic"], float(np.abs(got - want.astype(np.float64)).max()))
            mag["elastic"] = max(mag["elastic"], float(np.abs(want).max()))
            cur = want                       # stage 2 starts from the reference's own stage-1 output: nothing compounds
        chain = ar.color_chain(fx[pre + "colors"], blend=fx[pre + "auto_draws"][1],
                               translation=(fx[pre + "trans_rand"] - 0.5) * 255 * 2 * 0.1,
                               jitter_std=0.05, jitter_noise=fx[pre + "jitter_randn"])
        for key in ("auto", "trans", "jitter"):
            dev["colour"] = max(dev["colour"], float(np.abs(chain[key] - fx[pre + key + "_out"].astype(np.float64)).max()))
    return dev, mag


def compute_budgets(fx):
    dev, mag = reference_deviation(fx)
    out = {}
    for k in dev:
        floor = FLOOR_ULPS * ar.ulp32(mag[k])
        out[k] = {"reference_deviation": dev[k], "largest_magnitude": mag[k], "floor": floor, "budget": max(MARGIN * dev[k], floor)}
    return out


def test_restatement_reproduces_every_recorded_reference_output(fx):
    dev, mag = reference_deviation(fx)
    print("reference vs float64 restatement, max abs:", dev)
    # the reference rounds to float32 after every transform (and blurs in float32): a few ulp at the magnitudes involved, no more
    assert dev["elastic"] <= 4 * ar.ulp32(mag["elastic"]), dev
    assert dev["colour"] <= 4 * ar.ulp32(255.0), dev
    for s in (0, 1):
        pre = "s%d_" % s
        # noise_dim as the reference computed it (the shape of what it asked randn for), also at the 3-cell axis
        assert tuple(ar.noise_dims(fx[pre + "points"], 0.2)) == fx[pre + "e1_noise"].shape[:3]
        assert tuple(ar.noise_dims(fx[pre + "e1_out"], 0.8)) == fx[pre + "e2_noise"].shape[:3]
        draws = fx[pre + "flip_draws"]
        axes = [a for a, d in zip((0, 1), draws[1:]) if d < 0.5]
        assert draws[0] < 0.95 and axes
        assert np.array_equal(ar.flip(fx[pre + "vox"], axes), fx[pre + "flip_out"])
    assert fx["s1_e2_noise"].shape[2] == 3


def test_error_budget_is_computed_and_stored(fx):
    got = compute_budgets(fx)
    stored = json.load(open(BUDGET))
    print("budgets:", json.dumps(got, indent=1))
    for k in ("elastic", "colour"):
        for field in ("reference_deviation", "largest_magnitude", "floor", "budget"):
            assert stored[k][field] == pytest.approx(got[k][field], rel=1e-9), (k, field)
        assert got[k]["budget"] >= FLOOR_ULPS * ar.ulp32(got[k]["largest_magnitude"])
        assert got[k]["budget"] <= 16 * ar.ulp32(got[k]["largest_magnitude"])          # float32-level, not a loose bound


@pytest.mark.parametrize("shape", [(3, 3, 3), (4, 3, 5), (3, 4, 4), (7, 5, 3), (6, 9, 4), (11, 4, 8)])
def test_t2_weights_equal_two_rounds_of_zero_padded_box_blurs(shape):
    rng = np.random.default_rng(sum(shape))
    noise = rng.standard_normal(shape + (3,))
    want = noise
    bx, by, bz = np.ones((3, 1, 1, 1)) / 3, np.ones((1, 3, 1, 1)) / 3, np.ones((1, 1, 3, 1)) / 3
    for _ in range(2):
        for k in (bx, by, bz):
            want = scipy.ndimage.convolve(want, k, mode="constant", cval=0)
    got = ar.elastic_field(noise)
    assert np.abs(got - want).max() <= 1e-14
    for d in set(shape):
        t = (np.eye(d) + np.eye(d, k=1) + np.eye(d, k=-1)) / 3
        assert np.abs(ar.t2_weights(d) - t @ t).max() <= 1e-15
        if d >= 5:
            assert np.allclose(ar.t2_weights(d)[2, :5] * 9, [1, 2, 3, 2, 1])
        assert ar.t2_weights(d)[0, 0] * 9 == 2 and ar.t2_weights(d)[0, 1] * 9 == 2 and ar.t2_weights(d)[0, 2] * 9 == 1


def _augmentation(seed=0, **kw):
    from languagegroundedsemseg_amd.augment import DeviceAugmentation
    return DeviceAugmentation(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)),
                              scale_bound=(0.9, 1.1), rotation_axis="z", color_trans_ratio=0.1, color_jitter_std=0.05, seed=seed, **kw)


def test_draw_frequencies_bounds_matrix_and_determinism():
    n = 20000
    aug = _augmentation(seed=11)
    p = aug.draw(n)

    def within(count, prob):
        assert abs(count - n * prob) <= 5 * np.sqrt(n * prob * (1 - prob)), (count, prob)
    within(p.elastic.sum(), 0.95)
    within((p.flip_axes & 1 != 0).sum(), 0.95 * 0.5)
    within((p.flip_axes & 2 != 0).sum(), 0.95 * 0.5)
    within(((p.flip_axes & 3) != 0).sum(), 0.95 * 0.75)
    assert not (p.flip_axes & 4).any()                      # the upright axis is never flipped
    within(p.autocontrast.sum(), 0.2)
    within(p.translate.sum(), 0.95)
    within(p.jitter.sum(), 0.95)
    assert p.blend.min() >= 0 and p.blend.max() < 1 and abs(p.blend.mean() - 0.5) < 5 / np.sqrt(12 * n)
    assert np.abs(p.translation).max() <= 255 * 0.1 and np.abs(p.translation.mean(0)).max() < 5 * (255 * 0.2 / np.sqrt(12)) / np.sqrt(n)
    assert np.abs(p.angles[:, :2]).max() <= np.pi / 64 and np.abs(p.angles[:, 2]).max() <= np.pi and np.abs(p.angles[:, 2]).max() > 3.0
    assert p.scale.min() >= 0.9 / 0.02 and p.scale.max() <= 1.1 / 0.02
    assert len({tuple(o) for o in p.order}) == 6            # every multiplication order occurs
    r = p.matrices[:, :3, :3] / p.scale[:, None, None]
    assert np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(r) - 1).max() < 1e-12
    assert np.all(p.matrices[:, 3] == [0, 0, 0, 1]) and np.all(p.matrices[:, :3, 3] == 0)
    assert len(set(p.scene_seeds.tolist())) > 0.99 * n and (p.shift == 0).all()
    # one scene, by hand: M_r @ M_v with the three axis rotations multiplied in the drawn order (lib/voxelizer.py:44-74)
    from scipy.linalg import expm
    rots = [expm(np.cross(np.eye(3), np.eye(3)[a] * p.angles[5, a])) for a in range(3)]
    want = rots[p.order[5, 0]] @ rots[p.order[5, 1]] @ rots[p.order[5, 2]] * p.scale[5]
    assert np.abs(p.matrices[5, :3, :3] - want).max() < 1e-12
    q = _augmentation(seed=11).draw(n)
    for f in ("elastic", "flip_axes", "autocontrast", "blend", "translate", "translation", "jitter", "angles", "order", "scale", "matrices",
              "scene_seeds", "shift"):
        assert np.array_equal(getattr(p, f), getattr(q, f)), f
    assert p.seed == q.seed and _augmentation(seed=12).draw(4).seed != p.seed
    s = _augmentation(seed=3, coordinate_shift=True).draw(2).shift
    assert s.shape == (3,) and s.min() >= 0 and s.max() < 100


def test_out_of_scope_arguments_are_refused_by_name():
    for name, value in (("random_dropout", 0.2), ("hue_saturation", (0.5, 0.2)), ("clip_bound", 4.0), ("instance_augmentation", {}),
                        ("num_pairs", 2)):
        with pytest.raises(NotImplementedError, match="num_pairs|" + name):
            _augmentation(**{name: value})

    class Dataset:
        VOXEL_SIZE, CLIP_BOUND, ROTATION_AXIS = 0.02, None, "z"
        ELASTIC_DISTORT_PARAMS = ((0.2, 0.4), (0.8, 1.6))
        ROTATION_AUGMENTATION_BOUND = ((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi))
        SCALE_AUGMENTATION_BOUND = (0.9, 1.1)

    class Config:
        data_aug_color_trans_ratio, data_aug_color_jitter_std, data_aug_color_scaling_factor = 0.1, 0.05, 1.0
        normalize_color, data_aug_patch_dropout_ratio, elastic_distortion = True, 0.35, True
    from languagegroundedsemseg_amd.augment import DeviceAugmentation
    aug = DeviceAugmentation.from_dataset(Dataset, Config)
    assert aug.voxel_size == 0.02 and aug.elastic_params == ((0.2, 0.4), (0.8, 1.6)) and aug.normalize_color and aug.upright == 2
    Config.data_aug_patch_dropout_ratio = 0.0              # the configuration in which the reference adds RandomDropout
    with pytest.raises(NotImplementedError, match="random_dropout"):
        DeviceAugmentation.from_dataset(Dataset, Config)


def test_host_tensors_raise_without_a_gpu():
    import torch
    from languagegroundedsemseg_amd import augment
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.elastic_distortion(torch.zeros(4, 3), [0, 4], 0.2, 0.4, seed=1)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.horizontal_flip(torch.zeros(4, 4, dtype=torch.int32), [1])
    with pytest.raises(RuntimeError, match="HIP tensor"):
        augment.chromatic_augment(torch.zeros(4, 3), [0, 4], [augment.ColorParams()])
    with pytest.raises(RuntimeError, match="HIP tensor"):
        _augmentation()(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), [0, 4])


def test_philox_restatement_matches_the_known_answer_vectors():
    """The three philox4x32_10 vectors of Random123's known-answer file (counter, key -> output).  No second copy of that file exists
    next to this repository; the vectors are written here as published, and the device generator is held to this restatement in
    tests/test_gpu_augment.py.  (A restatement that reproduces 384 published bits did not get there by accident.)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = ar.philox4x32_10(np.asarray([ctr], np.uint64), key[0], key[1])[0]
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # vectorised over counters = one at a time
    ctr = np.arange(40, dtype=np.uint64).reshape(10, 4)
    many = ar.philox4x32_10(ctr, 7, 9)
    assert all(np.array_equal(many[i], ar.philox4x32_10(ctr[i:i + 1], 7, 9)[0]) for i in range(10))
    z = ar.elastic_noise((6, 5, 4), seed=(5 << 32) | 17, scene_seed=99, stage=1)
    assert z.shape == (6, 5, 4, 3) and np.isfinite(z).all() and abs(z.mean()) < 0.3 and 0.7 < z.std() < 1.3


if __name__ == "__main__":
    if "--write" in sys.argv:
        budgets = compute_budgets(dict(np.load(FIXTURE)))
        with open(BUDGET, "w") as f:
            json.dump(budgets, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(budgets, indent=1, sort_keys=True))
