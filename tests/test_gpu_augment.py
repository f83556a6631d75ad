"""The device augmentation chain (languagegroundedsemseg_amd/augment.py, csrc/lgs_augment.hip) against the float64 restatement
(tests/augment_reference.py) within the budget computed by tests/test_augment_cpu.py (tests/golden/augment_budget.json), and bit for
bit wherever the work is integer or index work.  Shapes are chosen for where the kernels can break, not for the workload."""
import json
import os

import numpy as np
import pytest
import torch

import augment_reference as ar
from languagegroundedsemseg_amd import augment
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = ((0.2, 0.4), (0.8, 1.6))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "augment.npz")))


@pytest.fixture(scope="module")
def budget():
    b = json.load(open(os.path.join(HERE, "golden", "augment_budget.json")))
    return {k: v["budget"] for k, v in b.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def two_scenes(fx, key):
    a, b = fx["s0_" + key], fx["s1_" + key]
    return np.concatenate([a, b]), [0, len(a), len(a) + len(b)]


# ---- bounds
def test_bounds_fp32_and_int32_bit_equal_to_numpy():
    sizes = [1, 257, 0, 4099]                         # one row, a workgroup and a row, an EMPTY scene in the middle, 16 workgroups and 3
    off = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((off[-1], 3)) * 50).astype(np.float32)
    x[1:258, 0] = -np.abs(x[1:258, 0])                # scene 1, column 0: all negative ...
    x[100, 0] = -0.0                                  # ... so that -0.0 is its maximum
    x[258 + 7, 1] = x[258 + 4000, 1] = x[258:, 1].max()      # a tie for the maximum
    x[300, 2], x[301, 2] = 0.0, -0.0                  # both zeros inside a column that spans them
    got, _ = augment.aug_bounds(dev(x), dev(off.astype(np.int64)))
    got = got.cpu().numpy()
    for s in (0, 1, 3):
        rows = x[off[s]:off[s + 1]]
        want = np.concatenate([rows.min(0), rows.max(0)])
        assert np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), (s, got[s], want)
    assert np.signbit(got[1, 3]) and got[1, 3] == 0                      # max of scene 1, column 0 is -0.0, bit for bit
    assert np.all(got[2, :3] == np.inf) and np.all(got[2, 3:] == -np.inf)        # the empty scene
    # where a column's extreme is a zero of either sign, numpy's answer depends on its reduction order; the key order is -0.0 < +0.0
    z = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -1.0]], np.float32)
    gz = augment.aug_bounds(dev(z), dev(np.array([0, 2], np.int64)))[0].cpu().numpy()[0]
    assert np.signbit(gz[0]) and np.signbit(gz[1]) and not np.signbit(gz[3]) and not np.signbit(gz[4]) and gz[2] == -1 and gz[5] == 1
    # int32 [n, 4]: the scene id is column 0, the offsets are derived on the device
    c = rng.integers(-2 ** 31, 2 ** 31, (off[-1], 4), dtype=np.int64).astype(np.int32)
    c[:, 0] = np.repeat(np.arange(4), sizes)
    gi, goff = augment.aug_bounds(dev(c), batch_size=4)
    gi = gi.cpu().numpy()
    assert np.array_equal(goff.cpu().numpy(), off)
    for s in (0, 1, 3):
        rows = c[off[s]:off[s + 1], 1:]
        assert np.array_equal(gi[s], np.concatenate([rows.min(0), rows.max(0)]))
    assert np.all(gi[2, :3] == 2 ** 31 - 1) and np.all(gi[2, 3:] == -2 ** 31)
    # trailing and leading empty scenes, and an empty table
    c2 = c[off[1]:off[2]].copy()
    _, o2 = augment.aug_bounds(dev(c2), batch_size=4)
    assert o2.cpu().tolist() == [0, 0, 257, 257, 257]
    _, o3 = augment.aug_bounds(torch.zeros((0, 4), dtype=torch.int32, device=DEV), batch_size=3)
    assert o3.cpu().tolist() == [0, 0, 0, 0]


# ---- elastic, teacher-forced noise
def test_elastic_teacher_forced_both_scenes_in_one_call_within_budget(fx, budget):
    pts, off = two_scenes(fx, "points")
    cur = dev(pts)
    for stage, (g, m) in enumerate(STAGES, 1):
        noise = [fx["s%d_e%d_noise" % (s, stage)] for s in (0, 1)]
        before = cur.cpu().numpy()
        cur, state = augment.elastic_distortion(cur, off, g, m, seed=0, noise=noise, return_state=True)
        got = cur.cpu().numpy()
        assert augment.aug_status(state["status"]) == []
        for s in (0, 1):
            rows = slice(off[s], off[s + 1])
            # stage 2 against the restatement applied to the DEVICE's stage-1 output: nothing compounds
            want = ar.elastic_stage(before[rows], noise[s], g, m)
            err = float(np.abs(got[rows].astype(np.float64) - want).max())
            print("stage %d scene %d: max |device - float64 restatement| = %.3e (budget %.3e), displacement up to %.3f"
                  % (stage, s, err, budget["elastic"], np.abs(want - before[rows]).max()))
            assert np.abs(want - before[rows]).max() > 0.01            # the stage moved the points
            assert err <= budget["elastic"]
            # the bounds the stage leaves for the next one are those of the displaced cloud, bit for bit
            b = state["bounds"][0][s].cpu().numpy()
            assert np.array_equal(b, np.concatenate([got[rows].min(0), got[rows].max(0)]))
    assert fx["s1_e2_noise"].shape[2] == 3                                # the noise_dim == 3 axis was part of it


def test_elastic_grid_larger_than_max_cells_leaves_the_scene_alone_and_sets_its_bit(fx):
    pts, off = two_scenes(fx, "points")
    noise = [fx["s0_e1_noise"], fx["s1_e1_noise"]]
    cells = [int(np.prod(n.shape[:3])) for n in noise]
    assert cells[1] < cells[0]
    out, state = augment.elastic_distortion(dev(pts), off, 0.2, 0.4, seed=0, noise=[None, noise[1]], max_cells=cells[1], return_state=True)
    got = out.cpu().numpy()
    assert augment.aug_status(state["status"]) == [0]
    assert np.array_equal(got[:off[1]].view(np.uint32), pts[:off[1]].view(np.uint32))        # scene 0 bit-identical
    want = ar.elastic_stage(pts[off[1]:], noise[1], 0.2, 0.4)
    assert np.abs(got[off[1]:] - want).max() < 1e-5 and np.abs(got[off[1]:] - pts[off[1]:]).max() > 0.01


# ---- device noise
def test_device_noise_is_a_function_of_seeds_and_scene_alone(fx):
    a, b = fx["s0_points"][:700], fx["s1_points"][:300]
    pts = np.concatenate([b, b[:5], a])
    off = [0, 300, 305, 1005]
    seeds = [11, 22, 33]
    kw = dict(seed=(9 << 32) | 1234, max_cells=20000, return_state=True)
    o1, s1 = augment.elastic_distortion(dev(pts), off, 0.2, 0.4, scene_seeds=seeds, **kw)
    o2, s2 = augment.elastic_distortion(dev(pts), off, 0.2, 0.4, scene_seeds=seeds, **kw)
    assert torch.equal(o1, o2)
    for s in range(3):                      # the used part of each scene's slot (the rest of a slot is never written)
        used = int(np.prod(ar.noise_dims(pts[off[s]:off[s + 1]], 0.2))) * 3
        assert torch.equal(s1["noise"][0][s, :used], s2["noise"][0][s, :used]) and torch.equal(s1["field"][0][s, :used], s2["field"][0][s, :used])
    # the third scene alone, with its own seed: the same field and the same points, bit for bit
    oa, sa = augment.elastic_distortion(dev(a), [0, 700], 0.2, 0.4, scene_seeds=[33], **kw)
    dims = ar.noise_dims(a, 0.2)
    n = int(np.prod(dims)) * 3
    assert torch.equal(sa["field"][0][0, :n], s1["field"][0][2, :n]) and torch.equal(oa, o1[305:])
    assert not torch.equal(s1["noise"][0][0, :100], s1["noise"][0][2, :100])
    # another stage, scene seed or seed gives another field
    for change in (dict(stage=1), dict(scene_seeds=[34]), dict(seed=(9 << 32) | 1235), dict(seed=(10 << 32) | 1234)):
        args = dict(kw, scene_seeds=[33])
        args.update(change)
        _, sb = augment.elastic_distortion(dev(a), [0, 700], 0.2, 0.4, **args)
        assert not torch.equal(sb["noise"][0][0, :n], sa["noise"][0][0, :n]), change
    # the numbers are the restatement's: Philox words -> Box-Muller (device in fp32, restatement in float64)
    want = ar.elastic_noise(dims, (9 << 32) | 1234, 33, 0).reshape(-1)
    got = sa["noise"][0][0, :n].cpu().numpy()
    assert np.abs(got - want).max() < 2e-5 * max(1.0, np.abs(want).max())
    assert np.abs(sa["field"][0][0, :n].cpu().numpy() - ar.elastic_field(got.reshape(tuple(dims) + (3,))).reshape(-1)).max() < 1e-6


def test_device_noise_statistics_on_2_to_the_20_samples():
    # two points span a grid of 73 x 73 x 66 cells at granularity 0.2: 351 714 cells x 3 >= 2^20 samples
    pts = np.array([[0.0, 0.0, 0.0], [14.1, 14.1, 12.7]], np.float32)
    dims = ar.noise_dims(pts, 0.2)
    cells = int(np.prod(dims))
    assert cells * 3 >= 1 << 20
    _, st = augment.elastic_distortion(dev(pts), [0, 2], 0.2, 0.4, seed=77, scene_seeds=[5], max_cells=cells, return_state=True)
    assert augment.aug_status(st["status"]) == []
    z = st["noise"][0][0, :1 << 20].double()
    n = float(z.numel())
    assert bool(torch.isfinite(z).all())
    mean, var, tail = float(z.mean()), float(z.var()), float((z.abs() > 3).double().mean())
    p3 = 0.0026997960632601866
    print("mean %.5f  var %.5f  share beyond 3 sigma %.6f" % (mean, var, tail))
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert abs(tail - p3) <= 5 * np.sqrt(p3 * (1 - p3) / n)


def test_raw_philox_words_equal_the_numpy_restatement():
    ctr = np.array([[0, 0, 0, 0], [0xffffffff] * 4, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [1, 2, 3, 4], [70000, 2, 1, 9]], np.uint32)
    for key in (0, 0xffffffffffffffff, (0x299f31d0 << 32) | 0xa4093822, (33 << 32) | 1234):
        got = augment.philox_words(dev(ctr.view(np.int32)), key).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, ar.philox4x32_10(ctr, key & 0xffffffff, key >> 32)), hex(key)


# ---- batched voxelise
def test_voxelize_batched_bit_equal_to_the_oracle_per_scene():
    from test_quantize_cpu import _points, _rigid
    sizes = [3001, 1, 5000]
    pts = np.concatenate([_points(s, n=k + 3)[0][:k] - np.float32(1.5 * s) for s, k in enumerate(sizes)])       # negative coordinates too
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    mats = np.stack([_rigid(20 + s, voxel=0.02 + 0.01 * s) for s in range(3)])
    got = augment.voxelize_batched(dev(pts), off, mats, batch_base=2).cpu().numpy()
    assert (pts < 0).any() and (got[:, 1:] < 0).any()
    for s in range(3):
        want, _, _, _ = orc.quantize(pts[off[s]:off[s + 1]], mats[s], batch_index=2 + s)
        assert np.array_equal(got[off[s]:off[s + 1]], want), s
    # more than 32 scenes: the wrapper splits
    many = np.concatenate([[0], np.cumsum(np.full(40, 50))]).tolist()
    m40 = np.stack([_rigid(s, voxel=0.05) for s in range(40)])
    g40 = augment.voxelize_batched(dev(pts[:2000]), many, m40).cpu().numpy()
    for s in (0, 31, 32, 39):
        assert np.array_equal(g40[many[s]:many[s + 1]], orc.quantize(pts[many[s]:many[s + 1]], m40[s], batch_index=s)[0]), s


# ---- flip and shift
def test_flip_and_shift_bit_equal_to_numpy():
    rng = np.random.default_rng(3)
    sizes = [700, 301]
    c = rng.integers(-400, 500, (sum(sizes), 4)).astype(np.int32)
    c[:, 0] = np.repeat([0, 1], sizes)
    shift = [17, 0, -93]
    got = augment.horizontal_flip(dev(c), [3, 0], shift=shift, batch_size=2).cpu().numpy()      # x and y in scene 0, nothing in scene 1
    want = c.copy()
    want[:700, 1:] = ar.flip(c[:700, 1:], (0, 1))
    want[:, 1:] += np.asarray(shift, np.int32)
    assert (c[:, 1:] < 0).any() and (c[:, 1:] > 0).any() and np.array_equal(got, want)
    got = augment.horizontal_flip(dev(c), [[False, False, False], [False, True, False]]).cpu().numpy()
    want = c.copy()
    want[700:, 1:] = ar.flip(c[700:, 1:], (1,))
    assert np.array_equal(got, want)


# ---- colour
@pytest.mark.parametrize("normalize", [False, True])
def test_colour_teacher_forced_within_budget(fx, budget, normalize):
    cols, off = two_scenes(fx, "colors")
    noise, _ = two_scenes(fx, "jitter_randn")
    noise = noise.astype(np.float32)
    noise[:50] *= 40                                   # jitter of +-2 sigma x 40 x 12.75: values that clip at 0 and at 255
    tr = [(fx["s%d_trans_rand" % s] - 0.5).reshape(3) * 255 * 2 * 0.1 for s in (0, 1)]
    tr[1] = tr[1] * 0 + [300.0, -300.0, 5.0]           # a translation that clips whole channels
    scenes = [augment.ColorParams(blend=float(fx["s0_auto_draws"][1]), translation=tuple(tr[0]), jitter_std=0.05),
              augment.ColorParams(blend=None, translation=tuple(tr[1]), jitter_std=None)]
    scale = 1.0 if not normalize else 0.9
    got = augment.chromatic_augment(dev(cols), off, scenes, scale=scale, normalize=normalize, noise=dev(noise)).cpu().numpy()
    worst = 0.0
    for s, p in enumerate(scenes):
        rows = slice(off[s], off[s + 1])
        want = ar.color_chain(cols[rows], blend=p.blend, translation=p.translation, jitter_std=p.jitter_std, jitter_noise=noise[rows],
                              scale=scale, normalize=normalize)["final"]
        worst = max(worst, float(np.abs(got[rows] - want).max()))
        if s == 0 and not normalize:
            assert (want == 0).any() and (want == 255).any()
        if s == 1 and not normalize:
            assert (want[:, 0] == 255).all() and (want[:, 1] == 0).all()
    print("colour: max |device - float64 restatement| = %.3e (budget %.3e)" % (worst, budget["colour"]))
    assert worst <= budget["colour"] * (1.0 if not normalize else scale / 255)
    # the recorded reference outputs themselves (scene 0's chain is the reference's: same draws, same noise)
    if not normalize:
        ref = augment.chromatic_augment(dev(fx["s0_colors"]), [0, off[1]], [augment.ColorParams(blend=float(fx["s0_auto_draws"][1]),
                                        translation=tuple((fx["s0_trans_rand"] - 0.5).reshape(3) * 25.5 * 2), jitter_std=0.05)],
                                        noise=dev(fx["s0_jitter_randn"].astype(np.float32))).cpu().numpy()
        assert np.abs(ref - fx["s0_jitter_out"]).max() <= 2 * budget["colour"]


def test_colour_constant_channel_stays_finite_and_unblended(budget):
    rng = np.random.default_rng(8)
    cols = np.floor(rng.random((600, 3)) * 180 + 40).astype(np.float32)
    cols[:, 1] = 77.0                                   # hi == lo in channel 1: inf / NaN in the reference
    p = augment.ColorParams(blend=0.6, translation=None, jitter_std=None)
    got = augment.chromatic_augment(dev(cols), [0, 600], [p]).cpu().numpy()
    want = ar.color_chain(cols, blend=0.6, skip_constant_channels=True)["final"]
    assert np.isfinite(got).all() and np.array_equal(got[:, 1], cols[:, 1])
    assert np.abs(got - want).max() <= budget["colour"] and np.abs(got - cols).max() > 1        # the other channels were blended


def test_device_jitter_depends_on_the_row_within_its_scene_alone():
    cols = np.full((1000, 3), 128.0, np.float32)
    p = augment.ColorParams(jitter_std=0.05, seed=4)
    alone = augment.chromatic_augment(dev(cols[:400]), [0, 400], [p], seed=21)
    batch = augment.chromatic_augment(dev(cols), [0, 600, 1000], [augment.ColorParams(jitter_std=0.05, seed=3), p], seed=21)
    assert torch.equal(alone, batch[600:]) and not torch.equal(batch[:400], batch[600:])
    z = (batch.double() - 128) / 12.75
    assert abs(float(z.mean())) < 5 / np.sqrt(3000) and abs(float(z.var()) - 1) < 5 * np.sqrt(2 / 3000)


# ---- the chain
def test_chain_equals_the_restatement_stage_by_stage(fx, budget):
    pts, off = two_scenes(fx, "points")
    cols, _ = two_scenes(fx, "colors")
    labels, _ = two_scenes(fx, "labels")
    aug = augment.DeviceAugmentation(voxel_size=0.05, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
                                     normalize_color=True, coordinate_shift=True, seed=2)
    plan = aug.draw(2)
    plan.elastic[:] = True
    plan.flip_axes[:] = [1, 2]
    plan.autocontrast[:], plan.translate[:], plan.jitter[:] = [True, False], True, [True, True]
    noise = [[fx["s%d_e%d_noise" % (s, stage)] for s in (0, 1)] for stage in (1, 2)]
    rng = np.random.default_rng(0)
    jit = {}

    def jitter_noise(n):
        jit["z"] = rng.standard_normal((n, 3)).astype(np.float32)
        return dev(jit["z"])
    torch.cuda.synchronize()
    coords, feats, lab, state = aug(dev(pts), dev(cols), dev(labels), off, plan=plan, elastic_noise=noise, jitter_noise=jitter_noise,
                                    return_state=True)
    assert torch.cuda.get_sync_debug_mode() == 0                      # the call ran its pre-dedup part under "error" and restored the mode
    assert augment.aug_status(state["status"]) == []
    # elastic: each stage from the device's previous output
    before = pts
    for stage, (g, m) in enumerate(STAGES):
        got = state["stages"][stage].cpu().numpy()
        for s in (0, 1):
            rows = slice(off[s], off[s + 1])
            assert np.abs(got[rows] - ar.elastic_stage(before[rows], noise[stage][s], g, m)).max() <= budget["elastic"]
        before = got
    # voxelise + dedup: bit-equal to the oracle per scene on the device's displaced points
    want_c, want_keep = [], []
    for s in (0, 1):
        c, ui, _, _ = orc.quantize(before[off[s]:off[s + 1]], plan.matrices[s], batch_index=s)
        want_c.append(c[ui])
        want_keep.append(ui + off[s])
    keep = np.concatenate(want_keep)
    assert np.array_equal(state["keep"].cpu().numpy(), keep)
    # flip over the surviving voxel rows, then the batch shift
    for s, axes in ((0, (0,)), (1, (1,))):
        want_c[s][:, 1:] = ar.flip(want_c[s][:, 1:], axes) + plan.shift.astype(np.int32)
    assert np.array_equal(coords.cpu().numpy(), np.concatenate(want_c))
    assert np.array_equal(lab.cpu().numpy(), labels[keep])
    # colour over the surviving rows (lo / hi are those of the voxel rows)
    got_f = feats.cpu().numpy()
    at = 0
    for s in (0, 1):
        k = want_keep[s]
        want = ar.color_chain(cols[k], blend=plan.blend[s] if plan.autocontrast[s] else None, translation=plan.translation[s],
                              jitter_std=0.05, jitter_noise=jit["z"][at:at + len(k)], normalize=True)["final"]
        assert np.abs(got_f[at:at + len(k)] - want).max() <= budget["colour"] / 255
        at += len(k)
    assert at == got_f.shape[0] and 1000 < at <= len(pts)
    # Philox path end to end: runs, is deterministic under a fixed plan, and raises for host tensors
    a1 = aug(dev(pts), dev(cols), dev(labels), off, plan=plan)
    a2 = aug(dev(pts), dev(cols), dev(labels), off, plan=plan)
    assert all(torch.equal(x, y) for x, y in zip(a1, a2)) and bool(torch.isfinite(a1[1]).all())
    with pytest.raises(RuntimeError, match="HIP tensor"):
        aug(torch.from_numpy(pts), dev(cols), dev(labels), off, plan=plan)


def test_pre_dedup_part_runs_under_sync_debug_error(fx):
    """the functional forms up to the voxeliser, under the mode set from outside as well: no synchronising call"""
    pts, off = two_scenes(fx, "points")
    p = dev(pts)
    mats = np.stack([np.diag([20.0, 20.0, 20.0, 1.0])] * 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = augment.elastic_distortion(p, off, 0.2, 0.4, seed=5, scene_seeds=[1, 2])
        c = augment.voxelize_batched(out, off, mats)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert c.shape == (len(pts), 4) and not torch.equal(out, p)
