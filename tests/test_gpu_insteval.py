"""Instance evaluation on the engine: lgs_inst_overlap against tests/insteval_reference.py (the tables, exact) and torch
(the confidences), insteval.InstanceEvaluator on HIP tensors against the reference's own numbers (tests/golden/insteval.npz), and
Clustering.get_proposals against Clustering.get_instances."""

import numpy as np
import pytest
import torch

import insteval_reference as ref
from languagegroundedsemseg_amd import engine
from languagegroundedsemseg_amd.insteval import InstanceEvaluator, Proposals, instance_overlaps, proposal_conf
from languagegroundedsemseg_amd.pointgroup import Clustering
from test_gpu_cluster import _scene
from test_insteval_cpu import GOLDEN, LABELS, N_SCENES, check_ap, proposals_of, sorted_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1 << 20          # class ids that are multiples of 2^20: their instance ids collide under a multiplicative hash
SIZES = (1, 63, 64, 65, 257, 0, 1 << 30, 5)      # 0: an empty proposal between full ones; 1 << 30: all points (clipped to n)


def make_gt(n, g, seed):
    """n ids with g distinct ground-truth instances (when n allows), ids 0 / -1 / -5000 and two invalid classes in between"""
    rng = np.random.default_rng(seed)
    valid = np.array([3, 5] + [BIG * (k + 1) for k in range(g)], dtype=np.int64)
    k = np.arange(g)
    inst_ids = np.where(k % 2 == 1, BIG * (k + 1) * 1000, 3000 + k // 2)      # the odd ones: multiples of 2^20 * 1000, one class each
    assert np.unique(inst_ids).shape[0] == g and g <= 2000
    pool = np.concatenate([inst_ids, [0, -1, -5000, 7001, 4000, 999]])
    gt = pool[rng.integers(0, len(pool), n)]
    k = min(n, g)
    gt[rng.permutation(n)[:k]] = inst_ids[:k]                     # every id at least once where there is room
    return gt.astype(np.int64), valid


def make_proposals(n, seed, sizes=SIZES):
    rng = np.random.default_rng(seed)
    sizes = [min(s, n) for s in sizes]
    member = np.concatenate([rng.permutation(n)[:s] for s in sizes] + [np.zeros(0, np.int64)]).astype(np.int32)      # distinct inside a proposal, shared between them
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    p = len(sizes)
    return Proposals(torch.from_numpy(member).to(DEV), torch.from_numpy(offsets).to(DEV), torch.zeros(p, dtype=torch.int64, device=DEV),
                     torch.zeros(p, dtype=torch.int64, device=DEV), torch.zeros(p, device=DEV), n)


def assert_tables_equal(t, p, want):
    assert int(t.status) == 0
    got = sorted_tables(t, p)
    for key in ("gt_id", "gt_count", "inter", "prop_void"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["prop_void"] + got["inter"].sum(1), got["size"])
    return got


@pytest.mark.parametrize("n,g,g_cap", [(1, 1, 1), (33, 2, 8), (4099, 64, 64), (20011, 1024, 1024), (20011, 300, 4096)])
def test_tables_equal_the_reference_module(n, g, g_cap):
    gt, valid = make_gt(n, g, seed=n + g)
    p = make_proposals(n, seed=n)
    want = ref.tables(p.member.cpu().numpy(), p.offsets.cpu().numpy(), gt, valid)
    assert want["gt_id"].shape[0] == min(n, g) and want["size"].max() == n
    t = instance_overlaps(p, torch.from_numpy(gt).to(DEV), valid, g_cap=g_cap)
    assert t.inter.shape == (len(p), g_cap) and t.gt_id.shape == (g_cap,) and t.inter.is_cuda
    assert_tables_equal(t, p, want)
    with engine.tuning(INST_EVAL_FUSED=0):                          # the torch lines agree exactly
        assert_tables_equal(instance_overlaps(p, torch.from_numpy(gt).to(DEV), valid, g_cap=g_cap), p, want)
    again = instance_overlaps(p, torch.from_numpy(gt).to(DEV), valid, g_cap=g_cap)      # two calls: the same tables once the slots are sorted
    a, b = sorted_tables(t, p), sorted_tables(again, p)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_empty_inputs_launch_nothing_that_reads_null():
    gt, valid = make_gt(500, 5, seed=1)
    gt_d = torch.from_numpy(gt).to(DEV)
    none = make_proposals(500, 0, sizes=())                         # p == 0
    t = instance_overlaps(none, gt_d, valid, g_cap=16)
    assert t.inter.shape == (0, 16) and int(t.status) == 0 and int((t.gt_count > 0).sum()) == 5 and int(t.gt_count.sum()) == int(np.isin(gt, ref.tables([], [0], gt, valid)["gt_id"]).sum())
    hollow = make_proposals(500, 0, sizes=(0, 0, 0))                # m == 0
    t = instance_overlaps(hollow, gt_d, valid, g_cap=16)
    assert int(t.status) == 0 and not bool(t.inter.any()) and not bool(t.prop_void.any())
    conf = proposal_conf(hollow.member, hollow.offsets, torch.zeros(3, dtype=torch.int32, device=DEV), torch.randn(500, 4, device=DEV), "max")
    assert bool(torch.isnan(conf).all())
    t = instance_overlaps(make_proposals(0, 0, sizes=(0,)), torch.zeros(0, dtype=torch.int64, device=DEV), valid, g_cap=16)      # n == 0
    assert int(t.status) == 0 and not bool(t.gt_count.any()) and t.inter.shape == (1, 16)
    bad = make_proposals(500, 3, sizes=(40,))
    bad.member[7], bad.member[9] = 500, -1                          # members outside [0, n): flagged and skipped
    t = instance_overlaps(bad, gt_d, valid, g_cap=16)
    assert int(t.status) == 2 and int(t.prop_void.sum() + t.inter.sum()) == 38


def test_more_ids_than_slots_is_flagged_and_the_next_call_is_exact():
    g_cap = 16
    gt, valid = make_gt(3000, g_cap + 1, seed=9)
    p = make_proposals(3000, 9)
    t = instance_overlaps(p, torch.from_numpy(gt).to(DEV), valid, g_cap=g_cap)
    assert int(t.status) & 1
    ev = InstanceEvaluator(["k%d" % i for i in range(len(valid))], valid, g_cap=g_cap)
    ev.add_gt(torch.from_numpy(gt).to(DEV), "scene0042_00")
    ev.add_prediction(p, "scene0042_00")
    with pytest.raises(RuntimeError, match="scene0042_00.*more distinct"):
        ev.evaluate()
    want = ref.tables(p.member.cpu().numpy(), p.offsets.cpu().numpy(), gt, valid)
    assert_tables_equal(instance_overlaps(p, torch.from_numpy(gt).to(DEV), valid, g_cap=32), p, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [1, 20, 200])
def test_confidences(dtype, c):
    n = 20011
    g = torch.Generator().manual_seed(c)
    scores = (torch.randn(n, c, generator=g) * 3 - 4).to(dtype).to(DEV)      # mostly negative logits
    p = make_proposals(n, seed=c)
    col = torch.randint(0, c, (len(p),), generator=g).int().to(DEV)
    sizes = (p.offsets[1:] - p.offsets[:-1]).tolist()
    out = {mode: proposal_conf(p.member, p.offsets, col, scores, mode) for mode in ("max", "mean")}
    assert out["max"].dtype == out["mean"].dtype == torch.float32
    for q, size in enumerate(sizes):
        if size == 0:
            assert bool(torch.isnan(out["max"][q])) and bool(torch.isnan(out["mean"][q]))
            continue
        x = scores[p.member[p.offsets[q]:p.offsets[q + 1]].long(), col[q].long()]
        assert out["max"][q].view(torch.int32).item() == torch.max(x).float().view(torch.int32).item(), (q, size)
        # one fp32 rounding of the float64 mean, plus size 2^-53 mean|x| for the fp64 accumulation
        mean = float(x.double().mean())
        bound = 2.0 ** -24 * abs(mean) + 2.0 ** -149 + size * 2.0 ** -53 * float(x.double().abs().mean())
        err = abs(float(out["mean"][q]) - mean)
        print("size %5d  |mean - fp64 mean| = %.3g  bound %.3g" % (size, err, bound))
        assert err <= bound, (q, size, err, bound)
    for mode in ("max", "mean"):                                    # two calls: the same bits
        assert torch.equal(proposal_conf(p.member, p.offsets, col, scores, mode).view(torch.int32), out[mode].view(torch.int32))
    with engine.tuning(INST_EVAL_FUSED=0):
        assert torch.equal(proposal_conf(p.member, p.offsets, col, scores, "max").view(torch.int32), out["max"].view(torch.int32))


def test_evaluator_on_hip_tensors_equals_the_fixture():
    fx = dict(np.load(GOLDEN))
    scenes = [(ref.tables(fx["s%d_member" % k], fx["s%d_offsets" % k], fx["s%d_gt_ids" % k], fx["valid_class_ids"]),
               fx["s%d_label_id" % k], fx["s%d_conf" % k]) for k in range(N_SCENES)]
    _, points = ref.evaluate(scenes, fx["valid_class_ids"])
    results = []
    for knob in (1, 0):
        with engine.tuning(INST_EVAL_FUSED=knob):
            ev = InstanceEvaluator(LABELS, fx["valid_class_ids"])
            for k in range(N_SCENES):
                ev.add_gt(torch.from_numpy(fx["s%d_gt_ids" % k]).to(DEV), k)
                ev.add_prediction(proposals_of(fx, k, DEV), k)
                t = instance_overlaps(proposals_of(fx, k, DEV), torch.from_numpy(fx["s%d_gt_ids" % k]).to(DEV), fx["valid_class_ids"])
                assert_tables_equal(t, proposals_of(fx, k), scenes[k][0])
            results.append(ev.evaluate())
            check_ap(ev.ap, fx, points)
            assert np.allclose(results[-1], fx["avgs"], rtol=0, atol=64 * 2.0 ** -53)
    assert results[0] == results[1]


@pytest.mark.parametrize("score_func", [torch.max, torch.mean])
def test_get_proposals_equals_get_instances(score_func):
    xyz, sem = _scene(3)
    g = torch.Generator().manual_seed(3)
    scores = (torch.nn.functional.one_hot(torch.from_numpy(sem).long(), 7).float() * 6 + torch.randn(len(sem), 7, generator=g) - 3).to(DEV)
    cl = Clustering(ignored_labels=[0], class_mapping=torch.tensor([0, 3, 4, 10, 12, 16, 39]), thresh=0.03, min_points=30, propose_points=40,
                    score_func=score_func)
    want = cl.get_instances(xyz, scores)
    prop = cl.get_proposals(xyz, scores)
    got = prop.to_instances()
    assert len(want) > 3 and list(got) == list(want) and prop.member.is_cuda and prop.n_points == len(sem)
    assert torch.equal(prop.label_id.cpu(), cl.class_mapping.cpu()[prop.label.cpu()])
    for k in want:
        assert np.array_equal(got[k]["pred_mask"], want[k]["pred_mask"]) and int(got[k]["label_id"]) == int(want[k]["label_id"])
        if score_func is torch.max:
            assert got[k]["conf"].tobytes() == want[k]["conf"].astype(np.float32).tobytes()
        else:
            x = scores[torch.from_numpy(want[k]["pred_mask"]).bool().to(DEV), prop.label[k]].double()
            size, mean, mabs = x.shape[0], float(x.mean()), float(x.abs().mean())
            assert abs(float(got[k]["conf"]) - mean) <= 2.0 ** -24 * abs(mean) + size * 2.0 ** -53 * mabs
            assert abs(float(want[k]["conf"]) - mean) <= 2.0 ** -24 * abs(mean) + size * 2.0 ** -24 * mabs      # torch's fp32 sum, at its worst
    with pytest.raises(NotImplementedError, match="median"):
        Clustering(ignored_labels=[0], class_mapping=torch.arange(7), score_func=torch.median).get_proposals(xyz, scores)


def test_add_gt_and_add_prediction_do_not_synchronise():
    fx = dict(np.load(GOLDEN))
    ev = InstanceEvaluator(LABELS, fx["valid_class_ids"])
    gts = [torch.from_numpy(fx["s%d_gt_ids" % k]).to(DEV) for k in range(N_SCENES)]
    props = [proposals_of(fx, k, DEV) for k in range(N_SCENES)]
    ev.add_gt(gts[0], 0)                                            # warm-up: library load, the valid-class table, the pinned allocator
    ev.add_prediction(props[0], 0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in (1, 2):
            ev.add_gt(gts[k], k)
            ev.add_prediction(props[k], k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ev.evaluate()
    assert np.array_equal(np.isnan(ev.ap), np.isnan(fx["ap"])) and np.allclose(ev.ap, fx["ap"], rtol=0, atol=2.0 ** -48, equal_nan=True)
