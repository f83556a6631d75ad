"""Instance evaluation on the host: tests/insteval_reference.py and insteval.InstanceEvaluator on CPU tensors against
tests/golden/insteval.npz, which the reference's own Evaluator produced (tests/golden/make_insteval_fixtures.py); merge_dual_set against
the literal loop of the trainer's nms; the container's round trip; the refusals; the knob."""
import os

import numpy as np
import pytest
import torch

import insteval_reference as ref
from languagegroundedsemseg_amd import insteval
from languagegroundedsemseg_amd.insteval import InstanceEvaluator, Proposals, instance_overlaps, merge_dual_set

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "insteval.npz")
LABELS = ["c%d" % i for i in range(1, 7)]
N_SCENES = 3


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def ref_result(fx):
    scenes = [(ref.tables(fx["s%d_member" % k], fx["s%d_offsets" % k], fx["s%d_gt_ids" % k], fx["valid_class_ids"]),
               fx["s%d_label_id" % k], fx["s%d_conf" % k]) for k in range(N_SCENES)]
    return scenes, ref.evaluate(scenes, fx["valid_class_ids"])


def proposals_of(fx, k, device="cpu"):
    p = fx["s%d_offsets" % k].shape[0] - 1
    return Proposals(torch.from_numpy(fx["s%d_member" % k]).to(device), torch.from_numpy(fx["s%d_offsets" % k]).to(device),
                     torch.full((p,), -1, dtype=torch.int64, device=device), torch.from_numpy(fx["s%d_label_id" % k]).to(device),
                     torch.from_numpy(fx["s%d_conf" % k]).to(device), fx["s%d_gt_ids" % k].shape[0])


def check_ap(ap, fx, points):
    """NaN positions equal; |delta| <= 4 K 2^-53 with K the curve points of the class: the bound of a float64 dot product of K terms that
    are each at most 1"""
    want = fx["ap"]
    assert ap.shape == want.shape == (6, 10) and ap.dtype == np.float64
    assert np.array_equal(np.isnan(ap), np.isnan(want))
    err = np.abs(np.where(np.isnan(want), 0.0, ap - want))
    print("max |ap - reference| = %.3g, curve points up to %d" % (err.max(), points.max()))
    assert np.all(err <= 4 * np.maximum(points, 1) * 2.0 ** -53), err.max()


def check_tables_against_reference_records(t, fx, k):
    """the table entries the reference's assign_instances_for_scan looked at: vert_count, void_intersection, every matched pair, every
    ground-truth instance, as integers"""
    kept = fx["s%d_ref_pred" % k]
    assert np.array_equal(t["size"][kept], fx["s%d_ref_vert_count" % k])
    assert np.array_equal(t["prop_void"][kept], fx["s%d_ref_void" % k])
    gt = fx["s%d_ref_gt" % k]
    order = np.argsort(gt[:, 0])
    assert np.array_equal(t["gt_id"], gt[order, 0]) and np.array_equal(t["gt_count"], gt[order, 1])
    pairs = {(int(q), int(g)): int(i) for q, g, i in fx["s%d_ref_match" % k]}
    cls = fx["s%d_label_id" % k]
    for q in kept:
        for gi, g in enumerate(t["gt_id"]):
            if g // 1000 == cls[q]:
                assert t["inter"][q, gi] == pairs.get((int(q), int(g)), 0), (q, g)
    assert np.array_equal(t["prop_void"] + t["inter"].sum(1), t["size"])


def test_reference_module_equals_the_fixture(fx, ref_result):
    scenes, (ap, points) = ref_result
    for k, (t, _, _) in enumerate(scenes):
        check_tables_against_reference_records(t, fx, k)
    check_ap(ap, fx, points)


def sorted_tables(t, p):
    """OverlapTables -> the layout of insteval_reference.tables (slots sorted by id, unused ones dropped)"""
    gt_id, gt_count = t.gt_id.cpu().numpy(), t.gt_count.cpu().numpy().astype(np.int64)
    used = np.nonzero(gt_count > 0)[0]
    used = used[np.argsort(gt_id[used])]
    return {"gt_id": gt_id[used], "gt_count": gt_count[used], "inter": t.inter.cpu().numpy().astype(np.int64)[:, used],
            "prop_void": t.prop_void.cpu().numpy().astype(np.int64), "size": np.diff(p.offsets.cpu().numpy()).astype(np.int64)}


def test_instance_overlaps_on_cpu_tensors_equals_the_reference_module(fx, ref_result):
    scenes, _ = ref_result
    for k in range(N_SCENES):
        p = proposals_of(fx, k)
        t = instance_overlaps(p, torch.from_numpy(fx["s%d_gt_ids" % k]), fx["valid_class_ids"], g_cap=64)
        assert int(t.status) == 0 and t.inter.shape == (len(p), 64) and t.inter.dtype == torch.int32
        got = sorted_tables(t, p)
        for key in ("gt_id", "gt_count", "inter", "prop_void"):
            assert np.array_equal(got[key], scenes[k][0][key]), key
        check_tables_against_reference_records(got, fx, k)
    small = instance_overlaps(proposals_of(fx, 0), fx["s0_gt_ids"], fx["valid_class_ids"], g_cap=4)      # more ids than slots: flagged
    assert int(small.status) & 1


@pytest.mark.parametrize("form", ["proposals", "dict"])
def test_evaluator_on_cpu_equals_the_fixture(fx, ref_result, form):
    ev = InstanceEvaluator(LABELS, fx["valid_class_ids"])
    for k in range(N_SCENES):
        p = proposals_of(fx, k)
        if form == "proposals":
            ev.add_gt(torch.from_numpy(fx["s%d_gt_ids" % k]), "scene%d" % k)
            ev.add_prediction(p, "scene%d" % k)
        else:
            ev.add_prediction(p.to_instances(), k)          # the reference's order: prediction first, numpy ground truth
            ev.add_gt(fx["s%d_gt_ids" % k], k)
    all_ap, ap50, ap25 = ev.evaluate()
    check_ap(ev.ap, fx, ref_result[1][1])
    # a mean of at most 54 numbers in [0, 1], each within 4 K 2^-53 (K <= 8 here) of the reference's: 64 2^-53 covers terms and sum
    assert np.allclose([all_ap, ap50, ap25], fx["avgs"], rtol=0, atol=64 * 2.0 ** -53)
    assert [ev.avgs[k] for k in ("all_ap", "all_ap_50%", "all_ap_25%")] == [all_ap, ap50, ap25]
    got = np.array([[ev.avgs["classes"][n][k] for k in ("ap", "ap50%", "ap25%")] for n in LABELS])
    assert np.array_equal(np.isnan(got), np.isnan(fx["class_avgs"]))
    assert np.allclose(got, fx["class_avgs"], rtol=0, atol=64 * 2.0 ** -53, equal_nan=True)


def test_evaluator_names_the_scene_of_a_set_status_bit(fx):
    ev = InstanceEvaluator(LABELS, fx["valid_class_ids"], g_cap=4)
    ev.add_gt(fx["s0_gt_ids"], "scene0000_00")
    ev.add_prediction(proposals_of(fx, 0), "scene0000_00")
    with pytest.raises(RuntimeError, match="scene0000_00.*g_cap"):
        ev.evaluate()
    ev = InstanceEvaluator(LABELS, fx["valid_class_ids"])
    ev.add_prediction(proposals_of(fx, 0), "lonely")
    with pytest.raises(KeyError, match="lonely"):
        ev.evaluate()


def nms_loop(instances, instances_):
    out, counter = {}, 0
    for key in instances:
        if instances[key]["label_id"].item() not in [10, 12, 16]:
            out[counter] = instances[key]
            counter += 1
    for key in instances_:
        if instances_[key]["label_id"].item() in [10, 12, 16]:
            out[counter] = instances_[key]
            counter += 1
    return out


def random_proposals(seed, n=500, p=12):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, 40, (p,), generator=g)
    member = torch.cat([torch.randperm(n, generator=g)[:s] for s in sizes]).int()
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(sizes, 0)]).int()
    label = torch.randint(0, 6, (p,), generator=g)
    label_id = torch.tensor([3, 10, 12, 16, 24, 39])[label]
    return Proposals(member, offsets, label, label_id, torch.rand(p, generator=g), n)


def assert_same_instances(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k]["pred_mask"], b[k]["pred_mask"]) and int(a[k]["label_id"]) == int(b[k]["label_id"])
        assert np.asarray(a[k]["conf"]).tobytes() == np.asarray(b[k]["conf"]).tobytes()


def test_merge_dual_set_is_the_trainers_nms():
    a, b = random_proposals(1), random_proposals(2)
    merged = merge_dual_set(a, b)
    want = nms_loop(a.to_instances(), b.to_instances())
    assert 0 < len(want) < len(a) + len(b)
    assert_same_instances(merged.to_instances(), want)
    assert merged.offsets[-1] == merged.member.shape[0] and merged.label.shape[0] == len(want)
    with pytest.raises(ValueError):
        merge_dual_set(a, random_proposals(3, n=400))


def test_proposals_round_trip_through_the_dict():
    p = random_proposals(4)
    inst = p.to_instances()
    assert inst[0]["pred_mask"].dtype == np.int32 and inst[0]["pred_mask"].shape == (500,) and inst[0]["conf"].dtype == np.float32
    back = Proposals.from_instances(inst)
    order = [torch.sort(p.member[p.offsets[q]:p.offsets[q + 1]])[0] for q in range(len(p))]      # the dict holds masks: ascending members
    assert torch.equal(back.member, torch.cat(order)) and torch.equal(back.offsets, p.offsets) and back.n_points == 500
    assert torch.equal(back.label_id, p.label_id) and torch.equal(back.conf, p.conf) and back.member.dtype == torch.int32
    assert_same_instances(back.to_instances(), inst)
    assert len(Proposals.from_instances({})) == 0


def test_refusals_name_what_they_refuse(fx):
    p = proposals_of(fx, 0)
    with pytest.raises(ValueError, match="valid class id 0 < 1"):
        instance_overlaps(p, fx["s0_gt_ids"], [0, 1, 2])
    with pytest.raises(ValueError, match="valid class id -3 < 1"):
        InstanceEvaluator(["a", "b"], [2, -3])
    with pytest.raises(ValueError, match="g_cap = 4097"):
        instance_overlaps(p, fx["s0_gt_ids"], fx["valid_class_ids"], g_cap=4097)
    with pytest.raises(ValueError, match="g_cap = 8192"):
        InstanceEvaluator(LABELS, fx["valid_class_ids"], g_cap=8192)
    from languagegroundedsemseg_amd.pointgroup import Clustering
    cl = Clustering(ignored_labels=[0], class_mapping=torch.arange(7), score_func=torch.median, device="cpu")
    with pytest.raises(NotImplementedError, match="median.*get_instances"):
        cl.get_proposals(np.zeros((4, 3), np.float32), torch.zeros(4, 7))


def test_the_knob_is_listed():
    from languagegroundedsemseg_amd import engine, tuning
    rows = {name: (d, v) for name, d, v, _ in engine.tuning_table()}
    assert rows["INST_EVAL_FUSED"][0] == 1
    assert any(name == "INST_EVAL_FUSED" for _, name, _, _, _ in tuning.describe())
    with engine.tuning(INST_EVAL_FUSED=0):
        assert engine.tuning_get("INST_EVAL_FUSED") == 0
    assert engine.tuning_get("INST_EVAL_FUSED") == rows["INST_EVAL_FUSED"][1]
    assert insteval.MAX_G_CAP == 4096
