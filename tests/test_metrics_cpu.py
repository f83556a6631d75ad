"""Segmentation metrics on the CPU (languagegroundedsemseg_amd/metrics.py): the meter's torch lines, the derived numbers, the
reference-signature wrappers, the null-argument refusal of lgs_seg_metrics and the two-rank sum.  Every expected value comes from
the numpy restatements in this file (np.bincount(n * label[k] + pred[k]), the formulas of lib/utils.py:92-109), never from the
code under test."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from languagegroundedsemseg_amd.metrics import SegmentationMeter, confusion_metrics, fast_hist, per_class_iu


# ---- numpy restatements
def np_confmat(pred, label, c, ignore):
    pred, label = np.asarray(pred), np.asarray(label)
    k = (label != ignore) & (label >= 0) & (label < c)
    return np.bincount(c * label[k].astype(np.int64) + pred[k], minlength=c * c).reshape(c, c)


def np_ratio(num, den, present):
    out = np.full(num.shape, np.nan)
    out[present] = 0.0
    ok = den > 0
    out[ok] = num[ok] / den[ok]
    return out


def np_metrics(cm, groups=None):
    cm = cm.astype(np.float64)
    d, r, c = np.diag(cm), cm.sum(1), cm.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = d / (r + c - d)
    out = {"iou": iou, "precision": np_ratio(d, c, (r + c) > 0), "recall": np_ratio(d, r, (r + c) > 0), "count": cm.sum()}
    out["miou"], out["precision_macro"], out["recall_macro"] = np.nanmean(iou), np.nanmean(out["precision"]), np.nanmean(out["recall"])
    if groups is not None:
        for g, name in enumerate(("head", "common", "tail")):
            ids = np.nonzero(groups[:, g])[0]
            sub = np.zeros_like(cm)
            sub[ids] = cm[ids]                              # the rows the reference's split_items[:, g] selects
            ds, rs, cs = np.diag(sub), sub.sum(1), sub.sum(0)
            out[name + "_precision"] = np_ratio(ds, cs, (rs + cs) > 0)
            out[name + "_recall"] = np_ratio(ds, rs, (rs + cs) > 0)
            out[name + "_precision_mean"] = np.nanmean(out[name + "_precision"][ids])
            out[name + "_recall_mean"] = np.nanmean(out[name + "_recall"][ids])
            out[name + "_miou"] = np.nanmean(iou[ids])
    return out


def assert_metrics(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


# ---- the hand-made 5-class case: class 4 is absent from labels and predictions, class 3 is labelled but never predicted
LABELS = np.array([0, 0, 1, 1, 2, 2, 3, 3, 0, 1, -1, 7, 2, 0], np.int64)
PREDS = np.array([0, 1, 1, 1, 2, 0, 0, 1, 0, 2, 2, 0, 2, 0], np.int64)
GROUPS = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]], bool)


def scores_for(preds, c, seed=0):
    """scores whose row maximum sits at preds[i]"""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((len(preds), c)).astype(np.float32)
    s[np.arange(len(preds)), preds] = 10.0 + rng.random(len(preds)).astype(np.float32)
    return torch.from_numpy(s)


def test_hand_made_case_against_numpy():
    m = SegmentationMeter(5, ignore_label=-1)
    x = scores_for(PREDS, 5)
    pred, prob = m.update(x, torch.from_numpy(LABELS), want_prob=True)
    assert pred.dtype == torch.int64 and np.array_equal(pred.numpy(), PREDS)
    np.testing.assert_allclose(prob.double().numpy(), torch.softmax(x.double(), 1).numpy(), atol=1e-6)
    cm = np_confmat(PREDS, LABELS, 5, -1)
    assert m.confmat.dtype == torch.int64 and np.array_equal(m.confmat.numpy(), cm)
    assert cm.sum() == 12                                   # the ignored row and the out-of-range label 7 add nothing
    got = m.compute(groups=torch.from_numpy(GROUPS))
    assert_metrics(got, np_metrics(cm, GROUPS))
    # the two cases the definitions name
    assert torch.isnan(got["iou"][4]) and torch.isnan(got["precision"][4]) and torch.isnan(got["recall"][4])
    assert got["iou"][3] == 0 and got["precision"][3] == 0 and got["recall"][3] == 0
    assert int(got["count"]) == 12
    assert_metrics(m.compute(), np_metrics(cm))
    assert_metrics(confusion_metrics(m.confmat), np_metrics(cm))


def test_pred_follows_torch_max_on_ties_nan_and_inf():
    x = torch.zeros(5, 7)
    x[0, 2] = x[0, 5] = 3.0                                 # tie -> lowest index
    x[1, 4] = float("nan"); x[1, 1] = float("nan"); x[1, 6] = 9.0      # first NaN
    x[2] = float("-inf")                                    # -> 0
    x[3, 3] = x[3, 6] = float("inf")
    m = SegmentationMeter(7)
    pred = m.update(x, torch.tensor([2, 1, 0, 3, -1]))
    assert pred.tolist() == [2, 1, 0, 3, 0] == torch.max(x, 1)[1].tolist()
    assert np.array_equal(m.confmat.numpy(), np_confmat(pred.numpy(), [2, 1, 0, 3, -1], 7, -1))


def test_out_of_range_labels_and_a_non_negative_ignore_label():
    rng = np.random.default_rng(3)
    c, n = 300, 4000                                         # ignore_label 255 is a class index here
    preds = rng.integers(0, c, n)
    labels = rng.integers(-3, c + 3, n)
    labels[rng.random(n) < 0.2] = 255
    m = SegmentationMeter(c, ignore_label=255)
    pred = m.update(scores_for(preds, c, 1), torch.from_numpy(labels))
    assert np.array_equal(pred.numpy(), preds)
    cm = np_confmat(preds, labels, c, 255)
    assert np.array_equal(m.confmat.numpy(), cm)
    assert cm[255].sum() == 0 and cm.sum() == ((labels != 255) & (labels >= 0) & (labels < c)).sum()


def test_sparse_tensor_input():
    import MinkowskiEngine as ME
    from oracle.backend import OracleBackend
    prev = ME.set_backend(OracleBackend("torch"))
    try:
        coords = torch.tensor([[0, i, 0, 0] for i in range(len(PREDS))], dtype=torch.int32)
        st = ME.SparseTensor(scores_for(PREDS, 5), coords)
        m = SegmentationMeter(5)
        pred = m.update(st, torch.from_numpy(LABELS))
    finally:
        ME.set_backend(prev)
    assert np.array_equal(pred.numpy(), PREDS) and np.array_equal(m.confmat.numpy(), np_confmat(PREDS, LABELS, 5, -1))


def test_two_updates_equal_one_update_on_the_concatenation_and_reset():
    rng = np.random.default_rng(5)
    c = 11
    preds, labels = rng.integers(0, c, 500), rng.integers(-1, c, 500)
    x, t = scores_for(preds, c, 2), torch.from_numpy(labels)
    a, b = SegmentationMeter(c), SegmentationMeter(c)
    a.update(x[:123].requires_grad_(True), t[:123])          # recording or not: update() detaches
    with torch.no_grad():
        a.update(x[123:], t[123:])
    b.update(x, t)
    assert torch.equal(a.confmat, b.confmat) and np.array_equal(b.confmat.numpy(), np_confmat(preds, labels, c, -1))
    a.reset()
    assert a.confmat.shape == (c, c) and int(a.confmat.abs().sum()) == 0
    a.update(x, t)
    assert torch.equal(a.confmat, b.confmat)


def test_confmat_is_a_buffer_that_moves_with_the_module():
    m = SegmentationMeter(4)
    assert "confmat" in dict(m.named_buffers()) and "confmat" in m.state_dict()
    m.update(scores_for([1, 2], 4), torch.tensor([1, 3]))
    m2 = m.to("meta")
    assert m2.confmat.device.type == "meta" and m2.confmat.dtype == torch.int64
    m3 = SegmentationMeter(4).double()                       # float casts leave the integer buffer alone
    assert m3.confmat.dtype == torch.int64


def test_fast_hist_and_per_class_iu_are_the_reference_formulas():
    rng = np.random.default_rng(7)
    n = 9
    pred, label = rng.integers(0, n, 2000), rng.integers(-2, n + 2, 2000)
    label[label == 5] = 6                                    # class 5 never labelled ...
    pred[pred == 5] = 4                                      # ... nor predicted: 0/0
    k = (label >= 0) & (label < n)                           # lib/utils.py:92-94
    want = np.bincount(n * label[k].astype(int) + pred[k], minlength=n ** 2).reshape(n, n)
    assert np.array_equal(fast_hist(pred, label, n), want)
    ht = fast_hist(torch.from_numpy(pred), torch.from_numpy(label), n)
    assert torch.is_tensor(ht) and np.array_equal(ht.numpy(), want)
    with np.errstate(divide="ignore", invalid="ignore"):     # lib/utils.py:102-104
        iu = np.diag(want) / (want.sum(1) + want.sum(0) - np.diag(want))
    assert np.isnan(iu[5])
    np.testing.assert_allclose(per_class_iu(want), iu, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(per_class_iu(ht).numpy(), iu, rtol=1e-12, equal_nan=True)


def test_null_arguments_are_refused_without_a_gpu():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    assert "lgs_seg_metrics" in engine.EXPORTS
    rc = L.lgs_seg_metrics(None, 5, 5, None, -1, None, None, None, engine.LGS_F32, None)
    assert rc != 0 and b"lgs_seg_metrics" in L.lgs_last_error()
    rc = L.lgs_seg_metrics(None, 0, 5, None, -1, None, None, None, engine.LGS_F32, None)      # no rows, but no matrix either
    assert rc != 0 and b"lgs_seg_metrics" in L.lgs_last_error()
    assert engine.lib().lgs_abi_version() == 18              # a new symbol only


def test_the_knob_is_in_the_tuning_table():
    from languagegroundedsemseg_amd import engine, tuning
    rows = {n: d for n, d, _, _ in engine.tuning_table()}
    assert rows["METRICS_BLOCKS"] >= 1
    assert any(name == "METRICS_BLOCKS" for _, name, _, _, _ in tuning.describe())


# ---- two ranks (gloo), in the manner of tests/test_ddp_cpu.py
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_data():
    rng = np.random.default_rng(11)
    c, n = 5, 600
    preds, labels = rng.integers(0, 4, n), rng.integers(-1, 4, n)      # class 4 stays absent
    return c, scores_for(preds, c, 4), torch.from_numpy(labels), preds, labels


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c, x, t, _, _ = _two_rank_data()
        half = slice(0, 250) if rank == 0 else slice(250, None)
        m = SegmentationMeter(c)
        m.update(x[half], t[half])
        local = m.confmat.clone()
        out = m.compute(groups=torch.from_numpy(GROUPS))
        grp = m.compute(groups=torch.from_numpy(GROUPS), process_group=dist.group.WORLD)
        ret[rank] = ({k: v.numpy() for k, v in out.items()}, {k: v.numpy() for k, v in grp.items()}, local.numpy(), m.confmat.numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_compute_the_sum_and_keep_their_local_buffers():
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    c, x, t, preds, labels = _two_rank_data()
    want = np_metrics(np_confmat(preds, labels, c, -1), GROUPS)
    single = SegmentationMeter(c)
    single.update(x, t)
    assert_metrics(single.compute(groups=torch.from_numpy(GROUPS)), want)
    for rank, half in ((0, slice(0, 250)), (1, slice(250, None))):
        out, grp, before, after = ret[rank]
        assert_metrics(out, want)
        assert_metrics(grp, want)
        assert np.array_equal(before, after) and np.array_equal(after, np_confmat(preds[half], labels[half], c, -1))
