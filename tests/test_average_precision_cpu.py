"""Per-class average precision without a GPU: the numpy reference (tests/ap_reference.py) against sklearn, the torch path of
metrics.average_precision against the reference, AveragePrecisionMeter, and the engine's new entry points as far as they go
without a device (exports, refusals).

Tolerance 4 N 2^-53 absolute: both sides are fp64 sums of at most N terms, each at most 1, divided by P_c."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ap_reference import ap_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tol(n):
    return 4 * max(n, 1) * 2.0 ** -53


def assert_ap(got, want, n):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    k = ~np.isnan(want)
    if k.any():
        err = np.abs(got[k] - want[k]).max()
        print("max |AP - reference| = %.3g (bound %.3g)" % (err, tol(n)))
        assert err <= tol(n)


def torch_ap(prob, target, **kw):
    from languagegroundedsemseg_amd.metrics import average_precision
    out = average_precision(prob, torch.as_tensor(target), **kw)
    assert out.dtype == torch.float64 and out.device.type == "cpu"
    return out.numpy()


def random_case(n, c, seed, levels=None, half_on_zero=False):
    rng = np.random.default_rng(seed)
    prob = rng.random((n, c)).astype(np.float32)
    prob /= prob.sum(1, keepdims=True)
    if levels:
        prob = (np.round(prob * c * (levels - 1) / 2).clip(0, levels - 1) / (levels - 1)).astype(np.float32)
    target = rng.integers(-1, c, n)
    if half_on_zero:
        target[rng.random(n) < 0.5] = 0
    return prob, target.astype(np.int64)


SK_CASES = [(33, 13, 4, False), (4099, 20, None, False), (4099, 20, None, True), (33, 13, None, True)]


@pytest.mark.parametrize("n,c,levels,half", SK_CASES)
def test_reference_equals_sklearn(n, c, levels, half):
    pytest.importorskip("sklearn")
    from sklearn.metrics import average_precision_score
    from sklearn.preprocessing import label_binarize
    prob, target = random_case(n, c, 7 * n + c, levels, half)
    if levels:
        assert len(np.unique(prob)) <= levels
    onehot = label_binarize(target, classes=np.arange(c))          # -1 rows become all-zero rows: negatives of every class
    ref = ap_reference(prob, target)
    present = [k for k in range(c) if (target == k).any()]
    assert present and np.isnan(ref[[k for k in range(c) if k not in present]]).all()
    sk = np.array([average_precision_score(onehot[:, k], prob[:, k].astype(np.float64)) for k in present])
    assert_ap(ref[present], sk, n)


@pytest.mark.parametrize("n,c,levels,half", SK_CASES)
def test_torch_path_equals_reference(n, c, levels, half):
    prob, target = random_case(n, c, 11 * n + c, levels, half)
    assert_ap(torch_ap(torch.from_numpy(prob), target), ap_reference(prob, target), n)


def test_class_without_positive_is_nan_and_all_positive_is_one():
    rng = np.random.default_rng(0)
    prob = rng.random((17, 3)).astype(np.float32)
    target = np.full(17, 1, dtype=np.int64)                       # every row a positive of class 1
    got = torch_ap(torch.from_numpy(prob), target)
    assert np.isnan(got[0]) and np.isnan(got[2]) and got[1] == 1.0
    assert_ap(got, ap_reference(prob, target), 17)


@pytest.mark.parametrize("k", [1, 2, 5, 9])
def test_single_positive_ranked_kth_gives_one_over_k(k):
    n = 9
    prob = np.zeros((n, 2), dtype=np.float32)
    prob[:, 0] = np.linspace(0.9, 0.1, n)                          # strictly falling: row i is ranked (i + 1)-th
    prob[:, 1] = 1 - prob[:, 0]
    target = np.full(n, 1, dtype=np.int64)
    target[k - 1] = 0
    got = torch_ap(torch.from_numpy(prob), target)
    assert got[0] == 1.0 / k
    assert_ap(got, ap_reference(prob, target), n)


def test_all_scores_equal_gives_the_class_frequency():
    n, c = 40, 4
    prob = np.full((n, c), 0.25, dtype=np.float32)
    target = (np.arange(n) % 5 - 1).astype(np.int64)               # 8 rows each of -1, 0, 1, 2, 3
    got = torch_ap(torch.from_numpy(prob), target)
    assert np.array_equal(got, np.full(c, 8 / n))
    assert_ap(got, ap_reference(prob, target), n)


def test_out_of_range_targets_are_negatives_everywhere():
    c = 5
    prob, target = random_case(64, c, 3)
    target[::4] = -1
    target[1::8] = c
    target[2::8] = c + 7
    ref = ap_reference(prob, target)
    assert_ap(torch_ap(torch.from_numpy(prob), target), ref, 64)
    # the same rows labelled with another ignored value: the same negatives
    other = np.where((target < 0) | (target >= c), 2, target)
    assert_ap(torch_ap(torch.from_numpy(prob), other, ignore_label=2), ap_reference(prob, other, ignore_label=2), 64)
    moved = np.where((target < 0) | (target >= c), -1, target)
    assert_ap(ref, ap_reference(prob, moved), 64)


def test_empty_batch_is_all_nan():
    got = torch_ap(torch.zeros(0, 7), np.zeros(0, dtype=np.int64))
    assert got.shape == (7,) and np.isnan(got).all()
    assert np.isnan(ap_reference(np.zeros((0, 7)), np.zeros(0, dtype=np.int64))).all()


def test_negative_zero_ties_with_zero():
    prob = np.array([[0.0, 1.0], [-0.0, 1.0], [0.0, 1.0], [-0.0, 1.0]], dtype=np.float32)
    target = np.array([0, 1, 1, 0], dtype=np.int64)
    got = torch_ap(torch.from_numpy(prob), target)
    assert np.array_equal(got, [0.5, 0.5])                        # one tie group per column: P_c / N
    assert_ap(got, ap_reference(prob, target), 4)


def test_bf16_input_and_logits():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(257, 20, generator=g) * 2).to(torch.bfloat16)
    target = np.random.default_rng(5).integers(-1, 20, 257).astype(np.int64)
    assert_ap(torch_ap(x, target), ap_reference(x.float().numpy(), target), 257)
    prob = torch.softmax(x.float(), 1)
    assert_ap(torch_ap(x, target, from_logits=True), ap_reference(prob.numpy(), target), 257)


def test_meter_accumulates_nanmean_over_steps():
    from languagegroundedsemseg_amd.metrics import AveragePrecisionMeter
    c = 6
    meter = AveragePrecisionMeter(c, ignore_label=-1)
    assert sorted(dict(meter.named_buffers())) == ["ap_sum", "steps"]
    rows = []
    for step in range(3):
        prob, target = random_case(50, c, 100 + step)
        if step == 1:
            target[target == 4] = -1                               # class 4 is absent in step 2
        out = meter.update(torch.from_numpy(prob), torch.from_numpy(target))
        rows.append(ap_reference(prob, target))
        assert_ap(out.numpy(), rows[-1], 50)
    rows = np.stack(rows)
    assert np.isnan(rows[1, 4]) and not np.isnan(rows[[0, 2], 4]).any()
    stats = meter.compute()
    assert_ap(stats["ap"].numpy(), np.nanmean(rows, 0), 50)
    assert abs(float(stats["map"]) - np.nanmean(np.nanmean(rows, 0))) <= tol(50)
    assert stats["steps"].tolist() == [3, 3, 3, 3, 2, 3]
    meter.reset()
    assert float(meter.ap_sum.abs().sum()) == 0 and int(meter.steps.sum()) == 0
    empty = meter.compute()
    assert bool(torch.isnan(empty["ap"]).all()) and bool(torch.isnan(empty["map"]))
    with pytest.raises(ValueError):
        meter.update(torch.zeros(4, c + 1), torch.zeros(4, dtype=torch.int64))


def test_new_symbols_are_exported_and_abi_stays_18():
    from languagegroundedsemseg_amd import engine
    header = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    L = engine.lib()
    for name in ("lgs_ap_workspace_bytes", "lgs_average_precision"):
        assert name in engine.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S))
        assert hasattr(L, name)
    assert L.lgs_abi_version() == 18


def test_null_pointers_and_wide_heads_are_refused_by_name():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    # (scores, n, c, labels, ignore_index, from_logits, ap_out, dtype, workspace, stream)
    for args in ((None, 4, 2, p, -1, 0, p, engine.LGS_F32, p, None),
                 (p, 4, 2, None, -1, 0, p, engine.LGS_F32, p, None),
                 (p, 4, 2, p, -1, 0, None, engine.LGS_F32, p, None),
                 (p, 4, 2, p, -1, 0, p, engine.LGS_F32, None, None),
                 (None, 0, 2, None, -1, 0, None, engine.LGS_F32, None, None)):
        assert L.lgs_average_precision(*args) != 0
        msg = L.lgs_last_error().decode()
        assert "lgs_average_precision" in msg and "null argument" in msg
    for c, dtype in ((513, engine.LGS_F32), (1025, engine.LGS_BF16), (0, engine.LGS_F32)):
        assert L.lgs_average_precision(p, 4, c, p, -1, 0, p, dtype, p, None) != 0
        msg = L.lgs_last_error().decode()
        assert "lgs_average_precision: more classes than one half-wave holds (512 fp32 / 1024 bf16)" in msg
    assert L.lgs_average_precision(p, 4, 2, p, -1, 0, p, 7, p, None) != 0
    assert "lgs_average_precision: unknown dtype" in L.lgs_last_error().decode()
    assert L.lgs_ap_workspace_bytes(-1, 2) == -1 and L.lgs_ap_workspace_bytes(4, 1025) == -1
