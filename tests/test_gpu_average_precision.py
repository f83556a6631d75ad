"""lgs_average_precision (csrc/lgs_ap.hip) behind metrics.average_precision / AveragePrecisionMeter on the MI355X.

Every case compares with tests/ap_reference.py (numpy fp64) fed the exact values the kernel ranks: the tensor itself, read as
float64, for probabilities; for from_logits the fp32 prob that SegmentationMeter.update(want_prob=True) returns.  Tolerance
4 N 2^-53 absolute (fp64 sums of at most N terms, each at most 1, divided by P_c), NaN positions equal."""
import numpy as np
import pytest
import torch

from ap_reference import ap_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tol(n):
    return 4 * max(n, 1) * 2.0 ** -53


def assert_ap(got, want, n):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    k = ~np.isnan(want)
    if k.any():
        err = np.abs(got[k] - want[k]).max()
        print("max |AP - reference| = %.3g (bound %.3g)" % (err, tol(n)))
        assert err <= tol(n)


def rank_launches():
    from languagegroundedsemseg_amd import engine
    return sum(v for k, v in engine.dispatch_counts().items() if "k_ap_rank" in k)


def gpu_ap(scores, target, **kw):
    from languagegroundedsemseg_amd.metrics import average_precision
    out = average_precision(scores.to(DEV), torch.as_tensor(target).to(DEV), **kw)
    assert out.dtype == torch.float64 and out.device.type == "cuda"
    return out


def meter_prob(scores, target, ignore=-1):
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    m = SegmentationMeter(scores.shape[1], ignore_label=ignore).to(DEV)
    _, prob = m.update(scores.to(DEV), torch.as_tensor(target).to(DEV), want_prob=True)
    return prob


def make_scores(n, c, dtype, seed):
    """logits with a spread that leaves some columns' scores below the lowest positive (the skip test) and some above"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, generator=g) * 3.0).to(dtype)


def make_labels(n, c, seed, ignore=-1):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, c, n)
    lab[rng.random(n) < 0.1] = ignore
    return lab.astype(np.int64)


SHAPES = [(n, c, dt) for c, dt in ((13, torch.float32), (20, torch.bfloat16), (200, torch.float32), (200, torch.bfloat16))
          for n in (1, 33, 4099)] + [(257, 512, torch.float32), (257, 1024, torch.bfloat16)]


@pytest.mark.parametrize("n,c,dtype", SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_shapes_prob_input_and_logits(n, c, dtype):
    x = make_scores(n, c, dtype, 1000 * c + n)
    lab = make_labels(n, c, n + c)
    before = rank_launches()
    # the stored values ranked as they are (negative scores included)
    assert_ap(gpu_ap(x, lab), ap_reference(x.float().numpy(), lab), n)
    # and their softmax
    prob = meter_prob(x, lab)
    assert_ap(gpu_ap(x, lab, from_logits=True), ap_reference(prob.cpu().numpy(), lab), n)
    assert rank_launches() == before + 2


def launches_of(kernel):
    from languagegroundedsemseg_amd import engine
    return sum(v for k, v in engine.dispatch_counts().items() if k.startswith(kernel + "<"))


@pytest.mark.parametrize("n,c,dtype,hot", [(2600, 200, torch.float32, False), (2700, 200, torch.float32, False),
                                           (2700, 200, torch.bfloat16, False), (80001, 13, torch.float32, True),
                                           (80001, 20, torch.bfloat16, True), (61441, 13, torch.float32, False)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_both_rank_kernels_and_the_hot_run(n, c, dtype, hot):
    """the rank pass keeps its counters in LDS from n c = 2^19 elements on (2622 rows of 200 classes): one case below, the others
    above; `hot`: every label inside one 16-byte chunk of columns, so that its run of positives is longer than the 65 536 LDS
    counters and adds to global memory; 61 441 rows: one more than a slab of rows holds"""
    x = make_scores(n, c, dtype, n)
    lab = make_labels(n, c, n)
    if hot:
        lab = np.where(lab >= 0, lab % 4, lab)
        assert (lab >= 0).sum() > 65536
    rows, cols = launches_of("k_ap_rank"), launches_of("k_ap_rank_cols")
    assert_ap(gpu_ap(x, lab), ap_reference(x.float().numpy(), lab), n)
    assert_ap(gpu_ap(x, lab, from_logits=True), ap_reference(meter_prob(x, lab).cpu().numpy(), lab), n)
    big = n * c >= 1 << 19
    assert launches_of("k_ap_rank") - rows == (0 if big else 2) and launches_of("k_ap_rank_cols") - cols == (2 if big else 0)


def test_wider_head_takes_the_torch_path_and_agrees():
    n, c = 257, 513
    x = make_scores(n, c, torch.float32, 3)
    lab = make_labels(n, c, 3)
    before = rank_launches()
    assert_ap(gpu_ap(torch.softmax(x, 1), lab), ap_reference(torch.softmax(x, 1).numpy(), lab), n)
    assert rank_launches() == before


def test_ties_four_levels():
    n, c = 4099, 200
    g = torch.Generator().manual_seed(11)
    prob = torch.round(torch.rand(n, c, generator=g) * 3) / 3
    assert len(torch.unique(prob)) == 4
    lab = make_labels(n, c, 11)
    for dtype in (torch.float32, torch.bfloat16):
        p = prob.to(dtype)
        assert_ap(gpu_ap(p, lab), ap_reference(p.float().numpy(), lab), n)


def test_saturated_logits_zero_scored_positive_ranks_last():
    n, c = 4099, 200
    g = torch.Generator().manual_seed(12)
    x = torch.where(torch.rand(n, c, generator=g) < 0.02, 80.0, -80.0)
    lab = make_labels(n, c, 12)
    prob = meter_prob(x, lab).cpu().numpy()
    assert ((prob == 0.0) | (prob == 1.0)).mean() > 0.5
    pos0 = [(i, l) for i, l in enumerate(lab) if l >= 0 and prob[i, l] == 0.0]
    assert pos0                                                    # positives whose own score is exactly 0.0: Rank = N
    assert_ap(gpu_ap(x, lab, from_logits=True), ap_reference(prob, lab), n)
    assert_ap(gpu_ap(torch.from_numpy(prob), lab), ap_reference(prob, lab), n)
    # one class whose only positive scores 0.0 while nothing in the column is below it: TP / Rank = 1 / N exactly
    p1 = np.abs(prob).copy()
    p1[:, 7] = np.where(np.arange(n) % 3 == 0, 0.0, 0.5)
    p1[3, 7] = -0.0
    l1 = np.where(lab == 7, -1, lab)
    l1[3] = 7
    got = gpu_ap(torch.from_numpy(p1), l1)
    assert float(got[7]) == 1.0 / n
    assert_ap(got, ap_reference(p1, l1), n)


LABEL_CASES = ["hot", "single", "absent", "all_ignored", "mixed_out_of_range", "other_ignore"]


@pytest.mark.parametrize("case", LABEL_CASES)
def test_label_shapes(case):
    n, c, ignore = 4099, 200, -1
    x = make_scores(n, c, torch.float32, 21)
    rng = np.random.default_rng(21)
    lab = rng.integers(0, c, n).astype(np.int64)
    if case == "hot":
        lab[rng.random(n) < 0.9] = 0                               # one hot segment
    elif case == "single":
        lab[lab == 5] = 6
        lab[1234] = 5                                              # exactly one positive
    elif case == "absent":
        lab[lab == 9] = 10
    elif case == "all_ignored":
        lab[:] = ignore
    elif case == "mixed_out_of_range":
        r = rng.random(n)
        lab[r < 0.1] = -1
        lab[(r >= 0.1) & (r < 0.2)] = c
        lab[(r >= 0.2) & (r < 0.3)] = 255
    elif case == "other_ignore":
        ignore = 17                                                # a class index as the ignored value
    prob = torch.softmax(x, 1)
    want = ap_reference(prob.numpy(), lab, ignore_label=ignore)
    if case == "all_ignored":
        assert np.isnan(want).all()
    if case == "absent":
        assert np.isnan(want[9])
    if case == "other_ignore":
        assert np.isnan(want[17])
    assert_ap(gpu_ap(prob, lab, ignore_label=ignore), want, n)
    assert_ap(gpu_ap(x.to(torch.bfloat16), lab, ignore_label=ignore, from_logits=True),
              ap_reference(meter_prob(x.to(torch.bfloat16), lab, ignore).cpu().numpy(), lab, ignore_label=ignore), n)


def test_empty_batch_is_all_nan():
    out = gpu_ap(torch.zeros(0, 200), np.zeros(0, dtype=np.int64))
    assert out.shape == (200,) and bool(torch.isnan(out).all())


@pytest.mark.parametrize("c", [200, 13])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_from_logits_is_bit_identical_to_the_meters_prob(c, dtype):
    n = 4099
    x = make_scores(n, c, dtype, 31 + c)
    lab = make_labels(n, c, 31)
    a = gpu_ap(x, lab, from_logits=True)
    b = gpu_ap(meter_prob(x, lab), lab)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_two_calls_give_the_same_bits():
    n, c = 4099, 200
    x = make_scores(n, c, torch.bfloat16, 41)
    lab = make_labels(n, c, 41)
    for kw in ({}, {"from_logits": True}):
        a, b = gpu_ap(x, lab, **kw), gpu_ap(x, lab, **kw)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_non_contiguous_view_and_sparse_tensor_argument():
    n, c = 33, 200
    wide = make_scores(n, 2 * c, torch.float32, 51)
    lab = make_labels(n, c, 51)
    view = wide.to(DEV)[:, ::2]
    assert not view.is_contiguous()
    want = ap_reference(wide[:, ::2].numpy(), lab)
    assert_ap(gpu_ap(view, lab), want, n)

    import MinkowskiEngine as ME
    from languagegroundedsemseg_amd.metrics import average_precision
    coords = torch.zeros(n, 4, dtype=torch.int32)
    coords[:, 1] = torch.arange(n, dtype=torch.int32)              # n distinct voxels: the rows keep their order
    st = ME.SparseTensor(view.contiguous(), coords.to(DEV))
    assert_ap(average_precision(st, torch.from_numpy(lab).to(DEV)), ap_reference(st.F.cpu().numpy(), lab), n)


def test_meter_update_and_compute_do_not_synchronise():
    from languagegroundedsemseg_amd.metrics import AveragePrecisionMeter
    n, c = 4099, 200
    meter = AveragePrecisionMeter(c, ignore_label=-1).to(DEV)
    steps = [(make_scores(n, c, torch.bfloat16, 60 + s).to(DEV), torch.from_numpy(make_labels(n, c, 60 + s)).to(DEV)) for s in range(2)]
    meter.update(*steps[0], from_logits=True)                      # (first use: library load, the workspace)
    meter.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [meter.update(x, t, from_logits=True) for x, t in steps]
        stats = meter.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows = np.stack([ap_reference(meter_prob(x, t).cpu().numpy(), t.cpu().numpy()) for x, t in steps])
    for o, r in zip(outs, rows):
        assert_ap(o, r, n)
    assert_ap(stats["ap"], np.nanmean(rows, 0), n)
    assert stats["steps"].tolist() == (~np.isnan(rows)).sum(0).tolist()
    assert abs(float(stats["map"]) - np.nanmean(np.nanmean(rows, 0))) <= tol(n)
