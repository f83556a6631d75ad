"""lgs_seg_metrics (csrc/lgs_metrics.hip) behind SegmentationMeter on the MI355X.  References, all written here: torch.max on the CPU
copy of the stored values for pred, np.bincount(c * label[k] + pred[k]) for the matrix, float64 softmax for prob.

Rows per workgroup tile, restated from the kernel's launch table (8 half-waves x R rows, Q x R = 4 with Q = 16-byte chunks per lane
and row = ceil(ceil(c / W) / 32), W = 4 fp32 / 8 bf16 elements): 32 rows while a row fits one chunk per lane (c <= 128 fp32 /
256 bf16), 16 rows up to two chunks (c <= 256 / 512), 8 rows beyond.  A launch has at most METRICS_BLOCKS workgroups; each walks
tiles blockIdx.x, + gridDim.x, ..."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tile_rows(c, dtype):
    w = 4 if dtype == torch.float32 else 8
    q = ((c + w - 1) // w + 31) // 32
    return 32 if q <= 1 else (16 if q == 2 else 8)


def np_confmat(pred, label, c, ignore):
    pred, label = np.asarray(pred), np.asarray(label)
    k = (label != ignore) & (label >= 0) & (label < c)
    return np.bincount(c * label[k].astype(np.int64) + pred[k], minlength=c * c).reshape(c, c)


def metric_launches():
    from languagegroundedsemseg_amd import engine
    return sum(v for k, v in engine.dispatch_counts().items() if "k_seg_metrics" in k)


def make_scores(n, c, dtype, seed):
    """half of the rows on a coarse grid (many exact ties of the maximum), the others continuous"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3.0
    coarse = torch.arange(n) % 2 == 0
    x[coarse] = torch.round(x[coarse])
    return x.to(dtype)


def make_labels(n, c, seed, ignore=-1):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, c, n)
    r = rng.random(n)
    lab[r < 0.10] = ignore
    lab[(r >= 0.10) & (r < 0.13)] = c + rng.integers(0, 5)       # out of range above
    lab[(r >= 0.13) & (r < 0.15)] = -7                            # and below
    return lab.astype(np.int64)


def run_meter(x, lab, c, ignore=-1, want_prob=False, meter=None):
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    m = meter if meter is not None else SegmentationMeter(c, ignore_label=ignore).to(DEV)
    out = m.update(x.to(DEV), torch.from_numpy(lab).to(DEV), want_prob=want_prob)
    torch.cuda.synchronize()
    return m, out


WIDTHS = [(200, torch.float32), (200, torch.bfloat16), (3, torch.float32), (3, torch.bfloat16), (8, torch.float32), (8, torch.bfloat16),
          (13, torch.float32), (13, torch.bfloat16), (512, torch.float32), (1024, torch.bfloat16)]


@pytest.mark.parametrize("c,dtype", WIDTHS, ids=["%d-%s" % (c, str(d).split(".")[1]) for c, d in WIDTHS])
def test_pred_and_matrix_are_exact(c, dtype):
    """every class width (13: rows that are no multiple of 16 bytes; 512 fp32 / 1024 bf16: the widest a half-wave holds) at the
    row counts around one workgroup tile, and 5003 rows once with the default grid and once with 3 workgroups walking 50+ tiles
    each (where the LDS table of 256 cells overflows into direct global adds for c = 200)"""
    from languagegroundedsemseg_amd import engine
    t = tile_rows(c, dtype)
    for n, blocks in [(1, None), (t - 1, None), (t, None), (t + 1, None), (5003, None), (5003, 3)]:
        x = make_scores(n, c, dtype, 100 + n)
        lab = make_labels(n, c, 200 + n)
        before = metric_launches()
        if blocks is None:
            m, pred = run_meter(x, lab, c)
        else:
            with engine.tuning(METRICS_BLOCKS=blocks):
                m, pred = run_meter(x, lab, c)
        assert metric_launches() == before + 1, "the kernel must have run (c=%d n=%d)" % (c, n)
        want = torch.max(x.float().cpu(), 1)[1]
        assert pred.dtype == torch.int64 and torch.equal(pred.cpu(), want), (c, n, blocks)
        assert np.array_equal(m.confmat.cpu().numpy(), np_confmat(want.numpy(), lab, c, -1)), (c, n, blocks)


def test_a_head_wider_than_the_half_wave_takes_the_torch_lines():
    c, n = 513, 301
    x, lab = make_scores(n, c, torch.float32, 1), make_labels(n, c, 2)
    before = metric_launches()
    m, (pred, prob) = run_meter(x, lab, c, want_prob=True)
    assert metric_launches() == before, "c = 513 fp32 does not fit the kernel"
    want = torch.max(x, 1)[1]
    assert torch.equal(pred.cpu(), want) and np.array_equal(m.confmat.cpu().numpy(), np_confmat(want.numpy(), lab, c, -1))
    assert float((prob.double().cpu() - torch.softmax(x.double(), 1)).abs().max()) < 1e-6
    # and the last width that does: one launch
    m, pred = run_meter(make_scores(n, 512, torch.float32, 3), make_labels(n, 512, 4), 512)
    assert metric_launches() == before + 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_hand_written_rows(dtype):
    inf, nan = float("inf"), float("nan")
    x = torch.full((6, 200), -1.0)
    x[0, 17] = x[0, 150] = 2.0                      # two-way tie -> 17
    x[1, 199] = x[1, 64] = x[1, 33] = 5.0           # three-way tie -> 33
    x[2, 120] = nan; x[2, 40] = nan; x[2, 7] = 100.0   # NaN at two places -> the first NaN, 40
    x[3] = -inf                                     # -> 0
    x[4, 90] = x[4, 31] = inf                       # -> 31
    x[5, 11] = 1.0                                  # an ignored row still gets its pred
    lab = np.array([17, 33, 40, 5, 31, -1], np.int64)
    m, pred = run_meter(x.to(dtype), lab, 200)
    assert pred.cpu().tolist() == [17, 33, 40, 0, 31, 11]
    assert pred.cpu().tolist() == torch.max(x.to(dtype).float(), 1)[1].tolist()
    assert np.array_equal(m.confmat.cpu().numpy(), np_confmat([17, 33, 40, 0, 31, 11], lab, 200, -1))


def test_contention_on_one_and_on_two_cells():
    n, c = 100000, 200
    x = torch.zeros(n, c, dtype=torch.bfloat16)
    x[:, 77] = 1.0
    m, pred = run_meter(x, np.full(n, 5, np.int64), c)
    cm = m.confmat.cpu().numpy()
    assert cm[5, 77] == n and cm.sum() == n and int(pred.min()) == int(pred.max()) == 77
    x[1::2, 77] = 0.0
    x[1::2, 3] = 1.0
    lab = np.full(n, 5, np.int64)
    lab[1::2] = 199
    m, pred = run_meter(x, lab, c)
    cm = m.confmat.cpu().numpy()
    assert cm[5, 77] == n // 2 and cm[199, 3] == n // 2 and cm.sum() == n


def test_accumulation_is_64_bit_and_adds_up():
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    c = 200
    m = SegmentationMeter(c).to(DEV)
    m.confmat[9, 4] = 2 ** 32 - 10
    x = torch.zeros(100, c)
    x[:, 4] = 1.0
    run_meter(x, np.full(100, 9, np.int64), c, meter=m)
    assert int(m.confmat[9, 4]) == 2 ** 32 + 90 and int(m.confmat.sum()) == 2 ** 32 + 90
    # two updates equal the sum of their matrices
    xa, xb = make_scores(700, c, torch.float32, 5), make_scores(900, c, torch.float32, 6)
    la, lb = make_labels(700, c, 7), make_labels(900, c, 8)
    m = SegmentationMeter(c).to(DEV)
    _, pa = run_meter(xa, la, c, meter=m)
    _, pb = run_meter(xb, lb, c, meter=m)
    want = np_confmat(torch.max(xa, 1)[1].numpy(), la, c, -1) + np_confmat(torch.max(xb, 1)[1].numpy(), lb, c, -1)
    assert np.array_equal(m.confmat.cpu().numpy(), want)
    m.reset()
    assert int(m.confmat.abs().sum()) == 0


def test_ignored_rows_add_nothing_and_still_get_a_pred():
    c, n = 300, 2000                                 # ignore_label 255 is a class index at this width
    x = make_scores(n, c, torch.bfloat16, 9)
    lab = make_labels(n, c, 10, ignore=255)
    lab[::7] = 255
    m, pred = run_meter(x, lab, c, ignore=255)
    want = torch.max(x.float(), 1)[1]
    assert torch.equal(pred.cpu(), want)
    cm = m.confmat.cpu().numpy()
    assert np.array_equal(cm, np_confmat(want.numpy(), lab, c, 255)) and cm[255].sum() == 0
    assert cm.sum() == ((lab != 255) & (lab >= 0) & (lab < c)).sum()
    # nothing but ignored / out-of-range rows: an empty matrix, every pred written
    lab2 = np.where(np.arange(n) % 2 == 0, 255, c + 1).astype(np.int64)
    m, pred = run_meter(x, lab2, c, ignore=255)
    assert int(m.confmat.abs().sum()) == 0 and torch.equal(pred.cpu(), want)


@pytest.mark.parametrize("c,dtype", [(200, torch.float32), (200, torch.bfloat16), (13, torch.float32), (3, torch.bfloat16), (1024, torch.bfloat16)],
                         ids=["200-float32", "200-bfloat16", "13-float32", "3-bfloat16", "1024-bfloat16"])
def test_prob_against_float64_softmax(c, dtype):
    """bound: 4 x the max-abs error of torch's own fp32 CPU softmax against float64 on the same stored values, + 1e-7 (the margin
    for a different but fixed reduction order; the floor for inputs where torch is exact).
    Measured on the MI355X (kernel / torch fp32 CPU, max-abs against float64): see DESIGN.md section 4, 'Segmentation metrics'."""
    n = 1003
    x = make_scores(n, c, dtype, 20 + c)
    lab = make_labels(n, c, 21)
    m, (pred, prob) = run_meter(x, lab, c, want_prob=True)
    stored = x.float()
    ref = torch.softmax(stored.double(), 1)
    torch_err = float((torch.softmax(stored, 1).double() - ref).abs().max())
    bound = 4 * torch_err + 1e-7
    assert prob.dtype == torch.float32 and prob.shape == (n, c)
    err = float((prob.double().cpu() - ref).abs().max())
    row_err = float((prob.double().cpu().sum(1) - 1).abs().max())
    print("softmax c=%d %s: kernel max-abs err %.3e, torch fp32 CPU %.3e, bound %.3e, rows sum to 1 within %.3e" % (
        c, str(dtype).split(".")[1], err, torch_err, bound, row_err))
    assert err <= bound
    assert row_err <= bound * c
    assert torch.equal(pred.cpu(), torch.max(stored, 1)[1])
    assert np.array_equal(m.confmat.cpu().numpy(), np_confmat(pred.cpu().numpy(), lab, c, -1))


def test_no_prob_tensor_is_allocated_unless_asked_for():
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    n, c = 5003, 200
    x = make_scores(n, c, torch.bfloat16, 30).to(DEV)
    lab = torch.from_numpy(make_labels(n, c, 31)).to(DEV)
    m = SegmentationMeter(c).to(DEV)
    m.update(x, lab)                                  # warm: library, caches
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pred = m.update(x, lab)
    torch.cuda.synchronize()
    held, peak = torch.cuda.memory_allocated() - base, torch.cuda.max_memory_allocated() - base
    assert held <= n * 8 + 4096 and peak < n * c * 4, (held, peak)        # pred only; a prob tensor would be 4 MB
    pred, prob = m.update(x, lab, want_prob=True)
    assert prob.shape == (n, c)


def test_two_runs_are_bit_identical():
    n, c = 5003, 200
    x, lab = make_scores(n, c, torch.bfloat16, 40), make_labels(n, c, 41)
    (ma, (pa, qa)), (mb, (pb, qb)) = run_meter(x, lab, c, want_prob=True), run_meter(x, lab, c, want_prob=True)
    assert torch.equal(pa, pb) and torch.equal(qa.view(torch.int32), qb.view(torch.int32)) and torch.equal(ma.confmat, mb.confmat)


def test_update_and_compute_run_without_a_host_sync():
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    n, c = 5003, 200
    x = make_scores(n, c, torch.bfloat16, 50).to(DEV)
    lab_h = make_labels(n, c, 51)
    lab = torch.from_numpy(lab_h).to(DEV)
    groups_h = np.zeros((c, 3), bool)
    groups_h[np.arange(c), np.arange(c) % 3] = True
    groups = torch.from_numpy(groups_h).to(DEV)
    m = SegmentationMeter(c).to(DEV)
    m.update(x[:8], lab[:8])                          # warm: library load
    m.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(x[:2000], lab[:2000])
        pred, prob = m.update(x[2000:], lab[2000:], want_prob=True)
        out = m.compute(groups=groups)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = torch.max(x.float().cpu(), 1)[1].numpy()
    cm = np_confmat(want, lab_h, c, -1)
    assert np.array_equal(m.confmat.cpu().numpy(), cm) and int(out["count"]) == cm.sum()
    d, r, s = np.diag(cm).astype(float), cm.sum(1).astype(float), cm.sum(0).astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = d / (r + s - d)
    np.testing.assert_allclose(out["iou"].cpu().numpy(), iou, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(float(out["miou"]), np.nanmean(iou), rtol=1e-12)
    for g, name in enumerate(("head", "common", "tail")):
        ids = np.nonzero(groups_h[:, g])[0]
        np.testing.assert_allclose(float(out[name + "_miou"]), np.nanmean(iou[ids]), rtol=1e-12)
        sub = np.zeros_like(cm)
        sub[ids] = cm[ids]
        rs = sub.sum(1).astype(float)
        rec = np.diag(sub)[ids] / np.maximum(rs[ids], 1)          # every class of the group has rows at this size
        assert (rs[ids] > 0).all()
        np.testing.assert_allclose(out[name + "_recall"].cpu().numpy()[ids], rec, rtol=1e-12)
        np.testing.assert_allclose(float(out[name + "_recall_mean"]), rec.mean(), rtol=1e-12)


def test_the_training_step_ends_in_the_meter():
    """Res16UNet14A on a 5 cm synthetic scene: per-point CE -> balanced category sampling (split='stats') -> meter.update"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import Cfg, deterministic_init
    import MinkowskiEngine as ME
    from languagegroundedsemseg_amd import models
    from languagegroundedsemseg_amd.losses import fused_cross_entropy, sample_categories_for_balancing
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    from languagegroundedsemseg_amd.synthetic import make_batch
    c = 200
    coords, feats, labels = make_batch([0], voxel=0.05, n_target=25000)
    model = deterministic_init(models.load_model("Res16UNet14A")(3, c, Cfg()), 42).to(DEV).train()
    lab = torch.from_numpy(labels).to(DEV)
    groups = torch.zeros(c, 3, dtype=torch.bool)
    groups[:66, 0] = True
    groups[66:132, 1] = True
    groups[132:, 2] = True
    groups = groups.to(DEV)
    meter = SegmentationMeter(c, ignore_label=-1).to(DEV)
    before = metric_launches()
    out, _ = model(ME.SparseTensor(torch.from_numpy(feats).to(DEV), torch.from_numpy(coords).to(DEV)))
    loss_rows = fused_cross_entropy(out.F, lab, ignore_index=-1, reduction="none")
    loss, stats, _ = sample_categories_for_balancing(loss_rows, lab, groups, -1.0, -1.0, ignore_label=-1, split="stats")
    pred = meter.update(out, lab)
    loss.backward()
    res = meter.compute(groups=groups)
    torch.cuda.synchronize()
    assert metric_launches() == before + 1
    logits = out.F.detach().float().cpu()
    want = torch.max(logits, 1)[1]
    n_valid = int((labels != -1).sum())
    assert n_valid < labels.shape[0] and int(res["count"]) == n_valid == int(stats[:, 1].sum())
    assert torch.equal(pred.cpu(), want)
    assert np.array_equal(meter.confmat.cpu().numpy(), np_confmat(want.numpy(), labels, c, -1))
