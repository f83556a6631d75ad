"""Segmentation metrics of a training / validation step without a host synchronisation.

The reference measures itself in EVERY step: `BaselineTrainerModule.eval_step` (lib/train_test/pl_BaselineTrainer.py:357-378) takes
`pred = soutput.F.max(1)[1]`, `prob = softmax(soutput.F, 1)` and feeds torchmetrics' Precision / Recall / JaccardIndex, once over all
valid rows and once over each of the head / common / tail row subsets.  Everything it logs from them except the per-class average
precision is a function of ONE integer matrix: the confusion matrix of the valid
rows, and -- because `split_items[:, g]` is `valid & group_of_class[target] == g` -- the three subsets are row subsets of the same
matrix.  `SegmentationMeter.update` is one pass over the scores (lgs_seg_metrics on HIP tensors); `compute` derives the numbers on
the device.

The per-class average precision (pl_BaselineTrainer.py:380: `AveragePrecision(num_classes, average=None)(prob, target)`, stacked per
step and nanmean-ed per class) is `average_precision` / `AveragePrecisionMeter`: sklearn's step-wise AP, computed from the sorted
positives and one counting pass over the scores (lgs_average_precision on HIP tensors), also straight from the logits, so that a
validation step needs no fp32 [N, C] `prob` at all.

The definitions below are THIS PROJECT'S (the reference's torchmetrics version is not a dependency here and its exact averaging
conventions were not reproduced); they are not a parity claim.  Only `fast_hist` / `per_class_iu` restate reference code
(lib/utils.py:92-109)."""
import torch
import torch.nn as nn

from .me.core import get_backend

GROUP_NAMES = ("head", "common", "tail")


def _features(x):
    return x.F if hasattr(x, "F") and not torch.is_tensor(x) else x


def _torch_update(scores, target, ignore_label, confmat, want_prob):
    """the kernel's semantics in torch lines: CPU tensors and heads wider than one half-wave holds"""
    c = scores.shape[1]
    x = scores.float()
    pred = torch.max(x, 1)[1]
    prob = torch.softmax(x, 1) if want_prob else None
    t = target.long()
    w = ((t != ignore_label) & (t >= 0) & (t < c)).long()         # rows that count; the others add weight 0 to cell 0
    cell = torch.where(w > 0, t * c + pred, torch.zeros_like(t))
    confmat += torch.zeros(c * c, dtype=torch.int64, device=confmat.device).scatter_add_(0, cell, w).view(c, c)
    return pred, prob


def _ratio(num, den, present):
    """num / den; a class that is present (anything in its row or column) with a zero denominator gives 0, an absent class NaN"""
    nan = torch.full_like(num, float("nan"))
    return torch.where(den > 0, num / den.clamp_min(1), torch.where(present, torch.zeros_like(num), nan))


def _nanmean_over(v, keep):
    return torch.nanmean(torch.where(keep, v, torch.full_like(v, float("nan"))))


def confusion_metrics(confmat, groups=None):
    """confmat [C, C] (rows = labels, columns = predictions) -> dict of float64 tensors on its device, no host sync:
      iou [C]        diag / (rowsum + colsum - diag), 0/0 = NaN  (lib/utils.py:107-109, what nanmean_t(ious) expects)
      precision [C]  diag / colsum,  recall [C] = diag / rowsum: NaN for a class with rowsum + colsum == 0, 0 for a class that is
                     present but has a zero denominator
      precision_macro, recall_macro, miou    means over the classes that are not NaN
      count          the sum of the matrix
    groups (bool [C, 3]: head / common / tail, the `frequency_organized_cats` of sample_categories_for_balancing) adds per group g
      <g>_precision [C], <g>_recall [C]   the same ratios on the ROW SUBSET confmat[groups[:, g]] (the reference's
                                          valid_pred[split_items[:, g]] meters)
      <g>_precision_mean, <g>_recall_mean their nanmean over the group's classes
      <g>_miou                            nanmean of iou over the group's classes"""
    cm = confmat.to(torch.float64)
    diag, rows, cols = cm.diagonal(), cm.sum(1), cm.sum(0)
    present = (rows + cols) > 0
    nan = torch.full_like(diag, float("nan"))
    union = rows + cols - diag
    out = {
        "iou": torch.where(union > 0, diag / union.clamp_min(1), nan),
        "precision": _ratio(diag, cols, present),
        "recall": _ratio(diag, rows, present),
        "count": confmat.sum(),
    }
    out["miou"] = torch.nanmean(out["iou"])
    out["precision_macro"] = torch.nanmean(out["precision"])
    out["recall_macro"] = torch.nanmean(out["recall"])
    if groups is not None:
        groups = groups.to(confmat.device).bool()
        for g, name in enumerate(GROUP_NAMES):
            in_g = groups[:, g]
            sub = cm * in_g[:, None].to(cm.dtype)         # the row subset, by masking: a boolean index would be a host sync
            d, r, c = sub.diagonal(), sub.sum(1), sub.sum(0)
            pres = (r + c) > 0
            out[name + "_precision"] = _ratio(d, c, pres)
            out[name + "_recall"] = _ratio(d, r, pres)
            out[name + "_precision_mean"] = _nanmean_over(out[name + "_precision"], in_g)
            out[name + "_recall_mean"] = _nanmean_over(out[name + "_recall"], in_g)
            out[name + "_miou"] = _nanmean_over(out["iou"], in_g)
    return out


class SegmentationMeter(nn.Module):
    """Confusion matrix of a run of steps, kept on the device.

        meter = SegmentationMeter(num_labels, ignore_label=config.ignore_label).to(device)
        pred = meter.update(soutput.F, target)                    # or: pred, prob = meter.update(soutput, target, want_prob=True)
        stats = meter.compute(groups=dataset.frequency_organized_cats)

    `confmat` is a registered int64 buffer [C, C]: it follows .to(device) and is what the reference reads as
    `iou_scores.confmat` (pl_BaselineTrainer.py:165, :203).  update() may be called with or without autograd recording; it detaches."""

    def __init__(self, num_classes, ignore_label=-1):
        super().__init__()
        self.num_classes = int(num_classes)
        self.ignore_label = int(ignore_label)
        self.register_buffer("confmat", torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64))

    @torch.no_grad()
    def update(self, scores, target, want_prob=False):
        """scores [N, C] (tensor or SparseTensor), target [N] -> pred [N] int64 (scores.max(1)[1]: lowest index among the maxima,
        first NaN if any), or (pred, prob [N, C] fp32 softmax) with want_prob.  Rows whose target is ignore_label or outside
        [0, C) add nothing to the matrix and still get a pred."""
        scores = _features(scores).detach()
        if scores.dim() != 2 or scores.shape[1] != self.num_classes:
            raise ValueError("scores must be [N, %d], got %s" % (self.num_classes, tuple(scores.shape)))
        if target.shape[0] != scores.shape[0]:
            raise ValueError("%d targets for %d rows" % (target.shape[0], scores.shape[0]))
        be = get_backend()
        if scores.is_cuda and hasattr(be, "seg_metrics") and be.seg_metrics_supports(scores):
            pred, prob = be.seg_metrics(scores, target.to(scores.device), self.ignore_label, self.confmat, want_prob)
        else:
            pred, prob = _torch_update(scores, target.to(scores.device), self.ignore_label, self.confmat, want_prob)
        return (pred, prob) if want_prob else pred

    def reset(self):
        self.confmat.zero_()

    @torch.no_grad()
    def compute(self, groups=None, process_group=None):
        """-> the dict of confusion_metrics().  When torch.distributed is initialised (or process_group is given) the matrix is
        sum-reduced over the ranks first (torchmetrics' dist_reduce_fx="sum"); the local buffer is left as it was."""
        cm = self.confmat
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized():
            cm = cm.clone()
            dist.all_reduce(cm, op=dist.ReduceOp.SUM, group=process_group)
        return confusion_metrics(cm, groups)


def _torch_average_precision(scores, target, ignore_label, from_logits):
    """lgs_average_precision's semantics in torch lines (sort, searchsorted): CPU tensors and heads wider than one half-wave holds.
    AP_c = (1 / P_c) sum over the positives i of c of TP_c(s_i) / Rank_c(s_i): TP_c(s) = #{positives j of c: prob[j, c] >= s},
    Rank_c(s) = #{all rows j: prob[j, c] >= s}."""
    x = scores.float()
    prob = (torch.softmax(x, 1) if from_logits else x).to(torch.float64)
    n, c = prob.shape
    t = target.long()
    cols = prob.t().contiguous()                                                        # [C, N]
    is_pos = ((t != ignore_label) & (t >= 0) & (t < c))[None, :] & (t[None, :] == torch.arange(c, device=t.device)[:, None])
    p = is_pos.sum(1)
    rank = n - torch.searchsorted(cols.sort(1).values, cols, right=False)               # rows with a score >= this one, per column
    inf = torch.full_like(cols, float("inf"))
    pos_sorted = torch.where(is_pos, cols, inf).sort(1).values                          # the positives first, then the padding
    tp = p[:, None] - torch.searchsorted(pos_sorted, cols, right=False)                 # positives with a score >= this one
    terms = torch.where(is_pos, tp.to(torch.float64) / rank.clamp_min(1).to(torch.float64), torch.zeros_like(cols))
    nan = torch.full((c,), float("nan"), dtype=torch.float64, device=prob.device)
    return torch.where(p > 0, terms.sum(1) / p.clamp_min(1).to(torch.float64), nan)


@torch.no_grad()
def average_precision(scores, target, ignore_label=-1, from_logits=False):
    """scores [N, C] (tensor or SparseTensor), target [N] -> float64 [C] on the scores' device: per class, sklearn's
    average_precision_score of the column against `target == c` (torchmetrics' AveragePrecision(num_classes, average=None)).
    A class without a positive row gives NaN (what a nanmean over steps expects).  Rows whose target is ignore_label or outside
    [0, C) are negatives of every class (label_binarize).  Equal scores share one threshold; -0.0 ties with +0.0.
    from_logits: rank the fp32 softmax of `scores` instead -- bit for bit the result on SegmentationMeter.update(...,
    want_prob=True)'s prob, without the [N, C] fp32 tensor.  HIP tensors of at most 512 (fp32) / 1024 (bf16) classes go to the
    engine (lgs_average_precision: no host sync, two calls give the same bits), everything else takes the same formula in torch.
    NaN scores are not supported: the result of a class they touch is unspecified (nothing is read out of bounds)."""
    scores = _features(scores).detach()
    if scores.dim() != 2:
        raise ValueError("scores must be [N, C], got %s" % (tuple(scores.shape),))
    if target.shape[0] != scores.shape[0]:
        raise ValueError("%d targets for %d rows" % (target.shape[0], scores.shape[0]))
    target = target.to(scores.device)
    be = get_backend()
    if scores.is_cuda and hasattr(be, "average_precision") and be.average_precision_supports(scores):
        return be.average_precision(scores, target, ignore_label, from_logits)
    return _torch_average_precision(scores, target, ignore_label, from_logits)


class AveragePrecisionMeter(nn.Module):
    """Per-class average precision over a run of steps, kept on the device: the reference stacks the [C] result of every validation
    step and takes the nanmean per class (pl_BaselineTrainer.py:380).

        meter = AveragePrecisionMeter(num_labels, ignore_label=config.ignore_label).to(device)
        ap_step = meter.update(soutput.F, target, from_logits=True)          # or: meter.update(prob, target)
        stats = meter.compute()                                              # {"ap": [C], "map": scalar, "steps": [C]}

    Two registered buffers: `ap_sum` (float64 [C], the sum over the steps in which the class had a positive) and `steps` (int64 [C],
    how many those were).  No host sync in update or compute."""

    def __init__(self, num_classes, ignore_label=-1):
        super().__init__()
        self.num_classes = int(num_classes)
        self.ignore_label = int(ignore_label)
        self.register_buffer("ap_sum", torch.zeros(self.num_classes, dtype=torch.float64))
        self.register_buffer("steps", torch.zeros(self.num_classes, dtype=torch.int64))

    @torch.no_grad()
    def update(self, scores, target, from_logits=False):
        """-> this step's average_precision(scores, target) [C]; its classes that are not NaN are added to the buffers"""
        scores = _features(scores)
        if scores.dim() != 2 or scores.shape[1] != self.num_classes:
            raise ValueError("scores must be [N, %d], got %s" % (self.num_classes, tuple(scores.shape)))
        ap = average_precision(scores, target, self.ignore_label, from_logits).to(self.ap_sum.device)
        seen = ~torch.isnan(ap)
        self.ap_sum += torch.where(seen, ap, torch.zeros_like(ap))
        self.steps += seen.to(torch.int64)
        return ap

    def reset(self):
        self.ap_sum.zero_()
        self.steps.zero_()

    @torch.no_grad()
    def compute(self, process_group=None):
        """-> {"ap": [C] mean over the steps that saw the class (NaN: none did), "map": its nanmean over the classes, "steps": [C]}.
        When torch.distributed is initialised the two buffers are sum-reduced over the ranks first; the local ones stay."""
        ap_sum, steps = self.ap_sum, self.steps
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized():
            ap_sum, steps = ap_sum.clone(), steps.clone()
            dist.all_reduce(ap_sum, op=dist.ReduceOp.SUM, group=process_group)
            dist.all_reduce(steps, op=dist.ReduceOp.SUM, group=process_group)
        nan = torch.full_like(ap_sum, float("nan"))
        ap = torch.where(steps > 0, ap_sum / steps.clamp_min(1).to(torch.float64), nan)
        return {"ap": ap, "map": torch.nanmean(ap), "steps": steps}


def fast_hist(pred, label, n):
    """lib/utils.py:92-99 (fast_hist / fast_hist_torch): [n, n] counts of (label, pred) over the rows with 0 <= label < n"""
    if not torch.is_tensor(pred):
        import numpy as np
        return fast_hist(torch.as_tensor(np.asarray(pred)), torch.as_tensor(np.asarray(label)), n).numpy()
    t, p = label.reshape(-1).long(), pred.reshape(-1).long()
    w = ((t >= 0) & (t < n)).long()
    cell = torch.where(w > 0, t * n + p, torch.zeros_like(t))
    return torch.zeros(n * n, dtype=torch.int64, device=t.device).scatter_add_(0, cell, w).view(n, n)


def per_class_iu(hist):
    """lib/utils.py:102-109: diag / (rowsum + colsum - diag), 0/0 = NaN"""
    if not torch.is_tensor(hist):
        return confusion_metrics(torch.as_tensor(hist))["iou"].numpy()
    return confusion_metrics(hist)["iou"]
