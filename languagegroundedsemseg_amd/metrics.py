"""Segmentation metrics of a training / validation step without a host synchronisation.

The reference measures itself in EVERY step: `BaselineTrainerModule.eval_step` (lib/train_test/pl_BaselineTrainer.py:357-378) takes
`pred = soutput.F.max(1)[1]`, `prob = softmax(soutput.F, 1)` and feeds torchmetrics' Precision / Recall / JaccardIndex, once over all
valid rows and once over each of the head / common / tail row subsets.  Everything it logs from them (except the per-class average
precision, which stays on torch and takes `prob` from here) is a function of ONE integer matrix: the confusion matrix of the valid
rows, and -- because `split_items[:, g]` is `valid & group_of_class[target] == g` -- the three subsets are row subsets of the same
matrix.  `SegmentationMeter.update` is one pass over the scores (lgs_seg_metrics on HIP tensors); `compute` derives the numbers on
the device.

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
