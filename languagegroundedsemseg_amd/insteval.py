"""Instance-segmentation AP from "clusters exist" to mAP.

Mirror of the reference's downstream/insseg/datasets/evaluation/evaluate_semantic_instance.py (`Evaluator`: add_gt / add_prediction /
evaluate -> mAP, mAP50, mAP25) and of the trainer's `nms` (downstream/insseg/lib/pl_Trainer.py:370-387), split in two:

  device  per scene ONE pass over the proposals' member lists (`instance_overlaps`, engine entry point lgs_inst_overlap): the distinct
          ground-truth instance ids with their point counts, the [P, g_cap] intersection counts and the void count of every proposal.
          That is all `assign_instances_for_scan` computes with one [N] pass per (proposal, ground-truth instance).
  host    `InstanceEvaluator.evaluate()`: the greedy matching and the AP integral of `evaluate_matches` over those compact tables, in
          float64 -- O(P G) data per scene.

Proposals travel as CSR lists (`Proposals`), not as a dense [P, N] mask; `Proposals.to_instances()` gives the reference's dict where the
masks are still wanted (`write_to_benchmark`)."""
from collections import namedtuple

import numpy as np
import torch

from .me.core import get_backend

OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)     # evaluate_semantic_instance.py:55
MIN_REGION_SIZE = 10                                       # :57
MAX_G_CAP = 4096
STATUS_BITS = {1: "more distinct ground-truth instance ids than g_cap", 2: "a proposal member outside [0, n)",
               4: "a score column outside [0, c)", 8: "a valid class id < 1"}

OverlapTables = namedtuple("OverlapTables", "gt_id gt_count inter prop_void status")


class Proposals:
    """Instance proposals of one scene as device (or host) tensors: member [M] int32 point indices grouped by proposal, offsets [P + 1]
    int32, label [P] int64 (the argmax column; -1 where unknown), label_id [P] int64 (class_mapping[label]), conf [P] float32."""

    def __init__(self, member, offsets, label, label_id, conf, n_points):
        self.member, self.offsets, self.label, self.label_id, self.conf, self.n_points = member, offsets, label, label_id, conf, int(n_points)

    def __len__(self):
        return self.offsets.shape[0] - 1

    @property
    def device(self):
        return self.member.device

    def to(self, device):
        return Proposals(*(t.to(device) for t in (self.member, self.offsets, self.label, self.label_id, self.conf)), self.n_points)

    def select(self, keep):
        """the proposals whose entry of `keep` [P] bool is set, in order"""
        sizes = (self.offsets[1:] - self.offsets[:-1]).long()
        member = self.member[torch.repeat_interleave(keep, sizes)]
        offsets = torch.cat([sizes.new_zeros(1), torch.cumsum(sizes[keep], 0)]).int()
        return Proposals(member, offsets, self.label[keep], self.label_id[keep], self.conf[keep], self.n_points)

    def to_instances(self):
        """-> {i: {"conf": 0-d float32 array, "label_id": 0-d tensor, "pred_mask": int32 [N] array}}, what Clustering.get_instances returns"""
        member, offsets = self.member.cpu().numpy(), self.offsets.cpu().numpy()
        conf, label_id = self.conf.cpu().numpy(), self.label_id.cpu()
        out = {}
        for i in range(len(self)):
            mask = np.zeros(self.n_points, dtype=np.int32)
            mask[member[offsets[i]:offsets[i + 1]]] = 1
            out[i] = {"conf": conf[i], "label_id": label_id[i], "pred_mask": mask}
        return out

    @classmethod
    def from_instances(cls, instances, n_points=None, device="cpu"):
        """the reference's dict -> Proposals (np.nonzero per mask; `label` is unknown there and set to -1)"""
        members, sizes, label_id, conf = [], [], [], []
        for key in instances:
            inst = instances[key]
            mask = np.asarray(inst["pred_mask"])
            n_points = mask.shape[0] if n_points is None else n_points
            idx = np.nonzero(mask)[0]
            members.append(idx.astype(np.int32))
            sizes.append(idx.shape[0])
            label_id.append(int(inst["label_id"]))
            conf.append(float(np.asarray(inst["conf"], dtype=np.float32)))
        member = np.concatenate(members) if members else np.zeros(0, np.int32)
        offsets = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int32)
        return cls(torch.from_numpy(member).to(device), torch.from_numpy(offsets).to(device),
                   torch.full((len(sizes),), -1, dtype=torch.int64, device=device),
                   torch.tensor(label_id, dtype=torch.int64).to(device), torch.tensor(conf, dtype=torch.float32).to(device),
                   0 if n_points is None else n_points)


def merge_dual_set(a, b, labels=(10, 12, 16)):
    """The trainer's `nms` (pl_Trainer.py:370-387): a's proposals whose label_id is not in `labels`, then b's whose label_id is."""
    if a.n_points != b.n_points:
        raise ValueError("merge_dual_set: proposals of %d and of %d points" % (a.n_points, b.n_points))
    in_a = torch.isin(a.label_id, torch.as_tensor(labels, dtype=a.label_id.dtype, device=a.label_id.device))
    in_b = torch.isin(b.label_id, torch.as_tensor(labels, dtype=b.label_id.dtype, device=b.label_id.device))
    a, b = a.select(~in_a), b.select(in_b)
    return Proposals(torch.cat([a.member, b.member]), torch.cat([a.offsets, b.offsets[1:] + a.offsets[-1]]), torch.cat([a.label, b.label]),
                     torch.cat([a.label_id, b.label_id]), torch.cat([a.conf, b.conf]), a.n_points)


def check_valid_class_ids(valid_class_ids):
    """-> ascending int64 array; every id must be >= 1 (with that, no ground-truth id below 1000 names an instance)"""
    valid = np.sort(np.asarray(valid_class_ids, dtype=np.int64).reshape(-1))
    if valid.size and valid[0] < 1:
        raise ValueError("instance evaluation: valid class id %d < 1 (valid_class_ids must all be >= 1)" % valid[0])
    return valid


def check_g_cap(g_cap):
    if not 1 <= g_cap <= MAX_G_CAP:
        raise ValueError("instance evaluation: g_cap = %d is outside 1 .. %d" % (g_cap, MAX_G_CAP))
    return int(g_cap)


def _fused(t):
    be = get_backend()
    return t.is_cuda and hasattr(be, "inst_overlap") and be.inst_eval_fused()


def _overlaps_torch(member, offsets, gt_ids, valid, g_cap):
    """the definition of lgs_inst_overlap's integer tables in torch lines (CPU tensors, INST_EVAL_FUSED=0); synchronises on a device"""
    dev = member.device
    p, n = offsets.shape[0] - 1, gt_ids.shape[0]
    ids = gt_ids.long()
    inst = (ids != 0) & torch.isin(torch.div(ids, 1000, rounding_mode="floor"), valid)
    uniq, counts = torch.unique(ids[inst], return_counts=True)
    status = 0
    if uniq.shape[0] > g_cap:
        status |= 1
        uniq, counts = uniq[:g_cap], counts[:g_cap]
    g = uniq.shape[0]
    gt_id = torch.zeros(g_cap, dtype=torch.int64, device=dev)
    gt_count = torch.zeros(g_cap, dtype=torch.int32, device=dev)
    gt_id[:g], gt_count[:g] = uniq, counts.int()
    mem = member.long()
    sizes = (offsets[1:] - offsets[:-1]).long()
    prop = torch.repeat_interleave(torch.arange(p, device=dev), sizes)
    ok = (mem >= 0) & (mem < n)
    if not bool(ok.all()):
        status |= 2
        mem, prop = mem[ok], prop[ok]
    mg = ids[mem]
    slot = torch.searchsorted(uniq, mg).clamp_(max=max(g - 1, 0))
    hit = inst[mem] & (uniq[slot] == mg) if g else torch.zeros_like(mem, dtype=torch.bool)
    inter = torch.bincount(prop[hit] * g_cap + slot[hit], minlength=p * g_cap).view(p, g_cap).int()
    void = ~inst[mem]
    prop_void = torch.bincount(prop[void], minlength=p).int()
    return OverlapTables(gt_id, gt_count, inter, prop_void, torch.tensor([status], dtype=torch.int32, device=dev))


def proposal_conf(member, offsets, score_col, scores, mode):
    """conf[q] = max / mean (mode "max" / "mean") of scores[member of q, score_col[q]], float32 [P]; NaN for an empty proposal.
    HIP tensors: lgs_inst_overlap (the max is torch.max's, the mean is summed in fp64 and rounded once)."""
    p = offsets.shape[0] - 1
    if _fused(member) and scores.dtype in (torch.float32, torch.bfloat16):
        return get_backend().inst_overlap(member, offsets, scores.shape[0], g_cap=1, scores=scores, score_col=score_col.int(), score_mode=mode)[4]
    sizes = (offsets[1:] - offsets[:-1]).long()
    prop = torch.repeat_interleave(torch.arange(p, device=member.device), sizes)
    vals = scores[member.long(), score_col.long()[prop]].float()
    if mode == "max":
        conf = torch.full((p,), float("-inf"), device=member.device).scatter_reduce_(0, prop, vals, "amax")
    else:
        conf = (torch.zeros(p, dtype=torch.float64, device=member.device).index_add_(0, prop, vals.double()) / sizes.double()).float()
    return torch.where(sizes > 0, conf, torch.full_like(conf, float("nan")))


def instance_overlaps(proposals, gt_ids, valid_class_ids, g_cap=1024):
    """-> OverlapTables(gt_id [g_cap] int64, gt_count [g_cap] int32, inter [P, g_cap] int32, prop_void [P] int32, status [1] int32) on the
    proposals' device.  A point's id g names a ground-truth instance iff g != 0 and g // 1000 is a valid class id; every other point is
    void.  Unused slots have gt_count == 0; which slot an id takes is unspecified.  status: see STATUS_BITS.  HIP tensors go to the engine
    (no host sync); CPU tensors, and HIP tensors under INST_EVAL_FUSED=0, take the same definition in torch lines."""
    g_cap = check_g_cap(g_cap)
    dev = proposals.device
    if isinstance(valid_class_ids, torch.Tensor) and valid_class_ids.device == dev and valid_class_ids.dtype == torch.int64:
        valid = valid_class_ids                    # the caller's checked, ascending table (InstanceEvaluator's)
    else:
        valid = torch.from_numpy(check_valid_class_ids(valid_class_ids.cpu() if isinstance(valid_class_ids, torch.Tensor) else valid_class_ids)).to(dev)
    gt = torch.as_tensor(gt_ids).to(dev).long().reshape(-1)
    if _fused(proposals.member):
        gt_id, gt_count, inter, prop_void, _, status = get_backend().inst_overlap(proposals.member, proposals.offsets, gt.shape[0], gt, valid, g_cap)
        return OverlapTables(gt_id, gt_count, inter, prop_void, status)
    return _overlaps_torch(proposals.member, proposals.offsets, gt, valid, g_cap)


def _status_text(status):
    return "; ".join(text for bit, text in STATUS_BITS.items() if status & bit)


def _curve_ap(y_score, y_true, hard_false_negatives):
    """the precision / recall curve over the distinct scores and its integral (evaluate_semantic_instance.py:176-223), on arrays"""
    order = np.argsort(y_score, kind="stable")
    ys, cs = y_score[order], np.cumsum(y_true[order])
    _, first = np.unique(ys, return_index=True)
    n_true = cs[-1] if cs.size else 0.0
    below = np.append(cs, 0.0)[first - 1]                  # positives under each threshold (first == 0 reads the appended 0)
    tp = n_true - below
    fp = ys.size - first - tp
    fn = below + hard_false_negatives
    precision = np.append(tp / (tp + fp), 1.0)             # the last point of the curve is artificial
    recall = np.append(tp / (tp + fn), 0.0)
    widths = np.convolve(np.concatenate([recall[:1], recall, [0.0]]), [-0.5, 0, 0.5], "valid")
    return float(np.dot(precision, widths))


class InstanceEvaluator:
    """The reference's `Evaluator` over compact per-scene tables.  add_gt(gt_ids, id) / add_prediction(x, id) with x a `Proposals` or the
    reference's dict; evaluate() -> (all_ap, all_ap_50, all_ap_25) and leaves `ap` (float64 [C, 10], overlaps 0.5 .. 0.9, 0.25) and `avgs`
    (the dict of compute_averages).  Once both halves of a scene are there its tables are computed (on the device for device inputs,
    without a host sync), copied to pinned host memory and the device buffers dropped; evaluate() synchronises once."""

    overlaps = OVERLAPS
    min_region_size = MIN_REGION_SIZE

    def __init__(self, CLASS_LABELS, VALID_CLASS_IDS, g_cap=1024):
        self.CLASS_LABELS = list(CLASS_LABELS)
        self.VALID_CLASS_IDS = np.asarray(VALID_CLASS_IDS, dtype=np.int64).reshape(-1)
        if len(self.CLASS_LABELS) != self.VALID_CLASS_IDS.shape[0]:
            raise ValueError("InstanceEvaluator: %d class labels for %d valid class ids" % (len(self.CLASS_LABELS), self.VALID_CLASS_IDS.shape[0]))
        self._valid_sorted = check_valid_class_ids(self.VALID_CLASS_IDS)
        self.g_cap = check_g_cap(g_cap)
        self._valid_dev = {}
        self._gt, self._pred, self._scenes = {}, {}, {}      # halves that wait for the other one; finished scenes in prediction order
        self.ap = self.avgs = None

    def _valid_on(self, dev):
        if dev not in self._valid_dev:
            self._valid_dev[dev] = torch.from_numpy(self._valid_sorted).to(dev)
        return self._valid_dev[dev]

    def add_gt(self, gt_ids, id):
        self._gt[id] = gt_ids
        self._pair(id)

    def add_prediction(self, instance_info, id):
        self._pred[id] = instance_info
        self._scenes.setdefault(id, None)
        self._pair(id)

    def _pair(self, id):
        if id not in self._gt or id not in self._pred:
            return
        gt, pred = self._gt.pop(id), self._pred.pop(id)
        gt = gt if isinstance(gt, torch.Tensor) else torch.from_numpy(np.asarray(gt))
        if not isinstance(pred, Proposals):
            pred = Proposals.from_instances(pred, n_points=gt.shape[0])
        dev = pred.device if pred.device.type == "cuda" else gt.device
        pred = pred if pred.device == dev else pred.to(dev)
        t = instance_overlaps(pred, gt, self._valid_on(dev), self.g_cap)
        p = len(pred)
        sizes = pred.offsets[1:] - pred.offsets[:-1]
        ints = torch.cat([t.gt_count, t.inter.reshape(-1), t.prop_void, sizes.int(), t.status])
        longs = torch.cat([t.gt_id, pred.label_id.long()])
        conf = pred.conf.float()
        if dev.type == "cuda":
            host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in (ints, longs, conf)]
            for h, x in zip(host, (ints, longs, conf)):
                h.copy_(x, non_blocking=True)
            ints, longs, conf = host
        self._scenes[id] = (p, ints, longs, conf)

    def _tables(self, id):
        if self._scenes[id] is None:
            raise KeyError("InstanceEvaluator: scene %r has predictions and no ground truth" % (id,))
        p, ints, longs, conf = self._scenes[id]
        g = self.g_cap
        ints, longs = ints.numpy(), longs.numpy()
        status = int(ints[-1])
        if status:
            raise RuntimeError("InstanceEvaluator: scene %r: %s (status %d, g_cap %d)" % (id, _status_text(status), status, g))
        gt_count, inter = ints[:g].astype(np.int64), ints[g:g + p * g].reshape(p, g).astype(np.int64)
        prop_void, sizes = ints[g + p * g:g + p * g + p].astype(np.int64), ints[g + p * g + p:g + p * g + 2 * p].astype(np.int64)
        return longs[:g], gt_count, inter, prop_void, sizes, longs[g:], conf.numpy().astype(np.float64)

    def _scene_records(self, id, rec):
        """the matching of evaluate_matches for one scene, the ten overlaps side by side: appends (class, mask [10], score [10], true)"""
        gt_id, gt_count, inter, prop_void, sizes, label_id, conf = self._tables(id)
        valid, th = self.VALID_CLASS_IDS, self.overlaps
        n_cls = valid.shape[0]
        used = np.nonzero(gt_count > 0)[0]
        used = used[np.argsort(gt_id[used])]                                   # np.unique's order: ascending id
        gt_id, gt_count, inter = gt_id[used], gt_count[used], inter[:, used]
        cls_of = {int(c): i for i, c in enumerate(valid)}
        gt_cls = np.array([cls_of[int(c)] for c in gt_id // 1000], dtype=np.int64)
        keep = np.nonzero(np.isin(label_id, valid) & (sizes >= self.min_region_size))[0]      # the predictions the reference keeps
        pr_cls = np.array([cls_of[int(c)] for c in label_id[keep]], dtype=np.int64)
        inter, prop_void, sizes, conf = inter[keep], prop_void[keep], sizes[keep], conf[keep]
        same = (pr_cls[:, None] == gt_cls[None, :]) & (inter > 0)              # [P, G]: the reference's matched_gt / matched_pred
        iou = np.where(same, inter / np.maximum(gt_count[None, :] + sizes[:, None] - inter, 1).astype(np.float64), 0.0)
        big = gt_count >= self.min_region_size
        has_gt, has_pred = np.zeros(n_cls, bool), np.zeros(n_cls, bool)
        has_gt[gt_cls[big]] = True
        has_pred[pr_cls] = True
        hard_fn = np.zeros((n_cls, th.shape[0]), dtype=np.int64)
        # greedy assignment: ground truths in id order, their predictions in order; `visited` is shared by the scene's ground truths
        visited = np.zeros((keep.shape[0], th.shape[0]), bool)
        for gi in np.nonzero(big)[0]:
            matched = np.zeros(th.shape[0], bool)
            score = np.full(th.shape[0], -np.inf)
            for pi in np.nonzero(iou[:, gi] > th.min())[0]:
                act = (iou[pi, gi] > th) & ~visited[pi]
                second = act & matched
                if second.any():            # the lower score of the two is a false positive; the prediction stays unvisited
                    rec.append((gt_cls[gi], second, np.minimum(score, conf[pi]), 0.0))
                    score = np.where(second, np.maximum(score, conf[pi]), score)
                first = act & ~matched
                matched |= first
                score = np.where(first, conf[pi], score)
                visited[pi] |= first
            hard_fn[gt_cls[gi]] += ~matched
            if matched.any():
                rec.append((gt_cls[gi], matched, score, 1.0))
        # predictions without a ground truth over the threshold: false positives unless mostly void / small ground truth
        if keep.shape[0]:
            best = iou.max(1) if iou.shape[1] else np.zeros(keep.shape[0])
            ignore = (prop_void + np.where(same & ~big[None, :], inter, 0).sum(1)) / sizes.astype(np.float64)
            fp = ~(best[:, None] > th[None, :]) & (ignore[:, None] <= th[None, :])
            for pi in np.nonzero(fp.any(1))[0]:
                rec.append((pr_cls[pi], fp[pi], np.full(th.shape[0], conf[pi]), 0.0))
        return has_gt, has_pred, hard_fn

    def evaluate(self):
        for dev in self._valid_dev:                          # the one synchronisation: the scenes' tables are on their way to the host
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
        n_cls, n_th = len(self.CLASS_LABELS), self.overlaps.shape[0]
        rec = []
        has_gt, has_pred = np.zeros(n_cls, bool), np.zeros(n_cls, bool)
        hard_fn = np.zeros((n_cls, n_th), dtype=np.int64)
        for id in self._scenes:
            g, p, h = self._scene_records(id, rec)
            has_gt |= g
            has_pred |= p
            hard_fn += h
        r_cls = np.array([r[0] for r in rec], dtype=np.int64)
        r_mask = np.array([r[1] for r in rec], dtype=bool).reshape(-1, n_th)
        r_score = np.array([r[2] for r in rec], dtype=np.float64).reshape(-1, n_th)
        r_true = np.array([r[3] for r in rec], dtype=np.float64)
        ap = np.full((n_cls, n_th), np.nan)
        for li in range(n_cls):
            if not has_gt[li]:
                continue                                   # NaN: no ground truth of the class
            if not has_pred[li]:
                ap[li] = 0.0
                continue
            rows = np.nonzero(r_cls == li)[0]
            for oi in range(n_th):
                sel = rows[r_mask[rows, oi]]
                ap[li, oi] = _curve_ap(r_score[sel, oi], r_true[sel], hard_fn[li, oi])
        self.ap = ap
        self.avgs = self.compute_averages(ap)
        return self.avgs["all_ap"], self.avgs["all_ap_50%"], self.avgs["all_ap_25%"]

    def compute_averages(self, ap):
        """evaluate_semantic_instance.py:232-249 on ap [C, 10] (the overlap axis first, as the reference's index expression lays it out)"""
        o50, o25 = np.isclose(self.overlaps, 0.5), np.isclose(self.overlaps, 0.25)
        avgs = {"all_ap": np.nanmean(np.ascontiguousarray(ap[:, ~o25].T)), "all_ap_50%": np.nanmean(np.ascontiguousarray(ap[:, o50].T)),
                "all_ap_25%": np.nanmean(np.ascontiguousarray(ap[:, o25].T)), "classes": {}}
        for li, name in enumerate(self.CLASS_LABELS):
            avgs["classes"][name] = {"ap": np.average(ap[li, ~o25]), "ap50%": np.average(ap[li, o50]), "ap25%": np.average(ap[li, o25])}
        return avgs
