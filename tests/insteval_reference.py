"""Slow, literal numpy statement of the instance evaluation, for the tests: the per-scene tables by the definition of lgs_inst_overlap
(include/lgs_engine.h) and the matching / AP of the reference's evaluate_matches
(downstream/insseg/datasets/evaluation/evaluate_semantic_instance.py:83-230) as plain loops over those tables.
tests/test_insteval_cpu.py holds it to tests/golden/insteval.npz, which the reference's own Evaluator produced."""
import numpy as np

OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
MIN_REGION = 10


def tables(member, offsets, gt_ids, valid_class_ids):
    """-> dict: gt_id [G] ascending, gt_count [G], inter [P, G], prop_void [P], size [P] (a member outside [0, n) is skipped)"""
    gt_ids = np.asarray(gt_ids, dtype=np.int64)
    n = gt_ids.shape[0]
    is_inst = (gt_ids != 0) & np.isin(gt_ids // 1000, np.asarray(valid_class_ids))
    gt_id, gt_count = np.unique(gt_ids[is_inst], return_counts=True)
    p = len(offsets) - 1
    inter = np.zeros((p, gt_id.shape[0]), dtype=np.int64)
    prop_void = np.zeros(p, dtype=np.int64)
    for q in range(p):
        for i in member[offsets[q]:offsets[q + 1]]:
            if not 0 <= i < n:
                continue
            if is_inst[i]:
                inter[q, np.searchsorted(gt_id, gt_ids[i])] += 1
            else:
                prop_void[q] += 1
    return {"gt_id": gt_id, "gt_count": gt_count.astype(np.int64), "inter": inter, "prop_void": prop_void,
            "size": np.diff(np.asarray(offsets)).astype(np.int64)}


def average_precision(y_score, y_true, hard_false_negatives):
    """the precision / recall curve over the distinct scores, point by point; -> (ap, number of curve points)"""
    order = np.argsort(y_score, kind="stable")
    y_score, y_true = y_score[order], y_true[order]
    thresholds = sorted(set(y_score.tolist()))
    n_true = float(y_true.sum())
    precision, recall = [], []
    for t in thresholds:
        first = int(np.searchsorted(y_score, t, side="left"))
        below = float(y_true[:first].sum())
        tp = n_true - below
        fp = len(y_score) - first - tp
        fn = below + hard_false_negatives
        precision.append(tp / (tp + fp))
        recall.append(tp / (tp + fn))
    precision.append(1.0)
    recall.append(0.0)
    padded = [recall[0]] + recall + [0.0]
    ap = 0.0
    for k in range(len(precision)):
        ap += precision[k] * (0.5 * padded[k] - 0.5 * padded[k + 2])      # np.convolve(recall_for_conv, [-0.5, 0, 0.5], 'valid')[k]
    return ap, len(precision)


def evaluate(scenes, valid_class_ids):
    """scenes: list of (tables dict, label_id [P], conf [P]) -> (ap [C, 10], curve points [C, 10])"""
    valid = [int(c) for c in valid_class_ids]
    ap = np.full((len(valid), len(OVERLAPS)), np.nan)
    points = np.zeros((len(valid), len(OVERLAPS)), dtype=np.int64)
    for oi, th in enumerate(OVERLAPS):
        for li, cls in enumerate(valid):
            y_true, y_score = [], []
            hard_fn, has_gt, has_pred = 0, False, False
            for t, label_id, conf in scenes:
                preds = [q for q in range(len(label_id)) if int(label_id[q]) == cls and t["size"][q] >= MIN_REGION]
                gts_all = [g for g in range(len(t["gt_id"])) if int(t["gt_id"][g]) // 1000 == cls]
                gts = [g for g in gts_all if t["gt_count"][g] >= MIN_REGION]
                has_gt |= bool(gts)
                has_pred |= bool(preds)

                def iou(q, g):
                    i = int(t["inter"][q, g])
                    return float(i) / (int(t["gt_count"][g]) + int(t["size"][q]) - i)

                visited = set()
                for g in gts:
                    matched, score = False, -np.inf
                    for q in preds:
                        if t["inter"][q, g] == 0 or q in visited or not iou(q, g) > th:
                            continue
                        c = float(conf[q])
                        if matched:                       # the lower of the two scores is a false positive
                            y_true.append(0.0)
                            y_score.append(min(score, c))
                            score = max(score, c)
                        else:
                            matched, score = True, c
                            visited.add(q)
                    if matched:
                        y_true.append(1.0)
                        y_score.append(score)
                    else:
                        hard_fn += 1
                for q in preds:
                    if any(t["inter"][q, g] > 0 and iou(q, g) > th for g in gts_all):
                        continue
                    ignore = int(t["prop_void"][q]) + sum(int(t["inter"][q, g]) for g in gts_all if t["gt_count"][g] < MIN_REGION)
                    if float(ignore) / int(t["size"][q]) <= th:
                        y_true.append(0.0)
                        y_score.append(float(conf[q]))
            if has_gt and has_pred:
                ap[li, oi], points[li, oi] = average_precision(np.array(y_score, dtype=np.float64), np.array(y_true, dtype=np.float64), hard_fn)
            elif has_gt:
                ap[li, oi] = 0.0
    return ap, points
