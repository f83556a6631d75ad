"""Generates tests/golden/insteval.npz by RUNNING THE REFERENCE'S OWN Evaluator
(downstream/insseg/datasets/evaluation/evaluate_semantic_instance.py, loaded by file path) on synthetic scenes.  The fixture is data
only: the scenes and what the reference computed on them.

    python tests/golden/make_insteval_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

The reference predates numpy 1.24, imports plyfile / imageio for file I/O that is not used here, and imports its helpers as
`datasets.evaluation.scannet_benchmark_utils`: np.float / np.bool are aliased, the two libraries are stubbed in sys.modules and the three
packages are stubbed too, the last with its real __path__.

3 scenes of 4000 points; valid classes 1 .. 6 ("c1" .. "c6"), class ids 0 and 7 are invalid.  Instances are contiguous runs of the point
index, predictions are jittered runs with 2 % holes.  Ground truth exists for classes 1, 2, 3, 5 (and the invalid ones), predictions carry
the labels 1, 2, 3, 4 (and the invalid ones): class 5 has ground truth and no prediction (AP 0), class 4 predictions only (NaN), class 6
neither (NaN).  5 % of the points have id 0 and 1 % id -1.  Confidences come from a grid of 8 values.
Per scene k (prefix "s<k>_"):
    gt_ids [4000] int64
    member [M] int32, offsets [P + 1] int32, label_id [P] int64, conf [P] float32      the predictions in CSR form, in dict order
    ref_pred [K] int64             the predictions assign_instances_for_scan kept (valid label, >= 10 points), in its order
    ref_vert_count, ref_void [K] int64       their vert_count / void_intersection
    ref_match [T, 3] int64         (prediction, ground-truth id, intersection) of every matched pair
    ref_gt [G, 2] int64            (instance id, vert_count) of the ground-truth instances of the valid classes
Overall: valid_class_ids [6], ap [6, 10] float64 of evaluate_matches (overlaps 0.5 .. 0.9, 0.25), avgs [3] (all_ap, all_ap_50%,
all_ap_25%), class_avgs [6, 3] (ap, ap50%, ap25% of compute_averages' per-class dict), seed.
The generator asserts that the scenes reach every branch of evaluate_matches (see `check_branches`) and moves to the next seed
otherwise."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N, N_INST, N_SCENES = 4000, 40, 3
VALID = np.arange(1, 7)
LABELS = ["c%d" % i for i in VALID]
GT_CLASSES = np.array([0, 1, 2, 3, 5, 7])
PRED_CLASSES = np.array([0, 1, 2, 3, 4, 7])


def load_reference(ref_root):
    ev_dir = os.path.join(ref_root, "downstream", "insseg", "datasets", "evaluation")
    np.float, np.bool = float, bool
    for name, path in (("datasets", None), ("datasets.evaluation", None),
                       ("datasets.evaluation.scannet_benchmark_utils", os.path.join(ev_dir, "scannet_benchmark_utils"))):
        m = types.ModuleType(name)
        m.__path__ = [path] if path else []
        sys.modules[name] = m
    sys.modules["imageio"] = types.ModuleType("imageio")
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    sys.modules["plyfile"] = ply
    spec = importlib.util.spec_from_file_location("reference_evaluate_semantic_instance", os.path.join(ev_dir, "evaluate_semantic_instance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_scene(seed):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(20, N - 20, 20), N_INST - 1, replace=False))
    cuts[5] = cuts[4] + 6                                   # instance 5: a ground truth under 10 points
    seg = np.searchsorted(cuts, np.arange(N), side="right")
    cls = GT_CLASSES[rng.integers(0, len(GT_CLASSES), N_INST)]
    cls[5] = 1
    cls[10] = cls[11] = 2                                   # two neighbours of one class: one prediction can cover both
    cls[20] = 0                                             # a run of an invalid class: a prediction on it is mostly void
    gt = (cls[seg] * 1000 + seg + 1).astype(np.int64)
    hole = rng.random(N)
    gt[hole < 0.05] = 0
    gt[hole > 0.99] = -1
    bounds = np.concatenate([[0], cuts, [N]])
    preds = {}

    def add(a, b, label):
        a, b = max(0, int(a)), min(N, int(b))
        mask = np.zeros(N, np.int32)
        mask[a:b] = 1
        mask[rng.random(N) < 0.02] = 0
        preds[len(preds)] = {"conf": np.float32(rng.integers(0, 8) / 8.0), "label_id": np.int64(label), "pred_mask": mask}

    for s in range(N_INST):
        lo, hi = bounds[s], bounds[s + 1]
        for _ in range(rng.integers(0, 3)):
            label = cls[s] if rng.random() < 0.8 else PRED_CLASSES[rng.integers(0, len(PRED_CLASSES))]
            if label == 5:
                label = 4                                   # class 5 is never predicted; class 4 is predicted and has no ground truth
            add(lo + rng.integers(-15, 15), hi + rng.integers(-15, 15), label)
    add(bounds[10], bounds[12], 2)                          # over 0.25 IoU with both neighbours when they are of similar size
    add(bounds[20], bounds[21], 1)                          # valid label on the invalid run
    add(bounds[30], bounds[30] + 6, 3)                      # a prediction under 10 points
    add(bounds[15] + 2, bounds[16] - 2, cls[15] if cls[15] in (1, 2, 3) else 1)
    add(bounds[15] + 1, bounds[16] - 1, cls[15] if cls[15] in (1, 2, 3) else 1)      # two predictions on one ground truth
    return gt, preds


def iou(i, a, b):
    return float(i) / (a + b - i)


def check_branches(matches, scenes, ap):
    seen = dict.fromkeys(("gt with two predictions over 0.5", "prediction over 0.25 with two ground truths", "ignored unmatched prediction",
                          "false-positive unmatched prediction", "ground truth under 10 points", "prediction under 10 points",
                          "prediction with an invalid label", "tied confidences in one class"), False)
    for k, (gt, preds) in enumerate(scenes):
        for name in LABELS:
            confs = [float(p["confidence"]) for p in matches[k]["pred"][name]]
            seen["tied confidences in one class"] |= len(set(confs)) < len(confs)
            for g in matches[k]["gt"][name]:
                over = [p for p in g["matched_pred"] if iou(p["intersection"], g["vert_count"], p["vert_count"]) > 0.5]
                seen["gt with two predictions over 0.5"] |= g["vert_count"] >= 10 and len(over) >= 2
                seen["ground truth under 10 points"] |= g["vert_count"] < 10
            for p in matches[k]["pred"][name]:
                ious = [iou(g["intersection"], g["vert_count"], p["vert_count"]) for g in p["matched_gt"]]
                seen["prediction over 0.25 with two ground truths"] |= sum(x > 0.25 for x in ious) >= 2
                if not any(x > 0.5 for x in ious):
                    ignore = p["void_intersection"] + sum(g["intersection"] for g in p["matched_gt"] if g["vert_count"] < 10)
                    seen["ignored unmatched prediction" if ignore / p["vert_count"] > 0.5 else "false-positive unmatched prediction"] = True
        for p in preds.values():
            seen["prediction under 10 points"] |= int(p["label_id"]) in VALID and np.count_nonzero(p["pred_mask"]) < 10
            seen["prediction with an invalid label"] |= int(p["label_id"]) not in VALID
    missing = [k for k, v in seen.items() if not v]
    # class 5: ground truth, no prediction; class 4: predictions only; class 6: neither; classes 1 - 3: a number
    if not (np.all(ap[4] == 0.0) and np.all(np.isnan(ap[3])) and np.all(np.isnan(ap[5])) and np.all(np.isfinite(ap[:3]))):
        missing.append("AP 0 / NaN / number per class")
    return missing


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["LGS_REFERENCE"]
    mod = load_reference(ref_root)
    for seed in range(100):
        ev = mod.Evaluator(LABELS, VALID)
        scenes = [make_scene(1000 * seed + k) for k in range(N_SCENES)]
        matches = {}
        for k, (gt, preds) in enumerate(scenes):
            ev.add_gt(gt, k)
            ev.add_prediction(preds, k)
            gt2pred, pred2gt = ev.assign_instances_for_scan(k)
            matches[k] = {"gt": gt2pred, "pred": pred2gt}
        ap = ev.evaluate_matches(matches)
        missing = check_branches(matches, scenes, ap[0])
        if not missing:
            break
        print("seed %d misses: %s" % (seed, ", ".join(missing)))
    else:
        raise SystemExit("no seed reaches every branch")
    avgs = ev.compute_averages(ap)
    out = {"valid_class_ids": VALID.astype(np.int64), "ap": ap[0].astype(np.float64), "seed": np.int64(seed),
           "avgs": np.array([avgs["all_ap"], avgs["all_ap_50%"], avgs["all_ap_25%"]], dtype=np.float64),
           "class_avgs": np.array([[avgs["classes"][n][k] for k in ("ap", "ap50%", "ap25%")] for n in LABELS], dtype=np.float64)}
    for k, (gt, preds) in enumerate(scenes):
        idx = [np.nonzero(p["pred_mask"])[0].astype(np.int32) for p in preds.values()]
        kept = sorted((p for name in LABELS for p in matches[k]["pred"][name]), key=lambda p: p["pred_id"])
        out["s%d_gt_ids" % k] = gt
        out["s%d_member" % k] = np.concatenate(idx)
        out["s%d_offsets" % k] = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int32)
        out["s%d_label_id" % k] = np.array([int(p["label_id"]) for p in preds.values()], dtype=np.int64)
        out["s%d_conf" % k] = np.array([p["conf"] for p in preds.values()], dtype=np.float32)
        out["s%d_ref_pred" % k] = np.array([int(p["filename"].split("/")[1]) for p in kept], dtype=np.int64)
        out["s%d_ref_vert_count" % k] = np.array([p["vert_count"] for p in kept], dtype=np.int64)
        out["s%d_ref_void" % k] = np.array([p["void_intersection"] for p in kept], dtype=np.int64)
        out["s%d_ref_match" % k] = np.array([(int(p["filename"].split("/")[1]), g["instance_id"], g["intersection"])
                                             for p in kept for g in p["matched_gt"]], dtype=np.int64).reshape(-1, 3)
        out["s%d_ref_gt" % k] = np.array([(g["instance_id"], g["vert_count"]) for name in LABELS for g in matches[k]["gt"][name]],
                                         dtype=np.int64).reshape(-1, 2)
    path = os.path.join(HERE, "insteval.npz")
    np.savez_compressed(path, **out)
    print("seed %d -> %s (%d bytes); ap =\n%s" % (seed, path, os.path.getsize(path), np.round(ap[0], 4)))


if __name__ == "__main__":
    main()
