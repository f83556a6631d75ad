"""Generates tests/golden/supcon_loss.npz by RUNNING THE REFERENCE'S OWN PointSupConLoss (lib/losses/PointSupConLoss.py, loaded by
file path; it needs torch, numpy and joblib) on the CPU in float32 -- its sample buffers are torch.zeros float32, it has no other
precision.  The fixture is data only: inputs, what the reference passed to np.random.choice, what it drew, and its outputs.

    python tests/golden/make_supcon_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

`loss.num_cores = 1`, so joblib runs the classes one after the other in sorted order, and np.random.choice is wrapped to record every
call: they come in (positive, negative) pairs per class (asserted).  np.random is re-seeded before each run, so the 'mean' and the
'none' run of a case draw the same indices (asserted).

Shared by the four C = 24 cases (key prefix "a_") and by the C = 96 case ("b_"):
    features [257, C] float32, labels [257] int64 in [-1, 13) (-1 = ignored, about 10 %; 9 classes present), preds [257] int64
    (about 25 % wrong), hist [13, 13] int64 (what update_confusion_hist is given; the loss adds 1)
Per case (prefix "a_cos_", "a_cos_preds_", "a_l2_", "a_l2_preds_": P = 2, K = 3;  "b_cos_": P = 1, K = 3):
    classes [U] int64              the classes of the batch, in the reference's order
    pos_cand [U, 257] bool         the candidate set of the positive draw of each class
    neg_p [U, 257] float32         the probability vector p of its negative draw
    pos_idx [257, P], neg_idx [257, K] int64    the indices the reference drew, -1 on ignored rows
    thresholds [3] float64         (contrast_pos_thresh, contrast_neg_thresh, contrast_neg_weight) of the case
    d_pos, d_neg [257] float32     feat_dist of the two sample sets
    mean_loss [], mean_pos_loss [257], mean_neg_loss [257], mean_grad [257, C]    reduction='mean' and the gradient of `loss`
    none_loss [257], none_pos_loss, none_neg_loss, none_grad                      reduction='none' and the gradient of `loss.sum()`
No counted row lies within 1e-3 of a hinge kink (|d_pos - pos_thresh|, |d_neg - neg_thresh|): the generator asserts it and moves to
the next seed otherwise, so the gradient comparison is well defined for every row.  At least 10 % of the counted rows sit on the active
side of each hinge and at least 10 % on the flat side of the negative one (asserted), so both terms carry a gradient."""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, L = 257, 13
PRESENT = [0, 1, 2, 4, 5, 7, 9, 10, 12]
# (distance, preds?, pos_thresh, neg_thresh, neg_weight): 'cos' runs the defaults of config.py; 'l2' distances are a few units, so its
# hinges sit where rows fall on both sides; the P = 1 case has pos_thresh 0.1 because a row that draws itself has d_pos = 0 exactly
CASES = (("a_", 24, 2, 3, [("cos", False, 0.0, 0.6, 1.0), ("cos", True, 0.0, 0.6, 1.0), ("l2", False, 4.5, 6.0, 0.5), ("l2", True, 4.5, 6.0, 0.5)]),
         ("b_", 96, 1, 3, [("cos", False, 0.1, 0.6, 1.0)]))


def load_reference(ref_root):
    path = os.path.join(ref_root, "lib", "losses", "PointSupConLoss.py")
    spec = importlib.util.spec_from_file_location("reference_point_supcon_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(c, seed):
    g = torch.Generator().manual_seed(seed)
    present = torch.tensor(PRESENT)
    labels = present[torch.randint(0, len(PRESENT), (N,), generator=g)]
    labels[:len(PRESENT)] = present                                      # every class at least once
    labels[torch.rand(N, generator=g) < 0.10] = -1
    labels[len(PRESENT)] = -1
    assert sorted(set(labels.tolist()) - {-1}) == PRESENT
    centres = torch.randn(L, c, generator=g)
    # a component all classes share keeps the similarity of two classes near the negative hinge, so both hinges have rows on both sides
    features = (torch.randn(1, c, generator=g) * 0.75 + centres[labels.clamp_min(0)] * 0.7 + torch.randn(N, c, generator=g) * 0.6).float()
    preds = labels.clone()
    wrong = torch.rand(N, generator=g) < 0.25
    preds[wrong] = present[torch.randint(0, len(PRESENT), (int(wrong.sum()),), generator=g)]
    hist = torch.randint(0, 50, (L, L), generator=g)
    hist[hist < 8] = 0
    return features, labels, preds, hist


def run_reference(mod, features, labels, preds, hist, p, k, dist, thresholds, reduction, np_seed):
    config = SimpleNamespace(ignore_label=-1, num_pos_samples=p, num_negative_samples=k, contrast_pos_thresh=thresholds[0],
                             contrast_neg_thresh=thresholds[1], contrast_neg_weight=thresholds[2], representation_distance_type=dist)
    crit = mod.PointSupConLoss(config, L, reduction=reduction)
    crit.num_cores = 1
    crit.update_confusion_hist(hist.clone())
    calls = []
    orig = np.random.choice

    def recording(a, size=None, replace=True, p=None):
        out = orig(a, size, replace, p)
        calls.append((np.array(a).copy(), None if p is None else np.array(p).copy(), np.array(out).copy()))
        return out
    np.random.seed(np_seed)
    mod.np.random.choice = recording
    dists = []
    orig_dist = crit.feat_dist
    crit.feat_dist = lambda a, b, t: dists.append(orig_dist(a, b, t)) or dists[-1]
    try:
        x = features.clone().requires_grad_(True)
        loss, pos_loss, neg_loss = crit(x, labels, preds=preds)
        loss.sum().backward()
    finally:
        mod.np.random.choice = orig
    classes = sorted(set(labels.tolist()) - {-1})
    assert len(calls) == 2 * len(classes) and len(dists) == 2
    pos_idx = np.full((N, p), -1, np.int64)
    neg_idx = np.full((N, k), -1, np.int64)
    pos_cand = np.zeros((len(classes), N), bool)
    neg_p = np.zeros((len(classes), N), np.float32)
    for i, u in enumerate(classes):
        (a_pos, p_pos, out_pos), (a_neg, p_neg, out_neg) = calls[2 * i], calls[2 * i + 1]
        rows = np.nonzero(labels.numpy() == u)[0]
        assert p_pos is None and p_neg is not None and p_neg.shape == (N,) and np.array_equal(a_neg, np.arange(N))
        assert np.array_equal(a_pos, rows), "the positive candidates are all points of the class"
        assert out_pos.shape == (len(rows), p) and out_neg.shape == (len(rows), k)
        pos_cand[i, a_pos] = True
        neg_p[i] = p_neg
        pos_idx[rows], neg_idx[rows] = out_pos, out_neg
    out = dict(classes=np.array(classes, np.int64), pos_cand=pos_cand, neg_p=neg_p, pos_idx=pos_idx, neg_idx=neg_idx,
               d_pos=dists[0].detach().numpy(), d_neg=dists[1].detach().numpy(), loss=loss.detach().numpy(),
               pos_loss=pos_loss.detach().numpy(), neg_loss=neg_loss.detach().numpy(), grad=x.grad.numpy())
    return out


def kink_free(r, labels, thresholds):
    keep = (labels != -1).numpy()
    return bool((np.abs(r["d_pos"][keep] - thresholds[0]) > 1e-3).all() and (np.abs(r["d_neg"][keep] - thresholds[1]) > 1e-3).all())


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LGS_REFERENCE")
    if not ref_root:
        raise SystemExit(__doc__)
    mod = load_reference(ref_root)
    out = {}
    for pre, c, p, k, cases in CASES:
        features, labels, preds, hist = make_inputs(c, 4000 + c)
        out[pre + "features"], out[pre + "labels"], out[pre + "preds"], out[pre + "hist"] = (
            features.numpy(), labels.numpy(), preds.numpy(), hist.numpy())
        for dist, with_preds, *thresholds in cases:
            for np_seed in range(100, 200):
                runs = {red: run_reference(mod, features, labels, preds if with_preds else None, hist, p, k, dist, thresholds, red, np_seed)
                        for red in ("mean", "none")}
                if kink_free(runs["mean"], labels, thresholds):
                    break
            else:
                raise SystemExit("no kink-free seed")
            m, n_ = runs["mean"], runs["none"]
            for key in ("classes", "pos_cand", "neg_p", "pos_idx", "neg_idx", "d_pos", "d_neg", "pos_loss", "neg_loss"):
                assert np.array_equal(m[key], n_[key]), key
            assert m["loss"].shape == () and n_["loss"].shape == (N,)
            ign = (labels == -1).numpy()
            assert (m["d_pos"][ign] == 0).all() and (m["d_neg"][ign] == 0).all() and (m["grad"][ign] == 0).all()
            tag = pre + dist + ("_preds_" if with_preds else "_")
            for key in ("classes", "pos_cand", "neg_p", "pos_idx", "neg_idx", "d_pos", "d_neg"):
                out[tag + key] = m[key]
            out[tag + "thresholds"] = np.array(thresholds, np.float64)
            keep = ~ign
            active = [float((m["pos_loss"][keep] > 0).mean()), float((m["neg_loss"][keep] > 0).mean())]
            assert active[0] > 0.1 and 0.1 < active[1] < 0.9, (tag, active, np.quantile(m["d_pos"][keep], [.1, .5, .9]), np.quantile(m["d_neg"][keep], [.1, .5, .9]))
            for red, r in runs.items():
                for key in ("loss", "pos_loss", "neg_loss", "grad"):
                    out[tag + red + "_" + key] = r[key]
            print("%-14s np seed %d, %d classes, loss %.6f, rows with an active positive / negative hinge %.2f / %.2f" % (
                tag, np_seed, len(m["classes"]), float(m["loss"]), active[0], active[1]))
    path = os.path.join(HERE, "supcon_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
