"""What tests/test_supcon_cpu.py and tests/test_gpu_supcon.py share: the fixture made by the reference's own PointSupConLoss
(tests/golden/supcon_loss.npz, make_supcon_fixtures.py), the structure and distribution checks of the sampler, and the error bar
of the cross-entropy / focal contract (max |err| <= tol * max |ref| per tensor; fp32 tensors 2e-5, bf16 gradients 1e-2)."""
import os

import numpy as np
import torch

TOL_F32, TOL_BF16 = 2e-5, 1e-2
N_LABELS = 13
CASES = {"a_cos_": ("a_", "cos", False, 2, 3), "a_cos_preds_": ("a_", "cos", True, 2, 3), "a_l2_": ("a_", "l2", False, 2, 3),
         "a_l2_preds_": ("a_", "l2", True, 2, 3), "b_cos_": ("b_", "cos", False, 1, 3)}
DRAW_ROUNDS = 32          # calls of `sample` per distribution check: >= 2000 negative draws per class of row on the N = 257 case


def fixture():
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supcon_loss.npz"))
    return {k: fx[k] for k in fx.files}


def case(tag):
    """-> dict of torch tensors (CPU) of one fixture case, the shared inputs under their plain names"""
    shared, dist, with_preds, p, k = CASES[tag]
    fx = fixture()
    out = {key[len(tag):]: torch.from_numpy(v) for key, v in fx.items() if key.startswith(tag) and
           not any(key.startswith(t) and len(t) > len(tag) for t in CASES)}
    for key in ("features", "labels", "preds", "hist"):
        out[key] = torch.from_numpy(fx[shared + key])
    if not with_preds:
        out["preds"] = None
    out.update(distance=dist, P=p, K=k, pos_thresh=float(out["thresholds"][0]), neg_thresh=float(out["thresholds"][1]),
               neg_weight=float(out["thresholds"][2]))
    return out


def make_loss(cs, reduction="mean", device="cpu"):
    from languagegroundedsemseg_amd.losses import PointSupConLoss
    crit = PointSupConLoss(N_LABELS, num_pos_samples=cs["P"], num_negative_samples=cs["K"], pos_thresh=cs["pos_thresh"],
                           neg_thresh=cs["neg_thresh"], neg_weight=cs["neg_weight"], ignore_label=-1, reduction=reduction,
                           distance_type=cs["distance"]).to(device)
    crit.update_confusion_hist(cs["hist"].to(device))
    return crit


def check(what, got, ref, tol, top=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    top = (float(ref.abs().max()) if ref.numel() else 0.0) if top is None else top
    print("%-44s max|err| %.3e  max|ref| %.3e  ratio %.2e (bar %.0e)" % (what, err, top, err / top if top > 0 else 0.0, tol))
    assert err <= tol * top, "%s: max|err| %.3e > %.1e * max|ref| %.3e" % (what, err, tol, top)


def check_structure(crit, labels, preds, pos, neg):
    """every positive has the row's label; every negative a different, counted label of weight > 0 and, with preds, a correctly
    predicted point; rows that are not counted are -1 everywhere"""
    labels, pos, neg = labels.cpu(), pos.cpu(), neg.cpu()
    n, L = labels.shape[0], crit.num_labels
    assert pos.shape == (n, crit.num_pos_samples) and neg.shape == (n, crit.num_negative_samples)
    assert pos.dtype == torch.int64 and neg.dtype == torch.int64
    valid = (labels != crit.ignore_label) & (labels >= 0) & (labels < L)
    assert bool((pos[~valid] == -1).all()) and bool((neg[~valid] == -1).all())
    pv, nv, lv = pos[valid], neg[valid], labels[valid]
    assert bool(((pv >= 0) & (pv < n)).all()) and bool((nv < n).all()) and bool((nv >= -1).all())
    assert bool((labels[pv] == lv[:, None]).all())
    drawn = nv >= 0
    nl = labels[nv.clamp_min(0)]
    assert bool((valid[nv.clamp_min(0)] | ~drawn).all())
    assert bool(((nl != lv[:, None]) | ~drawn).all())
    hist = crit.confusion_hist.cpu()
    assert bool(((hist[lv[:, None].expand_as(nl), nl.clamp(0, L - 1)] > 0) | ~drawn).all())
    if preds is not None:
        correct = labels == preds.cpu()
        assert bool((correct[nv.clamp_min(0)] | ~drawn).all())
    return drawn


def check_distribution(cs, sample):
    """DRAW_ROUNDS calls of sample(seed) -> (pos, neg) against what the reference passed to np.random.choice: per class of row u,
    the frequency f of every candidate class c among the D negative draws against p_c = sum of the recorded p over the points of c,
    and of every point among the D positive draws against 1 / n_u:  |f - p| <= 5 sqrt(p (1 - p) / D) + 1 / D  (binomial 5 sigma,
    about 6e-7 false alarms per bin; deterministic once the seeds are fixed); p == 0 must give f == 0."""
    labels = cs["labels"]
    n = labels.shape[0]
    draws = [sample(1000 + r) for r in range(DRAW_ROUNDS)]
    pos = torch.stack([d[0].cpu() for d in draws])                 # [R, N, P]
    neg = torch.stack([d[1].cpu() for d in draws])
    assert not torch.equal(pos[0], pos[1]) and not torch.equal(neg[0], neg[1])
    worst = 0.0
    for i, u in enumerate(cs["classes"].tolist()):
        rows = (labels == u).nonzero().squeeze(1)
        p_point = cs["neg_p"][i].double()
        nd = neg[:, rows, :].reshape(-1)
        D = nd.numel()
        assert D >= 2000 and bool((nd >= 0).all())
        for c in range(N_LABELS):
            p_c = float(p_point[labels == c].sum())
            f = float((labels[nd] == c).sum()) / D
            if p_c == 0:
                assert f == 0, (u, c, f)
                continue
            bound = 5 * (p_c * (1 - p_c) / D) ** 0.5 + 1.0 / D
            worst = max(worst, abs(f - p_c) / bound)
            assert abs(f - p_c) <= bound, "negatives of class %d: class %d drawn %.4f, reference p %.4f, bound %.4f (D = %d)" % (u, c, f, p_c, bound, D)
        assert float(p_point[labels == -1].sum()) == 0 and bool((labels[nd] != -1).all())
        pd = pos[:, rows, :].reshape(-1)
        D = pd.numel()
        cand = cs["pos_cand"][i]
        assert bool(cand[pd].all()) and torch.equal(cand.nonzero().squeeze(1), rows)
        p_u = 1.0 / rows.numel()
        bound = 5 * (p_u * (1 - p_u) / D) ** 0.5 + 1.0 / D
        f = torch.bincount(pd, minlength=n).double()[rows] / D
        worst = max(worst, float((f - p_u).abs().max()) / bound)
        assert float((f - p_u).abs().max()) <= bound, "positives of class %d: a point drawn %.4f of the time, 1 / n_u = %.4f, bound %.4f" % (
            u, float(f[(f - p_u).abs().argmax()]), p_u, bound)
    print("largest |f - p| / bound: %.2f" % worst)
