"""PointSupConLoss on the engine (k_supcon_sample, k_supcon_fwd, k_supcon_bwd; csrc/lgs_supcon.hip) against

* a float64 torch restatement with autograd -- gather the sampled rows, F.normalize, mean (losses.supcon_distances_torch, the gather
  path CPU tensors take) -- over every access variant (16-byte / element-wise rows), row counts around the workgroup's four rows and
  above one workgroup, P / K at both ends of 1 .. 8, fp32 and bf16, 'cos' and 'l2', with -1 samples, self samples, duplicates, the
  first and the last row, and rows of exactly zero features;
* the reference's own code: tests/golden/supcon_loss.npz (make_supcon_fixtures.py) with the indices it drew;
* the probabilities the reference passed to np.random.choice, for the device sampler.

Bars (the cross-entropy / focal contract, relative to the tensor's maximum): max |err| <= tol * max |ref|; d_pos, d_neg, losses and
fp32 gradients 2e-5, bf16 gradients 1e-2.  A row of exactly zero features has a 'cos' gradient of the order 1e12 (F.normalize divides
by its eps): such rows are held to the bar among themselves and the other rows to the bar over the other rows' maximum -- no less
than one bar over the whole tensor."""
import functools

import pytest
import torch

from languagegroundedsemseg_amd import engine
from languagegroundedsemseg_amd.losses import PointSupConLoss, supcon_distances_torch
from languagegroundedsemseg_amd.metrics import SegmentationMeter

import supcon_reference as sr
from supcon_reference import TOL_BF16, TOL_F32, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 13
NS = (1, 63, 64, 65, 1031)
PKS = ((1, 3), (2, 1), (8, 8))


@functools.lru_cache(maxsize=None)
def inputs(n, c, p, k):
    """bf16-representable features with rows of zeros, labels in [-1, L) plus one above the range, sample indices with the row itself,
    duplicates, -1, row 0 and row N - 1, and upstream gradients"""
    g = torch.Generator().manual_seed(7919 * c + 31 * n + p)
    x = torch.randn(n, c, generator=g).to(torch.bfloat16).double()
    lab = torch.randint(0, L, (n,), generator=g)
    pos = torch.randint(0, n, (n, p), generator=g)
    neg = torch.randint(0, n, (n, k), generator=g)
    zero_rows = [0]
    if n >= 63:
        lab[torch.rand(n, generator=g) < 0.1] = -1
        lab[7], lab[11] = L + 3, -5
        lab[1:7] = torch.arange(6)
        zero_rows = [2, n - 2]
        x[zero_rows] = 0
        rows = torch.arange(n)
        pos[1::5, 0] = rows[1::5]                    # the row itself
        neg[3::7, -1] = -1                           # no sample
        pos[4::9, -1] = -1
        neg[5, :] = -1
        pos[6, :] = -1
        neg[1, :] = 2                                # duplicates, of a zero row
        neg[2, 0], pos[2, 0] = 3, 2                  # a zero row with samples, one of them itself
        neg[3, 0], pos[3, 0] = 0, n - 1
        neg[4, -1], pos[4, -1] = n - 1, 0
        if k > 1:
            neg[8::6, 1] = neg[8::6, 0]
    else:
        x[0] = x[0] * 0 if c == 3 else x[0]
        # the one row can only sample itself or nothing; an all-self slot set would make the 'cos' distance 1 - 1, float64 rounding
        # noise with nothing to hold a relative bar against, so every slot set keeps one empty slot
        pos[0, -1] = -1
        neg[0, -1] = -1
    up_p = (torch.rand(n, generator=g) * 2 - 0.5).float().double()
    up_n = (torch.rand(n, generator=g) * 2 - 0.5).float().double()
    return x, lab, pos, neg, up_p, up_n


def reference(x, lab, pos, neg, up_p, up_n, dist):
    """float64 on the device: d_pos, d_neg, d(d_pos . up_p), d(d_neg . up_n)"""
    xr = x.clone().requires_grad_(True)
    d_pos, d_neg = supcon_distances_torch(xr, lab, pos, neg, -1, L, dist)
    g_pos, = torch.autograd.grad((d_pos * up_p).sum(), xr, retain_graph=True)
    g_neg, = torch.autograd.grad((d_neg * up_n).sum(), xr)
    return d_pos.detach(), d_neg.detach(), g_pos, g_neg


def check_grad(what, got, ref, tol, zero_rows, top=None):
    """rows of zero features among themselves, the rest against the rest's maximum (see the module docstring)"""
    keep = torch.ones(ref.shape[0], dtype=torch.bool)
    keep[zero_rows] = False
    check(what, got.cpu()[keep], ref.cpu()[keep], tol, top)
    check(what + " (zero rows)", got.cpu()[~keep], ref.cpu()[~keep], tol)


SWEEP = [(c, dt) for c in (3, 24, 96, 100, 512) for dt in (torch.float32, torch.bfloat16)]


@pytest.mark.parity("float64 torch restatement with autograd: gather, F.normalize, mean (losses.supcon_distances_torch)")
@pytest.mark.parametrize("c,dtype", SWEEP, ids=["c%d-%s" % (c, str(d).replace("torch.", "")) for c, d in SWEEP])
def test_parity_sweep(c, dtype):
    gtol = TOL_F32 if dtype == torch.float32 else TOL_BF16
    be_hits = 0
    for n in NS:
        for p, k in PKS:
            x, lab, pos, neg, up_p, up_n = (t.to(DEV) for t in inputs(n, c, p, k))
            counted = (lab != -1) & (lab >= 0) & (lab < L)
            zero_rows = (x == 0).all(1).nonzero().squeeze(1).cpu()
            assert n < 63 or zero_rows.numel() >= 2
            for dist in ("cos", "l2"):
                d_pos_ref, d_neg_ref, g_pos_ref, g_neg_ref = reference(x, lab, pos, neg, up_p, up_n, dist)
                tag = "n=%d P=%d K=%d %s" % (n, p, k, dist)
                crit = PointSupConLoss(L, p, k, distance_type=dist, reduction="none")
                for which in ("both", "pos", "neg"):
                    xh = x.to(dtype).requires_grad_(True)
                    engine.dispatch_counts(reset=True)
                    d_pos, d_neg = sr_apply(crit, xh, lab, pos, neg)
                    obj = 0
                    if which in ("both", "pos"):
                        obj = obj + (d_pos * up_p.float()).sum()
                    if which in ("both", "neg"):
                        obj = obj + (d_neg * up_n.float()).sum()
                    obj.backward()
                    hits = engine.dispatch_counts(reset=True)
                    assert sum(v for s, v in hits.items() if "k_supcon_fwd" in s) == 1 and sum(v for s, v in hits.items() if "k_supcon_bwd" in s) == 1, hits
                    be_hits += 1
                    assert d_pos.dtype == torch.float32 and d_pos.shape == (n,) and xh.grad.dtype == dtype and xh.grad.shape == (n, c)
                    if which == "both":
                        check("d_pos " + tag, d_pos, d_pos_ref, TOL_F32)
                        check("d_neg " + tag, d_neg, d_neg_ref, TOL_F32)
                        assert bool((d_pos[~counted] == 0).all()) and bool((d_neg[~counted] == 0).all())
                    want = {"both": g_pos_ref + g_neg_ref, "pos": g_pos_ref, "neg": g_neg_ref}[which]
                    top = None
                    if n == 1 and dist == "cos" and zero_rows.numel() == 0:
                        # one row can only sample itself or nothing, so its exact 'cos' gradient is 0: g / |a| (b^ - s a^) with b^ = a^,
                        # s = 1.  The float64 reference is rounding noise (1e-18) and says nothing about scale; the bar is held
                        # against the size of the two terms that cancel, max |g| / |a| -- what max |ref| is at every other shape
                        top = float(torch.maximum(up_p.abs().max(), up_n.abs().max()) / x.norm(dim=1).min())
                    check_grad("grad(%s) %s" % (which, tag), xh.grad, want, gtol, zero_rows, top)
                    assert bool((xh.grad[~counted] == 0).all()), tag
    assert be_hits == len(NS) * len(PKS) * 2 * 3


def sr_apply(crit, x, lab, pos, neg):
    """(d_pos, d_neg) of the module's fused path: the hinge with thresholds (0, huge) is the identity on them"""
    from languagegroundedsemseg_amd.losses import _SupConFused
    return _SupConFused.apply(x, lab, pos, neg, crit.ignore_label, crit.num_labels, crit.distance_type)


@pytest.mark.parametrize("tag", sorted(sr.CASES))
def test_against_the_reference_code(tag):
    """the reference's outputs with the indices it drew (golden fixture): fp32 on the device against the fixture itself; bf16 against
    the float64 restatement on the features rounded to bf16"""
    cs = sr.case(tag)
    labels, pos, neg = cs["labels"].to(DEV), cs["pos_idx"].to(DEV), cs["neg_idx"].to(DEV)
    preds = cs["preds"].to(DEV) if cs["preds"] is not None else None
    ignored = cs["labels"] == -1
    for reduction in ("mean", "none"):
        crit = sr.make_loss(cs, reduction, DEV)
        x = cs["features"].to(DEV).requires_grad_(True)
        engine.dispatch_counts(reset=True)
        loss, pos_loss, neg_loss = crit(x, labels, preds=preds, pos_indices=pos, neg_indices=neg)
        loss.sum().backward()
        hits = engine.dispatch_counts(reset=True)
        assert any("k_supcon_fwd" in s for s in hits) and any("k_supcon_bwd" in s for s in hits), hits
        check("%s %s loss" % (tag, reduction), loss, cs[reduction + "_loss"], TOL_F32)
        check("%s %s pos_loss" % (tag, reduction), pos_loss, cs[reduction + "_pos_loss"], TOL_F32)
        check("%s %s neg_loss" % (tag, reduction), neg_loss, cs[reduction + "_neg_loss"], TOL_F32)
        check("%s %s grad" % (tag, reduction), x.grad, cs[reduction + "_grad"], TOL_F32)
        assert bool((x.grad.cpu()[ignored] == 0).all()) and bool((pos_loss.cpu()[ignored] == 0).all())
        assert bool((neg_loss.cpu()[ignored] == torch.relu(torch.tensor(cs["neg_thresh"]) - torch.zeros(()))).all())
        # bf16: the restatement in float64 on the rounded features
        xb = cs["features"].to(DEV).to(torch.bfloat16)
        xr = xb.double().requires_grad_(True)
        ref = crit._hinge(*supcon_distances_torch(xr, labels, pos, neg, -1, L, cs["distance"]))
        ref[0].sum().backward()
        xh = xb.clone().requires_grad_(True)
        got = crit(xh, labels, preds=preds, pos_indices=pos, neg_indices=neg)
        got[0].sum().backward()
        # a row within the fp32 rounding of a hinge kink may fall on the other side after the features are rounded: none does
        d_pos, d_neg = supcon_distances_torch(xb.double(), labels, pos, neg, -1, L, cs["distance"])
        keep = ~ignored.to(DEV)
        assert float((d_pos[keep] - cs["pos_thresh"]).abs().min()) > 1e-5 and float((d_neg[keep] - cs["neg_thresh"]).abs().min()) > 1e-5
        for name, a, b in zip(("loss", "pos_loss", "neg_loss"), got, ref):
            check("%s %s bf16 %s" % (tag, reduction, name), a, b, TOL_F32)
        check("%s %s bf16 grad" % (tag, reduction), xh.grad, xr.grad, TOL_BF16)
    d_pos, d_neg = sr_apply(crit, cs["features"].to(DEV), labels, pos, neg)
    check(tag + " d_pos", d_pos, cs["d_pos"], TOL_F32)
    check(tag + " d_neg", d_neg, cs["d_neg"], TOL_F32)


@pytest.mark.parametrize("with_preds", [False, True], ids=["labels", "preds"])
def test_device_sampler_structure_and_reproducibility(with_preds):
    cs = sr.case("a_cos_preds_" if with_preds else "a_cos_")
    crit = sr.make_loss(cs, device=DEV)
    labels = cs["labels"].to(DEV)
    preds = cs["preds"].to(DEV) if with_preds else None
    engine.dispatch_counts(reset=True)
    pos, neg = crit.sample(labels, preds, generator=torch.Generator().manual_seed(5))
    assert sum(v for s, v in engine.dispatch_counts(reset=True).items() if "k_supcon_sample" in s) == 1
    assert pos.device == labels.device and neg.device == labels.device
    assert bool(sr.check_structure(crit, labels, preds, pos, neg).all())
    pos2, neg2 = crit.sample(labels, preds, generator=torch.Generator().manual_seed(5))
    assert torch.equal(pos, pos2) and torch.equal(neg, neg2)
    pos3, neg3 = crit.sample(labels, preds, generator=torch.Generator().manual_seed(6))
    assert not torch.equal(pos, pos3) and not torch.equal(neg, neg3)
    a, b = crit.sample(labels, preds), crit.sample(labels, preds)            # the module-owned generator advances
    assert not torch.equal(a[1], b[1])
    # a single-class batch: no negatives, a finite loss
    one = torch.full((40,), 4, device=DEV)
    one[::7] = -1
    p1, n1 = crit.sample(one, generator=torch.Generator().manual_seed(1))
    assert bool((n1 == -1).all()) and bool((p1[one == 4] >= 0).all()) and bool((p1[one == -1] == -1).all())
    x = torch.randn(40, 24, device=DEV, requires_grad=True)
    loss = crit(x, one)[0]
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize("tag", ["a_cos_", "a_cos_preds_"])
def test_device_sampler_distribution_against_the_reference_probabilities(tag):
    cs = sr.case(tag)
    crit = sr.make_loss(cs, device=DEV)
    labels = cs["labels"].to(DEV)
    preds = cs["preds"].to(DEV) if cs["preds"] is not None else None
    sr.check_distribution(cs, lambda seed: crit.sample(labels, preds, generator=torch.Generator().manual_seed(seed)))


def big_batch(n=1031):
    g = torch.Generator().manual_seed(77)
    labels = torch.randint(-1, L, (n,), generator=g)
    labels[100:200] = 3                                  # consecutive rows of one class
    preds = torch.where(torch.rand(n, generator=g) < 0.7, labels, torch.randint(0, L, (n,), generator=g))
    return labels.to(DEV), preds.to(DEV)


def test_device_sampler_at_1031_rows_with_predictions_and_decorrelated_neighbours():
    labels, preds = big_batch()
    crit = PointSupConLoss(L, 2, 3).to(DEV)
    crit.update_confusion_hist(torch.randint(0, 30, (L, L), generator=torch.Generator().manual_seed(3)).to(DEV))
    pos, neg = crit.sample(labels, preds, generator=torch.Generator().manual_seed(9))
    assert bool(sr.check_structure(crit, labels, preds, pos, neg).all())
    # consecutive rows of one class with >= 32 candidates: fewer than half share their first positive (and their first negative)
    assert int((labels == 3).sum()) >= 100
    first = pos[100:200, 0]
    assert float((first[1:] == first[:-1]).float().mean()) < 0.5
    assert float((neg[101:200, 0] == neg[100:199, 0]).float().mean()) < 0.5
    assert float((pos[100:200, 0] == pos[100:200, 1]).float().mean()) < 0.5


def test_sample_forward_and_backward_run_without_a_host_sync():
    labels, preds = big_batch()
    gen = torch.Generator().manual_seed(1)
    for dtype, dist in ((torch.bfloat16, "cos"), (torch.float32, "l2")):
        crit = PointSupConLoss(L, 2, 3, distance_type=dist).to(DEV)
        x = torch.randn(1031, 96, device=DEV).to(dtype).requires_grad_(True)
        crit(x, labels, preds=preds)[0].backward()             # (first use: library load)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            pos, neg = crit.sample(labels, preds, generator=gen)
            loss, _, _ = crit(x, labels, preds=preds)
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert pos.shape == (1031, 2) and neg.shape == (1031, 3)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad.float()).all()) and float(x.grad.float().abs().max()) > 0


def test_the_knob_switches_between_the_kernels_and_the_torch_path():
    cs = sr.case("a_cos_")
    labels, pos, neg = cs["labels"].to(DEV), cs["pos_idx"].to(DEV), cs["neg_idx"].to(DEV)
    crit = sr.make_loss(cs, "mean", DEV)
    out = {}
    for knob in (1, 0):
        with engine.tuning(SUPCON_FUSED=knob):
            x = cs["features"].to(DEV).requires_grad_(True)
            engine.dispatch_counts(reset=True)
            drawn = crit.sample(labels, generator=torch.Generator().manual_seed(2))
            loss, pos_loss, neg_loss = crit(x, labels, pos_indices=pos, neg_indices=neg)
            loss.backward()
            sites = [s for s in engine.dispatch_counts(reset=True) if "k_supcon" in s]
        sr.check_structure(crit, labels, None, *drawn)
        assert (sorted(s.split("<")[0].split()[0] for s in sites) == ["k_supcon_bwd", "k_supcon_fwd", "k_supcon_sample"]) if knob else not sites, sites
        out[knob] = (loss, pos_loss, neg_loss, x.grad)
    for name, a, b in zip(("loss", "pos_loss", "neg_loss", "grad"), out[1], out[0]):
        check("SUPCON_FUSED 1 against 0: " + name, a, b, TOL_F32)
    assert engine.tuning_get("SUPCON_FUSED") == 1


def test_end_to_end_with_the_meter_confusion_matrix():
    """SegmentationMeter.update x 2 -> update_confusion_hist(meter.confmat) -> loss(features, labels, preds=pred) -> backward"""
    torch.manual_seed(4)
    n = 1031
    labels, _ = big_batch(n)
    meter = SegmentationMeter(L, ignore_label=-1).to(DEV)
    crit = PointSupConLoss(L, 1, 3).to(DEV)
    feats = torch.randn(n, 96, device=DEV).to(torch.bfloat16).requires_grad_(True)
    scores = torch.randn(n, L, device=DEV) + 3.0 * torch.nn.functional.one_hot(labels.clamp_min(0), L)
    meter.update(scores, labels)
    crit(feats, labels)[0].backward()                           # (first use)
    feats.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred = meter.update(scores, labels)
        crit.update_confusion_hist(meter.confmat)
        loss, pos_loss, neg_loss = crit(feats, labels, preds=pred)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(crit.confusion_hist, meter.confmat + 1)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(pos_loss).all()) and bool(torch.isfinite(neg_loss).all())
    assert bool(torch.isfinite(feats.grad.float()).all()) and float(feats.grad.float().abs().max()) > 0


def test_empty_batch_launches_nothing():
    crit = PointSupConLoss(L, 2, 3, reduction="none").to(DEV)
    lab = torch.zeros(0, dtype=torch.int64, device=DEV)
    x = torch.zeros(0, 24, device=DEV, requires_grad=True)
    engine.dispatch_counts(reset=True)
    pos, neg = crit.sample(lab)
    loss, _, _ = crit(x, lab)
    loss.sum().backward()
    assert not [s for s in engine.dispatch_counts(reset=True) if "k_supcon" in s]
    assert pos.shape == (0, 2) and neg.shape == (0, 3) and loss.shape == (0,) and x.grad.shape == (0, 24)
