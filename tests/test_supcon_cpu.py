"""PointSupConLoss without a GPU: the module on CPU tensors against the reference's own code (tests/golden/supcon_loss.npz, written by
make_supcon_fixtures.py from lib/losses/PointSupConLoss.py), and the torch restatement of the two-level sampler against what the
reference passed to np.random.choice.

Bar (the fp32 bar of the cross-entropy / focal contract): max |err| <= 2e-5 * max |ref| per tensor."""
from types import SimpleNamespace

import pytest
import torch

from languagegroundedsemseg_amd.losses import PointSupConLoss, ReferencePointSupConLoss

import supcon_reference as sr
from supcon_reference import TOL_F32, check


@pytest.mark.parametrize("tag", sorted(sr.CASES))
def test_module_reproduces_the_reference_with_its_recorded_indices(tag):
    cs = sr.case(tag)
    ignored = cs["labels"] == -1
    assert 0.05 < float(ignored.float().mean()) < 0.2
    for reduction in ("mean", "none"):
        crit = sr.make_loss(cs, reduction)
        x = cs["features"].clone().requires_grad_(True)
        loss, pos_loss, neg_loss = crit(x, cs["labels"], preds=cs["preds"], pos_indices=cs["pos_idx"], neg_indices=cs["neg_idx"])
        loss.sum().backward()
        check("%s %s loss" % (tag, reduction), loss, cs[reduction + "_loss"], TOL_F32)
        check("%s %s pos_loss" % (tag, reduction), pos_loss, cs[reduction + "_pos_loss"], TOL_F32)
        check("%s %s neg_loss" % (tag, reduction), neg_loss, cs[reduction + "_neg_loss"], TOL_F32)
        check("%s %s grad" % (tag, reduction), x.grad, cs[reduction + "_grad"], TOL_F32)
        assert bool((x.grad[ignored] == 0).all())
        # ignored rows: distance 0, so exactly (relu(-pos_thresh), relu(neg_thresh))
        assert bool((pos_loss[ignored] == 0).all())
        assert bool((neg_loss[ignored] == torch.relu(torch.tensor(cs["neg_thresh"]) - torch.zeros(()))).all())
    from languagegroundedsemseg_amd.losses import supcon_distances_torch
    d_pos, d_neg = supcon_distances_torch(cs["features"], cs["labels"], cs["pos_idx"], cs["neg_idx"], -1, sr.N_LABELS, cs["distance"])
    check(tag + " d_pos", d_pos, cs["d_pos"], TOL_F32)
    check(tag + " d_neg", d_neg, cs["d_neg"], TOL_F32)
    assert bool((d_pos[ignored] == 0).all()) and bool((d_neg[ignored] == 0).all())


def test_labels_outside_the_range_are_ignored_rows_and_minus_one_is_the_zero_row():
    cs = sr.case("a_cos_")
    labels = cs["labels"].clone()
    labels[5], labels[6] = sr.N_LABELS, -7
    pos, neg = cs["pos_idx"].clone(), cs["neg_idx"].clone()
    neg[20:40] = -1
    pos[30:50, 0] = -1
    for dist in ("cos", "l2"):
        crit = PointSupConLoss(sr.N_LABELS, 2, 3, distance_type=dist, reduction="none")
        x = cs["features"].clone().requires_grad_(True)
        loss, pos_loss, neg_loss = crit(x, labels, pos_indices=pos, neg_indices=neg)
        loss.sum().backward()
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(x.grad).all())
        for r in (5, 6):
            assert float(pos_loss[r]) == 0 and abs(float(neg_loss[r]) - 0.6) < 1e-7 and bool((x.grad[r] == 0).all())
        counted = [r for r in range(20, 30) if labels[r] != -1]
        f = cs["features"][counted]
        want = torch.full((len(counted),), 1.0) if dist == "cos" else torch.sqrt((f * f).sum(1) + 1e-7)
        # all-zero samples: cosine similarity 0, l2 distance sqrt(|a|^2 + 1e-7)
        from languagegroundedsemseg_amd.losses import supcon_distances_torch
        _, dn = supcon_distances_torch(cs["features"], labels, pos, neg, -1, sr.N_LABELS, dist)
        check("d_neg of rows without a negative (%s)" % dist, dn[counted], want, TOL_F32)


@pytest.mark.parametrize("with_preds", [False, True], ids=["labels", "preds"])
def test_sampler_structure_on_cpu(with_preds):
    cs = sr.case("a_cos_preds_" if with_preds else "a_cos_")
    crit = sr.make_loss(cs)
    g = torch.Generator().manual_seed(5)
    pos, neg = crit.sample(cs["labels"], cs["preds"], generator=g)
    drawn = sr.check_structure(crit, cs["labels"], cs["preds"], pos, neg)
    assert bool(drawn.all())
    # the same generator state gives the same indices, another seed gives others
    pos2, neg2 = crit.sample(cs["labels"], cs["preds"], generator=torch.Generator().manual_seed(5))
    assert torch.equal(pos, pos2) and torch.equal(neg, neg2)
    pos3, neg3 = crit.sample(cs["labels"], cs["preds"], generator=torch.Generator().manual_seed(6))
    assert not torch.equal(pos, pos3) and not torch.equal(neg, neg3)
    # the module-owned generator advances: two calls differ
    a, b = crit.sample(cs["labels"], cs["preds"]), crit.sample(cs["labels"], cs["preds"])
    assert not torch.equal(a[1], b[1])
    sr.check_structure(crit, cs["labels"], cs["preds"], *b)


def test_single_class_batch_has_no_negatives_and_a_finite_loss():
    torch.manual_seed(0)
    labels = torch.full((40,), 4)
    labels[::7] = -1
    x = torch.randn(40, 12, requires_grad=True)
    for dist in ("cos", "l2"):
        crit = PointSupConLoss(sr.N_LABELS, 2, 3, distance_type=dist)
        pos, neg = crit.sample(labels, generator=torch.Generator().manual_seed(1))
        assert bool((neg == -1).all()) and bool((pos[labels == 4] >= 0).all()) and bool((pos[labels == -1] == -1).all())
        loss, pos_loss, neg_loss = crit(x, labels)
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())
    # a class whose only possible negatives were all mispredicted has none either
    labels = torch.tensor([0, 0, 1, 1])
    preds = torch.tensor([1, 1, 1, 1])
    crit = PointSupConLoss(3, 1, 2)
    pos, neg = crit.sample(labels, preds, generator=torch.Generator().manual_seed(1))
    assert bool((neg[2:] == -1).all()) and bool((neg[:2] >= 2).all()) and bool((pos[:2] <= 1).all()) and bool((pos[2:] >= 2).all())


@pytest.mark.parametrize("tag", ["a_cos_", "a_cos_preds_"])
def test_sampler_distribution_against_the_reference_probabilities(tag):
    cs = sr.case(tag)
    crit = sr.make_loss(cs)
    sr.check_distribution(cs, lambda seed: crit.sample(cs["labels"], cs["preds"], generator=torch.Generator().manual_seed(seed)))


def test_reference_constructor_reads_every_config_field():
    config = SimpleNamespace(ignore_label=255, num_pos_samples=2, num_negative_samples=5, contrast_neg_thresh=0.7, contrast_pos_thresh=0.1,
                             contrast_neg_weight=0.5, representation_distance_type="l2")
    crit = ReferencePointSupConLoss(config, 20, reduction="none")
    assert (crit.ignore_label, crit.num_pos_samples, crit.num_negative_samples) == (255, 2, 5)
    assert (crit.neg_thresh, crit.pos_thresh, crit.neg_weight, crit.distance_type, crit.reduction) == (0.7, 0.1, 0.5, "l2", "none")
    assert crit.num_labels == 20 and crit.temperature == 0.07 and crit.base_temperature == 0.07 and crit.config is config
    assert crit.confusion_hist.shape == (20, 20) and crit.confusion_hist.dtype == torch.int64
    for field in vars(config):
        partial = SimpleNamespace(**{k: v for k, v in vars(config).items() if k != field})
        with pytest.raises(AttributeError):
            ReferencePointSupConLoss(partial, 20)
    made = PointSupConLoss.from_config(config, 20)
    assert type(made) is ReferencePointSupConLoss and made.reduction == "mean"
    hist = torch.arange(400).view(20, 20)
    made.update_confusion_hist(hist)
    assert torch.equal(made.confusion_hist, hist + 1) and made.confusion_hist.dtype == torch.int64
    labels = torch.randint(0, 20, (50,))
    labels[:5] = 255
    loss, pos_loss, neg_loss = made(torch.randn(50, 8), labels, anchor_feats=None, preds=labels)
    assert loss.shape == () and pos_loss.shape == (50,) and neg_loss.shape == (50,)
    assert bool((neg_loss[:5] == torch.relu(torch.tensor(0.7))).all())


def test_bad_distance_type_raises():
    with pytest.raises(ValueError):
        PointSupConLoss(20, distance_type="l1")
    config = SimpleNamespace(ignore_label=-1, num_pos_samples=1, num_negative_samples=3, contrast_neg_thresh=0.6, contrast_pos_thresh=0.0,
                             contrast_neg_weight=1.0, representation_distance_type="dot")
    with pytest.raises(ValueError):
        ReferencePointSupConLoss(config, 20)
    with pytest.raises(ValueError):
        PointSupConLoss(20)(torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.int64))


def test_the_knob_is_listed():
    from languagegroundedsemseg_amd import engine, tuning
    rows = {name: (d, v) for name, d, v, _ in engine.tuning_table()}
    assert rows["SUPCON_FUSED"][0] == 1
    assert any(name == "SUPCON_FUSED" for _, name, _, _, _ in tuning.describe())
    with engine.tuning(SUPCON_FUSED=0):
        assert engine.tuning_get("SUPCON_FUSED") == 0
    assert engine.tuning_get("SUPCON_FUSED") == rows["SUPCON_FUSED"][1]
