"""Losses of the hot path on the engine's kernels.

* fused_cross_entropy  -- nn.CrossEntropyLoss(ignore_index=-1, reduction='mean') on [N,200] logits
                          (/root/reference/lib/train_test/pl_BaselineTrainer.py:94-99,350): one kernel computes
                          the loss and the gradient.
* fused_focal_loss, FocalLoss, loss_by_name -- the other two outcomes of the reference's loss selector
                          (lib/utils.py:112-118 `loss_by_name`, lib/losses/FocalLoss.py): focal loss with per-category weights and
                          nn.CrossEntropyLoss(weight=...), both on lgs_focal_forward_backward.
* ContrastiveLanguageLoss -- the CLIP text-anchor hinge loss
                          (/root/reference/lib/losses/ContrastiveLanguageLoss.py:97-194, feat_dist :73-95) written
                          on the dense MFMA contraction S = normalize(F) . normalize(T)^T plus index gathers, which
                          is mathematically the reference's [N,1+K,C] gather + bmm.
* fused_instance_offset_losses -- the two PointGroup offset losses of downstream/insseg/lib/pl_Trainer.py:286-298 from the instance
                          table of the batch (instances.instance_info): one streaming kernel per direction (lgs_insttarget.hip).
* PointSupConLoss         -- the supervised point-contrastive baseline (lib/losses/PointSupConLoss.py): samples drawn on the device
                          (k_supcon_sample), distances and their gradient from (1 + P + K) row reads per point (lgs_supcon.hip).
"""
import torch
import torch.nn as nn

from . import instances, tuning
from .me.core import get_backend


def _reduced(logits, labels, ignore_index, alpha, gamma, denom, grad_scale=None, inv_denom=None):
    """one backend call of a reduced loss -> (loss, dlogits, inv_denom).  gamma None: the unweighted kernel (cross_entropy)"""
    be = get_backend()
    if gamma is None:
        return be.cross_entropy(logits, labels, ignore_index, want_grad=False, grad_scale=grad_scale, inv_valid=inv_denom)
    return be.focal_loss(logits, labels, ignore_index, alpha, gamma, denom=denom, grad_scale=grad_scale, inv_denom=inv_denom)


def _rows(logits, labels, ignore_index, alpha, gamma, row_grad=None):
    be = get_backend()
    if gamma is None:
        return be.cross_entropy_rows(logits, labels, ignore_index, row_grad=row_grad)
    return be.focal_loss_rows(logits, labels, ignore_index, alpha, gamma, row_grad=row_grad)


class _FusedReduced(torch.autograd.Function):
    """reduced cross-entropy (gamma None: k_ce_fwd_bwd) or focal loss / weighted cross-entropy (k_focal_fwd_bwd).  forward: loss only;
    backward: the same kernel again writes d(logits) already scaled by the upstream gradient (one read of the logits instead of a
    write + read-modify-write of an [N, C] gradient tensor); nothing [N, C] is saved but the logits."""

    @staticmethod
    def forward(ctx, logits, labels, alpha, gamma, ignore_index, denom):
        loss, _, inv_denom = _reduced(logits, labels, ignore_index, alpha, gamma, denom)
        ctx.save_for_backward(logits, labels, inv_denom, alpha)
        ctx.gamma, ctx.ignore_index, ctx.denom = gamma, ignore_index, denom
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, inv_denom, alpha = ctx.saved_tensors
        _, dlogits, _ = _reduced(logits, labels, ctx.ignore_index, alpha, ctx.gamma, ctx.denom, grad_scale=g, inv_denom=inv_denom)
        return dlogits, None, None, None, None, None


class _FusedRows(torch.autograd.Function):
    """reduction='none' of either kernel: forward = the per-row losses, backward = the same kernel with the upstream per-row gradient
    as its row factor (lgs_ce_forward_backward_rows, lgs_focal_forward_backward) -- no [N, C] softmax is kept between the two."""

    @staticmethod
    def forward(ctx, logits, labels, alpha, gamma, ignore_index):
        ctx.save_for_backward(logits, labels, alpha)
        ctx.gamma, ctx.ignore_index = gamma, ignore_index
        return _rows(logits, labels, ignore_index, alpha, gamma)

    @staticmethod
    def backward(ctx, g):
        logits, labels, alpha = ctx.saved_tensors
        return _rows(logits, labels, ctx.ignore_index, alpha, ctx.gamma, row_grad=g), None, None, None, None


def fused_cross_entropy(logits, labels, ignore_index=-1, reduction="mean", weight=None):
    """softmax cross-entropy; logits may be bf16 or fp32, any class count the kernel's half-wave holds (the backend's class_limit);
    wider heads go through torch's device op.
    reduction='mean': over the non-ignored rows (pl_BaselineTrainer.py:350 with balanced_category_sampling off);
    reduction='none': per-row losses [N], 0 for ignored rows -- what `self.criterion` returns when the fine-tune script's
    --balanced_category_sampling True is on (scripts/train_models.sh:37, pl_BaselineTrainer.py:94), the input of
    sample_categories_for_balancing.
    weight: [C] per-class weights, nn.CrossEntropyLoss(weight=...) (lib/utils.py:116): rows are weight[label] * CE on the focal kernel
    at gamma 0, and 'mean' divides by the sum of weight[label] over the counted rows (torch's rule; an all-ignored batch gives 0).
    weight=None is the unweighted kernel, untouched."""
    if reduction not in ("mean", "none"):
        raise ValueError("fused_cross_entropy: reduction must be 'mean' or 'none'")
    if weight is not None:
        return _focal_dispatch(logits, labels, weight, 0.0, ignore_index, reduction, "weight")
    backend = get_backend()
    # (a dtype the kernel does not take goes to it within the fp32 limit and gets its refusal, not the torch path)
    if hasattr(backend, "cross_entropy") and logits.shape[1] <= (backend.class_limit(logits.dtype) or backend.class_limit(torch.float32)):
        if reduction == "none":
            return _FusedRows.apply(logits, labels, None, None, ignore_index)
        return _FusedReduced.apply(logits, labels, None, None, ignore_index, "valid")
    return torch.nn.functional.cross_entropy(logits.float(), labels, ignore_index=ignore_index, reduction=reduction)


class _FocalRowsTorch(torch.autograd.Function):
    """the closed form of the focal kernel in plain torch (CPU tensors, a backend without focal_loss, heads wider than the kernel's
    class limit): per-row losses [N] with the engine's conventions, gradient coef (p - onehot) -- not autograd through
    (1 - pt) ** gamma, which is NaN at pt == 1 for gamma < 1.  float32 arithmetic (float64 logits stay float64)."""

    @staticmethod
    def forward(ctx, logits, labels, alpha, gamma, ignore_index):
        z = logits if logits.dtype == torch.float64 else logits.float()
        n, c = z.shape
        valid = (labels != ignore_index) & (labels >= 0) & (labels < c)
        lab = torch.where(valid, labels, torch.zeros_like(labels))[:, None]
        mx = z.max(1, keepdim=True).values
        e = torch.exp(z - mx)
        se = e.sum(1)
        at_label = torch.arange(c, device=z.device)[None, :] == lab
        u = e.masked_fill(at_label, 0.0).sum(1) / se                   # 1 - pt without the subtraction
        pt = e.gather(1, lab).squeeze(1) / se
        log_pt = torch.where(u < 0.5, torch.log1p(-u), (z.gather(1, lab) - mx).squeeze(1) - torch.log(se))
        a = alpha.to(z.dtype)[lab.squeeze(1)] if alpha is not None else torch.ones_like(se)
        if gamma == 0:
            ug, coef = torch.ones_like(u), a
        else:
            ug = u ** gamma
            coef = a * (ug - gamma * pt * torch.where(u > 0, ug / u, torch.zeros_like(u)) * log_pt)
        zero = torch.zeros_like(se)
        ctx.save_for_backward(e / se[:, None], at_label, torch.where(valid, coef, zero), u)
        ctx.dtype = logits.dtype
        return torch.where(valid, -a * ug * log_pt, zero)

    @staticmethod
    def backward(ctx, g):
        p, at_label, coef, u = ctx.saved_tensors
        cs = (coef * g.to(coef.dtype))[:, None]
        return torch.where(at_label, -cs * u[:, None], cs * p).to(ctx.dtype), None, None, None, None


def _focal_dispatch(logits, labels, alpha, gamma, ignore_index, reduction, mean_over):
    """the one body of fused_focal_loss and fused_cross_entropy(weight=...): the kernel where it applies, else the torch closed form.
    mean_over: what 'mean' divides by -- 'valid' (the counted rows) or 'weight' (the sum of alpha[label])."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError("logits must be [N, C] and labels [N], got %s and %s" % (tuple(logits.shape), tuple(labels.shape)))
    c = logits.shape[1]
    if alpha is not None:
        if not isinstance(alpha, torch.Tensor):
            alpha = torch.as_tensor(alpha, dtype=torch.float32)
        if alpha.dim() != 1 or alpha.shape[0] != c:
            raise ValueError("per-class weights must be [%d] (one per class), got %s" % (c, tuple(alpha.shape)))
        alpha = alpha.detach().to(device=logits.device, dtype=torch.float32).contiguous()
    gamma = float(gamma)
    if not gamma >= 0.0:
        raise ValueError("gamma must be >= 0, got %r" % (gamma,))
    labels = labels.long()
    backend = get_backend()
    if logits.is_cuda and hasattr(backend, "focal_loss") and c <= backend.class_limit(logits.dtype):
        if reduction == "none":
            return _FusedRows.apply(logits, labels, alpha, gamma, ignore_index)
        denom = "sum" if reduction == "sum" else mean_over
        return _FusedReduced.apply(logits, labels, alpha, gamma, ignore_index, denom)
    rows = _FocalRowsTorch.apply(logits, labels, alpha, gamma, ignore_index)
    if reduction == "none":
        return rows
    total = rows.sum()
    if reduction == "sum":
        return total
    valid = (labels != ignore_index) & (labels >= 0) & (labels < c)
    if mean_over == "valid":
        return total / valid.sum().clamp_min(1).to(total.dtype)
    s = (alpha[labels.clamp(0, c - 1)] * valid).sum().to(total.dtype)
    return total / torch.where(s > 0, s, torch.ones_like(s))


def fused_focal_loss(logits, labels, alpha=None, gamma=2.0, ignore_index=-1, reduction="mean"):
    """FocalLoss(alpha, gamma) of lib/losses/FocalLoss.py on the engine: per row -alpha[l] (1 - pt)^gamma log(pt) and its gradient
    from one kernel per direction (lgs_focal_forward_backward; gamma == 0 is class-weighted cross-entropy), bf16 or fp32 logits.
    A row is counted iff its label is neither ignore_index nor outside [0, C) -- the predicate of every loss of the engine.
    reduction='mean': the mean over the counted rows, the reference's `loss.mean()` after its mask (NOT a weighted mean);
    reduction='sum':  the plain sum;
    reduction='none': [N] fp32 with 0 at ignored rows, the convention of fused_cross_entropy(reduction='none') and what
        sample_categories_for_balancing takes.  The reference returns the compacted counted rows instead (its caller handles both
        shapes, pl_BaselineTrainer.py:344-347): ours[labels != ignore_index] == reference.
    An all-ignored or empty batch gives 0 as a device tensor (the reference: the Python float 0.).
    Rows whose label's probability rounds to 1 take the limit: loss 0, gradient 0 (gamma > 0).  The reference computes 1 - exp(log pt),
    rounds the loss to exactly 0 from pt = 1 - 6e-8 on and yields NaN gradients there for gamma < 1 (0^(gamma-1)); here 1 - pt is
    the exponential sum without the label's term over the full sum, so the result is finite and slightly more accurate.
    CPU tensors, a backend without the kernel and heads wider than the backend's class_limit take the same closed form in
    plain torch.  gamma < 0 or an alpha that is not [C] raises ValueError."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError('Reduction must be one of: "mean", "sum", "none".')
    return _focal_dispatch(logits, labels, alpha, gamma, ignore_index, reduction, "valid")


def _flatten_scores(x, y):
    """(N, C, d1, ..., dK) scores and (N, d1, ..., dK) labels -> [M, C] and [M] (FocalLoss.py:59-64)"""
    if x.dim() > 2:
        c = x.shape[1]
        x = x.permute(0, *range(2, x.dim()), 1).reshape(-1, c)
        y = y.reshape(-1)
    return x, y


class FocalLoss(nn.Module):
    """Drop-in for lib/losses/FocalLoss.py: the same constructor, `__repr__` and forward(x, y), on fused_focal_loss (see there for
    the reduction='none' shape and the saturated rows).  alpha is a buffer, so it follows `.to()`."""

    def __init__(self, alpha=None, gamma=0., reduction='mean', ignore_index=-100):
        if reduction not in ('mean', 'sum', 'none'):
            raise ValueError('Reduction must be one of: "mean", "sum", "none".')
        super().__init__()
        if alpha is not None and not isinstance(alpha, torch.Tensor):
            if not hasattr(alpha, "__len__"):
                raise TypeError("alpha must be a [C] tensor of per-class weights or None (as nn.NLLLoss(weight=...) in the "
                                "reference), got %r" % (alpha,))
            alpha = torch.as_tensor(alpha, dtype=torch.float32)
        if float(gamma) < 0:
            raise ValueError("gamma must be >= 0, got %r" % (gamma,))
        self.register_buffer("alpha", alpha)
        self.gamma = gamma
        self.ignore_index = ignore_index
        self.reduction = reduction

    def __repr__(self):
        arg_keys = ['alpha', 'gamma', 'ignore_index', 'reduction']
        arg_strs = [f'{k}={getattr(self, k)}' for k in arg_keys]
        return f'{type(self).__name__}({", ".join(arg_strs)})'

    def forward(self, x, y):
        x, y = _flatten_scores(x, y)
        return fused_focal_loss(x, y, alpha=self.alpha, gamma=self.gamma, ignore_index=self.ignore_index, reduction=self.reduction)


class FusedCrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight, ignore_index, reduction) as loss_by_name builds it, on fused_cross_entropy; `weight` is a buffer.
    Labels outside [0, C) are ignored rows (nn.CrossEntropyLoss raises) and a batch without a counted row gives 0 (there: NaN)."""

    def __init__(self, weight=None, ignore_index=-100, reduction='mean'):
        if reduction not in ('mean', 'sum', 'none'):
            raise ValueError('Reduction must be one of: "mean", "sum", "none".')
        super().__init__()
        if weight is not None and not isinstance(weight, torch.Tensor):
            weight = torch.as_tensor(weight, dtype=torch.float32)
        self.register_buffer("weight", weight)
        self.ignore_index = ignore_index
        self.reduction = reduction

    def extra_repr(self):
        return "ignore_index=%s, reduction=%r, weighted=%s" % (self.ignore_index, self.reduction, self.weight is not None)

    def forward(self, x, y):
        x, y = _flatten_scores(x, y)
        if self.reduction == 'sum':            # (the unweighted kernel has no 'sum': gamma 0 of the focal kernel is the same rows)
            return fused_focal_loss(x, y, alpha=self.weight, gamma=0.0, ignore_index=self.ignore_index, reduction='sum')
        return fused_cross_entropy(x, y, ignore_index=self.ignore_index, reduction=self.reduction, weight=self.weight)


def loss_by_name(loss_name, ignore_index=0, alpha=0.5, gamma=2.0, reduction='mean', weight=None):
    """lib/utils.py:112-118, what `init_criterions` calls (pl_BaselineTrainer.py:96-99, downstream/insseg/lib/pl_Trainer.py:74):
    'focal' -> FocalLoss(alpha, gamma), 'cross_entropy' -> the weighted / unweighted cross-entropy module, anything else -> None.
    Both modules run the fused kernels in forward(x, y).  As in the reference, alpha must be the per-class weight tensor
    (`dataset.category_weights`) or None: the signature's default 0.5 is rejected there by nn.NLLLoss and here by FocalLoss."""
    if loss_name == 'focal':
        return FocalLoss(alpha, gamma, reduction=reduction, ignore_index=ignore_index)
    elif loss_name == 'cross_entropy':
        return FusedCrossEntropyLoss(weight=weight, ignore_index=ignore_index, reduction=reduction)
    else:
        return None


class _ClipSimilarity(torch.autograd.Function):
    """S[n,a] = <f_n/|f_n|, t_a/|t_a|>; backward only w.r.t. the features (anchors are frozen CLIP embeddings;
    a learned projection of the anchors gets its gradient through `anchor_grad=True`)."""

    @staticmethod
    def forward(ctx, feats, anchors, anchor_grad):
        sim, inv = get_backend().clip_similarity(feats, anchors)
        ctx.anchor_grad = anchor_grad
        ctx.save_for_backward(feats, anchors, sim, inv)
        return sim

    @staticmethod
    def backward(ctx, gs):
        feats, anchors, sim, inv = ctx.saved_tensors
        gs = gs.float()
        tn = torch.nn.functional.normalize(anchors.float(), dim=1)
        # dS/df = (t^ - s f^) / |f|
        fh = feats.float() * inv[:, None]
        gf = (gs @ tn - (gs * sim).sum(1, keepdim=True) * fh) * inv[:, None]
        ga = None
        if ctx.anchor_grad:
            an = anchors.float().norm(dim=1, keepdim=True).clamp_min(1e-12)
            gt = gs.t() @ fh                                  # d/d t^
            ga = (gt - (gt * tn).sum(1, keepdim=True) * tn) / an
            ga = ga.to(anchors.dtype)
        return gf.to(feats.dtype), ga, None


def clip_similarity(feats, anchors):
    return _ClipSimilarity.apply(feats, anchors, anchors.requires_grad)


class _ClipLossFused(torch.autograd.Function):
    """(d_pos, d_neg, pred[, sim]) of the text-anchor loss in ONE pass over the features (lgs_clip_loss_forward: MFMA
    contraction with the gathers, the arg-max and 1/|f| in its epilogue -- the [N, A] similarity matrix is never written
    unless asked for); backward = lgs_clip_loss_backward, a streaming kernel that uses the 4-sparse upstream gradient."""

    @staticmethod
    def forward(ctx, feats, anchors, labels, neg, ignore_label, want_sim):
        be = get_backend()
        d_pos, d_neg, pred, saved, sim = be.clip_loss_forward(feats, anchors, labels, neg, ignore_label, want_sim)
        ctx.ignore_label = ignore_label
        ctx.anchors = anchors if anchors.requires_grad else None      # a learned projection of the anchors (clip_models.py:192-200)
        ctx.save_for_backward(*saved, d_pos, d_neg)
        ctx.mark_non_differentiable(pred)
        if sim is None:
            sim = d_pos.new_empty(0)
        ctx.mark_non_differentiable(sim)
        return d_pos, d_neg, pred, sim

    @staticmethod
    def backward(ctx, g_dpos, g_dneg, _gp, _gs):
        *saved, d_pos, d_neg = ctx.saved_tensors
        be = get_backend()
        gf = be.clip_loss_backward(tuple(saved), d_pos, d_neg, g_dpos, g_dneg, ctx.ignore_label) if ctx.needs_input_grad[0] else None
        ga = None
        if ctx.anchors is not None and ctx.needs_input_grad[1]:
            # d/dT^ = G^T F^ on the weight-gradient kernels (lgs_clip_loss_backward_anchors), then through t^ = t / |t|
            gt = be.clip_loss_backward_anchors(tuple(saved), g_dpos, g_dneg, ctx.ignore_label)
            tn = saved[1]
            an = ctx.anchors.detach().float().norm(dim=1, keepdim=True).clamp_min(1e-12)
            ga = ((gt - (gt * tn).sum(1, keepdim=True) * tn) / an).to(ctx.anchors.dtype)
        return gf, ga, None, None, None, None


def feature_sim(output_feats, anchor_feats):
    """lib/losses/utils.py:80-103, cosine branch: S[n, a] = <f^_n, t^_a> (attribute anchors: the plain ones, :83-84)."""
    if anchor_feats.dim() == 3:
        anchor_feats = anchor_feats[:, 0, :]
    return clip_similarity(output_feats.detach(), anchor_feats.detach())


class ContrastiveLanguageLoss(nn.Module):
    """cos variant of the reference loss: per voxel one positive anchor (its class) and K negatives drawn
    uniformly from the other classes (clip_uniform_sampling=True, ContrastiveLanguageLoss.py:138-144):
        d = 1 - mean_j <f^, t^_j>;   loss = relu(d_pos - pos_thresh) + neg_weight * relu(neg_thresh - d_neg)
    ignored voxels contribute 0 but count in the mean (feat_dist zeroes them, :94).
    Negatives are sampled on the device (no host loop / joblib pool / np.random), or passed explicitly."""

    def __init__(self, num_labels=200, num_negative_samples=3, pos_thresh=0.0, neg_thresh=0.6, neg_weight=1.0,
                 ignore_label=-1, reduction="mean", uniform_sampling=True, distance_type="cos"):
        super().__init__()
        if distance_type not in ("cos", "l1", "l2"):
            raise ValueError("representation_distance_type must be 'cos', 'l1' or 'l2' (ContrastiveLanguageLoss.py:79-92), got %r" % (distance_type,))
        self.distance_type = distance_type            # config.representation_distance_type (config.py:159; default 'cos')
        self.num_labels, self.K = num_labels, num_negative_samples
        self.pos_thresh, self.neg_thresh, self.neg_weight = pos_thresh, neg_thresh, neg_weight
        self.ignore_label, self.reduction = ignore_label, reduction
        self.uniform_sampling = uniform_sampling      # config.clip_uniform_sampling (ContrastiveLanguageLoss.py:138-141)

    @classmethod
    def from_config(cls, config, num_labels, reduction="mean", feature_dim=512):
        """the reference's constructor arguments (ContrastiveLanguageLoss.py:22) -> ReferenceContrastiveLanguageLoss"""
        return ReferenceContrastiveLanguageLoss(config, num_labels, reduction=reduction, feature_dim=feature_dim)

    def sample_negatives(self, labels, generator=None):
        """K negative classes per voxel, on the device, no host sync.
        uniform_sampling=True : uniform over all other classes (clip_candidates minus own, :139)
        uniform_sampling=False: uniform over the OTHER classes present in this batch (unique_targets minus own, :141)"""
        n = labels.shape[0]
        lab = labels.clamp_min(0)
        if self.uniform_sampling:
            r = torch.randint(0, self.num_labels - 1, (n, self.K), device=labels.device, generator=generator)
            return r + (r >= lab[:, None]).long()
        L = self.num_labels
        valid = labels != self.ignore_label
        present = torch.zeros(L + 1, dtype=torch.bool, device=labels.device)
        present[torch.where(valid, lab, torch.full_like(lab, L))] = True
        present = present[:L]
        rank = torch.cumsum(present.long(), 0) - 1                          # rank of a present class among the present ones
        n_present = present.sum()                                           # device scalar: never read on the host
        cls_of_rank = torch.zeros(L + 1, dtype=torch.long, device=labels.device)
        cls_of_rank[torch.where(present, rank, torch.full_like(rank, L))] = torch.arange(L, device=labels.device)
        u = torch.rand((n, self.K), device=labels.device, generator=generator)
        r = torch.minimum((u * (n_present - 1).clamp_min(1)).long(), (n_present - 2).clamp_min(0))
        own = rank[lab][:, None]
        idx = torch.minimum(r + (r >= own).long(), (n_present - 1).clamp_min(0))   # a single-class batch has no negatives: own class
        return cls_of_rank[idx]

    def _raw_distances(self, features, anchors, labels, neg_indices, ignore_label):
        """representation_distance_type 'l1' / 'l2' (ContrastiveLanguageLoss.py:79-86) on the raw, un-normalised vectors, without
        the reference's [N, 1+K, C] gathers (9.8 GB at 1.2 M voxels x 512-d):
          l2: mean_j sqrt(|f - t_j|^2 + 1e-7) with |f - t|^2 = |f|^2 - 2 f.t + |t|^2 from ONE dense [N, C] x [C, A] product;
          l1: mean_j sum_c (f_c - t_jc) -- the reference sums SIGNED differences (no abs; reproduced as written) = sum(f) - sum(t_j).
        Not the measured path (config.py:159 defaults to 'cos', which owns the fused kernels): plain torch device ops."""
        f, t = features.float(), anchors.float()
        # a label outside [0, A) is an ignored row (what the fused cos kernel and the CE kernel do), never an index: a
        # non-negative ignore_label such as 255 with 200 anchors must not reach the gathers
        valid = (labels != ignore_label) & (labels >= 0) & (labels < t.shape[0])
        lab = torch.where(valid, labels, torch.zeros_like(labels))
        if self.distance_type == "l1":
            fs, ts = f.sum(1), t.sum(1)
            d_pos = fs - ts[lab]
            d_neg = (fs[:, None] - ts[neg_indices]).mean(1)
        else:
            d2 = ((f * f).sum(1)[:, None] - 2.0 * (f @ t.t()) + (t * t).sum(1)[None, :]).clamp_min(0)
            d_pos = torch.sqrt(d2.gather(1, lab[:, None]).squeeze(1) + 1e-7)
            d_neg = torch.sqrt(d2.gather(1, neg_indices) + 1e-7).mean(1)
        zero = torch.zeros((), dtype=d_pos.dtype, device=d_pos.device)
        return torch.where(valid, d_pos, zero), torch.where(valid, d_neg, zero)

    def forward(self, features, labels, anchor_feats, neg_indices=None, return_similarity=False, return_pred=False, ignore_label=None):
        """-> (loss, pos_loss, neg_loss[, sim][, pred]); pred = argmax_a <f^, t^_a>, what the reference's trainer gets from
        feature_sim(...).argmax(1) (pl_RepresentationTrainer.py:237-238) -- here a by-product of the same pass.
        ignore_label: overrides self.ignore_label for this call (the [N, 2]-label adapter passes a sentinel that cannot collide
        with a flattened (category, attribute) index)."""
        if features.dim() != 2:
            raise ValueError("`features` needs to be [n_points, feat_dim]")
        if anchor_feats.dim() == 3:                               # anchors with attributes: use the plain ones (:122-123)
            anchor_feats = anchor_feats[:, 0, :]
        labels = labels.long()
        ign = self.ignore_label if ignore_label is None else ignore_label
        if neg_indices is None:
            neg_indices = self.sample_negatives(labels)
        if self.distance_type != "cos":
            if return_similarity or return_pred:
                raise ValueError("similarity / arg-max outputs exist for the 'cos' distance only")
            d_pos, d_neg = self._raw_distances(features, anchor_feats, labels, neg_indices, ign)
            return self._hinge(d_pos, d_neg)
        be = get_backend()
        fused = (hasattr(be, "clip_loss_forward") and features.is_cuda
                 and (not anchor_feats.requires_grad or hasattr(be, "clip_loss_backward_anchors"))
                 and anchor_feats.shape[0] % 4 == 0 and 4 <= anchor_feats.shape[0] <= be.CLIP_LOSS_MAX_ANCHORS
                 and 1 <= neg_indices.shape[1] <= 7)
        if fused:
            d_pos, d_neg, pred, sim = _ClipLossFused.apply(features, anchor_feats, labels, neg_indices, ign, bool(return_similarity))
        else:
            # > 224 anchors, more than 7 negatives, or the CPU oracle backend of the tests: dense similarity matrix + index
            # gathers (learned anchor projections take the fused path too: lgs_clip_loss_backward_anchors)
            sim = clip_similarity(features, anchor_feats)         # [N, num_labels] -- the MFMA contraction
            valid = (labels != ign) & (labels >= 0) & (labels < sim.shape[1])
            lab = torch.where(valid, labels, torch.zeros_like(labels))
            d_pos = 1.0 - sim.gather(1, lab[:, None]).squeeze(1)
            d_neg = 1.0 - sim.gather(1, neg_indices).mean(1)
            zero = torch.zeros((), dtype=sim.dtype, device=sim.device)
            d_pos = torch.where(valid, d_pos, zero)
            d_neg = torch.where(valid, d_neg, zero)
            pred = sim.detach().argmax(1) if return_pred else None
        out = self._hinge(d_pos, d_neg)
        if return_similarity:
            out = out + (sim,)
        if return_pred:
            out = out + (pred,)
        return out


    def _hinge(self, d_pos, d_neg):
        """ContrastiveLanguageLoss.py:185-192"""
        pos_loss = torch.relu(d_pos - self.pos_thresh)
        neg_loss = torch.relu(self.neg_thresh - d_neg)
        if self.reduction == "mean":
            loss = pos_loss.mean() + neg_loss.mean() * self.neg_weight
        else:
            loss = pos_loss + neg_loss * self.neg_weight
        return (loss, pos_loss, neg_loss)


class ReferenceContrastiveLanguageLoss(ContrastiveLanguageLoss):
    """Drop-in for the reference class, same constructor and call signature:
        /root/reference/lib/losses/ContrastiveLanguageLoss.py:22   __init__(config, num_labels, temperature, base_temperature,
                                                                           reduction, feature_dim)
        /root/reference/lib/losses/ContrastiveLanguageLoss.py:97   forward(features, labels, anchor_feats, preds=None)
                                                                   -> (loss, pos_loss, neg_loss)
    as built by pl_RepresentationTrainer.py:45 (`ContrastiveLanguageLoss(self.config, num_labels=..., reduction=...)`) and
    called at :216 (`criterion(soutput.F, target, anchor_feats=anchor_feats)`).  The one-line swap is the import at
    pl_RepresentationTrainer.py:8.  It reads the same config fields (ignore_label,
    num_negative_samples with -1 = all labels, contrast_pos_thresh / contrast_neg_thresh / contrast_neg_weight,
    clip_uniform_sampling, representation_distance_type) and keeps the attributes the trainer touches
    (`augment_categories`, :46; `confusion_hist` buffer).  The arithmetic is the engine's fused kernel
    (lgs_clip_loss_forward / lgs_clip_loss_backward); negatives are drawn on the device instead of the reference's
    per-class np.random.choice inside a joblib thread pool (whose draw order is not reproducible even with a seed).
    Category + attribute labels ([N, 2], :149-178) select the anchor (category, attribute) as the positive and plain
    category anchors as negatives, like the reference.  With clip_uniform_sampling=False the reference draws negatives from
    `unique_targets_np[unique_targets_np != ut[0]]`, where unique_targets_np is an array of (category, attribute) PAIRS (:152-153,:173):
    the comparison broadcasts over both columns and the "candidates" are a mix of category and attribute ids -- a reference bug;
    this class draws from the other CATEGORIES present in the batch, which is what the 1-D branch (:141) does. its latent augmentation (a pretrained AttributeFittingModel that is
    not part of the hot path) is not reproduced and raises if configured."""

    def __init__(self, config, num_labels, temperature=0.07, base_temperature=0.07, reduction="mean", feature_dim=512):
        k = int(getattr(config, "num_negative_samples", 3))
        if k <= -1:
            k = num_labels                                            # :35-38
        dist_type = getattr(config, "representation_distance_type", "cos")
        super().__init__(num_labels=num_labels, num_negative_samples=k,
                         pos_thresh=float(getattr(config, "contrast_pos_thresh", 0.0)),
                         neg_thresh=float(getattr(config, "contrast_neg_thresh", 0.6)),
                         neg_weight=float(getattr(config, "contrast_neg_weight", 1.0)),
                         ignore_label=int(getattr(config, "ignore_label", -1)), reduction=reduction,
                         uniform_sampling=bool(getattr(config, "clip_uniform_sampling", True)), distance_type=dist_type)
        self.config = config
        self.temperature, self.base_temperature, self.feature_dim = temperature, base_temperature, feature_dim
        self.num_negative_samples = k
        self.register_buffer("confusion_hist", torch.zeros((num_labels, num_labels)).long())
        self.augment_categories = torch.empty(0)
        # latent attribute augmentation (:46-60): eight learned linear maps ("A red ", ..., "A small "), weights from
        # config.scannet_path / config.projection_model_path when that file exists (else the module's initial weights, as in
        # the reference), eval mode
        import os
        import numpy as np
        from .projection_models import AttributeFittingModel
        self.attributes = np.array(['A red ', 'A green ', 'A blue ', 'A yellow ', 'A dark ', 'A bright ', 'A big ', 'A small '])
        self.augment_probability = float(getattr(config, "instance_augmentation_color_aug_prob", 0.0))
        self.projection_model = AttributeFittingModel(feature_dim, feature_dim, self.attributes.shape[0])
        model_path = "%s/%s" % (getattr(config, "scannet_path", ""), getattr(config, "projection_model_path", ""))
        if os.path.isfile(model_path):
            self.projection_model.load_state_dict(torch.load(model_path))
        self.projection_model.eval()

    def plan_latent_augmentation(self, generator=None, device="cpu"):
        """The reference decides per unique (category, attribute) target of the batch, inside a thread pool, with the host RNGs
        (`random.random() < p`, then `np.random.randint(0, 8)`, :62-70).  Here ONE independent draw per possible (category,
        attribute-slot) pair, on the device, no host loop: -> (augment? [L * A] bool, new attribute [L * A] int64) for A slots."""
        A = self.attributes.shape[0] + 1                                   # slot 0 = the raw category, 1..8 = attributes
        # draw where the generator lives (a CPU generator cannot feed a device op), then move: 2 x 1800 numbers
        gdev = generator.device if generator is not None else device
        u = torch.rand(self.num_labels * A, generator=generator, device=gdev).to(device)
        k = torch.randint(0, self.attributes.shape[0], (self.num_labels * A,), generator=generator, device=gdev).to(device)
        return u < self.augment_probability, k

    def latent_augmentation(self, features, labels, plan=None, generator=None):
        """ContrastiveLanguageLoss.py:62-70,160-165 for the whole batch at once: rows whose category is in `augment_categories`
        and whose (category, attribute) target drew "augment" are replaced IN PLACE (like the reference's
        `features[ut_inds, :] = aug_feats`) by attribute a's projection of themselves; their attribute label becomes a and the
        positive anchor slot a + 1 (:68, `current_aug + 1`).  -> (features, labels, positive attribute slot [N])"""
        cat, att = labels[:, 0].long(), labels[:, 1].long()
        A = self.attributes.shape[0] + 1
        dev = features.device
        if plan is None:
            plan = self.plan_latent_augmentation(generator, dev)
        on, new_attr = plan[0].to(dev), plan[1].to(dev)
        cats = self.augment_categories.to(dev).long()
        in_aug = torch.zeros(self.num_labels + 1, dtype=torch.bool, device=dev)
        if cats.numel():
            in_aug[cats.clamp(0, self.num_labels)] = True
        valid = (cat != self.ignore_label) & (cat >= 0) & (cat < self.num_labels) & (att >= 0) & (att < A)
        pair = torch.where(valid, cat * A + att, torch.zeros_like(cat))
        in_aug_row = valid & in_aug[torch.where(valid, cat, torch.full_like(cat, self.num_labels))]
        do = in_aug_row & on[pair]
        k = new_attr[pair]
        idx = do.nonzero().squeeze(1)                                      # (one host sync; the reference loops over classes)
        if self.projection_model.attr_linears[0].weight.device != dev:
            self.projection_model = self.projection_model.to(dev)
        if idx.numel():
            proj = self.projection_model.project(features[idx].float(), k[idx])
            features.index_copy_(0, idx, proj.to(features.dtype))
        labels[:, 1] = torch.where(do, k, att).to(labels.dtype)
        # a target of an augment category whose draw said "no" keeps its features and labels, but the reference then sets ut[1] =
        # attribute_id = 0 (:70,:163-165): its positive anchor is slot 0, the raw category, whatever attribute it carried
        return features, labels, torch.where(do, k + 1, torch.where(in_aug_row, torch.zeros_like(att), att))

    def forward(self, features, labels, anchor_feats, preds=None, neg_indices=None, aug_plan=None):
        if labels.dim() == 2:                                        # (category, attribute) targets, :149-181
            if anchor_feats.dim() != 3:
                raise ValueError("[N, 2] labels need [num_labels, num_attributes, C] anchors")
            A = anchor_feats.shape[1]
            cat, att = labels[:, 0].long(), labels[:, 1].long()
            if getattr(self.config, "instance_augmentation", None) == "latent":
                features, labels, att = self.latent_augmentation(features, labels, plan=aug_plan)
            if neg_indices is None:
                neg_indices = self.sample_negatives(cat)
            valid = cat != self.ignore_label
            # ignored rows become -1, which no flattened (category, attribute) index can equal -- a non-negative
            # config.ignore_label (e.g. 255) would otherwise silently drop the valid pair whose flat index is 255
            flat_lab = torch.where(valid, cat.clamp_min(0) * A + att, torch.full_like(cat, -1))
            out = super().forward(features, flat_lab, anchor_feats.reshape(-1, anchor_feats.shape[-1]), neg_indices=neg_indices * A,
                                  ignore_label=-1)
            return out[:3]
        return super().forward(features, labels, anchor_feats, neg_indices=neg_indices)[:3]


def _supcon_gather(src, idx):
    """rows src[idx] with the all-zero row where idx is outside [0, N) (-1 = "no sample"): [N, S, C]"""
    n = src.shape[0]
    ok = (idx >= 0) & (idx < n)
    return src[idx.clamp(0, max(n - 1, 0))] * ok[..., None].to(src.dtype)


def supcon_distances_torch(features, labels, pos_idx, neg_idx, ignore_label, num_labels, distance_type):
    """The gather path of PointSupConLoss in plain torch, PointSupConLoss.py:44-71 line by line: gather the (detached) sampled
    rows into [N, S, C], F.normalize both sides and average the dot products ('cos'), or average sqrt(|a - b|^2 + 1e-7) ('l2');
    rows that are not counted get distance 0.  -> (d_pos [N], d_neg [N]); float32 arithmetic (float64 features stay float64).
    CPU tensors, a backend without the kernels, P or K outside 1 .. 8 and SUPCON_FUSED=0 take it; the GPU tests restate the
    kernels with it in float64."""
    f = features if features.dtype == torch.float64 else features.float()
    n = f.shape[0]
    if n == 0:
        z = f.sum(1)
        return z, z
    src = f.detach()
    valid = (labels != ignore_label) & (labels >= 0) & (labels < num_labels)
    out = []
    for idx in (pos_idx, neg_idx):
        b = _supcon_gather(src, idx)
        if distance_type == "l2":
            d = torch.sqrt((f[:, None, :] - b).pow(2).sum(-1) + 1e-7).mean(1)
        else:
            an = torch.nn.functional.normalize(f, p=2, dim=1)
            bn = torch.nn.functional.normalize(b, p=2, dim=2)
            d = 1 - (an[:, None, :] * bn).sum(-1).mean(1)
        out.append(torch.where(valid, d, torch.zeros_like(d)))
    return out[0], out[1]


class _SupConFused(torch.autograd.Function):
    """(d_pos, d_neg) of the supervised point-contrastive loss in one pass over the features and their P + K sampled rows
    (lgs_supcon_forward); backward = lgs_supcon_backward from the saved per-sample similarities and 1 / |row|.  The sampled rows are
    constants, as in the reference (`comp_feats = features.clone().detach()`)."""

    @staticmethod
    def forward(ctx, feats, labels, pos_idx, neg_idx, ignore_label, num_labels, distance):
        d_pos, d_neg, saved = get_backend().supcon_forward(feats.detach(), labels, pos_idx, neg_idx, ignore_label, num_labels, distance)
        ctx.args = (ignore_label, num_labels, distance)
        ctx.save_for_backward(*saved)
        ctx.set_materialize_grads(False)
        return d_pos, d_neg

    @staticmethod
    def backward(ctx, g_dpos, g_dneg):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        return (get_backend().supcon_backward(tuple(ctx.saved_tensors), g_dpos, g_dneg, *ctx.args),) + (None,) * 6


class PointSupConLoss(nn.Module):
    """The supervised point-contrastive criterion of lib/losses/PointSupConLoss.py, the baseline the language-grounded pre-training
    is compared against: per point P positives drawn from its own class and K negatives drawn from the other classes of the
    batch in proportion to the confusion matrix (hardest-negative mining),
        d = 1 - mean_j <f^, b^_j>  ('cos')   or   mean_j sqrt(|f - b_j|^2 + 1e-7)  ('l2');
        loss = relu(d_pos - pos_thresh) + neg_weight * relu(neg_thresh - d_neg)
    with the sampled rows b_j detached.  Kept as the reference is written: a row whose label is ignore_label (here also: outside
    [0, num_labels), the predicate of every loss of the engine) gets distance 0 -- pos_loss relu(-pos_thresh) and neg_loss
    relu(neg_thresh), so an ignored row adds 0.6 to neg_loss by default -- and counts in the mean.
    Sample indices: int64 [N, P] / [N, K]; -1 (anything outside [0, N)) is "no sample", the all-zero row the reference's
    zero-initialised sample buffers hold where nothing was drawn: cosine similarity 0, l2 distance sqrt(|f|^2 + 1e-7).
    `sample` draws them on the device without a host synchronisation (k_supcon_sample); HIP tensors in fp32 / bf16 with P, K in
    1 .. 8 run lgs_supcon_forward / lgs_supcon_backward, everything else supcon_distances_torch (tuning knob SUPCON_FUSED=0: that
    path and the torch sampler on HIP tensors too).
    `confusion_hist` starts as update_confusion_hist(0) = all ones (the reference starts at zeros, with which its np.random.choice
    raises until the first update)."""

    def __init__(self, num_labels, num_pos_samples=1, num_negative_samples=3, pos_thresh=0.0, neg_thresh=0.6, neg_weight=1.0,
                 ignore_label=-1, reduction='mean', distance_type='cos'):
        super().__init__()
        if distance_type not in ("cos", "l2"):
            raise ValueError("representation_distance_type must be 'cos' or 'l2' (PointSupConLoss.py:52-68), got %r" % (distance_type,))
        if int(num_pos_samples) < 1 or int(num_negative_samples) < 1:
            raise ValueError("num_pos_samples and num_negative_samples must be >= 1")
        self.num_labels = int(num_labels)
        self.num_pos_samples, self.num_negative_samples = int(num_pos_samples), int(num_negative_samples)
        self.pos_thresh, self.neg_thresh, self.neg_weight = pos_thresh, neg_thresh, neg_weight
        self.ignore_label, self.reduction, self.distance_type = ignore_label, reduction, distance_type
        self.register_buffer("confusion_hist", torch.ones((self.num_labels, self.num_labels), dtype=torch.int64))
        self._generator = None

    @classmethod
    def from_config(cls, config, num_labels, reduction="mean"):
        """the reference's constructor arguments (PointSupConLoss.py:17) -> ReferencePointSupConLoss"""
        return ReferencePointSupConLoss(config, num_labels, reduction=reduction)

    def update_confusion_hist(self, new_confusion_hist):
        """PointSupConLoss.py:41-42: hist + 1, so that no pair of classes has weight 0.  Takes SegmentationMeter.confmat as it is
        (int64, on the device)."""
        hist = torch.as_tensor(new_confusion_hist).detach().to(device=self.confusion_hist.device, dtype=torch.int64)
        if tuple(hist.shape) != (self.num_labels, self.num_labels):
            raise ValueError("confusion histogram must be [%d, %d], got %s" % (self.num_labels, self.num_labels, tuple(hist.shape)))
        self.confusion_hist = hist + 1

    def _seed_generator(self, generator):
        if generator is not None:
            if generator.device.type != "cpu":
                raise ValueError("PointSupConLoss.sample takes a CPU torch.Generator (its seed is drawn on the host)")
            return generator
        if self._generator is None:
            self._generator = torch.Generator().manual_seed(torch.initial_seed())
        return self._generator

    def sampling_tables(self, labels, preds=None):
        """The two-level form of the reference's draw, in device ops without a host synchronisation.  The reference draws a negative
        for class u among all points j with p_j ~ confusion_hist[u, label_j], zero where label_j == u, label_j is ignored or (with
        preds) label_j != preds_j (:124-139).  That is: class c with weight w[u, c] = hist[u, c] * m[c] * [c != u], m[c] = eligible
        points of c, then a uniform point among those m[c].
        -> (cum [L, L], order [N], seg_start [L], cls_count [L], elig_count [L]), all int64:
        one stable sort of 2 * label + (not eligible) (rows that are not counted: 2 L, last) gives `order`; binary searches for the
        2 L + 1 key boundaries give the segment starts and sizes; cum is the INT64 running sum of w along each row (exact: a class of
        weight 0 adds nothing and cannot be drawn)."""
        L = self.num_labels
        labels = labels.long()
        valid = (labels != self.ignore_label) & (labels >= 0) & (labels < L)
        elig = valid if preds is None else valid & (labels == preds.to(labels.device).long())
        key = torch.where(valid, 2 * labels + (~elig).long(), torch.full_like(labels, 2 * L))
        skey, order = torch.sort(key, stable=True)
        bounds = torch.searchsorted(skey, torch.arange(2 * L + 1, device=labels.device, dtype=skey.dtype))
        seg_start = bounds[0:2 * L:2]
        elig_count = bounds[1:2 * L:2] - seg_start
        cls_count = bounds[2:2 * L + 1:2] - seg_start
        hist = self.confusion_hist.to(labels.device).clamp_min(0)
        w = hist * elig_count[None, :]
        w = w - torch.diag_embed(w.diagonal())
        return torch.cumsum(w, 1), order, seg_start.contiguous(), cls_count.contiguous(), elig_count.contiguous()

    def sample(self, labels, preds=None, generator=None):
        """-> (pos_idx [N, P], neg_idx [N, K]) int64 on the labels' device, -1 = no sample: every slot of a row that is not counted,
        and the negative slots of a row whose class has no eligible negative in the batch (the reference raises inside
        np.random.choice there).  Positives are uniform, with replacement, over ALL points of the row's class -- the row itself and,
        with preds, the mispredicted points included (the reference's filter is commented out, :112-117).
        generator: a CPU torch.Generator (default: one the module owns, seeded from torch.initial_seed()).  HIP tensors: one 63-bit
        seed is drawn from it on the host and k_supcon_sample derives every index from (seed, row, slot).  CPU tensors (and
        SUPCON_FUSED=0): the same two-level draw with torch.rand from that generator -- the same distribution, other numbers."""
        if labels.dim() != 1:
            raise ValueError("labels must be [N]")
        labels = labels.long()
        n, L, P, K = labels.shape[0], self.num_labels, self.num_pos_samples, self.num_negative_samples
        gen = self._seed_generator(generator)
        be = get_backend()
        tables = self.sampling_tables(labels, preds)
        if (labels.is_cuda and hasattr(be, "supcon_sample") and be.supcon_enabled()
                and 1 <= P <= be.SUPCON_MAX_SAMPLES and 1 <= K <= be.SUPCON_MAX_SAMPLES):
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=gen).item())       # a CPU tensor: no device synchronisation
            return be.supcon_sample(labels, L, self.ignore_label, tables, P, K, seed)
        cum, order, seg_start, cls_count, elig_count = tables
        dev = labels.device
        if n == 0:
            return labels.new_empty((0, P)), labels.new_empty((0, K))
        u = torch.rand((3, n, max(P, K)), generator=gen, dtype=torch.float64).to(dev)
        valid = (labels != self.ignore_label) & (labels >= 0) & (labels < L)
        lab = torch.where(valid, labels, torch.zeros_like(labels))
        none = torch.full((), -1, dtype=torch.int64, device=dev)
        def below(r, t):                       # uniform integer in [0, t), t >= 1 (int64 tensors)
            return torch.minimum((r * t.double()).long(), t - 1).clamp_min(0)

        def pick(cls, count, r):               # a uniform member of the first `count` entries of a class's segment
            at = (seg_start[cls] + below(r, count.clamp_min(1))).clamp(0, n - 1)
            return order[at]
        pos = pick(lab[:, None].expand(n, P), cls_count[lab][:, None].expand(n, P), u[0, :, :P])
        pos = torch.where(valid[:, None], pos, none)
        row_cum = cum[lab]                                                              # [N, L]
        total = row_cum[:, -1:]
        x = below(u[1, :, :K], total.clamp_min(1).expand(n, K))
        cls = torch.searchsorted(row_cum, x, right=True).clamp_max(L - 1)               # the first class with cum > x
        neg = pick(cls, elig_count[cls], u[2, :, :K])
        neg = torch.where(valid[:, None] & (total > 0) & (elig_count[cls] > 0), neg, none)
        return pos, neg

    def forward(self, features, labels, anchor_feats=None, preds=None, pos_indices=None, neg_indices=None):
        """-> (loss, pos_loss [N], neg_loss [N]); the reference's call signature (anchor_feats is accepted and unused there too).
        preds: the model's predictions; negatives are then drawn among the correctly predicted points only (:133-135).
        pos_indices / neg_indices: explicit samples instead of a draw."""
        if features.dim() != 2:
            raise ValueError("`features` needs to be [n_points, feat_dim]")
        labels = labels.long()
        if pos_indices is None or neg_indices is None:
            drawn = self.sample(labels, preds)
            pos_indices = drawn[0] if pos_indices is None else pos_indices
            neg_indices = drawn[1] if neg_indices is None else neg_indices
        pos_indices, neg_indices = pos_indices.to(features.device).long(), neg_indices.to(features.device).long()
        be = get_backend()
        fused = (features.is_cuda and hasattr(be, "supcon_forward") and features.dtype in (torch.float32, torch.bfloat16)
                 and 1 <= pos_indices.shape[1] <= be.SUPCON_MAX_SAMPLES and 1 <= neg_indices.shape[1] <= be.SUPCON_MAX_SAMPLES
                 and features.shape[0] > 0 and be.supcon_enabled())
        if fused:
            d_pos, d_neg = _SupConFused.apply(features, labels, pos_indices, neg_indices, self.ignore_label, self.num_labels,
                                              self.distance_type)
        else:
            d_pos, d_neg = supcon_distances_torch(features, labels, pos_indices, neg_indices, self.ignore_label, self.num_labels,
                                                  self.distance_type)
        return self._hinge(d_pos, d_neg)

    def _hinge(self, d_pos, d_neg):
        """PointSupConLoss.py:144-154"""
        pos_loss = torch.relu(d_pos - self.pos_thresh)
        neg_loss = torch.relu(self.neg_thresh - d_neg)
        if self.reduction == "mean":
            loss = pos_loss.mean() + neg_loss.mean() * self.neg_weight
        else:
            loss = pos_loss + neg_loss * self.neg_weight
        return (loss, pos_loss, neg_loss)


class ReferencePointSupConLoss(PointSupConLoss):
    """Drop-in for the reference class, same constructor and call signature:
        lib/losses/PointSupConLoss.py:17   __init__(config, num_labels, temperature, base_temperature, reduction)
        lib/losses/PointSupConLoss.py:74   forward(features, labels, anchor_feats=None, preds=None) -> (loss, pos_loss, neg_loss)
    as built by BaselineTrainerModule.init_criterions (lib/train_test/pl_BaselineTrainer.py:92-108) for every embedding_loss_type
    other than MSE and 'contrast'.  It reads the same config fields (ignore_label, num_pos_samples, num_negative_samples,
    contrast_pos_thresh / contrast_neg_thresh / contrast_neg_weight, representation_distance_type) and keeps `confusion_hist` and
    update_confusion_hist (:165 feeds it `iou_scores.confmat.long()`, which metrics.SegmentationMeter keeps on the device).
    temperature / base_temperature are stored and unused, as in the reference."""

    def __init__(self, config, num_labels, temperature=0.07, base_temperature=0.07, reduction="mean"):
        super().__init__(num_labels=num_labels, num_pos_samples=int(config.num_pos_samples),
                         num_negative_samples=int(config.num_negative_samples),
                         pos_thresh=float(config.contrast_pos_thresh), neg_thresh=float(config.contrast_neg_thresh),
                         neg_weight=float(config.contrast_neg_weight), ignore_label=int(config.ignore_label), reduction=reduction,
                         distance_type=config.representation_distance_type)
        self.config = config
        self.temperature, self.base_temperature = temperature, base_temperature
        self.eps = 10e-5

    def forward(self, features, labels, anchor_feats=None, preds=None):
        return super().forward(features, labels, anchor_feats=anchor_feats, preds=preds)


class _ClipCE(torch.autograd.Function):
    """cross-entropy over the cosine similarities to ALL anchors, one autograd node: forward = lgs_clip_similarity (the MFMA
    contraction normalize(F) . normalize(T)^T, [N, A] fp32) + lgs_ce_forward_backward (loss only); backward = the CE kernel again
    (d S, already scaled by the upstream gradient) pushed through dS/df = (t^ - s f^) / |f| (and dS/dT for learned anchors)."""

    @staticmethod
    def forward(ctx, feats, anchors, labels, ignore_index):
        be = get_backend()
        sim, inv = be.clip_similarity(feats, anchors)
        loss, _, inv_valid = be.cross_entropy(sim, labels, ignore_index, want_grad=False)
        ctx.save_for_backward(feats, anchors, sim, inv, labels, inv_valid)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, g):
        feats, anchors, sim, inv, labels, inv_valid = ctx.saved_tensors
        _, gs, _ = get_backend().cross_entropy(sim, labels, ctx.ignore_index, grad_scale=g, inv_valid=inv_valid)
        tn = torch.nn.functional.normalize(anchors.float(), dim=1)
        fh = feats.float() * inv[:, None]
        gf = ((gs @ tn - (gs * sim).sum(1, keepdim=True) * fh) * inv[:, None]).to(feats.dtype) if ctx.needs_input_grad[0] else None
        ga = None
        if ctx.needs_input_grad[1]:
            an = anchors.float().norm(dim=1, keepdim=True).clamp_min(1e-12)
            gt = gs.t() @ fh
            ga = ((gt - (gt * tn).sum(1, keepdim=True) * tn) / an).to(anchors.dtype)
        return gf, ga, None, None


def _ce_like_the_engine(scores, labels, ignore_index, reduction):
    """torch cross-entropy with the conventions of the engine's fused kernel, so that the result does not depend on which path
    the gate selects (advisor, round 5): a label outside [0, A) is an ignored row (nn.CrossEntropyLoss raises on it), and the mean
    over a batch with no counted row is 0 (nn.CrossEntropyLoss returns NaN)."""
    a = scores.shape[1]
    lab = torch.where((labels >= 0) & (labels < a) & (labels != ignore_index), labels, torch.full_like(labels, -100))
    if reduction != "mean":
        return torch.nn.functional.cross_entropy(scores, lab, ignore_index=-100, reduction=reduction)
    total = torch.nn.functional.cross_entropy(scores, lab, ignore_index=-100, reduction="sum")
    return total / (lab != -100).sum().clamp_min(1).to(total.dtype)


class ReferenceContrastiveLanguageCELoss(ReferenceContrastiveLanguageLoss):
    """Drop-in for /root/reference/lib/losses/ContrastiveLanguageLoss.py:196-237 (`embedding_loss_type=contrast_ce`,
    lib/train_test/pl_RepresentationTrainer.py:42-43): nn.CrossEntropyLoss(ignore_index, reduction) over the per-voxel
    "distances" to ALL num_labels anchors -- for 'cos' literally normalize(F) . normalize(T)^T in [N, num_labels] (no temperature:
    the reference never applies it), the one dense contraction of the hot path; for 'l2' sqrt(|f - t^|^2 + 1e-7) against the
    NORMALISED anchors (as written, :208-211,:230).  forward(features, labels, anchor_feats, preds=None) -> (loss, zeros(1), loss).
    Two deliberate conventions, the same on every path (fused kernel, dense fallback, l2): a label outside [0, num_labels) is an
    ignored row (the reference's nn.CrossEntropyLoss raises), and a batch without a counted row gives 0 (the reference: NaN)."""

    def __init__(self, config, num_labels, temperature=0.07, base_temperature=0.07, reduction="mean"):
        super().__init__(config, num_labels, temperature, base_temperature, reduction)

    def forward(self, features, labels, anchor_feats, preds=None):
        if features.dim() != 2:
            raise ValueError("`features` needs to be [n_points, feat_dim]")
        labels = labels.long()
        be = get_backend()
        if self.distance_type == "cos":
            if (self.reduction == "mean" and hasattr(be, "cross_entropy") and features.is_cuda
                    and anchor_feats.shape[0] <= 512 and features.dtype in (torch.float32, torch.bfloat16)):
                loss = _ClipCE.apply(features, anchor_feats, labels, self.ignore_label)
            else:
                out = clip_similarity(features, anchor_feats)
                loss = _ce_like_the_engine(out, labels, self.ignore_label, self.reduction)
        elif self.distance_type == "l2":
            f = features.float()
            t = torch.nn.functional.normalize(anchor_feats.float(), p=2, dim=1)
            d2 = ((f * f).sum(1)[:, None] - 2.0 * (f @ t.t()) + (t * t).sum(1)[None, :]).clamp_min(0)
            loss = _ce_like_the_engine(torch.sqrt(d2 + 1e-7), labels, self.ignore_label, self.reduction)
        else:
            raise ValueError("ContrastiveLanguageCELoss supports representation_distance_type 'cos' and 'l2' (:206-220)")
        return loss, torch.zeros(1), loss


def sample_categories_for_balancing(loss, targets, frequency_organized_cats, head_ratio, common_ratio, ignore_label=-1,
                                    generator=None, split="tensors"):
    """lib/losses/utils.py:13-77 on the device, no host loop / np.random.choice: per-point `loss` [N] is masked so
    that every HEAD class keeps round(head_ratio * count) of its points, every COMMON class round(common_ratio * count)
    (drawn without replacement), TAIL classes keep all; ratio <= 0 keeps everything (:41,:54).
    frequency_organized_cats: bool [num_labels, 3] (head, common, tail), lib/datasets/scannet.py:131-141.
    split="tensors" (the reference's return shape):
        -> (masked loss mean over ALL points, (head, common, tail per-point losses, detached), loss_items [N_valid, 3]);
        the three variable-length tensors and the row-filtered mask are boolean-index results, i.e. THREE + ONE device->host
        syncs for their sizes, exactly what the reference's own `loss[loss_items[:, 0]]` costs.
    split="stats" (the training step: no host sync at all):
        -> (masked loss mean, stats [3, 2] = (sum of the per-point losses, number of points) of head / common / tail -- what the
        trainer feeds its meters, `nanmean_t(split_losses[i])` = stats[i, 0] / stats[i, 1] and `.size(0)` = stats[i, 1]
        (pl_BaselineTrainer.py:353-355) --, loss_items [N, 3] over ALL rows, False on ignored ones)."""
    if split not in ("tensors", "stats"):
        raise ValueError("split must be 'tensors' or 'stats'")
    dev = loss.device
    foc = frequency_organized_cats.to(dev).bool()
    valid = targets != ignore_label
    lab = targets.clamp_min(0).long()
    L = foc.shape[0]
    group = torch.where(foc[:, 0], 0, torch.where(foc[:, 1], 1, 2)).to(dev)     # anything not head/common is kept like tail (:58-62)
    # per-class keep ratio, built from host scalars with fills only (a torch.tensor([...]) would be a blocking host->device copy)
    ratio = torch.ones(L, dtype=torch.float64, device=dev)
    ratio.masked_fill_(group == 0, head_ratio if head_ratio > 0 else 1.0).masked_fill_(group == 1, common_ratio if common_ratio > 0 else 1.0)
    if head_ratio <= 0 and common_ratio <= 0:
        # the configured default (config.py:281-282: both ratios -1; scripts/train_models.sh sets neither): every class keeps all
        # of its points (:45,:56,:60), nothing is drawn
        point_mask = valid
    else:
        # rank of every point inside its class by a random key = a uniform draw without replacement.  Class sizes and first
        # positions come from the sorted keys (binary searches for the 200 class boundaries), not from 1.2 M atomics on 200 counters
        u = torch.rand(loss.shape[0], device=dev, generator=generator)
        key = lab.double() + u.double()
        key = torch.where(valid, key, torch.full_like(key, float(L + 1)))
        skey, order = torch.sort(key)
        bounds = torch.searchsorted(skey, torch.arange(L + 1, device=dev, dtype=torch.float64))
        start, counts = bounds[:L], bounds[1:] - bounds[:L]                       # first sorted position / size of every class
        keep_n = torch.round(ratio * counts.double()).long()                     # python round == torch.round: half to even
        pos = torch.empty_like(order)
        pos[order] = torch.arange(order.shape[0], device=dev)
        rank_in_class = pos - start[lab]
        point_mask = valid & (rank_in_class < keep_n[lab])
    masked = loss * point_mask.to(loss.dtype)
    be = get_backend()
    if split == "stats" and loss.is_cuda and hasattr(be, "split_stats"):
        # one streaming pass for the three meters (lgs_split_stats); the [N, 3] membership mask is built only if somebody reads it
        stats = be.split_stats(loss, targets, group, ignore_label)
        return masked.mean(), stats, _LazyItems(valid, group, lab)
    pg = group[lab]
    loss_items = torch.stack([valid & (pg == 0), valid & (pg == 1), valid & (pg == 2)], 1)
    if split == "stats":
        ld = loss.detach().float()
        stats = torch.stack([torch.stack([(ld * loss_items[:, i]).sum() for i in range(3)]), loss_items.sum(0).float()], 1)   # [3, 2]
        return masked.mean(), stats, loss_items
    head, common, tail = (loss[loss_items[:, i]].detach() for i in range(3))
    return masked.mean(), (head, common, tail), loss_items[valid]


class _LazyItems:
    """loss_items [N, 3] of split='stats' on the device path, built when it is indexed / converted (the training step never does:
    its meters take the statistics; the reference's evaluation code indexes predictions with it, pl_BaselineTrainer.py:358-370)"""

    def __init__(self, valid, group, lab):
        self._parts, self._t = (valid, group, lab), None

    def tensor(self):
        if self._t is None:
            valid, group, lab = self._parts
            pg = group[lab]
            self._t = torch.stack([valid & (pg == 0), valid & (pg == 1), valid & (pg == 2)], 1)
            self._parts = None
        return self._t

    def __getitem__(self, idx):
        return self.tensor()[idx]

    def __getattr__(self, name):
        return getattr(self.tensor(), name)


def instance_offset_losses(pt_offsets, coords_xyz, centers, instance_ids, voxel_size):
    """downstream/insseg/lib/pl_Trainer.py:271-299 (PointGroup offset losses): L1 norm loss and direction loss of the
    predicted per-voxel offset to its instance centre, averaged over voxels with an instance (id != -1).
    pt_offsets [N,3] (any float dtype), coords_xyz [N,3] voxel coordinates, centers [N,3] in voxel units.
    -> (offset_norm_loss, offset_dir_loss)"""
    po = pt_offsets.float()
    gt = (centers.float() - coords_xyz.float()) * voxel_size
    valid = (instance_ids != -1).float()
    denom = valid.sum() + 1e-6
    norm_loss = ((po - gt).abs().sum(-1) * valid).sum() / denom
    gt_n = gt / (gt.norm(p=2, dim=1, keepdim=True) + 1e-8)
    po_n = po / (po.norm(p=2, dim=1, keepdim=True) + 1e-8)
    dir_loss = (-(gt_n * po_n).sum(-1) * valid).sum() / denom
    return norm_loss, dir_loss


class _OffsetLossFused(torch.autograd.Function):
    """(norm_loss, dir_loss) of the offset head from one streaming kernel per direction (lgs_offset_loss_forward / _backward): the
    centre of a row is read from the instance table through its slot, nothing [N, 3] is allocated but the gradient, and the backward
    takes the upstream gradients and the valid count from device memory."""

    @staticmethod
    def forward(ctx, pt_offsets, coords, slot, center_table, voxel_size):
        po = pt_offsets.detach().contiguous()
        norm_loss, dir_loss, valid = instances.offset_loss_forward(po, coords, slot, center_table, voxel_size)
        ctx.save_for_backward(po, coords, slot, center_table, valid)
        ctx.voxel_size = voxel_size
        return norm_loss, dir_loss

    @staticmethod
    def backward(ctx, g_norm, g_dir):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        po, coords, slot, center_table, valid = ctx.saved_tensors
        g_norm, g_dir = (g.detach().to(torch.float32).reshape(()).contiguous() for g in (g_norm, g_dir))
        return instances.offset_loss_backward(po, coords, slot, center_table, ctx.voxel_size, valid, g_norm, g_dir), None, None, None, None


def fused_instance_offset_losses(pt_offsets, coords, info, voxel_size):
    """The offset losses of downstream/insseg/lib/pl_Trainer.py:286-298 from the instance table of the batch, without the [N, 3]
    `centers` upload of :280-284: pt_offsets [N, 3] (fp32 or bf16), coords int32 [N, 4] (batch index in column 0), info = what
    instances.instance_info(coords, instance_ids, ...) returned.  -> (offset_norm_loss, offset_dir_loss), differentiable in pt_offsets.
    HIP tensors: one kernel per direction, no host synchronisation, sums in fp64 in a fixed order (two calls give the same bits).
    Tuning knob LGS_INST_TARGETS_FUSED=0: the torch lines of instance_offset_losses on info.center instead.  CPU tensors always take
    those lines; there `info` is the [N] tensor of instance ids after masking (-1: none) and the centres are computed with torch
    (instances.centers_torch)."""
    if pt_offsets.dim() != 2 or pt_offsets.shape[1] != 3 or coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] != pt_offsets.shape[0]:
        raise ValueError("pt_offsets must be [N, 3] and coords [N, 4], got %s and %s" % (tuple(pt_offsets.shape), tuple(coords.shape)))
    is_info = isinstance(info, instances.InstanceInfo)
    rows = (info.ids if is_info else info).shape[0]
    if rows != pt_offsets.shape[0]:
        raise ValueError("instance targets of %d rows for %d offsets" % (rows, pt_offsets.shape[0]))
    if (pt_offsets.is_cuda and is_info and pt_offsets.dtype in (torch.float32, torch.bfloat16) and coords.dtype == torch.int32
            and tuning.host("INST_TARGETS_FUSED")):
        return _OffsetLossFused.apply(pt_offsets, coords.contiguous(), info.slot, info.center_table, float(voxel_size))
    ids = info.ids if is_info else info
    centers = info.center if is_info and info.center is not None else instances.centers_torch(coords, ids)
    return instance_offset_losses(pt_offsets, coords[:, 1:], centers, ids, voxel_size)


def feature_sim_argmax(sim):
    """lib/losses/utils.py:80-103 (cosine branch) + argmax for the metrics: reuse the similarity matrix."""
    return sim.argmax(1)
