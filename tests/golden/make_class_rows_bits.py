"""Generates tests/golden/class_rows_bits.json: SHA-256 digests of the raw bytes of everything the class-row kernels (k_ce_fwd_bwd,
k_focal_fwd_bwd, k_seg_metrics) write, recorded on an MI355X from the commit BEFORE csrc/lgs_classrows.h unified their accesses and
host dispatch.
tests/test_gpu_class_rows_bits.py imports this file for the inputs and the runs, and compares what the tree under test gives.

    python tests/golden/make_class_rows_bits.py          (on the GPU, with the engine of the commit to record built)

Inputs: torch.Generator seeds on the CPU, logits of scale 3 rounded to bf16 (so fp32 and bf16 hold the same values).  The n > 1 cases
put on rows 0..6: label -1 (ignore_index), -5, c + 2, class 0, class c - 1, a row whose label leads by a margin of 100 (u == 0) and
a row of all-equal values; the single row of an n = 1 case has label c - 1.
Shapes: Q = 1, 2, 4 chunks per lane, each with and without c % W == 0, and the 32- / 33-chunk boundaries; n = 1 and n = 8 R + 3 (one
full workgroup and a partial row group).
Per case: the cross-entropy rows, their gradient under a random upstream row gradient, the mean and its gradient under 0.37; for
gamma 0, 2, 0.5 with and without alpha the focal rows, both gradients and the reduced loss, and for gamma 0 with alpha the
weighted mean; pred (with and without prob), prob and the confusion matrix of one SegmentationMeter update."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "class_rows_bits.json")
DEV = "cuda:0"
SHAPES = [(torch.float32, c) for c in (13, 128, 130, 200, 509, 512)] + [(torch.bfloat16, c) for c in (13, 20, 200, 256, 264, 1021, 1024)]
GAMMAS = (0.0, 2.0, 0.5)


def rows_per_half_wave(c, dtype):
    w = 4 if dtype == torch.float32 else 8
    q = ((c + w - 1) // w + 31) // 32
    return 4 if q <= 1 else (2 if q == 2 else 1)


def row_counts(c, dtype):
    return (1, 8 * rows_per_half_wave(c, dtype) + 3)


def case_name(dtype, c, n):
    return "%s-c%d-n%d" % ("fp32" if dtype == torch.float32 else "bf16", c, n)


def make_inputs(dtype, c, n):
    """-> logits [n, c] dtype, labels [n] int64, upstream row gradient [n] fp32, alpha [c] fp32; all on the CPU"""
    g = torch.Generator().manual_seed(1000 * c + 10 * n + (1 if dtype == torch.bfloat16 else 0))
    x = (torch.randn(n, c, generator=g) * 3.0).bfloat16().float()
    lab = torch.randint(0, c, (n,), generator=g)
    row_grad = torch.randn(n, generator=g)
    alpha = torch.rand(c, generator=g) + 0.5
    if n == 1:
        lab[0] = c - 1
    else:
        lab[0], lab[1], lab[2], lab[3], lab[4] = -1, -5, c + 2, 0, c - 1
        j = int(lab[5])
        x[5] = x[5].round().clamp(-4.0, 4.0)
        x[5, j] = 104.0
        x[6] = 1.5
    return x.to(dtype), lab, row_grad, alpha


def digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def run_case(dtype, c, n):
    """-> {output name: digest} of one (dtype, c, n) through the public entry points"""
    from languagegroundedsemseg_amd.losses import fused_cross_entropy, fused_focal_loss
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    x, lab, row_grad, alpha = (t.to(DEV) for t in make_inputs(dtype, c, n))
    up = torch.tensor(0.37, device=DEV)
    out = {}

    def both(prefix, loss_fn):
        z = x.clone().requires_grad_(True)
        rows = loss_fn(z, "none")
        rows.backward(row_grad)
        out[prefix + "rows"], out[prefix + "rows_grad"] = digest(rows), digest(z.grad)
        z = x.clone().requires_grad_(True)
        mean = loss_fn(z, "mean")
        mean.backward(up)
        out[prefix + "mean"], out[prefix + "mean_grad"] = digest(mean), digest(z.grad)

    both("ce_", lambda z, red: fused_cross_entropy(z, lab, ignore_index=-1, reduction=red))
    for gamma in GAMMAS:
        for a in (None, alpha):
            both("focal_g%g_%s_" % (gamma, "alpha" if a is not None else "plain"),
                 lambda z, red: fused_focal_loss(z, lab, alpha=a, gamma=gamma, ignore_index=-1, reduction=red))
    out["wce_mean"] = digest(fused_cross_entropy(x, lab, ignore_index=-1, reduction="mean", weight=alpha))
    meter = SegmentationMeter(c, ignore_label=-1).to(DEV)
    pred, prob = meter.update(x, lab, want_prob=True)
    out["met_pred"], out["met_prob"], out["met_confmat"] = digest(pred), digest(prob), digest(meter.confmat)
    out["met_pred_noprob"] = digest(SegmentationMeter(c, ignore_label=-1).to(DEV).update(x, lab))
    torch.cuda.synchronize()
    return out


def environment():
    return {"hip": torch.version.hip, "arch": torch.cuda.get_device_properties(0).gcnArchName}


def main():
    sys.path.insert(0, ROOT)
    cases = {}
    for dtype, c in SHAPES:
        for n in row_counts(c, dtype):
            cases[case_name(dtype, c, n)] = run_case(dtype, c, n)
    doc = dict(environment(), cases=cases)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases, %d digests" % (len(cases), sum(len(v) for v in cases.values())))


if __name__ == "__main__":
    main()
