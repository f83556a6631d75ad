"""Generates tests/golden/focal_loss.npz by RUNNING THE REFERENCE'S OWN FocalLoss (lib/losses/FocalLoss.py, loaded by file path; it
needs only torch) and nn.CrossEntropyLoss(weight=...) in float64.  The fixture is data only: inputs and expected outputs.

    python tests/golden/make_focal_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

Per class count C in {200, 13} (key prefix "c200_" / "c13_"):
    logits [67, C] float32 (scale 3), labels [67] int64 in [-1, C) (-1 = ignored), alpha [C] float32 in [0.1, 2.1]
    g0_* / g2_*   FocalLoss(alpha, gamma = 0 / 2, ignore_index=-1):
                  rows  float64 [n_valid]  reduction='none' -- the reference returns the COMPACTED non-ignored rows
                  mean  float64 []         reduction='mean' (the mean over those rows)
                  grad  float32 [67, C]    autograd gradient of the 'mean' value (the gradient of 'sum' is n_valid times it)
    wce_mean / wce_grad   nn.CrossEntropyLoss(weight=alpha, ignore_index=-1) 'mean' and its gradient
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference_focal(ref_root):
    path = os.path.join(ref_root, "lib", "losses", "FocalLoss.py")
    spec = importlib.util.spec_from_file_location("reference_focal_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FocalLoss


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LGS_REFERENCE")
    if not ref_root:
        raise SystemExit(__doc__)
    FocalLoss = load_reference_focal(ref_root)
    out = {}
    for c in (200, 13):
        g = torch.Generator().manual_seed(1000 + c)
        logits = (torch.randn(67, c, generator=g) * 3).float()
        labels = torch.randint(-1, c, (67,), generator=g)
        labels[:3] = torch.tensor([-1, 0, c - 1])
        alpha = (0.1 + 2.0 * torch.rand(c, generator=g)).float()
        pre = "c%d_" % c
        out[pre + "logits"], out[pre + "labels"], out[pre + "alpha"] = logits.numpy(), labels.numpy(), alpha.numpy()
        for gamma in (0, 2):
            x = logits.double().requires_grad_(True)
            rows = FocalLoss(alpha=alpha.double(), gamma=float(gamma), reduction="none", ignore_index=-1)(x, labels)
            mean = FocalLoss(alpha=alpha.double(), gamma=float(gamma), reduction="mean", ignore_index=-1)(x, labels)
            mean.backward()
            assert rows.shape[0] == int((labels != -1).sum()) and abs(float((rows.mean() - mean).detach())) < 1e-14
            out[pre + "g%d_rows" % gamma] = rows.detach().numpy()
            out[pre + "g%d_mean" % gamma] = mean.detach().numpy()
            out[pre + "g%d_grad" % gamma] = x.grad.numpy().astype(np.float32)
        x = logits.double().requires_grad_(True)
        wce = torch.nn.CrossEntropyLoss(weight=alpha.double(), ignore_index=-1)(x, labels)
        wce.backward()
        out[pre + "wce_mean"] = wce.detach().numpy()
        out[pre + "wce_grad"] = x.grad.numpy().astype(np.float32)
    path = os.path.join(HERE, "focal_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
