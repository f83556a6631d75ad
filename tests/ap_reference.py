"""Per-class average precision in numpy fp64, the expected values of every average-precision test:
    AP_c = (1 / P_c) sum over the positives i of c of TP_c(s_i) / Rank_c(s_i),   s_i = prob[i, c]
    TP_c(s) = #{positives j of c: prob[j, c] >= s},   Rank_c(s) = #{all rows j: prob[j, c] >= s}
which is sklearn's step-wise sum over distinct thresholds (test_average_precision_cpu.py holds it to sklearn)."""
import numpy as np


def ap_reference(prob, target, ignore_label=-1):
    """prob [N, C] (read as float64), target [N] -> float64 [C]; NaN for a class without a positive.  Rows whose target is
    ignore_label or outside [0, C) are negatives of every class."""
    prob = np.asarray(prob, dtype=np.float64)
    target = np.asarray(target, dtype=np.int64)
    n, c = prob.shape
    out = np.full(c, np.nan)
    for k in range(c):
        pos = (target == k) & (target != ignore_label)
        p = int(pos.sum())
        if p == 0:
            continue
        s = prob[pos, k]
        rank = n - np.searchsorted(np.sort(prob[:, k]), s, side="left")
        tp = p - np.searchsorted(np.sort(s), s, side="left")
        out[k] = (tp / rank).sum() / p
    return out
