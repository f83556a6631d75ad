"""Furthest point sampling in numpy, for the tests of csrc/lgs_fps.hip and languagegroundedsemseg_amd/annotation.py.

  fps_contract      the contract of include/lgs_engine.h, restated: fp32, the written operation order, ties to the smallest index
  fps_as_written    the reference's kernel as it is written (lib/ext/pointnet2/_ext_src/src/sampling_gpu.cu:75-178): strided lanes
                    that keep their first maximum, then a halving tree in which the upper entry wins only when it is larger; the
                    block size is a parameter (the reference takes opt_n_threads(n))
  tie_free          whether every round of fps_contract has exactly one point at its maximum
  count_rule        max(min_points, round(ratio * n)) as the recipe writes it (lib/datasets/preprocessing/scannet_long.py:104)
  segments_contract / limited_annotation_contract: the CSR form and the label rule on top of fps_contract

numpy rounds every fp32 operation on its own and never contracts a multiply with an add, which is what the contract asks for."""
import math

import numpy as np

FAR = np.float32(1e10)


def eligible(p, skip_origin=True):
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    if not skip_origin:
        return np.ones(p.shape[0], dtype=bool)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return ((x * x + y * y) + z * z) > np.float32(1e-3)


def _dist(p, o):
    dx, dy, dz = p[:, 0] - p[o, 0], p[:, 1] - p[o, 1], p[:, 2] - p[o, 2]
    return (dx * dx + dy * dy) + dz * dz


def fps_contract(p, m, skip_origin=True, return_ties=False):
    """-> out int32 [m] (and, with return_ties, whether some round had more than one point at its maximum)"""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    m = int(m) if n else 0
    out = np.zeros(m, dtype=np.int32)
    ties = False
    if m > 1:
        ok = eligible(p, skip_origin)
        t = np.full(n, FAR, dtype=np.float32)
        with np.errstate(all="ignore"):
            for j in range(1, m):
                t = np.minimum(_dist(p, int(out[j - 1])), t)
                te = np.where(ok, t, np.float32(-1))
                k = int(np.argmax(te))            # the first maximum: the smallest index
                if te[k] < 0:
                    k = 0                         # no eligible point
                elif return_ties and np.count_nonzero(te == te[k]) > 1:
                    ties = True
                out[j] = k
    return (out, ties) if return_ties else out


def tie_free(p, m, skip_origin=True):
    return not fps_contract(p, m, skip_origin, return_ties=True)[1]


def opt_n_threads(n):
    """the reference's block size for n points (include/cuda_utils.h:20-24, TOTAL_THREADS 512)"""
    return max(min(1 << int(math.log(float(n)) / math.log(2.0)), 512), 1)


def fps_as_written(p, m, block=512):
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    m = int(m) if n else 0
    out = np.zeros(m, dtype=np.int32)
    if m <= 1:
        return out
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    mag = (x * x) + (y * y) + (z * z)
    skipped = mag.astype(np.float64) <= 1e-3              # a float against a double constant, as written
    rows = -(-n // block)
    lane = np.arange(block)
    t = np.full(n, FAR, dtype=np.float32)
    for j in range(1, m):
        o = int(out[j - 1])
        d2 = np.minimum(_dist(p, o), t)
        t = np.where(skipped, t, d2)
        v = np.full(rows * block, -2, dtype=np.float32)   # below the lanes' start of -1: never taken
        v[:n] = np.where(skipped, np.float32(-2), d2)
        v = v.reshape(rows, block)                        # lane `tid` walks k = tid, tid + block, ...
        first = np.argmax(v, axis=0)                      # d2 > best, strictly: a lane keeps its first maximum
        best = v[first, lane]
        taken = best > -1
        dists = np.where(taken, best, np.float32(-1))
        dists_i = np.where(taken, first * block + lane, 0)
        half = block // 2
        while half >= 1:
            v1, v2 = dists[:half].copy(), dists[half:2 * half]
            i1, i2 = dists_i[:half].copy(), dists_i[half:2 * half]
            dists[:half] = np.maximum(v1, v2)
            dists_i[:half] = np.where(v2 > v1, i2, i1)
            half //= 2
        out[j] = dists_i[0]
    return out


def count_rule(n, ratio, min_points=5):
    return max(min_points, round(ratio * n)) if n else 0


def clamp_offsets(seg_offsets, n):
    off = np.maximum.accumulate(np.maximum(np.asarray(seg_offsets, dtype=np.int64), 0))
    return np.minimum(off, n)


def segments_contract(points, seg_offsets, counts, through=None, skip_origin=True):
    """-> ([out of every segment], rank int32 [N])"""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = points.shape[0]
    off = clamp_offsets(seg_offsets, n)
    rank = np.full(n, -1, dtype=np.int32)
    outs = []
    for q in range(len(off) - 1):
        rows = np.arange(off[q], off[q + 1])
        if through is not None:
            rows = np.asarray(through)[rows]
        out = fps_contract(points[rows], counts[q], skip_origin)
        outs.append(out)
        for j, k in enumerate(out):
            r = rows[k]
            if rank[r] < 0 or j < rank[r]:
                rank[r] = j
    return outs, rank


def limited_annotation_contract(points, instance_ids, labels, scene_offsets, ratio, min_points=5, unannotated_label=0,
                                skip_origin=True):
    """scannet_long.py:98-109 on a batch -> (labels_out, annotated_mask, rank)"""
    points = np.asarray(points, dtype=np.float32)
    ids = np.asarray(instance_ids)
    labels_out = np.array(labels, copy=True)
    mask = np.zeros(ids.shape[0], dtype=bool)
    rank = np.full(ids.shape[0], -1, dtype=np.int32)
    for b in range(len(scene_offsets) - 1):
        lo, hi = int(scene_offsets[b]), int(scene_offsets[b + 1])
        for inst in np.unique(ids[lo:hi]):
            if inst < 0:
                continue
            rows = lo + np.where(ids[lo:hi] == inst)[0]
            out = fps_contract(points[rows], count_rule(len(rows), ratio, min_points), skip_origin)
            labels_out[rows] = unannotated_label
            for j, k in enumerate(out):
                if rank[rows[k]] < 0:
                    rank[rows[k]] = j
            chosen = rows[np.unique(out)]
            labels_out[chosen] = np.asarray(labels)[chosen]
            mask[chosen] = True
    return labels_out, mask, rank


def annotation_batch(big=0):
    """3 scenes (the middle one empty): ids -1 and another negative id, an id that one scene lacks, the same id in two scenes, an
    instance of 3 points (m = 5 > n); big > 0 appends that many points of one more instance to the last scene
    -> (points, instance_ids, labels, scene_offsets)"""
    rs = np.random.RandomState(5)
    n = 160 + big
    p = rs.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    ids = np.concatenate([rs.choice([-1, 0, 2, 7], size=90, p=[0.2, 0.3, 0.3, 0.2]), rs.choice([-1, 2, 5], size=70),
                          np.full(big, 9)]).astype(np.int64)
    ids[ids == 7] = -1
    ids[[3, 50, 88]] = 7                                    # 3 points
    ids[120] = -100                                         # any negative id is "no instance"
    labels = rs.randint(1, 20, size=n).astype(np.int64)
    return p, ids, labels, [0, 90, 90, n]
