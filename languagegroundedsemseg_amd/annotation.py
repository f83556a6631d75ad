"""Furthest point sampling and the limited-annotation subsets on the device (csrc/lgs_fps.hip).

The reference draws its limited-annotation training sets offline (lib/datasets/preprocessing/scannet_long.py:98-109): for every
annotated instance of a scene, `furthest_point_sample(t_coords, max(5, round(ratio * n)))` from its pointnet2 CUDA extension, and only
the chosen points keep their label.  Here the same subsets are drawn from device tensors, per run or per epoch:

    labels, annotated, rank = limited_annotation(points, instance_ids, labels, scene_offsets, ratio=0.05)     # no host synchronisation

  furthest_point_sample            pointnet2_utils.furthest_point_sample's signature and result: [B, N, 3] -> int32 [B, npoint]
  furthest_point_sample_segments   the CSR form: many segments of different sizes in one call
  limited_annotation               one segment per (scene, instance id >= 0), the recipe's count rule, the recipe's label rule

The contract of one segment is stated in include/lgs_engine.h (fp32, every operation rounded in the written order, ties to the smallest
index).  CPU tensors, and HIP tensors under LGS_FPS_FUSED=0, take torch lines of the same contract (`fps_torch`), which synchronise."""
import numpy as np
import torch

from . import engine, instances, tuning
from .hipcall import on_device, ptr, raw_stream, scratch

TIER_BOUNDS = (256, 2048, 8192)      # LGS_FPS_WAVE_MAX, LGS_FPS_GROUP4_MAX, LGS_FPS_GROUP16_MAX: the largest segment of each register tier
MAX_SEGMENTS = 1 << 20


def _fused(t):
    return t.is_cuda and bool(tuning.host("FPS_FUSED"))


def count_rule(n, ratio, min_points=5):
    """the recipe's sample count for a segment of n points (Python's round: half to even)"""
    return max(int(min_points), round(ratio * n)) if n else 0


def fps_torch(p, m, skip_origin=True):
    """The contract in torch lines for one segment p [n, 3] float32 (any device) -> int32 [m] on p's device.  Every line is one
    rounded fp32 operation; reads one index back per round."""
    n = p.shape[0]
    m = int(m) if n else 0
    out = torch.zeros(m, dtype=torch.int32, device=p.device)
    if m <= 1:
        return out
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    ok = ((x * x + y * y) + z * z) > 1e-3 if skip_origin else torch.ones(n, dtype=torch.bool, device=p.device)
    t = torch.full((n,), 1e10, dtype=torch.float32, device=p.device)
    below = torch.full((n,), -1.0, dtype=torch.float32, device=p.device)
    o = 0
    for j in range(1, m):
        dx, dy, dz = x - x[o], y - y[o], z - z[o]
        t = torch.minimum((dx * dx + dy * dy) + dz * dz, t)
        te = torch.where(ok, t, below)
        top = te.max()
        o = int(torch.nonzero(te == top)[0]) if float(top) >= 0 else 0      # the smallest index at the maximum
        out[j] = o
    return out


def _segments_torch(points, seg_offsets, counts, through, skip_origin):
    """the CSR form in torch lines -> ([out per segment], rank int32 [N]); counts: one host integer per segment"""
    n = points.shape[0]
    off = [min(max(int(v), 0), n) for v in seg_offsets.tolist()]
    for q in range(1, len(off)):
        off[q] = max(off[q], off[q - 1])
    rank = torch.full((n,), -1, dtype=torch.int32, device=points.device)
    outs = []
    for q in range(len(off) - 1):
        rows = torch.arange(off[q], off[q + 1], device=points.device)
        if through is not None:
            rows = through[rows].clamp(0, max(n - 1, 0))
        out = fps_torch(points[rows], counts[q], skip_origin)
        outs.append(out)
        if out.numel():
            chosen = rows[out.long()]
            first = torch.full((n,), 2 ** 31 - 1, dtype=torch.int32, device=points.device)
            first.scatter_reduce_(0, chosen, torch.arange(out.numel(), dtype=torch.int32, device=points.device), "amin")
            hit = first != 2 ** 31 - 1
            rank = torch.where(hit & ((rank < 0) | (first < rank)), first, rank)
    return outs, rank


def _check_points(points, what):
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("%s: points must be a float32 [N, 3] tensor (fp64 and fp16 points are out of scope)" % what)
    return points.detach().contiguous()


def _offsets_on(seg_offsets, device):
    if isinstance(seg_offsets, torch.Tensor):
        off = seg_offsets.detach().to(device=device, dtype=torch.int64).contiguous()
    else:
        off = torch.tensor([int(v) for v in seg_offsets], dtype=torch.int64, device=device)
    if off.dim() != 1 or off.shape[0] < 1 or off.shape[0] - 1 > MAX_SEGMENTS:
        raise ValueError("seg_offsets must be int64 [S + 1] with 0 <= S <= %d" % MAX_SEGMENTS)
    return off


def _fps_call(points, through, off, counts=None, fixed_count=-1, ratio=0.0, min_points=5, skip_origin=True, out_offsets=None,
              idx_out=None, rank_out=None):
    """lgs_fps_segments on checked device tensors; nothing synchronises"""
    L = engine.lib()
    dev = points.device
    n, s = points.shape[0], off.shape[0] - 1
    nbytes = int(L.lgs_fps_workspace_bytes(n, s))
    if nbytes <= 0:
        raise ValueError("furthest point sampling: bad shape (%d rows, %d segments)" % (n, s))
    with on_device(dev):
        ws = scratch(nbytes, dev)          # (lgs_fps_segments initialises what it reads of it)
        engine.check(L.lgs_fps_segments(ptr(points), n, ptr(through), ptr(off), s, ptr(counts), int(fixed_count), float(ratio),
                                        int(min_points), 1 if skip_origin else 0, ptr(out_offsets), ptr(idx_out), ptr(rank_out),
                                        ptr(ws), raw_stream()))


def furthest_point_sample(xyz, npoint):
    """xyz [B, N, 3] float32, npoint -> int32 [B, npoint]: pointnet2_utils.furthest_point_sample (non-differentiable).  One call with
    B segments; no host synchronisation on HIP tensors."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("furthest_point_sample: xyz must be a float32 [B, N, 3] tensor")
    npoint = int(npoint)
    if npoint < 0:
        raise ValueError("furthest_point_sample: npoint = %d" % npoint)
    B, N = xyz.shape[0], xyz.shape[1]
    xyz = xyz.detach().contiguous()
    if not _fused(xyz):
        if B == 0 or N == 0:
            return torch.zeros((B, npoint), dtype=torch.int32, device=xyz.device)
        return torch.stack([fps_torch(xyz[b], npoint) for b in range(B)])
    with on_device(xyz.device):
        idx = torch.zeros((B, npoint), dtype=torch.int32, device=xyz.device)
        if B and N and npoint:
            off = torch.arange(B + 1, dtype=torch.int64, device=xyz.device) * N
            _fps_call(xyz.view(B * N, 3), None, off, fixed_count=npoint, idx_out=idx)
    return idx


def furthest_point_sample_segments(points, seg_offsets, counts=None, ratio=None, min_points=5, through=None, skip_origin=True):
    """The CSR form.  points float32 [N, 3]; segment q owns the positions [seg_offsets[q], seg_offsets[q + 1]) (int64 [S + 1], a tensor
    or a host sequence; clamped into a non-decreasing table on [0, N]); position u is row through[u] (int64 [N]) or row u.
      counts = an int, or one integer per segment: the counts are known, -> (idx, out_offsets).  idx int32 [sum of counts]: segment
               q's picks, LOCAL to the segment, at out_offsets[q] (int64 [S + 1], on the device); the entries of an empty segment
               stay 0.  A host sequence costs no synchronisation; a device tensor of counts is read back once to size idx.
      ratio  = the recipe's rule max(min_points, round(ratio * n_q)), computed on the device, -> rank int32 [N]: per ROW the first
               round that chose it, -1 for every other row.  No output capacity, so no host round trip."""
    points = _check_points(points, "furthest_point_sample_segments")
    dev, n = points.device, points.shape[0]
    if (counts is None) == (ratio is None):
        raise ValueError("furthest_point_sample_segments: give counts or ratio, not both")
    if ratio is not None and not 0.0 <= float(ratio) <= 1.0:
        raise ValueError("furthest_point_sample_segments: ratio must lie in [0, 1], got %r" % (ratio,))
    off = _offsets_on(seg_offsets, dev)
    s = off.shape[0] - 1
    if through is not None:
        if not isinstance(through, torch.Tensor) or through.dtype != torch.int64 or through.shape != (n,):
            raise ValueError("furthest_point_sample_segments: through must be int64 [N]")
        through = through.to(dev).contiguous()
    host_counts = None
    if counts is not None:
        if isinstance(counts, (int, np.integer)):
            host_counts = [int(counts)] * s
        else:
            host_counts = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]      # (a device tensor: one read)
        if len(host_counts) != s or any(c < 0 for c in host_counts):
            raise ValueError("furthest_point_sample_segments: counts takes one non-negative integer per segment (%d)" % s)
    if not _fused(points):
        if host_counts is None:
            sizes = _segments_sizes_host(off, n)
            host_counts = [count_rule(v, float(ratio), min_points) for v in sizes]
        outs, rank = _segments_torch(points, off, host_counts, through, skip_origin)
        if counts is None:
            return rank
        idx = torch.zeros(sum(host_counts), dtype=torch.int32, device=dev)
        starts = np.concatenate([[0], np.cumsum(host_counts)]).astype(np.int64)
        for q, out in enumerate(outs):
            idx[starts[q]:starts[q] + out.numel()] = out
        return idx, torch.from_numpy(starts).to(dev)
    with on_device(dev):
        if counts is None:
            rank = torch.empty(n, dtype=torch.int32, device=dev)
            _fps_call(points, through, off, ratio=float(ratio), min_points=min_points, skip_origin=skip_origin, rank_out=rank)
            return rank
        starts = np.concatenate([[0], np.cumsum(host_counts)]).astype(np.int64)
        out_offsets = torch.from_numpy(starts).to(dev)
        idx = torch.zeros(int(starts[-1]), dtype=torch.int32, device=dev)
        if s and int(starts[-1]):
            cnt = torch.tensor(host_counts, dtype=torch.int32).to(dev)
            _fps_call(points, through, off, counts=cnt, skip_origin=skip_origin, out_offsets=out_offsets, idx_out=idx)
    return idx, out_offsets


def _segments_sizes_host(off, n):
    v = [min(max(int(x), 0), n) for x in off.tolist()]
    for q in range(1, len(v)):
        v[q] = max(v[q], v[q - 1])
    return [b - a for a, b in zip(v, v[1:])]


def _scene_of_rows(scene_offsets, n, device):
    off = _offsets_on(scene_offsets, device)
    return torch.bucketize(torch.arange(n, device=device), off[1:].contiguous(), right=True)


def limited_annotation(points, instance_ids, labels, scene_offsets, ratio, min_points=5, unannotated_label=0, skip_origin=True,
                       inst_cap=4096):
    """The limited-annotation subset of a batch (scannet_long.py:98-109) -> (labels_out, annotated_mask, rank).
    points float32 [N, 3], instance_ids [N] (< 0: no instance), labels [N], scene_offsets int64 [B + 1] (a tensor or a host sequence).
    One segment per (scene, instance id >= 0), its points in ascending row order (np.where gives the reference the same order, so the
    first pick is the instance's lowest row); max(min_points, round(ratio * n)) samples each.  Selected rows keep their label, the
    other rows of a segment get unannotated_label (the reference's zero-initialised labelled_pc), rows with id < 0 are untouched.
    annotated_mask: the selected rows; rank int32 [N]: the first round that chose the row, -1 elsewhere.
    On HIP tensors: instances.instance_info's slot and count table (at most inst_cap instances per batch), one stable sort, one scan,
    one lgs_fps_segments call; no host synchronisation anywhere."""
    points = _check_points(points, "limited_annotation")
    dev, n = points.device, points.shape[0]
    if not 0.0 <= float(ratio) <= 1.0:
        raise ValueError("limited_annotation: ratio must lie in [0, 1], got %r" % (ratio,))
    if instance_ids.shape != (n,) or labels.shape[0] != n:
        raise ValueError("limited_annotation: instance_ids and labels take one entry per point (%d)" % n)
    scene = _scene_of_rows(scene_offsets, n, dev)
    ids = instance_ids.detach().to(torch.int64)
    if _fused(points):
        with on_device(dev):
            coords = torch.zeros((n, 4), dtype=torch.int32, device=dev)
            coords[:, 0] = scene
            info = instances.instance_info(coords, torch.where(ids >= 0, ids, torch.full_like(ids, -1)), inst_cap=inst_cap,
                                           return_centers=False)
            cap = info.count.shape[0]
            in_seg = info.slot >= 0
            key = torch.where(in_seg, info.slot, torch.full_like(info.slot, cap))
            through = torch.sort(key, stable=True)[1]                  # segment after segment, ascending rows within each
            off = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
            off[1:] = torch.cumsum(info.count, 0, dtype=torch.int64)
            rank = torch.empty(n, dtype=torch.int32, device=dev)
            _fps_call(points, through, off, ratio=float(ratio), min_points=min_points, skip_origin=skip_origin, rank_out=rank)
    else:
        in_seg = ids >= 0
        key = torch.where(in_seg, (scene << 32) | ids.clamp_min(0), torch.full_like(ids, -1))
        uniq, inverse, count = torch.unique(key, return_inverse=True, return_counts=True)
        through = torch.sort(inverse, stable=True)[1]
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(count, 0)])
        first = int(uniq.numel() > 0 and int(uniq[0]) == -1)           # the rows of no instance sort in front
        off = off[first:]
        sizes = _segments_sizes_host(off, n)
        _, rank = _segments_torch(points, off, [count_rule(v, float(ratio), min_points) for v in sizes], through, skip_origin)
    selected = rank >= 0
    labels_out = torch.where(in_seg & ~selected, torch.full_like(labels, unannotated_label), labels)
    return labels_out, in_seg & selected, rank
