"""From voxel predictions back to the original point cloud, on the device.

Every number the reference reports at the end is in point space.  Two call sites carry voxel results to points, both by a
nearest-neighbour search on the host:

  * `ScannetVoxelizationDataset.test_pointcloud` (lib/datasets/scannet.py:391-439): a scipy KD-tree over `coords * voxel_size`, every
    vertex of the full PLY takes the label of its nearest voxel, `fast_hist` of that is the test mIoU;
  * `get_original_pointcloud` (downstream/insseg/datasets/scannet.py:149-170): a brute-force arg-min (pykeops) from every vertex to the
    voxel centres `coords + 0.5` taken through the inverse voxelisation matrix, in every validation iteration
    (`output[inds]`, `pt_offsets.F[inds]`: pl_Trainer.py:339-344).

Here both are one query of the coordinate map the network already ran on (`lgs_manager_nearest`: a ring search through the map's
block directory, an exact scan for the rare rest), with no host synchronisation.  The search runs in the SITE FRAME -- the frame in
which the voxels are the integer lattice -- so the voxelisation matrix is applied to the queries instead of its inverse to the voxels;
that finds the same neighbour exactly where the matrix is a similarity (rotation, uniform scale, translation), which is what
lib/voxelizer.py:44-74 builds.  Anything else is refused by name.  There is no CPU path."""
import numpy as np
import torch
import torch.nn as nn

from . import metrics as _metrics
from .hipcall import host_offsets, require_hip

SIMILARITY_RTOL = 1e-6


def _map_of(x):
    """-> (backend manager, key id, CoordinateManager) of a SparseTensor or a (coordinate_manager, coordinate_map_key) pair"""
    if isinstance(x, (tuple, list)):
        if len(x) != 2:
            raise ValueError("nearest_voxel: expected a SparseTensor or a (coordinate_manager, coordinate_map_key) pair")
        cm, key = x
    else:
        cm, key = x.coordinate_manager, x.coordinate_map_key
    m = getattr(cm, "_m", None)
    if m is None or not hasattr(m, "nearest"):
        raise NotImplementedError("nearest_voxel needs the HIP engine: backend %r has no nearest-site query (there is no fallback)"
                                  % getattr(getattr(cm, "backend", None), "name", None))
    return m, key.id


def affines_from_transformation(transformation, b):
    """one 4x4 / 3x4 matrix (or its 16 / 12 values), or [b, 16] / [b, 12] / [b, 4, 4] / [b, 3, 4] as the reference's collate carries it
    (`transformation[i, :16]`) -> b * 12 host floats, row-major 3x4 per scene.  A linear part that is not a similarity
    (A^T A = s^2 I within SIMILARITY_RTOL) raises NotImplementedError: nearest in the site frame would not be nearest in world space."""
    t = transformation.detach().cpu().numpy() if torch.is_tensor(transformation) else np.asarray(transformation)
    t = np.asarray(t, dtype=np.float64)
    if t.ndim == 1 and t.size in (12, 16):
        t = t.reshape(1, -1)
    elif t.ndim == 2 and t.shape in ((4, 4), (3, 4)):
        t = t.reshape(1, -1)
    elif t.ndim == 3 and t.shape[1:] in ((4, 4), (3, 4)):
        t = t.reshape(t.shape[0], -1)
    if t.ndim != 2 or t.shape[1] not in (12, 16):
        raise ValueError("transformation must be 4x4, 3x4, [b, 16] or [b, 12], got shape %s" % (tuple(np.shape(transformation)),))
    if t.shape[0] == 1 and b > 1:
        t = np.repeat(t, b, 0)
    if t.shape[0] != b:
        raise ValueError("%d transformations for %d scenes" % (t.shape[0], b))
    a = t[:, :12].reshape(b, 3, 4)
    if not np.all(np.isfinite(a)):
        raise ValueError("transformation has non-finite entries")
    for s in range(b):
        lin = a[s, :, :3]
        g = lin.T @ lin
        s2 = np.trace(g) / 3.0
        if not (s2 > 0.0 and np.abs(g - s2 * np.eye(3)).max() <= SIMILARITY_RTOL * s2):
            raise NotImplementedError("nearest_voxel: the linear part of transformation %d is not a similarity (A^T A != s^2 I); an "
                                      "anisotropic or sheared voxelisation is not supported" % s)
    return a.reshape(-1).tolist()


def _check_points(points):
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a tensor [M, 3], got %s" % (tuple(points.shape) if torch.is_tensor(points) else type(points),))
    if points.dtype != torch.float32:
        raise ValueError("points must be float32, got %s" % points.dtype)
    require_hip(points, "nearest_voxel: points")


def _scene_offsets(scene_offsets, m, device):
    """-> (device int64 [b + 1], b): None = one scene; host integers are copied up, a device tensor is used as it is"""
    if scene_offsets is None:
        return torch.tensor([0, m], dtype=torch.int64, device=device), 1
    if torch.is_tensor(scene_offsets):
        if scene_offsets.dim() != 1 or scene_offsets.shape[0] < 2:
            raise ValueError("scene_offsets must be [b + 1]")
        return scene_offsets.to(device=device, dtype=torch.int64).contiguous(), scene_offsets.shape[0] - 1
    off = host_offsets(scene_offsets, m)
    return torch.tensor(off, dtype=torch.int64, device=device), len(off) - 1


def nearest_voxel(x, points, scene_offsets=None, transformation=None, anchor=0.5, return_distance=False, batch_base=0):
    """rows int64 [M]: for every point the row of `x` (a SparseTensor, or a (coordinate_manager, coordinate_map_key) pair at any tensor
    stride) whose voxel is nearest; -1 for a non-finite point or a scene without voxels.  With return_distance also d2 float32 [M], the
    squared distance in voxel units of that map.

    points [M, 3] float32 on the device, the scenes of a batch concatenated; scene_offsets ([b + 1], host integers or a device tensor)
    says where each begins, and the points of scene s see only the voxels of batch index batch_base + s.  `transformation` takes a
    point to voxel units of tensor stride 1 (the voxelisation matrix); None = the points are in those units already.  anchor: where
    in its cell a voxel sits, 0.5 = the centre `coords + 0.5`, 0.0 = the corner `coords` (`coords * voxel_size` in world units)."""
    _check_points(points)
    m, key = _map_of(x)
    pts = points.detach().contiguous()
    off, b = _scene_offsets(scene_offsets, pts.shape[0], pts.device)
    a12 = None if transformation is None else affines_from_transformation(transformation, b)
    rows, d2 = m.nearest(key, pts, off, b, batch_base, a12, anchor, return_distance)
    return (rows, d2) if return_distance else rows


def original_pointcloud_mapping(sinput, transformation, query_xyz):
    """`get_original_pointcloud` without the file read (downstream/insseg/datasets/scannet.py:149-170): (inds, query_xyz) with
    inds[i] = the row of `sinput` whose voxel centre (coords + 0.5, through the inverse of transformation[0, :16]) is nearest to vertex i.
    One scene, as there."""
    t = transformation
    if torch.is_tensor(t) or isinstance(t, np.ndarray):
        if t.ndim == 2 and t.shape[0] >= 1 and tuple(t.shape) not in ((4, 4), (3, 4)):
            t = t[0, :16]
    return nearest_voxel(sinput, query_xyz, None, t, anchor=0.5), query_xyz


class PointCloudEvaluator(nn.Module):
    """`test_pointcloud` minus the file I/O (lib/datasets/scannet.py:391-439): voxel predictions carried to the vertices of the full
    cloud by the nearest voxel, and the confusion matrix of that, kept on the device.

        ev = PointCloudEvaluator(num_labels, ignore_label).to(device)
        point_pred = ev.update(soutput.F, soutput, query_xyz, query_label, transformation=T)     # per scene or per batch
        stats = ev.compute()                                                                     # metrics.confusion_metrics

    Neither call synchronises with the host."""

    def __init__(self, num_labels, ignore_label=-1):
        super().__init__()
        self.num_labels = int(num_labels)
        self.ignore_label = int(ignore_label)
        self.register_buffer("confmat", torch.zeros(self.num_labels, self.num_labels, dtype=torch.int64))

    @torch.no_grad()
    def update(self, pred_or_scores, x, points, point_labels, transformation=None, anchor=0.0, scene_offsets=None):
        """pred_or_scores: [N] class per voxel row of `x`, or [N, C] scores (arg-max taken first, lowest index among the maxima).
        -> int64 [M], the prediction of every point (-1 where it has no voxel).  The matrix counts (label, prediction) by the rule of
        metrics.fast_hist over the points with 0 <= label < num_labels and label != ignore_label; points without a voxel count nowhere."""
        p = _metrics._features(pred_or_scores).detach()
        if p.dim() == 2:
            p = torch.max(p.float(), 1)[1]
        if p.dim() != 1:
            raise ValueError("pred_or_scores must be [N] or [N, C], got %s" % (tuple(p.shape),))
        if point_labels.shape[0] != points.shape[0]:
            raise ValueError("%d labels for %d points" % (point_labels.shape[0], points.shape[0]))
        rows = nearest_voxel(x, points, scene_offsets, transformation, anchor)
        if p.shape[0] == 0:
            point_pred = torch.full_like(rows, -1)
        else:
            point_pred = torch.where(rows >= 0, p.long()[rows.clamp_min(0)], torch.full_like(rows, -1))
        n = self.num_labels
        t = point_labels.to(rows.device).reshape(-1).long()
        w = ((t >= 0) & (t < n) & (t != self.ignore_label) & (point_pred >= 0) & (point_pred < n)).long()
        cell = torch.where(w > 0, t * n + point_pred, torch.zeros_like(t))
        self.confmat += torch.zeros(n * n, dtype=torch.int64, device=rows.device).scatter_add_(0, cell, w).view(n, n)
        return point_pred

    @torch.no_grad()
    def compute(self, groups=None):
        return _metrics.confusion_metrics(self.confmat, groups)
