"""An independent numpy restatement of the instance targets of the reference's instance-segmentation trainer:
  * VoxelizationDataset.get_instance_info (downstream/insseg/datasets/dataset.py:280-304) with the masking of :336-341, for one scene
    and for a batch (an instance is the pair (batch index, id));
  * the two offset losses of downstream/insseg/lib/pl_Trainer.py:286-298, in float64.
tests/test_insttarget_cpu.py pins it to tests/golden/insttarget.npz, which the reference's own function wrote, and to the losses of
tests/golden/insseg_res16unet14a_forward.npz; the device kernels (csrc/lgs_insttarget.hip) are held to it in tests/test_gpu_insttarget.py.
Written on one stable sort and segment reductions, not on one mask per id; integer sums are int64 and exact, a centre is one float64
quotient rounded to float32 -- which is what numpy's mean of an integer array stored into a float32 row gives.  Nothing here is
shared with the package under test."""
import numpy as np


def mask_ids(instance_ids, labels=None, masked_labels=()):
    """the ids after the masking of dataset.py:336-341: -1 where the label is one of masked_labels"""
    ids = np.array(instance_ids, dtype=np.int64, copy=True)
    for v in masked_labels:
        ids[np.asarray(labels) == v] = -1
    return ids


def segments(keys):
    """-> (order, starts, uniq): rows sorted stably by key, the start of every run, its key"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if len(sk) else np.zeros(0, np.int64)
    return order, starts, sk[starts]


def instance_table(xyz, keys):
    """per distinct key >= 0 (ascending): (uniq [G], count [G] int64, bbox [G, 6] int64, center [G, 3] float32, row_of_point [n], -1 = none)"""
    xyz = np.asarray(xyz).astype(np.int64).reshape(-1, 3)
    keys = np.asarray(keys, dtype=np.int64)
    has = np.flatnonzero(keys >= 0)
    order, starts, uniq = segments(keys[has])
    g = len(uniq)
    row_of_point = np.full(len(keys), -1, np.int64)
    if g == 0:
        return uniq, np.zeros(0, np.int64), np.zeros((0, 6), np.int64), np.zeros((0, 3), np.float32), row_of_point
    pts = xyz[has][order]
    count = np.diff(np.concatenate([starts, [len(order)]]))
    sums = np.add.reduceat(pts, starts, axis=0)
    lo, hi = np.minimum.reduceat(pts, starts, axis=0), np.maximum.reduceat(pts, starts, axis=0)
    center = (sums.astype(np.float64) / count[:, None].astype(np.float64)).astype(np.float32)
    row_of_point[has[order]] = np.repeat(np.arange(g), count)
    return uniq, count, np.concatenate([lo, hi], 1), center, row_of_point


def get_instance_info(xyz, instance_ids):
    """one scene -> {"ids", "center" [n, 3] float32 (-1 without an instance), "occupancy" {id: points}, "bbox" {id: [6]}}"""
    ids = np.asarray(instance_ids, dtype=np.int64)
    uniq, count, bbox, center, row = instance_table(xyz, np.where(ids == -1, -1, ids))
    centers = np.full((len(ids), 3), -1, np.float32)
    centers[row >= 0] = center[row[row >= 0]]
    return {"ids": ids, "center": centers, "occupancy": {int(u): int(c) for u, c in zip(uniq, count)},
            "bbox": {int(u): b for u, b in zip(uniq, bbox)}}


def batch_keys(coords, ids):
    """(batch << 32) | id per row, -1 where the id is -1"""
    coords, ids = np.asarray(coords).astype(np.int64), np.asarray(ids, dtype=np.int64)
    return np.where(ids == -1, -1, (coords[:, 0] << 32) | ids)


def batch_instance_info(coords, ids):
    """a batch (coords [n, 4], batch index in column 0; ids after masking) -> (keys [G] ascending, count, bbox, center, row_of_point,
    centers [n, 3] float32)"""
    uniq, count, bbox, center, row = instance_table(np.asarray(coords)[:, 1:], batch_keys(coords, ids))
    centers = np.full((len(row), 3), -1, np.float32)
    centers[row >= 0] = center[row[row >= 0]]
    return uniq, count, bbox, center, row, centers


def offset_rows(pt_offsets, xyz, centers, voxel_size):
    """per row in float64: (L1 distance of po to gt, negative cosine of po and gt with the reference's + 1e-8 on both norms, gt)"""
    po = np.asarray(pt_offsets, dtype=np.float64)
    gt = (np.asarray(centers, dtype=np.float64) - np.asarray(xyz, dtype=np.float64)) * float(voxel_size)
    dist = np.abs(po - gt).sum(1)
    gt_unit = gt / (np.sqrt((gt * gt).sum(1))[:, None] + 1e-8)
    po_unit = po / (np.sqrt((po * po).sum(1))[:, None] + 1e-8)
    return dist, -(gt_unit * po_unit).sum(1), gt


def offset_losses(pt_offsets, xyz, centers, instance_ids, voxel_size):
    """-> (offset_norm_loss, offset_dir_loss) as Python floats: the means over the rows with an instance, denominator + 1e-6"""
    valid = (np.asarray(instance_ids) != -1).astype(np.float64)
    dist, direction, _ = offset_rows(pt_offsets, xyz, centers, voxel_size)
    den = valid.sum() + 1e-6
    return float((dist * valid).sum() / den), float((direction * valid).sum() / den)
