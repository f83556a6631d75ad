"""Instance targets of the instance-segmentation trainer on the device (csrc/lgs_insttarget.hip).

The reference builds them per scene on the host (`VoxelizationDataset.get_instance_info`, downstream/insseg/datasets/dataset.py:280-304,
after the masking of :336-341: one boolean mask over all points per instance id) and the trainer concatenates and uploads `centers` and
`ids` every step (lib/pl_Trainer.py:280-284).  Here a batch is the int32 [n, 4] coordinates of its voxels (batch index in column 0) and
one instance id per row, on the device:

    info = instance_info(coords, instance_ids, labels, masked_labels=dataset.IGNORE_LABELS_INSTANCE)     # no host synchronisation
    norm_loss, dir_loss = losses.fused_instance_offset_losses(pt_offsets.F, coords, info, dataset.VOXEL_SIZE)

An instance is the pair (batch index, id).  Host tensors raise RuntimeError: there is no CPU path (`centers_torch` states the centres
in torch lines; the loss takes them for CPU tensors and under LGS_INST_TARGETS_FUSED=0)."""
import ctypes

import numpy as np
import torch

from . import engine
from .hipcall import dtype_code, on_device, ptr, raw_stream, require_hip, scratch

MAX_INST_CAP = 65536
MAX_MASKED_LABELS = 32
STATUS_BITS = {1: "more distinct instances than inst_cap", 2: "an instance id outside [0, 2^31) other than -1",
               4: "a negative batch index"}
_WS_BYTES = {}


def _status_text(status):
    return "; ".join(text for bit, text in STATUS_BITS.items() if status & bit)


class InstanceInfo:
    """What lgs_instance_info answers, as device tensors:
      ids [n] int64           the ids after masking (-1: no instance): the reference's instance_info['ids']
      slot [n] int32          the point's row of the table, -1 for none
      center [n, 3] float32   the table's centre per point, -1 on rows without an instance (None with return_centers=False)
      key [inst_cap] int64    (batch << 32) | id, -1 on unused rows;  count [inst_cap] int32: the reference's occupancy
      bbox [inst_cap, 6] int32  min xyz, max xyz;  center_table [inst_cap, 3] float32
      status [1] int32        see STATUS_BITS; check() reads it"""

    def __init__(self, ids, slot, center, key, count, bbox, center_table, status, batch_index=None):
        self.ids, self.slot, self.center, self.key, self.count, self.bbox = ids, slot, center, key, count, bbox
        self.center_table, self.status = center_table, status
        self._batch_index = batch_index

    def check(self):
        """Reads the status word (this SYNCHRONISES, like augment.aug_status) and raises on a set bit -> self"""
        status = int(self.status.cpu()[0])
        if status:
            raise RuntimeError("instance_info: %s (status %d, inst_cap %d)" % (_status_text(status), status, self.key.shape[0]))
        return self

    def to_reference(self, scene):
        """The reference's per-scene dict {"ids", "center", "occupancy", "bbox"} on the host (numpy), for the rows whose batch index is
        `scene`: ids int64 [m], center float32 [m, 3], occupancy {id: points}, bbox {id: int [6]}.  Synchronises."""
        rows = (self._batch_index == int(scene)).cpu().numpy()
        ids = self.ids.cpu().numpy()[rows]
        slot = self.slot.cpu().numpy()[rows]
        table = self.center_table.cpu().numpy()
        center = np.where((slot >= 0)[:, None], table[np.maximum(slot, 0)], np.float32(-1)).astype(np.float32)
        key, count, bbox = self.key.cpu().numpy(), self.count.cpu().numpy(), self.bbox.cpu().numpy()
        mine = np.nonzero((key >= 0) & ((key >> 32) == int(scene)))[0]
        mine = mine[np.argsort(key[mine])]
        occupancy = {int(key[r] & 0xffffffff): int(count[r]) for r in mine}
        boxes = {int(key[r] & 0xffffffff): bbox[r].copy() for r in mine}
        return {"ids": ids, "center": center, "occupancy": occupancy, "bbox": boxes}


def _workspace(n, inst_cap, device):
    nbytes = _WS_BYTES.get(inst_cap)
    if nbytes is None:
        nbytes = int(engine.lib().lgs_instance_info_workspace_bytes(1, inst_cap))      # of inst_cap alone
        if nbytes < 0:
            raise RuntimeError("instance_info: lgs_instance_info_workspace_bytes(%d, %d) failed" % (n, inst_cap))
        _WS_BYTES[inst_cap] = nbytes
    return scratch(nbytes, device)


def instance_info(coords, instance_ids, labels=None, masked_labels=(), inst_cap=4096, return_centers=True):
    """coords int32 [n, 4] (batch index in column 0), instance_ids [n] (-1: none), HIP tensors -> InstanceInfo.
    labels [n] with masked_labels (at most 32 values): a point whose label is one of them has no instance -- what the reference does
    with ignore_mask and IGNORE_LABELS_INSTANCE before it calls get_instance_info.  More than inst_cap (1 .. 65536) distinct
    (batch, id) pairs set status bit 1.  One engine call, no host synchronisation."""
    require_hip(coords, "coords")
    require_hip(instance_ids, "instance_ids")
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError("instance_info: coords must be int32 [n, 4] with the batch index in column 0")
    n = coords.shape[0]
    if instance_ids.dim() != 1 or instance_ids.shape[0] != n:
        raise ValueError("instance_info: %s instance ids for %d rows" % (tuple(instance_ids.shape), n))
    inst_cap = int(inst_cap)
    if not 1 <= inst_cap <= MAX_INST_CAP:
        raise ValueError("instance_info: inst_cap = %d is outside 1 .. %d" % (inst_cap, MAX_INST_CAP))
    masked = [int(v) for v in masked_labels]
    if len(masked) > MAX_MASKED_LABELS:
        raise ValueError("instance_info: %d masked labels, more than %d" % (len(masked), MAX_MASKED_LABELS))
    if masked:
        if labels is None:
            raise ValueError("instance_info: masked_labels without labels")
        require_hip(labels, "labels")
        if labels.dim() != 1 or labels.shape[0] != n:
            raise ValueError("instance_info: %s labels for %d rows" % (tuple(labels.shape), n))
    dev = coords.device
    c = coords.contiguous()
    ids = instance_ids.detach().to(torch.int64).contiguous()
    lab = labels.detach().to(torch.int64).contiguous() if masked else None
    host_masked = (ctypes.c_int64 * max(len(masked), 1))(*masked)
    with on_device(dev):
        ids_out = torch.empty(n, dtype=torch.int64, device=dev)
        slot = torch.empty(n, dtype=torch.int32, device=dev)
        key = torch.empty(inst_cap, dtype=torch.int64, device=dev)
        count = torch.empty(inst_cap, dtype=torch.int32, device=dev)
        bbox = torch.empty((inst_cap, 6), dtype=torch.int32, device=dev)
        table = torch.empty((inst_cap, 3), dtype=torch.float32, device=dev)
        centers = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_centers else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(n, inst_cap, dev)
        engine.check(engine.lib().lgs_instance_info(ptr(c), ptr(ids), ptr(lab), n, host_masked, len(masked), inst_cap, ptr(ids_out), ptr(slot),
                                                    ptr(key), ptr(count), ptr(bbox), ptr(table), ptr(centers), ptr(status), ptr(ws),
                                                    raw_stream()))
    return InstanceInfo(ids_out, slot, centers, key, count, bbox, table, status, batch_index=c[:, 0])


def centers_torch(coords, ids):
    """The reference's `centers` [n, 3] float32 in torch lines, for coords [n, 4] (batch index in column 0; any device) and the ids
    after masking: per (batch, id) the mean of the coordinates, summed in float64 (exact for integer coordinates) and rounded once;
    -1 on the rows whose id is -1.  torch.unique synchronises on a device."""
    ids = ids.long()
    xyz = coords[:, 1:].to(torch.float64)
    has = ids != -1
    key = (coords[:, 0].long() << 32) | ids.clamp_min(0)
    key = torch.where(has, key, torch.full_like(key, -1))
    uniq, inverse = torch.unique(key, return_inverse=True)
    sums = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=coords.device).index_add_(0, inverse, xyz)
    counts = torch.zeros(uniq.shape[0], dtype=torch.float64, device=coords.device).index_add_(0, inverse, torch.ones_like(xyz[:, 0]))
    mean = (sums / counts[:, None]).float()[inverse]
    return torch.where(has[:, None], mean, torch.full_like(mean, -1.0))


def _partial_rows(n):
    """workgroups of the forward = rows of its partial sums: one per 2048 rows, 1 .. 1024"""
    return max(1, min(1024, (n + 2047) // 2048))


def offset_loss_forward(pt_offsets, coords, slot, center_table, voxel_size):
    """lgs_offset_loss_forward -> (norm_loss, dir_loss, valid): three device scalars (fp32), no host synchronisation"""
    require_hip(pt_offsets, "pt_offsets")
    dev = pt_offsets.device
    n = pt_offsets.shape[0]
    rows = _partial_rows(n)
    with on_device(dev):
        partial = scratch(rows * 3 * 8, dev)
        norm_loss, dir_loss, valid = (torch.empty((), dtype=torch.float32, device=dev) for _ in range(3))
        engine.check(engine.lib().lgs_offset_loss_forward(ptr(pt_offsets), ptr(coords), ptr(slot), ptr(center_table), n, float(voxel_size),
                                                          dtype_code(pt_offsets), ptr(partial), rows, ptr(norm_loss), ptr(dir_loss), ptr(valid),
                                                          raw_stream()))
    return norm_loss, dir_loss, valid


def offset_loss_backward(pt_offsets, coords, slot, center_table, voxel_size, valid, g_norm, g_dir):
    """lgs_offset_loss_backward -> d pt_offsets [n, 3] in the input's dtype; valid, g_norm, g_dir: device fp32 scalars"""
    dev = pt_offsets.device
    n = pt_offsets.shape[0]
    with on_device(dev):
        d = torch.empty_like(pt_offsets)
        engine.check(engine.lib().lgs_offset_loss_backward(ptr(pt_offsets), ptr(coords), ptr(slot), ptr(center_table), n, float(voxel_size),
                                                           dtype_code(pt_offsets), ptr(valid), ptr(g_norm), ptr(g_dir), ptr(d), raw_stream()))
    return d
