"""The reference's train-time augmentation chain on the device (csrc/lgs_augment.hip).

The reference runs these transforms as numpy / scipy code in DataLoader workers (lib/transforms.py, wired up in
lib/dataset.py:355-389): ElasticDistortion before the voxeliser; RandomHorizontalFlip, ChromaticAutoContrast, ChromaticTranslation,
ChromaticJitter (ChromaticScale when configured) after it.  Here a batch is B scenes concatenated on the device, rows of a scene
contiguous, `scene_offsets` (B + 1 host integers) saying where each begins.

    aug = DeviceAugmentation.from_dataset(ScannetVoxelization2cmDataset, config)      # the one-line switch
    coords, feats, labels = aug(points, colors, labels, scene_offsets)                 # HIP tensors in, HIP tensors out

Scalar decisions (apply or not, blend factor, translation vector, rigid matrix, seeds) are drawn on the host by `draw`; everything
per point, per voxel and per noise cell runs in HIP kernels, and nothing before the dedup's own row count synchronises.
Host tensors raise RuntimeError: there is no CPU path.

With `tail_instances=TailInstancePaste(bank, ...)` the chain also runs the reference's class-balanced instance sampling
(--sample_tail_instances, lib/datasets/scannet.py:143-241; csrc/lgs_paste.hip): the voxeliser applies M_v only, `paste_instances`
places the drawn bank instances on the scene's height map and rotates every row by M_r, and the chain's one dedup follows.

With `dropout=ratio` the chain also runs RandomDropout (csrc/lgs_dropout.hip): with probability `ratio` a scene keeps a uniformly
random int(n * (1 - ratio)) of its voxel rows, as the last transform (lib/dataset.py:385-386) or the first (`dropout_position="first"`,
downstream/insseg/datasets/dataset.py:505; `DeviceAugmentation.from_insseg_dataset` builds that recipe's chain).

With `instance_shifts=InstanceShifts(tail_labels, ...)` the chain also runs the reference's per-instance colour and scale shifts
(instance_augmentation == 'raw', lib/datasets/scannet.py:243-319 with lib/transforms.py:288-382; csrc/lgs_instshift.hip) between the
elastic stages and the voxeliser: every tail instance of a scene gets nothing, a colour shift or a scale shift, its rows move behind
the scene's other rows, and the labels come back as [n, 2] = (category, attribute).

Out of scope, refused by name: HueSaturationTranslation, the clip bound, the `instance_augmentation` keyword
(the raw shifts are instance_shifts=; the latent mode lives in the loss), instance shifts of pasted instances, the paired voxeliser."""
import collections
import ctypes
import dataclasses

import numpy as np
import torch

from . import engine
from .hipcall import host_offsets, i32, i64, on_device, ptr, raw_stream, require_hip, scratch

MAX_SCENES = engine.LGS_AUG_MAX_SCENES
DEFAULT_MAX_CELLS = 1 << 16           # 43 x 40 x 16 = 27 520 cells for an 8 m room at granularity 0.2


def _upload(array, device):
    """host array -> device without a synchronising copy (pinned staging buffer, asynchronous copy)"""
    return torch.from_numpy(np.ascontiguousarray(array)).pin_memory().to(device, non_blocking=True)


def _chunks(off):
    """scenes in groups of MAX_SCENES -> (first scene, last scene + 1)"""
    b = len(off) - 1
    return [(s, min(s + MAX_SCENES, b)) for s in range(0, b, MAX_SCENES)]


def aug_bounds(table, scene_offsets=None, batch_size=None):
    """Per-scene min / max of three columns -> (bounds [B, 6] on the device, device scene offsets [B + 1]).
    float32 [N, 3] with `scene_offsets` (a device int64 tensor, B <= 32), or int32 [N, 4] coordinates with `batch_size`: the scene
    id is column 0 and the offsets are derived from it on the device."""
    require_hip(table, "table")
    t = table.contiguous()
    dev = t.device
    with on_device(dev):
        if t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3:
            require_hip(scene_offsets, "scene_offsets (device form)")
            b, form, off = scene_offsets.shape[0] - 1, engine.LGS_AUG_F32X3, scene_offsets
        elif t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] == 4:
            b, form = int(batch_size), engine.LGS_AUG_I32X4
            off = torch.empty(b + 1, dtype=torch.int64, device=dev)
        else:
            raise ValueError("aug_bounds takes float32 [N, 3] or int32 [N, 4]")
        bounds = torch.empty((b, 6), dtype=t.dtype, device=dev)
        engine.check(engine.lib().lgs_aug_bounds(ptr(t), t.shape[0], form, ptr(off), b, ptr(bounds), raw_stream()))
    return bounds, off


def aug_status(status):
    """Reads the device status words of an elastic, paste or instance-shift call (this SYNCHRONISES) -> scenes whose noise grid
    exceeded max_cells (elastic) / that were left unpasted (paste) / that were left unshifted because the batch has more than seg_cap
    segments (instance_shifts: word 0 of its status; instance_shift_status reads both words)"""
    out = []
    if isinstance(status, torch.Tensor):          # one word: what paste_instances returns
        status = [status]
    for chunk, word in enumerate(status):
        f = ctypes.c_int(0)
        with on_device(word.device):
            engine.check(engine.lib().lgs_aug_status(ptr(word), ctypes.byref(f), raw_stream()))
        out += [chunk * MAX_SCENES + s for s in range(MAX_SCENES) if (f.value >> s) & 1]
    return out


def _pack_noise(noise, b, max_cells, device):
    host = np.zeros((b, max_cells * 3), np.float32)
    for s, a in enumerate(noise):
        if a is None:
            continue
        a = np.asarray(a, np.float32).reshape(-1)
        if a.size > max_cells * 3:
            raise ValueError("noise of scene %d has %d values, more than max_cells * 3" % (s, a.size))
        host[s, :a.size] = a
    return _upload(host, device)


def _elastic_stage(points, off_dev, b, bounds_in, granularity, magnitude, seed, scene_seeds, apply, stage, noise_dev, max_cells,
                   workspace, status):
    """one stage on at most MAX_SCENES scenes, in place -> bounds of the displaced cloud"""
    dev = points.device
    L = engine.lib()
    bounds_out = torch.empty((b, 6), dtype=torch.float32, device=dev)
    seeds = (ctypes.c_int32 * b)(*[i32(v) for v in scene_seeds])
    mask = i32(sum(1 << s for s in range(b) if apply[s]))
    engine.check(L.lgs_elastic_distort(ptr(points), points.shape[0], ptr(off_dev), b, ptr(bounds_in), float(granularity), float(magnitude),
                                       i64(seed), seeds, mask, int(stage), ptr(noise_dev), int(max_cells), ptr(workspace), ptr(bounds_out),
                                       ptr(status), raw_stream()))
    return bounds_out


def _elastic_workspace(b, max_cells, device):
    nbytes = int(engine.lib().lgs_elastic_workspace_bytes(b, int(max_cells)))
    if nbytes <= 0:
        raise ValueError("max_cells must be 27 .. 2^26")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def elastic_distortion(points, scene_offsets, granularity, magnitude, seed, noise=None, max_cells=DEFAULT_MAX_CELLS, scene_seeds=None,
                       apply=None, stage=0, return_state=False):
    """ElasticDistortion.elastic_distortion(granularity, magnitude) on every scene of a batch -> the displaced points (a new tensor).
    noise: None (Philox, keyed by seed / scene_seeds / stage) or one array per scene, [dx, dy, dz, 3] in C order (teacher-forced).
    A scene whose noise grid has more than max_cells cells is left as it is; aug_status(state["status"]) names such scenes.
    return_state: also return {"status", "bounds", "noise", "field"} (device tensors, per chunk of 32 scenes)."""
    require_hip(points, "points")
    pts = points.detach().to(torch.float32).contiguous().clone()
    assert pts.dim() == 2 and pts.shape[1] == 3
    off = host_offsets(scene_offsets, pts.shape[0])
    B = len(off) - 1
    scene_seeds = [0] * B if scene_seeds is None else list(scene_seeds)
    apply = [True] * B if apply is None else list(apply)
    dev = pts.device
    state = {"status": [], "bounds": [], "noise": [], "field": []}
    with on_device(dev):
        for s0, s1 in _chunks(off):
            b = s1 - s0
            rows = pts[off[s0]:off[s1]]
            off_dev = _upload(np.asarray(off[s0:s1 + 1], np.int64) - off[s0], dev)
            bounds, _ = aug_bounds(rows, off_dev)
            ws = _elastic_workspace(b, max_cells, dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            noise_dev = None if noise is None else _pack_noise(noise[s0:s1], b, max_cells, dev)
            out = _elastic_stage(rows, off_dev, b, bounds, granularity, magnitude, seed, scene_seeds[s0:s1], apply[s0:s1], stage, noise_dev,
                                 max_cells, ws, status)
            state["status"].append(status)
            state["bounds"].append(out)
            half = ws.numel() // 2
            state["noise"].append(noise_dev if noise_dev is not None else ws[:half].view(torch.float32)[:b * max_cells * 3].view(b, -1))
            state["field"].append(ws[half:].view(torch.float32)[:b * max_cells * 3].view(b, -1))
    return (pts, state) if return_state else pts


def voxelize_batched(points, scene_offsets, matrices, batch_base=0, offsets_dev=None):
    """ME.utils.voxelize with one rigid matrix per scene: points [N, 3] -> int32 [N, 4] = (scene, floor(M_s (x, y, z, 1))).
    matrices: [B, 4, 4] or [B, 3, 4] (host).  More than 32 scenes are split into several launches."""
    require_hip(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    assert pts.dim() == 2 and pts.shape[1] == 3
    off = host_offsets(scene_offsets, pts.shape[0])
    B = len(off) - 1
    m = np.asarray(matrices, dtype=np.float64)
    assert m.shape[0] == B and m.shape[1] in (3, 4) and m.shape[2] == 4
    dev = pts.device
    out = torch.empty((pts.shape[0], 4), dtype=torch.int32, device=dev)
    with on_device(dev):
        for s0, s1 in _chunks(off):
            b = s1 - s0
            rows, dst = pts[off[s0]:off[s1]], out[off[s0]:off[s1]]
            if offsets_dev is not None and B <= MAX_SCENES:
                off_dev = offsets_dev
            else:
                off_dev = _upload(np.asarray(off[s0:s1 + 1], np.int64) - off[s0], dev)
            a = np.ascontiguousarray(m[s0:s1, :3, :4]).reshape(-1)
            a12 = (ctypes.c_double * (12 * b))(*a.tolist())
            engine.check(engine.lib().lgs_voxelize_batched(ptr(rows), rows.shape[0], ptr(off_dev), b, a12, int(batch_base) + s0, ptr(dst), raw_stream()))
    return out


def _flip_words(flip_axes, b):
    f = np.asarray(flip_axes)
    if f.ndim == 2:                   # [B, 3] booleans
        f = (f.astype(bool) * np.array([1, 2, 4])).sum(1)
    f = f.astype(np.int64).reshape(-1)
    assert f.shape[0] == b
    return (ctypes.c_int32 * b)(*[int(v) & 7 for v in f])


def horizontal_flip(coords, flip_axes, shift=None, batch_size=None, return_offsets=False):
    """RandomHorizontalFlip's coordinate step on int32 [n, 4] batch-tagged coordinates -> new coordinates.
    flip_axes: per scene a bit mask (bit a = axis a) or [B, 3] booleans; a flipped axis becomes max - c, the max over the scene's
    rows.  shift: three integers added to every scene afterwards (the trainer's per-batch coordinate shift)."""
    require_hip(coords, "coords")
    assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4
    c = coords.contiguous().clone()
    b = int(batch_size) if batch_size is not None else len(np.asarray(flip_axes))
    if b > MAX_SCENES:
        raise ValueError("horizontal_flip takes at most %d scenes per call" % MAX_SCENES)
    with on_device(c.device):
        bounds, off = aug_bounds(c, batch_size=b)
        sh = None if shift is None else (ctypes.c_int32 * 3)(*[int(v) for v in shift])
        engine.check(engine.lib().lgs_coords_flip_shift(ptr(c), c.shape[0], ptr(off), b, ptr(bounds), _flip_words(flip_axes, b), sh, raw_stream()))
    return (c, off) if return_offsets else c       # off: the voxel rows' scene offsets, derived on the device from column 0


@dataclasses.dataclass
class ColorParams:
    """one scene's colour decisions; None = that transform is not applied"""
    blend: float = None               # ChromaticAutoContrast's blend factor
    translation: tuple = None         # ChromaticTranslation's vector (3 floats, in 0 .. 255 units)
    jitter_std: float = None          # ChromaticJitter's std (a fraction of 255)
    seed: int = 0


def chromatic_augment(colors, scene_offsets, scenes, scale=1.0, normalize=False, seed=0, noise=None):
    """ChromaticAutoContrast -> ChromaticTranslation -> ChromaticJitter -> ChromaticScale -> (f / 255 - 0.5) on float32 [n, 3] colours
    -> new colours.  scene_offsets: B + 1 host integers, or a device int64 tensor (e.g. the one aug_bounds derives from coordinates).
    scenes: one ColorParams per scene.  noise: device float32 [n, 3] standard normals for the jitter (teacher-forced) or None (Philox).
    A channel whose min equals its max over the scene is left unblended by the autocontrast (the reference yields inf / NaN)."""
    require_hip(colors, "colors")
    f = colors.detach().to(torch.float32).contiguous().clone()
    assert f.dim() == 2 and f.shape[1] == 3
    dev = f.device
    b = len(scenes)
    if b > MAX_SCENES:
        raise ValueError("chromatic_augment takes at most %d scenes per call" % MAX_SCENES)
    rec = (engine.ColorScene * b)()
    for s, p in enumerate(scenes):
        flags = 0
        if p.blend is not None:
            flags |= engine.LGS_COLOR_AUTOCONTRAST
            rec[s].blend = float(p.blend)
        if p.translation is not None:
            flags |= engine.LGS_COLOR_TRANSLATION
            for a in range(3):
                rec[s].translation[a] = float(p.translation[a])
        if p.jitter_std is not None:
            flags |= engine.LGS_COLOR_JITTER
            rec[s].jitter_std = float(p.jitter_std)
        rec[s].flags = flags
        rec[s].seed = i32(p.seed)
    with on_device(dev):
        if isinstance(scene_offsets, torch.Tensor) and scene_offsets.is_cuda:
            off_dev = scene_offsets
        else:
            off_dev = _upload(np.asarray(host_offsets(scene_offsets, f.shape[0]), np.int64), dev)
        assert off_dev.shape[0] == b + 1
        bounds, _ = aug_bounds(f, off_dev)
        nz = None
        if noise is not None:
            require_hip(noise, "noise")
            nz = noise.to(torch.float32).contiguous()
            assert nz.shape == f.shape
        engine.check(engine.lib().lgs_color_augment(ptr(f), f.shape[0], ptr(off_dev), b, ptr(bounds), rec, float(scale), int(bool(normalize)),
                                                    i64(seed), ptr(nz), raw_stream()))
    return f


def philox_words(counters, key):
    """Philox-4x32-10 blocks of the device generator: counters uint32-valued [n, 4] (device int32) -> int32 [n, 4] words (tests)"""
    require_hip(counters, "counters")
    c = counters.to(torch.int32).contiguous()
    out = torch.empty_like(c)
    with on_device(c.device):
        engine.check(engine.lib().lgs_debug_philox(ptr(c), c.shape[0], i64(key), ptr(out), raw_stream()))
    return out


DropoutOffsets = collections.namedtuple("DropoutOffsets", "device host")      # int64 [B + 1] on the device / B + 1 host integers


def _dropout_select(off_dev, n, apply, ratio, seed, scene_seeds, keys, through):
    """lgs_dropout_select on checked arguments -> (rows_out with capacity n, offsets_out), both on the device; nothing synchronises"""
    dev = off_dev.device
    b = off_dev.shape[0] - 1
    mask = sum(1 << s for s in range(b) if apply[s])
    seeds = (ctypes.c_int32 * b)(*[i32(v) for v in scene_seeds])
    L = engine.lib()
    nbytes = int(L.lgs_dropout_workspace_bytes(int(n), b))
    if nbytes <= 0:
        raise ValueError("random_dropout_rows: bad shape (n = %d rows, %d scenes)" % (n, b))
    ws = scratch(nbytes, dev)              # (lgs_dropout_select initialises what it reads of it)
    rows = torch.empty(int(n), dtype=torch.int64, device=dev)
    offsets = torch.empty(b + 1, dtype=torch.int64, device=dev)
    engine.check(L.lgs_dropout_select(ptr(off_dev), int(n), b, i32(mask), 1 - ratio, i64(seed), seeds, ptr(keys), ptr(through), ptr(ws),
                                      ptr(rows), ptr(offsets), raw_stream()))
    return rows, offsets


def random_dropout_rows(scene_offsets, n, apply, ratio=0.2, seed=0, scene_seeds=None, keys=None, through=None):
    """RandomDropout's row choice for every scene of a batch (csrc/lgs_dropout.hip) -> (rows int64 [m], offsets).
    scene_offsets: device int64 [B + 1], B <= 32, over n rows.  apply: one boolean per scene; a scene that applies keeps the
    int(n_s * (1 - ratio)) rows with the smallest (Philox key, row), the others keep every row.  rows: the kept rows in ascending
    order, scene after scene (through[row] instead when `through`, a device int64 [n] index, is given); offsets: a DropoutOffsets of
    where each scene's kept rows begin, as the device tensor and as host integers.  Reading those B + 1 integers to size `rows` is the
    call's only synchronisation.  keys: device int32 [n], read as uint32, in place of the generator (teacher-forced)."""
    ratio = float(ratio)
    if not 0.0 <= ratio < 1.0:
        raise ValueError("random_dropout_rows: ratio must lie in [0, 1), got %r" % ratio)
    require_hip(scene_offsets, "scene_offsets (device form)")
    if scene_offsets.dtype != torch.int64 or scene_offsets.dim() != 1 or not 2 <= scene_offsets.shape[0] <= MAX_SCENES + 1:
        raise ValueError("random_dropout_rows: scene_offsets must be int64 [B + 1] with 1 <= B <= %d" % MAX_SCENES)
    off_dev = scene_offsets.contiguous()
    b, n = off_dev.shape[0] - 1, int(n)
    apply = [bool(v) for v in apply]
    scene_seeds = [0] * b if scene_seeds is None else list(scene_seeds)
    if len(apply) != b or len(scene_seeds) != b:
        raise ValueError("random_dropout_rows: apply and scene_seeds take one value per scene (%d)" % b)
    for t, what, dtype in ((keys, "keys", torch.int32), (through, "through", torch.int64)):
        if t is not None:
            require_hip(t, what)
            if t.dtype != dtype or t.shape != (n,):
                raise ValueError("random_dropout_rows: %s must be %s [n]" % (what, dtype))
    keys = None if keys is None else keys.contiguous()
    through = None if through is None else through.contiguous()
    with on_device(off_dev.device):
        rows, offsets = _dropout_select(off_dev, n, apply, ratio, seed, scene_seeds, keys, through)
        host = [int(v) for v in offsets.tolist()]          # the one read
    return rows[:host[-1]], DropoutOffsets(offsets, host)


def random_dropout(coords, feats, labels, instances=None, scene_offsets=None, n=None, apply=None, **kw):
    """RandomDropout on a batch's voxel rows: random_dropout_rows (same arguments; n defaults to the number of rows) and the gathers
    -> (coords, feats, labels[, instances], rows, offsets)"""
    for t, what in ((coords, "coords"), (feats, "feats"), (labels, "labels")):
        require_hip(t, what)
    if instances is not None:
        require_hip(instances, "instances")
    rows, offsets = random_dropout_rows(scene_offsets, coords.shape[0] if n is None else n, apply, **kw)
    out = (coords.index_select(0, rows), feats.index_select(0, rows), labels.index_select(0, rows))
    if instances is not None:
        out += (instances.index_select(0, rows),)
    return out + (rows, offsets)


DEFAULT_SEG_CAP = 4096                # segments (scene, tail label, instance id) per batch of instance_shifts


def _tail_labels(tail_labels, who):
    tail = sorted({int(v) for v in np.asarray(list(tail_labels)).reshape(-1).tolist()})
    if len(tail) > engine.LGS_INSTSHIFT_MAX_TAIL:
        raise ValueError("%s: tail_labels holds %d labels, more than %d" % (who, len(tail), engine.LGS_INSTSHIFT_MAX_TAIL))
    return tail


def _check_shift_args(color_prob, scale_prob, seg_cap, who):
    if not (0.0 <= float(color_prob) <= 1.0 and 0.0 <= float(scale_prob) <= 1.0):
        raise ValueError("%s: color_prob and scale_prob must lie in [0, 1], got %r and %r" % (who, color_prob, scale_prob))
    if not 1 <= int(seg_cap) <= engine.LGS_INSTSHIFT_MAX_CAP:
        raise ValueError("%s: seg_cap must be in 1 .. %d, got %r" % (who, engine.LGS_INSTSHIFT_MAX_CAP, seg_cap))


def instance_shifts(points, colors, labels, instances, scene_offsets, tail_labels, color_prob, scale_prob, seed=0, scene_seeds=None,
                    scene_bounds=None, forced=None, hue_as_written=True, seg_cap=DEFAULT_SEG_CAP):
    """augment_instances (instance_augmentation == 'raw') on every scene of a batch (csrc/lgs_instshift.hip), without a host
    synchronisation.  points [n, 3], colors [n, 3] (0 .. 255), labels [n] (raw category ids), instances [n] (HIP tensors);
    scene_offsets: B + 1 host integers or a device int64 tensor, B <= 32; tail_labels: at most 256 category ids.
    A segment is the rows of one scene that share (label in tail_labels, instance id in [0, 2^31)).  Each gets one decision, a function
    of (seed, scene_seeds[s], label, id) alone: with probability color_prob a colour shift (attribute 1 .. 6: Red, Green, Blue, Yellow,
    Dark, Bright, uniform), else with probability scale_prob a scale shift about the box's (centre x, centre y, lowest z) (7 up, by at
    most min(1.5, what the scene's extent allows); 8 down, to at least 0.5), else nothing (0).  forced = (keys [m, 3] = (scene, label,
    id), attribute [m], factor [m] float64), host arrays, replaces the draws (teacher-forced); a segment it does not list gets 0.
    hue_as_written: the four hue shifts as the reference computes them (channels become 0 or 255); False: the evident intent.
    scene_bounds: device float32 [B, 6] as aug_bounds / the elastic stage return it; computed with aug_bounds when absent.
    -> (points [n, 3], colors [n, 3], labels2 [n, 2] int64 = (category, attribute), instances [n] int64, order [n] int64, status):
    per scene its rows of no segment, ascending, then the segments ascending by (label, id), rows ascending -- the reference's
    np.delete / np.vstack order; order[j] is the input row of output row j.  status: device int32 [2] of scene bits
    (instance_shift_status reads them): word 0, scenes left exactly as they were because the batch has more than seg_cap segments;
    word 1, scenes with a tail row whose id is neither -1 nor in [0, 2^31) (such rows, and rows with id -1, are in no segment)."""
    for t, what in ((points, "points"), (colors, "colors"), (labels, "labels"), (instances, "instances")):
        require_hip(t, what)
    tail = _tail_labels(tail_labels, "instance_shifts")
    _check_shift_args(color_prob, scale_prob, seg_cap, "instance_shifts")
    dev = points.device
    pts = points.detach().to(torch.float32).contiguous()
    col = colors.detach().to(torch.float32).contiguous()
    lab = labels.detach().to(torch.int64).contiguous()
    ids = instances.detach().to(torch.int64).contiguous()
    n = pts.shape[0]
    if pts.shape != (n, 3) or col.shape != (n, 3) or lab.shape != (n,) or ids.shape != (n,):
        raise ValueError("instance_shifts: points and colors must be [n, 3], labels and instances [n]")
    L = engine.lib()
    with on_device(dev):
        if isinstance(scene_offsets, torch.Tensor) and scene_offsets.is_cuda:
            off_dev = scene_offsets.to(torch.int64).contiguous()
        else:
            off_dev = _upload(np.asarray(host_offsets(scene_offsets, n), np.int64), dev)
        b = off_dev.shape[0] - 1
        if off_dev.dim() != 1 or not 1 <= b <= MAX_SCENES:
            raise ValueError("instance_shifts takes 1 .. %d scenes per call" % MAX_SCENES)
        scene_seeds = [0] * b if scene_seeds is None else list(scene_seeds)
        if len(scene_seeds) != b:
            raise ValueError("instance_shifts: scene_seeds takes one value per scene (%d)" % b)
        if scene_bounds is None:
            scene_bounds, _ = aug_bounds(pts, off_dev)
        require_hip(scene_bounds, "scene_bounds")
        if scene_bounds.dtype != torch.float32 or tuple(scene_bounds.shape) != (b, 6):
            raise ValueError("instance_shifts: scene_bounds must be float32 [B, 6]")
        scene_bounds = scene_bounds.contiguous()
        f_keys = f_attr = f_fac = None
        m = 0
        if forced is not None:
            keys = np.asarray(forced[0], np.int64).reshape(-1, 3)
            attr, fac = np.asarray(forced[1], np.int32).reshape(-1), np.asarray(forced[2], np.float64).reshape(-1)
            m = keys.shape[0]
            if attr.shape[0] != m or fac.shape[0] != m or (attr < 0).any() or (attr > 8).any():
                raise ValueError("instance_shifts: forced = (keys [m, 3], attribute [m] in 0 .. 8, factor [m])")
            if m == 0:                # an empty table still forces: every segment gets attribute 0
                keys, attr, fac = np.zeros((1, 3), np.int64), np.zeros(1, np.int32), np.ones(1, np.float64)
            f_keys, f_attr, f_fac = _upload(keys, dev), _upload(attr, dev), _upload(fac, dev)
        nbytes = int(L.lgs_instance_shift_workspace_bytes(n, b, int(seg_cap)))
        if nbytes <= 0:
            raise ValueError("instance_shifts: bad shape (n = %d rows, %d scenes, seg_cap = %d)" % (n, b, seg_cap))
        ws = scratch(nbytes, dev)          # (lgs_instance_shift initialises what it reads of it)
        pts_out, col_out = torch.empty_like(pts), torch.empty_like(col)
        lab_out = torch.empty((n, 2), dtype=torch.int64, device=dev)
        ids_out, order = torch.empty_like(ids), torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        tail_c = (ctypes.c_int64 * max(len(tail), 1))(*tail)
        seeds = (ctypes.c_int32 * b)(*[i32(v) for v in scene_seeds])
        engine.check(L.lgs_instance_shift(ptr(pts), ptr(col), ptr(lab), ptr(ids), n, ptr(off_dev), b, ptr(scene_bounds), tail_c, len(tail),
                                          float(color_prob), float(scale_prob), i64(seed), seeds, ptr(f_keys), ptr(f_attr), ptr(f_fac), m,
                                          int(bool(hue_as_written)), int(seg_cap), ptr(ws), ptr(pts_out), ptr(col_out), ptr(lab_out),
                                          ptr(ids_out), ptr(order), ptr(status), raw_stream()))
    return pts_out, col_out, lab_out, ids_out, order, status


def instance_shift_status(status):
    """Reads both status words of an instance_shifts call (this SYNCHRONISES)
    -> {"unshifted": scenes left as they were (more than seg_cap segments), "id_range": scenes with a tail row whose id is out of range}"""
    return {"unshifted": aug_status(status[0:1]), "id_range": aug_status(status[1:2])}


class InstanceShifts:
    """The per-instance colour and scale shifts of the reference's long-tail recipe (instance_augmentation == 'raw') as a stage of
    DeviceAugmentation: the raw category ids that count as tail, and the reference's two probabilities
    (config.instance_augmentation_color_aug_prob / _scale_aug_prob; the defaults are the config's).  See instance_shifts."""

    def __init__(self, tail_labels, color_prob=0.5, scale_prob=0.2, hue_as_written=True, seg_cap=DEFAULT_SEG_CAP):
        self.tail_labels = _tail_labels(tail_labels, "InstanceShifts")
        _check_shift_args(color_prob, scale_prob, seg_cap, "InstanceShifts")
        self.color_prob, self.scale_prob = float(color_prob), float(scale_prob)
        self.hue_as_written, self.seg_cap = bool(hue_as_written), int(seg_cap)


# ---- the chain
@dataclasses.dataclass
class AugmentPlan:
    """every scalar decision of one batch (host values); see DeviceAugmentation.draw"""
    elastic: np.ndarray               # [B] bool       ElasticDistortion applies (p = 0.95)
    flip_axes: np.ndarray             # [B] int        bit a set = horizontal axis a is flipped (0.95, then 0.5 per axis)
    autocontrast: np.ndarray          # [B] bool       (p = 0.2)
    blend: np.ndarray                 # [B] float      its blend factor
    translate: np.ndarray             # [B] bool       (p = 0.95)
    translation: np.ndarray           # [B, 3] float   (rand - 0.5) * 255 * 2 * ratio
    jitter: np.ndarray                # [B] bool       (p = 0.95)
    angles: np.ndarray                # [B, 3] float   rotation angle about x, y, z
    order: np.ndarray                 # [B, 3] int     the order in which the three rotations are multiplied
    scale: np.ndarray                 # [B] float      1 / voxel_size * U(scale bounds)
    matrices: np.ndarray              # [B, 4, 4]      M_r @ M_v of Voxelizer.get_transformation_matrix
    scene_seeds: np.ndarray           # [B] uint32     per-scene Philox key word
    seed: int                         # the batch's 64-bit Philox seed
    shift: np.ndarray                 # [3] int        the trainer's per-batch coordinate shift (zeros unless coordinate_shift)
    rotations: np.ndarray = None      # [B, 4, 4]      M_r alone (the paste rotates after it has placed the instances)
    paste: "PastePlan" = None         # the tail-instance decisions, when the chain has tail_instances
    dropout: np.ndarray = None        # [B] bool       RandomDropout applies (p = its ratio), when the chain has dropout


def axis_rotation(axis, theta):
    """expm(cross(eye(3), e_axis * theta)), lib/voxelizer.py:9-10, in closed form"""
    c, s = np.cos(theta), np.sin(theta)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def draw_rigid(r, n, voxel_size, rotation_bound=None, scale_bound=None):
    """Voxelizer.get_transformation_matrix with augmentation on, n times from the generator r
    -> (angles [n, 3], order [n, 3], scale [n], M_r [n, 4, 4], M_r @ M_v [n, 4, 4])"""
    angles = np.zeros((n, 3))
    if rotation_bound is not None:
        for a, bound in enumerate(rotation_bound):
            if bound is not None:
                angles[:, a] = r.uniform(bound[0], bound[1], n)
    order = np.stack([r.permutation(3) for _ in range(n)]) if n else np.zeros((0, 3), np.int64)
    scale = np.full(n, 1.0 / voxel_size)
    if scale_bound is not None:
        scale = scale * r.uniform(scale_bound[0], scale_bound[1], n)
    rotations, matrices = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    for s in range(n):
        rots = [axis_rotation(a, angles[s, a]) for a in range(3)]
        m_r, m_v = np.eye(4), np.eye(4)
        m_r[:3, :3] = rots[order[s, 0]] @ rots[order[s, 1]] @ rots[order[s, 2]]
        np.fill_diagonal(m_v[:3, :3], scale[s])
        rotations[s], matrices[s] = m_r, m_r @ m_v
    return angles, order, scale, rotations, matrices


# ---- class-balanced tail-instance paste
class InstanceBank:
    """The cropped instances of the training set, concatenated on the device.  points float32 [M, 3] in world units, colors [M, 3],
    labels [M] (HIP tensors); offsets: host CSR, I + 1 integers; categories: one host category id per instance."""

    def __init__(self, points, colors, labels, offsets, categories):
        for t, what in ((points, "bank points"), (colors, "bank colors"), (labels, "bank labels")):
            require_hip(t, what)
        self.points = points.detach().to(torch.float32).contiguous()
        self.colors = colors.detach().to(torch.float32).contiguous()
        self.labels = labels.detach().to(torch.int64).contiguous()
        m = self.points.shape[0]
        assert self.points.shape == (m, 3) and self.colors.shape == (m, 3) and self.labels.shape == (m,)
        self.offsets = np.asarray(offsets, np.int64).reshape(-1)
        self.categories = np.asarray(categories, np.int64).reshape(-1)
        if (len(self.offsets) != len(self.categories) + 1 or self.offsets[0] != 0 or self.offsets[-1] != m
                or (np.diff(self.offsets) < 1).any()):
            raise ValueError("InstanceBank: offsets must be I + 1 increasing integers from 0 to the number of rows, one more than categories")


@dataclasses.dataclass
class PastePlan:
    """every host decision of one batch's paste; see TailInstancePaste.draw"""
    bank: object                      # the InstanceBank the instance indices refer to
    instances: np.ndarray             # [B, K] int     bank instance per (scene, paste), -1 = none
    categories: np.ndarray            # [B, K] int     the category that was drawn for it
    matrices: np.ndarray              # [B, K, 4, 4]   the instance's own M_r @ M_v (it is voxelised with augmentation on)
    scene_seeds: np.ndarray           # [B] uint32     per-scene Philox key word
    seed: int                         # the batch's 64-bit Philox seed
    max_iterations: int               # placement trials per instance
    max_map_cells: int                # a scene whose height map is larger is left unpasted


class TailInstancePaste:
    """The host side of --sample_tail_instances: per scene num_instances categories from class_ids with probability weights
    (np.random.choice(VALID_CLASS_IDS, n, p=instance_sampling_weights)), one instance of that category uniformly
    (random.choice(os.listdir(cat_path))), and the instance's own voxeliser matrix.  `bank` needs host `offsets` and `categories`."""

    def __init__(self, bank, class_ids, weights, num_instances=5, max_iterations=50, max_map_cells=1 << 18, seed=0, rigid=None):
        self.bank = bank
        self.class_ids = np.asarray(class_ids, np.int64).reshape(-1)
        w = np.asarray(weights, np.float64).reshape(-1)
        if w.shape != self.class_ids.shape or (w < 0).any() or not w.sum() > 0:
            raise ValueError("TailInstancePaste: weights must be one non-negative number per class id, not all zero")
        self.weights = w / w.sum()
        self.num_instances, self.max_iterations, self.max_map_cells = int(num_instances), int(max_iterations), int(max_map_cells)
        if self.num_instances < 0 or self.max_iterations < 1 or not 1 <= self.max_map_cells <= 1 << 26:
            raise ValueError("TailInstancePaste: num_instances >= 0, max_iterations >= 1, 1 <= max_map_cells <= 2^26")
        cats = np.asarray(bank.categories, np.int64)
        self.by_category = {int(c): np.flatnonzero(cats == c) for c in self.class_ids}
        missing = [int(c) for c, p in zip(self.class_ids, self.weights) if p > 0 and len(self.by_category[int(c)]) == 0]
        if missing:
            raise ValueError("TailInstancePaste: the bank has no instance of categories %r, which have a sampling weight" % missing[:8])
        self.rigid = rigid            # callable(generator, n) -> [n, 4, 4]; DeviceAugmentation binds its own voxeliser's
        self.rng = np.random.default_rng(seed)

    def draw(self, batch_size, rigid=None):
        B, K, r = int(batch_size), self.num_instances, self.rng
        if B * K > engine.LGS_PASTE_MAX_SLOTS:
            raise ValueError("TailInstancePaste: B * K = %d (scene, instance) slots, more than LGS_PASTE_MAX_SLOTS = %d"
                             % (B * K, engine.LGS_PASTE_MAX_SLOTS))
        rigid = rigid if rigid is not None else self.rigid
        categories = r.choice(self.class_ids, size=(B, K), p=self.weights).astype(np.int64)
        instances = np.zeros((B, K), np.int64)
        for s in range(B):
            for k in range(K):
                pool = self.by_category[int(categories[s, k])]
                instances[s, k] = pool[r.integers(0, len(pool))]
        matrices = np.tile(np.eye(4), (B, K, 1, 1)) if rigid is None else np.asarray(rigid(r, B * K), np.float64).reshape(B, K, 4, 4)
        scene_seeds = r.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
        return PastePlan(self.bank, instances, categories, matrices, scene_seeds, int(r.integers(0, 1 << 63)), self.max_iterations,
                         self.max_map_cells)


def paste_instances(coords, feats, labels, scene_offsets, scene_boxes, plan, scale, rotations, trial_draws=None, return_state=False):
    """add_instances_to_cloud on every scene of a batch (csrc/lgs_paste.hip), without a host synchronisation.
    coords int32 [N, 4]: scene rows at floor(M_v p), scene index in column 0; feats [N, 3]; labels [N]; scene_offsets: B + 1 host
    integers.  scene_boxes: per scene a host float64 [m_s, 2, 3] array of world-space (min, max) corners, or None.  plan: a PastePlan.
    scale [B]: the scalar of each scene's M_v; rotations [B, 4, 4] or [B, 3, 4]: each scene's M_r.
    trial_draws: None (Philox) or int [B, K, T, 2], the (x, y) of every trial (teacher-forced).
    -> (coords_out [n, 4] int32, feats_out [n, 3] float32, labels_out [n] int64, offsets_out (B + 1 host integers), status): per scene
    its own rows, then instance 0 .. K - 1, every row rotated by M_r.  A scene without rows gets no instances.  aug_status(status)
    names the scenes that were left unpasted (height map larger than plan.max_map_cells, instance voxel outside 18 bits); their
    instance rows are copies of the scene's first row, which the dedup drops.
    return_state: also {"placement": device int32 [S, 4] = (winning trial, centroid), "slots": [(scene, k)]}."""
    for t, what in ((coords, "coords"), (feats, "feats"), (labels, "labels")):
        require_hip(t, what)
    assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4
    dev = coords.device
    c = coords.contiguous()
    f = feats.detach().to(torch.float32).contiguous()
    lab = labels.detach().to(torch.int64).contiguous()
    n = c.shape[0]
    assert f.shape == (n, 3) and lab.shape == (n,)
    off = host_offsets(scene_offsets, n)
    B = len(off) - 1
    if not 1 <= B <= MAX_SCENES:
        raise ValueError("paste_instances takes 1 .. %d scenes per call" % MAX_SCENES)
    bank = plan.bank
    require_hip(bank.points, "the bank")
    inst = np.asarray(plan.instances, np.int64).reshape(B, -1)
    K, T = inst.shape[1], int(plan.max_iterations)
    if ((inst >= len(bank.categories)) | (inst < -1)).any():
        raise ValueError("paste_instances: the plan names an instance the bank does not have")
    slots = [(s, k) for s in range(B) if off[s + 1] > off[s] for k in range(K) if inst[s, k] >= 0]
    S = len(slots)
    if S > engine.LGS_PASTE_MAX_SLOTS:
        raise ValueError("paste_instances: %d (scene, instance) slots, more than LGS_PASTE_MAX_SLOTS = %d (B * K)"
                         % (S, engine.LGS_PASTE_MAX_SLOTS))
    boxes = [np.zeros((0, 6)) if bx is None else np.asarray(bx, np.float64).reshape(-1, 6) for bx in (scene_boxes or [None] * B)]
    assert len(boxes) == B
    # the tables, front to back in one buffer of 8-byte words: one pinned upload
    SC, CC = engine.LGS_PASTE_SLOT_COLS, engine.LGS_PASTE_SCENE_COLS
    slot_table, scene_table = np.zeros((S + 1, SC), np.int64), np.zeros((B + 1, CC), np.int64)
    slot_aff = np.zeros((S, 12))
    mats = np.asarray(plan.matrices, np.float64).reshape(B, K, 4, 4)
    rows = np.diff(bank.offsets)
    offsets_out, pos, inst_rows, at = [0], 0, 0, 0
    for s in range(B):
        scene_table[s] = (pos, sum(len(b_) for b_ in boxes[:s]), int(np.asarray(plan.scene_seeds)[s]), off[s])
        pos += off[s + 1] - off[s]
        while at < S and slots[at][0] == s:
            k = slots[at][1]
            i = int(inst[s, k])
            slot_table[at] = (bank.offsets[i], inst_rows, pos, s, k, rows[i])
            slot_aff[at] = mats[s, k, :3, :4].reshape(-1)
            pos, inst_rows, at = pos + int(rows[i]), inst_rows + int(rows[i]), at + 1
        offsets_out.append(pos)
    n_boxes = sum(len(b_) for b_ in boxes)
    slot_table[S, 1] = inst_rows
    scene_table[B] = (pos, n_boxes, 0, n)
    xf = np.zeros((B, 13))
    xf[:, 0] = np.asarray(scale, np.float64).reshape(B)
    xf[:, 1:] = np.asarray(rotations, np.float64)[:, :3, :4].reshape(B, 12)
    parts = [slot_table.reshape(-1), slot_aff.reshape(-1).view(np.int64), scene_table.reshape(-1), xf.reshape(-1).view(np.int64),
             np.concatenate(boxes).reshape(-1).view(np.int64)]
    starts = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    draws = None
    if trial_draws is not None and S:
        td = np.asarray(trial_draws).reshape(B, K, T, 2)
        draws = np.stack([td[s, k] for s, k in slots]).astype(np.int32)
    L = engine.lib()
    with on_device(dev):
        tables = _upload(np.concatenate(parts), dev)
        tab = [tables.data_ptr() + 8 * int(a) for a in starts[:5]]
        draws_dev = None if draws is None else _upload(draws, dev)
        nbytes = int(L.lgs_paste_workspace_bytes(B, S, inst_rows, int(plan.max_map_cells)))
        if nbytes <= 0:
            raise ValueError("paste_instances: bad shape (max_map_cells must be 1 .. 2^26)")
        ws = scratch(nbytes, dev)          # (lgs_paste_instances initialises what it reads of it and is done with it at the next call)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        coords_out = torch.empty((n + inst_rows, 4), dtype=torch.int32, device=dev)
        feats_out = torch.empty((n + inst_rows, 3), dtype=torch.float32, device=dev)
        labels_out = torch.empty(n + inst_rows, dtype=torch.int64, device=dev)
        placement = torch.empty((S, 4), dtype=torch.int32, device=dev)
        engine.check(L.lgs_paste_instances(ptr(c), ptr(f), ptr(lab), n, B, ptr(bank.points), ptr(bank.colors), ptr(bank.labels), bank.points.shape[0],
                                           tab[0], tab[1], S, inst_rows, tab[2], tab[3], tab[4], n_boxes, ptr(draws_dev), T, i64(plan.seed),
                                           int(plan.max_map_cells), ptr(ws), ptr(coords_out), ptr(feats_out), ptr(labels_out), ptr(placement),
                                           ptr(status), raw_stream()))
    out = (coords_out, feats_out, labels_out, offsets_out, status)
    return out + ({"placement": placement, "slots": slots},) if return_state else out


_REFUSED = ("random_dropout", "hue_saturation", "clip_bound", "instance_augmentation")


class DeviceAugmentation:
    """The reference's default train-time chain for one batch: elastic stages -> per-scene rigid matrix + floor -> dedup (first
    occurrence wins) -> flip on the voxel rows -> colour on the voxel rows.  `draw` makes the host decisions, `__call__` runs the
    kernels.  At most 32 scenes per batch.  With tail_instances (a TailInstancePaste) the second step becomes: M_v + floor -> paste
    the drawn instances -> M_r + floor of every row (paste_instances); the dedup after it is still the chain's only one.
    With dropout (a ratio) a scene drops rows with probability `ratio` (the reference's application probability IS the ratio):
    dropout_position "last" selects after the colour stage (lib/dataset.py:385-386: colour statistics over all rows), "first" right
    after the dedup (insseg dataset.py:505: flip and autocontrast see the surviving rows only).
    With instance_shifts (an InstanceShifts) the per-instance colour and scale shifts run between the elastic stages and the
    voxeliser, on the plan's seed and scene seeds (no new host draw): the voxeliser, the dedup and every later stage see the shifted,
    reordered rows, __call__ needs instances= and the labels come back as [n, 2] = (category, attribute)."""

    def __init__(self, voxel_size, elastic_params=((0.2, 0.4), (0.8, 1.6)), rotation_bound=None, scale_bound=None, rotation_axis="z",
                 color_trans_ratio=0.1, color_jitter_std=0.05, color_scale=1.0, normalize_color=False, coordinate_shift=False,
                 max_cells=DEFAULT_MAX_CELLS, seed=0, random_dropout=None, hue_saturation=None, clip_bound=None,
                 instance_augmentation=None, num_pairs=1, tail_instances=None, dropout=None, dropout_position="last",
                 instance_shifts=None):
        given = dict(random_dropout=random_dropout, hue_saturation=hue_saturation, clip_bound=clip_bound,
                     instance_augmentation=instance_augmentation)
        for name in _REFUSED:
            if given[name] is not None:
                hint = {"random_dropout": "; RandomDropout on the device is dropout=ratio",
                        "instance_augmentation": "; the raw colour / scale shifts on the device are instance_shifts=InstanceShifts(...)"
                        }.get(name, "")
                raise NotImplementedError("DeviceAugmentation: %s is not part of the device chain (DESIGN.md section 8)%s" % (name, hint))
        if num_pairs != 1:
            raise NotImplementedError("DeviceAugmentation: the paired voxeliser (num_pairs == 2) is not part of the device chain")
        self.voxel_size = float(voxel_size)
        self.elastic_params = tuple((float(g), float(m)) for g, m in elastic_params) if elastic_params is not None else ()
        self.rotation_bound = rotation_bound
        self.scale_bound = scale_bound
        self.upright = {"x": 0, "y": 1, "z": 2}[rotation_axis.lower()]
        self.color_trans_ratio = float(color_trans_ratio)
        self.color_jitter_std = float(color_jitter_std)
        self.color_scale = float(color_scale)
        self.normalize_color = bool(normalize_color)
        self.coordinate_shift = bool(coordinate_shift)
        self.max_cells = int(max_cells)
        self.rng = np.random.default_rng(seed)
        self.tail = tail_instances
        self.shifts = instance_shifts
        if self.shifts is not None and not isinstance(self.shifts, InstanceShifts):
            raise ValueError("DeviceAugmentation: instance_shifts must be an InstanceShifts, got %r" % type(instance_shifts).__name__)
        if self.shifts is not None and self.tail is not None:
            raise NotImplementedError("DeviceAugmentation: instance_shifts together with tail_instances is not part of the device chain "
                                      "(the pasted instances would need their own shifts and the two-column label; DESIGN.md section 8)")
        self.dropout = None if dropout is None else float(dropout)
        if self.dropout is not None and not 0.0 <= self.dropout < 1.0:
            raise ValueError("DeviceAugmentation: dropout must be a ratio in [0, 1), got %r" % dropout)
        if dropout_position not in ("first", "last"):
            raise ValueError("DeviceAugmentation: dropout_position must be 'first' or 'last', got %r" % (dropout_position,))
        self.dropout_position = dropout_position
        if self.tail is not None and self.tail.rigid is None:          # an instance is voxelised by the scene's voxeliser, augmentation on
            self.tail.rigid = lambda r, n: draw_rigid(r, n, self.voxel_size, self.rotation_bound, self.scale_bound)[4]

    @classmethod
    def from_dataset(cls, DatasetClass, config, **kw):
        """The chain a reference dataset class and config describe (lib/dataset.py:337-389, lib/datasets/scannet.py)."""
        if getattr(DatasetClass, "CLIP_BOUND", None) is not None:
            kw.setdefault("clip_bound", DatasetClass.CLIP_BOUND)
        if float(getattr(config, "data_aug_patch_dropout_ratio", 0.35)) == 0.0 and kw.get("dropout") is None:
            kw.setdefault("random_dropout", 0.2)          # lib/dataset.py:385 adds RandomDropout in that case only: say dropout=0.2
        elastic = DatasetClass.ELASTIC_DISTORT_PARAMS if getattr(config, "elastic_distortion", True) else None
        bank, weights = kw.pop("instance_bank", None), kw.pop("instance_sampling_weights", None)
        tail_labels = kw.pop("tail_labels", None)
        if getattr(config, "instance_augmentation", None) == "raw" and kw.get("instance_shifts") is None:
            if tail_labels is None:
                raise NotImplementedError("DeviceAugmentation: config.instance_augmentation == 'raw' needs tail_labels= (the raw category "
                                          "ids that count as tail); without them the recipe would train without its instance shifts")
            kw["instance_shifts"] = InstanceShifts(tail_labels, config.instance_augmentation_color_aug_prob,
                                                   config.instance_augmentation_scale_aug_prob)
        if getattr(config, "sample_tail_instances", False) and kw.get("tail_instances") is None:
            if bank is None:
                raise NotImplementedError("DeviceAugmentation: config.sample_tail_instances needs instance_bank= (the cropped training "
                                          "instances as an InstanceBank); without one the recipe would train without its tail instances")
            ids = np.asarray(DatasetClass.VALID_CLASS_IDS)
            kw["tail_instances"] = TailInstancePaste(bank, ids, np.ones(len(ids)) if weights is None else weights,
                                                     num_instances=config.num_instances_to_add,
                                                     max_iterations=config.max_instance_placing_iterations, seed=kw.get("seed", 0))
        return cls(voxel_size=DatasetClass.VOXEL_SIZE, elastic_params=elastic,
                   rotation_bound=DatasetClass.ROTATION_AUGMENTATION_BOUND, scale_bound=DatasetClass.SCALE_AUGMENTATION_BOUND,
                   rotation_axis=DatasetClass.ROTATION_AXIS, color_trans_ratio=config.data_aug_color_trans_ratio,
                   color_jitter_std=config.data_aug_color_jitter_std, color_scale=config.data_aug_color_scaling_factor,
                   normalize_color=config.normalize_color, **kw)

    @classmethod
    def from_insseg_dataset(cls, DatasetClass, config, **kw):
        """The chain the instance-segmentation recipe describes (downstream/insseg/datasets/dataset.py:471-541 with augment_data):
        ElasticDistortion whenever the class has parameters (there is no elastic_distortion flag there), the voxeliser of
        dataset.py:244-252, then RandomDropout(0.2) FIRST, flip, autocontrast, translation, jitter; no ChromaticScale; the per-sample
        coordinate shift of dataset.py:330-332.  config: the recipe's nested config (config.augmentation.*)."""
        if getattr(DatasetClass, "CLIP_BOUND", None) is not None:
            kw.setdefault("clip_bound", DatasetClass.CLIP_BOUND)
        a = config.augmentation
        kw.setdefault("dropout", 0.2)
        kw.setdefault("dropout_position", "first")
        kw.setdefault("coordinate_shift", True)
        return cls(voxel_size=DatasetClass.VOXEL_SIZE, elastic_params=DatasetClass.ELASTIC_DISTORT_PARAMS,
                   rotation_bound=DatasetClass.ROTATION_AUGMENTATION_BOUND, scale_bound=DatasetClass.SCALE_AUGMENTATION_BOUND,
                   rotation_axis=DatasetClass.ROTATION_AXIS, color_trans_ratio=a.data_aug_color_trans_ratio,
                   color_jitter_std=a.data_aug_color_jitter_std, color_scale=1.0,
                   normalize_color=bool(getattr(a, "normalize_color", False)), **kw)

    def draw(self, batch_size):
        """Every decision the reference draws with random.random() / np.random.uniform, for each scene of a batch."""
        B, r = int(batch_size), self.rng
        horz = [a for a in range(3) if a != self.upright]
        elastic = r.random(B) < 0.95
        flip_on, flip_ax = r.random(B) < 0.95, r.random((B, 3)) < 0.5
        flip_axes = np.zeros(B, np.int64)
        for a in horz:
            flip_axes |= (flip_on & flip_ax[:, a]).astype(np.int64) << a
        autocontrast, blend = r.random(B) < 0.2, r.random(B)
        translate = r.random(B) < 0.95
        translation = (r.random((B, 3)) - 0.5) * 255 * 2 * self.color_trans_ratio
        jitter = r.random(B) < 0.95
        angles, order, scale, rotations, matrices = draw_rigid(r, B, self.voxel_size, self.rotation_bound, self.scale_bound)
        scene_seeds = r.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
        seed = int(r.integers(0, 1 << 63))
        shift = np.floor(r.random(3) * 100).astype(np.int64) if self.coordinate_shift else np.zeros(3, np.int64)
        paste = self.tail.draw(B) if self.tail is not None else None          # from the paste's own generator
        dropout = r.random(B) < self.dropout if self.dropout is not None else None      # last: the stream before it is unchanged
        return AugmentPlan(elastic, flip_axes, autocontrast, blend, translate, translation, jitter, angles, order, scale, matrices,
                           scene_seeds, seed, shift, rotations=rotations, paste=paste, dropout=dropout)

    def color_params(self, plan):
        return [ColorParams(blend=float(plan.blend[s]) if plan.autocontrast[s] else None,
                            translation=tuple(plan.translation[s]) if plan.translate[s] else None,
                            jitter_std=self.color_jitter_std if plan.jitter[s] else None, seed=int(plan.scene_seeds[s]))
                for s in range(len(plan.elastic))]

    def __call__(self, points, colors, labels, scene_offsets, plan=None, elastic_noise=None, jitter_noise=None, return_state=False,
                 scene_boxes=None, trial_draws=None, instances=None):
        """points [N, 3], colors [N, 3], labels [N] (HIP tensors), scene_offsets (B + 1 host integers)
        -> (coords [n, 4] int32, feats [n, 3] float32, labels [n]) of the surviving voxel rows.
        instances: [N] per-point instance ids (a HIP tensor); they ride through the chain like the labels (the dedup's first
        occurrence wins) and come back as a fourth value, ready for instances.instance_info.  Refused together with tail_instances:
        pasted rows have no scene instance id.  Required with instance_shifts; the labels then come back as [n, 2] = (category,
        attribute) and return_state has "instance_shift_order" (the stage's row order) and "instance_shift_status".
        elastic_noise: per stage a list of per-scene noise arrays; jitter_noise: callable(n) or device [n, 3] normals (teacher-forced).
        With tail_instances: scene_boxes (per scene a host [m_s, 2, 3] array of the scene's instance boxes, world units) and
        optionally trial_draws, as paste_instances takes them; the voxeliser then applies M_v only and the paste rotates.
        With dropout: a batch in which plan.dropout names a scene makes one more host read (the selection's B + 1 output offsets).
        return_state then also has "dropout_rows" (the selection: input rows in first position, where they are state["keep"] too;
        voxel rows in last position; None if no scene dropped) and "dedup_keep" (the dedup's rows before any dropout)."""
        if instances is not None and self.tail is not None:
            raise NotImplementedError("DeviceAugmentation: instances= together with tail_instances is not part of the device chain "
                                      "(pasted rows have no scene instance id; DESIGN.md section 8)")
        if self.shifts is not None and instances is None:
            raise ValueError("DeviceAugmentation: instance_shifts needs instances= (one instance id per point)")
        for t, what in ((points, "points"), (colors, "colors"), (labels, "labels")):
            require_hip(t, what)
        if instances is not None:
            require_hip(instances, "instances")
            if instances.dim() != 1 or instances.shape[0] != points.shape[0]:
                raise ValueError("DeviceAugmentation: instances must be [N], one id per point")
        dev = points.device
        off = host_offsets(scene_offsets, points.shape[0])
        B = len(off) - 1
        if B > MAX_SCENES:
            raise ValueError("DeviceAugmentation takes at most %d scenes per batch" % MAX_SCENES)
        plan = self.draw(B) if plan is None else plan
        if self.tail is not None and (plan.paste is None or plan.rotations is None):
            raise ValueError("DeviceAugmentation: the plan has no paste decisions (draw it from this chain)")
        if self.dropout is not None and plan.dropout is None:
            raise ValueError("DeviceAugmentation: the plan has no dropout decisions (draw it from this chain)")
        state = {"status": [], "stages": []}
        feats_in, labels_in = None, labels
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")        # nothing before the dedup's own row count may synchronise
        try:
            with on_device(dev):
                pts = points.detach().to(torch.float32).contiguous().clone()
                off_dev = _upload(np.asarray(off, np.int64), dev)
                bounds = None
                if self.elastic_params and plan.elastic.any():
                    bounds, _ = aug_bounds(pts, off_dev)
                    ws = _elastic_workspace(B, self.max_cells, dev)
                    status = torch.zeros(1, dtype=torch.int32, device=dev)
                    for stage, (g, m) in enumerate(self.elastic_params):
                        nz = None if elastic_noise is None else _pack_noise(elastic_noise[stage], B, self.max_cells, dev)
                        bounds = _elastic_stage(pts, off_dev, B, bounds, g, m, plan.seed, plan.scene_seeds, plan.elastic, stage, nz,
                                                self.max_cells, ws, status)
                        if return_state:
                            state["stages"].append(pts.clone())
                    state["status"].append(status)
                if self.shifts is not None:
                    sh = self.shifts
                    pts, colors, labels_in, instances, order, sstatus = instance_shifts(
                        pts, colors, labels, instances, off_dev, sh.tail_labels, sh.color_prob, sh.scale_prob, seed=plan.seed,
                        scene_seeds=plan.scene_seeds, scene_bounds=bounds, hue_as_written=sh.hue_as_written, seg_cap=sh.seg_cap)
                    state.update(instance_shift_order=order, instance_shift_status=sstatus)
                if self.tail is None:
                    coords = voxelize_batched(pts, off, plan.matrices, offsets_dev=off_dev)
                else:                 # lib/datasets/scannet.py:344-347: voxelise without augmentation, paste, then rotate
                    m_v = np.tile(np.eye(4), (B, 1, 1)) * np.asarray(plan.scale).reshape(B, 1, 1)
                    m_v[:, 3, 3] = 1.0
                    vox = voxelize_batched(pts, off, m_v, offsets_dev=off_dev)
                    coords, feats_in, labels_in, off_p, pstatus, pstate = paste_instances(
                        vox, colors, labels, off, scene_boxes, plan.paste, plan.scale, plan.rotations, trial_draws=trial_draws,
                        return_state=True)
                    state.update(paste_status=pstatus, paste=pstate, paste_offsets=off_p)
                    if return_state:
                        state.update(voxels=vox, pasted=(coords, feats_in, labels_in))
        finally:
            torch.cuda.set_sync_debug_mode(previous)
        from .me.utils import sparse_quantize
        keep = sparse_quantize(coords, return_maps_only=True)          # first occurrence wins, indices ascending (one host sync)
        dropping = self.dropout is not None and bool(np.asarray(plan.dropout).any())
        rows = None                   # dropout's selection: rows of the input ("first") or of the voxel rows ("last")
        if dropping:
            drop = dict(apply=plan.dropout, ratio=self.dropout, seed=plan.seed, scene_seeds=plan.scene_seeds)
        if dropping and self.dropout_position == "first":
            # the dedup keeps ascending input rows and the input's scenes are contiguous: voxel row offsets = positions of the input's
            # scene offsets in `keep`.  The selection composes with `keep`, so every later gather is the one the chain makes anyway
            off_in = off_dev if self.tail is None else _upload(np.asarray(off_p, np.int64), dev)
            off_rows = torch.searchsorted(keep, off_in)
            state["dedup_keep"] = keep
            rows, _ = random_dropout_rows(off_rows, keep.shape[0], through=keep, **drop)      # (the chain's second host sync)
            keep = rows
        coords, off_vox = horizontal_flip(coords.index_select(0, keep), plan.flip_axes, shift=plan.shift, batch_size=B, return_offsets=True)
        feats = (colors.detach().to(torch.float32) if feats_in is None else feats_in).index_select(0, keep)
        if callable(jitter_noise):
            jitter_noise = jitter_noise(feats.shape[0])
        feats = chromatic_augment(feats, off_vox, self.color_params(plan), scale=self.color_scale, normalize=self.normalize_color,
                                  seed=plan.seed, noise=jitter_noise)
        out = (coords, feats, labels_in.index_select(0, keep).to(labels.dtype))
        if instances is not None:
            out += (instances.index_select(0, keep),)
        if dropping and self.dropout_position == "last":
            rows, _ = random_dropout_rows(off_vox, coords.shape[0], **drop)                    # (the chain's second host sync)
            out = tuple(t.index_select(0, rows) for t in out)
        if return_state:
            state["points"], state["keep"] = pts, keep
            state.setdefault("dedup_keep", keep)
            state["dropout_rows"] = rows
            return out + (state,)
        return out
