"""Independent numpy restatement of the device instance shifts (languagegroundedsemseg_amd/augment.py instance_shifts,
csrc/lgs_instshift.hip): the reference's ScannetVoxelizationDataset.augment_instances (lib/datasets/scannet.py:243-319) with
InstanceAugmentation (lib/transforms.py:288-382) on a batch of scenes.  Shares no code with the product.
tests/test_instshift_cpu.py holds it to the reference's recorded outputs (tests/golden/instshift.npz), tests/test_gpu_instshift.py
holds the kernels to it.  The generator path draws with the numpy Philox of tests/augment_reference.py, which
tests/test_gpu_augment.py holds to the device's words (augment.philox_words)."""
import numpy as np

from augment_reference import philox4x32_10

STAGE = 19                            # LGS_AUG_STAGE_INSTSHIFT
HUE_SETS = {1: (0,), 2: (1,), 3: (2,), 4: (0, 1)}      # Red, Green, Blue, Yellow -> the channels of the hue
ST_OVERFLOW, ST_ID_RANGE = 0, 1       # the status words: scenes left as they were (seg_cap), scenes with an id out of range


def segments(labels, ids, tail):
    """one scene -> [(label, id, rows)] ascending by (label, id), rows ascending.  Rows with id -1 or outside [0, 2^31) are in none."""
    labels, ids = np.asarray(labels, np.int64), np.asarray(ids, np.int64)
    ok = np.isin(labels, np.asarray(tail, np.int64)) & (ids >= 0) & (ids < (1 << 31))
    out = []
    for lab in np.unique(labels[ok]):
        for i in np.unique(ids[ok & (labels == lab)]):
            out.append((int(lab), int(i), np.flatnonzero(ok & (labels == lab) & (ids == i))))
    return out


def draw(seed, scene_seed, label, inst, p_color, p_scale):
    """one segment's Philox block -> (attribute, u3): counter = (id, label lo, label hi, STAGE ^ seed hi), key = (seed lo, scene seed)"""
    ctr = [[inst & 0xffffffff, label & 0xffffffff, (label >> 32) & 0xffffffff, STAGE ^ ((seed >> 32) & 0xffffffff)]]
    w = philox4x32_10(ctr, seed & 0xffffffff, int(scene_seed) & 0xffffffff)[0]
    u = w.astype(np.float64) / 4294967296.0
    if u[0] < p_color:
        return 1 + int(np.floor(6.0 * u[2])), float(u[3])
    if u[1] < p_scale:
        return (7 if 2.0 * u[2] > 1.0 else 8), float(u[3])
    return 0, float(u[3])


def draw_many(seed, scene_seed, labels, ids, p_color, p_scale):
    """draw() for many (label, id) at once -> attributes int64 [m] (the statistics test)"""
    labels, ids = np.asarray(labels, np.int64), np.asarray(ids, np.int64)
    ctr = np.stack([ids & 0xffffffff, labels & 0xffffffff, (labels >> 32) & 0xffffffff,
                    np.full_like(ids, STAGE ^ ((seed >> 32) & 0xffffffff))], 1)
    u = philox4x32_10(ctr, seed & 0xffffffff, int(scene_seed) & 0xffffffff).astype(np.float64) / 4294967296.0
    color, scale = u[:, 0] < p_color, (u[:, 0] >= p_color) & (u[:, 1] < p_scale)
    attr = np.zeros(len(ids), np.int64)
    attr[color] = 1 + np.floor(6.0 * u[color, 2]).astype(np.int64)
    attr[scale] = np.where(2.0 * u[scale, 2] > 1.0, 7, 8)
    return attr


def up_bound(scene_ext, inst_ext):
    """h = min(1.5, min over the axes of fl32(scene / inst)); an axis whose quotient is inf or NaN does not bound it"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.asarray(scene_ext, np.float32) / np.asarray(inst_ext, np.float32)
    h = 1.5
    for v in q:
        if np.isfinite(v):
            h = min(h, float(v))
    return h


def shift_colors(c, attr, hue_as_written=True):
    """float32 [m, 3] of one segment -> float32 [m, 3]"""
    c = np.asarray(c, np.float32)
    if attr == 5:
        return np.trunc(c * np.float32(0.5)).astype(np.float32)
    if attr == 6:
        return np.trunc(np.float32(255) - (np.float32(255) - c) / np.float32(2)).astype(np.float32)
    if attr not in HUE_SETS:
        return c.copy()
    mx, mn = c.max(1), c.min(1)
    in_set = np.zeros(3, bool)
    in_set[list(HUE_SETS[attr])] = True
    if hue_as_written:                # hsv_to_rgb's astype('uint8') on values in [0, 1]: only an exact 1.0 survives
        on = (mx == 255)[:, None] & (in_set[None, :] | (mx == mn)[:, None])
        return np.where(on, np.float32(255), np.float32(0)).astype(np.float32)
    return np.where(in_set[None, :], mx[:, None], mn[:, None]).astype(np.float32)


def scale_points(p, f):
    """float32 [m, 3] of one segment, factor f (float64) -> float32 [m, 3]: fl32(fl32(p fl32(f)) + fl32(c fl32(1 - f)))"""
    p = np.asarray(p, np.float32)
    lo, hi = p.min(0), p.max(0)
    c = np.array([(lo[0] + hi[0]) / np.float32(2), (lo[1] + hi[1]) / np.float32(2), lo[2]], np.float32)
    return (p * np.float32(f) + c * np.float32(1.0 - f)).astype(np.float32)


def table_size(seg_cap):
    """entries of the device's segment table: the power of two >= max(64, 2 seg_cap)"""
    t = 64
    while t < 2 * seg_cap:
        t *= 2
    return t


def instance_shifts(points, colors, labels, ids, off, tail, p_color=0.5, p_scale=0.2, seed=0, scene_seeds=None, forced=None,
                    hue_as_written=True, seg_cap=None, decisions=None):
    """a batch -> (points, colors, labels2 [n, 2], ids, order, status [2] scene masks).  forced: (keys [m, 3], attribute [m],
    factor [m]) or None.  seg_cap: a scene with a segment whose rank among the batch's segments is >= seg_cap is left as it was;
    every scene is if the batch has more segments than the device's table has entries (table_size(seg_cap)).
    decisions: a list that receives (scene, label, id, attribute, factor) per segment."""
    points, colors = np.asarray(points, np.float32), np.asarray(colors, np.float32)
    labels, ids = np.asarray(labels, np.int64), np.asarray(ids, np.int64)
    B = len(off) - 1
    scene_seeds = [0] * B if scene_seeds is None else scene_seeds
    table = {}
    if forced is not None:
        for k, a, f in zip(np.asarray(forced[0]).reshape(-1, 3).tolist(), np.asarray(forced[1]).tolist(), np.asarray(forced[2]).tolist()):
            table[tuple(k)] = (int(a), float(f))
    out_p, out_c, out_l, out_i, order = points.copy(), colors.copy(), np.stack([labels, np.zeros_like(labels)], 1), ids.copy(), []
    status = [0, 0]
    rank = 0
    if seg_cap is not None:
        total = sum(len(segments(labels[off[s]:off[s + 1]], ids[off[s]:off[s + 1]], tail)) for s in range(B))
        if total > table_size(seg_cap):
            status[ST_OVERFLOW], seg_cap = (1 << B) - 1, -1
    for s in range(B):
        a, b = int(off[s]), int(off[s + 1])
        lab, iid = labels[a:b], ids[a:b]
        if np.any(np.isin(lab, tail) & (iid != -1) & ((iid < 0) | (iid >= (1 << 31)))):
            status[ST_ID_RANGE] |= 1 << s
        segs = segments(lab, iid, tail)
        rank += len(segs)
        if seg_cap is not None and (seg_cap < 0 or (segs and rank > seg_cap)):
            status[ST_OVERFLOW] |= 1 << s
            order.append(np.arange(a, b))
            continue
        moved = np.zeros(b - a, bool)
        for _, _, rows in segs:
            moved[rows] = True
        scene_order = [np.flatnonzero(~moved)] + [rows for _, _, rows in segs]
        p_s, c_s = points[a:b], colors[a:b]
        scene_ext = (p_s.max(0) - p_s.min(0)) if b > a else np.zeros(3, np.float32)
        for label, inst, rows in segs:
            if forced is not None:
                attr, f = table.get((s, label, inst), (0, 1.0))
            else:
                attr, u3 = draw(seed, scene_seeds[s], label, inst, p_color, p_scale)
                if attr == 8:
                    f = 0.5 + 0.5 * u3
                else:
                    h = up_bound(scene_ext, p_s[rows].max(0) - p_s[rows].min(0))
                    f = 1.0 + (h - 1.0) * u3
            if decisions is not None:
                decisions.append((s, label, inst, attr, f))
            if 1 <= attr <= 6:
                out_c[a + rows] = shift_colors(c_s[rows], attr, hue_as_written)
            elif attr in (7, 8):
                out_p[a + rows] = scale_points(p_s[rows], f)
            out_l[a + rows, 1] = attr
        order.append(a + np.concatenate(scene_order))
    order = np.concatenate(order).astype(np.int64) if order else np.zeros(0, np.int64)
    return out_p[order], out_c[order], out_l[order], out_i[order], order, status
