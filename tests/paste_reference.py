"""An independent numpy restatement of the reference's class-balanced instance paste (ScannetVoxelizationDataset.add_instances_to_cloud,
lib/datasets/scannet.py:143-241) for one scene: three dedups (the scene before the paste, each instance after its own voxelisation,
everything after the rotation), an explicit clamped-window maximum filter over the whole height map, sequential placement trials.
tests/test_paste_cpu.py pins it to tests/golden/paste.npz, which the reference's own function wrote; the device kernels
(csrc/lgs_paste.hip) are held to it in tests/test_gpu_paste.py.  Everything is float64 / int64; nothing here is shared with the
package under test except the Philox restatement of tests/augment_reference.py."""
import numpy as np

import augment_reference as ar

STAGE_PASTE = 17          # LGS_AUG_STAGE_PASTE


def first_rows(rows):
    """indices of the first occurrence of every distinct row, ascending (what ME.utils.sparse_quantize keeps)"""
    rows = np.asarray(rows)
    if len(rows) == 0:
        return np.zeros(0, np.int64)
    _, first = np.unique(rows, axis=0, return_index=True)
    return np.sort(first)


def affine_floor(points, m):
    """floor(M (x, y, z, 1)) per row in float64 as ((x a0 + y a1) + z a2) + a3"""
    p = np.asarray(points).astype(np.float64)
    m = np.asarray(m, np.float64)
    out = np.empty((len(p), 3))
    for r in range(3):
        out[:, r] = ((p[:, 0] * m[r, 0] + p[:, 1] * m[r, 1]) + p[:, 2] * m[r, 2]) + m[r, 3]
    return np.floor(out).astype(np.int64)


def floor_margin(points, m):
    """the smallest distance of any value that reaches the floor above from an integer"""
    p = np.asarray(points).astype(np.float64)
    v = p @ np.asarray(m, np.float64)[:3, :3].T + np.asarray(m, np.float64)[:3, 3]
    return float(np.abs(v - np.round(v)).min()) if v.size else 1.0


def height_map(coords):
    """max z per (x, y) cell over the scene's bounds, z_min where no voxel lies -> (map [dx, dy], mins, maxes)"""
    c = np.asarray(coords, np.int64)
    mins, maxes = c.min(0), c.max(0)
    hm = np.full((maxes[0] - mins[0] + 1, maxes[1] - mins[1] + 1), mins[2], np.int64)
    np.maximum.at(hm, (c[:, 0] - mins[0], c[:, 1] - mins[1]), c[:, 2])
    return hm, mins, maxes


def clamped_max_filter(hm, size=5):
    """the max over the size x size window centred on each cell, the window clamped to the map"""
    h = size // 2
    out = np.empty_like(hm)
    for i in range(hm.shape[0]):
        for j in range(hm.shape[1]):
            out[i, j] = hm[max(i - h, 0):i + h + 1, max(j - h, 0):j + h + 1].max()
    return out


def boxes_intersect(a_lo, a_hi, b_lo, b_hi):
    """inclusive on all six comparisons"""
    return bool(np.all(a_lo <= b_hi) and np.all(a_hi >= b_lo))


def philox_draws(seed, scene_seed, k, trials, mins, maxes):
    """the device's (x, y) of every trial of instance k of a scene -> int64 [trials, 2]"""
    ctr = np.zeros((trials, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(trials), k, STAGE_PASTE, (int(seed) >> 32) & 0xffffffff
    w = ar.philox4x32_10(ctr, int(seed) & 0xffffffff, int(scene_seed) & 0xffffffff).astype(np.uint64)
    d = (np.asarray(maxes[:2], np.int64) - np.asarray(mins[:2], np.int64) + 1).astype(np.uint64)
    return np.asarray(mins[:2], np.int64) + ((w[:, :2] * d) >> np.uint64(32)).astype(np.int64)


def place(filled, mins, maxes, dims, boxes_scaled, draws, trials):
    """sequential trials -> (trial that won, `trials` if none did; centroid int64 [3])"""
    centroid = np.zeros(3, np.int64)
    half = dims.astype(np.float64) / 2.0
    for t in range(trials):
        x, y = int(draws[t][0]), int(draws[t][1])
        assert mins[0] <= x <= maxes[0] and mins[1] <= y <= maxes[1]
        h = float(filled[x - mins[0], y - mins[1]])
        centroid = np.array([x, y, int(h + dims[2] / 2.0)], np.int64)
        lo, hi = centroid - half, centroid + half
        if not any(boxes_intersect(b[0], b[1], lo, hi) for b in boxes_scaled):
            return t, centroid
    return trials, centroid


def paste_scene(coords, feats, labels, boxes, scale, m_r, instances, draws, trials, three_dedups=True, seeds=None):
    """coords int [n, 3] = floor(M_v p) (duplicates allowed), feats [n, 3], labels [n]; boxes [m, 2, 3] world corners; scale: the
    scalar of M_v; m_r [4, 4]; instances: list of (points float32 [p, 3], colors, labels, matrix [4, 4]); draws: [K, trials, 2], or None
    with seeds = (batch seed, scene seed) for the device generator.
    three_dedups: dedup the scene first and every instance after its voxelisation, as the reference does; False: no dedup before the
    final one, the instance mean still over its distinct voxels (what the device does).
    -> dict: coords / feats / labels after the final dedup, trial [K], centroid [K, 3], and the rows before the final dedup"""
    c, f, lab = np.asarray(coords, np.int64), np.asarray(feats), np.asarray(labels)
    if len(c) == 0:
        return dict(coords=c.reshape(0, 3), feats=f, labels=lab, trial=np.zeros(0, np.int64), centroid=np.zeros((0, 3), np.int64),
                    pre_coords=c.reshape(0, 3), pre_feats=f, pre_labels=lab)
    if three_dedups:
        keep = first_rows(c)
        c, f, lab = c[keep], f[keep], lab[keep]
    hm, mins, maxes = height_map(c)
    filled = clamped_max_filter(hm)
    boxes_scaled = np.asarray(boxes, np.float64).reshape(-1, 2, 3) * float(scale)
    out_c, out_f, out_l, trial_of, centroids = [c], [f], [lab], [], []
    for k, (pts, cols, labs, m) in enumerate(instances):
        v = affine_floor(pts, m)
        uniq = first_rows(v)
        dims = v.max(0) - v.min(0) + 1
        mean = np.mean(v[uniq].astype(np.float64), axis=0).astype(np.int64)      # over the distinct voxels, truncated toward zero
        d = draws[k] if draws is not None else philox_draws(seeds[0], seeds[1], k, trials, mins, maxes)
        t, centroid = place(filled, mins, maxes, dims, boxes_scaled, d, trials)
        rows = uniq if three_dedups else np.arange(len(v))
        out_c.append(v[rows] - mean + centroid)
        out_f.append(np.asarray(cols)[rows])
        out_l.append(np.asarray(labs)[rows])
        trial_of.append(t)
        centroids.append(centroid)
    pre_c = affine_floor(np.concatenate(out_c), m_r)
    pre_f, pre_l = np.concatenate(out_f), np.concatenate(out_l)
    keep = first_rows(pre_c)
    return dict(coords=pre_c[keep], feats=pre_f[keep], labels=pre_l[keep], trial=np.asarray(trial_of, np.int64),
                centroid=np.asarray(centroids, np.int64).reshape(-1, 3), pre_coords=pre_c, pre_feats=pre_f, pre_labels=pre_l)
