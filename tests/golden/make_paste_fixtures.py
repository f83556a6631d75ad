"""Generates tests/golden/paste.npz by RUNNING THE REFERENCE'S OWN ScannetVoxelizationDataset.add_instances_to_cloud
(lib/datasets/scannet.py:143-241) as an unbound method on a stand-in object: config, VALID_CLASS_IDS, instance_sampling_weights,
bounding_boxes, id2cat_name, a real Voxelizer (lib/voxelizer.py), a load_ply_w_path that serves in-memory instances, and a temporary
directory of empty files for its os.listdir.  The reference's modules are imported from the checkout; what this machine lacks
(open3d, plyfile, ...) is replaced by stand-in modules that yield a dummy for any attribute, and the repository's MinkowskiEngine
package serves ME.utils.sparse_quantize (first occurrence wins).  random.randint, random.choice, np.random.choice, np.random.uniform
and np.random.shuffle are wrapped to RECORD what they returned.  The fixture is data only.

    python tests/golden/make_paste_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

Two scenes (key prefix "s0_" / "s1_"), K = 5 instances each, T = 50 trials, voxel size 0.05:
    points [n, 3] float32 (negative coordinates too), colors [n, 3] float32, labels [n] int64      the scene as loaded
    scale, m_r [4, 4]         the scalar of M_v and M_r that the scene's voxelize(augment=False) returned
    vox [n', 3], vox_feats, vox_labels     what add_instances_to_cloud received (the scene's first dedup is done)
    boxes [m, 2, 3] float64   the scene's instance boxes, world units
    samples [K]               np.random.choice's categories;  picked [K] the bank instance random.choice's file names
    matrices [K, 4, 4]        each instance's M_r @ M_v
    draws [K, T, 2]           what random.randint returned, (x, y) per trial; trials the reference did not run repeat the scene minimum
    trial [K]                 the trial that placed the instance, T if all T failed;  centroid [K, 3]
    out_coords, out_feats, out_labels      what add_instances_to_cloud returned
    uniform                   every np.random.uniform draw, in call order; shuffles: the order np.random.shuffle left, per call
bank_points / bank_colors / bank_labels / bank_offsets / bank_categories: the instances; class_ids, weights.
In scene 0 at least one instance lands at trial 0 and one later; scene 1's boxes cover its floor, so all of its instances exhaust the
50 trials.  Bank instance 0 has points that collide in a voxel: its mean over distinct voxels differs from its mean over rows.
The generator asserts that no value reaching a floor (instance voxelisation, final rotation) lies within 1e-6 of an integer."""
import importlib
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
K, T, VOXEL = 5, 50, 0.05
CLASS_IDS = (2, 4, 7, 9)
NAMES = {2: "chair", 4: "lamp", 7: "plant", 9: "bin"}
WEIGHTS = np.array([0.4, 0.2, 0.2, 0.2])


class _Stub(types.ModuleType):
    """a module that has every attribute: `from plyfile import PlyData` gets a dummy class"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def load_reference(ref_root):
    import collections
    import collections.abc
    if not hasattr(collections, "Iterable"):
        collections.Iterable = collections.abc.Iterable        # lib/voxelizer.py:53
    import scipy.ndimage
    if not hasattr(scipy.ndimage, "filters"):
        scipy.ndimage.filters = scipy.ndimage
    for p in (ROOT, ref_root):
        if p not in sys.path:
            sys.path.insert(0, p)           # the reference's `lib` package; the repository's MinkowskiEngine stands in for ME
    for _ in range(64):
        try:
            return importlib.import_module("lib.datasets.scannet"), importlib.import_module("lib.voxelizer")
        except ImportError as e:            # a third-party module this machine lacks, or a name a newer library dropped
            name = getattr(e, "name", None)
            if not name or name.split(".")[0] in ("lib", "MinkowskiEngine", "numpy", "torch"):
                raise
            if name in sys.modules and not isinstance(sys.modules[name], _Stub):      # `from scipy import misc` and the like
                raise
            sys.modules[name] = _Stub(name)
            if "." in name:
                setattr(importlib.import_module(name.rsplit(".", 1)[0]), name.rsplit(".", 1)[1], sys.modules[name])
    raise RuntimeError("too many missing modules")


class Recorder:
    """wraps the five generators; everything they return is kept in call order"""

    def __init__(self):
        self.randint, self.choice, self.np_choice, self.uniform, self.shuffles = [], [], [], [], []
        self._orig = (random.randint, random.choice, np.random.choice, np.random.uniform, np.random.shuffle)

    def __enter__(self):
        o_randint, o_choice, o_np_choice, o_uniform, o_shuffle = self._orig

        def keep(log, fn):
            def wrapped(*a, **kw):
                v = fn(*a, **kw)
                log.append(np.array(v) if isinstance(v, np.ndarray) else v)
                return v
            return wrapped

        def shuffle(x):
            ids = [id(e) for e in x]
            o_shuffle(x)
            self.shuffles.append([ids.index(id(e)) for e in x])
        random.randint, random.choice = keep(self.randint, o_randint), keep(self.choice, o_choice)
        np.random.choice, np.random.uniform, np.random.shuffle = keep(self.np_choice, o_np_choice), keep(self.uniform, o_uniform), shuffle
        return self

    def __exit__(self, *exc):
        random.randint, random.choice, np.random.choice, np.random.uniform, np.random.shuffle = self._orig


def make_scene(seed, n, size, origin):
    """a floor, two walls and a few blobs standing on the floor"""
    rng = np.random.default_rng(seed)
    floor = rng.random((n // 2, 3)) * [size[0], size[1], 0.04]
    wall = rng.random((n // 4, 3)) * [size[0], 0.06, size[2]]
    blobs = []
    for _ in range(4):
        centre = rng.random(3) * [size[0] - 0.6, size[1] - 0.6, 0] + [0.3, 0.3, 0]
        blobs.append(centre + rng.random((n // 16, 3)) * [0.5, 0.4, 0.3 + rng.random() * 0.6])
    pts = (np.concatenate([floor, wall] + blobs) + np.asarray(origin)).astype(np.float32)
    colors = np.floor(rng.random((len(pts), 3)) * 256).clip(0, 255).astype(np.float32)
    labels = rng.integers(0, 20, len(pts)).astype(np.int64)
    return pts, colors, labels


def make_bank():
    rng = np.random.default_rng(7)
    pts, cols, labs, cats, off = [], [], [], [], [0]
    for i, (cat, n) in enumerate([(2, 230), (2, 90), (4, 41), (4, 300), (7, 64), (7, 150), (9, 120), (9, 1)]):
        size = 0.15 + rng.random(3) * 0.45
        p = rng.random((n, 3)) * size + rng.random(3) * 3 - 1.5
        if i == 0:
            p[:150] = p[0] + rng.random((150, 3)) * 0.004          # 150 points inside a few millimetres: they collide in a voxel
        pts.append(p.astype(np.float32))
        cols.append(np.floor(rng.random((n, 3)) * 256).astype(np.float32))
        labs.append(np.full(n, cat, np.int64))
        cats.append(cat)
        off.append(off[-1] + n)
    return np.concatenate(pts), np.concatenate(cols), np.concatenate(labs), np.asarray(off, np.int64), np.asarray(cats, np.int64)


def run_scene(mod, vox_mod, bank, scene, boxes, seed, tmp):
    pts, colors, labels = scene
    b_pts, b_cols, b_labs, b_off, b_cats = bank
    random.seed(seed)
    np.random.seed(seed)
    voxelizer = vox_mod.Voxelizer(voxel_size=VOXEL, clip_bound=None, use_augmentation=True, scale_augmentation_bound=(0.9, 1.1),
                                  rotation_augmentation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)),
                                  translation_augmentation_ratio_bound=((-0.2, 0.2), (-0.2, 0.2), (0, 0)), ignore_label=255)
    transforms = []
    inner = voxelizer.get_transformation_matrix

    def recording_matrix():
        m_v, m_r = inner()
        transforms.append((m_v.copy(), m_r.copy()))
        return m_v, m_r
    voxelizer.get_transformation_matrix = recording_matrix
    log = []                                # (instance, trial, intersects, random_bb) per box test
    inner_intersect = mod.box_intersect

    def recording_intersect(a, b):
        v = inner_intersect(a, b)
        log.append((len(transforms) - 2, len(rec.randint) // 2 - 1, bool(v), np.array(b)))
        return v

    def load_ply_w_path(path, scene_name):
        i = int(os.path.basename(path).split("_")[1].split(".")[0])
        rows = slice(b_off[i], b_off[i + 1])
        return b_pts[rows], b_cols[rows], b_labs[rows], np.zeros(b_off[i + 1] - b_off[i], np.int64), None
    config = types.SimpleNamespace(is_train=True, scannet_path=tmp, num_instances_to_add=K, instance_augmentation=None,
                                   max_instance_placing_iterations=T, ignore_label=255)
    this = types.SimpleNamespace(config=config, VALID_CLASS_IDS=CLASS_IDS, instance_sampling_weights=WEIGHTS,
                                 bounding_boxes={"scene": {"instances": [{"bb": b} for b in boxes]}}, id2cat_name=NAMES,
                                 voxelizer=voxelizer, load_ply_w_path=load_ply_w_path)
    mod.box_intersect = recording_intersect
    try:
        with Recorder() as rec:
            vox, vf, vl, tr = voxelizer.voxelize(pts, colors, labels, augment=False)
            n_scene_randint = len(rec.randint)
            out_c, out_f, out_l = mod.ScannetVoxelizationDataset.add_instances_to_cloud(this, vox, vf, vl, "scene", tr)
    finally:
        mod.box_intersect = inner_intersect
    assert n_scene_randint == 0 and len(transforms) == K + 1 and len(rec.np_choice) == 1 and len(rec.choice) == K
    m_v, m_r = transforms[0]
    scale = float(m_v[0, 0])
    assert np.array_equal(m_v, np.diag([scale, scale, scale, 1.0]))
    picked = np.array([int(os.path.basename(f).split("_")[1].split(".")[0]) for f in rec.choice], np.int64)
    matrices = np.stack([t_r @ t_v for t_v, t_r in transforms[1:]])
    mins = vox.astype(np.int64).min(0)
    draws = np.tile(mins[:2], (K, T, 1)).astype(np.int64)
    trial, centroid = np.zeros(K, np.int64), np.zeros((K, 3), np.int64)
    flat = np.asarray(rec.randint, np.int64).reshape(-1, 2)
    per_instance = [sorted({t for i, t, _, _ in log if i == k}) for k in range(K)]
    at = 0
    for k in range(K):
        first = per_instance[k][0]
        n_trials = len(per_instance[k])
        assert per_instance[k] == list(range(first, first + n_trials)) and first == at
        draws[k, :n_trials] = flat[at:at + n_trials]
        last = [(hit, bb) for i, t, hit, bb in log if i == k and t == first + n_trials - 1]
        trial[k] = T if any(hit for hit, _ in last) else n_trials - 1
        assert trial[k] < T or n_trials == T
        c = (last[0][1][0] + last[0][1][1]) / 2.0
        assert np.array_equal(c, np.round(c))
        centroid[k] = c.astype(np.int64)
        at += n_trials
    assert at == len(flat)
    out = dict(points=pts, colors=colors, labels=labels, scale=np.float64(scale), m_r=m_r, vox=vox, vox_feats=vf, vox_labels=vl,
               boxes=np.asarray(boxes, np.float64), samples=np.asarray(rec.np_choice[0], np.int64), picked=picked, matrices=matrices,
               draws=draws, trial=trial, centroid=centroid, out_coords=out_c, out_feats=out_f, out_labels=out_l,
               uniform=np.asarray(rec.uniform, np.float64), shuffles=np.asarray(rec.shuffles, np.int64))
    # no value that reaches a floor lies within 1e-6 of an integer: the instance voxelisation and the final rotation
    margin = 1.0
    pre = [vox.astype(np.float64)]
    for k in range(K):
        rows = slice(b_off[picked[k]], b_off[picked[k] + 1])
        v = b_pts[rows].astype(np.float64) @ matrices[k][:3, :3].T + matrices[k][:3, 3]
        margin = min(margin, float(np.abs(v - np.round(v)).min()))
        vi = np.floor(v)
        uniq = vi[np.sort(np.unique(vi, axis=0, return_index=True)[1])]
        pre.append(vi - np.mean(uniq, axis=0).astype(int) + centroid[k])
        out["mean_differs_%d" % k] = np.bool_((np.mean(uniq, axis=0).astype(int) != np.mean(vi, axis=0).astype(int)).any())
    w = np.concatenate(pre) @ m_r[:3, :3].T
    margin = min(margin, float(np.abs(w - np.round(w)).min()))
    out["floor_margin"] = np.float64(margin)
    return out


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LGS_REFERENCE")
    if not ref_root:
        raise SystemExit(__doc__)
    mod, vox_mod = load_reference(os.path.abspath(ref_root))
    bank = make_bank()
    scenes = [make_scene(200, 3200, (4.1, 3.3, 2.4), (-2.9, -0.8, -0.35)), make_scene(201, 2400, (2.7, 1.9, 1.1), (0.4, -2.6, 0.2))]
    boxes = [np.array([[[-2.9, -0.8, -0.4], [-0.9, 2.5, 2.2]], [[-0.9, -0.8, -0.4], [1.2, 0.9, 2.2]], [[0.1, 1.6, -0.4], [0.7, 2.1, 2.2]]]),
             np.array([[[0.0, -3.0, 0.0], [3.5, -0.3, 2.0]], [[1.0, -2.0, 0.1], [1.5, -1.5, 0.6]]])]
    with tempfile.TemporaryDirectory() as tmp:
        for i, cat in enumerate(bank[4]):
            d = os.path.join(tmp, "train", "train_instances", NAMES[int(cat)])
            os.makedirs(d, exist_ok=True)
            open(os.path.join(d, "inst_%03d.ply" % i), "w").close()
        tmp_arg = tmp
        for seed in range(1000):
            got = [run_scene(mod, vox_mod, bank, scenes[s], boxes[s], 10 * seed + s, tmp_arg) for s in (0, 1)]
            t0, t1 = got[0]["trial"], got[1]["trial"]
            collide = any(g["picked"][k] == 0 and g["mean_differs_%d" % k] for g in got for k in range(K))
            if ((t0 == 0).any() and ((t0 > 0) & (t0 < T)).any() and (t1 == T).all() and collide
                    and min(g["floor_margin"] for g in got) > 1e-6):
                break
        else:
            raise RuntimeError("no seed found")
    out = dict(bank_points=bank[0], bank_colors=bank[1], bank_labels=bank[2], bank_offsets=bank[3], bank_categories=bank[4],
               class_ids=np.asarray(CLASS_IDS, np.int64), weights=WEIGHTS, seed=np.int64(seed))
    for s in (0, 1):
        assert (got[s]["vox"] < 0).any() and got[s]["floor_margin"] > 1e-6
        for k, v in got[s].items():
            out["s%d_%s" % (s, k)] = v
    path = os.path.join(HERE, "paste.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; seed", seed)
    for k, v in out.items():
        print("  %-18s %s %s" % (k, v.dtype, v.shape))
    print("trials", got[0]["trial"], got[1]["trial"])


if __name__ == "__main__":
    main()
