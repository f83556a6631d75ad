"""Generates tests/golden/insttarget.npz by RUNNING THE REFERENCE'S OWN VoxelizationDataset.get_instance_info
(downstream/insseg/datasets/dataset.py:280-304, loaded by file path) on a synthetic batch.  The fixture is data only: the batch and
what the reference computed on it.

    python tests/golden/make_insttarget_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

dataset.py imports plyfile, MinkowskiEngine and its sibling modules for file I/O and loaders that are not used here: all of them are
stubbed in sys.modules (the pattern of make_insteval_fixtures.py).  The function is called unbound (it does not read `self`).

3 scenes of 150 / 250 / 213 voxels (613 rows), int32 coordinates with negative values.  Ids 0 .. 7 per scene (the same ids in every
scene), 10 % of the rows -1; scene 1 holds an instance of exactly 3 points (id 9) whose mean is not representable; labels 0 .. 5, of
which 0 and 4 are masked as dataset.py:336-341 does it (`instances[labels == v] = -1`) before the call.
    coords [613, 4] int32 (batch index in column 0), instance_ids [613] int64 (before masking), labels [613] int64, masked_labels [2]
Per scene k (prefix "s<k>_"): what get_instance_info returned on the scene's rows,
    ids [m] int64, center [m, 3] float32, occ_id / occ_count [G] int64 (the occupancy dict, by ascending id), bbox [G, 6] int64."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (150, 250, 213)
MASKED = (0, 4)


def load_reference(ref_root):
    path = os.path.join(ref_root, "downstream", "insseg", "datasets", "dataset.py")
    np.int, np.float, np.bool = int, float, bool

    def stub(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    stub("plyfile", PlyData=object)
    stub("MinkowskiEngine")
    stub("datasets")
    stub("datasets.transforms")
    stub("datasets.dataloader", InfSampler=object, DistributedInfSampler=object)
    stub("datasets.voxelizer", Voxelizer=object)
    stub("lib")
    stub("lib.distributed", get_world_size=lambda: 1)
    spec = importlib.util.spec_from_file_location("reference_insseg_dataset", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_batch(seed=7):
    rng = np.random.default_rng(seed)
    coords, ids, labels = [], [], []
    for b, m in enumerate(SIZES):
        # distinct voxels around a centre that puts part of the scene at negative coordinates
        cells = rng.choice(40 * 40 * 12, m, replace=False)
        xyz = np.stack([cells % 40, cells // 40 % 40, cells // 1600], 1) + np.array([-17, 3 - 30 * b, -5])
        inst = rng.integers(0, 8, m)
        inst[rng.random(m) < 0.1] = -1
        if b == 1:
            inst[:3] = 9
            xyz[:3] = [[1, 0, -2], [2, 0, -2], [2, 1, -1]]          # sums 5, 1, -5 over 3 points: thirds
            xyz[3:] += np.array([0, 0, 40])                             # keep the other rows away from those three voxels
        lab = rng.integers(0, 6, m)
        if b == 1:
            lab[:3] = 1                                                 # not a masked label
        coords.append(np.concatenate([np.full((m, 1), b), xyz], 1))
        ids.append(inst)
        labels.append(lab)
    return np.concatenate(coords).astype(np.int32), np.concatenate(ids).astype(np.int64), np.concatenate(labels).astype(np.int64)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["LGS_REFERENCE"]
    mod = load_reference(ref_root)
    coords, ids, labels = make_batch()
    out = {"coords": coords, "instance_ids": ids, "labels": labels, "masked_labels": np.asarray(MASKED, np.int64)}
    for b in range(len(SIZES)):
        rows = coords[:, 0] == b
        instances = ids[rows].copy()
        for ignore_id in MASKED:                                        # dataset.py:336-341
            instances[labels[rows] == ignore_id] = -1
        info = mod.VoxelizationDataset.get_instance_info(None, coords[rows, 1:], instances)
        occ = sorted(info["occupancy"])
        out["s%d_ids" % b] = np.asarray(info["ids"], np.int64)
        out["s%d_center" % b] = np.asarray(info["center"])
        assert out["s%d_center" % b].dtype == np.float32
        out["s%d_occ_id" % b] = np.asarray(occ, np.int64)
        out["s%d_occ_count" % b] = np.asarray([info["occupancy"][k] for k in occ], np.int64)
        out["s%d_bbox" % b] = np.asarray([info["bbox"][k] for k in occ], np.int64).reshape(-1, 6)
    assert 9 in out["s1_occ_id"] and out["s1_occ_count"][list(out["s1_occ_id"]).index(9)] == 3
    path = os.path.join(HERE, "insttarget.npz")
    np.savez_compressed(path, **out)
    print("%s: %d rows, %d bytes, instances per scene %s" % (path, len(coords), os.path.getsize(path),
                                                             [len(out["s%d_occ_id" % b]) for b in range(len(SIZES))]))


if __name__ == "__main__":
    main()
