"""Independent numpy restatement of the device RandomDropout's contract (include/lgs_engine.h, csrc/lgs_dropout.hip).  Shares no code
with the product; tests/test_dropout_cpu.py holds its count rule to the reference's recorded counts (tests/golden/dropout_counts.npz)
and checks the rule's uniformity, tests/test_gpu_dropout.py holds the kernels to it bit for bit.

Scene s with n_s rows and its apply bit set keeps k_s = int(n_s * (1 - ratio)) rows: those smallest under (key as uint32, row), in
ascending row order.  Row i's key is word 0 of Philox-4x32-10 with counter (i & 2^32-1, i >> 32, 0, 18 ^ (seed >> 32)) and key
(seed & 2^32-1, scene seed)."""
import numpy as np

from augment_reference import philox4x32_10

STAGE_DROPOUT = 18


def keep_count(n, ratio):
    """the reference's int(N * (1 - self.dropout_ratio)), Python doubles"""
    return int(n * (1 - ratio))


def row_keys(n, seed, scene_seed):
    i = np.arange(n, dtype=np.uint64)
    hi = np.full(n, STAGE_DROPOUT ^ ((seed >> 32) & 0xffffffff), np.uint64)
    ctr = np.stack([i & np.uint64(0xffffffff), i >> np.uint64(32), np.zeros(n, np.uint64), hi], 1)
    return philox4x32_10(ctr, seed & 0xffffffff, int(scene_seed) & 0xffffffff)[:, 0] if n else np.zeros(0, np.uint32)


def select_scene(keys, k):
    """rows of the k smallest (key, row), ascending.  keys: uint32-valued"""
    keys = np.asarray(keys).astype(np.uint32).astype(np.int64)
    order = np.lexsort((np.arange(len(keys)), keys))          # by key, then by row
    return np.sort(order[:k]).astype(np.int64)


def select(offsets, apply, ratio, seed=0, scene_seeds=None, keys=None, through=None):
    """-> (rows int64 [m], offsets_out: B + 1 integers).  keys: int32 / uint32 [n] per batch row in place of the generator"""
    offsets = [int(v) for v in offsets]
    b = len(offsets) - 1
    scene_seeds = [0] * b if scene_seeds is None else scene_seeds
    rows, out = [], [0]
    for s in range(b):
        lo, hi = offsets[s], offsets[s + 1]
        n = hi - lo
        if apply[s]:
            k = np.asarray(keys)[lo:hi].astype(np.int64) & 0xffffffff if keys is not None else row_keys(n, seed, scene_seeds[s])
            kept = select_scene(k, keep_count(n, ratio)) + lo
        else:
            kept = np.arange(lo, hi, dtype=np.int64)
        rows.append(kept)
        out.append(out[-1] + len(kept))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if through is not None:
        rows = np.asarray(through, np.int64)[rows]
    return rows.astype(np.int64), out
