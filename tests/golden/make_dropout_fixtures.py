"""Generates tests/golden/dropout_counts.npz by RUNNING THE REFERENCE'S OWN two RandomDropout classes (lib/transforms.py:172-195 and
downstream/insseg/datasets/transforms.py:145-159, loaded by file path) under fixed `random` / `numpy` seeds, for n = 0 .. 300 rows at
ratios 0.2, 0.3 and 0.5.  The fixture is data only: per case which class, the ratio, n, the seed, whether dropout was applied and
how many rows came back.

    python tests/golden/make_dropout_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

Per (class, ratio, n) the seeds 1000 n, 1000 n + 1, ... are tried in order until one case in which the transform applied and one in
which it did not have been recorded (it applies with probability `ratio`), so every n has both.  Arrays, one entry per case:
    which [c] int8 (0 = lib, 1 = insseg), ratio [c] float64, n [c] int32, seed [c] int64, applied [c] bool, returned [c] int32"""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_augment_fixtures import load_reference_transforms      # noqa: E402  (lib/transforms.py, with its imports stubbed)

RATIOS = (0.2, 0.3, 0.5)
MAX_N = 300


def load_insseg_transforms(ref_root):
    path = os.path.join(ref_root, "downstream", "insseg", "datasets", "transforms.py")
    spec = importlib.util.spec_from_file_location("reference_insseg_transforms", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(transform, n, with_instances):
    coords = np.arange(n * 3, dtype=np.float64).reshape(n, 3)
    feats, labels = np.arange(n * 3, dtype=np.float32).reshape(n, 3), np.arange(n)
    out = transform(coords, feats, labels, np.arange(n)) if with_instances else transform(coords, feats, labels)
    assert all(len(o) == len(out[0]) for o in out)
    rows = out[0][:, 0].astype(np.int64) // 3
    assert len(set(rows.tolist())) == len(rows)                 # without replacement
    applied = len(rows) != n or not np.array_equal(rows, np.arange(n))
    return applied, len(rows)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LGS_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    classes = (load_reference_transforms(ref).RandomDropout, load_insseg_transforms(ref).RandomDropout)
    cases = []
    for which, cls in enumerate(classes):
        for ratio in RATIOS:
            t = cls(ratio)
            for n in range(MAX_N + 1):
                seen = set()
                for seed in range(1000 * n, 1000 * n + 200):
                    random.seed(seed)
                    np.random.seed(seed)
                    state = random.getstate()
                    _, returned = run(t, n, which == 1)
                    random.setstate(state)
                    applied = random.random() < ratio         # the decision itself (n <= 1 at k == n cannot show it in the rows)
                    if applied not in seen:
                        seen.add(applied)
                        cases.append((which, ratio, n, seed, applied, returned))
                    if len(seen) == 2:
                        break
                assert len(seen) == 2, (which, ratio, n)
    c = list(zip(*cases))
    out = os.path.join(HERE, "dropout_counts.npz")
    np.savez_compressed(out, which=np.asarray(c[0], np.int8), ratio=np.asarray(c[1], np.float64), n=np.asarray(c[2], np.int32),
                        seed=np.asarray(c[3], np.int64), applied=np.asarray(c[4], bool), returned=np.asarray(c[5], np.int32))
    print(out, len(cases), "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
