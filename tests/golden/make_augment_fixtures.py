"""Generates tests/golden/augment.npz by RUNNING THE REFERENCE'S OWN transforms (lib/transforms.py, loaded by file path with open3d and
matplotlib stubbed and scipy.ndimage.filters aliased where the installed scipy lacks it): ElasticDistortion, RandomHorizontalFlip,
ChromaticAutoContrast, ChromaticTranslation, ChromaticJitter.  np.random.randn / np.random.rand / random.random are wrapped to RECORD
what they returned.  The fixture is data only: inputs, the recorded draws, the reference's output after each transform.

    python tests/golden/make_augment_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

Two scenes (key prefix "s0_" / "s1_"); s1 is 0.5 m tall, less than the 0.8 granularity, so noise_dim is 3 along z in stage 2:
    points [n, 3] float32, colors [n, 3] float32 in [0, 255], labels [n] int64
    e1_noise / e2_noise   the randn block of each elastic stage, float32 [dx, dy, dz, 3] (the reference casts it to float32 itself)
    e1_out / e2_out       the points after stage 1 (0.2, 0.4) and stage 2 (0.8, 1.6), float32
    vox                   floor(e2_out / 0.05), float64 [n, 3]: the coordinates the flip receives
    flip_draws            what random.random() returned inside RandomHorizontalFlip('z');  flip_out  its coordinates
    auto_draws, auto_out  ChromaticAutoContrast (the seed is chosen so that it applies);  feats chain on: auto -> trans -> jitter
    trans_draws, trans_rand [1, 3], trans_out      ChromaticTranslation(0.1)
    jitter_draws, jitter_randn [n, 3], jitter_out  ChromaticJitter(0.05)
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def load_reference_transforms(ref_root):
    for name in ("open3d", "matplotlib"):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    import scipy.ndimage
    if not hasattr(scipy.ndimage, "filters"):
        scipy.ndimage.filters = scipy.ndimage
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)            # the repository's MinkowskiEngine package stands in for the import at the top
    spec = importlib.util.spec_from_file_location("reference_transforms", os.path.join(ref_root, "lib", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """wraps np.random.randn / np.random.rand / random.random; everything they return is kept in call order"""

    def __init__(self):
        self.randn, self.rand, self.random = [], [], []
        self._orig = (np.random.randn, np.random.rand, random.random)

    def __enter__(self):
        o_randn, o_rand, o_random = self._orig

        def randn(*a):
            v = o_randn(*a)
            self.randn.append(np.array(v))
            return v

        def rand(*a):
            v = o_rand(*a)
            self.rand.append(np.array(v))
            return v

        def rnd():
            v = o_random()
            self.random.append(v)
            return v
        np.random.randn, np.random.rand, random.random = randn, rand, rnd
        return self

    def __exit__(self, *exc):
        np.random.randn, np.random.rand, random.random = self._orig


def scene(seed, n, size):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * np.asarray(size) + np.asarray([-1.3, 0.7, -0.2])).astype(np.float32)
    colors = np.floor(rng.random((n, 3)) * np.asarray([200.0, 256.0, 120.0]) + np.asarray([30.0, 0.0, 90.0])).clip(0, 255).astype(np.float32)
    labels = rng.integers(0, 20, n).astype(np.int64)
    return pts, colors, labels


def run_until(make, applies, first_seed):
    """runs make(seed) with increasing seeds until the transform applied (its first random.random() draw decided that)"""
    for seed in range(first_seed, first_seed + 1000):
        random.seed(seed)
        np.random.seed(seed)
        with Recorder() as rec:
            out = make()
        if applies(rec):
            return out, rec
    raise RuntimeError("no seed found")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LGS_REFERENCE")
    if not ref_root:
        raise SystemExit(__doc__)
    t = load_reference_transforms(ref_root)
    out = {}
    for s, (n, size) in enumerate([(3000, (4.1, 3.3, 2.4)), (2000, (2.7, 1.9, 0.5))]):
        pre = "s%d_" % s
        pts, colors, labels = scene(100 + s, n, size)
        out[pre + "points"], out[pre + "colors"], out[pre + "labels"] = pts, colors, labels
        # elastic: the two stages one at a time, so that the cloud between them is recorded
        cur = pts.copy()
        for stage, (g, m) in enumerate(((0.2, 0.4), (0.8, 1.6)), 1):
            ed = t.ElasticDistortion(((g, m),))
            (cur, _, _), rec = run_until(lambda: ed(cur.copy(), colors, labels), lambda r: len(r.randn) == 1, 10 * s + stage)
            assert cur.dtype == np.float32
            out[pre + "e%d_noise" % stage] = rec.randn[0].astype(np.float32)
            out[pre + "e%d_out" % stage] = cur.copy()
        vox = np.floor(cur.astype(np.float64) / 0.05)
        out[pre + "vox"] = vox
        flip = t.RandomHorizontalFlip("z", False)
        (fc, _, _), rec = run_until(lambda: flip(vox.copy(), colors, labels), lambda r: r.random[0] < 0.95 and min(r.random[1:]) < 0.5, 40 + s)
        out[pre + "flip_draws"], out[pre + "flip_out"] = np.asarray(rec.random), fc
        feats = colors.copy()
        (_, feats, _), rec = run_until(lambda: t.ChromaticAutoContrast()(vox, feats.copy(), labels), lambda r: r.random[0] < 0.2, 50 + s)
        out[pre + "auto_draws"], out[pre + "auto_out"] = np.asarray(rec.random), feats.copy()
        (_, feats, _), rec = run_until(lambda: t.ChromaticTranslation(0.1)(vox, feats.copy(), labels), lambda r: r.random[0] < 0.95, 60 + s)
        out[pre + "trans_draws"], out[pre + "trans_rand"], out[pre + "trans_out"] = np.asarray(rec.random), rec.rand[0], feats.copy()
        (_, feats, _), rec = run_until(lambda: t.ChromaticJitter(0.05)(vox, feats.copy(), labels), lambda r: r.random[0] < 0.95, 70 + s)
        # (the reference scales its noise array in place afterwards: the recorder kept a copy of what randn returned)
        out[pre + "jitter_draws"], out[pre + "jitter_randn"], out[pre + "jitter_out"] = np.asarray(rec.random), rec.randn[0], feats.copy()
        assert feats.dtype == np.float32
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        print("  %-16s %s %s" % (k, v.dtype, v.shape))


if __name__ == "__main__":
    main()
