"""Generates tests/golden/instshift.npz by RUNNING THE REFERENCE'S OWN ScannetVoxelizationDataset.augment_instances
(lib/datasets/scannet.py:243-319) as an unbound method on a stand-in object that carries label_map, inverse_label_map, ignore_mask,
frequency_organized_cats, the two probabilities and a real InstanceAugmentation(config) (lib/transforms.py:288-382).  The reference's
modules are imported from the checkout as make_paste_fixtures.py imports them.  random.random, random.sample and np.random.uniform
are wrapped to RECORD what they returned; the decisions are read back from those records.  The fixture is data only.

    python tests/golden/make_instshift_fixtures.py <checkout of the reference>      (or LGS_REFERENCE=<checkout>)

Two scenes (key prefix "s0_" / "s1_"):
    points [n, 3] float32, colors [n, 3] float32 (0 .. 255), labels [n] int64 (raw ids), ids [n] int64      what augment_instances received
    out_points [n, 3] float32, out_colors [n, 3] float32, out_labels [n, 2] int64                        what it returned
tail [t] the raw tail labels; p_color, p_scale; forced_keys [m, 3] (scene, label, id), forced_attr [m], forced_factor [m] float64:
one record per tail segment in the reference's order, attribute 0 for a segment that drew nothing, factor = the scale the reference
drew (1.0 where it drew none).  hue_in [h, 3] float32 and hue_out [4, h, 3] float32: InstanceAugmentation.shift_hue itself on a set
of colours, for Red, Green, Blue, Yellow in that order.
Between them the scenes hold every attribute 0 .. 8, an ignored label, a non-tail label that shares an id with a tail one, one id
under two tail labels, grey rows and rows with a 255 channel in every segment, and a one-point segment."""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_paste_fixtures import load_reference      # noqa: E402

TAIL = (5, 8, 14)
RAW = (0, 3, 5, 8, 11, 14, 20)          # 20 is ignored
IGNORE = 255
P_COLOR, P_SCALE = 0.5, 0.2
DIRECTIONS = ["Red", "Green", "Blue", "Yellow", "Dark", "Bright"]


class Recorder:
    def __init__(self):
        self.log = []                   # ("random", v) / ("sample", name) / ("uniform", v) in call order
        self._orig = (random.random, random.sample, np.random.uniform)

    def __enter__(self):
        o_random, o_sample, o_uniform = self._orig

        def rnd():
            v = o_random()
            self.log.append(("random", v))
            return v

        def sample(pop, k):
            v = o_sample(pop, k)
            self.log.append(("sample", v[0]))
            return v

        def uniform(low=0.0, high=1.0, size=None):
            v = o_uniform(low=low, high=high, size=size)
            self.log.append(("uniform", float(v)))
            return v
        random.random, random.sample, np.random.uniform = rnd, sample, uniform
        return self

    def __exit__(self, *exc):
        random.random, random.sample, np.random.uniform = self._orig


def make_scene(seed, n, size, origin):
    """background rows of every label, and per tail label a few box-shaped instances; instance ids are shared across labels"""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3)) * size + origin
    labels = rng.choice([0, 3, 11, 20], n).astype(np.int64)
    ids = rng.integers(0, 4, n).astype(np.int64)
    at = 0
    plan = [(5, 1, 260), (5, 2, 75), (5, 7, 1), (8, 1, 190), (8, 3, 64), (8, 9, 130), (14, 2, 333), (14, 4, 90), (14, 5, 47),
            (14, 6, 210), (5, 9, 31), (8, 4, 140), (5, 4, 66), (3, 1, 120), (3, 2, 80)]      # (3, *): not tail, ids shared with tail
    order = rng.permutation(n)
    for lab, inst, m in plan:
        rows = order[at:at + m]
        at += m
        centre = rng.random(3) * (np.asarray(size) - 0.8) + origin + 0.2
        pts[rows] = centre + rng.random((m, 3)) * (0.15 + rng.random(3) * 0.5)
        labels[rows], ids[rows] = lab, inst
    colors = np.floor(rng.random((n, 3)) * 256).clip(0, 255)
    grey = rng.random(n) < 0.08
    colors[grey] = colors[grey, :1]
    top = rng.random(n) < 0.12
    colors[top, rng.integers(0, 3, top.sum())] = 255
    white = rng.random(n) < 0.02
    colors[white] = 255
    return pts.astype(np.float32), colors.astype(np.float32), labels, ids


def run_scene(mod, tf_mod, scene, seed):
    import torch
    pts, colors, labels, ids = scene
    random.seed(seed)
    np.random.seed(seed)
    label_map = {r: i for i, r in enumerate(RAW[:-1])}
    label_map[RAW[-1]] = IGNORE
    inverse = {i: r for r, i in label_map.items() if i != IGNORE}
    inverse[IGNORE] = 0
    cats = torch.zeros(len(RAW) - 1, 3).bool()
    for r in RAW[:-1]:
        cats[label_map[r], 2 if r in TAIL else 0] = True
    config = types.SimpleNamespace(instance_augmentation="raw")
    this = types.SimpleNamespace(label_map=label_map, inverse_label_map=inverse, ignore_mask=IGNORE, frequency_organized_cats=cats,
                                 aug_color_prob=P_COLOR, aug_scale_prob=P_SCALE,
                                 instance_augmentation_transform=tf_mod.InstanceAugmentation(config))
    labels2 = np.hstack((labels[:, None], np.zeros_like(labels)[:, None]))
    with Recorder() as rec:
        out_p, out_c, out_l = mod.ScannetVoxelizationDataset.augment_instances(this, pts.copy(), colors.copy(), labels2, ids.copy())
    # the decisions, read back from the record in the reference's loop order: labels ascending, ids ascending
    log, at, decisions = rec.log, 0, []
    for lab in sorted(set(labels.tolist())):
        if lab not in TAIL:
            continue
        for inst in sorted(set(ids[labels == lab].tolist())):
            attr, factor = 0, 1.0
            kind, v = log[at]
            assert kind == "random"
            at += 1
            if v < P_COLOR:
                kind, name = log[at]
                assert kind == "sample"
                at += 1
                attr = 1 + DIRECTIONS.index(name)
            else:
                kind, v = log[at]
                assert kind == "random"
                at += 1
                if v < P_SCALE:
                    (k0, d), (k1, factor) = log[at], log[at + 1]
                    assert k0 == k1 == "uniform"
                    at += 2
                    attr = 7 if d > 1.0 else 8
            decisions.append((lab, inst, attr, factor))
    assert at == len(log)
    return dict(points=pts, colors=colors, labels=labels, ids=ids, out_points=np.asarray(out_p, np.float32),
                out_colors=np.asarray(out_c, np.float64).astype(np.float32), out_labels=np.asarray(out_l).astype(np.int64)), decisions, \
        (np.asarray(out_p).dtype, np.asarray(out_c, np.float64))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LGS_REFERENCE")
    if not ref_root:
        raise SystemExit(__doc__)
    mod, _ = load_reference(os.path.abspath(ref_root))
    import importlib
    tf_mod = importlib.import_module("lib.transforms")
    scenes = [make_scene(300, 3100, (4.2, 3.1, 2.3), (-2.1, -0.7, -0.2)), make_scene(301, 2300, (2.9, 2.2, 1.4), (0.3, -2.4, 0.1))]
    for seed in range(2000):
        got = [run_scene(mod, tf_mod, scenes[s], 10 * seed + s) for s in (0, 1)]
        attrs = {d[2] for g in got for d in g[1]}
        if attrs == set(range(9)):
            break
    else:
        raise RuntimeError("no seed found")
    assert {7, 8} <= attrs and set(range(1, 7)) <= attrs and 0 in attrs      # both scale directions, all six colour directions, none
    out = dict(tail=np.asarray(TAIL, np.int64), p_color=np.float64(P_COLOR), p_scale=np.float64(P_SCALE), seed=np.int64(seed))
    keys, fattr, ffac = [], [], []
    for s in (0, 1):
        fields, decisions, (p_dtype, c64) = got[s]
        assert p_dtype == np.float32 and np.array_equal(c64, fields["out_colors"].astype(np.float64))      # nothing lost in float32
        for k, v in fields.items():
            out["s%d_%s" % (s, k)] = v
        for lab, inst, attr, factor in decisions:
            keys.append((s, lab, inst))
            fattr.append(attr)
            ffac.append(factor)
        one = [d for d in decisions if ((fields["labels"] == d[0]) & (fields["ids"] == d[1])).sum() == 1]
        assert one, "no one-point segment"
    out.update(forced_keys=np.asarray(keys, np.int64), forced_attr=np.asarray(fattr, np.int64), forced_factor=np.asarray(ffac, np.float64))
    # shift_hue itself, on every kind of colour: random, grey, a 255 channel, white, black
    rng = np.random.default_rng(5)
    hue_in = np.floor(rng.random((600, 3)) * 256)
    hue_in[:80] = hue_in[:80, :1]
    hue_in[80:200, 0] = 255
    hue_in[200:260, 1] = 255
    hue_in[260:320, 2] = 255
    hue_in[320:330] = 255
    hue_in[330:340] = 0
    hue_in[340:360] = [255, 255, 0]
    hue_in = hue_in.astype(np.float32)
    t = tf_mod.InstanceAugmentation(types.SimpleNamespace())
    hues = [t.red_hue, t.green_hue, t.blue_hue, t.yellow_hue]
    out["hue_in"] = hue_in
    out["hue_out"] = np.stack([np.asarray(t.shift_hue(hue_in.copy(), h), np.float64) for h in hues]).astype(np.float32)
    path = os.path.join(HERE, "instshift.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; seed", seed)
    for k, v in out.items():
        print("  %-18s %s %s" % (k, v.dtype, v.shape))
    print("decisions", sorted(zip(fattr, ffac)))


if __name__ == "__main__":
    main()
