"""The device instance shifts (languagegroundedsemseg_amd/augment.py instance_shifts, csrc/lgs_instshift.hip) against the reference's
recorded outputs (tests/golden/instshift.npz) and the numpy restatement of the contract (tests/instshift_reference.py), bit for bit:
everything compared is integer or pinned-order fp32 / fp64.  Shapes are the smallest that reach each branch: a fold workgroup takes
2048 consecutive rows (scenes may share one), its LDS table holds 512 segments, a workgroup is 256 threads, a wave 64 lanes."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import dropout_reference as dr
import instshift_reference as ir
from languagegroundedsemseg_amd import augment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 2048
TAIL = [5, 8, 14, (1 << 33) + 7]      # a label beyond 32 bits: both halves are in the counter
OTHER = [0, 3, 11, 20]
# wave, workgroup and tile boundaries; empty scenes first, in the middle and last; several tiles plus a row
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 0, 3 * TILE + 1, 5, 1000, 2 * TILE + 1, 0, 3, 127, 129, 511, 513, 1023,
         31, 33, 7, 300, TILE, 900, 2, 1, 0]
NO_TAIL, ONLY_TAIL, SPAN, MANY, BAD_IDS = 14, 20, 12, 27, 28      # scenes with a special content, see make_batch
SEED = (0x5eed << 32) | 0x89abcdef
SEEDS = [(s * 2654435761 + 99) % (1 << 32) for s in range(32)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_batch():
    assert len(SIZES) == 32
    rng = np.random.default_rng(21)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(off[-1])
    pts = (rng.random((n, 3)) * [4.0, 3.0, 2.5] - [1.5, 0.5, 0.2]).astype(np.float32)
    cols = np.floor(rng.random((n, 3)) * 256).clip(0, 255)
    grey = rng.random(n) < 0.1
    cols[grey] = cols[grey, :1]
    top = rng.random(n) < 0.15
    cols[top, rng.integers(0, 3, int(top.sum()))] = 255
    cols[rng.random(n) < 0.03] = 255
    labels = rng.choice(TAIL + OTHER, n).astype(np.int64)
    ids = rng.integers(0, 6, n).astype(np.int64)                      # the same ids in every scene and under every label
    at = lambda s: slice(off[s], off[s + 1])
    labels[at(NO_TAIL)] = rng.choice(OTHER, SIZES[NO_TAIL])          # a scene with no tail row
    labels[at(ONLY_TAIL)] = rng.choice(TAIL, SIZES[ONLY_TAIL])       # one with only tail rows
    a = off[SPAN]                                                     # a segment that spans the scene's four tiles: every third row
    labels[a:off[SPAN + 1]:3], ids[a:off[SPAN + 1]:3] = 8, 77
    labels[at(MANY)] = rng.choice(TAIL, SIZES[MANY])                  # ~1400 distinct segments in 2048 rows: more in either of the
    ids[at(MANY)] = rng.integers(0, 600, SIZES[MANY])                 # workgroups that share the scene than an LDS table holds
    ids[at(BAD_IDS)] = rng.choice([-1, -5, 1 << 31, 1 << 40, 2, (1 << 31) - 1], SIZES[BAD_IDS])      # -1 and out of range
    return pts, cols.astype(np.float32), labels, ids, off


@pytest.fixture(scope="module")
def batch():
    return make_batch()


@pytest.fixture(scope="module")
def reference(batch):
    """the restatement on the batch, computed once: (outputs, decisions)"""
    pts, cols, labels, ids, off = batch
    decisions = []
    out = ir.instance_shifts(pts, cols, labels, ids, off, TAIL, 0.5, 0.3, seed=SEED, scene_seeds=SEEDS, decisions=decisions)
    return out, decisions


def run(batch, **kw):
    pts, cols, labels, ids, off = batch
    kw.setdefault("seed", SEED)
    kw.setdefault("scene_seeds", SEEDS[:len(off) - 1])
    out = augment.instance_shifts(dev(pts), dev(cols), dev(labels), dev(ids), [int(v) for v in off], kw.pop("tail", TAIL),
                                  kw.pop("p_color", 0.5), kw.pop("p_scale", 0.3), **kw)
    assert out[2].dtype == torch.int64 and out[4].dtype == torch.int64 and out[5].dtype == torch.int32 and out[5].shape == (2,)
    return [t.cpu().numpy() for t in out]


def assert_equal(got, want, what=""):
    for g, w, name in zip(got[:5], want[:5], ("points", "colors", "labels2", "instances", "order")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, int((g != w).sum()))
    assert [int(v) & 0xffffffff for v in got[5]] == list(want[5]), (what, "status")


# ---- 1. the reference's own outputs, teacher-forced
def test_fixture_played_back_equals_the_reference_outputs_exactly():
    fx = dict(np.load(os.path.join(HERE, "golden", "instshift.npz")))
    cat = lambda k: np.concatenate([fx["s0_" + k], fx["s1_" + k]])
    off = [0, len(fx["s0_points"]), len(fx["s0_points"]) + len(fx["s1_points"])]
    forced = (fx["forced_keys"], fx["forced_attr"], fx["forced_factor"])
    got = run((cat("points"), cat("colors"), cat("labels"), cat("ids"), off), tail=fx["tail"], forced=forced, p_color=0.0, p_scale=0.0)
    for s in (0, 1):
        at = slice(off[s], off[s + 1])
        assert np.array_equal(got[0][at], fx["s%d_out_points" % s])
        assert np.array_equal(got[1][at], fx["s%d_out_colors" % s])
        assert np.array_equal(got[2][at], fx["s%d_out_labels" % s])
    assert np.array_equal(got[3], cat("ids")[got[4]]) and got[5].tolist() == [0, 0]
    assert set(got[2][:, 1].tolist()) == set(range(9))
    want = ir.instance_shifts(cat("points"), cat("colors"), cat("labels"), cat("ids"), off, fx["tail"], forced=forced)
    assert_equal(got, want, "fixture")                                # the row order itself, too


# ---- 2. the generator path
def test_generator_path_equals_the_restatement_exactly(batch, reference):
    want, decisions = reference
    attrs = [d[3] for d in decisions]
    assert set(attrs) == set(range(9)) and len(decisions) > 1200      # every decision occurs; more segments than MANY's LDS table holds
    pts, cols, labels, ids, off = batch
    rows = slice(off[MANY], (off[MANY] // TILE + 1) * TILE)           # the rows of MANY in the first fold workgroup that holds some
    assert rows.stop < off[MANY + 1] and len(set(zip(labels[rows].tolist(), ids[rows].tolist()))) > 2 * 512
    assert want[5] == [0, 1 << BAD_IDS]                               # the out-of-range ids are reported, -1 is not
    got = run(batch)
    assert_equal(got, want, "generator")
    again = run(batch)                                                # a second call gives the same bits
    for g, a in zip(got, again):
        assert g.tobytes() == a.tobytes()
    order = got[4]
    assert np.array_equal(order[off[NO_TAIL]:off[NO_TAIL + 1]], np.arange(off[NO_TAIL], off[NO_TAIL + 1]))      # no tail row: the identity
    span = [d for d in decisions if d[0] == SPAN and d[1] == 8 and d[2] == 77]
    assert len(span) == 1 and (np.diff(order[off[SPAN + 1] - 10:off[SPAN + 1]]) > 0).all()


def test_a_scene_alone_gives_the_rows_it_gets_inside_the_batch(batch, reference):
    pts, cols, labels, ids, off = batch
    want, _ = reference
    for s in (SPAN, MANY, 9):
        at = slice(off[s], off[s + 1])
        alone = run((pts[at], cols[at], labels[at], ids[at], [0, SIZES[s]]), scene_seeds=[SEEDS[s]])
        for k in range(4):
            assert np.array_equal(alone[k], want[k][at]), (s, k)
        assert np.array_equal(alone[4] + off[s], want[4][at]), s
    # elsewhere in a batch, behind an empty scene and a short one
    at = slice(off[MANY], off[MANY + 1])
    lead = 5
    cat = lambda a, fill: np.concatenate([np.full((lead,) + a.shape[1:], fill, a.dtype), a[at]])
    moved = run((cat(pts, 1.0), cat(cols, 9.0), cat(labels, 3), cat(ids, 0), [0, 0, lead, lead + SIZES[MANY]]),
                scene_seeds=[1, 2, SEEDS[MANY]])
    for k in range(4):
        assert np.array_equal(moved[k][lead:], want[k][at]), k
    assert np.array_equal(moved[4][lead:] - lead + off[MANY], want[4][at])


def test_the_hue_shifts_as_intended(batch):
    pts, cols, labels, ids, off = batch
    want = ir.instance_shifts(pts, cols, labels, ids, off, TAIL, 0.9, 0.3, seed=SEED, scene_seeds=SEEDS, hue_as_written=False)
    got = run(batch, p_color=0.9, hue_as_written=False)
    assert_equal(got, want, "intent")
    hued = (got[2][:, 1] >= 1) & (got[2][:, 1] <= 4)
    assert hued.sum() > 1000 and len(np.unique(got[1][hued])) > 100   # not the 0 / 255 of the reference's cast


def test_more_segments_than_seg_cap(batch, reference):
    """documented outcome: a scene that holds a segment of rank >= seg_cap stays exactly as it was, bit `scene` of status[0]; with more
    segments than the table has entries every scene does"""
    pts, cols, labels, ids, off = batch
    full = reference[0]
    n_seg = len(reference[1])
    for cap in (1500, 300):
        want = ir.instance_shifts(pts, cols, labels, ids, off, TAIL, 0.5, 0.3, seed=SEED, scene_seeds=SEEDS, seg_cap=cap)
        got = run(batch, seg_cap=cap)
        assert_equal(got, want, "seg_cap %d" % cap)
        first_bad = min(s for s in range(32) if (want[5][0] >> s) & 1)
        if n_seg <= ir.table_size(cap):                               # the scenes in front of the first overflowing one are shifted as ever
            assert 0 < first_bad and np.array_equal(got[4][:off[first_bad]], full[4][:off[first_bad]])
            assert np.array_equal(got[4][off[first_bad]:], np.arange(off[first_bad], off[-1]))
            assert augment.instance_shift_status(dev(np.asarray(got[5]))) == {
                "unshifted": [s for s in range(32) if (want[5][0] >> s) & 1], "id_range": [BAD_IDS]}
        else:
            assert want[5][0] == (1 << 32) - 1 and np.array_equal(got[4], np.arange(off[-1])) and (got[2][:, 1] == 0).all()
    assert n_seg > ir.table_size(300) and 1500 < n_seg <= ir.table_size(1500)       # both outcomes were met


def test_row_order_on_a_large_batch():
    """2^21 + 3 rows in three scenes: the sort's large-input path.  An empty forced table: every segment moves, nothing shifts."""
    rng = np.random.default_rng(4)
    sizes = [(1 << 20) + 1, 2, (1 << 20)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    labels = rng.choice(TAIL[:3] + OTHER, n).astype(np.int64)
    ids = rng.integers(0, 12, n).astype(np.int64)
    pts = rng.random((n, 3)).astype(np.float32)
    empty = (np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros(0))
    got = run((pts, pts * 255, labels, ids, off), forced=empty, scene_seeds=[0, 0, 0])
    scene = np.searchsorted(off, np.arange(n), side="right") - 1
    group = np.where(np.isin(labels, TAIL[:3]), 1 + labels * 16 + ids, 0)      # 0: stays; then ascending by (label, id)
    want = np.lexsort((np.arange(n), group, scene))
    assert np.array_equal(got[4], want) and np.array_equal(got[0], pts[want]) and (got[2][:, 1] == 0).all()
    assert np.array_equal(got[2][:, 0], labels[want]) and np.array_equal(got[3], ids[want]) and got[5].tolist() == [0, 0]


def test_workspace_size_and_nothing_synchronises():
    from languagegroundedsemseg_amd import engine
    W = engine.lib().lgs_instance_shift_workspace_bytes
    small, big = W(0, 1, 1), W(1 << 20, 32, 4096)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0 and big >= 16 * (1 << 20)      # four 4-byte words per row
    pts, cols, labels, ids, off = make_batch()
    args = (dev(pts), dev(cols), dev(labels), dev(ids), dev(off))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = augment.instance_shifts(*args, TAIL, 0.5, 0.3, seed=SEED, scene_seeds=SEEDS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out[4].shape == (off[-1],)


# ---- 3. the chain
def chain_inputs():
    """the fixture's two scenes, and a third in which six tail instances of ten rows each are followed by copies of their rows under a
    label that is not tail: in every voxel of those the tail row comes first in the input"""
    fx = dict(np.load(os.path.join(HERE, "golden", "instshift.npz")))
    rng = np.random.default_rng(9)
    p3 = (rng.random((60, 3)) * 2 + 0.3).astype(np.float32)
    c3 = np.floor(rng.random((120, 3)) * 256).astype(np.float32)
    l3 = np.concatenate([np.repeat([5, 5, 8, 8, 14, 14], 10), np.full(60, 3)]).astype(np.int64)
    i3 = np.concatenate([np.repeat([1, 2, 1, 2, 3, 4], 10), np.full(60, 9)]).astype(np.int64)
    cat = lambda k, third: np.concatenate([fx["s0_" + k], fx["s1_" + k], third])
    pts, cols, labels, ids = cat("points", np.concatenate([p3, p3])), cat("colors", c3), cat("labels", l3), cat("ids", i3)
    n0, n1 = len(fx["s0_points"]), len(fx["s1_points"])
    return pts, cols, labels, ids, [0, n0, n0 + n1, n0 + n1 + 120], [int(v) for v in fx["tail"]]


def chain(**kw):
    return augment.DeviceAugmentation(voxel_size=0.05, rotation_bound=((-0.05, 0.05), (-0.05, 0.05), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
                                      normalize_color=True, seed=2, **kw)


def forced_plan(aug, dropout=None):
    plan = aug.draw(3)
    plan.elastic[:] = True
    plan.flip_axes[:] = [1, 2, 0]
    plan.autocontrast[:], plan.translate[:], plan.jitter[:] = True, True, False
    plan.dropout = None if dropout is None else np.asarray(dropout, bool)
    return plan


@pytest.fixture(scope="module")
def chained():
    """the chain with the stage, once: (inputs, plan, outputs)"""
    pts, cols, labels, ids, off, tail = chain_inputs()
    aug = chain(instance_shifts=augment.InstanceShifts(tail, 0.5, 0.2))
    plan = forced_plan(aug)
    out = aug(dev(pts), dev(cols), dev(labels), off, plan=plan, instances=dev(ids), return_state=True)      # (the stage runs inside the
    return (pts, cols, labels, ids, off, tail), plan, out                                                     # chain's "error" sync region)


def test_chain_equals_the_restatement_composed_with_the_other_stages(chained):
    (pts, cols, labels, ids, off, tail), plan, (coords, feats, lab2, inst, state) = chained
    before = state["stages"][-1].cpu().numpy()                        # the cloud the stage received: after the elastic stages
    want = ir.instance_shifts(before, cols, labels, ids, off, tail, 0.5, 0.2, seed=plan.seed, scene_seeds=plan.scene_seeds)
    assert np.array_equal(state["instance_shift_order"].cpu().numpy(), want[4])
    assert np.array_equal(state["points"].cpu().numpy(), want[0]) and state["instance_shift_status"].tolist() == [0, 0]
    assert len(set(want[2][:, 1].tolist())) >= 4 and (want[2][:, 1] >= 7).any()      # several kinds of decision occurred, a scale shift too
    # the rest of the chain on the restatement's rows: the chain without the stage and without elastic, same plan
    rest = chain(elastic_params=None)(dev(want[0]), dev(want[1]), dev(want[2][:, 0]), off, plan=plan, instances=dev(want[3]), return_state=True)
    keep = rest[4]["keep"].cpu().numpy()
    assert np.array_equal(state["keep"].cpu().numpy(), keep)
    assert torch.equal(coords, rest[0]) and torch.equal(feats, rest[1]) and torch.equal(inst, rest[3])
    assert lab2.shape == (len(keep), 2) and lab2.dtype == torch.int64
    assert np.array_equal(lab2.cpu().numpy(), want[2][keep]) and torch.equal(lab2[:, 0], rest[2])      # [n, 2]; the ids ride along
    assert np.array_equal(inst.cpu().numpy(), ids[want[4]][keep])
    # the dedup's winner in a voxel that a stay row and a moved row share is the stay row, although the moved row came first in the input
    vox = augment.voxelize_batched(dev(want[0]), off, plan.matrices).cpu().numpy()
    moved = np.isin(want[2][:, 0], tail) & (want[3] >= 0)
    keys = {}
    for j in range(off[2], off[3]):
        keys.setdefault(tuple(vox[j]), []).append(j)
    shared = [rows for rows in keys.values() if moved[rows].any() and not moved[rows].all()]
    assert len(shared) >= 10
    kept = set(keep.tolist())
    for rows in shared:
        winner = [j for j in rows if j in kept]
        assert len(winner) == 1 and not moved[winner[0]] and want[2][winner[0], 0] == 3
        assert min(want[4][j] for j in rows if moved[j]) < want[4][winner[0]]      # in the input the moved row was ahead


@pytest.mark.parametrize("position", ["first", "last"])
def test_chain_with_dropout_in_both_positions(chained, position):
    (pts, cols, labels, ids, off, tail), plan, base = chained
    aug = chain(instance_shifts=augment.InstanceShifts(tail, 0.5, 0.2), dropout=0.2, dropout_position=position)
    plan = dataclasses.replace(plan, dropout=np.array([True, False, True]))
    if position == "first":           # flip and autocontrast would see the surviving rows only: without them the position does not show
        plan = dataclasses.replace(plan, flip_axes=np.zeros(3, np.int64), autocontrast=np.zeros(3, bool))
        base = chain(instance_shifts=augment.InstanceShifts(tail, 0.5, 0.2))(dev(pts), dev(cols), dev(labels), off, plan=plan,
                                                                             instances=dev(ids), return_state=True)
    got = aug(dev(pts), dev(cols), dev(labels), off, plan=plan, instances=dev(ids), return_state=True)
    keep0 = base[4]["keep"].cpu().numpy()
    sel, _ = dr.select(np.searchsorted(keep0, off).astype(np.int64), [True, False, True], 0.2, seed=plan.seed, scene_seeds=plan.scene_seeds)
    assert 0 < len(sel) < len(keep0)
    if position == "first":
        assert np.array_equal(got[4]["keep"].cpu().numpy(), keep0[sel])
    else:
        assert np.array_equal(got[4]["dropout_rows"].cpu().numpy(), sel)
    for g, w in zip(got[:4], base[:4]):                               # coordinates, colours, [n, 2] labels, instances
        assert torch.equal(g, w[dev(sel)])
    assert got[2].shape[1] == 2
