"""Instance targets on the device (csrc/lgs_insttarget.hip, languagegroundedsemseg_amd/instances.py, losses.fused_instance_offset_losses)
against the fixture the reference's own get_instance_info wrote (tests/golden/insttarget.npz) and the float64 numpy restatement
(tests/insttarget_reference.py).  Tables and centres are compared exactly; the losses and their gradient within bounds that come from
the arithmetic: a row costs about a dozen fp32 roundings at 6e-8 each, the sums are fp64, and the bounds keep an eight-fold margin."""
import functools
import os

import numpy as np
import pytest
import torch

import insttarget_reference as ir
from languagegroundedsemseg_amd import augment, engine, instances
from languagegroundedsemseg_amd.hipcall import ptr, raw_stream, scratch
from languagegroundedsemseg_amd.losses import fused_instance_offset_losses, instance_offset_losses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOXEL = 0.02
VOXEL_W = float(np.float32(VOXEL))             # the voxel size as the kernels see it (a C float), widened: the restatement takes this one


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- cases (built once, shared, never modified)
def _scenes(sizes, seed, n_ids=6, lo=-40, hi=40, p_none=0.15):
    rng = np.random.default_rng(seed)
    coords = np.concatenate([np.concatenate([np.full((m, 1), b), rng.integers(lo, hi, (m, 3))], 1) for b, m in enumerate(sizes)]).astype(np.int32)
    ids = rng.integers(0, n_ids, len(coords)).astype(np.int64)
    ids[rng.random(len(coords)) < p_none] = -1
    return coords, ids


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (coords int32 [n, 4], ids int64 [n], labels or None, masked labels)"""
    if name == "empty":
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int64), None, ()
    if name == "one":
        return np.array([[2, -7, 5, 11]], np.int32), np.array([4], np.int64), None, ()
    if name == "three_scenes_257":                       # the same ids 0 .. 5 in each of three scenes, -1 rows, negative coordinates
        return _scenes((100, 57, 100), 1) + (None, ())
    if name == "masked":
        coords, ids = _scenes((130, 127), 2)
        labels = np.random.default_rng(3).integers(0, 5, len(ids)).astype(np.int64)
        return coords, ids, labels, (1, 3)
    if name == "thirds":                                 # an instance of 3 points whose mean is not representable
        return (np.array([[0, 1, 0, -2], [0, 2, 0, -2], [0, 2, 1, -1], [0, 9, 9, 9]], np.int32), np.array([7, 7, 7, -1], np.int64), None, ())
    if name == "contention":                             # one instance owns 90 % of 20 000 rows, 299 small ones share the rest
        rng = np.random.default_rng(4)
        coords = np.concatenate([np.zeros((20000, 1)), rng.integers(-300, 300, (20000, 3))], 1).astype(np.int32)
        ids = np.where(rng.random(20000) < 0.9, 0, rng.integers(1, 300, 20000)).astype(np.int64)
        ids[np.arange(1, 300)] = np.arange(1, 300)       # every small one is there
        return coords, ids, None, ()
    if name == "far":                                    # coordinates near +-130 000, two scenes
        rng = np.random.default_rng(5)
        sign = np.where(rng.random((4000, 1)) < 0.5, -1, 1)
        coords = np.concatenate([rng.integers(0, 2, (4000, 1)), sign * rng.integers(129000, 130001, (4000, 3))], 1).astype(np.int32)
        return coords, rng.integers(-1, 5, 4000).astype(np.int64), None, ()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    coords, ids, labels, masked = case(name)
    mids = ir.mask_ids(ids, labels, masked)
    return (mids,) + ir.batch_instance_info(coords, mids)


def run(name, inst_cap=4096, **kw):
    coords, ids, labels, masked = case(name)
    return instances.instance_info(dev(coords), dev(ids), None if labels is None else dev(labels), masked, inst_cap=inst_cap, **kw)


def assert_table_equals(info, want, inst_cap):
    mids, keys, count, bbox, center, row, centers = want
    assert int(info.status.cpu()[0]) == 0
    assert np.array_equal(info.ids.cpu().numpy(), mids)
    got_key, got_count = info.key.cpu().numpy(), info.count.cpu().numpy()
    used = np.flatnonzero(got_key >= 0)
    assert len(used) == len(keys) and (got_count[got_key < 0] == 0).all() and got_key.shape == (inst_cap,)
    order = used[np.argsort(got_key[used])]
    assert np.array_equal(got_key[order], keys)
    assert np.array_equal(got_count[order], count)
    assert np.array_equal(info.bbox.cpu().numpy()[order], bbox)
    assert np.array_equal(info.center_table.cpu().numpy()[order].view(np.int32), center.view(np.int32))          # bit-equal
    slot = info.slot.cpu().numpy()
    assert np.array_equal(slot >= 0, row >= 0)
    assert np.array_equal(got_key[slot[slot >= 0]], keys[row[row >= 0]])
    if info.center is not None:
        assert np.array_equal(info.center.cpu().numpy().view(np.int32), centers.view(np.int32))


# ---- table and centres
@pytest.mark.parity("tests/insttarget_reference.py (numpy restatement of get_instance_info)")
@pytest.mark.parametrize("name", ["empty", "one", "three_scenes_257", "masked", "thirds", "contention", "far"])
def test_table_and_centres_equal_the_restatement_exactly(name):
    info = run(name)
    assert_table_equals(info, expected(name), 4096)
    info.check()
    if name == "three_scenes_257":
        assert len({int(k) >> 32 for k in expected(name)[1]}) == 3 and len({int(k) & 0xffffffff for k in expected(name)[1]}) == 6
    if name == "contention":
        assert expected(name)[2].max() > 17000 and len(expected(name)[1]) == 300
    if name == "thirds":
        assert np.array_equal(info.center.cpu().numpy()[0], np.array([5 / 3, 1 / 3, -5 / 3]).astype(np.float32))


@pytest.mark.parity("tests/golden/insttarget.npz (the reference's own get_instance_info)")
def test_table_and_centres_equal_the_recorded_reference():
    fx = np.load(os.path.join(G, "insttarget.npz"))
    masked = [int(v) for v in fx["masked_labels"]]
    info = instances.instance_info(dev(fx["coords"]), dev(fx["instance_ids"]), dev(fx["labels"]), masked, inst_cap=64).check()
    for b in range(3):
        ref = info.to_reference(b)
        assert np.array_equal(ref["ids"], fx["s%d_ids" % b])
        assert ref["center"].dtype == np.float32 and np.array_equal(ref["center"].view(np.int32), fx["s%d_center" % b].view(np.int32))
        assert sorted(ref["occupancy"]) == list(fx["s%d_occ_id" % b])
        assert [ref["occupancy"][k] for k in sorted(ref["occupancy"])] == list(fx["s%d_occ_count" % b])
        assert np.array_equal(np.array([ref["bbox"][k] for k in sorted(ref["bbox"])]), fx["s%d_bbox" % b])
    rows = dev(fx["coords"])[:, 0] == 1
    assert np.array_equal(info.center[rows].cpu().numpy().view(np.int32), fx["s1_center"].view(np.int32))
    # without the per-point array the table is the same
    lean = instances.instance_info(dev(fx["coords"]), dev(fx["instance_ids"]), dev(fx["labels"]), masked, inst_cap=64, return_centers=False)
    assert lean.center is None and torch.equal(lean.center_table, info.center_table) and torch.equal(lean.slot, info.slot)


def test_ids_outside_the_range_set_their_status_bit_and_count_as_none():
    coords = dev(np.array([[0, 1, 1, 1], [0, 2, 2, 2], [0, 3, 3, 3], [-1, 4, 4, 4]], np.int32))
    info = instances.instance_info(coords, dev(np.array([5, -2, 1 << 31, 5], np.int64)), inst_cap=8)
    assert int(info.status.cpu()[0]) == 2 | 4
    assert info.ids.cpu().tolist() == [5, -1, -1, -1] and info.count.cpu().sum().item() == 1
    with pytest.raises(RuntimeError, match="outside \\[0, 2\\^31\\).*negative batch index"):
        info.check()


# ---- capacity
GUARD = 64


def raw_instance_info(coords, ids, inst_cap):
    """the C-ABI directly, every output followed by a guard band of GUARD elements -> {name: (tensor, elements in use)}"""
    n = coords.shape[0]
    spec = {"ids_out": (n, torch.int64), "slot": (n, torch.int32), "key": (inst_cap, torch.int64), "count": (inst_cap, torch.int32),
            "bbox": (inst_cap * 6, torch.int32), "center": (inst_cap * 3, torch.float32), "centers": (n * 3, torch.float32),
            "status": (1, torch.int32)}
    out = {k: (torch.full((m + GUARD,), 77, dtype=t, device=DEV), m) for k, (m, t) in spec.items()}
    L = engine.lib()
    ws = scratch(L.lgs_instance_info_workspace_bytes(n, inst_cap), torch.device(DEV))
    engine.check(L.lgs_instance_info(ptr(coords), ptr(ids), None, n, None, 0, inst_cap, *(ptr(out[k][0]) for k in spec), ptr(ws), raw_stream()))
    return out


@pytest.mark.parity("tests/insttarget_reference.py (numpy restatement of get_instance_info)")
def test_capacity_is_exact_and_an_overflow_writes_nothing_out_of_bounds():
    coords, ids, _, _ = case("three_scenes_257")
    distinct = len(expected("three_scenes_257")[1])
    assert distinct == 18
    info = run("three_scenes_257", inst_cap=distinct)
    assert_table_equals(info, expected("three_scenes_257"), distinct)
    more_coords = np.concatenate([coords, [[3, 0, 0, 0]]]).astype(np.int32)            # one instance more: a fourth scene
    more_ids = np.concatenate([ids, [0]])
    for c, i, want_status in ((coords, ids, 0), (more_coords, more_ids, 1)):
        out = raw_instance_info(dev(c), dev(i), distinct)
        assert int(out["status"][0][0].cpu()) == want_status
        for name, (t, m) in out.items():
            assert (t[m:] == 77).all(), name                                           # the guard band is untouched
        slot = out["slot"][0][:len(i)].cpu().numpy()
        assert slot.max() < distinct and slot.min() >= -1
    assert slot[-1] == -1                                                              # the instance beyond the capacity has no row


# ---- the losses
@functools.lru_cache(maxsize=None)
def loss_case(dtype_name):
    """three_scenes_257 with offsets of |po| >= 0.1 -> (po as stored: numpy float32, bf16 values widened; the device tensor)"""
    coords, ids, _, _ = case("three_scenes_257")
    rng = np.random.default_rng(11)
    po = rng.normal(0, 0.5, (len(ids), 3))
    po *= np.maximum(1.0, 0.1 / np.linalg.norm(po, axis=1))[:, None] * 1.001
    t = torch.from_numpy(po.astype(np.float32)).to(getattr(torch, dtype_name))
    stored = t.float().numpy()
    assert np.linalg.norm(stored.astype(np.float64), axis=1).min() >= 0.1
    return stored, t.to(DEV)


def reference_losses_and_gradient(po_stored, coords, mids, centers, g_norm, g_dir):
    """the restatement's losses (float64) and autograd of instance_offset_losses evaluated in float64"""
    want = ir.offset_losses(po_stored, coords[:, 1:], centers, mids, VOXEL_W)
    p = torch.from_numpy(po_stored.astype(np.float64)).requires_grad_(True)
    nl, dl = instance_offset_losses_f64(p, coords, centers, mids)
    (g_norm * nl + g_dir * dl).backward()
    return want, p.grad.numpy()


def instance_offset_losses_f64(p, coords, centers, mids):
    """instance_offset_losses casts to float32; its lines in float64"""
    gt = (torch.from_numpy(centers.astype(np.float64)) - torch.from_numpy(coords[:, 1:].astype(np.float64))) * VOXEL_W
    valid = torch.from_numpy((mids != -1).astype(np.float64))
    denom = valid.sum() + 1e-6
    norm_loss = ((p - gt).abs().sum(-1) * valid).sum() / denom
    gt_n = gt / (gt.norm(p=2, dim=1, keepdim=True) + 1e-8)
    po_n = p / (p.norm(p=2, dim=1, keepdim=True) + 1e-8)
    return norm_loss, (-(gt_n * po_n).sum(-1) * valid).sum() / denom


def test_float64_lines_are_the_parents_lines():
    """the float64 transcription above against losses.instance_offset_losses itself (float32), so that the gradient reference is the
    parent's function and not a third formula"""
    coords, ids, _, _ = case("three_scenes_257")
    mids, _, _, _, _, _, centers = expected("three_scenes_257")
    po, _ = loss_case("float32")
    a = instance_offset_losses(torch.from_numpy(po), torch.from_numpy(coords[:, 1:]), torch.from_numpy(centers), torch.from_numpy(mids), VOXEL)
    b = instance_offset_losses_f64(torch.from_numpy(po.astype(np.float64)), coords, centers, mids)
    assert abs(float(a[0]) - float(b[0])) < 1e-5 * float(b[0]) + 1e-6 and abs(float(a[1]) - float(b[1])) < 1e-5


@pytest.mark.parity("tests/golden/insseg_res16unet14a_forward.npz (losses of the reference's trainer lines)")
def test_forward_reproduces_the_insseg_fixture():
    fx = np.load(os.path.join(G, "insseg_res16unet14a_forward.npz"))
    coords = fx["coords"].copy()
    coords[:, 0] = 0                    # that fixture took its centres over all rows: one scene as far as the ids go
    info = instances.instance_info(dev(coords), dev(fx["inst"].astype(np.int64))).check()
    valid = fx["inst"] != -1
    assert np.abs(info.center.cpu().numpy()[valid] - fx["centers"][valid]).max() <= 1e-5
    nl, dl = fused_instance_offset_losses(dev(fx["offsets"]), dev(coords), info, float(fx["voxel"]))
    print("fixture: norm %.8f (recorded %.8f)  dir %.8f (recorded %.8f)" % (float(nl), float(fx["norm_loss"]), float(dl), float(fx["dir_loss"])))
    assert abs(float(nl) - float(fx["norm_loss"])) < 1e-5 and abs(float(dl) - float(fx["dir_loss"])) < 1e-5


@pytest.mark.parity("tests/insttarget_reference.py (float64 restatement of the offset losses) + float64 autograd of instance_offset_losses")
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_losses_and_gradient_against_float64(dtype_name):
    coords, ids, _, _ = case("three_scenes_257")
    mids, _, _, _, _, _, centers = expected("three_scenes_257")
    stored, po = loss_case(dtype_name)
    g_norm, g_dir = 0.7, 1.9                                            # distinct upstream gradients
    want, want_grad = reference_losses_and_gradient(stored, coords, mids, centers, g_norm, g_dir)
    info = run("three_scenes_257")
    p = po.clone().requires_grad_(True)
    nl, dl = fused_instance_offset_losses(p, dev(coords), info, VOXEL)
    (g_norm * nl + g_dir * dl).backward()
    assert nl.dtype == torch.float32 and p.grad.dtype == po.dtype
    # forward: |d dir| <= 1e-5, |d norm| <= 1e-5 x mean(|po|_1 + |gt|_1) over the rows with an instance
    valid = mids != -1
    _, _, gt = ir.offset_rows(stored, coords[:, 1:], centers, VOXEL_W)
    scale = float((np.abs(stored).sum(1) + np.abs(gt).sum(1))[valid].mean())
    print("%s: norm %.9g (want %.9g, bound %.3g)  dir %.9g (want %.9g)" % (dtype_name, float(nl.detach()), want[0], 1e-5 * scale, float(dl.detach()), want[1]))
    assert abs(float(nl.detach()) - want[0]) <= 1e-5 * scale
    assert abs(float(dl.detach()) - want[1]) <= 1e-5
    # backward: each row within 1e-5 of that row's gradient norm; bf16 adds the output rounding, 2^-8 relative per entry
    got = p.grad.float().cpu().numpy().astype(np.float64)
    row_norm = np.linalg.norm(want_grad, axis=1)
    if dtype_name == "float32":
        err = np.linalg.norm(got - want_grad, axis=1)
        print("float32 gradient: worst row error / row norm %.3g" % float((err[valid] / row_norm[valid]).max()))
        assert (err <= 1e-5 * row_norm).all()
    else:
        excess = np.abs(got - want_grad) - (1e-5 * row_norm[:, None] + 2.0 ** -8 * np.abs(want_grad))
        print("bfloat16 gradient: worst excess over the bound %.3g" % float(excess.max()))
        assert (excess <= 0).all()
    assert (got[~valid] == 0).all() and valid.sum() > 150 and (~valid).sum() > 20


@pytest.mark.parity("float64 autograd of instance_offset_losses")
@pytest.mark.parametrize("which", ["po_is_zero", "po_is_gt"])
def test_gradient_at_the_two_kinks(which):
    """two points of one instance at x = 0 and x = 2: centre (1, 0, 0), gt of the first point = (1 * voxel, 0, 0) exactly.
    po == 0: the norm has torch's zero subgradient, the direction term is -gt_ / 1e-8.  po == gt: sign(0) = 0 for the L1 term."""
    coords = np.array([[0, 0, 0, 0], [0, 2, 0, 0]], np.int32)
    ids = np.array([3, 3], np.int64)
    centers = np.array([[1, 0, 0], [1, 0, 0]], np.float32)
    first = [0.0, 0.0, 0.0] if which == "po_is_zero" else [np.float32(VOXEL), 0.0, 0.0]
    stored = np.array([first, [0.3, -0.2, 0.1]], np.float32)
    _, want_grad = reference_losses_and_gradient(stored, coords, ids, centers, 0.7, 1.9)
    info = instances.instance_info(dev(coords), dev(ids), inst_cap=4).check()
    p = dev(stored).requires_grad_(True)
    nl, dl = fused_instance_offset_losses(p, dev(coords), info, VOXEL)
    (0.7 * nl + 1.9 * dl).backward()
    got = p.grad.cpu().numpy().astype(np.float64)
    print(which, "gradient of the row:", got[0], "want", want_grad[0])
    assert np.isfinite(got).all()
    assert np.linalg.norm(got[0] - want_grad[0]) <= 1e-5 * np.linalg.norm(want_grad[0])
    if which == "po_is_zero":
        assert abs(want_grad[0][0]) > 1e7                              # -1.9 / 2 / 1e-8
    else:
        assert abs(got[0][0]) < 1e-3 * (0.7 / 2)       # no L1 term along x (it would be 0.7 / 2): what is left is the direction term's


def test_all_ids_none_gives_zero_losses_and_a_zero_gradient():
    coords, ids, _, _ = case("three_scenes_257")
    info = instances.instance_info(dev(coords), dev(np.full(len(ids), -1, np.int64))).check()
    assert (info.slot == -1).all() and (info.count == 0).all() and (info.center == -1).all()
    p = loss_case("float32")[1].clone().requires_grad_(True)
    nl, dl = fused_instance_offset_losses(p, dev(coords), info, VOXEL)
    (nl + dl).backward()
    assert float(nl) == 0.0 and float(dl) == 0.0 and (p.grad == 0).all()


def test_the_knob_selects_the_torch_lines(monkeypatch):
    coords, ids, _, _ = case("three_scenes_257")
    info = run("three_scenes_257")
    po = loss_case("float32")[1]
    fused = fused_instance_offset_losses(po, dev(coords), info, VOXEL)
    engine.dispatch_counts(reset=True)
    monkeypatch.setenv("LGS_INST_TARGETS_FUSED", "0")
    lines = fused_instance_offset_losses(po, dev(coords), info, VOXEL)
    assert not any("k_ol_" in site for site in engine.dispatch_counts())
    parent = instance_offset_losses(po, dev(coords)[:, 1:], info.center, info.ids, VOXEL)
    assert torch.equal(lines[0], parent[0]) and torch.equal(lines[1], parent[1])
    assert abs(float(fused[0]) - float(lines[0])) < 1e-5 * max(1.0, float(lines[0])) and abs(float(fused[1]) - float(lines[1])) < 1e-5


# ---- determinism, synchronisation, the chain
def test_two_calls_give_identical_bits():
    coords, ids, _, _ = case("contention")
    po = dev(np.random.default_rng(12).normal(0, 0.5, (len(ids), 3)).astype(np.float32))
    runs = []
    for _ in range(2):
        info = run("contention")
        p = po.clone().requires_grad_(True)
        nl, dl = fused_instance_offset_losses(p, dev(coords), info, VOXEL)
        (0.7 * nl + 1.9 * dl).backward()
        runs.append([info.ids, info.slot, info.center, info.key, info.count, info.bbox, info.center_table, info.status, nl.detach(), dl.detach(),
                     p.grad])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_targets_losses_and_backward_never_synchronise():
    coords, ids, labels, masked = case("masked")
    c, i, lab = dev(coords), dev(ids), dev(labels)
    p = dev(np.random.default_rng(13).normal(0, 0.5, (len(ids), 3)).astype(np.float32)).requires_grad_(True)
    weights = dev(np.array([0.7, 1.9], np.float32))
    instances.instance_info(c, i, lab, masked)              # (the first call loads the library and sizes the scratch)
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        info = instances.instance_info(c, i, lab, masked)
        nl, dl = fused_instance_offset_losses(p, c, info, VOXEL)
        (weights[0] * nl + weights[1] * dl).backward()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert_table_equals(info, expected("masked"), 4096)


def test_the_chain_carries_the_instance_ids_through_the_dedup():
    rng = np.random.default_rng(14)
    off = [0, 1500, 2600]
    pts = dev(rng.uniform(0, 1.5, (off[-1], 3)).astype(np.float32))
    colors = dev(rng.uniform(0, 255, (off[-1], 3)).astype(np.float32))
    labels, ids = dev(rng.integers(0, 20, off[-1])), dev(rng.integers(-1, 9, off[-1]))
    aug = augment.DeviceAugmentation(0.05, seed=3)
    coords, feats, lab, inst, state = aug(pts, colors, labels, off, instances=ids, return_state=True)
    keep = state["keep"]
    assert 0 < keep.shape[0] < off[-1]                                   # the dedup dropped rows
    assert torch.equal(inst, ids[keep]) and torch.equal(lab, labels[keep]) and inst.shape[0] == coords.shape[0]
    info = instances.instance_info(coords, inst).check()                 # and the result feeds the targets
    want = ir.batch_instance_info(coords.cpu().numpy(), inst.cpu().numpy())
    assert_table_equals(info, (inst.cpu().numpy(),) + want, 4096)
    three = augment.DeviceAugmentation(0.05, seed=3)(pts, colors, labels, off)
    assert len(three) == 3 and torch.equal(three[0], coords)             # nothing changes without instances=
