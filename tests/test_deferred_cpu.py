"""The deferred ME surface (languagegroundedsemseg_amd/me/deferred.py) on the CPU oracle backend: what is recorded for the
reference's call sequence (/root/reference/models/modules/resnet_block.py:41-57, models/res16unet.py:196-270), that executing the
record equals executing every call immediately, and the rules that keep it a faithful ME surface (program order, in-place
semantics, hooks, grad modes, train/eval switches, failures)."""
import os
import types

import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
from helpers import Cfg, deterministic_init, small_scene
from languagegroundedsemseg_amd import models
from languagegroundedsemseg_amd.me import deferred
from oracle.backend import OracleBackend


@pytest.fixture(autouse=True)
def _oracle_backend():
    prev = ME.set_backend(OracleBackend("torch"))
    was = deferred.ENABLED, deferred.INCREMENTAL
    deferred.ENABLED, deferred.INCREMENTAL = True, False      # the whole record stays in the queue until a value is read
    yield
    deferred.ENABLED, deferred.INCREMENTAL = was
    ME.set_backend(prev)


def _scene(n=900, seed=3, ch=3):
    coords = small_scene(seed, n=n)
    feats = np.random.default_rng(seed).uniform(-0.5, 0.5, (coords.shape[0], ch)).astype(np.float32)
    return torch.from_numpy(coords), torch.from_numpy(feats)


def _block(cin=8, planes=8, seed=1, downsample=False):
    ds = None
    if downsample:
        ds = torch.nn.Sequential(ME.MinkowskiConvolution(cin, planes, kernel_size=1, stride=1, dimension=3), ME.MinkowskiBatchNorm(planes))
    return deterministic_init(models.BasicBlock(cin, planes, downsample=ds), seed).train()


def test_reference_block_sequence_is_recorded_as_fused_units():
    c, f = _scene(ch=8)
    for ds in (False, True):
        blk = _block(8, 16 if ds else 8, downsample=ds)
        x = ME.SparseTensor(f, c)
        y = blk(x)
        q = x.coordinate_manager._pending
        kinds = [(op.kind, op.relu, op.residual is not None) for op in q]
        C, B = deferred.CONV, deferred.BN
        if ds:    # conv1, norm1+relu, conv2, downsample conv, downsample norm, norm2 + residual + relu (moved behind its residual)
            assert kinds == [(C, False, False), (B, True, False), (C, False, False), (C, False, False), (B, False, False), (B, True, True)]
            assert q[-1].residual is q[-2].out and q[-1].mod is blk.norm2
        else:
            assert kinds == [(C, False, False), (B, True, False), (C, False, False), (B, True, True)]
            assert q[-1].residual is x
        assert y._op is q[-1] and y._F is None
        assert tuple(y.shape) == (c.shape[0], 16 if ds else 8)          # reading the shape executes the queue
        assert not x.coordinate_manager._pending and y._op is None


@pytest.mark.parametrize("name", ["Res16UNet14A", "Res16UNet34C"])
def test_deferred_equals_immediate_whole_network(name):
    c, f = _scene(1500)
    lab = torch.from_numpy(np.random.default_rng(0).integers(-1, 20, c.shape[0]).astype(np.int64))

    def run(defer):
        deferred.ENABLED = defer
        m = deterministic_init(models.load_model(name)(3, 20, Cfg()), 42).train()
        x = ME.SparseTensor(f, c)
        logits, out = m(x)
        n_pending = deferred.pending_ops(x.coordinate_manager)
        loss = torch.nn.functional.cross_entropy(logits.F, lab, ignore_index=-1)
        loss.backward()
        return (logits.F.detach(), out.F.detach(), {k: p.grad.clone() for k, p in m.named_parameters()},
                {k: b.clone() for k, b in m.named_buffers()}, n_pending)

    hints0 = deferred.STATS["cat_hints"]
    a, b = run(True), run(False)
    n_units = {"Res16UNet14A": 33 + 32 + 4, "Res16UNet34C": 63 + 62 + 4}[name]       # convs + norms + cats: ReLUs and adds are epilogues
    assert a[4] == n_units and b[4] == 0
    assert deferred.STATS["cat_hints"] == hints0 + 4                 # all four me.cat(up, skip): `up` goes straight into the concat buffer
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("name", ["Res16UNet14A", "Res16UNet34C"])
def test_incremental_execution_runs_the_head_of_the_queue_and_equals_immediate(name):
    """INCREMENTAL (the default): a recorded call executes as soon as no later call can change it, so the queue never holds more
    than the open tail of one residual block; results are those of immediate execution"""
    c, f = _scene(1500)
    lab = torch.from_numpy(np.random.default_rng(0).integers(-1, 20, c.shape[0]).astype(np.int64))
    deferred.INCREMENTAL = True
    depth = []
    orig = deferred.advance

    def spy(mgr):
        orig(mgr)
        depth.append(len(mgr._pending))
    deferred.advance = spy
    try:
        def run(defer):
            deferred.ENABLED = defer
            m = deterministic_init(models.load_model(name)(3, 20, Cfg()), 42).train()
            logits, out = m(ME.SparseTensor(f, c))
            loss = torch.nn.functional.cross_entropy(logits.F, lab, ignore_index=-1)
            loss.backward()
            return logits.F.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, {k: b.clone() for k, b in m.named_buffers()}
        hints0 = deferred.STATS["cat_hints"]
        a = run(True)
        assert deferred.STATS["cat_hints"] == hints0 + 4             # the four me.cat(up, skip): `up` written into the concat buffer
        assert depth and max(depth) <= 6                             # conv, norm, conv, norm, downsample conv, downsample norm
        b = run(False)
    finally:
        deferred.advance = orig
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_inplace_semantics_relu_and_iadd_after_a_consumer_are_not_absorbed():
    c, f = _scene(ch=8)
    bn = ME.MinkowskiBatchNorm(8).train()
    conv = ME.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3)
    relu = ME.MinkowskiReLU(inplace=True)
    x = ME.SparseTensor(f, c)
    out = bn(x)
    z = conv(out)                                  # consumes the un-rectified norm output
    op = out._op
    assert not deferred.relu_inplace(out) and not op.relu
    r = ME.SparseTensor(torch.ones_like(f), coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    assert not deferred.add_residual(out, r) and op.residual is None
    ref = torch.nn.functional.batch_norm(f, None, None, training=True)
    assert torch.allclose(out.F, ref, atol=1e-5)
    # the absorbed order is norm -> (+= residual) -> relu only: a `+=` after the ReLU runs on the value
    out2 = relu(bn(x))
    assert out2._op.relu
    out2 += r
    assert out2._op is None and torch.allclose(out2.F, torch.relu(ref) + 1, atol=1e-5)
    # not in place: a new tensor, the norm's own output stays un-rectified
    out3 = bn(x)
    y3 = ME.MinkowskiReLU(inplace=False)(out3)
    assert y3 is not out3 and torch.allclose(out3.F, ref, atol=1e-5) and torch.allclose(y3.F, torch.relu(ref), atol=1e-5)
    assert torch.isfinite(z.F).all()


def test_module_hooks_fire_at_call_time_and_force_the_call_by_call_sequence():
    c, f = _scene(ch=8)
    blk = _block()
    seen = []
    blk.norm2.register_forward_hook(lambda m, a, out: seen.append(float(out.F.abs().sum())))   # reads .F: executes what is recorded
    x = ME.SparseTensor(f, c)
    y = blk(x)
    assert len(seen) == 1
    deferred.ENABLED = False
    want = _block()(ME.SparseTensor(f, c)).F
    assert torch.equal(y.F, want)


def test_grad_mode_is_the_one_of_the_call_not_of_the_read():
    c, f = _scene(ch=8)
    blk = _block()
    with torch.no_grad():
        y = blk(ME.SparseTensor(f, c))
    assert y._op is not None
    assert not y.F.requires_grad                      # read with grad enabled, recorded without
    y2 = blk(ME.SparseTensor(f, c))
    with torch.no_grad():
        feats = y2.F
    assert feats.requires_grad


def test_train_eval_switch_executes_what_is_pending_first():
    c, f = _scene(ch=8)
    bn = ME.MinkowskiBatchNorm(8).train()
    x = ME.SparseTensor(f, c)
    out = bn(x)
    bn.eval()                                         # batch statistics were asked for: they are what runs
    assert out._op is None
    assert torch.allclose(out.F, torch.nn.functional.batch_norm(f, None, None, training=True), atol=1e-5)
    assert int(bn.bn.num_batches_tracked) == 1


def test_a_dropped_result_runs_when_it_is_dropped():
    """`norm(x)` whose result nobody keeps (a statistics-recalibration pass, a hook-free warm-up): nothing can read or modify the
    pending tensor any more, so the call executes when the tensor is collected -- running statistics move exactly as if the call
    had executed immediately"""
    c, f = _scene(ch=8)
    for incremental in (False, True):
        deferred.INCREMENTAL = incremental
        bn = ME.MinkowskiBatchNorm(8, momentum=0.5).train()
        x = ME.SparseTensor(f * 3 + 1, c)
        for k in range(2):
            bn(x)
            assert int(bn.bn.num_batches_tracked) == k + 1
        ref = torch.nn.BatchNorm1d(8, momentum=0.5).train()
        for _ in range(2):
            ref(f * 3 + 1)
        assert torch.allclose(bn.bn.running_mean, ref.running_mean, atol=1e-6) and torch.allclose(bn.bn.running_var, ref.running_var, atol=1e-5)
        assert not x.coordinate_manager._pending
    # a dropped model output: every norm of the network has updated its statistics once
    deferred.INCREMENTAL = True
    cc, ff = _scene(1500)
    m = deterministic_init(models.load_model("Res16UNet14A")(3, 20, Cfg()), 42).train()
    m.representation_only(True)
    m(ME.SparseTensor(ff, cc))
    assert all(int(b) == 1 for k, b in m.named_buffers() if k.endswith("num_batches_tracked"))


def test_failure_inside_the_queue_poisons_later_reads():
    c, f = _scene(ch=8)
    conv = ME.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3)
    bn = ME.MinkowskiBatchNorm(8).train()
    x = ME.SparseTensor(f, c)
    a = conv(x)
    b = bn(a)
    orig = conv._forward_now
    conv._forward_now = lambda *a_, **k_: (_ for _ in ()).throw(ValueError("boom"))
    try:
        with pytest.raises(ValueError):
            b.F
    finally:
        conv._forward_now = orig
    with pytest.raises(RuntimeError, match="boom"):
        b.F
    with pytest.raises(RuntimeError, match="boom"):
        a.F


def test_channel_mismatch_raises_at_the_call():
    c, f = _scene(ch=8)
    conv = ME.MinkowskiConvolution(8, 16, kernel_size=3, dimension=3)
    bad = ME.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3)
    with pytest.raises(AssertionError, match="Channel size mismatch"):
        bad(conv(ME.SparseTensor(f, c)))


def test_the_reference_files_unchanged_record_the_same_units_and_match_the_build_model():
    """the reference's models/res16unet.py + modules/resnet_block.py, imported as they are, were recorded as fused units and computed
    logits on this backend (tests/golden/make_fixtures.py deferred_units): the build's models.py has the same state-dict keys, is
    recorded as the same units and computes the same logits (the build model IS that call sequence)."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "deferred_units_res16unet34c.npz"))
    c, f = torch.from_numpy(fx["coords"]), torch.from_numpy(fx["feats"])
    ref_units = [(int(k), str(m), bool(r), bool(s)) for k, m, r, s in zip(fx["unit_kind"], fx["unit_mod"], fx["unit_relu"],
                                                                            fx["unit_residual"])]
    mine = deterministic_init(models.load_model("Res16UNet34C")(3, 20, Cfg()), 42).train()
    assert [k for k, _ in mine.state_dict().items()] == [str(k) for k in fx["state_keys"]]
    xm = ME.SparseTensor(f, c)
    lm, _ = mine(xm)
    units = [(op.kind, type(op.mod).__name__, op.relu, op.residual is not None) for op in xm.coordinate_manager._pending]
    assert units == ref_units and len(units) == 63 + 62 + 4
    ref = torch.from_numpy(fx["logits"])
    assert float((lm.F - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))     # BLAS summation order only
    deferred.ENABLED = False
    mine2 = deterministic_init(models.load_model("Res16UNet34C")(3, 20, Cfg()), 42).train()
    l2, _ = mine2(ME.SparseTensor(f, c))
    assert torch.equal(l2.F, lm.F)
