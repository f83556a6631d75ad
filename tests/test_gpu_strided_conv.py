"""Strided and dilated 3^3 convolutions on the engine (lgs_manager_kernel_map_ex): the three new kernel-map relations as sets of
coordinate triples against oracle.kernel_map, and forward / dgrad / dgrad-accumulate / wgrad on them, `transposed` 0 and 1, bf16
and fp32, against the fp64 reference and contracts of tests/precision.py (no tolerance of its own).

Scenes: two or three batch indices, negative coordinates, rows in random order, at tensor strides 1 and 2; one scene so sparse
that most strided offsets have no pair; a manager with zero rows."""
import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
import precision as P

pytestmark = [pytest.mark.gpu, pytest.mark.parity]
DEV = "cuda:0"


def _scene(seed, n=1400, extent=22, batches=3, step=1):
    """noisy planes in [-extent, extent)^3 per batch index, shuffled; step > 1 thins the cloud to multiples of `step`"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(batches):
        m = n // batches
        u = rng.integers(-extent, extent, (m, 2))
        h = (rng.integers(-2, 3, m) + rng.integers(-6, 6)).astype(np.int64)
        axis = int(rng.integers(0, 3))
        p = np.insert(u, axis, h, axis=1) * step
        out.append(np.concatenate([np.full((m, 1), b), p], 1))
    c = np.unique(np.concatenate(out).astype(np.int32), axis=0)
    return c[rng.permutation(c.shape[0])]


SCENES = {
    "planes": lambda: _scene(3),
    "planes2": lambda: _scene(4, n=900, batches=2),
    "sparse": lambda: _scene(5, n=500, extent=40, step=3),      # isolated voxels: most strided offsets are absent
}
# relation -> (kernel size, strided, dilation)
RELATIONS = {"3^3 stride 2": (3, True, 1), "1x1 stride 2": (1, True, 1), "3^3 dilation 2": (3, False, 2), "3^3 dilation 4": (3, False, 4)}


class Maps:
    """one manager: the maps of every relation at input tensor stride `ts` (1 or 2), with their oracle pair lists"""

    def __init__(self, coords, ts):
        self.x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), torch.from_numpy(coords).to(DEV))
        self.mgr = self.x.coordinate_manager
        self.key = self.x.coordinate_map_key
        if ts == 2:
            self.key = self.mgr.stride(self.key, 2)
        self.ts = ts
        self.cache = {}

    def get(self, rel):
        if rel not in self.cache:
            ks, strided, dil = RELATIONS[rel]
            out_key = self.mgr.stride(self.key, 2) if strided else self.key
            km = self.mgr.kernel_map_handle(self.key, out_key, ks, dil)
            ci = self.mgr.get_coordinates(self.key).cpu().numpy()
            co = self.mgr.get_coordinates(out_key).cpu().numpy()
            from oracle import oracle as orc
            k, i, o = orc.kernel_map(ci, co, ks, self.ts * dil)
            self.cache[rel] = (km, ci, co, (k, i, o), P.Pairs(k, i, o, ks ** 3))
        return self.cache[rel]


@pytest.fixture(scope="module")
def maps():
    cache = {}

    def get(scene, ts):
        if (scene, ts) not in cache:
            cache[(scene, ts)] = Maps(SCENES[scene](), ts)
        return cache[(scene, ts)]
    return get


def _triples(k, ci, co):
    return set(map(tuple, np.concatenate([np.asarray(k, np.int64)[:, None], ci, co], 1).tolist()))


@pytest.mark.parametrize("ts", [1, 2])
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("rel", list(RELATIONS))
def test_maps_equal_the_oracle_as_sets_of_coordinate_triples(rel, scene, ts, maps):
    m = maps(scene, ts)
    km, ci, co, (k, i, o), _ = m.get(rel)
    hk, hi, ho = (t.cpu().numpy() for t in km.export())
    assert hk.shape[0] == k.shape[0], (hk.shape, k.shape)
    want = _triples(k, ci[i], co[o])
    got = _triples(hk, ci[hi], co[ho])
    assert len(got) == hk.shape[0], "the engine exported a pair twice"
    assert got == want
    assert k.shape[0] > 0
    if scene == "sparse" and RELATIONS[rel][1] and RELATIONS[rel][0] == 3:
        assert k.shape[0] < 3 * co.shape[0], "the sparse scene is meant to leave most of the 27 strided offsets without a pair"
    assert m.mgr._m.check() == 0


def test_the_old_entry_point_and_the_cache_are_untouched(maps):
    """dilation 1 on the three old relations returns the object lgs_manager_kernel_map returns; the dilated and the strided maps
    are objects of their own; stride 2 with dilation > 1 and dilation on other kernel sizes are refused with a message"""
    import ctypes
    from languagegroundedsemseg_amd import engine
    m = maps("planes", 1)
    L, h = engine.lib(), m.mgr._m.h
    k0, k1 = m.key.id, m.mgr.stride(m.key, 2).id

    def ex(i, o, ks, d):
        p = ctypes.c_void_p(None)
        rc = L.lgs_manager_kernel_map_ex(h, i, o, ks, d, None, ctypes.byref(p))
        return rc, p.value

    def old(i, o, ks):
        p = ctypes.c_void_p(None)
        rc = L.lgs_manager_kernel_map(h, i, o, ks, None, ctypes.byref(p))
        return rc, p.value
    for i, o, ks in ((k0, k0, 3), (k0, k1, 2), (k0, k0, 1)):
        assert ex(i, o, ks, 1) == old(i, o, ks) and old(i, o, ks)[0] == 0
    d2 = ex(k0, k0, 3, 2)
    assert d2[0] == 0 and d2 == ex(k0, k0, 3, 2) and d2[1] != old(k0, k0, 3)[1] and d2[1] != ex(k0, k0, 3, 4)[1]
    s3 = ex(k0, k1, 3, 1)
    assert s3[0] == 0 and old(k0, k1, 3)[0] != 0, "the old entry point keeps refusing the strided 3^3 relation"
    assert old(k0, k0, 3)[1] != d2[1]
    for args in ((k0, k1, 3, 2), (k0, k1, 1, 2), (k0, k0, 1, 2), (k0, k0, 5, 1), (k1, k0, 3, 1), (k0, k0, 3, 1 << 17), (k0, k0, 3, 0)):
        rc, _ = ex(*args)
        assert rc != 0 and len(L.lgs_last_error()) > 0, args


def test_a_manager_with_zero_rows():
    x = ME.SparseTensor(torch.zeros(0, 8, device=DEV), torch.zeros((0, 4), dtype=torch.int32, device=DEV))
    mgr, key = x.coordinate_manager, x.coordinate_map_key
    ck = mgr.stride(key, 2)
    for ks, ok, d in ((3, ck, 1), (1, ck, 1), (3, key, 2)):
        km = mgr.kernel_map_handle(key, ok, ks, d)
        assert all(t.numel() == 0 for t in km.export())
        w = torch.randn(ks ** 3, 8, 16, device=DEV)
        for tr in (False, True):
            cin, cout = (16, 8) if tr else (8, 16)
            wt = w if not tr else torch.randn(ks ** 3, 16, 8, device=DEV)
            y = km.conv_forward(torch.zeros(0, cin, device=DEV), wt, None, tr)
            assert tuple(y.shape) == (0, cout)
            gw = km.conv_wgrad(torch.zeros(0, cin, device=DEV), torch.zeros(0, cout, device=DEV), tr)
            assert float(gw.abs().max()) == 0.0
    assert mgr._m.check() == 0


# ------------------------------------------------------------------------------------------- the ops
def _inputs(n_in, n_out, K, cin, cout, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    return x, w, g


def _modes(cin, cout):
    """the arithmetic modes of the fp32 launches, mapped as tests/test_gpu_precision_contracts.py maps them: forward / dgrad by
    FP32_SPLIT, the weight gradient by the kernel WGRAD_F32_LDS selects for the shape (lgs_wgrad.hip, wgrad_plan)"""
    from languagegroundedsemseg_amd import engine
    f = "f32_split6" if engine.tuning_get("FP32_SPLIT") else "f32_exact"
    mode = engine.tuning_get("WGRAD_F32_LDS")
    c = cin if (mode == 0 or cin % 4 == 0 or cout % 4 != 0) else (cin + 3) // 4 * 4
    split = mode != 0 and c % 4 == 0 and cout % 4 == 0 and (mode == 2 or (mode >= 3 and c >= 96 and cout <= 128))
    return f, "f32_split6" if split else "f32_exact"


SHAPES = [(64, 64), (64, 128), (128, 256), (256, 512), (3, 32)]
# every relation (dilations 2 and 4) x transposed x dtype x shape.  The narrow shapes run at input tensor strides 1 and 2 on the
# "planes" scene; the two wide ones on the smaller "planes2" scene at tensor stride 2, which keeps the fp64 reference affordable
OPS_CASES = [(rel, tr, dt, cin, cout, ts) for rel in RELATIONS for tr in (0, 1) for dt in ("bf16", "f32") for cin, cout in SHAPES
             for ts in ((2,) if cin >= 128 else (1, 2))]


@pytest.mark.parametrize("rel,tr,dt,cin,cout,ts", OPS_CASES, ids=["%s tr%d %s %d->%d ts%d" % c for c in OPS_CASES])
def test_forward_dgrad_accumulate_wgrad_meet_the_precision_contracts(rel, tr, dt, cin, cout, ts, maps):
    m = maps("planes2" if cin >= 128 else "planes", ts)
    km, ci, co, _, pr = m.get(rel)
    n_in, n_out = ci.shape[0], co.shape[0]
    if tr:                       # the transposed conv walks the same pairs from the other side: x lives on the map's out rows
        pr, n_in, n_out = pr.mirrored(), n_out, n_in
    bf16 = dt == "bf16"
    x, w, g = _inputs(n_in, n_out, pr.K, cin, cout, 7 * cin + cout + tr)
    tdt = torch.bfloat16 if bf16 else torch.float32
    xt, wt, gt = torch.from_numpy(x).to(DEV).to(tdt), torch.from_numpy(w).to(DEV), torch.from_numpy(g).to(DEV).to(tdt)
    xr, gr, wr = (P.bf16_rne(x), P.bf16_rne(g), P.bf16_rne(w)) if bf16 else (x, g, w)
    fmode, wmode = _modes(cin, cout)
    y = km.conv_forward(xt, wt, None, bool(tr))
    gin = km.conv_dgrad(gt, wt, bool(tr))
    acc0 = torch.from_numpy(np.random.default_rng(1).standard_normal((n_in, cin)).astype(np.float32)).to(DEV).to(tdt)
    acc = km.conv_dgrad(gt, wt, bool(tr), accumulate_into=acc0.clone())
    gw = km.conv_wgrad(xt, gt, bool(tr))
    gw2 = km.conv_wgrad(xt, gt, bool(tr))
    torch.cuda.synchronize()
    ref, mag, n = P.conv_ref(xr, wr, pr, n_out)
    h = y.float().cpu().numpy().astype(np.float64)
    print(P.fmt(P.check_bf16(h, ref, mag, n, "fwd") if bf16 else P.check_f32(h, ref, mag, fmode, "fwd")))
    ref, mag, n = P.dgrad_ref(gr, wr, pr, n_in)
    h = gin.float().cpu().numpy().astype(np.float64)
    print(P.fmt(P.check_bf16(h, ref, mag, n, "dgrad") if bf16 else P.check_f32(h, ref, mag, fmode, "dgrad")))
    # "store dgrad, then add", whichever of the epilogue and the separate add the launch shape takes
    assert torch.equal(acc, gin + acc0), "dgrad_accumulate differs from dgrad followed by the add"
    ref, mag, _ = P.wgrad_ref(xr, gr, pr)
    print(P.fmt(P.check_f32(gw.cpu().numpy().astype(np.float64), ref, mag, "bf16_wgrad" if bf16 else wmode, "wgrad")))
    # the pair-list and fp32 kernels write every partial once and k_wgrad_reduce adds them in a fixed order
    assert torch.equal(gw, gw2), "two runs of the weight gradient differ"


def test_the_reference_arithmetic_alone_stays_inside_contract_b(maps):
    """contract (b) lets 1 % of the elements differ from the correctly rounded reference: an fp32 accumulation in MFMA-sized blocks
    of the inputs used above must stay inside that on the CPU, or the GPU test would be measuring its inputs"""
    m = maps("planes", 1)
    _, ci, co, _, pr = m.get("3^3 stride 2")
    x, w, _ = _inputs(ci.shape[0], co.shape[0], 27, 64, 64, 7 * 64 + 64)
    xr, wr = P.bf16_rne(x), P.bf16_rne(w)
    ref, mag, n = P.conv_ref(xr, wr, pr, co.shape[0])
    emu = P.emulate_conv(xr, wr, pr, co.shape[0], "bf16", block=16, store="rne")
    rep = P.check_bf16(emu, ref, mag, n, "emulated strided forward")
    print(P.fmt(rep))
    assert rep["bit-equal"] >= 0.995


@pytest.mark.parametrize("rel", ["3^3 stride 2", "1x1 stride 2", "3^3 dilation 2"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_packed_weight_images_give_the_bits_of_the_internal_pack(rel, dt, maps):
    from languagegroundedsemseg_amd import engine
    from languagegroundedsemseg_amd.me.backend_hip import get_packed
    m = maps("planes", 1)
    km, ci, co, _, pr = m.get(rel)
    for tr in (False, True):
        n_in, n_out = (co.shape[0], ci.shape[0]) if tr else (ci.shape[0], co.shape[0])
        for cin, cout in ((64, 128), (3, 32)):
            x = torch.randn(n_in, cin, device=DEV).to(dt)
            g = torch.randn(n_out, cout, device=DEV).to(dt)
            w = torch.nn.Parameter(torch.randn(pr.K, cin, cout, device=DEV) / 8)
            cache = {}
            y0, g0 = km.conv_forward(x, w, None, tr), km.conv_dgrad(g, w, tr)
            y1, g1 = km.conv_forward(x, w, None, tr, pack_cache=cache), km.conv_dgrad(g, w, tr, pack_cache=cache)     # pack_mode 1
            y2, g2 = km.conv_forward(x, w, None, tr, pack_cache=cache), km.conv_dgrad(g, w, tr, pack_cache=cache)     # pack_mode 2
            assert torch.equal(y0, y1) and torch.equal(y0, y2) and torch.equal(g0, g1) and torch.equal(g0, g2), (rel, tr, cin, cout)
            code = engine.LGS_BF16 if dt == torch.bfloat16 else engine.LGS_F32
            for op in (0, 1):
                d = engine.PackDesc()
                engine.check(engine.lib().lgs_conv_pack_desc(km.h, op, int(tr), cin, cout, code, d))
                if d.bytes == 0:        # the host must not have made an image for it
                    assert get_packed().lookup(cache, km, op, tr, w, w, cin, cout, code) == (None, 0)
                    assert not any(k[0] == op for k in cache), (rel, tr, cin, cout, op)
                else:
                    assert any(k[0] == op for k in cache)


# ------------------------------------------------------------------------------------------- modules and autograd
@pytest.mark.parametrize("ks,st,dil", [(3, 2, 1), (1, 2, 1), (3, 1, 2), (3, 1, 4)])
def test_modules_run_forward_and_backward_through_autograd(ks, st, dil):
    """the module surface and autograd wiring on top of the op contracts above, fp32: output, input gradient and weight gradient
    of conv(x) are held to the fp32 contracts of tests/precision.py against the fp64 reference on the oracle's pair lists (no
    tolerance of this test's own)"""
    from oracle import oracle as orc
    torch.manual_seed(0)
    c = torch.from_numpy(_scene(8, n=1200)).to(DEV)
    conv = ME.MinkowskiConvolution(16, 32, kernel_size=ks, stride=st, dilation=dil, dimension=3).to(DEV)
    f = torch.randn(c.shape[0], 16, device=DEV, requires_grad=True)
    x = ME.SparseTensor(f, c)
    y = conv(x)
    g = torch.randn_like(y.F)
    y.F.backward(g)
    mgr = x.coordinate_manager
    ci, co = mgr.get_coordinates(x.coordinate_map_key).cpu().numpy(), y.C.cpu().numpy()
    want = {(b, *(v // st * st for v in xyz)) for b, *xyz in ci.tolist()}
    assert set(map(tuple, co.tolist())) == want and y.tensor_stride[0] == st
    pr = P.Pairs(*orc.kernel_map(ci, co, ks, dil), ks ** 3)
    xr, gr = f.detach().cpu().numpy(), g.cpu().numpy()
    wr = conv.kernel.detach().cpu().numpy().reshape(ks ** 3, 16, 32)
    fmode, wmode = _modes(16, 32)
    ref, mag, _ = P.conv_ref(xr, wr, pr, co.shape[0])
    print(P.fmt(P.check_f32(y.F.detach().cpu().numpy(), ref, mag, fmode, "module fwd")))
    ref, mag, _ = P.dgrad_ref(gr, wr, pr, ci.shape[0])
    print(P.fmt(P.check_f32(f.grad.cpu().numpy(), ref, mag, fmode, "module dgrad")))
    ref, mag, _ = P.wgrad_ref(xr, gr, pr)
    print(P.fmt(P.check_f32(conv.kernel.grad.cpu().numpy().reshape(ref.shape), ref, mag, wmode, "module wgrad")))


def test_transposed_strided_3x3x3_lands_on_the_cached_finer_map():
    from oracle import oracle as orc
    torch.manual_seed(1)
    c = torch.from_numpy(_scene(9, n=1000)).to(DEV)
    down = ME.MinkowskiConvolution(8, 16, kernel_size=3, stride=2, dimension=3).to(DEV)
    up = ME.MinkowskiConvolutionTranspose(16, 8, kernel_size=3, stride=2, dimension=3).to(DEV)
    x = ME.SparseTensor(torch.randn(c.shape[0], 8, device=DEV), c)
    mid = down(x)
    z = up(mid)
    assert z.coordinate_map_key == x.coordinate_map_key and tuple(z.F.shape) == (c.shape[0], 8)
    ci, co = z.C.cpu().numpy(), mid.C.cpu().numpy()
    pr = P.Pairs(*orc.kernel_map(ci, co, 3, 1), 27).mirrored()
    ref, mag, _ = P.conv_ref(mid.F.detach().cpu().numpy(), up.kernel.detach().cpu().numpy(), pr, ci.shape[0])
    print(P.fmt(P.check_f32(z.F.detach().cpu().numpy(), ref, mag, _modes(16, 8)[0], "transposed module fwd")))


def test_dilated_blocks_deferred_and_immediate_agree():
    """stride-1 BasicBlocks with dilation 2 and 4: off the fused-block fast path, op by op (conv -> norm -> relu still fused as for
    single ops); deferred execution and LGS_DEFER=0 agree"""
    from languagegroundedsemseg_amd import models
    from languagegroundedsemseg_amd.me import deferred
    from helpers import deterministic_init
    c = torch.from_numpy(_scene(11, n=3000, extent=30)).to(DEV)
    f = torch.randn(c.shape[0], 32, device=DEV)

    def run(enabled):
        prev = deferred.ENABLED
        deferred.ENABLED = enabled
        try:
            net = torch.nn.Sequential(models.BasicBlock(32, 32, dilation=2), models.BasicBlock(32, 32, dilation=4))
            net = deterministic_init(net, 5).to(DEV).train()
            y = net(ME.SparseTensor(f, c))
            y.F.float().square().mean().backward()
            return y.F.detach().cpu().numpy(), [p.grad.detach().cpu().numpy() for p in net.parameters()]
        finally:
            deferred.ENABLED = prev
    a, b = run(True), run(False)
    assert np.isfinite(a[0]).all()
    # the tolerances tests/test_gpu_model.py applies between two executions of one model (logits 1e-3; gradients 2e-3 relative L2)
    assert np.abs(a[0] - b[0]).max() < 1e-3
    for ga, gb in zip(a[1], b[1]):
        assert np.linalg.norm(ga - gb) / max(1e-12, np.linalg.norm(gb)) < 2e-3


# ------------------------------------------------------------------------------------------- ResNet14 against a restatement on the oracle's pair lists
def _o_conv(x, conv, c_in, c_out, ts_in):
    from oracle import oracle as orc
    ks = conv.kernel_size[0]
    k, i, o = orc.kernel_map(c_in, c_out, ks, ts_in * conv.dilation[0])
    w = conv.kernel.reshape(ks ** 3, conv.in_channels, conv.out_channels)
    out = torch.zeros(c_out.shape[0], conv.out_channels, dtype=x.dtype)
    for kk in range(ks ** 3):
        sel = np.nonzero(k == kk)[0]
        if sel.size:
            out = out.index_add(0, torch.from_numpy(o[sel]), x[torch.from_numpy(i[sel])] @ w[kk])
    return out if conv.bias is None else out + conv.bias


def _o_bn(x, norm):
    return torch.nn.functional.batch_norm(x, None, None, norm.bn.weight, norm.bn.bias, True, 0.0, norm.bn.eps)


def _o_resnet(m, c, f):
    """ResNetBase.forward restated: every kernel map (3^3, 3^3 stride 2, 1x1 stride 2, the 2^3 sum pooling) from oracle.kernel_map /
    oracle.stride_coords on the CPU, BatchNorm and ReLU from torch, autograd from torch.  -> (output coords, logits)"""
    from oracle import oracle as orc
    ts = 1
    x = torch.relu(_o_bn(_o_conv(f, m.conv1, c, c, ts), m.bn1))
    c2 = orc.stride_coords(c, ts * 2)[0]
    k, i, o = orc.kernel_map(c, c2, 2, ts)                       # sum pooling: every pair with unit weight
    x = torch.zeros(c2.shape[0], x.shape[1], dtype=x.dtype).index_add(0, torch.from_numpy(o), x[torch.from_numpy(i)])
    c, ts = c2, ts * 2
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            st = blk.conv1.stride[0]
            c2 = orc.stride_coords(c, ts * 2)[0] if st == 2 else c
            out = torch.relu(_o_bn(_o_conv(x, blk.conv1, c, c2, ts), blk.norm1))
            out = _o_bn(_o_conv(out, blk.conv2, c2, c2, ts * st), blk.norm2)
            res = x if blk.downsample is None else _o_bn(_o_conv(x, blk.downsample[0], c, c2, ts), blk.downsample[1])
            x = torch.relu(out + res)
            c, ts = c2, ts * st
    return c, _o_conv(x, m.final, c, c, ts)


def test_resnet14_forward_backward_against_the_oracle_pair_lists():
    """ResNet14, fp32, default dilations, HIP backend against a float64 restatement of the same weights and input on the oracle's
    coordinate and kernel maps (the oracle BACKEND has neither the sum pooling nor the 1x1 stride-2 map; oracle.kernel_map is
    generic in both).  The comparison and tolerances tests/test_gpu_model.py applies to Res16UNet14A: logits 1e-3, loss 1e-4,
    per-tensor gradients 2e-3 relative L2 and 3e-2 of the largest element; the output coordinates as a set."""
    import copy
    from languagegroundedsemseg_amd import models
    from helpers import Cfg, deterministic_init
    assert list(Cfg.dilations) == [1, 1, 1, 1]
    cn = _scene(10, n=6000, extent=40)
    fn = np.random.default_rng(0).standard_normal((cn.shape[0], 3)).astype(np.float32)

    def labels(coords):
        return torch.from_numpy((np.abs(coords[:, 1:]).sum(1) // 32 + coords[:, 0]) % 20).long()
    m = deterministic_init(models.load_model("ResNet14")(3, 20, Cfg()), 42)
    mo = copy.deepcopy(m).double().train()
    m = m.to(DEV).train()
    y = m(ME.SparseTensor(torch.from_numpy(fn).to(DEV), torch.from_numpy(cn).to(DEV)))
    hc = y.C.cpu().numpy()
    h_loss = torch.nn.functional.cross_entropy(y.F.float(), labels(hc).to(DEV))
    h_loss.backward()
    oc, ol = _o_resnet(mo, cn, torch.from_numpy(fn).double())
    o_loss = torch.nn.functional.cross_entropy(ol, labels(oc))
    o_loss.backward()
    assert y.tensor_stride[0] == 32 and hc.shape[0] == oc.shape[0] >= 8
    assert set(map(tuple, hc.tolist())) == set(map(tuple, oc.tolist()))
    hl = y.F.detach().cpu().numpy()[np.lexsort(hc.T[::-1])]
    olr = ol.detach().numpy()[np.lexsort(oc.T[::-1])]
    print("max |logit - reference| %.3g, loss %.6f vs %.6f" % (np.abs(hl - olr).max(), float(h_loss), float(o_loss)))
    assert np.abs(hl - olr).max() < 1e-3
    assert abs(float(h_loss) - float(o_loss)) < 1e-4
    og = dict(mo.named_parameters())
    for k, p in m.named_parameters():
        hg, rg = p.grad.detach().cpu().numpy().astype(np.float64), og[k].grad.numpy()
        e = np.linalg.norm(hg - rg) / max(1e-12, np.linalg.norm(rg))
        mx = np.abs(hg - rg).max() / max(1e-6, np.abs(rg).max())
        assert e < 2e-3 and mx < 3e-2, (k, e, mx)


def test_resnet14_deferred_and_immediate_agree():
    """the default (deferred execution) and LGS_DEFER=0 on ResNet14: same coordinates, logits and gradients"""
    from languagegroundedsemseg_amd import models
    from languagegroundedsemseg_amd.me import deferred
    from helpers import Cfg, deterministic_init
    c = torch.from_numpy(_scene(10, n=6000, extent=40)).to(DEV)
    f = torch.randn(c.shape[0], 3, device=DEV)

    def run(enabled):
        prev = deferred.ENABLED
        deferred.ENABLED = enabled
        try:
            m = deterministic_init(models.load_model("ResNet14")(3, 20, Cfg()), 42).to(DEV).train()
            y = m(ME.SparseTensor(f, c))
            y.F.float().square().mean().backward()
            return y.C.cpu().numpy(), y.F.detach().cpu().numpy(), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}
        finally:
            deferred.ENABLED = prev
    a, b = run(True), run(False)
    assert np.array_equal(a[0], b[0])
    # the tolerances tests/test_gpu_model.py applies between two executions of one model (logits 1e-3; gradients 2e-3 relative L2)
    assert np.isfinite(a[1]).all() and np.abs(a[1] - b[1]).max() < 1e-3
    for n in a[2]:
        assert np.linalg.norm(a[2][n] - b[2][n]) / max(1e-12, np.linalg.norm(b[2][n])) < 2e-3, n
