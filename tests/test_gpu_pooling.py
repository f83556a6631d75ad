"""Pooling, global pooling and broadcast on the engine (lgs_seg_reduce / lgs_seg_broadcast / lgs_seg_max_backward) against the
float64 torch reference of tests/pool_reference.py, which works from the coordinates alone.

  local pooling (kernel_size == stride == 2^k)  /root/reference/models/modules/common.py:239-300, models/resnet.py:48
  MinkowskiPoolingTranspose (8 / 4 / 2)          /root/reference/models/resunet.py:367,388,409
  global pooling + broadcast norms               /root/reference/downstream/insseg/lib/layers.py

Tolerances: fp32 sums / averages within n u of the reference (n = rows of the segment, u = 2^-24, relative to the sum of
magnitudes), bf16 within one bf16 ulp of the fp32-rounded reference, max and every copy bit-exact."""
import pytest
import torch

import MinkowskiEngine as ME
from pool_reference import batches, cells, max_argrow, max_backward, seg_reduce

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY = pytest.mark.parity("float64 torch pooling reference")
U32 = 2.0 ** -24


def _scene(seed, n=2500, span=14, batch_ids=(0, 1)):
    """unique random voxels, rows in random (not Morton) order"""
    g = torch.Generator().manual_seed(seed)
    per = n // len(batch_ids)
    rows = []
    for b in batch_ids:
        c = torch.randint(-span, span, (per * 2, 3), generator=g)
        c = torch.unique(c, dim=0)[:per]
        rows.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int64), c], 1))
    coords = torch.cat(rows, 0)
    coords = coords[torch.randperm(coords.shape[0], generator=g)]
    return coords.to(torch.int32)


def _keys(c):
    c = c.to(torch.int64)
    off, k = 1 << 15, 1 << 16          # |x|, |y|, |z| < 2^15, batch < 2^15: the key fits in 63 bits
    assert bool((c[:, 1:].abs() < off).all()) and bool((c[:, 0] < off).all())
    return ((c[:, 0] * k + c[:, 1] + off) * k + c[:, 2] + off) * k + c[:, 3] + off


def _match(engine_coords, ref_coords):
    """-> index into ref_coords of every engine row (asserts the two coordinate sets are equal)"""
    ke, kr = _keys(engine_coords), _keys(ref_coords)
    assert ke.shape == kr.shape
    srt, order = torch.sort(kr)
    pos = torch.searchsorted(srt, ke)
    assert torch.equal(srt[pos], ke), "engine and reference coordinates differ"
    return order[pos]


def _bf16_ulp(r):
    a = r.abs().to(torch.float64).clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def _check_sum_like(h, ref, abs_sum, cnt):
    """fp32: |h - ref| <= (cnt + 1) u sum|x|; bf16: within one ulp of the fp32-rounded reference"""
    if h.dtype == torch.float32:
        bound = (cnt.view(-1, 1).to(torch.float64) + 1) * U32 * abs_sum + 1e-30
        err = (h.double() - ref).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
    else:
        r = ref.float().to(torch.bfloat16).double()
        err = (h.double() - r).abs()
        assert bool((err <= _bf16_ulp(r)).all()), float(err.max())


def _source(x0, level, c, dtype, seed):
    """(leaf features, SparseTensor) on level 0 (the caller's row order) or level 1 (the identity-order path)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if level == 0:
        f = torch.randn(x0.F.shape[0], c, generator=g, device=DEV).to(dtype).requires_grad_(True)
        return f, ME.SparseTensor(f, coordinate_map_key=x0.coordinate_map_key, coordinate_manager=x0.coordinate_manager)
    mgr = x0.coordinate_manager
    key = mgr.coarser_key(x0.coordinate_map_key, 2)
    f = torch.randn(mgr.size(key), c, generator=g, device=DEV).to(dtype).requires_grad_(True)
    return f, ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=mgr)


POOLS = {"sum": ME.MinkowskiSumPooling, "avg": ME.MinkowskiAvgPooling, "max": ME.MinkowskiMaxPooling}


@PARITY
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("level,c", [(0, 96), (0, 3), (1, 32), (1, 200)])
@pytest.mark.parametrize("op", ["sum", "avg", "max"])
def test_local_pooling_forward_backward(op, level, c, s, dtype):
    coords = _scene(100 + s + c)
    x0 = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), coords.to(DEV))
    f, src = _source(x0, level, c, dtype, seed=s * 7 + c)
    out = POOLS[op](kernel_size=s, stride=s, dimension=3)(src)
    ts = src.tensor_stride[0]
    assert out.tensor_stride == [ts * s] * 3
    cin = src.C.cpu()
    uniq, idx = cells(cin, ts * s)
    m = uniq.shape[0]
    assert out.F.shape == (m, c)
    rix = _match(out.C.cpu(), uniq).to(DEV)
    idx = idx.to(DEV)
    fd = f.detach().double()
    ref = seg_reduce(fd, idx, m, op)[rix]
    h = out.F.detach()
    cnt = torch.bincount(idx, minlength=m).to(DEV)[rix]
    if op == "max":
        assert torch.equal(h.double(), ref)
    else:
        abs_sum = seg_reduce(fd.abs(), idx, m, "sum")[rix]
        _check_sum_like(h, ref, abs_sum / (cnt.view(-1, 1) if op == "avg" else 1), cnt)
    # backward against autograd of the reference (max: the smallest-row rule of max_argrow)
    dy = torch.randn(m, c, device=DEV).to(dtype)
    out.F.backward(dy)
    inv = torch.empty_like(rix)
    inv[rix] = torch.arange(m, device=DEV)
    dyr = dy.double()[inv]                                   # dy in reference row order
    if op == "max":
        want = max_backward(dyr, max_argrow(fd, idx, m), fd.shape[0])
        assert torch.equal(f.grad.double(), want)
    elif op == "sum":
        assert torch.equal(f.grad.double(), dyr[idx])
    else:
        xr = fd.clone().requires_grad_(True)
        seg_reduce(xr, idx, m, "avg").backward(dyr)
        want = xr.grad
        if dtype == torch.float32:
            assert bool(((f.grad.double() - want).abs() <= U32 * want.abs() + 1e-30).all())
        else:
            r = want.float().to(torch.bfloat16).double()
            assert bool(((f.grad.double() - r).abs() <= _bf16_ulp(r)).all())


@PARITY
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_max_pooling_tie_gradient_goes_to_the_smallest_row(dtype):
    coords = _scene(7, n=1200, span=6)
    n = coords.shape[0]
    x0 = ME.SparseTensor(torch.zeros(n, 1, device=DEV), coords.to(DEV))
    # 8 distinct values only: many ties inside every cell
    f = (torch.randint(0, 8, (n, 16), device=DEV).to(dtype) * 0.5).requires_grad_(True)
    x = ME.SparseTensor(f, coordinate_map_key=x0.coordinate_map_key, coordinate_manager=x0.coordinate_manager)
    out = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    uniq, idx = cells(coords, 2)
    rix = _match(out.C.cpu(), uniq).to(DEV)
    idx = idx.to(DEV)
    m = uniq.shape[0]
    arg = max_argrow(f.detach().double(), idx, m)
    assert int((seg_reduce(f.detach().double(), idx, m, "max")[idx] == f.detach().double()).sum()) > n * 16 // 4   # ties do occur
    dy = torch.randn(m, 16, device=DEV).to(dtype)
    out.F.backward(dy)
    inv = torch.empty_like(rix)
    inv[rix] = torch.arange(m, device=DEV)
    assert torch.equal(f.grad.double(), max_backward(dy.double()[inv], arg, n))


def test_pooled_key_equals_the_strided_convolution_key():
    coords = _scene(3)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 8, device=DEV), coords.to(DEV))
    conv = ME.MinkowskiConvolution(8, 4, kernel_size=2, stride=2, dimension=3).to(DEV)
    y = conv(x)
    p = ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3)(x)
    assert p.coordinate_map_key == y.coordinate_map_key
    z = p.F[:, :4] + y.F           # the two outputs can be added row by row
    assert z.shape == y.F.shape
    q = ME.MinkowskiAvgPooling(kernel_generator=ME.KernelGenerator(kernel_size=4, stride=4, dimension=3))(x)
    assert q.coordinate_map_key == x.coordinate_manager.coarser_key(y.coordinate_map_key, 2)


@PARITY
@pytest.mark.parametrize("cls", [ME.MinkowskiPoolingTranspose, ME.MinkowskiAvgUnpooling])
@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pooling_transpose_is_a_copy_and_its_backward_a_segment_sum(cls, s, dtype):
    coords = _scene(50 + s)
    n = coords.shape[0]
    x0 = ME.SparseTensor(torch.randn(n, 16, device=DEV).to(dtype), coords.to(DEV))
    with pytest.raises(RuntimeError, match="cached finer"):
        cls(kernel_size=s, stride=s, dimension=3)(x0)
    pooled = ME.MinkowskiSumPooling(kernel_size=s, stride=s, dimension=3)(x0)
    m = pooled.F.shape[0]
    g = torch.randn(m, 24, device=DEV).to(dtype).requires_grad_(True)
    coarse = ME.SparseTensor(g, coordinate_map_key=pooled.coordinate_map_key, coordinate_manager=x0.coordinate_manager)
    up = cls(kernel_size=s, stride=s, dimension=3)(coarse)
    assert up.coordinate_map_key == x0.coordinate_map_key
    uniq, idx = cells(coords, s)
    rix = _match(pooled.C.cpu(), uniq).to(DEV)
    inv = torch.empty_like(rix)
    inv[rix] = torch.arange(m, device=DEV)
    idx = idx.to(DEV)
    row_of = inv[idx]                              # engine coarse row of every level-0 row
    assert torch.equal(up.F.detach(), g.detach()[row_of])
    hyper = ME.cat(up, x0)                          # MinkUNetHyper-style: unpooled features next to the level-0 ones
    assert hyper.F.shape == (n, 24 + 16)
    dy = torch.randn(n, 40, device=DEV).to(dtype)
    hyper.F.backward(dy)
    want = seg_reduce(dy[:, :24].double(), row_of, m, "sum")
    abs_sum = seg_reduce(dy[:, :24].double().abs(), row_of, m, "sum")
    _check_sum_like(g.grad, want, abs_sum, torch.bincount(row_of, minlength=m))


@PARITY
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 16])
@pytest.mark.parametrize("batch_ids", [(0,), (4, 1, 9), (0, 2, 3, 5, 8, 9, 11, 20)])
@pytest.mark.parametrize("op,cls", [("sum", ME.MinkowskiGlobalSumPooling), ("avg", ME.MinkowskiGlobalAvgPooling),
                                    ("max", ME.MinkowskiGlobalMaxPooling), ("avg", ME.MinkowskiGlobalPooling)])
def test_global_pooling(op, cls, batch_ids, stride, dtype):
    coords = _scene(len(batch_ids) * 11 + stride, n=1500 * len(batch_ids), span=40, batch_ids=batch_ids)
    x0 = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), coords.to(DEV))
    mgr = x0.coordinate_manager
    key = x0.coordinate_map_key if stride == 1 else mgr.coarser_key(x0.coordinate_map_key, stride)
    c = 40
    f = torch.randn(mgr.size(key), c, device=DEV).to(dtype).requires_grad_(True)
    x = ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=mgr)
    out = cls()(x)
    b, idx = batches(x.C.cpu())
    assert b.tolist() == sorted(batch_ids)
    want_c = torch.zeros(len(batch_ids), 4, dtype=torch.int32)
    want_c[:, 0] = b.to(torch.int32)
    assert torch.equal(out.C.cpu(), want_c)
    assert out.coordinate_map_key == mgr.origin_key()
    idx = idx.to(DEV)
    m = len(batch_ids)
    fd = f.detach().double()
    ref = seg_reduce(fd, idx, m, op)
    cnt = torch.bincount(idx, minlength=m)
    if op == "max":
        assert torch.equal(out.F.detach().double(), ref)
    else:
        abs_sum = seg_reduce(fd.abs(), idx, m, "sum")
        _check_sum_like(out.F.detach(), ref, abs_sum / (cnt.view(-1, 1) if op == "avg" else 1), cnt)
    dy = torch.randn(m, c, device=DEV).to(dtype)
    out.F.backward(dy)
    if op == "max":
        assert torch.equal(f.grad.double(), max_backward(dy.double(), max_argrow(fd, idx, m), fd.shape[0]))
    elif op == "sum":
        assert torch.equal(f.grad.double(), dy.double()[idx])
    else:
        r = (dy.double() / cnt.view(-1, 1))[idx]
        if dtype == torch.float32:
            assert bool(((f.grad.double() - r).abs() <= U32 * r.abs() + 1e-30).all())
        else:
            rr = r.float().to(torch.bfloat16).double()
            assert bool(((f.grad.double() - rr).abs() <= _bf16_ulp(rr)).all())


@PARITY
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("op", ["add", "mul", "cat", "copy"])
def test_broadcast_ops(op, dtype):
    coords = _scene(21, n=3000, span=30, batch_ids=(2, 0, 7))
    n, c = coords.shape[0], 24
    f = torch.randn(n, c, device=DEV).to(dtype).requires_grad_(True)
    x = ME.SparseTensor(f, coords.to(DEV))
    pooled = ME.MinkowskiGlobalAvgPooling()(x)
    gcols = 8 if op == "cat" else c
    gf = torch.randn(pooled.F.shape[0], gcols, device=DEV).to(dtype).requires_grad_(True)
    g = ME.SparseTensor(gf, coordinate_map_key=pooled.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    mod = {"add": ME.MinkowskiBroadcastAddition, "mul": ME.MinkowskiBroadcastMultiplication,
           "cat": ME.MinkowskiBroadcastConcatenation, "copy": ME.MinkowskiBroadcast}[op]()
    y = mod(x, g)
    assert y.coordinate_map_key == x.coordinate_map_key
    _, bidx = batches(x.C.cpu())
    bidx = bidx.to(DEV)
    xr = f.detach().double().requires_grad_(True)
    gr = gf.detach().double().requires_grad_(True)
    want = {"add": lambda: xr + gr[bidx], "mul": lambda: xr * gr[bidx], "cat": lambda: torch.cat([xr, gr[bidx]], 1),
            "copy": lambda: gr[bidx]}[op]()
    h = y.F.detach().double()
    assert h.shape == want.shape
    # one rounding of an exact fp64 result: the engine's fp32 op rounded to `dtype` is the correctly rounded value
    assert torch.equal(y.F.detach(), want.detach().to(dtype)) if op in ("cat", "copy") else \
        torch.equal(y.F.detach(), want.detach().float().to(dtype))
    dy = torch.randn(*want.shape, device=DEV).to(dtype)
    y.F.backward(dy)
    want.backward(dy.double())
    m = gf.shape[0]
    if op != "copy":
        if op == "mul":
            assert torch.equal(f.grad, (dy.float() * gf.detach().float()[bidx]).to(dtype))
        else:
            assert torch.equal(f.grad.double(), xr.grad)
    else:
        assert f.grad is None
    cnt = torch.bincount(bidx, minlength=m)
    if op == "mul":
        abs_sum = seg_reduce((dy.double() * f.detach().double()).abs(), bidx, m, "sum")
    else:
        abs_sum = seg_reduce(dy.double()[:, -gcols:].abs(), bidx, m, "sum")
    _check_sum_like(gf.grad, gr.grad, abs_sum, cnt)


@PARITY
def test_instance_norm_built_from_global_pooling_and_broadcast():
    """the construction of downstream/insseg/lib/layers.py: mean, centred, variance, inverse std by global pooling and
    broadcast ops -- against a per-scene torch restatement, forward and input gradient"""
    coords = _scene(33, n=4000, span=30, batch_ids=(0, 3, 5))
    n, c, eps = coords.shape[0], 16, 1e-6
    f = (torch.randn(n, c, device=DEV) * 3 + 1).requires_grad_(True)
    x = ME.SparseTensor(f, coords.to(DEV))
    gap = ME.MinkowskiGlobalAvgPooling()
    badd, bmul = ME.MinkowskiBroadcastAddition(), ME.MinkowskiBroadcastMultiplication()
    mean = gap(x)
    xc = badd(x, ME.SparseTensor(-mean.F, coordinate_map_key=mean.coordinate_map_key, coordinate_manager=mean.coordinate_manager))
    var = gap(xc._like(xc.F ** 2))
    instd = var._like(1.0 / torch.sqrt(var.F + eps))
    y = bmul(xc, instd)
    _, bidx = batches(x.C.cpu())
    bidx = bidx.to(DEV)
    xr = f.detach().double().requires_grad_(True)
    m = int(bidx.max()) + 1
    mu = seg_reduce(xr, bidx, m, "avg")
    d = xr - mu[bidx]
    v = seg_reduce(d * d, bidx, m, "avg")
    want = d / torch.sqrt(v[bidx] + eps)
    assert float((y.F.detach().double() - want.detach()).abs().max()) < 1e-5
    dy = torch.randn(n, c, device=DEV)
    y.F.backward(dy)
    want.backward(dy.double())
    assert float((f.grad.double() - xr.grad).abs().max() / xr.grad.abs().max()) < 1e-5


@PARITY
def test_scene_head_on_the_trunk_matches_the_torch_pool():
    """Res16UNet14A trunk -> MinkowskiBatchNorm -> MinkowskiGlobalAvgPooling -> MinkowskiLinear -> cross-entropy, vs the same
    network with the pool replaced by the torch reference on the features (the norm's output is still a pending, deferred
    tensor when the engine pools it)"""
    from helpers import Cfg, deterministic_init
    from languagegroundedsemseg_amd import models
    from languagegroundedsemseg_amd.me import deferred
    from languagegroundedsemseg_amd.synthetic import make_batch
    coords, feats, _ = make_batch([0, 1, 2], voxel=0.05, n_target=8000)
    labels = torch.tensor([1, 4, 2], device=DEV)

    def run(engine_pool):
        torch.manual_seed(0)
        trunk = deterministic_init(models.load_model("Res16UNet14A")(3, 32, Cfg()), 42).to(DEV).train()
        norm = ME.MinkowskiBatchNorm(32).to(DEV).train()      # its call is recorded: a pending output to pool
        head = ME.MinkowskiLinear(32, 5).to(DEV)
        x = ME.SparseTensor(torch.from_numpy(feats).to(DEV), torch.from_numpy(coords).to(DEV))
        out = norm(trunk(x)[0])
        if engine_pool:
            assert out._op is not None or not deferred.ENABLED     # still pending: the pool materialises it
            logits = head(ME.MinkowskiGlobalAvgPooling()(out)).F
        else:
            f = out.F
            _, bidx = batches(out.C.cpu())
            logits = head.linear(seg_reduce(f, bidx.to(DEV), 3, "avg").float())
        loss = torch.nn.functional.cross_entropy(logits.float(), labels)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in trunk.named_parameters() if p.grad is not None}
        return logits.detach(), grads

    lh, gh = run(True)
    lr, gr = run(False)
    assert float((lh - lr).abs().max()) <= 1e-5 * max(1.0, float(lr.abs().max()))
    assert set(gh) == set(gr) and len(gh) > 10
    # per parameter within 1e-4 of its own gradient's magnitude, plus 1e-5 of the largest gradient of the network: a conv bias
    # in front of a BatchNorm has a gradient that is zero up to rounding, and only that rounding differs between the two runs
    gmax = max(float(g.abs().max()) for g in gr.values())
    for k in gr:
        scale = float(gr[k].abs().max())
        assert float((gh[k] - gr[k]).abs().max()) <= 1e-4 * scale + 1e-5 * gmax, k


@PARITY
def test_at_size_bf16_pooling_is_deterministic_and_host_sync_free():
    """the 8-scene batch (about 1.2 M voxels), C = 96 bf16: max and sum pooling (2, 2) and global avg pooling, forward and
    backward under torch's sync debugger, twice (bit-identical), against torch.scatter_reduce on the GPU"""
    from languagegroundedsemseg_amd.synthetic import make_batch
    coords_np, _, _ = make_batch(list(range(8)), voxel=0.02, n_target=150000)
    coords = torch.from_numpy(coords_np).to(DEV)
    n, c = coords.shape[0], 96
    assert n > 1_000_000
    feats = torch.randn(n, c, device=DEV).to(torch.bfloat16)
    dy_seed = 5

    def once():
        f = feats.clone().requires_grad_(True)
        x = ME.SparseTensor(f, coords)
        mgr = x.coordinate_manager
        n1 = mgr.size(mgr.coarser_key(x.coordinate_map_key, 2))
        g = torch.Generator(device=DEV).manual_seed(dy_seed)
        dy1 = torch.randn(n1, c, generator=g, device=DEV).to(torch.bfloat16)
        dy2 = torch.randn(8, c, generator=g, device=DEV).to(torch.bfloat16)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            mx = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
            sm = ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3)(x)
            gp = ME.MinkowskiGlobalAvgPooling()(x)
            loss = (mx.F.float() * dy1.float()).sum() + (sm.F.float() * dy1.float()).sum() + (gp.F.float() * dy2.float()).sum()
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return x, mx, sm, gp, f.grad, dy1, dy2

    x, mx, sm, gp, grad, dy1, dy2 = once()
    x2, mx2, sm2, gp2, grad2, _, _ = once()
    for a, b in ((mx.F, mx2.F), (sm.F, sm2.F), (gp.F, gp2.F), (grad, grad2)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # reference on the GPU: cell index of every row, torch.scatter_reduce
    C = x.C
    uniq, idx = torch.unique(torch.cat([C[:, :1], torch.div(C[:, 1:], 2, rounding_mode="floor") * 2], 1).to(torch.int64),
                             dim=0, return_inverse=True)
    rix = _match(mx.C, uniq)
    m = uniq.shape[0]
    fd = feats.double()
    ix = idx.view(-1, 1).expand(-1, c)
    rmax = torch.full((m, c), -float("inf"), dtype=torch.float64, device=DEV).scatter_reduce(0, ix, fd, "amax")[rix]
    assert torch.equal(mx.F.double(), rmax)
    rsum = torch.zeros(m, c, dtype=torch.float64, device=DEV).scatter_reduce(0, ix, fd, "sum")[rix]
    r = rsum.float().to(torch.bfloat16).double()
    assert bool(((sm.F.double() - r).abs() <= _bf16_ulp(r)).all())
    _, bidx = torch.unique(C[:, 0].to(torch.int64), return_inverse=True)
    bx = bidx.view(-1, 1).expand(-1, c)
    ravg = torch.zeros(8, c, dtype=torch.float64, device=DEV).scatter_reduce(0, bx, fd, "mean", include_self=False)
    r = ravg.float().to(torch.bfloat16).double()
    assert bool(((gp.F.double() - r).abs() <= _bf16_ulp(r)).all())
    # gradient: sum part copies dy1, max part routes dy1 to the arg-max rows, global avg adds dy2 / count
    inv = torch.empty_like(rix)
    inv[rix] = torch.arange(m, device=DEV)
    dyr = dy1.double()[inv]
    want = dyr[idx] + max_backward(dyr, max_argrow(fd, idx, m), n) + (dy2.double() / torch.bincount(bidx).view(-1, 1))[bidx]
    assert float((grad.double() - want).abs().max() / want.abs().max()) < 2e-2


@PARITY
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_misaligned_column_slice_takes_the_element_path_and_gives_the_same_bits(dtype):
    """the one alignment rule of the three entry points (csrc/lgs_rows.h rows_ok): x as a column slice of a wider buffer whose
    row stride is not a multiple of 16 bytes and whose start is misaligned goes through one-element accesses, the same data
    contiguous through 16-byte ones.  About 1 400 rows in 2 scenes, c = 8: the origin map reduces in two passes (a scene holds
    more than 512 rows), the stride-2 map in one.  Both meet the float64 reference, and -- the accumulation order does not
    depend on the access width -- each other bit for bit (but for the fp32 sum of products, see below)."""
    coords = _scene(61, n=1400, span=12)
    n, c = coords.shape[0], 8
    x0 = ME.SparseTensor(torch.zeros(n, 1, device=DEV), coords.to(DEV))
    mgr, k0 = x0.coordinate_manager, x0.coordinate_map_key
    be = ME.get_backend()
    g = torch.Generator(device=DEV).manual_seed(9)
    wide = torch.randn(n, c + 5, generator=g, device=DEV).to(dtype)
    wide2 = torch.randn(n, c + 5, generator=g, device=DEV).to(dtype)
    xs, x2s = wide[:, 3:3 + c], wide2[:, 3:3 + c]                 # case A: row stride 13 elements, start 3 elements in
    xc, x2c = xs.contiguous(), x2s.contiguous()                   # case B
    es = wide.element_size()
    assert (xs.stride(0) * es) % 16 != 0 and xs.data_ptr() % 16 != 0 and xc.data_ptr() % 16 == 0 and (c * es) % 16 == 0
    _, bidx = batches(x0.C.cpu())
    uniq, cidx = cells(x0.C.cpu(), 2)
    k1 = mgr.coarser_key(k0, 2)
    rix = _match(mgr.get_coordinates(k1).cpu(), uniq)
    for coarse_key, idx, order in ((mgr.origin_key(), bidx, None), (k1, cidx, rix)):
        sm = mgr.segment_map_handle(k0, coarse_key)
        idx = idx.to(DEV)
        m = sm.n_coarse
        assert (int(torch.bincount(idx).max()) > 512) == (order is None)      # two passes on the origin map, one on the stride-2 map
        take = (lambda t: t) if order is None else (lambda t: t[order.to(DEV)])
        cnt = take(torch.bincount(idx, minlength=m))
        fd, f2d = xc.double(), x2c.double()
        for op in ("sum", "avg", "max", "prod"):
            a, arg_a = be.pool_reduce(sm, op, xs, x2s if op == "prod" else None)
            b, arg_b = be.pool_reduce(sm, op, xc, x2c if op == "prod" else None)
            src = fd * f2d if op == "prod" else fd
            ref = take(seg_reduce(src, idx, m, "sum" if op == "prod" else op))
            for h in (a, b):
                if op == "max":
                    assert torch.equal(h.double(), ref)
                else:
                    abs_sum = take(seg_reduce(src.abs(), idx, m, "sum"))
                    _check_sum_like(h, ref, abs_sum / (cnt.view(-1, 1) if op == "avg" else 1), cnt)
            # fp32 sum of products: the compiler contracts v * w + acc into an FMA in some places of the unrolled loop and not in
            # others, differently per access width (the ISA of k_seg_reduce<float, VEC, 3, PART> shows it), so the two widths may
            # differ in the last bit there -- it holds to the reference bound only; bf16 products are exact in fp32 either way
            if not (op == "prod" and dtype == torch.float32):
                assert torch.equal(a, b), op
            if op == "max":
                assert torch.equal(arg_a, arg_b)
        gsrc = torch.randn(m, c, generator=g, device=DEV).to(dtype)
        ya, yb = be.pool_broadcast(sm, "add", gsrc, xs), be.pool_broadcast(sm, "add", gsrc, xc)
        inv = torch.arange(m, device=DEV) if order is None else torch.empty_like(order.to(DEV)).scatter_(0, order.to(DEV), torch.arange(m, device=DEV))
        want = (fd + gsrc.double()[inv[idx]]).float().to(dtype)       # one rounding of an exact fp64 result (test_broadcast_ops)
        assert torch.equal(ya, want) and torch.equal(yb, want)
