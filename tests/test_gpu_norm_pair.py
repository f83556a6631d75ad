"""The norms of a residual block on shared passes (csrc/lgs_norm.hip, knob BN_PAIR): lgs_bn_backward masks dy once, and
lgs_bn_forward_pair / lgs_bn_backward_pair run norm2 and the downsample-branch norm of
/root/reference/models/modules/resnet_block.py:41-57 + models/resnet.py:93-103 (out = relu?(norm2(conv2) + norm_d(conv_d(x)))) in
one statistics launch, one fold launch and one apply.

Every per-element expression and every summation order is the single kernels', so knob on and knob off (today's single calls, dy
masked in both launches) must agree BIT FOR BIT on every output -- y, res, dx*, dres, dgamma / dbeta, the saved statistics, the
running statistics and num_batches_tracked -- in bf16 and fp32, on both dual paths (`three`, `fold`, selected by the existing
knobs), at the smallest shapes at which these kernels can go wrong:
  n = 1 (fewer rows than one workgroup's slab), 127 / 128 (a ragged and an exact slab), 1037 (several slabs, a ragged last one and a
  tail in the unrolled loop), 70 001 (hundreds of workgroups; fp32 x 96 channels: more than one row per thread in the apply grid);
  c = 32 and 96 (4 / 8 and 12 / 24 channel groups per row: 96 leaves idle threads in a workgroup).
n = 0: the pair entry points do what the single calls do for an empty tensor (they hand the call to them).
One case per dtype and path is held against torch.nn.BatchNorm1d + autograd in fp64, to the tolerance tests/test_gpu_engine.py uses
for BatchNorm.  A downsample block and a plain block through lgs_block_forward / lgs_block_backward close the file.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
from helpers import small_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = {"three": dict(BN_FOLD=0, BN_FUSED=0), "fold": dict(BN_FOLD=1, BN_FOLD_MAX_MB=64)}
PAIR_KERNELS = {
    "three": {"k_colreduce_pair", "k_fold_fwd_pair", "k_bn_apply_pair", "k_fold_bwd_pair", "k_bn_bwd_apply_pair"},
    "fold": {"k_colreduce_pair", "k_bn_apply_pair", "k_bn_bwd_apply_pair"},
}


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def _norm_kernels(counts):
    return {re.match(r"\w+", k).group(0) for k in counts if k.startswith(("k_bn_", "k_colreduce", "k_fold_"))}


def _inputs(n, c, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n + c)
    d = {"xa": torch.randn(n, c, generator=g) * 2 + 0.5, "xb": torch.randn(n, c, generator=g) * 0.7 - 0.3,
         # the upstream gradient as a column slice of a wider buffer (the gradient of one ME.cat input), and contiguous
         "dy_wide": torch.randn(n, c + 32, generator=g),
         "ga": torch.rand(c, generator=g) + 0.5, "ba": torch.randn(c, generator=g) * 0.1,
         "gb": torch.rand(c, generator=g) + 0.5, "bb": torch.randn(c, generator=g) * 0.1}
    out = {k: v.to(DEV).to(dtype if k in ("xa", "xb", "dy_wide") else torch.float32) for k, v in d.items()}
    out["dy_slice"] = out["dy_wide"][:, 16:16 + c]
    out["dy"] = out["dy_slice"].contiguous()
    return out


def _bn(c):
    m = torch.nn.BatchNorm1d(c, momentum=0.1).to(DEV)
    with torch.no_grad():
        m.running_mean.fill_(0.25)
        m.running_var.fill_(1.5)
    return m


def _run_pair(t, c, relu, want_res, want_dres, dy_key):
    """forward + backward of the pair through the backend wrappers -> every output, as a dict of tensors"""
    be = ME.get_backend()
    na, nb = _bn(c), _bn(c)
    y, sta, stb, res = be.bn_forward_pair(t["xa"], na, t["ga"], t["ba"], t["xb"], nb, t["gb"], t["bb"], relu, want_res=want_res)
    dxa, dxb, dres, (dga, dba, dgb, dbb) = be.bn_backward_pair(t["xa"], y if relu else None, t["ga"], t["ba"], sta, 1 if relu else 0, t["xb"],
                                                                t["gb"], stb, t[dy_key], want_residual=want_dres)
    out = dict(y=y, sta=sta, stb=stb, dxa=dxa, dxb=dxb, dga=dga, dba=dba, dgb=dgb, dbb=dbb,
               rma=na.running_mean, rva=na.running_var, nbta=na.num_batches_tracked,
               rmb=nb.running_mean, rvb=nb.running_var, nbtb=nb.num_batches_tracked)
    if want_res:
        out["res"] = res
    if want_dres:
        out["dres"] = dres
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("path", ["three", "fold"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c", [32, 96])
@pytest.mark.parametrize("n", [1, 127, 128, 1037, 70001])
def test_pair_is_bitwise_the_two_single_calls(n, c, dtype, path):
    from languagegroundedsemseg_amd import engine
    t = _inputs(n, c, dtype)
    # (relu, res requested, dres requested, dy operand): relu mode 1 with and without dres, res with and without, dy strided and not
    for relu, want_res, want_dres, dy_key in [(True, False, False, "dy_slice"), (True, True, True, "dy"), (False, True, False, "dy"),
                                              (False, False, True, "dy_slice")]:
        with engine.tuning(BN_PAIR=0, **PATHS[path]):
            ref = _run_pair(t, c, relu, True, True, dy_key)            # the single calls always form both intermediates
        before = engine.dispatch_counts()
        with engine.tuning(BN_PAIR=1, **PATHS[path]):
            got = _run_pair(t, c, relu, want_res, want_dres, dy_key)
        hit = _norm_kernels(k for k, v in engine.dispatch_counts().items() if v > before.get(k, 0))
        assert hit == PAIR_KERNELS[path], (hit, path)
        for k, v in got.items():
            assert torch.equal(v, ref[k]), (k, n, c, dtype, path, relu, want_res, want_dres, dy_key)
        assert int(got["nbta"]) == 1 and int(got["nbtb"]) == 1


@pytest.mark.parametrize("path", ["three", "fold"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c", [32, 96])
@pytest.mark.parametrize("n", [1, 127, 128, 1037, 70001])
def test_single_backward_masks_dy_once_bitwise(n, c, dtype, path):
    """lgs_bn_backward, relu mode 1: with a dresidual output the reduce launch writes the masked gradient and the apply reads it back
    (knob on); without one nothing changes.  dx, dres, dgamma, dbeta equal the two-mask launches bit for bit."""
    from languagegroundedsemseg_amd import engine
    be = ME.get_backend()
    t = _inputs(n, c, dtype, seed=1)
    with engine.tuning(**PATHS[path]):
        y, st = be.bn_forward(t["xa"], t["ga"], t["ba"], 1e-5, 0.1, None, None, t["xb"], True)
        for want_res in (True, False):
            for dy_key in ("dy", "dy_slice"):
                outs = []
                for knob in (0, 1):
                    with engine.tuning(BN_PAIR=knob):
                        dx, dres, dg, db = be.bn_backward(t["xa"], y, t[dy_key], t["ga"], t["ba"], st, 1, want_res)
                        torch.cuda.synchronize()
                        outs.append([v.clone() for v in (dx, dg, db) + ((dres,) if want_res else ())])
                for a, b in zip(*outs):
                    assert torch.equal(a, b), (n, c, dtype, path, want_res, dy_key)
                if want_res:       # and the masked gradient is what it says it is
                    assert torch.equal(outs[1][3], torch.where(y > 0, t["dy"], torch.zeros_like(t["dy"])))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_empty_tensor_goes_to_the_single_calls(dtype):
    """n = 0: the pair entry points launch no pair kernel; they hand the call to the single norms, whose answer for an empty tensor
    (statistics 0 / 1 / sqrt(eps), running statistics, num_batches_tracked) is therefore also theirs"""
    from languagegroundedsemseg_amd import engine
    from languagegroundedsemseg_amd.me.backend_hip import _ptr, _stream
    L = engine.lib()
    c, code = 32, (engine.LGS_BF16 if dtype == torch.bfloat16 else engine.LGS_F32)
    outs = []
    for knob in (0, 1):
        na, nb = _bn(c), _bn(c)
        g, b = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
        x = torch.zeros(8, c, device=DEV, dtype=dtype)
        y, res = torch.zeros_like(x), torch.zeros_like(x)
        st = torch.full((2, 2 * c), -1.0, device=DEV)
        ws = torch.empty(L.lgs_bn_pair_workspace_bytes(0, c), dtype=torch.uint8, device=DEV)
        pa = engine.BnParams(_ptr(g), _ptr(b), _ptr(na.running_mean), _ptr(na.running_var), _ptr(na.num_batches_tracked), 1e-5, 0.1)
        pb = engine.BnParams(_ptr(g), _ptr(b), _ptr(nb.running_mean), _ptr(nb.running_var), _ptr(nb.num_batches_tracked), 1e-5, 0.1)
        before = engine.dispatch_counts()
        with engine.tuning(BN_PAIR=knob):
            engine.check(L.lgs_bn_forward_pair(_ptr(x), ctypes.byref(pa), _ptr(st[0]), _ptr(x), ctypes.byref(pb), _ptr(st[1]), 0, c, 1, _ptr(y), 0,
                                               _ptr(res), code, _ptr(ws), _stream()))
        torch.cuda.synchronize()
        hit = _norm_kernels(k for k, v in engine.dispatch_counts().items() if v > before.get(k, 0))
        assert not any(k.endswith("_pair") for k in hit), hit
        outs.append([v.clone() for v in (st, na.running_mean, na.running_var, na.num_batches_tracked, nb.running_mean, nb.running_var,
                                         nb.num_batches_tracked, y, res)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parity("plain torch: nn.BatchNorm1d + autograd in fp64")
@pytest.mark.parametrize("path", ["three", "fold"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 2e-2)])
def test_pair_matches_torch_batchnorm_fp64(dtype, tol, path):
    """y = relu(bn_a(xa) + stored(bn_b(xb))) and its gradients against two nn.BatchNorm1d in fp64 (tolerances of
    tests/test_gpu_engine.py::test_fused_bn_matches_torch: tol on outputs and statistics, 5 tol on gradients)"""
    from languagegroundedsemseg_amd import engine
    n, c = 5000, 96
    t = _inputs(n, c, dtype, seed=2)
    be = ME.get_backend()
    na, nb = _bn(c), _bn(c)
    ta, tb = torch.nn.BatchNorm1d(c, momentum=0.1).double(), torch.nn.BatchNorm1d(c, momentum=0.1).double()
    with torch.no_grad():
        for tm, hm, g, b in ((ta, na, "ga", "ba"), (tb, nb, "gb", "bb")):
            tm.weight.copy_(t[g].cpu()); tm.bias.copy_(t[b].cpu())
            tm.running_mean.copy_(hm.running_mean.cpu()); tm.running_var.copy_(hm.running_var.cpu())
    with engine.tuning(BN_PAIR=1, **PATHS[path]):
        y, sta, stb, res = be.bn_forward_pair(t["xa"], na, t["ga"], t["ba"], t["xb"], nb, t["gb"], t["bb"], True, want_res=True)
        dxa, dxb, dres, (dga, dba, dgb, dbb) = be.bn_backward_pair(t["xa"], y, t["ga"], t["ba"], sta, 1, t["xb"], t["gb"], stb, t["dy_slice"],
                                                                    want_residual=True)
    xa64 = t["xa"].double().cpu().requires_grad_(True)
    xb64 = t["xb"].double().cpu().requires_grad_(True)
    r64 = tb(xb64)
    r64.retain_grad()
    # the branch output is an intermediate STORED in `dtype` before it is added (the single calls materialise it, the pair rounds it
    # in registers): the reference adds the same stored value (straight-through for the gradient).  Without it ~100 of the
    # 480 000 bf16 outputs have |sum| below the branch's rounding step and the other sign, i.e. another ReLU mask.
    y64 = torch.relu(ta(xa64) + r64 + (r64.detach().to(dtype).double() - r64.detach()))
    y64.backward(t["dy"].double().cpu())
    f = lambda v: v.detach().double().cpu().numpy()
    assert rel_err(f(y), f(y64)) < tol
    assert rel_err(f(res), f(r64)) < tol
    assert rel_err(f(dres), f(r64.grad)) < tol
    for got, want in ((dxa, xa64.grad), (dxb, xb64.grad), (dga, ta.weight.grad), (dba, ta.bias.grad), (dgb, tb.weight.grad), (dbb, tb.bias.grad)):
        assert rel_err(f(got), f(want)) < tol * 5
    for hm, tm in ((na, ta), (nb, tb)):
        assert rel_err(f(hm.running_mean), f(tm.running_mean)) < max(tol, 1e-4)
        assert rel_err(f(hm.running_var), f(tm.running_var)) < max(tol, 1e-4)
        assert int(hm.num_batches_tracked) == int(tm.num_batches_tracked) == 1
    for st, x64 in ((sta, xa64), (stb, xb64)):
        assert rel_err(f(st[:c]), f(x64.mean(0))) < max(tol, 1e-4)
        assert rel_err(f(st[c:]), f(1.0 / torch.sqrt(x64.var(0, unbiased=False) + 1e-5))) < max(tol, 1e-4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("downsample", [True, False])
def test_block_is_bitwise_the_same_with_the_knob_off(monkeypatch, dtype, downsample):
    """one downsample block (128 -> 96, ~5000 rows) and one plain block (96 -> 96) through lgs_block_forward / lgs_block_backward:
    output, gradient of the input, the three weight gradients and all norm gradients, running statistics included"""
    from languagegroundedsemseg_amd import engine, models
    from languagegroundedsemseg_amd.me import backend_hip
    from helpers import deterministic_init
    monkeypatch.setattr(backend_hip, "_WGRAD_INLINE_BELOW", 1 << 30)        # weight gradients on the compute stream
    cin, planes = (128, 96) if downsample else (96, 96)
    coords = torch.from_numpy(small_scene(31, n=5000, extent=40)).to(DEV)
    feats = (torch.randn(coords.shape[0], cin, generator=torch.Generator().manual_seed(5)) * 1.5).to(DEV).to(dtype)
    gout = torch.randn(coords.shape[0], planes, generator=torch.Generator().manual_seed(6)).to(DEV).to(dtype)

    def run(knob):
        ds = None
        if downsample:
            ds = torch.nn.Sequential(ME.MinkowskiConvolution(cin, planes, kernel_size=1, stride=1, bias=False, dimension=3),
                                     ME.MinkowskiBatchNorm(planes, momentum=0.1))
        blk = deterministic_init(models.BasicBlock(cin, planes, downsample=ds, D=3), 3).to(DEV).train()
        be = ME.get_backend()
        calls0 = getattr(be, "block_calls", 0)
        with engine.tuning(BN_PAIR=knob):
            xf = feats.clone().requires_grad_(True)
            y = blk(ME.SparseTensor(xf, coords)).F
            y.backward(gout)
            torch.cuda.synchronize()
        assert getattr(be, "block_calls", 0) - calls0 == 2               # one engine call per direction
        out = {"y": y.detach().clone(), "gin": xf.grad.clone()}
        out.update({"grad " + k: p.grad.clone() for k, p in blk.named_parameters()})
        out.update({"buf " + k: b.clone() for k, b in blk.named_buffers()})
        return out

    a, b = run(1), run(0)
    assert len([k for k in a if k.startswith("grad ")]) == (9 if downsample else 6)
    for k in a:
        assert torch.equal(a[k], b[k]), k
