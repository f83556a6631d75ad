"""MinkowskiInstanceNorm on the engine (csrc/lgs_instnorm.hip) against the float64 reference of tests/instnorm_reference.py.

Tolerances.  No rigorous per-element bound of useful size exists for a mean over 10^3 - 10^5 fp32 terms, so the yardstick is the
error of the module's own torch lines (two passes, fp32, on a CPU copy of the same inputs) against the same reference:
E_torch = max |torch_fp32 - ref64|, per output (y, dx, dweight, dbias).  The engine's fp32 results must satisfy

    max |engine - ref64| <= K * E_torch + tiny          K = 4 for every case and output,  tiny = 4 fp32 ulps of max |ref|

K covers a different (chunked, fixed) summation order and nothing else.  It was fixed on the CPU before the first GPU run
(tests/test_instnorm_cpu.py::test_calibration_of_the_tolerance_factor) from a restatement of the kernels' order in fp32 torch --
deviations from the scene's first row, 512-row chunk items, 32-row runs summed sequentially in fp32, everything above in double.
Measured ratios restated / E_torch at the test sizes (6000 rows; y, dx, dweight, dbias):
    two scenes C=96 0.19 0.18 0.24 0.80 | absent indices C=32 0.27 0.19 0.31 1.03 | one scene C=3 0.13 0.12 0.06 0.19
    two scenes C=512 0.17 0.18 0.20 1.02 | cancellation (100 + N(0, 1)) C=96 0.02 0.07 0.02 0.72
worst 1.03 -> K = 4 (>= 2x the worst, <= 8).  A naive one-pass fp32 E[x^2] - E[x]^2 restatement misses the cancellation case by
366 x E_torch (1.15e-1 against 3.1e-4), i.e. by 90 x the bound: that case tests the statistics.
bf16 storage: one bf16 ulp of bf16_rne(ref) on top of the fp32 allowance (one rounding at the store), for y and dx; dweight and
dbias are fp32 in both modes.  For bf16 inputs E_torch is taken on the same bf16-representable values, widened to fp32.
"""
import pytest
import torch
import torch.nn as nn

import MinkowskiEngine as ME
import instnorm_reference as R
from test_instnorm_cpu import K, case_tensors, scene_coords, tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY = pytest.mark.parity("float64 torch instance-norm reference")
NEW_SITES = [("k_in_reduce", "kInFwd"), ("k_in_apply", "kInFwd"), ("k_in_reduce", "kInBwd"), ("k_in_apply", "kInBwd")]


def _level(coords, level):
    """-> (manager, key, coordinates [n, 4] on the CPU in the row order of that level's map)"""
    x0 = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), coords.to(DEV))
    mgr, key = x0.coordinate_manager, x0.coordinate_map_key
    if level:
        key = mgr.coarser_key(key, 2 ** level)
    return mgr, key, mgr.get_coordinates(key).cpu()


def _module(w, b):
    m = ME.MinkowskiInstanceNorm(w.numel()).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w.view(1, -1))
        m.bias.copy_(b.view(1, -1))
    return m


def _run(m, mgr, key, x, dy):
    """one forward + backward of the module -> (y, dx, dweight [C], dbias [C]) on the CPU"""
    m.zero_grad(set_to_none=True)
    f = x.to(DEV).requires_grad_(True)
    out = m(ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=mgr))
    assert out.coordinate_map_key == key and out.F.dtype == x.dtype and out.F.shape == x.shape
    out.F.backward(dy.to(DEV))
    return out.F.detach().cpu(), f.grad.cpu(), m.weight.grad.view(-1).cpu(), m.bias.grad.view(-1).cpu()


def _sites(counts):
    return [any(k in name and d in name for name in counts) for k, d in NEW_SITES]


def _check(got, x, lc, w, b, dy, what, k=K):
    """got = (y, dx, dweight, dbias) held to K * E_torch + tiny (+ one bf16 ulp for bf16 y and dx); prints every figure first"""
    xf, dyf = x.float(), dy.float()
    ref = R.reference(xf, lc, w, b, dyf)
    e_torch = [float((t.double() - r).abs().max()) for t, r in zip(R.torch_lines_all(xf, lc, w, b, dyf), ref)]
    fails = []
    for name, g, r, e in zip(("y", "dx", "dweight", "dbias"), got, ref, e_torch):
        allow = k * e + tiny(r)
        if g.dtype == torch.bfloat16:
            rb = r.float().to(torch.bfloat16).double()
            excess = (g.double() - rb).abs() - R.bf16_ulp(rb)
            err = float(excess.max()) if excess.numel() else 0.0
        else:
            assert g.dtype == torch.float32
            err = float((g.double() - r).abs().max()) if g.numel() else 0.0
        print("%s %s: error%s %.3e, E_torch %.3e, allowed %.3e" % (what, name, " beyond one bf16 ulp" if g.dtype == torch.bfloat16 else "",
                                                                  err, e, allow))
        if not err <= allow:
            fails.append((name, err, allow))
    assert not fails, (what, fails)
    return ref


@PARITY
@pytest.mark.parametrize("batch_ids", [(0, 1), (0, 2, 5), (3,)], ids=["two", "absent", "one"])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("c", [512, 96, 32, 20, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_backward_parity(dtype, c, level, batch_ids):
    seed = 100 * level + len(batch_ids)
    mgr, key, lc = _level(scene_coords(seed, batch_ids=batch_ids), level)
    x, w, b, dy = case_tensors(seed + c, lc.shape[0], c, dtype)
    got = _run(_module(w, b), mgr, key, x, dy)
    _check(got, x, lc, w, b, dy, "%s C=%d level %d ids %s" % (dtype, c, level, batch_ids))


@PARITY
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_single_voxel_scene_and_empty_tensor(dtype):
    coords = torch.cat([scene_coords(5, batch_ids=(0,)), torch.tensor([[3, 1, 2, 3]], dtype=torch.int32)])
    mgr, key, lc = _level(coords, 0)
    x, w, b, dy = case_tensors(5, lc.shape[0], 32, dtype)
    y, dx, dw, db = got = _run(_module(w, b), mgr, key, x, dy)
    _check(got, x, lc, w, b, dy, "single voxel %s" % dtype)
    assert torch.equal(y[-1].float(), b.view(-1).to(dtype).float())      # var = 0: y = bias
    assert float(dx[-1].abs().max()) == 0.0
    # an empty batch flows through
    e = ME.SparseTensor(torch.zeros(0, 32, device=DEV, dtype=dtype), torch.zeros(0, 4, dtype=torch.int32, device=DEV))
    m = _module(w, b)
    f = e.F.clone().requires_grad_(True)
    out = m(ME.SparseTensor(f, coordinate_map_key=e.coordinate_map_key, coordinate_manager=e.coordinate_manager))
    assert out.F.shape == (0, 32) and out.F.dtype == dtype
    out.F.sum().backward()
    assert f.grad.shape == (0, 32)
    assert m.weight.grad is not None and float(m.weight.grad.abs().sum()) == 0.0 and float(m.bias.grad.abs().sum()) == 0.0


@PARITY
def test_cancellation_case_offset_features():
    """features 100 + N(0, 1): what separates sums about a pivot from E[x^2] - mean^2 (the naive restatement misses this bound
    90-fold, tests/test_instnorm_cpu.py)"""
    mgr, key, lc = _level(scene_coords(15, batch_ids=(0, 1)), 0)
    x, w, b, dy = case_tensors(15, lc.shape[0], 96, offset=100.0)
    got = _run(_module(w, b), mgr, key, x, dy)
    _check(got, x, lc, w, b, dy, "cancellation")


def test_no_host_synchronisation():
    mgr, key, lc = _level(scene_coords(21), 0)
    x, w, b, dy = case_tensors(21, lc.shape[0], 96)
    m = _module(w, b)
    f = x.to(DEV).requires_grad_(True)
    g = dy.to(DEV)
    st = ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=mgr)
    m(st).F.backward(g)                       # warm-up: the segment map, the workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m(st).F.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_runs_are_bit_identical(dtype):
    mgr, key, lc = _level(scene_coords(22, n=40000, span=24, batch_ids=(0, 1, 4)), 0)
    x, w, b, dy = case_tensors(22, lc.shape[0], 96, dtype)
    m = _module(w, b)
    a = _run(m, mgr, key, x, dy)
    bb = _run(m, mgr, key, x, dy)
    for u, v in zip(a, bb):
        assert torch.equal(u, v)


def test_launch_sites_are_counted():
    from languagegroundedsemseg_amd import engine
    mgr, key, lc = _level(scene_coords(23), 0)
    x, w, b, dy = case_tensors(23, lc.shape[0], 32)
    m = _module(w, b)
    engine.dispatch_counts(reset=True)
    _run(m, mgr, key, x, dy)
    counts = engine.dispatch_counts()
    assert all(_sites(counts)), sorted(counts)


@PARITY
def test_the_knob_selects_the_torch_lines_on_a_live_module():
    from languagegroundedsemseg_amd import engine
    mgr, key, lc = _level(scene_coords(24), 0)
    x, w, b, dy = case_tensors(24, lc.shape[0], 32)
    m = _module(w, b)
    _run(m, mgr, key, x, dy)
    with engine.tuning(INSTANCE_NORM=0):
        engine.dispatch_counts(reset=True)
        got = _run(m, mgr, key, x, dy)
        assert not any(_sites(engine.dispatch_counts())), sorted(engine.dispatch_counts())
        _check(got, x, lc, w, b, dy, "INSTANCE_NORM=0")
    engine.dispatch_counts(reset=True)
    got = _run(m, mgr, key, x, dy)
    assert all(_sites(engine.dispatch_counts()))
    _check(got, x, lc, w, b, dy, "INSTANCE_NORM back to 1")


# ------------------------------------------------------------------------------------------ the reference's call sites
class _INBN(nn.Module):
    """NormType.INSTANCE_BATCH_NORM (models/modules/common.py): instance norm, then BatchNorm"""

    def __init__(self, c):
        super().__init__()
        self.norm = nn.Sequential(ME.MinkowskiInstanceNorm(c), ME.MinkowskiBatchNorm(c))

    def forward(self, x):
        return self.norm(x)


class _BlockIN(nn.Module):
    """BasicBlockIN (models/modules/resnet_block.py) spelled with ME calls"""

    def __init__(self, c):
        super().__init__()
        self.conv1 = ME.MinkowskiConvolution(c, c, kernel_size=3, dimension=3)
        self.norm1 = ME.MinkowskiInstanceNorm(c)
        self.conv2 = ME.MinkowskiConvolution(c, c, kernel_size=3, dimension=3)
        self.norm2 = ME.MinkowskiInstanceNorm(c)
        self.relu = ME.MinkowskiReLU(inplace=True)

    def forward(self, x):
        residual = x
        out = self.conv1(x)
        out = self.norm1(out)
        out = self.relu(out)
        out = self.conv2(out)
        out = self.norm2(out)
        out += residual
        out = self.relu(out)
        return out


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _call_site(cls, c, coords, x, dy, device, init):
    torch.manual_seed(0)
    m = cls(c)
    m.load_state_dict(init)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(device).train()
    f = x.to(device).requires_grad_(True)
    out = m(ME.SparseTensor(f, coords.to(device)))
    c4 = out.C.cpu().to(torch.int64)
    order = torch.argsort(((c4[:, 0] * 64 + c4[:, 1] + 32) * 64 + c4[:, 2] + 32) * 64 + c4[:, 3] + 32)   # rows by coordinate
    assert torch.equal(c4[order], coords.to(torch.int64)[torch.argsort(((coords[:, 0].long() * 64 + coords[:, 1] + 32) * 64
                                                                         + coords[:, 2] + 32) * 64 + coords[:, 3] + 32)])
    out.F.backward(dy.to(device))
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    return out.F.detach().cpu()[order], None, f.grad.cpu(), grads, state


@PARITY
@pytest.mark.parametrize("cls", [_INBN, _BlockIN], ids=["instance_batch_norm", "basic_block_in"])
def test_reference_call_sites_deferred_on_off_and_against_the_oracle(cls):
    """The gradient bar is DESIGN.md section 2's: rel-L2 over ALL parameters, 1e-2 (the bar is not per tensor there either).  It
    has to be: a BatchNorm removes any per-channel scale and shift of its input, so in INSTANCE_BATCH_NORM the true gradients of the
    instance norm's weight and bias are zero (up to BatchNorm's eps) and both backends return round-off noise for them -- measured
    per-tensor 'errors' of 9.5e-3 and 4.2e-1 on noise, next to 3e-7 / 5e-7 for the BatchNorm's own parameters."""
    from languagegroundedsemseg_amd.me import deferred
    from oracle.backend import OracleBackend
    c = 32
    coords = scene_coords(31, batch_ids=(0, 1, 2))
    g = torch.Generator().manual_seed(31)
    x = torch.randn(coords.shape[0], c, generator=g)
    dy = torch.randn(coords.shape[0], c, generator=g)
    # parameters away from their initial values (weight 1, bias 0 would hide a swapped or missing affine)
    torch.manual_seed(0)
    init = cls(c).state_dict()
    for k_, v in init.items():
        if v.dtype.is_floating_point and ("weight" in k_ or "bias" in k_) and "running" not in k_:
            v.add_(0.3 * torch.randn(v.shape, generator=g))

    def hip(flag):
        was = deferred.ENABLED
        deferred.ENABLED = flag
        try:
            return _call_site(cls, c, coords, x, dy, DEV, init)
        finally:
            deferred.ENABLED = was

    on, off = hip(True), hip(False)
    prev = ME.set_backend(OracleBackend("torch"))
    try:
        ora = _call_site(cls, c, coords, x, dy, "cpu", init)
    finally:
        ME.set_backend(prev)
    # the two execution modes: fp32 round-off
    d_out = float((on[0] - off[0]).abs().max())
    d_g = max(_rel_l2(on[3][n], off[3][n]) for n in on[3])
    print("%s deferred on vs off: outputs %.2e, parameter gradients rel-L2 %.2e" % (cls.__name__, d_out, d_g))
    assert d_out <= 1e-5 and _rel_l2(on[2], off[2]) <= 1e-5 and d_g <= 1e-5
    # against the CPU oracle backend (oracle convolutions, the unchanged torch lines for the instance norm)
    for name, r in (("deferred", on), ("call by call", off)):
        e_out = float((r[0] - ora[0]).abs().max())
        e_g = {n: _rel_l2(r[3][n], ora[3][n]) for n in ora[3]}          # printed per tensor, judged over all parameters
        tot = (sum(float((r[3][n].double() - ora[3][n].double()).norm()) ** 2 for n in ora[3])
               / sum(float(ora[3][n].double().norm()) ** 2 for n in ora[3])) ** 0.5
        print("%s %s vs oracle: outputs %.2e, dx rel-L2 %.2e, all-parameter gradient rel-L2 %.2e, per tensor %s" % (
            cls.__name__, name, e_out, _rel_l2(r[2], ora[2]), tot, {n: "%.1e" % v for n, v in e_g.items()}))
        assert e_out <= 1e-3
        assert tot <= 1e-2 and _rel_l2(r[2], ora[2]) <= 1e-2, (tot, e_g)


@PARITY
def test_a_state_dict_saved_before_the_change_loads_and_is_used():
    c = 20
    g = torch.Generator().manual_seed(9)
    saved = {"weight": 0.5 + torch.rand(1, c, generator=g), "bias": torch.randn(1, c, generator=g)}
    m = ME.MinkowskiInstanceNorm(c)
    assert m.load_state_dict(saved, strict=True).missing_keys == []
    m = m.to(DEV)
    mgr, key, lc = _level(scene_coords(9), 0)
    x, _, _, dy = case_tensors(9, lc.shape[0], c)
    got = _run(m, mgr, key, x, dy)
    _check(got, x, lc, saved["weight"], saved["bias"], dy, "state dict")
