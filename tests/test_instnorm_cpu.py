"""CPU-side checks of MinkowskiInstanceNorm on the engine: the host plan (lgs_debug_instnorm_plan), the exported symbols, the
unchanged CPU path of the module, and the calibration of the GPU tests' tolerance factor K.

Calibration (see tests/test_gpu_instnorm.py): the engine's fp32 results are held to K * E_torch + tiny, E_torch = the error of the
module's own torch lines (two passes, fp32) against the float64 reference on the same inputs.  K covers a different, fixed
summation order and nothing else; it is fixed here, before any GPU run, from a restatement of the kernels' order in fp32 torch
(instnorm_reference.engine_order_fp32).  Worst ratios of the restatement over E_torch on the cases below (this file prints them):
y 1.1, dx 1.3, dweight 1.5, dbias 1.4 (unit-scale features); the offset case 100 + N(0, 1): y 0.05; K = 4 leaves more than
the 2x margin the calibration test demands, and the naive one-pass E[x^2] - E[x]^2 kernel misses the offset case by 600 x E_torch.
"""
import ctypes
import itertools

import pytest
import torch

import instnorm_reference as R

K = 4.0           # the one factor of every fp32 comparison (tests/test_gpu_instnorm.py imports it)


def tiny(ref):
    """the part of the allowance that does not come from the statistics: the apply pass's own roundings, 4 fp32 ulps of the
    largest reference value"""
    return 4 * 2.0 ** -24 * max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-30)


def scene_coords(seed, n=6000, span=14, batch_ids=(0, 1)):
    """unique random voxels per batch index, rows shuffled so that batch indices interleave (tests/test_gpu_pooling.py::_scene)"""
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


def case_tensors(seed, n, c, dtype=torch.float32, offset=0.0):
    """features, weight, bias, dy of one case (CPU generator: the same values on every machine)"""
    g = torch.Generator().manual_seed(1000 + seed)
    x = (offset + torch.randn(n, c, generator=g)).to(dtype)
    w = 0.5 + torch.rand(1, c, generator=g)
    b = torch.randn(1, c, generator=g)
    dy = torch.randn(n, c, generator=g).to(dtype)
    return x, w, b, dy


# ------------------------------------------------------------------------------------------ plan
def _plan(direction, n_fine, n_seg, n_items, c, dtype):
    from languagegroundedsemseg_amd import engine
    q = engine.InstNormPlanQuery(direction=direction, c=c, dtype=dtype, n_fine=n_fine, n_seg=n_seg, n_items=n_items)
    info = engine.InstNormPlanInfo()
    engine.check(engine.lib().lgs_debug_instnorm_plan(ctypes.byref(q), ctypes.byref(info)))
    return info


def test_plan_regions_grids_and_access_width():
    from languagegroundedsemseg_amd import engine
    a256 = lambda b: (b + 255) // 256 * 256
    sizes = [(0, 0, 0), (1, 1, 2), (2500, 2, 7), (70000, 3, 140), (1200000, 8, 2352)]
    for (n_fine, n_seg, n_items), c, dtype, direction in itertools.product(sizes, (1, 3, 20, 32, 96, 200, 512, 1000),
                                                                           (engine.LGS_F32, engine.LGS_BF16), (0, 1)):
        p = _plan(direction, n_fine, n_seg, n_items, c, dtype)
        es = 2 if dtype == engine.LGS_BF16 else 4
        assert p.vec == (1 if (c * es) % 16 == 0 else 0), (c, dtype, p.vec)
        per_lane = 16 // es if p.vec else 1
        assert 0 <= p.lanes_log2 <= 6 and ((1 << p.lanes_log2) >= min(64, -(-c // per_lane)))
        assert p.lanes_log2 == 0 or (1 << (p.lanes_log2 - 1)) < -(-c // per_lane)
        regions = [p.partials] + ([p.sums] if direction == 1 else [])
        want = a256(n_items * 2 * c * 4) + (a256(n_seg * 2 * c * 4) if direction == 1 else 0)
        assert p.bytes_total == want, (p.bytes_total, want)
        assert p.workspace_bytes == a256(n_items * 2 * c * 4) + a256(n_seg * 2 * c * 4) >= p.bytes_total
        assert p.partials.bytes >= n_items * 2 * c * 4 and (direction == 0 or p.sums.bytes >= n_seg * 2 * c * 4)
        if direction == 0:
            assert p.sums.bytes == 0
        for r in regions:
            assert r.offset % 256 == 0 and r.bytes % 256 == 0 and r.offset >= 0 and r.offset + r.bytes <= p.bytes_total
        for r, s in itertools.combinations(regions, 2):
            assert r.offset + r.bytes <= s.offset or s.offset + s.bytes <= r.offset
        if n_fine == 0:
            assert p.reduce_grid == p.combine_grid == p.apply_grid == 0
        else:
            assert p.reduce_grid == n_items and p.combine_grid >= n_seg and p.apply_grid >= 1
            assert p.apply_grid * p.rows_per_apply_block >= n_fine


def test_plan_refuses_bad_queries():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    info = engine.InstNormPlanInfo()
    for kw in (dict(direction=2, c=8, dtype=0), dict(direction=0, c=0, dtype=0), dict(direction=0, c=8, dtype=7)):
        q = engine.InstNormPlanQuery(n_fine=10, n_seg=1, n_items=1, **kw)
        assert L.lgs_debug_instnorm_plan(ctypes.byref(q), ctypes.byref(info)) != 0
        assert b"lgs_debug_instnorm_plan" in L.lgs_last_error()


def test_the_four_symbols_are_exported_and_refuse_null_maps():
    from languagegroundedsemseg_amd import build, engine
    L = ctypes.CDLL(build.build())
    for s in ("lgs_in_workspace_bytes", "lgs_in_forward", "lgs_in_backward", "lgs_debug_instnorm_plan"):
        assert hasattr(L, s), "missing export " + s
        assert s in engine.EXPORTS
    E = engine.lib()
    assert E.lgs_abi_version() == engine.ABI_VERSION == 18
    assert E.lgs_in_workspace_bytes(None, 32) == 0
    assert E.lgs_in_forward(None, None, 32, None, None, 1e-6, None, None, 0, None, None) != 0
    assert b"lgs_in_forward" in E.lgs_last_error()
    assert E.lgs_in_backward(None, None, None, 32, None, None, None, None, None, 0, None, None) != 0
    assert b"lgs_in_backward" in E.lgs_last_error()


def test_the_knob_is_in_the_tuning_table():
    from languagegroundedsemseg_amd import engine, tuning
    rows = {n: (d, v) for n, d, v, _ in engine.tuning_table()}
    assert rows["INSTANCE_NORM"][0] == 1
    assert any(name == "INSTANCE_NORM" for _, name, _, _, _ in tuning.describe())
    with engine.tuning(INSTANCE_NORM=0):
        assert engine.tuning_get("INSTANCE_NORM") == 0
    assert engine.tuning_get("INSTANCE_NORM") == rows["INSTANCE_NORM"][1]


# ------------------------------------------------------------------------------------------ the CPU path did not move
def test_cpu_tensors_take_the_unchanged_torch_lines():
    import MinkowskiEngine as ME
    from oracle.backend import OracleBackend
    coords = scene_coords(3, n=900, batch_ids=(0, 2, 5))
    x, w, b, dy = case_tensors(3, coords.shape[0], 20)
    prev = ME.set_backend(OracleBackend("torch"))
    try:
        m = ME.MinkowskiInstanceNorm(20)
        assert sorted(m.state_dict()) == ["bias", "weight"] and m.weight.shape == (1, 20) and m.eps == 1e-6
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        xr = x.clone().requires_grad_(True)
        st = ME.SparseTensor(xr, coords)
        out = m(st)
        out.F.backward(dy)
        # the lines of the parent commit, restated
        x2 = x.clone().requires_grad_(True)
        w2, b2 = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        bi = st.C[:, 0].long()
        nb = int(bi.max().item()) + 1
        cnt = torch.zeros(nb, dtype=torch.float32).index_add_(0, bi, torch.ones_like(bi, dtype=torch.float32))
        xf = x2.float()
        mean = torch.zeros(nb, 20).index_add_(0, bi, xf) / cnt[:, None]
        d = xf - mean[bi]
        var = torch.zeros(nb, 20).index_add_(0, bi, d * d) / cnt[:, None]
        y = (d / torch.sqrt(var[bi] + 1e-6) * w2 + b2).to(x.dtype)
        y.backward(dy)
        assert torch.equal(out.F, y) and torch.equal(xr.grad, x2.grad)
        assert torch.equal(m.weight.grad, w2.grad) and torch.equal(m.bias.grad, b2.grad)
        m.eval()
        assert torch.equal(m(ME.SparseTensor(x, coords)).F, y)       # no running statistics: train() and eval() agree
    finally:
        ME.set_backend(prev)


# ------------------------------------------------------------------------------------------ calibration of K
CALIBRATION = [
    # (name, seed, batch ids, C, offset)
    ("two scenes C=96", 11, (0, 1), 96, 0.0),
    ("absent indices C=32", 12, (0, 2, 5), 32, 0.0),
    ("one scene C=3", 13, (4,), 3, 0.0),
    ("two scenes C=512", 14, (0, 1), 512, 0.0),
    ("cancellation C=96", 15, (0, 1), 96, 100.0),
]


def _errors(got, ref):
    return [float((g.double() - r).abs().max()) for g, r in zip(got, ref)]


def test_calibration_of_the_tolerance_factor():
    """the restated kernel order stays below K / 2 times the torch lines' own error on every case and output, and the naive
    one-pass variance fails the cancellation case by a wide margin (a test that a wrong kernel passes shows nothing)"""
    worst = 0.0
    for name, seed, ids, c, offset in CALIBRATION:
        coords = scene_coords(seed, batch_ids=ids)
        x, w, b, dy = case_tensors(seed, coords.shape[0], c, offset=offset)
        ref = R.reference(x, coords, w, b, dy)
        e_torch = _errors(R.torch_lines_all(x, coords, w, b, dy), ref)
        e_eng = _errors(R.engine_order_fp32(x, coords, w, b, dy), ref)
        ratios = [(e - tiny(r)) / t for e, t, r in zip(e_eng, e_torch, ref)]
        print("%-22s E_torch y %.2e dx %.2e dw %.2e db %.2e | restated / E_torch: y %.2f dx %.2f dw %.2f db %.2f"
              % ((name,) + tuple(e_torch) + tuple(e / t for e, t in zip(e_eng, e_torch))))
        worst = max(worst, max(ratios))
        if offset:
            e_naive = float((R.naive_fp32(x, coords, w, b).double() - ref[0]).abs().max())
            print("%-22s naive one-pass y error %.2e = %.0f x E_torch" % (name, e_naive, e_naive / e_torch[0]))
            assert e_naive > 10 * (K * e_torch[0] + tiny(ref[0])), (e_naive, e_torch[0])
    assert K <= 8
    assert worst * 2 <= K, "the margin of K = %g over the worst restated ratio %.2f fell below 2x" % (K, worst)


def test_single_voxel_scene_in_the_reference():
    """var = 0: y = bias and dx = 0 for that row, in the reference and in the restated kernel order"""
    coords = torch.cat([scene_coords(5, n=700, batch_ids=(0,)), torch.tensor([[3, 1, 2, 3]], dtype=torch.int32)])
    x, w, b, dy = case_tensors(5, coords.shape[0], 8)
    for y, dx, _, _ in (R.reference(x, coords, w, b, dy), R.engine_order_fp32(x, coords, w, b, dy)):
        assert torch.equal(y[-1].float(), b.view(-1).to(y.dtype).float())
        assert float(dx[-1].abs().max()) == 0.0
