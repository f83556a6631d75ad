"""Strided and dilated 3^3 convolutions without a GPU: the module surface, the new export, the strided conv on the oracle backend
against a dense conv3d, deferred against immediate execution, the ResNet manifests, and the launch plans of the new maps held
through the debug plan queries (synthetic views, no HIP call)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
from helpers import Cfg, deterministic_init
from oracle.backend import OracleBackend

HERE = os.path.dirname(os.path.abspath(__file__))
F32, BF16 = 0, 1


@pytest.fixture()
def oracle_backend():
    prev = ME.set_backend(OracleBackend("torch"))
    yield
    ME.set_backend(prev)


# ------------------------------------------------------------------------------------------- module surface
@pytest.mark.parametrize("cls", [ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose])
def test_the_new_configurations_construct(cls):
    for ks, st, dil in ((3, 2, 1), (1, 2, 1), (3, 1, 2), (3, 1, 4)):
        m = cls(8, 16, kernel_size=ks, stride=st, dilation=dil, dimension=3)
        assert tuple(m.kernel.shape) == (ks ** 3, 8, 16)
        kg = ME.KernelGenerator(kernel_size=ks, stride=st, dilation=dil, dimension=3)
        g = cls(8, 16, kernel_generator=kg, dimension=3)
        assert (g.kernel_size[0], g.stride[0], g.dilation[0]) == (ks, st, dil) and g.kernel.shape == m.kernel.shape
    for kw in (dict(kernel_size=3, stride=2, dilation=2), dict(kernel_size=5, stride=1), dict(kernel_size=3, stride=3),
               dict(kernel_size=[3, 3, 1], stride=1), dict(kernel_size=3, stride=[2, 2, 1]), dict(kernel_size=3, stride=1, dilation=[1, 2, 1]),
               dict(kernel_size=1, stride=1, dilation=2), dict(kernel_size=2, stride=2, dilation=2)):
        with pytest.raises(NotImplementedError):
            cls(8, 16, dimension=3, **kw)
        with pytest.raises(NotImplementedError):
            cls(8, 16, dimension=3, kernel_generator=ME.KernelGenerator(dimension=3, **kw))


def test_the_library_exports_the_new_entry_point_at_abi_18():
    from languagegroundedsemseg_amd import build, engine
    build.build()
    assert "lgs_manager_kernel_map_ex" in engine.EXPORTS
    f = engine.lib().lgs_manager_kernel_map_ex
    assert len(f.argtypes) == 7
    assert engine.lib().lgs_abi_version() == engine.ABI_VERSION == 18


# ------------------------------------------------------------------------------------------- oracle backend: strided conv == dense conv3d
def _scene(seed, n=300, extent=12, batches=2):
    rng = np.random.default_rng(seed)
    c = np.concatenate([np.concatenate([np.full((n, 1), b), rng.integers(0, extent, (n, 3))], 1) for b in range(batches)])
    c = np.unique(c.astype(np.int32), axis=0)
    return c[rng.permutation(c.shape[0])]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_strided_conv_on_the_oracle_backend_equals_dense_conv3d(seed, oracle_backend):
    torch.manual_seed(seed)
    c = _scene(seed)
    conv = ME.MinkowskiConvolution(8, 16, kernel_size=3, stride=2, dimension=3)
    f = torch.randn(c.shape[0], 8, requires_grad=True)
    y = conv(ME.SparseTensor(f, torch.from_numpy(c)))
    g = torch.randn(y.F.shape[0], 16)
    y.F.backward(g)
    # dense restatement in float64: the sparse conv reads in[c_out + off * ts], off in {-1,0,1}^3, kernel offset index with the
    # first spatial axis fastest -> conv3d weight [co, ci, kz, ky, kx] on a [B, C, Z, Y, X] volume, stride 2, padding 1
    B, E = int(c[:, 0].max()) + 1, int(c[:, 1:].max()) + 2
    E += E % 2
    fd = f.detach().double().requires_grad_(True)
    dense = torch.zeros(B, 8, E, E, E, dtype=torch.float64)
    idx = (torch.from_numpy(c[:, 0]).long(), torch.from_numpy(c[:, 3]).long(), torch.from_numpy(c[:, 2]).long(), torch.from_numpy(c[:, 1]).long())
    dense = dense.permute(0, 2, 3, 4, 1).index_put(idx, fd).permute(0, 4, 1, 2, 3)
    w = conv.kernel.detach().double().reshape(3, 3, 3, 8, 16).permute(4, 3, 0, 1, 2)      # [kz, ky, kx, ci, co] -> [co, ci, kz, ky, kx]
    out = torch.nn.functional.conv3d(dense, w, stride=2, padding=1)
    oc = y.C.numpy()
    assert y.tensor_stride[0] == 2 and (oc[:, 1:] % 2 == 0).all()
    want_cells = {(b, x // 2 * 2, yy // 2 * 2, z // 2 * 2) for b, x, yy, z in c.tolist()}
    assert set(map(tuple, oc.tolist())) == want_cells
    oi = (torch.from_numpy(oc[:, 0]).long(), slice(None), torch.from_numpy(oc[:, 3] // 2).long(), torch.from_numpy(oc[:, 2] // 2).long(),
          torch.from_numpy(oc[:, 1] // 2).long())
    ref = out[oi]
    assert float((y.F.detach().double() - ref).abs().max()) < 1e-4
    (ref * g.double()).sum().backward()
    assert float((f.grad.double() - fd.grad).abs().max()) < 1e-4


def test_dilated_and_strided_1x1_need_the_engine(oracle_backend):
    c = torch.from_numpy(_scene(3))
    x = ME.SparseTensor(torch.randn(c.shape[0], 8), c)
    for kw in (dict(kernel_size=3, dilation=2), dict(kernel_size=1, stride=2)):
        with pytest.raises(NotImplementedError, match="oracle"):
            y = ME.MinkowskiConvolution(8, 8, dimension=3, **kw)(x)
            y.F


# ------------------------------------------------------------------------------------------- deferred == immediate
def test_a_strided_basic_block_runs_the_same_deferred_and_immediately(oracle_backend):
    from languagegroundedsemseg_amd import models
    from languagegroundedsemseg_amd.me import deferred
    c = torch.from_numpy(_scene(4, n=500, extent=16))
    f = torch.randn(c.shape[0], 8)

    def run(enabled):
        prev = deferred.ENABLED
        deferred.ENABLED = enabled
        try:
            torch.manual_seed(0)
            # the residual branch: a 2^3 stride-2 conv + norm (the 1x1 stride-2 map does not exist on the oracle backend)
            down = torch.nn.Sequential(ME.MinkowskiConvolution(8, 16, kernel_size=2, stride=2, dimension=3), ME.MinkowskiBatchNorm(16))
            blk = deterministic_init(models.BasicBlock(8, 16, downsample=down, stride=2), 7).train()
            x = ME.SparseTensor(f.clone().requires_grad_(True), c)
            y = blk(x)
            y.F.square().sum().backward()
            return y.C.numpy(), y.F.detach().numpy(), x.F.grad.numpy(), [p.grad.numpy() for p in blk.parameters()]
        finally:
            deferred.ENABLED = prev
    a, b = run(True), run(False)
    assert (a[0] == b[0]).all() and a[1].shape[0] < c.shape[0]
    assert np.abs(a[1] - b[1]).max() < 1e-5 and np.abs(a[2] - b[2]).max() < 1e-4
    for ga, gb in zip(a[3], b[3]):
        assert np.abs(ga - gb).max() <= 1e-4 * max(1.0, np.abs(gb).max())


# ------------------------------------------------------------------------------------------- models
MAN = json.load(open(os.path.join(HERE, "golden", "resnet_manifest.json")))


@pytest.mark.parametrize("name", ["ResNet14", "ResNet18", "ResNet34"])
def test_resnet_state_dict_matches_the_reference(name):
    from languagegroundedsemseg_amd.models import load_model
    m = load_model(name)(3, 200, Cfg())
    sd = m.state_dict()
    ref = MAN[name]["state_dict"]
    assert [k for k, _ in ref] == list(sd.keys())
    for k, shape in ref:
        assert list(sd[k].shape) == shape, k
    assert sum(p.numel() for p in m.parameters()) == MAN[name]["num_parameters"]
    first = m.layer3[0]
    assert first.conv1.stride[0] == 2 and first.conv1.kernel_size[0] == 3 and first.downsample[0].stride[0] == 2 and first.downsample[0].kernel_size[0] == 1

    # config.dilations reaches every 3^3 conv of a layer's blocks, the strided first one included (resnet_block.py:27), and stride 2
    # combined with dilation > 1 is outside the supported set: such a config is refused at construction, by name
    class Dil(Cfg):
        dilations = [1, 1, 2, 4]
    with pytest.raises(NotImplementedError, match=r"\(3, 2, 2\)"):
        load_model(name)(3, 200, Dil())
    from languagegroundedsemseg_amd.models import BasicBlock
    blk = BasicBlock(16, 16, dilation=2)
    assert blk.conv1.dilation[0] == 2 and blk.conv2.dilation[0] == 2 and blk.conv1.stride[0] == 1


# ------------------------------------------------------------------------------------------- plans of the new maps
SHAPES = [(64, 64), (64, 128), (128, 256), (256, 512), (3, 32)]
N_PADS = [256, 4096, 19712, 65536, 1200128]


def _views(kind, n_pad):
    """(ks, fwd, bwd) as lgs_manager_kernel_map_ex builds them; n_pad = padded rows of the COARSE map, ~3 fine rows per coarse row"""
    from languagegroundedsemseg_amd.engine import ConvPlanView as V
    n_c = n_pad - 100
    n_f = 3 * n_c
    fp = (n_f + 255) // 256 * 256
    if kind == "3^3 stride 2":      # coarse-stationary 27-slot view with n_in > n_out, and its fine-stationary counterpart
        return 3, V(n_pad, n_f, n_c, 27, 27, 1, 0, 1), V(fp, n_c, n_f, 27, 27, 1, 0, 1)
    assert kind == "1x1 stride 2"   # plain nbr (/ out_row) pairs on the KS = 1 path
    return 1, V(n_pad, n_f, n_c, 1, 1, 1, 0, 0), V(fp, n_c, n_f, 1, 1, 1, 0, 1)


def _regions_sound(info, names, ws, where):
    used = sorted(((n, getattr(info, n).offset, getattr(info, n).bytes) for n in names if getattr(info, n).bytes > 0), key=lambda r: r[1])
    for n, o, b in used:
        assert o % 256 == 0 and o >= 0 and o + b <= info.bytes_total <= ws, (where, n, o, b, info.bytes_total, ws)
    for (n0, o0, b0), (n1, o1, b1) in zip(used, used[1:]):
        assert o0 + b0 <= o1, (where, n0, n1)


@pytest.mark.parametrize("kind", ["3^3 stride 2", "1x1 stride 2"])
def test_plans_of_the_strided_maps_are_sound(kind):
    from languagegroundedsemseg_amd import build, engine
    build.build()
    L = engine.lib()
    for n_pad in N_PADS:
        ks, fwd, bwd = _views(kind, n_pad)
        for cin, cout in SHAPES:
            for dtype in (BF16, F32):
                for tr in (0, 1):
                    for op in (0, 1):
                        view = fwd if (op == 1) == (tr != 0) else bwd
                        for epi in (0, 1 if op == 0 else 2):
                            where = (kind, n_pad, cin, cout, dtype, tr, op, epi)
                            q = engine.ConvPlanQuery(fwd, bwd, ks, op, tr, cin, cout, dtype, epi)
                            info = engine.ConvPlanInfo()
                            engine.check(L.lgs_debug_conv_plan(ctypes.byref(q), ctypes.byref(info)))
                            assert info.path in (3, 4), where               # wide / gather: never a pointwise kernel on a table view
                            _regions_sound(info, ("packed", "padded_in", "scratch", "bias", "partials"), info.workspace_bytes, where)
                            assert info.workspace_bytes >= info.bytes_total > 0 and info.total * 16 <= info.packed.bytes, where
                            if info.path == 4:
                                assert info.grid_x * info.tm == view.n_pad and info.grid_y * info.wb >= info.nb_total, where
                                assert info.bn_rows in (0, info.grid_x), where
                            # the public queries agree with the plan
                            if op == 0 and epi == 1:
                                assert info.q_bn_partial_rows == info.bn_rows, where
                            if op == 1 and epi == 2:
                                assert info.q_can_accumulate == info.can_accumulate, where
                            pd = info.pack_desc
                            if pd.bytes:
                                assert (pd.bytes, pd.K, pd.ncp, pd.nbp, pd.mirror, pd.transposed) == (info.total * 16, ks ** 3, info.ncp, info.nbp, 0, op), where
                            else:
                                assert info.pad_input or info.scratch_out, where
                    # weight gradient: a strided 3^3 map never goes to the kernels that were only run on the stride-1 table
                    where = (kind, n_pad, cin, cout, dtype, tr, "wgrad")
                    q = engine.WgradPlanQuery(fwd, bwd, ks, tr, cin, cout, dtype, 0)
                    info = engine.WgradPlanInfo()
                    engine.check(L.lgs_debug_wgrad_plan(ctypes.byref(q), ctypes.byref(info)))
                    assert info.path == (3 if dtype == BF16 else 4), where          # pair list / fp32
                    assert info.bwd_view == tr and info.supports_stride == 0, where
                    _regions_sound(info, ("partials", "padded_in", "padded_gout"), info.workspace_bytes, where)
                    assert info.workspace_bytes >= info.bytes_total > 0, where
                    assert info.partials.bytes >= info.slots * ks ** 3 * info.pad_a * info.pad_b * 4 > 0, where
                    view = bwd if tr else fwd
                    e = 2 if dtype == BF16 else 4
                    assert info.padded_in.bytes >= view.n_in * info.pad_in * e and info.padded_gout.bytes >= view.n_out * info.pad_gout * e, where
