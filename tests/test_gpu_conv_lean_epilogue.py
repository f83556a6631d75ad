"""k_conv_gather without the BatchNorm statistics epilogue (CONV_LEAN_EPI) computes what the instance with it computes.

A launch that writes no statistics runs, on the bf16 big-map tiles, an instance built without the epilogue (tile 7: 204 -> 137 / 147
registers, three workgroups per CU; its 3-chunk walk with one weight slab in LDS); CONV_LEAN_EPI=0 runs the instance with it, the
kernel as it was.  Tile 7 takes the lean instances on grids above 512 workgroups, with the knob at 2 on every grid.  Same
chunks, same order, same MFMAs, same stores: every case compares knob 1 against knob 0 BIT FOR BIT, in bf16 -- forward, dgrad and the
accumulating dgrad into a non-zero tensor.  SMALL_CFG=7 puts tile 7 on one small map (2 750 voxels: a ragged last 128-row tile, a
64-row group of padding only, isolated voxels whose 32-row blocks have no neighbour at most offsets); each shape runs there with the
slot split (fp32 partial images) and without it (the bf16 store epilogue).  One case runs the 96 -> 128 dgrad on a map of 65 536 + 37
voxels, where the plan picks tile 7 by itself.  The launch sites name tile and walk and are the same for both instances; the counter
"k_conv_gather:no_statistics_epilogue" says which ran.  A launch WITH statistics runs the same instance under
both knob values: its partial rows and output are compared bitwise too, and the partial rows against float64 column sums of the
stored output at the tolerance of test_conv_epilogue_batchnorm_statistics_equal_the_column_reduction (tests/test_gpu_parity_r2.py)."""
import ctypes

import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
from languagegroundedsemseg_amd import engine
from helpers import GATHER_LEAN_COUNTER as LEAN, GATHER_TILES
from test_gpu_map_build import _slab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T2, T7 = GATHER_TILES[2], GATHER_TILES[7]


class Map:
    def __init__(self, coords):
        self.x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), torch.from_numpy(np.ascontiguousarray(coords)).to(DEV))
        mgr, key = self.x.coordinate_manager, self.x.coordinate_map_key
        self.n = coords.shape[0]
        self.km = {3: mgr.kernel_map_handle(key, key, 3), 1: mgr.kernel_map_handle(key, key, 1)}


@pytest.fixture(scope="module")
def small():
    """2 550 voxels of a slab + 200 isolated voxels on a lattice of pitch 4 (no neighbour but themselves): 2 750 rows, 2 816 padded"""
    dense = _slab(5, 2550, 16, thick=4, batches=1)
    g = np.arange(200)
    lone = np.stack([np.zeros(200, np.int64), 100 + 4 * (g % 8), 100 + 4 * (g // 8 % 8), 100 + 4 * (g // 64)], 1).astype(np.int32)
    m = Map(np.concatenate([dense, lone], 0))
    assert m.n == 2750 and m.n % 128 != 0 and (m.n + 255) // 256 * 256 - m.n >= 64
    nbr, _, mask = m.km[3].tables(False)
    deg = (nbr.cpu().numpy() >= 0).sum(0)[:m.n]
    assert (deg == 1).sum() >= 200 and int(mask.cpu().numpy()[-1]) == 0          # isolated rows; a group of padding only
    return m


@pytest.fixture(scope="module")
def big():
    m = Map(_slab(77, 65536 + 37, 32, thick=64, batches=1))
    assert m.n == 65573
    return m


def _data(n, K, cin, cout):
    rng = np.random.default_rng(cin * 1000 + cout + K)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    g = rng.standard_normal((n, cout)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return dev(x).bfloat16(), dev(w), dev(g).bfloat16()


def _run(fn, **knobs):
    """-> (results of fn under the knobs as a tuple, the launch sites it hit); the counters are read, not reset"""
    before = engine.dispatch_counts()
    with engine.tuning(**knobs):
        out = fn()
        torch.cuda.synchronize()
    after = engine.dispatch_counts()
    return (out if isinstance(out, (tuple, list)) else (out,)), {k for k, c in after.items() if c > before.get(k, 0)}


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _ab(fn, tile, lean_runs=True, knob=1, **knobs):
    """knob 1 (2: tile 7 on a small grid too) against knob 0, bit for bit; both on `tile`, the lean instance under knob 1 only
    (never with statistics)"""
    a, sa = _run(fn, CONV_LEAN_EPI=knob, **knobs)
    b, sb = _run(fn, CONV_LEAN_EPI=0, **knobs)
    for s in (sa, sb):
        assert any("k_conv_gather<T,%s> [T=unsignedshort]" % tile in k for k in s), sorted(s)
    assert (LEAN in sa) == lean_runs and LEAN not in sb, (sorted(sa), sorted(sb))
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p.shape == q.shape and p.dtype == q.dtype and np.array_equal(_bits(p), _bits(q))
    return a


# (K, cin, cout) of the FORWARD layer; the dgrad is the cout -> cin reduction.  Which of the two runs on tile 7 under SMALL_CFG=7
# (an output of four or eight column blocks): 96 -> 128 the dgrad of 128 -> 96 (nc = 3); 128 -> 128 (nc = 4) and 256 -> 256
# (nc = 8, two column tiles) both; 96 -> 100 the forward, with a channel tail off the 32 grid
SMALL = [(27, 128, 96, "d"), (1, 128, 96, "d"), (27, 128, 128, "fd"), (27, 256, 256, "fd"), (27, 96, 100, "f")]


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("K,cin,cout,ops", SMALL)
def test_small_maps_bitwise(small, K, cin, cout, ops, split):
    km = small.km[3 if K == 27 else 1]
    x, w, g = _data(small.n, K, cin, cout)
    knobs = dict(SMALL_CFG=7, CONV_SPLIT=split, knob=2)
    if "f" in ops:
        _ab(lambda: km.conv_forward(x, w, None, False), T7, **knobs)
        bias = torch.linspace(-1, 1, cout, device=DEV)
        _ab(lambda: km.conv_forward(x, w, bias, False), T7, **knobs)
    if "d" in ops:
        _ab(lambda: km.conv_dgrad(g, w, False), T7, **knobs)
        _ab(lambda: km.conv_dgrad(g, w, False, accumulate_into=x.clone()), T7, **knobs)


def test_the_instance_query_predicts_the_launch_site(small):
    """lgs_debug_conv_gather_instance on the small map's sizes: the site it names is the site the 96 -> 128 dgrad is counted at"""
    v = engine.ConvPlanView(2816, small.n, small.n, 27, 27, 1, 0, 1)
    q, g = engine.ConvPlanQuery(v, v, 3, 1, 0, 128, 96, engine.LGS_BF16, 0), engine.ConvGatherInstance()
    _, w, grad = _data(small.n, 27, 128, 96)
    with engine.tuning(SMALL_CFG=7, CONV_LEAN_EPI=2):
        engine.check(engine.lib().lgs_debug_conv_gather_instance(ctypes.byref(q), 0, ctypes.byref(g)))
    _, sites = _run(lambda: small.km[3].conv_dgrad(grad, w, False), SMALL_CFG=7, CONV_LEAN_EPI=2)
    assert (g.tile_id, g.scl, g.bn, g.onebuf) == (7, 3, 0, 1) and g.site.decode() == "SlabWalk<3,false>::k_conv_gather<T,%s> [T=unsignedshort]" % T7
    assert g.site.decode() in sites and LEAN in sites, sorted(sites)


def test_tile7_as_the_plan_picks_it(big):
    """65 536 + 37 rows: the 96 -> 128 dgrad (three chunks) on tile 7 without any override, one slab of three and three slabs of
    one; the 128 -> 128 forward and dgrad (four chunks, the tile's own 2-chunk walk)"""
    km = big.km[3]
    x, w, g = _data(big.n, 27, 128, 96)
    for trim in (1, 2, 0):
        _ab(lambda: km.conv_dgrad(g, w, False), T7, CONV_SLAB_TRIM=trim)
    _ab(lambda: km.conv_dgrad(g, w, False, accumulate_into=x.clone()), T7)
    x, w, g = _data(big.n, 27, 128, 128)
    _ab(lambda: km.conv_forward(x, w, None, False), T7)
    _ab(lambda: km.conv_dgrad(g, w, False, accumulate_into=x.clone()), T7)


def test_tile2_control_bitwise(big):
    x, w, g = _data(big.n, 27, 96, 96)
    _ab(lambda: big.km[3].conv_forward(x, w, None, False), T2)
    _ab(lambda: big.km[3].conv_dgrad(g, w, False, accumulate_into=x.clone()), T2)


def _stats_case(m, cin, cout, tile, **knobs):
    x, w, _ = _data(m.n, 27, cin, cout)
    pivot = torch.linspace(-0.5, 0.5, cout, device=DEV)

    def stats():
        out, st = m.km[3].conv_forward(x, w, None, False, bn_pivot=pivot, want_bn_stats=True)
        assert st is not None
        return out, st[0]
    knobs["knob"] = 2 if knobs else 1
    out, part = _ab(stats, tile, lean_runs=False, **knobs)
    plain, = _ab(lambda: m.km[3].conv_forward(x, w, None, False), tile, **knobs)
    assert np.array_equal(_bits(out), _bits(plain))                  # the epilogue does not touch the output
    d = out.double() - pivot.double()
    n = float(m.n)
    s = part.double().sum(0)                                         # [2, cout]: sum d, sum d^2 over the position tiles
    assert part.shape[1:] == (2, cout) and float(part.abs().sum()) > 0
    assert torch.allclose(s[0] / n, d.sum(0) / n, rtol=2e-5, atol=1e-6), float((s[0] / n - d.sum(0) / n).abs().max())
    assert torch.allclose(s[1] / n, (d * d).sum(0) / n, rtol=2e-5, atol=1e-6), float((s[1] / n - (d * d).sum(0) / n).abs().max())


def test_statistics_instance_tile2(big):
    _stats_case(big, 96, 96, T2)


def test_statistics_instance_tile7(big, small):
    _stats_case(big, 128, 128, T7)
    _stats_case(small, 128, 128, T7, SMALL_CFG=7, CONV_SPLIT=0)      # (a split launch has no statistics)
    _stats_case(small, 96, 100, T7, SMALL_CFG=7, CONV_SPLIT=0)


def test_the_gpu_holds_three_workgroups_of_the_lean_tile7_per_cu():
    def resident(tile, scl, bn):
        n = ctypes.c_int(0)
        engine.check(engine.lib().lgs_debug_conv_gather_residency(tile, scl, bn, ctypes.byref(n)))
        return n.value
    got = {(scl, bn): resident(7, scl, bn) for scl in (1, 2, 3) for bn in (0, 1)}
    print("tile 7, workgroups per CU by (chunks per slab, with statistics):", got, " tile 2:", resident(2, 3, 0), resident(2, 3, 1))
    assert got[2, 0] == 3 and got[3, 0] == 3 and got[1, 0] >= 3      # built for three (__launch_bounds__): 46 / 38 / 30 KB of LDS
    assert got[1, 1] == got[2, 1] == got[3, 1] == 2      # with the epilogue: 204 registers


def test_the_knob_is_in_the_tuning_table():
    rows = {name: default for name, default, _, _ in engine.tuning_table()}
    assert rows["CONV_LEAN_EPI"] == 1
