"""k_conv_gather issues no load of a value that is zero by construction -- and computes what it computed before.

CONV_SLAB_TRIM walks the packed weight image with slabs of real chunks only (the image stays padded to the tile's slab length),
CONV_ROW_TRIM drops the second gather of a chunk on rows of one 16-byte piece (conv0).  Same chunks, same order, same MFMAs: every
case runs forward and dgrad with the knobs at 1 and at 0 in this process and compares the results BIT FOR BIT, in bf16.  One 3^3
stride-1 map of about 70 k voxels in a 64^3 box serves all cases: the big tiles (ids 0, 1, 2, 7) start at 65 536 padded positions.
The launch sites tell which instance ran: a trimmed one is "SlabWalk<chunks per slab, one-piece row>::k_conv_gather<T, tile...>".
One case per trimmed tile is also held to the fp64 reference over the CPU oracle's pair lists at the per-op bf16 contract
(tests/precision.py)."""
import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
import precision as P
from languagegroundedsemseg_amd import engine
from helpers import GATHER_TILES
from test_gpu_map_build import _slab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ON = dict(CONV_SLAB_TRIM=1, CONV_ROW_TRIM=1)
OFF = dict(CONV_SLAB_TRIM=0, CONV_ROW_TRIM=0)
T0, T1, T2, T7 = (GATHER_TILES[t] for t in (0, 1, 2, 7))


def walk(scl, tile, row1=False):
    return "SlabWalk<%d,%s>::k_conv_gather<T,%s> [T=unsignedshort]" % (scl, "true" if row1 else "false", tile)


def own(tile):
    return "k_conv_gather<T,%s> [T=unsignedshort]" % tile


class Map:
    def __init__(self):
        coords = _slab(77, 70000, 32, thick=64, batches=1)
        self.x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), torch.from_numpy(coords).to(DEV))
        self.mgr, self.key = self.x.coordinate_manager, self.x.coordinate_map_key
        self.n = coords.shape[0]
        self.coarse = self.mgr.stride(self.key, 2)
        self.n_coarse = self.mgr.get_coordinates(self.coarse).shape[0]
        self.km = {3: self.mgr.kernel_map_handle(self.key, self.key, 3), 1: self.mgr.kernel_map_handle(self.key, self.key, 1),
                   2: self.mgr.kernel_map_handle(self.key, self.coarse, 2)}
        self._pairs = None

    def pairs(self):
        if self._pairs is None:
            ci = self.mgr.get_coordinates(self.key).cpu().numpy()
            self._pairs = P.Pairs.from_oracle(ci, ci, 3, 1)
        return self._pairs


@pytest.fixture(scope="module")
def m():
    assert (70000 + 255) // 256 * 256 >= 65536
    return Map()


def _data(n_in, n_out, K, cin, cout):
    rng = np.random.default_rng(cin * 1000 + cout + K)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    return x, w, g


def _sites(fn, knobs):
    """-> (result of fn under knobs, the launch sites it hit); the counters are read, not reset: the suite's own record goes on"""
    before = engine.dispatch_counts()
    with engine.tuning(**knobs):
        out = fn()
        torch.cuda.synchronize()
    after = engine.dispatch_counts()
    return out, {k for k, c in after.items() if c > before.get(k, 0)}


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _ab(fn, on_site, off_site, on=ON):
    a, sa = _sites(fn, on)
    b, sb = _sites(fn, OFF)
    if on_site is not None:
        assert on_site in sa and on_site not in sb, (on_site, sorted(sa), sorted(sb))
    else:
        assert not any("SlabWalk<" in s for s in sa), sorted(sa)
    assert off_site in sb and not any("SlabWalk<" in s for s in sb), (off_site, sorted(sb))
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    for p, q in zip(a, b):
        assert p.shape == q.shape and np.array_equal(_bits(p), _bits(q))
    return a


# (cin, cout): forward site under the knobs, its own instance; dgrad (a cout -> cin reduction) likewise
SHAPES = {
    (96, 96): (walk(3, T2), own(T2), walk(3, T2), own(T2)),
    (128, 96): (None, own(T2), walk(3, T7), own(T7)),              # the dgrad is the tile-7 case: 3 chunks on 2-chunk image slabs
    (32, 32): (walk(1, T0), own(T0), walk(1, T0), own(T0)),
    (64, 64): (walk(2, T1), own(T1), walk(2, T1), own(T1)),
    (3, 32): (walk(1, T0, True), own(T0), walk(1, T0), own(T0)),   # conv0: the one-piece row; its dgrad goes through the scratch rows
    (192, 128): (None, own(T7), None, own(T2)),                    # 6 chunks on 2-chunk slabs, 4 on 4: whole slabs, nothing to trim
    (192, 96): (walk(3, T2), own(T2), walk(3, T2), own(T2)),       # 6 chunks on 4-chunk slabs: two slabs of 3 (the image holds 8)
    (160, 96): (None, own(T2), walk(3, T7), own(T7)),              # 5 chunks: no divisor, today's instance
}


@pytest.mark.parametrize("cin,cout", list(SHAPES))
def test_forward_and_dgrad_are_bitwise_the_same(m, cin, cout):
    fon, foff, don, doff = SHAPES[(cin, cout)]
    x, w, g = _data(m.n, m.n, 27, cin, cout)
    xt, gt, wt = torch.from_numpy(x).to(DEV).bfloat16(), torch.from_numpy(g).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
    km = m.km[3]
    _ab(lambda: km.conv_forward(xt, wt, None, False), fon, foff)
    _ab(lambda: km.conv_dgrad(gt, wt, False), don, doff)


def test_tile7_three_single_chunk_slabs(m):
    x, w, g = _data(m.n, m.n, 27, 128, 96)
    gt, wt = torch.from_numpy(g).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
    _ab(lambda: m.km[3].conv_dgrad(gt, wt, False), walk(1, T7), own(T7), on=dict(CONV_SLAB_TRIM=2, CONV_ROW_TRIM=1))


def test_row_trim_alone(m):
    """CONV_ROW_TRIM=0 with the slab trim on: conv0 runs the one-chunk walk with both gathers"""
    x, w, _ = _data(m.n, m.n, 27, 3, 32)
    xt, wt = torch.from_numpy(x).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
    _ab(lambda: m.km[3].conv_forward(xt, wt, None, False), walk(1, T0), own(T0), on=dict(CONV_SLAB_TRIM=1, CONV_ROW_TRIM=0))


def test_2x2x2_and_1x1(m):
    # 2^3 stride 2, 96 -> 96: the dgrad walks the grouped fine view (one weight matrix per 64-row group) on the big tile
    x, w, _ = _data(m.n, m.n_coarse, 8, 96, 96)
    g = np.random.default_rng(5).standard_normal((m.n_coarse, 96)).astype(np.float32)
    xt, gt, wt = torch.from_numpy(x).to(DEV).bfloat16(), torch.from_numpy(g).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
    _ab(lambda: m.km[2].conv_dgrad(gt, wt, False), walk(3, T2), own(T2))
    _ab(lambda: m.km[2].conv_forward(gt, wt, None, True), walk(3, T2), own(T2))         # the transposed convolution: coarse -> fine
    a, sa = _sites(lambda: m.km[2].conv_forward(xt, wt, None, False), ON)               # fine -> coarse: a small-map tile, untouched
    b, _ = _sites(lambda: m.km[2].conv_forward(xt, wt, None, False), OFF)
    assert not any("SlabWalk<" in s for s in sa) and np.array_equal(_bits(a), _bits(b))
    # 1 x 1, 128 -> 96 (four whole chunks forward) and its dgrad 96 -> 128 (tile 7, three chunks)
    x, w, g = _data(m.n, m.n, 1, 128, 96)
    xt, gt, wt = torch.from_numpy(x).to(DEV).bfloat16(), torch.from_numpy(g).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
    _ab(lambda: m.km[1].conv_forward(xt, wt, None, False), None, own(T2))
    _ab(lambda: m.km[1].conv_dgrad(gt, wt, False), walk(3, T7), own(T7))


def test_accumulating_dgrad_and_statistics_epilogue(m):
    x, w, g = _data(m.n, m.n, 27, 96, 96)
    xt, gt, wt = torch.from_numpy(x).to(DEV).bfloat16(), torch.from_numpy(g).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
    km = m.km[3]
    _ab(lambda: km.conv_dgrad(gt, wt, False, accumulate_into=xt.clone()), walk(3, T2), own(T2))
    pivot = torch.linspace(-0.5, 0.5, 96, device=DEV)

    def stats():
        out, st = km.conv_forward(xt, wt, None, False, bn_pivot=pivot, want_bn_stats=True)
        assert st is not None
        return out, st[0]
    out, partials = _ab(stats, walk(3, T2), own(T2))
    assert partials.shape[1:] == (2, 96) and float(partials.abs().sum()) > 0


def test_trimmed_instances_meet_the_bf16_contract(m):
    """forward of the trimmed tiles 2, 7 (one slab of 3 on the 2-chunk image), 0, 1 and of the one-piece row, against the fp64
    reference over the CPU oracle's pair lists.  One test: the pair lists are built once, and every launch site it reaches is
    reached by a test that ran against the oracle"""
    pr = m.pairs()
    for cin, cout in ((96, 96), (96, 128), (32, 32), (64, 64), (3, 32)):
        x, w, _ = _data(m.n, m.n, 27, cin, cout)
        xt, wt = torch.from_numpy(x).to(DEV).bfloat16(), torch.from_numpy(w).to(DEV)
        out, sites = _sites(lambda: m.km[3].conv_forward(xt, wt, None, False), ON)
        assert any("SlabWalk<" in s for s in sites), sorted(sites)
        ref, mag, n = P.conv_ref(P.bf16_rne(x), P.bf16_rne(w), pr, m.n, bias=None)
        print(P.fmt(P.check_bf16(out.float().cpu().numpy().astype(np.float64), ref, mag, n, "fwd %d->%d" % (cin, cout))))


def test_the_knobs_are_in_the_tuning_table():
    rows = {name: default for name, default, _, _ in engine.tuning_table()}
    assert rows["CONV_SLAB_TRIM"] == 1 and rows["CONV_ROW_TRIM"] == 1
