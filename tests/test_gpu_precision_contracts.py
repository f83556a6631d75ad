"""Precision contracts (tests/precision.py) of every convolution kernel and knob path, against an fp64 reference built from the
CPU oracle's pair lists.

Each case declares (scene, kernel size / stride / transposed, cin, cout, dtype, bias, knobs, the launch sites it must reach): it
runs forward, dgrad and wgrad through the kernel-map surface of the ME backend under engine.tuning(**knobs), asserts that the
declared launch sites were dispatched (a gate change cannot make a case pass on another kernel) and applies the contracts.
The live-map test toggles every workspace-changing knob on ONE kernel map and checks the backend's cached workspace sizes
against fresh engine answers."""
import numpy as np
import pytest
import torch

import MinkowskiEngine as ME
import precision as P
from helpers import GATHER_TILES as _TILES, small_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# launch sites of k_conv_gather: _TILES[tile id] is the <T, RB, NCB, WM, WN, SC, D> text, the instance told apart by the T binding.
# A site pattern "a&b" needs both substrings in ONE launch site.


def gather(tile, dt="bf16"):
    t = {"bf16": "[T=unsignedshort]", "f32": "[T=float]", "f32s": "f32s_t]"}[dt]
    return "k_conv_gather<T,%s> &%s" % (_TILES[tile], t)


def _hit(pattern, sites):
    parts = pattern.split("&")
    return any(all(p in k for p in parts) for k in sites)


# ------------------------------------------------------------------------------------------- scenes (module scoped)
def _trim(c, m):
    return c[:m]


def _gaps():
    c = small_scene(15, n=1500, batches=3)
    return c[c[:, 0] != 1]                       # batch index 1 empty, 0 and 2 populated


def _single():
    return np.array([[0, 5, 5, 5]], np.int32)


def _big():
    from languagegroundedsemseg_amd.synthetic import make_batch
    return make_batch([3], n_target=80000)[0]


def _holes():
    """a sparse cloud: many 3^3 offsets of a 2^3-strided map have no pair at all"""
    rng = np.random.default_rng(9)
    p = np.unique(rng.integers(0, 60, (400, 3)) * 3, axis=0)
    return np.concatenate([np.zeros((p.shape[0], 1), np.int32), p.astype(np.int32)], 1)


SCENES = {
    "small": lambda: small_scene(11, n=2500, extent=30),
    "r1": lambda: _trim(small_scene(12, n=4000, extent=34), 2049),     # rows = 1 (mod 64 / 128 / 256)
    "r255": lambda: _trim(small_scene(12, n=4000, extent=34), 2303),   # rows = tile - 1 (mod 64 / 128 / 256)
    "gaps": _gaps,
    "single": _single,
    "holes": _holes,
    "big": _big,
}


class Scene:
    def __init__(self, coords):
        self.coords = coords
        self.x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), torch.from_numpy(coords).to(DEV))
        self.mgr = self.x.coordinate_manager
        self.key = self.x.coordinate_map_key
        self.kmaps = {}

    def kmap(self, ks, kind):
        """kind: "same" (stride 1), "down" (stride 2), "up" (the transposed convolution of "down") -> (km, transposed, pairs
        of the forward direction, n_in, n_out)"""
        if (ks, kind) not in self.kmaps:
            out_key = self.key if kind == "same" else self.mgr.stride(self.key, 2)
            km = self.mgr.kernel_map_handle(self.key, out_key, ks)
            ci = self.mgr.get_coordinates(self.key).cpu().numpy()
            co = self.mgr.get_coordinates(out_key).cpu().numpy()
            pr = P.Pairs.from_oracle(ci, co, ks, 1)
            self.kmaps[(ks, kind)] = (km, pr, ci.shape[0], co.shape[0])
        km, pr, ni, no = self.kmaps[(ks, kind)]
        if kind == "up":
            return km, True, pr.mirrored(), no, ni
        return km, False, pr, ni, no


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Scene(SCENES[name]())
        return cache[name]
    return get


_REF = {}


def _inputs(n_in, n_out, K, cin, cout, bias, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    b = (rng.random(cout) - 0.5).astype(np.float32) if bias else None
    return x, w, g, b


def _ref(tag, op, pr, n_in, n_out, x, w, g, b, bf16):
    """fp64 reference of one op, shared between the cases of one (scene, map, shape, dtype)"""
    key = tag + (op,)
    if key not in _REF:
        xr, gr = (P.bf16_rne(x), P.bf16_rne(g)) if bf16 else (x, g)
        wr = P.bf16_rne(w) if bf16 else w
        if op == "fwd":
            _REF[key] = P.conv_ref(xr, wr, pr, n_out, bias=b)
        elif op == "dgrad":
            _REF[key] = P.dgrad_ref(gr, wr, pr, n_in)
        else:
            _REF[key] = P.wgrad_ref(xr, gr, pr)
    return _REF[key]


# ------------------------------------------------------------------------------------------- the matrix
def C(scene, ks, kind, cin, cout, dt="bf16", knobs=None, sites=(), bias=False, ops="fwd,dgrad,wgrad", fmode=None, wmode=None, strided=False):
    return dict(scene=scene, ks=ks, kind=kind, cin=cin, cout=cout, dt=dt, knobs=knobs or {}, sites=tuple(sites), bias=bias,
                ops=ops.split(","), fmode=fmode, wmode=wmode, strided=strided)


CASES = {
    # k_conv_gather bf16, default tiles
    "bf16 small 32->32 id4": C("small", 3, "same", 32, 32, sites=[gather(4), "k_wgrad_ps"]),
    "bf16 small 32->64 id8 split": C("small", 3, "same", 32, 64, sites=[gather(8), "k_sum_partials"]),
    "bf16 small 32->64 CONV_SPLIT=0": C("small", 3, "same", 32, 64, knobs=dict(CONV_SPLIT=0), sites=[gather(8)]),
    "bf16 big 32->32 id0": C("big", 3, "same", 32, 32, sites=[gather(0)]),
    "bf16 big 32->64 id1": C("big", 3, "same", 32, 64, sites=[gather(1)]),
    "bf16 big 32->96 id2": C("big", 3, "same", 32, 96, sites=[gather(2)]),
    "bf16 big 64->128 id7": C("big", 3, "same", 64, 128, sites=[gather(7)], ops="fwd,dgrad"),
    "bf16 big 1x1 96->200 id6 POINTWISE=0": C("big", 1, "same", 96, 200, knobs=dict(POINTWISE=0), sites=[gather(6)], bias=True),
    "bf16 big 1x1 96->200 HEAD_TILE=1": C("big", 1, "same", 96, 200, knobs=dict(POINTWISE=0, HEAD_TILE=1), sites=[gather(7)], ops="fwd"),
    "bf16 big 64->256 CONV_WIDE=0 id16": C("big", 3, "same", 64, 256, knobs=dict(CONV_WIDE=0), sites=[gather(16)], ops="fwd"),
    # k_pointwise
    "bf16 big 1x1 96->200 POINTWISE=1": C("big", 1, "same", 96, 200, knobs=dict(POINTWISE=1), sites=["k_pointwise<"], bias=True),
    "bf16 big 1x1 160->96 POINTWISE=1 (>128 reduction, 3 blocks)": C("big", 1, "same", 160, 96, knobs=dict(POINTWISE=1), sites=["k_pointwise<"], ops="fwd"),
    "bf16 big 1x1 96->128 POINTWISE=2": C("big", 1, "same", 96, 128, knobs=dict(POINTWISE=2), sites=["k_pointwise<"], ops="fwd"),
    "bf16 big 1x1 96->128 POINTWISE=0": C("big", 1, "same", 96, 128, knobs=dict(POINTWISE=0), sites=[gather(7)], ops="fwd"),
    "f32 big 1x1 96->200 k_pointwise_f32": C("big", 1, "same", 96, 200, dt="f32", sites=["k_pointwise_f32<"], ops="fwd", fmode="f32_exact"),
    # k_conv_wide
    **{"bf16 big 1x1 256->512 WIDE_SCHED=%d" % s: C("big", 1, "same", 256, 512, knobs=dict(WIDE_SCHED=s), sites=["k_conv_wide"], ops="fwd")
       for s in range(5)},
    **{"bf16 big up 512->256 WIDE_GC64=%d" % g: C("big", 2, "up", 512, 256, knobs=dict(WIDE_GC64=g), sites=["k_conv_wide"], ops="fwd")
       for g in (0, 1)},
    # fp32 forward / dgrad: the split and the exact instance, small tiles and 1 - 4 column blocks
    **{"f32 %s 32->%d FP32_SPLIT=%d" % (sc, co, s): C(sc, 3, "same", 32, co, dt="f32", knobs=dict(FP32_SPLIT=s),
                                                     sites=[gather(t, "f32s" if s else "f32")], ops="fwd,dgrad",
                                                     fmode="f32_split6" if s else "f32_exact")
       for s in (0, 1) for sc, co, t in (("small", 32, 4), ("small", 64, 5), ("big", 32, 0), ("big", 64, 1), ("big", 96, 2), ("big", 128, 3))},
    # weight gradients
    "bf16 small 512->256 PS_WIDE3=1": C("small", 3, "same", 512, 256, knobs=dict(PS_WIDE3=1), sites=["k_wgrad_ps&NCS=3"], ops="wgrad"),
    "bf16 small 512->256 PS_WIDE3=0": C("small", 3, "same", 512, 256, knobs=dict(PS_WIDE3=0), sites=["k_wgrad_ps&NCS=2"], ops="wgrad"),
    "bf16 small 64->96 PS_CUS=8": C("small", 3, "same", 64, 96, knobs=dict(PS_CUS=8), sites=["k_wgrad_ps"], ops="wgrad"),
    "bf16 small 64->96 PS_CUS=32": C("small", 3, "same", 64, 96, knobs=dict(PS_CUS=32), sites=["k_wgrad_ps"], ops="wgrad"),
    "bf16 small 64->96 WGRAD_PS=0": C("small", 3, "same", 64, 96, knobs=dict(WGRAD_PS=0), sites=["k_wgrad_bf16<"], ops="wgrad"),
    "bf16 small 256->256 WW_MIN_ROWS=0": C("small", 3, "same", 256, 256, knobs=dict(WW_MIN_ROWS=0), sites=["k_wgrad_wide"], ops="wgrad"),
    "bf16 big 256->256 WW_MIN_ROWS=0 WW_RANGE=32768": C("big", 3, "same", 256, 256, knobs=dict(WW_MIN_ROWS=0, WW_RANGE=32768), sites=["k_wgrad_wide"], ops="wgrad"),
    "bf16 small 256->256 WW_MIN_ROWS=0 WGRAD_WIDE=0": C("small", 3, "same", 256, 256, knobs=dict(WW_MIN_ROWS=0, WGRAD_WIDE=0), sites=["k_wgrad_ps"], ops="wgrad"),
    **{"f32 small %d->32 WGRAD_F32_LDS=%d" % (ci, m): C("small", 3, "same", ci, 32, dt="f32", knobs=dict(WGRAD_F32_LDS=m),
                                                       sites=[("k_wgrad_f32<", "k_wgrad_f32_lds<", "k_wgrad_f32s_lds<", "k_wgrad_f32_lds<")[m]],
                                                       ops="wgrad", wmode="f32_split6" if m == 2 else "f32_exact")
       for ci in (32, 3) for m in (0, 1, 2, 3)},
    "f32 small 96->96 WGRAD_F32_LDS=3 (split)": C("small", 3, "same", 96, 96, dt="f32", knobs=dict(WGRAD_F32_LDS=3), sites=["k_wgrad_f32s_lds<"], ops="wgrad", wmode="f32_split6"),
    # strided and transposed maps
    "bf16 down 2^3 32->64": C("small", 2, "down", 32, 64),
    "bf16 up 2^3 64->32": C("small", 2, "up", 64, 32),
    "f32 down 2^3 32->64": C("small", 2, "down", 32, 64, dt="f32", fmode="f32_split6", wmode="f32_split6"),
    "f32 up 2^3 64->96": C("small", 2, "up", 64, 96, dt="f32", fmode="f32_split6", wmode="f32_split6"),
    # edge shapes
    "bf16 rows=1 mod 256 32->64": C("r1", 3, "same", 32, 64),
    "bf16 rows=255 mod 256 32->64": C("r255", 3, "same", 32, 64),
    "bf16 rows=1 mod 256 32->32": C("r1", 3, "same", 32, 32),
    "f32 rows=255 mod 256 32->64": C("r255", 3, "same", 32, 64, dt="f32", fmode="f32_split6", wmode="f32_split6"),
    "bf16 single voxel 32->64": C("single", 3, "same", 32, 64),
    "bf16 empty batch index 32->32": C("gaps", 3, "same", 32, 32),
    "bf16 offsets without pairs 32->64": C("holes", 3, "same", 32, 64),
    "bf16 3->32": C("small", 3, "same", 3, 32),
    "bf16 8->20": C("small", 3, "same", 8, 20),
    "bf16 40->24": C("small", 3, "same", 40, 24),
    "bf16 32->3 bias (scratch path)": C("small", 3, "same", 32, 3, bias=True, ops="fwd,dgrad"),
    "f32 32->3 bias (scratch path)": C("small", 3, "same", 32, 3, dt="f32", bias=True, ops="fwd", fmode="f32_split6"),
    "f32 3->32": C("small", 3, "same", 3, 32, dt="f32", fmode="f32_split6", wmode="f32_split6"),
    "bf16 strided input (skip half of ME.cat) 64->96": C("small", 3, "same", 64, 96, strided=True, ops="fwd,wgrad"),
}
# SMALL_CFG on narrow and 96/128-wide layers, including the shapes whose packed image outgrew its region (32->64, 64->64, 32->96)
for _cfg in (3, 5, 7, 9, 10, 11, 12, 13):
    for _ci, _co in ((32, 64), (64, 64), (32, 96), (96, 128)):
        if _cfg in (3, 7) and _co % 128 != 0:
            continue                                     # ids 3 / 7 need a multiple of 4 column blocks
        CASES["bf16 small %d->%d SMALL_CFG=%d" % (_ci, _co, _cfg)] = C("small", 3, "same", _ci, _co, knobs=dict(SMALL_CFG=_cfg),
                                                                        sites=[gather(_cfg)], ops="fwd,dgrad")


def _run(case, scenes, knobs=None):
    from languagegroundedsemseg_amd import engine
    sc = scenes(case["scene"])
    km, transposed, pr, n_in, n_out = sc.kmap(case["ks"], case["kind"])
    cin, cout, bf16 = case["cin"], case["cout"], case["dt"] == "bf16"
    K = case["ks"] ** 3
    seed = cin * 1000 + cout
    x, w, g, b = _inputs(n_in, n_out, K, cin, cout, case["bias"], seed)
    tag = (case["scene"], case["ks"], case["kind"], cin, cout, case["dt"], case["bias"])
    tdt = torch.bfloat16 if bf16 else torch.float32
    xt = torch.from_numpy(x).to(DEV).to(tdt)
    if case["strided"]:
        buf = torch.zeros((n_in, cin + 32), dtype=tdt, device=DEV)     # the zero-copy ME.cat buffer: [up half | skip half]
        buf[:, 32:] = xt
        xt = buf[:, 32:]
    wt = torch.from_numpy(w).to(DEV)
    gt = torch.from_numpy(g).to(DEV).to(tdt)
    bt = torch.from_numpy(b).to(DEV) if b is not None else None
    out = {}
    engine.dispatch_counts(reset=True)
    with engine.tuning(**(knobs if knobs is not None else case["knobs"])):
        if "fwd" in case["ops"]:
            out["fwd"] = km.conv_forward(xt, wt, bt, transposed)
        if "dgrad" in case["ops"]:
            out["dgrad"] = km.conv_dgrad(gt, wt, transposed)
        if "wgrad" in case["ops"]:
            out["wgrad"] = km.conv_wgrad(xt, gt, transposed)
        torch.cuda.synchronize()
    sites = engine.dispatch_counts(reset=True)
    reps = []
    for op, h in out.items():
        ref, mag, n = _ref(tag, op, pr, n_in, n_out, x, w, g, b, bf16)
        h = h.float().cpu().numpy().astype(np.float64)
        what = "%s %s" % (op, case.get("name", ""))
        if op == "wgrad":
            reps.append(P.check_f32(h, ref, mag, "bf16_wgrad" if bf16 else (case["wmode"] or "f32_split6"), what))
        elif bf16:
            reps.append(P.check_bf16(h, ref, mag, n, what))
        else:
            reps.append(P.check_f32(h, ref, mag, case["fmode"] or "f32_split6", what))
    return sites, reps


@pytest.mark.parametrize("name", list(CASES))
def test_precision_contract(name, scenes):
    case = dict(CASES[name], name=name)
    sites, reps = _run(case, scenes)
    for r in reps:
        print(P.fmt(r))
    for s in case["sites"]:
        assert _hit(s, sites), "%s: launch site %r not dispatched; dispatched: %s" % (name, s, sorted(sites))


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_mask_order_and_window_keep_the_arithmetic(order):
    """MASK_ORDER / MASK_WINDOW re-order the rows of 3^3 maps (built under the knob), not the arithmetic"""
    from languagegroundedsemseg_amd import engine
    knobs = dict(MASK_ORDER=order, **({"MASK_WINDOW": 1024} if order == 3 else {}))
    with engine.tuning(**knobs):
        sc = Scene(small_scene(11, n=2500, extent=30))
        for cin, cout in ((32, 64), (64, 32)):
            _, reps = _run(C("mask%d" % order, 3, "same", cin, cout, ops="fwd,dgrad"), lambda _: sc)
            for r in reps:
                print("MASK_ORDER=%d" % order, P.fmt(r))


def test_live_map_knob_toggles_resize_the_workspace(scenes):
    """one kernel map, default knobs first, then every knob value that changes a workspace size: the backend's cached size
    must equal a fresh engine answer after each toggle, and the results must still meet their contracts"""
    from languagegroundedsemseg_amd import engine
    sc = scenes("small")
    L = engine.lib()
    km = sc.kmap(3, "same")[0]
    toggles = [
        ("f32 cin 3", C("small", 3, "same", 3, 32, dt="f32", fmode="f32_split6", wmode="f32_split6"), [dict(WGRAD_F32_LDS=0), dict(WGRAD_F32_LDS=2)]),
        ("bf16 256->256", C("small", 3, "same", 256, 256, ops="wgrad"), [dict(WW_MIN_ROWS=200000), dict(WW_MIN_ROWS=0), dict(WW_MIN_ROWS=0, WW_RANGE=32768)]),
        ("bf16 512->256", C("small", 3, "same", 512, 256, ops="wgrad"), [dict(PS_WIDE3=0), dict(PS_WIDE3=1), dict(PS_CUS=8), dict(PS_CUS=32)]),
        ("bf16 32->64", C("small", 3, "same", 32, 64, ops="fwd,dgrad"), [dict(SMALL_CFG=12), dict(SMALL_CFG=13), dict(SMALL_CFG=0)]),
        ("bf16 32->96", C("small", 3, "same", 32, 96, ops="fwd,dgrad"), [dict(SMALL_CFG=13), dict(SMALL_CFG=12)]),
    ]
    for label, case, seq in toggles:
        case = dict(case, name=label)
        _run(case, scenes, knobs={})                     # default knobs: the sizes are cached on the map
        dt = engine.LGS_BF16 if case["dt"] == "bf16" else engine.LGS_F32
        for knobs in seq:
            with engine.tuning(**knobs):
                _, reps = _run(case, scenes, knobs={})
                for op in (0, 1, 2):
                    cached = km._ws_bytes(L, case["cin"], case["cout"], dt, op)
                    fresh = L.lgs_conv_workspace_bytes(km.h, case["cin"], case["cout"], dt, op)
                    assert cached == fresh, (label, knobs, op, cached, fresh)
                ME.get_backend()._block_ws(L, km, None, case["cin"], case["cout"], dt, 16, torch.device(DEV))
                assert km.block_ws_bytes(L, None, case["cin"], case["cout"], dt) == \
                    L.lgs_block_workspace_bytes(km.h, None, case["cin"], case["cout"], dt), (label, knobs)
            for r in reps:
                print(label, knobs, P.fmt(r))

