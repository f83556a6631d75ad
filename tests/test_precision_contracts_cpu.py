"""The precision contracts of tests/precision.py have teeth: the CPU emulation of each arithmetic mode passes its contract at
the GPU module's shapes, and each mutant of the arithmetic (a dropped pair or offset, a truncating store, a partial image
rounded early, the cheaper 3-product split, a zeroed ragged tile, an ignored channel, a lost or doubled bias) fails it.
No GPU needed; the margins are printed (pytest -s)."""
import numpy as np
import pytest
import torch

import precision as P
from helpers import small_scene


@pytest.fixture(scope="module")
def scene():
    c = small_scene(11, n=2500, extent=30)
    return c, P.Pairs.from_oracle(c, c, 3, 1)


def _data(n, cin, cout, seed=0, K=27):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    return x, w


def _bf16_case(scene, cin, cout, bias=False, seed=0):
    c, pr = scene
    n = c.shape[0]
    x, w = _data(n, cin, cout, seed)
    xb, wb = P.bf16_rne(x), P.bf16_rne(w)            # bf16 features, weights rounded as k_pack_weights does
    b = (np.random.default_rng(seed + 1).random(cout) - 0.5).astype(np.float32) if bias else None
    ref, mag, nn = P.conv_ref(xb, wb, pr, n, bias=b)
    return x, w, b, ref, mag, nn


def _rejects(fn, *a, **k):
    with pytest.raises(P.ContractError) as ei:
        fn(*a, **k)
    print("rejected:", str(ei.value)[:200])
    return ei.value


@pytest.mark.parametrize("cin,cout", [(32, 64), (40, 24), (64, 96)])
@pytest.mark.parametrize("block", [16, 1])
def test_bf16_emulation_meets_its_contract(scene, cin, cout, block):
    c, pr = scene
    x, w, _, ref, mag, nn = _bf16_case(scene, cin, cout)
    h = P.emulate_conv(x, w, pr, c.shape[0], "bf16", block=block, store="rne")
    print(P.fmt(P.check_bf16(h, ref, mag, nn, "bf16 %d->%d block %d" % (cin, cout, block))))
    # dgrad on the mirrored map
    g = P.bf16_rne(np.random.default_rng(3).standard_normal((c.shape[0], cout)))
    rd, md, nd = P.dgrad_ref(g, P.bf16_rne(w), pr, c.shape[0])
    hd = P.emulate_conv(g, w.transpose(0, 2, 1), pr.mirrored(), c.shape[0], "bf16", block=block, store="rne")
    print(P.fmt(P.check_bf16(hd, rd, md, nd, "bf16 dgrad %d->%d block %d" % (cin, cout, block))))


@pytest.mark.parametrize("mode", ["f32_exact", "f32_split6"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (3, 32), (64, 128)])
def test_fp32_emulation_meets_its_contract_with_2x_margin(scene, mode, cin, cout):
    c, pr = scene
    n = c.shape[0]
    x, w = _data(n, cin, cout, 1)
    ref, mag, _ = P.conv_ref(x, w, pr, n)
    worst = (0.0, 0.0)
    for block in (16, 1):
        rep = P.check_f32(P.emulate_conv(x, w, pr, n, mode, block=block), ref, mag, mode, "%s fwd %d->%d block %d" % (mode, cin, cout, block))
        print(P.fmt(rep))
        worst = (max(worst[0], rep["max e"]), max(worst[1], rep["rms e"]))
    bmax, brms = P.F32_BOUNDS[mode]
    assert bmax >= 2 * worst[0] and brms >= 2 * worst[1], (mode, worst, P.F32_BOUNDS[mode])
    cmax, crms = P.CALIBRATION[mode]
    assert worst[0] <= cmax * 1.05 and worst[1] <= crms * 1.05, ("the emulation moved: re-derive the bounds", worst)


@pytest.mark.parametrize("mode", ["bf16_wgrad", "f32_exact", "f32_split6"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (3, 32)])
def test_wgrad_emulation_meets_its_contract_with_2x_margin(scene, mode, cin, cout):
    c, pr = scene
    n = c.shape[0]
    x, _ = _data(n, cin, 1, 2)
    g = np.random.default_rng(4).standard_normal((n, cout)).astype(np.float32)
    if mode == "bf16_wgrad":
        x, g = P.bf16_rne(x).astype(np.float32), P.bf16_rne(g).astype(np.float32)
    ref, mag, _ = P.wgrad_ref(x, g, pr)
    worst = (0.0, 0.0)
    for block in (16, 1):
        h = P.emulate_wgrad(x, g, pr, "bf16" if mode == "bf16_wgrad" else mode, block=block)
        rep = P.check_f32(h, ref, mag, mode, "%s wgrad %d->%d block %d" % (mode, cin, cout, block))
        print(P.fmt(rep))
        worst = (max(worst[0], rep["max e"]), max(worst[1], rep["rms e"]))
    bmax, brms = P.F32_BOUNDS[mode]
    assert bmax >= 2 * worst[0] and brms >= 2 * worst[1], (mode, worst, P.F32_BOUNDS[mode])


# ------------------------------------------------------------------------------------------- mutants
def test_mutant_one_pair_dropped(scene):
    c, pr = scene
    x, w, _, ref, mag, nn = _bf16_case(scene, 32, 64)
    s0 = pr.by_k[5][0][7]
    h = P.emulate_conv(x, w, pr, c.shape[0], "bf16", store="rne", drop=lambda k, s, d: ~((k == 5) & (s == s0)))
    _rejects(P.check_bf16, h, ref, mag, nn, "one pair dropped")


def test_mutant_one_offset_dropped(scene):
    c, pr = scene
    x, w, _, ref, mag, nn = _bf16_case(scene, 32, 64)
    h = P.emulate_conv(x, w, pr, c.shape[0], "bf16", store="rne", drop=lambda k, s, d: np.full(s.shape, k != 20))
    _rejects(P.check_bf16, h, ref, mag, nn, "offset 20 dropped")


def test_mutant_truncating_store(scene):
    c, pr = scene
    x, w, _, ref, mag, nn = _bf16_case(scene, 64, 96)
    h = P.emulate_conv(x, w, pr, c.shape[0], "bf16", store="trunc")
    _rejects(P.check_bf16, h, ref, mag, nn, "truncating store")


def test_mutant_slot_split_partial_rounded_to_bf16(scene):
    """the slot split sums three fp32 partial images (offsets 0-8, 9-17, 18-26); rounding one of them to bf16 first is a double rounding"""
    c, pr = scene
    n = c.shape[0]
    x, w, _, ref, mag, nn = _bf16_case(scene, 64, 96)
    parts = [P.emulate_conv(x, w, pr, n, "bf16", drop=lambda k, s, d, z=z: np.full(s.shape, k // 9 == z)) for z in range(3)]
    good = P.bf16_rne(P.f32(P.f32(parts[0] + parts[1]) + parts[2]))
    print(P.fmt(P.check_bf16(good, ref, mag, nn, "slot split, fp32 partials")))
    bad = P.bf16_rne(P.f32(P.f32(parts[0] + P.bf16_rne(parts[1])) + parts[2]))
    _rejects(P.check_bf16, bad, ref, mag, nn, "partial image 1 rounded to bf16")


@pytest.mark.parametrize("cin,cout", [(32, 64), (3, 32), (96, 96)])
def test_mutant_three_product_split_forward(scene, cin, cout):
    c, pr = scene
    n = c.shape[0]
    x, w = _data(n, cin, cout, 1)
    ref, mag, _ = P.conv_ref(x, w, pr, n)
    _rejects(P.check_f32, P.emulate_conv(x, w, pr, n, "f32_split3"), ref, mag, "f32_split6", "3-product split %d->%d" % (cin, cout))


@pytest.mark.parametrize("cin,cout", [(32, 64), (3, 32)])
def test_mutant_three_product_split_fp32_wgrad(scene, cin, cout):
    """WGRAD_F32_LDS=2 claims dropped terms < 2^-24 |x g|: the 3-product split drops hi*lo, lo*hi, mid*mid (~2^-17 |x g|)"""
    c, pr = scene
    n = c.shape[0]
    x, _ = _data(n, cin, 1, 2)
    g = np.random.default_rng(4).standard_normal((n, cout)).astype(np.float32)
    ref, mag, _ = P.wgrad_ref(x, g, pr)
    _rejects(P.check_f32, P.emulate_wgrad(x, g, pr, "f32_split3"), ref, mag, "f32_split6", "3-product split wgrad")


@pytest.mark.parametrize("tile", [64, 128, 256])
def test_mutant_last_ragged_row_tile_zeroed(scene, tile):
    c, pr = scene
    n = c.shape[0]
    assert n % tile != 0
    x, w, _, ref, mag, nn = _bf16_case(scene, 32, 64)
    h = P.emulate_conv(x, w, pr, n, "bf16", store="rne")
    h[n // tile * tile:] = 0
    _rejects(P.check_bf16, h, ref, mag, nn, "last %d-row tile zeroed (%d rows)" % (tile, n % tile))


def test_mutant_last_input_channel_of_cin40_ignored(scene):
    c, pr = scene
    x, w, _, ref, mag, nn = _bf16_case(scene, 40, 24)
    x2 = x.copy()
    x2[:, 39] = 0
    h = P.emulate_conv(x2, w, pr, c.shape[0], "bf16", store="rne")
    _rejects(P.check_bf16, h, ref, mag, nn, "channel 39 of 40 ignored")


@pytest.mark.parametrize("factor", [0.0, 2.0])
def test_mutant_bias_dropped_or_doubled_on_cout3(scene, factor):
    c, pr = scene
    x, w, b, ref, mag, nn = _bf16_case(scene, 32, 3, bias=True)
    h = P.emulate_conv(x, w, pr, c.shape[0], "bf16", store="rne", bias=b)
    print(P.fmt(P.check_bf16(h, ref, mag, nn, "cout 3 with bias")))
    hm = P.emulate_conv(x, w, pr, c.shape[0], "bf16", store="rne", bias=b * factor)
    _rejects(P.check_bf16, hm, ref, mag, nn, "bias x %g" % factor)


def test_checkers_reject_nan_and_shape_mismatch(scene):
    c, pr = scene
    x, w, _, ref, mag, nn = _bf16_case(scene, 32, 64)
    h = P.emulate_conv(x, w, pr, c.shape[0], "bf16", store="rne")
    h[3, 4] = np.nan
    _rejects(P.check_bf16, h, ref, mag, nn, "NaN")
    with pytest.raises(P.ContractError):
        P.check_f32(h, ref, mag, "f32_exact")
    with pytest.raises(AssertionError):
        P.check_bf16(h[:-1], ref, mag, nn)


def test_bf16_rounding_helpers():
    a = np.array([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8) * 3], np.float32)     # ties
    assert P.bf16_rne(a).tolist() == torch.from_numpy(a).bfloat16().double().tolist()
    assert P.bf16_rne(a)[0] == 1.0 and P.bf16_rne(a)[1] == 1.0 + 4 * 2 ** -8
    assert P.bf16_trunc(np.array([1.0 + 255 * 2 ** -16], np.float32))[0] == 1.0
    r = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    hi, mid, lo = P.split3(r)
    assert np.array_equal((hi + mid + lo).astype(np.float32), r)
