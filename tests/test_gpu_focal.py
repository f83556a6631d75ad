"""Focal loss and class-weighted cross-entropy on the engine (k_focal_fwd_bwd, k_ce_weight_sum) against

* the reference's closed form -a (1 - pt)^gamma log(pt) (lib/losses/FocalLoss.py) restated in float64 with autograd: a sweep over
  every kernel shape (Q x R = 1x4 / 2x2 / 4x1, 16-byte and element-wise rows), row counts around the tile, four gammas, with and
  without alpha, every reduction;
* the reference's own code: the float64 vectors of tests/golden/focal_loss.npz (make_focal_fixtures.py);
* the float64 closed form with u = se_excl / se on saturated rows (label 30 / 100 / 800 above the rest).

Bars (the cross-entropy contract of test_per_point_cross_entropy_and_its_row_scaled_gradient, relative to the tensor's maximum):
max |err| <= tol * max |ref| per tensor; fp32 tensors (all loss rows, fp32 gradients) 2e-5, bf16 gradients 1e-2."""
import functools
import os

import numpy as np
import pytest
import torch

from languagegroundedsemseg_amd import engine
from languagegroundedsemseg_amd.losses import fused_cross_entropy, fused_focal_loss, loss_by_name, sample_categories_for_balancing

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_F32, TOL_BF16 = 2e-5, 1e-2
GAMMAS = (0.0, 0.5, 2.0, 3.5)
WORST = {}                      # (what, dtype) -> largest err / max|ref| seen in this session (printed per test)


def tile_rows(c, dtype):
    """rows of one workgroup: 8 half-waves x R rows, R = 4 / 2 / 1 for one / two / more 16-byte chunks per lane"""
    w = 8 if dtype == torch.bfloat16 else 4
    q = ((c + w - 1) // w + 31) // 32
    return 32 if q <= 1 else 16 if q == 2 else 8


def check(what, got, ref, tol, dtype=torch.float32):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err, top = float((got - ref).abs().max()) if ref.numel() else 0.0, float(ref.abs().max()) if ref.numel() else 0.0
    key = (what.split(" ")[0], str(dtype).replace("torch.", ""))
    if top > 0:
        WORST[key] = max(WORST.get(key, 0.0), err / top)
    assert err <= tol * top, "%s: max|err| %.3e > %.1e * max|ref| %.3e" % (what, err, tol, top)


@functools.lru_cache(maxsize=None)
def inputs(n, c):
    """bf16-representable logits of scale 3, labels in [-1, C) plus (n >= 2) one above the range and one below -1, alpha, and an
    upstream gradient for reduction='none'"""
    g = torch.Generator().manual_seed(7919 * c + n)
    x = (torch.randn(n, c, generator=g) * 3).to(torch.bfloat16).double()
    lab = torch.randint(-1 if n > 1 else 0, c, (n,), generator=g)
    if n >= 2:
        lab[-1], lab[0] = c + 3, -7
    alpha = (0.1 + 2.0 * torch.rand(c, generator=g)).float().double()
    up = (torch.rand(n, generator=g) * 2 - 0.5).float().double()
    return x, lab, alpha, up


@functools.lru_cache(maxsize=None)
def reference(n, c, gamma, with_alpha):
    """float64: rows [N] (0 at ignored rows), d(rows . up), d(sum rows), number of counted rows"""
    x, lab, alpha, up = inputs(n, c)
    valid = (lab != -1) & (lab >= 0) & (lab < c)
    safe = lab.clamp(0, c - 1)
    xr = x.clone().requires_grad_(True)
    log_pt = torch.log_softmax(xr, 1).gather(1, safe[:, None]).squeeze(1)
    pt = log_pt.exp()
    assert not bool(valid.any()) or float(pt.detach()[valid].max()) < 1 - 1e-10      # 1 - pt keeps >= 6 digits in float64: the formula is finite
    a = alpha[safe] if with_alpha else torch.ones(n, dtype=torch.float64)
    rows = torch.where(valid, -a * (1 - pt) ** gamma * log_pt, torch.zeros(n, dtype=torch.float64))
    g_none, = torch.autograd.grad((rows * up).sum(), xr, retain_graph=True)
    g_sum, = torch.autograd.grad(rows.sum(), xr)
    assert bool(torch.isfinite(g_none).all()) and bool(torch.isfinite(g_sum).all())
    return rows.detach(), g_none, g_sum, int(valid.sum())


SHAPES = [(200, torch.float32), (200, torch.bfloat16), (20, torch.bfloat16), (13, torch.float32), (13, torch.bfloat16),
          (3, torch.float32), (3, torch.bfloat16), (512, torch.float32), (1024, torch.bfloat16)]


@pytest.mark.parity("the reference's closed form -a (1 - pt)^gamma log(pt) in float64 + autograd")
@pytest.mark.parametrize("c,dtype", SHAPES, ids=["c%d-%s" % (c, str(d).replace("torch.", "")) for c, d in SHAPES])
def test_parity_sweep(c, dtype):
    t = tile_rows(c, dtype)
    assert t == {200: 16 if dtype == torch.float32 else 32, 512: 8, 1024: 8}.get(c, 32)
    gtol = TOL_F32 if dtype == torch.float32 else TOL_BF16
    for n in ((t + 1, 203) if c >= 512 else (1, t - 1, t, t + 1, 5003)):
        x, lab, alpha, up = inputs(n, c)
        ignored = ~((lab != -1) & (lab >= 0) & (lab < c))
        xd, labd, alphad, upd = x.to(DEV).to(dtype), lab.to(DEV), alpha.float().to(DEV), up.float().to(DEV)
        for gamma in GAMMAS:
            for with_alpha in (False, True):
                rows_ref, g_none, g_sum, n_valid = reference(n, c, gamma, with_alpha)
                a = alphad if with_alpha else None
                tag = "n=%d gamma=%g alpha=%d" % (n, gamma, with_alpha)
                xh = xd.clone().requires_grad_(True)
                rows = fused_focal_loss(xh, labd, alpha=a, gamma=gamma, ignore_index=-1, reduction="none")
                assert rows.shape == (n,) and rows.dtype == torch.float32
                (rows * upd).sum().backward()
                assert xh.grad.dtype == dtype and xh.grad.shape == (n, c)
                check("rows " + tag, rows, rows_ref, TOL_F32)
                check("grad none " + tag, xh.grad, g_none, gtol, dtype)
                assert bool((rows.cpu()[ignored] == 0).all()) and bool((xh.grad.cpu()[ignored] == 0).all()), tag
                for reduction, k in (("sum", 1.0), ("mean", 1.0 / max(n_valid, 1))):
                    xh = xd.clone().requires_grad_(True)
                    loss = fused_focal_loss(xh, labd, alpha=a, gamma=gamma, ignore_index=-1, reduction=reduction)
                    assert loss.shape == () and loss.dtype == torch.float32
                    loss.backward()
                    check("loss %s %s" % (reduction, tag), loss, rows_ref.sum() * k, TOL_F32)
                    check("grad %s %s" % (reduction, tag), xh.grad, g_sum * k, gtol, dtype)
                    assert bool((xh.grad.cpu()[ignored] == 0).all()), tag
    print("largest err / max|ref| so far:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("c", [200, 13])
def test_against_the_reference_code(c):
    """the reference's FocalLoss / nn.CrossEntropyLoss(weight) outputs in float64 (golden fixture), fp32 on the device"""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "focal_loss.npz"))
    g = lambda k: torch.from_numpy(fx["c%d_%s" % (c, k)])
    logits, labels, alpha = g("logits").to(DEV), g("labels").to(DEV), g("alpha").to(DEV)
    keep = g("labels") != -1
    n_valid = int(keep.sum())
    for gamma in (0, 2):
        x = logits.clone().requires_grad_(True)
        rows = fused_focal_loss(x, labels, alpha=alpha, gamma=gamma, ignore_index=-1, reduction="none")
        rows.sum().backward()
        check("rows fixture gamma=%d" % gamma, rows.cpu()[keep], g("g%d_rows" % gamma), TOL_F32)
        assert bool((rows.cpu()[~keep] == 0).all())
        check("grad fixture none gamma=%d" % gamma, x.grad, g("g%d_grad" % gamma) * n_valid, TOL_F32)
        x = logits.clone().requires_grad_(True)
        loss = loss_by_name("focal", ignore_index=-1, alpha=alpha, gamma=float(gamma))(x, labels)
        loss.backward()
        check("loss fixture mean gamma=%d" % gamma, loss, g("g%d_mean" % gamma), TOL_F32)
        check("grad fixture mean gamma=%d" % gamma, x.grad, g("g%d_grad" % gamma), TOL_F32)
    x = logits.clone().requires_grad_(True)
    loss = loss_by_name("cross_entropy", ignore_index=-1, weight=alpha)(x, labels)
    loss.backward()
    check("loss fixture weighted-ce", loss, g("wce_mean"), TOL_F32)
    check("grad fixture weighted-ce", x.grad, g("wce_grad"), TOL_F32)


def saturated_reference(x, lab, alpha, gamma):
    """float64 closed form with u = se_excl / se (never 1 - pt): rows, d(sum rows); all labels valid"""
    n, c = x.shape
    e = torch.exp(x - x.max(1, keepdim=True).values)
    se = e.sum(1)
    at = torch.arange(c)[None, :] == lab[:, None]
    u = e.masked_fill(at, 0.0).sum(1) / se
    pt = e[at] / se
    log_pt = torch.log1p(-u)
    a = alpha[lab]
    ug = u ** gamma
    rows = -a * ug * log_pt
    coef = a * (ug - gamma * pt * torch.where(u > 0, ug / u, torch.zeros_like(u)) * log_pt)
    grad = torch.where(at, (-coef * u)[:, None], coef[:, None] * e / se[:, None])
    return rows, grad, u


@pytest.mark.parity("the closed form with u = se_excl / se in float64")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_saturated_rows(dtype):
    c, per = 200, 5
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3 * per, c, generator=g) * 3).to(torch.bfloat16).double()
    lab = torch.randint(0, c, (3 * per,), generator=g)
    margin = torch.tensor([30.0, 100.0, 800.0]).repeat_interleave(per).double()
    rest = x.masked_fill(torch.arange(c)[None, :] == lab[:, None], -1e9).max(1).values
    x[torch.arange(3 * per), lab] = (rest + margin).to(torch.bfloat16).double()
    alpha = (0.1 + 2.0 * torch.rand(c, generator=g)).float().double()
    xd, labd, alphad = x.to(DEV).to(dtype), lab.to(DEV), alpha.float().to(DEV)
    for gamma in (0.5, 1.0, 2.0):
        rows_ref, grad_ref, u = saturated_reference(x, lab, alpha, gamma)
        assert bool((u[2 * per:] == 0).all()) and bool((u[:per] > 0).all())
        xh = xd.clone().requires_grad_(True)
        rows = fused_focal_loss(xh, labd, alpha=alphad, gamma=gamma, ignore_index=-1, reduction="none")
        rows.sum().backward()
        check("saturated-rows gamma=%g" % gamma, rows, rows_ref, TOL_F32)
        check("saturated-grad gamma=%g" % gamma, xh.grad, grad_ref, TOL_F32 if dtype == torch.float32 else TOL_BF16, dtype)
        assert bool((xh.grad.cpu()[2 * per:] == 0).all()) and bool((rows.cpu()[2 * per:] == 0).all())
    print("largest err / max|ref| so far:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def test_gamma_zero_without_alpha_is_cross_entropy():
    """different kernels (log1p(-u) against lse - z_l, -u against pt - 1): close, not bit-identical"""
    x, lab, _, up = inputs(5003, 200)
    xd, labd, upd = x.float().to(DEV), lab.to(DEV), up.float().to(DEV)
    a = xd.clone().requires_grad_(True)
    rows_a = fused_focal_loss(a, labd, gamma=0.0, ignore_index=-1, reduction="none")
    (rows_a * upd).sum().backward()
    b = xd.clone().requires_grad_(True)
    rows_b = fused_cross_entropy(b, labd, ignore_index=-1, reduction="none")
    (rows_b * upd).sum().backward()
    assert float((rows_a - rows_b).detach().abs().max()) <= 2e-6 * float(rows_b.detach().abs().max())
    assert float((a.grad - b.grad).abs().max()) <= 2e-6 * float(b.grad.abs().max())


def _launches(counts, name):
    return sum(v for k, v in counts.items() if name in k)


def test_the_focal_kernel_ran_and_the_old_path_is_untouched():
    x, lab, alpha, _ = inputs(203, 200)
    labd, alphad = lab.to(DEV), alpha.float().to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        for kwargs in (dict(gamma=2.0, alpha=alphad), dict(gamma=0.5), dict(gamma=0.0, alpha=alphad, reduction="none")):
            xh = x.to(DEV).to(dtype).requires_grad_(True)
            engine.dispatch_counts(reset=True)
            loss = fused_focal_loss(xh, labd, ignore_index=-1, **kwargs)
            fwd = engine.dispatch_counts(reset=True)
            loss.sum().backward()
            bwd = engine.dispatch_counts(reset=True)
            for d in (fwd, bwd):
                assert _launches(d, "k_focal_fwd_bwd") == 1 and _launches(d, "k_ce_fwd_bwd") == 0, d
        xh = x.to(DEV).to(dtype).requires_grad_(True)
        engine.dispatch_counts(reset=True)
        loss = fused_cross_entropy(xh, labd, ignore_index=-1, weight=alphad)
        fwd = engine.dispatch_counts(reset=True)
        loss.backward()
        bwd = engine.dispatch_counts(reset=True)
        assert _launches(fwd, "k_focal_fwd_bwd") == 1 and _launches(fwd, "k_ce_weight_sum") == 1 and _launches(fwd, "k_ce_fwd_bwd") == 0, fwd
        assert _launches(bwd, "k_focal_fwd_bwd") == 1 and _launches(bwd, "k_ce_weight_sum") == 0 and _launches(bwd, "k_ce_fwd_bwd") == 0, bwd
        for reduction in ("mean", "none"):
            xh = x.to(DEV).to(dtype).requires_grad_(True)
            engine.dispatch_counts(reset=True)
            fused_cross_entropy(xh, labd, ignore_index=-1, reduction=reduction).sum().backward()
            d = engine.dispatch_counts(reset=True)
            assert _launches(d, "k_focal_fwd_bwd") == 0 and _launches(d, "k_ce_weight_sum") == 0 and _launches(d, "k_ce_fwd_bwd") == 2, d


def test_focal_and_weighted_losses_run_without_a_host_sync():
    torch.manual_seed(3)
    n, L = 5003, 200
    foc = torch.zeros(L, 3, dtype=torch.bool)
    foc[:66, 0], foc[66:134, 1], foc[134:, 2] = True, True, True
    foc = foc.to(DEV)
    logits = torch.randn(n, L, device=DEV).to(torch.bfloat16).requires_grad_(True)
    lab = torch.randint(-1, L, (n,), device=DEV)
    w = (torch.rand(L) + 0.5).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    rows_crit = loss_by_name("focal", ignore_index=-1, alpha=w, reduction="none").to(DEV)
    mean_crit = loss_by_name("focal", ignore_index=-1, alpha=w, reduction="mean").to(DEV)
    wce_crit = loss_by_name("cross_entropy", ignore_index=-1, weight=w).to(DEV)
    rows_crit(logits, lab).sum().backward()          # (first use: library load, the cached device constant)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for hr, cr in ((-1.0, -1.0), (0.5, 0.25)):
            rows = rows_crit(logits, lab)
            loss, stats, _ = sample_categories_for_balancing(rows, lab, foc, hr, cr, ignore_label=-1, generator=gen, split="stats")
            loss.backward()
        mean_crit(logits, lab).backward()
        wce_crit(logits, lab).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(logits.grad.float()).all()) and float(logits.grad.float().abs().max()) > 0
    assert stats.shape == (3, 2) and int(stats[:, 1].sum()) == int((lab != -1).sum())


def test_weighted_mean_and_focal_mean_are_deterministic():
    x, lab, alpha, _ = inputs(5003, 200)
    labd, alphad = lab.to(DEV), alpha.float().to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        runs = []
        for _ in range(2):
            out = []
            for fn in (lambda t: fused_cross_entropy(t, labd, ignore_index=-1, weight=alphad),
                       lambda t: fused_focal_loss(t, labd, alpha=alphad, gamma=2.0, ignore_index=-1)):
                xh = x.to(DEV).to(dtype).requires_grad_(True)
                loss = fn(xh)
                loss.backward()
                out += [loss.detach().clone(), xh.grad.clone()]
            runs.append(out)
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_empty_batch_launches_nothing():
    w = torch.ones(200, device=DEV)
    lab = torch.zeros(0, dtype=torch.int64, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        for fn in (lambda t: fused_focal_loss(t, lab, alpha=w, gamma=2.0), lambda t: fused_focal_loss(t, lab, gamma=0.5, reduction="sum"),
                   lambda t: fused_cross_entropy(t, lab, weight=w)):
            x = torch.zeros(0, 200, device=DEV, dtype=dtype, requires_grad=True)
            engine.dispatch_counts(reset=True)
            loss = fn(x)
            loss.backward()
            assert sum(engine.dispatch_counts(reset=True).values()) == 0
            assert loss.shape == () and float(loss.detach()) == 0.0 and x.grad.shape == (0, 200) and x.grad.dtype == dtype
        x = torch.zeros(0, 200, device=DEV, dtype=dtype, requires_grad=True)
        rows = fused_focal_loss(x, lab, alpha=w, reduction="none")
        rows.sum().backward()
        assert rows.shape == (0,) and x.grad.shape == (0, 200)
