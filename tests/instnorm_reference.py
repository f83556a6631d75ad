"""Independent float64 reference of MinkowskiInstanceNorm, computed from the batch column of the coordinates and the
features alone (no engine, no row order of the coordinate manager), its gradients by float64 autograd of the same
function; and two fp32 restatements the tolerance calibration uses:

  torch_lines        the module's torch lines as they stand (two passes, fp32, index_add_): the yardstick E_torch
  engine_order_fp32  the summation order of csrc/lgs_instnorm.hip in fp32 torch: per scene, deviations from the scene's
                     first row, 512-row chunk items, 32-row runs summed sequentially in fp32, runs and items folded in double
  naive_fp32         one pass E[x^2] - E[x]^2 about zero in fp32: the kernel NOT to write (the cancellation case must reject it)
"""
import torch

EPS = 1e-6
CHUNK = 512     # kSegChunk (csrc/lgs_common.h)
RUN = 32        # kInRun (csrc/lgs_instnorm.hip)


def scenes(coords):
    """-> (batch indices present, ascending [m], index [n] of each row's scene)"""
    return torch.unique(coords[:, 0].to(torch.int64), return_inverse=True)


def instance_norm64(x, idx, m, weight, bias, eps=EPS):
    """float64, differentiable: y = (x - mean[scene]) / sqrt(var[scene] + eps) * weight + bias (biased variance)"""
    x = x.to(torch.float64)
    ix = idx.view(-1, 1).expand(-1, x.shape[1])
    cnt = torch.zeros(m, dtype=torch.float64, device=x.device).index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
    mean = torch.zeros(m, x.shape[1], dtype=torch.float64, device=x.device).scatter_add(0, ix, x) / cnt[:, None]
    d = x - mean[idx]
    var = torch.zeros(m, x.shape[1], dtype=torch.float64, device=x.device).scatter_add(0, ix, d * d) / cnt[:, None]
    return d / torch.sqrt(var[idx] + eps) * weight.to(torch.float64).view(1, -1) + bias.to(torch.float64).view(1, -1)


def reference(x, coords, weight, bias, dy, eps=EPS):
    """-> (y, dx, dweight, dbias) in float64 for the stored values of x / weight / bias / dy"""
    _, idx = scenes(coords)
    m = int(idx.max()) + 1 if idx.numel() else 0
    xr = x.detach().to(torch.float64).requires_grad_(True)
    wr = weight.detach().to(torch.float64).view(-1).requires_grad_(True)
    br = bias.detach().to(torch.float64).view(-1).requires_grad_(True)
    y = instance_norm64(xr, idx, m, wr, br, eps)
    y.backward(dy.detach().to(torch.float64))
    return y.detach(), xr.grad, wr.grad, br.grad


def torch_lines(x, b, weight, bias, eps=EPS):
    """the torch lines of MinkowskiInstanceNorm.forward (me/modules.py), differentiable; b: int64 batch index per row"""
    nb = int(b.max().item()) + 1 if b.numel() else 0
    cnt = torch.zeros(nb, device=x.device, dtype=torch.float32).index_add_(0, b, torch.ones_like(b, dtype=torch.float32))
    xf = x.float()
    mean = torch.zeros(nb, x.shape[1], device=x.device).index_add_(0, b, xf) / cnt[:, None]
    d = xf - mean[b]
    var = torch.zeros(nb, x.shape[1], device=x.device).index_add_(0, b, d * d) / cnt[:, None]
    y = d / torch.sqrt(var[b] + eps) * weight + bias
    return y.to(x.dtype)


def torch_lines_all(x, coords, weight, bias, dy):
    """-> (y, dx, dweight, dbias) of the torch lines in fp32 arithmetic (x may be bf16: widened first, as the lines do)"""
    b = coords[:, 0].to(torch.int64)
    xr = x.detach().clone().requires_grad_(True)
    wr = weight.detach().float().view(1, -1).clone().requires_grad_(True)
    br = bias.detach().float().view(1, -1).clone().requires_grad_(True)
    y = torch_lines(xr, b, wr, br)
    y.backward(dy.detach().to(y.dtype))
    return y.detach(), xr.grad, wr.grad.view(-1), br.grad.view(-1)


def _chunked_sums(a, b):
    """sum a and sum b over rows ([n, C] fp32 each) in the engine's order: 32-row runs in fp32, sequentially; everything
    above a run in double -> two float64 [C] (each chunk item's sum rounded to fp32, as the partial rows are)"""
    n, c = a.shape
    s0 = torch.zeros(c, dtype=torch.float64)
    s1 = torch.zeros(c, dtype=torch.float64)
    for i0 in range(0, n, CHUNK):
        i1 = min(i0 + CHUNK, n)
        p0 = torch.zeros(c, dtype=torch.float64)
        p1 = torch.zeros(c, dtype=torch.float64)
        for r0 in range(i0, i1, RUN):
            f0 = torch.zeros(c, dtype=torch.float32)
            f1 = torch.zeros(c, dtype=torch.float32)
            for r in range(r0, min(r0 + RUN, i1)):
                f0 = f0 + a[r]
                f1 = f1 + b[r]
            p0 += f0.double()
            p1 += f1.double()
        s0 += p0.float().double()
        s1 += p1.float().double()
    return s0, s1


def engine_order_fp32(x, coords, weight, bias, dy, eps=EPS):
    """-> (y, dx, dweight, dbias) in fp32, the kernels' arithmetic restated (rows of a scene in the caller's order)"""
    _, idx = scenes(coords)
    m = int(idx.max()) + 1 if idx.numel() else 0
    xf, g = x.float(), dy.float()
    w, bb = weight.float().view(-1), bias.float().view(-1)
    n, c = xf.shape
    y = torch.empty(n, c)
    dx = torch.empty(n, c)
    dw = torch.zeros(c, dtype=torch.float64)
    db = torch.zeros(c, dtype=torch.float64)
    for s in range(m):
        rows = torch.nonzero(idx == s).view(-1)
        xs, gs = xf[rows], g[rows]
        cnt = float(rows.numel())
        a = xs - xs[0]
        s1, s2 = _chunked_sums(a, a * a)
        d = s1 / cnt
        mean = (xs[0].double() + d).float()
        rstd = (1.0 / torch.sqrt((s2 / cnt - d * d).clamp_min(0.0) + float(torch.tensor(eps, dtype=torch.float32)))).float()
        y[rows] = (xs - mean) * (rstd * w) + bb
        xhat = (xs - mean) * rstd
        sdy, sdx = _chunked_sums(gs, gs * xhat)
        sdy, sdx = sdy.float(), sdx.float()
        inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(cnt, dtype=torch.float32)
        dx[rows] = (rstd * w) * (gs - sdy * inv_n - (xs - mean) * (sdx * inv_n * rstd))
        db += sdy.double()
        dw += sdx.double()
    return y, dx, dw.float(), db.float()


def naive_fp32(x, coords, weight, bias, eps=EPS):
    """-> y of a one-pass fp32 kernel that takes var = E[x^2] - E[x]^2 about zero (sequential fp32 sums)"""
    _, idx = scenes(coords)
    m = int(idx.max()) + 1 if idx.numel() else 0
    xf = x.float()
    y = torch.empty_like(xf)
    for s in range(m):
        rows = torch.nonzero(idx == s).view(-1)
        xs = xf[rows]
        s1 = torch.zeros(xs.shape[1])
        s2 = torch.zeros(xs.shape[1])
        for r in range(xs.shape[0]):
            s1 = s1 + xs[r]
            s2 = s2 + xs[r] * xs[r]
        mean = s1 / xs.shape[0]
        var = (s2 / xs.shape[0] - mean * mean).clamp_min(0.0)
        y[rows] = (xs - mean) / torch.sqrt(var + eps) * weight.float().view(1, -1) + bias.float().view(1, -1)
    return y


def bf16_ulp(r):
    a = r.abs().to(torch.float64).clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)
