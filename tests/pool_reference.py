"""Independent float64 reference of the pooling / global pooling / broadcast operators, computed from the coordinates alone
(no engine, no row order of the coordinate manager).

  local pooling (kernel_size == stride == s): output cell = floor(coord / s) per batch; the output rows are the distinct
                cells, ordered however the caller wants (`cells` returns them sorted lexicographically, the caller matches
                them to the engine's rows by coordinate)
  global pooling: one output row per batch index present, ascending
  max: the gradient goes to the smallest input row among equal maxima
"""
import torch


def cells(coords, s):
    """-> (cell coordinates [m, 4] = (b, floor(x / s) * s, ...), index [n] of each input row's cell)"""
    c = coords.to(torch.int64).clone()
    c[:, 1:] = torch.div(c[:, 1:], s, rounding_mode="floor") * s
    uniq, idx = torch.unique(c, dim=0, return_inverse=True)
    return uniq, idx


def batches(coords):
    """-> (batch indices present, ascending [m], index [n] of each input row's batch)"""
    uniq, idx = torch.unique(coords[:, 0].to(torch.int64), return_inverse=True)
    return uniq, idx


def seg_reduce(x, idx, m, op):
    """float64 reduction of the rows of x into m segments by idx; op in sum / avg / max (differentiable through torch)"""
    x = x.to(torch.float64)
    ix = idx.view(-1, 1).expand(-1, x.shape[1])
    if op == "sum":
        return torch.zeros(m, x.shape[1], dtype=torch.float64, device=x.device).scatter_add(0, ix, x)
    if op == "avg":
        return torch.zeros(m, x.shape[1], dtype=torch.float64, device=x.device).scatter_reduce(0, ix, x, "mean", include_self=False)
    if op == "max":
        return torch.full((m, x.shape[1]), -float("inf"), dtype=torch.float64, device=x.device).scatter_reduce(
            0, ix, x, "amax", include_self=True)
    raise ValueError(op)


def max_argrow(x, idx, m):
    """[m, C] the input row that wins each (segment, channel) max: the SMALLEST row among equal maxima"""
    x = x.to(torch.float64)
    n, c = x.shape
    best = seg_reduce(x, idx, m, "max")
    rows = torch.arange(n, device=x.device).view(-1, 1).expand(n, c)
    hit = x == best[idx]
    cand = torch.where(hit, rows, torch.full_like(rows, n))
    return torch.full((m, c), n, dtype=torch.int64, device=x.device).scatter_reduce(
        0, idx.view(-1, 1).expand(n, c), cand, "amin", include_self=True)


def max_backward(dy, argrow, n):
    """dx [n, C]: dy[q][c] goes to row argrow[q][c]"""
    dy = dy.to(torch.float64)
    dx = torch.zeros(n, dy.shape[1], dtype=torch.float64, device=dy.device)
    return dx.scatter_add(0, argrow, dy)
