"""The bits of the BatchNorm kernels (csrc/lgs_norm.hip + csrc/lgs_normmath.h).

(a) Every output of every path -- y, the saved statistics, the running statistics, num_batches_tracked, dx, dres, dgamma, dbeta,
    sums and mean_m2 -- as SHA-256 digests against tests/golden/norm_bits.json, which tests/golden/make_norm_bits.py recorded on an
    MI355X from the commit BEFORE the kernels' arithmetic moved into csrc/lgs_normmath.h.  The generator imports CASES, EXTRA and
    the run functions from this module.  One digest per variant: SHA-256 over the "name:digest" lines of its outputs (VARIANT
    OUTPUTS below names them), which keeps the fixture at ~50 KB.
    Paths `three`, `fold`, `fused` by tuning knobs; a case whose kernels are not exactly its path's fails.
    n = 1 (one row, variance 0, the n > 1 branch of the unbiased variance), 127 (a ragged slab), 1037 (nine slabs and a tail in the
    unrolled loops; nine workgroups at most, so the `fused` summation order does not depend on the device); c = 32 and 96 (96
    leaves idle threads in a workgroup); bf16 and fp32.
(b) The ReLU mask that the backward recomputes from x (mode 2) against the mask from the stored output (mode 1), on inputs where
    only the fused multiply-add of the forward expression decides the sign: with mean 0, invstd 1, x[:, ch] = d[ch] and
    beta[ch] = -fl32(d[ch] * fl32(invstd * gamma[ch])) the unfused value is exactly 0 in every channel and the fused one is the
    product's rounding residual.
"""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import MinkowskiEngine as ME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_bits.json")

# path -> (knobs, kernels of one forward, of one backward, of a forward on conv-epilogue partial rows)
PATHS = {
    "three": (dict(BN_FOLD=0, BN_FUSED=0), {"k_colreduce", "k_fold_fwd", "k_bn_apply"}, {"k_colreduce", "k_fold_bwd", "k_bn_bwd_apply"},
              {"k_partial_reduce", "k_fold_fwd", "k_bn_apply"}),
    "fold": (dict(BN_FOLD=1, BN_FOLD_MAX_MB=64), {"k_colreduce", "k_bn_apply_fold"}, {"k_colreduce", "k_bn_bwd_apply_fold"}, None),
    "fused": (dict(BN_FOLD=0, BN_FUSED=1, BN_FUSED_FWD_MAX_MB=24), {"k_bn_fwd_fused"}, {"k_bn_bwd_fused"}, {"k_bn_fwd_fused"}),
}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
CASES = [(path, n, c, dt) for path in PATHS for n in (1, 127, 1037) for c in (32, 96) for dt in DTYPES]
# forward variants: name -> (relu, residual, y into a column slice)
FWD = {"f_plain": (False, False, False), "f_plain_into": (False, False, True), "f_relu_res": (True, True, False),
       "f_relu_res_into": (True, True, True), "f_relu": (True, False, False), "f_relu_into": (True, False, True)}
# backward variants: name -> (forward it follows, relu mode, dres wanted, dy operand)
BWD = {"b_plain": ("f_plain", 0, False, "dy"), "b_plain_slice": ("f_plain_into", 0, False, "dy_slice"),
       "b_m1_dres_slice": ("f_relu_res", 1, True, "dy_slice"), "b_m1_dres": ("f_relu_res", 1, True, "dy"),
       "b_m1": ("f_relu_res", 1, False, "dy"), "b_m1_slice": ("f_relu_res_into", 1, False, "dy_slice"),
       "b_m2": ("f_relu", 2, False, "dy"), "b_m2_slice": ("f_relu_into", 2, False, "dy_slice")}
# VARIANT OUTPUTS: forward -> y, stats, running_mean, running_var, num_batches_tracked; backward -> dx, dgamma, dbeta (, dres)
# the extra cases: (dtype, c); each runs the partial-row forwards and the split entry points at n = 1037
EXTRA = [(dt, c) for dt in DTYPES for c in (32, 96)]
EXTRA_N = 1037
PARTIAL_ROWS = (5, 300)


def case_name(path, n, c, dt):
    return "%s-n%d-c%d-%s" % (path, n, c, dt)


def digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def combined(outputs):
    """{output name: tensor} -> (one digest over all of them, {name: digest})"""
    each = {k: digest(v) for k, v in outputs.items()}
    return hashlib.sha256("".join("%s:%s\n" % kv for kv in sorted(each.items())).encode()).hexdigest(), each


def norm_kernels(before):
    from languagegroundedsemseg_amd import engine
    return {re.match(r"\w+", k).group(0) for k, v in engine.dispatch_counts().items()
            if v > before.get(k, 0) and k.startswith(("k_bn_", "k_colreduce", "k_fold_", "k_partial_reduce", "k_sync_combine"))}


def make_inputs(n, c, dtype):
    g = torch.Generator().manual_seed(7000 + 10 * n + c)
    d = {"x": torch.randn(n, c, generator=g) * 2 + 0.5, "res": torch.randn(n, c, generator=g),
         "dy_wide": torch.randn(n, c + 32, generator=g),      # the upstream gradient as a column slice of a wider buffer
         "gamma": torch.rand(c, generator=g) + 0.5, "beta": torch.randn(c, generator=g) * 0.1}
    out = {k: v.to(DEV).to(dtype if k in ("x", "res", "dy_wide") else torch.float32) for k, v in d.items()}
    out["dy_slice"] = out["dy_wide"][:, 16:16 + c]
    out["dy"] = out["dy_slice"].contiguous()
    for rows in PARTIAL_ROWS:      # synthetic conv-epilogue rows [rows][sum (x - pivot) | sum (x - pivot)^2] and the pivot
        s = torch.randn(rows, c, generator=g) * 2
        ss = (torch.rand(rows, c, generator=g) + 0.5) * (4.0 * n / rows)
        out["partials%d" % rows] = torch.cat([s, ss], dim=1).contiguous().to(DEV)
    out["pivot"] = (torch.randn(c, generator=g) * 0.5).to(DEV)
    return out


def _running(c):
    return (torch.full((c,), 0.25, device=DEV), torch.full((c,), 1.5, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))


def _forward(t, c, relu, res, into, conv_stats=None):
    be = ME.get_backend()
    rm, rv, nbt = _running(c)
    out_into = None
    if into:
        out_into = (torch.zeros(t["x"].shape[0], c + 64, dtype=t["x"].dtype, device=DEV), 32)
    y, stats = be.bn_forward(t["x"], t["gamma"], t["beta"], 1e-5, 0.1, rm, rv, t["res"] if res else None, relu, num_batches_tracked=nbt,
                             conv_stats=conv_stats, out_into=out_into)
    torch.cuda.synchronize()
    return dict(y=y, stats=stats, running_mean=rm, running_var=rv, num_batches_tracked=nbt)


def run_case(path, n, c, dt):
    """-> ({variant: digest}, {variant: {output: digest}}); asserts that every call ran the kernels of `path`"""
    from languagegroundedsemseg_amd import engine
    be = ME.get_backend()
    knobs, fwd_kernels, bwd_kernels, _ = PATHS[path]
    t = make_inputs(n, c, DTYPES[dt])
    one, each, fwd = {}, {}, {}
    with engine.tuning(**knobs):
        for name, (relu, res, into) in FWD.items():
            before = engine.dispatch_counts()
            fwd[name] = _forward(t, c, relu, res, into)
            assert norm_kernels(before) == fwd_kernels, (name, path, norm_kernels(before))
            one[name], each[name] = combined(fwd[name])
        for name, (f, mode, want_dres, dy_key) in BWD.items():
            before = engine.dispatch_counts()
            dx, dres, dg, db = be.bn_backward(t["x"], fwd[f]["y"] if mode == 1 else None, t[dy_key], t["gamma"], t["beta"], fwd[f]["stats"],
                                              mode, want_dres)
            torch.cuda.synchronize()
            assert norm_kernels(before) == bwd_kernels, (name, path, norm_kernels(before))
            outs = dict(dx=dx, dgamma=dg, dbeta=db)
            if want_dres:
                outs["dres"] = dres
            one[name], each[name] = combined(outs)
    return one, each


def run_extra(dt, c):
    """forward on synthetic conv-epilogue rows (`three`, `fused`) and the split entry points -> as run_case"""
    from languagegroundedsemseg_amd import engine
    be = ME.get_backend()
    n = EXTRA_N
    t = make_inputs(n, c, DTYPES[dt])
    one, each = {}, {}

    def keep(name, outs, before, kernels):
        torch.cuda.synchronize()
        assert norm_kernels(before) == kernels, (name, norm_kernels(before))
        one[name], each[name] = combined(outs)

    for path in ("three", "fused"):
        with engine.tuning(**PATHS[path][0]):
            for rows in PARTIAL_ROWS:
                before = engine.dispatch_counts()
                outs = _forward(t, c, True, True, False, conv_stats=(t["partials%d" % rows], t["pivot"]))
                keep("%s_partials%d" % (path, rows), outs, before, PATHS[path][3])
    with engine.tuning(**PATHS["three"][0]):
        before = engine.dispatch_counts()
        rec = be.bn_stats(t["x"])
        keep("stats_x", dict(mean_m2=rec), before, {"k_colreduce", "k_fold_stats"})
        for rows in PARTIAL_ROWS:
            before = engine.dispatch_counts()
            keep("stats_partials%d" % rows, dict(mean_m2=be.bn_stats(t["x"], conv_stats=(t["partials%d" % rows], t["pivot"]))), before,
                 {"k_partial_reduce", "k_fold_stats"})
        # SyncBN records [mean | M2 | count]: this rank's, and three synthetic ranks (other means, other counts)
        g = torch.Generator().manual_seed(99 + c)
        others = [torch.cat([torch.randn(c, generator=g) * 0.3 + 0.5, (torch.rand(c, generator=g) + 0.5) * 4.0 * k, torch.tensor([float(k)])])
                  for k in (300, 1, 5000)]
        for world, records in ((1, rec[None]), (3, torch.stack(others).to(DEV))):
            rm, rv, nbt = _running(c)
            before = engine.dispatch_counts()
            stats, inv_n = be.bn_sync_combine(records.contiguous(), c, 1e-5, 0.1, rm, rv, nbt)
            keep("sync_combine%d" % world, dict(stats=stats, inv_n=inv_n, running_mean=rm, running_var=rv, num_batches_tracked=nbt), before,
                 {"k_sync_combine"})
            if world == 1:
                stats1, inv1 = stats, inv_n
        for relu, res, into in ((False, False, False), (True, True, False), (True, False, True)):
            before = engine.dispatch_counts()
            buf = (torch.zeros(n, c + 64, dtype=t["x"].dtype, device=DEV), 32) if into else None
            y = be.bn_apply(t["x"], t["gamma"], t["beta"], stats1, t["res"] if res else None, relu, out_into=buf)
            keep("apply_relu%d_res%d_into%d" % (relu, res, into), dict(y=y), before, {"k_bn_apply"})
            if relu and res:
                y1 = y
        for mode, dy_key in ((0, "dy"), (1, "dy_slice"), (2, "dy")):
            rg, rb = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
            before = engine.dispatch_counts()
            sums = be.bn_backward_reduce(t["x"], y1 if mode == 1 else None, t[dy_key], t["gamma"], t["beta"], stats1, mode, rg, rb)
            keep("bwd_reduce_m%d" % mode, dict(sums=sums, dgamma=rg, dbeta=rb), before, {"k_colreduce", "k_fold_bwd"})
            for inv_name, inv in (("host", 1.0 / n), ("dev", inv1)):
                before = engine.dispatch_counts()
                dx, dres = be.bn_backward_apply(t["x"], y1 if mode == 1 else None, t[dy_key], t["gamma"], t["beta"], stats1, sums, inv, mode,
                                                mode == 1)
                keep("bwd_apply_m%d_%s" % (mode, inv_name), dict(dx=dx, dres=dres) if mode == 1 else dict(dx=dx), before, {"k_bn_bwd_apply"})
    return one, each


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parity("golden: tests/golden/norm_bits.json, the bits of the commit before csrc/lgs_normmath.h")
@pytest.mark.parametrize("path,n,c,dt", CASES)
def test_every_path_gives_the_recorded_bits(golden, path, n, c, dt):
    got, _ = run_case(path, n, c, dt)
    want = golden[case_name(path, n, c, dt)]
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, (case_name(path, n, c, dt), wrong)


@pytest.mark.parity("golden: tests/golden/norm_bits.json, the bits of the commit before csrc/lgs_normmath.h")
@pytest.mark.parametrize("dt,c", EXTRA)
def test_partial_rows_and_split_entry_points_give_the_recorded_bits(golden, dt, c):
    got, _ = run_extra(dt, c)
    want = golden["extra-c%d-%s" % (c, dt)]
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, (dt, c, wrong)


# ------------------------------------------------------------------------------------------------ (b)
def mask_inputs(c, dtype, seed=11):
    """-> x [300, c], gamma, beta, stats (mean 0 | invstd 1), dy, and the sign the fused forward expression must give per channel"""
    n = 300
    g = torch.Generator().manual_seed(seed + c)
    d = (torch.randn(c, generator=g) * 2 + 0.5).to(dtype).float()          # exact in `dtype`
    gamma = torch.rand(c, generator=g) + 0.5
    sc = torch.ones(c) * gamma                                             # fl32(invstd * gamma)
    prod = d * sc                                                          # fl32(d * sc)
    beta = -prod
    # fma(d, sc, beta) = the exact product (48 bits: exact in a double) minus its fp32 rounding, which fp32 holds exactly
    residual = d.double().numpy() * sc.double().numpy() - prod.double().numpy()
    dy = torch.randn(n, c, generator=g)
    stats = torch.cat([torch.zeros(c), torch.ones(c)])
    t = dict(x=d[None, :].expand(n, c).contiguous().to(dtype), dy=dy.to(dtype), gamma=gamma, beta=beta, stats=stats)
    return {k: v.to(DEV) for k, v in t.items()}, np.sign(residual)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("c", [32, 96])
def test_recomputed_mask_is_the_stored_mask_where_only_the_fma_decides(c, dt):
    from languagegroundedsemseg_amd import engine
    be = ME.get_backend()
    n = 300
    t, sign = mask_inputs(c, DTYPES[dt])
    assert (sign > 0).sum() >= c / 4 and (sign <= 0).sum() >= c / 4, sign       # the seed's own condition, in numpy
    with engine.tuning(**PATHS["three"][0]):
        y = be.bn_apply(t["x"], t["gamma"], t["beta"], t["stats"], None, True)
        pos = (y[0] > 0).cpu().numpy()
        assert torch.equal(y, y[:1].expand(n, c))
        assert pos.sum() >= c / 4 and (y[0] == 0).sum().item() >= c / 4, (int(pos.sum()), c)
        assert np.array_equal(pos, sign > 0)
        outs = {}
        for mode in (1, 2):
            dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
            sums = be.bn_backward_reduce(t["x"], y if mode == 1 else None, t["dy"], t["gamma"], t["beta"], t["stats"], mode, dg, db)
            dx, _ = be.bn_backward_apply(t["x"], y if mode == 1 else None, t["dy"], t["gamma"], t["beta"], t["stats"], sums, 1.0 / n, mode, False)
            before = engine.dispatch_counts()
            fdx, _, fdg, fdb = be.bn_backward(t["x"], y if mode == 1 else None, t["dy"], t["gamma"], t["beta"], t["stats"], mode, False)
            torch.cuda.synchronize()
            assert norm_kernels(before) == PATHS["three"][2]
            outs[mode] = dict(sums=sums, dgamma=dg, dbeta=db, dx=dx, full_dx=fdx, full_dgamma=fdg, full_dbeta=fdb)
    for k, v in outs[1].items():
        assert torch.equal(v, outs[2][k]), (k, c, dt)
    assert torch.equal(outs[1]["dx"], outs[1]["full_dx"])
