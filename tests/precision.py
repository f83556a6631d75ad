"""Precision contracts of the sparse-convolution kernels: an fp64 reference, the error model, and the checkers.

CPU only (no GPU import): tests/test_precision_contracts_cpu.py proves the checkers reject wrong arithmetic,
tests/test_gpu_precision_contracts.py applies them to the HIP kernels.

Reference
---------
The reference is built from the pair lists of `oracle.oracle.kernel_map` -- (k, src, dst): out[dst] += x[src] @ w[k] --
on the coordinates whose rows the kernel's output has.  Before the fp64 sum the inputs are rounded to what the kernel
actually multiplies: bf16 tensors are exact, weights of the bf16 path are rounded to bf16 with round-to-nearest-even (as
k_pack_weights does), fp32 operands keep their full 24-bit significands.  Per output element:
    ref = sum x * w,   mag = sum |x| * |w|  (the condition scale),   n = terms summed
(a bias adds one term b: ref += b, mag += |b|, n += 1).  dgrad is the same sum on the mirrored map (src <-> dst, w[k]^T);
wgrad sums x[src] (x) g[dst] over the pairs of each offset (n = pairs of that offset).

Error model (u = 2^-24, the unit roundoff of fp32)
--------------------------------------------------
bf16-stored outputs (bf16 forward / dgrad).  Inputs are exact, bf16 x bf16 products are exact in fp32, accumulation is
fp32 in any order or blocking (MFMA blocks, slot-split partial images added afterwards, the bias), and there is ONE
round-to-nearest-even store to bf16.  So |acc - ref| <= gamma_n mag with gamma_n = n u / (1 - n u), and |h - acc| <= 2^-8 |acc| (bf16 keeps 8 significant bits):
  (a) every element: |h - ref| <= 2^-8 |ref| + 2 n u mag.  The factor 2 covers gamma_n (1 + 2^-8) for every n u <= 1/4;
      this bound is rigorous and cannot flake.
  (b) at least BF16_EQUAL_FRACTION of the elements equal bf16_rne(ref) bit for bit: an element can differ only where the fp32
      accumulation error carries ref across a bf16 rounding boundary, and that error is ~2^-16 of a bf16 ulp per term.
      Truncating instead of rounding, rounding a partial sum to bf16 before the last add, or losing a few pairs moves far more.
fp32 outputs (fp32 forward / dgrad, every weight gradient).  With e_i = |h_i - ref_i| / (u mag_i), both max e and rms e are
bounded by a constant per arithmetic mode (F32_BOUNDS):
  f32_exact   exact-fp32 MFMA: every product rounded to fp32, fp32 accumulation;
  f32_split6  fp32 operands split exactly into three bf16 pieces (x = hi + mid + lo), the six products hi*hi, hi*mid, mid*hi,
              mid*mid, hi*lo, lo*hi summed in fp32; the dropped mid*lo, lo*mid, lo*lo are <= 2 u |x w| together;
  bf16_wgrad  bf16 x bf16 -> fp32 weight gradients (exact products, fp32 accumulation).
The constants come from the CPU emulation below (`emulate_conv`, `emulate_wgrad`) of each mode at the shapes the GPU module
uses, accumulating in 16-term blocks (an MFMA: exact block sum, rounded into the fp32 accumulator) and sequentially term by
term (the pessimistic case), with at least a 2x margin over the larger of the two (CALIBRATION below records the measured
values; test_precision_contracts_cpu.py re-measures them and fails if the margin shrinks below 2x).  They were fixed before
any GPU run and are not fitted to GPU results.
"""
import numpy as np
import torch

U = 2.0 ** -24
BF16_EQUAL_FRACTION = 0.99

# max e, rms e per mode: >= 2x the emulated values recorded in CALIBRATION
F32_BOUNDS = {
    "f32_exact": (14.0, 1.1),
    "f32_split6": (28.0, 2.1),
    "bf16_wgrad": (4.0, 0.4),
}
# what the emulation measured (max e, rms e; the worse of 16-term blocks and sequential accumulation, over forward and weight
# gradient) at the CPU module's shapes.  The sequential split emulation adds each of the six piece products into the
# accumulator on its own (six roundings per term): the most pessimistic order a kernel could use.
CALIBRATION = {
    "f32_exact": (6.5, 0.51),
    "f32_split6": (12.0, 1.03),
    "bf16_wgrad": (1.9, 0.20),
}


# ------------------------------------------------------------------------------------------- rounding helpers
def bf16_rne(a):
    """-> float64 array of the bf16 values nearest (ties to even) to the fp32 values of `a`"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.bfloat16().double().numpy()


def bf16_trunc(a):
    """-> float64 array of `a` (fp32) truncated to bf16 (round toward zero): the mutant of a store without rounding"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


def split3(a):
    """exact split of fp32 values into three bf16 pieces: a = hi + mid + lo (each difference is exact in fp32)"""
    a = np.asarray(a, np.float32)
    hi = bf16_rne(a)
    r = (a.astype(np.float64) - hi).astype(np.float32)
    mid = bf16_rne(r)
    lo = bf16_rne((r.astype(np.float64) - mid).astype(np.float32))
    return hi, mid, lo


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------- pair lists
class Pairs:
    """pair lists grouped by offset: out[dst] += x[src] @ w[k] for (k, src, dst)"""

    def __init__(self, k, src, dst, K):
        k, src, dst = (np.asarray(a, np.int64) for a in (k, src, dst))
        self.K = K
        self.by_k = []
        for kk in range(K):
            sel = np.nonzero(k == kk)[0]
            self.by_k.append((src[sel], dst[sel]))

    @classmethod
    def from_oracle(cls, in_coords, out_coords, ks, ts_in):
        from oracle import oracle as orc
        if ks == 1:
            n = np.asarray(in_coords).shape[0]
            return cls(np.zeros(n), np.arange(n), np.arange(n), 1)
        k, i, o = orc.kernel_map(in_coords, out_coords, ks, ts_in)
        return cls(k, i, o, ks ** 3)

    def mirrored(self):
        """src <-> dst (the dgrad of this map, or the forward of its transposed convolution)"""
        m = Pairs.__new__(Pairs)
        m.K, m.by_k = self.K, [(d, s) for s, d in self.by_k]
        return m

    def terms_per_dst(self, n_dst):
        c = np.zeros(n_dst, np.int64)
        for _, d in self.by_k:
            np.add.at(c, d, 1)
        return c


# ------------------------------------------------------------------------------------------- fp64 references
def conv_ref(x, w, pairs, n_out, bias=None):
    """out[dst] += x[src] @ w[k]  ->  (ref, mag, n) [n_out, cout] in fp64 (x, w: the values the kernel multiplies)"""
    xt, wt = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64))
    cout = wt.shape[2]
    ref = torch.zeros((n_out, cout), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    xa, wa = xt.abs(), wt.abs()
    for kk, (s, d) in enumerate(pairs.by_k):
        if s.size == 0:
            continue
        st, dt = torch.from_numpy(s), torch.from_numpy(d)
        ref.index_add_(0, dt, xt.index_select(0, st) @ wt[kk])
        mag.index_add_(0, dt, xa.index_select(0, st) @ wa[kk])
    n = np.repeat((pairs.terms_per_dst(n_out) * xt.shape[1])[:, None], cout, 1)
    ref, mag = ref.numpy(), mag.numpy()
    if bias is not None:
        b = np.asarray(bias, np.float64).reshape(1, -1)
        ref, mag, n = ref + b, mag + np.abs(b), n + 1
    return ref, mag, n


def dgrad_ref(g, w, pairs, n_in):
    """gin[src] += g[dst] @ w[k]^T"""
    return conv_ref(g, np.asarray(w, np.float64).transpose(0, 2, 1), pairs.mirrored(), n_in)


def wgrad_ref(x, g, pairs):
    """gw[k] = sum over the pairs of offset k of x[src] (x) g[dst]  ->  (ref, mag, n) [K, cin, cout]"""
    xt, gt = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(g, np.float64))
    K, cin, cout = pairs.K, xt.shape[1], gt.shape[1]
    ref = torch.zeros((K, cin, cout), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    n = np.zeros((K, cin, cout), np.int64)
    for kk, (s, d) in enumerate(pairs.by_k):
        if s.size == 0:
            continue
        a, b = xt.index_select(0, torch.from_numpy(s)), gt.index_select(0, torch.from_numpy(d))
        ref[kk] = a.t() @ b
        mag[kk] = a.abs().t() @ b.abs()
        n[kk] = s.size
    return ref.numpy(), mag.numpy(), n


# ------------------------------------------------------------------------------------------- CPU emulation of the kernels' arithmetic
MODES = {
    # name: (pieces of each operand, piece pairs multiplied)
    "bf16": (1, [(0, 0)]),
    "f32_exact": (0, [(0, 0)]),
    "f32_split6": (3, [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]),
    "f32_split3": (3, [(0, 0), (0, 1), (1, 0)]),              # mutant: the cheaper split
}


def _pieces(a, mode):
    npc, _ = MODES[mode]
    if npc == 0:
        return [np.asarray(a, np.float32).astype(np.float64)]
    if npc == 1:
        return [bf16_rne(a)]
    return list(split3(a))


def emulate_conv(x, w, pairs, n_out, mode, block=16, bias=None, store=None, drop=None):
    """fp32 accumulation of out[dst] += x[src] @ w[k] as the kernel performs it: reduction channels in blocks of `block` (an
    exact block sum rounded into the fp32 accumulator; block=1 = sequential fp32), for every piece pair of `mode`.
    store: None (fp32 result), "rne" / "trunc" (bf16 store).  drop: callable(k, src, dst) -> keep mask (mutants)."""
    xp, wp = _pieces(x, mode), _pieces(w, mode)
    cin, cout = np.asarray(w).shape[1], np.asarray(w).shape[2]
    acc = np.zeros((n_out, cout), np.float32)
    for kk, (s, d) in enumerate(pairs.by_k):
        if drop is not None:
            keep = drop(kk, s, d)
            s, d = s[keep], d[keep]
        if s.size == 0:
            continue
        for c0 in range(0, cin, block):
            c1 = min(cin, c0 + block)
            for a, b in MODES[mode][1]:
                prod = xp[a][s, c0:c1] @ wp[b][kk, c0:c1]
                if mode == "f32_exact" and block == 1:
                    prod = f32(prod)                       # exact-fp32 MFMA: the product itself is rounded
                acc[d] = (acc[d].astype(np.float64) + f32(prod)).astype(np.float32)
    if bias is not None:
        acc = (acc.astype(np.float64) + np.asarray(bias, np.float64).reshape(1, -1)).astype(np.float32)
    if store == "rne":
        return bf16_rne(acc)
    if store == "trunc":
        return bf16_trunc(acc)
    return acc.astype(np.float64)


def emulate_wgrad(x, g, pairs, mode, block=16):
    """gw[k] = sum over pairs of x[src] (x) g[dst], pairs in blocks of `block` summed exactly and rounded into fp32"""
    xp, gp = _pieces(x, mode), _pieces(g, mode)
    K, cin, cout = pairs.K, np.asarray(x).shape[1], np.asarray(g).shape[1]
    acc = np.zeros((K, cin, cout), np.float32)
    for kk, (s, d) in enumerate(pairs.by_k):
        for p0 in range(0, s.size, block):
            ss, dd = s[p0:p0 + block], d[p0:p0 + block]
            for a, b in MODES[mode][1]:
                prod = xp[a][ss].T @ gp[b][dd]
                if mode == "f32_exact" and block == 1:
                    prod = f32(prod)
                acc[kk] = (acc[kk].astype(np.float64) + f32(prod)).astype(np.float32)
    return acc.astype(np.float64)


# ------------------------------------------------------------------------------------------- contracts
class ContractError(AssertionError):
    pass


def check_bf16(h, ref, mag, n, what=""):
    """contracts (a) and (b) of a bf16-stored output; -> report dict (margins > 1 mean "holds with room to spare")"""
    h = np.asarray(h, np.float64)
    assert h.shape == ref.shape, (what, h.shape, ref.shape)
    if h.size == 0:
        return {"what": what, "elements": 0}
    bound = 2.0 ** -8 * np.abs(ref) + 2.0 * n * U * mag
    err = np.abs(h - ref)
    bad = ~(err <= bound)                  # NaN counts as a violation
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    frac = float(np.mean(h == bf16_rne(ref)))
    rep = {"what": what, "elements": int(h.size), "max err/bound": worst, "bit-equal": frac,
           "margin (a)": (1.0 / worst) if worst > 0 else np.inf, "margin (b)": (1 - BF16_EQUAL_FRACTION) / max(1e-12, 1 - frac)}
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err - np.nan_to_num(bound), -np.inf))), h.shape)
        raise ContractError("%s: bf16 contract (a) violated at %d of %d elements; worst at %s: h=%r ref=%r bound=%r" % (
            what, int(bad.sum()), h.size, i, h[i], ref[i], bound[i]))
    if frac < BF16_EQUAL_FRACTION:
        raise ContractError("%s: bf16 contract (b): only %.4f of the elements equal the correctly rounded reference (need %.2f)" % (
            what, frac, BF16_EQUAL_FRACTION))
    return rep


def f32_errors(h, ref, mag):
    h = np.asarray(h, np.float64)
    err = np.abs(h - ref)
    scale = U * mag
    e = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0.0))
    e = np.where(np.isnan(h), np.inf, e)
    return e


def check_f32(h, ref, mag, mode, what=""):
    """max e and rms e of an fp32 output against the bounds of its arithmetic mode; -> report dict"""
    assert np.asarray(h).shape == ref.shape, (what, np.asarray(h).shape, ref.shape)
    e = f32_errors(h, ref, mag)
    if e.size == 0:
        return {"what": what, "elements": 0}
    emax, erms = float(e.max()), float(np.sqrt(np.mean(e ** 2)))
    bmax, brms = F32_BOUNDS[mode]
    rep = {"what": what, "mode": mode, "elements": int(e.size), "max e": emax, "rms e": erms,
           "margin max": bmax / emax if emax > 0 else np.inf, "margin rms": brms / erms if erms > 0 else np.inf}
    if not (emax <= bmax and erms <= brms):
        raise ContractError("%s: fp32 contract %s violated: max e %.3g (bound %.3g), rms e %.3g (bound %.3g)" % (
            what, mode, emax, bmax, erms, brms))
    return rep


def fmt(rep):
    return "  ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in rep.items())
