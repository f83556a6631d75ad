"""Independent float64 numpy restatement of every stage of the device augmentation chain (languagegroundedsemseg_amd/augment.py,
csrc/lgs_augment.hip), plus a numpy Philox-4x32-10.  Shares no code with the product; tests/test_augment_cpu.py holds it to the
reference's recorded outputs (tests/golden/augment.npz), tests/test_gpu_augment.py holds the kernels to it."""
import numpy as np


# ---- Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
def philox4x32_10(counter, k0, k1):
    """counter: uint32-valued [n, 4]; key words k0, k1 -> uint32 [n, 4]"""
    c = np.asarray(counter, dtype=np.uint64).reshape(-1, 4).copy()
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = m0 * c[:, 0], m1 * c[:, 2]
        c = np.stack([(p1 >> np.uint64(32)) ^ c[:, 1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[:, 3] ^ k1, p0 & mask], 1)
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c.astype(np.uint32)


def normal_from_words(w0, w1):
    """the device's Box-Muller sample, evaluated in float64: sqrt(-2 ln((w0 + 1) / 2^32)) cos(2 pi w1 / 2^32)"""
    u1 = (np.asarray(w0, np.float64) + 1.0) / 4294967296.0
    u2 = np.asarray(w1, np.float64) / 4294967296.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def elastic_noise(dims, seed, scene_seed, stage):
    """the device's noise block [dx, dy, dz, 3]: counter = (cell, component, stage, seed >> 32), key = (seed & 2^32-1, scene seed)"""
    cells = int(np.prod(dims))
    e = np.arange(cells * 3, dtype=np.uint64)
    ctr = np.stack([e // 3, e % 3, np.full_like(e, stage), np.full_like(e, (seed >> 32) & 0xffffffff)], 1)
    w = philox4x32_10(ctr, seed & 0xffffffff, scene_seed)
    return normal_from_words(w[:, 0], w[:, 1]).reshape(tuple(dims) + (3,))


# ---- elastic distortion
def t2_weights(d):
    """count(i, j) / 9 with count(i, j) = |{k in [0, d): |i - k| <= 1 and |k - j| <= 1}|, by counting"""
    w = np.zeros((d, d))
    for i in range(d):
        for j in range(d):
            w[i, j] = sum(1 for k in range(d) if abs(i - k) <= 1 and abs(k - j) <= 1) / 9.0
    return w


def noise_dims(points, granularity):
    """noise_dim of lib/transforms.py:241 in the reference's own float32 arithmetic"""
    p = np.asarray(points, np.float32)
    return ((p - p.min(0)).max(0) // np.float32(granularity)).astype(int) + 3


def elastic_field(noise):
    """two rounds of zero-padded 3-tap box blurs along x, y, z = T^2 per axis, float64"""
    f = np.asarray(noise, np.float64)
    f = np.einsum("ai,ijkc->ajkc", t2_weights(f.shape[0]), f)
    f = np.einsum("bj,ajkc->abkc", t2_weights(f.shape[1]), f)
    f = np.einsum("ck,abkd->abcd", t2_weights(f.shape[2]), f)
    return f


def elastic_stage(points, noise, granularity, magnitude):
    """one stage on one scene: points float32 [n, 3], noise [dx, dy, dz, 3] -> float64 [n, 3] (not rounded)"""
    p32 = np.asarray(points, np.float32)
    p = p32.astype(np.float64)
    dims = noise_dims(p32, granularity)
    assert tuple(dims) == tuple(noise.shape[:3]), (dims, noise.shape)
    field = elastic_field(noise)
    g = float(granularity)
    u = (p - (p32.min(0).astype(np.float64) - g)) / g                      # axes: min - g + k g
    inside = np.all((u >= 0) & (u <= dims - 1), axis=1)
    i0 = np.clip(np.floor(u).astype(np.int64), 0, dims - 2)
    t = u - i0
    val = np.zeros_like(p)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                w = (t[:, 0] if cx else 1 - t[:, 0]) * (t[:, 1] if cy else 1 - t[:, 1]) * (t[:, 2] if cz else 1 - t[:, 2])
                val += w[:, None] * field[i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz]
    val[~inside] = 0.0
    return p + val * float(magnitude)


# ---- flip / colour
def flip(coords, axes):
    """coords [n, 3] of one scene; axes: the flipped ones"""
    c = np.array(coords, copy=True)
    for a in axes:
        c[:, a] = c[:, a].max() - c[:, a]
    return c


def color_chain(feats, blend=None, translation=None, jitter_std=None, jitter_noise=None, scale=1.0, normalize=False,
                skip_constant_channels=False):
    """one scene's colours through autocontrast -> translation -> jitter -> scale -> normalise in float64;
    -> dict of the value after each stage that ran.  skip_constant_channels: the device's rule for hi == lo (left unblended)."""
    f = np.asarray(feats, np.float32).astype(np.float64)
    out = {}
    if blend is not None:
        lo, hi = f.min(0, keepdims=True), f.max(0, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            contrast = (f - lo) * (255.0 / (hi - lo))
            g = (1 - blend) * f + blend * contrast
        if skip_constant_channels:
            g = np.where(hi == lo, f, g)
        f = out["auto"] = g
    if translation is not None:
        f = out["trans"] = np.clip(f + np.asarray(translation, np.float64).reshape(1, 3), 0, 255)
    if jitter_std is not None:
        f = out["jitter"] = np.clip(f + np.asarray(jitter_noise, np.float64) * (jitter_std * 255), 0, 255)
    f = f * scale
    if normalize:
        f = f / 255.0 - 0.5
    out["final"] = f
    return out


def ulp32(x):
    """one float32 unit in the last place at magnitude |x|"""
    return float(np.spacing(np.float32(abs(x))))
