"""Per-op timings on the GPU (HIP events on torch's current stream) for the hot layer shapes.
usage: python tools/microbench.py [scenes | wide | wgrad | coarse | cluster | insseg | quantize | clip | pool | instnorm | strided | metrics | focal | supcon | augment | paste | dropout | instshift | fps | nearest | ap | lean]"""
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import MinkowskiEngine as ME
from languagegroundedsemseg_amd.synthetic import make_batch

DEV = "cuda:0"


def timeit(fn, iters=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    coords, feats, labels = make_batch(list(range(B)), n_target=150000, shift_seed=0)
    if os.environ.get("LGS_MB_SORT") == "1":   # experiment: spatially sorted input rows instead of the dataset's arbitrary order
        from languagegroundedsemseg_amd.synthetic import morton_order
        perm = morton_order(coords)
        coords, feats, labels = coords[perm], feats[perm], labels[perm]
        print("input rows in Morton order")
    c = torch.from_numpy(coords).to(DEV)
    n = coords.shape[0]
    print("voxels", n)
    t0 = time.time()
    x = ME.SparseTensor(torch.from_numpy(feats).to(DEV), c)
    torch.cuda.synchronize()
    print("insert (first call, incl. lib load) %.1f ms" % ((time.time() - t0) * 1e3))

    def build_maps():
        xx = ME.SparseTensor(torch.zeros(n, 3, device=DEV), c)
        m = xx.coordinate_manager
        k = xx.coordinate_map_key
        for lvl in range(5):
            m.kernel_map_handle(k, k, 3)
            if lvl < 4:
                k2 = m.stride(k, 2)
                m.kernel_map_handle(k, k2, 2)
                k = k2
    print("all maps (5x 3^3 + 4x 2^3 + 4 strides + insert): %.2f ms" % timeit(build_maps, 3, 1))

    mgr, k0 = x.coordinate_manager, x.coordinate_map_key
    km = mgr.kernel_map_handle(k0, k0, 3)
    kk, ii, oo = km.export()
    M = kk.shape[0]
    print("3^3 pairs at L0: %d (%.2f per voxel)" % (M, M / n))
    for dtype in (torch.bfloat16, torch.float32):
        e = 2 if dtype == torch.bfloat16 else 4
        for cin, cout in ((96, 96), (128, 96), (32, 32)):
            f = torch.randn(n, cin, device=DEV).to(dtype)
            g = torch.randn(n, cout, device=DEV).to(dtype)
            w = torch.randn(27, cin, cout, device=DEV) * 0.05
            tf = timeit(lambda: km.conv_forward(f, w, None, False))
            td = timeit(lambda: km.conv_dgrad(g, w, False))
            tw = timeit(lambda: km.conv_wgrad(f, g, False))
            flop = 2.0 * M * cin * cout
            bf = M * cin * e + n * cout * e + 8 * M + 27 * cin * cout * e
            print("%-9s %3d->%3d  fwd %.3f ms (%.1f TF, %.2f TB/s alg)  dgrad %.3f ms  wgrad %.3f ms (%.1f TF)" % (
                str(dtype).split(".")[1], cin, cout, tf, flop / tf / 1e9, bf / tf / 1e9, td, tw, flop / tw / 1e9))
        f = torch.randn(n, 96, device=DEV).to(dtype)
        bn = ME.MinkowskiBatchNorm(96).to(DEV)
        sx = ME.SparseTensor(f.clone().requires_grad_(True), coordinate_map_key=k0, coordinate_manager=mgr)
        tb = timeit(lambda: bn(sx, relu=True))
        print("%-9s BN+ReLU fwd 96ch %.3f ms (%.2f TB/s of 3*N*C*e)" % (str(dtype).split(".")[1], tb, 3 * n * 96 * e / tb / 1e9))
        be = ME.get_backend()
        g1, b1 = torch.ones(96, device=DEV), torch.zeros(96, device=DEV)
        rm, rv = torch.zeros(96, device=DEV), torch.ones(96, device=DEV)
        y, st = be.bn_forward(f, g1, b1, 1e-5, 0.1, rm, rv, None, 1)
        dy = torch.randn_like(f)
        for mode, want in ((2, False), (1, True)):
            t_all = timeit(lambda: be.bn_backward(f, y, dy, g1, b1, st, mode, want))
            t_red = timeit(lambda: be.bn_backward_reduce(f, y, dy, g1, b1, st, mode))
            sums = be.bn_backward_reduce(f, y, dy, g1, b1, st, mode)
            t_app = timeit(lambda: be.bn_backward_apply(f, y, dy, g1, b1, st, sums, 1.0 / n, mode, want))
            nt = (5 if mode == 2 else 7) + (1 if want else 0)
            print("%-9s BN bwd 96ch relu-mode %d res %d: %.3f ms (%.2f TB/s of %d*N*C*e)  reduce %.3f  apply %.3f" % (
                str(dtype).split(".")[1], mode, want, t_all, nt * n * 96 * e / t_all / 1e9, nt, t_red, t_app))


def clip():
    """MFMA sub-report: S = normalize(F) . normalize(T)^T, [N,C] x [C,200]"""
    n = 1200000
    for c in (512, 96):
        for dtype in (torch.bfloat16, torch.float32):
            f = torch.randn(n, c, device=DEV).to(dtype)
            t = torch.randn(200, c, device=DEV)
            be = ME.get_backend()
            ms = timeit(lambda: be.clip_similarity(f, t))
            flop = 2.0 * n * c * 200
            byts = n * c * f.element_size() + n * 200 * 4
            print("clip similarity N=%d C=%d %-8s %.3f ms  %.1f TFLOP/s  %.2f TB/s (read F + write S)" % (
                n, c, str(dtype).split(".")[1], ms, flop / ms / 1e9, byts / ms / 1e9))
            lab = torch.randint(-1, 200, (n,), device=DEV)
            neg = torch.randint(0, 200, (n, 3), device=DEV)
            ms = timeit(lambda: be.clip_loss_forward(f, t, lab, neg, -1))
            byts = n * c * f.element_size() + n * (3 * 4 + 8 + 4 * 8)
            print("fused clip loss fwd (d_pos, d_neg, argmax, 1/|f|; no S) %.3f ms  %.1f TFLOP/s (%.1f %% of 2.5 PF)  %.2f TB/s "
                  "(%.1f %% of 8 TB/s)" % (ms, flop / ms / 1e9, flop / ms / 1e9 / 2500.0 * 100.0, byts / ms / 1e9, byts / ms / 1e9 / 8.0 * 100.0))
            d_pos, d_neg, pred, saved, _ = be.clip_loss_forward(f, t, lab, neg, -1)
            gp, gn = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
            ms = timeit(lambda: be.clip_loss_backward(saved, d_pos, d_neg, gp, gn, -1))
            byts = 2 * n * c * f.element_size()
            print("fused clip loss bwd (4-sparse upstream) %.3f ms  %.2f TB/s (read F + write gF)" % (ms, byts / ms / 1e9))


def quantize():
    """raw points -> voxel coordinates on the device (voxelize + dedup + label vote)"""
    import numpy as np
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    rep = np.repeat(coords, 2, 0)                                   # ~2 points per voxel, like a 2 cm voxelisation of ScanNet
    pts = (rep[:, 1:].astype(np.float64) + rng.uniform(0.05, 0.95, (rep.shape[0], 3))) * 0.02
    p = torch.from_numpy(pts.astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.repeat(labels, 2)).to(DEV)
    n = p.shape[0]
    tv = timeit(lambda: ME.utils.voxelize(p, quantization_size=0.02))
    tq = timeit(lambda: ME.utils.sparse_quantize(p, None, lab, ignore_label=-1, quantization_size=0.02, return_index=True))
    print("voxelize %d points: %.3f ms (%.2f TB/s of 28 B/point)" % (n, tv, n * 28 / tv / 1e9))
    print("sparse_quantize (voxelize + dedup + label vote) %d points -> voxels: %.3f ms (%.1f M points/s)" % (n, tq, n / tq / 1e3))
    import time
    m = 300000                                                      # bounded CPU sample of the same workload (host path = numpy)
    ph, lh = p[:m].cpu(), lab[:m].cpu()
    t0 = time.perf_counter()
    ME.utils.sparse_quantize(ph, None, lh, ignore_label=-1, quantization_size=0.02, return_index=True)
    tc = time.perf_counter() - t0
    print("host path (numpy, 1 core) on the first %d points: %.1f ms (%.2f M points/s)" % (m, tc * 1e3, m / tc / 1e6))


def insseg():
    """instance-seg model (trunk + offset head), CE + offset losses, forward + backward, bf16"""
    import numpy as np
    from languagegroundedsemseg_amd import models
    from languagegroundedsemseg_amd.losses import fused_cross_entropy, instance_offset_losses
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    c = torch.from_numpy(coords).to(DEV)
    f = torch.from_numpy(feats).to(DEV).bfloat16()
    lab = torch.from_numpy(labels).to(DEV)
    rng = np.random.default_rng(0)
    inst = torch.from_numpy(rng.integers(-1, 30, coords.shape[0])).to(DEV)
    centers = (c[:, 1:].float() + torch.randn(coords.shape[0], 3, device=DEV) * 20)

    class Cfg:
        bn_momentum, conv1_kernel_size = 0.02, 3
    m = models.load_model("InsSegRes16UNet34C")(3, 200, Cfg()).to(DEV).train()

    def step():
        for p in m.parameters():
            p.grad = None
        x = ME.SparseTensor(f, c)
        off, logits, _ = m(x)
        nl, dl = instance_offset_losses(off.F, c[:, 1:], centers, inst, 0.02)
        (fused_cross_entropy(logits.F, lab, ignore_index=-1) + nl + dl).backward()
    t = timeit(step)
    print("InsSegRes16UNet34C fwd+bwd (CE + offset losses, incl. map build) %d voxels: %.2f ms = %.1f M voxels/s" % (
        coords.shape[0], t, coords.shape[0] / t / 1e3))
    insseg_targets(coords, c, inst, centers)


def insseg_targets(coords, c, inst, centers):
    """the instance targets of that batch: the torch lines the trainer runs on uploaded centres (forward + backward) against
    instance_info + fused_instance_offset_losses + backward, and the host time of get_instance_info's numpy restatement for one scene"""
    import time
    from languagegroundedsemseg_amd import instances
    from languagegroundedsemseg_amd.losses import fused_instance_offset_losses, instance_offset_losses
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    n = coords.shape[0]
    po = (torch.randn(n, 3, device=DEV) * 0.3).bfloat16().requires_grad_(True)
    xyz = c[:, 1:].contiguous()

    def torch_lines():
        po.grad = None
        nl, dl = instance_offset_losses(po, xyz, centers, inst, 0.02)
        (nl + dl).backward()

    def fused(targets=True, info=[None]):
        po.grad = None
        if targets or info[0] is None:
            info[0] = instances.instance_info(c, inst, return_centers=False)
        nl, dl = fused_instance_offset_losses(po, c, info[0], 0.02)
        (nl + dl).backward()
    # 200 calls per window, three windows each, the variants alternating: medians, and the spread of the three in brackets
    variants = [("offset losses, torch lines on given centres, fwd + bwd", torch_lines),
                ("instance_info + fused offset losses, fwd + bwd", fused),
                ("  fused offset losses alone, fwd + bwd", lambda: fused(False)),
                ("  instance_info alone (table, ids, slots)", lambda: instances.instance_info(c, inst, return_centers=False)),
                ("  instance_info with the [n, 3] centres", lambda: instances.instance_info(c, inst))]
    times = [[] for _ in variants]
    for _ in range(3):
        for k, (_, fn) in enumerate(variants):
            times[k].append(timeit(fn, 200, 5))
    print("instance targets, %d voxels, bf16 offsets:" % n)
    for (name, _), t in zip(variants, times):
        print("%-66s %9.3f ms   [%.3f .. %.3f]" % (name, sorted(t)[1], min(t), max(t)))
    import insttarget_reference as ir          # the tests' numpy restatement of get_instance_info (one sort + segment reductions)
    rows = coords[:, 0] == 0
    xyz0, ids0 = coords[rows, 1:], inst.cpu().numpy()[rows]
    ir.get_instance_info(xyz0, ids0)
    t0 = time.perf_counter()
    for _ in range(5):
        ir.get_instance_info(xyz0, ids0)
    t_host = (time.perf_counter() - t0) * 1e3 / 5
    print("host: numpy restatement of get_instance_info, ONE scene (%d voxels, %d ids) %9.3f ms" % (xyz0.shape[0], len(np.unique(ids0)), t_host))


def cluster():
    """PointGroup proposal clustering of one scene (ball query radius 3 cm + same-label components)"""
    import time
    import numpy as np
    from languagegroundedsemseg_amd.pointgroup import cluster_points
    from oracle import oracle as orc
    coords, feats, labels = make_batch([0], n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    xyz = (coords[:, 1:].astype(np.float32) + rng.uniform(0.2, 0.8, (coords.shape[0], 3)).astype(np.float32)) * np.float32(0.02)
    blk = np.floor(xyz / np.float32(0.4)).astype(np.int64)
    sem = ((blk[:, 0] * 3 + blk[:, 1] * 5 + blk[:, 2] * 7) % 7).astype(np.int32)
    x, s = torch.from_numpy(xyz).to(DEV), torch.from_numpy(sem).to(DEV)
    t = timeit(lambda: cluster_points(x, s, 0.03, 50))
    idx, off = cluster_points(x, s, 0.03, 50)
    print("cluster_points %d points -> %d clusters: %.3f ms (%.1f M points/s)" % (xyz.shape[0], off.shape[0] - 1, t, xyz.shape[0] / t / 1e3))
    m = 30000
    t0 = time.perf_counter()
    orc.pointgroup_clusters(xyz[:m], sem[:m], 0.03, 50)
    tc = time.perf_counter() - t0
    print("oracle (KD-tree + python BFS, 1 core) on the first %d points: %.0f ms (%.3f M points/s)" % (m, tc * 1e3, m / tc / 1e6))


def coarse():
    """coarse-level layer shapes (L2..L4 of an 8-scene batch)"""
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    c = torch.from_numpy(coords).to(DEV)
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 3, device=DEV), c)
    m = x.coordinate_manager
    k = x.coordinate_map_key
    for lvl in range(1, 5):
        k = m.stride(k, 2)
        n = m.size(k)
        km = m.kernel_map_handle(k, k, 3)
        M = km.export()[0].shape[0]
        for cin, cout in {1: [(32, 32), (96, 96)], 2: [(64, 64), (128, 128)], 3: [(128, 128), (256, 256)], 4: [(256, 256)]}[lvl]:
            f = torch.randn(n, cin, device=DEV).bfloat16()
            g = torch.randn(n, cout, device=DEV).bfloat16()
            w = torch.randn(27, cin, cout, device=DEV) * 0.05
            tf = timeit(lambda: km.conv_forward(f, w, None, False), 10, 3)
            tw = timeit(lambda: km.conv_wgrad(f, g, False), 10, 3)
            flop = 2.0 * M * cin * cout
            print("L%d rows %7d pairs %8d  %3d->%3d  fwd %.3f ms (%.0f TF)  wgrad %.3f ms (%.0f TF)" % (
                lvl, n, M, cin, cout, tf, flop / tf / 1e9, tw, flop / tw / 1e9))


def wgrad():
    """every weight-gradient shape of a Res16UNet34C step on the maps of the 8-scene batch (bf16)"""
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    c = torch.from_numpy(coords).to(DEV)
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 3, device=DEV), c)
    m = x.coordinate_manager
    keys = [x.coordinate_map_key]
    for lvl in range(4):
        keys.append(m.stride(keys[-1], 2))
    # (level, kernel, cin, cout, transposed, count per step)
    if os.environ.get("LGS_WGRAD_DBG"):
        shapes_sel = [(0, 3, 96, 96, 0, 3), (0, 3, 128, 96, 0, 1), (1, 3, 96, 96, 0, 3)]
    shapes = [(0, 3, 3, 32, 0, 1), (0, 3, 128, 96, 0, 1), (0, 3, 96, 96, 0, 3), (0, 2, 32, 32, 0, 1), (0, 2, 96, 96, 1, 1),
              (1, 3, 32, 32, 0, 4), (1, 3, 128, 96, 0, 1), (1, 3, 96, 96, 0, 3), (1, 2, 32, 32, 0, 1), (1, 2, 128, 96, 1, 1),
              (2, 3, 32, 64, 0, 1), (2, 3, 64, 64, 0, 5), (2, 3, 192, 128, 0, 1), (2, 3, 128, 128, 0, 3), (2, 2, 64, 64, 0, 1), (2, 2, 256, 128, 1, 1),
              (3, 3, 64, 128, 0, 1), (3, 3, 128, 128, 0, 7), (3, 3, 384, 256, 0, 1), (3, 3, 256, 256, 0, 3), (3, 2, 128, 128, 0, 1), (3, 2, 256, 256, 1, 1),
              (4, 3, 128, 256, 0, 1), (4, 3, 256, 256, 0, 11)]
    tot = 0.0
    if os.environ.get("LGS_WGRAD_DBG"):
        shapes = shapes_sel
    for lvl, ks, cin, cout, tr, cnt in shapes:
        if ks == 3:
            km = m.kernel_map_handle(keys[lvl], keys[lvl], 3)
            n_in = n_out = m.size(keys[lvl])
        else:
            km = m.kernel_map_handle(keys[lvl], keys[lvl + 1], 2)
            n_in, n_out = (m.size(keys[lvl + 1]), m.size(keys[lvl])) if tr else (m.size(keys[lvl]), m.size(keys[lvl + 1]))
        M = km.export()[0].shape[0]
        f = torch.randn(n_in, cin, device=DEV).bfloat16()
        g = torch.randn(n_out, cout, device=DEV).bfloat16()
        tw = timeit(lambda: km.conv_wgrad(f, g, bool(tr)), 10, 3)
        flop = 2.0 * M * cin * cout
        byts = M * (cin + cout) * 2 + 8 * M
        tot += tw * cnt
        print("L%d k%d%s %3d->%3d rows %7d pairs %8d x%-2d  wgrad %.3f ms (%.0f TF, %.2f TB/s alg)" % (
            lvl, ks, "T" if tr else " ", cin, cout, n_out, M, cnt, tw, flop / tw / 1e9, byts / tw / 1e9))
    print("sum over a step (stand-alone launches): %.2f ms" % tot)


def wide():
    """the wide-channel launches of the CLIP pretrain model (Res16UNet34D, BASELINE configs[2]) on the 8-scene maps"""
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    coords, feats, labels = make_batch(list(range(B)), n_target=150000, shift_seed=0)
    c = torch.from_numpy(coords).to(DEV)
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 3, device=DEV), c)
    m = x.coordinate_manager
    keys = [x.coordinate_map_key]
    for lvl in range(2):
        keys.append(m.stride(keys[-1], 2))
    for lvl, cin, cout in ((0, 512, 512), (0, 640, 512), (1, 256, 256), (1, 512, 256), (2, 256, 256)):
        km = m.kernel_map_handle(keys[lvl], keys[lvl], 3)
        n = m.size(keys[lvl])
        M = km.export()[0].shape[0]
        f = torch.randn(n, cin, device=DEV).bfloat16()
        g = torch.randn(n, cout, device=DEV).bfloat16()
        w = torch.randn(27, cin, cout, device=DEV) * 0.02
        tf = timeit(lambda: km.conv_forward(f, w, None, False), 3, 1)
        td = timeit(lambda: km.conv_dgrad(g, w, False), 3, 1)
        tw = timeit(lambda: km.conv_wgrad(f, g, False), 3, 1)
        flop = 2.0 * M * cin * cout
        print("L%d 3^3 %3d->%3d rows %7d pairs %8d  fwd %.3f ms (%.0f TF = %.1f %% of 2.5 PF)  dgrad %.3f ms (%.0f TF)  wgrad %.3f ms (%.0f TF)" % (
            lvl, cin, cout, n, M, tf, flop / tf / 1e9, flop / tf / 1e9 / 25, td, flop / td / 1e9, tw, flop / tw / 1e9))
    # the other wide launches of Res16UNet34D at level 0: 1x1 downsample 544 -> 512, transposed 2^3 256 -> 512 (level 1 -> 0)
    n0 = m.size(keys[0])
    km1 = m.kernel_map_handle(keys[0], keys[0], 1)
    f = torch.randn(n0, 544, device=DEV).bfloat16()
    g = torch.randn(n0, 512, device=DEV).bfloat16()
    w = torch.randn(1, 544, 512, device=DEV) * 0.02
    tf = timeit(lambda: km1.conv_forward(f, w, None, False), 3, 1)
    td = timeit(lambda: km1.conv_dgrad(g, w, False), 3, 1)
    print("L0 1x1 544->512 rows %7d  fwd %.3f ms (%.0f TF)  dgrad %.3f ms (%.0f TF)" % (n0, tf, 2.0 * n0 * 544 * 512 / tf / 1e9, td, 2.0 * n0 * 544 * 512 / td / 1e9))
    km2 = m.kernel_map_handle(keys[0], keys[1], 2)
    n1 = m.size(keys[1])
    f = torch.randn(n1, 256, device=DEV).bfloat16()
    w = torch.randn(8, 256, 512, device=DEV) * 0.02
    tf = timeit(lambda: km2.conv_forward(f, w, None, True), 3, 1)
    td = timeit(lambda: km2.conv_dgrad(g, w, True), 3, 1)
    print("L1->L0 transposed 2^3 256->512 rows %7d  fwd %.3f ms (%.0f TF)  dgrad %.3f ms (%.0f TF)" % (n0, tf, 2.0 * n0 * 256 * 512 / tf / 1e9, td, 2.0 * n0 * 256 * 512 / td / 1e9))

def pool():
    """pooling / global pooling / broadcast on the 8-scene level-0 map (C = 96, bf16): us per op and the fraction of 8 TB/s on
    algorithmic bytes (features read + written once, int32 index arrays read once, arg-max rows written / read once)"""
    be = ME.get_backend()
    coords, _, _ = make_batch(list(range(8)), voxel=0.02, n_target=150000)
    c = torch.from_numpy(coords).to(DEV)
    C, e = 96, 2
    x = ME.SparseTensor(torch.randn(c.shape[0], C, device=DEV).bfloat16(), c)
    m, k0 = x.coordinate_manager, x.coordinate_map_key
    n0 = m.size(k0)
    k1, k3, ko = m.coarser_key(k0, 2), m.coarser_key(k0, 8), m.origin_key()
    n1, n3, nb = m.size(k1), m.size(k3), m.size(ko)
    s1, s3, so = m.segment_map_handle(k0, k1), m.segment_map_handle(k0, k3), m.segment_map_handle(k0, ko)
    f0 = x.F
    y1 = torch.randn(n1, C, device=DEV).bfloat16()
    y3 = torch.randn(n3, C, device=DEV).bfloat16()
    g = torch.randn(nb, C, device=DEV).bfloat16()
    _, amax = be.pool_reduce(s1, "max", f0)
    torch.cuda.synchronize()
    peak = 8e12
    print("level 0: %d rows, level 1: %d, level 3: %d, %d batch items; C = %d bf16" % (n0, n1, n3, nb, C))
    rows = [
        ("sum pool (2,2) fwd", lambda: be.pool_reduce(s1, "sum", f0), (n0 + n1) * C * e + n0 * 4 + n1 * 4),
        ("avg pool (2,2) fwd", lambda: be.pool_reduce(s1, "avg", f0), (n0 + n1) * C * e + n0 * 4 + n1 * 4),
        ("max pool (2,2) fwd", lambda: be.pool_reduce(s1, "max", f0), (n0 + n1) * C * e + n1 * C * 4 + n0 * 4 + n1 * 4),
        ("sum pool (2,2) bwd", lambda: be.pool_broadcast(s1, "copy", y1), (n0 + n1) * C * e + n0 * 8),
        ("avg pool (2,2) bwd", lambda: be.pool_broadcast(s1, "scale", y1), (n0 + n1) * C * e + n0 * 8 + n1 * 4),
        ("max pool (2,2) bwd", lambda: be.pool_max_backward(s1, y1, amax), (n0 + n1) * C * e + n1 * C * 4 + n0 * 8),
        ("PoolingTranspose (8,8) fwd", lambda: be.pool_broadcast(s3, "copy", y3), (n0 + n3) * C * e + n0 * 8),
        ("PoolingTranspose (8,8) bwd", lambda: be.pool_reduce(s3, "sum", f0), (n0 + n3) * C * e + n0 * 4 + n3 * 4),
        ("global avg pool fwd", lambda: be.pool_reduce(so, "avg", f0), (n0 + nb) * C * e + n0 * 4),
        ("global avg pool bwd", lambda: be.pool_broadcast(so, "scale", g), (n0 + nb) * C * e + n0 * 8),
        ("broadcast mul fwd", lambda: be.pool_broadcast(so, "mul", g, f0), (2 * n0 + nb) * C * e + n0 * 8),
        ("broadcast mul bwd (d g)", lambda: be.pool_reduce(so, "prod", f0, f0), (2 * n0 + nb) * C * e + n0 * 4),
    ]
    for name, fn, nbytes in rows:
        t = timeit(fn, 20, 3)
        print("%-28s %8.1f us  %6.1f MB  %.2f TB/s  %.2f of 8 TB/s" % (name, t * 1e3, nbytes / 1e6, nbytes / t / 1e9, nbytes / t / 1e9 * 1e12 / peak))


def instnorm():
    """MinkowskiInstanceNorm on the 8-scene batch: the engine kernels, the torch lines (INSTANCE_NORM=0, same process, same
    tensors, alternating) and BatchNorm (lgs_bn_forward / lgs_bn_backward, training mode) on the same tensor.  Algorithmic bytes:
    forward 3 N C e + 4 N (x twice, y once, the scene index per row), backward 5 N C e + 4 N (x and dy twice, dx once)."""
    from languagegroundedsemseg_amd import engine
    be = ME.get_backend()
    coords, _, _ = make_batch(list(range(8)), voxel=0.02, n_target=150000)
    x0 = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), torch.from_numpy(coords).to(DEV))
    m, k0 = x0.coordinate_manager, x0.coordinate_map_key
    keys = {0: k0, 2: m.coarser_key(k0, 4)}
    peak = 8e12
    for level, C, dtype in [(0, 96, torch.bfloat16), (0, 96, torch.float32), (0, 512, torch.bfloat16), (0, 512, torch.float32),
                            (2, 128, torch.bfloat16), (2, 128, torch.float32)]:
        key = keys[level]
        n, e = m.size(key), (2 if dtype == torch.bfloat16 else 4)
        f = torch.randn(n, C, device=DEV).to(dtype).requires_grad_(True)
        dy = torch.randn(n, C, device=DEV).to(dtype)
        st = ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=m)
        mod = ME.MinkowskiInstanceNorm(C).to(DEV)
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
        fd = f.detach()
        bwd_bytes, fwd_bytes = 5 * n * C * e + 4 * n, 3 * n * C * e + 4 * n
        print("level %d: %d rows, %d scenes, C = %d %s" % (level, n, m.size(m.origin_key()), C, str(dtype).replace("torch.", "")))
        res = {}
        for rep in range(2):                       # alternating: engine, torch lines, engine, torch lines
            for knob in (1, 0):
                with engine.tuning(INSTANCE_NORM=knob):
                    out = mod(st).F
                    tf = timeit(lambda: mod(st).F, 10 if knob else 3, 2)
                    tb = timeit(lambda: out.backward(dy, retain_graph=True), 10 if knob else 3, 2)
                    f.grad = None
                    del out
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    mod(st).F.backward(dy)
                    torch.cuda.synchronize()
                    pk = torch.cuda.max_memory_allocated() - base
                    f.grad = None
                res[knob] = (min(tf, res[knob][0]) if knob in res else tf, min(tb, res[knob][1]) if knob in res else tb, pk)
        y, stats = be.bn_forward(fd, gamma, beta, 1e-5, 0.1, rm, rv, None, 0, nbt)
        tbf = timeit(lambda: be.bn_forward(fd, gamma, beta, 1e-5, 0.1, rm, rv, None, 0, nbt), 10, 2)
        tbb = timeit(lambda: be.bn_backward(fd, y, dy, gamma, beta, stats, 0, False), 10, 2)
        del y
        for name, t, nbytes in [("instance norm fwd (engine)", res[1][0], fwd_bytes), ("instance norm bwd (engine)", res[1][1], bwd_bytes),
                                ("instance norm fwd (INSTANCE_NORM=0)", res[0][0], fwd_bytes),
                                ("instance norm bwd (INSTANCE_NORM=0)", res[0][1], bwd_bytes),
                                ("lgs_bn_forward", tbf, fwd_bytes - 4 * n), ("lgs_bn_backward", tbb, bwd_bytes - 4 * n)]:
            print("%-36s %9.1f us  %7.1f MB  %.2f TB/s  %.2f of 8 TB/s" % (name, t * 1e3, nbytes / 1e6, nbytes / t / 1e9, nbytes / t / 1e9 * 1e12 / peak))
        print("%-36s fwd %.2f x, bwd %.2f x faster than the torch lines; %.2f x / %.2f x BatchNorm's time" % (
            "  engine", res[0][0] / res[1][0], res[0][1] / res[1][1], res[1][0] / tbf, res[1][1] / tbb))
        print("%-36s engine %.1f MB, INSTANCE_NORM=0 %.1f MB (x is %.1f MB)" % ("  peak memory of one fwd + bwd", res[1][2] / 1e6, res[0][2] / 1e6, n * C * e / 1e6))
        del f, dy, st, fd


def strided():
    """the kernel maps of lgs_manager_kernel_map_ex on the 8-scene batch, levels 0 and 1 (bf16): the three builders, and forward /
    dgrad / wgrad of 64 -> 128 and 256 -> 512 on the 3^3 stride-2 map and a dilation-2 map, each beside the stride-1 3^3 conv of the
    same level and channels from the same run.  Rates are REAL pairs per second (pairs = exported triples of the map)."""
    coords, _, _ = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    c = torch.from_numpy(coords).to(DEV)
    n0 = coords.shape[0]

    def fresh(level):
        x = ME.SparseTensor(torch.zeros(n0, 1, device=DEV), c)
        m, k = x.coordinate_manager, x.coordinate_map_key
        for _ in range(level):
            k = m.stride(k, 2)
        return x, m, k, m.stride(k, 2)

    for level in (0, 1):
        # builders: a fresh manager per call (the maps are cached per manager), its cost measured alone and subtracted
        base = timeit(lambda: fresh(level), 5, 2)
        for name, ks, to_coarse, d in (("3^3 stride 1", 3, False, 1), ("3^3 dilation 2", 3, False, 2), ("3^3 stride 2 (both views)", 3, True, 1),
                                       ("1x1 stride 2 (both views)", 1, True, 1)):
            def build():
                x, m, k, kc = fresh(level)
                m.kernel_map_handle(k, kc if to_coarse else k, ks, d)
            t = timeit(build, 5, 2)
            print("L%d builder %-26s %.3f ms (insert + strides alone: %.3f ms)" % (level, name, t - base, base))
        x, m, k, kc = fresh(level)
        nf, nc = m.size(k), m.size(kc)
        kms = {"stride 1": (m.kernel_map_handle(k, k, 3), nf, nf), "dilation 2": (m.kernel_map_handle(k, k, 3, 2), nf, nf),
               "stride 2": (m.kernel_map_handle(k, kc, 3), nf, nc)}
        for cin, cout in ((64, 128), (256, 512)):
            w = torch.randn(27, cin, cout, device=DEV) * 0.02
            ref = None
            for name, (km, n_in, n_out) in kms.items():
                M = km.export()[0].shape[0]
                f = torch.randn(n_in, cin, device=DEV).bfloat16()
                g = torch.randn(n_out, cout, device=DEV).bfloat16()
                tf = timeit(lambda: km.conv_forward(f, w, None, False), 5, 2)
                td = timeit(lambda: km.conv_dgrad(g, w, False), 5, 2)
                tw = timeit(lambda: km.conv_wgrad(f, g, False), 5, 2)
                rate = [M / t / 1e6 for t in (tf, td, tw)]                  # G pairs / s
                if ref is None:
                    ref = rate
                print("L%d %-10s %3d->%3d rows %7d -> %7d pairs %8d  fwd %.3f ms  dgrad %.3f ms  wgrad %.3f ms  | G pairs/s %.2f %.2f %.2f  "
                      "(x stride 1: %.2f %.2f %.2f)" % (level, name, cin, cout, n_in, n_out, M, tf, td, tw, rate[0], rate[1], rate[2],
                                                        rate[0] / ref[0], rate[1] / ref[1], rate[2] / ref[2]))
                del f, g


def metrics():
    """lgs_seg_metrics on [1.2 M, 200] scores (bf16 / fp32, with and without prob, uniform labels and a skewed set where 90 % of the
    rows share one (label, pred) cell) beside the torch composition it replaces (max(1) + softmax + masked bincount), all variants
    alternating inside this process; then the grid knob METRICS_BLOCKS.  Algorithmic bytes: n c e + 8 n read, 8 n written, + 4 n c
    for prob.  min / median over the rounds."""
    from languagegroundedsemseg_amd import engine
    from languagegroundedsemseg_amd.metrics import SegmentationMeter
    n, c, peak, rounds = 1200000, 200, 8e12, 3
    g = torch.Generator(device=DEV).manual_seed(0)
    base = torch.randn(n, c, device=DEV, generator=g)
    lab_u = torch.randint(0, c, (n,), device=DEV, generator=g)
    lab_u[torch.rand(n, device=DEV, generator=g) < 0.1] = -1
    hot = torch.rand(n, device=DEV, generator=g) < 0.9          # rows of the one hot cell (label 3, pred 7), scattered over the batch
    skew = base.clone()
    skew[hot, 7] = 10.0
    lab_s = torch.where(hot, torch.full_like(lab_u, 3), lab_u)
    meter = SegmentationMeter(c).to(DEV)

    def torch_lines(x, lab, want_prob):
        pred = x.max(1)[1]
        prob = torch.softmax(x.float(), 1) if want_prob else None
        k = (lab >= 0) & (lab < c) & (lab != -1)
        meter.confmat += torch.bincount(c * lab[k] + pred[k], minlength=c * c).view(c, c)
        return pred, prob

    def report(name, ts, nbytes):
        t, med = min(ts), sorted(ts)[len(ts) // 2]
        print("%-58s %8.1f us (median %8.1f)  %7.1f MB  %.2f TB/s  %.2f of 8 TB/s" % (name, t * 1e3, med * 1e3, nbytes / 1e6, nbytes / t / 1e9,
                                                                                     nbytes / t / 1e9 * 1e12 / peak))
        return t

    for dtype in (torch.bfloat16, torch.float32):
        e = 2 if dtype == torch.bfloat16 else 4
        xs = {"uniform": (base.to(dtype), lab_u), "skewed": (skew.to(dtype), lab_s)}
        times = {}
        for rnd in range(rounds):                      # alternating: every variant once per round
            for want_prob in (False, True):
                for dist_name, (x, lab) in xs.items():
                    times.setdefault(("kernel", want_prob, dist_name), []).append(timeit(lambda: meter.update(x, lab, want_prob=want_prob), 20, 3))
                    times.setdefault(("torch", want_prob, dist_name), []).append(timeit(lambda: torch_lines(x, lab, want_prob), 4, 1))
        best = {}
        for (who, want_prob, dist_name), ts in times.items():
            nbytes = n * c * e + 16 * n + (4 * n * c if want_prob else 0)
            label = "%s %s %s labels %s" % ("lgs_seg_metrics" if who == "kernel" else "torch max+softmax+bincount" if want_prob else "torch max+bincount",
                                            str(dtype).split(".")[1], dist_name, "+ prob" if want_prob else "no prob")
            best[(who, want_prob, dist_name)] = report(label, ts, nbytes)
        for want_prob in (False, True):
            print("  %s %s: kernel %.2f x faster than the torch lines (uniform), %.2f x (skewed); skewed / uniform = %.2f" % (
                str(dtype).split(".")[1], "+ prob" if want_prob else "no prob",
                best[("torch", want_prob, "uniform")] / best[("kernel", want_prob, "uniform")],
                best[("torch", want_prob, "skewed")] / best[("kernel", want_prob, "skewed")],
                best[("kernel", want_prob, "skewed")] / best[("kernel", want_prob, "uniform")]))
        del xs
    x_u, x_s = base.to(torch.bfloat16), skew.to(torch.bfloat16)
    times = {}
    for rnd in range(rounds):
        for blocks in (512, 1024, 2048, 4096, 8192, 16384, 65536):
            with engine.tuning(METRICS_BLOCKS=blocks):
                times.setdefault((blocks, "uniform"), []).append(timeit(lambda: meter.update(x_u, lab_u), 20, 3))
                times.setdefault((blocks, "skewed"), []).append(timeit(lambda: meter.update(x_s, lab_s), 20, 3))
    for (blocks, dist_name), ts in times.items():
        report("METRICS_BLOCKS=%d bfloat16 %s labels no prob" % (blocks, dist_name), ts, n * c * 2 + 16 * n)


def ap():
    """lgs_average_precision behind metrics.average_precision: the whole call (HIP events) and its four stages (kernel times from
    torch.profiler, by kernel name: 1 keys, 2 sort + segment starts, 3 rank pass, 4 scan + terms + finish) on
      scene      [151 k, 200], "trained" scores (the row's own class lifted), 90 % of the rows on two classes
      batch      [1.2 M, 200], the same
      untrained  [1.2 M, 200], near-uniform probabilities, uniform labels: the skip test of stage 3 ends almost nothing
    each from bf16 logits (from_logits=True) and from fp32 prob; beside a per-column torch.sort AP on the same device (cumulative
    precision at each positive; ties are not grouped: a timing baseline) and, on the scene shape (every shape with `ap full`),
    sklearn's average_precision_score per class on the host, the copy included."""
    from languagegroundedsemseg_amd.metrics import average_precision
    c, rounds = 200, 3
    full = len(sys.argv) > 2 and sys.argv[2] == "full"
    g = torch.Generator(device=DEV).manual_seed(0)

    def make(n, trained):
        lab = torch.randint(0, c, (n,), device=DEV, generator=g)
        if trained:
            r = torch.rand(n, device=DEV, generator=g)
            lab = torch.where(r < 0.45, torch.full_like(lab, 3), torch.where(r < 0.9, torch.full_like(lab, 7), lab))
            x = torch.randn(n, c, device=DEV, generator=g) * 2.0
            hit = torch.rand(n, device=DEV, generator=g) < 0.8          # 80 % of the rows score their own class highest
            x[torch.arange(n, device=DEV)[hit], lab[hit]] += 8.0
        else:
            x = torch.randn(n, c, device=DEV, generator=g) * 0.01
        lab[torch.rand(n, device=DEV, generator=g) < 0.1] = -1
        return x.to(torch.bfloat16), lab

    def sort_ap(prob, lab):
        cols = prob.t().contiguous()
        ar = torch.arange(1, prob.shape[0] + 1, device=prob.device, dtype=torch.float64)
        out = []
        for k in range(c):
            s, idx = torch.sort(cols[k], descending=True)
            y = (lab[idx] == k).to(torch.float64)
            out.append((torch.cumsum(y, 0) / ar * y).sum() / y.sum())
        return torch.stack(out)

    def sklearn_ap(prob, lab):
        from sklearn.metrics import average_precision_score
        p, t = prob.cpu().numpy(), lab.cpu().numpy()
        return [average_precision_score(t == k, p[:, k]) for k in range(c) if (t == k).any()]

    def stage_of(name):
        if "k_ap_softmax_keys" in name or "k_ap_keys" in name:
            return 1
        if "k_ap_rank" in name:
            return 3
        if "k_ap_terms" in name or "k_ap_finish" in name:
            return 4
        if "k_ap_offsets" in name or "onesweep" in name or "radix" in name or "sort" in name:
            return 2
        if "scan" in name:
            return 4
        return 0

    def stages(fn, iters=5):
        """-> us per call of the stages 1 .. 4 and of the device work that belongs to none (memset), or None without a profiler"""
        try:
            from torch.profiler import profile, ProfilerActivity
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
            out = [0.0] * 5
            for ev in prof.key_averages():
                t = getattr(ev, "self_device_time_total", None)
                if t is None:
                    t = ev.self_cuda_time_total
                out[stage_of(ev.key)] += t / iters
            return out if sum(out) > 0 else None
        except Exception as exc:          # a build without the tracer: the whole-call times stand
            print("  (no stage times: %s)" % exc)
            return None

    print("%-44s %10s | %8s %8s %8s %8s %8s | %12s %12s" % ("case", "call us", "1 keys", "2 sort", "3 rank", "4 finish", "other",
                                                             "torch.sort us", "sklearn ms"))
    for name, n, trained in (("scene [151k,200]", 151000, True), ("batch [1.2M,200]", 1200000, True), ("untrained [1.2M,200]", 1200000, False)):
        x, lab = make(n, trained)
        prob = torch.softmax(x.float(), 1)
        t_sort = min(timeit(lambda: sort_ap(prob, lab), 1, 1) for _ in range(2))
        t_sk = None
        if n < 200000 or full:
            try:
                t0 = time.perf_counter()
                sklearn_ap(prob, lab)
                t_sk = (time.perf_counter() - t0) * 1e3
            except ImportError:
                pass
        for kind, src, kw in (("bf16 logits", x, {"from_logits": True}), ("fp32 prob", prob, {})):
            call = lambda: average_precision(src, lab, **kw)
            ts = [timeit(call, 10, 2) for _ in range(rounds)]
            st = stages(call)
            cells = " ".join("%8.1f" % v for v in (st[1:] + st[:1])) if st else " ".join(["%8s" % "-"] * 5)
            print("%-44s %10.1f | %s | %12.1f %12s" % ("%s %s (median %.1f)" % (name, kind, sorted(ts)[len(ts) // 2] * 1e3), min(ts) * 1e3,
                                                        cells, t_sort * 1e3, "%.0f" % t_sk if t_sk is not None else "-"))
        del x, prob


def focal():
    """k_focal_fwd_bwd (gamma 0 / 2 / 2.5, with and without alpha) beside k_ce_fwd_bwd on the same [1.2 M, 200] scores, bf16 and fp32,
    forward (loss rows) and backward (d logits) calls, all variants alternating inside this process; min / median over the rounds.
    Byte model: forward n c e + 8 n labels + 4 n loss rows, backward 2 n c e + 8 n + 4 n row factors; the focal kernel adds 4 n
    (alpha[label]) when it has a table."""
    be = ME.get_backend()
    n, c, rounds = 1200000, 200, 5
    g = torch.Generator(device=DEV).manual_seed(0)
    base = torch.randn(n, c, device=DEV, generator=g) * 3
    lab = torch.randint(-1, c, (n,), device=DEV, generator=g)
    alpha = torch.rand(c, device=DEV, generator=g) * 2 + 0.1
    up = torch.rand(n, device=DEV, generator=g)
    for dtype in (torch.bfloat16, torch.float32):
        e = 2 if dtype == torch.bfloat16 else 4
        x = base.to(dtype)
        variants = [("k_ce_fwd_bwd", None, None)] + [("k_focal_fwd_bwd gamma %g %s" % (gm, "alpha" if a is not None else "no alpha"), gm, a)
                                                     for gm in (0.0, 2.0, 2.5) for a in (None, alpha)]
        times = {}
        for rnd in range(rounds):
            for name, gm, a in variants:
                if gm is None:
                    fwd = lambda: be.cross_entropy_rows(x, lab, -1)
                    bwd = lambda: be.cross_entropy_rows(x, lab, -1, row_grad=up)
                else:
                    fwd = lambda: be.focal_loss_rows(x, lab, -1, a, gm)
                    bwd = lambda: be.focal_loss_rows(x, lab, -1, a, gm, row_grad=up)
                times.setdefault((name, "fwd"), []).append(timeit(fwd, 20, 3))
                times.setdefault((name, "bwd"), []).append(timeit(bwd, 20, 3))
        ref = {d: min(times[("k_ce_fwd_bwd", d)]) for d in ("fwd", "bwd")}
        for name, gm, a in variants:
            for d in ("fwd", "bwd"):
                ts = times[(name, d)]
                t, med = min(ts), sorted(ts)[len(ts) // 2]
                nbytes = n * c * e * (1 if d == "fwd" else 2) + 12 * n + (4 * n if a is not None else 0)
                print("%-8s %-36s %s %8.1f us (median %8.1f)  %7.1f MB  %.2f TB/s  x k_ce_fwd_bwd %.3f" % (
                    str(dtype).split(".")[1], name, d, t * 1e3, med * 1e3, nbytes / 1e6, nbytes / t / 1e9, t / ref[d]))
        del x


def supcon():
    """PointSupConLoss (P = 1, K = 3, 'cos', 200 labels) at the benchmark batch's 1.2 M rows, bf16, C = 96 and C = 512: the device
    sampler (table plumbing in torch device ops + k_supcon_sample), k_supcon_fwd and k_supcon_bwd, beside the torch gather path on the
    same device (SUPCON_FUSED=0: index gathers into [N, S, C] fp32, F.normalize, mean, autograd) with the same indices.
    Byte model: forward (1 + P + K) n c e, backward the same reads + n c e written; the fraction is of 8 TB/s."""
    from languagegroundedsemseg_amd import engine
    from languagegroundedsemseg_amd.losses import PointSupConLoss
    be = ME.get_backend()
    n, L, P, K, rounds = 1200000, 200, 1, 3, 3
    g = torch.Generator(device=DEV).manual_seed(0)
    lab = torch.randint(-1, L, (n,), device=DEV, generator=g)
    preds = torch.where(torch.rand(n, device=DEV, generator=g) < 0.7, lab, torch.randint(0, L, (n,), device=DEV, generator=g))
    crit = PointSupConLoss(L, P, K).to(DEV)
    crit.update_confusion_hist(torch.randint(0, 1000, (L, L), device=DEV, generator=g))
    gen = torch.Generator().manual_seed(1)
    pos, neg = crit.sample(lab, preds, generator=gen)
    tables = crit.sampling_tables(lab, preds)
    up = torch.rand(n, device=DEV, generator=g)
    t_sample = min(timeit(lambda: crit.sample(lab, preds, generator=gen), 10, 2) for _ in range(rounds))
    t_kernel = min(timeit(lambda: be.supcon_sample(lab, L, -1, tables, P, K, 12345), 10, 2) for _ in range(rounds))
    print("sample: tables + k_supcon_sample %8.1f us, k_supcon_sample alone %8.1f us  (n = %d, %d labels, P = %d, K = %d)" % (
        t_sample * 1e3, t_kernel * 1e3, n, L, P, K))
    with engine.tuning(SUPCON_FUSED=0):
        t_torch_sample = timeit(lambda: crit.sample(lab, preds, generator=gen), 3, 1)
    print("sample: torch restatement (SUPCON_FUSED=0) %8.1f us" % (t_torch_sample * 1e3))
    for c in (96, 512):
        x = torch.randn(n, c, device=DEV, generator=g).to(torch.bfloat16)
        e = 2
        _, _, saved = be.supcon_forward(x, lab, pos, neg, -1, L, "cos")
        t_fwd = min(timeit(lambda: be.supcon_forward(x, lab, pos, neg, -1, L, "cos"), 10, 2) for _ in range(rounds))
        t_bwd = min(timeit(lambda: be.supcon_backward(saved, up, up, -1, L, "cos"), 10, 2) for _ in range(rounds))
        fb, bb = (1 + P + K) * n * c * e, (2 + P + K) * n * c * e
        print("C = %3d bf16  k_supcon_fwd %8.1f us  %7.1f MB  %.2f TB/s (%.0f %% of 8 TB/s)" % (c, t_fwd * 1e3, fb / 1e6, fb / t_fwd / 1e9, fb / t_fwd / 8e7))
        print("C = %3d bf16  k_supcon_bwd %8.1f us  %7.1f MB  %.2f TB/s (%.0f %% of 8 TB/s)" % (c, t_bwd * 1e3, bb / 1e6, bb / t_bwd / 1e9, bb / t_bwd / 8e7))
        xr = x.clone().requires_grad_(True)

        def step():
            xr.grad = None
            crit(xr, lab, pos_indices=pos, neg_indices=neg)[0].backward()
        t_mod = min(timeit(step, 5, 2) for _ in range(rounds))
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        m_fused = torch.cuda.max_memory_allocated()
        with engine.tuning(SUPCON_FUSED=0):
            t_torch = min(timeit(step, 2, 1) for _ in range(2))
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            m_torch = torch.cuda.max_memory_allocated()
        print("C = %3d bf16  module forward + backward (hinge and means included): kernels %8.1f us, torch gather path %8.1f us (x %.1f); "
              "peak memory %.2f GB against %.2f GB" % (c, t_mod * 1e3, t_torch * 1e3, t_torch / t_mod, m_fused / 1e9, m_torch / 1e9))
        del x, xr, saved


def augment():
    """the train-time augmentation chain on the benchmark's 8-scene batch, raw points before the dedup; the numpy
    restatement of the same stages (tests/augment_reference.py, one scene, one thread) beside it"""
    from languagegroundedsemseg_amd import augment as A
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    order = np.argsort(coords[:, 0], kind="stable")
    coords, labels = coords[order], labels[order]
    rep = np.repeat(coords, 2, 0)                                   # ~2 points per voxel, like a 2 cm voxelisation of ScanNet
    pts = ((rep[:, 1:].astype(np.float64) + rng.uniform(0.05, 0.95, (rep.shape[0], 3))) * 0.02).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rep[:, 0], minlength=8))]).tolist()
    for s in range(8):                                              # every scene at its own origin, as a dataset hands it over
        pts[off[s]:off[s + 1]] -= pts[off[s]:off[s + 1]].min(0)
    cols = np.floor(rng.random(pts.shape) * 256).astype(np.float32)
    p, c, lab = torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV), torch.from_numpy(np.repeat(labels, 2)).to(DEV)
    n = p.shape[0]
    aug = A.DeviceAugmentation(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)),
                               scale_bound=(0.9, 1.1), normalize_color=True, seed=1)
    plan = aug.draw(8)
    plan.elastic[:], plan.autocontrast[:], plan.translate[:], plan.jitter[:] = True, True, True, True
    plan.flip_axes[:] = 3
    print("%d points in 8 scenes, extents up to %s m" % (n, np.round(max(pts[off[s]:off[s + 1]].max(0).max() for s in range(8)), 2)))
    off_dev = torch.tensor(off, dtype=torch.int64, device=DEV)

    def show(name, ms, rows=n):
        print("%-44s %8.3f ms per batch  %8.1f M points/s" % (name, ms, rows / ms / 1e3))
    show("bounds (fp32 [N, 3])", timeit(lambda: A.aug_bounds(p, off_dev)))
    for stage, (g, m) in enumerate(aug.elastic_params):
        show("elastic stage %d (granularity %.1f), incl. bounds" % (stage + 1, g),
             timeit(lambda: A.elastic_distortion(p, off, g, m, seed=3, scene_seeds=plan.scene_seeds, stage=stage)))
    show("batched voxelise", timeit(lambda: A.voxelize_batched(p, off, plan.matrices)))
    vox = A.voxelize_batched(p, off, plan.matrices)
    keep = ME.utils.sparse_quantize(vox, return_maps_only=True)
    show("dedup (engine insert, existing)", timeit(lambda: ME.utils.sparse_quantize(vox, return_maps_only=True)))
    vc, vf = vox.index_select(0, keep), c.index_select(0, keep)
    nv = vc.shape[0]
    show("flip + shift on %d voxel rows, incl. bounds" % nv, timeit(lambda: A.horizontal_flip(vc, plan.flip_axes, batch_size=8)), nv)
    _, off_v = A.aug_bounds(vc, batch_size=8)
    show("colour on %d voxel rows, incl. bounds" % nv, timeit(lambda: A.chromatic_augment(vf, off_v, aug.color_params(plan), normalize=True, seed=5)), nv)
    t_chain = timeit(lambda: aug(p, c, lab, off, plan=plan))
    show("chain (elastic x2, voxelise, dedup, flip, colour)", t_chain)
    print("chain = %.1f %% of a 27 ms training step" % (100 * t_chain / 27.0))
    assert A.aug_status([torch.zeros(1, dtype=torch.int32, device=DEV)]) == []
    # the numpy restatement on scene 0, one thread
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import augment_reference as ar
    torch.set_num_threads(1)
    s0 = pts[off[0]:off[1]]
    t_cpu = {}
    cur = s0
    for stage, (g, m) in enumerate(aug.elastic_params):
        t0 = time.perf_counter()
        noise = np.random.default_rng(stage).standard_normal(tuple(ar.noise_dims(cur, g)) + (3,)).astype(np.float32)
        cur = ar.elastic_stage(cur, noise, g, m).astype(np.float32)
        t_cpu["elastic stage %d" % (stage + 1)] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ar.color_chain(cols[off[0]:off[1]], blend=0.5, translation=(3.0, -4.0, 5.0), jitter_std=0.05,
                   jitter_noise=np.random.default_rng(9).standard_normal((len(s0), 3)), normalize=True)
    t_cpu["colour"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ar.flip(np.floor(cur / 0.02), (0, 1))
    t_cpu["flip"] = time.perf_counter() - t0
    for k, v in t_cpu.items():
        print("numpy restatement, scene 0 (%d points), 1 thread: %-16s %8.1f ms" % (len(s0), k, v * 1e3))
    print("numpy restatement, scene 0, these stages together: %.1f ms (x 8 scenes = %.0f ms per batch; device chain %.2f ms)"
          % (sum(t_cpu.values()) * 1e3, 8 * sum(t_cpu.values()) * 1e3, t_chain))


def paste():
    """The class-balanced tail-instance paste (csrc/lgs_paste.hip) on the benchmark's 8-scene batch with a synthetic bank and boxes:
    the call, its kernels one by one (the profiler's device times), what it adds to the augmentation chain, and the numpy
    restatement of the reference's host method (tests/paste_reference.py, scene 0, one thread) beside it"""
    from languagegroundedsemseg_amd import augment as A
    from languagegroundedsemseg_amd.synthetic import make_instance_bank, make_scene_boxes
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    order = np.argsort(coords[:, 0], kind="stable")
    coords, labels = coords[order], labels[order]
    rep = np.repeat(coords, 2, 0)
    pts = ((rep[:, 1:].astype(np.float64) + rng.uniform(0.05, 0.95, (rep.shape[0], 3))) * 0.02).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rep[:, 0], minlength=8))]).tolist()
    for s in range(8):
        pts[off[s]:off[s + 1]] -= pts[off[s]:off[s + 1]].min(0)
    cols = np.floor(rng.random(pts.shape) * 256).astype(np.float32)
    lab_h = np.repeat(labels, 2)
    p, c, lab = torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV), torch.from_numpy(lab_h).to(DEV)
    n = p.shape[0]
    bp, bc, bl, boff, bcat = make_instance_bank()
    bank = A.InstanceBank(torch.from_numpy(bp).to(DEV), torch.from_numpy(bc).to(DEV), torch.from_numpy(bl).to(DEV), boff, bcat)
    ids = np.unique(bcat)
    kw = dict(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
              normalize_color=True, seed=1)
    aug = A.DeviceAugmentation(tail_instances=A.TailInstancePaste(bank, ids, np.ones(len(ids)), num_instances=5, max_iterations=50, seed=2), **kw)
    plain = A.DeviceAugmentation(**kw)
    plan = aug.draw(8)
    plan.elastic[:], plan.autocontrast[:], plan.translate[:], plan.jitter[:] = True, True, True, True
    plan.flip_axes[:] = 3
    boxes = [make_scene_boxes(pts[off[s]:off[s + 1]], seed=s) for s in range(8)]
    m_v = np.stack([np.diag([v, v, v, 1.0]) for v in plan.scale])
    vox = A.voxelize_batched(p, off, m_v)
    inst_rows = int(np.diff(boff)[plan.paste.instances].sum())
    print("%d points in 8 scenes, 40 instances of %d rows, %d boxes per scene" % (n, inst_rows, len(boxes[0])))

    def call():
        return A.paste_instances(vox, c, lab, off, boxes, plan.paste, plan.scale, plan.rotations, return_state=True)
    out = call()
    assert A.aug_status(out[4]) == []
    trials = out[5]["placement"][:, 0].cpu().numpy()
    print("winning trials: %d at trial 0, %d later, %d exhausted" % ((trials == 0).sum(), ((trials > 0) & (trials < 50)).sum(), (trials == 50).sum()))
    t_call = timeit(call, iters=20)
    print("%-52s %8.3f ms per batch" % ("paste_instances (tables, upload, 8 launches)", t_call))
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                call()
            torch.cuda.synchronize()
        for ev in sorted(prof.key_averages(), key=lambda e: e.key):
            if "k_paste" in ev.key or "k_aug_bounds" in ev.key or "k_aug_scene" in ev.key:
                us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                name = re.search(r"k_[a-z_]+(<[^>]*>)?", ev.key).group(0)
                print("  %-50s %8.1f us per call (%d launches)" % (name, us / 10.0, ev.count // 10))
    except Exception as e:      # the profiler is a convenience: the call's own time above stands without it
        print("  (no per-kernel times: %s)" % e)
    t_plain = timeit(lambda: plain(p, c, lab, off, plan=plan), iters=10)
    t_tail = timeit(lambda: aug(p, c, lab, off, plan=plan, scene_boxes=boxes), iters=10)
    print("%-52s %8.3f ms per batch" % ("chain without the paste", t_plain))
    print("%-52s %8.3f ms per batch  (+ %.3f ms)" % ("chain with the paste", t_tail, t_tail - t_plain))
    # the numpy restatement of the reference's host method on scene 0, one thread: three dedups, filter over the whole map, sequential trials
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import paste_reference as pr
    torch.set_num_threads(1)
    v0 = vox[off[0]:off[1], 1:].cpu().numpy()
    inst = [(bp[boff[i]:boff[i + 1]], bc[boff[i]:boff[i + 1]], bl[boff[i]:boff[i + 1]], plan.paste.matrices[0, k])
            for k, i in enumerate(plan.paste.instances[0])]
    t0 = time.perf_counter()
    pr.paste_scene(v0, cols[off[0]:off[1]], lab_h[off[0]:off[1]], boxes[0], plan.scale[0], plan.rotations[0], inst, None, 50,
                   seeds=(plan.paste.seed, plan.paste.scene_seeds[0]))
    t_cpu = time.perf_counter() - t0
    print("numpy restatement, scene 0 (%d points), 1 thread: %.1f ms (x 8 scenes = %.0f ms per batch; device call %.3f ms)"
          % (len(v0), t_cpu * 1e3, 8 * t_cpu * 1e3, t_call))


def dropout():
    """RandomDropout on the device (csrc/lgs_dropout.hip) on the benchmark's 8-scene, 1.2 M-voxel batch: the selection alone, the chain
    with dropout first against the same chain without it, torch's randperm formulation per scene on the same device, and
    np.random.choice on one host core for one scene.  Device events around 200 back-to-back calls."""
    from languagegroundedsemseg_amd import augment as A
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    order = np.argsort(coords[:, 0], kind="stable")
    coords, labels = coords[order], labels[order]
    sizes = np.bincount(coords[:, 0], minlength=8)
    off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    nv = int(off_h[-1])
    off_v = torch.from_numpy(off_h).to(DEV)
    seeds = list(range(1, 9))
    every = [True] * 8
    print("%d voxel rows in 8 scenes (%d .. %d per scene), ratio 0.2, every scene drops" % (nv, sizes.min(), sizes.max()))

    def show(name, ms):
        print("%-64s %8.3f ms per batch" % (name, ms))
    rows, o = A.random_dropout_rows(off_v, nv, every, ratio=0.2, seed=7, scene_seeds=seeds)
    assert np.diff(o.host).tolist() == [int(n * (1 - 0.2)) for n in sizes] and bool((rows[1:] > rows[:-1]).all())
    show("lgs_dropout_select alone (11 launches, nothing read back)",
         timeit(lambda: A._dropout_select(off_v, nv, every, 0.2, 7, seeds, None, None), iters=200, warm=5))
    show("random_dropout_rows (the call and its read of 9 offsets)",
         timeit(lambda: A.random_dropout_rows(off_v, nv, every, ratio=0.2, seed=7, scene_seeds=seeds), iters=200, warm=5))
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                A._dropout_select(off_v, nv, every, 0.2, 7, seeds, None, None)
            torch.cuda.synchronize()
        for ev in sorted(prof.key_averages(), key=lambda e: e.key):
            if "k_drop" in ev.key:
                us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                print("  %-62s %8.1f us per call (%d launches)" % (re.search(r"k_[a-z_]+(<[^>]*>)?", ev.key).group(0), us / 10.0, ev.count // 10))
    except Exception as e:      # the profiler is a convenience: the call's own time above stands without it
        print("  (no per-kernel times: %s)" % e)
    ks = [int(n * (1 - 0.2)) for n in sizes]

    def torch_formulation():
        return [torch.randperm(int(n), device=DEV)[:k].sort()[0] for n, k in zip(sizes, ks)]
    show("torch.randperm(n_s, device)[:k].sort() per scene, 8 scenes", timeit(torch_formulation, iters=200, warm=5))
    # the chain, raw points before the dedup (~2 per voxel), as `augment` builds them
    rep = np.repeat(coords, 2, 0)
    pts = ((rep[:, 1:].astype(np.float64) + rng.uniform(0.05, 0.95, (rep.shape[0], 3))) * 0.02).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rep[:, 0], minlength=8))]).tolist()
    for s in range(8):
        pts[off[s]:off[s + 1]] -= pts[off[s]:off[s + 1]].min(0)
    cols = np.floor(rng.random(pts.shape) * 256).astype(np.float32)
    p, c, lab = torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV), torch.from_numpy(np.repeat(labels, 2)).to(DEV)
    kw = dict(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
              normalize_color=True, seed=1)
    plain, first, last = A.DeviceAugmentation(**kw), A.DeviceAugmentation(dropout=0.2, dropout_position="first", **kw), \
        A.DeviceAugmentation(dropout=0.2, dropout_position="last", **kw)
    plan = first.draw(8)
    plan.elastic[:], plan.autocontrast[:], plan.translate[:], plan.jitter[:], plan.dropout[:] = True, True, True, True, True
    plan.flip_axes[:] = 3
    t_plain = timeit(lambda: plain(p, c, lab, off, plan=plan), iters=200, warm=5)
    t_first = timeit(lambda: first(p, c, lab, off, plan=plan), iters=200, warm=5)
    t_last = timeit(lambda: last(p, c, lab, off, plan=plan), iters=200, warm=5)
    show("chain without dropout (%d points)" % p.shape[0], t_plain)
    show("chain with dropout first, every scene drops", t_first)
    print("%-64s %+8.3f ms" % ("  difference (selection, second read; fewer rows afterwards)", t_first - t_plain))
    show("chain with dropout last, every scene drops", t_last)
    print("%-64s %+8.3f ms" % ("  difference (selection, second read, three gathers)", t_last - t_plain))
    # the reference's own call on one host core, one scene
    torch.set_num_threads(1)
    n0 = int(sizes.max())
    np.random.seed(0)
    t0 = time.perf_counter()
    for _ in range(20):
        np.random.choice(n0, int(n0 * (1 - 0.2)), replace=False)
    t_cpu = (time.perf_counter() - t0) / 20
    print("np.random.choice(%d, %d, replace=False), 1 host thread: %.2f ms per scene (x 8 scenes = %.1f ms per batch), without the gathers"
          % (n0, int(n0 * 0.8), t_cpu * 1e3, 8 * t_cpu * 1e3))


def fps():
    """Furthest point sampling on the device (csrc/lgs_fps.hip) on the benchmark's 8-scene, 1.2 M-point batch, ratio 0.05: the whole
    limited_annotation call, lgs_fps_segments alone, the largest segment alone (its rounds are the critical path), the time of a round
    in every tier and on both sides of every tier bound, the torch lines of the same rounds on the same device, and the numpy
    restatement on one host core, both for one scene.  SYNTHETIC CHOICE: per scene the lowest 10 cm are the floor, the outer 10 cm in
    x and y are two walls, the rest belongs to the nearest of 40 random centres in the plan (one instance each); 10 % of the rows have
    no instance.  Device events around back-to-back calls."""
    from languagegroundedsemseg_amd import annotation as AN, instances as IN
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import fps_reference as fr
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    order = np.argsort(coords[:, 0], kind="stable")
    coords, labels = coords[order], labels[order].astype(np.int64)
    sizes = np.bincount(coords[:, 0], minlength=8)
    off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off_h[-1])
    pts = ((coords[:, 1:].astype(np.float64) + rng.uniform(0.05, 0.95, (n, 3))) * 0.02).astype(np.float32)
    ids = np.empty(n, dtype=np.int64)
    for s in range(8):
        q = pts[off_h[s]:off_h[s + 1]]
        lo, hi = q.min(0), q.max(0)
        centres = rng.uniform(lo[:2], hi[:2], (40, 2))
        i = 3 + np.argmin(((q[:, None, :2] - centres[None]) ** 2).sum(-1), axis=1)
        i[(q[:, 0] < lo[0] + 0.1) | (q[:, 0] > hi[0] - 0.1)] = 1
        i[(q[:, 1] < lo[1] + 0.1) | (q[:, 1] > hi[1] - 0.1)] = 2
        i[q[:, 2] < lo[2] + 0.1] = 0
        i[rng.random(len(q)) < 0.1] = -1
        ids[off_h[s]:off_h[s + 1]] = i
    seg_sizes = np.sort(np.concatenate([np.bincount(ids[off_h[s]:off_h[s + 1]][ids[off_h[s]:off_h[s + 1]] >= 0]) for s in range(8)]))
    seg_sizes = seg_sizes[seg_sizes > 0]
    b1, b2, b3 = AN.TIER_BOUNDS
    print("%d points in 8 scenes, %d instances of %d .. %d points (median %d); per tier: %d wave, %d group<4>, %d group<16>, %d stream; "
          "ratio 0.05: %d samples in all, %d in the largest" % (
              n, len(seg_sizes), seg_sizes[0], seg_sizes[-1], int(np.median(seg_sizes)), (seg_sizes <= b1).sum(),
              ((seg_sizes > b1) & (seg_sizes <= b2)).sum(), ((seg_sizes > b2) & (seg_sizes <= b3)).sum(), (seg_sizes > b3).sum(),
              sum(fr.count_rule(int(v), 0.05) for v in seg_sizes), fr.count_rule(int(seg_sizes[-1]), 0.05)))
    p, i_dev, l_dev, off_dev = (torch.from_numpy(a).to(DEV) for a in (pts, ids, labels, off_h))

    def show(name, ms):
        print("%-72s %9.3f ms" % (name, ms))
    out = AN.limited_annotation(p, i_dev, l_dev, off_dev, 0.05)
    assert 0 < int(out[1].sum()) <= sum(min(int(v), fr.count_rule(int(v), 0.05)) for v in seg_sizes)
    show("limited_annotation, the batch (instance table, sort, scan, lgs_fps_segments)",
         timeit(lambda: AN.limited_annotation(p, i_dev, l_dev, off_dev, 0.05), iters=5, warm=1))
    # the engine call alone on the same segments
    c4 = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
    c4[:, 0] = torch.from_numpy(coords[:, 0].astype(np.int32)).to(DEV)
    info = IN.instance_info(c4, i_dev, return_centers=False)
    cap = info.count.shape[0]
    through = torch.sort(torch.where(info.slot >= 0, info.slot, torch.full_like(info.slot, cap)), stable=True)[1]
    seg_off = torch.zeros(cap + 1, dtype=torch.int64, device=DEV)
    seg_off[1:] = torch.cumsum(info.count, 0, dtype=torch.int64)
    rank = torch.empty(n, dtype=torch.int32, device=DEV)
    show("lgs_fps_segments alone, %d segment slots (6 launches, nothing read back)" % cap,
         timeit(lambda: AN._fps_call(p, through, seg_off, ratio=0.05, rank_out=rank), iters=5, warm=1))
    # the largest segment alone
    big = int(np.argmax(info.count.cpu().numpy()))
    lo, hi = int(seg_off[big]), int(seg_off[big + 1])
    pb = p[through[lo:hi]].contiguous()[None]
    mb = fr.count_rule(hi - lo, 0.05)
    tb = timeit(lambda: AN.furthest_point_sample(pb, mb), iters=5, warm=1)
    show("the largest segment alone (%d points, %d samples)" % (hi - lo, mb), tb)
    print("%-72s %9.3f us" % ("  per round", tb * 1e3 / (mb - 1)))
    # a round in every tier: one segment, 1001 samples; 64 equal segments in one call for the throughput side
    print("one round, us (one segment alone | 64 segments in one call, per segment):")
    cloud = torch.from_numpy(rng.uniform(-3, 3, (64 * 100000, 3)).astype(np.float32)).to(DEV)
    for size in (64, b1, b1 + 1, 1024, b2, b2 + 1, 4096, b3, b3 + 1, 20000, 100000):
        tier = "k_fps_wave" if size <= b1 else "k_fps_group<4>" if size <= b2 else "k_fps_group<16>" if size <= b3 else "k_fps_stream"
        one = cloud[:size][None]
        many = cloud[:64 * size].view(64, size, 3)
        t1 = timeit(lambda: AN.furthest_point_sample(one, 1001), iters=3, warm=1)
        t64 = timeit(lambda: AN.furthest_point_sample(many, 1001), iters=3, warm=1)
        print("  n = %6d  %-16s %9.3f | %9.3f" % (size, tier, t1, t64 / 64))
    # one scene: the torch lines of the same rounds on the device, the numpy restatement on one host core
    ids0, p0 = ids[:off_h[1]], pts[:off_h[1]]
    groups = [np.nonzero(ids0 == v)[0] for v in np.unique(ids0[ids0 >= 0])]
    rounds = sum(fr.count_rule(len(g), 0.05) - 1 for g in groups)
    dev_groups = [p[torch.from_numpy(g).to(DEV)].contiguous() for g in groups]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in dev_groups:
        AN.fps_torch(g, fr.count_rule(g.shape[0], 0.05))
    torch.cuda.synchronize()
    t_torch = time.perf_counter() - t0
    off0 = torch.from_numpy(np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)).to(DEV)
    p0g = torch.cat(dev_groups)
    rank0 = torch.empty(p0g.shape[0], dtype=torch.int32, device=DEV)
    t_dev = timeit(lambda: AN._fps_call(p0g, None, off0, ratio=0.05, rank_out=rank0), iters=5, warm=1)
    print("scene 0 (%d instances, %d rounds in all): lgs_fps_segments %.3f ms; torch lines per segment on the device %.1f ms (%.1f us per "
          "round)" % (len(groups), rounds, t_dev, t_torch * 1e3, t_torch * 1e6 / rounds))
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    want = [fr.fps_contract(p0[g], fr.count_rule(len(g), 0.05)) for g in groups]
    t_cpu = time.perf_counter() - t0
    got = rank0.cpu().numpy()
    start = 0
    for g, w in zip(groups, want):
        assert np.array_equal(np.argsort(np.where(got[start:start + len(g)] < 0, 1 << 30, got[start:start + len(g)]),
                                         kind="stable")[:len(np.unique(w))], w[:len(np.unique(w))])
        start += len(g)
    print("numpy restatement, scene 0, 1 host thread: %.0f ms (x 8 scenes = %.1f s per batch)" % (t_cpu * 1e3, 8 * t_cpu))


def instshift():
    """The per-instance colour and scale shifts on the device (csrc/lgs_instshift.hip) on the benchmark's 8-scene, 2.4 M-point batch
    (the points `dropout` feeds its chain): the stage alone, the chain with and without it, and the host method's shape of work (one
    boolean mask over the cloud per instance, np.delete / np.vstack) on one host core for one scene.  SYNTHETIC CHOICE: 5 % of the
    rows lie in tail segments, 40 segments per scene (4 tail labels x 10 ids), their rows spread at random over the scene.
    Device events around 200 back-to-back calls."""
    from languagegroundedsemseg_amd import augment as A
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    rng = np.random.default_rng(0)
    order = np.argsort(coords[:, 0], kind="stable")
    coords, labels = coords[order], labels[order]
    rep = np.repeat(coords, 2, 0)
    pts = ((rep[:, 1:].astype(np.float64) + rng.uniform(0.05, 0.95, (rep.shape[0], 3))) * 0.02).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rep[:, 0], minlength=8))]).tolist()
    for s in range(8):
        pts[off[s]:off[s + 1]] -= pts[off[s]:off[s + 1]].min(0)
    cols = np.floor(rng.random(pts.shape) * 256).astype(np.float32)
    n = pts.shape[0]
    tail = [1001, 1002, 1003, 1004]                                   # ids no synthetic label uses
    lab = np.repeat(labels, 2).astype(np.int64)
    in_tail = rng.random(n) < 0.05
    lab[in_tail] = rng.choice(tail, int(in_tail.sum()))
    ids = rng.integers(0, 10, n).astype(np.int64)
    print("%d points in 8 scenes; synthetic: %.1f %% of the rows in tail segments, 40 segments per scene, rows at random"
          % (n, 100.0 * in_tail.mean()))
    p, c, l, i = (torch.from_numpy(a).to(DEV) for a in (pts, cols, lab, ids))
    off_dev = torch.from_numpy(np.asarray(off, np.int64)).to(DEV)
    seeds = list(range(1, 9))

    def show(name, ms):
        print("%-64s %8.3f ms per batch" % (name, ms))
    bounds, _ = A.aug_bounds(p, off_dev)
    out = A.instance_shifts(p, c, l, i, off_dev, tail, 0.5, 0.2, seed=7, scene_seeds=seeds, scene_bounds=bounds)
    assert A.instance_shift_status(out[5]) == {"unshifted": [], "id_range": []} and int((out[2][:, 1] > 0).sum()) > 0
    show("instance_shifts alone, bounds given (5 launches + the sort)",
         timeit(lambda: A.instance_shifts(p, c, l, i, off_dev, tail, 0.5, 0.2, seed=7, scene_seeds=seeds, scene_bounds=bounds), iters=200, warm=5))
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                A.instance_shifts(p, c, l, i, off_dev, tail, 0.5, 0.2, seed=7, scene_seeds=seeds, scene_bounds=bounds)
            torch.cuda.synchronize()
        for ev in sorted(prof.key_averages(), key=lambda e: e.key):
            us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            m = re.search(r"k_is_[a-z_]+", ev.key)
            if not m and "rocprim" not in ev.key:
                continue
            name = m.group(0) if m else "rocPRIM " + (re.search(r"(onesweep|block_sort|merge|histogram|scan)\w*", ev.key) or re.search("sort", "sort")).group(0)
            print("  %-62s %8.1f us per call (%d launches)" % (name, us / 10.0, ev.count // 10))
    except Exception as e:      # the profiler is a convenience: the call's own time above stands without it
        print("  (no per-kernel times: %s)" % e)
    kw = dict(voxel_size=0.02, rotation_bound=((-np.pi / 64, np.pi / 64), (-np.pi / 64, np.pi / 64), (-np.pi, np.pi)), scale_bound=(0.9, 1.1),
              normalize_color=True, seed=1)
    plain, shifted = A.DeviceAugmentation(**kw), A.DeviceAugmentation(instance_shifts=A.InstanceShifts(tail), **kw)
    plan = plain.draw(8)
    plan.elastic[:], plan.autocontrast[:], plan.translate[:], plan.jitter[:] = True, True, True, True
    plan.flip_axes[:] = 3
    t_plain = timeit(lambda: plain(p, c, l, off, plan=plan), iters=200, warm=5)
    t_shift = timeit(lambda: shifted(p, c, l, off, plan=plan, instances=i), iters=200, warm=5)
    show("chain without the stage (%d points)" % n, t_plain)
    show("chain with instance_shifts (and instances=)", t_shift)
    print("%-64s %+8.3f ms" % ("  difference (the stage, the instances' gather)", t_shift - t_plain))
    # the host method's shape of work on one core, one scene: a mask over the cloud per instance, then np.delete / np.vstack
    torch.set_num_threads(1)
    a, b = off[0], off[1]
    hp, hc, hl, hi = pts[a:b], cols[a:b], lab[a:b], ids[a:b]
    t0 = time.perf_counter()
    for _ in range(3):
        moved_p, moved_c, gone = [], [], []
        idx = np.arange(b - a)
        for cat in np.unique(hl):
            if cat not in tail:
                continue
            cat_rows = hl == cat
            for inst in np.unique(hi[cat_rows]):
                rows = cat_rows * (hi == inst)
                moved_p.append(hp[rows] * np.float32(0.9))
                moved_c.append((hc[rows] * 0.5).astype(int))
                gone.append(idx[rows])
        gone = np.concatenate(gone)
        np.vstack([np.delete(hp, gone, axis=0)] + moved_p), np.vstack([np.delete(hc, gone, axis=0)] + moved_c)
    t_cpu = (time.perf_counter() - t0) / 3
    print("host method (numpy: one mask per instance, np.delete / np.vstack), %d points, 1 host thread: %.1f ms per scene (x 8 scenes = %.0f ms per batch)"
          % (b - a, t_cpu * 1e3, 8 * t_cpu * 1e3))


def nearest():
    """lgs_manager_nearest at the evaluation shape -- 8 scenes x ~150 k voxels, three points inside every occupied cell -- at
    NEAREST_MAX_RING 1, 2 and 4, anchors 0.0 and 0.5, with both lookup tables, and the share of queries that the ring search leaves to
    the exact scan (read off the returned d2: a query is unfinished after ring r exactly when d2 >= (r + 1/2)^2).  Beside it, on ONE
    scene (the insseg validation is one scene per iteration): a chunked torch.cdist arg-min on the device, the brute force
    get_original_pointcloud does today, and scipy's cKDTree on one host core, the search of test_pointcloud."""
    from scipy.spatial import cKDTree
    from languagegroundedsemseg_amd import engine
    from languagegroundedsemseg_amd.pointcloud import nearest_voxel
    scenes = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    coords, _, _ = make_batch(list(range(scenes)))
    rng = np.random.default_rng(0)
    pts, off = [], [0]
    for s in range(scenes):
        c = coords[coords[:, 0] == s][:, 1:].astype(np.float64)
        pts.append((np.repeat(c, 3, 0) + rng.random((3 * len(c), 3))).astype(np.float32))
        off.append(off[-1] + len(pts[-1]))
    q = torch.from_numpy(np.concatenate(pts)).to(DEV)
    off_dev = torch.tensor(off, dtype=torch.int64, device=DEV)
    c_dev = torch.from_numpy(coords).to(DEV)
    x = ME.SparseTensor(torch.zeros(len(coords), 1, device=DEV), c_dev)
    print("%d scenes, %d voxels, %d queries" % (scenes, len(coords), q.shape[0]))
    for table in (1, 0):
        for anchor in (0.0, 0.5):
            for ring in (1, 2, 4):
                with engine.tuning(MAP_BLOCK_DIR=table, NEAREST_MAX_RING=ring):
                    ts = [timeit(lambda: nearest_voxel(x, q, off_dev, None, anchor, return_distance=True), 200, 5) for _ in range(3)]
                    _, d2 = nearest_voxel(x, q, off_dev, None, anchor, return_distance=True)
                    left = float((d2 >= (ring + 0.5) ** 2).float().mean())
                print("lgs_manager_nearest  MAP_BLOCK_DIR=%d anchor %.1f NEAREST_MAX_RING=%d  %8.3f ms (median %8.3f)  to the exact scan: %.5f %%"
                      % (table, anchor, ring, min(ts), sorted(ts)[1], 100.0 * left))
    # one scene: the engine, the device brute force, the host KD-tree
    s0 = slice(off[0], off[1])
    q0, sites0 = q[s0], c_dev[c_dev[:, 0] == 0][:, 1:].float() + 0.5
    one = ME.SparseTensor(torch.zeros(sites0.shape[0], 1, device=DEV), c_dev[c_dev[:, 0] == 0].contiguous())
    t_one = min(timeit(lambda: nearest_voxel(one, q0, None, None, 0.5), 500, 5) for _ in range(3))
    rows = nearest_voxel(one, q0, None, None, 0.5)

    def brute(chunk=2048):
        out = torch.empty(q0.shape[0], dtype=torch.int64, device=DEV)
        for i in range(0, q0.shape[0], chunk):
            out[i:i + chunk] = torch.cdist(q0[i:i + chunk], sites0).argmin(1)
        return out
    t_brute = timeit(brute, 1, 1)
    agree = float((brute() == rows).float().mean())
    t0 = time.perf_counter()
    tree = cKDTree(sites0.double().cpu().numpy())
    _, idx = tree.query(q0.double().cpu().numpy(), workers=1)
    t_tree = (time.perf_counter() - t0) * 1e3
    agree_tree = float((torch.from_numpy(idx).to(DEV) == rows).float().mean())
    print("scene 0 (%d voxels, %d queries), anchor 0.5: lgs_manager_nearest %.3f ms | chunked torch.cdist arg-min %.1f ms (same rows: %.5f) | "
          "cKDTree build + query, one core %.1f ms (same rows: %.5f)" % (sites0.shape[0], q0.shape[0], t_one, t_brute, agree, t_tree, agree_tree))


def _insteval_runs(n, n_inst, n_cls, seed):
    """one synthetic scene for the host-side timing: instances are runs of the point index, predictions jittered runs (the shape of
    tests/golden/make_insteval_fixtures.py at any size) -> (gt_ids, the reference's prediction dict)"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), n_inst - 1, replace=False))
    seg = np.searchsorted(cuts, np.arange(n), side="right")
    cls = rng.integers(0, n_cls + 2, n_inst)                       # 1 .. n_cls are valid
    gt = (cls[seg] * 1000 + seg + 1).astype(np.int64)
    gt[rng.random(n) < 0.05] = 0
    bounds = np.concatenate([[0], cuts, [n]])
    preds = {}
    for s in range(n_inst):
        for _ in range(rng.integers(0, 3)):
            a, b = max(0, bounds[s] + rng.integers(-40, 40)), min(n, bounds[s + 1] + rng.integers(-40, 40))
            if b - a < 5:
                continue
            mask = np.zeros(n, np.int32)
            mask[a:b] = 1
            mask[rng.random(n) < 0.02] = 0
            label = cls[s] if rng.random() < 0.8 else rng.integers(0, n_cls + 2)
            preds[len(preds)] = {"conf": np.float32(rng.integers(0, 8) / 8.0), "label_id": torch.tensor(int(label)), "pred_mask": mask}
    return gt, preds


def insteval_host():
    """CPU only: InstanceEvaluator.evaluate() against the reference's own Evaluator.evaluate() on identical inputs (the reference's
    checkout is argv[2]): one 18-class 150 k-point scene, and a set of 50 scenes of 20 k points.  Both sides get the dict with dense masks;
    the evaluator's side is timed once from the dict (np.nonzero per mask included) and once from Proposals."""
    import importlib.util
    import io
    from contextlib import redirect_stdout
    from languagegroundedsemseg_amd.insteval import InstanceEvaluator, Proposals
    spec = importlib.util.spec_from_file_location("make_insteval_fixtures", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                       "tests", "golden", "make_insteval_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ref = gen.load_reference(sys.argv[2])
    labels, valid = ["c%d" % i for i in range(1, 19)], np.arange(1, 19)
    warm = InstanceEvaluator(labels, valid)                        # first use of the torch operators at this size (their thread pool: ~1 s, once)
    gt, preds = _insteval_runs(150000, 10, 18, 0)
    warm.add_gt(gt, 0)
    warm.add_prediction(preds, 0)
    warm.evaluate()
    for name, scenes in (("1 scene, 150 k points, 120 instances", [_insteval_runs(150000, 120, 18, 7)]),
                         ("50 scenes, 20 k points, 60 instances each", [_insteval_runs(20000, 60, 18, 100 + k) for k in range(50)])):
        t0 = time.perf_counter()
        rev = ref.Evaluator(labels, valid)
        for k, (gt, preds) in enumerate(scenes):
            rev.add_gt(gt, k)
            rev.add_prediction(preds, k)
        with redirect_stdout(io.StringIO()):
            want = rev.evaluate()
        t_ref = time.perf_counter() - t0
        t0 = time.perf_counter()
        ev = InstanceEvaluator(labels, valid)
        for k, (gt, preds) in enumerate(scenes):
            ev.add_gt(gt, k)
            ev.add_prediction(preds, k)
        got = ev.evaluate()
        t_dict = time.perf_counter() - t0
        props = [Proposals.from_instances(preds) for _, preds in scenes]
        t0 = time.perf_counter()
        ev = InstanceEvaluator(labels, valid)
        for k, (gt, _) in enumerate(scenes):
            ev.add_gt(torch.from_numpy(gt), k)
            ev.add_prediction(props[k], k)
        t_tab = time.perf_counter() - t0
        t0 = time.perf_counter()
        got2 = ev.evaluate()
        t_eval = time.perf_counter() - t0
        assert got == got2 and np.allclose(got, want, rtol=0, atol=1e-14), (got, got2, want)
        print("%-44s %4d predictions | reference add + evaluate %8.3f s | InstanceEvaluator from the dict %8.3f s | from Proposals: tables (CPU "
              "torch lines) %8.3f s, evaluate() %8.3f s | mAP %.6f / %.6f / %.6f equal" % (name, sum(len(p) for _, p in scenes), t_ref, t_dict, t_tab, t_eval, *got))


def insteval():
    """from "clusters exist" to the overlap tables on the host, on one synthetic scene of ~150 k voxels with its point cloud
    (three points per occupied cell, the shape `nearest` builds): Clustering.get_proposals + InstanceEvaluator.add_prediction up to the
    tables' arrival on the host, against Clustering.get_instances alone (the dense [P, N] mask and the per-proposal host loop), the
    clustering both share, and the kernels alone."""
    from languagegroundedsemseg_amd.insteval import InstanceEvaluator, instance_overlaps, proposal_conf
    from languagegroundedsemseg_amd.pointgroup import Clustering
    coords, _, _ = make_batch([1000], n_target=150000)
    rng = np.random.default_rng(0)
    cells = np.repeat(coords[:, 1:].astype(np.float64), 3, 0)
    xyz = ((cells + rng.random(cells.shape)) * 0.02).astype(np.float32)
    n, n_cls = xyz.shape[0], 20
    blk = np.floor(xyz / np.float32(0.6)).astype(np.int64)
    blk_id = (blk[:, 0] * 31 + blk[:, 1]) * 31 + blk[:, 2]
    blk_id -= blk_id.min()
    sem = (blk_id * 7 % n_cls).astype(np.int64)
    valid = np.arange(2, n_cls)                                     # columns 0 and 1 are wall and floor: ignored, as in the reference
    gt = np.where(sem >= 2, sem * 1000 + blk_id % 1000, 0).astype(np.int64)      # one instance per 0.6 m block; the predictions see 2 % label noise
    noise = rng.random(n) < 0.02
    sem[noise] = rng.integers(0, n_cls, int(noise.sum()))
    g = torch.Generator().manual_seed(0)
    scores = (torch.nn.functional.one_hot(torch.from_numpy(sem), n_cls).float() * 6 + torch.randn(n, n_cls, generator=g)).to(DEV)
    xyz_d, gt_d = torch.from_numpy(xyz).to(DEV), torch.from_numpy(gt).to(DEV)
    cl = Clustering(ignored_labels=[0, 1], class_mapping=torch.arange(n_cls), thresh=0.03, min_points=50, propose_points=100, score_func=torch.max)

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts[1:])

    def new_route():
        ev = InstanceEvaluator(["c%d" % c for c in valid], valid)
        ev.add_gt(gt_d, 0)
        ev.add_prediction(cl.get_proposals(xyz_d, scores), 0)
        return ev
    prop = cl.get_proposals(xyz_d, scores)
    p, m = len(prop), prop.member.shape[0]
    n_gt = len(np.unique(gt[gt != 0]))
    assert n_gt <= 1024, n_gt
    print("%d points, %d classes, %d proposals with %d members, %d ground-truth instances" % (n, n_cls, p, m, n_gt))
    t_cluster = wall(lambda: cl.cluster_(xyz_d, torch.max(scores, 1)[1]))
    t_new = wall(new_route)
    t_old = wall(lambda: cl.get_instances(xyz_d, scores))
    t_tab = timeit(lambda: instance_overlaps(prop, gt_d, valid), 200, 5)
    t_conf = timeit(lambda: proposal_conf(prop.member, prop.offsets, prop.label.int(), scores, "max"), 200, 5)
    ev = new_route()
    t0 = time.perf_counter()
    res = ev.evaluate()
    t_eval = (time.perf_counter() - t0) * 1e3
    print("clustering alone (cluster_, shared by both routes)               %9.2f ms" % t_cluster)
    print("get_proposals + add_gt + add_prediction, tables on the host       %9.2f ms   (%.2f MB to the host: [P, 1024] int32 + ids)"
          % (t_new, (p * 1024 * 4 + 1024 * 12 + p * 20) / 1e6))
    print("get_instances alone (dense [P, N] mask, per-proposal host loop)   %9.2f ms   (%.1f MB to the host: P masks of N int32)" % (t_old, p * n * 4 / 1e6))
    print("lgs_inst_overlap, tables (ids + overlap + zeroing [P, 1024])      %9.3f ms   reads %.2f MB: gt_ids once, 4 + 8 B per member" % (t_tab, (8 * n + 12 * m) / 1e6))
    print("lgs_inst_overlap, conf (max over one score column per proposal)   %9.3f ms   reads %.2f MB: 4 B + one 32 B sector per member" % (t_conf, 36 * m / 1e6))
    print("InstanceEvaluator.evaluate() on the host, this scene              %9.2f ms   mAP %.4f mAP50 %.4f mAP25 %.4f" % (t_eval, *res))
    print("new route / get_instances: x %.1f" % (t_old / t_new))


def lean():
    """CONV_LEAN_EPI: k_conv_gather with and without the BatchNorm statistics epilogue (profiles/conv_lean_epilogue.txt section 2).
    The tile-7 shapes of a Res16UNet34C step on the maps of the 8-scene batch and the 96 -> 96 control on tile 2; knob 0 / 1
    alternating inside this process, three rounds, 20 calls after 3 warm-up calls, us per call (each call includes the op's
    k_pack_weights launch).  Third column of the 96 -> 128 rows = knob 1 with CONV_SLAB_TRIM=2: the three-chunk reduction as three
    1-chunk slabs; of the 256 -> 256 rows = knob 2: the lean instance on a grid of at most two workgroups per CU, which knob 1
    leaves on the instance it had.  First the GPU's own count of resident workgroups per CU."""
    import ctypes
    from languagegroundedsemseg_amd import engine
    for tile, scl in ((7, 1), (7, 2), (7, 3), (2, 3), (2, 4)):
        got = []
        for bn in (1, 0):
            r = ctypes.c_int(0)
            engine.check(engine.lib().lgs_debug_conv_gather_residency(tile, scl, bn, ctypes.byref(r)))
            got.append(r.value)
        print("resident workgroups / CU  tile %d, %d-chunk slabs: with the statistics epilogue %d, without %d" % (tile, scl, got[0], got[1]))
    coords, feats, labels = make_batch(list(range(8)), n_target=150000, shift_seed=0)
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 3, device=DEV), torch.from_numpy(coords).to(DEV))
    m, k = x.coordinate_manager, x.coordinate_map_key
    keys = [k]
    for _ in range(3):
        keys.append(m.stride(keys[-1], 2))
    # (level, K, cin, cout of the FORWARD layer, op): a dgrad reduces cout -> cin
    cases = [(0, 27, 128, 96, "dgrad"), (0, 1, 128, 96, "dgrad"), (1, 27, 128, 96, "dgrad"), (1, 1, 128, 96, "dgrad"),
             (2, 27, 128, 128, "fwd"), (2, 27, 128, 128, "dgrad"), (3, 27, 256, 256, "fwd"), (3, 27, 256, 256, "dgrad"),
             (0, 27, 96, 96, "fwd"), (0, 27, 96, 96, "dgrad")]
    print("%-34s %s" % ("shape", "   ".join("round %d: knob 0 / 1%s" % (r, "" if r else " (/ 1+trim2 | 2)") for r in range(3))))
    for lvl, K, cin, cout, op in cases:
        km = m.kernel_map_handle(keys[lvl], keys[lvl], 3 if K == 27 else 1)
        n = m.size(keys[lvl])
        f = torch.randn(n, cin, device=DEV).bfloat16()
        g = torch.randn(n, cout, device=DEV).bfloat16()
        w = torch.randn(K, cin, cout, device=DEV) * 0.05
        fn = (lambda: km.conv_forward(f, w, None, False)) if op == "fwd" else (lambda: km.conv_dgrad(g, w, False))
        settings = [dict(CONV_LEAN_EPI=0), dict(CONV_LEAN_EPI=1)] + ([dict(CONV_LEAN_EPI=1, CONV_SLAB_TRIM=2)] if (cin, cout, op) == (128, 96, "dgrad") else []) + \
                   ([dict(CONV_LEAN_EPI=2)] if cin == 256 else [])
        cols = []
        for _ in range(3):
            ts = []
            for kn in settings:
                with engine.tuning(**kn):
                    ts.append(timeit(fn, 20, 3) * 1e3)
            cols.append(" / ".join("%7.1f" % t for t in ts))
        a, b_ = (cout, cin) if op == "dgrad" else (cin, cout)
        print("L%d rows %7d K=%-2d %3d->%3d %-5s  %s" % (lvl, n, K, a, b_, op, "    ".join(cols)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "lean":
        lean()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "insteval":
        insteval()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "insteval_host":
        insteval_host()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ap":
        ap()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "nearest":
        nearest()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "augment":
        augment()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "dropout":
        dropout()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "instshift":
        instshift()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "fps":
        fps()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "paste":
        paste()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "supcon":
        supcon()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "focal":
        focal()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "metrics":
        metrics()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "strided":
        strided()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "pool":
        pool()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "instnorm":
        instnorm()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "wide":
        wide()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "wgrad":
        wgrad()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "coarse":
        coarse()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "cluster":
        cluster()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "insseg":
        insseg()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "quantize":
        quantize()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "clip":
        clip()
        sys.exit(0)
    main()
