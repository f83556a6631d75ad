"""Generates tests/golden/wgrad_f32_bits.json: SHA-256 digests of the raw bytes of the fp32 weight gradients that k_wgrad_f32,
k_wgrad_f32_lds and k_wgrad_f32s_lds (csrc/lgs_wgrad.hip) give, recorded on an MI355X from the commit BEFORE the three kernels were
rewritten over one pair-list skeleton.
tests/test_gpu_wgrad_f32_bits.py imports this file for the inputs and the runs, and compares what the tree under test gives.

    python tests/golden/make_wgrad_f32_bits.py          (on the GPU, with the engine of the commit to record built)

Scenes: helpers.small_scene.  "big" has more than 4096 voxels, the least at which the plan uses two partial slots (S = chunks / 4
with chunks of 512 positions), so blockIdx.x > 0 is run; "small" has between 513 and 767 voxels: S = 1, two chunks, the second
one half full.
Operands: seeded fp32 randn on the device, as tests/test_gpu_parity_r5.py draws them.
Every case runs under WGRAD_F32_LDS = 0, 1, 2, 3 and asserts through engine.dispatch_counts() that the launch reached the kernel
and the column-tile width (NCB) the case is meant for."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "wgrad_f32_bits.json")
DEV = "cuda:0"
KNOBS = (0, 1, 2, 3)
SCENES = {"big": dict(seed=11, n=5000, extent=40), "small": dict(seed=12, n=700, extent=24)}
# relation -> (kernel size, strided, dilation, transposed)
RELATIONS = {"k3": (3, False, 1, False), "k1": (1, False, 1, False), "k2": (2, True, 1, False), "k2t": (2, True, 1, True),
             "k3s2": (3, True, 1, False), "k3d2": (3, False, 2, False)}
# (relation, cin, cout, NCB, an operand one element off the 16-byte grid)
MAP_CASES = [("k3", 32, 32, 1, False), ("k3", 32, 64, 2, False), ("k3", 96, 96, 3, False), ("k3", 32, 128, 4, False),
             ("k3", 130, 32, 1, False), ("k3", 36, 20, 1, False), ("k3", 3, 32, 1, False), ("k3", 32, 30, 1, False),
             ("k1", 96, 200, 4, False), ("k2", 32, 64, 2, False), ("k2t", 32, 64, 2, False),
             ("k3s2", 32, 32, 1, False), ("k3d2", 32, 32, 1, False), ("k3", 32, 32, 1, True)]
CLIP = dict(n=2000, c=32, n_anchor=20, k_neg=3)


def case_name(scene, rel, cin, cout, offgrid):
    return "%s-%s-%dx%d%s" % (scene, rel, cin, cout, "-offgrid" if offgrid else "")


def all_case_names():
    return [case_name(s, *c[:3], c[4]) for s in SCENES for c in MAP_CASES] + ["clip-anchors"]


def expected_kernel(cin, cout, knob, offgrid=False):
    """the rule of wgrad_plan and launch_wgrad_f32, restated: the prefix of the launch site"""
    c = (cin + 3) // 4 * 4 if (knob != 0 and cout % 4 == 0) else cin     # input rows zero-padded to the 16-byte grid
    if knob == 0 or offgrid or c % 4 != 0 or cout % 4 != 0:
        return "k_wgrad_f32<"
    if knob == 2 or (knob >= 3 and c >= 96 and cout <= 128):
        return "k_wgrad_f32s_lds<"
    return "k_wgrad_f32_lds<"


def check_sites(sites, kernel, ncb, what):
    """the launch sites of one call: exactly one fp32 weight-gradient kernel, the expected one, at the expected NCB"""
    hit = [s for s, n in sites.items() if s.startswith("k_wgrad_f32") and n > 0]
    assert len(hit) == 1 and hit[0].startswith(kernel) and "[NCB=%d]" % ncb in hit[0], (what, kernel, ncb, sites)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class Maps:
    """one coordinate manager per scene and its kernel maps, built once"""

    def __init__(self):
        self.scenes, self.maps = {}, {}

    def get(self, scene, rel):
        import MinkowskiEngine as ME
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from helpers import small_scene
        if scene not in self.scenes:
            coords = small_scene(**SCENES[scene])
            x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=DEV), torch.from_numpy(coords).to(DEV))
            self.scenes[scene] = (x, coords.shape[0])
        if (scene, rel) not in self.maps:
            x, _ = self.scenes[scene]
            mgr, k0 = x.coordinate_manager, x.coordinate_map_key
            ks, strided, dil, _ = RELATIONS[rel]
            self.maps[(scene, rel)] = mgr.kernel_map_handle(k0, mgr.stride(k0, 2) if strided else k0, ks, dil)
        return self.maps[(scene, rel)]

    def n_voxels(self, scene):
        self.get(scene, "k3")
        return self.scenes[scene][1]


def run_map_case(maps, scene, rel, cin, cout, ncb, offgrid):
    """-> {"knob<m>": digest of gw} of one map case"""
    from languagegroundedsemseg_amd import engine
    km = maps.get(scene, rel)
    transposed = RELATIONS[rel][3]
    n_in, n_out = km._rows(transposed)
    g = torch.Generator(device=DEV).manual_seed(3)
    a = torch.randn(n_in, cin, device=DEV, generator=g)
    b = torch.randn(n_out, cout, device=DEV, generator=g)
    if offgrid:      # the same values in a contiguous [n, cin] view that starts one element (4 bytes) into a flat buffer
        flat = torch.zeros(n_in * cin + 4, device=DEV)
        flat[1:1 + n_in * cin] = a.reshape(-1)
        a = flat[1:1 + n_in * cin].view(n_in, cin)
        assert a.is_contiguous() and a.data_ptr() % 16 == 4
    out = {}
    for knob in KNOBS:
        engine.dispatch_counts(reset=True)
        with engine.tuning(WGRAD_F32_LDS=knob):
            gw = km.conv_wgrad(a, b, transposed)
        check_sites(engine.dispatch_counts(reset=True), expected_kernel(cin, cout, knob, offgrid), ncb,
                    (case_name(scene, rel, cin, cout, offgrid), knob))
        out["knob%d" % knob] = digest(gw)
    if offgrid:
        assert out["knob2"] == out["knob0"], "an operand off the 16-byte grid runs k_wgrad_f32 whatever the knob says"
    return out


def run_clip_case():
    """-> {"knob<m>": digest} of d loss / d anchors of the CLIP loss on fp32 features: the identity-map launch of the same kernels"""
    import MinkowskiEngine as ME
    from languagegroundedsemseg_amd import engine
    n, c, na, k = CLIP["n"], CLIP["c"], CLIP["n_anchor"], CLIP["k_neg"]
    g = torch.Generator().manual_seed(n + c)
    feats = torch.randn(n, c, generator=g).to(DEV)
    anchors = torch.nn.functional.normalize(torch.randn(na, c, generator=g), dim=1).to(DEV)
    labels = torch.randint(-1, na, (n,), generator=g).to(DEV)
    neg = torch.randint(0, na, (n, k), generator=g).to(DEV)
    inv = (1.0 / feats.norm(dim=1)).contiguous()
    g_dpos, g_dneg = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    be = ME.get_backend()
    out = {}
    for knob in KNOBS:
        engine.dispatch_counts(reset=True)
        with engine.tuning(WGRAD_F32_LDS=knob):
            gt = be.clip_loss_backward_anchors((feats, anchors, labels, neg, inv), g_dpos, g_dneg, -1)
        check_sites(engine.dispatch_counts(reset=True), expected_kernel(c, (na + 7) // 8 * 8, knob), 1, ("clip-anchors", knob))
        out["knob%d" % knob] = digest(gt)
    return out


def run_all():
    maps = Maps()
    assert maps.n_voxels("big") > 4096 and 512 < maps.n_voxels("small") < 768, (maps.n_voxels("big"), maps.n_voxels("small"))
    cases = {case_name(s, *c[:3], c[4]): run_map_case(maps, s, *c) for s in SCENES for c in MAP_CASES}
    cases["clip-anchors"] = run_clip_case()
    torch.cuda.synchronize()
    return cases


def environment():
    return {"hip": torch.version.hip, "arch": torch.cuda.get_device_properties(0).gcnArchName}


def main():
    sys.path.insert(0, ROOT)
    cases = run_all()
    doc = dict(environment(), cases=cases)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases, %d digests" % (len(cases), sum(len(v) for v in cases.values())))


if __name__ == "__main__":
    main()
