"""Registers, LDS, scratch and residency of every bf16 k_conv_gather instance, read from the compiler's assembly.  No GPU needed.

    python tools/conv_isa_table.py [path/to/lgs_conv.hip | path/to/lgs_conv.s] [--all]

A .hip source is compiled device-only (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S); a .s file is read as it
stands (e.g. the parent commit's, compiled the same way).  Per kernel descriptor: .amdhsa_next_free_vgpr is the unified register
count (architectural + accumulation registers; .amdhsa_accum_offset says where the accumulation registers start),
.amdhsa_group_segment_fixed_size the LDS bytes, .amdhsa_private_segment_fixed_size the scratch bytes.  Residency is arithmetic on
those: a SIMD lane has 512 unified registers in granules of 8, a CU 160 KB of LDS and four SIMDs, and a four-wave workgroup puts
one wave on each SIMD (eight waves: two).  The GPU's own answer is lgs_debug_conv_gather_residency (tools/microbench.py lean).
The tile id of an instance is the engine's (its instance table, asked through lgs_debug_conv_gather_instance: the library must be built).
Layout of profiles/conv_zero_loads.txt section 1; instances are <RB,NCB,WM,WN,SC,D,EPI,SCL,ROW1,BN,ONEBUF>, BN = 1: with the
BatchNorm statistics epilogue, ONEBUF = 1: one weight slab in LDS."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

LDS_PER_CU = 160 * 1024
REGS_PER_LANE = 512


def tiles():
    """-> {(RB, NCB, WM, WN, SC, D): tile id} of the bf16 instances, as the engine's instance table has them: the answers of
    lgs_debug_conv_gather_instance over launches that reach every tile (big and small maps, 1 .. 8 column blocks, SMALL_CFG)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from languagegroundedsemseg_amd import engine
    out = {}
    for knobs in [{}, {"CONV_WIDE": 0}] + [{"SMALL_CFG": v} for v in (3, 5, 7, 9, 10, 11, 12, 13)]:
        for n_pad, ks, cout in ((n, ks, c) for n in (4096, 65536) for ks in (3, 1) for c in (32, 64, 96, 128, 200, 256)):
            v = engine.ConvPlanView(n_pad, n_pad, n_pad, ks ** 3, ks ** 3, int(ks == 3), 0, int(ks == 3))
            q, g = engine.ConvPlanQuery(v, v, ks, 0, 0, 128, cout, engine.LGS_BF16, 1), engine.ConvGatherInstance()
            with engine.tuning(**knobs):
                if engine.lib().lgs_debug_conv_gather_instance(ctypes.byref(q), 0, ctypes.byref(g)) == 0:      # (else: not a k_conv_gather launch)
                    out[(g.rb, g.ncb, g.wm, g.wn, g.sc, g.d)] = g.tile_id
    return out


def assembly(path):
    if path.endswith(".s"):
        return open(path).read()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "lgs_conv.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", path, "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(text):
    """-> [(mangled name, {field: int})] of every kernel descriptor"""
    out = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        f = {k: int(v) for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size) (\d+)", m.group(2))}
        out.append((m.group(1), f))
    return out


def demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()


def rows(text, bf16_only=True):
    ks = [k for k in kernels(text) if "k_conv_gather" in k[0]]
    TILES = tiles()
    res = []
    for (_, f), name in zip(ks, demangle([k[0] for k in ks])):
        m = re.search(r"k_conv_gather<([^>]*)>", name)
        a = [x.strip() for x in m.group(1).split(",")]
        if bf16_only and a[0] != "unsigned short":
            continue
        num = [int(x.replace("true", "1").replace("false", "0")) if re.fullmatch(r"\d+|true|false", x) else x for x in a[1:]]
        if len(num) < 10:               # the parent has no BN parameter: every EPI = 0 instance carries the epilogue
            num.append(1 if num[6] == 0 else 0)
        if len(num) < 11:
            num.append(0)
        regs, lds = f["next_free_vgpr"], f["group_segment_fixed_size"]
        waves_wg = num[2] * num[3]
        per_simd = REGS_PER_LANE // ((regs + 7) // 8 * 8)
        by_regs = per_simd * 4 // waves_wg
        by_lds = LDS_PER_CU // lds if lds else 99
        acc = max(regs - f["accum_offset"], 0)          # (no accumulation register: the offset lies at or past the count)
        res.append(dict(tile=TILES.get(tuple(num[:6]), -1), inst=num, arch=regs - acc, acc=acc, regs=regs, lds=lds,
                        scratch=f["private_segment_fixed_size"], per_simd=per_simd, wg=min(by_regs, by_lds, 32 // waves_wg),
                        bound="registers" if by_regs <= by_lds else "LDS"))
    res.sort(key=lambda r: (r["tile"], r["inst"][6], r["inst"][7], r["inst"][8], -r["inst"][9]))
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    here = os.path.dirname(os.path.abspath(__file__))
    path = args[0] if args else os.path.join(here, "..", "languagegroundedsemseg_amd", "csrc", "lgs_conv.hip")
    print("  tile  instance <RB,NCB,WM,WN,SC,D,EPI,SCL,ROW1,BN,ONEBUF>   VGPR+AGPR = total   LDS B    scratch B   waves/SIMD   workgroups/CU (bound by)")
    for r in rows(assembly(path), bf16_only="--all" not in sys.argv):
        print("  %-5d <%-41s  %3d + %3d = %3d     %6d   %-9d   %-10d   %d (%s)" % (
            r["tile"], ",".join(str(x) for x in r["inst"]) + ">", r["arch"], r["acc"], r["regs"], r["lds"], r["scratch"], r["per_simd"], r["wg"], r["bound"]))


if __name__ == "__main__":
    main()
