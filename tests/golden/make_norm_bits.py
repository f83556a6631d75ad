"""Generates tests/golden/norm_bits.json: SHA-256 digests of everything the BatchNorm kernels of csrc/lgs_norm.hip write, on every
path (`three`, `fold`, `fused`, the conv-epilogue partial rows, the split entry points), recorded on an MI355X from the commit BEFORE
their arithmetic moved into csrc/lgs_normmath.h.  The cases, the inputs and the runs are those of tests/test_gpu_norm_bits.py, which
this file imports.

    python tests/golden/make_norm_bits.py [out.json [per_output.json]]     (on the GPU, with the engine of the commit to record built)

per_output.json (not committed): the digest of every single output, to find which one moved when a variant's digest does."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "norm_bits.json")


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_gpu_norm_bits as t
    cases, detail = {}, {}
    for path, n, c, dt in t.CASES:
        name = t.case_name(path, n, c, dt)
        cases[name], detail[name] = t.run_case(path, n, c, dt)
    for dt, c in t.EXTRA:
        name = "extra-c%d-%s" % (c, dt)
        cases[name], detail[name] = t.run_extra(dt, c)
    env = {"hip": torch.version.hip, "arch": torch.cuda.get_device_properties(0).gcnArchName}
    for doc, out in ((cases, sys.argv[1] if len(sys.argv) > 1 else PATH), (detail, sys.argv[2] if len(sys.argv) > 2 else None)):
        if out:
            with open(out, "w") as f:
                json.dump(dict(env, cases=doc), f, indent=0, sort_keys=True)
                f.write("\n")
    print("wrote %d cases, %d digests" % (len(cases), sum(len(v) for v in cases.values())))


if __name__ == "__main__":
    main()
