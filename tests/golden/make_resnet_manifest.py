"""Writes tests/golden/resnet_manifest.json: state-dict keys / shapes and parameter counts of the reference's ResNet encoders
(models/resnet.py: ResNet14 / 18 / 34), instantiated from the reference's own model files through the MinkowskiEngine alias
package.  tests/test_strided_conv_cpu.py pins languagegroundedsemseg_amd.models against it.

    python tests/golden/make_resnet_manifest.py <path of the reference checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import MinkowskiEngine as ME  # noqa: E402,F401
from helpers import Cfg  # noqa: E402


def main(reference):
    sys.path.insert(0, reference)
    from models import resnet
    out = {}
    for name in ["ResNet14", "ResNet18", "ResNet34"]:
        m = getattr(resnet, name)(3, 200, Cfg())
        out[name] = {"num_parameters": int(sum(p.numel() for p in m.parameters())),
                     "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]}
    with open(os.path.join(HERE, "resnet_manifest.json"), "w") as f:
        json.dump(out, f)
    print("manifest:", {k: v["num_parameters"] for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
