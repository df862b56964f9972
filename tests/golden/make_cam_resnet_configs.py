"""Records the `encoders.camera.backbone` and `encoders.camera.neck` blocks of the reference YAMLs that tests/test_cam_resnet.py builds
(settings only), so that the test runs without the reference tree:

    python tests/golden/make_cam_resnet_configs.py /path/to/reference/configs
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

LEAVES = ["nuscenes/det/centerhead/lssfpn/camera/256x704/resnet/default.yaml",
          "nuscenes/det/centerhead/lssfpn/camera+radar/resnet50/default.yaml"]
OUT = os.path.join(HERE, "cam_resnet_configs.json")


def blocks(configs, leaf):
    from bevfusion_amd.config import load_config

    camera = load_config(os.path.join(configs, leaf))["model"]["encoders"]["camera"]
    return dict(backbone=camera.get("backbone"), neck=camera.get("neck"))


if __name__ == "__main__":
    rec = {leaf: blocks(sys.argv[1], leaf) for leaf in LEAVES}
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
