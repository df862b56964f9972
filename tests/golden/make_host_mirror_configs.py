"""tests/golden/host_mirror_configs.json: the two reference configs tests/test_host_mirror.py builds modules from, as
bevfusion_amd.config.load_config resolves them (inheritance merged, every ${...} evaluated: settings only).

    python tests/golden/make_host_mirror_configs.py /path/to/reference/configs"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bevfusion_amd.config import load_config  # noqa: E402

CONFIGS = {
    "flagship": "nuscenes/det/transfusion/secfpn/camera+lidar/swint_v0p075/convfuser.yaml",
    "camera_lss": "nuscenes/det/centerhead/lssfpn/camera/256x704/swint/default.yaml",
}

if __name__ == "__main__":
    src = sys.argv[1]
    out = {name: load_config(os.path.join(src, rel)) for name, rel in CONFIGS.items()}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_mirror_configs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
