"""Event-timed duration of one `centerhead_get_targets` call (and one `transfusion_heatmap_targets` call) at the nuScenes CenterHead
shape: 180 x 180 maps, six tasks of (1, 2, 2, 1, 2, 2) classes, max_objs 500, about 30 boxes per sample, packed inputs.

    python tools/bench_head_targets.py [--batch 4] [--iters 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevfusion_amd import heads  # noqa: E402

CLASSES = [1, 2, 2, 1, 2, 2]
CFG = dict(grid_size=[1440, 1440, 40], out_size_factor=8, voxel_size=[0.075, 0.075, 0.2], point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0],
           max_objs=500, dense_reg=1, gaussian_overlap=0.1, min_radius=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=30)
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    counts = rng.integers(args.boxes - 5, args.boxes + 6, args.batch)
    m = int(counts.sum())
    boxes = np.concatenate([rng.uniform(-53, 53, (m, 2)), rng.uniform(-3, 1, (m, 1)), rng.uniform(0.5, 12, (m, 2)), rng.uniform(0.5, 4, (m, 1)),
                            rng.uniform(-3, 3, (m, 1)), rng.uniform(-5, 5, (m, 2))], 1).astype(np.float32)
    packed = (torch.from_numpy(boxes).to(dev), torch.from_numpy(rng.integers(0, sum(CLASSES), m)).to(dev),
              torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev))
    res = dict(batch=args.batch, boxes=m, iters=args.iters)
    for name, fn in (("centerhead_get_targets", lambda: heads.centerhead_get_targets(packed, None, CLASSES, CFG, max_boxes_per_sample=64)),
                     ("transfusion_heatmap_targets", lambda: heads.transfusion_heatmap_targets(packed, None, sum(CLASSES), CFG, max_boxes_per_sample=64))):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3)
        res[name + "_us"] = dict(median=float(np.median(times)), p10=float(np.percentile(times, 10)), p90=float(np.percentile(times, 90)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
