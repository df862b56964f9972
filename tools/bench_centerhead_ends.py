"""Times the CenterHead end on one GPU at the shape of configs/nuscenes/det/centerhead/default.yaml: 6 tasks of (1, 2, 2, 1, 2, 2)
classes, B = 8, 128 x 128 maps, max_num = 500, rotated NMS (nms_thr 0.2, pre_max_size 1000, post_max_size 83, score_threshold 0.1).

  (a) `heads.centerhead_get_bboxes(..., sync=False)`: two selection launches, one decode launch, one NMS launch and the merge;
  (b) the composition the library offered before it for the same work on the same inputs: the reference's formulation of the
      selection and decode in torch ops on the GPU, then a per-task, per-sample loop of boolean-mask indexing and `iou3d.nms_gpu`
      (one read-back each).
The reference's own loop cannot be timed here: its circle NMS is a numba function and its nms_gpu a CUDA extension.

Device events around `--calls` calls after `--warmup` calls, the two paths alternating inside each of `--rounds` rounds, medians.
The kernel count of one call of (a) comes from torch.profiler (null when the profiler reports no device events).  The two paths
are first checked to keep the same rows.  Writes one JSON line, and `--out` if given.

    python tools/bench_centerhead_ends.py [--out profiles/centerhead_ends_timing.json]
"""
import argparse
import json
import statistics
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevfusion_amd import centerhead, heads, iou3d  # noqa: E402

CLASSES = [1, 2, 2, 1, 2, 2]
CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1,
           nms_type="rotate", pre_max_size=1000, post_max_size=83, nms_thr=0.2)


def make_inputs(B, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    preds = []
    for ct in CLASSES:
        size = torch.stack([torch.empty(B, H, W).uniform_(0.4, 1.8, generator=g), torch.empty(B, H, W).uniform_(0.4, 1.8, generator=g),
                            torch.empty(B, H, W).uniform_(0.0, 1.1, generator=g)], 1)
        ang = torch.empty(B, 1, H, W).uniform_(-3.14, 3.14, generator=g)
        # init_bias -2.19 of the reference's heat-map head: most of a map lies below the 0.1 threshold, the peaks above it
        p = dict(heatmap=torch.randn(B, ct, H, W, generator=g) * 1.2 - 2.19 - 2.0, reg=torch.rand(B, 2, H, W, generator=g),
                 height=torch.empty(B, 1, H, W).uniform_(-3, 1, generator=g), dim=size, rot=torch.cat([ang.sin(), ang.cos()], 1),
                 vel=torch.randn(B, 2, H, W, generator=g))
        preds.append([{k: v.to(dev) for k, v in p.items()}])
    return preds


def composition(preds, coder, cfg, K):
    """(b): torch ops for selection / decode (the host formulation's ops run on the GPU), then the loop over iou3d.nms_gpu."""
    heats = [p[0]["heatmap"] for p in preds]
    maps = [dict(reg=p[0]["reg"], height=p[0]["height"], dim=p[0]["dim"], rot=p[0]["rot"], vel=p[0]["vel"]) for p in preds]
    T = len(preds)
    boxes, scores, labels, live, post = centerhead._rows_host(heats, maps, coder, K, True, True, [True] * T, cfg["score_threshold"],
                                                              cfg["post_center_limit_range"])
    B = boxes.shape[0]
    keep = torch.zeros_like(live)
    for t in range(T):
        for b in range(B):
            rows = torch.nonzero(live[b, t])[:, 0]
            if rows.numel() == 0:
                continue
            sel = iou3d.nms_gpu(heads._lidar_bev_xyxyr(boxes[b, t][rows]), scores[b, t][rows], cfg["nms_thr"], cfg["pre_max_size"], cfg["post_max_size"])
            sel = rows[sel]
            keep[b, t, sel[post[b, t][sel]]] = True
    return keep.view(B, -1)


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--max-num", type=int, default=500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K = a.max_num
    coder = heads.CenterPointBBoxCoder([-51.2, -51.2], 8, [0.1, 0.1], post_center_range=CFG["post_center_limit_range"], max_num=K,
                                       score_threshold=0.1)
    preds = make_inputs(a.batch, a.size, a.size, dev)
    ours = lambda: heads.centerhead_get_bboxes(preds, coder, CFG, CLASSES, sync=False)   # noqa: E731
    theirs = lambda: composition(preds, coder, CFG, K)   # noqa: E731
    out = ours()
    same = bool(torch.equal(out["keep"], theirs()))
    live = int((out["scores"] >= 0.1).sum())
    for _ in range(a.warmup):
        ours(), theirs()
    t_ours, t_theirs = [], []
    for _ in range(a.rounds):
        t_ours.append(timed(ours, a.calls))
        t_theirs.append(timed(theirs, max(1, a.calls // 5)))
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ours()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        launches = n or None
    except Exception as e:   # the profiler is optional: the timings stand without it
        print(f"profiler: {e}", file=sys.stderr)
    res = dict(tool="bench_centerhead_ends", device=torch.cuda.get_device_name(0), batch=a.batch, tasks=len(CLASSES), map=[a.size, a.size],
               max_num=K, rows_at_or_above_threshold=live, rows=a.batch * len(CLASSES) * K, kept=int(out["counts"].sum()),
               same_rows_kept=same, centerhead_get_bboxes_ms=statistics.median(t_ours), centerhead_get_bboxes_ms_rounds=t_ours,
               nms_gpu_loop_composition_ms=statistics.median(t_theirs), nms_gpu_loop_composition_ms_rounds=t_theirs,
               device_kernels_per_call=launches)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
