"""Event-timed duration of `seg_iou_counts` against the reference's own torch formulation (the body of evaluate_map), on the same
GPU in the same process, alternating the two per round, at the config shape: 4 samples of [6, 200, 200], seven thresholds.  Prints
one JSON line: the medians in microseconds, the bytes the op has to move (every prediction and label read once: 5 bytes a cell) and
the achieved bytes/s of ours against the 8 TB/s HBM peak.

    python profiles/seg_head_timing.py [--iters 200] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevfusion_amd import heads, seg_head  # noqa: E402

HBM_PEAK = 8e12


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def torch_counts(pred, label, thresholds):
    K = pred.shape[1]
    tp = torch.zeros(K, len(thresholds), device=pred.device)
    fp, fn = torch.zeros_like(tp), torch.zeros_like(tp)
    for s in range(pred.shape[0]):
        p = pred[s].reshape(K, -1)[:, :, None] >= thresholds
        l = label[s].bool().reshape(K, -1)[:, :, None]
        tp += (p & l).sum(dim=1)
        fp += (p & ~l).sum(dim=1)
        fn += (~p & l).sum(dim=1)
    return tp, fp, fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_head_timing needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pred = torch.rand(args.samples, 6, 200, 200, device=dev)
    label = torch.rand(args.samples, 6, 200, 200, device=dev) < 0.3
    thr = torch.tensor(seg_head.MAP_THRESHOLDS, device=dev)
    ours, theirs = (lambda: heads.seg_iou_counts(pred, label, thr)), (lambda: torch_counts(pred, label, thr))
    got, (tp, fp, fn) = ours(), theirs()
    assert torch.equal(got.float(), torch.stack([tp, fp, fn], dim=-1)), "the two formulations disagree"
    for f in (ours, theirs):
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(args.rounds):                              # alternating: both see the same machine
        a.append(timed(ours, args.iters))
        b.append(timed(theirs, args.iters))
    nbytes = pred.numel() * 5
    ours_us, torch_us = float(np.median(a)), float(np.median(b))
    print(json.dumps(dict(op="seg_iou_counts", samples=args.samples, iters=args.iters, rounds=args.rounds, ours_us=ours_us, torch_us=torch_us,
                          ours_min_max_us=[min(a), max(a)], torch_min_max_us=[min(b), max(b)], speedup=torch_us / ours_us, bytes=nbytes,
                          ours_bytes_per_s=nbytes / (ours_us * 1e-6), share_of_hbm_peak=nbytes / (ours_us * 1e-6) / HBM_PEAK)))


if __name__ == "__main__":
    main()
