"""Times the two non-learned ends of TransFusionHead on an MI355X at the flagship shape (C = 10, H = W = 180, Cf = 128, K = 200,
B = 8 and B = 1):

  (i)  the reference's formulation in torch ops on the same device — selection: sigmoid, max_pool2d, compare, a full argsort of
       C * H * W values per sample and three gathers; get_bboxes: the score / decode op chain, boolean-mask indexing per sample
       and, for nms_type "circle", the round trip to the host and the greedy loop there per task (a numpy loop here, numba in the
       reference: the "none" rows carry no host loop and compare like for like) — the yardstick;
  (ii) this package's device path (csrc/ext/head_ends.hip): `transfusion_select_proposals` and `transfusion_get_bboxes` with
       sync=False (no read-back) and sync=True (one read-back of the B counts).

Device events around `--iters` calls after `--warmup` calls, the paths alternating inside every round; the median round is
reported.  Selection and get_bboxes are reported separately.

    python tools/bench_head_ends.py [--iters 20] [--warmup 5] [--rounds 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevfusion_amd import heads  # noqa: E402

C, H, W, CF, K = 10, 180, 180, 128, 200
CODER = dict(pc_range=[-54.0, -54.0], out_size_factor=8, voxel_size=[0.075, 0.075],
             post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], score_threshold=0.0, code_size=10)


def torch_select(logits, feat, pos):
    """(i): transfusion.py:239-295, :322-325 op for op on GPU tensors (the default, unstable argsort)."""
    B = logits.shape[0]
    heatmap = heads._suppressed_heatmap_host(logits, 3, "nuScenes")
    top = heatmap.view(B, -1).argsort(dim=-1, descending=True)[..., :K]
    cls, idx = top // heatmap.shape[-1], top % heatmap.shape[-1]
    qf = feat.gather(index=idx[:, None, :].expand(-1, feat.shape[1], -1), dim=-1)
    qp = pos.repeat(B, 1, 1).gather(index=idx[:, None, :].permute(0, 2, 1).expand(-1, -1, 2), dim=1)
    qs = heatmap.gather(index=idx[:, None, :].expand(-1, C, -1), dim=-1)
    return cls, idx, qf, qp, qs, heatmap.view(B, -1).gather(1, top)


def torch_get_bboxes(preds, labels, coder, cfg):
    """(i): transfusion.py:725-838 on GPU tensors."""
    one_hot = F.one_hot(labels, num_classes=C).permute(0, 2, 1)
    score = preds["heatmap"].sigmoid() * preds["query_heatmap_score"] * one_hot
    boxes, scores, lab = heads._decode_host(score, preds["rot"], preds["dim"], preds["center"], preds["height"], preds["vel"], coder)
    valid = heads._valid_host(boxes, scores, coder)
    out = []
    for i in range(boxes.shape[0]):
        b3, sc, lb = boxes[i, valid[i]], scores[i, valid[i]], lab[i, valid[i]]
        if cfg["nms_type"] is not None:
            keep = heads._task_loop_keep(b3, sc, lb, torch.ones_like(sc, dtype=torch.bool), cfg)
            b3, sc, lb = b3[keep], sc[keep], lb[keep]
        out.append(dict(bboxes=b3, scores=sc, labels=lb))
    return out


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_ends needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    coder = heads.TransFusionBBoxCoder(**CODER)
    results = {}
    for B in (8, 1):
        rng = np.random.default_rng(B)
        f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)   # noqa: E731
        logits = f32(rng.standard_normal((B, C, H, W)) * 2 - 4)               # a trained heatmap is mostly far below zero
        feat = f32(rng.standard_normal((B, CF, H * W)))
        pos = f32(rng.uniform(0, 180, (1, H * W, 2)))
        sel = heads.transfusion_select_proposals(logits, feat, pos, K, 3, "nuScenes")
        ref = torch_select(logits, feat, pos)
        assert torch.allclose(ref[5], sel.top_proposals_score, rtol=1e-6, atol=0)   # the same scores (near-ties may swap neighbours)
        preds = dict(heatmap=f32(rng.uniform(-3, 3, (B, C, K))), rot=f32(rng.uniform(-1, 1, (B, 2, K))),
                     dim=f32(rng.uniform(-0.5, 1.2, (B, 3, K))), height=f32(rng.uniform(-2, 2, (B, 1, K))),
                     center=sel.query_pos.permute(0, 2, 1).contiguous() + f32(rng.uniform(-1, 1, (B, 2, K))),
                     vel=f32(rng.uniform(-5, 5, (B, 2, K))), query_heatmap_score=sel.query_heatmap_score)
        labels = sel.top_proposals_class
        paths = {"select/torch_reference": lambda: torch_select(logits, feat, pos),
                 "select/device": lambda: heads.transfusion_select_proposals(logits, feat, pos, K, 3, "nuScenes")}
        for nms in (None, "circle"):
            cfg = dict(dataset="nuScenes", nms_type=nms)
            tag = f"get_bboxes_{nms or 'none'}"
            paths[tag + "/torch_reference"] = lambda cfg=cfg: torch_get_bboxes(preds, labels, coder, cfg)
            paths[tag + "/device_nosync"] = lambda cfg=cfg: heads.transfusion_get_bboxes(preds, labels, coder, cfg, K, C, sync=False)
            paths[tag + "/device_sync"] = lambda cfg=cfg: heads.transfusion_get_bboxes(preds, labels, coder, cfg, K, C, sync=True)
            want, got = paths[tag + "/torch_reference"](), paths[tag + "/device_sync"]()
            assert [len(r["scores"]) for r in want] == [len(r["scores"]) for r in got], tag      # the same boxes survive
        with torch.no_grad():
            for fn in paths.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            rounds = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, fn in paths.items():
                    rounds[k].append(timed(fn, args.iters))
        results[f"B{B}"] = dict(ms={k: sorted(v)[len(v) // 2] for k, v in rounds.items()},
                                spread={k: [min(v), max(v)] for k, v in rounds.items()})
    line = json.dumps(dict(shape=dict(C=C, H=H, W=W, Cf=CF, K=K), results=results))
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
