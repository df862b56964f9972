"""Event-timed forward + backward of `transfusion_loss` and `centerhead_loss` at the config shapes against the reference's
formulation in torch ops (`head_losses._losses_host`) on the same GPU in the same process, the two alternating per round.

  TransFusion: B = 4, dense map 10 x 180 x 180, 200 proposals, one decoder layer, 10-column code.
  CenterHead : B = 4, six tasks of (1, 2, 2, 1, 2, 2) classes at 180 x 180, max_objs 500, about 30 boxes per sample.

Writes profiles/head_losses_timing.json (or --out) and prints it: medians in microseconds of one eager forward + backward, wrapper
included, and the bytes the dense part has to move (8 B a cell forward, 12 B backward).  The torch formulation is given every
count as a device tensor (a clamp where the reference calls `.item()` and `max`), so it pays none of the reference's read-backs:
what is compared is launches and traffic alone, which favours the torch side.

    python tools/bench_head_losses.py [--iters 100] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevfusion_amd import head_losses, heads  # noqa: E402

CLASSES = (1, 2, 2, 1, 2, 2)
SIZE, K, C, MAX_OBJS = 180, 200, 10, 500
CODE_WEIGHTS = list(head_losses._DEFAULT_CODE_WEIGHTS)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def heat_target(g, shape, dev, ones):
    t = torch.rand(shape, generator=g, device=dev) ** 6
    flat = t.view(-1)
    flat[torch.randperm(flat.numel(), generator=g, device=dev)[:ones]] = 1.0
    return t


def transfusion_inputs(B, dev, g):
    preds = {"dense_heatmap": torch.randn(B, C, SIZE, SIZE, generator=g, device=dev), "heatmap": torch.randn(B, C, K, generator=g, device=dev)}
    for n, w in zip(head_losses.PIECES, (2, 1, 3, 2, 2)):
        preds[n] = torch.randn(B, w, K, generator=g, device=dev)
    labels = torch.full((B, K), C, dtype=torch.int64, device=dev)
    pos = torch.rand(B, K, generator=g, device=dev) < 0.15
    labels[pos] = torch.randint(0, C, (int(pos.sum()),), generator=g, device=dev)
    live = (labels < C)[..., None]
    num_pos = live.sum().to(torch.int32)
    targets = (labels, torch.ones(B, K, dtype=torch.int64, device=dev), torch.randn(B, K, 10, generator=g, device=dev) * live,
               live.expand(B, K, 10).float().contiguous(), None, num_pos, torch.full((), 0.3, device=dev),
               heat_target(g, (B, C, SIZE, SIZE), dev, 30 * B))
    return preds, targets


def centerhead_inputs(B, dev, g):
    preds, anno, inds, masks = [], [], [], []
    flat = heat_target(g, (B * sum(CLASSES) * SIZE * SIZE,), dev, 30 * B)
    heat, base = [], 0
    for c in CLASSES:
        d = {"heatmap": torch.randn(B, c, SIZE, SIZE, generator=g, device=dev)}
        for n, w in zip(head_losses.CH_PIECES, (2, 1, 3, 2, 2)):
            d[n] = torch.randn(B, w, SIZE, SIZE, generator=g, device=dev)
        preds.append(d)
        heat.append(flat[base:base + B * c * SIZE * SIZE].view(B, c, SIZE, SIZE))
        base += B * c * SIZE * SIZE
        mask = torch.zeros(B, MAX_OBJS, dtype=torch.uint8, device=dev)
        mask[:, :5 * c] = 1
        masks.append(mask)
        inds.append(torch.randint(0, SIZE * SIZE, (B, MAX_OBJS), generator=g, device=dev) * mask)
        anno.append(torch.randn(B, MAX_OBJS, 10, generator=g, device=dev) * mask[..., None])
    return preds, (heat, anno, inds, masks)


def leaves_of(preds):
    if isinstance(preds, dict):
        return {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    return [leaves_of(d) for d in preds]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_losses_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_losses needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    B = args.batch
    tf_preds, tf_targets = transfusion_inputs(B, dev, g)
    ch_preds, ch_targets = centerhead_inputs(B, dev, g)
    tf_leaves, ch_leaves = leaves_of(tf_preds), leaves_of(ch_preds)
    cfgs = (head_losses._CLS, head_losses._BOX, head_losses._HEAT)

    every_leaf = list(tf_leaves.values()) + [v for d in ch_leaves for v in d.values()]

    def backward(losses):
        for v in every_leaf:
            v.grad = None
        sum(v for k, v in losses.items() if k != "matched_ious").backward()

    def tf_ours():
        backward(heads.transfusion_loss(tf_leaves, tf_targets, K, C, 1))

    def tf_torch():
        backward(head_losses._losses_host("transfusion", tf_leaves, tf_targets, K, C, 1, CODE_WEIGHTS, *cfgs))

    def ch_ours():
        backward(heads.centerhead_loss(ch_leaves, ch_targets))

    def ch_torch():
        backward(head_losses._losses_host("centerhead", ch_leaves, ch_targets, CODE_WEIGHTS, head_losses._HEAT, head_losses._BOX))

    runs = {"transfusion_loss": tf_ours, "transfusion_torch": tf_torch, "centerhead_loss": ch_ours, "centerhead_torch": ch_torch}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            samples[k].append(timed(fn, args.iters))
    cells_tf, cells_ch = B * C * SIZE * SIZE, B * sum(CLASSES) * SIZE * SIZE
    res = dict(batch=B, iters=args.iters, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               what="median microseconds of one eager forward + backward, Python wrapper and autograd included",
               us={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in samples.items()},
               dense_bytes=dict(transfusion=20 * cells_tf, centerhead=20 * cells_ch),
               launches=dict(transfusion_loss=dict(forward=3, backward=2), centerhead_loss=dict(forward=3, backward=3)))
    res["ratio_torch_over_ours"] = dict(transfusion=res["us"]["transfusion_torch"]["median"] / res["us"]["transfusion_loss"]["median"],
                                        centerhead=res["us"]["centerhead_torch"]["median"] / res["us"]["centerhead_loss"]["median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
