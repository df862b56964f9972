"""Times TransFusionHead.get_targets' assignment end on an MI355X at the config shape (B = 4, K = 200 proposals, C = 10 classes,
40 / 120 / 7 / 260 ground-truth boxes: the seeded `config_shape` fixture of tests/golden/make_head_assign_golden.py), two ways on
the same device:

  (i)  the reference's formulation, the yardstick: per sample and decoder layer the same three costs as torch ops on the device (the
       BEV overlap by this package's `iou3d.boxes_overlap_bev`, which is the reference's own kernel restated), `cost.detach().cpu()`,
       scipy's `linear_sum_assignment` on the host, the indices copied back, and the target rows by torch indexing
       (transfusion.py:424-524, 575), plus the dense heatmap by `transfusion_heatmap_targets` (common to both routes);
  (ii) this package's device path `heads.transfusion_get_targets(..., sync=False)`: seven launches (decode, sizes, costs, solver,
       targets, heatmap zero and draw), eager and as one captured graph replay.

Host wall clock around `--iters` calls ended by a device synchronise (route (i) does host work, so device events alone would miss
it), after `--warmup` calls, the routes alternating inside every round; medians over `--rounds` paired rounds.  The tool FAILS if
the device path's median is slower than the round-trip route's: removing the B x L syncs is the point.

    python tools/bench_head_assign.py [--iters 20] [--warmup 5] [--rounds 7] [--json out.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevfusion_amd import heads, iou3d  # noqa: E402
from bevfusion_amd.registry import BBOX_ASSIGNERS  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_head_assign_golden", os.path.join(ROOT, "tests", "golden", "make_head_assign_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASE = "config_shape"
LAUNCHES = dict(transfusion_decode=1, match_costs=2, linear_sum_assignment=1, transfusion_assign_targets=1, heatmap_targets=2)


def round_trip(preds, gt_boxes, gt_labels, coder, cfg, K, L, w):
    """(i): hungarian_assigner.py:94-142 and transfusion.py:424-524, 575 on device tensors, one host round trip per problem."""
    heat = preds["heatmap"]
    B, P = heat.shape[0], heat.shape[2]
    dev = heat.device
    boxes = torch.stack([d["bboxes"] for d in coder.decode(heat, preds["rot"], preds["dim"], preds["center"], preds["height"], preds.get("vel"))])
    pc = cfg["point_cloud_range"]
    start, span = boxes.new_tensor(pc[0:2]), boxes.new_tensor(pc[3:5]) - boxes.new_tensor(pc[0:2])
    labels = boxes.new_full((B, P), gen.C, dtype=torch.long)
    label_weights = boxes.new_ones((B, P), dtype=torch.long)
    bbox_targets = boxes.new_zeros((B, P, coder.code_size))
    bbox_weights = boxes.new_zeros((B, P, coder.code_size))
    ious = boxes.new_zeros((B, P))
    num_pos, means = 0, []
    xyxyr = heads._lidar_bev_xyxyr
    for b in range(B):
        gb, gl = gt_boxes[b], gt_labels[b]
        for l in range(L):
            sl = slice(l * K, (l + 1) * K)
            pb = boxes[b, sl]
            p = heat[b, :, sl].T.sigmoid()
            neg = -(1 - p + 1e-12).log() * (1 - w["alpha"]) * p.pow(w["gamma"])
            pos = -(p + 1e-12).log() * w["alpha"] * (1 - p).pow(w["gamma"])
            cls_cost = (pos[:, gl] - neg[:, gl]) * w["cls"]
            reg_cost = torch.cdist((pb[:, :2] - start) / span, (gb[:, :2] - start) / span, p=1) * w["reg"]
            bev = iou3d.boxes_overlap_bev(xyxyr(pb).contiguous(), xyxyr(gb).contiguous())
            top = torch.min((pb[:, 2] + pb[:, 5]).view(-1, 1), (gb[:, 2] + gb[:, 5]).view(1, -1))
            bottom = torch.max(pb[:, 2].view(-1, 1), gb[:, 2].view(1, -1))
            o3 = bev * torch.clamp(top - bottom, min=0)
            va, vb = (pb[:, 3] * pb[:, 4] * pb[:, 5]).view(-1, 1), (gb[:, 3] * gb[:, 4] * gb[:, 5]).view(1, -1)
            iou = o3 / torch.clamp(va + vb - o3, min=1e-8)
            cost = (cls_cost + reg_cost - iou * w["iou"]).detach().cpu()                      # the forced sync
            r, c = linear_sum_assignment(cost)
            r, c = torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev)
            rows = r + l * K
            labels[b, rows] = gl[c]
            ious[b, rows] = iou[r, c].clamp(0.0, 1.0)
            bbox_targets[b, rows] = coder.encode(gb[c])
            bbox_weights[b, rows] = 1.0
            num_pos += int(r.shape[0])
        pos_mask = bbox_weights[b, :, 0] > 0
        means.append(float(ious[b][pos_mask].sum() / max(int(pos_mask.sum()), 1)))              # float(mean_iou): another read-back
    heatmap = heads.transfusion_heatmap_targets(gt_boxes, gt_labels, gen.C, cfg)
    return labels, label_weights, bbox_targets, bbox_weights, ious, num_pos, float(np.mean(means)), heatmap


def timed(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_assign needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    c = gen.CASES[CASE]
    K, L = c["K"], c["L"]
    d = gen.inputs(CASE)
    preds = {k: torch.from_numpy(v).to(dev) for k, v in d["preds"].items()}
    gt_boxes = [torch.from_numpy(b).to(dev) for b in d["gt_boxes"]]
    gt_labels = [torch.from_numpy(l).to(dev) for l in d["gt_labels"]]
    packed = tuple(torch.from_numpy(a).to(dev) for a in gen.packed(CASE))
    bound = max(c["G"])
    coder = heads.TransFusionBBoxCoder(**gen.coder_kwargs(CASE))
    assigner = BBOX_ASSIGNERS.build(gen.assigner_cfg(CASE))
    cfg = gen.case_cfg(CASE)

    def device():
        return heads.transfusion_get_targets(packed, None, preds, coder, assigner, cfg, K, gen.C, num_decoder_layers=L,
                                             max_boxes_per_sample=bound, sync=False)

    def reference():
        return round_trip(preds, gt_boxes, gt_labels, coder, cfg, K, L, gen.WEIGHTS)

    with torch.no_grad():
        want, got = reference(), device()
        torch.cuda.synchronize()
        assert want[5] == int(got[5]), (want[5], int(got[5]))                                  # the same number of positives
        assert abs(want[6] - float(got[6])) < 1e-3 and torch.equal(want[7], got[7])             # equal totals admit other pairs: means only
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            device()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = device()                                                                    # noqa: F841  (the replay's outputs)
        paths = {"round_trip_reference": reference, "device_eager": device, "device_graph_replay": graph.replay}
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                rounds[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    result = dict(shape=dict(B=c["B"], K=K, L=L, C=gen.C, G=list(c["G"]), max_boxes_per_sample=bound), ms_per_call=med,
                  spread={k: [min(v), max(v)] for k, v in rounds.items()}, launches=LAUNCHES, launches_total=sum(LAUNCHES.values()),
                  host_syncs=dict(round_trip_reference=c["B"] * L + c["B"], device_eager=0, device_graph_replay=0),
                  clock="host wall clock around iters calls ended by a device synchronise", iters=args.iters, rounds=args.rounds,
                  device=torch.cuda.get_device_name(0))
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    if med["device_eager"] > med["round_trip_reference"]:
        raise SystemExit(f"the device path ({med['device_eager']:.3f} ms) is slower than the round trip ({med['round_trip_reference']:.3f} ms)")


if __name__ == "__main__":
    main()
