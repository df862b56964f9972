"""GPU: the CenterHead end kernels (csrc/ext/centerpoint_ends.hip) against tests/golden/centerhead_ref.npz (the REFERENCE on CPU
torch with its rotated NMS backed by the oracle, see tests/golden/make_centerhead_golden.py) and, where the reference leaves the
order open, against the host formulation with a stable argsort.

Bars (test_gpu_head_ends.column_bars): selection order, labels, kept rows and counts exactly equal; the centre and velocity
columns of the boxes bit-equal (same fp32 operations, no FMA contraction); dim, yaw, height and score columns within 4 x the
reference CPU result's own maximum error against the fixture's float64 values, per column, with a floor of 2 ulp of the column's
largest magnitude.  Shapes: B = 2, T = 3 tasks of (1, 2, 2) classes, 16 x 16 and 12 x 20 maps, K = 32 and 130; NMS segments of 0,
1, 2, 65 and 130 live rows (the 64-row block boundary inside a segment, one segment past two blocks)."""
import numpy as np
import pytest
import torch

import iou3d_families as families
from bevfusion_amd import heads, iou3d
from conftest import record_parity
from test_centerhead_ends import (TIE_CFG, case_preds, check_case, check_decode, check_sync, gen, get_bboxes, gold, tie_coder,  # noqa: F401
                                  tie_preds)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(gen.CASES))
def test_get_bboxes_matches_the_reference(case, gold, dev):
    preds = case_preds(case, gold, dev)
    before = [{k: v.clone() for k, v in p[0].items()} for p in preds]
    out = get_bboxes(case, preds, sync=False)
    assert all(torch.equal(p[0][k], b[k]) for p, b in zip(preds, before) for k in b), "the inputs were modified"
    assert all(v.is_cuda for v in out.values())
    rows = check_case(case, gold, out, record_parity)
    check_sync(out, get_bboxes(case, preds), rows)                        # sync=True: the reference's list, row for row


def test_the_caps_bite_on_the_device(gold, dev):
    for case, key, loose in (("premax_16_k32", "pre_max_size", 1000), ("postmax_16_k130", "post_max_size", 83)):
        tight = get_bboxes(case, case_preds(case, gold, dev), sync=False)
        free, host = get_bboxes(case, case_preds(case, gold, dev), sync=False, **{key: loose}), get_bboxes(case, case_preds(case, gold), sync=False, **{key: loose})
        assert not torch.equal(tight["keep"], free["keep"]) and torch.equal(free["keep"].cpu(), host["keep"])


@pytest.mark.parametrize("reg", [True, False])
def test_coder_decode_matches_the_reference(reg, gold, dev):
    check_decode(reg, gold, dev)


def test_equal_scores_come_in_the_host_order(dev):
    """Logits from two values: the device selection, labels and kept rows equal the host formulation's (stable argsort)."""
    want = heads.centerhead_get_bboxes(tie_preds(), tie_coder(), TIE_CFG, [1, 2], sync=False)
    got = heads.centerhead_get_bboxes(tie_preds(dev), tie_coder(), TIE_CFG, [1, 2], sync=False)
    assert torch.equal(got["labels"].cpu(), want["labels"]) and torch.equal(got["keep"].cpu(), want["keep"])
    assert torch.equal(got["bboxes"][..., :2].cpu(), want["bboxes"][..., :2]) and torch.equal(got["counts"].cpu(), want["counts"])
    assert gen.ulps(got["scores"].cpu().numpy(), want["scores"].numpy()).max() <= 2


def test_segmented_nms_keeps_the_rows_of_nms_sorted(dev):
    """Axis-aligned boxes in clusters, far from the threshold either way (IoU of a cluster's members >= 0.6, of others 0): the
    segmented kernel and iou3d.nms_sorted keep the same rows.  130 rows: two full blocks of 64 and a tail."""
    rng = np.random.default_rng(11)
    S, R = 3, 130
    anchors = np.stack(np.meshgrid(np.arange(8) * 10.0, np.arange(8) * 10.0), -1).reshape(-1, 2)
    boxes = np.zeros((S, R, 7), np.float32)
    for s in range(S):
        a = anchors[rng.integers(0, [8, 40, 64][s], R)]
        boxes[s, :, :2] = a + rng.uniform(-0.2, 0.2, (R, 2))
        boxes[s, :, 3:5] = rng.uniform(3.8, 4.0, (R, 2))
        boxes[s, :, 5] = 1.5
    b = torch.from_numpy(boxes).to(dev)
    keep, counts = heads.rotate_nms_segments(b, None, 0.3)
    for s in range(S):
        bev = heads._lidar_bev_xyxyr(b[s])
        ious = iou3d.boxes_iou_bev(bev, bev)
        assert not ((ious > 0.01) & (ious < 0.6)).any()
        rows = iou3d.nms_sorted(bev, 0.3)
        assert torch.equal(torch.nonzero(keep[s])[:, 0], rows) and int(counts[s]) == len(rows) and 1 < len(rows) < R
    host, _ = heads.rotate_nms_segments(b.cpu(), None, 0.3)
    assert torch.equal(keep.cpu(), host)


def test_segmented_nms_on_clusters_of_duplicates(dev):
    """Detector-like input (tests/iou3d_families.clusters: objects 12 m apart with 1 .. 12 copies each, among them bit-exact
    duplicates, yaw + pi and sizes exchanged with yaw + pi / 2), rows in descending score, one segment with a third of its rows
    not live.  At 0.2 the kept rows are the first live copy of every object, which needs no oracle; they are also the rows of
    iou3d.nms_sorted over the live rows and of the host path."""
    S, R, thr = 3, 130, 0.2
    boxes, objs = np.zeros((S, R, 7), np.float32), np.zeros((S, R), np.int64)
    for s in range(S):
        b5, scores, obj = families.clusters(R, seed=families.SEGMENT_SEEDS[s])
        order = np.argsort(-scores, kind="stable")
        boxes[s], objs[s] = families.lift(b5[order]), obj[order]
        intra = families.intra_cluster_ious(families.lidar_bev(boxes[s]), objs[s])
        assert intra.min() > thr + 1e-3, "a cluster pair sits within 1e-3 of the threshold: choose another seed"
    live = np.ones((S, R), bool)
    live[1, np.random.default_rng(4).choice(R, R // 3, replace=False)] = False
    b, lv = torch.from_numpy(boxes).to(dev), torch.from_numpy(live).to(dev)
    keep, counts = heads.rotate_nms_segments(b, lv, thr)
    for s in range(S):
        rows = np.nonzero(live[s])[0]
        truth = rows[np.unique(objs[s][rows], return_index=True)[1]]       # first live row of every object
        got = torch.nonzero(keep[s])[:, 0].cpu().numpy()
        assert np.array_equal(got, np.sort(truth)) and int(counts[s]) == len(truth) and 1 < len(truth) < len(rows)
        sorted_rows = iou3d.nms_sorted(heads._lidar_bev_xyxyr(b[s][lv[s]]), thr).cpu().numpy()
        assert np.array_equal(rows[sorted_rows], got)
    host, host_counts = heads.rotate_nms_segments(b.cpu(), lv.cpu(), thr)
    assert torch.equal(keep.cpu(), host) and torch.equal(counts.cpu(), host_counts)


def test_more_than_1024_rows_per_segment_raise(dev):
    preds = [[dict(heatmap=torch.zeros(1, 1, 40, 40, device=dev), reg=torch.zeros(1, 2, 40, 40, device=dev),
                   height=torch.zeros(1, 1, 40, 40, device=dev), dim=torch.zeros(1, 3, 40, 40, device=dev),
                   rot=torch.ones(1, 2, 40, 40, device=dev))]]
    coder = heads.CenterPointBBoxCoder([-8, -8], 8, [0.5, 0.5], post_center_range=[-900.0] * 3 + [900.0] * 3, max_num=1025)
    with pytest.raises(RuntimeError, match="1024"):
        heads.centerhead_get_bboxes(preds, coder, dict(TIE_CFG, nms_type="rotate"), [1])
    with pytest.raises(RuntimeError, match="not supported"):
        heads.rotate_nms_segments(torch.zeros(1, 1025, 7, device=dev), None, 0.2)


def test_selection_decode_and_both_nms_replay_in_one_graph(gold, dev):
    """A mixed rotate / circle configuration captured on one stream, replayed on fresh inputs: the replay equals the eager call."""
    case, other = "mixed_rect_k32_nonorm_scalar", "rot_rect_k130_nested"
    static = case_preds(case, gold, dev)
    fresh = [case_preds(other, gold, dev), [[{k: v.clone() for k, v in p[0].items()}] for p in static]]
    keys = ("bboxes", "scores", "labels", "keep", "counts")

    def step():
        return get_bboxes(case, static, sync=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                             # warm-up: builds the cached segment tables
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for new in fresh:
        for p, q in zip(static, new):
            for k in p[0]:
                p[0][k].copy_(q[0][k])
        graph.replay()
        torch.cuda.synchronize()
        got = [out[k].clone() for k in keys]
        want = step()
        assert all(torch.equal(g, want[k]) for g, k in zip(got, keys))
    assert int(got[4].sum()) == int(gold[case + ".counts"].sum())          # the last replay ran the fixture's inputs
