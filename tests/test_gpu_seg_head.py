"""GPU: the IoU count kernels (csrc/ext/seg_head.hip) through the public functions against tests/golden/seg_head_ref.npz: exact
equality with the reference for every label dtype and threshold form, no host sync, graph replay over fresh contents, sizes around
the grid's steps."""
import numpy as np
import pytest
import torch

from bevfusion_amd import heads
from test_seg_head import check_metrics, gen, gold  # noqa: F401

pytestmark = pytest.mark.gpu


def on(dev):
    pred, label = gen.counts_inputs()
    return torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)


def test_counts_are_exact(gold, dev):
    p, l = on(dev)
    want = gold["counts.counts"]
    for lab in (l, l.to(torch.uint8), l.float(), l.long() * 3):
        counts = heads.seg_iou_counts(p, lab)
        assert counts.dtype == torch.int64 and counts.shape == (6, 7, 3) and np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(heads.seg_iou_counts(p, l, torch.tensor(gen.THRESHOLDS, device=dev)).cpu().numpy(), want)
    assert np.array_equal(heads.seg_iou_counts(p, l, [0.5]).cpu().numpy(), want[:, 3:4])
    assert np.array_equal(heads.seg_iou_counts(p.half(), l).cpu().numpy(), heads.seg_iou_counts(p.half().float().cpu(), l.cpu()).numpy())
    results = [dict(masks_bev=p[s], gt_masks_bev=l[s]) for s in range(p.shape[0])]
    check_metrics(heads.evaluate_map(results, list(gen.MAP_CLASSES)), gold)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 63), (1, 2, 2049), (5, 1, 4096 + 17), (2, 40, 333)])
def test_sizes_around_the_grid_steps(shape, dev):
    """One cell; less than a wave; one workgroup's share plus one; several workgroups with a ragged end; many classes.  Sixteen
    thresholds, NaN and infinite predictions: against the host formulation."""
    g = torch.Generator().manual_seed(sum(shape))
    pred = torch.rand(shape, generator=g)
    pred.view(-1)[::7] = float("nan")
    pred.view(-1)[3::11] = float("inf")
    pred.view(-1)[5::13] = -float("inf")
    label = torch.rand(shape, generator=g) < 0.5
    thr = [i / 17 for i in range(1, 17)]
    want = heads.seg_iou_counts(pred, label, thr)
    got = heads.seg_iou_counts(pred.to(dev), label.to(dev), thr)
    assert got.shape == (shape[1], 16, 3) and torch.equal(got.cpu(), want)


def test_no_host_sync_and_graph_replay(gold, dev):
    """The call captured once and replayed over fresh prediction and label contents: every replay equals the host formulation of
    its contents, with nothing left from the replay before (the call zeroes the counts itself)."""
    p, l = on(dev)
    heads.seg_iou_counts(p, l)                                              # uploads the cached thresholds
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        counts = heads.seg_iou_counts(p, l)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(counts.cpu().numpy(), gold["counts.counts"])
    pred, label = torch.zeros_like(p), torch.zeros_like(l)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        heads.seg_iou_counts(pred, label)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # a capture admits no sync and no read-back
        out = heads.seg_iou_counts(pred, label)
    g = torch.Generator().manual_seed(9)
    fresh = [(p.cpu(), l.cpu()), (torch.rand(p.shape, generator=g), torch.rand(p.shape, generator=g) < 0.1), (p.cpu(), l.cpu())]
    for a, b in fresh:
        pred.copy_(a)
        label.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), heads.seg_iou_counts(a, b))
