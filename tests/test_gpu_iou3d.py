"""GPU parity of the HIP iou3d (csrc/iou3d.hip through the C ABI and the reference-named Python API) against the golden
outputs of the reference's own kernels and against the CPU oracle.

Bars: overlap / IoU within 1e-4 (fp32 geometry with device sin/cos/atan2; north_star tolerance for float outputs);
NMS keep sets bit-exact on the fixtures (no pair sits within rounding of a threshold); device sweep == oracle sweep."""
import os

import numpy as np
import pytest
import torch

import iou3d_families as families
import oracle
from bevfusion_amd import iou3d
from conftest import record_parity

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "iou3d_ref.npz")


def _boxes(rng, n, spread):
    c, wh = rng.uniform(-spread, spread, (n, 2)), rng.uniform(0.4, 6.0, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


def test_pairwise_vs_reference_golden(dev):
    z = np.load(GOLDEN)
    a, b = torch.from_numpy(z["boxes_a"]).to(dev), torch.from_numpy(z["boxes_b"]).to(dev)
    ov = iou3d.boxes_overlap_bev(a, b).cpu().numpy()
    iou = iou3d.boxes_iou_bev(a, b).cpu().numpy()
    assert np.max(np.abs(ov - z["overlap"])) <= 1e-4 and np.max(np.abs(iou - z["iou"])) <= 1e-4
    # drop-in module: writes into caller tensors
    out = torch.zeros((a.shape[0], b.shape[0]), device=dev)
    assert iou3d.iou3d_cuda.boxes_iou_bev_gpu(a, b, out) == 1
    assert torch.equal(out.cpu(), torch.from_numpy(iou))


@pytest.mark.parametrize("m,n", [(1, 1), (3, 200), (65, 64), (130, 257)])
def test_pairwise_vs_oracle_random(dev, m, n):
    rng = np.random.default_rng(m * 1000 + n)
    a, b = _boxes(rng, m, 8.0), _boxes(rng, n, 8.0)
    got = iou3d.boxes_iou_bev(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    assert np.max(np.abs(got - oracle.iou3d_pairwise(a, b, "iou"))) <= 1e-4
    got = iou3d.boxes_overlap_bev(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    assert np.max(np.abs(got - oracle.iou3d_pairwise(a, b, "overlap"))) <= 1e-4


def test_nms_vs_reference_golden(dev):
    z = np.load(GOLDEN)
    boxes = torch.from_numpy(z["nms_boxes"]).to(dev)
    scores = torch.arange(boxes.shape[0], 0, -1, device=dev, dtype=torch.float32)   # already in score order
    for thr in ("0.1", "0.5"):
        assert np.array_equal(iou3d.nms_gpu(boxes, scores, float(thr)).cpu().numpy(), z[f"nms_keep_{thr}"])
        assert np.array_equal(iou3d.nms_normal_gpu(boxes, scores, float(thr)).cpu().numpy(), z[f"nms_normal_keep_{thr}"])
        keep = torch.zeros(boxes.shape[0], dtype=torch.long)
        k = iou3d.iou3d_cuda.nms_gpu(boxes, keep, float(thr), 0)
        assert np.array_equal(keep[:k].numpy(), z[f"nms_keep_{thr}"])


@pytest.mark.parametrize("n,spread,thr", [(1, 5.0, 0.3), (63, 4.0, 0.3), (64, 4.0, 0.2), (65, 4.0, 0.2), (1000, 9.0, 0.25),
                                          (5000, 40.0, 0.1)])
def test_nms_vs_oracle_random_with_scores_and_limits(dev, n, spread, thr):
    rng = np.random.default_rng(n)
    b = _boxes(rng, n, spread)
    s = rng.random(n).astype(np.float32)
    order = np.argsort(-s, kind="stable")
    want = order[oracle.iou3d_nms(b[order], thr)]
    got = iou3d.nms_gpu(torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), thr).cpu().numpy()
    assert np.array_equal(got, want)
    want_n = order[oracle.iou3d_nms(b[order], thr, normal=True)]
    assert np.array_equal(iou3d.nms_normal_gpu(torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), thr).cpu().numpy(), want_n)
    if n >= 64:
        pre = n // 2
        want_p = order[:pre][oracle.iou3d_nms(b[order[:pre]], thr)][:10]
        got_p = iou3d.nms_gpu(torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), thr, pre_maxsize=pre, post_max_size=10)
        assert np.array_equal(got_p.cpu().numpy(), want_p)
    # device-resident count variant
    keep, cnt = iou3d.nms_sorted(torch.from_numpy(b[order]).to(dev), thr, sync=False)
    assert int(cnt) == want.shape[0] and np.array_equal(order[keep[: int(cnt)].cpu().numpy()], want)


def test_empty_and_bad_inputs(dev):
    e = torch.zeros((0, 5), device=dev)
    one = torch.tensor([[0, 0, 1, 1, 0.0]], device=dev)
    assert tuple(iou3d.boxes_iou_bev(e, one).shape) == (0, 1)
    assert iou3d.nms_sorted(e, 0.5).numel() == 0
    with pytest.raises(RuntimeError, match="GPU tensor"):
        iou3d.boxes_iou_bev(torch.zeros(2, 5), one)
    with pytest.raises(RuntimeError, match=r"\[N, 5\]"):
        iou3d.boxes_iou_bev(torch.zeros((2, 7), device=dev), one)


# ---- near-duplicate, collinear and far-away boxes against float64 (tests/iou3d_families.py) ------------------------------------
@pytest.fixture(scope="module")
def refs():
    """Per family: the float64 values, the fp32 oracle's, the well-conditioned mask and the device's allowance."""
    return {name: families.reference(name) for name in families.FAMILIES}


@pytest.mark.parametrize("name", families.FAMILIES)
def test_family_pairs_stay_within_four_oracle_errors_of_float64(name, refs, dev):
    """Pair p = (A[p], B[p]) is the diagonal of the [P, P] result.  On well-conditioned pairs the device stays within
    max(4 x the oracle's own maximum error on the family, 1e-6), at most 1e-4, of float64 (overlap: scaled by the union area);
    on every pair the result is a number, not negative, and the same on a second call; off the diagonal the 1e-4 bar against
    the oracle holds as for random boxes."""
    r = refs[name]
    a, b = torch.from_numpy(r["A"]).to(dev), torch.from_numpy(r["B"]).to(dev)
    well = r["well"]
    for mode, fn, want, scale, allowed in (("iou", iou3d.boxes_iou_bev, r["iou64"], 1.0, r["bar_iou"]),
                                           ("overlap", iou3d.boxes_overlap_bev, r["ov64"], r["union"], r["bar_ov"])):
        full = fn(a, b)
        assert torch.equal(full, fn(a, b)), f"{name} {mode}: two calls differ"
        full = full.cpu().numpy()
        got = np.diagonal(full).astype(np.float64)
        assert not np.isnan(got).any() and (got >= 0).all(), f"{name} {mode}: NaN or negative on the diagonal"
        err = np.abs(got - want) / scale
        worst = float(err[well].max())
        print(f"{name} {mode}: device max error against float64 {worst:.3g} on {int(well.sum())} well-conditioned pairs "
              f"(allowed {allowed:.3g}; oracle {r['oracle_err_' + ('iou' if mode == 'iou' else 'ov')]:.3g}); "
              f"{int((err[well] > allowed).sum())} over; {int((~well).sum())} ill-conditioned")
        record_parity(f"iou3d_family/{name}/device_{mode}_vs_f64", worst, allowed)
        assert worst <= allowed, f"{name} {mode}: {worst} > {allowed} at pair {int(np.argmax(np.where(well, err, 0)))}"
        # off the diagonal: ordinary pairs (most of them apart), the bar of test_pairwise_vs_oracle_random
        off = ~np.eye(families.P, dtype=bool)
        assert np.max(np.abs(full[off] - oracle.iou3d_pairwise(r["A"], r["B"], mode)[off])) <= 1e-4


def test_special_boxes_pairwise_have_the_oracles_nans(dev):
    """The 16 pairs (A[p], B[p]): NaN where the oracle has NaN, and within 1e-4 of it where both are finite.  The other 240
    entries of the [16, 16] result pair two degenerate boxes; they must agree on NaN and on the overlap area, but not on the IoU: a
    zero-area and a negative-extent box have a union <= 0, the 1e-8 floor becomes the denominator and the rounding noise of the
    overlap (1e-8) becomes an IoU of order 1."""
    A, B = families.special()
    a, b = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    for mode, fn in (("iou", iou3d.boxes_iou_bev), ("overlap", iou3d.boxes_overlap_bev)):
        got, want = fn(a, b).cpu().numpy(), oracle.iou3d_pairwise(A, B, mode)
        assert np.array_equal(np.isnan(got), np.isnan(want)), mode
        both = np.isfinite(got) & np.isfinite(want)
        assert np.array_equal(both, np.isfinite(want)) and np.diagonal(both).sum() >= 10
        pairs = np.diagonal(both)
        assert np.max(np.abs(np.diagonal(got)[pairs] - np.diagonal(want)[pairs])) <= 1e-4, mode
        if mode == "overlap":
            assert np.max(np.abs(got[both] - want[both])) <= 1e-4


# ---- NMS on detector-like duplicates ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cluster_sets():
    out = {}
    for n in sorted(families.CLUSTER_SEEDS):
        boxes, scores, obj = families.clusters(n)
        order = np.argsort(-scores, kind="stable")
        intra = families.intra_cluster_ious(boxes, obj)
        out[n] = dict(boxes=boxes, scores=scores, obj=obj, order=order, intra=intra,
                      truth=families.top_of_each_object(scores, obj),
                      oracle={thr: order[oracle.iou3d_nms(boxes[order], thr)] for thr in families.NMS_THRESHOLDS})
    return out


@pytest.mark.parametrize("thr", families.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", sorted(families.CLUSTER_SEEDS))
def test_nms_on_clusters_of_duplicates(n, thr, cluster_sets, dev):
    """Objects 12 m apart, each with 1 .. 12 copies (jittered, bit-exact duplicates, yaw + pi, sizes exchanged with yaw + pi / 2).
    At 0.2 the kept set is the best copy of every object, which needs no oracle; at both thresholds it is the oracle's."""
    c = cluster_sets[n]
    assert np.abs(c["intra"] - thr).min() > 1e-3, "a cluster pair sits within 1e-3 of the threshold: choose another seed"
    want = c["oracle"][thr]
    if thr == 0.2:
        assert c["intra"].min() > thr and np.array_equal(want, c["truth"])
        want = c["truth"]
    boxes, scores = torch.from_numpy(c["boxes"]).to(dev), torch.from_numpy(c["scores"]).to(dev)
    assert np.array_equal(iou3d.nms_gpu(boxes, scores, thr).cpu().numpy(), want)
    srt = torch.from_numpy(c["boxes"][c["order"]]).to(dev)
    keep, cnt = iou3d.nms_sorted(srt, thr, sync=False)
    assert int(cnt) == len(want) and np.array_equal(c["order"][keep[: int(cnt)].cpu().numpy()], want)
    out = torch.zeros(n, dtype=torch.long)
    k = iou3d.iou3d_cuda.nms_gpu(srt, out, thr, 0)
    assert k == len(want) and np.array_equal(c["order"][out[:k].numpy()], want)


def test_nms_sweep_beyond_256_column_blocks(dev):
    """16 600 boxes are 260 column blocks: the sweep's `j += 256` loop takes a second trip (the other tests stop at 79 blocks).
    Rows of blocks 257 .. 259 are suppressed only by rows kept in blocks 0 .. 2, which only that second trip carries over
    (test_oracle_iou3d.py asserts it of the fixture); other late rows overlap nothing earlier and are kept.
    Axis-aligned mode: the oracle stays quick and the clusters (IoU >= 0.6 inside, 0 between) are far from the threshold."""
    boxes = families.axis_aligned_clusters(families.SWEEP_N)
    want = oracle.iou3d_nms(boxes, 0.3, normal=True)
    scores = torch.arange(families.SWEEP_N, 0, -1, device=dev, dtype=torch.float32)      # already in score order
    got = iou3d.nms_normal_gpu(torch.from_numpy(boxes).to(dev), scores, 0.3).cpu().numpy()
    assert want.max() > 256 * 64 and np.array_equal(got, want)


def test_nms_with_special_boxes_mixed_in(dev):
    """The 7 distinct boxes of the special pairs among 123 clustered ones: the kept set is the oracle's; a box with a NaN yaw
    overlaps nothing (every comparison is false), so it is kept and suppresses nothing."""
    boxes, scores, obj = families.clusters(130)
    A, B = families.special()
    odd = np.unique(np.concatenate([A, B]).view(np.uint32), axis=0).view(np.float32)
    rows = np.random.default_rng(3).choice(130, len(odd), replace=False)
    boxes[rows] = odd
    nan_rows = np.nonzero(np.isnan(boxes[:, 4]))[0]
    assert len(odd) >= 7 and len(nan_rows) == 1
    order = np.argsort(-scores, kind="stable")
    want = order[oracle.iou3d_nms(boxes[order], 0.2)]
    got = iou3d.nms_gpu(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), 0.2).cpu().numpy()
    assert np.array_equal(got, want) and nan_rows[0] in got
    without = np.delete(np.arange(130), nan_rows)                     # the same set without the NaN box keeps the same other rows
    sub = torch.from_numpy(boxes[without]).to(dev), torch.from_numpy(scores[without]).to(dev)
    assert np.array_equal(without[iou3d.nms_gpu(*sub, 0.2).cpu().numpy()], got[got != nan_rows[0]])
