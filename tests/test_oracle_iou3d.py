"""CPU: the iou3d oracle (oracle/iou3d_oracle.c, a C restatement of iou3d_kernel.cu / iou3d.cpp) is pinned to
tests/golden/iou3d_ref.npz — outputs of the REFERENCE's own kernels (hipified into oracle/_ref, run on an MI355X by
tests/golden/make_iou3d_golden.py) — and cross-checked against an independent float64 polygon clipping."""
import os

import numpy as np
import pytest

import iou3d_families as families
import oracle
from conftest import record_parity

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "iou3d_ref.npz")


def test_pairwise_matches_reference_kernel_outputs():
    z = np.load(GOLDEN)
    ov = oracle.iou3d_pairwise(z["boxes_a"], z["boxes_b"], "overlap")
    iou = oracle.iou3d_pairwise(z["boxes_a"], z["boxes_b"], "iou")
    assert int((z["overlap"] > 0).sum()) > 500                       # the fixture exercises real intersections
    assert np.max(np.abs(ov - z["overlap"])) <= 2e-5                 # libm vs device sin/cos/atan2 roundings
    assert np.max(np.abs(iou - z["iou"])) <= 2e-6
    assert np.array_equal(ov > 0, z["overlap"] > 0)


def test_nms_matches_reference_kernel_outputs():
    z = np.load(GOLDEN)
    for thr in ("0.1", "0.5"):
        assert np.array_equal(oracle.iou3d_nms(z["nms_boxes"], float(thr)), z[f"nms_keep_{thr}"])
        assert np.array_equal(oracle.iou3d_nms(z["nms_boxes"], float(thr), normal=True), z[f"nms_normal_keep_{thr}"])


def test_overlap_agrees_with_float64_clipping():
    rng = np.random.default_rng(1)
    c, wh = rng.uniform(-8, 8, (60, 2)), rng.uniform(0.5, 5, (60, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(-3.2, 3.2, (60, 1))], 1).astype(np.float32)
    ov = oracle.iou3d_pairwise(boxes[:30], boxes[30:], "overlap")
    ref = np.array([[oracle.rotated_overlap_float64(a, b) for b in boxes[30:]] for a in boxes[:30]])
    assert np.max(np.abs(ov - ref)) <= 5e-5 and (ref > 0).sum() > 50


def test_known_answers():
    sq = np.array([[0, 0, 2, 2, 0.0]], np.float32)
    assert abs(oracle.iou3d_pairwise(sq, sq, "iou")[0, 0] - 1.0) < 1e-6
    half = np.array([[1, 0, 3, 2, 0.0]], np.float32)                  # half overlap: 2 / (4 + 4 - 2)
    assert abs(oracle.iou3d_pairwise(sq, half, "iou")[0, 0] - 1 / 3) < 1e-6
    rot = np.array([[0, 0, 2, 2, np.pi / 4]], np.float32)             # octagon: 8 (sqrt 2 - 1)
    assert abs(oracle.iou3d_pairwise(sq, rot, "overlap")[0, 0] - 8 * (np.sqrt(2) - 1)) < 1e-5
    far = np.array([[10, 10, 11, 11, 0.3]], np.float32)
    assert oracle.iou3d_pairwise(sq, far, "overlap")[0, 0] == 0.0
    assert oracle.iou3d_pairwise(np.zeros((0, 5), np.float32), sq, "iou").shape == (0, 1)


# ---- the families of tests/iou3d_families.py: what the reference's algorithm alone does on them ---------------------------------
def _clip_by_direction_cross(box_a, box_b):
    """The clipper this suite used before: the crossing parameter divides by the cross product of the two edge directions, which
    vanishes on parallel edges.  Kept to show that the division-safe one computes the same thing where this one is defined."""
    def corners(bx):
        x1, y1, x2, y2, ang = [float(v) for v in bx]
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
        c, s = np.cos(ang), np.sin(ang)
        return [((px - cx) * c + (py - cy) * s + cx, -(px - cx) * s + (py - cy) * c + cy)
                for px, py in [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]]

    def area(poly):
        return 0.5 * sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1]
                         for i in range(len(poly)))

    subj, clip = corners(box_a), corners(box_b)
    if area(clip) < 0:
        clip = clip[::-1]
    for i in range(4):
        p, q = clip[i], clip[(i + 1) % 4]
        if not subj:
            break
        inside = lambda r: (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]) >= 0  # noqa: E731
        out = []
        for j in range(len(subj)):
            cur, prev = subj[j], subj[j - 1]
            if inside(cur) != inside(prev):
                d1, d2 = (q[0] - p[0], q[1] - p[1]), (cur[0] - prev[0], cur[1] - prev[1])
                t = ((prev[0] - p[0]) * d2[1] - (prev[1] - p[1]) * d2[0]) / (d1[0] * d2[1] - d1[1] * d2[0])
                out.append((p[0] + t * d1[0], p[1] + t * d1[1]))
            if inside(cur):
                out.append(cur)
        subj = out
    return abs(area(subj)) if len(subj) >= 3 else 0.0


@pytest.mark.parametrize("name", families.FAMILIES)
def test_family_is_well_conditioned_but_for_a_capped_share(name):
    """The fp32 oracle against float64 on a family: at most 0.2 % of the pairs are ill-conditioned (oracle IoU more than 1e-4 off;
    the reference's own pathology), so the GPU tests cannot hide a failure behind the exclusion; the error on the rest
    is what the device's allowance is built from."""
    r = families.reference(name)
    assert r["A"].shape == r["B"].shape == (families.P, 5) and r["A"].dtype == np.float32
    assert np.isfinite(r["ov64"]).all() and np.isfinite(r["iou64"]).all() and (r["ov64"] >= 0).all()
    assert (r["iou64"] <= 1 + 1e-9).all()
    share = float((~r["well"]).mean())
    print(f"{name}: ill-conditioned {int((~r['well']).sum())} / {families.P}, oracle max error on the rest: IoU "
          f"{r['oracle_err_iou']:.3g}, overlap / union {r['oracle_err_ov']:.3g}")
    record_parity(f"iou3d_family/{name}/oracle_iou_vs_f64", r["oracle_err_iou"], families.ILL_BAR)
    record_parity(f"iou3d_family/{name}/oracle_overlap_vs_f64", r["oracle_err_ov"], families.ILL_BAR)
    record_parity(f"iou3d_family/{name}/ill_conditioned_share", share, families.MAX_ILL_SHARE)
    assert share <= families.MAX_ILL_SHARE
    lifted = families.reference_lifted(name)
    assert np.isfinite(lifted["iou64"]).all() and float((~lifted["well"]).mean()) <= families.MAX_ILL_SHARE
    record_parity(f"iou3d_family/{name}/oracle_iou3d_vs_f64", lifted["oracle_err_iou"], families.ILL_BAR)


def test_some_family_has_an_ill_conditioned_pair():
    assert sum(int((~families.reference(name)["well"]).sum()) for name in families.FAMILIES) >= 1
    assert sum(int((~families.reference_lifted(name)["well"]).sum()) for name in families.FAMILIES) >= 1


def test_families_are_what_they_say():
    A, B = families.family("duplicate")
    assert np.array_equal(A, B)
    A, B = families.family("slide")
    assert np.array_equal(A[:, 4], B[:, 4]) and np.max(np.abs((A[:, 2:4] - A[:, :2]) - (B[:, 2:4] - B[:, :2]))) < 1e-5
    A, B = families.family("right_angles")
    edge, corner = np.arange(families.P) % 4 == 0, np.arange(families.P) % 4 == 1
    even = np.isin(B[:, 4], np.float32([-np.pi, 0, np.pi]))
    assert (A[:, 4] == 0).all() and 100 < even.sum() < families.P - 100
    assert np.array_equal(B[edge & even, 0], A[edge & even, 2]) and np.array_equal(B[corner & even, :2], A[corner & even, 2:4])
    r = families.reference("right_angles")
    assert r["iou64"][edge | corner].max() < 1e-6 and (r["iou64"][~(edge | corner)] > 0.01).sum() > 200
    A, B = families.family("small_far")
    c = (A[:, :2] + A[:, 2:4]) / 2
    assert np.hypot(c[:, 0], c[:, 1]).min() > 44.9 and (A[:, 2:4] - A[:, :2]).max() < 0.81
    assert families.reference("small_far")["iou64"].min() > 0.5
    for name in ("swapped", "flipped", "duplicate"):      # the same rectangle, up to the fp32 rounding of the rewritten sizes and yaw
        assert np.abs(families.reference(name)["iou64"] - 1).max() < 1e-4, name
    A, B = families.special()
    assert A.shape == (16, 5) and np.isnan(A).any() and np.isinf(A).any()
    a7 = families.lift(families.family("random")[0])
    assert a7.shape == (families.P, 7) and (a7[:, 2] == -1).all() and (a7[:, 5] == 1.5).all()


def test_float64_clipper_on_hand_computable_cases():
    ov, iou = oracle.rotated_overlap_float64, oracle.rotated_iou_float64
    sq = np.array([0, 0, 2, 2, 0.0], np.float32)
    assert iou(sq, sq) == 1.0 and ov(sq, sq) == 4.0
    for yaw in (0.3, -2.0, np.pi / 2):                                   # identical boxes give 1 at any yaw
        b = np.array([-3.5, 1.25, 0.5, 2.0, yaw], np.float32)
        assert abs(iou(b, b) - 1.0) <= 1e-12
    assert ov(sq, np.array([2, 0, 4, 2, 0.0], np.float32)) == 0.0           # a shared edge
    assert ov(sq, np.array([2, 2, 3, 5, 0.0], np.float32)) == 0.0           # a shared corner
    assert ov(sq, np.array([2.5, 0, 4, 2, 0.0], np.float32)) == 0.0         # apart
    assert abs(iou(sq, np.array([1, 0, 3, 2, 0.0], np.float32)) - 1 / 3) <= 1e-15
    rot = np.array([0, 0, 2, 2, np.pi / 4], np.float32)                     # the octagon of two squares at pi / 4
    octagon = 8 * (np.sqrt(2) - 1)
    assert abs(ov(sq, rot) - octagon) <= 1e-6 and abs(ov(rot, sq) - octagon) <= 1e-6   # pi / 4 is rounded to fp32
    assert abs(iou(sq, rot) - octagon / (8 - octagon)) <= 1e-6
    inner = np.array([0.5, 0.5, 1.5, 1.0, 1.0], np.float32)                 # contained: the inner box's area, either way round
    assert abs(ov(sq, inner) - 0.5) <= 1e-12 and abs(ov(inner, sq) - 0.5) <= 1e-12
    assert ov(sq, np.array([2, 0, 0, 2, 0.0], np.float32)) == 4.0           # a clockwise clip polygon
    # parallel edges one ulp apart: the old clipper's denominator is a cross product of directions and vanishes here
    a = np.array([10.0, 10.0, 12.0, 11.0, 0.5], np.float32)
    b = a.copy()
    b[0] = np.nextafter(b[0], np.float32(100))
    assert abs(iou(a, b) - 1.0) <= 1e-6
    A, B = families.special()
    with np.errstate(divide="raise"):
        vals = [iou(x, y) for x, y in zip(A, B)] + [ov(x, y) for x, y in zip(A, B)]
    assert np.isfinite(vals).all()


def test_float64_clipper_equals_the_old_one_on_random_pairs_and_iou_is_its_quotient():
    r = families.reference("random")
    old = np.array([_clip_by_direction_cross(a, b) for a, b in zip(r["A"], r["B"])])
    assert np.max(np.abs(old - r["ov64"])) <= 1e-12 and (old > 0).sum() > 500
    for name in ("random", "near_dup[1e-07]", "slide"):
        r = families.reference(name)
        got = np.array([oracle.rotated_iou_float64(a, b) for a, b in zip(r["A"][:64], r["B"][:64])])
        assert np.array_equal(got, r["iou64"][:64])


@pytest.mark.parametrize("n", sorted(families.CLUSTER_SEEDS))
def test_cluster_generator_keeps_clear_of_the_nms_thresholds(n):
    """Precondition of the GPU NMS tests, stated where the seed is chosen: every copy of an object overlaps every other by more
    than 0.2 (so the one-per-object truth needs no oracle), objects do not overlap, and no intra-cluster oracle IoU is within
    1e-3 of a threshold (so a device rounding cannot flip a decision)."""
    boxes, scores, obj = families.clusters(n)
    assert boxes.shape == (n, 5) and len(np.unique(scores)) == n and np.abs(boxes[:, 4]).max() <= np.float32(np.pi)
    sizes = np.bincount(obj)
    assert sizes.min() >= 1 and sizes.max() <= 12 and len(sizes) > n // 12
    intra = families.intra_cluster_ious(boxes, obj)
    for thr in families.NMS_THRESHOLDS:
        assert np.abs(intra - thr).min() > 1e-3
    assert intra.min() > 0.2 + 1e-3
    full = oracle.iou3d_pairwise(boxes, boxes, "iou")
    assert not full[obj[:, None] != obj[None, :]].any()
    same = (boxes[:, None, :] == boxes[None, :, :]).all(2) & ~np.eye(n, dtype=bool)
    assert same.any(1).sum() >= n // 12                                     # bit-exact duplicates are there
    order = np.argsort(-scores, kind="stable")
    assert np.array_equal(order[oracle.iou3d_nms(boxes[order], 0.2)], families.top_of_each_object(scores, obj))


@pytest.mark.parametrize("seed", families.SEGMENT_SEEDS)
def test_segment_clusters_keep_clear_of_the_nms_threshold(seed):
    """The same precondition for the CenterHead segments: 130 rows as LiDAR boxes, whose BEV rectangle is rounded once more."""
    boxes, scores, obj = families.clusters(130, seed=seed)
    bev = families.lidar_bev(families.lift(boxes))
    assert families.intra_cluster_ious(bev, obj).min() > 0.2 + 1e-3
    assert not oracle.iou3d_pairwise(bev, bev, "iou")[obj[:, None] != obj[None, :]].any()


def test_sweep_fixture_spans_more_than_256_column_blocks():
    boxes = families.axis_aligned_clusters(families.SWEEP_N)
    assert (families.SWEEP_N + 63) // 64 > 256 and (boxes[:, 4] == 0).all()
    kept = oracle.iou3d_nms(boxes, 0.3, normal=True)
    assert 1000 < len(kept) <= 1640
    # thread t of the sweep serves column blocks rb + 1 + t + 256 m of row block rb: a word is reached on the second trip (m = 1)
    # when its column block is at least 257 past the kept row's block
    late = np.arange(257 * 64, families.SWEEP_N)
    hits = oracle.iou3d_pairwise(boxes[late], boxes[kept], "iou_normal") > 0.3      # [late row, kept row]
    hits &= kept[None, :] < late[:, None]
    is_kept = np.isin(late, kept)
    assert not hits[is_kept].any() and hits[~is_kept].any(1).all()
    second_trip = (late[:, None] // 64 - kept[None, :] // 64) >= 257
    only_second = ~is_kept & ~(hits & ~second_trip).any(1)                  # suppressed by nothing the first trip reaches
    assert only_second.sum() >= 30
    for block in (257, 258, 259):                                           # from row blocks 0, 1 and 2
        rows = only_second & (late // 64 == block)
        assert rows.any() and (kept[hits[rows].any(0)] // 64).max() == block - 257
    assert is_kept.sum() >= 10                                              # late rows with no such overlap are kept
