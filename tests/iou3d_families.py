"""Box families for the rotated IoU / NMS tests: the inputs NMS and the IoU match cost exist for (several detections of one
object, equal yaw, the same rectangle written twice, small boxes far from the origin), which decide the branches of the
polygon-of-crossings algorithm (strict straddle test on collinear edges, the second intersection formula, MARGIN containment of
coincident corners, equal atan2 keys, a polygon of 8 coincident vertices).

A family is a seeded pair (A, B) of float32 [P, 5] arrays (x1, y1, x2, y2, yaw); pair p is (A[p], B[p]).  Unless a family says
otherwise the centre is uniform in +-54 m, both sizes in 0.4 .. 6 m and the yaw in +-pi.  `reference(name)` holds, per family
and computed once per process, the float64 values (oracle.rotated_overlap_float64), the fp32 oracle's values and the
well-conditioned mask: a pair is ill-conditioned when the fp32 oracle's own IoU is more than 1e-4 away from float64 (the
reference's algorithm loses the polygon there), and only there is a device result left unjudged.

`clusters(n, seed)` is the detector-like NMS input: objects on a 12 m grid, each with 1 .. 12 jittered copies."""
import functools

import numpy as np

import oracle

P = 1024
SIGMAS = (1e-7, 1e-6, 1e-5, 1e-4, 1e-2)
FAMILIES = ("random", "duplicate") + tuple(f"near_dup[{s:g}]" for s in SIGMAS) + (
    "same_yaw", "slide", "swapped", "flipped", "concentric", "right_angles", "small_far")
ILL_BAR = 1e-4          # the pairwise bar of test_gpu_iou3d.py, applied to the oracle itself
MAX_ILL_SHARE = 0.002   # cap on a family's ill-conditioned share: four times the largest share measured (0.05 %)

# one seed per family, fixed here so that CPU and GPU tests see the same boxes (tests/test_oracle_iou3d.py asserts the cap)
SEEDS = {name: 100 + i for i, name in enumerate(FAMILIES)}


def xyxyr(c, wh, yaw):
    c, wh = np.asarray(c, np.float64), np.asarray(wh, np.float64)
    return np.concatenate([c - wh / 2, c + wh / 2, np.asarray(yaw, np.float64).reshape(-1, 1)], 1).astype(np.float32)


def _base(rng, n):
    return rng.uniform(-54, 54, (n, 2)), rng.uniform(0.4, 6.0, (n, 2)), rng.uniform(-np.pi, np.pi, n)


def family(name, n=P, seed=None):
    """(A, B) of family `name`."""
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    c, wh, yaw = _base(rng, n)
    A = xyxyr(c, wh, yaw)
    if name == "random":
        B = xyxyr(c + rng.uniform(-3, 3, (n, 2)), rng.uniform(0.4, 6.0, (n, 2)), rng.uniform(-np.pi, np.pi, n))
    elif name == "duplicate":
        B = A.copy()
    elif name.startswith("near_dup["):
        s = float(name[9:-1])
        B = xyxyr(c + rng.normal(0, s, (n, 2)), wh * (1 + rng.normal(0, s, (n, 2))), yaw + rng.normal(0, s, n))
    elif name == "same_yaw":
        B = xyxyr(c + rng.uniform(-1, 1, (n, 2)), rng.uniform(0.4, 6.0, (n, 2)), yaw)
    elif name == "slide":      # (cos yaw, -sin yaw) is the image of the box's own x axis under rotate_around_center
        d = rng.uniform(-1, 1, n)
        B = xyxyr(c + d[:, None] * np.stack([np.cos(yaw), -np.sin(yaw)], 1), wh, yaw)
    elif name == "swapped":
        B = xyxyr(c, wh[:, ::-1], yaw + np.pi / 2)
    elif name == "flipped":
        B = xyxyr(c, wh, yaw + np.pi)
    elif name == "concentric":  # first half: one factor (one box inside the other); second half: a factor per axis (a cross)
        f = rng.uniform(0.5, 1.5, (n, 2))
        f[: n // 2, 1] = f[: n // 2, 0]
        B = xyxyr(c, wh * f, yaw)
    elif name == "right_angles":
        A, B = _right_angles(rng, c, wh, n)
    elif name == "small_far":
        r, phi = rng.uniform(45, 54, n), rng.uniform(-np.pi, np.pi, n)
        c, wh = np.stack([r * np.cos(phi), r * np.sin(phi)], 1), rng.uniform(0.4, 0.8, (n, 2))
        A = xyxyr(c, wh, yaw)
        B = xyxyr(c + rng.uniform(-0.03, 0.03, (n, 2)) * wh, wh, yaw + rng.uniform(-0.05, 0.05, n))
    else:
        raise KeyError(name)
    return A, B


def _right_angles(rng, c, wh, n):
    """A has yaw 0, B yaw k pi / 2.  Rows 0 mod 4: B's footprint shares A's right edge; rows 1 mod 4: it touches A's upper right
    corner; the rest overlap A freely.  For even k the stored B.x1 (and B.y1 at a corner) IS A.x2 (A.y2) bit for bit; for odd k
    the stored sizes are the footprint's exchanged, about the footprint's centre."""
    k = rng.integers(-2, 3, n)
    A = xyxyr(c, wh, np.zeros(n))
    foot = rng.uniform(0.4, 6.0, (n, 2))                       # B's footprint (extent along x, y)
    lo = A[:, :2].astype(np.float64) + rng.uniform(-3, 3, (n, 2))
    kind = np.arange(n) % 4
    lo[kind == 0, 0] = A[kind == 0, 2]
    lo[kind == 0, 1] = A[kind == 0, 1] + rng.uniform(-1, 1, int((kind == 0).sum())) * wh[kind == 0, 1] * 0.5
    lo[kind == 1] = A[kind == 1, 2:4]
    B = np.empty((n, 5), np.float32)
    B[:, :2], B[:, 2:4] = lo, (lo.astype(np.float32) + foot.astype(np.float32))
    odd = k % 2 != 0
    B[odd, :4] = xyxyr(lo + foot / 2, foot[:, ::-1], np.zeros(n))[odd, :4]
    B[:, 4] = (k * (np.pi / 2)).astype(np.float32)
    return A, B


def special():
    """16 hand-written pairs: a zero-area box, a negative extent, a NaN yaw, an inf coordinate and yaw = 1e4 rad, each against a
    normal box (both ways round) and against itself, and a box that is one point against itself."""
    normal = [0.0, 0.0, 4.0, 2.0, 0.3]
    odd = [[1.0, -1.0, 1.0, 3.0, 0.2],                          # zero area: x1 == x2
           [3.0, 0.5, 1.0, 1.5, -0.4],                          # negative extent: x2 < x1
           [0.5, 0.5, 3.0, 1.5, float("nan")],                  # NaN yaw
           [1.0, 0.0, float("inf"), 2.0, 0.1],                  # inf coordinate
           [0.5, -0.5, 3.5, 1.5, 1e4]]                          # yaw far outside +-pi
    a, b = [], []
    for o in odd:
        a += [o, normal, o]
        b += [normal, o, o]
    a.append([2.0, 1.0, 2.0, 1.0, 0.7])
    b.append([2.0, 1.0, 2.0, 1.0, 0.7])
    return np.array(a, np.float32), np.array(b, np.float32)


def lift(boxes, z=-1.0, height=1.5):
    """xyxyr [P, 5] -> LiDAR boxes [P, 7] (x, y, z bottom, dx, dy, dz, yaw), fp32."""
    b = np.asarray(boxes, np.float32)
    out = np.empty((b.shape[0], 7), np.float32)
    out[:, 0], out[:, 1] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    out[:, 2], out[:, 5] = z, height
    out[:, 3], out[:, 4], out[:, 6] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], b[:, 4]
    return out


def lidar_bev(b7):
    """What the kernels make of a LiDAR box, in fp32: (x - dx / 2, y - dy / 2, x + dx / 2, y + dy / 2, yaw)."""
    b7 = np.asarray(b7, np.float32)
    hx, hy = b7[:, 3] / np.float32(2), b7[:, 4] / np.float32(2)
    return np.stack([b7[:, 0] - hx, b7[:, 1] - hy, b7[:, 0] + hx, b7[:, 1] + hy, b7[:, 6]], 1)


def oracle_diag(A, B, mode):
    """The fp32 oracle on pair p = (A[p], B[p]) only."""
    return np.array([oracle.iou3d_pairwise(a[None], b[None], mode)[0, 0] for a, b in zip(A, B)], np.float32)


def areas64(boxes):
    b = np.asarray(boxes, np.float32).astype(np.float64)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def bar(oracle_err):
    """What a device result may be off float64 on a well-conditioned pair: 4 x the oracle's own maximum error on the family (the
    margin the head tests give the device over the reference CPU result; it pays for the device's sinf / cosf / atan2f), at
    least 1e-6, never more than 1e-4."""
    return min(max(4 * oracle_err, 1e-6), ILL_BAR)


def judge(A, B):
    """The float64 values, the fp32 oracle's and what follows from them for pairs (A[p], B[p])."""
    ov64 = np.array([oracle.rotated_overlap_float64(a, b) for a, b in zip(A, B)], np.float64)
    union = np.maximum(areas64(A) + areas64(B) - ov64, 1e-8)
    iou64 = ov64 / union                                                     # == oracle.rotated_iou_float64, pair by pair
    ov32, iou32 = oracle_diag(A, B, "overlap"), oracle_diag(A, B, "iou")
    with np.errstate(invalid="ignore"):
        well = np.abs(iou32.astype(np.float64) - iou64) <= ILL_BAR           # NaN or huge: ill-conditioned
    err_iou = float(np.max(np.abs(iou32[well] - iou64[well]))) if well.any() else 0.0
    err_ov = float(np.max(np.abs(ov32[well] - ov64[well]) / union[well])) if well.any() else 0.0
    return dict(A=A, B=B, ov64=ov64, iou64=iou64, ov32=ov32, iou32=iou32, union=union, well=well,
                oracle_err_iou=err_iou, oracle_err_ov=err_ov, bar_iou=bar(err_iou), bar_ov=bar(err_ov))


@functools.lru_cache(maxsize=None)
def reference(name):
    """judge() of a family, once per process; callers do not modify it."""
    return judge(*family(name))


@functools.lru_cache(maxsize=None)
def reference_lifted(name):
    """The same for the family lifted to LiDAR boxes, as BboxOverlaps3D sees it: the BEV rectangle is what fp32 makes of
    (x -+ dx / 2, y -+ dy / 2), the 3D IoU is o h / (va + vb - o h) with h the common height.  Values are 3D IoUs."""
    A, B = family(name)
    a7, b7 = lift(A), lift(B)
    r = judge(lidar_bev(a7), lidar_bev(b7))
    a64, b64 = a7.astype(np.float64), b7.astype(np.float64)
    h = np.maximum(np.minimum(a64[:, 2] + a64[:, 5], b64[:, 2] + b64[:, 5]) - np.maximum(a64[:, 2], b64[:, 2]), 0.0)
    va, vb = a64[:, 3] * a64[:, 4] * a64[:, 5], b64[:, 3] * b64[:, 4] * b64[:, 5]

    def iou3d(ov):
        o = ov.astype(np.float64) * h
        return o / np.maximum(va + vb - o, 1e-8)

    iou64, iou32 = iou3d(r["ov64"]), iou3d(r["ov32"])
    with np.errstate(invalid="ignore"):
        well = np.abs(iou32 - iou64) <= ILL_BAR
    err = float(np.max(np.abs(iou32[well] - iou64[well]))) if well.any() else 0.0
    return dict(a7=a7, b7=b7, iou64=iou64, iou32=iou32, well=well, oracle_err_iou=err, bar_iou=bar(err))


# ---- detector-like duplicates for NMS ------------------------------------------------------------------------------------------
CLUSTER_SEEDS = {130: 7, 1000: 8}     # tests/test_oracle_iou3d.py asserts that no intra-cluster IoU is within 1e-3 of 0.2 / 0.7
NMS_THRESHOLDS = (0.2, 0.7)
SEGMENT_SEEDS = (20, 21, 22)          # the three 130-row segments of the CenterHead NMS test, as lifted LiDAR boxes
SWEEP_N = 16600                       # 260 column blocks: the sweep kernel's `j += 256` loop takes a second trip


def clusters(n, seed=None, grid=12.0):
    """n boxes in clusters: object k sits on a `grid`-metre lattice (sizes <= 6 m: no two objects touch) and has m_k in 1 .. 12
    copies with the centre jittered by +-0.03 min(w, h), both sizes by +-3 % and the yaw by +-0.03 rad (uniform, so that every
    copy overlaps every other copy of its object by far more than 0.2).  Of the copies a sixth are bit-exact duplicates of
    another copy of the object, a sixth carry yaw + pi and a sixth are written as (l, w, yaw + pi / 2).
    Returns (boxes [n, 5] xyxyr fp32, scores [n] fp32 distinct, obj [n] int64)."""
    rng = np.random.default_rng(CLUSTER_SEEDS[n] if seed is None else seed)
    counts = []
    while sum(counts) < n:
        counts.append(int(rng.integers(1, 13)))
    counts[-1] -= sum(counts) - n
    K = len(counts)
    side = int(np.ceil(np.sqrt(K)))
    cells = rng.permutation(side * side)[:K]
    centre = (np.stack([cells % side, cells // side], 1) - (side - 1) / 2) * grid
    wh0, yaw0 = rng.uniform(0.4, 6.0, (K, 2)), rng.uniform(-np.pi, np.pi, K)
    obj = np.repeat(np.arange(K), counts)
    small = wh0.min(1)[obj]
    c = centre[obj] + rng.uniform(-0.03, 0.03, (n, 2)) * small[:, None]
    wh = wh0[obj] * (1 + rng.uniform(-0.03, 0.03, (n, 2)))
    yaw = yaw0[obj] + rng.uniform(-0.03, 0.03, n)
    form = rng.integers(0, 6, n)                                 # 0: duplicate, 1: yaw + pi, 2: (l, w, yaw + pi / 2), else plain
    yaw = np.where(form == 1, yaw + np.pi, yaw)
    yaw = np.where(form == 2, yaw + np.pi / 2, yaw)
    wh = np.where((form == 2)[:, None], wh[:, ::-1], wh)
    yaw = (yaw + np.pi) % (2 * np.pi) - np.pi                     # a real yaw in [-pi, pi)
    boxes = xyxyr(c, wh, yaw)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    for i in np.nonzero(form == 0)[0]:                           # a copy of another row of the same object, bit for bit
        k = obj[i]
        others = [j for j in range(first[k], first[k] + counts[k]) if form[j] != 0]
        if others:
            boxes[i] = boxes[others[int(rng.integers(len(others)))]]
    scores = ((rng.permutation(n) + 1) / np.float32(n + 1)).astype(np.float32)
    return boxes, scores, obj


def top_of_each_object(scores, obj):
    """The one-per-object truth: the best-scoring copy of every object, in descending score."""
    seen, keep = set(), []
    for i in np.argsort(-scores, kind="stable"):
        if obj[i] not in seen:
            seen.add(obj[i])
            keep.append(i)
    return np.array(keep, np.int64)


def intra_cluster_ious(boxes, obj):
    """fp32 oracle IoU of every ordered pair of distinct rows of one object."""
    out = [np.zeros(0, np.float32)]
    for k in np.unique(obj):
        rows = np.nonzero(obj == k)[0]
        if len(rows) > 1:
            m = oracle.iou3d_pairwise(boxes[rows], boxes[rows], "iou")
            out.append(m[~np.eye(len(rows), dtype=bool)])
    return np.concatenate(out)


def axis_aligned_clusters(n, seed=5):
    """n axis-aligned boxes (yaw 0) of 3.8 .. 4 m about anchors 10 m apart, jittered by +-0.2 m: IoU >= 0.6 inside a cluster and 0
    between clusters; the first row of an anchor is the one NMS keeps and the only one that suppresses the others.
    The last 200 rows are built for the sweep kernel, whose thread t serves the column blocks rb + 1 + t, rb + 257 + t, ...
    of row block rb: half of them sit about 40 anchors of their own (rows are kept up to the end of the list), the other half
    about anchors whose first row lies in block 0 or, for a row of column block j >= 257, in block j - 257: such a row is
    suppressed only by a kept row at least 257 blocks before it, that is only on the loop's second trip."""
    rng = np.random.default_rng(seed)
    side = 40
    a = rng.integers(0, side * side, n)
    anchors, first = np.unique(a[: n - 200], return_index=True)
    for i in range(n - 200, n):
        if i % 2 == 0:
            a[i] = side * side + rng.integers(0, side)
        else:
            block = max(i // 64 - 257, 0) if i % 4 == 3 else 0
            a[i] = rng.choice(anchors[first // 64 == block])
    c = np.stack([a % side, a // side], 1) * 10.0 + rng.uniform(-0.2, 0.2, (n, 2))
    return xyxyr(c, rng.uniform(3.8, 4.0, (n, 2)), np.zeros(n))
