"""Writes tests/golden/centerhead_ref.npz: recorded outputs of the REFERENCE's CenterHead end on seeded inputs.

The reference's `centerpoint_bbox_coders.py` and `box3d_nms.py` are exec'd unmodified from where they lie, under inert
`sys.modules` stubs (mmdet, mmdet3d.ops, numba with `jit` as the identity), on CPU torch with one thread.  `get_bboxes` and
`get_task_detections` are methods of a class that cannot be constructed here: their statements (centerpoint.py:637-757 and
:759-884, without the fp16 decorator) and `xywhr2xyxyr` (core/bbox/structures/utils.py:71-89) are read from the files at run time,
dedented, exec'd, and bound to a namespace object carrying the attributes they read.  `metas[i]["box_type_3d"]` is a minimal class
whose `.bev` is columns [0, 1, 3, 4, 6] (the LiDAR convention).  `nms_gpu` is iou3d_utils.py:23-48 with the `iou3d_cuda.nms_gpu`
call backed by `oracle.iou3d_nms`, which tests/test_oracle_iou3d.py pins to the reference's GPU op.  Nothing of the reference's
text is stored: only the seeded inputs' digests and recorded results (fp32 outputs of every selected row, a float64 recomputation
of them for the error bars, the kept rows and counts).  Inputs are NOT stored: `inputs()` regenerates them (the tests import this
file for it and check the stored SHA-256); it needs numpy and the pure-Python `oracle.rotated_overlap_float64` only.

Every case is built so that the reference's own answer is well defined.  `inputs()` keeps, by redrawing the regression values of
one offending row at a time (bounded, asserted), and `main()` asserts again on the reference's own outputs:
  * logits of a (sample, task) are distinct multiples of 2^-10 and the K + 8 best lie in distinct cells; consecutive scores among
    the first K + 1 are at least 4 ulp apart; scores are 1e-3 away from the coder's and the head's thresholds;
  * centres and heights are 1e-2 m away from the limits of both ranges;
  * every pair of live boxes of a rotate segment has a float64 IoU at least IOU_MARGIN away from nms_thr, and `main()` asserts that
    this is at least 10 x the largest fp32-vs-float64 IoU difference seen on the case and at least 1e-3; no pair is exempted;
  * every pair of live rows of a circle segment has a squared distance 1e-3 away from the radius;
  * box angles are at least 0.1 rad away from the axes (the float64 check holds away from degenerate contacts).

    python tests/golden/make_centerhead_golden.py
"""
import functools
import hashlib
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "centerhead_ref.npz")
REF = "/root/reference/mmdet3d"

CLASSES = (1, 2, 2)
B, T = 2, 3
CODER = dict(pc_range=[-51.2, -51.2], out_size_factor=8, voxel_size=[0.4, 0.4], post_center_range=[-45.0, -45.0, -3.0, 45.0, 45.0, 3.0],
             score_threshold=0.1, code_size=9)
WIDE = [-100.0, -100.0, -10.0, 100.0, 100.0, 10.0]
TEST_CFG = dict(min_radius=[4, 12, 10], post_max_size=83, pre_max_size=1000, nms_thr=0.2, score_threshold=0.2,
                post_center_limit_range=[-40.5, -40.5, -2.5, 40.5, 40.5, 2.5])
IOU_MARGIN = 5e-3
MAX_REDRAWS = 400
NESTED = [[1.0], [1.0, 1.4], [1.0, 1.0]]

# live: per (sample, task) the number of rows above the head's threshold and between the two thresholds (None: 5/8 and 1/8 of K)
# the coder's decode on its own, without `reg` (the head always passes one): task and inputs of a case above
DECODE_NOREG = dict(case="rot_16_k32", task=1)
CASES = {
    "rot_16_k32": dict(H=16, W=16, K=32, vel=True, reg=True, norm=True, nms="rotate", seed=701),
    "rot_rect_k130_nested": dict(H=12, W=20, K=130, vel=True, reg=True, norm=True, nms="rotate", scale=NESTED, seed=702),
    "circle_16_k32_novel": dict(H=16, W=16, K=32, vel=False, reg=True, norm=True, nms="circle", seed=703),
    "mixed_rect_k32_nonorm_scalar": dict(H=12, W=20, K=32, vel=True, reg=True, norm=False, nms=["rotate", "circle", "rotate"],
                                         scale=1.2, seed=704),
    "sizes_16_k130": dict(H=16, W=16, K=130, vel=True, reg=True, norm=True, nms="rotate", wide=True, seed=705,
                          live=[[(130, 0), (65, 0), (2, 0)], [(1, 0), (0, 0), (130, 0)]]),
    "premax_16_k32": dict(H=16, W=16, K=32, vel=True, reg=True, norm=True, nms="rotate", cfg=dict(pre_max_size=10), seed=706),
    "postmax_16_k130": dict(H=16, W=16, K=130, vel=False, reg=True, norm=True, nms=["rotate", "circle", "rotate"], wide=True,
                            cfg=dict(post_max_size=5), seed=707),
}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def nms_types(case):
    n = CASES[case]["nms"]
    return list(n) if isinstance(n, list) else [n] * T


def coder_args(case):
    c = CASES[case]
    return dict(CODER, max_num=c["K"], post_center_range=WIDE if c.get("wide") else CODER["post_center_range"])


def test_cfg(case):
    c = CASES[case]
    cfg = dict(TEST_CFG, nms_type=c["nms"], **c.get("cfg", {}))
    if c.get("wide"):
        cfg["post_center_limit_range"] = WIDE
    if "scale" in c:
        cfg["nms_scale"] = c["scale"]
    return cfg


def scales(case):
    s = CASES[case].get("scale", 1.0)
    return s if isinstance(s, list) else [[s] * n for n in CLASSES]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
_BANDS = ((-1.3, 4.0), (-2.1, -1.5), (-7.0, -2.4), (-12.0, -7.5))   # above the head's 0.2; between; below the coder's 0.1; the rest


def _band(rng, band, n):
    lo, hi = int(np.ceil(band[0] * 1024)), int(np.floor(band[1] * 1024))
    return (rng.choice(hi - lo + 1, size=n, replace=False) + lo) / 1024.0


def _draw_cell(c, rng):
    ang = rng.uniform(0.1, np.pi / 2 - 0.1) + rng.integers(0, 4) * np.pi / 2
    mag = rng.uniform(0.5, 1.5)
    size = np.array([rng.uniform(np.log(1.5), np.log(6.0)), rng.uniform(np.log(1.5), np.log(6.0)), rng.uniform(0.0, np.log(3.0))])
    return dict(reg=rng.uniform(0.02, 0.98, 2), height=rng.uniform(-4, 4, 1) if not c.get("wide") else rng.uniform(-2, 2, 1),
                dim=size if c["norm"] else np.exp(size), rot=np.array([np.sin(ang), np.cos(ang)]) * mag, vel=rng.uniform(-5, 5, 2))


def _decode64(case, d, b, t, rows):
    """float64 restatement for the margins: (xy [n, 2], z [n], bev xyxyr [n, 5] of the fp32 boxes' values) of the given
    (class, cell) rows."""
    c = CASES[case]
    W = c["W"]
    cell = rows[:, 1]
    f = lambda name: d[f"{name}{t}"][b].reshape(d[f"{name}{t}"].shape[1], -1)[:, cell].astype(np.float64)   # noqa: E731
    off = f("reg") if c["reg"] else np.full((2, len(cell)), 0.5)
    x = ((cell // W) + off[0]) * 8 * 0.4 - 51.2
    y = ((cell % W) + off[1]) * 8 * 0.4 - 51.2
    dim = np.exp(f("dim")) if c["norm"] else f("dim")
    rot = f("rot")
    yaw = np.arctan2(rot[0], rot[1])
    sc = np.array([scales(case)[t][k] for k in rows[:, 0]])
    w, l = dim[0] * sc, dim[1] * sc
    return np.stack([x, y], 1), f("height")[0], np.stack([x - w / 2, y - l / 2, x + w / 2, y + l / 2, yaw], 1)


def iou64(a, b):
    from oracle import rotated_overlap_float64

    if np.hypot((a[0] + a[2] - b[0] - b[2]) / 2, (a[1] + a[3] - b[1] - b[3]) / 2) >= 0.5 * (np.hypot(a[2] - a[0], a[3] - a[1]) + np.hypot(b[2] - b[0], b[3] - b[1])):
        return 0.0
    ov = rotated_overlap_float64(a, b)
    return ov / max((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - ov, 1e-8)


def _offender(case, d, b, t, rows, n_live_hi, n_live_mid, cache):
    """Index into `rows` of one row that breaks a margin, or None.  rows: the K best (class, cell) in descending score."""
    c = CASES[case]
    cfg, rot = test_cfg(case), nms_types(case)[t] == "rotate"
    xy, z, bev = _decode64(case, d, b, t, rows)
    ranges = [coder_args(case)["post_center_range"]] + ([cfg["post_center_limit_range"]] if rot else [])
    p = np.concatenate([xy, z[:, None]], 1)
    inside = np.ones(len(rows), bool)
    for r in ranges:
        near = (np.abs(p - np.array(r[:3])) < 1e-2) | (np.abs(p - np.array(r[3:])) < 1e-2)
        if near.any():
            return int(np.nonzero(near.any(1))[0][0])
    r = ranges[0]
    inside = ((p >= np.array(r[:3])) & (p <= np.array(r[3:]))).all(1)
    n_score = n_live_hi if rot else n_live_hi + n_live_mid
    live = np.nonzero(inside & (np.arange(len(rows)) < n_score))[0]
    if rot:
        for jj, j in enumerate(live):
            for i in live[:jj]:
                key = (bev[i].tobytes(), bev[j].tobytes())
                if key not in cache:
                    cache[key] = iou64(bev[i].astype(np.float32), bev[j].astype(np.float32))
                if abs(cache[key] - cfg["nms_thr"]) < IOU_MARGIN:
                    return int(j)
    else:
        q = xy[live]
        d2 = ((q[:, None, :] - q[None, :, :]) ** 2).sum(-1)
        bad = np.abs(d2 - cfg["min_radius"][t]) < 1e-3
        bad[np.tril_indices(len(live))] = False
        if bad.any():
            return int(live[np.nonzero(bad.any(0))[0][0]])
    return None


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict of fp32 arrays: heatmap{t} [B, Ct, H, W] logits, reg{t}, height{t}, dim{t}, rot{t}, vel{t} for t in 0 .. T - 1 (reg / vel
    are drawn for every case; the case's flags say whether the head has them)."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    H, W, K = c["H"], c["W"], c["K"]
    hw = H * W
    d, tops, lives = {}, {}, {}
    for t, ct in enumerate(CLASSES):
        heat = np.zeros((B, ct * hw))
        for b in range(B):
            n_hi, n_mid = c["live"][b][t] if "live" in c else (K * 5 // 8, K // 8)
            n_top = K + 8
            cells = rng.choice(hw, size=n_top, replace=False)
            slots = rng.integers(0, ct, n_top) * hw + cells
            vals = np.concatenate([_band(rng, _BANDS[0], n_hi), _band(rng, _BANDS[1], n_mid), _band(rng, _BANDS[2], n_top - n_hi - n_mid)])
            rest = np.setdiff1d(np.arange(ct * hw), slots)
            heat[b, rest] = _band(rng, _BANDS[3], len(rest))
            heat[b, slots] = vals
            order = np.argsort(-heat[b], kind="stable")[:K]
            tops[b, t] = np.stack([order // hw, order % hw], 1)
            lives[b, t] = (min(n_hi, K), min(n_mid, K - min(n_hi, K)))
        d[f"heatmap{t}"] = heat.reshape(B, ct, H, W)
        for name, ch in (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2)):
            d[f"{name}{t}"] = np.zeros((B, ch, hw))
        for b in range(B):
            for cell in range(hw):
                for name, v in _draw_cell(c, rng).items():
                    d[f"{name}{t}"][b, :, cell] = v
    d = {k: v.astype(np.float32) for k, v in d.items()}
    redraws, cache = 0, {}
    for t in range(T):
        for b in range(B):
            while True:
                view = {k: v.reshape(B, v.shape[1], H, W) if v.ndim == 3 else v for k, v in d.items()}
                bad = _offender(case, view, b, t, tops[b, t], *lives[b, t], cache)
                if bad is None:
                    break
                redraws += 1
                assert redraws <= MAX_REDRAWS, f"{case}: more than {MAX_REDRAWS} redraws"
                for name, v in _draw_cell(c, rng).items():
                    d[f"{name}{t}"][b, :, tops[b, t][bad, 1]] = v.astype(np.float32)
    out = {k: np.ascontiguousarray(v.reshape(B, v.shape[1], H, W)) for k, v in d.items()}
    out["_redraws"] = redraws
    return out


def arrays(case):
    d = inputs(case)
    return [d[k] for k in sorted(d) if not k.startswith("_")]


def preds(case, d=None):
    """The head's output for the case as numpy arrays: one [dict] per task."""
    c = CASES[case]
    d = inputs(case) if d is None else d
    names = ["heatmap", "height", "dim", "rot"] + (["reg"] if c["reg"] else []) + (["vel"] if c["vel"] else [])
    return [[{n: d[f"{n}{t}"] for n in names}] for t in range(T)]


# ---- the reference, exec'd under stubs -------------------------------------------------------------------------------------
def load_reference():
    import torch

    import oracle

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    class _Coders:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def jit(*a, **k):
        if a and callable(a[0]):
            return a[0]
        return lambda f: f

    stubs = {
        "mmdet": mod("mmdet"), "mmdet.core": mod("mmdet.core"),
        "mmdet.core.bbox": mod("mmdet.core.bbox", BaseBBoxCoder=object),
        "mmdet.core.bbox.builder": mod("mmdet.core.bbox.builder", BBOX_CODERS=_Coders()),
        "numba": mod("numba", jit=jit),
        "mmdet3d": mod("mmdet3d"), "mmdet3d.ops": mod("mmdet3d.ops"), "mmdet3d.ops.iou3d": mod("mmdet3d.ops.iou3d"),
        "mmdet3d.ops.iou3d.iou3d_utils": mod("mmdet3d.ops.iou3d.iou3d_utils", nms_gpu=None, nms_normal_gpu=None),
    }
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        mods = {}
        for key, rel in (("coder", "core/bbox/coders/centerpoint_bbox_coders.py"), ("nms", "core/post_processing/box3d_nms.py")):
            path = os.path.join(REF, rel)
            m = types.ModuleType("reference_" + key)
            exec(compile(open(path).read(), path, "exec"), m.__dict__)
            mods[key] = m
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    torch.set_num_threads(1)

    def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
        """iou3d_utils.py:23-48 with iou3d_cuda.nms_gpu backed by the oracle."""
        order = scores.sort(0, descending=True)[1]
        if pre_maxsize is not None:
            order = order[:pre_maxsize]
        keep = order[torch.from_numpy(oracle.iou3d_nms(boxes[order].contiguous().numpy(), thresh))].contiguous()
        if post_max_size is not None:
            keep = keep[:post_max_size]
        return keep

    def block(rel, first, last, sentinel):
        path = os.path.join(REF, rel)
        src = textwrap.dedent("\n".join(open(path).read().split("\n")[first - 1:last]))
        assert src.split("\n")[0].startswith(sentinel), (first, src.split("\n")[0])
        return compile("\n" * (first - 1) + src, path, "exec")

    ns = dict(torch=torch, circle_nms=mods["nms"].circle_nms, nms_gpu=nms_gpu)
    exec(block("core/bbox/structures/utils.py", 71, 89, "def xywhr2xyxyr("), ns)
    exec(block("models/heads/bbox/centerpoint.py", 637, 757, "def get_bboxes("), ns)
    exec(block("models/heads/bbox/centerpoint.py", 759, 884, "def get_task_detections("), ns)
    head = type("Head", (), dict(get_bboxes=ns["get_bboxes"], get_task_detections=ns["get_task_detections"]))
    return mods["coder"], head


class Boxes:
    """The minimum of LiDARInstance3DBoxes that get_bboxes / get_task_detections read."""

    def __init__(self, tensor, box_dim=7):
        self.tensor = tensor

    @property
    def bev(self):
        return self.tensor[:, [0, 1, 3, 4, 6]]


def _rows_of(sub, full):
    rows, j = [], 0
    for r in sub:
        while not np.array_equal(full[j].view(np.int32), r.view(np.int32)):
            j += 1
        rows.append(j)
        j += 1
    return np.asarray(rows, np.int16)


def record(case, ref_coder, head_cls, out):
    import torch

    import oracle

    c = CASES[case]
    d = inputs(case)
    K, cfg = c["K"], test_cfg(case)

    def tensors(dtype):
        return [[{k: torch.from_numpy(v).to(dtype) for k, v in p[0].items()}] for p in preds(case)]

    def full(dtype):
        """Every selected row, no filter: (boxes [B, T * K, w] with the merge's z shift, scores, labels with the merge's offset)."""
        coder = ref_coder.CenterPointBBoxCoder(**dict(coder_args(case), post_center_range=[-1e9] * 3 + [1e9] * 3, score_threshold=None))
        parts, base = [], 0
        for t, p in enumerate(tensors(dtype)):
            p = p[0]
            dim = torch.exp(p["dim"]) if c["norm"] else p["dim"]
            res = coder.decode(p["heatmap"].sigmoid(), p["rot"][:, 0].unsqueeze(1), p["rot"][:, 1].unsqueeze(1), p["height"], dim, p.get("vel"),
                               reg=p.get("reg"), task_id=t)
            assert all(len(r["scores"]) == K for r in res)
            boxes = torch.stack([r["bboxes"] for r in res])
            boxes[..., 2] = boxes[..., 2] - boxes[..., 5] * 0.5
            parts.append((boxes, torch.stack([r["scores"] for r in res]), torch.stack([r["labels"] for r in res]) + base))
            base += CLASSES[t]
        return [torch.cat([q[i] for q in parts], 1).numpy() for i in range(3)]

    box32, score32, label32 = full(torch.float32)
    box64, score64, label64 = full(torch.float64)
    assert np.array_equal(label32, label64) and box32.dtype == np.float32 and box64.dtype == np.float64
    for b in range(B):                                         # the first K + 1 scores of every segment: >= 4 ulp apart
        for t, ct in enumerate(CLASSES):
            s = torch.from_numpy(d[f"heatmap{t}"]).sigmoid()[b].numpy().ravel()
            top = np.sort(s)[::-1][:K + 1]
            assert ulps(top[:-1], top[1:]).min() >= 4, case
            assert np.array_equal(top[:K], score32[b, t * K:(t + 1) * K])
    thr = [CODER["score_threshold"], cfg["score_threshold"]]
    assert min(np.abs(score64 - v).min() for v in thr) >= 1e-3, case

    head = head_cls()
    head.test_cfg, head.num_classes, head.norm_bbox = cfg, list(CLASSES), c["norm"]
    head.bbox_coder = ref_coder.CenterPointBBoxCoder(**coder_args(case))
    ret = head.get_bboxes(tensors(torch.float32), [dict(box_type_3d=Boxes)] * B)
    rows = []
    key32 = np.concatenate([box32, score32[..., None]], -1)
    for i, (boxes, scores, labels) in enumerate(ret):
        assert labels.dtype == torch.int32
        r = _rows_of(np.concatenate([boxes.tensor.numpy(), scores.numpy()[:, None]], 1), key32[i])
        assert np.array_equal(labels.numpy(), label32[i][r].astype(np.int32))
        rows.append(r)

    # margins on the reference's own numbers: ranges, rotated IoU (fp32 oracle vs float64), circle distances
    worst, closest = 0.0, np.inf
    gravity = box64.copy()
    gravity[..., 2] += gravity[..., 5] * 0.5
    for t, kind in enumerate(nms_types(case)):
        sl = slice(t * K, (t + 1) * K)
        ranges = [coder_args(case)["post_center_range"]] + ([cfg["post_center_limit_range"]] if kind == "rotate" else [])
        for r in ranges:
            p = gravity[:, sl, :3]
            assert min(np.abs(p - np.array(r[:3])).min(), np.abs(p - np.array(r[3:])).min()) >= 1e-2 - 1e-6, (case, t)
        r = ranges[0]
        for b in range(B):
            p, s = gravity[b, sl, :3], score64[b, sl]
            live = ((p >= np.array(r[:3])) & (p <= np.array(r[3:]))).all(1) & (s > thr[0])
            if kind == "rotate":
                live &= s >= thr[1]
                bx = box32[b, sl][live]
                sc = np.array([scales(case)[t][int(k) - sum(CLASSES[:t])] for k in label32[b, sl][live]], np.float32)
                w, l = bx[:, 3] * sc / 2, bx[:, 4] * sc / 2
                bev = np.stack([bx[:, 0] - w, bx[:, 1] - l, bx[:, 0] + w, bx[:, 1] + l, bx[:, 6]], 1).astype(np.float32)
                assert np.abs(np.mod(bev[:, 4], np.pi / 2) - np.pi / 4).max(initial=0) <= np.pi / 4 - 0.09, case
                i32 = oracle.iou3d_pairwise(bev, bev, "iou") if len(bev) else np.zeros((0, 0), np.float32)
                for j in range(len(bev)):
                    for i in range(j):
                        v = iou64(bev[i], bev[j])
                        worst = max(worst, abs(v - float(i32[i, j])))
                        closest = min(closest, abs(v - cfg["nms_thr"]))
            else:
                q = gravity[b, sl, :2][live]
                d2 = ((q[:, None, :] - q[None, :, :]) ** 2).sum(-1)[np.triu_indices(len(q), 1)]
                assert len(d2) == 0 or np.abs(d2 - cfg["min_radius"][t]).min() >= 1e-3 - 1e-9, (case, t)
            if "live" in c:
                assert int(live.sum()) == c["live"][b][t][0], (case, b, t, int(live.sum()))
    assert closest >= max(10 * worst, 1e-3), (case, closest, worst)

    p = case + "."
    out[p + "inputs_sha256"] = np.array(sha(*arrays(case)))
    out[p + "boxes"], out[p + "scores"], out[p + "labels"] = box32, score32, label32.astype(np.int16)
    out[p + "boxes64"], out[p + "scores64"] = box64, score64
    out[p + "counts"] = np.asarray([len(r) for r in rows], np.int32)
    out[p + "rows"] = np.concatenate(rows) if rows else np.zeros(0, np.int16)
    live_total = sum(int((score64[b] >= thr[1]).sum()) for b in range(B))
    print(f"  {case}: kept {out[p + 'counts'].tolist()} of {T * K} ({live_total} above the head's threshold), {d['_redraws']} redraws, "
          f"IoU fp32-vs-float64 {worst:.2e}, closest to nms_thr {closest:.2e}")


def decode_noreg_args(d=None, as_tensor=np.asarray):
    """Arguments of CenterPointBBoxCoder.decode for DECODE_NOREG: scores, rot_sine, rot_cosine, hei, dim (sizes), vel."""
    d = inputs(DECODE_NOREG["case"]) if d is None else d
    t = DECODE_NOREG["task"]
    heat = d[f"heatmap{t}"].astype(np.float64)
    return [as_tensor(a) for a in ((1 / (1 + np.exp(-heat))).astype(np.float32), d[f"rot{t}"][:, 0:1], d[f"rot{t}"][:, 1:2], d[f"height{t}"],
                                   np.exp(d[f"dim{t}"].astype(np.float64)).astype(np.float32), d[f"vel{t}"])]


def record_decode_noreg(ref_coder, out):
    import torch

    case = DECODE_NOREG["case"]
    K = CASES[case]["K"]

    def run(dtype, **over):
        coder = ref_coder.CenterPointBBoxCoder(**dict(coder_args(case), **over))
        return coder.decode(*[torch.from_numpy(a).to(dtype) for a in decode_noreg_args()], reg=None, task_id=DECODE_NOREG["task"])

    wide = dict(post_center_range=[-1e9] * 3 + [1e9] * 3, score_threshold=None)
    full32, full64, res = run(torch.float32, **wide), run(torch.float64, **wide), run(torch.float32)
    box32 = np.stack([r["bboxes"].numpy() for r in full32])
    assert box32.shape == (B, K, 9) and np.abs(np.abs(box32[..., :2]) - 45.0).min() >= 1e-2
    p = "decode_noreg."
    out[p + "inputs_sha256"] = np.array(sha(*decode_noreg_args()))
    out[p + "boxes"], out[p + "boxes64"] = box32, np.stack([r["bboxes"].numpy() for r in full64])
    out[p + "scores"], out[p + "labels"] = np.stack([r["scores"].numpy() for r in full32]), np.stack([r["labels"].numpy() for r in full32])
    assert out[p + "labels"].dtype == np.float32
    rows = [_rows_of(r["bboxes"].numpy(), box32[i]) for i, r in enumerate(res)]
    out[p + "counts"], out[p + "rows"] = np.asarray([len(r) for r in rows], np.int32), np.concatenate(rows)
    assert all(0 < len(r) < K for r in rows)
    print(f"  decode_noreg: kept {out[p + 'counts'].tolist()} of {K}")


def main():
    ref_coder, head_cls = load_reference()
    out = {}
    for case in CASES:
        record(case, ref_coder, head_cls, out)
    record_decode_noreg(ref_coder, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
