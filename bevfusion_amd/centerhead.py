"""The non-learned end of the CenterPoint detection head (reference: mmdet3d/models/heads/bbox/centerpoint.py:637-884,
mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py), over csrc/ext/centerpoint_ends.hip.  `heads` re-exports everything here.

  * `CenterPointBBoxCoder`: the reference's coder, registered in `registry.BBOX_CODERS`;
  * `centerhead_get_bboxes`: get_bboxes / get_task_detections for all tasks and samples at once: per-task top-K, gather-decode,
    the coder's and the head's masks, circle or rotated NMS per task, the post-NMS range test and the merge.  On device tensors:
    two launches for the selection, one for the decode, one per NMS type in use, a handful of small torch ops for the merge; one
    read-back of the B counts with sync=True, none with sync=False;
  * `rotate_nms_segments`: the segmented rotated NMS on its own.

Dispatch as in `heads`: device tensors go through the library or raise; host tensors run the reference's formulation in torch /
numpy with a STABLE descending argsort (equal scores in ascending flat index c * H * W + cell; equal NMS scores: lower row first),
which is the order the kernels are defined to produce.  The host rotated IoU clips the two rectangles in float64.

Differences from the reference, on purpose: the order among equal scores is defined; `decode` does not need `heat` on the device
of a tensor it builds; an empty `post_center_limit_range` means no test (the reference compares against an empty list).
"""
import math

import numpy as np
import torch

from . import _capi
from .registry import register_everywhere

__all__ = ["CenterPointBBoxCoder", "centerhead_get_bboxes", "rotate_nms_segments"]

MAX_NUM = 1024        # HE_MAX_K of the kernels: rows per (sample, task) segment
MAX_TASKS = 16
MAX_TASK_CLASSES = 8
_MAP_CHANNELS = dict(reg=2, height=1, dim=3, rot=2, vel=2)
_CONST_CACHE = {}


# ---- selection + decode ----------------------------------------------------------------------------------------------------------
def _check_maps(heats, maps):
    """heats: per task [B, Ct, H, W]; maps: per task dict(reg | None, height, dim, rot, vel | None) -> (B, H, W, classes)."""
    if not 1 <= len(heats) <= MAX_TASKS:
        raise RuntimeError(f"{len(heats)} tasks (1 .. {MAX_TASKS})")
    if heats[0].dim() != 4:
        raise RuntimeError(f"heatmap must be [B, C, H, W], got {tuple(heats[0].shape)}")
    B, _, H, W = heats[0].shape
    dev, classes = heats[0].device, []
    has = {k: maps[0].get(k) is not None for k in ("reg", "vel")}
    for t, (heat, m) in enumerate(zip(heats, maps)):
        if heat.dim() != 4 or (heat.shape[0], heat.shape[2], heat.shape[3]) != (B, H, W) or heat.dtype != torch.float32 or heat.device != dev:
            raise RuntimeError(f"task {t}: heatmap must be float32 [{B}, C, {H}, {W}] on {dev}, got {tuple(heat.shape)} {heat.dtype} on {heat.device}")
        if not 1 <= heat.shape[1] <= MAX_TASK_CLASSES:
            raise RuntimeError(f"task {t}: {heat.shape[1]} classes (1 .. {MAX_TASK_CLASSES})")
        classes.append(int(heat.shape[1]))
        for name, c in _MAP_CHANNELS.items():
            v = m.get(name)
            if v is None:
                if name in has and not has[name]:
                    continue
                raise RuntimeError(f"task {t}: {name} is missing" + (" (reg / vel come for every task or for none)" if name in has else ""))
            if name in has and not has[name]:
                raise RuntimeError(f"task {t}: {name} given, task 0 has none (reg / vel come for every task or for none)")
            if tuple(v.shape) != (B, c, H, W) or v.dtype != torch.float32 or v.device != dev:
                raise RuntimeError(f"task {t}: {name} must be float32 [{B}, {c}, {H}, {W}] on {dev}, got {tuple(v.shape)} {v.dtype} on {v.device}")
    return B, H, W, classes


def _rows_device(heats, maps, coder, K, apply_sigmoid, norm_bbox, rotate, head_thr, post_limit, bottom_centre=True):
    lib = _capi.load()
    B, H, W, classes = _check_maps(heats, maps)
    if K > MAX_NUM:
        raise RuntimeError(f"max_num {K}: the device selection serves up to {MAX_NUM} rows per task and sample")
    T, dev = len(heats), heats[0].device
    heats = [h.detach().contiguous() for h in heats]
    flat_maps = []
    for m in maps:
        flat_maps += [None if m.get(k) is None else m[k].detach().contiguous() for k in ("reg", "height", "dim", "rot", "vel")]
    width = 9 if maps[0].get("vel") is not None else 7
    top_flat = torch.empty((B, T, K), dtype=torch.int32, device=dev)
    scores = torch.empty((B, T, K), dtype=torch.float32, device=dev)
    boxes = torch.empty((B, T, K, width), dtype=torch.float32, device=dev)
    labels = torch.empty((B, T, K), dtype=torch.int32, device=dev)
    live = torch.empty((B, T, K), dtype=torch.uint8, device=dev)
    post_ok = torch.empty((B, T, K), dtype=torch.uint8, device=dev)
    wsb = lib.bevamd_centerpoint_select_workspace_bytes(B, sum(classes), H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    consts = _capi.floats([coder.out_size_factor, coder.voxel_size[0], coder.voxel_size[1], coder.pc_range[0], coder.pc_range[1]])
    cthr = coder.score_threshold
    with torch.cuda.device(dev):
        stream = _capi.stream_ptr(dev)
        rc = lib.bevamd_centerpoint_select(_capi.pointers(heats), _capi.ints(classes), T, B, H, W, K, 1 if apply_sigmoid else 0,
                                           _capi.ptr(top_flat), _capi.ptr(scores), _capi.ptr(ws), wsb, stream)
        _capi.check(rc, "centerpoint_select")
        rc = lib.bevamd_centerpoint_decode(
            _capi.pointers(flat_maps), _capi.ints(classes), _capi.ints([1 if r else 0 for r in rotate]), T, B, H, W, K,
            _capi.ptr(top_flat), _capi.ptr(scores), 1 if norm_bbox else 0, 1 if bottom_centre else 0, consts, _capi.floats(list(coder.post_center_range)),
            float(cthr) if cthr else 0.0, 1 if cthr else 0, float(head_thr) if head_thr else 0.0, 1 if head_thr else 0,
            _capi.floats(list(post_limit)) if post_limit is not None else None, _capi.ptr(boxes), _capi.ptr(labels), _capi.ptr(live),
            _capi.ptr(post_ok), stream)
        _capi.check(rc, "centerpoint_decode")
    return boxes, scores, labels, live.bool(), post_ok.bool()


def _inside(x, y, z, rng):
    lo, hi = [float(np.float32(v)) for v in rng[:3]], [float(np.float32(v)) for v in rng[3:]]
    return (x >= lo[0]) & (y >= lo[1]) & (z >= lo[2]) & (x <= hi[0]) & (y <= hi[1]) & (z <= hi[2])


def _rows_host(heats, maps, coder, K, apply_sigmoid, norm_bbox, rotate, head_thr, post_limit, bottom_centre=True):
    """The reference's arithmetic on host tensors, per task, with the stable order; same outputs as _rows_device."""
    B, H, W, classes = _check_maps(heats, maps)
    out, base = [], 0
    for t, (heat, m) in enumerate(zip(heats, maps)):
        heat = heat.detach()
        flat_scores = (heat.sigmoid() if apply_sigmoid else heat).reshape(B, -1)
        top = flat_scores.argsort(dim=-1, descending=True, stable=True)[:, :K]
        sc = flat_scores.gather(1, top)
        cls, cell = top // (H * W), top % (H * W)

        def at(name, cell=cell, m=m):
            v = m[name].detach()
            return v.reshape(B, v.shape[1], H * W).gather(2, cell[:, None, :].expand(-1, v.shape[1], -1))

        xs, ys = (cell // W).float(), (cell % W).float()          # centerpoint_bbox_coders.py:87-90: the row comes first
        if m.get("reg") is not None:
            reg = at("reg")
            xs, ys = xs + reg[:, 0], ys + reg[:, 1]
        else:
            xs, ys = xs + 0.5, ys + 0.5
        xs = xs * coder.out_size_factor * coder.voxel_size[0] + coder.pc_range[0]
        ys = ys * coder.out_size_factor * coder.voxel_size[1] + coder.pc_range[1]
        hei, dim, rot = at("height")[:, 0], at("dim"), at("rot")
        if norm_bbox:
            dim = dim.exp()
        yaw = torch.atan2(rot[:, 0], rot[:, 1])
        cols = [xs, ys, hei - dim[:, 2] * 0.5 if bottom_centre else hei, dim[:, 0], dim[:, 1], dim[:, 2], yaw]
        if m.get("vel") is not None:
            vel = at("vel")
            cols += [vel[:, 0], vel[:, 1]]
        live = _inside(xs, ys, hei, coder.post_center_range)
        if coder.score_threshold:
            live &= sc > coder.score_threshold
        post = torch.ones_like(live)
        if rotate[t]:
            if head_thr:
                live &= sc >= torch.tensor([head_thr]).type_as(sc)
            if post_limit is not None:
                post = _inside(xs, ys, hei, post_limit)
        out.append((torch.stack(cols, -1), sc, (cls + base).to(torch.int32), live, post))
        base += classes[t]
    return tuple(torch.stack([o[i] for o in out], 1) for i in range(5))


# ---- rotated NMS ------------------------------------------------------------------------------------------------------------------
def _clip_area(a, b):
    """Area of the intersection of two convex quadrilaterals (float64 Sutherland-Hodgman; b counter-clockwise)."""
    subj = a
    for i in range(4):
        p, q = b[i], b[(i + 1) % 4]
        if not subj:
            return 0.0
        ex, ey = q[0] - p[0], q[1] - p[1]
        side = [ex * (r[1] - p[1]) - ey * (r[0] - p[0]) for r in subj]
        nxt = []
        for j in range(len(subj)):
            cur, prev, sc, sp = subj[j], subj[j - 1], side[j], side[j - 1]
            if (sc >= 0) != (sp >= 0):
                u = sp / (sp - sc)
                nxt.append((prev[0] + u * (cur[0] - prev[0]), prev[1] + u * (cur[1] - prev[1])))
            if sc >= 0:
                nxt.append(cur)
        subj = nxt
    if len(subj) < 3:
        return 0.0
    return abs(0.5 * sum(subj[i][0] * subj[(i + 1) % len(subj)][1] - subj[(i + 1) % len(subj)][0] * subj[i][1] for i in range(len(subj))))


def _corners(bx):
    x1, y1, x2, y2, ang = [float(v) for v in bx]
    cx, cy, c, s = (x1 + x2) / 2, (y1 + y2) / 2, math.cos(ang), math.sin(ang)
    pts = [((px - cx) * c + (py - cy) * s + cx, -(px - cx) * s + (py - cy) * c + cy) for px, py in ((x1, y1), (x2, y1), (x2, y2), (x1, y2))]
    area2 = sum(pts[i][0] * pts[(i + 1) % 4][1] - pts[(i + 1) % 4][0] * pts[i][1] for i in range(4))
    return pts if area2 >= 0 else pts[::-1]


def _rotate_nms_host(bev, thresh):
    """Greedy NMS (iou3d.cpp:115-132) over [n, 5] float32 (x1, y1, x2, y2, yaw) rows in descending score -> kept rows."""
    n = bev.shape[0]
    b64 = bev.astype(np.float64)
    centre = np.stack([(b64[:, 0] + b64[:, 2]) / 2, (b64[:, 1] + b64[:, 3]) / 2], 1)
    radius = 0.5 * np.hypot(b64[:, 2] - b64[:, 0], b64[:, 3] - b64[:, 1])
    area = (b64[:, 2] - b64[:, 0]) * (b64[:, 3] - b64[:, 1])
    corners = [None] * n
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if suppressed[i]:
            continue
        keep.append(i)
        rest = np.nonzero(~suppressed[i + 1:])[0] + i + 1
        near = rest[np.hypot(*(centre[rest] - centre[i]).T) < radius[rest] + radius[i]]
        for j in near:
            for q in (i, j):
                if corners[q] is None:
                    corners[q] = _corners(b64[q])
            inter = _clip_area(corners[i], corners[j])
            if inter / max(area[i] + area[j] - inter, 1e-8) > thresh:
                suppressed[j] = True
    return keep


def _bev_xyxyr_host(boxes, labels, label_base, scales):
    """box.bev with the per-class scale on (w, l) (centerpoint.py:826-833), then xywhr2xyxyr, in fp32."""
    bev = boxes[:, [0, 1, 3, 4, 6]].astype(np.float32)
    for cls, scale in enumerate(scales):
        bev[labels - label_base == cls, 2:4] *= np.float32(scale)
    hw, hl = bev[:, 2] / 2, bev[:, 3] / 2
    return np.stack([bev[:, 0] - hw, bev[:, 1] - hl, bev[:, 0] + hw, bev[:, 1] + hl, bev[:, 4]], 1)


def rotate_nms_segments(boxes, live, thresh, pre_max_size=None, post_max_size=None, labels=None, scales=None, post_ok=None,
                        enabled=None, label_base=None):
    """Segmented rotated NMS, no sync: boxes [S, R, >= 7] fp32 (x, y, z, w, l, h, yaw, ...) with the rows of a segment ALREADY in
    descending score, live [S, R] bool or None.  Segment s belongs to task s % T, T = len(thresh) (a float: one task); labels
    [S, R] int32, scales [T][classes], label_base [T] and enabled [T] are per task.  Returns (keep [S, R] bool, counts [S] int32):
    greedy at rotated BEV IoU > thresh over the first pre_max_size live rows, the first post_max_size kept rows, then post_ok."""
    thresh = [float(thresh)] if not isinstance(thresh, (list, tuple)) else [float(v) for v in thresh]
    T = len(thresh)
    if boxes.dim() != 3 or boxes.shape[2] < 7 or boxes.dtype != torch.float32:
        raise RuntimeError(f"boxes must be float32 [S, R, >= 7], got {tuple(boxes.shape)} {boxes.dtype}")
    S, R, width = boxes.shape
    pre = R if pre_max_size is None else int(pre_max_size)
    post = R if post_max_size is None else int(post_max_size)
    enabled = [True] * T if enabled is None else list(enabled)
    label_base = [0] * T if label_base is None else list(label_base)
    if scales is not None and labels is None:
        raise RuntimeError("per-class scales need labels")
    if not boxes.is_cuda:
        keep = torch.zeros((S, R), dtype=torch.bool)
        b, lb = boxes.detach().numpy(), (labels.numpy() if labels is not None else np.zeros((S, R), np.int32))
        for s in range(S):
            t = s % T
            if not enabled[t]:
                continue
            rows = (np.nonzero(live[s].numpy())[0] if live is not None else np.arange(R))[:pre]
            bev = _bev_xyxyr_host(b[s][rows], lb[s][rows], label_base[t], scales[t] if scales is not None else [])
            kept = rows[_rotate_nms_host(bev, thresh[t])[:post]]
            keep[s, kept] = True
        if post_ok is not None:
            keep &= post_ok
        return keep, keep.sum(1, dtype=torch.int32)
    lib = _capi.load()
    dev = boxes.device
    table = None
    if scales is not None:
        table = []
        for t in range(T):
            if len(scales[t]) > MAX_TASK_CLASSES:
                raise RuntimeError(f"task {t}: {len(scales[t])} scales (at most {MAX_TASK_CLASSES})")
            table += [float(v) for v in scales[t]] + [1.0] * (MAX_TASK_CLASSES - len(scales[t]))
    u8 = lambda v: None if v is None else v.to(torch.uint8).contiguous()   # noqa: E731
    boxes, live, post_ok = boxes.detach().contiguous(), u8(live), u8(post_ok)
    if labels is not None:
        labels = labels.to(torch.int32).contiguous()
    keep = torch.empty((S, R), dtype=torch.uint8, device=dev)
    counts = torch.empty(S, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bevamd_rotate_nms_segments(_capi.ptr(boxes), width, _capi.ptr(labels), _capi.ptr(live), _capi.ptr(post_ok), S, R, T,
                                            _capi.ints([1 if e else 0 for e in enabled]), _capi.floats(thresh), _capi.ints(label_base),
                                            _capi.floats(table) if table is not None else None, pre, post, _capi.ptr(keep),
                                            _capi.ptr(counts), _capi.stream_ptr(dev))
    _capi.check(rc, "rotate_nms_segments")
    return keep.bool(), counts


# ---- box coder ---------------------------------------------------------------------------------------------------------------------
class CenterPointBBoxCoder:
    """mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py: the max_num best cells of a heatmap and their boxes in metres."""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None, max_num=100, score_threshold=None, code_size=9):
        self.pc_range = pc_range
        self.out_size_factor = out_size_factor
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.code_size = code_size

    def encode(self):
        pass

    def _check(self, height, width):
        if self.post_center_range is None:
            raise NotImplementedError("Need to reorganize output as a batch, only support post_center_range is not None for now!")
        if self.max_num > height * width:
            raise RuntimeError(f"max_num {self.max_num} is out of range: a {height} x {width} map has {height * width} cells")

    def decode(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, task_id=-1):
        """heat [B, C, H, W] SCORES, rot_sine / rot_cosine / hei [B, 1, H, W], dim [B, 3, H, W] (sizes, not logs), vel [B, 2, H, W] or
        None, reg [B, 2, H, W] or None -> per sample dict(bboxes [n, 7|9], scores [n], labels [n] float): the max_num best cells
        inside post_center_range (inclusive) whose score exceeds a non-zero score_threshold, in descending score."""
        if heat.dim() != 4:
            raise RuntimeError(f"heat must be [B, C, H, W], got {tuple(heat.shape)}")
        self._check(heat.shape[2], heat.shape[3])
        for name, v in (("rot_sine", rot_sine), ("rot_cosine", rot_cosine)):
            if tuple(v.shape) != (heat.shape[0], 1) + tuple(heat.shape[2:]):
                raise RuntimeError(f"{name} must be [{heat.shape[0]}, 1, {heat.shape[2]}, {heat.shape[3]}], got {tuple(v.shape)}")
        maps = [dict(reg=reg, height=hei, dim=dim, rot=torch.cat([rot_sine, rot_cosine], 1), vel=vel)]
        rows = _rows_device if heat.is_cuda else _rows_host
        boxes, scores, labels, live, _ = rows([heat], maps, self, int(self.max_num), False, False, [False], None, None,
                                              bottom_centre=False)       # the coder returns the gravity centre's height
        return [dict(bboxes=boxes[i, 0][live[i, 0]], scores=scores[i, 0][live[i, 0]], labels=labels[i, 0][live[i, 0]].float())
                for i in range(heat.shape[0])]


register_everywhere("bbox_coder", CenterPointBBoxCoder)


# ---- get_bboxes ------------------------------------------------------------------------------------------------------------------
def _per_task(value, T, name):
    values = list(value) if isinstance(value, (list, tuple)) else [value] * T
    if len(values) != T:
        raise ValueError(f"{name} has {len(values)} entries for {T} tasks")
    return values


def _circle_tables(B, T, K, radii, circle, dev):
    """(seg_offsets [B * T + 1] int32, seg_thresh [B * T] fp32, circle-task mask [1, T, 1] bool) on `dev`, built once per key:
    creating them copies from the host, which a graph capture does not allow."""
    key = (B, T, K, tuple(radii), tuple(circle), str(dev))
    if key not in _CONST_CACHE:
        _CONST_CACHE[key] = ((torch.arange(B * T + 1, dtype=torch.int64) * K).to(torch.int32).to(dev),
                             torch.tensor(list(radii) * B, dtype=torch.float32, device=dev),
                             torch.tensor(list(circle), dtype=torch.bool, device=dev).view(1, T, 1))
    return _CONST_CACHE[key]


def centerhead_get_bboxes(preds_dicts, bbox_coder, test_cfg, num_classes, norm_bbox=True, sync=True):
    """get_bboxes of CenterHead.  preds_dicts: one [dict] per task with heatmap [B, Ct, H, W] LOGITS, reg [B, 2, H, W], height
    [B, 1, H, W], dim [B, 3, H, W], rot [B, 2, H, W] and optionally vel [B, 2, H, W]; num_classes: the per-task list; test_cfg:
    nms_type ("circle" / "rotate" or a per-task list), min_radius (per task, circle), post_max_size, pre_max_size, nms_thr,
    score_threshold (tested with >= before the rotated NMS), post_center_limit_range (after the NMS cap of a rotate task; empty: no
    test), nms_scale (scalar, nested list or absent).  K = bbox_coder.max_num rows per task.

    sync=True : [dict(bboxes [n, 7|9], scores [n], labels [n] int32)] per sample: tasks in order, descending score within a task,
                labels offset by the running class count, z moved to the bottom centre (device tensors: one read-back of the B counts).
    sync=False: dict(bboxes [B, T * K, 7|9], scores, labels [B, T * K], keep [B, T * K] bool, counts [B] int32), no sync, rows in
                (task, descending score) order: x[b][keep[b]] is the sync=True result.
    Wrapping into metas[i]["box_type_3d"] stays with the caller; the rotated NMS uses the LiDAR box convention."""
    T = len(preds_dicts)
    num_classes = list(num_classes)
    if len(num_classes) != T:
        raise RuntimeError(f"{T} tasks, num_classes lists {len(num_classes)}")
    preds = [p[0] if isinstance(p, (list, tuple)) else p for p in preds_dicts]
    heats = [p["heatmap"] for p in preds]
    for t, h in enumerate(heats):
        if h.dim() != 4 or h.shape[1] != num_classes[t]:
            raise RuntimeError(f"task {t}: heatmap {tuple(h.shape)}, num_classes says {num_classes[t]}")
    nms_types = _per_task(test_cfg["nms_type"], T, "nms_type")
    for v in nms_types:
        if v not in ("circle", "rotate"):
            raise ValueError(f"nms_type {v!r} ('circle', 'rotate')")
    rotate = [v == "rotate" for v in nms_types]
    if "nms_scale" in test_cfg:
        scale = test_cfg["nms_scale"]
        scales = [list(s) for s in scale] if isinstance(scale, list) else [[scale] * num_classes[t] for t in range(T)]
        if len(scales) != T or any(len(scales[t]) > num_classes[t] for t in range(T)):
            raise ValueError("nms_scale lists at most one factor per class of every task")
    else:
        scales = [[1.0] * num_classes[t] for t in range(T)]
    K = int(bbox_coder.max_num)
    bbox_coder._check(heats[0].shape[2], heats[0].shape[3])
    head_thr = test_cfg["score_threshold"] if any(rotate) and test_cfg["score_threshold"] > 0.0 else None
    post_limit = None
    if any(rotate) and len(test_cfg["post_center_limit_range"]) > 0:
        post_limit = list(test_cfg["post_center_limit_range"])
    maps = [dict(reg=p["reg"], height=p["height"], dim=p["dim"], rot=p["rot"], vel=p.get("vel")) for p in preds]
    device = heats[0].is_cuda
    rows = _rows_device if device else _rows_host
    boxes, scores, labels, live, post_ok = rows(heats, maps, bbox_coder, K, True, norm_bbox, rotate, head_thr, post_limit)
    B, width = boxes.shape[0], boxes.shape[-1]
    label_base = [sum(num_classes[:t]) for t in range(T)]
    pms = test_cfg["post_max_size"]

    keep = None
    if any(rotate):
        keep, _ = rotate_nms_segments(boxes.view(B * T, K, width), live.view(B * T, K), [float(test_cfg["nms_thr"])] * T,
                                      test_cfg.get("pre_max_size"), pms, labels.view(B * T, K), scales, post_ok.view(B * T, K), rotate,
                                      label_base)
        keep = keep.view(B, T, K)
    if not all(rotate):
        radii = [float(r) if not rotate[t] else 0.0 for t, r in enumerate(_per_task(test_cfg["min_radius"], T, "min_radius"))]
        cap = K if pms is None else int(pms)
        circle = [not r for r in rotate]
        if device:
            from .heads import circle_nms_segments

            seg_off, seg_thr, cmask = _circle_tables(B, T, K, radii, circle, boxes.device)
            live_c = live & cmask if any(rotate) else live
            kc, _, _ = circle_nms_segments(boxes[..., :2].reshape(-1, 2), scores.reshape(-1), seg_off, seg_thr, K, cap, live_c.reshape(-1))
            kc = kc.view(B, T, K)
        else:
            from .heads import _circle_nms_host

            kc = torch.zeros_like(live)
            for b in range(B):
                for t in range(T):
                    if circle[t]:
                        r = torch.nonzero(live[b, t])[:, 0]
                        dets = torch.cat([boxes[b, t][r][:, :2], scores[b, t][r][:, None]], 1).numpy()
                        kc[b, t, r[torch.as_tensor(_circle_nms_host(dets, radii[t], cap), dtype=torch.int64)]] = True
        keep = kc if keep is None else keep | kc

    boxes, scores, labels, keep = boxes.view(B, T * K, width), scores.view(B, T * K), labels.view(B, T * K), keep.view(B, T * K)
    counts = keep.sum(1, dtype=torch.int32)
    if not sync:
        return dict(bboxes=boxes, scores=scores, labels=labels, keep=keep, counts=counts)
    # kept rows first, in row order; then ONE read-back
    front = torch.sort(keep.to(torch.uint8), dim=1, descending=True, stable=True).indices
    boxes = boxes.gather(1, front[:, :, None].expand(-1, -1, width))
    scores, labels = scores.gather(1, front), labels.gather(1, front)
    return [dict(bboxes=boxes[i, :n], scores=scores[i, :n], labels=labels[i, :n]) for i, n in enumerate(counts.tolist())]
