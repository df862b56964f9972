"""Training targets of the two detection heads on the device (reference: CenterHead.get_targets / get_targets_single,
mmdet3d/models/heads/bbox/centerpoint.py:375-582; the dense heatmap of TransFusionHead.get_targets_single, transfusion.py:526-573;
mmdet3d/core/utils/gaussian.py), over csrc/ext/head_targets.hip.  `heads` re-exports everything here.

  * `centerhead_get_targets`: the reference's tuple (heatmaps, anno_boxes, inds, masks), each a list over tasks of [B, ...] tensors:
    three launches for any number of samples, tasks and boxes, no host sync;
  * `transfusion_heatmap_targets`: the dense [B, C, H, W] heatmap: two launches, no host sync.

Ground truth comes as the reference's lists (one [n_i, 7|9] tensor, or an object with such a `.tensor`, and one [n_i] label tensor
per sample: packed here from the shapes alone) or already packed as `(boxes [M, 7|9], labels [M], offsets [B + 1] int32)` with
`gt_labels_3d=None` and the caller's `max_boxes_per_sample`, which is the form a captured graph replays with fresh box buffers.

There is no CPU path: host tensors raise.  `_targets_host` restates the arithmetic in fp32 / float64 numpy for the tests.

Differences from the reference, on purpose: maps are square (the reference draws on a [size[1], size[0]] plane at row cell_x,
column cell_y and indexes it with cell_x * size[1] + cell_y: consistent only when size[0] == size[1]); 7-column boxes give zero
velocity targets (the reference's `vx, vy = box[7:]` raises); a sample over `max_boxes_per_sample` yields zeros and an overflow
flag; `transfusion_heatmap_targets` skips a box whose centre cell is outside the map or whose label is outside [0, C), where the
reference's negative slices index from the end.
"""
import numpy as np
import torch

from . import _capi

__all__ = ["centerhead_get_targets", "transfusion_heatmap_targets"]

MAX_BOXES = 1024         # HT_MAX_BOXES of the kernels: boxes per sample
MAX_CLASSES = 64
MAX_TASKS = 16
_OFFSET_CACHE = {}


def _map_size(train_cfg):
    grid = [int(v) for v in list(train_cfg["grid_size"])[:2]]
    osf = int(train_cfg["out_size_factor"])
    size = [g // osf for g in grid]
    if size[0] != size[1]:
        raise ValueError(f"feature map {size[0]} x {size[1]}: only square maps are served (the reference draws the heatmap at "
                         "(row cell_x, column cell_y) of a [size[1], size[0]] plane and indexes it with cell_x * size[1] + cell_y: its "
                         "row/column use is inconsistent unless size[0] == size[1])")
    return size[0], osf


def _check_classes(total):
    if not 1 <= total <= MAX_CLASSES:
        raise ValueError(f"{total} classes (1 .. {MAX_CLASSES})")


def _check_bound(bound):
    if bound is None:
        raise ValueError("packed ground truth needs max_boxes_per_sample")
    if not 1 <= int(bound) <= MAX_BOXES:
        raise ValueError(f"max_boxes_per_sample {bound} (1 .. {MAX_BOXES})")
    return int(bound)


def _offsets(counts, dev):
    """[B + 1] int32 on `dev` for the given per-sample counts, built once per key through pinned memory without a sync."""
    key = (tuple(counts), str(dev))
    if key not in _OFFSET_CACHE:
        if len(_OFFSET_CACHE) > 4096:
            _OFFSET_CACHE.clear()
        host = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).pin_memory()
        _OFFSET_CACHE[key] = (host, host.to(dev, non_blocking=True))      # the pinned source outlives the copy
    return _OFFSET_CACHE[key][1]


def _pack(gt_bboxes_3d, gt_labels_3d, max_boxes_per_sample):
    """-> (boxes [M, 7|9] fp32, labels [M] int64, offsets [B + 1] int32, B, bound), all on one device, without a sync."""
    if max_boxes_per_sample is not None:
        _check_bound(max_boxes_per_sample)
    if gt_labels_3d is None:
        if not (isinstance(gt_bboxes_3d, (tuple, list)) and len(gt_bboxes_3d) == 3):
            raise ValueError("packed ground truth is the triple (boxes, labels, offsets) with gt_labels_3d=None")
        boxes, labels, offsets = gt_bboxes_3d
        bound = _check_bound(max_boxes_per_sample)
        for t in (boxes, labels, offsets):
            if not t.is_cuda:
                raise RuntimeError("head targets need GPU tensors (there is no CPU path)")
        if boxes.dim() != 2 or boxes.shape[1] not in (7, 9) or labels.shape != (boxes.shape[0],) or offsets.dim() != 1 or offsets.shape[0] < 2:
            raise RuntimeError(f"boxes [M, 7|9], labels [M], offsets [B + 1] expected, got {tuple(boxes.shape)}, {tuple(labels.shape)}, "
                               f"{tuple(offsets.shape)}")
        if boxes.dtype != torch.float32 or labels.dtype != torch.int64 or offsets.dtype != torch.int32:
            raise RuntimeError(f"boxes float32, labels int64, offsets int32 expected, got {boxes.dtype}, {labels.dtype}, {offsets.dtype}")
        return boxes.detach().contiguous(), labels.contiguous(), offsets.contiguous(), offsets.shape[0] - 1, bound
    tensors = [b.tensor if hasattr(b, "tensor") else b for b in gt_bboxes_3d]
    if len(tensors) == 0 or len(tensors) != len(gt_labels_3d):
        raise ValueError(f"{len(tensors)} box tensors for {len(gt_labels_3d)} label tensors")
    for b, l in zip(tensors, gt_labels_3d):
        if not (b.is_cuda and l.is_cuda):
            raise RuntimeError("head targets need GPU tensors (there is no CPU path)")
        if b.dim() != 2 or b.shape[1] != tensors[0].shape[1] or b.shape[1] not in (7, 9) or l.shape != (b.shape[0],):
            raise RuntimeError(f"per sample boxes [n, 7|9] and labels [n] expected, got {tuple(b.shape)} and {tuple(l.shape)}")
    counts = [int(b.shape[0]) for b in tensors]
    bound = max(max(counts), 1) if max_boxes_per_sample is None else int(max_boxes_per_sample)
    if max(counts) > MAX_BOXES and max_boxes_per_sample is None:
        raise ValueError(f"a sample has {max(counts)} boxes: max_boxes_per_sample is at most {MAX_BOXES}")
    bound = _check_bound(bound)
    dev = tensors[0].device
    boxes = torch.cat([b.detach().to(torch.float32) for b in tensors]).contiguous()
    labels = torch.cat([l.to(torch.int64) for l in gt_labels_3d]).contiguous()
    return boxes, labels, _offsets(counts, dev), len(tensors), bound


def _cfg_arrays(train_cfg):
    return (_capi.floats(list(train_cfg["point_cloud_range"])[:2]), _capi.floats(list(train_cfg["voxel_size"])[:2]),
            float(train_cfg["gaussian_overlap"]), int(train_cfg["min_radius"]))


def centerhead_get_targets(gt_bboxes_3d, gt_labels_3d, num_classes, train_cfg, norm_bbox=True, max_boxes_per_sample=None,
                           return_overflow=False):
    """get_targets of CenterHead.  num_classes: the per-task list (task t owns the labels [flag_t, flag_t + num_classes[t]); other
    labels are ignored); train_cfg: grid_size, out_size_factor, voxel_size, point_cloud_range, max_objs, dense_reg,
    gaussian_overlap, min_radius.  Returns (heatmaps, anno_boxes, inds, masks): lists over tasks of [B, C_t, H, W] fp32,
    [B, max_objs * dense_reg, 10] fp32, [B, max_objs * dense_reg] int64 and uint8 (views of four buffers); with return_overflow a
    fifth entry, [B] int32: 1 for a sample with more boxes than max_boxes_per_sample (its targets are all zero)."""
    num_classes = [int(c) for c in num_classes]
    if not 1 <= len(num_classes) <= MAX_TASKS:
        raise ValueError(f"{len(num_classes)} tasks (1 .. {MAX_TASKS})")
    _check_classes(sum(num_classes))
    size, osf = _map_size(train_cfg)
    boxes, labels, offsets, B, bound = _pack(gt_bboxes_3d, gt_labels_3d, max_boxes_per_sample)
    lib = _capi.load()
    T, dev = len(num_classes), boxes.device
    max_objs = int(train_cfg["max_objs"]) * int(train_cfg["dense_reg"])
    heat = torch.empty(B * sum(num_classes) * size * size, dtype=torch.float32, device=dev)
    anno = torch.empty((T, B, max_objs, 10), dtype=torch.float32, device=dev)
    ind = torch.empty((T, B, max_objs), dtype=torch.int64, device=dev)
    mask = torch.empty((T, B, max_objs), dtype=torch.uint8, device=dev)
    overflow = torch.empty(B, dtype=torch.int32, device=dev)
    pc, vs, overlap, min_radius = _cfg_arrays(train_cfg)
    with torch.cuda.device(dev):
        rc = lib.bevamd_centerhead_targets(_capi.ptr(boxes), _capi.ptr(labels), _capi.ptr(offsets), boxes.shape[0], boxes.shape[1], B,
                                           bound, _capi.ints(num_classes), T, max_objs, pc, vs, osf, size, overlap, min_radius,
                                           1 if norm_bbox else 0, _capi.ptr(heat), _capi.ptr(anno), _capi.ptr(ind), _capi.ptr(mask),
                                           _capi.ptr(overflow), _capi.stream_ptr(dev))
    _capi.check(rc, "centerhead_targets")
    heatmaps, base = [], 0
    for c in num_classes:
        heatmaps.append(heat[base:base + B * c * size * size].view(B, c, size, size))
        base += B * c * size * size
    out = (heatmaps, list(anno.unbind(0)), list(ind.unbind(0)), list(mask.unbind(0)))
    return out + (overflow,) if return_overflow else out


def transfusion_heatmap_targets(gt_bboxes_3d, gt_labels_3d, num_classes, train_cfg, max_boxes_per_sample=None, return_overflow=False):
    """The dense heatmap of TransFusionHead.get_targets_single for all samples: [B, num_classes, H, W] fp32 (with return_overflow:
    and the [B] int32 flags).  train_cfg: grid_size, out_size_factor, voxel_size, point_cloud_range, gaussian_overlap, min_radius.
    A box whose centre cell is outside the map or whose label is outside [0, num_classes) is skipped."""
    num_classes = int(num_classes)
    _check_classes(num_classes)
    size, osf = _map_size(train_cfg)
    boxes, labels, offsets, B, bound = _pack(gt_bboxes_3d, gt_labels_3d, max_boxes_per_sample)
    lib = _capi.load()
    dev = boxes.device
    heat = torch.empty((B, num_classes, size, size), dtype=torch.float32, device=dev)
    overflow = torch.empty(B, dtype=torch.int32, device=dev)
    pc, vs, overlap, min_radius = _cfg_arrays(train_cfg)
    with torch.cuda.device(dev):
        rc = lib.bevamd_heatmap_targets(_capi.ptr(boxes), _capi.ptr(labels), _capi.ptr(offsets), boxes.shape[0], boxes.shape[1], B, bound,
                                        num_classes, pc, vs, osf, size, overlap, min_radius, _capi.ptr(heat), _capi.ptr(overflow),
                                        _capi.stream_ptr(dev))
    _capi.check(rc, "heatmap_targets")
    return (heat, overflow) if return_overflow else heat


# ---- host mirror (tests only) ------------------------------------------------------------------------------------------------------
def _geometry_host(boxes, train_cfg, size, osf):
    """Per box, as the kernels' ht_geometry: (live [M] bool, radius [M] int64, coor [M, 2] fp32, cell [M, 2] int64)."""
    f = np.float32
    boxes = np.asarray(boxes, np.float32).reshape(-1, boxes.shape[-1])
    pc0, pc1 = (f(v) for v in list(train_cfg["point_cloud_range"])[:2])
    vs0, vs1 = (f(v) for v in list(train_cfg["voxel_size"])[:2])
    m, osf = float(train_cfg["gaussian_overlap"]), f(osf)
    k1, k2, km2, kmm1, k16m = f(1 - m), f(1 + m), f(-2 * m), f(m - 1), f(4 * (4 * m))
    with np.errstate(all="ignore"):
        w = boxes[:, 3] / vs0 / osf
        h = boxes[:, 4] / vs1 / osf
        ok = (w > 0) & (h > 0)
        hw = h + w
        b1 = hw
        c1 = w * h * k1 / k2
        r1 = (b1 + np.sqrt(b1 * b1 - f(4) * c1)) / f(2)
        b2 = f(2) * hw
        c2 = k1 * w * h
        r2 = (b2 + np.sqrt(b2 * b2 - f(16) * c2)) / f(2)
        b3 = km2 * hw
        c3 = kmm1 * w * h
        r3 = (b3 + np.sqrt(b3 * b3 - k16m * c3)) / f(2)
        r = np.where(r2 < r1, r2, r1)
        r = np.where(r3 < r, r3, r)
        assert r.dtype == np.float32
        radius = np.maximum(int(train_cfg["min_radius"]), np.trunc(np.where(ok & (r < 2.0 ** 30), r, 0)).astype(np.int64))
        coor = np.stack([(boxes[:, 0] - pc0) / vs0 / osf, (boxes[:, 1] - pc1) / vs1 / osf], 1)
        assert coor.dtype == np.float32
        inside = ((coor > -1) & (coor < size)).all(1)
        cell = np.trunc(np.where(inside[:, None], coor, 0)).astype(np.int64)
    return ok & inside, radius, coor, cell


def _draw_host(plane, row, col, radius):
    """draw_heatmap_gaussian(plane, (col, row), radius) with the float64 Gaussian restated."""
    size = plane.shape[0]
    left, right, top, bottom = min(col, radius), min(size - col, radius + 1), min(row, radius), min(size - row, radius + 1)
    ys = np.arange(-top, bottom, dtype=np.float64)[:, None]
    xs = np.arange(-left, right, dtype=np.float64)[None, :]
    sigma = (2 * radius + 1) / 6
    g = np.exp(-(xs * xs + ys * ys) / (2 * sigma * sigma))
    g[g < np.finfo(np.float64).eps * 1.0] = 0                # the full window's maximum is the centre's 1
    win = plane[row - top:row + bottom, col - left:col + right]
    np.maximum(win, g.astype(np.float32), out=win)


def _targets_host(boxes, labels, offsets, num_classes, train_cfg, norm_bbox=True, max_boxes_per_sample=MAX_BOXES):
    """The kernels' arithmetic in fp32 / float64 numpy on packed host arrays.  num_classes a list: (heatmaps, anno_boxes, inds,
    masks, overflow) as centerhead_get_targets returns them; an int: (heatmap, overflow) as transfusion_heatmap_targets does."""
    size, osf = _map_size(train_cfg)
    boxes, labels = np.asarray(boxes, np.float32), np.asarray(labels, np.int64)
    offsets = np.asarray(offsets, np.int64)
    B = len(offsets) - 1
    live, radius, coor, cell = _geometry_host(boxes, train_cfg, size, osf)
    overflow = ((offsets[1:] - offsets[:-1]) > max_boxes_per_sample).astype(np.int32)
    if not isinstance(num_classes, (list, tuple)):
        heat = np.zeros((B, int(num_classes), size, size), np.float32)
        for b in range(B):
            if overflow[b]:
                continue
            for i in range(offsets[b], offsets[b + 1]):
                if live[i] and 0 <= labels[i] < int(num_classes):
                    _draw_host(heat[b, labels[i]], cell[i, 0], cell[i, 1], int(radius[i]))
        return heat, overflow
    T = len(num_classes)
    max_objs = int(train_cfg["max_objs"]) * int(train_cfg["dense_reg"])
    heatmaps = [np.zeros((B, c, size, size), np.float32) for c in num_classes]
    anno = np.zeros((T, B, max_objs, 10), np.float32)
    ind = np.zeros((T, B, max_objs), np.int64)
    mask = np.zeros((T, B, max_objs), np.uint8)
    b64 = boxes.astype(np.float64)
    with np.errstate(all="ignore"):
        dims = np.log(b64[:, 3:6]).astype(np.float32) if norm_bbox else boxes[:, 3:6]
    sin, cos = np.sin(b64[:, 6]).astype(np.float32), np.cos(b64[:, 6]).astype(np.float32)
    z = boxes[:, 2] + boxes[:, 5] * np.float32(0.5)
    for b in range(B):
        if overflow[b]:
            continue
        rows = np.arange(offsets[b], offsets[b + 1])
        flag = 0
        for t, ct in enumerate(num_classes):
            order = np.concatenate([rows[labels[rows] == flag + c] for c in range(ct)])[:max_objs]   # class-major, stable
            for k, i in enumerate(order):
                if not live[i]:
                    continue
                _draw_host(heatmaps[t][b, labels[i] - flag], cell[i, 0], cell[i, 1], int(radius[i]))
                ind[t, b, k] = cell[i, 0] * size + cell[i, 1]
                mask[t, b, k] = 1
                vel = boxes[i, 7:9] if boxes.shape[1] >= 9 else np.zeros(2, np.float32)
                anno[t, b, k] = np.concatenate([coor[i] - cell[i].astype(np.float32), z[i:i + 1], dims[i], sin[i:i + 1], cos[i:i + 1], vel])
            flag += ct
    return heatmaps, list(anno), list(ind), list(mask), overflow
