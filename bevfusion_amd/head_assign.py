"""The assignment end of TransFusionHead.get_targets on the device (reference: mmdet3d/models/heads/bbox/transfusion.py:357-585,
mmdet3d/core/bbox/assigners/hungarian_assigner.py, BaseInstance3DBoxes.overlaps of core/bbox/structures/base_box3d.py:378-445, and
mmdet 2.x's FocalLossCost / ClassificationCost / AssignResult, which the reference imports), over csrc/ext/head_assign.hip.
`heads` re-exports everything here.

  * `linear_sum_assignment_batch`: scipy.optimize.linear_sum_assignment for a batch of rectangular fp32 problems whose live sizes
    are read from device memory: one launch, one wave per problem, fp64 duals;
  * `FocalLossCost`, `ClassificationCost`, `BBoxBEVL1Cost`, `IoU3DCost`, `BboxOverlaps3D`: the match costs and the IoU calculator
    with the constructor signatures of the reference and mmdet, registered in `registry.MATCH_COST` / `IOU_CALCULATORS`;
  * `HungarianAssigner3D`: the reference's assigner (`registry.BBOX_ASSIGNERS`); `.assign` returns an `AssignResult`;
  * `transfusion_get_targets`: get_targets for all samples and decoder layers: box decode, match costs, assignment, target rows and
    the dense heatmap as seven launches with no host sync (sync=False) or one 8-byte read-back at the very end (sync=True).

There is no CPU path: host tensors raise.  `_targets_host` restates the arithmetic in numpy with scipy's solver for the tests.

Differences from the reference, on purpose: a sample without ground truth yields all-negative targets (the reference's
`AssignResult(max_overlaps=None)` makes its `torch.cat` raise); a sample over `max_boxes_per_sample`, or with a status word (a
non-finite cost, a label outside [0, num_classes), a solver bound), yields all-negative targets and a flag; a fractional
`pos_weight` raises (the reference writes it into an int64 tensor, which truncates it); only `HungarianAssigner3D` is served
(`HeuristicAssigner` raises NotImplementedError); where the optimum is not unique (equal totals) the matching may differ from
scipy's, the total does not.
"""
import numpy as np
import torch

from . import _capi
from .head_targets import MAX_BOXES, MAX_CLASSES, _pack, transfusion_heatmap_targets
from .registry import BBOX_ASSIGNERS, IOU_CALCULATORS, MATCH_COST, build_from_cfg, register_everywhere

__all__ = ["linear_sum_assignment_batch", "FocalLossCost", "ClassificationCost", "BBoxBEVL1Cost", "IoU3DCost", "BboxOverlaps3D",
           "AssignResult", "HungarianAssigner3D", "transfusion_get_targets", "BBOX_ASSIGNERS", "MATCH_COST", "IOU_CALCULATORS",
           "STATUS_NONFINITE", "STATUS_LABEL", "STATUS_OVERFLOW", "STATUS_BOUND"]

MAX_SIDE = 1024          # HA_MAX_SIDE of the kernels: rows / columns of one problem, proposals per layer
STATUS_NONFINITE, STATUS_LABEL, STATUS_OVERFLOW, STATUS_BOUND = 1, 2, 4, 8


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the assignment needs GPU tensors (there is no CPU path)")


# ---- the solver ------------------------------------------------------------------------------------------------------------------
def linear_sum_assignment_batch(cost, rows=None, cols=None):
    """cost [N, R, C] (or [R, C]) fp32 on the device, rows / cols [N] int32 device tensors with the live size of every problem
    (None: the full side; entries outside the live block are never read).  Returns (col4row [N, R] int32: the column matched to
    every row, -1 for none; status [N] int32: 0, STATUS_NONFINITE or STATUS_BOUND, with all rows -1).  min(rows, cols) rows are
    matched and the total is minimal for the fp32 matrix.  No host sync."""
    _need_gpu(cost, rows, cols)
    single = cost.dim() == 2
    if single:
        cost = cost[None]
    if cost.dim() != 3 or cost.dtype != torch.float32:
        raise RuntimeError(f"cost must be a float32 [N, R, C] tensor, got {tuple(cost.shape)} {cost.dtype}")
    N, R, C = cost.shape
    if not (1 <= R <= MAX_SIDE and 1 <= C <= MAX_SIDE):
        raise ValueError(f"a {R} x {C} problem: each side is 1 .. {MAX_SIDE}")
    if N < 1:
        raise ValueError("no problems")
    for name, t in (("rows", rows), ("cols", cols)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (N,)):
            raise RuntimeError(f"{name} must be an int32 [{N}] tensor, got {tuple(t.shape)} {t.dtype}")
    dev = cost.device
    cost = cost.detach().contiguous()
    col4row = torch.empty((N, R), dtype=torch.int32, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    lib = _capi.load()
    with torch.cuda.device(dev):
        rc = lib.bevamd_linear_sum_assignment(_capi.ptr(cost), _capi.ptr(None if rows is None else rows.contiguous()),
                                              _capi.ptr(None if cols is None else cols.contiguous()), N, R, C, _capi.ptr(col4row),
                                              _capi.ptr(status), _capi.stream_ptr(dev))
    _capi.check(rc, "linear_sum_assignment")
    return (col4row[0], status[0]) if single else (col4row, status)


# ---- match costs -----------------------------------------------------------------------------------------------------------------
def _match_costs(boxes, logits, gt, layers, K, bound, cls_cost=None, reg_cost=None, iou_cost=None, pc_range=None, want_iou=False):
    """bevamd_match_costs.  boxes [B, L * K, 7|9] or None, logits [B, C, L * K] or None, gt = (boxes [M, 7|9], labels [M], offsets
    [B + 1]) packed.  -> (cost, iou [B, L, K, bound] fp32, num_gt, status [B * L] int32)."""
    gt_boxes, gt_labels, offsets = gt
    B = offsets.shape[0] - 1
    dev = gt_boxes.device
    mode, classes = 0, 0
    w_cls, alpha, gamma, eps = 0.0, 0.25, 2.0, 1e-12
    if cls_cost is not None:
        if isinstance(cls_cost, ClassificationCost):                       # (a subclass of FocalLossCost: first)
            mode = 2
        elif isinstance(cls_cost, FocalLossCost):
            mode, alpha, gamma, eps = 1, cls_cost.alpha, cls_cost.gamma, cls_cost.eps
        else:
            raise NotImplementedError(f"classification cost {type(cls_cost).__name__} (FocalLossCost, ClassificationCost)")
        w_cls, classes = cls_cost.weight, logits.shape[1]
        if not 1 <= classes <= MAX_CLASSES:
            raise ValueError(f"{classes} classes (1 .. {MAX_CLASSES})")
        if logits.dtype != torch.float32 or tuple(logits.shape) != (B, classes, layers * K):
            raise RuntimeError(f"class logits must be float32 [{B}, C, {layers * K}], got {tuple(logits.shape)} {logits.dtype}")
        logits = logits.detach().contiguous()
    use_iou = iou_cost is not None or want_iou
    if reg_cost is not None or use_iou:
        if boxes.dtype != torch.float32 or boxes.dim() != 3 or tuple(boxes.shape[:2]) != (B, layers * K) or boxes.shape[2] != gt_boxes.shape[1]:
            raise RuntimeError(f"decoded boxes must be float32 [{B}, {layers * K}, {gt_boxes.shape[1]}], got {tuple(boxes.shape)} {boxes.dtype}")
        boxes = boxes.detach().contiguous()
    if reg_cost is not None and pc_range is None:
        raise ValueError("BBoxBEVL1Cost needs train_cfg['point_cloud_range']")
    if not 1 <= K <= MAX_SIDE:
        raise ValueError(f"{K} proposals per layer (1 .. {MAX_SIDE})")
    cost = torch.empty((B, layers, K, bound), dtype=torch.float32, device=dev)
    iou = torch.empty((B, layers, K, bound), dtype=torch.float32, device=dev)
    num_gt = torch.empty(B * layers, dtype=torch.int32, device=dev)
    status = torch.empty(B * layers, dtype=torch.int32, device=dev)
    lib = _capi.load()
    with torch.cuda.device(dev):
        rc = lib.bevamd_match_costs(
            _capi.ptr(boxes if (reg_cost is not None or use_iou) else None), _capi.ptr(logits if mode else None), _capi.ptr(gt_boxes),
            _capi.ptr(gt_labels), _capi.ptr(offsets), gt_boxes.shape[0], gt_boxes.shape[1], B, layers, K, classes, bound, mode, float(w_cls),
            float(alpha), float(gamma), float(eps), 1 if reg_cost is not None else 0, float(reg_cost.weight) if reg_cost is not None else 0.0,
            1 if use_iou else 0, float(iou_cost.weight) if iou_cost is not None else 0.0,
            _capi.floats(list(pc_range)[:6]) if pc_range is not None else None, _capi.ptr(cost), _capi.ptr(iou), _capi.ptr(num_gt),
            _capi.ptr(status), _capi.stream_ptr(dev))
    _capi.check(rc, "match_costs")
    return cost, iou, num_gt, status


def _one_problem(gt_boxes, gt_labels):
    """A single sample's ground truth as the packed triple; (None, None) when it has no box (nothing to launch)."""
    G = gt_boxes.shape[0] if gt_boxes is not None else gt_labels.shape[0]
    if G == 0:
        return None, 0
    if G > MAX_BOXES:
        raise ValueError(f"{G} ground-truth boxes: at most {MAX_BOXES}")
    dev = (gt_boxes if gt_boxes is not None else gt_labels).device
    if gt_boxes is None:
        gt_boxes = torch.zeros((G, 7), dtype=torch.float32, device=dev)
    if gt_labels is None:
        gt_labels = torch.zeros(G, dtype=torch.int64, device=dev)
    return _pack([gt_boxes], [gt_labels], None)[:3], G


class FocalLossCost:
    """mmdet 2.x match_cost.py FocalLossCost: cls_pred [K, C] logits, gt_labels [G] -> [K, G]."""

    def __init__(self, weight=1.0, alpha=0.25, gamma=2, eps=1e-12):
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        _need_gpu(cls_pred, gt_labels)
        gt, G = _one_problem(None, gt_labels)
        if G == 0:
            return cls_pred.new_zeros((cls_pred.shape[0], 0))
        logits = cls_pred.detach().float().t().contiguous()[None]
        return _match_costs(None, logits, gt, 1, cls_pred.shape[0], G, cls_cost=self)[0][0, 0]


class ClassificationCost(FocalLossCost):
    """mmdet 2.x match_cost.py ClassificationCost: -softmax(cls_pred)[:, gt_labels] * weight."""

    def __init__(self, weight=1.0):
        self.weight = weight


class BBoxBEVL1Cost:
    """hungarian_assigner.py:13-25: L1 distance of the box centres normalised by the point cloud range."""

    def __init__(self, weight):
        self.weight = weight

    def __call__(self, bboxes, gt_bboxes, train_cfg):
        _need_gpu(bboxes, gt_bboxes)
        gt, G = _one_problem(gt_bboxes, None)
        if G == 0:
            return bboxes.new_zeros((bboxes.shape[0], 0))
        return _match_costs(bboxes.detach().float()[None], None, gt, 1, bboxes.shape[0], G, reg_cost=self,
                            pc_range=train_cfg["point_cloud_range"])[0][0, 0]


class IoU3DCost:
    """hungarian_assigner.py:28-35: -iou * weight."""

    def __init__(self, weight):
        self.weight = weight

    def __call__(self, iou):
        return -iou * self.weight


class BboxOverlaps3D:
    """mmdet3d's BboxOverlaps3D for LiDAR boxes: BaseInstance3DBoxes.overlaps (base_box3d.py:389-445), [N, 7|9] x [M, 7|9] -> [N, M]."""

    def __init__(self, coordinate="lidar"):
        if coordinate != "lidar":
            raise NotImplementedError(f"coordinate {coordinate!r}: the LiDAR box convention is served")
        self.coordinate = coordinate

    def __call__(self, bboxes1, bboxes2, mode="iou"):
        if mode != "iou":
            raise NotImplementedError(f"mode {mode!r}: 'iou' is served")
        _need_gpu(bboxes1, bboxes2)
        gt, G = _one_problem(bboxes2, None)
        if G == 0:
            return bboxes1.new_zeros((bboxes1.shape[0], 0))
        return _match_costs(bboxes1.detach().float()[None], None, gt, 1, bboxes1.shape[0], G, want_iou=True)[1][0, 0]


for _cls in (FocalLossCost, ClassificationCost, BBoxBEVL1Cost, IoU3DCost):
    register_everywhere("match_cost", _cls)
register_everywhere("iou_calculator", BboxOverlaps3D)


# ---- the assigner ----------------------------------------------------------------------------------------------------------------
class AssignResult:
    """mmdet 2.x AssignResult, the fields the head reads: gt_inds 0 for background, 1-based for matches."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


def _build(cfg, registry):
    return build_from_cfg(cfg, registry) if isinstance(cfg, dict) else cfg


class HungarianAssigner3D:
    """hungarian_assigner.py:82-142 with the costs and the solver on the device."""

    def __init__(self, cls_cost=dict(type="ClassificationCost", weight=1.0), reg_cost=dict(type="BBoxBEVL1Cost", weight=1.0),
                 iou_cost=dict(type="IoU3DCost", weight=1.0), iou_calculator=dict(type="BboxOverlaps3D")):
        self.cls_cost = _build(cls_cost, MATCH_COST)
        self.reg_cost = _build(reg_cost, MATCH_COST)
        self.iou_cost = _build(iou_cost, MATCH_COST)
        self.iou_calculator = _build(iou_calculator, IOU_CALCULATORS)
        if not isinstance(self.cls_cost, FocalLossCost) or not isinstance(self.reg_cost, BBoxBEVL1Cost) \
                or not isinstance(self.iou_cost, IoU3DCost) or not isinstance(self.iou_calculator, BboxOverlaps3D):
            raise NotImplementedError("HungarianAssigner3D serves FocalLossCost / ClassificationCost, BBoxBEVL1Cost, IoU3DCost and BboxOverlaps3D")

    def _solve(self, boxes, logits, gt, layers, K, bound, train_cfg):
        """-> (cost, iou, col4row [B * L, K], status_cost, status_lsa)."""
        cost, iou, num_gt, st_cost = _match_costs(boxes, logits, gt, layers, K, bound, self.cls_cost, self.reg_cost, self.iou_cost,
                                                  train_cfg["point_cloud_range"])
        col4row, st_lsa = linear_sum_assignment_batch(cost.view(-1, K, bound), None, num_gt)
        return cost, iou, col4row, st_cost, st_lsa

    def assign(self, bboxes, gt_bboxes, gt_labels, cls_pred, train_cfg):
        """bboxes [K, 7|9] decoded, gt_bboxes [G, 7|9], gt_labels [G], cls_pred [1, C, K] logits.  No host sync."""
        _need_gpu(bboxes, gt_bboxes, gt_labels, cls_pred)
        K, G = bboxes.shape[0], gt_bboxes.shape[0]
        gt_inds = bboxes.new_zeros(K, dtype=torch.long)
        labels = bboxes.new_full((K,), -1, dtype=torch.long)
        if G == 0 or K == 0:
            return AssignResult(G, gt_inds, None, labels=labels)
        gt, _ = _one_problem(gt_bboxes, gt_labels)
        _, iou, col4row, _, _ = self._solve(bboxes.detach().float()[None], cls_pred.detach().float(), gt, 1, K, G, train_cfg)
        col = col4row[0].long()
        pos = col >= 0
        safe = col.clamp(min=0)
        gt_inds = torch.where(pos, col + 1, gt_inds)
        labels = torch.where(pos, gt_labels.long()[safe], labels)
        overlaps = torch.where(pos, iou[0, 0].gather(1, safe[:, None])[:, 0], torch.zeros_like(iou[0, 0, :, 0]))
        return AssignResult(G, gt_inds, overlaps, labels=labels)


class HeuristicAssigner3D:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("HeuristicAssigner is not served: only HungarianAssigner3D runs on the device")


register_everywhere("bbox_assigner", HungarianAssigner3D)
register_everywhere("bbox_assigner", HeuristicAssigner3D)
register_everywhere("bbox_assigner", HeuristicAssigner3D, name="HeuristicAssigner")


# ---- get_targets -----------------------------------------------------------------------------------------------------------------
def _pos_weight(train_cfg):
    w = train_cfg["pos_weight"] if "pos_weight" in train_cfg else -1
    if float(w) != int(w):
        raise ValueError(f"pos_weight {w}: label_weights is an int64 tensor (the reference truncates a fractional weight silently)")
    return int(w)


def _coder_consts(coder):
    return (float(coder.pc_range[0]), float(coder.pc_range[1]), float(coder.out_size_factor * coder.voxel_size[0]),
            float(coder.out_size_factor * coder.voxel_size[1]))


def _assign_targets(col4row, iou, st_cost, st_lsa, gt, B, layers, K, bound, num_classes, coder, pos_weight):
    gt_boxes, gt_labels, offsets = gt
    dev = gt_boxes.device
    P, code = layers * K, int(coder.code_size)
    if code not in (8, 10) or (code == 10 and gt_boxes.shape[1] != 9):
        raise ValueError(f"code_size {code} with {gt_boxes.shape[1]}-column boxes (8, or 10 with 9 columns)")
    labels = torch.empty((B, P), dtype=torch.int64, device=dev)
    label_weights = torch.empty((B, P), dtype=torch.int64, device=dev)
    bbox_targets = torch.empty((B, P, code), dtype=torch.float32, device=dev)
    bbox_weights = torch.empty((B, P, code), dtype=torch.float32, device=dev)
    ious = torch.empty((B, P), dtype=torch.float32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    summary = torch.empty(2, dtype=torch.int32, device=dev)              # num_pos, and the bits of matched_ious: ONE read-back
    consts = (_capi.ctypes.c_double * 4)(*_coder_consts(coder))
    lib = _capi.load()
    with torch.cuda.device(dev):
        rc = lib.bevamd_transfusion_assign_targets(
            _capi.ptr(col4row), _capi.ptr(iou), _capi.ptr(st_cost), _capi.ptr(st_lsa), _capi.ptr(gt_boxes), _capi.ptr(gt_labels),
            _capi.ptr(offsets), gt_boxes.shape[0], gt_boxes.shape[1], B, layers, K, bound, int(num_classes), code, pos_weight, consts,
            _capi.ptr(labels), _capi.ptr(label_weights), _capi.ptr(bbox_targets), _capi.ptr(bbox_weights), _capi.ptr(ious),
            _capi.ptr(flags), _capi.c_void_p(summary.data_ptr()), _capi.c_void_p(summary.data_ptr() + 4), _capi.stream_ptr(dev))
    _capi.check(rc, "transfusion_assign_targets")
    return labels, label_weights, bbox_targets, bbox_weights, ious, flags, summary


def transfusion_get_targets(gt_bboxes_3d, gt_labels_3d, preds_dict, bbox_coder, assigner, train_cfg, num_proposals, num_classes,
                            num_decoder_layers=1, auxiliary=True, max_boxes_per_sample=None, sync=True):
    """get_targets of TransFusionHead (transfusion.py:357-585).  preds_dict: the head's dict (or the reference's list whose first
    entry it is) of heatmap [B, C, P] logits, center [B, 2, P], height [B, 1, P], dim [B, 3, P], rot [B, 2, P], optional vel
    [B, 2, P], with P = num_proposals * (num_decoder_layers if auxiliary else 1): every layer is assigned on its own against the
    same ground truth.  Ground truth in both forms of the head targets (lists, or the packed triple with gt_labels_3d=None and
    max_boxes_per_sample).  train_cfg: point_cloud_range, pos_weight and what `transfusion_heatmap_targets` reads.

    sync=True : (labels [B, P] int64, label_weights [B, P] int64, bbox_targets [B, P, code_size], bbox_weights, ious [B, P],
                num_pos int, matched_ious float, heatmap [B, C, H, W]), as the reference returns them: one 8-byte read-back.
    sync=False: the same with num_pos (int32) and matched_ious (fp32) as 0-dim device tensors, and a ninth entry flags [B] int32
                (the OR of the STATUS_* bits of the sample: it is then all negative); no host sync, capturable in a graph."""
    if not isinstance(assigner, HungarianAssigner3D):
        raise NotImplementedError(f"assigner {type(assigner).__name__}: only HungarianAssigner3D is served")
    preds = preds_dict[0] if isinstance(preds_dict, (list, tuple)) else preds_dict
    heat = preds["heatmap"]
    K = int(num_proposals)
    layers = int(num_decoder_layers) if auxiliary else 1
    pos_weight = _pos_weight(train_cfg)
    if not 1 <= K <= MAX_SIDE or layers < 1:
        raise ValueError(f"num_proposals {K} (1 .. {MAX_SIDE}) in {layers} layers")
    _need_gpu(heat)
    if heat.dim() != 3 or heat.shape[1] != num_classes or heat.shape[2] != layers * K:
        raise RuntimeError(f"heatmap must be [B, {num_classes}, {layers * K}], got {tuple(heat.shape)}")
    gt_boxes, gt_labels, offsets, B, bound = _pack(gt_bboxes_3d, gt_labels_3d, max_boxes_per_sample)
    if B != heat.shape[0]:
        raise RuntimeError(f"{B} samples of ground truth for {heat.shape[0]} of predictions")
    vel = preds.get("vel")
    if (9 if vel is not None else 7) != gt_boxes.shape[1]:
        raise RuntimeError(f"ground truth has {gt_boxes.shape[1]} columns, the predictions decode to {9 if vel is not None else 7}")
    from .heads import _decode_device                                      # heads re-exports this module

    boxes = _decode_device(heat, preds["rot"], preds["dim"], preds["center"], preds["height"], vel, bbox_coder, layers * K)[0]
    gt = (gt_boxes, gt_labels, offsets)
    _, iou, col4row, st_cost, st_lsa = assigner._solve(boxes, heat.detach().contiguous(), gt, layers, K, bound, train_cfg)
    labels, label_weights, bbox_targets, bbox_weights, ious, flags, summary = _assign_targets(
        col4row, iou, st_cost, st_lsa, gt, B, layers, K, bound, num_classes, bbox_coder, pos_weight)
    heatmap = transfusion_heatmap_targets(gt, None, num_classes, train_cfg, max_boxes_per_sample=bound)
    if not sync:
        return (labels, label_weights, bbox_targets, bbox_weights, ious, summary[0], summary[1:].view(torch.float32)[0], heatmap, flags)
    host = summary.cpu().numpy()
    return (labels, label_weights, bbox_targets, bbox_weights, ious, int(host[0]), float(host[1:].view(np.float32)[0]), heatmap)


# ---- host mirror (tests only) ----------------------------------------------------------------------------------------------------
def _costs_host(boxes, logits, gt_boxes, gt_labels, cls, reg_weight, iou_weight, pc_range, bev_overlap):
    """One problem in the kernels' arithmetic: boxes [K, 7|9], logits [C, K], gt_boxes [G, 7|9], gt_labels [G]; cls = ("focal",
    weight, alpha, gamma, eps) or ("softmax", weight); bev_overlap(xyxyr_a [K, 5], xyxyr_b [G, 5]) -> [K, G] fp32 BEV overlap
    areas (the tests pass the oracle's).  -> (cost, iou) [K, G] fp32."""
    f = np.float32
    boxes, gt_boxes = np.asarray(boxes, f), np.asarray(gt_boxes, f)
    x = np.asarray(logits, f).T.astype(np.float64)[:, gt_labels]                       # [K, G]
    with np.errstate(all="ignore"):
        if cls[0] == "focal":
            _, w, alpha, gamma, eps = cls
            p = (1.0 / (1.0 + np.exp(-x))).astype(f)
            power = (lambda t: t * t) if gamma == 2 else (lambda t: np.power(t.astype(np.float64), gamma).astype(f))
            neg = -np.log((f(1) - p + f(eps)).astype(np.float64)).astype(f) * f(1 - alpha) * power(p)
            pos = -np.log((p + f(eps)).astype(np.float64)).astype(f) * f(alpha) * power(f(1) - p)
            cost = (pos - neg) * f(w)
        else:
            full = np.asarray(logits, f).T.astype(np.float64)
            e = np.exp(full - full.max(1, keepdims=True))
            cost = -(e / e.sum(1, keepdims=True)).astype(f)[:, gt_labels] * f(cls[1])
        pc = np.asarray(pc_range, f)
        start, span = pc[0:2], pc[3:5] - pc[0:2]
        a, g = (boxes[:, :2] - start) / span, (gt_boxes[:, :2] - start) / span
        cost = cost + (np.abs(a[:, None, 0] - g[None, :, 0]) + np.abs(a[:, None, 1] - g[None, :, 1])) * f(reg_weight)

        def xyxyr(t):
            return np.stack([t[:, 0] - t[:, 3] / f(2), t[:, 1] - t[:, 4] / f(2), t[:, 0] + t[:, 3] / f(2), t[:, 1] + t[:, 4] / f(2), t[:, 6]], 1)

        bev = np.asarray(bev_overlap(xyxyr(boxes), xyxyr(gt_boxes)), f)
        h = np.maximum(np.minimum((boxes[:, 2] + boxes[:, 5])[:, None], (gt_boxes[:, 2] + gt_boxes[:, 5])[None, :])
                       - np.maximum(boxes[:, 2][:, None], gt_boxes[:, 2][None, :]), f(0))
        o = bev * h
        va, vb = boxes[:, 3] * boxes[:, 4] * boxes[:, 5], gt_boxes[:, 3] * gt_boxes[:, 4] * gt_boxes[:, 5]
        iou = o / np.maximum(va[:, None] + vb[None, :] - o, f(1e-8))
        cost = cost + (-iou) * f(iou_weight)
    assert cost.dtype == np.float32 and iou.dtype == np.float32
    return cost, iou


def _targets_host(boxes, logits, gt_boxes, gt_labels, offsets, layers, K, cls, reg_weight, iou_weight, pc_range, coder_consts,
                  num_classes, code_size, pos_weight, bev_overlap=None, col4row=None, iou=None, max_boxes_per_sample=MAX_BOXES):
    """The whole chain on host arrays: boxes [B, L * K, 7|9] decoded, logits [B, C, L * K]; scipy solves each (sample, layer)
    problem, unless `col4row` [B * L, K] and `iou` [B, L, K, Gmax] are given (targets re-derived from a device assignment).
    -> dict(cost, iou: per problem [K, G] lists; col4row [B * L, K]; labels, label_weights, bbox_targets, bbox_weights, ious, flags,
    num_pos, matched_ious)."""
    from scipy.optimize import linear_sum_assignment

    f = np.float32
    boxes, gt_boxes = np.asarray(boxes, f), np.asarray(gt_boxes, f)
    gt_labels, offsets = np.asarray(gt_labels, np.int64), np.asarray(offsets, np.int64)
    B, P = len(offsets) - 1, layers * K
    pc0, pc1, div0, div1 = (f(v) for v in coder_consts)
    out = dict(cost=[], iou=[], col4row=np.full((B * layers, K), -1, np.int32), labels=np.full((B, P), num_classes, np.int64),
               label_weights=np.ones((B, P), np.int64), bbox_targets=np.zeros((B, P, code_size), f),
               bbox_weights=np.zeros((B, P, code_size), f), ious=np.zeros((B, P), f), flags=np.zeros(B, np.int32))
    means, num_pos = [], 0
    for b in range(B):
        first, G = offsets[b], offsets[b + 1] - offsets[b]
        if G > max_boxes_per_sample:
            out["flags"][b] = STATUS_OVERFLOW
            G = 0
        gb, gl = gt_boxes[first:first + G], gt_labels[first:first + G]
        if G and ((gl < 0) | (gl >= num_classes)).any():
            out["flags"][b] |= STATUS_LABEL | STATUS_NONFINITE
        rows = []
        for l in range(layers):
            sl = slice(l * K, (l + 1) * K)
            if col4row is not None:
                c4r, pair_iou = np.asarray(col4row)[b * layers + l], np.asarray(iou)[b, l]
            elif G == 0 or out["flags"][b]:
                c4r, pair_iou = np.full(K, -1, np.int32), np.zeros((K, 0), f)
            else:
                cost, pair_iou = _costs_host(boxes[b, sl], np.asarray(logits, f)[b][:, sl], gb, gl, cls, reg_weight, iou_weight, pc_range,
                                             bev_overlap)
                out["cost"].append(cost)
                out["iou"].append(pair_iou)
                if not np.isfinite(cost).all():
                    out["flags"][b] |= STATUS_NONFINITE
                    c4r = np.full(K, -1, np.int32)
                else:
                    r, c = linear_sum_assignment(cost)
                    c4r = np.full(K, -1, np.int32)
                    c4r[r] = c
            rows.append((c4r, pair_iou))
        total, n = f(0), 0
        for l, (c4r, pair_iou) in enumerate(rows):
            out["col4row"][b * layers + l] = -1 if out["flags"][b] else c4r
            if out["flags"][b]:
                continue
            for k in np.nonzero(c4r >= 0)[0]:
                g, p = c4r[k], l * K + k
                box = gb[g]
                t = np.zeros(code_size, f)
                t[0], t[1] = (box[0] - pc0) / div0, (box[1] - pc1) / div1
                t[2] = box[2] + box[5] * f(0.5)
                t[3:6] = np.log(box[3:6].astype(np.float64)).astype(f)
                t[6], t[7] = f(np.sin(np.float64(box[6]))), f(np.cos(np.float64(box[6])))
                if code_size == 10:
                    t[8:10] = box[7:9]
                out["labels"][b, p] = gl[g]
                out["label_weights"][b, p] = pos_weight if pos_weight > 0 else 1
                out["bbox_targets"][b, p], out["bbox_weights"][b, p] = t, 1
                out["ious"][b, p] = min(max(pair_iou[k, g], f(0)), f(1))
                total, n = total + np.float64(out["ious"][b, p]), n + 1
        means.append(float(f(total / max(n, 1))))
        num_pos += n
    out["num_pos"], out["matched_ious"] = num_pos, float(f(np.mean(means)))
    return out
