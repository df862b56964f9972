"""The losses of the two detection heads on the device (reference: TransFusionHead.loss, mmdet3d/models/heads/bbox/
transfusion.py:587-713; CenterHead.loss, centerpoint.py:584-634; both `clip_sigmoid`s; mmdet 2.x GaussianFocalLoss, FocalLoss
(py_sigmoid_focal_loss) and L1Loss, which the reference imports), over csrc/ext/head_losses.hip.  `heads` re-exports everything here.

  * `transfusion_loss`: the reference's loss dict from the head's predictions and what `transfusion_get_targets` returns, in either
    sync form: three launches forward, two backward, no host sync with the sync=False targets;
  * `centerhead_loss`: the per-task dict from the task predictions and `centerhead_get_targets`' tuple: three launches forward, three
    backward, for any number of tasks;
  * the op functions under them (`gaussian_focal_forward / _backward`, `transfusion_layer_losses_forward / _backward`,
    `centerhead_box_loss_forward / _backward`, `transfusion_loss_forward / _backward`, `centerhead_loss_forward / _backward`): no
    autograd, capturable in a graph;
  * `GaussianFocalLoss`, `FocalLoss`, `L1Loss`: mmdet's modules (`registry.LOSSES`).

Inputs are fp32 (the reference's `force_fp32`): the caller widens fp16.  Device tensors go through the library or raise; host
tensors run `_losses_host`, the reference's formulation in torch ops, which is also the tests' mirror.

Differences from the reference, on purpose: `centerhead_loss` does not overwrite `preds_dict[0]["heatmap"]` with its sigmoid (the
reference's `clip_sigmoid` works in place); the `on_the_image_mask` branch of TransFusionHead.loss (transfusion.py:608-611, an
attribute nothing in the reference sets) is not served; `reduction="none"`, softmax focal loss and a per-element `weight` of
GaussianFocalLoss raise; cell terms are evaluated in double and summed in fp64, so a loss lies nearer the reference's float64 run
than its own fp32 run does.
"""
import ctypes

import torch
from torch import nn

from . import _capi
from .registry import LOSSES, build_from_cfg, register_everywhere

__all__ = ["transfusion_loss", "centerhead_loss", "GaussianFocalLoss", "FocalLoss", "L1Loss", "LOSSES", "head_loss_plan",
           "gaussian_focal_forward", "gaussian_focal_backward", "transfusion_layer_losses_forward", "transfusion_layer_losses_backward",
           "centerhead_box_loss_forward", "centerhead_box_loss_backward", "transfusion_loss_forward", "transfusion_loss_backward",
           "centerhead_loss_forward", "centerhead_loss_backward"]

MAX_MAPS = 16
MAX_SLOTS = 1024
PIECES = ("center", "height", "dim", "rot", "vel")            # TransFusion code columns 0-1, 2, 3-5, 6-7, 8-9
CH_PIECES = ("reg", "height", "dim", "rot", "vel")
_WIDTH = (2, 1, 3, 2, 2)
_DEFAULT_CODE_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2)


# ---- host formulation (the reference's torch ops; the tests' mirror) ----------------------------------------------------------------
def _clip_sigmoid(x, eps=1e-4):
    return torch.clamp(x.sigmoid(), min=eps, max=1 - eps)


def _gaussian_focal_host(pred, target, alpha=2.0, gamma=4.0):
    """mmdet 2.x gaussian_focal_loss, element-wise."""
    eps = 1e-12
    pos_weights = target.eq(1)
    neg_weights = (1 - target).pow(gamma)
    pos_loss = -(pred + eps).log() * (1 - pred).pow(alpha) * pos_weights
    neg_loss = -(1 - pred + eps).log() * pred.pow(alpha) * neg_weights
    return pos_loss + neg_loss


def _sigmoid_focal_host(pred, target, weight, gamma=2.0, alpha=0.25):
    """mmdet 2.x py_sigmoid_focal_loss before the reduction: pred [N, C] logits, target [N] with C for background, weight [N]."""
    onehot = torch.nn.functional.one_hot(target, pred.shape[1] + 1)[:, :pred.shape[1]].type_as(pred)
    s = pred.sigmoid()
    pt = (1 - s) * onehot + s * (1 - onehot)
    focal = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, onehot, reduction="none") * focal
    return loss * weight.type_as(pred).view(-1, 1)


def _losses_host(head, *args, **kwargs):
    """The reference's formulation in torch ops, in the dtype of the predictions (fp32, or float64 for the tests' mirror)."""
    return {"transfusion": _transfusion_host, "centerhead": _centerhead_host}[head](*args, **kwargs)


def _transfusion_host(preds, targets, K, C, layers, code_weights, cls_cfg, box_cfg, heat_cfg):
    labels, label_weights, bbox_targets, bbox_weights, _, num_pos, matched_ious, heatmap = targets[:8]
    dense = preds["dense_heatmap"]
    dt = dense.dtype
    out = {}
    heat_avg = torch.clamp(heatmap.eq(1).to(dt).sum(), min=1)
    out["loss_heatmap"] = heat_cfg["loss_weight"] * (
        _gaussian_focal_host(_clip_sigmoid(dense), heatmap.to(dt), heat_cfg["alpha"], heat_cfg["gamma"]).sum() / heat_avg)
    avg = torch.clamp(torch.as_tensor(num_pos).to(dt), min=1)
    for i in range(layers):
        prefix = "layer_-1" if i == layers - 1 else f"layer_{i}"
        sl = slice(i * K, (i + 1) * K)
        score = preds["heatmap"][..., sl].permute(0, 2, 1).reshape(-1, C)
        cls = _sigmoid_focal_host(score, labels[..., sl].reshape(-1), label_weights[..., sl].reshape(-1), cls_cfg["gamma"], cls_cfg["alpha"])
        out[f"{prefix}_loss_cls"] = cls_cfg["loss_weight"] * (cls.sum() / avg)
        names = PIECES if "vel" in preds and preds["vel"] is not None else PIECES[:4]
        pred = torch.cat([preds[n][..., sl] for n in names], dim=1).permute(0, 2, 1)
        bw = bbox_weights[:, sl, :].to(dt)
        reg_weights = bw * bw.new_tensor(code_weights[:pred.shape[2]])
        out[f"{prefix}_loss_bbox"] = box_cfg["loss_weight"] * (((pred - bbox_targets[:, sl, :].to(dt)).abs() * reg_weights).sum() / avg)
    out["matched_ious"] = torch.as_tensor(matched_ious).to(dt).detach()
    return out


def _centerhead_host(preds_dicts, targets, code_weights, cls_cfg, box_cfg):
    heatmaps, anno_boxes, inds, masks = targets[:4]
    out = {}
    for t, pd in enumerate(preds_dicts):
        pd = pd[0] if isinstance(pd, (list, tuple)) else pd
        dt = pd["heatmap"].dtype
        heat = heatmaps[t].to(dt)
        avg = torch.clamp(heat.eq(1).to(dt).sum(), min=1)
        out[f"heatmap/task{t}"] = cls_cfg["loss_weight"] * (
            _gaussian_focal_host(_clip_sigmoid(pd["heatmap"]), heat, cls_cfg["alpha"], cls_cfg["gamma"]).sum() / avg)
        target_box = anno_boxes[t].to(dt)
        anno = torch.cat([pd[n] for n in CH_PIECES], dim=1)
        num = masks[t].float().sum()                                        # fp32 in the reference whatever the predictions' dtype
        pred = anno.permute(0, 2, 3, 1).contiguous()
        pred = pred.view(pred.size(0), -1, pred.size(3))
        ind = inds[t].unsqueeze(2).expand(inds[t].size(0), inds[t].size(1), pred.size(2))
        pred = pred.gather(1, ind)
        mask = masks[t].unsqueeze(2).expand_as(target_box).float()           # ... and so are the weights: fp32(mask * code_weights)
        mask = mask * (~torch.isnan(target_box)).float()
        weights = mask * mask.new_tensor(code_weights)
        out[f"bbox/task{t}"] = box_cfg["loss_weight"] * (((pred - target_box).abs() * weights).sum() / (num + 1e-4))
    return out


# ---- op functions (device) ------------------------------------------------------------------------------------------------------------
def _f32(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the head-loss ops need GPU tensors")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32 (widen fp16 first, as the reference's force_fp32 does), got {t.dtype}")
    return t.contiguous()


def _cells(values):
    return (ctypes.c_longlong * len(values))(*[int(v) for v in values])


def head_loss_plan(cells):
    """(workgroups, cells per workgroup pass) of the dense kernels for a map of `cells` cells.  Host only."""
    plan = (ctypes.c_int * 2)()
    _capi.check(_capi.load().bevamd_head_loss_plan(int(cells), plan), "head_loss_plan")
    return int(plan[0]), int(plan[1])


def _avg_pointers(avg, T):
    if avg is None:
        return None, None
    avg = [None if a is None else _f32(a, "avg").reshape(1) for a in avg]
    if len(avg) != T:
        raise ValueError(f"{len(avg)} avg entries for {T} maps")
    return avg, _capi.pointers(avg)


def _gf_maps(preds, targets):
    if not 1 <= len(preds) <= MAX_MAPS or len(preds) != len(targets):
        raise ValueError(f"{len(preds)} prediction maps and {len(targets)} targets (1 .. {MAX_MAPS}, equal)")
    preds = [_f32(p, "pred") for p in preds]
    targets = [_f32(t, "target") for t in targets]
    for p, t in zip(preds, targets):
        if p.numel() != t.numel() or p.numel() == 0:
            raise RuntimeError(f"a prediction map of {tuple(p.shape)} for a target of {tuple(t.shape)}")
    return preds, targets


def gaussian_focal_forward(preds, targets, alpha=2.0, gamma=4.0, loss_weight=1.0, pred_is_logit=True, avg=None, out=None):
    """Dense Gaussian focal loss of up to 16 maps: preds / targets lists of equal-sized fp32 tensors; avg: None, or a list with a
    device scalar (or None) per map.  -> (loss [T], num_pos [T]) fp32; `out`: a [T] fp32 tensor to write the loss to."""
    preds, targets = _gf_maps(preds, targets)
    T, dev = len(preds), preds[0].device
    avg, avg_ptr = _avg_pointers(avg, T)
    width = head_loss_plan(max(p.numel() for p in preds))[0]
    partials = torch.empty(T * width * 2, dtype=torch.float64, device=dev)
    loss = torch.empty(T, dtype=torch.float32, device=dev) if out is None else out
    num_pos = torch.empty(T, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_gaussian_focal_forward(
            _capi.pointers(preds), _capi.pointers(targets), _cells([p.numel() for p in preds]), T, 1 if pred_is_logit else 0, float(alpha),
            float(gamma), float(loss_weight), avg_ptr, _capi.ptr(partials), _capi.ptr(loss), _capi.ptr(num_pos), _capi.stream_ptr(dev))
    _capi.check(rc, "gaussian_focal_forward")
    return loss, num_pos


def gaussian_focal_backward(preds, targets, num_pos, grad_out, alpha=2.0, gamma=4.0, loss_weight=1.0, pred_is_logit=True, avg=None,
                            out=None):
    """-> the list of d loss[t] / d preds[t] * grad_out[t], each in the shape of its map (`out`: contiguous fp32 tensors to write
    them to).  num_pos: the forward's."""
    preds, targets = _gf_maps(preds, targets)
    T, dev = len(preds), preds[0].device
    avg, avg_ptr = _avg_pointers(avg, T)
    grads = [torch.empty_like(p) for p in preds] if out is None else list(out)
    if any(g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != p.numel() for g, p in zip(grads, preds)):
        raise RuntimeError("out: one contiguous float32 tensor of its map's size per map")
    grad_out = _f32(grad_out, "grad_out")
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_gaussian_focal_backward(
            _capi.pointers(preds), _capi.pointers(targets), _cells([p.numel() for p in preds]), T, 1 if pred_is_logit else 0, float(alpha),
            float(gamma), float(loss_weight), avg_ptr, _capi.ptr(_f32(num_pos, "num_pos")), _capi.ptr(grad_out), _capi.pointers(grads),
            _capi.stream_ptr(dev))
    _capi.check(rc, "gaussian_focal_backward")
    return grads


def _layer_args(scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights, num_pos, avg_cls, avg_box, layers,
                cls_cfg, box_cfg):
    """The argument list both layer entry points share (up to box_weight), the tensors it points into, and (B, C, L, K, D)."""
    keep, B, C, D, P = [], None, 0, 0, None
    wdtype = 0
    if scores is not None:
        scores = _f32(scores, "scores")
        B, C, P = scores.shape
        labels = labels.contiguous()
        label_weights = label_weights.contiguous()
        if labels.dtype != torch.int64 or tuple(labels.shape) != (B, P) or tuple(label_weights.shape) != (B, P):
            raise RuntimeError(f"labels int64 [{B}, {P}] and label_weights [{B}, {P}] expected, got {labels.dtype} {tuple(labels.shape)}, "
                               f"{tuple(label_weights.shape)}")
        wdtype = {torch.float32: 0, torch.int64: 2}.get(label_weights.dtype, -1)
        keep += [scores, labels, label_weights]
    packed = False
    if pieces is not None:
        packed = not isinstance(pieces, (list, tuple))
        pieces = [_f32(pieces, "pred")] + [None] * 4 if packed else [None if p is None else _f32(p, "box piece") for p in pieces]
        bbox_targets, bbox_weights = _f32(bbox_targets, "bbox_targets"), _f32(bbox_weights, "bbox_weights")
        Bb, Pb, D = bbox_targets.shape
        if (B is not None and (B, P) != (Bb, Pb)) or bbox_weights.shape != bbox_targets.shape:
            raise RuntimeError(f"bbox_targets / bbox_weights {tuple(bbox_targets.shape)} / {tuple(bbox_weights.shape)} for [{B}, {P}] rows")
        B, P = Bb, Pb
        if packed:
            if tuple(pieces[0].shape) != (B, P, D):
                raise RuntimeError(f"a packed prediction is [{B}, {P}, {D}], got {tuple(pieces[0].shape)}")
        else:
            for p, w in zip(pieces, _WIDTH):
                if p is not None and tuple(p.shape) != (B, w, P):
                    raise RuntimeError(f"a box piece of {tuple(p.shape)}: [{B}, {w}, {P}] expected")
        keep += pieces + [bbox_targets, bbox_weights]
    else:
        pieces = [None] * 5
    if P is None or P % layers:
        raise ValueError(f"{P} proposals in {layers} layers")
    for t in (num_pos, avg_cls, avg_box):
        if t is not None and not t.is_cuda:
            raise RuntimeError("num_pos / avg are device scalars")
    if num_pos is not None and num_pos.dtype != torch.int32:
        raise RuntimeError(f"num_pos must be int32, got {num_pos.dtype}")
    cw = None if code_weights is None or pieces[0] is None else _capi.floats(list(code_weights)[:D])
    if cw is not None and len(cw) != D:
        raise ValueError(f"{len(cw)} code weights for {D} columns")
    args = [_capi.ptr(scores), _capi.ptr(labels if scores is not None else None), _capi.ptr(label_weights if scores is not None else None),
            wdtype] + [_capi.ptr(p) for p in pieces] + [
        _capi.ptr(bbox_targets if pieces[0] is not None else None), _capi.ptr(bbox_weights if pieces[0] is not None else None), cw,
        _capi.ptr(num_pos), _capi.ptr(None if avg_cls is None else _f32(avg_cls, "avg")), _capi.ptr(None if avg_box is None else _f32(avg_box, "avg")),
        B, C, layers, P // layers, D, float(cls_cfg["alpha"]), float(cls_cfg["gamma"]), float(cls_cfg["loss_weight"]), float(box_cfg["loss_weight"])]
    return args, keep, scores, pieces, packed


_CLS = dict(alpha=0.25, gamma=2.0, loss_weight=1.0)
_BOX = dict(loss_weight=0.25)
_HEAT = dict(alpha=2.0, gamma=4.0, loss_weight=1.0)


def transfusion_layer_losses_forward(scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights, num_pos, layers=1,
                                     cls_cfg=_CLS, box_cfg=_BOX, avg_cls=None, avg_box=None, out_cls=None, out_box=None):
    """Per decoder layer: the sigmoid focal loss of scores [B, C, L * K] (None: left out) and the L1 of the box pieces (a list
    center, height, dim, rot, vel-or-None of [B, c, L * K] tensors, ONE packed [B, P, D] tensor, or None).  num_pos: device int32
    scalar (avg = max(num_pos, 1)) unless avg_cls / avg_box, device fp32 scalars, are given.  -> (loss_cls [L], loss_box [L])."""
    args, keep, scores, pieces, _ = _layer_args(scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights, num_pos,
                                               avg_cls, avg_box, layers, cls_cfg, box_cfg)
    dev = keep[0].device
    loss_cls = None if scores is None else (torch.empty(layers, dtype=torch.float32, device=dev) if out_cls is None else out_cls)
    loss_box = None if pieces[0] is None else (torch.empty(layers, dtype=torch.float32, device=dev) if out_box is None else out_box)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_transfusion_layer_losses_forward(*args, _capi.ptr(loss_cls), _capi.ptr(loss_box), _capi.stream_ptr(dev))
    _capi.check(rc, "transfusion_layer_losses_forward")
    return loss_cls, loss_box


def transfusion_layer_losses_backward(scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights, num_pos, grad_cls,
                                      grad_box, layers=1, cls_cfg=_CLS, box_cfg=_BOX, avg_cls=None, avg_box=None):
    """-> (grad_scores or None, the list of box-piece gradients (None where the piece is), or the packed gradient, or None)."""
    args, keep, scores, pieces, packed = _layer_args(scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights,
                                                    num_pos, avg_cls, avg_box, layers, cls_cfg, box_cfg)
    dev = keep[0].device
    grad_scores = None if scores is None else torch.empty_like(scores)
    grads = [None if p is None else torch.empty_like(p) for p in pieces]
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_transfusion_layer_losses_backward(
            *args, _capi.ptr(None if scores is None else _f32(grad_cls, "grad_cls")),
            _capi.ptr(None if pieces[0] is None else _f32(grad_box, "grad_box")), _capi.ptr(grad_scores), *[_capi.ptr(g) for g in grads],
            _capi.stream_ptr(dev))
    _capi.check(rc, "transfusion_layer_losses_backward")
    if pieces[0] is None:
        return grad_scores, None
    return grad_scores, (grads[0] if packed else grads)


def _ch_args(maps, inds, anno_boxes, masks, code_weights, loss_weight):
    T = len(maps)
    if not 1 <= T <= MAX_MAPS or not (len(inds) == len(anno_boxes) == len(masks) == T):
        raise ValueError(f"{T} tasks (1 .. {MAX_MAPS}) with {len(inds)} / {len(anno_boxes)} / {len(masks)} target entries")
    flat = [_f32(m, "regression map") for task in maps for m in task]
    B, _, H, W = flat[0].shape
    M = inds[0].shape[1]
    for t in range(T):
        for m, w in zip(flat[5 * t:5 * t + 5], _WIDTH):
            if tuple(m.shape) != (B, w, H, W):
                raise RuntimeError(f"task {t}: a regression map of {tuple(m.shape)}, [{B}, {w}, {H}, {W}] expected")
    inds = [i.contiguous() for i in inds]
    masks = [m.contiguous() for m in masks]
    anno = [_f32(a, "anno_box") for a in anno_boxes]
    for i, m, a in zip(inds, masks, anno):
        if i.dtype != torch.int64 or m.dtype not in (torch.uint8, torch.bool) or tuple(i.shape) != (B, M) or tuple(m.shape) != (B, M) \
                or tuple(a.shape) != (B, M, 10) or not (i.is_cuda and m.is_cuda):
            raise RuntimeError(f"ind int64 [{B}, {M}], mask uint8 [{B}, {M}] and anno_box [{B}, {M}, 10] device tensors expected")
    if len(code_weights) != 10:
        raise ValueError(f"{len(code_weights)} code weights (10)")
    args = [_capi.pointers(flat), _capi.pointers(inds), _capi.pointers(anno), _capi.pointers(masks), T, B, M, H * W,
            _capi.floats(code_weights), float(loss_weight)]
    return args, flat, (inds, masks, anno), T


def centerhead_box_loss_forward(maps, inds, anno_boxes, masks, code_weights, loss_weight=0.25, out=None):
    """maps: per task the five maps (reg, height, dim, rot, vel) [B, c, H, W], read only at inds[t] [B, M].  -> (loss [T], avg [T])."""
    args, flat, keep, T = _ch_args(maps, inds, anno_boxes, masks, code_weights, loss_weight)
    dev = flat[0].device
    loss = torch.empty(T, dtype=torch.float32, device=dev) if out is None else out
    avg = torch.empty(T, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_centerhead_box_loss_forward(*args, _capi.ptr(loss), _capi.ptr(avg), _capi.stream_ptr(dev))
    _capi.check(rc, "centerhead_box_loss_forward")
    return loss, avg


def centerhead_box_loss_backward(maps, inds, anno_boxes, masks, code_weights, avg, grad_out, loss_weight=0.25):
    """-> per task the list of the five gradient maps; avg: the forward's."""
    args, flat, keep, T = _ch_args(maps, inds, anno_boxes, masks, code_weights, loss_weight)
    dev = flat[0].device
    grads = [torch.empty_like(m) for m in flat]
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_centerhead_box_loss_backward(*args, _capi.ptr(_f32(avg, "avg")), _capi.ptr(_f32(grad_out, "grad_out")),
                                                              _capi.pointers(grads), _capi.stream_ptr(dev))
    _capi.check(rc, "centerhead_box_loss_backward")
    return [grads[5 * t:5 * t + 5] for t in range(T)]


def transfusion_loss_forward(dense, heatmap, scores, labels, label_weights, pieces, bbox_targets, bbox_weights, num_pos, layers,
                             code_weights=_DEFAULT_CODE_WEIGHTS, cls_cfg=_CLS, box_cfg=_BOX, heat_cfg=_HEAT):
    """All losses of TransFusionHead.loss: 3 launches.  -> (losses [1 + 2 L] fp32 = loss_heatmap, loss_cls per layer, loss_bbox per
    layer; heat_pos [1] fp32: the count of heatmap == 1, which the backward reads)."""
    losses = torch.empty(1 + 2 * layers, dtype=torch.float32, device=dense.device)
    _, heat_pos = gaussian_focal_forward([dense], [heatmap], heat_cfg["alpha"], heat_cfg["gamma"], heat_cfg["loss_weight"], out=losses[:1])
    transfusion_layer_losses_forward(scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights, num_pos, layers,
                                     cls_cfg, box_cfg, out_cls=losses[1:1 + layers], out_box=losses[1 + layers:])
    return losses, heat_pos


def transfusion_loss_backward(dense, heatmap, scores, labels, label_weights, pieces, bbox_targets, bbox_weights, num_pos, heat_pos,
                              grad_losses, layers, code_weights=_DEFAULT_CODE_WEIGHTS, cls_cfg=_CLS, box_cfg=_BOX, heat_cfg=_HEAT):
    """2 launches.  grad_losses [1 + 2 L].  -> (grad_dense, grad_scores, [the box-piece gradients])."""
    grad_losses = _f32(grad_losses, "grad_losses")
    grad_dense = gaussian_focal_backward([dense], [heatmap], heat_pos, grad_losses[:1], heat_cfg["alpha"], heat_cfg["gamma"],
                                         heat_cfg["loss_weight"])[0]
    grad_scores, grad_pieces = transfusion_layer_losses_backward(
        scores, labels, label_weights, pieces, bbox_targets, bbox_weights, code_weights, num_pos, grad_losses[1:1 + layers],
        grad_losses[1 + layers:], layers, cls_cfg, box_cfg)
    return grad_dense, grad_scores, grad_pieces


def centerhead_loss_forward(heat_preds, heatmaps, maps, inds, anno_boxes, masks, code_weights=_DEFAULT_CODE_WEIGHTS, cls_cfg=_HEAT,
                            box_cfg=_BOX):
    """All losses of CenterHead.loss: 3 launches for any number of tasks.  -> (losses [2 T] = heatmap per task, bbox per task;
    heat_pos [T]; avg [T]: what the backward reads)."""
    T = len(heat_preds)
    losses = torch.empty(2 * T, dtype=torch.float32, device=heat_preds[0].device)
    _, heat_pos = gaussian_focal_forward(heat_preds, heatmaps, cls_cfg["alpha"], cls_cfg["gamma"], cls_cfg["loss_weight"], out=losses[:T])
    _, avg = centerhead_box_loss_forward(maps, inds, anno_boxes, masks, code_weights, box_cfg["loss_weight"], out=losses[T:])
    return losses, heat_pos, avg


def centerhead_loss_backward(heat_preds, heatmaps, maps, inds, anno_boxes, masks, heat_pos, avg, grad_losses,
                             code_weights=_DEFAULT_CODE_WEIGHTS, cls_cfg=_HEAT, box_cfg=_BOX):
    """3 launches.  -> (the heatmap gradients per task, per task the five regression-map gradients)."""
    T = len(heat_preds)
    grad_losses = _f32(grad_losses, "grad_losses")
    grad_heat = gaussian_focal_backward(heat_preds, heatmaps, heat_pos, grad_losses[:T], cls_cfg["alpha"], cls_cfg["gamma"],
                                        cls_cfg["loss_weight"])
    grad_maps = centerhead_box_loss_backward(maps, inds, anno_boxes, masks, code_weights, avg, grad_losses[T:], box_cfg["loss_weight"])
    return grad_heat, grad_maps


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
class _TransFusionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, fixed, dense, scores, *pieces):
        heatmap, labels, label_weights, bbox_targets, bbox_weights, num_pos = fixed
        pieces = list(pieces) + [None] * (5 - len(pieces))
        losses, heat_pos = transfusion_loss_forward(dense, heatmap, scores, labels, label_weights, pieces, bbox_targets, bbox_weights,
                                                    num_pos, *cfg)
        ctx.cfg, ctx.fixed, ctx.n = cfg, fixed, len([p for p in pieces if p is not None])
        ctx.save_for_backward(dense, scores, heat_pos, *[p for p in pieces if p is not None])
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        dense, scores, heat_pos, *pieces = ctx.saved_tensors
        heatmap, labels, label_weights, bbox_targets, bbox_weights, num_pos = ctx.fixed
        pieces = list(pieces) + [None] * (5 - len(pieces))
        gd, gs, gp = transfusion_loss_backward(dense, heatmap, scores, labels, label_weights, pieces, bbox_targets, bbox_weights, num_pos,
                                               heat_pos, grad_losses, *ctx.cfg)
        return (None, None, gd.view_as(dense), gs) + tuple(gp[:ctx.n])


class _CenterHeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, fixed, *tensors):
        T = len(tensors) // 6
        heatmaps, anno_boxes, inds, masks = fixed
        heat_preds, maps = list(tensors[:T]), [list(tensors[T + 5 * t:T + 5 * t + 5]) for t in range(T)]
        losses, heat_pos, avg = centerhead_loss_forward(heat_preds, heatmaps, maps, inds, anno_boxes, masks, *cfg)
        ctx.cfg, ctx.fixed, ctx.T = cfg, fixed, T
        ctx.save_for_backward(heat_pos, avg, *tensors)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        heat_pos, avg, *tensors = ctx.saved_tensors
        T = ctx.T
        heatmaps, anno_boxes, inds, masks = ctx.fixed
        heat_preds, maps = list(tensors[:T]), [list(tensors[T + 5 * t:T + 5 * t + 5]) for t in range(T)]
        grad_heat, grad_maps = centerhead_loss_backward(heat_preds, heatmaps, maps, inds, anno_boxes, masks, heat_pos, avg, grad_losses,
                                                        *ctx.cfg)
        return (None, None) + tuple(g.view_as(p) for g, p in zip(grad_heat, heat_preds)) + tuple(g for task in grad_maps for g in task)


class _GaussianFocal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, avg, alpha, gamma, loss_weight):
        loss, num_pos = gaussian_focal_forward([pred], [target], alpha, gamma, loss_weight, pred_is_logit=False, avg=[avg])
        ctx.cfg, ctx.fixed = (alpha, gamma, loss_weight), (target, avg)
        ctx.save_for_backward(pred, num_pos)
        return loss[0]

    @staticmethod
    def backward(ctx, grad):
        pred, num_pos = ctx.saved_tensors
        target, avg = ctx.fixed
        g = gaussian_focal_backward([pred], [target], num_pos, grad.reshape(1), *ctx.cfg, pred_is_logit=False, avg=[avg])[0]
        return g.view_as(pred), None, None, None, None, None


class _LayerLoss(torch.autograd.Function):
    """One half of the layer losses for the modules: kind "cls" (pred [N, C] logits) or "box" (pred [..., D] packed)."""

    @staticmethod
    def forward(ctx, pred, kind, target, weight, avg, cfg):
        ctx.kind, ctx.fixed, ctx.cfg = kind, (target, weight, avg), cfg
        ctx.save_for_backward(pred)
        if kind == "cls":
            N, C = pred.shape
            return transfusion_layer_losses_forward(pred.view(N, C, 1), target.view(N, 1), weight.view(N, 1), None, None, None, None, None, 1,
                                                    cls_cfg=cfg, avg_cls=avg)[0][0]
        D = pred.shape[-1]
        return transfusion_layer_losses_forward(None, None, None, pred.reshape(1, -1, D), target.reshape(1, -1, D), weight.reshape(1, -1, D),
                                                None, None, 1, box_cfg=cfg, avg_box=avg)[1][0]

    @staticmethod
    def backward(ctx, grad):
        (pred,) = ctx.saved_tensors
        target, weight, avg = ctx.fixed
        grad = grad.reshape(1)
        if ctx.kind == "cls":
            N, C = pred.shape
            g = transfusion_layer_losses_backward(pred.view(N, C, 1), target.view(N, 1), weight.view(N, 1), None, None, None, None, None, grad,
                                                  None, 1, cls_cfg=ctx.cfg, avg_cls=avg)[0]
        else:
            D = pred.shape[-1]
            g = transfusion_layer_losses_backward(None, None, None, pred.reshape(1, -1, D), target.reshape(1, -1, D), weight.reshape(1, -1, D),
                                                  None, None, None, grad, 1, box_cfg=ctx.cfg, avg_box=avg)[1]
        return g.view_as(pred), None, None, None, None, None


# ---- the loss modules -----------------------------------------------------------------------------------------------------------------
class _Loss(nn.Module):
    def _reduction(self, override):
        reduction = override if override else self.reduction
        if reduction == "none":
            raise NotImplementedError("reduction='none' is not served: 'mean' and 'sum' are")
        if reduction not in ("mean", "sum"):
            raise ValueError(f"reduction {reduction!r}")
        return reduction

    @staticmethod
    def _avg(reduction, avg_factor, count, like):
        """The divisor as a 0-dim tensor on the device (and in the dtype) of `like`: 1 for a sum, avg_factor, or the element count."""
        if reduction == "sum":
            if avg_factor is not None:
                raise ValueError('avg_factor can not be used with reduction="sum"')
            avg_factor = 1.0
        elif avg_factor is None:
            avg_factor = float(count)
        if torch.is_tensor(avg_factor):
            return avg_factor.detach().to(device=like.device, dtype=like.dtype).reshape(())
        return torch.full((), float(avg_factor), dtype=like.dtype, device=like.device)


class GaussianFocalLoss(_Loss):
    """mmdet 2.x GaussianFocalLoss: pred holds PROBABILITIES (the heads pass clip_sigmoid's output), target the Gaussian heatmap."""

    def __init__(self, alpha=2.0, gamma=4.0, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.alpha, self.gamma, self.reduction, self.loss_weight = alpha, gamma, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        if weight is not None:
            raise NotImplementedError("GaussianFocalLoss: a per-element weight is not served (neither head passes one)")
        avg = self._avg(self._reduction(reduction_override), avg_factor, pred.numel(), pred)
        if not pred.is_cuda:
            return self.loss_weight * (_gaussian_focal_host(pred, target, self.alpha, self.gamma).sum() / avg)
        return _GaussianFocal.apply(_f32(pred, "pred"), _f32(target, "target"), avg, self.alpha, self.gamma, self.loss_weight)


class FocalLoss(_Loss):
    """mmdet 2.x FocalLoss, the sigmoid form: pred [N, C] logits, target [N] labels with C for background, weight [N]."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0):
        super().__init__()
        if use_sigmoid is not True:
            raise NotImplementedError("only the sigmoid focal loss is served")
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = True, gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        avg = self._avg(self._reduction(reduction_override), avg_factor, pred.numel(), pred)
        if weight is None:
            weight = torch.ones(pred.shape[0], dtype=pred.dtype, device=pred.device)
        if not pred.is_cuda:
            return self.loss_weight * (_sigmoid_focal_host(pred, target, weight, self.gamma, self.alpha).sum() / avg)
        if weight.dtype not in (torch.float32, torch.int64):
            weight = weight.float()
        cfg = dict(alpha=self.alpha, gamma=self.gamma, loss_weight=self.loss_weight)
        return _LayerLoss.apply(_f32(pred, "pred"), "cls", target.long().contiguous(), weight.contiguous(), avg, cfg)


class L1Loss(_Loss):
    """mmdet 2.x L1Loss: pred, target and weight of one shape [..., D], D at most 16 on the device."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        avg = self._avg(self._reduction(reduction_override), avg_factor, pred.numel(), pred)
        if weight is None:
            weight = torch.ones_like(pred)
        if not pred.is_cuda:
            return self.loss_weight * (((pred - target).abs() * weight).sum() / avg)
        return _LayerLoss.apply(_f32(pred, "pred"), "box", _f32(target, "target"), _f32(weight, "weight"), avg, dict(loss_weight=self.loss_weight))


for _cls in (GaussianFocalLoss, FocalLoss, L1Loss):
    register_everywhere("loss", _cls)


# ---- the heads' loss functions ----------------------------------------------------------------------------------------------------------
def _loss_cfg(cfg, kind, defaults):
    """A loss block (a config dict or a module) -> the plain numbers the kernels take; `kind`: the class the head supports there."""
    module = build_from_cfg(cfg, LOSSES) if isinstance(cfg, dict) else cfg
    if not isinstance(module, kind):
        raise NotImplementedError(f"{type(module).__name__}: this loss of the head is a {kind.__name__}")
    if module.reduction != "mean":
        raise NotImplementedError(f"reduction {module.reduction!r}: the heads' losses are means over avg_factor")
    out = dict(defaults)
    for k in out:
        out[k] = float(getattr(module, k))
    return out


def _as_dict(preds):
    while isinstance(preds, (list, tuple)):
        preds = preds[0]
    return preds


def transfusion_loss(preds_dict, targets, num_proposals, num_classes, num_decoder_layers=1, auxiliary=True,
                     code_weights=_DEFAULT_CODE_WEIGHTS, loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25,
                                                                      reduction="mean", loss_weight=1.0),
                     loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25),
                     loss_heatmap=dict(type="GaussianFocalLoss", reduction="mean", loss_weight=1.0)):
    """TransFusionHead.loss after get_targets (transfusion.py:612-711).  preds_dict: the head's dict (or the reference's nested list
    around it) with dense_heatmap [B, C, H, W] LOGITS, heatmap [B, C, P] logits, center / height / dim / rot [B, c, P] and optionally
    vel, P = num_proposals * layers; targets: what `transfusion_get_targets` returns, sync=True or sync=False (with the latter
    nothing is read back).  Returns the reference's dict: loss_heatmap, layer_{i}_loss_cls / layer_{i}_loss_bbox (`layer_-1_` for
    the last layer) and matched_ious.  The `on_the_image_mask` branch of the reference (transfusion.py:608-611) is not served: nothing
    in the reference sets that attribute."""
    preds = _as_dict(preds_dict)
    K, C = int(num_proposals), int(num_classes)
    layers = int(num_decoder_layers) if auxiliary else 1
    cls_cfg, box_cfg = _loss_cfg(loss_cls, FocalLoss, _CLS), _loss_cfg(loss_bbox, L1Loss, _BOX)
    heat_cfg = _loss_cfg(loss_heatmap, GaussianFocalLoss, _HEAT)
    dense, scores = preds["dense_heatmap"], preds["heatmap"]
    if scores.dim() != 3 or scores.shape[1] != C or scores.shape[2] != layers * K:
        raise RuntimeError(f"heatmap must be [B, {C}, {layers * K}], got {tuple(scores.shape)}")
    names = PIECES if preds.get("vel") is not None else PIECES[:4]
    code_weights = [float(w) for w in code_weights][:10 if len(names) == 5 else 8]
    if not dense.is_cuda:
        return _losses_host("transfusion", preds, targets, K, C, layers, code_weights, cls_cfg, box_cfg, heat_cfg)
    labels, label_weights, bbox_targets, bbox_weights, _, num_pos, matched_ious, heatmap = targets[:8]
    dev = dense.device
    if not torch.is_tensor(num_pos):
        num_pos = torch.full((), int(num_pos), dtype=torch.int32, device=dev)
    if not torch.is_tensor(matched_ious):
        matched_ious = torch.full((), float(matched_ious), dtype=torch.float32, device=dev)
    fixed = (heatmap, labels, label_weights, bbox_targets, bbox_weights, num_pos)
    cfg = (layers, tuple(code_weights), cls_cfg, box_cfg, heat_cfg)
    losses = _TransFusionLoss.apply(cfg, fixed, _f32(dense, "dense_heatmap"), _f32(scores, "heatmap"), *[_f32(preds[n], n) for n in names])
    parts = losses.unbind(0)
    out = {"loss_heatmap": parts[0]}
    for i in range(layers):
        prefix = "layer_-1" if i == layers - 1 else f"layer_{i}"
        out[f"{prefix}_loss_cls"] = parts[1 + i]
        out[f"{prefix}_loss_bbox"] = parts[1 + layers + i]
    out["matched_ious"] = matched_ious.detach().to(torch.float32)
    return out


def centerhead_loss(preds_dicts, targets, code_weights=_DEFAULT_CODE_WEIGHTS, loss_cls=dict(type="GaussianFocalLoss", reduction="mean"),
                    loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25)):
    """CenterHead.loss after get_targets (centerpoint.py:597-633).  preds_dicts: per task the dict (or the reference's one-entry
    list around it) of heatmap [B, C_t, H, W] LOGITS and reg, height, dim, rot, vel [B, c, H, W]; targets: `centerhead_get_targets`'
    tuple.  Returns heatmap/task{t} and bbox/task{t}.  The prediction dicts are left as they are: the reference replaces
    preds_dict[0]["heatmap"] by its clipped sigmoid in place and adds an "anno_box" entry."""
    tasks = [_as_dict(p) for p in preds_dicts]
    T = len(tasks)
    cls_cfg, box_cfg = _loss_cfg(loss_cls, GaussianFocalLoss, _HEAT), _loss_cfg(loss_bbox, L1Loss, _BOX)
    code_weights = [float(w) for w in code_weights]
    if not tasks[0]["heatmap"].is_cuda:
        return _losses_host("centerhead", tasks, targets, code_weights, cls_cfg, box_cfg)
    heatmaps, anno_boxes, inds, masks = (list(v) for v in targets[:4])
    tensors = [_f32(p["heatmap"], "heatmap") for p in tasks] + [_f32(p[n], n) for p in tasks for n in CH_PIECES]
    losses = _CenterHeadLoss.apply((tuple(code_weights), cls_cfg, box_cfg), (heatmaps, anno_boxes, inds, masks), *tensors)
    parts = losses.unbind(0)
    out = {}
    for t in range(T):
        out[f"heatmap/task{t}"] = parts[t]
        out[f"bbox/task{t}"] = parts[T + t]
    return out
