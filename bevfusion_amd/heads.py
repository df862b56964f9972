"""The two non-learned ends of the TransFusion detection head (reference: mmdet3d/models/heads/bbox/transfusion.py,
mmdet3d/core/bbox/coders/transfusion_bbox_coder.py, mmdet3d/core/post_processing/box3d_nms.py), over csrc/ext/head_ends.hip.

  * `transfusion_select_proposals`: forward_single's proposal selection (transfusion.py:239-295, :322-325) — sigmoid, 3x3 local
    maximum, top-K over all classes and the three gathers — as four launches with no host sync;
  * `transfusion_get_bboxes`: get_bboxes (transfusion.py:725-838) — score, box decode, range / score filter and the per-task NMS;
    `nms_type` None and "circle" stay on the device (one read-back of the B kept counts with sync=True, none with sync=False),
    "rotate" goes through `iou3d.nms_gpu`;
  * `TransFusionBBoxCoder`: the reference's coder, registered in `registry.BBOX_CODERS`;
  * `circle_nms`: the reference's function (also what CenterHead.get_bboxes calls);
  * `CenterPointBBoxCoder`, `centerhead_get_bboxes`, `rotate_nms_segments`: the CenterHead end, re-exported from `centerhead`;
  * `centerhead_get_targets`, `transfusion_heatmap_targets`: the training targets of both heads, re-exported from `head_targets`;
  * `transfusion_get_targets`, `HungarianAssigner3D`, the match costs, `BboxOverlaps3D`, `linear_sum_assignment_batch`: the
    assignment end of TransFusionHead.get_targets, re-exported from `head_assign`;
  * `seg_iou_counts`, `evaluate_map`: the map segmentation metrics of NuScenesDataset.evaluate_map, re-exported from `seg_head`;
  * `TransformerDecoderLayer`, `MultiheadAttention`, `PositionEmbeddingLearned`, `fused_attention`: the head's learned stage, the
    decoder layer over the fused attention kernels, re-exported from `decoder`;
  * `transfusion_loss`, `centerhead_loss`, `GaussianFocalLoss`, `FocalLoss`, `L1Loss`: the losses of both heads with their
    gradients, re-exported from `head_losses`;
  * `TransFusionHead`, `FFN`, `ConvModule`, `head_class_encoding`, `head_ffn_forward`: the head as a module, its category encoding
    and its prediction heads fused for eval mode, re-exported from `transfusion_head`;
  * `CenterHead`, `SeparateHead`, `center_heads_forward`: the other detection head as a module and its task heads fused for eval
    mode, re-exported from `centerhead_module`;
  * `ConvFuser`, `SECOND`, `SECONDFPN`, `bev_conv_forward`, `fold_bev_layer`: the dense BEV trunk in front of the heads as modules
    and its fused convolution + BatchNorm + ReLU layer for eval mode, re-exported from `bev_trunk`;
  * `fold_conv_bias_bn`, `fold_depth_stem`, `fold_depth_head`, `depth_stem_forward`, `depth_head_forward`: the learned nets of the
    camera view transforms on 16-bit operands, re-exported from `cam_nets`;
  * `GeneralizedLSSFPN`, `LSSFPN`, `cam_neck_conv_forward`, `fold_conv_bias`: the camera necks as modules and their fused
    resampling + `cat` + convolution + BatchNorm + ReLU layer for eval mode, re-exported from `cam_neck`;
  * `GeneralizedResNet`, `BasicBlock`, `make_res_layer`, `res_block_forward`, `fold_res_block`, `res_block_spec`: the residual BEV
    backbone of the camera configs as a module and its fused block tail (conv2 + BatchNorm + residual + ReLU) for eval mode,
    re-exported from `bev_resnet`;
  * `ResNet`, `Bottleneck`, `bottleneck_tail_forward`, `fold_bottleneck`, `bottleneck_spec`, `stem_forward`, `fold_stem`,
    `stem_spec`, `stem_pack_weight`, `stem_unpack_weight`: the camera backbone of the ResNet-50 configs as a module and its fused
    Bottleneck tail (conv3 + BatchNorm + residual + ReLU) and stem (conv 7x7 + BatchNorm + ReLU + MaxPool) for eval mode,
    re-exported from `cam_resnet`;
  * `SwinTransformer`, `SwinBlockSequence`, `SwinBlock`, `ShiftWindowMSA`, `WindowMSA`, `PatchEmbed`, `PatchMerging`, `SwinFFN`
    (mmcv's FFN, `cam_swin.FFN`; `heads.FFN` stays the TransFusion head's), `DropPath`, `window_attention`, `fold_window_bias`, `window_attention_spec`, `swin_convert`, `swin_ffn`,
    `fold_swin_ffn`, `swin_ffn_spec`, `swin_pack_ffn`: the camera backbone of the Swin-T configs as a module, its fused
    shifted-window attention and its fused block FFN (LayerNorm, fc1, GELU, fc2, residual) for eval mode, re-exported from
    `cam_swin`.

Dispatch: device tensors go through the library or raise (no torch formulation for them); host tensors run the reference's
formulation written in torch / numpy with a STABLE descending argsort, which is the order the kernels are defined to produce
(equal values in ascending flat index; equal NMS scores: lower row first).

Differences from the reference, on purpose: `decode` does not overwrite the caller's `center` and `dim`; `decode` does not turn
`self.post_center_range` into a tensor; the proposal order is defined where the reference's unstable argsort leaves it open.
"""
from dataclasses import dataclass

import numpy as np
import torch
from torch.nn import functional as F

from . import _capi
from .bev_trunk import (SECOND, SECONDFPN, ConvFuser, FoldedBevLayer, bev_conv_forward, bev_pack_weight,  # noqa: F401  (the BEV trunk)
                        bev_unpack_weight, fold_bev_layer)
from .bev_resnet import (BasicBlock, FoldedResBlock, GeneralizedResNet, fold_res_block, make_res_layer,  # noqa: F401
                         res_block_forward, res_block_spec)                 # (the residual BEV backbone)
from .cam_resnet import (Bottleneck, FoldedBottleneckTail, FoldedStem, ResNet, bottleneck_spec, bottleneck_tail_forward,  # noqa: F401
                         fold_bottleneck, fold_stem, stem_forward, stem_pack_weight, stem_spec, stem_unpack_weight)  # (the camera ResNet)
from .cam_swin import (DropPath, PatchEmbed, PatchMerging, ShiftWindowMSA, SwinBlock, SwinBlockSequence, SwinFFN,  # noqa: F401
                       SwinTransformer, WindowMSA, fold_swin_ffn, fold_window_bias, swin_convert, swin_ffn, swin_ffn_spec,
                       swin_pack_ffn, window_attention, window_attention_spec)  # (the camera Swin Transformer)
from .cam_nets import (DepthHeadFold, DepthStemFold, depth_head_forward, depth_stem_forward, fold_conv_bias_bn,  # noqa: F401
                       fold_depth_head, fold_depth_stem)                    # (the camera depth nets)
from .cam_neck import (LSSFPN, GeneralizedLSSFPN, cam_neck_conv_forward, fold_conv_bias, fold_neck_layer,  # noqa: F401
                       neck_layer_spec)                                     # (the camera necks)
from .centerhead import CenterPointBBoxCoder, centerhead_get_bboxes, rotate_nms_segments  # noqa: F401  (the CenterHead end)
from .decoder import MultiheadAttention, PositionEmbeddingLearned, TransformerDecoderLayer, fused_attention  # noqa: F401  (the decoder layer)
from .head_targets import centerhead_get_targets, transfusion_heatmap_targets  # noqa: F401  (the training targets)
from .head_assign import (BBOX_ASSIGNERS, IOU_CALCULATORS, MATCH_COST, AssignResult, BBoxBEVL1Cost, BboxOverlaps3D,  # noqa: F401
                          ClassificationCost, FocalLossCost, HungarianAssigner3D, IoU3DCost, linear_sum_assignment_batch,
                          transfusion_get_targets)                          # (the TransFusion assignment)
from .head_losses import LOSSES, FocalLoss, GaussianFocalLoss, L1Loss, centerhead_loss, transfusion_loss  # noqa: F401  (the losses)
from .registry import BBOX_CODERS, register_everywhere
from .seg_head import evaluate_map, seg_iou_counts  # noqa: F401  (the map segmentation metrics)
from .centerhead_module import (CenterHead, FoldedCenterHeads, SeparateHead, center_heads_forward,  # noqa: F401  (the CenterHead module)
                                center_heads_pack_w1, center_heads_unpack_w1, fold_center_heads)
from .transfusion_head import HEADS, FFN, ConvModule, TransFusionHead, head_class_encoding, head_ffn_forward  # noqa: F401  (the module)

__all__ = ["circle_nms", "circle_nms_segments", "TransFusionBBoxCoder", "ProposalSelection", "transfusion_select_proposals",
           "transfusion_get_bboxes", "exempt_classes", "nms_tasks", "BBOX_CODERS", "CenterPointBBoxCoder", "centerhead_get_bboxes",
           "rotate_nms_segments", "centerhead_get_targets", "transfusion_heatmap_targets", "transfusion_get_targets",
           "linear_sum_assignment_batch", "HungarianAssigner3D", "AssignResult", "FocalLossCost", "ClassificationCost", "BBoxBEVL1Cost",
           "IoU3DCost", "BboxOverlaps3D", "BBOX_ASSIGNERS", "MATCH_COST", "IOU_CALCULATORS", "seg_iou_counts", "evaluate_map",
           "fused_attention", "MultiheadAttention", "PositionEmbeddingLearned", "TransformerDecoderLayer", "transfusion_loss",
           "centerhead_loss", "GaussianFocalLoss", "FocalLoss", "L1Loss", "LOSSES", "TransFusionHead", "FFN", "ConvModule",
           "head_class_encoding", "head_ffn_forward", "HEADS", "CenterHead", "SeparateHead", "FoldedCenterHeads", "center_heads_forward",
           "center_heads_pack_w1", "center_heads_unpack_w1", "fold_center_heads", "ConvFuser", "SECOND", "SECONDFPN", "FoldedBevLayer",
           "bev_conv_forward", "bev_pack_weight", "bev_unpack_weight", "fold_bev_layer", "DepthStemFold", "DepthHeadFold",
           "fold_conv_bias_bn", "fold_depth_stem", "fold_depth_head", "depth_stem_forward", "depth_head_forward", "GeneralizedLSSFPN",
           "LSSFPN", "cam_neck_conv_forward", "fold_conv_bias", "fold_neck_layer", "neck_layer_spec", "GeneralizedResNet", "BasicBlock",
           "make_res_layer", "FoldedResBlock", "fold_res_block", "res_block_forward", "res_block_spec",
           "ResNet", "Bottleneck", "FoldedBottleneckTail", "FoldedStem", "bottleneck_spec", "fold_bottleneck", "bottleneck_tail_forward",
           "stem_spec", "fold_stem", "stem_forward", "stem_pack_weight", "stem_unpack_weight",
           "SwinTransformer", "SwinBlockSequence", "SwinBlock", "ShiftWindowMSA", "WindowMSA", "PatchEmbed", "PatchMerging", "SwinFFN",
           "DropPath", "window_attention", "fold_window_bias", "window_attention_spec", "swin_convert", "swin_ffn", "fold_swin_ffn",
           "swin_ffn_spec", "swin_pack_ffn"]

MAX_PROPOSALS = 1024     # HE_MAX_K of the kernels: proposals per sample, rows per NMS segment
_UNSUPPORTED = 4

# transfusion.py:247-265: classes whose heatmap is not suppressed (small objects), per test_cfg["dataset"]
_EXEMPT = {"nuScenes": (8, 9), "Waymo": (1, 2)}
# transfusion.py:751-779: (class indices, radius) per NMS task
_TASKS = {
    "nuScenes": (((0, 1, 2, 3, 4, 5, 6, 7), -1), ((8,), 0.175), ((9,), 0.175)),
    "Waymo": (((0,), 0.7), ((1,), 0.7), ((2,), 0.7)),
}
CIRCLE_POST_MAX_SIZE = 83   # get_bboxes calls circle_nms with its default post_max_size


def exempt_classes(dataset, num_classes):
    classes = _EXEMPT.get(dataset, ())
    if classes and max(classes) >= num_classes:
        raise ValueError(f"dataset {dataset!r} exempts classes {classes}, the heatmap has {num_classes}")
    return classes


def nms_tasks(dataset):
    if dataset not in _TASKS:
        raise ValueError(f"no NMS task table for dataset {dataset!r} (nuScenes, Waymo)")
    return _TASKS[dataset]


# ---- circle NMS ----------------------------------------------------------------------------------------------------------------
def _circle_nms_host(dets, thresh, post_max_size):
    """box3d_nms.py:181-219 on an [N, 3] float array: greedy in descending score (stable: equal scores, lower row first)."""
    x1, y1, scores = dets[:, 0], dets[:, 1], dets[:, 2]
    order = np.argsort(-scores, kind="stable")
    suppressed = np.zeros(dets.shape[0], dtype=bool)
    keep = []
    for _i, i in enumerate(order):
        if suppressed[i]:
            continue
        keep.append(int(i))
        rest = order[_i + 1:]
        dist = (x1[i] - x1[rest]) ** 2 + (y1[i] - y1[rest]) ** 2
        suppressed[rest[dist <= thresh]] = True
    return keep[:post_max_size]


def circle_nms_segments(xy, score, seg_offsets, seg_thresh, max_segment_rows, post_max_size=CIRCLE_POST_MAX_SIZE, live=None):
    """Segmented circle NMS on device tensors, no sync: xy [N, 2], score [N] fp32, seg_offsets [S + 1] int32, seg_thresh [S] fp32,
    live [N] uint8 / bool or None.  Returns (keep [N] bool, keep_order [N] int64, counts [S] int32); a threshold <= 0 keeps every
    live row of its segment."""
    if not xy.is_cuda:
        raise RuntimeError("circle_nms_segments needs GPU tensors (host data: circle_nms)")
    lib = _capi.load()
    dev = xy.device
    xy, score = xy.detach().float().contiguous(), score.detach().float().contiguous()
    n, s = score.shape[0], seg_thresh.shape[0]
    if xy.shape != (n, 2) or seg_offsets.shape != (s + 1,) or seg_offsets.dtype != torch.int32 or seg_thresh.dtype != torch.float32:
        raise RuntimeError(f"xy [N, 2], score [N], seg_offsets [S + 1] int32, seg_thresh [S] float32 expected, got "
                           f"{tuple(xy.shape)}, {tuple(score.shape)}, {tuple(seg_offsets.shape)} {seg_offsets.dtype}, "
                           f"{tuple(seg_thresh.shape)} {seg_thresh.dtype}")
    if live is not None:
        live = live.to(torch.uint8).contiguous()
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(s, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bevamd_circle_nms(_capi.ptr(xy), _capi.ptr(score), n, _capi.ptr(seg_offsets.contiguous()), s,
                                   _capi.ptr(seg_thresh.contiguous()), int(max_segment_rows), int(post_max_size), _capi.ptr(live),
                                   _capi.ptr(keep), _capi.ptr(order), _capi.ptr(counts), _capi.stream_ptr(dev))
    _capi.check(rc, "circle_nms")
    return keep.bool(), order, counts


def circle_nms(dets, thresh, post_max_size=83):
    """Circular NMS (box3d_nms.py:181-219): dets [N, 3] = (x, y, score); a detection is kept if no kept detection with a higher
    score lies within squared distance `thresh`.  Returns the kept indices in descending score order, at most post_max_size:
    a list for a numpy array, an int64 tensor for a tensor.  Device tensors run the HIP kernel (one 4-byte read-back)."""
    if isinstance(dets, np.ndarray):
        return _circle_nms_host(dets, thresh, post_max_size)
    if dets.dim() != 2 or dets.shape[1] != 3:
        raise RuntimeError(f"dets must be [N, 3] (x, y, score), got {tuple(dets.shape)}")
    if not dets.is_cuda:
        return torch.tensor(_circle_nms_host(dets.detach().numpy(), thresh, post_max_size), dtype=torch.int64)
    n = dets.shape[0]
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dets.device)
    if n > MAX_PROPOSALS:
        raise RuntimeError(f"circle_nms on the device serves up to {MAX_PROPOSALS} detections, got {n}")
    d = dets.detach().float()
    off = torch.tensor([0, n], dtype=torch.int32, device=dets.device)
    thr = torch.full((1,), float(thresh), dtype=torch.float32, device=dets.device)
    _, order, counts = circle_nms_segments(d[:, :2], d[:, 2], off, thr, n, post_max_size)
    return order[: min(int(counts.item()), post_max_size)]


# ---- box coder -----------------------------------------------------------------------------------------------------------------
def _decode_device(heatmap, rot, dim, center, height, vel, coder, num_proposals, query_heatmap_score=None, query_labels=None):
    """bevamd_transfusion_decode on the LAST num_proposals columns -> (boxes [B, K, 7|9], scores, labels int64, valid bool)."""
    lib = _capi.load()
    dev = heatmap.device
    tensors = dict(heatmap=heatmap, rot=rot, dim=dim, center=center, height=height)
    if vel is not None:
        tensors["vel"] = vel
    B, C, P = heatmap.shape
    K = int(num_proposals)
    want = dict(heatmap=C, rot=2, dim=3, center=2, height=1, vel=2)
    for name, t in tensors.items():
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (B, want[name], P):
            raise RuntimeError(f"{name} must be a float32 GPU tensor [{B}, {want[name]}, {P}], got {tuple(t.shape)} {t.dtype} on {t.device}")
        tensors[name] = t.detach().contiguous()
    if (query_heatmap_score is None) != (query_labels is None):
        raise RuntimeError("query_heatmap_score and query_labels come together")
    if query_labels is not None:
        if tuple(query_heatmap_score.shape) != (B, C, K) or tuple(query_labels.shape) != (B, K):
            raise RuntimeError(f"query_heatmap_score [{B}, {C}, {K}] and query_labels [{B}, {K}] expected, got "
                               f"{tuple(query_heatmap_score.shape)} and {tuple(query_labels.shape)}")
        query_heatmap_score = query_heatmap_score.detach().to(device=dev, dtype=torch.float32).contiguous()
        query_labels = query_labels.detach().to(device=dev, dtype=torch.int64).contiguous()
    width = 9 if vel is not None else 7
    boxes = torch.empty((B, K, width), dtype=torch.float32, device=dev)
    scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    labels = torch.empty((B, K), dtype=torch.int64, device=dev)
    valid = torch.empty((B, K), dtype=torch.uint8, device=dev)
    consts = _capi.floats([coder.out_size_factor, coder.voxel_size[0], coder.voxel_size[1], coder.pc_range[0], coder.pc_range[1]])
    rng = _capi.floats(list(coder.post_center_range)) if coder.post_center_range is not None else None
    thr = coder.score_threshold
    with torch.cuda.device(dev):
        rc = lib.bevamd_transfusion_decode(
            _capi.ptr(tensors["heatmap"]), _capi.ptr(tensors["center"]), _capi.ptr(tensors["height"]), _capi.ptr(tensors["dim"]),
            _capi.ptr(tensors["rot"]), _capi.ptr(tensors.get("vel")), _capi.ptr(query_heatmap_score), _capi.ptr(query_labels), B, C, K,
            P, consts, rng, float(thr) if thr else 0.0, 1 if thr else 0, _capi.ptr(boxes), _capi.ptr(scores), _capi.ptr(labels),
            _capi.ptr(valid), _capi.stream_ptr(dev))
    _capi.check(rc, "transfusion_decode")
    return boxes, scores, labels, valid.bool()


def _decode_host(heatmap, rot, dim, center, height, vel, coder):
    """TransFusionBBoxCoder.decode's arithmetic on host tensors -> (boxes [B, K, 7|9], scores, labels); inputs untouched."""
    m = heatmap.max(1, keepdims=False)
    center, dim = center.clone(), dim.clone()
    center[:, 0, :] = center[:, 0, :] * coder.out_size_factor * coder.voxel_size[0] + coder.pc_range[0]
    center[:, 1, :] = center[:, 1, :] * coder.out_size_factor * coder.voxel_size[1] + coder.pc_range[1]
    dim[:, 0, :] = dim[:, 0, :].exp()
    dim[:, 1, :] = dim[:, 1, :].exp()
    dim[:, 2, :] = dim[:, 2, :].exp()
    height = height - dim[:, 2:3, :] * 0.5   # gravity centre to bottom centre
    rot = torch.atan2(rot[:, 0:1, :], rot[:, 1:2, :])
    parts = [center, height, dim, rot] + ([vel] if vel is not None else [])
    return torch.cat(parts, dim=1).permute(0, 2, 1), m.values, m.indices


def _valid_host(boxes, scores, coder):
    rng = torch.tensor(coder.post_center_range, device=boxes.device)
    mask = (boxes[..., :3] >= rng[:3]).all(2)
    mask &= (boxes[..., :3] <= rng[3:]).all(2)
    if coder.score_threshold:   # the reference skips the test for a falsy threshold (0.0 included)
        mask &= scores > coder.score_threshold
    return mask


class TransFusionBBoxCoder:
    """mmdet3d/core/bbox/coders/transfusion_bbox_coder.py: (x, y) in feature-map cells <-> metres, log sizes, sin / cos yaw."""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None, score_threshold=None, code_size=8):
        self.pc_range = pc_range
        self.out_size_factor = out_size_factor
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.score_threshold = score_threshold
        self.code_size = code_size

    def encode(self, dst_boxes):
        targets = torch.zeros([dst_boxes.shape[0], self.code_size]).to(dst_boxes.device)
        targets[:, 0] = (dst_boxes[:, 0] - self.pc_range[0]) / (self.out_size_factor * self.voxel_size[0])
        targets[:, 1] = (dst_boxes[:, 1] - self.pc_range[1]) / (self.out_size_factor * self.voxel_size[1])
        targets[:, 3:6] = dst_boxes[:, 3:6].log()
        targets[:, 2] = dst_boxes[:, 2] + dst_boxes[:, 5] * 0.5   # bottom centre to gravity centre
        targets[:, 6] = torch.sin(dst_boxes[:, 6])
        targets[:, 7] = torch.cos(dst_boxes[:, 6])
        if self.code_size == 10:
            targets[:, 8:10] = dst_boxes[:, 7:]
        return targets

    def decode(self, heatmap, rot, dim, center, height, vel, filter=False):
        """heatmap [B, C, K] class scores, rot [B, 2, K], dim [B, 3, K] (log), center [B, 2, K] (cells), height [B, 1, K],
        vel [B, 2, K] or None -> per sample dict(bboxes [n, 7|9], scores [n], labels [n]); filter=True keeps the boxes inside
        post_center_range whose score exceeds a non-zero score_threshold."""
        if filter and self.post_center_range is None:
            raise NotImplementedError("Need to reorganize output as a batch, only support post_center_range is not None for now!")
        if heatmap.is_cuda:
            boxes, scores, labels, valid = _decode_device(heatmap, rot, dim, center, height, vel, self, heatmap.shape[-1])
        else:
            boxes, scores, labels = _decode_host(heatmap, rot, dim, center, height, vel, self)
            valid = _valid_host(boxes, scores, self) if filter else None
        out = []
        for i in range(heatmap.shape[0]):
            if filter:
                out.append(dict(bboxes=boxes[i, valid[i]], scores=scores[i, valid[i]], labels=labels[i, valid[i]]))
            else:
                out.append(dict(bboxes=boxes[i], scores=scores[i], labels=labels[i]))
        return out


register_everywhere("bbox_coder", TransFusionBBoxCoder)


# ---- proposal selection --------------------------------------------------------------------------------------------------------
@dataclass
class ProposalSelection:
    top_proposals_class: torch.Tensor   # [B, K] int64 (the head's query_labels)
    top_proposals_index: torch.Tensor   # [B, K] int64, position in H * W
    top_proposals_score: torch.Tensor   # [B, K] the suppressed sigmoid of each proposal
    query_feat: torch.Tensor            # [B, Cf, K], BEFORE the category encoding (a torch layer of the caller)
    query_pos: torch.Tensor             # [B, K, 2]
    query_heatmap_score: torch.Tensor   # [B, C, K]


def _suppressed_heatmap_host(dense_heatmap, nms_kernel_size, dataset):
    """transfusion.py:239-267 -> [B, C, H * W]."""
    heatmap = dense_heatmap.detach().sigmoid()
    padding = nms_kernel_size // 2
    local_max = torch.zeros_like(heatmap)
    local_max_inner = F.max_pool2d(heatmap, kernel_size=nms_kernel_size, stride=1, padding=0)
    if padding:
        local_max[:, :, padding:(-padding), padding:(-padding)] = local_max_inner
    else:
        local_max = local_max_inner
    for c in exempt_classes(dataset, heatmap.shape[1]):
        local_max[:, c] = heatmap[:, c]
    heatmap = heatmap * (heatmap == local_max)
    return heatmap.view(heatmap.shape[0], heatmap.shape[1], -1)


def transfusion_select_proposals(dense_heatmap, lidar_feat_flatten, bev_pos, num_proposals, nms_kernel_size=3, dataset="nuScenes"):
    """forward_single's query initialisation.  dense_heatmap [B, C, H, W] fp32 LOGITS (finite), lidar_feat_flatten [B, Cf, H * W]
    fp32 / fp16, bev_pos [1 or B, H * W, 2] fp32.  The num_proposals largest suppressed sigmoids of every sample in stable
    descending order (equal values: ascending c * H * W + y * W + x).  No host sync; capturable in a torch.cuda.graph."""
    if dense_heatmap.dim() != 4:
        raise RuntimeError(f"dense_heatmap must be [B, C, H, W], got {tuple(dense_heatmap.shape)}")
    B, C, H, W = dense_heatmap.shape
    K, k = int(num_proposals), int(nms_kernel_size)
    Cf = lidar_feat_flatten.shape[1]
    if tuple(lidar_feat_flatten.shape) != (B, Cf, H * W) or bev_pos.dim() != 3 or bev_pos.shape[0] not in (1, B) \
            or tuple(bev_pos.shape[1:]) != (H * W, 2):
        raise RuntimeError(f"lidar_feat_flatten [B, Cf, {H * W}] and bev_pos [1 or B, {H * W}, 2] expected, got "
                           f"{tuple(lidar_feat_flatten.shape)} and {tuple(bev_pos.shape)}")
    if not 1 <= K <= min(MAX_PROPOSALS, C * H * W) or k < 1 or k % 2 == 0 or k > min(H, W):
        raise RuntimeError(f"num_proposals {K} (1 .. {min(MAX_PROPOSALS, C * H * W)}) or nms_kernel_size {k} (odd, <= {min(H, W)}) out of range")
    exempt = exempt_classes(dataset, C)

    if not dense_heatmap.is_cuda:
        heatmap = _suppressed_heatmap_host(dense_heatmap, k, dataset)
        top = heatmap.view(B, -1).argsort(dim=-1, descending=True, stable=True)[..., :K]
        cls, idx = top // heatmap.shape[-1], top % heatmap.shape[-1]
        return ProposalSelection(
            top_proposals_class=cls, top_proposals_index=idx, top_proposals_score=heatmap.view(B, -1).gather(1, top),
            query_feat=lidar_feat_flatten.gather(index=idx[:, None, :].expand(-1, Cf, -1), dim=-1),
            query_pos=bev_pos.expand(B, -1, -1).gather(index=idx[:, :, None].expand(-1, -1, 2), dim=1),
            query_heatmap_score=heatmap.gather(index=idx[:, None, :].expand(-1, C, -1), dim=-1))

    lib = _capi.load()
    dev = dense_heatmap.device
    if dense_heatmap.dtype != torch.float32 or lidar_feat_flatten.dtype not in (torch.float32, torch.float16) \
            or bev_pos.dtype != torch.float32 or lidar_feat_flatten.device != dev:
        raise RuntimeError(f"dense_heatmap / bev_pos float32 and lidar_feat_flatten float32 or float16 on one device expected, got "
                           f"{dense_heatmap.dtype}, {bev_pos.dtype}, {lidar_feat_flatten.dtype}")
    logits = dense_heatmap.detach().contiguous()
    feat = lidar_feat_flatten.detach().contiguous()
    pos = bev_pos.detach().to(dev).contiguous()
    mask = sum(1 << c for c in exempt)
    cls = torch.empty((B, K), dtype=torch.int64, device=dev)
    idx = torch.empty((B, K), dtype=torch.int64, device=dev)
    score = torch.empty((B, K), dtype=torch.float32, device=dev)
    qfeat = torch.empty((B, Cf, K), dtype=feat.dtype, device=dev)
    qpos = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
    qscore = torch.empty((B, C, K), dtype=torch.float32, device=dev)
    wsb = lib.bevamd_head_proposals_workspace_bytes(B, C, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = _capi.stream_ptr(dev)
        rc = lib.bevamd_head_proposals(_capi.ptr(logits), B, C, H, W, k, mask, K, _capi.ptr(cls), _capi.ptr(idx), _capi.ptr(score),
                                       _capi.ptr(ws), wsb, stream)
        _capi.check(rc, "head_proposals")
        rc = lib.bevamd_head_gather_queries(_capi.ptr(logits), B, C, H, W, k, mask, _capi.ptr(idx), K, _capi.ptr(feat),
                                            0 if feat.dtype == torch.float32 else 1, Cf, _capi.ptr(pos), pos.shape[0],
                                            _capi.ptr(qfeat), _capi.ptr(qpos), _capi.ptr(qscore), stream)
        _capi.check(rc, "head_gather_queries")
    return ProposalSelection(cls, idx, score, qfeat, qpos, qscore)


# ---- get_bboxes ------------------------------------------------------------------------------------------------------------------
_CONST_CACHE = {}


def _task_tables(dataset, num_classes, B, K, dev):
    """(class -> task [num_classes] int64, task ids [1, T, 1], seg_offsets [B * T + 1] int32, seg_thresh [B * T] fp32) on `dev`,
    built once per key: creating them copies from the host, which a graph capture does not allow."""
    key = (dataset, num_classes, B, K, str(dev))
    if key not in _CONST_CACHE:
        tasks = nms_tasks(dataset)
        T = len(tasks)
        table = [-1] * num_classes
        for t, (indices, _) in enumerate(tasks):
            for c in indices:
                if c < num_classes:
                    table[c] = t
        _CONST_CACHE[key] = (torch.tensor(table, dtype=torch.int64, device=dev),
                             torch.arange(T, dtype=torch.int64, device=dev).view(1, T, 1),
                             (torch.arange(B * T + 1, dtype=torch.int64) * K).to(torch.int32).to(dev),
                             torch.tensor([r for _, r in tasks] * B, dtype=torch.float32, device=dev))
    return _CONST_CACHE[key]


def _lidar_bev_xyxyr(boxes):
    """xywhr2xyxyr(LiDARInstance3DBoxes(boxes[:, :7]).bev): (x - w / 2, y - h / 2, x + w / 2, y + h / 2, yaw)."""
    x, y, w, h, r = boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], boxes[:, 6]
    return torch.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2, r], dim=1)


def _task_loop_keep(boxes, scores, labels, valid, test_cfg):
    """transfusion.py:786-830 per sample on [K] tensors (host circle NMS, or rotate NMS through iou3d.nms_gpu) -> keep [K] bool."""
    keep = torch.zeros_like(valid)
    rows = torch.nonzero(valid)[:, 0]
    b3, sc, lb = boxes[rows], scores[rows], labels[rows]
    for indices, radius in nms_tasks(test_cfg["dataset"]):
        task_mask = torch.zeros_like(lb, dtype=torch.bool)
        for c in indices:
            task_mask |= lb == c
        task_rows = torch.nonzero(task_mask)[:, 0]
        if radius > 0:
            if test_cfg["nms_type"] == "circle":
                dets = torch.cat([b3[task_rows][:, :2], sc[task_rows][:, None]], dim=1)
                kept = torch.as_tensor(_circle_nms_host(dets.detach().cpu().numpy(), radius, CIRCLE_POST_MAX_SIZE), dtype=torch.int64)
            else:
                from .iou3d import nms_gpu

                kept = nms_gpu(_lidar_bev_xyxyr(b3[task_rows]), sc[task_rows], thresh=radius, pre_maxsize=test_cfg["pre_maxsize"],
                               post_max_size=test_cfg["post_maxsize"])
            task_rows = task_rows[kept.to(task_rows.device)]
        keep[rows[task_rows]] = True
    return keep


def transfusion_get_bboxes(preds_dict, query_labels, bbox_coder, test_cfg, num_proposals, num_classes, sync=True):
    """get_bboxes of TransFusionHead for one decoder output.  preds_dict: heatmap [B, C, P] logits, center [B, 2, P], height
    [B, 1, P], dim [B, 3, P], rot [B, 2, P], optional vel [B, 2, P] (the LAST num_proposals columns are used) and
    query_heatmap_score [B, C, num_proposals]; query_labels [B, num_proposals] int64; test_cfg: dataset, nms_type (None, "circle",
    "rotate"; "rotate" also pre_maxsize / post_maxsize and the LiDAR box convention for the BEV boxes).

    sync=True : [dict(bboxes [n, 7|9], scores [n], labels [n])] per sample (device tensors: one read-back of the B counts).
    sync=False: dict(bboxes [B, K, 7|9], scores [B, K], labels [B, K], keep [B, K] bool, counts [B] int32), no sync; rows outside
                `keep` are decoded all the same.
    Wrapping into metas[0]["box_type_3d"] stays with the caller."""
    heat = preds_dict["heatmap"]
    K = int(num_proposals)
    B, C = heat.shape[0], heat.shape[1]
    if C != num_classes:
        raise RuntimeError(f"heatmap has {C} classes, num_classes is {num_classes}")
    nms_type = test_cfg.get("nms_type")
    if nms_type not in (None, "circle", "rotate"):
        raise ValueError(f"nms_type {nms_type!r} (None, 'circle', 'rotate')")
    if bbox_coder.post_center_range is None:
        raise NotImplementedError("Need to reorganize output as a batch, only support post_center_range is not None for now!")
    vel = preds_dict.get("vel")
    qscore = preds_dict["query_heatmap_score"]

    if heat.is_cuda:
        boxes, scores, labels, valid = _decode_device(heat, preds_dict["rot"], preds_dict["dim"], preds_dict["center"],
                                                      preds_dict["height"], vel, bbox_coder, K, qscore, query_labels)
    else:
        sl = lambda t: t[..., -K:]   # noqa: E731
        one_hot = F.one_hot(query_labels, num_classes=num_classes).permute(0, 2, 1)
        batch_score = sl(heat).sigmoid() * qscore * one_hot
        boxes, scores, labels = _decode_host(batch_score, sl(preds_dict["rot"]), sl(preds_dict["dim"]), sl(preds_dict["center"]),
                                             sl(preds_dict["height"]), sl(vel) if vel is not None else None, bbox_coder)
        valid = _valid_host(boxes, scores, bbox_coder)

    if nms_type is None:
        keep = valid
    elif nms_type == "circle" and heat.is_cuda:
        if K > MAX_PROPOSALS:
            raise RuntimeError(f"circle NMS on the device serves up to {MAX_PROPOSALS} proposals, got {K}")
        table, task_ids, seg_off, seg_thr = _task_tables(test_cfg["dataset"], num_classes, B, K, heat.device)
        T = task_ids.shape[1]
        live = valid[:, None, :] & (table[labels][:, None, :] == task_ids)           # [B, T, K]: one segment per (sample, task)
        xy = boxes[:, None, :, :2].expand(B, T, K, 2).reshape(-1, 2)
        sc = scores[:, None, :].expand(B, T, K).reshape(-1)
        keep3, _, _ = circle_nms_segments(xy, sc, seg_off, seg_thr, K, CIRCLE_POST_MAX_SIZE, live.reshape(-1))
        keep = keep3.view(B, T, K).any(1)
    else:
        if not sync and heat.is_cuda:
            raise NotImplementedError("sync=False serves nms_type None and 'circle' on device tensors: nms_gpu reads its count back")
        keep = torch.stack([_task_loop_keep(boxes[i], scores[i], labels[i], valid[i], test_cfg) for i in range(B)])

    counts = keep.sum(1, dtype=torch.int32)
    if not sync:
        return dict(bboxes=boxes, scores=scores, labels=labels, keep=keep, counts=counts)
    # kept rows first, in row order; then ONE read-back
    front = torch.sort(keep.to(torch.uint8), dim=1, descending=True, stable=True).indices
    boxes = boxes.gather(1, front[:, :, None].expand(-1, -1, boxes.shape[2]))
    scores, labels = scores.gather(1, front), labels.gather(1, front)
    return [dict(bboxes=boxes[i, :n], scores=scores[i, :n], labels=labels[i, :n]) for i, n in enumerate(counts.tolist())]
