"""Map segmentation metrics on the device (reference: NuScenesDataset.evaluate_map, mmdet3d/datasets/nuscenes_dataset.py:498-530),
over csrc/ext/seg_head.hip.  `heads` re-exports everything here.

  * `seg_iou_counts`: tp / fp / fn of every class and threshold over all samples, [K, T, 3] int64, in two launches with no host
    sync (the reference materialises a [K, H * W, 7] boolean tensor three times per sample);
  * `evaluate_map`: the reference's metrics dict from those counts.

Dispatch: device tensors go through the library or raise; host tensors run the reference's torch formulation.
"""
import torch

from . import _capi

__all__ = ["seg_iou_counts", "evaluate_map", "MAP_THRESHOLDS"]

MAX_THRESHOLDS = 16      # SG_MAX_THRESHOLDS of the kernel
MAP_THRESHOLDS = (0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65)
_THRESHOLD_CACHE = {}


def _device_thresholds(thr, dev):
    """Host threshold values on `dev`, uploaded once per (values, device) through pinned memory without a sync."""
    key = (tuple(thr.tolist()), str(dev))
    if key not in _THRESHOLD_CACHE:
        if len(_THRESHOLD_CACHE) > 256:
            _THRESHOLD_CACHE.clear()
        host = thr.contiguous().pin_memory()
        _THRESHOLD_CACHE[key] = (host, host.to(dev, non_blocking=True))      # the pinned source outlives the copy
    return _THRESHOLD_CACHE[key][1]


def seg_iou_counts(pred, label, thresholds=MAP_THRESHOLDS):
    """pred, label [S, K, ...] -> [K, T, 3] int64: tp, fp, fn of `pred >= threshold` (fp32) against `label != 0`, summed over
    samples and cells.  `thresholds`: a sequence or an fp32 tensor of 1 .. 16 values (a device tensor is used as it is)."""
    if pred.dim() < 2 or pred.shape != label.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and label {tuple(label.shape)}: equal [S, K, ...] shapes expected")
    on_device = torch.is_tensor(thresholds) and thresholds.is_cuda
    thr = thresholds if torch.is_tensor(thresholds) else torch.tensor(list(thresholds), dtype=torch.float32)
    thr = thr.to(torch.float32).reshape(-1)
    if not 1 <= thr.numel() <= MAX_THRESHOLDS:
        raise ValueError(f"{thr.numel()} thresholds (1 .. {MAX_THRESHOLDS})")
    S, K = pred.shape[:2]
    if pred.is_cuda != label.is_cuda:
        raise RuntimeError("pred and label must be on the same device")
    if not pred.is_cuda:
        hit = pred.detach().float().reshape(S, K, -1, 1) >= thr.cpu()
        truth = label.detach().bool().reshape(S, K, -1, 1)
        return torch.stack([(hit & truth).sum(dim=(0, 2)), (hit & ~truth).sum(dim=(0, 2)), (~hit & truth).sum(dim=(0, 2))], dim=-1)
    if pred.numel() == 0:
        raise RuntimeError("IoU counts of an empty tensor")
    lib = _capi.load()
    dev = pred.device
    pred = pred.detach().float().reshape(S, K, -1).contiguous()
    label = label.detach().reshape(S, K, -1).contiguous()
    if label.dtype == torch.bool:
        label = label.view(torch.uint8)
    elif label.dtype not in (torch.float32, torch.uint8):
        label = label.ne(0).view(torch.uint8)
    thr = thr.contiguous() if on_device else _device_thresholds(thr, dev)
    counts = torch.empty((K, thr.numel(), 3), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bevamd_seg_iou_counts(_capi.ptr(pred), _capi.ptr(label), 0 if label.dtype == torch.float32 else 3, S, K, pred.shape[2],
                                       _capi.ptr(thr), thr.numel(), _capi.ptr(counts), _capi.stream_ptr(dev))
    _capi.check(rc, "seg_iou_counts")
    return counts


def evaluate_map(results, map_classes):
    """NuScenesDataset.evaluate_map: `results` is a list of dicts with "masks_bev" and "gt_masks_bev" ([K, H, W] each).  Returns the
    reference's dict: map/{name}/iou@{threshold}, map/{name}/iou@max and map/mean/iou@max (one read-back of the counts)."""
    thresholds = torch.tensor(MAP_THRESHOLDS)
    K = len(map_classes)
    pred = torch.stack([r["masks_bev"].detach().reshape(K, -1) for r in results])
    label = torch.stack([r["gt_masks_bev"].detach().reshape(K, -1) for r in results])
    counts = seg_iou_counts(pred, label, thresholds).cpu().to(torch.float32)
    tp, fp, fn = counts[..., 0], counts[..., 1], counts[..., 2]
    ious = tp / (tp + fp + fn + 1e-7)
    metrics = {}
    for index, name in enumerate(map_classes):
        metrics[f"map/{name}/iou@max"] = ious[index].max().item()
        for threshold, iou in zip(thresholds, ious[index]):
            metrics[f"map/{name}/iou@{threshold.item():.2f}"] = iou.item()
    metrics["map/mean/iou@max"] = ious.max(dim=1).values.mean().item()
    return metrics
