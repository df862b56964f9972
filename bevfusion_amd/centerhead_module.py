"""CenterHead as a module (reference: mmdet3d/models/heads/bbox/centerpoint.py:19-125 SeparateHead, :248-366 CenterHead), registered
in `registry.HEADS` under the reference's names so that `type: CenterHead` of `configs/nuscenes/det/centerhead/default.yaml` builds.
`heads` re-exports everything here.

Module tree and state-dict keys are the reference's (`shared_conv.conv.weight`, `shared_conv.bn.*`,
`task_heads.<t>.<head>.0.conv.weight`, `task_heads.<t>.<head>.0.bn.*`, `task_heads.<t>.<head>.1.weight`, `.1.bias`), so
`load_state_dict(strict=True)` takes its checkpoints' `heads.object.*`.  `type: DCNSeparateHead` is NOT registered: the
deformable convolution it needs is not part of this project, and the registry's `KeyError` is the answer.

`forward_single`: `shared_conv` is a torch convolution in both paths (its input is 256 or 512 channels wide and belongs to the
vendor library); the task heads dispatch as `FFN` does:

  * GPU fp32 tensors, eval mode, no gradient needed, `use_fused`, every head of every task foldable: `bevamd_center_heads_forward`
    (csrc/ext/center_heads.hip): all heads of all tasks in ONE launch, BatchNorm folded, the hidden maps kept in LDS, written into
    one flat buffer of which every returned tensor is a contiguous [B, c, H, W] view;
  * otherwise (train mode, a gradient, `use_fused = False`, a BatchNorm without running statistics, num_conv != 2, a width other
    than 64, more than 16 channels): the module's own torch layers in the reference's order, with autograd, batch statistics and
    running-stat updates.  They are also the only path on host tensors: unlike TransFusionHead this head has no attention, so
    `forward` works on the CPU.

A head is foldable when num_conv == 2, its first stage is Conv2d (no bias) + BatchNorm2d with running statistics + ReLU, its last
a Conv2d with a bias, final_kernel is 1 or 3 and the sizes are the kernel's (64 -> 64 -> 1 .. 16; 1 .. 8 tasks of 1 .. 8 heads).

There is no host sync anywhere in `forward`, and in eval mode it can be captured in a `torch.cuda.graph` after one warm-up forward
(which builds the fold); in eval mode `shared_conv` runs under the backend's deterministic flag
(`transfusion_head._deterministic_convs`; `deterministic_convs = False` opts out), so equal calls give equal bits.

`get_targets`, `loss` and `get_bboxes` are thin methods over `centerhead_get_targets`, `centerhead_loss` and
`centerhead_get_bboxes` with the head's own settings.

Differences from the reference, on purpose: the constructor does NOT mutate the caller's `separate_head` / `common_heads` dicts
(the reference's `separate_head.update(...)` writes in_channels, heads and num_cls into the caller's dict, so that a config
used twice carries the last task's heads); `init_weights` writes under `no_grad` instead of through `.data`, so the fold cache sees
the change; `loss` leaves the prediction dicts as they are (the reference replaces the heatmap by its clipped sigmoid in place);
`get_bboxes` takes `sync` and returns what `centerhead_get_bboxes` returns, wrapping the boxes in `metas[i]["box_type_3d"]` only
where metas carry one.
"""
import contextlib
import copy
from dataclasses import dataclass, field

import torch
from torch import nn

from . import _capi
from .registry import BBOX_CODERS, HEADS, LOSSES, build_conv_layer, build_from_cfg, register_everywhere
from .transfusion_head import ConvModule, _deterministic_convs, _get

__all__ = ["SeparateHead", "CenterHead", "FoldedCenterHeads", "center_heads_forward", "center_heads_pack_w1", "center_heads_unpack_w1",
           "fold_center_heads"]

_UNSUPPORTED = 4   # BEVAMD_ERR_UNSUPPORTED
# limits of bevamd_center_heads_forward
CH_CHANNELS, CH_MAX_TASKS, CH_MAX_TASK_HEADS, CH_MAX_HEAD_CHANNELS = 64, 8, 8, 16
CH_TILE = {1: (8, 16), 3: (6, 14)}   # output cells (H, W) of one workgroup per final_kernel


# ---- the packed weight order -----------------------------------------------------------------------------------------------------
def center_heads_pack_w1(w1):
    """[64, 64, k, k] -> the A-fragment order of v_mfma_f32_32x32x2_f32, flat [4096 k^2]: element [m][s4][lane][q] is
    w1[m * 32 + (lane & 31), ci, tap // k, tap % k] with 2 * (4 * s4 + q) + (lane >> 5) = tap * 64 + ci, so that a lane's four
    consecutive k-steps are one 16-byte load."""
    co, ci, k, _ = w1.shape
    wk = w1.permute(0, 2, 3, 1).reshape(co, k * k * ci)                 # [channel][tap * 64 + ci]
    wk = wk.reshape(co // 32, 32, k * k * ci // 8, 4, 2)                # [m][row][s4][q][half]
    return wk.permute(0, 2, 4, 1, 3).reshape(-1).contiguous()          # [m][s4][half][row][q], lane = half * 32 + row


def center_heads_unpack_w1(flat, k):
    """The inverse of `center_heads_pack_w1`: flat [4096 k^2] -> [64, 64, k, k]."""
    c = CH_CHANNELS
    wk = flat.reshape(c // 32, k * k * c // 8, 2, 32, 4).permute(0, 3, 1, 4, 2).reshape(c, k, k, c)
    return wk.permute(0, 3, 1, 2).contiguous()


@dataclass
class FoldedCenterHeads:
    """The eval-mode task heads in the kernel's layout.  packed: one fp32 device buffer holding per head (w1 in fragment order,
    scale [64], shift [64], w2 as [c][tap][64], bias padded to a multiple of 4); offsets: the first float of every head's block."""
    packed: torch.Tensor
    final_kernel: int
    heads_per_task: list
    channels: list                      # per head, tasks in order
    names: list                         # per task the head names
    offsets: list = field(default_factory=list)
    scales: list = field(default_factory=list)    # per head [64] (views of packed)
    shifts: list = field(default_factory=list)


def fold_center_heads(stacks, final_kernel):
    """stacks: per task a list of (name, nn.Sequential(ConvModule, Conv2d)) -> FoldedCenterHeads on the parameters' device."""
    k2 = final_kernel * final_kernel
    pieces, offsets, channels, names, per_task, where = [], [], [], [], [], []
    total = 0
    for task in stacks:
        per_task.append(len(task))
        names.append([name for name, _ in task])
        for _, seq in task:
            bn = seq[0].norm
            inv = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
            g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(inv)
            b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(inv)
            scale = g * inv
            shift = b - bn.running_mean.detach().float() * scale
            w2 = seq[1].weight.detach().float()
            c = w2.shape[0]
            bias = torch.zeros((c + 3) // 4 * 4, dtype=torch.float32, device=w2.device)
            bias[:c] = seq[1].bias.detach().float()
            block = [center_heads_pack_w1(seq[0].conv.weight.detach().float()), scale, shift,
                     w2.permute(0, 2, 3, 1).reshape(-1), bias]
            offsets.append(total)
            where.append(total + CH_CHANNELS * CH_CHANNELS * k2)
            channels.append(c)
            pieces += block
            total += sum(p.numel() for p in block)
    packed = torch.cat([p.reshape(-1) for p in pieces]).contiguous()   # a fresh allocation: 16-byte aligned, as every block is
    scales = [packed[o:o + CH_CHANNELS] for o in where]
    shifts = [packed[o + CH_CHANNELS:o + 2 * CH_CHANNELS] for o in where]
    return FoldedCenterHeads(packed, final_kernel, per_task, channels, names, offsets, scales, shifts)


def _foldable_stack(seq, classes, num_conv, in_channels, head_conv, final_kernel):
    if num_conv != 2 or not 1 <= classes <= CH_MAX_HEAD_CHANNELS or in_channels != CH_CHANNELS or head_conv != CH_CHANNELS:
        return False
    if final_kernel not in (1, 3) or len(seq) != 2 or not isinstance(seq[0], ConvModule):
        return False
    first, last = seq[0], seq[1]
    bn = first.norm
    if not (type(first.conv) is nn.Conv2d and type(last) is nn.Conv2d and isinstance(bn, nn.BatchNorm2d)):
        return False
    if first.conv.bias is not None or not first.with_activation or last.bias is None:
        return False
    return not bn.training and bn.running_mean is not None and bn.running_var is not None


def _fold_tensors(seq):
    bn = seq[0].norm
    return [seq[0].conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, seq[1].weight, seq[1].bias]


def _cached_fold(owner, separate_heads):
    """The fold of a list of SeparateHead, cached on `owner` on the parameters' and buffers' addresses and versions."""
    tensors = [t for sh in separate_heads for name in sh.heads for t in _fold_tensors(getattr(sh, name))]
    key = tuple((t.data_ptr(), t._version, t.dtype, t.device) if t is not None else None for t in tensors)
    cache = owner.__dict__.get("_bevamd_folded")
    if cache is not None and cache[0] == key:
        return cache[1]
    val = fold_center_heads([[(name, getattr(sh, name)) for name in sh.heads] for sh in separate_heads], separate_heads[0].final_kernel)
    owner.__dict__["_bevamd_folded"] = (key, val)
    return val


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def center_heads_forward(x, folded, out=None):
    """All task heads of a CenterHead in one launch.  x [B, 64, H, W] fp32 on the device (the output of shared_conv); folded: a
    `FoldedCenterHeads` on the same device; out: a flat contiguous fp32 buffer of B * sum(c) * H * W elements (None: a fresh one).
    Returns per task the list of [B, c, H, W] tensors, contiguous views of `out` in head order, or None where the kernel does not
    serve the sizes.  No sync, no copy from the host."""
    if not x.is_cuda:
        raise RuntimeError("center_heads_forward needs GPU tensors (host tensors: the module's torch layers)")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError(f"x must be a float32 [B, C, H, W], got {tuple(x.shape)} {x.dtype}")
    x = x.detach().contiguous()
    B, C, H, W = x.shape
    dev = x.device
    packed = folded.packed
    if packed.device != dev or packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous():
        raise RuntimeError("folded.packed must be a flat contiguous float32 tensor on the device of x")
    if sum(folded.heads_per_task) != len(folded.channels):
        raise RuntimeError(f"heads_per_task {folded.heads_per_task} does not add up to {len(folded.channels)} heads")
    total = B * sum(folded.channels) * H * W
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dev)
    elif out.device != dev or out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous() or out.numel() != total:
        raise RuntimeError(f"out must be a flat contiguous float32 tensor of {total} elements on the device of x")
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_center_heads_forward(_capi.ptr(x), B, C, CH_CHANNELS, H, W, int(folded.final_kernel), len(folded.heads_per_task),
                                                      _capi.ints(folded.heads_per_task), _capi.ints(folded.channels), _capi.ptr(packed),
                                                      packed.numel(), _capi.ptr(out), out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "center_heads_forward")
    res, base, it = [], 0, iter(folded.channels)
    for n in folded.heads_per_task:
        task = []
        for _ in range(n):
            c = next(it)
            task.append(out[base:base + B * c * H * W].view(B, c, H, W))
            base += B * c * H * W
        res.append(task)
    return res


def _fusable_input(x, channels):
    return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == channels \
        and x.shape[2] >= 1 and x.shape[3] >= 1


# ---- modules ---------------------------------------------------------------------------------------------------------------------
class SeparateHead(nn.Module):
    """centerpoint.py:19-125: one small stack per head, `heads` = {name: (classes, num_conv)}, children named after the heads: an
    `nn.Sequential` of num_conv - 1 `ConvModule`s (conv, bn, ReLU) and a convolution with a bias, all final_kernel x final_kernel.
    forward(x [B, in_channels, H, W]) -> {name: [B, classes, H, W]}.  `type: DCNSeparateHead` is not registered (no deformable
    convolution in this project): building one raises the registry's KeyError."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, init_bias=-2.19, conv_cfg=dict(type="Conv2d"),
                 norm_cfg=dict(type="BN2d"), bias="auto", init_cfg=None, **kwargs):
        assert init_cfg is None, "To prevent abnormal initialization behavior, init_cfg is not allowed to be set"
        super().__init__()
        self.heads = heads
        self.init_bias = init_bias
        self.in_channels, self.head_conv, self.final_kernel = in_channels, head_conv, final_kernel
        self.use_fused = True   # eval mode on GPU tensors: all heads in one launch (False: the torch layers)
        same = dict(kernel_size=final_kernel, stride=1, padding=final_kernel // 2)
        for name, (classes, num_conv) in heads.items():
            widths = [in_channels] + [head_conv] * (num_conv - 1)
            stack = [ConvModule(a, b, bias=bias, conv_cfg=conv_cfg, norm_cfg=norm_cfg, **same) for a, b in zip(widths, widths[1:])]
            stack.append(build_conv_layer(conv_cfg, head_conv, classes, bias=True, **same))
            setattr(self, name, nn.Sequential(*stack))
        self.init_cfg = dict(type="Kaiming", layer="Conv2d")

    def init_weights(self):
        """Kaiming weights on every Conv2d (mmcv's `Kaiming` initialiser: fan_out, relu, normal, bias 0), then `init_bias` on the
        last convolution of `heatmap`.  Written under no_grad, not through `.data`: the parameters' versions move and `folded()`
        sees the change."""
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, a=0, mode="fan_out", nonlinearity="relu")
                    if m.bias is not None:
                        m.bias.zero_()
            for name in self.heads:
                if name == "heatmap":
                    getattr(self, name)[-1].bias.fill_(self.init_bias)

    # ---- fused eval path ----
    def _foldable(self):
        if not 1 <= len(self.heads) <= CH_MAX_TASK_HEADS:
            return False
        return all(_foldable_stack(getattr(self, name), classes, num_conv, self.in_channels, self.head_conv, self.final_kernel)
                   for name, (classes, num_conv) in self.heads.items())

    def _no_grad_needed(self, x):
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))

    def fusable(self, x):
        """True when forward(x) runs the fused kernel."""
        return bool(self.use_fused and not self.training and _fusable_input(x, self.in_channels) and self._no_grad_needed(x)
                    and self._foldable())

    def folded(self):
        """`FoldedCenterHeads` of the eval-mode stacks, cached on the parameters' and buffers' addresses and versions.  Every
        in-place torch operation moves the version (`load_state_dict`, an optimizer step, `init_weights`); a write through `.data`
        does not, and after one the cache has to be dropped by hand (`del head._bevamd_folded`).  Run one forward before capturing
        a graph: a fold computed inside a capture is filled only when the graph replays."""
        return _cached_fold(self, [self])

    def forward(self, x):
        if self.fusable(x):
            folded = self.folded()
            if folded.packed.device != x.device:
                raise RuntimeError("module parameters and x live on different devices")
            res = center_heads_forward(x, folded)
            if res is not None:
                return dict(zip(self.heads, res[0]))
        return {name: getattr(self, name)(x) for name in self.heads}


class CenterHead(nn.Module):
    def __init__(self, in_channels=[128], tasks=None, train_cfg=None, test_cfg=None, bbox_coder=None, common_heads=dict(),
                 loss_cls=dict(type="GaussianFocalLoss", reduction="mean"),
                 loss_bbox=dict(type="L1Loss", reduction="none", loss_weight=0.25),
                 separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3), share_conv_channel=64, num_heatmap_convs=2,
                 conv_cfg=dict(type="Conv2d"), norm_cfg=dict(type="BN2d"), bias="auto", norm_bbox=True, init_cfg=None):
        assert init_cfg is None, "To prevent abnormal initialization behavior, init_cfg is not allowed to be set"
        super().__init__()
        from . import heads  # noqa: F401  (fills the coder and loss registries the config blocks are built from)

        num_classes = [len(t) for t in tasks]
        self.class_names = [t for t in tasks]
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.norm_bbox = norm_bbox

        self.loss_cls = build_from_cfg(loss_cls, LOSSES) if isinstance(loss_cls, dict) else loss_cls
        self.loss_bbox = build_from_cfg(loss_bbox, LOSSES) if isinstance(loss_bbox, dict) else loss_bbox
        self.bbox_coder = build_from_cfg(bbox_coder, BBOX_CODERS) if isinstance(bbox_coder, dict) else bbox_coder
        self.num_anchor_per_locs = [n for n in num_classes]
        self.fp16_enabled = False

        self.shared_conv = ConvModule(in_channels, share_conv_channel, kernel_size=3, padding=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                                      bias=bias)
        self.share_conv_channel = share_conv_channel
        self.task_heads = nn.ModuleList()
        for num_cls in num_classes:
            heads_cfg = {k: tuple(v) for k, v in copy.deepcopy(common_heads).items()}
            heads_cfg.update(dict(heatmap=(num_cls, num_heatmap_convs)))
            cfg = copy.deepcopy(separate_head)      # the reference updates the caller's dict in place
            cfg.update(in_channels=share_conv_channel, heads=heads_cfg, num_cls=num_cls)
            self.task_heads.append(build_from_cfg(cfg, HEADS))

        self.use_fused = True   # eval mode: every head of every task in one launch (False: the torch layers)
        # eval mode: shared_conv runs with cudnn.benchmark off and cudnn.deterministic on (process-wide flags, set around the call
        # and restored); False leaves the caller's flags alone and gives up bit-equal calls
        self.deterministic_convs = True

    @property
    def use_fused(self):
        return self._use_fused

    @use_fused.setter
    def use_fused(self, value):
        """One switch for the head and for every task's SeparateHead."""
        self._use_fused = bool(value)
        for task in self.task_heads:
            if hasattr(task, "use_fused"):
                task.use_fused = bool(value)

    def init_weights(self):
        for task in self.task_heads:
            task.init_weights()

    # ---- forward ----
    def _foldable(self):
        tasks = list(self.task_heads)
        if not 1 <= len(tasks) <= CH_MAX_TASKS or not all(type(t) is SeparateHead for t in tasks):
            return False
        if any(t.final_kernel != tasks[0].final_kernel or t.in_channels != self.share_conv_channel for t in tasks):
            return False
        return all(t._foldable() for t in tasks)

    def fusable(self, x):
        """True when forward_single(x) runs the fused kernel for the task heads (x: the input of the head, before shared_conv)."""
        if not (self.use_fused and not self.training and torch.is_tensor(x) and x.dim() == 4 and _fusable_input(x, x.shape[1])):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return self._foldable()

    def folded(self):
        """`FoldedCenterHeads` of all tasks; cache and caveat as `SeparateHead.folded`."""
        return _cached_fold(self, list(self.task_heads))

    def forward_single(self, x):
        """x [B, in_channels, H, W] -> per task {head: [B, c, H, W]}."""
        fused = self.fusable(x)
        det = self.deterministic_convs and not self.training and torch.is_tensor(x) and x.is_cuda
        with _deterministic_convs() if det else contextlib.nullcontext():
            x = self.shared_conv(x)
        if fused:
            folded = self.folded()
            if folded.packed.device != x.device:
                raise RuntimeError("module parameters and x live on different devices")
            res = center_heads_forward(x, folded)
            if res is not None:
                return [dict(zip(task.heads, tensors)) for task, tensors in zip(self.task_heads, res)]
        return [task(x) for task in self.task_heads]

    def forward(self, feats, metas=None):
        """feats: [B, in_channels, H, W] or a list of levels -> the reference's multi_apply shape: a tuple over tasks of lists over
        levels of dicts, so preds_dicts[task][0] is the task's dict of the first level."""
        if isinstance(feats, torch.Tensor):
            feats = [feats]
        results = [self.forward_single(f) for f in feats]
        return tuple(map(list, zip(*results)))

    # ---- the ends ----
    def get_targets(self, gt_bboxes_3d, gt_labels_3d, **kwargs):
        from .heads import centerhead_get_targets

        if self.train_cfg is None:
            raise RuntimeError("get_targets needs the head's train_cfg")
        return centerhead_get_targets(gt_bboxes_3d, gt_labels_3d, self.num_classes, self.train_cfg, norm_bbox=self.norm_bbox, **kwargs)

    def loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, **kwargs):
        """-> {heatmap/task{t}, bbox/task{t}} (centerpoint.py:632-633)."""
        from .heads import centerhead_loss

        targets = self.get_targets(gt_bboxes_3d, gt_labels_3d, **kwargs)
        code_weights = _get(self.train_cfg, "code_weights")
        extra = {} if code_weights is None else dict(code_weights=code_weights)
        return centerhead_loss(preds_dicts, targets, loss_cls=self.loss_cls, loss_bbox=self.loss_bbox, **extra)

    def get_bboxes(self, preds_dicts, metas=None, img=None, rescale=False, sync=True):
        from .heads import centerhead_get_bboxes

        ret = centerhead_get_bboxes(preds_dicts, self.bbox_coder, self.test_cfg, self.num_classes, norm_bbox=self.norm_bbox, sync=sync)
        if not sync or metas is None:
            return ret
        out = []
        for i, r in enumerate(ret):
            box_type = metas[i].get("box_type_3d") if i < len(metas) else None
            boxes = box_type(r["bboxes"], box_dim=r["bboxes"].shape[-1]) if box_type is not None else r["bboxes"]
            out.append([boxes, r["scores"], r["labels"]])
        return out


register_everywhere("head", SeparateHead)
register_everywhere("head", CenterHead)
