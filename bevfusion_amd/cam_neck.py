"""The camera necks as modules: `GeneralizedLSSFPN` (reference: mmdet3d/models/necks/generalized_lss.py) and `LSSFPN`
(models/necks/lss.py), registered in `registry.NECKS` under the reference's names, so that the `encoders.camera.neck:` and
`decoder.neck:` blocks of its YAMLs build.  `heads` re-exports everything here.

Module trees and state-dict keys are the reference's (`lateral_convs.<i>.conv.weight`, `lateral_convs.<i>.bn.*`,
`fpn_convs.<i>.conv.weight`, `fpn_convs.<i>.bn.*`; `fuse.{0,1,3,4}.*`, `upsample.{1,2}.*`), so `load_state_dict(strict=True)` takes
its checkpoints' `encoders.camera.neck.*` and `decoder.neck.*`.

Per level the reference runs F.interpolate(bilinear, align_corners=True), torch.cat, a 1x1 layer and a 3x3 layer: eight launches,
with the upsampled map and the concatenation written and read once each.  Dispatch, per module, as `bev_trunk.SECOND` does:

  * GPU fp16 or bf16 tensors of the parameters' dtype, eval mode, no gradient needed, `use_fused`, `upsample_cfg` bilinear with
    align_corners=True: per level TWO launches.  The 1x1 layer is one `cam_neck_conv_forward` (`bevamd_neck_conv_forward`,
    csrc/ext/cam_neck.hip), which resamples the coarser map and concatenates while it stages its input tile: no upsampled tensor
    and no `cat` exist.  The 3x3 layer is one `bev_trunk.bev_conv_forward`.  `LSSFPN` with `scale_factor > 1` adds a third launch,
    `cam_neck_conv_forward` with kernel 3 on the map resampled to floor(scale_factor * size), as nn.Upsample sizes it.  The
    resampled value is rounded once to the storage type, as F.interpolate on a 16-bit tensor does; BatchNorm is NOT folded into
    the 16-bit weights.  A layer the kernels do not serve (see `neck_layer_spec`) runs through its torch layers inside the fused
    chain.  `fusable(inputs)` is True when at least one layer goes through a kernel.
  * otherwise (train mode, host tensors, fp32 tensors, a gradient, `use_fused = False`, another `upsample_cfg`): the module's own
    torch layers in the reference's order, with autograd, batch statistics and running-stat updates.

Memory formats of what `forward` returns.  Torch path: whatever the torch layers return.  Fused path: logical [B, C, H, W] tensors
with channels-last strides (an NHWC buffer permuted), as `SECOND` returns them: `cam_nets` reads them in place, and
`x.view(B, N, C, H, W)` of the model still works on them (the leading dimension is contiguous).  Inputs with channels-last strides
or contiguous NCHW are read in place, each source in its own layout; anything else is made contiguous NCHW first.

There is no host sync anywhere in `forward`; intermediates come from `torch.empty` per call and no workspace is cached, so in eval
mode `forward` can be captured in a `torch.cuda.graph` after one warm-up forward (which builds the folds).

`use_fused` defaults follow the measurement in DESIGN 3.25 (tools/bench_cam_neck.py, profiles/cam_neck_timing.json): True for both
modules.  The torch layers win one cell there, a channels-last twin of GeneralizedLSSFPN on channels-last inputs at one frame
(0.24 against 0.28 ms); on the contiguous NCHW maps a backbone hands over they take 2.05 ms.
"""
import math

import torch
from torch import nn
from torch.nn import functional as F

from . import _capi
from .bev_trunk import (FoldedBevLayer, _DTYPES, _as_source, _empty, _fusable_tensor, _is_nhwc, _no_grad_needed, bev_conv_forward,
                        bev_pack_weight, fold_bev_layer)
from .cam_nets import _bn_ok, _cached, _plain_conv, fold_conv_bias_bn
from .registry import NECKS, register_everywhere  # noqa: F401
from .transfusion_head import ConvModule

__all__ = ["GeneralizedLSSFPN", "LSSFPN", "cam_neck_conv_forward", "fold_conv_bias", "fold_neck_layer", "neck_layer_spec",
           "upsample_size"]

_UNSUPPORTED = 4          # BEVAMD_ERR_UNSUPPORTED


# ---- which layers the kernel serves, and their folds -----------------------------------------------------------------------------
def neck_layer_spec(conv, bn=None):
    """The kernel size (1 or 3) of a (Conv2d with or without bias, optional eval-mode BatchNorm2d) pair `cam_neck_conv_forward`
    serves, else None: 1x1 padding 0 or 3x3 padding 1, stride 1, no dilation, no groups; out_channels a multiple of 32 and
    in_channels a multiple of 16."""
    if bn is not None and (not _bn_ok(bn) or bn.num_features != conv.out_channels):
        return None
    if not _plain_conv(conv) or conv.out_channels % 32 or conv.out_channels < 32 or conv.in_channels % 16 or conv.in_channels < 16:
        return None
    if conv.stride != (1, 1):
        return None
    if conv.kernel_size == (1, 1) and conv.padding == (0, 0):
        return 1
    if conv.kernel_size == (3, 3) and conv.padding == (1, 1):
        return 3
    return None


def fold_conv_bias(conv):
    """`FoldedBevLayer` of a convolution WITHOUT a BatchNorm behind it (`no_norm_on_lateral=True`): scale is ones, shift is the
    bias (zeros without one), both fp32; the weights are packed with `bev_pack_weight` in the parameters' 16-bit dtype.  Cached on
    `conv` on the tensors' addresses and versions, as `bev_trunk.fold_bev_layer` is."""
    kernel = neck_layer_spec(conv)
    if kernel is None:
        raise RuntimeError(f"the neck convolution kernel does not serve {conv}")
    dtype = conv.weight.dtype
    if dtype not in _DTYPES:
        raise RuntimeError(f"the fused path takes float16 or bfloat16 weights, got {dtype} (fp32 belongs to the torch layers)")

    def make():
        w = conv.weight.detach()
        shift = conv.bias.detach().to(torch.float32).contiguous() if conv.bias is not None else \
            torch.zeros(conv.out_channels, dtype=torch.float32, device=w.device)
        return FoldedBevLayer(bev_pack_weight(w, "conv"), torch.ones(conv.out_channels, dtype=torch.float32, device=w.device), shift,
                              conv.in_channels, conv.out_channels, kernel, 1, "conv")
    return _cached(conv, "_bevamd_neck_folded", dtype, [conv.weight, conv.bias], (), make)


def fold_neck_layer(conv, bn=None):
    """The fold of a served layer: `fold_bev_layer` (no bias, BatchNorm), `cam_nets.fold_conv_bias_bn` (bias and BatchNorm) or
    `fold_conv_bias` (no BatchNorm)."""
    if bn is None:
        return fold_conv_bias(conv)
    if conv.bias is None:
        return fold_bev_layer(conv, bn)
    return fold_conv_bias_bn(conv, bn, conv.weight.dtype)


def upsample_size(size, scale_factor):
    """The output map of nn.Upsample(scale_factor=...): floor(scale_factor * size) per axis."""
    return tuple(int(math.floor(float(s) * float(scale_factor))) for s in size)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def cam_neck_conv_forward(srcs, fold, *, out_size=None, relu=True, out=None, out_channel_offset=0, out_layout="nhwc"):
    """One fused layer.  srcs: one or two [B, c_i, h_i, w_i] fp16 / bf16 tensors on the device, each with its OWN map; the layer's
    input is the channel concatenation, in the order given, of every source brought to `out_size`: a source of that map is copied,
    any other is resampled bilinearly with align_corners=True (fp32, rounded once to the storage type).  out_size: (H, W) of the
    output; None: the map of the FIRST source.  A source with channels-last strides is read in place as NHWC and a contiguous one
    as NCHW, each on its own; anything else is made contiguous NCHW.  fold: a `FoldedBevLayer` of the same dtype and device with
    kernel 1 or 3, stride 1, mode "conv"; relu: apply the ReLU.  out: a logical [B, C_total, H, W] tensor, contiguous NCHW or with
    channels-last strides, of which the channels [out_channel_offset, out_channel_offset + Cout) are written and nothing else;
    None: a fresh [B, Cout, H, W] in `out_layout` ("nhwc": channels-last strides, "nchw": contiguous).  Returns out, or None where
    the kernel does not serve the sizes.  No sync, no host copy."""
    if torch.is_tensor(srcs):
        srcs = [srcs]
    srcs = list(srcs)
    if not 1 <= len(srcs) <= 2:
        raise RuntimeError(f"cam_neck_conv_forward takes one or two sources, got {len(srcs)}")
    x0 = srcs[0]
    if any(not torch.is_tensor(t) or not t.is_cuda for t in srcs):
        raise RuntimeError("cam_neck_conv_forward needs GPU tensors (host tensors: the module's torch layers)")
    if any(t.dim() != 4 or t.dtype != x0.dtype or t.device != x0.device or t.shape[0] != x0.shape[0] or min(t.shape[2:]) < 1
           for t in srcs) or x0.dtype not in _DTYPES:
        raise RuntimeError(f"sources must be float16 or bfloat16 [B, c, h, w] of one dtype, device and batch, got "
                           f"{[(tuple(t.shape), t.dtype) for t in srcs]}")
    if fold.mode != "conv" or fold.stride != 1 or fold.kernel not in (1, 3):
        raise RuntimeError(f"the fold must be a convolution with kernel 1 or 3 and stride 1, got ({fold.mode}, {fold.kernel}, {fold.stride})")
    if out_layout not in ("nhwc", "nchw"):
        raise RuntimeError(f"out_layout is 'nhwc' or 'nchw', got {out_layout!r}")
    dev = x0.device
    for t in (fold.packed, fold.scale, fold.shift):
        if t.device != dev or not t.is_contiguous():
            raise RuntimeError("the fold must be contiguous on the device of the sources")
    if fold.packed.dtype != x0.dtype or fold.scale.dtype != torch.float32 or fold.shift.dtype != torch.float32:
        raise RuntimeError(f"the fold holds {fold.packed.dtype} weights, the sources are {x0.dtype}")
    if fold.scale.numel() != fold.out_channels or fold.shift.numel() != fold.out_channels:
        raise RuntimeError("scale and shift must hold out_channels floats")
    if sum(t.shape[1] for t in srcs) != fold.in_channels:
        raise RuntimeError(f"the sources have {[t.shape[1] for t in srcs]} channels, the fold takes {fold.in_channels}")
    OH, OW = (int(v) for v in (out_size if out_size is not None else x0.shape[2:]))
    if OH < 1 or OW < 1:
        raise RuntimeError(f"out_size must be at least 1 x 1, got {(OH, OW)}")
    srcs = [_as_source(t) for t in srcs]
    layouts = [0 if t.is_contiguous() else 1 for t in srcs]
    B = x0.shape[0]
    if out is None:
        out = _empty((B, fold.out_channels, OH, OW), x0.dtype, dev, out_layout)
    if out.device != dev or out.dtype != x0.dtype or out.dim() != 4 or out.shape[0] != B or tuple(out.shape[2:]) != (OH, OW):
        raise RuntimeError(f"out must be a {x0.dtype} [{B}, C, {OH}, {OW}] on the device of the sources, got {tuple(out.shape)} {out.dtype}")
    if out.is_contiguous():
        dst_nhwc = 0
    elif _is_nhwc(out):
        dst_nhwc = 1
    else:
        raise RuntimeError("out must be contiguous NCHW or have channels-last strides")
    second = srcs[1] if len(srcs) == 2 else None
    s1 = (second.shape[1], second.shape[2], second.shape[3], layouts[1]) if second is not None else (0, 0, 0, 0)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_neck_conv_forward(
            _capi.ptr(srcs[0]), srcs[0].shape[1], srcs[0].shape[2], srcs[0].shape[3], layouts[0], _capi.ptr(second), *s1,
            _DTYPES[x0.dtype], B, OH, OW, fold.out_channels, fold.kernel, _capi.ptr(fold.packed), fold.packed.numel(),
            _capi.ptr(fold.scale), _capi.ptr(fold.shift), int(bool(relu)), _capi.ptr(out), out.shape[1], int(out_channel_offset),
            dst_nhwc, out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "neck_conv_forward")
    return out


def _fused_neck_layer(conv, bn, relu, srcs, out_size=None):
    """(conv, bn or None, ReLU or not) over the resampled concatenation of `srcs` through a kernel, or None where none serves it.
    A 3x3 layer with BatchNorm and ReLU on one source of the output's map is `bev_conv_forward`'s; everything else goes to
    `cam_neck_conv_forward`."""
    if neck_layer_spec(conv, bn) is None or any(t.shape[1] % 16 for t in srcs):
        return None
    srcs = [_as_source(t) for t in srcs]
    fold = fold_neck_layer(conv, bn)
    plain = len(srcs) == 1 and (out_size is None or tuple(out_size) == tuple(srcs[0].shape[2:]))
    if plain and relu and fold.kernel == 3:
        return bev_conv_forward(srcs, fold, out_layout="nhwc")
    return cam_neck_conv_forward(srcs, fold, out_size=out_size, relu=relu, out_layout="nhwc")


def _bilinear_aligned(cfg):
    return dict(cfg) == dict(mode="bilinear", align_corners=True)


# ---- modules ---------------------------------------------------------------------------------------------------------------------
class GeneralizedLSSFPN(nn.Module):
    """necks/generalized_lss.py: top down, per level F.interpolate of the coarser map to the level's, `cat` (level first), a 1x1
    ConvModule and a 3x3 ConvModule.  forward(list of [B, c_i, H_i, W_i]) -> tuple of the len(inputs) - 1 finest levels; fused path:
    every output has channels-last strides."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, no_norm_on_lateral=False, conv_cfg=None,
                 norm_cfg=dict(type="BN2d"), act_cfg=dict(type="ReLU"), upsample_cfg=dict(mode="bilinear", align_corners=True)):
        super().__init__()
        assert isinstance(in_channels, list)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.fp16_enabled = False
        self.upsample_cfg = upsample_cfg.copy()
        if end_level == -1:
            self.backbone_end_level = self.num_ins - 1
        else:
            self.backbone_end_level = end_level
            assert end_level <= len(in_channels)
            assert num_outs == end_level - start_level
        self.start_level = start_level
        self.end_level = end_level
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(
                in_channels[i] + (in_channels[i + 1] if i == self.backbone_end_level - 1 else out_channels), out_channels, 1,
                conv_cfg=conv_cfg, norm_cfg=norm_cfg if not self.no_norm_on_lateral else None, act_cfg=act_cfg, inplace=False))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                                             act_cfg=act_cfg, inplace=False))
        self.use_fused = True    # eval mode on GPU fp16 / bf16 tensors: two launches per level (False: the torch layers); DESIGN 3.25

    def init_weights(self):
        """The reference gives the neck no init_cfg: torch's own initialisation stays."""

    def _served(self, m):
        return neck_layer_spec(m.conv, m.norm) is not None

    def fusable(self, inputs):
        """True when forward(inputs) runs the fused chain: at least one layer goes through a kernel; the layers the kernels do not
        serve run through their torch layers inside the chain.  False: every layer runs through torch."""
        if not (self.use_fused and not self.training and isinstance(inputs, (list, tuple)) and len(inputs) == len(self.in_channels)
                and len(inputs) >= 2 and _bilinear_aligned(self.upsample_cfg) and len(self.lateral_convs) > 0):
            return False
        weight = getattr(self.lateral_convs[0].conv, "weight", None)
        if not all(_fusable_tensor(t, weight) for t in inputs) or any(t.shape[0] != inputs[0].shape[0] for t in inputs):
            return False
        if not _no_grad_needed(self, inputs):
            return False
        return any(self._served(m) for m in list(self.lateral_convs) + list(self.fpn_convs))

    def forward(self, inputs):
        assert len(inputs) == len(self.in_channels)
        fused = self.fusable(inputs)
        laterals = [inputs[i + self.start_level] for i in range(len(inputs))]
        used_backbone_levels = len(laterals) - 1
        for i in range(used_backbone_levels - 1, -1, -1):
            lat, fpn = self.lateral_convs[i], self.fpn_convs[i]
            y = _fused_neck_layer(lat.conv, lat.norm, lat.with_activation, [laterals[i], laterals[i + 1]]) if fused else None
            if y is None:
                x = F.interpolate(laterals[i + 1], size=laterals[i].shape[2:], **self.upsample_cfg)
                y = lat(torch.cat([laterals[i], x], dim=1))
            z = _fused_neck_layer(fpn.conv, fpn.norm, fpn.with_activation, [y]) if fused else None
            laterals[i] = z if z is not None else fpn(y)
        return tuple(laterals[i] for i in range(used_backbone_levels))


class LSSFPN(nn.Module):
    """necks/lss.py: x[in_indices[0]] resampled to the map of x[in_indices[1]], `cat` (the resampled one first), Conv2d 1x1 +
    BatchNorm2d + ReLU, Conv2d 3x3 + BatchNorm2d + ReLU and, with scale_factor > 1, nn.Upsample(bilinear, align_corners=True) +
    Conv2d 3x3 + BatchNorm2d + ReLU.  forward(list of [B, c_i, H_i, W_i]) -> [B, out_channels, H, W]; fused path: channels-last
    strides."""

    def __init__(self, in_indices, in_channels, out_channels, scale_factor=1):
        super().__init__()
        self.in_indices = in_indices
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.scale_factor = scale_factor
        self.fuse = nn.Sequential(
            nn.Conv2d(in_channels[0] + in_channels[1], out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True),
            nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
        if scale_factor > 1:
            self.upsample = nn.Sequential(
                nn.Upsample(scale_factor=scale_factor, mode="bilinear", align_corners=True),
                nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
        self.use_fused = True    # eval mode on GPU fp16 / bf16 tensors: two or three launches (False: the torch layers); DESIGN 3.25

    def init_weights(self):
        """The reference gives the neck no init_cfg: torch's own initialisation stays."""

    def _pairs(self):
        pairs = [(self.fuse[0], self.fuse[1]), (self.fuse[3], self.fuse[4])]
        if self.scale_factor > 1:
            pairs.append((self.upsample[1], self.upsample[2]))
        return pairs

    def fusable(self, x):
        """True when forward(x) runs the fused chain (at least one layer through a kernel), False: every layer through torch."""
        if not (self.use_fused and not self.training and isinstance(x, (list, tuple))):
            return False
        try:
            x1, x2 = x[self.in_indices[0]], x[self.in_indices[1]]
        except IndexError:
            return False
        if not all(_fusable_tensor(t, self.fuse[0].weight) for t in (x1, x2)) or x1.shape[0] != x2.shape[0]:
            return False
        if not _no_grad_needed(self, [x1, x2]):
            return False
        return any(neck_layer_spec(c, n) is not None for c, n in self._pairs())

    def forward(self, x):
        fused = self.fusable(x)
        x1 = x[self.in_indices[0]]
        assert x1.shape[1] == self.in_channels[0]
        x2 = x[self.in_indices[1]]
        assert x2.shape[1] == self.in_channels[1]
        if not fused:
            x1 = F.interpolate(x1, size=x2.shape[-2:], mode="bilinear", align_corners=True)
            x = self.fuse(torch.cat([x1, x2], dim=1))
            if self.scale_factor > 1:
                x = self.upsample(x)
            return x
        y = _fused_neck_layer(self.fuse[0], self.fuse[1], True, [x1, x2], out_size=tuple(x2.shape[-2:]))
        if y is None:
            y = self.fuse[:3](torch.cat([F.interpolate(x1, size=x2.shape[-2:], mode="bilinear", align_corners=True), x2], dim=1))
        z = _fused_neck_layer(self.fuse[3], self.fuse[4], True, [y])
        y = z if z is not None else self.fuse[3:](y)
        if self.scale_factor > 1:
            z = _fused_neck_layer(self.upsample[1], self.upsample[2], True, [y], out_size=upsample_size(y.shape[-2:], self.scale_factor))
            y = z if z is not None else self.upsample(y)
        return y


register_everywhere("neck", GeneralizedLSSFPN)
register_everywhere("neck", LSSFPN)
