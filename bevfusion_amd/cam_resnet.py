"""`ResNet`, the `encoders.camera.backbone` of the reference's `centerhead/lssfpn/camera/256x704/resnet` and `camera+radar/resnet50`
configs, registered in `registry.BACKBONES` under the reference's name.  The configs mean mmdet 2.x's
mmdet/models/backbones/resnet.py, which the reference imports and does not vendor; `ResNet` and `Bottleneck` are written after it,
over the `BasicBlock` of `bev_resnet` for depths 18 and 34.  `heads` re-exports everything here.

Module tree and state-dict keys are torchvision's (`conv1.weight`, `bn1.*`, `layer<i>.<j>.conv{1,2,3}.weight`,
`layer<i>.<j>.bn{1,2,3}.*`, `layer<i>.0.downsample.{0,1}.*`), so `load_state_dict(strict=True)` takes a `torchvision://resnet50`
state dict with its `fc.*` keys removed and a BEVFusion checkpoint's `encoders.camera.backbone.*`.  A `Pretrained` `init_cfg` (or
`pretrained=`) is RECORDED on the module and never fetched: nothing here opens a URL or a file; load the weights with
`load_state_dict`.

Dispatch, as `GeneralizedResNet` does it:

  * GPU fp16 or bf16 tensors of the parameters' dtype, eval mode, no gradient needed, `use_fused`: the stem (conv 7x7 stride 2 + bn1
    + ReLU + MaxPool 3x3 stride 2) is ONE launch of `bevamd_resnet_stem_forward` (csrc/ext/resnet_stem.hip); per Bottleneck conv1 +
    bn1 + ReLU and conv2 + bn2 + ReLU are one launch each of `bevamd_bev_conv_forward` (bev_trunk.bev_conv_forward) and conv3 + bn3
    + residual (identity, or the 1x1 downsample + its BatchNorm) + ReLU is ONE launch of `bevamd_bottleneck_tail_forward`
    (csrc/ext/bottleneck.hip); a BasicBlock runs as in `GeneralizedResNet` (`res_block_forward`).  All are implicit GEMMs on the
    16-bit MFMA with fp32 accumulation, BatchNorm applied in fp32 and NOT folded into the 16-bit weights, one rounding per kernel.
    A part the kernels do not serve (see `stem_spec`, `layer_spec`, `bottleneck_spec`: a dilated conv2, a `caffe`-style stride-2
    conv1, widths off the multiples) or that the class switches send to torch runs through its torch layers inside the chain.
    `fusable(x)` is True when at least one part goes through a kernel.
  * otherwise (train mode, host tensors, fp32 tensors, a gradient, `use_fused = False`): the torch layers in mmdet's order, with
    autograd, batch statistics and running-stat updates.

Fused outputs are logical [N, C, H, W] tensors with channels-last strides (which `SECONDFPN` reads in place).  No host sync;
intermediates come from `torch.empty` per call and no workspace is cached, so the eval forward can be captured in a
`torch.cuda.graph` after one warm-up forward (which builds the folds).

The class switches `use_fused`, `fused_stem`, `fused_stride2` (conv2 at stride 2 through `bev_conv_forward`) and `fused_tails`
(which classes of Bottleneck / BasicBlock tail go through a kernel: "identity", "down1", "down2") follow DESIGN 3.27.
"""
from dataclasses import dataclass

import torch
from torch import nn

from . import _capi
from .bev_resnet import BasicBlock, _bn_served, _layout, _scale_shift, _tail_class, fold_res_block, res_block_forward, res_block_spec
from .bev_trunk import (_DTYPES, _as_source, _empty, _fusable_tensor, _fused_layer, _is_nhwc, _no_grad_needed, _tensor_key, bev_pack_weight,
                        layer_spec)
from .registry import BACKBONES, build_conv_layer, build_norm_layer, register_everywhere  # noqa: F401

__all__ = ["ResNet", "Bottleneck", "FoldedBottleneckTail", "FoldedStem", "bottleneck_spec", "fold_bottleneck",
           "bottleneck_tail_forward", "stem_spec", "fold_stem", "stem_forward", "stem_pack_weight", "stem_unpack_weight"]

_UNSUPPORTED = 4          # BEVAMD_ERR_UNSUPPORTED
STEM_PACKED_ELEMS = 4 * 6 * 64 * 8
_DEFAULT_NORM = dict(type="BN", requires_grad=True)


# ---- mmdet/models/backbones/resnet.py: the Bottleneck ----------------------------------------------------------------------------
class Bottleneck(nn.Module):
    """mmdet 2.x's Bottleneck: conv 1x1 + norm + ReLU, conv 3x3 (padding = dilation) + norm + ReLU, conv 1x1 to 4 planes + norm, the
    residual (x, or downsample(x)) added, ReLU.  style "pytorch" puts the stride on conv2, "caffe" on conv1."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style="pytorch", with_cp=False, conv_cfg=None,
                 norm_cfg=None, dcn=None, plugins=None):
        super().__init__()
        assert style in ["pytorch", "caffe"]
        for name, val in (("with_cp", with_cp), ("dcn", dcn), ("plugins", plugins)):
            if val:
                raise NotImplementedError(f"Bottleneck: {name} is not supported")
        norm_cfg = dict(_DEFAULT_NORM) if norm_cfg is None else norm_cfg
        self.inplanes, self.planes, self.stride, self.dilation, self.style = inplanes, planes, stride, dilation, style
        self.conv1_stride, self.conv2_stride = (1, stride) if style == "pytorch" else (stride, 1)
        self.conv1 = build_conv_layer(conv_cfg, inplanes, planes, kernel_size=1, stride=self.conv1_stride, bias=False)
        self.bn1 = build_norm_layer(norm_cfg, planes, postfix=1)[1]
        self.conv2 = build_conv_layer(conv_cfg, planes, planes, kernel_size=3, stride=self.conv2_stride, padding=dilation,
                                      dilation=dilation, bias=False)
        self.bn2 = build_norm_layer(norm_cfg, planes, postfix=2)[1]
        self.conv3 = build_conv_layer(conv_cfg, planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = build_norm_layer(norm_cfg, planes * self.expansion, postfix=3)[1]
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def _make_stage(block, inplanes, planes, num_blocks, stride, dilation, style, conv_cfg, norm_cfg):
    """mmdet's ResLayer without avg_down: the first block carries the stride and, when stride != 1 or the widths differ, a
    downsample = Sequential(conv 1x1 stride, norm)."""
    def make(inp, s, down):
        if block is Bottleneck:
            return Bottleneck(inp, planes, s, dilation, down, style=style, conv_cfg=conv_cfg, norm_cfg=norm_cfg)
        blk = BasicBlock(inp, planes, s, dilation, down, style=style)
        blk.bn1 = build_norm_layer(norm_cfg, planes, postfix=1)[1]       # the same slots, the configured norm
        blk.bn2 = build_norm_layer(norm_cfg, planes, postfix=2)[1]
        return blk
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = nn.Sequential(build_conv_layer(conv_cfg, inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                   build_norm_layer(norm_cfg, planes * block.expansion)[1])
    layers = [make(inplanes, stride, downsample)]
    for _ in range(1, num_blocks):
        layers.append(make(planes * block.expansion, 1, None))
    return nn.Sequential(*layers)


# ---- which Bottleneck tails the kernel serves ------------------------------------------------------------------------------------
def _plain_1x1(conv, strides=((1, 1),)):
    return type(conv) is nn.Conv2d and conv.bias is None and conv.groups == 1 and conv.dilation == (1, 1) \
        and conv.kernel_size == (1, 1) and conv.padding == (0, 0) and conv.padding_mode == "zeros" and conv.stride in strides


def bottleneck_spec(block):
    """("identity", 1) or ("downsample", stride) of a block whose tail (conv3, bn3, residual, ReLU) the kernel serves, else None.
    Served: conv3 a Conv2d 1x1 stride 1 without bias, groups, dilation or padding, P -> C with P a multiple of 16 and C a multiple
    of 32; bn3 and the downsample's BatchNorm2d in eval mode with running statistics; downsample None (the block's input then has C
    channels and the output's map) or Sequential(Conv2d 1x1 stride 1 or 2 without bias or padding, BatchNorm2d) from a multiple of
    16 channels."""
    conv3, bn3 = getattr(block, "conv3", None), getattr(block, "bn3", None)
    if not _plain_1x1(conv3):
        return None
    P, C = conv3.in_channels, conv3.out_channels
    if C < 32 or C % 32 or P < 16 or P % 16 or not _bn_served(bn3, C):
        return None
    down = getattr(block, "downsample", None)
    if down is None:
        conv1, conv2 = getattr(block, "conv1", None), getattr(block, "conv2", None)
        if not isinstance(conv1, nn.Conv2d) or not isinstance(conv2, nn.Conv2d) or conv1.in_channels != C:
            return None
        if conv1.stride != (1, 1) or conv2.stride != (1, 1):
            return None
        return ("identity", 1)
    if type(down) is not nn.Sequential or len(down) != 2:
        return None
    conv, bn = down[0], down[1]
    if not _plain_1x1(conv, ((1, 1), (2, 2))):
        return None
    if conv.out_channels != C or conv.in_channels < 16 or conv.in_channels % 16 or not _bn_served(bn, C):
        return None
    return ("downsample", conv.stride[0])


@dataclass
class FoldedBottleneckTail:
    """The tail of one eval-mode Bottleneck in the kernel's layout.  packed3: conv3's weight, packed_d: the downsample's 1x1 weight
    (None: identity), flat 16-bit in fragment order (`bev_pack_weight`, one tap); scale3, shift3, scale_d, shift_d: [C] fp32 (scale
    = bn.weight / sqrt(running_var + eps), shift = bn.bias - running_mean * scale, computed in float64 and each rounded once)."""
    packed3: torch.Tensor
    scale3: torch.Tensor
    shift3: torch.Tensor
    packed_d: torch.Tensor
    scale_d: torch.Tensor
    shift_d: torch.Tensor
    planes: int
    channels: int
    x_channels: int
    residual: str
    stride: int


def _cache_key(tensors, bns):
    return _tensor_key(tensors) + tuple(bn.eps for bn in bns)


def _fold_tail(block):
    spec = bottleneck_spec(block)
    if spec is None:
        raise RuntimeError(f"the Bottleneck tail kernel does not serve the tail of {block}")
    residual, stride = spec
    w3 = block.conv3.weight.detach()
    if w3.dtype not in _DTYPES:
        raise RuntimeError(f"the fused path takes float16 or bfloat16 weights, got {w3.dtype} (fp32 belongs to the torch layers)")
    s3, t3 = _scale_shift(block.bn3)
    P, C = block.conv3.in_channels, block.conv3.out_channels
    if residual == "identity":
        return FoldedBottleneckTail(bev_pack_weight(w3), s3, t3, None, None, None, P, C, C, residual, 1)
    conv, bn = block.downsample[0], block.downsample[1]
    sd, td = _scale_shift(bn)
    return FoldedBottleneckTail(bev_pack_weight(w3), s3, t3, bev_pack_weight(conv.weight.detach()), sd, td, P, C, conv.in_channels,
                                residual, stride)


def fold_bottleneck(block):
    """`FoldedBottleneckTail` of an eval-mode block on the parameters' device, cached on `block` on the tensors' addresses and
    versions (see `fold_bev_layer` for what moves a version).  Run one forward before capturing a graph."""
    bns = [block.bn3] + ([block.downsample[1]] if block.downsample is not None else [])
    tensors = [block.conv3.weight] + ([block.downsample[0].weight] if block.downsample is not None else [])
    for bn in bns:
        tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    key = _cache_key(tensors, bns)
    cache = block.__dict__.get("_bevamd_folded_tail")
    if cache is not None and cache[0] == key:
        return cache[1]
    val = _fold_tail(block)
    block.__dict__["_bevamd_folded_tail"] = (key, val)
    return val


def bottleneck_tail_forward(h, x, fold, *, out_layout="nhwc"):
    """The tail of a Bottleneck in one launch: relu(bn3(conv3(h)) + residual(x)).  h [B, P, OH, OW] (conv2 + bn2 + ReLU) and x
    [B, Cx, Hx, Wx] (the block's input): fp16 / bf16 device tensors of one dtype, each contiguous NCHW or with channels-last strides
    and read in place.  fold: a `FoldedBottleneckTail` of the same dtype and device.  Returns a fresh [B, C, OH, OW] in `out_layout`
    ("nhwc": channels-last strides, "nchw": contiguous), or None where the kernel does not serve the sizes.  No sync, no host copy."""
    if not torch.is_tensor(h) or not torch.is_tensor(x) or not h.is_cuda or not x.is_cuda:
        raise RuntimeError("bottleneck_tail_forward needs GPU tensors (host tensors: the module's torch layers)")
    if h.dim() != 4 or x.dim() != 4 or h.dtype != x.dtype or h.device != x.device or h.shape[0] != x.shape[0] or h.dtype not in _DTYPES:
        raise RuntimeError(f"h and x must be float16 or bfloat16 [B, c, H, W] of one dtype, device and batch, got "
                           f"{tuple(h.shape)} {h.dtype} and {tuple(x.shape)} {x.dtype}")
    if out_layout not in ("nhwc", "nchw"):
        raise RuntimeError(f"out_layout is 'nhwc' or 'nchw', got {out_layout!r}")
    dev = h.device
    down = fold.residual == "downsample"
    parts = [fold.packed3, fold.scale3, fold.shift3] + ([fold.packed_d, fold.scale_d, fold.shift_d] if down else [])
    for t in parts:
        if t is None or t.device != dev or not t.is_contiguous():
            raise RuntimeError("the fold must be contiguous on the device of the tensors")
    if any(t.dtype != h.dtype for t in parts[0::3]) or any(t.dtype != torch.float32 for t in parts[1::3] + parts[2::3]):
        raise RuntimeError(f"the fold holds {fold.packed3.dtype} weights and {fold.scale3.dtype} scales, the tensors are {h.dtype}")
    if any(t.numel() != fold.channels for t in parts[1::3] + parts[2::3]):
        raise RuntimeError("scales and shifts must hold `channels` floats")
    B, P, OH, OW = h.shape
    Cx, Hx, Wx = x.shape[1:]
    s, C = fold.stride, fold.channels
    if P != fold.planes or Cx != fold.x_channels or (OH, OW) != ((Hx - 1) // s + 1, (Wx - 1) // s + 1):
        raise RuntimeError(f"h {tuple(h.shape)} and x {tuple(x.shape)} do not fit the fold ({fold.planes} planes, {fold.x_channels} -> "
                           f"{fold.channels} channels, {fold.residual}, stride {s})")
    h, h_nhwc = _layout(h, "h")
    x, x_nhwc = _layout(x, "x")
    out = _empty((B, C, OH, OW), h.dtype, dev, out_layout)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_bottleneck_tail_forward(
            _capi.ptr(h), h_nhwc, P, _capi.ptr(x), x_nhwc, Cx, Hx, Wx, _DTYPES[h.dtype], B, C, OH, OW, int(down), s,
            _capi.ptr(fold.packed3), fold.packed3.numel(), _capi.ptr(fold.scale3), _capi.ptr(fold.shift3),
            _capi.ptr(fold.packed_d) if down else None, fold.packed_d.numel() if down else 0,
            _capi.ptr(fold.scale_d) if down else None, _capi.ptr(fold.shift_d) if down else None, _capi.ptr(out),
            int(out_layout == "nhwc"), out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "bottleneck_tail_forward")
    return out


# ---- the stem --------------------------------------------------------------------------------------------------------------------
def stem_pack_weight(w):
    """Conv2d weight [64, 3, 7, 7] -> the A-fragment order of v_mfma_f32_16x16x32 over K = 192, flat [mt 4][kstep 6][lane 64][j 8]:
    the element is w[co = 16 mt + (lane & 15)][ci][ky][kx = j] with pair = 7 ci + ky = 4 kstep + (lane >> 4); zero at the padding
    positions kx = 7 and pair >= 21 (12288 - 64 * 147 = 2880 elements).  A lane's fragment is one 16-byte load;
    the matching B fragment is 8 consecutive input pixels of row (ci, 2 cy + ky)."""
    if w.dim() != 4 or tuple(w.shape) != (64, 3, 7, 7):
        raise RuntimeError(f"the stem kernel takes a [64, 3, 7, 7] weight, got {tuple(w.shape)}")
    wk = w.new_zeros(64, 24, 8)
    wk[:, :21, :7] = w.reshape(64, 21, 7)
    wk = wk.reshape(4, 16, 6, 4, 8)                              # [mt][row][kstep][h][j]
    return wk.permute(0, 2, 3, 1, 4).reshape(-1).contiguous()    # [mt][kstep][h][row][j], lane = 16 h + row


def stem_unpack_weight(flat):
    """The inverse of `stem_pack_weight`: flat [12288] -> [64, 3, 7, 7] (the padding positions are dropped)."""
    wk = flat.reshape(4, 6, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(64, 24, 8)
    return wk[:, :21, :7].reshape(64, 3, 7, 7).contiguous()


def stem_spec(conv, bn, pool):
    """(7, 2, 3) = (kernel, stride, padding) of a stem the kernel serves, else None.  Served: Conv2d 3 -> 64, 7x7 stride 2 padding 3
    without bias, groups or dilation; a BatchNorm2d of 64 channels in eval mode with running statistics; MaxPool2d 3x3 stride 2
    padding 1 without dilation, `ceil_mode` or indices."""
    if type(conv) is not nn.Conv2d or conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1) or conv.padding_mode != "zeros":
        return None
    if (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) != (3, 64, (7, 7), (2, 2), (3, 3)):
        return None
    if not _bn_served(bn, 64) or type(pool) is not nn.MaxPool2d:
        return None
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)      # noqa: E731
    if (pair(pool.kernel_size), pair(pool.stride), pair(pool.padding), pair(pool.dilation)) != ((3, 3), (2, 2), (1, 1), (1, 1)):
        return None
    if pool.ceil_mode or pool.return_indices:
        return None
    return (7, 2, 3)


@dataclass
class FoldedStem:
    """An eval-mode stem in the kernel's layout.  packed: conv1's weight in `stem_pack_weight`'s order; scale, shift: [64] fp32 from
    float64, as in `FoldedResBlock`."""
    packed: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


def fold_stem(conv, bn, pool):
    """`FoldedStem` of an eval-mode (conv1, bn1, maxpool) on the parameters' device, cached on `conv` on the tensors' addresses and
    versions like `fold_res_block`.  Run one forward before capturing a graph."""
    if stem_spec(conv, bn, pool) is None:
        raise RuntimeError(f"the stem kernel does not serve {conv}, {bn}, {pool}")
    key = _cache_key([conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var], [bn])
    cache = conv.__dict__.get("_bevamd_folded_stem")
    if cache is not None and cache[0] == key:
        return cache[1]
    w = conv.weight.detach()
    if w.dtype not in _DTYPES:
        raise RuntimeError(f"the fused path takes float16 or bfloat16 weights, got {w.dtype} (fp32 belongs to the torch layers)")
    scale, shift = _scale_shift(bn)
    val = FoldedStem(stem_pack_weight(w), scale, shift)
    conv.__dict__["_bevamd_folded_stem"] = (key, val)
    return val


def stem_forward(x, fold, *, out_layout="nhwc"):
    """The stem in one launch: maxpool(relu(bn1(conv1(x)))).  x [N, 3, H, W]: an fp16 / bf16 device tensor, read in place when
    contiguous NCHW (anything else is made contiguous first).  fold: a `FoldedStem` of the same dtype and device.  Returns a fresh
    [N, 64, PH, PW] in `out_layout` ("nhwc": channels-last strides, "nchw": contiguous), or None where the kernel does not serve
    the sizes (an input that does not have 3 channels).  No sync, no host copy."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("stem_forward needs a GPU tensor (host tensors: the module's torch layers)")
    if x.dim() != 4 or x.dtype not in _DTYPES:
        raise RuntimeError(f"x must be a float16 or bfloat16 [N, 3, H, W], got {tuple(x.shape)} {x.dtype}")
    if out_layout not in ("nhwc", "nchw"):
        raise RuntimeError(f"out_layout is 'nhwc' or 'nchw', got {out_layout!r}")
    dev = x.device
    for t in (fold.packed, fold.scale, fold.shift):
        if t.device != dev or not t.is_contiguous():
            raise RuntimeError("the fold must be contiguous on the device of the tensors")
    if fold.packed.dtype != x.dtype or fold.scale.dtype != torch.float32 or fold.shift.dtype != torch.float32:
        raise RuntimeError(f"the fold holds {fold.packed.dtype} weights and {fold.scale.dtype} scales, the tensor is {x.dtype}")
    if fold.packed.numel() != STEM_PACKED_ELEMS or fold.scale.numel() != 64 or fold.shift.numel() != 64:
        raise RuntimeError(f"the fold must hold {STEM_PACKED_ELEMS} packed weights and 64 scales and shifts")
    x = x.detach().contiguous()
    N, cin, H, W = x.shape
    if H < 1 or W < 1:
        raise RuntimeError(f"x must have a map of at least 1 x 1, got {tuple(x.shape)}")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = _empty((N, 64, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1), x.dtype, dev, out_layout)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_resnet_stem_forward(
            _capi.ptr(x), _DTYPES[x.dtype], N, cin, H, W, 64, 7, 2, 3, 3, 2, 1, 0, _capi.ptr(fold.packed), fold.packed.numel(),
            _capi.ptr(fold.scale), _capi.ptr(fold.shift), _capi.ptr(out), int(out_layout == "nhwc"), out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "stem_forward")
    return out


# ---- the module ------------------------------------------------------------------------------------------------------------------
class ResNet(nn.Module):
    """mmdet 2.x's ResNet backbone.  forward(x [N, in_channels, H, W]) -> tuple of the `out_indices` stage outputs (stage i at
    1 / 2^(i+2) of the image with the default strides); fused path: every output has channels-last strides.

    `deep_stem`, `avg_down`, `dcn`, `plugins`, `with_cp` and a `conv_cfg` other than None / Conv2d raise NotImplementedError.  A
    `Pretrained` init_cfg (or `pretrained`) is recorded in `self.init_cfg` and NOT fetched: `init_weights()` then leaves the weights
    alone, and the checkpoint is loaded with `load_state_dict`.  Nothing here opens a URL."""

    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)), 50: (Bottleneck, (3, 4, 6, 3)),
                     101: (Bottleneck, (3, 4, 23, 3)), 152: (Bottleneck, (3, 8, 36, 3))}

    # defaults from the measurement in DESIGN 3.27
    use_fused = True            # eval mode on GPU fp16 / bf16 tensors: the fused chain (False: the torch layers)
    fused_stem = True           # the stem through stem_forward (False: its torch layers inside the chain)
    fused_stride2 = True        # conv2 (BasicBlock: conv1) at stride 2 through bev_conv_forward too
    fused_tails = ("identity", "down1", "down2")     # the tail classes that go through a tail kernel

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style="pytorch", deep_stem=False, avg_down=False, frozen_stages=-1,
                 conv_cfg=None, norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True, pretrained=None,
                 init_cfg=None):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError(f"invalid depth {depth} for resnet")
        for name, val in (("deep_stem", deep_stem), ("avg_down", avg_down), ("dcn", dcn), ("plugins", plugins), ("with_cp", with_cp)):
            if val:
                raise NotImplementedError(f"ResNet: {name} is not supported")
        if conv_cfg is not None and dict(conv_cfg) != dict(type="Conv2d"):
            raise NotImplementedError(f"ResNet: conv_cfg {conv_cfg} is not supported (None or Conv2d)")
        if init_cfg and pretrained:
            raise AssertionError("init_cfg and pretrained cannot be specified at the same time")
        if isinstance(pretrained, str):
            init_cfg = dict(type="Pretrained", checkpoint=pretrained)
        elif pretrained is not None:
            raise TypeError("pretrained must be a str or None")
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages
        if stem_channels is None:
            stem_channels = base_channels
        self.depth, self.in_channels, self.stem_channels, self.base_channels = depth, in_channels, stem_channels, base_channels
        self.num_stages, self.strides, self.dilations, self.out_indices = num_stages, tuple(strides), tuple(dilations), tuple(out_indices)
        self.style, self.frozen_stages, self.norm_eval, self.zero_init_residual = style, frozen_stages, norm_eval, zero_init_residual
        self.conv_cfg, self.norm_cfg, self.init_cfg = conv_cfg, norm_cfg, init_cfg
        self.block, stage_blocks = self.arch_settings[depth]
        self.stage_blocks = stage_blocks[:num_stages]

        self.conv1 = build_conv_layer(conv_cfg, in_channels, stem_channels, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = build_norm_layer(norm_cfg, stem_channels, postfix=1)[1]
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = stem_channels
        for i, num_blocks in enumerate(self.stage_blocks):
            planes = base_channels * 2 ** i
            name = f"layer{i + 1}"
            self.add_module(name, _make_stage(self.block, inplanes, planes, num_blocks, strides[i], dilations[i], style, conv_cfg, norm_cfg))
            inplanes = planes * self.block.expansion
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self._freeze_stages()

    # ---- mmdet's training behaviour ----
    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in (self.conv1, self.bn1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, f"layer{i}")
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()
        return self

    def init_weights(self):
        """mmdet's default: Kaiming (fan_out, relu) for the convolutions, 1 for the norms' weights and 0 for their biases, then 0
        for the last norm of every block when `zero_init_residual`.  With a `Pretrained` init_cfg nothing is written and nothing
        is fetched."""
        if isinstance(self.init_cfg, dict) and self.init_cfg.get("type") == "Pretrained":
            return
        if self.init_cfg is not None:
            raise NotImplementedError(f"ResNet: init_cfg {self.init_cfg} is not supported (None or Pretrained)")
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, a=0, mode="fan_out", nonlinearity="relu")
                    if m.bias is not None:
                        m.bias.zero_()
                elif isinstance(m, (nn.modules.batchnorm._BatchNorm, nn.GroupNorm)):
                    if m.weight is not None:
                        m.weight.fill_(1.0)
                    if m.bias is not None:
                        m.bias.zero_()
            if self.zero_init_residual:
                for blk in self._all_blocks():
                    last = blk.bn3 if isinstance(blk, Bottleneck) else blk.bn2
                    if last.weight is not None:
                        last.weight.zero_()

    # ---- dispatch ----
    def _stages(self):
        return [getattr(self, name) for name in self.res_layers]

    def _all_blocks(self):
        return [blk for stage in self._stages() for blk in stage]

    def _stem_wanted(self):
        return self.fused_stem and stem_spec(self.conv1, self.bn1, self.maxpool) is not None

    def _conv_wanted(self, conv, bn):
        """(conv, bn, ReLU) goes through bev_conv_forward: it is served and, at stride 2, `fused_stride2` is set."""
        return layer_spec(conv, bn) is not None and (self.fused_stride2 or conv.stride == (1, 1))

    def _tail_wanted(self, blk):
        spec = bottleneck_spec(blk) if isinstance(blk, Bottleneck) else res_block_spec(blk)
        return spec is not None and _tail_class(spec) in self.fused_tails

    def _block_wanted(self, blk):
        if self._tail_wanted(blk) or self._conv_wanted(blk.conv1, blk.bn1):
            return True
        return isinstance(blk, Bottleneck) and self._conv_wanted(blk.conv2, blk.bn2)

    def fusable(self, x):
        """True when forward(x) runs the fused chain: at least one part (the stem, a conv + norm + ReLU, a block tail) goes through a
        kernel; the parts the kernels do not serve run through their torch layers inside the chain.  False: every layer runs through
        torch."""
        if not (self.use_fused and not self.training and _fusable_tensor(x, self.conv1.weight) and _no_grad_needed(self, [x])):
            return False
        return (self._stem_wanted() and x.shape[1] == 3) or any(self._block_wanted(b) for b in self._all_blocks())

    def _fused_stem(self, x):
        y = None
        if self._stem_wanted() and x.shape[1] == 3:
            y = stem_forward(x, fold_stem(self.conv1, self.bn1, self.maxpool), out_layout="nhwc")
        if y is None:
            y = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return y

    def _fused_conv(self, conv, bn, relu, x):
        h = _fused_layer(conv, bn, [x], out_layout="nhwc") if self._conv_wanted(conv, bn) else None
        return relu(bn(conv(x))) if h is None else h

    def _fused_block(self, blk, x):
        h = self._fused_conv(blk.conv1, blk.bn1, blk.relu, x)
        bottleneck = isinstance(blk, Bottleneck)
        if bottleneck:
            h = self._fused_conv(blk.conv2, blk.bn2, blk.relu, _as_source(h))
        y = None
        if self._tail_wanted(blk) and (h.is_contiguous() or _is_nhwc(h)):
            fold = fold_bottleneck(blk) if bottleneck else fold_res_block(blk)
            if tuple(h.shape[2:]) == ((x.shape[2] - 1) // fold.stride + 1, (x.shape[3] - 1) // fold.stride + 1) \
                    and x.shape[1] == fold.x_channels:
                y = (bottleneck_tail_forward if bottleneck else res_block_forward)(h, x, fold, out_layout="nhwc")
        if y is None:
            out = blk.bn3(blk.conv3(h)) if bottleneck else blk.bn2(blk.conv2(h))
            out += blk.downsample(x) if blk.downsample is not None else x
            y = blk.relu(out)
        return y

    def forward(self, x):
        outs = []
        if self.fusable(x):
            x = _as_source(self._fused_stem(_as_source(x)))
            for i, stage in enumerate(self._stages()):
                for blk in stage:
                    x = _as_source(self._fused_block(blk, x))
                if i in self.out_indices:
                    outs.append(x)
            return tuple(outs)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        for i, stage in enumerate(self._stages()):
            x = stage(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)


register_everywhere("backbone", ResNet)
