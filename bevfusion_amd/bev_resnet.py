"""`GeneralizedResNet` (reference: mmdet3d/models/backbones/resnet.py), the `decoder.backbone` of the camera-only, camera+radar and
BEV-segmentation-camera configs, registered in `registry.BACKBONES` under the reference's name; `BasicBlock` and `make_res_layer`
after mmcv 1.x's mmcv/cnn/resnet.py, which the reference imports.  `heads` re-exports everything here.

Module tree and state-dict keys are the reference's (`<stage>.<block>.conv1.weight`, `.bn1.*`, `.conv2.weight`, `.bn2.*`,
`<stage>.0.downsample.0.weight`, `<stage>.0.downsample.1.*`), so `load_state_dict(strict=True)` takes a checkpoint's
`decoder.backbone.*`.

Dispatch, as `SECOND` does it:

  * GPU fp16 or bf16 tensors of the parameters' dtype, eval mode, no gradient needed, `use_fused`: per block, conv1 + bn1 + ReLU is
    one launch of `bevamd_bev_conv_forward` (bev_trunk.bev_conv_forward; its stride-2 case only with `fused_stride2`), and conv2 +
    bn2 + residual (identity, or the 1x1 downsample + its BatchNorm) + ReLU is ONE launch of `bevamd_res_block_forward`
    (csrc/ext/res_block.hip): implicit GEMM on the 16-bit MFMA with fp32 accumulation, `y = relu(acc2 * s2 + t2 + r)` in fp32
    rounded once; BatchNorm is NOT folded into the 16-bit weights.  A half the kernels do not serve (see `layer_spec`,
    `res_block_spec`) or that the class switches below send to torch runs through its torch layers inside the chain.
    `fusable(x)` is True when at least one half goes through a kernel.
  * otherwise (train mode, host tensors, fp32 tensors, a gradient, `use_fused = False`): the torch layers in the reference's order,
    with autograd, batch statistics and running-stat updates.

Fused outputs are logical [B, C, H, W] tensors with channels-last strides (which `LSSFPN` reads in place); inputs with
channels-last strides or contiguous NCHW are read in place.  No host sync; intermediates come from `torch.empty` per call and no
workspace is cached, so the eval forward can be captured in a `torch.cuda.graph` after one warm-up forward (which builds the folds).

The switches `use_fused`, `fused_stride2` (conv1 at stride 2 through the kernel) and `fused_tails` (which classes of block tail
go through `res_block_forward`: "identity", "down1", "down2") follow the measurement in DESIGN 3.26.
"""
from dataclasses import dataclass

import torch
from torch import nn

from . import _capi
from .bev_trunk import (_DTYPES, _as_source, _empty, _fusable_tensor, _fused_layer, _is_nhwc, _no_grad_needed, _tensor_key, bev_pack_weight,
                        layer_spec)
from .registry import BACKBONES, register_everywhere  # noqa: F401

__all__ = ["GeneralizedResNet", "BasicBlock", "make_res_layer", "FoldedResBlock", "fold_res_block", "res_block_forward",
           "res_block_spec"]

_UNSUPPORTED = 4          # BEVAMD_ERR_UNSUPPORTED


# ---- mmcv/cnn/resnet.py ----------------------------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    """mmcv 1.x's BasicBlock: conv3x3(stride, dilation) + BatchNorm2d + ReLU, conv3x3 + BatchNorm2d, the residual (x, or
    downsample(x)) added, ReLU."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style="pytorch", with_cp=False):
        super().__init__()
        assert style in ["pytorch", "caffe"]
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride
        self.dilation = dilation
        assert not with_cp

    def forward(self, x):
        residual = x
        out = self.conv1(x)
        out = self.bn1(out)
        out = self.relu(out)
        out = self.conv2(out)
        out = self.bn2(out)
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        out = self.relu(out)
        return out


def make_res_layer(block, inplanes, planes, blocks, stride=1, dilation=1, style="pytorch", with_cp=False):
    """mmcv 1.x's make_res_layer: `blocks` blocks; the first carries the stride and, when stride != 1 or the widths differ, a
    downsample = Sequential(Conv2d 1x1 stride, BatchNorm2d)."""
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                   nn.BatchNorm2d(planes * block.expansion))
    layers = [block(inplanes, planes, stride, dilation, downsample, style=style, with_cp=with_cp)]
    inplanes = planes * block.expansion
    for _ in range(1, blocks):
        layers.append(block(inplanes, planes, 1, dilation, style=style, with_cp=with_cp))
    return nn.Sequential(*layers)


# ---- which block tails the kernel serves -----------------------------------------------------------------------------------------
def _bn_served(bn, channels):
    return isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.running_mean is not None and bn.running_var is not None \
        and bn.num_features == channels


def res_block_spec(block):
    """("identity", 1) or ("downsample", stride) of a block whose tail (conv2, bn2, residual, ReLU) the kernel serves, else None.
    Served: conv2 a Conv2d 3x3 stride 1 padding 1 without bias, groups or dilation, C -> C with C a multiple of 32; bn2 and the
    downsample's BatchNorm2d in eval mode with running statistics; downsample None (the block's input then has C channels and the
    output's map: conv1 at stride 1, padding = dilation) or Sequential(Conv2d 1x1 stride 1 or 2 without bias or padding,
    BatchNorm2d) from a multiple of 16 channels."""
    conv2, bn2 = getattr(block, "conv2", None), getattr(block, "bn2", None)
    if type(conv2) is not nn.Conv2d or conv2.bias is not None or conv2.groups != 1 or conv2.dilation != (1, 1):
        return None
    if conv2.kernel_size != (3, 3) or conv2.stride != (1, 1) or conv2.padding != (1, 1) or conv2.padding_mode != "zeros":
        return None
    C = conv2.out_channels
    if conv2.in_channels != C or C < 32 or C % 32 or not _bn_served(bn2, C):
        return None
    down = getattr(block, "downsample", None)
    if down is None:
        return ("identity", 1)
    if type(down) is not nn.Sequential or len(down) != 2:
        return None
    conv, bn = down[0], down[1]
    if type(conv) is not nn.Conv2d or conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1):
        return None
    if conv.kernel_size != (1, 1) or conv.padding != (0, 0) or conv.stride not in ((1, 1), (2, 2)) or conv.padding_mode != "zeros":
        return None
    if conv.out_channels != C or conv.in_channels < 16 or conv.in_channels % 16 or not _bn_served(bn, C):
        return None
    return ("downsample", conv.stride[0])


@dataclass
class FoldedResBlock:
    """The tail of one eval-mode BasicBlock in the kernel's layout.  packed2: conv2's weight, packed_d: the downsample's 1x1 weight
    (None: identity), flat 16-bit in fragment order (`bev_pack_weight`); scale2, shift2, scale_d, shift_d: [C] fp32 (scale =
    bn.weight / sqrt(running_var + eps), shift = bn.bias - running_mean * scale, computed in float64 and each rounded once)."""
    packed2: torch.Tensor
    scale2: torch.Tensor
    shift2: torch.Tensor
    packed_d: torch.Tensor
    scale_d: torch.Tensor
    shift_d: torch.Tensor
    channels: int
    x_channels: int
    residual: str
    stride: int


def _scale_shift(bn):
    f64 = lambda t: t.detach().to(torch.float64)      # noqa: E731
    inv = 1.0 / torch.sqrt(f64(bn.running_var) + bn.eps)
    scale = f64(bn.weight) * inv if bn.weight is not None else inv
    shift = (f64(bn.bias) if bn.bias is not None else torch.zeros_like(inv)) - f64(bn.running_mean) * scale
    return scale.to(torch.float32).contiguous(), shift.to(torch.float32).contiguous()


def _fold(block):
    spec = res_block_spec(block)
    if spec is None:
        raise RuntimeError(f"the residual block kernel does not serve the tail of {block}")
    residual, stride = spec
    w2 = block.conv2.weight.detach()
    if w2.dtype not in _DTYPES:
        raise RuntimeError(f"the fused path takes float16 or bfloat16 weights, got {w2.dtype} (fp32 belongs to the torch layers)")
    s2, t2 = _scale_shift(block.bn2)
    C = block.conv2.out_channels
    if residual == "identity":
        return FoldedResBlock(bev_pack_weight(w2), s2, t2, None, None, None, C, C, residual, 1)
    conv, bn = block.downsample[0], block.downsample[1]
    sd, td = _scale_shift(bn)
    return FoldedResBlock(bev_pack_weight(w2), s2, t2, bev_pack_weight(conv.weight.detach()), sd, td, C, conv.in_channels, residual,
                          stride)


def fold_res_block(block):
    """`FoldedResBlock` of an eval-mode block on the parameters' device, cached on `block` on the tensors' addresses and versions
    (see `fold_bev_layer` for what moves a version).  Run one forward before capturing a graph."""
    bns = [block.bn2] + ([block.downsample[1]] if block.downsample is not None else [])
    tensors = [block.conv2.weight] + ([block.downsample[0].weight] if block.downsample is not None else [])
    for bn in bns:
        tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    key = _tensor_key(tensors) + tuple(bn.eps for bn in bns)
    cache = block.__dict__.get("_bevamd_folded")
    if cache is not None and cache[0] == key:
        return cache[1]
    val = _fold(block)
    block.__dict__["_bevamd_folded"] = (key, val)
    return val


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _layout(t, what):
    """(tensor the kernel reads in place, its layout flag)."""
    t = t.detach()
    if t.is_contiguous():
        return t, 0
    if _is_nhwc(t):
        return t, 1
    raise RuntimeError(f"{what} must be contiguous NCHW or have channels-last strides")


def res_block_forward(h, x, fold, *, out_layout="nhwc"):
    """The tail of a BasicBlock in one launch: relu(bn2(conv2(h)) + residual(x)).  h [B, C, OH, OW] (conv1 + bn1 + ReLU of x) and x
    [B, Cx, Hx, Wx] (the block's input): fp16 / bf16 device tensors of one dtype, each contiguous NCHW or with channels-last strides
    and read in place.  fold: a `FoldedResBlock` of the same dtype and device.  Returns a fresh [B, C, OH, OW] in `out_layout`
    ("nhwc": channels-last strides, "nchw": contiguous), or None where the kernel does not serve the sizes.  No sync, no host copy."""
    if not torch.is_tensor(h) or not torch.is_tensor(x) or not h.is_cuda or not x.is_cuda:
        raise RuntimeError("res_block_forward needs GPU tensors (host tensors: the module's torch layers)")
    if h.dim() != 4 or x.dim() != 4 or h.dtype != x.dtype or h.device != x.device or h.shape[0] != x.shape[0] or h.dtype not in _DTYPES:
        raise RuntimeError(f"h and x must be float16 or bfloat16 [B, c, H, W] of one dtype, device and batch, got "
                           f"{tuple(h.shape)} {h.dtype} and {tuple(x.shape)} {x.dtype}")
    if out_layout not in ("nhwc", "nchw"):
        raise RuntimeError(f"out_layout is 'nhwc' or 'nchw', got {out_layout!r}")
    dev = h.device
    down = fold.residual == "downsample"
    parts = [fold.packed2, fold.scale2, fold.shift2] + ([fold.packed_d, fold.scale_d, fold.shift_d] if down else [])
    for t in parts:
        if t is None or t.device != dev or not t.is_contiguous():
            raise RuntimeError("the fold must be contiguous on the device of the tensors")
    if any(t.dtype != h.dtype for t in parts[0::3]) or any(t.dtype != torch.float32 for t in parts[1::3] + parts[2::3]):
        raise RuntimeError(f"the fold holds {fold.packed2.dtype} weights and {fold.scale2.dtype} scales, the tensors are {h.dtype}")
    if any(t.numel() != fold.channels for t in parts[1::3] + parts[2::3]):
        raise RuntimeError("scales and shifts must hold `channels` floats")
    B, C, OH, OW = h.shape
    Cx, Hx, Wx = x.shape[1:]
    s = fold.stride
    if C != fold.channels or Cx != fold.x_channels or (OH, OW) != ((Hx - 1) // s + 1, (Wx - 1) // s + 1):
        raise RuntimeError(f"h {tuple(h.shape)} and x {tuple(x.shape)} do not fit the fold ({fold.x_channels} -> {fold.channels} channels, "
                           f"{fold.residual}, stride {s})")
    h, h_nhwc = _layout(h, "h")
    x, x_nhwc = _layout(x, "x")
    out = _empty((B, C, OH, OW), h.dtype, dev, out_layout)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_res_block_forward(
            _capi.ptr(h), h_nhwc, _capi.ptr(x), x_nhwc, Cx, Hx, Wx, _DTYPES[h.dtype], B, C, OH, OW, int(down), s,
            _capi.ptr(fold.packed2), fold.packed2.numel(), _capi.ptr(fold.scale2), _capi.ptr(fold.shift2),
            _capi.ptr(fold.packed_d) if down else None, fold.packed_d.numel() if down else 0,
            _capi.ptr(fold.scale_d) if down else None, _capi.ptr(fold.shift_d) if down else None, _capi.ptr(out),
            int(out_layout == "nhwc"), out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "res_block_forward")
    return out


def _tail_class(spec):
    return "identity" if spec[0] == "identity" else f"down{spec[1]}"


# ---- the module ------------------------------------------------------------------------------------------------------------------
class GeneralizedResNet(nn.ModuleList):
    """backbones/resnet.py: per (num_blocks, out_channels, stride) of `blocks` one make_res_layer(BasicBlock, ...) stage.
    forward(x [B, in_channels, H, W]) -> list of the stage outputs; fused path: every output has channels-last strides."""

    def __init__(self, in_channels, blocks):
        super().__init__()
        self.in_channels = in_channels
        self.blocks = blocks
        for num_blocks, out_channels, stride in self.blocks:
            stage = make_res_layer(BasicBlock, in_channels, out_channels, num_blocks, stride=stride, dilation=1)
            in_channels = out_channels
            self.append(stage)
        # defaults from the measurement in DESIGN 3.26: at B = 8 the chain with every half through a kernel was the fastest path of
        # both width sets; sending the stride-2 conv1 to torch inside the chain (SECOND's default) was slower than either pure path
        self.use_fused = True         # eval mode on GPU fp16 / bf16 tensors: two launches per block (False: the torch layers)
        self.fused_stride2 = True     # conv1 at stride 2 through bev_conv_forward too (False: its torch layers inside the chain)
        self.fused_tails = ("identity", "down1", "down2")     # the tail classes that go through res_block_forward

    def init_weights(self):
        """The reference gives GeneralizedResNet no init_cfg: torch's own initialisation stays."""

    def _all_blocks(self):
        return [blk for stage in self for blk in stage]

    def _head_wanted(self, blk):
        """conv1 + bn1 + ReLU goes through bev_conv_forward: it is served and, at stride 2, `fused_stride2` is set."""
        return isinstance(blk, BasicBlock) and layer_spec(blk.conv1, blk.bn1) is not None \
            and (self.fused_stride2 or blk.conv1.stride == (1, 1))

    def _tail_wanted(self, blk):
        if not isinstance(blk, BasicBlock):
            return False
        spec = res_block_spec(blk)
        return spec is not None and _tail_class(spec) in self.fused_tails

    def fusable(self, x):
        """True when forward(x) runs the fused chain: at least one half of one block goes through a kernel; the halves the kernels
        do not serve run through their torch layers inside the chain.  False: every layer runs through torch."""
        blocks = self._all_blocks()
        if not blocks or not isinstance(blocks[0], BasicBlock):
            return False
        if not (self.use_fused and not self.training and _fusable_tensor(x, blocks[0].conv1.weight) and _no_grad_needed(self, [x])):
            return False
        return all(isinstance(b, BasicBlock) for b in blocks) and any(self._head_wanted(b) or self._tail_wanted(b) for b in blocks)

    def _fused_block(self, blk, x):
        h = _fused_layer(blk.conv1, blk.bn1, [x], out_layout="nhwc") if self._head_wanted(blk) else None
        if h is None:
            h = blk.relu(blk.bn1(blk.conv1(x)))
        y = None
        if self._tail_wanted(blk) and (h.is_contiguous() or _is_nhwc(h)):
            fold = fold_res_block(blk)
            if tuple(h.shape[2:]) == ((x.shape[2] - 1) // fold.stride + 1, (x.shape[3] - 1) // fold.stride + 1) \
                    and x.shape[1] == fold.x_channels:
                y = res_block_forward(h, x, fold, out_layout="nhwc")
        if y is None:
            out = blk.bn2(blk.conv2(h))
            out += blk.downsample(x) if blk.downsample is not None else x
            y = blk.relu(out)
        return y

    def forward(self, x):
        outputs = []
        if self.fusable(x):
            x = _as_source(x)
            for stage in self:
                for blk in stage:
                    x = _as_source(self._fused_block(blk, x))
                outputs.append(x)
            return outputs
        for module in self:
            x = module(x)
            outputs.append(x)
        return outputs


register_everywhere("backbone", GeneralizedResNet)
