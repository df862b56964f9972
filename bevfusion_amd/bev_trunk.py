"""The dense BEV trunk as modules: `ConvFuser` (reference: mmdet3d/models/fusers/conv.py), `SECOND` (models/backbones/second.py)
and `SECONDFPN` (models/necks/second.py), registered in `registry.FUSERS`, `registry.BACKBONES` and `registry.NECKS` under the
reference's names, so that the `fuser:`, `decoder.backbone:` and `decoder.neck:` blocks of its YAMLs build.  `heads` re-exports
everything here.

Module trees and state-dict keys are the reference's (`0.weight`, `1.*`; `blocks.<i>.<3j>.weight`, `blocks.<i>.<3j+1>.*`;
`deblocks.<i>.0.weight`, `deblocks.<i>.1.*`), so `load_state_dict(strict=True)` takes its checkpoints' `fuser.*`,
`decoder.backbone.*` and `decoder.neck.*`.

Dispatch, per module, as `CenterHead` does:

  * GPU fp16 or bf16 tensors of the parameters' dtype, eval mode, no gradient needed, `use_fused`: every (convolution, BatchNorm2d,
    ReLU) triple the kernel serves is ONE launch of `bevamd_bev_conv_forward` (csrc/ext/bev_conv.hip): implicit GEMM on the 16-bit
    MFMA with fp32 accumulation, `y = relu(acc * scale + shift)` in fp32 rounded once; BatchNorm is NOT folded into the 16-bit
    weights.  ConvFuser reads its inputs as one concatenated input (no `cat`), SECONDFPN writes every level into its channel window
    of the output (no `cat`).  A triple the kernel does not serve (see `layer_spec`) runs through its torch layers inside the
    fused chain: SECOND hands its result to the next layer, SECONDFPN copies it into the level's window.  `fusable(x)` is True
    when at least one layer goes through the kernel.
  * otherwise (train mode, host tensors, fp32 tensors, a gradient, `use_fused = False`): the module's own torch layers in the
    reference's order, with autograd, batch statistics and running-stat updates.

fp32 is NOT served by the fused path on purpose: gfx950 runs the fp32 MFMA at 1/16 of the fp16 rate, and fp32 convolutions of this
size belong to the vendor library.

Memory formats of what `forward` returns.  Torch path: whatever the torch layers return (contiguous NCHW for contiguous inputs).
Fused path: `ConvFuser` returns a logical [B, C, H, W] tensor with channels-last strides (an NHWC buffer permuted); `SECOND`
returns a tuple of such tensors; `SECONDFPN` returns `[out]` with `out` a contiguous NCHW [B, sum(C), H, W], which is what the
heads read.  `SECOND` and `SECONDFPN` recognise channels-last strides on their inputs and read them in place; any other input is
made contiguous NCHW (which the kernel transposes while staging).

There is no host sync anywhere in `forward`; intermediates come from `torch.empty` per call and no workspace is cached, so in eval
mode `forward` can be captured in a `torch.cuda.graph` after one warm-up forward (which builds the folds).

`use_fused` defaults follow the measurement in DESIGN 3.23 (tools/bench_bev_trunk.py, profiles/bev_trunk_timing.json): True for the
three modules, with `SECOND.fused_stride2 = False`: the stride-2 layer was slower through the kernel than through the vendor
library and runs through its torch layers inside the otherwise fused chain.
"""
from dataclasses import dataclass

import numpy as np
import torch
from torch import nn

from . import _capi
from .registry import BACKBONES, FUSERS, NECKS, build_conv_layer, build_norm_layer, build_upsample_layer, register_everywhere  # noqa: F401

__all__ = ["ConvFuser", "SECOND", "SECONDFPN", "FoldedBevLayer", "fold_bev_layer", "bev_conv_forward", "bev_pack_weight",
           "bev_unpack_weight", "layer_spec"]

_UNSUPPORTED = 4          # BEVAMD_ERR_UNSUPPORTED
BEV_CHUNK = 32            # channels of one staged chunk (BC_CK): Cin is padded with zeros to a multiple of it in the packed weights
BEV_TILE = (8, 16)        # output pixels (H, W) of one workgroup
_DTYPES = {torch.float16: 0, torch.bfloat16: 1}


# ---- the packed weight order -----------------------------------------------------------------------------------------------------
def _canonical(w, mode):
    """-> [groups, Cout, taps, Cin]: conv weight [Cout, Cin, k, k] (groups 1, taps k^2) or deconv weight [Cin, Cout, 2, 2] (groups 4
    = (dy, dx), taps 1)."""
    if mode == "deconv":
        cin, cout, kh, kw = w.shape
        return w.permute(2, 3, 1, 0).reshape(kh * kw, cout, 1, cin)
    cout, cin, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(1, cout, kh * kw, cin)


def bev_pack_weight(w, mode="conv"):
    """Conv2d weight [Cout, Cin, k, k] (mode "conv") or ConvTranspose2d weight [Cin, Cout, 2, 2] (mode "deconv") -> the A-fragment
    order of v_mfma_f32_16x16x32, flat: element [g][mt][chunk][tap][lane][j] is w[co = 16 mt + (lane & 15)][ci = 32 chunk +
    8 (lane >> 4) + j] of tap (ky, kx) = (tap // k, tap % k) (conv, g = 0) or of (dy, dx) = (g // 2, g % 2) (deconv, tap = 0); zero
    where ci >= Cin.  A lane's fragment is one 16-byte load."""
    wk = _canonical(w, mode)
    g, cout, taps, cin = wk.shape
    nch = -(-cin // BEV_CHUNK)
    if nch * BEV_CHUNK != cin:
        wk = torch.cat([wk, wk.new_zeros(g, cout, taps, nch * BEV_CHUNK - cin)], dim=3)
    wk = wk.reshape(g, cout // 16, 16, taps, nch, 4, 8)                  # [g][mt][row][tap][chunk][h][j]
    return wk.permute(0, 1, 4, 3, 5, 2, 6).reshape(-1).contiguous()      # [g][mt][chunk][tap][h][row][j], lane = 16 h + row


def bev_unpack_weight(flat, in_channels, out_channels, kernel, mode="conv"):
    """The inverse of `bev_pack_weight`: flat -> [Cout, Cin, k, k] (conv) or [Cin, Cout, 2, 2] (deconv)."""
    g, taps = (4, 1) if mode == "deconv" else (1, kernel * kernel)
    nch = -(-in_channels // BEV_CHUNK)
    wk = flat.reshape(g, out_channels // 16, nch, taps, 4, 16, 8).permute(0, 1, 5, 3, 2, 4, 6)
    wk = wk.reshape(g, out_channels, taps, nch * BEV_CHUNK)[..., :in_channels]
    if mode == "deconv":
        return wk.reshape(2, 2, out_channels, in_channels).permute(3, 2, 0, 1).contiguous()
    return wk.reshape(out_channels, kernel, kernel, in_channels).permute(0, 3, 1, 2).contiguous()


# ---- which layers the kernel serves ----------------------------------------------------------------------------------------------
def layer_spec(conv, bn=None):
    """(mode, kernel, stride) of a (convolution, BatchNorm2d) pair the kernel serves, else None.  Served: Conv2d 3x3 padding 1 stride
    1 or 2; Conv2d 1x1 stride 1; ConvTranspose2d with kernel = stride = 1 (a 1x1 convolution with the weight transposed) or 2; no
    bias, no dilation, no groups, zero padding mode; out_channels a multiple of 32 and in_channels a multiple of 16; a BatchNorm2d in
    eval mode with running statistics."""
    if bn is not None:
        if not isinstance(bn, nn.BatchNorm2d) or bn.training or bn.running_mean is None or bn.running_var is None:
            return None
    if type(conv) not in (nn.Conv2d, nn.ConvTranspose2d) or conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1):
        return None
    if conv.out_channels % 32 or conv.out_channels < 32 or conv.in_channels % 16 or conv.in_channels < 16:
        return None
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if type(conv) is nn.Conv2d:
        if conv.padding_mode != "zeros" or isinstance(p, str):
            return None
        if k == (3, 3) and p == (1, 1) and s in ((1, 1), (2, 2)):
            return ("conv", 3, s[0])
        if k == (1, 1) and p == (0, 0) and s == (1, 1):
            return ("conv", 1, 1)
        return None
    if p != (0, 0) or conv.output_padding != (0, 0):
        return None
    if k == (1, 1) and s == (1, 1):
        return ("conv", 1, 1)
    if k == (2, 2) and s == (2, 2):
        return ("deconv", 2, 2)
    return None


@dataclass
class FoldedBevLayer:
    """One eval-mode (convolution, BatchNorm2d, ReLU) triple in the kernel's layout.  packed: flat 16-bit weights in fragment order
    (`bev_pack_weight`); scale, shift: [Cout] fp32 (scale = bn.weight / sqrt(running_var + eps), shift = bn.bias - running_mean *
    scale, both computed in float64 from the float64 scale and each rounded once to fp32)."""
    packed: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    in_channels: int
    out_channels: int
    kernel: int
    stride: int
    mode: str


def _fold(conv, bn):
    spec = layer_spec(conv)
    if spec is None:
        raise RuntimeError(f"the BEV convolution kernel does not serve {conv}")
    mode, kernel, stride = spec
    w = conv.weight.detach()
    if w.dtype not in _DTYPES:
        raise RuntimeError(f"the fused path takes float16 or bfloat16 weights, got {w.dtype} (fp32 belongs to the torch layers)")
    if type(conv) is nn.ConvTranspose2d and mode == "conv":
        w = w.permute(1, 0, 2, 3)                      # kernel = stride = 1: a 1x1 convolution with the weight transposed
    f64 = lambda t: t.detach().to(torch.float64)      # noqa: E731
    inv = 1.0 / torch.sqrt(f64(bn.running_var) + bn.eps)
    scale = f64(bn.weight) * inv if bn.weight is not None else inv
    shift = (f64(bn.bias) if bn.bias is not None else torch.zeros_like(inv)) - f64(bn.running_mean) * scale
    return FoldedBevLayer(bev_pack_weight(w, mode), scale.to(torch.float32).contiguous(), shift.to(torch.float32).contiguous(),
                          conv.in_channels, conv.out_channels, kernel, stride, mode)


def fold_bev_layer(conv, bn):
    """`FoldedBevLayer` of an eval-mode (conv, bn) pair on the parameters' device, cached on `conv` on the tensors' addresses and
    versions.  Every in-place torch operation moves the version (`load_state_dict`, an optimizer step, `init_weights`); a write
    through `.data` does not, and after one the cache has to be dropped by hand (`del conv._bevamd_folded`).  Run one forward before
    capturing a graph: a fold computed inside a capture is filled only when the graph replays."""
    tensors = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    key = _tensor_key(tensors) + (bn.eps,)
    cache = conv.__dict__.get("_bevamd_folded")
    if cache is not None and cache[0] == key:
        return cache[1]
    val = _fold(conv, bn)
    conv.__dict__["_bevamd_folded"] = (key, val)
    return val


def _tensor_key(tensors):
    """What a cached fold is keyed on: the tensors' addresses and versions (None for an absent one)."""
    return tuple((t.data_ptr(), t._version, t.dtype, t.device) if t is not None else None for t in tensors)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _is_nhwc(t):
    return t.is_contiguous(memory_format=torch.channels_last)


def _as_source(t):
    """A tensor the kernel reads in place: contiguous NCHW or channels-last strides; anything else is made contiguous NCHW."""
    t = t.detach()
    return t if t.is_contiguous() or _is_nhwc(t) else t.contiguous()


def _empty(shape, dtype, dev, out_layout):
    """A fresh logical [B, C, H, W]: channels-last strides for "nhwc", contiguous otherwise."""
    B, C, H, W = shape
    if out_layout == "nhwc":
        return torch.empty((B, H, W, C), dtype=dtype, device=dev).permute(0, 3, 1, 2)
    return torch.empty((B, C, H, W), dtype=dtype, device=dev)


def bev_conv_forward(srcs, fold, *, stride=None, mode=None, out=None, out_channel_offset=0, out_layout="nhwc"):
    """One fused layer.  srcs: one or two [B, c_i, H, W] fp16 / bf16 tensors on the device, read as one channel-concatenated input;
    sources with channels-last strides are read in place as NHWC when all have them, otherwise all are read as contiguous NCHW.
    fold: a `FoldedBevLayer` of the same dtype and device; stride, mode: checked against the fold when given.  out: a logical
    [B, C_total, OH, OW] tensor, contiguous NCHW or with channels-last strides, of which the channels [out_channel_offset,
    out_channel_offset + Cout) are written and nothing else; None: a fresh [B, Cout, OH, OW] in `out_layout` ("nhwc": channels-last
    strides, "nchw": contiguous).  Returns out, or None where the kernel does not serve the sizes.  No sync, no host copy."""
    if torch.is_tensor(srcs):
        srcs = [srcs]
    srcs = list(srcs)
    if not 1 <= len(srcs) <= 2:
        raise RuntimeError(f"bev_conv_forward takes one or two sources, got {len(srcs)}")
    x0 = srcs[0]
    if any(not torch.is_tensor(t) or not t.is_cuda for t in srcs):
        raise RuntimeError("bev_conv_forward needs GPU tensors (host tensors: the module's torch layers)")
    if any(t.dim() != 4 or t.dtype != x0.dtype or t.device != x0.device or t.shape[0] != x0.shape[0] or t.shape[2:] != x0.shape[2:]
           for t in srcs) or x0.dtype not in _DTYPES:
        raise RuntimeError(f"sources must be float16 or bfloat16 [B, c, H, W] of one dtype, device and map, got "
                           f"{[(tuple(t.shape), t.dtype) for t in srcs]}")
    if (stride is not None and stride != fold.stride) or (mode is not None and mode != fold.mode):
        raise RuntimeError(f"stride {stride} / mode {mode} do not match the fold ({fold.stride}, {fold.mode})")
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
    srcs = [t.detach() for t in srcs]
    nhwc = all(_is_nhwc(t) for t in srcs)
    if not nhwc:
        srcs = [t.contiguous() for t in srcs]
    B, _, H, W = x0.shape
    if fold.mode == "deconv":
        OH, OW = 2 * H, 2 * W
    else:
        OH, OW = (H + 2 * (fold.kernel // 2) - fold.kernel) // fold.stride + 1, (W + 2 * (fold.kernel // 2) - fold.kernel) // fold.stride + 1
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
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_bev_conv_forward(
            _capi.ptr(srcs[0]), srcs[0].shape[1], _capi.ptr(second), second.shape[1] if second is not None else 0, int(nhwc),
            _DTYPES[x0.dtype], B, H, W, fold.out_channels, fold.kernel, fold.stride, 1 if fold.mode == "deconv" else 0,
            _capi.ptr(fold.packed), fold.packed.numel(), _capi.ptr(fold.scale), _capi.ptr(fold.shift), _capi.ptr(out), out.shape[1],
            int(out_channel_offset), dst_nhwc, out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "bev_conv_forward")
    return out


# ---- shared module machinery -----------------------------------------------------------------------------------------------------
def _fusable_tensor(x, weight):
    return torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _DTYPES and x.dtype == weight.dtype \
        and x.device == weight.device and x.shape[2] >= 1 and x.shape[3] >= 1


def _no_grad_needed(module, tensors):
    return not (torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters())))


def _fused_layer(conv, bn, srcs, **kwargs):
    """The triple through the kernel, or None where it does not serve it."""
    if layer_spec(conv, bn) is None or any(t.shape[1] % 16 for t in srcs):
        return None
    return bev_conv_forward(srcs, fold_bev_layer(conv, bn), **kwargs)


def _apply_init_cfg(module, init_cfg):
    """The part of mmcv's initialisers the reference's trunk uses, written under no_grad (the parameters' versions move, so the folds
    see it): Kaiming (kaiming_normal_, fan_out, relu, bias 0) and Constant (weight val, bias 0) on the layer types named."""
    cfgs = init_cfg if isinstance(init_cfg, (list, tuple)) else [init_cfg]
    with torch.no_grad():
        for cfg in cfgs:
            if not cfg:
                continue
            typ = cfg["type"]
            if typ == "Pretrained":
                raise RuntimeError("init_cfg Pretrained: load the checkpoint with load_state_dict")
            layers = cfg.get("layer", [])
            layers = [layers] if isinstance(layers, str) else list(layers)
            for m in module.modules():
                if type(m).__name__ not in layers:
                    continue
                if typ == "Kaiming":
                    nn.init.kaiming_normal_(m.weight, a=cfg.get("a", 0), mode=cfg.get("mode", "fan_out"),
                                            nonlinearity=cfg.get("nonlinearity", "relu"))
                elif typ == "Constant":
                    if getattr(m, "weight", None) is not None:
                        m.weight.fill_(cfg["val"])
                else:
                    raise KeyError(f"init_cfg type {typ} is not supported")
                if getattr(m, "bias", None) is not None:
                    m.bias.fill_(cfg.get("bias", 0))


# ---- modules ---------------------------------------------------------------------------------------------------------------------
class ConvFuser(nn.Sequential):
    """fusers/conv.py: Conv2d(sum(in_channels) -> out_channels, 3x3, padding 1, no bias), BatchNorm2d (torch defaults), ReLU over the
    channel concatenation of the inputs.  forward(list of [B, c_i, H, W]) -> [B, out_channels, H, W]; fused path: channels-last
    strides, the inputs are read in place (up to two; more are concatenated into the second source first)."""

    def __init__(self, in_channels, out_channels):
        self.in_channels = in_channels
        self.out_channels = out_channels
        super().__init__(nn.Conv2d(sum(in_channels), out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
        self.use_fused = True    # eval mode on GPU fp16 / bf16 tensors: one launch, no cat (False: the torch layers); DESIGN 3.23

    def init_weights(self):
        """The reference gives ConvFuser no init_cfg: torch's own initialisation stays."""

    def fusable(self, inputs):
        """True when forward(inputs) runs the fused kernel."""
        inputs = [inputs] if torch.is_tensor(inputs) else list(inputs)
        if not (self.use_fused and not self.training and inputs and all(_fusable_tensor(t, self[0].weight) for t in inputs)):
            return False
        if any(t.shape[1] % 16 for t in inputs) or layer_spec(self[0], self[1]) is None:
            return False
        return _no_grad_needed(self, inputs)

    def forward(self, inputs):
        inputs = [inputs] if torch.is_tensor(inputs) else list(inputs)
        if self.fusable(inputs):
            srcs = inputs if len(inputs) <= 2 else [inputs[0], torch.cat(inputs[1:], dim=1)]
            y = _fused_layer(self[0], self[1], srcs, out_layout="nhwc")
            if y is not None:
                return y
        return super().forward(torch.cat(inputs, dim=1))


class SECOND(nn.Module):
    """backbones/second.py: per stage Conv2d 3x3 (stride layer_strides[i], padding 1) + norm + ReLU followed by layer_nums[i] times
    Conv2d 3x3 + norm + ReLU.  forward(x [B, in_channels, H, W]) -> tuple of the stage outputs; fused path: every output has
    channels-last strides."""

    def __init__(self, in_channels=128, out_channels=[128, 128, 256], layer_nums=[3, 5, 5], layer_strides=[2, 2, 2],
                 norm_cfg=dict(type="BN", eps=1e-3, momentum=0.01), conv_cfg=dict(type="Conv2d", bias=False), init_cfg=None,
                 pretrained=None):
        super().__init__()
        assert len(layer_strides) == len(layer_nums)
        assert len(out_channels) == len(layer_nums)
        in_filters = [in_channels, *out_channels[:-1]]
        blocks = []
        for i, layer_num in enumerate(layer_nums):
            block = [build_conv_layer(conv_cfg, in_filters[i], out_channels[i], 3, stride=layer_strides[i], padding=1),
                     build_norm_layer(norm_cfg, out_channels[i])[1], nn.ReLU(inplace=True)]
            for _ in range(layer_num):
                block += [build_conv_layer(conv_cfg, out_channels[i], out_channels[i], 3, padding=1),
                          build_norm_layer(norm_cfg, out_channels[i])[1], nn.ReLU(inplace=True)]
            blocks.append(nn.Sequential(*block))
        self.blocks = nn.ModuleList(blocks)
        assert not (init_cfg and pretrained), "init_cfg and pretrained cannot be setting at the same time"
        if isinstance(pretrained, str):
            self.init_cfg = dict(type="Pretrained", checkpoint=pretrained)
        elif init_cfg is not None:
            self.init_cfg = init_cfg
        else:
            self.init_cfg = dict(type="Kaiming", layer="Conv2d")
        self.in_channels = in_channels
        # defaults from the measurement in DESIGN 3.23: the stride-1 layers are faster through the kernel, the stride-2 layer is not
        self.use_fused = True        # eval mode on GPU fp16 / bf16 tensors: one launch per layer (False: the torch layers)
        self.fused_stride2 = False   # the stride-2 layers too (False: they run through their torch layers inside the fused chain)

    def init_weights(self):
        _apply_init_cfg(self, self.init_cfg)

    def _triples(self):
        return [tuple(block[j:j + 3]) for block in self.blocks for j in range(0, len(block), 3)]

    def _wanted(self, conv, bn, relu):
        """The triple goes through the kernel: it is served and, at stride 2, `fused_stride2` is set."""
        return layer_spec(conv, bn) is not None and isinstance(relu, nn.ReLU) and (self.fused_stride2 or conv.stride == (1, 1))

    def fusable(self, x):
        """True when forward(x) runs the fused chain: at least one layer goes through the kernel (every served stride-1 layer, the
        served stride-2 layers too with `fused_stride2`); the layers the kernel does not serve run through their torch layers
        inside the chain.  False: every layer runs through torch."""
        first = self.blocks[0][0]
        if not (self.use_fused and not self.training and _fusable_tensor(x, getattr(first, "weight", None)) and _no_grad_needed(self, [x])):
            return False
        return all(len(block) % 3 == 0 for block in self.blocks) and any(self._wanted(c, n, r) for c, n, r in self._triples())

    def forward(self, x):
        outs = []
        if self.fusable(x):
            x = _as_source(x)
            for block in self.blocks:
                for j in range(0, len(block), 3):
                    wanted = self._wanted(block[j], block[j + 1], block[j + 2])
                    y = _fused_layer(block[j], block[j + 1], [x], out_layout="nhwc") if wanted else None
                    x = y if y is not None else block[j + 2](block[j + 1](block[j](x)))
                outs.append(x)
            return tuple(outs)
        for block in self.blocks:
            x = block(x)
            outs.append(x)
        return tuple(outs)


class SECONDFPN(nn.Module):
    """necks/second.py: per level an upsampling layer (upsample_strides[i] > 1, or 1 without use_conv_for_no_stride: `upsample_cfg`
    with kernel = stride = upsample_strides[i]; otherwise a convolution with kernel = stride = round(1 / upsample_strides[i])) + norm
    + ReLU, concatenated along the channels.  forward(list of [B, c_i, H_i, W_i]) -> [out]; fused path: `out` is a contiguous NCHW
    [B, sum(out_channels), H, W] into which every level writes its own channel window."""

    def __init__(self, in_channels=[128, 128, 256], out_channels=[256, 256, 256], upsample_strides=[1, 2, 4],
                 norm_cfg=dict(type="BN", eps=1e-3, momentum=0.01), upsample_cfg=dict(type="deconv", bias=False),
                 conv_cfg=dict(type="Conv2d", bias=False), use_conv_for_no_stride=False, init_cfg=None):
        super().__init__()
        assert len(out_channels) == len(upsample_strides) == len(in_channels)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.fp16_enabled = False
        deblocks = []
        for i, out_channel in enumerate(out_channels):
            stride = upsample_strides[i]
            if stride > 1 or (stride == 1 and not use_conv_for_no_stride):
                layer = build_upsample_layer(upsample_cfg, in_channels=in_channels[i], out_channels=out_channel,
                                             kernel_size=upsample_strides[i], stride=upsample_strides[i])
            else:
                stride = int(np.round(1 / stride).astype(np.int64))
                layer = build_conv_layer(conv_cfg, in_channels=in_channels[i], out_channels=out_channel, kernel_size=stride, stride=stride)
            deblocks.append(nn.Sequential(layer, build_norm_layer(norm_cfg, out_channel)[1], nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(deblocks)
        self.init_cfg = init_cfg if init_cfg is not None else [dict(type="Kaiming", layer="ConvTranspose2d"),
                                                               dict(type="Constant", layer="NaiveSyncBatchNorm2d", val=1.0)]
        self.use_fused = True    # eval mode on GPU fp16 / bf16 tensors: one launch per level, no cat (False: the torch layers); DESIGN 3.23

    def init_weights(self):
        _apply_init_cfg(self, self.init_cfg)

    def _served(self, i, t):
        return layer_spec(self.deblocks[i][0], self.deblocks[i][1]) is not None and t.shape[1] % 16 == 0

    def fusable(self, x):
        """True when forward(x) runs at least one level through the fused kernel; the levels it does not serve run through their
        torch layers and are copied into their channel window.  False: every level runs through torch, followed by `cat`."""
        if not (self.use_fused and not self.training and isinstance(x, (list, tuple)) and len(x) == len(self.deblocks)):
            return False
        if not all(_fusable_tensor(t, getattr(d[0], "weight", None)) for t, d in zip(x, self.deblocks)):
            return False
        if not _no_grad_needed(self, x) or any(t.shape[0] != x[0].shape[0] for t in x):
            return False
        return any(self._served(i, t) for i, t in enumerate(x))

    def forward(self, x):
        assert len(x) == len(self.in_channels)
        if self.fusable(x):
            # the unserved levels first, through torch: their results also give the output size
            ups = [None if self._served(i, t) else self.deblocks[i](t) for i, t in enumerate(x)]
            sizes = []
            for i, (t, u) in enumerate(zip(x, ups)):
                f = 2 if u is None and layer_spec(self.deblocks[i][0])[0] == "deconv" else 1
                sizes.append((t.shape[2] * f, t.shape[3] * f) if u is None else tuple(u.shape[2:]))
            if all(sz == sizes[0] for sz in sizes):
                total = sum(d[0].out_channels for d in self.deblocks)
                out = torch.empty((x[0].shape[0], total) + sizes[0], dtype=x[0].dtype, device=x[0].device)
                offset = 0
                for t, u, d in zip(x, ups, self.deblocks):
                    c = d[0].out_channels
                    if u is None:
                        u = _fused_layer(d[0], d[1], [_as_source(t)], out=out, out_channel_offset=offset)
                        if u is None:                      # refused by the entry point after all: this level through torch
                            out[:, offset:offset + c].copy_(d(t))
                    else:
                        out[:, offset:offset + c].copy_(u)
                    offset += c
                return [out]
            return [torch.cat([u if u is not None else d(t) for t, u, d in zip(x, ups, self.deblocks)], dim=1)]
        ups = [deblock(x[i]) for i, deblock in enumerate(self.deblocks)]
        return [torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]]


register_everywhere("fuser", ConvFuser)
register_everywhere("backbone", SECOND)
register_everywhere("neck", SECONDFPN)
