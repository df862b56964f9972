"""The learned nets of the camera -> BEV view transforms on the device: `DepthLSSTransform.dtransform` (the depth stem), the two
3x3 layers of its `depthnet`, and the 1x1 convolution + softmax + split that ends the `depthnet` of both transforms
(reference: mmdet3d/models/vtransforms/depth_lss.py:43-97, lss.py:63-75).  `heads` re-exports everything here.

The reference runs these layers in fp32 (`@force_fp32`), and so does this package by default.  With
`BaseTransform.cam_nets_dtype = torch.float16 | torch.bfloat16` the user opts into 16-bit operands with fp32 accumulation:

  * `depth_stem_forward`: `bevamd_cam_depth_stem_forward` (csrc/ext/cam_nets.hip), two launches.  Layer 1 is a per-pixel function
    of the scalar depth and is never stored; layers 2 and 3 are implicit GEMMs on the 16-bit MFMA.  The result is the NHWC
    [n, fH, fW, 64] second source `bev_conv_forward` reads without a transpose.
  * the two 3x3 layers: `bev_trunk.bev_conv_forward` through `fold_conv_bias_bn` (the convolution's bias goes into the shift; the
    first layer reads the stem's output and the image features as its two sources, no `cat`).
  * `depth_head_forward`: `bevamd_cam_depth_head_forward`, one launch: the logits stay in registers, depth [n, D, H, W] and context
    [n, H, W, C] come out in fp32 in the layouts `BevPoolPlan.fused` takes.

BatchNorm is never folded into the 16-bit weights: scale and shift are fp32 arrays applied to the fp32 accumulator.  Folds are
cached on the parameters' addresses and versions, as `bev_trunk.fold_bev_layer` does.  No host sync and no cached workspace: after
one warm-up forward (which builds the folds) the route can be captured in a `torch.cuda.graph`.
"""
from dataclasses import dataclass

import torch
from torch import nn

from . import _capi
from .bev_trunk import _DTYPES, FoldedBevLayer, _tensor_key, bev_pack_weight

__all__ = ["DepthStemFold", "DepthHeadFold", "fold_conv_bias_bn", "fold_depth_stem", "fold_depth_head", "depth_stem_forward",
           "depth_head_forward", "depth_stem_structure", "bias_layer_spec", "stem_output_size", "head_served", "pack_stem_layer2",
           "pack_head_weight"]

_UNSUPPORTED = 4          # BEVAMD_ERR_UNSUPPORTED
HEAD_MAX_IN, HEAD_MAX_D, HEAD_MAX_C = 512, 128, 128
_STEM = [(1, 8, 1, 1, 0), (8, 32, 5, 4, 2), (32, 64, 5, 2, 2)]        # (in, out, kernel, stride, padding) of dtransform's layers


def _bn_ok(bn):
    return isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.running_mean is not None and bn.running_var is not None


def _plain_conv(conv):
    return type(conv) is nn.Conv2d and conv.groups == 1 and conv.dilation == (1, 1) and conv.padding_mode == "zeros" \
        and not isinstance(conv.padding, str)


def bias_layer_spec(conv, bn=None):
    """(mode, kernel, stride) of a (Conv2d with or without bias, eval-mode BatchNorm2d) pair that `bev_conv_forward` serves through
    `fold_conv_bias_bn`, else None: 3x3 padding 1 stride 1 or 2, or 1x1 stride 1; out_channels a multiple of 32, in_channels a
    multiple of 16."""
    if bn is not None and (not _bn_ok(bn) or bn.num_features != conv.out_channels):
        return None
    if not _plain_conv(conv) or conv.out_channels % 32 or conv.out_channels < 32 or conv.in_channels % 16 or conv.in_channels < 16:
        return None
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if k == (3, 3) and p == (1, 1) and s in ((1, 1), (2, 2)):
        return ("conv", 3, s[0])
    if k == (1, 1) and p == (0, 0) and s == (1, 1):
        return ("conv", 1, 1)
    return None


def depth_stem_structure(dtransform):
    """True when `dtransform` is exactly the stem the kernel is built for: Conv2d(1, 8, 1), Conv2d(8, 32, 5, stride 4, padding 2),
    Conv2d(32, 64, 5, stride 2, padding 2), each followed by an eval-mode BatchNorm2d with running statistics and a ReLU."""
    if not isinstance(dtransform, nn.Sequential) or len(dtransform) != 9:
        return False
    for i, (cin, cout, k, s, p) in enumerate(_STEM):
        conv, bn, relu = dtransform[3 * i], dtransform[3 * i + 1], dtransform[3 * i + 2]
        if not _plain_conv(conv) or not _bn_ok(bn) or not isinstance(relu, nn.ReLU):
            return False
        if (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) != (cin, cout, (k, k), (s, s), (p, p)):
            return False
        if bn.num_features != cout:
            return False
    return True


def stem_output_size(H, W):
    """The stem's output map of an H x W raster."""
    oh2, ow2 = (H - 1) // 4 + 1, (W - 1) // 4 + 1
    return (oh2 - 1) // 2 + 1, (ow2 - 1) // 2 + 1


# ---- folds -------------------------------------------------------------------------------------------------------------------------
def _scale_shift64(conv, bn):
    """scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale, in float64."""
    f64 = lambda t: t.detach().to(torch.float64)      # noqa: E731
    std = torch.sqrt(f64(bn.running_var) + bn.eps)
    scale = f64(bn.weight) / std if bn.weight is not None else 1.0 / std
    beta = f64(bn.bias) if bn.bias is not None else torch.zeros_like(scale)
    bias = f64(conv.bias) if conv.bias is not None else torch.zeros_like(scale)
    return scale, beta + (bias - f64(bn.running_mean)) * scale


def _scale_shift(conv, bn):
    """The same, each rounded once to fp32."""
    scale, shift = _scale_shift64(conv, bn)
    return scale.to(torch.float32).contiguous(), shift.to(torch.float32).contiguous()


def _cached(owner, slot, dtype, tensors, extra, make):
    """`make()` cached on `owner` per dtype, keyed on the tensors' addresses and versions (see `bev_trunk.fold_bev_layer`: every
    in-place torch operation moves the version; after a write through `.data` drop the cache by hand)."""
    key = _tensor_key(tensors) + tuple(extra)
    store = owner.__dict__.setdefault(slot, {})
    hit = store.get(dtype)
    if hit is not None and hit[0] == key:
        return hit[1]
    val = make()
    store[dtype] = (key, val)
    return val


def _check_dtype(dtype):
    if dtype not in _DTYPES:
        raise RuntimeError(f"the camera nets run on float16 or bfloat16 operands, got {dtype}")


def fold_conv_bias_bn(conv, bn, dtype=torch.float16):
    """`FoldedBevLayer` of an eval-mode (Conv2d WITH a bias, BatchNorm2d) pair for `bev_conv_forward`: the weights rounded once from
    the parameters to `dtype` and packed with `bev_pack_weight`; scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) *
    scale, in float64 and rounded once to fp32.  Cached on `conv` per dtype."""
    _check_dtype(dtype)
    spec = bias_layer_spec(conv, bn)
    if spec is None:
        raise RuntimeError(f"the BEV convolution kernel does not serve {conv} with {bn}")

    def make():
        scale, shift = _scale_shift(conv, bn)
        return FoldedBevLayer(bev_pack_weight(conv.weight.detach().to(dtype), "conv"), scale, shift, conv.in_channels,
                              conv.out_channels, spec[1], spec[2], "conv")
    return _cached(conv, "_bevamd_cam_folded", dtype, [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var],
                   (bn.eps,), make)


@dataclass
class DepthStemFold:
    """`dtransform` in the stem kernel's layout.  scale1, shift1 [8]; packed2 [32 * 224] (a 1x1 layer over k = 8 tap + ci, zero for
    k >= 200), scale2, shift2 [32]; packed3 [64 * 800], scale3, shift3 [64]; scales and shifts fp32, weights `dtype`."""
    scale1: torch.Tensor
    shift1: torch.Tensor
    packed2: torch.Tensor
    scale2: torch.Tensor
    shift2: torch.Tensor
    packed3: torch.Tensor
    scale3: torch.Tensor
    shift3: torch.Tensor
    dtype: torch.dtype


def pack_stem_layer2(w):
    """Conv2d(8, 32, 5) weight [32, 8, 5, 5] -> the packed order of a 1x1 layer over the 200 inputs k = 8 (5 ky + kx) + ci."""
    return bev_pack_weight(w.permute(0, 2, 3, 1).reshape(32, 200, 1, 1), "conv")


def fold_depth_stem(dtransform, dtype=torch.float16):
    """`DepthStemFold` of an eval-mode `dtransform` on the parameters' device, cached on the module per dtype.  Layer 1 has no
    16-bit weight: its 1x1 weight is multiplied into its scale in float64 (scale1 = w1 * gamma / sqrt(var + eps)), so that a1 =
    max(fma(d, scale1, shift1), 0) is computed from the fp32 depth with one rounding."""
    _check_dtype(dtype)
    if not depth_stem_structure(dtransform):
        raise RuntimeError("the depth stem kernel serves exactly Conv2d(1, 8, 1), Conv2d(8, 32, 5, 4, 2), Conv2d(32, 64, 5, 2, 2) with "
                           "eval-mode BatchNorm2d and ReLU")
    convs, bns = [dtransform[0], dtransform[3], dtransform[6]], [dtransform[1], dtransform[4], dtransform[7]]

    def make():
        s1, t1 = _scale_shift64(convs[0], bns[0])
        s1 = (s1 * convs[0].weight.detach().to(torch.float64).reshape(8)).to(torch.float32).contiguous()
        t1 = t1.to(torch.float32).contiguous()
        s2, t2 = _scale_shift(convs[1], bns[1])
        s3, t3 = _scale_shift(convs[2], bns[2])
        return DepthStemFold(s1, t1, pack_stem_layer2(convs[1].weight.detach().to(dtype)), s2, t2,
                             bev_pack_weight(convs[2].weight.detach().to(dtype), "conv"), s3, t3, dtype)
    tensors = [t for c, b in zip(convs, bns) for t in (c.weight, c.bias, b.weight, b.bias, b.running_mean, b.running_var)]
    return _cached(dtransform, "_bevamd_cam_folded", dtype, tensors, tuple(b.eps for b in bns), make)


@dataclass
class DepthHeadFold:
    """The 1x1 convolution that ends a depthnet: packed [(D + C rounded up to 16) * Cin] weights of `dtype` (zero rows past D + C),
    bias [D + C] fp32 (zeros for a convolution without one)."""
    packed: torch.Tensor
    bias: torch.Tensor
    in_channels: int
    D: int
    C: int
    dtype: torch.dtype


def head_served(in_channels, D, C):
    """The sizes `bevamd_cam_depth_head_forward` serves."""
    return in_channels >= 32 and in_channels % 32 == 0 and in_channels <= HEAD_MAX_IN and 1 <= D <= HEAD_MAX_D \
        and 4 <= C <= HEAD_MAX_C and C % 4 == 0


def pack_head_weight(w):
    """[D + C, Cin, 1, 1] -> packed with the rows padded with zeros to a multiple of 16."""
    rows = w.shape[0]
    pad = -rows % 16
    if pad:
        w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], dim=0)
    return bev_pack_weight(w, "conv")


def fold_depth_head(conv, D, C, dtype=torch.float16):
    """`DepthHeadFold` of Conv2d(Cin, D + C, 1) on the parameters' device, cached on `conv` per dtype."""
    _check_dtype(dtype)
    if not _plain_conv(conv) or (conv.kernel_size, conv.stride, conv.padding) != ((1, 1), (1, 1), (0, 0)) or conv.out_channels != D + C:
        raise RuntimeError(f"the depth head takes Conv2d(Cin, {D} + {C}, 1), got {conv}")

    def make():
        w = conv.weight.detach()
        bias = conv.bias.detach().to(torch.float32).contiguous() if conv.bias is not None else w.new_zeros(D + C, dtype=torch.float32)
        return DepthHeadFold(pack_head_weight(w.to(dtype)), bias, conv.in_channels, int(D), int(C), dtype)
    return _cached(conv, "_bevamd_cam_head_folded", dtype, [conv.weight, conv.bias], (int(D), int(C)), make)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def _on_device(dev, what, *tensors):
    for t in tensors:
        if not torch.is_tensor(t) or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"{what}: the fold must be contiguous on the device of the input")


def depth_stem_forward(depth, fold, *, scratch=None, out=None):
    """The depth stem.  depth: fp32 [n, H, W] or [n, 1, H, W] on the device, contiguous (what `depth_raster` returns, read in
    place); fold: a `DepthStemFold` on the same device.  scratch: [n, OH2, OW2, 32] and out: [n, OH3, OW3, 64] buffers of the fold's
    dtype (None: fresh ones).  Returns the logical [n, 64, OH3, OW3] view of `out` with channels-last strides, which
    `bev_conv_forward` reads in place.  No sync, no host copy."""
    if not torch.is_tensor(depth) or not depth.is_cuda:
        raise RuntimeError("depth_stem_forward needs GPU tensors (host tensors: the module's torch layers)")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3 or depth.dtype != torch.float32 or not depth.is_contiguous() or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise RuntimeError(f"depth must be a contiguous float32 [n, H, W] or [n, 1, H, W], got {tuple(depth.shape)} {depth.dtype}")
    dev, dtype = depth.device, fold.dtype
    _on_device(dev, "depth_stem_forward", fold.scale1, fold.shift1, fold.packed2, fold.scale2, fold.shift2, fold.packed3, fold.scale3,
               fold.shift3)
    if fold.packed2.dtype != dtype or fold.packed3.dtype != dtype or dtype not in _DTYPES:
        raise RuntimeError(f"the fold holds {fold.packed2.dtype} / {fold.packed3.dtype} weights, its dtype says {dtype}")
    if any(t.dtype != torch.float32 for t in (fold.scale1, fold.shift1, fold.scale2, fold.shift2, fold.scale3, fold.shift3)) or \
            [t.numel() for t in (fold.scale1, fold.shift1, fold.scale2, fold.shift2, fold.scale3, fold.shift3)] != [8, 8, 32, 32, 64, 64]:
        raise RuntimeError("scales and shifts must be float32 arrays of 8, 32 and 64 elements")
    n, H, W = depth.shape
    oh2, ow2 = (H - 1) // 4 + 1, (W - 1) // 4 + 1
    oh3, ow3 = (oh2 - 1) // 2 + 1, (ow2 - 1) // 2 + 1
    if scratch is None:
        scratch = torch.empty((n, oh2, ow2, 32), dtype=dtype, device=dev)
    if out is None:
        out = torch.empty((n, oh3, ow3, 64), dtype=dtype, device=dev)
    for t, shape, name in ((scratch, (n, oh2, ow2, 32), "scratch"), (out, (n, oh3, ow3, 64), "out")):
        if t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous {dtype} {list(shape)} on the device of the input, got {tuple(t.shape)} {t.dtype}")
    depth = depth.detach()
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_cam_depth_stem_forward(
            _capi.ptr(depth), depth.numel(), n, H, W, _DTYPES[dtype], _capi.ptr(fold.scale1), _capi.ptr(fold.shift1),
            _capi.ptr(fold.packed2), fold.packed2.numel(), _capi.ptr(fold.scale2), _capi.ptr(fold.shift2), _capi.ptr(fold.packed3),
            fold.packed3.numel(), _capi.ptr(fold.scale3), _capi.ptr(fold.shift3), _capi.ptr(scratch), scratch.numel(), _capi.ptr(out),
            out.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "cam_depth_stem_forward")
    return out.permute(0, 3, 1, 2)


def depth_head_forward(x, fold, *, depth=None, ctx=None):
    """The end of a depthnet.  x: a logical [n, Cin, H, W] tensor of the fold's dtype on the device with channels-last strides (what
    `bev_conv_forward(..., out_layout="nhwc")` returns; anything else is made so, one copy); fold: a `DepthHeadFold`.  depth:
    [n, D, H, W] and ctx: [n, H, W, C] contiguous fp32 buffers (None: fresh ones).  Returns (depth, ctx) = (softmax over the first D
    output channels, the other C channels, NHWC), or None where the kernel does not serve the sizes.  No sync, no host copy."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("depth_head_forward needs GPU tensors (host tensors: the module's torch layers)")
    dev, dtype = x.device, fold.dtype
    if x.dim() != 4 or x.dtype != dtype or dtype not in _DTYPES or x.shape[1] != fold.in_channels or x.shape[2] < 1 or x.shape[3] < 1:
        raise RuntimeError(f"x must be a {dtype} [n, {fold.in_channels}, H, W], got {tuple(x.shape)} {x.dtype}")
    _on_device(dev, "depth_head_forward", fold.packed, fold.bias)
    if fold.packed.dtype != dtype or fold.bias.dtype != torch.float32 or fold.bias.numel() != fold.D + fold.C:
        raise RuntimeError(f"the fold holds {fold.packed.dtype} weights and {fold.bias.numel()} {fold.bias.dtype} biases, it says "
                           f"{dtype} and {fold.D} + {fold.C}")
    x = x.detach()
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    n, cin, H, W = x.shape
    if depth is None:
        depth = torch.empty((n, fold.D, H, W), dtype=torch.float32, device=dev)
    if ctx is None:
        ctx = torch.empty((n, H, W, fold.C), dtype=torch.float32, device=dev)
    for t, shape, name in ((depth, (n, fold.D, H, W), "depth"), (ctx, (n, H, W, fold.C), "ctx")):
        if t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous float32 {list(shape)} on the device of the input, got {tuple(t.shape)} {t.dtype}")
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_cam_depth_head_forward(
            _capi.ptr(x), x.numel(), n, H, W, cin, fold.D, fold.C, _DTYPES[dtype], _capi.ptr(fold.packed), fold.packed.numel(),
            _capi.ptr(fold.bias), _capi.ptr(depth), depth.numel(), _capi.ptr(ctx), ctx.numel(), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "cam_depth_head_forward")
    return depth, ctx
