"""`SwinTransformer`, the `encoders.camera.backbone` of the reference's default camera+LiDAR detector, its camera-only detector and
both BEV-segmentation camera configs, registered in `registry.BACKBONES` under the reference's name.  The configs mean mmdet 2.x's
mmdet/models/backbones/swin.py over mmcv's `FFN` and mmdet's `PatchEmbed` / `PatchMerging`, which the reference imports and does not
vendor; the modules here are written after them.  `heads` re-exports everything here.

Module tree and state-dict keys are mmdet's (`patch_embed.projection.*`, `patch_embed.norm.*`, `stages.i.blocks.j.norm1.*`,
`stages.i.blocks.j.attn.w_msa.{relative_position_bias_table, relative_position_index, qkv.*, proj.*}`, `stages.i.blocks.j.norm2.*`,
`stages.i.blocks.j.ffn.layers.0.0.*`, `stages.i.blocks.j.ffn.layers.1.*`, `stages.i.downsample.{norm.*, reduction.weight}`,
`norm{i}.*`), so `load_state_dict(strict=True)` takes a BEVFusion checkpoint's `encoders.camera.backbone.*`; `swin_convert` is
mmdet's `swin_converter` for an official Swin checkpoint.  A `Pretrained` `init_cfg` (or `pretrained=`) is RECORDED on the module
and never fetched: nothing here opens a URL or a file.

Dispatch, as `cam_resnet.ResNet` does it:

  * GPU fp16 or bf16 tensors of the parameters' dtype, eval mode, no gradient needed, `use_fused`: per block the attention is
    `norm1` (torch) -> the `qkv` Linear (torch) on the [B, H, W, C] token map -> ONE launch of `bevamd_window_attention_forward`
    (csrc/ext/window_attention.hip: pad, roll, window partition, q k^T, relative position bias, shift mask, softmax, attn v,
    window reverse, roll back and crop by index arithmetic, one wave per (window, head) on the 16-bit MFMA with an fp32 softmax) ->
    the `proj` Linear (torch) -> residual.  The Linear layers, the LayerNorms and the FFN stay with torch.  A block whose window or
    head size the kernel does not serve (anything but 7 and 32), or whose stage is not in `fused_stages`, runs its torch layers
    inside the chain.
  * on that path, a block of a stage listed in `fused_ffn_stages` (default: none) ends in ONE launch of `bevamd_swin_ffn_forward`
    (csrc/ext/swin_ffn.hip: `norm2`, fc1, GELU, fc2 and the residual, the hidden activations in registers) where `swin_ffn_spec`
    holds; any other block ends in its torch layers.
  * otherwise (train mode, host tensors, fp32 tensors, a gradient, `use_fused = False`): the torch layers in mmdet's order, with
    autograd, dropout and drop-path.

Fused outputs are logical [B, C, H, W] tensors with channels-last strides (the token map permuted, no copy), which
`GeneralizedLSSFPN` reads in place.  No host sync; the dense relative position bias of a block is expanded once and cached on its
`WindowMSA` (`fold_window_bias`), so the eval forward can be captured in a `torch.cuda.graph` after one warm-up forward.

`use_fused` and `fused_stages` follow the measurement in DESIGN 3.29, `fused_ffn_stages` the one in DESIGN 3.30.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from . import _capi
from .bev_trunk import _DTYPES, _fusable_tensor, _no_grad_needed, _tensor_key
from .registry import BACKBONES, build_norm_layer, register_everywhere  # noqa: F401

__all__ = ["SwinTransformer", "SwinBlockSequence", "SwinBlock", "ShiftWindowMSA", "WindowMSA", "PatchEmbed", "PatchMerging", "SwinFFN",
           "DropPath", "window_attention", "fold_window_bias", "window_attention_spec", "swin_convert", "swin_ffn", "fold_swin_ffn",
           "swin_ffn_spec", "swin_pack_ffn"]

_UNSUPPORTED = 4          # BEVAMD_ERR_UNSUPPORTED
KERNEL_WINDOW = 7
KERNEL_HEAD_DIM = 32
KERNEL_FFN_CMAX = 192     # SF_CMAX of csrc/ext/swin_ffn.hip: the widest token of the fused FFN; its hidden width goes to 4 times that
_DEFAULT_NORM = dict(type="LN")
_DEFAULT_ACT = dict(type="GELU")


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def window_attention(qkv, bias, scale, shift, pad_qkv=None, *, window=KERNEL_WINDOW, out=None):
    """Shifted-window attention in one launch.  qkv [B, H, W, 3C]: the qkv Linear of the un-padded, un-rolled token map, fp16 / bf16
    on the device, contiguous, channel `which * C + head * head_dim + d`; bias [heads, window^2, window^2] fp32 (`fold_window_bias`);
    pad_qkv [3C] of qkv's dtype: the q, k, v of a padded token (the Linear's bias), None for zeros; 0 <= shift < window.  out: a
    contiguous [B, H, W, C] of qkv's dtype to write, None for a fresh one.  Returns out, or None where the kernel does not serve the
    sizes (window 7 and head dimension 32 are built).  No sync, no host copy."""
    if not torch.is_tensor(qkv) or not torch.is_tensor(bias) or not qkv.is_cuda or not bias.is_cuda:
        raise RuntimeError("window_attention needs GPU tensors (host tensors: the module's torch layers)")
    if qkv.dim() != 4 or qkv.dtype not in _DTYPES or not qkv.is_contiguous() or qkv.shape[3] % 3:
        raise RuntimeError(f"qkv must be a contiguous float16 or bfloat16 [B, H, W, 3C], got {tuple(qkv.shape)} {qkv.dtype}")
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    n = window * window
    if bias.dim() != 3 or bias.dtype != torch.float32 or not bias.is_contiguous() or bias.device != qkv.device \
            or tuple(bias.shape[1:]) != (n, n):
        raise RuntimeError(f"bias must be a contiguous float32 [heads, {n}, {n}] on qkv's device, got {tuple(bias.shape)} {bias.dtype}")
    heads = bias.shape[0]
    if heads < 1 or C % heads or H < 1 or W < 1:
        raise RuntimeError(f"{C} channels do not split into {heads} heads, or the map {H} x {W} is empty")
    if pad_qkv is not None:
        if not torch.is_tensor(pad_qkv) or pad_qkv.device != qkv.device or pad_qkv.dtype != qkv.dtype or tuple(pad_qkv.shape) != (C3,) \
                or not pad_qkv.is_contiguous():
            raise RuntimeError(f"pad_qkv must be a contiguous [{C3}] of qkv's dtype and device")
        pad_qkv = pad_qkv.detach()
        if pad_qkv.data_ptr() % 16:
            pad_qkv = pad_qkv.clone()
    if not 0 <= int(shift) < window:
        raise RuntimeError(f"shift {shift} must lie in [0, {window})")
    if out is None:
        out = torch.empty((B, H, W, C), dtype=qkv.dtype, device=qkv.device)
    elif not torch.is_tensor(out) or out.device != qkv.device or out.dtype != qkv.dtype or tuple(out.shape) != (B, H, W, C) \
            or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous [{B}, {H}, {W}, {C}] of qkv's dtype and device")
    qkv = qkv.detach()
    with torch.cuda.device(qkv.device):
        rc = _capi.load().bevamd_window_attention_forward(
            _capi.ptr(qkv), qkv.numel(), _capi.ptr(pad_qkv), 0 if pad_qkv is None else pad_qkv.numel(), _capi.ptr(bias), bias.numel(),
            _DTYPES[qkv.dtype], B, H, W, C, heads, int(window), C // heads, float(scale), int(shift), _capi.ptr(out), out.numel(),
            _capi.stream_ptr(qkv.device))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "window_attention_forward")
    return out


def _fold_bias(w_msa):
    n = w_msa.window_size[0] * w_msa.window_size[1]
    index = w_msa.relative_position_index.reshape(-1).long()          # the module's buffer: a checkpoint's index rules
    table = w_msa.relative_position_bias_table.detach()
    return table[index].reshape(n, n, -1).permute(2, 0, 1).to(torch.float32).contiguous()


def fold_window_bias(w_msa):
    """The dense relative position bias `relative_position_bias_table[relative_position_index]` of a `WindowMSA` as [heads, N, N]
    fp32 on the parameters' device, cached on `w_msa` on the tensors' addresses and versions (see `fold_bev_layer` for what moves a
    version).  Run one forward before capturing a graph."""
    key = _tensor_key([w_msa.relative_position_bias_table, w_msa.relative_position_index])
    cache = w_msa.__dict__.get("_bevamd_folded")
    if cache is not None and cache[0] == key:
        return cache[1]
    val = _fold_bias(w_msa)
    w_msa.__dict__["_bevamd_folded"] = (key, val)
    return val


def window_attention_spec(attn):
    """True for a `ShiftWindowMSA` whose attention the kernel serves: a 7 x 7 window and heads of 32 channels."""
    w = getattr(attn, "w_msa", None)
    return isinstance(w, WindowMSA) and tuple(w.window_size) == (KERNEL_WINDOW, KERNEL_WINDOW) \
        and w.embed_dims == w.num_heads * KERNEL_HEAD_DIM and 0 <= attn.shift_size < KERNEL_WINDOW \
        and attn.window_size == KERNEL_WINDOW


# ---- mmcv / mmdet building blocks ------------------------------------------------------------------------------------------------
class DropPath(nn.Module):
    """mmcv's DropPath (stochastic depth per sample): identity in eval mode and at drop_prob 0."""

    def __init__(self, drop_prob=0.1):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        shape = (x.shape[0],) + (1,) * (x.dim() - 1)
        mask = keep + torch.rand(shape, dtype=x.dtype, device=x.device)
        return x.div(keep) * mask.floor()


def _build_dropout(cfg):
    if cfg is None:
        return nn.Identity()
    cfg = dict(cfg)
    typ = cfg.pop("type")
    if typ == "DropPath":
        return DropPath(**cfg)
    if typ == "Dropout":
        return nn.Dropout(cfg.pop("drop_prob", 0.5), **cfg)
    raise KeyError(f"Unrecognized dropout type {typ}")


def _build_activation(cfg):
    cfg = dict(cfg)
    typ = cfg.pop("type")
    if typ == "GELU":
        return nn.GELU(**cfg)              # the erf form
    if typ == "ReLU":
        return nn.ReLU(**cfg)
    raise KeyError(f"Unrecognized activation type {typ}")


def _corner_pad(x, kernel, stride):
    """mmdet's AdaptivePadding('corner') of a [B, C, H, W] map: zeros at the bottom / right so that the kernel covers every pixel."""
    H, W = x.shape[-2:]
    pad_h = max((math.ceil(H / stride) - 1) * stride + kernel - H, 0)
    pad_w = max((math.ceil(W / stride) - 1) * stride + kernel - W, 0)
    if pad_h > 0 or pad_w > 0:
        x = F.pad(x, [0, pad_w, 0, pad_h])
    return x


class FFN(nn.Module):
    """mmcv's FFN with num_fcs 2: Linear - activation - Dropout, Linear, Dropout; the identity is added inside."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.0,
                 dropout_layer=None, add_identity=True):
        super().__init__()
        assert num_fcs >= 2
        self.embed_dims, self.feedforward_channels, self.num_fcs = embed_dims, feedforward_channels, num_fcs
        layers, in_channels = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(in_channels, feedforward_channels), _build_activation(act_cfg), nn.Dropout(ffn_drop)))
            in_channels = feedforward_channels
        layers.append(nn.Linear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        self.dropout_layer = _build_dropout(dropout_layer)
        self.add_identity = add_identity

    def forward(self, x, identity=None):
        out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        if identity is None:
            identity = x
        return identity + self.dropout_layer(out)


SwinFFN = FFN          # the name `heads` re-exports it under (`heads.FFN` is the TransFusion head's)


class PatchEmbed(nn.Module):
    """mmdet's PatchEmbed: corner padding, Conv2d kernel = stride = patch, LayerNorm.  forward(x [B, C, H, W]) -> (tokens [B, L,
    embed_dims], (H', W'))."""

    def __init__(self, in_channels=3, embed_dims=768, kernel_size=16, stride=None, norm_cfg=None):
        super().__init__()
        stride = kernel_size if stride is None else stride
        self.embed_dims, self.kernel_size, self.stride = embed_dims, kernel_size, stride
        self.projection = nn.Conv2d(in_channels, embed_dims, kernel_size=kernel_size, stride=stride, padding=0)
        self.norm = build_norm_layer(norm_cfg, embed_dims)[1] if norm_cfg is not None else None

    def forward(self, x):
        x = self.projection(_corner_pad(x, self.kernel_size, self.stride))
        out_size = (x.shape[2], x.shape[3])
        x = x.flatten(2).transpose(1, 2)
        if self.norm is not None:
            x = self.norm(x)
        return x, out_size


class PatchMerging(nn.Module):
    """mmdet's PatchMerging: corner padding, nn.Unfold 2 x 2 (channel c * 4 + ky * 2 + kx), LayerNorm(4C), Linear 4C -> out without
    bias.  forward(x [B, L, C], (H, W)) -> (tokens [B, L', out_channels], (H', W'))."""

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=None, norm_cfg=dict(type="LN"), bias=False):
        super().__init__()
        stride = kernel_size if stride is None else stride
        self.in_channels, self.out_channels, self.kernel_size, self.stride = in_channels, out_channels, kernel_size, stride
        self.sampler = nn.Unfold(kernel_size=kernel_size, dilation=1, padding=0, stride=stride)
        sample_dim = kernel_size * kernel_size * in_channels
        self.norm = build_norm_layer(norm_cfg, sample_dim)[1] if norm_cfg is not None else None
        self.reduction = nn.Linear(sample_dim, out_channels, bias=bias)

    def forward(self, x, input_size):
        B, L, C = x.shape
        H, W = input_size
        assert L == H * W, "input feature has wrong size"
        x = _corner_pad(x.view(B, H, W, C).permute(0, 3, 1, 2), self.kernel_size, self.stride)
        H, W = x.shape[-2:]
        x = self.sampler(x)
        out_h = (H - (self.kernel_size - 1) - 1) // self.stride + 1
        out_w = (W - (self.kernel_size - 1) - 1) // self.stride + 1
        x = x.transpose(1, 2)
        if self.norm is not None:
            x = self.norm(x)
        return self.reduction(x), (out_h, out_w)


# ---- mmdet/models/backbones/swin.py ----------------------------------------------------------------------------------------------
def _relative_position_index(wh, ww):
    """index[i][j] = (y_i - y_j + wh - 1) * (2 ww - 1) + (x_i - x_j + ww - 1) of the tokens i, j = y * ww + x of a window."""
    ys, xs = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    return (ys[:, None] - ys[None, :] + wh - 1) * (2 * ww - 1) + (xs[:, None] - xs[None, :] + ww - 1)


class WindowMSA(nn.Module):
    """Window multi-head self-attention with a relative position bias.  forward(x [windows * B, N, C], mask [windows, N, N] or
    None)."""

    def __init__(self, embed_dims, num_heads, window_size, qkv_bias=True, qk_scale=None, attn_drop_rate=0.0, proj_drop_rate=0.0):
        super().__init__()
        self.embed_dims, self.window_size, self.num_heads = embed_dims, tuple(window_size), num_heads
        head_embed_dims = embed_dims // num_heads
        self.scale = qk_scale or head_embed_dims ** -0.5
        wh, ww = self.window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        self.register_buffer("relative_position_index", _relative_position_index(wh, ww).contiguous())
        self.qkv = nn.Linear(embed_dims, embed_dims * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop_rate)
        self.proj = nn.Linear(embed_dims, embed_dims)
        self.proj_drop = nn.Dropout(proj_drop_rate)
        self.softmax = nn.Softmax(dim=-1)
        self.init_weights()

    def init_weights(self):
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x, mask=None):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        q = q * self.scale
        attn = q @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1)
        attn = attn + bias.permute(2, 0, 1).contiguous().unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = attn.view(B // nW, nW, self.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, self.num_heads, N, N)
        attn = self.attn_drop(self.softmax(attn))
        x = (attn @ v).transpose(1, 2).reshape(B, N, C)
        return self.proj_drop(self.proj(x))


class ShiftWindowMSA(nn.Module):
    """Shifted-window attention: pad to a multiple of the window, roll by -shift, partition, `WindowMSA` under the shift mask,
    reverse, roll back, crop, drop-path.  forward(query [B, H * W, C], (H, W))."""

    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None, attn_drop_rate=0,
                 proj_drop_rate=0, dropout_layer=dict(type="DropPath", drop_prob=0.0)):
        super().__init__()
        self.window_size, self.shift_size = window_size, shift_size
        assert 0 <= self.shift_size < self.window_size
        self.w_msa = WindowMSA(embed_dims, num_heads, (window_size, window_size), qkv_bias, qk_scale, attn_drop_rate, proj_drop_rate)
        self.drop = _build_dropout(dropout_layer)

    def window_partition(self, x):
        B, H, W, C = x.shape
        ws = self.window_size
        x = x.view(B, H // ws, ws, W // ws, ws, C)
        return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)

    def window_reverse(self, windows, H, W):
        ws = self.window_size
        B = int(windows.shape[0] / (H * W / ws / ws))
        x = windows.view(B, H // ws, W // ws, ws, ws, -1)
        return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)

    def forward(self, query, hw_shape):
        B, L, C = query.shape
        H, W = hw_shape
        assert L == H * W, "input feature has wrong size"
        ws, shift = self.window_size, self.shift_size
        query = query.view(B, H, W, C)
        pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
        query = F.pad(query, (0, 0, 0, pad_r, 0, pad_b))
        H_pad, W_pad = query.shape[1], query.shape[2]
        if shift > 0:
            shifted = torch.roll(query, shifts=(-shift, -shift), dims=(1, 2))
            img_mask = torch.zeros((1, H_pad, W_pad, 1), device=query.device)
            slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
            cnt = 0
            for h in slices:
                for w in slices:
                    img_mask[:, h, w, :] = cnt
                    cnt += 1
            mask_windows = self.window_partition(img_mask).view(-1, ws * ws)
            attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
            attn_mask = attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))
            attn_mask = attn_mask.to(query.dtype)
        else:
            shifted, attn_mask = query, None
        windows = self.window_partition(shifted).view(-1, ws * ws, C)
        windows = self.w_msa(windows, mask=attn_mask).view(-1, ws, ws, C)
        x = self.window_reverse(windows, H_pad, W_pad)
        if shift > 0:
            x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
        if pad_r > 0 or pad_b > 0:
            x = x[:, :H, :W, :].contiguous()
        return self.drop(x.view(B, H * W, C))

    def forward_fused(self, query, hw_shape):
        """The eval-mode attention of `forward` on a normalised token map through the kernel, or None where it does not serve the
        sizes: qkv Linear on the un-padded, un-rolled map, one launch, proj Linear.  (Dropout and drop-path are the identity in eval
        mode.)"""
        B, L, C = query.shape
        H, W = hw_shape
        w = self.w_msa
        qkv = w.qkv(query).view(B, H, W, 3 * C)
        out = window_attention(qkv, fold_window_bias(w), w.scale, self.shift_size, w.qkv.bias, window=self.window_size)
        if out is None:
            return None
        return w.proj(out.view(B, L, C))


class SwinBlock(nn.Module):
    """norm1 - ShiftWindowMSA - residual, norm2 - FFN (the residual inside).  forward(x [B, L, C], (H, W)); `fused`: the attention
    through its kernel, `fused_ffn`: norm2 - FFN through `swin_ffn`, each where the block is served (eval mode on the device: the
    caller decides)."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, window_size=7, shift=False, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, act_cfg=None, norm_cfg=None, with_cp=False):
        super().__init__()
        if with_cp:
            raise NotImplementedError("SwinBlock: with_cp is not supported")
        act_cfg = dict(_DEFAULT_ACT) if act_cfg is None else act_cfg
        norm_cfg = dict(_DEFAULT_NORM) if norm_cfg is None else norm_cfg
        self.norm1 = build_norm_layer(norm_cfg, embed_dims)[1]
        self.attn = ShiftWindowMSA(embed_dims, num_heads, window_size, window_size // 2 if shift else 0, qkv_bias, qk_scale,
                                   attn_drop_rate, drop_rate, dict(type="DropPath", drop_prob=drop_path_rate))
        self.norm2 = build_norm_layer(norm_cfg, embed_dims)[1]
        self.ffn = FFN(embed_dims, feedforward_channels, 2, act_cfg, drop_rate, dict(type="DropPath", drop_prob=drop_path_rate), True)

    def forward(self, x, hw_shape, fused=False, fused_ffn=False):
        identity = x
        h = self.norm1(x)
        a = self.attn.forward_fused(h, hw_shape) if fused and window_attention_spec(self.attn) else None
        if a is None:
            a = self.attn(h, hw_shape)
        x = a + identity
        if fused_ffn and swin_ffn_spec(self):
            y = _swin_ffn_served(x, self.norm2, self.ffn)
            if y is not None:
                return y
        return self.ffn(self.norm2(x), identity=x)


class SwinBlockSequence(nn.Module):
    """One stage: `depth` blocks, every second one shifted, and the optional PatchMerging.  forward(x, hw) -> (x after the
    downsample, its (H, W), x before it, its (H, W))."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, depth, window_size=7, qkv_bias=True, qk_scale=None, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.0, downsample=None, act_cfg=None, norm_cfg=None, with_cp=False):
        super().__init__()
        rates = list(drop_path_rate) if isinstance(drop_path_rate, (list, tuple)) else [drop_path_rate] * depth
        assert len(rates) == depth
        self.blocks = nn.ModuleList(
            SwinBlock(embed_dims, num_heads, feedforward_channels, window_size, i % 2 == 1, qkv_bias, qk_scale, drop_rate, attn_drop_rate,
                      rates[i], act_cfg, norm_cfg, with_cp) for i in range(depth))
        self.downsample = downsample

    def forward(self, x, hw_shape, fused=False, fused_ffn=False):
        for block in self.blocks:
            x = block(x, hw_shape, fused, fused_ffn)
        if self.downsample is not None:
            x_down, down_hw = self.downsample(x, hw_shape)
            return x_down, down_hw, x, hw_shape
        return x, hw_shape, x, hw_shape


class SwinTransformer(nn.Module):
    """mmdet 2.x's Swin Transformer backbone.  forward(x [B, in_channels, H, W]) -> tuple of the `out_indices` stage outputs [B,
    embed_dims * 2^i, H / (4 * 2^i), W / (4 * 2^i)] (the stage's tokens before its PatchMerging through `norm{i}`); fused path: every
    output has channels-last strides.

    `use_abs_pos_embed` and `with_cp` raise NotImplementedError.  A `Pretrained` init_cfg (or `pretrained`) and `convert_weights`
    are recorded and NOT acted on: `init_weights()` then leaves the weights alone, and the checkpoint is loaded with
    `load_state_dict` (through `swin_convert` for an official one).  Nothing here opens a URL."""

    # defaults from the measurement in DESIGN 3.29
    use_fused = True                 # eval mode on GPU fp16 / bf16 tensors: the attention of every served block through the kernel
    fused_stages = (0, 1, 2, 3)      # the stages whose blocks do
    # opt-in, measurement in DESIGN 3.30: the stages whose served blocks end in one launch of the fused FFN (consulted only where
    # `fusable` holds)
    fused_ffn_stages = ()

    def __init__(self, pretrain_img_size=224, in_channels=3, embed_dims=96, patch_size=4, window_size=7, mlp_ratio=4,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), strides=(4, 2, 2, 2), out_indices=(0, 1, 2, 3), qkv_bias=True,
                 qk_scale=None, patch_norm=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_abs_pos_embed=False,
                 act_cfg=dict(type="GELU"), norm_cfg=dict(type="LN"), with_cp=False, pretrained=None, convert_weights=False,
                 frozen_stages=-1, init_cfg=None):
        super().__init__()
        if use_abs_pos_embed:
            raise NotImplementedError("SwinTransformer: use_abs_pos_embed is not supported")
        if with_cp:
            raise NotImplementedError("SwinTransformer: with_cp is not supported")
        if init_cfg and pretrained:
            raise AssertionError("init_cfg and pretrained cannot be specified at the same time")
        if isinstance(pretrained, str):
            init_cfg = dict(type="Pretrained", checkpoint=pretrained)
        elif pretrained is not None:
            raise TypeError("pretrained must be a str or None")
        if isinstance(pretrain_img_size, int):
            pretrain_img_size = (pretrain_img_size, pretrain_img_size)
        num_layers = len(depths)
        assert len(num_heads) == num_layers and len(strides) >= num_layers and max(out_indices) < num_layers
        assert strides[0] == patch_size, "Use non-overlapping patch embed."
        self.pretrain_img_size, self.embed_dims, self.depths, self.num_heads = tuple(pretrain_img_size), embed_dims, tuple(depths), tuple(num_heads)
        self.out_indices, self.convert_weights, self.frozen_stages, self.init_cfg = tuple(out_indices), convert_weights, frozen_stages, init_cfg
        self.use_abs_pos_embed = False

        self.patch_embed = PatchEmbed(in_channels, embed_dims, patch_size, strides[0], norm_cfg if patch_norm else None)
        self.drop_after_pos = nn.Dropout(p=drop_rate)
        total = sum(depths)
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, total)]
        self.stages = nn.ModuleList()
        channels = embed_dims
        for i in range(num_layers):
            down = PatchMerging(channels, 2 * channels, stride=strides[i + 1], norm_cfg=norm_cfg) if i < num_layers - 1 else None
            self.stages.append(SwinBlockSequence(channels, num_heads[i], mlp_ratio * channels, depths[i], window_size, qkv_bias, qk_scale,
                                                 drop_rate, attn_drop_rate, dpr[sum(depths[:i]):sum(depths[:i + 1])], down, act_cfg,
                                                 norm_cfg, with_cp))
            if down is not None:
                channels = down.out_channels
        self.num_features = [int(embed_dims * 2 ** i) for i in range(num_layers)]
        for i in self.out_indices:
            self.add_module(f"norm{i}", build_norm_layer(norm_cfg, self.num_features[i])[1])
        self._freeze_stages()

    # ---- mmdet's training behaviour ----
    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
            self.drop_after_pos.eval()
        for i in range(1, self.frozen_stages + 1):
            mods = [self.stages[i - 1]] + ([getattr(self, f"norm{i - 1}")] if (i - 1) in self.out_indices else [])
            for m in mods:
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self

    def init_weights(self):
        """mmdet's default: truncated normal (std 0.02) for the Linear weights and the bias tables, 0 for the Linear biases, 1 / 0 for
        the LayerNorms.  With a `Pretrained` init_cfg nothing is written and nothing is fetched."""
        if isinstance(self.init_cfg, dict) and self.init_cfg.get("type") == "Pretrained":
            return
        if self.init_cfg is not None:
            raise NotImplementedError(f"SwinTransformer: init_cfg {self.init_cfg} is not supported (None or Pretrained)")
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    nn.init.trunc_normal_(m.weight, std=0.02)
                    if m.bias is not None:
                        m.bias.zero_()
                elif isinstance(m, nn.LayerNorm):
                    m.weight.fill_(1.0)
                    m.bias.zero_()
                elif isinstance(m, WindowMSA):
                    m.init_weights()

    # ---- dispatch ----
    def fusable(self, x):
        """True when forward(x) sends the attention of at least one block through the kernel."""
        if not (self.use_fused and not self.training and _fusable_tensor(x, self.patch_embed.projection.weight)
                and _no_grad_needed(self, [x])):
            return False
        return any(i in self.fused_stages and any(window_attention_spec(b.attn) for b in s.blocks) for i, s in enumerate(self.stages))

    def forward(self, x):
        fused = self.fusable(x)
        x, hw_shape = self.patch_embed(x)
        x = self.drop_after_pos(x)
        outs = []
        for i, stage in enumerate(self.stages):
            x, hw_shape, out, out_hw = stage(x, hw_shape, fused and i in self.fused_stages, fused and i in self.fused_ffn_stages)
            if i in self.out_indices:
                out = getattr(self, f"norm{i}")(out)
                out = out.view(-1, *out_hw, self.num_features[i]).permute(0, 3, 1, 2)
                outs.append(out if fused else out.contiguous())
        return tuple(outs)


def swin_pack_ffn(w1, w2):
    """fc1.weight [hidden, C] and fc2.weight [C, hidden] in the MFMA fragment order of csrc/ext/swin_ffn.hip (both multiples of 32):
    packed1[tile][ks][lane][e] = w1[16 tile + (lane & 15)][32 ks + 8 (lane >> 4) + e], packed2[s][ct][lane][e] = w2[16 ct + (lane & 15)]
    [32 s + 16 (e >> 2) + 4 (lane >> 4) + (e & 3)].  Returns two flat contiguous tensors of the inputs' dtype and device."""
    hidden, C = w1.shape
    if tuple(w2.shape) != (C, hidden) or C % 32 or hidden % 32:
        raise ValueError(f"fc1 {tuple(w1.shape)} and fc2 {tuple(w2.shape)} must be [hidden, C] and [C, hidden], both multiples of 32")
    # w1: [tile, lane & 15, ks, lane >> 4, e] -> [tile, ks, lane >> 4, lane & 15, e]
    p1 = w1.detach().reshape(hidden // 16, 16, C // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    # w2: [ct, lane & 15, s, e >> 2, lane >> 4, e & 3] -> [s, ct, lane >> 4, lane & 15, e >> 2, e & 3]
    p2 = w2.detach().reshape(C // 16, 16, hidden // 32, 2, 4, 4).permute(2, 0, 4, 1, 3, 5).contiguous().view(-1)
    return p1, p2


def _ffn_linears(ffn):
    return ffn.layers[0][0], ffn.layers[1]


def fold_swin_ffn(norm, ffn):
    """(packed1, packed2, gamma, beta, b1, b2) of a block's `norm2` and `ffn` for `bevamd_swin_ffn_forward`: the two weights in
    fragment order (`swin_pack_ffn`) and the LayerNorm's and the Linears' vectors widened to fp32 (exact), cached on `ffn` on the
    tensors' addresses and versions (see `fold_bev_layer` for what moves a version); None for widths that are no multiples of 32,
    which have no fragment order.  Run one forward before capturing a graph."""
    fc1, fc2 = _ffn_linears(ffn)
    tensors = [norm.weight, norm.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    key = _tensor_key(tensors)
    cache = ffn.__dict__.get("_bevamd_folded")
    if cache is not None and cache[0] == key:
        return cache[1]
    val = None
    if fc1.weight.shape[0] % 32 == 0 and fc1.weight.shape[1] % 32 == 0:
        val = swin_pack_ffn(fc1.weight, fc2.weight) + tuple(t.detach().to(torch.float32).contiguous() for t in
                                                            (norm.weight, norm.bias, fc1.bias, fc2.bias))
    ffn.__dict__["_bevamd_folded"] = (key, val)
    return val


def _ffn_modules_served(norm, ffn):
    """The structure `bevamd_swin_ffn_forward` computes: an affine LayerNorm over the last dimension, Linear - exact GELU - Linear
    with biases, the identity added."""
    if not isinstance(norm, nn.LayerNorm) or not isinstance(ffn, FFN) or ffn.num_fcs != 2 or not ffn.add_identity:
        return False
    fc1, fc2 = _ffn_linears(ffn)
    act = ffn.layers[0][1]
    C = ffn.embed_dims
    return norm.weight is not None and norm.bias is not None and tuple(norm.normalized_shape) == (C,) \
        and type(act) is nn.GELU and getattr(act, "approximate", "none") == "none" \
        and fc1.bias is not None and fc2.bias is not None and fc1.in_features == C and fc2.out_features == C \
        and fc1.out_features == fc2.in_features


def swin_ffn_spec(block):
    """True for a `SwinBlock` whose tail the kernel serves: `norm2` an affine nn.LayerNorm over C, an FFN of two Linears around an
    exact nn.GELU with the identity added, C a multiple of 32 up to 192 and the hidden width a multiple of 32 up to 768."""
    norm, ffn = getattr(block, "norm2", None), getattr(block, "ffn", None)
    if not _ffn_modules_served(norm, ffn):
        return False
    C, hidden = ffn.embed_dims, ffn.layers[0][0].out_features
    return C % 32 == 0 and 32 <= C <= KERNEL_FFN_CMAX and hidden % 32 == 0 and 32 <= hidden <= 4 * KERNEL_FFN_CMAX


def swin_ffn(x, norm, ffn, *, out=None):
    """`ffn(norm(x), identity=x)` of a Swin block in eval mode in one launch.  x [.., C]: fp16 / bf16 on the device, contiguous, of
    the parameters' dtype; norm: the block's `norm2`, ffn: its `FFN`.  out: a contiguous tensor of x's shape and dtype to write
    (not x itself), None for a fresh one.  Returns out, or None where the kernel does not serve the modules or the sizes (see
    `swin_ffn_spec`).  No sync, no host copy; after one call nothing is allocated but out."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("swin_ffn needs GPU tensors (host tensors: the module's torch layers)")
    if not _ffn_modules_served(norm, ffn):
        return None
    return _swin_ffn_served(x, norm, ffn, out)


def _swin_ffn_served(x, norm, ffn, out=None):
    """`swin_ffn` for modules whose structure the caller has checked (`SwinBlock.forward`, through `swin_ffn_spec`)."""
    if x.dim() < 1 or x.dtype not in _DTYPES or not x.is_contiguous():
        raise RuntimeError(f"x must be a contiguous float16 or bfloat16 [.., C], got {tuple(x.shape)} {x.dtype}")
    fc1, _ = _ffn_linears(ffn)
    C, hidden = fc1.in_features, fc1.out_features
    if x.shape[-1] != C or fc1.weight.dtype != x.dtype or fc1.weight.device != x.device or norm.weight.dtype != x.dtype \
            or norm.weight.device != x.device:
        raise RuntimeError(f"x {tuple(x.shape)} {x.dtype} on {x.device} does not match the modules ({C} channels, "
                           f"{fc1.weight.dtype} on {fc1.weight.device})")
    fold = fold_swin_ffn(norm, ffn)
    if fold is None:
        return None
    if out is None:
        out = torch.empty_like(x)
    elif not torch.is_tensor(out) or out.device != x.device or out.dtype != x.dtype or out.shape != x.shape or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous {tuple(x.shape)} of x's dtype and device")
    p1, p2, gamma, beta, b1, b2 = fold
    x = x.detach()
    with torch.cuda.device(x.device):
        rc = _capi.load().bevamd_swin_ffn_forward(
            _capi.ptr(x), x.numel(), _capi.ptr(gamma), gamma.numel(), _capi.ptr(beta), beta.numel(), _capi.ptr(p1), p1.numel(),
            _capi.ptr(b1), b1.numel(), _capi.ptr(p2), p2.numel(), _capi.ptr(b2), b2.numel(), _DTYPES[x.dtype], x.numel() // C, C, hidden,
            float(norm.eps), _capi.ptr(out), out.numel(), _capi.stream_ptr(x.device))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "swin_ffn_forward")
    return out


# ---- mmdet's swin_converter ------------------------------------------------------------------------------------------------------
def swin_convert(state_dict):
    """An official Swin checkpoint's state dict (`convert_weights: true`) under this module's keys: `layers.` -> `stages.`, `attn.` ->
    `attn.w_msa.`, `mlp.fc1.` -> `ffn.layers.0.0.`, `mlp.fc2.` -> `ffn.layers.1.`, `patch_embed.proj` -> `patch_embed.projection`;
    `head.*` and the `attn_mask` buffers are dropped; `downsample.reduction.weight` and `downsample.norm.*` go from the official
    concatenation order (x0, x1, x2, x3 = pixels (0, 0), (1, 0), (0, 1), (1, 1)) to nn.Unfold's c * 4 + ky * 2 + kx.  A plain function on
    a dict; the values of the result are new tensors or the input's own."""
    def reduction_order(w):
        out_c, in_c = w.shape
        return w.reshape(out_c, 4, in_c // 4)[:, [0, 2, 1, 3], :].transpose(1, 2).reshape(out_c, in_c)

    def norm_order(v):
        in_c = v.shape[0]
        return v.reshape(4, in_c // 4)[[0, 2, 1, 3], :].transpose(0, 1).reshape(in_c)

    out = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith("head") or k.endswith("attn_mask"):
            continue
        new_k, new_v = k, v
        if k.startswith("layers"):
            if "attn." in k:
                new_k = k.replace("attn.", "attn.w_msa.")
            elif "mlp." in k:
                if "mlp.fc1." in k:
                    new_k = k.replace("mlp.fc1.", "ffn.layers.0.0.")
                elif "mlp.fc2." in k:
                    new_k = k.replace("mlp.fc2.", "ffn.layers.1.")
                else:
                    new_k = k.replace("mlp.", "ffn.")
            elif "downsample" in k:
                if "reduction." in k:
                    new_v = reduction_order(v)
                elif "norm." in k:
                    new_v = norm_order(v)
            new_k = new_k.replace("layers", "stages", 1)
        elif k.startswith("patch_embed") and "proj" in k:
            new_k = k.replace("proj", "projection")
        out[new_k] = new_v
    return out


register_everywhere("backbone", SwinTransformer)
