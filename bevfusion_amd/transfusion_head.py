"""TransFusionHead as a module (reference: mmdet3d/models/heads/bbox/transfusion.py, FFN of mmdet3d/models/utils/transformer.py:496-575),
registered in `registry.HEADS` under the reference's name so that `type: TransFusionHead` of
`configs/nuscenes/det/transfusion/default.yaml` builds.  `heads` re-exports everything here.

Module tree and state-dict keys are the reference's (`shared_conv.*`, `heatmap_head.0.conv.weight`, `heatmap_head.0.bn.*`,
`heatmap_head.1.*`, `class_encoding.*`, `decoder.i.*`, `prediction_heads.i.<head>.0.conv.weight`, `.0.bn.*`, `.1.weight`,
`.1.bias`), so `load_state_dict(strict=True)` takes its checkpoints' `heads.object.*`.

`forward_single`: `shared_conv` and `heatmap_head` are torch convolutions; `transfusion_select_proposals` picks the queries; the
category encoding and the prediction heads dispatch as `PillarFeatureNet` does:

  * GPU fp32 tensors, eval mode, no gradient needed, `use_fused`: `bevamd_head_class_encoding` (one launch, in place) and
    `bevamd_head_ffn_forward` (csrc/ext/head_ffn.hip: all heads of a layer in ONE launch, BatchNorm folded, `+ query_pos` on the
    center head, written straight into the [B, c, L * P] tensors the reference builds with `torch.cat`);
  * otherwise (train mode, a gradient, `use_fused = False`, a BatchNorm without running statistics, a head with num_conv != 2,
    a shape outside the kernel's limits): the module's own torch layers in the reference's order, with autograd, batch
    statistics and running-stat updates.  They are also the only path of `FFN` on host tensors.

There is no host sync anywhere in `forward`, and in eval mode it can be captured in a `torch.cuda.graph`; in eval mode the two
torch convolution stages run under the backend's deterministic flag (`_deterministic_convs`; `deterministic_convs = False` opts
out), so equal calls give equal bits.  The decoder returns a permuted view, so inside the module the fused heads are preceded by
one copy of `query_feat` to [B, C, P] order (the kernel takes a dense x).  The head itself has
no CPU path (the decoder's attention has none): host inputs raise.

`get_bboxes`, `get_targets` and `loss` are thin methods over `transfusion_get_bboxes`, `transfusion_get_targets` and
`transfusion_loss`.

Differences from the reference, on purpose: `bev_pos` is a non-persistent buffer (it moves with the module; the reference copies
it to the device in every forward); the proposal order is the stable one `transfusion_select_proposals` defines; `loss_iou` is
kept as its config only (the reference builds a VarifocalLoss and never calls it); `init_weights` also runs `FFN.init_weights`,
so a fresh head has the heatmap bias of -2.19 the FFN is built for (the reference defines it and never calls it);
`get_bboxes` returns the per-sample dicts of `transfusion_get_bboxes` for EVERY sample and wraps the boxes in
`metas[i]["box_type_3d"]` only where metas carry one (the reference returns sample 0 alone); ground truth reaches `get_targets`
in the forms `transfusion_get_targets` documents.
"""
import contextlib
import copy
import ctypes

import torch
from torch import nn
from torch.nn import functional as F

from . import _capi
from .decoder import PositionEmbeddingLearned, TransformerDecoderLayer
from .registry import BBOX_ASSIGNERS, BBOX_CODERS, HEADS, LOSSES, build_conv_layer, build_from_cfg, build_norm_layer, register_everywhere

__all__ = ["ConvModule", "FFN", "TransFusionHead", "head_class_encoding", "head_ffn_forward", "HEADS"]

_UNSUPPORTED = 4   # BEVAMD_ERR_UNSUPPORTED
# limits of bevamd_head_ffn_forward
FFN_MAX_IN, FFN_MAX_HEAD_CONV, FFN_MAX_CHANNELS, FFN_MAX_HEADS = 256, 128, 32, 8


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("TransFusionHead needs GPU tensors (the decoder attention has no CPU path)")


def _deterministic_convs():
    """Backend flags for the head's torch convolutions in eval mode: the vendor library's deterministic algorithms.  Its default
    choice for the 3 x 3 convolutions of a small BEV map sums in an order that changes from call to call (3.6e-7 on a 12 x 12 map,
    measured on an MI355X): equal calls would then differ in dense_heatmap and a replayed graph from the eager forward.  At
    180 x 180 the same algorithm is chosen either way."""
    cudnn = torch.backends.cudnn
    return cudnn.flags(enabled=cudnn.enabled, benchmark=False, deterministic=True, allow_tf32=cudnn.allow_tf32)


def _dense(t):
    """Contiguous fp32 and 16-byte aligned (the kernel loads the weights 16 bytes at a time)."""
    t = t.detach().float().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


# ---- the two kernels -------------------------------------------------------------------------------------------------------------
def head_class_encoding(query_feat, labels, weight, bias):
    """query_feat [B, C, K] fp32 (contiguous, on the device) += weight[:, labels] + bias, IN PLACE; labels [B, K] int64, weight
    [C, num_classes(, 1)], bias [C].  A label outside [0, num_classes) adds nothing.  One launch, no sync.  Returns query_feat."""
    if not query_feat.is_cuda:
        raise RuntimeError("head_class_encoding needs GPU tensors (host tensors: the module's Conv1d over a one-hot)")
    if query_feat.dim() != 3 or query_feat.dtype != torch.float32 or not query_feat.is_contiguous():
        raise RuntimeError(f"query_feat must be a contiguous float32 [B, C, K], got {tuple(query_feat.shape)} {query_feat.dtype}")
    B, C, K = query_feat.shape
    if weight.dim() == 3 and weight.shape[2] == 1:
        weight = weight[:, :, 0]
    if tuple(labels.shape) != (B, K) or labels.dtype != torch.int64 or weight.dim() != 2 or weight.shape[0] != C \
            or tuple(bias.shape) != (C,):
        raise RuntimeError(f"labels [{B}, {K}] int64, weight [{C}, classes] and bias [{C}] expected, got {tuple(labels.shape)} "
                           f"{labels.dtype}, {tuple(weight.shape)}, {tuple(bias.shape)}")
    dev = query_feat.device
    labels = labels.to(dev).contiguous()
    weight, bias = weight.detach().to(dev).float().contiguous(), bias.detach().to(dev).float().contiguous()
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_head_class_encoding(_capi.ptr(query_feat), _capi.ptr(labels), _capi.ptr(weight), _capi.ptr(bias), B, C, K,
                                                     weight.shape[1], _capi.stream_ptr(dev))
    _capi.check(rc, "head_class_encoding")
    return query_feat


def head_ffn_forward(x, params, query_pos=None, center_head=-1, outs=None, col_offset=0):
    """All prediction heads of one decoder layer in one launch.  x [B, Cin, P] fp32 on the device; params: per head the tuple
    (w1 [head_conv, Cin], scale [head_conv], shift [head_conv], w2 [c, head_conv], bias [c]) of contiguous fp32 device tensors;
    query_pos [B, P, 2] or None, added to head `center_head`; outs: per head a contiguous [B, c, out_stride] tensor whose columns
    [col_offset, col_offset + P) are written (None: fresh [B, c, P]).  Returns the list of outs, or None where the kernel does not
    serve the shape."""
    if not x.is_cuda:
        raise RuntimeError("head_ffn_forward needs GPU tensors (host tensors: the FFN module's torch layers)")
    if x.dim() != 3 or x.dtype != torch.float32:
        raise RuntimeError(f"x must be a float32 [B, Cin, P], got {tuple(x.shape)} {x.dtype}")
    x = x.detach().contiguous()
    B, Cin, P = x.shape
    dev = x.device
    n = len(params)
    head_conv = params[0][0].shape[0] if n else 0
    chans = [p[3].shape[0] for p in params]
    for w1, scale, shift, w2, bias in params:
        if tuple(w1.shape) != (head_conv, Cin) or tuple(scale.shape) != (head_conv,) or tuple(shift.shape) != (head_conv,) \
                or w2.shape[1] != head_conv or tuple(bias.shape) != (w2.shape[0],):
            raise RuntimeError(f"head parameters do not fit x [{B}, {Cin}, {P}] and head_conv {head_conv}")
        if any(t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() for t in (w1, scale, shift, w2, bias)):
            raise RuntimeError("head parameters must be contiguous float32 tensors on the device of x")
    if query_pos is not None:
        if tuple(query_pos.shape) != (B, P, 2) or query_pos.device != dev:
            raise RuntimeError(f"query_pos must be [{B}, {P}, 2] on the device of x, got {tuple(query_pos.shape)}")
        query_pos = query_pos.detach().float().contiguous()
    if outs is None:
        outs = [torch.empty((B, c, P), dtype=torch.float32, device=dev) for c in chans]
    if len(outs) != n:
        raise RuntimeError(f"{len(outs)} outputs for {n} heads")
    stride = outs[0].shape[2] if n else 0
    for o, c in zip(outs, chans):
        if o.dim() != 3 or tuple(o.shape[:2]) != (B, c) or o.shape[2] != stride or o.dtype != torch.float32 or o.device != dev \
                or not o.is_contiguous():
            raise RuntimeError(f"every output must be a contiguous float32 [{B}, c, {stride}] on the device of x, got {tuple(o.shape)}")
    arr = lambda k: (ctypes.c_void_p * max(n, 1))(*[p[k].data_ptr() for p in params])   # noqa: E731
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_head_ffn_forward(_capi.ptr(x), B, Cin, P, head_conv, n, _capi.ints(chans), arr(0), arr(1), arr(2), arr(3),
                                                  arr(4), _capi.ptr(query_pos), int(center_head), _capi.pointers(outs), stride,
                                                  int(col_offset), _capi.stream_ptr(dev))
    if rc == _UNSUPPORTED:
        return None
    _capi.check(rc, "head_ffn_forward")
    return outs


# ---- modules ---------------------------------------------------------------------------------------------------------------------
class ConvModule(nn.Module):
    """The part of mmcv.cnn.ConvModule the heads use: conv -> norm -> ReLU with the children `conv`, `bn` and `activate`.
    bias="auto": the convolution has a bias only without a norm."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias="auto", conv_cfg=None,
                 norm_cfg=None, act_cfg=dict(type="ReLU"), inplace=True):
        super().__init__()
        if act_cfg is not None and act_cfg.get("type") != "ReLU":
            raise NotImplementedError(f"activation {act_cfg.get('type')!r}: ConvModule serves ReLU or none")
        self.with_norm = norm_cfg is not None
        self.with_activation = act_cfg is not None
        if bias == "auto":
            bias = not self.with_norm
        self.with_bias = bias
        self.conv = build_conv_layer(conv_cfg, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                     groups=groups, bias=bias)
        if self.with_norm:
            self.norm_name, norm = build_norm_layer(norm_cfg, out_channels)
            self.add_module(self.norm_name, norm)
        if self.with_activation:
            self.activate = nn.ReLU(inplace=inplace)

    @property
    def norm(self):
        return getattr(self, self.norm_name) if self.with_norm else None

    def forward(self, x):
        x = self.conv(x)
        if self.with_norm:
            x = self.norm(x)
        if self.with_activation:
            x = self.activate(x)
        return x


class FFN(nn.Module):
    """transformer.py:496-575: one small stack per head, `heads` = {name: (classes, num_conv)}, children named after the heads.
    forward(x [B, Cin, P], query_pos [B, P, 2] or None, out, layer) -> {name: [B, classes, P]}; with query_pos the `center` head
    gets `+ query_pos.permute(0, 2, 1)` (the reference's head does that right after the call); with out = {name: [B, classes,
    L * P]} the results are written into columns [layer * P, (layer + 1) * P) of it and the returned tensors are views of them."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, init_bias=-2.19, conv_cfg=dict(type="Conv1d"),
                 norm_cfg=dict(type="BN1d"), bias="auto", **kwargs):
        super().__init__()
        self.heads = heads
        self.init_bias = init_bias
        self.in_channels, self.head_conv, self.final_kernel = in_channels, head_conv, final_kernel
        self.use_fused = True   # eval mode on GPU tensors: all heads in one launch (False: the torch layers)
        same = dict(kernel_size=final_kernel, stride=1, padding=final_kernel // 2)
        for name, (channels, num_conv) in heads.items():
            # num_conv - 1 hidden stages (conv, norm, ReLU) of width head_conv, then the output convolution with its bias
            widths = [in_channels] + [head_conv] * (num_conv - 1)
            stack = [ConvModule(a, b, bias=bias, conv_cfg=conv_cfg, norm_cfg=norm_cfg, **same) for a, b in zip(widths, widths[1:])]
            stack.append(build_conv_layer(conv_cfg, head_conv, channels, bias=True, **same))
            setattr(self, name, nn.Sequential(*stack))

    def init_weights(self):
        """The heatmap head starts from `init_bias` (a sigmoid of 0.1); 2-d convolutions of the other heads get Kaiming weights.
        Written under no_grad, not through `.data`: the parameter's version moves and `folded()` sees the change."""
        with torch.no_grad():
            for name in self.heads:
                if name == "heatmap":
                    getattr(self, name)[-1].bias.fill_(self.init_bias)
                    continue
                for m in getattr(self, name).modules():
                    if isinstance(m, nn.Conv2d):
                        nn.init.kaiming_normal_(m.weight, a=0, mode="fan_out", nonlinearity="relu")
                        if m.bias is not None:
                            m.bias.zero_()

    # ---- fused eval path ----
    def _foldable(self):
        """Every head is Conv1d(k = 1, no bias) -> BatchNorm1d with running statistics, in eval mode -> ReLU -> Conv1d(k = 1)."""
        if self.final_kernel != 1 or not 1 <= len(self.heads) <= FFN_MAX_HEADS:
            return False
        if self.in_channels % 4 or self.in_channels > FFN_MAX_IN or self.head_conv % 16 or self.head_conv > FFN_MAX_HEAD_CONV:
            return False
        for head, (classes, num_conv) in self.heads.items():
            seq = getattr(self, head)
            if num_conv != 2 or not 1 <= classes <= FFN_MAX_CHANNELS or not isinstance(seq[0], ConvModule):
                return False
            first, last = seq[0], seq[1]
            bn = first.norm
            if not (isinstance(first.conv, nn.Conv1d) and isinstance(last, nn.Conv1d) and isinstance(bn, nn.BatchNorm1d)):
                return False
            if first.conv.bias is not None or not first.with_activation or last.bias is None:
                return False
            if bn.training or bn.running_mean is None or bn.running_var is None:
                return False
        return True

    def fusable(self, x):
        """True when forward(x) runs the fused kernel."""
        if not (self.use_fused and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and not self.training):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return x.shape[1] == self.in_channels and x.shape[2] >= 1 and self._foldable()

    def folded(self):
        """Per head (w1 [head_conv, Cin], scale, shift, w2 [c, head_conv], bias [c]) of the eval-mode stack, fp32, cached on the
        parameters' and buffers' addresses and versions.  Every in-place torch operation moves the version (`load_state_dict`,
        an optimizer step, `init_weights`); a write through `.data` does not, and after one the cache has to be dropped by hand
        (`del ffn._bevamd_folded`).  Run one forward before capturing a graph: a fold computed inside a capture is filled only
        when the graph replays."""
        tensors = []
        for head in self.heads:
            seq = getattr(self, head)
            bn = seq[0].norm
            tensors += [seq[0].conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, seq[1].weight, seq[1].bias]
        key = tuple((t.data_ptr(), t._version, t.dtype, t.device) if t is not None else None for t in tensors)
        cache = self.__dict__.get("_bevamd_folded")
        if cache is not None and cache[0] == key:
            return cache[1]
        val = []
        for head in self.heads:
            seq = getattr(self, head)
            bn = seq[0].norm
            inv = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
            g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(inv)
            b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(inv)
            scale = (g * inv).contiguous()
            shift = (b - bn.running_mean.detach().float() * scale).contiguous()
            val.append((_dense(seq[0].conv.weight[:, :, 0]), scale, shift, _dense(seq[1].weight[:, :, 0]), _dense(seq[1].bias)))
        self.__dict__["_bevamd_folded"] = (key, val)
        return val

    def forward(self, x, query_pos=None, out=None, layer=0):
        names = list(self.heads)
        if query_pos is not None and ("center" not in self.heads or self.heads["center"][0] != 2):
            raise RuntimeError("query_pos is added to a `center` head of 2 channels: this FFN has none")
        P = x.shape[-1]
        lo = int(layer) * P
        if out is not None and any(name not in out or out[name].shape[-1] < lo + P for name in names):
            raise RuntimeError(f"out must hold every head with at least {lo + P} columns")
        if self.fusable(x):
            params = self.folded()
            if any(t.device != x.device for p in params for t in p):
                raise RuntimeError("module parameters and x live on different devices")
            outs = None if out is None else [out[name] for name in names]
            if outs is None or all(o.is_contiguous() and o.dtype == torch.float32 and o.device == x.device for o in outs):
                center = names.index("center") if query_pos is not None else -1
                res = head_ffn_forward(x, params, query_pos, center, outs, lo)
                if res is not None:
                    return {name: (t if out is None else t[..., lo:lo + P]) for name, t in zip(names, res)}
        ret = {}
        for head in names:
            ret[head] = getattr(self, head)(x)
        if query_pos is not None:
            ret["center"] = ret["center"] + query_pos.permute(0, 2, 1)
        if out is not None:
            for head in names:
                out[head][..., lo:lo + P] = ret[head]
                ret[head] = out[head][..., lo:lo + P]
        return ret


def _build(cfg, registry):
    return build_from_cfg(cfg, registry) if isinstance(cfg, dict) else cfg


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg[key] if key in cfg else default


class TransFusionHead(nn.Module):
    def __init__(self, num_proposals=128, auxiliary=True, in_channels=128 * 3, hidden_channel=128, num_classes=4,
                 # config for Transformer
                 num_decoder_layers=3, num_heads=8, nms_kernel_size=1, ffn_channel=256, dropout=0.1, bn_momentum=0.1, activation="relu",
                 # config for FFN
                 common_heads=dict(), num_heatmap_convs=2, conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"), bias="auto",
                 # loss
                 loss_cls=dict(type="GaussianFocalLoss", reduction="mean"),
                 loss_iou=dict(type="VarifocalLoss", use_sigmoid=True, iou_weighted=True, reduction="mean"),
                 loss_bbox=dict(type="L1Loss", reduction="mean"), loss_heatmap=dict(type="GaussianFocalLoss", reduction="mean"),
                 # others
                 train_cfg=None, test_cfg=None, bbox_coder=None):
        super().__init__()
        from . import heads  # noqa: F401  (fills the coder, assigner and loss registries the config blocks are built from)

        self.fp16_enabled = False
        self.num_classes = num_classes
        self.num_proposals = num_proposals
        self.auxiliary = auxiliary
        self.in_channels = in_channels
        self.num_heads = num_heads
        self.num_decoder_layers = num_decoder_layers
        self.bn_momentum = bn_momentum
        self.nms_kernel_size = nms_kernel_size
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg

        self.use_sigmoid_cls = loss_cls.get("use_sigmoid", False)
        if not self.use_sigmoid_cls:
            self.num_classes += 1
        self.loss_cls = _build(loss_cls, LOSSES)
        self.loss_bbox = _build(loss_bbox, LOSSES)
        self.loss_iou = loss_iou            # never called by the reference's loss(); kept as its config
        self.loss_heatmap = _build(loss_heatmap, LOSSES)
        self.bbox_coder = _build(bbox_coder, BBOX_CODERS) if bbox_coder is not None else None
        self.sampling = False

        self.shared_conv = build_conv_layer(dict(type="Conv2d"), in_channels, hidden_channel, kernel_size=3, padding=1,
                                            bias=True if bias == "auto" else bias)
        layers = [ConvModule(hidden_channel, hidden_channel, kernel_size=3, padding=1, bias=bias, conv_cfg=dict(type="Conv2d"),
                             norm_cfg=dict(type="BN2d")),
                  build_conv_layer(dict(type="Conv2d"), hidden_channel, num_classes, kernel_size=3, padding=1,
                                   bias=True if bias == "auto" else bias)]
        self.heatmap_head = nn.Sequential(*layers)
        self.class_encoding = nn.Conv1d(num_classes, hidden_channel, 1)

        self.decoder = nn.ModuleList()
        for _ in range(self.num_decoder_layers):
            self.decoder.append(TransformerDecoderLayer(hidden_channel, num_heads, ffn_channel, dropout, activation,
                                                        self_posembed=PositionEmbeddingLearned(2, hidden_channel),
                                                        cross_posembed=PositionEmbeddingLearned(2, hidden_channel)))

        self.prediction_heads = nn.ModuleList()
        for _ in range(self.num_decoder_layers):
            heads = copy.deepcopy(common_heads)
            heads.update(dict(heatmap=(self.num_classes, num_heatmap_convs)))
            self.prediction_heads.append(FFN(hidden_channel, heads, conv_cfg=conv_cfg, norm_cfg=norm_cfg, bias=bias))

        self.use_fused = True   # eval mode: the category-encoding kernel and the fused prediction heads (False: the torch layers)
        # eval mode: shared_conv and heatmap_head run with cudnn.benchmark off and cudnn.deterministic on (process-wide flags, set
        # around the two calls and restored); False leaves the caller's flags alone and gives up bit-equal calls
        self.deterministic_convs = True

        self.init_weights()
        self._init_assigner_sampler()

        # positions of the BEV cells for the cross-attention
        x_size = self.test_cfg["grid_size"][0] // self.test_cfg["out_size_factor"]
        y_size = self.test_cfg["grid_size"][1] // self.test_cfg["out_size_factor"]
        self.register_buffer("bev_pos", self.create_2D_grid(x_size, y_size), persistent=False)
        self.img_feat_pos = None
        self.img_feat_collapsed_pos = None
        self.query_labels = None

    @property
    def use_fused(self):
        return self._use_fused

    @use_fused.setter
    def use_fused(self, value):
        """One switch for the category encoding and for every layer's prediction heads."""
        self._use_fused = bool(value)
        for ffn in self.prediction_heads:
            ffn.use_fused = bool(value)

    def create_2D_grid(self, x_size, y_size):
        """[1, x_size * y_size, 2]: the centre (i + 0.5, j + 0.5) of BEV cell i * y_size + j."""
        i = torch.linspace(0, x_size - 1, x_size) + 0.5
        j = torch.linspace(0, y_size - 1, y_size) + 0.5
        return torch.stack([i[:, None].expand(x_size, y_size), j[None, :].expand(x_size, y_size)], dim=-1).reshape(1, -1, 2).contiguous()

    def init_weights(self):
        """Xavier-uniform matrices in the decoder, the prediction heads' own initialisation, then the BatchNorm momentum."""
        for p in self.decoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for ffn in self.prediction_heads:
            ffn.init_weights()
        self.init_bn_momentum()

    def init_bn_momentum(self):
        for m in self.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                m.momentum = self.bn_momentum

    def _init_assigner_sampler(self):
        if self.train_cfg is None:
            return
        assigner = self.train_cfg["assigner"]
        if isinstance(assigner, dict):
            self.bbox_assigner = _build(assigner, BBOX_ASSIGNERS)
        elif isinstance(assigner, list):
            self.bbox_assigner = [_build(res, BBOX_ASSIGNERS) for res in assigner]
        else:
            self.bbox_assigner = assigner

    # ---- forward ----
    def _fused(self, x):
        return self.use_fused and not self.training and x.is_cuda and x.dtype == torch.float32 and not (
            torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.class_encoding.parameters())))

    def forward_single(self, inputs, img_inputs=None, metas=None):
        from .heads import transfusion_select_proposals                       # heads re-exports this module

        _need_gpu(inputs)
        batch_size = inputs.shape[0]
        with _deterministic_convs() if self.deterministic_convs and not self.training else contextlib.nullcontext():
            lidar_feat = self.shared_conv(inputs)
            dense_heatmap = self.heatmap_head(lidar_feat)
        lidar_feat_flatten = lidar_feat.view(batch_size, lidar_feat.shape[1], -1)     # [B, C, H * W]
        bev_pos = self.bev_pos
        if bev_pos.device != lidar_feat.device:
            raise RuntimeError(f"the module lives on {bev_pos.device}, the features on {lidar_feat.device}")

        sel = transfusion_select_proposals(dense_heatmap.float(), lidar_feat_flatten, bev_pos, self.num_proposals, self.nms_kernel_size,
                                           self.test_cfg["dataset"])
        self.query_labels = sel.top_proposals_class
        index = sel.top_proposals_index

        # category encoding
        if self._fused(lidar_feat_flatten):
            query_feat = head_class_encoding(sel.query_feat, sel.top_proposals_class, self.class_encoding.weight, self.class_encoding.bias)
        else:
            query_feat = lidar_feat_flatten.gather(index=index[:, None, :].expand(-1, lidar_feat_flatten.shape[1], -1), dim=-1)
            one_hot = F.one_hot(sel.top_proposals_class, num_classes=self.num_classes).permute(0, 2, 1)
            query_feat = query_feat + self.class_encoding(one_hot.to(query_feat.dtype))
        query_pos = sel.query_pos
        bev_pos = bev_pos.expand(batch_size, -1, -1)

        L, P = self.num_decoder_layers, self.num_proposals
        ret_dicts = []
        outs = None
        for i in range(L):
            query_feat = self.decoder[i](query_feat, lidar_feat_flatten, query_pos, bev_pos)
            ffn = self.prediction_heads[i]
            if self.auxiliary and L > 1 and i == 0 and all(f.fusable(query_feat) for f in self.prediction_heads):
                outs = {name: torch.empty((batch_size, c, L * P), dtype=torch.float32, device=query_feat.device)
                        for name, (c, _) in ffn.heads.items()}
            res_layer = ffn(query_feat, query_pos, out=outs, layer=i)
            ret_dicts.append(res_layer)
            query_pos = res_layer["center"].detach().clone().permute(0, 2, 1)          # the next layer's positions

        ret_dicts[0]["query_heatmap_score"] = sel.query_heatmap_score                 # [B, num_classes, num_proposals]
        ret_dicts[0]["dense_heatmap"] = dense_heatmap
        if self.auxiliary is False:
            return [ret_dicts[-1]]                                                    # the last layer only
        new_res = {}
        for key in ret_dicts[0].keys():
            if key in ("dense_heatmap", "dense_heatmap_old", "query_heatmap_score"):
                new_res[key] = ret_dicts[0][key]
            elif outs is not None:
                new_res[key] = outs[key]
            elif L == 1:
                new_res[key] = ret_dicts[0][key]
            else:
                new_res[key] = torch.cat([ret_dict[key] for ret_dict in ret_dicts], dim=-1)
        return [new_res]

    def forward(self, feats, metas=None):
        """feats: [B, in_channels, H, W] (or a one-entry list of it) -> [[dict]], first index level, second the one dict."""
        if isinstance(feats, torch.Tensor):
            feats = [feats]
        assert len(feats) == 1, "only support one level features."
        return [self.forward_single(feats[0], None, metas)]

    # ---- the ends ----
    def _layers(self):
        return self.num_decoder_layers if self.auxiliary else 1

    def get_targets(self, gt_bboxes_3d, gt_labels_3d, preds_dict, **kwargs):
        from .heads import transfusion_get_targets

        if self.train_cfg is None:
            raise RuntimeError("get_targets needs the head's train_cfg")
        return transfusion_get_targets(gt_bboxes_3d, gt_labels_3d, preds_dict, self.bbox_coder, self.bbox_assigner, self.train_cfg,
                                       self.num_proposals, self.num_classes, self.num_decoder_layers, self.auxiliary, **kwargs)

    def loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, **kwargs):
        from .heads import transfusion_loss

        targets = self.get_targets(gt_bboxes_3d, gt_labels_3d, preds_dicts[0], **kwargs)
        code_weights = _get(self.train_cfg, "code_weights")
        extra = {} if code_weights is None else dict(code_weights=code_weights)
        return transfusion_loss(preds_dicts, targets, self.num_proposals, self.num_classes, self.num_decoder_layers, self.auxiliary,
                                loss_cls=self.loss_cls, loss_bbox=self.loss_bbox, loss_heatmap=self.loss_heatmap, **extra)

    def get_bboxes(self, preds_dicts, metas=None, img=None, rescale=False, for_roi=False, sync=True):
        from .heads import transfusion_get_bboxes

        assert len(preds_dicts) == 1 and len(preds_dicts[0]) == 1, "one level, one dict"
        ret = transfusion_get_bboxes(preds_dicts[0][0], self.query_labels, self.bbox_coder, self.test_cfg, self.num_proposals,
                                     self.num_classes, sync=sync)
        if not sync or metas is None:
            return ret
        out = []
        for i, r in enumerate(ret):
            box_type = metas[i].get("box_type_3d") if i < len(metas) else None
            boxes = box_type(r["bboxes"], box_dim=r["bboxes"].shape[-1]) if box_type is not None else r["bboxes"]
            out.append([boxes, r["scores"], r["labels"].int()])
        return out


register_everywhere("head", TransFusionHead)
