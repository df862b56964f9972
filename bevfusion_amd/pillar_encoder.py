"""Pillar and radar encoders: PillarFeatureNet, RadarFeatureNet, PointPillarsScatter and the two encoders that chain them
(reference: mmdet3d/models/backbones/pillar_encoder.py, radar_encoder.py), registered under the reference's names so that
`configs/nuscenes/det/transfusion/secfpn/lidar/pointpillars.yaml` and `.../centerhead/lssfpn/camera+radar/default.yaml` build.

Module trees and state-dict keys are the reference's (`pfn_layers.0.linear.weight`, `rfn_layers.3.norm.running_var`, ...), so its
checkpoints load.  Dispatch of the feature nets:

  * GPU tensors, eval mode: ONE launch of the fused stack (csrc/ext/pillar_encoder.hip: decorate -> [Linear -> folded BatchNorm
    -> ReLU -> combine] per layer, per pillar from LDS and registers; only [M, C_out] is written);
  * GPU tensors, train mode (or a shape outside the fused kernel's limits: more than 4 layers, a width above 128 or not a
    multiple of 4, more than 64 input columns, more than 32 rows per pillar): the decorate kernel, then the module's own
    nn.Linear / BatchNorm1d / ReLU / max — batch statistics, running-stat updates and autograd exactly as in the reference
    (the Linear's weight gradient is summed in blocks of 512 rows: same value, a tenth of the rounding error of one long GEMM);
  * host tensors: the reference's formulation in plain torch (a host algorithm like `bev_pool()` on host tensors, never a
    fallback for GPU tensors).  Without the ext library GPU tensors raise `NativeLibraryMissing`.

`PointPillarsScatter` on GPU tensors is two kernels without a batch loop (winner plane by atomicMax of the row id, then one pass
over the whole canvas), with a backward that reuses the winner plane.

Differences from the reference, on purpose:

  * `RadarFeatureNet` does not overwrite the caller's `features` (the reference normalises xyz in place);
  * the result is [M, C] for every M (the reference's bare `.squeeze()` collapses M = 1);
  * `num_voxels >= 1` per pillar is required (the reference yields NaN rows from 0 / 0 in `PillarFeatureNet`; the fused kernel
    returns the padded-row value for such a pillar);
  * the inputs are sensor data and carry no gradient: `features.requires_grad` raises;
  * scatter: a duplicated cell takes the HIGHEST row (what the reference's sequential index_put leaves on one CPU thread;
    deterministic here); rows whose batch index is outside [0, batch_size) are dropped as the reference's mask drops them; rows
    with x or y outside the canvas — an index error in the reference — are dropped by the GPU kernels.
"""
import ctypes
from typing import Any, Dict

import torch
from torch import nn
from torch.nn import functional as F

from . import _capi
from .registry import BACKBONES, build_norm_layer, register_everywhere

__all__ = ["PillarFeatureNet", "RadarFeatureNet", "PointPillarsScatter", "PointPillarsEncoder", "RadarEncoder", "PFNLayer",
           "RFNLayer", "get_paddings_indicator", "pillar_decorate", "pillar_scatter"]

MODE_PILLAR, MODE_RADAR = 0, 1
_UNSUPPORTED = 4   # BEVAMD_ERR_UNSUPPORTED


def build_backbone(cfg):
    return BACKBONES.build(cfg)


def get_paddings_indicator(actual_num, max_num, axis=0):
    """Boolean mask [N, max_num]: True for the first actual_num[i] entries of row i."""
    actual_num = torch.unsqueeze(actual_num, axis + 1)
    max_num_shape = [1] * len(actual_num.shape)
    max_num_shape[axis + 1] = -1
    max_num = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(max_num_shape)
    return actual_num.int() > max_num


_WGRAD_ROWS = 512   # rows per partial sum of the weight gradient on GPU tensors


class _RowsLinear(torch.autograd.Function):
    """`F.linear(x, w)` over [M, P, K] rows (no bias) whose weight gradient is summed in blocks of _WGRAD_ROWS rows.

    The forward and the input gradient are torch's own GEMMs.  The weight gradient g^T x reduces over all M * P rows (1.2 M at
    the radar config's cap); as ONE fp32 GEMM on the GPU its error against float64 was 1.5e-5 / 4.0e-5 of max |dW| on the last
    layer of the pillar / radar nets (16 000 / 7 200 rows), ten times what the CPU's blocked GEMM leaves.  Per-block partial
    GEMMs (one bmm) followed by a sum over the blocks give 1.5e-6 / 5.0e-6, measured on an MI355X."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return F.linear(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx = g @ w if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            g2, x2 = g.reshape(-1, g.shape[-1]), x.reshape(-1, x.shape[-1])
            pad = (-g2.shape[0]) % _WGRAD_ROWS
            if pad:
                g2, x2 = F.pad(g2, (0, 0, 0, pad)), F.pad(x2, (0, 0, 0, pad))
            dw = torch.bmm(g2.view(-1, _WGRAD_ROWS, g2.shape[1]).transpose(1, 2), x2.view(-1, _WGRAD_ROWS, x2.shape[1])).sum(0)
        return dx, dw


class _FNLayer(nn.Module):
    """Linear (no bias) -> BatchNorm1d -> ReLU over [M, P, C_in]; the subclasses differ in `units` and in what they return."""

    def __init__(self, in_channels, units, norm_cfg, last_layer):
        super().__init__()
        self.last_vfe = last_layer
        self.units = units
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
        self.norm_cfg = norm_cfg
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = build_norm_layer(self.norm_cfg, self.units)[1]

    def _activations(self, inputs):
        if inputs.is_cuda and self.linear.bias is None and torch.is_grad_enabled() and self.linear.weight.requires_grad:
            x = _RowsLinear.apply(inputs, self.linear.weight)
        else:
            x = self.linear(inputs)
        with torch.backends.cudnn.flags(enabled=False):   # the reference switches the vendor BatchNorm off around this call
            x = self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
        return F.relu(x)

    def folded(self):
        """(weight transposed [K, units], scale, shift) of the eval-mode layer, fp32, cached on the parameter versions."""
        bn = self.norm
        tensors = (self.linear.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = tuple((t.data_ptr(), t._version, t.dtype, t.device) if t is not None else None for t in tensors)
        cache = self.__dict__.get("_bevamd_folded")
        if cache is not None and cache[0] == key:
            return cache[1]
        inv = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
        g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(inv)
        b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(inv)
        scale = (g * inv).contiguous()
        shift = (b - bn.running_mean.detach().float() * scale).contiguous()
        val = (self.linear.weight.detach().float().t().contiguous(), scale, shift)
        self.__dict__["_bevamd_folded"] = (key, val)
        return val

    def foldable(self):
        bn = self.norm
        return (isinstance(bn, nn.BatchNorm1d) and not bn.training and bn.running_mean is not None
                and bn.running_var is not None and self.linear.bias is None)


class PFNLayer(_FNLayer):
    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__(in_channels, out_channels if last_layer else out_channels // 2, norm_cfg, last_layer)
        self.name = "PFNLayer"

    def forward(self, inputs):
        x = self._activations(inputs)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)


class RFNLayer(_FNLayer):
    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__(in_channels, out_channels, norm_cfg, last_layer)
        self.name = "RFNLayer"

    def forward(self, inputs):
        x = self._activations(inputs)
        if self.last_vfe:
            return torch.max(x, dim=1, keepdim=True)[0]
        return x


def _geom(net):
    r = net.pc_range
    return _capi.floats([net.vx, net.vy, net.x_offset, net.y_offset, r[0], r[1], r[2], r[3] - r[0], r[4] - r[1], r[5] - r[2]])


def _gpu_inputs(features, num_voxels, coors):
    if features.requires_grad:
        raise RuntimeError("pillar features are sensor data and carry no gradient: features.requires_grad is set")
    if features.dim() != 3 or features.dtype != torch.float32:
        raise RuntimeError(f"features must be [M, P, F] float32, got {tuple(features.shape)} {features.dtype}")
    M = features.shape[0]
    if num_voxels.shape != (M,) or coors.dim() != 2 or coors.shape[0] != M or coors.shape[1] < 3:
        raise RuntimeError(f"num_voxels must be [M] and coors [M, 4], got {tuple(num_voxels.shape)} and {tuple(coors.shape)}")
    if coors.shape[1] != 4:
        coors = F.pad(coors, (0, 4 - coors.shape[1]))
    return (features.detach().contiguous(), num_voxels.to(device=features.device, dtype=torch.int32).contiguous(),
            coors.to(device=features.device, dtype=torch.int32).contiguous())


def pillar_decorate(features, num_voxels, coors, net):
    """[M, P, F_out] decorated rows of `net` (a PillarFeatureNet / RadarFeatureNet) on GPU tensors: one HIP launch."""
    if not features.is_cuda:
        raise RuntimeError("pillar_decorate needs GPU tensors (host tensors run the module's torch formulation)")
    lib = _capi.load()
    features, num_voxels, coors = _gpu_inputs(features, num_voxels, coors)
    M, P, Fin = features.shape
    out = torch.empty((M, P, net.decorated_channels), dtype=torch.float32, device=features.device)
    with torch.cuda.device(features.device):
        rc = lib.bevamd_pillar_decorate(_capi.ptr(features), _capi.ptr(num_voxels), _capi.ptr(coors), M, P, Fin, net.mode,
                                        int(net._with_distance), _geom(net), _capi.ptr(out), _capi.stream_ptr(features.device))
    _capi.check(rc, "pillar_decorate")
    return out


class _FeatureNet(nn.Module):
    mode = MODE_PILLAR
    layer_cls = PFNLayer
    layers_name = "pfn_layers"

    def __init__(self, in_channels=4, feat_channels=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 point_cloud_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None):
        super().__init__()
        assert len(feat_channels) > 0
        self.in_channels = in_channels
        self._with_distance = with_distance
        self.decorated_channels = self._decorated(in_channels, with_distance)
        widths = [self.decorated_channels] + list(feat_channels)
        layers = [self.layer_cls(widths[i], widths[i + 1], norm_cfg=norm_cfg, last_layer=i == len(widths) - 2)
                  for i in range(len(widths) - 1)]
        setattr(self, self.layers_name, nn.ModuleList(layers))
        # pillar size and the centre of cell 0, in double as the reference's constructor computes them
        self.vx = voxel_size[0]
        self.vy = voxel_size[1]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.pc_range = point_cloud_range
        self.use_fused = True   # eval mode on GPU tensors: the fused stack (False: decorate kernel + torch layers)

    @property
    def layers(self):
        return getattr(self, self.layers_name)

    # ---- host tensors: the reference's formulation ----
    def _decorate_host(self, features, num_voxels, coors):
        raise NotImplementedError

    def _center(self, features, coors):
        dtype = features.dtype
        f_center = torch.zeros_like(features[:, :, :2])
        f_center[:, :, 0] = features[:, :, 0] - (coors[:, 1].to(dtype).unsqueeze(1) * self.vx + self.x_offset)
        f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * self.vy + self.y_offset)
        return f_center

    def decorate(self, features, num_voxels, coors):
        """The decorated, masked [M, P, F_out] rows the layers consume."""
        if features.is_cuda:
            return pillar_decorate(features, num_voxels, coors, self)
        if features.requires_grad:
            raise RuntimeError("pillar features are sensor data and carry no gradient: features.requires_grad is set")
        return self._decorate_host(features, num_voxels, coors)

    def _fused(self, features, num_voxels, coors):
        """[M, C] from the fused stack, None when the kernel does not support the shape."""
        lib = _capi.load()
        features, num_voxels, coors = _gpu_inputs(features, num_voxels, coors)
        M, P, Fin = features.shape
        layers = list(self.layers)
        n = len(layers)
        params = [layer.folded() for layer in layers]
        if any(t.device != features.device for p in params for t in p):
            raise RuntimeError("module parameters and features live on different devices")
        out = torch.empty((M, layers[-1].units), dtype=torch.float32, device=features.device)
        arr = lambda k: (ctypes.c_void_p * n)(*[p[k].data_ptr() for p in params])   # noqa: E731
        with torch.cuda.device(features.device):
            rc = lib.bevamd_pillar_stack_forward(_capi.ptr(features), _capi.ptr(num_voxels), _capi.ptr(coors), M, P, Fin, self.mode,
                                                 int(self._with_distance), _geom(self), n, _capi.ints([l.units for l in layers]),
                                                 arr(0), arr(1), arr(2), _capi.ptr(out), _capi.stream_ptr(features.device))
        if rc == _UNSUPPORTED:
            return None
        _capi.check(rc, "pillar_stack_forward")
        return out

    def forward(self, features, num_voxels, coors):
        if features.is_cuda and self.use_fused and not self.training:   # inference: the result carries no gradient
            if all(layer.foldable() for layer in self.layers):
                out = self._fused(features, num_voxels, coors)
                if out is not None:
                    return out
        x = self.decorate(features, num_voxels, coors)
        for layer in self.layers:
            x = layer(x)
        return x.squeeze(1)


class PillarFeatureNet(_FeatureNet):
    """Pillar Feature Net: [features, f_cluster, f_center(, distance)] -> PFNLayers -> [M, C]."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.name = "PillarFeatureNet"

    @staticmethod
    def _decorated(in_channels, with_distance):
        return in_channels + 5 + (1 if with_distance else 0)

    def _decorate_host(self, features, num_voxels, coors):
        points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_voxels.type_as(features).view(-1, 1, 1)
        f_cluster = features[:, :, :3] - points_mean
        features_ls = [features, f_cluster, self._center(features, coors)]
        if self._with_distance:
            features_ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
        features = torch.cat(features_ls, dim=-1)
        mask = get_paddings_indicator(num_voxels, features.shape[1], axis=0)
        features *= torch.unsqueeze(mask, -1).type_as(features)
        return features


class RadarFeatureNet(_FeatureNet):
    """Radar Feature Net: [features with xyz normalised to the range, f_center] -> RFNLayers -> [M, C]."""
    mode = MODE_RADAR
    layer_cls = RFNLayer
    layers_name = "rfn_layers"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.name = "RadarFeatureNet"
        self.export_onnx = False

    @staticmethod
    def _decorated(in_channels, with_distance):
        return in_channels + 2

    def _decorate_host(self, features, num_voxels, coors):
        f_center = self._center(features, coors)
        features = features.clone()   # the reference normalises the caller's tensor in place
        r = self.pc_range
        features[:, :, 0:1] = (features[:, :, 0:1] - r[0]) / (r[3] - r[0])
        features[:, :, 1:2] = (features[:, :, 1:2] - r[1]) / (r[4] - r[1])
        features[:, :, 2:3] = (features[:, :, 2:3] - r[2]) / (r[5] - r[2])
        features = torch.cat([features, f_center], dim=-1)
        mask = get_paddings_indicator(num_voxels, features.shape[1], axis=0)
        features *= torch.unsqueeze(mask, -1).type_as(features)
        return torch.nan_to_num(features)


_SCATTER_DTYPES = {torch.float32: 0, torch.float16: 1}


class _PillarScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, coors, batch_size, nx, ny):
        lib = _capi.load()
        if feats.dtype not in _SCATTER_DTYPES:
            raise RuntimeError(f"pillar_scatter handles float32 and float16 features, got {feats.dtype}")
        feats = feats.contiguous()
        M, C = feats.shape
        winner = torch.empty((batch_size, nx * ny), dtype=torch.int32, device=feats.device)
        canvas = torch.empty((batch_size, C, nx, ny), dtype=feats.dtype, device=feats.device)
        with torch.cuda.device(feats.device):
            rc = lib.bevamd_pillar_scatter_forward(_capi.ptr(feats), _SCATTER_DTYPES[feats.dtype], _capi.ptr(coors), M, C,
                                                   batch_size, nx, ny, _capi.ptr(winner), _capi.ptr(canvas),
                                                   _capi.stream_ptr(feats.device))
        _capi.check(rc, "pillar_scatter_forward")
        ctx.save_for_backward(coors, winner)
        ctx.geom = (M, C, batch_size, nx, ny)
        return canvas

    @staticmethod
    def backward(ctx, grad):
        coors, winner = ctx.saved_tensors
        M, C, B, nx, ny = ctx.geom
        grad = grad.contiguous()
        out = torch.empty((M, C), dtype=grad.dtype, device=grad.device)
        with torch.cuda.device(grad.device):
            rc = _capi.load().bevamd_pillar_scatter_backward(_capi.ptr(grad), _SCATTER_DTYPES[grad.dtype], _capi.ptr(coors),
                                                             _capi.ptr(winner), M, C, B, nx, ny, _capi.ptr(out),
                                                             _capi.stream_ptr(grad.device))
        _capi.check(rc, "pillar_scatter_backward")
        return out, None, None, None, None


def pillar_scatter(voxel_features, coords, batch_size, nx, ny):
    """canvas [B, C, nx, ny] with canvas[b, :, x, y] = voxel_features[row] for coords[row] = (b, x, y, z); GPU tensors."""
    if not voxel_features.is_cuda:
        raise RuntimeError("pillar_scatter needs GPU tensors (host tensors run the module's torch formulation)")
    if voxel_features.dim() != 2 or coords.dim() != 2 or coords.shape[0] != voxel_features.shape[0] or coords.shape[1] < 3:
        raise RuntimeError(f"voxel_features must be [M, C] and coords [M, 4], got {tuple(voxel_features.shape)} and "
                           f"{tuple(coords.shape)}")
    if coords.shape[1] != 4:
        coords = F.pad(coords, (0, 4 - coords.shape[1]))
    coords = coords.to(device=voxel_features.device, dtype=torch.int32).contiguous()
    return _PillarScatter.apply(voxel_features, coords, int(batch_size), int(nx), int(ny))


class PointPillarsScatter(nn.Module):
    """Learned pillar features [M, C] -> dense pseudo image [B, C, nx, ny]."""

    def __init__(self, in_channels=64, output_shape=(512, 512), **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.output_shape = output_shape
        self.nx = output_shape[0]
        self.ny = output_shape[1]

    def extra_repr(self):
        return f"in_channels={self.in_channels}, output_shape={tuple(self.output_shape)}"

    def forward(self, voxel_features, coords, batch_size):
        if voxel_features.is_cuda:
            if voxel_features.shape[1] != self.in_channels:
                raise RuntimeError(f"expected {self.in_channels} channels, got {voxel_features.shape[1]}")
            return pillar_scatter(voxel_features, coords, batch_size, self.nx, self.ny)
        batch_canvas = []
        for batch_itt in range(batch_size):
            canvas = torch.zeros(self.in_channels, self.nx * self.ny, dtype=voxel_features.dtype, device=voxel_features.device)
            batch_mask = coords[:, 0] == batch_itt
            this_coords = coords[batch_mask, :]
            indices = (this_coords[:, 1] * self.ny + this_coords[:, 2]).type(torch.long)
            canvas[:, indices] = voxel_features[batch_mask, :].t()
            batch_canvas.append(canvas)
        return torch.stack(batch_canvas, 0).view(batch_size, self.in_channels, self.nx, self.ny)


class PointPillarsEncoder(nn.Module):
    def __init__(self, pts_voxel_encoder: Dict[str, Any], pts_middle_encoder: Dict[str, Any], **kwargs):
        super().__init__()
        self.pts_voxel_encoder = build_backbone(pts_voxel_encoder)
        self.pts_middle_encoder = build_backbone(pts_middle_encoder)

    def forward(self, feats, coords, batch_size, sizes):
        x = self.pts_voxel_encoder(feats, sizes, coords)
        return self.pts_middle_encoder(x, coords, batch_size)


class RadarEncoder(nn.Module):
    def __init__(self, pts_voxel_encoder: Dict[str, Any], pts_middle_encoder: Dict[str, Any], pts_transformer_encoder=None,
                 pts_bev_encoder=None, post_scatter=None, **kwargs):
        super().__init__()
        self.pts_voxel_encoder = build_backbone(pts_voxel_encoder)
        self.pts_middle_encoder = build_backbone(pts_middle_encoder)
        self.pts_transformer_encoder = build_backbone(pts_transformer_encoder) if pts_transformer_encoder is not None else None
        self.pts_bev_encoder = build_backbone(pts_bev_encoder) if pts_bev_encoder is not None else None
        self.post_scatter = build_backbone(post_scatter) if post_scatter is not None else None

    def forward(self, feats, coords, batch_size, sizes, img_features=None):
        x = self.pts_voxel_encoder(feats, sizes, coords)
        if self.pts_transformer_encoder is not None:
            x = self.pts_transformer_encoder(x, sizes, coords, batch_size)
        x = self.pts_middle_encoder(x, coords, batch_size)
        if self.post_scatter is not None:
            x = self.post_scatter(x, img_features)
        if self.pts_bev_encoder is not None:
            x = self.pts_bev_encoder(x)
        return x


for _cls in (PillarFeatureNet, RadarFeatureNet, PointPillarsScatter, PointPillarsEncoder, RadarEncoder):
    register_everywhere("backbone", _cls)
