"""The camera depth nets (cam_nets.py, csrc/ext/cam_nets.hip) without a GPU: the folds against float64, the fold caches, which calls
take the fused route, the unchanged default, the entry points' refusals, the binding table and the kernels' resources."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import test_kernel_resources as resources
from bevfusion_amd import _capi, bev_trunk as bt, cam_nets as cn, heads
from bevfusion_amd.vtransforms import BaseTransform, DepthLSSTransform, FactoredCamFeats, LSSTransform
from test_centerhead_module import _lds_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL = dict(out_channels=4, image_size=(16, 24), feature_size=(2, 3), xbound=[-8.0, 8.0, 1.0], ybound=[-8.0, 8.0, 1.0],
             zbound=[-10.0, 10.0, 20.0], dbound=[1.0, 6.0, 1.0])


def randomise(module, seed):
    """Parameters and running statistics that are not the defaults, biases included."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                K = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / K) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_((0.8 + 0.4 * torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.25, -1.0, 1.0))
                m.bias.copy_(0.3 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(n, generator=g))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=g))
    return module


def small_transform(kind="depth", in_channels=32, seed=0):
    cls = DepthLSSTransform if kind == "depth" else LSSTransform
    return randomise(cls(in_channels=in_channels, **SMALL), seed).eval()


def small_inputs(in_channels=32, seed=1, B=1, N=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, in_channels, 2, 3, generator=g)
    d = torch.where(torch.rand(B, N, 1, 16, 24, generator=g) < 0.3, 40.0 * torch.rand(B, N, 1, 16, 24, generator=g), torch.zeros(()))
    return x, d


# ---- exports -----------------------------------------------------------------------------------------------------------------------
def test_the_module_is_reexported_where_the_bev_trunk_is():
    for name in ("fold_conv_bias_bn", "fold_depth_stem", "fold_depth_head", "depth_stem_forward", "depth_head_forward", "DepthStemFold",
                 "DepthHeadFold"):
        assert getattr(heads, name) is getattr(cn, name) and name in heads.__all__
    assert small_transform().cam_nets_dtype is None and small_transform("lss").cam_nets_dtype is None      # the default: fp32 layers


# ---- the folds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("seed", range(4))
def test_fold_conv_bias_bn_against_float64(seed, dtype):
    """scale * conv(x, w16) + shift of the fold against float64 bn(conv(x, w16) + bias): the bias is in the shift with its sign."""
    conv = nn.Conv2d(48, 64, 3, padding=1)
    bn = nn.BatchNorm2d(64, eps=1e-3)
    randomise(nn.Sequential(conv, bn), seed).eval()
    assert conv.bias.abs().min() > 0 and conv.bias.abs().max() > 1.0
    fold = cn.fold_conv_bias_bn(conv, bn, dtype)
    assert isinstance(fold, bt.FoldedBevLayer) and fold.packed.dtype == dtype and fold.scale.dtype == fold.shift.dtype == torch.float32
    assert (fold.in_channels, fold.out_channels, fold.kernel, fold.stride, fold.mode) == (48, 64, 3, 1, "conv")
    w16 = bt.bev_unpack_weight(fold.packed, 48, 64, 3)
    assert torch.equal(w16, conv.weight.detach().to(dtype))                  # one rounding of the fp32 parameter
    x = torch.randn(2, 48, 5, 7, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    acc = F.conv2d(x, w16.double(), padding=1)
    ref = copy.deepcopy(bn).double()(acc + conv.bias.detach().double().view(1, -1, 1, 1))
    got = fold.scale.double().view(1, -1, 1, 1) * acc + fold.shift.double().view(1, -1, 1, 1)
    mag = fold.scale.double().abs().view(1, -1, 1, 1) * acc.abs() + fold.shift.double().abs().view(1, -1, 1, 1)
    assert ((got - ref).abs() <= 2.0 ** -21 * mag).all()
    s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t64 = bn.bias.double() + (conv.bias.double() - bn.running_mean.double()) * s64
    wrong = bn.bias.double() - (conv.bias.double() + bn.running_mean.double()) * s64          # the bias with the wrong sign
    assert ((fold.shift.double() - t64).abs() <= 2.0 ** -22 * (bn.bias.double().abs() + (conv.bias.double().abs() + bn.running_mean.double().abs()) * s64.abs())).all()
    assert (fold.shift.double() - wrong).abs().max() > 0.1
    assert torch.equal(fold.scale, s64.float())


def test_fold_conv_bias_bn_refuses_what_the_kernel_does_not_serve_and_leaves_layer_spec_alone():
    bn = nn.BatchNorm2d(64).eval()
    assert cn.bias_layer_spec(nn.Conv2d(32, 64, 3, padding=1), bn) == ("conv", 3, 1)
    assert bt.layer_spec(nn.Conv2d(32, 64, 3, padding=1), bn) is None                 # the trunk's own spec still refuses a bias
    for conv in (nn.Conv2d(32, 48, 3, padding=1), nn.Conv2d(8, 64, 3, padding=1), nn.Conv2d(32, 64, 5, padding=2), nn.Conv2d(32, 64, 3)):
        assert cn.bias_layer_spec(conv, nn.BatchNorm2d(conv.out_channels).eval()) is None
        with pytest.raises(RuntimeError, match="does not serve"):
            cn.fold_conv_bias_bn(conv, nn.BatchNorm2d(conv.out_channels).eval())
    assert cn.bias_layer_spec(nn.Conv2d(32, 64, 3, padding=1), nn.BatchNorm2d(64)) is None   # a BatchNorm in train mode
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        cn.fold_conv_bias_bn(nn.Conv2d(32, 64, 3, padding=1), bn, torch.float32)


def test_fold_caches_hit_and_miss_after_an_in_place_write():
    m = small_transform()
    conv, bn = m.depthnet[0], m.depthnet[1]
    a = cn.fold_conv_bias_bn(conv, bn, torch.float16)
    assert cn.fold_conv_bias_bn(conv, bn, torch.float16) is a
    b16 = cn.fold_conv_bias_bn(conv, bn, torch.bfloat16)
    assert b16 is not a and b16.packed.dtype == torch.bfloat16 and cn.fold_conv_bias_bn(conv, bn, torch.float16) is a
    with torch.no_grad():
        conv.bias.add_(1.0)
    b = cn.fold_conv_bias_bn(conv, bn, torch.float16)
    assert b is not a and not torch.equal(b.shift, a.shift) and torch.equal(b.scale, a.scale) and torch.equal(b.packed, a.packed)
    s = cn.fold_depth_stem(m.dtransform, torch.float16)
    assert cn.fold_depth_stem(m.dtransform, torch.float16) is s
    with torch.no_grad():
        m.dtransform[4].running_mean.mul_(2.0)
    s2 = cn.fold_depth_stem(m.dtransform, torch.float16)
    assert s2 is not s and not torch.equal(s2.shift2, s.shift2) and torch.equal(s2.shift3, s.shift3)
    h = cn.fold_depth_head(m.depthnet[6], m.D, m.C, torch.float16)
    assert cn.fold_depth_head(m.depthnet[6], m.D, m.C, torch.float16) is h
    with torch.no_grad():
        m.depthnet[6].weight.mul_(2.0)
    h2 = cn.fold_depth_head(m.depthnet[6], m.D, m.C, torch.float16)
    assert h2 is not h and torch.equal(h2.bias, h.bias) and not torch.equal(h2.packed, h.packed)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_stem_and_head_folds_name_the_kernels_operands(dtype):
    m = small_transform(seed=3)
    f = cn.fold_depth_stem(m.dtransform, dtype)
    c1, b1, c2, b2, c3, b3 = (m.dtransform[i] for i in (0, 1, 3, 4, 6, 7))
    s1 = b1.weight.double() / torch.sqrt(b1.running_var.double() + b1.eps)
    want_s1 = s1 * c1.weight.double().reshape(8)
    want_t1 = b1.bias.double() + (c1.bias.double() - b1.running_mean.double()) * s1
    assert torch.equal(f.scale1, want_s1.float()) and torch.equal(f.shift1, want_t1.float())
    # layer 1 through the fold in float64 is the torch layers' in float64
    d = torch.tensor([0.0, 1.5, 40.0], dtype=torch.float64).view(3, 1, 1, 1)
    ref = torch.relu(copy.deepcopy(b1).double()(copy.deepcopy(c1).double()(d))).reshape(3, 8)
    got = torch.relu(d.reshape(3, 1) * want_s1 + want_t1)
    assert (got - ref).abs().max() <= 1e-12 * (1 + ref.abs().max())
    assert f.packed2.numel() == 32 * 224 and f.packed3.numel() == 64 * 800 and f.packed2.dtype == f.packed3.dtype == dtype
    w2 = bt.bev_unpack_weight(f.packed2, 200, 32, 1).reshape(32, 5, 5, 8).permute(0, 3, 1, 2)       # k = 8 (5 ky + kx) + ci
    assert torch.equal(w2, c2.weight.detach().to(dtype))
    assert not bt.bev_unpack_weight(f.packed2, 224, 32, 1)[:, 200:].any()                            # the padding is zero
    assert torch.equal(bt.bev_unpack_weight(f.packed3, 32, 64, 5), c3.weight.detach().to(dtype))
    s3 = b3.weight.double() / torch.sqrt(b3.running_var.double() + b3.eps)
    assert torch.equal(f.scale3, s3.float())
    assert torch.equal(f.shift3, (b3.bias.double() + (c3.bias.double() - b3.running_mean.double()) * s3).float())
    assert [t.numel() for t in (f.scale1, f.shift1, f.scale2, f.shift2, f.scale3, f.shift3)] == [8, 8, 32, 32, 64, 64]
    h = cn.fold_depth_head(m.depthnet[6], m.D, m.C, dtype)
    assert (h.in_channels, h.D, h.C) == (32, 5, 4) and h.packed.numel() == 16 * 32 and torch.equal(h.bias, m.depthnet[6].bias.detach())
    w = bt.bev_unpack_weight(h.packed, 32, 16, 1)
    assert torch.equal(w[:9], m.depthnet[6].weight.detach().to(dtype)) and not w[9:].any()
    with pytest.raises(RuntimeError, match="depth head takes"):
        cn.fold_depth_head(m.depthnet[6], 6, 4, dtype)


def test_the_functional_wrappers_refuse_host_tensors():
    m = small_transform()
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cn.depth_stem_forward(torch.zeros(2, 16, 24), cn.fold_depth_stem(m.dtransform))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cn.depth_head_forward(torch.zeros(2, 32, 2, 3, dtype=torch.float16), cn.fold_depth_head(m.depthnet[6], 5, 4))


# ---- which calls take the fused route ----------------------------------------------------------------------------------------------
def test_the_default_transforms_are_served_and_the_changed_ones_are_not():
    for kind in ("depth", "lss"):
        assert small_transform(kind).cam_nets_served()
        assert not small_transform(kind, in_channels=48).cam_nets_served()                # in_channels 48: no multiple of 32
        assert not small_transform(kind).train().cam_nets_served() or kind == "lss"       # train-mode BatchNorms (the stem has them)
    m = small_transform()
    m.dtransform[3] = nn.Conv2d(8, 32, 3, stride=4, padding=1)                            # one kernel size changed
    assert not m.eval().cam_nets_served()
    m = small_transform()
    m.depthnet[1].track_running_stats, m.depthnet[1].running_mean, m.depthnet[1].running_var = False, None, None
    assert not m.cam_nets_served()                                                        # a BatchNorm without running statistics
    m = small_transform()
    m.depthnet[3] = nn.Conv2d(32, 32, 3, padding=1, dilation=1, groups=2)
    assert not m.cam_nets_served()
    assert not BaseTransform(in_channels=32, **SMALL).cam_nets_served()


NOT_FUSABLE = [(k, h) for k in ("depth", "lss") for h in ("dtype_none", "train", "host", "grad", "in_channels_48")] + [("depth", "kernel_size")]


def unfusable_case(kind, how):
    """A transform and inputs that differ from a fusable call in ONE respect -> (module, x, d or None, grad mode)."""
    m = small_transform(kind, in_channels=48 if how == "in_channels_48" else 32)
    m.cam_nets_dtype = None if how == "dtype_none" else torch.float16
    x, d = small_inputs(48 if how == "in_channels_48" else 32)
    if how == "train":
        m.train()
    if how == "kernel_size":
        m.dtransform[3] = nn.Conv2d(8, 32, 3, stride=4, padding=1)
        m.eval()
    if how == "grad":
        x.requires_grad_(True)
    return m, x, (d if kind == "depth" else None), how == "grad"


@pytest.mark.parametrize("kind, how", NOT_FUSABLE)
def test_cam_nets_fusable_is_false(kind, how):
    """Host tensors here; tests/test_gpu_cam_nets.py repeats every case with the module and the tensors on the device."""
    m, x, d, grad = unfusable_case(kind, how)
    served = how != "in_channels_48" and how != "kernel_size" and not (how == "train" and kind == "depth")
    assert m.cam_nets_served() == served
    with torch.enable_grad() if grad else torch.no_grad():
        assert m.cam_nets_fusable(x, d) is False


# ---- the default is unchanged ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factored", [True, False])
def test_with_cam_nets_dtype_none_get_cam_feats_is_the_modules_own_layers(factored):
    x, d = small_inputs()
    with torch.no_grad():
        m = small_transform("depth")
        m.fused_cam_feats = factored
        got = m.get_cam_feats(x, d)
        z = m.depthnet(torch.cat([m.dtransform(d.view(2, 1, 16, 24)), x.view(2, 32, 2, 3)], dim=1))
        depth, ctx = z[:, :5].softmax(dim=1), z[:, 5:9]
        lss = small_transform("lss")
        lss.fused_cam_feats = factored
        got_l = lss.get_cam_feats(x)
        zl = lss.depthnet(x.view(2, 32, 2, 3))
        depth_l, ctx_l = zl[:, :5].softmax(dim=1), zl[:, 5:9]
    for g, dp, cx in ((got, depth, ctx), (got_l, depth_l, ctx_l)):
        if factored:
            assert isinstance(g, FactoredCamFeats) and torch.equal(g.depth, dp.view(1, 2, 5, 2, 3)) and torch.equal(g.ctx, cx.view(1, 2, 4, 2, 3))
        else:
            want = (dp.unsqueeze(1) * cx.unsqueeze(2)).view(1, 2, 4, 5, 2, 3).permute(0, 1, 3, 4, 5, 2)
            assert torch.equal(g, want)


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def _addr(on):
    return ctypes.c_void_p(on * 4096 or None)


def _head(lib, cin=64, D=5, C=4, H=3, W=5, batch=2, dtype=0, x=1, packed=1, bias=1, depth=1, ctx=1, x_elems=None, packed_elems=None,
          depth_elems=None, ctx_elems=None):
    """bevamd_cam_depth_head_forward with made-up non-null addresses: every case here is refused before any GPU work."""
    pix = batch * H * W
    return lib.bevamd_cam_depth_head_forward(
        _addr(x), pix * cin if x_elems is None else x_elems, batch, H, W, cin, D, C, dtype, _addr(packed),
        -(-(D + C) // 16) * 16 * cin if packed_elems is None else packed_elems, _addr(bias), _addr(depth),
        pix * D if depth_elems is None else depth_elems, _addr(ctx), pix * C if ctx_elems is None else ctx_elems, None)


def _stem(lib, H=9, W=13, batch=2, dtype=0, depth=1, s1=1, packed2=1, s2=1, packed3=1, s3=1, scratch=1, out=1, depth_elems=None,
          packed2_elems=32 * 224, packed3_elems=64 * 800, scratch_elems=None, out_elems=None):
    oh2, ow2 = (H - 1) // 4 + 1, (W - 1) // 4 + 1
    oh3, ow3 = (oh2 - 1) // 2 + 1, (ow2 - 1) // 2 + 1
    return lib.bevamd_cam_depth_stem_forward(
        _addr(depth), batch * H * W if depth_elems is None else depth_elems, batch, H, W, dtype, _addr(s1), _addr(s1), _addr(packed2),
        packed2_elems, _addr(s2), _addr(s2), _addr(packed3), packed3_elems, _addr(s3), _addr(s3), _addr(scratch),
        batch * oh2 * ow2 * 32 if scratch_elems is None else scratch_elems, _addr(out),
        batch * oh3 * ow3 * 64 if out_elems is None else out_elems, None)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(D=0), 4, "depth_bins 0"),
    (dict(D=129), 4, "depth_bins 129"),
    (dict(C=6), 4, "context_channels 6"),
    (dict(C=0), 4, "context_channels 0"),
    (dict(C=132), 4, "context_channels 132"),
    (dict(cin=48), 4, "in_channels 48"),
    (dict(cin=544), 4, "in_channels 544"),
    (dict(dtype=2), 1, "dtype 2"),
    (dict(H=0), 1, "bad sizes"),
    (dict(batch=-1), 1, "batch"),
    (dict(x=0), 1, "is null"),
    (dict(depth=0), 1, "is null"),
    (dict(ctx=0), 1, "is null"),
    (dict(packed=0), 1, "packed is null"),
    (dict(bias=0), 1, "bias is null"),
    (dict(x_elems=2 * 15 * 64 - 1), 1, "x holds"),
    (dict(packed_elems=9 * 64), 1, "packed holds"),
    (dict(depth_elems=2 * 15 * 5 - 1), 1, "depth holds"),
    (dict(ctx_elems=2 * 15 * 4 - 1), 1, "context holds"),
])
def test_head_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _head(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(dtype=2), 1, "dtype 2"),
    (dict(H=0), 1, "bad sizes"),
    (dict(batch=65536), 1, "batch"),
    (dict(depth=0), 1, "is null"),
    (dict(scratch=0), 1, "is null"),
    (dict(out=0), 1, "is null"),
    (dict(packed2=0), 1, "packed weights are null"),
    (dict(packed3=0), 1, "packed weights are null"),
    (dict(s1=0), 1, "scale or shift"),
    (dict(s3=0), 1, "scale or shift"),
    (dict(depth_elems=2 * 9 * 13 - 1), 1, "depth holds"),
    (dict(packed2_elems=32 * 200), 1, "packed weights hold"),
    (dict(packed3_elems=64 * 800 - 8), 1, "packed weights hold"),
    (dict(scratch_elems=2 * 3 * 4 * 32 - 1), 1, "scratch holds"),
    (dict(out_elems=2 * 2 * 2 * 64 - 1), 1, "out holds"),
])
def test_stem_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _stem(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_an_empty_batch_is_nothing_to_do():
    lib = _capi.load()
    assert _head(lib, batch=0, x=0, depth=0, ctx=0) == 0
    assert _stem(lib, batch=0, depth=0, scratch=0, out=0) == 0


def test_binding_table_equals_the_header():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_cam_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_cam_depth_head_forward", "bevamd_cam_depth_stem_forward"]
    assert sorted(n for n in _capi._EXT_SIGNATURES if n.startswith("bevamd_cam_")) == sorted(protos)
    for name, args in protos.items():
        res, argtypes = _capi._EXT_SIGNATURES[name]
        want = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_int for a in args.split(",")]
        assert res is ctypes.c_int and argtypes == want, name
        assert "size_t" not in args and ctypes.c_size_t not in argtypes
        assert name in _capi.ext_exported_names()


# ---- the code object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(resources.OBJ, "cam_nets.o")) or not all(os.path.exists(t) for t in resources.TOOLS),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_the_kernels_use_no_scratch_and_spill_nothing():
    kernels = {n: v for n, v in resources._kernels().items() if v["obj"] == "cam_nets"}
    names = sorted([f"void bevamd::cam_stem12_kernel<{b}>" for b in ("false", "true")] +
                   [f"void bevamd::cam_stem3_kernel<{b}>" for b in ("false", "true")] +
                   [f"void bevamd::cam_head_kernel<{b}, {mt}>" for b in ("false", "true") for mt in (4, 8, 16)])
    assert sorted(kernels) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "cam_nets.o"))
    for name in names:
        got = kernels[name]
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= (512 if "cam_head_kernel" in name else 256), (name, got)     # stem: two workgroups of four waves per CU
        want = 33 * 65 * 16 if "stem12" in name else 19 * 35 * 80 if "stem3" in name else 0
        assert lds[name] == want and 2 * lds[name] <= 160 * 1024, (name, lds[name], want)
