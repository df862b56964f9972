"""The camera necks (cam_neck.py, csrc/ext/cam_neck.hip) without a GPU: registries and config blocks, state-dict names, the torch
path against a literal restatement of the reference, the fold without BatchNorm, the host mirror of the resampling against
F.interpolate, the entry point's refusals, the binding table and the kernels' resources."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import cam_neck_reference as ref
import test_kernel_resources as resources
from bevfusion_amd import _capi, bev_trunk as bt, cam_neck as cnk, heads, registry
from test_centerhead_module import _lds_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the neck blocks of the reference's configs, written out (configs/nuscenes/.../default.yaml and the leaves that override them)
GEN_SWIN = dict(type="GeneralizedLSSFPN", in_channels=[192, 384, 768], out_channels=256, start_level=0, num_outs=3,
                norm_cfg=dict(type="BN2d", requires_grad=True), act_cfg=dict(type="ReLU", inplace=True),
                upsample_cfg=dict(mode="bilinear", align_corners=True))
GEN_RESNET = dict(GEN_SWIN, in_channels=[512, 1024, 2048])
LSS_640 = dict(type="LSSFPN", in_indices=[-1, 0], in_channels=[640, 160], out_channels=256, scale_factor=2)
LSS_512 = dict(LSS_640, in_channels=[512, 128])

# source map -> output map: the pairs tests/test_gpu_cam_neck.py runs on the device
PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((2, 3), (1, 7)), ((3, 5), (5, 9)), ((2, 3), (5, 9)), ((4, 11), (8, 22)), ((8, 16), (9, 17)),
         ((9, 17), (17, 33)), ((5, 9), (5, 9)), ((9, 17), (4, 7))]
EXACT_PAIRS = [((1, 1), (3, 5)), ((3, 5), (5, 9)), ((2, 3), (5, 9)), ((8, 16), (9, 17)), ((9, 17), (17, 33)), ((5, 9), (5, 9))]
INEXACT_PAIRS = [((2, 3), (1, 7)), ((4, 11), (8, 22)), ((9, 17), (4, 7))]


# ---- registries and config ---------------------------------------------------------------------------------------------------------
def test_the_modules_are_registered_and_reexported():
    assert registry.NECKS.get("GeneralizedLSSFPN") is cnk.GeneralizedLSSFPN and registry.NECKS.get("LSSFPN") is cnk.LSSFPN
    for name in ("GeneralizedLSSFPN", "LSSFPN", "cam_neck_conv_forward", "fold_conv_bias", "fold_neck_layer", "neck_layer_spec"):
        assert getattr(heads, name) is getattr(cnk, name) and name in heads.__all__
    assert cnk.ConvModule is heads.ConvModule          # the one ConvModule of the package, not a second copy


@pytest.mark.parametrize("cfg", [GEN_SWIN, GEN_RESNET], ids=["swin", "resnet"])
def test_the_generalized_lss_fpn_blocks_build(cfg):
    before = copy.deepcopy(cfg)
    m = registry.NECKS.build(cfg)
    assert cfg == before and type(m) is cnk.GeneralizedLSSFPN
    c = cfg["in_channels"]
    assert len(m.lateral_convs) == len(m.fpn_convs) == 2 and m.backbone_end_level == 2 and m.num_outs == 3
    assert [l.conv.in_channels for l in m.lateral_convs] == [c[0] + 256, c[1] + c[2]]
    for l, f in zip(m.lateral_convs, m.fpn_convs):
        assert l.conv.kernel_size == (1, 1) and l.conv.bias is None and type(l.bn) is nn.BatchNorm2d and type(l.activate) is nn.ReLU
        assert f.conv.kernel_size == (3, 3) and f.conv.padding == (1, 1) and f.conv.bias is None and f.bn.eps == 1e-5
        assert l.conv.out_channels == f.conv.in_channels == f.conv.out_channels == 256
        assert l.activate.inplace is False and f.activate.inplace is False
    assert m.upsample_cfg == dict(mode="bilinear", align_corners=True)


@pytest.mark.parametrize("cfg", [LSS_640, LSS_512], ids=["640+160", "512+128"])
def test_the_lss_fpn_blocks_build(cfg):
    m = registry.NECKS.build(cfg)
    assert type(m) is cnk.LSSFPN and m.fuse[0].in_channels == sum(cfg["in_channels"]) and m.fuse[0].kernel_size == (1, 1)
    assert m.fuse[3].kernel_size == (3, 3) and m.fuse[3].padding == (1, 1) and m.fuse[0].bias is None and m.fuse[3].bias is None
    assert type(m.upsample[0]) is nn.Upsample and m.upsample[0].scale_factor == 2 and m.upsample[0].mode == "bilinear"
    assert m.upsample[0].align_corners is True and m.upsample[1].kernel_size == (3, 3)
    assert not hasattr(cnk.LSSFPN([-1, 0], [64, 32], 64), "upsample")            # scale_factor 1: no third stage


def test_the_constructor_keeps_the_references_asserts_and_defaults():
    with pytest.raises(AssertionError):
        cnk.GeneralizedLSSFPN((32, 64), 32, 2)                                    # in_channels must be a list
    with pytest.raises(AssertionError):
        cnk.GeneralizedLSSFPN([32, 64, 128], 32, 3, end_level=2)                  # num_outs == end_level - start_level
    m = cnk.GeneralizedLSSFPN([32, 64, 128], 32, 2, end_level=2)
    assert m.backbone_end_level == 2 and len(m.lateral_convs) == 2
    m = cnk.GeneralizedLSSFPN([32, 64], 32, 1, no_norm_on_lateral=True)
    assert m.lateral_convs[0].conv.bias is not None and not m.lateral_convs[0].with_norm and m.fpn_convs[0].with_norm
    assert m.upsample_cfg == dict(mode="bilinear", align_corners=True) and m.start_level == 0 and m.end_level == -1


# ---- state dict --------------------------------------------------------------------------------------------------------------------
def bn_keys(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
            (prefix + ".num_batches_tracked", ())]


def reference_keys(which):
    """Written out from the reference's module definitions."""
    if which == "gen":
        keys = []
        for i, cin in enumerate([192 + 256, 384 + 768]):
            keys += [(f"lateral_convs.{i}.conv.weight", (256, cin, 1, 1))] + bn_keys(f"lateral_convs.{i}.bn", 256)
            keys += [(f"fpn_convs.{i}.conv.weight", (256, 256, 3, 3))] + bn_keys(f"fpn_convs.{i}.bn", 256)
        return keys
    return [("fuse.0.weight", (256, 800, 1, 1))] + bn_keys("fuse.1", 256) + [("fuse.3.weight", (256, 256, 3, 3))] + bn_keys("fuse.4", 256) + \
        [("upsample.1.weight", (256, 256, 3, 3))] + bn_keys("upsample.2", 256)


@pytest.mark.parametrize("which, cfg", [("gen", GEN_SWIN), ("lss", LSS_640)])
def test_state_dict_names_and_shapes_equal_the_reference(which, cfg):
    module = registry.NECKS.build(cfg)
    got = sorted((k, tuple(v.shape)) for k, v in module.state_dict().items())
    assert got == sorted(reference_keys(which))
    g = torch.Generator().manual_seed(3)
    state = {k: (torch.rand(s, generator=g) + 0.5) if s else torch.tensor(7) for k, s in reference_keys(which)}
    other = registry.NECKS.build(cfg)
    assert other.load_state_dict(state, strict=True).missing_keys == []
    assert all(torch.equal(v, state[k]) for k, v in other.state_dict().items())
    if which == "lss":
        assert sorted(k for k in cnk.LSSFPN([-1, 0], [64, 32], 64).state_dict() if k.endswith("weight")) == \
            ["fuse.0.weight", "fuse.1.weight", "fuse.3.weight", "fuse.4.weight"]


# ---- the torch path ----------------------------------------------------------------------------------------------------------------
def randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                K = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / K) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.8 + 0.4 * torch.rand(n, generator=g))
                m.bias.copy_(0.3 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=g))
    return module


def small_gen(seed=0, **kw):
    return randomise(cnk.GeneralizedLSSFPN([32, 64, 128], 64, 3, **kw), seed)


def small_lss(seed=0, scale_factor=2):
    return randomise(cnk.LSSFPN([-1, 0], [64, 32], 64, scale_factor=scale_factor), seed)


def gen_inputs(seed=1, B=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, h, w, generator=g) for c, (h, w) in zip([32, 64, 128], [(8, 22), (4, 11), (2, 6)])]


def lss_inputs(seed=2, B=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 32, 6, 10, generator=g), torch.randn(B, 64, 3, 5, generator=g)]


def literal_gen(m, inputs):
    """generalized_lss.py:84-103 restated with F.interpolate, torch.cat and plain Sequentials over the same parameters."""
    lat = list(inputs)
    for i in range(len(lat) - 2, -1, -1):
        x = F.interpolate(lat[i + 1], size=lat[i].shape[2:], mode="bilinear", align_corners=True)
        x = torch.cat([lat[i], x], dim=1)
        l, f = m.lateral_convs[i], m.fpn_convs[i]
        x = nn.Sequential(*([l.conv] + ([l.bn] if l.with_norm else []) + [nn.ReLU()]))(x)
        lat[i] = nn.Sequential(f.conv, f.bn, nn.ReLU())(x)
    return tuple(lat[:-1])


def literal_lss(m, x):
    x1, x2 = x[m.in_indices[0]], x[m.in_indices[1]]
    y = torch.cat([F.interpolate(x1, size=x2.shape[-2:], mode="bilinear", align_corners=True), x2], dim=1)
    y = nn.Sequential(*list(m.fuse))(y)
    if m.scale_factor > 1:
        y = nn.Sequential(m.upsample[1], m.upsample[2], nn.ReLU())(
            F.interpolate(y, scale_factor=m.scale_factor, mode="bilinear", align_corners=True))
    return y


@pytest.mark.parametrize("no_norm", [False, True])
def test_generalized_lss_fpn_on_the_cpu_bit_equals_the_literal_restatement(no_norm):
    m = small_gen(no_norm_on_lateral=no_norm).eval()
    xs = gen_inputs()
    assert not m.fusable(xs)
    with torch.no_grad():
        got, want = m(xs), literal_gen(m, xs)
    assert isinstance(got, tuple) and len(got) == len(xs) - 1
    assert [tuple(t.shape) for t in got] == [(2, 64, 8, 22), (2, 64, 4, 11)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("scale_factor", [1, 2])
def test_lss_fpn_on_the_cpu_bit_equals_the_literal_restatement(scale_factor):
    m = small_lss(scale_factor=scale_factor).eval()
    xs = lss_inputs()
    assert not m.fusable(xs)
    with torch.no_grad():
        got, want = m(xs), literal_lss(m, xs)
    assert tuple(got.shape) == (2, 64, 6 * scale_factor, 10 * scale_factor) and torch.equal(got, want)
    with pytest.raises(AssertionError):
        m([xs[1], xs[0]])                                                  # the channel asserts of the reference


def test_train_mode_updates_the_running_statistics_and_gradients_flow():
    for m, xs in ((small_gen(), gen_inputs()), (small_lss(), lss_inputs())):
        xs = [x.requires_grad_(True) for x in xs]
        bns = [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
        before = [b.running_mean.clone() for b in bns]
        out = m(xs)
        sum(o.sum() for o in (out if isinstance(out, tuple) else (out,))).backward()
        assert all(int(b.num_batches_tracked) == 1 for b in bns)
        assert all(not torch.equal(b.running_mean, old) for b, old in zip(bns, before))
        assert all(x.grad is not None and x.grad.abs().sum() > 0 for x in xs)
        assert all(p.grad is not None for p in m.parameters())


def test_host_tensors_and_fp32_take_the_torch_layers():
    m, l = small_gen().eval(), small_lss().eval()
    assert m.use_fused in (True, False) and l.use_fused in (True, False)
    m.use_fused = l.use_fused = True
    with torch.no_grad():
        assert not m.fusable(gen_inputs()) and not l.fusable(lss_inputs())
        assert not m.half().fusable([x.half() for x in gen_inputs()])          # 16-bit, but host tensors
    conv, bn = nn.Conv2d(48, 64, 1, bias=False).half().eval(), nn.BatchNorm2d(64).half().eval()
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cnk.cam_neck_conv_forward([torch.zeros(1, 48, 4, 4, dtype=torch.float16)], bt.fold_bev_layer(conv, bn))


# ---- the folds and the specs -------------------------------------------------------------------------------------------------------
def test_neck_layer_spec_names_what_the_kernel_serves():
    bn = nn.BatchNorm2d(64).eval()
    assert cnk.neck_layer_spec(nn.Conv2d(32, 64, 1, bias=False), bn) == 1 and cnk.neck_layer_spec(nn.Conv2d(32, 64, 1)) == 1
    assert cnk.neck_layer_spec(nn.Conv2d(32, 64, 3, padding=1), bn) == 3
    for conv in (nn.Conv2d(32, 48, 1), nn.Conv2d(8, 64, 1), nn.Conv2d(32, 64, 3), nn.Conv2d(32, 64, 3, padding=1, stride=2),
                 nn.Conv2d(32, 64, 5, padding=2), nn.Conv2d(32, 64, 3, padding=1, groups=2), nn.Conv2d(32, 64, 3, padding=2, dilation=2)):
        assert cnk.neck_layer_spec(conv) is None, conv
    assert cnk.neck_layer_spec(nn.Conv2d(32, 64, 1, bias=False), nn.BatchNorm2d(64)) is None          # a BatchNorm in train mode


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_fold_conv_bias_is_ones_and_the_bias_and_is_cached(dtype):
    conv = randomise(nn.Conv2d(48, 64, 1), 5).to(dtype)
    f = cnk.fold_conv_bias(conv)
    assert isinstance(f, bt.FoldedBevLayer) and (f.in_channels, f.out_channels, f.kernel, f.stride, f.mode) == (48, 64, 1, 1, "conv")
    assert f.scale.dtype == f.shift.dtype == torch.float32 and f.packed.dtype == dtype
    assert torch.equal(f.scale, torch.ones(64)) and torch.equal(f.shift, conv.bias.detach().float()) and f.shift.abs().max() > 0
    assert torch.equal(bt.bev_unpack_weight(f.packed, 48, 64, 1), conv.weight.detach())
    assert cnk.fold_conv_bias(conv) is f and cnk.fold_neck_layer(conv) is f
    with torch.no_grad():
        conv.bias.add_(1.0)
    g = cnk.fold_conv_bias(conv)
    assert g is not f and torch.equal(g.shift, conv.bias.detach().float()) and torch.equal(g.packed, f.packed)
    nobias = cnk.fold_conv_bias(nn.Conv2d(32, 32, 3, padding=1, bias=False).to(dtype))
    assert not nobias.shift.any() and nobias.kernel == 3
    with pytest.raises(RuntimeError, match="does not serve"):
        cnk.fold_conv_bias(nn.Conv2d(32, 48, 1).to(dtype))
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        cnk.fold_conv_bias(nn.Conv2d(32, 64, 1))


def test_fold_neck_layer_picks_the_fold_of_the_layer():
    conv, bn = nn.Conv2d(32, 64, 1, bias=False).half().eval(), randomise(nn.BatchNorm2d(64), 1).half().eval()
    assert cnk.fold_neck_layer(conv, bn) is bt.fold_bev_layer(conv, bn)
    biased = randomise(nn.Conv2d(32, 64, 3, padding=1), 2).half()
    f = cnk.fold_neck_layer(biased, bn)
    s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    assert torch.equal(f.shift, (bn.bias.double() + (biased.bias.double() - bn.running_mean.double()) * s64).float())


def test_upsample_size_is_what_nn_upsample_yields():
    for size, s in [((3, 5), 2), ((90, 90), 2), ((3, 5), 1.5), ((7, 2), 2.5), ((1, 1), 3)]:
        want = tuple(nn.Upsample(scale_factor=s, mode="bilinear", align_corners=True)(torch.zeros(1, 1, *size)).shape[2:])
        assert cnk.upsample_size(size, s) == want


# ---- the host mirror of the resampling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_the_mirror_agrees_with_interpolate_in_float32(pair):
    """The mirror and torch's float32 kernel compute the same real interpolant with a handful of float32 roundings each."""
    (h, w), out = pair
    worst = 0.0
    for seed in range(4):
        x = torch.randn(2, 5, h, w, generator=torch.Generator().manual_seed(seed))
        got = torch.from_numpy(ref.resample32(x.numpy(), out))
        want = F.interpolate(x, size=out, mode="bilinear", align_corners=True)
        assert got.dtype == torch.float32 and got.shape == want.shape
        err = (got.double() - want.double()).abs().max().item()
        worst = max(worst, err / x.abs().max().item())
        assert err <= 4 * 2.0 ** -23 * x.abs().max().item(), (pair, err)
    print(f"{pair}: worst |mirror - F.interpolate| / max|x| = {worst:.3e}")


def _bilinear64(x, out):
    """The exact interpolant of the mirror's own fp32 indices and weights, evaluated in float64."""
    y0, y1, ly, hy = (torch.from_numpy(np.asarray(v)) for v in ref.axis_table(x.shape[2], out[0]))
    x0, x1, lx, hx = (torch.from_numpy(np.asarray(v)) for v in ref.axis_table(x.shape[3], out[1]))
    x = x.double()
    ly, hy, lx, hx = ly.double()[:, None], hy.double()[:, None], lx.double(), hx.double()
    y0, y1, x0, x1 = y0.long(), y1.long(), x0.long(), x1.long()
    return hy * (hx * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]) + ly * (hx * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1])


def _integer_source(h, w, seed=0):
    return 16.0 * torch.randint(-2, 3, (2, 6, h, w), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("pair", EXACT_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_the_resampling_of_small_integers_is_exact_on_the_dyadic_pairs(pair):
    """What the exact GPU cases rest on: on these pairs the fp32 resampling of 16 * {-2 .. 2} has no rounding at all and its values
    are representable in both storage types."""
    (h, w), out = pair
    for seed in range(3):
        x = _integer_source(h, w, seed)
        v = torch.from_numpy(ref.resample32(x.numpy(), out))
        assert torch.equal(v.double(), _bilinear64(x, out))
        for dtype in (torch.float16, torch.bfloat16):
            assert torch.equal(v.to(dtype).float(), v)
            assert torch.equal(ref.staged(x.to(dtype), out).float(), v)


@pytest.mark.parametrize("pair", INEXACT_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_the_other_pairs_are_not_exact_and_stay_with_the_float64_test(pair):
    (h, w), out = pair
    x = _integer_source(h, w)
    v = torch.from_numpy(ref.resample32(x.numpy(), out))
    assert not (torch.equal(v.double(), _bilinear64(x, out)) and torch.equal(v.to(torch.bfloat16).float(), v)
                and torch.equal(v.to(torch.float16).float(), v))


def test_the_mirror_copies_a_source_of_the_output_map_and_clamps_at_the_edges():
    x = torch.randn(1, 3, 5, 9).half()
    assert ref.staged(x, (5, 9)) is not None and torch.equal(ref.staged(x, (5, 9)), x)
    for n, N in [(1, 1), (1, 5), (3, 1), (4, 8), (11, 22), (17, 7), (768, 4096)]:
        i0, i1, l, h = ref.axis_table(n, N)
        assert i0.min() >= 0 and i1.max() <= n - 1 and ((i1 == i0) | (i1 == i0 + 1)).all() and (l >= 0).all() and (l < 1).all()
        assert i0[0] == 0 and l[0] == 0


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def _call(lib, c0=16, c1=32, cout=64, kernel=1, hw0=(5, 7), hw1=(3, 4), out=(5, 7), batch=2, src=1, src1=1, packed=1, dst=1, scale=1,
          layout0=0, layout1=1, dst_layout=0, dtype=0, dst_c=None, dst_off=0, packed_elems=None, dst_elems=None, relu=1, align=4096):
    """bevamd_neck_conv_forward with made-up non-null addresses: every case here is refused before any GPU work."""
    dst_c = cout if dst_c is None else dst_c
    if packed_elems is None:
        packed_elems = cout * (-(-(c0 + c1) // 32)) * kernel * kernel * 32
    if dst_elems is None:
        dst_elems = batch * dst_c * out[0] * out[1]
    addr = lambda on, a=4096: ctypes.c_void_p(on * a or None)   # noqa: E731
    return lib.bevamd_neck_conv_forward(addr(src, align), c0, hw0[0], hw0[1], layout0, addr(src1 if c1 else 0, align), c1, hw1[0], hw1[1],
                                        layout1, dtype, batch, out[0], out[1], cout, kernel, addr(packed), packed_elems, addr(scale),
                                        addr(scale), relu, addr(dst, align), dst_c, dst_off, dst_layout, dst_elems, None)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(kernel=5), 4, "kernel 5"),
    (dict(kernel=2), 4, "kernel 2"),
    (dict(c0=8), 4, "multiples of 16"),
    (dict(c0=0, c1=0), 4, "multiples of 16"),
    (dict(c1=24), 4, "multiples of 16"),
    (dict(cout=48), 4, "multiple of 32"),
    (dict(dst_layout=1, dst_c=66), 4, "multiples of 4"),
    (dict(dst_layout=1, dst_c=128, dst_off=2), 4, "multiples of 4"),
    (dict(hw0=(0, 7)), 1, "bad sizes"),
    (dict(hw1=(3, 0)), 1, "bad sizes"),
    (dict(out=(0, 7)), 1, "bad sizes"),
    (dict(batch=65536), 1, "batch"),
    (dict(batch=-1), 1, "batch"),
    (dict(dtype=2), 1, "dtype"),
    (dict(layout0=3), 1, "layouts"),
    (dict(layout1=2), 1, "layouts"),
    (dict(dst_layout=-1), 1, "layouts"),
    (dict(dst_c=96, dst_off=64), 1, "does not fit"),
    (dict(packed_elems=7), 1, "packed holds 7"),
    (dict(dst_elems=5), 1, "dst holds 5"),
    (dict(packed=0), 1, "packed is null"),
    (dict(scale=0), 1, "scale or shift"),
    (dict(src=0), 1, "is null"),
    (dict(src1=0), 1, "is null"),
    (dict(dst=0), 1, "is null"),
    (dict(align=8), 1, "NHWC source is not 16-byte aligned"),
    (dict(align=4, layout1=0, dst_layout=1), 1, "NHWC dst is not 8-byte aligned"),
])
def test_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _call(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_an_empty_batch_is_nothing_to_do():
    assert _call(_capi.load(), batch=0, src=0, src1=0, dst=0) == 0
    assert _call(_capi.load(), batch=0, src=0, src1=0, dst=0, kernel=3, c1=0, hw0=(2, 3), out=(9, 4)) == 0


def test_binding_table_equals_the_header():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_neck_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_neck_conv_forward"]
    assert sorted(n for n in _capi._EXT_SIGNATURES if n.startswith("bevamd_neck_")) == sorted(protos)
    args = protos["bevamd_neck_conv_forward"].split(",")
    res, argtypes = _capi._EXT_SIGNATURES["bevamd_neck_conv_forward"]
    want = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_int for a in args]
    assert res is ctypes.c_int and argtypes == want and len(args) == 27
    assert "size_t" not in protos["bevamd_neck_conv_forward"] and ctypes.c_size_t not in argtypes
    assert "bevamd_neck_conv_forward" in _capi.ext_exported_names()


# ---- the code object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(resources.OBJ, "cam_neck.o")) or not all(os.path.exists(t) for t in resources.TOOLS),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_the_kernels_use_no_scratch_spill_nothing_and_fit_two_workgroups():
    kernels = {n: v for n, v in resources._kernels().items() if v["obj"] == "cam_neck"}
    names = sorted(f"void bevamd::cam_neck_conv_kernel<{b}, {mt}, {ks}, {rs}>" for b in ("false", "true") for mt in (1, 2, 4)
                   for ks in (1, 3) for rs in ("false", "true"))
    assert sorted(kernels) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "cam_neck.o"))
    for name in names:
        got = kernels[name]
        ks = int(name.split(",")[2])
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= 256, (name, got)                          # two workgroups of four waves per compute unit
        tile = (7 + ks) * (15 + ks) * 80                                # haloed tile x 80-byte pixels
        tables = 2 * 3 * 4 * ((7 + ks) + (15 + ks)) if name.endswith("true>") else 0      # per source: y0, y1, ly and x0, x1, lx
        assert lds[name] == tile + tables and 2 * lds[name] <= 160 * 1024, (name, lds[name], tile + tables)
