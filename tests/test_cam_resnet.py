"""The camera ResNet (bevfusion_amd/cam_resnet.py) without a GPU: registry and configs, torchvision's state-dict names, the torch path
against a plainly written chain, mmdet's `train()` behaviour, `bottleneck_spec` / `stem_spec`, the folds and the stem's packed
weight order, both entry points' refusals, the header against the binding table and the kernels' resources."""
import copy
import ctypes
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import test_kernel_resources as resources
from bevfusion_amd import _capi, bev_resnet as br, bev_trunk as bt, cam_resnet as cr, heads, registry
from bevfusion_amd.config import load_config
from test_centerhead_module import REF_CONFIGS, _lds_bytes, needs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORDED = json.load(open(os.path.join(HERE, "golden", "cam_resnet_configs.json")))
LEAVES = ["nuscenes/det/centerhead/lssfpn/camera/256x704/resnet/default.yaml",
          "nuscenes/det/centerhead/lssfpn/camera+radar/resnet50/default.yaml"]
FAMILY = LEAVES + ["nuscenes/det/centerhead/lssfpn/camera/256x704/resnet/bevdepth.yaml",
                   "nuscenes/det/centerhead/lssfpn/camera+radar/resnet50/dlss.yaml"]
SMALL = dict(depth=50, base_channels=32, stem_channels=64, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1))


# ---- registry and config -----------------------------------------------------------------------------------------------------------
def test_the_module_is_registered_and_reexported():
    assert registry.BACKBONES.get("ResNet") is cr.ResNet
    assert sorted(cr.__all__) == sorted(["ResNet", "Bottleneck", "FoldedBottleneckTail", "FoldedStem", "bottleneck_spec", "fold_bottleneck",
                                         "bottleneck_tail_forward", "stem_spec", "fold_stem", "stem_forward", "stem_pack_weight",
                                         "stem_unpack_weight"])
    assert all(getattr(heads, n) is getattr(cr, n) and n in heads.__all__ for n in cr.__all__)


@pytest.mark.parametrize("leaf", LEAVES)
def test_the_recorded_backbone_block_builds_and_leaves_its_dict_alone(leaf):
    cfg = RECORDED[leaf]["backbone"]
    before = copy.deepcopy(cfg)
    net = registry.BACKBONES.build(cfg)
    assert cfg == before and type(net) is cr.ResNet and net.depth == 50
    blocks = net._all_blocks()
    assert len(blocks) == 16 and all(type(b) is cr.Bottleneck for b in blocks) and [len(getattr(net, f"layer{i}")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert net.init_cfg == dict(type="Pretrained", checkpoint="torchvision://resnet50") and net.norm_eval is False
    assert net.init_weights() is None                                     # recorded, nothing fetched, nothing written
    x = torch.zeros(1, 3, 64, 96)
    with torch.no_grad():
        outs = net.eval()(x)
    assert isinstance(outs, tuple)
    assert [tuple(t.shape) for t in outs] == [(1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
    assert RECORDED[leaf]["neck"]["in_channels"] == [t.shape[1] for t in outs]


@needs_ref
@pytest.mark.parametrize("leaf", FAMILY)
def test_the_reference_leaves_load_and_their_backbone_builds(leaf):
    cfg = load_config(os.path.join(REF_CONFIGS, leaf))["model"]["encoders"]["camera"]["backbone"]
    assert cfg["type"] == "ResNet" and cfg["depth"] == 50
    before = copy.deepcopy(cfg)
    net = registry.BACKBONES.build(cfg)
    assert cfg == before and type(net) is cr.ResNet and len(net._all_blocks()) == 16
    if leaf in LEAVES:
        assert cfg == RECORDED[leaf]["backbone"]


# ---- state dict --------------------------------------------------------------------------------------------------------------------
def bn_keys(prefix):
    return [prefix + "." + k for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]


def expected_keys(stage_blocks, convs):
    """torchvision's names by the rule: conv1, bn1, layer<i>.<j>.conv<k> / bn<k>, layer<i>.0.downsample.{0,1}."""
    keys = ["conv1.weight"] + bn_keys("bn1")
    for i, n in enumerate(stage_blocks, start=1):
        for j in range(n):
            for k in range(1, convs + 1):
                keys += [f"layer{i}.{j}.conv{k}.weight"] + bn_keys(f"layer{i}.{j}.bn{k}")
            if j == 0:
                keys += [f"layer{i}.0.downsample.0.weight"] + bn_keys(f"layer{i}.0.downsample.1")
    return keys


def test_state_dict_keys_are_torchvisions():
    net = cr.ResNet(depth=50)
    want = expected_keys((3, 4, 6, 3), 3)
    nbt = [k for k in want if k.endswith("num_batches_tracked")]
    assert len(want) == 6 + 16 * 3 * 6 + 4 * 6 and len(want) - len(nbt) == 5 + 16 * 3 * 5 + 4 * 5
    assert sorted(net.state_dict()) == sorted(want)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert shapes["conv1.weight"] == (64, 3, 7, 7) and shapes["layer1.0.conv1.weight"] == (64, 64, 1, 1)
    assert shapes["layer1.0.conv3.weight"] == (256, 64, 1, 1) and shapes["layer1.0.downsample.0.weight"] == (256, 64, 1, 1)
    assert shapes["layer2.0.conv2.weight"] == (128, 128, 3, 3) and shapes["layer4.0.downsample.0.weight"] == (2048, 1024, 1, 1)
    assert net.layer1[0].downsample[0].stride == (1, 1) and net.layer2[0].downsample[0].stride == (2, 2)
    assert net.layer2[0].conv2.stride == (2, 2) and net.layer2[0].conv1.stride == (1, 1) and net.layer2[1].downsample is None
    # a torchvision state dict is this plus fc.*: with those removed it loads strictly
    g = torch.Generator().manual_seed(0)
    state = {k: torch.rand(v.shape, generator=g) if v.dtype.is_floating_point else torch.tensor(3) for k, v in net.state_dict().items()}
    other = cr.ResNet(depth=50)
    res = other.load_state_dict(state, strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []
    assert all(torch.equal(v, state[k]) for k, v in other.state_dict().items())
    with pytest.raises(RuntimeError, match="fc.weight"):
        other.load_state_dict(dict(state, **{"fc.weight": torch.zeros(1000, 2048)}), strict=True)


def test_depth_18_has_basic_block_keys_and_the_other_depths_their_blocks():
    net = cr.ResNet(depth=18)
    assert sorted(net.state_dict()) == sorted(k for k in expected_keys((2, 2, 2, 2), 2) if not k.startswith("layer1.0.downsample"))
    assert all(type(b) is br.BasicBlock for b in net._all_blocks()) and net.layer1[0].downsample is None and net.feat_dim == 512
    assert [len(getattr(cr.ResNet(depth=34), f"layer{i}")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert [len(s) for s in cr.ResNet(depth=101)._stages()] == [3, 4, 23, 3] and [len(s) for s in cr.ResNet(depth=152)._stages()] == [3, 8, 36, 3]
    with pytest.raises(KeyError):
        cr.ResNet(depth=20)


@pytest.mark.parametrize("name, kwargs", [("deep_stem", dict(deep_stem=True)), ("avg_down", dict(avg_down=True)),
                                          ("dcn", dict(dcn=dict(type="DCN", deform_groups=1), stage_with_dcn=(False, True, True, True))),
                                          ("plugins", dict(plugins=[dict(cfg=dict(type="ContextBlock"), stages=(True,) * 4)])),
                                          ("with_cp", dict(with_cp=True)), ("conv_cfg", dict(conv_cfg=dict(type="ConvWS")))])
def test_unsupported_arguments_raise_and_name_themselves(name, kwargs):
    with pytest.raises(NotImplementedError, match=name):
        cr.ResNet(depth=50, **kwargs)


def test_norm_cfg_goes_through_the_registry_and_conv_cfg_conv2d_is_plain():
    net = cr.ResNet(depth=50, num_stages=1, strides=(1,), dilations=(1,), out_indices=(0,), conv_cfg=dict(type="Conv2d"),
                    norm_cfg=dict(type="SyncBN", requires_grad=False))
    norms = [m for m in net.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    assert len(norms) == 1 + 3 * 3 + 1 and all(type(m) is nn.SyncBatchNorm for m in norms)
    assert all(not p.requires_grad for m in norms for p in m.parameters()) and net.conv1.weight.requires_grad
    net18 = cr.ResNet(depth=18, norm_cfg=dict(type="BN2d", requires_grad=False, eps=1e-3))
    assert net18.layer1[0].bn1.eps == 1e-3 and not net18.layer1[0].bn2.weight.requires_grad and type(net18.layer1[0].bn1) is nn.BatchNorm2d


def test_init_weights_is_kaiming_ones_and_a_zero_last_norm():
    torch.manual_seed(0)
    net = cr.ResNet(**SMALL)
    with torch.no_grad():
        for p in net.parameters():
            p.fill_(0.37)
    v0 = net.layer1[0].conv3.weight._version
    net.init_weights()
    assert net.layer1[0].conv3.weight._version > v0                      # written in place: the folds see it
    for blk in net._all_blocks():
        assert not blk.bn3.weight.detach().any() and not blk.bn3.bias.detach().any()
        assert torch.equal(blk.bn1.weight, torch.ones_like(blk.bn1.weight)) and not blk.bn2.bias.detach().any()
        std = blk.conv2.weight.std().item()
        assert abs(std - (2.0 / (9 * blk.conv2.out_channels)) ** 0.5) < 0.15 * std
    assert torch.equal(net.bn1.weight, torch.ones(64)) and torch.equal(net.layer2[0].downsample[1].weight, torch.ones(256))
    keep = cr.ResNet(zero_init_residual=False, **SMALL)
    keep.init_weights()
    assert torch.equal(keep.layer1[0].bn3.weight, torch.ones(128))
    named = cr.ResNet(pretrained="torchvision://resnet50", **SMALL)
    assert named.init_cfg == dict(type="Pretrained", checkpoint="torchvision://resnet50")
    before = {k: v.clone() for k, v in named.state_dict().items()}
    named.init_weights()
    assert all(torch.equal(v, before[k]) for k, v in named.state_dict().items())
    with pytest.raises(AssertionError):
        cr.ResNet(pretrained="a", init_cfg=dict(type="Pretrained", checkpoint="b"), **SMALL)


# ---- the torch path ----------------------------------------------------------------------------------------------------------------
def randomise(net, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                K = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / K) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.8 + 0.4 * torch.rand(n, generator=g))
                m.bias.copy_(0.3 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=g))
    return net


def plain_chain(net, x):
    """mmdet's order from the same parameters, written with functional calls only."""
    def bn(m, t):
        return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
    x = F.max_pool2d(torch.relu(bn(net.bn1, F.conv2d(x, net.conv1.weight, None, 2, 3))), 3, 2, 1)
    outs = []
    for i in range(net.num_stages):
        for blk in getattr(net, f"layer{i + 1}"):
            s1, s2 = (1, blk.stride) if blk.style == "pytorch" else (blk.stride, 1)
            out = torch.relu(bn(blk.bn1, F.conv2d(x, blk.conv1.weight, None, s1, 0)))
            out = torch.relu(bn(blk.bn2, F.conv2d(out, blk.conv2.weight, None, s2, blk.dilation, blk.dilation)))
            out = bn(blk.bn3, F.conv2d(out, blk.conv3.weight, None, 1, 0))
            res = x if blk.downsample is None else bn(blk.downsample[1], F.conv2d(x, blk.downsample[0].weight, None, blk.stride, 0))
            x = torch.relu(out + res)
        if i in net.out_indices:
            outs.append(x)
    return outs


@pytest.mark.parametrize("kwargs", [dict(), dict(style="caffe"), dict(dilations=(1, 2), strides=(1, 1)), dict(out_indices=(1,))],
                         ids=["pytorch", "caffe", "dilated", "last_only"])
def test_float64_torch_path_equals_a_plain_chain(kwargs):
    net = randomise(cr.ResNet(**dict(SMALL, **kwargs))).double().eval()
    x = torch.randn(2, 3, 33, 47, generator=torch.Generator().manual_seed(1)).double()
    assert not net.fusable(x) and len(net._all_blocks()) == 7
    with torch.no_grad():
        got, want = net(x), plain_chain(net, x)
    assert isinstance(got, tuple) and len(got) == len(net.out_indices)
    if not kwargs:
        assert [tuple(t.shape) for t in got] == [(2, 128, 9, 12), (2, 256, 5, 6)]
    if kwargs.get("style") == "caffe":
        blk = net.layer2[0]
        assert blk.conv1.stride == (2, 2) and blk.conv2.stride == (1, 1) and tuple(got[1].shape) == (2, 256, 5, 6)
    if "dilations" in kwargs:
        blk = net.layer2[1]
        assert blk.conv2.dilation == (2, 2) and blk.conv2.padding == (2, 2) and tuple(got[1].shape) == (2, 256, 9, 12)
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()


def test_train_follows_mmdets_frozen_stages_and_norm_eval():
    net = cr.ResNet(frozen_stages=1, norm_eval=False, **SMALL)
    net.train()
    assert net.training and not net.bn1.training and not net.conv1.weight.requires_grad and not net.bn1.weight.requires_grad
    assert all(not m.training for m in net.layer1.modules()) and all(not p.requires_grad for p in net.layer1.parameters())
    assert all(m.training for m in net.layer2.modules()) and all(p.requires_grad for p in net.layer2.parameters())
    x = torch.randn(2, 3, 33, 47, generator=torch.Generator().manual_seed(2))
    assert not net.fusable(x)
    net(x)[-1].sum().backward()
    assert int(net.bn1.num_batches_tracked) == 0 and int(net.layer1[0].bn1.num_batches_tracked) == 0
    assert all(int(m.num_batches_tracked) == 1 for m in net.layer2.modules() if isinstance(m, nn.BatchNorm2d))
    assert net.layer2[0].conv1.weight.grad is not None and net.conv1.weight.grad is None

    stem_only = cr.ResNet(frozen_stages=0, norm_eval=False, **SMALL).train()
    assert not stem_only.bn1.training and stem_only.layer1[0].bn1.training and stem_only.layer1[0].conv1.weight.requires_grad

    quiet = cr.ResNet(norm_eval=True, **SMALL).train()
    assert quiet.training and quiet.layer1[0].training and all(not m.training for m in quiet.modules() if isinstance(m, nn.BatchNorm2d))
    quiet(x)
    assert all(int(m.num_batches_tracked) == 0 for m in quiet.modules() if isinstance(m, nn.BatchNorm2d))
    assert quiet.conv1.weight.requires_grad and not quiet.fusable(x)

    loud = cr.ResNet(norm_eval=False, **SMALL).train()
    loud(x)
    assert all(int(m.num_batches_tracked) == 1 for m in loud.modules() if isinstance(m, nn.BatchNorm2d))
    assert all(not m.training for m in loud.eval().modules())


def test_host_tensors_and_fp32_take_the_torch_layers():
    net = randomise(cr.ResNet(**SMALL)).eval()
    assert net.use_fused and net.fused_stem and isinstance(net.fused_tails, tuple)
    x = torch.randn(1, 3, 16, 16)
    with torch.no_grad():
        assert not net.fusable(x) and not net.half().fusable(x.half())
    z = torch.zeros(1, 32, 4, 4, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cr.bottleneck_tail_forward(z, torch.zeros(1, 128, 4, 4, dtype=torch.float16), cr.fold_bottleneck(net.layer1[1]))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        cr.stem_forward(x.half(), cr.fold_stem(net.conv1, net.bn1, net.maxpool))


# ---- what the kernels serve --------------------------------------------------------------------------------------------------------
def _bottleneck(inplanes=64, planes=16, stride=1, down=True, **kw):
    d = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4)) if down else None
    return cr.Bottleneck(inplanes, planes, stride, downsample=d, **kw).eval()


def test_bottleneck_structure_and_spec():
    blk = _bottleneck(64, 16, 2)
    assert cr.Bottleneck.expansion == 4 and blk.conv2.stride == (2, 2) and blk.conv1.stride == (1, 1) and blk.conv3.out_channels == 64
    caffe = _bottleneck(64, 16, 2, style="caffe")
    assert caffe.conv1.stride == (2, 2) and caffe.conv2.stride == (1, 1)
    dil = _bottleneck(64, 16, 1, dilation=2)
    assert dil.conv2.padding == (2, 2) and dil.conv2.dilation == (2, 2)
    assert cr.bottleneck_spec(_bottleneck(64, 16, down=False)) == ("identity", 1)
    assert cr.bottleneck_spec(_bottleneck(48, 16, 1)) == ("downsample", 1)
    assert cr.bottleneck_spec(blk) == ("downsample", 2) and cr.bottleneck_spec(caffe) == ("downsample", 2)
    assert cr.bottleneck_spec(dil) == ("downsample", 1)                            # the dilation is conv2's business, not the tail's
    assert cr.bottleneck_spec(_bottleneck(256, 128, 2)) == ("downsample", 2)
    assert cr.bottleneck_spec(_bottleneck(64, 12, 1)) is None                      # C = 48, P = 12
    assert cr.bottleneck_spec(_bottleneck(64, 24, 1)) is None                      # P = 24 (C = 96 is a multiple of 32)
    assert cr.bottleneck_spec(_bottleneck(24, 16, 1)) is None                      # Cx = 24
    assert cr.bottleneck_spec(_bottleneck(64, 16, 1).train()) is None              # BatchNorm in train mode
    assert cr.bottleneck_spec(br.BasicBlock(32, 32)) is None
    b = _bottleneck(64, 16, 1)
    b.downsample[1].train()
    assert cr.bottleneck_spec(b) is None
    b = _bottleneck(64, 16, 1)
    b.bn3 = nn.BatchNorm2d(64, track_running_stats=False).eval()
    assert cr.bottleneck_spec(b) is None
    for conv3 in (nn.Conv2d(16, 64, 1), nn.Conv2d(16, 64, 1, groups=2, bias=False), nn.Conv2d(16, 64, 3, padding=1, bias=False),
                  nn.Conv2d(16, 64, 1, stride=2, bias=False), nn.Conv2d(16, 64, 1, padding=1, bias=False)):
        b = _bottleneck(64, 16, 1)
        b.conv3 = conv3
        assert cr.bottleneck_spec(b) is None, conv3
    for down in (nn.Sequential(nn.Conv2d(64, 64, 1, stride=4, bias=False), nn.BatchNorm2d(64)),
                 nn.Sequential(nn.Conv2d(64, 64, 1), nn.BatchNorm2d(64)),
                 nn.Sequential(nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)),
                 nn.Sequential(nn.Conv2d(64, 64, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU()),
                 nn.Sequential(nn.Conv2d(64, 64, 1, bias=False), nn.GroupNorm(2, 64)),
                 nn.Sequential(nn.AvgPool2d(1), nn.BatchNorm2d(64)), nn.Conv2d(64, 64, 1, bias=False)):
        b = _bottleneck(64, 16, 1)
        b.downsample = down.eval()
        assert cr.bottleneck_spec(b) is None, down
    with pytest.raises(RuntimeError, match="does not serve"):
        cr.fold_bottleneck(_bottleneck(64, 12, 1).half())
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        cr.fold_bottleneck(_bottleneck(64, 16, 1))


def test_stem_spec_names_what_the_kernel_serves():
    conv, bn, pool = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64).eval(), nn.MaxPool2d(3, 2, 1)
    assert cr.stem_spec(conv, bn, pool) == (7, 2, 3)
    for bad in (nn.Conv2d(3, 64, 3, 2, 1, bias=False), nn.Conv2d(3, 64, 7, 2, 3), nn.Conv2d(3, 32, 7, 2, 3, bias=False),
                nn.Conv2d(4, 64, 7, 2, 3, bias=False), nn.Conv2d(3, 64, 7, 1, 3, bias=False), nn.Conv2d(3, 64, 7, 2, 2, bias=False),
                nn.Conv2d(3, 64, 7, 2, 6, dilation=2, bias=False), nn.Conv2d(3, 64, 7, 2, 3, bias=False, padding_mode="reflect")):
        assert cr.stem_spec(bad, bn, pool) is None, bad
    assert cr.stem_spec(conv, nn.BatchNorm2d(64), pool) is None                    # train mode
    assert cr.stem_spec(conv, nn.BatchNorm2d(64, track_running_stats=False).eval(), pool) is None
    assert cr.stem_spec(conv, nn.GroupNorm(2, 64), pool) is None
    for bad in (nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(2, 2), nn.MaxPool2d(3, 2, 0), nn.MaxPool2d(3, 1, 1),
                nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(3, 2, 1, return_indices=True), nn.AvgPool2d(3, 2, 1)):
        assert cr.stem_spec(conv, bn, bad) is None, bad
    with pytest.raises(RuntimeError, match="does not serve"):
        cr.fold_stem(conv, bn, nn.MaxPool2d(3, 2, 1, ceil_mode=True))
    net = cr.ResNet(**SMALL).eval()
    assert cr.stem_spec(net.conv1, net.bn1, net.maxpool) == (7, 2, 3)
    assert cr.stem_spec(cr.ResNet(depth=50, base_channels=32).conv1, bn, pool) is None          # a 32-channel stem


# ---- the folds ---------------------------------------------------------------------------------------------------------------------
def half_bottleneck(seed, inplanes=48, planes=16, stride=2, down=True):
    g = torch.Generator().manual_seed(seed)
    blk = _bottleneck(inplanes, planes, stride, down)
    with torch.no_grad():
        for bn in [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if down else []):
            c = bn.num_features
            bn.weight.copy_((torch.rand(c, generator=g) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0))
            bn.bias.copy_(torch.randn(c, generator=g))
            bn.running_mean.copy_(torch.randn(c, generator=g))
            bn.running_var.copy_(torch.rand(c, generator=g) + 0.1)
    return blk.half().eval()


@pytest.mark.parametrize("down", [True, False])
def test_tail_fold_against_the_float64_formula(down):
    blk = half_bottleneck(1, inplanes=48 if down else 64, stride=2 if down else 1, down=down)
    fold = cr.fold_bottleneck(blk)
    pairs = [(blk.bn3, fold.scale3, fold.shift3)] + ([(blk.downsample[1], fold.scale_d, fold.shift_d)] if down else [])
    for bn, scale, shift in pairs:
        s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        t64 = bn.bias.double() - bn.running_mean.double() * s64
        assert scale.dtype == torch.float32 and shift.dtype == torch.float32
        assert ((scale.double() - s64).abs() <= 2.0 ** -22 * s64.abs()).all() and ((shift.double() - t64).abs() <= 2.0 ** -22 * t64.abs()).all()
    assert fold.packed3.dtype == torch.float16 and fold.packed3.numel() == 64 * 32           # P 16 padded to one chunk of 32
    assert torch.equal(bt.bev_unpack_weight(fold.packed3, 16, 64, 1), blk.conv3.weight.detach())
    if down:
        assert (fold.planes, fold.channels, fold.x_channels, fold.residual, fold.stride) == (16, 64, 48, "downsample", 2)
        assert fold.packed_d.numel() == 64 * 64 and torch.equal(bt.bev_unpack_weight(fold.packed_d, 48, 64, 1), blk.downsample[0].weight.detach())
    else:
        assert (fold.planes, fold.channels, fold.x_channels, fold.residual, fold.stride) == (16, 64, 64, "identity", 1)
        assert fold.packed_d is None and fold.scale_d is None and fold.shift_d is None


def test_fold_caches_are_reused_and_refreshed():
    blk = half_bottleneck(0)
    a = cr.fold_bottleneck(blk)
    assert cr.fold_bottleneck(blk) is a
    with torch.no_grad():
        blk.downsample[1].bias.add_(1.0)                            # an in-place write moves the version
    b = cr.fold_bottleneck(blk)
    assert b is not a and not torch.equal(b.shift_d, a.shift_d) and torch.equal(b.scale_d, a.scale_d) and torch.equal(b.shift3, a.shift3)
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    state["conv3.weight"] = state["conv3.weight"] * 2
    blk.load_state_dict(state)
    c = cr.fold_bottleneck(blk)
    assert c is not b and torch.equal(bt.bev_unpack_weight(c.packed3, 16, 64, 1), state["conv3.weight"]) and cr.fold_bottleneck(blk) is c
    blk.conv3.weight = nn.Parameter(blk.conv3.weight.detach().clone())          # a new tensor: the address moves
    assert cr.fold_bottleneck(blk) is not c

    net = randomise(cr.ResNet(**SMALL)).half().eval()
    stem = (net.conv1, net.bn1, net.maxpool)
    f = cr.fold_stem(*stem)
    assert cr.fold_stem(*stem) is f and f.packed.dtype == torch.float16 and f.packed.numel() == cr.STEM_PACKED_ELEMS == 12288
    assert f.scale.dtype == torch.float32 and f.scale.numel() == 64 and torch.equal(cr.stem_unpack_weight(f.packed), net.conv1.weight.detach())
    s64 = net.bn1.weight.double() / torch.sqrt(net.bn1.running_var.double() + net.bn1.eps)
    assert ((f.scale.double() - s64).abs() <= 2.0 ** -22 * s64.abs()).all()
    with torch.no_grad():
        net.bn1.running_mean.mul_(2.0)
    f2 = cr.fold_stem(*stem)
    assert f2 is not f and torch.equal(f2.scale, f.scale) and not torch.equal(f2.shift, f.shift) and cr.fold_stem(*stem) is f2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_stem_pack_and_unpack_are_exact_inverses(dtype):
    g = torch.Generator().manual_seed(4)
    w = torch.randn(64, 3, 7, 7, generator=g).to(dtype)
    w[w == 0] = 1.0                                                     # so that every zero below is a padding position
    flat = cr.stem_pack_weight(w)
    assert flat.shape == (12288,) and flat.dtype == dtype and flat.is_contiguous()
    back = cr.stem_unpack_weight(flat)
    assert torch.equal(back, w) and int((flat == 0).sum()) == 12288 - 64 * 147
    # the order the docstring defines, element by element
    f = flat.reshape(4, 6, 64, 8)
    for mt, ks, lane, j in ((0, 0, 0, 0), (1, 2, 37, 5), (3, 4, 63, 6), (2, 5, 0, 3), (0, 3, 21, 6)):
        pair = 4 * ks + (lane >> 4)
        assert pair < 21 and f[mt, ks, lane, j] == w[16 * mt + (lane & 15), pair // 7, pair % 7, j]
    assert float(f[:, :, :, 7].abs().max()) == 0.0 and float(f[:, 5, 16:, :].abs().max()) == 0.0      # kx = 7; pairs 21 .. 23
    assert torch.equal(cr.stem_pack_weight(back), flat)
    with pytest.raises(RuntimeError, match=r"\[64, 3, 7, 7\]"):
        cr.stem_pack_weight(torch.zeros(64, 3, 3, 3))


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def _addr(on):
    return ctypes.c_void_p(on * (64 << 20) or None)


def _tail(lib, P=32, C=64, Cx=48, Hx=9, Wx=7, s=2, residual=1, batch=2, h=1, x=2, dst=3, packed3=4, packed_d=5, scale3=6, scale_d=7,
          h_layout=1, x_layout=0, dst_layout=1, dtype=0, OH=None, OW=None, packed3_elems=None, packed_d_elems=None, dst_elems=None,
          addr_of=None):
    """bevamd_bottleneck_tail_forward with made-up non-null addresses (64 MiB apart): every case here is refused before any GPU work."""
    st = max(s, 1)
    OH = (Hx - 1) // st + 1 if OH is None else OH
    OW = (Wx - 1) // st + 1 if OW is None else OW
    if packed3_elems is None:
        packed3_elems = C * (-(-P // 32)) * 32
    if packed_d_elems is None:
        packed_d_elems = C * (-(-Cx // 32)) * 32 if residual == 1 else 0
    if dst_elems is None:
        dst_elems = batch * C * OH * OW
    addr = addr_of or _addr
    return lib.bevamd_bottleneck_tail_forward(addr(h), h_layout, P, addr(x), x_layout, Cx, Hx, Wx, dtype, batch, C, OH, OW, residual, s,
                                              addr(packed3), packed3_elems, addr(scale3), addr(scale3), addr(packed_d), packed_d_elems,
                                              addr(scale_d), addr(scale_d), addr(dst), dst_layout, dst_elems, None)


IDENT = dict(residual=0, s=1, Cx=64, packed_d=0, scale_d=0)


def _off(which, by):
    return lambda on: ctypes.c_void_p(on * (64 << 20) + (by if on == which else 0) or None)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(C=48), 4, "channels 48 must be a multiple of 32"),
    (dict(C=0), 4, "multiple of 32"),
    (dict(P=24), 4, "planes 24 must be a multiple of 16"),
    (dict(P=0), 4, "planes 0"),
    (dict(Cx=24), 4, "x_channels 24 must be a multiple of 16"),
    (dict(Cx=8), 4, "multiple of 16"),
    (dict(s=3), 4, "stride 3"),
    (dict(s=0), 4, "stride 0"),
    (dict(residual=2), 4, "residual mode 2"),
    (dict(batch=65536), 1, "batch"),
    (dict(batch=-1), 1, "batch"),
    (dict(Hx=0, OH=1), 1, "bad sizes"),
    (dict(OW=0), 1, "bad sizes"),
    (dict(dtype=2), 1, "dtype"),
    (dict(h_layout=2), 1, "layouts"),
    (dict(x_layout=-1), 1, "layouts"),
    (dict(dst_layout=3), 1, "layouts"),
    (dict(OH=4), 1, "does not give"),
    (dict(s=1, OW=4), 1, "does not give"),
    (dict(IDENT, Cx=32), 1, "identity residual"),
    (dict(IDENT, OH=8), 1, "identity residual"),
    (dict(IDENT, s=2, Hx=1, Wx=1), 1, "identity residual"),
    (dict(packed3_elems=7), 1, "packed3 holds 7"),
    (dict(P=48, packed3_elems=64 * 48), 1, "packed3 holds 3072"),
    (dict(packed_d_elems=64 * 48), 1, "packed_d holds 3072"),
    (dict(IDENT, packed_d_elems=64 * 64), 1, "packed_d holds 4096"),
    (dict(dst_elems=5), 1, "dst holds 5"),
    (dict(batch=65535, Hx=400, Wx=400, s=1), 1, "too many pixels"),
    (dict(packed3=0), 1, "packed3 is null"),
    (dict(packed_d=0), 1, "packed_d is null"),
    (dict(scale3=0), 1, "scale3 or shift3"),
    (dict(scale_d=0), 1, "scale_d or shift_d"),
    (dict(h=0), 1, "is null"),
    (dict(x=0), 1, "is null"),
    (dict(dst=0), 1, "is null"),
    (dict(addr_of=_off(4, 8)), 1, "packed3 is null or not 16-byte"),
    (dict(addr_of=_off(7, 4)), 1, "scale_d or shift_d"),
    (dict(addr_of=_off(1, 8)), 1, "NHWC h is not 16-byte"),
    (dict(x_layout=1, addr_of=_off(2, 8)), 1, "NHWC x is not 16-byte"),
    (dict(addr_of=_off(3, 4)), 1, "NHWC dst is not 8-byte"),
    (dict(dst_layout=0, addr_of=_off(3, 1)), 1, "2-byte aligned"),
    (dict(dst=1), 1, "overlaps"),
    (dict(dst=2), 1, "overlaps"),
    (dict(addr_of=lambda on: ctypes.c_void_p((on * (64 << 20) if on != 3 else 2 * (64 << 20) + 2 * 2 * 48 * 9 * 7 - 16) or None)), 1, "overlaps"),
    (dict(addr_of=lambda on: ctypes.c_void_p((on * (64 << 20) if on != 3 else (64 << 20) + 2 * 2 * 32 * 5 * 4 - 16) or None)), 1, "overlaps"),
])
def test_tail_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _tail(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_tail_entry_point_does_not_require_four_planes_and_an_empty_batch_is_nothing_to_do():
    lib = _capi.load()
    assert _tail(lib, batch=0, h=0, x=0, dst=0) == 0 and _tail(lib, batch=0, h=0, x=0, dst=0, **IDENT) == 0
    assert _tail(lib, batch=0, h=0, x=0, dst=0, P=48, C=160) == 0 and _tail(lib, batch=0, h=0, x=0, dst=0, P=128, C=32) == 0


def _stem(lib, batch=2, cin=3, H=9, W=7, cout=64, k=7, s=2, p=3, pk=3, ps=2, pp=1, ceil=0, x=1, dst=2, packed=3, scale=4, dtype=0,
          dst_layout=1, packed_elems=12288, dst_elems=None, addr_of=None):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if dst_elems is None:
        dst_elems = batch * 64 * ((OH - 1) // 2 + 1) * ((OW - 1) // 2 + 1)
    addr = addr_of or _addr
    return lib.bevamd_resnet_stem_forward(addr(x), dtype, batch, cin, H, W, cout, k, s, p, pk, ps, pp, ceil, addr(packed), packed_elems,
                                          addr(scale), addr(scale), addr(dst), dst_layout, dst_elems, None)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(cin=4), 4, "convolution 4 -> 64"),
    (dict(cout=32), 4, "convolution 3 -> 32"),
    (dict(k=3), 4, "kernel 3"),
    (dict(s=1), 4, "stride 1"),
    (dict(p=2), 4, "padding 2"),
    (dict(pk=2), 4, "pooling kernel 2"),
    (dict(ps=1), 4, "stride 1"),
    (dict(pp=0), 4, "padding 0"),
    (dict(ceil=1), 4, "ceil_mode 1"),
    (dict(batch=65536), 1, "batch"),
    (dict(batch=-1), 1, "batch"),
    (dict(H=0), 1, "bad sizes"),
    (dict(W=-3), 1, "bad sizes"),
    (dict(dtype=2), 1, "dtype"),
    (dict(dst_layout=2), 1, "dst_layout"),
    (dict(packed_elems=64 * 147), 1, "packed holds 9408"),
    (dict(dst_elems=5), 1, "dst holds 5"),
    (dict(packed=0), 1, "packed is null"),
    (dict(scale=0), 1, "scale or shift"),
    (dict(x=0), 1, "is null"),
    (dict(dst=0), 1, "is null"),
    (dict(addr_of=_off(3, 8)), 1, "packed is null or not 16-byte"),
    (dict(addr_of=_off(4, 4)), 1, "scale or shift"),
    (dict(addr_of=_off(1, 1)), 1, "2-byte aligned"),
    (dict(addr_of=_off(2, 8)), 1, "NHWC dst is not 16-byte"),
    (dict(dst_layout=0, addr_of=_off(2, 1)), 1, "2-byte aligned"),
    (dict(dst=1), 1, "overlaps"),
    (dict(dst_layout=0, addr_of=lambda on: ctypes.c_void_p((on * (64 << 20) if on != 2 else (64 << 20) + 2 * 2 * 3 * 9 * 7 - 16) or None)), 1, "overlaps"),
])
def test_stem_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _stem(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_stem_empty_batch_is_nothing_to_do():
    assert _stem(_capi.load(), batch=0, x=0, dst=0) == 0


def test_binding_table_equals_the_header():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_(?:bottleneck|resnet_stem)_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_bottleneck_tail_forward", "bevamd_resnet_stem_forward"]
    for name, count in (("bevamd_bottleneck_tail_forward", 27), ("bevamd_resnet_stem_forward", 22)):
        args = protos[name].split(",")
        res, argtypes = _capi._EXT_SIGNATURES[name]
        want = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_int for a in args]
        assert res is ctypes.c_int and argtypes == want and len(want) == count, name
        assert "size_t" not in protos[name] and name in _capi.ext_exported_names()
        assert not re.match(r"bevamd_res_block_\w+", name) and not re.match(r"bevamd_bev_conv_\w+", name)


# ---- the code objects --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(resources.OBJ, "bottleneck.o")) or not all(os.path.exists(t) for t in resources.TOOLS),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_the_kernels_use_no_scratch_spill_nothing_and_fit_two_workgroups():
    found = resources._kernels()
    tails = {n: v for n, v in found.items() if v["obj"] == "bottleneck"}
    names = sorted(f"void bevamd::bottleneck_tail_kernel<{b}, {mt}, {ds}>" for b in ("false", "true") for mt in (1, 2, 4) for ds in ("false", "true"))
    assert sorted(tails) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "bottleneck.o"))
    for name in names:
        got = tails[name]
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= 256, (name, got)                          # two workgroups of four waves per compute unit
        assert lds[name] == 128 * 80 and 2 * lds[name] <= 160 * 1024, (name, lds[name])          # 128 pixels x 80-byte pixels
    stems = {n: v for n, v in found.items() if v["obj"] == "resnet_stem"}
    names = sorted(f"void bevamd::resnet_stem_kernel<{b}>" for b in ("false", "true"))
    assert sorted(stems) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "resnet_stem.o"))
    for name in names:
        got = stems[name]
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= 256, (name, got)
        # the 3 x 23 x 72 input tile and the 9 x 32 conv tile of 68 16-bit elements per pixel
        assert lds[name] == 2 * (3 * 23 * 72 + 9 * 32 * 68) and 2 * lds[name] <= 160 * 1024, (name, lds[name])
