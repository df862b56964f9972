"""GeneralizedResNet (bevfusion_amd/bev_resnet.py) without a GPU: registry and config, the block structure of mmcv's make_res_layer,
state-dict names, the torch path against a plainly written chain, `res_block_spec`, the fold, the entry point's refusals and the
kernels' resources."""
import copy
import ctypes
import json
import os
import re

import pytest
import torch
from torch import nn

import test_kernel_resources as resources
from bevfusion_amd import _capi, bev_resnet as br, bev_trunk as bt, heads, registry
from bevfusion_amd.config import load_config
from test_centerhead_module import REF_CONFIGS, _lds_bytes, needs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORDED = json.load(open(os.path.join(HERE, "golden", "bev_trunk_configs.json")))
RESNET = "nuscenes/det/centerhead/lssfpn/camera/256x704/resnet/default.yaml"
LEAVES = [RESNET, "nuscenes/det/centerhead/lssfpn/camera/256x704/swint/default.yaml",
          "nuscenes/det/centerhead/lssfpn/camera+radar/resnet50/default.yaml", "nuscenes/seg/camera-bev256d2.yaml"]
RECORDED_BLOCKS = [[2, 128, 2], [2, 256, 2], [2, 512, 1]]
LSSFPN_BLOCKS = [[2, 160, 2], [2, 320, 2], [2, 640, 1]]


# ---- registry and config -----------------------------------------------------------------------------------------------------------
def test_the_module_is_registered_and_reexported():
    assert registry.BACKBONES.get("GeneralizedResNet") is br.GeneralizedResNet
    assert heads.GeneralizedResNet is br.GeneralizedResNet and heads.BasicBlock is br.BasicBlock
    assert heads.make_res_layer is br.make_res_layer and heads.res_block_forward is br.res_block_forward
    assert heads.fold_res_block is br.fold_res_block and heads.res_block_spec is br.res_block_spec
    assert all(n in heads.__all__ for n in br.__all__)


def test_the_recorded_backbone_block_builds_and_leaves_its_dict_alone():
    cfg = RECORDED[RESNET]["backbone"]
    before = copy.deepcopy(cfg)
    net = registry.BACKBONES.build(cfg)
    assert cfg == before and type(net) is br.GeneralizedResNet
    assert net.in_channels == 64 and net.blocks == RECORDED_BLOCKS and len(net) == 3
    neck = registry.NECKS.build(RECORDED[RESNET]["neck"])              # the LSSFPN behind it reads stages -1 and 0
    x = torch.zeros(1, 64, 16, 16)
    with torch.no_grad():
        outs = net.eval()(x)
        assert isinstance(outs, list) and [tuple(t.shape) for t in outs] == [(1, 128, 8, 8), (1, 256, 4, 4), (1, 512, 4, 4)]
        assert tuple(neck.eval()(outs).shape) == (1, 256, 16, 16)


@pytest.mark.parametrize("in_channels, blocks", [(64, RECORDED_BLOCKS), (336, LSSFPN_BLOCKS)])
def test_block_structure_is_make_res_layers(in_channels, blocks):
    net = br.GeneralizedResNet(in_channels, blocks)
    assert isinstance(net, nn.ModuleList) and len(net) == len(blocks)
    cin = in_channels
    for stage, (num, cout, stride) in zip(net, blocks):
        assert type(stage) is nn.Sequential and len(stage) == num
        for j, blk in enumerate(stage):
            assert type(blk) is br.BasicBlock and blk.expansion == 1
            s = stride if j == 0 else 1
            c = cin if j == 0 else cout
            assert (blk.conv1.in_channels, blk.conv1.out_channels, blk.conv1.kernel_size, blk.conv1.stride, blk.conv1.padding,
                    blk.conv1.dilation, blk.conv1.bias) == (c, cout, (3, 3), (s, s), (1, 1), (1, 1), None)
            assert (blk.conv2.in_channels, blk.conv2.out_channels, blk.conv2.kernel_size, blk.conv2.stride, blk.conv2.padding,
                    blk.conv2.bias) == (cout, cout, (3, 3), (1, 1), (1, 1), None)
            assert type(blk.bn1) is nn.BatchNorm2d and type(blk.bn2) is nn.BatchNorm2d and blk.bn1.num_features == cout
            assert (blk.bn2.eps, blk.bn2.momentum) == (1e-5, 0.1) and type(blk.relu) is nn.ReLU and blk.relu.inplace
            if j == 0:      # on block 0 of EVERY stage here (the stride-1 stage changes its width), nowhere else
                d = blk.downsample
                assert type(d) is nn.Sequential and len(d) == 2 and type(d[0]) is nn.Conv2d and type(d[1]) is nn.BatchNorm2d
                assert (d[0].in_channels, d[0].out_channels, d[0].kernel_size, d[0].stride, d[0].padding, d[0].bias) == \
                    (cin, cout, (1, 1), (stride, stride), (0, 0), None)
            else:
                assert blk.downsample is None
        cin = cout
    assert br.make_res_layer(br.BasicBlock, 32, 32, 2)[0].downsample is None          # same width at stride 1: no downsample


# ---- state dict --------------------------------------------------------------------------------------------------------------------
def bn_keys(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
            (prefix + ".num_batches_tracked", ())]


def reference_keys():
    """Written out from the reference's module definition at the recorded sizes (64 -> 128, 256, 512; two blocks per stage)."""
    keys = []
    for i, (cin, c) in enumerate([(64, 128), (128, 256), (256, 512)]):
        keys += [(f"{i}.0.conv1.weight", (c, cin, 3, 3))] + bn_keys(f"{i}.0.bn1", c)
        keys += [(f"{i}.0.conv2.weight", (c, c, 3, 3))] + bn_keys(f"{i}.0.bn2", c)
        keys += [(f"{i}.0.downsample.0.weight", (c, cin, 1, 1))] + bn_keys(f"{i}.0.downsample.1", c)
        keys += [(f"{i}.1.conv1.weight", (c, c, 3, 3))] + bn_keys(f"{i}.1.bn1", c)
        keys += [(f"{i}.1.conv2.weight", (c, c, 3, 3))] + bn_keys(f"{i}.1.bn2", c)
    return keys


def test_state_dict_names_and_shapes_equal_the_reference():
    module = br.GeneralizedResNet(64, RECORDED_BLOCKS)
    got = sorted((k, tuple(v.shape)) for k, v in module.state_dict().items())
    assert got == sorted(reference_keys()) and len(got) == 3 * (5 + 5 * 5)
    g = torch.Generator().manual_seed(3)
    state = {k: (torch.rand(s, generator=g) + 0.5) if s else torch.tensor(7) for k, s in reference_keys()}
    other = br.GeneralizedResNet(64, RECORDED_BLOCKS)
    assert other.load_state_dict(state, strict=True).missing_keys == []
    assert all(torch.equal(v, state[k]) for k, v in other.state_dict().items())
    module.load_state_dict(other.state_dict(), strict=True)


# ---- the torch path ----------------------------------------------------------------------------------------------------------------
def small_net(seed=0, in_channels=32, blocks=((2, 32, 2), (1, 64, 1))):
    torch.manual_seed(seed)
    net = br.GeneralizedResNet(in_channels, [list(b) for b in blocks])
    net.init_weights()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.2)
    return net


def plain_chain(net, x):
    """The specification's order from the same parameters, written with functional calls only."""
    F = torch.nn.functional

    def bn(m, t):
        return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
    outs = []
    for stage in net:
        for blk in stage:
            out = F.conv2d(x, blk.conv1.weight, None, blk.conv1.stride, 1)
            out = torch.relu(bn(blk.bn1, out))
            out = bn(blk.bn2, F.conv2d(out, blk.conv2.weight, None, 1, 1))
            res = x if blk.downsample is None else bn(blk.downsample[1], F.conv2d(x, blk.downsample[0].weight, None, blk.downsample[0].stride, 0))
            x = torch.relu(out + res)
        outs.append(x)
    return outs


def test_torch_path_on_the_cpu_bit_equals_a_plain_chain():
    net = small_net().eval()
    x = torch.randn(2, 32, 12, 10, generator=torch.Generator().manual_seed(1))
    assert not net.fusable(x)
    with torch.no_grad():
        got, want = net(x), plain_chain(net, x)
    assert isinstance(got, list) and [tuple(t.shape) for t in got] == [(2, 32, 6, 5), (2, 64, 6, 5)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert net.init_weights() is None


def test_train_mode_updates_the_running_statistics_and_gradients_flow():
    net = small_net()
    x = torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    before = [m.running_mean.clone() for m in bns]
    assert net.training and not net.fusable(x)
    net(x)[-1].sum().backward()
    assert len(bns) == 8 and all(int(m.num_batches_tracked) == 1 for m in bns)
    assert all(not torch.equal(m.running_mean, b) for m, b in zip(bns, before))
    assert x.grad is not None and x.grad.abs().sum() > 0 and all(p.grad is not None for p in net.parameters())


def test_host_tensors_and_fp32_take_the_torch_layers():
    net = small_net().eval()
    assert net.use_fused
    x = torch.randn(1, 32, 8, 8)
    with torch.no_grad():
        assert not net.fusable(x) and not net.half().fusable(x.half()) and not net.fusable(x)
    blk = net[0][1]
    fold = br.fold_res_block(blk)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        br.res_block_forward(torch.zeros(1, 32, 4, 4, dtype=torch.float16), torch.zeros(1, 32, 4, 4, dtype=torch.float16), fold)


# ---- what the kernel serves --------------------------------------------------------------------------------------------------------
def _block(inplanes=32, planes=64, stride=1, down=True):
    d = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes)) if down else None
    return br.BasicBlock(inplanes, planes, stride, downsample=d).eval()


def test_res_block_spec_names_what_the_kernel_serves():
    assert br.res_block_spec(_block(64, 64, down=False)) == ("identity", 1)
    assert br.res_block_spec(_block(32, 64, 1)) == ("downsample", 1)
    assert br.res_block_spec(_block(48, 64, 2)) == ("downsample", 2)
    assert br.res_block_spec(_block(336, 160, 2)) == ("downsample", 2)
    assert br.res_block_spec(_block(32, 48, 1)) is None                      # C = 48
    assert br.res_block_spec(_block(24, 64, 1)) is None                      # Cx = 24
    assert br.res_block_spec(_block(32, 64, 1).train()) is None              # BatchNorm in train mode
    blk = _block(32, 64, 1)
    blk.downsample[1].train()
    assert br.res_block_spec(blk) is None
    blk = _block(32, 64, 1)
    blk.bn2 = nn.BatchNorm2d(64, track_running_stats=False).eval()
    assert br.res_block_spec(blk) is None
    for conv2 in (nn.Conv2d(64, 64, 3, padding=1), nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False),
                  nn.Conv2d(64, 64, 3, padding=2, dilation=2, bias=False), nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False),
                  nn.Conv2d(64, 64, 5, padding=2, bias=False), nn.Conv2d(64, 64, 3, padding=0, bias=False)):
        blk = _block(64, 64, down=False)
        blk.conv2 = conv2
        assert br.res_block_spec(blk) is None, conv2
    for down in (nn.Sequential(nn.Conv2d(32, 64, 1, stride=4, bias=False), nn.BatchNorm2d(64)),
                 nn.Sequential(nn.Conv2d(32, 64, 1), nn.BatchNorm2d(64)),
                 nn.Sequential(nn.Conv2d(32, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)),
                 nn.Sequential(nn.Conv2d(32, 64, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU()),
                 nn.Sequential(nn.Conv2d(32, 64, 1, bias=False), nn.GroupNorm(2, 64)),
                 nn.Conv2d(32, 64, 1, bias=False)):
        blk = _block(32, 64, 1)
        blk.downsample = down.eval()
        assert br.res_block_spec(blk) is None, down
    with pytest.raises(RuntimeError, match="does not serve"):
        br.fold_res_block(_block(32, 48, 1).half())


# ---- the fold ----------------------------------------------------------------------------------------------------------------------
def half_block(seed, cx=48, c=64, stride=2, down=True):
    g = torch.Generator().manual_seed(seed)
    blk = _block(cx, c, stride, down)
    with torch.no_grad():
        for bn in [blk.bn1, blk.bn2] + ([blk.downsample[1]] if down else []):
            bn.weight.copy_((torch.rand(c, generator=g) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0))
            bn.bias.copy_(torch.randn(c, generator=g))
            bn.running_mean.copy_(torch.randn(c, generator=g))
            bn.running_var.copy_(torch.rand(c, generator=g) + 0.1)
    return blk.half().eval()


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("down", [True, False])
def test_scales_and_shifts_against_the_float64_formula(seed, down):
    blk = half_block(seed, cx=48 if down else 64, stride=2 if down else 1, down=down)
    fold = br.fold_res_block(blk)
    pairs = [(blk.bn2, fold.scale2, fold.shift2)] + ([(blk.downsample[1], fold.scale_d, fold.shift_d)] if down else [])
    for bn, scale, shift in pairs:
        s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        t64 = bn.bias.double() - bn.running_mean.double() * s64
        assert scale.dtype == torch.float32 and shift.dtype == torch.float32
        # float64 arithmetic, rounded once: within one fp32 step of the formula written in another order
        assert ((scale.double() - s64).abs() <= 2.0 ** -22 * s64.abs()).all()
        assert ((shift.double() - t64).abs() <= 2.0 ** -22 * t64.abs()).all()
    assert fold.packed2.dtype == torch.float16 and torch.equal(bt.bev_unpack_weight(fold.packed2, 64, 64, 3), blk.conv2.weight.detach())
    if down:
        assert (fold.channels, fold.x_channels, fold.residual, fold.stride) == (64, 48, "downsample", 2)
        assert fold.packed_d.numel() == 64 * 64                                             # Cx 48 padded to two chunks of 32
        assert torch.equal(bt.bev_unpack_weight(fold.packed_d, 48, 64, 1), blk.downsample[0].weight.detach())
    else:
        assert (fold.channels, fold.x_channels, fold.residual, fold.stride) == (64, 64, "identity", 1)
        assert fold.packed_d is None and fold.scale_d is None and fold.shift_d is None


def test_fold_cache_is_reused_and_refreshed():
    blk = half_block(0)
    a = br.fold_res_block(blk)
    assert br.fold_res_block(blk) is a
    with torch.no_grad():
        blk.downsample[1].bias.add_(1.0)                            # an in-place write moves the version
    b = br.fold_res_block(blk)
    assert b is not a and not torch.equal(b.shift_d, a.shift_d) and torch.equal(b.scale_d, a.scale_d) and torch.equal(b.shift2, a.shift2)
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    state["conv2.weight"] = state["conv2.weight"] * 2
    blk.load_state_dict(state)
    c = br.fold_res_block(blk)
    assert c is not b and torch.equal(bt.bev_unpack_weight(c.packed2, 64, 64, 3), state["conv2.weight"])
    assert br.fold_res_block(blk) is c


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def _call(lib, C=64, Cx=48, Hx=9, Wx=7, s=2, residual=1, batch=2, h=1, x=2, dst=3, packed2=4, packed_d=5, scale2=6, scale_d=7,
          h_layout=1, x_layout=0, dst_layout=1, dtype=0, OH=None, OW=None, packed2_elems=None, packed_d_elems=None, dst_elems=None,
          addr_of=None):
    """bevamd_res_block_forward with made-up non-null addresses (64 MiB apart): every case here is refused before any GPU work."""
    st = max(s, 1)
    OH = (Hx - 1) // st + 1 if OH is None else OH
    OW = (Wx - 1) // st + 1 if OW is None else OW
    if packed2_elems is None:
        packed2_elems = 9 * C * C
    if packed_d_elems is None:
        packed_d_elems = C * (-(-Cx // 32)) * 32 if residual == 1 else 0
    if dst_elems is None:
        dst_elems = batch * C * OH * OW
    addr = addr_of or (lambda on: ctypes.c_void_p(on * (64 << 20) or None))
    return lib.bevamd_res_block_forward(addr(h), h_layout, addr(x), x_layout, Cx, Hx, Wx, dtype, batch, C, OH, OW, residual, s,
                                        addr(packed2), packed2_elems, addr(scale2), addr(scale2), addr(packed_d), packed_d_elems,
                                        addr(scale_d), addr(scale_d), addr(dst), dst_layout, dst_elems, None)


IDENT = dict(residual=0, s=1, Cx=64, packed_d=0, scale_d=0)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(C=48), 4, "multiple of 32"),
    (dict(C=0), 4, "multiple of 32"),
    (dict(Cx=24), 4, "multiple of 16"),
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
    (dict(packed2_elems=7), 1, "packed2 holds 7"),
    (dict(packed_d_elems=64 * 48), 1, "packed_d holds 3072"),
    (dict(IDENT, packed_d_elems=64 * 64), 1, "packed_d holds 4096"),
    (dict(dst_elems=5), 1, "dst holds 5"),
    (dict(packed2=0), 1, "packed2 is null"),
    (dict(packed_d=0), 1, "packed_d is null"),
    (dict(scale2=0), 1, "scale2 or shift2"),
    (dict(scale_d=0), 1, "scale_d or shift_d"),
    (dict(h=0), 1, "is null"),
    (dict(x=0), 1, "is null"),
    (dict(dst=0), 1, "is null"),
    (dict(addr_of=lambda on: ctypes.c_void_p(on * (64 << 20) + (8 if on == 4 else 0) or None)), 1, "packed2 is null or not 16-byte"),
    (dict(addr_of=lambda on: ctypes.c_void_p(on * (64 << 20) + (4 if on == 7 else 0) or None)), 1, "scale_d or shift_d"),
    (dict(addr_of=lambda on: ctypes.c_void_p(on * (64 << 20) + (8 if on == 1 else 0) or None)), 1, "NHWC h is not 16-byte"),
    (dict(x_layout=1, addr_of=lambda on: ctypes.c_void_p(on * (64 << 20) + (8 if on == 2 else 0) or None)), 1, "NHWC x is not 16-byte"),
    (dict(addr_of=lambda on: ctypes.c_void_p(on * (64 << 20) + (4 if on == 3 else 0) or None)), 1, "NHWC dst is not 8-byte"),
    (dict(dst_layout=0, addr_of=lambda on: ctypes.c_void_p(on * (64 << 20) + (1 if on == 3 else 0) or None)), 1, "2-byte aligned"),
    (dict(dst=1), 1, "overlaps"),
    (dict(dst=2), 1, "overlaps"),
    (dict(addr_of=lambda on: ctypes.c_void_p((on * (64 << 20) if on != 3 else 2 * (64 << 20) + 2 * 2 * 48 * 9 * 7 - 16) or None)), 1, "overlaps"),
])
def test_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _call(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_an_empty_batch_is_nothing_to_do():
    assert _call(_capi.load(), batch=0, h=0, x=0, dst=0) == 0
    assert _call(_capi.load(), batch=0, h=0, x=0, dst=0, **IDENT) == 0


def test_binding_table_equals_the_header():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_res_block_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_res_block_forward"]
    args = protos["bevamd_res_block_forward"].split(",")
    res, argtypes = _capi._EXT_SIGNATURES["bevamd_res_block_forward"]
    want = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_int for a in args]
    assert res is ctypes.c_int and argtypes == want and len(want) == 26
    assert "size_t" not in protos["bevamd_res_block_forward"]
    assert "bevamd_res_block_forward" in _capi.ext_exported_names()
    assert not re.match(r"bevamd_bev_conv_\w+", "bevamd_res_block_forward")


# ---- the code object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(resources.OBJ, "bev_conv.o")) or not all(os.path.exists(t) for t in resources.TOOLS),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_the_kernels_use_no_scratch_spill_nothing_and_fit_two_workgroups():
    kernels = {n: v for n, v in resources._kernels().items() if v["obj"] == "res_block"}
    names = sorted(f"void bevamd::res_block_kernel<{b}, {mt}, {ds}>" for b in ("false", "true") for mt in (1, 2, 4) for ds in ("false", "true"))
    assert sorted(kernels) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "res_block.o"))
    for name in names:
        got = kernels[name]
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= 256, (name, got)                          # two workgroups of four waves per compute unit
        assert lds[name] == 10 * 18 * 80 and 2 * lds[name] <= 160 * 1024, (name, lds[name])      # the haloed tile x 80-byte pixels


# ---- the reference's configs -------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("leaf", LEAVES)
def test_the_reference_leaves_load_and_their_backbone_builds(leaf):
    model = load_config(os.path.join(REF_CONFIGS, leaf))["model"]
    cfg = model["decoder"]["backbone"]
    assert cfg["type"] == "GeneralizedResNet"
    before = copy.deepcopy(cfg)
    net = registry.BACKBONES.build(cfg)
    assert cfg == before and type(net) is br.GeneralizedResNet and len(net) == len(cfg["blocks"])
    assert net[0][0].conv1.in_channels == cfg["in_channels"] and all(stage[0].downsample is not None for stage in net)
    if leaf == RESNET:
        assert cfg == RECORDED[RESNET]["backbone"]
