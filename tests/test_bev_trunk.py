"""The BEV trunk modules (ConvFuser, SECOND, SECONDFPN) without a GPU: registries and config, state-dict names, the torch path
against plain nn.Sequential chains, the fold, the packed weight order, the entry point's refusals and the kernels' resources."""
import ctypes
import copy
import importlib.util
import json
import os
import re

import pytest
import torch
from torch import nn

import test_kernel_resources as resources
from bevfusion_amd import _capi, bev_trunk as bt, heads, registry
from bevfusion_amd.config import load_config
from test_centerhead_module import REF_CONFIGS, _lds_bytes, needs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORDED = json.load(open(os.path.join(HERE, "golden", "bev_trunk_configs.json")))
FLAGSHIP = "nuscenes/det/transfusion/secfpn/camera+lidar/swint_v0p075/convfuser.yaml"
LIDAR = "nuscenes/det/transfusion/secfpn/lidar/voxelnet_0p075.yaml"
SEG = "nuscenes/seg/fusion-bev256d2-lss.yaml"
RESNET = "nuscenes/det/centerhead/lssfpn/camera/256x704/resnet/default.yaml"
WHERE = {"fuser": registry.FUSERS, "backbone": registry.BACKBONES, "neck": registry.NECKS, "camera_neck": registry.NECKS}
OURS = {"ConvFuser": bt.ConvFuser, "SECOND": bt.SECOND, "SECONDFPN": bt.SECONDFPN}

_spec = importlib.util.spec_from_file_location("make_bev_trunk_configs", os.path.join(HERE, "golden", "make_bev_trunk_configs.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def build_blocks(blocks):
    """Every block of a recorded leaf that names one of the three modules, built from its own dict."""
    out = {}
    for key, cfg in blocks.items():
        if cfg and cfg["type"] in OURS:
            before = copy.deepcopy(cfg)
            out[key] = WHERE[key].build(cfg)
            assert cfg == before and type(out[key]) is OURS[cfg["type"]]
    return out


# ---- registries and config ---------------------------------------------------------------------------------------------------------
def test_the_modules_are_registered_and_reexported():
    assert registry.FUSERS.get("ConvFuser") is bt.ConvFuser and registry.BACKBONES.get("SECOND") is bt.SECOND
    assert registry.NECKS.get("SECONDFPN") is bt.SECONDFPN
    assert heads.ConvFuser is bt.ConvFuser and heads.SECOND is bt.SECOND and heads.SECONDFPN is bt.SECONDFPN
    assert heads.bev_conv_forward is bt.bev_conv_forward and heads.fold_bev_layer is bt.fold_bev_layer


def test_build_upsample_layer_covers_what_the_configs_use():
    up = registry.build_upsample_layer(dict(type="deconv", bias=False), in_channels=4, out_channels=6, kernel_size=2, stride=2)
    assert type(up) is nn.ConvTranspose2d and up.bias is None and up.kernel_size == (2, 2) and up.stride == (2, 2)
    for mode in ("nearest", "bilinear"):
        up = registry.build_upsample_layer(dict(type=mode, scale_factor=2))
        assert type(up) is nn.Upsample and up.mode == mode and up.scale_factor == 2
    with pytest.raises(KeyError):
        registry.build_upsample_layer(dict(type="pixel_shuffle"))


@pytest.mark.parametrize("leaf, keys", [(FLAGSHIP, ["backbone", "fuser", "neck"]), (LIDAR, ["backbone", "neck"]),
                                        (SEG, ["backbone", "fuser", "neck"]), (RESNET, ["camera_neck"])])
def test_the_recorded_yaml_blocks_build(leaf, keys):
    built = build_blocks(RECORDED[leaf])
    assert sorted(built) == keys
    if "fuser" in built:
        f = built["fuser"]
        assert f[0].in_channels == 336 and f[0].out_channels == 256 and f[0].bias is None and f[1].eps == 1e-5 and f[1].momentum == 0.1
    if "backbone" in built:
        b = built["backbone"]
        assert [len(blk) for blk in b.blocks] == [18, 18] and b.blocks[1][0].stride == (2, 2) and b.blocks[0][0].stride == (1, 1)
        assert b.blocks[0][1].eps == 1e-3 and b.blocks[0][1].momentum == 0.01 and b.blocks[0][0].bias is None
    if "neck" in built:
        n = built["neck"]
        assert type(n.deblocks[0][0]) is nn.Conv2d and n.deblocks[0][0].kernel_size == (1, 1)      # use_conv_for_no_stride
        assert type(n.deblocks[1][0]) is nn.ConvTranspose2d and n.deblocks[1][0].kernel_size == (2, 2) and n.deblocks[1][0].bias is None
    if "camera_neck" in built:      # upsample_strides [0.25, 0.5, 1, 2]: the reference's branch logic
        layers = [d[0] for d in built["camera_neck"].deblocks]
        assert [type(l) for l in layers] == [nn.Conv2d, nn.Conv2d, nn.ConvTranspose2d, nn.ConvTranspose2d]
        assert [l.kernel_size for l in layers] == [(4, 4), (2, 2), (1, 1), (2, 2)] and [l.stride for l in layers] == [(4, 4), (2, 2), (1, 1), (2, 2)]
        x = [torch.zeros(1, c, s, s) for c, s in zip([256, 512, 1024, 2048], [16, 8, 4, 2])]
        assert tuple(built["camera_neck"].eval()(x)[0].shape) == (1, 512, 4, 4)


@needs_ref
@pytest.mark.parametrize("leaf", [FLAGSHIP, LIDAR, SEG, RESNET])
def test_the_reference_yaml_chains_build(leaf):
    blocks = gen.blocks(REF_CONFIGS, leaf)
    assert blocks == RECORDED[leaf]
    assert build_blocks(blocks)
    assert load_config(os.path.join(REF_CONFIGS, leaf))["model"] is not None


# ---- state dict --------------------------------------------------------------------------------------------------------------------
def bn_keys(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
            (prefix + ".num_batches_tracked", ())]


def reference_keys():
    """Written out from the reference's module definitions at the flagship sizes."""
    fuser = [("0.weight", (256, 336, 3, 3))] + bn_keys("1", 256)
    second = []
    for i, (cin, c) in enumerate([(256, 128), (128, 256)]):
        for j in range(6):
            second += [(f"blocks.{i}.{3 * j}.weight", (c, cin if j == 0 else c, 3, 3))] + bn_keys(f"blocks.{i}.{3 * j + 1}", c)
    neck = [("deblocks.0.0.weight", (256, 128, 1, 1))] + bn_keys("deblocks.0.1", 256) + \
           [("deblocks.1.0.weight", (256, 256, 2, 2))] + bn_keys("deblocks.1.1", 256)      # ConvTranspose2d: [in, out, 2, 2]
    return dict(fuser=fuser, backbone=second, neck=neck)


@pytest.mark.parametrize("key", ["fuser", "backbone", "neck"])
def test_state_dict_names_and_shapes_equal_the_reference(key):
    module = build_blocks(RECORDED[FLAGSHIP])[key]
    got = sorted((k, tuple(v.shape)) for k, v in module.state_dict().items())
    assert got == sorted(reference_keys()[key])
    g = torch.Generator().manual_seed(3)
    state = {k: (torch.rand(s, generator=g) + 0.5) if s else torch.tensor(7) for k, s in reference_keys()[key]}
    other = build_blocks(RECORDED[FLAGSHIP])[key]
    assert other.load_state_dict(state, strict=True).missing_keys == []
    assert all(torch.equal(v, state[k]) for k, v in other.state_dict().items())
    module.load_state_dict(other.state_dict(), strict=True)


# ---- the torch path ----------------------------------------------------------------------------------------------------------------
def small_modules(seed=0):
    torch.manual_seed(seed)
    fuser = bt.ConvFuser([16, 32], 32)
    second = bt.SECOND(32, [32, 64], [1, 2], [1, 2])
    neck = bt.SECONDFPN([32, 64], [32, 32], [1, 2], use_conv_for_no_stride=True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in (fuser, second, neck):
            m.init_weights()
            for mod in m.modules():
                if isinstance(mod, nn.BatchNorm2d):
                    mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                    mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                    mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.2)
    return fuser, second, neck


def small_inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, 16, 8, 6, generator=g), torch.randn(2, 32, 8, 6, generator=g)]


def plain_chain(fuser, second, neck, xs):
    """conv, norm, ReLU in the reference's order from the same parameters, with `cat` where the reference has it."""
    f = nn.Sequential(fuser[0], fuser[1], nn.ReLU())(torch.cat(xs, dim=1))
    x, stages = f, []
    for blk in second.blocks:
        x = nn.Sequential(*list(blk))(x)
        stages.append(x)
    ups = [nn.Sequential(*list(d))(t) for d, t in zip(neck.deblocks, stages)]
    return f, stages, torch.cat(ups, dim=1)


def test_torch_path_on_the_cpu_bit_equals_plain_sequential_chains():
    fuser, second, neck = [m.eval() for m in small_modules()]
    xs = small_inputs()
    assert not fuser.fusable(xs)
    with torch.no_grad():
        f = fuser(xs)
        s = second(f)
        n = neck(s)
        pf, ps, pn = plain_chain(fuser, second, neck, xs)
    assert isinstance(s, tuple) and isinstance(n, list) and len(n) == 1
    assert torch.equal(f, pf) and all(torch.equal(a, b) for a, b in zip(s, ps)) and torch.equal(n[0], pn)
    assert tuple(n[0].shape) == (2, 64, 8, 6) and [tuple(t.shape) for t in s] == [(2, 32, 8, 6), (2, 64, 4, 3)]
    assert tuple(bt.SECONDFPN([32], [32], [1])([f])[0].shape) == (2, 32, 8, 6)      # one level: no cat


def test_train_mode_updates_the_running_statistics_and_gradients_flow():
    fuser, second, neck = small_modules()
    xs = [x.requires_grad_(True) for x in small_inputs()]
    before = [m.running_mean.clone() for mod in (fuser, second, neck) for m in mod.modules() if isinstance(m, nn.BatchNorm2d)]
    out = neck(second(fuser(xs)))[0]
    out.sum().backward()
    bns = [m for mod in (fuser, second, neck) for m in mod.modules() if isinstance(m, nn.BatchNorm2d)]
    assert all(int(m.num_batches_tracked) == 1 for m in bns)
    assert all(not torch.equal(m.running_mean, b) for m, b in zip(bns, before))
    assert all(x.grad is not None and x.grad.abs().sum() > 0 for x in xs)
    assert all(p.grad is not None for mod in (fuser, second, neck) for p in mod.parameters())


def test_init_weights_follows_the_init_cfg_and_moves_the_versions():
    second = bt.SECOND(32, [32], [1], [1])
    assert second.init_cfg == dict(type="Kaiming", layer="Conv2d")
    assert bt.SECOND(32, [32], [1], [1], pretrained="x.pth").init_cfg == dict(type="Pretrained", checkpoint="x.pth")
    neck = bt.SECONDFPN([32], [32], [2])
    assert neck.init_cfg[0] == dict(type="Kaiming", layer="ConvTranspose2d")
    for module, layer in ((second, second.blocks[0][0]), (neck, neck.deblocks[0][0])):
        w, v = layer.weight.clone(), layer.weight._version
        module.init_weights()
        assert layer.weight._version > v and not torch.equal(layer.weight, w)
    custom = bt.SECOND(32, [32], [0], [1], init_cfg=dict(type="Constant", layer="Conv2d", val=0.5))
    custom.init_weights()
    assert bool((custom.blocks[0][0].weight == 0.5).all())


# ---- the fold ----------------------------------------------------------------------------------------------------------------------
def half_pair(mode="conv", kernel=3, stride=1, cin=48, cout=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    if mode == "deconv":
        conv = nn.ConvTranspose2d(cin, cout, 2, stride=2, bias=False)
    else:
        conv = nn.Conv2d(cin, cout, kernel, stride=stride, padding=kernel // 2, bias=False)
    bn = nn.BatchNorm2d(cout, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cout, generator=g))
        bn.running_mean.copy_(torch.randn(cout, generator=g))
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.1)
    return conv.half().eval(), bn.half().eval()


@pytest.mark.parametrize("seed", range(8))
def test_scale_and_shift_against_the_float64_formula(seed):
    conv, bn = half_pair(seed=seed)
    fold = bt.fold_bev_layer(conv, bn)
    s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t64 = bn.bias.double() - bn.running_mean.double() * s64
    assert fold.scale.dtype == torch.float32 and fold.shift.dtype == torch.float32 and fold.packed.dtype == torch.float16
    assert ((fold.scale.double() - s64).abs() <= 2.0 ** -21 * s64.abs()).all()
    assert ((fold.shift.double() - t64).abs() <= 2.0 ** -21 * t64.abs()).all()
    assert (fold.in_channels, fold.out_channels, fold.kernel, fold.stride, fold.mode) == (48, 64, 3, 1, "conv")
    assert torch.equal(bt.bev_unpack_weight(fold.packed, 48, 64, 3), conv.weight.detach())


def test_fold_cache_is_reused_and_refreshed():
    conv, bn = half_pair()
    a = bt.fold_bev_layer(conv, bn)
    assert bt.fold_bev_layer(conv, bn) is a
    with torch.no_grad():
        bn.bias.add_(1.0)                                           # an in-place write moves the version
    b = bt.fold_bev_layer(conv, bn)
    assert b is not a and not torch.equal(b.shift, a.shift) and torch.equal(b.scale, a.scale)
    state = {k: v.clone() for k, v in conv.state_dict().items()}
    state["weight"] = state["weight"] * 2
    conv.load_state_dict(state)
    c = bt.fold_bev_layer(conv, bn)
    assert c is not b and torch.equal(bt.bev_unpack_weight(c.packed, 48, 64, 3), state["weight"])


@pytest.mark.parametrize("mode, kernel, cin, cout", [("conv", 1, 32, 32), ("conv", 3, 48, 64), ("conv", 3, 336, 256), ("deconv", 2, 48, 64),
                                                     ("deconv", 2, 256, 256)])
def test_pack_and_unpack_round_trip(mode, kernel, cin, cout):
    shape = (cin, cout, 2, 2) if mode == "deconv" else (cout, cin, kernel, kernel)
    w = torch.arange(cin * cout * kernel * kernel, dtype=torch.float32).reshape(shape).to(torch.bfloat16 if kernel == 1 else torch.float32)
    flat = bt.bev_pack_weight(w, mode)
    nch = -(-cin // 32)
    assert flat.numel() == (4 if mode == "deconv" else 1) * cout * nch * (1 if mode == "deconv" else kernel * kernel) * 32
    assert torch.equal(bt.bev_unpack_weight(flat, cin, cout, kernel, mode), w)


def test_packed_order_names_the_fragment_element():
    cin, cout = 48, 64
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3)
    flat = bt.bev_pack_weight(w).reshape(1, cout // 16, 2, 9, 64, 8)
    for mt, chunk, tap, lane, j in [(0, 0, 0, 0, 0), (3, 0, 5, 37, 6), (1, 1, 8, 15, 7), (2, 1, 4, 63, 0)]:
        ci = 32 * chunk + 8 * (lane >> 4) + j
        want = w[16 * mt + (lane & 15), ci, tap // 3, tap % 3] if ci < cin else 0.0
        assert flat[0, mt, chunk, tap, lane, j] == want
    wd = torch.arange(cin * cout * 4, dtype=torch.float32).reshape(cin, cout, 2, 2)
    fd = bt.bev_pack_weight(wd, "deconv").reshape(4, cout // 16, 2, 1, 64, 8)
    assert fd[3, 2, 0, 0, 21, 3] == wd[8 + 3, 32 + 5, 1, 1] and fd[1, 0, 1, 0, 16, 0] == wd[40, 0, 0, 1]


def test_layer_spec_names_what_the_kernel_serves():
    bn = nn.BatchNorm2d(64).eval()
    assert bt.layer_spec(nn.Conv2d(32, 64, 3, padding=1, bias=False), bn) == ("conv", 3, 1)
    assert bt.layer_spec(nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False), bn) == ("conv", 3, 2)
    assert bt.layer_spec(nn.Conv2d(32, 64, 1, bias=False), bn) == ("conv", 1, 1)
    assert bt.layer_spec(nn.ConvTranspose2d(32, 64, 1, bias=False), bn) == ("conv", 1, 1)
    assert bt.layer_spec(nn.ConvTranspose2d(32, 64, 2, stride=2, bias=False), bn) == ("deconv", 2, 2)
    for conv in (nn.Conv2d(32, 48, 3, padding=1, bias=False), nn.Conv2d(8, 64, 3, padding=1, bias=False), nn.Conv2d(32, 64, 5, padding=2, bias=False),
                 nn.Conv2d(32, 64, 3, padding=1), nn.Conv2d(32, 64, 2, stride=2, bias=False), nn.ConvTranspose2d(32, 64, 4, stride=4, bias=False),
                 nn.Conv2d(32, 64, 3, padding=0, bias=False)):
        assert bt.layer_spec(conv, bn) is None, conv
    assert bt.layer_spec(nn.Conv2d(32, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)) is None        # a BatchNorm in train mode


def test_host_tensors_and_fp32_take_the_torch_layers():
    fuser, second, neck = [m.eval() for m in small_modules()]
    for m in (fuser, second, neck):
        m.use_fused = True
    xs = small_inputs()
    with torch.no_grad():
        assert not fuser.fusable(xs) and not second.fusable(torch.cat(xs, 1)[:, :32]) and not neck.fusable([xs[1], xs[1]])
    conv, bn = half_pair()
    with pytest.raises(RuntimeError, match="GPU tensors"):
        bt.bev_conv_forward([torch.zeros(1, 48, 4, 4, dtype=torch.float16)], bt.fold_bev_layer(conv, bn))


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def _call(lib, c0=16, c1=32, cout=64, kernel=3, stride=1, mode=0, H=5, W=7, batch=2, src=1, packed=1, dst=1, scale=1, src_layout=0,
          dst_layout=0, dtype=0, dst_c=None, dst_off=0, packed_elems=None, dst_elems=None):
    """bevamd_bev_conv_forward with made-up non-null addresses: every case here is refused before any GPU work."""
    taps, groups, up = (1, 4, 2) if mode == 1 else (kernel * kernel, 1, 1)
    OH, OW = (H, W) if mode == 1 else ((H + 2 * (kernel // 2) - kernel) // max(stride, 1) + 1, (W + 2 * (kernel // 2) - kernel) // max(stride, 1) + 1)
    dst_c = cout if dst_c is None else dst_c
    if packed_elems is None:
        packed_elems = groups * cout * (-(-(c0 + c1) // 32)) * taps * 32
    if dst_elems is None:
        dst_elems = batch * dst_c * OH * up * OW * up
    addr = lambda on: ctypes.c_void_p(on * 4096 or None)   # noqa: E731
    return lib.bevamd_bev_conv_forward(addr(src), c0, addr(src if c1 else 0), c1, src_layout, dtype, batch, H, W, cout, kernel, stride, mode,
                                       addr(packed), packed_elems, addr(scale), addr(scale), addr(dst), dst_c, dst_off, dst_layout, dst_elems,
                                       None)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(c0=8), 4, "multiples of 16"),
    (dict(c1=24), 4, "multiples of 16"),
    (dict(cout=48), 4, "multiple of 32"),
    (dict(kernel=5), 4, "kernel 5"),
    (dict(kernel=1, stride=2), 4, "stride 2"),
    (dict(mode=1, kernel=3, stride=1), 4, "mode 1"),
    (dict(mode=1, kernel=2, stride=2, dst_layout=1, dst_c=66), 4, "multiples of 4"),
    (dict(H=0), 1, "bad sizes"),
    (dict(batch=65536), 1, "batch"),
    (dict(dtype=2), 1, "dtype"),
    (dict(src_layout=3), 1, "layouts"),
    (dict(dst_c=96, dst_off=64), 1, "does not fit"),
    (dict(packed_elems=7), 1, "packed holds 7"),
    (dict(dst_elems=5), 1, "dst holds 5"),
    (dict(packed=0), 1, "packed is null"),
    (dict(scale=0), 1, "scale or shift"),
    (dict(src=0), 1, "is null"),
    (dict(dst=0), 1, "is null"),
])
def test_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _call(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_an_empty_batch_is_nothing_to_do():
    assert _call(_capi.load(), batch=0, src=0, dst=0) == 0


def test_binding_table_equals_the_header():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_bev_conv_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_bev_conv_forward"]
    args = protos["bevamd_bev_conv_forward"].split(",")
    res, argtypes = _capi._EXT_SIGNATURES["bevamd_bev_conv_forward"]
    want = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_int for a in args]
    assert res is ctypes.c_int and argtypes == want
    assert "size_t" not in protos["bevamd_bev_conv_forward"]
    assert "bevamd_bev_conv_forward" in _capi.ext_exported_names()


# ---- the code object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(resources.OBJ, "bev_conv.o")) or not all(os.path.exists(t) for t in resources.TOOLS),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_the_kernels_use_no_scratch_spill_nothing_and_fit_two_workgroups():
    kernels = {n: v for n, v in resources._kernels().items() if v["obj"] == "bev_conv"}
    names = sorted(f"void bevamd::bev_conv_kernel<{b}, {mt}, {ks}, {s}>" for b in ("false", "true") for mt in (1, 2, 4)
                   for ks, s in ((3, 1), (3, 2), (1, 1)))
    assert sorted(kernels) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "bev_conv.o"))
    for name in names:
        got = kernels[name]
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= 256, (name, got)                          # two workgroups of four waves per compute unit
        assert 0 < lds[name] and 2 * lds[name] <= 160 * 1024, (name, lds[name])
        want = (7 * int(name[-2]) + int(name[-5])) * (15 * int(name[-2]) + int(name[-5])) * 80      # haloed tile x 80-byte pixels
        assert lds[name] == want, (name, lds[name], want)
