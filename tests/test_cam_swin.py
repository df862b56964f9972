"""`cam_swin` on the host: the registry entry and the reference YAML's backbone dict, mmdet's state-dict names, the torch path against
the float64 restatement of tests/swin_reference.py, the relative position index, PatchMerging on odd sizes, `swin_convert`, the
training behaviour, the refusals, the entry point's binding."""
import builtins
import os
import re

import pytest
import torch
from torch import nn

import swin_reference as ref
from bevfusion_amd import _capi, heads, registry
from bevfusion_amd import cam_swin as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# encoders.camera.backbone of the reference's Swin-T configs
SWIN_T = dict(type="SwinTransformer", embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4,
              qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2, patch_norm=True, out_indices=[1, 2, 3],
              with_cp=False, convert_weights=True,
              init_cfg=dict(type="Pretrained",
                            checkpoint="https://github.com/SwinTransformer/storage/releases/download/v1.0.0/swin_tiny_patch4_window7_224.pth"))
SMALL = dict(embed_dims=32, depths=[2, 2], num_heads=[1, 2], out_indices=[0, 1], drop_path_rate=0.2)


def _randomise(module, seed):
    """Every parameter away from its initial value: LayerNorm weights and biases, Linear biases and the bias tables included."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * fan_in ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(0.8 + 0.4 * torch.rand(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return module


def _expected_keys(embed, depths, num_heads, out_indices, mlp_ratio=4, in_channels=3, patch=4, ws=7):
    keys = {"patch_embed.projection.weight": (embed, in_channels, patch, patch), "patch_embed.projection.bias": (embed,),
            "patch_embed.norm.weight": (embed,), "patch_embed.norm.bias": (embed,)}
    c = embed
    for i, depth in enumerate(depths):
        for j in range(depth):
            p = f"stages.{i}.blocks.{j}"
            for n in ("norm1", "norm2"):
                keys[f"{p}.{n}.weight"] = keys[f"{p}.{n}.bias"] = (c,)
            keys[f"{p}.attn.w_msa.relative_position_bias_table"] = ((2 * ws - 1) ** 2, num_heads[i])
            keys[f"{p}.attn.w_msa.relative_position_index"] = (ws * ws, ws * ws)
            keys[f"{p}.attn.w_msa.qkv.weight"], keys[f"{p}.attn.w_msa.qkv.bias"] = (3 * c, c), (3 * c,)
            keys[f"{p}.attn.w_msa.proj.weight"], keys[f"{p}.attn.w_msa.proj.bias"] = (c, c), (c,)
            keys[f"{p}.ffn.layers.0.0.weight"], keys[f"{p}.ffn.layers.0.0.bias"] = (mlp_ratio * c, c), (mlp_ratio * c,)
            keys[f"{p}.ffn.layers.1.weight"], keys[f"{p}.ffn.layers.1.bias"] = (c, mlp_ratio * c), (c,)
        if i in out_indices:
            keys[f"norm{i}.weight"] = keys[f"norm{i}.bias"] = (c,)
        if i < len(depths) - 1:
            keys[f"stages.{i}.downsample.norm.weight"] = keys[f"stages.{i}.downsample.norm.bias"] = (4 * c,)
            keys[f"stages.{i}.downsample.reduction.weight"] = (2 * c, 4 * c)
            c *= 2
    return keys


def test_registered_and_re_exported():
    assert registry.BACKBONES.get("SwinTransformer") is cs.SwinTransformer
    assert all(getattr(heads, n) is getattr(cs, n) and n in heads.__all__ for n in cs.__all__)


def test_the_reference_config_builds_with_mmdet_state_dict_names():
    net = registry.build_from_cfg(dict(SWIN_T), registry.BACKBONES)
    assert isinstance(net, cs.SwinTransformer) and net.convert_weights and net.init_cfg["type"] == "Pretrained"
    sd = net.state_dict()
    want = _expected_keys(96, SWIN_T["depths"], SWIN_T["num_heads"], SWIN_T["out_indices"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(net.num_features) == [96, 192, 384, 768]
    # a checkpoint's encoders.camera.backbone.* loads strictly
    ckpt = {"encoders.camera.backbone." + k: torch.zeros(s, dtype=sd[k].dtype) for k, s in want.items()}
    own = {k[len("encoders.camera.backbone."):]: v for k, v in ckpt.items()}
    net.load_state_dict(own, strict=True)
    rates = [m.drop_prob for m in net.modules() if isinstance(m, cs.DropPath)]
    assert len(rates) == 24 and rates[0] == rates[1] == 0.0 and rates[-1] == pytest.approx(0.2)
    assert rates[2] == pytest.approx(0.2 / 11) and rates[::2] == sorted(rates[::2])          # linspace over the 12 blocks


def test_relative_position_index_is_the_formula():
    w = cs.WindowMSA(32, 1, (7, 7))
    idx = w.relative_position_index
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (49, 49) and "relative_position_index" in w.state_dict()
    for i in (0, 5, 13, 24, 48):
        for j in (0, 6, 7, 30, 48):
            yi, xi, yj, xj = i // 7, i % 7, j // 7, j % 7
            assert idx[i, j].item() == (yi - yj + 6) * 13 + (xi - xj + 6)
    assert idx.min().item() == 0 and idx.max().item() == 168


def test_torch_path_equals_the_float64_restatement():
    net = _randomise(cs.SwinTransformer(**SMALL), 3).eval()
    img = torch.randn(2, 3, 40, 72, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        assert not net.fusable(img)
        got = net(img)
    want = ref.swin_forward(net.state_dict(), img, SMALL["depths"], SMALL["num_heads"], SMALL["out_indices"])
    assert [tuple(g.shape) for g in got] == [(2, 32, 10, 18), (2, 64, 5, 9)]            # both maps pad to the window, the first merges evenly
    for g, w in zip(got, want):
        assert g.is_contiguous() and (g.double() - w).abs().max().item() <= 1e-5 * w.abs().max().item()


def test_a_checkpoint_index_buffer_rules():
    """The fold and the torch path read the module's index buffer: a permuted buffer changes the bias both see."""
    w = _randomise(cs.WindowMSA(32, 1, (7, 7)), 5)
    a = cs.fold_window_bias(w)
    assert cs.fold_window_bias(w) is a and tuple(a.shape) == (1, 49, 49) and a.dtype == torch.float32
    assert torch.equal(a[0], w.relative_position_bias_table[w.relative_position_index.view(-1)].view(49, 49, 1)[..., 0])
    with torch.no_grad():
        w.relative_position_index.copy_(w.relative_position_index.flip(0))
    b = cs.fold_window_bias(w)
    assert b is not a and torch.equal(b[0], a[0].flip(0))
    with torch.no_grad():
        w.relative_position_bias_table.mul_(2.0)
    assert torch.equal(cs.fold_window_bias(w)[0], 2 * b[0])


@pytest.mark.parametrize("hw", [(5, 7), (6, 9), (1, 1)])
def test_patch_merging_on_odd_sizes(hw):
    m = _randomise(cs.PatchMerging(8, 16), 6).double()
    x = torch.randn(2, hw[0] * hw[1], 8, dtype=torch.float64)
    got, out_hw = m(x, hw)
    want, want_hw = ref.patch_merging(x, hw, {"d." + k: v for k, v in m.state_dict().items()}, "d")
    assert tuple(out_hw) == tuple(want_hw) == (-(-hw[0] // 2), -(-hw[1] // 2))
    assert (got - want).abs().max().item() <= 1e-12
    assert m.reduction.bias is None and tuple(m.norm.normalized_shape) == (32,)


def test_patch_embed_pads_the_corner():
    m = cs.PatchEmbed(3, 8, 4, 4, dict(type="LN")).double()
    x = torch.randn(1, 3, 9, 6, dtype=torch.float64)
    y, hw = m(x)
    assert tuple(hw) == (3, 2) and tuple(y.shape) == (1, 6, 8)
    full = torch.zeros(1, 3, 12, 8, dtype=torch.float64)
    full[:, :, :9, :6] = x
    assert torch.equal(m(full)[0], y)


def _official_forward(sd, x, hw):
    """The official implementation's PatchMerging: cat of x0 .. x3, LayerNorm, Linear."""
    B, L, C = x.shape
    x = x.view(B, hw[0], hw[1], C)
    x0, x1, x2, x3 = x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]
    x = torch.cat([x0, x1, x2, x3], -1).view(B, -1, 4 * C)
    x = nn.functional.layer_norm(x, (4 * C,), sd["layers.0.downsample.norm.weight"], sd["layers.0.downsample.norm.bias"])
    return nn.functional.linear(x, sd["layers.0.downsample.reduction.weight"])


def test_swin_convert_renames_reorders_and_loads_strictly():
    net = _randomise(cs.SwinTransformer(**SMALL), 8).double()
    own = net.state_dict()
    g = torch.Generator().manual_seed(9)
    official = {}
    for k, v in own.items():                                     # the official names of this architecture, fresh values
        ok = k.replace("stages.", "layers.").replace("attn.w_msa.", "attn.").replace("ffn.layers.0.0.", "mlp.fc1.") \
            .replace("ffn.layers.1.", "mlp.fc2.").replace("patch_embed.projection", "patch_embed.proj")
        official[ok] = v.clone() if not v.is_floating_point() else torch.randn(v.shape, generator=g, dtype=torch.float64)
    official["head.weight"], official["head.bias"] = torch.zeros(10, 64), torch.zeros(10)
    official["layers.0.blocks.1.attn_mask"] = torch.zeros(4, 49, 49)
    conv = cs.swin_convert(official)
    assert set(conv) == set(own) and not any(k.startswith("head") for k in conv)
    net.load_state_dict(conv, strict=True)
    assert torch.equal(net.stages[0].blocks[1].ffn.layers[0][0].weight, official["layers.0.blocks.1.mlp.fc1.weight"])
    assert torch.equal(net.stages[1].blocks[0].attn.w_msa.qkv.bias, official["layers.1.blocks.0.attn.qkv.bias"])
    assert torch.equal(net.patch_embed.projection.weight, official["patch_embed.proj.weight"])
    x = torch.randn(2, 6 * 8, 32, dtype=torch.float64, generator=g)
    got, hw = net.stages[0].downsample(x, (6, 8))
    assert tuple(hw) == (3, 4) and (got - _official_forward(official, x, (6, 8))).abs().max().item() <= 1e-12


def test_frozen_stages_and_train():
    net = cs.SwinTransformer(frozen_stages=1, **SMALL)
    frozen = [net.patch_embed, net.stages[0], net.norm0]
    assert all(not p.requires_grad for m in frozen for p in m.parameters())
    assert all(p.requires_grad for p in net.stages[1].parameters()) and all(p.requires_grad for p in net.norm1.parameters())
    net.train()
    assert net.training and net.stages[1].training and not any(m.training for m in frozen) and not net.drop_after_pos.training
    assert cs.SwinTransformer(**SMALL).train().patch_embed.training


def test_drop_path_is_the_identity_in_eval_and_drops_samples_in_training():
    d = cs.DropPath(0.5)
    x = torch.ones(64, 3, 2)
    assert d.eval()(x) is x
    torch.manual_seed(0)
    y = d.train()(x)
    per = y.reshape(64, -1)
    assert all(v in (0.0, 2.0) for v in per[:, 0].tolist()) and 0 < (per[:, 0] == 0).sum().item() < 64
    assert (per == per[:, :1]).all()                              # a sample is kept or dropped whole
    net = _randomise(cs.SwinTransformer(**SMALL), 10)
    img = torch.randn(1, 3, 28, 28)
    with torch.no_grad():
        a, b = net.eval()(img), net.eval()(img)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_unsupported_arguments_raise():
    with pytest.raises(NotImplementedError):
        cs.SwinTransformer(use_abs_pos_embed=True, **SMALL)
    with pytest.raises(NotImplementedError):
        cs.SwinTransformer(with_cp=True, **SMALL)
    with pytest.raises(AssertionError):
        cs.SwinTransformer(pretrained="a.pth", init_cfg=dict(type="Pretrained", checkpoint="b.pth"), **SMALL)


def test_pretrained_opens_nothing(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError(f"opened {a}")
    monkeypatch.setattr(builtins, "open", refuse)
    monkeypatch.setattr(torch, "load", refuse)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    net = cs.SwinTransformer(pretrained="https://example.invalid/swin.pth", convert_weights=True, **SMALL)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.init_weights()
    assert net.init_cfg == dict(type="Pretrained", checkpoint="https://example.invalid/swin.pth")
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def test_host_and_fp32_tensors_are_refused_by_the_op_and_take_the_torch_path():
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cs.window_attention(torch.zeros(1, 7, 7, 96, dtype=torch.float16), torch.zeros(1, 49, 49), 1.0, 0)
    net = cs.SwinTransformer(**SMALL).eval()
    assert not net.fusable(torch.zeros(1, 3, 28, 28)) and not net.half().fusable(torch.zeros(1, 3, 28, 28, dtype=torch.float16))
    assert cs.window_attention_spec(net.stages[0].blocks[1].attn)
    assert not cs.window_attention_spec(cs.SwinBlock(48, 2, 96).attn)                         # heads of 24
    assert not cs.window_attention_spec(cs.SwinBlock(32, 1, 64, window_size=8).attn)


def _refuse(**kw):
    """bevamd_window_attention_forward with made-up non-null addresses: every case here is refused before any GPU work."""
    a = dict(qkv=1 << 30, qkv_elems=2 * 8 * 10 * 192, pad=None, pad_elems=0, bias=3 << 30, bias_elems=2 * 2401, dtype=0, batch=2, H=8,
             W=10, C=64, heads=2, window=7, hd=32, scale=0.17, shift=3, out=2 << 30, out_elems=2 * 8 * 10 * 64)
    a.update(kw)
    return _capi.load().bevamd_window_attention_forward(a["qkv"], a["qkv_elems"], a["pad"], a["pad_elems"], a["bias"], a["bias_elems"],
                                                        a["dtype"], a["batch"], a["H"], a["W"], a["C"], a["heads"], a["window"], a["hd"],
                                                        a["scale"], a["shift"], a["out"], a["out_elems"], None)


def test_entry_point_refusals_before_any_gpu_work():
    assert _refuse(window=8) == 4 and "window 8" in _capi.last_error()
    assert _refuse(hd=16) == 4
    assert _refuse(dtype=2) == 1
    assert _refuse(shift=7) == 1 and _refuse(shift=-1) == 1
    assert _refuse(C=96) == 1                                      # not heads * 32
    assert _refuse(qkv_elems=2 * 8 * 10 * 192 - 1) == 1 and "qkv holds" in _capi.last_error()
    assert _refuse(out_elems=2 * 8 * 10 * 64 + 1) == 1 and "out holds" in _capi.last_error()
    assert _refuse(bias_elems=2401) == 1
    assert _refuse(pad=5 << 30, pad_elems=0) == 1 and _refuse(pad=None, pad_elems=192) == 1
    assert _refuse(qkv=None) == 1 and _refuse(out=None) == 1 and _refuse(bias=None) == 1
    assert _refuse(qkv=(1 << 30) + 8) == 1 and _refuse(out=(2 << 30) + 4) == 1 and _refuse(pad=(5 << 30) + 8, pad_elems=192) == 1
    assert _refuse(out=(1 << 30) + 1024) == 1 and "overlaps" in _capi.last_error()
    assert _refuse(scale=float("nan")) == 1
    assert _refuse(batch=0, qkv=None, out=None, qkv_elems=0, out_elems=0) == 0          # nothing to do


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_window_attention_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_window_attention_forward"]
    args = protos["bevamd_window_attention_forward"].split(",")
    res, argtypes = _capi._EXT_SIGNATURES["bevamd_window_attention_forward"]
    assert len(args) == len(argtypes) == 19
    assert "size_t" not in protos["bevamd_window_attention_forward"]
    for a, t in zip(args, argtypes):
        a = a.strip()
        want = _capi.P if "*" in a else _capi.LL if a.startswith("long long") else _capi.c_float if a.startswith("float") else _capi.I
        assert t is want, (a, t)
