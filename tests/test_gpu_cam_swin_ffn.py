"""`cam_swin.SwinTransformer` with `fused_ffn_stages` on the device: the blocks of the listed stages end in one launch of
`bevamd_swin_ffn_forward`.  The small model of tests/test_cam_swin.py (C = 32 and 64, hidden 128 and 256) against the float64
restatement of tests/swin_reference.py; graph capture; a stage the kernel refuses; dispatch; the default.

The bar is the ratio bar of test_gpu_cam_swin.py: per output level the error is at most 2 x the torch layers' own (`use_fused =
False`).  The figures are appended to profiles/swin_ffn_observed.json."""
import copy
import json
import os

import pytest
import torch

import swin_reference as ref
from bevfusion_amd import cam_swin as cs
from conftest import record_parity
from test_cam_swin import SMALL, _randomise
from test_gpu_cam_swin import _image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]


def _net(dtype, dev, stages=(0, 1), **cfg):
    net = _randomise(cs.SwinTransformer(**dict(SMALL, **cfg)), 3).to(dtype).to(dev).eval()
    net.fused_ffn_stages = stages
    return net


def _errors(net, x, cfg):
    """Per level: (error of net(x), error of the torch layers of the same module), both over the reference's largest value."""
    plain = copy.deepcopy(net)
    plain.use_fused = False
    with torch.no_grad():
        assert net.fusable(x) and not plain.fusable(x)
        got, torch_outs = net(x), plain(x)
    want = ref.swin_forward({k: v.cpu() for k, v in net.state_dict().items()}, x.cpu(), cfg["depths"], cfg["num_heads"],
                            cfg["out_indices"])
    out = []
    for g, t, w in zip(got, torch_outs, want):
        top = w.abs().max().item()
        out.append(((g.cpu().double() - w).abs().max().item() / top, (t.cpu().double() - w).abs().max().item() / top))
    return out


def _count_ffn_launches(net, x, monkeypatch):
    calls = []
    real = cs._swin_ffn_served

    def counting(*a, **k):
        y = real(*a, **k)
        calls.append(y is not None)
        return y
    monkeypatch.setattr(cs, "_swin_ffn_served", counting)
    with torch.no_grad():
        outs = net(x)
    monkeypatch.setattr(cs, "_swin_ffn_served", real)
    return outs, calls


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_error_is_within_twice_the_torch_layers_own(dev, dtype, monkeypatch):
    net = _net(dtype, dev)
    x = _image().to(dtype).to(dev)
    _, calls = _count_ffn_launches(net, x, monkeypatch)
    assert calls == [True] * sum(SMALL["depths"])                   # every block's tail went through the kernel
    figures = {}
    for i, (e_fused, e_torch) in enumerate(_errors(net, x, SMALL)):
        print(f"{dtype} level {i}: fused attention + FFN {e_fused:.3e}, torch layers {e_torch:.3e}, ratio {e_fused / e_torch:.3f}")
        record_parity(f"cam_swin_ffn/level{i}/{dtype}", e_fused, 2 * e_torch)
        figures[f"level{i}"] = dict(fused=e_fused, torch_layers=e_torch, ratio=e_fused / e_torch, bar_ratio=2.0)
    path = os.path.join(ROOT, "profiles", "swin_ffn_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.setdefault("swin_small_end_to_end_fused_ffn", {})[str(dtype)] = figures
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass      # a read-only checkout: the figures are printed above
    for v in figures.values():
        assert v["fused"] <= 2 * v["torch_layers"], figures


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_the_eval_forward_replays_from_a_graph_to_the_eager_bits(dev, dtype):
    net = _net(dtype, dev)
    static = _image().to(dtype).to(dev)
    with torch.no_grad():
        eager = [t.clone() for t in net(static)]                   # the warm-up forward: the folds exist now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = net(static)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(c, e) for c, e in zip(captured, eager))
        static.copy_(_image(9).to(dtype))
        graph.replay()
        torch.cuda.synchronize()
        other = net(static)
    assert all(torch.equal(c, o) for c, o in zip(captured, other)) and not any(torch.equal(o, e) for o, e in zip(other, eager))


@pytest.mark.parametrize("how", ["relu", "wide"])
def test_a_stage_the_kernel_refuses_runs_its_torch_ffn_inside_the_model(dev, how, monkeypatch):
    """`fused_ffn_stages = (0,)` on a model whose first stage the kernel does not serve: a ReLU FFN, or a hidden width of 896 (past
    the 768 it is built for)."""
    cfg = dict(act_cfg=dict(type="ReLU")) if how == "relu" else dict(mlp_ratio=28)          # hidden 896 > 768 at C = 32
    net = _net(torch.float16, dev, stages=(0,), **cfg)
    x = _image().half().to(dev)
    assert not any(cs.swin_ffn_spec(b) for b in net.stages[0].blocks)
    _, calls = _count_ffn_launches(net, x, monkeypatch)
    assert calls == []                                              # the spec keeps such a block off the op
    blk = net.stages[0].blocks[0]
    assert cs.swin_ffn(torch.zeros(1, 9, 32, dtype=torch.float16, device=dev), blk.norm2, blk.ffn) is None
    with torch.no_grad():
        tail = blk(torch.zeros(1, 49, 32, dtype=torch.float16, device=dev), (7, 7), True, True)   # asked for, refused, torch layers
    assert tail.shape == (1, 49, 32) and torch.isfinite(tail).all()
    for e_fused, e_torch in _errors(net, x, dict(SMALL, **cfg)) if how == "wide" else []:
        assert e_fused <= 2 * e_torch
    # every tail was refused, so the bits are those of the model that never asks (for the ReLU model the float64 restatement, which
    # has the GELU, does not apply)
    never = copy.deepcopy(net)
    never.fused_ffn_stages = ()
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(net(x), never(x)))


@pytest.mark.parametrize("how", ["train", "fp32", "requires_grad", "use_fused_false"])
def test_the_setting_is_ignored_off_the_fused_path_and_gradients_reach_every_parameter(dev, how, monkeypatch):
    dtype = torch.float32 if how == "fp32" else torch.float16
    net = _net(dtype, dev, drop_path_rate=0.0)
    x = _image().to(dtype).to(dev)
    if how == "train":
        net.train()
    elif how == "use_fused_false":
        net.use_fused = False
    elif how == "requires_grad":
        x.requires_grad_(True)
    monkeypatch.setattr(cs, "_swin_ffn_served", lambda *a, **k: pytest.fail("the fused FFN ran off the fused path"))
    assert not net.fusable(x)
    outs = net(x)
    assert all(o.is_contiguous() and o.requires_grad for o in outs)
    sum(o.float().square().mean() for o in outs).backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all() or not p.grad.any()]
    assert not missing, missing


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_the_default_is_the_explicit_false_bit_for_bit(dev, dtype, monkeypatch):
    net = _net(dtype, dev, stages=())
    assert cs.SwinTransformer.fused_ffn_stages == () and net.fused_ffn_stages == ()
    x = _image().to(dtype).to(dev)
    outs, calls = _count_ffn_launches(net, x, monkeypatch)
    assert calls == []
    other = copy.deepcopy(net)
    for stage in other.stages:
        for blk in stage.blocks:
            fwd = blk.forward
            blk.forward = lambda t, hw, fused=False, fused_ffn=False, fwd=fwd: fwd(t, hw, fused, fused_ffn=False)
    other.fused_ffn_stages = (0, 1)                                 # asked for at the model, switched off at every block
    with torch.no_grad():
        assert other.fusable(x)
        explicit = other(x)
    assert all(torch.equal(a, b) for a, b in zip(outs, explicit))
    fused = _net(dtype, dev)                                        # and the setting does change the bits when it is on
    with torch.no_grad():
        assert not all(torch.equal(a, b) for a, b in zip(outs, fused(x)))
