"""The fused Swin block FFN on the host: the packed weight order against a numpy restatement of the header's fragment map, the
fold's cache, `swin_ffn_spec`, the entry point's refusals (before any GPU work), its binding, and the default dispatch."""
import os
import re

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, heads
from bevfusion_amd import cam_swin as cs
from test_cam_swin import SMALL, _randomise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMAX = 192


def _unpack(p1, p2, C, hidden):
    """include/bevfusion_amd_ext.h, bevamd_swin_ffn_forward, restated: where each packed element comes from.  Returns W1, W2 and how
    often each of their elements was named."""
    KS, CT = C // 32, C // 16
    w1, n1 = np.zeros((hidden, C), p1.dtype), np.zeros((hidden, C), np.int64)
    tile, ks, lane, e = np.indices((hidden // 16, KS, 64, 8))
    idx = ((tile * KS + ks) * 64 + lane) * 8 + e
    row, col = 16 * tile + (lane & 15), 32 * ks + 8 * (lane >> 4) + e
    w1[row, col] = p1[idx]
    np.add.at(n1, (row, col), 1)
    w2, n2 = np.zeros((C, hidden), p2.dtype), np.zeros((C, hidden), np.int64)
    s, ct, lane, e = np.indices((hidden // 32, CT, 64, 8))
    idx = ((s * CT + ct) * 64 + lane) * 8 + e
    row, col = 16 * ct + (lane & 15), 32 * s + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3)
    w2[row, col] = p2[idx]
    np.add.at(n2, (row, col), 1)
    return w1, n1, w2, n2


@pytest.mark.parametrize("C", [32, 96, 192])
@pytest.mark.parametrize("hidden", [64, 128, "4C"])
def test_pack_then_unpack_through_the_header_map_returns_the_matrices(C, hidden):
    hidden = 4 * C if hidden == "4C" else hidden
    g = torch.Generator().manual_seed(C + hidden)
    w1 = torch.randperm(hidden * C, generator=g).reshape(hidden, C).float()          # every element distinct, asymmetric
    w2 = torch.randperm(hidden * C, generator=g).reshape(C, hidden).float() + 0.5
    p1, p2 = cs.swin_pack_ffn(w1, w2)
    assert p1.shape == p2.shape == (hidden * C,) and p1.is_contiguous() and p2.is_contiguous()
    u1, n1, u2, n2 = _unpack(p1.numpy(), p2.numpy(), C, hidden)
    assert (n1 == 1).all() and (n2 == 1).all()
    assert np.array_equal(u1, w1.numpy()) and np.array_equal(u2, w2.numpy())


def test_pack_refuses_sizes_without_a_fragment_order():
    with pytest.raises(ValueError):
        cs.swin_pack_ffn(torch.zeros(96, 48), torch.zeros(48, 96))
    with pytest.raises(ValueError):
        cs.swin_pack_ffn(torch.zeros(128, 32), torch.zeros(32, 64))


def test_the_fold_is_cached_and_follows_the_parameters():
    b = _randomise(cs.SwinBlock(32, 1, 64), 2).half()
    f = cs.fold_swin_ffn(b.norm2, b.ffn)
    assert cs.fold_swin_ffn(b.norm2, b.ffn) is f and len(f) == 6
    p1, p2, gamma, beta, b1, b2 = f
    assert p1.dtype == p2.dtype == torch.float16 and all(t.dtype == torch.float32 for t in (gamma, beta, b1, b2))
    fc1, fc2 = b.ffn.layers[0][0], b.ffn.layers[1]
    assert torch.equal(gamma, b.norm2.weight.float()) and torch.equal(beta, b.norm2.bias.float())
    assert torch.equal(b1, fc1.bias.float()) and torch.equal(b2, fc2.bias.float())
    u1, _, u2, _ = _unpack(p1.numpy(), p2.numpy(), 32, 64)
    assert np.array_equal(u1, fc1.weight.detach().numpy()) and np.array_equal(u2, fc2.weight.detach().numpy())
    with torch.no_grad():
        fc2.bias.add_(1.0)                                          # an in-place update moves the version
    g = cs.fold_swin_ffn(b.norm2, b.ffn)
    assert g is not f and torch.equal(g[5], fc2.bias.float()) and not torch.equal(g[5], b2)
    b.load_state_dict({k: torch.zeros_like(v) for k, v in b.state_dict().items()})
    z = cs.fold_swin_ffn(b.norm2, b.ffn)
    assert z is not g and not z[0].any() and not z[2].any()
    assert cs.fold_swin_ffn(cs.SwinBlock(48, 2, 96).norm2, cs.SwinBlock(48, 2, 96).ffn) is None


def test_spec():
    assert cs.swin_ffn_spec(cs.SwinBlock(96, 3, 384))
    assert cs.swin_ffn_spec(cs.SwinBlock(CMAX, 6, 4 * CMAX)) and cs.swin_ffn_spec(cs.SwinBlock(32, 1, 96))
    assert not cs.swin_ffn_spec(cs.SwinBlock(96, 3, 384, act_cfg=dict(type="ReLU")))
    three = cs.SwinBlock(96, 3, 384)
    three.ffn = cs.FFN(96, 384, num_fcs=3, act_cfg=dict(type="GELU"))
    assert not cs.swin_ffn_spec(three)
    assert not cs.swin_ffn_spec(cs.SwinBlock(48, 2, 192))
    assert not cs.swin_ffn_spec(cs.SwinBlock(CMAX + 32, 7, 4 * (CMAX + 32)))
    assert not cs.swin_ffn_spec(cs.SwinBlock(96, 3, 100)) and not cs.swin_ffn_spec(cs.SwinBlock(CMAX, 6, 4 * CMAX + 32))
    tanh = cs.SwinBlock(96, 3, 384)
    tanh.ffn.layers[0][1] = torch.nn.GELU(approximate="tanh")
    assert not cs.swin_ffn_spec(tanh)
    no_identity = cs.SwinBlock(96, 3, 384)
    no_identity.ffn.add_identity = False
    assert not cs.swin_ffn_spec(no_identity)
    plain = cs.SwinBlock(96, 3, 384)
    plain.norm2 = torch.nn.LayerNorm(96, elementwise_affine=False)
    assert not cs.swin_ffn_spec(plain)
    assert cs.KERNEL_FFN_CMAX == CMAX


NAMES = ["x", "x_elems", "gamma", "gamma_elems", "beta", "beta_elems", "packed1", "packed1_elems", "b1", "b1_elems", "packed2",
         "packed2_elems", "b2", "b2_elems", "dtype", "tokens", "channels", "hidden", "eps", "out", "out_elems"]
POINTERS = ["x", "gamma", "beta", "packed1", "b1", "packed2", "b2", "out"]


def _refuse(T=10, C=96, hidden=384, **kw):
    """bevamd_swin_ffn_forward with made-up non-null addresses: every case here is refused (or has nothing to do) before any GPU
    work."""
    a = dict(x=1 << 30, x_elems=T * C, gamma=3 << 30, gamma_elems=C, beta=(3 << 30) + 4096, beta_elems=C, packed1=4 << 30,
             packed1_elems=hidden * C, b1=5 << 30, b1_elems=hidden, packed2=6 << 30, packed2_elems=hidden * C, b2=7 << 30, b2_elems=C,
             dtype=0, tokens=T, channels=C, hidden=hidden, eps=1e-5, out=2 << 30, out_elems=T * C)
    a.update(kw)
    return _capi.load().bevamd_swin_ffn_forward(*[a[n] for n in NAMES], None)


def test_entry_point_refusals_before_any_gpu_work():
    assert _refuse(C=48, hidden=192) == 4 and "48 channels" in _capi.last_error()
    assert _refuse(hidden=100) == 4 and "100 hidden" in _capi.last_error()
    assert _refuse(C=CMAX + 32, hidden=4 * CMAX) == 4 and f"{CMAX + 32} channels" in _capi.last_error()
    assert _refuse(C=CMAX, hidden=4 * CMAX + 32) == 4 and _refuse(C=0, hidden=0) == 4 and _refuse(hidden=0) == 4
    assert _refuse(dtype=2) == 1 and _refuse(dtype=-1) == 1
    assert _refuse(eps=0.0) == 1 and "eps" in _capi.last_error()
    assert _refuse(eps=float("nan")) == 1 and _refuse(eps=float("inf")) == 1 and _refuse(eps=-1e-5) == 1
    assert _refuse(tokens=-1, x_elems=-96, out_elems=-96) == 1
    good = dict(x_elems=960, out_elems=960, gamma_elems=96, beta_elems=96, b2_elems=96, b1_elems=384, packed1_elems=36864,
                packed2_elems=36864)
    assert sorted(good) == sorted(n for n in NAMES if n.endswith("_elems"))
    for name, count in good.items():
        assert _refuse(**{name: count - 1}) == 1 and "hold" in _capi.last_error(), name
        assert _refuse(**{name: count + 1}) == 1 and "hold" in _capi.last_error(), name
    for name in POINTERS:
        assert _refuse(**{name: None}) == 1 and "null" in _capi.last_error(), name
    for name in POINTERS:
        step = 4 if name in ("gamma", "beta", "b1", "b2") else 8
        assert _refuse(**{name: (9 << 30) + step}) == 1 and "aligned" in _capi.last_error(), name
    assert _refuse(out=(1 << 30) + 64) == 1 and "overlaps x" in _capi.last_error()
    assert _refuse(out=(1 << 30) - 64) == 1 and "overlaps x" in _capi.last_error()
    assert _refuse(out=(4 << 30) + 1024) == 1 and "overlaps" in _capi.last_error()
    assert _refuse(out=(5 << 30) - 16 * 60) == 1 and "overlaps" in _capi.last_error()
    assert _refuse(T=0, x=None, out=None) == 0                      # nothing to do
    assert _refuse(T=0, x=None, out=None, dtype=1, C=32, hidden=64) == 0
    assert _refuse(T=0, x=None, out=None, packed1=None) == 1      # the operands are checked all the same


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_swin_ffn\w*)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_swin_ffn_forward"]
    proto = protos["bevamd_swin_ffn_forward"]
    args = [a.strip() for a in proto.split(",")]
    res, argtypes = _capi._EXT_SIGNATURES["bevamd_swin_ffn_forward"]
    assert res is _capi.I and len(args) == len(argtypes) == len(NAMES) + 1
    assert "size_t" not in proto
    for a, t, name in zip(args, argtypes, NAMES + ["stream"]):
        want = _capi.P if "*" in a else _capi.LL if a.startswith("long long") else _capi.c_float if a.startswith("float") else _capi.I
        assert t is want and re.search(r"\b%s$" % name, a), (a, t, name)
    # every pointer but the stream is followed by its extent in elements
    for i, a in enumerate(args[:-1]):
        if "*" in a:
            assert args[i + 1].startswith("long long") and args[i + 1].endswith("_elems"), a
    assert not any(n.startswith("bevamd_window_attention_") for n in protos)


def test_defaults_run_the_torch_ffn(monkeypatch):
    assert cs.SwinTransformer.fused_ffn_stages == ()
    calls = []
    real = cs.FFN.forward

    def counting(self, x, identity=None):
        calls.append(self)
        return real(self, x, identity)
    monkeypatch.setattr(cs.FFN, "forward", counting)
    monkeypatch.setattr(cs, "_swin_ffn_served", lambda *a, **k: pytest.fail("the fused FFN ran under default attributes"))
    net = _randomise(cs.SwinTransformer(**SMALL), 3).eval()
    assert net.fused_ffn_stages == ()
    with torch.no_grad():
        net(torch.randn(1, 3, 28, 28))
        assert len(calls) == sum(SMALL["depths"])
        blk = net.stages[0].blocks[0]
        x = torch.randn(1, 49, 32)
        assert torch.equal(blk(x, (7, 7)), blk(x, (7, 7), False, False)) and len(calls) == sum(SMALL["depths"]) + 2
    # on a host tensor the setting is not consulted: `fusable` is false there
    net.fused_ffn_stages = (0, 1)
    with torch.no_grad():
        net(torch.randn(1, 3, 28, 28))
    assert len(calls) == 2 * sum(SMALL["depths"]) + 2


def test_the_op_raises_on_host_tensors_and_is_re_exported():
    b = cs.SwinBlock(96, 3, 384).half()
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cs.swin_ffn(torch.zeros(4, 96, dtype=torch.float16), b.norm2, b.ffn)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        cs.swin_ffn(None, b.norm2, b.ffn)
    for n in ("swin_ffn", "fold_swin_ffn", "swin_ffn_spec", "swin_pack_ffn"):
        assert n in cs.__all__ and n in heads.__all__ and getattr(heads, n) is getattr(cs, n)
