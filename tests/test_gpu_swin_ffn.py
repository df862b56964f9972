"""`bevamd_swin_ffn_forward` on the device (through `cam_swin.swin_ffn`): LayerNorm, fc1, GELU, fc2 and the residual of a Swin block
in one launch, against the float64 restatement of tests/swin_ffn_reference.py on the same 16-bit inputs.

Shapes: T in {1, 15, 16, 17, 63, 65, 129, 323} (a wave owns 32 tokens = two MFMA tiles of 16: tails of a tile, of a wave, several
workgroups plus a tail), C in {32, 96, 192} with hidden = 4 C, and C = 32 with hidden 64 and 96 (one k-step of the second product,
an odd number of them).  A token's result depends on its own row alone, so ONE reference of 323 rows per (C, hidden, dtype) serves
every T.

The bar is the project's ratio bar for chains (test_gpu_bev_trunk.py, test_gpu_cam_swin.py): max |op - ref| / max |ref| is at most
twice the same figure of the torch sequence (LayerNorm, Linear, GELU, Linear, add) on the device in the same dtype.  Both figures
are recorded and written to profiles/swin_ffn_observed.json."""
import json
import os

import pytest
import torch

import swin_ffn_reference as ref
from bevfusion_amd import cam_swin as cs
from conftest import record_parity
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
TOKENS = [1, 15, 16, 17, 63, 65, 129, 323]
SHAPES = [(32, 128), (96, 384), (192, 768), (32, 64), (32, 96)]
TMAX = max(TOKENS)
_CASES = {}
_OBSERVED = {}


def make_block(C, hidden, dtype, seed, eps=1e-5):
    """A SwinBlock whose FFN term is as large as its residual: fc1 rows of norm 1.5, fc2 rows of norm 2.5, every vector non-trivial."""
    g = torch.Generator().manual_seed(seed)
    blk = cs.SwinBlock(C, max(C // 32, 1), hidden)
    fc1, fc2 = blk.ffn.layers[0][0], blk.ffn.layers[1]
    with torch.no_grad():
        blk.norm2.weight.copy_(0.8 + 0.4 * torch.rand(C, generator=g))
        blk.norm2.bias.copy_(0.3 * torch.randn(C, generator=g))
        fc1.weight.copy_(torch.randn(hidden, C, generator=g) * 1.5 * C ** -0.5)
        fc1.bias.copy_(0.3 * torch.randn(hidden, generator=g))
        fc2.weight.copy_(torch.randn(C, hidden, generator=g) * 2.5 * hidden ** -0.5)
        fc2.bias.copy_(0.3 * torch.randn(C, generator=g))
    blk.norm2.eps = eps
    return blk.to(dtype).eval()


def torch_tail(blk, x):
    return blk.ffn(blk.norm2(x), identity=x)


def _case(C, hidden, dtype, dev):
    """The block on the device, its 323 input rows, their float64 reference, the torch sequence's output."""
    key = (C, hidden, dtype)
    if key not in _CASES:
        blk = make_block(C, hidden, dtype, 100 + C + hidden)
        x = torch.randn(TMAX, C, generator=torch.Generator().manual_seed(7 + C)).to(dtype)
        want = ref.module_forward(x, blk.norm2, blk.ffn)
        # a condition on the inputs, not a tolerance: the FFN term is not hidden under the residual
        assert (want - x.double()).abs().max().item() >= 0.5 * x.double().abs().max().item()
        blk = blk.to(dev)
        xd = x.to(dev)
        with torch.no_grad():
            plain = torch_tail(blk, xd).cpu().double()
        _CASES[key] = (blk, xd, want, plain)
    return _CASES[key]


def _write_observed():
    path = os.path.join(ROOT, "profiles", "swin_ffn_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.setdefault("swin_ffn_op", {}).update(_OBSERVED)
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass      # a read-only checkout: the figures are printed


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("C,hidden", SHAPES)
def test_error_is_within_twice_the_torch_sequence_own(dev, C, hidden, dtype):
    blk, x, want, plain = _case(C, hidden, dtype, dev)
    figures = {}
    with torch.no_grad():
        for T in TOKENS:
            got = cs.swin_ffn(x[:T].contiguous(), blk.norm2, blk.ffn)
            assert got is not None and got.shape == (T, C) and got.dtype == dtype
            top = want[:T].abs().max().item()
            e_op = (got.cpu().double() - want[:T]).abs().max().item() / top
            e_torch = (plain[:T] - want[:T]).abs().max().item() / top
            print(f"C {C} hidden {hidden} {dtype} T {T}: op {e_op:.3e}, torch sequence {e_torch:.3e}, ratio {e_op / e_torch:.3f}")
            record_parity(f"swin_ffn/C{C}h{hidden}/T{T}/{dtype}", e_op, 2 * e_torch)
            figures[f"T{T}"] = dict(op=e_op, torch_sequence=e_torch, ratio=e_op / e_torch, bar_ratio=2.0)
    _OBSERVED[f"C{C}_hidden{hidden}_{dtype}"] = figures
    _write_observed()
    for T, v in figures.items():
        assert v["op"] <= 2 * v["torch_sequence"], (T, v)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("C,hidden", SHAPES[:3])
def test_with_a_zero_fc2_the_output_is_the_residual_exactly(dev, C, hidden, dtype):
    blk = make_block(C, hidden, dtype, 5).to(dev)
    fc2 = blk.ffn.layers[1]
    x = torch.randn(TMAX, C, generator=torch.Generator().manual_seed(8)).to(dtype).to(dev)
    with torch.no_grad():
        fc2.weight.zero_()
        with_bias = [cs.swin_ffn(x[:T].contiguous(), blk.norm2, blk.ffn) for T in TOKENS]
        want = (x.float() + fc2.bias.float()).to(dtype)              # round16(x + b2) in fp32
        for T, got in zip(TOKENS, with_bias):
            assert torch.equal(got, want[:T]), T
        assert not torch.equal(want, x)
        fc2.bias.zero_()
        for T in TOKENS:
            assert torch.equal(cs.swin_ffn(x[:T].contiguous(), blk.norm2, blk.ffn), x[:T]), T


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_eps_is_honoured(dev, dtype):
    """Rows whose variance is of the order of eps (3e-3 squared): 1e-5 and 1e-3 give different normalised rows, each inside the bar
    against its own reference."""
    C, hidden, T = 96, 384, 129
    x = (3e-3 * torch.randn(T, C, generator=torch.Generator().manual_seed(11))).to(dtype)
    outs = []
    for eps in (1e-5, 1e-3):
        blk = make_block(C, hidden, dtype, 12, eps=eps)
        want = ref.module_forward(x, blk.norm2, blk.ffn)
        blk = blk.to(dev)
        with torch.no_grad():
            got = cs.swin_ffn(x.to(dev), blk.norm2, blk.ffn)
            plain = torch_tail(blk, x.to(dev))
        top = want.abs().max().item()
        e_op = (got.cpu().double() - want).abs().max().item() / top
        e_torch = (plain.cpu().double() - want).abs().max().item() / top
        print(f"eps {eps} {dtype}: op {e_op:.3e}, torch sequence {e_torch:.3e}")
        record_parity(f"swin_ffn/eps{eps}/{dtype}", e_op, 2 * e_torch)
        _OBSERVED[f"eps{eps}_{dtype}"] = dict(op=e_op, torch_sequence=e_torch, ratio=e_op / e_torch, bar_ratio=2.0)
        assert e_op <= 2 * e_torch
        outs.append(got)
    _write_observed()
    assert not torch.equal(outs[0], outs[1]) and (outs[0].float() - outs[1].float()).abs().max().item() > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("C,hidden", SHAPES[:3])
def test_rows_do_not_depend_on_their_tile_and_equal_calls_give_equal_bits(dev, C, hidden, dtype):
    blk, x, _, _ = _case(C, hidden, dtype, dev)
    with torch.no_grad():
        whole = cs.swin_ffn(x[:129].contiguous(), blk.norm2, blk.ffn)
        a = cs.swin_ffn(x[:64].contiguous(), blk.norm2, blk.ffn)
        b = cs.swin_ffn(x[64:129].contiguous(), blk.norm2, blk.ffn)
        assert torch.equal(torch.cat([a, b]), whole)
        assert torch.equal(cs.swin_ffn(x[:129].contiguous(), blk.norm2, blk.ffn), whole)
        c = cs.swin_ffn(x[1:66].contiguous(), blk.norm2, blk.ffn)              # every row in another lane slot
        assert torch.equal(c, whole[1:66])
        given = torch.full((129, C), float("nan"), dtype=dtype, device=dev)
        assert cs.swin_ffn(x[:129].contiguous(), blk.norm2, blk.ffn, out=given) is given and torch.equal(given, whole)
        lead = cs.swin_ffn(x[:120].reshape(2, 3, 20, C), blk.norm2, blk.ffn)    # leading dimensions are tokens
        assert lead.shape == (2, 3, 20, C) and torch.equal(lead.reshape(120, C), whole[:120])
        with pytest.raises(RuntimeError):
            cs.swin_ffn(x[:129].contiguous(), blk.norm2, blk.ffn, out=given[:64])
        assert cs.swin_ffn(x[:0].contiguous(), blk.norm2, blk.ffn).shape == (0, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("C,hidden", SHAPES[:3])
def test_guarded_buffers(dev, C, hidden, dtype):
    """x and out of exact size inside an arena whose every other byte is 0xFF (a NaN in both storage types): the guards around out
    stay intact, and out, which held NaNs, is finite everywhere: every element was written and nothing past x's extent was read."""
    blk, x, want, _ = _case(C, hidden, dtype, dev)
    arena = Arena(dev, 0xFF)
    with torch.no_grad():
        for T in TOKENS:
            xin = arena.put(x[:T], f"x{T}")
            out = arena.out((T, C), dtype, f"out{T}")
            assert torch.isnan(out).all()
            assert cs.swin_ffn(xin, blk.norm2, blk.ffn, out=out) is out
            arena.check()
            assert torch.isfinite(out).all(), T
            assert torch.equal(out, cs.swin_ffn(x[:T].contiguous(), blk.norm2, blk.ffn)), T


def test_sizes_the_kernel_does_not_serve_answer_none(dev):
    for C, hidden in [(48, 192), (224, 896), (32, 800)]:
        blk = cs.SwinBlock(C, 1, hidden).half().to(dev).eval()
        assert not cs.swin_ffn_spec(blk)
        assert cs.swin_ffn(torch.zeros(5, C, dtype=torch.float16, device=dev), blk.norm2, blk.ffn) is None
    relu = cs.SwinBlock(96, 3, 384, act_cfg=dict(type="ReLU")).half().to(dev).eval()
    assert cs.swin_ffn(torch.zeros(5, 96, dtype=torch.float16, device=dev), relu.norm2, relu.ffn) is None
