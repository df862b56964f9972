"""`bevamd_window_attention_forward` (bevfusion_amd/csrc/ext/window_attention.hip) through `cam_swin.window_attention`, pinned to the
float64 restatement of tests/swin_reference.py on the exact 16-bit operand values.

The bar is derived, not observed:   |out - ref| <= 1.01 * (u |ref| + (u + eps) mag) + d
  mag = sum_j p_j |v_j| in float64;  u = 2^-11 (fp16) or 2^-8 (bf16): ONE rounding of P to the storage type and ONE of the output;
  d = 2^-24 (fp16: the subnormal spacing) or 0 (bf16);
  eps = 2 [(32 + 8) 2^-23 max_j (scale sum_d |q_d| |k_jd| + |bias_j|) + 2^-21]: the fp32 logit sum of 32 products in any order, the
  scale, the bias, the maximum's own error and the exp, once for the numerator and once for the denominator.
The exact case needs no tolerance: with q = k = 0 and a bias that is 0 at j = pi(i) and -10^4 elsewhere P is one-hot, and the output
must be the selected token's v bit for bit, which catches every lane-map, shift, window, pad and head-offset error.

The observed worst error / bar is written to profiles/cam_swin_observed.json.
"""
import json
import os

import pytest
import torch

import swin_reference as ref
from bevfusion_amd import _capi
from bevfusion_amd import cam_swin as cs
from conftest import record_parity
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
D = {torch.float16: 2.0 ** -24, torch.bfloat16: 0.0}
MAPS = [((7, 7), 0), ((7, 7), 3), ((5, 3), 0), ((5, 3), 3), ((8, 10), 0), ((8, 10), 3), ((15, 22), 3), ((14, 7), 6)]
HD, WS, N = 32, 7, 49
SCALE = 32 ** -0.5
_OBSERVED = {}


def _padded(hw):
    return tuple(-(-s // WS) * WS for s in hw)


def _pixel_regions(hw, shift):
    """[H, W] region id of every source pixel (its place in the rolled frame), and the per-window region sets."""
    Hp, Wp = _padded(hw)
    if shift == 0:
        return torch.zeros(hw, dtype=torch.int64), [set([0])]
    rolled = ref.region_map(Hp, Wp, WS, shift)
    sets = [set(rolled[y:y + WS, x:x + WS].reshape(-1).tolist()) for y in range(0, Hp, WS) for x in range(0, Wp, WS)]
    return torch.roll(rolled, shifts=(shift, shift), dims=(0, 1))[:hw[0], :hw[1]], sets


_CASES = {}


def _case(hw, shift, heads, with_pad, dtype):
    """Inputs on the host in `dtype` and their float64 reference, computed once per case."""
    key = (hw, shift, heads, with_pad, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * hw[0] + 10 * hw[1] + shift + 7 * heads)
        B, (H, W), C = 2, hw, heads * HD
        qkv = torch.randn(B, H, W, 3 * C, generator=g)                  # different data per sample
        regions, sets = _pixel_regions(hw, shift)
        qkv[..., 2 * C:] += (1.5 * (regions.double() - 4.0)).float()[None, :, :, None] if shift else 0.0
        pad = torch.randn(3 * C, generator=g).to(dtype) if with_pad else None
        bias = torch.randn(heads, N, N, generator=g)
        qkv = qkv.to(dtype)
        out, mag, row = ref.shifted_window_attention(qkv.double(), None if pad is None else pad.double(), bias.double(), SCALE, shift, heads)
        # the inputs are telling
        if shift:
            assert max(len(s) for s in sets) == 4, sets
        if H % WS or W % WS:
            Hp, Wp = _padded(hw)
            assert Hp * Wp - H * W > 0                                   # padded tokens exist, and every token of a window is a key
        _CASES[key] = (qkv, pad, bias, out, mag, row)
    return _CASES[key]


def test_the_cases_cover_padding_and_four_region_windows():
    assert any((hw[0] % WS or hw[1] % WS) and shift for hw, shift in MAPS) and any((hw[0] % WS or hw[1] % WS) and not shift for hw, shift in MAPS)
    for hw, shift in MAPS:
        if shift:
            assert max(len(s) for s in _pixel_regions(hw, shift)[1]) == 4, (hw, shift)


def _run(dev, qkv, pad, bias, shift, **kw):
    return cs.window_attention(qkv.to(dev), bias.to(dev), SCALE, shift, None if pad is None else pad.to(dev), **kw)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("with_pad", [True, False], ids=["pad", "nullpad"])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("hw, shift", MAPS)
def test_against_float64(dev, hw, shift, heads, with_pad, dtype):
    qkv, pad, bias, want, mag, row = _case(hw, shift, heads, with_pad, dtype)
    got = _run(dev, qkv, pad, bias, shift)
    assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
    u = U[dtype]
    eps = 2 * ((32 + 8) * 2.0 ** -23 * row + 2.0 ** -21)
    bar = 1.01 * (u * want.abs() + (u + eps) * mag) + D[dtype]
    err = (got.cpu().double() - want).abs()
    worst = (err / bar).max().item()
    print(f"{hw} shift {shift} heads {heads} {'pad' if with_pad else 'null'} {dtype}: worst error / bar {worst:.3f}, max |err| {err.max().item():.3e}")
    record_parity(f"window_attention/{dtype}", worst, 1.0)
    _OBSERVED[str(dtype)] = max(_OBSERVED.get(str(dtype), 0.0), worst)
    path = os.path.join(ROOT, "profiles", "cam_swin_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.setdefault("window_attention_worst_error_over_bar", {})[str(dtype)] = _OBSERVED[str(dtype)]
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass      # a read-only checkout: the figures are printed above
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hw, shift", MAPS)
def test_one_hot_bias_selects_a_token_bit_for_bit(dev, hw, shift, dtype):
    heads, B, (H, W) = 3, 2, hw
    C = heads * HD
    g = torch.Generator().manual_seed(77 + hw[0] + shift)
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    qkv[..., :2 * C] = 0.0
    pad = torch.randn(3 * C, generator=g)
    pad[:2 * C] = 0.0
    bias = torch.full((heads, N, N), -1.0e4)
    for h in range(heads):
        bias[h, torch.arange(N), torch.randperm(N, generator=g)] = 0.0
    qkv, pad = qkv.to(dtype), pad.to(dtype)
    want, _, _ = ref.shifted_window_attention(qkv.double(), pad.double(), bias.double(), SCALE, shift, heads)
    assert torch.equal(want.to(dtype).double(), want)                    # the reference IS a selection of 16-bit values
    if H % WS or W % WS:                                                 # and some rows select the padded token's v
        assert any(torch.equal(want[b, y, x, :HD], pad[2 * C:2 * C + HD].double()) for b in range(B) for y in range(H) for x in range(W))
    got = _run(dev, qkv, pad, bias, shift)
    assert torch.equal(got.cpu().double(), want)


# ---- contracts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("hw, shift", [((8, 10), 3), ((5, 3), 0)])
def test_guarded_buffers_of_exact_size(dev, hw, shift, fill):
    qkv, pad, bias, _, _, _ = _case(hw, shift, 3, True, torch.float16)
    plain = _run(dev, qkv, pad, bias, shift)
    arena = Arena(dev, fill, capacity=8 << 20)
    gq, gp, gb = arena.put(qkv, "qkv"), arena.put(pad, "pad"), arena.put(bias, "bias")
    out = arena.out(tuple(plain.shape), torch.float16, "out")
    assert cs.window_attention(gq, gb, SCALE, shift, gp, out=out) is out
    arena.check()
    assert torch.equal(gq.cpu(), qkv) and torch.equal(gp.cpu(), pad) and torch.equal(gb.cpu(), bias)
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)) and not torch.isnan(out).any()


@pytest.mark.parametrize("hw, shift", [((8, 10), 3), ((15, 22), 3)])
def test_batch_equals_samples_and_equal_calls_equal_bits(dev, hw, shift):
    qkv, pad, bias, _, _, _ = _case(hw, shift, 3, True, torch.bfloat16)
    both = _run(dev, qkv, pad, bias, shift)
    again = _run(dev, qkv, pad, bias, shift)
    assert torch.equal(both.view(torch.int16), again.view(torch.int16))
    for b in range(qkv.shape[0]):
        alone = _run(dev, qkv[b:b + 1].contiguous(), pad, bias, shift)
        assert torch.equal(alone.view(torch.int16), both[b:b + 1].view(torch.int16))


def test_refusals_launch_nothing(dev):
    heads, H, W = 2, 8, 10
    C = heads * HD
    arena = Arena(dev, 0x7B, capacity=8 << 20)
    qkv = arena.put(torch.randn(1, H, W, 3 * C).half(), "qkv")
    bias = arena.put(torch.randn(heads, N, N), "bias")
    out = arena.out((1, H, W, C), torch.float16, "out")
    # window 8: not built
    assert cs.window_attention(qkv, arena.put(torch.zeros(heads, 64, 64), "bias8"), SCALE, 0, window=8, out=out) is None
    # head dimension 16 (four heads over the same 64 channels)
    assert cs.window_attention(qkv, arena.put(torch.zeros(4, N, N), "bias4"), SCALE, 0, out=out) is None
    with pytest.raises(RuntimeError):
        cs.window_attention(qkv.float(), bias, SCALE, 0)
    with pytest.raises(RuntimeError):
        cs.window_attention(qkv.cpu(), bias.cpu(), SCALE, 0)
    with pytest.raises(RuntimeError, match="overlaps"):
        cs.window_attention(qkv, bias, SCALE, 0, out=qkv.view(-1)[C:C + H * W * C].view(1, H, W, C))
    lib = _capi.load()

    def call(qkv_elems, out_elems, shift=0):
        with torch.cuda.device(dev):
            return lib.bevamd_window_attention_forward(_capi.ptr(qkv), qkv_elems, None, 0, _capi.ptr(bias), bias.numel(), 0, 1, H, W, C, heads,
                                                       7, 32, SCALE, shift, _capi.ptr(out), out_elems, _capi.stream_ptr(dev))
    assert call(qkv.numel(), out.numel() - 1) == 1 and "out holds" in _capi.last_error()
    assert call(qkv.numel() - 1, out.numel()) == 1 and "qkv holds" in _capi.last_error()
    assert call(qkv.numel(), out.numel(), shift=7) == 1
    arena.check()
    arena.untouched(out)
    assert call(qkv.numel(), out.numel()) == 0                           # and the same call with the right counts runs
    arena.check()
    assert not torch.isnan(out).any()
