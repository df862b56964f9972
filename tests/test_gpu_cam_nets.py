"""The camera depth nets on the device (`bevamd_cam_depth_stem_forward`, `bevamd_cam_depth_head_forward`, the fused route of
`LSSTransform` / `DepthLSSTransform.get_cam_feats`), pinned to float64 on the CPU.

Every reference is float64 computed from the exact 16-bit operand values and the folds' own fp32 scale, shift and bias, the
convention of tests/test_gpu_bev_trunk.py: u = 2^-11 (fp16) or 2^-8 (bf16) is one rounding to the storage type, 2^-23 per term
covers any fp32 summation order, d = 2^-24 is fp16's subnormal step (0 for bf16).

Stem.  The float64 chain ref_1 = relu(d s1 + t1), ref_i = relu(s_i conv(ref_{i-1}, w_i) + t_i) is never rounded; the bar carries the
error of every layer to the next (ReLU is 1-Lipschitz, so an input error e reaches the output as at most |s| conv(e, |w|)):

    e_1 = u |ref_1| + 4 * 2^-23 (|d s1| + |t1|)
    e_i = 1.01 (u |ref_i| + (K_i + 8) 2^-23 mag_i) + d + |s_i| conv(e_{i-1}, |w_i|),   mag_i = |s_i| conv(|ref_{i-1}|, |w_i|) + |t_i|

with K_2 = 200 and K_3 = 800.  The exact cases have no tolerance: integer depths, integer weights in [-2, 2], power-of-two scales
and integer shifts chosen so that every intermediate of the float64 chain is an integer the storage type holds.

Head.  z_ref = W x + b in float64, E = 1.01 (K + 8) 2^-23 mag with mag = sum |w| |x| + |b|:

    |ctx - z_ref| <= E                      |p - p_ref| <= p_ref (expm1(2 E_pixel) + c 2^-23) + 2^-126

E_pixel is the largest E over the pixel's depth rows (a logit error of at most E moves a softmax by at most a factor exp(2 E)),
2^-126 is fp32's smallest normal (flushed tails) and c covers the implementation's exp, sum and divide: twice the worst
(|p - p_ref| - p_ref expm1(2 E)) / (2^-23 p_ref) observed on an MI355X over the cases of this file, and at most D + 64 (D - 1
half-ulps for the sum, the rest for exp and one division).  That observation is NEGATIVE in every case (the largest is -411.8, at
Cin 32, D 5 on 8 x 17: profiles/cam_nets_observed.json): the derived term alone, at least (32 + 8) 2^-23 mag per logit, covers the
whole error; the raw |p - p_ref| stays within 24.5 x 2^-23 p_ref, most of it the logits' own error.  Twice a negative number is no
allowance, so C_SOFTMAX = 0: the bar is the derived term and the flush term, nothing else.
"""
import copy
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from bevfusion_amd import bev_trunk as bt, cam_nets as cn
from bevfusion_amd.vtransforms import DepthLSSTransform, FactoredCamFeats
from conftest import record_parity
from guarded import Arena
from test_cam_nets import NOT_FUSABLE, SMALL, randomise, small_inputs, small_transform, unfusable_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "cam_nets_observed.json")
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB = {torch.float16: 2.0 ** -24, torch.bfloat16: 0.0}
TOP = {torch.float16: 2.0 ** 11, torch.bfloat16: 2.0 ** 8}          # integers up to here are exact in the storage type
DTYPES = [torch.float16, torch.bfloat16]
DIDS = ["f16", "bf16"]
STEM_MAPS = [(1, 1), (4, 4), (5, 9), (9, 13), (33, 70), (64, 136)]
HEAD_SIZES = [(32, 1, 4), (32, 5, 4), (32, 16, 16), (64, 17, 12), (256, 118, 80), (512, 59, 64), (32, 128, 128)]
HEAD_MAPS = [(1, 1), (3, 5), (8, 17)]
C_SOFTMAX = 0.0          # max(0, twice the worst observation); the observation is negative (docstring); condition: <= D + 64
EPS23 = 2.0 ** -23


def _update_observed(section, key, value, worst=False):
    """Write one figure into profiles/cam_nets_observed.json (worst: keep the larger of the old and the new one)."""
    try:
        old = json.load(open(OBSERVED)) if os.path.exists(OBSERVED) else {}
        sec = old.setdefault(section, {})
        sec[key] = max(value, sec.get(key, value)) if worst else value
        with open(OBSERVED, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass      # a read-only checkout: the figures are printed


# ---- the stem: data and the float64 reference ------------------------------------------------------------------------------------
def _stem_fold(p, dtype, dev):
    return cn.DepthStemFold(p["s1"].to(dev), p["t1"].to(dev), cn.pack_stem_layer2(p["w2"].to(dtype)).to(dev), p["s2"].to(dev),
                            p["t2"].to(dev), bt.bev_pack_weight(p["w3"].to(dtype)).to(dev), p["s3"].to(dev), p["t3"].to(dev), dtype)


def _stem_random(seed, hw, dtype, n=2):
    """A raster as `depth_raster` leaves it (mostly zero, ranges up to 60 m) and parameters that keep the activations' scale."""
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    depth = torch.where(torch.rand(n, H, W, generator=g) < 0.3, 60.0 * torch.rand(n, H, W, generator=g), torch.zeros(()))
    sign = lambda c: torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)      # noqa: E731
    p = dict(s1=(0.02 + 0.05 * torch.rand(8, generator=g)) * sign(8), t1=0.5 * torch.randn(8, generator=g),
             w2=(torch.randn(32, 8, 5, 5, generator=g) / 200 ** 0.5).to(dtype), s2=(0.5 + torch.rand(32, generator=g)) * sign(32),
             t2=0.5 * torch.randn(32, generator=g), w3=(torch.randn(64, 32, 5, 5, generator=g) / 800 ** 0.5).to(dtype),
             s3=(0.5 + torch.rand(64, generator=g)) * sign(64), t3=0.5 * torch.randn(64, generator=g))
    return depth, {k: v.float() if k[0] in "st" else v for k, v in p.items()}


def _sparse_ints(shape, density, g):
    return torch.randint(-2, 3, shape, generator=g).float() * (torch.rand(shape, generator=g) < density).float()


def _stem_exact(seed, hw, dtype, kind, n=2):
    """Integer depths, integer weights in [-2, 2] (sparse, so that the sums stay inside the storage type's exact integers),
    power-of-two scales, integer shifts.  kind: "random" (a sparse raster of 0 / 2 / 4), "zero" (an all-zero raster: with t1 != 0
    the output tells "pad the layer-1 output" from "pad the depth"), "corners" (one non-zero pixel in each corner)."""
    g = torch.Generator().manual_seed(2000 + seed)
    H, W = hw
    if kind == "random":
        depth = 2.0 * torch.randint(0, 3, (n, H, W), generator=g).float() * (torch.rand(n, H, W, generator=g) < 0.25).float()
    elif kind == "zero":
        depth = torch.zeros(n, H, W)
    else:
        depth = torch.zeros(n, H, W)
        for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            depth[:, y, x] = 2.0 * (i + 1)
    dens2, dens3, big = (0.5, 0.1, 2.0) if dtype == torch.float16 else (0.1, 0.008, 1.0)      # bf16 holds integers up to 256 only
    p = dict(s1=torch.tensor([1.0, -0.5, 0.5, 1.0, -1.0, 0.5, 1.0, -0.5]), t1=torch.tensor([1.0, 2.0, -1.0, 0.0, 3.0, 1.0, -2.0, 0.0]),
             w2=_sparse_ints((32, 8, 5, 5), dens2, g).to(dtype), s2=torch.tensor([(-1.0 if c % 5 == 3 else 1.0) * (big if c % 4 == 1 else 1.0) for c in range(32)]),
             t2=torch.tensor([float((c * 7) % 5 - 1) for c in range(32)]), w3=_sparse_ints((64, 32, 5, 5), dens3, g).to(dtype),
             s3=torch.tensor([(-1.0 if c % 5 == 2 else 1.0) * (big if c % 4 == 3 else 1.0) for c in range(64)]),
             t3=torch.tensor([float((c * 3) % 7 - 2) for c in range(64)]))
    return depth, p


def _stem_ref64(depth, p):
    """-> (ref_3 [n, 64, OH3, OW3], bar pieces) of the never-rounded float64 chain."""
    d = depth.double().unsqueeze(1)
    s = lambda k: p[k].double().view(1, -1, 1, 1)      # noqa: E731
    pre1 = d * s("s1") + s("t1")
    ref1 = torch.relu(pre1)
    mag1 = (d * s("s1")).abs() + s("t1").abs()
    w2, w3 = p["w2"].double(), p["w3"].double()
    pre2 = s("s2") * F.conv2d(ref1, w2, stride=4, padding=2) + s("t2")
    ref2 = torch.relu(pre2)
    mag2 = s("s2").abs() * F.conv2d(ref1.abs(), w2.abs(), stride=4, padding=2) + s("t2").abs()
    pre3 = s("s3") * F.conv2d(ref2, w3, stride=2, padding=2) + s("t3")
    ref3 = torch.relu(pre3)
    mag3 = s("s3").abs() * F.conv2d(ref2.abs(), w3.abs(), stride=2, padding=2) + s("t3").abs()
    return dict(ref1=ref1, ref2=ref2, ref3=ref3, mag1=mag1, mag2=mag2, mag3=mag3, pre=(pre1, pre2, pre3), w2=w2, w3=w3,
                s2=s("s2").abs(), s3=s("s3").abs())


def _stem_bar(r, dtype):
    u, sub = U[dtype], SUB[dtype]
    e1 = u * r["ref1"].abs() + 4 * EPS23 * r["mag1"]
    e2 = 1.01 * (u * r["ref2"].abs() + (200 + 8) * EPS23 * r["mag2"]) + sub + r["s2"] * F.conv2d(e1, r["w2"].abs(), stride=4, padding=2)
    e3 = 1.01 * (u * r["ref3"].abs() + (800 + 8) * EPS23 * r["mag3"]) + sub + r["s3"] * F.conv2d(e2, r["w3"].abs(), stride=2, padding=2)
    return e2, e3


def _run_stem(depth, p, dtype, dev, **kw):
    y = cn.depth_stem_forward(depth.to(dev), _stem_fold(p, dtype, dev), **kw)
    n, H, W = depth.shape
    assert y is not None and y.dtype == dtype and tuple(y.shape) == (n, 64) + cn.stem_output_size(H, W)
    assert y.is_contiguous(memory_format=torch.channels_last)
    return y


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("kind", ["random", "zero", "corners"])
@pytest.mark.parametrize("hw", STEM_MAPS, ids=lambda hw: "%dx%d" % hw)
def test_stem_is_exact_on_integers(dev, hw, kind, dtype):
    depth, p = _stem_exact(STEM_MAPS.index(hw), hw, dtype, kind)
    r = _stem_ref64(depth, p)
    for pre in r["pre"]:      # the test's own inputs: every intermediate is an integer the storage type holds exactly
        assert torch.equal(pre, pre.round()) and pre.abs().max().item() <= TOP[dtype], pre.abs().max().item()
    assert (r["ref1"] > 0).any() and (p["t1"] > 0).any()
    assert (r["ref3"] > 0).double().mean().item() >= 0.1 and (r["ref2"] > 0).double().mean().item() >= 0.1, "the case tells nothing"
    if kind == "zero":        # padding the depth instead of the layer-1 output gives another answer on this very case
        full = torch.relu(p["t1"].double()).view(1, 8, 1, 1).expand(depth.shape[0], 8, hw[0] + 4, hw[1] + 4)
        wrong2 = torch.relu(p["s2"].double().view(1, -1, 1, 1) * F.conv2d(full, r["w2"], stride=4) + p["t2"].double().view(1, -1, 1, 1))
        assert wrong2.shape == r["ref2"].shape and not torch.equal(wrong2, r["ref2"])
    y = _run_stem(depth, p, dtype, dev).cpu()
    want = r["ref3"].to(dtype)
    assert torch.equal(y.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), (y.double() - r["ref3"]).abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("hw", STEM_MAPS, ids=lambda hw: "%dx%d" % hw)
def test_stem_against_float64(dev, hw, dtype):
    depth, p = _stem_random(STEM_MAPS.index(hw), hw, dtype)
    r = _stem_ref64(depth, p)
    e2, e3 = _stem_bar(r, dtype)
    n = depth.shape[0]
    oh2, ow2 = (hw[0] - 1) // 4 + 1, (hw[1] - 1) // 4 + 1
    scratch = torch.empty((n, oh2, ow2, 32), dtype=dtype, device=dev)
    y = _run_stem(depth, p, dtype, dev, scratch=scratch)
    worst2 = ((scratch.permute(0, 3, 1, 2).cpu().double() - r["ref2"]).abs() / e2).max().item()
    worst3 = ((y.cpu().double() - r["ref3"]).abs() / e3).max().item()
    print(f"stem {hw} {dtype}: worst error / bar = {worst2:.3f} (layer 2), {worst3:.3f} (layer 3)")
    record_parity(f"cam_stem/layer2/{dtype}", worst2, 1.0)
    record_parity(f"cam_stem/layer3/{dtype}", worst3, 1.0)
    if hw[0] * hw[1] >= 36:
        assert 0.1 <= (r["ref3"] > 0).double().mean().item() <= 0.9
    assert worst2 <= 1.0 and worst3 <= 1.0, (worst2, worst3)
    again = _run_stem(depth, p, dtype, dev)
    assert torch.equal(again, y)                                           # equal calls give equal bits
    one = _run_stem(depth[1:], p, dtype, dev)
    assert torch.equal(one, y[1:])                                         # a sample ignores its batch


# ---- the head: data and the float64 reference ------------------------------------------------------------------------------------
def _head_fold(w, b, D, C, dtype, dev):
    return cn.DepthHeadFold(cn.pack_head_weight(w.to(dtype)).to(dev), b.float().to(dev), w.shape[1], D, C, dtype)


def _head_random(seed, cin, D, C, hw, dtype, n=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin) + tuple(hw), generator=g).to(dtype)
    w = (2.0 * torch.randn(D + C, cin, 1, 1, generator=g) / cin ** 0.5).to(dtype)      # logits that spread over several units
    b = torch.randn(D + C, generator=g)
    return x, w, b


def _head_ref64(x, w, b, D):
    """-> z_ref, E (both [n, D + C, H, W]), p_ref [n, D, H, W], all float64."""
    xd, wd, bd = x.double(), w.double(), b.float().double().view(1, -1, 1, 1)
    z = F.conv2d(xd, wd) + bd
    mag = F.conv2d(xd.abs(), wd.abs()) + bd.abs()
    E = 1.01 * (x.shape[1] + 8) * EPS23 * mag
    return z, E, torch.softmax(z[:, :D], dim=1)


def _run_head(x, w, b, D, C, dtype, dev, **kw):
    res = cn.depth_head_forward(x.to(dev).contiguous(memory_format=torch.channels_last), _head_fold(w, b, D, C, dtype, dev), **kw)
    assert res is not None
    depth, ctx = res
    n, _, H, W = x.shape
    assert depth.dtype == ctx.dtype == torch.float32 and tuple(depth.shape) == (n, D, H, W) and tuple(ctx.shape) == (n, H, W, C)
    assert depth.is_contiguous() and ctx.is_contiguous()
    return depth, ctx


def _softmax_excess(p, p_ref, E_pix):
    """The worst (|p - p_ref| - p_ref expm1(2 E)) / (2^-23 p_ref) and the worst raw |p - p_ref| / (2^-23 p_ref), both over the
    elements whose p_ref is a normal fp32 number (0 when there is none), and the bar's verdict."""
    err = (p - p_ref).abs()
    live = p_ref >= 2.0 ** -126
    ulp = EPS23 * p_ref.clamp_min(2.0 ** -126)
    excess = torch.where(live, (err - p_ref * torch.expm1(2 * E_pix)) / ulp, torch.full_like(err, -math.inf))
    raw = torch.where(live, err / ulp, torch.zeros_like(err))
    ok = err <= p_ref * (torch.expm1(2 * E_pix) + C_SOFTMAX * EPS23) + 2.0 ** -126
    worst = excess.max().item()
    return (worst if math.isfinite(worst) else 0.0), raw.max().item(), bool(ok.all())


HEAD_CASES = [(s, hw) for s in HEAD_SIZES for hw in HEAD_MAPS]
HEAD_IDS = ["%d-%d-%d-%dx%d" % (s + hw) for s, hw in HEAD_CASES]


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=HEAD_IDS)
def test_head_against_float64(dev, case, dtype):
    (cin, D, C), hw = case
    x, w, b = _head_random(HEAD_CASES.index(case), cin, D, C, hw, dtype)
    z, E, p_ref = _head_ref64(x, w, b, D)
    depth, ctx = _run_head(x, w, b, D, C, dtype, dev)
    depth, ctx = depth.cpu().double(), ctx.cpu().double().permute(0, 3, 1, 2)
    worst_ctx = ((ctx - z[:, D:]).abs() / E[:, D:]).max().item()
    E_pix = E[:, :D].max(dim=1, keepdim=True).values
    excess, raw, ok = _softmax_excess(depth, p_ref, E_pix)
    total = (depth.sum(dim=1) - 1.0).abs().max().item() / EPS23
    print(f"head {HEAD_IDS[HEAD_CASES.index(case)]} {dtype}: context error / bar = {worst_ctx:.3f}, softmax excess = {excess:.3f} x 2^-23 p "
          f"(raw error {raw:.2f} x 2^-23 p; c = {C_SOFTMAX}, D + 64 = {D + 64}), |sum - 1| = {total:.2f} x 2^-23")
    record_parity(f"cam_head/context/{dtype}", worst_ctx, 1.0)
    record_parity(f"cam_head/depth_sum_ulps/{dtype}", total, D + C_SOFTMAX)
    _update_observed("softmax_excess_ulps", "%d-%d-%d/%s" % (cin, D, C, dtype), round(excess, 3), worst=True)
    _update_observed("softmax_raw_ulps", "%d-%d-%d/%s" % (cin, D, C, dtype), round(raw, 3), worst=True)
    _update_observed("softmax_c", "value", C_SOFTMAX)
    assert C_SOFTMAX <= D + 64
    assert torch.isfinite(depth).all() and worst_ctx <= 1.0, worst_ctx
    assert ok, excess
    assert total <= D + C_SOFTMAX, total
    if D == 1:
        assert bool((depth == 1.0).all())
    if D > 1 and hw != (1, 1):
        assert (depth.max(dim=1).values < 0.999).any() and (depth.min(dim=1).values < 0.2 / D).any(), "the logits do not spread"


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("size", HEAD_SIZES, ids=lambda s: "%d-%d-%d" % s)
def test_head_is_exact_on_integers_and_subtracts_the_maximum(dev, size, dtype):
    """Integer inputs and weights: the context output is exact.  The bias gives every pixel a logit >= 100: a kernel that skips the
    max subtraction overflows exp and returns NaN or inf."""
    cin, D, C = size
    g = torch.Generator().manual_seed(3000 + HEAD_SIZES.index(size))
    x = torch.randint(-2, 3, (2, cin, 3, 5), generator=g).to(dtype)
    w = (torch.randint(-2, 3, (D + C, cin, 1, 1), generator=g).float() * (torch.rand(D + C, cin, 1, 1, generator=g) < 0.25).float()).to(dtype)
    b = torch.randint(-3, 4, (D + C,), generator=g).float()
    b[D // 2] = 100.0 + 4.0 * cin
    z, E, p_ref = _head_ref64(x, w, b, D)
    assert z[:, :D].max(dim=1).values.min().item() >= 100.0 and z.abs().max().item() < 2.0 ** 24
    depth, ctx = _run_head(x, w, b, D, C, dtype, dev)
    depth, ctx = depth.cpu(), ctx.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(depth).all(), "NaN or inf: exp overflowed, the maximum was not subtracted"
    assert torch.equal(ctx, z[:, D:].float())
    excess, _, ok = _softmax_excess(depth.double(), p_ref, E[:, :D].max(dim=1, keepdim=True).values)
    print(f"head exact {size} {dtype}: softmax excess = {excess:.3f} x 2^-23 p")
    assert ok, excess


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("D", [1, 5, 17, 118, 128])
def test_equal_logits_give_one_over_D(dev, D, dtype):
    x = torch.randn(2, 32, 3, 5, generator=torch.Generator().manual_seed(D)).to(dtype)
    w = torch.zeros(D + 4, 32, 1, 1)
    w[D:] = torch.randn(4, 32, 1, 1, generator=torch.Generator().manual_seed(D + 1)) / 32 ** 0.5
    b = torch.cat([torch.full((D,), 0.75), torch.zeros(4)])
    z, E, p_ref = _head_ref64(x, w.to(dtype), b, D)
    depth, _ = _run_head(x, w.to(dtype), b, D, 4, dtype, dev)
    excess, _, ok = _softmax_excess(depth.cpu().double(), p_ref, E[:, :D].max(dim=1, keepdim=True).values)
    assert ok and (p_ref - 1.0 / D).abs().max().item() < 1e-15, excess
    if D == 1:
        assert bool((depth == 1.0).all())


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("hw", [(1, 1), (9, 13), (33, 70)], ids=lambda hw: "%dx%d" % hw)
def test_stem_guarded_buffers_of_exact_size(dev, hw, fill):
    """Depth, every parameter, the scratch map and the output carved from one arena filled with a dirty byte (0xFF: NaN halves): no
    guard byte changes, the inputs are unchanged, every element of scratch and out is written, the bits equal an unguarded call's."""
    dtype = torch.float16
    depth, p = _stem_random(40, hw, dtype)
    n = depth.shape[0]
    oh2, ow2 = (hw[0] - 1) // 4 + 1, (hw[1] - 1) // 4 + 1
    oh3, ow3 = cn.stem_output_size(*hw)
    fold = _stem_fold(p, dtype, dev)
    plain_scratch = torch.empty((n, oh2, ow2, 32), dtype=dtype, device=dev)
    plain = cn.depth_stem_forward(depth.to(dev), fold, scratch=plain_scratch)
    arena = Arena(dev, fill, capacity=16 << 20)
    gdepth = arena.put(depth, "depth")
    gfold = copy.copy(fold)
    for name in ("scale1", "shift1", "packed2", "scale2", "shift2", "packed3", "scale3", "shift3"):
        setattr(gfold, name, arena.put(getattr(fold, name), name))
    scratch, out = arena.out((n, oh2, ow2, 32), dtype, "scratch"), arena.out((n, oh3, ow3, 64), dtype, "out")
    res = cn.depth_stem_forward(gdepth, gfold, scratch=scratch, out=out)
    assert res is not None and res.data_ptr() == out.data_ptr()
    arena.check()
    assert torch.equal(gdepth.cpu(), depth) and torch.equal(gfold.packed3, fold.packed3) and torch.equal(gfold.shift1, fold.shift1)
    assert torch.equal(scratch.view(torch.int16), plain_scratch.view(torch.int16))
    assert torch.equal(res.contiguous().view(torch.int16), plain.contiguous().view(torch.int16))
    assert not torch.isnan(out).any() and not torch.isnan(scratch).any()


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("size, hw", [((32, 1, 4), (1, 1)), ((64, 17, 12), (3, 5)), ((256, 118, 80), (8, 17)), ((32, 128, 128), (3, 5))])
def test_head_guarded_buffers_of_exact_size(dev, size, hw, fill):
    cin, D, C = size
    dtype = torch.bfloat16
    x, w, b = _head_random(50, cin, D, C, hw, dtype)
    fold = _head_fold(w, b, D, C, dtype, dev)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    plain = cn.depth_head_forward(xd, fold)
    arena = Arena(dev, fill, capacity=16 << 20)
    gx = arena.put(xd.permute(0, 2, 3, 1).contiguous(), "x").permute(0, 3, 1, 2)
    gfold = copy.copy(fold)
    gfold.packed, gfold.bias = arena.put(fold.packed, "packed"), arena.put(fold.bias, "bias")
    n = x.shape[0]
    depth, ctx = arena.out((n, D) + hw, torch.float32, "depth"), arena.out((n,) + hw + (C,), torch.float32, "ctx")
    res = cn.depth_head_forward(gx, gfold, depth=depth, ctx=ctx)
    assert res is not None and res[0] is depth and res[1] is ctx
    arena.check()
    assert torch.equal(gx, xd) and torch.equal(gfold.packed, fold.packed) and torch.equal(gfold.bias, fold.bias)
    assert torch.equal(depth.view(torch.int32), plain[0].view(torch.int32)) and torch.equal(ctx.view(torch.int32), plain[1].view(torch.int32))
    assert not torch.isnan(depth).any() and not torch.isnan(ctx).any()


# ---- the modules -----------------------------------------------------------------------------------------------------------------
def _functional_chain(m, x, d, dtype):
    """get_cam_feats' fused route written out with the functional wrappers and the module's own folds -> (depth, ctx NHWC)."""
    B, N, C, fH, fW = x.shape
    xh = x.reshape(B * N, C, fH, fW).to(dtype=dtype, memory_format=torch.channels_last)
    if isinstance(m, DepthLSSTransform):
        dh = cn.depth_stem_forward(d.reshape(B * N, d.shape[3], d.shape[4]), cn.fold_depth_stem(m.dtransform, dtype))
        y = bt.bev_conv_forward([dh, xh], cn.fold_conv_bias_bn(m.depthnet[0], m.depthnet[1], dtype))
        y = bt.bev_conv_forward([y], cn.fold_conv_bias_bn(m.depthnet[3], m.depthnet[4], dtype))
        head = m.depthnet[6]
    else:
        y, head = xh, m.depthnet
    return cn.depth_head_forward(y, cn.fold_depth_head(head, m.D, m.C, dtype))


def _call(m, x, d):
    return m.get_cam_feats(x, d) if isinstance(m, DepthLSSTransform) else m.get_cam_feats(x)


def _chain64(m, x, d):
    """The module's torch layers in float64 from its fp32 master parameters, on the CPU -> (depth [B N, D, fH, fW], ctx [B N, C, fH, fW])."""
    m64 = copy.deepcopy(m).cpu().double().eval()
    B, N, C, fH, fW = x.shape
    z = x.detach().cpu().double().view(B * N, C, fH, fW)
    if isinstance(m, DepthLSSTransform):
        z = torch.cat([m64.dtransform(d.detach().cpu().double().view(B * N, 1, d.shape[3], d.shape[4])), z], dim=1)
    z = m64.depthnet(z)
    return z[:, :m.D].softmax(dim=1), z[:, m.D:m.D + m.C]


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("kind", ["depth", "lss"])
@torch.no_grad()
def test_module_route_bit_equals_the_functional_chain(dev, kind, dtype):
    m = small_transform(kind).to(dev)
    x, d = (t.to(dev) for t in small_inputs())
    assert not m.cam_nets_fusable(x, d)
    m.cam_nets_dtype = dtype
    assert m.cam_nets_fusable(x, d if kind == "depth" else None)
    got = _call(m, x, d)
    depth, ctx = _functional_chain(m, x, d, dtype)
    assert isinstance(got, FactoredCamFeats) and tuple(got.depth.shape) == (1, 2, 5, 2, 3) and tuple(got.ctx.shape) == (1, 2, 4, 2, 3)
    assert got.depth.dtype == got.ctx.dtype == torch.float32
    assert torch.equal(got.depth, depth.view(1, 2, 5, 2, 3)) and torch.equal(got.ctx, ctx.view(1, 2, 2, 3, 4).permute(0, 1, 4, 2, 3))
    # what bev_pool does with it copies nothing
    cl = got.ctx.float().permute(0, 1, 3, 4, 2)
    assert cl.contiguous().data_ptr() == got.ctx.data_ptr() and cl.is_contiguous()
    assert got.depth.float().contiguous().data_ptr() == got.depth.data_ptr()
    # and against float64 of the fp32 master parameters the 16-bit route is close (the derived bars are on the kernels above)
    ref_depth, ref_ctx = _chain64(m, x, d)
    assert (got.depth.cpu().double().view(2, 5, 2, 3) - ref_depth).abs().max().item() <= 64 * U[dtype]
    assert (got.ctx.cpu().double().reshape(2, 4, 2, 3) - ref_ctx).abs().max().item() <= 64 * U[dtype] * (1 + ref_ctx.abs().max().item())
    # fused_cam_feats = False: the reference's materialised layout with the same values
    m.fused_cam_feats = False
    mat = _call(m, x, d)
    assert torch.is_tensor(mat) and tuple(mat.shape) == (1, 2, 5, 2, 3, 4) and torch.equal(mat, got.materialize())


@pytest.mark.parametrize("kind", ["depth", "lss"])
@torch.no_grad()
def test_bev_pool_takes_the_fused_result_as_it_is(dev, kind):
    m = small_transform(kind).to(dev)
    m.cam_nets_dtype = torch.float16
    x, d = (t.to(dev) for t in small_inputs())
    got = _call(m, x, d)
    eye = torch.eye(3, device=dev).view(1, 1, 3, 3).repeat(1, 2, 1, 1)
    intr = torch.tensor([[8.0, 0.0, 12.0], [0.0, 8.0, 8.0], [0.0, 0.0, 1.0]], device=dev).view(1, 1, 3, 3).repeat(1, 2, 1, 1)
    zero = torch.zeros(1, 2, 3, device=dev)
    geom = m.get_geometry(eye, zero, intr, eye, zero)
    out = m.bev_pool(geom, got)
    twin = m.bev_pool(geom, FactoredCamFeats(got.depth.clone(), got.ctx.contiguous()))
    assert torch.equal(out, twin) and torch.isfinite(out).all() and out.abs().sum().item() > 0


@pytest.mark.parametrize("kind", ["depth", "lss"])
@torch.no_grad()
def test_graph_replay_bit_equals_eager(dev, kind):
    m = small_transform(kind).to(dev)
    m.cam_nets_dtype = torch.float16
    x, d = (t.to(dev) for t in small_inputs())
    sx, sd = x.clone(), d.clone()
    eager = _call(m, sx, sd)                                   # the warm-up forward: the folds exist now
    e_depth, e_ctx = eager.depth.clone(), eager.ctx.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = _call(m, sx, sd)
    x2, d2 = (t.to(dev) for t in small_inputs(seed=7))
    sx.copy_(x2)
    sd.copy_(d2)
    graph.replay()
    torch.cuda.synchronize()
    other = _call(m, x2, d2)
    assert torch.equal(cap.depth, other.depth) and torch.equal(cap.ctx, other.ctx) and not torch.equal(other.ctx, e_ctx)
    sx.copy_(x)
    sd.copy_(d)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.depth, e_depth) and torch.equal(cap.ctx, e_ctx)


@pytest.mark.parametrize("kind", ["depth", "lss"])
@torch.no_grad()
def test_with_cam_nets_dtype_none_the_module_is_its_torch_layers(dev, kind):
    m = small_transform(kind).to(dev)
    x, d = (t.to(dev) for t in small_inputs())
    assert m.cam_nets_dtype is None and not m.cam_nets_fusable(x, d if kind == "depth" else None)
    got = _call(m, x, d)
    if kind == "depth":
        z = m.depthnet(torch.cat([m.dtransform(d.view(2, 1, 16, 24)), x.view(2, 32, 2, 3)], dim=1))
    else:
        z = m.depthnet(x.view(2, 32, 2, 3))
    assert torch.equal(got.depth, z[:, :5].softmax(dim=1).view(1, 2, 5, 2, 3)) and torch.equal(got.ctx, z[:, 5:9].view(1, 2, 4, 2, 3))


@pytest.mark.parametrize("kind, how", NOT_FUSABLE)
def test_dispatch_keeps_the_torch_layers(dev, kind, how):
    """Every case of tests/test_cam_nets.py with the module and the tensors on the device (but for the host-tensor case): not
    fusable, and get_cam_feats returns what the same module returns with cam_nets_dtype None."""
    m, x, d, grad = unfusable_case(kind, how)
    m = m.to(dev)
    if how != "host":
        x = x.detach().to(dev).requires_grad_(x.requires_grad)
        d = d.to(dev) if d is not None else None
    else:
        m = m.cpu()
    twin = copy.deepcopy(m)
    twin.cam_nets_dtype = None
    with torch.enable_grad() if grad or how == "train" else torch.no_grad():
        assert m.cam_nets_fusable(x, d) is False
        got, want = _call(m, x, d), _call(twin, x, d)
    assert isinstance(got, FactoredCamFeats) and got.depth.dtype == torch.float32
    tol = 1e-5 * (1 + want.ctx.detach().abs().max().item())
    assert (got.depth - want.depth).abs().max().item() <= 1e-5 and (got.ctx - want.ctx).abs().max().item() <= tol
    if grad:
        got.ctx.sum().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all()
    if how in ("train", "grad", "host"):      # the same module does take the kernels once the reason is gone
        m = m.to(dev).eval()
        with torch.no_grad():
            assert m.cam_nets_fusable(x.detach().to(dev), d.to(dev) if d is not None else None)


# ---- the end-to-end observation (recorded, not barred) ---------------------------------------------------------------------------
@torch.no_grad()
def test_end_to_end_error_of_the_four_routes_is_recorded(dev):
    """DepthLSSTransform at the flagship widths (in_channels 256, D 118, C 80) on a 64 x 136 image, B = 1, N = 2: the largest error of
    depth and of context against the float64 chain of the fp32 master parameters, normalised by the output's largest magnitude."""
    cfg = dict(SMALL, out_channels=80, image_size=(64, 136), feature_size=(8, 17), dbound=[1.0, 60.0, 0.5])
    m = randomise(DepthLSSTransform(in_channels=256, **cfg), 5).eval()
    assert (m.D, m.C) == (118, 80)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 2, 256, 8, 17, generator=g)
    d = torch.where(torch.rand(1, 2, 1, 64, 136, generator=g) < 0.3, 60.0 * torch.rand(1, 2, 1, 64, 136, generator=g), torch.zeros(()))
    ref_depth, ref_ctx = _chain64(m, x, d)
    m = m.to(dev)
    xd, dd = x.to(dev), d.to(dev)
    routes = {}
    for name, dtype in (("fused_fp16", torch.float16), ("fused_bf16", torch.bfloat16)):
        m.cam_nets_dtype = dtype
        assert m.cam_nets_fusable(xd, dd)
        routes[name] = m.get_cam_feats(xd, dd)
    m.cam_nets_dtype = None
    routes["torch_fp32"] = m.get_cam_feats(xd, dd)
    with torch.autocast("cuda", dtype=torch.float16):
        routes["torch_autocast_fp16"] = copy.deepcopy(m).to(memory_format=torch.channels_last).get_cam_feats(xd, dd)
    out = {}
    for name, r in routes.items():
        e_depth = (r.depth.cpu().double().view(2, 118, 8, 17) - ref_depth).abs().max().item() / ref_depth.abs().max().item()
        e_ctx = (r.ctx.cpu().double().reshape(2, 80, 8, 17) - ref_ctx).abs().max().item() / ref_ctx.abs().max().item()
        out[name] = dict(depth=e_depth, context=e_ctx)
        print(f"end to end {name}: depth {e_depth:.3e}, context {e_ctx:.3e} (of the output's largest magnitude)")
        assert math.isfinite(e_depth) and math.isfinite(e_ctx)
    _update_observed("end_to_end", "in256_D118_C80_8x17", out)
