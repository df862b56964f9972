"""The Bottleneck tail (`bevamd_bottleneck_tail_forward`), the stem (`bevamd_resnet_stem_forward`) and the camera `ResNet` over them on
the device, pinned to float64 on the CPU.

Every tail is compared with float64 computed from the exact 16-bit operand values and the fold's own fp32 scales and shifts:

    ref = relu(s3 * conv64(h, W3) + t3 + R)         mag = |s3| * conv64(|h|, |W3|) + |t3| + M
    identity:   R = x                               M = |x|
    downsample: R = sd * conv64(x, Wd) + td         M = |sd| * conv64(|x|, |Wd|) + |td|
    |y - ref| <= 1.01 * (u * |ref| + (K + 8) * 2^-23 * mag) + d

u = 2^-11 (fp16) or 2^-8 (bf16) is the one rounding to the storage type, K the length of the sums (P, plus Cx with a downsample),
2^-23 per term covers any fp32 summation order, a non-nearest rounding inside the MFMA and the two fp32 operations of the epilogue,
d = 2^-24 is fp16's subnormal step (0 for bf16).  The bar is DESIGN 3.23's, derived, not tuned.  The stem's reference is
max_pool2d(relu(s * conv64(x, W) + t)) with K = 147 and mag the MAXIMUM of the convolution's mag over the pooling window, since
|max a - max b| <= max |a - b|.  The exact cases (small integers, power-of-two scales, integer shifts) have no tolerance at all.

The tail kernel's pixel tile is 128 consecutive FLAT pixels of the batch ((b OH + oy) OW + ox).  With B = 2 the 1 x 127 output ends
sample 0 one pixel short of the first tile edge and the 3 x 43 output (129 pixels) carries it one pixel past, so a tile holds pixels
of both samples.  The stem kernel's pooled tile is 4 x 15: the 18 x 62 image pools to 5 x 16, one past the tile on both axes (16 x
64 pools to 4 x 16).

The observed end-to-end errors are written to profiles/cam_resnet_observed.json.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from bevfusion_amd import _capi, bev_resnet as br, bev_trunk as bt, cam_resnet as cr
from conftest import record_parity
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
D = {torch.float16: 2.0 ** -24, torch.bfloat16: 0.0}
DTYPES = [torch.float16, torch.bfloat16]
# (h layout, x layout, dst layout)
LAYOUTS = [(hl, xl, dl) for hl in ("nhwc", "nchw") for xl in ("nchw", "nhwc") for dl in ("nhwc", "nchw")]
OUT_MAPS = [(1, 1), (3, 5), (8, 16), (9, 17), (17, 33)]
S2_MAPS = [(1, 1), (5, 9), (8, 8), (9, 9), (16, 32), (18, 34), (17, 33)]          # stride 2: the map of x
ALL_LAYOUTS_ON = [(9, 17), (3, 5)]
EDGE_MAPS = {1: [(1, 127), (3, 43)], 2: [(1, 253), (5, 85)]}                        # outputs 1 x 127 and 3 x 43: see the docstring


def _out_map(xmap, s):
    return ((xmap[0] - 1) // s + 1, (xmap[1] - 1) // s + 1)


def _cases():
    """(mode, stride, map of x, P, C, Cx, layouts)."""
    out = []
    for mode, s, maps in (("identity", 1, OUT_MAPS), ("down", 1, OUT_MAPS), ("down", 2, S2_MAPS)):
        full_done = set()
        for xmap in maps:
            om = _out_map(xmap, s)
            if om in ALL_LAYOUTS_ON and om not in full_done:
                full_done.add(om)
                out += [(mode, s, xmap, 16, 64, 64, lay) for lay in LAYOUTS]
            else:
                out.append((mode, s, xmap, 16, 64, 64, LAYOUTS[len(out) % 8]))
        xm = (9, 17) if s == 1 else (17, 33)
        for p, c, cx in ((32, 128, 64), (48, 160, 48)):
            out.append((mode, s, xm, p, c, c if mode == "identity" else cx, LAYOUTS[len(out) % 8]))
        if mode == "identity":
            out.append((mode, s, xm, 64, 256, 256, LAYOUTS[len(out) % 8]))
        if s == 2:
            out.append((mode, s, (6, 9), 128, 512, 256, LAYOUTS[len(out) % 8]))         # the real widths of layer2's first block
        for xmap in EDGE_MAPS[s]:
            out.append((mode, s, xmap, 16, 64, 64, LAYOUTS[len(out) % 8]))
    return out


CASES = _cases()
IDS = ["%s%d-%dx%d-%d-%dto%d-%s-%s-%s" % (m, s, xm[0], xm[1], p, cx, c, l[0], l[1], l[2]) for m, s, xm, p, c, cx, l in CASES]


# ---- data and the float64 reference ----------------------------------------------------------------------------------------------
def _random_block(seed, mode, s, xmap, P, C, Cx, dtype, B=2):
    g = torch.Generator().manual_seed(seed)
    om = _out_map(xmap, s)
    h = torch.randn((B, P) + om, generator=g).to(dtype)
    x = torch.randn((B, Cx) + tuple(xmap), generator=g).to(dtype)
    w3 = (torch.randn((C, P, 1, 1), generator=g) / P ** 0.5).to(dtype)
    wd = (torch.randn((C, Cx, 1, 1), generator=g) / Cx ** 0.5).to(dtype) if mode == "down" else None

    def affine():
        scale = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
        return scale.float(), (0.5 * torch.randn(C, generator=g)).float()
    s3, t3 = affine()
    sd, td = affine() if mode == "down" else (None, None)
    return dict(h=h, x=x, w3=w3, wd=wd, s3=s3, t3=t3, sd=sd, td=td, mode=mode, stride=s)


def _exact_block(seed, mode, s, xmap, P, C, Cx, dtype, B=2):
    """Integers in [-2, 2] with no symmetry in any axis (a fixed random draw), power-of-two scales (some negative), integer shifts."""
    g = torch.Generator().manual_seed(1000 + seed)
    om = _out_map(xmap, s)
    h = torch.randint(-2, 3, (B, P) + om, generator=g).to(dtype)
    x = torch.randint(-2, 3, (B, Cx) + tuple(xmap), generator=g).to(dtype)
    w3 = torch.randint(-2, 3, (C, P, 1, 1), generator=g).to(dtype)
    wd = torch.randint(-2, 3, (C, Cx, 1, 1), generator=g).to(dtype) if mode == "down" else None
    s3 = torch.tensor([2.0 ** ((c % 4) - 2) * (-1.0 if c % 5 == 3 else 1.0) for c in range(C)])
    t3 = torch.tensor([float((c * 7) % 9 - 3) for c in range(C)])
    sd = torch.tensor([2.0 ** (((c + 1) % 3) - 1) * (-1.0 if c % 7 == 2 else 1.0) for c in range(C)]) if mode == "down" else None
    td = torch.tensor([float((c * 5) % 7 - 2) for c in range(C)]) if mode == "down" else None
    return dict(h=h, x=x, w3=w3, wd=wd, s3=s3, t3=t3, sd=sd, td=td, mode=mode, stride=s)


def _d(t):
    return t.detach().cpu().double()


def _c(t):
    return _d(t).view(1, -1, 1, 1)


def _ref64(blk):
    """-> (ref, mag, v, r) in float64 from the exact operand values; v: the conv3 + bn3 term, r: the residual term."""
    h, x = _d(blk["h"]), _d(blk["x"])
    v = _c(blk["s3"]) * F.conv2d(h, _d(blk["w3"])) + _c(blk["t3"])
    mag = _c(blk["s3"]).abs() * F.conv2d(h.abs(), _d(blk["w3"]).abs()) + _c(blk["t3"]).abs()
    if blk["mode"] == "identity":
        r, m = x, x.abs()
    else:
        r = _c(blk["sd"]) * F.conv2d(x, _d(blk["wd"]), stride=blk["stride"]) + _c(blk["td"])
        m = _c(blk["sd"]).abs() * F.conv2d(x.abs(), _d(blk["wd"]).abs(), stride=blk["stride"]) + _c(blk["td"]).abs()
    return torch.relu(v + r), mag + m, v, r


def _bar(ref, mag, K, dtype):
    return 1.01 * (U[dtype] * ref.abs() + (K + 8) * 2.0 ** -23 * mag) + D[dtype]


def _sum_length(blk):
    return blk["w3"].shape[1] + (blk["x"].shape[1] if blk["mode"] == "down" else 0)


def _make_fold(blk, dev):
    C, P = blk["w3"].shape[:2]
    down = blk["mode"] == "down"
    on = lambda t: t.to(dev) if t is not None else None      # noqa: E731
    return cr.FoldedBottleneckTail(bt.bev_pack_weight(blk["w3"]).to(dev), on(blk["s3"]), on(blk["t3"]),
                                   bt.bev_pack_weight(blk["wd"]).to(dev) if down else None, on(blk["sd"]), on(blk["td"]), P, C,
                                   blk["x"].shape[1], "downsample" if down else "identity", blk["stride"])


def _to_layout(t, layout, dev):
    t = t.to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t.contiguous()


def check_inputs_are_telling(blk, ref, v, r):
    """A condition on the DATA (checked on the CPU, before anything runs on the device): the ReLU cuts, the shifts matter, and in
    the identity cases a dropped residual changes the sign under the ReLU at one output in ten at least."""
    frac = (ref > 0).double().mean().item()
    assert 0.25 <= frac <= 0.75, frac
    assert (blk["t3"] > 0).double().mean().item() >= 0.25
    if blk["mode"] == "down":
        assert (blk["td"] > 0).double().mean().item() >= 0.25
    else:
        flips = (((v < 0) & (v + r > 0)) | ((v + r < 0) & (v > 0))).double().mean().item()
        assert flips >= 0.10, flips


def _run(blk, lay, dev):
    y = cr.bottleneck_tail_forward(_to_layout(blk["h"], lay[0], dev), _to_layout(blk["x"], lay[1], dev), _make_fold(blk, dev), out_layout=lay[2])
    B, C = blk["h"].shape[0], blk["w3"].shape[0]
    assert y is not None and y.dtype == blk["h"].dtype and tuple(y.shape) == (B, C) + tuple(blk["h"].shape[2:])
    assert y.is_contiguous() if lay[2] == "nchw" else y.is_contiguous(memory_format=torch.channels_last)
    return y


# ---- the tail --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tail_against_float64(dev, case, dtype):
    mode, s, xmap, P, C, Cx, lay = case
    blk = _random_block(CASES.index(case), mode, s, xmap, P, C, Cx, dtype)
    ref, mag, v, r = _ref64(blk)
    check_inputs_are_telling(blk, ref, v, r)
    y = _run(blk, lay, dev)
    err, bar = (y.cpu().double() - ref).abs(), _bar(ref, mag, _sum_length(blk), dtype)
    worst = (err / bar).max().item()
    print(f"{IDS[CASES.index(case)]} {dtype}: worst error / bar = {worst:.3f}")
    record_parity(f"bottleneck_tail/{mode}{s}/{dtype}", worst, 1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tail_is_exact_on_integers(dev, case, dtype):
    mode, s, xmap, P, C, Cx, lay = case
    blk = _exact_block(CASES.index(case), mode, s, xmap, P, C, Cx, dtype)
    ref, _, v, r = _ref64(blk)
    assert 0.25 <= (ref > 0).double().mean().item() <= 0.75
    assert ref.abs().max().item() < 2.0 ** 15          # inside the finite range of fp16; fp32 holds every partial sum exactly
    y = _run(blk, lay, dev)
    want = ref.to(dtype)          # the sums are quarter-integers below 2^22: fp32 holds them exactly, so one rounding of the same real number
    got = y.cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), (got.double() - ref).abs().max().item()


def test_the_functionals_return_none_where_the_entry_points_refuse_the_sizes(dev):
    """Code 4 comes back as None, with no launch; a fold that does not fit the tensors raises."""
    for P, C, Cx, mode in ((16, 48, 48, "identity"), (24, 64, 64, "identity"), (16, 64, 24, "down")):
        blk = _random_block(3, mode, 1, (5, 7), P, C, Cx, torch.float16)
        assert cr.bottleneck_tail_forward(blk["h"].to(dev), blk["x"].to(dev), _make_fold(blk, dev)) is None
        assert "not supported" in _capi.last_error()
    blk = _random_block(3, "identity", 1, (5, 7), 16, 64, 64, torch.float16)
    with pytest.raises(RuntimeError, match="do not fit the fold"):
        cr.bottleneck_tail_forward(blk["h"].to(dev), blk["x"][:, :32].to(dev), _make_fold(blk, dev))
    with pytest.raises(RuntimeError, match="one dtype"):
        cr.bottleneck_tail_forward(blk["h"].to(dev), blk["x"].to(dev).bfloat16(), _make_fold(blk, dev))
    st = _stem_data(0, (7, 9), torch.float16)
    fold = _stem_fold(st, dev)
    assert cr.stem_forward(torch.zeros(1, 4, 7, 9, dtype=torch.float16, device=dev), fold) is None and "not supported" in _capi.last_error()
    with pytest.raises(RuntimeError, match="the tensor is"):
        cr.stem_forward(st["x"].to(dev).bfloat16(), fold)


# ---- the stem --------------------------------------------------------------------------------------------------------------------
STEM_MAPS = [(1, 1), (2, 3), (7, 9), (13, 15), (16, 64), (18, 66), (37, 135), (18, 62)]


def _stem_data(seed, hw, dtype, exact=False, B=2):
    g = torch.Generator().manual_seed(77 + seed)
    if exact:
        x = torch.randint(-2, 3, (B, 3) + tuple(hw), generator=g).to(dtype)
        w = torch.randint(-2, 3, (64, 3, 7, 7), generator=g).to(dtype)
        s = torch.tensor([2.0 ** ((c % 4) - 2) * (-1.0 if c % 5 == 3 else 1.0) for c in range(64)])
        t = torch.tensor([float((c * 7) % 9 - 3) for c in range(64)])
    else:
        x = torch.randn((B, 3) + tuple(hw), generator=g).to(dtype)
        w = (torch.randn((64, 3, 7, 7), generator=g) / 147 ** 0.5).to(dtype)
        s = ((0.5 + torch.rand(64, generator=g)) * torch.where(torch.rand(64, generator=g) < 0.25, -1.0, 1.0)).float()
        t = (0.3 * torch.randn(64, generator=g)).float()
    return dict(x=x, w=w, s=s, t=t)


def _stem_fold(st, dev):
    return cr.FoldedStem(cr.stem_pack_weight(st["w"]).to(dev), st["s"].to(dev), st["t"].to(dev))


def _stem_ref64(st):
    """-> (ref, mag, a, idx): the pooled reference, the window maximum of the convolution's mag, the conv map after the ReLU and
    max_pool2d's argmax indices."""
    x, w = _d(st["x"]), _d(st["w"])
    pre = _c(st["s"]) * F.conv2d(x, w, stride=2, padding=3) + _c(st["t"])
    mag = _c(st["s"]).abs() * F.conv2d(x.abs(), w.abs(), stride=2, padding=3) + _c(st["t"]).abs()
    a = torch.relu(pre)
    ref, idx = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    return ref, F.max_pool2d(mag, 3, 2, 1), pre, idx


def check_stem_inputs_are_telling(pre, idx):
    frac = (pre > 0).double().mean().item()
    assert 0.25 <= frac <= 0.75, frac
    OH, OW = pre.shape[2:]
    PH, PW = idx.shape[2:]
    phs = [p for p in range(PH) if 2 * p - 1 >= 0 and 2 * p + 1 <= OH - 1]
    pws = [p for p in range(PW) if 2 * p - 1 >= 0 and 2 * p + 1 <= OW - 1]
    if len(phs) < 4 or len(pws) < 4:
        return False
    ph = torch.tensor(phs).view(1, 1, -1, 1)
    pw = torch.tensor(pws).view(1, 1, 1, -1)
    sub = idx[:, :, phs][:, :, :, pws]
    pos = (sub // OW - (2 * ph - 1)) * 3 + (sub % OW - (2 * pw - 1))
    share = torch.bincount(pos.reshape(-1), minlength=9).double() / pos.numel()
    assert pos.min().item() >= 0 and pos.max().item() <= 8 and share.min().item() >= 0.05, share
    return True


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("hw", STEM_MAPS, ids=["%dx%d" % m for m in STEM_MAPS])
def test_stem_against_float64(dev, hw, dtype, layout):
    st = _stem_data(STEM_MAPS.index(hw), hw, dtype)
    ref, mag, pre, idx = _stem_ref64(st)
    checked = check_stem_inputs_are_telling(pre, idx)
    assert checked == (hw == (37, 135))                       # the one map with a 4 x 4 interior of whole windows
    y = cr.stem_forward(st["x"].to(dev), _stem_fold(st, dev), out_layout=layout)
    assert y is not None and y.dtype == dtype and tuple(y.shape) == tuple(ref.shape)
    assert y.is_contiguous() if layout == "nchw" else y.is_contiguous(memory_format=torch.channels_last)
    worst = ((y.cpu().double() - ref).abs() / _bar(ref, mag, 147, dtype)).max().item()
    print(f"stem {hw} {dtype} {layout}: worst error / bar = {worst:.3f}")
    record_parity(f"resnet_stem/{dtype}", worst, 1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("hw", STEM_MAPS, ids=["%dx%d" % m for m in STEM_MAPS])
def test_stem_is_exact_on_integers(dev, hw, dtype, layout):
    st = _stem_data(STEM_MAPS.index(hw), hw, dtype, exact=True)
    ref, _, pre, _ = _stem_ref64(st)
    assert 0.2 <= (pre > 0).double().mean().item() <= 0.8 and pre.abs().max().item() < 2 * 600 + 6
    y = cr.stem_forward(st["x"].to(dev), _stem_fold(st, dev), out_layout=layout)
    want, got = ref.to(dtype), y.cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), (got.double() - ref).abs().max().item()


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------
def _raw_tail(h, h_nhwc, x, x_nhwc, fold, out, out_nhwc, shape, xshape):
    B, C, OH, OW = shape
    down = fold.residual == "downsample"
    with torch.cuda.device(h.device):
        return _capi.load().bevamd_bottleneck_tail_forward(
            _capi.ptr(h), h_nhwc, fold.planes, _capi.ptr(x), x_nhwc, xshape[1], xshape[2], xshape[3], 0 if h.dtype == torch.float16 else 1,
            B, C, OH, OW, int(down), fold.stride, _capi.ptr(fold.packed3), fold.packed3.numel(), _capi.ptr(fold.scale3),
            _capi.ptr(fold.shift3), _capi.ptr(fold.packed_d) if down else None, fold.packed_d.numel() if down else 0,
            _capi.ptr(fold.scale_d) if down else None, _capi.ptr(fold.shift_d) if down else None, _capi.ptr(out), out_nhwc, out.numel(),
            _capi.stream_ptr(h.device))


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("mode, s, xmap, lay", [("identity", 1, (3, 5), ("nhwc", "nchw", "nhwc")), ("identity", 1, (3, 43), ("nchw", "nhwc", "nchw")),
                                                ("down", 1, (3, 5), ("nchw", "nhwc", "nchw")), ("down", 1, (3, 43), ("nhwc", "nchw", "nhwc")),
                                                ("down", 2, (5, 9), ("nhwc", "nhwc", "nchw")), ("down", 2, (5, 85), ("nchw", "nchw", "nhwc"))])
def test_tail_guarded_buffers_of_exact_size(dev, mode, s, xmap, lay, fill):
    """h, x, both weights, the scales, the shifts and dst carved from one arena filled with a dirty byte (0xFF: NaN halves), each of
    its exact size: no guard byte changes, the inputs are unchanged, every output element is written, and the result bit-equals
    an unguarded call's."""
    dtype = torch.float16
    blk = _random_block(31, mode, s, xmap, 16, 64, 64 if mode == "identity" else 48, dtype)
    fold = _make_fold(blk, dev)
    plain = _run(blk, lay, dev)
    arena = Arena(dev, fill, capacity=16 << 20)

    def carve(t, layout, name):     # the kernel's own element order, exactly its bytes
        return arena.put(t.to(dev).permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else t.to(dev).contiguous(), name)
    gh, gx = carve(blk["h"], lay[0], "h"), carve(blk["x"], lay[1], "x")
    gfold = copy.copy(fold)
    gfold.packed3, gfold.scale3, gfold.shift3 = arena.put(fold.packed3, "packed3"), arena.put(fold.scale3, "scale3"), arena.put(fold.shift3, "shift3")
    if mode == "down":
        gfold.packed_d, gfold.scale_d, gfold.shift_d = arena.put(fold.packed_d, "packed_d"), arena.put(fold.scale_d, "scale_d"), arena.put(fold.shift_d, "shift_d")
    B, C, OH, OW = plain.shape
    out = arena.out((B, OH, OW, C) if lay[2] == "nhwc" else (B, C, OH, OW), dtype, "out")
    before = [t.clone() for t in (gh, gx, gfold.packed3, gfold.scale3, gfold.shift3)]
    rc = _raw_tail(gh, int(lay[0] == "nhwc"), gx, int(lay[1] == "nhwc"), gfold, out, int(lay[2] == "nhwc"), (B, C, OH, OW), tuple(blk["x"].shape))
    assert rc == 0, _capi.last_error()
    arena.check()
    assert all(torch.equal(a, b) for a, b in zip(before, (gh, gx, gfold.packed3, gfold.scale3, gfold.shift3)))
    if mode == "down":
        assert torch.equal(gfold.packed_d, fold.packed_d) and torch.equal(gfold.scale_d, fold.scale_d) and torch.equal(gfold.shift_d, fold.shift_d)
    logical = out.permute(0, 3, 1, 2) if lay[2] == "nhwc" else out
    assert torch.equal(logical.contiguous().view(torch.int16), plain.contiguous().view(torch.int16))
    assert not torch.isnan(out).any()


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("hw, layout", [((7, 9), "nhwc"), ((37, 135), "nchw"), ((37, 135), "nhwc")])
def test_stem_guarded_buffers_of_exact_size(dev, hw, layout, fill):
    dtype = torch.float16
    st = _stem_data(5, hw, dtype)
    fold = _stem_fold(st, dev)
    plain = cr.stem_forward(st["x"].to(dev), fold, out_layout=layout)
    arena = Arena(dev, fill, capacity=16 << 20)
    gx = arena.put(st["x"].to(dev).contiguous(), "x")
    gp, gs, gt = arena.put(fold.packed, "packed"), arena.put(fold.scale, "scale"), arena.put(fold.shift, "shift")
    B, C, PH, PW = plain.shape
    out = arena.out((B, PH, PW, C) if layout == "nhwc" else (B, C, PH, PW), dtype, "out")
    before = [t.clone() for t in (gx, gp, gs, gt)]
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_resnet_stem_forward(_capi.ptr(gx), 0, B, 3, hw[0], hw[1], 64, 7, 2, 3, 3, 2, 1, 0, _capi.ptr(gp), gp.numel(),
                                                     _capi.ptr(gs), _capi.ptr(gt), _capi.ptr(out), int(layout == "nhwc"), out.numel(),
                                                     _capi.stream_ptr(dev))
    assert rc == 0, _capi.last_error()
    arena.check()
    assert all(torch.equal(a, b) for a, b in zip(before, (gx, gp, gs, gt)))
    logical = out.permute(0, 3, 1, 2) if layout == "nhwc" else out
    assert torch.equal(logical.contiguous().view(torch.int16), plain.contiguous().view(torch.int16))
    assert not torch.isnan(out).any()


# ---- the module ------------------------------------------------------------------------------------------------------------------
SMALL = dict(depth=50, base_channels=32, stem_channels=64, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1))


def _randomise(module, seed):
    """Weights that keep the activations' scale through the chain (variance 2 / K), BatchNorm statistics that are not the defaults."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                K = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / K) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.8 + 0.4 * torch.rand(n, generator=g))
                m.bias.copy_(0.3 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=g))
    return module


def _all_on(net):
    net.use_fused, net.fused_stem, net.fused_stride2 = True, True, True      # every part through a kernel, whatever the measured defaults
    net.fused_tails = ("identity", "down1", "down2")
    return net


def _net(dtype, dev, seed=1, **kwargs):
    return _all_on(_randomise(cr.ResNet(**dict(SMALL, **kwargs)), seed).to(dev).to(dtype).eval())


def _input(dtype, dev, B=2, hw=(33, 47), seed=5):
    return torch.randn((B, 3) + hw, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def _conv_node(x, conv, bn, dtype, nodes):
    fold = bt.fold_bev_layer(conv, bn)
    h = bt.bev_conv_forward([x], fold, out_layout="nhwc")
    assert h is not None
    s, t = _c(fold.scale), _c(fold.shift)
    ref = torch.relu(s * F.conv2d(_d(x), _d(conv.weight), stride=conv.stride, padding=conv.padding) + t)
    mag = s.abs() * F.conv2d(_d(x).abs(), _d(conv.weight).abs(), stride=conv.stride, padding=conv.padding) + t.abs()
    K = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
    nodes.append(((h.cpu().double() - ref).abs() / _bar(ref, mag, K, dtype)).max().item())
    return h


def _functional_bottleneck(blk, x, dtype, nodes):
    """One Bottleneck through the three functionals, each node checked against float64 of that node's OWN input."""
    h = _conv_node(x, blk.conv1, blk.bn1, dtype, nodes)
    h = _conv_node(h, blk.conv2, blk.bn2, dtype, nodes)
    fold = cr.fold_bottleneck(blk)
    y = cr.bottleneck_tail_forward(h, x, fold, out_layout="nhwc")
    assert y is not None
    down = blk.downsample is not None
    data = dict(h=h, x=x, w3=blk.conv3.weight, wd=blk.downsample[0].weight if down else None, s3=fold.scale3, t3=fold.shift3,
                sd=fold.scale_d, td=fold.shift_d, mode="down" if down else "identity", stride=fold.stride)
    ref, mag, _, _ = _ref64(data)
    nodes.append(((y.cpu().double() - ref).abs() / _bar(ref, mag, _sum_length(data), dtype)).max().item())
    return y


def _functional_stem(net, x, dtype, nodes):
    fold = cr.fold_stem(net.conv1, net.bn1, net.maxpool)
    y = cr.stem_forward(x, fold, out_layout="nhwc")
    assert y is not None
    ref, mag, _, _ = _stem_ref64(dict(x=x, w=net.conv1.weight, s=fold.scale, t=fold.shift))
    nodes.append(((y.cpu().double() - ref).abs() / _bar(ref, mag, 147, dtype)).max().item())
    return y


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "bf16"])
def chain(request, dev):
    """The two-stage ResNet-50 variant (seven Bottlenecks: a stride-1 downsample, a stride-2 downsample and five identity tails) on
    2 x 3 x 33 x 47, driven node by node through the functionals; computed once and shared."""
    dtype = request.param
    net = _net(dtype, dev)
    x = _input(dtype, dev)
    nodes, stages = [], []
    with torch.no_grad():
        y = _functional_stem(net, x, dtype, nodes)
        for stage in net._stages():
            for blk in stage:
                y = _functional_bottleneck(blk, y, dtype, nodes)
            stages.append(y)
    return dict(dtype=dtype, net=net, x=x, stages=stages, nodes=nodes)


def test_every_node_of_the_chain_against_float64(chain):
    net = chain["net"]
    assert len(chain["nodes"]) == 1 + 3 * 7
    assert sorted(cr._tail_class(cr.bottleneck_spec(b)) for b in net._all_blocks()) == ["down1", "down2"] + ["identity"] * 5
    print("worst error / bar per node:", ["%.3f" % v for v in chain["nodes"]])
    for i, v in enumerate(chain["nodes"]):
        record_parity(f"cam_resnet/node{i}/{chain['dtype']}", v, 1.0)
    assert max(chain["nodes"]) <= 1.0, chain["nodes"]


@torch.no_grad()
def test_module_forward_bit_equals_the_functional_chain(chain):
    net, x, dtype = chain["net"], chain["x"], chain["dtype"]
    assert net.fusable(x)
    outs = net(x)
    assert isinstance(outs, tuple) and [tuple(t.shape) for t in outs] == [(2, 128, 9, 12), (2, 256, 5, 6)]
    assert all(t.dtype == dtype and t.is_contiguous(memory_format=torch.channels_last) for t in outs)
    assert all(torch.equal(a, b) for a, b in zip(outs, chain["stages"]))
    # an input with channels-last strides gives the same bits as the contiguous one
    assert all(torch.equal(a, b) for a, b in zip(net(x.contiguous(memory_format=torch.channels_last)), outs))


def _observed(update):
    path = os.path.join(ROOT, "profiles", "cam_resnet_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(update)
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass      # a read-only checkout: the figures are printed


def test_end_to_end_error_is_within_twice_the_torch_layers_own(chain, dev):
    """Both paths against the float64 twin of the same 16-bit parameters; errors normalised by the output's largest magnitude.  The
    fused path rounds once per kernel where torch rounds after every convolution, BatchNorm, pooling and add."""
    net, x, dtype = chain["net"], chain["x"], chain["dtype"]
    m64 = copy.deepcopy(net).cpu().double()
    twin = copy.deepcopy(net)
    twin.use_fused = False
    with torch.no_grad():
        ref = m64(x.cpu().double())[-1]
        assert not twin.fusable(x)
        y_torch, y_fused = twin(x)[-1], net(x)[-1]
    top = ref.abs().max().item()
    e_fused = (y_fused.cpu().double() - ref).abs().max().item() / top
    e_torch = (y_torch.cpu().double() - ref).abs().max().item() / top
    print(f"{dtype}: fused {e_fused:.3e}, torch layers {e_torch:.3e}, ratio {e_fused / e_torch:.3f}")
    record_parity(f"cam_resnet/end_to_end/{dtype}", e_fused, 2 * e_torch)
    _observed({str(dtype): dict(fused=e_fused, torch_layers=e_torch, ratio=e_fused / e_torch, bar_ratio=2.0,
                                nodes_worst_error_over_bar=chain["nodes"])})
    assert e_fused <= 2 * e_torch, (e_fused, e_torch)


def _spread_bar(y, dtype):
    """Two runs of the SAME torch layers may pick another algorithm, i.e. another summation order: a few roundings of the storage
    type at the output's scale per layer."""
    return 8 * U[dtype] * y.abs().max().item()


@pytest.mark.parametrize("how", ["train", "fp32", "requires_grad", "use_fused_false", "norm_eval_false_train"])
def test_dispatch_takes_the_torch_layers(dev, how):
    dtype = torch.float32 if how == "fp32" else torch.float16
    # The case that normalises with batch statistics compares two runs of torch's OWN layers, which on this backend do not repeat
    # their bits (the eval cases differ by up to 5 u of the top too).  Every train-mode BatchNorm brings the map back to unit scale,
    # so the differences of all layers before it stay at the output's scale instead of shrinking against a growing top: the bar of
    # "a few roundings per layer" is for a few layers, and this case runs ONE stage (three Bottlenecks, ten BatchNorms) on maps of
    # 16 x 24, 768 samples a channel, so that no statistic rests on a handful of pixels.
    stage1 = dict(num_stages=1, strides=(1,), dilations=(1,), out_indices=(0,)) if how == "norm_eval_false_train" else {}
    net = _net(dtype, dev, seed=4, norm_eval=how != "norm_eval_false_train", **stage1)
    x = _input(dtype, dev, hw=(64, 96) if how == "norm_eval_false_train" else (21, 19), seed=1)
    net.use_fused = how != "use_fused_false"
    twin = copy.deepcopy(net)
    twin.use_fused = False
    if how in ("train", "norm_eval_false_train"):
        net.train()
        twin.train()
    if how == "requires_grad":
        x.requires_grad_(True)
    with torch.enable_grad() if how in ("train", "requires_grad", "norm_eval_false_train") else torch.no_grad():
        assert not net.fusable(x)
        got, want = net(x), twin(x)
    assert isinstance(got, tuple) and len(got) == len(net.out_indices) == len(want)
    for a, b in zip(got, want):
        diff = (a.detach().float() - b.detach().float()).abs().max().item()
        print(f"{how}: largest difference {diff:.3e}, bar {_spread_bar(b.detach().float(), torch.float16):.3e}")
        assert diff <= _spread_bar(b.detach().float(), torch.float16)
    if how == "requires_grad":
        got[-1].float().sum().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all()
    if how == "train":               # norm_eval: the statistics stay
        assert int(net.layer1[0].bn1.num_batches_tracked) == 0 and not net.bn1.training
    if how == "norm_eval_false_train":
        assert int(net.layer1[0].bn1.num_batches_tracked) == 1 and int(net.bn1.num_batches_tracked) == 1
    if how != "fp32":                # the same module does take the kernels once the reason is gone
        net.eval()
        net.use_fused = True
        with torch.no_grad():
            assert net.fusable(x.detach())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_class_switches_send_their_part_to_torch_inside_the_fused_chain(dev, dtype):
    net = _net(dtype, dev, seed=12)
    x = _input(dtype, dev, seed=4)
    full = net(x)
    want = copy.deepcopy(net)
    want.use_fused = False
    want = want(x)
    for switch in (dict(fused_stem=False), dict(fused_stride2=False), dict(fused_tails=("down1", "down2")), dict(fused_tails=("identity", "down2")),
                   dict(fused_tails=("identity", "down1")), dict(fused_tails=())):
        part = copy.deepcopy(net)
        for k, v in switch.items():
            setattr(part, k, v)
        assert part.fusable(x), switch
        outs = part(x)
        for a, b, c in zip(outs, full, want):
            assert tuple(a.shape) == tuple(b.shape) and a.dtype == dtype
            top = c.float().abs().max().item()
            assert (a.float() - b.float()).abs().max().item() <= 16 * U[dtype] * top, switch
            assert (a.float() - c.float()).abs().max().item() <= 16 * U[dtype] * top, switch
    # a switched-off stem is exactly the torch stem in front of the functional chain
    part = copy.deepcopy(net)
    part.fused_stem = False
    y = bt._as_source(part.maxpool(part.relu(part.bn1(part.conv1(x)))))
    for blk in part.layer1:
        y = _functional_bottleneck(blk, y, dtype, [])
    assert torch.equal(part(x)[0], y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_parts_the_kernels_do_not_serve_run_through_torch_inside_the_chain(dev, dtype):
    """A dilated second stage (conv2 through torch), a caffe-style net (the stride-2 conv1 through torch) and a 3 x 3 stem."""
    x = _input(dtype, dev, seed=3)
    for kwargs, blocked in ((dict(dilations=(1, 2), strides=(1, 1)), "conv2"), (dict(style="caffe"), "conv1")):
        net = _net(dtype, dev, seed=11, **kwargs)
        blk = net.layer2[0]
        assert bt.layer_spec(getattr(blk, blocked), blk.bn1) is None and cr.bottleneck_spec(blk) is not None and net.fusable(x)
        got = net(x)
        twin = copy.deepcopy(net)
        twin.use_fused = False
        want = twin(x)
        for a, b in zip(got, want):
            assert tuple(a.shape) == tuple(b.shape)
            assert (a.float() - b.float()).abs().max().item() <= 16 * U[dtype] * b.float().abs().max().item()
    net = _net(dtype, dev, seed=13)
    net.conv1 = torch.nn.Conv2d(3, 64, 3, 2, 1, bias=False).to(dev).to(dtype)
    assert cr.stem_spec(net.conv1, net.bn1, net.maxpool) is None and net.fusable(x)
    twin = copy.deepcopy(net)
    twin.use_fused = False
    for a, b in zip(net(x), twin(x)):
        assert (a.float() - b.float()).abs().max().item() <= 16 * U[dtype] * b.float().abs().max().item()
    # nothing left for a kernel: 24 planes (conv1, conv2 and the tail's P off the multiples) behind a 3 x 3 stem
    bare = _randomise(cr.ResNet(depth=50, base_channels=24, stem_channels=40, num_stages=1, strides=(1,), dilations=(1,), out_indices=(0,)), 2)
    bare = _all_on(bare.to(dev).to(dtype).eval())
    assert not bare.fusable(x) and tuple(bare(x)[0].shape) == (2, 96, 9, 12)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_depth_18_runs_its_basic_blocks_through_res_block_forward(dev, dtype):
    net = _all_on(_randomise(cr.ResNet(depth=18, base_channels=32, stem_channels=64, num_stages=2, strides=(1, 2), dilations=(1, 1),
                                       out_indices=(0, 1)), 6).to(dev).to(dtype).eval())
    x = _input(dtype, dev, seed=8)
    assert net.fusable(x) and all(type(b) is br.BasicBlock and br.res_block_spec(b) is not None for b in net._all_blocks())
    got = net(x)
    y = cr.stem_forward(x, cr.fold_stem(net.conv1, net.bn1, net.maxpool))
    stages = []
    for stage in net._stages():
        for blk in stage:                                   # GeneralizedResNet's functional block
            h = bt.bev_conv_forward([y], bt.fold_bev_layer(blk.conv1, blk.bn1), out_layout="nhwc")
            y = br.res_block_forward(h, y, br.fold_res_block(blk), out_layout="nhwc")
        stages.append(y)
    assert [tuple(t.shape) for t in got] == [(2, 32, 9, 12), (2, 64, 5, 6)] and all(torch.equal(a, b) for a, b in zip(got, stages))
    twin = copy.deepcopy(net)
    twin.use_fused = False
    for a, b in zip(got, twin(x)):
        assert (a.float() - b.float()).abs().max().item() <= 16 * U[dtype] * b.float().abs().max().item()


def test_equal_calls_give_equal_bits_and_a_sample_ignores_its_batch(chain):
    net, x = chain["net"], chain["x"]
    with torch.no_grad():
        a, b, one = net(x), net(x), net(x[1:].contiguous())
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and all(torch.equal(p, q) for p, q in zip(a, chain["stages"]))
    assert all(torch.equal(p[1:], q) for p, q in zip(a, one))


def test_the_eval_forward_replays_from_a_graph_to_the_eager_bits(chain, dev):
    net, x = chain["net"], chain["x"]
    static = x.clone()
    with torch.no_grad():
        eager = [t.clone() for t in net(static)]                    # the warm-up forward: the folds exist now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = net(static)
        static.copy_(_input(chain["dtype"], dev, seed=9))
        graph.replay()
        torch.cuda.synchronize()
        other = net(static)
        assert all(torch.equal(p, q) for p, q in zip(captured, other)) and not torch.equal(other[-1], eager[-1])
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(captured, eager))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_the_tuple_feeds_secondfpn(dev, dtype):
    """The camera pair of the ResNet-50 configs at a sixteenth of the widths.  16 planes in layer1: its conv1 and conv2 are off the
    kernel's multiples and run through torch inside the chain; SECONDFPN's two strided-convolution levels are not served by
    bev_conv_forward either."""
    net = _all_on(_randomise(cr.ResNet(depth=50, base_channels=16, stem_channels=64), 14).to(dev).to(dtype).eval())
    neck = _randomise(bt.SECONDFPN([64, 128, 256, 512], [32, 32, 32, 32], upsample_strides=[0.25, 0.5, 1, 2]), 15).to(dev).to(dtype).eval()
    x = _input(dtype, dev, hw=(64, 96), seed=2)
    assert net.fusable(x)
    feats = net(x)
    assert [tuple(t.shape) for t in feats] == [(2, 64, 16, 24), (2, 128, 8, 12), (2, 256, 4, 6), (2, 512, 2, 3)]
    assert bt.layer_spec(neck.deblocks[0][0], neck.deblocks[0][1]) is None and bt.layer_spec(neck.deblocks[1][0], neck.deblocks[1][1]) is None
    assert neck.fusable(feats)
    out = neck(feats)
    assert isinstance(out, list) and len(out) == 1 and tuple(out[0].shape) == (2, 128, 4, 6)
    tnet, tneck = copy.deepcopy(net), copy.deepcopy(neck)
    tnet.use_fused = tneck.use_fused = False
    want = tneck(tnet(x))[0]
    assert (out[0].float() - want.float()).abs().max().item() <= 16 * U[dtype] * want.float().abs().max().item()
