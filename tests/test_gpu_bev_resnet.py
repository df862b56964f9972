"""The BasicBlock tail (`bevamd_res_block_forward`) and `GeneralizedResNet` over it on the device, pinned to float64 on the CPU.

Every tail is compared with float64 computed from the exact 16-bit operand values and the fold's own fp32 scales and shifts:

    ref = relu(s2 * conv64(h, W2) + t2 + R)         mag = |s2| * conv64(|h|, |W2|) + |t2| + M
    identity:   R = x                               M = |x|
    downsample: R = sd * conv64(x, Wd) + td         M = |sd| * conv64(|x|, |Wd|) + |td|
    |y - ref| <= 1.01 * (u * |ref| + (K + 8) * 2^-23 * mag) + d

u = 2^-11 (fp16) or 2^-8 (bf16) is the one rounding to the storage type, K the length of the sums (9 C, plus Cx with a downsample),
2^-23 per term covers any fp32 summation order, a non-nearest rounding inside the MFMA and the two fp32 operations of the epilogue,
d = 2^-24 is fp16's subnormal step (0 for bf16).  The bar is DESIGN 3.23's, derived, not tuned.  The exact cases (small integers,
power-of-two scales, integer shifts) have no tolerance at all: they catch every lane-map, tap, transpose, stride, border and
residual-index error.

The observed errors are written to profiles/bev_resnet_observed.json.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from bevfusion_amd import _capi, bev_resnet as br, bev_trunk as bt
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
# stride 2: the map of x -> the output map
S2_MAPS = [(1, 1), (5, 9), (8, 8), (9, 9), (16, 32), (18, 34), (17, 33)]
ALL_LAYOUTS_ON = [(9, 17), (3, 5)]


def _out_map(xmap, s):
    return ((xmap[0] - 1) // s + 1, (xmap[1] - 1) // s + 1)


def _cases():
    """(mode, stride, map of x, C, Cx, layouts).  Every map in all three residual modes; all eight layout triples on the 9 x 17 and
    3 x 5 outputs, one (rotating) elsewhere; C over the three channel tiles and the five-tile width 160, Cx over {16, 48, 64}, and
    336 -> 160 on 3 x 5."""
    out = []
    for mode, s, maps in (("identity", 1, OUT_MAPS), ("down", 1, OUT_MAPS), ("down", 2, S2_MAPS)):
        full_done = set()
        for xmap in maps:
            om = _out_map(xmap, s)
            cx = 64 if mode == "identity" else 48
            if om in ALL_LAYOUTS_ON and om not in full_done:
                full_done.add(om)
                out += [(mode, s, xmap, 64, cx, lay) for lay in LAYOUTS]
            else:
                out.append((mode, s, xmap, 64, cx, LAYOUTS[len(out) % 8]))
        xm = (9, 17) if s == 1 else (17, 33)
        for c, cx in ((32, 16), (128, 64), (160, 48)):
            out.append((mode, s, xm, c, c if mode == "identity" else cx, LAYOUTS[len(out) % 8]))
        if mode == "down":
            out.append((mode, s, (3, 5) if s == 1 else (6, 9), 160, 336, LAYOUTS[len(out) % 8]))
    return out


CASES = _cases()
IDS = ["%s%d-%dx%d-%dto%d-%s-%s-%s" % (m, s, xm[0], xm[1], cx, c, l[0], l[1], l[2]) for m, s, xm, c, cx, l in CASES]


# ---- data and the float64 reference ----------------------------------------------------------------------------------------------
def _random_block(seed, mode, s, xmap, C, Cx, dtype, B=2):
    g = torch.Generator().manual_seed(seed)
    om = _out_map(xmap, s)
    h = torch.randn((B, C) + om, generator=g).to(dtype)
    x = torch.randn((B, Cx) + tuple(xmap), generator=g).to(dtype)
    w2 = (torch.randn((C, C, 3, 3), generator=g) / (9 * C) ** 0.5).to(dtype)
    wd = (torch.randn((C, Cx, 1, 1), generator=g) / Cx ** 0.5).to(dtype) if mode == "down" else None

    def affine():
        scale = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
        return scale.float(), (0.5 * torch.randn(C, generator=g)).float()
    s2, t2 = affine()
    sd, td = affine() if mode == "down" else (None, None)
    return dict(h=h, x=x, w2=w2, wd=wd, s2=s2, t2=t2, sd=sd, td=td, mode=mode, stride=s)


def _exact_block(seed, mode, s, xmap, C, Cx, dtype, B=2):
    """Integers in [-2, 2] with no symmetry in any axis (a fixed random draw), power-of-two scales (some negative), integer shifts."""
    g = torch.Generator().manual_seed(1000 + seed)
    om = _out_map(xmap, s)
    h = torch.randint(-2, 3, (B, C) + om, generator=g).to(dtype)
    x = torch.randint(-2, 3, (B, Cx) + tuple(xmap), generator=g).to(dtype)
    w2 = torch.randint(-2, 3, (C, C, 3, 3), generator=g).to(dtype)
    wd = torch.randint(-2, 3, (C, Cx, 1, 1), generator=g).to(dtype) if mode == "down" else None
    s2 = torch.tensor([2.0 ** ((c % 4) - 2) * (-1.0 if c % 5 == 3 else 1.0) for c in range(C)])
    t2 = torch.tensor([float((c * 7) % 9 - 3) for c in range(C)])
    sd = torch.tensor([2.0 ** (((c + 1) % 3) - 1) * (-1.0 if c % 7 == 2 else 1.0) for c in range(C)]) if mode == "down" else None
    td = torch.tensor([float((c * 5) % 7 - 2) for c in range(C)]) if mode == "down" else None
    return dict(h=h, x=x, w2=w2, wd=wd, s2=s2, t2=t2, sd=sd, td=td, mode=mode, stride=s)


def _ref64(blk):
    """-> (ref, mag, v, r) in float64 from the exact operand values; v: the conv2 + bn2 term, r: the residual term."""
    d = lambda t: t.detach().cpu().double()      # noqa: E731
    c = lambda t: d(t).view(1, -1, 1, 1)         # noqa: E731
    h, x = d(blk["h"]), d(blk["x"])
    v = c(blk["s2"]) * F.conv2d(h, d(blk["w2"]), padding=1) + c(blk["t2"])
    mag = c(blk["s2"]).abs() * F.conv2d(h.abs(), d(blk["w2"]).abs(), padding=1) + c(blk["t2"]).abs()
    if blk["mode"] == "identity":
        r, m = x, x.abs()
    else:
        r = c(blk["sd"]) * F.conv2d(x, d(blk["wd"]), stride=blk["stride"]) + c(blk["td"])
        m = c(blk["sd"]).abs() * F.conv2d(x.abs(), d(blk["wd"]).abs(), stride=blk["stride"]) + c(blk["td"]).abs()
    return torch.relu(v + r), mag + m, v, r


def _bar(ref, mag, K, dtype):
    return 1.01 * (U[dtype] * ref.abs() + (K + 8) * 2.0 ** -23 * mag) + D[dtype]


def _sum_length(blk):
    C, Cx = blk["w2"].shape[0], blk["x"].shape[1]
    return 9 * C + (Cx if blk["mode"] == "down" else 0)


def _make_fold(blk, dev):
    C, Cx = blk["w2"].shape[0], blk["x"].shape[1]
    down = blk["mode"] == "down"
    on = lambda t: t.to(dev) if t is not None else None      # noqa: E731
    return br.FoldedResBlock(bt.bev_pack_weight(blk["w2"]).to(dev), on(blk["s2"]), on(blk["t2"]),
                             bt.bev_pack_weight(blk["wd"]).to(dev) if down else None, on(blk["sd"]), on(blk["td"]), C, Cx,
                             "downsample" if down else "identity", blk["stride"])


def _to_layout(t, layout, dev):
    t = t.to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t.contiguous()


def check_inputs_are_telling(blk, ref, v, r):
    """A condition on the DATA (checked on the CPU, before anything runs on the device): the ReLU cuts, the shifts matter, and in
    the identity cases a dropped residual changes the sign under the ReLU at one output in ten at least."""
    frac = (ref > 0).double().mean().item()
    assert 0.25 <= frac <= 0.75, frac
    assert (blk["t2"] > 0).double().mean().item() >= 0.25
    if blk["mode"] == "down":
        assert (blk["td"] > 0).double().mean().item() >= 0.25
    else:
        flips = (((v < 0) & (v + r > 0)) | ((v + r < 0) & (v > 0))).double().mean().item()
        assert flips >= 0.10, flips


def _run(blk, lay, dev):
    y = br.res_block_forward(_to_layout(blk["h"], lay[0], dev), _to_layout(blk["x"], lay[1], dev), _make_fold(blk, dev), out_layout=lay[2])
    assert y is not None and y.dtype == blk["h"].dtype and tuple(y.shape) == tuple(blk["h"].shape)
    assert y.is_contiguous() if lay[2] == "nchw" else y.is_contiguous(memory_format=torch.channels_last)
    return y


# ---- the layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tail_against_float64(dev, case, dtype):
    mode, s, xmap, C, Cx, lay = case
    blk = _random_block(CASES.index(case), mode, s, xmap, C, Cx, dtype)
    ref, mag, v, r = _ref64(blk)
    check_inputs_are_telling(blk, ref, v, r)
    y = _run(blk, lay, dev)
    err, bar = (y.cpu().double() - ref).abs(), _bar(ref, mag, _sum_length(blk), dtype)
    worst = (err / bar).max().item()
    print(f"{IDS[CASES.index(case)]} {dtype}: worst error / bar = {worst:.3f}")
    record_parity(f"res_block/{mode}{s}/{dtype}", worst, 1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tail_is_exact_on_integers(dev, case, dtype):
    mode, s, xmap, C, Cx, lay = case
    blk = _exact_block(CASES.index(case), mode, s, xmap, C, Cx, dtype)
    ref, _, v, r = _ref64(blk)
    assert 0.25 <= (ref > 0).double().mean().item() <= 0.75
    assert ref.abs().max().item() < 2.0 ** 15          # inside the finite range of fp16; fp32 holds every partial sum exactly
    y = _run(blk, lay, dev)
    want = ref.to(dtype)          # the sums are quarter-integers below 2^22: fp32 holds them exactly, so one rounding of the same real number
    got = y.cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), (got.double() - ref).abs().max().item()


def test_the_functional_returns_none_where_the_entry_point_refuses_the_sizes(dev):
    """Code 4 (48 channels, and 24 channels of x) comes back as None, with no launch; a fold that does not fit the tensors raises."""
    for C, Cx, mode in ((48, 48, "identity"), (64, 24, "down")):
        blk = _random_block(3, mode, 1, (5, 7), C, Cx, torch.float16)
        assert br.res_block_forward(blk["h"].to(dev), blk["x"].to(dev), _make_fold(blk, dev)) is None
        assert "not supported" in _capi.last_error()
    blk = _random_block(3, "identity", 1, (5, 7), 64, 64, torch.float16)
    with pytest.raises(RuntimeError, match="do not fit the fold"):
        br.res_block_forward(blk["h"].to(dev), blk["x"][:, :32].to(dev), _make_fold(blk, dev))
    with pytest.raises(RuntimeError, match="one dtype"):
        br.res_block_forward(blk["h"].to(dev), blk["x"].to(dev).bfloat16(), _make_fold(blk, dev))


def _raw_call(h, h_nhwc, x, x_nhwc, fold, out, out_nhwc, shape, xshape):
    B, C, OH, OW = shape
    down = fold.residual == "downsample"
    with torch.cuda.device(h.device):
        return _capi.load().bevamd_res_block_forward(
            _capi.ptr(h), h_nhwc, _capi.ptr(x), x_nhwc, xshape[1], xshape[2], xshape[3], 0 if h.dtype == torch.float16 else 1, B, C, OH,
            OW, int(down), fold.stride, _capi.ptr(fold.packed2), fold.packed2.numel(), _capi.ptr(fold.scale2), _capi.ptr(fold.shift2),
            _capi.ptr(fold.packed_d) if down else None, fold.packed_d.numel() if down else 0, _capi.ptr(fold.scale_d) if down else None,
            _capi.ptr(fold.shift_d) if down else None, _capi.ptr(out), out_nhwc, out.numel(), _capi.stream_ptr(h.device))


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("mode, s, xmap, lay", [("identity", 1, (3, 5), ("nhwc", "nchw", "nhwc")), ("identity", 1, (17, 33), ("nchw", "nhwc", "nchw")),
                                                ("down", 1, (3, 5), ("nchw", "nhwc", "nchw")), ("down", 1, (17, 33), ("nhwc", "nchw", "nhwc")),
                                                ("down", 2, (5, 9), ("nhwc", "nhwc", "nchw")), ("down", 2, (33, 65), ("nchw", "nchw", "nhwc"))])
def test_guarded_buffers_of_exact_size(dev, mode, s, xmap, lay, fill):
    """h, x, both weights, the scales, the shifts and dst carved from one arena filled with a dirty byte (0xFF: NaN halves), each of
    its exact size: no guard byte changes, the inputs are unchanged, every output element is written, and the result bit-equals
    an unguarded call's."""
    dtype = torch.float16
    blk = _random_block(31, mode, s, xmap, 64, 64 if mode == "identity" else 48, dtype)
    fold = _make_fold(blk, dev)
    plain = _run(blk, lay, dev)
    arena = Arena(dev, fill, capacity=16 << 20)

    def carve(t, layout, name):     # the kernel's own element order, exactly its bytes
        return arena.put(t.to(dev).permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else t.to(dev).contiguous(), name)
    gh, gx = carve(blk["h"], lay[0], "h"), carve(blk["x"], lay[1], "x")
    gfold = copy.copy(fold)
    gfold.packed2, gfold.scale2, gfold.shift2 = arena.put(fold.packed2, "packed2"), arena.put(fold.scale2, "scale2"), arena.put(fold.shift2, "shift2")
    if mode == "down":
        gfold.packed_d, gfold.scale_d, gfold.shift_d = arena.put(fold.packed_d, "packed_d"), arena.put(fold.scale_d, "scale_d"), arena.put(fold.shift_d, "shift_d")
    B, C, OH, OW = plain.shape
    out = arena.out((B, OH, OW, C) if lay[2] == "nhwc" else (B, C, OH, OW), dtype, "out")
    before = [t.clone() for t in (gh, gx, gfold.packed2, gfold.scale2, gfold.shift2)]
    rc = _raw_call(gh, int(lay[0] == "nhwc"), gx, int(lay[1] == "nhwc"), gfold, out, int(lay[2] == "nhwc"), (B, C, OH, OW), tuple(blk["x"].shape))
    assert rc == 0, _capi.last_error()
    arena.check()
    assert all(torch.equal(a, b) for a, b in zip(before, (gh, gx, gfold.packed2, gfold.scale2, gfold.shift2)))
    if mode == "down":
        assert torch.equal(gfold.packed_d, fold.packed_d) and torch.equal(gfold.scale_d, fold.scale_d) and torch.equal(gfold.shift_d, fold.shift_d)
    logical = out.permute(0, 3, 1, 2) if lay[2] == "nhwc" else out
    assert torch.equal(logical.contiguous().view(torch.int16), plain.contiguous().view(torch.int16))
    assert not torch.isnan(out).any()


# ---- the module ------------------------------------------------------------------------------------------------------------------
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


def _net(dtype, dev, in_channels=32, blocks=((2, 32, 2), (1, 64, 1)), seed=1):
    net = _randomise(br.GeneralizedResNet(in_channels, [list(b) for b in blocks]), seed).to(dev).to(dtype).eval()
    net.use_fused = True
    net.fused_stride2 = True                                   # every half through a kernel, whatever the measured defaults are
    net.fused_tails = ("identity", "down1", "down2")
    return net


def _input(dtype, dev, B=2, c=32, hw=(12, 12), seed=5):
    return torch.randn((B, c) + hw, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def _conv_ref64(x, conv, fold):
    d = lambda t: t.detach().cpu().double()      # noqa: E731
    s, t = d(fold.scale).view(1, -1, 1, 1), d(fold.shift).view(1, -1, 1, 1)
    acc = F.conv2d(d(x), d(conv.weight), stride=conv.stride, padding=1)
    mag = F.conv2d(d(x).abs(), d(conv.weight).abs(), stride=conv.stride, padding=1)
    return torch.relu(s * acc + t), s.abs() * mag + t.abs()


def _functional_block(blk, x, dtype, nodes=None):
    """One block through the two functionals, each node checked against float64 of that node's OWN input."""
    f1 = bt.fold_bev_layer(blk.conv1, blk.bn1)
    h = bt.bev_conv_forward([x], f1, out_layout="nhwc")
    assert h is not None
    ref, mag = _conv_ref64(x, blk.conv1, f1)
    w1 = ((h.cpu().double() - ref).abs() / _bar(ref, mag, 9 * blk.conv1.in_channels, dtype)).max().item()
    fold = br.fold_res_block(blk)
    y = br.res_block_forward(h, x, fold, out_layout="nhwc")
    assert y is not None
    down = blk.downsample is not None
    data = dict(h=h, x=x, w2=blk.conv2.weight, wd=blk.downsample[0].weight if down else None, s2=fold.scale2, t2=fold.shift2,
                sd=fold.scale_d, td=fold.shift_d, mode="down" if down else "identity", stride=fold.stride)
    ref, mag, _, _ = _ref64(data)
    w2 = ((y.cpu().double() - ref).abs() / _bar(ref, mag, _sum_length(data), dtype)).max().item()
    if nodes is not None:
        nodes += [w1, w2]
    return y


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "bf16"])
def chain(request, dev):
    """GeneralizedResNet(32, [[2, 32, 2], [1, 64, 1]]) on 12 x 12, B = 2 (a stride-2 downsample, an identity and a stride-1
    downsample block), driven block by block through the functionals; computed once and shared."""
    dtype = request.param
    net = _net(dtype, dev)
    x = _input(dtype, dev)
    nodes, stages = [], []
    y = x
    for stage in net:
        for blk in stage:
            y = _functional_block(blk, y, dtype, nodes)
        stages.append(y)
    return dict(dtype=dtype, net=net, x=x, stages=stages, nodes=nodes)


def test_every_node_of_the_chain_against_float64(chain):
    assert len(chain["nodes"]) == 6
    print("worst error / bar per node:", ["%.3f" % v for v in chain["nodes"]])
    for i, v in enumerate(chain["nodes"]):
        record_parity(f"bev_resnet/node{i}/{chain['dtype']}", v, 1.0)
    assert max(chain["nodes"]) <= 1.0, chain["nodes"]


@torch.no_grad()
def test_module_forward_bit_equals_the_functional_chain(chain):
    net, x, dtype = chain["net"], chain["x"], chain["dtype"]
    assert net.fusable(x)
    outs = net(x)
    assert isinstance(outs, list) and [tuple(t.shape) for t in outs] == [(2, 32, 6, 6), (2, 64, 6, 6)]
    assert all(t.dtype == dtype and t.is_contiguous(memory_format=torch.channels_last) for t in outs)
    assert all(torch.equal(a, b) for a, b in zip(outs, chain["stages"]))
    # an input with channels-last strides gives the same bits as the contiguous one
    assert all(torch.equal(a, b) for a, b in zip(net(x.contiguous(memory_format=torch.channels_last)), outs))


def _observed(update):
    path = os.path.join(ROOT, "profiles", "bev_resnet_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(update)
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass      # a read-only checkout: the figures are printed


def test_end_to_end_error_is_within_twice_the_torch_layers_own(chain, dev):
    """Both paths against the float64 chain of the same 16-bit parameters; errors normalised by the output's largest magnitude.  The
    fused path rounds once per half block where torch rounds after every convolution, BatchNorm and add."""
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
    record_parity(f"bev_resnet/end_to_end/{dtype}", e_fused, 2 * e_torch)
    _observed({str(dtype): dict(fused=e_fused, torch_layers=e_torch, ratio=e_fused / e_torch, bar_ratio=2.0,
                                nodes_worst_error_over_bar=chain["nodes"])})
    assert e_fused <= 2 * e_torch, (e_fused, e_torch)


def _spread_bar(y, dtype):
    """Two runs of the SAME torch layers may pick another algorithm, i.e. another summation order: a few roundings of the storage
    type at the output's scale per layer."""
    return 8 * U[dtype] * y.abs().max().item()


@pytest.mark.parametrize("how", ["train", "fp32", "requires_grad", "use_fused_false", "c48"])
def test_dispatch_takes_the_torch_layers(dev, how):
    dtype = torch.float32 if how == "fp32" else torch.float16
    net = _net(dtype, dev, blocks=((1, 48, 1),) if how == "c48" else ((2, 32, 2), (1, 64, 1)), seed=4)
    x = _input(dtype, dev, hw=(9, 9), seed=1)
    net.use_fused = how != "use_fused_false"
    twin = copy.deepcopy(net)
    twin.use_fused = False
    if how == "train":
        net.train()
        twin.train()
    if how == "requires_grad":
        x.requires_grad_(True)
    with torch.enable_grad() if how in ("train", "requires_grad") else torch.no_grad():
        assert not net.fusable(x)
        got, want = net(x), twin(x)
    for a, b in zip(got, want):
        assert (a.detach().float() - b.detach().float()).abs().max().item() <= _spread_bar(b.detach().float(), torch.float16)
    if how == "requires_grad":
        got[-1].float().sum().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all()
    if how == "train":
        assert int(net[0][0].bn1.num_batches_tracked) == 1
    if how not in ("fp32", "c48"):     # the same module does take the kernels once the reason is gone
        net.eval()
        net.use_fused = True
        with torch.no_grad():
            assert net.fusable(x.detach())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_a_half_the_kernels_do_not_serve_runs_through_torch_inside_the_fused_chain(dev, dtype):
    """A 48-wide first stage (neither half served) in front of a served 48 -> 64 stage; then the class switches: conv1 at stride 2
    and the tails sent to torch one at a time.  The served halves bit-equal the functionals on the same input; the whole agrees with
    the torch layers within a few roundings of the storage type per layer."""
    net = _net(dtype, dev, blocks=((1, 48, 1), (1, 64, 1)), seed=11)
    x = _input(dtype, dev, hw=(9, 7), seed=3)
    assert bt.layer_spec(net[0][0].conv1, net[0][0].bn1) is None and br.res_block_spec(net[0][0]) is None and net.fusable(x)
    got = net(x)
    twin = copy.deepcopy(net)
    twin.use_fused = False
    want = twin(x)
    assert (got[0].float() - want[0].float()).abs().max().item() <= _spread_bar(want[0].float(), dtype)
    assert torch.equal(got[1], _functional_block(net[1][0], bt._as_source(got[0]), dtype))
    assert (got[1].float() - want[1].float()).abs().max().item() <= 16 * U[dtype] * want[1].float().abs().max().item()

    net = _net(dtype, dev, seed=12)
    x = _input(dtype, dev, seed=4)
    full = net(x)
    want = copy.deepcopy(net)
    want.use_fused = False
    want = want(x)
    for switch in (dict(fused_stride2=False), dict(fused_tails=("identity",)), dict(fused_tails=("down1", "down2")), dict(fused_tails=())):
        part = copy.deepcopy(net)
        for k, v in switch.items():
            setattr(part, k, v)
        assert part.fusable(x)
        outs = part(x)
        for a, b, c in zip(outs, full, want):
            assert tuple(a.shape) == tuple(b.shape) and a.dtype == dtype
            top = c.float().abs().max().item()
            assert (a.float() - b.float()).abs().max().item() <= 16 * U[dtype] * top
            assert (a.float() - c.float()).abs().max().item() <= 16 * U[dtype] * top
    part = copy.deepcopy(net)
    part.fused_stride2, part.fused_tails = False, ()
    part[0][1].conv1 = torch.nn.Conv2d(32, 32, 3, padding=1, bias=True).to(dev).to(dtype)      # no half left for a kernel ...
    part[1][0].conv1 = torch.nn.Conv2d(32, 64, 3, padding=1, bias=True).to(dev).to(dtype)
    assert not part.fusable(x)


def test_equal_calls_give_equal_bits_and_a_sample_ignores_its_batch(chain):
    net, x = chain["net"], chain["x"]
    with torch.no_grad():
        a, b, one = net(x), net(x), net(x[:1].contiguous())
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and all(torch.equal(p, q) for p, q in zip(a, chain["stages"]))
    assert all(torch.equal(p[:1], q) for p, q in zip(a, one))


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
def test_the_real_widths_336_to_160_at_stride_2(dev, dtype):
    stage = _randomise(br.make_res_layer(br.BasicBlock, 336, 160, 1, stride=2), 21).to(dev).to(dtype).eval()
    x = _input(dtype, dev, B=1, c=336, hw=(16, 16), seed=6)
    nodes = []
    y = _functional_block(stage[0], x, dtype, nodes)
    assert tuple(y.shape) == (1, 160, 8, 8) and torch.isfinite(y).all()
    print("worst error / bar:", nodes)
    assert max(nodes) <= 1.0, nodes
