"""The camera necks' fused layer (`bevamd_neck_conv_forward`) and the modules over it on the device, pinned to float64 on the CPU.

Every layer is compared with float64 computed from the exact 16-bit operand values and the fold's own fp32 scale and shift.  The
operand of a resampled source is the host mirror's (tests/cam_neck_reference.py: the kernel's fp32 arithmetic, one numpy operation
per rounding, rounded once to the storage type), which the kernel has to reproduce bit for bit, so the resampling adds NOTHING to
the bar of tests/test_gpu_bev_trunk.py:

    ref = [relu](s * conv64(x, w) + t)          mag = |s| * conv64(|x|, |w|) + |t|
    |y - ref| <= 1.01 * (u * |ref| + (K + 8) * 2^-23 * mag) + d

u = 2^-11 (fp16) or 2^-8 (bf16), K = Cin * kernel^2, d = 2^-24 (fp16's subnormal step; 0 for bf16).  The exact cases (sources 16 *
{-2 .. 2}, integer weights, power-of-two scales, integer shifts, on the map pairs whose resampling is exact: tests/test_cam_neck.py
shows that on the CPU) have no tolerance at all.

The observed end-to-end errors are written to profiles/cam_neck_observed.json.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from bevfusion_amd import bev_trunk as bt, cam_neck as cnk
from cam_neck_reference import ref64
from conftest import record_parity
from guarded import Arena
from test_cam_neck import EXACT_PAIRS, PAIRS, randomise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
D = {torch.float16: 2.0 ** -24, torch.bfloat16: 0.0}
DTYPES = [torch.float16, torch.bfloat16]
LAYOUTS2 = [("nchw", "nchw"), ("nchw", "nhwc"), ("nhwc", "nchw"), ("nhwc", "nhwc")]


def _pid(pair):
    return "%dx%d-%dx%d" % (pair[0] + pair[1])


def _cases(pairs):
    """(tag, [(channels, resampled)], Cout, kernel, pair, source layouts, dst layout, relu)."""
    out = []
    for pair in pairs:
        for order in ("dr", "rd"):                                   # direct + resampled, and the LSSFPN order
            chans = [(16, False), (32, True)] if order == "dr" else [(32, True), (16, False)]
            for sl in LAYOUTS2:
                for dl in ("nhwc", "nchw"):
                    out.append((f"k1-{order}", chans, 64, 1, pair, sl, dl, True))
        out.append(("k3-r", [(32, True)], 32, 3, pair, ("nchw",), "nhwc", True))
        out.append(("k3-r", [(32, True)], 32, 3, pair, ("nhwc",), "nchw", True))
    return out


def _wide():
    pair = ((2, 3), (3, 5))
    out = []
    for c in ([(192, False), (256, True)], [(384, False), (768, True)]):
        out.append(("k1-wide", c, 256, 1, pair, ("nchw", "nhwc"), "nhwc", True))
        out.append(("k1-wide", c, 256, 1, pair, ("nchw", "nchw"), "nchw", True))
    out.append(("k1-norelu", [(16, False), (32, True)], 64, 1, ((3, 5), (5, 9)), ("nchw", "nhwc"), "nhwc", False))
    out.append(("k3-norelu", [(32, True)], 32, 3, ((2, 3), (5, 9)), ("nhwc",), "nchw", False))
    return out


def _cid(case):
    tag, chans, cout, kernel, pair, sl, dl, relu = case
    return "%s-%s-%s-%d-%s-%s" % (tag, _pid(pair), "+".join(str(c) for c, _ in chans), cout, "+".join(sl), dl)


CASES = _cases(PAIRS) + _wide()
EXACT = _cases(EXACT_PAIRS)


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _shapes(chans, pair, B):
    return [(B, c) + tuple(pair[0] if rs else pair[1]) for c, rs in chans]


def _random_layer(seed, chans, cout, kernel, pair, dtype, B=2):
    """As `_random_layer` of tests/test_gpu_bev_trunk.py: unit-variance sources, weights of variance 1 / K, scales of either sign."""
    g = torch.Generator().manual_seed(seed)
    cin = sum(c for c, _ in chans)
    K = cin * kernel * kernel
    srcs = [torch.randn(s, generator=g).to(dtype) for s in _shapes(chans, pair, B)]
    w = (torch.randn((cout, cin, kernel, kernel), generator=g) / K ** 0.5).to(dtype)
    scale = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)
    shift = 0.5 * torch.randn(cout, generator=g)
    return srcs, w, scale.float(), shift.float()


def _exact_layer(seed, chans, cout, kernel, pair, dtype, B=2):
    """Sources 16 * {-2 .. 2} and weights {-2 .. 2} with no symmetry in any axis, power-of-two scales, integer shifts."""
    g = torch.Generator().manual_seed(1000 + seed)
    cin = sum(c for c, _ in chans)
    srcs = [(16 * torch.randint(-2, 3, s, generator=g)).to(dtype) for s in _shapes(chans, pair, B)]
    w = torch.randint(-2, 3, (cout, cin, kernel, kernel), generator=g).to(dtype)
    scale = torch.tensor([2.0 ** ((c % 4) - 2) for c in range(cout)]) * torch.tensor([-1.0 if c % 5 == 3 else 1.0 for c in range(cout)])
    shift = torch.tensor([float((c * 7) % 9 - 3) for c in range(cout)])
    return srcs, w, scale.float(), shift.float()


def _bar(ref, mag, K, dtype):
    return 1.01 * (U[dtype] * ref.abs() + (K + 8) * 2.0 ** -23 * mag) + D[dtype]


def _make_fold(w, scale, shift, kernel, dev):
    return bt.FoldedBevLayer(bt.bev_pack_weight(w, "conv").to(dev), scale.to(dev), shift.to(dev), w.shape[1], w.shape[0], kernel, 1, "conv")


def _to_layout(t, layout, dev):
    t = t.to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t.contiguous()


def _check_inputs_are_telling(ref, shift):
    frac = (ref > 0).double().mean().item()
    assert 0.25 <= frac <= 0.75, frac
    assert (shift > 0).double().mean().item() >= 0.25


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- the layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_layer_against_float64(dev, case, dtype):
    tag, chans, cout, kernel, pair, sl, dl, relu = case
    srcs, w, scale, shift = _random_layer(CASES.index(case), chans, cout, kernel, pair, dtype)
    ref, mag = ref64(srcs, w, scale, shift, kernel, relu, pair[1])
    _check_inputs_are_telling(ref, shift)
    y = cnk.cam_neck_conv_forward([_to_layout(s, l, dev) for s, l in zip(srcs, sl)], _make_fold(w, scale, shift, kernel, dev),
                                  out_size=pair[1], relu=relu, out_layout=dl)
    assert y is not None and tuple(y.shape) == tuple(ref.shape) and y.dtype == dtype
    assert y.is_contiguous() if dl == "nchw" else y.is_contiguous(memory_format=torch.channels_last)
    K = sum(c for c, _ in chans) * kernel * kernel
    err, bar = (y.cpu().double() - ref).abs(), _bar(ref, mag, K, dtype)
    worst = (err / bar).max().item()
    print(f"{_cid(case)} {dtype}: worst error / bar = {worst:.3f}")
    record_parity(f"cam_neck_conv/{tag}/{dtype}", worst, 1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", EXACT, ids=[_cid(c) for c in EXACT])
def test_layer_is_exact_on_integers(dev, case, dtype):
    tag, chans, cout, kernel, pair, sl, dl, relu = case
    srcs, w, scale, shift = _exact_layer(EXACT.index(case), chans, cout, kernel, pair, dtype)
    ref, _ = ref64(srcs, w, scale, shift, kernel, relu, pair[1])
    _check_inputs_are_telling(ref, shift)
    y = cnk.cam_neck_conv_forward([_to_layout(s, l, dev) for s, l in zip(srcs, sl)], _make_fold(w, scale, shift, kernel, dev),
                                  out_size=pair[1], relu=relu, out_layout=dl)
    assert y is not None
    want = ref.to(dtype)          # every fp32 value on the way is exact, so one rounding of the same real number
    assert _same_bits(y.cpu(), want), (y.cpu().double() - ref).abs().max().item()


def test_out_size_defaults_to_the_map_of_the_first_source(dev):
    chans, pair = [(16, False), (32, True)], ((3, 5), (5, 9))
    srcs, w, scale, shift = _random_layer(3, chans, 64, 1, pair, torch.float16)
    fold = _make_fold(w, scale, shift, 1, dev)
    xs = [s.to(dev) for s in srcs]
    assert torch.equal(cnk.cam_neck_conv_forward(xs, fold), cnk.cam_neck_conv_forward(xs, fold, out_size=(5, 9)))
    assert tuple(cnk.cam_neck_conv_forward(xs[::-1], _make_fold(torch.cat([w[:, 16:], w[:, :16]], 1), scale, shift, 1, dev)).shape[2:]) == (3, 5)
    with pytest.raises(RuntimeError, match="channels"):
        cnk.cam_neck_conv_forward(xs[:1], fold)
    assert cnk.cam_neck_conv_forward([torch.zeros(2, 24, 3, 5, dtype=torch.float16, device=dev), xs[1][:, :24]],
                                     bt.FoldedBevLayer(fold.packed, fold.scale, fold.shift, 48, 64, 1, 1, "conv")) is None      # code 4


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_windowed_destination_is_written_exactly(dev, layout, dtype):
    """Two layers write the windows [0, 64) and [64, 128) of one NaN-filled [2, 128, 5, 9] buffer."""
    pair = ((3, 5), (5, 9))
    a = _random_layer(7, [(16, False), (32, True)], 64, 1, pair, dtype)
    b = _random_layer(8, [(32, True)], 64, 3, pair, dtype)
    fa, fb = _make_fold(a[1], a[2], a[3], 1, dev), _make_fold(b[1], b[2], b[3], 3, dev)
    xa, xb = [s.to(dev) for s in a[0]], [s.to(dev) for s in b[0]]
    buf = torch.full((2, 128, 5, 9), float("nan"), dtype=dtype, device=dev)
    if layout == "nhwc":
        buf = buf.contiguous(memory_format=torch.channels_last)
    alone_a = cnk.cam_neck_conv_forward(xa, fa, out_size=pair[1], out_layout=layout)
    alone_b = cnk.cam_neck_conv_forward(xb, fb, out_size=pair[1], out_layout=layout)
    assert cnk.cam_neck_conv_forward(xa, fa, out_size=pair[1], out=buf, out_channel_offset=0) is buf
    assert torch.isnan(buf[:, 64:]).all() and torch.equal(buf[:, :64], alone_a)
    assert cnk.cam_neck_conv_forward(xb, fb, out_size=pair[1], out=buf, out_channel_offset=64) is buf
    assert torch.equal(buf[:, :64], alone_a) and torch.equal(buf[:, 64:], alone_b) and not torch.isnan(buf).any()
    ref, mag = ref64(b[0], b[1], b[2], b[3], 3, True, pair[1])
    assert ((buf[:, 64:].cpu().double() - ref).abs() <= _bar(ref, mag, 288, dtype)).all()


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("chans, kernel, pair, sl, dl", [
    ([(16, False), (32, True)], 1, ((3, 5), (5, 9)), ("nchw", "nhwc"), "nhwc"),
    ([(32, True), (16, False)], 1, ((9, 17), (17, 33)), ("nchw", "nchw"), "nchw"),
    ([(32, True), (16, False)], 1, ((1, 1), (3, 5)), ("nhwc", "nhwc"), "nchw"),
    ([(16, False), (32, True)], 1, ((9, 17), (4, 7)), ("nhwc", "nchw"), "nhwc"),
    ([(32, True)], 3, ((8, 16), (9, 17)), ("nhwc",), "nchw"),
    ([(32, True)], 3, ((2, 3), (1, 7)), ("nchw",), "nhwc"),
])
def test_guarded_buffers_of_exact_size(dev, chans, kernel, pair, sl, dl, fill):
    """Sources, weights, scale, shift and the output carved from one arena filled with a dirty byte (0xFF: NaN halves): no guard
    byte changes, the inputs are unchanged, every output element is written, and the result bit-equals an unguarded call's."""
    dtype = torch.float16
    srcs, w, scale, shift = _random_layer(21, chans, 64, kernel, pair, dtype)
    fold = _make_fold(w, scale, shift, kernel, dev)
    plain_srcs = [_to_layout(s, l, dev) for s, l in zip(srcs, sl)]
    plain = cnk.cam_neck_conv_forward(plain_srcs, fold, out_size=pair[1], out_layout=dl)
    arena = Arena(dev, fill, capacity=16 << 20)

    def carve(t, lay, name):     # the same bytes and the same strides inside the arena
        flat = arena.put(t.permute(0, 2, 3, 1).contiguous() if lay == "nhwc" else t.contiguous(), name)
        return flat.permute(0, 3, 1, 2) if lay == "nhwc" else flat
    gs = [carve(s, l, f"src{i}") for i, (s, l) in enumerate(zip(plain_srcs, sl))]
    gfold = copy.copy(fold)
    gfold.packed, gfold.scale, gfold.shift = arena.put(fold.packed, "packed"), arena.put(fold.scale, "scale"), arena.put(fold.shift, "shift")
    B, C, OH, OW = plain.shape
    out = arena.out((B, OH, OW, C), dtype, "out").permute(0, 3, 1, 2) if dl == "nhwc" else arena.out((B, C, OH, OW), dtype, "out")
    res = cnk.cam_neck_conv_forward(gs, gfold, out_size=pair[1], out=out)
    assert res is out
    arena.check()
    assert all(torch.equal(a, b) for a, b in zip(gs, plain_srcs)) and torch.equal(gfold.packed, fold.packed)
    assert _same_bits(out, plain)
    assert not torch.isnan(out).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("hw", [(5, 9), (17, 33)])
def test_equal_maps_bit_equal_the_bev_trunk_layer(dev, hw, layout, dtype):
    srcs, w, scale, shift = _random_layer(31, [(16, False), (32, False)], 64, 1, (hw, hw), dtype)
    fold = _make_fold(w, scale, shift, 1, dev)
    xs = [_to_layout(s, layout, dev) for s in srcs]
    for dl in ("nhwc", "nchw"):
        assert _same_bits(cnk.cam_neck_conv_forward(xs, fold, out_layout=dl), bt.bev_conv_forward(xs, fold, out_layout=dl))
    w3 = _random_layer(32, [(32, False)], 64, 3, (hw, hw), dtype)
    f3 = _make_fold(w3[1], w3[2], w3[3], 3, dev)
    x3 = [_to_layout(w3[0][0], layout, dev)]
    assert _same_bits(cnk.cam_neck_conv_forward(x3, f3), bt.bev_conv_forward(x3, f3))


# ---- the modules -----------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "gen-small": (lambda: cnk.GeneralizedLSSFPN([32, 64, 128], 64, 3), [(32, (8, 22)), (64, (4, 11)), (128, (2, 6))]),
    "gen-flagship-widths": (lambda: cnk.GeneralizedLSSFPN([192, 384, 768], 256, 3), [(192, (4, 11)), (384, (2, 6)), (768, (1, 3))]),
    "lss": (lambda: cnk.LSSFPN([-1, 0], [64, 32], 64, scale_factor=2), [(32, (6, 10)), (64, (3, 5))]),
}


def _module(name, dtype, dev, seed=1):
    m = randomise(CONFIGS[name][0](), seed).to(dev).to(dtype).eval()
    m.use_fused = True            # every layer through the kernels, whatever the measured default is
    return m


def _inputs(name, dtype, dev, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, c) + hw, generator=g).to(dtype).to(dev) for c, hw in CONFIGS[name][1]]


def _as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


@pytest.fixture(scope="module", params=[(n, d) for n in CONFIGS for d in DTYPES], ids=lambda p: f"{p[0]}-{'f16' if p[1] is torch.float16 else 'bf16'}")
def chain(request, dev):
    """The functional chain of one module, B = 2, driven layer by layer, every node checked against float64 of that node's OWN
    input; computed once and shared."""
    name, dtype = request.param
    m = _module(name, dtype, dev)
    xs = _inputs(name, dtype, dev)
    nodes = []

    def run(conv, bn, srcs, out_size, through_trunk=False):
        fold = cnk.fold_neck_layer(conv, bn)
        if through_trunk:
            y = bt.bev_conv_forward(srcs, fold)
        else:
            y = cnk.cam_neck_conv_forward(srcs, fold, out_size=out_size)
        assert y is not None
        ref, mag = ref64(srcs, conv.weight.detach(), fold.scale, fold.shift, fold.kernel, True, out_size)
        _check_inputs_are_telling(ref, fold.shift)
        worst = ((y.cpu().double() - ref).abs() / _bar(ref, mag, fold.in_channels * fold.kernel ** 2, dtype)).max().item()
        nodes.append(worst)
        return y

    if name.startswith("gen"):
        lat = list(xs)
        for i in range(len(lat) - 2, -1, -1):
            size = tuple(lat[i].shape[2:])
            y = run(m.lateral_convs[i].conv, m.lateral_convs[i].bn, [lat[i], lat[i + 1]], size)
            lat[i] = run(m.fpn_convs[i].conv, m.fpn_convs[i].bn, [y], size, through_trunk=True)
        outs = tuple(lat[:-1])
    else:
        x1, x2 = xs[-1], xs[0]
        size = tuple(x2.shape[2:])
        y = run(m.fuse[0], m.fuse[1], [x1, x2], size)
        y = run(m.fuse[3], m.fuse[4], [y], size, through_trunk=True)
        outs = (run(m.upsample[1], m.upsample[2], [y], (2 * size[0], 2 * size[1])),)
    return dict(name=name, dtype=dtype, mod=m, xs=xs, outs=outs, nodes=nodes)


def test_every_node_of_the_chain_against_float64(chain):
    assert len(chain["nodes"]) == (3 if chain["name"] == "lss" else 4)
    print("worst error / bar per node:", ["%.3f" % v for v in chain["nodes"]])
    for i, v in enumerate(chain["nodes"]):
        record_parity(f"cam_neck/{chain['name']}/node{i}/{chain['dtype']}", v, 1.0)
    assert max(chain["nodes"]) <= 1.0, chain["nodes"]


@torch.no_grad()
def test_module_forward_bit_equals_the_functional_chain(chain):
    m, xs, dtype = chain["mod"], chain["xs"], chain["dtype"]
    assert m.fusable(xs)
    got = m(xs)
    if chain["name"] == "lss":
        assert torch.is_tensor(got) and tuple(got.shape) == (2, 64, 12, 20)
    else:
        c = m.out_channels
        assert isinstance(got, tuple) and len(got) == len(xs) - 1
        assert [tuple(t.shape) for t in got] == [(2, c) + tuple(x.shape[2:]) for x in xs[:-1]]
    got = _as_tuple(got)
    assert all(t.dtype == dtype and t.is_contiguous(memory_format=torch.channels_last) for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, chain["outs"]))
    # channels-last inputs give the same bits as contiguous NCHW ones, and the model's view of the result still works
    again = _as_tuple(m([x.contiguous(memory_format=torch.channels_last) for x in xs]))
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    assert tuple(got[0].view(1, 2, *got[0].shape[1:]).shape) == (1, 2) + tuple(got[0].shape[1:])


def test_end_to_end_error_is_within_twice_the_torch_layers_own(chain, dev):
    """Both paths against the module's float64 twin of the same 16-bit parameters; errors normalised by the output's largest
    magnitude.  The fused path rounds once per layer where torch rounds after the convolution and again after BatchNorm."""
    m, xs, dtype, name = chain["mod"], chain["xs"], chain["dtype"], chain["name"]
    twin64 = copy.deepcopy(m).cpu().double()
    twin64.use_fused = False
    torch_mod = copy.deepcopy(m)
    torch_mod.use_fused = False
    with torch.no_grad():
        ref = _as_tuple(twin64([x.cpu().double() for x in xs]))
        assert not torch_mod.fusable(xs)
        y_torch, y_fused = _as_tuple(torch_mod(xs)), _as_tuple(m(xs))
    e_fused = max((y.cpu().double() - r).abs().max().item() / r.abs().max().item() for y, r in zip(y_fused, ref))
    e_torch = max((y.cpu().double() - r).abs().max().item() / r.abs().max().item() for y, r in zip(y_torch, ref))
    print(f"{name} {dtype}: fused {e_fused:.3e}, torch layers {e_torch:.3e}, ratio {e_fused / e_torch:.3f}")
    record_parity(f"cam_neck/{name}/end_to_end/{dtype}", e_fused, 2 * e_torch)
    path = os.path.join(ROOT, "profiles", "cam_neck_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[f"{name}/{dtype}"] = dict(fused=e_fused, torch_layers=e_torch, ratio=e_fused / e_torch, bar_ratio=2.0,
                                      nodes_worst_error_over_bar=chain["nodes"])
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass      # a read-only checkout: the figures are printed above
    assert e_fused <= 2 * e_torch, (e_fused, e_torch)


def _spread_bar(y, dtype):
    """Two runs of the SAME torch layers may pick another algorithm, i.e. another summation order: a few roundings of the storage
    type at the output's scale per layer."""
    return 8 * U[dtype] * y.abs().max().item()


HOWS = ["train", "fp32", "requires_grad", "use_fused_false", "cout48"]


@pytest.mark.parametrize("kind, how", [("gen", h) for h in HOWS + ["nearest"]] + [("lss", h) for h in HOWS])      # LSSFPN has no upsample_cfg
def test_dispatch_takes_the_torch_layers(dev, kind, how):
    dtype = torch.float32 if how == "fp32" else torch.float16
    cout = 48 if how == "cout48" else 64
    if kind == "gen":
        mod = cnk.GeneralizedLSSFPN([32, 64, 128], cout, 3, upsample_cfg=dict(mode="nearest") if how == "nearest" else
                                    dict(mode="bilinear", align_corners=True))
        name = "gen-small"
    else:
        mod = cnk.LSSFPN([-1, 0], [64, 32], cout, scale_factor=2)
        name = "lss"
    mod = randomise(mod, 4).to(dev).to(dtype).eval()
    xs = _inputs(name, dtype, dev, seed=6)
    mod.use_fused = how != "use_fused_false"
    twin = copy.deepcopy(mod)
    twin.use_fused = False
    if how == "train":
        mod.train()
        twin.train()
    if how == "requires_grad":
        xs[0].requires_grad_(True)
    with torch.enable_grad() if how in ("train", "requires_grad") else torch.no_grad():
        assert not mod.fusable(xs)
        got, want = _as_tuple(mod(xs)), _as_tuple(twin(xs))
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert (a.detach().float() - b.detach().float()).abs().max().item() <= _spread_bar(b.detach().float(), torch.float16)
    if how == "requires_grad":
        got[0].float().sum().backward()
        assert xs[0].grad is not None and torch.isfinite(xs[0].grad).all()
    if how == "train":
        assert all(int(b.num_batches_tracked) == 1 for b in mod.modules() if isinstance(b, torch.nn.BatchNorm2d))
    if how not in ("fp32", "cout48"):     # the same module does take the kernels once the reason is gone
        mod.eval()
        mod.use_fused = True
        if how == "nearest":
            mod.upsample_cfg = dict(mode="bilinear", align_corners=True)
        with torch.no_grad():
            assert mod.fusable([x.detach() for x in xs])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_a_lateral_without_batchnorm_goes_through_the_kernel(dev, dtype):
    """no_norm_on_lateral=True: convolution + bias + ReLU, scale ones and shift the bias."""
    m = randomise(cnk.GeneralizedLSSFPN([32, 64], 64, 1, no_norm_on_lateral=True), 9).to(dev).to(dtype).eval()
    m.use_fused = True
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(2, 32, 5, 9, generator=g).to(dtype).to(dev), torch.randn(2, 64, 3, 5, generator=g).to(dtype).to(dev)]
    assert m.fusable(xs) and m.lateral_convs[0].conv.bias is not None and m.lateral_convs[0].norm is None
    conv = m.lateral_convs[0].conv
    fold = cnk.fold_neck_layer(conv, None)
    y = cnk.cam_neck_conv_forward(xs, fold)
    ref, mag = ref64(xs, conv.weight.detach(), fold.scale, fold.shift, 1, True, (5, 9))
    _check_inputs_are_telling(ref, fold.shift)
    worst = ((y.cpu().double() - ref).abs() / _bar(ref, mag, 96, dtype)).max().item()
    record_parity(f"cam_neck/no_norm_lateral/{dtype}", worst, 1.0)
    assert worst <= 1.0, worst
    out = m(xs)
    f = m.fpn_convs[0]
    assert len(out) == 1 and torch.equal(out[0], bt.bev_conv_forward([y], bt.fold_bev_layer(f.conv, f.bn)))


def test_equal_calls_give_equal_bits_and_a_sample_ignores_its_batch(chain):
    m, xs = chain["mod"], chain["xs"]
    with torch.no_grad():
        a, b = _as_tuple(m(xs)), _as_tuple(m(xs))
        one = _as_tuple(m([x[:1].contiguous() for x in xs]))
    assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a, b, chain["outs"]))
    assert all(torch.equal(p[:1], q) for p, q in zip(a, one))


def test_the_eval_forward_replays_from_a_graph_to_the_eager_bits(chain, dev):
    m, xs = chain["mod"], chain["xs"]
    static = [x.clone() for x in xs]
    with torch.no_grad():
        eager = [t.clone() for t in _as_tuple(m(static))]              # the warm-up forward: the folds exist now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = _as_tuple(m(static))
        for s, x in zip(static, _inputs(chain["name"], chain["dtype"], dev, seed=9)):
            s.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        other = _as_tuple(m(static))
        assert all(torch.equal(c, o) for c, o in zip(captured, other)) and not torch.equal(other[0], eager[0])
        for s, x in zip(static, xs):
            s.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(c, e) for c, e in zip(captured, eager))


def test_the_flagship_neck_runs_six_images_at_256x704(dev):
    m = randomise(cnk.GeneralizedLSSFPN([192, 384, 768], 256, 3), 2).to(dev).half().eval()
    m.use_fused = True
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn((6, c) + hw, generator=g).half().to(dev) for c, hw in [(192, (32, 88)), (384, (16, 44)), (768, (8, 22))]]
    with torch.no_grad():
        assert m.fusable(xs)
        out = m(xs)
    assert [tuple(t.shape) for t in out] == [(6, 256, 32, 88), (6, 256, 16, 44)]
    assert all(torch.isfinite(t).all() and t.is_contiguous(memory_format=torch.channels_last) for t in out)
    lss = randomise(cnk.LSSFPN([-1, 0], [640, 160], 256, scale_factor=2), 3).to(dev).half().eval()
    lss.use_fused = True
    xl = [torch.randn(1, 160, 24, 24, generator=g).half().to(dev), torch.randn(1, 640, 12, 12, generator=g).half().to(dev)]
    with torch.no_grad():
        y = lss(xl)
    assert tuple(y.shape) == (1, 256, 48, 48) and torch.isfinite(y).all()
