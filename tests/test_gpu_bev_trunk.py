"""The BEV trunk's fused layer (`bevamd_bev_conv_forward`) and the modules over it on the device, pinned to float64 on the CPU.

Every layer is compared with float64 computed from the exact 16-bit operand values and the fold's own fp32 scale and shift:

    ref = relu(s * conv64(x, w) + t)          mag = |s| * conv64(|x|, |w|) + |t|
    |y - ref| <= 1.01 * (u * |ref| + (K + 8) * 2^-23 * mag) + d

u = 2^-11 (fp16) or 2^-8 (bf16) is the one rounding to the storage type, K the length of the sum (9 Cin, or Cin for 1x1 and the
deconvolution), 2^-23 per term covers any fp32 summation order and a non-nearest rounding inside the MFMA, d = 2^-24 is fp16's
subnormal step (0 for bf16).  The bar is derived, not tuned.  The exact cases (small integers, power-of-two scale, integer shift)
have no tolerance at all: they catch every lane-map, tap, transpose and border error.

The observed end-to-end errors are written to profiles/bev_trunk_observed.json.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from bevfusion_amd import bev_trunk as bt
from conftest import record_parity
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
D = {torch.float16: 2.0 ** -24, torch.bfloat16: 0.0}
DTYPES = [torch.float16, torch.bfloat16]
MODES = {"c3s1": ("conv", 3, 1), "c3s2": ("conv", 3, 2), "c1": ("conv", 1, 1), "dc": ("deconv", 2, 2)}
MAPS = {"c3s1": [(1, 1), (1, 7), (3, 5), (8, 16), (9, 16), (8, 17), (17, 33)], "c3s2": [(8, 8), (9, 9), (17, 33)],
        "c1": [(3, 5), (9, 16), (17, 33)], "dc": [(3, 5), (9, 16), (17, 33)]}
LAYOUTS = [("nchw", "nhwc"), ("nhwc", "nhwc"), ("nchw", "nchw"), ("nhwc", "nchw")]


def _cases():
    out = []
    for tag, maps in MODES.items():
        for hw in MAPS[tag]:
            for lay in LAYOUTS:
                out.append((tag, hw, (16, 32), 64, lay))
            out.append((tag, hw, (32,), 32, LAYOUTS[0]))
        out.append((tag, (3, 5), (80, 256), 256, LAYOUTS[0]))
        out.append((tag, (3, 5), (80, 256), 256, LAYOUTS[3]))
    return out


CASES = _cases()
IDS = ["%s-%dx%d-%s-%d-%s-%s" % (t, hw[0], hw[1], "+".join(map(str, c)), co, l[0], l[1]) for t, hw, c, co, l in CASES]


# ---- data and the float64 reference ----------------------------------------------------------------------------------------------
def _weight_shape(mode, kernel, cin, cout):
    return (cin, cout, 2, 2) if mode == "deconv" else (cout, cin, kernel, kernel)


def _random_layer(seed, mode, kernel, cins, cout, hw, dtype, B=2):
    g = torch.Generator().manual_seed(seed)
    cin = sum(cins)
    K = cin * (1 if mode == "deconv" else kernel * kernel)
    srcs = [torch.randn((B, c) + tuple(hw), generator=g).to(dtype) for c in cins]
    w = (torch.randn(_weight_shape(mode, kernel, cin, cout), generator=g) / K ** 0.5).to(dtype)
    scale = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)
    shift = 0.5 * torch.randn(cout, generator=g)
    return srcs, w, scale.float(), shift.float()


def _exact_layer(seed, mode, kernel, cins, cout, hw, dtype, B=2):
    """Integers in [-2, 2] with no symmetry in any axis (a fixed random draw), power-of-two scales, integer shifts."""
    g = torch.Generator().manual_seed(1000 + seed)
    cin = sum(cins)
    srcs = [torch.randint(-2, 3, (B, c) + tuple(hw), generator=g).to(dtype) for c in cins]
    w = torch.randint(-2, 3, _weight_shape(mode, kernel, cin, cout), generator=g).to(dtype)
    scale = torch.tensor([2.0 ** ((c % 4) - 2) for c in range(cout)]) * torch.tensor([-1.0 if c % 5 == 3 else 1.0 for c in range(cout)])
    shift = torch.tensor([float((c * 7) % 9 - 3) for c in range(cout)])
    return srcs, w, scale.float(), shift.float()


def _ref64(srcs, w, scale, shift, mode, kernel, stride):
    """-> (ref, mag) in float64 from the exact operand values."""
    x = torch.cat([s.detach().cpu().double() for s in srcs], dim=1)
    w = w.detach().cpu().double()
    if mode == "deconv":
        acc, mag = F.conv_transpose2d(x, w, stride=2), F.conv_transpose2d(x.abs(), w.abs(), stride=2)
    else:
        acc = F.conv2d(x, w, stride=stride, padding=kernel // 2)
        mag = F.conv2d(x.abs(), w.abs(), stride=stride, padding=kernel // 2)
    s, t = scale.detach().cpu().double().view(1, -1, 1, 1), shift.detach().cpu().double().view(1, -1, 1, 1)
    return torch.relu(s * acc + t), s.abs() * mag + t.abs()


def _bar(ref, mag, K, dtype):
    return 1.01 * (U[dtype] * ref.abs() + (K + 8) * 2.0 ** -23 * mag) + D[dtype]


def _make_fold(w, scale, shift, mode, kernel, stride, dev):
    cin, cout = (w.shape[0], w.shape[1]) if mode == "deconv" else (w.shape[1], w.shape[0])
    return bt.FoldedBevLayer(bt.bev_pack_weight(w, mode).to(dev), scale.to(dev), shift.to(dev), cin, cout, kernel, stride, mode)


def _to_layout(t, layout, dev):
    t = t.to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t.contiguous()


def _check_inputs_are_telling(ref, shift):
    frac = (ref > 0).double().mean().item()
    assert 0.25 <= frac <= 0.75, frac
    assert (shift > 0).double().mean().item() >= 0.25


# ---- the layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layer_against_float64(dev, case, dtype):
    tag, hw, cins, cout, (sl, dl) = case
    mode, kernel, stride = MODES[tag]
    srcs, w, scale, shift = _random_layer(CASES.index(case), mode, kernel, cins, cout, hw, dtype)
    ref, mag = _ref64(srcs, w, scale, shift, mode, kernel, stride)
    _check_inputs_are_telling(ref, shift)
    y = bt.bev_conv_forward([_to_layout(s, sl, dev) for s in srcs], _make_fold(w, scale, shift, mode, kernel, stride, dev),
                            stride=stride, mode=mode, out_layout=dl)
    assert y is not None and tuple(y.shape) == tuple(ref.shape) and y.dtype == dtype
    assert y.is_contiguous() if dl == "nchw" else y.is_contiguous(memory_format=torch.channels_last)
    K = sum(cins) * (1 if mode == "deconv" else kernel * kernel)
    err, bar = (y.cpu().double() - ref).abs(), _bar(ref, mag, K, dtype)
    worst = (err / bar).max().item()
    print(f"{IDS[CASES.index(case)]} {dtype}: worst error / bar = {worst:.3f}")
    record_parity(f"bev_conv/{tag}/{dtype}", worst, 1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layer_is_exact_on_integers(dev, case, dtype):
    tag, hw, cins, cout, (sl, dl) = case
    mode, kernel, stride = MODES[tag]
    srcs, w, scale, shift = _exact_layer(CASES.index(case), mode, kernel, cins, cout, hw, dtype)
    ref, _ = _ref64(srcs, w, scale, shift, mode, kernel, stride)
    _check_inputs_are_telling(ref, shift)
    y = bt.bev_conv_forward([_to_layout(s, sl, dev) for s in srcs], _make_fold(w, scale, shift, mode, kernel, stride, dev),
                            stride=stride, mode=mode, out_layout=dl)
    assert y is not None
    want = ref.to(dtype)          # the sums are integers below 2^24: fp32 holds them exactly, so one rounding of the same real number
    got = y.cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), (got.double() - ref).abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_windowed_destination_is_written_exactly(dev, layout, dtype):
    """A 1x1 convolution and a deconvolution write the windows [0, 64) and [64, 128) of one NaN-filled [2, 128, 6, 10] buffer."""
    H, W = 3, 5
    a = _random_layer(7, "conv", 1, (32,), 64, (2 * H, 2 * W), dtype)
    b = _random_layer(8, "deconv", 2, (32,), 64, (H, W), dtype)
    fa, fb = _make_fold(a[1], a[2], a[3], "conv", 1, 1, dev), _make_fold(b[1], b[2], b[3], "deconv", 2, 2, dev)
    xa, xb = [s.to(dev) for s in a[0]], [s.to(dev) for s in b[0]]
    buf = torch.full((2, 128, 2 * H, 2 * W), float("nan"), dtype=dtype, device=dev)
    if layout == "nhwc":
        buf = buf.contiguous(memory_format=torch.channels_last)
    alone_a = bt.bev_conv_forward(xa, fa, out_layout=layout)
    alone_b = bt.bev_conv_forward(xb, fb, out_layout=layout)
    assert bt.bev_conv_forward(xa, fa, out=buf, out_channel_offset=0) is buf
    assert torch.isnan(buf[:, 64:]).all() and torch.equal(buf[:, :64], alone_a)
    assert bt.bev_conv_forward(xb, fb, out=buf, out_channel_offset=64) is buf
    assert torch.equal(buf[:, :64], alone_a) and torch.equal(buf[:, 64:], alone_b) and not torch.isnan(buf).any()
    ref, mag = _ref64(b[0], b[1], b[2], b[3], "deconv", 2, 2)
    assert ((buf[:, 64:].cpu().double() - ref).abs() <= _bar(ref, mag, 32, dtype)).all()


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
@pytest.mark.parametrize("tag, hw, lay", [("c3s1", (3, 5), ("nchw", "nhwc")), ("c3s1", (17, 33), ("nhwc", "nchw")),
                                          ("c3s2", (17, 33), ("nchw", "nchw")), ("c3s2", (3, 5), ("nhwc", "nhwc")),
                                          ("dc", (3, 5), ("nhwc", "nchw")), ("c1", (17, 33), ("nchw", "nhwc"))])
def test_guarded_buffers_of_exact_size(dev, tag, hw, lay, fill):
    """Sources, weights, scale, shift and the output carved from one arena filled with a dirty byte (0xFF: NaN halves): no guard
    byte changes, the inputs are unchanged, every output element is written, and the result bit-equals an unguarded call's."""
    mode, kernel, stride = MODES[tag]
    dtype = torch.float16
    srcs, w, scale, shift = _random_layer(21, mode, kernel, (16, 32), 64, hw, dtype)
    fold = _make_fold(w, scale, shift, mode, kernel, stride, dev)
    plain_srcs = [_to_layout(s, lay[0], dev) for s in srcs]
    plain = bt.bev_conv_forward(plain_srcs, fold, out_layout=lay[1])
    arena = Arena(dev, fill, capacity=16 << 20)

    def carve(t, name):     # the same bytes and the same strides inside the arena
        flat = arena.put(t.permute(0, 2, 3, 1).contiguous() if lay[0] == "nhwc" else t.contiguous(), name)
        return flat.permute(0, 3, 1, 2) if lay[0] == "nhwc" else flat
    gs = [carve(s, f"src{i}") for i, s in enumerate(plain_srcs)]
    gfold = copy.copy(fold)
    gfold.packed, gfold.scale, gfold.shift = arena.put(fold.packed, "packed"), arena.put(fold.scale, "scale"), arena.put(fold.shift, "shift")
    B, C, OH, OW = plain.shape
    out = arena.out((B, OH, OW, C), dtype, "out").permute(0, 3, 1, 2) if lay[1] == "nhwc" else arena.out((B, C, OH, OW), dtype, "out")
    res = bt.bev_conv_forward(gs, gfold, out=out)
    assert res is out
    arena.check()
    assert all(torch.equal(a, b) for a, b in zip(gs, plain_srcs)) and torch.equal(gfold.packed, fold.packed)
    assert torch.equal(out.contiguous().view(torch.int16), plain.contiguous().view(torch.int16))
    assert not torch.isnan(out).any()


# ---- the modules -----------------------------------------------------------------------------------------------------------------
def _randomise(module, seed):
    """Weights that keep the activations' scale through the chain (variance 2 / K), BatchNorm statistics that are not the defaults."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                K = m.in_channels * (m.kernel_size[0] * m.kernel_size[1] if isinstance(m, torch.nn.Conv2d) else 1)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / K) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.8 + 0.4 * torch.rand(n, generator=g))
                m.bias.copy_(0.3 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=g))
    return module


def _trunk(dtype, dev, fused=True):
    mods = [_randomise(bt.ConvFuser([80, 256], 256), 1), _randomise(bt.SECOND(256, [128, 256], [5, 5], [1, 2]), 2),
            _randomise(bt.SECONDFPN([128, 256], [256, 256], [1, 2], use_conv_for_no_stride=True), 3)]
    for m in mods:
        m.to(dev).to(dtype).eval()
        m.use_fused = fused
    mods[1].fused_stride2 = True      # every layer through the kernel, whatever the measured default is
    return mods


def _inputs(dtype, dev, B=2, hw=(12, 12), seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, c) + hw, generator=g).to(dtype).to(dev) for c in (80, 256)]


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "bf16"])
def chain(request, dev):
    """The functional chain at flagship widths on 12 x 12, B = 2, driven layer by layer, every node checked against float64 of that
    node's OWN input; computed once and shared."""
    dtype = request.param
    fuser, second, neck = _trunk(dtype, dev)
    xs = _inputs(dtype, dev)
    nodes = []

    def run(conv, bn, srcs, **kw):
        fold = bt.fold_bev_layer(conv, bn)
        y = bt.bev_conv_forward(srcs, fold, stride=fold.stride, mode=fold.mode, **kw)
        assert y is not None
        w = conv.weight.detach()
        if isinstance(conv, torch.nn.ConvTranspose2d) and fold.mode == "conv":
            w = w.permute(1, 0, 2, 3)
        ref, mag = _ref64(srcs, w, fold.scale, fold.shift, fold.mode, fold.kernel, fold.stride)
        _check_inputs_are_telling(ref, fold.shift)
        K = fold.in_channels * (1 if fold.mode == "deconv" else fold.kernel ** 2)
        off = kw.get("out_channel_offset", 0)
        got = y[:, off:off + fold.out_channels].cpu().double()
        worst = ((got - ref).abs() / _bar(ref, mag, K, dtype)).max().item()
        nodes.append(worst)
        return y

    x = run(fuser[0], fuser[1], xs)
    fused_out = x
    stages = []
    for blk in second.blocks:
        for j in range(0, len(blk), 3):
            x = run(blk[j], blk[j + 1], [x])
        stages.append(x)
    out = torch.empty((2, 512, 12, 12), dtype=dtype, device=dev)
    off = 0
    for t, d in zip(stages, neck.deblocks):
        run(d[0], d[1], [t], out=out, out_channel_offset=off)
        off += d[0].out_channels
    return dict(dtype=dtype, mods=(fuser, second, neck), xs=xs, fused=fused_out, stages=stages, out=out, nodes=nodes)


def test_every_node_of_the_chain_against_float64(chain):
    assert len(chain["nodes"]) == 15
    print("worst error / bar per node:", ["%.3f" % v for v in chain["nodes"]])
    for i, v in enumerate(chain["nodes"]):
        record_parity(f"bev_trunk/node{i}/{chain['dtype']}", v, 1.0)
    assert max(chain["nodes"]) <= 1.0, chain["nodes"]


@torch.no_grad()
def test_module_forward_bit_equals_the_functional_chain(chain):
    fuser, second, neck = chain["mods"]
    dtype = chain["dtype"]
    assert fuser.fusable(chain["xs"])
    f = fuser(chain["xs"])
    assert tuple(f.shape) == (2, 256, 12, 12) and f.dtype == dtype and f.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(f, chain["fused"])
    assert second.fusable(f)
    s = second(f)
    assert isinstance(s, tuple) and [tuple(t.shape) for t in s] == [(2, 128, 12, 12), (2, 256, 6, 6)]
    assert all(t.dtype == dtype and t.is_contiguous(memory_format=torch.channels_last) for t in s)
    assert all(torch.equal(a, b) for a, b in zip(s, chain["stages"]))
    assert neck.fusable(s)
    n = neck(s)
    assert isinstance(n, list) and len(n) == 1 and tuple(n[0].shape) == (2, 512, 12, 12) and n[0].dtype == dtype and n[0].is_contiguous()
    assert torch.equal(n[0], chain["out"])
    # a contiguous NCHW input of SECOND gives the same bits as the channels-last one
    assert all(torch.equal(a, b) for a, b in zip(second(f.contiguous()), s))


def _float64_chain(mods, xs):
    """The whole trunk in float64 from the 16-bit parameters, no rounding between the layers."""
    ms = [copy.deepcopy(m).cpu().double() for m in mods]
    for m in ms:
        m.use_fused = False
    with torch.no_grad():
        return ms[2](ms[1](ms[0]([x.cpu().double() for x in xs])))[0]


def test_end_to_end_error_is_within_twice_the_torch_layers_own(chain, dev):
    """Both paths against the float64 chain of the same 16-bit parameters; errors normalised by the output's largest magnitude.  The
    fused path rounds once per layer where torch rounds after the convolution and again after BatchNorm."""
    mods, xs, dtype = chain["mods"], chain["xs"], chain["dtype"]
    ref = _float64_chain(mods, xs)
    torch_mods = [copy.deepcopy(m) for m in mods]
    for m in torch_mods:
        m.use_fused = False
    with torch.no_grad():
        assert not torch_mods[0].fusable(xs)
        y_torch = torch_mods[2](torch_mods[1](torch_mods[0](xs)))[0]
        y_fused = mods[2](mods[1](mods[0](xs)))[0]
    top = ref.abs().max().item()
    e_fused = (y_fused.cpu().double() - ref).abs().max().item() / top
    e_torch = (y_torch.cpu().double() - ref).abs().max().item() / top
    print(f"{dtype}: fused {e_fused:.3e}, torch layers {e_torch:.3e}, ratio {e_fused / e_torch:.3f}")
    record_parity(f"bev_trunk/end_to_end/{dtype}", e_fused, 2 * e_torch)
    path = os.path.join(ROOT, "profiles", "bev_trunk_observed.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[str(dtype)] = dict(fused=e_fused, torch_layers=e_torch, ratio=e_fused / e_torch, bar_ratio=2.0,
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


@pytest.mark.parametrize("how", ["train", "fp32", "requires_grad", "use_fused_false", "cout48"])
def test_dispatch_takes_the_torch_layers(dev, how):
    dtype = torch.float32 if how == "fp32" else torch.float16
    if how == "cout48":
        mod = _randomise(bt.SECOND(32, [48], [1], [1]), 4).to(dev).to(dtype).eval()
        x = torch.randn(2, 32, 9, 9, generator=torch.Generator().manual_seed(1)).to(dtype).to(dev)
    else:
        mod = _randomise(bt.SECOND(32, [32, 64], [1, 1], [1, 2]), 4).to(dev).to(dtype).eval()
        x = torch.randn(2, 32, 9, 9, generator=torch.Generator().manual_seed(1)).to(dtype).to(dev)
    mod.use_fused = how != "use_fused_false"
    mod.fused_stride2 = True
    twin = copy.deepcopy(mod)
    twin.use_fused = False
    if how == "train":
        mod.train()
        twin.train()
    if how == "requires_grad":
        x.requires_grad_(True)
    with torch.enable_grad() if how in ("train", "requires_grad") else torch.no_grad():
        assert not mod.fusable(x)
        got, want = mod(x), twin(x)
    for a, b in zip(got, want):
        assert (a.detach().float() - b.detach().float()).abs().max().item() <= _spread_bar(b.detach().float(), torch.float16)
    if how == "requires_grad":
        got[-1].float().sum().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all()
    if how == "train":
        assert int(mod.blocks[0][1].num_batches_tracked) == 1
    if how not in ("fp32", "cout48"):     # the same module does take the kernel once the reason is gone
        mod.eval()
        mod.use_fused = True
        with torch.no_grad():
            assert mod.fusable(x.detach())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_a_transposed_convolution_with_kernel_1_is_a_1x1_convolution(dev, dtype):
    """upsample_strides 1 without use_conv_for_no_stride: ConvTranspose2d(kernel = stride = 1), its weight transposed at fold time."""
    neck = _randomise(bt.SECONDFPN([32], [64], [1]), 6).to(dev).to(dtype).eval()
    neck.use_fused = True
    x = torch.randn(2, 32, 9, 7, generator=torch.Generator().manual_seed(2)).to(dtype).to(dev)
    conv, bn = neck.deblocks[0][0], neck.deblocks[0][1]
    assert type(conv) is torch.nn.ConvTranspose2d and neck.fusable([x])
    y = neck([x])[0]
    fold = bt.fold_bev_layer(conv, bn)
    ref, mag = _ref64([x], conv.weight.detach().permute(1, 0, 2, 3), fold.scale, fold.shift, "conv", 1, 1)
    _check_inputs_are_telling(ref, fold.shift)
    assert tuple(y.shape) == (2, 64, 9, 7) and y.is_contiguous()
    assert ((y.cpu().double() - ref).abs() <= _bar(ref, mag, 32, dtype)).all()


@torch.no_grad()
def test_without_fused_stride2_the_stride_2_layer_runs_its_torch_layers_inside_the_chain(chain):
    """The stride-1 layers stay on the kernel; the result is the torch layers' for the one layer, so it is compared with the
    all-fused chain by the end-to-end bar of one more pair of roundings."""
    fuser, second, neck = chain["mods"]
    half = copy.deepcopy(second)
    half.fused_stride2 = False
    f = chain["fused"]
    assert half.fusable(f)
    s = half(f)
    assert torch.equal(s[0], chain["stages"][0])
    assert tuple(s[1].shape) == (2, 256, 6, 6) and s[1].dtype == chain["dtype"]
    top = chain["stages"][1].float().abs().max().item()
    assert (s[1].float() - chain["stages"][1].float()).abs().max().item() <= 16 * U[chain["dtype"]] * top


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@torch.no_grad()
def test_a_layer_the_kernel_does_not_serve_runs_through_torch_inside_the_fused_chain(dev, dtype):
    """SECOND with a 48-wide first stage (not served: Cout 48) and a served second stage; SECONDFPN with a strided convolution
    (upsample stride 0.5, not served) beside a served level.  The served layers bit-equal the functional form on the same input; the
    whole agrees with the torch layers within a few roundings of the storage type per layer."""
    second = _randomise(bt.SECOND(32, [48, 64], [0, 1], [1, 1]), 11).to(dev).to(dtype).eval()
    second.use_fused = True
    x = torch.randn(2, 32, 9, 7, generator=torch.Generator().manual_seed(3)).to(dtype).to(dev)
    assert bt.layer_spec(second.blocks[0][0], second.blocks[0][1]) is None and second.fusable(x)
    got = second(x)
    twin = copy.deepcopy(second)
    twin.use_fused = False
    want = twin(x)
    # the unserved stage IS its torch layers (two runs of them: the backend's call-to-call spread)
    assert (got[0].float() - want[0].float()).abs().max().item() <= _spread_bar(want[0].float(), dtype)
    y = got[0]
    for j in (0, 3):
        y = bt.bev_conv_forward([y], bt.fold_bev_layer(second.blocks[1][j], second.blocks[1][j + 1]))
    assert torch.equal(got[1], y)
    assert (got[1].float() - want[1].float()).abs().max().item() <= 16 * U[dtype] * want[1].float().abs().max().item()

    neck = _randomise(bt.SECONDFPN([32, 32], [32, 64], [0.5, 1]), 12).to(dev).to(dtype).eval()
    neck.use_fused = True
    xs = [torch.randn(2, 32, 8, 6, generator=torch.Generator().manual_seed(4)).to(dtype).to(dev),
          torch.randn(2, 32, 4, 3, generator=torch.Generator().manual_seed(5)).to(dtype).to(dev)]
    assert bt.layer_spec(neck.deblocks[0][0], neck.deblocks[0][1]) is None and neck.fusable(xs)
    out = neck(xs)[0]
    ntwin = copy.deepcopy(neck)
    ntwin.use_fused = False
    nwant = ntwin(xs)[0]
    assert tuple(out.shape) == (2, 96, 4, 3) and out.is_contiguous()
    assert (out[:, :32].float() - nwant[:, :32].float()).abs().max().item() <= _spread_bar(nwant[:, :32].float(), dtype)
    alone = bt.bev_conv_forward([xs[1]], bt.fold_bev_layer(neck.deblocks[1][0], neck.deblocks[1][1]), out_layout="nchw")
    assert torch.equal(out[:, 32:], alone)
    assert (out.float() - nwant.float()).abs().max().item() <= 8 * U[dtype] * nwant.float().abs().max().item()


def test_equal_calls_give_equal_bits_and_a_sample_ignores_its_batch(chain):
    mods, xs = chain["mods"], chain["xs"]
    with torch.no_grad():
        a = mods[2](mods[1](mods[0](xs)))[0]
        b = mods[2](mods[1](mods[0](xs)))[0]
        one = mods[2](mods[1](mods[0]([x[:1].contiguous() for x in xs])))[0]
    assert torch.equal(a, b) and torch.equal(a, chain["out"])
    assert torch.equal(a[:1], one)


def test_the_eval_forward_replays_from_a_graph_to_the_eager_bits(chain, dev):
    mods, xs = chain["mods"], chain["xs"]
    static = [x.clone() for x in xs]
    with torch.no_grad():
        eager = mods[2](mods[1](mods[0](static)))[0].clone()        # the warm-up forward: the folds exist now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = mods[2](mods[1](mods[0](static)))[0]
        for s, x in zip(static, _inputs(chain["dtype"], dev, seed=9)):
            s.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        other = mods[2](mods[1](mods[0](static)))[0]
        assert torch.equal(captured, other) and not torch.equal(other, eager)
        for s, x in zip(static, xs):
            s.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


def test_the_flagship_blocks_run_to_512_channels_on_180x180(dev):
    mods = _trunk(torch.float16, dev)
    xs = _inputs(torch.float16, dev, B=1, hw=(180, 180))
    with torch.no_grad():
        out = mods[2](mods[1](mods[0](xs)))
    assert tuple(out[0].shape) == (1, 512, 180, 180) and out[0].is_contiguous() and torch.isfinite(out[0]).all()
