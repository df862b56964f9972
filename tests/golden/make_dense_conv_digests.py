"""Records sha256 digests of what the dense 16-bit convolution kernels (csrc/ext/dense_tile.h and the six units over it) write, so
that a change of their text that is meant to leave every bit alone can be held to that (tests/test_gpu_dense_conv_digests.py):

    python tests/golden/make_dense_conv_digests.py            # on an MI355X, in a checkout of the commit to record FROM

Run it in a built checkout of the commit whose bits are to be kept, never in the tree under test, and copy the JSON over.  A change
that moves a summation order on purpose re-records with this same recorder and says so.

Only the public functionals are used.  Inputs, weights and BatchNorm statistics come from a seeded CPU generator, are rounded to
the storage dtype and folded on the CPU, then moved to the device; a digest is over the output's bytes in logical NCHW order.
The cases reach every (dtype, channel tile, kernel, stride, downsample / resample) instantiation the launch code can choose, on
maps with two partial tiles each way and 48 input channels (one full chunk and a half one), and every family crosses both source
and both destination layouts.
"""
import dataclasses
import hashlib
import json
import os
import sys

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from bevfusion_amd import bev_resnet, bev_trunk, cam_neck, cam_nets, cam_resnet  # noqa: E402

OUT = os.path.join(HERE, "dense_conv_digests.json")
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
B, OH, OW, CIN = 2, 9, 17, 48            # two 8 x 16 tiles each way, both edge tiles partial; a full chunk of 32 channels and a half
WIDE = 64                                # cam_neck takes the channel tiles 64 and 128 only from NK_FILL = 256 workgroups: 4 tiles x 64
COUTS = (32, 64, 128)                    # channel tiles of 32 (MT 1), 64 (MT 2), 128 (MT 4)
LAYOUTS = ("nchw", "nhwc")


def _gen(name):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))


def _tensor(g, shape, dtype, layout="nchw", scale=1.0):
    t = (torch.randn(shape, generator=g) * scale).to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t


def _fill(module, g, dtype):
    """Weights ~ N(0, 1 / fan_in), BatchNorm weight and variance in [0.5, 1.5), bias and mean ~ N(0, 0.1), all rounded to dtype."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                fan = m.weight[0].numel() if isinstance(m, nn.Conv2d) else m.weight.shape[0] * m.weight[0, 0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * fan ** -0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return module.to(dtype).eval()


def _to(fold, dev):
    return dataclasses.replace(fold, **{f.name: getattr(fold, f.name).to(dev) for f in dataclasses.fields(fold)
                                        if torch.is_tensor(getattr(fold, f.name))})


def digest(t):
    """sha256 of a tensor's bytes in logical (NCHW for a 4-d view) order."""
    t = t.detach().contiguous().cpu()
    raw = t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def _pick(i, n=2):
    """n layouts and a flag for case i, from a hash of i so that they do not move in step with the loops that number the cases."""
    bits = hashlib.sha256(b"layouts %d" % i).digest()[0]
    return tuple(LAYOUTS[(bits >> k) & 1] for k in range(n)), bool((bits >> n) & 1)


# ---- the cases: name -> function(dev) -> {suffix: tensor} ----------------------------------------------------------------------
def _bev_conv(name, dtype, cout, mode, kernel, stride, lay, split=None, window=False):
    def run(dev):
        g = _gen(name)
        if mode == "deconv":
            conv = nn.ConvTranspose2d(CIN, cout, 2, stride=2, bias=False)
        else:
            conv = nn.Conv2d(CIN, cout, kernel, stride=stride, padding=kernel // 2, bias=False)
        bn = _fill(nn.BatchNorm2d(cout), g, dtype)
        fold = _to(bev_trunk.fold_bev_layer(_fill(conv, g, dtype), bn), dev)
        hw = (2 * OH - 1, 2 * OW - 1) if stride == 2 and mode == "conv" else (OH, OW)
        srcs = [_tensor(g, (B, c) + hw, dtype, lay[0]).to(dev) for c in (split or (CIN,))]
        if not window:
            return {"": bev_trunk.bev_conv_forward(srcs, fold, out_layout=lay[1])}
        out = torch.zeros((B, OH, OW, cout + 8), dtype=dtype, device=dev).permute(0, 3, 1, 2)      # NHWC, the window at offset 4
        bev_trunk.bev_conv_forward(srcs, fold, out=out, out_channel_offset=4)
        return {"": out}
    return run


def _res_block(name, dtype, C, residual, stride, lay):
    def run(dev):
        g = _gen(name)
        cx = C if residual == "identity" else CIN
        down = None if residual == "identity" else nn.Sequential(nn.Conv2d(cx, C, 1, stride=stride, bias=False), nn.BatchNorm2d(C))
        fold = _to(bev_resnet.fold_res_block(_fill(bev_resnet.BasicBlock(cx, C, stride=stride, downsample=down), g, dtype)), dev)
        xhw = (2 * OH - 1, 2 * OW - 1) if stride == 2 else (OH, OW)
        h = _tensor(g, (B, C, OH, OW), dtype, lay[0]).to(dev)
        x = _tensor(g, (B, cx) + xhw, dtype, lay[1]).to(dev)
        return {"": bev_resnet.res_block_forward(h, x, fold, out_layout=lay[2])}
    return run


def _bottleneck(name, dtype, C, residual, stride, lay):
    def run(dev):
        g = _gen(name)
        cx = C if residual == "identity" else CIN
        down = None if residual == "identity" else nn.Sequential(nn.Conv2d(cx, C, 1, stride=stride, bias=False), nn.BatchNorm2d(C))
        block = cam_resnet.Bottleneck(cx, CIN, stride=stride, downsample=down)                       # P = 48 planes
        block.conv3, block.bn3 = nn.Conv2d(CIN, C, 1, bias=False), nn.BatchNorm2d(C)                 # C need not be 4 P for the tail
        fold = _to(cam_resnet.fold_bottleneck(_fill(block, g, dtype)), dev)
        xhw = (2 * OH - 1, 2 * OW - 1) if stride == 2 else (OH, OW)
        h = _tensor(g, (B, CIN, OH, OW), dtype, lay[0]).to(dev)                                      # 306 flat pixels: 128 + 128 + 50
        x = _tensor(g, (B, cx) + xhw, dtype, lay[1]).to(dev)
        return {"": cam_resnet.bottleneck_tail_forward(h, x, fold, out_layout=lay[2])}
    return run


def _cam_neck(name, dtype, cout, batch, kernel, resample, relu, lay):
    def run(dev):
        g = _gen(name)
        conv = nn.Conv2d(CIN, cout, kernel, padding=kernel // 2, bias=False)
        fold = _to(cam_neck.fold_neck_layer(_fill(conv, g, dtype), _fill(nn.BatchNorm2d(cout), g, dtype)), dev)
        s0 = _tensor(g, (batch, 32, OH, OW), dtype, lay[0]).to(dev)                                  # on the output map: copied
        s1 = _tensor(g, (batch, 16) + ((5, 9) if resample else (OH, OW)), dtype, lay[1]).to(dev)     # 5 x 9: resampled
        return {"": cam_neck.cam_neck_conv_forward([s0, s1], fold, out_size=(OH, OW), relu=relu, out_layout=lay[2])}
    return run


def _depth_stem(name, dtype):
    def run(dev):
        g = _gen(name)
        stem = nn.Sequential(nn.Conv2d(1, 8, 1), nn.BatchNorm2d(8), nn.ReLU(True), nn.Conv2d(8, 32, 5, stride=4, padding=2),
                             nn.BatchNorm2d(32), nn.ReLU(True), nn.Conv2d(32, 64, 5, stride=2, padding=2), nn.BatchNorm2d(64),
                             nn.ReLU(True))
        fold = _to(cam_nets.fold_depth_stem(_fill(stem, g, torch.float32), dtype), dev)
        H, W = 4 * (2 * OH - 2) + 1, 4 * (2 * OW - 2) + 1       # 65 x 129: the smallest raster whose layer-3 map is 9 x 17
        assert cam_nets.stem_output_size(H, W) == (OH, OW) and cam_nets.stem_output_size(H - 1, W - 1) != (OH, OW)
        depth = (torch.rand((B, H, W), generator=g) * 60.0).to(dev)
        mid = torch.zeros((B, (H - 1) // 4 + 1, (W - 1) // 4 + 1, 32), dtype=dtype, device=dev)
        return {"/mid": mid, "": cam_nets.depth_stem_forward(depth, fold, scratch=mid)}
    return run


def _depth_head(name, dtype, cin, D, C):
    def run(dev):
        g = _gen(name)
        assert cam_nets.head_served(cin, D, C) and (B * OH * OW) % 32                                # CN_HEAD_PIX = 32
        fold = _to(cam_nets.fold_depth_head(_fill(nn.Conv2d(cin, D + C, 1), g, torch.float32), D, C, dtype), dev)
        depth, ctx = cam_nets.depth_head_forward(_tensor(g, (B, cin, OH, OW), dtype, "nhwc").to(dev), fold)
        return {"/depth": depth, "/ctx": ctx}
    return run


def _stem(name, dtype, lay):
    def run(dev):
        g = _gen(name)
        conv, bn, pool = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.MaxPool2d(3, stride=2, padding=1)
        assert cam_resnet.stem_spec(conv, bn.eval(), pool) == (7, 2, 3)
        fold = _to(cam_resnet.fold_stem(_fill(conv, g, dtype), _fill(bn, g, dtype), pool), dev)
        x = _tensor(g, (B, 3, 18, 62), dtype).to(dev)           # conv map 9 x 31, pooled 5 x 16: two 4 x 15 tiles each way, partial
        return {"": cam_resnet.stem_forward(x, fold, out_layout=lay)}
    return run


def cases():
    out, i = {}, 0

    def add(name, make, *args, **kw):
        out[name] = make(name, *args, **kw)
    for dn, dt in DTYPES.items():
        for cout in COUTS:
            for mn, (mode, k, s) in (("k3s1", ("conv", 3, 1)), ("k3s2", ("conv", 3, 2)), ("k1", ("conv", 1, 1))):
                lay, _ = _pick(i)
                i += 1
                add(f"bev_conv/{dn}/c{cout}/{mn}/{lay[0]}-{lay[1]}", _bev_conv, dt, cout, mode, k, s, lay)
        add(f"bev_conv/{dn}/c64/deconv/nhwc-nchw", _bev_conv, dt, 64, "deconv", 2, 2, ("nhwc", "nchw"))
        add(f"bev_conv/{dn}/c64/k3s1/two-sources/nchw-nhwc", _bev_conv, dt, 64, "conv", 3, 1, ("nchw", "nhwc"), split=(32, 16))
        add(f"bev_conv/{dn}/c32/k3s1/window/nhwc-nhwc", _bev_conv, dt, 32, "conv", 3, 1, ("nhwc", "nhwc"), window=True)
        for fam, make in (("res_block", _res_block), ("bottleneck", _bottleneck)):
            for C in COUTS:
                for rn, (res, s) in (("identity", ("identity", 1)), ("down1", ("downsample", 1)), ("down2", ("downsample", 2))):
                    lay, _ = _pick(i, 3)
                    i += 1
                    add(f"{fam}/{dn}/c{C}/{rn}/{'-'.join(lay)}", make, dt, C, res, s, lay)
        for cout, batch in ((32, B), (64, WIDE), (128, WIDE)):
            for k in (1, 3):
                for rs in (False, True):
                    lay, relu = _pick(i, 3)
                    i += 1
                    add(f"cam_neck/{dn}/c{cout}/k{k}/{'resampled' if rs else 'copied'}/{'relu' if relu else 'linear'}/{'-'.join(lay)}",
                        _cam_neck, dt, cout, batch, k, rs, relu, lay)
        add(f"depth_stem/{dn}", _depth_stem, dt)
        for D in (1, 61, 125):                      # D + 4 rows: 1, 5 and 9 tiles of 16, the head kernels built for 4, 8 and 16
            add(f"depth_head/{dn}/in32/d{D}/c4", _depth_head, dt, 32, D, 4)
        for lay in LAYOUTS:
            add(f"resnet_stem/{dn}/{lay}", _stem, dt, lay)
    for fam in ("bev_conv", "res_block", "bottleneck", "cam_neck"):       # each family crosses both layouts on either side
        lays = [n.split("/")[-1].split("-") for n in out if n.startswith(fam)]
        assert all({l[k] for l in lays} == set(LAYOUTS) for k in (0, -1)), fam
    return out


def record(dev):
    rec = {}
    with torch.no_grad():
        for name, run in cases().items():
            for suffix, t in run(dev).items():
                assert t is not None, f"{name}: the kernel does not serve the case"
                rec[name + suffix] = digest(t)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available(), "the digests are recorded on the device"
    rec = record(torch.device("cuda:0"))
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(rec)} digests")
