"""Times the learned nets of the camera view transform (`DepthLSSTransform.get_cam_feats`) on an MI355X at the flagship sizes: 6
cameras, 256 x 704 images, a 32 x 88 feature map, in_channels 256, D = 118, C = 80, at B = 1 and B = 8.  Four routes:

  fused_fp16, fused_bf16   `cam_nets_dtype` set: the cast, the stem kernel, two `bev_conv_forward` layers, the head kernel;
  torch_fp32               `cam_nets_dtype = None`: the module's fp32 torch layers (the default, what the reference computes);
  torch_autocast_fp16      the same torch layers in channels-last under `torch.autocast(float16)`.

  whole    every route's whole `get_cam_feats` (returning the factored depth and context);
  parts    the stem, the two 3x3 layers and the head on their own.  The torch parts include what the fused parts make
           unnecessary: the `cat` in front of the 3x3 layers, and behind the 1x1 convolution the slice, the softmax and the
           channels-last copy of the context that `bev_pool` makes.

Device events around `--iters` calls after `--warmup` calls, the routes alternating inside every round; the median round is
reported with the spread.  The backend's benchmark mode is on for the torch routes.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_cam_nets.py [--iters 20] [--warmup 3] [--rounds 5] [--json profiles/cam_nets_timing.json]
"""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bev_trunk import compare, randomise  # noqa: E402

BATCHES = (1, 8)
CAMERAS, IN_CHANNELS, IMAGE, FEATURE = 6, 256, (256, 704), (32, 88)
CONFIG = dict(in_channels=IN_CHANNELS, out_channels=80, image_size=IMAGE, feature_size=FEATURE, xbound=[-54.0, 54.0, 0.3],
              ybound=[-54.0, 54.0, 0.3], zbound=[-10.0, 10.0, 20.0], dbound=[1.0, 60.0, 0.5])
STEP_SECONDS = {"whole": 420, "parts": 420}
ROUTES = ("fused_fp16", "fused_bf16", "torch_fp32", "torch_autocast_fp16")


def setup(dev):
    import torch

    from bevfusion_amd.vtransforms import DepthLSSTransform

    torch.backends.cudnn.benchmark = True
    m = DepthLSSTransform(**CONFIG)
    randomise(m, 7)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.Conv2d) and mod.bias is not None:
                mod.bias.normal_(0.0, 0.2)
    m.to(dev).eval()
    assert (m.D, m.C) == (118, 80)
    return m, copy.deepcopy(m).to(memory_format=torch.channels_last)


def inputs(B, dev):
    import torch

    g = torch.Generator().manual_seed(B)
    x = torch.randn((B, CAMERAS, IN_CHANNELS) + FEATURE, generator=g).to(dev)
    d = torch.where(torch.rand((B, CAMERAS, 1) + IMAGE, generator=g) < 0.05, 60.0 * torch.rand((B, CAMERAS, 1) + IMAGE, generator=g),
                    torch.zeros(())).to(dev)
    return x, d


def macs(B):
    n = B * CAMERAS
    oh2, ow2 = (IMAGE[0] - 1) // 4 + 1, (IMAGE[1] - 1) // 4 + 1
    fh, fw = FEATURE
    return dict(stem=n * (oh2 * ow2 * 32 * 200 + fh * fw * 64 * 800 + IMAGE[0] * IMAGE[1] * 8),
                convs=n * fh * fw * 9 * IN_CHANNELS * (IN_CHANNELS + 64 + IN_CHANNELS), head=n * fh * fw * IN_CHANNELS * (118 + 80))


def step_whole(args):
    import torch

    dev = torch.device("cuda:0")
    m, twin = setup(dev)
    out = {}
    with torch.no_grad():
        for B in BATCHES:
            x, d = inputs(B, dev)

            def fused(dtype):
                def fn():
                    m.cam_nets_dtype = dtype
                    return m.get_cam_feats(x, d)
                return fn

            def torch_fp32():
                m.cam_nets_dtype = None
                return m.get_cam_feats(x, d)

            def torch_autocast():
                with torch.autocast("cuda", dtype=torch.float16):
                    return twin.get_cam_feats(x, d)

            paths = {"fused_fp16": fused(torch.float16), "fused_bf16": fused(torch.bfloat16), "torch_fp32": torch_fp32,
                     "torch_autocast_fp16": torch_autocast}
            m.cam_nets_dtype = torch.float16
            assert m.cam_nets_fusable(x, d)
            ref = torch_fp32()
            diff = {}
            for k in ROUTES:
                r = paths[k]()
                diff[k] = dict(depth=float((r.depth.float() - ref.depth).abs().max()) / float(ref.depth.abs().max()),
                               context=float((r.ctx.float() - ref.ctx).abs().max()) / float(ref.ctx.abs().max()))
                assert diff[k]["depth"] < 0.5 and diff[k]["context"] < 0.1, (k, diff[k])      # the routes compute the same nets
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            out[f"B{B}"] = dict(ms=med, spread=spread, mac=sum(macs(B).values()), max_diff_to_torch_fp32=diff)
    return out


def step_parts(args):
    import torch

    from bevfusion_amd import bev_trunk as bt, cam_nets as cn

    dev = torch.device("cuda:0")
    m, twin = setup(dev)
    D = m.D
    out = {}
    with torch.no_grad():
        for B in BATCHES:
            x, d = inputs(B, dev)
            n = B * CAMERAS
            x4, d4, d3 = x.view((n, IN_CHANNELS) + FEATURE), d.view((n, 1) + IMAGE), d.view((n,) + IMAGE)
            res = {}
            # the stem
            stem = {f"fused_{k}": (lambda f=cn.fold_depth_stem(m.dtransform, t): cn.depth_stem_forward(d3, f))
                    for k, t in (("fp16", torch.float16), ("bf16", torch.bfloat16))}
            stem["torch_fp32"] = lambda: m.dtransform(d4)

            def stem_autocast():
                with torch.autocast("cuda", dtype=torch.float16):
                    return twin.dtransform(d4)
            stem["torch_autocast_fp16"] = stem_autocast
            # the two 3x3 layers
            ds32 = m.dtransform(d4)
            convs = {}
            for k, t in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
                f1, f2 = cn.fold_conv_bias_bn(m.depthnet[0], m.depthnet[1], t), cn.fold_conv_bias_bn(m.depthnet[3], m.depthnet[4], t)
                dh, xh = ds32.to(dtype=t, memory_format=torch.channels_last), x4.to(dtype=t, memory_format=torch.channels_last)
                convs[f"fused_{k}"] = lambda f1=f1, f2=f2, dh=dh, xh=xh: bt.bev_conv_forward([bt.bev_conv_forward([dh, xh], f1)], f2)
            convs["torch_fp32"] = lambda: m.depthnet[:6](torch.cat([ds32, x4], dim=1))
            ds_cl, x_cl = ds32.contiguous(memory_format=torch.channels_last), x4.contiguous(memory_format=torch.channels_last)

            def convs_autocast():
                with torch.autocast("cuda", dtype=torch.float16):
                    return twin.depthnet[:6](torch.cat([ds_cl, x_cl], dim=1))
            convs["torch_autocast_fp16"] = convs_autocast
            # the head
            y32 = convs["torch_fp32"]()
            head = {}
            for k, t in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
                f, yh = cn.fold_depth_head(m.depthnet[6], m.D, m.C, t), y32.to(dtype=t, memory_format=torch.channels_last)
                head[f"fused_{k}"] = lambda f=f, yh=yh: cn.depth_head_forward(yh, f)

            def head_torch(net, y):
                z = net.depthnet[6](y)
                return z[:, :D].softmax(dim=1), z[:, D:].float().permute(0, 2, 3, 1).contiguous()
            head["torch_fp32"] = lambda: head_torch(m, y32)
            y_cl = y32.contiguous(memory_format=torch.channels_last)

            def head_autocast():
                with torch.autocast("cuda", dtype=torch.float16):
                    return head_torch(twin, y_cl)
            head["torch_autocast_fp16"] = head_autocast
            mac = macs(B)
            for name, paths in (("stem", stem), ("convs", convs), ("head", head)):
                med, spread = compare(paths, args.iters, args.warmup, args.rounds)
                res[name] = dict(ms=med, spread=spread, mac=mac[name])
            out[f"B{B}"] = res
    return out


STEPS = {"whole": step_whole, "parts": step_parts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_cam_nets needs a GPU: nothing is measured without one")
        print("RESULT " + json.dumps(STEPS[args.step](args)), flush=True)
        return
    results = {}
    for step, seconds in STEP_SECONDS.items():
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"step {step} ended with status {r.returncode}: nothing further is started")
        results[step] = json.loads(lines[-1][len("RESULT "):])
        print(f"{step}: {lines[-1][len('RESULT '):]}", file=sys.stderr, flush=True)
    line = json.dumps(results)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
