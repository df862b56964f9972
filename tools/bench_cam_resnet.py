"""Times the camera ResNet-50's eval-mode forward on an MI355X on 256 x 704 images, at N = 6 (one frame's cameras), in fp16:

  parts    the stem and one Bottleneck of every class at every stage's real widths and maps (64 x 176, 32 x 88, 16 x 44, 8 x 22):
           "fused_all" (the stem through `bevamd_resnet_stem_forward`; conv1 and conv2 through `bevamd_bev_conv_forward`, the tail
           through `bevamd_bottleneck_tail_forward`: three launches), "tail_torch" (`fused_tails = ()`: the two convolutions through
           the kernel, the tail through its torch layers), and the part's own torch layers in contiguous NCHW and in channels-last
           with the backend's benchmark mode on; the faster of the two torch formats is the comparison.
  nets     the whole ResNet-50 at N = 1 and N = 6: "fused" is the module's default choice of classes (`fused_stem`, `fused_stride2`,
           `fused_tails`), "fused_all" every part through a kernel, and the two torch formats.

Device events around `--iters` calls after `--warmup` calls, the paths alternating inside every round; the median round is reported
with the spread.  The MFMA floor 2 * MAC / 2.5 PFLOP/s is printed beside the times.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_cam_resnet.py [--iters 20] [--warmup 3] [--rounds 5] [--json profiles/cam_resnet_timing.json]
"""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bev_trunk import PEAK_FP16_MATRIX, compare, randomise  # noqa: E402

IMAGE, CAMERAS = (256, 704), 6
STEP_SECONDS = {"parts": 500, "nets": 500}
ALL_TAILS = ("identity", "down1", "down2")
# name -> (stage, block, map of the block's input)
BLOCKS = {"down1_64_256": (1, 0, (64, 176)), "identity_256": (1, 1, (64, 176)), "down2_256_512": (2, 0, (64, 176)),
          "identity_512": (2, 1, (32, 88)), "down2_512_1024": (3, 0, (32, 88)), "identity_1024": (3, 1, (16, 44)),
          "down2_1024_2048": (4, 0, (16, 44)), "identity_2048": (4, 1, (8, 22))}


def set_mode(net, mode, defaults):
    """mode: "default" (the module's own switches), "all", "tail_torch", "torch"."""
    net.use_fused = mode != "torch"
    if mode == "default":
        net.fused_stem, net.fused_stride2, net.fused_tails = defaults
    elif mode == "all":
        net.fused_stem, net.fused_stride2, net.fused_tails = True, True, ALL_TAILS
    elif mode == "tail_torch":
        net.fused_stem, net.fused_stride2, net.fused_tails = True, True, ()


def last(y):
    while isinstance(y, (list, tuple)):
        y = y[-1]
    return y


def conv_macs(module, fn):
    import torch

    total = 0

    def hook(m, args, out):
        nonlocal total
        total += out.shape[0] * out.shape[2] * out.shape[3] * m.in_channels * m.out_channels * m.kernel_size[0] * m.kernel_size[1]
    hooks = [m.register_forward_hook(hook) for m in module.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        fn()
    for h in hooks:
        h.remove()
    return total


def prepare(dev):
    import torch

    from bevfusion_amd import cam_resnet as cr

    torch.backends.cudnn.benchmark = True
    net = randomise(cr.ResNet(depth=50), 7).to(dev).half().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net, copy.deepcopy(net).to(memory_format=torch.channels_last), (net.fused_stem, net.fused_stride2, net.fused_tails)


def report(paths, args, mac):
    ref = last(paths["torch_nchw"]()).float()
    errs = {k: float((last(fn()).float() - ref).abs().max()) / float(ref.abs().max()) for k, fn in paths.items()}
    assert max(errs.values()) < 2e-2, errs              # every path computes the same layers (fp16 storage)
    med, spread = compare(paths, args.iters, args.warmup, args.rounds)
    best = min(med["torch_nchw"], med["torch_nhwc"])
    return dict(ms=med, spread=spread, mac=mac, floor_ms=2 * mac / PEAK_FP16_MATRIX * 1e3, torch_best_ms=best,
                speedup={k: best / v for k, v in med.items() if not k.startswith("torch")}, max_rel_diff=errs)


def step_parts(args):
    import torch

    from bevfusion_amd.bev_trunk import _as_source

    dev = torch.device("cuda:0")
    net, twin, defaults = prepare(dev)
    out = {}
    with torch.no_grad():
        x_n = torch.randn((CAMERAS, 3) + IMAGE, generator=torch.Generator().manual_seed(3)).half().to(dev)
        x_c = x_n.contiguous(memory_format=torch.channels_last)

        def torch_stem(m, x):
            return lambda: m.maxpool(m.relu(m.bn1(m.conv1(x))))

        def fused_stem():
            set_mode(net, "all", defaults)
            return net._fused_stem(x_n)
        paths = {"torch_nchw": torch_stem(net, x_n), "torch_nhwc": torch_stem(twin, x_c), "fused_all": fused_stem}
        out["stem"] = report(paths, args, conv_macs(net.conv1, paths["torch_nchw"]))
        print(f"stem: {json.dumps(out['stem'])}", file=sys.stderr, flush=True)
        for i, (name, (stage, j, size)) in enumerate(BLOCKS.items()):
            blk, tblk = getattr(net, f"layer{stage}")[j], getattr(twin, f"layer{stage}")[j]
            b_n = torch.randn((CAMERAS, blk.conv1.in_channels) + size, generator=torch.Generator().manual_seed(10 + i)).half().to(dev)
            b_c = b_n.contiguous(memory_format=torch.channels_last)

            def fused(mode, blk=blk, x=b_c):
                def fn():
                    set_mode(net, mode, defaults)
                    return net._fused_block(blk, _as_source(x))
                return fn
            paths = {"torch_nchw": lambda blk=blk, x=b_n: blk(x), "torch_nhwc": lambda blk=tblk, x=b_c: blk(x),
                     "fused_all": fused("all"), "tail_torch": fused("tail_torch")}
            out[name] = report(paths, args, conv_macs(blk, paths["torch_nchw"]))
            print(f"{name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    return out


def step_nets(args):
    import torch

    dev = torch.device("cuda:0")
    net, twin, defaults = prepare(dev)
    out = {}
    with torch.no_grad():
        for N in (1, CAMERAS):
            x_n = torch.randn((N, 3) + IMAGE, generator=torch.Generator().manual_seed(30 + N)).half().to(dev)
            x_c = x_n.contiguous(memory_format=torch.channels_last)

            def path(mode, m=net, x=x_n):
                def fn():
                    set_mode(m, mode, defaults)
                    return m(x)
                return fn
            paths = {"torch_nchw": path("torch"), "torch_nhwc": path("torch", twin, x_c), "fused_all": path("all"), "fused": path("default")}
            set_mode(net, "all", defaults)
            assert net.fusable(x_n)
            out[f"N{N}"] = report(paths, args, conv_macs(net, paths["torch_nchw"]))
            set_mode(net, "default", defaults)
            print(f"N{N}: {json.dumps(out[f'N{N}'])}", file=sys.stderr, flush=True)
    return out


STEPS = {"parts": step_parts, "nets": step_nets}


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
            raise SystemExit("bench_cam_resnet needs a GPU: nothing is measured without one")
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
