"""Times GeneralizedResNet's eval-mode forward on an MI355X on a 128 x 128 BEV map, at B = 1 and B = 8, in fp16:

  blocks   one BasicBlock of every class at the recorded leaf's widths (64 -> 128 / 256 / 512) and at lssfpn/default.yaml's (336 ->
           160 / 320 / 640): identity, downsample stride 1, downsample stride 2.  Paths: "fused_all" (conv1 through
           `bevamd_bev_conv_forward`, the tail through `bevamd_res_block_forward`: two launches), "tail_only" (`fused_stride2 = False`: a
           stride-2 conv1 + bn1 + ReLU through torch, the tail through the kernel; a stride-1 block is "fused_all" again),
           "head_only" (conv1 through the kernel, the tail through torch), and the block's own torch layers with
           `use_fused = False` in contiguous NCHW and in channels-last with the backend's benchmark mode on; the faster of the two
           torch formats is the comparison.
  nets     the recorded leaf (64 -> 128 / 256 / 512), the lssfpn widths (336 -> 160 / 320 / 640) and the whole decoder
           (GeneralizedResNet + LSSFPN of the recorded leaf): "fused" is the module's default choice of classes (`fused_stride2`,
           `fused_tails`), "fused_all" every half through a kernel, and the two torch formats.

Device events around `--iters` calls after `--warmup` calls, the paths alternating inside every round; the median round is reported
with the spread.  The MFMA floor 2 * MAC / 2.5 PFLOP/s is printed beside the times.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_bev_resnet.py [--iters 20] [--warmup 3] [--rounds 5] [--json profiles/bev_resnet_timing.json]
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

MAP, BATCHES = 128, (1, 8)
STEP_SECONDS = {"blocks": 500, "nets": 500}
ALL_TAILS = ("identity", "down1", "down2")
RECORDED = [[2, 128, 2], [2, 256, 2], [2, 512, 1]]
LSSFPN_WIDTHS = [[2, 160, 2], [2, 320, 2], [2, 640, 1]]
# name -> (in_channels, planes, stride, map of the block's input)
BLOCKS = {
    "down2_64_128": (64, 128, 2, MAP), "identity_128": (128, 128, 1, MAP // 2), "down2_128_256": (128, 256, 2, MAP // 2),
    "identity_256": (256, 256, 1, MAP // 4), "down1_256_512": (256, 512, 1, MAP // 4), "identity_512": (512, 512, 1, MAP // 4),
    "down2_336_160": (336, 160, 2, MAP), "identity_160": (160, 160, 1, MAP // 2), "down1_320_640": (320, 640, 1, MAP // 4),
    "identity_640": (640, 640, 1, MAP // 4),
}


def set_mode(mods, mode, defaults):
    """mode: "default" (the module's own switches), "all", "tail_only", "head_only", "torch"."""
    for m, d in zip(mods, defaults):
        m.use_fused = mode != "torch"
        if d is None:
            continue
        if mode == "default":
            m.fused_stride2, m.fused_tails = d
        elif mode == "all":
            m.fused_stride2, m.fused_tails = True, ALL_TAILS
        elif mode == "tail_only":
            m.fused_stride2, m.fused_tails = False, ALL_TAILS
        elif mode == "head_only":
            m.fused_stride2, m.fused_tails = True, ()


def run(mods, x):
    for m in mods:
        x = m(x)
    return x


def last(y):
    while isinstance(y, (list, tuple)):
        y = y[-1]
    return y


def macs(mods, x):
    import torch

    total = 0

    def hook(m, args, out):
        nonlocal total
        total += out.shape[0] * out.shape[2] * out.shape[3] * m.in_channels * m.out_channels * m.kernel_size[0] * m.kernel_size[1]
    hooks = [m.register_forward_hook(hook) for m in mods.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        run(mods, x)
    for h in hooks:
        h.remove()
    return total


def measure(mods, make, args, dev, per_class):
    import torch

    defaults = [(m.fused_stride2, m.fused_tails) if hasattr(m, "fused_tails") else None for m in mods]
    torch.backends.cudnn.benchmark = True
    randomise(mods, 7)
    mods.to(dev).half().eval()
    for p in mods.parameters():
        p.requires_grad_(False)
    twin = copy.deepcopy(mods).to(memory_format=torch.channels_last)
    out = {}
    with torch.no_grad():
        for B in BATCHES:
            x_n = make(B)
            x_c = x_n.contiguous(memory_format=torch.channels_last)

            def path(mode, m=mods, x=x_n):
                def fn():
                    set_mode(m, mode, defaults)
                    return run(m, x)
                return fn
            paths = {"torch_nchw": path("torch"), "torch_nhwc": path("torch", twin, x_c), "fused_all": path("all")}
            if per_class:
                paths["tail_only"], paths["head_only"] = path("tail_only"), path("head_only")
            else:
                paths["fused"] = path("default")
            set_mode(mods, "all", defaults)
            assert mods[0].fusable(x_n)
            ref = last(paths["torch_nchw"]()).float()
            errs = {k: float((last(fn()).float() - ref).abs().max()) / float(ref.abs().max()) for k, fn in paths.items()}
            assert max(errs.values()) < 2e-2, errs              # every path computes the same layers (fp16 storage)
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            set_mode(mods, "torch", defaults)
            mac = macs(mods, x_n)
            best = min(med["torch_nchw"], med["torch_nhwc"])
            out[f"B{B}"] = dict(ms=med, spread=spread, mac=mac, floor_ms=2 * mac / PEAK_FP16_MATRIX * 1e3, torch_best_ms=best,
                                speedup={k: best / v for k, v in med.items() if not k.startswith("torch")}, max_rel_diff=errs)
            set_mode(mods, "default", defaults)
    return out


def inputs(dev, channels, size, seed):
    import torch

    def make(B):
        return torch.randn((B, channels, size, size), generator=torch.Generator().manual_seed(seed + B)).half().to(dev)
    return make


def step_blocks(args):
    import torch
    from torch import nn

    from bevfusion_amd import bev_resnet as br

    dev = torch.device("cuda:0")
    out = {}
    for i, (name, (cin, planes, stride, size)) in enumerate(BLOCKS.items()):
        mods = nn.ModuleList([br.GeneralizedResNet(cin, [[1, planes, stride]])])
        out[name] = measure(mods, inputs(dev, cin, size, 10 + i), args, dev, per_class=True)
        print(f"{name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    return out


def step_nets(args):
    import torch
    from torch import nn

    from bevfusion_amd import bev_resnet as br, cam_neck as cnk

    dev = torch.device("cuda:0")
    nets = {
        "recorded_64": (nn.ModuleList([br.GeneralizedResNet(64, RECORDED)]), 64),
        "lssfpn_336": (nn.ModuleList([br.GeneralizedResNet(336, LSSFPN_WIDTHS)]), 336),
        "decoder_64": (nn.ModuleList([br.GeneralizedResNet(64, RECORDED), cnk.LSSFPN([-1, 0], [512, 128], 256, scale_factor=2)]), 64),
    }
    out = {}
    for i, (name, (mods, cin)) in enumerate(nets.items()):
        out[name] = measure(mods, inputs(dev, cin, MAP, 30 + i), args, dev, per_class=False)
        print(f"{name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    return out


STEPS = {"blocks": step_blocks, "nets": step_nets}


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
            raise SystemExit("bench_bev_resnet needs a GPU: nothing is measured without one")
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
